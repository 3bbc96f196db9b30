// TriDiagKernels.hip -- the array form of the batched tridiagonal solvers (TriDiagSolvers.h) on gfx950.
//
// PCR: lanes along the rows.  A workgroup holds floor(256 / NRow) systems side by side (one for NRow > 256, up to 1024
// lanes), so a system's row of each array is one coalesced run of loads; each lane keeps its row's coefficients in
// registers and exchanges them through a double-buffered LDS workspace (kernels/TriDiagKernels.h: pcrSolveRow), one
// barrier per level.  Thomas: one lane per column, the eliminated diagonal in LDS ([row][lane], so the lanes of a
// wave read consecutive doubles), X used in place as the reference's scratch X; correctness is what it is for.
#include "TriDiagKernels.h"

namespace OMEGA {

namespace {

constexpr int PcrLanes    = 256;  // lanes a workgroup of short systems fills
constexpr int ThomasBytes = 32768; // LDS of one Thomas workgroup (eliminated diagonal of its columns)

/// Systems per PCR workgroup and the lanes they occupy
struct PcrShape {
   int Sys, Rows, Threads;
   explicit PcrShape(int NRow) {
      Sys     = NRow <= PcrLanes ? PcrLanes / NRow : 1;
      Rows    = Sys * NRow;
      Threads = (Rows + 63) / 64 * 64;
   }
};

template <bool Diffusion>
__global__ void __launch_bounds__(TriDiagMaxRows) pcrKernel(TriDiagArgs A, int SysPerBlock, int Rows) {
   extern __shared__ Real Lds[];
   const int T    = threadIdx.x;
   const int S    = T / A.NRow;
   const int K    = T - S * A.NRow;
   const long I   = (long)blockIdx.x * SysPerBlock + S;
   const bool Act = T < Rows && I < A.NBatch;
   Real *Sys      = Lds + S * A.NRow;
   if (Diffusion) {
      Real G = 0, H = 0, X = 0;
      if (Act) {
         G = A.A[I * A.PitchA + K];
         H = A.B[I * A.PitchB + K];
         X = A.X[I * A.PitchX + K];
      }
      X = pcrDiffSolveRow(Act, K, A.NRow, G, H, X, Sys, Rows);
      if (Act)
         A.X[I * A.PitchX + K] = X;
   } else {
      Real DL = 0, D = 0, DU = 0, X = 0;
      if (Act) {
         DL = A.A[I * A.PitchA + K];
         D  = A.B[I * A.PitchB + K];
         DU = A.C[I * A.PitchC + K];
         X  = A.X[I * A.PitchX + K];
      }
      X = pcrSolveRow(Act, K, A.NRow, DL, D, DU, X, Sys, Rows);
      if (Act)
         A.X[I * A.PitchX + K] = X;
   }
}

template <bool Diffusion> __global__ void __launch_bounds__(64) thomasKernel(TriDiagArgs A, int Cols) {
   extern __shared__ Real Lds[];
   const long I = (long)blockIdx.x * Cols + threadIdx.x;
   if (I >= A.NBatch)
      return;
   Real *X = A.X + I * A.PitchX;
   if (Diffusion)
      thomasDiffSolveColumn(A.NRow, A.A + I * A.PitchA, A.B + I * A.PitchB, 1, X, 1, Lds + threadIdx.x, Cols);
   else
      thomasSolveColumn(A.NRow, A.A + I * A.PitchA, A.B + I * A.PitchB, A.C + I * A.PitchC, 1, X, 1,
                        Lds + threadIdx.x, Cols);
}

} // namespace

void launchTriDiag(TriDiagAlgo Algo, const TriDiagArgs &A, hipStream_t Str) {
   OMEGA_REQUIRE(A.NRow >= 1 && A.NRow <= TriDiagMaxRows,
                 "TriDiagSolver: NRow = " + std::to_string(A.NRow) + " is outside the supported 1 <= NRow <= " +
                     std::to_string(TriDiagMaxRows));
   if (A.NBatch <= 0)
      return;
   const bool Diff = Algo == TriDiagAlgo::ThomasDiffusion || Algo == TriDiagAlgo::PCRDiffusion;
   if (Algo == TriDiagAlgo::PCR || Algo == TriDiagAlgo::PCRDiffusion) {
      const PcrShape P(A.NRow);
      const dim3 Grid((A.NBatch + P.Sys - 1) / P.Sys);
      const size_t Bytes = (size_t)2 * (Diff ? 3 : 4) * P.Rows * sizeof(Real);
      if (Diff)
         hipLaunchKernelGGL(pcrKernel<true>, Grid, dim3(P.Threads), Bytes, Str, A, P.Sys, P.Rows);
      else
         hipLaunchKernelGGL(pcrKernel<false>, Grid, dim3(P.Threads), Bytes, Str, A, P.Sys, P.Rows);
   } else {
      int Cols = ThomasBytes / (int)sizeof(Real) / A.NRow;
      Cols     = Cols > 64 ? 64 : Cols;
      const dim3 Grid((A.NBatch + Cols - 1) / Cols);
      const size_t Bytes = (size_t)Cols * A.NRow * sizeof(Real);
      if (Diff)
         hipLaunchKernelGGL(thomasKernel<true>, Grid, dim3(Cols), Bytes, Str, A, Cols);
      else
         hipLaunchKernelGGL(thomasKernel<false>, Grid, dim3(Cols), Bytes, Str, A, Cols);
   }
   HIP_CHECK(hipGetLastError());
}

} // namespace OMEGA
