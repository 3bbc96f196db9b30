// TriDiagKernels.hip -- the array form of the batched tridiagonal solvers (TriDiagSolvers.h) on gfx950.
//
// PCR: lanes along the rows, in the packed-column shape (kernels/PackedColumns.h): a system's row of each array is one
// coalesced run of loads; each lane keeps its row's coefficients in registers and exchanges them through a
// double-buffered LDS workspace (kernels/TriDiagKernels.h: pcrSolveRow, pcrDiffSolveRowRagged), one barrier per level.  Thomas: one lane per column, the eliminated diagonal in LDS ([row][lane], so the lanes of a
// wave read consecutive doubles), X used in place as the reference's scratch X; correctness is what it is for.
#include "PackedColumns.h"

namespace OMEGA {

namespace {

constexpr int ThomasBytes = 32768; // LDS of one Thomas workgroup (eliminated diagonal of its columns)

template <bool Diffusion> __global__ void __launch_bounds__(TriDiagMaxRows) pcrKernel(TriDiagArgs A, PackedShape P) {
   extern __shared__ Real Lds[];
   const PackedLane L = packedLane(P, A.NRow, A.NBatch);
   const int K        = L.I;   // row K
   const long I       = L.Col; // of system I
   const bool Act     = L.InSys;
   Real *Sys          = Lds + L.S * A.NRow;
   if (Diffusion) {
      Real G = 0, H = 0, X = 0;
      if (Act) {
         G = A.A[I * A.PitchA + K];
         H = A.B[I * A.PitchB + K];
         X = A.X[I * A.PitchX + K];
      }
      X = pcrDiffSolveRowRagged(Act, K, A.NRow, pcrLevels(A.NRow), G, H, X, Sys, P.Rows);
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
      X = pcrSolveRow(Act, K, A.NRow, DL, D, DU, X, Sys, P.Rows);
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
      const PackedShape P(A.NRow);
      const dim3 Grid = P.grid(A.NBatch);
      const size_t Bytes = (size_t)2 * (Diff ? 3 : 4) * P.Rows * sizeof(Real);
      if (Diff)
         hipLaunchKernelGGL(pcrKernel<true>, Grid, dim3(P.Threads), Bytes, Str, A, P);
      else
         hipLaunchKernelGGL(pcrKernel<false>, Grid, dim3(P.Threads), Bytes, Str, A, P);
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
