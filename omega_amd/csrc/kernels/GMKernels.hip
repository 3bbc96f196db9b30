// GMKernels.hip -- the eddy bolus-velocity kernel behind GentMcWilliams (GentMcWilliams.h) on gfx950.
//
// One launch, the edge geometry of the implicit vertical-mixing solves (kernels/VertMixKernels.hip): lanes along the
// layers of an edge column (layer Lo + I on lane I), floor(256 / K) columns per workgroup (one for K > 256, up to 1024
// lanes).  A lane reads its layer of the two cells once -- SpecVol, SpecVolDisplaced, ZMid, thickness: coalesced along
// the levels -- and hands the seven values the interface below it needs (the two densities, the two heights, the two
// displaced densities, the edge thickness) to the next lane through LDS: no row is fetched from HBM twice by one column.
// Lane I >= 1 then holds row I - 1 of the column's system (the interface at the top of its layer) in registers and
// solves it with pcrDiffSolveRowRagged below: the expressions of pcrDiffSolveRow (kernels/TriDiagKernels.h), so its
// bits, with the barriers counted for the workgroup as pcrDiffSolveRowMulti counts them, which lets columns of
// different depth share a workgroup; G, H and X go through the levels together, one barrier per level (the
// multi-right-hand-side body takes two).  The exchange area and the solver's workspace are the same LDS (7 and 6
// arrays of one double per lane); the stream function goes through it once more, to the lane above, for the vertical
// difference.  No scratch, no global atomics; the column tile of LevelTile.h (lanes along the columns) does not fit a
// solve that has its rows on the lanes, so only the launch shape is shared, with the mixing solves.
#include "GMKernels.h"
#include "TriDiagKernels.h"

namespace OMEGA {

namespace {

constexpr int GMLanes  = 256; // lanes a workgroup of short columns fills
constexpr int GMArrays = 7;   // LDS doubles per lane: the exchange (7) covers the solver's workspace (2 x 3)

/// pcrDiffSolveRow (kernels/TriDiagKernels.h) for the systems of one workgroup when they differ in NRow: the same
/// expressions on (G, H, X) level by level, so the bits of pcrDiffSolveRow, with the barriers counted for the workgroup
/// -- NLevWg, at least pcrLevels(NRow) of every system in it -- as pcrDiffSolveRowMulti counts them.  A system that
/// has finished its own levels keeps joining the barriers without touching the workspace, and reads its last level
/// after them: the systems own disjoint rows.  One right-hand side, so G, H and X go through the levels together (one
/// barrier per level, no Alpha / Beta kept).  `Sys` points to row 0 of the thread's system in a workspace of 2 x 3
/// arrays of `Span` doubles (array A of buffer B at Sys[(B * 3 + A) * Span + row]); a caller that reuses it barriers
/// first.
__device__ inline Real pcrDiffSolveRowRagged(bool Active, int K, int NRow, int NLevWg, Real G, Real H, Real X,
                                             Real *Sys, int Span) {
   const int NLev = Active ? pcrLevels(NRow) : 0;
   int B          = 0;
   for (int Lev = 1; Lev <= NLevWg; ++Lev) { // workgroup-uniform
      Real *W = Sys + B * 3 * Span;
      if (Lev <= NLev) {
         W[0 * Span + K] = G, W[1 * Span + K] = H, W[2 * Span + K] = X;
      }
      __syncthreads();
      if (Lev < NLev) {
         const int Stride     = 1 << Lev;
         const int HalfStride = 1 << (Lev - 1);

         int Kmh         = K - HalfStride;
         const Real Gkmh = Kmh < 0 ? 0 : W[0 * Span + Kmh];
         Kmh             = Kmh < 0 ? 0 : Kmh;

         const int Kms   = K - Stride;
         const Real Gkms = Kms < 0 ? 0 : W[0 * Span + Kms];

         int Kph = K + HalfStride;
         Kph     = Kph >= NRow ? NRow - 1 : Kph;

         const Real Alpha = Gkmh / (W[1 * Span + Kmh] + Gkms + Gkmh);
         const Real Beta  = G / (W[1 * Span + Kph] + G + W[0 * Span + Kph]);

         const Real NewG = W[0 * Span + Kph] * Beta;
         const Real NewX = X + Alpha * W[2 * Span + Kmh] + Beta * W[2 * Span + Kph];
         const Real NewH = H + Alpha * W[1 * Span + Kmh] + Beta * W[1 * Span + Kph];
         G = NewG, H = NewH, X = NewX;
         B ^= 1; // the next level writes the other buffer; the last level's buffer stays to be read below
      }
   }
   if (!Active)
      return X;
   if (NRow == 1) // the 1x1 solve (TriDiagSolvers.h)
      return X / (H + G);
   const Real *W    = Sys + B * 3 * Span;
   const int Stride = 1 << (NLev - 1);
   if (K + Stride < NRow) { // 2x2 system (K, K + Stride), row K
      const int P      = K + Stride;
      const int Kms    = K - Stride;
      const Real Gkms  = Kms < 0 ? 0 : W[0 * Span + Kms];
      const Real Dk    = H + Gkms + G;
      const Real Dkps  = W[1 * Span + P] + G + W[0 * Span + P];
      const Real DUk   = -G;
      const Real DLkps = -G;
      const Real Det   = Dk * Dkps - DLkps * DUk;
      const Real Xk    = X;
      const Real Xkps  = W[2 * Span + P];
      return (Dkps * Xk - DUk * Xkps) / Det;
   }
   if (K - Stride >= 0) { // 2x2 system (K - Stride, K), row K
      const int P      = K - Stride;
      const int Kms    = P - Stride;
      const Real Gp    = W[0 * Span + P];
      const Real Gkms  = Kms < 0 ? 0 : W[0 * Span + Kms];
      const Real Dk    = W[1 * Span + P] + Gkms + Gp;
      const Real Dkps  = H + Gp + G;
      const Real DUk   = -Gp;
      const Real DLkps = -Gp;
      const Real Det   = Dk * Dkps - DLkps * DUk;
      const Real Xk    = W[2 * Span + P];
      const Real Xkps  = X;
      return (-DLkps * Xk + Dk * Xkps) / Det;
   }
   const int Kms   = K - Stride; // 1x1 system
   const Real Gkms = Kms < 0 ? 0 : W[0 * Span + Kms];
   return X / (H + Gkms + G);
}

__global__ void __launch_bounds__(TriDiagMaxRows) bolusVelocityKernel(GMArgs A, int Pitch, int SysPerBlock, int Rows) {
   extern __shared__ Real Lds[];
   __shared__ int NLevShared;
   const int T      = threadIdx.x;
   const int S      = T / A.K;
   const int I      = T - S * A.K; // layer of the column: level Lo + I
   const long Col   = (long)blockIdx.x * SysPerBlock + S;
   const bool InSys = T < Rows && Col < A.NEdgesAll;
   int Lo = 0, N = 0;
   if (InSys) {
      Lo           = A.MinLayerEdgeBot[Col];
      const int Hi = A.MaxLayerEdgeTop[Col];
      if (Lo >= 0 && Lo <= Hi && Hi < A.K)
         N = Hi - Lo + 1;
   }
   if (T == 0)
      NLevShared = 0;
   __syncthreads();
   if (InSys && I == 0 && N > 1)
      atomicMax(&NLevShared, pcrLevels(N - 1));
   __syncthreads();
   const int NLevWg = NLevShared;
   const bool Act   = InSys && I < N;
   const int Lev    = Lo + I;

   // ---- this lane's layer of the two cells, and what the interface below it needs of it
   Real Rho0 = 0, Rho1 = 0, Z0 = 0, Z1 = 0, Rd0 = 0, Rd1 = 0, HE = 1, InvDc = 0;
   if (Act) {
      const size_t C0 = (size_t)A.CellsOnEdge[2 * Col] * Pitch + Lev, C1 = (size_t)A.CellsOnEdge[2 * Col + 1] * Pitch + Lev;
      Rho0  = 1.0 / A.SpecVol[C0];
      Rho1  = 1.0 / A.SpecVol[C1];
      HE    = 0.5 * (A.LayerThickness[C0] + A.LayerThickness[C1]);
      Z0    = A.ZMid[C0];
      Z1    = A.ZMid[C1];
      InvDc = 1.0 / A.DcEdge[Col];
      if (I < N - 1) { // the bottom layer's displaced volume is not part of the contract (it may be unset)
         Rd0 = 1.0 / A.SpecVolDisplaced[C0];
         Rd1 = 1.0 / A.SpecVolDisplaced[C1];
      }
      Lds[0 * Rows + T] = Rho0, Lds[1 * Rows + T] = Rho1, Lds[2 * Rows + T] = Z0, Lds[3 * Rows + T] = Z1;
      Lds[4 * Rows + T] = Rd0, Lds[5 * Rows + T] = Rd1, Lds[6 * Rows + T] = HE;
   }
   __syncthreads();

   // ---- row I - 1 of the system: the interface between layer Lev - 1 (the lane above) and layer Lev
   const bool Row = Act && I >= 1;
   const int NRow = N - 1, R = I - 1;
   Real G = 0, H = 1, X = 0;
   if (Row) {
      const int U      = T - 1;
      const Real Rho0u = Lds[0 * Rows + U], Rho1u = Lds[1 * Rows + U], Z0u = Lds[2 * Rows + U], Z1u = Lds[3 * Rows + U];
      const Real Rd0u = Lds[4 * Rows + U], Rd1u = Lds[5 * Rows + U], HEu = Lds[6 * Rows + U];
      const Real GR    = A.GOverRho0;
      const Real GradRho = (Rho1 - Rho0) * InvDc, GradRhoU = (Rho1u - Rho0u) * InvDc;
      const Real GradZ = (Z1 - Z0) * InvDc, GradZU = (Z1u - Z0u) * InvDc;
      const Real Dz0 = Z0u - Z0, Dz1 = Z1u - Z1;
      const Real RhoZ0 = (Rho0u - Rho0) / Dz0, RhoZ1 = (Rho1u - Rho1) / Dz1;
      const Real N20 = (GR * (Rho0 - Rd0u)) / Dz0, N21 = (GR * (Rho1 - Rd1u)) / Dz1;
      const Real RhoZE = 0.5 * (RhoZ0 + RhoZ1);
      Real N2E         = 0.5 * (N20 + N21);
      N2E              = N2E < 0.0 ? 0.0 : N2E;
      const Real GradRhoZ = 0.5 * (GradRhoU + GradRho) - RhoZE * (0.5 * (GradZU + GradZ));
      const Real DzMid    = 0.5 * (HEu + HE);
      G = R < NRow - 1 ? A.C2 / HE : 0.0;
      H = N2E * DzMid;
      if (R == 0)
         H = H + A.C2 / HEu;
      if (R == NRow - 1)
         H = H + A.C2 / HE;
      X = DzMid * ((A.Kappa[Col] * GR) * GradRhoZ);
   }
   __syncthreads(); // the exchange has been read: the solver takes the LDS over

   Real Psi = pcrDiffSolveRowRagged(Row, R, NRow, NLevWg, G, H, X, Lds + S * A.K, Rows);
   if (!Row)
      Psi = 0; // the surface, and the lanes without a layer
   __syncthreads(); // the solver's last step has read its workspace

   // ---- u* = -(d Psi / dz) over the layer: the interface below is the next lane's
   if (Act)
      Lds[T] = Psi; // 0 on lane 0: the surface
   __syncthreads();
   if (Act) {
      const Real Top = I == 0 ? 0.0 : Psi;
      const Real Bot = I == N - 1 ? 0.0 : Lds[T + 1];
      const Real Ub  = (Bot - Top) / HE;
      const size_t E = (size_t)Col * Pitch + Lev;
      A.StreamFunction[E] = Top;
      A.BolusVelocity[E]  = Ub;
      if (A.Transport != nullptr)
         A.Transport[E] = A.Transport[E] + Ub;
   }
}

} // namespace

void launchBolusVelocity(const GMArgs &A, hipStream_t S) {
   OMEGA_REQUIRE(A.K >= 1 && A.K <= TriDiagMaxRows, "GentMcWilliams: NVertLayers = " + std::to_string(A.K) +
                                                        " is outside the supported 1 <= NVertLayers <= " +
                                                        std::to_string(TriDiagMaxRows));
   if (A.NEdgesAll <= 0)
      return;
   // columns per workgroup and the lanes they occupy (as the mixing solves and the PCR array launcher)
   const int Sys     = A.K <= GMLanes ? GMLanes / A.K : 1;
   const int Rows    = Sys * A.K;
   const int Threads = (Rows + 63) / 64 * 64;
   const dim3 Grid((A.NEdgesAll + Sys - 1) / Sys);
   const size_t Bytes = (size_t)GMArrays * Rows * sizeof(Real);
   hipLaunchKernelGGL(bolusVelocityKernel, Grid, dim3(Threads), Bytes, S, A, levelPitch(A.K), Sys, Rows);
   HIP_CHECK(hipGetLastError());
}

} // namespace OMEGA
