// TriDiagKernels.h -- the bodies of the batched tridiagonal solvers behind TriDiagSolvers.h (the reference's
// components/omega/src/base/TriDiagSolvers.h) as device functions, and the host-callable launchers of their array form
// (kernels/TriDiagKernels.hip).  The numerical contract is written down in TriDiagSolvers.h.
//
// The device functions are the counterpart of the reference's team-level solve(Member, Scratch): a kernel that has
// assembled its columns itself (in registers, one row per lane, for PCR; in any memory, one column per lane, for Thomas)
// solves them in place.  Every expression keeps the reference's association; the library is built with
// -ffp-contract=off and divides with the IEEE `/`, so the results are bit for bit those of the reference run serially.
#ifndef OMEGA_AMD_TRIDIAGKERNELS_H
#define OMEGA_AMD_TRIDIAGKERNELS_H

#include "../Base.h"

namespace OMEGA {

/// Largest system the solvers accept (one row per lane of a workgroup for PCR)
constexpr int TriDiagMaxRows = 1024;

// ---------------------------------------------------------------------------------------------------------------------
// device bodies
// ---------------------------------------------------------------------------------------------------------------------

/// Number of PCR levels, ceil(log2(NRow)) for NRow > 1 (TriDiagSolvers.h:160, in integers: exact for NRow <= 2^31)
__host__ __device__ inline int pcrLevels(int NRow) {
   int L = 0;
   while ((1 << L) < NRow)
      ++L;
   return L;
}

/// PCRSolver::solve(Member, Scratch) (TriDiagSolvers.h:152-213) for the row K of one system of NRow rows whose
/// coefficients this thread holds (DL, D, DU, X); returns the solution of row K.
///
/// Every thread of the workgroup calls it with the same NRow (it holds pcrLevels(NRow) __syncthreads()); a thread
/// with no row passes Active = false and only joins the barriers.  `Sys` points to row 0 of the thread's system in a
/// workspace of 2 x 4 arrays of `Span` doubles each (array A of buffer B at Sys[(B * 4 + A) * Span + row]), in LDS;
/// several systems may share one workspace at different offsets.  The workspace is read until the function returns:
/// a caller that reuses it barriers first.
__device__ inline Real pcrSolveRow(bool Active, int K, int NRow, Real DL, Real D, Real DU, Real X, Real *Sys,
                                   int Span) {
   if (NRow == 1) // the reference's 1 << -1; defined as the 1x1 solve (TriDiagSolvers.h)
      return X / D;
   const int NLevels = pcrLevels(NRow);
   int B             = 0;
   for (int Lev = 1; Lev < NLevels; ++Lev) {
      Real *W = Sys + B * 4 * Span;
      if (Active) {
         W[0 * Span + K] = DL, W[1 * Span + K] = D, W[2 * Span + K] = DU, W[3 * Span + K] = X;
      }
      __syncthreads();
      if (Active) {
         const int HalfStride = 1 << (Lev - 1);
         int Kmh              = K - HalfStride;
         Kmh                  = Kmh < 0 ? 0 : Kmh;
         int Kph              = K + HalfStride;
         Kph                  = Kph >= NRow ? NRow - 1 : Kph;

         const Real Alpha = -DL / W[1 * Span + Kmh];
         const Real Gamma = -DU / W[1 * Span + Kph];

         const Real NewD  = D + Alpha * W[2 * Span + Kmh] + Gamma * W[0 * Span + Kph];
         const Real NewX  = X + Alpha * W[3 * Span + Kmh] + Gamma * W[3 * Span + Kph];
         const Real NewDL = Alpha * W[0 * Span + Kmh];
         const Real NewDU = Gamma * W[2 * Span + Kph];
         DL = NewDL, D = NewD, DU = NewDU, X = NewX;
      }
      B ^= 1; // the next level writes the other buffer: one barrier per level
   }
   Real *W = Sys + B * 4 * Span;
   if (Active) {
      W[0 * Span + K] = DL, W[1 * Span + K] = D, W[2 * Span + K] = DU, W[3 * Span + K] = X;
   }
   __syncthreads();
   if (!Active)
      return X;
   const int Stride = 1 << (NLevels - 1);
   // The 2x2 systems (K, K + Stride): the reference's thread K (K < NRow / 2) writes both rows; here each row's thread
   // computes its own row with the same expressions.  K + Stride < NRow implies K < NRow / 2 because Stride >= NRow / 2.
   if (K + Stride < NRow) {
      const int P     = K + Stride;
      const Real Det  = D * W[1 * Span + P] - W[0 * Span + P] * DU;
      const Real Xk   = X;
      const Real Xkps = W[3 * Span + P];
      return (W[1 * Span + P] * Xk - DU * Xkps) / Det;
   }
   if (K - Stride >= 0) {
      const int P     = K - Stride;
      const Real Det  = W[1 * Span + P] * D - DL * W[2 * Span + P];
      const Real Xk   = W[3 * Span + P];
      const Real Xkps = X;
      return (-DL * Xk + W[1 * Span + P] * Xkps) / Det;
   }
   return X / D; // 1x1 system
}

/// One level of PCRDiffusionSolver::solve(Member, Scratch) (TriDiagSolvers.h:377-454) on (G, H) of row K: W holds the
/// level's G of every row of the system at W[row] and its H at W[Span + row].  G and H become the next level's; what
/// is returned takes a right-hand side through the same level: X = X + Alpha * X[Kmh] + Beta * X[Kph].
struct PcrDiffLevel {
   Real Alpha, Beta;
   int Kmh, Kph;
};
__device__ inline PcrDiffLevel pcrDiffLevel(int Lev, int K, int NRow, Real &G, Real &H, const Real *W, int Span) {
   const int Stride     = 1 << Lev;
   const int HalfStride = 1 << (Lev - 1);
   PcrDiffLevel L;

   int Kmh         = K - HalfStride;
   const Real Gkmh = Kmh < 0 ? 0 : W[0 * Span + Kmh];
   L.Kmh           = Kmh < 0 ? 0 : Kmh;

   const int Kms   = K - Stride;
   const Real Gkms = Kms < 0 ? 0 : W[0 * Span + Kms];

   const int Kph = K + HalfStride;
   L.Kph         = Kph >= NRow ? NRow - 1 : Kph;

   L.Alpha = Gkmh / (W[1 * Span + L.Kmh] + Gkms + Gkmh);
   L.Beta  = G / (W[1 * Span + L.Kph] + G + W[0 * Span + L.Kph]);

   const Real NewG = W[0 * Span + L.Kph] * L.Beta;
   const Real NewH = H + L.Alpha * W[1 * Span + L.Kmh] + L.Beta * W[1 * Span + L.Kph];
   G = NewG, H = NewH;
   return L;
}

/// The final 2x2 / 1x1 systems of the diffusion-form PCR for row K, from the reduced G, H of the last level (W as in
/// pcrDiffLevel; NLev = pcrLevels(NRow)): the reference's thread K (K < NRow / 2) writes both rows of a 2x2 system,
/// here each row's thread computes its own row with the same expressions, value() below.
struct PcrDiffFinal {
   int Partner = -1; ///< the other row of the 2x2 system; -1: a 1x1 system
   bool Upper  = false; ///< this row is the first of the two
   Real Ca = 1, Cb = 0, Det = 1;
   /// X of this row and Xw[row] of the others
   __device__ Real value(Real X, const Real *Xw) const {
      if (Partner < 0)
         return X / Det;
      if (Upper)
         return (Ca * X - Cb * Xw[Partner]) / Det;
      return (Ca * Xw[Partner] + Cb * X) / Det; // the reference's order: its row K's term first
   }
};
__device__ inline PcrDiffFinal pcrDiffFinal(int K, int NRow, int NLev, Real G, Real H, const Real *W, int Span) {
   PcrDiffFinal F;
   if (NRow == 1) { // the reference's 1 << -1; defined as the 1x1 solve (TriDiagSolvers.h)
      F.Det = H + G;
      return F;
   }
   const int Stride = 1 << (NLev - 1);
   if (K + Stride < NRow) { // 2x2 system (K, K + Stride), row K: (Dkps * Xk - DUk * Xkps) / Det
      const int P      = K + Stride;
      const int Kms    = K - Stride;
      const Real Gkms  = Kms < 0 ? 0 : W[0 * Span + Kms];
      const Real Dk    = H + Gkms + G;
      const Real Dkps  = W[1 * Span + P] + G + W[0 * Span + P];
      const Real DUk   = -G;
      const Real DLkps = -G;
      F.Det            = Dk * Dkps - DLkps * DUk;
      F.Partner = P, F.Upper = true, F.Ca = Dkps, F.Cb = DUk;
   } else if (K - Stride >= 0) { // 2x2 system (K - Stride, K), row K: (-DLkps * Xk + Dk * Xkps) / Det
      const int P      = K - Stride;
      const int Kms    = P - Stride;
      const Real Gp    = W[0 * Span + P];
      const Real Gkms  = Kms < 0 ? 0 : W[0 * Span + Kms];
      const Real Dk    = W[1 * Span + P] + Gkms + Gp;
      const Real Dkps  = H + Gp + G;
      const Real DUk   = -Gp;
      const Real DLkps = -Gp;
      F.Det            = Dk * Dkps - DLkps * DUk;
      F.Partner = P, F.Ca = -DLkps, F.Cb = Dk;
   } else { // 1x1 system
      const int Kms   = K - Stride;
      const Real Gkms = Kms < 0 ? 0 : W[0 * Span + Kms];
      F.Det           = H + Gkms + G;
   }
   return F;
}

/// PCRDiffusionSolver::solve(Member, Scratch) (TriDiagSolvers.h:377-454) for row K, as pcrSolveRow, for the systems of
/// one workgroup, which may differ in NRow: NLevWg is the workgroup-uniform number of barrier steps, at least
/// pcrLevels(NRow) of every system in it (pcrLevels(NRow) itself when they are all alike).  A system that has finished
/// its own levels keeps joining the barriers without touching the workspace, and reads its last level after them: the
/// systems own disjoint rows.  One right-hand side, so G, H and X go through the levels together (one barrier per
/// level, no Alpha / Beta kept).  `Sys` points to row 0 of the thread's system in a workspace of 2 x 3 arrays (G, H, X)
/// of `Span` doubles (array A of buffer B at Sys[(B * 3 + A) * Span + row]); a caller that reuses it barriers first.
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
         const PcrDiffLevel L = pcrDiffLevel(Lev, K, NRow, G, H, W, Span);
         X                    = X + L.Alpha * W[2 * Span + L.Kmh] + L.Beta * W[2 * Span + L.Kph];
         B ^= 1; // the next level writes the other buffer; the last level's buffer stays to be read below
      }
   }
   if (!Active)
      return X;
   const Real *W = Sys + B * 3 * Span;
   return pcrDiffFinal(K, NRow, NLev, G, H, W, Span).value(X, W + 2 * Span);
}

/// Largest PCR level count (pcrLevels(TriDiagMaxRows)): the multi-right-hand-side body keeps one Alpha / Beta per level
/// in registers, so its level loops have this compile-time bound
constexpr int TriDiagMaxLevels = 10;

/// pcrDiffSolveRowRagged for NRhs right-hand sides that share G and H (e.g. every tracer of a column): the result for
/// each right-hand side is bit for bit that of pcrDiffSolveRowRagged on (G, H, X_t).  Everything that depends only on G and H --
/// Alpha, Beta, NewG, NewH of every level and the final Dk / Dkps / Det -- is computed once; each X_t then goes
/// through the same levels with the stored Alpha / Beta, Chunk right-hand sides at a time.  LoadX(T) returns X of
/// right-hand side T of this row and StoreX(T, V) takes its solution (called only when Active).
///
/// The systems of one workgroup may have different NRow (columns of different depth): NLevWg is the workgroup-uniform
/// number of barrier steps, at least pcrLevels(NRow) of every system in it.  A system that has finished its own levels
/// keeps joining the barriers without touching the workspace.  `Sys` points to row 0 of the thread's system in a
/// workspace of 2 x 2 arrays (G, H) followed by 2 x Chunk arrays (X) of `Span` doubles each, in LDS.
template <int Chunk, class LoadX, class StoreX>
__device__ inline void pcrDiffSolveRowMulti(bool Active, int K, int NRow, int NLevWg, Real G, Real H, int NRhs,
                                            LoadX Load, StoreX Store, Real *Sys, int Span) {
   const int NLev = Active ? pcrLevels(NRow) : 0;
   Real Alpha[TriDiagMaxLevels], Beta[TriDiagMaxLevels];
   Real *GH = Sys, *XW = Sys + 4 * Span;
   // ---- G and H: the levels of pcrDiffSolveRowRagged, keeping Alpha and Beta; the last step writes the reduced G, H
   int B = 0;
#pragma unroll
   for (int Lev = 1; Lev <= TriDiagMaxLevels; ++Lev) {
      if (Lev > NLevWg) // workgroup-uniform: a condition, not a break, so that the loop unrolls
         continue;
      Real *W = GH + B * 2 * Span;
      if (Lev <= NLev) {
         W[0 * Span + K] = G, W[1 * Span + K] = H;
      }
      __syncthreads();
      if (Lev < NLev) {
         const PcrDiffLevel L = pcrDiffLevel(Lev, K, NRow, G, H, W, Span);
         Alpha[Lev - 1] = L.Alpha, Beta[Lev - 1] = L.Beta;
         B ^= 1;
      }
   }
   // ---- the final 2x2 / 1x1 systems, once for every right-hand side
   const PcrDiffFinal F = Active ? pcrDiffFinal(K, NRow, NLev, G, H, GH + B * 2 * Span, Span) : PcrDiffFinal();
   // ---- every right-hand side through the stored levels
   for (int T0 = 0; T0 < NRhs; T0 += Chunk) {
      if (T0 > 0)
         __syncthreads(); // the previous chunk's final step read the workspace
      Real X[Chunk];
#pragma unroll
      for (int J = 0; J < Chunk; ++J)
         X[J] = (Active && T0 + J < NRhs) ? Load(T0 + J) : 0;
      int Bx = 0;
#pragma unroll
      for (int Lev = 1; Lev <= TriDiagMaxLevels; ++Lev) {
         if (Lev > NLevWg)
            continue;
         Real *W = XW + Bx * Chunk * Span;
         if (Lev <= NLev) {
#pragma unroll
            for (int J = 0; J < Chunk; ++J)
               W[J * Span + K] = X[J];
         }
         __syncthreads();
         if (Lev < NLev) {
            const int HalfStride = 1 << (Lev - 1);
            int Kmh              = K - HalfStride;
            Kmh                  = Kmh < 0 ? 0 : Kmh;
            int Kph              = K + HalfStride;
            Kph                  = Kph >= NRow ? NRow - 1 : Kph;
            const Real A = Alpha[Lev - 1], Bt = Beta[Lev - 1];
#pragma unroll
            for (int J = 0; J < Chunk; ++J)
               X[J] = X[J] + A * W[J * Span + Kmh] + Bt * W[J * Span + Kph];
            Bx ^= 1;
         }
      }
      if (Active) {
         const Real *W = XW + Bx * Chunk * Span;
#pragma unroll
         for (int J = 0; J < Chunk; ++J) {
            if (T0 + J >= NRhs)
               break;
            Store(T0 + J, F.value(X[J], W + J * Span));
         }
      }
   }
}

/// ThomasSolver::solve(Member, Scratch) (TriDiagSolvers.h:69-93) for one column of NRow rows, by one thread.  Row K of
/// DL / D / DU is at [K * InStride], of X at [K * XStride] (overwritten with the solution), and `Dw` is a workspace of
/// NRow doubles at [K * WStride] that takes the eliminated diagonal (the reference's scratch copy of D).
__device__ inline void thomasSolveColumn(int NRow, const Real *DL, const Real *D, const Real *DU, int InStride,
                                         Real *X, int XStride, Real *Dw, int WStride) {
   Real Dp = D[0], Xp = X[0];
   Dw[0] = Dp;
   for (int K = 1; K < NRow; ++K) {
      const Real W = DL[K * InStride] / Dp;
      Dp           = D[K * InStride] - W * DU[(K - 1) * InStride];
      Xp           = X[K * XStride] - W * Xp;
      Dw[K * WStride] = Dp;
      X[K * XStride]  = Xp;
   }
   Xp = Xp / Dp;
   X[(NRow - 1) * XStride] = Xp;
   for (int K = NRow - 2; K >= 0; --K) {
      Xp             = (X[K * XStride] - DU[K * InStride] * Xp) / Dw[K * WStride];
      X[K * XStride] = Xp;
   }
}

/// ThomasDiffusionSolver::solve(Member, Scratch) (TriDiagSolvers.h:276-320) for one column, as thomasSolveColumn;
/// `Hw` takes the eliminated diagonal (the reference's in-place H).  The reference's Alpha array is carried as one
/// running value: its loop over K only reads the original G and H.
__device__ inline void thomasDiffSolveColumn(int NRow, const Real *G, const Real *H, int InStride, Real *X,
                                             int XStride, Real *Hw, int WStride) {
   Real Alpha = 0;
   Real Hp    = H[0] + G[0];
   Real Xp    = X[0];
   Hw[0]      = Hp;
   for (int K = 1; K < NRow; ++K) {
      const Real Gm = G[(K - 1) * InStride], Hm = H[(K - 1) * InStride];
      Alpha           = Gm * (Hm + Alpha) / (Hm + Alpha + Gm);
      const Real AddH = Alpha + G[K * InStride];
      Xp              = X[K * XStride] + Gm / Hp * Xp;
      Hp              = H[K * InStride] + AddH;
      Hw[K * WStride] = Hp;
      X[K * XStride]  = Xp;
   }
   Xp = Xp / Hp;
   X[(NRow - 1) * XStride] = Xp;
   for (int K = NRow - 2; K >= 0; --K) {
      Xp             = (X[K * XStride] + G[K * InStride] * Xp) / Hw[K * WStride];
      X[K * XStride] = Xp;
   }
}

// ---------------------------------------------------------------------------------------------------------------------
// array launchers (kernels/TriDiagKernels.hip)
// ---------------------------------------------------------------------------------------------------------------------

/// One batched solve of NBatch systems of NRow rows (1 <= NRow <= TriDiagMaxRows).  Row I of each array starts at
/// Ptr + I * Pitch.  General form: A = DL, B = D, C = DU; diffusion form: A = G, B = H, C unused.
struct TriDiagArgs {
   int NBatch = 0, NRow = 0;
   const Real *A = nullptr, *B = nullptr, *C = nullptr;
   int PitchA = 0, PitchB = 0, PitchC = 0;
   Real *X    = nullptr;
   int PitchX = 0;
};

enum class TriDiagAlgo { Thomas, PCR, ThomasDiffusion, PCRDiffusion };

/// Asynchronous on stream S; writes X[0:NBatch][0:NRow] only and allocates nothing.
void launchTriDiag(TriDiagAlgo Algo, const TriDiagArgs &A, hipStream_t S);

} // namespace OMEGA
#endif
