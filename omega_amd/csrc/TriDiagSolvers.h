// TriDiagSolvers.h -- batched tridiagonal solvers: Thomas and parallel cyclic reduction (PCR), for general systems and
// for diffusion-type systems.  Interface and names after the reference (components/omega/src/base/TriDiagSolvers.h).
//
// Systems: NBatch independent systems of NRow rows, one per row I of [NBatch][NRow] arrays (each array with its own
// row pitch, so DeviceArray::levels arrays work as they are).
//  - general (ThomasSolver, PCRSolver):  DL(K) x(K-1) + D(K) x(K) + DU(K) x(K+1) = X(K)
//  - diffusion (ThomasDiffusionSolver, PCRDiffusionSolver):
//      -G(K-1) x(K-1) + (H(K) + G(K-1) + G(K)) x(K) - G(K) x(K+1) = X(K)
//    which stays well conditioned where G is many orders of magnitude above H (the general form then gives NaN).
// The reference assumes DL(:,0) = DU(:,NRow-1) = 0 and G(:,NRow-1) = 0.  With other values each algorithm still returns
// exactly its own arithmetic below, and the Thomas and PCR results then differ, as they do in the reference.
//
// Numerical contract (FP64; the library is built with -ffp-contract=off; divisions are the IEEE `/`, no reciprocal
// approximations), restated in NumPy in tests/tridiag_reference.py and bit-identical to it:
//  - Every algorithm follows the reference's operation order and association line for line, e.g. Thomas diffusion's
//    (G(K-1) / H(K-1)) * X(K-1) and PCR diffusion's ((H(Kph) + G(K)) + G(Kph)).
//  - PCR: NLevels = ceil(log2(NRow)) for NRow > 1; levels 1 .. NLevels-1 at half stride 2^(Lev-1) with the index
//    clamps Kmh = max(K - 2^(Lev-1), 0), Kph = min(K + 2^(Lev-1), NRow - 1) and, in the diffusion form, the zero
//    substitutes Gkmh, Gkms for indices below 0; then the 2x2 systems (K, K + 2^(NLevels-1)) and the 1x1 rest.
//  - solve() overwrites X[0:NBatch][0:NRow] with the solution and writes nothing else (no pad columns, no other rows);
//    DL / D / DU (G / H) are left bit for bit unchanged, as the reference's scratch copies leave them.  Nothing is
//    allocated per call.
//
// Deviations from the reference:
//  - NRow = 1: the reference's PCR is undefined there (1 << -1).  It is defined as the 1x1 solve, X / D (general) and
//    X / (H + G) (diffusion), which is also what both Thomas solvers compute.
//  - Supported sizes are 1 <= NRow <= 1024 (TriDiagMaxRows: one row per lane of one workgroup); anything else raises
//    OmegaError naming the limit.
//  - The Kokkos-only members -- makeTeamPolicy and the TriDiagScratch / TriDiagDiffScratch structs -- are not
//    reproduced.  A kernel that solves columns it has assembled itself calls the device bodies of
//    kernels/TriDiagKernels.h (pcrSolveRow, pcrDiffSolveRowRagged, thomasSolveColumn, thomasDiffSolveColumn), the
//    counterpart of the reference's team-level solve(Member, Scratch).
#ifndef OMEGA_AMD_TRIDIAGSOLVERS_H
#define OMEGA_AMD_TRIDIAGSOLVERS_H

#include "Base.h"
#include "kernels/TriDiagKernels.h"

namespace OMEGA {

struct ThomasSolver;
struct PCRSolver;
struct ThomasDiffusionSolver;
struct PCRDiffusionSolver;

// What the reference selects under OMEGA_TARGET_DEVICE (TriDiagSolvers.h:26-35): PCR, for bit compatibility with the
// reference's GPU build
using TriDiagSolver     = PCRSolver;
using TriDiagDiffSolver = PCRDiffusionSolver;

/// ThomasSolver (TriDiagSolvers.h:55-136)
struct ThomasSolver {
   /// ThomasSolver::solve(DL, D, DU, X) (TriDiagSolvers.h:97-134), on stream S
   static void solve(const Array2DReal &DL, const Array2DReal &D, const Array2DReal &DU, const Array2DReal &X,
                     hipStream_t S);
   /// the reference's signature: on the null stream, as Kokkos' default execution space
   static void solve(const Array2DReal &DL, const Array2DReal &D, const Array2DReal &DU, const Array2DReal &X) {
      solve(DL, D, DU, X, nullptr);
   }
};

/// PCRSolver (TriDiagSolvers.h:138-246)
struct PCRSolver {
   /// PCRSolver::solve(DL, D, DU, X) (TriDiagSolvers.h:217-244), on stream S
   static void solve(const Array2DReal &DL, const Array2DReal &D, const Array2DReal &DU, const Array2DReal &X,
                     hipStream_t S);
   static void solve(const Array2DReal &DL, const Array2DReal &D, const Array2DReal &DU, const Array2DReal &X) {
      solve(DL, D, DU, X, nullptr);
   }
};

/// ThomasDiffusionSolver (TriDiagSolvers.h:262-360)
struct ThomasDiffusionSolver {
   /// ThomasDiffusionSolver::solve(G, H, X) (TriDiagSolvers.h:324-359), on stream S
   static void solve(const Array2DReal &G, const Array2DReal &H, const Array2DReal &X, hipStream_t S);
   static void solve(const Array2DReal &G, const Array2DReal &H, const Array2DReal &X) { solve(G, H, X, nullptr); }
};

/// PCRDiffusionSolver (TriDiagSolvers.h:363-485)
struct PCRDiffusionSolver {
   /// PCRDiffusionSolver::solve(G, H, X) (TriDiagSolvers.h:458-483), on stream S
   static void solve(const Array2DReal &G, const Array2DReal &H, const Array2DReal &X, hipStream_t S);
   static void solve(const Array2DReal &G, const Array2DReal &H, const Array2DReal &X) { solve(G, H, X, nullptr); }
};

} // namespace OMEGA
#endif
