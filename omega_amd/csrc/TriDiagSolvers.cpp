// TriDiagSolvers.cpp -- see TriDiagSolvers.h.
#include "TriDiagSolvers.h"

namespace OMEGA {

namespace {

/// Extents of X (NBatch, NRow) after checking every array against them
void requireSame(const char *Who, const Array2DReal &X, std::initializer_list<std::pair<const char *, const Array2DReal *>> In) {
   const int NBatch = X.Ext[0], NRow = X.Ext[1];
   OMEGA_REQUIRE(NRow >= 1 && NRow <= TriDiagMaxRows, std::string(Who) + ": NRow = " + std::to_string(NRow) +
                                                        " is outside the supported 1 <= NRow <= " +
                                                        std::to_string(TriDiagMaxRows));
   OMEGA_REQUIRE(NBatch >= 0, std::string(Who) + ": negative NBatch");
   OMEGA_REQUIRE(X.Pitch >= NRow, std::string(Who) + ": X has a row pitch below NRow");
   OMEGA_REQUIRE(NBatch == 0 || X.Ptr != nullptr, std::string(Who) + ": X is empty");
   for (const auto &P : In) {
      const Array2DReal &A = *P.second;
      OMEGA_REQUIRE(A.Ext[0] == NBatch && A.Ext[1] == NRow,
                    std::string(Who) + ": " + P.first + " is [" + std::to_string(A.Ext[0]) + "][" +
                        std::to_string(A.Ext[1]) + "], X is [" + std::to_string(NBatch) + "][" +
                        std::to_string(NRow) + "]: extents must match");
      OMEGA_REQUIRE(A.Pitch >= NRow, std::string(Who) + ": " + P.first + " has a row pitch below NRow");
      OMEGA_REQUIRE(NBatch == 0 || A.Ptr != nullptr, std::string(Who) + ": " + P.first + " is empty");
   }
}

TriDiagArgs args(const Array2DReal &A, const Array2DReal &B, const Array2DReal *C, const Array2DReal &X) {
   TriDiagArgs T;
   T.NBatch = X.Ext[0], T.NRow = X.Ext[1];
   T.A = A.Ptr, T.PitchA = A.Pitch;
   T.B = B.Ptr, T.PitchB = B.Pitch;
   if (C)
      T.C = C->Ptr, T.PitchC = C->Pitch;
   T.X = X.Ptr, T.PitchX = X.Pitch;
   return T;
}

} // namespace

void ThomasSolver::solve(const Array2DReal &DL, const Array2DReal &D, const Array2DReal &DU, const Array2DReal &X,
                         hipStream_t S) {
   requireSame("ThomasSolver::solve", X, {{"DL", &DL}, {"D", &D}, {"DU", &DU}});
   launchTriDiag(TriDiagAlgo::Thomas, args(DL, D, &DU, X), S);
}

void PCRSolver::solve(const Array2DReal &DL, const Array2DReal &D, const Array2DReal &DU, const Array2DReal &X,
                      hipStream_t S) {
   requireSame("PCRSolver::solve", X, {{"DL", &DL}, {"D", &D}, {"DU", &DU}});
   launchTriDiag(TriDiagAlgo::PCR, args(DL, D, &DU, X), S);
}

void ThomasDiffusionSolver::solve(const Array2DReal &G, const Array2DReal &H, const Array2DReal &X, hipStream_t S) {
   requireSame("ThomasDiffusionSolver::solve", X, {{"G", &G}, {"H", &H}});
   launchTriDiag(TriDiagAlgo::ThomasDiffusion, args(G, H, nullptr, X), S);
}

void PCRDiffusionSolver::solve(const Array2DReal &G, const Array2DReal &H, const Array2DReal &X, hipStream_t S) {
   requireSame("PCRDiffusionSolver::solve", X, {{"G", &G}, {"H", &H}});
   launchTriDiag(TriDiagAlgo::PCRDiffusion, args(G, H, nullptr, X), S);
}

} // namespace OMEGA
