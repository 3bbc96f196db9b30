// SplitExplicitStepper.cpp -- see SplitExplicitStepper.h.
#include "SplitExplicitStepper.h"
#include "PressureGrad.h"
#include "VertMixStep.h"

namespace OMEGA {

void SplitExplicitStepper::attachBarotropic(BarotropicMode *B, int N) {
   OMEGA_REQUIRE(Tend && Mesh && Trc, "SplitExplicitStepper::attachBarotropic: attachData first");
   OMEGA_REQUIRE(B != nullptr, "SplitExplicitStepper::attachBarotropic: the BarotropicMode is NULL");
   OMEGA_REQUIRE(B->Mesh == Mesh && B->NVertLayers == Tend->LayerThicknessTend.Ext[1],
                 "SplitExplicitStepper::attachBarotropic: the BarotropicMode was built for another mesh or layer count");
   OMEGA_REQUIRE(N >= 1, "SplitExplicitStepper::attachBarotropic: NSub = " + std::to_string(N) +
                             " is not a number of sub-steps (>= 1)");
   OMEGA_REQUIRE(!MeshHalo || MeshHalo->NNghbr == 0,
                 "SplitExplicitStepper::attachBarotropic: this stepper's halo has neighbours: BarotropicMode knows no "
                 "Halo, and more sub-steps than the halo is wide need an exchange per sub-step, which is not built");
   Btr  = B;
   NSub = N;
}

void SplitExplicitStepper::requireMonotoneAdvFits(const MonotoneAdv *M, const char *Where) const {
   const std::string W = std::string(Where) + ": ";
   OMEGA_REQUIRE(M->Mesh == Mesh && M->NVertLayers == Tend->LayerThicknessTend.Ext[1],
                 W + "the MonotoneAdv was built for another mesh or layer count");
   OMEGA_REQUIRE(M->MaxTracers >= Tend->NTracers, W + "the MonotoneAdv has MaxTracers = " + std::to_string(M->MaxTracers) +
                                                      ", below the stepper's " + std::to_string(Tend->NTracers) + " tracers");
   const bool AuxUpwind = AuxState->LayerThicknessAux.FluxThickEdgeChoice == FluxThickEdgeOption::Upwind;
   OMEGA_REQUIRE(M->Config.FluxThicknessUpwind == AuxUpwind,
                 W + "the MonotoneAdv's FluxThicknessUpwind differs from the AuxiliaryState's FluxThickEdgeChoice: the "
                     "limiter must see the mass fluxes the thickness equation uses");
   OMEGA_REQUIRE(!Tend->Params.TracerHorzAdvTendencyEnable,
                 W + "TracerHorzAdvTendencyEnable is on: the Tendencies' own horizontal tracer advection and the "
                     "MonotoneAdv would both be applied; switch the term off");
   if (const VertAdv *V = M->vertAdv()) { // the 3-D form: VerticalTransport must be the step's, and limited only once
      OMEGA_REQUIRE(V == Tend->vertAdv(), W + "the MonotoneAdv's VertAdv is not the one attached to the Tendencies: its "
                                              "VerticalTransport would not be that of the step");
      OMEGA_REQUIRE(!V->TracerTermEnable,
                    W + "the VertAdv's TracerTermEnable is on: the Tendencies' vertical tracer term and the MonotoneAdv's "
                        "limited one would both be applied; switch the term off");
   }
}

void SplitExplicitStepper::attachMonotoneAdv(MonotoneAdv *M) {
   if (M == nullptr) {
      Mono = nullptr;
      return;
   }
   OMEGA_REQUIRE(Tend && Mesh && Trc && AuxState, "SplitExplicitStepper::attachMonotoneAdv: attachData first");
   requireMonotoneAdvFits(M, "SplitExplicitStepper::attachMonotoneAdv");
   Mono = M;
}

void SplitExplicitStepper::requireColumnPassFits(const ColumnPass &C, const std::string &Class,
                                                 const std::string &W) const {
   OMEGA_REQUIRE(C.Mesh == Mesh && C.NVertLayers == Tend->LayerThicknessTend.Ext[1],
                 W + "the " + Class + " was built for another mesh or layer count");
   OMEGA_REQUIRE(Tend->NTracers >= 2, W + "the stepper has " + std::to_string(Tend->NTracers) +
                                          " tracers: the column pass needs temperature and salinity (tracers 0 and 1)");
}

void SplitExplicitStepper::requirePressureGradShares(const ColumnPass &C, const std::string &Class, const std::string &W,
                                                     const char *Tail) const {
   if (const PressureGrad *P = Tend->pressureGrad()) // two column passes on two sets of column fields: refused
      OMEGA_REQUIRE(C.VCoord == P->VCoord && C.EqState == P->EqState,
                    W + "the " + Class + " and the PressureGrad attached to the Tendencies are on different VertCoord " +
                        "or Eos objects: both run the column pass, on one set of column fields" + Tail);
}

void SplitExplicitStepper::requireGentMcWilliamsFits(const GentMcWilliams *G, const char *Where) const {
   const std::string W = std::string(Where) + ": ";
   requireColumnPassFits(*G, "GentMcWilliams", W);
   requirePressureGradShares(*G, "GentMcWilliams", W, ", and keeping their forcing arrays equal is the caller's responsibility");
}

void SplitExplicitStepper::attachGentMcWilliams(GentMcWilliams *G) {
   if (G == nullptr) {
      GM = nullptr;
      return;
   }
   OMEGA_REQUIRE(Tend && Mesh && Trc, "SplitExplicitStepper::attachGentMcWilliams: attachData first");
   requireGentMcWilliamsFits(G, "SplitExplicitStepper::attachGentMcWilliams");
   GM = G;
}

void SplitExplicitStepper::requireRediFits(const Redi *R, const char *Where) const {
   const std::string W = std::string(Where) + ": ";
   requireColumnPassFits(*R, "Redi", W);
   OMEGA_REQUIRE(R->MaxTracers >= Tend->NTracers, W + "the Redi has MaxTracers = " + std::to_string(R->MaxTracers) +
                                                      ", below the stepper's " + std::to_string(Tend->NTracers) + " tracers");
   if (GM) // one column pass, on one set of column fields
      OMEGA_REQUIRE(R->VCoord == GM->VCoord && R->EqState == GM->EqState,
                    W + "the Redi and the attached GentMcWilliams are on different VertCoord or Eos objects: the step "
                        "runs one column pass for both");
   requirePressureGradShares(*R, "Redi", W, "");
   OMEGA_REQUIRE(VMixStep != nullptr, W + "the stepper has no VertMixStep attached: without the implicit S.S term of the "
                                          "vertical mixing the explicit part of the isoneutral tensor is indefinite");
   OMEGA_REQUIRE(VMixStep->redi() == R, W + "the stepper's VertMixStep does not have this Redi attached "
                                            "(VertMixStep::attachRedi): the implicit S.S term would be missing");
}

void SplitExplicitStepper::attachRedi(Redi *R) {
   if (R == nullptr) {
      RediTerm = nullptr;
      return;
   }
   OMEGA_REQUIRE(Tend && Mesh && Trc, "SplitExplicitStepper::attachRedi: attachData first");
   requireRediFits(R, "SplitExplicitStepper::attachRedi");
   RediTerm = R;
}

void SplitExplicitStepper::requireVertRemapFits(const VertRemap *R, const char *Where) const {
   const std::string W = std::string(Where) + ": ";
   OMEGA_REQUIRE(R->Mesh == Mesh && R->NVertLayers == Tend->LayerThicknessTend.Ext[1],
                 W + "the VertRemap was built for another mesh or layer count");
   OMEGA_REQUIRE(R->MaxTracers >= Tend->NTracers, W + "the VertRemap has MaxTracers = " + std::to_string(R->MaxTracers) +
                                                      ", below the stepper's " + std::to_string(Tend->NTracers) + " tracers");
   OMEGA_REQUIRE(Tend->vertAdv() == nullptr,
                 W + "a VertAdv is attached to the Tendencies: its vertical transport and the VertRemap would both hold "
                     "the layers to the coordinate; detach one of them");
}

void SplitExplicitStepper::attachVertRemap(VertRemap *R) {
   if (R == nullptr) {
      Remap = nullptr;
      return;
   }
   OMEGA_REQUIRE(Tend && Mesh && Trc, "SplitExplicitStepper::attachVertRemap: attachData first");
   requireVertRemapFits(R, "SplitExplicitStepper::attachVertRemap");
   Remap = R;
}

void SplitExplicitStepper::doStep(OceanState *State, hipStream_t S) {
   OMEGA_REQUIRE(Btr != nullptr, "Split-Explicit doStep: no BarotropicMode is attached: attachBarotropic first");
   if (Mono)
      requireMonotoneAdvFits(Mono, "Split-Explicit doStep");
   if (GM)
      requireGentMcWilliamsFits(GM, "Split-Explicit doStep");
   if (RediTerm)
      requireRediFits(RediTerm, "Split-Explicit doStep");
   if (Remap)
      requireVertRemapFits(Remap, "Split-Explicit doStep");
   requireHealthyWire();
   const int CurLevel = 0, NextLevel = 1;
   const StepArrays A = stepArrays("Split-Explicit", State);
   const R8 Dt = coeff(1.0);
   const R8 T0 = simTime();
   // R^{n} = RHS(u^{n}, h^{n}, phi^{n}, t^{n}); its velocity part is kept
   Tend->ModelTime = T0;
   if (UseMomentumRHS) // (steps 6-7 write the other two tendencies)
      Tend->computeMomentumTendencies(State, AuxState, A.CurTr, CurLevel, CurLevel, S);
   else
      Tend->computeAllTendencies(State, AuxState, A.CurTr, CurLevel, CurLevel, S);
   // the 2-D system over the step, forced by the mean of R_u^{n} less what the sub-steps compute themselves
   Btr->splitVelocityAndSSH(A.CurH, A.CurU, S);
   Btr->computeResidualForcing(A.CurH, Tend->NormalVelocityTend, S);
   Btr->subcycle(NSub, Dt / (R8)NSub, S);
   // h^{n+1} and phi^{n+1} by the transporting velocity: baroclinic u^{n} + the sub-cycle's mean flux over the thickness
   Btr->transportVelocity(A.CurU, A.NextU, S);
   if (GM) { // ... plus the eddy-induced velocity of the stratification of h^{n}, phi^{n}
      GM->updateColumn(A.CurH, A.CurTr, S);
      GM->computeBolusVelocity(A.CurH, A.NextU, S);
   }
   if (RediTerm) { // the isopycnal slopes of the same stratification: the column pass is GM's where it has just run
      if (!GM)
         RediTerm->updateColumn(A.CurH, A.CurTr, S);
      RediTerm->computeSlope(A.CurH, S);
   }
   // (with tracers and their hyperdiffusion term off the tracer update rides in the first transport launch, which loses a
   // wave to it: measured no faster than the three calls, DESIGN.md section 4.9, so those run)
   const bool Fold = UseFusedTransport && FoldUpdates && (Tend->NTracers <= 0 || Tend->Params.TracerHyperDiffTendencyEnable);
   if (Mono || RediTerm) {
      // the limiter needs h^{n+1} and the tracer tendency's other terms: both tendencies, the thickness update, the
      // limited flux divergence onto TracerTend, the tracer update; the isoneutral term joins TracerTend the same way
      if (UseFusedTransport)
         Tend->computeTransportTendencies(State, AuxState, A.CurTr, CurLevel, NextLevel, S);
      else {
         Tend->computeThicknessTendencies(State, AuxState, CurLevel, NextLevel, S);
         Tend->computeTracerTendencies(State, AuxState, A.CurTr, CurLevel, NextLevel, S);
      }
      updateThicknessByTend(State, NextLevel, State, CurLevel, Dt, S);
      if (Mono && Tend->NTracers > 0)
         Mono->addTracerTend(Tend->TracerTend, A.CurH, A.NextH, A.NextU, A.CurTr, Tend->NTracers, Dt, S);
      if (RediTerm)
         RediTerm->addTracerTend(Tend->TracerTend, A.CurH, A.CurTr, Tend->NTracers, S);
      updateTracersByTend(A.NextTr, A.CurTr, State, NextLevel, State, CurLevel, Dt, S);
   } else if (Fold) {
      // both tendencies and both updates in the transport kernels; the tendencies are stored as the calls below do
      Tend->computeTransportTendenciesAndUpdate(State, AuxState, A.CurTr, CurLevel, NextLevel, A.NextH, A.NextTr, Dt, true, S);
   } else if (UseFusedTransport) {
      // both tendencies first: the tracer tendency reads h^{n} and the transporting velocity, neither of which the
      // thickness update writes, so the order of the three calls below is free
      Tend->computeTransportTendencies(State, AuxState, A.CurTr, CurLevel, NextLevel, S);
      updateThicknessByTend(State, NextLevel, State, CurLevel, Dt, S);
      updateTracersByTend(A.NextTr, A.CurTr, State, NextLevel, State, CurLevel, Dt, S);
   } else {
      Tend->computeThicknessTendencies(State, AuxState, CurLevel, NextLevel, S);
      updateThicknessByTend(State, NextLevel, State, CurLevel, Dt, S);
      Tend->computeTracerTendencies(State, AuxState, A.CurTr, CurLevel, NextLevel, S);
      updateTracersByTend(A.NextTr, A.CurTr, State, NextLevel, State, CurLevel, Dt, S);
   }
   // u^{n+1} = (baroclinic u^{n} + Dt*(R_u^{n} - its mean)) + the barotropic velocity the sub-cycle ended with
   Btr->advanceVelocity(A.CurU, Tend->NormalVelocityTend, Dt, A.NextU, S);
   if (Remap) // the Lagrangian column back onto the coordinate's target grid, before the mixing sees it
      Remap->remap(A.NextH, A.NextU, A.NextTr, Tend->NTracers, S);
   mixNewLevel(State, S);
   updateTimeLevels(State, S);
   ++NStepsDone;
}

} // namespace OMEGA
