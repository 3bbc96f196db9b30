// TimeStepper.cpp -- see TimeStepper.h.
#include "TimeStepper.h"
#include "Pacer.h"
#include "SplitExplicitStepper.h"
#include "VertMixStep.h"

namespace OMEGA {

R8 TimeStepper::coeffSeconds(R8 Mult, R8 TimeStepSeconds) {
   // (Real * TimeInterval, then TimeInterval::get(seconds): TimeStepper.cpp:392-393)
   return (TimeFrac::fromSeconds(TimeStepSeconds) * Mult).getSeconds();
}

TimeStepper::TimeStepper(const std::string &Name_, TimeStepperType Type_, int NTimeLevels_, R8 Dt)
    : Name(Name_), Type(Type_), NTimeLevels(NTimeLevels_), TimeStep(Dt, TimeUnits::Seconds), TimeStepSeconds(Dt) {
   OMEGA_REQUIRE(Dt > 0, "TimeStepper: time step must be positive");
}

// TimeStepper.h:82-84.  The model time of the stages is SimTime + RKC * TimeStep in the reference; here the schemes
// derive it from StartTime + NStepsDone * TimeStep, so the step is anchored at SimTime first.
void TimeStepper::doStep(OceanState *State, TimeInstant &SimTime) const {
   TimeStepper *Self = const_cast<TimeStepper *>(this);
   Self->StartTime   = SimTime.getSeconds();
   Self->NStepsDone  = 0;
   Self->doStep(State, Stream);
   SimTime += TimeStep;
}

TimeStepperType TimeStepper::getFromStr(const std::string &In) {
   if (In == "Forward-Backward")
      return TimeStepperType::ForwardBackward;
   if (In == "RungeKutta4")
      return TimeStepperType::RungeKutta4;
   if (In == "RungeKutta2")
      return TimeStepperType::RungeKutta2;
   if (In == "Split-Explicit")
      return TimeStepperType::SplitExplicit;
   return TimeStepperType::Invalid;
}

namespace {
std::map<std::string, std::unique_ptr<TimeStepper>> &allSteppers() {
   static std::map<std::string, std::unique_ptr<TimeStepper>> M;
   return M;
}
} // namespace
TimeStepper *TimeStepper::create(const std::string &Name, TimeStepperType Type, R8 Dt, Tendencies *T, AuxiliaryState *A,
                                 const HorzMesh *M, Halo *H, TracerStore *Tr) {
   auto &All = allSteppers();
   if (All.find(Name) != All.end())
      return nullptr;
   TimeStepper *St = make(Name, Type, Dt);
   All[Name].reset(St);
   St->attachData(T, A, M, H, Tr);
   St->finalizeInit();
   return St;
}
TimeStepper *TimeStepper::get(const std::string &Name) {
   auto It = allSteppers().find(Name);
   return It == allSteppers().end() ? nullptr : It->second.get();
}
void TimeStepper::erase(const std::string &Name) { allSteppers().erase(Name); }
void TimeStepper::clear() { allSteppers().clear(); }

TimeStepper *TimeStepper::make(const std::string &Name, TimeStepperType Type, R8 Dt) {
   switch (Type) {
   case TimeStepperType::ForwardBackward:
      return new ForwardBackwardStepper(Name, Dt);
   case TimeStepperType::RungeKutta4:
      return new RungeKutta4Stepper(Name, Dt);
   case TimeStepperType::RungeKutta2:
      return new RungeKutta2Stepper(Name, Dt);
   case TimeStepperType::SplitExplicit:
      return new SplitExplicitStepper(Name, Dt);
   default:
      OMEGA_ABORT("TimeStepper::make: unknown time stepper type");
   }
}

void TimeStepper::attachData(Tendencies *T, AuxiliaryState *A, const HorzMesh *M, Halo *H, TracerStore *Tr) {
   Tend     = T;
   AuxState = A;
   Mesh     = M;
   MeshHalo = H;
   Trc      = Tr ? Tr : Tracers::getDefault();
}

void TimeStepper::finalizeInit() {
   if (MeshHalo && MeshHalo->NNghbr > 0 && Tend)
      MeshHalo->reserveState(Tend->LayerThicknessTend, Tend->NormalVelocityTend, Tend->NTracers > 0 ? &Tend->TracerTend : nullptr,
                             Tend->NTracers);
}

void TimeStepper::attachVertMix(VertMixStep *Mix) {
   if (Mix) {
      OMEGA_REQUIRE(Tend && Mesh && Trc, "TimeStepper::attachVertMix: attachData first");
      OMEGA_REQUIRE(Mix->Mesh == Mesh && Mix->NVertLayers == Tend->LayerThicknessTend.Ext[1],
                    "TimeStepper::attachVertMix: the VertMixStep was built for another mesh or layer count");
      OMEGA_REQUIRE(Mix->NTracers == Trc->NTracers,
                    "TimeStepper::attachVertMix: the VertMixStep was built for another tracer count");
      OMEGA_REQUIRE(!MeshHalo || MeshHalo->NNghbr == 0,
                    "TimeStepper::attachVertMix: this stepper's halo has neighbours: multi-rank mixing needs the halo of "
                    "the new level before and after the solve and is not built");
   }
   VMixStep = Mix;
}

void TimeStepper::mixNewLevel(OceanState *State, hipStream_t S) const {
   if (VMixStep)
      VMixStep->apply(State, 1, Trc, 1, TimeStepSeconds, S);
}

// ---- update kernels ----
void TimeStepper::updateThicknessByTend(OceanState *S1, int L1, OceanState *S2, int L2, R8 C, hipStream_t S) const {
   Array2DReal H1, H2;
   OMEGA_REQUIRE(S1->getLayerThickness(H1, L1) == 0 && S2->getLayerThickness(H2, L2) == 0,
                 "TimeStepper updateThickness: error retrieving layer thick");
   launchUpdateByTend(Mesh->NCellsAll, H1.Pitch, H1.Ptr, H2.Ptr, Tend->LayerThicknessTend.Ptr, C, S);
}
void TimeStepper::updateVelocityByTend(OceanState *S1, int L1, OceanState *S2, int L2, R8 C, hipStream_t S) const {
   Array2DReal U1, U2;
   OMEGA_REQUIRE(S1->getNormalVelocity(U1, L1) == 0 && S2->getNormalVelocity(U2, L2) == 0,
                 "TimeStepper updateVelocity: error retrieving velocity");
   launchUpdateByTend(Mesh->NEdgesAll, U1.Pitch, U1.Ptr, U2.Ptr, Tend->NormalVelocityTend.Ptr, C, S);
}
void TimeStepper::updateStateByTend(OceanState *S1, int L1, OceanState *S2, int L2, R8 C, hipStream_t S) const {
   updateThicknessByTend(S1, L1, S2, L2, C, S);
   updateVelocityByTend(S1, L1, S2, L2, C, S);
}
void TimeStepper::updateTracersByTend(const Array3DReal &Next, const Array3DReal &Cur, OceanState *S1, int L1,
                                      OceanState *S2, int L2, R8 C, hipStream_t S) const {
   Array2DReal H1, H2;
   OMEGA_REQUIRE(S1->getLayerThickness(H1, L1) == 0 && S2->getLayerThickness(H2, L2) == 0,
                 "TimeStepper updateTracers: error retrieving layer thick");
   launchUpdateTracersByTend(Trc ? Trc->NTracers : 0, Mesh->NCellsAll, Mesh->NCellsSize, H1.Pitch, Next.Ptr, Cur.Ptr,
                             H1.Ptr, H2.Ptr, Tend->TracerTend.Ptr, C, S);
}
void TimeStepper::weightTracers(const Array3DReal &Next, const Array3DReal &Cur, OceanState *St, int L1,
                                hipStream_t S) const {
   Array2DReal H;
   OMEGA_REQUIRE(St->getLayerThickness(H, L1) == 0, "TimeStepper weightTracers: bad time level");
   launchWeightTracers(Trc ? Trc->NTracers : 0, Mesh->NCellsAll, Mesh->NCellsSize, H.Pitch, Next.Ptr, Cur.Ptr, H.Ptr,
                       S);
}
void TimeStepper::accumulateTracersUpdate(const Array3DReal &Accum, R8 C, hipStream_t S) const {
   launchAccumulateTracers(Trc ? Trc->NTracers : 0, Mesh->NCellsAll, Mesh->NCellsSize, Accum.Pitch, Accum.Ptr,
                           Tend->TracerTend.Ptr, C, S);
}
void TimeStepper::finalizeTracersUpdate(const Array3DReal &Next, OceanState *St, int L, hipStream_t S) const {
   Array2DReal H;
   OMEGA_REQUIRE(St->getLayerThickness(H, L) == 0, "TimeStepper finalizeTracers: bad time level");
   launchFinalizeTracers(Trc ? Trc->NTracers : 0, Mesh->NCellsAll, Mesh->NCellsSize, H.Pitch, Next.Ptr, H.Ptr, S);
}

void TimeStepper::requireHealthyWire() const {
   OMEGA_REQUIRE(!MeshHalo || MeshHalo->checkWire() == 0,
                 "TimeStepper: a halo exchange of an earlier step failed" + MeshHalo->wireError());
}

TimeStepper::StepArrays TimeStepper::stepArrays(const char *Scheme, OceanState *State) const {
   StepArrays A;
   OMEGA_REQUIRE(Trc->getAll(A.CurTr, 0) == 0 && Trc->getAll(A.NextTr, 1) == 0,
                 Scheme + std::string(" doStep: error retrieving tracers"));
   if (State)
      OMEGA_REQUIRE(State->getLayerThickness(A.CurH, 0) == 0 && State->getNormalVelocity(A.CurU, 0) == 0 &&
                        State->getLayerThickness(A.NextH, 1) == 0 && State->getNormalVelocity(A.NextU, 1) == 0,
                    Scheme + std::string(" doStep: error retrieving the state"));
   return A;
}

void TimeStepper::exchangeState(OceanState *State, int Level, const Array3DReal *Tr, hipStream_t S, const char *TimerName,
                                const char *ErrorPrefix) const {
   Array2DReal H, U;
   State->getLayerThickness(H, Level);
   State->getNormalVelocity(U, Level);
   const int NT = Trc ? Trc->NTracers : 0;
   Pacer::Range Timer(TimerName, 3);
   OMEGA_REQUIRE(MeshHalo->exchangeState(H, U, NT > 0 ? Tr : nullptr, NT, S) == 0, ErrorPrefix + MeshHalo->wireError());
}

void TimeStepper::updateTimeLevels(OceanState *State, hipStream_t S) const {
   if (MeshHalo && MeshHalo->NNghbr > 0) {
      Array3DReal Tr;
      if (Trc && Trc->NTracers > 0)
         Trc->getAll(Tr, 1);
      // (the reference's name for this exchange: "RK4:haloExch" / "RK2:haloExch" / "ForwardBackward:haloExch", level 3)
      exchangeState(State, 1, &Tr, S,
                    Type == TimeStepperType::RungeKutta4   ? "RK4:haloExch"
                    : Type == TimeStepperType::RungeKutta2 ? "RK2:haloExch"
                                                           : "ForwardBackward:haloExch",
                    "TimeStepper: halo exchange failed");
   }
   State->rotateTimeLevels();
   if (Trc)
      Trc->rotateTimeLevels();
}

// ---- ForwardBackwardStepper::doStep (ForwardBackwardStepper.cpp:27-82) ----
void ForwardBackwardStepper::doStep(OceanState *State, hipStream_t S) {
   requireHealthyWire();
   const int CurLevel = 0, NextLevel = 1;
   const StepArrays A = stepArrays("ForwardBackward");
   const R8 Dt = coeff(1.0);
   const R8 T0 = simTime();
   // R_h^{n} = RHS_h(u^{n}, h^{n}, t^{n});  h^{n+1} = h^{n} + R_h^{n}
   Tend->ModelTime = T0;
   Tend->computeThicknessTendencies(State, AuxState, CurLevel, CurLevel, S);
   updateThicknessByTend(State, NextLevel, State, CurLevel, Dt, S);
   // R_phi^{n};  phi^{n+1} = (phi^{n} * h^{n} + R_phi^{n}) / h^{n+1}
   Tend->computeTracerTendencies(State, AuxState, A.CurTr, CurLevel, CurLevel, S);
   updateTracersByTend(A.NextTr, A.CurTr, State, NextLevel, State, CurLevel, Dt, S);
   // R_u^{n+1} = RHS_u(u^{n}, h^{n+1}, t^{n+1});  u^{n+1} = u^{n} + R_u^{n+1}
   Tend->ModelTime = T0 + Dt;
   Tend->computeVelocityTendencies(State, AuxState, NextLevel, CurLevel, S);
   updateVelocityByTend(State, NextLevel, State, CurLevel, Dt, S);
   mixNewLevel(State, S);
   updateTimeLevels(State, S);
   ++NStepsDone;
}

// ---- RungeKutta2Stepper::doStep (RungeKutta2Stepper.cpp:27-73) ----
void RungeKutta2Stepper::doStep(OceanState *State, hipStream_t S) {
   requireHealthyWire();
   const int CurLevel = 0, NextLevel = 1;
   const StepArrays A = stepArrays("RungeKutta2");
   const R8 Half = coeff(0.5), Full = coeff(1.0);
   const R8 T0 = simTime();
   Tend->ModelTime = T0;
   Tend->computeAllTendencies(State, AuxState, A.CurTr, CurLevel, CurLevel, S);
   updateStateByTend(State, NextLevel, State, CurLevel, Half, S);
   updateTracersByTend(A.NextTr, A.CurTr, State, NextLevel, State, CurLevel, Half, S);
   Tend->ModelTime = T0 + Half;
   Tend->computeAllTendencies(State, AuxState, A.NextTr, NextLevel, NextLevel, S);
   updateStateByTend(State, NextLevel, State, CurLevel, Full, S);
   updateTracersByTend(A.NextTr, A.CurTr, State, NextLevel, State, CurLevel, Full, S);
   mixNewLevel(State, S);
   updateTimeLevels(State, S);
   ++NStepsDone;
}

} // namespace OMEGA
