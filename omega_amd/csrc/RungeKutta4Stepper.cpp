// RungeKutta4Stepper.cpp -- the RungeKutta4 scheme of TimeStepper.h (RungeKutta4Stepper.cpp:17-137): the plain stage
// sequence, and the stage-fused form with its overlapped halo exchange and its graph replay.
#include "RK4StagePlan.h"
#include "TimeStepper.h"

namespace OMEGA {

static_assert(RK4StagePlan::NStages == 4, "RK4StagePlan.h plans the four stages of RungeKutta4Stepper");

// The overlapped exchange of a stage's output: the communication stream and the "band is final" / "halo is in place" /
// "everything queued so far" events.  Made by finalizeInit when the halo has neighbours, so a step creates nothing.
class RungeKutta4Stepper::HaloOverlap {
 public:
   /// what StageUpdate::AfterBand is handed: the output whose band is final on stream S
   struct Job {
      HaloOverlap *Self;
      const RungeKutta4Stepper *Stepper;
      hipStream_t S;
      OceanState *State;
      int Level;
      const Array3DReal *Tr;
      bool Provis; ///< the mid-step exchange of the provisional state (timer "RK4:haloExchProvis")
   };
   hipStream_t CommStream = nullptr;
   hipEvent_t EvFork      = nullptr; ///< StageUpdate::BandReady

   HaloOverlap() {
      // the highest priority the device offers: the band launches and the pack / unpack kernels on this stream are
      // small and everything else waits for them, the interior launch next to them fills the GPU for much longer
      int Least = 0, Greatest = 0;
      HIP_CHECK(hipDeviceGetStreamPriorityRange(&Least, &Greatest));
      HIP_CHECK(hipStreamCreateWithPriority(&CommStream, hipStreamNonBlocking, Greatest));
      HIP_CHECK(hipEventCreateWithFlags(&EvBand, hipEventDisableTiming));
      HIP_CHECK(hipEventCreateWithFlags(&EvDone, hipEventDisableTiming));
      HIP_CHECK(hipEventCreateWithFlags(&EvFork, hipEventDisableTiming));
      noteDeviceResource(4);
   }
   HaloOverlap(const HaloOverlap &) = delete;
   ~HaloOverlap() {
      (void)hipEventDestroy(EvBand);
      (void)hipEventDestroy(EvDone);
      (void)hipEventDestroy(EvFork);
      (void)hipStreamDestroy(CommStream);
   }

   static void startThunk(void *J) { static_cast<Job *>(J)->Self->start(*static_cast<Job *>(J)); }
   // Called by the RHS launcher between the band and the interior part of a stage: everything a neighbour
   // receives is final on stream S.  Pack, send / receive and unpack run on the communication stream.
   void start(const Job &J) {
      HIP_CHECK(hipEventRecord(EvBand, J.S));
      HIP_CHECK(hipStreamWaitEvent(CommStream, EvBand, 0));
      J.Stepper->exchangeState(J.State, J.Level, J.Tr, CommStream, J.Provis ? "RK4:haloExchProvis" : "RK4:haloExch",
                               "RungeKutta4: overlapped halo exchange failed");
      HIP_CHECK(hipEventRecord(EvDone, CommStream));
      Pending = true;
   }
   /// the next consumer of the exchanged halo, on stream S, waits for it
   void join(hipStream_t S) {
      if (Pending)
         HIP_CHECK(hipStreamWaitEvent(S, EvDone, 0));
      Pending = false;
   }

 private:
   hipEvent_t EvBand = nullptr, EvDone = nullptr;
   bool Pending      = false;
};

RungeKutta4Stepper::RungeKutta4Stepper(const std::string &Name, R8 Dt)
    : TimeStepper(Name, TimeStepperType::RungeKutta4, 2, Dt) {
   RKA[0] = 0, RKA[1] = 1. / 2, RKA[2] = 1. / 2, RKA[3] = 1;
   RKB[0] = 1. / 6, RKB[1] = 1. / 3, RKB[2] = 1. / 3, RKB[3] = 1. / 6;
   RKC[0] = 0, RKC[1] = 1. / 2, RKC[2] = 1. / 2, RKC[3] = 1;
}
RungeKutta4Stepper::~RungeKutta4Stepper() = default;

void RungeKutta4Stepper::finalizeInit() {
   OMEGA_REQUIRE(Tend && Mesh && Trc, "RungeKutta4Stepper: attachData before finalizeInit");
   const int K = Tend->LayerThicknessTend.Ext[1];
   const int NT = Trc->NTracers;
   ProvisState.reset(new OceanState("Provis" + Name, Mesh, MeshHalo, K, 1)); // 1 time level (:56-60)
   ProvisTracers = Array3DReal::levels("ProvisTracers", NT > 0 ? NT : 1, Mesh->NCellsSize, K);
   // Everything a step needs is created here, as the reference does (RungeKutta4Stepper.cpp:43-64), never inside doStep:
   // the second provisional buffer of the stage-fused form, and with neighbours the communication stream, its events and
   // the halo's job tables and message buffers for the state exchange (h + u + tracers in one message per neighbour).
   ProvisState2.reset(new OceanState("Provis2" + Name, Mesh, MeshHalo, K, 1));
   ProvisTracers2 = Array3DReal::levels("ProvisTracers2", NT > 0 ? NT : 1, Mesh->NCellsSize, K);
   if (MeshHalo && MeshHalo->NNghbr > 0 && !Overlap)
      Overlap.reset(new HaloOverlap);
   TimeStepper::finalizeInit();
}

// The same scheme with every stage's updates applied in the epilogue of the kernels that produce
// the tendencies.  Stage s computes R = RHS(q_in) and, element by element,
//    q^{n+1} (+)= RKB[s]*dt*R          (first stage: = q^n + ..., tracers thickness-weighted)
//    q_out     = q^n + RKA[s+1]*dt*R   (the next stage's input; tracers divided by the new thickness)
// which is what weightTracers / updateStateByTend / accumulateTracersUpdate / updateTracersByTend /
// finalizeTracersUpdate do in separate sweeps.  q_in and q_out alternate between two buffers.
// Returns false when the first stage was refused: nothing has been touched, the caller runs the plain sequence.
bool RungeKutta4Stepper::runStages(OceanState *State, const StepArrays &A, hipStream_t S) {
   const int CurLevel = 0, NextLevel = 1;
   OceanState *Prov[2]   = {ProvisState.get(), ProvisState2.get()};
   Array3DReal *ProvT[2] = {&ProvisTracers, &ProvisTracers2};
   const bool Exchanges  = MeshHalo && MeshHalo->NNghbr > 0;
   const bool Overlapped = Exchanges && OverlapHaloExchange;
   const int HaloW       = (int)Mesh->NCellsHaloH.size();
   auto Through          = [&](int Layer) { return Layer ? Mesh->NCellsHaloH(Layer - 1) : 0; }; // 0 = all local cells
   for (int Stage = 0; Stage < NStages; ++Stage) {
      const RK4StagePlan Plan = rk4StagePlan(Stage, Exchanges, Overlapped, HaloW, StoreStageTendencies);
      OceanState *In          = Stage == 0 ? State : Prov[(Stage - 1) % 2];
      const Array3DReal &InTr = Stage == 0 ? A.CurTr : *ProvT[(Stage - 1) % 2];
      OceanState *Out         = Prov[Stage % 2];
      Array3DReal *OutTr      = ProvT[Stage % 2];
      Array2DReal OutH, OutU;
      Out->getLayerThickness(OutH, CurLevel), Out->getNormalVelocity(OutU, CurLevel);
      StageUpdate Su;
      Su.CB        = coeff(RKB[Stage]);
      Su.CA        = Stage + 1 < NStages ? coeff(RKA[Stage + 1]) : 0.0;
      Su.First     = Stage == 0;
      Su.Last      = Stage == NStages - 1;
      Su.StoreTend = StoreStageTendencies ? 1 : 0;
      Su.NextH = A.NextH.Ptr, Su.NextU = A.NextU.Ptr, Su.NextTr = A.NextTr.Ptr;
      Su.CurH = A.CurH.Ptr, Su.CurU = A.CurU.Ptr, Su.CurTr = A.CurTr.Ptr;
      Su.ProvH = OutH.Ptr, Su.ProvU = OutU.Ptr, Su.ProvTr = OutTr->Ptr;
      Su.NCellsTr = Through(Plan.TrLayer), Su.NCellsVel = Through(Plan.VelLayer), Su.NCellsL1 = Through(Plan.L1Layer);
      Su.HaloOutputsReplaced = Plan.HaloOutputsReplaced;
      HaloOverlap::Job Job{Overlap.get(), this, S, Out, CurLevel, OutTr, true};
      if (Plan.ExchangeAfter == RK4StagePlan::New)
         Job.State = State, Job.Level = NextLevel, Job.Tr = &A.NextTr, Job.Provis = false;
      if (Plan.BandOnComm) { // the exchange starts when the band is final; the band launches go where it follows them
         Su.AfterBand = &HaloOverlap::startThunk, Su.AfterBandCtx = &Job;
         Su.BandStream = Overlap->CommStream, Su.BandReady = Overlap->EvFork;
      }
      const bool Ok = Tend->computeAllTendenciesStage(In, AuxState, InTr, CurLevel, CurLevel, Su, S);
      if (Stage == 0 && !Ok)
         return false;
      OMEGA_REQUIRE(Ok, "RungeKutta4: stage-fused RHS became unavailable mid-step");
      // the next stage reads the provisional halo: wait for the exchange this stage started, or make it now
      // (the new state's exchange is the end of the step: doStepFused)
      if (Plan.ExchangeAfter == RK4StagePlan::Provis) {
         if (Overlapped)
            Overlap->join(S);
         else
            exchangeState(Out, CurLevel, OutTr, S, "RK4:haloExchProvis", "RungeKutta4: provisional halo exchange failed");
      }
   }
   return true;
}

// everything that enters the launches of a stage-fused step on one rank
GraphCache::Key RungeKutta4Stepper::stepGraphKey(OceanState *State, const StepArrays &A, hipStream_t S) const {
   GraphCache::Key Key;
   GraphCache::add(Key, State), GraphCache::add(Key, A.CurH.Ptr), GraphCache::add(Key, A.NextH.Ptr);
   GraphCache::add(Key, A.CurU.Ptr), GraphCache::add(Key, A.NextU.Ptr), GraphCache::add(Key, A.CurTr.Ptr);
   GraphCache::add(Key, A.NextTr.Ptr), GraphCache::add(Key, TimeStepSeconds), GraphCache::add(Key, (int)StoreStageTendencies);
   GraphCache::add(Key, Tend), GraphCache::add(Key, AuxState), GraphCache::add(Key, Tend->Params), GraphCache::add(Key, S);
   GraphCache::add(Key, (int)Tend->UseFusedRHS);
   GraphCache::add(Key, tuningGeneration()); // (the kernel structure options are read at every launch)
   GraphCache::add(Key, (int)AuxState->LayerThicknessAux.FluxThickEdgeChoice);
   GraphCache::add(Key, (int)AuxState->TracerAux.TracersOnEdgeChoice);
   GraphCache::add(Key, (int)AuxState->WindForcingAux.InterpChoice);
   return Key;
}

bool RungeKutta4Stepper::doStepFused(OceanState *State, hipStream_t S) {
   if (VMixStep) // the mixing sequence follows the plain stage sequence; nothing of it goes into a graph
      return false;
   const StepArrays A   = stepArrays("RungeKutta4", State);
   const bool Exchanges = MeshHalo && MeshHalo->NNghbr > 0;
   bool FirstStageOk    = true;
   if (!Exchanges && (UseGraphs || GraphCache::defaultOn()) && StageFusedKnownGood && !Tend->addsTermsAfterFusedRHS()) {
      // one rank: nothing but kernel launches on S -- replay them as a graph (keyed by everything that enters them)
      Graphs.run(stepGraphKey(State, A, S), S, [&]() { FirstStageOk = runStages(State, A, S); });
   } else {
      FirstStageOk = runStages(State, A, S);
   }
   if (!FirstStageOk)
      return false;
   StageFusedKnownGood = true;
   if (Exchanges && OverlapHaloExchange) { // the end-of-step exchange was started by the last stage: wait for it, then rotate
      Overlap->join(S);
      State->rotateTimeLevels();
      Trc->rotateTimeLevels();
   } else {
      updateTimeLevels(State, S);
   }
   ++NStepsDone;
   return true;
}

void RungeKutta4Stepper::doStep(OceanState *State, hipStream_t S) {
   if (!ProvisState)
      finalizeInit();
   // the one lazy creation: attachData can bring a Halo with neighbours after finalizeInit has run
   if (!Overlap && MeshHalo && MeshHalo->NNghbr > 0)
      Overlap.reset(new HaloOverlap);
   requireHealthyWire();
   if (FuseStageUpdates && doStepFused(State, S))
      return;
   const int CurLevel = 0, NextLevel = 1;
   const StepArrays A = stepArrays("RungeKutta4");
   const R8 T0        = simTime();
   for (int Stage = 0; Stage < NStages; ++Stage) {
      Tend->ModelTime = T0 + coeff(RKC[Stage]); // StageTime (:87)
      if (Stage == 0) {
         // R^{(0)} = RHS(q^{n}, t^{n});  q^{n+1} = q^{n} + dt * RKB[0] * R^{(0)}
         weightTracers(A.NextTr, A.CurTr, State, CurLevel, S);
         Tend->computeAllTendencies(State, AuxState, A.CurTr, CurLevel, CurLevel, S);
         updateStateByTend(State, NextLevel, State, CurLevel, coeff(RKB[Stage]), S);
         accumulateTracersUpdate(A.NextTr, coeff(RKB[Stage]), S);
      } else {
         // q^{provis} = q^{n} + RKA[stage]*dt*R^{(s-1)};  R^{(s)} = RHS(q^{provis});  q^{n+1} += RKB[stage]*dt*R^{(s)}
         updateStateByTend(ProvisState.get(), CurLevel, State, CurLevel, coeff(RKA[Stage]), S);
         updateTracersByTend(ProvisTracers, A.CurTr, ProvisState.get(), CurLevel, State, CurLevel, coeff(RKA[Stage]), S);
         if (Stage == 2 && MeshHalo && MeshHalo->NNghbr > 0) // depends on the halo width (:107-113)
            exchangeState(ProvisState.get(), CurLevel, &ProvisTracers, S, "RK4:haloExchProvis",
                          "RungeKutta4: provisional halo exchange failed");
         Tend->computeAllTendencies(ProvisState.get(), AuxState, ProvisTracers, CurLevel, CurLevel, S);
         updateStateByTend(State, NextLevel, State, NextLevel, coeff(RKB[Stage]), S);
         accumulateTracersUpdate(A.NextTr, coeff(RKB[Stage]), S);
      }
   }
   finalizeTracersUpdate(A.NextTr, State, NextLevel, S);
   mixNewLevel(State, S);
   updateTimeLevels(State, S);
   ++NStepsDone;
}

} // namespace OMEGA
