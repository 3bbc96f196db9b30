// RK4StagePlan.h -- what one stage of the stage-fused RungeKutta4 step does about the halo.  A pure function, free of
// HIP, so a host compiler builds it (tests/native/stage_plan_test.cpp); RungeKutta4Stepper.cpp turns the plan into a
// StageUpdate (kernels/Kernels.h) with the mesh's halo-layer bounds and the arrays' pointers.
#ifndef OMEGA_AMD_RK4STAGEPLAN_H
#define OMEGA_AMD_RK4STAGEPLAN_H

namespace OMEGA {

struct RK4StagePlan {
   static constexpr int NStages = 4;
   enum Output { None, Provis, New };
   /// the halo layer through which the level-3 tracer and velocity sweeps and the merged level-1 sweep go (layers are
   /// prefixes of the local numbering: owned, layer 1, 2, ...); 0 = every local cell
   int TrLayer = 0, VelLayer = 0, L1Layer = 0;
   /// exchanged after this stage: the provisional state, the next stage's input, after stage 1
   /// (RungeKutta4Stepper.cpp:107-113 "depends on halo width"), the new state after the last (:130-131)
   Output ExchangeAfter     = None;
   bool HaloOutputsReplaced = false; ///< that exchange replaces every halo element the stage writes (StageUpdate)
   bool BandOnComm = false; ///< it starts when the band is final; the band runs on the communication stream before it
};

/// Exchanges: the halo has neighbours; Overlap: ... and the exchange is overlapped with the stage's interior work.
///
/// How far the sweeps of a stage have to go.  An evaluation reaches two cells far (the del4 terms), so with the input
/// valid on every layer:
///  * a stage whose output is exchanged at once (overlapped: stage 1, last) is read on owned elements only: level 3
///    runs on the send band + interior, level 1 through layer 2 (level 2 keeps its full sweeps);
///  * the stage before it (0, 2) feeds that evaluation: tracers through layer 2, and every edge of those cells --
///    finished in the thread of the edge's second cell -- through layer 3.  Only at HaloWidth >= 4, where these
///    layers are valid at all; at the reference's default 3 the outer layers' values enter the next evaluation as
///    they are (RungeKutta4Stepper.cpp:107 "depends on halo width"), so nothing is left out there.
/// Stored stage tendencies keep their halo values: every sweep is full then and no halo cell is skipped.
///
///                      stage 0, 2                        stage 1 (Provis), 3 (New)
///    no neighbours     all, nothing exchanged            all, nothing exchanged
///    sequential        width >= 4: Tr 2, Vel 3           all; exchanged on the compute stream after the stage
///    overlapped        width >= 4: Tr 2, Vel 3           width >= 3: L1 2; replaced, band on the communication stream
inline RK4StagePlan rk4StagePlan(int Stage, bool Exchanges, bool Overlap, int HaloWidth, bool StoreStageTendencies) {
   RK4StagePlan P;
   const bool Exchanged = Stage == 1 || Stage == RK4StagePlan::NStages - 1;
   if (Exchanges && Exchanged)
      P.ExchangeAfter = Stage == 1 ? RK4StagePlan::Provis : RK4StagePlan::New;
   P.BandOnComm = Exchanges && Overlap && Exchanged;
   if (StoreStageTendencies)
      return P;
   P.HaloOutputsReplaced = P.BandOnComm;
   if (Exchanges && !Exchanged && HaloWidth >= 4)
      P.TrLayer = 2, P.VelLayer = 3;
   if (P.BandOnComm && HaloWidth >= 3)
      P.L1Layer = 2;
   return P;
}

} // namespace OMEGA
#endif
