// stage_plan_test.cpp -- prints the halo plan of every stage of the stage-fused RungeKutta4 step
// (omega_amd/csrc/RK4StagePlan.h) for the three exchange modes and the halo widths 2, 3 and 4, one row per case:
//    <mode> <width> <stage> <TrLayer> <VelLayer> <L1Layer> <exchanged output> <HaloOutputsReplaced> <BandOnComm>
// Host compiler only, no GPU: tests/test_rk4_stage_plan.py compares the rows with a table written out by hand.
#include "RK4StagePlan.h"

#include <cstdio>

int main() {
   const char *Modes[3]   = {"none", "sequential", "overlapped"};
   const char *Outputs[3] = {"none", "provis", "new"};
   for (int Mode = 0; Mode < 3; ++Mode)
      for (int Width = 2; Width <= 4; ++Width)
         for (int Stage = 0; Stage < OMEGA::RK4StagePlan::NStages; ++Stage) {
            const OMEGA::RK4StagePlan P = OMEGA::rk4StagePlan(Stage, Mode >= 1, Mode == 2, Width, false);
            std::printf("%s %d %d %d %d %d %s %d %d\n", Modes[Mode], Width, Stage, P.TrLayer, P.VelLayer, P.L1Layer,
                        Outputs[P.ExchangeAfter], (int)P.HaloOutputsReplaced, (int)P.BandOnComm);
         }
   return 0;
}
