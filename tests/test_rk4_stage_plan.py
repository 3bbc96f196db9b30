"""The halo plan of the stage-fused RungeKutta4 step (omega_amd/csrc/RK4StagePlan.h) is a pure function that a host
compiler builds: tests/native/stage_plan_test.cpp prints it for every stage, exchange mode and halo width, and the rows
are compared with the table below.  No GPU.

The table was written out by hand from the stage loop as it stood before the plan was a function of its own:
  * stages 0 and 2 with neighbours at halo width >= 4: tracer sweeps through halo layer 2 (NCellsHaloH(1)), velocity
    sweeps through layer 3 (NCellsHaloH(2)); otherwise every local cell (0);
  * stages 1 and 3 with the overlapped exchange: the exchange starts at the band (band on the communication stream),
    every halo output is replaced, and at halo width >= 3 the level-1 sweep goes through layer 2 (NCellsHaloH(1));
  * with neighbours the provisional output of stage 1 is exchanged before stage 2 reads it and the new state after
    stage 3 (sequential: on the compute stream, by the stage loop and by updateTimeLevels)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")

# mode width stage TrLayer VelLayer L1Layer exchanged HaloOutputsReplaced BandOnComm
EXPECTED = """\
none 2 0 0 0 0 none 0 0
none 2 1 0 0 0 none 0 0
none 2 2 0 0 0 none 0 0
none 2 3 0 0 0 none 0 0
none 3 0 0 0 0 none 0 0
none 3 1 0 0 0 none 0 0
none 3 2 0 0 0 none 0 0
none 3 3 0 0 0 none 0 0
none 4 0 0 0 0 none 0 0
none 4 1 0 0 0 none 0 0
none 4 2 0 0 0 none 0 0
none 4 3 0 0 0 none 0 0
sequential 2 0 0 0 0 none 0 0
sequential 2 1 0 0 0 provis 0 0
sequential 2 2 0 0 0 none 0 0
sequential 2 3 0 0 0 new 0 0
sequential 3 0 0 0 0 none 0 0
sequential 3 1 0 0 0 provis 0 0
sequential 3 2 0 0 0 none 0 0
sequential 3 3 0 0 0 new 0 0
sequential 4 0 2 3 0 none 0 0
sequential 4 1 0 0 0 provis 0 0
sequential 4 2 2 3 0 none 0 0
sequential 4 3 0 0 0 new 0 0
overlapped 2 0 0 0 0 none 0 0
overlapped 2 1 0 0 0 provis 1 1
overlapped 2 2 0 0 0 none 0 0
overlapped 2 3 0 0 0 new 1 1
overlapped 3 0 0 0 0 none 0 0
overlapped 3 1 0 0 2 provis 1 1
overlapped 3 2 0 0 0 none 0 0
overlapped 3 3 0 0 2 new 1 1
overlapped 4 0 2 3 0 none 0 0
overlapped 4 1 0 0 2 provis 1 1
overlapped 4 2 2 3 0 none 0 0
overlapped 4 3 0 0 2 new 1 1
"""


def test_stage_plan_matches_the_table():
    subprocess.check_call(["make", "-C", NATIVE, "-s", "build/stage_plan_test"])
    out = subprocess.run([os.path.join(NATIVE, "build", "stage_plan_test")], capture_output=True, text=True, check=True).stdout
    assert out.splitlines() == EXPECTED.splitlines()
