"""Every tools/probes/*_diag.py at the smallest size it accepts, one fresh child process per case, one at a time.

Each case asserts: return code 0; exactly one JSON line on stdout and the same line in --out; the record's key tree
contains the golden key tree (tests/golden/probe_records_tiny.json); the golden's deterministic leaves -- those on which
two runs of the probes of the commit before tools/probes/probe_rig.py agreed exactly: counts, active levels, *_GB, finite
and bitwise flags, maxima such as slope_max_abs and bolus_max_abs, limited fractions, launch counts -- are equal bit for
bit.  A probe left half-converted, a random draw out of order or a lost key fails here.  (At two iterations a few
clock-made leaves agreed between the two runs too, a device tick being coarse: leaves named ms_*, *_ms and
*faster_by_more_than_the_spread are kept out of "equal" by name.  vert_mix_forcing_diag.py's record has nothing that is
not made by a clock beyond its arguments, the two counts and state_finite_after_steps: that case checks little more than
that the probe runs and keeps its keys.)

After a child that ends with 124, 134, 137, 139, -6 or -11, or that runs out its limit, the remaining cases skip: nothing
more is started on a card that may have faulted.

Time: measured on an MI355X at these arguments, around subprocess.run of the whole child (interpreter start, imports,
library load and device initialisation included), the probes of the commit before the rig took 0.39 to 0.53 s each,
WALL_MEASURED_S at the most; the sixteen cases of this module together take 8 s.  The limit of a child is LIMIT_S: that
times a generous factor for a cold import on a busy machine.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "probe_records_tiny.json")
WALL_MEASURED_S = 0.53
LIMIT_S = 60

MESH = ["--nx", "16", "--levels", "8"]
LOOP = ["--iters", "2", "--warmup", "1"]
NT = ["--tracers", "2"]
STEP = ["--nsub", "2"]
# the flags differ from probe to probe (column_diag.py has no --tracers, only the stepping probes have --nsub)
CASES = {
    "barotropic": ("barotropic_diag.py", MESH + NT + STEP + LOOP),
    "column": ("column_diag.py", MESH + LOOP),
    "gm": ("gm_diag.py", MESH + NT + LOOP),
    "momentum_update": ("momentum_update_diag.py", MESH + NT + STEP + LOOP),
    "monotone_adv_2d": ("monotone_adv_diag.py", ["--form", "2d"] + MESH + NT + STEP + LOOP),
    "monotone_adv_3d": ("monotone_adv_diag.py", ["--form", "3d"] + MESH + NT + STEP + LOOP),
    "monotone_adv_ho": ("monotone_adv_diag.py", ["--form", "ho"] + MESH + NT + STEP + LOOP),
    "pressure_grad": ("pressure_grad_diag.py", MESH + NT + LOOP),
    "redi": ("redi_diag.py", MESH + NT + STEP + LOOP),
    "split_explicit": ("split_explicit_diag.py", MESH + NT + STEP + LOOP),
    "transport": ("transport_diag.py", MESH + NT + STEP + LOOP),
    "tridiag": ("tridiag_diag.py", ["--sizes", "ref_500x64"] + LOOP),
    "vert_adv": ("vert_adv_diag.py", MESH + NT + LOOP),
    "vert_mix": ("vert_mix_diag.py", MESH + NT + LOOP),
    "vert_mix_forcing": ("vert_mix_forcing_diag.py", MESH + NT + LOOP),
    "vert_remap": ("vert_remap_diag.py", MESH + NT + STEP + LOOP),
}
BAD_EXITS = (124, 134, 137, 139, -6, -11)
_stopped = {"why": ""}


def run_probe(tools, case, out, limit=LIMIT_S):
    """one child process; -> (return code or None at the limit, stdout, stderr)"""
    script, args = CASES[case]
    cmd = [sys.executable, os.path.join(tools, "probes", script)] + args + ["--out", out]
    try:
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit)
    except subprocess.TimeoutExpired as e:
        return None, (e.stdout or b"").decode(), (e.stderr or b"").decode()
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def leaves(rec, path=()):
    """{key path: leaf} of a record; a dict is a node, everything else a leaf"""
    if not isinstance(rec, dict):
        return {"/".join(path): rec}
    out = {}
    for k, v in rec.items():
        assert "/" not in k
        out.update(leaves(v, path + (k,)))
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_probe_record(case, golden, tmp_path):
    if _stopped["why"]:
        pytest.skip(_stopped["why"])
    out = str(tmp_path / "record.json")
    rc, stdout, stderr = run_probe(os.path.join(ROOT, "tools"), case, out)
    if rc is None or rc in BAD_EXITS:
        _stopped["why"] = f"{case} ended with {'its time limit' if rc is None else rc}: no further probe is started"
    assert rc == 0, (rc, stderr[-2000:])
    lines = [ln for ln in stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, stdout[-2000:]
    with open(out) as f:
        assert f.read() == lines[0] + "\n"
    got = leaves(json.loads(lines[0]))
    want = golden[case]
    assert want["args"] == CASES[case][1]
    missing = sorted(set(want["keys"]) - set(got))
    assert not missing, missing
    differ = {k: (v, got[k]) for k, v in want["equal"].items() if got[k] != v}
    assert not differ, differ
