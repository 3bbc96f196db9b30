"""Two whole Split-Explicit steps on the GPU against two steps of the all-host composition
(tests/model_step_reference.py: the C oracle's tendencies and the NumPy restatements of every attached object, put
together as SplitExplicitStepper.h and VertMixStep.h write the sequence; the product has no part in it).  Both sides start
from the same host arrays (tests/model_step_fixtures.py).  After each step every array the product keeps is compared
bit for bit, in the order of the sequence, so that the first failure names the earliest stage that went wrong; then the
state itself, both time levels, row padding and sentinel rows included.  No masks: an entry no contract names holds the
rig's seed on both sides.

The rungs (tests.model_step_fixtures.RUNGS) add one object each: A nothing attached (K = 1 and 5), B PressureGrad and
VertAdv, C the 2-D MonotoneAdv with the unlimited vertical tracer term, D the 3-D MonotoneAdv at order 4 and 3, E the
GentMcWilliams, F the VertMixStep hook with wind stress, drags and surface fluxes -- on planar_hex(8, 8) with K = 5, and
on hex24x20 with K = 17 (padded rows) with both flux thicknesses, with the three switches of the stepper off, and with
the linear Eos -- and G everything on fib300_coast_ragged with K = 6: a sphere with land, ragged ranges and KMin > 0.
Then the objects attached since: H the Redi on top of F (and alone, on centred advection), I the Kpp on top of F (and
with the Redi: steps 4, 4a, 4b, 4c, 5 of VertMixStep.h in a step), J the VertRemap at its three orders in a step
without a VertAdv, K Redi, Kpp and VertRemap together on hex24x20 with K = 17 (with the switches off and the linear Eos
too) and L the same on the ragged sphere, once with the VertAdv and once with the VertRemap: one-layer columns, the
sentinel cell at the coast, ranges that start below the top.  The Kpp rungs are forced so that no velocity scale takes
a cbrt branch (tests/model_step_fixtures.py): there the restatement is the device's bit for bit."""
import numpy as np
import pytest

import omega_amd as oa
from tests import model_step_reference as HM
from tests.model_step_fixtures import NT, PAD, RUNGS, ModelRig
from tests.vert_fixtures import same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    oa.device_init(0)


def stages(rig):
    """(stage, names) in the order of the sequence"""
    o = rig.opt
    out = [("1 momentum RHS", ["NormalVelocityTend"]), ("2-5, 8 BarotropicMode", list(HM.BTR_FIELDS))]
    if o["gm"]:
        out.append(("5b GentMcWilliams", ["BolusVelocity", "StreamFunction"]))
    if o["redi"]:
        out.append(("5c Redi", ["SlopeInterface"]))
    out.append(("6 thickness", ["LayerThicknessTend"] + (["VerticalTransport"] if o["vert_adv"] is not None else [])))
    if o["mono"] is not None:
        out.append(("7 MonotoneAdv", ["ScaleIn", "ScaleOut"] + (["Hess"] if o["mono"][0] != 2 else [])))
    out.append(("7 tracers", ["TracerTend"]))
    if o["remap"] is not None:
        out.append(("8b VertRemap", ["RemapTarget"]))
    if o["mix"]:
        names = ["BruntVaisalaFreqSq", "TangentialVelocity"]
        if o["kpp"]:
            names += ["BulkRichardson", "BoundaryLayerIndex", "BoundaryLayerDepth", "NonLocalShape"]
        if o["redi"]:
            names.append("VertDiffusivity")
        out.append(("9 VertMixStep", names + ["VertVisc", "VertDiff"]))
    if rig.has_column:
        out.append(("column fields", list(HM.COLUMN_FIELDS) + ["LayerThicknessTarget"]))
    return out


@pytest.mark.parametrize("rung", list(RUNGS))
def test_two_steps_equal_the_host_composition(rung):
    x = ModelRig(rung, device=True)
    host, n, ne, K = x.host, x.nc, x.ne, x.K
    for step in (1, 2):
        x.stepper.do_step(x.p.state)
        oa.device_synchronize()
        host.step()
        for stage, names in stages(x):
            for name in names:
                got, want = x.device_array(name), x.host_array(name)
                assert got.dtype == want.dtype == (np.int32 if name == "BoundaryLayerIndex" else np.float64), name
                assert np.isfinite(want).all() and np.isfinite(got).all(), f"step {step}, {stage}: {name}"
                same(got, want, f"step {step}, {stage}: {name}")
        for level, when in ((0, "new"), (1, "old")):
            for name, got, want in zip(("h", "u", "tracers"), x.raw_state(level), (host.h[level], host.u[level], host.tr[level])):
                assert np.isfinite(got).all(), f"step {step}: {name} ({when} level)"
                same(got, x.padded(want), f"step {step}: {name} ({when} level, row padding and sentinel row included)")
        # ... and the step was not a step of nothing
        for name, got, start in zip(("h", "u", "tracers"), x.raw_state(0), host.start):
            assert not np.array_equal(got[..., :K], start), name
        o = x.opt
        if o["gm"]:
            assert np.abs(x.device_array("BolusVelocity")[:ne]).max() > 0.0
        if o["vert_adv"] is not None:
            assert np.abs(x.device_array("VerticalTransport")[:n]).max() > 0.0
        if o["mono"] is not None:
            assert (x.device_array("ScaleIn")[:, :n] < 1.0).any() and (x.device_array("ScaleOut")[:, :n] < 1.0).any()
        if o["mix"]:
            _, u, tr = x.raw_state(0)
            assert not np.array_equal(u[:, :K], host.unmixed[0]) and not np.array_equal(tr[..., :K], host.unmixed[1])
        if o["redi"]:
            assert np.abs(x.device_array("SlopeInterface")[:ne][host.e_range[:ne]]).max() > 0.0
            faces = host.c_range[:n, 1:] & host.c_range[:n, :-1]
            assert np.abs(x.device_array("VertDiffusivity")[:n, 1:][faces]).max() > 0.0
        if o["kpp"]:
            wet = host.c_range[:n].any(axis=1)
            assert (x.device_array("NonLocalShape")[:n] > 0.0).any() and np.all(x.device_array("BoundaryLayerDepth")[:n][wet] > 0.0)
        if o["remap"] is not None:
            h = x.raw_state(0)[0][:, :K]
            assert np.array_equal(h[host.c_range], x.device_array("RemapTarget")[host.c_range])
            assert not np.array_equal(h[host.c_range], host.lagrangian_h[host.c_range])
    assert x.stepper.time == 2 * host.dt_seconds and host.steps_done == 2
    assert PAD != 0.0 and NT == 2
