"""The 3-D form of MonotoneAdv on the GPU (MonotoneAdv::attachVertAdv; omega_amd/csrc/MonotoneAdv.h,
kernels/MonotoneAdvKernels.hip, Vert = true), VertAdv::TracerTermEnable and the attachment to the Split-Explicit
stepper.

The yardstick of the call is the restatement (tests/monotone_adv_reference.py), compared as
tests/test_monotone_adv_gpu.py compares the 2-D form: outputs seeded with NaN and read back raw.  VerticalTransport is
NaN wherever no flux passes (tests/monotone_adv_fixtures.py) and in its row padding, like the padding of every input."""
import numpy as np
import pytest

import omega_amd as oa
from tests.column_reference import RHO0
from tests.monotone_adv_fixtures import RANDOM, Inputs, Mono3Rig
from tests.rank_rig import raw
from tests.split_explicit_fixtures import StepRig
from tests.test_monotone_adv_3d import margin_value
from tests.test_monotone_adv_gpu import MAXT, NO_ADV, Dev, assert_bits, mono_step_by_hand

pytestmark = pytest.mark.gpu

# no interface (1); one interface inside a two-level lane (2); one-level lanes (3, 15, 17, 37); an interface across a
# lane pair and, at 16 | 17, across a 128-byte line; level chunks over gridDim.y, an interface across two chunks (80)
LEVELS = (1, 2, 3, 15, 16, 17, 37, 80)


@pytest.fixture(scope="module", autouse=True)
def _device():
    oa.device_init(0)


class Dev3(Dev):
    """Dev with a VertCoord of the rig's ranges and a VertAdv holding the inputs' VerticalTransport, attached"""

    def __init__(self, R, I, max_tracers=MAXT):
        super().__init__(R, I, max_tracers)
        self.vc = oa.VertCoord(R.mesh, R.K, RHO0, "Uniform", R.min_level, R.max_level, decomp=R.decomp)
        assert np.array_equal(self.vc.get("MinLayerCell"), R.lo) and np.array_equal(self.vc.get("MaxLayerCell"), R.hi)
        self.va = oa.VertAdv(R.mesh, self.vc, 2)
        self.wt = self.padded(I.wt)
        oa.copy_to_device(self.va.device_ptr("VerticalTransport"), self.wt)
        self.mono.attach_vert_adv(self.va)

    def check(self, nt, stream=None):
        got = super().check(nt, stream)
        assert_bits(raw(self.va.device_ptr("VerticalTransport"), self.wt.shape), self.wt, "VerticalTransport")
        return got


_CASES = {}


def case(name, K, upwind):
    key = (name, K, upwind)
    if key not in _CASES:
        R = Mono3Rig(name, K, device=True)
        _CASES[key] = Dev3(R, R.inputs(seed=3 + K, upwind=upwind, ntracers=MAXT, check=False))
    return _CASES[key]


@pytest.mark.parametrize("upwind", (False, True), ids=("centre", "upwind"))
@pytest.mark.parametrize("nt", (1, 2, 3, 4, MAXT))
@pytest.mark.parametrize("K", LEVELS)
@pytest.mark.parametrize("name", ("hex24x20", "fib700_coast_ragged"))
def test_bit_exact_on_nan_seeded_arrays(name, K, nt, upwind):
    D = case(name, K, upwind)
    _, si, so = D.check(nt)
    if nt == MAXT and K >= 3:  # the comparison is about a limiter at work, in the vertical too
        r = si[RANDOM, : D.R.nc, :K]
        assert (r < 1.0).any() and (r == 1.0).any() and (so[RANDOM, : D.R.nc, :K] < 1.0).any()
        lim, free = D.R.limited_interfaces(D.I, RANDOM)
        assert lim > 0.0 and free > 0.0


def test_launch_shape_with_a_tail_split():
    """hex130x130, K = 32, NT = 2: the last tiles are tail-split, one level chunk per workgroup (derived in
    tests/test_transport_gpu.py): an interface between two workgroups"""
    R = Mono3Rig("hex130x130", 32, device=True)
    Dev3(R, R.inputs(seed=2, ntracers=2, check=False), max_tracers=2).check(2)


def test_stream_forms_agree_and_detach_gives_the_2d_bits():
    D = case("hex24x20", 16, False)
    a = D.check(3)
    b = D.check(3, stream=oa.Stream())
    for x, y in zip(a, b):
        assert_bits(x, y, "null stream / stream")
    # detached: the 2-D restatement on the same inputs, and not what the 3-D form gave
    D.mono.attach_vert_adv(None)
    t_seed, s_seed = D.seed(3)
    D.run(3)
    got = D.read()
    want = D.R.reference_2d(D.I, 3, D.tend0)
    for g, w, seed, name in zip(got, want, (t_seed, s_seed, s_seed), ("Tend", "ScaleIn", "ScaleOut")):
        expect = seed.copy()
        expect[:3, : D.R.nc, : D.K] = w[:3, : D.R.nc]
        assert_bits(g, expect, f"{name}, detached")
    assert not np.array_equal(got[0][:3, : D.R.nc, : D.K], a[0][:3, : D.R.nc, : D.K])
    D.mono.attach_vert_adv(D.va)
    for x, y in zip(a, D.check(3)):
        assert_bits(x, y, "attached again")


def test_calls_create_no_device_resource():
    D = case("hex24x20", 16, False)
    D.run(2)
    oa.device_synchronize()
    before = oa.device_resource_count()
    for nt in (1, 2, 5, MAXT):
        D.run(nt)
    D.mono.attach_vert_adv(None)
    D.run(2)
    D.mono.attach_vert_adv(D.va)
    D.run(2)
    oa.device_synchronize()
    assert oa.device_resource_count() == before


def test_two_part_decomposition_matches_on_owned_cells():
    """halo width 3, as in tests/test_monotone_adv_gpu.py: the vertical part needs no other cell, so the rule stays"""
    K, nt = 5, 3
    R1 = Mono3Rig("hex24x20", K, device=True)
    I1 = R1.inputs(seed=8, ntracers=nt, check=False)
    D1 = Dev3(R1, I1, nt)
    D1.tend0[:] = 0.0  # (the seed is drawn in local order)
    one = D1.check(nt)
    cid1, eid1 = R1.decomp.get_array("CellID")[: R1.nc] - 1, R1.decomp.get_array("EdgeID")[: R1.ne] - 1
    ncg, neg = cid1.max() + 1, eid1.max() + 1
    glob = {}
    for n, ids, rows in (("h_old", cid1, ncg), ("h_new", cid1, ncg), ("wt", cid1, ncg), ("u", eid1, neg)):
        glob[n] = np.zeros((rows, K))
        glob[n][ids] = getattr(I1, n)[: len(ids)]
    glob["tracers"] = np.zeros((nt, ncg, K))
    glob["tracers"][:, cid1] = I1.tracers[:, : R1.nc]
    result = np.zeros((3, nt, ncg, K))
    for w in range(3):
        result[w][:, cid1] = one[w][:nt, : R1.nc, :K]
    for rank in range(2):
        R = Mono3Rig("hex24x20", K, nparts=2, rank=rank, device=True, halo=3)
        own = R.mesh.NCellsOwned
        assert R.nc > own
        cid, eid = R.decomp.get_array("CellID")[: R.nc] - 1, R.decomp.get_array("EdgeID")[: R.ne] - 1
        I = Inputs()
        I.upwind, I.dt = False, I1.dt
        for n, ids, size in (("h_old", cid, R.nc_size), ("h_new", cid, R.nc_size), ("wt", cid, R.nc_size),
                             ("u", eid, R.ne_size)):
            a = np.full((size, K), np.nan)
            a[: len(ids)] = glob[n][ids]
            setattr(I, n, a)
        I.tracers = np.full((nt, R.nc_size, K), np.nan)
        I.tracers[:, : R.nc] = glob["tracers"][:, cid]
        D = Dev3(R, I, nt)
        D.tend0[:] = 0.0
        got = D.check(nt)  # every local cell against the local restatement ...
        for w, name in enumerate(("Tend", "ScaleIn", "ScaleOut")):  # ... and the owned ones against the one-part run
            assert_bits(got[w][:nt, :own, :K], result[w][:, cid[:own]], f"{name} on the owned cells of part {rank}")


# ---------------------------------------------------------------------------------------------------------------------
# the switch on the Tendencies
# ---------------------------------------------------------------------------------------------------------------------
def test_tracer_term_switch():
    """off: TracerTend of the three paths that add the term is that of a Tendencies without a VertAdv; the thickness and
    velocity tendencies keep the attached one's bits; VertAdv.add_tracers itself does not look at the switch"""
    K = 5
    off, on, none = StepRig(K=K), StepRig(K=K), StepRig(K=K)
    off.va.set_tracer_term(False)
    none.p.tend.attach_vert_adv(None)

    def tendencies(x, path):
        p = x.p
        p.tend.compute_all_tendencies(p.state, p.aux, p.tracers, 0, 0, 0)  # (VerticalTransport for the group call)
        if path != "all":
            for which in range(3):
                ptr, n = p.tend.device_ptr(which)
                oa.copy_to_device(ptr, np.full(n, np.nan))
            if path == "transport":
                p.tend.compute_transport_tendencies(p.state, p.aux, p.tracers, 0, 0, 0)
            else:
                p.tend.compute_tracer_tendencies(p.state, p.aux, p.tracers, 0, 0, 0)
        oa.device_synchronize()
        return [p.tend.get(which) for which in range(3)]

    for path in ("all", "transport", "tracer_group"):
        a, b, c = tendencies(off, path), tendencies(on, path), tendencies(none, path)
        assert np.isfinite(a[2][:, : off.p.mesh.NCellsAll]).all()  # (the seed stays on the sentinel row)
        assert_bits(a[2], c[2], f"TracerTend, {path}: switched off / no VertAdv")
        assert not np.array_equal(a[2], b[2]), path  # the term is not nothing
        if path != "tracer_group":
            assert_bits(a[0], b[0], f"LayerThicknessTend, {path}")
            assert not np.array_equal(a[0], c[0]), path
        if path == "all":
            assert_bits(a[1], b[1], "NormalVelocityTend")
            assert not np.array_equal(a[1], c[1])
        assert_bits(off.va.get("VerticalTransport"), on.va.get("VerticalTransport"), "VerticalTransport")
    # the direct call ignores the switch
    m = off.p.mesh
    zero = np.zeros((off.nt, m.NCellsSize, K))
    a = off.va.add_tracers(zero.copy(), off.h, off.tr, off.nt)
    b = on.va.add_tracers(zero.copy(), on.h, on.tr, on.nt)
    assert a[:, : m.NCellsAll].any()
    assert_bits(a, b, "VertAdv.add_tracers with the switch off / on")
    off.va.set_tracer_term(True)
    assert_bits(tendencies(off, "all")[2], tendencies(on, "all")[2], "switched on again")


# ---------------------------------------------------------------------------------------------------------------------
# the stepper
# ---------------------------------------------------------------------------------------------------------------------
def mono3(x, term_off=True):
    """a MonotoneAdv with the rig's VertAdv attached (the one on its Tendencies)"""
    mono = oa.MonotoneAdv(x.p.mesh, x.K, x.nt)
    mono.attach_vert_adv(x.va)
    x.va.set_tracer_term(not term_off)
    return mono


@pytest.mark.parametrize("fused", (True, False), ids=("fused_transport", "group_calls"))
@pytest.mark.parametrize("nsub", (1, 7))
def test_attached_step_equals_the_calls_by_hand(nsub, fused):
    dt, K = 20.0, 5
    a, b = StepRig(K=K, config=NO_ADV), StepRig(K=K, config=NO_ADV)
    ma, mb = mono3(a), mono3(b)
    st = a.stepper("Split-Explicit", dt, nsub)
    st.set_fused_transport(fused)
    st.attach_monotone_adv(ma)
    st.do_step(a.p.state)
    mono_step_by_hand(b, mb, dt, nsub, fused)
    got, want = a.result(), b.result()
    for name, g, w, start in zip(("h", "u", "tracers"), got, want, (a.h, a.u, a.tr)):
        assert np.isfinite(g).all() and not np.array_equal(g, start), name
        assert_bits(g, w, name)
    for name in ("ScaleIn", "ScaleOut"):
        assert_bits(ma.get(name), mb.get(name), name)
    assert np.abs(a.va.get("VerticalTransport")).max() > 0.0
    before = oa.device_resource_count()  # a step creates no device resource
    for _ in range(2):
        st.do_step(a.p.state)
    oa.device_synchronize()
    assert oa.device_resource_count() == before
    # and the vertical limiter was part of it: the parent's configuration on the same rig differs
    c = StepRig(K=K, config=NO_ADV)
    sc = c.stepper("Split-Explicit", dt, nsub)
    sc.attach_monotone_adv(oa.MonotoneAdv(c.p.mesh, K, c.nt))
    sc.do_step(c.p.state)
    assert not np.array_equal(c.result()[2], want[2])


def test_eight_steps_keep_a_step_tracer_in_its_range():
    """planar_hex(8, 8), K = 5, z-star VertAdv and PressureGrad, Dt = 600 s, tracer 0 a 0/1 step in x and at mid-depth.
    With the VertAdv attached to the MonotoneAdv and its tracer term off the tracer stays in [0, 1] up to the margin of
    tests/test_monotone_adv_3d.py, once per step; the parent's configuration -- the 2-D MonotoneAdv and the unlimited
    vertical term -- leaves the interval by more than that.  The Courant numbers are measured on the way: the horizontal
    estimate of tests/test_monotone_adv_gpu.py plus Dt*max|VerticalTransport|*2/min(h), required below 0.5."""
    dt, nsub, steps, K = 600.0, 30, 8, 5
    off = dict(NO_ADV, TracerDiffTendencyEnable=0, TracerHyperDiffTendencyEnable=0)
    results = {}
    for limited in (True, False):
        x = StepRig(K=K, config=off)
        m = x.p.mesh
        nc = m.NCellsAll
        xc = m.get_array("XCell")[:nc]
        x.tr[0, :nc] = ((xc > np.median(xc))[:, None] != (np.arange(K) >= (K + 1) // 2)[None, :]).astype(float)
        x.load()
        st = x.stepper("Split-Explicit", dt, nsub)
        st.attach_monotone_adv(mono3(x) if limited else oa.MonotoneAdv(m, K, x.nt))
        h_min, u_max, w_max = x.h[:nc].min(), 0.0, 0.0
        for _ in range(steps):
            st.do_step(x.p.state)
            h, u, _ = x.result()
            h_min, u_max = min(h_min, h[:nc].min()), max(u_max, np.abs(u[: m.NEdgesAll]).max())
            w_max = max(w_max, np.abs(x.va.get("VerticalTransport")[:nc]).max())
        h, u, tr = x.result()
        area, dv = m.get_array("AreaCell")[:nc], m.get_array("DvEdge")[: m.NEdgesAll]
        courant = dt * u_max * 3.0 * dv.max() / area.min() + dt * w_max * 2.0 / h_min
        print("3-D" if limited else "parent", "Courant estimate", courant, "max |Wt|", w_max, "min h", h_min)
        assert np.isfinite(tr).all() and h_min > 0.0 and w_max > 0.0 and courant < 0.5
        results[limited] = (tr[:, :nc], h, h_min)
    n = m.get_array("EdgesOnCell").shape[1]
    tr, h, h_min = results[True]
    mg = steps * margin_value(n, h.max(), 1.0, h_min)
    over = max(tr[0].max() - 1.0, 0.0 - tr[0].min())
    print("3-D: outside [0, 1] by", over, "margin", mg)
    assert over <= mg
    lo, hi = x.tr[1, :nc].min(), x.tr[1, :nc].max()  # the second tracer in its own range
    assert max(tr[1].max() - hi, lo - tr[1].min()) <= steps * margin_value(n, h.max(), hi, h_min)
    tr, h, h_min = results[False]
    over = max(tr[0].max() - 1.0, 0.0 - tr[0].min())
    print("parent's configuration: outside [0, 1] by", over)
    assert over > steps * margin_value(n, h.max(), 1.0, h_min)


def test_refusals():
    K = 4
    x = StepRig(K=K, config=NO_ADV)
    m, nt = x.p.mesh, x.nt
    E = oa.OmegaAmdError
    # the attachment to the MonotoneAdv
    mono = oa.MonotoneAdv(m, K, nt)
    other = oa.HorzMesh(x.p.decomp, K)
    with pytest.raises(E, match="attachVertAdv: the VertAdv was built for another mesh or layer count"):
        mono.attach_vert_adv(oa.VertAdv(other, oa.VertCoord(other, K, RHO0, "Uniform", decomp=x.p.decomp), 2))
    with pytest.raises(E, match="attachVertAdv: the VertAdv was built for another mesh or layer count"):
        oa.MonotoneAdv(m, K + 1, nt).attach_vert_adv(x.va)
    # the attachment to the stepper
    step = x.stepper("Split-Explicit", 20.0, 2)
    foreign = oa.VertAdv(m, x.vc, 2)
    foreign.set_tracer_term(False)
    mono.attach_vert_adv(foreign)
    with pytest.raises(E, match="attachMonotoneAdv: the MonotoneAdv's VertAdv is not the one attached to the Tendencies"):
        step.attach_monotone_adv(mono)
    mono.attach_vert_adv(x.va)
    with pytest.raises(E, match="attachMonotoneAdv: the VertAdv's TracerTermEnable is on"):
        step.attach_monotone_adv(mono)
    x.va.set_tracer_term(False)
    step.attach_monotone_adv(mono)
    step.do_step(x.p.state)
    # doStep checks again
    x.va.set_tracer_term(True)
    with pytest.raises(E, match="doStep: the VertAdv's TracerTermEnable is on"):
        step.do_step(x.p.state)
    x.va.set_tracer_term(False)
    x.p.tend.attach_vert_adv(None)
    with pytest.raises(E, match="doStep: the MonotoneAdv's VertAdv is not the one attached"):
        step.do_step(x.p.state)
    x.p.tend.attach_vert_adv(x.va)
    step.do_step(x.p.state)
    # a MonotoneAdv without a VertAdv goes on as before, whatever the Tendencies' VertAdv says
    mono.attach_vert_adv(None)
    x.va.set_tracer_term(True)
    step.do_step(x.p.state)
    step.attach_monotone_adv(None)
    oa.device_synchronize()
