"""Tendencies::computeMomentumTendencies and Tendencies::computeTransportTendenciesAndUpdate on the GPU, and the two
switches of the Split-Explicit stepper that use them (UseMomentumRHS, FoldUpdates).

The yardstick is that of tests/test_transport_gpu.py: poison the arrays with NaN, run the sequence the new call stands
for and read the raw device arrays back (row padding, level padding and sentinel row included); poison again, run the new
call; every local row must hold the sequence's bits and everything else the poison.

  momentum   against compute_all_tendencies with the same arguments: NormalVelocityTend on rows < NEdgesAll and
             LayerThicknessTend on rows < NCellsAll; TracerTend and Del2TracersCell keep their poison.
  folded     against compute_transport_tendencies, update_by_tend and update_tracers_by_tend (the streaming kernels of the
             time steppers): the thickness of time level 1 and the tracers of time level 1 on [:NCellsAll, :K]; their
             level padding, which the streaming kernels sweep, keeps the poison.  The new values are also compared with
             the two update formulas evaluated by NumPy (IEEE double, no contraction: the same roundings), so the check
             does not rest on the GPU's division alone.

As in test_transport_gpu.py the thickness is read from time level 0 and the velocity from time level 1, which holds
another velocity (both upwind directions occur)."""
import numpy as np
import pytest

import omega_amd as oa
from tests.meshes import named_mesh
from tests.problem import Problem, poison_tendencies
from tests.rank_rig import raw
from tests.split_explicit_fixtures import StepRig
from tests.vert_adv_fixtures import adv_inputs

pytestmark = pytest.mark.gpu

STEP_DT = 20.0
COEFF = 37.5  # seconds; not a power of two, so Coeff*Tend rounds
LEVELS = [1, 3, 16, 17, 60]  # odd K (one level per lane), K < 16 (lanes span the column), pitch != K (17 -> 32, 60 -> 64)
# the smallest spherical mesh and the smallest culled-coast mesh of tests/test_gpu_parity.py: pentagons (the lists of
# the rarer valences in levels 1 and 3 of the fused RHS) and boundary edges (the irregular-edge lists)
MOMENTUM_MESHES = ["hex16x16", "ico2", "hex20x16_coast_channel_compact"]
NO_PV = dict(PVTendencyEnable=0, KETendencyEnable=0, EddyDiff4=2.5e9)  # the Fast = false instantiations


@pytest.fixture(scope="module", autouse=True)
def _device():
    oa.device_init(0)


def bits_equal(a, b):
    """the same 64 bits (so -0 differs from +0), or NaN on both sides"""
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def assert_bits(got, want, name):
    assert got.shape == want.shape, name
    bad = ~bits_equal(np.ascontiguousarray(got), np.ascontiguousarray(want))
    assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


def raw_tendencies(P):
    """the three whole device arrays (planes, rows, pitch), as poison_tendencies lays them out"""
    pitch = oa.level_pitch(P.K)
    m = P.mesh
    return [raw(P.tend.device_ptr(w)[0], (planes, rows, pitch))
            for w, rows, planes in ((0, m.NCellsSize, 1), (1, m.NEdgesSize, 1), (2, m.NCellsSize, max(P.NT, 1)))]


def second_level(P):
    """time level 1: another velocity, a NaN thickness (not to be read)"""
    m = P.mesh
    P.u1 = P.u * np.where(np.arange(m.NEdgesSize) % 2, -0.75, 0.75)[:, None]
    h1 = np.zeros_like(P.h)
    h1[: m.NCellsAll] = np.nan
    P.state.copy_to_device(h1, P.u1, 1)


def expect_rows(poison, want, n, K):
    """the poison with the wanted values on [:, :n, :K]"""
    e = poison.copy()
    e[:, :n, :K] = want[:, :n, :K]
    return e


# ---------------------------------------------------------------------------------------------------------------------
# computeMomentumTendencies
# ---------------------------------------------------------------------------------------------------------------------
def check_momentum(P, args=(0, 0, 0), tracers_untouched=True, before_new=None):
    """the yardstick; returns compute_all_tendencies' raw arrays"""
    m, K = P.mesh, P.K
    seed = np.random.default_rng(3).uniform(1.0, 2.0, P.aux._shape("Del2TracersCell"))
    poison_tendencies(P)
    oa.device_synchronize()
    poison = raw_tendencies(P)
    P.tend.compute_all_tendencies(P.state, P.aux, P.tracers, *args)
    oa.device_synchronize()
    want = raw_tendencies(P)
    assert np.isfinite(want[1][0, : m.NEdgesOwned, :K]).all() and np.isfinite(want[0][0, : m.NCellsOwned, :K]).all()
    poison_tendencies(P)
    P.aux.set("Del2TracersCell", seed)
    if before_new:
        before_new()
    P.tend.compute_momentum_tendencies(P.state, P.aux, P.tracers, *args)
    oa.device_synchronize()
    got = raw_tendencies(P)
    assert_bits(got[1], expect_rows(poison[1], want[1], m.NEdgesAll, K), "NormalVelocityTend")
    assert_bits(got[0], expect_rows(poison[0], want[0], m.NCellsAll, K), "LayerThicknessTend")
    if tracers_untouched:
        assert_bits(got[2], poison[2], "TracerTend")
        assert_bits(P.aux.get("Del2TracersCell"), seed, "Del2TracersCell")
    return want


@pytest.mark.parametrize("config", [{}, NO_PV], ids=["default_terms", "pv_and_ke_off"])
@pytest.mark.parametrize("K", LEVELS)
@pytest.mark.parametrize("mesh", MOMENTUM_MESHES)
def test_momentum_equals_compute_all(mesh, K, config):
    planar = mesh == "hex16x16"
    P = Problem(named_mesh(mesh), K, 2, config=config, oracle=planar and K <= 16)
    want = check_momentum(P)
    if hasattr(P, "oracle"):  # ... and compute_all_tendencies' velocity tendency is the CPU oracle's
        own = P.mesh.NEdgesOwned
        uT = P.oracle.compute_all_tendencies(P.h, P.u, P.tr)[1]
        assert_bits(want[1][0, :own, :K], uT[:own], "NormalVelocityTend against the oracle")


def test_momentum_reads_the_time_levels_it_is_given():
    P = Problem(named_mesh("hex16x16"), 6, 2, oracle=False)
    plain = check_momentum(P)
    second_level(P)
    P.state.copy_to_device(P.h * 1.25, P.u1, 1)
    other = check_momentum(P, args=(0, 1, 1))
    assert not bits_equal(other[1], plain[1])[0, : P.mesh.NEdgesAll, : P.K].all()


def test_momentum_with_pressure_grad_and_vert_adv_attached():
    x = StepRig(attached=True)
    P, m, K = x.p, x.p.mesh, x.K
    # (the velocity term reads the transport that the call itself derives from its thickness tendency)
    want = check_momentum(P, before_new=lambda: x.va.set("VerticalTransport", np.full((m.NCellsSize, K), np.nan)))
    P.tend.attach_vert_adv(None)
    P.tend.attach_pressure_grad(None)
    plain = check_momentum(P)
    for w, n in ((0, m.NCellsAll), (1, m.NEdgesAll)):  # the attached terms changed both: the comparison was about them
        assert not bits_equal(want[w][:, :n, :K], plain[w][:, :n, :K]).all()


def test_momentum_with_a_custom_velocity_hook_runs_compute_all():
    from tests import manufactured as ms
    g = named_mesh("hex16x16")
    P = Problem(g, 4, 2, oracle=False)
    wx, wy = ms.wavelengths(g)
    plain = check_momentum(P)
    P.tend.use_manufactured_solution(P.mesh, wx, wy, ms.ETA0)
    want = check_momentum(P, tracers_untouched=False)
    n = P.mesh.NEdgesAll
    assert not bits_equal(want[1][:, :n, : P.K], plain[1][:, :n, : P.K]).all()  # the hook added its term
    oa.device_synchronize()
    got = raw_tendencies(P)  # the documented side effect of the fallback: TracerTend is written too
    assert_bits(got[2][:, : P.mesh.NCellsAll, : P.K], want[2][:, : P.mesh.NCellsAll, : P.K], "TracerTend of the fallback")
    P.tend.clear_custom_tendencies()


# ---------------------------------------------------------------------------------------------------------------------
# computeTransportTendenciesAndUpdate
# ---------------------------------------------------------------------------------------------------------------------
class Outputs:
    """the raw arrays the folded call writes: thickness of time level 1, tracers of time level `tracer_tl`"""

    def __init__(self, P, tracer_tl=1):
        m = P.mesh
        self.P, self.pitch, self.tracer_tl = P, oa.level_pitch(P.K), tracer_tl
        self.h_cur, self.h_next = P.state.device_ptr(0, 0), P.state.device_ptr(0, 1)
        self.h_shape = (1, m.NCellsSize, self.pitch)
        self.tr_shape = (max(P.NT, 1), m.NCellsSize, self.pitch)
        if P.NT > 0:
            self.tr_cur, self.tr_next = P.tracers.device_ptr(0), P.tracers.device_ptr(tracer_tl)

    def poison(self):
        """NaN everywhere, the zero sentinel row excepted (as poison_tendencies)"""
        for ptr, shape in self._arrays():
            p = np.full(shape, np.nan)
            p[:, -1, :] = 0.0
            oa.copy_to_device(ptr, p)
        poison_tendencies(self.P)

    def _arrays(self):
        out = [(self.h_next, self.h_shape)]
        if self.P.NT > 0 and self.tracer_tl != 0:
            out.append((self.tr_next, self.tr_shape))
        return out

    def read(self):
        oa.device_synchronize()
        h = raw(self.h_next, self.h_shape)
        tr = raw(self.tr_next, self.tr_shape) if self.P.NT > 0 else None
        return h, tr, raw_tendencies(self.P)

    def sequence(self, coeff):
        """what the folded call stands for: the transport call and the two streaming update kernels"""
        P, m = self.P, self.P.mesh
        P.tend.compute_transport_tendencies(P.state, P.aux, P.tracers, 0, 0, 1)
        oa.update_by_tend(self.h_next, self.h_cur, P.tend.device_ptr(0)[0], coeff, m.NCellsAll, self.pitch)
        if P.NT > 0:
            oa.update_tracers_by_tend(self.tr_next, self.tr_cur, self.h_next, self.h_cur, P.tend.device_ptr(2)[0], coeff,
                                      P.NT, m.NCellsAll, m.NCellsSize, self.pitch)

    def folded(self, coeff, keep):
        P = self.P
        P.tend.compute_transport_tendencies_and_update(P.state, P.aux, P.tracers, 0, 0, 1, 1, self.tracer_tl, coeff, keep)


def check_folded(P, keeps=(1, 0), coeff=COEFF, numpy_too=True):
    """the yardstick, once per value of KeepTendencies; returns the sequence's raw arrays (h, tracers, tendencies)"""
    m, K, n = P.mesh, P.K, P.mesh.NCellsAll
    if not hasattr(P, "u1"):
        second_level(P)
    out = Outputs(P)
    out.poison()
    p_h, p_tr, p_tend = out.read()
    out.sequence(coeff)
    w_h, w_tr, w_tend = out.read()
    assert_bits(w_tend[1], p_tend[1], "NormalVelocityTend after the sequence")
    if numpy_too:  # the streaming kernels' formulas in IEEE double
        with np.errstate(all="ignore"):
            hn = P.h[:n] + coeff * w_tend[0][0, :n, :K]
            assert_bits(w_h[0, :n, :K], hn, "the sequence's thickness against NumPy")
            if P.NT > 0:
                assert_bits(w_tr[:, :n, :K], (P.tr[:, :n] * P.h[:n] + coeff * w_tend[2][:, :n, :K]) / hn,
                            "the sequence's tracers against NumPy")
    for keep in keeps:
        out.poison()
        out.folded(coeff, keep)
        g_h, g_tr, g_tend = out.read()
        assert_bits(g_h, expect_rows(p_h, w_h, n, K), f"thickness of the new level (keep {keep})")  # level padding: poison
        if P.NT > 0:
            assert_bits(g_tr, expect_rows(p_tr, w_tr, n, K), f"tracers of the new level (keep {keep})")
        assert_bits(g_tend[1], p_tend[1], "NormalVelocityTend")
        for w, name in ((0, "LayerThicknessTend"), (2, "TracerTend")):
            expect = expect_rows(p_tend[w], w_tend[w], n, K) if (w == 0 or P.NT > 0) else p_tend[w]
            if keep:
                assert_bits(g_tend[w], expect, name)
            else:  # unspecified on the local rows; untouched everywhere else
                g = g_tend[w].copy()
                g[:, :n, :K] = expect[:, :n, :K]
                assert_bits(g, expect, f"{name} outside the local rows (keep 0)")
    return w_h, w_tr, w_tend


@pytest.mark.parametrize("upwind", [0, 1])
@pytest.mark.parametrize("hyper", [0, 1])
@pytest.mark.parametrize("NT", [0, 1, 2, 3])
@pytest.mark.parametrize("K", LEVELS)
def test_folded_update_equals_the_sequence(K, NT, hyper, upwind):
    """no tracers, the odd tracer alone, one whole block of the tracer loop, a block with remainder; the tracer update in
    launch 1 (hyperdiffusion off) and in launch 2 (on); KeepTendencies 1 and 0 inside check_folded"""
    cfg = dict(TracerHyperDiffTendencyEnable=hyper, EddyDiff4=3.0e9, FluxThicknessUpwind=upwind, FluxTracerUpwind=upwind)
    P = Problem(named_mesh("hex16x16"), K, NT, config=cfg, oracle=False)
    w_h, w_tr, _ = check_folded(P)
    own = P.mesh.NCellsOwned
    assert np.isfinite(w_h[0, :own, :K]).all() and not np.array_equal(w_h[0, :own, :K], P.h[:own])
    if NT > 0:
        assert np.isfinite(w_tr[:, :own, :K]).all() and not np.array_equal(w_tr[:, :own, :K], P.tr[:, :own])


@pytest.mark.parametrize("hyper", [0, 1])
def test_folded_update_on_a_two_part_decomposition_with_dry_cells(hyper):
    """every local row, halo included; a cell and its ring with zero thickness, so that the centre's new thickness is
    zero and the tracer update divides by it: the same NaN / Inf bits from the folded division as from the streaming one"""
    for rank in range(2):
        P = Problem(named_mesh("hex32x32"), 16, 3, nparts=2, rank=rank, halo_width=3, oracle=False,
                    config=dict(TracerHyperDiffTendencyEnable=hyper, EddyDiff4=3.0e9))
        m = P.mesh
        assert m.NCellsAll > m.NCellsOwned
        eoc, nec, coe = m.get_array("EdgesOnCell"), m.get_array("NEdgesOnCell"), m.get_array("CellsOnEdge")
        for centre in (5, m.NCellsAll - 3):  # an owned cell and a halo cell
            ring = np.unique(coe[eoc[centre, : nec[centre]]])
            P.h[ring[ring < m.NCellsAll]] = 0.0
        P.state.copy_to_device(P.h, P.u, 0)
        w_h, w_tr, _ = check_folded(P)
        assert (w_h[0, 5, : P.K] == 0.0).all()
        assert not np.isfinite(w_tr[:, 5, : P.K]).any() and np.isfinite(w_tr[:, : m.NCellsOwned, : P.K]).any()


# hex130x130, K = 32, NT = 2: 2113 tiles of 8 cells, of which the last 65 are tail-split (one level chunk per workgroup);
# derived in tests/test_transport_gpu.py.  Both launches' update variants go through that shape.
@pytest.mark.parametrize("hyper", [0, 1])
def test_folded_update_launch_shape_with_a_tail_split(hyper):
    P = Problem(named_mesh("hex130x130"), 32, 2, config=dict(TracerHyperDiffTendencyEnable=hyper, EddyDiff4=3.0e9), oracle=False)
    check_folded(P, keeps=(1,), numpy_too=False)


def test_folded_update_with_a_vert_adv_attached_runs_the_sequence():
    g, K, nt = named_mesh("hex24x20"), 16, 2
    P = Problem(g, K, nt, oracle=False)
    G = adv_inputs(g, K, nt)
    m, n = P.mesh, P.mesh.NCellsAll
    vc = oa.VertCoord(m, K, 1026.0, "Uniform", G["min_level"], G["max_level"], decomp=P.decomp)
    ref = np.zeros((m.NCellsSize, K))
    ref[:n] = G["ref"][P.cell_id[:n] - 1]
    vc.set("RefLayerThickness", ref)
    va = oa.VertAdv(m, vc, 2)
    plain = check_folded(P, numpy_too=False)
    P.tend.attach_vert_adv(va)
    second_level(P)
    out = Outputs(P)
    out.poison()
    out.sequence(COEFF)
    w_h, w_tr, w_tend = out.read()
    for keep in (1, 0):  # (the fallback keeps the tendencies either way)
        out.poison()
        va.set("VerticalTransport", np.full((m.NCellsSize, K), np.nan))
        out.folded(COEFF, keep)
        g_h, g_tr, g_tend = out.read()
        assert_bits(g_h[:, :n, :K], w_h[:, :n, :K], "thickness of the new level")
        assert_bits(g_tr[:, :n, :K], w_tr[:, :n, :K], "tracers of the new level")
        for w in (0, 2):
            assert_bits(g_tend[w][:, :n, :K], w_tend[w][:, :n, :K], "the tendencies")
    assert not bits_equal(w_h[:, :n, :K], plain[0][:, :n, :K]).all()  # the attached terms changed the result
    assert not bits_equal(w_tr[:, :n, :K], plain[1][:, :n, :K]).all()
    P.tend.attach_vert_adv(None)


def test_folded_update_onto_its_own_tracers_runs_the_sequence():
    """NextTracers aliased to TracerArray: cells still gather their neighbours' tracers while others would store new
    ones, so the tendencies are completed first"""
    P = Problem(named_mesh("hex16x16"), 16, 2, oracle=False)
    n, K = P.mesh.NCellsAll, P.K
    second_level(P)
    out = Outputs(P, tracer_tl=0)
    results = []
    for run in (lambda: out.sequence(COEFF), lambda: out.folded(COEFF, 1)):
        P.tracers.copy_to_device(P.tr, 0)
        out.poison()
        run()
        results.append(out.read())
    (w_h, w_tr, w_tend), (g_h, g_tr, g_tend) = results
    assert_bits(g_h[:, :n, :K], w_h[:, :n, :K], "thickness of the new level")
    assert_bits(g_tr[:, :n, :K], w_tr[:, :n, :K], "the tracers, updated in place")
    assert np.isfinite(w_tr[:, : P.mesh.NCellsOwned, :K]).all() and not np.array_equal(w_tr[:, :n, :K], P.tr[:, :n])
    for w in (0, 2):
        assert_bits(g_tend[w][:, :n, :K], w_tend[w][:, :n, :K], "the tendencies")


def test_bad_time_levels_are_refused():
    P = Problem(named_mesh("hex16x16"), 4, 2, oracle=False)
    for args in ((0, 2, 0), (0, 0, 2), (0, -1, 0)):
        with pytest.raises(oa.OmegaAmdError, match="bad time level"):
            P.tend.compute_momentum_tendencies(P.state, P.aux, P.tracers, *args)
        with pytest.raises(oa.OmegaAmdError, match="bad time level"):
            P.tend.compute_transport_tendencies_and_update(P.state, P.aux, P.tracers, *args, 1, 1, COEFF, True)
    with pytest.raises(oa.OmegaAmdError, match="time level out of range"):
        P.tend.compute_momentum_tendencies(P.state, P.aux, P.tracers, 2, 0, 0)
    with pytest.raises(oa.OmegaAmdError, match="time level out of range"):
        P.tend.compute_transport_tendencies_and_update(P.state, P.aux, P.tracers, 2, 0, 0, 1, 1, COEFF, True)
    with pytest.raises(oa.OmegaAmdError, match="bad time level"):
        P.tend.compute_transport_tendencies_and_update(P.state, P.aux, P.tracers, 0, 0, 0, 2, 1, COEFF, True)
    with pytest.raises(oa.OmegaAmdError, match="time level out of range"):
        P.tend.compute_transport_tendencies_and_update(P.state, P.aux, P.tracers, 0, 0, 0, 1, 2, COEFF, True)


# ---------------------------------------------------------------------------------------------------------------------
# the stepper
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attached", [False, True], ids=["nothing_attached", "pressure_grad_and_vert_adv"])
@pytest.mark.parametrize("nsub", [1, 7])
def test_split_explicit_steps_are_the_same_bits_under_every_switch(nsub, attached):
    runs = {}
    for momentum, fold in ((False, False), (True, False), (False, True), (True, True)):
        x = StepRig(attached=attached)
        st = x.stepper("Split-Explicit", STEP_DT, nsub)
        st.set_momentum_rhs(momentum)
        st.set_folded_updates(fold)
        st.do_step(x.p.state)
        oa.device_synchronize()
        before = oa.device_resource_count()
        for _ in range(2):
            st.do_step(x.p.state)
        oa.device_synchronize()
        assert oa.device_resource_count() == before  # a step creates no buffer, stream or event
        runs[momentum, fold] = (x, x.result())
    x, off = runs[False, False]
    for key, (_, on) in runs.items():
        for name, a, b, start in zip(("h", "u", "tracers"), off, on, (x.h, x.u, x.tr)):
            assert np.isfinite(b).all(), (key, name)
            assert_bits(b, a, f"{name} after three steps, (momentum, fold) = {key}")
            assert not np.array_equal(b, start), (key, name)


@pytest.mark.parametrize("fused_transport,config", [(False, None), (True, dict(TracerHyperDiffTendencyEnable=0))],
                         ids=["group_calls", "hyperdiffusion_off"])
def test_the_fold_switch_where_the_stepper_does_not_take_it(fused_transport, config):
    """the fold has effect only with the fused transport, and the stepper does not take it with the tracer
    hyperdiffusion term off (no faster there): the same bits with the switch off and on in both cases"""
    runs = []
    for fold in (False, True):
        x = StepRig(attached=False, config=config)
        st = x.stepper("Split-Explicit", STEP_DT, 2)
        st.set_fused_transport(fused_transport)
        st.set_folded_updates(fold)
        st.do_step(x.p.state)
        runs.append(x.result())
    for a, b in zip(*runs):
        assert np.isfinite(b).all()
        assert_bits(b, a, "fold switch off / on")
