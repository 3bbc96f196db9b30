"""VertAdv on the GPU: each of the four methods equals the NumPy restatement of the contract
(tests/vert_adv_reference.py) bit for bit on NaN-seeded arrays -- entries outside the ranges, the row padding, rows
>= N*All and the sentinel row are NaN and must stay so; the combined launch equals the two calls; the stream and
null-stream forms agree; attached to Tendencies the three tendencies are "plain RHS, then the restatement", before an
attached PressureGrad; RK4, RK2 and FB keep each cell's total thickness and a constant tracer; a 2-part decomposition
gives the 1-part values; bad arguments are refused."""
import numpy as np
import pytest

import omega_amd as oa
from tests import pressure_grad_reference as PR
from tests import vert_adv_reference as VR
from tests.column_reference import RHO0
from tests.meshes import named_mesh
from tests.vert_adv_fixtures import AdvRig, adv_inputs, assert_both_signs
from tests.vert_fixtures import same as _same

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
MESHES = ("hex24x20", "fib700_coast_ragged")
LEVELS = (1, 2, 15, 16, 37, 80)
TRACERS = (1, 2, 9)
STEPPERS = ("RungeKutta4", "RungeKutta2", "Forward-Backward")


@pytest.fixture(scope="module", autouse=True)
def _device():
    oa.device_init(0)


@pytest.mark.parametrize("K", LEVELS)
@pytest.mark.parametrize("mesh", MESHES)
def test_bit_exact_on_nan_seeded_arrays(mesh, K):
    x = AdvRig(named_mesh(mesh), K, max(TRACERS))
    d = x.seeded(x.d)
    want_wt = x.want_transport(d)
    cnt = assert_both_signs(want_wt, x.lo, x.hi, x.n_all)
    assert (cnt > 0) == (K > 1)
    # the transport, and nothing else
    for order in (2, 1):
        x.poison_transport(order)
        buf = x.dev(d)
        x.va[order].compute_transport(buf.ptr)
        oa.device_synchronize()
        _same(x.transport_padded(order), x.padded(want_wt), "VerticalTransport")
        _same(buf.to_host(), x.padded(d), "the tendency handed in")
    assert np.isfinite(want_wt[x.active]).all() and x.active.any()
    # the thickness update from the transport as it stands
    buf = x.dev(d)
    x.va[2].add_thickness(buf.ptr)
    oa.device_synchronize()
    want_th = VR.add_thickness_tend(d.copy(), want_wt, x.lo, x.hi, x.n_all)
    _same(buf.to_host(), x.padded(want_th), "LayerThicknessTend")
    _same(x.transport_padded(), x.padded(want_wt), "VerticalTransport after addThicknessTend")
    # the combined launch
    x.poison_transport()
    buf = x.dev(d)
    x.va[2].compute_transport(buf.ptr, add_thickness=True)
    oa.device_synchronize()
    _same(buf.to_host(), x.padded(want_th), "LayerThicknessTend (combined launch)")
    _same(x.transport_padded(), x.padded(want_wt), "VerticalTransport (combined launch)")
    if K > 1:
        assert not np.array_equal(want_th[x.active], d[x.active])
    # tracers: every count, both orders; planes beyond the count are not touched
    h, tr = x.dev(x.seeded(x.h)), x.dev(x.seeded(x.tr))
    t0 = x.seeded(x.tr * 1.0e-3)
    for order in (2, 1):
        for nt in TRACERS:
            buf = x.dev(t0)
            x.va[order].add_tracers(buf.ptr, h.ptr, tr.ptr, nt)
            oa.device_synchronize()
            want = t0.copy()
            VR.add_tracer_tend(want[:nt], x.seeded(x.h), x.seeded(x.tr)[:nt], want_wt, x.lo, x.hi, x.n_all, order)
            _same(buf.to_host(), x.padded(want), f"TracerTend (order {order}, {nt} tracers)")
            if K > 1:
                assert not np.array_equal(want[:nt, x.active], t0[:nt, x.active])
    # velocity
    u0 = x.seeded(x.u * 1.0e-2, edge=True)
    buf, u = x.dev(u0), x.dev(x.seeded(x.u, edge=True))
    x.va[2].add_velocity(buf.ptr, h.ptr, u.ptr)
    oa.device_synchronize()
    want = VR.add_velocity_tend(u0.copy(), x.seeded(x.h), x.seeded(x.u, edge=True), want_wt, x.coe, x.mask, x.lo_e,
                                x.hi_e, x.e_all)
    _same(buf.to_host(), x.padded(want), "NormalVelocityTend")
    assert np.isfinite(want[x.e_active]).all()
    if K > 1:
        assert not np.array_equal(want[x.e_active], u0[x.e_active])
    if "coast" in mesh:
        assert (~x.active[: x.n_all]).all(axis=1).any() and (~x.e_active[: x.e_all]).all(axis=1).any()  # land
    if K > 2:
        assert (x.lo[: x.n_all] > 0).any()  # KMin > 0
    # the numpy forms of the binding
    got = x.va[2].add_thickness(np.nan_to_num(d))
    _same(got, VR.add_thickness_tend(np.nan_to_num(d), np.nan_to_num(want_wt), x.lo, x.hi, x.n_all), "numpy form")


def test_stream_and_null_stream_forms_agree():
    g = named_mesh("fib700_coast_ragged")
    s = oa.Stream()
    out = []
    for st in (None, s):
        x = AdvRig(g, 37, 2)
        x.poison_transport()
        d, d2 = x.dev(x.seeded(x.d)), x.dev(x.seeded(x.d))
        h, tr, u = x.dev(x.h), x.dev(x.tr), x.dev(x.u)
        tt, ut = x.dev(x.tr * 1.0e-3), x.dev(x.u * 1.0e-2)
        x.va[2].compute_transport(d.ptr, stream=st)
        x.va[2].add_thickness(d.ptr, stream=st)
        x.va[2].compute_transport(d2.ptr, add_thickness=True, stream=st)
        x.va[2].add_tracers(tt.ptr, h.ptr, tr.ptr, 2, stream=st)
        x.va[2].add_velocity(ut.ptr, h.ptr, u.ptr, stream=st)
        if st is not None:
            st.synchronize()
        oa.device_synchronize()
        out.append([b.to_host() for b in (d, d2, tt, ut)] + [x.transport_padded()])
    for p, q in zip(*out):
        _same(q, p, "stream form")


def _poison_tend(x):
    pitch = oa.level_pitch(x.K)
    for which, rows, planes in ((0, x.n_size, 1), (1, x.e_size, 1), (2, x.n_size, x.nt)):
        ptr, _ = x.tend.device_ptr(which)
        poison = np.full((planes, rows, pitch), np.nan)
        poison[:, -1, :] = 0.0
        oa.copy_to_device(ptr, poison)


def _rhs(x, stream=None):
    _poison_tend(x)
    x.tend.compute_all_tendencies(x.state, x.aux, x.tracers, stream=stream)
    if stream is not None:
        stream.synchronize()
    oa.device_synchronize()
    return [x.tend.get(i) for i in range(3)]


def _restated(x, base, order, wt=None):
    """plain RHS, then the restatement: (thickness, velocity, tracers, transport)"""
    if wt is None:
        wt = VR.vertical_transport(base[0], x.ref, x.w, x.lo, x.hi, x.n_all, np.zeros((x.n_size, x.K)))
    th = VR.add_thickness_tend(base[0].copy(), wt, x.lo, x.hi, x.n_all)
    tt = VR.add_tracer_tend(base[2].copy(), x.h, x.tr, wt, x.lo, x.hi, x.n_all, order)
    ut = VR.add_velocity_tend(base[1].copy(), x.h, x.u, wt, x.coe, x.mask, x.lo_e, x.hi_e, x.e_all)
    return th, ut, tt, wt


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "reference_structured"])
@pytest.mark.parametrize("mesh,K,nt,order", [("hex24x20", 16, 2, 2), ("fib700_coast_ragged", 37, 9, 1),
                                             ("fib700_coast_ragged", 15, 1, 2)])
def test_attached_rhs_is_plain_rhs_then_the_terms(mesh, K, nt, order, fused):
    x = AdvRig(named_mesh(mesh), K, nt, config={})
    x.vc.set("RefLayerThickness", x.ref)
    x.tend.set_fused(fused)
    oa.device_synchronize()
    before = oa.device_resource_count()
    base = _rhs(x)
    x.tend.attach_vert_adv(x.va[order])
    got = _rhs(x)
    th, ut, tt, wt = _restated(x, base, order)
    assert_both_signs(wt, x.lo, x.hi, x.n_all)
    _same(got[0], th, "LayerThicknessTend")
    _same(got[1], ut, "NormalVelocityTend")
    _same(got[2], tt, "TracerTend")
    _same(np.where(x.active, x.va[order].get("VerticalTransport"), 0.0), np.where(x.active, wt, 0.0), "VerticalTransport")
    for a, b in zip(got, base):
        assert not np.array_equal(a, b, equal_nan=True)
    # the group methods: the thickness group computes the transport, the other two use it as it stands
    x.tend.attach_vert_adv(None)
    x.tend.compute_thickness_tendencies(x.state, x.aux)
    x.tend.compute_velocity_tendencies(x.state, x.aux)
    x.tend.compute_tracer_tendencies(x.state, x.aux, x.tracers)
    oa.device_synchronize()
    plain = [x.tend.get(i) for i in range(3)]
    x.tend.attach_vert_adv(x.va[order])
    x.tend.compute_thickness_tendencies(x.state, x.aux)
    oa.device_synchronize()
    th2, _, _, wt2 = _restated(x, plain, order)
    _same(x.tend.get(0), th2, "LayerThicknessTend (thickness group)")
    other = np.where(x.active, wt2 * 0.5 + 1.0e-5, 0.0)
    x.va[order].set("VerticalTransport", other)
    x.tend.compute_velocity_tendencies(x.state, x.aux)
    x.tend.compute_tracer_tendencies(x.state, x.aux, x.tracers)
    oa.device_synchronize()
    _, ut2, tt2, _ = _restated(x, plain, order, other)
    _same(x.tend.get(1), ut2, "NormalVelocityTend (velocity group)")
    _same(x.tend.get(2), tt2, "TracerTend (tracer group)")
    # detached: the plain bits again, and nothing was allocated on the way
    x.tend.attach_vert_adv(None)
    for a, b, name in zip(_rhs(x), base, ("LayerThicknessTend", "NormalVelocityTend", "TracerTend")):
        _same(a, b, name + " (detached)")
    assert oa.device_resource_count() == before


def test_nothing_attached_is_the_plain_rhs_with_the_same_counters():
    """two Tendencies on one mesh, one of which had a VertAdv attached and detached: the same bits, the same fused
    kernels recorded by the kernel timer, the same graph statistics, the same resources per evaluation"""
    x = AdvRig(named_mesh("hex24x20"), 16, 2, config={})
    cfg = oa.default_config()
    other = oa.Tendencies(x.mesh, x.K, x.nt, cfg)
    x.tend.attach_vert_adv(x.va[2])
    x.tend.attach_vert_adv(None)
    stats = []
    for t in (x.tend, other):
        t.kernel_timing(True)
        oa.device_synchronize()
        r0 = oa.device_resource_count()
        t.compute_all_tendencies(x.state, x.aux, x.tracers)
        oa.device_synchronize()
        r1 = oa.device_resource_count()
        names = [k for k, _ in t.collect_kernel_times()]
        t.kernel_timing(False)
        stats.append(([t.get(i) for i in range(3)], names, t.graph_stats(), r1 - r0))
    for a, b in zip(stats[0][0], stats[1][0]):
        _same(a, b, "tendencies")
    assert stats[0][1:] == stats[1][1:] and len(stats[0][1]) > 0


def test_attached_with_pressure_grad_vert_adv_comes_first():
    """NormalVelocityTend = (plain - vertical advection) - pressure gradient, in that order"""
    g, K, nt = named_mesh("fib700_coast_ragged"), 16, 2
    x = AdvRig(g, K, nt, config=dict(SSHTendencyEnable=0))
    x.vc.set("RefLayerThickness", x.ref)
    rng = np.random.default_rng(11)
    x.vc.set("BottomDepth", np.concatenate([rng.uniform(100.0, 6000.0, x.n_all), np.zeros(x.n_size - x.n_all)]))
    eos = oa.Eos(x.mesh, K, "teos10")
    pg = oa.PressureGrad(x.mesh, x.vc, eos)
    base = _rhs(x)
    x.tend.attach_vert_adv(x.va[2])
    x.tend.attach_pressure_grad(pg)
    got = _rhs(x)
    th, ut, tt, _ = _restated(x, base, 2)
    fields = (x.vc.get("PressureMid"), x.vc.get("GeopotentialMid"), eos.get("SpecVol"))
    dc = x.mesh.get_array("DcEdge")
    first = PR.pressure_grad(ut.copy(), *fields, x.coe, dc, x.mask, x.lo_e, x.hi_e, x.e_all)
    _same(got[1], first, "NormalVelocityTend")
    _same(got[0], th, "LayerThicknessTend")
    _same(got[2], tt, "TracerTend")
    # the other order gives other bits somewhere: the test can tell them apart
    pg_first = PR.pressure_grad(base[1].copy(), *fields, x.coe, dc, x.mask, x.lo_e, x.hi_e, x.e_all)
    second = VR.add_velocity_tend(pg_first, x.h, x.u, VR.vertical_transport(
        base[0], x.ref, x.w, x.lo, x.hi, x.n_all, np.zeros((x.n_size, K))), x.coe, x.mask, x.lo_e, x.hi_e, x.e_all)
    assert not np.array_equal(second, first, equal_nan=True)


STEP_CONFIG = dict(PVTendencyEnable=0, KETendencyEnable=0, SSHTendencyEnable=0, VelDiffTendencyEnable=0,
                   VelHyperDiffTendencyEnable=0, WindForcingTendencyEnable=0, BottomDragTendencyEnable=0,
                   TracerDiffTendencyEnable=0, TracerHyperDiffTendencyEnable=0, FluxThicknessUpwind=0, FluxTracerUpwind=0)


@pytest.mark.parametrize("kind", STEPPERS)
def test_steppers_keep_total_thickness_and_a_constant_tracer(kind):
    """Thickness and tracer advection by a frozen, vertically uniform velocity (every velocity term off) with centred
    edge values: the horizontal thickness tendency is linear in h level by level, so its column sum depends on the
    column's total thickness only, and the vertical transport moves thickness between the layers of a column without
    changing their sum (W[KMin] = 0).  Each cell's total thickness therefore evolves as in the unattached run.
    Rounding: a stage update h + c dt Tend rounds each level by eps/2 |h|, a column of K levels by K eps/2 max h <=
    eps/2 H with H the largest total thickness times the spread max h / mean h <= 2.5; RK4 applies 8 such operations
    per step (4 provisional states, 4 accumulations), the others fewer; two runs, 3 steps, and the sum taken here:
    within 2 * 3 * 8 * 1.25 eps H + K eps/2 H <= 70 eps H.  A constant tracer stays constant to 1e-13 relative."""
    g, K, nt, dt, steps, phi0 = named_mesh("hex24x20"), 16, 2, 10.0, 3, 34.7
    G = adv_inputs(g, K, nt)
    G["un"] = np.repeat(G["un"][:, :1], K, axis=1)
    G["tr"] = np.full_like(G["tr"], phi0)
    runs = []
    for attach in (True, False):
        x = AdvRig(g, K, nt, config=STEP_CONFIG, G=G)
        x.vc.set("RefLayerThickness", x.ref)
        if attach:
            x.tend.attach_vert_adv(x.va[2])
        st = oa.TimeStepper(kind, dt, x.tend, x.aux, x.mesh, None, x.tracers)
        s = oa.Stream()
        st.do_step(x.state, stream=s)  # (whatever a stepper sets up at its first step)
        s.synchronize()
        oa.device_synchronize()
        before = oa.device_resource_count()
        for _ in range(steps - 1):
            st.do_step(x.state, stream=s)
        s.synchronize()
        oa.device_synchronize()
        assert oa.device_resource_count() == before  # no step allocates
        runs.append((x, x.state.copy_to_host(0)[0], x.tracers.copy_to_host(0)))
    (x, h_att, tr_att), (_, h_plain, _) = runs
    n = x.n_all
    tot_att, tot_plain, tot0 = h_att[:n].sum(axis=1), h_plain[:n].sum(axis=1), x.h[:n].sum(axis=1)
    err = np.abs(tot_att - tot_plain).max()
    print(f"{kind}: max |total thickness attached - plain| = {err:.3e} = {err / (EPS * tot0.max()):.2f} eps H; "
          f"max |change of total| = {np.abs(tot_plain - tot0).max():.3e}; "
          f"max |h attached - plain| = {np.abs(h_att[:n] - h_plain[:n]).max():.3e}")
    assert err <= 70.0 * EPS * tot0.max()
    assert np.abs(tot_plain - tot0).max() > 1.0e6 * EPS * tot0.max()  # the totals did move
    assert np.abs(h_att[:n] - h_plain[:n]).max() > 1.0e6 * EPS * x.h.max()  # and the layers moved differently
    assert np.isfinite(h_att[:n]).all() and h_att[:n][x.active[:n]].min() > 0.0
    dev = np.abs(tr_att[:, :n] / phi0 - 1.0).max()
    print(f"{kind}: max relative deviation of the constant tracer = {dev:.3e}")
    assert dev <= 1.0e-13


@pytest.mark.parametrize("mesh,K", [("hex24x20", 37), ("fib700_coast_ragged", 16)])
def test_two_part_decomposition_matches_one_part(mesh, K):
    g, nt = named_mesh(mesh), 2

    def run(nparts, rank):
        x = AdvRig(g, K, nt, nparts=nparts, rank=rank)
        x.vc.set("RefLayerThickness", x.ref)
        d, tt, ut = x.dev(x.d), x.dev(x.tr * 1.0e-3), x.dev(x.u * 1.0e-2)
        h, tr, u = x.dev(x.h), x.dev(x.tr), x.dev(x.u)
        x.va[2].compute_transport(d.ptr, add_thickness=True)
        x.va[2].add_tracers(tt.ptr, h.ptr, tr.ptr, nt)
        x.va[2].add_velocity(ut.ptr, h.ptr, u.ptr)
        oa.device_synchronize()
        return x, d.to_host(), tt.to_host(), ut.to_host(), x.va[2].get("VerticalTransport")

    one, d1, tt1, ut1, wt1 = run(1, 0)
    cell1 = {int(c): i for i, c in enumerate(one.cid[: one.n_all])}
    edge1 = {int(e): i for i, e in enumerate(one.eid[: one.e_all])}
    for rank in (0, 1):
        x, d, tt, ut, wt = run(2, rank)
        ci = np.array([cell1[int(c)] for c in x.cid[: x.n_own]])
        ei = np.array([edge1[int(e)] for e in x.eid[: x.e_own]])
        _same(d[: x.n_own], d1[ci], f"LayerThicknessTend rank {rank}")
        _same(wt[: x.n_own], wt1[ci], f"VerticalTransport rank {rank}")
        _same(tt[:, : x.n_own], tt1[:, ci], f"TracerTend rank {rank}")
        _same(ut[: x.e_own], ut1[ei], f"NormalVelocityTend rank {rank}")
        assert x.n_own < one.n_own


def test_refusals():
    g = named_mesh("hex24x20")
    x, y = AdvRig(g, 16, 2, config={}), AdvRig(g, 15, 2, config={})
    with pytest.raises(oa.OmegaAmdError, match="TracerFluxOrder = 3"):
        oa.VertAdv(x.mesh, x.vc, 3)
    with pytest.raises(oa.OmegaAmdError, match="TracerFluxOrder = 0"):
        oa.VertAdv(x.mesh, x.vc, 0)
    with pytest.raises(oa.OmegaAmdError, match="another mesh"):
        oa.VertAdv(x.mesh, y.vc, 2)
    with pytest.raises(oa.OmegaAmdError, match="VertCoord is NULL"):
        oa.VertAdv(x.mesh, None, 2)
    with pytest.raises(oa.OmegaAmdError, match="another mesh or layer count"):
        x.tend.attach_vert_adv(y.va[2])
    # a VertCoord of the same mesh with another layer count
    short = oa.VertCoord(x.mesh, 8, RHO0, "Uniform")
    with pytest.raises(oa.OmegaAmdError, match="another layer count"):
        oa.VertAdv(x.mesh, short, 2)
    # columns too long for the LDS tile: the message names the limit
    limit = oa.VertAdv.max_layers()
    assert limit >= 1024
    small = named_mesh("hex24x20")
    gm = oa.GlobalMesh(small)
    decomp = oa.Decomp(gm, 1, 0, 3)
    for K, ok in ((limit, True), (limit + 1, False)):
        m = oa.HorzMesh(decomp, K)
        vc = oa.VertCoord(m, K, RHO0, "Uniform", decomp=decomp)
        if ok:
            va = oa.VertAdv(m, vc, 2)
            d = np.random.default_rng(1).uniform(-1.0e-3, 1.0e-3, (m.NCellsSize, K))
            vc.set("RefLayerThickness", np.ones((m.NCellsSize, K)))
            got = va.compute_transport(d.copy(), add_thickness=True)
            lo, hi = np.zeros(m.NCellsSize, np.int32), np.full(m.NCellsSize, K - 1, np.int32)
            wt = VR.vertical_transport(d, np.ones((m.NCellsSize, K)), np.ones(K), lo, hi, m.NCellsAll,
                                       np.zeros((m.NCellsSize, K)))
            _same(got, VR.add_thickness_tend(d.copy(), wt, lo, hi, m.NCellsAll), "the longest column")
        else:
            with pytest.raises(oa.OmegaAmdError, match=f"NVertLayers <= {limit}"):
                oa.VertAdv(m, vc, 2)
