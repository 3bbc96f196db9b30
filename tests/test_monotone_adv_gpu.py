"""MonotoneAdv on the GPU (omega_amd/csrc/MonotoneAdv.h, kernels/MonotoneAdvKernels.hip) and its attachment to the
Split-Explicit stepper.

The yardstick of the call is the restatement (tests/monotone_adv_reference.py): the outputs are seeded with NaN -- the
tendency everywhere but on the entries the call accumulates onto, the scale factors everywhere -- and read back raw, row
padding, sentinel row and the planes >= NTracers included; every entry must hold the restatement's bits or its seed, and
the inputs what was uploaded.  The yardstick of the attached step is the sequence SplitExplicitStepper.h documents,
issued through the public calls."""
import numpy as np
import pytest

import omega_amd as oa
from tests import monotone_adv_reference as MR
from tests.monotone_adv_fixtures import RANDOM, STEP, Inputs, MonoRig
from tests.rank_rig import raw
from tests.split_explicit_fixtures import StepRig
from tests.test_monotone_adv import margin, margin_value

pytestmark = pytest.mark.gpu

MAXT = 9
# one- and two-level lanes (odd / even K), rows shorter than a line, line-aligned and padded rows (37 -> 48, 80),
# level chunks spread over gridDim.y (80 levels on these small meshes)
LEVELS = (1, 2, 15, 16, 37, 80)


@pytest.fixture(scope="module", autouse=True)
def _device():
    oa.device_init(0)


def bits_equal(a, b):
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def assert_bits(got, want, name):
    assert got.shape == want.shape, name
    bad = ~bits_equal(np.ascontiguousarray(got), np.ascontiguousarray(want))
    assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


class Dev:
    """the inputs of `I` on the device (NaN in the level padding) and a MonotoneAdv of MaxTracers planes"""

    def __init__(self, R, I, max_tracers=MAXT):
        self.R, self.I, self.maxt = R, I, max_tracers
        self.K, self.pitch = R.K, oa.level_pitch(R.K)
        self.host = {n: self.padded(getattr(I, n)) for n in ("h_old", "h_new", "u", "tracers")}
        self.buf = {n: oa.DeviceBuffer(a) for n, a in self.host.items()}
        self.shape = (max_tracers, R.nc_size, self.pitch)
        self.tend = oa.DeviceBuffer(np.zeros(self.shape))
        self.mono = oa.MonotoneAdv(R.mesh, R.K, max_tracers, I.upwind)
        rng = np.random.default_rng(5)
        self.tend0 = rng.uniform(-1.0e-3, 1.0e-3, (max_tracers, R.nc_size, R.K))

    def padded(self, a):
        pad = np.full(a.shape[:-1] + (self.pitch,), np.nan)
        pad[..., : self.K] = a
        return pad

    def seed(self, nt):
        """(tendency seed, scale seed) as uploaded"""
        t = np.full(self.shape, np.nan)
        t[:nt, : self.R.nc, : self.K] = self.tend0[:nt, : self.R.nc]
        s = np.full(self.shape, np.nan)
        oa.copy_to_device(self.tend.ptr, t)
        for name in ("ScaleIn", "ScaleOut"):
            oa.copy_to_device(self.mono.device_ptr(name), s)
        return t, s

    def run(self, nt, stream=None, dt=None):
        b = self.buf
        self.mono.add_tracers(self.tend.ptr, b["h_old"].ptr, b["h_new"].ptr, b["u"].ptr, b["tracers"].ptr, nt,
                              self.I.dt if dt is None else dt, stream)

    def read(self):
        oa.device_synchronize()
        return (self.tend.to_host(), raw(self.mono.device_ptr("ScaleIn"), self.shape),
                raw(self.mono.device_ptr("ScaleOut"), self.shape))

    def reference(self):
        """the restatement for all planes, from tend0, once"""
        if not hasattr(self, "_ref"):
            self._ref = self.R.reference(self.I, self.I.tracers.shape[0], self.tend0)
        return self._ref

    def check(self, nt, stream=None):
        R, K = self.R, self.K
        t_seed, s_seed = self.seed(nt)
        self.run(nt, stream)
        if stream is not None:
            stream.synchronize()
        got = self.read()
        for g, want, seed, name in zip(got, self.reference(), (t_seed, s_seed, s_seed), ("Tend", "ScaleIn", "ScaleOut")):
            expect = seed.copy()
            expect[:nt, : R.nc, :K] = want[:nt, : R.nc]
            assert np.isfinite(want[:nt, : R.nc]).all(), name
            assert_bits(g, expect, f"{name} (NT = {nt})")
        for n, a in self.host.items():  # the inputs are what was uploaded
            assert_bits(self.buf[n].to_host(), a, n)
        return got


_CASES = {}


def case(name, K, upwind, nparts=1, rank=0):
    key = (name, K, upwind, nparts, rank)
    if key not in _CASES:
        R = MonoRig(name, K, nparts=nparts, rank=rank, device=True)
        _CASES[key] = Dev(R, R.inputs(seed=3 + K, upwind=upwind, ntracers=MAXT))
    return _CASES[key]


@pytest.mark.parametrize("upwind", (False, True), ids=("centre", "upwind"))
@pytest.mark.parametrize("nt", (1, 2, MAXT))
@pytest.mark.parametrize("K", LEVELS)
@pytest.mark.parametrize("name", ("hex24x20", "fib700_coast_ragged"))
def test_bit_exact_on_nan_seeded_arrays(name, K, nt, upwind):
    D = case(name, K, upwind)
    _, si, so = D.check(nt)
    if nt == MAXT:  # the comparison is about a limiter at work
        r = si[RANDOM, : D.R.nc, :K]
        assert (r < 1.0).any() and (r == 1.0).any() and (so[RANDOM, : D.R.nc, :K] < 1.0).any()


@pytest.mark.parametrize("nt", (3, 4, 5, 7, 8))
def test_every_remainder_of_the_tracer_blocks(nt):
    """the tracers go in blocks of three: whole blocks only, and a remainder of one and of two after one and two blocks"""
    for K in (15, 16):
        case("hex24x20", K, False).check(nt)


def test_launch_shape_with_a_tail_split():
    """hex130x130, K = 32, NT = 2: 2113 tiles of 8 cells, of which the last 65 are tail-split (one level chunk per
    workgroup); derived in tests/test_transport_gpu.py"""
    R = MonoRig("hex130x130", 32, device=True)
    Dev(R, R.inputs(seed=2, ntracers=2, check=False), max_tracers=2).check(2)


def test_stream_forms_agree():
    D = case("hex24x20", 16, False)
    a = D.check(3)
    b = D.check(3, stream=oa.Stream())
    for x, y in zip(a, b):
        assert_bits(x, y, "null stream / stream")


def test_calls_create_no_device_resource():
    D = case("hex24x20", 16, False)
    D.run(2)
    oa.device_synchronize()
    before = oa.device_resource_count()
    for nt in (1, 2, 5, MAXT):
        D.run(nt)
    oa.device_synchronize()
    assert oa.device_resource_count() == before


def test_two_part_decomposition_matches_on_owned_cells():
    """halo width 3: the owned cells, and the halo cells two layers in, have every edge's scale factors right"""
    K, nt = 4, 3
    R1 = MonoRig("hex24x20", K, device=True)
    I1 = R1.inputs(seed=8, ntracers=nt)
    D1 = Dev(R1, I1, nt)
    D1.tend0[:] = 0.0  # (the seed is drawn in local order)
    one = D1.check(nt)
    cid1, eid1 = R1.decomp.get_array("CellID")[: R1.nc] - 1, R1.decomp.get_array("EdgeID")[: R1.ne] - 1
    ncg, neg = cid1.max() + 1, eid1.max() + 1
    glob = {}
    for n, ids, rows in (("h_old", cid1, ncg), ("h_new", cid1, ncg), ("u", eid1, neg)):
        glob[n] = np.zeros((rows, K))
        glob[n][ids] = getattr(I1, n)[: len(ids)]
    glob["tracers"] = np.zeros((nt, ncg, K))
    glob["tracers"][:, cid1] = I1.tracers[:, : R1.nc]
    result = np.zeros((3, nt, ncg, K))
    for w in range(3):
        result[w][:, cid1] = one[w][:nt, : R1.nc, :K]
    for rank in range(2):
        R = MonoRig("hex24x20", K, nparts=2, rank=rank, device=True, halo=3)
        own = R.mesh.NCellsOwned
        assert R.nc > own
        cid, eid = R.decomp.get_array("CellID")[: R.nc] - 1, R.decomp.get_array("EdgeID")[: R.ne] - 1
        I = Inputs()
        I.upwind, I.dt = False, I1.dt
        for n, ids, size in (("h_old", cid, R.nc_size), ("h_new", cid, R.nc_size), ("u", eid, R.ne_size)):
            a = np.full((size, K), np.nan)
            a[: len(ids)] = glob[n][ids]
            setattr(I, n, a)
        I.tracers = np.full((nt, R.nc_size, K), np.nan)
        I.tracers[:, : R.nc] = glob["tracers"][:, cid]
        D = Dev(R, I, nt)
        D.tend0[:] = 0.0
        got = D.check(nt)  # every local cell against the local restatement ...
        for w, name in enumerate(("Tend", "ScaleIn", "ScaleOut")):  # ... and the owned ones against the one-part run
            assert_bits(got[w][:nt, :own, :K], result[w][:, cid[:own]], f"{name} on the owned cells of part {rank}")


def test_one_forward_step_stays_in_range_where_the_centred_term_does_not():
    """update_tracers_by_tend on the fixture's inputs: with the limited tendency the bounds of
    tests/test_monotone_adv.py (i); with the Tendencies' own centred advection term they are left by more than 1e-2"""
    K, nt = 3, 3
    R = MonoRig("hex24x20", K, device=True)
    I = R.inputs(seed=11)
    D = Dev(R, I, nt)
    D.tend0[:] = 0.0
    nc, pitch = R.nc, D.pitch
    nxt = oa.DeviceBuffer(np.zeros(D.shape))

    def update(tend_ptr):
        oa.update_tracers_by_tend(nxt.ptr, D.buf["tracers"].ptr, D.buf["h_new"].ptr, D.buf["h_old"].ptr, tend_ptr, I.dt, nt,
                                  nc, R.nc_size, pitch)
        oa.device_synchronize()
        return nxt.to_host()[:, :nc, :K]

    D.seed(nt)
    D.run(nt)
    new = update(D.tend.ptr)
    bounds = [MR.scale_factors(R.M, I.h_old, I.h_new, I.u, I.tracers[L], I.dt)[2:] for L in range(nt)]
    for L in range(nt):
        over = max((new[L] - bounds[L][1]).max(), (bounds[L][0] - new[L]).max())
        print("limited", L, "outside by", over, "margin", margin(R, I, L))
        assert np.isfinite(new[L]).all() and over <= margin(R, I, L)
    # the built-in term on the same inputs (zero on the sentinel rows: its kernels multiply masks, they do not skip)
    m = R.mesh
    state, trc = oa.OceanState(m, None, K, 2), oa.Tracers(m, None, K, nt, 2)
    aux = oa.AuxiliaryState(m, None, K, nt)
    aux.set_options(False, False, True)
    tend = oa.Tendencies(m, K, nt, oa.default_config(TracerDiffTendencyEnable=0, TracerHyperDiffTendencyEnable=0))
    state.copy_to_device(np.nan_to_num(I.h_old), np.nan_to_num(I.u), 0)
    trc.copy_to_device(np.nan_to_num(I.tracers), 0)
    tend.compute_tracer_tendencies(state, aux, trc, 0, 0, 0)
    new = update(tend.device_ptr(2)[0])
    over = max((new[STEP] - bounds[STEP][1]).max(), (bounds[STEP][0] - new[STEP]).max())
    print("built-in centred term outside by", over)
    assert over > 1.0e-2


# ---------------------------------------------------------------------------------------------------------------------
# the stepper
# ---------------------------------------------------------------------------------------------------------------------
NO_ADV = dict(TracerHorzAdvTendencyEnable=0)


def mono_step_by_hand(x, mono, dt_seconds, nsub, fused):
    """SplitExplicitStepper::doStep with a MonotoneAdv attached, through the public calls on the null stream"""
    p, bm = x.p, x.bm
    m, K, pitch = p.mesh, x.K, oa.level_pitch(x.K)
    dt = oa.coeff_seconds(1.0, dt_seconds)
    st, tend = p.state, p.tend
    h_cur, u_cur, h_next, u_next = st.device_ptr(0, 0), st.device_ptr(1, 0), st.device_ptr(0, 1), st.device_ptr(1, 1)
    tend.set_time(0.0)
    tend.compute_all_tendencies(st, p.aux, p.tracers, 0, 0, 0)
    vel_tend = tend.device_ptr(1)[0]
    bm.split_velocity(h_cur, u_cur, with_ssh=True)
    bm.compute_residual_forcing(h_cur, vel_tend)
    bm.subcycle(nsub, dt / nsub)
    bm.transport_velocity(u_cur, u_next)
    if fused:
        tend.compute_transport_tendencies(st, p.aux, p.tracers, 0, 0, 1)
    else:
        tend.compute_thickness_tendencies(st, p.aux, 0, 1)
        tend.compute_tracer_tendencies(st, p.aux, p.tracers, 0, 0, 1)
    oa.update_by_tend(h_next, h_cur, tend.device_ptr(0)[0], dt, m.NCellsAll, pitch)
    mono.add_tracers(tend.device_ptr(2)[0], h_cur, h_next, u_next, p.tracers.device_ptr(0), x.nt, dt)
    oa.update_tracers_by_tend(p.tracers.device_ptr(1), p.tracers.device_ptr(0), h_next, h_cur, tend.device_ptr(2)[0], dt,
                              x.nt, m.NCellsAll, m.NCellsSize, pitch)
    bm.advance_velocity(u_cur, vel_tend, dt, u_next)
    st.update_time_levels()
    p.tracers.update_time_levels()
    oa.device_synchronize()


@pytest.mark.parametrize("config", (NO_ADV, dict(NO_ADV, TracerDiffTendencyEnable=0, TracerHyperDiffTendencyEnable=0)),
                         ids=("diffusion_terms_on", "every_tracer_term_off"))
@pytest.mark.parametrize("fused", (True, False), ids=("fused_transport", "group_calls"))
@pytest.mark.parametrize("nsub", (1, 7))
def test_attached_step_equals_the_calls_by_hand(nsub, fused, config):
    dt = 20.0
    a, b = StepRig(K=4, attached=False, config=config), StepRig(K=4, attached=False, config=config)
    ma, mb = oa.MonotoneAdv(a.p.mesh, a.K, a.nt), oa.MonotoneAdv(b.p.mesh, b.K, b.nt)
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
    # a step creates no device resource
    before = oa.device_resource_count()
    for _ in range(2):
        st.do_step(a.p.state)
    oa.device_synchronize()
    assert oa.device_resource_count() == before
    # and the limiter was what moved the tracers: the plain step with the same terms differs
    c = StepRig(K=4, attached=False, config=config)
    c.stepper("Split-Explicit", dt, nsub).do_step(c.p.state)
    assert not np.array_equal(c.result()[2], want[2])


def test_eight_steps_keep_a_step_tracer_in_its_range():
    """Dt = 600 s on 30 km hexagons, 4 layers of 8 .. 12 m.  Courant estimate: the random layer thicknesses make a
    surface noise of about +-4 m on 40 m of water, which the barotropic mode turns into |u| <= sqrt(g/H)*eta ~ 2 m/s at
    the very most; the outflow Courant number Dt*|u|*(half the perimeter)/AreaCell = 600*2*(3*17.3 km)/(779 km^2) is then
    below 0.08.  The test measures it on the velocities it ends with and requires it below 0.5."""
    dt, nsub, steps = 600.0, 30, 8
    off = dict(TracerDiffTendencyEnable=0, TracerHyperDiffTendencyEnable=0)
    results = {}
    for limited in (True, False):
        x = StepRig(K=4, attached=False, config=dict(off, TracerHorzAdvTendencyEnable=0 if limited else 1))
        m = x.p.mesh
        xc = m.get_array("XCell")[: m.NCellsAll]
        x.tr[0, : m.NCellsAll] = (xc > np.median(xc)).astype(float)[:, None]
        x.load()
        st = x.stepper("Split-Explicit", dt, nsub)
        if limited:
            mono = oa.MonotoneAdv(m, x.K, x.nt)
            st.attach_monotone_adv(mono)
        h_min, u_max = x.h[: m.NCellsAll].min(), 0.0
        for _ in range(steps):
            st.do_step(x.p.state)
            h, u, _ = x.result()
            h_min, u_max = min(h_min, h[: m.NCellsAll].min()), max(u_max, np.abs(u[: m.NEdgesAll]).max())
        h, u, tr = x.result()
        area, dv = m.get_array("AreaCell")[: m.NCellsAll], m.get_array("DvEdge")[: m.NEdgesAll]
        courant = dt * u_max * 3.0 * dv.max() / area.min()
        print("limited" if limited else "centred", "Courant estimate", courant, "min h", h_min)
        assert np.isfinite(tr).all() and h_min > 0.0 and courant < 0.5
        results[limited] = (tr[:, : m.NCellsAll], h, h_min)
    n = m.get_array("EdgesOnCell").shape[1]
    for L in range(2):
        lo, hi = x.tr[L, : m.NCellsAll].min(), x.tr[L, : m.NCellsAll].max()
        tr, h, h_min = results[True]
        # the margin of tests/test_monotone_adv.py (i), once per step
        mg = steps * margin_value(n, h.max(), max(abs(lo), abs(hi)), h_min)
        over = max(tr[L].max() - hi, lo - tr[L].min())
        print("tracer", L, "outside its initial range by", over, "margin", mg)
        assert over <= mg
    tr, h, h_min = results[False]
    over = max(tr[0].max() - 1.0, 0.0 - tr[0].min())
    print("centred: outside by", over)
    assert over > steps * margin_value(n, h.max(), 1.0, h_min) and not np.array_equal(tr, results[True][0])


def test_refusals():
    K, nt = 4, 2
    x = StepRig(K=K, attached=False, config=NO_ADV)
    m = x.p.mesh
    E = oa.OmegaAmdError
    # the constructor
    with pytest.raises(E, match="invalid argument"):
        oa.MonotoneAdv(None, K, nt)
    with pytest.raises(E, match="host-only"):
        oa.MonotoneAdv(oa.HorzMesh(x.p.decomp, K, host_only=True), K, nt)
    for bad in (0, -3):
        with pytest.raises(E, match="MaxTracers"):
            oa.MonotoneAdv(m, K, bad)
    with pytest.raises(E, match="NVertLayers"):
        oa.MonotoneAdv(m, 0, nt)
    # the call
    mono = oa.MonotoneAdv(m, K, nt)
    st = x.p.state
    args = (x.p.tend.device_ptr(2)[0], st.device_ptr(0, 0), st.device_ptr(0, 1), st.device_ptr(1, 0), x.p.tracers.device_ptr(0))
    for bad in (0, -1, nt + 1):
        with pytest.raises(E, match="NTracers"):
            mono.add_tracers(*args, bad, 10.0)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(E, match="not finite and positive"):
            mono.add_tracers(*args, nt, bad)
    # the attachment
    with pytest.raises(E, match="not a Split-Explicit"):
        x.stepper("RungeKutta4", 20.0).attach_monotone_adv(mono)
    step = x.stepper("Split-Explicit", 20.0, 2)
    with pytest.raises(E, match="another mesh or layer count"):
        step.attach_monotone_adv(oa.MonotoneAdv(oa.HorzMesh(x.p.decomp, K), K, nt))
    with pytest.raises(E, match="another mesh or layer count"):
        step.attach_monotone_adv(oa.MonotoneAdv(m, K + 1, nt))
    with pytest.raises(E, match="MaxTracers = 1"):
        step.attach_monotone_adv(oa.MonotoneAdv(m, K, 1))
    with pytest.raises(E, match="FluxThicknessUpwind differs"):
        step.attach_monotone_adv(oa.MonotoneAdv(m, K, nt, flux_thickness_upwind=True))
    y = StepRig(K=K, attached=False)  # the Tendencies' own advection term is on
    with pytest.raises(E, match="TracerHorzAdvTendencyEnable is on"):
        y.stepper("Split-Explicit", 20.0, 2).attach_monotone_adv(oa.MonotoneAdv(y.p.mesh, K, nt))
    # doStep checks again: the option changed after the attachment
    step.attach_monotone_adv(mono)
    step.do_step(st)
    x.p.aux.set_options(True, False, True)
    with pytest.raises(E, match="doStep: the MonotoneAdv's FluxThicknessUpwind differs"):
        step.do_step(st)
    x.p.aux.set_options(False, False, True)
    step.attach_monotone_adv(None)
    step.do_step(st)
    oa.device_synchronize()


def test_nothing_attached_is_the_step_it_was():
    """attached and detached again: the bits of a stepper that never saw a MonotoneAdv, and no device resource made by
    the steps; graph statistics untouched"""
    runs = []
    for touch in (False, True):
        x = StepRig(K=4, attached=False, config=NO_ADV)
        st = x.stepper("Split-Explicit", 20.0, 3)
        if touch:
            st.attach_monotone_adv(oa.MonotoneAdv(x.p.mesh, x.K, x.nt))
            st.attach_monotone_adv(None)
        st.do_step(x.p.state)
        oa.device_synchronize()
        before = oa.device_resource_count()
        st.do_step(x.p.state)
        oa.device_synchronize()
        assert oa.device_resource_count() == before and st.graph_stats() == {"captures": 0, "replays": 0}
        runs.append(x.result())
    for a, b in zip(*runs):
        assert_bits(a, b, "never attached / detached")
