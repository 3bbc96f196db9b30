"""GentMcWilliams on the GPU: the kernel equals the NumPy restatement of the contract (tests/gent_mcwilliams_reference.py)
bit for bit on NaN-seeded outputs -- entries outside each edge's range, the sentinel row and the row padding are NaN and
must stay so -- at every layer count at which the launch changes shape; the two compute forms and the two stream forms
agree; a given Transport takes Transport + BolusVelocity; updateColumn leaves the fields VertMix's N^2 is made of; attached
to the split-explicit stepper a step equals the public calls made by hand, the bolus flow moves the tracers (and the
thickness, where the layers are not held to z-star) and never reaches the velocity, the transporting velocity still carries the sub-cycle's mean flux, no step allocates,
and detaching restores the unattached bits; the refusals that need a device."""
from fractions import Fraction

import numpy as np
import pytest

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests import gent_mcwilliams_reference as GR
from tests import pressure_grad_reference as PR
from tests import vert_mix_reference as MR
from tests.column_reference import RHO0
from tests.meshes import named_mesh
from tests.rank_rig import RankRig, raw
from tests.split_explicit_fixtures import StepRig
from tests.vert_fixtures import (FUSED, STAGE_SPEC_VOL_DISP, column_limit, level_pitch, mix_inputs, pcr_levels,
                                 same as _same, systems_launch)

pytestmark = pytest.mark.gpu

NT = 2
EPS = np.finfo(np.float64).eps
KAPPA, SPEED = 450.0, 0.25
MESHES = ("hex24x20", "fib300_coast_ragged")
LEVELS = (1, 2, 3, 5, 15, 16, 17, 64, 85, 86, 128, 129, 255, 256, 257, 512, 513, 1024)
CASES = [(m, K, e) for m in MESHES for K in LEVELS for e in ("teos10", "linear")]
COLUMN_LIMIT = column_limit(FUSED | STAGE_SPEC_VOL_DISP)  # the column pass with the displaced volume
LDS_BYTES, MAX_ROWS, LANES, LDS_ARRAYS = 65536, 1024, 256, 7


def gm_launch(K):
    """launchBolusVelocity (kernels/GMKernels.hip), restated: columns per workgroup, the lanes they occupy, the lanes of
    the workgroup, its pad lanes and its dynamic LDS (seven doubles per occupied lane)"""
    sys, rows, threads = systems_launch(K)
    return dict(Sys=sys, Rows=rows, Threads=threads, PadLanes=threads - rows, LdsBytes=LDS_ARRAYS * rows * 8)


@pytest.fixture(scope="module", autouse=True)
def _device():
    oa.device_init(0)


def synthetic_fields(rng, h):
    """(SpecVol, SpecVolDisplaced, ZMid) for layer counts beyond the column pass: heights monotone in z, density
    increasing downward, the displaced parcel a quarter of the way to the layer below (N^2 > 0)"""
    n, K = h.shape
    z = -(np.cumsum(h, axis=1) - 0.5 * h) + rng.uniform(-0.1, 0.1, (n, 1))
    rho = 1020.0 + rng.uniform(0.0, 0.5, (n, 1)) + np.cumsum(rng.uniform(1.0e-4, 2.0e-3, (n, K)), axis=1)
    disp = rho + 1.0e-4
    disp[:, :-1] = rho[:, :-1] + 0.25 * (rho[:, 1:] - rho[:, :-1])
    return 1.0 / rho, 1.0 / disp, z


class Rig(RankRig):
    """One rank's VertCoord, Eos and GentMcWilliams on global inputs (tests.vert_fixtures.mix_inputs: layer ranges with
    land, KMin > 0, single layers) in local order, a per-edge Kappa with zeros in it, and the column fields: from
    update_column up to the column pass's limit, synthetic beyond it (handed to the array form)."""

    def __init__(self, g, K, eos_kind, seed=7, full=False):
        super().__init__(g, K)
        self.P = level_pitch(K)
        m = self.mesh
        G = mix_inputs(g, K, seed, full, NT)
        rng = self.rng = np.random.default_rng(seed + 100)
        n = int(g["nCells"])
        self.h, self.tr = self.cells(G["h"]), self.cells(G["tr"])
        self.layers(G["min_level"], G["max_level"])
        self.vc.set("BottomDepth", self.cells(rng.uniform(100.0, 6000.0, n)))
        self.eos = oa.Eos(m, K, eos_kind)
        self.gm = oa.GentMcWilliams(m, self.vc, self.eos, kappa=KAPPA, grav_wave_speed=SPEED)
        assert np.all(self.gm.get("Kappa") == KAPPA)  # GMKappa at construction
        for name, v in (("SurfacePressure", rng.uniform(0.9e5, 1.1e5, n)), ("TidalPotential", rng.uniform(-1.0, 1.0, n)),
                        ("SelfAttractionLoading", rng.uniform(-0.1, 0.1, n))):
            assert np.all(self.gm.get(name) == 0.0)  # zero at construction
            self.gm.set(name, self.cells(v))
        for name in ("BolusVelocity", "StreamFunction"):
            assert np.all(raw(self.gm.device_ptr(name), (self.e_size, self.P)) == 0.0)
        self.kappa = rng.uniform(100.0, 900.0, self.e_size)
        self.kappa[::7] = 0.0
        self.gm.set("Kappa", self.kappa)
        self.coe, self.dc = m.get_array("CellsOnEdge"), m.get_array("DcEdge")
        self.column_pass = K <= COLUMN_LIMIT
        self.synthetic = None if self.column_pass else synthetic_fields(rng, self.h)

    def poison(self):
        """both outputs NaN everywhere, padding and sentinel row included"""
        for name in ("BolusVelocity", "StreamFunction"):
            oa.copy_to_device(self.gm.device_ptr(name), np.full((self.e_size, self.P), np.nan))

    def update_column(self, stream=None):
        for name in ("SpecVol", "SpecVolDisplaced"):
            self.eos.set(name, np.full((self.n_size, self.K), np.nan))
        self.vc.set("ZMid", np.full((self.n_size, self.K), np.nan))
        self.gm.update_column(self.h, self.tr, NT, stream=stream)
        oa.device_synchronize()

    def fields(self):
        if self.synthetic is not None:
            return self.synthetic
        return self.eos.get("SpecVol"), self.eos.get("SpecVolDisplaced"), self.vc.get("ZMid")

    def compute(self, transport=None, array_form=None, stream=None):
        """the attached form where the column pass ran, else the array form on the synthetic fields"""
        array_form = self.synthetic is not None if array_form is None else array_form
        extra = dict(zip(("spec_vol", "spec_vol_displaced", "z_mid"), self.fields())) if array_form else {}
        self.gm.compute(self.h, transport, stream=stream, **extra)
        if stream is not None:
            stream.synchronize()
        oa.device_synchronize()

    def outputs(self):
        return {name: raw(self.gm.device_ptr(name), (self.e_size, self.P)) for name in ("BolusVelocity", "StreamFunction")}

    def restated(self, transport=None):
        u, psi = np.full((self.e_size, self.K), np.nan), np.full((self.e_size, self.K), np.nan)
        GR.bolus_velocity(self.h, *self.fields(), self.coe, self.dc, self.kappa, self.lo_e, self.hi_e, self.e_all, RHO0,
                          SPEED, u, psi, transport)
        return u, psi

    def seeded_transport(self, seed=1):
        rng = np.random.default_rng(seed)
        t = np.full((self.e_size, self.K), np.nan)
        t[self.e_active] = rng.uniform(-0.1, 0.1, int(self.e_active.sum()))
        return t, oa.DeviceBuffer(self.padded(t))


def test_the_levels_cover_the_launch_rule():
    """what the layer counts of the sweep are there for, from the launch rule restated above"""
    L = {K: gm_launch(K) for K in LEVELS}
    assert [L[K]["Sys"] for K in (1, 2, 3, 5, 15, 16, 17, 64, 85, 86, 128, 129, 255, 256)] == \
        [256, 128, 85, 51, 17, 16, 15, 4, 3, 2, 2, 1, 1, 1]  # every change of the columns per workgroup around a case
    assert all(L[K]["Sys"] == 1 and L[K]["Threads"] > LANES for K in (257, 512, 513, 1024))  # one long column
    assert L[3]["PadLanes"] == 1 and L[17]["PadLanes"] == 1 and L[257]["PadLanes"] == 63 and L[513]["PadLanes"] == 63
    assert all(L[K]["PadLanes"] == 0 for K in (1, 2, 16, 64, 128, 256, 512, 1024))
    assert L[129]["Threads"] == 192 and L[255]["Threads"] == 256 and L[1024]["Threads"] == MAX_ROWS
    # a full column has K - 1 rows: every number of PCR levels from 0 to 10 except 3 and 5 occurs
    assert [pcr_levels(K - 1) for K in LEVELS if K > 1] == [0, 1, 2, 4, 4, 4, 6, 7, 7, 7, 7, 8, 8, 8, 9, 9, 10]
    assert all(L[K]["LdsBytes"] <= LDS_BYTES and L[K]["Threads"] <= MAX_ROWS for K in LEVELS)
    assert COLUMN_LIMIT < 1024  # the largest cases go through the array form


@pytest.mark.parametrize("mesh,K,eos_kind", CASES)
def test_bit_exact_on_nan_seeded_outputs(mesh, K, eos_kind):
    x = Rig(named_mesh(mesh), K, eos_kind)
    if x.column_pass:
        x.update_column()
    x.poison()
    x.compute()
    want_u, want_psi = x.restated()
    got = x.outputs()
    _same(got["BolusVelocity"], x.padded(want_u), "BolusVelocity")
    _same(got["StreamFunction"], x.padded(want_psi), "StreamFunction")
    assert np.isfinite(want_u[x.e_active]).all() and np.isfinite(want_psi[x.e_active]).all() and x.e_active.any()
    assert np.isnan(want_u[~x.e_active]).all()
    # ... and the case is what it is there for
    n = x.e_all
    nlay = x.e_active[:n].sum(axis=1)
    shape = gm_launch(K)
    assert (nlay == 0).any()  # edges next to land (an empty range) are left alone
    assert (nlay == 1).any()  # Lo == Hi: no system, 0 / hE
    assert nlay.max() == K    # a full column: pcr_levels(K - 1) levels
    if K > 2:
        assert np.abs(want_u[x.e_active]).max() > 0.0 and (x.lo_e[:n][nlay > 0] > 0).any()
    if shape["Sys"] > 1 and K > 1:  # columns of different depth share a workgroup
        assert any(len(set(nlay[i: i + shape["Sys"]])) > 1 for i in range(0, n, shape["Sys"]))
    if "coast" in mesh:
        assert len(set(np.bincount(x.coe[:n].ravel())[: x.n_all])) > 2  # valences 5, 6, 7 and coast cells


@pytest.mark.parametrize("mesh,K,eos_kind", [("fib300_coast_ragged", 16, "teos10"), ("hex24x20", 85, "linear"),
                                             ("fib300_coast_ragged", 257, "linear")])
def test_the_compute_forms_and_the_stream_forms_agree(mesh, K, eos_kind):
    x = Rig(named_mesh(mesh), K, eos_kind)
    s = oa.Stream()
    outs = []
    for array_form in (False, True):
        for stream in (None, s):
            if x.column_pass:
                x.update_column(stream=stream)
                if stream is not None:
                    stream.synchronize()
            elif not array_form:
                continue  # beyond the column pass only the array form has fields
            x.poison()
            x.compute(array_form=array_form, stream=stream)
            outs.append(x.outputs())
    assert len(outs) == (4 if x.column_pass else 2)
    for o in outs[1:]:
        for name in o:
            _same(o[name], outs[0][name], name)
    # the array form reads its arguments, not the attached arrays
    sv, svd, zm = x.fields()
    other = (sv * 1.01, svd * 1.01, zm * 1.5)
    x.poison()
    x.gm.compute(x.h, None, *other)
    oa.device_synchronize()
    x.synthetic = other
    want_u, want_psi = x.restated()
    _same(x.outputs()["BolusVelocity"], x.padded(want_u), "BolusVelocity (caller's arrays)")
    _same(x.outputs()["StreamFunction"], x.padded(want_psi), "StreamFunction (caller's arrays)")
    assert not np.array_equal(x.outputs()["BolusVelocity"], outs[0]["BolusVelocity"], equal_nan=True)


@pytest.mark.parametrize("mesh,K", [("fib300_coast_ragged", 17), ("hex24x20", 5), ("hex24x20", 129)])
def test_a_given_transport_takes_the_bolus_velocity(mesh, K):
    x = Rig(named_mesh(mesh), K, "teos10")
    assert x.column_pass
    x.update_column()
    x.poison()
    x.compute()
    base = x.outputs()
    t, buf = x.seeded_transport()
    x.poison()
    x.compute(transport=buf.ptr)
    for name, v in x.outputs().items():
        _same(v, base[name], name)
    want = t.copy()
    want[x.e_active] = (t + base["BolusVelocity"][:, :K])[x.e_active]
    _same(buf.to_host(), x.padded(want), "Transport")  # NaN outside the ranges, in the padding and on the sentinel row
    assert not np.array_equal(want[x.e_active], t[x.e_active])
    got = x.gm.compute(x.h, np.nan_to_num(t))  # the numpy form of the binding
    _same(got[x.e_active], want[x.e_active], "Transport (numpy form)")
    assert np.all(got[~x.e_active] == 0.0)


def test_update_column_leaves_the_fields_of_vertmix_n2():
    """N2_c of the contract, recomputed on the host from the device fields after updateColumn, against
    VertMix::computeBruntVaisalaFreqSq on the same fields"""
    K = 16
    x = Rig(named_mesh("fib300_coast_ragged"), K, "teos10")
    x.update_column()
    sv, svd, zm = x.fields()
    lo_c, hi_c = x.vc.get("MinLayerCell"), x.vc.get("MaxLayerCell")
    host = MR.bvf(sv, svd, zm, lo_c, hi_c, x.n_all, RHO0)
    vm = oa.VertMix(x.mesh, x.vc)
    vm.compute_bvf(x.eos)
    oa.device_synchronize()
    dev = vm.get("BruntVaisalaFreqSq")
    _same(dev, host, "BruntVaisalaFreqSq")
    # ... and the contract's N2_c on the edges is that expression on the edge's two cells
    checked = 0
    for s in GR.edge_systems(x.h, sv, svd, zm, x.coe, x.dc, x.kappa, x.lo_e, x.hi_e, x.e_all, RHO0, SPEED):
        if s["he"].shape[1] < 2:
            continue
        for side, n2 in enumerate(s["n2_cells"]):
            c = x.coe[s["es"], side][:, None]
            _same(n2, dev[c, s["k"][:, 1:]], f"N2 of cell {side}")
            checked += n2.size
    assert checked > 0 and np.abs(dev).max() > 0.0


# ---------------------------------------------------------------------------------------------------------------------
# attached to the split-explicit stepper
# ---------------------------------------------------------------------------------------------------------------------
STEP_K, NSUB, STEP_DT = 5, 3, 20.0


def step_rig(attached):
    """tests.split_explicit_fixtures.StepRig on hex24x20 with an Eos (its own where PressureGrad is attached) and a
    GentMcWilliams on the rig's VertCoord"""
    x = StepRig(K=STEP_K, attached=attached, g=named_mesh("hex24x20"))
    if not attached:
        x.eos = oa.Eos(x.p.mesh, STEP_K, "teos10")
    x.gm = oa.GentMcWilliams(x.p.mesh, x.vc, x.eos)
    return x


def hand_step(x, dt_seconds, nsub, t0=0.0, gm=True, stop_after_5b=False):
    """SplitExplicitStepper::doStep with step 5b through the public calls, on the null stream (after
    tests.split_explicit_fixtures.step_by_hand)"""
    p, bm = x.p, x.bm
    m, K = p.mesh, x.K
    dt = oa.coeff_seconds(1.0, dt_seconds)
    st, tend = p.state, p.tend
    h_cur, u_cur, h_next, u_next = st.device_ptr(0, 0), st.device_ptr(1, 0), st.device_ptr(0, 1), st.device_ptr(1, 1)
    tend.set_time(t0)
    tend.compute_all_tendencies(st, p.aux, p.tracers, 0, 0, 0)                       # 1
    vel_tend = tend.device_ptr(1)[0]
    bm.split_velocity(h_cur, u_cur, with_ssh=True)                                   # 2
    bm.compute_residual_forcing(h_cur, vel_tend)                                     # 3
    bm.subcycle(nsub, dt / nsub)                                                     # 4
    bm.transport_velocity(u_cur, u_next)                                             # 5
    if gm:
        x.gm.update_column(h_cur, p.tracers.device_ptr(0), x.nt)                     # 5b
        x.gm.compute(h_cur, u_next)
    if stop_after_5b:
        oa.device_synchronize()
        return
    tend.compute_thickness_tendencies(st, p.aux, 0, 1)                               # 6
    oa.update_by_tend(h_next, h_cur, tend.device_ptr(0)[0], dt, m.NCellsAll, oa.level_pitch(K))
    tend.compute_tracer_tendencies(st, p.aux, p.tracers, 0, 0, 1)                    # 7
    oa.device_synchronize()
    cur, nxt = p.tracers.copy_to_host(0), p.tracers.copy_to_host(1)
    hc, hn = st.copy_to_host(0)[0], st.copy_to_host(1)[0]
    n = m.NCellsAll
    nxt[:, :n] = (cur[:, :n] * hc[:n] + dt * tend.get(2)[:, :n]) / hn[:n]
    p.tracers.copy_to_device(nxt, 1)
    bm.advance_velocity(u_cur, vel_tend, dt, u_next)                                 # 8
    st.update_time_levels()                                                          # 9
    p.tracers.update_time_levels()
    oa.device_synchronize()


def _stepper(x, switches_on=True, attach=True):
    st = x.stepper("Split-Explicit", STEP_DT, NSUB)
    if not switches_on:
        st.set_fused_transport(False)
        st.set_momentum_rhs(False)
        st.set_folded_updates(False)
    if attach:
        st.attach_gent_mcwilliams(x.gm)
    return st


@pytest.mark.parametrize("switches_on", [True, False], ids=["defaults", "all_off"])
@pytest.mark.parametrize("attached", [True, False], ids=["pgrad_vertadv", "nothing_attached"])
def test_step_equals_its_calls_by_hand(attached, switches_on):
    a, b = step_rig(attached), step_rig(attached)
    st = _stepper(a, switches_on)
    st.do_step(a.p.state)
    oa.device_synchronize()
    before = oa.device_resource_count()
    st.do_step(a.p.state)
    oa.device_synchronize()
    assert oa.device_resource_count() == before  # a step with the closure attached allocates nothing
    for i in range(2):
        hand_step(b, STEP_DT, NSUB, i * STEP_DT)
    for name, got, want, start in zip(("h", "u", "tracers"), a.result(), b.result(), (a.h, a.u, a.tr)):
        assert np.all(np.isfinite(got)), name
        _same(got, want, f"{name}: the stepper against its calls by hand")
        assert not np.array_equal(got, start), name
    for name in ("BolusVelocity", "StreamFunction"):
        _same(a.gm.get(name), b.gm.get(name), name)
    assert np.abs(a.gm.get("BolusVelocity")).max() > 0.0
    # the column fields are those of a Displaced = true pass of the step's inputs
    for name in ("SpecVol", "SpecVolDisplaced"):
        _same(a.eos.get(name), b.eos.get(name), name)
    _same(a.vc.get("ZMid"), b.vc.get("ZMid"), "ZMid")


@pytest.mark.parametrize("attached", [True, False], ids=["pgrad_vertadv", "nothing_attached"])
def test_the_bolus_flow_moves_thickness_and_tracers_and_not_the_velocity(attached):
    """One step with the closure against one without: the velocity is the same bit for bit, the tracers differ, and so
    does the thickness where the layers move freely (nothing attached).  With the VertAdv attached the layers are held to
    the z-star shape: the new thickness is the column's total divergence dealt out by the coordinate's weights, and the
    bolus transport has no column integral (tests/test_gent_mcwilliams.py: it telescopes, to about 2^-53 of max|Psi| per
    layer), so there the thickness must NOT move beyond rounding -- measured: equal in every bit -- and what the bolus
    flow moves is the VertAdv's VerticalTransport.  The bound 1e-9 max h is far above any accumulation of roundings
    (K = 5 layers, 6 edges, a few eps each) and seven orders below the layer-by-layer change without z-star."""
    a, b = step_rig(attached), step_rig(attached)
    _stepper(a).do_step(a.p.state)
    _stepper(b, attach=False).do_step(b.p.state)
    (ha, ua, ta), (hb, ub, tb) = a.result(), b.result()
    _same(ua, ub, "u after the step: no bolus part")
    n = a.p.mesh.NCellsAll
    assert not np.array_equal(ta[:, :n], tb[:, :n])
    dh = np.abs(ha[:n] - hb[:n]).max()
    print(f"attached {attached}: max |h with - h without| = {dh:.3e} m, max |T, S with - without| = "
          f"{np.abs(ta[:, :n] - tb[:, :n]).max():.3e}")
    if attached:
        assert dh <= 1.0e-9 * np.abs(hb[:n]).max()
        wa, wb = a.va.get("VerticalTransport"), b.va.get("VerticalTransport")
        assert not np.array_equal(wa[:n], wb[:n])
    else:
        assert not np.array_equal(ha[:n], hb[:n])
    for name in ("BtrVelocity", "SSH", "BtrFluxMean"):
        _same(a.bm.get(name), b.bm.get(name), name)


@pytest.mark.parametrize("attached", [True, False], ids=["pgrad_vertadv", "nothing_attached"])
def test_the_transporting_velocity_still_carries_the_mean_flux(attached):
    """sum_K hE[K] * u[Next][e][K] just after step 5b against BtrFluxMean[e], the products and the sum taken exactly
    (rationals).  Without the closure the difference is bounded by eps/2 (T ((4 n + 7) U + n |Q|) + |Flux|)
    (tests/test_split_explicit.py: test_transport_velocity_carries_the_mean_flux, with T = BtrThickEdge, Q = Flux / T,
    U = max |u|, n = Hi - Lo + 1); the bolus velocity adds a column sum bounded by 4 n max|Psi| 2^-53
    (tests/test_gent_mcwilliams.py: test_the_column_transport_telescopes_to_zero).  The bound is the sum of the two."""
    x = step_rig(attached)
    hand_step(x, STEP_DT, NSUB, stop_after_5b=True)
    m, K = x.p.mesh, x.K
    ne = m.NEdgesAll
    u_next = x.p.state.copy_to_host(1)[1]
    h = x.p.state.copy_to_host(0)[0]
    coe = m.get_array("CellsOnEdge")
    lo, hi = x.vc.get("MinLayerEdgeBot"), x.vc.get("MaxLayerEdgeTop")
    mask = PR.range_mask(lo, hi, ne, K)
    flux, thick = x.bm.get("BtrFluxMean"), x.bm.get("BtrThickEdge")
    psi = x.gm.get("StreamFunction")
    umax = np.abs(x.u[:ne][mask]).max()
    worst = 0.0
    for e in np.nonzero(mask.any(axis=1))[0]:
        lev = mask[e]
        he = 0.5 * (h[coe[e, 0]][lev] + h[coe[e, 1]][lev])
        total = sum((Fraction(float(a)) * Fraction(float(v)) for a, v in zip(he, u_next[e][lev])), Fraction(0))
        n = int(lev.sum())
        t, fl = thick[e], abs(flux[e])
        bound = EPS / 2 * (t * ((4 * n + 7) * umax + n * abs(flux[e] / t)) + fl) * (1.0 + 1.0e-6) \
            + 4.0 * n * np.abs(psi[e][lev]).max() * (EPS / 2) * (1.0 + 1.0e-6)
        err = abs(float(total - Fraction(float(flux[e]))))
        worst = max(worst, err / bound)
        assert err <= bound, (e, err, bound)
    print(f"worst |sum hE u - BtrFluxMean| / bound = {worst:.3f}")
    assert worst > 0.0 and np.abs(x.gm.get("BolusVelocity")[:ne][mask]).max() > 0.0


def test_detaching_restores_the_unattached_bits():
    a, b = step_rig(True), step_rig(True)
    st = _stepper(a)
    st.attach_gent_mcwilliams(None)
    st.do_step(a.p.state)
    _stepper(b, attach=False).do_step(b.p.state)
    for name, got, want in zip(("h", "u", "tracers"), a.result(), b.result()):
        _same(got, want, name)
    assert np.all(a.gm.get("BolusVelocity") == 0.0)  # never computed


def test_refusals_on_a_device():
    K = 4
    g = planar_hex(6, 4, 30.0e3)
    d = oa.Decomp(oa.GlobalMesh(g), 1, 0, 3)
    m, m2 = oa.HorzMesh(d, K), oa.HorzMesh(d, K)
    vc, eos = oa.VertCoord(m, K, RHO0, "Uniform", decomp=d), oa.Eos(m, K, "linear")
    vc2, eos2 = oa.VertCoord(m2, K, RHO0, "Uniform", decomp=d), oa.Eos(m2, K, "linear")
    for args, msg in (((m, None, eos), "VertCoord is NULL"), ((m, vc, None), "Eos is NULL"),
                      ((m, vc2, eos), "another mesh"), ((m, vc, eos2), "another mesh"),
                      ((m, vc, oa.Eos(m, K + 1, "linear")), "layer counts")):
        with pytest.raises(oa.OmegaAmdError, match=msg):
            oa.GentMcWilliams(*args)
    for kw, msg in ((dict(kappa=-1.0), "GMKappa"), (dict(kappa=np.inf), "GMKappa"), (dict(grav_wave_speed=0.0), "GravWaveSpeed"),
                    (dict(grav_wave_speed=np.nan), "GravWaveSpeed")):
        with pytest.raises(oa.OmegaAmdError, match=msg):
            oa.GentMcWilliams(m, vc, eos, **kw)
    oa.GentMcWilliams(m, vc, eos, kappa=0.0)  # zero is a diffusivity
    big = oa.HorzMesh(d, 1025)
    with pytest.raises(oa.OmegaAmdError, match="1 <= NVertLayers <= 1024"):
        oa.GentMcWilliams(big, oa.VertCoord(big, 1025, RHO0, "Uniform", decomp=d), oa.Eos(big, 1025, "linear"))
    # the attachment
    x = step_rig(True)
    pm = x.p.mesh
    with pytest.raises(oa.OmegaAmdError, match="Split-Explicit"):
        x.stepper("RungeKutta4", STEP_DT).attach_gent_mcwilliams(x.gm)
    st = x.stepper("Split-Explicit", STEP_DT, NSUB)
    with pytest.raises(oa.OmegaAmdError, match="another mesh or layer count"):
        st.attach_gent_mcwilliams(oa.GentMcWilliams(m, vc, eos))
    other_vc = oa.VertCoord(pm, STEP_K, RHO0, "Uniform", decomp=x.p.decomp)
    with pytest.raises(oa.OmegaAmdError, match="different VertCoord or Eos"):
        st.attach_gent_mcwilliams(oa.GentMcWilliams(pm, other_vc, x.eos))
    with pytest.raises(oa.OmegaAmdError, match="different VertCoord or Eos"):
        st.attach_gent_mcwilliams(oa.GentMcWilliams(pm, x.vc, oa.Eos(pm, STEP_K, "teos10")))
    st.attach_gent_mcwilliams(x.gm)
    base = x.result()
    one = oa.Tracers(pm, None, STEP_K, 1, 2)
    tend1 = oa.Tendencies(pm, STEP_K, 1, oa.default_config(SSHTendencyEnable=1))
    aux1 = oa.AuxiliaryState(pm, None, STEP_K, 1)
    st1 = oa.TimeStepper("Split-Explicit", STEP_DT, tend1, aux1, pm, None, one)
    with pytest.raises(oa.OmegaAmdError, match="tracers"):
        st1.attach_gent_mcwilliams(x.gm)
    for got, want in zip(x.result(), base):
        _same(got, want, "a refused attachment leaves the state alone")
