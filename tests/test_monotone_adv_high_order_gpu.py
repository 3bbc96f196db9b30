"""The high-order horizontal flux of MonotoneAdv on the GPU (MonotoneAdv::setHorzOrder; omega_amd/csrc/MonotoneAdv.h,
kernels/MonotoneAdvKernels.hip: MonoHessBody and the High = true forms of the two bodies).

The yardstick of the call is the restatement (tests/monotone_adv_reference.py) on the tables read back from the
object, compared as tests/test_monotone_adv_gpu.py compares the centred form: Hess, ScaleIn, ScaleOut and the tendency
are seeded with NaN and read back raw; every entry must hold the restatement's bits or its seed."""
import numpy as np
import pytest

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests import monotone_adv_reference as MR
from tests.monotone_adv_fixtures import ORDERS, RANDOM, Ho3Rig, HoRig, Inputs, MonoRig
from tests.monotone_adv_reference import MonoMesh
from tests.rank_rig import raw
from tests.split_explicit_fixtures import StepRig
from tests.test_monotone_adv_3d_gpu import Dev3
from tests.test_monotone_adv_3d_gpu import LEVELS as LEVELS_3D
from tests.test_monotone_adv_gpu import LEVELS, NO_ADV, Dev, assert_bits, mono_step_by_hand
from tests.test_monotone_adv_high_order import growth, margin_value

pytestmark = pytest.mark.gpu

MAXT = 7
TABLES = ("FitCell", "HessWeight", "EdgeDirOwn", "EdgeDirAcross")
NAMES = ("Tend", "ScaleIn", "ScaleOut", "Hess")


@pytest.fixture(scope="module", autouse=True)
def _device():
    oa.device_init(0)


class _Ho:
    """mixin of Dev / Dev3: the object at (order, coef), the restatement on the tables read back from it"""

    def setup_ho(self, order, coef):
        R = self.R
        self.mono.set_horz_order(order, coef, **MR.geometry(R.g))
        tabs = {n: self.mono.get(n) for n in TABLES}
        host = oa.monotone_adv_high_order_tables(R.mesh, order, coef, **MR.geometry(R.g))
        for n in TABLES:  # what was uploaded is what the host builder gives
            assert_bits(tabs[n], host[n], n)
        R.H = MR.HoTables(R.M, tabs, 0.0 if order == 4 else coef)
        self.hshape = (self.maxt, 3, R.nc_size, self.pitch)
        return self

    def seed(self, nt):
        t, s = super().seed(nt)
        self.hseed = np.full(self.hshape, np.nan)
        oa.copy_to_device(self.mono.device_ptr("Hess"), self.hseed)
        return t, s

    def read(self):
        return super().read() + (raw(self.mono.device_ptr("Hess"), self.hshape),)

    def reference(self):
        if not hasattr(self, "_ref_ho"):
            self._ref_ho = self.R.reference_ho(self.I, self.I.tracers.shape[0], self.tend0)
        return self._ref_ho

    def check(self, nt, stream=None):
        R, K = self.R, self.K
        t_seed, s_seed = self.seed(nt)
        self.run(nt, stream)
        if stream is not None:
            stream.synchronize()
        got = self.read()
        for g, want, seed, name in zip(got, self.reference(), (t_seed, s_seed, s_seed, self.hseed), NAMES):
            expect = seed.copy()
            expect[:nt, ..., : R.nc, :K] = want[:nt, ..., : R.nc, :]
            assert np.isfinite(want[:nt, ..., : R.nc, :]).all(), name
            assert_bits(g, expect, f"{name} (NT = {nt})")
        for n, a in self.host.items():  # the inputs are what was uploaded
            assert_bits(self.buf[n].to_host(), a, n)
        return got


class DevHo(_Ho, Dev):
    pass


class DevHo3(_Ho, Dev3):
    def check(self, nt, stream=None):
        got = super().check(nt, stream)
        assert_bits(raw(self.va.device_ptr("VerticalTransport"), self.wt.shape), self.wt, "VerticalTransport")
        return got


_CASES = {}


def case(name, K, upwind, order, coef, vert=False):
    key = (name, K, upwind, order, coef, vert)
    if key not in _CASES:
        R = (Ho3Rig if vert else HoRig)(name, K, device=True)
        I = R.inputs(seed=3 + K, upwind=upwind, ntracers=MAXT, check=False)
        _CASES[key] = (DevHo3 if vert else DevHo)(R, I, MAXT).setup_ho(order, coef)
    return _CASES[key]


@pytest.mark.parametrize("upwind", (False, True), ids=("centre", "upwind"))
@pytest.mark.parametrize("order,coef", ORDERS)
@pytest.mark.parametrize("nt", (1, 2, 3, 4, MAXT))
@pytest.mark.parametrize("K", LEVELS)
@pytest.mark.parametrize("name", ("hex24x20", "fib700_coast_ragged"))
def test_bit_exact_on_nan_seeded_arrays(name, K, nt, order, coef, upwind):
    D = case(name, K, upwind, order, coef)
    _, si, so, hs = D.check(nt)
    if nt == MAXT:  # the comparison is about a correction and a limiter at work
        r = si[RANDOM, : D.R.nc, :K]
        assert (r < 1.0).any() and (r == 1.0).any() and (so[RANDOM, : D.R.nc, :K] < 1.0).any()
        assert hs[RANDOM, :, : D.R.nc, :K].any()
        if name != "hex24x20":  # cells that are not fit cells hold 0.0
            assert not hs[:nt, :, : D.R.nc, :K][:, :, ~D.R.H.fit[: D.R.nc]].any()


@pytest.mark.parametrize("order,coef", ORDERS)
@pytest.mark.parametrize("nt", (1, 2, 3, 4, MAXT))
@pytest.mark.parametrize("K", LEVELS_3D)
@pytest.mark.parametrize("name", ("hex24x20", "fib700_coast_ragged"))
def test_the_3d_form_is_bit_exact(name, K, nt, order, coef):
    """Vert = true, High = true: the 3-D restatement fed the high-order FHigh, on the fixtures of
    tests/monotone_adv_fixtures.py"""
    case(name, K, False, order, coef, vert=True).check(nt)


def test_order_2_is_unchanged():
    """set_horz_order(2), and 4 and back to 2: the bits of the centred form (Dev.check compares them with the restatement
    of tests/monotone_adv_reference.py, which an object never configured reproduces) in two launches"""
    R = MonoRig("fib700_coast_ragged", 16, device=True)
    I = R.inputs(seed=19, ntracers=4)
    D, plain = Dev(R, I, 4), Dev(R, I, 4)
    never = plain.check(4)

    def two_launches_and_the_same_bits(what):
        before = D.mono.launch_count()
        got = D.check(4)
        assert D.mono.launch_count() == before + 2, what
        for a, b, n in zip(got, never, NAMES):
            assert_bits(a, b, f"{n}: {what}")

    two_launches_and_the_same_bits("never configured")
    D.mono.set_horz_order(2)
    two_launches_and_the_same_bits("order 2")
    D.mono.set_horz_order(4, **MR.geometry(R.g))
    before = D.mono.launch_count()
    D.seed(4)
    D.run(4)
    high = D.read()
    assert D.mono.launch_count() == before + 3
    assert not np.array_equal(high[0][:4, : R.nc, : R.K], never[0][:4, : R.nc, : R.K])
    D.mono.set_horz_order(2)
    two_launches_and_the_same_bits("order 4 and back to 2")
    D.mono.set_horz_order(3, 0.25, **MR.geometry(R.g))  # Hess and the tables are reused
    D.mono.set_horz_order(2, float("nan"))  # (the coefficient is looked at at order 3 only)
    two_launches_and_the_same_bits("order 3 and back to 2")


def test_calls_create_no_device_resource():
    D = case("hex24x20", 16, False, 4, 0.25)
    D.run(2)
    oa.device_synchronize()
    before = oa.device_resource_count()
    for nt in (1, 2, 5, MAXT):
        D.run(nt)
    D.mono.set_horz_order(2)
    D.run(2)
    D.mono.set_horz_order(4, **MR.geometry(D.R.g))  # the second time: nothing new
    D.run(2)
    oa.device_synchronize()
    assert oa.device_resource_count() == before


def test_launch_shape_with_a_tail_split():
    """hex130x130, K = 32, NT = 2: the last tiles are tail-split, one level chunk per workgroup (derived in
    tests/test_transport_gpu.py)"""
    R = HoRig("hex130x130", 32, device=True)
    DevHo(R, R.inputs(seed=2, ntracers=2, check=False), max_tracers=2).setup_ho(4, 0.25).check(2)


def test_stream_forms_agree():
    D = case("hex24x20", 16, False, 3, 0.25)
    a = D.check(3)
    b = D.check(3, stream=oa.Stream())
    for x, y in zip(a, b):
        assert_bits(x, y, "null stream / stream")


def test_two_part_decomposition_matches_on_owned_cells():
    """halo width 3: Hess of a cell needs its neighbours, the scale factors Hess of the cells across, the fluxes the
    scale factors of the cells across"""
    K, nt, order, coef = 4, 3, 4, 0.25
    R1 = HoRig("hex24x20", K, device=True)
    I1 = R1.inputs(seed=8, ntracers=nt)
    D1 = DevHo(R1, I1, nt).setup_ho(order, coef)
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
    result = []
    for w in range(4):
        a = np.moveaxis(one[w][:nt, ..., : R1.nc, :K], -2, 0)  # cells first
        r = np.zeros((ncg,) + a.shape[1:])
        r[cid1] = a
        result.append(r)
    for rank in range(2):
        R = HoRig("hex24x20", K, nparts=2, rank=rank, device=True, halo=3)
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
        D = DevHo(R, I, nt).setup_ho(order, coef)
        D.tend0[:] = 0.0
        got = D.check(nt)  # every local cell against the local restatement ...
        for w, name in enumerate(NAMES):  # ... and the owned ones against the one-part run
            a = np.moveaxis(got[w][:nt, ..., :own, :K], -2, 0)
            assert_bits(a, result[w][cid[:own]], f"{name} on the owned cells of part {rank}")


def step_geometry():
    return MR.geometry(planar_hex(8, 8, 30.0e3))  # StepRig's mesh


def test_attached_step_at_order_4_equals_the_calls_by_hand():
    dt, nsub = 20.0, 7
    a, b = StepRig(K=4, attached=False, config=NO_ADV), StepRig(K=4, attached=False, config=NO_ADV)
    ma, mb = oa.MonotoneAdv(a.p.mesh, a.K, a.nt), oa.MonotoneAdv(b.p.mesh, b.K, b.nt)
    for m in (ma, mb):
        m.set_horz_order(4, **step_geometry())
        assert m.get("FitCell")[: a.p.mesh.NCellsAll].all()
    st = a.stepper("Split-Explicit", dt, nsub)
    st.attach_monotone_adv(ma)
    st.do_step(a.p.state)
    mono_step_by_hand(b, mb, dt, nsub, True)
    got, want = a.result(), b.result()
    for name, g, w, start in zip(("h", "u", "tracers"), got, want, (a.h, a.u, a.tr)):
        assert np.isfinite(g).all() and not np.array_equal(g, start), name
        assert_bits(g, w, name)
    for name in ("ScaleIn", "ScaleOut", "Hess"):
        assert_bits(ma.get(name), mb.get(name), name)
    assert ma.get("Hess").any() and ma.launch_count() == 3
    before = oa.device_resource_count()  # a step creates no device resource
    for _ in range(2):
        st.do_step(a.p.state)
    oa.device_synchronize()
    assert oa.device_resource_count() == before and ma.launch_count() == 9
    # and the correction was what moved the tracers: the attached step at order 2 differs
    c = StepRig(K=4, attached=False, config=NO_ADV)
    sc = c.stepper("Split-Explicit", dt, nsub)
    sc.attach_monotone_adv(oa.MonotoneAdv(c.p.mesh, c.K, c.nt))
    sc.do_step(c.p.state)
    assert not np.array_equal(c.result()[2], want[2])


def test_eight_steps_keep_a_step_tracer_in_its_range():
    """the run of tests/test_monotone_adv_gpu.py (Dt = 600 s, 30 km hexagons, Courant number far below 0.5, measured) at
    order 4: the 0/1 step stays in [0, 1] to the margin of tests/test_monotone_adv_high_order.py, once per step"""
    dt, nsub, steps = 600.0, 30, 8
    off = dict(TracerDiffTendencyEnable=0, TracerHyperDiffTendencyEnable=0, TracerHorzAdvTendencyEnable=0)
    x = StepRig(K=4, attached=False, config=off)
    m = x.p.mesh
    xc = m.get_array("XCell")[: m.NCellsAll]
    x.tr[0, : m.NCellsAll] = (xc > np.median(xc)).astype(float)[:, None]
    x.load()
    st = x.stepper("Split-Explicit", dt, nsub)
    mono = oa.MonotoneAdv(m, x.K, x.nt)
    mono.set_horz_order(4, **step_geometry())
    st.attach_monotone_adv(mono)
    h_min, u_max = x.h[: m.NCellsAll].min(), 0.0
    for _ in range(steps):
        st.do_step(x.p.state)
        h, u, _ = x.result()
        h_min, u_max = min(h_min, h[: m.NCellsAll].min()), max(u_max, np.abs(u[: m.NEdgesAll]).max())
    h, u, tr = x.result()
    area, dv = m.get_array("AreaCell")[: m.NCellsAll], m.get_array("DvEdge")[: m.NEdgesAll]
    courant = dt * u_max * 3.0 * dv.max() / area.min()
    print("Courant estimate", courant, "min h", h_min)
    assert np.isfinite(tr).all() and h_min > 0.0 and courant < 0.5 and mono.launch_count() == 3 * steps
    H = MR.HoTables(MonoMesh.of(m), {n: mono.get(n) for n in TABLES}, 0.0)
    n = m.get_array("EdgesOnCell").shape[1]
    for L in range(2):
        lo, hi = x.tr[L, : m.NCellsAll].min(), x.tr[L, : m.NCellsAll].max()
        mg = steps * margin_value(n, h.max(), max(abs(lo), abs(hi)), h_min, growth(H))
        over = max(tr[L, : m.NCellsAll].max() - hi, lo - tr[L, : m.NCellsAll].min())
        print("tracer", L, "outside its initial range by", over, "margin", mg)
        assert over <= mg


def test_refusals():
    R = MonoRig("hex24x20", 2, device=True)
    E = oa.OmegaAmdError
    mono = oa.MonotoneAdv(R.mesh, 2, 1)
    for name in ("Hess",) + TABLES:  # they exist after set_horz_order(3 or 4) only
        with pytest.raises(E, match="after setHorzOrder"):
            mono.get(name)
    for order in (1, 5, 0, -4):
        with pytest.raises(E, match="is not 2, 3 or 4"):
            mono.set_horz_order(order)
    for coef in (0.0, -0.25, 1.5, float("nan")):
        with pytest.raises(E, match=r"outside \(0, 1\]"):
            mono.set_horz_order(3, coef)
    for bad in (-1.0, float("inf"), float("nan")):
        for kw in ("sphere_radius", "x_period", "y_period"):
            with pytest.raises(E, match="negative or not finite"):
                mono.set_horz_order(4, **{kw: bad})
            with pytest.raises(E, match="negative or not finite"):
                mono.set_horz_order(2, **{kw: bad})
    with pytest.raises(E, match="after setHorzOrder"):  # a refused call configured nothing
        mono.get("Hess")
    assert mono.launch_count() == 0
    mono.set_horz_order(3, 1.0, **MR.geometry(R.g))
    assert mono.get("Hess").shape == (1, 3, R.nc_size, 2) and mono.get("FitCell")[: R.nc].all()
