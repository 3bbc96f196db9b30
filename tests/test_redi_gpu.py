"""Redi on the GPU: each of the three launches equals the NumPy restatement of the contract (tests/redi_reference.py) bit
for bit on NaN-seeded outputs -- entries outside the ranges, the sentinel row and the row padding are NaN and must stay
so -- at every layer count at which a launch changes shape; the attached, array and stream forms agree and the array
form reads its arguments; NaN outside the cells' layer ranges never reaches an output; a given VertDiff takes VertDiff +
VertDiffusivity, Tend is accumulated, tracer planes beyond NTracers are left alone; attached to the split-explicit
stepper a step equals the public calls made by hand, moves the tracers only, allocates nothing, and detaching restores
the unattached bits; the refusals that need a device."""
import numpy as np
import pytest

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests import redi_reference as RR
from tests.column_reference import RHO0
from tests.meshes import named_mesh
from tests.rank_rig import RankRig, raw
from tests.split_explicit_fixtures import StepRig
from tests.test_gent_mcwilliams_gpu import LEVELS as SLOPE_LEVELS
from tests.vert_fixtures import (FUSED, STAGE_SPEC_VOL_DISP, column_limit, level_pitch, mix_inputs, same as _same,
                                 systems_launch)

pytestmark = pytest.mark.gpu

NT, MAX_TRACERS = 2, 3
KAPPA = 450.0
MESHES = ("hex24x20", "fib300_coast_ragged")
CELL_LEVELS = (1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 32, 33, 64, 65, 128, 129, 257)
LEVELS = tuple(sorted(set(SLOPE_LEVELS) | set(CELL_LEVELS)))
CASES = [(m, K, e) for m in MESHES for K in LEVELS for e in ("teos10", "linear")]
COLUMN_LIMIT = column_limit(FUSED | STAGE_SPEC_VOL_DISP)  # the column pass with the displaced volume
LDS_BYTES, MAX_ROWS, LANES, SLOPE_LDS_ARRAYS = 65536, 1024, 256, 6
TILE_CELLS, MAX_LANES_K = 32, 16


def slope_launch(K):
    """launchRediSlope (kernels/RediKernels.hip), restated: the bolus-velocity launch's shape with six LDS doubles per
    occupied lane"""
    sys, rows, threads = systems_launch(K)
    return dict(Sys=sys, Rows=rows, Threads=threads, PadLanes=threads - rows, LdsBytes=SLOPE_LDS_ARRAYS * rows * 8)


def cell_launch(K, max_edges=8):
    """rediCellShape (kernels/RediKernels.hip), restated: the lanes along a cell's levels (the power of two that holds
    min(K, 16)), the cells of a workgroup (32 at most, 256 lanes at most), its lanes, the strides of 16 levels a lane
    walks, and the dynamic LDS of the staged connectivity (per cell and slot five doubles and five ints, per cell one
    double and two ints)"""
    lanes = 1
    while lanes < K and lanes < MAX_LANES_K:
        lanes *= 2
    tile = min(256 // lanes, TILE_CELLS)
    return dict(LanesK=lanes, Tile=tile, Threads=tile * lanes, Strides=-(-K // lanes),
                LdsBytes=(5 * tile * max_edges + tile) * 8 + (5 * tile * max_edges + 2 * tile) * 4)


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
    """One rank's VertCoord, Eos and Redi on global inputs (tests.vert_fixtures.mix_inputs: layer ranges with land,
    KMin > 0, single layers) in local order, a per-edge Kappa with zeros in it, and the column fields: from update_column
    up to the column pass's limit, synthetic beyond it (handed to the array forms).  SlopeMax is the median magnitude of
    the unclipped slopes of the case (from the restatement), so that clipped and unclipped slopes both occur."""

    def __init__(self, g, K, eos_kind, seed=7, full=False, synthetic=False):
        super().__init__(g, K)
        self.P = level_pitch(K)
        m = self.mesh
        G = mix_inputs(g, K, seed, full, MAX_TRACERS)
        rng = self.rng = np.random.default_rng(seed + 100)
        n = int(g["nCells"])
        self.h, self.tr = self.cells(G["h"]), self.cells(G["tr"])
        self.layers(G["min_level"], G["max_level"])
        self.vc.set("BottomDepth", self.cells(rng.uniform(100.0, 6000.0, n)))
        self.eos = oa.Eos(m, K, eos_kind)
        self.forcing = (("SurfacePressure", rng.uniform(0.9e5, 1.1e5, n)), ("TidalPotential", rng.uniform(-1.0, 1.0, n)),
                        ("SelfAttractionLoading", rng.uniform(-0.1, 0.1, n)))
        self.kappa = rng.uniform(100.0, 900.0, self.e_size)
        self.kappa[::7] = 0.0
        self.t = RR.tables(m)
        self.coe, self.dc = self.t["CellsOnEdge"], self.t["DcEdge"]
        self.column_pass = K <= COLUMN_LIMIT and not synthetic
        self.synthetic = None if self.column_pass else synthetic_fields(rng, self.h)
        first = self.make()
        assert np.all(first.get("Kappa") == KAPPA)  # RediKappa at construction
        for name, _ in self.forcing:
            assert np.all(first.get(name) == 0.0)  # zero at construction
        assert np.all(raw(first.device_ptr("SlopeInterface"), (self.e_size, self.P)) == 0.0)
        assert np.all(raw(first.device_ptr("VertDiffusivity"), (self.n_size, self.P)) == 0.0)
        self.redi = self.setup(first)
        if self.column_pass:
            self.update_column()
        free = RR.slope(self.h, *self.fields(), self.coe, self.dc, self.lo_e, self.hi_e, self.e_all, RHO0,
                        np.full((self.e_size, K), np.nan), slope_max=1.0e300)
        inner = np.abs(free[np.isfinite(free) & (free != 0.0)])
        self.slope_max = float(np.median(inner)) if inner.size else RR.SLOPE_MAX
        self.redi = self.setup(self.make(slope_max=self.slope_max))

    def make(self, **kw):
        return oa.Redi(self.mesh, self.vc, self.eos, MAX_TRACERS, kappa=KAPPA, **kw)

    def setup(self, r):
        for name, v in self.forcing:
            r.set(name, self.cells(v))
        r.set("Kappa", self.kappa)
        return r

    def poison(self, slope=True):
        """both outputs (slope False: VertDiffusivity alone) NaN everywhere, padding and sentinel row included"""
        if slope:
            oa.copy_to_device(self.redi.device_ptr("SlopeInterface"), np.full((self.e_size, self.P), np.nan))
        oa.copy_to_device(self.redi.device_ptr("VertDiffusivity"), np.full((self.n_size, self.P), np.nan))

    def update_column(self, stream=None):
        for name in ("SpecVol", "SpecVolDisplaced"):
            self.eos.set(name, np.full((self.n_size, self.K), np.nan))
        self.vc.set("ZMid", np.full((self.n_size, self.K), np.nan))
        self.redi.update_column(self.h, self.tr[:NT], NT, stream=stream)
        oa.device_synchronize()

    def fields(self):
        if self.synthetic is not None:
            return self.synthetic
        return self.eos.get("SpecVol"), self.eos.get("SpecVolDisplaced"), self.vc.get("ZMid")

    def sync(self, stream=None):
        if stream is not None:
            stream.synchronize()
        oa.device_synchronize()

    def compute_slope(self, array_form=None, stream=None):
        """the attached form where the column pass ran, else the array form on the synthetic fields"""
        array_form = self.synthetic is not None if array_form is None else array_form
        extra = dict(zip(("spec_vol", "spec_vol_displaced", "z_mid"), self.fields())) if array_form else {}
        self.redi.compute_slope(self.h, stream=stream, **extra)
        self.sync(stream)

    def slope(self):
        return raw(self.redi.device_ptr("SlopeInterface"), (self.e_size, self.P))

    def vert_diffusivity(self):
        return raw(self.redi.device_ptr("VertDiffusivity"), (self.n_size, self.P))

    def restated_slope(self):
        s = np.full((self.e_size, self.K), np.nan)
        return RR.slope(self.h, *self.fields(), self.coe, self.dc, self.lo_e, self.hi_e, self.e_all, RHO0, s,
                        slope_max=self.slope_max)

    def seeded_tend(self, nt, seed=1):
        """a tendency to accumulate onto: random inside the cells' ranges, NaN elsewhere; (host, device buffer)"""
        rng = np.random.default_rng(seed)
        t = np.full((nt, self.n_size, self.K), np.nan)
        t[:, self.active] = rng.uniform(-1.0e-6, 1.0e-6, (nt, int(self.active.sum())))
        return t, oa.DeviceBuffer(self.padded(t))

    def add_tracer_tend(self, buf, nt=NT, tracers=None, h=None, array_form=None, stream=None):
        array_form = self.synthetic is not None if array_form is None else array_form
        tracers = self.tr if tracers is None else tracers
        self.redi.add_tracer_tend(buf.ptr, self.h if h is None else h, tracers[:nt], nt,
                                  z_mid=self.fields()[2] if array_form else None, stream=stream)
        self.sync(stream)

    def restated_tend(self, tend, slope, nt=NT, tracers=None, h=None, zmid=None):
        tracers = self.tr if tracers is None else tracers
        return RR.add_tracer_tend(tend, self.h if h is None else h, tracers, nt, self.fields()[2] if zmid is None else zmid,
                                  slope, self.kappa, self.t, self.lo, self.hi, self.lo_e, self.hi_e)

    def restated_vert_diffusivity(self, slope, vert_diff=None):
        out = np.full((self.n_size, self.K), np.nan)
        return RR.vert_diffusivity(out, vert_diff, slope, self.kappa, self.t, self.lo, self.hi, self.lo_e, self.hi_e)


def test_the_levels_cover_the_launch_rules():
    """what the layer counts of the sweep are there for, from the launch rules restated above"""
    L = {K: slope_launch(K) for K in LEVELS}
    assert [L[K]["Sys"] for K in (1, 2, 3, 5, 15, 16, 17, 64, 85, 86, 128, 129, 255, 256)] == \
        [256, 128, 85, 51, 17, 16, 15, 4, 3, 2, 2, 1, 1, 1]  # every change of the columns per workgroup around a case
    assert all(L[K]["Sys"] == 1 and L[K]["Threads"] > LANES for K in (257, 512, 513, 1024))  # one long column
    assert L[3]["PadLanes"] == 1 and L[17]["PadLanes"] == 1 and L[257]["PadLanes"] == 63 and L[513]["PadLanes"] == 63
    assert all(L[K]["LdsBytes"] <= LDS_BYTES and L[K]["Threads"] <= MAX_ROWS for K in LEVELS)
    assert set(SLOPE_LEVELS) <= set(LEVELS) and COLUMN_LIMIT < 1024  # the largest cases go through the array form
    # the cell launches: every number of lanes along the levels, on both sides of each change ...
    Cl = {K: cell_launch(K) for K in LEVELS}
    assert [Cl[K]["LanesK"] for K in (1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 64)] == [1, 2, 4, 4, 8, 8, 16, 16, 16, 16, 16]
    assert {Cl[K]["LanesK"] for K in LEVELS} == {1, 2, 4, 8, 16}
    # ... the tile of 32 cells until the lanes fill the workgroup, then 256 lanes and 16 cells ...
    assert [Cl[K]["Tile"] for K in (1, 2, 4, 8, 9, 16, 17, 257)] == [32, 32, 32, 32, 16, 16, 16, 16]
    assert all(Cl[K]["Threads"] == (256 if K > 4 else 32 * Cl[K]["LanesK"]) for K in LEVELS)
    # ... and one, two, three and more strides of 16 levels per lane, with a last stride that is full (16, 32, 64, 128),
    # one level (17, 33, 65, 129, 257) or ragged (85, 86, 255)
    assert [Cl[K]["Strides"] for K in (15, 16, 17, 32, 33, 64, 65, 128, 129, 257, 1024)] == \
        [1, 1, 2, 2, 3, 4, 5, 8, 9, 17, 64]
    assert all(Cl[K]["LdsBytes"] <= LDS_BYTES for K in LEVELS)
    assert set(CELL_LEVELS) >= {1, 2, 3, 15, 16, 17, 64, 65, 129, 257}


@pytest.mark.parametrize("mesh,K,eos_kind", CASES)
def test_bit_exact_on_nan_seeded_outputs(mesh, K, eos_kind):
    x = Rig(named_mesh(mesh), K, eos_kind)
    x.poison()
    before = x.redi.launch_count()
    x.compute_slope()
    want_s = x.restated_slope()
    got_s = x.slope()
    _same(got_s, x.padded(want_s), "SlopeInterface")
    assert np.isfinite(want_s[x.e_active]).all() and x.e_active.any() and np.isnan(want_s[~x.e_active]).all()
    # the tendency, accumulated onto a seeded one
    t0, buf = x.seeded_tend(NT)
    x.add_tracer_tend(buf)
    want_t = x.restated_tend(t0.copy(), want_s)
    _same(buf.to_host(), x.padded(want_t), "TracerTend")
    assert np.isfinite(want_t[:, x.active]).all() and np.isnan(want_t[:, ~x.active]).all()
    # the diffusivity
    x.redi.compute_vert_diffusivity()
    oa.device_synchronize()
    want_d, _ = x.restated_vert_diffusivity(want_s)
    _same(x.vert_diffusivity(), x.padded(want_d), "VertDiffusivity")
    assert x.redi.launch_count() == before + 3  # one launch each
    # ... and the case is what it is there for
    n = x.e_all
    nlay = x.e_active[:n].sum(axis=1)
    assert (nlay == 0).any()  # edges next to land (an empty range) are left alone
    assert (nlay == 1).any()  # Lo == Hi: one zero, no flux through either interface
    assert nlay.max() == K    # a full column
    assert (x.kappa[:n][nlay > 0] == 0.0).any()  # a Kappa of 0
    if K > 2:
        inner = want_s[x.e_active]
        assert (np.abs(inner) == x.slope_max).any() and ((np.abs(inner) < x.slope_max) & (inner != 0.0)).any()
        assert (x.lo_e[:n][nlay > 0] > 0).any()
        assert not np.array_equal(want_t[:, x.active], t0[:, x.active])
        assert np.nanmax(want_d) > 0.0 and np.nanmin(want_d) >= 0.0
    if "coast" in mesh:
        assert len(set(np.bincount(x.coe[:n].ravel())[: x.n_all])) > 2  # valences 5, 6, 7 and coast cells


@pytest.mark.parametrize("mesh,K,eos_kind", [("fib300_coast_ragged", 16, "teos10"), ("hex24x20", 85, "linear"),
                                             ("fib300_coast_ragged", 257, "linear")])
def test_the_forms_agree_and_the_array_form_reads_its_arguments(mesh, K, eos_kind):
    x = Rig(named_mesh(mesh), K, eos_kind)
    s = oa.Stream()
    outs = []
    for array_form in (False, True):
        for stream in (None, s):
            if x.column_pass:
                x.update_column(stream=stream)
                x.sync(stream)
            elif not array_form:
                continue  # beyond the column pass only the array forms have fields
            x.poison()
            x.compute_slope(array_form=array_form, stream=stream)
            t0, buf = x.seeded_tend(NT)
            x.add_tracer_tend(buf, array_form=array_form, stream=stream)
            x.redi.compute_vert_diffusivity(stream=stream)
            x.sync(stream)
            outs.append(dict(SlopeInterface=x.slope(), TracerTend=buf.to_host(), VertDiffusivity=x.vert_diffusivity()))
    assert len(outs) == (4 if x.column_pass else 2)
    for o in outs[1:]:
        for name in o:
            _same(o[name], outs[0][name], name)
    # the array forms read their arguments, not the attached arrays
    sv, svd, zm = x.fields()
    other = (sv * 1.01, svd * 1.01, zm * 1.5)
    x.poison()
    x.redi.compute_slope(x.h, *other)
    oa.device_synchronize()
    x.synthetic = other
    want_s = x.restated_slope()
    _same(x.slope(), x.padded(want_s), "SlopeInterface (caller's arrays)")
    assert not np.array_equal(x.slope(), outs[0]["SlopeInterface"], equal_nan=True)
    t0, buf = x.seeded_tend(NT)
    x.add_tracer_tend(buf, array_form=True)
    _same(buf.to_host(), x.padded(x.restated_tend(t0.copy(), want_s)), "TracerTend (caller's ZMid)")
    t1, buf1 = x.seeded_tend(NT)
    x.redi.add_tracer_tend(buf1.ptr, x.h, x.tr[:NT], NT, z_mid=zm)
    oa.device_synchronize()
    assert not np.array_equal(buf1.to_host(), buf.to_host(), equal_nan=True)


@pytest.mark.parametrize("mesh,K", [("fib300_coast_ragged", 17), ("hex24x20", 5), ("hex24x20", 65)])
def test_nan_outside_the_layer_ranges_never_reaches_an_output(mesh, K):
    """tracers, h and ZMid (and the two volumes) NaN outside every cell's layer range, through the array forms"""
    x = Rig(named_mesh(mesh), K, "linear", synthetic=True)
    sv, svd, zm = (x.seeded(a) for a in x.synthetic)
    x.synthetic = (sv, svd, zm)
    h, tr = x.seeded(x.h), x.seeded(x.tr)
    assert np.isnan(h[~x.active]).all() and np.isnan(tr[:, ~x.active]).all() and np.isnan(zm[~x.active]).all()
    x.poison()
    x.redi.compute_slope(h, sv, svd, zm)
    oa.device_synchronize()
    x.h = h
    want_s = x.restated_slope()
    _same(x.slope(), x.padded(want_s), "SlopeInterface")
    assert np.isfinite(want_s[x.e_active]).all()
    t0, buf = x.seeded_tend(NT)
    x.add_tracer_tend(buf, tracers=tr, h=h, array_form=True)
    want_t = x.restated_tend(t0.copy(), want_s, tracers=tr, h=h)
    got = buf.to_host()
    _same(got, x.padded(want_t), "TracerTend")
    assert np.isfinite(got[:, :, :K][:, x.active]).all() and not np.array_equal(want_t[:, x.active], t0[:, x.active])
    x.redi.compute_vert_diffusivity()
    oa.device_synchronize()
    _, faces = RR.cell_mask(x.lo, x.hi, x.n_all, K)
    assert np.isfinite(x.vert_diffusivity()[: x.n_all, :K][faces]).all()


@pytest.mark.parametrize("mesh,K", [("fib300_coast_ragged", 17), ("hex24x20", 5), ("hex24x20", 129)])
def test_a_given_vert_diff_takes_the_diffusivity(mesh, K):
    x = Rig(named_mesh(mesh), K, "teos10")
    x.compute_slope()
    want_s = x.restated_slope()
    x.redi.compute_vert_diffusivity()
    oa.device_synchronize()
    base = x.vert_diffusivity()
    rng = np.random.default_rng(1)
    _, faces = RR.cell_mask(x.lo, x.hi, x.n_all, K)
    v = np.full((x.n_size, K), np.nan)
    v[: x.n_all][faces] = rng.uniform(1.0e-5, 1.0e-2, int(faces.sum()))
    buf = oa.DeviceBuffer(x.padded(v))
    x.poison(slope=False)
    x.redi.compute_vert_diffusivity(buf.ptr)
    oa.device_synchronize()
    _same(x.vert_diffusivity()[: x.n_all, :K][faces], base[: x.n_all, :K][faces], "VertDiffusivity")
    want_d, want_v = x.restated_vert_diffusivity(want_s, v.copy())
    _same(x.vert_diffusivity(), x.padded(want_d), "VertDiffusivity (NaN-seeded)")
    _same(buf.to_host(), x.padded(want_v), "VertDiff")  # NaN outside the interfaces, in the padding, on the sentinel row
    assert np.array_equal(want_v[: x.n_all][faces], (v[: x.n_all] + want_d[: x.n_all])[faces])
    assert not np.array_equal(want_v[: x.n_all][faces], v[: x.n_all][faces])
    got = x.redi.compute_vert_diffusivity(np.nan_to_num(v))  # the numpy form of the binding
    _same(got[: x.n_all][faces], want_v[: x.n_all][faces], "VertDiff (numpy form)")


@pytest.mark.parametrize("mesh,K", [("fib300_coast_ragged", 16), ("hex24x20", 3)])
def test_the_tendency_is_accumulated_and_other_planes_are_left_alone(mesh, K):
    x = Rig(named_mesh(mesh), K, "teos10")
    x.compute_slope()
    want_s = x.restated_slope()
    zero = np.zeros((MAX_TRACERS, x.n_size, K))
    alone = x.restated_tend(zero.copy(), want_s, nt=MAX_TRACERS)
    t0, buf = x.seeded_tend(MAX_TRACERS)
    x.add_tracer_tend(buf, nt=1)                      # one tracer of three: planes 1 and 2 stay
    got = buf.to_host()
    _same(got[1:], x.padded(t0)[1:], "planes beyond NTracers")
    want = t0.copy()
    want[0][x.active] = (t0[0] + alone[0])[x.active]  # accumulated, not overwritten
    _same(got[0], x.padded(want)[0], "TracerTend[0]")
    assert not np.array_equal(want[0][x.active], t0[0][x.active])
    x.add_tracer_tend(buf, nt=MAX_TRACERS)            # an odd count: a pair and a single
    want2 = x.restated_tend(want.copy(), want_s, nt=MAX_TRACERS)
    _same(buf.to_host(), x.padded(want2), "TracerTend (three tracers onto the first call)")
    got = x.redi.add_tracer_tend(np.nan_to_num(t0[:NT]), x.h, x.tr[:NT], NT)  # the numpy form of the binding
    _same(got[:, x.active], x.restated_tend(np.nan_to_num(t0[:NT]), want_s)[:, x.active], "TracerTend (numpy form)")
    hb, tb = x.dev(x.h), x.dev(x.tr)
    before = buf.to_host()
    for nt in (0, -1, MAX_TRACERS + 1):  # refused before anything is launched
        with pytest.raises(oa.OmegaAmdError, match="NTracers"):
            x.redi.add_tracer_tend(buf.ptr, hb.ptr, tb.ptr, nt)
    oa.device_synchronize()
    _same(buf.to_host(), before, "TracerTend after the refused calls")


# ---------------------------------------------------------------------------------------------------------------------
# attached to the split-explicit stepper
# ---------------------------------------------------------------------------------------------------------------------
STEP_K, NSUB, STEP_DT = 5, 3, 20.0


def step_rig(attached, mono=False):
    """tests.split_explicit_fixtures.StepRig on hex24x20 with an Eos (its own where PressureGrad is attached), a
    GentMcWilliams, a Redi and a VertMixStep on the rig's VertCoord, optionally a MonotoneAdv (the Tendencies' own
    horizontal advection then off).  The VertMix has its shear and convective terms off: its coefficients are then
    the background's whatever the tracers are, so that what the closure changes in a step can be told apart from what
    the mixing scheme makes of the changed stratification."""
    cfg = dict(TracerHorzAdvTendencyEnable=0) if mono else None
    x = StepRig(K=STEP_K, attached=attached, g=named_mesh("hex24x20"), config=cfg)
    m = x.p.mesh
    if not attached:
        x.eos = oa.Eos(m, STEP_K, "teos10")
    x.gm = oa.GentMcWilliams(m, x.vc, x.eos)
    x.redi = oa.Redi(m, x.vc, x.eos, x.nt, slope_max=0.01)
    x.vm = oa.VertMix(m, x.vc, EnableShearMix=False, EnableConvectiveMix=False)
    x.mix = oa.VertMixStep(m, x.vm, x.vc, x.eos, x.nt)
    x.mono = oa.MonotoneAdv(m, STEP_K, x.nt) if mono else None
    return x


def _stepper(x, gm=False, redi=True, switches_on=True):
    st = x.stepper("Split-Explicit", STEP_DT, NSUB)
    if not switches_on:
        st.set_fused_transport(False)
        st.set_momentum_rhs(False)
        st.set_folded_updates(False)
    st.attach_vert_mix(x.mix)
    if x.mono is not None:
        st.attach_monotone_adv(x.mono)
    if gm:
        st.attach_gent_mcwilliams(x.gm)
    if redi:
        x.mix.attach_redi(x.redi)
        st.attach_redi(x.redi)
    return st


def hand_step(x, dt_seconds, nsub, t0=0.0, gm=False):
    """SplitExplicitStepper::doStep with steps 5b, 5c and the Redi term through the public calls, on the null stream
    (after tests.test_gent_mcwilliams_gpu.hand_step)"""
    p, bm = x.p, x.bm
    m, K = p.mesh, x.K
    dt = oa.coeff_seconds(1.0, dt_seconds)
    st, tend = p.state, p.tend
    h_cur, u_cur, h_next, u_next = st.device_ptr(0, 0), st.device_ptr(1, 0), st.device_ptr(0, 1), st.device_ptr(1, 1)
    tr_cur = p.tracers.device_ptr(0)
    tend.set_time(t0)
    tend.compute_all_tendencies(st, p.aux, p.tracers, 0, 0, 0)                       # 1
    vel_tend = tend.device_ptr(1)[0]
    bm.split_velocity(h_cur, u_cur, with_ssh=True)                                   # 2
    bm.compute_residual_forcing(h_cur, vel_tend)                                     # 3
    bm.subcycle(nsub, dt / nsub)                                                     # 4
    bm.transport_velocity(u_cur, u_next)                                             # 5
    if gm:
        x.gm.update_column(h_cur, tr_cur, x.nt)                                      # 5b
        x.gm.compute(h_cur, u_next)
    else:
        x.redi.update_column(h_cur, tr_cur, x.nt)                                    # 5c
    x.redi.compute_slope(h_cur)
    tend.compute_thickness_tendencies(st, p.aux, 0, 1)                               # 6
    oa.update_by_tend(h_next, h_cur, tend.device_ptr(0)[0], dt, m.NCellsAll, oa.level_pitch(K))
    tend.compute_tracer_tendencies(st, p.aux, p.tracers, 0, 0, 1)                    # 7
    tr_tend = tend.device_ptr(2)[0]
    if x.mono is not None:
        x.mono.add_tracers(tr_tend, h_cur, h_next, u_next, tr_cur, x.nt, dt)
    x.redi.add_tracer_tend(tr_tend, h_cur, tr_cur, x.nt)
    oa.device_synchronize()
    cur, nxt = p.tracers.copy_to_host(0), p.tracers.copy_to_host(1)
    hc, hn = st.copy_to_host(0)[0], st.copy_to_host(1)[0]
    n = m.NCellsAll
    nxt[:, :n] = (cur[:, :n] * hc[:n] + dt * tend.get(2)[:, :n]) / hn[:n]
    p.tracers.copy_to_device(nxt, 1)
    bm.advance_velocity(u_cur, vel_tend, dt, u_next)                                 # 8
    x.mix.apply_state(st, p.tracers, dt_seconds, 1, 1)                               # 9 (with the Redi attached to it)
    st.update_time_levels()
    p.tracers.update_time_levels()
    oa.device_synchronize()


@pytest.mark.parametrize("mono", [False, True], ids=["centred", "monotone"])
@pytest.mark.parametrize("gm", [False, True], ids=["alone", "with_gm"])
@pytest.mark.parametrize("attached", [True, False], ids=["pgrad_vertadv", "nothing_attached"])
def test_step_equals_its_calls_by_hand(attached, gm, mono):
    a, b = step_rig(attached, mono), step_rig(attached, mono)
    st = _stepper(a, gm=gm, switches_on=not mono)
    st.do_step(a.p.state)
    oa.device_synchronize()
    before = oa.device_resource_count()
    st.do_step(a.p.state)
    oa.device_synchronize()
    assert oa.device_resource_count() == before  # a step with the closure attached allocates nothing
    b.mix.attach_redi(b.redi)
    for i in range(2):
        hand_step(b, STEP_DT, NSUB, i * STEP_DT, gm=gm)
    for name, got, want, start in zip(("h", "u", "tracers"), a.result(), b.result(), (a.h, a.u, a.tr)):
        assert np.all(np.isfinite(got)), name
        _same(got, want, f"{name}: the stepper against its calls by hand")
        assert not np.array_equal(got, start), name
    for name in ("SlopeInterface", "VertDiffusivity"):
        _same(a.redi.get(name), b.redi.get(name), name)
        assert np.abs(a.redi.get(name)).max() > 0.0
    _same(a.vm.get("VertDiff"), b.vm.get("VertDiff"), "VertDiff")


@pytest.mark.parametrize("gm", [False, True], ids=["alone", "with_gm"])
@pytest.mark.parametrize("attached", [True, False], ids=["pgrad_vertadv", "nothing_attached"])
def test_redi_moves_the_tracers_only(attached, gm):
    """One step with the closure against one without (the same stepper, the same VertMixStep, no Redi on either): the
    velocity and the thickness are the same bit for bit, the tracers differ, and VertMix's VertDiff is the unattached
    one plus VertDiffusivity.  Detaching restores the unattached bits."""
    a, b, c = step_rig(attached), step_rig(attached), step_rig(attached)
    _stepper(a, gm=gm).do_step(a.p.state)
    _stepper(b, gm=gm, redi=False).do_step(b.p.state)
    st = _stepper(c, gm=gm)
    st.attach_redi(None)
    c.mix.attach_redi(None)
    st.do_step(c.p.state)
    (ha, ua, ta), (hb, ub, tb), (hc, uc, tc) = a.result(), b.result(), c.result()
    _same(ua, ub, "u after the step")
    _same(ha, hb, "h after the step")
    n = a.p.mesh.NCellsAll
    assert not np.array_equal(ta[:, :n], tb[:, :n])
    print(f"attached {attached} gm {gm}: max |T, S with - without| = {np.abs(ta[:, :n] - tb[:, :n]).max():.3e}")
    d = a.redi.get("VertDiffusivity")
    assert np.abs(d[:n]).max() > 0.0 and np.all(d[:n] >= 0.0)
    _same(a.vm.get("VertDiff")[:n], b.vm.get("VertDiff")[:n] + d[:n], "VertDiff = the unattached one + VertDiffusivity")
    for name, got, want in zip(("h", "u", "tracers"), (hc, uc, tc), (hb, ub, tb)):
        _same(got, want, f"{name}: detached against unattached")
    assert np.all(c.redi.get("SlopeInterface") == 0.0)  # never computed
    _same(c.vm.get("VertDiff"), b.vm.get("VertDiff"), "VertDiff (detached)")


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
            oa.Redi(*args, 2)
    for kw, msg in ((dict(kappa=-1.0), "RediKappa"), (dict(kappa=np.inf), "RediKappa"), (dict(slope_max=0.0), "SlopeMax"),
                    (dict(slope_max=np.nan), "SlopeMax"), (dict(n2_floor=0.0), "N2Floor"), (dict(n2_floor=np.inf), "N2Floor")):
        with pytest.raises(oa.OmegaAmdError, match=msg):
            oa.Redi(m, vc, eos, 2, **kw)
    with pytest.raises(oa.OmegaAmdError, match="MaxTracers"):
        oa.Redi(m, vc, eos, 0)
    r = oa.Redi(m, vc, eos, 2, kappa=0.0)  # zero is a diffusivity
    with pytest.raises(oa.OmegaAmdError, match="no array named"):
        r.get("NoSuchArray")
    big = oa.HorzMesh(d, 1025)
    with pytest.raises(oa.OmegaAmdError, match="1 <= NVertLayers <= 1024"):
        oa.Redi(big, oa.VertCoord(big, 1025, RHO0, "Uniform", decomp=d), oa.Eos(big, 1025, "linear"), 2)
    # ---- VertMixStep::attachRedi
    x = step_rig(True)
    pm = x.p.mesh
    other_vc = oa.VertCoord(pm, STEP_K, RHO0, "Uniform", decomp=x.p.decomp)
    other_eos = oa.Eos(pm, STEP_K, "teos10")
    with pytest.raises(oa.OmegaAmdError, match="another mesh or layer count"):
        x.mix.attach_redi(r)
    with pytest.raises(oa.OmegaAmdError, match="different VertCoord or Eos"):
        x.mix.attach_redi(oa.Redi(pm, other_vc, x.eos, 2))
    with pytest.raises(oa.OmegaAmdError, match="different VertCoord or Eos"):
        x.mix.attach_redi(oa.Redi(pm, x.vc, other_eos, 2))
    # ---- SplitExplicitStepper::attachRedi
    with pytest.raises(oa.OmegaAmdError, match="Split-Explicit"):
        x.stepper("RungeKutta4", STEP_DT).attach_redi(x.redi)
    st = x.stepper("Split-Explicit", STEP_DT, NSUB)
    base = x.result()
    with pytest.raises(oa.OmegaAmdError, match="no VertMixStep attached"):
        st.attach_redi(x.redi)
    st.attach_vert_mix(x.mix)
    with pytest.raises(oa.OmegaAmdError, match="does not have this Redi attached"):
        st.attach_redi(x.redi)
    x.mix.attach_redi(oa.Redi(pm, x.vc, x.eos, 2))
    with pytest.raises(oa.OmegaAmdError, match="does not have this Redi attached"):
        st.attach_redi(x.redi)
    x.mix.attach_redi(x.redi)
    with pytest.raises(oa.OmegaAmdError, match="another mesh or layer count"):
        st.attach_redi(r)
    with pytest.raises(oa.OmegaAmdError, match="MaxTracers = 1"):
        st.attach_redi(oa.Redi(pm, x.vc, x.eos, 1))
    with pytest.raises(oa.OmegaAmdError, match="PressureGrad"):  # the rig's PressureGrad is on x.vc and x.eos
        st.attach_redi(oa.Redi(pm, other_vc, x.eos, 2))
    y = step_rig(False)  # no PressureGrad: the GentMcWilliams's objects decide
    sty = y.stepper("Split-Explicit", STEP_DT, NSUB)
    sty.attach_vert_mix(y.mix)
    sty.attach_gent_mcwilliams(oa.GentMcWilliams(y.p.mesh, y.vc, oa.Eos(y.p.mesh, STEP_K, "teos10")))
    y.mix.attach_redi(y.redi)
    with pytest.raises(oa.OmegaAmdError, match="GentMcWilliams"):
        sty.attach_redi(y.redi)
    sty.attach_gent_mcwilliams(y.gm)
    sty.attach_redi(y.redi)
    y.mix.attach_redi(None)  # checked again in every step
    with pytest.raises(oa.OmegaAmdError, match="does not have this Redi attached"):
        sty.do_step(y.p.state)
    one = oa.Tracers(pm, None, STEP_K, 1, 2)
    tend1 = oa.Tendencies(pm, STEP_K, 1, oa.default_config(SSHTendencyEnable=1))
    aux1 = oa.AuxiliaryState(pm, None, STEP_K, 1)
    st1 = oa.TimeStepper("Split-Explicit", STEP_DT, tend1, aux1, pm, None, one)
    with pytest.raises(oa.OmegaAmdError, match="tracers"):
        st1.attach_redi(x.redi)
    st.attach_redi(x.redi)
    for got, want in zip(x.result(), base):
        _same(got, want, "a refused attachment leaves the state alone")
