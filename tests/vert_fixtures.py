"""Shared rigs of the vertical-column GPU tests (VertCoord / Eos: `Col`; VertMix: `Mix`), the layer-range generators
they draw from, and Python restatements of the launch rules of kernels/ColumnKernels.hip, kernels/VertAdvKernels.hip
(its column launch) and kernels/VertMixKernels.hip (which tile, how many columns per workgroup, how many right-hand sides per pass, how much
LDS), so that a shape sweep can assert which branch each of its cases lands on."""
import numpy as np

import omega_amd as oa
from tests import column_reference as CR
from tests import vert_mix_reference as MR
from tests.column_reference import RHO0
from tests.rank_rig import RankRig

VC_OUT = ("PressureInterface", "PressureMid", "ZInterface", "ZMid", "GeopotentialMid", "LayerThicknessTarget")
EOS_OUT = ("SpecVol", "SpecVolDisplaced")
MIX_OUT = ("VertDiff", "VertVisc", "BruntVaisalaFreqSq")
COL_NT = 3  # tracers of `Col`: T and S are picked by index (1 and 2 in some cases: not only the default 0 / 1)
MIX_NT = 6


# ---------------------------------------------------------------------------------------------------------------------
# launch rules, restated
# ---------------------------------------------------------------------------------------------------------------------
STAGE_PRESSURE, STAGE_SPEC_VOL, STAGE_SPEC_VOL_DISP, STAGE_ZHEIGHT, STAGE_GEOPOTENTIAL, STAGE_TARGET = (
    1, 2, 4, 8, 16, 32)
FUSED = STAGE_PRESSURE | STAGE_SPEC_VOL | STAGE_ZHEIGHT | STAGE_GEOPOTENTIAL
LDS_BYTES = 65536
MIX_MAX_ROWS = 1024  # TriDiagMaxRows
MIX_LANES = 256
MIX_CHUNKS = (1, 2, 4, 6, 8)


def level_pitch(K):
    """Base.h levelPitch: rows of 16 or more levels are padded to a multiple of 16 values"""
    return (K + 15) // 16 * 16 if (K >= 16 and K % 16 != 0) else K


def lds_pitch(P):
    """ColumnKernels.hip ldsPitch: odd"""
    return P + (1 if P % 2 == 0 else 0)


def column_lds_doubles(mask, tile, K):
    """ColLayout(mask, tile, LP, LP1).End"""
    lp, lp1 = lds_pitch(level_pitch(K)), lds_pitch(level_pitch(K + 1))
    need_h = bool(mask & (STAGE_PRESSURE | STAGE_ZHEIGHT | STAGE_TARGET))
    need_b = bool(mask & (STAGE_PRESSURE | STAGE_SPEC_VOL | STAGE_SPEC_VOL_DISP | STAGE_ZHEIGHT | STAGE_GEOPOTENTIAL))
    need_s = bool(mask & STAGE_ZHEIGHT)
    return (tile * lp + tile * lp1 if need_h else 0) + (tile * lp if need_b else 0) + (tile * lp if need_s else 0) \
        + 3 * tile


def column_tile(mask, K):
    """launchColumn: the largest of 16, 8, 4, 2 columns per workgroup whose LDS layout fits 64 KiB; None: refused"""
    for tile in (16, 8, 4, 2):
        if column_lds_doubles(mask, tile, K) * 8 <= LDS_BYTES:
            return tile
    return None


def column_limit(mask):
    """the largest NVertLayers a column launch of this stage mask accepts"""
    K = 1
    while column_tile(mask, K + 1) is not None:
        K += 1
    return K


def vert_adv_lds_doubles(tile, K):
    """VertAdvKernels.hip colLdsDoubles: three [tile][LP] buffers (tendency, reference thickness or nothing,
    transport) and the per-column layer range (2 x tile ints = tile doubles)"""
    return tile * (3 * lds_pitch(level_pitch(K)) + 1)


def vert_adv_tile(K):
    """vertAdvColumnTile: the largest of 16, 8, 4, 2 columns per workgroup whose LDS fits 64 KiB; None: refused"""
    for tile in (16, 8, 4, 2):
        if vert_adv_lds_doubles(tile, K) * 8 <= LDS_BYTES:
            return tile
    return None


def vert_adv_limit():
    """the largest NVertLayers the VertAdv column launch accepts (VertAdv::maxLayers)"""
    K = 1
    while vert_adv_tile(K + 1) is not None:
        K += 1
    return K


def rows_unaligned(K):
    """True if some row of a [cell][levelPitch(K)] array of doubles does not start on 16 bytes"""
    return level_pitch(K) % 2 == 1


def pcr_levels(n):
    lev = 0
    while (1 << lev) < n:
        lev += 1
    return lev


def systems_launch(K):
    """what launchMix and launchBolusVelocity share: (columns per workgroup, the lanes they occupy, the lanes of the
    workgroup) -- as many whole columns as 256 lanes hold, a longer column alone, whole wavefronts"""
    sys = MIX_LANES // K if K <= MIX_LANES else 1
    rows = sys * K
    return sys, rows, (rows + 63) // 64 * 64


def mix_launch(K, nrhs):
    """launchMix (PackedShape of kernels/PackedColumns.h, mixChunk): columns per workgroup, lanes, right-hand sides per pass and its LDS cap, passes,
    dynamic LDS bytes"""
    sys, rows, threads = systems_launch(K)
    cap = (LDS_BYTES // 8 // rows - 4) // 2
    chunk = 1
    for o in MIX_CHUNKS:
        if o <= cap and chunk < nrhs:
            chunk = o
    want = next(o for o in MIX_CHUNKS if o >= min(nrhs, MIX_CHUNKS[-1]))  # what the rule picks without the LDS limit
    return dict(Sys=sys, Rows=rows, Threads=threads, Cap=cap, Chunk=chunk, Capped=chunk < want,
                Passes=-(-nrhs // chunk), LdsBytes=(4 + 2 * chunk) * rows * 8, PadLanes=threads - rows,
                Levels=pcr_levels(K))


# ---------------------------------------------------------------------------------------------------------------------
# layer ranges
# ---------------------------------------------------------------------------------------------------------------------
def column_levels(rng, n, K, kinds):
    """Global 1-based (minLevelCell, maxLevelCell) of n cells: full columns, KMin > 0 to the bottom, short, single
    layer, random and (kinds = 6) land, one kind per cell.  Valid for every K >= 1: a kind that does not exist at that
    K (KMin > 0 at K = 1, three layers at K = 2) falls back to the nearest one that does."""
    kind = rng.integers(0, kinds, n)
    mn, mx = np.ones(n, np.int32), np.full(n, K, np.int32)
    a = np.minimum(rng.integers(2, max(3, K // 3), n), K)
    mn[kind == 1] = a[kind == 1]                                     # KMin > 0, to the bottom
    mx[kind == 2] = np.minimum(rng.integers(1, 4, n), K)[kind == 2]  # short columns
    s = rng.integers(1, K + 1, n)
    mn[kind == 3], mx[kind == 3] = s[kind == 3], s[kind == 3]        # single layer
    lo = rng.integers(1, K + 1, n)
    hi = np.minimum(K, lo + rng.integers(0, K, n))
    mn[kind == 4], mx[kind == 4] = lo[kind == 4], hi[kind == 4]      # random
    mx[kind == 5] = 0                                                # land: MaxLayerCell -1
    return mn, mx


def ragged_depths(K):
    """The depths one workgroup of the mixing solve should see side by side: 1, 2, 3, a power of two, a power of two
    plus one, full depth, and 0 (land); those that exceed K are dropped."""
    p2 = 1 << max(pcr_levels(K) - 1, 0)  # the largest power of two below K (K itself for K = 1)
    d = [x for x in (1, 2, 3, p2, p2 + 1, K) if x <= K]
    return sorted(set(d)) + [0]


def ragged_levels_local(rng, n_local, K):
    """Per local cell index, cycling through ragged_depths(K) (an odd cycle where possible, so that every pair of
    neighbours occurs in a two-column workgroup): 1-based (min, max); two columns in three start at the top."""
    depths = ragged_depths(K)
    if len(depths) % 2 == 0 and len(depths) > 2:
        depths = depths + [depths[0]]
    mn, mx = np.ones(n_local, np.int32), np.zeros(n_local, np.int32)
    for c in range(n_local):
        d = depths[c % len(depths)]
        if d == 0:
            continue
        top = 0 if c % 3 else int(rng.integers(0, K - d + 1))
        mn[c], mx[c] = top + 1, top + d
    return mn, mx


def col_inputs(g, K, seed):
    """Global per-cell inputs of `Col`: layer ranges, thickness, tracers, surface pressure, tidal potential, SAL,
    bottom depth, reference thickness."""
    n = int(g["nCells"])
    rng = np.random.default_rng(seed)
    mn, mx = column_levels(rng, n, K, 5)
    return dict(
        min_level=mn, max_level=mx,
        h=rng.uniform(0.5, 40.0, (n, K)),
        tr=np.stack([rng.uniform(-1.0, 1.0, (n, K)), rng.uniform(-2.0, 30.0, (n, K)), rng.uniform(30.0, 38.0, (n, K))]),
        ps=rng.uniform(0.9e5, 1.1e5, n), tidal=rng.uniform(-1.0, 1.0, n), sal=rng.uniform(-0.1, 0.1, n),
        bot=rng.uniform(100.0, 6000.0, n), ref=rng.uniform(1.0, 30.0, (n, K)))


def mix_inputs(g, K, seed, full=False, nt=MIX_NT):
    """Global per-cell / per-edge inputs of `Mix`: layer ranges (with land), thickness, tracers (T, S first), edge
    velocities."""
    n, ne = int(g["nCells"]), int(g["nEdges"])
    rng = np.random.default_rng(seed)
    if full:
        rng.integers(0, 6, n)
        mn, mx = np.ones(n, np.int32), np.full(n, K, np.int32)
    else:
        mn, mx = column_levels(rng, n, K, 6)
    tr = np.concatenate([rng.uniform(-2.0, 30.0, (1, n, K)), rng.uniform(30.0, 38.0, (1, n, K)),
                         rng.uniform(-1.0, 1.0, (nt - 2, n, K))])
    return dict(min_level=mn, max_level=mx, h=rng.uniform(0.5, 40.0, (n, K)), tr=tr,
                un=rng.uniform(-0.05, 0.05, (ne, K)), ut=rng.uniform(-0.05, 0.05, (ne, K)))


def same(got, want, name):
    """bit for bit, NaN equal to NaN"""
    assert got.shape == want.shape, name
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), f"{name}: {bad.sum()} elements differ, first at {np.argwhere(bad)[0]}"


# ---------------------------------------------------------------------------------------------------------------------
# rigs
# ---------------------------------------------------------------------------------------------------------------------
class Col(RankRig):
    """One rank's objects (VertCoord, Eos, OceanState, Tracers) with the global inputs in local order."""

    def __init__(self, g, K, eos_kind, nparts=1, rank=0, seed=7, weights="Uniform"):
        super().__init__(g, K, nparts, rank)
        self.eos_kind = eos_kind
        m = self.mesh
        G = self.G = col_inputs(g, K, seed)
        self.h, self.tr = self.cells(G["h"]), self.cells(G["tr"])
        self.ps, self.tidal, self.sal, self.bot, self.ref = (self.cells(G[k]) for k in ("ps", "tidal", "sal", "bot", "ref"))
        self.layers(G["min_level"], G["max_level"], weights=weights)
        self.eos = oa.Eos(m, K, eos_kind)
        self.state = oa.OceanState(m, None, K, 2)
        self.tracers = oa.Tracers(m, None, K, COL_NT, 2)
        self.state.copy_to_device(self.h, np.zeros((m.NEdgesSize, K)), 0)
        self.tracers.copy_to_device(self.tr, 0)
        self.vc.set("BottomDepth", self.bot)
        self.vc.set("RefLayerThickness", self.ref)
        self.poison()

    def poison(self):
        for name in VC_OUT:
            self.vc.set(name, np.full(self.vc.get(name).shape, np.nan))
        for name in EOS_OUT:
            self.eos.set(name, np.full((self.n_size, self.K), np.nan))

    def nan_state(self):
        K, n = self.K, self.n_size
        return {"PressureInterface": np.full((n, K + 1), np.nan), "PressureMid": np.full((n, K), np.nan),
                "ZInterface": np.full((n, K + 1), np.nan), "ZMid": np.full((n, K), np.nan),
                "GeopotentialMid": np.full((n, K), np.nan), "SpecVol": np.full((n, K), np.nan),
                "SpecVolDisplaced": np.full((n, K), np.nan), "LayerThicknessTarget": np.full((n, K), np.nan)}

    def outputs(self):
        out = {name: self.vc.get(name) for name in VC_OUT}
        out.update({name: self.eos.get(name) for name in EOS_OUT})
        return out

    def run_fused(self, kdisp, ti, si):
        self.vc.compute_column(self.state, self.tracers, self.eos, self.ps, self.tidal, self.sal, kdisp=kdisp,
                               temp_index=ti, salt_index=si)
        oa.device_synchronize()

    def run_sequence(self, kdisp, ti, si):
        """the four launches the fused pass replaces, on the device"""
        vc, eos = self.vc, self.eos
        hp = self.state.device_ptr(0)
        tp, sp = oa.tracer_rows_ptr(self.tracers, ti), oa.tracer_rows_ptr(self.tracers, si)
        vc.compute_pressure(hp, self.ps)
        eos.compute_spec_vol(tp, sp, vc.device_ptr("PressureMid"), p_scale=1.0e-4)
        if kdisp is not None:
            eos.compute_spec_vol_disp(tp, sp, vc.device_ptr("PressureMid"), kdisp, p_scale=1.0e-4)
        vc.compute_zheight(hp, eos.device_ptr("SpecVol"))
        vc.compute_geopotential(self.tidal, self.sal)
        oa.device_synchronize()

    def expected(self, kdisp, ti, si):
        st = self.nan_state()
        CR.column_sequence(self.h, self.tr[ti], self.tr[si], self.ps, self.tidal, self.sal, self.bot, self.lo, self.hi,
                           self.n_all, RHO0, self.eos_kind, st, kdisp)
        return st


class Mix(RankRig):
    """One rank's VertCoord, Eos, OceanState, Tracers and VertMix, with the global inputs in local order and the
    column pass (with SpecVolDisplaced at KDisp = 1) already run.  ragged: the layer ranges cycle through
    ragged_depths(K) in local cell order instead of being drawn at random.  column_pass = False skips the column pass
    (NVertLayers beyond its limit): N^2 and the coefficients are then the caller's to set."""

    def __init__(self, g, K, eos_kind="teos10", nparts=1, rank=0, seed=7, full=False, ntracers=MIX_NT, ragged=False,
                 column_pass=True, **cfg):
        super().__init__(g, K, nparts, rank)
        self.nt = ntracers
        m = self.mesh
        G = self.G = mix_inputs(g, K, seed, full, ntracers)
        if ragged:
            mn, mx = ragged_levels_local(np.random.default_rng(seed + 1), self.n_all, K)
            G["min_level"][self.crow], G["max_level"][self.crow] = mn, mx
        self.h, self.tr = self.cells(G["h"]), self.cells(G["tr"])
        self.un, self.ut = self.edges(G["un"]), self.edges(G["ut"])
        self.layers(G["min_level"], G["max_level"])
        self.eos = oa.Eos(m, K, eos_kind)
        self.state = oa.OceanState(m, None, K, 2)
        self.tracers = oa.Tracers(m, None, K, ntracers, 2)
        self.state.copy_to_device(self.h, self.un, 0)
        self.tracers.copy_to_device(self.tr, 0)
        if column_pass:
            self.vc.compute_column(self.state, self.tracers, self.eos, kdisp=1)
            oa.device_synchronize()
        self.vm = oa.VertMix(m, self.vc, **cfg)
        self.cfg = MR.config(**cfg)
        for name in MIX_OUT:
            self.vm.set(name, np.full((self.n_size, K), np.nan))

    def mesh_arrays(self):
        m = self.mesh
        return (m.get_array("NEdgesOnCell"), m.get_array("EdgesOnCell"), m.get_array("DcEdge"),
                m.get_array("DvEdge"), m.get_array("AreaCell"))

    def expected_coefficients(self, un, ut, n2):
        return MR.coefficients(un, ut, n2, self.vc.get("ZMid"), self.lo, self.hi, self.n_all, *self.mesh_arrays(),
                               self.cfg)

    def expected_bvf(self):
        return MR.bvf(self.eos.get("SpecVol"), self.eos.get("SpecVolDisplaced"), self.vc.get("ZMid"), self.lo,
                      self.hi, self.n_all, RHO0)

    def compute(self, ut=None, stream=None):
        self.vm.compute_bvf(self.eos, stream=stream)
        self.vm.compute(self.un, self.ut if ut is None else ut, stream=stream)
        oa.device_synchronize()

    def seeded_tracers(self):
        """time level 0: the tracers, NaN outside each owned column's range, on halo and sentinel rows and in the
        pad of land; time level 1: distinct values"""
        t0 = np.full_like(self.tr, np.nan)
        for c in range(self.n_own):
            lo, hi = self.lo[c], self.hi[c]
            if 0 <= lo <= hi < self.K:
                t0[:, c, lo: hi + 1] = self.tr[:, c, lo: hi + 1]
        t1 = np.arange(self.tr.size, dtype=np.float64).reshape(self.tr.shape) * 0.5 + 0.25
        self.tracers.copy_to_device(t0, 0)
        self.tracers.copy_to_device(t1, 1)
        return t0, t1

    def seeded_velocity(self):
        """u at level 0 with NaN outside each owned edge's range and on halo / sentinel rows; level 1 distinct"""
        lo, hi = self.lo_e, self.hi_e
        u0 = np.full_like(self.un, np.nan)
        for e in range(self.e_own):
            if 0 <= lo[e] <= hi[e] < self.K:
                u0[e, lo[e]: hi[e] + 1] = self.un[e, lo[e]: hi[e] + 1]
        u1 = np.arange(self.un.size, dtype=np.float64).reshape(self.un.shape) * 0.25 - 3.0
        self.state.copy_to_device(self.h, u0, 0)
        self.state.copy_to_device(self.h, u1, 1)
        return u0, u1, lo, hi
