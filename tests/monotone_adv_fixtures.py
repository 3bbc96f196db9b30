"""Shared by the MonotoneAdv tests (CPU: tests/test_monotone_adv.py, tests/test_monotone_adv_3d.py,
tests/test_monotone_adv_high_order.py; GPU: their *_gpu.py counterparts and tests/test_c_abi_monotone_adv*.py): one
rank's mesh as the restatement reads it and the inputs of one forward step, for the 2-D form (MonoRig), the 3-D form
(Mono3Rig) and either with the library's tables for one order (HoRig, Ho3Rig: `set_order`).

The inputs: h in 5 .. 30 m, u of both signs with some edges at u == 0.0 exactly (the tie of the upwind flux thickness),
Dt such that the largest outflow Courant number Dt*(sum of outflow)/(AreaCell*h) is 0.4, hNew from the same mass fluxes,
and three tracers: a 0/1 step, a uniform random field and a constant.  Rows >= NCellsAll / NEdgesAll (the sentinel
rows) hold NaN: nothing may read them.  The fixture asserts that its inputs exercise the limiter: on the random tracer at
least 20 % of the masked-in edge-levels are limited (Sc < 1) and at least 20 % are not (Sc == 1); the constant tracer
has no limited edge-level.

Mono3Rig adds ragged layer ranges and a vertical transport.  The ranges are drawn per global cell (so every part of a
decomposition sees the same): KMin in 0 .. 2, KMax in K-4 .. K-1, both clipped to 0 <= KMin <= KMax < K, and one column
in sixteen is land (MaxLayerCell = -1).  VerticalTransport is uniform in +-amp on the interfaces KMin < K <= KMax and NaN
everywhere else -- at KMin, outside the range, on land and on the sentinel row: nothing may use it there.  amp is the
median horizontal outflow rate (sum of outflow |Fm|)/AreaCell of the mesh, so that the two directions limit each other
on every mesh.  Dt puts the largest combined outflow Courant number
Dt*(horizontal outflow + max(Wv[K], 0) + max(-Wv[K+1], 0))/h at 0.4, hNew is the thickness of the same fluxes, and the
step tracer jumps in x and at mid-depth.  It asserts (on request: `check`) that its inputs show the need and exercise
the limiter: the parent's path -- the 2-D limiter plus VertAdv's unlimited order-2 vertical flux -- leaves the 3-D
neighbourhood range by more than 1e-2 on the step and on the random tracer, and on the random tracer at least 20 % of
the interfaces that carry flux are limited (ScV < 1) and at least 20 % are not.

`check_ho` asserts that the inputs exercise the limiter with the high-order flux as well: the two edge-level checks
above with the corrected flux, and on fib700_coast_ragged at least 5 % of the edges are high and at least 5 % of the
masked-in edges are not, so that both branches of the correction's select are compared."""
import numpy as np

import omega_amd as oa
from tests import column_reference as CR
from tests import monotone_adv_reference as MR
from tests import vert_adv_reference as VR
from tests.meshes import named_mesh

COURANT = 0.4
STEP, RANDOM, CONST = 0, 1, 2
CONST_VALUE = 3.7
ORDERS = ((4, 0.25), (3, 0.25))  # (order, Coef3rdOrder): beta = 0.0 and beta = 0.25


class Inputs:
    pass


class MonoRig:
    """One rank's mesh (host-only unless `device`) with the restatement's view of it; after `set_order`, `H` the
    library's tables of (order, coef) on it"""

    def __init__(self, g, K, nparts=1, rank=0, device=False, halo=3):
        if isinstance(g, str):
            g = named_mesh(g)
        self.g, self.K = g, K
        self.decomp = oa.Decomp(oa.GlobalMesh(g), nparts, rank, halo)
        self.mesh = m = oa.HorzMesh(self.decomp, K, host_only=not device)
        self.nc, self.ne, self.nc_size, self.ne_size = m.NCellsAll, m.NEdgesAll, m.NCellsSize, m.NEdgesSize
        self.M = MR.MonoMesh.of(m)
        self.area = m.get_array("AreaCell")

    def set_order(self, order, coef=0.25):
        self.order, self.coef = order, coef
        self.H = MR.HoTables.of(self.M, self.mesh, self.g, order, coef)
        return self

    def inputs(self, seed=0, upwind=False, ntracers=3, check=True):
        """h_old, h_new [NCellsSize][K], u [NEdgesSize][K], tracers [ntracers][NCellsSize][K], dt.  The first three
        tracers are the step, the random field and the constant; further ones are random fields of other ranges."""
        rng = np.random.default_rng(seed)
        M, K, nc, ne = self.M, self.K, self.nc, self.ne
        I = Inputs()
        I.upwind = bool(upwind)
        I.h_old = np.full((self.nc_size, K), np.nan)
        I.h_old[:nc] = rng.uniform(5.0, 30.0, (nc, K))
        I.u = np.full((self.ne_size, K), np.nan)
        I.u[:ne] = rng.uniform(-1.0, 1.0, (ne, K))
        I.u[:ne][rng.random((ne, K)) < 0.05] = 0.0
        div, out = MR.mass_divergence(M, I.h_old, I.u, upwind)
        I.dt = float(COURANT / (out / I.h_old[:nc]).max())
        I.h_new = np.full((self.nc_size, K), np.nan)
        I.h_new[:nc] = I.h_old[:nc] + I.dt * div
        I.courant = I.dt * out / I.h_old[:nc]
        assert I.h_new[:nc].min() > 0.0 and abs(I.courant.max() - COURANT) < 1e-12
        I.tracers = np.full((ntracers, self.nc_size, K), np.nan)
        x = self.mesh.get_array("XCell")[:nc]
        I.tracers[STEP, :nc] = (x > np.median(x)).astype(float)[:, None]
        if ntracers > RANDOM:
            I.tracers[RANDOM, :nc] = rng.uniform(0.0, 1.0, (nc, K))
        if ntracers > CONST:
            I.tracers[CONST, :nc] = CONST_VALUE
        for L in range(3, ntracers):
            I.tracers[L, :nc] = rng.uniform(-1.0, 1.0, (nc, K)) * 10.0 ** (L % 4)
        if check and ntracers >= 3:
            self.check(I)
        return I

    def vert(self, I):
        """the 3-D form's extra inputs (the layer ranges are the rig's), or None"""
        return (I.wt, self.lo, self.hi) if hasattr(I, "wt") else None

    def hess(self, I, L):
        return MR.hessians(self.H, I.tracers[L])

    def limited_fraction(self, I, L, high=False):
        """the fractions of the masked-in edge-levels with Sc < 1 and with Sc == 1 (the horizontal passes alone)"""
        high = (self.H, self.hess(I, L)) if high else None
        si, so, _, _ = MR.scale_factors(self.M, I.h_old, I.h_new, I.u, I.tracers[L], I.dt, I.upwind, high=high)
        sc = MR.edge_limits(self.M, I.h_old, I.u, I.tracers[L], si, so, I.upwind, high)
        return float((sc < 1.0).mean()), float((sc == 1.0).mean())

    def check_edges(self, I, high=False):
        lim, free = self.limited_fraction(I, RANDOM, high)
        assert lim >= 0.2 and free >= 0.2, (lim, free)
        assert self.limited_fraction(I, CONST, high) == (0.0, 1.0)
        return lim, free

    def check(self, I):
        self.check_edges(I)

    def check_ho(self, I):
        lim, free = self.check_edges(I, high=True)
        if not self.M.open_edge.all():  # a coast
            high, open_ = self.H.high, self.M.open_edge
            assert high.mean() >= 0.05 and (open_ & ~high).sum() >= 0.05 * open_.sum(), (high.mean(), open_.mean())
        return lim, free

    def _reference(self, I, ntracers, tend0, max_tracers, vert, high):
        """(Tend, ScaleIn, ScaleOut, Hess) of the restatement, from tend0 (default zeros), zero scale arrays and NaN in
        Hess, which stays so unless `high`"""
        tend = np.zeros((ntracers, self.nc_size, self.K)) if tend0 is None else tend0.copy()
        si = np.zeros((max_tracers or ntracers, self.nc_size, self.K))
        so = np.zeros_like(si)
        hess = np.full((max_tracers or ntracers, 3, self.nc_size, self.K), np.nan)
        MR.add_tracer_tend(self.M, tend, I.h_old, I.h_new, I.u, I.tracers, ntracers, I.dt, I.upwind, si, so,
                           self.vert(I) if vert else None, (self.H, hess) if high else None)
        return tend, si, so, hess

    def reference(self, I, ntracers, tend0=None, max_tracers=None):
        """(Tend, ScaleIn, ScaleOut) at order 2, of the 3-D form where the inputs carry a vertical transport"""
        return self._reference(I, ntracers, tend0, max_tracers, True, False)[:3]

    def reference_2d(self, I, ntracers, tend0=None, max_tracers=None):
        """the same without the vertical part"""
        return self._reference(I, ntracers, tend0, max_tracers, False, False)[:3]

    def reference_ho(self, I, ntracers, tend0=None, max_tracers=None):
        """(Tend, ScaleIn, ScaleOut, Hess) at the order of `set_order`"""
        return self._reference(I, ntracers, tend0, max_tracers, True, True)


def global_ranges(n, K, seed=17):
    """0-based (KMin, KMax) of n global cells; land: (0, -1)"""
    rng = np.random.default_rng(seed)
    hi = np.clip(K - 1 - rng.integers(0, 4, n), 0, K - 1)
    lo = np.minimum(rng.integers(0, 3, n), hi)
    land = rng.integers(0, 16, n) == 0
    lo[land], hi[land] = 0, -1
    return lo.astype(np.int32), hi.astype(np.int32)


class Mono3Rig(MonoRig):
    def __init__(self, g, K, nparts=1, rank=0, device=False, halo=3):
        super().__init__(g, K, nparts, rank, device, halo)
        lo, hi = global_ranges(int(self.g["nCells"]), K)
        self.min_level, self.max_level = lo + 1, hi + 1  # the global 1-based arrays a VertCoord takes
        self.cell_id = self.decomp.get_array("CellID")
        self.lo, self.hi = CR.local_layer_ranges(self.cell_id, self.min_level, self.max_level, self.nc, self.nc_size, K)
        self.inside = MR.interface_mask(self.lo, self.hi, self.nc, K)

    def inputs(self, seed=0, upwind=False, ntracers=3, check=True, wt_scale=1.0):
        I = super().inputs(seed, upwind, ntracers, check=False)
        rng = np.random.default_rng(seed + 1000)
        M, K, nc = self.M, self.K, self.nc
        div, out = MR.mass_divergence(M, I.h_old, I.u, upwind)
        I.wt_amp = float(np.median(out)) * wt_scale
        # drawn per global cell, so that the parts of a decomposition agree
        wt_g = rng.uniform(-1.0, 1.0, (int(self.g["nCells"]), K))
        I.wt = np.full((self.nc_size, K), np.nan)
        I.wt[:nc][self.inside] = (I.wt_amp * wt_g[self.cell_id[:nc] - 1])[self.inside]
        vdiv, vout = MR.thickness_divergence(I.wt, self.lo, self.hi, nc)
        I.dt = float(COURANT / ((out + vout) / I.h_old[:nc]).max())
        I.h_new[:nc] = I.h_old[:nc] + I.dt * (div + vdiv)
        I.courant = I.dt * (out + vout) / I.h_old[:nc]
        assert I.h_new[:nc].min() > 0.0 and abs(I.courant.max() - COURANT) < 1e-12
        x = self.mesh.get_array("XCell")[:nc]
        I.tracers[STEP, :nc] = ((x > np.median(x))[:, None] != (np.arange(K) >= (K + 1) // 2)[None, :]).astype(float)
        I.lo, I.hi = self.lo, self.hi
        if check and ntracers >= 3:
            self.check(I)
        return I

    def forward(self, I, L, tend):
        return (I.h_old[: self.nc] * I.tracers[L, : self.nc] + I.dt * tend) / I.h_new[: self.nc]

    def parent_path_excess(self, I, L):
        """how far the parent's update -- the 2-D limiter and VertAdv's order-2 term, unlimited -- leaves the 3-D range"""
        nc, M = self.nc, self.M
        si, so, _, _ = MR.scale_factors(M, I.h_old, I.h_new, I.u, I.tracers[L], I.dt, I.upwind)
        tend = np.zeros((1, self.nc_size, self.K))
        tend[0, :nc] = MR.flux_divergence(M, I.h_old, I.u, I.tracers[L], si, so, I.upwind)
        VR.add_tracer_tend(tend, I.h_old, I.tracers[L: L + 1], I.wt, self.lo, self.hi, nc, 2)
        new = self.forward(I, L, tend[0, :nc])
        _, _, p_min, p_max = MR.scale_factors(M, I.h_old, I.h_new, I.u, I.tracers[L], I.dt, I.upwind, self.vert(I))
        return float(max((new - p_max).max(), (p_min - new).max()))

    def limited_interfaces(self, I, L):
        si, so, _, _ = MR.scale_factors(self.M, I.h_old, I.h_new, I.u, I.tracers[L], I.dt, I.upwind, self.vert(I))
        sc = MR.interface_limits(I.h_old, I.tracers[L], I.wt, self.lo, self.hi, self.nc, si, so)
        return float((sc < 1.0).mean()), float((sc == 1.0).mean())

    def check(self, I):
        for L in (STEP, RANDOM):
            over = self.parent_path_excess(I, L)
            assert over > 1.0e-2, (L, over)
        lim, free = self.limited_interfaces(I, RANDOM)
        assert lim >= 0.2 and free >= 0.2, (lim, free)


# any rig takes an order; the names say which form a test means
HoRig, Ho3Rig = MonoRig, Mono3Rig
