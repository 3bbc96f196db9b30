"""Shared by the tests of the 3-D form of MonotoneAdv (CPU: tests/test_monotone_adv_3d.py, GPU:
tests/test_monotone_adv_3d_gpu.py, tests/test_c_abi_monotone_adv_3d.py): MonoRig with ragged layer ranges and the inputs
of one forward step with a vertical transport.

The ranges are drawn per global cell (so every part of a decomposition sees the same): KMin in 0 .. 2, KMax in
K-4 .. K-1, both clipped to 0 <= KMin <= KMax < K, and one column in sixteen is land (MaxLayerCell = -1).
VerticalTransport is uniform in +-amp on the interfaces KMin < K <= KMax and NaN everywhere else -- at KMin, outside the
range, on land and on the sentinel row: nothing may use it there.  amp is the median horizontal outflow rate
(sum of outflow |Fm|)/AreaCell of the mesh, so that the two directions limit each other on every mesh.  Dt puts the
largest combined outflow Courant number Dt*(horizontal outflow + max(Wv[K], 0) + max(-Wv[K+1], 0))/h at 0.4, hNew is the
thickness of the same fluxes, and the step tracer jumps in x and at mid-depth.

The fixture asserts (on request: `check`) that its inputs show the need and exercise the limiter: the parent's path --
the 2-D limiter plus VertAdv's unlimited order-2 vertical flux -- leaves the 3-D neighbourhood range by more than 1e-2
on the step and on the random tracer, and on the random tracer at least 20 % of the interfaces that carry flux are
limited (ScV < 1) and at least 20 % are not."""
import numpy as np

from tests import column_reference as CR
from tests import monotone_adv3d_reference as M3
from tests import monotone_adv_reference as MR
from tests import vert_adv_reference as VR
from tests.monotone_adv_fixtures import COURANT, RANDOM, STEP, MonoRig


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
        self.inside = M3.interface_mask(self.lo, self.hi, self.nc, K)

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
        vdiv, vout = M3.thickness_divergence(I.wt, self.lo, self.hi, nc)
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
        _, _, p_min, p_max = M3.scale_factors(M, I.h_old, I.h_new, I.u, I.tracers[L], I.dt, I.wt, self.lo, self.hi, I.upwind)
        return float(max((new - p_max).max(), (p_min - new).max()))

    def limited_interfaces(self, I, L):
        si, so, _, _ = M3.scale_factors(self.M, I.h_old, I.h_new, I.u, I.tracers[L], I.dt, I.wt, self.lo, self.hi, I.upwind)
        sc = M3.interface_limits(I.h_old, I.tracers[L], I.wt, self.lo, self.hi, self.nc, si, so)
        return float((sc < 1.0).mean()), float((sc == 1.0).mean())

    def check(self, I):
        for L in (STEP, RANDOM):
            over = self.parent_path_excess(I, L)
            assert over > 1.0e-2, (L, over)
        lim, free = self.limited_interfaces(I, RANDOM)
        assert lim >= 0.2 and free >= 0.2, (lim, free)

    def reference(self, I, ntracers, tend0=None, max_tracers=None):
        """(Tend, ScaleIn, ScaleOut) of the 3-D restatement, from tend0 (default zeros) and zero scale arrays"""
        tend = np.zeros((ntracers, self.nc_size, self.K)) if tend0 is None else tend0.copy()
        si = np.zeros((max_tracers or ntracers, self.nc_size, self.K))
        so = np.zeros_like(si)
        M3.add_tracer_tend(self.M, tend, I.h_old, I.h_new, I.u, I.tracers, ntracers, I.dt, I.upwind, si, so, I.wt,
                           self.lo, self.hi)
        return tend, si, so

    def reference_2d(self, I, ntracers, tend0=None, max_tracers=None):
        return MonoRig.reference(self, I, ntracers, tend0, max_tracers)
