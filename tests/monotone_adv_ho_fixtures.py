"""Shared by the tests of the high-order horizontal flux of MonotoneAdv (CPU: tests/test_monotone_adv_high_order.py,
GPU: tests/test_monotone_adv_high_order_gpu.py, tests/test_c_abi_monotone_adv_high_order.py): the rigs of
tests/monotone_adv_fixtures.py and tests/monotone_adv3d_fixtures.py with the library's tables for one order, and the
same inputs.

The fixture asserts that its inputs exercise the limiter with the high-order flux as well: on the random tracer at least
20 % of the masked-in edge-levels are limited (Sc < 1) and at least 20 % are not; the constant tracer has no limited
edge-level; and on fib700_coast_ragged at least 5 % of the edges are high and at least 5 % of the masked-in edges are
not, so that both branches of the correction's select are compared."""
import numpy as np

from tests import monotone_adv_ho_reference as HO
from tests.monotone_adv3d_fixtures import Mono3Rig
from tests.monotone_adv_fixtures import CONST, RANDOM, MonoRig

ORDERS = ((4, 0.25), (3, 0.25))  # (order, Coef3rdOrder): beta = 0.0 and beta = 0.25


class _HighOrder:
    """mixin: `H` the tables of (order, coef) on the rig's mesh; `vert(I)` the 3-D form's extra inputs or None"""

    def set_order(self, order, coef=0.25):
        self.order, self.coef = order, coef
        self.H = HO.HoTables.of(self.M, self.mesh, self.g, order, coef)
        return self

    def vert(self, I):
        return (I.wt, I.lo, I.hi) if hasattr(I, "wt") else None

    def hess(self, I, L):
        return HO.hessians(self.H, I.tracers[L])

    def limited_fraction_ho(self, I, L):
        hs = self.hess(I, L)
        si, so, _, _ = HO.scale_factors(self.H, I.h_old, I.h_new, I.u, I.tracers[L], hs, I.dt, I.upwind)
        sc = HO.edge_limits(self.H, I.h_old, I.u, I.tracers[L], hs, si, so, I.upwind)
        return float((sc < 1.0).mean()), float((sc == 1.0).mean())

    def check_ho(self, I):
        lim, free = self.limited_fraction_ho(I, RANDOM)
        assert lim >= 0.2 and free >= 0.2, (lim, free)
        assert self.limited_fraction_ho(I, CONST) == (0.0, 1.0)
        if not self.M.open_edge.all():  # a coast
            high, open_ = self.H.high, self.M.open_edge
            assert high.mean() >= 0.05 and (open_ & ~high).sum() >= 0.05 * open_.sum(), (high.mean(), open_.mean())
        return lim, free

    def reference_ho(self, I, ntracers, tend0=None, max_tracers=None):
        """(Tend, ScaleIn, ScaleOut, Hess) of the restatement, from tend0 (default zeros), zero scale arrays and NaN in
        Hess"""
        tend = np.zeros((ntracers, self.nc_size, self.K)) if tend0 is None else tend0.copy()
        si = np.zeros((max_tracers or ntracers, self.nc_size, self.K))
        so = np.zeros_like(si)
        hess = np.full((max_tracers or ntracers, 3, self.nc_size, self.K), np.nan)
        HO.add_tracer_tend(self.H, tend, I.h_old, I.h_new, I.u, I.tracers, ntracers, I.dt, I.upwind, si, so, hess,
                           self.vert(I))
        return tend, si, so, hess


class HoRig(_HighOrder, MonoRig):
    pass


class Ho3Rig(_HighOrder, Mono3Rig):
    pass
