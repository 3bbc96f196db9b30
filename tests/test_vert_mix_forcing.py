"""The forced implicit solves without a device: the NumPy restatement (tests/vert_mix_forcing_reference.py) against
what must hold of it independently -- zero forcing is the unforced solve, the tracer and momentum budgets of a column
close, Rayleigh drag alone is a division, and a large bottom drag keeps the sign of the bottom velocity."""
import numpy as np
import pytest

from tests import vert_mix_forcing_reference as F
from tests import vert_mix_reference as R
from tests.column_reference import RHO0

EPS = np.finfo(np.float64).eps
DT = 1800.0


class Columns:
    """nc cells in a ring, edge e between cells e and e+1 (mod nc), K levels; ragged cell ranges (land, one level, full
    depth); the edge ranges are the levels active in both cells."""

    def __init__(self, nc=24, K=12, seed=3):
        rng = np.random.default_rng(seed)
        self.nc, self.K = nc, K
        self.lo = rng.integers(0, 3, nc).astype(np.int32)
        self.hi = np.minimum(K - 1, self.lo + rng.integers(0, K, nc)).astype(np.int32)
        self.hi[::7] = -1                      # land
        self.hi[1::7] = self.lo[1::7]          # one level
        self.lo[2::7], self.hi[2::7] = 0, K - 1  # full depth
        self.h = rng.uniform(0.5, 40.0, (nc, K))
        self.diff = rng.uniform(1.0e-5, 1.0e-2, (nc, K))
        self.visc = rng.uniform(1.0e-4, 1.0e-1, (nc, K))
        self.tr = rng.uniform(-2.0, 30.0, (3, nc, K))
        self.flux = rng.uniform(-1.0e-4, 1.0e-4, (3, nc))
        self.coe = np.stack([np.arange(nc), (np.arange(nc) + 1) % nc], axis=1).astype(np.int32)
        c1, c2 = self.coe[:, 0], self.coe[:, 1]
        land = (self.hi[c1] < 0) | (self.hi[c2] < 0)
        self.elo = np.where(land, K + 1, np.maximum(self.lo[c1], self.lo[c2])).astype(np.int32)
        self.ehi = np.where(land, 0, np.minimum(self.hi[c1], self.hi[c2])).astype(np.int32)
        self.u = rng.uniform(-0.5, 0.5, (nc, K))
        self.ut = rng.uniform(-0.5, 0.5, (nc, K))
        self.stress = rng.uniform(-0.2, 0.2, nc)
        self.mask = np.where(np.arange(nc) % 5 == 0, 0.0, 1.0)

    def edges(self):
        """(e, lo, hi) of the edges with a non-empty range"""
        return [(e, int(self.elo[e]), int(self.ehi[e])) for e in range(self.nc)
                if 0 <= self.elo[e] <= self.ehi[e] < self.K]

    def he(self, e):
        return 0.5 * (self.h[self.coe[e, 0]] + self.h[self.coe[e, 1]])


def test_zero_forcing_is_the_unforced_solve_bit_for_bit():
    x = Columns()
    want_u = R.velocity_mix(x.h, x.visc, x.u, DT, x.coe, x.elo, x.ehi, x.nc)
    zero = np.zeros(x.nc)
    for kw in (dict(), dict(cd=0.0, ra=0.0, ut=x.ut), dict(stress=zero, edge_mask=x.mask),
               dict(stress=x.stress, edge_mask=zero)):
        got = F.velocity_mix_forced(x.h, x.visc, x.u, DT, x.coe, x.elo, x.ehi, x.nc, rho0=RHO0, **kw)
        assert np.array_equal(got, want_u), kw.keys()
    want_t = R.tracer_mix(x.h, x.diff, x.tr, 3, DT, x.lo, x.hi, x.nc)
    assert np.array_equal(F.tracer_mix_forced(x.h, x.diff, x.tr, 3, DT, x.lo, x.hi, x.nc), want_t)
    assert np.array_equal(F.tracer_mix_forced(x.h, x.diff, x.tr, 3, DT, x.lo, x.hi, x.nc, np.zeros((3, x.nc))), want_t)
    assert len(x.edges()) < x.nc and any(lo == hi for _, lo, hi in x.edges())  # empty and one-level edge ranges


def test_tracer_budget_changes_by_dt_times_flux():
    x = Columns()
    got = F.tracer_mix_forced(x.h, x.diff, x.tr, 3, DT, x.lo, x.hi, x.nc, x.flux)
    checked = 0
    for c in range(x.nc):
        lo, hi = x.lo[c], x.hi[c]
        if hi < lo:
            assert np.array_equal(got[:, c], x.tr[:, c])
            continue
        n, s = hi - lo + 1, slice(lo, hi + 1)
        for t in range(3):
            before, after = x.h[c, s] * x.tr[t, c, s], x.h[c, s] * got[t, c, s]
            # a sum of n rounded products and the solve's rounding
            tol = 4 * n * EPS * max(np.abs(before).max(), np.abs(after).max())
            assert abs((after.sum() - before.sum()) - DT * x.flux[t, c]) <= tol, (c, t)
            checked += 1
        assert np.array_equal(got[:, c, :lo], x.tr[:, c, :lo]) and np.array_equal(got[:, c, hi + 1:], x.tr[:, c, hi + 1:])
    assert checked > 30


@pytest.mark.parametrize("cd,ra,wind", [(2.5e-3, 0.0, False), (0.0, 1.0e-5, False), (0.0, 0.0, True),
                                        (2.5e-3, 1.0e-5, True)])
def test_momentum_budget(cd, ra, wind):
    x = Columns()
    got = F.velocity_mix_forced(x.h, x.visc, x.u, DT, x.coe, x.elo, x.ehi, x.nc, cd=cd, ra=ra,
                                stress=x.stress if wind else None, ut=x.ut, edge_mask=x.mask, rho0=RHO0)
    active = {e for e, _, _ in x.edges()}
    for e in range(x.nc):
        if e not in active:
            assert np.array_equal(got[e], x.u[e])  # whatever its stress
    for e, lo, hi in x.edges():
        n, s = hi - lo + 1, slice(lo, hi + 1)
        he = x.he(e)[s]
        before, after = he * x.u[e, s], he * got[e, s]
        speed = np.sqrt(x.u[e, hi] ** 2 + x.ut[e, hi] ** 2)
        terms = [DT * x.mask[e] * x.stress[e] / RHO0 if wind else 0.0, -DT * cd * speed * got[e, hi],
                 -DT * ra * after.sum()]
        scale = max(np.abs(before).max(), np.abs(after).max(), max(abs(t) for t in terms))
        assert abs((after.sum() - before.sum()) - sum(terms)) <= 4 * n * EPS * scale, e
        assert np.array_equal(got[e, :lo], x.u[e, :lo]) and np.array_equal(got[e, hi + 1:], x.u[e, hi + 1:])


def test_rayleigh_alone_without_viscosity_is_a_division():
    x = Columns()
    ra = 3.0e-5
    got = F.velocity_mix_forced(x.h, np.zeros_like(x.visc), x.u, DT, x.coe, x.elo, x.ehi, x.nc, ra=ra)
    for e, lo, hi in x.edges():
        want = x.u[e, lo: hi + 1] / (1.0 + DT * ra)
        assert np.all(np.abs(got[e, lo: hi + 1] - want) <= 2 * np.spacing(np.abs(want))), e


@pytest.mark.parametrize("n", [1, 2, 5])
def test_large_bottom_drag_keeps_the_sign_and_shrinks_monotonically(n):
    rng = np.random.default_rng(11)
    ne = 16
    he = rng.uniform(0.5, 40.0, (ne, n))
    nue = rng.uniform(1.0e-4, 1.0e-2, (ne, n))
    u = rng.uniform(0.05, 0.5, (ne, n)) * np.where(np.arange(ne) % 2 == 0, 1.0, -1.0)[:, None]
    utb = rng.uniform(-0.5, 0.5, ne)
    speed = np.sqrt(u[:, -1] ** 2 + utb ** 2)
    prev = np.abs(u[:, -1]) if n == 1 else None  # n > 1: mixing alone may move the bottom value either way
    for ratio in 10.0 ** np.arange(0, 7):
        ub = np.empty(ne)
        for e in range(ne):
            c = ratio * he[e, -1] / (DT * speed[e])  # dt*Cd*Speed/hE = ratio for this edge
            g, d, xx = F.velocity_system(he[e: e + 1], nue[e: e + 1], u[e: e + 1], utb[e: e + 1], DT, c, 0.0, None,
                                         None, RHO0)
            ub[e] = F.pcr_diff(g, d, xx)[0, -1]
        assert np.all(np.sign(ub) == np.sign(u[:, -1])), ratio
        if prev is not None:
            assert np.all(np.abs(ub) < prev), ratio
        prev = np.abs(ub)
