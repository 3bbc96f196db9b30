"""The three BarotropicMode calls of a split-explicit step as the NumPy restatement evaluates them
(tests/split_explicit_reference.py; the GPU tests hold the library to the restatement bit for bit): the residual is the
bracket of the first sub-step, a state without 3-D tendency and without flux divergence is held bit for bit, the
transporting velocity carries the sub-cycle's mean flux, and the two level calls write the unsplit values outside the
ranges and nothing beyond the local edges.  Tests of the restatement alone: no device."""
from fractions import Fraction

import numpy as np
import pytest

from tests import barotropic_reference as BR
from tests import split_explicit_reference as SR
from tests.barotropic_fixtures import GRAVITY, HostRig, btr_mesh, closed_basin
from tests.test_barotropic import _split_rig

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def basin():
    return HostRig(closed_basin(12, 14, 30.0e3, 1.0e-4, 1000.0))


def test_residual_is_the_bracket_of_the_first_sub_step(basin):
    """One sub-step with forcing 0 from fields whose flux vanishes (so SSHn = SSH) moves the velocity by DtBtr*R, and
    with DtBtr a power of two the product is exact.  (a) zero velocity, random SSH: the increment itself is DtBtr*R;
    (b) random velocity over water of depth exactly 0 (BottomDepth = -SSH): the Coriolis sum is live as well and the new
    velocity is vel + DtBtr*R, the sub-step's own last rounding."""
    x, dt = basin, 32.0
    rng = np.random.default_rng(12)
    ssh, vel, forcing, flux = x.zeros()
    ssh[: x.nc] = rng.uniform(-0.5, 0.5, x.nc)
    r = SR.residual(x.M, ssh, vel, GRAVITY)
    s, v = ssh.copy(), vel.copy()
    BR.substep(x.M, s, v, forcing, flux, dt, GRAVITY)
    assert np.array_equal(s, ssh) and np.array_equal(v[: x.ne], dt * r)
    assert np.abs(r).max() > 0.0 and np.all(r[x.M.mask[: x.ne] == 0.0] == 0.0)
    # (b)
    M0 = btr_mesh(x.mesh, -ssh)
    vel[: x.ne] = rng.uniform(-0.1, 0.1, x.ne) * (M0.mask[: x.ne] != 0.0)
    assert np.abs(M0.coriolis(vel)).max() > 0.0 and np.all(M0.flux(ssh, vel) == 0.0)
    r = SR.residual(M0, ssh, vel, GRAVITY)
    s, v = ssh.copy(), vel.copy()
    BR.substep(M0, s, v, forcing, np.zeros_like(flux), dt, GRAVITY)
    assert np.array_equal(s, ssh) and np.array_equal(v[: x.ne], vel[: x.ne] + dt * r)
    assert not np.array_equal(r, SR.residual(M0, ssh, np.zeros_like(vel), GRAVITY))  # the Coriolis sum is in R


@pytest.mark.parametrize("f0,uniform", [(0.0, True), (1.0e-4, False)])
def test_a_state_without_tendency_or_flux_divergence_is_held_bit_for_bit(f0, uniform):
    """VelTend = 0 gives G = 0 and BtrForcing = -R; a sub-step then adds DtBtr*(R + (-R)) = 0 to the velocity, and with
    zero flow the flux and its divergence are 0, so SSH stays too.  Uniform SSH without rotation (R = 0), and a random
    SSH with f != 0 and zero flow, which alone would accelerate every open edge."""
    K = 3
    x = HostRig(closed_basin(12, 14, 30.0e3, f0, 1000.0), K)
    rng = np.random.default_rng(5)
    h = np.full((x.nc_size, K), np.nan)
    h[: x.nc] = rng.uniform(200.0, 400.0, (x.nc, K))
    lo_e, hi_e = np.zeros(x.ne_size, np.int32), np.full(x.ne_size, K - 1, np.int32)
    shut = x.M.mask[: x.ne] == 0.0
    lo_e[: x.ne][shut], hi_e[: x.ne][shut] = 1, -1  # a shut edge lacks a cell: its range is empty
    s = SR.Split(x.M, x.nc_size, x.ne_size, K)
    s.ssh[: x.nc] = 0.3 if uniform else rng.uniform(-0.5, 0.5, x.nc)
    SR.compute_residual_forcing(x.M, h, np.zeros((x.ne_size, K)), lo_e, hi_e, s.ssh, s.vel, GRAVITY, s.tend_mean, s.forcing)
    assert np.all(s.tend_mean == 0.0)
    assert np.all(s.forcing == 0.0) if uniform else np.abs(s.forcing).max() > 1.0e-6
    ssh0 = s.ssh.copy()
    BR.subcycle(x.M, s.ssh, s.vel, s.forcing, s.flux, 5, 40.0, GRAVITY)
    assert np.array_equal(s.ssh, ssh0) and np.all(s.vel == 0.0) and np.all(s.flux == 0.0)
    if not uniform:  # and without the residual the same start moves
        v = np.zeros(x.ne_size)
        BR.subcycle(x.M, ssh0.copy(), v, np.zeros(x.ne_size), np.zeros(x.ne_size), 1, 40.0, GRAVITY)
        assert np.abs(v).max() > 0.0


def _exact_column_sums(h_e, u, m):
    out = []
    for e in range(h_e.shape[0]):
        out.append(sum((Fraction(float(a)) * Fraction(float(b)) for a, b in zip(h_e[e][m[e]], u[e][m[e]])), Fraction(0)))
    return out


@pytest.mark.parametrize("K", [1, 3, 17])
def test_transport_velocity_carries_the_mean_flux(K):
    """sum_K hE[K]*uOut[e][K] against BtrFluxMean[e], the sum taken exactly (rationals).  With n = Hi - Lo + 1 levels,
    T = BtrThickEdge, Q = fl(Flux/T), uOut[K] = fl(Bcl[K] + Q):
        sum hE uOut - Flux = sum hE Bcl + Q (sum hE - T) + (Q T - Flux) + sum hE d_K
    The call's own n + 1 roundings are the quotient, |Q T - Flux| <= eps/2 |Flux|, and the n sums d_K, |d_K| <= eps/2
    |Bcl[K] + Q| <= eps/2 (2 U + |Q|) with U = max|u| of the split (|Btr| <= U, |Bcl| <= 2 U).  What the inputs bring:
    T is an ascending sum of n positive terms, |sum hE - T| <= (n - 1) eps/2 T, and sum hE Bcl is the split's residue,
    <= (4 n + 5) eps/2 T U (derived beside the assertion in tests/test_barotropic.py, there for a rounded sum: it covers
    the exact one).  Together
        |sum hE uOut - Flux| <= eps/2 (T ((4 n + 7) U + n |Q|) + |Flux|),
    up to second order in eps (the factor 1 + 1e-6).  Everything on the right comes from the inputs."""
    x, h, u, lo, hi, lo_e, hi_e = _split_rig("fib700_coast_ragged", K)
    coe = x.mesh.get_array("CellsOnEdge")
    m = BR.range_mask(lo_e, hi_e, x.ne, K)
    s = SR.Split(x.M, x.nc_size, x.ne_size, K)
    BR.split_velocity(h, np.nan_to_num(u), coe, lo_e, hi_e, x.ne, s.thick, s.vel, s.bcl)
    rng = np.random.default_rng(3)
    s.ssh[: x.nc] = rng.uniform(-0.5, 0.5, x.nc)
    s.forcing[: x.ne] = rng.uniform(-1.0e-5, 1.0e-5, x.ne)
    s.vel[: x.ne] *= x.M.mask[: x.ne] != 0.0
    BR.subcycle(x.M, s.ssh, s.vel, s.forcing, s.flux, 3, 20.0, GRAVITY)
    u_out = SR.transport_velocity(np.nan_to_num(u), np.full((x.ne_size, K), np.nan), s.bcl, s.flux, s.thick, lo_e, hi_e, x.ne)
    wet = m.any(axis=1)
    h_e = np.zeros((x.ne, K))
    h_e[wet] = 0.5 * (h[coe[: x.ne, 0][wet]] + h[coe[: x.ne, 1][wet]])
    sums = _exact_column_sums(h_e, u_out[: x.ne], m)
    n = m.sum(axis=1)
    umax = np.abs(np.nan_to_num(u)[: x.ne][m]).max()
    with np.errstate(all="ignore"):
        q = np.abs(s.flux[: x.ne] / s.thick[: x.ne])
    worst = 0.0
    for e in np.nonzero(wet)[0]:
        t, fl = s.thick[e], abs(s.flux[e])
        bound = EPS / 2 * (t * ((4 * n[e] + 7) * umax + n[e] * q[e]) + fl) * (1.0 + 1.0e-6)
        err = abs(float(sums[e] - Fraction(float(s.flux[e]))))
        worst = max(worst, err / bound)
        assert err <= bound, (e, err, bound)
    print(f"K {K}: worst |sum hE uOut - BtrFluxMean| / bound = {worst:.3f}")
    assert np.abs(s.flux[: x.ne][wet]).max() > 0.0 and worst > 0.0


def test_the_level_calls_outside_the_ranges():
    """Outside Lo .. Hi (land edges: every level) transportVelocity copies the old velocity and advanceVelocity makes
    the unsplit update; inside, neither reads the old velocity (NaN there); no row >= NEdgesAll is written; uOut may
    be uOld."""
    K, dt = 5, 600.0
    x, h, u, lo, hi, lo_e, hi_e = _split_rig("fib700_coast_ragged", K)
    m = np.zeros((x.ne_size, K), bool)
    m[: x.ne] = BR.range_mask(lo_e, hi_e, x.ne, K)
    rng = np.random.default_rng(8)
    out_rows = np.zeros((x.ne_size, K), bool)
    out_rows[: x.ne] = ~m[: x.ne]
    assert out_rows.any() and (~m[: x.ne]).all(axis=1).any() and (lo_e[: x.ne][m[: x.ne].any(axis=1)] > 0).any()
    u_old = np.where(out_rows, rng.uniform(-0.1, 0.1, (x.ne_size, K)), np.nan)  # NaN inside the ranges and beyond NEdgesAll
    tend = rng.uniform(-1.0e-5, 1.0e-5, (x.ne_size, K))
    tend[x.ne:] = np.nan
    bcl = np.where(m, rng.uniform(-0.05, 0.05, (x.ne_size, K)), np.nan)
    btr, flux, mean = (rng.uniform(-0.1, 0.1, x.ne_size) for _ in range(3))
    thick = rng.uniform(100.0, 400.0, x.ne_size)
    got = SR.transport_velocity(u_old, np.full((x.ne_size, K), np.nan), bcl, flux, thick, lo_e, hi_e, x.ne)
    assert np.isnan(got[x.ne:]).all() and np.isfinite(got[: x.ne]).all()
    assert np.array_equal(got[out_rows], u_old[out_rows])
    assert np.array_equal(got[m], (bcl + (flux / thick)[:, None])[m])
    got = SR.advance_velocity(u_old, tend, dt, np.full((x.ne_size, K), np.nan), bcl, btr, mean, lo_e, hi_e, x.ne)
    assert np.isnan(got[x.ne:]).all() and np.isfinite(got[: x.ne]).all()
    assert np.array_equal(got[out_rows], (u_old + dt * tend)[out_rows])
    assert np.array_equal(got[m], ((bcl + dt * (tend - mean[:, None])) + btr[:, None])[m])
    alias = u_old.copy()
    assert SR.advance_velocity(alias, tend, dt, alias, bcl, btr, mean, lo_e, hi_e, x.ne) is alias
    assert np.array_equal(alias, got, equal_nan=True)
