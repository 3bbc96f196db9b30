"""The BarotropicMode contract as the NumPy restatement evaluates it (tests/barotropic_reference.py; the GPU tests hold
the library to the restatement bit for bit): what the split and the forward-backward sub-cycling must do as numerics --
rest stays at rest, volume is kept, the mean flux explains the change of SSH, split and recombine invert each other, a
standing gravity wave has the period of the forward-backward dispersion relation (second order in DtBtr, tending to
2L/sqrt(gH)), a uniform flow turns clockwise for f > 0, and nothing outside the stated entries is written.  These are
tests of the restatement alone; of this file only test_the_binding_exists needs the class in the library (the GPU and
C ABI tests are the ones that hold the library itself to the contract)."""
import numpy as np
import pytest

import omega_amd as oa
from tests import barotropic_reference as BR
from tests import column_reference as CR
from tests.barotropic_fixtures import GRAVITY, HostRig, closed_basin
from tests.meshes import named_mesh
from tests.vert_fixtures import mix_inputs

EPS = np.finfo(np.float64).eps


def test_the_binding_exists():
    assert hasattr(oa, "BarotropicMode") and oa.BarotropicMode.max_layers() >= 1024


@pytest.fixture(scope="module")
def basin():
    return HostRig(closed_basin(12, 14, 30.0e3, 1.0e-4, 1000.0))


@pytest.mark.parametrize("nsub", [1, 2, 7])
def test_rest_stays_at_rest(basin, nsub):
    ssh, vel, forcing, flux = basin.zeros()
    BR.subcycle(basin.M, ssh, vel, forcing, flux, nsub, 40.0)
    assert np.all(ssh == 0.0) and np.all(vel == 0.0) and np.all(flux == 0.0)


def _random_start(x, seed=3, amp=0.5, speed=0.1):
    rng = np.random.default_rng(seed)
    ssh, vel, forcing, flux = x.zeros()
    ssh[: x.nc] = rng.uniform(-amp, amp, x.nc)
    vel[: x.ne] = rng.uniform(-speed, speed, x.ne) * (x.M.mask[: x.ne] != 0.0)
    forcing[: x.ne] = rng.uniform(-1.0e-5, 1.0e-5, x.ne)
    return ssh, vel, forcing, flux


def test_volume_changes_by_rounding_only(basin):
    """Every edge of the closed basin is either shut (F = 0) or adds (Dv F)/A0 to one cell and subtracts (Dv F)/A1
    from the other, so sum(A * SSH) changes by rounding alone.  Per sub-step and cell the NE = 6 terms
    ((Dv F)*InvA, each rounded twice, the running sum, the product with DtBtr and the final subtraction) carry at most
    (3 NE + 2) eps/2 of max|Dt Dv F / A| =: T, and A*SSH itself rounds by eps/2 A |SSH|; the sum over NC cells of the
    products, taken here with math.fsum, adds nothing.  So |dV| <= NSub NC Amax ((3 NE + 2) T + max|SSH|) eps/2 ... a
    bound in terms of the inputs, not of the result."""
    import math
    x, nsub, dt = basin, 7, 40.0
    ssh, vel, forcing, flux = _random_start(x)
    v0 = math.fsum(x.area[: x.nc] * ssh[: x.nc])
    depth = x.bottom[: x.nc].max() + 1.0
    speed = 0.1 + nsub * dt * (1.0e-5 + GRAVITY * 2.0 / 30.0e3 + 1.0e-4 * 0.2)  # |u| can grow by Dt(|forcing|+g grad+f u)
    term = dt * x.M.dv.max() * depth * speed / x.area[: x.nc].min()
    BR.subcycle(x.M, ssh, vel, forcing, flux, nsub, dt)
    v1 = math.fsum(x.area[: x.nc] * ssh[: x.nc])
    bound = nsub * x.nc * x.area[: x.nc].max() * ((3 * 6 + 2) * term + 1.0) * EPS / 2
    print(f"volume change {abs(v1 - v0):.3e} m^3 of {x.area[: x.nc].sum():.3e} m^2 x O(1 m); bound {bound:.3e}")
    assert abs(v1 - v0) <= bound
    assert np.abs(ssh[: x.nc]).max() > 0.0 and abs(v0) > 1.0e3 * bound  # a volume the bound is small against


@pytest.mark.parametrize("nsub", [1, 5])
def test_flux_mean_identity(basin, nsub):
    """SSH_end - SSH_0 = -(NSub DtBtr) Div(BtrFluxMean).  Exactly, SSH_end - SSH_0 = -DtBtr sum_s Div(F_s); Div is
    linear, so the two sides differ by rounding only: (a) each sub-step rounds SSH - Dt*Div once: eps/2 max|SSH| per
    sub-step; (b) each Div(F_s) carries (3 NE + 1) eps/2 D, D = max over cells of sum_j |Dv F/A|, and so does
    Div(mean), where the mean itself carries (NSub + 1) eps/2 relative (NSub additions, one division); (c) the product
    with NSub*DtBtr two more eps/2.  With S = NSub Dt D:  |lhs - rhs| <= eps/2 (NSub max|SSH| + S ((3 NE + 1) 2 +
    NSub + 1 + 2)), everything taken from the inputs and the fluxes, nothing from the difference under test."""
    x, dt = basin, 40.0
    ssh, vel, forcing, flux = _random_start(x, seed=5)
    ssh0 = ssh.copy()
    per_cell = []
    s_, v_, f_ = ssh.copy(), vel.copy(), np.zeros_like(flux)
    for _ in range(nsub):  # the magnitude of the terms, from a run of the sub-steps one by one
        f = x.M.flux(s_, v_)
        mag = np.zeros(x.nc)
        for j in range(x.M.eoc.shape[1]):
            r = np.nonzero(j < x.M.neoc[: x.nc])[0]
            mag[r] += np.abs(x.M.dv[x.M.eoc[r, j]] * f[x.M.eoc[r, j]]) * x.M.inv_area[r]
        per_cell.append(mag.max())
        BR.substep(x.M, s_, v_, forcing, f_, dt, GRAVITY)
    BR.subcycle(x.M, ssh, vel, forcing, flux, nsub, dt)
    assert np.array_equal(ssh, s_) and np.array_equal(vel, v_)
    lhs = ssh[: x.nc] - ssh0[: x.nc]
    rhs = -(nsub * dt) * x.M.divergence(flux[: x.ne])
    S = nsub * dt * max(per_cell)
    ssh_max = max(np.abs(ssh0).max(), np.abs(ssh).max()) + S
    bound = EPS / 2 * (nsub * ssh_max + S * ((3 * 6 + 1) * 2 + nsub + 3))
    err = np.abs(lhs - rhs).max()
    print(f"NSub {nsub}: max |dSSH + T Div(mean F)| = {err:.3e}, bound {bound:.3e}, max |dSSH| = {np.abs(lhs).max():.3e}")
    assert err <= bound
    assert np.abs(lhs).max() > 1.0e6 * bound


def _split_rig(mesh_name, K, seed=7):
    g = named_mesh(mesh_name)
    x = HostRig(g, K)
    G = mix_inputs(g, K, seed, False, 2)
    cid = x.decomp.get_array("CellID")
    eid = x.decomp.get_array("EdgeID")
    lo, hi = CR.local_layer_ranges(cid, G["min_level"], G["max_level"], x.nc, x.nc_size, K)
    _, lo_e, hi_e, _ = CR.min_max_layer(x.mesh.get_array("CellsOnEdge"), x.ne, lo, hi, K)
    h, u = np.full((x.nc_size, K), np.nan), np.full((x.ne_size, K), np.nan)
    h[: x.nc], u[: x.ne] = G["h"][cid[: x.nc] - 1], G["un"][eid[: x.ne] - 1]
    return x, h, u, lo, hi, lo_e, hi_e


@pytest.mark.parametrize("K", [1, 3, 17])
def test_split_and_recombine(K):
    x, h, u, lo, hi, lo_e, hi_e = _split_rig("fib700_coast_ragged", K)
    coe = x.mesh.get_array("CellsOnEdge")
    m = np.zeros((x.ne_size, K), bool)
    m[: x.ne] = BR.range_mask(lo_e, hi_e, x.ne, K)
    u = np.where(m, u, np.nan)  # NaN outside the ranges: never read
    thick, btr, bcl = np.full(x.ne_size, np.nan), np.full(x.ne_size, np.nan), np.full((x.ne_size, K), np.nan)
    BR.split_velocity(h, u, coe, lo_e, hi_e, x.ne, thick, btr, bcl)
    # masking: every edge < NEdgesAll gets its two scalars (0 on an empty range), nothing else is written
    assert np.isfinite(thick[: x.ne]).all() and np.isnan(thick[x.ne:]).all() and np.isnan(btr[x.ne:]).all()
    empty = ~m[: x.ne].any(axis=1)
    assert empty.any() and np.all(thick[: x.ne][empty] == 0.0) and np.all(btr[: x.ne][empty] == 0.0)
    assert np.array_equal(np.isfinite(bcl), m)
    if K > 2:
        assert (lo_e[: x.ne][~empty] > 0).any()
    # sum_K hE*Bcl is rounding residue.  Bcl = u - Btr rounds by eps/2 max(|u|,|Btr|) <= eps/2 U, the product with hE
    # once more, the n-term sum n eps/2 of sum hE |Bcl| <= 2 Thick U; and Btr itself is the quotient of two n-term sums,
    # (2n + 2) eps/2 relative, which moves the exact sum by Thick*|Btr| times that.  Together <= (4n + 5) eps/2 Thick U
    # with n <= K levels and U = max|u| (|Btr| <= U up to rounding, a weighted mean).
    umax = np.nanmax(np.abs(u))
    c0, c1 = coe[: x.ne, 0], coe[: x.ne, 1]
    safe = ~empty
    h_e = np.zeros((x.ne, K))
    h_e[safe] = 0.5 * (h[c0[safe]] + h[c1[safe]])
    resid = np.abs(np.where(m[: x.ne], h_e * np.nan_to_num(bcl[: x.ne]), 0.0).sum(axis=1))
    bound = (4 * K + 5) * EPS / 2 * thick[: x.ne] * umax * (1 + K * EPS)
    print(f"K {K}: max residue / (Thick max|u|) = {np.max(resid[safe] / (thick[: x.ne][safe] * umax)):.3e}, "
          f"bound {(4 * K + 5) * EPS / 2:.3e}")
    assert np.all(resid <= bound)
    # recombine(split(u)) == u to 1 ulp of m = max(|u|, |Btr|), g = ulp(m), m in [2^E, 2^(E+1)).  d = fl(u - b) errs by
    # e1 <= ulp(d)/2, and x = d + b = u + e1 exactly.  (A) |u - b| < 2^(E+1): e1 <= g/2, and the float nearest to x is no
    # further from x than the float u is: |fl(x) - u| <= 2 e1 <= g.  (B) |u - b| >= 2^(E+1) (opposite signs): d is a
    # multiple of 2g and e1 <= g.  If b is in m's binade, b and hence x are multiples of g below 2^(E+1): x is a float
    # and the error is e1 <= g.  Otherwise u is (u > 2^E, on the grid g) and x = u + e1 lies in [2^E, 2^(E+1)], so fl(x)
    # is on the grid g too: |fl(x) - u| <= e1 + g/2 is a multiple of g, hence <= g.
    back = recombine_into(np.full((x.ne_size, K), np.nan), btr, bcl, lo_e, hi_e, x.ne)
    assert np.array_equal(np.isfinite(back), m)
    scale = np.maximum(np.abs(u[: x.ne]), np.abs(btr[: x.ne])[:, None])
    ok = np.abs(back[: x.ne] - u[: x.ne]) <= np.spacing(scale)
    assert np.all(ok[m[: x.ne]])
    # a range of one level (every range at K = 1): BtrVelocity is that level's u bit for bit, BclVelocity zero
    single = safe & (lo_e[: x.ne] == hi_e[: x.ne])
    assert single.any() and (K > 1 or single.sum() == safe.sum())
    at = np.clip(lo_e[: x.ne], 0, K - 1)
    assert np.array_equal(btr[: x.ne][single], u[np.arange(x.ne), at][single])
    assert np.all(bcl[np.arange(x.ne), at][single] == 0.0)
    # a depth-independent u gives it back
    u_flat = np.where(m, np.repeat(np.nan_to_num(u[:, :1]) + 0.01, K, axis=1), np.nan)
    BR.split_velocity(h, u_flat, coe, lo_e, hi_e, x.ne, thick, btr, bcl)
    first = u_flat[np.arange(x.ne), np.clip(lo_e[: x.ne], 0, K - 1)]
    assert np.all(np.abs(btr[: x.ne][safe] - first[safe]) <= (2 * K + 2) * EPS / 2 * np.abs(first[safe]) * (1 + 1e-6))
    assert np.nanmax(np.abs(bcl)) <= (2 * K + 3) * EPS / 2 * np.nanmax(np.abs(u_flat)) * (1 + 1e-6)


def recombine_into(u, btr, bcl, lo_e, hi_e, n):
    return BR.recombine(u, btr, bcl, lo_e, hi_e, n)


def test_one_level_barotropic_velocity_is_u_bit_for_bit():
    """K = 1, random thickness: BtrVelocity is u bit for bit (the quotient (hE*u)/hE would miss it on some edges, which
    is why the contract takes the level's own value on a range of one level), BclVelocity zero, and the same of
    BtrForcing"""
    x, h, u, lo, hi, lo_e, hi_e = _split_rig("hex24x20", 1)
    coe = x.mesh.get_array("CellsOnEdge")
    h_e = 0.5 * (h[coe[: x.ne, 0], 0] + h[coe[: x.ne, 1], 0])
    assert ((h_e * u[: x.ne, 0]) / h_e != u[: x.ne, 0]).any()  # the inputs can tell the two apart
    thick, btr, bcl = np.zeros(x.ne_size), np.zeros(x.ne_size), np.zeros((x.ne_size, 1))
    BR.split_velocity(h, u, coe, lo_e, hi_e, x.ne, thick, btr, bcl)
    act = BR.range_mask(lo_e, hi_e, x.ne, 1)[:, 0]
    assert act.any() and np.array_equal(btr[: x.ne][act], u[: x.ne, 0][act]) and np.all(bcl[: x.ne][act] == 0.0)
    f = BR.compute_forcing(h, u, coe, lo_e, hi_e, x.ne, np.zeros(x.ne_size))
    assert np.array_equal(f[: x.ne][act], u[: x.ne, 0][act]) and np.all(f[: x.ne][~act] == 0.0)


def test_ssh_and_forcing_masking():
    x, h, u, lo, hi, lo_e, hi_e = _split_rig("fib700_coast_ragged", 5)
    rng = np.random.default_rng(2)
    bottom = np.concatenate([rng.uniform(10.0, 100.0, x.nc), [np.nan]])
    ssh = BR.compute_ssh(h, bottom, lo, hi, x.nc, np.full(x.nc_size, np.nan))
    wet = (lo[: x.nc] >= 0) & (lo[: x.nc] <= hi[: x.nc])
    assert (~wet).any() and np.array_equal(np.isfinite(ssh[: x.nc]), wet) and np.isnan(ssh[x.nc])
    c = np.nonzero(wet)[0][0]
    assert ssh[c] == np.cumsum(np.concatenate([[0.0], h[c, lo[c]: hi[c] + 1]]))[-1] - bottom[c]
    f = BR.compute_forcing(h, np.nan_to_num(u), x.mesh.get_array("CellsOnEdge"), lo_e, hi_e, x.ne, np.full(x.ne_size, np.nan))
    assert np.isfinite(f[: x.ne]).all() and np.isnan(f[x.ne:]).all()


def test_boundary_edges_keep_their_velocity_and_read_nothing(basin):
    """NaN beyond the local elements (the sentinel rows a shut edge's missing cell points at): nothing of it is read;
    shut edges keep BtrVelocity = 0 whatever the forcing"""
    x = basin
    ssh, vel, forcing, flux = _random_start(x, seed=9)
    forcing[: x.ne] = 1.0e-4
    for a, n in ((ssh, x.nc), (vel, x.ne), (forcing, x.ne), (flux, x.ne)):
        a[n:] = np.nan
    shut = x.M.mask[: x.ne] == 0.0
    assert shut.any() and np.all(vel[: x.ne][shut] == 0.0)
    BR.subcycle(x.M, ssh, vel, forcing, flux, 3, 40.0)
    assert np.all(vel[: x.ne][shut] == 0.0) and np.all(flux[: x.ne][shut] == 0.0)
    assert np.isfinite(ssh[: x.nc]).all() and np.isfinite(vel[: x.ne]).all() and np.isfinite(flux[: x.ne]).all()
    assert np.isnan(ssh[x.nc:]).all() and np.isnan(vel[x.ne:]).all() and np.isnan(flux[x.ne:]).all()


# ---------------------------------------------------------------------------------------------------------------------
WAVE = dict(nx=4, ny=34, dc=30.0e3, depth=1000.0, amp=1.0e-3)


def _wave_period(x, dt, nsteps=8):
    """The period of the gravest standing mode along y, from three consecutive samples of its amplitude: the
    forward-backward scheme is linear in the limit of small amplitude and the start is an eigenvector of the discrete
    operator, so the amplitude obeys A[n+1] - 2 A[n] + A[n-1] = -(w dt)^2 A[n] and cos(theta) = (A[n+1] + A[n-1]) /
    (2 A[n]) gives the phase step theta = 2 pi dt / T with no fitting and no interpolation"""
    g = x.g
    L, y0 = g["basin_L"], g["basin_y0"]
    shape = np.cos(np.pi * (x.y_cell[: x.nc] - y0) / L)
    ssh, vel, forcing, flux = x.zeros()
    ssh[: x.nc] = WAVE["amp"] * shape
    amp = [float(shape @ ssh[: x.nc])]
    for _ in range(nsteps):
        BR.subcycle(x.M, ssh, vel, forcing, flux, 1, dt)
        amp.append(float(shape @ ssh[: x.nc]))
    thetas = [np.arccos((amp[n + 1] + amp[n - 1]) / (2.0 * amp[n])) for n in range(2, nsteps)]
    return 2.0 * np.pi * dt / float(np.mean(thetas))


def test_standing_gravity_wave_period_converges_at_second_order():
    """Flat bottom, f = 0, a channel closed across y.  With rows dy apart the discrete operator along y is the 1-D
    second difference, whose gravest Neumann mode cos(pi (y - y0)/L) has w_h = (2 c/dy) sin(k dy/2), k = pi/L,
    c = sqrt(g H); forward-backward stepping gives sin(w dt/2) = w_h dt/2, so T(dt) = T_h (x/2)/asin(x/2), x = w_h dt:
    T_h - T(dt) = T_h (x^2/24 + O(x^4)), second order, and T_h -> 2L/c like (k dy)^2/24.  Asserted: the observed
    order from dt, dt/2, dt/4 against T_h.  The ratio of successive errors is 4 (1 + c2 x^2) with |c2| < 0.1 (next
    term of the series), |order - 2| <= log2(1.025) = 0.036 at x <= 0.5; the amplitude/depth = 1e-6 nonlinearity
    against the smallest relative error x^2/24 = 6.5e-4 (x = 0.125) moves a ratio by < 0.4 %, the order by < 0.006:
    |order - 2| <= 0.05."""
    x = HostRig(closed_basin(WAVE["nx"], WAVE["ny"], WAVE["dc"], 0.0, WAVE["depth"], walls="y"))
    g = x.g
    L, dy = g["basin_L"], g["basin_dy"]
    c = np.sqrt(GRAVITY * WAVE["depth"])
    k = np.pi / L
    w_h = 2.0 * c / dy * np.sin(0.5 * k * dy)
    t_h, t_a = 2.0 * np.pi / w_h, 2.0 * L / c
    dts = [0.5 / w_h, 0.25 / w_h, 0.125 / w_h]
    periods = [_wave_period(x, dt) for dt in dts]
    errs = [t_h - t for t in periods]
    orders = [np.log2(errs[i] / errs[i + 1]) for i in range(2)]
    for dt, t, e in zip(dts, periods, errs):
        print(f"DtBtr {dt:8.2f} s: period {t:.4f} s, (T_h - T)/T_h = {e / t_h:.4e}, (T - 2L/c)/(2L/c) = {(t - t_a) / t_a:+.4e}")
    print(f"T_h = {t_h:.4f} s, 2L/sqrt(gH) = {t_a:.4f} s, (T_h - T_a)/T_a = {(t_h - t_a) / t_a:.4e}; orders {orders}")
    assert all(e > 0.0 for e in errs)
    assert all(abs(p - 2.0) <= 0.05 for p in orders)
    # and against the analytic period: what is left at the smallest dt is the two series' leading terms
    xs = w_h * dts[-1]
    assert abs(periods[-1] - t_a) / t_a <= 1.1 * ((k * dy) ** 2 + xs ** 2) / 24.0


def test_inertial_rotation_is_clockwise_and_no_faster_than_forward_euler():
    """Uniform flow (U, 0), flat SSH, f > 0: away from the walls the divergence is zero and the sub-step is forward
    Euler of dU/dt = -f k x U: the vector turns clockwise (V < 0 growing from U > 0) and |U| grows by exactly
    sqrt(1 + (f dt)^2) per sub-step where the tangential reconstruction is exact (regular hexagons); a few eps for the
    12-term sums."""
    f0, dt, nsub = 1.0e-4, 100.0, 3
    x = HostRig(closed_basin(32, 32, 30.0e3, f0, 1000.0))
    ssh, vel, forcing, flux = x.zeros()
    u0 = 0.1
    vel[: x.ne] = u0 * np.cos(x.angle[: x.ne]) * (x.M.mask[: x.ne] != 0.0)
    # interior: what the walls disturb travels at most 2.5 cells per sub-step (the new SSH of a cell moves its edges in
    # the same sub-step, and the Coriolis stencil of an edge spans the two cells next to it)
    xe, ye = x.x_edge[: x.ne], x.y_edge[: x.ne]
    far = (2.5 * nsub + 2.0) * 30.0e3
    inner = (xe > xe.min() + far) & (xe < xe.max() - far) & (ye > ye.min() + far) & (ye < ye.max() - far)
    assert inner.sum() >= 12
    basis = np.stack([np.cos(x.angle[: x.ne][inner]), np.sin(x.angle[: x.ne][inner])], axis=1)

    def vector():
        sol, res, _, _ = np.linalg.lstsq(basis, vel[: x.ne][inner], rcond=None)
        assert np.abs(basis @ sol - vel[: x.ne][inner]).max() <= 1.0e-12 * u0  # still a uniform flow there
        return sol

    prev = vector()
    assert abs(prev[0] - u0) <= 1.0e-15 and abs(prev[1]) <= 1.0e-15
    for s in range(nsub):
        BR.subcycle(x.M, ssh, vel, forcing, flux, 1, dt)
        cur = vector()
        turn = np.arctan2(cur[1], cur[0]) - np.arctan2(prev[1], prev[0])
        growth = np.hypot(*cur) / np.hypot(*prev)
        print(f"sub-step {s + 1}: (U, V) = ({cur[0]:+.6e}, {cur[1]:+.6e}), turned {turn:+.6e} rad, growth - 1 = {growth - 1:.6e}")
        assert turn < 0.0 and abs(turn + np.arctan(f0 * dt)) <= 1.0e-9  # clockwise, by atan(f dt)
        assert growth <= np.sqrt(1.0 + (f0 * dt) ** 2) * (1.0 + 64 * EPS)
        prev = cur
