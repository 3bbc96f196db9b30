"""The high-order horizontal flux of MonotoneAdv (omega_amd/csrc/MonotoneAdv.h, "The high-order horizontal flux") on
the CPU: the tables the library builds on the host (omg_monoadv_high_order_tables: what MonotoneAdv::setHorzOrder
uploads; a MonotoneAdv itself needs a device), and the properties of the contract on its NumPy restatement
(tests/monotone_adv_reference.py), which the device reproduces bit for bit
(tests/test_monotone_adv_high_order_gpu.py)."""
import math

import numpy as np
import pytest

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests import monotone_adv_reference as MR
from tests.meshes import named_mesh
from tests.monotone_adv_fixtures import CONST, CONST_VALUE, ORDERS, RANDOM, STEP, HoRig, Inputs, MonoRig

MESHES = ("hex24x20", "ico3", "fib700_coast_ragged")
K = 3
EPS = 2.0 ** -53

_RIGS = {}


def rig(name, order=4, coef=0.25, upwind=False):
    """(rig, inputs) of a mesh and an order, built once; the fixture's conditions (4) are asserted here"""
    key = (name, order, coef, upwind)
    if key not in _RIGS:
        R = HoRig(name, K).set_order(order, coef)
        I = R.inputs(seed=11, upwind=upwind)
        R.fractions = R.check_ho(I)
        _RIGS[key] = (R, I)
    return _RIGS[key]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the tables
# ---------------------------------------------------------------------------------------------------------------------
class NumpyFit:
    """The rule of MonotoneAdv.h for the fit cells and the fit, evaluated in NumPy on a rig's mesh: `cand` the cells
    that pass the connectivity conditions, and for each of them the offsets d [n][2] in the documented frame, L, the
    scaled matrix P [n][5] and its singular values."""

    def __init__(self, R):
        M, m, nc, ne = R.M, R.mesh, R.nc, R.ne
        geo = MR.geometry(R.g)
        X = np.stack([m.get_array(a + "Cell") for a in "XYZ"], axis=1)
        rad = geo["sphere_radius"]
        self.cell, self.nbr, self.d, self.L, self.P, self.sv = [], {}, {}, {}, {}, {}
        for c in range(nc):
            n = int(M.neoc[c])
            e = M.eoc[c, :n]
            if n < 5 or not ((e >= 0) & (e < ne)).all() or not M.open_edge[e].all():
                continue
            nb = np.where(M.coe[e, 0] == c, M.coe[e, 1], M.coe[e, 0])
            if not ((nb >= 0) & (nb < nc)).all():
                continue
            dx = X[nb] - X[c]
            if rad > 0.0:
                rc = X[c] / np.linalg.norm(X[c])
                axis = np.array([0.0, 0.0, 1.0]) if abs(rc[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
                e1 = np.cross(axis, rc)
                e1 /= np.linalg.norm(e1)
                e2 = np.cross(rc, e1)
                rn = X[nb] / np.linalg.norm(X[nb], axis=1)[:, None]
                tan = dx - (dx @ rc)[:, None] * rc
                arc = rad * np.arctan2(np.linalg.norm(np.cross(rc, rn), axis=1), rn @ rc)
                tan *= (arc / np.linalg.norm(tan, axis=1))[:, None]
                d = np.stack([tan @ e1, tan @ e2], axis=1)
            else:
                for a, per in ((0, geo["x_period"]), (1, geo["y_period"])):
                    if per > 0.0:
                        dx[:, a] -= per * np.rint(dx[:, a] / per)
                d = dx[:, :2]
            L = np.hypot(d[:, 0], d[:, 1]).mean()
            x, y = d[:, 0] / L, d[:, 1] / L
            P = np.stack([x, y, x * x, x * y, y * y], axis=1)
            self.cell.append(c)
            self.nbr[c], self.d[c], self.L[c], self.P[c] = nb, d, L, P
            self.sv[c] = np.linalg.svd(P, compute_uv=False)
        self.fit = np.zeros(R.nc_size, bool)
        for c in self.cell:
            self.fit[c] = self.sv[c][-1] > 1.0e-8 * self.sv[c][0]  # full column rank

    def gamma(self, c):
        """n*p*eps: the constant of a Householder least-squares solve of an n x p system (Higham, Accuracy and Stability
        of Numerical Algorithms, theorem 20.3 has c*n*p*eps with a small integer c)"""
        return len(self.nbr[c]) * 5 * EPS

    def cond(self, c):
        return self.sv[c][0] / self.sv[c][-1]


_FITS = {}


def numpy_fit(name):
    if name not in _FITS:
        _FITS[name] = NumpyFit(rig(name)[0])
    return _FITS[name]


@pytest.mark.parametrize("name", MESHES)
def test_fit_cells_are_those_of_the_rule(name):
    R, _ = rig(name)
    F = numpy_fit(name)
    assert np.array_equal(R.H.fit, F.fit)
    assert not R.H.fit[R.nc:].any()
    print(name, "fit cells", int(F.fit.sum()), "of", R.nc, "largest cond", max(F.cond(c) for c in F.cell))
    # a cell that is not a fit cell has zero weights; an edge is high when it is masked in and both its cells are fit
    assert not R.H.weight[~R.H.fit].any()
    M = R.M
    e = np.arange(M.ne)
    c0, c1 = np.minimum(M.coe[e, 0], R.nc_size - 1), np.minimum(M.coe[e, 1], R.nc_size - 1)
    assert np.array_equal(R.H.high, M.open_edge & F.fit[c0] & F.fit[c1])


def test_weights_give_the_exact_hessians_of_the_quadratics():
    """hex24x20: HessWeight applied to 1, x, y, x^2, x*y, y^2 in minimum-image coordinates about each cell.  The solve
    has no residual on these, so its forward error is of the order eps*cond(P): with the computed weights W + dW,
    |dW[:, t]| <= gamma*cond(P)*|W[:, t]| in the 2-norm (gamma = n*p*eps), the error of sum_j W[j][t]*b[j] is at most
    gamma*cond(P)*|W[:, t]|*|b| plus the n roundings of the sum, n*eps*sum_j |W[j][t]*b[j]|."""
    R, _ = rig("hex24x20")
    F = numpy_fit("hex24x20")
    assert F.fit[: R.nc].all()
    exact = np.zeros((6, 3))
    exact[3, 0], exact[4, 1], exact[5, 2] = 2.0, 1.0, 2.0
    worst = 0.0
    for c in F.cell:
        d, n = F.d[c], len(F.nbr[c])
        x, y = d[:, 0], d[:, 1]
        b = np.stack([np.zeros(n), x, y, x * x, x * y, y * y])  # m(d_j) - m(0)
        W = R.H.weight[c, :n]  # [n][3]
        got = b @ W
        bound = (F.gamma(c) * F.cond(c) * np.linalg.norm(b, axis=1)[:, None] * np.linalg.norm(W, axis=0)[None, :]
                 + n * EPS * (np.abs(b) @ np.abs(W)))
        err = np.abs(got - exact)
        assert (err <= bound).all(), (c, err, bound)
        worst = max(worst, (err / np.maximum(bound, 1e-300)).max())
    print("hex24x20: largest error / bound", worst, "cond", F.cond(F.cell[0]))


@pytest.mark.parametrize("name", ("ico3", "fib700_coast_ragged"))
def test_weights_agree_with_numpy_lstsq(name):
    """Both solves err by at most gamma*cond(P)*|P+| (2-norm, |P+| = 1/sigma_min) in the scaled pseudo-inverse, and the
    two evaluations of the offsets differ by roundings that perturb P+ by no more (a relative perturbation dP of P
    changes P+ by about cond(P)*|P+|*|dP|/|P|); the weights are rows of P+ times at most 2/L^2."""
    R, _ = rig(name)
    F = numpy_fit(name)
    worst = 0.0
    for c in F.cell:
        if not F.fit[c]:
            continue
        n, L = len(F.nbr[c]), F.L[c]
        pinv = np.linalg.lstsq(F.P[c], np.eye(n), rcond=None)[0]  # [5][n]
        want = np.stack([2.0 * pinv[2], pinv[3], 2.0 * pinv[4]], axis=1) / (L * L)
        bound = 3.0 * F.gamma(c) * F.cond(c) / F.sv[c][-1] * 2.0 / (L * L)
        err = np.abs(R.H.weight[c, :n] - want).max()
        assert err <= bound, (c, err, bound)
        worst = max(worst, err / bound)
    print(name, "largest difference / bound", worst, "largest cond", max(F.cond(c) for c in F.cell if F.fit[c]))


@pytest.mark.parametrize("name", MESHES)
def test_direction_coefficients(name):
    R, _ = rig(name)
    F = numpy_fit(name)
    M, H = R.M, R.H
    dc = R.mesh.get_array("DcEdge")
    n_high = 0
    for c in range(R.nc):
        for j in range(int(M.neoc[c])):
            e = M.eoc[c, j]
            if not (0 <= e < M.ne and H.high[e]):
                assert not H.own[c, j].any() and not H.across[c, j].any()
                continue
            n_high += 1
            nb = M.coe[e, 1] if M.coe[e, 0] == c else M.coe[e, 0]
            j2 = int(np.nonzero(M.eoc[nb, : M.neoc[nb]] == e)[0][0])
            assert H.across[c, j].tobytes() == H.own[nb, j2].tobytes()  # a copy: the same bits
            assert H.own[c, j, 0] != 0.0 or H.own[c, j, 2] != 0.0  # (how the kernels tell a high slot)
            d = F.d[c][j]
            cs, sn = d / np.hypot(*d)
            want = dc[e] ** 2 / 12.0 * np.array([cs * cs, 2.0 * cs * sn, sn * sn])
            # cs, sn: a few roundings each on operands of relative size 1; the products a few more
            assert np.abs(H.own[c, j] - want).max() <= 32 * EPS * dc[e] ** 2 / 12.0
    assert not H.own[R.nc:].any() and not H.across[R.nc:].any()
    assert n_high == 2 * int(H.high.sum())


def test_refusals_of_the_configuration():
    R, _ = rig("hex24x20")
    E = oa.OmegaAmdError
    for order in (1, 5, 0, -4):
        with pytest.raises(E, match="is not 2, 3 or 4"):
            oa.monotone_adv_high_order_tables(R.mesh, order)
    for coef in (0.0, -0.25, 1.5, float("nan")):
        with pytest.raises(E, match=r"outside \(0, 1\]"):
            oa.monotone_adv_high_order_tables(R.mesh, 3, coef)
        oa.monotone_adv_high_order_tables(R.mesh, 4, coef)  # unused at the other orders
    for bad in (-1.0, float("inf"), float("nan")):
        for kw in ("sphere_radius", "x_period", "y_period"):
            with pytest.raises(E, match="negative or not finite"):
                oa.monotone_adv_high_order_tables(R.mesh, 4, **{kw: bad})
    assert not any(a.any() for a in oa.monotone_adv_high_order_tables(R.mesh, 2).values())  # order 2 builds nothing


# ---------------------------------------------------------------------------------------------------------------------
# 2. the order of accuracy
# ---------------------------------------------------------------------------------------------------------------------
def divergence_error(n, order, coef):
    """max |unlimited flux divergence - (-U.grad(phi))| over the cells of planar_hex(n, n) of unit width: a smooth field
    in a uniform oblique flow, h = 1"""
    g = planar_hex(n, n, 1.0 / n)
    R = HoRig(g, 1)
    M, nc, ne = R.M, R.nc, R.ne
    lx, ly = g["x_period"], g["y_period"]
    kx, ky = 2.0 * np.pi / lx, 2.0 * np.pi / ly
    x, y = R.mesh.get_array("XCell")[:nc], R.mesh.get_array("YCell")[:nc]
    ux, uy = 1.0, 0.6
    phi = np.full((R.nc_size, 1), np.nan)
    phi[:nc, 0] = np.sin(kx * x + 0.3) * np.cos(ky * y) + 0.5 * np.cos(kx * x + 2.0 * ky * y)
    px = kx * np.cos(kx * x + 0.3) * np.cos(ky * y) - 0.5 * kx * np.sin(kx * x + 2.0 * ky * y)
    py = -ky * np.sin(kx * x + 0.3) * np.sin(ky * y) - ky * np.sin(kx * x + 2.0 * ky * y)
    ang = R.mesh.get_array("AngleEdge")
    u = np.full((R.ne_size, 1), np.nan)
    u[:ne, 0] = ux * np.cos(ang[:ne]) + uy * np.sin(ang[:ne])
    h = np.full((R.nc_size, 1), np.nan)
    h[:nc] = 1.0
    if order == 2:
        got = MR.flux_divergence(M, h, u, phi, None, None, flux="high")
    else:
        R.set_order(order, coef)
        assert R.H.high.all()
        got = MR.flux_divergence(M, h, u, phi, None, None, flux="high", high=(R.H, MR.hessians(R.H, phi)))
    return float(np.abs(got[:, 0] + (ux * px + uy * py)).max())


def test_order_of_accuracy():
    orders = {}
    for label, order, coef in (("centred", 2, 0.25), ("order 4", 4, 0.25), ("order 3, beta = 1", 3, 1.0),
                               ("order 3, beta = 0.25", 3, 0.25)):
        e24, e48 = divergence_error(24, order, coef), divergence_error(48, order, coef)
        orders[label] = math.log2(e24 / e48)
        print(label, "errors", e24, e48, "observed order", orders[label])
    assert orders["order 4"] >= 3.5
    assert orders["order 3, beta = 1"] >= 2.7
    assert orders["centred"] <= 2.3


# ---------------------------------------------------------------------------------------------------------------------
# 3. the limiter's properties
# ---------------------------------------------------------------------------------------------------------------------
def forward_step(R, I, L, flux="limited", hess=None):
    nc = R.nc
    hs = R.hess(I, L) if hess is None else hess
    si, so, p_min, p_max = MR.scale_factors(R.M, I.h_old, I.h_new, I.u, I.tracers[L], I.dt, I.upwind, high=(R.H, hs))
    tend = MR.flux_divergence(R.M, I.h_old, I.u, I.tracers[L], si, so, I.upwind, flux, high=(R.H, hs))
    return (I.h_old[:nc] * I.tracers[L, :nc] + I.dt * tend) / I.h_new[:nc], p_min, p_max


def growth(H):
    """G: how much larger than max|phi| the corrected edge value 0.5*(phi0 + phi1) - Corr can be.  |Hess[t][c]| <=
    (sum_j |W[c][j][t]|)*2*max|phi|, so |D| of a side <= g = sum_t |Q[t]|*(sum_j |W[j][t]|)*2 times max|phi|, and
    |Corr| <= |S| + beta*|T| <= (1 + beta)*(g0 + g1)*max|phi|; the largest over the high edges."""
    wsum = np.abs(H.weight).sum(axis=1)  # [cell][3]
    M = H.M
    e = np.nonzero(H.high)[0]
    g0 = (np.abs(H.q0[e]) * wsum[M.coe[e, 0]]).sum(axis=1) * 2.0
    g1 = (np.abs(H.q1[e]) * wsum[M.coe[e, 1]]).sum(axis=1) * 2.0
    return float(((1.0 + H.beta) * (g0 + g1)).max()) if e.size else 0.0


def margin(R, I, L):
    """tests/test_monotone_adv.py::margin re-derived for the corrected flux: a term is now at most S*(1 + G) in magnitude,
    S = 2*max(h)*max|phi| and G of `growth`, and its chain is 9 roundings longer (D0 and D1 are evaluated side by side:
    3 products and 2 sums = 5 on the longer path, then S or T 1, Beta*T 1, S +- B 1, 0.5*(..) - Corr 1), so a quantity
    errs by at most (n + 1)*(n + 20)*eps*S*(1 + G) and the margin is 5 of them over min(hNew)."""
    nc = R.nc
    return margin_value(R.M.eoc.shape[1], I.h_old[:nc].max(), np.abs(I.tracers[L, :nc]).max(), I.h_new[:nc].min(),
                        growth(R.H))


def margin_value(n, h_max, phi_max, h_new_min, g):
    """the margin derived in `margin` from its five figures"""
    return 5.0 * (n + 1) * (n + 20) * EPS * (2.0 * h_max * phi_max * (1.0 + g)) / h_new_min


@pytest.mark.parametrize("upwind", (False, True))
@pytest.mark.parametrize("order,coef", ORDERS)
@pytest.mark.parametrize("name", MESHES)
def test_update_stays_inside_the_neighbourhood_range(name, order, coef, upwind):
    R, I = rig(name, order, coef, upwind)
    print(name, order, "limited / free fraction of the random tracer", R.fractions, "G", growth(R.H))
    for L in (STEP, RANDOM, CONST):
        new, p_min, p_max = forward_step(R, I, L)
        m = margin(R, I, L)
        over = max((new - p_max).max(), (p_min - new).max())
        print(name, order, upwind, L, "outside by", over, "margin", m)
        assert np.isfinite(new).all()
        assert over <= m


@pytest.mark.parametrize("order,coef", ORDERS)
@pytest.mark.parametrize("name", MESHES)
def test_unlimited_high_order_flux_leaves_the_range(name, order, coef):
    R, I = rig(name, order, coef)
    new, p_min, p_max = forward_step(R, I, STEP, flux="high")
    over = max((new - p_max).max(), (p_min - new).max())
    print(name, order, "unlimited high-order flux outside by", over)
    assert over > 1.0e-2
    # and it is not the centred flux: the correction is at work
    centred = MR.flux_divergence(R.M, I.h_old, I.u, I.tracers[STEP], None, None, flux="high")
    high = MR.flux_divergence(R.M, I.h_old, I.u, I.tracers[STEP], None, None, flux="high", high=(R.H, R.hess(I, STEP)))
    assert not np.array_equal(centred, high)


@pytest.mark.parametrize("order,coef", ORDERS)
def test_tracer_content_is_conserved_on_the_periodic_mesh(order, coef):
    """the bound of tests/test_monotone_adv.py (iii): it is about F, whatever FHigh is made of"""
    R, I = rig("hex24x20", order, coef)
    M, nc, n = R.M, R.nc, R.M.eoc.shape[1]
    assert M.open_edge.all() and R.H.high.all()
    e = np.arange(M.ne)
    for L in (STEP, RANDOM):
        hs = R.hess(I, L)
        si, so, _, _ = MR.scale_factors(M, I.h_old, I.h_new, I.u, I.tracers[L], I.dt, high=(R.H, hs))
        tend = MR.flux_divergence(M, I.h_old, I.u, I.tracers[L], si, so, high=(R.H, hs))
        _, f_low, _, a = MR.edge_terms(M, e, M.coe[e, 0], M.coe[e, 1], I.h_old, I.u, I.tracers[L], False, (R.H, hs))
        f = f_low + MR.edge_scale(a, si, so, M.coe[e, 0], M.coe[e, 1]) * a
        for k in range(K):
            drift = abs(math.fsum(R.area[:nc] * tend[:, k]))
            bound = (n + 3) * EPS * 2.0 * np.abs(f[:, k]).sum()
            print(order, L, k, "drift", drift, "bound", bound)
            assert drift <= bound


@pytest.mark.parametrize("order,coef", ORDERS)
@pytest.mark.parametrize("name", MESHES)
def test_constant_tracer_stays_constant(name, order, coef):
    R, I = rig(name, order, coef)
    hs = R.hess(I, CONST)
    assert not hs[:, : R.nc].any()  # Hess == 0.0 exactly
    e = np.nonzero(R.M.open_edge)[0]
    a = MR.edge_terms(R.M, e, R.M.coe[e, 0], R.M.coe[e, 1], I.h_old, I.u, I.tracers[CONST], False, (R.H, hs))[3]
    assert not a.any()  # A = 0 exactly
    new, p_min, p_max = forward_step(R, I, CONST)
    assert (p_min == CONST_VALUE).all() and (p_max == CONST_VALUE).all()
    assert np.abs(new - CONST_VALUE).max() <= margin(R, I, CONST)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the coast
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,coef", ORDERS)
def test_an_edge_that_is_not_high_has_the_centred_flux(order, coef):
    R, I = rig("fib700_coast_ragged", order, coef)
    M, H, nc = R.M, R.H, R.nc
    low = np.nonzero(M.open_edge & ~H.high)[0]
    high = np.nonzero(H.high)[0]
    assert low.size and high.size
    hs = R.hess(I, RANDOM)
    for e, same in ((low, True), (high, False)):
        c0, c1 = M.coe[e, 0], M.coe[e, 1]
        got = MR.edge_terms(M, e, c0, c1, I.h_old, I.u, I.tracers[RANDOM], False, (H, hs))[2]
        centred = MR.edge_terms(M, e, c0, c1, I.h_old, I.u, I.tracers[RANDOM], False)[2]
        assert np.array_equal(got, centred) == same
    # NaN in the Hess rows of the cells that are not fit cells changes nothing
    ref = R.reference_ho(I, 3)
    assert all(np.isfinite(x[:, :nc]).all() for x in ref[:3])
    planted = hs.copy()
    planted[:, ~H.fit] = np.nan
    assert (~H.fit[:nc]).any()
    a = forward_step(R, I, RANDOM, hess=planted)
    b = forward_step(R, I, RANDOM)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.isfinite(a[0]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the halo
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,coef", ORDERS)
def test_two_parts_at_halo_3_match_on_owned_cells(order, coef):
    nt, halo = 3, 3
    R1 = HoRig("hex24x20", K).set_order(order, coef)
    I1 = R1.inputs(seed=8, ntracers=nt)
    one = R1.reference_ho(I1, nt)
    cid1, eid1 = R1.decomp.get_array("CellID")[: R1.nc] - 1, R1.decomp.get_array("EdgeID")[: R1.ne] - 1
    ncg, neg = cid1.max() + 1, eid1.max() + 1
    glob = {}
    for n, ids, rows in (("h_old", cid1, ncg), ("h_new", cid1, ncg), ("u", eid1, neg)):
        glob[n] = np.zeros((rows, K))
        glob[n][ids] = getattr(I1, n)[: len(ids)]
    glob["tracers"] = np.zeros((nt, ncg, K))
    glob["tracers"][:, cid1] = I1.tracers[:, : R1.nc]
    names = ("Tend", "ScaleIn", "ScaleOut", "Hess")
    result = {}
    for w, name in enumerate(names):
        a = np.moveaxis(one[w], -2, 0)[: R1.nc]  # cells first
        result[name] = np.zeros((ncg,) + a.shape[1:])
        result[name][cid1] = a
    for rank in range(2):
        R = HoRig("hex24x20", K, nparts=2, rank=rank, halo=halo).set_order(order, coef)
        own = R.mesh.NCellsOwned
        assert R.nc > own and not R.H.fit[: R.nc].all()  # the rim is not fitted
        cid, eid = R.decomp.get_array("CellID")[: R.nc] - 1, R.decomp.get_array("EdgeID")[: R.ne] - 1
        I = Inputs()
        I.upwind, I.dt = False, I1.dt
        for n, ids, size in (("h_old", cid, R.nc_size), ("h_new", cid, R.nc_size), ("u", eid, R.ne_size)):
            a = np.full((size, K), np.nan)
            a[: len(ids)] = glob[n][ids]
            setattr(I, n, a)
        I.tracers = np.full((nt, R.nc_size, K), np.nan)
        I.tracers[:, : R.nc] = glob["tracers"][:, cid]
        got = R.reference_ho(I, nt)
        for w, name in enumerate(names):
            a = np.moveaxis(got[w], -2, 0)[:own]
            assert np.array_equal(a, result[name][cid[:own]]), f"{name} on the owned cells of part {rank}"
