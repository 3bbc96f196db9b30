"""Properties of the restatement of VertRemap's contract (tests/vert_remap_reference.py) itself -- what makes it an oracle
worth comparing the kernels against: it conserves the column integral to rounding, it stays inside the source values it
overlaps, a uniform column and a remap onto the same grid come back bit for bit, the L1 error of a smooth profile falls
with the order of the reconstruction, the shapes at which the boundary rules meet behave, and its target thickness is
VertCoord's.  No device."""
import math

import numpy as np
import pytest

from tests import column_reference as CR
from tests import vert_remap_reference as VR

U = 2.0 ** -53  # the unit roundoff
ORDERS = (1, 2, 3)


def random_columns(rng, M, N, spread=0.3, ragged=True):
    """M packed columns of up to N rows: thickness of scale 10, the target the source perturbed by up to +-spread and
    rescaled to the source's total (to rounding), means of scale 1 with sign changes and flat runs"""
    n = rng.integers(1, N + 1, M) if ragged else np.full(M, N)
    if ragged:
        n[: min(4, M)] = np.arange(1, 5)[: min(4, M)].clip(max=N)
    hs = rng.uniform(2.0, 20.0, (M, N))
    ht = hs * rng.uniform(1.0 - spread, 1.0 + spread, (M, N))
    valid = np.arange(N)[None, :] < n[:, None]
    ht *= (np.where(valid, hs, 0.0).sum(axis=1) / np.where(valid, ht, 0.0).sum(axis=1))[:, None]
    a = np.cumsum(rng.uniform(-1.0, 1.0, (M, N)), axis=1)
    if N >= 6:
        a[:, N // 2: N // 2 + 2] = a[:, N // 2: N // 2 + 1]  # a flat pair
    return hs, ht, a, n


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("spread", [0.3, 0.9])
def test_the_column_integral_is_conserved(order, spread):
    """sum_k ht'[k]*new[k] = sum_j hs[j]*a[j] per column, ht'[k] = ZT[k+1] - ZT[k].  The bound, first order in u, with
    A = max|a|, H = zs[N]:
      - a piece is hs[j] times a polynomial of about 14 operations on terms of at most 4A (|aL| <= A, |Dl| <= 2A and the
        limiter leaves |a6| <= |Dl|): 64 u A hs[j] at most; the fractions x a piece ends and the next one starts with are
        the same bits, so the pieces of a cell telescope to hs[j]*a[j] in exact arithmetic: in all 64 u A S, with S the
        sum of hs[j] over all pieces;
      - a layer that is one source cell takes a[j] with the width fl(zs[j+1] - zs[j]), which differs from hs[j] by the
        rounding of the interface, u H, and of the difference: 2 u A H per layer at most;
      - the span-1 additions of a layer's sum, its division by the width, the width itself and the product the test
        forms: (span + 3) u A ht'[k], over the column (N + 3) u A H at most; the clamp moves a result by no more than
        its own rounding error (the limited reconstructions are monotone), which doubles this;
      - the test's two sums are math.fsum of rounded products: 2 u A H more.
    Total: u A (64 S + (4N + 8) H)."""
    rng = np.random.default_rng(11 + order)
    hs, ht, a, n = random_columns(rng, 200, 40, spread)
    info = {}
    new = VR.column_core(hs, ht, a, n, order, info)
    worst = 0.0
    for m in range(len(n)):
        N = n[m]
        w = np.diff(info["ZT"][m, : N + 1])
        got = math.fsum(w * new[m, :N])
        want = math.fsum(hs[m, :N] * a[m, :N])
        A, H = np.abs(a[m, :N]).max(), info["zs"][m, N]
        S = sum(hs[m, info["j0"][m, k]: info["j1"][m, k] + 1].sum() for k in range(N))
        bound = U * A * (64.0 * S + (4 * N + 8) * H)
        assert abs(got - want) <= bound, (m, N, got - want, bound)
        worst = max(worst, abs(got - want) / bound)
    print(f"order {order} spread {spread}: worst |error| / bound = {worst:.3f}")
    assert 0.0 < worst


@pytest.mark.parametrize("order", ORDERS)
def test_results_stay_inside_the_overlapped_source_values(order):
    rng = np.random.default_rng(5)
    hs, ht, a, n = random_columns(rng, 300, 33, 0.9)
    info = {}
    new = VR.column_core(hs, ht, a, n, order, info)
    for m in range(len(n)):
        for k in range(n[m]):
            j0, j1 = info["j0"][m, k], info["j1"][m, k]
            s = a[m, max(j0 - 1, 0): min(j1 + 1, n[m] - 1) + 1]
            assert s.min() <= new[m, k] <= s.max(), (m, k)
    assert np.array_equal(new[np.arange(33)[None, :] >= n[:, None]], a[np.arange(33)[None, :] >= n[:, None]])
    # a uniform column stays uniform bit for bit, whatever the grids
    flat = np.full_like(a, 0.1 + 1.0 / 3.0)
    assert np.array_equal(VR.column_core(hs, ht, flat, n, order), flat)
    # the same grid returns the same bits
    assert np.array_equal(VR.column_core(hs, hs, a, n, order), a)


def smooth_case(N):
    """Cell means of f(z) = cos(2 pi z) + 0.3 cos(6 pi z) on [0, 1] between two grids z(xi), xi = j/N, with the spacings
    (1 + 0.3 cos(2 pi xi))/N and (1 + 0.2 cos(2 pi xi) - 0.25 cos(4 pi xi))/N: from 0.7 to 1.3 and from 0.55 to 1.45 of
    the mean, with different wave numbers, so that the offset of the two grids runs through every fraction of a cell
    (two mirror images of one grid would not do: the PCM error is a sawtooth of that offset, and its L1 norm then depends
    on how N happens to align the two).  f' = 0 at both ends: the contract keeps the first and the last cell constant
    whatever the order, and a profile with a gradient there would measure that rule (an O(h^2) term in L1), not the
    reconstruction."""
    xi = np.arange(N + 1) / N
    zs = xi + 0.3 * np.sin(2 * np.pi * xi) / (2 * np.pi)
    zt = xi + 0.2 * np.sin(2 * np.pi * xi) / (2 * np.pi) - 0.25 * np.sin(4 * np.pi * xi) / (4 * np.pi)

    def F(z):  # the antiderivative
        return np.sin(2 * np.pi * z) / (2 * np.pi) + 0.3 * np.sin(6 * np.pi * z) / (6 * np.pi)

    return zs, zt, F


@pytest.mark.parametrize("order,nominal", [(1, 1.0), (2, 2.0), (3, 3.0)])
def test_the_error_falls_with_the_order(order, nominal):
    err = []
    for N in (64, 128, 256):
        zs, zt, F = smooth_case(N)
        hs, ht = np.diff(zs)[None, :], np.diff(zt)[None, :]
        a = (np.diff(F(zs)) / np.diff(zs))[None, :]
        info = {}
        new = VR.column_core(hs, ht, a, np.array([N]), order, info)[0]
        ZT = info["ZT"][0]
        exact = np.diff(F(ZT)) / np.diff(ZT)
        err.append(float(np.sum(np.diff(ZT) * np.abs(new - exact))))
    rates = [math.log2(err[i] / err[i + 1]) for i in range(2)]
    print(f"order {order}: L1 error {err[0]:.3e} {err[1]:.3e} {err[2]:.3e}, observed order {rates[0]:.2f} {rates[1]:.2f}")
    # the restatement's own figures (N = 64 -> 128 -> 256): PCM 1.26 1.18, PLM 2.66 2.51, PPM 2.99 3.00
    assert min(rates) >= nominal - 0.25, rates


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_short_columns_where_the_boundary_rules_meet(order, N):
    rng = np.random.default_rng(N)
    hs, ht, a, n = random_columns(rng, 50, N, 0.5, ragged=False)
    info = {}
    new = VR.column_core(hs, ht, a, n, order, info)
    assert np.isfinite(new).all()
    if N == 1:
        assert np.array_equal(new, a)  # one layer: ZT is the source cell
    if N <= 2 or order == 1:  # every cell constant: PCM whatever the order
        assert np.array_equal(new, VR.column_core(hs, ht, a, n, 1))
    if N >= 3 and order > 1:
        assert not np.array_equal(new, VR.column_core(hs, ht, a, n, 1))
    w = np.diff(info["ZT"], axis=1)
    assert np.allclose((w * new).sum(axis=1), (hs * a).sum(axis=1), rtol=1e-13, atol=1e-12)


@pytest.mark.parametrize("order", ORDERS)
def test_shapes_that_can_go_wrong(order):
    one = np.array([5])
    hs = np.array([[10.0, 10.0, 10.0, 10.0, 10.0]])
    a = np.array([[1.0, 2.0, 4.0, 3.0, 2.5]])
    info = {}
    # a target layer inside one source cell (layer 1 is 2 .. 4 of cell 0) and one over three cells and more (layer 2)
    ht = np.array([[2.0, 2.0, 31.0, 5.0, 10.0]])
    new = VR.column_core(hs, ht, a, one, order, info)
    assert info["span"][0].tolist() == [1, 1, 4, 1, 1] and info["j0"][0, 1] == 0 and info["j1"][0, 1] == 0
    assert new[0, 0] == 1.0 and new[0, 1] == 1.0  # cell 0 is constant
    assert new[0, 4] == 2.5  # the last layer is the last source cell bit for bit
    assert math.isclose((np.diff(info["ZT"][0]) * new[0]).sum(), (hs * a).sum(), rel_tol=1e-14)
    # the target total larger than the source's: the layers past the source's bottom have no width and take the value
    # there; the last one with width ends at the bottom
    ht = np.array([[10.0, 10.0, 10.0, 25.0, 10.0]])
    new = VR.column_core(hs, ht, a, one, order, info)
    assert info["ZT"][0].tolist() == [0.0, 10.0, 20.0, 30.0, 50.0, 50.0] and info["span"][0].tolist() == [1, 1, 1, 2, 0]
    assert new[0, :3].tolist() == [1.0, 2.0, 4.0] and new[0, 4] == 2.5  # the point value of the constant last cell
    assert math.isclose(new[0, 3], (3.0 + 2.5) / 2, rel_tol=1e-15)
    # ... and smaller: the last layer is widened to the source's bottom
    ht = np.array([[10.0, 10.0, 10.0, 5.0, 1.0]])
    new = VR.column_core(hs, ht, a, one, order, info)
    assert info["ZT"][0].tolist() == [0.0, 10.0, 20.0, 30.0, 35.0, 50.0] and info["span"][0].tolist() == [1, 1, 1, 1, 2]
    assert math.isclose((np.diff(info["ZT"][0]) * new[0]).sum(), (hs * a).sum(), rel_tol=1e-14)
    # zt[k] equal to a zs[j] bit for bit, inside a longer layer: 0.1 + 0.2 is not 0.3, the interfaces are compared as
    # they were summed
    hs = np.array([[0.1, 0.2, 0.4, 0.3]])
    ht = np.array([[0.1 + 0.2, 0.2, 0.2, 0.3]])
    a = np.array([[1.0, 2.0, 4.0, 3.0]])
    new = VR.column_core(hs, ht, a, np.array([4]), order, info)
    assert info["ZT"][0, 1] == info["zs"][0, 2] and info["span"][0].tolist() == [2, 1, 1, 2]
    assert new[0, 0] == (0.1 * 1.0 + 0.2 * 2.0) / (0.1 + 0.2)  # two whole cells: no reconstruction enters
    # ... and where they differ in the last bit they differ: zt[3] = 0.7 lies one ulp above zs[3], layer 3 starts with
    # that sliver of cell 2
    assert info["ZT"][0, 3] < info["zs"][0, 3] and info["j0"][0, 3] == 2 and 3.0 <= new[0, 3] <= 4.0


def test_the_target_is_vert_coords():
    """compute_target against the restatement of VertCoord::computeTargetThickness (tests/column_reference.py) after its
    pressure pass.  The two differ in the column total only: SumH, N - 1 additions, against
    (PInt[KMax+1] - PInt[KMin]) / (g Rho0), where PInt[KMax+1] = fl(Ps + acc) and acc sums the N rounded products
    (g Rho0) h[K].  First order in u: |SumH - sum h| <= (N-1) u sum h;  acc = g Rho0 sum h (1 + (N-1+1) u), Ps + acc is
    rounded once (u (Ps + acc)), the difference with PInt[KMin] = Ps once more, the product g*Rho0 and the quotient once
    each: |total_p - sum h| <= (N + 4) u sum h + u Ps / (g Rho0).  So the two Coeff differ by at most
    dC = (2N + 3) u sum h + u Ps / (g Rho0) -- plus u |Coeff| for each one's own subtraction, which the four roundings
    of the point-wise expression below absorb -- and the targets by Ref W / SumWh dC + 4 u |Target|."""
    rng = np.random.default_rng(3)
    M, K = 120, 24
    lo = rng.integers(0, 4, M)
    hi = np.minimum(K - 1, lo + rng.integers(0, K, M))
    lo[:3], hi[:3] = (0, 5, 1), (K - 1, 5, -1)  # a full column, a single layer, land
    h, ref = rng.uniform(0.5, 40.0, (M, K)), rng.uniform(1.0, 30.0, (M, K))
    ps = rng.uniform(0.9e5, 1.1e5, M)
    for kind in ("Uniform", "Fixed"):
        w = CR.movement_weights(kind, K)
        if kind == "Fixed":
            lo[lo > 0] = 0  # (the one moving level must be in the column, as in VertCoord)
        pint, pmid = np.zeros((M, K + 1)), np.zeros((M, K))
        CR.pressure(h, ps, lo, hi, M, CR.RHO0, pint, pmid)
        want, got = np.full((M, K), np.nan), np.full((M, K), np.nan)
        CR.target_thickness(pint, ref, w, lo, hi, M, CR.RHO0, want)
        VR.compute_target(h, ref, w, lo, hi, M, got)
        inside = (np.arange(K)[None, :] >= lo[:, None]) & (np.arange(K)[None, :] <= hi[:, None])
        assert np.array_equal(np.isnan(got), ~inside) and np.array_equal(np.isnan(want), ~inside)
        n = hi - lo + 1
        sum_h = np.where(inside, h, 0.0).sum(axis=1)
        sum_wh = np.where(inside, w[None, :] * ref, 0.0).sum(axis=1)
        dC = (2 * n + 3) * U * sum_h + U * ps / (CR.GRAVITY * CR.RHO0)
        with np.errstate(all="ignore"):
            bound = ref * w[None, :] / sum_wh[:, None] * dC[:, None] + 4 * U * np.abs(want)
        err = np.abs(got - want)
        assert np.all(err[inside] <= bound[inside])
        assert err[inside].max() > 0.0  # the two totals are not formed the same way
        print(f"{kind}: worst error / bound = {np.max(err[inside] / bound[inside]):.3f}")
        # the target conserves the column: its total is the thickness's
        assert np.allclose(np.where(inside, got, 0.0).sum(axis=1), sum_h, rtol=1e-13)
