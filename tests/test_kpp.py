"""The restatement of the Kpp contract (tests/kpp_reference.py) on its own, without a device: the scan is a cumulative
sum, the branches of the velocity scales meet where Large et al. chose their constants to make them meet, the neutral
limit, the boundary layer deepens with the friction velocity, the non-local redistribution conserves the column, and
the inputs of the GPU tests (tests/kpp_fixtures.py) are what those tests need them to be."""
import numpy as np
import pytest

from tests import kpp_reference as KR
from tests.kpp_fixtures import NT, KppRig
from tests.meshes import named_mesh

MESHES = ("hex24x20", "fib300_coast_ragged")
LEVELS = (1, 2, 3, 5, 8, 9, 33, 64, 65, 129, 256, 257, 1024)
KAPPA = KR.DEFAULTS["VonKarman"]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9, 33, 64, 65, 257, 1024])
def test_the_scan_is_the_cumulative_sum_to_rounding(n):
    rng = np.random.default_rng(n)
    W = n + 3
    t = rng.uniform(-1.0, 1.0, (40, W))
    start = rng.integers(0, 4, 40)
    stop = start + n - 1
    got = KR.scan(t, start, stop)
    k = np.arange(W)[None, :]
    inside = (k >= start[:, None]) & (k <= stop[:, None])
    want = np.cumsum(np.where(inside, t, 0.0), axis=1)
    assert np.array_equal(got[~inside], t[~inside])  # entries outside the range come back as they went in
    # both are sums of the same terms in another order: n roundings of partial sums no larger than sum |t|
    bound = n * np.finfo(float).eps * np.cumsum(np.where(inside, np.abs(t), 0.0), axis=1)
    assert np.all(np.abs(got - want)[inside] <= bound[inside])
    if n == 1:
        assert np.array_equal(got, t)
    if n == 2:  # one pass: T_1 + T_0, one rounding, the same as the sequential sum
        assert np.array_equal(got[inside], want[inside])


@pytest.mark.parametrize("momentum,zeta,near_value,far_value", [(False, KR.ZETA_S, 4.12311, 4.12325),
                                                                 (True, KR.ZETA_M, 1.43157, 1.43192)])
def test_the_branches_of_the_velocity_scales_meet(momentum, zeta, near_value, far_value):
    """at z = Zeta * u3, from either side, to 1e-3 relative (in units of kappa * us: 4.12311 against 4.12325 for wS,
    1.43157 against 1.43192 for wM)"""
    us, bf, h = 0.01, -1.0e-7, 50.0
    sig = zeta * ((us * us) * us) / (KAPPA * h * bf)  # z = Zeta * u3
    near, cb_near = KR.scale(momentum, KAPPA, us, bf, sig * (1.0 - 1.0e-9), h)
    far, cb_far = KR.scale(momentum, KAPPA, us, bf, sig * (1.0 + 1.0e-9), h)
    assert not cb_near and cb_far
    assert abs(far - near) <= 1.0e-3 * near
    assert abs(near / (KAPPA * us) - near_value) < 1.0e-5 and abs(far / (KAPPA * us) - far_value) < 1.0e-5


def test_the_neutral_limit_bit_for_bit():
    """Bf = 0: wS = wM = kappa * us, and VertDiff = BackgroundDiffusivity + (hbl * (kappa * us)) * G, bit for bit.
    The contract's ((kappa*us)*u3)/den returns kappa*us exactly when u3 is a power of two (the product and the quotient
    are then exact); for another u3 a product followed by a quotient may round twice and land one ulp off, whatever the
    library does.  So the bit-for-bit statement is made at friction velocities that are powers of two, and at any other
    it is: wS and wM agree bit for bit and are within one ulp of kappa * us."""
    us = 2.0 ** -np.arange(5, 12)
    for momentum in (False, True):
        w, cb = KR.scale(momentum, KAPPA, us, 0.0, 0.37, 80.0)
        assert np.array_equal(w, KAPPA * us) and not cb.any()
    any_us = np.random.default_rng(3).uniform(1.0e-4, 0.02, 1000)
    ws, _ = KR.scale(False, KAPPA, any_us, 0.0, 0.37, 80.0)
    wm, _ = KR.scale(True, KAPPA, any_us, 0.0, 0.37, 80.0)
    assert np.array_equal(ws, wm)
    assert np.all(np.abs(ws - KAPPA * any_us) <= np.spacing(KAPPA * any_us))
    # a whole column pass
    x = KppRig(named_mesh("hex24x20"), 33, device=False)
    us_c = 2.0 ** -(6.0 + np.arange(x.n_size) % 4)
    r = x.expected(us=us_c, bf=np.zeros(x.n_size))
    inside = r["inside"]
    assert inside.sum() > 1000 and not r["used_cbrt"].any()
    hbl = r["BoundaryLayerDepth"][:, None]
    with np.errstate(all="ignore"):
        sig = (x.zint[np.arange(x.n_size), np.clip(x.lo, 0, None)][:, None] - x.zint[:, : x.K]) / hbl
        g = sig * ((1.0 - sig) * (1.0 - sig))
        want = x.bg_diff + (hbl * (KAPPA * us_c[:, None])) * g
        want_v = x.bg_visc + (hbl * (KAPPA * us_c[:, None])) * g
    assert np.array_equal(r["VertDiff"][inside], want[inside]) and np.array_equal(r["VertVisc"][inside], want_v[inside])
    assert np.all(r["NonLocalShape"] == 0.0)


@pytest.mark.parametrize("mesh,K", [("hex24x20", 33), ("fib300_coast_ragged", 9)])
def test_the_boundary_layer_deepens_with_the_friction_velocity(mesh, K):
    """hbl is non-decreasing in us on a fixed column: a larger us raises the unresolved shear Vt2 and with it lowers
    every positive bulk Richardson number.  The columns are fixed as stable water (N2 >= 0: the buoyancy difference is
    positive) under a flux that is not destabilising (Bf >= 0: w = kappa us^4 / (us^3 + 5 z) grows with us); under a
    destabilising flux the convective scale kappa cbrt(As u3 - Cs z) falls with us, As being negative, and the depth
    need not grow."""
    x = KppRig(named_mesh(mesh), K, device=False)
    n2, bf = np.abs(x.n2), np.abs(x.bf)
    last = None
    for us in np.linspace(0.0, 0.02, 9):
        r = x.expected(n2=n2, bf=bf, us=np.full(x.n_size, us))
        hbl = r["BoundaryLayerDepth"]
        assert np.all(hbl[r["valid"]] > 0.0) and np.all(hbl[~r["valid"]] == 0.0)
        if last is not None:
            assert np.all(hbl >= last)
        last = hbl
    assert (r["BoundaryLayerIndex"][r["valid"]] > x.lo[r["valid"]]).all()


@pytest.mark.parametrize("mesh,K", [("hex24x20", 33), ("fib300_coast_ragged", 9), ("fib300_coast_ragged", 1)])
def test_the_non_local_flux_conserves_the_column_and_vanishes_for_a_stabilising_flux(mesh, K):
    x = KppRig(named_mesh(mesh), K, device=False)
    r = x.expected()
    dt = 600.0
    new = KR.apply_non_local(x.h, x.tr, NT, dt, x.flux, r["NonLocalShape"], x.lo, x.hi, x.n_own)
    own = np.zeros(x.n_size, bool)
    own[: x.n_own] = True
    act = x.active & own[:, None]
    changed = (new != x.tr) & ~np.isnan(x.tr)
    assert not changed[:, ~act].any()  # nothing outside the owned columns' ranges
    unstable = own & (x.bf < 0.0) & r["valid"]
    assert not changed[:, ~unstable].any()  # the identity for Bf >= 0 (NonLocalShape is 0 there)
    if K > 2:
        assert changed[:, unstable].any()
    h = np.where(act, x.h, 0.0)
    for t in range(NT):
        before, after = (np.where(act, h * a[t], 0.0) for a in (x.tr, new))
        # each level's increment is rounded a few times relative to its own size; the increments telescope to zero
        inc = np.abs(np.where(act, h * (new[t] - x.tr[t]), 0.0)).sum(axis=1) + np.abs(before).sum(axis=1)
        assert np.all(np.abs(after.sum(axis=1) - before.sum(axis=1)) <= 8.0 * K * np.finfo(float).eps * inc)
    assert np.array_equal(KR.apply_non_local(x.h, x.tr, NT, dt, None, r["NonLocalShape"], x.lo, x.hi, x.n_own), x.tr,
                          equal_nan=True)


@pytest.mark.parametrize("mesh", MESHES)
@pytest.mark.parametrize("K", LEVELS)
def test_the_inputs_are_what_the_gpu_tests_need(mesh, K):
    """few marginal columns; each of the three regimes of the velocity scales on at least 5 % of the active columns; a
    crossing inside the column and none at all both occur"""
    x = KppRig(named_mesh(mesh), K, device=False)
    r = x.expected()
    v = r["valid"]
    n = int(v.sum())
    assert n > 100
    assert r["marginal"][v].sum() <= 0.01 * n
    stable = v & (x.bf >= 0.0)
    cbrt = v & r["used_cbrt"]
    near = v & (x.bf < 0.0) & ~r["used_cbrt"]
    assert not (stable & cbrt).any()
    for regime in (stable, cbrt, near):
        assert regime.sum() >= 0.05 * n
    assert (x.us[v] == 0.0).any() and (x.bf[v] == 0.0).any()
    kb = r["BoundaryLayerIndex"]
    assert np.all(kb[~v] == -1) and np.all(kb[v] > x.lo[v]) and np.all(kb[v] <= x.hi[v] + 1)
    if K >= 3:
        assert (kb[v] <= x.hi[v]).any() and (kb[v] == x.hi[v] + 1).any()
        assert len(np.unique((kb - x.lo)[v])) >= min(K, 8) // 2  # spread over the column
    assert np.isfinite(r["BoundaryLayerDepth"]).all() and np.isfinite(r["BulkRichardson"]).all()
    assert np.isfinite(r["NonLocalShape"]).all()
