"""VertAdv without a device: the NumPy restatement of the contract (tests/vert_adv_reference.py) against what the
continuous terms must give -- a closed column, the z-level and Lagrangian limits of the transport, a constant tracer
advected like thickness, no force on a vertically uniform flow, a second-order interface value -- and its masking
rules.  Every test that draws random inputs asserts the fixture condition: a transport of both signs."""
import numpy as np
import pytest

from tests import vert_adv_reference as VR
from tests.meshes import named_mesh
from tests.vert_adv_fixtures import AdvRig, assert_both_signs, sign_fractions

EPS = np.finfo(np.float64).eps
MESHES = ("hex24x20", "fib700_coast_ragged")


def test_fixture_transport_has_both_signs():
    for mesh in MESHES:
        for K in (2, 15, 16, 37, 80):
            x = AdvRig(named_mesh(mesh), K, device=False)
            cnt = assert_both_signs(x.transport(), x.lo, x.hi, x.n_all)
            assert cnt > 0
    x = AdvRig(named_mesh("hex24x20"), 1, device=False)
    assert sign_fractions(x.transport(), x.lo, x.hi, x.n_all)[2] == 0  # one level: no interior interface


@pytest.mark.parametrize("mesh", MESHES)
@pytest.mark.parametrize("weights", ["Uniform", "Fixed"])
def test_column_is_closed(mesh, weights):
    """W[KMin] == 0 exactly, and the column sum of the new thickness tendency is SumD.  In exact arithmetic the sum
    telescopes to SumD - W[KMin].  Rounding: |Wt[K]| <= sum|D - TT| <= 2 sum|D| =: 2 S, so each of the two operations
    of (D - Wt[K]) + Wb rounds a number of at most 3 S (eps/2 each: 3 eps S per level), and summing K results of
    magnitude <= 5 S adds at most K * 5 S * eps/2 per partial sum over K sums; with K levels that is within
    (3 K + 2.5 K) eps S <= 6 K eps S.  (Fixed weights need KMin = 0: full columns.)"""
    K = 12
    x = AdvRig(named_mesh(mesh), K, weights=weights, full=weights == "Fixed", device=False)
    wt = x.transport()
    assert_both_signs(wt, x.lo, x.hi, x.n_all)
    rows = np.nonzero(x.active.any(axis=1))[0]
    assert np.all(wt[rows, x.lo[rows]] == 0.0)
    tend = VR.add_thickness_tend(x.d.copy(), wt, x.lo, x.hi, x.n_all)
    s_new = np.where(x.active, tend, 0.0).sum(axis=1)
    s_old = np.where(x.active, x.d, 0.0).sum(axis=1)
    s_abs = np.where(x.active, np.abs(x.d), 0.0).sum(axis=1)
    err = np.abs(s_new - s_old)
    print(f"closure: max |sum new - SumD| / (eps sum|D|) = {(err[rows] / (EPS * s_abs[rows])).max():.2f}")
    assert np.all(err <= 6.0 * K * EPS * s_abs)
    assert not np.array_equal(tend[x.active], x.d[x.active])


def test_fixed_weights_give_a_z_level_grid():
    """"Fixed" weights (1 at level 0): TT[K] = 0 exactly for K > 0, so Wt[K] = fl(Wt[K+1] + D[K]) and the new tendency
    (D[K] - Wt[K]) + Wt[K+1] is the rounding error of that one addition and of the two operations that undo it:
    at most 3 * eps/2 * max(|Wt[K]|, |Wt[K+1]|, |D[K]|) <= 1.5 eps sum|D|.  The top layer takes SumD."""
    K = 15
    x = AdvRig(named_mesh("hex24x20"), K, weights="Fixed", full=True, device=False)
    wt = x.transport()
    assert_both_signs(wt, x.lo, x.hi, x.n_all)
    tend = VR.add_thickness_tend(x.d.copy(), wt, x.lo, x.hi, x.n_all)
    s_abs = np.abs(x.d[: x.n_all]).sum(axis=1)
    assert np.all(np.abs(tend[: x.n_all, 1:]) <= 1.5 * EPS * s_abs[:, None])
    s_d = x.d[: x.n_all].sum(axis=1)
    assert np.all(np.abs(tend[: x.n_all, 0] - s_d) <= 2.0 * K * EPS * s_abs)
    assert np.abs(x.d[: x.n_all, 1:]).min() > 1.0e3 * EPS * s_abs.max()  # the inputs were not small


@pytest.mark.parametrize("mesh", MESHES)
def test_lagrangian_limit(mesh):
    """D = a_c * W * Ref per column (every layer already moves like its target): TT[K] = ((W Ref)/SumWh) * SumD with
    SumD = a SumWh (1 + K eps) at worst, so |D[K] - TT[K]| <= (K + 3) eps |D[K]| and the K-term sum Acc stays within
    K (K + 4) eps max|D|."""
    K = 16
    x = AdvRig(named_mesh(mesh), K, device=False)
    rng = np.random.default_rng(3)
    a = rng.uniform(-1.0e-4, 1.0e-4, x.n_size)
    d = a[:, None] * (x.w[None, :] * x.ref)
    wt = x.transport(d=d)
    bound = K * (K + 4) * EPS * np.where(x.active, np.abs(d), 0.0).max(axis=1)
    assert np.all(np.abs(np.where(x.active, wt, 0.0)) <= bound[:, None])
    assert np.abs(a).min() > 0.0


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("mesh", MESHES)
def test_constant_tracer_follows_thickness(mesh, order):
    """phi = phi0: the tracer update is phi0 times the thickness update.  Order 1 picks phi0 exactly; order 2 computes
    ((h0 phi0) + (h1 phi0)) / (h0 + h1) = phi0 (1 + 2.5 eps) at worst (two products, a sum, a quotient); a flux is one
    more rounding, the two operations of the update two more, and the thickness update they are compared with has two
    of its own: within 8 eps |phi0| (|Wt[K]| + |Wb|)."""
    K, phi0 = 16, 34.7
    x = AdvRig(named_mesh(mesh), K, device=False)
    wt = x.transport()
    assert_both_signs(wt, x.lo, x.hi, x.n_all)
    tr = np.full((2, x.n_size, K), phi0)
    got = VR.add_tracer_tend(np.zeros((2, x.n_size, K)), x.h, tr, wt, x.lo, x.hi, x.n_all, order)
    thick = VR.add_thickness_tend(np.zeros((x.n_size, K)), wt, x.lo, x.hi, x.n_all)
    wb = np.zeros_like(wt)
    wb[:, : K - 1] = wt[:, 1:]
    wb = np.where(np.arange(K)[None, :] < x.hi[:, None], wb, 0.0)
    bound = 8.0 * EPS * phi0 * (np.abs(wt) + np.abs(wb))
    for l in range(2):
        assert np.all(np.abs(got[l] - phi0 * thick)[x.active] <= bound[x.active])
    assert np.abs(thick[x.active]).max() > 0.0


@pytest.mark.parametrize("mesh", MESHES)
def test_vertically_uniform_flow_feels_no_force(mesh):
    """u[e][K] = u_e: UTop = 0.5 (u + u) = u exactly, both fluxes are exactly zero and the tendency keeps its bits"""
    K = 15
    x = AdvRig(named_mesh(mesh), K, device=False)
    wt = x.transport()
    assert_both_signs(wt, x.lo, x.hi, x.n_all)
    u = np.repeat(x.u[:, :1], K, axis=1)
    rng = np.random.default_rng(5)
    tend = rng.uniform(-1.0e-3, 1.0e-3, (x.e_size, K))
    got = VR.add_velocity_tend(tend.copy(), x.h, u, wt, x.coe, x.mask, x.lo_e, x.hi_e, x.e_all)
    assert np.array_equal(got, tend)
    sheared = VR.add_velocity_tend(tend.copy(), x.h, x.u, wt, x.coe, x.mask, x.lo_e, x.hi_e, x.e_all)
    assert not np.array_equal(sheared, tend)  # the term is there


def test_centred_interface_value_is_second_order():
    """A smooth profile sampled at the mid-depths of a smoothly stretched column: the order-2 interface value is the
    linear interpolant between the two mid-depths, so its error at the interface is (d1 d2 / 2) |phi''| with d1, d2 the
    half thicknesses -- it falls by 4 per doubling of the layer count, up to the next term of the expansion (relative
    size O(1/N): 7 % at N = 32).  Asserted: a ratio within 4 +- 0.5 over two doublings."""
    errs = []
    for n in (32, 64, 128):
        k = np.arange(n)
        h = 1.0 + 0.5 * np.sin(2.0 * np.pi * (k + 0.5) / n)
        h = h / h.sum()
        z_int = np.concatenate([[0.0], np.cumsum(h)])  # depth of the interfaces, top first
        z_mid = 0.5 * (z_int[:-1] + z_int[1:])
        phi = np.sin(3.0 * z_mid)
        top = VR.interface_value(h[None, :], phi[None, :], np.zeros((1, n)), 2, 1)[0]
        errs.append(np.abs(top[1:] - np.sin(3.0 * z_int[1:-1])).max())
    r1, r2 = errs[0] / errs[1], errs[1] / errs[2]
    print(f"interface value errors {errs}, ratios {r1:.3f} {r2:.3f}")
    assert 3.5 <= r1 <= 4.5 and 3.5 <= r2 <= 4.5


def test_upwind_interface_value_takes_the_donor_cell():
    h = np.ones((1, 4))
    phi = np.array([[1.0, 2.0, 3.0, 4.0]])
    wt = np.array([[0.0, 1.0, -1.0, 0.0]])
    top = VR.interface_value(h, phi, wt, 1, 1)[0]
    assert top[1] == 2.0  # upward through the top of level 1: the value of level 1
    assert top[2] == 2.0  # downward through the top of level 2: the value of level 1 above it
    assert top[3] == 3.0  # no transport: the upper value (Wt > 0.0 is false)
    with pytest.raises(ValueError):
        VR.interface_value(h, phi, wt, 3, 1)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("mesh", MESHES)
def test_masking(mesh, order):
    """NaN wherever a call must not write or read -- outside the ranges, on land, on rows >= N*All: the NaN stay
    where they were and nothing inside a range becomes NaN"""
    K, nt = 15, 3
    x = AdvRig(named_mesh(mesh), K, nt=nt, device=False)

    def seed(a, m):
        out = np.full(a.shape, np.nan)
        out[..., m] = a[..., m]
        return out

    e_active = np.zeros((x.e_size, K), bool)
    k = np.arange(K)[None, :]
    e_active[: x.e_all] = (k >= x.lo_e[: x.e_all, None]) & (k <= x.hi_e[: x.e_all, None])
    d, ref, h = seed(x.d, x.active), seed(x.ref, x.active), seed(x.h, x.active)
    tr, u = seed(x.tr, x.active), seed(x.u, e_active)
    wt = VR.vertical_transport(d, ref, x.w, x.lo, x.hi, x.n_all, np.full((x.n_size, K), np.nan))
    assert np.isfinite(wt[x.active]).all() and np.isnan(wt[~x.active]).all()
    assert_both_signs(wt, x.lo, x.hi, x.n_all)
    th = VR.add_thickness_tend(d.copy(), wt, x.lo, x.hi, x.n_all)
    assert np.isfinite(th[x.active]).all() and np.isnan(th[~x.active]).all()
    tt = VR.add_tracer_tend(seed(x.tr * 1.0e-3, x.active), h, tr, wt, x.lo, x.hi, x.n_all, order)
    assert np.isfinite(tt[:, x.active]).all() and np.isnan(tt[:, ~x.active]).all()
    ut = VR.add_velocity_tend(seed(x.u * 1.0e-2, e_active), h, u, wt, x.coe, x.mask, x.lo_e, x.hi_e, x.e_all)
    assert np.isfinite(ut[e_active]).all() and np.isnan(ut[~e_active]).all()
    if "coast" in mesh:
        assert (~x.active[: x.n_all]).all(axis=1).any()   # land columns
        assert (~e_active[: x.e_all]).all(axis=1).any()   # edges next to land
    assert (x.lo[: x.n_all] > 0).any()                    # KMin > 0
