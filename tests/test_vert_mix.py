"""VertMix without a device: the NumPy restatement (tests/vert_mix_reference.py) against quantities computed here
independently -- closed forms of N^2, S^2, Ri, viscosity and diffusivity on a column with linear profiles (the design
document's test cases), a dense solve of the backward-Euler system, conservation, and the limits of small and large
coefficients -- and the argument refusals that need no device."""
import numpy as np
import pytest

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests import vert_mix_reference as R
from tests.column_reference import RHO0

G = R.GRAVITY


# ---- one column of K layers in a cell with six edges: linear profiles in depth
class LinearColumn:
    """Cell 0 of a one-cell, six-edge 'mesh' (plus the sentinel row), K layers of thickness dz, ZMid linear; Un and Ut
    linear in depth on every edge, slopes a_e and b_e; linear EOS with T linear in depth, S uniform."""

    def __init__(self, K=12, dtdz=0.5, klo=0, khi=None):
        rng = np.random.default_rng(5)
        self.K, self.dz = K, 10.0
        khi = K - 1 if khi is None else khi
        self.lo, self.hi = np.array([klo, -1], np.int32), np.array([khi, -1], np.int32)
        self.zmid = np.zeros((2, K))
        self.zmid[0] = -(np.arange(K) + 0.5) * self.dz
        self.ne = np.array([6, 0], np.int32)
        self.eoc = np.array([[0, 1, 2, 3, 4, 5], [6] * 6], np.int32)
        self.dc = np.append(rng.uniform(2.0e4, 3.0e4, 6), 0.0)
        self.dv = np.append(rng.uniform(1.0e4, 2.0e4, 6), 0.0)
        self.area = np.array([2.5e9, 0.0])
        self.a = rng.uniform(-5.0e-2, 5.0e-2, 6)
        self.b = rng.uniform(-5.0e-2, 5.0e-2, 6)
        self.un, self.ut = np.zeros((7, K)), np.zeros((7, K))
        self.un[:6] = self.a[:, None] * self.zmid[0][None, :]
        self.ut[:6] = self.b[:, None] * self.zmid[0][None, :]
        # linear EOS (DRhoDT -0.2, DRhoDS 0.8, RhoT0S0 1000); T = 10 + dtdz * z (a steep gradient keeps the density
        # differences well above rounding: rtol 1e-12 holds); the displaced volume of a linear EOS
        # does not depend on pressure
        t = 10.0 + dtdz * self.zmid
        self.spec_vol = 1.0 / (1000.0 + (-0.2 * t + 0.8 * 35.0))
        self.spec_vol[1] = 0.0
        self.dtdz = dtdz

    # independent closed forms
    def n2(self):
        return (G / RHO0) * 0.2 * self.dtdz

    def s2(self):
        f = (0.5 * self.dc[:6]) * self.dv[:6] / self.area[0]
        return float(np.sum(f * (self.a ** 2 + self.b ** 2)))

    def mask(self):
        k = np.arange(self.K)
        return (k > self.lo[0]) & (k <= self.hi[0])

    def run(self, **cfg):
        n2 = R.bvf(self.spec_vol, self.spec_vol, self.zmid, self.lo, self.hi, 1, RHO0)
        visc, diff = R.coefficients(self.un, self.ut, n2, self.zmid, self.lo, self.hi, 1, self.ne, self.eoc, self.dc,
                                    self.dv, self.area, R.config(**cfg))
        return n2, visc, diff


@pytest.mark.parametrize("klo,khi", [(0, 11), (3, 9)])
def test_bvf_closed_form(klo, khi):
    col = LinearColumn(klo=klo, khi=khi)
    n2, _, _ = col.run()
    m = col.mask()
    assert np.allclose(n2[0, m], col.n2(), rtol=1e-12, atol=0.0)
    assert np.all(n2[0, ~m] == 0.0) and np.all(n2[1] == 0.0)
    assert col.n2() > 0.0  # T decreasing with depth: stable


@pytest.mark.parametrize("case", ["background", "shear", "convective", "combined"])
@pytest.mark.parametrize("klo,khi", [(0, 11), (2, 8)])
def test_design_document_cases(case, klo, khi):
    stable = case in ("background", "shear")
    col = LinearColumn(dtdz=0.5 if stable else -0.5, klo=klo, khi=khi)
    shear, conv = case in ("shear", "combined"), case in ("convective", "combined")
    nu_b, ka_b, nu0, alpha, kc = 1.0e-4, 1.0e-5, 0.005, 5.0, 1.0
    n2, visc, diff = col.run(EnableShearMix=shear, EnableConvectiveMix=conv)
    ri = max(col.n2() / col.s2(), 0.0)
    want_v, want_d = nu_b, ka_b
    if shear:
        want_v = nu_b + nu0 / (1.0 + alpha * ri) ** 2
        want_d = ka_b + want_v / (1.0 + alpha * ri)
    if conv and col.n2() < 0.0:
        want_v, want_d = want_v + kc, want_d + kc
    m = col.mask()
    assert np.allclose(visc[0, m], want_v, rtol=1e-12, atol=0.0)
    assert np.allclose(diff[0, m], want_d, rtol=1e-12, atol=0.0)
    for a in (visc, diff):  # the no-flux top interface, levels outside the range, the sentinel row
        assert np.all(a[0, ~m] == 0.0) and np.all(a[1] == 0.0)
    if case == "shear":
        assert 0.0 < ri < 10.0 and want_v > nu_b  # the shear term is exercised


def test_ri_clamp_and_convective_trigger():
    col = LinearColumn(dtdz=-0.5)  # unstable: N2 < 0
    assert col.n2() < 0.0
    _, visc, diff = col.run()
    m = col.mask()
    # Ri clamped to 0: D = 1, the full shear term, then the convective term
    assert np.allclose(visc[0, m], 1.0e-4 + 0.005 + 1.0, rtol=1e-12, atol=0.0)
    assert np.allclose(diff[0, m], 1.0e-5 + (1.0e-4 + 0.005) + 1.0, rtol=1e-12, atol=0.0)
    # a trigger below N2 switches the convective term off
    _, visc2, _ = col.run(ConvectiveTriggerBVF=2.0 * col.n2())
    assert np.allclose(visc2[0, m], 1.0e-4 + 0.005, rtol=1e-12, atol=0.0)


def test_integer_exponent_is_repeated_multiplication():
    d = np.random.default_rng(1).uniform(1.0, 50.0, 1000)
    assert np.array_equal(R.shear_pow(d, 3.0), (d * d) * d)
    assert np.allclose(R.shear_pow(d, 1.5), d ** 1.5, rtol=1e-15)


# ---- the column solves
def _columns(n, ncols, seed, kappa_scale=1.0e-2):
    rng = np.random.default_rng(seed)
    h = rng.uniform(0.5, 40.0, (ncols, n))
    coef = rng.uniform(0.0, kappa_scale, (ncols, n))
    phi = rng.uniform(-2.0, 30.0, (ncols, n))
    return h, coef, phi


@pytest.mark.parametrize("n", [1, 2, 3, 7, 37, 80])
def test_solve_matches_dense_solve(n):
    h, coef, phi = _columns(n, 5, n)
    g, hh, x = R.assemble(h, coef, phi, 3600.0)
    assert np.allclose(R.pcr_diff(g, hh, x), R.dense_solve(g, hh, x), rtol=1e-11, atol=0.0)


def _one_cell_mesh_arrays(K, n_cells=6, seed=3):
    """a small set of cells (plus the sentinel row) with varied ranges, for the array-level functions"""
    rng = np.random.default_rng(seed)
    h = np.zeros((n_cells + 1, K))
    h[:n_cells] = rng.uniform(0.5, 40.0, (n_cells, K))
    lo = np.array([0, 3, 0, 5, 0, 2, -1], np.int32)
    hi = np.array([K - 1, K - 1, 2, 5, K - 1, K - 4, -1], np.int32)
    hi[4] = -1  # land
    return rng, h, lo, hi


def test_tracer_mix_against_dense_and_conservation():
    K, nt, dt = 20, 3, 1800.0
    rng, h, lo, hi = _one_cell_mesh_arrays(K)
    kappa = rng.uniform(0.0, 5.0e-2, h.shape)
    tr = rng.uniform(-2.0, 30.0, (nt, h.shape[0], K))
    out = R.tracer_mix(h, kappa, tr, nt, dt, lo, hi, 6)
    for c in range(6):
        if not (0 <= lo[c] <= hi[c] < K):
            assert np.array_equal(out[:, c], tr[:, c])
            continue
        k = np.arange(lo[c], hi[c] + 1)
        outside = np.setdiff1d(np.arange(K), k)
        assert np.array_equal(out[:, c, outside], tr[:, c, outside])
        for t in range(nt):
            g, hh, x = R.assemble(h[c, k][None], kappa[c, k][None], tr[t, c, k][None], dt)
            assert np.allclose(out[t, c, k], R.dense_solve(g, hh, x)[0], rtol=1e-11, atol=0.0)
            before, after = np.sum(h[c, k] * tr[t, c, k]), np.sum(h[c, k] * out[t, c, k])
            assert after == pytest.approx(before, rel=1e-13, abs=0.0)
    assert np.array_equal(out[:, 6], tr[:, 6])


def test_velocity_mix_against_dense():
    K, dt = 16, 900.0
    rng, h, lo, hi = _one_cell_mesh_arrays(K)
    visc = rng.uniform(0.0, 5.0e-2, h.shape)
    cells_on_edge = np.array([[0, 1], [1, 2], [2, 3], [0, 5], [3, 4], [0, 6], [6, 6]], np.int32)
    elo = np.array([3, 3, 5, 2, 6, 18, 18], np.int32)
    ehi = np.array([K - 1, 2, 2, K - 4, -1, -1, -1], np.int32)
    u = rng.uniform(-1.0, 1.0, (7, K))
    out = R.velocity_mix(h, visc, u, dt, cells_on_edge, elo, ehi, 6)
    for e in range(6):
        if not (0 <= elo[e] <= ehi[e] < K):
            assert np.array_equal(out[e], u[e])
            continue
        k = np.arange(elo[e], ehi[e] + 1)
        c1, c2 = cells_on_edge[e]
        he = 0.5 * (h[c1, k] + h[c2, k])
        nue = 0.5 * (visc[c1, k] + visc[c2, k])
        g, hh, x = R.assemble(he[None], nue[None], u[e, k][None], dt)
        assert np.allclose(out[e, k], R.dense_solve(g, hh, x)[0], rtol=1e-11, atol=0.0)
        assert np.sum(he * out[e, k]) == pytest.approx(np.sum(he * u[e, k]), rel=1e-13, abs=0.0)
    assert np.array_equal(out[6], u[6])


@pytest.mark.parametrize("n", [2, 5, 37, 80])
def test_uniform_column_stays_uniform(n):
    h, coef, _ = _columns(n, 4, 11)  # G of order H: the elimination stays well conditioned
    phi = np.full_like(h, 13.25)
    g, hh, x = R.assemble(h, coef, phi, 3600.0)
    out = R.pcr_diff(g, hh, x)
    assert np.max(np.abs(out - 13.25)) <= 8 * np.spacing(13.25)


@pytest.mark.parametrize("n", [1, 4, 37, 80])
def test_zero_coefficients_leave_the_field(n):
    h, _, phi = _columns(n, 4, 12)
    g, hh, x = R.assemble(h, np.zeros_like(h), phi, 3600.0)
    out = R.pcr_diff(g, hh, x)
    assert np.all(np.abs(out - phi) <= np.spacing(np.abs(phi)))


@pytest.mark.parametrize("n", [2, 9, 37, 80])
def test_large_coefficients_homogenise_the_column(n):
    h, _, phi = _columns(n, 4, 13)
    g, hh, x = R.assemble(h, np.full_like(h, 1.0e14), phi, 1.0)  # the reference's stability value
    out = R.pcr_diff(g, hh, x)
    assert np.all(np.isfinite(out))
    mean = np.sum(h * phi, axis=1) / np.sum(h, axis=1)
    # G / H ~ 1e12: the 2x2 determinants cancel about twelve digits, so the mean holds to ~1e-5 at worst (n = 2);
    # without mixing the column would spread over tens of percent
    assert np.allclose(out, mean[:, None], rtol=1e-4, atol=0.0)
    assert np.all(np.ptp(phi, axis=1) > 1.0)


# ---- refusals that need no device
def _host_only_mesh(K=8):
    gm = oa.GlobalMesh(planar_hex(8, 8, 1.0))
    d = oa.Decomp(gm, 1, 0, 3)
    return gm, d, oa.HorzMesh(d, K, host_only=True)


@pytest.mark.parametrize("field", ["BackgroundViscosity", "BackgroundDiffusivity", "ShearNuZero",
                                   "ConvectiveDiffusivity"])
def test_negative_coefficients_are_refused(field):
    gm, d, m = _host_only_mesh()
    with pytest.raises(oa.OmegaAmdError, match=f"{field}.*negative"):
        oa.VertMix(m, None, **{field: -1.0e-6})


def test_too_many_layers_and_host_only_mesh_are_refused():
    gm, d, m = _host_only_mesh(K=1025)
    with pytest.raises(oa.OmegaAmdError, match="1024"):
        oa.VertMix(m, None)
    gm, d, m = _host_only_mesh(K=8)
    with pytest.raises(oa.OmegaAmdError, match="host-only"):
        oa.VertMix(m, None)


def test_config_defaults_and_unknown_fields():
    c = oa.vertmix_config()
    for k, v in R.DEFAULTS.items():
        assert getattr(c, k) == v, k
    assert oa.vertmix_config(ShearExponent=3.0).ShearExponent == 3.0
    with pytest.raises(KeyError):
        oa.vertmix_config(ShearExponet=3.0)
