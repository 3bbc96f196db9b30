"""Redi without a device: the NumPy restatement of the contract (tests/redi_reference.py) against what isoneutral
diffusion must give -- bounded slopes that vanish at the top of every edge column, finite answers in unstable and
unstratified water and between identical columns, exact zeros (and the plain along-layer diffusion, bit for bit) where
the layers are the isopycnals, a non-negative implicit diffusivity, conservation to a derived rounding bound, and the
isoneutral property itself: no flux of density along a tilted isopycnal, horizontally or vertically -- plus the refusals
that need no device."""
from fractions import Fraction

import numpy as np
import pytest

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests import column_reference as CR
from tests import redi_reference as RR
from tests.column_reference import RHO0
from tests.meshes import named_mesh
from tests.rank_rig import RankRig
from tests.vert_fixtures import mix_inputs

U = np.finfo(np.float64).eps / 2  # the unit roundoff 2^-53
MESHES = ("hex24x20", "fib300_coast_ragged")


class Host(RankRig):
    """One rank's host-only mesh, its layer ranges and the mesh tables of the cell sweeps; the column fields either
    from the column restatement (tests/column_reference.py, with the displaced volume) or given."""

    def __init__(self, g, K, min_level=None, max_level=None):
        super().__init__(g, K, device=False)
        self.layers(min_level, max_level)
        self.t = RR.tables(self.mesh)
        self.coe, self.dc = self.t["CellsOnEdge"], self.t["DcEdge"]
        self.kappa = np.full(self.e_size, RR.REDI_KAPPA)

    def column(self, h, ct, sa, bot, eos_kind, ps=None):
        n, K = self.n_size, self.K
        st = {"PressureInterface": np.full((n, K + 1), np.nan), "PressureMid": np.full((n, K), np.nan),
              "ZInterface": np.full((n, K + 1), np.nan), "ZMid": np.full((n, K), np.nan),
              "GeopotentialMid": np.full((n, K), np.nan), "SpecVol": np.full((n, K), np.nan),
              "SpecVolDisplaced": np.full((n, K), np.nan)}
        ps = np.full(n, 1.01325e5) if ps is None else ps
        CR.column_sequence(h, ct, sa, ps, None, None, bot, self.lo, self.hi, self.n_all, RHO0, eos_kind, st, 1)
        self.fields(h, st["SpecVol"], st["SpecVolDisplaced"], st["ZMid"])

    def fields(self, h, sv, svd, zmid):
        self.h, self.sv, self.svd, self.zmid = h, sv, svd, zmid

    def slope(self, **kw):
        """SlopeInterface, NaN wherever the contract writes nothing"""
        s = np.full((self.e_size, self.K), np.nan)
        return RR.slope(self.h, self.sv, self.svd, self.zmid, self.coe, self.dc, self.lo_e, self.hi_e, self.e_all, RHO0, s,
                        **kw)

    def tend(self, tracers, slope, tend=None, diag=None):
        nt = len(tracers)
        tend = np.zeros((nt, self.n_size, self.K)) if tend is None else tend
        return RR.add_tracer_tend(tend, self.h, tracers, nt, self.zmid, slope, self.kappa, self.t, self.lo, self.hi,
                                  self.lo_e, self.hi_e, diag)

    def vert_diffusivity(self, slope, vert_diff=None):
        out = np.full((self.n_size, self.K), np.nan)
        return RR.vert_diffusivity(out, vert_diff, slope, self.kappa, self.t, self.lo, self.hi, self.lo_e, self.hi_e)


def _random(mesh, K, eos_kind="teos10", seed=7):
    g = named_mesh(mesh)
    n = int(g["nCells"])
    G = mix_inputs(g, K, seed, False, 2)
    x = Host(g, K, G["min_level"], G["max_level"])
    rng = np.random.default_rng(seed + 100)
    x.column(x.cells(G["h"]), x.cells(G["tr"][0]), x.cells(G["tr"][1]), x.cells(rng.uniform(100.0, 6000.0, n)), eos_kind,
             ps=x.cells(rng.uniform(0.9e5, 1.1e5, n)))
    x.tr = x.cells(G["tr"])
    return x


def _front(K=8, dtdz=-1.5, dtdx=-0.05 / 30.0e3):
    """hex24x20, every layer active, linear Eos: T = 20 + dtdz * k + dtdx * x (per layer, per metre), S uniform"""
    g = named_mesh("hex24x20")
    x = Host(g, K)
    xc = x.cells(g["xCell"])[:, None]
    ct = 20.0 + dtdz * np.arange(K)[None, :] + dtdx * xc
    x.column(np.full((x.n_size, K), 50.0), ct, np.full((x.n_size, K), 35.0), np.full(x.n_size, 50.0 * K), "linear")
    x.tr = np.stack([ct, np.full((x.n_size, K), 35.0)])
    return x


@pytest.mark.parametrize("eos_kind", ["teos10", "linear"])
@pytest.mark.parametrize("K", [5, 16])
@pytest.mark.parametrize("mesh", MESHES)
def test_slopes_are_bounded_and_zero_at_the_top(mesh, K, eos_kind):
    x = _random(mesh, K, eos_kind)
    s = x.slope()
    assert np.isnan(s[~x.e_active]).all() and np.isfinite(s[x.e_active]).all()  # nothing outside the ranges
    assert np.abs(s[x.e_active]).max() <= RR.SLOPE_MAX
    wet = np.nonzero(x.e_active.any(axis=1))[0]
    assert len(wet) > 0 and np.all(s[wet, x.lo_e[wet]] == 0.0)
    # random columns are steep: both clips occur, and so do slopes inside them
    inner = s[x.e_active]
    assert (inner == RR.SLOPE_MAX).any() and (inner == -RR.SLOPE_MAX).any()
    gentle = x.slope(slope_max=1.0e30)
    assert (np.abs(gentle[x.e_active]) > RR.SLOPE_MAX).any()
    d = x.vert_diffusivity(s)[0]
    _, faces = RR.cell_mask(x.lo, x.hi, x.n_all, K)
    assert np.isnan(d[: x.n_all][~faces]).all() and np.isnan(d[x.n_all:]).all()
    assert faces.any() and np.all(d[: x.n_all][faces] >= 0.0) and d[: x.n_all][faces].max() > 0.0  # VertDiffusivity >= 0


@pytest.mark.parametrize("dtdz", [1.5, 0.0], ids=["unstable", "unstratified"])
def test_unstable_and_unstratified_columns_are_finite(dtdz):
    """N2 <= 0 everywhere: N2E is clipped to 0 and the floor alone divides; the slopes are the clip's"""
    x = _front(dtdz=dtdz)
    for s in RR.edge_systems(x.h, x.sv, x.svd, x.zmid, x.coe, x.dc, x.kappa, x.lo_e, x.hi_e, x.e_all, RHO0, 1.0):
        assert all((n2 <= 0.0).all() for n2 in s["n2_cells"]) and np.all(s["n2_e"] == 0.0)
    s = x.slope()
    assert x.e_active[: x.e_all].all() and np.isfinite(s[: x.e_all]).all()
    assert np.abs(s[: x.e_all]).max() == RR.SLOPE_MAX
    tend = x.tend(x.tr, s)
    d = x.vert_diffusivity(s)[0]
    assert np.isfinite(tend[:, : x.n_all]).all() and np.isfinite(d[: x.n_all, 1:]).all()
    assert np.abs(tend[0, : x.n_all]).max() > 0.0


@pytest.mark.parametrize("eos_kind", ["teos10", "linear"])
def test_identical_columns_are_finite_and_flat(eos_kind):
    """flat bottom, h, T, S uniform across the cells, stratified: GradRho and GradZ are exact zeros, so are the slopes"""
    K = 12
    x = Host(planar_hex(12, 10, 30.0e3, bottom_depth=800.0), K)
    k = np.arange(K)
    ones = np.ones((x.n_size, 1))
    ct, sa = ones * (18.0 - 1.3 * k), ones * (34.0 + 0.11 * k)
    x.column(ones * (20.0 + 7.5 * k), ct, sa, np.full(x.n_size, 800.0), eos_kind)
    s = x.slope()
    assert np.all(s[: x.e_all] == 0.0) and np.isnan(s[x.e_all:]).all()
    tend = x.tend(np.stack([ct, sa]), s)
    assert np.all(tend[:, : x.n_all] == 0.0)
    assert np.all(x.vert_diffusivity(s)[0][: x.n_all, 1:] == 0.0)


@pytest.mark.parametrize("mesh", MESHES)
def test_layers_along_the_isopycnals_give_the_plain_diffusion(mesh):
    """Density a function of the layer index only, ZMid level-uniform: every GradRho and GradZ is an exact zero, so
    every slope and VertDiffusivity is, and the tendency is the divergence of Kappa * hE * GradPhi along the layers --
    formed here on its own, in the contract's order -- bit for bit."""
    K = 9
    g = named_mesh(mesh)
    G = mix_inputs(g, K, 11, False, 2)
    x = Host(g, K, G["min_level"], G["max_level"])
    rng = np.random.default_rng(5)
    ones = np.ones((x.n_size, 1))
    rho = 1024.0 + np.cumsum(rng.uniform(0.01, 0.3, K))[None, :] * ones
    disp = rho + 0.25 * np.diff(rho, axis=1, append=rho[:, -1:] + 0.1)
    z = -np.cumsum(rng.uniform(5.0, 30.0, K))[None, :] * ones
    x.fields(x.cells(G["h"]), 1.0 / rho, 1.0 / disp, z)
    x.kappa = rng.uniform(100.0, 900.0, x.e_size)
    s = x.slope()
    assert np.all(s[x.e_active] == 0.0) and x.e_active.any()
    d = x.vert_diffusivity(s)[0]
    _, faces = RR.cell_mask(x.lo, x.hi, x.n_all, K)
    assert np.all(d[: x.n_all][faces] == 0.0)
    tr = x.cells(G["tr"])
    tend = x.tend(tr, s)
    t, n = x.t, x.n_all
    kk = np.arange(K)[None, :]
    want = np.zeros((2, x.n_size, K))
    for tracer in range(2):
        acc = np.zeros((n, K))
        for j in range(t["MaxEdges"]):
            e = np.where(j < t["NEdgesOnCell"][:n], t["EdgesOnCell"][:n, j], 0)
            m = (j < t["NEdgesOnCell"][:n])[:, None] & x.e_active[e] & x.active[:n]
            c0, c1 = x.coe[e, 0][:, None], x.coe[e, 1][:, None]
            he = 0.5 * (x.h[c0, kk] + x.h[c1, kk])
            grad = (tr[tracer][c1, kk] - tr[tracer][c0, kk]) * (1.0 / x.dc[e])[:, None]
            flux = (x.kappa[e][:, None] * he) * grad
            acc = np.where(m, acc - t["EdgeSignOnCell"][:n, j][:, None] * (t["DvEdge"][e][:, None] * flux), acc)
        want[tracer, :n] = acc * (1.0 / t["AreaCell"][:n])[:, None]
    assert np.array_equal(tend[:, :n][:, x.active[:n]], want[:, :n][:, x.active[:n]])
    assert np.all(tend[:, ~x.active] == 0.0) and np.abs(tend).max() > 0.0


@pytest.mark.parametrize("mesh,K", [("hex24x20", 5), ("fib300_coast_ragged", 5), ("fib300_coast_ragged", 16)])
def test_the_domain_integral_is_conserved(mesh, K):
    """sum_c AreaCell[c] sum_K Tend[c][K] on a one-rank mesh (every edge sees both its cells), the products and the
    sum taken exactly (rationals), Tend added to zeros.

    Exactly, the integral is zero: the two cells of an edge form FluxE, and fl(DvEdge * FluxE), from the same operands
    in the same order, so the two terms t_J = EdgeSignOnCell * fl(DvEdge * FluxE) are exact negatives of each other;
    and layer K's WTop is, bit for bit, layer K-1's WBot (the same slots in the same order on the same operands), 0 at
    the top of the column as WBot is at its bottom.  What is left are the roundings on the way from these terms to
    Tend[c][K] = fl(fl(Acc * InvA) + fl(WTop - WBot)), with u = 2^-53 and S1 = sum_J |t_J| over the n_e slots that hold K:
      - Acc is a running sum of n_e terms from 0.0: the first addition is exact, each of the n_e - 1 others rounds a
        partial sum no larger than S1:                                                  (n_e - 1) u S1
      - InvA = fl(1 / AreaCell) and the product fl(Acc * InvA): AreaCell * fl(Acc * InvA) = Acc (1 + d1)(1 + d2), with
        |Acc| <= S1 (1 + (n_e - 1) u):                                                   2 u S1
      - Y = fl(WTop - WBot): the difference of the exact values, which telescope, is off by  u |Y|  per layer
      - the last addition rounds Tend itself:                                            u |Tend|
    so  |integral| <= u sum_{c,K} ((n_e + 1) S1 + AreaCell (|Y| + |Tend|)), up to second order (the factor 1 + 1e-6).
    The slot count n_e is taken at its largest, NEdgesOnCell[c]."""
    x = _random(mesh, K)
    s = x.slope()
    diag = []
    tend = x.tend(x.tr, s, diag=diag)
    area, n = x.t["AreaCell"], x.n_all
    for tracer, d in enumerate(diag):
        s1 = np.zeros((n, K))
        for m, flux, slot in d["fluxes"]:
            s1 += np.where(m, np.abs(slot["dv"] * flux), 0.0)
        y = d["wtop"] - d["wbot"]
        ne = x.t["NEdgesOnCell"][:n][:, None]
        per = (ne + 1) * s1 + area[:n, None] * (np.abs(y) + np.abs(tend[tracer, :n]))
        bound = U * float(per[d["layers"]].sum()) * (1.0 + 1.0e-6)
        total = Fraction(0)
        for c, kk in zip(*np.nonzero(d["layers"])):
            total += Fraction(float(area[c])) * Fraction(float(tend[tracer, c, kk]))
        err = abs(float(total))
        print(f"{mesh} K {K} tracer {tracer}: |integral| = {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
        assert bound > 0.0 and err <= bound
        assert np.abs(tend[tracer, :n][d["layers"]]).max() > 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the isoneutral property
# ---------------------------------------------------------------------------------------------------------------------
ISO_K, ISO_H, ISO_A, ISO_B, ISO_RHO1 = 6, 8.0, 2.0 ** -20, 2.0 ** -10, 1024.0


def _exact_spec_vol(rho):
    """SpecVol with 1.0 / SpecVol == rho exactly: near 1024 the doubles of 1 / rho lie twice as densely as those of rho,
    so one of fl(1 / rho) and its neighbours inverts to rho"""
    sv = 1.0 / rho
    for cand in (sv, np.nextafter(sv, 0.0), np.nextafter(sv, 1.0)):
        hit = (1.0 / cand) == rho
        sv = np.where(hit & ((1.0 / sv) != rho), cand, sv)
    assert np.all(1.0 / sv == rho)
    return sv


def _tilted():
    """planar hex 24 x 20 (dc = 30 km), flat uniform layers of 8 m, rho = rho1 + a x - b z with a = 2^-20, b = 2^-10
    (a / b = 2^-10 < SlopeMax), SpecVolDisplaced[K-1] = SpecVol[K-1], an integer Kappa per edge.  x is a multiple of
    dc / 2 and z of 4 m, so every density is a dyadic number held exactly, 1 / SpecVol returns it exactly, and every
    density difference is exact."""
    K = ISO_K
    g = named_mesh("hex24x20")
    x = Host(g, K)
    xc = x.cells(g["xCell"])
    assert np.all(xc == np.round(xc / 15.0e3) * 15.0e3)
    z = -(np.arange(K) + 0.5) * ISO_H
    rho = ISO_RHO1 + (ISO_A * xc)[:, None] - (ISO_B * z)[None, :]
    for c in (0, 7, x.n_all - 1):  # held exactly
        assert Fraction(float(rho[c, 3])) == Fraction(ISO_RHO1) + Fraction(ISO_A) * Fraction(float(xc[c])) - Fraction(ISO_B) * Fraction(float(z[3]))
    sv = _exact_spec_vol(rho)
    x.fields(np.full((x.n_size, K), ISO_H), sv, sv.copy(), np.ones((x.n_size, 1)) * z[None, :])
    x.kappa = np.random.default_rng(3).integers(300, 901, x.e_size).astype(np.float64)
    x.rho = rho
    # interior: an edge whose two cells are neighbours in x as they are in the mesh (not across the period), a cell
    # whose six edges are
    dx = xc[x.coe[: x.e_all, 1]] - xc[x.coe[: x.e_all, 0]]
    x.e_inner = np.zeros(x.e_size, bool)
    x.e_inner[: x.e_all] = np.abs(dx) <= 30.0e3
    x.c_inner = x.e_inner[x.t["EdgesOnCell"][: x.n_all]].all(axis=1)
    assert x.e_inner.sum() > 0.8 * x.e_all and x.c_inner.sum() > 0.8 * x.n_all
    return x


def test_no_density_flux_along_a_tilted_isopycnal():
    """The tracer is the density.  With the inputs of _tilted every step of the slope is exact but two: on an interior
    edge G = GradRho = GradPhi (the same bits), GradZ = 0, RhoZE = PhiZE = -b and N2E = GR b exactly, so
    SRel = fl(fl(GR * G) / (GR b)) = (G / b)(1 + d1)(1 + d2), Up = Dn = SRel * (-b) = -G (1 + d1)(1 + d2) exactly (b is a
    power of two), 0.5 * (Up + Dn) = Up, and GradPhi + Up = -G ((1 + d1)(1 + d2) - 1) is an exact difference:
      |FluxE| <= (Kappa hE) |G| (2 u + u^2), one more rounding for the product, |G| <= |a| (1 + 2 u)
    -- two roundings, eps = 2 u:  |FluxE| <= eps * Kappa * hE * |a|, up to second order (the factor 1 + 1e-6).  The plain
    along-layer flux Kappa hE GradPhi of the same tracer is at least Kappa hE |a| / 2 there, and with Kappa varying from
    edge to edge its divergence, the plain Laplacian tendency, does not vanish either."""
    x = _tilted()
    K = x.K
    s = x.slope()
    inner = x.e_inner[: x.e_all]
    assert np.all(np.abs(s[: x.e_all][inner][:, 1:]) <= (ISO_A / ISO_B) * (1 + 8 * U))  # unclipped: |n_x| a / b
    assert np.abs(s[: x.e_all][inner][:, 1:]).min() >= 0.5 * (ISO_A / ISO_B) * (1 - 8 * U)
    diag = []
    tend = x.tend(x.rho[None], s, diag=diag)
    worst, checked, plain_min = 0.0, 0, np.inf
    kk = np.arange(K)[None, :]
    for m, flux, slot in diag[0]["fluxes"]:
        e = slot["e"][:, 0]
        sel = m & x.e_inner[e][:, None] & (kk >= 1) & (kk <= K - 2)  # interior layers Lo+1 .. Hi-1 of interior edges
        bound = (2 * U) * slot["kappa"] * ISO_H * ISO_A * (1.0 + 1.0e-6)
        ratio = np.abs(flux) / bound
        assert np.all(ratio[sel] <= 1.0)
        worst, checked = max(worst, ratio[sel].max()), checked + int(sel.sum())
        plain = (slot["kappa"] * ISO_H) * ((x.rho[slot["c1"], kk] - x.rho[slot["c0"], kk]) * slot["inv_dc"])
        plain_min = min(plain_min, np.abs(plain[sel]).min())
    print(f"worst |FluxE| / (eps Kappa hE |a|) = {worst:.3e} over {checked} edge-layers; least plain flux "
          f"{plain_min:.3e}")
    assert checked > 0 and plain_min >= 0.49 * 300.0 * ISO_H * ISO_A
    # the plain Laplacian tendency of the same tracer (zero slopes) does not vanish on the same cells and layers
    lap = x.tend(x.rho[None], np.zeros_like(s))
    cells = np.nonzero(x.c_inner)[0]
    # (an integer Kappa can balance around a single cell by chance: the median over the cells, not the least)
    horizontal = diag[0]["acc"] * (1.0 / x.t["AreaCell"][: x.n_all])[:, None]  # the isoneutral flux's divergence
    assert np.median(np.abs(lap[0][cells][:, 1: K - 1])) > 1.0e6 * np.abs(horizontal[cells][:, 1: K - 1]).max()
    assert np.isfinite(tend[0][: x.n_all]).all()


def test_no_vertical_density_flux_across_a_tilted_isopycnal():
    """W[K] + VertDiffusivity[K] * PhiZ_c[K] on the interior interfaces of interior cells: the explicit cross flux
    W = sum_J F_J ((Kappa S_J) GInt_J) against the implicit S.S flux.  With the inputs of _tilted GInt_J = G_J and
    PhiZ_c = -b exactly, S_J = (G_J / b)(1 + d1)(1 + d2), so term by term F_J Kappa S_J (G_J - S_J b) is
    2 u F_J Kappa |S_J| |G_J| at most; the two sums add three roundings per term each (Kappa * S, * GInt, F_J *; S * S,
    Kappa *, F_J *) and n_e - 1 = 5 roundings of partial sums each, the product with the power of two b none, and the
    last addition one: 2 + 3 + 3 + 2 * 5 + 1 = 19 roundings of terms bounded by F_J Kappa (a / b) |a|, where
    sum_J F_J = 2 on a regular hexagon and Kappa <= 900:
      |W + VertDiffusivity * PhiZ| <= 19 u * 2 * 900 * (a / b) * |a|, up to second order (the factor 1 + 1e-6)."""
    x = _tilted()
    K = x.K
    s = x.slope()
    diag = []
    x.tend(x.rho[None], s, diag=diag)
    d = x.vert_diffusivity(s)[0]
    w = diag[0]["wtop"]
    cells = np.nonzero(x.c_inner)[0]
    assert np.allclose(sum(slot["f"][cells] for _, _, slot in diag[0]["fluxes"]), 2.0, rtol=1.0e-12)
    resid = w[cells][:, 1:] + d[cells][:, 1:] * (-ISO_B)
    bound = 19 * U * 2.0 * 900.0 * (ISO_A / ISO_B) * ISO_A * (1.0 + 1.0e-6)
    worst = np.abs(resid).max() / bound
    print(f"worst |W + VertDiffusivity PhiZ| / bound = {worst:.3e}; max |W| = {np.abs(w[cells][:, 1:]).max():.3e}")
    assert worst <= 1.0
    assert np.abs(w[cells][:, 1:]).min() > 1.0e6 * bound  # each part alone is far from zero


def test_refusals_without_a_device():
    """through the C ABI: the parameters are checked before the mesh is looked at; a host-only mesh is refused"""
    x = Host(planar_hex(6, 4, 30.0e3), 4)
    with pytest.raises(oa.OmegaAmdError, match="host-only"):
        oa.Redi(x.mesh, None, None, 2)
    for kappa in (-1.0, np.nan, np.inf):
        with pytest.raises(oa.OmegaAmdError, match="RediKappa"):
            oa.Redi(x.mesh, None, None, 2, kappa=kappa)
    for v in (0.0, -0.01, np.nan, np.inf):
        with pytest.raises(oa.OmegaAmdError, match="SlopeMax"):
            oa.Redi(x.mesh, None, None, 2, slope_max=v)
        with pytest.raises(oa.OmegaAmdError, match="N2Floor"):
            oa.Redi(x.mesh, None, None, 2, n2_floor=v)
    with pytest.raises(oa.OmegaAmdError, match="MaxTracers"):
        oa.Redi(x.mesh, None, None, 0)
