"""GentMcWilliams without a device: the NumPy restatement of the contract (tests/gent_mcwilliams_reference.py) on column
fields from tests/column_reference.py, against what the boundary-value problem must give -- the solution of the
un-premultiplied system by a dense solve, exact zeros between identical columns and where Kappa is zero, a bolus flow
that flattens the front, a column transport that telescopes to zero, finite answers in unstable and unstratified water
-- plus the refusals that need no device."""
from fractions import Fraction

import numpy as np
import pytest

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests import column_reference as CR
from tests import gent_mcwilliams_reference as GR
from tests import pressure_grad_reference as PR
from tests.column_reference import RHO0
from tests.meshes import named_mesh
from tests.vert_fixtures import mix_inputs

EPS = np.finfo(np.float64).eps
KAPPA, SPEED = 600.0, 0.3


class Host:
    """One rank's host-only mesh in the library's local order, the layer ranges of cells and edges, and the column
    fields of given h, T, S through the column restatement with the displaced volume (NaN outside every column's
    active range)."""

    def __init__(self, g, K, min_level=None, max_level=None):
        self.K = K
        self.gm = oa.GlobalMesh(g)
        self.decomp = oa.Decomp(self.gm, 1, 0, 3)
        self.mesh = m = oa.HorzMesh(self.decomp, K, host_only=True)
        self.nc_all, self.nc_size, self.ne_all, self.ne_size = m.NCellsAll, m.NCellsSize, m.NEdgesAll, m.NEdgesSize
        self.cid = self.decomp.get_array("CellID")
        self.coe, self.dc = m.get_array("CellsOnEdge"), m.get_array("DcEdge")
        self.lo_c, self.hi_c = CR.local_layer_ranges(self.cid, min_level, max_level, self.nc_all, self.nc_size, K)
        self.lo, self.hi = PR.edge_ranges(self.coe, self.ne_all, self.lo_c, self.hi_c, K)
        self.in_range = np.zeros((self.ne_size, K), bool)
        self.in_range[: self.ne_all] = PR.range_mask(self.lo, self.hi, self.ne_all, K)
        self.kappa = np.full(self.ne_size, KAPPA)

    def cells(self, glob):
        """a global per-cell array in local order, zero on the sentinel row"""
        glob = np.asarray(glob, dtype=np.float64)
        out = np.zeros((self.nc_size,) + glob.shape[1:])
        out[: self.nc_all] = glob[self.cid[: self.nc_all] - 1]
        return out

    def column(self, h, ct, sa, bot, eos_kind, ps=None, linear=(-0.2, 0.8, 1000.0)):
        n, K = self.nc_size, self.K
        st = {"PressureInterface": np.full((n, K + 1), np.nan), "PressureMid": np.full((n, K), np.nan),
              "ZInterface": np.full((n, K + 1), np.nan), "ZMid": np.full((n, K), np.nan),
              "GeopotentialMid": np.full((n, K), np.nan), "SpecVol": np.full((n, K), np.nan),
              "SpecVolDisplaced": np.full((n, K), np.nan)}
        ps = np.full(n, 1.01325e5) if ps is None else ps
        CR.column_sequence(h, ct, sa, ps, None, None, bot, self.lo_c, self.hi_c, self.nc_all, RHO0, eos_kind, st, 1,
                           linear)
        self.h, self.st = h, st
        return st

    def args(self):
        st = self.st
        return (self.h, st["SpecVol"], st["SpecVolDisplaced"], st["ZMid"], self.coe, self.dc, self.kappa, self.lo,
                self.hi, self.ne_all, RHO0, SPEED)

    def systems(self):
        return list(GR.edge_systems(*self.args()))

    def bolus(self, transport=None):
        """(BolusVelocity, StreamFunction), NaN wherever the contract writes nothing"""
        u, psi = np.full((self.ne_size, self.K), np.nan), np.full((self.ne_size, self.K), np.nan)
        GR.bolus_velocity(*self.args(), u, psi, transport)
        return u, psi


def _random(mesh, K, eos_kind="teos10", seed=7):
    g = named_mesh(mesh)
    n = int(g["nCells"])
    G = mix_inputs(g, K, seed, False, 2)
    x = Host(g, K, G["min_level"], G["max_level"])
    rng = np.random.default_rng(seed + 100)
    x.column(x.cells(G["h"]), x.cells(G["tr"][0]), x.cells(G["tr"][1]), x.cells(rng.uniform(100.0, 6000.0, n)), eos_kind,
             ps=x.cells(rng.uniform(0.9e5, 1.1e5, n)))
    return x


# Largest max_i |Psi_pcr - Psi_dense| / max_i |Psi_dense| over the columns of the four cases below, as measured: 1.077e-15
# (hex24x20, K = 5), 2.532e-15 (hex24x20, K = 16), 7.946e-16 and 1.109e-15 (fib300_coast_ragged, K = 5 and 16), with
# condition numbers up to 2.5e+02.  The dense solve's own error scales with the condition number of the column, which
# varies with the ragged ranges, so the bound is the largest figure times 10.
DENSE_MEASURED = 2.532e-15
DENSE_FACTOR = 10.0


@pytest.mark.parametrize("K", [5, 16])
@pytest.mark.parametrize("mesh", ["hex24x20", "fib300_coast_ragged"])
def test_against_an_independent_dense_solve(mesh, K):
    """the restatement's PCR solve of the premultiplied diffusion form against numpy.linalg.solve on the
    un-premultiplied general system (tests/gent_mcwilliams_reference.py: dense_solve)"""
    x = _random(mesh, K)
    _, psi = x.bolus()
    worst, worst_cond, rows = 0.0, 0.0, 0
    for s in x.systems():
        if s["he"].shape[1] < 2:
            continue
        want, cond = GR.dense_solve(s)
        got = psi[s["es"][:, None], s["k"][:, 1:]]
        assert np.isfinite(got).all() and np.isfinite(want).all()
        rel = np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)
        worst, worst_cond, rows = max(worst, rel.max()), max(worst_cond, cond.max()), rows + got.size
    print(f"{mesh} K {K}: max relative |Psi - dense| = {worst:.3e} over {rows} rows, largest condition number "
          f"{worst_cond:.3e}")
    assert rows > 0
    assert worst <= DENSE_FACTOR * DENSE_MEASURED  # measured: at most 2.532e-15 (DENSE_MEASURED above)


@pytest.mark.parametrize("eos_kind", ["teos10", "linear"])
def test_identical_columns_give_exact_zeros(eos_kind):
    """flat bottom, h, T, S uniform across the cells, stratified: GradRho and GradZ are exact zeros, so X = 0"""
    K = 12
    x = Host(planar_hex(12, 10, 30.0e3, bottom_depth=800.0), K)
    k = np.arange(K)
    ones = np.ones((x.nc_size, 1))
    st = x.column(ones * (20.0 + 7.5 * k), ones * (18.0 - 1.3 * k), ones * (34.0 + 0.11 * k), np.full(x.nc_size, 800.0),
                  eos_kind)
    u, psi = x.bolus()
    assert x.in_range[: x.ne_all].all()
    assert np.all(u[: x.ne_all] == 0.0) and np.all(psi[: x.ne_all] == 0.0)
    assert np.isnan(u[x.ne_all:]).all() and np.isnan(psi[x.ne_all:]).all()
    assert np.ptp(st["SpecVol"][: x.nc_all], axis=1).min() > 0.0  # stratified: the columns are not trivial
    assert all((s["n2_e"] > 0.0).all() for s in x.systems())


def _front(K=8, dtdz=-1.5, dtdx=-0.05 / 30.0e3):
    """hex24x20, every layer active, linear Eos: T = 20 + dtdz * k + dtdx * x (per layer, per metre), S uniform"""
    g = named_mesh("hex24x20")
    x = Host(g, K)
    xc = x.cells(g["xCell"])[:, None]
    ct = 20.0 + dtdz * np.arange(K)[None, :] + dtdx * xc
    x.column(np.full((x.nc_size, K), 50.0), ct, np.full((x.nc_size, K), 35.0), np.full(x.nc_size, 50.0 * K), "linear")
    return x


def test_the_bolus_flow_flattens_the_front():
    """Stable linear stratification, temperature falling in +x: the surface water flows toward the denser cell, and the
    stream function has one sign through the column."""
    x = _front()
    u, psi = x.bolus()
    assert x.in_range[: x.ne_all].all() and np.isfinite(u[: x.ne_all]).all()
    checked = 0
    for s in x.systems():
        es, k = s["es"], s["k"]
        assert (s["n2_e"] > 0.0).all()  # stable
        gr0 = s["grad_rho"][:, 0]
        use = np.abs(gr0) > 0.0
        surf = u[es, k[:, 0]]
        assert np.all(surf[use] * gr0[use] > 0.0)
        p = psi[es[:, None], k[:, 1:]][use]
        assert np.all(np.sign(p) == np.sign(gr0[use])[:, None])
        checked += int(use.sum())
    assert checked == x.ne_all


@pytest.mark.parametrize("mesh,K", [("hex24x20", 16), ("fib300_coast_ragged", 5), ("fib300_coast_ragged", 16)])
def test_the_column_transport_telescopes_to_zero(mesh, K):
    """sum_K hE[K] * BolusVelocity[e][K], the products and the sum taken exactly (rationals).  Exactly,
    hE[K] * ((Bot - Top) / hE[K]) = Bot - Top, and the differences telescope to Psi[bottom] - Psi[surface] = 0.  In
    floating point BolusVelocity[K] = fl(fl(Bot - Top) / hE[K]) carries two roundings, the difference and the quotient:
        hE[K] * BolusVelocity[K] = (Bot - Top) (1 + d1) (1 + d2),  |d1|, |d2| <= 2^-53,
    so each layer misses its exact term by at most (2 + 2^-53) 2^-53 |Bot - Top| <= (2 + 2^-53) 2^-53 * 2 max|Psi|, and
    the n = Hi - Lo + 1 layers together by at most  4 n max|Psi| 2^-53  up to second order (the factor 1 + 1e-6):
    c = 4 in c (Hi - Lo + 1) max|Psi| 2^-53."""
    x = _random(mesh, K)
    u, psi = x.bolus()
    worst, columns = 0.0, 0
    for s in x.systems():
        es, k, he = s["es"], s["k"], s["he"]
        n = he.shape[1]
        for b, e in enumerate(es):
            total = sum((Fraction(float(a)) * Fraction(float(v)) for a, v in zip(he[b], u[e, k[b]])), Fraction(0))
            pmax = np.abs(psi[e, k[b]]).max()
            bound = 4.0 * n * pmax * (EPS / 2) * (1.0 + 1.0e-6)
            err = abs(float(total))
            assert err <= bound, (e, err, bound)
            if bound > 0.0:
                worst = max(worst, err / bound)
            columns += 1
    print(f"{mesh} K {K}: worst |sum hE u*| / bound = {worst:.3f} over {columns} columns")
    assert columns > 0 and worst > 0.0


@pytest.mark.parametrize("dtdz", [1.5, 0.0], ids=["unstable", "unstratified"])
def test_unstable_and_unstratified_columns_are_finite(dtdz):
    """N2 <= 0 everywhere (clipped to 0): c^2 > 0 alone keeps every system definite"""
    x = _front(dtdz=dtdz)
    u, psi = x.bolus()
    for s in x.systems():
        assert all((n2 <= 0.0).all() for n2 in s["n2_cells"]) and np.all(s["n2_e"] == 0.0)
        g, h = s["g"], s["h"]
        assert (h >= 0.0).all() and (h[:, 0] > 0.0).all() and (h[:, -1] > 0.0).all()  # interior rows: H = 0 here
        assert (h + g + np.concatenate([np.zeros((len(g), 1)), g[:, :-1]], axis=1) > 0.0).all()  # the diagonal
    assert np.isfinite(u[: x.ne_all]).all() and np.isfinite(psi[: x.ne_all]).all()
    assert np.abs(u[: x.ne_all]).max() > 0.0


def test_zero_kappa_gives_exact_zeros_on_that_edge():
    x = _random("fib300_coast_ragged", 16)
    base_u, base_psi = x.bolus()
    wet = np.nonzero(x.in_range.sum(axis=1) > 1)[0]
    off = wet[::3]
    x.kappa[off] = 0.0
    u, psi = x.bolus()
    assert np.all(u[off][x.in_range[off]] == 0.0) and np.all(psi[off][x.in_range[off]] == 0.0)
    assert np.abs(base_u[off][x.in_range[off]]).max() > 0.0
    keep = np.ones(x.ne_size, bool)
    keep[off] = False
    assert np.array_equal(u[keep], base_u[keep], equal_nan=True) and np.array_equal(psi[keep], base_psi[keep], equal_nan=True)
    assert np.isnan(u[~x.in_range]).all() and np.isnan(psi[~x.in_range]).all()  # nothing outside the ranges


def test_transport_is_accumulated():
    """Transport_in + BolusVelocity on the ranges, untouched elsewhere"""
    x = _random("fib300_coast_ragged", 5)
    rng = np.random.default_rng(2)
    t_in = rng.uniform(-0.1, 0.1, (x.ne_size, x.K))
    t = t_in.copy()
    u, _ = x.bolus(t)
    assert np.array_equal(t[x.in_range], (t_in + u)[x.in_range]) and np.array_equal(t[~x.in_range], t_in[~x.in_range])
    single = x.in_range.sum(axis=1) == 1
    assert single.any() and np.all(u[single][x.in_range[single]] == 0.0)  # Lo == Hi: 0 / hE


def test_refusals_without_a_device():
    """through the C ABI: the two parameters are checked before the mesh is looked at; a host-only mesh is refused"""
    x = Host(planar_hex(6, 4, 30.0e3), 4)
    with pytest.raises(oa.OmegaAmdError, match="host-only"):
        oa.GentMcWilliams(x.mesh, None, None)
    for kappa in (-1.0, np.nan, np.inf):
        with pytest.raises(oa.OmegaAmdError, match="GMKappa"):
            oa.GentMcWilliams(x.mesh, None, None, kappa=kappa)
    for speed in (0.0, -0.3, np.nan, np.inf):
        with pytest.raises(oa.OmegaAmdError, match="GravWaveSpeed"):
            oa.GentMcWilliams(x.mesh, None, None, grav_wave_speed=speed)
