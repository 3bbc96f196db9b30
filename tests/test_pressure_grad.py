"""PressureGrad without a device: the NumPy restatement of the contract (tests/pressure_grad_reference.py) on column
fields from tests/column_reference.py, against what the continuous term -(grad Phi) - alpha grad p must give -- zero for
an ocean at rest, the barotropic force of a homogeneous ocean, second-order convergence to the analytic gradient --
and its masking and accumulation rules; plus the refusal that needs no device."""
import numpy as np
import pytest

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests import column_reference as CR
from tests import pressure_grad_reference as PR
from tests.column_reference import RHO0
from tests.meshes import named_mesh
from tests.vert_fixtures import column_levels

G = CR.GRAVITY
EPS = np.finfo(np.float64).eps


class Host:
    """One rank's host-only mesh in the library's local order, layer ranges of cells and edges, and the column fields
    of given h, T, S through the column restatement (NaN outside every column's active range)."""

    def __init__(self, g, K, min_level=None, max_level=None):
        self.K = K
        self.gm = oa.GlobalMesh(g)
        self.decomp = oa.Decomp(self.gm, 1, 0, 3)
        self.mesh = m = oa.HorzMesh(self.decomp, K, host_only=True)
        self.nc_all, self.nc_size, self.ne_all, self.ne_size = m.NCellsAll, m.NCellsSize, m.NEdgesAll, m.NEdgesSize
        self.cid = self.decomp.get_array("CellID")
        self.coe, self.dc = m.get_array("CellsOnEdge"), m.get_array("DcEdge")
        self.mask = np.ascontiguousarray(m.get_array("EdgeMask")[:, 0])
        self.lo_c, self.hi_c = CR.local_layer_ranges(self.cid, min_level, max_level, self.nc_all, self.nc_size, K)
        self.lo, self.hi = PR.edge_ranges(self.coe, self.ne_all, self.lo_c, self.hi_c, K)
        self.in_range = np.zeros((self.ne_size, K), bool)
        self.in_range[: self.ne_all] = PR.range_mask(self.lo, self.hi, self.ne_all, K)

    def cells(self, glob):
        """a global per-cell array in local order, zero on the sentinel row"""
        glob = np.asarray(glob, dtype=np.float64)
        out = np.zeros((self.nc_size,) + glob.shape[1:])
        out[: self.nc_all] = glob[self.cid[: self.nc_all] - 1]
        return out

    def column(self, h, ct, sa, ps, bot, eos_kind, linear=(-0.2, 0.8, 1000.0), tidal=None, sal=None):
        n, K = self.nc_size, self.K
        st = {"PressureInterface": np.full((n, K + 1), np.nan), "PressureMid": np.full((n, K), np.nan),
              "ZInterface": np.full((n, K + 1), np.nan), "ZMid": np.full((n, K), np.nan),
              "GeopotentialMid": np.full((n, K), np.nan), "SpecVol": np.full((n, K), np.nan)}
        CR.column_sequence(h, ct, sa, ps, tidal, sal, bot, self.lo_c, self.hi_c, self.nc_all, RHO0, eos_kind, st, None,
                           linear)
        return st

    def term(self, st, tend=None):
        tend = np.zeros((self.ne_size, self.K)) if tend is None else tend
        return PR.pressure_grad(tend, st["PressureMid"], st["GeopotentialMid"], st["SpecVol"], self.coe, self.dc,
                                self.mask, self.lo, self.hi, self.ne_all)


@pytest.mark.parametrize("eos_kind", ["teos10", "linear"])
def test_rest_is_exactly_zero(eos_kind):
    """horizontally uniform h, T, S on a flat bottom: every difference across an edge is exactly 0"""
    K = 12
    x = Host(planar_hex(12, 10, 30.0e3, bottom_depth=800.0), K)
    k = np.arange(K)
    ones = np.ones((x.nc_size, 1))
    h = ones * (20.0 + 7.5 * k)
    ct = ones * (18.0 - 1.3 * k)
    sa = ones * (34.0 + 0.11 * k)
    st = x.column(h, ct, sa, np.full(x.nc_size, 1.01325e5), np.full(x.nc_size, 800.0), eos_kind)
    out = x.term(st)
    assert x.in_range[: x.ne_all].all()
    assert np.all(out == 0.0)
    assert np.ptp(st["SpecVol"][: x.nc_all], axis=1).min() > 0.0  # stratified: the columns are not trivial


def test_homogeneous_ocean_is_barotropic():
    """Constant density (linear Eos, zero expansion coefficients): the term is the same at every level of an edge and
    equals -grad(g (Rho0 alpha sum(h) - Bot)) - alpha grad(Ps).  In a layer the two parts of the term each carry the
    whole column -- g z of the order g Bot, alpha p of the order alpha p_bottom -- and cancel down to the barotropic
    force.  Every cell value that enters (ZMid, PressureMid) is a sequential sum of at most K + 1 positive terms, so
    its rounding error is at most (K + 1) eps times its magnitude; multiplied by g or alpha, differenced across the
    edge (two cells) and through the few remaining operations of the term and of the expected expression (8 roundings
    of at most that magnitude), the two sides differ by at most (2 (K + 1) + 8) eps M / Dc with
    M = g (max Bot + Rho0 alpha max sum(h)) + alpha max PressureInterface."""
    K = 10
    g = planar_hex(12, 10, 30.0e3)
    x = Host(g, K)
    rng = np.random.default_rng(11)
    n = int(g["nCells"])
    h = x.cells(rng.uniform(5.0, 400.0, (n, K)))
    bot = x.cells(rng.uniform(500.0, 4000.0, n))
    ps = x.cells(rng.uniform(0.9e5, 1.1e5, n))
    rho = 1031.5
    alpha = 1.0 / rho
    st = x.column(h, np.zeros_like(h), np.zeros_like(h), ps, bot, "linear", linear=(0.0, 0.0, rho))
    assert np.all(st["SpecVol"][: x.nc_all] == alpha)
    out = x.term(st)
    c0, c1 = x.coe[: x.ne_all, 0], x.coe[: x.ne_all, 1]
    total = h.sum(axis=1)
    baro = G * (RHO0 * alpha * total - bot)
    want = -((baro[c1] - baro[c0]) / x.dc[: x.ne_all]) - alpha * ((ps[c1] - ps[c0]) / x.dc[: x.ne_all])
    M = G * (bot.max() + RHO0 * alpha * total.max()) + alpha * np.nanmax(st["PressureInterface"])
    bound = (2 * (K + 1) + 8) * EPS * M / x.dc[: x.ne_all].min()
    err = np.abs(out[: x.ne_all] - want[:, None]).max()
    spread = np.ptp(out[: x.ne_all], axis=1).max()
    print(f"homogeneous: max |term - expected| = {err:.3e}, level spread = {spread:.3e}, bound = {bound:.3e}, "
          f"max |term| = {np.abs(want).max():.3e}")
    assert err <= bound
    assert spread <= 2 * bound
    assert np.abs(want).max() > 1.0e6 * bound  # the bound is tight against the signal


def _analytic(x, y, K, lx, ly):
    """Phi, p, alpha and the gradients of Phi and p on points (x, y), level by level: [n][K] each"""
    k = np.arange(K)[None, :]
    ax, ay = 2.0 * np.pi / lx, 2.0 * np.pi / ly
    X, Y = (ax * x)[:, None], (ay * y)[:, None]
    a, b = 10.0 + 0.5 * k, 1.0e4 * (1.0 + 0.1 * k)
    phi = a * np.sin(X + 0.3) * np.cos(Y)
    phi_x, phi_y = a * ax * np.cos(X + 0.3) * np.cos(Y), -a * ay * np.sin(X + 0.3) * np.sin(Y)
    p = 1.0e5 * (1.0 + k) + b * np.cos(X) * np.sin(2.0 * Y + 0.1)
    p_x, p_y = -b * ax * np.sin(X) * np.sin(2.0 * Y + 0.1), 2.0 * b * ay * np.cos(X) * np.cos(2.0 * Y + 0.1)
    alpha = 1.0e-3 * (1.0 + 0.02 * np.sin(X) * np.sin(Y + 0.7)) + 0.0 * k
    return phi, p, alpha, phi_x, phi_y, p_x, p_y


def test_converges_at_second_order():
    """Analytic Phi, p, alpha (periodic on the plane) handed to the array form on hexagon meshes of 16, 32 and 64 cells
    across a fixed domain: the L-infinity error against -(d_n Phi + alpha d_n p) at the edge midpoint falls at second
    order.  Measured: errors 2.68e-06, 6.92e-07, 1.74e-07; observed orders 1.953 and 1.990 (required: >= 1.8, the
    margin covers the pre-asymptotic step)."""
    K, L = 3, 1.92e6
    errs = []
    for n in (16, 32, 64):
        g = planar_hex(n, n, L / n)
        x = Host(g, K)
        m = x.mesh
        lx, ly = g["x_period"], g["y_period"]
        phi, p, alpha, *_ = _analytic(m.get_array("XCell"), m.get_array("YCell"), K, lx, ly)
        out = PR.pressure_grad(np.zeros((x.ne_size, K)), p, phi, alpha, x.coe, x.dc, x.mask, x.lo, x.hi, x.ne_all)
        _, _, alpha_e, phi_x, phi_y, p_x, p_y = _analytic(m.get_array("XEdge"), m.get_array("YEdge"), K, lx, ly)
        ang = m.get_array("AngleEdge")
        nx, ny = np.cos(ang)[:, None], np.sin(ang)[:, None]
        want = -((phi_x * nx + phi_y * ny) + alpha_e * (p_x * nx + p_y * ny))
        errs.append(np.abs(out[: x.ne_all] - want[: x.ne_all]).max())
        assert np.abs(want[: x.ne_all]).max() > 1.0e-5
    orders = [np.log2(errs[i] / errs[i + 1]) for i in range(2)]
    print("convergence: errors", " ".join(f"{e:.3e}" for e in errs), "orders", " ".join(f"{o:.3f}" for o in orders))
    assert min(orders) >= 1.8


def _ragged(K=37, seed=3):
    g = named_mesh("fib700_coast_ragged")
    n = int(g["nCells"])
    rng = np.random.default_rng(seed)
    mn, mx = column_levels(rng, n, K, 6)
    x = Host(g, K, mn, mx)
    h = x.cells(rng.uniform(0.5, 40.0, (n, K)))
    ct = x.cells(rng.uniform(-2.0, 30.0, (n, K)))
    sa = x.cells(rng.uniform(30.0, 38.0, (n, K)))
    st = x.column(h, ct, sa, x.cells(rng.uniform(0.9e5, 1.1e5, n)), x.cells(rng.uniform(100.0, 6000.0, n)), "teos10",
                  tidal=x.cells(rng.uniform(-1.0, 1.0, n)), sal=x.cells(rng.uniform(-0.1, 0.1, n)))
    return x, st, rng


def test_masking_on_a_ragged_coast():
    """partial-depth columns next to land: only the levels active in both cells of an edge are written"""
    x, st, rng = _ragged()
    tend = np.full((x.ne_size, x.K), np.nan)
    tend[x.in_range] = rng.uniform(-1.0e-3, 1.0e-3, int(x.in_range.sum()))
    out = x.term(st, tend.copy())
    assert np.isnan(out[~x.in_range]).all()
    assert np.isfinite(out[x.in_range]).all()
    ok = (x.lo[: x.ne_all] >= 0) & (x.lo[: x.ne_all] <= x.hi[: x.ne_all]) & (x.hi[: x.ne_all] < x.K)
    partial = ok & ((x.lo[: x.ne_all] > 0) | (x.hi[: x.ne_all] < x.K - 1))
    assert (~ok).any() and partial.any() and (x.in_range.sum(axis=1) == x.K).any()  # empty, partial and full ranges
    assert not np.array_equal(out[x.in_range], tend[x.in_range])


def test_accumulates_into_the_tendency():
    """Tend_in - term, bit for bit"""
    x, st, rng = _ragged(K=16, seed=4)
    tend_in = rng.uniform(-1.0e-3, 1.0e-3, (x.ne_size, x.K))
    minus_term = x.term(st)  # 0 - term
    out = x.term(st, tend_in.copy())
    assert np.array_equal(out[x.in_range], (tend_in + minus_term)[x.in_range])  # a - b == a + (-b) in IEEE arithmetic
    assert np.array_equal(out[~x.in_range], tend_in[~x.in_range])
    assert np.abs(minus_term[x.in_range]).max() > 0.0


def test_host_only_mesh_is_refused():
    x = Host(planar_hex(6, 4, 30.0e3), 4)
    with pytest.raises(oa.OmegaAmdError, match="host-only"):
        oa.PressureGrad(x.mesh, None, None)
