"""VertCoord / Eos (host): the NumPy restatement of the column contract (tests/column_reference.py) pinned to the
reference's own known answers (components/omega/test/ocn/EosTest.cpp, VertCoordTest.cpp), and the loud failures
of the C++ objects that need no device."""
import numpy as np
import pytest

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests import column_reference as R
from tests.column_reference import RHO0

G = R.GRAVITY
ATOL = 1.0e-10  # VertCoordTest.cpp's tolerance


# ---- EosTest.cpp: Sa = 30 g/kg, Ct = 10 degC, p = 1000 dbar, KDisp = 1, RTol 1e-10
TEOS_EXPECTED = 0.0009732819628
LINEAR_EXPECTED = 0.0009784735812133072


def _uniform(n_size, K, v):
    return np.full((n_size, K), v)


def test_teos10_known_answer():
    v = R.spec_vol_teos10(np.float64(10.0), np.float64(30.0), np.float64(1000.0))
    assert np.isclose(v, TEOS_EXPECTED, rtol=1e-10, atol=0.0)


def test_linear_known_answer():
    assert R.spec_vol_linear(10.0, 30.0) == LINEAR_EXPECTED


@pytest.mark.parametrize("kind,expected", [("teos10", TEOS_EXPECTED), ("linear", LINEAR_EXPECTED)])
@pytest.mark.parametrize("kdisp", [None, 1, -3])
def test_spec_vol_uniform_input_plain_and_displaced(kind, expected, kdisp):
    n_all, K = 7, 60
    ct, sa, p = _uniform(n_all + 1, K, 10.0), _uniform(n_all + 1, K, 30.0), _uniform(n_all + 1, K, 1000.0)
    out = R.eos_spec_vol(kind, ct, sa, p, n_all, kdisp)
    assert np.allclose(out[:n_all], expected, rtol=1e-10, atol=0.0)
    assert np.all(out[n_all] == 0.0)  # sentinel row


def test_displaced_uses_the_clamped_level():
    n_all, K = 3, 6
    ct, sa = _uniform(n_all + 1, K, 10.0), _uniform(n_all + 1, K, 30.0)
    p = np.tile(np.arange(K, dtype=np.float64) * 500.0, (n_all + 1, 1))
    for kdisp in (-2, 1, 4):
        out = R.eos_spec_vol("teos10", ct, sa, p, n_all, kdisp)
        for k in range(K):
            kk = min(max(k + kdisp, 0), K - 1)
            assert out[0, k] == R.spec_vol_teos10(np.float64(10.0), np.float64(30.0), np.float64(p[0, kk]))


def _ranges(n_size, n_all, K):
    lo = np.full(n_size, -1, np.int32)
    hi = np.full(n_size, -1, np.int32)
    lo[:n_all], hi[:n_all] = 0, K - 1
    return lo, hi


def test_pressure_uniform_thickness():
    # VertCoordTest.cpp: h = 1/(g rho0), Ps = 1 -> PInt = K + 1, PMid = K + 1.5 (here Ps = 0: PInt = K, PMid = K + 1/2)
    n_all, K = 10, 60
    lo, hi = _ranges(n_all + 1, n_all, K)
    h = _uniform(n_all + 1, K, 1.0 / (G * RHO0))
    for ps0, off in ((0.0, 0.0), (1.0, 1.0)):
        pint, pmid = np.full((n_all + 1, K + 1), np.nan), np.full((n_all + 1, K), np.nan)
        R.pressure(h, np.full(n_all + 1, ps0), lo, hi, n_all, RHO0, pint, pmid)
        k = np.arange(K + 1)
        assert np.allclose(pint[:n_all], k + off, atol=ATOL, rtol=0)
        assert np.allclose(pmid[:n_all], np.arange(K) + 0.5 + off, atol=ATOL, rtol=0)
        assert np.all(np.isnan(pint[n_all])) and np.all(np.isnan(pmid[n_all]))


def test_pressure_nonuniform_thickness_and_surface_pressure():
    # VertCoordTest.cpp: h = (K+1)/(g rho0), Ps = ICell -> PInt = K(K+1)/2 + ICell
    n_all, K = 10, 60
    lo, hi = _ranges(n_all + 1, n_all, K)
    h = np.tile((np.arange(K) + 1.0) / (G * RHO0), (n_all + 1, 1))
    ps = np.arange(n_all + 1, dtype=np.float64)
    pint, pmid = np.full((n_all + 1, K + 1), np.nan), np.full((n_all + 1, K), np.nan)
    R.pressure(h, ps, lo, hi, n_all, RHO0, pint, pmid)
    k = np.arange(K + 1)
    assert np.allclose(pint[:n_all], (k + 1.0) * k / 2.0 + ps[:n_all, None], atol=ATOL, rtol=0)


def test_zheight_uniform_and_nonuniform():
    # VertCoordTest.cpp: SpecVol = 1, bottom depth = NVertLayers, h = 1/rho0 -> ZInt = -K, ZMid = -K - 0.5
    n_all, K = 10, 60
    lo, hi = _ranges(n_all + 1, n_all, K)
    sv = _uniform(n_all + 1, K, 1.0)
    bot = np.full(n_all + 1, float(K))
    h = _uniform(n_all + 1, K, 1.0 / RHO0)
    zint, zmid = np.full((n_all + 1, K + 1), np.nan), np.full((n_all + 1, K), np.nan)
    R.zheight(h, sv, bot, lo, hi, n_all, RHO0, zint, zmid)
    assert np.allclose(zint[:n_all], -(K - (K - np.arange(K + 1.0))), atol=ATOL, rtol=0)
    assert np.allclose(zmid[:n_all], -np.arange(K) - 0.5, atol=ATOL, rtol=0)
    # h = (K+1)/rho0, bottom depth K(K+1)/2 -> ZInt = -K(K+1)/2
    h2 = np.tile((np.arange(K) + 1.0) / RHO0, (n_all + 1, 1))
    bot2 = np.full(n_all + 1, K * (K + 1) / 2.0)
    zint, zmid = np.full((n_all + 1, K + 1), np.nan), np.full((n_all + 1, K), np.nan)
    R.zheight(h2, sv, bot2, lo, hi, n_all, RHO0, zint, zmid)
    k = np.arange(K + 1.0)
    assert np.allclose(zint[:n_all], -((k + 1.0) * k) / 2.0, atol=ATOL, rtol=0)


def test_geopotential():
    # VertCoordTest.cpp: ZMid = (ICell + K)/g, tidal = SAL = 0 -> GeoMid = ICell + K
    n_all, K = 10, 60
    lo, hi = _ranges(n_all + 1, n_all, K)
    zmid = (np.arange(n_all + 1)[:, None] + np.arange(K)[None, :]) / G
    geo = np.full((n_all + 1, K), np.nan)
    R.geopotential(zmid, np.zeros(n_all + 1), np.zeros(n_all + 1), lo, hi, n_all, geo)
    assert np.allclose(geo[:n_all], np.arange(n_all)[:, None] + np.arange(K)[None, :], atol=ATOL, rtol=0)
    assert np.all(np.isnan(geo[n_all]))


def test_target_thickness_uniform_and_fixed():
    # VertCoordTest.cpp: h = 2, Ref = 1, Ps = 0 [so (PInt(KMax+1) - PInt(KMin))/(g rho0) = 2 K]
    n_all, K = 10, 60
    lo, hi = _ranges(n_all + 1, n_all, K)
    h = _uniform(n_all + 1, K, 2.0)
    ref = _uniform(n_all + 1, K, 1.0)
    pint, pmid = np.zeros((n_all + 1, K + 1)), np.zeros((n_all + 1, K))
    R.pressure(h, np.zeros(n_all + 1), lo, hi, n_all, RHO0, pint, pmid)
    tgt = np.full((n_all + 1, K), np.nan)
    R.target_thickness(pint, ref, R.movement_weights("Uniform", K), lo, hi, n_all, RHO0, tgt)
    assert np.allclose(tgt[:n_all], 2.0, atol=ATOL, rtol=0)
    tgt = np.full((n_all + 1, K), np.nan)
    R.target_thickness(pint, ref, R.movement_weights("Fixed", K), lo, hi, n_all, RHO0, tgt)
    # Fixed: the whole change goes to the top layer: MaxLayerCell + 2 there, 1 below
    assert np.allclose(tgt[:n_all, 0], hi[:n_all] + 2.0, atol=ATOL, rtol=0)
    assert np.allclose(tgt[:n_all, 1:], 1.0, atol=ATOL, rtol=0)


def test_edge_and_vertex_ranges_pattern():
    # VertCoordTest.cpp: MinLayerCell = -2 ICell, MaxLayerCell = 2 ICell (no cell has Max == -1, none is land):
    # the edge / vertex ranges are plain min / max over their cells
    g = planar_hex(6, 6, 1.0)
    n_cells = g["nCells"]
    K = 60
    mn = np.array([-2 * c for c in range(n_cells + 1)], np.int32)
    mx = np.array([2 * c for c in range(n_cells + 1)], np.int32)
    coe = np.asarray(g["cellsOnEdge"])  # 0-based
    cov = np.asarray(g["cellsOnVertex"])
    for cells_on, n in ((coe, g["nEdges"]), (cov, g["nVertices"])):
        top, bot, mxt, mxb = R.min_max_layer(cells_on, n, mn, mx, K)
        assert np.array_equal(top[:n], np.min(-2 * cells_on, axis=1))
        assert np.array_equal(bot[:n], np.max(-2 * cells_on, axis=1))
        assert np.array_equal(mxt[:n], np.min(2 * cells_on, axis=1))
        assert np.array_equal(mxb[:n], np.max(2 * cells_on, axis=1))
        assert (top[n], bot[n], mxt[n], mxb[n]) == (K + 1, K + 1, -1, -1)


def test_edge_ranges_with_land():
    # a cell with MaxLayerCell == -1 is land: it does not lower MinTop nor raise MinBot
    K = 10
    mn = np.array([2, 3, -1], np.int32)
    mx = np.array([7, 9, -1], np.int32)
    cells_on = np.array([[0, 1], [1, 2], [2, 0]])
    top, bot, mxt, mxb = R.min_max_layer(cells_on, 3, mn, mx, K)
    assert list(top) == [2, 3, 2, K + 1]
    assert list(bot) == [3, 3, 2, K + 1]
    assert list(mxt) == [7, -1, -1, -1]
    assert list(mxb) == [9, 9, 7, -1]


def test_local_layer_ranges_gather():
    cell_id = np.array([3, 1, 2, 4], np.int32)  # 1-based global ids of 3 local cells + sentinel
    lo, hi = R.local_layer_ranges(cell_id, [1, 2, 5], [10, 20, 30], 3, 4, 40)
    assert list(lo) == [4, 0, 1, -1] and list(hi) == [29, 9, 19, -1]
    lo, hi = R.local_layer_ranges(cell_id, None, None, 3, 4, 40)
    assert list(lo) == [0, 0, 0, -1] and list(hi) == [39, 39, 39, -1]


# ---- the C++ objects: no device needed to be refused
def _host_only_mesh(K=8):
    gm = oa.GlobalMesh(planar_hex(8, 8, 1.0))
    d = oa.Decomp(gm, 1, 0, 3)
    return gm, d, oa.HorzMesh(d, K, host_only=True)


def test_host_only_mesh_is_refused():
    gm, d, m = _host_only_mesh()
    with pytest.raises(oa.OmegaAmdError, match="host-only"):
        oa.VertCoord(m, 8)
    with pytest.raises(oa.OmegaAmdError, match="host-only"):
        oa.Eos(m, 8)


def test_unknown_movement_weight_and_eos_type_are_refused():
    gm, d, m = _host_only_mesh()
    with pytest.raises(oa.OmegaAmdError, match="MovementWeightType"):
        oa.VertCoord(m, 8, movement_weight_type="Linear")
    with pytest.raises(oa.OmegaAmdError, match="EosType"):
        oa.Eos(m, 8, eos_type="jmd95")
