"""VertCoord / Eos on the GPU: every method and the fused column pass equal the NumPy restatement of the contract
(tests/column_reference.py) bit for bit, on NaN-filled output arrays (exactly the contract's entries are written,
the rest still hold NaN); the fused pass equals the four-launch sequence on every element; the reference's known
answers pass through the device; a 2-part decomposition gives the 1-part values at the same global ids."""
import numpy as np
import pytest

import omega_amd as oa
from tests import column_reference as R
from tests.meshes import named_mesh
from tests.vert_fixtures import EOS_OUT, RHO0, Col, same as _assert_same

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module", autouse=True)
def _device():
    oa.device_init(0)


CASES = [("hex24x20", 80, "teos10", 3, 0, 1), ("hex24x20", 60, "linear", None, 1, 2),
         ("hex24x20", 37, "teos10", -2, 1, 2), ("fib700_coast_ragged", 80, "linear", 2, 0, 1),
         ("fib700_coast_ragged", 60, "teos10", None, 0, 1), ("fib700_coast_ragged", 37, "teos10", 5, 2, 1)]


@pytest.mark.parametrize("mesh,K,eos_kind,kdisp,ti,si", CASES)
def test_layer_ranges(mesh, K, eos_kind, kdisp, ti, si):
    c = Col(named_mesh(mesh), K, eos_kind)
    assert np.array_equal(c.vc.get("MinLayerCell"), c.lo) and np.array_equal(c.vc.get("MaxLayerCell"), c.hi)
    m = c.mesh
    for cells_name, n_all, names in (("CellsOnEdge", m.NEdgesAll, ("MinLayerEdgeTop", "MinLayerEdgeBot",
                                                                  "MaxLayerEdgeTop", "MaxLayerEdgeBot")),
                                     ("CellsOnVertex", m.NVerticesAll, ("MinLayerVertexTop", "MinLayerVertexBot",
                                                                       "MaxLayerVertexTop", "MaxLayerVertexBot"))):
        cells_on = m.get_array(cells_name)
        want = R.min_max_layer(cells_on, n_all, c.lo, c.hi, K)
        for name, w in zip(names, want):
            assert np.array_equal(c.vc.get(name), w), name
    if "coast" in mesh:  # edges and vertices on the coast see the land sentinel cell
        assert (m.get_array("CellsOnEdge")[: m.NEdgesAll] == m.NCellsAll).any()


@pytest.mark.parametrize("mesh,K,eos_kind,kdisp,ti,si", CASES)
def test_every_method_bit_exact(mesh, K, eos_kind, kdisp, ti, si):
    c = Col(named_mesh(mesh), K, eos_kind)
    want = c.nan_state()
    c.run_sequence(kdisp, ti, si)
    got = c.outputs()
    R.pressure(c.h, c.ps, c.lo, c.hi, c.n_all, RHO0, want["PressureInterface"], want["PressureMid"])
    for name in ("PressureInterface", "PressureMid"):
        _assert_same(got[name], want[name], name)
    pdbar = want["PressureMid"] * 1.0e-4
    _assert_same(got["SpecVol"], R.eos_spec_vol(eos_kind, c.tr[ti], c.tr[si], pdbar, c.n_all), "SpecVol")
    if kdisp is not None:
        _assert_same(got["SpecVolDisplaced"], R.eos_spec_vol(eos_kind, c.tr[ti], c.tr[si], pdbar, c.n_all, kdisp),
                     "SpecVolDisplaced")
    else:
        assert np.all(np.isnan(got["SpecVolDisplaced"]))
    sv = R.eos_spec_vol(eos_kind, c.tr[ti], c.tr[si], pdbar, c.n_all)
    R.zheight(c.h, sv, c.bot, c.lo, c.hi, c.n_all, RHO0, want["ZInterface"], want["ZMid"])
    R.geopotential(want["ZMid"], c.tidal, c.sal, c.lo, c.hi, c.n_all, want["GeopotentialMid"])
    for name in ("ZInterface", "ZMid", "GeopotentialMid"):
        _assert_same(got[name], want[name], name)
    # target thickness, Uniform and Fixed weights
    c.vc.compute_target_thickness()
    oa.device_synchronize()
    R.target_thickness(want["PressureInterface"], c.ref, R.movement_weights("Uniform", K), c.lo, c.hi, c.n_all, RHO0,
                       want["LayerThicknessTarget"])
    _assert_same(c.vc.get("LayerThicknessTarget"), want["LayerThicknessTarget"], "LayerThicknessTarget")
    # Eos on its own, pressure in dbar as given (p_scale 1)
    p = np.random.default_rng(3).uniform(0.0, 6000.0, (c.n_size, K))
    c.eos.set("SpecVol", np.full((c.n_size, K), np.nan))
    c.eos.compute_spec_vol(c.tr[ti], c.tr[si], p)
    _assert_same(c.eos.get("SpecVol"), R.eos_spec_vol(eos_kind, c.tr[ti], c.tr[si], p, c.n_all), "SpecVol(p)")


def test_target_thickness_fixed_weights():
    K = 60
    c = Col(named_mesh("hex24x20"), K, "teos10", weights="Fixed")
    c.vc.compute_pressure(c.state.device_ptr(0), c.ps)
    c.vc.compute_target_thickness()
    oa.device_synchronize()
    want = c.nan_state()
    R.pressure(c.h, c.ps, c.lo, c.hi, c.n_all, RHO0, want["PressureInterface"], want["PressureMid"])
    R.target_thickness(want["PressureInterface"], c.ref, R.movement_weights("Fixed", K), c.lo, c.hi, c.n_all, RHO0,
                       want["LayerThicknessTarget"])
    _assert_same(c.vc.get("LayerThicknessTarget"), want["LayerThicknessTarget"], "LayerThicknessTarget")


@pytest.mark.parametrize("mesh,K,eos_kind,kdisp,ti,si", CASES)
def test_fused_equals_restatement_and_sequence(mesh, K, eos_kind, kdisp, ti, si):
    g = named_mesh(mesh)
    fused, seq = Col(g, K, eos_kind), Col(g, K, eos_kind)
    fused.run_fused(kdisp, ti, si)
    seq.run_sequence(kdisp, ti, si)
    got, got_seq = fused.outputs(), seq.outputs()
    want = fused.expected(kdisp, ti, si)
    for name in ("PressureInterface", "PressureMid", "SpecVol", "ZInterface", "ZMid", "GeopotentialMid") + (
            ("SpecVolDisplaced",) if kdisp is not None else ()):
        _assert_same(got[name], want[name], name)
    for name in got:  # every element, NaN where neither wrote
        _assert_same(got[name], got_seq[name], name + " (fused vs sequence)")
    # the fused pass leaves entries outside the active ranges alone, and a second call gives the same bits
    fused.run_fused(kdisp, ti, si)
    for name, v in fused.outputs().items():
        _assert_same(v, got[name], name + " (second call)")


def test_known_answers_on_the_device():
    K = 60
    c = Col(named_mesh("hex24x20"), K, "teos10")
    n = c.n_size
    # EosTest.cpp: Sa = 30, Ct = 10, p = 1000 dbar; TEOS-10 plain and displaced (KDisp 1), linear
    ct, sa, p = np.full((n, K), 10.0), np.full((n, K), 30.0), np.full((n, K), 1000.0)
    c.eos.compute_spec_vol(ct, sa, p)
    c.eos.compute_spec_vol_disp(ct, sa, p, 1)
    for name in EOS_OUT:
        v = c.eos.get(name)
        assert np.allclose(v[: c.n_all], 0.0009732819628, rtol=1e-10, atol=0.0) and np.all(v[c.n_all] == 0.0)
    lin = oa.Eos(c.mesh, K, "Linear")
    lin.compute_spec_vol(ct, sa, p)
    assert np.all(lin.get("SpecVol")[: c.n_all] == 0.0009784735812133072)
    # VertCoordTest.cpp, every layer active
    vc = oa.VertCoord(c.mesh, K, RHO0)
    g = vc.get_real("Gravity")
    assert g == 9.80616
    vc.compute_pressure(np.full((n, K), 1.0 / (g * RHO0)), np.zeros(n))
    assert np.allclose(vc.get("PressureInterface")[: c.n_all], np.arange(K + 1.0), atol=1e-10, rtol=0)
    assert np.allclose(vc.get("PressureMid")[: c.n_all], np.arange(K) + 0.5, atol=1e-10, rtol=0)
    ps = np.arange(n, dtype=np.float64)
    vc.compute_pressure(np.tile((np.arange(K) + 1.0) / (g * RHO0), (n, 1)), ps)
    k = np.arange(K + 1.0)
    assert np.allclose(vc.get("PressureInterface")[: c.n_all], (k + 1.0) * k / 2.0 + ps[: c.n_all, None], atol=1e-10,
                       rtol=0)
    vc.set("BottomDepth", np.full(n, float(K)))
    vc.compute_zheight(np.full((n, K), 1.0 / RHO0), np.ones((n, K)))
    assert np.allclose(vc.get("ZInterface")[: c.n_all], -np.arange(K + 1.0), atol=1e-10, rtol=0)
    assert np.allclose(vc.get("ZMid")[: c.n_all], -np.arange(K) - 0.5, atol=1e-10, rtol=0)
    zmid = (np.arange(n)[:, None] + np.arange(K)[None, :]) / g
    vc.set("ZMid", zmid)
    vc.compute_geopotential()
    oa.device_synchronize()
    assert np.allclose(vc.get("GeopotentialMid")[: c.n_all], np.arange(c.n_all)[:, None] + np.arange(K)[None, :],
                       atol=1e-10, rtol=0)
    vc.compute_pressure(np.full((n, K), 2.0), np.zeros(n))
    vc.set("RefLayerThickness", np.ones((n, K)))
    vc.compute_target_thickness()
    oa.device_synchronize()
    assert np.allclose(vc.get("LayerThicknessTarget")[: c.n_all], 2.0, atol=1e-10, rtol=0)
    # the MinLayerCell = -2 ICell, MaxLayerCell = 2 ICell pattern through the device range kernels
    m = c.mesh
    vc.set("MinLayerCell", -2 * np.arange(n, dtype=np.int32))
    vc.set("MaxLayerCell", 2 * np.arange(n, dtype=np.int32))
    vc.min_max_layer_edge()
    vc.min_max_layer_vertex()
    for cells_name, n_all, tag in (("CellsOnEdge", m.NEdgesAll, "Edge"), ("CellsOnVertex", m.NVerticesAll, "Vertex")):
        co = m.get_array(cells_name)[:n_all]
        assert np.array_equal(vc.get(f"MinLayer{tag}Top")[:n_all], np.min(-2 * co, axis=1))
        assert np.array_equal(vc.get(f"MinLayer{tag}Bot")[:n_all], np.max(-2 * co, axis=1))
        assert np.array_equal(vc.get(f"MaxLayer{tag}Top")[:n_all], np.min(2 * co, axis=1))
        assert np.array_equal(vc.get(f"MaxLayer{tag}Bot")[:n_all], np.max(2 * co, axis=1))


@pytest.mark.parametrize("mesh,K", [("hex24x20", 37), ("fib700_coast_ragged", 80)])
def test_two_part_decomposition_matches_one_part(mesh, K):
    g = named_mesh(mesh)
    one = Col(g, K, "teos10")
    one.run_fused(1, 0, 1)
    ref = one.outputs()
    ref_cell = {int(gid): i for i, gid in enumerate(one.cid[: one.n_all])}
    m1, d1 = one.mesh, one.decomp
    ranges1 = {n: one.vc.get(n) for n in oa.VCOORD_I4}
    eid1 = {int(x): i for i, x in enumerate(d1.get_array("EdgeID")[: m1.NEdgesAll])}
    vid1 = {int(x): i for i, x in enumerate(d1.get_array("VertexID")[: m1.NVerticesAll])}
    for rank in (0, 1):
        c = Col(g, K, "teos10", nparts=2, rank=rank)
        c.run_fused(1, 0, 1)
        got = c.outputs()
        idx = np.array([ref_cell[int(gid)] for gid in c.cid[: c.n_all]])
        for name, v in got.items():
            _assert_same(v[: c.n_all], ref[name][idx], f"{name} rank {rank}")
        for name in ("MinLayerCell", "MaxLayerCell"):
            assert np.array_equal(c.vc.get(name)[: c.n_all], ranges1[name][idx])
        m = c.mesh
        eids = c.decomp.get_array("EdgeID")[: m.NEdgesOwned]
        vids = c.decomp.get_array("VertexID")[: m.NVerticesOwned]
        ei = np.array([eid1[int(x)] for x in eids])
        vi = np.array([vid1[int(x)] for x in vids])
        for name in oa.VCOORD_I4:
            if "Edge" in name:
                assert np.array_equal(c.vc.get(name)[: m.NEdgesOwned], ranges1[name][ei]), name
            elif "Vertex" in name:
                assert np.array_equal(c.vc.get(name)[: m.NVerticesOwned], ranges1[name][vi]), name
