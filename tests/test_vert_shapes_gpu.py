"""VertCoord / Eos at every launch shape the column kernel branches on: a sweep of NVertLayers over the tile
thresholds of launchColumn (16, 8, 4, 2 columns per workgroup, then the refusal), over rows that do not start on 16
bytes (odd levelPitch: the one-value path of load2 / store2 and pairs that straddle two rows) and down to a single
layer.  Every output of the fused pass and of each single-stage launch equals tests/column_reference.py bit for bit,
on NaN-poisoned outputs.  Which tile a case lands on is computed from the layout rule restated in
tests/vert_fixtures.py, and the sweep asserts that it covers every tile, the refusal and an unaligned case."""
import numpy as np
import pytest

import omega_amd as oa
from tests import column_reference as R
from tests import vert_fixtures as F
from tests.meshes import named_mesh
from tests.vert_fixtures import RHO0, Col, same

pytestmark = pytest.mark.gpu

MESH = "fib300_coast_ragged"  # 251 cells, land, valence 5 / 6 / 7
FUSED_LIMIT = F.column_limit(F.FUSED | F.STAGE_SPEC_VOL_DISP)
# both sides of every tile threshold of the fused mask (112|113, 240|241, 496|497, the limit), rows of odd pitch
# (K or K + 1 odd below 16), K = 16 / 17 / 31 around the first padded pitch, and the one-layer column
K_SWEEP = [1, 2, 3, 5, 8, 15, 16, 17, 31, 112, 113, 240, 241, 496, 497, FUSED_LIMIT]
STAGES = (F.STAGE_PRESSURE, F.STAGE_SPEC_VOL, F.STAGE_SPEC_VOL_DISP, F.STAGE_ZHEIGHT, F.STAGE_GEOPOTENTIAL,
          F.STAGE_TARGET)


@pytest.fixture(scope="module", autouse=True)
def _device():
    oa.device_init(0)


def _eos_kind(K):
    return "linear" if K in (8, 240) else "teos10"


def test_sweep_covers_every_launch_branch():
    """the thresholds come from the restated layout rule, so a layout change moves the sweep's claim with it"""
    fused = F.FUSED | F.STAGE_SPEC_VOL_DISP
    assert F.column_limit(F.FUSED) == FUSED_LIMIT  # SpecVolDisplaced needs no LDS buffer of its own
    assert {F.column_tile(F.FUSED, K) for K in K_SWEEP} == {16, 8, 4, 2}
    assert {F.column_tile(fused, K) for K in K_SWEEP} == {16, 8, 4, 2}
    for tile in (16, 8, 4):  # both sides of each threshold
        last = max(K for K in range(1, FUSED_LIMIT + 1) if F.column_tile(fused, K) == tile)
        assert last in K_SWEEP and last + 1 in K_SWEEP, (tile, last)
    assert F.column_tile(fused, FUSED_LIMIT) == 2 and F.column_tile(fused, FUSED_LIMIT + 1) is None
    # rows that start off 16 bytes, in the level arrays and in the interface arrays, and the aligned case
    assert any(F.rows_unaligned(K) for K in K_SWEEP) and any(F.rows_unaligned(K + 1) for K in K_SWEEP)
    assert any(not F.rows_unaligned(K) and not F.rows_unaligned(K + 1) for K in K_SWEEP)
    # the single-stage launches reach smaller tiles later than the fused pass: the sweep still leaves tile 16 in each
    for mask in STAGES:
        assert len({F.column_tile(mask, K) for K in K_SWEEP}) >= 2, mask
    # the pitch rule the thresholds rest on is the library's
    for K in K_SWEEP + [FUSED_LIMIT + 1, 1024]:
        assert F.level_pitch(K) == oa.level_pitch(K) and F.level_pitch(K + 1) == oa.level_pitch(K + 1)
    # VertMix accepts more layers than the fused column pass it is usually fed by
    assert FUSED_LIMIT < F.MIX_MAX_ROWS


@pytest.mark.parametrize("K", K_SWEEP)
def test_layer_ranges_hold_every_kind_that_exists(K):
    c = Col(named_mesh(MESH), K, "linear")
    lo, hi = c.lo[: c.n_all], c.hi[: c.n_all]
    assert np.all((lo >= 0) & (lo <= hi) & (hi < K))  # the generator is valid at this K: no column is dropped
    n = hi - lo + 1
    assert (n == K).any() and (n == 1).any()
    if K > 1:
        assert ((lo > 0) & (hi == K - 1)).any()   # KMin > 0, to the bottom
        assert ((lo == 0) & (hi < K - 1)).any()   # short
    assert np.array_equal(c.vc.get("MinLayerCell"), c.lo) and np.array_equal(c.vc.get("MaxLayerCell"), c.hi)
    m = c.mesh
    assert (m.get_array("CellsOnEdge")[: m.NEdgesAll] == m.NCellsAll).any()  # the coast sees the sentinel cell
    want = R.min_max_layer(m.get_array("CellsOnEdge"), m.NEdgesAll, c.lo, c.hi, K)
    for name, w in zip(("MinLayerEdgeTop", "MinLayerEdgeBot", "MaxLayerEdgeTop", "MaxLayerEdgeBot"), want):
        assert np.array_equal(c.vc.get(name), w), name


@pytest.mark.parametrize("K", K_SWEEP)
def test_fused_pass_bit_exact(K):
    kind = _eos_kind(K)
    c = Col(named_mesh(MESH), K, kind)
    seq = Col(named_mesh(MESH), K, kind)
    # no SpecVolDisplaced; one level down; two up; a displacement of the whole column and beyond, both ways
    for kdisp, ti, si in ((None, 0, 1), (1, 1, 2), (-2, 1, 2), (K, 0, 1), (-(K + 3), 1, 2)):
        c.poison()
        c.run_fused(kdisp, ti, si)
        got, want = c.outputs(), c.expected(kdisp, ti, si)
        for name in ("PressureInterface", "PressureMid", "SpecVol", "SpecVolDisplaced", "ZInterface", "ZMid",
                     "GeopotentialMid", "LayerThicknessTarget"):
            same(got[name], want[name], f"{name} (kdisp {kdisp})")  # NaN wherever the pass must not write
        if kdisp is None:
            assert np.all(np.isnan(got["SpecVolDisplaced"]))
        else:
            assert np.all(got["SpecVolDisplaced"][c.n_all] == 0.0)  # sentinel row
        assert np.all(got["SpecVol"][c.n_all] == 0.0)
        seq.poison()
        seq.run_sequence(kdisp, ti, si)
        for name, v in seq.outputs().items():
            same(got[name], v, f"{name} (fused vs sequence, kdisp {kdisp})")


@pytest.mark.parametrize("K", K_SWEEP)
def test_every_single_stage_launch_bit_exact(K):
    kind = _eos_kind(K)
    c = Col(named_mesh(MESH), K, kind)
    ti, si = 1, 2
    hp = c.state.device_ptr(0)
    tp, sp = oa.tracer_rows_ptr(c.tracers, ti), oa.tracer_rows_ptr(c.tracers, si)
    want = c.nan_state()
    # each launch on its own, every output read back before the next stage runs
    c.vc.compute_pressure(hp, c.ps)
    oa.device_synchronize()
    R.pressure(c.h, c.ps, c.lo, c.hi, c.n_all, RHO0, want["PressureInterface"], want["PressureMid"])
    same(c.vc.get("PressureInterface"), want["PressureInterface"], "PressureInterface")
    same(c.vc.get("PressureMid"), want["PressureMid"], "PressureMid")
    # the equation of state reads every level: a pressure array without NaN, in dbar
    p = np.random.default_rng(3).uniform(0.0, 6000.0, (c.n_size, K))
    c.eos.compute_spec_vol(tp, sp, p)
    sv = R.eos_spec_vol(kind, c.tr[ti], c.tr[si], p, c.n_all)
    same(c.eos.get("SpecVol"), sv, "SpecVol")
    assert np.all(np.isnan(c.eos.get("SpecVolDisplaced")))
    for kdisp in (1, -1, K, -(K + 1)):
        c.eos.set("SpecVolDisplaced", np.full((c.n_size, K), np.nan))
        c.eos.compute_spec_vol_disp(tp, sp, p, kdisp)
        same(c.eos.get("SpecVolDisplaced"), R.eos_spec_vol(kind, c.tr[ti], c.tr[si], p, c.n_all, kdisp),
             f"SpecVolDisplaced (kdisp {kdisp})")
    same(c.eos.get("SpecVol"), sv, "SpecVol (after the displaced launches)")
    c.vc.compute_zheight(hp, c.eos.device_ptr("SpecVol"))
    oa.device_synchronize()
    R.zheight(c.h, sv, c.bot, c.lo, c.hi, c.n_all, RHO0, want["ZInterface"], want["ZMid"])
    same(c.vc.get("ZInterface"), want["ZInterface"], "ZInterface")
    same(c.vc.get("ZMid"), want["ZMid"], "ZMid")
    assert np.all(np.isnan(c.vc.get("GeopotentialMid")))
    c.vc.compute_geopotential(c.tidal, c.sal)
    oa.device_synchronize()
    R.geopotential(want["ZMid"], c.tidal, c.sal, c.lo, c.hi, c.n_all, want["GeopotentialMid"])
    same(c.vc.get("GeopotentialMid"), want["GeopotentialMid"], "GeopotentialMid")
    # target thickness with both movement weights
    for weights in ("Uniform", "Fixed"):
        t = c if weights == "Uniform" else Col(named_mesh(MESH), K, kind, weights="Fixed")
        if t is not c:
            t.vc.compute_pressure(t.state.device_ptr(0), t.ps)
        t.vc.compute_target_thickness()
        oa.device_synchronize()
        tgt = np.full((c.n_size, K), np.nan)
        R.target_thickness(want["PressureInterface"], c.ref, R.movement_weights(weights, K), c.lo, c.hi, c.n_all,
                           RHO0, tgt)
        same(t.vc.get("LayerThicknessTarget"), tgt, f"LayerThicknessTarget ({weights})")
    same(c.vc.get("PressureInterface"), want["PressureInterface"], "PressureInterface (at the end)")


def test_fused_pass_beyond_the_lds_tile_is_refused_and_writes_nothing():
    K = FUSED_LIMIT + 1
    assert K <= F.MIX_MAX_ROWS  # a layer count VertMix itself accepts
    c = Col(named_mesh(MESH), K, "teos10")
    for kdisp in (None, 1):
        with pytest.raises(oa.OmegaAmdError, match=rf"NVertLayers {K} is too long for the LDS tile"):
            c.run_fused(kdisp, 0, 1)
    oa.device_synchronize()
    for name, v in c.outputs().items():
        assert np.all(np.isnan(v)), name
    # the single-stage launches need less LDS and still run at this K
    c.vc.compute_pressure(c.state.device_ptr(0), c.ps)
    oa.device_synchronize()
    want = c.nan_state()
    R.pressure(c.h, c.ps, c.lo, c.hi, c.n_all, RHO0, want["PressureInterface"], want["PressureMid"])
    same(c.vc.get("PressureInterface"), want["PressureInterface"], "PressureInterface")
    same(c.vc.get("PressureMid"), want["PressureMid"], "PressureMid")
