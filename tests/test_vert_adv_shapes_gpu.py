"""The VertAdv column launch at every tile it branches on: a sweep of NVertLayers over both sides of the thresholds of
vertAdvColumnTile (16, 8, 4, 2 columns per workgroup) up to the longest column it accepts, then the refusal.  At each K
the transport scan, the thickness update and the combined launch equal tests/vert_adv_reference.py bit for bit on
NaN-seeded arrays (the first third of tests/test_vert_adv_gpu.py::test_bit_exact_on_nan_seeded_arrays, whose own K stop
at 80: tile 16).  Which tile a case lands on is computed from the rule restated in tests/vert_fixtures.py, and the sweep
asserts that it covers every tile."""
import numpy as np
import pytest

import omega_amd as oa
from tests import vert_adv_reference as VR
from tests import vert_fixtures as F
from tests.column_reference import RHO0
from tests.meshes import named_mesh
from tests.vert_adv_fixtures import AdvRig, assert_both_signs
from tests.vert_fixtures import same

pytestmark = pytest.mark.gpu

MESH = "fib300_coast_ragged"  # 251 cells, land, valence 5 / 6 / 7
# T * (3 * LP + 1) <= 8192 doubles with LP = levelPitch(K) | 1: tile 16 up to K = 160, 8 up to 336, 4 up to 672, 2 up
# to 1360
K_SWEEP = [160, 161, 336, 337, 672, 673, 1360]
LIMIT = 1360


@pytest.fixture(scope="module", autouse=True)
def _device():
    oa.device_init(0)


def test_sweep_covers_every_tile_of_the_column_launch():
    """the thresholds come from the restated LDS rule, so a layout change moves the sweep's claim with it"""
    assert F.vert_adv_limit() == LIMIT == oa.VertAdv.max_layers()
    assert {F.vert_adv_tile(K) for K in K_SWEEP} == {16, 8, 4, 2}
    for tile in (16, 8, 4):  # both sides of each threshold
        last = max(K for K in range(1, LIMIT + 1) if F.vert_adv_tile(K) == tile)
        assert last in K_SWEEP and last + 1 in K_SWEEP, (tile, last)
        assert F.vert_adv_tile(last + 1) == tile // 2
    assert F.vert_adv_tile(LIMIT) == 2 and F.vert_adv_tile(LIMIT + 1) is None
    for K in K_SWEEP + [LIMIT + 1]:  # the pitch rule the thresholds rest on is the library's
        assert F.level_pitch(K) == oa.level_pitch(K)


@pytest.mark.parametrize("K", K_SWEEP)
def test_column_launch_bit_exact_at_every_tile(K):
    x = AdvRig(named_mesh(MESH), K, 1)
    # the fixture still holds every kind of column at this K: full, one layer, KMin > 0, land
    lo, hi = x.lo[: x.n_all], x.hi[: x.n_all]
    ok = (lo >= 0) & (lo <= hi) & (hi < K)
    n = np.where(ok, hi - lo + 1, 0)
    assert (n == K).any() and (n == 1).any() and (ok & (lo > 0)).any() and (~ok).any()
    d = x.seeded(x.d)
    want_wt = x.want_transport(d)
    assert assert_both_signs(want_wt, x.lo, x.hi, x.n_all) > 0
    # the transport, and nothing else
    for order in (2, 1):
        x.poison_transport(order)
        buf = x.dev(d)
        x.va[order].compute_transport(buf.ptr)
        oa.device_synchronize()
        same(x.transport_padded(order), x.padded(want_wt), "VerticalTransport")
        same(buf.to_host(), x.padded(d), "the tendency handed in")
    assert np.isfinite(want_wt[x.active]).all() and x.active.any()
    # the thickness update from the transport as it stands
    buf = x.dev(d)
    x.va[2].add_thickness(buf.ptr)
    oa.device_synchronize()
    want_th = VR.add_thickness_tend(d.copy(), want_wt, x.lo, x.hi, x.n_all)
    same(buf.to_host(), x.padded(want_th), "LayerThicknessTend")
    same(x.transport_padded(), x.padded(want_wt), "VerticalTransport after addThicknessTend")
    # the combined launch
    x.poison_transport()
    buf = x.dev(d)
    x.va[2].compute_transport(buf.ptr, add_thickness=True)
    oa.device_synchronize()
    same(buf.to_host(), x.padded(want_th), "LayerThicknessTend (combined launch)")
    same(x.transport_padded(), x.padded(want_wt), "VerticalTransport (combined launch)")
    assert not np.array_equal(want_th[x.active], d[x.active])


def test_one_layer_beyond_the_lds_tile_is_refused():
    K = LIMIT + 1
    decomp = oa.Decomp(oa.GlobalMesh(named_mesh(MESH)), 1, 0, 3)
    m = oa.HorzMesh(decomp, K)
    vc = oa.VertCoord(m, K, RHO0, "Uniform", decomp=decomp)
    with pytest.raises(oa.OmegaAmdError, match=rf"NVertLayers = {K} is outside the supported 1 <= NVertLayers <= {LIMIT} "):
        oa.VertAdv(m, vc, 2)
