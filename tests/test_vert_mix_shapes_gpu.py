"""VertMix at every launch shape the implicit solves branch on: NVertLayers from 1 to 1024 (256 columns per workgroup
down to one column on 1024 lanes, workgroups with up to 63 pad lanes, 0 to 10 PCR levels) times the number of
right-hand sides (every chunk 1, 2, 4, 6, 8 uncapped, every LDS cap the rule can produce binding, one pass and many),
on columns that are ragged on purpose.  Results equal tests/vert_mix_reference.py bit for bit and the merged tracer
pass equals one PCR diffusion solve per tracer.  Which (columns per workgroup, lanes, chunk, passes, LDS bytes) a case
lands on is asserted from the launch rule restated in tests/vert_fixtures.py, and the sweep asserts its own coverage.
N^2 and the coefficients are swept over the small layer counts, padded MaxEdges and cells of valence 5 and 7."""
import numpy as np
import pytest

import omega_amd as oa
from tests import vert_fixtures as F
from tests import vert_mix_reference as R
from tests.meshes import named_mesh
from tests.vert_fixtures import Mix, same

pytestmark = pytest.mark.gpu

MESH = "fib300_coast_ragged"  # 251 cells, land, valence 5 / 6 / 7
DT = 1800.0
COLUMN_LIMIT = F.column_limit(F.FUSED | F.STAGE_SPEC_VOL_DISP)  # beyond it there is no column pass to feed VertMix
K_SWEEP = [1, 2, 3, 5, 15, 16, 17, 51, 64, 85, 86, 128, 129, 255, 256, 257, 410, 512, 513, 586, 683, 1024]

# (K, NTracers) -> (Sys, Threads, Chunk, passes, dynamic LDS bytes) the launch rule gives
TRACER_CASES = {
    (1, 1): (256, 256, 1, 1, 12288), (1, 5): (256, 256, 6, 1, 32768), (2, 2): (128, 256, 2, 1, 16384),
    (3, 3): (85, 256, 4, 1, 24480), (5, 9): (51, 256, 8, 2, 40800), (15, 6): (17, 256, 6, 1, 32640),
    (16, 37): (16, 256, 8, 5, 40960), (17, 2): (15, 256, 2, 1, 16320), (51, 3): (5, 256, 4, 1, 24480),
    (64, 5): (4, 256, 6, 1, 32768), (85, 1): (3, 256, 1, 1, 12240), (86, 9): (2, 192, 8, 2, 27520),
    (128, 37): (2, 256, 8, 5, 40960), (129, 3): (1, 192, 4, 1, 12384), (129, 6): (1, 192, 6, 1, 16512),
    (255, 2): (1, 256, 2, 1, 16320), (256, 9): (1, 256, 8, 2, 40960), (257, 5): (1, 320, 6, 1, 32896),
    (410, 9): (1, 448, 6, 2, 52480), (410, 6): (1, 448, 6, 1, 52480), (512, 6): (1, 512, 6, 1, 65536),
    (512, 37): (1, 512, 6, 7, 65536), (513, 5): (1, 576, 4, 2, 49248), (586, 5): (1, 640, 4, 2, 56256), (586, 3): (1, 640, 4, 1, 56256),
    (683, 37): (1, 704, 2, 19, 43712), (683, 3): (1, 704, 2, 2, 43712), (1024, 1): (1, 1024, 1, 1, 49152),
    (1024, 2): (1, 1024, 2, 1, 65536), (1024, 6): (1, 1024, 2, 3, 65536),
}
STRONG_ZERO_CASES = [(3, 2), (17, 6), (129, 3), (512, 6), (1024, 6)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    oa.device_init(0)


def _shape(K, nt):
    s = F.mix_launch(K, nt)
    return (s["Sys"], s["Threads"], s["Chunk"], s["Passes"], s["LdsBytes"])


def test_sweep_covers_every_launch_branch():
    shapes = {c: F.mix_launch(*c) for c in TRACER_CASES}
    for c, want in TRACER_CASES.items():
        assert _shape(*c) == want, c
        assert shapes[c]["LdsBytes"] <= F.LDS_BYTES
    assert {K for K, _ in TRACER_CASES} == set(K_SWEEP)
    assert {nt for _, nt in TRACER_CASES} == {1, 2, 3, 5, 6, 9, 37}
    assert {(512, 6), (1024, 2), (1024, 6), (683, 37)} <= set(TRACER_CASES)
    # every chunk value where the LDS limit does not bind, and every cap the rule can produce binding
    assert {s["Chunk"] for s in shapes.values() if not s["Capped"]} == set(F.MIX_CHUNKS)
    caps = {F.mix_launch(K, 8)["Chunk"] for K in range(1, F.MIX_MAX_ROWS + 1)} - {8}
    assert caps == {6, 4, 2}
    assert {s["Chunk"] for s in shapes.values() if s["Capped"]} == caps
    for cap in caps:  # the first K at which each cap binds is in the sweep
        assert min(K for K in range(1, F.MIX_MAX_ROWS + 1) if F.mix_launch(K, 8)["Chunk"] == cap) in K_SWEEP
    # NTracers a multiple of the chunk and not, one pass and many, for capped and uncapped chunks
    # (an uncapped chunk below 8 is a single pass, and no NTracers of the sweep is a multiple of 8)
    for capped in (False, True):
        sel = [(c, s) for c, s in shapes.items() if s["Capped"] == capped]
        assert any(c[1] % s["Chunk"] == 0 and (s["Passes"] > 1 or not capped) for c, s in sel), capped
        assert any(c[1] % s["Chunk"] != 0 and s["Passes"] > 1 for c, s in sel), capped
    assert any(s["Passes"] == 1 and c[1] < s["Chunk"] for c, s in shapes.items())  # a partly filled single pass
    # columns per workgroup from 256 to 1, workgroups with many pad lanes, every PCR level count, the full LDS
    assert {s["Sys"] for s in shapes.values()} >= {256, 128, 85, 51, 17, 16, 15, 5, 4, 3, 2, 1}
    assert max(s["PadLanes"] for s in shapes.values()) == 63
    assert {s["Levels"] for s in shapes.values()} == set(range(11))
    assert sum(s["LdsBytes"] == F.LDS_BYTES for s in shapes.values()) >= 3
    assert all(F.mix_launch(K, 1)["Chunk"] == 1 for K in K_SWEEP)  # the velocity solve: one right-hand side


def _rig(K, nt, coef="computed", seed=11):
    """A Mix on ragged columns with VertDiff / VertVisc in place.  computed: from the column pass and compute() where
    the column pass exists, else random; strong_zero: the convective value (1.0 m2/s over layers of 0.5 m) on some
    interfaces, exactly 0 on others (a zero G splits the column into independent systems), background on the rest.
    Entries the solves must not read (every column's top interface and everything outside its range) are NaN."""
    x = Mix(named_mesh(MESH), K, "teos10", ntracers=max(nt, 2), ragged=True, column_pass=K <= COLUMN_LIMIT,
            seed=seed)
    rng = np.random.default_rng(seed + K)
    if coef == "strong_zero":
        x.h = np.where(rng.random(x.h.shape) < 0.5, 0.5, x.h)
        x.state.copy_to_device(x.h, x.un, 0)
    if coef == "computed" and K <= COLUMN_LIMIT:
        x.compute()
        visc, diff = x.vm.get("VertVisc"), x.vm.get("VertDiff")
    elif coef == "computed":
        visc, diff = rng.uniform(1.0e-5, 1.0e-2, (2, x.n_size, K))
    else:
        pick = rng.integers(0, 3, (2, x.n_size, K))
        visc, diff = np.where(pick == 0, 0.0, np.where(pick == 1, 1.0, 1.0e-5))
    k = np.arange(K)[None, :]
    ok = (x.lo >= 0) & (x.lo <= x.hi) & (x.hi < K)
    inside = ok[:, None] & (k > x.lo[:, None]) & (k <= x.hi[:, None])
    visc, diff = np.where(inside, visc, np.nan), np.where(inside, diff, np.nan)
    x.vm.set("VertVisc", visc)
    x.vm.set("VertDiff", diff)
    return x, visc, diff


def _check_ragged(x, K):
    """the depths the sweep is about occur among the owned columns, side by side in local order"""
    n = np.where((x.lo >= 0) & (x.lo <= x.hi) & (x.hi < K), x.hi - x.lo + 1, 0)[: x.n_own]
    assert set(np.unique(n)) == set(F.ragged_depths(K))
    per_wg = F.mix_launch(K, 1)["Sys"]
    if per_wg >= 7:
        first = n[: per_wg]
        assert set(np.unique(first)) == set(F.ragged_depths(K))  # from land and one level to all K in one workgroup


def _tracer_case(K, nt, coef):
    x, _, diff = _rig(K, nt, coef)
    _check_ragged(x, K)
    t0, t1 = x.seeded_tracers()
    x.vm.apply_tracers(x.state.device_ptr(0, 0), x.tracers.device_ptr(0), nt, DT)
    oa.device_synchronize()
    got = x.tracers.copy_to_host(0)
    want = R.tracer_mix(x.h, diff, t0, nt, DT, x.lo, x.hi, x.n_own)
    same(got, want, "tracers (level 0)")
    same(x.tracers.copy_to_host(1), t1, "tracers (level 1)")
    if K > 1:
        assert not np.array_equal(want[:nt], t0[:nt], equal_nan=True)  # the solve changed something
    # the merged pass against one PCR diffusion solve per tracer and column depth, through the array launcher
    n = np.where((x.lo >= 0) & (x.lo <= x.hi) & (x.hi < K), x.hi - x.lo + 1, 0)[: x.n_own]
    for depth in np.unique(n[n > 0]):
        cols = np.nonzero(n == depth)[0]
        lev = x.lo[cols][:, None] + np.arange(depth)[None, :]
        c = cols[:, None]
        for t in range(nt):
            g, hh, xx = R.assemble(x.h[c, lev], diff[c, lev], t0[t][c, lev], DT)
            sep = oa.tridiag_diff_solve(g, hh, xx, "pcr")
            assert np.array_equal(got[t][c, lev], sep), f"tracer {t}, depth {depth}"
    return x, got, t0


@pytest.mark.parametrize("K,nt", sorted(TRACER_CASES))
def test_tracer_solve_bit_exact(K, nt):
    _tracer_case(K, nt, "computed")


@pytest.mark.parametrize("K,nt", STRONG_ZERO_CASES)
def test_tracer_solve_strong_and_zero_coefficients(K, nt):
    x, got, t0 = _tracer_case(K, nt, "strong_zero")
    g = (1.0 * DT) / 0.5
    assert g / 0.5 > 1.0e3  # G / H of the convective interfaces over the thin layers
    assert np.all(np.isfinite(got[:nt][~np.isnan(t0[:nt])]))


@pytest.mark.parametrize("K,coef",
                         [(K, "computed") for K in K_SWEEP] + [(K, "strong_zero") for K in (2, 17, 129, 1024)])
def test_velocity_solve_bit_exact(K, coef):
    x, visc, _ = _rig(K, 2, coef)
    u0, u1, lo, hi = x.seeded_velocity()
    x.vm.apply_velocity(x.state.device_ptr(0, 0), x.state.device_ptr(1, 0), DT)
    oa.device_synchronize()
    want = R.velocity_mix(x.h, visc, u0, DT, x.mesh.get_array("CellsOnEdge"), lo, hi, x.e_own)
    _, got0 = x.state.copy_to_host(0)
    _, got1 = x.state.copy_to_host(1)
    same(got0, want, "normal velocity (level 0)")
    same(got1, u1, "normal velocity (level 1)")
    n = np.where((lo >= 0) & (lo <= hi) & (hi < K), hi - lo + 1, 0)[: x.e_own]
    assert (n == 0).any() and (n > 0).any()  # empty edge ranges (coast, land) beside solved ones
    if K > 1:
        assert (n > 1).any()


N2_CASES = [(MESH, 1), (MESH, 2), (MESH, 3), (MESH, 5), (MESH, 15), (MESH, 16), (MESH, 17), (MESH, 257),
            ("fib300_pad8_coast_ragged", 17), ("fib300_pad8_coast_ragged", 3)]


@pytest.mark.parametrize("mesh,K", N2_CASES)
@pytest.mark.parametrize("ragged", [False, True])
def test_bvf_and_coefficients_bit_exact(mesh, K, ragged):
    padded = "_pad8" in mesh
    keep = oa.get_option("KeepMaxEdges")
    if padded:  # keep the file's maxEdges = 8 as the table width: rows of EdgesOnCell longer than any cell's valence
        oa.set_option("KeepMaxEdges", 1)
    try:
        x = Mix(named_mesh(mesh), K, "teos10", ragged=ragged)
    finally:
        oa.set_option("KeepMaxEdges", keep)
    nec = x.mesh.get_array("NEdgesOnCell")[: x.n_all]
    assert (nec == 5).any() and (nec == 7).any()  # the shear gather loops over cells of each valence
    assert x.mesh.get_array("EdgesOnCell").shape[1] == (8 if padded else 7)
    x.compute()
    n2 = x.expected_bvf()
    same(x.vm.get("BruntVaisalaFreqSq"), n2, "BruntVaisalaFreqSq")
    depth = np.where(x.hi >= x.lo, x.hi - x.lo + 1, 0)[: x.n_all]
    assert np.count_nonzero(n2) <= int(np.sum(np.maximum(depth - 1, 0)))  # at most one value per interior interface
    if K == 1:
        assert not n2.any()
    else:
        assert n2.any()
    visc, diff = x.expected_coefficients(x.un, x.ut, n2)
    same(x.vm.get("VertVisc"), visc, "VertVisc")
    same(x.vm.get("VertDiff"), diff, "VertDiff")
    if K == 1:
        assert not visc.any() and not diff.any()
    other = n2 * 0.5 - 1.0e-5  # the caller's N^2 instead of the object's own
    x.vm.compute(x.un, x.ut, bvf=other)
    oa.device_synchronize()
    visc, diff = x.expected_coefficients(x.un, x.ut, other)
    same(x.vm.get("VertVisc"), visc, "VertVisc (caller's N2)")
    same(x.vm.get("VertDiff"), diff, "VertDiff (caller's N2)")
