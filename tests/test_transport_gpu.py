"""Tendencies::computeTransportTendencies on the GPU: the fused transport half equals the two group calls
(compute_thickness_tendencies, then compute_tracer_tendencies) bit for bit on every local row, halo included, and writes
nothing else of the tendency arrays; on the small cases the CPU oracle is compared too, so the check does not rest on GPU
code alone.  The yardstick of every case: poison the tendency arrays with NaN, run the pair, read back; poison again, run
the fused call; the raw device arrays -- row padding, sentinel row and NormalVelocityTend included -- must be the pair's
values on [:, :NCellsAll, :K] and the poison everywhere else.

The thickness is read from time level 0 and the velocity from time level 1, which holds another velocity (both signs
flipped on every other edge, so both upwind directions occur); the thickness of level 1 is NaN."""
import itertools

import numpy as np
import pytest

import omega_amd as oa
from tests.meshes import named_mesh
from tests.problem import Problem, poison_tendencies
from tests.rank_rig import raw
from tests.split_explicit_fixtures import StepRig
from tests.vert_adv_fixtures import adv_inputs

pytestmark = pytest.mark.gpu

FLAGS = ("ThicknessFluxTendencyEnable", "TracerHorzAdvTendencyEnable", "TracerDiffTendencyEnable",
         "TracerHyperDiffTendencyEnable")
EDGE_AUX = ("FluxLayerThickEdge", "MeanLayerThickEdge", "HTracersEdge")
STEP_DT = 20.0


@pytest.fixture(scope="module", autouse=True)
def _device():
    oa.device_init(0)


def bits_equal(a, b):
    """the same 64 bits (so -0 differs from +0), or NaN on both sides"""
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def assert_bits(got, want, name):
    assert got.shape == want.shape, name
    bad = ~bits_equal(np.ascontiguousarray(got), np.ascontiguousarray(want))
    assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


def raw_tendency(P, which):
    """the whole device array (planes, rows, pitch), row padding included"""
    ptr, _ = P.tend.device_ptr(which)
    rows = P.mesh.NEdgesSize if which == 1 else P.mesh.NCellsSize
    return raw(ptr, (max(P.NT, 1) if which == 2 else 1, rows, oa.level_pitch(P.K)))  # as poison_tendencies lays them out


def second_level(P):
    """time level 1: another velocity, a NaN thickness (not to be read)"""
    m = P.mesh
    P.u1 = P.u * np.where(np.arange(m.NEdgesSize) % 2, -0.75, 0.75)[:, None]
    h1 = np.zeros_like(P.h)
    h1[: m.NCellsAll] = np.nan
    P.state.copy_to_device(h1, P.u1, 1)


def pair(P):
    P.tend.compute_thickness_tendencies(P.state, P.aux, 0, 1)
    P.tend.compute_tracer_tendencies(P.state, P.aux, P.tracers, 0, 0, 1)


def fused(P):
    P.tend.compute_transport_tendencies(P.state, P.aux, P.tracers, 0, 0, 1)


def check_fused_against_pair(P, oracle=False, before_fused=None):
    """the yardstick; returns the pair's raw arrays"""
    m, K, n = P.mesh, P.K, P.mesh.NCellsAll
    if not hasattr(P, "u1"):
        second_level(P)
    poison_tendencies(P)
    oa.device_synchronize()
    poison = [raw_tendency(P, w) for w in range(3)]
    pair(P)
    oa.device_synchronize()
    want = [raw_tendency(P, w) for w in range(3)]
    assert_bits(want[1], poison[1], "NormalVelocityTend after the group calls")
    own = m.NCellsOwned
    assert np.isfinite(want[0][0, :own, :K]).all()
    if P.NT > 0:
        assert np.isfinite(want[2][:, :own, :K]).all()
    poison_tendencies(P)
    if before_fused:
        before_fused()
    fused(P)
    oa.device_synchronize()
    got = [raw_tendency(P, w) for w in range(3)]
    for w, name in ((0, "LayerThicknessTend"), (2, "TracerTend")):
        expect = poison[w].copy()
        if w == 0 or P.NT > 0:
            expect[:, :n, :K] = want[w][:, :n, :K]
        assert_bits(got[w], expect, name)  # every local row, halo included; padding, rows >= NCellsAll: poison
    assert_bits(got[1], poison[1], "NormalVelocityTend")
    if oracle:
        hT = P.oracle.compute_thickness_tendencies(P.h, P.u1)
        assert_bits(got[0][0, :own, :K], hT[:own], "LayerThicknessTend against the oracle")
        if P.NT > 0:
            trT = P.oracle.compute_tracer_tendencies(P.h, P.u1, P.tr)
            assert_bits(got[2][:, :own, :K], trT[:, :own], "TracerTend against the oracle")
    return want


# ---------------------------------------------------------------------------------------------------------------------
# arithmetic and options
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eddy4", [0.0, 3.0e9])
@pytest.mark.parametrize("upwind", [0, 1])
@pytest.mark.parametrize("flags", list(itertools.product((0, 1), repeat=4)), ids=lambda f: "".join(map(str, f)))
def test_every_option(flags, upwind, eddy4):
    cfg = dict(zip(FLAGS, flags), FluxThicknessUpwind=upwind, FluxTracerUpwind=upwind, EddyDiff4=eddy4)
    P = Problem(named_mesh("hex16x16"), 4, 2, config=cfg)
    hyper = flags[3]
    rng = np.random.default_rng(5)
    seed = {name: rng.uniform(1.0, 2.0, P.aux._shape(name)) for name in EDGE_AUX + ("Del2TracersCell",)}

    def seed_aux():
        for name, v in seed.items():
            P.aux.set(name, v)

    check_fused_against_pair(P, oracle=True, before_fused=seed_aux)
    for name in EDGE_AUX:  # the deviation of the contract: the edge-located arrays are not materialised
        assert_bits(P.aux.get(name), seed[name], name)
    d2 = P.aux.get("Del2TracersCell")
    if hyper:
        n = P.mesh.NCellsAll
        pair(P)
        oa.device_synchronize()
        assert_bits(d2[:, :n], P.aux.get("Del2TracersCell")[:, :n], "Del2TracersCell")
        assert_bits(d2[:, n:], seed["Del2TracersCell"][:, n:], "Del2TracersCell beyond NCellsAll")
    else:
        assert_bits(d2, seed["Del2TracersCell"], "Del2TracersCell with the hyperdiffusion term off")


def test_a_non_finite_del2_propagates_with_eddy_diff4_zero():
    """EddyDiff4 = 0 takes no shortcut: 0 * Inf of the group call is NaN here too (checked by the yardstick), and the
    tracer tendency is NaN next to the cell"""
    P = Problem(named_mesh("hex16x16"), 4, 2, config=dict(EddyDiff4=0.0))
    P.tr[0, 7, 1] = np.inf
    P.tracers.copy_to_device(P.tr, 0)
    second_level(P)
    poison_tendencies(P)
    pair(P)
    oa.device_synchronize()
    want = raw_tendency(P, 2)
    poison_tendencies(P)
    fused(P)
    oa.device_synchronize()
    n, K = P.mesh.NCellsAll, P.K
    got = raw_tendency(P, 2)
    assert_bits(got[:, :n, :K], want[:, :n, :K], "TracerTend")
    assert np.isnan(got[0, :n, 1]).sum() > 1 and np.isfinite(got[1, :n, :K]).all()


# ---------------------------------------------------------------------------------------------------------------------
# mesh classes, halo
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["ico4", "fib1500", "hex24x24_pad8", "hex24x24_perm10", "hex32x32_coast_mixed",
                                  "fib1500_coast_island_raw"])
def test_mesh_classes(mesh):
    check_fused_against_pair(Problem(named_mesh(mesh), 16, 2, config=dict(EddyDiff4=3.0e9)), oracle=True)


@pytest.mark.parametrize("upwind", [0, 1])
@pytest.mark.parametrize("mesh", ["fib1500", "hex32x32"])
def test_two_part_decomposition_every_local_row(mesh, upwind):
    """What the fused path recomputes at the rim of the halo.  The group path reads the edge-located arrays there; the
    fused path goes through CellsOnEdgeOnCell, where a cell that is not local is the zero sentinel cell NCellsAll (the
    same entries the edge kernels read from CellsOnEdge) and where a slot whose edge is the sentinel row NEdgesAll has
    the sentinel cell on both sides (HorzMesh::buildCoefficientTables; Decomp fills the sentinel row of CellsOnEdge
    with NCellsAll).  Decomp makes every edge of every local cell local, so on these meshes the first kind occurs --
    asserted -- and the second does not (printed); every local row is compared either way."""
    for rank in range(2):
        P = Problem(named_mesh(mesh), 16, 2, nparts=2, rank=rank, halo_width=3,
                    config=dict(EddyDiff4=3.0e9, FluxThicknessUpwind=upwind, FluxTracerUpwind=upwind))
        m = P.mesh
        assert m.NCellsAll > m.NCellsOwned
        eoc, nec, coe = m.get_array("EdgesOnCell"), m.get_array("NEdgesOnCell"), m.get_array("CellsOnEdge")
        slots = np.arange(eoc.shape[1])[None, :] < nec[: m.NCellsAll, None]
        edges = eoc[: m.NCellsAll][slots]
        assert np.all(coe[m.NEdgesAll] == m.NCellsAll)  # the sentinel edge's cells are the sentinel cell
        rim = (coe[edges[edges < m.NEdgesAll]] == m.NCellsAll).any(axis=1).sum()
        print(f"{mesh} rank {rank}: {rim} slots with a cell that is not local, {(edges == m.NEdgesAll).sum()} with the sentinel edge")
        assert rim > 0
        check_fused_against_pair(P, oracle=True)


# ---------------------------------------------------------------------------------------------------------------------
# level and launch shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NT", [0, 1, 6, 9])
@pytest.mark.parametrize("K", [1, 3, 16, 17, 60, 64])
def test_level_shapes(K, NT):
    """odd K (one level per lane), K < 16 (the lanes span the column), pitch != K (60 -> 64, 17 -> 32); no tracers, one,
    two whole blocks of the tracer loop, and blocks with a remainder"""
    P = Problem(named_mesh("hex16x16"), K, NT, config=dict(EddyDiff4=3.0e9))
    check_fused_against_pair(P, oracle=True)


# makeGeom(N, K, W = 2, pitch, MaxTY) for these bodies (MaxTY = 16 while NT <= 8, else none), rows of whole lines:
#   K = 32: KV = 16 level pairs, TX = 8, so 2 level chunks; TY = 32, cut to 16 by MaxTY, halved while > 8 and
#   ceil(N/TY) < 4096.  One wavefront per 64 threads: a round of workgroups is Cap = 2048/(TX*TY/64).
#     hex100x100  N = 10 000: 625 tiles of 16 < 4096 -> tile 8, 1250 tiles; 1250 >= 1200: no gridDim.y split; < Cap = 2048:
#                 no tail split
#     hex130x130  N = 16 900: 1057 tiles of 16 < 4096 -> tile 8, 2113 tiles >= Cap = 2048: the last 65 are tail-split
#     hex260x260  N = 67 600: 4225 tiles of 16 >= 4096 -> tile 16, Cap = 1024, 4225 % 1024 = 129 tail-split tiles
#   K = 16, NT = 9: KV = 8 = TX, one chunk, TY = 32 uncut; hex364x364 N = 132 496: 4141 tiles of 32 >= 4096 -> tile 32
@pytest.mark.parametrize("mesh,K,NT", [("hex100x100", 32, 2), ("hex130x130", 32, 2), ("hex260x260", 32, 2),
                                       ("hex364x364", 16, 9)])
def test_launch_shapes(mesh, K, NT):
    P = Problem(named_mesh(mesh), K, NT, config=dict(EddyDiff4=3.0e9), oracle=False)
    check_fused_against_pair(P)


# ---------------------------------------------------------------------------------------------------------------------
# attached terms
# ---------------------------------------------------------------------------------------------------------------------
def test_with_a_vert_adv_attached():
    g, K, nt = named_mesh("hex24x20"), 16, 2
    P = Problem(g, K, nt, oracle=False)
    G = adv_inputs(g, K, nt)
    m = P.mesh
    vc = oa.VertCoord(m, K, 1026.0, "Uniform", G["min_level"], G["max_level"], decomp=P.decomp)
    ref = np.zeros((m.NCellsSize, K))
    ref[: m.NCellsAll] = G["ref"][P.cell_id[: m.NCellsAll] - 1]
    vc.set("RefLayerThickness", ref)
    va = oa.VertAdv(m, vc, 2)
    plain = check_fused_against_pair(P)
    P.tend.attach_vert_adv(va)
    want = check_fused_against_pair(P, before_fused=lambda: va.set("VerticalTransport", np.full((m.NCellsSize, K), np.nan)))
    n = m.NCellsAll
    for w in (0, 2):  # the attached terms changed both tendencies: the comparison above was about them
        assert not bits_equal(want[w][:, :n, :K], plain[w][:, :n, :K]).all()
    P.tend.attach_vert_adv(None)


def test_with_a_custom_thickness_hook_the_group_calls_run():
    from tests import manufactured as ms
    g = named_mesh("hex16x16")
    P = Problem(g, 4, 2, oracle=False)
    wx, wy = ms.wavelengths(g)
    plain = check_fused_against_pair(P)
    P.tend.use_manufactured_solution(P.mesh, wx, wy, ms.ETA0)
    rng = np.random.default_rng(9)
    seed = {name: rng.uniform(1.0, 2.0, P.aux._shape(name)) for name in EDGE_AUX}

    def seed_aux():
        for name, v in seed.items():
            P.aux.set(name, v)

    want = check_fused_against_pair(P, before_fused=seed_aux)
    n = P.mesh.NCellsAll
    assert not bits_equal(want[0][:, :n, : P.K], plain[0][:, :n, : P.K]).all()  # the hook added its term
    for name in EDGE_AUX:  # the fallback materialises what the hook may read
        assert not bits_equal(P.aux.get(name)[..., : P.mesh.NEdgesAll, :], seed[name][..., : P.mesh.NEdgesAll, :]).any(), name
    P.tend.clear_custom_tendencies()


def test_bad_time_levels_are_refused():
    P = Problem(named_mesh("hex16x16"), 4, 2, oracle=False)
    for args in ((0, 2, 0), (0, 0, 2), (0, -1, 0)):
        with pytest.raises(oa.OmegaAmdError, match="bad time level"):
            P.tend.compute_transport_tendencies(P.state, P.aux, P.tracers, *args)
    with pytest.raises(oa.OmegaAmdError, match="time level out of range"):
        P.tend.compute_transport_tendencies(P.state, P.aux, P.tracers, 2, 0, 0)


# ---------------------------------------------------------------------------------------------------------------------
# the stepper
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attached", [False, True], ids=["nothing_attached", "pressure_grad_and_vert_adv"])
@pytest.mark.parametrize("nsub", [1, 7])
def test_split_explicit_steps_are_the_same_bits_either_way(nsub, attached):
    runs = []
    for on in (False, True):
        x = StepRig(attached=attached)
        st = x.stepper("Split-Explicit", STEP_DT, nsub)
        st.set_fused_transport(on)
        st.do_step(x.p.state)
        oa.device_synchronize()
        before = oa.device_resource_count()
        for _ in range(2):
            st.do_step(x.p.state)
        oa.device_synchronize()
        assert oa.device_resource_count() == before  # a step creates no buffer, stream or event
        runs.append((x, x.result()))
    (x, off), (_, on) = runs
    for name, a, b, start in zip(("h", "u", "tracers"), off, on, (x.h, x.u, x.tr)):
        assert np.isfinite(b).all(), name
        assert_bits(b, a, f"{name} after three steps")
        assert not np.array_equal(b, start), name


def test_set_fused_transport_is_for_split_explicit_only():
    x = StepRig()
    with pytest.raises(oa.OmegaAmdError, match="not a Split-Explicit one"):
        x.stepper("RungeKutta4", STEP_DT).set_fused_transport(True)
    st = x.stepper("Split-Explicit", STEP_DT, 2)
    st.set_fused_transport(False)
    st.set_fused_transport(True)
    st.do_step(x.p.state)
    assert all(np.isfinite(r).all() for r in x.result())
