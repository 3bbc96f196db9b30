"""BarotropicMode on the GPU: every call equals the NumPy restatement of the contract (tests/barotropic_reference.py)
bit for bit on NaN-seeded arrays -- entries outside the ranges, the row padding, rows >= N*All and the sentinel row are
NaN and must stay so; the combined split + SSH launch equals the two calls; subcycle at odd and even counts (both
parities of the double buffers), subcycle(2) against two subcycle(1); the stream and null-stream forms agree; no call
allocates; bad arguments are refused; a 2-part decomposition gives the 1-part bits."""
import numpy as np
import pytest

import omega_amd as oa
from tests import barotropic_reference as BR
from tests.barotropic_fixtures import GRAVITY, BtrRig
from tests.column_reference import RHO0
from tests.meshes import named_mesh
from tests.vert_fixtures import same as _same

pytestmark = pytest.mark.gpu

MESHES = ("hex24x20", "ico2", "fib700_coast_ragged")
LEVELS = (1, 3, 16, 17, 65)  # compact rows, odd pitch, whole lines, padded rows, more levels than a wavefront
DT = 20.0


@pytest.fixture(scope="module", autouse=True)
def _device():
    oa.device_init(0)


@pytest.mark.parametrize("K", LEVELS)
@pytest.mark.parametrize("mesh", MESHES)
def test_column_calls_bit_exact_on_nan_seeded_arrays(mesh, K):
    x = BtrRig(named_mesh(mesh), K)
    h, u, t = x.seeded(x.h), x.seeded(x.u, edge=True), x.seeded(x.tend, edge=True)
    bh, bu, bt = x.dev(h), x.dev(u), x.dev(t)
    # splitVelocity alone
    x.poison()
    x.bm.split_velocity(bh.ptr, bu.ptr)
    oa.device_synchronize()
    want = x.nan_state()
    BR.split_velocity(h, u, x.coe, x.lo_e, x.hi_e, x.e_all, want["BtrThickEdge"], want["BtrVelocity"], want["BclVelocity"])
    x.check(want, "splitVelocity")
    _same(bu.to_host(), x.padded(u), "NormalVelocity handed in")
    assert np.isfinite(want["BclVelocity"][x.e_active]).all() and x.e_active.any()
    if K > 1:
        assert np.abs(want["BclVelocity"][x.e_active]).max() > 0.0
    # computeSSH alone, on top
    x.bm.compute_ssh(bh.ptr)
    oa.device_synchronize()
    BR.compute_ssh(h, x.bot, x.lo, x.hi, x.n_all, want["SSH"])
    x.check(want, "computeSSH")
    split_and_ssh = {k: v.copy() for k, v in want.items()}
    # computeForcing: BtrForcing and nothing else
    x.bm.compute_forcing(bh.ptr, bt.ptr)
    oa.device_synchronize()
    BR.compute_forcing(h, t, x.coe, x.lo_e, x.hi_e, x.e_all, want["BtrForcing"])
    x.check(want, "computeForcing")
    assert np.abs(want["BtrForcing"][: x.e_all]).max() > 0.0
    # recombine into a NaN array: the ranges and nothing else
    out = x.dev(np.full((x.e_size, K), np.nan))
    x.bm.recombine(out.ptr)
    oa.device_synchronize()
    back = BR.recombine(np.full((x.e_size, K), np.nan), want["BtrVelocity"], want["BclVelocity"], x.lo_e, x.hi_e, x.e_all)
    _same(out.to_host(), x.padded(back), "recombine")
    x.check(want, "after recombine")
    # the combined launch: the bits of the two calls
    x.poison()
    x.bm.split_velocity(bh.ptr, bu.ptr, with_ssh=True)
    oa.device_synchronize()
    x.check(split_and_ssh, "splitVelocityAndSSH")
    if "coast" in mesh:
        empty = ~x.e_active[: x.e_all].any(axis=1)
        assert empty.any() and (~x.active[: x.n_all]).all(axis=1).any()
        assert sorted(set(x.mesh.get_array("NEdgesOnCell")[: x.n_all])) == [5, 6, 7]
        if K > 2:
            assert (x.lo_e[: x.e_all][~empty] > 0).any()
    # the numpy form of the binding
    got = x.bm.recombine(np.zeros((x.e_size, K)))
    _same(got, BR.recombine(np.zeros((x.e_size, K)), want["BtrVelocity"], want["BclVelocity"], x.lo_e, x.hi_e, x.e_all), "numpy form")


@pytest.mark.parametrize("nsub", [1, 2, 7])
@pytest.mark.parametrize("mesh", MESHES)
def test_subcycle_bit_exact(mesh, nsub):
    x = BtrRig(named_mesh(mesh), 3)
    ssh, vel, forcing, flux = x.load_2d()
    x.bm.subcycle(nsub, DT)
    oa.device_synchronize()
    BR.subcycle(x.M, ssh, vel, forcing, flux, nsub, DT, GRAVITY)
    want = x.nan_state()
    want.update(SSH=ssh, BtrVelocity=vel, BtrForcing=forcing, BtrFluxMean=flux)
    x.check(want, f"subcycle({nsub})")
    assert np.isfinite(ssh[: x.n_all]).all() and np.isfinite(vel[: x.e_all]).all() and np.isfinite(flux[: x.e_all]).all()
    assert not np.array_equal(ssh[: x.n_all], x.ssh0[: x.n_all]) and not np.array_equal(vel[: x.e_all], x.vel0[: x.e_all])
    shut = x.M.mask[: x.e_all] == 0.0
    if "coast" in mesh:
        assert shut.any()
    assert np.all(vel[: x.e_all][shut] == 0.0) and np.all(flux[: x.e_all][shut] == 0.0)
    if mesh != "hex24x20":
        assert np.abs(x.M.cor[: x.e_all]).max() > 0.0 and len(set(np.abs(x.mesh.get_array("FEdge")[: x.e_all]))) > 10


def test_two_sub_steps_are_two_calls_of_one():
    x = BtrRig(named_mesh("fib700_coast_ragged"), 3)
    x.load_2d()
    x.bm.subcycle(2, DT)
    oa.device_synchronize()
    two = x.state()
    x.load_2d()
    x.bm.subcycle(1, DT)
    oa.device_synchronize()
    f1 = x.bm.get("BtrFluxMean")
    x.bm.subcycle(1, DT)
    oa.device_synchronize()
    one = x.state()
    _same(one["SSH"], two["SSH"], "SSH")
    _same(one["BtrVelocity"], two["BtrVelocity"], "BtrVelocity")
    # subcycle(1) leaves F/1 = F; subcycle(2) leaves ((0 + F1) + F2)/2
    _same(two["BtrFluxMean"], (f1 + one["BtrFluxMean"]) / 2.0, "BtrFluxMean")


def test_stream_and_null_stream_forms_agree():
    g = named_mesh("fib700_coast_ragged")
    s = oa.Stream()
    out = []
    for st in (None, s):
        x = BtrRig(g, 17)
        bh, bu, bt = x.dev(x.h), x.dev(x.u), x.dev(x.tend)
        x.poison()
        x.bm.split_velocity(bh.ptr, bu.ptr, stream=st)
        x.bm.compute_ssh(bh.ptr, stream=st)
        x.bm.compute_forcing(bh.ptr, bt.ptr, stream=st)
        x.bm.split_velocity(bh.ptr, bu.ptr, with_ssh=True, stream=st)
        r = x.dev(np.full((x.e_size, 17), np.nan))
        x.bm.recombine(r.ptr, stream=st)
        if st is not None:
            st.synchronize()
        oa.device_synchronize()
        a = x.state()
        x.load_2d()
        x.bm.subcycle(3, DT, stream=st)
        if st is not None:
            st.synchronize()
        oa.device_synchronize()
        out.append(list(a.values()) + [r.to_host()] + list(x.state().values()))
    for p, q in zip(*out):
        _same(q, p, "stream form")


def test_no_call_allocates():
    x = BtrRig(named_mesh("hex24x20"), 16)
    bh, bu, bt, r = x.dev(x.h), x.dev(x.u), x.dev(x.tend), x.dev(x.u)

    def calls():
        x.bm.split_velocity(bh.ptr, bu.ptr)
        x.bm.compute_ssh(bh.ptr)
        x.bm.split_velocity(bh.ptr, bu.ptr, with_ssh=True)
        x.bm.compute_forcing(bh.ptr, bt.ptr)
        x.bm.subcycle(3, DT)
        x.bm.recombine(r.ptr)
        oa.device_synchronize()

    calls()
    before = oa.device_resource_count()
    calls()
    assert oa.device_resource_count() == before


def test_refusals():
    g = named_mesh("hex24x20")
    x, y = BtrRig(g, 16), BtrRig(g, 15)
    with pytest.raises(oa.OmegaAmdError, match="another mesh"):
        oa.BarotropicMode(x.mesh, y.vc)
    with pytest.raises(oa.OmegaAmdError, match="VertCoord is NULL"):
        oa.BarotropicMode(x.mesh, None)
    short = oa.VertCoord(x.mesh, 8, RHO0, "Uniform")
    with pytest.raises(oa.OmegaAmdError, match="another layer count"):
        oa.BarotropicMode(x.mesh, short)
    host = oa.HorzMesh(x.decomp, 16, host_only=True)
    with pytest.raises(oa.OmegaAmdError, match="host-only"):
        oa.BarotropicMode(host, x.vc)
    for nsub in (0, -3):
        with pytest.raises(oa.OmegaAmdError, match=f"NSub = {nsub}"):
            x.bm.subcycle(nsub, DT)
    for dt in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(oa.OmegaAmdError, match="DtBtr"):
            x.bm.subcycle(1, dt)
    with pytest.raises(oa.OmegaAmdError, match="no array named"):
        x.bm.get("NoSuchArray")


def test_the_longest_column_and_the_refusal_above_it():
    limit = oa.BarotropicMode.max_layers()
    assert limit >= 1024
    g = named_mesh("hex24x20")
    decomp = oa.Decomp(oa.GlobalMesh(g), 1, 0, 3)
    for K, ok in ((limit, True), (limit + 1, False)):
        m = oa.HorzMesh(decomp, K)
        vc = oa.VertCoord(m, K, RHO0, "Uniform", decomp=decomp)
        if not ok:
            with pytest.raises(oa.OmegaAmdError, match=f"NVertLayers <= {limit}"):
                oa.BarotropicMode(m, vc)
            continue
        bm = oa.BarotropicMode(m, vc)
        rng = np.random.default_rng(1)
        nc, ne, n_all, e_all = m.NCellsSize, m.NEdgesSize, m.NCellsAll, m.NEdgesAll
        h, u = rng.uniform(0.5, 40.0, (nc, K)), rng.uniform(-0.05, 0.05, (ne, K))
        bm.split_velocity(h, u, with_ssh=True)
        lo, hi = np.zeros(nc, np.int32), np.full(nc, K - 1, np.int32)
        lo[n_all:], hi[n_all:] = -1, -1
        lo_e, hi_e = vc.get("MinLayerEdgeBot"), vc.get("MaxLayerEdgeTop")
        thick, btr, bcl = np.zeros(ne), np.zeros(ne), np.zeros((ne, K))
        BR.split_velocity(h, u, m.get_array("CellsOnEdge"), lo_e, hi_e, e_all, thick, btr, bcl)
        _same(bm.get("BtrThickEdge"), thick, "BtrThickEdge at the longest column")
        _same(bm.get("BtrVelocity"), btr, "BtrVelocity at the longest column")
        _same(bm.get("BclVelocity"), bcl, "BclVelocity at the longest column")
        _same(bm.get("SSH"), BR.compute_ssh(h, vc.get("BottomDepth"), lo, hi, n_all, np.zeros(nc)), "SSH at the longest column")


@pytest.mark.parametrize("mesh,K", [("hex24x20", 17), ("fib700_coast_ragged", 16)])
def test_two_part_decomposition_matches_one_part(mesh, K):
    """Compared per global id.  Column calls: every local cell (a column needs nothing but itself), and every local
    edge both of whose cells are local (EdgeMask != 0 on the rank: an edge on the rim of the halo lacks a cell, so its
    range is empty there and not on one part).  subcycle(1): owned cells and owned edges only -- a sub-step reaches two
    cells out, which the 3 halo layers hold, while the halo's own results lack their outer neighbours."""
    g = named_mesh(mesh)

    def run(nparts, rank):
        x = BtrRig(g, K, nparts=nparts, rank=rank)
        bh, bu, bt = x.dev(x.h), x.dev(x.u), x.dev(x.tend)
        x.bm.split_velocity(bh.ptr, bu.ptr, with_ssh=True)
        x.bm.compute_forcing(bh.ptr, bt.ptr)
        r = x.dev(np.zeros((x.e_size, K)))
        x.bm.recombine(r.ptr)
        oa.device_synchronize()
        col = x.state() | {"Recombined": r.to_host()}
        x.load_2d()
        x.bm.subcycle(1, DT)
        oa.device_synchronize()
        return x, col, x.state()

    one, col1, sub1 = run(1, 0)
    cell1 = {int(c): i for i, c in enumerate(one.cid[: one.n_all])}
    edge1 = {int(e): i for i, e in enumerate(one.eid[: one.e_all])}
    for rank in (0, 1):
        x, col, sub = run(2, rank)
        assert x.n_own < one.n_own and x.n_all > x.n_own
        ci = np.array([cell1[int(c)] for c in x.cid[: x.n_all]])
        _same(col["SSH"][: x.n_all], col1["SSH"][ci], f"SSH rank {rank}")
        inner = np.nonzero(x.M.mask[: x.e_all] != 0.0)[0]
        ei = np.array([edge1[int(e)] for e in x.eid[inner]])
        for n in ("BtrThickEdge", "BtrVelocity", "BtrForcing", "BclVelocity", "Recombined"):
            _same(col[n][inner], col1[n][ei], f"{n} rank {rank}")
        co, eo = ci[: x.n_own], np.array([edge1[int(e)] for e in x.eid[: x.e_own]])
        _same(sub["SSH"][: x.n_own], sub1["SSH"][co], f"SSH after subcycle rank {rank}")
        for n in ("BtrVelocity", "BtrFluxMean"):
            _same(sub[n][: x.e_own], sub1[n][eo], f"{n} after subcycle rank {rank}")
