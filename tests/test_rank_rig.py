"""tests/rank_rig.py without a device: the scatter to local order, the restated layer ranges and their masks, the
device layout of `padded` and the NaN seeding of `seeded` -- what every column and edge physics rig builds on -- on a
periodic mesh and a coast mesh, at compact rows (K = 1), an odd pitch (3), whole lines (16) and padded rows (17), on one
part and on rank 1 of two.  The layer ranges are those of tests.vert_fixtures.mix_inputs, which most rigs draw."""
import functools

import numpy as np
import pytest

from tests import barotropic_reference as BR
from tests import pressure_grad_reference as PR
from tests import vert_adv_reference as VR
from tests.meshes import named_mesh
from tests.rank_rig import RankRig
from tests.vert_fixtures import level_pitch, mix_inputs

CASES = [(mesh, K, nparts, rank) for mesh in ("hex24x20", "fib300_coast_ragged") for K in (1, 3, 16, 17)
         for nparts, rank in ((1, 0), (2, 1))]
NT = 3


@functools.lru_cache(maxsize=None)
def rig(mesh, K, nparts, rank):
    g = named_mesh(mesh)
    x = RankRig(g, K, nparts, rank, device=False)
    x.G = mix_inputs(g, K, 7, False, 2)
    x.layers(x.G["min_level"], x.G["max_level"])
    return x, int(g["nCells"]), int(g["nEdges"])


@pytest.mark.parametrize("mesh,K,nparts,rank", CASES)
def test_scatter_puts_each_global_row_in_its_local_row_and_fill_in_the_rest(mesh, K, nparts, rank):
    x, nc, ne = rig(mesh, K, nparts, rank)
    assert (nparts == 1) == (x.n_all == nc)  # the second case really is a part of the mesh
    assert x.n_own <= x.n_all < x.n_size and x.e_own <= x.e_all < x.e_size
    rng = np.random.default_rng(3)
    for scatter, n, n_all, n_size, ids in ((x.cells, nc, x.n_all, x.n_size, x.cid), (x.edges, ne, x.e_all, x.e_size, x.eid)):
        for shape, axis in (((n,), 0), ((n, K), 0), ((NT, n, K), 1)):
            a = rng.uniform(1.0, 2.0, shape)
            for fill in (0.0, np.nan):
                got = np.moveaxis(scatter(a, fill) if fill != 0.0 else scatter(a), axis, 0)
                src = np.moveaxis(a, axis, 0)
                assert got.shape == (n_size,) + src.shape[1:]
                for i in range(n_all):
                    assert np.array_equal(got[i], src[ids[i] - 1])
                rest = got[n_all:]
                assert rest.size > 0 and (np.isnan(rest).all() if np.isnan(fill) else np.all(rest == 0.0))


@pytest.mark.parametrize("mesh,K,nparts,rank", CASES)
def test_masks_are_the_levels_lo_to_hi_of_each_local_row(mesh, K, nparts, rank):
    x, _, _ = rig(mesh, K, nparts, rank)
    for mask, lo, hi, n_all, n_size in ((x.active, x.lo, x.hi, x.n_all, x.n_size),
                                        (x.e_active, x.lo_e, x.hi_e, x.e_all, x.e_size)):
        want = np.zeros((n_size, K), bool)
        for i in range(n_all):
            for k in range(lo[i], hi[i] + 1):
                want[i, k] = True
        assert mask.dtype == bool and np.array_equal(mask, want)
        assert len(lo) == len(hi) == n_size
        # the three restatements' own masks are one function
        for f in (PR.range_mask, BR.range_mask, VR.active_mask):
            assert np.array_equal(f(lo, hi, n_all, K), want[:n_all])
    # the cell ranges are the global ones, 0-based, in local order
    mn, mx = x.G["min_level"], x.G["max_level"]
    for i in range(x.n_all):
        assert (x.lo[i], x.hi[i]) == (mn[x.cid[i] - 1] - 1, mx[x.cid[i] - 1] - 1)
    # an edge's levels are those active in both of its cells
    coe = x.mesh.get_array("CellsOnEdge")
    for e in range(x.e_all):
        assert np.array_equal(x.e_active[e], x.active[coe[e, 0]] & x.active[coe[e, 1]])


@pytest.mark.parametrize("mesh,K,nparts,rank", CASES)
def test_the_ranges_hold_the_kinds_the_rigs_rely_on(mesh, K, nparts, rank):
    x, _, _ = rig(mesh, K, nparts, rank)
    n_cell, n_edge = x.active[: x.n_all].sum(axis=1), x.e_active[: x.e_all].sum(axis=1)
    assert (n_cell == 0).any() and (n_edge == 0).any()  # land, and edges next to it
    assert (n_edge == 1).any() and (x.lo_e[: x.e_all][n_edge == 1] == x.hi_e[: x.e_all][n_edge == 1]).all()  # Lo == Hi
    assert (n_cell == K).any() and (n_edge == K).any()  # full columns


@pytest.mark.parametrize("mesh,K,nparts,rank", CASES)
def test_padded_is_the_device_layout_with_nan_in_the_padding(mesh, K, nparts, rank):
    x, _, _ = rig(mesh, K, nparts, rank)
    P = level_pitch(K)
    assert P == {1: 1, 3: 3, 16: 16, 17: 32}[K]
    rng = np.random.default_rng(4)
    for shape in ((x.n_size, K), (x.e_size, K), (NT, x.n_size, K)):
        a = rng.uniform(1.0, 2.0, shape)
        pad = x.padded(a)
        assert pad.shape == shape[:-1] + (P,) and pad.flags.c_contiguous
        assert np.array_equal(pad[..., :K], a) and np.isnan(pad[..., K:]).all()
        assert np.all(x.padded(a, fill=-3.25)[..., K:] == -3.25)


@pytest.mark.parametrize("mesh,K,nparts,rank", CASES)
def test_seeded_is_nan_exactly_outside_the_ranges(mesh, K, nparts, rank):
    x, _, _ = rig(mesh, K, nparts, rank)
    rng = np.random.default_rng(5)
    for edge, mask, n_size in ((False, x.active, x.n_size), (True, x.e_active, x.e_size)):
        for shape in ((n_size, K), (NT, n_size, K)):
            a = rng.uniform(1.0, 2.0, shape)
            s = x.seeded(a, edge=edge)
            assert s.shape == shape
            assert np.array_equal(np.isnan(s), np.broadcast_to(~mask, shape))
            assert np.array_equal(s[..., mask], a[..., mask])
            assert np.isfinite(a).all()  # the input is left alone
