"""Shared by the BarotropicMode tests (CPU: tests/test_barotropic.py, GPU: tests/test_barotropic_gpu.py,
tests/test_c_abi_barotropic.py, and through tests/split_explicit_fixtures.py the split-explicit ones): a rank's mesh
arrays as the restatement reads them, the closed planar basin, and the NaN-seeded rig of the calls on random inputs."""
import numpy as np

import omega_amd as oa
from omega_amd.meshgen import cull, planar_hex
from tests import barotropic_reference as BR
from tests.rank_rig import RankRig
from tests.vert_fixtures import mix_inputs, same

GRAVITY = 9.80616


def btr_mesh(mesh, bottom_depth):
    """BR.BtrMesh of an oa.HorzMesh (host arrays only: works on a host-only mesh)"""
    g = mesh.get_array
    return BR.BtrMesh(mesh.NCellsAll, mesh.NEdgesAll, g("CellsOnEdge"), g("NEdgesOnCell"), g("EdgesOnCell"),
                      g("EdgeSignOnCell"), g("NEdgesOnEdge"), g("EdgesOnEdge"), g("WeightsOnEdge"), g("FEdge"),
                      g("DvEdge"), g("DcEdge"), g("AreaCell"), np.ascontiguousarray(g("EdgeMask")[:, 0]), bottom_depth)


def closed_basin(nx, ny, dc, f0, depth, walls="xy"):
    """A flat-bottomed planar basin of hexagons: the periodic mesh with its row 0 (walls across y) and, with "x" in
    `walls`, its column 0 (walls across x) removed.  Rows are straight lines of cells dc*sqrt(3)/2 apart, so the
    basin is L = (ny - 1)*dc*sqrt(3)/2 long in y, from half a row spacing below row 1 to half above row ny - 1;
    `y0` is its lower wall."""
    g0 = planar_hex(nx, ny, dc, f0=f0, bottom_depth=depth)
    row, col = np.arange(nx * ny) // nx, np.arange(nx * ny) % nx
    keep = row != 0
    if "x" in walls:
        keep &= col != 0
    g = cull(g0, keep)
    dy = dc * np.sqrt(3.0) / 2.0
    g["basin_dy"], g["basin_L"] = dy, (ny - 1) * dy
    g["basin_y0"] = g0["yCell"][nx] - 0.5 * dy  # row 1 is the first row of water
    return g


class BtrRig(RankRig):
    """One rank's VertCoord and BarotropicMode on random global inputs in local order, NaN on the rows >= N*All (layer
    ranges with land and KMin > 0 from tests.vert_fixtures.mix_inputs, `full`: every layer active).  A subclass with
    other fields overrides `draw`."""

    EDGE_1D = ("BtrVelocity", "BtrThickEdge", "BtrForcing", "BtrFluxMean")

    def __init__(self, g, K, nparts=1, rank=0, full=False, seed=7):
        super().__init__(g, K, nparts, rank)
        m = self.mesh
        G = mix_inputs(g, K, seed, full, 2)
        self.h, self.u = self.cells(G["h"], np.nan), self.edges(G["un"], np.nan)
        self.draw(np.random.default_rng(seed + 50), int(g["nCells"]), int(g["nEdges"]))
        self.layers(G["min_level"], G["max_level"])
        self.vc.set("BottomDepth", self.bot)
        self.coe = m.get_array("CellsOnEdge")
        self.M = btr_mesh(m, self.bot)
        self.bm = oa.BarotropicMode(m, self.vc)
        for name in self.EDGE_1D + ("SSH", "BclVelocity"):
            assert np.all(self.bm.get(name) == 0.0)  # zero at construction

    def draw(self, rng, nc, ne):
        """the rig's own fields, in the order of its draws"""
        K = self.K
        bot, ssh, vel = rng.uniform(100.0, 6000.0, nc), rng.uniform(-0.5, 0.5, nc), rng.uniform(-0.1, 0.1, ne)
        forcing, tend = rng.uniform(-1.0e-5, 1.0e-5, ne), rng.uniform(-1.0e-5, 1.0e-5, (ne, K))
        self.tend = self.edges(tend, np.nan)
        self.bot, self.ssh0 = self.cells(bot, np.nan), self.cells(ssh, np.nan)
        self.vel0, self.forcing0 = self.edges(vel, np.nan), self.edges(forcing, np.nan)
        shut = self.mesh.get_array("EdgeMask")[: self.e_all, 0] == 0.0
        self.vel0[: self.e_all][shut] = 0.0  # no flow through a shut edge

    def poison(self):
        for name in self.EDGE_1D:
            self.bm.set(name, np.full(self.e_size, np.nan))
        self.bm.set("SSH", np.full(self.n_size, np.nan))
        oa.copy_to_device(self.bm.device_ptr("BclVelocity"), np.full((self.e_size, oa.level_pitch(self.K)), np.nan))

    def bcl_padded(self):
        return self.raw(self.bm.device_ptr("BclVelocity"), (self.e_size, oa.level_pitch(self.K)))

    def state(self):
        return {n: self.bm.get(n) for n in self.EDGE_1D + ("SSH",)} | {"BclVelocity": self.bcl_padded()}

    def nan_state(self):
        out = {n: np.full(self.e_size, np.nan) for n in self.EDGE_1D}
        out["SSH"] = np.full(self.n_size, np.nan)
        out["BclVelocity"] = np.full((self.e_size, self.K), np.nan)
        return out

    def check(self, want, what):
        got = self.state()
        for n in want:
            same(got[n], self.padded(want[n]) if n == "BclVelocity" else want[n], f"{n} ({what})")

    def load_2d(self):
        """SSH, BtrVelocity, BtrForcing on the local elements, NaN beyond; BtrFluxMean NaN everywhere"""
        self.poison()
        self.bm.set("SSH", self.ssh0), self.bm.set("BtrVelocity", self.vel0), self.bm.set("BtrForcing", self.forcing0)
        return self.ssh0.copy(), self.vel0.copy(), self.forcing0.copy(), np.full(self.e_size, np.nan)


class HostRig:
    """One rank's mesh (host-only unless `device`) with the restatement's view of it, K levels, all active"""

    def __init__(self, g, K=1, nparts=1, rank=0, device=False):
        self.g, self.K = g, K
        self.decomp = oa.Decomp(oa.GlobalMesh(g), nparts, rank, 3)
        self.mesh = m = oa.HorzMesh(self.decomp, K, host_only=not device)
        self.nc, self.ne, self.nc_size, self.ne_size = m.NCellsAll, m.NEdgesAll, m.NCellsSize, m.NEdgesSize
        self.bottom = m.get_array("BottomDepth")
        self.M = btr_mesh(m, self.bottom)
        self.area = m.get_array("AreaCell")
        self.angle = m.get_array("AngleEdge")
        self.x_edge, self.y_edge = m.get_array("XEdge"), m.get_array("YEdge")
        self.y_cell = m.get_array("YCell")

    def zeros(self):
        return np.zeros(self.nc_size), np.zeros(self.ne_size), np.zeros(self.ne_size), np.zeros(self.ne_size)
