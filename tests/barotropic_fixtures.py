"""Shared by the BarotropicMode tests (CPU: tests/test_barotropic.py, GPU: tests/test_barotropic_gpu.py,
tests/test_c_abi_barotropic.py): a rank's mesh arrays as the restatement reads them, the closed planar basin, and the
random inputs."""
import numpy as np

import omega_amd as oa
from omega_amd.meshgen import cull, planar_hex
from tests import barotropic_reference as BR

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
