"""The rig under the column and edge physics rigs: one rank's mesh with global inputs in local order, the layer ranges
of cells and edges restated on the host, and NaN everywhere a kernel must not write.  A subclass adds its component
objects and its random draws; what "local order", "inside the ranges" and "the device layout" mean is stated here,
once.

Local order: local row i < N*All holds global row ID[i] - 1; the rows from N*All on (the sentinel row among them)
belong to no element.  Level-indexed device arrays are [rows][levelPitch(K)]: `padded` is that layout with NaN in the
row padding, `seeded` a host array with NaN outside the ranges, `raw` device memory read back padding and all."""
import numpy as np

import omega_amd as oa
from tests import column_reference as CR
from tests import pressure_grad_reference as PR
from tests.column_reference import RHO0


def raw(ptr, shape):
    """raw device memory as a host array of doubles (row padding and sentinel row included); a failed copy raises"""
    buf = np.empty(shape)
    oa._chk(oa.lib().omg_copy_to_host(buf.ctypes.data_as(oa.C.c_void_p), oa.C.c_void_p(ptr), oa.C.c_size_t(buf.nbytes)))
    return buf


def _scatter(x, rows, n_size, fill):
    if x.ndim == 3:  # a stack [NT][n][K]
        return np.stack([_scatter(t, rows, n_size, fill) for t in x])
    out = np.full((n_size,) + x.shape[1:], fill)
    out[: len(rows)] = x[rows]
    return out


class RankRig:
    """Decomp and HorzMesh of one rank (host-only unless `device`), the counts owned / all / size of cells (n_*) and
    edges (e_*), the 1-based global ids `cid` / `eid` and the global rows `crow` / `erow` of the local elements"""

    raw = staticmethod(raw)

    def __init__(self, g, K, nparts=1, rank=0, halo=3, device=True):
        self.K, self.device = K, device
        self.decomp = oa.Decomp(oa.GlobalMesh(g), nparts, rank, halo)
        self.mesh = m = oa.HorzMesh(self.decomp, K, host_only=not device)
        self.n_own, self.n_all, self.n_size = m.NCellsOwned, m.NCellsAll, m.NCellsSize
        self.e_own, self.e_all, self.e_size = m.NEdgesOwned, m.NEdgesAll, m.NEdgesSize
        self.cid, self.eid = self.decomp.get_array("CellID"), self.decomp.get_array("EdgeID")
        self.crow, self.erow = self.cid[: self.n_all] - 1, self.eid[: self.e_all] - 1

    def cells(self, x, fill=0.0):
        """a global per-cell array -- [n], [n][K] or a stack [NT][n][K] -- in local order, `fill` on the rows >=
        NCellsAll"""
        return _scatter(x, self.crow, self.n_size, fill)

    def edges(self, x, fill=0.0):
        """a global per-edge array in local order, `fill` on the rows >= NEdgesAll"""
        return _scatter(x, self.erow, self.e_size, fill)

    def layers(self, min_level, max_level, rho0=RHO0, weights="Uniform"):
        """From the global 1-based (minLevelCell, maxLevelCell): the cell ranges lo, hi, the edge ranges lo_e, hi_e
        (the levels active in both cells of an edge) and the in-range masks active [NCellsSize][K], e_active
        [NEdgesSize][K], False on the rows >= N*All -- all restated on the host.  With a device, `vc`: a VertCoord on
        the same global ranges, whose own four range arrays must equal the restatement."""
        K = self.K
        self.lo, self.hi = CR.local_layer_ranges(self.cid, min_level, max_level, self.n_all, self.n_size, K)
        self.lo_e, self.hi_e = PR.edge_ranges(self.mesh.get_array("CellsOnEdge"), self.e_all, self.lo, self.hi, K)
        self.active = np.zeros((self.n_size, K), bool)
        self.active[: self.n_all] = PR.range_mask(self.lo, self.hi, self.n_all, K)
        self.e_active = np.zeros((self.e_size, K), bool)
        self.e_active[: self.e_all] = PR.range_mask(self.lo_e, self.hi_e, self.e_all, K)
        if self.device:
            self.vc = oa.VertCoord(self.mesh, K, rho0, weights, min_level, max_level, decomp=self.decomp)
            for name, want in (("MinLayerCell", self.lo), ("MaxLayerCell", self.hi), ("MinLayerEdgeBot", self.lo_e),
                               ("MaxLayerEdgeTop", self.hi_e)):
                assert np.array_equal(self.vc.get(name), want), name

    def padded(self, a, fill=np.nan):
        """the device layout of a level-indexed host array of any leading shape, `fill` in the row padding"""
        pad = np.full(a.shape[:-1] + (oa.level_pitch(self.K),), fill)
        pad[..., : self.K] = a
        return pad

    def dev(self, a):
        return oa.DeviceBuffer(self.padded(a))

    def seeded(self, a, edge=False):
        """`a` inside the ranges, NaN everywhere else -- other levels, land, rows >= N*All, the sentinel row"""
        m = self.e_active if edge else self.active
        out = np.full(a.shape, np.nan)
        out[..., m] = a[..., m]
        return out
