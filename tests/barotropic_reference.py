"""NumPy restatement of the BarotropicMode numerical contract (omega_amd/csrc/BarotropicMode.h).

Every output is the FP64 evaluation order the contract states; the library is built with -ffp-contract=off, so the
device results equal these bit for bit.  The sequential sums are vectorised across edges / cells, one level or one slot
at a time: each element still sees its own additions in the stated order.

Arrays are host arrays in the library's local order: cell arrays [NCellsSize] or [NCellsSize][K], edge arrays
[NEdgesSize] or [NEdgesSize][K].  The column functions write into the arrays they are given and leave every entry the
contract does not name as it was; entries outside the ranges may hold anything, NaN included, and are never used.
`BtrMesh` holds what the sub-steps read of a mesh.
"""
import numpy as np


def _ranges(lo, hi, n, K):
    lo, hi = np.asarray(lo[:n]), np.asarray(hi[:n])
    return lo, hi, (lo >= 0) & (lo <= hi) & (hi < K)


def range_mask(lo, hi, n, K):
    """[n][K] True on the levels of each row's range (an invalid range: none)"""
    lo, hi, ok = _ranges(lo, hi, n, K)
    k = np.arange(K)[None, :]
    return ok[:, None] & (k >= lo[:, None]) & (k <= hi[:, None])


def _edge_means(h, field, cells_on_edge, lo_e, hi_e, n_edges_all):
    """(Sum, mean, ok): the contract's two ascending sums and SumHF/Sum -- the level's own value on a range of one
    level; 0, 0 on an empty range"""
    n, K = n_edges_all, h.shape[1]
    lo, hi, ok = _ranges(lo_e, hi_e, n, K)
    coe = np.asarray(cells_on_edge)[:n]
    ok = ok & (coe >= 0).all(axis=1) & (coe < h.shape[0]).all(axis=1)
    rows = np.nonzero(ok)[0]
    c0, c1 = coe[rows, 0], coe[rows, 1]
    total, weighted = np.zeros(n), np.zeros(n)
    for k in range(K):
        sel = (lo[rows] <= k) & (k <= hi[rows])
        r = rows[sel]
        h_e = 0.5 * (h[c0[sel], k] + h[c1[sel], k])
        total[r] = total[r] + h_e
        weighted[r] = weighted[r] + h_e * field[r, k]
    mean = np.zeros(n)
    with np.errstate(all="ignore"):
        mean[rows] = weighted[rows] / total[rows]
    one = rows[lo[rows] == hi[rows]]  # the mean of one level is that level, bit for bit
    mean[one] = field[one, lo[one]]
    return total, mean, ok


def split_velocity(h, u, cells_on_edge, lo_e, hi_e, n_edges_all, btr_thick, btr_vel, bcl_vel):
    """BtrThickEdge, BtrVelocity on every edge < NEdgesAll; BclVelocity = u - BtrVelocity on Lo .. Hi"""
    n, K = n_edges_all, h.shape[1]
    total, mean, ok = _edge_means(h, u, cells_on_edge, lo_e, hi_e, n)
    btr_thick[:n], btr_vel[:n] = total, mean
    m = range_mask(lo_e, hi_e, n, K) & ok[:, None]
    with np.errstate(all="ignore"):
        val = u[:n] - mean[:, None]
    bcl_vel[:n][m] = val[m]
    return btr_thick, btr_vel, bcl_vel


def compute_forcing(h, vel_tend, cells_on_edge, lo_e, hi_e, n_edges_all, btr_forcing):
    btr_forcing[:n_edges_all] = _edge_means(h, vel_tend, cells_on_edge, lo_e, hi_e, n_edges_all)[1]
    return btr_forcing


def compute_ssh(h, bottom_depth, lo, hi, n_cells_all, ssh):
    """SSH[c] = (ascending sum of h over KMin .. KMax) - BottomDepth[c]; land columns are not written"""
    n, K = n_cells_all, h.shape[1]
    lo, hi, ok = _ranges(lo, hi, n, K)
    rows = np.nonzero(ok)[0]
    s = np.zeros(n)
    for k in range(K):
        r = rows[(lo[rows] <= k) & (k <= hi[rows])]
        s[r] = s[r] + h[r, k]
    ssh[rows] = s[rows] - np.asarray(bottom_depth)[rows]
    return ssh


def recombine(u, btr_vel, bcl_vel, lo_e, hi_e, n_edges_all):
    n, K = n_edges_all, u.shape[1]
    m = range_mask(lo_e, hi_e, n, K)
    with np.errstate(all="ignore"):
        val = bcl_vel[:n] + np.asarray(btr_vel)[:n, None]
    u[:n][m] = val[m]
    return u


def cor_weight(weights_on_edge, edges_on_edge, n_edges_on_edge, f_edge, n_edges_all):
    """CorWeight[e][j] = WeightsOnEdge[e][j]*FEdge[EdgesOnEdge[e][j]]; 0 for j >= NEdgesOnEdge[e] and where the slot
    names no local edge"""
    eoe = np.asarray(edges_on_edge)
    out = np.zeros(np.asarray(weights_on_edge).shape)
    n = n_edges_all
    j = np.arange(eoe.shape[1])[None, :]
    valid = (j < np.asarray(n_edges_on_edge)[:n, None]) & (eoe[:n] >= 0) & (eoe[:n] < n)
    safe = np.where(valid, eoe[:n], 0)
    out[:n] = np.where(valid, np.asarray(weights_on_edge)[:n] * np.asarray(f_edge)[safe], 0.0)
    return out


class BtrMesh:
    """What the sub-steps read: connectivity, DvEdge, EdgeSignOnCell, AreaCell, DcEdge, EdgeMask, CorWeight,
    BottomDepth; `n_cells_all`, `n_edges_all` the local counts."""

    def __init__(self, n_cells_all, n_edges_all, cells_on_edge, n_edges_on_cell, edges_on_cell, edge_sign_on_cell,
                 n_edges_on_edge, edges_on_edge, weights_on_edge, f_edge, dv_edge, dc_edge, area_cell, edge_mask,
                 bottom_depth):
        a = np.asarray
        self.nc, self.ne = int(n_cells_all), int(n_edges_all)
        self.coe, self.neoc, self.eoc, self.sign = a(cells_on_edge), a(n_edges_on_cell), a(edges_on_cell), a(edge_sign_on_cell)
        self.neoe, self.eoe = a(n_edges_on_edge), a(edges_on_edge)
        self.dv, self.area, self.mask = a(dv_edge, float), a(area_cell, float), a(edge_mask, float)
        self.inv_dc = 1.0 / a(dc_edge, float)[: self.ne]
        self.inv_area = 1.0 / self.area[: self.nc]
        self.bottom = a(bottom_depth, float)
        self.cor = cor_weight(weights_on_edge, edges_on_edge, n_edges_on_edge, f_edge, self.ne)
        coe = self.coe[: self.ne]
        self.open = (self.mask[: self.ne] != 0.0) & (coe >= 0).all(axis=1) & (coe < self.nc).all(axis=1)

    def flux(self, ssh, vel):
        """F[e]; 0.0 exactly on an edge with EdgeMask 0, which reads no cell"""
        f = np.zeros(self.ne)
        e = np.nonzero(self.open)[0]
        c0, c1 = self.coe[e, 0], self.coe[e, 1]
        f[e] = self.mask[e] * ((0.5 * ((ssh[c0] + self.bottom[c0]) + (ssh[c1] + self.bottom[c1]))) * vel[e])
        return f

    def divergence(self, f):
        """the chain of DivergenceOnCell on a one-level edge field"""
        div = np.zeros(self.nc)
        cells = np.arange(self.nc)
        for j in range(self.eoc.shape[1]):
            r = cells[j < self.neoc[: self.nc]]
            e = self.eoc[r, j]
            ok = (e >= 0) & (e < self.ne)
            fe = np.where(ok, f[np.where(ok, e, 0)], 0.0)
            dvs = np.where(ok, self.dv[np.where(ok, e, 0)] * self.sign[r, j], 0.0)
            div[r] = div[r] - (dvs * fe) * self.inv_area[r]
        return div

    def coriolis(self, vel):
        cor = np.zeros(self.ne)
        edges = np.arange(self.ne)
        for j in range(self.eoe.shape[1]):
            ej = self.eoe[: self.ne, j]
            r = edges[(j < self.neoe[: self.ne]) & (ej >= 0) & (ej < self.ne)]
            cor[r] = cor[r] + self.cor[r, j] * vel[self.eoe[r, j]]
        return cor


def substep(M, ssh, vel, forcing, flux_sum, dt, gravity):
    """one forward-backward sub-step, in place on ssh, vel and flux_sum (rows < N*All only)"""
    nc, ne = M.nc, M.ne
    f = M.flux(ssh, vel)
    ssh_n = ssh[:nc] - dt * M.divergence(f)
    e = np.nonzero(M.open)[0]
    c0, c1 = M.coe[e, 0], M.coe[e, 1]
    cor = M.coriolis(vel)
    vel_n = vel[:ne].copy()
    vel_n[e] = vel[e] + dt * (M.mask[e] * ((cor[e] - gravity * ((ssh_n[c1] - ssh_n[c0]) * M.inv_dc[e])) + forcing[e]))
    flux_sum[:ne] = flux_sum[:ne] + f
    ssh[:nc], vel[:ne] = ssh_n, vel_n


def subcycle(M, ssh, vel, forcing, flux_mean, nsub, dt, gravity=9.80616):
    """BtrFluxMean = 0; nsub sub-steps; BtrFluxMean = BtrFluxMean/nsub.  In place; returns (ssh, vel, flux_mean)"""
    flux_mean[: M.ne] = 0.0
    for _ in range(nsub):
        substep(M, ssh, vel, forcing, flux_mean, dt, gravity)
    flux_mean[: M.ne] = flux_mean[: M.ne] / float(nsub)
    return ssh, vel, flux_mean
