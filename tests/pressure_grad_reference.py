"""NumPy restatement of the PressureGrad numerical contract (omega_amd/csrc/PressureGrad.h).

Every output is the FP64 evaluation order the contract states; the library is built with -ffp-contract=off, so the
device results equal these bit for bit.

Arrays are host arrays in the library's local order: cell arrays [NCellsSize][K], edge arrays [NEdgesSize][K], per-edge
arrays [NEdgesSize]; `n_edges_all` is NEdgesAll.  Nothing outside each edge's level range is written.
"""
import numpy as np

from tests import column_reference as CR


def edge_ranges(cells_on_edge, n_edges_all, min_layer_cell, max_layer_cell, nvertlayers):
    """(MinLayerEdgeBot, MaxLayerEdgeTop): the levels active in both cells of an edge, sized NEdgesAll + 1"""
    _, min_bot, max_top, _ = CR.min_max_layer(cells_on_edge, n_edges_all, min_layer_cell, max_layer_cell, nvertlayers)
    return min_bot, max_top


def range_mask(lo, hi, n_edges_all, nvertlayers):
    """[n_edges_all][K] True on the levels the term applies to (an invalid or empty range: none)"""
    lo, hi = np.asarray(lo[:n_edges_all]), np.asarray(hi[:n_edges_all])
    ok = (lo >= 0) & (lo <= hi) & (hi < nvertlayers)
    k = np.arange(nvertlayers)[None, :]
    return ok[:, None] & (k >= lo[:, None]) & (k <= hi[:, None])


def pressure_grad(tend, pressure_mid, geopotential_mid, spec_vol, cells_on_edge, dc_edge, edge_mask, lo, hi,
                  n_edges_all):
    """Tend[e][K] = Tend[e][K] - EdgeMask[e] * (GradGeo + AlphaE * GradP) on K in lo[e] .. hi[e], in place:
         InvDc = 1.0 / DcEdge[e]; GradGeo = (Geo[c1][K] - Geo[c0][K]) * InvDc; GradP = (P[c1][K] - P[c0][K]) * InvDc
         AlphaE = 0.5 * (SpecVol[c0][K] + SpecVol[c1][K])"""
    n, K = n_edges_all, tend.shape[1]
    m = range_mask(lo, hi, n, K)
    c0, c1 = np.asarray(cells_on_edge)[:n, 0], np.asarray(cells_on_edge)[:n, 1]
    with np.errstate(all="ignore"):  # entries outside the ranges may hold anything
        inv_dc = (1.0 / np.asarray(dc_edge[:n], dtype=np.float64))[:, None]
        grad_geo = (geopotential_mid[c1] - geopotential_mid[c0]) * inv_dc
        grad_p = (pressure_mid[c1] - pressure_mid[c0]) * inv_dc
        alpha_e = 0.5 * (spec_vol[c0] + spec_vol[c1])
        val = tend[:n] - np.asarray(edge_mask[:n])[:, None] * (grad_geo + alpha_e * grad_p)
    tend[:n][m] = val[m]
    return tend
