"""NumPy restatement of the three BarotropicMode calls of a split-explicit step and of the step's glue
(omega_amd/csrc/BarotropicMode.h, SplitExplicitStepper.h), in the written order: the device results equal these bit for
bit.  The sums and the sub-step are those of tests/barotropic_reference.py.

Arrays as there: host arrays in the library's local order, edge arrays [NEdgesSize] or [NEdgesSize][K]; the functions
write into the arrays they are given and leave every entry the contract does not name as it was.
"""
import numpy as np

from tests import barotropic_reference as BR


def residual(M, ssh, vel, gravity):
    """R[e] = EdgeMask[e]*(Cor - Gravity*((SSH[c1] - SSH[c0])*InvDcEdge[e])) on the open edges, 0.0 on the others
    (which read no cell and no neighbour)"""
    r = np.zeros(M.ne)
    e = np.nonzero(M.open)[0]
    c0, c1 = M.coe[e, 0], M.coe[e, 1]
    cor = M.coriolis(vel)
    r[e] = M.mask[e] * (cor[e] - gravity * ((ssh[c1] - ssh[c0]) * M.inv_dc[e]))
    return r


def compute_residual_forcing(M, h, vel_tend, lo_e, hi_e, ssh, vel, gravity, tend_mean, forcing):
    """BtrTendMean = G (computeForcing's mean); BtrForcing = G - R on the open edges, G on the others"""
    n = M.ne
    g = BR._edge_means(h, vel_tend, M.coe, lo_e, hi_e, n)[1]
    tend_mean[:n] = g
    out = g.copy()
    e = np.nonzero(M.open)[0]
    out[e] = g[e] - residual(M, ssh, vel, gravity)[e]
    forcing[:n] = out
    return tend_mean, forcing


def transport_velocity(u_old, u_out, bcl_vel, flux_mean, thick, lo_e, hi_e, n_edges_all):
    """u_out = BclVelocity + BtrFluxMean/BtrThickEdge on Lo .. Hi (one quotient per edge), u_old on the other levels"""
    n, K = n_edges_all, u_old.shape[1]
    m = BR.range_mask(lo_e, hi_e, n, K)
    with np.errstate(all="ignore"):
        q = np.asarray(flux_mean)[:n] / np.asarray(thick)[:n]
        val = bcl_vel[:n] + q[:, None]
    u_out[:n] = np.where(m, val, u_old[:n])
    return u_out


def advance_velocity(u_old, vel_tend, dt, u_out, bcl_vel, btr_vel, tend_mean, lo_e, hi_e, n_edges_all):
    """u_out = (BclVelocity + dt*(VelTend - BtrTendMean)) + BtrVelocity on Lo .. Hi, u_old + dt*VelTend on the other
    levels; u_out may be u_old"""
    n, K = n_edges_all, u_old.shape[1]
    m = BR.range_mask(lo_e, hi_e, n, K)
    with np.errstate(all="ignore"):
        inside = (bcl_vel[:n] + dt * (vel_tend[:n] - np.asarray(tend_mean)[:n, None])) + np.asarray(btr_vel)[:n, None]
        outside = u_old[:n] + dt * vel_tend[:n]
    u_out[:n] = np.where(m, inside, outside)
    return u_out


class Split:
    """The 2-D fields of one BarotropicMode, zero at construction"""

    def __init__(self, M, n_cells_size, n_edges_size, K):
        self.M, self.K = M, K
        self.ssh = np.zeros(n_cells_size)
        self.vel, self.thick, self.forcing, self.flux, self.tend_mean = (np.zeros(n_edges_size) for _ in range(5))
        self.bcl = np.zeros((n_edges_size, K))


def step(x, h, u, vel_tend, dt, nsub, lo_c, hi_c, lo_e, hi_e, gravity, thickness_and_tracers):
    """The glue of one split-explicit step (steps 2-5 and 8 of SplitExplicitStepper.h) on the Split `x`.  `vel_tend` is
    step 1's NormalVelocityTend; `thickness_and_tracers(u_transport)` is the caller's steps 6 and 7 (it computes no
    right-hand side here) and returns whatever the caller wants back.  Returns (u_new, that)."""
    M = x.M
    BR.split_velocity(h, u, M.coe, lo_e, hi_e, M.ne, x.thick, x.vel, x.bcl)
    BR.compute_ssh(h, M.bottom, lo_c, hi_c, M.nc, x.ssh)
    compute_residual_forcing(M, h, vel_tend, lo_e, hi_e, x.ssh, x.vel, gravity, x.tend_mean, x.forcing)
    BR.subcycle(M, x.ssh, x.vel, x.forcing, x.flux, nsub, dt / float(nsub), gravity)
    u_tr = transport_velocity(u, np.zeros_like(u), x.bcl, x.flux, x.thick, lo_e, hi_e, M.ne)
    other = thickness_and_tracers(u_tr)
    u_new = advance_velocity(u, vel_tend, dt, np.zeros_like(u), x.bcl, x.vel, x.tend_mean, lo_e, hi_e, M.ne)
    return u_new, other
