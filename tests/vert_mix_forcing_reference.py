"""NumPy restatement of the forced implicit solves of VertMix (omega_amd/csrc/VertMix.h: wind stress, bottom drag,
Rayleigh drag, surface tracer fluxes), built on tests/vert_mix_reference.py and tests/tridiag_reference.py: the same
FP64 evaluation order, so the device results equal these bit for bit.

Arrays are host arrays in the library's local order, as in tests/vert_mix_reference.py; surface_flux is
[NT][NCellsSize], stress and edge_mask [NEdgesSize], ut [NEdgesSize][K].  A term whose coefficient is zero, or whose
array is None, is skipped: with all of them skipped the functions return tracer_mix / velocity_mix bit for bit."""
import numpy as np

from tests import vert_mix_reference as MR
from tests.tridiag_reference import pcr_diff


def velocity_system(he, nue, ucol, utbot, dt, cd, ra, stress, mask, rho0):
    """(G, D, X) of edge columns [nedges][n]: he, nue, ucol at the column's levels, utbot [nedges] the tangential
    velocity at the bottom level (None without drag), stress / mask [nedges] (stress None: no term).
      D_i = hE;  Rayleigh: D_i = D_i + (dt*Ra)*hE;  bottom row: D = D + (dt*Cd)*sqrt((u*u) + (ut*ut))
      X_i = hE*u;  top row with a stress array: X_0 = X_0 + (dt*mask)*(stress/rho0)"""
    g, d, x = MR.assemble(he, nue, ucol, dt)
    if ra != 0.0:
        d = d + (dt * ra) * he
    if cd != 0.0:
        ub = ucol[:, -1]
        speed = np.sqrt((ub * ub) + (utbot * utbot))
        d[:, -1] = d[:, -1] + (dt * cd) * speed
    if stress is not None:
        x[:, 0] = x[:, 0] + (dt * mask) * (stress / rho0)
    return g, d, x


def velocity_mix_forced(h, vert_visc, u, dt, cells_on_edge, lo_edge_bot, hi_edge_top, n_owned, cd=0.0, ra=0.0,
                        stress=None, ut=None, edge_mask=None, rho0=1026.0):
    """The forced applyVelocityVertMix: a new normal-velocity array"""
    assert cd >= 0.0 and ra >= 0.0
    assert cd == 0.0 or ut is not None
    assert stress is None or edge_mask is not None
    out = np.array(u, dtype=np.float64, copy=True)
    for es, k, he, nue, ucol in MR.edge_columns(h, vert_visc, out, cells_on_edge, lo_edge_bot, hi_edge_top, n_owned):
        utbot = ut[es, k[:, -1]] if cd != 0.0 else None
        g, d, x = velocity_system(he, nue, ucol, utbot, dt, cd, ra, None if stress is None else stress[es],
                                  None if stress is None else edge_mask[es], rho0)
        out[es[:, None], k] = pcr_diff(g, d, x)
    return out


def tracer_columns(h, vert_diff, lo, hi, n_owned):
    """per column length: (cells, levels, h, VertDiff) of the owned cells with a valid range"""
    K = h.shape[1]
    lo, hi = np.asarray(lo[:n_owned]), np.asarray(hi[:n_owned])
    ok = (lo >= 0) & (lo <= hi) & (hi < K)
    n = np.where(ok, hi - lo + 1, 0)
    for length in np.unique(n[n > 0]):
        cols = np.nonzero(n == length)[0]
        k = lo[cols][:, None] + np.arange(length)[None, :]
        yield cols, k, h[cols[:, None], k], vert_diff[cols[:, None], k]


def tracer_system(hcol, dcol, phi, flux, dt):
    """(G, H, X) of cell columns: X_0 = (h*phi) + dt*flux (flux [ncols] or None)"""
    g, hh, x = MR.assemble(hcol, dcol, phi, dt)
    if flux is not None:
        x[:, 0] = x[:, 0] + dt * flux
    return g, hh, x


def tracer_mix_forced(h, vert_diff, tracers, ntracers, dt, lo, hi, n_owned, surface_flux=None):
    """The forced applyTracerVertMix: a new tracer array"""
    out = np.array(tracers, dtype=np.float64, copy=True)
    for cols, k, hcol, dcol in tracer_columns(h, vert_diff, lo, hi, n_owned):
        c = cols[:, None]
        for t in range(ntracers):
            g, hh, x = tracer_system(hcol, dcol, out[t][c, k], None if surface_flux is None else surface_flux[t][cols],
                                     dt)
            out[t][c, k] = pcr_diff(g, hh, x)
    return out
