"""NumPy restatement of the 3-D form of the MonotoneAdv numerical contract (omega_amd/csrc/MonotoneAdv.h, "The 3-D
form"): the horizontal edge terms are those of tests/monotone_adv_reference.py, reused as they are; this file adds the
interface quantities and the vertical part of the two passes, every chain in the order the header writes it.

Arrays as there: cell arrays [NCellsSize][K], tracer arrays [NTracers][NCellsSize][K]; `wt` is VerticalTransport
[NCellsSize][K], `lo` / `hi` MinLayerCell / MaxLayerCell [NCellsSize].  Interface K is the top of layer K; values at an
interface outside lo < K <= hi are selected to 0.0 and whatever the arithmetic made of the (possibly NaN) operands there
is dropped.
"""
import numpy as np

from tests import monotone_adv_reference as MR
from tests.monotone_adv_reference import kmax, kmin


def interface_mask(lo, hi, nc, K):
    """[nc][K] True where interface K carries flux: lo < K <= hi (a land column, hi < lo: nowhere)"""
    k = np.arange(K)[None, :]
    return (lo[:nc, None] < k) & (k <= hi[:nc, None])


def _up(x):
    """x[K-1] at K (column 0: NaN, never selected)"""
    out = np.full_like(x, np.nan)
    out[:, 1:] = x[:, :-1]
    return out


def _down(x, fill=np.nan):
    """x[K+1] at K (the last column: fill)"""
    out = np.full_like(x, fill)
    out[:, :-1] = x[:, 1:]
    return out


def interface_terms(h_old, phi, wt, lo, hi, nc):
    """(inside, Wv, VLow, PhiT, AV) at the top interface of every level, [nc][K]"""
    K = h_old.shape[1]
    inside = interface_mask(lo, hi, nc, K)
    h, p = h_old[:nc], phi[:nc]
    with np.errstate(all="ignore"):
        wv = np.where(inside, wt[:nc], 0.0)
        pu, hu = _up(p), _up(h)
        v_low = np.where(wv > 0.0, wv * p, wv * pu)
        phi_t = pu + (hu / (hu + h)) * (p - pu)
        v_high = wv * phi_t
        av = v_high - v_low
    return inside, wv, np.where(inside, v_low, 0.0), phi_t, np.where(inside, av, 0.0)


def scale_factors(M, h_old, h_new, u, phi, dt, wt, lo, hi, upwind=False):
    """pass 1 for one tracer: (ScaleIn, ScaleOut, PMin, PMax), [NCellsAll][K]"""
    nc, K = M.nc, h_old.shape[1]
    p_c = phi[:nc]
    p_max, p_min = p_c.copy(), p_c.copy()
    div_low, s_in, s_out = np.zeros((nc, K)), np.zeros((nc, K)), np.zeros((nc, K))
    with np.errstate(all="ignore"):
        for r, e, c0, c1, s in M.slots():
            n = np.where(s < 0, c1, c0)
            _, f_low, _, a = MR.edge_terms(M, e, c0, c1, h_old, u, phi, upwind)
            p_max[r] = kmax(p_max[r], phi[n])
            p_min[r] = kmin(p_min[r], phi[n])
            sa = MR._signed(s, a)
            div_low[r] = div_low[r] + MR._signed(s, f_low)
            s_in[r] = s_in[r] + kmax(sa, 0.0)
            s_out[r] = s_out[r] + kmax(-sa, 0.0)
        top, _, v_low, _, av = interface_terms(h_old, phi, wt, lo, hi, nc)
        bot = _down(top, False)
        v_low_b, av_b = _down(v_low, 0.0), _down(av, 0.0)
        p_max = np.where(top, kmax(p_max, _up(p_c)), p_max)
        p_min = np.where(top, kmin(p_min, _up(p_c)), p_min)
        p_max = np.where(bot, kmax(p_max, _down(p_c)), p_max)
        p_min = np.where(bot, kmin(p_min, _down(p_c)), p_min)
        inv_a = M.inv_area[:, None]
        h_td = h_old[:nc] * p_c + dt * (((div_low * inv_a) - v_low) + v_low_b)
        p_in = dt * (((s_in * inv_a) + kmax(-av, 0.0)) + kmax(av_b, 0.0))
        p_out = dt * (((s_out * inv_a) + kmax(av, 0.0)) + kmax(-av_b, 0.0))
        q_in = kmax(0.0, p_max * h_new[:nc] - h_td)
        q_out = kmax(0.0, h_td - p_min * h_new[:nc])
        scale_in = np.where(p_in > 0.0, kmin(1.0, q_in / p_in), 1.0)
        scale_out = np.where(p_out > 0.0, kmin(1.0, q_out / p_out), 1.0)
    return scale_in, scale_out, p_min, p_max


def interface_scale(av, inside, scale_in, scale_out):
    """ScV at the top interface of every level (NaN where the interface carries no flux)"""
    with np.errstate(all="ignore"):
        sc = np.where(av >= 0.0, kmin(scale_out, _up(scale_in)), kmin(scale_in, _up(scale_out)))
    return np.where(inside, sc, np.nan)


def vertical_flux(h_old, phi, wt, lo, hi, nc, scale_in, scale_out, flux="limited"):
    """FV at the top interface of every level, [nc][K], 0.0 where it carries no flux.  flux: "limited" (the contract),
    "low" VLow, "high" VLow + AV"""
    inside, _, v_low, _, av = interface_terms(h_old, phi, wt, lo, hi, nc)
    with np.errstate(all="ignore"):
        if flux == "limited":
            f = v_low + interface_scale(av, inside, scale_in[:nc], scale_out[:nc]) * av
        else:
            f = v_low if flux == "low" else v_low + av
    return np.where(inside, f, 0.0)


def flux_divergence(M, h_old, u, phi, scale_in, scale_out, wt, lo, hi, upwind=False, flux="limited"):
    """pass 2 for one tracer: (((sum of s*F)*InvA) - FV[K]) + FV[K+1], [NCellsAll][K]"""
    nc, K = M.nc, h_old.shape[1]
    total = np.zeros((nc, K))
    with np.errstate(all="ignore"):
        for r, e, c0, c1, s in M.slots():
            _, f_low, f_high, a = MR.edge_terms(M, e, c0, c1, h_old, u, phi, upwind)
            if flux == "limited":
                f = f_low + MR.edge_scale(a, scale_in, scale_out, c0, c1) * a
            else:
                f = f_low if flux == "low" else f_high
            total[r] = total[r] + MR._signed(s, f)
        fv = vertical_flux(h_old, phi, wt, lo, hi, nc, scale_in, scale_out, flux)
        return ((total * M.inv_area[:, None]) - fv) + _down(fv, 0.0)


def add_tracer_tend(M, tend, h_old, h_new, u, tracers, ntracers, dt, upwind, scale_in, scale_out, wt, lo, hi):
    """MonotoneAdv::addTracerTend with a VertAdv attached, in place on tend, scale_in, scale_out: only the entries
    [L < ntracers][c < NCellsAll] are written"""
    nc = M.nc
    for L in range(ntracers):
        si, so, _, _ = scale_factors(M, h_old, h_new, u, tracers[L], dt, wt, lo, hi, upwind)
        scale_in[L, :nc], scale_out[L, :nc] = si, so
        with np.errstate(all="ignore"):
            tend[L, :nc] = tend[L, :nc] + flux_divergence(M, h_old, u, tracers[L], si, so, wt, lo, hi, upwind)
    return tend


def thickness_divergence(wt, lo, hi, nc):
    """(-Wv[K] + Wv[K+1], max(Wv[K], 0) + max(-Wv[K+1], 0)): the vertical part of the thickness tendency and of the
    outflow, [nc][K]"""
    K = wt.shape[1]
    wv = np.where(interface_mask(lo, hi, nc, K), wt[:nc], 0.0)
    wb = _down(wv, 0.0)
    return -wv + wb, kmax(wv, 0.0) + kmax(-wb, 0.0)


def interface_limits(h_old, phi, wt, lo, hi, nc, scale_in, scale_out):
    """ScV on the interfaces that carry flux (Wv != 0), 1-D"""
    inside, wv, _, _, av = interface_terms(h_old, phi, wt, lo, hi, nc)
    sc = interface_scale(av, inside, scale_in[:nc], scale_out[:nc])
    return sc[inside & (wv != 0.0)]
