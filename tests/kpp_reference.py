"""NumPy restatement of the Kpp numerical contract (omega_amd/csrc/Kpp.h), vectorised over the columns.

Every chain is evaluated in FP64 in the order the contract states; the library is built with -ffp-contract=off, so the
device results equal these bit for bit wherever no cbrt is evaluated (np.cbrt and the device's cbrt are each within a
few ulp of the root, not of each other).  `compute` therefore also reports, per column, `used_cbrt` (some evaluated
velocity scale took a cbrt branch) and `marginal` (a comparison of the contract is within rounding of flipping, or the
interpolation of the boundary-layer depth is ill conditioned), so that a test can say where bits and where a bound are
due.  VtCoef and NonLocalCoeff are inputs: the library forms them once, `constants` restates how.

Arrays are host arrays in the library's local order: level-indexed [rows][K], ZInterface [rows][K + 1], tracers
[NT][NCellsSize][K]; lo / hi are the cell level ranges; n_all / n_owned count the rows computed or updated.
"""
import numpy as np

CS, CM, AS, AM, ZETA_S, ZETA_M = 98.96, 8.38, -28.86, 1.26, -1.0, -0.2  # Large et al. (1994)

DEFAULTS = dict(VonKarman=0.4, CritBulkRichardson=0.3, SurfaceLayerFraction=0.1, Cv=1.7, EntrainmentRatio=0.2, CStar=10.0)


def config(**over):
    c = dict(DEFAULTS)
    for k, v in over.items():
        if k not in c:
            raise KeyError(k)
        c[k] = v
    return c


def constants(cfg):
    """(VtCoef, NonLocalCoeff) in the order the constructor forms them"""
    kappa, ric, eps = (np.float64(cfg[k]) for k in ("VonKarman", "CritBulkRichardson", "SurfaceLayerFraction"))
    cv, er, cstar = (np.float64(cfg[k]) for k in ("Cv", "EntrainmentRatio", "CStar"))
    vt = (cv * np.sqrt(er)) / ((ric * (kappa * kappa)) * np.sqrt(CS * eps))
    nl = (cstar * kappa) * np.cbrt((CS * kappa) * eps)
    return float(vt), float(nl)


def scale(momentum, kappa, us, bf, sig, h):
    """The turbulent velocity scale w(sig, h) -- wM if `momentum`, else wS -- and where it took the cbrt branch;
    the arguments broadcast"""
    us, bf, sig, h = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (us, bf, sig, h)))
    with np.errstate(all="ignore"):
        u3 = (us * us) * us
        z = ((kappa * sig) * h) * bf
        den = u3 + 5.0 * z
        stable = np.where(den > 0.0, ((kappa * us) * u3) / den, 0.0)
        if momentum:
            near = z >= ZETA_M * u3
            a = (kappa * us) * np.sqrt(np.sqrt(1.0 - (16.0 * z) / u3))
            b = kappa * np.cbrt(AM * u3 - CM * z)
        else:
            near = z >= ZETA_S * u3
            a = (kappa * us) * np.sqrt(1.0 - (16.0 * z) / u3)
            b = kappa * np.cbrt(AS * u3 - CS * z)
    is_stable = bf >= 0.0
    return np.where(is_stable, stable, np.where(near, a, b)), ~is_stable & ~near


def scan(t, start, stop):
    """The inclusive Hillis-Steele scan of the contract along axis 1 of t [cols][W], on the entries start <= k <= stop
    of each column (row i = k - start): for s = 1, 2, 4, ... below the column's length, T_i <- T_i + T_(i-s) for
    i >= s, every i from the values before the pass.  Entries outside the range are returned as they came."""
    t = np.array(t, dtype=np.float64, copy=True)
    k = np.arange(t.shape[1])[None, :]
    start, stop = np.asarray(start)[:, None], np.asarray(stop)[:, None]
    longest = int(np.max(stop - start + 1, initial=0))
    s = 1
    while s < longest:
        shifted = np.zeros_like(t)
        shifted[:, s:] = t[:, :-s]
        with np.errstate(all="ignore"):
            t = np.where((k - start >= s) & (k <= stop), t + shifted, t)
        s *= 2
    return t


def compute(un, ut, n2, zmid, zint, vert_diff, vert_visc, us, bf, lo, hi, n_all, n_edges_on_cell, edges_on_cell, dc_edge,
            dv_edge, area_cell, background_visc, background_diff, vt_coef, non_local_coeff, cfg):
    """Kpp::compute: a dict of the six outputs -- BoundaryLayerDepth, BoundaryLayerIndex (int32), BulkRichardson,
    NonLocalShape, VertDiff, VertVisc (copies of the given ones, rewritten inside the boundary layer) -- and of the
    per-column flags `valid`, `used_cbrt` and `marginal`, all over the rows of n2"""
    kappa, ric, eps = (np.float64(cfg[k]) for k in ("VonKarman", "CritBulkRichardson", "SurfaceLayerFraction"))
    n_size, K = n2.shape
    rows = np.arange(n_all)
    lo_, hi_ = np.asarray(lo[:n_all]).astype(np.int64), np.asarray(hi[:n_all]).astype(np.int64)
    ok = (lo_ >= 0) & (lo_ <= hi_) & (hi_ < K)
    lo_s, hi_s = np.where(ok, lo_, 0), np.where(ok, hi_, 0)
    k = np.arange(K)[None, :]
    act = ok[:, None] & (k >= lo_s[:, None]) & (k <= hi_s[:, None])
    i = k - lo_s[:, None]
    us_, bf_ = np.asarray(us[:n_all], dtype=np.float64)[:, None], np.asarray(bf[:n_all], dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        zs = zint[rows, lo_s][:, None]
        zm = zmid[:n_all]
        d = zs - zm
        zm_up = np.full_like(zm, np.nan)
        zm_up[:, 1:] = zm[:, :-1]
        N2 = n2[:n_all]
        t = np.where(act & (i >= 1), N2 * (zm_up - zm), 0.0)
        db = scan(t, lo_s, np.where(ok, hi_s, -1))
        # the shear to the top layer
        dv2 = np.zeros((n_all, K))
        inv_a = 1.0 / np.asarray(area_cell[:n_all], dtype=np.float64)
        ne = np.asarray(n_edges_on_cell[:n_all])
        for j in range(edges_on_cell.shape[1]):
            use = (j < ne)[:, None]
            e = np.where(j < ne, edges_on_cell[:n_all, j], 0)
            f = ((0.5 * dc_edge[e]) * dv_edge[e]) * inv_a
            du = un[e, lo_s][:, None] - un[e]
            dv = ut[e, lo_s][:, None] - ut[e]
            dv2 = np.where(use, dv2 + f[:, None] * ((du * du) + (dv * dv)), dv2)
        n2_dn = np.zeros_like(N2)
        n2_dn[:, :-1] = N2[:, 1:]
        n2_dn = np.where(k < hi_s[:, None], n2_dn, 0.0)
        nmid = 0.5 * (N2 + n2_dn)
        nk = np.sqrt(np.where(nmid > 0.0, nmid, 0.0))
        ws_eps, cb_vt = scale(False, kappa, us_, bf_, eps, d)
        vt2 = ((vt_coef * d) * nk) * ws_eps
        rib = (db * d) / ((dv2 + vt2) + 1.0e-10)
        rib = np.where(act, rib, 0.0)
        # the first crossing and the depth
        cross = act & (i >= 1) & (rib > ric)
        has = cross.any(axis=1)
        kb = np.where(has, np.argmax(cross, axis=1), hi_s + 1)
        kb_s = np.where(has, kb, 1 if K > 1 else 0)
        km = kb_s - 1
        r_m, r_k, d_m, d_k = rib[rows, km], rib[rows, kb_s], d[rows, km], d[rows, kb_s]
        hbl = np.where(has, d_m + ((ric - r_m) / (r_k - r_m)) * (d_k - d_m), zs[:, 0] - zint[rows, hi_s + 1])
        hbl_ = hbl[:, None]
        # the interfaces inside the layer
        face = act & (i >= 1)
        di = zs - zint[:n_all, :K]
        inside = face & (di < hbl_)
        sig = di / hbl_
        sw = np.where((bf_ < 0.0) & (sig > eps), eps, sig)
        g = sig * ((1.0 - sig) * (1.0 - sig))
        wm, cb_m = scale(True, kappa, us_, bf_, sw, hbl_)
        ws, cb_s = scale(False, kappa, us_, bf_, sw, hbl_)
        visc = background_visc + (hbl_ * wm) * g
        diff = background_diff + (hbl_ * ws) * g
        shape = np.where(bf_ < 0.0, non_local_coeff * g, 0.0)
        # what makes a column marginal
        near_ric = (face & (np.abs(rib - ric) <= 1.0e-9 * ric)).any(axis=1)
        near_hbl = (face & (np.abs(di - hbl_) < 1.0e-9 * hbl_)).any(axis=1)
        flat = has & (np.abs(r_k - r_m) < 1.0e-3 * np.maximum(np.maximum(np.abs(r_k), np.abs(r_m)), ric))
    out = dict(BoundaryLayerDepth=np.zeros(n_size), BoundaryLayerIndex=np.full(n_size, -1, np.int32),
               BulkRichardson=np.zeros((n_size, K)), NonLocalShape=np.zeros((n_size, K)),
               VertDiff=np.array(vert_diff, dtype=np.float64, copy=True),
               VertVisc=np.array(vert_visc, dtype=np.float64, copy=True),
               valid=np.zeros(n_size, bool), used_cbrt=np.zeros(n_size, bool), marginal=np.zeros(n_size, bool))
    out["BoundaryLayerDepth"][:n_all] = np.where(ok, hbl, 0.0)
    out["BoundaryLayerIndex"][:n_all] = np.where(ok, kb, -1)
    out["BulkRichardson"][:n_all] = rib
    out["NonLocalShape"][:n_all] = np.where(inside, shape, 0.0)
    out["VertDiff"][:n_all] = np.where(inside, diff, out["VertDiff"][:n_all])
    out["VertVisc"][:n_all] = np.where(inside, visc, out["VertVisc"][:n_all])
    out["valid"][:n_all] = ok
    out["used_cbrt"][:n_all] = (act & cb_vt).any(axis=1) | (inside & (cb_m | cb_s)).any(axis=1)
    out["marginal"][:n_all] = ok & (near_ric | near_hbl | flat)
    out["inside"] = np.zeros((n_size, K), bool)
    out["inside"][:n_all] = inside
    return out


def apply_non_local(h, tracers, ntracers, dt, flux, non_local_shape, lo, hi, n_owned):
    """Kpp::applyNonLocalTracerFlux: a new tracer array; only the owned columns' active levels of tracers
    0 .. ntracers-1 change.  flux None: the tracers as they came."""
    out = np.array(tracers, dtype=np.float64, copy=True)
    if flux is None or ntracers == 0:
        return out
    K = h.shape[1]
    lo_, hi_ = np.asarray(lo[:n_owned]).astype(np.int64), np.asarray(hi[:n_owned]).astype(np.int64)
    ok = (lo_ >= 0) & (lo_ <= hi_) & (hi_ < K)
    k = np.arange(K)[None, :]
    act = ok[:, None] & (k >= lo_[:, None]) & (k <= hi_[:, None])
    nl = non_local_shape[:n_owned]
    below = np.zeros_like(nl)
    below[:, :-1] = nl[:, 1:]
    below = np.where(k < hi_[:, None], below, 0.0)
    with np.errstate(all="ignore"):
        d = nl - below
        for t in range(ntracers):
            phi = out[t, :n_owned]
            val = phi + ((dt * np.asarray(flux[t][:n_owned])[:, None]) * d) / h[:n_owned]
            out[t, :n_owned] = np.where(act, val, phi)
    return out
