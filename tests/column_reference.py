"""NumPy restatement of the VertCoord / Eos numerical contract (omega_amd/csrc/VertCoord.h, Eos.h).

Every output is the FP64 evaluation order the contract states; the library is built with -ffp-contract=off, so the
device results equal these bit for bit.  The sequential column sums are vectorised across cells, one level at a
time: each cell still sees its own additions in the stated order.

Arrays are host arrays in the library's local order: level-indexed [NCellsSize][K] (interface: [NCellsSize][K+1]),
per-cell [NCellsSize]; `n_all` is NCellsAll (the sentinel row NCellsAll is never a column).  The range functions
write into the arrays they are given and leave every entry outside the active ranges as it was.
"""
import numpy as np

GRAVITY = 9.80616  # VertCoord's own g (not the 9.80665 of the tendencies)
RHO0 = 1026.0  # the reference density every test hands to its VertCoord (and to the restatements)


def local_layer_ranges(cell_id, min_level_global, max_level_global, n_all, n_size, nvertlayers):
    """MinLayerCell / MaxLayerCell: the global 1-based minLevelCell / maxLevelCell gathered to local order through
    the 1-based cell ids; absent: 0 and K-1; the sentinel cell -1 / -1."""
    lo = np.full(n_size, -1, dtype=np.int32)
    hi = np.full(n_size, -1, dtype=np.int32)
    if min_level_global is None:
        lo[:n_all], hi[:n_all] = 0, nvertlayers - 1
    else:
        g = np.asarray(cell_id[:n_all]) - 1
        lo[:n_all] = np.asarray(min_level_global)[g] - 1
        hi[:n_all] = np.asarray(max_level_global)[g] - 1
    return lo, hi


def min_max_layer(cells_on, n_all, min_cell, max_cell, nvertlayers):
    """Edge (cells_on = CellsOnEdge) or vertex (CellsOnVertex) layer ranges: (MinTop, MinBot, MaxTop, MaxBot),
    sized n_all + 1 with the sentinel row NVertLayers+1, NVertLayers+1, -1, -1."""
    kp1 = nvertlayers + 1
    c = np.asarray(cells_on)[:n_all]
    mn, mx = np.asarray(min_cell)[c], np.asarray(max_cell)[c]
    land = mx == -1
    top = np.where(land, kp1, mn)
    bot = np.where(land, 0, mn)
    out = [np.empty(n_all + 1, dtype=np.int32) for _ in range(4)]
    out[0][:n_all], out[1][:n_all] = top.min(axis=1), bot.max(axis=1)
    out[2][:n_all], out[3][:n_all] = mx.min(axis=1), mx.max(axis=1)
    out[0][n_all], out[1][n_all], out[2][n_all], out[3][n_all] = kp1, kp1, -1, -1
    return tuple(out)


def _columns(lo, hi, n_all, nvertlayers):
    lo, hi = np.asarray(lo[:n_all]), np.asarray(hi[:n_all])
    ok = (lo >= 0) & (lo <= hi) & (hi < nvertlayers)
    return lo, hi, ok


def pressure(h, ps, lo, hi, n_all, rho0, pint, pmid):
    """computePressure: top-down over KMin..KMax; inc = (g*Rho0)*h; acc += inc; PInt[K+1] = Ps + acc;
    PMid[K] = (Ps + acc) - 0.5*inc; PInt[KMin] = Ps."""
    K = h.shape[1]
    lo, hi, ok = _columns(lo, hi, n_all, K)
    ps = np.zeros(n_all) if ps is None else np.asarray(ps[:n_all], dtype=np.float64)
    grho = GRAVITY * rho0
    rows = np.nonzero(ok)[0]
    pint[rows, lo[rows]] = ps[rows]
    acc = np.zeros(n_all)
    for k in range(K):
        r = rows[(lo[rows] <= k) & (k <= hi[rows])]
        inc = grho * h[r, k]
        acc[r] = acc[r] + inc
        s = ps[r] + acc[r]
        pint[r, k + 1] = s
        pmid[r, k] = s - 0.5 * inc


def zheight(h, specvol, bottom_depth, lo, hi, n_all, rho0, zint, zmid):
    """computeZHeight: bottom-up over KMax..KMin; dz = (Rho0*SpecVol)*h; acc += dz; ZInt[K] = -Bot + acc;
    ZMid[K] = (-Bot + acc) - 0.5*dz; ZInt[KMax+1] = -Bot."""
    K = h.shape[1]
    lo, hi, ok = _columns(lo, hi, n_all, K)
    nb = -np.asarray(bottom_depth[:n_all], dtype=np.float64)
    rows = np.nonzero(ok)[0]
    zint[rows, hi[rows] + 1] = nb[rows]
    acc = np.zeros(n_all)
    for k in range(K - 1, -1, -1):
        r = rows[(lo[rows] <= k) & (k <= hi[rows])]
        dz = (rho0 * specvol[r, k]) * h[r, k]
        acc[r] = acc[r] + dz
        s = nb[r] + acc[r]
        zint[r, k] = s
        zmid[r, k] = s - 0.5 * dz


def _active_mask(lo, hi, n_all, nvertlayers, width):
    lo, hi, ok = _columns(lo, hi, n_all, nvertlayers)
    k = np.arange(width)[None, :]
    return ok[:, None] & (k >= lo[:, None]) & (k <= hi[:, None])


def geopotential(zmid, tidal, sal, lo, hi, n_all, geo):
    """computeGeopotential: GeoMid = ((g*ZMid) + Tidal) + SAL on the active layers."""
    K = zmid.shape[1]
    m = _active_mask(lo, hi, n_all, K, K)
    t = np.zeros(n_all) if tidal is None else np.asarray(tidal[:n_all], dtype=np.float64)
    s = np.zeros(n_all) if sal is None else np.asarray(sal[:n_all], dtype=np.float64)
    val = ((GRAVITY * zmid[:n_all]) + t[:, None]) + s[:, None]
    geo[:n_all][m] = val[m]


def target_thickness(pint, ref, weights, lo, hi, n_all, rho0, target):
    """computeTargetThickness: ascending sums of W*Ref (SumWh) and Ref (SumRef) over KMin..KMax;
    Coeff = (PInt[KMax+1] - PInt[KMin])/(g*Rho0) - SumRef; Target = Ref*(1 + (Coeff*W)/SumWh)."""
    K = ref.shape[1]
    lo, hi, ok = _columns(lo, hi, n_all, K)
    rows = np.nonzero(ok)[0]
    sum_wh, sum_ref = np.zeros(n_all), np.zeros(n_all)
    for k in range(K):
        r = rows[(lo[rows] <= k) & (k <= hi[rows])]
        sum_wh[r] = sum_wh[r] + weights[k] * ref[r, k]
        sum_ref[r] = sum_ref[r] + ref[r, k]
    coeff = np.zeros(n_all)
    coeff[rows] = (pint[rows, hi[rows] + 1] - pint[rows, lo[rows]]) / (GRAVITY * rho0) - sum_ref[rows]
    m = _active_mask(lo, hi, n_all, K, K)
    with np.errstate(divide="ignore", invalid="ignore"):
        val = ref[:n_all] * (1.0 + (coeff[:, None] * np.asarray(weights)[None, :]) / sum_wh[:, None])
    target[:n_all][m] = val[m]


def movement_weights(kind, nvertlayers):
    if kind == "Uniform":
        return np.ones(nvertlayers)
    if kind == "Fixed":
        w = np.zeros(nvertlayers)
        w[0] = 1.0
        return w
    raise ValueError(kind)


# ---- equation of state
def spec_vol_linear(ct, sa, drhodt=-0.2, drhods=0.8, rhot0s0=1000.0):
    return 1.0 / (rhot0s0 + (drhodt * ct + drhods * sa))


# TEOS-10 75-term specific volume, Roquet, Madec, McDougall and Barker (2015), Ocean Modelling 90, 29-43, A.2.
# V[i, j, k]: power i of ss, j of tt, k of pp.
_V = {
    (0, 0, 0): 1.0769995862e-03, (1, 0, 0): -3.1038981976e-04, (2, 0, 0): 6.6928067038e-04,
    (3, 0, 0): -8.5047933937e-04, (4, 0, 0): 5.8086069943e-04, (5, 0, 0): -2.1092370507e-04,
    (6, 0, 0): 3.1932457305e-05, (0, 1, 0): -1.5649734675e-05, (1, 1, 0): 3.5009599764e-05,
    (2, 1, 0): -4.3592678561e-05, (3, 1, 0): 3.4532461828e-05, (4, 1, 0): -1.1959409788e-05,
    (5, 1, 0): 1.3864594581e-06, (0, 2, 0): 2.7762106484e-05, (1, 2, 0): -3.7435842344e-05,
    (2, 2, 0): 3.5907822760e-05, (3, 2, 0): -1.8698584187e-05, (4, 2, 0): 3.8595339244e-06,
    (0, 3, 0): -1.6521159259e-05, (1, 3, 0): 2.4141479483e-05, (2, 3, 0): -1.4353633048e-05,
    (3, 3, 0): 2.2863324556e-06, (0, 4, 0): 6.9111322702e-06, (1, 4, 0): -8.7595873154e-06,
    (2, 4, 0): 4.3703680598e-06, (0, 5, 0): -8.0539615540e-07, (1, 5, 0): -3.3052758900e-07,
    (0, 6, 0): 2.0543094268e-07,
    (0, 0, 1): -1.6784136540e-05, (1, 0, 1): 2.4262468747e-05, (2, 0, 1): -3.4792460974e-05,
    (3, 0, 1): 3.7470777305e-05, (4, 0, 1): -1.7322218612e-05, (5, 0, 1): 3.0927427253e-06,
    (0, 1, 1): 1.8505765429e-05, (1, 1, 1): -9.5677088156e-06, (2, 1, 1): 1.1100834765e-05,
    (3, 1, 1): -9.8447117844e-06, (4, 1, 1): 2.5909225260e-06, (0, 2, 1): -1.1716606853e-05,
    (1, 2, 1): -2.3678308361e-07, (2, 2, 1): 2.9283346295e-06, (3, 2, 1): -4.8826139200e-07,
    (0, 3, 1): 7.9279656173e-06, (1, 3, 1): -3.4558773655e-06, (2, 3, 1): 3.1655306078e-07,
    (0, 4, 1): -3.4102187482e-06, (1, 4, 1): 1.2956717783e-06, (0, 5, 1): 5.0736766814e-07,
    (0, 0, 2): 3.0623833435e-06, (1, 0, 2): -5.8484432984e-07, (2, 0, 2): -4.8122251597e-06,
    (3, 0, 2): 4.9263106998e-06, (4, 0, 2): -1.7811974727e-06, (0, 1, 2): -1.1736386731e-06,
    (1, 1, 2): -5.5699154557e-06, (2, 1, 2): 5.4620748834e-06, (3, 1, 2): -1.3544185627e-06,
    (0, 2, 2): 2.1305028740e-06, (1, 2, 2): 3.9137387080e-07, (2, 2, 2): -6.5731104067e-07,
    (0, 3, 2): -4.6132540037e-07, (1, 3, 2): 7.7618888092e-09, (0, 4, 2): -6.3352916514e-08,
    (0, 0, 3): -3.8088938393e-07, (1, 0, 3): 3.6310188515e-07, (2, 0, 3): 1.6746303780e-08,
    (0, 1, 3): -3.6527006553e-07, (1, 1, 3): -2.7295696237e-07, (0, 2, 3): 2.8695905159e-07,
    (0, 0, 4): 8.8302421514e-08, (1, 0, 4): -1.1147125423e-07, (0, 1, 4): 3.1454099902e-07,
    (0, 0, 5): 4.2369007180e-09,
}
_V0 = (-4.4015007269e-05, 6.9232335784e-06, -7.5004675975e-07, 1.7009109288e-08, -1.6884162004e-08,
       1.9613503930e-09)  # reference profile v0(pp) = (((((v05*pp + v04)*pp + ...)*pp + v00)*pp


# named as in the paper: V{i}{j}{k}
globals().update({f"V{i}{j}{k}": v for (i, j, k), v in _V.items()})


def teos10_pcoeffs(ct, sa):
    """The six pressure coefficients c0..c5 of delta(ss, tt, pp), each polynomial in nested form as the contract
    writes it (a*b + c*d + e groups as ((a*b) + (c*d)) + e, in Python as in C++)."""
    sau, ctu, delta_s = 40.0 * 35.16504 / 35.0, 40.0, 24.0
    ss = np.sqrt((sa + delta_s) / sau)
    tt = ct / ctu
    c5 = V005 + 0.0 * tt
    c4 = V014 * tt + V104 * ss + V004
    c3 = (V023 * tt + V113 * ss + V013) * tt + (V203 * ss + V103) * ss + V003
    c2 = ((((V042 * tt + V132 * ss + V032) * tt + (V222 * ss + V122) * ss + V022) * tt
           + ((V312 * ss + V212) * ss + V112) * ss + V012) * tt
          + (((V402 * ss + V302) * ss + V202) * ss + V102) * ss + V002)
    c1 = (((((V051 * tt + V141 * ss + V041) * tt + (V231 * ss + V131) * ss + V031) * tt
            + ((V321 * ss + V221) * ss + V121) * ss + V021) * tt
           + (((V411 * ss + V311) * ss + V211) * ss + V111) * ss + V011) * tt
          + ((((V501 * ss + V401) * ss + V301) * ss + V201) * ss + V101) * ss + V001)
    c0 = ((((((V060 * tt + V150 * ss + V050) * tt + (V240 * ss + V140) * ss + V040) * tt
             + ((V330 * ss + V230) * ss + V130) * ss + V030) * tt
            + (((V420 * ss + V320) * ss + V220) * ss + V120) * ss + V020) * tt
           + ((((V510 * ss + V410) * ss + V310) * ss + V210) * ss + V110) * ss + V010) * tt
          + (((((V600 * ss + V500) * ss + V400) * ss + V300) * ss + V200) * ss + V100) * ss + V000)
    return [c0, c1, c2, c3, c4, c5]


def spec_vol_teos10_from_coeffs(c, p):
    pp = p / 1.0e4
    v00, v01, v02, v03, v04, v05 = _V0
    v0 = (((((v05 * pp + v04) * pp + v03) * pp + v02) * pp + v01) * pp + v00) * pp
    delta = ((((c[5] * pp + c[4]) * pp + c[3]) * pp + c[2]) * pp + c[1]) * pp + c[0]
    return v0 + delta


def spec_vol_teos10(ct, sa, p):
    return spec_vol_teos10_from_coeffs(teos10_pcoeffs(ct, sa), p)


def eos_spec_vol(kind, ct, sa, p, n_all, kdisp=None, linear=(-0.2, 0.8, 1000.0)):
    """SpecVol (kdisp None) or SpecVolDisplaced of [NCellsSize][K] inputs (p in dbar): rows 0..n_all-1 on every
    level, the sentinel row n_all (and any row beyond) 0."""
    out = np.zeros_like(np.asarray(ct, dtype=np.float64))
    K = out.shape[1]
    t, s, pr = ct[:n_all], sa[:n_all], p[:n_all]
    if kind == "linear":
        out[:n_all] = spec_vol_linear(t, s, *linear)
        return out
    if kdisp is not None:
        kk = np.clip(np.arange(K) + kdisp, 0, K - 1)
        pr = pr[:, kk]
    out[:n_all] = spec_vol_teos10(t, s, pr)
    return out


def column_sequence(h, ct, sa, ps, tidal, sal, bottom_depth, lo, hi, n_all, rho0, eos_kind, state, kdisp=None,
                    linear=(-0.2, 0.8, 1000.0)):
    """computePressure -> computeSpecVol(T, S, PMid*1e-4) -> computeZHeight -> computeGeopotential on the arrays of
    `state` (dict: PressureInterface, PressureMid, SpecVol, [SpecVolDisplaced], ZInterface, ZMid, GeopotentialMid),
    updated in place: what the fused pass writes."""
    pressure(h, ps, lo, hi, n_all, rho0, state["PressureInterface"], state["PressureMid"])
    pdbar = state["PressureMid"] * 1.0e-4
    state["SpecVol"][:] = eos_spec_vol(eos_kind, ct, sa, pdbar, n_all, None, linear)
    if kdisp is not None:
        state["SpecVolDisplaced"][:] = eos_spec_vol(eos_kind, ct, sa, pdbar, n_all, kdisp, linear)
    zheight(h, state["SpecVol"], bottom_depth, lo, hi, n_all, rho0, state["ZInterface"], state["ZMid"])
    geopotential(state["ZMid"], tidal, sal, lo, hi, n_all, state["GeopotentialMid"])
