"""NumPy restatement of the VertMix numerical contract (omega_amd/csrc/VertMix.h).

Every output is the FP64 evaluation order the contract states; the library is built with -ffp-contract=off, so the
device results equal these bit for bit (a non-integer ShearExponent excepted: the device pow is a few ulp from
NumPy's).  The column solves use tests/tridiag_reference.py: pcr_diff, the restated PCRDiffusionSolver.

Arrays are host arrays in the library's local order: level-indexed [rows][K], tracers [NT][NCellsSize][K]; lo / hi
are the cell (or edge) level ranges; n_all / n_owned count the rows computed or solved.
"""
import numpy as np

from tests.tridiag_reference import pcr_diff

GRAVITY = 9.80616  # VertCoord's own g

DEFAULTS = dict(BackgroundViscosity=1.0e-4, BackgroundDiffusivity=1.0e-5, EnableShearMix=True, ShearNuZero=0.005,
                ShearAlpha=5.0, ShearExponent=2.0, EnableConvectiveMix=True, ConvectiveDiffusivity=1.0,
                ConvectiveTriggerBVF=0.0)


def config(**over):
    c = dict(DEFAULTS)
    for k, v in over.items():
        if k not in c:
            raise KeyError(k)
        c[k] = v
    return c


def _interfaces(lo, hi, n_all, K):
    """[n_all][K] mask of the interfaces KMin < K <= KMax of valid columns"""
    lo, hi = np.asarray(lo[:n_all]), np.asarray(hi[:n_all])
    ok = (lo >= 0) & (lo <= hi) & (hi < K)
    k = np.arange(K)[None, :]
    return ok[:, None] & (k > lo[:, None]) & (k <= hi[:, None])


def bvf(spec_vol, spec_vol_disp, zmid, lo, hi, n_all, rho0):
    """computeBruntVaisalaFreqSq: N2[K] = ((g / Rho0) * ((1.0 / SpecVol[K]) - (1.0 / SpecVolDisplaced[K-1]))) /
    (ZMid[K-1] - ZMid[K]) on KMin < K <= KMax; 0 on every other entry of every row."""
    n_size, K = spec_vol.shape
    out = np.zeros((n_size, K))
    m = _interfaces(lo, hi, n_all, K)
    with np.errstate(all="ignore"):
        v = ((GRAVITY / rho0) * ((1.0 / spec_vol[:n_all, 1:]) - (1.0 / spec_vol_disp[:n_all, :-1]))) / \
            (zmid[:n_all, :-1] - zmid[:n_all, 1:])
    out[:n_all, 1:] = np.where(m[:, 1:], v, 0.0)
    return out


def shear_pow(d, n):
    """D^n: D*D*...*D left to right for an integer n in 1 .. 8, else pow(D, n)"""
    if 1.0 <= n <= 8.0 and float(int(n)) == n:
        p = d.copy()
        for _ in range(int(n) - 1):
            p = p * d
        return p
    return np.power(d, n)


def coefficients(un, ut, n2, zmid, lo, hi, n_all, n_edges_on_cell, edges_on_cell, dc_edge, dv_edge, area_cell, cfg):
    """computeVertMix: (VertVisc, VertDiff) [n_size][K], in the contract's order"""
    n_size, K = n2.shape
    visc, diff = np.zeros((n_size, K)), np.zeros((n_size, K))
    m = _interfaces(lo, hi, n_all, K)[:, 1:]
    with np.errstate(all="ignore"):
        N2 = n2[:n_all, 1:]
        v = np.full((n_all, K - 1), cfg["BackgroundViscosity"])
        d = np.full((n_all, K - 1), cfg["BackgroundDiffusivity"])
        if cfg["EnableShearMix"]:
            s2 = np.zeros((n_all, K - 1))
            inv_a = 1.0 / np.asarray(area_cell[:n_all], dtype=np.float64)
            ne = np.asarray(n_edges_on_cell[:n_all])
            for j in range(edges_on_cell.shape[1]):
                use = (j < ne)[:, None]
                e = np.where(j < ne, edges_on_cell[:n_all, j], 0)
                f = ((0.5 * dc_edge[e]) * dv_edge[e]) * inv_a
                du = un[e, :-1] - un[e, 1:]
                dv = ut[e, :-1] - ut[e, 1:]
                s2 = np.where(use, s2 + f[:, None] * ((du * du) + (dv * dv)), s2)
            dz = zmid[:n_all, :-1] - zmid[:n_all, 1:]
            s2 = s2 / (dz * dz)
            s2c = np.where(s2 < 1.0e-12, 1.0e-12, s2)
            ri = N2 / s2c
            ri = np.where(ri < 0.0, 0.0, ri)
            D = 1.0 + cfg["ShearAlpha"] * ri
            v = v + cfg["ShearNuZero"] / shear_pow(D, cfg["ShearExponent"])
            d = d + v / D
        if cfg["EnableConvectiveMix"]:
            conv = N2 < cfg["ConvectiveTriggerBVF"]
            v = np.where(conv, v + cfg["ConvectiveDiffusivity"], v)
            d = np.where(conv, d + cfg["ConvectiveDiffusivity"], d)
    visc[:n_all, 1:] = np.where(m, v, 0.0)
    diff[:n_all, 1:] = np.where(m, d, 0.0)
    return visc, diff


def _ranges(lo, hi, rows, K):
    lo, hi = np.asarray(lo[:rows]), np.asarray(hi[:rows])
    ok = (lo >= 0) & (lo <= hi) & (hi < K)
    return lo, hi, ok


def assemble(hcol, coef, phi, dt):
    """(G, H, X) of columns [ncols][n] from thickness, coefficient and field values at the column's levels:
    H = h; G_i = (coef[i+1] * dt) / ((h[i+1] + h[i]) / 2), G_{n-1} = 0; X = h * phi"""
    g = np.zeros_like(hcol)
    g[:, :-1] = (coef[:, 1:] * dt) / ((hcol[:, 1:] + hcol[:, :-1]) / 2)
    return g, hcol.copy(), hcol * phi


def tracer_mix(h, vert_diff, tracers, ntracers, dt, lo, hi, n_owned):
    """applyTracerVertMix: a new tracer array; only the owned columns' active levels of tracers 0..ntracers-1 change"""
    out = np.array(tracers, dtype=np.float64, copy=True)
    K = h.shape[1]
    lo, hi, ok = _ranges(lo, hi, n_owned, K)
    n = np.where(ok, hi - lo + 1, 0)
    for length in np.unique(n[n > 0]):
        cols = np.nonzero(n == length)[0]
        k = lo[cols][:, None] + np.arange(length)[None, :]
        c = cols[:, None]
        hcol, dcol = h[c, k], vert_diff[c, k]
        for t in range(ntracers):
            g, hh, x = assemble(hcol, dcol, out[t][c, k], dt)
            out[t][c, k] = pcr_diff(g, hh, x)
    return out


def edge_columns(h, visc, u, cells_on_edge, lo, hi, n_owned):
    """per edge length: (edges, levels, hE, nuE, u) for the owned edges with a non-empty range"""
    K = h.shape[1]
    lo, hi, ok = _ranges(lo, hi, n_owned, K)
    n = np.where(ok, hi - lo + 1, 0)
    for length in np.unique(n[n > 0]):
        es = np.nonzero(n == length)[0]
        k = lo[es][:, None] + np.arange(length)[None, :]
        c1, c2 = cells_on_edge[es, 0][:, None], cells_on_edge[es, 1][:, None]
        he = 0.5 * (h[c1, k] + h[c2, k])
        nue = 0.5 * (visc[c1, k] + visc[c2, k])
        yield es, k, he, nue, u[es[:, None], k]


def velocity_mix(h, vert_visc, u, dt, cells_on_edge, lo_edge_bot, hi_edge_top, n_owned):
    """applyVelocityVertMix: a new normal-velocity array"""
    out = np.array(u, dtype=np.float64, copy=True)
    for es, k, he, nue, ucol in edge_columns(h, vert_visc, out, cells_on_edge, lo_edge_bot, hi_edge_top, n_owned):
        g, hh, x = assemble(he, nue, ucol, dt)
        out[es[:, None], k] = pcr_diff(g, hh, x)
    return out


def dense_solve(g, h, x):
    """the backward-Euler system -G(i-1) x(i-1) + (H(i) + G(i-1) + G(i)) x(i) - G(i) x(i+1) = X(i), by
    numpy.linalg.solve (an independent check of the PCR solve)"""
    out = np.empty_like(x)
    for b in range(x.shape[0]):
        n = x.shape[1]
        a = np.zeros((n, n))
        for i in range(n):
            a[i, i] = h[b, i] + (g[b, i - 1] if i > 0 else 0.0) + g[b, i]
            if i + 1 < n:
                a[i, i + 1] = -g[b, i]
                a[i + 1, i] = -g[b, i]
        out[b] = np.linalg.solve(a, x[b])
    return out
