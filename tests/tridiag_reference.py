"""NumPy restatement of the batched tridiagonal solvers' contract (omega_amd/csrc/TriDiagSolvers.h), vectorised over
the batch and, for PCR, over the rows.  Each function follows the reference's operation order and association
(components/omega/src/base/TriDiagSolvers.h) expression by expression, in FP64 without contraction, so the GPU results
equal these bit for bit.  Inputs are [NBatch][NRow] arrays; they are not modified; the solution is returned."""
import numpy as np


def _f(a):
    return np.array(a, dtype=np.float64, copy=True)


def pcr_levels(nrow: int) -> int:
    """ceil(log2(nrow)) for nrow > 1 (TriDiagSolvers.h:160)"""
    lev = 0
    while (1 << lev) < nrow:
        lev += 1
    return lev


def thomas(dl, d, du, x):
    """ThomasSolver::solve (TriDiagSolvers.h:69-93)"""
    dl, d, du, x = _f(dl), _f(d), _f(du), _f(x)
    n = x.shape[1]
    with np.errstate(all="ignore"):
        for k in range(1, n):
            w = dl[:, k] / d[:, k - 1]
            d[:, k] = d[:, k] - w * du[:, k - 1]
            x[:, k] = x[:, k] - w * x[:, k - 1]
        x[:, n - 1] = x[:, n - 1] / d[:, n - 1]
        for k in range(n - 2, -1, -1):
            x[:, k] = (x[:, k] - du[:, k] * x[:, k + 1]) / d[:, k]
    return x


def thomas_diff(g, h, x):
    """ThomasDiffusionSolver::solve (TriDiagSolvers.h:276-320)"""
    g, h, x = _f(g), _f(h), _f(x)
    n = x.shape[1]
    alpha = np.zeros_like(x)
    with np.errstate(all="ignore"):
        for k in range(1, n):
            alpha[:, k] = g[:, k - 1] * (h[:, k - 1] + alpha[:, k - 1]) / (h[:, k - 1] + alpha[:, k - 1] + g[:, k - 1])
        h[:, 0] = h[:, 0] + g[:, 0]
        for k in range(1, n):
            add_h = alpha[:, k] + g[:, k]
            h[:, k] = h[:, k] + add_h
            x[:, k] = x[:, k] + g[:, k - 1] / h[:, k - 1] * x[:, k - 1]
        x[:, n - 1] = x[:, n - 1] / h[:, n - 1]
        for k in range(n - 2, -1, -1):
            x[:, k] = (x[:, k] + g[:, k] * x[:, k + 1]) / h[:, k]
    return x


def pcr(dl, d, du, x):
    """PCRSolver::solve (TriDiagSolvers.h:152-213); nrow = 1 is the 1x1 solve x / d"""
    dl, d, du, x = _f(dl), _f(d), _f(du), _f(x)
    n = x.shape[1]
    with np.errstate(all="ignore"):
        if n == 1:
            return x / d
        nlev = pcr_levels(n)
        k = np.arange(n)
        for lev in range(1, nlev):
            hs = 1 << (lev - 1)
            kmh = np.maximum(k - hs, 0)
            kph = np.minimum(k + hs, n - 1)
            alpha = -dl / d[:, kmh]
            gamma = -du / d[:, kph]
            new_d = d + alpha * du[:, kmh] + gamma * dl[:, kph]
            new_x = x + alpha * x[:, kmh] + gamma * x[:, kph]
            new_dl = alpha * dl[:, kmh]
            new_du = gamma * du[:, kph]
            d, x, dl, du = new_d, new_x, new_dl, new_du
        s = 1 << (nlev - 1)
        out = x.copy()
        for kk in range(n):
            if kk + s < n or kk - s >= 0:
                if kk < n // 2:
                    p = kk + s
                    det = d[:, kk] * d[:, p] - dl[:, p] * du[:, kk]
                    xk, xkps = x[:, kk], x[:, p]
                    out[:, kk] = (d[:, p] * xk - du[:, kk] * xkps) / det
                    out[:, p] = (-dl[:, p] * xk + d[:, kk] * xkps) / det
            else:
                out[:, kk] = x[:, kk] / d[:, kk]
    return out


def pcr_diff(g, h, x):
    """PCRDiffusionSolver::solve (TriDiagSolvers.h:377-454); nrow = 1 is the 1x1 solve x / (h + g)"""
    g, h, x = _f(g), _f(h), _f(x)
    n = x.shape[1]
    with np.errstate(all="ignore"):
        if n == 1:
            return x / (h + g)
        nlev = pcr_levels(n)
        k = np.arange(n)
        nb = x.shape[0]
        zero = np.zeros((nb, n))
        for lev in range(1, nlev):
            st, hs = 1 << lev, 1 << (lev - 1)
            kmh = k - hs
            gkmh = np.where(kmh < 0, zero, g[:, np.maximum(kmh, 0)])
            kmh = np.maximum(kmh, 0)
            kms = k - st
            gkms = np.where(kms < 0, zero, g[:, np.maximum(kms, 0)])
            kph = np.minimum(k + hs, n - 1)
            alpha = gkmh / (h[:, kmh] + gkms + gkmh)
            beta = g / (h[:, kph] + g + g[:, kph])
            new_g = g[:, kph] * beta
            new_x = x + alpha * x[:, kmh] + beta * x[:, kph]
            new_h = h + alpha * h[:, kmh] + beta * h[:, kph]
            h, g, x = new_h, new_g, new_x
        s = 1 << (nlev - 1)
        out = x.copy()
        for kk in range(n):
            if kk + s < n or kk - s >= 0:
                if kk < n // 2:
                    p = kk + s
                    gkms = g[:, kk - s] if kk - s >= 0 else 0.0
                    dk = h[:, kk] + gkms + g[:, kk]
                    dkps = h[:, p] + g[:, kk] + g[:, p]
                    duk = -g[:, kk]
                    dlkps = -g[:, kk]
                    det = dk * dkps - dlkps * duk
                    xk, xkps = x[:, kk], x[:, p]
                    out[:, kk] = (dkps * xk - duk * xkps) / det
                    out[:, p] = (-dlkps * xk + dk * xkps) / det
            else:
                gkms = g[:, kk - s] if kk - s >= 0 else 0.0
                out[:, kk] = x[:, kk] / (h[:, kk] + gkms + g[:, kk])
    return out


GENERAL = {"thomas": thomas, "pcr": pcr}
DIFFUSION = {"thomas": thomas_diff, "pcr": pcr_diff}


# ---------------------------------------------------------------------------------------------------------------------
# the reference's unit test (components/omega/test/base/TriDiagSolversTest.cpp), with the solve as a parameter
# ---------------------------------------------------------------------------------------------------------------------

def correctness_system(nbatch, nrow):
    """testCorrectness (TriDiagSolversTest.cpp:15-65): (dl, d, du, x_exact, ax)"""
    i = np.arange(nbatch)[:, None].astype(np.float64)
    ii = np.arange(nbatch)[:, None]
    k = np.arange(nrow)[None, :]
    kf = k.astype(np.float64)
    x = 0.1 * kf + 0.3 * (ii % 12) + 0 * i
    dl = np.where(k == 0, 0.0, 1 + 0.1 * (ii % 3) + 0.2 * (k % 7))
    d = 4 + 0.2 * (ii % 11) + 0.1 * (k % 5) + 0 * kf
    du = np.where(k == nrow - 1, 0.0, 1 + 0.05 * (ii % 5) - 0.1 * (k % 11))
    ax = d * x
    ax[:, 1:] += dl[:, 1:] * x[:, :-1]
    ax[:, :-1] += du[:, :-1] * x[:, 1:]
    return dl, d, du, x, ax


def diffusion_correctness_system(nbatch, nrow):
    """testDiffusionCorrectness (TriDiagSolversTest.cpp:67-119): (g, h, x_exact, ax)"""
    ii = np.arange(nbatch)[:, None]
    k = np.arange(nrow)[None, :]
    kf = k.astype(np.float64)
    x = 0.1 * kf + 0.3 * (ii % 12)
    g = np.where(k == nrow - 1, 0.0, 1 + 0.1 * (ii % 3) + 0.2 * (k % 7))
    h = 4 + 0.2 * (ii % 11) + 0.1 * (k % 5) + 0 * kf
    dlm = np.where(k == 0, 0.0, -np.concatenate([np.zeros((nbatch, 1)), g[:, :-1]], axis=1))
    dum = -g
    dm = h - dlm - dum
    ax = dm * x
    ax[:, 1:] += dlm[:, 1:] * x[:, :-1]
    ax[:, :-1] += dum[:, :-1] * x[:, 1:]
    return g, h, x, ax


def diff_manufactured(ncells, diff_solve):
    """runDiffManufactured (TriDiagSolversTest.cpp:122-244): backward Euler on a manufactured solution, one
    diff_solve(g, h, x) per step on [1][ncells] systems; returns the L2 error at t = 1"""
    nvert = ncells + 1
    time_end = 1.0
    dt = 0.001 / (ncells // 100)
    nsteps = int(np.ceil(time_end / dt))
    xv = np.tanh(5 * (np.arange(nvert) * (1.0 / ncells)))
    diffusivity = 2 + np.sin(xv)
    xc = (xv[1:] + xv[:-1]) / 2
    thick = xv[1:] - xv[:-1]
    u = np.cos(xc) * np.sin(0.0)
    xbnd = xv[ncells]
    bcoeff = -(2 + np.sin(xbnd)) * np.tan(xbnd)
    avg = (thick[1:] + thick[:-1]) / 2
    for step in range(nsteps):
        t_next = (step + 1) * dt
        f = (2 * np.sin(t_next) * np.sin(xc) + 2 * np.sin(t_next) + np.cos(t_next)) * np.cos(xc)
        h = thick.copy()
        h[-1] -= dt * bcoeff
        g = np.zeros(ncells)
        g[:-1] = diffusivity[1:ncells] * dt / avg
        x = thick * (u + dt * f)
        u = np.asarray(diff_solve(g[None, :], h[None, :], x[None, :]))[0]
    du = u - np.cos(xc) * np.sin(time_end)
    return float(np.sqrt(np.sum(thick * du * du)))


def diffusion_stability(general, diff_value, solve):
    """runDiffusionStability (TriDiagSolversTest.cpp:270-435): 100 backward-Euler steps with a discontinuous
    diffusivity, solve(dl, d, du, x) (general) or solve(g, h, x); returns the normalised change of the norm"""
    ncells = 100
    dx = 1.0 / ncells
    xv = np.arange(ncells + 1) * dx
    diffusivity = np.where(np.abs(xv - 0.5) < 0.2, diff_value, 0.0)
    xc = np.arange(ncells) * dx + dx / 2
    thick = np.full(ncells, dx)
    tmp = xc - 0.5
    u = np.exp(-tmp * tmp)
    norm0 = np.sqrt(np.sum(thick * u * u))
    dt = 1.0
    avg = (thick[1:] + thick[:-1]) / 2
    with np.errstate(all="ignore"):
        for _ in range(100):
            if general:
                du = np.zeros(ncells)
                du[:-1] = -diffusivity[1:ncells] * dt / avg
                dl = np.zeros(ncells)
                dl[1:] = -diffusivity[1:ncells] * dt / avg
                d = thick - du - dl
                x = thick * u
                u = np.asarray(solve(dl[None, :], d[None, :], du[None, :], x[None, :]))[0]
            else:
                g = np.zeros(ncells)
                g[:-1] = diffusivity[1:ncells] * dt / avg
                x = thick * u
                u = np.asarray(solve(g[None, :], thick[None, :].copy(), x[None, :]))[0]
        norm = np.sqrt(np.sum(thick * u * u))
    return float((norm - norm0) / norm0)


def is_approx(x, y, rtol, atol=0.0):
    """isApprox (test/ocn/OceanTestCommon.h:15-23)"""
    if not (np.isfinite(x) and np.isfinite(y)):
        return False
    return abs(x - y) <= max(atol, rtol * max(abs(x), abs(y)))
