"""Properties of the MonotoneAdv contract (omega_amd/csrc/MonotoneAdv.h), checked on its NumPy restatement
(tests/monotone_adv_reference.py), which the device reproduces bit for bit (tests/test_monotone_adv_gpu.py): one forward
step stays inside the range of each cell's neighbourhood where the centred flux does not, conserves the tracer content,
keeps a constant, reads nothing across a coast, and is the centred scheme where nothing is limited."""
import math

import numpy as np
import pytest

from tests import monotone_adv_reference as MR
from tests.monotone_adv_fixtures import CONST, CONST_VALUE, RANDOM, STEP, MonoRig

MESHES = ("hex24x20", "ico3", "fib700_coast_ragged")
K = 3
EPS = 2.0 ** -53

_RIGS = {}


def rig(name, upwind=False):
    """(rig, inputs) of a mesh, built once"""
    key = (name, upwind)
    if key not in _RIGS:
        R = MonoRig(name, K)
        _RIGS[key] = (R, R.inputs(seed=11, upwind=upwind))
    return _RIGS[key]


def forward_step(R, I, L, flux="limited"):
    """(phi_new, PMin, PMax) on the local cells: (hOld*phi + Dt*Tend)/hNew with Tend the divergence of `flux`"""
    nc = R.nc
    si, so, p_min, p_max = MR.scale_factors(R.M, I.h_old, I.h_new, I.u, I.tracers[L], I.dt, I.upwind)
    tend = MR.flux_divergence(R.M, I.h_old, I.u, I.tracers[L], si, so, I.upwind, flux)
    return (I.h_old[:nc] * I.tracers[L, :nc] + I.dt * tend) / I.h_new[:nc], p_min, p_max


def margin(R, I, L):
    """How far rounding may carry the updated value outside [PMin, PMax].

    In exact arithmetic it is inside (MonotoneAdv.h).  In FP64 the argument compares quantities of dimension h*phi: HTd,
    PMax*hNew (PMin*hNew), Dt*InvA*(the sum of the positive s*A), Dt*InvA*(the sum of the limited s*F) and the numerator
    hOld*phi + Dt*Tend.  Each is a sum of at most n + 1 terms, n = MaxEdges slots and the cell's own.  Under an outflow
    Courant number <= 1 a term is at most S = 2*max(h)*max|phi| in magnitude: Dt*InvA*|Fm| <= h of the upwind cell
    times the ratio of the two cells' areas, which is below 2 on these meshes.  A term is a product chain of at most 8
    roundings (hE 1, hE*u 1, DvEdge* 1, phi0 + phi1 1, Fm* 1, FHigh - FLow 1, Sc*A 1, FLow + 1; 0.5* and s* are exact),
    its sum adds n, and Dt*, *InvA and the quantity's last operation 3: an absolute error of at most
    (n + 1)*(n + 11)*eps*S per quantity, eps = 2^-53.  Five quantities enter -- the four the limiter compares and hNew,
    which is the thickness of the same mass fluxes only up to such an error, times phi -- and the division by hNew turns
    their sum into the margin 5*(n + 1)*(n + 11)*eps*S/min(hNew).  (Observed: at most 2 ulp of max|phi|.)"""
    nc = R.nc
    return margin_value(R.M.eoc.shape[1], I.h_old[:nc].max(), np.abs(I.tracers[L, :nc]).max(), I.h_new[:nc].min())


def margin_value(n, h_max, phi_max, h_new_min):
    """the margin derived in `margin` from its four figures"""
    return 5.0 * (n + 1) * (n + 11) * EPS * (2.0 * h_max * phi_max) / h_new_min


@pytest.mark.parametrize("upwind", (False, True))
@pytest.mark.parametrize("name", MESHES)
def test_update_stays_inside_the_neighbourhood_range(name, upwind):  # (i)
    R, I = rig(name, upwind)
    for L in (STEP, RANDOM, CONST):
        new, p_min, p_max = forward_step(R, I, L)
        m = margin(R, I, L)
        over = max((new - p_max).max(), (p_min - new).max())
        print(name, upwind, L, "outside by", over, "margin", m)
        assert np.isfinite(new).all()
        assert over <= m


@pytest.mark.parametrize("name", MESHES)
def test_centred_flux_leaves_the_range(name):  # (ii): the assertion of (i) can fail
    R, I = rig(name)
    new, p_min, p_max = forward_step(R, I, STEP, flux="high")
    over = max((new - p_max).max(), (p_min - new).max())
    print(name, "centred flux outside by", over)
    assert over > 1.0e-2
    # and the upwind flux alone stays inside, to the same margin
    new, p_min, p_max = forward_step(R, I, STEP, flux="low")
    assert max((new - p_max).max(), (p_min - new).max()) <= margin(R, I, STEP)


def test_tracer_content_is_conserved_on_the_periodic_mesh():  # (iii)
    """sum_c AreaCell*(Dt*Tend) = 0 in exact arithmetic: both cells of an edge hold the same bits of F with opposite
    signs.  Computed: the sum of a cell's n terms errs by at most n*eps*sum|F|, *InvA and the test's own *AreaCell and
    the inexact 1/AreaCell add 3 relative roundings, so |sum_c A_c*Tend_c| <= (n + 3)*eps*(sum over cells and slots of
    |F|) = (n + 3)*eps*2*(sum over edges of |F|); the sum over cells is taken exactly (math.fsum)."""
    R, I = rig("hex24x20")
    M, nc, n = R.M, R.nc, R.M.eoc.shape[1]
    assert M.open_edge.all()
    e = np.arange(M.ne)
    for L in (STEP, RANDOM):
        si, so, _, _ = MR.scale_factors(M, I.h_old, I.h_new, I.u, I.tracers[L], I.dt)
        tend = MR.flux_divergence(M, I.h_old, I.u, I.tracers[L], si, so)
        _, f_low, _, a = MR.edge_terms(M, e, M.coe[e, 0], M.coe[e, 1], I.h_old, I.u, I.tracers[L], False)
        f = f_low + MR.edge_scale(a, si, so, M.coe[e, 0], M.coe[e, 1]) * a
        for k in range(K):
            drift = abs(math.fsum(R.area[:nc] * tend[:, k]))
            bound = (n + 3) * EPS * 2.0 * np.abs(f[:, k]).sum()
            content = math.fsum(R.area[:nc] * I.h_old[:nc, k] * I.tracers[L, :nc, k])
            print(L, k, "drift", drift, "bound", bound, "relative", I.dt * drift / abs(content))
            assert drift <= bound


@pytest.mark.parametrize("name", MESHES)
def test_constant_tracer_stays_constant(name):  # (iv)
    R, I = rig(name)
    e = np.nonzero(R.M.open_edge)[0]
    a = MR.edge_terms(R.M, e, R.M.coe[e, 0], R.M.coe[e, 1], I.h_old, I.u, I.tracers[CONST], False)[3]
    assert not a.any()  # A = 0 exactly: FHigh == FLow bit for bit
    new, p_min, p_max = forward_step(R, I, CONST)
    assert (p_min == CONST_VALUE).all() and (p_max == CONST_VALUE).all()
    assert np.abs(new - CONST_VALUE).max() <= margin(R, I, CONST)  # the margin of (i) with PMin = PMax


def test_coast_edges_contribute_nothing():  # (v)
    R, I = rig("fib700_coast_ragged")
    M, nc, ne = R.M, R.nc, R.ne
    closed = np.nonzero(~M.open_edge)[0]
    assert closed.size > 0 and np.isnan(I.h_old[nc:]).all() and np.isnan(I.tracers[:, nc:]).all()
    assert (M.coe[closed] >= nc).any()  # the missing cell is the sentinel row, which holds NaN
    ref = R.reference(I, 3)
    assert all(np.isfinite(x[:, :nc]).all() for x in ref)
    # the velocity on a closed edge is never read
    J = R.inputs(seed=11)
    J.u[closed] = np.nan
    assert all(np.array_equal(a, b) for a, b in zip(R.reference(J, 3), ref))
    # PMin / PMax are those of the neighbours across open edges only
    phi = I.tracers[RANDOM]
    _, _, p_min, p_max = MR.scale_factors(M, I.h_old, I.h_new, I.u, phi, I.dt)
    lo, hi = phi[:nc].copy(), phi[:nc].copy()
    e = np.nonzero(M.open_edge)[0]
    for a, b in ((M.coe[e, 0], M.coe[e, 1]), (M.coe[e, 1], M.coe[e, 0])):
        np.minimum.at(lo, a, phi[b])
        np.maximum.at(hi, a, phi[b])
    assert np.array_equal(lo, p_min) and np.array_equal(hi, p_max)


@pytest.mark.parametrize("name", MESHES)
def test_unlimited_is_the_centred_tendency(name):  # (vi)
    """with Sc == 1 on every edge pass 2 is the divergence of FLow + A, bit for bit -- written here from the edges, not
    from the cells' slots -- which is the centred flux FHigh up to the rounding of (FHigh - FLow) + FLow"""
    R, I = rig(name)
    M, nc = R.M, R.nc
    one = np.ones((nc, K))
    got = MR.flux_divergence(M, I.h_old, I.u, I.tracers[RANDOM], one, one)
    e = np.arange(M.ne)[M.open_edge]
    c0, c1 = M.coe[e, 0], M.coe[e, 1]
    _, f_low, f_high, a = MR.edge_terms(M, e, c0, c1, I.h_old, I.u, I.tracers[RANDOM], False)
    f_of = np.zeros((M.ne, K))
    f_of[e] = f_low + 1.0 * a
    want = np.zeros((nc, K))
    for j in range(M.eoc.shape[1]):
        r = np.nonzero(j < M.neoc[:nc])[0]
        ej = M.eoc[r, j]
        ok = (ej >= 0) & (ej < M.ne)
        r, ej = r[ok], ej[ok]
        r, ej = r[M.open_edge[ej]], ej[M.open_edge[ej]]
        want[r] = want[r] + M.sign[r, j][:, None] * f_of[ej]
    want = want * M.inv_area[:, None]
    assert np.array_equal(got, want)
    # (FHigh - FLow) + FLow misses FHigh by the two roundings, each at most eps*(|FLow| + |FHigh|)
    assert (np.abs((f_low + a) - f_high) <= 2.0 * EPS * (np.abs(f_low) + np.abs(f_high))).all()
