"""Properties of the 3-D form of the MonotoneAdv contract (omega_amd/csrc/MonotoneAdv.h), checked on its NumPy
restatement (tests/monotone_adv_reference.py), which the device reproduces bit for bit
(tests/test_monotone_adv_3d_gpu.py): with a vertical transport one forward step stays inside the range of each cell's
3-D neighbourhood, where the parent's path (the fixture asserts it) does not; it conserves the tracer content, keeps a
constant, is the 2-D form where nothing moves vertically, and agrees with VertAdv on the interface value."""
import math

import numpy as np
import pytest

from tests import monotone_adv_reference as MR
from tests import vert_adv_reference as VR
from tests.monotone_adv_fixtures import CONST, CONST_VALUE, RANDOM, STEP, Mono3Rig

MESHES = ("hex24x20", "ico3", "fib700_coast_ragged")
K = 6
EPS = 2.0 ** -53

_RIGS = {}


def rig(name, upwind=False):
    key = (name, upwind)
    if key not in _RIGS:
        R = Mono3Rig(name, K)
        _RIGS[key] = (R, R.inputs(seed=11, upwind=upwind))
    return _RIGS[key]


def margin_value(n, h_max, phi_max, h_new_min):
    """The margin of tests/test_monotone_adv.py (`margin`) with two more terms per sum.

    The quantities the limiter compares are now sums of at most n + 3 terms: the n slots, the cell's own and the two
    interfaces.  Under a combined outflow Courant number <= 1 an interface term is bounded like an edge term,
    Dt*|Wv|*|PhiT| <= max(h)*max|phi| <= S (PhiT is a convex combination of two phi for positive h).  Its chain has 9
    roundings (h[K-1] + h[K] 1, the quotient 1, phi[K] - phi[K-1] 1, its product 1, PhiT's sum 1, Wv* 1, VHigh - VLow 1,
    ScV*AV 1, VLow + 1) against the edge's 8; the sum adds n + 2, and Dt*, *InvA and the last operation 3: at most
    (n + 3)*(n + 14)*eps*S per quantity.  Five quantities and the division by hNew as there."""
    return 5.0 * (n + 3) * (n + 14) * EPS * (2.0 * h_max * phi_max) / h_new_min


def margin(R, I, L):
    nc = R.nc
    return margin_value(R.M.eoc.shape[1], I.h_old[:nc].max(), np.abs(I.tracers[L, :nc]).max(), I.h_new[:nc].min())


def forward_step(R, I, L):
    si, so, p_min, p_max = MR.scale_factors(R.M, I.h_old, I.h_new, I.u, I.tracers[L], I.dt, I.upwind, R.vert(I))
    tend = MR.flux_divergence(R.M, I.h_old, I.u, I.tracers[L], si, so, I.upwind, vert=R.vert(I))
    return R.forward(I, L, tend), p_min, p_max


def neighbourhood_range(R, I, L):
    """the 3-D range written from the edges and the interfaces, not from the cells' slots"""
    M, nc, phi = R.M, R.nc, I.tracers[L]
    lo, hi = phi[:nc].copy(), phi[:nc].copy()
    e = np.nonzero(M.open_edge)[0]
    for a, b in ((M.coe[e, 0], M.coe[e, 1]), (M.coe[e, 1], M.coe[e, 0])):
        np.minimum.at(lo, a, phi[b])
        np.maximum.at(hi, a, phi[b])
    for c in range(nc):
        for k in range(R.lo[c] + 1, R.hi[c] + 1):  # interface k joins the layers k-1 and k
            for a, b in ((k, k - 1), (k - 1, k)):
                lo[c, a], hi[c, a] = min(lo[c, a], phi[c, b]), max(hi[c, a], phi[c, b])
    return lo, hi


@pytest.mark.parametrize("upwind", (False, True))
@pytest.mark.parametrize("name", MESHES)
def test_update_stays_inside_the_3d_neighbourhood_range(name, upwind):
    R, I = rig(name, upwind)  # (the fixture has asserted that the parent's path leaves the range by > 1e-2)
    for L in (STEP, RANDOM, CONST):
        new, p_min, p_max = forward_step(R, I, L)
        lo, hi = neighbourhood_range(R, I, L)
        assert np.array_equal(lo, p_min) and np.array_equal(hi, p_max)
        m = margin(R, I, L)
        over = max((new - p_max).max(), (p_min - new).max())
        print(name, upwind, L, "outside by", over, "margin", m, "parent's path", R.parent_path_excess(I, L))
        assert np.isfinite(new).all()
        assert over <= m


def test_tracer_content_is_conserved_on_the_periodic_mesh():
    """sum over cells and levels of AreaCell*Tend = 0 in exact arithmetic: both cells of an edge hold the same bits of F
    and both layers of an interface the same bits of FV, with opposite signs.  Computed, per level as in
    tests/test_monotone_adv.py: a cell-level's sum of n + 2 terms errs by at most (n + 2)*eps*(sum of its |F|*InvA and
    |FV|), and *InvA, the test's *AreaCell and the inexact 1/AreaCell add 3 relative roundings, so the drift is at most
    (n + 5)*eps*2*(sum over edges of |F| + sum over interfaces of AreaCell*|FV|); the sum over cells and levels is
    taken exactly (math.fsum)."""
    R, I = rig("hex24x20")
    M, nc, n = R.M, R.nc, R.M.eoc.shape[1]
    assert M.open_edge.all()
    e = np.arange(M.ne)
    for L in (STEP, RANDOM):
        si, so, _, _ = MR.scale_factors(M, I.h_old, I.h_new, I.u, I.tracers[L], I.dt, vert=R.vert(I))
        tend = MR.flux_divergence(M, I.h_old, I.u, I.tracers[L], si, so, vert=R.vert(I))
        _, f_low, _, a = MR.edge_terms(M, e, M.coe[e, 0], M.coe[e, 1], I.h_old, I.u, I.tracers[L], False)
        f = f_low + MR.edge_scale(a, si, so, M.coe[e, 0], M.coe[e, 1]) * a
        fv = MR.vertical_flux(I.h_old, I.tracers[L], I.wt, R.lo, R.hi, nc, si, so)
        assert np.abs(fv).max() > 0.0
        drift = abs(math.fsum((R.area[:nc, None] * tend).ravel()))
        bound = (n + 5) * EPS * 2.0 * (np.abs(f).sum() + (R.area[:nc, None] * np.abs(fv)).sum())
        content = math.fsum((R.area[:nc, None] * I.h_old[:nc] * I.tracers[L, :nc]).ravel())
        print(L, "drift", drift, "bound", bound, "relative", I.dt * drift / abs(content))
        assert drift <= bound


@pytest.mark.parametrize("name", MESHES)
def test_constant_tracer_has_no_antidiffusive_vertical_flux(name):
    R, I = rig(name)
    inside, wv, _, phi_t, av = MR.interface_terms(I.h_old, I.tracers[CONST], I.wt, R.lo, R.hi, R.nc)
    assert (wv[inside] != 0.0).all() and not av.any()  # AV = 0 exactly: PhiT == phi bit for bit
    assert (phi_t[inside] == CONST_VALUE).all()
    assert R.limited_interfaces(I, CONST) == (0.0, 1.0)
    new, p_min, p_max = forward_step(R, I, CONST)
    assert (p_min == CONST_VALUE).all() and (p_max == CONST_VALUE).all()
    assert np.abs(new - CONST_VALUE).max() <= margin(R, I, CONST)


@pytest.mark.parametrize("name", MESHES)
def test_zero_transport_is_the_2d_form(name):
    """With VerticalTransport == 0 every vertical flux is 0.0 and (x - 0.0) + 0.0 == x for every x but -0.0, which
    becomes +0.0 (np.array_equal does not tell them apart).  What remains of the third dimension is the range: PMax and
    PMin take the levels above and below whatever moves through the interface, so a cell whose vertical neighbours
    widen its range may get larger scale factors than the 2-D form gives it.  Hence: tracers that are uniform in each
    column give the 2-D restatement's Tend, ScaleIn and ScaleOut; any tracer gives its scale factors on the cell-levels
    whose range the vertical neighbours leave as it is, and its Tend where that holds for the cell and all its
    neighbours."""
    R = rig(name)[0]
    nc = R.nc
    I = R.inputs(seed=11, check=False, wt_scale=0.0)
    assert not I.wt[:nc][R.inside].any() and np.isnan(I.wt[:nc][~R.inside]).all()
    want = R.reference_2d(I, 3)
    got = R.reference(I, 3)
    assert all(np.isfinite(a[:, :nc]).all() for a in got)
    for L in (STEP, RANDOM, CONST):
        _, _, p_min, p_max = MR.scale_factors(R.M, I.h_old, I.h_new, I.u, I.tracers[L], I.dt, vert=R.vert(I))
        _, _, q_min, q_max = MR.scale_factors(R.M, I.h_old, I.h_new, I.u, I.tracers[L], I.dt)
        same = (p_min == q_min) & (p_max == q_max)
        assert same.any()
        for w in (1, 2):
            assert np.array_equal(got[w][L, :nc][same], want[w][L, :nc][same])
        ok = same.copy()  # the cell and every cell across an open edge
        e = np.nonzero(R.M.open_edge)[0]
        for a, b in ((R.M.coe[e, 0], R.M.coe[e, 1]), (R.M.coe[e, 1], R.M.coe[e, 0])):
            np.logical_and.at(ok, a, same[b])
        assert np.array_equal(got[0][L, :nc][ok], want[0][L, :nc][ok])
    assert np.array_equal(got[0][CONST], want[0][CONST])
    I.tracers[:, :nc] = I.tracers[:, :nc, :1]  # uniform in each column
    for a, b in zip(R.reference(I, 3), R.reference_2d(I, 3)):
        assert np.isfinite(a[:, :nc]).all() and np.array_equal(a, b)


@pytest.mark.parametrize("name", MESHES)
def test_interface_value_is_vert_advs(name):
    """PhiT = phi[K-1] + (h[K-1]/(h[K-1] + h[K]))*(phi[K] - phi[K-1]) against VertAdv's order 2,
    (h[K-1]*phi[K] + h[K]*phi[K-1])/(h[K-1] + h[K]): each is the same convex combination with at most 5 roundings of
    values no larger than max|phi|, so they differ by at most 10 eps max|phi|"""
    R, I = rig(name)
    nc = R.nc
    inside, _, _, phi_t, _ = MR.interface_terms(I.h_old, I.tracers[RANDOM], I.wt, R.lo, R.hi, nc)
    want = VR.interface_value(I.h_old, I.tracers[RANDOM], I.wt, 2, nc)
    diff = np.abs(phi_t - want)[inside].max()
    print(name, "PhiT differs from VertAdv's by", diff)
    assert inside.any() and diff <= 10.0 * EPS * np.abs(I.tracers[RANDOM, :nc]).max()


def test_no_vertical_term_without_an_interface():
    # K = 1
    R = Mono3Rig("hex24x20", 1)
    I = R.inputs(seed=4, check=False)
    assert not R.inside.any() and np.isnan(I.wt).all()
    for a, b in zip(R.reference(I, 3), R.reference_2d(I, 3)):
        assert np.array_equal(a, b)
    # single-layer columns in a deep mesh: hNew, hence everything, is the 2-D one's there whatever the neighbours do
    R, I = rig("hex24x20")
    lo, hi = R.lo.copy(), R.hi.copy()
    cells = np.arange(0, R.nc, 5)
    lo[cells], hi[cells] = 2, 2
    J = R.inputs(seed=11, check=False)
    keep = MR.interface_mask(lo, hi, R.nc, K)
    J.wt[: R.nc][~keep] = np.nan
    vdiv, _ = MR.thickness_divergence(J.wt, lo, hi, R.nc)
    assert not vdiv[cells].any()
    for L in (STEP, RANDOM):
        fv = MR.vertical_flux(J.h_old, J.tracers[L], J.wt, lo, hi, R.nc, np.ones((R.nc, K)), np.ones((R.nc, K)))
        assert not fv[cells].any() and fv.any()
        _, _, p_min, p_max = MR.scale_factors(R.M, J.h_old, J.h_new, J.u, J.tracers[L], J.dt, vert=(J.wt, lo, hi))
        _, _, q_min, q_max = MR.scale_factors(R.M, J.h_old, J.h_new, J.u, J.tracers[L], J.dt)
        assert np.array_equal(p_min[cells], q_min[cells]) and np.array_equal(p_max[cells], q_max[cells])
