"""The all-host Split-Explicit step (tests/model_step_reference.py) by itself, and the rig's power to see mistakes: what
two host steps on the periodic rig conserve and keep, every named deviation of the sequence changing the state on every
rig the GPU comparison (tests/test_model_step_gpu.py) runs, and the empty rung equal to the oracle-fed
split_explicit_reference.step written out on the spot.  For the rungs that attach the Redi, the Kpp and the VertRemap
also: volume and tracer content conserved on every one of them, a constant tracer constant through Redi and remap, and
the conditions on the inputs under which the Kpp rungs can be compared bit for bit (no cbrt evaluated, no marginal
column, and a boundary layer that does something).  No device."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as O
from tests import split_explicit_reference as SR
from tests.barotropic_fixtures import GRAVITY, btr_mesh
from tests.model_step_fixtures import DT, NEW_RUNGS, NSUB, RUNGS, ModelRig, deviations_of
from tests.model_step_reference import DEVIATIONS

EPS = np.finfo(np.float64).eps
STEPS = 2
PERIODIC = RUNGS["F"]  # planar_hex(8, 8), K = 5, everything attached


def _exact(area, *fields):
    """sum over cells and levels of area * field * field ..., in rationals"""
    total = Fraction(0)
    for c in range(len(area)):
        a = Fraction(float(area[c]))
        for k in range(fields[0].shape[1]):
            t = a
            for f in fields:
                t *= Fraction(float(f[c, k]))
            total += t
    return total


def _transport_scale(x):
    """D: an upper bound of Dt times the sum of the magnitudes of the terms of one cell-level's thickness tendency --
    MaxEdges horizontal ones, each at most DvEdge hE |u| / AreaCell, and the transport through its two interfaces"""
    n, ne = x.nc, x.ne
    h_max = max(x.h[0][:n].max(), x.h[1][:n].max())
    per_edge = x.dv[:ne].max() * h_max * np.abs(x.transporting_velocity[:ne]).max() / x.area[:n].min()
    return x.dt * (x.eoc.shape[1] * per_edge + 2.0 * np.abs(x.VerticalTransport[:n]).max())


def _no_surface_flux(g, G):
    G["SurfaceTracerFlux"][:] = 0.0


def test_total_volume_is_conserved():
    """sum A h, the products and the sum taken exactly, after each of two steps against the step's start.  In exact
    arithmetic the horizontal fluxes cancel between the two cells of an edge and the vertical ones between the two layers
    of an interface, with whatever rounded value the flux itself has.  What does not cancel, per cell-level, in units of
    eps/2: the update h + Dt Tend rounds once at |hNew| and its product Dt*Tend once at Dt |Tend| <= D; the tendency is a
    chain over at most MaxEdges = 6 terms (DvEdge s F) InvA with 3 roundings each after F (the two products and InvA
    itself) and 6 additions, then 2 additions for the vertical pair: at most 3 + 6 + 2 = 11 roundings of at most D.  So
    |sum A hNew - sum A h| <= eps/2 sum_{c,K} A_c (|hNew| + 12 D), D as in _transport_scale.  VertMixStep does not touch
    the thickness."""
    x = ModelRig(PERIODIC, device=False).host
    n, area = x.nc, x.area
    before = _exact(area[:n], x.h[0][:n])
    for step in range(STEPS):
        h, _, _ = x.step()
        after = _exact(area[:n], h[:n])
        bound = EPS / 2 * float((area[:n, None] * (np.abs(h[:n]) + 12.0 * _transport_scale(x))).sum())
        err = abs(float(after - before))
        print(f"step {step + 1}: |change of sum A h| = {err:.3e} m^3 of {float(after):.3e}, bound {bound:.3e} ({err / bound:.3f})")
        assert err <= bound
        assert not np.array_equal(h[:n], x.h[1][:n])  # the layers moved
        before = after


def test_total_tracer_content_is_conserved_without_surface_fluxes():
    """sum A h phi, taken exactly, for temperature and salinity with SurfaceTracerFlux = 0 and everything else of rung F
    on.  Per cell-level, in units of eps/2:
      - the update phiNew = ((phi h) + Dt Tend) / hNew rounds 4 times (two products, the sum, the quotient) at about
        |h phi| each: 4 |h phi|;
      - TracerTend is flux-form in every term (the limited horizontal and vertical fluxes, the Laplacian's edge fluxes):
        a flux's own roundings cancel between its two cells; what is left is the chain over at most 6 + 2 flux terms and
        up to 3 tendency terms added together, 3 roundings each after the flux and one per addition, fewer than 16 on
        the sum of their magnitudes, which is at most |phi|max D for the advective ones plus the diffusive
        Dt EddyDiff2 6 (Dv / Dc) hMax spread / A, spread the tracer's range: 16 (|phi|max D + Ddiff);
      - the implicit vertical diffusion conserves sum_K h phi of a column exactly (the rows of its matrix sum to H); the
        PCR solve of L = ceil(log2 n) levels leaves a residual of at most (8 L + 6) roundings of (|A| |x| + |b|) per row,
        |A| |x| <= (h + 4 G) |phi|max, G = VertDiff Dt / hMid: (8 L + 6) ((h + 4 G) |phi|max + |h phi|).
    Bound: eps/2 sum A_c of the three."""
    rig = ModelRig(PERIODIC, device=False, change=_no_surface_flux)
    x = rig.host
    n, area, K = x.nc, x.area, x.K
    assert np.all(x.f["SurfaceTracerFlux"] == 0.0) and x.opt["mix"] and x.opt["gm"]
    levels = int(np.ceil(np.log2(K)))
    before = [_exact(area[:n], x.h[0][:n], x.tr[0][t, :n]) for t in range(x.nt)]
    for step in range(STEPS):
        old_tr = x.tr[0].copy()
        h, _, tr = x.step()
        D = _transport_scale(x)
        h_max = max(h[:n].max(), x.h[1][:n].max())
        g_max = x.VertDiff[:n].max() * x.dt_seconds / h[:n].min()
        for t in range(x.nt):
            p_max = max(np.abs(tr[t, :n]).max(), np.abs(old_tr[t, :n]).max())
            spread = old_tr[t, :n].max() - old_tr[t, :n].min()
            d_diff = x.dt * x.orc.c.EddyDiff2 * 6.0 * (x.dv[: x.ne] / x.dc[: x.ne]).max() * h_max * spread / area[:n].min()
            per = 4.0 * h_max * p_max + 16.0 * (p_max * D + d_diff) + (8 * levels + 6) * (h_max * (1.0 + 4.0 * g_max) * p_max + h_max * p_max)
            bound = EPS / 2 * float(area[:n].sum() * K * per)
            after = _exact(area[:n], h[:n], tr[t, :n])
            err = abs(float(after - before[t]))
            print(f"step {step + 1}, tracer {t}: |change of sum A h phi| = {err:.3e} of {float(after):.3e}, bound {bound:.3e} "
                  f"({err / bound:.3f})")
            assert err <= bound
            before[t] = after
        assert not np.array_equal(tr[:, :n], old_tr[:, :n])


def test_a_constant_tracer_stays_constant_under_the_3d_limiter_and_the_bolus_flow():
    """Temperature = 10 everywhere, rung E (3-D MonotoneAdv at order 4, GentMcWilliams, PressureGrad, VertAdv).  With a
    constant phi the Hessians are 0 exactly, the high and the low flux are both Fm phi, the vertical interface value is
    phi (hu + hl) / (hu + hl), and the Laplacian's differences are 0: TracerTend = phi times the thickness tendency up to
    rounding, so phiNew = (phi h + Dt phi Tend) / hNew = phi.  Roundings, relative, in units of eps/2: 4 of the update
    (two products, the sum, the quotient); and the two tendencies, evaluated by different chains, differ by fewer than
    2 (6 + 2 + 5) + 6 roundings of the sum of the magnitudes of their terms, which relative to h is C = D / min h:
    |phiNew / phi - 1| <= eps/2 (4 + 32 C) per step."""
    phi0 = 10.0

    def constant(g, G):
        G["tr"][0][:] = phi0

    x = ModelRig(RUNGS["E"], device=False, change=constant).host
    n = x.nc
    bound = 0.0
    for step in range(STEPS):
        h, _, tr = x.step()
        c = _transport_scale(x) / min(h[:n].min(), x.h[1][:n].min())
        bound += EPS / 2 * (4.0 + 32.0 * c)
        dev = np.abs(tr[0, :n] / phi0 - 1.0).max()
        print(f"step {step + 1}: max |T / T0 - 1| = {dev:.3e}, bound {bound:.3e}, C = {c:.3e}")
        assert dev <= bound * (1.0 + 1.0e-6)
    assert np.abs(x.BolusVelocity[: x.ne]).max() > 0.0 and np.abs(x.VerticalTransport[:n]).max() > 0.0
    assert (x.ScaleIn[1, :n] < 1.0).any()  # the limiter was at work on the salinity
    assert not np.array_equal(tr[1, :n], x.start[2][1, :n])


def test_the_bolus_flow_never_reaches_the_prognostic_velocity():
    """one step of rung E against one of rung D (the same without the GentMcWilliams): u equal in every bit, tracers not"""
    with_gm, without = ModelRig(RUNGS["E"], device=False).host, ModelRig(RUNGS["D_order4"], device=False).host
    (_, ua, ta), (_, ub, tb) = with_gm.step(), without.step()
    assert np.array_equal(ua, ub) and not np.array_equal(ua, with_gm.start[1])
    assert not np.array_equal(ta, tb)
    assert not np.array_equal(with_gm.transporting_velocity, without.transporting_velocity)


def test_rest_with_flat_layers_stays_at_rest():
    """u = 0, every cell the same column (thickness, temperature, salinity), BottomDepth the ascending sum of the
    thicknesses, uniform forcing, no wind, everything of rung F attached: every horizontal difference is of two equal
    numbers, so the velocity stays 0.0 and the thickness keeps its bits through two steps; the tracers only mix
    vertically and stay the same in every cell."""
    def flat(g, G):
        K = G["h"].shape[1]
        col = 10.0 + np.arange(K)
        G["h"][:], G["ref"][:] = col, col
        G["un"][:] = 0.0
        G["tr"][0][:], G["tr"][1][:] = 20.0 - 3.0 * np.arange(K), 34.0 + 0.3 * np.arange(K)
        total = 0.0
        for k in range(K):
            total = total + col[k]
        G["bottom"][:] = total
        G["SurfacePressure"][:], G["TidalPotential"][:], G["SelfAttractionLoading"][:] = 1.0e5, 0.25, -0.05
        G["NormalStressEdge"][:] = 0.0
        G["SurfaceTracerFlux"][0][:], G["SurfaceTracerFlux"][1][:] = 1.0e-4, -2.0e-5

    x = ModelRig(PERIODIC, device=False, change=flat).host
    n, ne = x.nc, x.ne
    h0 = x.h[0].copy()
    for _ in range(STEPS):
        h, u, tr = x.step()
        assert np.all(u[:ne] == 0.0) and np.all(x.split.vel[:ne] == 0.0) and np.all(x.split.ssh[:n] == 0.0)
        assert np.array_equal(h, h0)
        assert np.all(tr[:, :n] == tr[:, :1]) and np.isfinite(tr).all()
        assert np.all(x.BolusVelocity[:ne] == 0.0) and np.all(x.VerticalTransport[:n] == 0.0)
    assert not np.array_equal(tr[:, :n], x.start[2][:, :n])  # the surface fluxes and the mixing moved them


# ---------------------------------------------------------------------------------------------------------------------
# the rungs with the Redi, the Kpp and the VertRemap
# ---------------------------------------------------------------------------------------------------------------------
KPP_RUNGS = [r for r in NEW_RUNGS if RUNGS[r]["opt"].get("kpp")]


def _masked(x, field):
    """the field on the rows < NCellsAll with 0.0 outside the layer ranges"""
    return np.where(x.c_range[: x.nc], field[: x.nc], 0.0)


def _closed_coast(g, G):
    """No flow through the coast: the rigs draw a velocity on every edge, those with one cell included, and what
    passes such an edge is a source of volume.  (Its velocity then stays 0.0: EdgeMask.)"""
    G["un"][np.asarray(g["cellsOnEdge"]).min(axis=1) < 0] = 0.0


def _closed(g, G):
    _closed_coast(g, G)
    _no_surface_flux(g, G)


@pytest.mark.parametrize("rung", KPP_RUNGS)
def test_the_kpp_rungs_evaluate_no_cbrt_and_have_a_boundary_layer_at_work(rung):
    """What lets the GPU comparison ask for bits on a rung with a Kpp, shown on the host reference alone, in both steps.
    The forcing: with sw <= eps under Bf < 0 every velocity scale is evaluated at z = kappa sig h Bf with sig <= eps and
    h at most the column's depth d, and the cbrt branches are taken below ZetaM u3 = -0.2 us^3 (wM) and -us^3 (wS): none
    is, where kappa eps d |Bf| <= 0.2 us^3.  The restatement's own flags say the same and that no comparison of the
    contract is within rounding of flipping.  And the layer is not an empty one: the non-local shape is there under
    Bf < 0, both signs of Bf occur, the layer ends inside at least a quarter of the columns of three or more layers and
    reaches the bottom of others, and inside it VertDiff is no longer what step 4 wrote."""
    x = ModelRig(rung, device=False).host
    n, lo, hi = x.nc, x.lo[: x.nc].astype(np.int64), x.hi[: x.nc].astype(np.int64)
    us, bf = x.f["FrictionVelocity"][:n], x.f["SurfaceBuoyancyFlux"][:n]
    cfg = x.kpp_config
    for step in range(STEPS):
        h, _, _ = x.step()
        flags = x.kpp_flags[step]
        valid = flags["valid"][:n]
        assert np.array_equal(valid, x.c_range[:n].any(axis=1)) and valid.any()
        depth = _masked(x, h).sum(axis=1)
        assert np.all((cfg["VonKarman"] * cfg["SurfaceLayerFraction"] * depth * np.abs(bf))[valid] <= (0.2 * us**3)[valid])
        assert not flags["used_cbrt"][:n][valid].any() and not flags["marginal"][:n][valid].any()
        shape = (x.NonLocalShape[:n] > 0.0).any(axis=1)
        assert (valid & (bf < 0.0) & shape).any() and (valid & (bf >= 0.0)).any() and not (shape & (bf >= 0.0)).any()
        kb = x.BoundaryLayerIndex[:n].astype(np.int64)
        deep = valid & (hi - lo + 1 >= 3)
        inside_column, to_the_bottom = deep & (lo < kb) & (kb <= hi), deep & (kb == hi + 1)
        print(f"{rung}, step {step + 1}: of {deep.sum()} columns of >= 3 layers the layer ends inside {inside_column.sum()} and "
              f"reaches the bottom of {to_the_bottom.sum()}; NonLocalShape > 0 in {(valid & shape).sum()} columns")
        assert 4 * inside_column.sum() >= deep.sum() and to_the_bottom.any()
        assert np.all(x.BoundaryLayerDepth[:n][valid] > 0.0)
        inside = flags["inside"][:n]
        assert inside.any() and np.all(flags["VertDiffAfter"][:n][inside] != flags["VertDiffBefore"][:n][inside])
    assert len(x.kpp_flags) == STEPS


def _remap_volume_roundings(x, h_new):
    """What VertRemap's computeTarget and adoptTarget add to the change of sum A h, in units of eps/2, first order.
    Exactly, sum_K Ref (1 + Coeff W / SumWh) = SumRef + Coeff = SumH.  In floating point, for a column of n layers with
    H, HRef the totals of |h| and |Ref|: SumH and SumRef round n - 1 times each at no more than H and HRef, so does
    Coeff = SumH - SumRef, once more at |Coeff|; SumWh takes n products and n - 1 additions, so the quotient
    (Coeff W) / SumWh carries 2 n + 1 relative roundings of a term whose sum over the column is |Coeff|; 1.0 + q and the
    product with Ref round once each at the target: (n - 1) (H + HRef) + (2 n + 2) |Coeff| + 2 HTarget."""
    n = x.nc
    count = x.c_range[:n].sum(axis=1)
    H, href, target = (np.abs(_masked(x, a)).sum(axis=1) for a in (x.lagrangian_h, x.ref, h_new))
    per_column = np.maximum(count - 1, 0) * (H + href) + (2 * count + 2) * np.abs(H - href) + 2.0 * target
    return float((x.area[:n] * per_column).sum())


@pytest.mark.parametrize("rung", NEW_RUNGS)
def test_total_volume_is_conserved_on_the_new_rungs(rung):
    """test_total_volume_is_conserved on every rung that attaches a Redi, a Kpp or a VertRemap: the same bound,
    eps/2 sum A (|hNew| + 12 D) -- Redi and Kpp move no thickness -- and with a VertRemap, where hNew is the Lagrangian
    thickness the remap starts from, the roundings of its target on top (_remap_volume_roundings).  The sum is over
    every level of every cell: the Tendencies know no layer ranges, so on the ragged rigs a level outside a cell's range
    trades volume with its neighbours like any other, and the sum over the ranges alone is not conserved.  The coast is
    closed (_closed_coast)."""
    x = ModelRig(rung, device=False, change=_closed_coast).host
    n, area = x.nc, x.area
    assert np.all(x.u[0][: x.ne][x.mask[: x.ne] == 0.0] == 0.0)
    before = _exact(area[:n], x.h[0][:n])
    for step in range(STEPS):
        h, u, _ = x.step()
        assert np.all(u[: x.ne][x.mask[: x.ne] == 0.0] == 0.0)
        after = _exact(area[:n], h[:n])
        moved = x.lagrangian_h if x.opt["remap"] is not None else h
        units = float((area[:n, None] * (np.abs(moved[:n]) + 12.0 * _transport_scale(x))).sum())
        if x.opt["remap"] is not None:
            units += _remap_volume_roundings(x, h)
        bound = EPS / 2 * units
        err = abs(float(after - before))
        print(f"{rung}, step {step + 1}: |change of sum A h| = {err:.3e} m^3 of {float(after):.3e}, bound {bound:.3e} "
              f"({err / bound:.3f})")
        assert err <= bound * (1.0 + 1.0e-6)
        assert not np.array_equal(h[:n], x.h[1][:n])
        before = after


@pytest.mark.parametrize("rung", NEW_RUNGS)
def test_total_tracer_content_is_conserved_on_the_new_rungs(rung):
    """test_total_tracer_content_is_conserved_without_surface_fluxes on every rung that attaches a Redi, a Kpp or a
    VertRemap, summed over every level of every cell with the coast closed (as the volume is, above), to the bound
    derived there and no other.  The terms the new objects add fit
    in it as they are: Redi's two explicit parts are flux-form (FluxE is formed alike by the two cells of an edge, WBot
    of a layer is WTop of the one below: Redi.h), its S.S part rides in the implicit solve; the Kpp's non-local term
    telescopes to NonLocalShape[KMin] = 0 and vanishes anyway with the surface flux; the remap integrates each source
    cell's parabola exactly over the target layers."""
    x = ModelRig(rung, device=False, change=_closed).host
    n, area, K = x.nc, x.area, x.K
    assert np.all(x.f["SurfaceTracerFlux"] == 0.0) and x.opt["mix"]
    levels = int(np.ceil(np.log2(K)))
    rng = x.c_range[:n]
    before = [_exact(area[:n], x.h[0][:n], x.tr[0][t, :n]) for t in range(x.nt)]
    for step in range(STEPS):
        old_tr, old_h = x.tr[0].copy(), x.h[0].copy()
        h, _, tr = x.step()
        D = _transport_scale(x)
        hs = [h[:n], old_h[:n]] + ([x.lagrangian_h[:n]] if x.opt["remap"] is not None else [])
        h_max, h_min = max(a.max() for a in hs), min(a.min() for a in hs)
        g_max = x.VertDiff[:n][rng].max() * x.dt_seconds / h_min
        for t in range(x.nt):
            p_max = max(np.abs(tr[t, :n]).max(), np.abs(old_tr[t, :n]).max())
            spread = old_tr[t, :n].max() - old_tr[t, :n].min()
            d_diff = x.dt * x.orc.c.EddyDiff2 * 6.0 * (x.dv[: x.ne] / x.dc[: x.ne]).max() * h_max * spread / area[:n].min()
            per = 4.0 * h_max * p_max + 16.0 * (p_max * D + d_diff) + (8 * levels + 6) * (h_max * (1.0 + 4.0 * g_max) * p_max + h_max * p_max)
            bound = EPS / 2 * float(area[:n].sum() * K * per)
            after = _exact(area[:n], h[:n], tr[t, :n])
            err = abs(float(after - before[t]))
            print(f"{rung}, step {step + 1}, tracer {t}: |change of sum A h phi| = {err:.3e} of {float(after):.3e}, "
                  f"bound {bound:.3e} ({err / bound:.3f})")
            assert err <= bound
            before[t] = after
        assert not np.array_equal(tr[:, :n], old_tr[:, :n])


def test_a_constant_tracer_stays_constant_through_redi_and_the_remap():
    """Temperature = 10 everywhere, no surface flux of it, on planar_hex(8, 8) with K = 5: PressureGrad, the 2-D
    MonotoneAdv at order 4, GentMcWilliams, Redi, the VertMixStep hook and the PPM VertRemap.  Two parts are exact.  Redi's
    term is built from differences of phi alone (GradPhi, PhiZ, GInt): every one is 0.0 and the tendency keeps its bits.
    The remap of a constant column has aL = aR = a and a6 = 0.0 in every cell, and whatever the quadrature rounds to, the
    final clamp to the range of the source cells, [a, a], returns a.  Both are shown on the rig's own arrays after the
    steps.  The rest is rounding: the advection as in
    test_a_constant_tracer_stays_constant_under_the_3d_limiter_and_the_bolus_flow, eps/2 (4 + 32 C) per step, and the
    implicit solve of step 9, M phi = h phi0 with a matrix that is diagonally dominant by rows with margin h (so
    |M^-1| <= 1 / hMin) and, as the content test has it, a residual of at most (8 L + 6) roundings of
    |A| |x| + |b| <= (h (1 + 4 G) + h) phi0: relative eps/2 (8 L + 6) (2 + 4 G) hMax / hMin per step."""
    from tests import redi_reference as RR
    from tests import vert_remap_reference as WR
    from tests.model_step_fixtures import CD, RA
    phi0 = 10.0

    def constant(g, G):
        G["tr"][0][:] = phi0
        G["SurfaceTracerFlux"][0][:] = 0.0

    spec = dict(mesh="planar8", K=5, opt=dict(pgrad=True, mono=(4, 0.25), gm=True, mix=True, cd=CD, ra=RA, wind=True, redi=True,
                                              remap=3))
    x = ModelRig(spec, device=False, change=constant).host
    n, K = x.nc, x.K
    levels = int(np.ceil(np.log2(K)))
    bound = 0.0
    for step in range(STEPS):
        h_old = x.h[0].copy()
        h, _, tr = x.step()
        h_min = min(h[:n].min(), h_old[:n].min(), x.lagrangian_h[:n].min())
        h_max = max(h[:n].max(), h_old[:n].max(), x.lagrangian_h[:n].max())
        c = _transport_scale(x) / h_min
        g_max = x.VertDiff[:n].max() * x.dt_seconds / h_min
        bound += EPS / 2 * ((4.0 + 32.0 * c) + (8 * levels + 6) * (2.0 + 4.0 * g_max) * h_max / h_min)
        dev = np.abs(tr[0, :n] / phi0 - 1.0).max()
        print(f"step {step + 1}: max |T / T0 - 1| = {dev:.3e}, bound {bound:.3e}, C = {c:.3e}, G = {g_max:.3e}")
        assert dev <= bound * (1.0 + 1.0e-6)
    assert np.abs(x.SlopeInterface[: x.ne]).max() > 0.0 and np.abs(x.VertDiffusivity[:n, 1:]).max() > 0.0
    assert not np.array_equal(x.h[0][:n], x.lagrangian_h[:n])
    assert not np.array_equal(tr[1, :n], x.start[2][1, :n])  # the salinity went through all of it
    # the two exact parts, on the arrays the last step left
    flat = np.full((1, x.nc_size, K), phi0)
    tend = np.full((1, x.nc_size, K), 0.375)
    RR.add_tracer_tend(tend, x.h[1], flat, 1, x.column["ZMid"], x.SlopeInterface, x.f["RediKappa"], x.redi_tables, x.lo, x.hi,
                       x.lo_e, x.hi_e)
    assert np.all(tend == 0.375)
    WR.remap_tracers(x.lagrangian_h, x.RemapTarget, flat, 1, x.lo, x.hi, n, 3)
    assert np.all(flat == phi0)


_BASE = {}


def _two_steps(rung, deviations=(), change=None):
    x = ModelRig(rung, device=False, deviations=deviations, change=change).host
    for _ in range(STEPS):
        x.step()
    return x


def _base(rung):
    if rung not in _BASE:
        x = _two_steps(rung)
        assert all(np.isfinite(a[0]).all() for a in (x.h, x.u, x.tr))
        _BASE[rung] = (x.h[0], x.u[0], x.tr[0], {name: np.array(getattr(x, name)) for name in ("TracerTend",)})
    return _BASE[rung]


# A mistake that only reorders a sum changes the last bit of a tendency, which the update it feeds mostly rounds away
# (Dt TracerTend is some 2^-15 of h phi on these rigs).  The GPU comparison sees the tendency itself; so does this test,
# for the mistakes named here and for no other.
ALSO_COMPARED = {"redi_before_mono": ("TracerTend",)}


@pytest.mark.parametrize("deviation", DEVIATIONS)
def test_a_deviation_changes_the_state_on_every_rig_it_is_used_with(deviation):
    """Two steps of the sequence with one mistake in it differ from two steps of the sequence in at least one bit of
    (h, u, tracers), on the rig of every rung of the GPU comparison that attaches what the mistake is about (for a
    mistake of ALSO_COMPARED: of the state or of the kept arrays named there, which the GPU comparison reads as well).

    btr_velocity_reset zeroes BtrVelocity between steps in both senses: between two time steps, which alone changes
    nothing on any rig -- step 2 of the sequence, splitVelocityAndSSH, writes BtrVelocity on every edge < NEdgesAll before
    anything reads it (test_no_barotropic_field_is_carried_between_steps_but_the_surface_of_dry_columns) -- and between
    steps 5 and 8 of the sequence, where advanceVelocity then adds 0 instead of the velocity the sub-cycle ended with."""
    rungs = [r for r in RUNGS if deviation in deviations_of(RUNGS[r]["opt"])]
    assert rungs
    blind = []
    for rung in rungs:
        got = _two_steps(rung, (deviation,))
        base = _base(rung)
        differs = [not np.array_equal(a[0], b) for a, b in zip((got.h, got.u, got.tr), base)]
        also = {name: not np.array_equal(getattr(got, name), base[3][name]) for name in ALSO_COMPARED.get(deviation, ())}
        print(f"{deviation} on {rung}: h, u, tracers differ: {differs} {also or ''}")
        differs += list(also.values())
        if not any(differs):
            blind.append(rung)
    assert not blind, f"{deviation} changes nothing on {blind}"


def test_every_deviation_is_used_on_some_rung():
    used = set()
    for spec in RUNGS.values():
        used |= set(deviations_of(spec["opt"]))
    assert used == set(DEVIATIONS)
    # all of the sequence up to the VertMixStep hook on the rung that attaches all of that ...
    assert set(deviations_of(RUNGS["G"]["opt"])) == set(DEVIATIONS[:9]) and DEVIATIONS[8] == "btr_velocity_reset"
    # ... and all of them on the two ragged rungs that attach everything between them (the VertRemap and the VertAdv
    # refuse each other)
    both = set(deviations_of(RUNGS["L_vertadv"]["opt"])) | set(deviations_of(RUNGS["L_remap"]["opt"]))
    assert both == set(DEVIATIONS) and len(DEVIATIONS) == 19


@pytest.mark.parametrize("rung", ["F", "G"])
def test_no_barotropic_field_is_carried_between_steps_but_the_surface_of_dry_columns(rung):
    """Every array of the BarotropicMode filled with other values before the first step: two steps end in the same bits,
    the arrays themselves included.  The one exception is SSH on a column that is dry by its layer range (rung G has
    some): computeSSH does not write it, the sub-cycle treats every cell of the mesh as wet (BarotropicMode.h) and
    advances it from what it held, so it is left at its starting value here, and changing it as well changes the
    result."""
    want = _two_steps(rung)
    rng = np.random.default_rng(3)

    def junk(x, dry_ssh):
        s = x.split
        for a in (s.vel, s.thick, s.forcing, s.flux, s.tend_mean, s.bcl):
            a[:] = rng.uniform(-1.0, 1.0, a.shape)
        wet = x.c_range.any(axis=1)
        s.ssh[wet | dry_ssh] = rng.uniform(-1.0, 1.0, int((wet | dry_ssh).sum()))
        return wet

    got = ModelRig(rung, device=False).host
    wet = junk(got, False)
    for _ in range(STEPS):
        got.step()
    for name in ("h", "u", "tr"):
        assert np.array_equal(getattr(got, name)[0], getattr(want, name)[0]), name
    ne = got.ne
    for name in ("BtrVelocity", "BtrThickEdge", "BtrForcing", "BtrFluxMean", "BtrTendMean", "SSH"):
        assert np.array_equal(got.btr(name)[:ne], want.btr(name)[:ne]), name
    assert np.array_equal(got.btr("BclVelocity")[got.e_range], want.btr("BclVelocity")[want.e_range])
    dry = ~wet[: got.nc]
    assert dry.any() == (rung == "G")
    if dry.any():
        other = ModelRig(rung, device=False).host
        junk(other, np.arange(other.nc_size) < other.nc)
        for _ in range(STEPS):
            other.step()
        assert not np.array_equal(other.u[0], want.u[0])


def test_the_empty_rung_is_the_oracle_fed_reference_step():
    """nothing attached, K = 1: the composition against split_explicit_reference.step fed by the oracle's three
    tendencies and the two updates of TimeStepper.cpp, written out here"""
    rig = ModelRig("A_K1", device=False)
    x = rig.host
    for _ in range(STEPS):
        x.step()
    got = (x.h[0].copy(), x.u[0].copy(), x.tr[0].copy(), x.split.ssh.copy(), x.split.vel.copy())
    m, orc, n = rig.mesh, rig.p.oracle, rig.nc
    s = SR.Split(btr_mesh(m, rig.bottom), rig.nc_size, rig.ne_size, 1)
    h, u, tr = rig.h.copy(), rig.u.copy(), rig.tr.copy()
    dt = O.coeff_seconds(1.0, DT)
    lo_e, hi_e = np.zeros(rig.ne_size, np.int32), np.zeros(rig.ne_size, np.int32)

    def thickness_and_tracers(u_tr):
        h_new, tr_new = h.copy(), tr.copy()
        h_new[:n] = h[:n] + dt * orc.compute_thickness_tendencies(h, u_tr)[:n]
        tr_new[:, :n] = (tr[:, :n] * h[:n] + dt * orc.compute_tracer_tendencies(h, u_tr, tr)[:, :n]) / h_new[:n]
        return h_new, tr_new

    for _ in range(STEPS):
        vel_tend = orc.compute_velocity_tendencies(h, u)
        u, (h, tr) = SR.step(s, h, u, vel_tend, dt, NSUB, rig.lo, rig.hi, lo_e, hi_e, GRAVITY, thickness_and_tracers)
    for name, a, b in zip(("h", "u", "tracers", "SSH", "BtrVelocity"), got, (h, u, tr, s.ssh, s.vel)):
        assert np.array_equal(a, b), name
    assert not np.array_equal(h, rig.h) and not np.array_equal(u, rig.u) and not np.array_equal(tr, rig.tr)
