"""SplitExplicitStepper and the three BarotropicMode calls under it on the GPU.  The calls equal the NumPy restatement
(tests/split_explicit_reference.py) bit for bit on NaN-seeded arrays; a step equals its nine calls made by hand; rest
stays rest; the sub-cycle's surface and the column sum of the new thickness agree to rounding; a standing gravity wave
is carried over one period at a step where RungeKutta4 blows up, with the forward-backward period of the sub-step; bad
arguments are refused."""
import numpy as np
import pytest

import omega_amd as oa
from tests import split_explicit_reference as SR
from tests.barotropic_fixtures import GRAVITY, closed_basin
from tests.column_reference import RHO0
from tests.meshes import named_mesh
from tests.split_explicit_fixtures import CallRig, StepRig, step_by_hand
from tests.vert_fixtures import same

pytestmark = pytest.mark.gpu

MESHES = ("hex24x20", "ico2", "fib700_coast_ragged")
LEVELS = (1, 3, 16, 17, 65)  # compact rows, odd pitch, whole lines, padded rows, more levels than a wavefront
EPS = np.finfo(np.float64).eps
STEP_DT = 20.0


@pytest.fixture(scope="module", autouse=True)
def _device():
    oa.device_init(0)


@pytest.mark.parametrize("K", LEVELS)
@pytest.mark.parametrize("mesh", MESHES)
def test_calls_bit_exact_on_nan_seeded_arrays(mesh, K):
    x = CallRig(named_mesh(mesh), K)
    n, ne = x.e_all, x.e_size
    h, u = np.where(x.active, x.h, np.nan), np.where(x.e_active, x.u, np.nan)
    t_in = np.where(x.e_active, x.tend, np.nan)  # what computeResidualForcing may read
    bh, bu, bt_in = x.dev(h), x.dev(u), x.dev(t_in)
    x.poison()
    x.bm.split_velocity(bh.ptr, bu.ptr)
    x.bm.set("SSH", x.ssh0), x.bm.set("BtrVelocity", x.vel0)  # every local cell and edge, land included: NaN beyond
    oa.device_synchronize()
    want = x.state()
    # computeResidualForcing: BtrTendMean and BtrForcing, nothing else
    x.bm.compute_residual_forcing(bh.ptr, bt_in.ptr)
    oa.device_synchronize()
    SR.compute_residual_forcing(x.M, h, t_in, x.lo_e, x.hi_e, x.ssh0, x.vel0, GRAVITY, want["BtrTendMean"], want["BtrForcing"])
    got = x.state()
    for name in want:
        same(got[name], want[name], f"{name} (computeResidualForcing)")
    same(bt_in.to_host(), x.padded(t_in), "VelTend handed in")
    assert np.isfinite(want["BtrForcing"][:n]).all() and np.isnan(want["BtrForcing"][n:]).all()
    shut = ~x.M.open
    same(want["BtrForcing"][:n][shut], want["BtrTendMean"][:n][shut], "BtrForcing = G on a shut edge")
    assert not np.array_equal(want["BtrForcing"][:n][~shut], want["BtrTendMean"][:n][~shut])
    assert shut.any() if "coast" in mesh else True
    # transportVelocity: uOld is NaN inside the ranges (not read there) and beyond NEdgesAll
    x.bm.set("BtrFluxMean", x.flux0)
    u_old = np.where(x.e_outside, x.u_old, np.nan)
    b_old, out = x.dev(u_old), x.dev(np.full((ne, K), np.nan))
    x.bm.transport_velocity(b_old.ptr, out.ptr)
    oa.device_synchronize()
    want["BtrFluxMean"] = x.flux0
    w = SR.transport_velocity(u_old, np.full((ne, K), np.nan), want["BclVelocity"][:, :K], x.flux0, want["BtrThickEdge"],
                              x.lo_e, x.hi_e, n)
    g = out.to_host()
    same(g, x.padded(w), "transportVelocity")  # rows >= NEdgesAll, the sentinel row and the padding stay NaN
    same(g[:, :K][x.e_outside], u_old[x.e_outside], "transportVelocity outside the ranges")
    assert np.isfinite(w[:n]).all() and x.e_outside.any() and x.e_active.any()
    same(b_old.to_host(), x.padded(u_old), "uOld handed in")
    # advanceVelocity: the tendency on every level of the local edges
    tend = np.where(np.arange(ne)[:, None] < n, x.tend, np.nan)
    b_t, out = x.dev(tend), x.dev(np.full((ne, K), np.nan))
    dt = 600.0
    x.bm.advance_velocity(b_old.ptr, b_t.ptr, dt, out.ptr)
    oa.device_synchronize()
    w = SR.advance_velocity(u_old, tend, dt, np.full((ne, K), np.nan), want["BclVelocity"][:, :K], want["BtrVelocity"],
                            want["BtrTendMean"], x.lo_e, x.hi_e, n)
    g = out.to_host()
    same(g, x.padded(w), "advanceVelocity")
    same(g[:, :K][x.e_outside], (u_old + dt * tend)[x.e_outside], "advanceVelocity outside the ranges")
    assert np.isfinite(w[:n]).all()
    same(b_old.to_host(), x.padded(u_old), "uOld handed in")
    same(b_t.to_host(), x.padded(tend), "VelTend handed in")
    # ... and with uOut = uOld
    x.bm.advance_velocity(b_old.ptr, b_t.ptr, dt, b_old.ptr)
    oa.device_synchronize()
    same(b_old.to_host(), g, "advanceVelocity in place")
    got = x.state()
    for name in want:  # the two level calls write nothing of the class
        same(got[name], want[name], f"{name} (after the level calls)")
    if "coast" in mesh:
        empty = ~x.e_active[:n].any(axis=1)
        assert empty.any() and (x.lo_e[:n][~empty] > 0).any() if K > 2 else empty.any()


def _compare_step_with_the_calls(a, b, nsub):
    st = a.stepper("Split-Explicit", STEP_DT, nsub)
    st.do_step(a.p.state)
    oa.device_synchronize()
    before = oa.device_resource_count()
    st.do_step(a.p.state)
    oa.device_synchronize()
    assert oa.device_resource_count() == before  # a step creates no buffer, stream or event
    assert st.time == 2 * STEP_DT
    for i in range(2):
        step_by_hand(b, STEP_DT, nsub, i * STEP_DT)
    for name, got, want, start in zip(("h", "u", "tracers"), a.result(), b.result(), (a.h, a.u, a.tr)):
        assert np.all(np.isfinite(got)), name
        same(got, want, f"{name}: the stepper against its calls by hand")
        assert not np.array_equal(got, start), name
    for name in ("SSH", "BtrVelocity", "BtrForcing", "BtrFluxMean", "BtrTendMean", "BclVelocity"):
        same(a.bm.get(name), b.bm.get(name), name)


@pytest.mark.parametrize("nsub", [1, 7])
def test_step_equals_its_calls_by_hand(nsub):
    _compare_step_with_the_calls(StepRig(), StepRig(), nsub)


def test_step_equals_its_calls_by_hand_nothing_attached_one_layer():
    _compare_step_with_the_calls(StepRig(K=1, attached=False), StepRig(K=1, attached=False), 3)


def test_the_reference_signature_of_do_step_and_a_stream():
    """do_step on a stream gives the bits of the null stream"""
    a, b = StepRig(), StepRig()
    s = oa.Stream()
    sa, sb = a.stepper("Split-Explicit", STEP_DT, 4), b.stepper("Split-Explicit", STEP_DT, 4)
    sa.do_step(a.p.state, stream=s)
    s.synchronize()
    sb.do_step(b.p.state)
    for name, got, want in zip(("h", "u", "tracers"), a.result(), b.result()):
        same(got, want, name)


def test_rest_stays_rest():
    K = 4
    x = StepRig(K=K, attached=False, g=closed_basin(10, 12, 30.0e3, 1.0e-4, 1000.0))
    m = x.p.mesh
    x.h[: m.NCellsAll], x.u[:] = 250.0, 0.0
    x.tr[:, : m.NCellsAll] = 1.0
    x.load()
    x.vc.set("BottomDepth", np.full(m.NCellsSize, 1000.0))
    st = x.stepper("Split-Explicit", 1200.0, 4)
    for _ in range(5):
        st.do_step(x.p.state)
    h, u, _ = x.result()
    assert np.all(u == 0.0)
    same(h, x.h, "h at rest")
    assert np.all(x.bm.get("BtrVelocity") == 0.0) and np.all(x.bm.get("SSH")[: m.NCellsAll] == 0.0)


def test_the_2d_and_3d_surfaces_agree():
    """After one step, computeSSH(h_new) against the SSH the sub-cycle ended with.  Exactly (no rounding) they are
    equal: the transporting velocity carries BtrFluxMean through the column (tests/test_split_explicit.py), the centred
    flux thickness of the 3-D thickness tendency is hE, so sum_K h_new = sum_K h - Dt Div(BtrFluxMean), which is what
    NSub sub-steps of DtBtr make of SSH.  Roundings, in units of eps/2 = 2^-53 times the column depth D = max sum_K h:
      3-D side: each h_new[K] = fl(h[K] + Dt*tend) rounds by eps/2 h_new[K], together eps/2 D (1); computeSSH's
        ascending sum K - 1 roundings of at most eps/2 D each; the same K - 1 in the SSH the sub-cycle started from;
      2-D side, per sub-step: the MaxEdges terms ((Dv F) InvA) of Div, three roundings each, times DtBtr, are each at
        most c D with c = DtBtr max(Dv/A) |BtrVelocity| -- c <= 1/3 is asserted below for |BtrVelocity| <= 1 m/s, twenty
        times the start -- so at most eps/2 D per term; and SSH - DtBtr*Div rounds by eps/2 |SSH| <= eps/2 D;
      the tendency's own roundings are c times smaller than the update's and the flux identity's eps/2 (5 K + 8) D U
        per edge enters through Dt Dv/A U <= c NSub: both are inside the slack of the 2-D count.
    Bound: (2 K - 1 + (MaxEdges + 1) NSub) D 2^-53."""
    K, nsub, dt, bottom = 5, 6, 240.0, 45.0
    x = StepRig(K=K, attached=False, config=dict(FluxThicknessUpwind=0))
    m = x.p.mesh
    x.vc.set("BottomDepth", np.full(m.NCellsSize, bottom))
    st = x.stepper("Split-Explicit", dt, nsub)
    st.do_step(x.p.state)
    h_new, _, _ = x.result()
    ssh_2d = x.bm.get("SSH")[: m.NCellsAll]
    x.bm.compute_ssh(x.p.state.device_ptr(0, 0))
    oa.device_synchronize()
    ssh_3d = x.bm.get("SSH")[: m.NCellsAll]
    depth = h_new[: m.NCellsAll].sum(axis=1).max()
    max_edges = m.get_array("EdgesOnCell").shape[1]
    c = dt / nsub * (m.get_array("DvEdge")[: m.NEdgesAll].max() / m.get_array("AreaCell")[: m.NCellsAll].min()) * 1.0
    assert c <= 1.0 / 3.0 and np.abs(x.u).max() <= 0.05
    bound = (2 * K - 1 + (max_edges + 1) * nsub) * depth * EPS / 2
    diff = np.abs(ssh_3d - ssh_2d).max()
    moved = np.abs(ssh_2d - (x.h[: m.NCellsAll].sum(axis=1) - bottom)).max()
    print(f"max |SSH(h_new) - SSH of the sub-cycle| = {diff:.3e} m, bound {bound:.3e} m; the surface moved by {moved:.3e} m")
    assert diff <= bound
    assert moved > 1.0e6 * bound  # a change the bound is small against


WAVE = dict(nx=8, ny=18, dc=30.0e3, depth=1000.0, amp=1.0e-3, K=3, dt_over_dc_c=4.0, nsub=16)


class WaveRig(StepRig):
    """The standing gravity wave of DESIGN.md section 4.6 in the smallest basin used here: 17 rows of 8 cells closed
    across y, f = 0, flat bottom 1000 m, K = 3 equal layers of one density (linear equation of state without thermal or
    haline terms, PressureGrad attached, no viscosity), the gravest discrete eigenvector at 1 mm"""

    def __init__(self):
        w = WAVE
        g = closed_basin(w["nx"], w["ny"], w["dc"], 0.0, w["depth"], walls="y")
        cfg = dict(SSHTendencyEnable=0, VelDiffTendencyEnable=0, VelHyperDiffTendencyEnable=0, FluxThicknessUpwind=0)
        K = w["K"]
        self.g = g
        super().__init__(K=K, attached=False, g=g, config=cfg)
        m = self.p.mesh
        self.eos = oa.Eos(m, K, "linear", drhodt=0.0, drhods=0.0, rhot0s0=RHO0)
        self.pg = oa.PressureGrad(m, self.vc, self.eos)
        self.p.tend.attach_pressure_grad(self.pg)
        self.vc.set("BottomDepth", np.full(m.NCellsSize, w["depth"]))
        self.vc.set("RefLayerThickness", np.full((m.NCellsSize, K), w["depth"] / K))
        n = m.NCellsAll
        y = m.get_array("YCell")[:n]
        self.shape = np.cos(np.pi * (y - g["basin_y0"]) / g["basin_L"])
        self.h[:], self.u[:] = 0.0, 0.0
        self.h[:n] = ((w["depth"] + w["amp"] * self.shape) / K)[:, None]
        self.tr[0, :n], self.tr[1, :n] = 10.0, 35.0
        self.load()
        self.c = np.sqrt(GRAVITY * w["depth"])
        self.dt = w["dt_over_dc_c"] * w["dc"] / self.c
        k, dy = np.pi / g["basin_L"], g["basin_dy"]
        self.w_h = 2.0 * self.c / dy * np.sin(0.5 * k * dy)

    def amplitude(self):
        oa.device_synchronize()
        h = self.p.state.copy_to_host(0)[0][: self.p.mesh.NCellsAll]
        return h, float(self.shape @ (h.sum(axis=1) - WAVE["depth"]))


def test_the_long_step_carries_the_standing_gravity_wave():
    """Dt = 4 dc/sqrt(gH) (1212 s on the 30 km mesh; the explicit limit of RungeKutta4 for the mesh's fastest gravity
    mode, omega_max = sqrt(6) c/dc, is 2.83/sqrt(6) = 1.15 dc/c) and NSub = 16, so sqrt(gH) DtBtr/dc = 0.25.  Over one
    wave period (8 steps):
      - RungeKutta4 on the same rig goes non-finite or grows the surface tenfold: the condition of this test's Dt;
      - Split-Explicit keeps the projected amplitude within the forward-backward scheme's neutral bound.  From rest the
        sub-step recursion A[n+1] - 2 A[n] + A[n-1] = -x^2 A[n], x = omega_h DtBtr, has A[1] = A[0], so A[n] = A0 (cos
        n th + tan(th/2) sin n th) with sin(th/2) = x/2: |A[n]| <= A0 / cos(th/2) = A0 / sqrt(1 - x^2/4);
      - its period is the forward-backward T_h (x/2)/asin(x/2) of section 4.6 with x at DtBtr, not at Dt.
    Margins: the sub-cycle of a step starts from the surface and the barotropic velocity the last one ended with, up to
    rounding, so the linear problem has the sub-step's period exactly; what is left is nonlinear -- the flux thickness
    H + eta, the kinetic-energy gradient -- and enters at most at first order in amplitude/depth = 1e-6, which is the
    margin taken for both the amplitude and the period.  The rounding of a 333 m thickness (6e-14 m) against the 1 mm
    signal is 1e-10 per step and sits inside it.  The period is read from the phase step of the long-step samples by
    least squares: cos(Th) = sum A[n](A[n+1] + A[n-1]) / (2 sum A[n]^2), Th = 2 pi Dt/T < pi.
    Measured on an MI355X: see DESIGN.md section 4.7."""
    w = WAVE
    x = WaveRig()
    x_sub = x.w_h * x.dt / w["nsub"]
    assert x.c * (x.dt / w["nsub"]) / w["dc"] <= 0.25
    t_fb = 2.0 * np.pi / x.w_h * (x_sub / 2.0) / np.arcsin(x_sub / 2.0)
    nsteps = int(np.ceil(t_fb / x.dt))
    a0 = x.amplitude()[1]
    # RungeKutta4 at this step
    rk = x.stepper("RungeKutta4", x.dt)
    worst = 0.0
    for _ in range(nsteps):
        rk.do_step(x.p.state)
        h, _ = x.amplitude()
        worst = np.abs(h.sum(axis=1) - w["depth"]).max() if np.isfinite(h).all() else np.inf
        if worst >= 10.0 * w["amp"]:
            break
    print(f"RungeKutta4 at Dt = {x.dt:.1f} s: max |SSH| = {worst:.3e} m after at most {nsteps} steps")
    assert worst >= 10.0 * w["amp"]
    # Split-Explicit, from the same start
    x = WaveRig()
    se = x.stepper("Split-Explicit", x.dt, w["nsub"])
    amps = [a0]
    for _ in range(nsteps + 1):
        se.do_step(x.p.state)
        h, a = x.amplitude()
        assert np.isfinite(h).all()
        amps.append(a)
    a = np.array(amps)
    margin = w["amp"] / w["depth"]
    neutral = 1.0 / np.sqrt(1.0 - x_sub ** 2 / 4.0)
    growth = np.abs(a).max() / abs(a0)
    cos_th = float(np.sum(a[1:-1] * (a[2:] + a[:-2])) / (2.0 * np.sum(a[1:-1] ** 2)))
    period = 2.0 * np.pi * x.dt / np.arccos(cos_th)
    print(f"Split-Explicit at Dt = {x.dt:.1f} s, NSub = {w['nsub']}, x = {x_sub:.5f}: max |A|/A0 = {growth:.9f} "
          f"(neutral bound {neutral:.9f}); period {period:.4f} s against T_fb = {t_fb:.4f} s: (T - T_fb)/T_fb = "
          f"{(period - t_fb) / t_fb:+.3e} (margin {margin:.1e})")
    assert growth <= neutral * (1.0 + margin)
    assert a.min() < -0.9 * abs(a0)  # the wave went through its other extreme: a period was covered
    assert abs(period - t_fb) / t_fb <= margin


def test_refusals():
    a = StepRig()
    st = a.stepper("Split-Explicit", STEP_DT)
    with pytest.raises(oa.OmegaAmdError, match="no BarotropicMode is attached"):
        st.do_step(a.p.state)
    with pytest.raises(oa.OmegaAmdError, match="NSub = 0"):
        st.attach_barotropic(a.bm, 0)
    with pytest.raises(oa.OmegaAmdError, match="BarotropicMode is NULL"):
        st.attach_barotropic(None, 2)
    other = StepRig()
    with pytest.raises(oa.OmegaAmdError, match="another mesh or layer count"):
        st.attach_barotropic(other.bm, 2)
    m = a.p.mesh
    vc5 = oa.VertCoord(oa.HorzMesh(a.p.decomp, 5), 5, RHO0, "Uniform", decomp=a.p.decomp)
    with pytest.raises(oa.OmegaAmdError, match="another mesh or layer count"):
        st.attach_barotropic(oa.BarotropicMode(vc5.mesh, vc5), 2)
    two = StepRig(nparts=2)
    assert two.p.halo is not None
    with pytest.raises(oa.OmegaAmdError, match="more sub-steps than the halo is wide need an exchange per sub-step"):
        two.stepper("Split-Explicit", STEP_DT).attach_barotropic(two.bm, 2)
    with pytest.raises(oa.OmegaAmdError, match="not a Split-Explicit one"):
        a.stepper("RungeKutta4", STEP_DT).attach_barotropic(a.bm, 2)
    u = a.p.state.device_ptr(1, 0)
    for dt in (0.0, float("nan"), -1.0):
        with pytest.raises(oa.OmegaAmdError, match="advanceVelocity: Dt"):
            a.bm.advance_velocity(u, a.p.tend.device_ptr(1)[0], dt, a.p.state.device_ptr(1, 1))
    st.attach_barotropic(a.bm, 2)  # and the refused calls left the stepper usable
    st.do_step(a.p.state)
    assert all(np.isfinite(r).all() for r in a.result())
