"""The forced implicit solves, VertMixStep and the stepper hook on the GPU.  The velocity solve (wind stress, bottom
drag, Rayleigh drag) and the tracer solve (surface fluxes) equal tests/vert_mix_forcing_reference.py bit for bit at the
launch shapes the kernel branches on, on ragged columns and on NaN-seeded entries they must not touch; zero or absent
forcing gives the unforced bits; VertMixStep.apply equals its six calls made by hand; RK4 / RK2 / Forward-Backward with
the hook equal a step followed by apply; a stepper with neighbours is refused."""
import ctypes as C

import numpy as np
import pytest

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests import vert_fixtures as F
from tests import vert_mix_forcing_reference as FR
from tests import vert_mix_reference as R
from tests.meshes import named_mesh
from tests.problem import Problem
from tests.vert_fixtures import RHO0, Mix, same

pytestmark = pytest.mark.gpu

MESH = "fib300_coast_ragged"  # 251 cells, land, valence 5 / 6 / 7
DT = 1800.0
CD, RA = 2.5e-3, 1.0e-5
COLUMN_LIMIT = F.column_limit(F.FUSED | F.STAGE_SPEC_VOL_DISP)
VELOCITY_K = [1, 2, 3, 17, 64, 86, 129, 257, 1024]
TRACER_CASES = [(1, 1), (3, 3), (16, 37), (129, 6), (512, 6), (1024, 2)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    oa.device_init(0)


def _rig(K, nt=2, seed=11):
    """A Mix on ragged columns with VertVisc / VertDiff in place (from the column pass where it exists, else random),
    NaN on every entry the solves must not read"""
    x = Mix(named_mesh(MESH), K, "teos10", ntracers=max(nt, 2), ragged=True, column_pass=K <= COLUMN_LIMIT, seed=seed)
    if K <= COLUMN_LIMIT:
        x.compute()
        visc, diff = x.vm.get("VertVisc"), x.vm.get("VertDiff")
    else:
        visc, diff = np.random.default_rng(seed + K).uniform(1.0e-5, 1.0e-2, (2, x.n_size, K))
    k = np.arange(K)[None, :]
    ok = (x.lo >= 0) & (x.lo <= x.hi) & (x.hi < K)
    inside = ok[:, None] & (k > x.lo[:, None]) & (k <= x.hi[:, None])
    visc, diff = np.where(inside, visc, np.nan), np.where(inside, diff, np.nan)
    x.vm.set("VertVisc", visc)
    x.vm.set("VertDiff", diff)
    return x, visc, diff


def _edge_depths(lo, hi, n, K):
    return np.where((lo >= 0) & (lo <= hi) & (hi < K), hi - lo + 1, 0)[:n]


def _velocity_forcing(x, lo, hi):
    """stress on every edge (also those with an empty range), Ut NaN except at the bottom level of the owned edges
    with a range: the only entries the solve may read"""
    rng = np.random.default_rng(5)
    stress = rng.uniform(-0.2, 0.2, x.e_size)
    stress[stress == 0.0] = 0.1
    ut = np.full((x.e_size, x.K), np.nan)
    for e in range(x.e_own):
        if 0 <= lo[e] <= hi[e] < x.K:
            ut[e, hi[e]] = x.ut[e, hi[e]]
    return stress, ut, np.ascontiguousarray(x.mesh.get_array("EdgeMask")[:, 0])


def _velocity_case(K, cd, ra, wind):
    x, visc, _ = _rig(K)
    u0, u1, lo, hi = x.seeded_velocity()
    stress, ut, mask = _velocity_forcing(x, lo, hi)
    x.vm.apply_velocity(x.state.device_ptr(0, 0), x.state.device_ptr(1, 0), DT, boundary=(cd, ra),
                        stress=stress if wind else None, ut=ut if cd != 0.0 else None)
    oa.device_synchronize()
    want = FR.velocity_mix_forced(x.h, visc, u0, DT, x.mesh.get_array("CellsOnEdge"), lo, hi, x.e_own, cd=cd, ra=ra,
                                  stress=stress if wind else None, ut=ut, edge_mask=mask, rho0=RHO0)
    _, got0 = x.state.copy_to_host(0)
    _, got1 = x.state.copy_to_host(1)
    same(got0, want, "normal velocity (level 0)")
    same(got1, u1, "normal velocity (level 1)")
    n = _edge_depths(lo, hi, x.e_own, K)
    assert (n == 0).any() and np.all(stress[: x.e_own][n == 0] != 0.0)  # empty ranges with a stress
    same(got0[: x.e_own][n == 0], u0[: x.e_own][n == 0], "edges with an empty range")
    plain = R.velocity_mix(x.h, visc, u0, DT, x.mesh.get_array("CellsOnEdge"), lo, hi, x.e_own)
    assert not np.array_equal(want, plain, equal_nan=True)  # the forcing changed something
    assert np.all(np.isfinite(want[: x.e_own][n > 0, :][~np.isnan(u0[: x.e_own][n > 0, :])]))


@pytest.mark.parametrize("K", VELOCITY_K)
def test_velocity_solve_all_terms_bit_exact(K):
    _velocity_case(K, CD, RA, True)


@pytest.mark.parametrize("cd,ra,wind", [(CD, 0.0, False), (0.0, RA, False), (0.0, 0.0, True)])
def test_velocity_solve_each_term_alone(cd, ra, wind):
    _velocity_case(17, cd, ra, wind)


def test_velocity_sweep_covers_the_edge_kinds():
    seen = set()
    for K in VELOCITY_K:
        x = Mix(named_mesh(MESH), K, "teos10", ragged=True, column_pass=False)
        lo, hi = x.vc.get("MinLayerEdgeBot"), x.vc.get("MaxLayerEdgeTop")
        n = _edge_depths(lo, hi, x.e_own, K)
        mask = x.mesh.get_array("EdgeMask")[: x.e_own, 0]
        seen |= {"n=1"} if (n == 1).any() else set()
        seen |= {"n>1"} if (n > 1).any() else set()
        seen |= {"empty"} if (n == 0).any() else set()
        seen |= {"mask0"} if (mask == 0.0).any() else set()
        seen |= {"mask1 with a range"} if ((mask == 1.0) & (n > 0)).any() else set()
        s = F.mix_launch(K, 1)
        seen |= {("sys", s["Sys"]), ("levels", s["Levels"])}
        seen |= {"pad lanes"} if s["PadLanes"] > 0 else set()
    assert {"n=1", "n>1", "empty", "mask0", "mask1 with a range", "pad lanes"} <= seen
    assert {("sys", 256), ("sys", 1), ("levels", 0), ("levels", 10)} <= seen


@pytest.mark.parametrize("K,nt", TRACER_CASES)
def test_tracer_solve_bit_exact(K, nt):
    x, _, diff = _rig(K, nt)
    t0, t1 = x.seeded_tracers()
    rng = np.random.default_rng(9)
    flux = rng.uniform(-1.0e-4, 1.0e-4, (nt, x.n_size))
    valid = np.zeros(x.n_size, bool)
    valid[: x.n_own] = ((x.lo >= 0) & (x.lo <= x.hi) & (x.hi < K))[: x.n_own]
    flux[:, ~valid] = np.nan  # land, halo and sentinel cells: not read
    assert (flux[:, valid] > 0).any() and (flux[:, valid] < 0).any()
    x.vm.apply_tracers(x.state.device_ptr(0, 0), x.tracers.device_ptr(0), nt, DT, surface_flux=flux)
    oa.device_synchronize()
    got = x.tracers.copy_to_host(0)
    want = FR.tracer_mix_forced(x.h, diff, t0, nt, DT, x.lo, x.hi, x.n_own, flux)
    same(got, want, "tracers (level 0)")
    same(x.tracers.copy_to_host(1), t1, "tracers (level 1)")
    assert not np.array_equal(want[:nt], R.tracer_mix(x.h, diff, t0, nt, DT, x.lo, x.hi, x.n_own)[:nt], equal_nan=True)
    s = F.mix_launch(K, nt)
    assert (s["Chunk"], s["Passes"] > 1) == {(1, 1): (1, False), (3, 3): (4, False), (16, 37): (8, True),
                                             (129, 6): (6, False), (512, 6): (6, False), (1024, 2): (2, False)}[(K, nt)]
    # every tracer against a separate PCR diffusion solve on the forced right-hand side
    for cols, lev, hcol, dcol in FR.tracer_columns(x.h, diff, x.lo, x.hi, x.n_own):
        c = cols[:, None]
        for t in range(nt):
            g, hh, xx = FR.tracer_system(hcol, dcol, t0[t][c, lev], flux[t][cols], DT)
            assert np.array_equal(got[t][c, lev], oa.tridiag_diff_solve(g, hh, xx, "pcr")), f"tracer {t}"


@pytest.mark.parametrize("K", [17, 1024])
def test_forced_calls_without_forcing_equal_the_unforced_calls(K):
    nt = 2
    x, _, _ = _rig(K, nt)
    L = oa.lib()
    hp, up, tp = x.state.device_ptr(0, 0), x.state.device_ptr(1, 0), x.tracers.device_ptr(0)
    vp = C.c_void_p

    def run(velocity, tracers):
        x.seeded_velocity()
        x.seeded_tracers()
        velocity()
        tracers()
        oa.device_synchronize()
        return x.state.copy_to_host(0)[1], x.tracers.copy_to_host(0)

    u_plain, t_plain = run(lambda: x.vm.apply_velocity(hp, up, DT), lambda: x.vm.apply_tracers(hp, tp, nt, DT))
    zeros_e, zeros_c = np.zeros(x.e_size), np.zeros((nt, x.n_size))
    forms = [
        (lambda: x.vm.apply_velocity(hp, up, DT, boundary=(0.0, 0.0)),
         lambda: oa._chk(L.omg_vertmix_apply_tracers_forced(x.vm.h, vp(hp), vp(tp), nt, C.c_double(DT), None, None))),
        (lambda: x.vm.apply_velocity(hp, up, DT, boundary=(0.0, 0.0), stress=zeros_e, ut=x.ut),
         lambda: x.vm.apply_tracers(hp, tp, nt, DT, surface_flux=zeros_c)),
    ]
    for velocity, tracers in forms:
        u, t = run(velocity, tracers)
        same(u, u_plain, "normal velocity")
        same(t, t_plain, "tracers")


STEP_NT = 3
STEP_ARRAYS = ("TangentialVelocity", "NormalStressEdge", "SurfaceTracerFlux", "SurfacePressure", "TidalPotential",
               "SelfAttractionLoading")


def _step_forcing(x, nt):
    rng = np.random.default_rng(21)
    return dict(NormalStressEdge=rng.uniform(-0.2, 0.2, x.e_size), SurfaceTracerFlux=rng.uniform(-1e-4, 1e-4, (nt, x.n_size)),
                SurfacePressure=rng.uniform(0.9e5, 1.1e5, x.n_size), TidalPotential=rng.uniform(-1.0, 1.0, x.n_size),
                SelfAttractionLoading=rng.uniform(-0.1, 0.1, x.n_size))


@pytest.mark.parametrize("eos_kind", ["teos10", "linear"])
@pytest.mark.parametrize("K", [3, 17, 64])
def test_vert_mix_step_equals_the_six_calls(K, eos_kind):
    nt = STEP_NT
    x = Mix(named_mesh(MESH), K, eos_kind, ntracers=nt, ragged=True)
    step = oa.VertMixStep(x.mesh, x.vm, x.vc, x.eos, nt)
    for name in STEP_ARRAYS:
        assert np.all(step.get(name) == 0.0), name  # zero at construction
    f = _step_forcing(x, nt)
    for name, v in f.items():  # the named-array triple
        step.set(name, v)
        same(step.get(name), v, name)
        assert step.device_ptr(name)
    with pytest.raises(oa.OmegaAmdError, match="no array named"):
        step.get("NoSuchArray")
    step.set_boundary(CD, RA, True)
    with pytest.raises(oa.OmegaAmdError, match="negative"):
        step.set_boundary(-1.0, 0.0, True)
    hp, up, tp = x.state.device_ptr(0, 0), x.state.device_ptr(1, 0), x.tracers.device_ptr(0)

    def reset():
        x.state.copy_to_device(x.h, x.un, 0)
        x.tracers.copy_to_device(x.tr, 0)
        for name in F.MIX_OUT:
            x.vm.set(name, np.full((x.n_size, K), np.nan))

    def results():
        oa.device_synchronize()
        out = {name: x.vm.get(name) for name in F.MIX_OUT}
        out.update({name: x.vc.get(name) for name in ("PressureMid", "ZMid", "GeopotentialMid")})
        out.update({name: x.eos.get(name) for name in F.EOS_OUT})
        out["u"], out["tr"] = x.state.copy_to_host(0)[1], x.tracers.copy_to_host(0)
        return out

    reset()
    x.vc.compute_column(x.state, x.tracers, x.eos, f["SurfacePressure"], f["TidalPotential"],
                        f["SelfAttractionLoading"], kdisp=1)
    x.vm.compute_bvf(x.eos)
    ut = oa.HorzOperators(x.mesh).tangential_recon(x.un)
    x.vm.compute(x.un, ut)
    x.vm.apply_tracers(hp, tp, nt, DT, surface_flux=f["SurfaceTracerFlux"])
    x.vm.apply_velocity(hp, up, DT, boundary=(CD, RA), stress=f["NormalStressEdge"], ut=ut)
    by_hand = results()
    reset()
    step.apply(hp, up, tp, DT)
    got = results()
    for name, want in by_hand.items():
        same(got[name], want, name)
    same(step.get("TangentialVelocity"), ut, "TangentialVelocity")
    assert not np.array_equal(got["u"], x.un) and not np.array_equal(got["tr"], x.tr)
    # the state form, and the wind-stress switch off
    step.set_boundary(CD, RA, False)
    reset()
    step.apply_state(x.state, x.tracers, DT)
    no_wind = results()
    same(no_wind["tr"], by_hand["tr"], "tracers (state form)")
    assert not np.array_equal(no_wind["u"], by_hand["u"])
    want_u = FR.velocity_mix_forced(x.h, no_wind["VertVisc"], x.un, DT, x.mesh.get_array("CellsOnEdge"),
                                    x.vc.get("MinLayerEdgeBot"), x.vc.get("MaxLayerEdgeTop"), x.e_own, cd=CD, ra=RA, ut=ut)
    same(no_wind["u"], want_u, "normal velocity (no wind stress)")


def test_vert_mix_step_refusals():
    x = Mix(named_mesh(MESH), COLUMN_LIMIT + 1, "teos10", column_pass=False)
    assert COLUMN_LIMIT == 1008
    with pytest.raises(oa.OmegaAmdError, match="1008"):
        oa.VertMixStep(x.mesh, x.vm, x.vc, x.eos, 2)
    y = Mix(named_mesh(MESH), 3, "teos10", column_pass=False)
    with pytest.raises(oa.OmegaAmdError, match="NTracers = 1"):
        oa.VertMixStep(y.mesh, y.vm, y.vc, y.eos, 1)
    with pytest.raises(oa.OmegaAmdError, match="VertMix is NULL"):
        oa.VertMixStep(y.mesh, None, y.vc, y.eos, 2)
    z = Mix(named_mesh(MESH), 3, "teos10", column_pass=False)
    with pytest.raises(oa.OmegaAmdError, match="another mesh"):
        oa.VertMixStep(y.mesh, z.vm, y.vc, y.eos, 2)
    w = Mix(named_mesh(MESH), 4, "teos10", column_pass=False)
    with pytest.raises(oa.OmegaAmdError, match="another mesh|layer count"):
        oa.VertMixStep(y.mesh, y.vm, y.vc, w.eos, 2)
    with pytest.raises(oa.OmegaAmdError, match="negative"):
        y.vm.apply_velocity(y.state.device_ptr(0, 0), y.state.device_ptr(1, 0), DT, boundary=(0.0, -1.0e-5))
    with pytest.raises(oa.OmegaAmdError, match="tangential velocity"):
        y.vm.apply_velocity(y.state.device_ptr(0, 0), y.state.device_ptr(1, 0), DT, boundary=(CD, 0.0))


# ---- steppers
STEP_K, STEP_DT = 6, 20.0
KINDS = ["RungeKutta4", "RungeKutta2", "Forward-Backward"]


class StepRig:
    """planar_hex(8, 8), 6 layers, temperature and salinity, PressureGrad and VertAdv attached, every forcing on"""

    def __init__(self, nparts=1):
        K, nt = STEP_K, 2
        p = self.p = Problem(planar_hex(8, 8, 30.0e3), K, nt, nparts=nparts, config=dict(SSHTendencyEnable=0),
                             oracle=False)
        m = p.mesh
        rng = np.random.default_rng(31)
        nc, ne = m.NCellsSize, m.NEdgesSize
        self.h = np.zeros((nc, K))
        self.h[: m.NCellsAll] = rng.uniform(8.0, 12.0, (m.NCellsAll, K))
        self.u = np.zeros((ne, K))
        self.u[: m.NEdgesAll] = rng.uniform(-0.05, 0.05, (m.NEdgesAll, K))
        self.tr = np.zeros((nt, nc, K))
        self.tr[0, : m.NCellsAll] = rng.uniform(2.0, 20.0, (m.NCellsAll, K))
        self.tr[1, : m.NCellsAll] = rng.uniform(33.0, 36.0, (m.NCellsAll, K))
        p.state.copy_to_device(self.h, self.u, 0)
        p.tracers.copy_to_device(self.tr, 0)
        self.vc = oa.VertCoord(m, K, RHO0, "Uniform", decomp=p.decomp)
        self.vc.set("RefLayerThickness", np.full((nc, K), 10.0))
        self.eos = oa.Eos(m, K, "teos10")
        self.pg = oa.PressureGrad(m, self.vc, self.eos)
        self.va = oa.VertAdv(m, self.vc, 2)
        p.tend.attach_vert_adv(self.va)
        p.tend.attach_pressure_grad(self.pg)
        self.vm = oa.VertMix(m, self.vc)
        self.step = oa.VertMixStep(m, self.vm, self.vc, self.eos, nt)
        self.step.set("NormalStressEdge", rng.uniform(-0.2, 0.2, ne))
        self.step.set("SurfaceTracerFlux", rng.uniform(-1.0e-4, 1.0e-4, (nt, nc)))
        self.step.set_boundary(CD, RA, True)

    def stepper(self, kind):
        p = self.p
        return oa.TimeStepper(kind, STEP_DT, p.tend, p.aux, p.mesh, p.halo, p.tracers)

    def result(self):
        oa.device_synchronize()
        h, u = self.p.state.copy_to_host(0)
        return h, u, self.p.tracers.copy_to_host(0)


@pytest.mark.parametrize("kind", KINDS)
def test_steppers_with_the_hook_equal_step_then_apply(kind):
    a = StepRig()
    st = a.stepper(kind)
    st.attach_vert_mix(a.step)
    st.do_step(a.p.state)
    oa.device_synchronize()
    before = oa.device_resource_count()
    st.do_step(a.p.state)
    oa.device_synchronize()
    assert oa.device_resource_count() == before  # a step creates no buffer, stream or event
    attached = a.result()

    b = StepRig()
    st = b.stepper(kind)
    for _ in range(2):
        st.do_step(b.p.state)
        b.step.apply_state(b.p.state, b.p.tracers, STEP_DT, 0, 0)
    by_hand = b.result()

    c = StepRig()
    st = c.stepper(kind)
    for _ in range(2):
        st.do_step(c.p.state)
    plain = c.result()

    d = StepRig()
    st = d.stepper(kind)
    st.attach_vert_mix(d.step)
    st.attach_vert_mix(None)
    for _ in range(2):
        st.do_step(d.p.state)
    detached = d.result()

    for name, x, y, z, w in zip(("h", "u", "tracers"), attached, by_hand, plain, detached):
        assert np.all(np.isfinite(x)), name
        same(x, y, f"{name}: attached against step + apply")
        same(w, z, f"{name}: detached against unattached")
    assert not np.array_equal(attached[1], plain[1]) and not np.array_equal(attached[2], plain[2])


def test_attach_refusals():
    a = StepRig()
    st = a.stepper("RungeKutta4")
    other = StepRig()
    with pytest.raises(oa.OmegaAmdError, match="another mesh or layer count"):
        st.attach_vert_mix(other.step)
    two = StepRig(nparts=2)
    assert two.p.halo is not None
    for kind in KINDS:
        with pytest.raises(oa.OmegaAmdError,
                           match="multi-rank mixing needs the halo of the new level before and after the solve"):
            two.stepper(kind).attach_vert_mix(two.step)
