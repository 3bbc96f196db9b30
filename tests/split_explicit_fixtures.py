"""Shared by the split-explicit tests on a device (tests/test_split_explicit_gpu.py, tests/test_c_abi_split_explicit.py):
the NaN-seeded rig of the three new BarotropicMode calls, the rig of a step, and the nine steps of
SplitExplicitStepper::doStep issued one by one through the public Python calls."""
import numpy as np

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests.barotropic_fixtures import BtrRig
from tests.column_reference import RHO0
from tests.problem import Problem


class CallRig(BtrRig):
    """tests.barotropic_fixtures.BtrRig with the fields of the three new calls (its own draws) and BtrTendMean among
    the per-edge arrays"""

    EDGE_1D = BtrRig.EDGE_1D + ("BtrTendMean",)

    def __init__(self, g, K, seed=7):
        super().__init__(g, K, seed=seed)
        self.e_outside = np.zeros((self.e_size, K), bool)
        self.e_outside[: self.e_all] = ~self.e_active[: self.e_all]

    def draw(self, rng, nc, ne):
        K = self.K
        self.tend = self.edges(rng.uniform(-1.0e-5, 1.0e-5, (ne, K)), np.nan)
        self.u_old = self.edges(rng.uniform(-0.1, 0.1, (ne, K)), np.nan)
        self.bot, self.ssh0 = self.cells(rng.uniform(100.0, 6000.0, nc), np.nan), self.cells(rng.uniform(-0.5, 0.5, nc), np.nan)
        self.vel0, self.flux0 = self.edges(rng.uniform(-0.1, 0.1, ne), np.nan), self.edges(rng.uniform(-50.0, 50.0, ne), np.nan)


class StepRig:
    """planar_hex(8, 8, 30 km), K layers, temperature and salinity; `attached`: PressureGrad and VertAdv on the
    Tendencies with SSHTendencyEnable = 0, else nothing attached and the built-in surface-height gradient.  After
    tests/test_vert_mix_forcing_gpu.py's StepRig, with a BarotropicMode."""

    def __init__(self, K=6, attached=True, nparts=1, g=None, config=None):
        nt = 2
        cfg = dict(SSHTendencyEnable=0 if attached else 1)
        cfg.update(config or {})
        p = self.p = Problem(g if g is not None else planar_hex(8, 8, 30.0e3), K, nt, nparts=nparts, config=cfg, oracle=False)
        m, self.K, self.nt = p.mesh, K, nt
        rng = np.random.default_rng(31)
        nc, ne = m.NCellsSize, m.NEdgesSize
        self.h, self.u, self.tr = np.zeros((nc, K)), np.zeros((ne, K)), np.zeros((nt, nc, K))
        self.h[: m.NCellsAll] = rng.uniform(8.0, 12.0, (m.NCellsAll, K))
        self.u[: m.NEdgesAll] = rng.uniform(-0.05, 0.05, (m.NEdgesAll, K))
        self.tr[0, : m.NCellsAll] = rng.uniform(2.0, 20.0, (m.NCellsAll, K))
        self.tr[1, : m.NCellsAll] = rng.uniform(33.0, 36.0, (m.NCellsAll, K))
        self.load()
        self.vc = oa.VertCoord(m, K, RHO0, "Uniform", decomp=p.decomp)
        self.vc.set("RefLayerThickness", np.full((nc, K), 10.0))
        if attached:
            self.eos = oa.Eos(m, K, "teos10")
            self.pg = oa.PressureGrad(m, self.vc, self.eos)
            self.va = oa.VertAdv(m, self.vc, 2)
            p.tend.attach_vert_adv(self.va)
            p.tend.attach_pressure_grad(self.pg)
        self.bm = oa.BarotropicMode(m, self.vc)

    def load(self):
        self.p.state.copy_to_device(self.h, self.u, 0)
        self.p.tracers.copy_to_device(self.tr, 0)

    def stepper(self, kind, dt, nsub=None):
        p = self.p
        st = oa.TimeStepper(kind, dt, p.tend, p.aux, p.mesh, p.halo, p.tracers)
        if nsub is not None:
            st.attach_barotropic(self.bm, nsub)
        return st

    def result(self):
        oa.device_synchronize()
        h, u = self.p.state.copy_to_host(0)
        return h, u, self.p.tracers.copy_to_host(0)


def step_by_hand(x, dt_seconds, nsub, t0=0.0):
    """The nine steps of SplitExplicitStepper::doStep on the StepRig `x` through the public calls, on the null stream.
    The thickness update is update_by_tend on raw pointers; the tracer update is updateTracersByTend's formula
    (TimeStepper.cpp) in NumPy: Next = (Cur*hCur + Dt*TracerTend)/hNext on the cells < NCellsAll."""
    p, bm = x.p, x.bm
    m, K = p.mesh, x.K
    dt = oa.coeff_seconds(1.0, dt_seconds)
    st, tend = p.state, p.tend
    h_cur, u_cur, h_next, u_next = st.device_ptr(0, 0), st.device_ptr(1, 0), st.device_ptr(0, 1), st.device_ptr(1, 1)
    tend.set_time(t0)
    tend.compute_all_tendencies(st, p.aux, p.tracers, 0, 0, 0)                       # 1
    vel_tend = tend.device_ptr(1)[0]
    bm.split_velocity(h_cur, u_cur, with_ssh=True)                                   # 2
    bm.compute_residual_forcing(h_cur, vel_tend)                                     # 3
    bm.subcycle(nsub, dt / nsub)                                                     # 4
    bm.transport_velocity(u_cur, u_next)                                             # 5
    tend.compute_thickness_tendencies(st, p.aux, 0, 1)                               # 6
    oa.update_by_tend(h_next, h_cur, tend.device_ptr(0)[0], dt, m.NCellsAll, oa.level_pitch(K))
    tend.compute_tracer_tendencies(st, p.aux, p.tracers, 0, 0, 1)                    # 7
    oa.device_synchronize()
    cur, nxt = p.tracers.copy_to_host(0), p.tracers.copy_to_host(1)
    hc, hn = st.copy_to_host(0)[0], st.copy_to_host(1)[0]
    n = m.NCellsAll
    nxt[:, :n] = (cur[:, :n] * hc[:n] + dt * tend.get(2)[:, :n]) / hn[:n]
    p.tracers.copy_to_device(nxt, 1)
    bm.advance_velocity(u_cur, vel_tend, dt, u_next)                                 # 8
    st.update_time_levels()                                                          # 9
    p.tracers.update_time_levels()
    oa.device_synchronize()
