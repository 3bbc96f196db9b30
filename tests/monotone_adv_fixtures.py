"""Shared by the MonotoneAdv tests (CPU: tests/test_monotone_adv.py, GPU: tests/test_monotone_adv_gpu.py,
tests/test_c_abi_monotone_adv.py): one rank's mesh as the restatement reads it and the inputs of one forward step.

The inputs: h in 5 .. 30 m, u of both signs with some edges at u == 0.0 exactly (the tie of the upwind flux thickness),
Dt such that the largest outflow Courant number Dt*(sum of outflow)/(AreaCell*h) is 0.4, hNew from the same mass fluxes,
and three tracers: a 0/1 step, a uniform random field and a constant.  Rows >= NCellsAll / NEdgesAll (the sentinel
rows) hold NaN: nothing may read them.  The fixture asserts that its inputs exercise the limiter: on the random tracer at
least 20 % of the masked-in edge-levels are limited (Sc < 1) and at least 20 % are not (Sc == 1); the constant tracer
has no limited edge-level."""
import numpy as np

import omega_amd as oa
from tests import monotone_adv_reference as MR
from tests.meshes import named_mesh

COURANT = 0.4
STEP, RANDOM, CONST = 0, 1, 2
CONST_VALUE = 3.7


class Inputs:
    pass


class MonoRig:
    """One rank's mesh (host-only unless `device`) with the restatement's view of it"""

    def __init__(self, g, K, nparts=1, rank=0, device=False, halo=3):
        if isinstance(g, str):
            g = named_mesh(g)
        self.g, self.K = g, K
        self.decomp = oa.Decomp(oa.GlobalMesh(g), nparts, rank, halo)
        self.mesh = m = oa.HorzMesh(self.decomp, K, host_only=not device)
        self.nc, self.ne, self.nc_size, self.ne_size = m.NCellsAll, m.NEdgesAll, m.NCellsSize, m.NEdgesSize
        self.M = MR.MonoMesh.of(m)
        self.area = m.get_array("AreaCell")

    def inputs(self, seed=0, upwind=False, ntracers=3, check=True):
        """h_old, h_new [NCellsSize][K], u [NEdgesSize][K], tracers [ntracers][NCellsSize][K], dt.  The first three
        tracers are the step, the random field and the constant; further ones are random fields of other ranges."""
        rng = np.random.default_rng(seed)
        M, K, nc, ne = self.M, self.K, self.nc, self.ne
        I = Inputs()
        I.upwind = bool(upwind)
        I.h_old = np.full((self.nc_size, K), np.nan)
        I.h_old[:nc] = rng.uniform(5.0, 30.0, (nc, K))
        I.u = np.full((self.ne_size, K), np.nan)
        I.u[:ne] = rng.uniform(-1.0, 1.0, (ne, K))
        I.u[:ne][rng.random((ne, K)) < 0.05] = 0.0
        div, out = MR.mass_divergence(M, I.h_old, I.u, upwind)
        I.dt = float(COURANT / (out / I.h_old[:nc]).max())
        I.h_new = np.full((self.nc_size, K), np.nan)
        I.h_new[:nc] = I.h_old[:nc] + I.dt * div
        I.courant = I.dt * out / I.h_old[:nc]
        assert I.h_new[:nc].min() > 0.0 and abs(I.courant.max() - COURANT) < 1e-12
        I.tracers = np.full((ntracers, self.nc_size, K), np.nan)
        x = self.mesh.get_array("XCell")[:nc]
        I.tracers[STEP, :nc] = (x > np.median(x)).astype(float)[:, None]
        if ntracers > RANDOM:
            I.tracers[RANDOM, :nc] = rng.uniform(0.0, 1.0, (nc, K))
        if ntracers > CONST:
            I.tracers[CONST, :nc] = CONST_VALUE
        for L in range(3, ntracers):
            I.tracers[L, :nc] = rng.uniform(-1.0, 1.0, (nc, K)) * 10.0 ** (L % 4)
        if check and ntracers >= 3:
            self.check(I)
        return I

    def limited_fraction(self, I, L):
        si, so, _, _ = MR.scale_factors(self.M, I.h_old, I.h_new, I.u, I.tracers[L], I.dt, I.upwind)
        sc = MR.edge_limits(self.M, I.h_old, I.u, I.tracers[L], si, so, I.upwind)
        return float((sc < 1.0).mean()), float((sc == 1.0).mean())

    def check(self, I):
        lim, free = self.limited_fraction(I, RANDOM)
        assert lim >= 0.2 and free >= 0.2, (lim, free)
        assert self.limited_fraction(I, CONST) == (0.0, 1.0)

    def reference(self, I, ntracers, tend0=None, max_tracers=None):
        """(Tend, ScaleIn, ScaleOut) of the restatement, from tend0 (default zeros) and zero scale arrays"""
        nt = ntracers
        tend = np.zeros((nt, self.nc_size, self.K)) if tend0 is None else tend0.copy()
        si = np.zeros((max_tracers or nt, self.nc_size, self.K))
        so = np.zeros_like(si)
        MR.add_tracer_tend(self.M, tend, I.h_old, I.h_new, I.u, I.tracers, nt, I.dt, I.upwind, si, so)
        return tend, si, so
