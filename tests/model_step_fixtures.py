"""One rig, two sides (tests/test_model_step.py on the host, tests/test_model_step_gpu.py on a device): from one set of
host arrays, the all-host step of tests/model_step_reference.py and -- with `device` -- the product's objects with the
same things attached.  RUNGS is the ladder of configurations: each rung adds one object to the one before.

The inputs make every term of the step do something: a random BottomDepth close to the column's depth (so the surface
is uneven by decimetres), SurfacePressure, TidalPotential and SelfAttractionLoading, equal on the PressureGrad, the
GentMcWilliams and the VertMixStep as SplitExplicitStepper.h requires, temperature falling and salinity rising with
depth under noise, a per-edge Kappa with zeros in it, wind stress, bottom and Rayleigh drag and surface tracer fluxes.
Wind forcing in the Tendencies stays off (its cos / sin is the one documented departure from the host's libm); the
stress enters through VertMixStep.NormalStressEdge.

Every slot a step does not fully overwrite holds a known finite value, the same on both sides: the second time level
(SEED_*), the column fields (column_seed), and on the device the row padding of the state arrays (PAD)."""
import numpy as np

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests import column_reference as CR
from tests import model_step_reference as HM
from tests import monotone_adv_reference as MR
from tests.column_reference import RHO0
from tests.meshes import named_mesh
from tests.problem import Problem
from tests.rank_rig import raw
from tests.vert_fixtures import mix_inputs

NT, NSUB, DT = 2, 3, 20.0
PAD = -3.25
CD, RA = 2.5e-3, 1.0e-5

_PG = dict(pgrad=True, vert_adv=2)
_3D = dict(_PG, mono_3d=True, tracer_term=False)
_F = dict(_3D, mono=(4, 0.25), gm=True, mix=True, cd=CD, ra=RA, wind=True)
RUNGS = {
    "A_K1": dict(mesh="planar8", K=1, opt={}),
    "A_K5": dict(mesh="planar8", K=5, opt={}),
    "B": dict(mesh="planar8", K=5, opt=_PG),
    "C": dict(mesh="planar8", K=5, opt=dict(_PG, mono=(2, 0.25))),
    "D_order4": dict(mesh="planar8", K=5, opt=dict(_3D, mono=(4, 0.25))),
    "D_order3": dict(mesh="planar8", K=5, opt=dict(_3D, mono=(3, 0.25))),
    "E": dict(mesh="planar8", K=5, opt=dict(_3D, mono=(4, 0.25), gm=True)),
    "F": dict(mesh="planar8", K=5, opt=_F),
    "F_hex_centred": dict(mesh="hex24x20", K=17, opt=_F),
    "F_hex_upwind": dict(mesh="hex24x20", K=17, opt=dict(_F, upwind=True)),
    "F_hex_switches_off": dict(mesh="hex24x20", K=17, opt=_F, switches=False),
    "F_hex_linear_eos": dict(mesh="hex24x20", K=17, opt=dict(_F, eos="linear")),
    "G": dict(mesh="fib300_coast_ragged", K=6, opt=_F, ragged=True),
}


def deviations_of(opt):
    """the deviations of tests/model_step_reference.py that a configuration can show: those of the objects it attaches"""
    o = HM.options(**opt)
    out = ["tracers_divided_by_h_cur", "btr_velocity_reset"]
    if o["vert_adv"] is not None:
        out.append("transport_from_step_1")
    if o["vert_adv"] is not None and o["pgrad"]:
        out.append("pressure_grad_first")
    if o["mono"] is not None:
        out += ["mono_reads_u_cur", "mono_reads_h_cur_as_new"]
    if o["gm"]:
        out += ["gm_reads_h_next", "bolus_left_in_velocity"]
    if o["mix"]:
        out.append("mix_on_the_old_level")
    return out


def mesh_of(name):
    return planar_hex(8, 8, 30.0e3) if name == "planar8" else named_mesh(name)


def global_inputs(g, K, ragged, seed=41):
    """Global arrays: layer ranges (1-based, None: full columns), h, un, T and S, BottomDepth, RefLayerThickness, and
    the forcing"""
    nc, ne = int(g["nCells"]), int(g["nEdges"])
    rng = np.random.default_rng(seed)
    if ragged:
        G = mix_inputs(g, K, 7, False, NT)
        mn, mx, h, un = G["min_level"], G["max_level"], G["h"], G["un"]
    else:
        mn = mx = None
        h, un = rng.uniform(8.0, 12.0, (nc, K)), rng.uniform(-0.05, 0.05, (ne, K))
    k = np.arange(K)[None, :]
    inside = np.ones((nc, K), bool) if mn is None else (k >= mn[:, None] - 1) & (k <= mx[:, None] - 1)
    z = (np.cumsum(h, axis=1) - 0.5 * h) / h.sum(axis=1)[:, None]  # depth of the layer's middle as a fraction
    temp = 20.0 - 15.0 * z + rng.uniform(-0.5, 0.5, (nc, K))
    salt = 34.0 + 1.5 * z + rng.uniform(-0.1, 0.1, (nc, K))
    bottom = np.where(inside, h, 0.0).sum(axis=1) + rng.uniform(-0.3, 0.3, nc)
    bottom[~inside.any(axis=1)] = 100.0  # land
    kappa = rng.uniform(100.0, 900.0, ne)
    kappa[::7] = 0.0
    return dict(min_level=mn, max_level=mx, h=h, un=un, tr=np.stack([temp, salt]), bottom=bottom,
                ref=h * rng.uniform(0.9, 1.1, (nc, K)),
                SurfacePressure=rng.uniform(0.9e5, 1.1e5, nc), TidalPotential=rng.uniform(-1.0, 1.0, nc),
                SelfAttractionLoading=rng.uniform(-0.1, 0.1, nc), Kappa=kappa,
                NormalStressEdge=rng.uniform(-0.2, 0.2, ne), SurfaceTracerFlux=rng.uniform(-1.0e-4, 1.0e-4, (NT, nc)))


def column_seed(n_size, K):
    """finite, plausible values for every column field (the equation of state is evaluated on them outside the ranges)"""
    r, k = np.arange(n_size, dtype=np.float64)[:, None], np.arange(K + 1, dtype=np.float64)[None, :]
    pint, zint = 1.0e5 + 1.0e3 * k + 0.5 * r, -10.0 * k - 1.0e-3 * r
    return {"PressureInterface": pint, "PressureMid": pint[:, :K] + 500.0, "ZInterface": zint, "ZMid": zint[:, :K] - 5.0,
            "GeopotentialMid": 9.8 * (zint[:, :K] - 5.0), "SpecVol": 9.7e-4 + 1.0e-8 * k[:, :K] + 0.0 * r,
            "SpecVolDisplaced": 9.7e-4 + 2.0e-8 * k[:, :K] + 0.0 * r, "LayerThicknessTarget": 5.0 + k[:, :K] + 0.0 * r}


class ModelRig:
    """`host`: the HostModel; with `device` the product's objects (p, vc, eos, pg, va, bm, mono, gm, vm, mix, stepper)"""

    def __init__(self, rung, device, deviations=(), change=None, config=None):
        spec = RUNGS[rung] if isinstance(rung, str) else rung
        self.K = K = spec["K"]
        self.opt = o = HM.options(**spec["opt"])
        g = dict(mesh_of(spec["mesh"]))
        G = global_inputs(g, K, spec.get("ragged", False))
        if change is not None:
            change(g, G)
        g["bottomDepth"] = G["bottom"]  # the mesh's BottomDepth: the Tendencies', the VertCoord's and the oracle's
        self.g, self.G = g, G
        attached = o["pgrad"]
        cfg = dict(SSHTendencyEnable=0 if attached else 1, TracerHorzAdvTendencyEnable=0 if o["mono"] is not None else 1,
                   FluxThicknessUpwind=int(o["upwind"]))
        cfg.update(config or {})
        assert not cfg.get("WindForcingTendencyEnable", 0)
        p = self.p = Problem(g, K, NT, device=device, config=cfg, oracle=True)
        m = self.mesh = p.mesh
        self.nc, self.ne, self.nc_size, self.ne_size = m.NCellsAll, m.NEdgesAll, m.NCellsSize, m.NEdgesSize
        crow, erow = p.cell_id[: self.nc] - 1, p.edge_id[: self.ne] - 1

        def cells(x):
            if x.ndim == 1:
                out = np.zeros(self.nc_size)
                out[: self.nc] = x[crow]
                return out
            out = np.zeros(x.shape[:-2] + (self.nc_size, x.shape[-1]))
            out[..., : self.nc, :] = x[..., crow, :]
            return out

        def edges(x):
            out = np.zeros((self.ne_size,) + x.shape[1:])
            out[: self.ne] = x[erow]
            return out

        self.h, self.u, self.tr = cells(G["h"]), edges(G["un"]), cells(G["tr"])
        # the second level: what a step must overwrite (or leave) -- finite and plausible, zero on the sentinel rows
        self.h1, self.u1, self.tr1 = cells(G["h"] * 1.02 + 0.05), edges(0.5 * G["un"] + 1.0e-3), cells(G["tr"] + 0.25)
        self.bottom, self.ref = cells(G["bottom"]), cells(G["ref"])
        self.forcing = {n: cells(G[n]) for n in ("SurfacePressure", "TidalPotential", "SelfAttractionLoading")}
        self.forcing.update(Kappa=edges(G["Kappa"]), NormalStressEdge=edges(G["NormalStressEdge"]),
                            SurfaceTracerFlux=np.stack([cells(f) for f in G["SurfaceTracerFlux"]]))
        self.lo, self.hi = CR.local_layer_ranges(p.cell_id, G["min_level"], G["max_level"], self.nc, self.nc_size, K)
        self.column0 = column_seed(self.nc_size, K)
        assert np.array_equal(m.get_array("BottomDepth"), self.bottom)
        self.host = HM.HostModel(m, g, p.oracle, K, NT, (self.h, self.h1), (self.u, self.u1), (self.tr, self.tr1), self.lo,
                                 self.hi, self.bottom, self.ref, self.forcing, self.column0, o, DT, NSUB, deviations)
        self.has_column = o["pgrad"] or o["gm"] or o["mix"]
        if device:
            self._device(spec, G)

    # ---- the product's side
    def padded(self, a):
        out = np.full(a.shape[:-1] + (oa.level_pitch(self.K),), PAD)
        out[..., : self.K] = a
        return out

    def _device(self, spec, G):
        p, m, K, o = self.p, self.mesh, self.K, self.opt
        for level, (h, u, tr) in enumerate(((self.h, self.u, self.tr), (self.h1, self.u1, self.tr1))):
            oa.copy_to_device(p.state.device_ptr(0, level), self.padded(h))
            oa.copy_to_device(p.state.device_ptr(1, level), self.padded(u))
            oa.copy_to_device(p.tracers.device_ptr(level), self.padded(tr))
        self.vc = vc = oa.VertCoord(m, K, RHO0, "Uniform", G["min_level"], G["max_level"], decomp=p.decomp)
        vc.set("RefLayerThickness", self.ref)
        assert np.array_equal(vc.get("BottomDepth"), self.bottom)
        assert np.array_equal(vc.get("MinLayerCell"), self.lo) and np.array_equal(vc.get("MaxLayerCell"), self.hi)
        n = self.ne
        assert np.array_equal(vc.get("MinLayerEdgeBot")[:n], self.host.lo_e[:n])
        assert np.array_equal(vc.get("MaxLayerEdgeTop")[:n], self.host.hi_e[:n])
        for name in ("PressureInterface", "PressureMid", "ZInterface", "ZMid", "GeopotentialMid", "LayerThicknessTarget"):
            vc.set(name, self.column0[name])
        self.eos = self.pg = self.va = self.mono = self.gm = self.vm = self.mix = None
        if self.has_column:
            self.eos = oa.Eos(m, K, o["eos"])
            for name in ("SpecVol", "SpecVolDisplaced"):
                self.eos.set(name, self.column0[name])
        column_forcing = ("SurfacePressure", "TidalPotential", "SelfAttractionLoading")
        if o["vert_adv"] is not None:
            self.va = oa.VertAdv(m, vc, o["vert_adv"])
            self.va.set_tracer_term(o["tracer_term"])
            p.tend.attach_vert_adv(self.va)
        if o["pgrad"]:
            self.pg = oa.PressureGrad(m, vc, self.eos)
            for name in column_forcing:
                self.pg.set(name, self.forcing[name])
            p.tend.attach_pressure_grad(self.pg)
        self.bm = oa.BarotropicMode(m, vc)
        st = self.stepper = oa.TimeStepper("Split-Explicit", DT, p.tend, p.aux, m, p.halo, p.tracers)
        st.attach_barotropic(self.bm, NSUB)
        if not spec.get("switches", True):
            st.set_fused_transport(False)
            st.set_momentum_rhs(False)
            st.set_folded_updates(False)
        if o["mono"] is not None:
            self.mono = oa.MonotoneAdv(m, K, NT, flux_thickness_upwind=o["upwind"])
            if o["mono_3d"]:
                self.mono.attach_vert_adv(self.va)
            order, coef = o["mono"]
            if order != 2:
                self.mono.set_horz_order(order, coef, **MR.geometry(self.g))
            st.attach_monotone_adv(self.mono)
        if o["gm"]:
            self.gm = oa.GentMcWilliams(m, vc, self.eos, grav_wave_speed=o["gm_speed"])
            for name in column_forcing + ("Kappa",):
                self.gm.set(name, self.forcing[name])
            st.attach_gent_mcwilliams(self.gm)
        if o["mix"]:
            self.vm = oa.VertMix(m, vc, **(o["mix_config"] or {}))
            self.mix = oa.VertMixStep(m, self.vm, vc, self.eos, NT)
            for name in column_forcing + ("NormalStressEdge", "SurfaceTracerFlux"):
                self.mix.set(name, self.forcing[name])
            self.mix.set_boundary(o["cd"], o["ra"], o["wind"])
            st.attach_vert_mix(self.mix)

    def raw_state(self, level):
        """(h, u, tracers) of a time level as the device holds them, row padding included"""
        p, P = self.p, oa.level_pitch(self.K)
        return (raw(p.state.device_ptr(0, level), (self.nc_size, P)), raw(p.state.device_ptr(1, level), (self.ne_size, P)),
                raw(p.tracers.device_ptr(level), (NT, self.nc_size, P)))

    def device_array(self, name):
        """a named array of the product after a step, as the HostModel attribute of that name is laid out"""
        p = self.p
        if name in ("LayerThicknessTend", "NormalVelocityTend", "TracerTend"):
            return p.tend.get(("LayerThicknessTend", "NormalVelocityTend", "TracerTend").index(name))
        if name in HM.BTR_FIELDS:
            return self.bm.get(name)
        if name in ("BolusVelocity", "StreamFunction"):
            return self.gm.get(name)
        if name == "VerticalTransport":
            return self.va.get(name)
        if name in ("ScaleIn", "ScaleOut", "Hess"):
            return self.mono.get(name)
        if name in ("VertVisc", "VertDiff", "BruntVaisalaFreqSq"):
            return self.vm.get(name)
        if name == "TangentialVelocity":
            return self.mix.get(name)
        if name in ("SpecVol", "SpecVolDisplaced"):
            return self.eos.get(name)
        return self.vc.get(name)

    def host_array(self, name):
        x = self.host
        if name in HM.BTR_FIELDS:
            return x.btr(name)
        if name in HM.COLUMN_FIELDS:
            return x.column[name]
        if name == "LayerThicknessTarget":
            return self.column0[name]  # no call of a step names it
        return getattr(x, name)
