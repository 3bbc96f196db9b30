"""One rig, two sides (tests/test_model_step.py on the host, tests/test_model_step_gpu.py on a device): from one set of
host arrays, the all-host step of tests/model_step_reference.py and -- with `device` -- the product's objects with the
same things attached.  RUNGS is the ladder of configurations: each rung up to G adds one object to the one before; H to L
attach the Redi, the Kpp and the VertRemap, alone and together.

The inputs make every term of the step do something: a random BottomDepth close to the column's depth (so the surface
is uneven by decimetres), SurfacePressure, TidalPotential and SelfAttractionLoading, equal on the PressureGrad, the
GentMcWilliams and the VertMixStep as SplitExplicitStepper.h requires, temperature falling and salinity rising with
depth under noise, a per-edge Kappa with zeros in it (and another for the Redi), wind stress, bottom and Rayleigh drag
and surface tracer fluxes.  The rungs with a Kpp replace the top of every column by a mixed layer of a depth drawn per
column -- so that the boundary layer ends inside some columns and reaches the bottom of others -- under a friction
velocity of a few cm/s and a surface buoyancy flux of either sign and at most 1e-7 m^2/s^3: with
kappa eps d |Bf| <= 0.2 us^3 over every column's depth no velocity scale takes a cbrt branch (Kpp.h), and the
restatement, whose cbrt is not the device's, stays bit for bit (tests/test_model_step.py checks that it is so).
Wind forcing in the Tendencies stays off (its cos / sin is the one documented departure from the host's libm); the
stress enters through VertMixStep.NormalStressEdge.

Every slot a step does not fully overwrite holds a known finite value, the same on both sides: the second time level
(SEED_*), the column fields (column_seed), the Redi's and the VertRemap's arrays (object_seeds), and on the device the
row padding of the state arrays (PAD)."""
import numpy as np

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests import column_reference as CR
from tests import kpp_reference as KR
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
_MIX = dict(mix=True, cd=CD, ra=RA, wind=True)
_J = dict(_MIX, pgrad=True, mono=(4, 0.25), gm=True)  # no VertAdv: the layers move with the flow until the remap
_K = dict(_J, redi=True, kpp=True, remap=3)
RUNGS.update({
    "H": dict(mesh="planar8", K=5, opt=dict(_F, redi=True)),
    "H_alone": dict(mesh="planar8", K=5, opt=dict(_MIX, pgrad=True, redi=True)),
    "I": dict(mesh="planar8", K=5, opt=dict(_F, kpp=True)),
    "I_redi": dict(mesh="planar8", K=5, opt=dict(_F, redi=True, kpp=True)),
    "J_ppm": dict(mesh="planar8", K=5, opt=dict(_J, remap=3)),
    "J_plm": dict(mesh="planar8", K=5, opt=dict(_J, remap=2)),
    "J_pcm": dict(mesh="planar8", K=5, opt=dict(_J, remap=1)),
    "K_hex": dict(mesh="hex24x20", K=17, opt=_K),
    "K_hex_switches_off": dict(mesh="hex24x20", K=17, opt=_K, switches=False),
    "K_hex_linear_eos": dict(mesh="hex24x20", K=17, opt=dict(_K, eos="linear")),
    # (a seed of its own: under the common one the deviation pressure_grad_first, a reordered sum whose last bit the
    # velocity update mostly rounds away, happened to leave no bit of the state changed on this rung)
    "L_vertadv": dict(mesh="fib300_coast_ragged", K=6, opt=dict(_F, redi=True, kpp=True), ragged=True, seed=42),
    "L_remap": dict(mesh="fib300_coast_ragged", K=6, opt=_K, ragged=True),
})
NEW_RUNGS = [r for r in RUNGS if r[0] in "HIJKL"]


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
    if o["redi"]:
        out += ["redi_slopes_of_the_new_level", "redi_diffusivity_from_new_slopes"]
    if o["redi"] and o["mono"] is not None:
        out.append("redi_before_mono")
    if o["redi"] and o["kpp"]:
        out.append("redi_diffusivity_before_kpp")
    if o["kpp"]:
        out += ["non_local_after_the_solve", "kpp_on_the_old_level"]
    if o["remap"] is not None:
        out += ["remap_target_from_h_cur", "remap_leaves_h", "remap_skips_velocity"]
    if o["remap"] is not None and o["mix"]:
        out.append("remap_after_mix")
    return out


def mesh_of(name):
    return planar_hex(8, 8, 30.0e3) if name == "planar8" else named_mesh(name)


def global_inputs(g, K, ragged, seed=41, mixed_layer=False):
    """Global arrays: layer ranges (1-based, None: full columns), h, un, T and S, BottomDepth, RefLayerThickness, and
    the forcing.  What the Redi and the Kpp read besides comes from a generator of its own, so that the other arrays
    are the same with and without them; mixed_layer: T and S of the layers down to a level drawn per column (anything
    from the top layer alone to the whole column) are those of the top layer under a noise of 1e-3 of the usual one."""
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
    own = np.random.default_rng(seed + 1000)
    redi_kappa = own.uniform(100.0, 900.0, ne)
    redi_kappa[3::5] = 0.0
    us, bf = own.uniform(0.02, 0.05, nc), own.uniform(-1.0e-7, 1.0e-7, nc)
    top = np.zeros(nc, np.int64) if mn is None else np.clip(mn.astype(np.int64) - 1, 0, K - 1)
    base = top + own.integers(0, K + 1, nc)  # the last level of the mixed layer; >= the column's last: all of it
    noise_t, noise_s = own.uniform(-5.0e-4, 5.0e-4, (nc, K)), own.uniform(-1.0e-4, 1.0e-4, (nc, K))
    if mixed_layer:
        rows = np.arange(nc)
        mixed = k <= base[:, None]
        temp = np.where(mixed, temp[rows, top][:, None] + noise_t, temp)
        salt = np.where(mixed, salt[rows, top][:, None] + noise_s, salt)
    return dict(min_level=mn, max_level=mx, h=h, un=un, tr=np.stack([temp, salt]), bottom=bottom,
                RediKappa=redi_kappa, FrictionVelocity=us, SurfaceBuoyancyFlux=bf,
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


def object_seeds(nc_size, ne_size, K):
    """what the arrays of the Redi and of the VertRemap hold where their contracts write nothing"""
    k = np.arange(K, dtype=np.float64)[None, :]
    return {"SlopeInterface": 2.5e-3 - 1.0e-4 * k + 0.0 * np.arange(ne_size)[:, None],
            "VertDiffusivity": 0.125 + 0.0625 * k + 0.0 * np.arange(nc_size)[:, None],
            "RemapTarget": 7.0 + k + 0.0 * np.arange(nc_size)[:, None]}


class ModelRig:
    """`host`: the HostModel; with `device` the product's objects (p, vc, eos, pg, va, bm, mono, gm, redi, vm, kpp, mix,
    remap, stepper)"""

    def __init__(self, rung, device, deviations=(), change=None, config=None):
        spec = RUNGS[rung] if isinstance(rung, str) else rung
        self.K = K = spec["K"]
        self.opt = o = HM.options(**spec["opt"])
        g = dict(mesh_of(spec["mesh"]))
        G = global_inputs(g, K, spec.get("ragged", False), spec.get("seed", 41), mixed_layer=o["kpp"])
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
                            SurfaceTracerFlux=np.stack([cells(f) for f in G["SurfaceTracerFlux"]]),
                            RediKappa=edges(G["RediKappa"]), FrictionVelocity=cells(G["FrictionVelocity"]),
                            SurfaceBuoyancyFlux=cells(G["SurfaceBuoyancyFlux"]))
        self.lo, self.hi = CR.local_layer_ranges(p.cell_id, G["min_level"], G["max_level"], self.nc, self.nc_size, K)
        self.column0 = column_seed(self.nc_size, K)
        self.seeds = object_seeds(self.nc_size, self.ne_size, K)
        assert np.array_equal(m.get_array("BottomDepth"), self.bottom)
        self.host = HM.HostModel(m, g, p.oracle, K, NT, (self.h, self.h1), (self.u, self.u1), (self.tr, self.tr1), self.lo,
                                 self.hi, self.bottom, self.ref, self.forcing, self.column0, o, DT, NSUB, deviations,
                                 seeds=self.seeds)
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
        self.eos = self.pg = self.va = self.mono = self.gm = self.vm = self.mix = self.redi = self.kpp = self.remap = None
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
        if o["kpp"]:
            self.kpp = oa.Kpp(m, vc, self.vm)
            for name in ("FrictionVelocity", "SurfaceBuoyancyFlux"):
                self.kpp.set(name, self.forcing[name])
            # the two constants as the library formed them (tests/kpp_fixtures.py): NonLocalCoeff holds a cbrt
            vt, nl = self.kpp.constants()
            mine = KR.constants(self.host.kpp_config)
            assert vt == mine[0] and abs(nl - mine[1]) <= 4.0 * np.spacing(nl)
            self.host.kpp_constants = (vt, nl)
            self.mix.attach_kpp(self.kpp)
        if o["redi"]:
            self.redi = oa.Redi(m, vc, self.eos, NT)
            for name in column_forcing:
                self.redi.set(name, self.forcing[name])
            self.redi.set("Kappa", self.forcing["RediKappa"])
            for name in ("SlopeInterface", "VertDiffusivity"):
                self.redi.set(name, self.seeds[name])
            self.mix.attach_redi(self.redi)
            st.attach_redi(self.redi)
        if o["remap"] is not None:
            self.remap = oa.VertRemap(m, vc, NT, o["remap"])
            self.remap.set("LayerThicknessTarget", self.seeds["RemapTarget"])
            st.attach_vert_remap(self.remap)

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
        if name in ("SlopeInterface", "VertDiffusivity"):
            return self.redi.get(name)
        if name in ("BoundaryLayerDepth", "BoundaryLayerIndex", "BulkRichardson", "NonLocalShape"):
            return self.kpp.get(name)
        if name == "RemapTarget":
            return self.remap.get("LayerThicknessTarget")
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
