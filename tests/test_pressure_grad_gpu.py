"""PressureGrad on the GPU: the kernel equals the NumPy restatement of the contract (tests/pressure_grad_reference.py)
bit for bit on NaN-seeded arrays -- tendency entries outside each edge's range, the row padding and the column fields
outside each cell's range are NaN and must stay so; the two compute forms agree; updateColumn equals the VertCoord's
column pass; attached to Tendencies the term is subtracted from NormalVelocityTend and nothing else moves; an ocean at
rest stays at rest under all three steppers; one homogeneous layer steps like the built-in SSH gradient; a 2-part
decomposition gives the 1-part values; the null-stream and stream forms agree; no step allocates."""
import numpy as np
import pytest

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests import pressure_grad_reference as PR
from tests.column_reference import RHO0
from tests.meshes import named_mesh
from tests.rank_rig import RankRig
from tests.vert_fixtures import EOS_OUT, VC_OUT, mix_inputs, same as _same

pytestmark = pytest.mark.gpu

NT = 2
EPS = np.finfo(np.float64).eps
MESHES = ("hex24x20", "fib700_coast_ragged")
LEVELS = (1, 15, 16, 37, 60, 80, 100)
CASES = [(m, K, e) for m in MESHES for K in LEVELS for e in ("teos10", "linear")]
STEPPERS = ("RungeKutta4", "RungeKutta2", "Forward-Backward")


@pytest.fixture(scope="module", autouse=True)
def _device():
    oa.device_init(0)


def forcing_inputs(g, seed):
    n = int(g["nCells"])
    rng = np.random.default_rng(seed + 100)
    return dict(ps=rng.uniform(0.9e5, 1.1e5, n), tidal=rng.uniform(-1.0, 1.0, n), sal=rng.uniform(-0.1, 0.1, n),
                bot=rng.uniform(100.0, 6000.0, n))


class Rig(RankRig):
    """One rank's VertCoord, Eos, OceanState, Tracers (T, S) and PressureGrad -- with `config` also AuxiliaryState and
    Tendencies -- on global inputs G (default: tests.vert_fixtures.mix_inputs, layer ranges with land) and forcing F
    in local order."""

    def __init__(self, g, K, eos_kind, nparts=1, rank=0, seed=7, full=False, G=None, F=None, linear=(-0.2, 0.8, 1000.0),
                 rho0=RHO0, config=None):
        super().__init__(g, K, nparts, rank)
        m = self.mesh
        G = self.G = mix_inputs(g, K, seed, full, NT) if G is None else G
        F = self.F = forcing_inputs(g, seed) if F is None else F
        self.h, self.tr, self.un = self.cells(G["h"]), self.cells(G["tr"]), self.edges(G["un"])
        self.ps, self.tidal, self.sal, self.bot = (self.cells(F[k]) for k in ("ps", "tidal", "sal", "bot"))
        self.layers(G["min_level"], G["max_level"], rho0=rho0)
        self.vc.set("BottomDepth", self.bot)
        self.eos = oa.Eos(m, K, eos_kind, *linear)
        self.state = oa.OceanState(m, None, K, 2)
        self.tracers = oa.Tracers(m, None, K, NT, 2)
        self.state.copy_to_device(self.h, self.un, 0)
        self.tracers.copy_to_device(self.tr, 0)
        self.pg = oa.PressureGrad(m, self.vc, self.eos)
        for name, v in (("SurfacePressure", self.ps), ("TidalPotential", self.tidal), ("SelfAttractionLoading", self.sal)):
            assert np.all(self.pg.get(name) == 0.0)  # zero at construction
            self.pg.set(name, v)
        self.coe, self.dc = m.get_array("CellsOnEdge"), m.get_array("DcEdge")
        self.mask = np.ascontiguousarray(m.get_array("EdgeMask")[:, 0])
        if config is not None:
            cfg = oa.default_config(**config)
            self.aux = oa.AuxiliaryState(m, None, K, NT)
            self.aux.set_options(cfg.FluxThicknessUpwind, cfg.FluxTracerUpwind, cfg.WindInterpIsotropic)
            self.tend = oa.Tendencies(m, K, NT, cfg)

    def poison(self):
        """every column field NaN: whatever a pass does not write stays NaN"""
        for name in VC_OUT:
            self.vc.set(name, np.full(self.vc.get(name).shape, np.nan))
        for name in EOS_OUT:
            self.eos.set(name, np.full((self.n_size, self.K), np.nan))

    def column(self, stream=None):
        self.vc.compute_column(self.state, self.tracers, self.eos, self.pg.device_ptr("SurfacePressure"),
                               self.pg.device_ptr("TidalPotential"), self.pg.device_ptr("SelfAttractionLoading"),
                               stream=stream)
        oa.device_synchronize()

    def fields(self):
        return self.vc.get("PressureMid"), self.vc.get("GeopotentialMid"), self.eos.get("SpecVol")

    def column_outputs(self):
        out = {name: self.vc.get(name) for name in VC_OUT}
        out["SpecVol"] = self.eos.get("SpecVol")
        return out

    def seeded_tend(self, seed=1):
        """(host [NEdgesSize][K], padded device copy): values inside each edge's range, NaN everywhere else -- other
        levels, the sentinel row, the pitch padding"""
        rng = np.random.default_rng(seed)
        t = np.full((self.e_size, self.K), np.nan)
        t[self.e_active] = rng.uniform(-1.0e-3, 1.0e-3, int(self.e_active.sum()))
        return t, oa.DeviceBuffer(self.padded(t))

    def restated(self, tend, fields=None):
        p, geo, sv = self.fields() if fields is None else fields
        return PR.pressure_grad(tend.copy(), p, geo, sv, self.coe, self.dc, self.mask, self.lo_e, self.hi_e, self.e_all)


@pytest.mark.parametrize("mesh,K,eos_kind", CASES)
def test_bit_exact_on_nan_seeded_arrays(mesh, K, eos_kind):
    x = Rig(named_mesh(mesh), K, eos_kind)
    x.poison()
    x.column()
    t, buf = x.seeded_tend()
    x.pg.compute(buf.ptr)
    oa.device_synchronize()
    want = x.restated(t)
    _same(buf.to_host(), x.padded(want), "Tend")
    assert np.isfinite(want[x.e_active]).all() and x.e_active.any()
    assert not np.array_equal(want[x.e_active], t[x.e_active])
    if "coast" in mesh:
        assert (~x.e_active[: x.e_all]).all(axis=1).any()  # edges next to land are left alone


@pytest.mark.parametrize("mesh,K,eos_kind", CASES)
def test_array_form_equals_attached_form(mesh, K, eos_kind):
    x = Rig(named_mesh(mesh), K, eos_kind)
    x.poison()
    x.column()
    t, a = x.seeded_tend()
    _, b = x.seeded_tend()
    x.pg.compute(a.ptr)
    x.pg.compute(b.ptr, x.vc.device_ptr("PressureMid"), x.vc.device_ptr("GeopotentialMid"), x.eos.device_ptr("SpecVol"))
    oa.device_synchronize()
    _same(b.to_host(), a.to_host(), "Tend (array form)")
    # the array form reads its arguments, not the attached arrays
    p, geo, sv = x.fields()
    other = (p * 0.75 + 10.0, geo * 1.5 - 3.0, sv * 1.25)
    _, c = x.seeded_tend()
    x.pg.compute(c.ptr, *other)
    oa.device_synchronize()
    _same(c.to_host(), x.padded(x.restated(t, other)), "Tend (caller's arrays)")
    got = x.pg.compute(np.nan_to_num(t), *other)  # the numpy form of the binding
    _same(got, x.restated(np.nan_to_num(t), other), "Tend (numpy form)")


@pytest.mark.parametrize("mesh,K,eos_kind", CASES)
def test_update_column_equals_compute_column(mesh, K, eos_kind):
    x = Rig(named_mesh(mesh), K, eos_kind)
    x.poison()
    x.column()
    t, a = x.seeded_tend()
    x.pg.compute(a.ptr)
    oa.device_synchronize()
    want = x.column_outputs()
    x.poison()
    x.pg.update_column(x.state.device_ptr(0, 0), x.tracers.device_ptr(0), NT)
    _, b = x.seeded_tend()
    x.pg.compute(b.ptr)
    oa.device_synchronize()
    for name, w in want.items():
        _same(x.column_outputs()[name], w, name)
    _same(b.to_host(), a.to_host(), "Tend")
    assert np.isnan(x.eos.get("SpecVolDisplaced")).all()  # Displaced = false


def _poison_tend(x):
    pitch = oa.level_pitch(x.K)
    for which, rows, planes in ((0, x.n_size, 1), (1, x.e_size, 1), (2, x.n_size, NT)):
        ptr, _ = x.tend.device_ptr(which)
        poison = np.full((planes, rows, pitch), np.nan)
        poison[:, -1, :] = 0.0
        oa.copy_to_device(ptr, poison)


def _rhs(x, stream=None):
    _poison_tend(x)
    x.tend.compute_all_tendencies(x.state, x.aux, x.tracers, stream=stream)
    if stream is not None:
        stream.synchronize()
    oa.device_synchronize()
    return [x.tend.get(i) for i in range(3)]


NO_SSH = dict(SSHTendencyEnable=0)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "reference_structured"])
@pytest.mark.parametrize("mesh,K,eos_kind", [("hex24x20", 60, "teos10"), ("fib700_coast_ragged", 37, "linear"),
                                             ("fib700_coast_ragged", 16, "teos10")])
def test_attached_rhs_subtracts_the_term_and_nothing_else(mesh, K, eos_kind, fused):
    x = Rig(named_mesh(mesh), K, eos_kind, config=NO_SSH)
    x.tend.set_fused(fused)
    base = _rhs(x)
    x.poison()  # the attached evaluation refreshes the column fields itself
    x.tend.attach_pressure_grad(x.pg)
    got = _rhs(x)
    fields = x.column_outputs()
    _same(got[1], x.restated(base[1]), "NormalVelocityTend")
    _same(got[0], base[0], "LayerThicknessTend")
    _same(got[2], base[2], "TracerTend")
    assert not np.array_equal(got[1], base[1], equal_nan=True)
    # ... with the fields of the stage's thickness and tracers
    x.poison()
    x.column()
    for name, w in x.column_outputs().items():
        _same(fields[name], w, name)
    # the velocity-only evaluation adds the term from the fields as they stand
    x.tend.attach_pressure_grad(None)
    x.tend.compute_velocity_tendencies(x.state, x.aux)
    oa.device_synchronize()
    vel = x.tend.get(1)
    x.tend.attach_pressure_grad(x.pg)
    other = (fields["PressureMid"] * 0.5, fields["GeopotentialMid"] * 2.0, fields["SpecVol"])
    x.vc.set("PressureMid", other[0])
    x.vc.set("GeopotentialMid", other[1])
    x.tend.compute_velocity_tendencies(x.state, x.aux)
    oa.device_synchronize()
    _same(x.tend.get(1), x.restated(vel, other), "NormalVelocityTend (velocity only)")


def test_attaching_with_the_ssh_gradient_enabled_raises():
    x = Rig(named_mesh("hex24x20"), 16, "teos10", config={})
    assert x.tend.config.SSHTendencyEnable
    with pytest.raises(oa.OmegaAmdError, match="SSHTendencyEnable"):
        x.tend.attach_pressure_grad(x.pg)
    base = _rhs(x)
    again = _rhs(x)  # nothing was attached
    for a, b in zip(again, base):
        _same(a, b, "tendencies")
    y = Rig(named_mesh("hex24x20"), 15, "teos10")
    with pytest.raises(oa.OmegaAmdError, match="another mesh"):
        oa.PressureGrad(x.mesh, y.vc, x.eos)
    with pytest.raises(oa.OmegaAmdError, match="another mesh"):
        oa.PressureGrad(x.mesh, x.vc, y.eos)


def test_detaching_restores_the_unattached_bits():
    g = named_mesh("hex24x20")
    x, twin = Rig(g, 37, "teos10", config=NO_SSH), Rig(g, 37, "teos10", config=NO_SSH)
    base = _rhs(x)
    x.tend.attach_pressure_grad(x.pg)
    assert not np.array_equal(_rhs(x)[1], base[1], equal_nan=True)
    x.tend.attach_pressure_grad(None)
    for a, b, name in zip(_rhs(x), base, ("LayerThicknessTend", "NormalVelocityTend", "TracerTend")):
        _same(a, b, name)
    for r in (x, twin):
        st = oa.TimeStepper("RungeKutta4", 60.0, r.tend, r.aux, r.mesh, None, r.tracers)
        st.do_step(r.state)
        oa.device_synchronize()
    for a, b in zip(x.state.copy_to_host(0), twin.state.copy_to_host(0)):
        _same(a, b, "state after a step")
    _same(x.tracers.copy_to_host(0), twin.tracers.copy_to_host(0), "tracers after a step")


def _rest_inputs(g, K):
    """Horizontally uniform and stratified; thicknesses are powers of two, so that (phi * h) / h, which the tracer
    updates of the steppers evaluate, returns phi exactly"""
    n, ne = int(g["nCells"]), int(g["nEdges"])
    k = np.arange(K)
    ones = np.ones((n, 1))
    G = dict(min_level=np.ones(n, np.int32), max_level=np.full(n, K, np.int32), h=ones * 2.0 ** (3 + k % 4),
             tr=np.stack([ones * (18.0 - 1.3 * k), ones * (34.0 + 0.11 * k)]), un=np.zeros((ne, K)))
    F = dict(ps=np.full(n, 1.01325e5), tidal=np.zeros(n), sal=np.zeros(n), bot=np.full(n, 400.0))
    return G, F


@pytest.mark.parametrize("kind", STEPPERS)
@pytest.mark.parametrize("eos_kind", ["teos10", "linear"])
def test_rest_stays_at_rest(kind, eos_kind):
    g, K = named_mesh("hex24x20"), 12
    G, F = _rest_inputs(g, K)
    x = Rig(g, K, eos_kind, G=G, F=F, config=NO_SSH)
    x.poison()
    x.column()  # Forward-Backward evaluates the velocity tendency alone: from the fields as they stand
    x.tend.attach_pressure_grad(x.pg)
    st = oa.TimeStepper(kind, 300.0, x.tend, x.aux, x.mesh, None, x.tracers)
    for _ in range(3):
        st.do_step(x.state)
    oa.device_synchronize()
    h, u = x.state.copy_to_host(0)
    assert np.all(u[: x.e_all] == 0.0)
    _same(h[: x.n_all], x.h[: x.n_all], "h")
    _same(x.tracers.copy_to_host(0)[:, : x.n_all], x.tr[:, : x.n_all], "T, S")
    p, geo, sv = x.fields()
    assert np.isfinite(p[: x.n_all]).all() and np.ptp(sv[: x.n_all], axis=1).min() > 0.0  # stratified, and computed


def test_one_homogeneous_layer_steps_like_the_ssh_gradient():
    """One layer of constant density (linear Eos without expansion, Rho0 = RhoT0S0 = R): the term is
    -g (R alpha) grad(h) + g grad(Bot) with g = 9.80616 -- the built-in SSH gradient -g' grad(h - Bot) with g' = 9.80665
    up to dg = |g' - g| / g, the rounding |R alpha - 1| of Rho0 * SpecVol, and the rounding of ZMid and PressureMid
    (two sums of magnitude Bot + h and g R h, a few eps each) against the signal, the largest thickness difference
    across an edge: 4 eps (Bot + max h) / max |dh|, plus 8 eps for the remaining operations.  From rest the velocity
    after a time t that is short against the gravity-wave period of the bump (g H t^2 (3 / sigma)^2 ~ 0.06 << 1) is
    -g t grad(eta) (1 + O((omega t)^2)): proportional to the force coefficient, with a sensitivity exponent within
    1 +- 1.  So the two runs agree to 2 (dg + |R alpha - 1| + 4 eps (Bot + max h) / max |dh| + 8 eps) of max |u|."""
    R, bot, dc, dt, steps = 1000.0, 1000.0, 30.0e3, 20.0, 5
    g = planar_hex(24, 20, dc, bottom_depth=bot)
    n, ne = int(g["nCells"]), int(g["nEdges"])
    sigma = 4.0 * dc
    r2 = (g["xCell"] - 0.5 * g["x_period"]) ** 2 + (g["yCell"] - 0.5 * g["y_period"]) ** 2
    G = dict(min_level=np.ones(n, np.int32), max_level=np.ones(n, np.int32),
             h=(bot + 0.5 * np.exp(-r2 / (2.0 * sigma ** 2)))[:, None],
             tr=np.stack([np.full((n, 1), 10.0), np.full((n, 1), 35.0)]), un=np.zeros((ne, 1)))
    F = dict(ps=np.zeros(n), tidal=np.zeros(n), sal=np.zeros(n), bot=np.full(n, bot))
    assert 9.80616 * bot * (steps * dt) ** 2 * (3.0 / sigma) ** 2 < 0.1
    ssh = Rig(g, 1, "linear", G=G, F=F, config={})
    lay = Rig(g, 1, "linear", G=G, F=F, linear=(0.0, 0.0, R), rho0=R, config=NO_SSH)
    lay.tend.attach_pressure_grad(lay.pg)
    us = []
    for x in (ssh, lay):
        st = oa.TimeStepper("RungeKutta4", dt, x.tend, x.aux, x.mesh, None, x.tracers)
        for _ in range(steps):
            st.do_step(x.state)
        oa.device_synchronize()
        us.append(x.state.copy_to_host(0)[1][: x.e_all])
    alpha = lay.eos.get("SpecVol")[0, 0]
    assert alpha == 1.0 / R
    dh = np.abs(lay.h[lay.coe[: lay.e_all, 1]] - lay.h[lay.coe[: lay.e_all, 0]]).max()
    dg = abs(9.80665 - 9.80616) / 9.80616
    bound = 2.0 * (dg + abs(R * alpha - 1.0) + 4.0 * EPS * (bot + lay.h.max()) / dh + 8.0 * EPS)
    scale = np.abs(us[0]).max()
    diff = np.abs(us[1] - us[0]).max()
    print(f"one layer: max |u| = {scale:.3e}, max |u_layered - u_ssh| = {diff:.3e} = {diff / scale:.3e} of it, "
          f"bound {bound:.3e} (dg = {dg:.3e})")
    assert scale > 0.0
    assert diff <= bound * scale


@pytest.mark.parametrize("mesh,K", [("hex24x20", 37), ("fib700_coast_ragged", 80), ("fib700_coast_ragged", 15)])
def test_two_part_decomposition_matches_one_part(mesh, K):
    g = named_mesh(mesh)

    def run(nparts, rank):
        x = Rig(g, K, "teos10", nparts=nparts, rank=rank)
        x.poison()
        x.pg.update_column(x.state.device_ptr(0, 0), x.tracers.device_ptr(0), NT)
        buf = oa.DeviceBuffer(x.padded(x.un))
        x.pg.compute(buf.ptr)
        oa.device_synchronize()
        return x, buf.to_host()

    one, ref = run(1, 0)
    edge1 = {int(e): i for i, e in enumerate(one.eid[: one.e_all])}
    for rank in (0, 1):
        x, got = run(2, rank)
        ei = np.array([edge1[int(e)] for e in x.eid[: x.e_own]])
        _same(got[: x.e_own], ref[ei], f"Tend rank {rank}")
        assert x.e_own < one.e_own


def test_stream_and_null_stream_forms_agree():
    g = named_mesh("fib700_coast_ragged")
    a, b = Rig(g, 60, "teos10", config=NO_SSH), Rig(g, 60, "teos10", config=NO_SSH)
    s = oa.Stream()
    out = []
    for x, st in ((a, None), (b, s)):
        x.poison()
        x.pg.update_column(x.state.device_ptr(0, 0), x.tracers.device_ptr(0), NT, stream=st)
        _, t1 = x.seeded_tend()
        _, t2 = x.seeded_tend()
        x.pg.compute(t1.ptr, stream=st)
        x.pg.compute(t2.ptr, x.vc.device_ptr("PressureMid"), x.vc.device_ptr("GeopotentialMid"),
                     x.eos.device_ptr("SpecVol"), stream=st)
        x.tend.attach_pressure_grad(x.pg)
        rhs = _rhs(x, stream=st)
        if st is not None:
            st.synchronize()
        oa.device_synchronize()
        out.append([t1.to_host(), t2.to_host()] + rhs)
    for p, q in zip(*out):
        _same(q, p, "stream form")


@pytest.mark.parametrize("kind", STEPPERS)
def test_no_allocation_in_a_step(kind):
    g = named_mesh("hex24x20")
    F = forcing_inputs(g, 7)
    F["bot"] = np.full(int(g["nCells"]), 4000.0)  # (random depths next to each other are a force no step survives)
    x = Rig(g, 37, "teos10", F=F, config=NO_SSH)
    x.tend.attach_pressure_grad(x.pg)
    st = oa.TimeStepper(kind, 1.0, x.tend, x.aux, x.mesh, None, x.tracers)
    _, buf = x.seeded_tend()
    s = oa.Stream()
    oa.device_synchronize()
    before = oa.device_resource_count()
    assert before > 0
    for _ in range(3):
        st.do_step(x.state, stream=s)
        x.pg.update_column(x.state.device_ptr(0, 0), x.tracers.device_ptr(0), NT, stream=s)
        x.pg.compute(buf.ptr, stream=s)
        x.pg.compute(buf.ptr, x.vc.device_ptr("PressureMid"), x.vc.device_ptr("GeopotentialMid"),
                     x.eos.device_ptr("SpecVol"), stream=s)
    s.synchronize()
    assert oa.device_resource_count() == before
    assert np.isfinite(x.state.copy_to_host(0)[0][: x.n_all]).all()
