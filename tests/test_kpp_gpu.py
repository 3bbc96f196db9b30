"""Kpp on the GPU against the NumPy restatement of its contract (tests/kpp_reference.py), at every layer count at which
the scan takes another pass or the packed-column launch changes shape, on NaN-seeded outputs: columns that evaluate no
cbrt equal the restatement bit for bit in all six outputs, columns that do have the same boundary-layer index and agree
within a derived bound; what the contract does not write stays as it was; the attached, array and stream forms agree in
one launch and without an allocation; the non-local redistribution equals its restatement bit for bit; VertMixStep and
an RK4 step with a Kpp attached equal the public calls made by hand, and detaching restores the unattached bits."""
import numpy as np
import pytest

import omega_amd as oa
from tests import kpp_reference as KR
from tests.column_reference import RHO0
from tests.kpp_fixtures import NT, OUT2, KppRig
from tests.meshes import named_mesh
from tests.problem import Problem
from tests.rank_rig import raw
from tests.vert_fixtures import Mix, pcr_levels, same, systems_launch

pytestmark = pytest.mark.gpu

MESHES = ("hex24x20", "fib300_coast_ragged")
LEVELS = (1, 2, 3, 5, 8, 9, 33, 64, 65, 129, 256, 257, 1024)
# The device's cbrt and glibc's are each within about 1 - 2 ulp of the root (2.2e-16 each).  A column that is not
# `marginal` amplifies a relative error of its bulk Richardson numbers by at most 1e3 through the interpolation of hbl
# (|Rib_kb - Rib_(kb-1)| >= 1e-3 of the larger), so hbl and what follows from it move by about 1e3 * 4 ulp ~ 1e-12 to
# 1e-11 of their size; ten times that.
CBRT_BOUND = 1.0e-10
DT = 1800.0


@pytest.fixture(scope="module", autouse=True)
def _device():
    oa.device_init(0)


def test_the_levels_cover_the_scan_passes_and_the_launch_shapes():
    # 0 .. 10 passes of the scan in the deepest column (5 passes: the shorter columns of the larger cases)
    assert sorted({pcr_levels(K) for K in LEVELS}) == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10]
    shape = {K: systems_launch(K) for K in LEVELS}
    assert [shape[K][0] for K in LEVELS] == [256, 128, 85, 51, 32, 28, 7, 4, 3, 1, 1, 1, 1]  # columns per workgroup
    assert shape[3][2] - shape[3][1] == 1 and shape[257][2] - shape[257][1] == 63  # lanes without a row
    assert shape[256][2] == 256 and shape[257][2] == 320 and shape[1024][2] == 1024  # one long column, up to 1024 lanes


def compare(x, r, out, vd, vv):
    """the six outputs of a compute against the restatement r, by column class"""
    got = dict(out, VertDiff=vd, VertVisc=vv)
    exact = ~r["used_cbrt"] & ~r["marginal"]  # land and the sentinel row among them
    close = r["used_cbrt"] & ~r["marginal"]
    for name in ("BulkRichardson", "NonLocalShape", "VertDiff", "VertVisc"):
        want = x.padded(r[name])
        same(got[name][exact], want[exact], name)
        # the columns with a cbrt: the same entries written, zeroed and left alone, and the values within the bound
        g, w = got[name][close], want[close]
        assert np.array_equal(np.isnan(g), np.isnan(w)), name
        scale = np.where(np.isnan(w), 0.0, np.abs(w)).max(axis=1, initial=0.0)[:, None]  # the column's largest
        assert np.all(np.abs(g - w)[~np.isnan(w)] <= (CBRT_BOUND * scale * np.ones_like(w))[~np.isnan(w)]), name
        assert np.array_equal(g == 0.0, w == 0.0), name
    same(got["BoundaryLayerDepth"][exact], r["BoundaryLayerDepth"][exact], "BoundaryLayerDepth")
    assert np.array_equal(got["BoundaryLayerIndex"][exact | close], r["BoundaryLayerIndex"][exact | close])
    hg, hw = got["BoundaryLayerDepth"][close], r["BoundaryLayerDepth"][close]
    assert np.all(np.abs(hg - hw) <= CBRT_BOUND * np.abs(hw))
    # below the boundary layer (and everywhere the contract writes nothing) the coefficients keep the seeded bits
    keep = ~x.padded(r["inside"], fill=False).astype(bool)
    keep[r["marginal"]] = False
    same(vd[keep], x.padded(x.vd)[keep], "VertDiff outside the layer")
    same(vv[keep], x.padded(x.vv)[keep], "VertVisc outside the layer")
    return exact, close


@pytest.mark.parametrize("mesh", MESHES)
@pytest.mark.parametrize("K", LEVELS)
def test_values_against_the_restatement_on_nan_seeded_outputs(mesh, K):
    x = KppRig(named_mesh(mesh), K)
    assert x.kpp.constants() == x.consts and x.consts[0] == KR.constants(x.cfg)[0]
    for name in OUT2:  # zero at construction
        assert np.all(raw(x.kpp.device_ptr(name), (x.n_size, x.P)) == 0.0)
    assert np.all(x.kpp.get("BoundaryLayerDepth") == 0.0) and np.all(x.kpp.get("BoundaryLayerIndex") == 0)
    x.poison()
    before = x.kpp.launch_count()
    vd, vv = x.compute_arrays()
    assert x.kpp.launch_count() == before + 1
    r = x.expected()
    out = x.outputs()
    exact, close = compare(x, r, out, vd, vv)
    # the case is what it is there for
    v = r["valid"]
    assert (exact & v).sum() >= 0.2 * v.sum() and close.sum() >= 0.05 * v.sum() and (~v[: x.n_all]).any()
    assert np.isnan(out["BulkRichardson"][:, K:]).all() and np.isnan(vd[:, K:]).all()  # the row padding
    assert np.all(out["BulkRichardson"][-1, :K] == 0.0) and out["BoundaryLayerIndex"][-1] == -1  # the sentinel row
    if K >= 3:
        inside = r["inside"]
        assert inside.any() and (x.faces & ~inside).any()  # interfaces inside and below the layer
        assert (r["NonLocalShape"] > 0.0).any() and (r["BulkRichardson"] < 0.0).any()


@pytest.mark.parametrize("mesh,K", [("fib300_coast_ragged", 9), ("hex24x20", 65), ("fib300_coast_ragged", 257)])
def test_the_forms_agree_in_one_launch_without_an_allocation(mesh, K):
    x = KppRig(named_mesh(mesh), K)
    r = x.expected()
    s = oa.Stream()
    un, ut = x.dev(x.un), x.dev(x.ut)
    results = []
    for stream in (None, s):
        x.poison()
        vd, vv = x.compute_arrays(stream=stream)
        results.append(dict(x.outputs(), VertDiff=vd[:, :K], VertVisc=vv[:, :K]))
        # the attached form: the VertMix's and the VertCoord's arrays as they stand
        x.vm.set("BruntVaisalaFreqSq", x.n2)
        x.vm.set("VertDiff", x.vd)
        x.vm.set("VertVisc", x.vv)
        x.vc.set("ZMid", x.zmid)
        x.vc.set("ZInterface", x.zint)
        x.poison()
        oa.device_synchronize()
        before, launches = oa.device_resource_count(), x.kpp.launch_count()
        x.kpp.compute(un.ptr, ut.ptr, stream=stream)
        x.sync(stream)
        assert oa.device_resource_count() == before and x.kpp.launch_count() == launches + 1
        results.append(dict(x.outputs(), VertDiff=x.vm.get("VertDiff"), VertVisc=x.vm.get("VertVisc")))
    for o in results[1:]:
        for name, want in results[0].items():
            same(o[name], want, name)
    compare(x, r, {n: results[0][n] for n in OUT2 + ("BoundaryLayerDepth", "BoundaryLayerIndex")},
            x.padded(results[0]["VertDiff"]), x.padded(results[0]["VertVisc"]))
    # the array form reads its arguments: other heights, another answer, still the restatement's
    zmid, zint = x.zmid * 1.25, x.zint * 1.25
    x.poison()
    vd, vv = x.compute_arrays(zmid=zmid, zint=zint)
    other = x.outputs()
    compare(x, x.expected(zmid=zmid, zint=zint), other, vd, vv)
    assert not np.array_equal(other["BoundaryLayerDepth"], results[0]["BoundaryLayerDepth"])
    with pytest.raises(oa.OmegaAmdError, match="together"):
        x.kpp.compute(un.ptr, ut.ptr, bvf=x.n2)


@pytest.mark.parametrize("mesh,K,nparts", [("hex24x20", 9, 2), ("fib300_coast_ragged", 33, 1), ("hex24x20", 257, 1),
                                           ("fib300_coast_ragged", 1, 1)])
def test_the_non_local_redistribution(mesh, K, nparts):
    x = KppRig(named_mesh(mesh), K, nparts=nparts, rank=nparts - 1)
    assert (x.n_own < x.n_all) == (nparts > 1)  # halo cells
    x.compute_arrays()
    shape = x.outputs()["NonLocalShape"][:, :K]
    tr = x.seeded(x.tr)  # NaN outside the ranges, on land and on the rows from NCellsAll on
    h = x.seeded(x.h)
    flux = np.where(np.arange(x.n_size)[None, :] < x.n_own, x.flux, np.nan)  # not read beyond the owned cells
    buf, hb, fb = x.dev(tr), x.dev(h), oa.DeviceBuffer(flux)
    oa.device_synchronize()
    before, launches = oa.device_resource_count(), x.kpp.launch_count()
    x.kpp.apply_non_local(hb.ptr, buf.ptr, NT - 1, DT, surface_flux=fb.ptr)  # the last plane is beyond NTracers
    oa.device_synchronize()
    assert oa.device_resource_count() == before and x.kpp.launch_count() == launches + 1
    want = KR.apply_non_local(h, tr, NT - 1, DT, flux, shape, x.lo, x.hi, x.n_own)
    got = buf.to_host()
    same(got, x.padded(want), "Tracers")
    same(want[NT - 1], tr[NT - 1], "the plane beyond NTracers")
    same(want[:, x.n_own:], tr[:, x.n_own:], "halo cells")
    if K >= 3:
        assert not np.array_equal(want[: NT - 1], tr[: NT - 1], equal_nan=True)
    # a stream, and an empty flux: no launch, nothing written
    s = oa.Stream()
    buf2 = x.dev(tr)
    x.kpp.apply_non_local(hb.ptr, buf2.ptr, NT - 1, DT, surface_flux=fb.ptr, stream=s)
    x.sync(s)
    same(buf2.to_host(), got, "Tracers (stream)")
    launches = x.kpp.launch_count()
    x.kpp.apply_non_local(hb.ptr, buf2.ptr, NT - 1, DT)
    oa.device_synchronize()
    assert x.kpp.launch_count() == launches
    same(buf2.to_host(), got, "Tracers (empty flux)")
    with pytest.raises(oa.OmegaAmdError, match="invalid argument"):
        x.kpp.apply_non_local(hb.ptr, buf2.ptr, -1, DT, surface_flux=fb.ptr)


# ---- VertMixStep and the steppers
def _forcing(n_size, e_size, nt, seed=21):
    rng = np.random.default_rng(seed)
    us, bf = rng.uniform(0.0, 0.02, n_size), rng.uniform(-2.0e-7, 1.0e-7, n_size)
    us[::9], bf[::11] = 0.0, 0.0
    return dict(us=us, bf=bf, flux=rng.uniform(-1.0e-4, 1.0e-4, (nt, n_size)), stress=rng.uniform(-0.2, 0.2, e_size))


def _by_hand(mesh, vc, eos, vm, kpp, redi, hp, up, tp, un_host, nt, f, dt, cd, ra):
    """steps 3 to 6 of VertMixStep.h with 4a, 4b and 4c, as public calls (the column pass and N2 are the caller's)"""
    ut = oa.HorzOperators(mesh).tangential_recon(un_host)
    keep = []
    unp, utp = oa._level_dev(un_host, mesh.NEdgesSize, vm.K, keep), oa._level_dev(ut, mesh.NEdgesSize, vm.K, keep)
    vm.compute(unp.value, utp.value)
    if kpp is not None:
        kpp.compute(unp.value, utp.value)
    if redi is not None:
        redi.compute_vert_diffusivity(vm.device_ptr("VertDiff"))
    if kpp is not None:
        kpp.apply_non_local(hp, tp, nt, dt, surface_flux=f["flux"])
    vm.apply_tracers(hp, tp, nt, dt, surface_flux=f["flux"])
    vm.apply_velocity(hp, up, dt, boundary=(cd, ra), stress=f["stress"], ut=ut)
    oa.device_synchronize()


@pytest.mark.parametrize("K,with_redi", [(3, False), (17, True), (64, False), (17, False)])
def test_vert_mix_step_with_a_kpp_equals_the_calls_by_hand(K, with_redi):
    nt, cd, ra = 3, 2.5e-3, 1.0e-5
    x = Mix(named_mesh("fib300_coast_ragged"), K, "teos10", ntracers=nt, ragged=True)
    f = _forcing(x.n_size, x.e_size, nt)
    step = oa.VertMixStep(x.mesh, x.vm, x.vc, x.eos, nt)
    step.set("NormalStressEdge", f["stress"])
    step.set("SurfaceTracerFlux", f["flux"])
    step.set_boundary(cd, ra, True)
    kpp = oa.Kpp(x.mesh, x.vc, x.vm)
    kpp.set("FrictionVelocity", f["us"])
    kpp.set("SurfaceBuoyancyFlux", f["bf"])
    redi = None
    if with_redi:
        redi = oa.Redi(x.mesh, x.vc, x.eos, nt)
        redi.update_column(x.h, x.tr[:2], 2)
        redi.compute_slope(x.h)
    hp, up, tp = x.state.device_ptr(0, 0), x.state.device_ptr(1, 0), x.tracers.device_ptr(0)

    def reset():
        x.state.copy_to_device(x.h, x.un, 0)
        x.tracers.copy_to_device(x.tr, 0)
        for name in ("VertDiff", "VertVisc", "BruntVaisalaFreqSq"):
            x.vm.set(name, np.full((x.n_size, K), np.nan))
        for name in OUT2:
            kpp.set(name, np.full((x.n_size, K), np.nan))

    def results():
        oa.device_synchronize()
        out = {name: x.vm.get(name) for name in ("VertDiff", "VertVisc", "BruntVaisalaFreqSq")}
        out.update({name: kpp.get(name) for name in OUT2 + ("BoundaryLayerDepth", "BoundaryLayerIndex")})
        out["u"], out["tr"] = x.state.copy_to_host(0)[1], x.tracers.copy_to_host(0)
        return out

    def hand(with_kpp):
        reset()
        x.vc.compute_column(x.state, x.tracers, x.eos, kdisp=1)
        x.vm.compute_bvf(x.eos)
        _by_hand(x.mesh, x.vc, x.eos, x.vm, kpp if with_kpp else None, redi, hp, up, tp, x.un, nt, f, DT, cd, ra)
        return results()

    by_hand, plain = hand(True), hand(False)
    step.attach_redi(redi)
    step.attach_kpp(kpp)
    launches = kpp.launch_count()
    reset()
    step.apply(hp, up, tp, DT)
    got = results()
    assert kpp.launch_count() == launches + 2
    for name, want in by_hand.items():
        same(got[name], want, name)
    assert np.isfinite(got["tr"][:, x.active]).all() and np.isfinite(got["u"][x.e_active]).all()
    assert not np.array_equal(got["VertDiff"], plain["VertDiff"], equal_nan=True)
    if K > 3:
        assert not np.array_equal(got["tr"], plain["tr"], equal_nan=True)
    assert (got["BoundaryLayerDepth"] > 0.0).any()
    # detached: the unattached bits
    step.attach_kpp(None)
    reset()
    step.apply(hp, up, tp, DT)
    got = results()
    for name in ("VertDiff", "VertVisc", "u", "tr"):
        same(got[name], plain[name], name + " (detached)")


class _StepRig:
    """hex24x20, 9 layers, temperature and salinity; a VertMixStep with every forcing on and a Kpp for it"""

    def __init__(self):
        K, nt = 9, 2
        p = self.p = Problem(named_mesh("hex24x20"), K, nt, config=dict(SSHTendencyEnable=0), oracle=False)
        m = p.mesh
        rng = np.random.default_rng(31)
        nc, ne = m.NCellsSize, m.NEdgesSize
        h, u, tr = np.zeros((nc, K)), np.zeros((ne, K)), np.zeros((nt, nc, K))
        h[: m.NCellsAll] = rng.uniform(8.0, 12.0, (m.NCellsAll, K))
        u[: m.NEdgesAll] = rng.uniform(-0.05, 0.05, (m.NEdgesAll, K))
        tr[0, : m.NCellsAll] = 20.0 - np.cumsum(rng.uniform(0.0, 1.5, (m.NCellsAll, K)), axis=1)  # warm above cold
        tr[1, : m.NCellsAll] = rng.uniform(34.9, 35.0, (m.NCellsAll, K))
        p.state.copy_to_device(h, u, 0)
        p.tracers.copy_to_device(tr, 0)
        self.vc = oa.VertCoord(m, K, RHO0, "Uniform", decomp=p.decomp)
        self.eos = oa.Eos(m, K, "teos10")
        self.vm = oa.VertMix(m, self.vc)
        self.step = oa.VertMixStep(m, self.vm, self.vc, self.eos, nt)
        self.f = _forcing(nc, ne, nt)
        self.step.set("NormalStressEdge", self.f["stress"])
        self.step.set("SurfaceTracerFlux", self.f["flux"])
        self.step.set_boundary(2.5e-3, 1.0e-5, True)
        self.kpp = oa.Kpp(m, self.vc, self.vm)
        self.kpp.set("FrictionVelocity", self.f["us"])
        self.kpp.set("SurfaceBuoyancyFlux", self.f["bf"])
        self.st = oa.TimeStepper("RungeKutta4", 20.0, p.tend, p.aux, m, p.halo, p.tracers)

    def result(self):
        oa.device_synchronize()
        h, u = self.p.state.copy_to_host(0)
        return dict(h=h, u=u, tr=self.p.tracers.copy_to_host(0), hbl=self.kpp.get("BoundaryLayerDepth"))


def test_an_rk4_step_with_the_hook_equals_the_step_and_the_calls_by_hand():
    a = _StepRig()
    a.step.attach_kpp(a.kpp)
    a.st.attach_vert_mix(a.step)
    a.st.do_step(a.p.state)
    oa.device_synchronize()
    before = oa.device_resource_count()
    a.st.do_step(a.p.state)
    attached = a.result()
    assert oa.device_resource_count() == before  # a step creates no buffer, stream or event

    b = _StepRig()
    p = b.p
    for _ in range(2):
        b.st.do_step(p.state)
        oa.device_synchronize()
        b.vc.compute_column(p.state, p.tracers, b.eos, kdisp=1)
        b.vm.compute_bvf(b.eos)
        _by_hand(p.mesh, b.vc, b.eos, b.vm, b.kpp, None, p.state.device_ptr(0, 0), p.state.device_ptr(1, 0),
                 p.tracers.device_ptr(0), p.state.copy_to_host(0)[1], 2, b.f, 20.0, 2.5e-3, 1.0e-5)
    by_hand = b.result()

    c = _StepRig()
    c.st.attach_vert_mix(c.step)  # no Kpp: only the mixing differs
    for _ in range(2):
        c.st.do_step(c.p.state)
    plain = c.result()

    d = _StepRig()
    d.step.attach_kpp(d.kpp)
    d.step.attach_kpp(None)
    d.st.attach_vert_mix(d.step)
    for _ in range(2):
        d.st.do_step(d.p.state)
    detached = d.result()

    for name in ("h", "u", "tr"):
        assert np.all(np.isfinite(attached[name])), name
        same(attached[name], by_hand[name], f"{name}: attached against step + calls by hand")
        same(detached[name], plain[name], f"{name}: detached against unattached")
    same(attached["hbl"], by_hand["hbl"], "BoundaryLayerDepth")
    assert (attached["hbl"][: a.p.mesh.NCellsAll] > 0.0).all() and np.all(detached["hbl"] == 0.0)
    assert not np.array_equal(attached["u"], plain["u"]) and not np.array_equal(attached["tr"], plain["tr"])


def test_refusals_that_need_a_device():
    g = named_mesh("fib300_coast_ragged")
    x, y = KppRig(g, 5), KppRig(g, 5)
    with pytest.raises(oa.OmegaAmdError, match="VertCoord is NULL"):
        oa.Kpp(x.mesh, None, x.vm)
    with pytest.raises(oa.OmegaAmdError, match="VertMix is NULL"):
        oa.Kpp(x.mesh, x.vc, None)
    with pytest.raises(oa.OmegaAmdError, match="another mesh"):
        oa.Kpp(x.mesh, y.vc, x.vm)
    with pytest.raises(oa.OmegaAmdError, match="another mesh"):
        oa.Kpp(x.mesh, x.vc, y.vm)
    other_vc = oa.VertCoord(x.mesh, 5, RHO0, "Uniform", decomp=x.decomp)
    with pytest.raises(oa.OmegaAmdError, match="different VertCoord"):
        oa.Kpp(x.mesh, other_vc, x.vm)
    with pytest.raises(oa.OmegaAmdError, match="layer counts"):
        oa.Kpp(x.mesh, oa.VertCoord(x.mesh, 4, RHO0, "Uniform", decomp=x.decomp), x.vm)
    with pytest.raises(KeyError):
        oa.Kpp(x.mesh, x.vc, x.vm, NoSuchField=1.0)
    for bad in (dict(VonKarman=0.0), dict(CritBulkRichardson=-0.3), dict(SurfaceLayerFraction=1.0),
                dict(SurfaceLayerFraction=0.0), dict(Cv=-1.0), dict(EntrainmentRatio=-0.2), dict(CStar=-10.0)):
        with pytest.raises(oa.OmegaAmdError, match=next(iter(bad))):
            oa.Kpp(x.mesh, x.vc, x.vm, **bad)
    with pytest.raises(oa.OmegaAmdError, match="no array named"):
        x.kpp.get("NoSuchArray")
    # a shape that is not the object's
    un, ut = x.dev(x.un), x.dev(x.ut)
    with pytest.raises(oa.OmegaAmdError, match="invalid argument"):
        oa._chk(oa.lib().omg_kpp_compute(x.kpp.h, None, oa.C.c_void_p(ut.ptr), None))
    # attachKpp
    eos = oa.Eos(x.mesh, 5, "linear")
    step = oa.VertMixStep(x.mesh, x.vm, x.vc, eos, 2)
    with pytest.raises(oa.OmegaAmdError, match="another mesh or layer count"):
        step.attach_kpp(y.kpp)
    other_vm = oa.VertMix(x.mesh, x.vc)
    with pytest.raises(oa.OmegaAmdError, match="different VertCoord or VertMix"):
        step.attach_kpp(oa.Kpp(x.mesh, x.vc, other_vm))
    step.attach_kpp(x.kpp)
    step.attach_kpp(None)
    # a non-default configuration reaches the kernel
    z = KppRig(g, 9, CritBulkRichardson=0.25, Cv=1.5, CStar=5.0, SurfaceLayerFraction=0.15, VonKarman=0.41,
               EntrainmentRatio=0.3, vmix_cfg=dict(BackgroundViscosity=2.0e-4, BackgroundDiffusivity=3.0e-5))
    z.poison()
    vd, vv = z.compute_arrays()
    compare(z, z.expected(), z.outputs(), vd, vv)
