"""The C entry points of Kpp (include/omega_amd.h: omg_kpp_*, omg_vmix_step_attach_kpp) called as a C program would:
return codes and messages for null handles, a bad configuration, a host-only mesh and unknown array names without a
device; on a device the handle's lifetime, the two constants, the named arrays, the calls against the restatement and
the attachment."""
import ctypes as C
import os

import numpy as np
import pytest

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests import kpp_reference as KR

SYMBOLS = ("omg_kpp_config_default", "omg_kpp_create", "omg_kpp_destroy", "omg_kpp_compute", "omg_kpp_compute_arrays",
           "omg_kpp_apply_non_local", "omg_kpp_device_ptr", "omg_kpp_copy_to_host", "omg_kpp_copy_to_device",
           "omg_kpp_copy_to_host_i4", "omg_kpp_copy_to_device_i4", "omg_kpp_constants", "omg_kpp_launch_count",
           "omg_vmix_step_attach_kpp")
NAMES = (b"FrictionVelocity", b"SurfaceBuoyancyFlux", b"BoundaryLayerDepth", b"BulkRichardson", b"NonLocalShape")
FIELDS = ("VonKarman", "CritBulkRichardson", "SurfaceLayerFraction", "Cv", "EntrainmentRatio", "CStar")
PDBL = C.POINTER(C.c_double)


_err = oa.last_error


def test_symbols_are_exported_and_declared():
    L = oa.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omega_amd.h")).read()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert f"int {s}(" in header, s


def test_the_default_configuration():
    c = oa.kpp_config()
    assert [getattr(c, f) for f in FIELDS] == [0.4, 0.3, 0.1, 1.7, 0.2, 10.0]
    assert [getattr(c, f) for f in FIELDS] == [KR.DEFAULTS[f] for f in FIELDS]
    assert oa.kpp_config(Cv=1.5).Cv == 1.5
    with pytest.raises(KeyError):
        oa.kpp_config(NoSuchField=1.0)
    assert oa.lib().omg_kpp_config_default(None) == 1 and "invalid argument" in _err()


def test_null_handles_a_bad_configuration_and_a_host_only_mesh_are_errors():
    L = oa.lib()
    buf = (C.c_double * 4)()
    ibuf = (C.c_int32 * 4)()
    p = PDBL()
    n = C.c_int64()
    a, b = C.c_double(), C.c_double()
    assert L.omg_kpp_compute(None, buf, buf, None) == 1 and "invalid argument" in _err()
    assert L.omg_kpp_compute_arrays(None, buf, buf, buf, buf, buf, buf, buf, None) == 1 and "invalid argument" in _err()
    assert L.omg_kpp_apply_non_local(None, buf, buf, 1, C.c_double(1.0), buf, None) == 1 and "invalid argument" in _err()
    assert L.omg_kpp_constants(None, C.byref(a), C.byref(b)) == 1 and "invalid argument" in _err()
    assert L.omg_kpp_launch_count(None, C.byref(n)) == 1 and "invalid argument" in _err()
    for name in NAMES:
        assert L.omg_kpp_device_ptr(None, name, C.byref(p), None) == 1 and "invalid argument" in _err()
        assert L.omg_kpp_copy_to_host(None, name, buf, C.c_size_t(4)) == 1
        assert L.omg_kpp_copy_to_device(None, name, buf, C.c_size_t(4)) == 1
    assert L.omg_kpp_copy_to_host_i4(None, b"BoundaryLayerIndex", ibuf, C.c_size_t(4)) == 1
    assert L.omg_kpp_copy_to_device_i4(None, b"BoundaryLayerIndex", ibuf, C.c_size_t(4)) == 1
    assert L.omg_vmix_step_attach_kpp(None, None) == 1 and "invalid argument" in _err()
    assert L.omg_kpp_destroy(None) == 0
    h = C.c_void_p()
    assert L.omg_kpp_create(None, None, None, None, C.byref(h)) == 1 and "invalid argument" in _err() and not h
    d = oa.Decomp(oa.GlobalMesh(planar_hex(8, 8, 1.0)), 1, 0, 3)
    m = oa.HorzMesh(d, 4, host_only=True)
    assert L.omg_kpp_create(m.h, None, None, None, None) == 1 and "invalid argument" in _err()
    assert L.omg_kpp_create(m.h, None, None, None, C.byref(h)) == 1 and "host-only" in _err() and not h
    nan, inf = float("nan"), float("inf")
    bad = [("VonKarman", (0.0, -0.4, nan, inf), "not positive"), ("CritBulkRichardson", (0.0, -0.3, nan), "not positive"),
           ("SurfaceLayerFraction", (0.0, 1.0, -0.1, 1.5, nan), "outside (0, 1)"), ("Cv", (-1.0e-300, nan), "negative"),
           ("EntrainmentRatio", (-0.2, inf), "negative"), ("CStar", (-10.0, nan), "negative")]
    for field, values, rule in bad:
        for v in values:
            c = oa.kpp_config(**{field: v})
            assert L.omg_kpp_create(m.h, None, None, C.byref(c), C.byref(h)) == 1 and not h
            assert f"Kpp: {field} = " in _err() and rule in _err(), _err()
    # the limits of the ranges are inside them where the issue says so: zero Cv, EntrainmentRatio and CStar pass the
    # configuration check (the host-only mesh is what is refused next)
    c = oa.kpp_config(Cv=0.0, EntrainmentRatio=0.0, CStar=0.0)
    assert L.omg_kpp_create(m.h, None, None, C.byref(c), C.byref(h)) == 1 and "host-only" in _err() and not h


@pytest.mark.gpu
def test_calls_on_a_device():
    oa.device_init(0)
    L = oa.lib()
    K, nt = 6, 2
    d = oa.Decomp(oa.GlobalMesh(planar_hex(8, 8, 30.0e3)), 1, 0, 3)
    m = oa.HorzMesh(d, K)
    vc = oa.VertCoord(m, K, 1026.0, "Uniform", decomp=d)
    vm = oa.VertMix(m, vc)
    nc, ne = m.NCellsSize, m.NEdgesSize
    h = C.c_void_p()
    assert L.omg_kpp_create(m.h, None, vm.h, None, C.byref(h)) == 1 and "VertCoord is NULL" in _err() and not h
    assert L.omg_kpp_create(m.h, vc.h, None, None, C.byref(h)) == 1 and "VertMix is NULL" in _err() and not h
    m2 = oa.HorzMesh(d, K)
    vc2 = oa.VertCoord(m2, K, 1026.0, "Uniform", decomp=d)
    vm2 = oa.VertMix(m2, vc2)
    assert L.omg_kpp_create(m.h, vc2.h, vm.h, None, C.byref(h)) == 1 and "another mesh" in _err() and not h
    assert L.omg_kpp_create(m.h, vc.h, vm2.h, None, C.byref(h)) == 1 and "another mesh" in _err() and not h
    cfg = oa.kpp_config(Cv=1.5, CStar=7.0, VonKarman=0.41)
    assert L.omg_kpp_create(m.h, vc.h, vm.h, C.byref(cfg), C.byref(h)) == 0 and h
    # the two constants: the two expressions of Kpp.h
    a, b = C.c_double(), C.c_double()
    assert L.omg_kpp_constants(h, C.byref(a), None) == 1 and "invalid argument" in _err()
    assert L.omg_kpp_constants(h, C.byref(a), C.byref(b)) == 0
    kappa, ric, eps = np.float64(0.41), np.float64(0.3), np.float64(0.1)
    assert a.value == (np.float64(1.5) * np.sqrt(np.float64(0.2))) / ((ric * (kappa * kappa)) * np.sqrt(98.96 * eps))
    # (the host's cbrt and NumPy's are each within an ulp or two of the root, not of each other: the product within 4)
    want_b = (np.float64(7.0) * kappa) * np.cbrt((98.96 * kappa) * eps)
    assert abs(b.value - want_b) <= 4.0 * np.spacing(want_b)
    consts = (a.value, b.value)  # the restatement takes them as inputs
    assert consts[0] == KR.constants(KR.config(Cv=1.5, CStar=7.0, VonKarman=0.41))[0]
    h0 = C.c_void_p()
    assert L.omg_kpp_create(m.h, vc.h, vm.h, None, C.byref(h0)) == 0  # NULL: the defaults
    assert L.omg_kpp_constants(h0, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == KR.constants(KR.config())
    assert L.omg_kpp_destroy(h0) == 0
    # the named arrays
    p, cnt = PDBL(), C.c_size_t()
    sizes = {b"FrictionVelocity": nc, b"SurfaceBuoyancyFlux": nc, b"BoundaryLayerDepth": nc, b"BulkRichardson": nc * K,
             b"NonLocalShape": nc * K}
    for name in NAMES:
        assert L.omg_kpp_device_ptr(h, name, C.byref(p), C.byref(cnt)) == 0 and cnt.value == sizes[name] and p
        out = np.ones(sizes[name])
        pd = out.ctypes.data_as(PDBL)
        assert L.omg_kpp_copy_to_host(h, name, pd, C.c_size_t(out.size - 1)) == 1 and "too small" in _err()
        assert L.omg_kpp_copy_to_device(h, name, pd, C.c_size_t(out.size - 1)) == 1 and "size mismatch" in _err()
        assert L.omg_kpp_copy_to_host(h, name, pd, C.c_size_t(out.size)) == 0 and np.all(out == 0.0)
    assert L.omg_kpp_device_ptr(h, b"NoSuchArray", C.byref(p), None) == 1 and "Kpp: no array named NoSuchArray" in _err()
    idx = np.ones(nc, np.int32)
    pi = idx.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.omg_kpp_copy_to_host_i4(h, b"BoundaryLayerIndex", pi, C.c_size_t(nc - 1)) == 1 and "too small" in _err()
    assert L.omg_kpp_copy_to_host_i4(h, b"NonLocalShape", pi, C.c_size_t(nc)) == 1 and "no int array named" in _err()
    assert L.omg_kpp_copy_to_host_i4(h, b"BoundaryLayerIndex", pi, C.c_size_t(nc)) == 0 and np.all(idx == 0)
    assert L.omg_kpp_copy_to_device_i4(h, b"BoundaryLayerIndex", pi, C.c_size_t(nc + 1)) == 1 and "size mismatch" in _err()
    # the calls against the restatement (K = 6: compact rows, no padding)
    assert oa.level_pitch(K) == K and oa.level_pitch(K + 1) == K + 1
    rng = np.random.default_rng(5)
    hh = rng.uniform(2.0, 12.0, (nc, K))
    zint = -np.concatenate([np.zeros((nc, 1)), np.cumsum(hh, axis=1)], axis=1)
    zmid = 0.5 * (zint[:, :-1] + zint[:, 1:])
    n2 = np.where(np.arange(K)[None, :] < 3, rng.uniform(-2.0e-9, 1.0e-8, (nc, K)), rng.uniform(1.0e-6, 6.0e-5, (nc, K)))
    un, ut = rng.uniform(-0.1, 0.1, (2, ne, K))
    us, bf = 2.0 ** -rng.integers(6, 10, nc).astype(np.float64), rng.uniform(0.0, 1.0e-7, nc)  # no cbrt: bit for bit
    vd, vv = rng.uniform(1.0e-5, 1.0e-2, (2, nc, K))
    tr, flux = rng.uniform(0.0, 30.0, (nt, nc, K)), rng.uniform(-1.0e-4, 1.0e-4, (nt, nc))
    assert L.omg_kpp_copy_to_device(h, b"FrictionVelocity", us.ctypes.data_as(PDBL), C.c_size_t(nc)) == 0
    assert L.omg_kpp_copy_to_device(h, b"SurfaceBuoyancyFlux", bf.ctypes.data_as(PDBL), C.c_size_t(nc)) == 0
    bun, but, bn2, bzm, bzi, bvd, bvv, bh, btr, bfl = (oa.DeviceBuffer(x) for x in (un, ut, n2, zmid, zint, vd, vv, hh, tr, flux))
    vp = C.c_void_p
    launches = C.c_int64(-1)
    assert L.omg_kpp_launch_count(h, C.byref(launches)) == 0 and launches.value == 0
    assert L.omg_kpp_compute_arrays(h, vp(bun.ptr), vp(but.ptr), vp(bn2.ptr), vp(bzm.ptr), None, vp(bvd.ptr), vp(bvv.ptr),
                                    None) == 1 and "invalid argument" in _err()
    assert L.omg_kpp_compute_arrays(h, vp(bun.ptr), vp(but.ptr), vp(bn2.ptr), vp(bzm.ptr), vp(bzi.ptr), vp(bvd.ptr),
                                    vp(bvv.ptr), None) == 0
    oa.device_synchronize()
    lo, hi = vc.get("MinLayerCell"), vc.get("MaxLayerCell")
    cfgd = KR.config(Cv=1.5, CStar=7.0, VonKarman=0.41)
    r = KR.compute(un, ut, n2, zmid, zint, vd, vv, us, bf, lo, hi, m.NCellsAll, m.get_array("NEdgesOnCell"),
                   m.get_array("EdgesOnCell"), m.get_array("DcEdge"), m.get_array("DvEdge"), m.get_array("AreaCell"),
                   1.0e-4, 1.0e-5, *consts, cfgd)
    assert not r["used_cbrt"].any() and r["inside"].any()

    def named(name, shape):
        out = np.empty(shape)
        assert L.omg_kpp_copy_to_host(h, name, out.ctypes.data_as(PDBL), C.c_size_t(out.size)) == 0
        return out

    assert np.array_equal(named(b"BulkRichardson", (nc, K)), r["BulkRichardson"])
    assert np.array_equal(named(b"NonLocalShape", (nc, K)), r["NonLocalShape"])
    assert np.array_equal(named(b"BoundaryLayerDepth", (nc,)), r["BoundaryLayerDepth"])
    assert L.omg_kpp_copy_to_host_i4(h, b"BoundaryLayerIndex", pi, C.c_size_t(nc)) == 0
    assert np.array_equal(idx, r["BoundaryLayerIndex"])
    assert np.array_equal(bvd.to_host(), r["VertDiff"]) and np.array_equal(bvv.to_host(), r["VertVisc"])
    assert not np.array_equal(r["VertDiff"], vd)
    # the attached form on the VertMix's and the VertCoord's arrays
    vm.set("BruntVaisalaFreqSq", n2)
    vm.set("VertDiff", vd)
    vm.set("VertVisc", vv)
    vc.set("ZMid", zmid)
    vc.set("ZInterface", zint)
    assert L.omg_kpp_compute(h, vp(bun.ptr), None, None) == 1 and "invalid argument" in _err()
    assert L.omg_kpp_compute(h, vp(bun.ptr), vp(but.ptr), None) == 0
    oa.device_synchronize()
    assert np.array_equal(vm.get("VertDiff"), r["VertDiff"]) and np.array_equal(vm.get("VertVisc"), r["VertVisc"])
    # the non-local redistribution (Bf >= 0 here: a shape of zeros; a destabilising flux for a non-trivial one)
    bf2 = -bf - 1.0e-9
    assert L.omg_kpp_copy_to_device(h, b"SurfaceBuoyancyFlux", bf2.ctypes.data_as(PDBL), C.c_size_t(nc)) == 0
    assert L.omg_kpp_compute(h, vp(bun.ptr), vp(but.ptr), None) == 0
    oa.device_synchronize()
    shape = named(b"NonLocalShape", (nc, K))
    assert (shape > 0.0).any()
    dt = C.c_double(600.0)
    assert L.omg_kpp_apply_non_local(h, None, vp(btr.ptr), nt, dt, vp(bfl.ptr), None) == 1 and "invalid argument" in _err()
    assert L.omg_kpp_apply_non_local(h, vp(bh.ptr), vp(btr.ptr), -1, dt, vp(bfl.ptr), None) == 1
    assert L.omg_kpp_apply_non_local(h, vp(bh.ptr), vp(btr.ptr), nt, dt, None, None) == 0  # no flux: nothing is done
    oa.device_synchronize()
    assert np.array_equal(btr.to_host(), tr)
    assert L.omg_kpp_apply_non_local(h, vp(bh.ptr), vp(btr.ptr), nt, dt, vp(bfl.ptr), None) == 0
    oa.device_synchronize()
    want = KR.apply_non_local(hh, tr, nt, 600.0, flux, shape, lo, hi, m.NCellsOwned)
    assert np.array_equal(btr.to_host(), want) and not np.array_equal(want, tr)
    assert L.omg_kpp_launch_count(h, C.byref(launches)) == 0 and launches.value == 4
    # attach / detach
    eos = oa.Eos(m, K, "linear")
    mix = oa.VertMixStep(m, vm, vc, eos, nt)
    h2 = C.c_void_p()
    assert L.omg_kpp_create(m2.h, vc2.h, vm2.h, None, C.byref(h2)) == 0
    assert L.omg_vmix_step_attach_kpp(mix.h, h2) == 1 and "another mesh or layer count" in _err()
    assert L.omg_vmix_step_attach_kpp(mix.h, h) == 0
    assert L.omg_vmix_step_attach_kpp(mix.h, None) == 0
    assert L.omg_kpp_destroy(h2) == 0
    assert L.omg_kpp_destroy(h) == 0
