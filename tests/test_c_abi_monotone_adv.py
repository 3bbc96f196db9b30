"""The C entry points of MonotoneAdv (include/omega_amd.h: omg_monoadv_*, omg_stepper_attach_monotone_adv) called as a C
program would: return codes and messages for null handles, a host-only mesh and unknown array names without a device;
on a device the calls give the restatement's bits and the named-array triple moves ScaleIn / ScaleOut."""
import ctypes as C
import os

import numpy as np
import pytest

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests.monotone_adv_fixtures import MonoRig

SYMBOLS = ("omg_monoadv_create", "omg_monoadv_destroy", "omg_monoadv_add_tracers", "omg_monoadv_device_ptr",
           "omg_monoadv_copy_to_host", "omg_monoadv_copy_to_device", "omg_stepper_attach_monotone_adv")


_err = oa.last_error


def test_symbols_are_exported_and_declared():
    L = oa.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omega_amd.h")).read()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert f"int {s}(" in header, s


def test_null_handles_and_a_host_only_mesh_are_errors():
    L = oa.lib()
    buf = (C.c_double * 4)()
    p = C.POINTER(C.c_double)()
    dt = C.c_double(1.0)
    assert L.omg_monoadv_add_tracers(None, buf, buf, buf, buf, buf, 1, dt, None) == 1 and "invalid argument" in _err()
    assert L.omg_monoadv_device_ptr(None, b"ScaleIn", C.byref(p), None) == 1 and "invalid argument" in _err()
    assert L.omg_monoadv_copy_to_host(None, b"ScaleIn", buf, C.c_size_t(4)) == 1
    assert L.omg_monoadv_copy_to_device(None, b"ScaleOut", buf, C.c_size_t(4)) == 1
    assert L.omg_stepper_attach_monotone_adv(None, None) == 1 and "invalid argument" in _err()
    assert L.omg_monoadv_destroy(None) == 0
    h = C.c_void_p()
    assert L.omg_monoadv_create(None, 4, 2, 0, C.byref(h)) == 1 and "invalid argument" in _err() and not h
    d = oa.Decomp(oa.GlobalMesh(planar_hex(8, 8, 1.0)), 1, 0, 3)
    m = oa.HorzMesh(d, 4, host_only=True)
    assert L.omg_monoadv_create(m.h, 4, 2, 0, None) == 1 and "invalid argument" in _err()
    assert L.omg_monoadv_create(m.h, 4, 2, 0, C.byref(h)) == 1 and "host-only" in _err() and not h


@pytest.mark.gpu
def test_calls_on_a_device():
    oa.device_init(0)
    L = oa.lib()
    K, nt, maxt = 6, 2, 3
    assert oa.level_pitch(K) == K  # compact rows, no padding
    R = MonoRig("hex24x20", K, device=True)
    I = R.inputs(seed=4, ntracers=3)
    m, nc = R.mesh, R.nc_size
    h = C.c_void_p()
    assert L.omg_monoadv_create(m.h, K, 0, 0, C.byref(h)) == 1 and "MaxTracers = 0" in _err() and not h
    assert L.omg_monoadv_create(m.h, 0, maxt, 0, C.byref(h)) == 1 and "NVertLayers = 0" in _err() and not h
    assert L.omg_monoadv_create(m.h, K, maxt, 0, C.byref(h)) == 0 and h
    # the named-array triple
    p, cnt = C.POINTER(C.c_double)(), C.c_size_t()
    for name in (b"ScaleIn", b"ScaleOut"):
        assert L.omg_monoadv_device_ptr(h, name, C.byref(p), C.byref(cnt)) == 0 and cnt.value == maxt * nc * K
    assert L.omg_monoadv_device_ptr(h, b"NoSuchArray", C.byref(p), None) == 1
    assert "MonotoneAdv: no array named NoSuchArray" in _err()
    out = np.ones((maxt, nc, K))
    pd = out.ctypes.data_as(C.POINTER(C.c_double))
    assert L.omg_monoadv_copy_to_host(h, b"NoSuchArray", pd, C.c_size_t(out.size)) == 1
    assert L.omg_monoadv_copy_to_device(h, b"NoSuchArray", pd, C.c_size_t(out.size)) == 1
    assert L.omg_monoadv_copy_to_host(h, b"ScaleIn", pd, C.c_size_t(out.size - 1)) == 1 and "too small" in _err()
    assert L.omg_monoadv_copy_to_device(h, b"ScaleIn", pd, C.c_size_t(out.size - 1)) == 1
    assert L.omg_monoadv_copy_to_host(h, b"ScaleIn", pd, C.c_size_t(out.size)) == 0 and np.all(out == 0.0)
    # the call against the restatement
    tend0 = np.random.default_rng(1).uniform(-1.0e-3, 1.0e-3, (nt, nc, K))
    bt, bho, bhn, bu, btr = (oa.DeviceBuffer(a) for a in (tend0, I.h_old, I.h_new, I.u, I.tracers))
    vp, dt = C.c_void_p, C.c_double(I.dt)
    args = (vp(bt.ptr), vp(bho.ptr), vp(bhn.ptr), vp(bu.ptr), vp(btr.ptr))
    assert L.omg_monoadv_add_tracers(h, None, *args[1:], nt, dt, None) == 1 and "invalid argument" in _err()
    assert L.omg_monoadv_add_tracers(h, *args[:3], None, args[4], nt, dt, None) == 1 and "invalid argument" in _err()
    for bad in (0, -1, maxt + 1):
        assert L.omg_monoadv_add_tracers(h, *args, bad, dt, None) == 1 and "is outside 1 .. MaxTracers = 3" in _err()
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        assert L.omg_monoadv_add_tracers(h, *args, nt, C.c_double(bad), None) == 1 and "not finite and positive" in _err()
    assert L.omg_monoadv_add_tracers(h, *args, nt, dt, None) == 0
    oa.device_synchronize()
    want, si, so = R.reference(I, nt, tend0, max_tracers=maxt)
    n = R.nc
    assert np.array_equal(bt.to_host()[:, :n], want[:, :n]) and np.array_equal(bt.to_host()[:, n:], tend0[:, n:])
    for name, ref in ((b"ScaleIn", si), (b"ScaleOut", so)):
        assert L.omg_monoadv_copy_to_host(h, name, pd, C.c_size_t(out.size)) == 0
        assert np.array_equal(out, ref) and (ref[:nt, :n] < 1.0).any() and (ref[nt:] == 0.0).all()
    assert L.omg_monoadv_copy_to_device(h, b"ScaleOut", pd, C.c_size_t(out.size)) == 0
    # attach / detach
    from tests.split_explicit_fixtures import StepRig
    x = StepRig(K=K, attached=False, config=dict(TracerHorzAdvTendencyEnable=0))
    st = x.stepper("Split-Explicit", 20.0, 2)
    assert L.omg_stepper_attach_monotone_adv(st.h, h) == 1 and "another mesh or layer count" in _err()
    h2 = C.c_void_p()
    assert L.omg_monoadv_create(x.p.mesh.h, K, x.nt, 0, C.byref(h2)) == 0
    assert L.omg_stepper_attach_monotone_adv(st.h, h2) == 0
    st.do_step(x.p.state)
    oa.device_synchronize()
    assert all(np.isfinite(a).all() for a in x.result())
    assert L.omg_stepper_attach_monotone_adv(st.h, None) == 0
    rk = x.stepper("RungeKutta4", 20.0)
    assert L.omg_stepper_attach_monotone_adv(rk.h, h2) == 1 and "not a Split-Explicit" in _err()
    assert L.omg_monoadv_destroy(h2) == 0 and L.omg_monoadv_destroy(h) == 0
