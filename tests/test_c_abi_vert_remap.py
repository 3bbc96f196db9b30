"""The C entry points of VertRemap (include/omega_amd.h: omg_vremap_*, omg_stepper_attach_vert_remap) called as a C
program would: return codes and messages for null handles, bad parameters, a host-only mesh and unknown array names
without a device; on a device the handle's lifetime, the named-array triple, the five calls against the restatement and
the attachment."""
import ctypes as C
import os

import numpy as np
import pytest

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests import column_reference as CR
from tests import vert_remap_reference as VR

SYMBOLS = ("omg_vremap_create", "omg_vremap_destroy", "omg_vremap_max_layers", "omg_vremap_compute_target",
           "omg_vremap_remap_tracers", "omg_vremap_remap_velocity", "omg_vremap_adopt_target", "omg_vremap_remap",
           "omg_vremap_launch_count", "omg_vremap_device_ptr", "omg_vremap_copy_to_device", "omg_vremap_copy_to_host",
           "omg_stepper_attach_vert_remap")
NAME = b"LayerThicknessTarget"
PDBL = C.POINTER(C.c_double)


_err = oa.last_error


def test_symbols_are_exported_and_declared():
    L = oa.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omega_amd.h")).read()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert f"int {s}(" in header, s


def test_null_handles_bad_parameters_and_a_host_only_mesh_are_errors():
    L = oa.lib()
    buf = (C.c_double * 4)()
    p = PDBL()
    n = C.c_int64()
    assert L.omg_vremap_compute_target(None, buf, None) == 1 and "invalid argument" in _err()
    assert L.omg_vremap_remap_tracers(None, buf, buf, 1, None) == 1 and "invalid argument" in _err()
    assert L.omg_vremap_remap_velocity(None, buf, buf, None) == 1 and "invalid argument" in _err()
    assert L.omg_vremap_adopt_target(None, buf, None) == 1 and "invalid argument" in _err()
    assert L.omg_vremap_remap(None, buf, buf, buf, 1, None) == 1 and "invalid argument" in _err()
    assert L.omg_vremap_launch_count(None, C.byref(n)) == 1 and "invalid argument" in _err()
    assert L.omg_vremap_max_layers(None) == 1 and "invalid argument" in _err()
    assert L.omg_vremap_device_ptr(None, NAME, C.byref(p), None) == 1 and "invalid argument" in _err()
    assert L.omg_vremap_copy_to_host(None, NAME, buf, C.c_size_t(4)) == 1
    assert L.omg_vremap_copy_to_device(None, NAME, buf, C.c_size_t(4)) == 1
    assert L.omg_stepper_attach_vert_remap(None, None) == 1 and "invalid argument" in _err()
    assert L.omg_vremap_destroy(None) == 0
    limit = C.c_int()
    assert L.omg_vremap_max_layers(C.byref(limit)) == 0 and limit.value >= 256  # (needs no device)
    h = C.c_void_p()
    assert L.omg_vremap_create(None, None, 3, 2, C.byref(h)) == 1 and "invalid argument" in _err() and not h
    d = oa.Decomp(oa.GlobalMesh(planar_hex(8, 8, 1.0)), 1, 0, 3)
    m = oa.HorzMesh(d, 4, host_only=True)
    assert L.omg_vremap_create(m.h, None, 3, 2, None) == 1 and "invalid argument" in _err()
    assert L.omg_vremap_create(m.h, None, 3, 2, C.byref(h)) == 1 and "host-only" in _err() and not h


@pytest.mark.gpu
def test_calls_on_a_device():
    oa.device_init(0)
    L = oa.lib()
    K, nt, rho0 = 6, 2, 1026.0
    d = oa.Decomp(oa.GlobalMesh(planar_hex(8, 8, 30.0e3)), 1, 0, 3)
    m = oa.HorzMesh(d, K)
    vc = oa.VertCoord(m, K, rho0, "Uniform", decomp=d)
    nc, ne = m.NCellsSize, m.NEdgesSize
    h = C.c_void_p()
    assert L.omg_vremap_create(m.h, None, 3, nt, C.byref(h)) == 1 and "VertCoord is NULL" in _err() and not h
    m2 = oa.HorzMesh(d, K)
    vc2 = oa.VertCoord(m2, K, rho0, "Uniform", decomp=d)
    assert L.omg_vremap_create(m.h, vc2.h, 3, nt, C.byref(h)) == 1 and "another mesh" in _err() and not h
    for order in (0, 4):
        assert L.omg_vremap_create(m.h, vc.h, order, nt, C.byref(h)) == 1 and "Order" in _err() and not h
    assert L.omg_vremap_create(m.h, vc.h, 3, -1, C.byref(h)) == 1 and "MaxTracers" in _err() and not h
    assert L.omg_vremap_create(m.h, vc.h, 3, nt, C.byref(h)) == 0 and h
    # the named-array triple
    p, cnt = PDBL(), C.c_size_t()
    assert L.omg_vremap_device_ptr(h, NAME, C.byref(p), C.byref(cnt)) == 0 and cnt.value == nc * K and p
    out = np.ones(nc * K)
    pd = out.ctypes.data_as(PDBL)
    assert L.omg_vremap_copy_to_host(h, NAME, pd, C.c_size_t(out.size - 1)) == 1 and "too small" in _err()
    assert L.omg_vremap_copy_to_device(h, NAME, pd, C.c_size_t(out.size - 1)) == 1 and "size mismatch" in _err()
    assert L.omg_vremap_copy_to_host(h, NAME, pd, C.c_size_t(out.size)) == 0 and np.all(out == 0.0)  # zero at creation
    assert L.omg_vremap_device_ptr(h, b"NoSuchArray", C.byref(p), None) == 1
    assert "VertRemap: no array named NoSuchArray" in _err()
    assert L.omg_vremap_copy_to_host(h, b"NoSuchArray", pd, C.c_size_t(4)) == 1
    assert L.omg_vremap_copy_to_device(h, b"NoSuchArray", pd, C.c_size_t(4)) == 1
    # the calls against the restatement (K = 6: compact rows, no padding)
    assert oa.level_pitch(K) == K
    rng = np.random.default_rng(5)
    ref = rng.uniform(5.0, 30.0, (nc, K))
    vc.set("RefLayerThickness", ref)
    hh = ref * rng.uniform(0.9, 1.1, (nc, 1)) * rng.uniform(0.7, 1.3, (nc, K))
    tr = np.stack([rng.uniform(2.0, 20.0, (nc, K)), rng.uniform(33.0, 36.0, (nc, K))])
    uu = rng.uniform(-0.1, 0.1, (ne, K))
    lo_c, hi_c = vc.get("MinLayerCell"), vc.get("MaxLayerCell")
    lo_e, hi_e = vc.get("MinLayerEdgeBot"), vc.get("MaxLayerEdgeTop")
    coe, w = m.get_array("CellsOnEdge"), CR.movement_weights("Uniform", K)
    want_t = VR.compute_target(hh, ref, w, lo_c, hi_c, m.NCellsAll, np.zeros((nc, K)))
    want_tr = VR.remap_tracers(hh, want_t, tr.copy(), nt, lo_c, hi_c, m.NCellsAll, 3)
    want_u = VR.remap_velocity(hh, want_t, uu.copy(), coe, lo_e, hi_e, m.NEdgesAll, nc, 3)
    want_h = VR.adopt_target(hh.copy(), want_t, lo_c, hi_c, m.NCellsAll)
    bh, btr, bu = (oa.DeviceBuffer(a) for a in (hh, tr, uu))
    vp = C.c_void_p
    launches = C.c_int64(-1)
    assert L.omg_vremap_launch_count(h, C.byref(launches)) == 0 and launches.value == 0
    assert L.omg_vremap_compute_target(h, None, None) == 1 and "invalid argument" in _err()
    assert L.omg_vremap_compute_target(h, vp(bh.ptr), None) == 0
    oa.device_synchronize()
    got = np.empty((nc, K))
    assert L.omg_vremap_copy_to_host(h, NAME, got.ctypes.data_as(PDBL), C.c_size_t(got.size)) == 0
    assert np.array_equal(got, want_t) and not np.array_equal(want_t[: m.NCellsAll], hh[: m.NCellsAll])
    assert L.omg_vremap_remap_tracers(h, vp(bh.ptr), None, nt, None) == 1 and "invalid argument" in _err()
    for bad in (-1, 3):
        assert L.omg_vremap_remap_tracers(h, vp(bh.ptr), vp(btr.ptr), bad, None) == 1 and "NTracers" in _err()
    assert L.omg_vremap_remap_tracers(h, vp(bh.ptr), vp(btr.ptr), 0, None) == 0  # no launch
    assert L.omg_vremap_remap_tracers(h, vp(bh.ptr), vp(btr.ptr), nt, None) == 0
    assert L.omg_vremap_remap_velocity(h, vp(bh.ptr), None, None) == 1 and "invalid argument" in _err()
    assert L.omg_vremap_remap_velocity(h, vp(bh.ptr), vp(bu.ptr), None) == 0
    assert L.omg_vremap_adopt_target(h, None, None) == 1 and "invalid argument" in _err()
    assert L.omg_vremap_adopt_target(h, vp(bh.ptr), None) == 0
    oa.device_synchronize()
    assert np.array_equal(btr.to_host(), want_tr) and not np.array_equal(want_tr, tr)
    assert np.array_equal(bu.to_host(), want_u) and not np.array_equal(want_u, uu)
    assert np.array_equal(bh.to_host(), want_h)
    assert L.omg_vremap_launch_count(h, C.byref(launches)) == 0 and launches.value == 4
    # the one call, from the same start
    bh2, btr2, bu2 = (oa.DeviceBuffer(a) for a in (hh, tr, uu))
    assert L.omg_vremap_remap(h, vp(bh2.ptr), None, vp(btr2.ptr), nt, None) == 1 and "invalid argument" in _err()
    assert L.omg_vremap_remap(h, vp(bh2.ptr), vp(bu2.ptr), vp(btr2.ptr), 3, None) == 1 and "NTracers" in _err()
    assert L.omg_vremap_remap(h, vp(bh2.ptr), vp(bu2.ptr), vp(btr2.ptr), nt, None) == 0
    oa.device_synchronize()
    assert np.array_equal(bh2.to_host(), want_h) and np.array_equal(bu2.to_host(), want_u)
    assert np.array_equal(btr2.to_host(), want_tr)
    assert L.omg_vremap_launch_count(h, C.byref(launches)) == 0 and launches.value == 7
    # attach / detach
    aux = oa.AuxiliaryState(m, None, K, nt)
    tracers = oa.Tracers(m, None, K, nt, 2)
    tend = oa.Tendencies(m, K, nt)
    rk = oa.TimeStepper("RungeKutta4", 60.0, tend, aux, m, None, tracers)
    assert L.omg_stepper_attach_vert_remap(rk.h, h) == 1 and "Split-Explicit" in _err()
    se = oa.TimeStepper("Split-Explicit", 60.0, tend, aux, m, None, tracers)
    h2 = C.c_void_p()
    assert L.omg_vremap_create(m2.h, vc2.h, 2, nt, C.byref(h2)) == 0
    assert L.omg_stepper_attach_vert_remap(se.h, h2) == 1 and "another mesh or layer count" in _err()
    h1 = C.c_void_p()
    assert L.omg_vremap_create(m.h, vc.h, 1, 1, C.byref(h1)) == 0
    assert L.omg_stepper_attach_vert_remap(se.h, h1) == 1 and "MaxTracers = 1" in _err()
    va = oa.VertAdv(m, vc, 2)
    tend.attach_vert_adv(va)
    assert L.omg_stepper_attach_vert_remap(se.h, h) == 1 and "a VertAdv is attached" in _err()
    tend.attach_vert_adv(None)
    assert L.omg_stepper_attach_vert_remap(se.h, h) == 0
    assert L.omg_stepper_attach_vert_remap(se.h, None) == 0
    for x in (h1, h2, h):
        assert L.omg_vremap_destroy(x) == 0
