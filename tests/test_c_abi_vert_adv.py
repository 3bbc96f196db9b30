"""The C entry points of VertAdv (include/omega_amd.h: omg_vertadv_*, omg_tend_attach_vert_adv) called as a C program
would: return codes and messages for null handles, a host-only mesh and unknown array names without a device; on a
device the calls give the restatement's bits and the named-array triple moves VerticalTransport."""
import ctypes as C

import numpy as np
import pytest

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests import vert_adv_reference as VR

SYMBOLS = ("omg_vertadv_create", "omg_vertadv_destroy", "omg_vertadv_max_layers", "omg_vertadv_compute_transport",
           "omg_vertadv_add_thickness", "omg_vertadv_add_tracers", "omg_vertadv_add_velocity", "omg_vertadv_device_ptr",
           "omg_vertadv_copy_to_host", "omg_vertadv_copy_to_device", "omg_tend_attach_vert_adv")


_err = oa.last_error


def test_symbols_are_exported_and_declared():
    L = oa.lib()
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omega_amd.h")).read()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert f"int {s}(" in header, s


def test_null_handles_and_a_host_only_mesh_are_errors():
    L = oa.lib()
    buf = (C.c_double * 4)()
    p = C.POINTER(C.c_double)()
    assert L.omg_vertadv_compute_transport(None, buf, 0, None) == 1 and "invalid argument" in _err()
    assert L.omg_vertadv_add_thickness(None, buf, None) == 1 and "invalid argument" in _err()
    assert L.omg_vertadv_add_tracers(None, buf, buf, buf, 1, None) == 1 and "invalid argument" in _err()
    assert L.omg_vertadv_add_velocity(None, buf, buf, buf, None) == 1 and "invalid argument" in _err()
    assert L.omg_vertadv_device_ptr(None, b"VerticalTransport", C.byref(p), None) == 1 and "invalid argument" in _err()
    assert L.omg_vertadv_copy_to_host(None, b"VerticalTransport", buf, C.c_size_t(4)) == 1
    assert L.omg_vertadv_copy_to_device(None, b"VerticalTransport", buf, C.c_size_t(4)) == 1
    assert L.omg_tend_attach_vert_adv(None, None) == 1 and "invalid argument" in _err()
    assert L.omg_vertadv_destroy(None) == 0
    h = C.c_void_p()
    assert L.omg_vertadv_create(None, None, 2, C.byref(h)) == 1 and "invalid argument" in _err() and not h
    n = C.c_int()
    assert L.omg_vertadv_max_layers(C.byref(n)) == 0 and n.value >= 1024
    assert L.omg_vertadv_max_layers(None) == 1
    d = oa.Decomp(oa.GlobalMesh(planar_hex(8, 8, 1.0)), 1, 0, 3)
    m = oa.HorzMesh(d, 4, host_only=True)
    assert L.omg_vertadv_create(m.h, None, 2, C.byref(h)) == 1 and "host-only" in _err() and not h


@pytest.mark.gpu
def test_calls_on_a_device():
    oa.device_init(0)
    L = oa.lib()
    K, nt = 6, 2
    d = oa.Decomp(oa.GlobalMesh(planar_hex(8, 8, 30.0e3)), 1, 0, 3)
    m = oa.HorzMesh(d, K)
    vc = oa.VertCoord(m, K, 1026.0, "Uniform", decomp=d)
    nc, ne, n_all, e_all = m.NCellsSize, m.NEdgesSize, m.NCellsAll, m.NEdgesAll
    rng = np.random.default_rng(2)
    ref = rng.uniform(1.0, 30.0, (nc, K))
    vc.set("RefLayerThickness", ref)
    h = C.c_void_p()
    assert L.omg_vertadv_create(m.h, vc.h, 7, C.byref(h)) == 1 and "TracerFluxOrder = 7" in _err() and not h
    assert L.omg_vertadv_create(m.h, None, 2, C.byref(h)) == 1 and "VertCoord is NULL" in _err() and not h
    assert L.omg_vertadv_create(m.h, vc.h, 2, C.byref(h)) == 0 and h
    # the named-array triple
    p, cnt = C.POINTER(C.c_double)(), C.c_size_t()
    assert L.omg_vertadv_device_ptr(h, b"VerticalTransport", C.byref(p), C.byref(cnt)) == 0 and cnt.value == nc * K
    assert L.omg_vertadv_device_ptr(h, b"NoSuchArray", C.byref(p), None) == 1
    assert "VertAdv: no array named NoSuchArray" in _err()
    out = np.ones((nc, K))
    pd = out.ctypes.data_as(C.POINTER(C.c_double))
    assert L.omg_vertadv_copy_to_host(h, b"NoSuchArray", pd, C.c_size_t(out.size)) == 1
    assert L.omg_vertadv_copy_to_device(h, b"NoSuchArray", pd, C.c_size_t(out.size)) == 1
    assert L.omg_vertadv_copy_to_host(h, b"VerticalTransport", pd, C.c_size_t(out.size - 1)) == 1 and "too small" in _err()
    assert L.omg_vertadv_copy_to_device(h, b"VerticalTransport", pd, C.c_size_t(out.size - 1)) == 1
    assert L.omg_vertadv_copy_to_host(h, b"VerticalTransport", pd, C.c_size_t(out.size)) == 0 and np.all(out == 0.0)
    # the four calls against the restatement (K = 6: compact rows, no padding)
    assert oa.level_pitch(K) == K
    lo, hi = np.zeros(nc, np.int32), np.full(nc, K - 1, np.int32)
    lo_e, hi_e = vc.get("MinLayerEdgeBot"), vc.get("MaxLayerEdgeTop")
    coe, mask = m.get_array("CellsOnEdge"), np.ascontiguousarray(m.get_array("EdgeMask")[:, 0])
    dd, hh = rng.uniform(-1.0e-3, 1.0e-3, (nc, K)), rng.uniform(0.5, 40.0, (nc, K))
    tr, uu = rng.uniform(-1.0, 1.0, (nt, nc, K)), rng.uniform(-0.05, 0.05, (ne, K))
    bd, bd2, bh, btr, bu = (oa.DeviceBuffer(a) for a in (dd, dd, hh, tr, uu))
    btt, but = oa.DeviceBuffer(tr * 1.0e-3), oa.DeviceBuffer(uu * 1.0e-2)
    vp = C.c_void_p
    assert L.omg_vertadv_compute_transport(h, None, 0, None) == 1 and "invalid argument" in _err()
    assert L.omg_vertadv_compute_transport(h, vp(bd.ptr), 0, None) == 0
    assert L.omg_vertadv_add_thickness(h, vp(bd.ptr), None) == 0
    assert L.omg_vertadv_compute_transport(h, vp(bd2.ptr), 1, None) == 0
    assert L.omg_vertadv_add_tracers(h, vp(btt.ptr), vp(bh.ptr), vp(btr.ptr), nt, None) == 0
    assert L.omg_vertadv_add_tracers(h, vp(btt.ptr), vp(bh.ptr), vp(btr.ptr), -1, None) == 1
    assert L.omg_vertadv_add_velocity(h, vp(but.ptr), vp(bh.ptr), vp(bu.ptr), None) == 0
    assert L.omg_vertadv_add_velocity(h, vp(but.ptr), None, vp(bu.ptr), None) == 1
    oa.device_synchronize()
    wt = VR.vertical_transport(dd, ref, np.ones(K), lo, hi, n_all, np.zeros((nc, K)))
    th = VR.add_thickness_tend(dd.copy(), wt, lo, hi, n_all)
    assert np.array_equal(bd.to_host(), th) and np.array_equal(bd2.to_host(), th)
    assert L.omg_vertadv_copy_to_host(h, b"VerticalTransport", pd, C.c_size_t(out.size)) == 0
    assert np.array_equal(out, wt) and np.abs(wt).max() > 0.0
    assert np.array_equal(btt.to_host(), VR.add_tracer_tend(tr * 1.0e-3, hh, tr, wt, lo, hi, n_all, 2))
    assert np.array_equal(but.to_host(), VR.add_velocity_tend(uu * 1.0e-2, hh, uu, wt, coe, mask, lo_e, hi_e, e_all))
    # copy_to_device, attach / detach
    assert L.omg_vertadv_copy_to_device(h, b"VerticalTransport", pd, C.c_size_t(out.size)) == 0
    t = oa.Tendencies(m, K, nt)
    assert L.omg_tend_attach_vert_adv(t.h, h) == 0
    assert L.omg_tend_attach_vert_adv(t.h, None) == 0
    m2 = oa.HorzMesh(d, K)
    t2 = oa.Tendencies(m2, K, nt)
    assert L.omg_tend_attach_vert_adv(t2.h, h) == 1 and "another mesh or layer count" in _err()
    assert L.omg_vertadv_destroy(h) == 0
