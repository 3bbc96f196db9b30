"""The C entry points of BarotropicMode (include/omega_amd.h: omg_btr_*) called as a C program would: return codes and
messages for null handles, a host-only mesh and unknown array names without a device; on a device the calls give the
restatement's bits and the named-array triple moves each of the six arrays."""
import ctypes as C
import os

import numpy as np
import pytest

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests import barotropic_reference as BR
from tests.barotropic_fixtures import GRAVITY, btr_mesh

SYMBOLS = ("omg_btr_create", "omg_btr_destroy", "omg_btr_max_layers", "omg_btr_split_velocity",
           "omg_btr_compute_forcing", "omg_btr_compute_ssh", "omg_btr_recombine", "omg_btr_subcycle",
           "omg_btr_device_ptr", "omg_btr_copy_to_host", "omg_btr_copy_to_device")
ARRAYS = ("BtrVelocity", "BtrThickEdge", "BtrForcing", "BtrFluxMean", "SSH", "BclVelocity")
G = C.c_double(GRAVITY)


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
    assert L.omg_btr_split_velocity(None, buf, buf, 0, None) == 1 and "invalid argument" in _err()
    assert L.omg_btr_compute_forcing(None, buf, buf, None) == 1 and "invalid argument" in _err()
    assert L.omg_btr_compute_ssh(None, buf, None) == 1 and "invalid argument" in _err()
    assert L.omg_btr_recombine(None, buf, None) == 1 and "invalid argument" in _err()
    assert L.omg_btr_subcycle(None, 1, C.c_double(1.0), None) == 1 and "invalid argument" in _err()
    for name in ARRAYS:
        assert L.omg_btr_device_ptr(None, name.encode(), C.byref(p), None) == 1 and "invalid argument" in _err()
        assert L.omg_btr_copy_to_host(None, name.encode(), buf, C.c_size_t(4)) == 1
        assert L.omg_btr_copy_to_device(None, name.encode(), buf, C.c_size_t(4)) == 1
    assert L.omg_btr_destroy(None) == 0
    h = C.c_void_p()
    assert L.omg_btr_create(None, None, G, C.byref(h)) == 1 and "invalid argument" in _err() and not h
    n = C.c_int()
    assert L.omg_btr_max_layers(C.byref(n)) == 0 and n.value >= 1024
    assert L.omg_btr_max_layers(None) == 1
    d = oa.Decomp(oa.GlobalMesh(planar_hex(8, 8, 1.0)), 1, 0, 3)
    m = oa.HorzMesh(d, 4, host_only=True)
    assert L.omg_btr_create(m.h, None, G, C.byref(h)) == 1 and "host-only" in _err() and not h


@pytest.mark.gpu
def test_calls_on_a_device():
    oa.device_init(0)
    L = oa.lib()
    K = 6
    d = oa.Decomp(oa.GlobalMesh(planar_hex(8, 8, 30.0e3, bottom_depth=500.0)), 1, 0, 3)
    m = oa.HorzMesh(d, K)
    vc = oa.VertCoord(m, K, 1026.0, "Uniform", decomp=d)
    nc, ne, n_all, e_all = m.NCellsSize, m.NEdgesSize, m.NCellsAll, m.NEdgesAll
    h = C.c_void_p()
    assert L.omg_btr_create(m.h, None, G, C.byref(h)) == 1 and "VertCoord is NULL" in _err() and not h
    assert L.omg_btr_create(m.h, vc.h, G, C.byref(h)) == 0 and h
    shapes = {name: (ne,) for name in ARRAYS}
    shapes.update(SSH=(nc,), BclVelocity=(ne, K))
    # the named-array triple of every array
    p, cnt = C.POINTER(C.c_double)(), C.c_size_t()
    assert L.omg_btr_device_ptr(h, b"NoSuchArray", C.byref(p), None) == 1
    assert "BarotropicMode: no array named NoSuchArray" in _err()
    rng = np.random.default_rng(4)
    for name in ARRAYS:
        size = int(np.prod(shapes[name]))
        assert L.omg_btr_device_ptr(h, name.encode(), C.byref(p), C.byref(cnt)) == 0 and cnt.value == size and p
        out = np.ones(shapes[name])
        pd = out.ctypes.data_as(C.POINTER(C.c_double))
        assert L.omg_btr_copy_to_host(h, name.encode(), pd, C.c_size_t(size - 1)) == 1 and "too small" in _err()
        assert L.omg_btr_copy_to_device(h, name.encode(), pd, C.c_size_t(size - 1)) == 1
        assert L.omg_btr_copy_to_host(h, name.encode(), pd, C.c_size_t(size)) == 0 and np.all(out == 0.0)
        val = rng.uniform(-1.0, 1.0, shapes[name])
        assert L.omg_btr_copy_to_device(h, name.encode(), val.ctypes.data_as(C.POINTER(C.c_double)), C.c_size_t(size)) == 0
        assert L.omg_btr_copy_to_host(h, name.encode(), pd, C.c_size_t(size)) == 0 and np.array_equal(out, val)
    out = np.ones(4)
    pd = out.ctypes.data_as(C.POINTER(C.c_double))
    assert L.omg_btr_copy_to_host(h, b"NoSuchArray", pd, C.c_size_t(4)) == 1
    assert L.omg_btr_copy_to_device(h, b"NoSuchArray", pd, C.c_size_t(4)) == 1
    # the five calls against the restatement (K = 6: compact rows, no padding)
    assert oa.level_pitch(K) == K
    lo, hi = np.zeros(nc, np.int32), np.full(nc, K - 1, np.int32)
    lo[n_all:], hi[n_all:] = -1, -1
    lo_e, hi_e = vc.get("MinLayerEdgeBot"), vc.get("MaxLayerEdgeTop")
    coe = m.get_array("CellsOnEdge")
    hh, uu, tt = rng.uniform(0.5, 40.0, (nc, K)), rng.uniform(-0.05, 0.05, (ne, K)), rng.uniform(-1e-5, 1e-5, (ne, K))
    bh, bu, bt, br = (oa.DeviceBuffer(a) for a in (hh, uu, tt, np.zeros((ne, K))))
    vp = C.c_void_p

    def get(name):
        o = np.zeros(shapes[name])
        assert L.omg_btr_copy_to_host(h, name.encode(), o.ctypes.data_as(C.POINTER(C.c_double)), C.c_size_t(o.size)) == 0
        return o

    assert L.omg_btr_split_velocity(h, None, vp(bu.ptr), 0, None) == 1 and "invalid argument" in _err()
    assert L.omg_btr_split_velocity(h, vp(bh.ptr), vp(bu.ptr), 0, None) == 0
    assert L.omg_btr_compute_ssh(h, None, None) == 1
    assert L.omg_btr_compute_ssh(h, vp(bh.ptr), None) == 0
    assert L.omg_btr_compute_forcing(h, vp(bh.ptr), None, None) == 1
    assert L.omg_btr_compute_forcing(h, vp(bh.ptr), vp(bt.ptr), None) == 0
    assert L.omg_btr_recombine(h, None, None) == 1
    assert L.omg_btr_recombine(h, vp(br.ptr), None) == 0
    oa.device_synchronize()
    thick, btr, bcl = get("BtrThickEdge"), get("BtrVelocity"), get("BclVelocity")
    w_thick, w_btr, w_bcl = thick.copy(), btr.copy(), bcl.copy()
    BR.split_velocity(hh, uu, coe, lo_e, hi_e, e_all, w_thick, w_btr, w_bcl)
    assert np.array_equal(thick, w_thick) and np.array_equal(btr, w_btr) and np.array_equal(bcl, w_bcl)
    bottom = vc.get("BottomDepth")
    ssh = get("SSH")
    assert np.array_equal(ssh[:n_all], BR.compute_ssh(hh, bottom, lo, hi, n_all, np.zeros(nc))[:n_all])
    forcing = get("BtrForcing")
    assert np.array_equal(forcing[:e_all], BR.compute_forcing(hh, tt, coe, lo_e, hi_e, e_all, np.zeros(ne))[:e_all])
    assert np.array_equal(br.to_host(), BR.recombine(np.zeros((ne, K)), btr, bcl, lo_e, hi_e, e_all))
    assert L.omg_btr_split_velocity(h, vp(bh.ptr), vp(bu.ptr), 1, None) == 0
    oa.device_synchronize()
    assert np.array_equal(get("SSH"), ssh) and np.array_equal(get("BclVelocity"), bcl)
    # subcycle
    assert L.omg_btr_subcycle(h, 0, C.c_double(10.0), None) == 1 and "NSub = 0" in _err()
    assert L.omg_btr_subcycle(h, 1, C.c_double(-1.0), None) == 1 and "DtBtr" in _err()
    assert L.omg_btr_subcycle(h, 3, C.c_double(10.0), None) == 0
    oa.device_synchronize()
    flux = get("BtrFluxMean")
    BR.subcycle(btr_mesh(m, bottom), ssh, btr, forcing, flux, 3, 10.0, GRAVITY)
    assert np.array_equal(get("SSH")[:n_all], ssh[:n_all]) and np.array_equal(get("BtrVelocity")[:e_all], btr[:e_all])
    assert np.array_equal(get("BtrFluxMean")[:e_all], flux[:e_all]) and np.abs(flux[:e_all]).max() > 0.0
    assert L.omg_btr_destroy(h) == 0
