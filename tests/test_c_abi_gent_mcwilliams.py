"""The C entry points of GentMcWilliams (include/omega_amd.h: omg_gm_*, omg_stepper_attach_gm) called as a C program
would: return codes and messages for null handles, bad parameters, a host-only mesh and unknown array names without a
device; on a device the handle's lifetime, the named-array triple and the three calls against the restatement."""
import ctypes as C
import os

import numpy as np
import pytest

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests import gent_mcwilliams_reference as GR

SYMBOLS = ("omg_gm_create", "omg_gm_destroy", "omg_gm_update_column", "omg_gm_compute", "omg_gm_compute_arrays",
           "omg_gm_device_ptr", "omg_gm_copy_to_device", "omg_gm_copy_to_host", "omg_stepper_attach_gm")
NAMES = (b"Kappa", b"BolusVelocity", b"StreamFunction", b"SurfacePressure", b"TidalPotential", b"SelfAttractionLoading")
D = C.c_double


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
    p = C.POINTER(C.c_double)()
    assert L.omg_gm_update_column(None, buf, buf, 2, None) == 1 and "invalid argument" in _err()
    assert L.omg_gm_compute(None, buf, None, None) == 1 and "invalid argument" in _err()
    assert L.omg_gm_compute_arrays(None, buf, buf, buf, buf, None, None) == 1 and "invalid argument" in _err()
    for name in NAMES:
        assert L.omg_gm_device_ptr(None, name, C.byref(p), None) == 1 and "invalid argument" in _err()
        assert L.omg_gm_copy_to_host(None, name, buf, C.c_size_t(4)) == 1
        assert L.omg_gm_copy_to_device(None, name, buf, C.c_size_t(4)) == 1
    assert L.omg_stepper_attach_gm(None, None) == 1 and "invalid argument" in _err()
    assert L.omg_gm_destroy(None) == 0
    h = C.c_void_p()
    assert L.omg_gm_create(None, None, None, D(600.0), D(0.3), C.byref(h)) == 1 and "invalid argument" in _err() and not h
    d = oa.Decomp(oa.GlobalMesh(planar_hex(8, 8, 1.0)), 1, 0, 3)
    m = oa.HorzMesh(d, 4, host_only=True)
    assert L.omg_gm_create(m.h, None, None, D(600.0), D(0.3), None) == 1 and "invalid argument" in _err()
    assert L.omg_gm_create(m.h, None, None, D(600.0), D(0.3), C.byref(h)) == 1 and "host-only" in _err() and not h
    for kappa in (-1.0e-300, float("nan"), float("inf")):
        assert L.omg_gm_create(m.h, None, None, D(kappa), D(0.3), C.byref(h)) == 1 and "GMKappa" in _err() and not h
    for speed in (0.0, -1.0, float("nan"), float("inf")):
        assert L.omg_gm_create(m.h, None, None, D(600.0), D(speed), C.byref(h)) == 1 and "GravWaveSpeed" in _err()
        assert not h


@pytest.mark.gpu
def test_calls_on_a_device():
    oa.device_init(0)
    L = oa.lib()
    K, nt = 6, 2
    d = oa.Decomp(oa.GlobalMesh(planar_hex(8, 8, 30.0e3)), 1, 0, 3)
    m = oa.HorzMesh(d, K)
    vc = oa.VertCoord(m, K, 1026.0, "Uniform", decomp=d)
    eos = oa.Eos(m, K, "linear")
    nc, ne, e_all = m.NCellsSize, m.NEdgesSize, m.NEdgesAll
    h = C.c_void_p()
    assert L.omg_gm_create(m.h, None, eos.h, D(600.0), D(0.3), C.byref(h)) == 1 and "VertCoord is NULL" in _err() and not h
    assert L.omg_gm_create(m.h, vc.h, None, D(600.0), D(0.3), C.byref(h)) == 1 and "Eos is NULL" in _err() and not h
    m2 = oa.HorzMesh(d, K)
    vc2, eos2 = oa.VertCoord(m2, K, 1026.0, "Uniform", decomp=d), oa.Eos(m2, K, "linear")
    assert L.omg_gm_create(m.h, vc2.h, eos.h, D(600.0), D(0.3), C.byref(h)) == 1 and "another mesh" in _err() and not h
    assert L.omg_gm_create(m.h, vc.h, eos2.h, D(600.0), D(0.3), C.byref(h)) == 1 and "another mesh" in _err() and not h
    eos3 = oa.Eos(m, K - 1, "linear")
    assert L.omg_gm_create(m.h, vc.h, eos3.h, D(600.0), D(0.3), C.byref(h)) == 1 and "layer counts" in _err() and not h
    assert L.omg_gm_create(m.h, vc.h, eos.h, D(250.0), D(0.5), C.byref(h)) == 0 and h
    # the named-array triple
    p, cnt = C.POINTER(C.c_double)(), C.c_size_t()
    sizes = {b"Kappa": ne, b"BolusVelocity": ne * K, b"StreamFunction": ne * K, b"SurfacePressure": nc,
             b"TidalPotential": nc, b"SelfAttractionLoading": nc}
    for name in NAMES:
        assert L.omg_gm_device_ptr(h, name, C.byref(p), C.byref(cnt)) == 0 and cnt.value == sizes[name] and p
        out = np.ones(sizes[name])
        pd = out.ctypes.data_as(C.POINTER(C.c_double))
        assert L.omg_gm_copy_to_host(h, name, pd, C.c_size_t(out.size - 1)) == 1 and "too small" in _err()
        assert L.omg_gm_copy_to_device(h, name, pd, C.c_size_t(out.size - 1)) == 1 and "size mismatch" in _err()
        assert L.omg_gm_copy_to_host(h, name, pd, C.c_size_t(out.size)) == 0
        assert np.all(out == (250.0 if name == b"Kappa" else 0.0))  # the initial values
    assert L.omg_gm_device_ptr(h, b"NoSuchArray", C.byref(p), None) == 1
    assert "GentMcWilliams: no array named NoSuchArray" in _err()
    assert L.omg_gm_copy_to_host(h, b"NoSuchArray", pd, C.c_size_t(4)) == 1
    assert L.omg_gm_copy_to_device(h, b"NoSuchArray", pd, C.c_size_t(4)) == 1
    rng = np.random.default_rng(5)
    kappa = rng.uniform(100.0, 900.0, ne)
    assert L.omg_gm_copy_to_device(h, b"Kappa", kappa.ctypes.data_as(C.POINTER(C.c_double)), C.c_size_t(ne)) == 0
    # the three calls against the restatement (K = 6: compact rows, no padding)
    assert oa.level_pitch(K) == K
    hh = rng.uniform(5.0, 40.0, (nc, K))
    tr = np.stack([rng.uniform(2.0, 20.0, (nc, K)), rng.uniform(33.0, 36.0, (nc, K))])
    tt = rng.uniform(-0.1, 0.1, (ne, K))
    bh, btr, bt, bt2 = (oa.DeviceBuffer(a) for a in (hh, tr, tt, tt))
    vp = C.c_void_p
    assert L.omg_gm_update_column(h, vp(bh.ptr), vp(btr.ptr), 1, None) == 1 and "invalid argument" in _err()
    assert L.omg_gm_update_column(h, None, vp(btr.ptr), nt, None) == 1
    assert L.omg_gm_update_column(h, vp(bh.ptr), vp(btr.ptr), nt, None) == 0
    assert L.omg_gm_compute(h, None, None, None) == 1 and "invalid argument" in _err()
    assert L.omg_gm_compute(h, vp(bh.ptr), vp(bt.ptr), None) == 0
    oa.device_synchronize()
    sv, svd, zm = eos.get("SpecVol"), eos.get("SpecVolDisplaced"), vc.get("ZMid")
    lo, hi = vc.get("MinLayerEdgeBot"), vc.get("MaxLayerEdgeTop")
    want_t = tt.copy()
    want_u, want_psi, _ = GR.bolus_velocity(hh, sv, svd, zm, m.get_array("CellsOnEdge"), m.get_array("DcEdge"), kappa, lo,
                                            hi, e_all, 1026.0, 0.5, np.zeros((ne, K)), np.zeros((ne, K)), want_t)
    got_u, got_psi = np.empty((ne, K)), np.empty((ne, K))
    for name, out in ((b"BolusVelocity", got_u), (b"StreamFunction", got_psi)):
        assert L.omg_gm_copy_to_host(h, name, out.ctypes.data_as(C.POINTER(C.c_double)), C.c_size_t(out.size)) == 0
    assert np.array_equal(got_u, want_u) and np.array_equal(got_psi, want_psi) and np.abs(want_u).max() > 0.0
    assert np.array_equal(bt.to_host(), want_t)
    bsv, bsvd, bzm = (oa.DeviceBuffer(a) for a in (sv, svd, zm))
    assert L.omg_gm_compute_arrays(h, vp(bh.ptr), vp(bsv.ptr), None, vp(bzm.ptr), None, None) == 1
    assert L.omg_gm_compute_arrays(h, vp(bh.ptr), vp(bsv.ptr), vp(bsvd.ptr), vp(bzm.ptr), vp(bt2.ptr), None) == 0
    oa.device_synchronize()
    assert np.array_equal(bt2.to_host(), want_t)
    # attach / detach
    aux = oa.AuxiliaryState(m, None, K, nt)
    state, tracers = oa.OceanState(m, None, K, 2), oa.Tracers(m, None, K, nt, 2)
    tend = oa.Tendencies(m, K, nt)
    rk = oa.TimeStepper("RungeKutta4", 60.0, tend, aux, m, None, tracers)
    assert L.omg_stepper_attach_gm(rk.h, h) == 1 and "Split-Explicit" in _err()
    se = oa.TimeStepper("Split-Explicit", 60.0, tend, aux, m, None, tracers)
    assert L.omg_stepper_attach_gm(se.h, h) == 0
    assert L.omg_stepper_attach_gm(se.h, None) == 0
    del state
    assert L.omg_gm_destroy(h) == 0
