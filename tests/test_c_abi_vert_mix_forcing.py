"""The C entry points of the forced solves, VertMixStep and the stepper hook (include/omega_amd.h) called as a C program
would, without a device: the symbols are exported and declared; null handles, a host-only mesh, NTracers = 1 and a
negative coefficient return 1 with a message naming the cause."""
import ctypes as C
import os

import omega_amd as oa
from omega_amd.meshgen import planar_hex

SYMBOLS = ("omg_vertmix_apply_tracers_forced", "omg_vertmix_apply_velocity_forced", "omg_vertmix_step_create",
           "omg_vertmix_step_destroy", "omg_vertmix_step_apply", "omg_vertmix_step_apply_state",
           "omg_vertmix_step_set_boundary", "omg_vertmix_step_copy_to_host", "omg_vertmix_step_copy_to_device",
           "omg_vertmix_step_device_ptr", "omg_stepper_attach_vert_mix")


_err = oa.last_error


def test_symbols_are_exported_and_declared():
    L = oa.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omega_amd.h")).read()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert f"int {s}(" in header, s
    assert "typedef struct omg_vertmix_step omg_vertmix_step;" in header


def test_null_handles_are_errors():
    L = oa.lib()
    buf = (C.c_double * 4)()
    p = C.POINTER(C.c_double)()
    d = C.c_double
    assert L.omg_vertmix_apply_tracers_forced(None, buf, buf, 1, d(1.0), buf, None) == 1 and "invalid argument" in _err()
    assert L.omg_vertmix_apply_velocity_forced(None, buf, buf, d(1.0), d(0.0), d(0.0), None, None, None) == 1
    assert "invalid argument" in _err()
    assert L.omg_vertmix_step_apply(None, buf, buf, buf, d(1.0), None) == 1 and "invalid argument" in _err()
    assert L.omg_vertmix_step_apply_state(None, None, 0, None, 0, d(1.0), None) == 1 and "invalid argument" in _err()
    assert L.omg_vertmix_step_set_boundary(None, d(0.0), d(0.0), 0) == 1 and "invalid argument" in _err()
    assert L.omg_vertmix_step_device_ptr(None, b"NormalStressEdge", C.byref(p), None) == 1 and "invalid argument" in _err()
    assert L.omg_vertmix_step_copy_to_host(None, b"NormalStressEdge", buf, C.c_size_t(4)) == 1
    assert L.omg_vertmix_step_copy_to_device(None, b"NormalStressEdge", buf, C.c_size_t(4)) == 1
    assert L.omg_stepper_attach_vert_mix(None, None) == 1 and "invalid argument" in _err()
    assert L.omg_vertmix_step_destroy(None) == 0
    h = C.c_void_p()
    assert L.omg_vertmix_step_create(None, None, None, None, 2, C.byref(h)) == 1 and "invalid argument" in _err()
    assert not h


def test_host_only_mesh_one_tracer_and_negative_coefficients_are_refused():
    L = oa.lib()
    d = C.c_double
    dec = oa.Decomp(oa.GlobalMesh(planar_hex(8, 8, 1.0)), 1, 0, 3)
    m = oa.HorzMesh(dec, 4, host_only=True)
    h = C.c_void_p()
    assert L.omg_vertmix_step_create(m.h, None, None, None, 2, C.byref(h)) == 1 and "host-only" in _err() and not h
    assert L.omg_vertmix_step_create(m.h, None, None, None, 1, C.byref(h)) == 1 and "NTracers = 1" in _err() and not h
    buf = (C.c_double * 4)()
    assert L.omg_vertmix_apply_velocity_forced(None, buf, buf, d(1.0), d(-1.0e-3), d(0.0), None, None, None) == 1
    assert "BottomDragCoeff" in _err() and "negative" in _err()
    assert L.omg_vertmix_apply_velocity_forced(None, buf, buf, d(1.0), d(0.0), d(-1.0e-5), None, None, None) == 1
    assert "RayleighDragCoeff" in _err() and "negative" in _err()
