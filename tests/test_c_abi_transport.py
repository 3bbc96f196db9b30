"""The C entry points of the fused transport evaluation (include/omega_amd.h: omg_tend_compute_transport,
omg_stepper_set_fused_transport) called as a C program would: exported and declared, null handles are errors without a
device; on a device a call through ctypes alone gives the bits of the two group calls, bad time levels return the error
code with omg_last_error() set, and the stepper switch is refused for a stepper that is not Split-Explicit."""
import ctypes as C
import os

import numpy as np
import pytest

import omega_amd as oa
from tests.split_explicit_fixtures import StepRig

SYMBOLS = ("omg_tend_compute_transport", "omg_stepper_set_fused_transport")


_err = oa.last_error


def test_symbols_are_exported_and_declared():
    L = oa.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omega_amd.h")).read()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert f"int {s}(" in header, s
    assert hasattr(oa.Tendencies, "compute_transport_tendencies") and hasattr(oa.TimeStepper, "set_fused_transport")


def test_null_handles_are_errors():
    L = oa.lib()
    assert L.omg_tend_compute_transport(None, None, None, None, 0, 0, 0, None) == 1 and "invalid argument" in _err()
    assert L.omg_stepper_set_fused_transport(None, 1) == 1 and "invalid argument" in _err()


@pytest.mark.gpu
def test_round_trip_and_refusals_on_a_device():
    oa.device_init(0)
    L = oa.lib()
    x = StepRig(attached=False)
    p, m = x.p, x.p.mesh
    t, s, a, tr = p.tend.h, p.state.h, p.aux.h, p.tracers.h
    p.state.copy_to_device(x.h, -x.u, 1)
    # handles missing one at a time
    assert L.omg_tend_compute_transport(None, s, a, tr, 0, 0, 1, None) == 1 and "invalid argument" in _err()
    assert L.omg_tend_compute_transport(t, None, a, tr, 0, 0, 1, None) == 1 and "invalid argument" in _err()
    assert L.omg_tend_compute_transport(t, s, None, tr, 0, 0, 1, None) == 1 and "invalid argument" in _err()
    assert L.omg_tend_compute_transport(t, s, a, None, 0, 0, 1, None) == 1 and "tracers handle is NULL" in _err()
    # bad time levels
    assert L.omg_tend_compute_transport(t, s, a, tr, 0, 2, 0, None) == 1 and "bad time level" in _err()
    assert L.omg_tend_compute_transport(t, s, a, tr, 0, 0, -1, None) == 1 and "bad time level" in _err()
    assert L.omg_tend_compute_transport(t, s, a, tr, 2, 0, 0, None) == 1 and "time level out of range" in _err()
    # the call against the two group calls
    assert L.omg_tend_compute_thickness(t, s, a, 0, 1, None) == 0
    assert L.omg_tend_compute_tracer(t, s, a, tr, 0, 0, 1, None) == 0
    oa.device_synchronize()
    n = m.NCellsAll
    want = p.tend.get(0)[:n].copy(), p.tend.get(2)[:, :n].copy()
    for which, rows, planes in ((0, m.NCellsSize, 1), (2, m.NCellsSize, x.nt)):
        oa.copy_to_device(p.tend.device_ptr(which)[0], np.zeros((planes, rows, oa.level_pitch(x.K))))
    assert L.omg_tend_compute_transport(t, s, a, tr, 0, 0, 1, None) == 0
    oa.device_synchronize()
    got = p.tend.get(0)[:n], p.tend.get(2)[:, :n]
    for g, w in zip(got, want):
        assert np.isfinite(w).all() and np.abs(w).max() > 0.0
        assert np.array_equal(g.view(np.uint64), w.view(np.uint64))
    # the stepper switch
    vp, dbl = C.c_void_p, C.c_double
    rk, se = vp(), vp()
    assert L.omg_stepper_create(b"RungeKutta4", dbl(20.0), t, a, m.h, None, tr, C.byref(rk)) == 0
    assert L.omg_stepper_set_fused_transport(rk, 1) == 1 and "not a Split-Explicit one" in _err()
    assert L.omg_stepper_destroy(rk) == 0
    assert L.omg_stepper_create(b"Split-Explicit", dbl(20.0), t, a, m.h, None, tr, C.byref(se)) == 0
    assert L.omg_stepper_set_fused_transport(se, 0) == 0 and L.omg_stepper_set_fused_transport(se, 1) == 0
    assert L.omg_stepper_attach_barotropic(se, x.bm.h, 3) == 0
    assert L.omg_stepper_do_step(se, s, None) == 0
    oa.device_synchronize()
    assert all(np.isfinite(r).all() for r in x.result())
    assert L.omg_stepper_destroy(se) == 0
