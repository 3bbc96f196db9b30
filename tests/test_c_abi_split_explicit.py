"""The C entry points of the split-explicit step (include/omega_amd.h: omg_btr_compute_residual_forcing,
omg_btr_transport_velocity, omg_btr_advance_velocity, omg_stepper_attach_barotropic and the "Split-Explicit" type of
omg_stepper_create) called as a C program would: exported and declared, null handles are errors without a device; on a
device the three calls give the restatement's bits, BtrTendMean moves through the named-array triple, and one step made
through ctypes alone has the checksum of the Python binding's."""
import ctypes as C
import os

import numpy as np
import pytest

import omega_amd as oa
from tests import split_explicit_reference as SR
from tests.barotropic_fixtures import GRAVITY, btr_mesh
from tests.split_explicit_fixtures import StepRig

SYMBOLS = ("omg_btr_compute_residual_forcing", "omg_btr_transport_velocity", "omg_btr_advance_velocity",
           "omg_stepper_attach_barotropic")


_err = oa.last_error


def test_symbols_are_exported_and_declared():
    L = oa.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omega_amd.h")).read()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert f"int {s}(" in header, s
    assert '"Split-Explicit"' in header


def test_null_handles_are_errors():
    L = oa.lib()
    buf = (C.c_double * 4)()
    one = C.c_double(1.0)
    assert L.omg_btr_compute_residual_forcing(None, buf, buf, None) == 1 and "invalid argument" in _err()
    assert L.omg_btr_transport_velocity(None, buf, buf, None) == 1 and "invalid argument" in _err()
    assert L.omg_btr_advance_velocity(None, buf, buf, one, buf, None) == 1 and "invalid argument" in _err()
    assert L.omg_stepper_attach_barotropic(None, None, 1) == 1 and "invalid argument" in _err()
    p = C.POINTER(C.c_double)()
    assert L.omg_btr_device_ptr(None, b"BtrTendMean", C.byref(p), None) == 1 and "invalid argument" in _err()


@pytest.mark.gpu
def test_calls_and_a_step_on_a_device():
    oa.device_init(0)
    L = oa.lib()
    vp, dbl = C.c_void_p, C.c_double
    a, b = StepRig(), StepRig()
    p, m, K, h = a.p, a.p.mesh, a.K, a.bm.h
    ne, n_all, e_all = m.NEdgesSize, m.NCellsAll, m.NEdgesAll
    assert oa.level_pitch(K) == K

    def get(name, shape):
        o = np.zeros(shape)
        assert L.omg_btr_copy_to_host(h, name.encode(), o.ctypes.data_as(C.POINTER(C.c_double)), C.c_size_t(o.size)) == 0
        return o

    # the named-array triple of BtrTendMean
    ptr, cnt = C.POINTER(C.c_double)(), C.c_size_t()
    assert L.omg_btr_device_ptr(h, b"BtrTendMean", C.byref(ptr), C.byref(cnt)) == 0 and cnt.value == ne and ptr
    assert np.all(get("BtrTendMean", ne) == 0.0)  # zero at construction
    val = np.random.default_rng(2).uniform(-1.0, 1.0, ne)
    assert L.omg_btr_copy_to_device(h, b"BtrTendMean", val.ctypes.data_as(C.POINTER(C.c_double)), C.c_size_t(ne - 1)) == 1
    assert L.omg_btr_copy_to_device(h, b"BtrTendMean", val.ctypes.data_as(C.POINTER(C.c_double)), C.c_size_t(ne)) == 0
    assert np.array_equal(get("BtrTendMean", ne), val)
    # the three calls against the restatement
    rng = np.random.default_rng(6)
    tend = rng.uniform(-1.0e-5, 1.0e-5, (ne, K))
    bt, out = oa.DeviceBuffer(tend), oa.DeviceBuffer(np.zeros((ne, K)))
    hp, up = vp(p.state.device_ptr(0, 0)), vp(p.state.device_ptr(1, 0))
    assert L.omg_btr_split_velocity(h, hp, up, 1, None) == 0
    assert L.omg_btr_compute_residual_forcing(h, hp, None, None) == 1 and "invalid argument" in _err()
    assert L.omg_btr_compute_residual_forcing(h, hp, vp(bt.ptr), None) == 0
    oa.device_synchronize()
    lo_e, hi_e = a.vc.get("MinLayerEdgeBot"), a.vc.get("MaxLayerEdgeTop")
    M = btr_mesh(m, a.vc.get("BottomDepth"))
    ssh, vel, thick, bcl = get("SSH", m.NCellsSize), get("BtrVelocity", ne), get("BtrThickEdge", ne), get("BclVelocity", (ne, K))
    w_mean, w_forcing = np.zeros(ne), np.zeros(ne)
    SR.compute_residual_forcing(M, a.h, tend, lo_e, hi_e, ssh, vel, GRAVITY, w_mean, w_forcing)
    assert np.array_equal(get("BtrTendMean", ne)[:e_all], w_mean[:e_all]) and np.abs(w_mean).max() > 0.0
    assert np.array_equal(get("BtrForcing", ne)[:e_all], w_forcing[:e_all])
    assert L.omg_btr_subcycle(h, 3, dbl(5.0), None) == 0
    assert L.omg_btr_transport_velocity(h, up, None, None) == 1 and "invalid argument" in _err()
    assert L.omg_btr_transport_velocity(h, up, vp(out.ptr), None) == 0
    oa.device_synchronize()
    flux, vel = get("BtrFluxMean", ne), get("BtrVelocity", ne)
    want = SR.transport_velocity(a.u, np.zeros((ne, K)), bcl, flux, thick, lo_e, hi_e, e_all)
    assert np.array_equal(out.to_host(), want) and np.abs(flux).max() > 0.0
    assert L.omg_btr_advance_velocity(h, up, vp(bt.ptr), dbl(0.0), vp(out.ptr), None) == 1 and "advanceVelocity: Dt" in _err()
    assert L.omg_btr_advance_velocity(h, up, None, dbl(15.0), vp(out.ptr), None) == 1 and "invalid argument" in _err()
    assert L.omg_btr_advance_velocity(h, up, vp(bt.ptr), dbl(15.0), vp(out.ptr), None) == 0
    oa.device_synchronize()
    want = SR.advance_velocity(a.u, tend, 15.0, np.zeros((ne, K)), bcl, vel, w_mean, lo_e, hi_e, e_all)
    assert np.array_equal(out.to_host(), want)
    # one step through ctypes alone against the Python binding's
    st = vp()
    assert L.omg_stepper_create(b"Split-Explicit", dbl(20.0), p.tend.h, p.aux.h, m.h, None, p.tracers.h, C.byref(st)) == 0 and st
    assert L.omg_stepper_do_step(st, p.state.h, None) == 1 and "no BarotropicMode is attached" in _err()
    assert L.omg_stepper_attach_barotropic(st, None, 4) == 1 and "BarotropicMode is NULL" in _err()
    assert L.omg_stepper_attach_barotropic(st, h, 0) == 1 and "NSub = 0" in _err()
    rk = vp()
    assert L.omg_stepper_create(b"RungeKutta4", dbl(20.0), p.tend.h, p.aux.h, m.h, None, p.tracers.h, C.byref(rk)) == 0
    assert L.omg_stepper_attach_barotropic(rk, h, 4) == 1 and "not a Split-Explicit one" in _err()
    assert L.omg_stepper_destroy(rk) == 0
    assert L.omg_stepper_attach_barotropic(st, h, 4) == 0
    assert L.omg_stepper_do_step(st, p.state.h, None) == 0
    t = dbl()
    assert L.omg_stepper_get_time(st, C.byref(t)) == 0 and t.value == 20.0
    other = b.stepper("Split-Explicit", 20.0, 4)
    other.do_step(b.p.state)
    for got, want, start in zip(a.result(), b.result(), (a.h, a.u, a.tr)):
        assert np.isfinite(got).all() and got.sum() == want.sum() and np.array_equal(got, want)
        assert not np.array_equal(got, start)
    assert L.omg_stepper_destroy(st) == 0
