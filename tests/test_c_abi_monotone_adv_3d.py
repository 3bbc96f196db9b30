"""The C entry points of the 3-D form of MonotoneAdv (include/omega_amd.h: omg_monoadv_attach_vert_adv,
omg_vertadv_set_tracer_term) called as a C program would: null handles without a device; on a device the attachment, its
refusal, NULL detaching, the switch, and the stepper's refusals as omg_stepper_attach_monotone_adv documents them."""
import ctypes as C
import os

import numpy as np
import pytest

import omega_amd as oa
from tests.column_reference import RHO0
from tests.monotone_adv_fixtures import Mono3Rig
from tests.split_explicit_fixtures import StepRig

SYMBOLS = ("omg_monoadv_attach_vert_adv", "omg_vertadv_set_tracer_term")


_err = oa.last_error


def test_symbols_are_exported_and_declared():
    L = oa.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omega_amd.h")).read()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert f"int {s}(" in header, s
    assert "omg_vertadv_set_tracer_term" in header.split("int omg_stepper_attach_monotone_adv(")[0].rsplit("/*", 1)[1]


def test_null_handles_are_errors():
    L = oa.lib()
    assert L.omg_monoadv_attach_vert_adv(None, None) == 1 and "invalid argument" in _err()
    assert L.omg_vertadv_set_tracer_term(None, 0) == 1 and "invalid argument" in _err()


@pytest.mark.gpu
def test_calls_on_a_device():
    oa.device_init(0)
    L = oa.lib()
    K, nt = 6, 2
    assert oa.level_pitch(K) == K  # compact rows, no padding
    R = Mono3Rig("hex24x20", K, device=True)
    I = R.inputs(seed=4, ntracers=3, check=False)
    m, nc, n = R.mesh, R.nc_size, R.nc
    vc = oa.VertCoord(m, K, RHO0, "Uniform", R.min_level, R.max_level, decomp=R.decomp)
    va = oa.VertAdv(m, vc, 2)
    oa.copy_to_device(va.device_ptr("VerticalTransport"), I.wt)
    mono = oa.MonotoneAdv(m, K, nt)
    tend0 = np.random.default_rng(1).uniform(-1.0e-3, 1.0e-3, (nt, nc, K))
    bho, bhn, bu, btr = (oa.DeviceBuffer(a) for a in (I.h_old, I.h_new, I.u, I.tracers))
    vp, dt = C.c_void_p, C.c_double(I.dt)

    def call():
        bt = oa.DeviceBuffer(tend0)
        assert L.omg_monoadv_add_tracers(mono.h, vp(bt.ptr), vp(bho.ptr), vp(bhn.ptr), vp(bu.ptr), vp(btr.ptr), nt, dt,
                                         None) == 0
        oa.device_synchronize()
        return bt.to_host(), mono.get("ScaleIn"), mono.get("ScaleOut")

    flat = call()
    assert all(np.array_equal(a[:, :n], b[:, :n]) for a, b in zip(flat, R.reference_2d(I, nt, tend0)))
    # a VertAdv of another layer count
    other = oa.HorzMesh(R.decomp, K + 1)
    va_other = oa.VertAdv(other, oa.VertCoord(other, K + 1, RHO0, "Uniform", decomp=R.decomp), 2)
    assert L.omg_monoadv_attach_vert_adv(mono.h, va_other.h) == 1
    assert "MonotoneAdv::attachVertAdv: the VertAdv was built for another mesh or layer count" in _err()
    assert all(np.array_equal(a, b) for a, b in zip(call(), flat))  # nothing was attached
    # attached: the 3-D restatement; NULL: the 2-D bits again
    assert L.omg_monoadv_attach_vert_adv(mono.h, va.h) == 0
    deep = call()
    want = R.reference(I, nt, tend0)
    for a, b in zip(deep, want):
        assert np.isfinite(b[:, :n]).all() and np.array_equal(a[:, :n], b[:, :n])
    assert np.array_equal(deep[0][:, n:], tend0[:, n:]) and not np.array_equal(deep[0], flat[0])
    assert L.omg_monoadv_attach_vert_adv(mono.h, None) == 0
    assert all(np.array_equal(a, b) for a, b in zip(call(), flat))
    # the switch and the stepper's refusals
    x = StepRig(K=K, config=dict(TracerHorzAdvTendencyEnable=0))
    st = x.stepper("Split-Explicit", 20.0, 2)
    m2 = oa.MonotoneAdv(x.p.mesh, K, x.nt)
    foreign = oa.VertAdv(x.p.mesh, x.vc, 2)
    assert L.omg_vertadv_set_tracer_term(foreign.h, 0) == 0
    assert L.omg_monoadv_attach_vert_adv(m2.h, foreign.h) == 0
    assert L.omg_stepper_attach_monotone_adv(st.h, m2.h) == 1 and "is not the one attached to the Tendencies" in _err()
    assert L.omg_monoadv_attach_vert_adv(m2.h, x.va.h) == 0
    assert L.omg_stepper_attach_monotone_adv(st.h, m2.h) == 1 and "TracerTermEnable is on" in _err()
    assert L.omg_vertadv_set_tracer_term(x.va.h, 0) == 0
    assert L.omg_stepper_attach_monotone_adv(st.h, m2.h) == 0
    st.do_step(x.p.state)
    oa.device_synchronize()
    assert all(np.isfinite(a).all() for a in x.result())
    assert L.omg_vertadv_set_tracer_term(x.va.h, 7) == 0  # any non-zero value: on
    assert L.omg_stepper_do_step(st.h, x.p.state.h, None) == 1 and "doStep: the VertAdv's TracerTermEnable is on" in _err()
    assert L.omg_stepper_attach_monotone_adv(st.h, None) == 0
    assert L.omg_monoadv_attach_vert_adv(m2.h, None) == 0
