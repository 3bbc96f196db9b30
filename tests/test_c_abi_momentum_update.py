"""The C entry points of the momentum-only RHS and of the folded transport update (include/omega_amd.h:
omg_tend_compute_momentum, omg_tend_compute_transport_update, omg_update_tracers_by_tend, omg_stepper_set_momentum_rhs,
omg_stepper_set_folded_updates) called as a C program would: exported and declared with their signatures, null handles are
errors without a device.  A stepper cannot be made without a device, so the refusal of the two switches by the steppers
that are not Split-Explicit is the one test here that is marked gpu."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import omega_amd as oa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "omg_tend_compute_momentum": "omg_tend *t, const omg_state *s, omg_aux *a, const omg_tracers *tr, int tracer_time_level, "
                                 "int thick_time_level, int vel_time_level, void *stream",
    "omg_tend_compute_transport_update": "omg_tend *t, omg_state *s, omg_aux *a, omg_tracers *tr, int tracer_time_level, "
                                         "int thick_time_level, int vel_time_level, int next_thick_time_level, "
                                         "int next_tracer_time_level, double coeff, int keep_tendencies, void *stream",
    "omg_update_tracers_by_tend": "double *next_dev, const double *cur_dev, const double *h_next_dev, const double *h_cur_dev, "
                                  "const double *tend_dev, double coeff, int n_tracers, int n_rows, int rows_size, "
                                  "int row_length, void *stream",
    "omg_stepper_set_momentum_rhs": "omg_stepper *st, int on",
    "omg_stepper_set_folded_updates": "omg_stepper *st, int on",
}


_err = oa.last_error


def test_symbols_are_exported_and_declared_with_their_signatures():
    L = oa.lib()
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "omega_amd.h")).read())
    for name, params in SIGNATURES.items():
        assert hasattr(L, name), name
        assert f"int {name}({params});" in header, name
    for method in ("compute_momentum_tendencies", "compute_transport_tendencies_and_update"):
        assert hasattr(oa.Tendencies, method), method
    for method in ("set_momentum_rhs", "set_folded_updates"):
        assert hasattr(oa.TimeStepper, method), method
    assert hasattr(oa, "update_tracers_by_tend")


def test_null_handles_are_errors():
    L = oa.lib()
    dbl = C.c_double
    assert L.omg_tend_compute_momentum(None, None, None, None, 0, 0, 0, None) == 1 and "invalid argument" in _err()
    assert (L.omg_tend_compute_transport_update(None, None, None, None, 0, 0, 1, 1, 1, dbl(1.0), 1, None) == 1
            and "invalid argument" in _err())
    assert L.omg_update_tracers_by_tend(None, None, None, None, None, dbl(1.0), 1, 1, 1, 1, None) == 1 and "invalid argument" in _err()
    assert L.omg_stepper_set_momentum_rhs(None, 1) == 1 and "invalid argument" in _err()
    assert L.omg_stepper_set_folded_updates(None, 1) == 1 and "invalid argument" in _err()


@pytest.mark.gpu
def test_the_switches_are_for_split_explicit_only():
    from tests.split_explicit_fixtures import StepRig
    oa.device_init(0)
    L = oa.lib()
    x = StepRig(attached=False)
    p = x.p
    for kind in ("RungeKutta4", "RungeKutta2", "Forward-Backward"):
        st = x.stepper(kind, 20.0)
        for setter in (st.set_momentum_rhs, st.set_folded_updates):
            for on in (False, True):
                with pytest.raises(oa.OmegaAmdError, match="not a Split-Explicit one"):
                    setter(on)
        assert L.omg_stepper_set_momentum_rhs(st.h, 1) == 1 and "not a Split-Explicit one" in _err()
        assert L.omg_stepper_set_folded_updates(st.h, 0) == 1 and "not a Split-Explicit one" in _err()
    se = x.stepper("Split-Explicit", 20.0, 3)
    for on in (False, True):
        se.set_momentum_rhs(on)
        se.set_folded_updates(on)
    # one handle missing at a time, then a call through ctypes alone
    t, s, a, tr = p.tend.h, p.state.h, p.aux.h, p.tracers.h
    assert L.omg_tend_compute_momentum(t, None, a, tr, 0, 0, 0, None) == 1 and "invalid argument" in _err()
    assert L.omg_tend_compute_momentum(t, s, a, None, 0, 0, 0, None) == 1 and "tracers handle is NULL" in _err()
    assert L.omg_tend_compute_transport_update(t, s, None, tr, 0, 0, 0, 1, 1, C.c_double(1.0), 1, None) == 1 and "invalid argument" in _err()
    assert L.omg_tend_compute_momentum(t, s, a, tr, 0, 0, 0, None) == 0
    assert L.omg_tend_compute_transport_update(t, s, a, tr, 0, 0, 0, 1, 1, C.c_double(20.0), 0, None) == 0
    se.do_step(p.state)
    assert all(np.isfinite(r).all() for r in x.result())
