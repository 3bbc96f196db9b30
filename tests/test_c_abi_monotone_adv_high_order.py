"""The C entry points of the high-order horizontal flux of MonotoneAdv (include/omega_amd.h:
omg_monoadv_set_horz_order, omg_monoadv_high_order_tables, omg_monoadv_launch_count and the five named arrays) called as
a C program would: null handles and the refusals of the configuration without a device (the table builder works on a
host-only mesh); on a device the setter, the named arrays and their shapes, the refusals, and one call that gives the
restatement's bits."""
import ctypes as C
import os

import numpy as np
import pytest

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests import monotone_adv_reference as MR
from tests.monotone_adv_fixtures import HoRig

SYMBOLS = ("omg_monoadv_set_horz_order", "omg_monoadv_high_order_tables", "omg_monoadv_launch_count")
ARRAYS = (b"Hess", b"HessWeight", b"EdgeDirOwn", b"EdgeDirAcross", b"FitCell")


_err = oa.last_error


def _d(x):
    return C.c_double(x)


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_symbols_are_exported_and_declared():
    L = oa.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omega_amd.h")).read()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert f"int {s}(" in header, s
    doc = header.split("int omg_monoadv_device_ptr(")[0].rsplit("/*", 1)[1]
    for name in ARRAYS:
        assert f'"{name.decode()}"' in doc, name


def test_null_handles_and_the_refusals_without_a_device():
    L = oa.lib()
    n = C.c_int64(-1)
    assert L.omg_monoadv_set_horz_order(None, 4, _d(0.25), _d(0.0), _d(0.0), _d(0.0)) == 1 and "invalid argument" in _err()
    assert L.omg_monoadv_launch_count(None, C.byref(n)) == 1 and "invalid argument" in _err() and n.value == -1
    g = planar_hex(8, 8, 1.0)
    m = oa.HorzMesh(oa.Decomp(oa.GlobalMesh(g), 1, 0, 3), 2, host_only=True)
    nc, me = m.NCellsSize, m.MaxEdges
    fit, w, own, acr = np.zeros(nc), np.zeros((nc, me, 3)), np.zeros((nc, me, 3)), np.zeros((nc, me, 3))
    per = (_d(g["x_period"]), _d(g["y_period"]))
    out = (_p(fit), _p(w), _p(own), _p(acr))
    assert L.omg_monoadv_high_order_tables(None, 4, _d(0.25), _d(0.0), *per, *out) == 1 and "invalid argument" in _err()
    assert L.omg_monoadv_high_order_tables(m.h, 4, _d(0.25), _d(0.0), *per, None, *out[1:]) == 1
    for order in (1, 5):
        assert L.omg_monoadv_high_order_tables(m.h, order, _d(0.25), _d(0.0), *per, *out) == 1
        assert "is not 2, 3 or 4" in _err()
    for coef in (0.0, 1.25, float("nan")):
        assert L.omg_monoadv_high_order_tables(m.h, 3, _d(coef), _d(0.0), *per, *out) == 1 and "outside (0, 1]" in _err()
    for bad in (-1.0, float("inf"), float("nan")):
        assert L.omg_monoadv_high_order_tables(m.h, 4, _d(0.25), _d(bad), *per, *out) == 1
        assert "negative or not finite" in _err()
        assert L.omg_monoadv_high_order_tables(m.h, 4, _d(0.25), _d(0.0), _d(bad), per[1], *out) == 1
        assert L.omg_monoadv_high_order_tables(m.h, 4, _d(0.25), _d(0.0), per[0], _d(bad), *out) == 1
    assert not fit.any() and not w.any()  # a refused call wrote nothing
    assert L.omg_monoadv_high_order_tables(m.h, 2, _d(0.25), _d(0.0), *per, *out) == 0 and not fit.any()
    assert L.omg_monoadv_high_order_tables(m.h, 4, _d(0.25), _d(0.0), *per, *out) == 0
    n_all = m.NCellsAll
    assert fit[:n_all].all() and not fit[n_all:].any() and w[:n_all, :6].any() and np.array_equal(own != 0.0, acr != 0.0)


@pytest.mark.gpu
def test_calls_on_a_device():
    oa.device_init(0)
    L = oa.lib()
    K, nt, maxt = 6, 2, 3
    assert oa.level_pitch(K) == K  # compact rows, no padding
    R = HoRig("fib700_coast_ragged", K, device=True).set_order(3, 0.5)
    I = R.inputs(seed=4, ntracers=3, check=False)
    m, nc, n, me = R.mesh, R.nc_size, R.nc, R.mesh.MaxEdges
    geo = MR.geometry(R.g)
    geo_args = (_d(geo["sphere_radius"]), _d(geo["x_period"]), _d(geo["y_period"]))
    h = C.c_void_p()
    assert L.omg_monoadv_create(m.h, K, maxt, 0, C.byref(h)) == 0 and h
    p, cnt, count = C.POINTER(C.c_double)(), C.c_size_t(), C.c_int64(-1)
    for name in ARRAYS:  # they exist after the setter only
        assert L.omg_monoadv_device_ptr(h, name, C.byref(p), C.byref(cnt)) == 1 and "after setHorzOrder" in _err()
    # the refusals
    for order in (1, 5, -2):
        assert L.omg_monoadv_set_horz_order(h, order, _d(0.25), *geo_args) == 1 and "is not 2, 3 or 4" in _err()
    for coef in (0.0, 1.25, float("nan")):
        assert L.omg_monoadv_set_horz_order(h, 3, _d(coef), *geo_args) == 1 and "outside (0, 1]" in _err()
    for bad in (-1.0, float("inf"), float("nan")):
        for k in range(3):
            a = list(geo_args)
            a[k] = _d(bad)
            assert L.omg_monoadv_set_horz_order(h, 4, _d(0.25), *a) == 1 and "negative or not finite" in _err()
    assert L.omg_monoadv_device_ptr(h, b"Hess", C.byref(p), None) == 1  # a refused call configured nothing
    assert L.omg_monoadv_set_horz_order(h, 2, _d(0.25), *geo_args) == 0
    assert L.omg_monoadv_device_ptr(h, b"Hess", C.byref(p), None) == 1  # nor did order 2
    # the setter, the five named arrays and their shapes
    assert L.omg_monoadv_set_horz_order(h, 3, _d(0.5), *geo_args) == 0
    sizes = {b"Hess": maxt * 3 * nc * K, b"HessWeight": nc * me * 3, b"EdgeDirOwn": nc * me * 3,
             b"EdgeDirAcross": nc * me * 3, b"FitCell": nc}
    for name in ARRAYS:
        assert L.omg_monoadv_device_ptr(h, name, C.byref(p), C.byref(cnt)) == 0 and cnt.value == sizes[name], name
    for name, want in ((b"FitCell", R.H.fit.astype(float)), (b"HessWeight", R.H.weight), (b"EdgeDirOwn", R.H.own),
                       (b"EdgeDirAcross", R.H.across)):
        out = np.full(want.shape, -1.0)
        assert L.omg_monoadv_copy_to_host(h, name, _p(out), C.c_size_t(out.size - 1)) == 1 and "too small" in _err()
        assert L.omg_monoadv_copy_to_host(h, name, _p(out), C.c_size_t(out.size)) == 0
        assert np.array_equal(out, want), name
    hess = np.full((maxt, 3, nc, K), np.nan)
    assert L.omg_monoadv_copy_to_device(h, b"Hess", _p(hess), C.c_size_t(hess.size - 1)) == 1 and "size mismatch" in _err()
    assert L.omg_monoadv_copy_to_device(h, b"Hess", _p(hess), C.c_size_t(hess.size)) == 0
    # one call against the restatement: three launches
    tend0 = np.random.default_rng(1).uniform(-1.0e-3, 1.0e-3, (nt, nc, K))
    bt, bho, bhn, bu, btr = (oa.DeviceBuffer(a) for a in (tend0, I.h_old, I.h_new, I.u, I.tracers))
    vp = C.c_void_p
    args = (vp(bt.ptr), vp(bho.ptr), vp(bhn.ptr), vp(bu.ptr), vp(btr.ptr))
    assert L.omg_monoadv_launch_count(h, C.byref(count)) == 0 and count.value == 0
    assert L.omg_monoadv_add_tracers(h, *args, nt, _d(I.dt), None) == 0
    oa.device_synchronize()
    assert L.omg_monoadv_launch_count(h, C.byref(count)) == 0 and count.value == 3
    want, si, so, hs = R.reference_ho(I, nt, tend0, max_tracers=maxt)
    assert np.array_equal(bt.to_host()[:, :n], want[:, :n]) and np.array_equal(bt.to_host()[:, n:], tend0[:, n:])
    out = np.ones((maxt, nc, K))
    for name, ref in ((b"ScaleIn", si), (b"ScaleOut", so)):
        assert L.omg_monoadv_copy_to_host(h, name, _p(out), C.c_size_t(out.size)) == 0
        assert np.array_equal(out, ref) and (ref[:nt, :n] < 1.0).any()
    assert L.omg_monoadv_copy_to_host(h, b"Hess", _p(hess), C.c_size_t(hess.size)) == 0
    assert np.array_equal(hess[:nt, :, :n], hs[:nt, :, :n]) and np.isnan(hess[nt:]).all() and np.isnan(hess[:, :, n:]).all()
    assert hess[:nt, :, :n].any() and not hess[:nt, :, :n][:, :, ~R.H.fit[:n]].any()
    # order 2 again: two launches and the centred form's bits
    assert L.omg_monoadv_set_horz_order(h, 2, _d(0.25), *geo_args) == 0
    oa.copy_to_device(bt.ptr, tend0)
    assert L.omg_monoadv_add_tracers(h, *args, nt, _d(I.dt), None) == 0
    oa.device_synchronize()
    assert L.omg_monoadv_launch_count(h, C.byref(count)) == 0 and count.value == 5
    want2 = R.reference(I, nt, tend0, max_tracers=maxt)[0]
    assert np.array_equal(bt.to_host()[:, :n], want2[:, :n]) and not np.array_equal(want2[:, :n], want[:, :n])
    assert L.omg_monoadv_destroy(h) == 0
