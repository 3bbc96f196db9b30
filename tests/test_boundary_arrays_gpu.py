"""The named-array accessors of the C / Python boundary, one of each class that has them: AuxiliaryState, VertCoord
(real and integer arrays), Eos, VertMix, PressureGrad -- set / get round trips bit for bit with the documented shape and
dtype, device_ptr points at the same first row, the two size rules (copy-to-device wants exactly the size, copy-to-host
at least the size) and the unknown-name errors -- and the `which`-indexed accessors of Tendencies.

K = 17 is the smallest depth at which levelPitch pads both the K rows and the K + 1 rows (17 -> 32, 18 -> 32), so every
level-indexed copy goes through the pitched row copy."""
import ctypes as C
import re

import numpy as np
import pytest

import omega_amd as oa
from omega_amd.meshgen import planar_hex
from tests.rank_rig import raw
from tests.vert_fixtures import EOS_OUT, MIX_OUT

pytestmark = pytest.mark.gpu

K = 17
NT = 2


class Rig:
    def __init__(self):
        oa.device_init(0)
        self.gm = oa.GlobalMesh(planar_hex(8, 8, 30.0e3))
        self.decomp = oa.Decomp(self.gm, 1, 0, 3)
        self.mesh = m = oa.HorzMesh(self.decomp, K)
        self.aux = oa.AuxiliaryState(m, None, K, NT)
        self.vcoord = oa.VertCoord(m, K)
        self.eos = oa.Eos(m, K)
        self.vertmix = oa.VertMix(m, self.vcoord)
        self.pgrad = oa.PressureGrad(m, self.vcoord, self.eos)
        self.tend = oa.Tendencies(m, K, NT)
        self.rows = {"C": m.NCellsSize, "E": m.NEdgesSize, "V": m.NVerticesSize}
        oa.device_synchronize()

    def shape(self, spec):
        """the documented shape of an array from its letters in AUX_SHAPES / VCOORD_SHAPES / VCOORD_I4"""
        r = self.rows
        if spec in ("C", "E", "V"):
            return (r[spec],)
        return {"K": (K,), "CK": (r["C"], K), "CK1": (r["C"], K + 1), "EK": (r["E"], K), "VK": (r["V"], K),
                "TC": (NT, r["C"], K), "TE": (NT, r["E"], K), "C1": (r["C"],), "E1": (r["E"],)}[spec]


@pytest.fixture(scope="module")
def rig():
    return Rig()


def cases(r):
    """(object, symbol prefix, suffix of the copy functions, name, shape, dtype) of every named array"""
    out = []
    for name, s in oa.AUX_SHAPES.items():
        out.append((r.aux, "omg_aux", "", name, r.shape(s + "K" if s in ("C", "E", "V") else s), np.float64))
    for name, s in oa.VCOORD_SHAPES.items():
        out.append((r.vcoord, "omg_vcoord", "", name, r.shape(s), np.float64))
    for name, s in oa.VCOORD_I4.items():
        out.append((r.vcoord, "omg_vcoord", "_i4", name, r.shape(s), np.int32))
    for name in oa.PGRAD_ARRAYS:
        out.append((r.pgrad, "omg_pgrad", "", name, r.shape("C"), np.float64))
    for name in EOS_OUT:
        out.append((r.eos, "omg_eos", "", name, r.shape("CK"), np.float64))
    for name in MIX_OUT:
        out.append((r.vertmix, "omg_vertmix", "", name, r.shape("CK"), np.float64))
    return out


def random_values(rng, shape, dtype):
    if dtype == np.int32:
        return rng.integers(0, K, shape).astype(np.int32)
    return rng.uniform(-1.0, 1.0, shape)


def message(text=None):
    """a library error without its "[omega_amd] file:line: " prefix (default: the last error)"""
    text = oa.lib().omg_last_error().decode() if text is None else text
    m = re.fullmatch(r"\[omega_amd\] \w+\.\w+:\d+: (.*)", text)
    assert m, text
    return m.group(1)


def test_named_arrays(rig):
    rng = np.random.default_rng(17)
    all_cases = cases(rig)
    assert len(all_cases) == 18 + 9 + 10 + 3 + 2 + 3
    for obj, prefix, suffix, name, shape, dtype in all_cases:
        what = f"{prefix}{suffix} {name}"
        v = random_values(rng, shape, dtype)
        obj.set(name, v)
        got = obj.get(name)
        assert got.shape == shape and got.dtype == dtype, what
        assert np.array_equal(got, v), what
        if hasattr(obj, "device_ptr") and dtype == np.float64:
            p = obj.device_ptr(name)
            assert p, what
            first = v.reshape(-1, shape[-1])[0]
            assert np.array_equal(raw(p, first.size), first), what
        with pytest.raises(oa.OmegaAmdError, match="size mismatch"):
            obj.set(name, np.zeros(v.size + 1, dtype=dtype))
        out = np.zeros(shape, dtype=dtype)
        to_host = getattr(oa.lib(), f"{prefix}_copy_to_host{suffix}")
        assert to_host(obj.h, name.encode(), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size - 1)) != 0, what
        assert "too small" in oa.lib().omg_last_error().decode(), what
        assert to_host(obj.h, name.encode(), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size)) == 0, what
        assert np.array_equal(out, v), what


def test_unknown_names(rig):
    with pytest.raises(KeyError):
        rig.aux.get("NoSuchArray")
    with pytest.raises(oa.OmegaAmdError, match="AuxiliaryState: no array named NoSuchArray"):
        rig.aux.set("NoSuchArray", np.zeros(4))
    for obj, start in ((rig.vcoord, "VertCoord: no real array named"), (rig.eos, "Eos: no array named"),
                       (rig.vertmix, "VertMix: no array named"), (rig.pgrad, "PressureGrad: no array named")):
        for call in (lambda: obj.get("NoSuchArray"), lambda: obj.set("NoSuchArray", np.zeros(4)),
                     lambda: obj.device_ptr("NoSuchArray")):
            with pytest.raises(oa.OmegaAmdError, match="no .*array named") as e:
                call()
            assert message(str(e.value)) == start + " NoSuchArray"
    with pytest.raises(oa.OmegaAmdError, match="VertCoord: no real array named NoSuchArray"):
        rig.vcoord.get("NoSuchArray")
    # an integer array's name is no real array's (and the other way round)
    with pytest.raises(oa.OmegaAmdError, match="VertCoord: no real array named MinLayerCell"):
        rig.vcoord.device_ptr("MinLayerCell")
    buf = np.zeros(4, dtype=np.int32)
    for fn in ("omg_vcoord_copy_to_host_i4", "omg_vcoord_copy_to_device_i4"):
        assert getattr(oa.lib(), fn)(rig.vcoord.h, b"ZMid", buf.ctypes.data_as(C.c_void_p), C.c_size_t(4)) != 0
        assert message() == "VertCoord: no integer array named ZMid"


def test_tendencies_by_index(rig):
    m, t = rig.mesh, rig.tend
    shapes = [(m.NCellsSize, K), (m.NEdgesSize, K), (NT, m.NCellsSize, K)]
    pitch = oa.level_pitch(K)
    assert pitch == 32 and oa.level_pitch(K + 1) == 32
    for which, shape in enumerate(shapes):
        got = t.get(which)
        assert got.shape == shape and got.dtype == np.float64
        p, n = t.device_ptr(which)
        assert p and n == got.size
        # write through the device address (rows of `pitch` values), read through the accessor
        v = np.random.default_rng(which).uniform(-1.0, 1.0, shape)
        pad = np.zeros(shape[:-1] + (pitch,))
        pad[..., :K] = v
        oa.copy_to_device(p, pad)
        assert np.array_equal(t.get(which), v)
        out = np.zeros(shape)
        assert oa.lib().omg_tend_copy_to_host(t.h, which, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size - 1)) != 0
        assert message() == "output buffer too small for tendency array"
    # `which` = 3: the Python wrapper has no shape for it; the library's own message through the two C accessors
    with pytest.raises(IndexError):
        t.get(3)
    with pytest.raises(oa.OmegaAmdError, match="`which` must be 0, 1 or 2"):
        t.device_ptr(3)
    out = np.zeros(4)
    assert oa.lib().omg_tend_copy_to_host(t.h, 3, out.ctypes.data_as(C.c_void_p), C.c_size_t(4)) != 0
    assert message() == "Tendencies: `which` must be 0, 1 or 2"
