"""The Python binding takes every C prototype and struct layout from include/omega_amd.h (omega_amd/header.py): the
reader against declarations written out by hand, nothing skipped, the prototypes set on every function lib() hands out,
undeclared names and wrong arguments refused before the library is entered, a 64-bit address passed as a bare int, and
the four struct mirrors against the header's members.  Needs the built library, no device."""
import ctypes as C
import re

import numpy as np
import pytest

import omega_amd as oa
from omega_amd import header

FUNCTIONS, STRUCTS = header.read(oa.HEADER_PATH)

# (return kind, parameter kinds) written from the header by hand: every scalar kind and every awkward shape in it
BY_HAND = {
    "omg_restart_create": ("int", ["const char *", "int64_t", "int64_t", "int", "int", "double", "int64_t"]),  # 2 lines
    "omg_rccl_get_unique_id": ("int", ["char *"]),                            # a comment inside the parameter list
    "omg_device_synchronize": ("int", []),                                    # (void)
    "omg_halo_set_transport": ("int", ["omg_halo *", "omg_transport_fn", "void *"]),   # a callback typedef
    "omg_tend_config_default": ("void", ["omg_tend_config *"]),
    "omg_last_error": ("const char *", []),
    "omg_state_device_ptr": ("int", ["const omg_state *", "int", "int", "double **"]),
    "omg_rccl_exchange": ("int", ["omg_rccl *", "int", "const int *", "void *const *", "const size_t *", "void *const *",
                                  "const size_t *", "void *"]),
    "omg_redi_create": ("int", ["const omg_mesh *", "omg_vcoord *", "omg_eos *", "int", "double", "double", "double",
                                "omg_redi **"]),
    "omg_halo_required_bytes": ("int", ["const omg_halo *", "int", "size_t", "size_t", "size_t", "size_t *"]),
}
SCALAR = {"int": C.c_int, "double": C.c_double, "size_t": C.c_size_t, "int64_t": C.c_int64}


def _argtype(kind):
    """the table of the binding's contract, restated: scalars by name, strings as c_char_p, any other pointer opaque"""
    if kind in SCALAR:
        return SCALAR[kind]
    return C.c_char_p if kind in ("const char *", "char *") else C.c_void_p


def test_the_reader_against_declarations_written_by_hand():
    for name, want in BY_HAND.items():
        assert FUNCTIONS[name] == want, name
    p, i, d, s = C.c_void_p, C.c_int, C.c_double, C.c_char_p
    L = oa.lib()
    assert L.omg_restart_create.argtypes == [s, C.c_int64, C.c_int64, i, i, d, C.c_int64]
    assert L.omg_halo_set_transport.argtypes == [p, p, p] and L.omg_rccl_get_unique_id.argtypes == [s]
    assert L.omg_redi_create.argtypes == [p, p, p, i, d, d, d, p] and L.omg_device_synchronize.argtypes == []
    assert L.omg_rccl_exchange.argtypes == [p, i, p, p, p, p, p, p]
    assert L.omg_halo_required_bytes.argtypes == [p, i, C.c_size_t, C.c_size_t, C.c_size_t, p]
    assert L.omg_last_error.restype is s and L.omg_tend_config_default.restype is None and L.omg_redi_create.restype is i


def test_no_declaration_is_skipped():
    text = header.strip_comments(open(oa.HEADER_PATH).read())
    assert len(FUNCTIONS) == len(re.findall(r"\bomg_\w+\s*\(", text)) > 0
    kinds = [r for r, _ in FUNCTIONS.values()]
    assert kinds.count("const char *") == 2 and kinds.count("void") == 1 and set(kinds) == {"int", "void", "const char *"}


def test_a_declaration_the_reader_cannot_classify_is_named(tmp_path):
    for decl in ("int omg_x(unsigned n);", "long omg_x(void);", "int omg_x(omg_unknown_fn f);", "int omg_x(const int n);"):
        f = tmp_path / "h.h"
        f.write_text("int omg_fine(int a, double *b);\n" + decl + "\n")
        with pytest.raises(header.HeaderError, match="omg_x"):
            header.read(str(f))
    f.write_text("typedef struct s { float a; } s;\n")
    with pytest.raises(header.HeaderError, match="float a"):
        header.read(str(f))


def test_the_prototypes_are_applied_to_every_declared_function():
    L = oa.lib()
    for name, (ret, params) in FUNCTIONS.items():
        fn = getattr(L, name)
        assert hasattr(L, name) and fn.argtypes == [_argtype(k) for k in params], name
        assert fn.restype is {"int": C.c_int, "void": None, "const char *": C.c_char_p}[ret], name


def test_undeclared_names_are_refused():
    L = oa.lib()
    with pytest.raises(AttributeError, match=r"include/omega_amd\.h"):
        L.omg_no_such_function
    assert not hasattr(L, "omg_no_such_function") and not hasattr(L, "hipMalloc")   # (the library links the HIP runtime)


def test_a_function_the_library_does_not_export_is_an_error_at_load(monkeypatch):
    monkeypatch.setitem(oa._FUNCTIONS, "omg_declared_but_not_exported", ("int", []))
    with pytest.raises(oa.OmegaAmdError, match="omg_declared_but_not_exported"):
        oa._Library(C.CDLL(oa.LIB_PATH))


def test_a_64_bit_address_survives_as_a_bare_int():
    n = 1 << 16   # 1 MiB each: the allocator maps blocks of this size, above 4 GiB
    pairs = np.random.default_rng(3).uniform(-1.0, 1.0, (n, 2)) * np.array([1.0, 1.0e-17])
    out = np.zeros(2 * n)
    assert pairs.ctypes.data >= 2**32 and out.ctypes.data >= 2**32
    assert oa.lib().omg_combine_dd(pairs.ctypes.data, n, out.ctypes.data) == 0
    assert (out[0], out[1]) == oa.combine_dd(pairs) and not out[2:].any()


def test_wrong_arguments_are_stopped_before_the_library():
    L = oa.lib()
    v = C.c_int()
    assert L.omg_get_option(b"NoSuchOption", C.byref(v)) != 0
    before = oa.last_error()
    assert "NoSuchOption" in before
    # every one of these would fail inside the library with another message, or succeed, if it got there
    for call in (lambda: L.omg_set_option(b"AlsoNoOption", 1.5),            # a float for an int
                 lambda: L.omg_set_option(b"AlsoNoOption", C.c_size_t(1)),  # a c_size_t instance for an int
                 lambda: L.omg_level_pitch(C.c_size_t(80)),
                 lambda: L.omg_set_option("AlsoNoOption", 1),               # a str for a const char *
                 lambda: L.omg_set_option(b"AlsoNoOption"),                 # one argument too few
                 lambda: L.omg_combine_dd(np.int64(8), 1, None)):           # a numpy integer is no address
        with pytest.raises((C.ArgumentError, TypeError)):
            call()
        assert oa.last_error() == before


MIRRORS = {"omg_global_mesh": oa.GlobalMeshC, "omg_tend_config": oa.TendConfig, "omg_vertmix_config": oa.VertMixConfig,
           "omg_kpp_config": oa.KppConfig}
MEMBER = {"int32_t": (C.c_int32, 4), "double": (C.c_double, 8), "const int32_t *": (C.POINTER(C.c_int32), 8),
          "const double *": (C.POINTER(C.c_double), 8)}


@pytest.mark.parametrize("struct", sorted(MIRRORS))
def test_the_struct_mirrors_match_the_header(struct):
    members, mirror = STRUCTS[struct], MIRRORS[struct]
    assert set(STRUCTS) == set(MIRRORS)
    assert [(n, t) for n, t in mirror._fields_] == [(n, MEMBER[k][0]) for n, k in members]
    size = 0
    for _, kind in members:   # natural alignment: every member at the next multiple of its own size
        width = MEMBER[kind][1]
        size = -(-size // width) * width + width
    widest = max(MEMBER[k][1] for _, k in members)
    assert C.sizeof(mirror) == -(-size // widest) * widest


def test_the_struct_members_by_hand():
    assert STRUCTS["omg_kpp_config"] == [(n, "double") for n in ("VonKarman", "CritBulkRichardson", "SurfaceLayerFraction",
                                                                  "Cv", "EntrainmentRatio", "CStar")]
    vm = STRUCTS["omg_vertmix_config"]
    assert [n for n, k in vm if k == "int32_t"] == ["EnableShearMix", "EnableConvectiveMix"] and len(vm) == 9
    assert C.sizeof(oa.VertMixConfig) == 72 and oa.VertMixConfig.ShearNuZero.offset == 24
    gm = STRUCTS["omg_global_mesh"]
    assert gm[:6] == [("nCells", "int32_t"), ("nEdges", "int32_t"), ("nVertices", "int32_t"), ("maxEdges", "int32_t"),
                      ("vertexDegree", "int32_t"), ("cellsOnCell", "const int32_t *")]
    assert gm[-1] == ("bottomDepth", "const double *") and len(gm) == 5 + 8 + 26
    assert oa.GlobalMeshC._I[0] == "cellsOnCell" and len(oa.GlobalMeshC._I) == 8 and len(oa.GlobalMeshC._R) == 26
    assert oa.CONFIG_FLAGS[0] == "ThicknessFluxTendencyEnable" and oa.CONFIG_FLAGS[-1] == "WindInterpIsotropic"
    assert len(oa.CONFIG_FLAGS) == 14 and oa.CONFIG_REALS[0] == "ViscDel2" and len(oa.CONFIG_REALS) == 7
