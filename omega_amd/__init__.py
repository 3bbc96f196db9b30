"""omega_amd -- Python binding of libomega_amd.so (include/omega_amd.h).

Thin ctypes plumbing used by tests/, bench.py and __graft_entry__.py: the product is the
C++/HIP library under omega_amd/csrc (classes named after Omega's own: Decomp, Halo,
HorzMesh, OceanState, Tracers, AuxiliaryState, VertCoord, Eos, VertMix, VertMixStep, PressureGrad, VertAdv, GentMcWilliams, Redi, Tendencies,
TimeStepper).  There is no
Python or CPU implementation of the hot path here: if the shared library is missing,
importing the binding raises, and without a HIP device every device call fails.

The header is also the binding's statement of what the functions take: omega_amd/header.py reads it, lib() sets the
argtypes and restype of every declared function from it and hands out no other symbol, and the struct mirrors are
built from its struct bodies.  So call sites pass plain Python values -- an int for an int, a size or an address of
any width, a float for a double, bytes for a string, None for NULL -- and a wrong type or count is a ctypes error
before the library is entered.  numpy integers are not addresses to ctypes: int(x) where one may arrive.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from . import header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OMEGA_AMD_LIB", os.path.join(_HERE, "lib", "libomega_amd.so"))
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "omega_amd.h")

ON_CELL, ON_EDGE, ON_VERTEX = 0, 1, 2

PD = C.POINTER(C.c_double)
PI = C.POINTER(C.c_int32)


class OmegaAmdError(RuntimeError):
    pass


def build(force: bool = False) -> str:
    """Compile libomega_amd.so for gfx950 with hipcc (omega_amd/csrc/Makefile)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8", "-s"]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd)
    return LIB_PATH


try:
    _FUNCTIONS, _STRUCTS = header.read(HEADER_PATH)
except (OSError, header.HeaderError) as e:   # a missing header, or a declaration the reader does not know
    raise OmegaAmdError(f"the binding takes its prototypes and structs from include/omega_amd.h: {e}") from None
_MEMBER = {"int32_t": C.c_int32, "double": C.c_double, "const int32_t *": PI, "const double *": PD}


def _mirror(struct: str) -> list:
    """the _fields_ of the header's struct, in its order"""
    return [(name, _MEMBER[kind]) for name, kind in _STRUCTS[struct]]


class GlobalMeshC(C.Structure):
    _fields_ = _mirror("omg_global_mesh")
    _I = tuple(n for n, t in _fields_ if t is PI)
    _R = tuple(n for n, t in _fields_ if t is PD)


class TendConfig(C.Structure):
    _fields_ = _mirror("omg_tend_config")


CONFIG_FLAGS = tuple(n for n, t in TendConfig._fields_ if t is C.c_int32)
CONFIG_REALS = tuple(n for n, t in TendConfig._fields_ if t is C.c_double)


TRANSPORT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, PI, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                           C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p)

CUSTOM_TEND_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                             C.c_int, C.c_double, C.c_void_p)

_ARGTYPE = {"int": C.c_int, "double": C.c_double, "size_t": C.c_size_t, "int64_t": C.c_int64,
            "const char *": C.c_char_p, "char *": C.c_char_p}   # every other kind is a pointer: c_void_p
_RESTYPE = {"int": C.c_int, "void": None, "const char *": C.c_char_p}


class _Library:
    """The functions include/omega_amd.h declares, each with the header's prototype set, and no other attribute."""

    def __init__(self, dll):
        missing = [name for name in _FUNCTIONS if not hasattr(dll, name)]
        if missing:
            raise OmegaAmdError(f"{LIB_PATH} does not export what {HEADER_PATH} declares: {', '.join(missing)}")
        for name, (ret, params) in _FUNCTIONS.items():
            fn = getattr(dll, name)
            fn.restype, fn.argtypes = _RESTYPE[ret], [_ARGTYPE.get(kind, C.c_void_p) for kind in params]
            setattr(self, name, fn)

    def __getattr__(self, name):
        raise AttributeError(f"{name} is not declared in include/omega_amd.h: the binding hands out no other symbol")


_lib = None


def lib():
    """The loaded library with the header's prototypes applied; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OmegaAmdError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc, gfx950). omega_amd has no CPU fallback.")
        _lib = _Library(C.CDLL(LIB_PATH))
        # test / measurement plumbing (this file, not the library): OMEGA_AMD_OPTIONS="MergeL1=0,Pair=0" is turned into
        # omg_set_option calls, so that a whole pytest or bench.py run can be repeated under another kernel structure
        for item in filter(None, os.environ.get("OMEGA_AMD_OPTIONS", "").split(",")):
            name, _, val = item.partition("=")
            set_option(name.strip(), int(val))
    return _lib


def set_option(name: str, value: int):
    """omg_set_option (omega_amd/csrc/Tuning.h): measurement / test switches; the library never reads the environment."""
    _chk(lib().omg_set_option(name.encode(), value))


def get_option(name: str) -> int:
    return _out(C.c_int, lib().omg_get_option, name.encode())


def last_error() -> str:
    """omg_last_error: the message of the last failure on the calling thread"""
    return lib().omg_last_error().decode()


def _chk(rc):
    if rc != 0:
        raise OmegaAmdError(last_error())


def _out(ctype, fn, *args):
    """what `fn` writes through its last parameter, a pointer to a `ctype`"""
    v = ctype()
    _chk(fn(*args, C.byref(v)))
    return v.value


def _pd(a):
    if a is None:
        return PD()
    assert a.dtype == np.float64 and a.flags.c_contiguous, "need C-contiguous float64"
    return a.ctypes.data_as(PD)


def _pi(a):
    if a is None:
        return PI()
    assert a.dtype == np.int32 and a.flags.c_contiguous, "need C-contiguous int32"
    return a.ctypes.data_as(PI)


class _Handle:
    """Base of every class that owns a library handle: `self.h`, made by `_create`, freed once through the class's
    `_destroy` symbol when the object goes (or by the `close()` of the classes that have one)."""
    _destroy = None

    def _create(self, symbol: str, *args):
        """self.h from a create / open function whose last argument receives the handle"""
        self.h = C.c_void_p(_out(C.c_void_p, getattr(lib(), symbol), *args))

    def _release(self):
        if self.h:
            getattr(lib(), self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass


def device_count() -> int:
    return _out(C.c_int, lib().omg_device_count)


def device_init(dev: int = 0):
    _chk(lib().omg_device_init(dev))


def device_synchronize():
    _chk(lib().omg_device_synchronize())


class Stream:
    def __init__(self, handle=None):
        self.own = handle is None
        if handle is None:
            handle = _out(C.c_void_p, lib().omg_stream_create)
        self.h = C.c_void_p(handle)

    def synchronize(self):
        _chk(lib().omg_stream_synchronize(self.h))

    def __del__(self):
        try:
            if self.own and self.h:
                lib().omg_stream_destroy(self.h)
        except Exception:
            pass


class Event(_Handle):
    _destroy = "omg_event_destroy"

    def __init__(self):
        self._create("omg_event_create")

    def record(self, stream: "Stream | None"):
        _chk(lib().omg_event_record(self.h, stream.h if stream else None))

    def elapsed_ms(self, stop: "Event") -> float:
        return _out(C.c_float, lib().omg_event_elapsed_ms, self.h, stop.h)


def _sh(s):
    """the handle of a Stream or of any object that owns one, NULL for None"""
    return s.h if s is not None else None


class GlobalMesh:
    """Keeps the numpy arrays of a meshgen mesh alive behind an omg_global_mesh."""

    def __init__(self, g: dict):
        self.g = g
        self.keep = {}
        s = GlobalMeshC()
        s.nCells, s.nEdges, s.nVertices = g["nCells"], g["nEdges"], g["nVertices"]
        s.maxEdges, s.vertexDegree = g["maxEdges"], g["vertexDegree"]
        for names, dtype, pointer in ((GlobalMeshC._I, np.int32, _pi), (GlobalMeshC._R, np.float64, _pd)):
            for n in names:
                self.keep[n] = np.ascontiguousarray(g[n], dtype=dtype)
                setattr(s, n, pointer(self.keep[n]))
        self.s = s


def write_restart(path, decomp, state, tracers, K, NT, simulation_time, steps_done, rank=0, barrier=None):
    """Restart dump: rank 0 creates the file, every rank writes the rows of its OWNED cells / edges (time
    level 0) at their global positions.  `barrier` (callable) separates the two phases when there are
    several ranks."""
    if rank == 0:
        _chk(lib().omg_restart_create(os.fsencode(path), decomp.get_int("NCellsGlobal"), decomp.get_int("NEdgesGlobal"),
                                      K, NT, simulation_time, steps_done))
    if barrier is not None:
        barrier()
    f = _out(C.c_void_p, lib().omg_restart_open, os.fsencode(path), 1)
    try:
        nc, ne = decomp.get_int("NCellsOwned"), decomp.get_int("NEdgesOwned")
        cid = np.ascontiguousarray(decomp.get_array("CellID")[:nc], dtype=np.int32)
        eid = np.ascontiguousarray(decomp.get_array("EdgeID")[:ne], dtype=np.int32)
        h, u = state.copy_to_host(0)
        _chk(lib().omg_restart_write_rows(f, b"layerThickness", 0, _pi(cid), nc, _pd(np.ascontiguousarray(h[:nc]))))
        _chk(lib().omg_restart_write_rows(f, b"normalVelocity", 0, _pi(eid), ne, _pd(np.ascontiguousarray(u[:ne]))))
        if NT > 0:
            tr = tracers.copy_to_host(0)
            for l in range(NT):
                _chk(lib().omg_restart_write_rows(f, b"tracers", l, _pi(cid), nc, _pd(np.ascontiguousarray(tr[l, :nc]))))
    finally:
        lib().omg_restart_close(f)
    if barrier is not None:
        barrier()


def write_history(path, decomp, state, tracers, aux, contents="State,Tracers,AuxiliaryState", simulation_time=0.0,
                  time_level=0, create_file=True, stream=None) -> int:
    """One history dump (omg_history_write): field names / groups as in the reference's History stream Contents."""
    return _out(C.c_int, lib().omg_history_write, os.fsencode(path), decomp.h, state.h, _sh(tracers), aux.h,
                contents.encode(), simulation_time, time_level, create_file, _sh(stream))


def read_restart(path, decomp, mesh, state, tracers, K, NT):
    """Restart load: every rank reads the rows of ALL its local cells / edges (owned and halo, by global
    id) into time level 0, so no halo exchange is needed afterwards.  Returns (simulation_time, steps_done)."""
    f = _out(C.c_void_p, lib().omg_restart_open, os.fsencode(path), 0)
    try:
        info = [C.c_int64(), C.c_int64(), C.c_int(), C.c_int(), C.c_double(), C.c_int64()]
        _chk(lib().omg_restart_info(f, *[C.byref(x) for x in info]))
        if (info[0].value, info[1].value, info[2].value) != (decomp.get_int("NCellsGlobal"), decomp.get_int("NEdgesGlobal"), K) \
                or info[3].value < max(NT, 1):
            raise OmegaAmdError(f"{path}: restart file does not match this mesh / configuration")
        nc, ne = mesh.NCellsAll, mesh.NEdgesAll
        cid = np.ascontiguousarray(decomp.get_array("CellID")[:nc], dtype=np.int32)
        eid = np.ascontiguousarray(decomp.get_array("EdgeID")[:ne], dtype=np.int32)
        h = np.zeros((mesh.NCellsSize, K))
        u = np.zeros((mesh.NEdgesSize, K))
        rows = np.empty((nc, K))
        _chk(lib().omg_restart_read_rows(f, b"layerThickness", 0, _pi(cid), nc, _pd(rows)))
        h[:nc] = rows
        rows = np.empty((ne, K))
        _chk(lib().omg_restart_read_rows(f, b"normalVelocity", 0, _pi(eid), ne, _pd(rows)))
        u[:ne] = rows
        state.copy_to_device(h, u, 0)
        if NT > 0:
            tr = np.zeros((NT, mesh.NCellsSize, K))
            rows = np.empty((nc, K))
            for l in range(NT):
                _chk(lib().omg_restart_read_rows(f, b"tracers", l, _pi(cid), nc, _pd(rows)))
                tr[l, :nc] = rows
            tracers.copy_to_device(tr, 0)
        return info[4].value, info[5].value
    finally:
        lib().omg_restart_close(f)


class MeshFile(_Handle):
    """An MPAS mesh / initial-state file (NetCDF classic CDF-1/2/5) opened by the library's own reader;
    `.gm` is the GlobalMesh to build a Decomp from (the arrays live inside the file handle)."""
    _destroy = "omg_mesh_file_close"

    def __init__(self, path: str, mesh: bool = True):
        self._create("omg_mesh_file_open", os.fsencode(path))
        self.gm = None
        if not mesh:   # a state-only file (initial conditions, forcing): variables through read()
            return
        gm = GlobalMesh.__new__(GlobalMesh)
        gm.s = GlobalMeshC()
        gm.keep = {"file": self}
        _chk(lib().omg_mesh_file_global_mesh(self.h, C.byref(gm.s)))
        self.gm = gm

    def dim(self, name: str) -> int:
        return _out(C.c_int64, lib().omg_mesh_file_dim, self.h, name.encode())

    def read(self, name: str, record: int = -1) -> np.ndarray:
        n = _out(C.c_int64, lib().omg_mesh_file_var_size, self.h, name.encode(), record)
        if n < 0:
            raise KeyError(name)
        out = np.empty(n, dtype=np.float64)
        _chk(lib().omg_mesh_file_read_f64(self.h, name.encode(), record, _pd(out), n))
        return out

    def arrays(self) -> dict:
        """The global mesh as numpy copies, keyed like a meshgen mesh (test use)."""
        s = self.gm.s
        nC, nE, nV, mE, vD = s.nCells, s.nEdges, s.nVertices, s.maxEdges, s.vertexDegree
        shp = {"cellsOnCell": (nC, mE), "edgesOnCell": (nC, mE), "verticesOnCell": (nC, mE), "cellsOnEdge": (nE, 2),
               "verticesOnEdge": (nE, 2), "edgesOnEdge": (nE, 2 * mE), "cellsOnVertex": (nV, vD),
               "edgesOnVertex": (nV, vD), "kiteAreasOnVertex": (nV, vD), "weightsOnEdge": (nE, 2 * mE)}
        out = {"nCells": nC, "nEdges": nE, "nVertices": nV, "maxEdges": mE, "vertexDegree": vD}
        for n in GlobalMeshC._I + GlobalMeshC._R:
            p = getattr(s, n)
            el = n[-4:] == "Cell" and nC or n[-4:] == "Edge" and nE or nV
            if n == "areaTriangle":
                el = nV
            if n == "bottomDepth":
                el = nC
            shape = shp.get(n, (el,))
            out[n] = np.ctypeslib.as_array(p, shape=(int(np.prod(shape)),)).reshape(shape).copy()
        return out


class DeviceBuffer:
    """A device copy of a host array (omg_device_malloc / omg_copy_to_device)."""

    def __init__(self, host: np.ndarray):
        self.host = np.ascontiguousarray(host)
        self.ptr = _out(C.c_void_p, lib().omg_device_malloc, self.host.nbytes)
        _chk(lib().omg_copy_to_device(self.ptr, self.host.ctypes.data, self.host.nbytes))

    def to_host(self) -> np.ndarray:
        out = np.empty_like(self.host)
        _chk(lib().omg_copy_to_host(out.ctypes.data, self.ptr, out.nbytes))
        return out

    def __del__(self):
        try:
            lib().omg_device_free(self.ptr)
        except Exception:
            pass


def copy_to_device(dev_ptr: int, host: np.ndarray):
    """omg_copy_to_device: a contiguous host array to raw device memory (synchronous)"""
    a = np.ascontiguousarray(host)
    _chk(lib().omg_copy_to_device(dev_ptr, a.ctypes.data, a.nbytes))


def combine_dd(pairs) -> tuple:
    """ddSum (Reductions.h:24-35) over an [n][2] array of (hi, lo) partial sums, in order."""
    p = np.ascontiguousarray(pairs, dtype=np.float64).reshape(-1, 2)
    out = (C.c_double * 2)()
    _chk(lib().omg_combine_dd(_pd(p), p.shape[0], out))
    return out[0], out[1]


def local_sum_dd(a_ptr: int, n: int, b_ptr: int = 0, stream=None) -> tuple:
    """Double-double sum of n device doubles at a_ptr (times those at b_ptr if given)."""
    out = (C.c_double * 2)()
    _chk(lib().omg_local_sum_dd(a_ptr, b_ptr or None, n, _sh(stream), out))
    return out[0], out[1]


def level_pitch(k: int) -> int:
    """Row pitch (in values) of the library's own level-indexed device arrays (omg_level_pitch)."""
    return lib().omg_level_pitch(k)


def local_weighted_sum_dd(w_ptr: int, a_ptr: int, nrows: int, k: int, b_ptr: int = 0, stream=None, row_pitch: int = 0) -> tuple:
    """row_pitch: pitch of the [rows][k] arrays in values (level_pitch(k) for arrays owned by the library, 0 = compact)"""
    out = (C.c_double * 2)()
    _chk(lib().omg_local_weighted_sum_dd(w_ptr, a_ptr, b_ptr or None, nrows, k, row_pitch, _sh(stream), out))
    return out[0], out[1]


def device_resource_count() -> int:
    """omg_device_resource_count: device buffers, streams and events the library has created so far"""
    return _out(C.c_int64, lib().omg_device_resource_count)


_TRIDIAG = {("general", "pcr"): "omg_tridiag_pcr_solve", ("general", "thomas"): "omg_tridiag_thomas_solve",
            ("diffusion", "pcr"): "omg_tridiag_pcr_diff_solve", ("diffusion", "thomas"): "omg_tridiag_thomas_diff_solve"}


def _tridiag(form, algorithm, coeffs, x, stream, nbatch, nrow, row_pitch):
    """The batched tridiagonal solvers (omega_amd/csrc/TriDiagSolvers.h).  With numpy arrays: [NBatch][NRow] inputs,
    staged to the device, solved, and the solution returned as a new array.  With device addresses (ints): solved in
    place on `stream` (asynchronous), nbatch / nrow / row_pitch (0 = nrow) given."""
    key = (form, algorithm)
    if key not in _TRIDIAG:
        raise ValueError(f"algorithm must be 'pcr' or 'thomas', not {algorithm!r}")
    fn = getattr(lib(), _TRIDIAG[key])
    if isinstance(x, (int, np.integer)):
        if nbatch is None or nrow is None:
            raise ValueError("the device-address form needs nbatch and nrow")
        _chk(fn(*[int(a) for a in (*coeffs, x)], nbatch, nrow, row_pitch, _sh(stream)))
        return None
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (*coeffs, x)]
    shape = arrs[-1].shape
    if len(shape) != 2 or any(a.shape != shape for a in arrs):
        raise OmegaAmdError(f"tridiagonal solve: every array must be [NBatch][NRow] of one shape, got "
                            f"{[a.shape for a in arrs]}")
    bufs = [DeviceBuffer(a) for a in arrs]
    _chk(fn(*[b.ptr for b in bufs], shape[0], shape[1], 0, _sh(stream)))
    if stream is not None:
        stream.synchronize()
    return bufs[-1].to_host()


def tridiag_solve(dl, d, du, x, algorithm: str = "pcr", stream=None, nbatch=None, nrow=None, row_pitch: int = 0):
    """Solve DL x(k-1) + D x(k) + DU x(k+1) = X per row: ThomasSolver / PCRSolver::solve (TriDiagSolvers.h)."""
    return _tridiag("general", algorithm, (dl, d, du), x, stream, nbatch, nrow, row_pitch)


def tridiag_diff_solve(g, h, x, algorithm: str = "pcr", stream=None, nbatch=None, nrow=None, row_pitch: int = 0):
    """Solve -G(k-1) x(k-1) + (H(k) + G(k-1) + G(k)) x(k) - G(k) x(k+1) = X per row: ThomasDiffusionSolver /
    PCRDiffusionSolver::solve (TriDiagSolvers.h)."""
    return _tridiag("diffusion", algorithm, (g, h), x, stream, nbatch, nrow, row_pitch)


def global_sum_dd(local_hi_lo, group=None, halo=None, stream=None) -> float:
    """globalSum (Reductions.h:71-84): all-gather the ranks' (hi, lo) partial sums and combine them with the
    ddSum operator in rank order -- the same value on every rank and for every partition.  With `halo` the gather
    runs inside the library over that Halo's wire (omg_halo_global_sum_dd: RCCL or peer wire); without, over
    torch.distributed (test rigs on the host-staged transport)."""
    if halo is not None:
        return halo.global_sum_dd([local_hi_lo], stream=stream)[0]
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return combine_dd([local_hi_lo])[0]
    dev = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
    mine = torch.tensor(list(local_hi_lo), dtype=torch.float64, device=dev)
    allp = [torch.empty_like(mine) for _ in range(dist.get_world_size(group))]
    dist.all_gather(allp, mine, group=group)
    return combine_dd(torch.stack(allp).cpu().numpy())[0]


def read_partition_file(path: str) -> np.ndarray:
    """A METIS partition file (`graph.info.part.N`: one owner task per line, cell order) as the
    cell_task vector of Decomp -- the reference calls METIS itself (Decomp.cpp:868-1000); production
    runs with pre-computed partitions pass them here."""
    return np.loadtxt(path, dtype=np.int32, ndmin=1)


def partition_cells(gm: GlobalMesh, nparts: int, method: str = "graph"):
    """(cell_task[nCells], edge_cut) of the built-in partitioners: "rcb" or "graph" (omg_partition_cells)."""
    out = np.zeros(gm.s.nCells, dtype=np.int32)
    return out, _out(C.c_int64, lib().omg_partition_cells, C.byref(gm.s), nparts, method.encode(), _pi(out))


class Decomp(_Handle):
    _destroy = "omg_decomp_destroy"

    def __init__(self, gm: GlobalMesh, nparts: int = 1, mytask: int = 0, halo_width: int = 3, cell_task=None,
                 local_order: str = "global"):
        """local_order: "global" (the reference's numbering by global id), "curve" (Morton curve through the cell
        centres: spatially compact local numbering whatever the file's order), "hilbert" (Hilbert curve) or "kd" (k-d
        order: compact tiles on the surface -- what spheres want)."""
        self.gm = gm
        ct = None if cell_task is None else np.ascontiguousarray(cell_task, dtype=np.int32)
        self._create("omg_decomp_create_ordered", C.byref(gm.s), nparts, mytask, halo_width, _pi(ct),
                     {"global": 0, "curve": 1, "hilbert": 2, "kd": 3}[local_order])

    def get_int(self, name: str) -> int:
        return _out(C.c_int32, lib().omg_decomp_get_int, self.h, name.encode())

    def get_array(self, name: str) -> np.ndarray:
        hw = self.get_int("HaloWidth")
        shapes = {"CellID": (self.get_int("NCellsSize"),), "EdgeID": (self.get_int("NEdgesSize"),),
                  "VertexID": (self.get_int("NVerticesSize"),), "CellLoc": (self.get_int("NCellsSize"), 2),
                  "EdgeLoc": (self.get_int("NEdgesSize"), 2), "VertexLoc": (self.get_int("NVerticesSize"), 2),
                  "NCellsHalo": (hw,), "NEdgesHalo": (hw,), "NVerticesHalo": (hw,),
                  "CellTask": (self.get_int("NCellsGlobal"),)}
        out = np.zeros(shapes[name], dtype=np.int32)
        _chk(lib().omg_decomp_get_array(self.h, name.encode(), _pi(out), out.size))
        return out


class RcclComm(_Handle):
    """RCCL communicator owned by the library (omega_amd/csrc/Rccl.cpp).  `unique_id()` on rank 0, distribute the
    128 bytes by any side channel, then every rank constructs RcclComm(id, nranks, rank) after device_init."""
    _destroy = "omg_rccl_destroy"

    ID_BYTES = 128

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(RcclComm.ID_BYTES)
        _chk(lib().omg_rccl_get_unique_id(buf))
        return buf.raw

    def __init__(self, unique_id: bytes, nranks: int, rank: int):
        assert len(unique_id) == RcclComm.ID_BYTES
        self._create("omg_rccl_create", C.create_string_buffer(unique_id, RcclComm.ID_BYTES), nranks, rank)

    def info(self) -> dict:
        n, r, v, e = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
        _chk(lib().omg_rccl_info(self.h, C.byref(n), C.byref(r), C.byref(v), C.byref(e)))
        return {"nranks": n.value, "rank": r.value, "version": v.value, "exchanges": e.value}

    def abort(self):
        _chk(lib().omg_rccl_abort(self.h))

    def exchange(self, peers, send_ptrs, send_bytes, recv_ptrs, recv_bytes, stream=None):
        n = len(peers)
        _chk(lib().omg_rccl_exchange(self.h, n, (C.c_int * n)(*peers), (C.c_void_p * n)(*send_ptrs),
                                     (C.c_size_t * n)(*send_bytes), (C.c_void_p * n)(*recv_ptrs),
                                     (C.c_size_t * n)(*recv_bytes), _sh(stream)))

    def close(self):
        """omg_rccl_destroy (ncclCommDestroy): explicitly, while the peers are still there -- not left to a destructor at
        interpreter exit"""
        self._release()


class PeerWire(_Handle):
    """Direct peer-copy halo wire owned by the library (omega_amd/csrc/PeerWire.cpp): mailbox + flags exported with
    HIP IPC, exchanges fully stream-ordered.  Create after device_init, all_gather `handle()` over any side channel,
    `connect(list_of_handles_in_rank_order)`, then `Halo.use_peer(wire)`."""
    _destroy = "omg_peer_destroy"

    HANDLE_BYTES = 160

    def __init__(self, nranks: int, rank: int, mailbox_bytes: int):
        self._create("omg_peer_create", nranks, rank, mailbox_bytes)
        self.nranks = nranks

    def handle(self) -> bytes:
        buf = C.create_string_buffer(PeerWire.HANDLE_BYTES)
        _chk(lib().omg_peer_local_handle(self.h, buf))
        return buf.raw

    def connect(self, handles):
        blob = b"".join(handles)
        assert len(blob) == self.nranks * PeerWire.HANDLE_BYTES
        _chk(lib().omg_peer_connect(self.h, C.create_string_buffer(blob, len(blob))))

    def info(self) -> dict:
        e, s = C.c_int64(), C.c_int()
        _chk(lib().omg_peer_info(self.h, C.byref(e), C.byref(s)))
        return {"exchanges": e.value, "status": s.value}

    def set_timeout(self, seconds: float):
        _chk(lib().omg_peer_set_timeout(self.h, seconds))

    def close(self):
        self._release()


class Halo(_Handle):
    _destroy = "omg_halo_destroy"

    def __init__(self, decomp: Decomp):
        self.decomp = decomp
        self._create("omg_halo_create", decomp.h)
        self._cb = None
        self._bufs = None

    @property
    def neighbors(self):
        n = _out(C.c_int, lib().omg_halo_num_neighbors, self.h)
        return [_out(C.c_int, lib().omg_halo_neighbor_task, self.h, i) for i in range(n)]

    def get_list(self, i: int, elem: int, recv: bool) -> np.ndarray:
        n = _out(C.c_int, lib().omg_halo_list_size, self.h, i, elem, recv)
        out = np.zeros(max(n, 1), dtype=np.int32)
        _chk(lib().omg_halo_get_list(self.h, i, elem, recv, _pi(out)))
        return out[:n]

    def required_bytes(self, i: int, per_cell: int, per_edge: int, per_vertex: int = 0) -> int:
        return _out(C.c_size_t, lib().omg_halo_required_bytes, self.h, i, per_cell, per_edge, per_vertex)

    def use_rccl(self, comm: "RcclComm"):
        """Route the exchanges through RCCL send / recv issued inside the library (production wire)."""
        _chk(lib().omg_halo_use_rccl(self.h, comm.h))
        self._comm = comm

    def use_peer(self, wire: "PeerWire"):
        """Route the exchanges through direct peer copies into the neighbours' mailboxes (stream-ordered, no host waits)."""
        _chk(lib().omg_halo_use_peer(self.h, wire.h))
        self._wire = wire

    def global_sum_dd(self, local_pairs, stream=None) -> list:
        """omg_halo_global_sum_dd: [(hi, lo), ...] local partial sums -> the global sums (hi parts), same bits on every rank"""
        p = np.ascontiguousarray(local_pairs, dtype=np.float64).reshape(-1, 2)
        out = np.zeros_like(p)
        _chk(lib().omg_halo_global_sum_dd(self.h, _pd(p), p.shape[0], _pd(out), _sh(stream)))
        return [float(x) for x in out[:, 0]]

    def exchange_state(self, state, tracers=None, time_level: int = 0, tracers_time_level: int | None = None, stream=None):
        """omg_halo_exchange_state: h, u and the tracers as ONE message per neighbour (what the time steppers do after a stage)"""
        _chk(lib().omg_halo_exchange_state(self.h, state.h, time_level, _sh(tracers),
                                           time_level if tracers_time_level is None else tracers_time_level, _sh(stream)))

    def check(self):
        """omg_halo_check: raises if a peer-wire wait of an earlier exchange gave up (ask after synchronising)"""
        _chk(lib().omg_halo_check(self.h))

    def recv_rows(self, per_cell: int, per_edge: int, per_vertex: int = 0) -> int:
        return _out(C.c_size_t, lib().omg_halo_recv_rows, self.h, per_cell, per_edge, per_vertex)

    def set_transport(self, fn):
        """fn(tasks, send_ptrs, send_bytes, recv_ptrs, recv_bytes, stream_handle) -> int"""
        def _cb(_ctx, n, tasks, sp, sb, rp, rb, stream):
            try:
                return int(fn([tasks[i] for i in range(n)], [sp[i] for i in range(n)], [sb[i] for i in range(n)],
                              [rp[i] for i in range(n)], [rb[i] for i in range(n)], stream) or 0)
            except Exception as e:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1
        self._cb = TRANSPORT_FN(_cb)
        _chk(lib().omg_halo_set_transport(self.h, self._cb, None))

    def exchange(self, dev_ptr: int, nt: int, rows_size: int, k: int, elem: int, stream=None, row_pitch: int = 0,
                 elem_bytes: int = 8):
        """Halo::exchangeFullArrayHalo on a raw device array [nt][rows_size][row_pitch or k] of elem_bytes-byte values
        (8: R8 / I8, 4: I4 / R4); rank 1 is nt = 1, k = 1."""
        if elem_bytes == 8:
            _chk(lib().omg_halo_exchange(self.h, dev_ptr, nt, rows_size, k, row_pitch, elem, _sh(stream)))
        else:
            _chk(lib().omg_halo_exchange_bytes(self.h, dev_ptr, elem_bytes, nt, rows_size, k, row_pitch, elem, _sh(stream)))


_MESH_I4 = {"CellsOnCell": ("C", "ME"), "EdgesOnCell": ("C", "ME"), "NEdgesOnCell": ("C",),
            "VerticesOnCell": ("C", "ME"), "CellsOnEdge": ("E", 2), "EdgesOnEdge": ("E", "ME2"),
            "NEdgesOnEdge": ("E",), "VerticesOnEdge": ("E", 2), "CellsOnVertex": ("V", "VD"),
            "EdgesOnVertex": ("V", "VD")}
_MESH_R8 = {"AreaCell": ("C",), "AreaTriangle": ("V",), "KiteAreasOnVertex": ("V", "VD"), "DvEdge": ("E",),
            "DcEdge": ("E",), "AngleEdge": ("E",), "WeightsOnEdge": ("E", "ME2"), "FEdge": ("E",), "FCell": ("C",),
            "FVertex": ("V",), "BottomDepth": ("C",), "EdgeSignOnCell": ("C", "ME"), "EdgeSignOnVertex": ("V", "VD"),
            "EdgeMask": ("E", "K"), "MeshScalingDel2": ("E",), "MeshScalingDel4": ("E",)}
for _el, _d in (("Cell", "C"), ("Edge", "E"), ("Vertex", "V")):
    for _p in ("X", "Y", "Z", "Lon", "Lat"):
        _MESH_R8[_p + _el] = (_d,)


class HorzMesh(_Handle):
    _destroy = "omg_mesh_destroy"

    def __init__(self, decomp: Decomp, nvertlayers: int, host_only: bool = False):
        self.decomp = decomp
        self._create("omg_mesh_create", decomp.h, nvertlayers, host_only)
        self._dims = None

    def get_int(self, name: str) -> int:
        return _out(C.c_int32, lib().omg_mesh_get_int, self.h, name.encode())

    def __getattr__(self, name):
        if name.startswith("N") or name in ("MaxEdges", "MaxEdges2", "VertexDegree"):
            try:
                return self.get_int(name)
            except OmegaAmdError:
                pass
        raise AttributeError(name)

    def _shape(self, spec):
        if self._dims is None:
            self._dims = {"C": self.get_int("NCellsSize"), "E": self.get_int("NEdgesSize"),
                          "V": self.get_int("NVerticesSize"), "ME": self.get_int("MaxEdges"),
                          "ME2": self.get_int("MaxEdges2"), "VD": self.get_int("VertexDegree"),
                          "K": self.get_int("NVertLayers")}
        return tuple(self._dims[s] if isinstance(s, str) else s for s in spec)

    def get_array(self, name: str) -> np.ndarray:
        if name in _MESH_I4:
            out = np.zeros(self._shape(_MESH_I4[name]), dtype=np.int32)
            _chk(lib().omg_mesh_get_array_i4(self.h, name.encode(), _pi(out), out.size))
        else:
            out = np.zeros(self._shape(_MESH_R8[name]), dtype=np.float64)
            _chk(lib().omg_mesh_get_array_r8(self.h, name.encode(), _pd(out), out.size))
        return out

    def local_arrays(self) -> dict:
        """All host arrays + sizes, in the dict form oracle.Mesh consumes (test use)."""
        L = {n: self.get_int(n) for n in ("NCellsOwned", "NCellsAll", "NCellsSize", "NEdgesOwned", "NEdgesAll",
                                          "NEdgesSize", "NVerticesOwned", "NVerticesAll", "NVerticesSize",
                                          "MaxEdges", "MaxEdges2", "VertexDegree")}
        for n in list(_MESH_I4) + [k for k in _MESH_R8 if k not in ("EdgeSignOnCell", "EdgeSignOnVertex", "EdgeMask",
                                                                    "MeshScalingDel2", "MeshScalingDel4")]:
            L[n] = self.get_array(n)
        return L

    def set_fvertex(self, values: np.ndarray):
        _chk(lib().omg_mesh_set_fvertex(self.h, _pd(np.ascontiguousarray(values, dtype=np.float64))))


class HorzOperators:
    """DivergenceOnCell / GradientOnEdge / CurlOnVertex / TangentialReconOnEdge / InterpCellToEdge
    (HorzOperators.h:9-187) on host arrays staged through device buffers (test / tooling use; the
    C entry points omg_horz_* take raw device pointers)."""

    def __init__(self, mesh: HorzMesh):
        self.mesh = mesh

    def _run(self, fn, x: np.ndarray, rows_out: int, n: int, *extra):
        x = np.ascontiguousarray(x, dtype=np.float64)
        one_d = x.ndim == 1
        k = 1 if one_d else x.shape[1]
        din = DeviceBuffer(x)
        dout = DeviceBuffer(np.zeros((rows_out,) if one_d else (rows_out, k)))
        if one_d:
            _chk(fn(self.mesh.h, din.ptr, dout.ptr, *extra, n, None))
        else:
            _chk(fn(self.mesh.h, din.ptr, dout.ptr, k, 0, n, None))
        device_synchronize()
        return dout.to_host()

    def divergence(self, vec_edge, n=-1):
        return self._run(lib().omg_horz_divergence, vec_edge, self.mesh.NCellsSize, n)

    def gradient(self, scalar_cell, n=-1):
        return self._run(lib().omg_horz_gradient, scalar_cell, self.mesh.NEdgesSize, n)

    def curl(self, vec_edge, n=-1):
        return self._run(lib().omg_horz_curl, vec_edge, self.mesh.NVerticesSize, n)

    def tangential_recon(self, vec_edge, n=-1):
        return self._run(lib().omg_horz_tangential_recon, vec_edge, self.mesh.NEdgesSize, n)

    def interp_cell_to_edge(self, array_cell, isotropic: bool, n=-1):
        return self._run(lib().omg_horz_interp_cell_to_edge, array_cell, self.mesh.NEdgesSize, n, isotropic)


def _config(cls, default: str, over: dict):
    """A `cls` struct with the library's defaults (the function `default`) and the fields in `over` replaced; an
    unknown field raises KeyError."""
    c = cls()
    _chk(getattr(lib(), default)(C.byref(c)) or 0)   # (omg_tend_config_default returns nothing)
    for k, v in over.items():
        if k not in {f[0] for f in cls._fields_}:
            raise KeyError(k)
        setattr(c, k, v)
    return c


def default_config(**over) -> TendConfig:
    return _config(TendConfig, "omg_tend_config_default", over)


class OceanState(_Handle):
    _destroy = "omg_state_destroy"

    def __init__(self, mesh: HorzMesh, halo: Halo | None, nvertlayers: int, ntimelevels: int = 2):
        self.mesh, self.halo, self.K = mesh, halo, nvertlayers
        self._create("omg_state_create", mesh.h, halo.h if halo else None, nvertlayers, ntimelevels)

    def copy_to_device(self, h=None, u=None, time_level: int = 0):
        _chk(lib().omg_state_copy_to_device(self.h, time_level, _pd(h), _pd(u)))

    def copy_to_host(self, time_level: int = 0):
        h = np.zeros((self.mesh.NCellsSize, self.K))
        u = np.zeros((self.mesh.NEdgesSize, self.K))
        _chk(lib().omg_state_copy_to_host(self.h, time_level, _pd(h), _pd(u)))
        return h, u

    def device_ptr(self, which: int, time_level: int = 0) -> int:
        return _out(C.c_void_p, lib().omg_state_device_ptr, self.h, time_level, which)

    def exchange_halo(self, time_level: int = 0, stream=None):
        _chk(lib().omg_state_exchange_halo(self.h, time_level, _sh(stream)))

    def update_time_levels(self, stream=None):
        _chk(lib().omg_state_update_time_levels(self.h, _sh(stream)))


class Tracers(_Handle):
    _destroy = "omg_tracers_destroy"

    def __init__(self, mesh: HorzMesh, halo: Halo | None, nvertlayers: int, ntracers: int, ntimelevels: int = 2):
        self.mesh, self.K, self.NT = mesh, nvertlayers, ntracers
        self._create("omg_tracers_create", mesh.h, halo.h if halo else None, nvertlayers, ntracers, ntimelevels)

    def copy_to_device(self, tr, time_level: int = 0):
        _chk(lib().omg_tracers_copy_to_device(self.h, time_level, _pd(tr)))

    def copy_to_host(self, time_level: int = 0):
        tr = np.zeros((max(self.NT, 1), self.mesh.NCellsSize, self.K))
        if self.NT > 0:
            _chk(lib().omg_tracers_copy_to_host(self.h, time_level, _pd(tr)))
        return tr

    def device_ptr(self, time_level: int = 0) -> int:
        return _out(C.c_void_p, lib().omg_tracers_device_ptr, self.h, time_level)

    def exchange_halo(self, time_level: int = 0, stream=None):
        _chk(lib().omg_tracers_exchange_halo(self.h, time_level, _sh(stream)))

    def update_time_levels(self, stream=None):
        _chk(lib().omg_tracers_update_time_levels(self.h, _sh(stream)))


class _NamedArrays:
    """get / set / device_ptr of a class whose library object has named device arrays: `_arrays` is the prefix of its
    <prefix>_copy_to_host / _copy_to_device / _device_ptr symbols and `_shape(name)` the class's own shape rule for a
    host copy.  A name in `_i4` (VertCoord) is an int32 array and goes through the <prefix>_copy_to_*_i4 symbols."""
    _arrays = None
    _i4 = ()

    def _array_call(self, op: str, name: str, *args):
        _chk(getattr(lib(), f"{self._arrays}_{op}")(self.h, name.encode(), *args))

    def get(self, name: str) -> np.ndarray:
        if name in self._i4:
            out = np.zeros(self._shape(name), dtype=np.int32)
            self._array_call("copy_to_host_i4", name, _pi(out), out.size)
        else:
            out = np.zeros(self._shape(name))
            self._array_call("copy_to_host", name, _pd(out), out.size)
        return out

    def set(self, name: str, values: np.ndarray):
        if name in self._i4:
            v = np.ascontiguousarray(values, dtype=np.int32)
            self._array_call("copy_to_device_i4", name, _pi(v), v.size)
        else:
            v = np.ascontiguousarray(values, dtype=np.float64)
            self._array_call("copy_to_device", name, _pd(v), v.size)

    def device_ptr(self, name: str) -> int:
        p = C.c_void_p()
        self._array_call("device_ptr", name, C.byref(p), None)
        return p.value


AUX_SHAPES = {"KineticEnergyCell": "C", "VelocityDivCell": "C", "FluxLayerThickEdge": "E", "MeanLayerThickEdge": "E",
              "SshCell": "C", "RelVortVertex": "V", "NormRelVortVertex": "V", "NormPlanetVortVertex": "V",
              "NormRelVortEdge": "E", "NormPlanetVortEdge": "E", "Del2Edge": "E", "Del2DivCell": "C",
              "Del2RelVortVertex": "V", "HTracersEdge": "TE", "Del2TracersCell": "TC", "NormalStressEdge": "E1",
              "ZonalStressCell": "C1", "MeridStressCell": "C1"}


class AuxiliaryState(_Handle, _NamedArrays):
    _destroy, _arrays = "omg_aux_destroy", "omg_aux"

    def __init__(self, mesh: HorzMesh, halo: Halo | None, nvertlayers: int, ntracers: int):
        self.mesh, self.K, self.NT = mesh, nvertlayers, ntracers
        self._create("omg_aux_create", mesh.h, halo.h if halo else None, nvertlayers, ntracers)

    def set_options(self, flux_thickness_upwind=False, flux_tracer_upwind=False, wind_interp_isotropic=True):
        _chk(lib().omg_aux_set_options(self.h, flux_thickness_upwind, flux_tracer_upwind, wind_interp_isotropic))

    def compute_mom_aux(self, state: OceanState, thick_tl=0, vel_tl=0, stream=None):
        _chk(lib().omg_aux_compute_mom_aux(self.h, state.h, thick_tl, vel_tl, _sh(stream)))

    def compute_all(self, state: OceanState, tracers: Tracers, tracer_tl=0, thick_tl=0, vel_tl=0, stream=None):
        _chk(lib().omg_aux_compute_all(self.h, state.h, tracers.h, tracer_tl, thick_tl, vel_tl, _sh(stream)))

    def _shape(self, name):
        m, K, nt = self.mesh, self.K, max(self.NT, 1)
        rows = {"C": m.NCellsSize, "E": m.NEdgesSize, "V": m.NVerticesSize}
        s = AUX_SHAPES[name]
        if s in rows:
            return (rows[s], K)
        if s[0] == "T":
            return (nt, rows[s[1]], K)
        return (rows[s[0]],)


def _stage_levels(x, lead: tuple, k: int, keep: "list | None" = None):
    """A level-indexed array as (device pointer, staged buffer or None): an int is taken as the device address of
    [*lead][level_pitch(k)] doubles and passed through; a numpy array [*lead][k] is staged into a padded device copy
    (also appended to `keep`, if given, to stay alive there).  The pointer is a c_void_p object, as every handle is:
    callers read its address as `.value`."""
    if isinstance(x, (int, np.integer)):
        return C.c_void_p(int(x)), None
    a = np.asarray(x, dtype=np.float64)
    assert a.shape == lead + (k,), f"expected shape {lead + (k,)}, got {a.shape}"
    pad = np.zeros(lead + (level_pitch(k),))
    pad[..., :k] = a
    b = DeviceBuffer(pad)
    if keep is not None:
        keep.append(b)
    return C.c_void_p(b.ptr), b


def _read_back(buf, k: int, stream):
    """The result of an in-place call on a buffer staged by _stage_levels, without the row padding, once the stream
    and the device have drained; None for None (a device address was passed: nothing to return)."""
    if buf is None:
        return None
    if stream is not None:
        stream.synchronize()
    device_synchronize()
    return buf.to_host()[..., :k]


def _level_dev(x, rows: int, k: int, keep: list):
    """A level-indexed input as a device pointer: an int is taken as a device address of [rows][level_pitch(k)]
    doubles, a numpy array [rows][k] is staged into a padded device copy (kept alive in `keep`)."""
    return _stage_levels(x, (rows,), k, keep)[0]


def _cell_dev(x, rows: int, keep: list):
    """A per-cell input as a device pointer: None (NULL: read as zero), an int device address or a numpy array."""
    return None if x is None else _flat_dev(x, (rows,), keep)


def _flat_dev(x, shape: tuple, keep: list):
    """An array without a level index as a device pointer: an int device address or a numpy array of `shape`."""
    if isinstance(x, (int, np.integer)):
        return C.c_void_p(int(x))
    a = np.ascontiguousarray(x, dtype=np.float64)
    assert a.shape == shape, f"expected shape {shape}, got {a.shape}"
    b = DeviceBuffer(a)
    keep.append(b)
    return C.c_void_p(b.ptr)


def tracer_rows_ptr(tracers: Tracers, index: int, time_level: int = 0) -> int:
    """Device address of the rows of tracer `index` ([NCellsSize][level_pitch(K)]) in the tracer array: a view
    with no copy, what Eos.compute_spec_vol takes for T and S."""
    if not 0 <= index < tracers.NT:
        raise OmegaAmdError(f"tracer index {index} out of range (0..{tracers.NT - 1})")
    return tracers.device_ptr(time_level) + index * tracers.mesh.NCellsSize * level_pitch(tracers.K) * 8


class Eos(_Handle, _NamedArrays):
    """Eos (omega_amd/csrc/Eos.h): specific volume, linear or TEOS-10.  Level-indexed inputs are numpy arrays
    [NCellsSize][K] or device addresses of [NCellsSize][level_pitch(K)] doubles."""
    _destroy, _arrays = "omg_eos_destroy", "omg_eos"

    def __init__(self, mesh: HorzMesh, nvertlayers: int, eos_type: str = "teos10", drhodt: float = -0.2,
                 drhods: float = 0.8, rhot0s0: float = 1000.0):
        self.mesh, self.K = mesh, nvertlayers
        self._create("omg_eos_create", mesh.h, nvertlayers, eos_type.encode(), drhodt, drhods, rhot0s0)

    def compute_spec_vol(self, conserv_temp, abs_salinity, pressure, p_scale: float = 1.0, stream=None):
        keep, n = [], self.mesh.NCellsSize
        _chk(lib().omg_eos_compute_spec_vol(self.h, _level_dev(conserv_temp, n, self.K, keep),
                                            _level_dev(abs_salinity, n, self.K, keep),
                                            _level_dev(pressure, n, self.K, keep), p_scale, _sh(stream)))
        if keep:
            device_synchronize()

    def compute_spec_vol_disp(self, conserv_temp, abs_salinity, pressure, kdisp: int, p_scale: float = 1.0,
                              stream=None):
        keep, n = [], self.mesh.NCellsSize
        _chk(lib().omg_eos_compute_spec_vol_disp(self.h, _level_dev(conserv_temp, n, self.K, keep),
                                                 _level_dev(abs_salinity, n, self.K, keep),
                                                 _level_dev(pressure, n, self.K, keep), kdisp, p_scale, _sh(stream)))
        if keep:
            device_synchronize()

    def _shape(self, name):
        return (self.mesh.NCellsSize, self.K)


VCOORD_SHAPES = {"PressureInterface": "CK1", "PressureMid": "CK", "ZInterface": "CK1", "ZMid": "CK",
                 "GeopotentialMid": "CK", "LayerThicknessTarget": "CK", "RefLayerThickness": "CK",
                 "VertCoordMovementWeights": "K", "BottomDepth": "C"}
VCOORD_I4 = {"MinLayerCell": "C", "MaxLayerCell": "C", "MinLayerEdgeTop": "E", "MaxLayerEdgeTop": "E",
             "MinLayerEdgeBot": "E", "MaxLayerEdgeBot": "E", "MinLayerVertexTop": "V", "MaxLayerVertexTop": "V",
             "MinLayerVertexBot": "V", "MaxLayerVertexBot": "V"}


class VertCoord(_Handle, _NamedArrays):
    """VertCoord (omega_amd/csrc/VertCoord.h): layer ranges, pressure, z-height, geopotential, target thickness and
    the fused column pass.  min_level_cell / max_level_cell: the mesh file's global 1-based arrays [nCells], gathered
    through `decomp` (default: the mesh's)."""
    _destroy, _arrays, _i4 = "omg_vcoord_destroy", "omg_vcoord", VCOORD_I4

    def __init__(self, mesh: HorzMesh, nvertlayers: int, rho0: float = 1026.0, movement_weight_type: str = "Uniform",
                 min_level_cell=None, max_level_cell=None, decomp: Decomp | None = None):
        self.mesh, self.K = mesh, nvertlayers
        d = decomp if decomp is not None else getattr(mesh, "decomp", None)
        mn = None if min_level_cell is None else np.ascontiguousarray(min_level_cell, dtype=np.int32)
        mx = None if max_level_cell is None else np.ascontiguousarray(max_level_cell, dtype=np.int32)
        self._create("omg_vcoord_create", mesh.h, _sh(d), nvertlayers, rho0, movement_weight_type.encode(), _pi(mn), _pi(mx))

    def min_max_layer_edge(self, stream=None):
        _chk(lib().omg_vcoord_min_max_layer_edge(self.h, _sh(stream)))

    def min_max_layer_vertex(self, stream=None):
        _chk(lib().omg_vcoord_min_max_layer_vertex(self.h, _sh(stream)))

    def compute_pressure(self, layer_thickness, surface_pressure=None, stream=None):
        keep, n = [], self.mesh.NCellsSize
        _chk(lib().omg_vcoord_compute_pressure(self.h, _level_dev(layer_thickness, n, self.K, keep),
                                               _cell_dev(surface_pressure, n, keep), _sh(stream)))
        if keep:
            device_synchronize()

    def compute_zheight(self, layer_thickness, spec_vol, stream=None):
        keep, n = [], self.mesh.NCellsSize
        _chk(lib().omg_vcoord_compute_zheight(self.h, _level_dev(layer_thickness, n, self.K, keep),
                                              _level_dev(spec_vol, n, self.K, keep), _sh(stream)))
        if keep:
            device_synchronize()

    def compute_geopotential(self, tidal_potential=None, self_attraction_loading=None, stream=None):
        keep, n = [], self.mesh.NCellsSize
        _chk(lib().omg_vcoord_compute_geopotential(self.h, _cell_dev(tidal_potential, n, keep),
                                                   _cell_dev(self_attraction_loading, n, keep), _sh(stream)))
        if keep:
            device_synchronize()

    def compute_target_thickness(self, stream=None):
        _chk(lib().omg_vcoord_compute_target_thickness(self.h, _sh(stream)))

    def compute_column(self, state: OceanState, tracers: Tracers, eos: Eos, surface_pressure=None,
                       tidal_potential=None, self_attraction_loading=None, kdisp: int | None = None,
                       thick_tl: int = 0, tracer_tl: int = 0, temp_index: int = 0, salt_index: int = 1, stream=None):
        """The fused pass: PressureInterface/Mid, eos.SpecVol (pressure PressureMid * 1e-4 dbar), ZInterface/ZMid,
        GeopotentialMid -- and eos.SpecVolDisplaced when kdisp is given -- in one launch."""
        keep, n = [], self.mesh.NCellsSize
        _chk(lib().omg_vcoord_compute_column(self.h, state.h, thick_tl, tracers.h, tracer_tl, eos.h, temp_index,
                                             salt_index, _cell_dev(surface_pressure, n, keep),
                                             _cell_dev(tidal_potential, n, keep),
                                             _cell_dev(self_attraction_loading, n, keep), int(kdisp is not None),
                                             int(kdisp or 0), _sh(stream)))
        if keep:
            device_synchronize()

    def _shape(self, name):
        m = self.mesh
        spec = VCOORD_I4[name] if name in VCOORD_I4 else VCOORD_SHAPES.get(name, "CK")
        rows = {"C": m.NCellsSize, "E": m.NEdgesSize, "V": m.NVerticesSize}
        if spec == "K":
            return (self.K,)
        if spec == "CK":
            return (rows["C"], self.K)
        if spec == "CK1":
            return (rows["C"], self.K + 1)
        return (rows[spec],)

    def get_real(self, name: str) -> float:
        return _out(C.c_double, lib().omg_vcoord_get_real, self.h, name.encode())


class VertMixConfig(C.Structure):
    """omg_vertmix_config (VerticalMixingCoeff.md section 4.1.1)"""
    _fields_ = _mirror("omg_vertmix_config")


def vertmix_config(**over) -> VertMixConfig:
    """The defaults (omg_vertmix_config_default) with the given fields replaced; an unknown field raises KeyError."""
    return _config(VertMixConfig, "omg_vertmix_config_default", over)


class VertMix(_Handle, _NamedArrays):
    """VertMix (omega_amd/csrc/VertMix.h): N^2, mixing coefficients and the implicit vertical diffusion of tracers and
    normal velocity.  `config` fields as in VertMixConfig (e.g. ShearExponent=3.0, EnableConvectiveMix=False).
    Level-indexed inputs are numpy arrays [rows][K] or device addresses of [rows][level_pitch(K)] doubles; the in-place
    solves take a device address (solved asynchronously on `stream`) or a numpy array (staged, solved, returned)."""
    _destroy, _arrays = "omg_vertmix_destroy", "omg_vertmix"

    def __init__(self, mesh: HorzMesh, vcoord: "VertCoord | None", **config):
        self.mesh, self.vcoord = mesh, vcoord
        self.K = vcoord.K if vcoord is not None else mesh.NVertLayers
        self.config = vertmix_config(**config)
        self._create("omg_vertmix_create", mesh.h, _sh(vcoord), C.byref(self.config))

    def compute_bvf(self, eos: Eos, stream=None):
        _chk(lib().omg_vertmix_compute_bvf(self.h, eos.h, _sh(stream)))

    def compute(self, normal_velocity, tangential_velocity, bvf=None, stream=None):
        """VertVisc, VertDiff from the edge velocities and N^2 (bvf None: this object's BruntVaisalaFreqSq)"""
        keep, ne, nc = [], self.mesh.NEdgesSize, self.mesh.NCellsSize
        _chk(lib().omg_vertmix_compute(self.h, _level_dev(normal_velocity, ne, self.K, keep),
                                       _level_dev(tangential_velocity, ne, self.K, keep),
                                       None if bvf is None else _level_dev(bvf, nc, self.K, keep), _sh(stream)))
        if keep:
            device_synchronize()

    def apply_tracers(self, layer_thickness, tracers, ntracers: int, dt: float, stream=None, surface_flux=None):
        """Backward-Euler diffusion of tracers [ntracers][NCellsSize][K] with VertDiff, all in one pass.  surface_flux
        (a numpy array [ntracers][NCellsSize] or a device address; tracer units * m/s, positive into the ocean) goes
        through the forced solve; None calls the unforced entry point."""
        keep, n = [], self.mesh.NCellsSize
        h = _level_dev(layer_thickness, n, self.K, keep)
        p, buf = _stage_levels(tracers, (int(ntracers), n), self.K)
        if surface_flux is None:
            _chk(lib().omg_vertmix_apply_tracers(self.h, h, p, ntracers, dt, _sh(stream)))
        else:
            f = _flat_dev(surface_flux, (int(ntracers), n), keep)
            _chk(lib().omg_vertmix_apply_tracers_forced(self.h, h, p, ntracers, dt, f, _sh(stream)))
            if keep:
                device_synchronize()
        return _read_back(buf, self.K, stream)

    def apply_velocity(self, layer_thickness, normal_velocity, dt: float, stream=None, boundary=None, stress=None,
                       ut=None):
        """Backward-Euler diffusion of the normal velocity [NEdgesSize][K] with VertVisc averaged to the edges.
        boundary = (BottomDragCoeff, RayleighDragCoeff), stress [NEdgesSize] (Pa) and ut [NEdgesSize][K] (needed with a
        bottom drag) go through the forced solve; with all three None the unforced entry point is called."""
        keep = []
        h = _level_dev(layer_thickness, self.mesh.NCellsSize, self.K, keep)
        p, buf = _stage_levels(normal_velocity, (self.mesh.NEdgesSize,), self.K)
        if boundary is None and stress is None and ut is None:
            _chk(lib().omg_vertmix_apply_velocity(self.h, h, p, dt, _sh(stream)))
        else:
            cd, ra = boundary if boundary is not None else (0.0, 0.0)
            ne = self.mesh.NEdgesSize
            t = None if stress is None else _flat_dev(stress, (ne,), keep)
            v = None if ut is None else _level_dev(ut, ne, self.K, keep)
            _chk(lib().omg_vertmix_apply_velocity_forced(self.h, h, p, dt, cd, ra, t, v, _sh(stream)))
            if keep:
                device_synchronize()
        return _read_back(buf, self.K, stream)

    def _shape(self, name):
        return (self.mesh.NCellsSize, self.K)


class VertMixStep(_Handle, _NamedArrays):
    """VertMixStep (omega_amd/csrc/VertMixStep.h): the displaced column pass, N^2, the tangential velocity, the
    coefficients and the forced tracer and velocity solves as one call.  Its arrays (TangentialVelocity,
    NormalStressEdge, SurfaceTracerFlux, SurfacePressure, TidalPotential, SelfAttractionLoading) are zero at creation
    and set with `set`; the coefficients and the wind-stress switch with `set_boundary`."""
    _destroy, _arrays = "omg_vertmix_step_destroy", "omg_vertmix_step"

    def __init__(self, mesh: HorzMesh, vert_mix: "VertMix | None", vcoord: "VertCoord | None", eos: "Eos | None",
                 ntracers: int):
        self.mesh, self.vert_mix, self.vcoord, self.eos, self.NT = mesh, vert_mix, vcoord, eos, int(ntracers)
        self.K = vcoord.K if vcoord is not None else mesh.NVertLayers
        self._create("omg_vertmix_step_create", mesh.h, _sh(vert_mix), _sh(vcoord), _sh(eos), ntracers)

    def set_boundary(self, bottom_drag_coeff: float = 0.0, rayleigh_drag_coeff: float = 0.0,
                     use_wind_stress: bool = False):
        _chk(lib().omg_vertmix_step_set_boundary(self.h, bottom_drag_coeff, rayleigh_drag_coeff, use_wind_stress))

    def attach_redi(self, redi: "Redi | None"):
        """VertMixStep::attachRedi: apply adds `redi`'s VertDiffusivity (from the slopes it last computed) to the
        VertMix's VertDiff before the tracer solve; None detaches."""
        _chk(lib().omg_vertmixstep_attach_redi(self.h, _sh(redi)))
        self._redi = redi  # the library keeps a pointer to it

    def attach_kpp(self, kpp: "Kpp | None"):
        """VertMixStep::attachKpp: apply runs `kpp`'s compute after the coefficients and its non-local redistribution
        of SurfaceTracerFlux before the tracer solve; None detaches."""
        _chk(lib().omg_vmix_step_attach_kpp(self.h, _sh(kpp)))
        self._kpp = kpp  # the library keeps a pointer to it

    def apply(self, layer_thickness: int, normal_velocity: int, tracers: int, dt: float, stream=None):
        """On device addresses: thickness [NCellsSize][pitch]; velocity [NEdgesSize][pitch] and tracers
        [NT][NCellsSize][pitch] are mixed in place, asynchronously on `stream`."""
        _chk(lib().omg_vertmix_step_apply(self.h, int(layer_thickness), int(normal_velocity), int(tracers), dt, _sh(stream)))

    def apply_state(self, state: OceanState, tracers: Tracers, dt: float, time_level: int = 0,
                    tracer_time_level: int = 0, stream=None):
        _chk(lib().omg_vertmix_step_apply_state(self.h, state.h, time_level, tracers.h, tracer_time_level, dt, _sh(stream)))

    def _shape(self, name):
        m = self.mesh
        return {"TangentialVelocity": (m.NEdgesSize, self.K), "NormalStressEdge": (m.NEdgesSize,),
                "SurfaceTracerFlux": (self.NT, m.NCellsSize)}.get(name, (m.NCellsSize,))


class KppConfig(C.Structure):
    """omg_kpp_config (omega_amd/csrc/Kpp.h)"""
    _fields_ = _mirror("omg_kpp_config")


def kpp_config(**over) -> KppConfig:
    """The defaults (omg_kpp_config_default) with the given fields replaced; an unknown field raises KeyError."""
    return _config(KppConfig, "omg_kpp_config_default", over)


class Kpp(_Handle, _NamedArrays):
    """Kpp (omega_amd/csrc/Kpp.h): K-profile boundary-layer mixing on top of `vert_mix` -- the boundary-layer depth from
    a bulk Richardson number, the K-profile viscosity and diffusivity inside the layer (compute) and the non-local
    redistribution of a surface tracer flux (apply_non_local).  `config` fields as in KppConfig (e.g. Cv=1.5).  The
    caller sets "FrictionVelocity" and "SurfaceBuoyancyFlux" ([NCellsSize]) with `set`; the results are
    "BoundaryLayerDepth", "BoundaryLayerIndex" (int32), "BulkRichardson" and "NonLocalShape" (`get`).  Level-indexed
    inputs are numpy arrays [rows][K] or device addresses of [rows][level_pitch(K)] doubles."""
    _destroy, _arrays, _i4 = "omg_kpp_destroy", "omg_kpp", ("BoundaryLayerIndex",)

    def __init__(self, mesh: HorzMesh, vcoord: "VertCoord | None", vert_mix: "VertMix | None", **config):
        self.mesh, self.vcoord, self.vert_mix = mesh, vcoord, vert_mix
        self.K = vcoord.K if vcoord is not None else mesh.NVertLayers
        self.config = kpp_config(**config)
        self._create("omg_kpp_create", mesh.h, _sh(vcoord), _sh(vert_mix), C.byref(self.config))

    def constants(self) -> tuple:
        """(VtCoef, NonLocalCoeff) as formed at creation"""
        a, b = C.c_double(), C.c_double()
        _chk(lib().omg_kpp_constants(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def compute(self, normal_velocity, tangential_velocity, bvf=None, z_mid=None, z_interface=None, vert_diff=None,
                vert_visc=None, stream=None):
        """The boundary layer from the edge velocities: on the five given cell arrays (the array form; all five or
        none; z_interface is [NCellsSize][K + 1]), or on the VertMix's and the VertCoord's arrays as they stand.
        vert_diff and vert_visc are rewritten inside the layer: device addresses, or numpy arrays (staged, computed and
        returned as a pair)."""
        keep, ne, nc = [], self.mesh.NEdgesSize, self.mesh.NCellsSize
        un = _level_dev(normal_velocity, ne, self.K, keep)
        ut = _level_dev(tangential_velocity, ne, self.K, keep)
        given = [a is not None for a in (bvf, z_mid, z_interface, vert_diff, vert_visc)]
        if not any(given):
            _chk(lib().omg_kpp_compute(self.h, un, ut, _sh(stream)))
            if keep:
                device_synchronize()
            return None
        if not all(given):
            raise OmegaAmdError("Kpp.compute: the array form takes bvf, z_mid, z_interface, vert_diff and vert_visc together")
        n2 = _level_dev(bvf, nc, self.K, keep)
        zm = _level_dev(z_mid, nc, self.K, keep)
        zi = _level_dev(z_interface, nc, self.K + 1, keep)
        pd, bd = _stage_levels(vert_diff, (nc,), self.K)
        pv, bv = _stage_levels(vert_visc, (nc,), self.K)
        _chk(lib().omg_kpp_compute_arrays(self.h, un, ut, n2, zm, zi, pd, pv, _sh(stream)))
        if keep or bd is not None or bv is not None:
            if stream is not None:
                stream.synchronize()
            device_synchronize()
        return _read_back(bd, self.K, stream), _read_back(bv, self.K, stream)

    def apply_non_local(self, layer_thickness, tracers, ntracers: int, dt: float, surface_flux=None, stream=None):
        """tracers [ntracers][NCellsSize][K] take the counter-gradient part of surface_flux ([ntracers][NCellsSize], a
        numpy array or a device address; None: nothing is done) on NonLocalShape as it stands; in place on a device
        address, or a numpy array (staged, computed, returned)."""
        keep, n = [], self.mesh.NCellsSize
        h = _level_dev(layer_thickness, n, self.K, keep)
        p, buf = _stage_levels(tracers, (int(ntracers), n), self.K)
        f = None if surface_flux is None else _flat_dev(surface_flux, (int(ntracers), n), keep)
        _chk(lib().omg_kpp_apply_non_local(self.h, h, p, ntracers, dt, f, _sh(stream)))
        if keep:
            device_synchronize()
        return _read_back(buf, self.K, stream)

    def launch_count(self) -> int:
        """kernel launches compute and apply_non_local have issued on this object so far"""
        return _out(C.c_int64, lib().omg_kpp_launch_count, self.h)

    def _shape(self, name):
        m = self.mesh
        return (m.NCellsSize, self.K) if name in ("BulkRichardson", "NonLocalShape") else (m.NCellsSize,)


PGRAD_ARRAYS = ("SurfacePressure", "TidalPotential", "SelfAttractionLoading")


class _ColumnPass:
    """What PressureGrad, GentMcWilliams and Redi share (omega_amd/csrc/ColumnPass.h): the mesh, VertCoord and Eos they
    are built on, the column pass with the object's own forcing, and the staging of a stratification given as arrays.
    `_arrays` is also the prefix of the class's C symbols."""

    def _create_on(self, mesh: HorzMesh, vcoord: "VertCoord | None", eos: "Eos | None", *args):
        self.mesh, self.vcoord, self.eos = mesh, vcoord, eos
        self.K = vcoord.K if vcoord is not None else mesh.NVertLayers
        self._create(self._arrays + "_create", mesh.h, _sh(vcoord), _sh(eos), *args)

    def _update_column(self, layer_thickness, tracers, ntracers: int, stream):
        keep, n = [], self.mesh.NCellsSize
        h = _level_dev(layer_thickness, n, self.K, keep)
        t = _stage_levels(tracers, (int(ntracers), n), self.K, keep)[0]
        _chk(getattr(lib(), self._arrays + "_update_column")(self.h, h, t, ntracers, _sh(stream)))
        if keep:
            device_synchronize()

    def _stratification(self, spec_vol, spec_vol_displaced, z_mid, keep: list):
        """the three cell arrays staged on the device (all three or none: then None, the objects' arrays as they stand)"""
        given = [x is not None for x in (spec_vol, spec_vol_displaced, z_mid)]
        assert all(given) or not any(given), "give SpecVol, SpecVolDisplaced and ZMid, or none of them"
        if not all(given):
            return None
        return [_level_dev(x, self.mesh.NCellsSize, self.K, keep) for x in (spec_vol, spec_vol_displaced, z_mid)]


class PressureGrad(_Handle, _NamedArrays, _ColumnPass):
    """PressureGrad (omega_amd/csrc/PressureGrad.h): the layered-ocean pressure-gradient force on edges,
    Tend -= EdgeMask * (grad GeopotentialMid + 0.5 (SpecVol0 + SpecVol1) grad PressureMid), from the column fields of
    `vcoord` and `eos`.  Level-indexed inputs are numpy arrays [rows][K] or device addresses of [rows][level_pitch(K)]
    doubles; `tend` is accumulated in place: a device address (asynchronous on `stream`) or a numpy array (staged,
    computed, returned)."""
    _destroy, _arrays = "omg_pgrad_destroy", "omg_pgrad"

    def __init__(self, mesh: HorzMesh, vcoord: "VertCoord | None", eos: "Eos | None"):
        self._create_on(mesh, vcoord, eos)

    def update_column(self, layer_thickness, tracers, ntracers: int, stream=None):
        """The fused column pass from raw arrays: thickness [NCellsSize][K], tracers [ntracers][NCellsSize][K]
        (temperature 0, salinity 1), with this object's SurfacePressure / TidalPotential / SelfAttractionLoading."""
        self._update_column(layer_thickness, tracers, ntracers, stream)

    def compute(self, tend, pressure_mid=None, geopotential_mid=None, spec_vol=None, stream=None):
        """tend -= the term: from the three given cell arrays (the array form; all three or none), or from the
        VertCoord's and the Eos's arrays as they stand."""
        given = [x is not None for x in (pressure_mid, geopotential_mid, spec_vol)]
        assert all(given) or not any(given), "give PressureMid, GeopotentialMid and SpecVol, or none of them"
        p, buf = _stage_levels(tend, (self.mesh.NEdgesSize,), self.K)
        keep, n = [], self.mesh.NCellsSize
        if all(given):
            _chk(lib().omg_pgrad_compute_arrays(self.h, p, _level_dev(pressure_mid, n, self.K, keep),
                                                _level_dev(geopotential_mid, n, self.K, keep),
                                                _level_dev(spec_vol, n, self.K, keep), _sh(stream)))
        else:
            _chk(lib().omg_pgrad_compute(self.h, p, _sh(stream)))
        if keep:
            device_synchronize()
        return _read_back(buf, self.K, stream)

    def _shape(self, name):
        return (self.mesh.NCellsSize,)


class VertAdv(_Handle, _NamedArrays):
    """VertAdv (omega_amd/csrc/VertAdv.h): the vertical transport that holds the layers to the VertCoord's z-star /
    z-level shape and the vertical advection of thickness, tracers and momentum.  Level-indexed inputs are numpy arrays
    [rows][K] or device addresses of [rows][level_pitch(K)] doubles; a tendency is accumulated in place: a device
    address (asynchronous on `stream`) or a numpy array (staged, computed, returned)."""
    _destroy, _arrays = "omg_vertadv_destroy", "omg_vertadv"

    def __init__(self, mesh: HorzMesh, vcoord: "VertCoord | None", tracer_flux_order: int = 2):
        self.mesh, self.vcoord, self.order = mesh, vcoord, tracer_flux_order
        self.K = vcoord.K if vcoord is not None else mesh.NVertLayers
        self._create("omg_vertadv_create", mesh.h, _sh(vcoord), tracer_flux_order)

    @staticmethod
    def max_layers() -> int:
        return _out(C.c_int, lib().omg_vertadv_max_layers)

    def compute_transport(self, thickness_tend, add_thickness: bool = False, stream=None):
        """VerticalTransport from the horizontal thickness tendency; add_thickness: also the thickness update, in the
        same launch (computeAndAddThickness)"""
        p, buf = _stage_levels(thickness_tend, (self.mesh.NCellsSize,), self.K)
        _chk(lib().omg_vertadv_compute_transport(self.h, p, bool(add_thickness), _sh(stream)))
        return _read_back(buf, self.K, stream)

    def add_thickness(self, thickness_tend, stream=None):
        p, buf = _stage_levels(thickness_tend, (self.mesh.NCellsSize,), self.K)
        _chk(lib().omg_vertadv_add_thickness(self.h, p, _sh(stream)))
        return _read_back(buf, self.K, stream)

    def add_tracers(self, tracer_tend, layer_thickness, tracers, ntracers: int, stream=None):
        keep, n = [], self.mesh.NCellsSize
        h = _level_dev(layer_thickness, n, self.K, keep)
        t = _stage_levels(tracers, (int(ntracers), n), self.K, keep)[0]
        p, buf = _stage_levels(tracer_tend, (int(ntracers), n), self.K)
        _chk(lib().omg_vertadv_add_tracers(self.h, p, h, t, ntracers, _sh(stream)))
        if keep:
            device_synchronize()
        return _read_back(buf, self.K, stream)

    def set_tracer_term(self, on: bool):
        """VertAdv::TracerTermEnable (default on): off, a Tendencies this object is attached to leaves its tracer term
        out -- for a MonotoneAdv that limits the vertical flux itself (MonotoneAdv.attach_vert_adv).  add_tracers
        called directly does not look at it."""
        _chk(lib().omg_vertadv_set_tracer_term(self.h, bool(on)))

    def add_velocity(self, velocity_tend, layer_thickness, normal_velocity, stream=None):
        keep = []
        h = _level_dev(layer_thickness, self.mesh.NCellsSize, self.K, keep)
        u = _level_dev(normal_velocity, self.mesh.NEdgesSize, self.K, keep)
        p, buf = _stage_levels(velocity_tend, (self.mesh.NEdgesSize,), self.K)
        _chk(lib().omg_vertadv_add_velocity(self.h, p, h, u, _sh(stream)))
        if keep:
            device_synchronize()
        return _read_back(buf, self.K, stream)

    def _shape(self, name):
        return (self.mesh.NCellsSize, self.K)


def monotone_adv_high_order_tables(mesh: "HorzMesh", order: int, coef_3rd_order: float = 0.25, sphere_radius: float = 0.0,
                                   x_period: float = 0.0, y_period: float = 0.0) -> dict:
    """omg_monoadv_high_order_tables: the tables MonotoneAdv.set_horz_order builds on `mesh` (host-only will do), as
    {"FitCell" [NCellsSize], "HessWeight", "EdgeDirOwn", "EdgeDirAcross" [NCellsSize][MaxEdges][3]}"""
    n, me = mesh.NCellsSize, mesh.MaxEdges
    out = {"FitCell": np.zeros(n), "HessWeight": np.zeros((n, me, 3)), "EdgeDirOwn": np.zeros((n, me, 3)),
           "EdgeDirAcross": np.zeros((n, me, 3))}
    _chk(lib().omg_monoadv_high_order_tables(mesh.h, order, coef_3rd_order, sphere_radius, x_period, y_period,
                                             *(_pd(a) for a in out.values())))
    return out


class MonotoneAdv(_Handle, _NamedArrays):
    """MonotoneAdv (omega_amd/csrc/MonotoneAdv.h): flux-corrected horizontal tracer advection -- the centred edge flux
    limited against the upwind one, so that a forward update over `dt` creates no new extremum.  Level-indexed inputs
    are numpy arrays [rows][K] or device addresses of [rows][level_pitch(K)] doubles; the tendency is accumulated in
    place: a device address (asynchronous on `stream`) or a numpy array (staged, computed, returned).  The named arrays
    are "ScaleIn" and "ScaleOut", [max_tracers][NCellsSize][K], and after set_horz_order(3 or 4) those it names."""
    _destroy, _arrays = "omg_monoadv_destroy", "omg_monoadv"

    def __init__(self, mesh: HorzMesh, nvertlayers: int, max_tracers: int, flux_thickness_upwind: bool = False):
        self.mesh, self.K, self.max_tracers = mesh, int(nvertlayers), int(max_tracers)
        self.flux_thickness_upwind = bool(flux_thickness_upwind)
        self._create("omg_monoadv_create", _sh(mesh), nvertlayers, max_tracers, self.flux_thickness_upwind)

    def attach_vert_adv(self, vert_adv: "VertAdv | None"):
        """MonotoneAdv::attachVertAdv: while attached add_tracers limits the vertical flux of `vert_adv`'s
        VerticalTransport (as it stands) together with the horizontal ones; None detaches."""
        _chk(lib().omg_monoadv_attach_vert_adv(self.h, _sh(vert_adv)))
        self.vert_adv = vert_adv  # (the C++ object keeps the pointer)

    def add_tracers(self, tracer_tend, h_old, h_new, normal_velocity, tracers, ntracers: int, dt: float, stream=None):
        keep, n, nt = [], self.mesh.NCellsSize, max(int(ntracers), 0)
        ho = _level_dev(h_old, n, self.K, keep)
        hn = _level_dev(h_new, n, self.K, keep)
        u = _level_dev(normal_velocity, self.mesh.NEdgesSize, self.K, keep)
        t = _stage_levels(tracers, (nt, n), self.K, keep)[0]
        p, buf = _stage_levels(tracer_tend, (nt, n), self.K)
        _chk(lib().omg_monoadv_add_tracers(self.h, p, ho, hn, u, t, ntracers, dt, _sh(stream)))
        if keep:
            device_synchronize()
        return _read_back(buf, self.K, stream)

    def set_horz_order(self, order: int, coef_3rd_order: float = 0.25, sphere_radius: float = 0.0,
                       x_period: float = 0.0, y_period: float = 0.0):
        """MonotoneAdv::setHorzOrder: 2 the centred flux (the state at creation), 4 the fourth-order flux, 3 the
        third-order one with the upwind-biased term times `coef_3rd_order` (in (0, 1]).  Orders 3 and 4 build the
        tables from the mesh's cell positions -- on a sphere of `sphere_radius` (0: planar, with the periods of a
        periodic mesh) -- and add the named arrays "Hess" [max_tracers][3][NCellsSize][K], "HessWeight", "EdgeDirOwn",
        "EdgeDirAcross" [NCellsSize][MaxEdges][3] and "FitCell" [NCellsSize]; add_tracers then makes three launches."""
        _chk(lib().omg_monoadv_set_horz_order(self.h, order, coef_3rd_order, sphere_radius, x_period, y_period))
        self.horz_order = int(order)

    def launch_count(self) -> int:
        """kernel launches add_tracers has issued on this object so far"""
        return _out(C.c_int64, lib().omg_monoadv_launch_count, self.h)

    def _shape(self, name):
        if name == "Hess":
            return (self.max_tracers, 3, self.mesh.NCellsSize, self.K)
        if name in ("HessWeight", "EdgeDirOwn", "EdgeDirAcross"):
            return (self.mesh.NCellsSize, self.mesh.MaxEdges, 3)
        if name == "FitCell":
            return (self.mesh.NCellsSize,)
        return (self.max_tracers, self.mesh.NCellsSize, self.K)


BTR_ARRAYS = {"BtrVelocity": "E", "BtrThickEdge": "E", "BtrForcing": "E", "BtrFluxMean": "E", "BtrTendMean": "E",
              "SSH": "C", "BclVelocity": "EK"}


class BarotropicMode(_Handle, _NamedArrays):
    """BarotropicMode (omega_amd/csrc/BarotropicMode.h): the split of the edge velocity into its thickness-weighted
    vertical mean (BtrVelocity) and the baroclinic remainder (BclVelocity), the sea-surface height of the columns, and
    forward-backward sub-cycling of the 2-D (SSH, BtrVelocity) system under BtrForcing.  Level-indexed inputs are numpy
    arrays [rows][K] or device addresses of [rows][level_pitch(K)] doubles; every call is one library call,
    asynchronous on `stream` when it is given device addresses."""
    _destroy, _arrays = "omg_btr_destroy", "omg_btr"

    def __init__(self, mesh: HorzMesh, vcoord: "VertCoord | None", gravity: float = 9.80616):
        self.mesh, self.vcoord, self.gravity = mesh, vcoord, float(gravity)
        self.K = vcoord.K if vcoord is not None else mesh.NVertLayers
        self._create("omg_btr_create", mesh.h, _sh(vcoord), gravity)

    @staticmethod
    def max_layers() -> int:
        return _out(C.c_int, lib().omg_btr_max_layers)

    def _edge_call(self, symbol, layer_thickness, edge_field, *args, stream=None):
        keep = []
        h = _level_dev(layer_thickness, self.mesh.NCellsSize, self.K, keep)
        u = _level_dev(edge_field, self.mesh.NEdgesSize, self.K, keep)
        _chk(getattr(lib(), symbol)(self.h, h, u, *args, _sh(stream)))
        if keep:
            device_synchronize()

    def split_velocity(self, layer_thickness, normal_velocity, with_ssh: bool = False, stream=None):
        """BtrThickEdge, BtrVelocity and BclVelocity; with_ssh: also compute_ssh, in the same launch"""
        self._edge_call("omg_btr_split_velocity", layer_thickness, normal_velocity, bool(with_ssh), stream=stream)

    def compute_forcing(self, layer_thickness, velocity_tend, stream=None):
        self._edge_call("omg_btr_compute_forcing", layer_thickness, velocity_tend, stream=stream)

    def compute_ssh(self, layer_thickness, stream=None):
        keep = []
        h = _level_dev(layer_thickness, self.mesh.NCellsSize, self.K, keep)
        _chk(lib().omg_btr_compute_ssh(self.h, h, _sh(stream)))
        if keep:
            device_synchronize()

    def recombine(self, normal_velocity, stream=None):
        """normal_velocity = BclVelocity + BtrVelocity on each edge's level range, in place: a device address, or a
        numpy array (staged, computed, returned)"""
        p, buf = _stage_levels(normal_velocity, (self.mesh.NEdgesSize,), self.K)
        _chk(lib().omg_btr_recombine(self.h, p, _sh(stream)))
        return _read_back(buf, self.K, stream)

    def subcycle(self, nsub: int, dt_btr: float, stream=None):
        _chk(lib().omg_btr_subcycle(self.h, nsub, dt_btr, _sh(stream)))

    def compute_residual_forcing(self, layer_thickness, velocity_tend, stream=None):
        """BtrTendMean (the vertical mean of velocity_tend) and BtrForcing = BtrTendMean less the sub-step's bracket at
        SSH and BtrVelocity as they stand"""
        self._edge_call("omg_btr_compute_residual_forcing", layer_thickness, velocity_tend, stream=stream)

    def transport_velocity(self, velocity_old, velocity_out, stream=None):
        """velocity_out = BclVelocity + BtrFluxMean/BtrThickEdge on each edge's level range, velocity_old elsewhere;
        device addresses of [NEdgesSize][level_pitch(K)] doubles"""
        _chk(lib().omg_btr_transport_velocity(self.h, velocity_old, velocity_out, _sh(stream)))

    def advance_velocity(self, velocity_old, velocity_tend, dt: float, velocity_out, stream=None):
        """velocity_out = (BclVelocity + dt*(velocity_tend - BtrTendMean)) + BtrVelocity on each edge's level range,
        velocity_old + dt*velocity_tend elsewhere; device addresses, velocity_out may be velocity_old"""
        _chk(lib().omg_btr_advance_velocity(self.h, velocity_old, velocity_tend, dt, velocity_out, _sh(stream)))

    def _shape(self, name):
        s = BTR_ARRAYS.get(name, "E")  # (an unknown name: the library says so)
        if s == "C":
            return (self.mesh.NCellsSize,)
        return (self.mesh.NEdgesSize, self.K) if s == "EK" else (self.mesh.NEdgesSize,)


GM_ARRAYS = {"Kappa": "E", "BolusVelocity": "EK", "StreamFunction": "EK", "SurfacePressure": "C",
             "TidalPotential": "C", "SelfAttractionLoading": "C"}


class GentMcWilliams(_Handle, _NamedArrays, _ColumnPass):
    """GentMcWilliams (omega_amd/csrc/GentMcWilliams.h): the eddy-induced (bolus) velocity of the Gent-McWilliams closure
    on the edges from the stratification of `vcoord` / `eos`, one tridiagonal solve per edge column.  Level-indexed
    inputs are numpy arrays [rows][K] or device addresses of [rows][level_pitch(K)] doubles; the results are the
    object's BolusVelocity and StreamFunction (`get`); `transport` is accumulated in place: a device address
    (asynchronous on `stream`) or a numpy array (staged, computed, returned)."""
    _destroy, _arrays = "omg_gm_destroy", "omg_gm"

    def __init__(self, mesh: HorzMesh, vcoord: "VertCoord | None", eos: "Eos | None", kappa: float = 600.0,
                 grav_wave_speed: float = 0.3):
        self._create_on(mesh, vcoord, eos, kappa, grav_wave_speed)

    def update_column(self, layer_thickness, tracers, ntracers: int, stream=None):
        """The fused column pass with the displaced volume (kdisp = 1) from raw arrays: thickness [NCellsSize][K],
        tracers [ntracers][NCellsSize][K] (temperature 0, salinity 1), with this object's SurfacePressure /
        TidalPotential / SelfAttractionLoading."""
        self._update_column(layer_thickness, tracers, ntracers, stream)

    def compute(self, layer_thickness, transport=None, spec_vol=None, spec_vol_displaced=None, z_mid=None, stream=None):
        """BolusVelocity and StreamFunction from the three given cell arrays (the array form; all three or none), or from
        the Eos's and the VertCoord's arrays as they stand; transport += BolusVelocity if it is given."""
        keep = []
        strat = self._stratification(spec_vol, spec_vol_displaced, z_mid, keep)
        p, buf = (None, None) if transport is None else _stage_levels(transport, (self.mesh.NEdgesSize,), self.K)
        h = _level_dev(layer_thickness, self.mesh.NCellsSize, self.K, keep)
        if strat:
            _chk(lib().omg_gm_compute_arrays(self.h, h, *strat, p, _sh(stream)))
        else:
            _chk(lib().omg_gm_compute(self.h, h, p, _sh(stream)))
        if keep:
            device_synchronize()
        return _read_back(buf, self.K, stream)

    def _shape(self, name):
        s = GM_ARRAYS.get(name, "C")  # (an unknown name: the library says so)
        if s == "C":
            return (self.mesh.NCellsSize,)
        return (self.mesh.NEdgesSize, self.K) if s == "EK" else (self.mesh.NEdgesSize,)


REDI_ARRAYS = {"Kappa": "E", "SlopeInterface": "EK", "VertDiffusivity": "CK", "SurfacePressure": "C",
               "TidalPotential": "C", "SelfAttractionLoading": "C"}


class Redi(_Handle, _NamedArrays, _ColumnPass):
    """Redi (omega_amd/csrc/Redi.h): isoneutral diffusion of the tracers -- the isopycnal slope relative to the layers on
    the edge interfaces from the stratification of `vcoord` / `eos` (compute_slope), the explicit cross terms of the
    small-slope tensor on a tracer tendency (add_tracer_tend) and its slope-squared part as a vertical diffusivity for
    VertMix's implicit solve (compute_vert_diffusivity).  Level-indexed inputs are numpy arrays [rows][K] or device
    addresses of [rows][level_pitch(K)] doubles; the results are the object's SlopeInterface and VertDiffusivity
    (`get`); `tracer_tend` and `vert_diff` are accumulated in place: a device address (asynchronous on `stream`) or a
    numpy array (staged, computed, returned)."""
    _destroy, _arrays = "omg_redi_destroy", "omg_redi"

    def __init__(self, mesh: HorzMesh, vcoord: "VertCoord | None", eos: "Eos | None", max_tracers: int,
                 kappa: float = 600.0, slope_max: float = 0.01, n2_floor: float = 1.0e-10):
        self.max_tracers = int(max_tracers)
        self._create_on(mesh, vcoord, eos, max_tracers, kappa, slope_max, n2_floor)

    def update_column(self, layer_thickness, tracers, ntracers: int, stream=None):
        """The fused column pass with the displaced volume (kdisp = 1) from raw arrays, as
        GentMcWilliams.update_column, with this object's SurfacePressure / TidalPotential / SelfAttractionLoading."""
        self._update_column(layer_thickness, tracers, ntracers, stream)

    def compute_slope(self, layer_thickness, spec_vol=None, spec_vol_displaced=None, z_mid=None, stream=None):
        """SlopeInterface from the three given cell arrays (the array form; all three or none), or from the Eos's and
        the VertCoord's arrays as they stand."""
        keep = []
        strat = self._stratification(spec_vol, spec_vol_displaced, z_mid, keep)
        h = _level_dev(layer_thickness, self.mesh.NCellsSize, self.K, keep)
        if strat:
            _chk(lib().omg_redi_compute_slope_arrays(self.h, h, *strat, _sh(stream)))
        else:
            _chk(lib().omg_redi_compute_slope(self.h, h, _sh(stream)))
        if keep:
            device_synchronize()

    def add_tracer_tend(self, tracer_tend, layer_thickness, tracers, ntracers: int, z_mid=None, stream=None):
        """tracer_tend [ntracers][NCellsSize][K] += the isoneutral cross terms of `tracers` on the slopes as they stand;
        z_mid None: the VertCoord's ZMid."""
        keep, n, nt = [], self.mesh.NCellsSize, max(int(ntracers), 0)
        h = _level_dev(layer_thickness, n, self.K, keep)
        t = _stage_levels(tracers, (nt, n), self.K, keep)[0]
        z = None if z_mid is None else _level_dev(z_mid, n, self.K, keep)
        p, buf = _stage_levels(tracer_tend, (nt, n), self.K)
        _chk(lib().omg_redi_add_tracer_tend(self.h, p, h, t, ntracers, z, _sh(stream)))
        if keep:
            device_synchronize()
        return _read_back(buf, self.K, stream)

    def compute_vert_diffusivity(self, vert_diff=None, stream=None):
        """VertDiffusivity from the slopes as they stand; vert_diff [NCellsSize][K] += VertDiffusivity if it is given."""
        p, buf = (None, None) if vert_diff is None else _stage_levels(vert_diff, (self.mesh.NCellsSize,), self.K)
        _chk(lib().omg_redi_compute_vert_diffusivity(self.h, p, _sh(stream)))
        return _read_back(buf, self.K, stream)

    def launch_count(self) -> int:
        """kernel launches the three compute calls have issued on this object so far"""
        return _out(C.c_int64, lib().omg_redi_launch_count, self.h)

    def _shape(self, name):
        s = REDI_ARRAYS.get(name, "C")  # (an unknown name: the library says so)
        m = self.mesh
        return {"C": (m.NCellsSize,), "E": (m.NEdgesSize,), "EK": (m.NEdgesSize, self.K), "CK": (m.NCellsSize, self.K)}[s]


class VertRemap(_Handle, _NamedArrays):
    """VertRemap (omega_amd/csrc/VertRemap.h): vertical Lagrangian remapping -- the target thickness of the VertCoord
    from the column totals of a thickness ("LayerThicknessTarget", [NCellsSize][K]) and the conservative remap of tracers
    and velocity from that thickness onto it, `order` 1 PCM, 2 PLM, 3 PPM.  Level-indexed arguments are numpy arrays
    [rows][K] or device addresses of [rows][level_pitch(K)] doubles; what a call changes in place is a device address
    (asynchronous on `stream`, nothing returned) or a numpy array (staged, computed, returned)."""
    _destroy, _arrays = "omg_vremap_destroy", "omg_vremap"

    def __init__(self, mesh: HorzMesh, vcoord: "VertCoord | None", max_tracers: int, order: int = 3):
        self.mesh, self.vcoord, self.order, self.max_tracers = mesh, vcoord, int(order), int(max_tracers)
        self.K = vcoord.K if vcoord is not None else (mesh.NVertLayers if mesh is not None else 0)
        self._create("omg_vremap_create", _sh(mesh), _sh(vcoord), order, max_tracers)

    @staticmethod
    def max_layers() -> int:
        return _out(C.c_int, lib().omg_vremap_max_layers)

    def compute_target(self, layer_thickness, stream=None):
        keep = []
        h = _level_dev(layer_thickness, self.mesh.NCellsSize, self.K, keep)
        _chk(lib().omg_vremap_compute_target(self.h, h, _sh(stream)))
        if keep:
            device_synchronize()

    def remap_tracers(self, layer_thickness, tracers, ntracers: int, stream=None):
        keep, n, nt = [], self.mesh.NCellsSize, max(int(ntracers), 0)
        h = _level_dev(layer_thickness, n, self.K, keep)
        p, buf = _stage_levels(tracers, (nt, n), self.K)
        _chk(lib().omg_vremap_remap_tracers(self.h, h, p, ntracers, _sh(stream)))
        if keep:
            device_synchronize()
        return _read_back(buf, self.K, stream)

    def remap_velocity(self, layer_thickness, normal_velocity, stream=None):
        keep = []
        h = _level_dev(layer_thickness, self.mesh.NCellsSize, self.K, keep)
        p, buf = _stage_levels(normal_velocity, (self.mesh.NEdgesSize,), self.K)
        _chk(lib().omg_vremap_remap_velocity(self.h, h, p, _sh(stream)))
        if keep:
            device_synchronize()
        return _read_back(buf, self.K, stream)

    def adopt_target(self, layer_thickness, stream=None):
        p, buf = _stage_levels(layer_thickness, (self.mesh.NCellsSize,), self.K)
        _chk(lib().omg_vremap_adopt_target(self.h, p, _sh(stream)))
        return _read_back(buf, self.K, stream)

    def remap(self, layer_thickness, normal_velocity, tracers, ntracers: int, stream=None):
        """compute_target, remap_tracers, remap_velocity, adopt_target in three launches; numpy arguments come back as
        (layer_thickness, normal_velocity, tracers), None in the place of a device address"""
        n, nt = self.mesh.NCellsSize, max(int(ntracers), 0)
        ph, bh = _stage_levels(layer_thickness, (n,), self.K)
        pu, bu = _stage_levels(normal_velocity, (self.mesh.NEdgesSize,), self.K)
        pt, bt = (None, None) if tracers is None else _stage_levels(tracers, (nt, n), self.K)
        _chk(lib().omg_vremap_remap(self.h, ph, pu, pt, ntracers, _sh(stream)))
        return tuple(_read_back(b, self.K, stream) for b in (bh, bu, bt))

    def launch_count(self) -> int:
        """kernel launches the five calls have issued on this object so far"""
        return _out(C.c_int64, lib().omg_vremap_launch_count, self.h)

    def _shape(self, name):
        return (self.mesh.NCellsSize, self.K)


def fused_limit(ncells_size: int, nedges_size: int, nvertices_size: int, max_edges: int, nvertlayers: int):
    """omg_tend_fused_limit: (True, "") if the fused RHS covers arrays of these row counts (sentinel row included), else
    (False, reason).  Sizes only: needs neither a mesh nor a device."""
    ok, why = C.c_int(), C.create_string_buffer(1024)
    _chk(lib().omg_tend_fused_limit(ncells_size, nedges_size, nvertices_size, max_edges, nvertlayers, C.byref(ok), why,
                                    len(why)))
    return bool(ok.value), why.value.decode()


class Tendencies(_Handle):
    _destroy = "omg_tend_destroy"

    def __init__(self, mesh: HorzMesh, nvertlayers: int, ntracers: int, config: TendConfig | None = None,
                 allow_reference_structured: bool = False):
        """Raises for a mesh outside the fused RHS (fused_limit) unless allow_reference_structured: then
        compute_all_tendencies takes the reference-structured 23-launch path."""
        self.mesh, self.K, self.NT = mesh, nvertlayers, ntracers
        self.config = config if config is not None else default_config()
        self._create("omg_tend_create_reference_structured" if allow_reference_structured else "omg_tend_create",
                     mesh.h, nvertlayers, ntracers, C.byref(self.config))

    def set_fused(self, on: bool):
        _chk(lib().omg_tend_set_fused(self.h, on))

    def attach_pressure_grad(self, pgrad: "PressureGrad | None"):
        """Tendencies::attachPressureGrad: the layered pressure gradient as an opt-in velocity term (None detaches);
        raises while SSHTendencyEnable is on."""
        _chk(lib().omg_tend_attach_pressure_grad(self.h, _sh(pgrad)))
        self._pgrad = pgrad  # the library keeps a pointer to it

    def attach_vert_adv(self, vert_adv: "VertAdv | None"):
        """Tendencies::attachVertAdv: vertical transport and advection as opt-in terms of all three tendencies (None
        detaches)."""
        _chk(lib().omg_tend_attach_vert_adv(self.h, _sh(vert_adv)))
        self._vert_adv = vert_adv  # the library keeps a pointer to it

    def set_graphs(self, on: bool):
        _chk(lib().omg_tend_set_graphs(self.h, on))

    def graph_stats(self):
        c, r = C.c_int64(), C.c_int64()
        _chk(lib().omg_tend_graph_stats(self.h, C.byref(c), C.byref(r)))
        return {"captures": c.value, "replays": r.value}

    def compute_all_tendencies(self, state, aux, tracers, tracer_tl=0, thick_tl=0, vel_tl=0, stream=None):
        _chk(lib().omg_tend_compute_all(self.h, state.h, aux.h, tracers.h, tracer_tl, thick_tl, vel_tl, _sh(stream)))

    def compute_thickness_tendencies(self, state, aux, thick_tl=0, vel_tl=0, stream=None):
        _chk(lib().omg_tend_compute_thickness(self.h, state.h, aux.h, thick_tl, vel_tl, _sh(stream)))

    def compute_velocity_tendencies(self, state, aux, thick_tl=0, vel_tl=0, stream=None):
        _chk(lib().omg_tend_compute_velocity(self.h, state.h, aux.h, thick_tl, vel_tl, _sh(stream)))

    def compute_tracer_tendencies(self, state, aux, tracers, tracer_tl=0, thick_tl=0, vel_tl=0, stream=None):
        _chk(lib().omg_tend_compute_tracer(self.h, state.h, aux.h, tracers.h, tracer_tl, thick_tl, vel_tl, _sh(stream)))

    def compute_transport_tendencies(self, state, aux, tracers, tracer_tl=0, thick_tl=0, vel_tl=0, stream=None):
        """Tendencies::computeTransportTendencies: LayerThicknessTend and TracerTend as compute_thickness_tendencies
        followed by compute_tracer_tendencies leave them, bit for bit, in two launches; the edge-located auxiliary
        arrays are not written."""
        _chk(lib().omg_tend_compute_transport(self.h, state.h, aux.h, tracers.h, tracer_tl, thick_tl, vel_tl, _sh(stream)))

    def compute_transport_tendencies_and_update(self, state, aux, tracers, tracer_tl=0, thick_tl=0, vel_tl=0,
                                                next_thick_tl=1, next_tracer_tl=1, coeff=0.0, keep_tendencies=True,
                                                stream=None):
        """Tendencies::computeTransportTendenciesAndUpdate: compute_transport_tendencies with the thickness and tracer
        updates folded into its kernels.  The thickness of next_thick_tl and the tracers of next_tracer_tl hold, bit for
        bit on rows < NCellsAll and levels < K, what the transport call followed by update_by_tend and
        update_tracers_by_tend leave there; with keep_tendencies the tendency arrays are the transport call's, without
        it their contents are unspecified."""
        _chk(lib().omg_tend_compute_transport_update(self.h, state.h, aux.h, tracers.h, tracer_tl, thick_tl, vel_tl,
                                                     next_thick_tl, next_tracer_tl, coeff, bool(keep_tendencies), _sh(stream)))

    def compute_momentum_tendencies(self, state, aux, tracers, tracer_tl=0, thick_tl=0, vel_tl=0, stream=None):
        """Tendencies::computeMomentumTendencies: NormalVelocityTend and LayerThicknessTend as compute_all_tendencies
        leaves them, bit for bit, attached terms included, from the fused RHS without its tracer half; TracerTend and
        Del2TracersCell are not written (with a custom tendency installed compute_all_tendencies itself runs)."""
        _chk(lib().omg_tend_compute_momentum(self.h, state.h, aux.h, tracers.h, tracer_tl, thick_tl, vel_tl, _sh(stream)))

    def compute_thickness_tendencies_only(self, state, aux, thick_tl=0, vel_tl=0, stream=None):
        _chk(lib().omg_tend_compute_thickness_only(self.h, state.h, aux.h, thick_tl, vel_tl, _sh(stream)))

    def compute_velocity_tendencies_only(self, state, aux, thick_tl=0, vel_tl=0, stream=None):
        _chk(lib().omg_tend_compute_velocity_only(self.h, state.h, aux.h, thick_tl, vel_tl, _sh(stream)))

    def compute_tracer_tendencies_only(self, state, aux, tracers, tracer_tl=0, thick_tl=0, vel_tl=0, stream=None):
        _chk(lib().omg_tend_compute_tracer_only(self.h, state.h, aux.h, tracers.h, tracer_tl, thick_tl, vel_tl,
                                                _sh(stream)))

    def use_manufactured_solution(self, mesh, wavelength_x: float, wavelength_y: float, amplitude: float):
        """Tendencies config UseCustomTendency + ManufacturedSolutionTendency (CustomTendencyTerms.cpp)."""
        _chk(lib().omg_tend_use_manufactured_solution(self.h, mesh.h, wavelength_x, wavelength_y, amplitude))

    def set_custom_tendency(self, which: int, fn):
        """Tendencies::CustomThicknessTend (which 0) / CustomVelocityTend (which 1) as a Python callable
        fn(tend_ptr, h_ptr, u_ptr, n_rows_all, n_rows_size, K, row_pitch, time_seconds, stream_handle); None clears it."""
        if not hasattr(self, "_custom"):
            self._custom = {}
        if fn is None:
            _chk(lib().omg_tend_set_custom_tendency(self.h, which, None, None))
            self._custom.pop(which, None)
            return

        def _cb(_ctx, tend, h, u, nall, nsize, k, pitch, t, stream):
            try:
                fn(tend, h, u, nall, nsize, k, pitch, t, stream)
                return 0
            except Exception:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1
        self._custom[which] = CUSTOM_TEND_FN(_cb)
        _chk(lib().omg_tend_set_custom_tendency(self.h, which, self._custom[which], None))

    def clear_custom_tendencies(self):
        _chk(lib().omg_tend_clear_custom_tendencies(self.h))

    def set_time(self, seconds: float):
        """model time (s since the reference time) the custom tendencies see in direct compute_* calls"""
        _chk(lib().omg_tend_set_time(self.h, seconds))

    def kernel_timing(self, on: bool):
        _chk(lib().omg_tend_kernel_timing(self.h, on))

    def collect_kernel_times(self):
        """[(kernel name, mean ms)] over the RHS evaluations recorded since kernel_timing(True)."""
        ms = (C.c_double * 16)()
        nk, ns = C.c_int(), C.c_int()
        _chk(lib().omg_tend_collect_kernel_times(self.h, ms, C.byref(nk), C.byref(ns)))
        if ns.value == 0:
            return []
        out = [(lib().omg_tend_kernel_name(i).decode(), ms[i] / ns.value) for i in range(nk.value)]
        return [(k, v) for k, v in out if k]

    def device_ptr(self, which: int):
        """omg_tend_device_ptr: (device address, number of values incl. the row padding) of LayerThicknessTend (0),
        NormalVelocityTend (1), TracerTend (2)"""
        p, n = C.c_void_p(), C.c_size_t()
        _chk(lib().omg_tend_device_ptr(self.h, which, C.byref(p), C.byref(n)))
        return p.value, n.value

    def get(self, which: int) -> np.ndarray:
        m = self.mesh
        shape = [(m.NCellsSize, self.K), (m.NEdgesSize, self.K), (max(self.NT, 1), m.NCellsSize, self.K)][which]
        out = np.zeros(shape)
        _chk(lib().omg_tend_copy_to_host(self.h, which, _pd(out), out.size))
        return out


class TimeStepper(_Handle):
    _destroy = "omg_stepper_destroy"

    def __init__(self, kind: str, dt: float, tend: Tendencies, aux: AuxiliaryState, mesh: HorzMesh,
                 halo: Halo | None, tracers: Tracers):
        self.refs = (tend, aux, mesh, halo, tracers)
        self._create("omg_stepper_create", kind.encode(), dt, tend.h, aux.h, mesh.h, halo.h if halo else None, tracers.h)

    def attach_vert_mix(self, vert_mix_step: "VertMixStep | None"):
        """TimeStepper::attachVertMix: every do_step runs the mixing sequence on the new time level before the time
        levels rotate (None detaches); raises for another mesh, layer or tracer count and for a halo with neighbours."""
        _chk(lib().omg_stepper_attach_vert_mix(self.h, _sh(vert_mix_step)))
        self._vert_mix_step = vert_mix_step  # the library keeps a pointer to it

    def attach_barotropic(self, btr: "BarotropicMode", nsub: int):
        """SplitExplicitStepper::attachBarotropic: required before the first do_step of a "Split-Explicit" stepper;
        raises on any other kind, for another mesh or layer count, nsub < 1 and a halo with neighbours."""
        _chk(lib().omg_stepper_attach_barotropic(self.h, _sh(btr), nsub))
        self._barotropic = btr  # the library keeps a pointer to it

    def attach_monotone_adv(self, mono: "MonotoneAdv | None"):
        """SplitExplicitStepper::attachMonotoneAdv: the step's horizontal tracer advection through `mono` (None
        detaches); raises on any other kind, for another mesh or layer count, too few tracers, a flux-thickness option
        that differs from the AuxiliaryState's, and while the Tendencies' own TracerHorzAdvTendencyEnable is on."""
        _chk(lib().omg_stepper_attach_monotone_adv(self.h, _sh(mono)))
        self._monotone_adv = mono  # the library keeps a pointer to it

    def attach_gent_mcwilliams(self, gm: "GentMcWilliams | None"):
        """SplitExplicitStepper::attachGentMcWilliams: every step adds the bolus velocity of the current level's
        stratification to its transporting velocity (None detaches); raises on any other kind, for another mesh or layer
        count, fewer than 2 tracers, and, with a PressureGrad attached to the Tendencies, for a `gm` on another VertCoord
        or Eos than its (the caller keeps the forcing arrays of the two equal)."""
        _chk(lib().omg_stepper_attach_gm(self.h, _sh(gm)))
        self._gent_mcwilliams = gm  # the library keeps a pointer to it

    def attach_redi(self, redi: "Redi | None"):
        """SplitExplicitStepper::attachRedi: every step computes the isopycnal slopes of the current level and adds the
        isoneutral cross terms to the tracer tendency before the tracer update (None detaches); raises on any other
        kind, for another mesh or layer count, too few tracers, another VertCoord or Eos than an attached
        GentMcWilliams's or PressureGrad's, and unless a VertMixStep with this same `redi` attached is attached."""
        _chk(lib().omg_stepper_attach_redi(self.h, _sh(redi)))
        self._redi = redi  # the library keeps a pointer to it

    def attach_vert_remap(self, vert_remap: "VertRemap | None"):
        """SplitExplicitStepper::attachVertRemap: every step remaps the new time level back onto the VertCoord's target
        grid (VertRemap.remap) between the velocity update and the vertical mixing (None detaches); raises on any other
        kind, for another mesh or layer count, too few tracers, and while a VertAdv is attached to the Tendencies."""
        _chk(lib().omg_stepper_attach_vert_remap(self.h, _sh(vert_remap)))
        self._vert_remap = vert_remap  # the library keeps a pointer to it

    def set_fused_transport(self, on: bool):
        """SplitExplicitStepper::UseFusedTransport (default on): the step's thickness and tracer tendencies through
        Tendencies.compute_transport_tendencies instead of the two group calls; raises on any other kind."""
        _chk(lib().omg_stepper_set_fused_transport(self.h, on))

    def set_momentum_rhs(self, on: bool):
        """SplitExplicitStepper::UseMomentumRHS: the step's first evaluation through
        Tendencies.compute_momentum_tendencies instead of compute_all_tendencies; raises on any other kind."""
        _chk(lib().omg_stepper_set_momentum_rhs(self.h, on))

    def set_folded_updates(self, on: bool):
        """SplitExplicitStepper::FoldUpdates: with the fused transport on, the transport tendencies and the thickness
        and tracer updates through Tendencies.compute_transport_tendencies_and_update (not with tracers and their
        hyperdiffusion term off: no faster there); raises on any other kind."""
        _chk(lib().omg_stepper_set_folded_updates(self.h, on))

    def do_step(self, state: OceanState, stream=None):
        _chk(lib().omg_stepper_do_step(self.h, state.h, _sh(stream)))

    def set_start_time(self, seconds: float):
        _chk(lib().omg_stepper_set_start_time(self.h, seconds))

    @property
    def time(self) -> float:
        return _out(C.c_double, lib().omg_stepper_get_time, self.h)

    def graph_stats(self):
        c, r = C.c_int64(), C.c_int64()
        _chk(lib().omg_stepper_graph_stats(self.h, C.byref(c), C.byref(r)))
        return {"captures": c.value, "replays": r.value}

    def change_time_step(self, dt: float):
        _chk(lib().omg_stepper_change_time_step(self.h, dt))

    def set_option(self, name: str, value: bool):
        """RungeKutta4: "FuseStageUpdates" (default on), "StoreStageTendencies" (default off)."""
        _chk(lib().omg_stepper_set_option(self.h, name.encode(), value))


def update_by_tend(out_ptr: int, in_ptr: int, tend_ptr: int, coeff: float, n_rows: int, k: int, stream_handle=None):
    """out = in + coeff * tend on raw [n_rows][k] device arrays (TimeStepper::update*ByTend's kernel)."""
    _chk(lib().omg_update_by_tend(out_ptr, in_ptr, tend_ptr, coeff, n_rows, k, stream_handle or None))


def update_tracers_by_tend(next_ptr: int, cur_ptr: int, h_next_ptr: int, h_cur_ptr: int, tend_ptr: int, coeff: float,
                           n_tracers: int, n_rows: int, rows_size: int, k: int, stream_handle=None):
    """next = (cur*h_cur + coeff*tend)/h_next on raw device arrays of row length k, tracer planes rows_size rows apart
    (TimeStepper::updateTracersByTend's kernel)."""
    _chk(lib().omg_update_tracers_by_tend(next_ptr, cur_ptr, h_next_ptr, h_cur_ptr, tend_ptr, coeff, n_tracers, n_rows,
                                          rows_size, k, stream_handle or None))


def coeff_seconds(mult: float, dt: float) -> float:
    return _out(C.c_double, lib().omg_stepper_coeff_seconds, mult, dt)
