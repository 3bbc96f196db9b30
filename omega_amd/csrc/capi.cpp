// capi.cpp -- extern "C" boundary of libomega_amd.so (see include/omega_amd.h).
#include "../../include/omega_amd.h"

#include "AuxiliaryState.h"
#include "Decomp.h"
#include "Halo.h"
#include "HorzMesh.h"
#include "HorzOperators.h"
#include "OceanState.h"
#include "Tendencies.h"
#include "CustomTendencyTerms.h"
#include "MeshIO.h"
#include "Partition.h"
#include "History.h"
#include "Pacer.h"
#include "PeerWire.h"
#include "Rccl.h"
#include "Tuning.h"
#include "TimeStepper.h"
#include "VertCoord.h"
#include "Eos.h"
#include "TriDiagSolvers.h"
#include "VertMix.h"
#include "GentMcWilliams.h"
#include "Redi.h"
#include "PressureGrad.h"
#include "MonotoneAdv.h"
#include "VertAdv.h"
#include "VertRemap.h"
#include "Kpp.h"
#include "VertMixStep.h"
#include "BarotropicMode.h"
#include "SplitExplicitStepper.h"

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>

using namespace OMEGA;

struct omg_decomp {
   std::unique_ptr<Decomp> D;
};
struct omg_halo {
   std::unique_ptr<Halo> H;
};
struct omg_rccl {
   std::unique_ptr<RcclComm> C;
};
struct omg_peer {
   std::unique_ptr<PeerWire> P;
};
struct omg_mesh {
   std::unique_ptr<HorzMesh> M;
};
struct omg_state {
   std::unique_ptr<OceanState> S;
};
struct omg_tracers {
   std::unique_ptr<TracerStore> T;
};
struct omg_aux {
   std::unique_ptr<AuxiliaryState> A;
};
struct omg_mesh_file {
   std::unique_ptr<MeshFile> F;
};
struct omg_tend {
   std::unique_ptr<Tendencies> T;
   std::shared_ptr<ManufacturedSolution> Ms;
};
struct omg_stepper {
   std::unique_ptr<TimeStepper> St;
};
struct omg_vcoord {
   std::unique_ptr<VertCoord> V;
};
struct omg_eos {
   std::unique_ptr<Eos> E;
};
struct omg_vertmix {
   std::unique_ptr<VertMix> X;
};
struct omg_vertmix_step {
   std::unique_ptr<VertMixStep> M;
};
struct omg_pgrad {
   std::unique_ptr<PressureGrad> P;
};
struct omg_vertadv {
   std::unique_ptr<VertAdv> A;
};
struct omg_btr {
   std::unique_ptr<BarotropicMode> B;
};
struct omg_monoadv {
   std::unique_ptr<MonotoneAdv> A;
};
struct omg_gm {
   std::unique_ptr<GentMcWilliams> G;
};
struct omg_redi {
   std::unique_ptr<Redi> R;
};
struct omg_vremap {
   std::unique_ptr<VertRemap> R;
};
struct omg_kpp {
   std::unique_ptr<Kpp> K;
};

static thread_local std::string LastError;

#define OMG_TRY try {
#define OMG_CATCH                                                              \
   }                                                                           \
   catch (const std::exception &E) {                                           \
      LastError = E.what();                                                    \
      return 1;                                                                \
   }                                                                           \
   catch (...) {                                                               \
      LastError = "unknown exception";                                         \
      return 1;                                                                \
   }                                                                           \
   return 0;

#define OMG_ARG(cond)                                                          \
   if (!(cond))                                                                \
   OMEGA_ABORT(std::string("invalid argument: ") + #cond)

/// a device array as (pointer, rows of the last index, width, row pitch) -- see copyRowsToHost
struct ArrRef {
   Real *Ptr;
   size_t Rows;
   int Width, Pitch;
   size_t size() const { return Rows * (size_t)Width; }
};
template <int N> static ArrRef arrRef(const DeviceArray<Real, N> &A) {
   return ArrRef{A.Ptr, A.rows(), A.Ext[N - 1], A.Pitch};
}
/// the three things the boundary does with an ArrRef: a compact host copy of at most n values out, one of exactly
/// n values in, the device address (and the number of values, if asked for) out
static void refCopyToHost(const ArrRef &R, const char *Name, double *Host, size_t N) {
   if (N < R.size())
      OMEGA_ABORT(std::string("output buffer too small for ") + Name);
   copyRowsToHost(Host, R.Ptr, R.Pitch, R.Rows, R.Width);
}
static void refCopyToDevice(const ArrRef &R, const char *Name, const double *Host, size_t N) {
   if (N != R.size())
      OMEGA_ABORT(std::string("size mismatch for ") + Name);
   copyRowsToDevice(R.Ptr, R.Pitch, Host, R.Rows, R.Width);
}
static void refPointerOut(const ArrRef &R, double **Dev, size_t *N) {
   *Dev = R.Ptr;
   if (N)
      *N = R.size();
}

/// A new handle: `Fill` constructs the payload into the handle struct, which reaches *Out only if that did not throw
/// (a throwing constructor leaks nothing and leaves *Out as it was).
template <class Handle, class FillFn> static void newHandle(Handle **Out, FillFn &&Fill) {
   auto R = std::make_unique<Handle>();
   Fill(*R);
   *Out = R.release();
}

/// Name-to-member tables: a flat list of {name, value} and the one finder; `What` is the start of the message an
/// unknown name aborts with ("Eos: no array named ").
template <class T> struct Named {
   const char *Name;
   T Value;
};
template <class T> static T findNamed(std::initializer_list<Named<T>> Table, const char *Name, const char *What) {
   for (const Named<T> &E : Table)
      if (std::strcmp(E.Name, Name) == 0)
         return E.Value;
   OMEGA_ABORT(std::string(What) + Name);
}

/// The accessors of a class with named Real arrays, from its handle type, the handle parameter's name (it appears in
/// the invalid-argument message) and its lookup, an expression in that parameter and `name` that gives the ArrRef.
#define OMG_NAMED_ARRAYS(TO_HOST, TO_DEVICE, DEVICE_PTR, HANDLE, H, LOOKUP)                                          \
   int TO_HOST(const HANDLE *H, const char *name, double *host, size_t n) {                                          \
      OMG_TRY                                                                                                        \
      OMG_ARG(H && name && host);                                                                                    \
      refCopyToHost(LOOKUP, name, host, n);                                                                          \
      OMG_CATCH                                                                                                      \
   }                                                                                                                 \
   int TO_DEVICE(HANDLE *H, const char *name, const double *host, size_t n) {                                        \
      OMG_TRY                                                                                                        \
      OMG_ARG(H && name && host);                                                                                    \
      refCopyToDevice(LOOKUP, name, host, n);                                                                        \
      OMG_CATCH                                                                                                      \
   }                                                                                                                 \
   int DEVICE_PTR(const HANDLE *H, const char *name, double **dev, size_t *n) {                                      \
      OMG_TRY                                                                                                        \
      OMG_ARG(H && name && dev);                                                                                     \
      refPointerOut(LOOKUP, dev, n);                                                                                 \
      OMG_CATCH                                                                                                      \
   }

extern "C" {

const char *omg_last_error(void) { return LastError.c_str(); }

int omg_device_count(int *n) {
   OMG_TRY
   OMG_ARG(n);
   int C = 0;
   if (hipGetDeviceCount(&C) != hipSuccess)
      C = 0;
   *n = C;
   OMG_CATCH
}
int omg_device_init(int device_id) {
   OMG_TRY
   deviceInit(device_id);
   OMG_CATCH
}
int omg_device_synchronize(void) {
   OMG_TRY
   HIP_CHECK(hipDeviceSynchronize());
   OMG_CATCH
}
int omg_stream_create(void **stream) {
   OMG_TRY
   OMG_ARG(stream);
   hipStream_t S;
   HIP_CHECK(hipStreamCreateWithFlags(&S, hipStreamNonBlocking));
   *stream = (void *)S;
   OMG_CATCH
}
int omg_stream_destroy(void *stream) {
   OMG_TRY
   if (stream)
      HIP_CHECK(hipStreamDestroy((hipStream_t)stream));
   OMG_CATCH
}
int omg_stream_synchronize(void *stream) {
   OMG_TRY
   HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
   OMG_CATCH
}
int omg_event_create(void **event) {
   OMG_TRY
   OMG_ARG(event);
   hipEvent_t E;
   HIP_CHECK(hipEventCreate(&E));
   *event = (void *)E;
   OMG_CATCH
}
int omg_event_destroy(void *event) {
   OMG_TRY
   if (event)
      HIP_CHECK(hipEventDestroy((hipEvent_t)event));
   OMG_CATCH
}
int omg_event_record(void *event, void *stream) {
   OMG_TRY
   HIP_CHECK(hipEventRecord((hipEvent_t)event, (hipStream_t)stream));
   OMG_CATCH
}
int omg_event_elapsed_ms(void *start, void *stop, float *ms) {
   OMG_TRY
   OMG_ARG(ms);
   HIP_CHECK(hipEventSynchronize((hipEvent_t)stop));
   HIP_CHECK(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
   OMG_CATCH
}

// ---------------------------------------------------------------- raw device buffers
int omg_device_resource_count(int64_t *n) {
   OMG_TRY
   OMG_ARG(n);
   *n = deviceResourceCount();
   OMG_CATCH
}
int omg_device_malloc(size_t bytes, void **ptr) {
   OMG_TRY
   OMG_ARG(ptr);
   HIP_CHECK(hipMalloc(ptr, bytes ? bytes : 1));
   OMG_CATCH
}
int omg_device_free(void *ptr) {
   OMG_TRY
   if (ptr)
      HIP_CHECK(hipFree(ptr));
   OMG_CATCH
}
int omg_copy_to_device(void *dst, const void *src, size_t bytes) {
   OMG_TRY
   OMG_ARG(dst && src);
   HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
   OMG_CATCH
}
int omg_copy_to_host(void *dst, const void *src, size_t bytes) {
   OMG_TRY
   OMG_ARG(dst && src);
   HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
   OMG_CATCH
}

// ---------------------------------------------------------------- reductions
int omg_local_sum_dd(const double *a, const double *b, size_t n, void *stream, double *hi_lo) {
   OMG_TRY
   OMG_ARG(a && hi_lo);
   localSumDD(a, b, n, (hipStream_t)stream, hi_lo);
   OMG_CATCH
}
int omg_local_weighted_sum_dd(const double *w, const double *a, const double *b, int nrows, int k, int row_pitch,
                              void *stream, double *hi_lo) {
   OMG_TRY
   OMG_ARG(w && a && hi_lo && nrows >= 0 && k > 0 && (row_pitch == 0 || row_pitch >= k));
   localWeightedSumDD(w, a, b, nrows, k, row_pitch > 0 ? row_pitch : k, (hipStream_t)stream, hi_lo);
   OMG_CATCH
}
int omg_combine_dd(const double *pairs, int npairs, double *hi_lo) {
   OMG_TRY
   OMG_ARG(pairs && hi_lo && npairs >= 0);
   combineDD(pairs, npairs, hi_lo);
   OMG_CATCH
}

// ---------------------------------------------------------------- mesh file
int omg_mesh_file_open(const char *path, omg_mesh_file **out) {
   OMG_TRY
   OMG_ARG(path && out);
   newHandle(out, [&](omg_mesh_file &R) { R.F.reset(new MeshFile(path)); });
   OMG_CATCH
}
int omg_mesh_file_close(omg_mesh_file *f) {
   delete f;
   return 0;
}
int omg_mesh_file_global_mesh(const omg_mesh_file *f, omg_global_mesh *m) {
   OMG_TRY
   OMG_ARG(f && m);
   const GlobalMeshDesc &G = f->F->desc();
   m->nCells = G.NCells, m->nEdges = G.NEdges, m->nVertices = G.NVertices, m->maxEdges = G.MaxEdges;
   m->vertexDegree = G.VertexDegree;
   m->cellsOnCell = G.CellsOnCell, m->edgesOnCell = G.EdgesOnCell, m->verticesOnCell = G.VerticesOnCell;
   m->cellsOnEdge = G.CellsOnEdge, m->verticesOnEdge = G.VerticesOnEdge, m->edgesOnEdge = G.EdgesOnEdge;
   m->cellsOnVertex = G.CellsOnVertex, m->edgesOnVertex = G.EdgesOnVertex;
   m->xCell = G.XCell, m->yCell = G.YCell, m->zCell = G.ZCell, m->lonCell = G.LonCell, m->latCell = G.LatCell;
   m->xEdge = G.XEdge, m->yEdge = G.YEdge, m->zEdge = G.ZEdge, m->lonEdge = G.LonEdge, m->latEdge = G.LatEdge;
   m->xVertex = G.XVertex, m->yVertex = G.YVertex, m->zVertex = G.ZVertex, m->lonVertex = G.LonVertex;
   m->latVertex = G.LatVertex;
   m->areaCell = G.AreaCell, m->areaTriangle = G.AreaTriangle, m->kiteAreasOnVertex = G.KiteAreasOnVertex;
   m->dcEdge = G.DcEdge, m->dvEdge = G.DvEdge, m->angleEdge = G.AngleEdge, m->weightsOnEdge = G.WeightsOnEdge;
   m->fCell = G.FCell, m->fEdge = G.FEdge, m->fVertex = G.FVertex, m->bottomDepth = G.BottomDepth;
   OMG_CATCH
}
int omg_mesh_file_dim(const omg_mesh_file *f, const char *name, int64_t *len) {
   OMG_TRY
   OMG_ARG(f && name && len);
   *len = f->F->file().hasDim(name) ? f->F->file().dimLen(name) : -1;
   OMG_CATCH
}
int omg_mesh_file_var_size(const omg_mesh_file *f, const char *name, int64_t record, int64_t *n) {
   OMG_TRY
   OMG_ARG(f && name && n);
   if (!f->F->file().hasVar(name)) {
      *n = -1;
   } else {
      const std::vector<I8> S = f->F->file().shape(name);
      const bool Rec          = f->F->file().var(name).IsRecord;
      I8 N                    = 1;
      for (size_t D = (Rec && record >= 0) ? 1 : 0; D < S.size(); ++D)
         N *= S[D];
      *n = N;
   }
   OMG_CATCH
}
int omg_mesh_file_read_f64(const omg_mesh_file *f, const char *name, int64_t record, double *out, size_t n) {
   OMG_TRY
   OMG_ARG(f && name && out);
   std::vector<R8> V;
   f->F->file().read(name, V, record);
   if (V.size() != n)
      OMEGA_ABORT(std::string("omg_mesh_file_read_f64: ") + name + " has " + std::to_string(V.size()) +
                  " values, buffer holds " + std::to_string(n));
   std::memcpy(out, V.data(), n * sizeof(double));
   OMG_CATCH
}

// ---------------------------------------------------------------- restart file
struct omg_restart_file {
   std::unique_ptr<RestartFile> F;
};
int omg_restart_create(const char *path, int64_t ncells_global, int64_t nedges_global, int nvertlevels, int ntracers,
                       double simulation_time, int64_t steps_done) {
   OMG_TRY
   OMG_ARG(path);
   RestartFile::create(path, ncells_global, nedges_global, nvertlevels, ntracers, simulation_time, steps_done);
   OMG_CATCH
}
int omg_restart_open(const char *path, int write, omg_restart_file **out) {
   OMG_TRY
   OMG_ARG(path && out);
   newHandle(out, [&](omg_restart_file &R) { R.F.reset(new RestartFile(path, write != 0)); });
   OMG_CATCH
}
int omg_restart_close(omg_restart_file *f) {
   delete f;
   return 0;
}
int omg_restart_info(const omg_restart_file *f, int64_t *ncells, int64_t *nedges, int *nvertlevels, int *ntracers,
                     double *simulation_time, int64_t *steps_done) {
   OMG_TRY
   OMG_ARG(f && ncells && nedges && nvertlevels && ntracers && simulation_time && steps_done);
   *ncells = f->F->NCells, *nedges = f->F->NEdges, *nvertlevels = f->F->NVertLevels, *ntracers = f->F->NTracers;
   *simulation_time = f->F->SimulationTime, *steps_done = f->F->StepsDone;
   OMG_CATCH
}
int omg_restart_write_rows(omg_restart_file *f, const char *var, int plane, const int32_t *global_id, int64_t n,
                           const double *rows) {
   OMG_TRY
   OMG_ARG(f && var && global_id && rows);
   f->F->writeRows(var, plane, global_id, n, rows);
   OMG_CATCH
}
int omg_restart_read_rows(const omg_restart_file *f, const char *var, int plane, const int32_t *global_id, int64_t n,
                          double *rows) {
   OMG_TRY
   OMG_ARG(f && var && global_id && rows);
   f->F->readRows(var, plane, global_id, n, rows);
   OMG_CATCH
}

// ---------------------------------------------------------------- Decomp
static GlobalMeshDesc toDesc(const omg_global_mesh &M) {
   const omg_global_mesh *m = &M;
   GlobalMeshDesc G;
   G.NCells = m->nCells, G.NEdges = m->nEdges, G.NVertices = m->nVertices, G.MaxEdges = m->maxEdges;
   G.VertexDegree = m->vertexDegree;
   G.CellsOnCell = m->cellsOnCell, G.EdgesOnCell = m->edgesOnCell, G.VerticesOnCell = m->verticesOnCell;
   G.CellsOnEdge = m->cellsOnEdge, G.VerticesOnEdge = m->verticesOnEdge, G.EdgesOnEdge = m->edgesOnEdge;
   G.CellsOnVertex = m->cellsOnVertex, G.EdgesOnVertex = m->edgesOnVertex;
   G.XCell = m->xCell, G.YCell = m->yCell, G.ZCell = m->zCell, G.LonCell = m->lonCell, G.LatCell = m->latCell;
   G.XEdge = m->xEdge, G.YEdge = m->yEdge, G.ZEdge = m->zEdge, G.LonEdge = m->lonEdge, G.LatEdge = m->latEdge;
   G.XVertex = m->xVertex, G.YVertex = m->yVertex, G.ZVertex = m->zVertex, G.LonVertex = m->lonVertex;
   G.LatVertex = m->latVertex;
   G.AreaCell = m->areaCell, G.AreaTriangle = m->areaTriangle, G.KiteAreasOnVertex = m->kiteAreasOnVertex;
   G.DcEdge = m->dcEdge, G.DvEdge = m->dvEdge, G.AngleEdge = m->angleEdge, G.WeightsOnEdge = m->weightsOnEdge;
   G.FCell = m->fCell, G.FEdge = m->fEdge, G.FVertex = m->fVertex, G.BottomDepth = m->bottomDepth;
   return G;
}
int omg_decomp_create_ordered(const omg_global_mesh *mesh, int nparts, int mytask, int halo_width,
                              const int32_t *cell_task, int local_order, omg_decomp **out);
int omg_decomp_create(const omg_global_mesh *m, int nparts, int mytask, int halo_width, const int32_t *cell_task,
                      omg_decomp **out) {
   return omg_decomp_create_ordered(m, nparts, mytask, halo_width, cell_task, 0, out);
}
int omg_decomp_create_ordered(const omg_global_mesh *mesh, int nparts, int mytask, int halo_width,
                              const int32_t *cell_task, int local_order, omg_decomp **out) {
   OMG_TRY
   OMG_ARG(mesh && out && local_order >= 0 && local_order <= 3);
   newHandle(out, [&](omg_decomp &R) {
      R.D.reset(new Decomp(toDesc(*mesh), nparts, mytask, halo_width, cell_task, (LocalOrder)local_order));
   });
   OMG_CATCH
}
int omg_partition_cells(const omg_global_mesh *mesh, int nparts, const char *method, int32_t *cell_task_out,
                        int64_t *edge_cut) {
   OMG_TRY
   OMG_ARG(mesh && method && cell_task_out && nparts >= 1);
   const GlobalMeshDesc G = toDesc(*mesh);
   std::vector<I4> T;
   const std::string M(method);
   if (M == "graph") {
      partitionGraph(G, nparts, T);
   } else if (M == "rcb") {
      partitionRCB(G, nparts, T);
   } else {
      OMEGA_ABORT("omg_partition_cells: method must be \"rcb\" or \"graph\"");
   }
   std::memcpy(cell_task_out, T.data(), T.size() * sizeof(I4));
   if (edge_cut)
      *edge_cut = edgeCut(G, T);
   OMG_CATCH
}
int omg_decomp_destroy(omg_decomp *d) {
   delete d;
   return 0;
}
int omg_decomp_get_int(const omg_decomp *d, const char *name, int32_t *out) {
   OMG_TRY
   OMG_ARG(d && name && out);
   const Decomp &D = *d->D;
   *out = findNamed<I4>({{"NCellsGlobal", D.NCellsGlobal},
                         {"NCellsOwned", D.NCellsOwned},
                         {"NCellsAll", D.NCellsAll},
                         {"NCellsSize", D.NCellsSize},
                         {"NEdgesGlobal", D.NEdgesGlobal},
                         {"NEdgesOwned", D.NEdgesOwned},
                         {"NEdgesAll", D.NEdgesAll},
                         {"NEdgesSize", D.NEdgesSize},
                         {"NVerticesGlobal", D.NVerticesGlobal},
                         {"NVerticesOwned", D.NVerticesOwned},
                         {"NVerticesAll", D.NVerticesAll},
                         {"NVerticesSize", D.NVerticesSize},
                         {"MaxEdges", D.MaxEdges},
                         {"VertexDegree", D.VertexDegree},
                         {"HaloWidth", D.HaloWidth},
                         {"NumTasks", D.NumTasks},
                         {"MyTask", D.MyTask}},
                        name, "Decomp: no integer member named ");
   OMG_CATCH
}
static void copyOutI4(const I4 *Src, size_t Cnt, int32_t *Out, size_t N, const char *Name) {
   if (N < Cnt)
      OMEGA_ABORT(std::string("output buffer too small for ") + Name);
   std::memcpy(Out, Src, Cnt * sizeof(I4));
}
int omg_decomp_get_array(const omg_decomp *d, const char *name, int32_t *out, size_t n) {
   OMG_TRY
   OMG_ARG(d && name && out);
   const Decomp &D = *d->D;
   if (std::strcmp(name, "CellTask") == 0) { // a std::vector, not a host array
      copyOutI4(D.CellTask.data(), D.CellTask.size(), out, n, name);
      return 0;
   }
   const HostArrayI4 *A = findNamed<const HostArrayI4 *>(
       {{"CellID", &D.CellIDH},         {"EdgeID", &D.EdgeIDH},         {"VertexID", &D.VertexIDH},
        {"CellLoc", &D.CellLocH},       {"EdgeLoc", &D.EdgeLocH},       {"VertexLoc", &D.VertexLocH},
        {"NCellsHalo", &D.NCellsHaloH}, {"NEdgesHalo", &D.NEdgesHaloH}, {"NVerticesHalo", &D.NVerticesHaloH}},
       name, "Decomp: no array member named ");
   copyOutI4(A->data(), A->size(), out, n, name);
   OMG_CATCH
}

// ---------------------------------------------------------------- Halo
int omg_halo_create(const omg_decomp *d, omg_halo **out) {
   OMG_TRY
   OMG_ARG(d && out);
   newHandle(out, [&](omg_halo &R) { R.H.reset(new Halo("Default", d->D.get())); });
   OMG_CATCH
}
int omg_halo_destroy(omg_halo *h) {
   delete h;
   return 0;
}
int omg_halo_num_neighbors(const omg_halo *h, int *n) {
   OMG_TRY
   OMG_ARG(h && n);
   *n = h->H->NNghbr;
   OMG_CATCH
}
int omg_halo_neighbor_task(const omg_halo *h, int i, int *task) {
   OMG_TRY
   OMG_ARG(h && task && i >= 0 && i < h->H->NNghbr);
   *task = h->H->NeighborList[i];
   OMG_CATCH
}
int omg_halo_list_size(const omg_halo *h, int i, int elem, int recv, int *n) {
   OMG_TRY
   OMG_ARG(h && n && i >= 0 && i < h->H->NNghbr && elem >= 0 && elem < 3);
   *n = (int)(recv ? h->H->RecvLists[elem][i] : h->H->SendLists[elem][i]).size();
   OMG_CATCH
}
int omg_halo_get_list(const omg_halo *h, int i, int elem, int recv, int32_t *out) {
   OMG_TRY
   OMG_ARG(h && out && i >= 0 && i < h->H->NNghbr && elem >= 0 && elem < 3);
   const auto &L = recv ? h->H->RecvLists[elem][i] : h->H->SendLists[elem][i];
   std::memcpy(out, L.data(), L.size() * sizeof(I4));
   OMG_CATCH
}
int omg_halo_required_bytes(const omg_halo *h, int i, size_t pc, size_t pe, size_t pv, size_t *bytes) {
   OMG_TRY
   OMG_ARG(h && bytes && i >= 0 && i < h->H->NNghbr);
   *bytes = h->H->requiredBytes(i, pc, pe, pv);
   OMG_CATCH
}
int omg_history_write(const char *path, const omg_decomp *d, const omg_state *s, const omg_tracers *t, omg_aux *a,
                      const char *contents, double simulation_time, int time_level, int create_file, void *stream,
                      int *n_variables_written) {
   OMG_TRY
   OMG_ARG(path && d && s && a && contents);
   const int N = writeHistory(path, d->D.get(), s->S.get(), t ? t->T.get() : nullptr, a->A.get(), contents,
                              simulation_time, time_level, create_file != 0, (hipStream_t)stream);
   if (n_variables_written)
      *n_variables_written = N;
   OMG_CATCH
}
int omg_rccl_get_unique_id(char *id) {
   OMG_TRY
   OMG_ARG(id);
   RcclComm::getUniqueId(id);
   OMG_CATCH
}
int omg_rccl_create(const char *id, int nranks, int rank, omg_rccl **out) {
   OMG_TRY
   OMG_ARG(id && out);
   newHandle(out, [&](omg_rccl &R) { R.C.reset(new RcclComm(id, nranks, rank)); });
   OMG_CATCH
}
int omg_rccl_destroy(omg_rccl *c) {
   delete c;
   return 0;
}
int omg_rccl_abort(omg_rccl *c) {
   OMG_TRY
   OMG_ARG(c);
   c->C->abort();
   OMG_CATCH
}
int omg_rccl_info(const omg_rccl *c, int *nranks, int *rank, int *version, int64_t *exchanges) {
   OMG_TRY
   OMG_ARG(c);
   if (nranks)
      *nranks = c->C->NRanks;
   if (rank)
      *rank = c->C->Rank;
   if (version)
      *version = c->C->Version;
   if (exchanges)
      *exchanges = c->C->NExchanges;
   OMG_CATCH
}
int omg_rccl_exchange(omg_rccl *c, int n, const int *peers, void *const *send_ptrs, const size_t *send_bytes,
                      void *const *recv_ptrs, const size_t *recv_bytes, void *stream) {
   OMG_TRY
   OMG_ARG(c && n >= 0 && (n == 0 || (peers && send_ptrs && send_bytes && recv_ptrs && recv_bytes)));
   if (c->C->exchange(n, peers, send_ptrs, send_bytes, recv_ptrs, recv_bytes, (hipStream_t)stream) != 0)
      OMEGA_ABORT(c->C->lastError());
   OMG_CATCH
}
int omg_halo_use_rccl(omg_halo *h, omg_rccl *c) {
   OMG_TRY
   OMG_ARG(h && c);
   h->H->useRccl(c->C.get());
   OMG_CATCH
}
int omg_set_option(const char *name, int value) {
   OMG_TRY
   OMG_ARG(name);
   if (!setTuningOption(name, value))
      OMEGA_ABORT(std::string("omg_set_option: no option named '") + name + "'");
   OMG_CATCH
}
int omg_get_option(const char *name, int *value) {
   OMG_TRY
   OMG_ARG(name && value);
   if (!getTuningOption(name, *value))
      OMEGA_ABORT(std::string("omg_get_option: no option named '") + name + "'");
   OMG_CATCH
}
int omg_set_timing_level(int level) {
   Pacer::timingLevel() = level;
   return 0;
}
int omg_peer_create(int nranks, int rank, size_t mailbox_bytes, omg_peer **out) {
   OMG_TRY
   OMG_ARG(out);
   newHandle(out, [&](omg_peer &R) { R.P.reset(new PeerWire(nranks, rank, mailbox_bytes)); });
   OMG_CATCH
}
int omg_peer_destroy(omg_peer *p) {
   delete p;
   return 0;
}
int omg_peer_local_handle(const omg_peer *p, char *out) {
   OMG_TRY
   OMG_ARG(p && out);
   p->P->localHandle(out);
   OMG_CATCH
}
int omg_peer_connect(omg_peer *p, const char *all_handles) {
   OMG_TRY
   OMG_ARG(p && all_handles);
   p->P->connect(all_handles);
   OMG_CATCH
}
int omg_peer_info(const omg_peer *p, int64_t *exchanges, int *status) {
   OMG_TRY
   OMG_ARG(p);
   if (exchanges)
      *exchanges = p->P->NExchanges;
   if (status)
      *status = p->P->status();
   OMG_CATCH
}
int omg_peer_set_timeout(omg_peer *p, double seconds) {
   OMG_TRY
   OMG_ARG(p);
   p->P->setTimeout(seconds);
   OMG_CATCH
}
int omg_halo_use_peer(omg_halo *h, omg_peer *p) {
   OMG_TRY
   OMG_ARG(h && p);
   h->H->usePeerWire(p->P.get());
   OMG_CATCH
}
int omg_halo_recv_rows(const omg_halo *h, size_t per_cell, size_t per_edge, size_t per_vertex, size_t *rows) {
   OMG_TRY
   OMG_ARG(h && rows);
   *rows = h->H->recvRows(per_cell, per_edge, per_vertex);
   OMG_CATCH
}
int omg_halo_set_transport(omg_halo *h, omg_transport_fn fn, void *ctx) {
   OMG_TRY
   OMG_ARG(h);
   h->H->setTransport((HaloTransportFn)fn, ctx);
   OMG_CATCH
}
int omg_halo_exchange(omg_halo *h, double *dev_array, int nt, int rows_size, int k, int row_pitch, int elem,
                      void *stream) {
   OMG_TRY
   OMG_ARG(h && dev_array && nt >= 1 && elem >= 0 && elem < 3 && k >= 1 && (row_pitch == 0 || row_pitch >= k));
   if (h->H->exchangeRaw(dev_array, nt, rows_size, k, row_pitch, (MeshElement)elem, (hipStream_t)stream) != 0)
      OMEGA_ABORT("Halo::exchangeFullArrayHalo failed" + h->H->wireError());
   OMG_CATCH
}

int omg_halo_exchange_bytes(omg_halo *h, void *dev_array, int elem_bytes, int nt, int rows_size, int k, int row_pitch,
                            int elem, void *stream) {
   OMG_TRY
   OMG_ARG(h && dev_array && (elem_bytes == 4 || elem_bytes == 8) && nt >= 1 && elem >= 0 && elem < 3 && k >= 1 &&
           (row_pitch == 0 || row_pitch >= k));
   if (h->H->exchangeRawBytes(dev_array, elem_bytes, nt, rows_size, k, row_pitch, (MeshElement)elem, (hipStream_t)stream) != 0)
      OMEGA_ABORT("Halo::exchangeFullArrayHalo failed" + h->H->wireError());
   OMG_CATCH
}
int omg_halo_exchange_i4(omg_halo *h, int32_t *dev_array, int nt, int rows_size, int k, int row_pitch, int elem,
                         void *stream) {
   return omg_halo_exchange_bytes(h, dev_array, 4, nt, rows_size, k, row_pitch, elem, stream);
}
int omg_halo_global_sum_dd(omg_halo *h, const double *local_hi_lo, int npairs, double *hi_lo, void *stream) {
   OMG_TRY
   OMG_ARG(h && local_hi_lo && hi_lo && npairs >= 0);
   if (h->H->globalSumDD(local_hi_lo, npairs, hi_lo, (hipStream_t)stream) != 0)
      OMEGA_ABORT("Halo::globalSumDD failed" + h->H->wireError());
   OMG_CATCH
}
int omg_halo_check(const omg_halo *h) {
   OMG_TRY
   OMG_ARG(h);
   if (h->H->checkWire() != 0)
      OMEGA_ABORT("Halo: the wire reports a failed exchange" + h->H->wireError());
   OMG_CATCH
}

// ---------------------------------------------------------------- HorzMesh
int omg_mesh_create(const omg_decomp *d, int nvertlayers, int host_only, omg_mesh **out) {
   OMG_TRY
   OMG_ARG(d && out);
   newHandle(out, [&](omg_mesh &R) { R.M.reset(new HorzMesh("Default", d->D.get(), nvertlayers, host_only != 0)); });
   OMG_CATCH
}
int omg_mesh_destroy(omg_mesh *m) {
   delete m;
   return 0;
}
int omg_mesh_get_int(const omg_mesh *m, const char *name, int32_t *out) {
   OMG_TRY
   OMG_ARG(m && name && out);
   const HorzMesh &M = *m->M;
   const std::map<std::string, I4> V{{"NCellsOwned", M.NCellsOwned},       {"NCellsAll", M.NCellsAll},
                                     {"NCellsSize", M.NCellsSize},         {"NEdgesOwned", M.NEdgesOwned},
                                     {"NEdgesAll", M.NEdgesAll},           {"NEdgesSize", M.NEdgesSize},
                                     {"NVerticesOwned", M.NVerticesOwned}, {"NVerticesAll", M.NVerticesAll},
                                     {"NVerticesSize", M.NVerticesSize},   {"MaxEdges", M.MaxEdges},
                                     {"MaxEdgesFile", M.MaxEdgesFile},
                                     {"MaxEdges2", M.MaxEdges2},           {"VertexDegree", M.VertexDegree},
                                     {"NVertLayers", M.NVertLayers},       {"MaxCellsOnEdge", M.MaxCellsOnEdge}};
   if (!M.HostOnly) { // kernel-side table statistics (diagnostics)
      const MeshView &W = M.view();
      const std::map<std::string, I4> D{{"PVChainOK", W.PVChainOK},
                                        {"CellPVOK", W.CellPVOK},
                                        {"CellL1OK", W.CellL1OK},
                                        {"CellPVFinalOK", W.CellPVFinalOK},
                                        {"NIrregularEdges", W.NIrregularEdges},
                                        {"NIrregularOwned", W.NIrregularOwned},
                                        {"NIrregularInner", W.NIrregularInner},
                                        {"DomM1", W.DomM1},
                                        {"NWideCells", W.NWideCells},
                                        {"NBadCells", W.NBadCells},
                                        {"NOrphanVertices", W.NOrphanVertices},
                                        {"NarrowTables", M.narrowView() ? 1 : 0},
                                        {"Del2RingOK", W.Del2RingOK},
                                        {"Del2VertOK", W.Del2VertOK},
                                        {"NBandCells", W.NBandCells},
                                        {"NBandSendCells", W.NBandSendCells},
                                        {"NInteriorCells", W.NInteriorCells},
                                        {"NPatchTiles8", M.NPatchTiles[0]},
                                        {"NPatchTiles16", M.NPatchTiles[1]},
                                        {"NPatchTiles32", M.NPatchTiles[2]},
                                        {"NPatchFallback8", M.NPatchFallback[0]},
                                        {"NPatchFallback16", M.NPatchFallback[1]},
                                        {"NPatchFallback32", M.NPatchFallback[2]}};
      auto Jt = D.find(name);
      if (Jt != D.end()) {
         *out = Jt->second;
         return 0;
      }
   }
   auto It = V.find(name);
   if (It == V.end())
      OMEGA_ABORT(std::string("HorzMesh: no integer member named ") + name);
   *out = It->second;
   OMG_CATCH
}
int omg_mesh_get_array_i4(const omg_mesh *m, const char *name, int32_t *out, size_t n) {
   OMG_TRY
   OMG_ARG(m && name && out);
   const HorzMesh &M = *m->M;
   const HostArrayI4 *A = findNamed<const HostArrayI4 *>(
       {{"CellsOnCell", &M.CellsOnCellH},       {"EdgesOnCell", &M.EdgesOnCellH},   {"NEdgesOnCell", &M.NEdgesOnCellH},
        {"VerticesOnCell", &M.VerticesOnCellH}, {"CellsOnEdge", &M.CellsOnEdgeH},   {"EdgesOnEdge", &M.EdgesOnEdgeH},
        {"NEdgesOnEdge", &M.NEdgesOnEdgeH},     {"VerticesOnEdge", &M.VerticesOnEdgeH},
        {"CellsOnVertex", &M.CellsOnVertexH},   {"EdgesOnVertex", &M.EdgesOnVertexH},
        {"NCellsHalo", &M.NCellsHaloH},         {"NEdgesHalo", &M.NEdgesHaloH},     {"NVerticesHalo", &M.NVerticesHaloH}},
       name, "HorzMesh: no int array member named ");
   copyOutI4(A->data(), A->size(), out, n, name);
   OMG_CATCH
}
int omg_mesh_get_array_r8(const omg_mesh *m, const char *name, double *out, size_t n) {
   OMG_TRY
   OMG_ARG(m && name && out);
   const HorzMesh &M = *m->M;
   if (std::strcmp(name, "EdgeMask") == 0) { // expanded to the reference's (NEdgesSize, NVertLayers) shape
      const HostArrayReal M2 = M.edgeMask2D();
      if (n < M2.size())
         OMEGA_ABORT("output buffer too small for EdgeMask");
      std::memcpy(out, M2.data(), M2.size() * sizeof(double));
      return 0;
   }
   const HostArrayReal *A = findNamed<const HostArrayReal *>(
       {{"XCell", &M.XCellH},           {"YCell", &M.YCellH},       {"ZCell", &M.ZCellH},
        {"LonCell", &M.LonCellH},       {"LatCell", &M.LatCellH},   {"XEdge", &M.XEdgeH},
        {"YEdge", &M.YEdgeH},           {"ZEdge", &M.ZEdgeH},       {"LonEdge", &M.LonEdgeH},
        {"LatEdge", &M.LatEdgeH},       {"XVertex", &M.XVertexH},   {"YVertex", &M.YVertexH},
        {"ZVertex", &M.ZVertexH},       {"LonVertex", &M.LonVertexH}, {"LatVertex", &M.LatVertexH},
        {"AreaCell", &M.AreaCellH},     {"AreaTriangle", &M.AreaTriangleH},
        {"KiteAreasOnVertex", &M.KiteAreasOnVertexH},               {"DvEdge", &M.DvEdgeH},
        {"DcEdge", &M.DcEdgeH},         {"AngleEdge", &M.AngleEdgeH}, {"WeightsOnEdge", &M.WeightsOnEdgeH},
        {"FEdge", &M.FEdgeH},           {"FCell", &M.FCellH},       {"FVertex", &M.FVertexH},
        {"BottomDepth", &M.BottomDepthH}, {"EdgeSignOnCell", &M.EdgeSignOnCellH},
        {"EdgeSignOnVertex", &M.EdgeSignOnVertexH},                 {"EdgeMask1D", &M.EdgeMask1DH},
        {"MeshScalingDel2", &M.MeshScalingDel2H},                   {"MeshScalingDel4", &M.MeshScalingDel4H}},
       name, "HorzMesh: no real array member named ");
   if (n < A->size())
      OMEGA_ABORT(std::string("output buffer too small for ") + name);
   std::memcpy(out, A->data(), A->size() * sizeof(double));
   OMG_CATCH
}
int omg_mesh_set_fvertex(omg_mesh *m, const double *host_values) {
   OMG_TRY
   OMG_ARG(m && host_values);
   m->M->setFVertex(host_values);
   OMG_CATCH
}

static void requireDevice(const HorzMesh *M) {
   OMEGA_REQUIRE(!M->HostOnly, "this mesh was created host-only: no device arrays, compute is unavailable");
}

// ---------------------------------------------------------------- options
#define OMG_HORZ_OP(NAME, LAUNCH, NALL)                                                                              \
   int NAME(const omg_mesh *m, const double *in, double *out, int k, int row_pitch, int n, void *stream) {         \
      OMG_TRY                                                                                                      \
      OMG_ARG(m && in && out && k > 0 && (row_pitch == 0 || row_pitch >= k));                                      \
      OMEGA_REQUIRE(!m->M->HostOnly, #NAME ": needs a device mesh");                                               \
      OMG_ARG(n <= m->M->NALL);                                                                                    \
      LAUNCH(m->M->view(), n < 0 ? m->M->NALL : n, k, row_pitch > 0 ? row_pitch : k, out, in, (hipStream_t)stream); \
      OMG_CATCH                                                                                                    \
   }
OMG_HORZ_OP(omg_horz_divergence, launchDivergenceOnCell, NCellsAll)
OMG_HORZ_OP(omg_horz_gradient, launchGradientOnEdge, NEdgesAll)
OMG_HORZ_OP(omg_horz_curl, launchCurlOnVertex, NVerticesAll)
OMG_HORZ_OP(omg_horz_tangential_recon, launchTangentialReconOnEdge, NEdgesAll)
#undef OMG_HORZ_OP
int omg_horz_interp_cell_to_edge(const omg_mesh *m, const double *cell, double *edge, int isotropic, int n, void *stream) {
   OMG_TRY
   OMG_ARG(m && cell && edge && n <= m->M->NEdgesAll);
   OMEGA_REQUIRE(!m->M->HostOnly, "omg_horz_interp_cell_to_edge: needs a device mesh");
   launchInterpCellToEdge(m->M->view(), n < 0 ? m->M->NEdgesAll : n, edge, cell, isotropic, (hipStream_t)stream);
   OMG_CATCH
}

void omg_tend_config_default(omg_tend_config *c) {
   const TendParams P;
   c->ThicknessFluxTendencyEnable   = P.ThicknessFluxTendencyEnable;
   c->PVTendencyEnable              = P.PVTendencyEnable;
   c->KETendencyEnable              = P.KETendencyEnable;
   c->SSHTendencyEnable             = P.SSHTendencyEnable;
   c->VelDiffTendencyEnable         = P.VelDiffTendencyEnable;
   c->VelHyperDiffTendencyEnable    = P.VelHyperDiffTendencyEnable;
   c->WindForcingTendencyEnable     = P.WindForcingTendencyEnable;
   c->BottomDragTendencyEnable      = P.BottomDragTendencyEnable;
   c->TracerHorzAdvTendencyEnable   = P.TracerHorzAdvTendencyEnable;
   c->TracerDiffTendencyEnable      = P.TracerDiffTendencyEnable;
   c->TracerHyperDiffTendencyEnable = P.TracerHyperDiffTendencyEnable;
   c->FluxThicknessUpwind           = P.FluxThicknessUpwind;
   c->FluxTracerUpwind              = P.FluxTracerUpwind;
   c->WindInterpIsotropic           = P.WindInterpIsotropic;
   c->ViscDel2 = P.ViscDel2, c->ViscDel4 = P.ViscDel4, c->DivFactor = P.DivFactor;
   c->EddyDiff2 = P.EddyDiff2, c->EddyDiff4 = P.EddyDiff4, c->Density0 = P.Density0;
   c->BottomDragCoeff = P.BottomDragCoeff;
}
static TendParams toParams(const omg_tend_config *c) {
   TendParams P;
   P.ThicknessFluxTendencyEnable   = c->ThicknessFluxTendencyEnable;
   P.PVTendencyEnable              = c->PVTendencyEnable;
   P.KETendencyEnable              = c->KETendencyEnable;
   P.SSHTendencyEnable             = c->SSHTendencyEnable;
   P.VelDiffTendencyEnable         = c->VelDiffTendencyEnable;
   P.VelHyperDiffTendencyEnable    = c->VelHyperDiffTendencyEnable;
   P.WindForcingTendencyEnable     = c->WindForcingTendencyEnable;
   P.BottomDragTendencyEnable      = c->BottomDragTendencyEnable;
   P.TracerHorzAdvTendencyEnable   = c->TracerHorzAdvTendencyEnable;
   P.TracerDiffTendencyEnable      = c->TracerDiffTendencyEnable;
   P.TracerHyperDiffTendencyEnable = c->TracerHyperDiffTendencyEnable;
   P.FluxThicknessUpwind           = c->FluxThicknessUpwind;
   P.FluxTracerUpwind              = c->FluxTracerUpwind;
   P.WindInterpIsotropic           = c->WindInterpIsotropic;
   P.ViscDel2 = c->ViscDel2, P.ViscDel4 = c->ViscDel4, P.DivFactor = c->DivFactor;
   P.EddyDiff2 = c->EddyDiff2, P.EddyDiff4 = c->EddyDiff4, P.Density0 = c->Density0;
   P.BottomDragCoeff = c->BottomDragCoeff;
   return P;
}

// ---------------------------------------------------------------- OceanState
int omg_state_create(const omg_mesh *m, omg_halo *halo, int nvertlayers, int ntimelevels, omg_state **out) {
   OMG_TRY
   OMG_ARG(m && out);
   requireDevice(m->M.get());
   newHandle(out, [&](omg_state &R) {
      R.S.reset(new OceanState("Default", m->M.get(), halo ? halo->H.get() : nullptr, nvertlayers, ntimelevels));
   });
   OMG_CATCH
}
int omg_state_destroy(omg_state *s) {
   delete s;
   return 0;
}
int omg_state_copy_to_device(omg_state *s, int tl, const double *h, const double *u) {
   OMG_TRY
   OMG_ARG(s);
   if (s->S->copyToDevice(h, u, tl) != 0)
      OMEGA_ABORT("OceanState: time level out of range");
   OMG_CATCH
}
int omg_state_copy_to_host(const omg_state *s, int tl, double *h, double *u) {
   OMG_TRY
   OMG_ARG(s);
   if (s->S->copyToHost(h, u, tl) != 0)
      OMEGA_ABORT("OceanState: time level out of range");
   OMG_CATCH
}
int omg_state_device_ptr(const omg_state *s, int tl, int which, double **dev) {
   OMG_TRY
   OMG_ARG(s && dev);
   Array2DReal A;
   const I4 E = which == 0 ? s->S->getLayerThickness(A, tl) : s->S->getNormalVelocity(A, tl);
   if (E != 0)
      OMEGA_ABORT("OceanState: time level out of range");
   *dev = A.Ptr;
   OMG_CATCH
}
int omg_state_exchange_halo(omg_state *s, int tl, void *stream) {
   OMG_TRY
   OMG_ARG(s);
   if (s->S->exchangeHalo(tl, (hipStream_t)stream) != 0)
      OMEGA_ABORT("OceanState::exchangeHalo failed");
   OMG_CATCH
}
int omg_halo_exchange_state(omg_halo *h, omg_state *s, int tl, omg_tracers *t, int tl_tr, void *stream) {
   OMG_TRY
   OMG_ARG(h && s);
   Array2DReal H, U;
   Array3DReal Tr;
   OMEGA_REQUIRE(s->S->getLayerThickness(H, tl) == 0 && s->S->getNormalVelocity(U, tl) == 0,
                 "omg_halo_exchange_state: bad state time level");
   const int NT = t ? t->T->NTracers : 0;
   if (NT > 0)
      OMEGA_REQUIRE(t->T->getAll(Tr, tl_tr) == 0, "omg_halo_exchange_state: bad tracer time level");
   if (h->H->exchangeState(H, U, NT > 0 ? &Tr : nullptr, NT, (hipStream_t)stream) != 0)
      OMEGA_ABORT("Halo::exchangeState failed" + h->H->wireError());
   OMG_CATCH
}
int omg_state_update_time_levels(omg_state *s, void *stream) {
   OMG_TRY
   OMG_ARG(s);
   s->S->updateTimeLevels((hipStream_t)stream);
   OMG_CATCH
}

// ---------------------------------------------------------------- Tracers
int omg_tracers_create(const omg_mesh *m, omg_halo *halo, int nvertlayers, int ntracers, int ntimelevels,
                       omg_tracers **out) {
   OMG_TRY
   OMG_ARG(m && out);
   requireDevice(m->M.get());
   newHandle(out, [&](omg_tracers &R) {
      R.T.reset(new TracerStore(m->M.get(), halo ? halo->H.get() : nullptr, nvertlayers, ntracers, ntimelevels));
   });
   OMG_CATCH
}
int omg_tracers_destroy(omg_tracers *t) {
   delete t;
   return 0;
}
int omg_tracers_copy_to_device(omg_tracers *t, int tl, const double *host) {
   OMG_TRY
   OMG_ARG(t && host);
   if (t->T->copyToDevice(host, tl) != 0)
      OMEGA_ABORT("Tracers: time level out of range");
   OMG_CATCH
}
int omg_tracers_copy_to_host(const omg_tracers *t, int tl, double *host) {
   OMG_TRY
   OMG_ARG(t && host);
   if (t->T->copyToHost(host, tl) != 0)
      OMEGA_ABORT("Tracers: time level out of range");
   OMG_CATCH
}
int omg_tracers_device_ptr(const omg_tracers *t, int tl, double **dev) {
   OMG_TRY
   OMG_ARG(t && dev);
   Array3DReal A;
   if (t->T->getAll(A, tl) != 0)
      OMEGA_ABORT("Tracers: time level out of range");
   *dev = A.Ptr;
   OMG_CATCH
}
int omg_tracers_exchange_halo(omg_tracers *t, int tl, void *stream) {
   OMG_TRY
   OMG_ARG(t);
   if (t->T->exchangeHalo(tl, (hipStream_t)stream) != 0)
      OMEGA_ABORT("Tracers::exchangeHalo failed");
   OMG_CATCH
}
int omg_tracers_update_time_levels(omg_tracers *t, void *stream) {
   OMG_TRY
   OMG_ARG(t);
   t->T->updateTimeLevels((hipStream_t)stream);
   OMG_CATCH
}

// ---------------------------------------------------------------- AuxiliaryState
int omg_aux_create(const omg_mesh *m, omg_halo *halo, int nvertlayers, int ntracers, omg_aux **out) {
   OMG_TRY
   OMG_ARG(m && out);
   requireDevice(m->M.get());
   newHandle(out, [&](omg_aux &R) {
      R.A.reset(new AuxiliaryState("Default", m->M.get(), halo ? halo->H.get() : nullptr, nvertlayers, ntracers));
   });
   OMG_CATCH
}
int omg_aux_destroy(omg_aux *a) {
   delete a;
   return 0;
}
int omg_aux_set_options(omg_aux *a, int ftu, int ftru, int wiso) {
   OMG_TRY
   OMG_ARG(a);
   a->A->LayerThicknessAux.FluxThickEdgeChoice = ftu ? FluxThickEdgeOption::Upwind : FluxThickEdgeOption::Center;
   a->A->TracerAux.TracersOnEdgeChoice         = ftru ? FluxTracerEdgeOption::Upwind : FluxTracerEdgeOption::Center;
   a->A->WindForcingAux.InterpChoice = wiso ? InterpCellToEdgeOption::Isotropic : InterpCellToEdgeOption::Anisotropic;
   OMG_CATCH
}
int omg_aux_compute_mom_aux(omg_aux *a, const omg_state *s, int ttl, int vtl, void *stream) {
   OMG_TRY
   OMG_ARG(a && s);
   a->A->computeMomAux(s->S.get(), ttl, vtl, (hipStream_t)stream);
   OMG_CATCH
}
static Array3DReal tracerArray(const omg_tracers *t, int tl) {
   Array3DReal A;
   OMEGA_REQUIRE(t != nullptr, "tracers handle is NULL");
   if (t->T->getAll(A, tl) != 0)
      OMEGA_ABORT("Tracers: time level out of range");
   return A;
}
int omg_aux_compute_all(omg_aux *a, const omg_state *s, const omg_tracers *t, int trtl, int ttl, int vtl,
                        void *stream) {
   OMG_TRY
   OMG_ARG(a && s);
   a->A->computeAll(s->S.get(), tracerArray(t, trtl), ttl, vtl, (hipStream_t)stream);
   OMG_CATCH
}
static ArrRef auxLookup(const AuxiliaryState &A, const char *Name) {
   return findNamed<ArrRef>({{"KineticEnergyCell", arrRef(A.KineticAux.KineticEnergyCell)},
                             {"VelocityDivCell", arrRef(A.KineticAux.VelocityDivCell)},
                             {"FluxLayerThickEdge", arrRef(A.LayerThicknessAux.FluxLayerThickEdge)},
                             {"MeanLayerThickEdge", arrRef(A.LayerThicknessAux.MeanLayerThickEdge)},
                             {"SshCell", arrRef(A.LayerThicknessAux.SshCell)},
                             {"RelVortVertex", arrRef(A.VorticityAux.RelVortVertex)},
                             {"NormRelVortVertex", arrRef(A.VorticityAux.NormRelVortVertex)},
                             {"NormPlanetVortVertex", arrRef(A.VorticityAux.NormPlanetVortVertex)},
                             {"NormRelVortEdge", arrRef(A.VorticityAux.NormRelVortEdge)},
                             {"NormPlanetVortEdge", arrRef(A.VorticityAux.NormPlanetVortEdge)},
                             {"Del2Edge", arrRef(A.VelocityDel2Aux.Del2Edge)},
                             {"Del2DivCell", arrRef(A.VelocityDel2Aux.Del2DivCell)},
                             {"Del2RelVortVertex", arrRef(A.VelocityDel2Aux.Del2RelVortVertex)},
                             {"HTracersEdge", arrRef(A.TracerAux.HTracersEdge)},
                             {"Del2TracersCell", arrRef(A.TracerAux.Del2TracersCell)},
                             {"NormalStressEdge", arrRef(A.WindForcingAux.NormalStressEdge)},
                             {"ZonalStressCell", arrRef(A.WindForcingAux.ZonalStressCell)},
                             {"MeridStressCell", arrRef(A.WindForcingAux.MeridStressCell)}},
                            Name, "AuxiliaryState: no array named ");
}
OMG_NAMED_ARRAYS(omg_aux_copy_to_host, omg_aux_copy_to_device, omg_aux_device_ptr, omg_aux, a, auxLookup(*a->A, name))

// ---------------------------------------------------------------- Tendencies
static int tendCreate(const omg_mesh *m, int nvertlayers, int ntracers, const omg_tend_config *c, omg_tend **out, bool Allow) {
   OMG_TRY
   OMG_ARG(m && out);
   requireDevice(m->M.get());
   newHandle(out, [&](omg_tend &R) {
      R.T.reset(new Tendencies("Default", m->M.get(), nvertlayers, ntracers, c ? toParams(c) : TendParams(), Allow));
   });
   OMG_CATCH
}
int omg_tend_create(const omg_mesh *m, int nvertlayers, int ntracers, const omg_tend_config *c, omg_tend **out) {
   return tendCreate(m, nvertlayers, ntracers, c, out, false);
}
int omg_tend_create_reference_structured(const omg_mesh *m, int nvertlayers, int ntracers, const omg_tend_config *c,
                                         omg_tend **out) {
   return tendCreate(m, nvertlayers, ntracers, c, out, true);
}
int omg_tend_fused_limit(int64_t ncells_size, int64_t nedges_size, int64_t nvertices_size, int max_edges, int nvertlayers,
                         int *supported, char *why, size_t why_bytes) {
   OMG_TRY
   OMG_ARG(supported && ncells_size >= 0 && nedges_size >= 0 && nvertices_size >= 0 && nvertlayers > 0);
   const std::string W = Tendencies::fusedLimit((size_t)ncells_size, (size_t)nedges_size, (size_t)nvertices_size, max_edges,
                                                nvertlayers);
   if (why && why_bytes > 0) {
      std::strncpy(why, W.c_str(), why_bytes - 1);
      why[why_bytes - 1] = 0;
   }
   *supported = W.empty() ? 1 : 0;
   OMG_CATCH
}
int omg_tend_destroy(omg_tend *t) {
   delete t;
   return 0;
}
int omg_tend_set_fused(omg_tend *t, int use_fused_rhs) {
   OMG_TRY
   OMG_ARG(t);
   t->T->UseFusedRHS = use_fused_rhs != 0;
   OMG_CATCH
}
int omg_tend_set_graphs(omg_tend *t, int use_graphs) {
   OMG_TRY
   OMG_ARG(t);
   t->T->UseGraphs = use_graphs != 0;
   OMG_CATCH
}
int omg_tend_graph_stats(const omg_tend *t, int64_t *captures, int64_t *replays) {
   OMG_TRY
   OMG_ARG(t);
   if (captures)
      *captures = t->T->Graphs.NCaptures;
   if (replays)
      *replays = t->T->Graphs.NReplays;
   OMG_CATCH
}
int omg_stepper_graph_stats(const omg_stepper *st, int64_t *captures, int64_t *replays) {
   OMG_TRY
   OMG_ARG(st);
   auto *Rk4 = dynamic_cast<RungeKutta4Stepper *>(st->St.get());
   if (captures)
      *captures = Rk4 ? Rk4->Graphs.NCaptures : 0;
   if (replays)
      *replays = Rk4 ? Rk4->Graphs.NReplays : 0;
   OMG_CATCH
}
int omg_tend_compute_all(omg_tend *t, const omg_state *s, omg_aux *a, const omg_tracers *tr, int trtl, int ttl,
                         int vtl, void *stream) {
   OMG_TRY
   OMG_ARG(t && s && a);
   t->T->computeAllTendencies(s->S.get(), a->A.get(), tracerArray(tr, trtl), ttl, vtl, (hipStream_t)stream);
   OMG_CATCH
}
int omg_tend_compute_thickness(omg_tend *t, const omg_state *s, omg_aux *a, int ttl, int vtl, void *stream) {
   OMG_TRY
   OMG_ARG(t && s && a);
   t->T->computeThicknessTendencies(s->S.get(), a->A.get(), ttl, vtl, (hipStream_t)stream);
   OMG_CATCH
}
int omg_tend_compute_velocity(omg_tend *t, const omg_state *s, omg_aux *a, int ttl, int vtl, void *stream) {
   OMG_TRY
   OMG_ARG(t && s && a);
   t->T->computeVelocityTendencies(s->S.get(), a->A.get(), ttl, vtl, (hipStream_t)stream);
   OMG_CATCH
}
int omg_tend_compute_tracer(omg_tend *t, const omg_state *s, omg_aux *a, const omg_tracers *tr, int trtl, int ttl,
                            int vtl, void *stream) {
   OMG_TRY
   OMG_ARG(t && s && a);
   t->T->computeTracerTendencies(s->S.get(), a->A.get(), tracerArray(tr, trtl), ttl, vtl, (hipStream_t)stream);
   OMG_CATCH
}
int omg_tend_compute_transport(omg_tend *t, const omg_state *s, omg_aux *a, const omg_tracers *tr, int trtl, int ttl,
                               int vtl, void *stream) {
   OMG_TRY
   OMG_ARG(t && s && a);
   t->T->computeTransportTendencies(s->S.get(), a->A.get(), tracerArray(tr, trtl), ttl, vtl, (hipStream_t)stream);
   OMG_CATCH
}
int omg_tend_compute_transport_update(omg_tend *t, omg_state *s, omg_aux *a, omg_tracers *tr, int trtl, int ttl, int vtl,
                                      int next_ttl, int next_trtl, double coeff, int keep_tendencies, void *stream) {
   OMG_TRY
   OMG_ARG(t && s && a);
   Array2DReal NextThick;
   OMEGA_REQUIRE(s->S->getLayerThickness(NextThick, next_ttl) == 0, "Tendencies: bad time level");
   t->T->computeTransportTendenciesAndUpdate(s->S.get(), a->A.get(), tracerArray(tr, trtl), ttl, vtl, NextThick,
                                             tracerArray(tr, next_trtl), coeff, keep_tendencies != 0, (hipStream_t)stream);
   OMG_CATCH
}
int omg_tend_compute_momentum(omg_tend *t, const omg_state *s, omg_aux *a, const omg_tracers *tr, int trtl, int ttl,
                              int vtl, void *stream) {
   OMG_TRY
   OMG_ARG(t && s && a);
   t->T->computeMomentumTendencies(s->S.get(), a->A.get(), tracerArray(tr, trtl), ttl, vtl, (hipStream_t)stream);
   OMG_CATCH
}
int omg_tend_compute_thickness_only(omg_tend *t, const omg_state *s, omg_aux *a, int ttl, int vtl, void *stream) {
   OMG_TRY
   OMG_ARG(t && s && a);
   t->T->computeThicknessTendenciesOnly(s->S.get(), a->A.get(), ttl, vtl, (hipStream_t)stream);
   OMG_CATCH
}
int omg_tend_compute_velocity_only(omg_tend *t, const omg_state *s, omg_aux *a, int ttl, int vtl, void *stream) {
   OMG_TRY
   OMG_ARG(t && s && a);
   t->T->computeVelocityTendenciesOnly(s->S.get(), a->A.get(), ttl, vtl, (hipStream_t)stream);
   OMG_CATCH
}
int omg_tend_compute_tracer_only(omg_tend *t, const omg_state *s, omg_aux *a, const omg_tracers *tr, int trtl,
                                 int ttl, int vtl, void *stream) {
   OMG_TRY
   OMG_ARG(t && s && a);
   t->T->computeTracerTendenciesOnly(s->S.get(), a->A.get(), tracerArray(tr, trtl), ttl, vtl, (hipStream_t)stream);
   OMG_CATCH
}
int omg_tend_use_manufactured_solution(omg_tend *t, const omg_mesh *m, double wavelength_x, double wavelength_y,
                                       double amplitude) {
   OMG_TRY
   OMG_ARG(t && m);
   const TendParams &P = t->T->Params;
   auto Ms = std::make_shared<ManufacturedSolution>(m->M.get(), wavelength_x, wavelength_y, amplitude,
                                                    P.VelDiffTendencyEnable != 0, P.VelHyperDiffTendencyEnable != 0,
                                                    P.ViscDel2, P.ViscDel4);
   t->Ms                     = Ms;
   t->T->CustomThicknessTend = [Ms](const Array2DReal &Tend, const OceanState *, const AuxiliaryState *, int, int,
                                    R8 Time, hipStream_t S) { Ms->thicknessTendency(Tend, Time, S); };
   t->T->CustomVelocityTend  = [Ms](const Array2DReal &Tend, const OceanState *, const AuxiliaryState *, int, int,
                                    R8 Time, hipStream_t S) { Ms->velocityTendency(Tend, Time, S); };
   OMG_CATCH
}
int omg_tend_set_custom_tendency(omg_tend *t, int which, omg_custom_tend_fn fn, void *ctx) {
   OMG_TRY
   OMG_ARG(t && (which == 0 || which == 1));
   Tendencies::CustomTendencyType F;
   if (fn) {
      const HorzMesh *M = t->T->Mesh;
      const int NAll = which == 0 ? M->NCellsAll : M->NEdgesAll, NSize = which == 0 ? M->NCellsSize : M->NEdgesSize;
      F = [fn, ctx, NAll, NSize](const Array2DReal &Tend, const OceanState *State, const AuxiliaryState *, int ThickLvl,
                                 int VelLvl, R8 Time, hipStream_t S) {
         Array2DReal H, U;
         OMEGA_REQUIRE(State->getLayerThickness(H, ThickLvl) == 0 && State->getNormalVelocity(U, VelLvl) == 0,
                       "custom tendency: bad time level");
         OMEGA_REQUIRE(fn(ctx, Tend.Ptr, H.Ptr, U.Ptr, NAll, NSize, Tend.Ext[1], Tend.Pitch, Time, (void *)S) == 0,
                       "custom tendency callback reported an error");
      };
   }
   (which == 0 ? t->T->CustomThicknessTend : t->T->CustomVelocityTend) = F;
   OMG_CATCH
}
int omg_tend_clear_custom_tendencies(omg_tend *t) {
   OMG_TRY
   OMG_ARG(t);
   t->T->CustomThicknessTend = nullptr;
   t->T->CustomVelocityTend  = nullptr;
   t->Ms.reset();
   OMG_CATCH
}
int omg_tend_set_time(omg_tend *t, double seconds) {
   OMG_TRY
   OMG_ARG(t);
   t->T->ModelTime = seconds;
   OMG_CATCH
}
int omg_tend_kernel_timing(omg_tend *t, int enable) {
   OMG_TRY
   OMG_ARG(t);
   t->T->enableKernelTiming(enable != 0);
   OMG_CATCH
}
int omg_tend_collect_kernel_times(omg_tend *t, double *ms_sum, int *n_kernels, int *n_samples) {
   OMG_TRY
   OMG_ARG(t && ms_sum && n_kernels && n_samples);
   *n_samples = t->T->collectKernelTimes(ms_sum);
   *n_kernels = FusedNumKernels;
   OMG_CATCH
}
const char *omg_tend_kernel_name(int i) { return (i >= 0 && i < FusedNumKernels) ? FusedKernelNames[i] : ""; }
static ArrRef tendLookup(const Tendencies &T, int Which) {
   switch (Which) {
   case 0:
      return arrRef(T.LayerThicknessTend);
   case 1:
      return arrRef(T.NormalVelocityTend);
   case 2:
      return arrRef(T.TracerTend);
   default:
      OMEGA_ABORT("Tendencies: `which` must be 0, 1 or 2");
   }
}
int omg_tend_copy_to_host(const omg_tend *t, int which, double *host, size_t n) {
   OMG_TRY
   OMG_ARG(t && host);
   refCopyToHost(tendLookup(*t->T, which), "tendency array", host, n);
   OMG_CATCH
}
int omg_tend_device_ptr(const omg_tend *t, int which, double **dev, size_t *n) {
   OMG_TRY
   OMG_ARG(t && dev);
   refPointerOut(tendLookup(*t->T, which), dev, n);
   OMG_CATCH
}
int omg_level_pitch(int nvertlayers) { return levelPitch(nvertlayers); }

// ---------------------------------------------------------------- TimeStepper
int omg_stepper_create(const char *type, double dt, omg_tend *t, omg_aux *a, const omg_mesh *m, omg_halo *halo,
                       omg_tracers *tr, omg_stepper **out) {
   OMG_TRY
   OMG_ARG(type && t && a && m && tr && out);
   const TimeStepperType Ty = TimeStepper::getFromStr(type);
   if (Ty == TimeStepperType::Invalid)
      OMEGA_ABORT(std::string("TimeStepper: unknown type ") + type);
   newHandle(out, [&](omg_stepper &R) {
      R.St.reset(TimeStepper::make("Default", Ty, dt));
      R.St->attachData(t->T.get(), a->A.get(), m->M.get(), halo ? halo->H.get() : nullptr, tr->T.get());
      R.St->finalizeInit();
   });
   OMG_CATCH
}
int omg_stepper_destroy(omg_stepper *st) {
   delete st;
   return 0;
}
int omg_stepper_do_step(omg_stepper *st, omg_state *s, void *stream) {
   OMG_TRY
   OMG_ARG(st && s);
   st->St->doStep(s->S.get(), (hipStream_t)stream);
   OMG_CATCH
}
int omg_stepper_change_time_step(omg_stepper *st, double dt) {
   OMG_TRY
   OMG_ARG(st && dt > 0);
   st->St->changeTimeStep(dt);
   OMG_CATCH
}
int omg_update_by_tend(double *out, const double *in, const double *tend, double coeff, int n_rows, int k, void *stream) {
   OMG_TRY
   OMG_ARG(out && in && tend && n_rows >= 0 && k > 0);
   launchUpdateByTend(n_rows, k, out, in, tend, coeff, (hipStream_t)stream);
   OMG_CATCH
}
int omg_update_tracers_by_tend(double *next, const double *cur, const double *h_next, const double *h_cur, const double *tend,
                               double coeff, int n_tracers, int n_rows, int rows_size, int k, void *stream) {
   OMG_TRY
   OMG_ARG(next && cur && h_next && h_cur && tend && n_tracers >= 0 && n_rows >= 0 && rows_size >= n_rows && k > 0);
   launchUpdateTracersByTend(n_tracers, n_rows, rows_size, k, next, cur, h_next, h_cur, tend, coeff, (hipStream_t)stream);
   OMG_CATCH
}
int omg_stepper_set_start_time(omg_stepper *st, double seconds) {
   OMG_TRY
   OMG_ARG(st);
   st->St->StartTime = seconds - (double)st->St->NStepsDone * st->St->TimeStepSeconds;
   OMG_CATCH
}
int omg_stepper_get_time(const omg_stepper *st, double *seconds) {
   OMG_TRY
   OMG_ARG(st && seconds);
   *seconds = st->St->simTime();
   OMG_CATCH
}
int omg_stepper_set_option(omg_stepper *st, const char *name, int value) {
   OMG_TRY
   OMG_ARG(st && name);
   auto *Rk4 = dynamic_cast<RungeKutta4Stepper *>(st->St.get());
   const std::string N(name);
   if (Rk4 && N == "FuseStageUpdates")
      Rk4->FuseStageUpdates = value != 0;
   else if (Rk4 && N == "StoreStageTendencies")
      Rk4->StoreStageTendencies = value != 0;
   else if (Rk4 && N == "OverlapHaloExchange")
      Rk4->OverlapHaloExchange = value != 0;
   else if (Rk4 && N == "UseGraphs")
      Rk4->UseGraphs = value != 0;
   else
      OMEGA_ABORT("TimeStepper: no option named " + N + " for this scheme");
   OMG_CATCH
}
int omg_stepper_coeff_seconds(double mult, double dt, double *out) {
   OMG_TRY
   OMG_ARG(out);
   *out = TimeStepper::coeffSeconds(mult, dt);
   OMG_CATCH
}

// ---------------------------------------------------------------- VertCoord / Eos
/// a raw device array [rows][levelPitch(k)] of the caller's as a 2-D array handle (no ownership)
static Array2DReal levelView(const double *Dev, int Rows, int K) {
   Array2DReal A;
   A.Ptr    = const_cast<Real *>(Dev);
   A.Ext[0] = Rows, A.Ext[1] = K;
   A.Pitch  = levelPitch(K);
   return A;
}
/// a raw device array [ntracers][rows][levelPitch(k)] of the caller's as a 3-D array handle (no ownership)
static Array3DReal tracerView(const double *Dev, int NTracers, int Rows, int K) {
   Array3DReal A;
   A.Ptr    = const_cast<Real *>(Dev);
   A.Ext[0] = NTracers, A.Ext[1] = Rows, A.Ext[2] = K;
   A.Pitch  = levelPitch(K);
   return A;
}
/// a raw device array [rows] of the caller's (NULL: empty, read as zero)
static Array1DReal cellView(const double *Dev, int Rows) {
   Array1DReal A;
   A.Ptr    = const_cast<Real *>(Dev);
   A.Ext[0] = Dev ? Rows : 0;
   A.Pitch  = 1;
   return A;
}
int omg_vcoord_create(const omg_mesh *m, const omg_decomp *d, int nvertlayers, double rho0,
                      const char *movement_weight_type, const int32_t *min_level_cell, const int32_t *max_level_cell,
                      omg_vcoord **out) {
   OMG_TRY
   OMG_ARG(m && out && movement_weight_type);
   newHandle(out, [&](omg_vcoord &R) {
      R.V.reset(new VertCoord("Default", m->M.get(), d ? d->D.get() : nullptr, nvertlayers, rho0,
                              movement_weight_type, min_level_cell, max_level_cell));
   });
   OMG_CATCH
}
int omg_vcoord_destroy(omg_vcoord *v) {
   delete v;
   return 0;
}
int omg_vcoord_min_max_layer_edge(omg_vcoord *v, void *stream) {
   OMG_TRY
   OMG_ARG(v);
   v->V->minMaxLayerEdge((hipStream_t)stream);
   OMG_CATCH
}
int omg_vcoord_min_max_layer_vertex(omg_vcoord *v, void *stream) {
   OMG_TRY
   OMG_ARG(v);
   v->V->minMaxLayerVertex((hipStream_t)stream);
   OMG_CATCH
}
int omg_vcoord_compute_pressure(omg_vcoord *v, const double *layer_thickness, const double *surface_pressure,
                                void *stream) {
   OMG_TRY
   OMG_ARG(v && layer_thickness);
   const HorzMesh *M = v->V->Mesh;
   v->V->computePressure(levelView(layer_thickness, M->NCellsSize, v->V->NVertLayers),
                         cellView(surface_pressure, M->NCellsSize), (hipStream_t)stream);
   OMG_CATCH
}
int omg_vcoord_compute_zheight(omg_vcoord *v, const double *layer_thickness, const double *spec_vol, void *stream) {
   OMG_TRY
   OMG_ARG(v && layer_thickness && spec_vol);
   const HorzMesh *M = v->V->Mesh;
   v->V->computeZHeight(levelView(layer_thickness, M->NCellsSize, v->V->NVertLayers),
                        levelView(spec_vol, M->NCellsSize, v->V->NVertLayers), (hipStream_t)stream);
   OMG_CATCH
}
int omg_vcoord_compute_geopotential(omg_vcoord *v, const double *tidal_potential,
                                    const double *self_attraction_loading, void *stream) {
   OMG_TRY
   OMG_ARG(v);
   const HorzMesh *M = v->V->Mesh;
   v->V->computeGeopotential(cellView(tidal_potential, M->NCellsSize), cellView(self_attraction_loading, M->NCellsSize),
                             (hipStream_t)stream);
   OMG_CATCH
}
int omg_vcoord_compute_target_thickness(omg_vcoord *v, void *stream) {
   OMG_TRY
   OMG_ARG(v);
   v->V->computeTargetThickness((hipStream_t)stream);
   OMG_CATCH
}
int omg_vcoord_compute_column(omg_vcoord *v, const omg_state *s, int thick_time_level, const omg_tracers *t,
                              int tracer_time_level, const omg_eos *e, int temp_index, int salt_index,
                              const double *surface_pressure, const double *tidal_potential,
                              const double *self_attraction_loading, int displaced, int kdisp, void *stream) {
   OMG_TRY
   OMG_ARG(v && s && t && e);
   const int N = v->V->Mesh->NCellsSize;
   v->V->computeColumn(s->S.get(), thick_time_level, t->T.get(), tracer_time_level, *e->E, cellView(surface_pressure, N),
                       cellView(tidal_potential, N), cellView(self_attraction_loading, N), displaced != 0, kdisp,
                       (hipStream_t)stream, temp_index, salt_index);
   OMG_CATCH
}
static ArrRef vcoordLookup(const VertCoord &V, const char *Name) {
   return findNamed<ArrRef>({{"PressureInterface", arrRef(V.PressureInterface)},
                             {"PressureMid", arrRef(V.PressureMid)},
                             {"ZInterface", arrRef(V.ZInterface)},
                             {"ZMid", arrRef(V.ZMid)},
                             {"GeopotentialMid", arrRef(V.GeopotentialMid)},
                             {"LayerThicknessTarget", arrRef(V.LayerThicknessTarget)},
                             {"RefLayerThickness", arrRef(V.RefLayerThickness)},
                             {"VertCoordMovementWeights", arrRef(V.VertCoordMovementWeights)},
                             {"BottomDepth", arrRef(V.BottomDepth)}},
                            Name, "VertCoord: no real array named ");
}
static const Array1DI4 &vcoordLookupI4(const VertCoord &V, const char *Name) {
   return *findNamed<const Array1DI4 *>(
       {{"MinLayerCell", &V.MinLayerCell},           {"MaxLayerCell", &V.MaxLayerCell},
        {"MinLayerEdgeTop", &V.MinLayerEdgeTop},     {"MaxLayerEdgeTop", &V.MaxLayerEdgeTop},
        {"MinLayerEdgeBot", &V.MinLayerEdgeBot},     {"MaxLayerEdgeBot", &V.MaxLayerEdgeBot},
        {"MinLayerVertexTop", &V.MinLayerVertexTop}, {"MaxLayerVertexTop", &V.MaxLayerVertexTop},
        {"MinLayerVertexBot", &V.MinLayerVertexBot}, {"MaxLayerVertexBot", &V.MaxLayerVertexBot}},
       Name, "VertCoord: no integer array named ");
}
OMG_NAMED_ARRAYS(omg_vcoord_copy_to_host, omg_vcoord_copy_to_device, omg_vcoord_device_ptr, omg_vcoord, v,
                 vcoordLookup(*v->V, name))
int omg_vcoord_copy_to_host_i4(const omg_vcoord *v, const char *name, int32_t *host, size_t n) {
   OMG_TRY
   OMG_ARG(v && name && host);
   const Array1DI4 &A = vcoordLookupI4(*v->V, name);
   if (n < A.size())
      OMEGA_ABORT(std::string("output buffer too small for ") + name);
   HIP_CHECK(hipDeviceSynchronize());
   copyToHost(host, A.Ptr, A.bytes());
   OMG_CATCH
}
int omg_vcoord_copy_to_device_i4(omg_vcoord *v, const char *name, const int32_t *host, size_t n) {
   OMG_TRY
   OMG_ARG(v && name && host);
   const Array1DI4 &A = vcoordLookupI4(*v->V, name);
   if (n != A.size())
      OMEGA_ABORT(std::string("size mismatch for ") + name);
   HIP_CHECK(hipDeviceSynchronize());
   copyToDevice(A.Ptr, host, A.bytes());
   HIP_CHECK(hipDeviceSynchronize());
   OMG_CATCH
}
int omg_vcoord_get_real(const omg_vcoord *v, const char *name, double *value) {
   OMG_TRY
   OMG_ARG(v && name && value);
   const std::string N(name);
   if (N == "Rho0")
      *value = v->V->Rho0;
   else if (N == "Gravity")
      *value = VertCoord::Gravity;
   else
      OMEGA_ABORT("VertCoord: no scalar named " + N);
   OMG_CATCH
}

int omg_eos_create(const omg_mesh *m, int nvertlayers, const char *eos_type, double drhodt, double drhods,
                   double rhot0s0, omg_eos **out) {
   OMG_TRY
   OMG_ARG(m && out && eos_type);
   newHandle(out, [&](omg_eos &R) {
      R.E.reset(new Eos("Default", m->M.get(), nvertlayers, eos_type, drhodt, drhods, rhot0s0));
   });
   OMG_CATCH
}
int omg_eos_destroy(omg_eos *e) {
   delete e;
   return 0;
}
int omg_eos_compute_spec_vol(omg_eos *e, const double *conserv_temp, const double *abs_salinity,
                             const double *pressure, double p_scale, void *stream) {
   OMG_TRY
   OMG_ARG(e && conserv_temp && abs_salinity && pressure);
   const int N = e->E->Mesh->NCellsSize, K = e->E->NVertLayers;
   e->E->computeSpecVol(levelView(conserv_temp, N, K), levelView(abs_salinity, N, K), levelView(pressure, N, K),
                        p_scale, (hipStream_t)stream);
   OMG_CATCH
}
int omg_eos_compute_spec_vol_disp(omg_eos *e, const double *conserv_temp, const double *abs_salinity,
                                  const double *pressure, int kdisp, double p_scale, void *stream) {
   OMG_TRY
   OMG_ARG(e && conserv_temp && abs_salinity && pressure);
   const int N = e->E->Mesh->NCellsSize, K = e->E->NVertLayers;
   e->E->computeSpecVolDisp(levelView(conserv_temp, N, K), levelView(abs_salinity, N, K), levelView(pressure, N, K),
                            kdisp, p_scale, (hipStream_t)stream);
   OMG_CATCH
}
static ArrRef eosLookup(const Eos &E, const char *Name) {
   return findNamed<ArrRef>({{"SpecVol", arrRef(E.SpecVol)}, {"SpecVolDisplaced", arrRef(E.SpecVolDisplaced)}}, Name,
                            "Eos: no array named ");
}
OMG_NAMED_ARRAYS(omg_eos_copy_to_host, omg_eos_copy_to_device, omg_eos_device_ptr, omg_eos, e, eosLookup(*e->E, name))

// ---- VertMix (VertMix.h)
static VertMixConfig toVertMixConfig(const omg_vertmix_config &c) {
   VertMixConfig V;
   V.BackgroundViscosity   = c.BackgroundViscosity;
   V.BackgroundDiffusivity = c.BackgroundDiffusivity;
   V.EnableShearMix        = c.EnableShearMix != 0;
   V.ShearNuZero           = c.ShearNuZero;
   V.ShearAlpha            = c.ShearAlpha;
   V.ShearExponent         = c.ShearExponent;
   V.EnableConvectiveMix   = c.EnableConvectiveMix != 0;
   V.ConvectiveDiffusivity = c.ConvectiveDiffusivity;
   V.ConvectiveTriggerBVF  = c.ConvectiveTriggerBVF;
   return V;
}
int omg_vertmix_config_default(omg_vertmix_config *c) {
   OMG_TRY
   OMG_ARG(c);
   const VertMixConfig V;
   c->BackgroundViscosity   = V.BackgroundViscosity;
   c->BackgroundDiffusivity = V.BackgroundDiffusivity;
   c->EnableShearMix        = V.EnableShearMix;
   c->ShearNuZero           = V.ShearNuZero;
   c->ShearAlpha            = V.ShearAlpha;
   c->ShearExponent         = V.ShearExponent;
   c->EnableConvectiveMix   = V.EnableConvectiveMix;
   c->ConvectiveDiffusivity = V.ConvectiveDiffusivity;
   c->ConvectiveTriggerBVF  = V.ConvectiveTriggerBVF;
   OMG_CATCH
}
int omg_vertmix_create(const omg_mesh *m, const omg_vcoord *v, const omg_vertmix_config *c, omg_vertmix **out) {
   OMG_TRY
   OMG_ARG(m && out);
   const VertMixConfig Cfg = c ? toVertMixConfig(*c) : VertMixConfig();
   newHandle(out, [&](omg_vertmix &R) {
      R.X.reset(new VertMix("Default", m->M.get(), v ? v->V.get() : nullptr, Cfg));
   });
   OMG_CATCH
}
int omg_vertmix_destroy(omg_vertmix *x) {
   delete x;
   return 0;
}
int omg_vertmix_compute_bvf(omg_vertmix *x, const omg_eos *e, void *stream) {
   OMG_TRY
   OMG_ARG(x && e);
   x->X->computeBruntVaisalaFreqSq(*e->E, (hipStream_t)stream);
   OMG_CATCH
}
int omg_vertmix_compute(omg_vertmix *x, const double *normal_velocity, const double *tangential_velocity,
                        const double *bvf, void *stream) {
   OMG_TRY
   OMG_ARG(x && normal_velocity && tangential_velocity);
   const HorzMesh *M = x->X->Mesh;
   const int K       = x->X->NVertLayers;
   x->X->computeVertMix(levelView(normal_velocity, M->NEdgesSize, K), levelView(tangential_velocity, M->NEdgesSize, K),
                        bvf ? levelView(bvf, M->NCellsSize, K) : x->X->BruntVaisalaFreqSq, (hipStream_t)stream);
   OMG_CATCH
}
int omg_vertmix_apply_tracers(omg_vertmix *x, const double *layer_thickness, double *tracers, int ntracers, double dt,
                              void *stream) {
   OMG_TRY
   OMG_ARG(x && layer_thickness && ntracers >= 0 && (tracers || ntracers == 0));
   const HorzMesh *M = x->X->Mesh;
   const int K       = x->X->NVertLayers;
   x->X->applyTracerVertMix(levelView(layer_thickness, M->NCellsSize, K), tracerView(tracers, ntracers, M->NCellsSize, K),
                            ntracers, dt, (hipStream_t)stream);
   OMG_CATCH
}
int omg_vertmix_apply_velocity(omg_vertmix *x, const double *layer_thickness, double *normal_velocity, double dt,
                               void *stream) {
   OMG_TRY
   OMG_ARG(x && layer_thickness && normal_velocity);
   const HorzMesh *M = x->X->Mesh;
   const int K       = x->X->NVertLayers;
   x->X->applyVelocityVertMix(levelView(layer_thickness, M->NCellsSize, K), levelView(normal_velocity, M->NEdgesSize, K),
                              dt, (hipStream_t)stream);
   OMG_CATCH
}
/// a raw device array [ntracers][rows] of the caller's (NULL: empty, an absent array)
static Array2DReal fluxView(const double *Dev, int NTracers, int Rows) {
   Array2DReal A;
   A.Ptr    = const_cast<Real *>(Dev);
   A.Ext[0] = Dev ? NTracers : 0, A.Ext[1] = Dev ? Rows : 0;
   A.Pitch  = Rows;
   return A;
}
int omg_vertmix_apply_tracers_forced(omg_vertmix *x, const double *layer_thickness, double *tracers, int ntracers,
                                     double dt, const double *surface_flux, void *stream) {
   OMG_TRY
   OMG_ARG(x && layer_thickness && ntracers >= 0 && (tracers || ntracers == 0));
   const HorzMesh *M = x->X->Mesh;
   const int K       = x->X->NVertLayers;
   x->X->applyTracerVertMix(levelView(layer_thickness, M->NCellsSize, K), tracerView(tracers, ntracers, M->NCellsSize, K),
                            ntracers, dt, fluxView(surface_flux, ntracers, M->NCellsSize), (hipStream_t)stream);
   OMG_CATCH
}
int omg_vertmix_apply_velocity_forced(omg_vertmix *x, const double *layer_thickness, double *normal_velocity, double dt,
                                      double bottom_drag_coeff, double rayleigh_drag_coeff, const double *normal_stress,
                                      const double *tangential_velocity, void *stream) {
   OMG_TRY
   VertMixBoundary B;
   B.BottomDragCoeff = bottom_drag_coeff, B.RayleighDragCoeff = rayleigh_drag_coeff;
   VertMix::requireBoundary(B); // the coefficients first: they need no object to be judged
   OMG_ARG(x && layer_thickness && normal_velocity);
   const HorzMesh *M = x->X->Mesh;
   const int K       = x->X->NVertLayers;
   x->X->applyVelocityVertMix(levelView(layer_thickness, M->NCellsSize, K), levelView(normal_velocity, M->NEdgesSize, K),
                              dt, B, cellView(normal_stress, M->NEdgesSize),
                              tangential_velocity ? levelView(tangential_velocity, M->NEdgesSize, K) : Array2DReal(),
                              (hipStream_t)stream);
   OMG_CATCH
}
static ArrRef vertMixLookup(const VertMix &X, const char *Name) {
   return findNamed<ArrRef>({{"VertDiff", arrRef(X.VertDiff)},
                             {"VertVisc", arrRef(X.VertVisc)},
                             {"BruntVaisalaFreqSq", arrRef(X.BruntVaisalaFreqSq)}},
                            Name, "VertMix: no array named ");
}
OMG_NAMED_ARRAYS(omg_vertmix_copy_to_host, omg_vertmix_copy_to_device, omg_vertmix_device_ptr, omg_vertmix, x,
                 vertMixLookup(*x->X, name))

// ---- VertMixStep (VertMixStep.h)
int omg_vertmix_step_create(const omg_mesh *m, omg_vertmix *x, omg_vcoord *v, omg_eos *e, int ntracers,
                            omg_vertmix_step **out) {
   OMG_TRY
   OMG_ARG(m && out);
   newHandle(out, [&](omg_vertmix_step &R) {
      R.M.reset(new VertMixStep("Default", m->M.get(), x ? x->X.get() : nullptr, v ? v->V.get() : nullptr,
                                e ? e->E.get() : nullptr, ntracers));
   });
   OMG_CATCH
}
int omg_vertmix_step_destroy(omg_vertmix_step *ms) {
   delete ms;
   return 0;
}
int omg_vertmix_step_set_boundary(omg_vertmix_step *ms, double bottom_drag_coeff, double rayleigh_drag_coeff,
                                  int use_wind_stress) {
   OMG_TRY
   OMG_ARG(ms);
   VertMixBoundary B;
   B.BottomDragCoeff = bottom_drag_coeff, B.RayleighDragCoeff = rayleigh_drag_coeff;
   VertMix::requireBoundary(B);
   ms->M->Boundary      = B;
   ms->M->UseWindStress = use_wind_stress != 0;
   OMG_CATCH
}
int omg_vertmix_step_apply(omg_vertmix_step *ms, const double *layer_thickness, double *normal_velocity, double *tracers,
                           double dt, void *stream) {
   OMG_TRY
   OMG_ARG(ms && layer_thickness && normal_velocity && tracers);
   const HorzMesh *M = ms->M->Mesh;
   const int K       = ms->M->NVertLayers;
   ms->M->apply(levelView(layer_thickness, M->NCellsSize, K), levelView(normal_velocity, M->NEdgesSize, K),
                tracerView(tracers, ms->M->NTracers, M->NCellsSize, K), dt, (hipStream_t)stream);
   OMG_CATCH
}
int omg_vertmix_step_apply_state(omg_vertmix_step *ms, const omg_state *s, int time_level, const omg_tracers *t,
                                 int tracer_time_level, double dt, void *stream) {
   OMG_TRY
   OMG_ARG(ms && s && t);
   ms->M->apply(s->S.get(), time_level, t->T.get(), tracer_time_level, dt, (hipStream_t)stream);
   OMG_CATCH
}
static ArrRef vertMixStepLookup(const VertMixStep &M, const char *Name) {
   return findNamed<ArrRef>({{"TangentialVelocity", arrRef(M.TangentialVelocity)},
                             {"NormalStressEdge", arrRef(M.NormalStressEdge)},
                             {"SurfaceTracerFlux", arrRef(M.SurfaceTracerFlux)},
                             {"SurfacePressure", arrRef(M.SurfacePressure)},
                             {"TidalPotential", arrRef(M.TidalPotential)},
                             {"SelfAttractionLoading", arrRef(M.SelfAttractionLoading)}},
                            Name, "VertMixStep: no array named ");
}
OMG_NAMED_ARRAYS(omg_vertmix_step_copy_to_host, omg_vertmix_step_copy_to_device, omg_vertmix_step_device_ptr,
                 omg_vertmix_step, ms, vertMixStepLookup(*ms->M, name))
int omg_stepper_attach_vert_mix(omg_stepper *st, omg_vertmix_step *ms) {
   OMG_TRY
   OMG_ARG(st);
   st->St->attachVertMix(ms ? ms->M.get() : nullptr);
   OMG_CATCH
}

// ---- PressureGrad (PressureGrad.h)
/// the column pass of a PressureGrad (Displaced = false), GentMcWilliams or Redi (true) on the caller's raw arrays
static void updateColumnOf(const ColumnPass &C, bool Displaced, const double *LayerThickness, const double *Tracers,
                           int NTracers, void *Stream) {
   const int N = C.Mesh->NCellsSize, K = C.NVertLayers;
   C.updateColumn(levelView(LayerThickness, N, K), tracerView(Tracers, NTracers, N, K), Displaced, (hipStream_t)Stream);
}
int omg_pgrad_create(const omg_mesh *m, omg_vcoord *v, omg_eos *e, omg_pgrad **out) {
   OMG_TRY
   OMG_ARG(m && out);
   newHandle(out, [&](omg_pgrad &R) {
      R.P.reset(new PressureGrad("Default", m->M.get(), v ? v->V.get() : nullptr, e ? e->E.get() : nullptr));
   });
   OMG_CATCH
}
int omg_pgrad_destroy(omg_pgrad *p) {
   delete p;
   return 0;
}
int omg_pgrad_update_column(omg_pgrad *p, const double *layer_thickness, const double *tracers, int ntracers,
                            void *stream) {
   OMG_TRY
   OMG_ARG(p && layer_thickness && tracers && ntracers >= 2);
   updateColumnOf(*p->P, false, layer_thickness, tracers, ntracers, stream);
   OMG_CATCH
}
int omg_pgrad_compute(omg_pgrad *p, double *tend, void *stream) {
   OMG_TRY
   OMG_ARG(p && tend);
   p->P->computePressureGrad(levelView(tend, p->P->Mesh->NEdgesSize, p->P->NVertLayers), (hipStream_t)stream);
   OMG_CATCH
}
int omg_pgrad_compute_arrays(omg_pgrad *p, double *tend, const double *pressure_mid, const double *geopotential_mid,
                             const double *spec_vol, void *stream) {
   OMG_TRY
   OMG_ARG(p && tend && pressure_mid && geopotential_mid && spec_vol);
   const HorzMesh *M = p->P->Mesh;
   const int K       = p->P->NVertLayers;
   p->P->computePressureGrad(levelView(tend, M->NEdgesSize, K), levelView(pressure_mid, M->NCellsSize, K),
                             levelView(geopotential_mid, M->NCellsSize, K), levelView(spec_vol, M->NCellsSize, K),
                             (hipStream_t)stream);
   OMG_CATCH
}
static ArrRef pgradLookup(const PressureGrad &P, const char *Name) {
   return findNamed<ArrRef>({{"SurfacePressure", arrRef(P.SurfacePressure)},
                             {"TidalPotential", arrRef(P.TidalPotential)},
                             {"SelfAttractionLoading", arrRef(P.SelfAttractionLoading)}},
                            Name, "PressureGrad: no array named ");
}
OMG_NAMED_ARRAYS(omg_pgrad_copy_to_host, omg_pgrad_copy_to_device, omg_pgrad_device_ptr, omg_pgrad, p,
                 pgradLookup(*p->P, name))
int omg_tend_attach_pressure_grad(omg_tend *t, omg_pgrad *p) {
   OMG_TRY
   OMG_ARG(t);
   t->T->attachPressureGrad(p ? p->P.get() : nullptr);
   OMG_CATCH
}

// ---- VertAdv (VertAdv.h)
int omg_vertadv_create(const omg_mesh *m, const omg_vcoord *v, int tracer_flux_order, omg_vertadv **out) {
   OMG_TRY
   OMG_ARG(m && out);
   VertAdvConfig Cfg;
   Cfg.TracerFluxOrder = tracer_flux_order;
   newHandle(out, [&](omg_vertadv &R) { R.A.reset(new VertAdv("Default", m->M.get(), v ? v->V.get() : nullptr, Cfg)); });
   OMG_CATCH
}
int omg_vertadv_destroy(omg_vertadv *a) {
   delete a;
   return 0;
}
int omg_vertadv_compute_transport(omg_vertadv *a, double *thickness_tend, int add_thickness, void *stream) {
   OMG_TRY
   OMG_ARG(a && thickness_tend);
   const Array2DReal T = levelView(thickness_tend, a->A->Mesh->NCellsSize, a->A->NVertLayers);
   if (add_thickness)
      a->A->computeAndAddThickness(T, (hipStream_t)stream);
   else
      a->A->computeVerticalTransport(T, (hipStream_t)stream);
   OMG_CATCH
}
int omg_vertadv_add_thickness(omg_vertadv *a, double *thickness_tend, void *stream) {
   OMG_TRY
   OMG_ARG(a && thickness_tend);
   a->A->addThicknessTend(levelView(thickness_tend, a->A->Mesh->NCellsSize, a->A->NVertLayers), (hipStream_t)stream);
   OMG_CATCH
}
int omg_vertadv_add_tracers(omg_vertadv *a, double *tracer_tend, const double *layer_thickness, const double *tracers,
                            int ntracers, void *stream) {
   OMG_TRY
   OMG_ARG(a && layer_thickness && ntracers >= 0 && ((tracer_tend && tracers) || ntracers == 0));
   const HorzMesh *M = a->A->Mesh;
   const int K       = a->A->NVertLayers;
   a->A->addTracerTend(tracerView(tracer_tend, ntracers, M->NCellsSize, K), levelView(layer_thickness, M->NCellsSize, K),
                       tracerView(tracers, ntracers, M->NCellsSize, K), ntracers, (hipStream_t)stream);
   OMG_CATCH
}
int omg_vertadv_add_velocity(omg_vertadv *a, double *velocity_tend, const double *layer_thickness,
                             const double *normal_velocity, void *stream) {
   OMG_TRY
   OMG_ARG(a && velocity_tend && layer_thickness && normal_velocity);
   const HorzMesh *M = a->A->Mesh;
   const int K       = a->A->NVertLayers;
   a->A->addVelocityTend(levelView(velocity_tend, M->NEdgesSize, K), levelView(layer_thickness, M->NCellsSize, K),
                         levelView(normal_velocity, M->NEdgesSize, K), (hipStream_t)stream);
   OMG_CATCH
}
int omg_vertadv_set_tracer_term(omg_vertadv *a, int on) {
   OMG_TRY
   OMG_ARG(a);
   a->A->TracerTermEnable = on != 0;
   OMG_CATCH
}
int omg_vertadv_max_layers(int *n) {
   OMG_TRY
   OMG_ARG(n);
   *n = VertAdv::maxLayers();
   OMG_CATCH
}
static ArrRef vertAdvLookup(const VertAdv &A, const char *Name) {
   return findNamed<ArrRef>({{"VerticalTransport", arrRef(A.VerticalTransport)}}, Name, "VertAdv: no array named ");
}
OMG_NAMED_ARRAYS(omg_vertadv_copy_to_host, omg_vertadv_copy_to_device, omg_vertadv_device_ptr, omg_vertadv, a,
                 vertAdvLookup(*a->A, name))
int omg_tend_attach_vert_adv(omg_tend *t, omg_vertadv *a) {
   OMG_TRY
   OMG_ARG(t);
   t->T->attachVertAdv(a ? a->A.get() : nullptr);
   OMG_CATCH
}

// ---- BarotropicMode (BarotropicMode.h)
int omg_btr_create(const omg_mesh *m, const omg_vcoord *v, double gravity, omg_btr **out) {
   OMG_TRY
   OMG_ARG(m && out);
   BarotropicConfig Cfg;
   Cfg.Gravity = gravity;
   newHandle(out, [&](omg_btr &R) { R.B.reset(new BarotropicMode("Default", m->M.get(), v ? v->V.get() : nullptr, Cfg)); });
   OMG_CATCH
}
int omg_btr_destroy(omg_btr *b) {
   delete b;
   return 0;
}
int omg_btr_max_layers(int *n) {
   OMG_TRY
   OMG_ARG(n);
   *n = BarotropicMode::maxLayers();
   OMG_CATCH
}
int omg_btr_split_velocity(omg_btr *b, const double *layer_thickness, const double *normal_velocity, int with_ssh,
                           void *stream) {
   OMG_TRY
   OMG_ARG(b && layer_thickness && normal_velocity);
   const HorzMesh *M = b->B->Mesh;
   const int K       = b->B->NVertLayers;
   const Array2DReal H = levelView(layer_thickness, M->NCellsSize, K), U = levelView(normal_velocity, M->NEdgesSize, K);
   if (with_ssh)
      b->B->splitVelocityAndSSH(H, U, (hipStream_t)stream);
   else
      b->B->splitVelocity(H, U, (hipStream_t)stream);
   OMG_CATCH
}
int omg_btr_compute_forcing(omg_btr *b, const double *layer_thickness, const double *velocity_tend, void *stream) {
   OMG_TRY
   OMG_ARG(b && layer_thickness && velocity_tend);
   const HorzMesh *M = b->B->Mesh;
   const int K       = b->B->NVertLayers;
   b->B->computeForcing(levelView(layer_thickness, M->NCellsSize, K), levelView(velocity_tend, M->NEdgesSize, K),
                        (hipStream_t)stream);
   OMG_CATCH
}
int omg_btr_compute_ssh(omg_btr *b, const double *layer_thickness, void *stream) {
   OMG_TRY
   OMG_ARG(b && layer_thickness);
   b->B->computeSSH(levelView(layer_thickness, b->B->Mesh->NCellsSize, b->B->NVertLayers), (hipStream_t)stream);
   OMG_CATCH
}
int omg_btr_recombine(omg_btr *b, double *normal_velocity, void *stream) {
   OMG_TRY
   OMG_ARG(b && normal_velocity);
   b->B->recombine(levelView(normal_velocity, b->B->Mesh->NEdgesSize, b->B->NVertLayers), (hipStream_t)stream);
   OMG_CATCH
}
int omg_btr_subcycle(omg_btr *b, int nsub, double dt_btr, void *stream) {
   OMG_TRY
   OMG_ARG(b);
   b->B->subcycle(nsub, dt_btr, (hipStream_t)stream);
   OMG_CATCH
}
int omg_btr_compute_residual_forcing(omg_btr *b, const double *layer_thickness, const double *velocity_tend, void *stream) {
   OMG_TRY
   OMG_ARG(b && layer_thickness && velocity_tend);
   const HorzMesh *M = b->B->Mesh;
   const int K       = b->B->NVertLayers;
   b->B->computeResidualForcing(levelView(layer_thickness, M->NCellsSize, K), levelView(velocity_tend, M->NEdgesSize, K),
                                (hipStream_t)stream);
   OMG_CATCH
}
int omg_btr_transport_velocity(omg_btr *b, const double *velocity_old, double *velocity_out, void *stream) {
   OMG_TRY
   OMG_ARG(b && velocity_old && velocity_out);
   const int NE = b->B->Mesh->NEdgesSize, K = b->B->NVertLayers;
   b->B->transportVelocity(levelView(velocity_old, NE, K), levelView(velocity_out, NE, K), (hipStream_t)stream);
   OMG_CATCH
}
int omg_btr_advance_velocity(omg_btr *b, const double *velocity_old, const double *velocity_tend, double dt,
                             double *velocity_out, void *stream) {
   OMG_TRY
   OMG_ARG(b && velocity_old && velocity_tend && velocity_out);
   const int NE = b->B->Mesh->NEdgesSize, K = b->B->NVertLayers;
   b->B->advanceVelocity(levelView(velocity_old, NE, K), levelView(velocity_tend, NE, K), dt, levelView(velocity_out, NE, K),
                         (hipStream_t)stream);
   OMG_CATCH
}
int omg_stepper_attach_barotropic(omg_stepper *st, omg_btr *b, int nsub) {
   OMG_TRY
   OMG_ARG(st);
   auto *Split = dynamic_cast<SplitExplicitStepper *>(st->St.get());
   OMEGA_REQUIRE(Split != nullptr, "TimeStepper: attachBarotropic: this stepper is not a Split-Explicit one");
   Split->attachBarotropic(b ? b->B.get() : nullptr, nsub);
   OMG_CATCH
}
int omg_stepper_set_fused_transport(omg_stepper *st, int on) {
   OMG_TRY
   OMG_ARG(st);
   auto *Split = dynamic_cast<SplitExplicitStepper *>(st->St.get());
   OMEGA_REQUIRE(Split != nullptr, "TimeStepper: setFusedTransport: this stepper is not a Split-Explicit one");
   Split->UseFusedTransport = on != 0;
   OMG_CATCH
}
/// the Split-Explicit stepper behind a handle, for the switches only it has
static SplitExplicitStepper *splitExplicit(omg_stepper *st, const char *What) {
   auto *Split = dynamic_cast<SplitExplicitStepper *>(st->St.get());
   OMEGA_REQUIRE(Split != nullptr, std::string("TimeStepper: ") + What + ": this stepper is not a Split-Explicit one");
   return Split;
}
int omg_stepper_set_momentum_rhs(omg_stepper *st, int on) {
   OMG_TRY
   OMG_ARG(st);
   splitExplicit(st, "setMomentumRHS")->UseMomentumRHS = on != 0;
   OMG_CATCH
}
int omg_stepper_set_folded_updates(omg_stepper *st, int on) {
   OMG_TRY
   OMG_ARG(st);
   splitExplicit(st, "setFoldedUpdates")->FoldUpdates = on != 0;
   OMG_CATCH
}
static ArrRef btrLookup(const BarotropicMode &B, const char *Name) {
   return findNamed<ArrRef>({{"BtrVelocity", arrRef(B.BtrVelocity)},
                             {"BtrThickEdge", arrRef(B.BtrThickEdge)},
                             {"BtrForcing", arrRef(B.BtrForcing)},
                             {"BtrFluxMean", arrRef(B.BtrFluxMean)},
                             {"BtrTendMean", arrRef(B.BtrTendMean)},
                             {"SSH", arrRef(B.SSH)},
                             {"BclVelocity", arrRef(B.BclVelocity)}},
                            Name, "BarotropicMode: no array named ");
}
OMG_NAMED_ARRAYS(omg_btr_copy_to_host, omg_btr_copy_to_device, omg_btr_device_ptr, omg_btr, b, btrLookup(*b->B, name))

// ---- MonotoneAdv (MonotoneAdv.h)
int omg_monoadv_create(const omg_mesh *m, int nvertlayers, int max_tracers, int flux_thickness_upwind, omg_monoadv **out) {
   OMG_TRY
   OMG_ARG(m && out);
   MonotoneAdvConfig Cfg;
   Cfg.FluxThicknessUpwind = flux_thickness_upwind != 0;
   newHandle(out, [&](omg_monoadv &R) { R.A.reset(new MonotoneAdv("Default", m->M.get(), nvertlayers, max_tracers, Cfg)); });
   OMG_CATCH
}
int omg_monoadv_destroy(omg_monoadv *a) {
   delete a;
   return 0;
}
int omg_monoadv_add_tracers(omg_monoadv *a, double *tracer_tend, const double *h_old, const double *h_new,
                            const double *normal_velocity, const double *tracers, int ntracers, double dt, void *stream) {
   OMG_TRY
   OMG_ARG(a && tracer_tend && h_old && h_new && normal_velocity && tracers);
   const HorzMesh *M = a->A->Mesh;
   const int K       = a->A->NVertLayers;
   const int NT      = ntracers > 0 ? ntracers : 0; // (the class refuses a count outside 1 .. MaxTracers)
   a->A->addTracerTend(tracerView(tracer_tend, NT, M->NCellsSize, K), levelView(h_old, M->NCellsSize, K),
                       levelView(h_new, M->NCellsSize, K), levelView(normal_velocity, M->NEdgesSize, K),
                       tracerView(tracers, NT, M->NCellsSize, K), ntracers, dt, (hipStream_t)stream);
   OMG_CATCH
}
int omg_monoadv_attach_vert_adv(omg_monoadv *a, omg_vertadv *v) {
   OMG_TRY
   OMG_ARG(a);
   a->A->attachVertAdv(v ? v->A.get() : nullptr);
   OMG_CATCH
}
static MonoHighOrderConfig monoHighCfg(int Order, double Coef3rd, double Radius, double XPeriod, double YPeriod) {
   MonoHighOrderConfig Cfg;
   Cfg.HorzOrder = Order, Cfg.Coef3rdOrder = Coef3rd, Cfg.SphereRadius = Radius;
   Cfg.XPeriod = XPeriod, Cfg.YPeriod = YPeriod;
   return Cfg;
}
int omg_monoadv_set_horz_order(omg_monoadv *a, int order, double coef3rd, double sphere_radius, double x_period,
                               double y_period) {
   OMG_TRY
   OMG_ARG(a);
   a->A->setHorzOrder(monoHighCfg(order, coef3rd, sphere_radius, x_period, y_period));
   OMG_CATCH
}
int omg_monoadv_high_order_tables(const omg_mesh *m, int order, double coef3rd, double sphere_radius, double x_period,
                                  double y_period, double *fit_cell, double *hess_weight, double *edge_dir_own,
                                  double *edge_dir_across) {
   OMG_TRY
   OMG_ARG(m && fit_cell && hess_weight && edge_dir_own && edge_dir_across);
   MonoHighOrderTables T;
   T.build(*m->M, monoHighCfg(order, coef3rd, sphere_radius, x_period, y_period));
   std::copy(T.Fit.V.begin(), T.Fit.V.end(), fit_cell);
   std::copy(T.Weight.V.begin(), T.Weight.V.end(), hess_weight);
   std::copy(T.Own.V.begin(), T.Own.V.end(), edge_dir_own);
   std::copy(T.Acr.V.begin(), T.Acr.V.end(), edge_dir_across);
   OMG_CATCH
}
int omg_monoadv_launch_count(const omg_monoadv *a, int64_t *n) {
   OMG_TRY
   OMG_ARG(a && n);
   *n = a->A->LaunchCount;
   OMG_CATCH
}
static ArrRef monoAdvLookup(const MonotoneAdv &A, const char *Name) {
   const ArrRef R = findNamed<ArrRef>({{"ScaleIn", arrRef(A.ScaleIn)},
                                       {"ScaleOut", arrRef(A.ScaleOut)},
                                       {"Hess", arrRef(A.Hess)},
                                       {"HessWeight", arrRef(A.HessWeight)},
                                       {"EdgeDirOwn", arrRef(A.EdgeDirOwn)},
                                       {"EdgeDirAcross", arrRef(A.EdgeDirAcross)},
                                       {"FitCell", arrRef(A.FitCell)}},
                                      Name, "MonotoneAdv: no array named ");
   OMEGA_REQUIRE(R.Ptr != nullptr, std::string("MonotoneAdv: ") + Name + " exists after setHorzOrder(3 or 4) only");
   return R;
}
OMG_NAMED_ARRAYS(omg_monoadv_copy_to_host, omg_monoadv_copy_to_device, omg_monoadv_device_ptr, omg_monoadv, a,
                 monoAdvLookup(*a->A, name))
int omg_stepper_attach_monotone_adv(omg_stepper *st, omg_monoadv *a) {
   OMG_TRY
   OMG_ARG(st);
   splitExplicit(st, "attachMonotoneAdv")->attachMonotoneAdv(a ? a->A.get() : nullptr);
   OMG_CATCH
}

// ---- GentMcWilliams (GentMcWilliams.h)
int omg_gm_create(const omg_mesh *m, omg_vcoord *v, omg_eos *e, double kappa, double grav_wave_speed, omg_gm **out) {
   OMG_TRY
   OMG_ARG(m && out);
   newHandle(out, [&](omg_gm &R) {
      R.G.reset(new GentMcWilliams("Default", m->M.get(), v ? v->V.get() : nullptr, e ? e->E.get() : nullptr, kappa,
                                   grav_wave_speed));
   });
   OMG_CATCH
}
int omg_gm_destroy(omg_gm *g) {
   delete g;
   return 0;
}
int omg_gm_update_column(omg_gm *g, const double *layer_thickness, const double *tracers, int ntracers, void *stream) {
   OMG_TRY
   OMG_ARG(g && layer_thickness && tracers && ntracers >= 2);
   updateColumnOf(*g->G, true, layer_thickness, tracers, ntracers, stream);
   OMG_CATCH
}
/// the optional transport of the two compute calls: NULL is the empty array (no term)
static Array2DReal gmTransport(const GentMcWilliams &G, double *Transport) {
   return Transport ? levelView(Transport, G.Mesh->NEdgesSize, G.NVertLayers) : Array2DReal();
}
int omg_gm_compute(omg_gm *g, const double *layer_thickness, double *transport, void *stream) {
   OMG_TRY
   OMG_ARG(g && layer_thickness);
   g->G->computeBolusVelocity(levelView(layer_thickness, g->G->Mesh->NCellsSize, g->G->NVertLayers),
                              gmTransport(*g->G, transport), (hipStream_t)stream);
   OMG_CATCH
}
int omg_gm_compute_arrays(omg_gm *g, const double *layer_thickness, const double *spec_vol,
                          const double *spec_vol_displaced, const double *z_mid, double *transport, void *stream) {
   OMG_TRY
   OMG_ARG(g && layer_thickness && spec_vol && spec_vol_displaced && z_mid);
   const int N = g->G->Mesh->NCellsSize, K = g->G->NVertLayers;
   g->G->computeBolusVelocity(levelView(layer_thickness, N, K), levelView(spec_vol, N, K),
                              levelView(spec_vol_displaced, N, K), levelView(z_mid, N, K), gmTransport(*g->G, transport),
                              (hipStream_t)stream);
   OMG_CATCH
}
static ArrRef gmLookup(const GentMcWilliams &G, const char *Name) {
   return findNamed<ArrRef>({{"Kappa", arrRef(G.Kappa)},
                             {"BolusVelocity", arrRef(G.BolusVelocity)},
                             {"StreamFunction", arrRef(G.StreamFunction)},
                             {"SurfacePressure", arrRef(G.SurfacePressure)},
                             {"TidalPotential", arrRef(G.TidalPotential)},
                             {"SelfAttractionLoading", arrRef(G.SelfAttractionLoading)}},
                            Name, "GentMcWilliams: no array named ");
}
OMG_NAMED_ARRAYS(omg_gm_copy_to_host, omg_gm_copy_to_device, omg_gm_device_ptr, omg_gm, g, gmLookup(*g->G, name))
int omg_stepper_attach_gm(omg_stepper *st, omg_gm *g) {
   OMG_TRY
   OMG_ARG(st);
   splitExplicit(st, "attachGentMcWilliams")->attachGentMcWilliams(g ? g->G.get() : nullptr);
   OMG_CATCH
}

// ---- Redi (Redi.h)
int omg_redi_create(const omg_mesh *m, omg_vcoord *v, omg_eos *e, int max_tracers, double kappa, double slope_max,
                    double n2_floor, omg_redi **out) {
   OMG_TRY
   OMG_ARG(m && out);
   newHandle(out, [&](omg_redi &H) {
      H.R.reset(new Redi("Default", m->M.get(), v ? v->V.get() : nullptr, e ? e->E.get() : nullptr, max_tracers, kappa,
                         slope_max, n2_floor));
   });
   OMG_CATCH
}
int omg_redi_destroy(omg_redi *r) {
   delete r;
   return 0;
}
int omg_redi_update_column(omg_redi *r, const double *layer_thickness, const double *tracers, int ntracers, void *stream) {
   OMG_TRY
   OMG_ARG(r && layer_thickness && tracers && ntracers >= 2);
   updateColumnOf(*r->R, true, layer_thickness, tracers, ntracers, stream);
   OMG_CATCH
}
int omg_redi_compute_slope(omg_redi *r, const double *layer_thickness, void *stream) {
   OMG_TRY
   OMG_ARG(r && layer_thickness);
   r->R->computeSlope(levelView(layer_thickness, r->R->Mesh->NCellsSize, r->R->NVertLayers), (hipStream_t)stream);
   OMG_CATCH
}
int omg_redi_compute_slope_arrays(omg_redi *r, const double *layer_thickness, const double *spec_vol,
                                  const double *spec_vol_displaced, const double *z_mid, void *stream) {
   OMG_TRY
   OMG_ARG(r && layer_thickness && spec_vol && spec_vol_displaced && z_mid);
   const int N = r->R->Mesh->NCellsSize, K = r->R->NVertLayers;
   r->R->computeSlope(levelView(layer_thickness, N, K), levelView(spec_vol, N, K), levelView(spec_vol_displaced, N, K),
                      levelView(z_mid, N, K), (hipStream_t)stream);
   OMG_CATCH
}
int omg_redi_add_tracer_tend(omg_redi *r, double *tracer_tend, const double *layer_thickness, const double *tracers,
                             int ntracers, const double *z_mid, void *stream) {
   OMG_TRY
   OMG_ARG(r && tracer_tend && layer_thickness && tracers);
   const int N = r->R->Mesh->NCellsSize, K = r->R->NVertLayers;
   const int NT = ntracers > 0 ? ntracers : 0; // (the class refuses the count; the views need an extent)
   if (z_mid)
      r->R->addTracerTend(tracerView(tracer_tend, NT, N, K), levelView(layer_thickness, N, K), tracerView(tracers, NT, N, K),
                          ntracers, levelView(z_mid, N, K), (hipStream_t)stream);
   else
      r->R->addTracerTend(tracerView(tracer_tend, NT, N, K), levelView(layer_thickness, N, K), tracerView(tracers, NT, N, K),
                          ntracers, (hipStream_t)stream);
   OMG_CATCH
}
int omg_redi_compute_vert_diffusivity(omg_redi *r, double *vert_diff, void *stream) {
   OMG_TRY
   OMG_ARG(r);
   r->R->computeVertDiffusivity(vert_diff ? levelView(vert_diff, r->R->Mesh->NCellsSize, r->R->NVertLayers) : Array2DReal(),
                                (hipStream_t)stream);
   OMG_CATCH
}
int omg_redi_launch_count(const omg_redi *r, int64_t *n) {
   OMG_TRY
   OMG_ARG(r && n);
   *n = r->R->LaunchCount;
   OMG_CATCH
}
static ArrRef rediLookup(const Redi &R, const char *Name) {
   return findNamed<ArrRef>({{"Kappa", arrRef(R.Kappa)},
                             {"SlopeInterface", arrRef(R.SlopeInterface)},
                             {"VertDiffusivity", arrRef(R.VertDiffusivity)},
                             {"SurfacePressure", arrRef(R.SurfacePressure)},
                             {"TidalPotential", arrRef(R.TidalPotential)},
                             {"SelfAttractionLoading", arrRef(R.SelfAttractionLoading)}},
                            Name, "Redi: no array named ");
}
OMG_NAMED_ARRAYS(omg_redi_copy_to_host, omg_redi_copy_to_device, omg_redi_device_ptr, omg_redi, r, rediLookup(*r->R, name))
int omg_stepper_attach_redi(omg_stepper *st, omg_redi *r) {
   OMG_TRY
   OMG_ARG(st);
   splitExplicit(st, "attachRedi")->attachRedi(r ? r->R.get() : nullptr);
   OMG_CATCH
}
int omg_vertmixstep_attach_redi(omg_vertmix_step *ms, omg_redi *r) {
   OMG_TRY
   OMG_ARG(ms);
   ms->M->attachRedi(r ? r->R.get() : nullptr);
   OMG_CATCH
}

// ---- VertRemap (VertRemap.h)
int omg_vremap_create(const omg_mesh *m, const omg_vcoord *v, int order, int max_tracers, omg_vremap **out) {
   OMG_TRY
   OMG_ARG(m && out);
   VertRemapConfig Cfg;
   Cfg.Order = order;
   newHandle(out, [&](omg_vremap &H) {
      H.R.reset(new VertRemap("Default", m->M.get(), v ? v->V.get() : nullptr, max_tracers, Cfg));
   });
   OMG_CATCH
}
int omg_vremap_destroy(omg_vremap *r) {
   delete r;
   return 0;
}
int omg_vremap_max_layers(int *n) {
   OMG_TRY
   OMG_ARG(n);
   *n = VertRemap::maxLayers();
   OMG_CATCH
}
int omg_vremap_compute_target(omg_vremap *r, const double *layer_thickness, void *stream) {
   OMG_TRY
   OMG_ARG(r && layer_thickness);
   r->R->computeTarget(levelView(layer_thickness, r->R->Mesh->NCellsSize, r->R->NVertLayers), (hipStream_t)stream);
   OMG_CATCH
}
int omg_vremap_remap_tracers(omg_vremap *r, const double *layer_thickness, double *tracers, int ntracers, void *stream) {
   OMG_TRY
   OMG_ARG(r && layer_thickness && (tracers || ntracers <= 0));
   const int N = r->R->Mesh->NCellsSize, K = r->R->NVertLayers;
   const int NT = ntracers > 0 ? ntracers : 0; // (the class refuses the count; the view needs an extent)
   r->R->remapTracers(levelView(layer_thickness, N, K), tracerView(tracers, NT, N, K), ntracers, (hipStream_t)stream);
   OMG_CATCH
}
int omg_vremap_remap_velocity(omg_vremap *r, const double *layer_thickness, double *normal_velocity, void *stream) {
   OMG_TRY
   OMG_ARG(r && layer_thickness && normal_velocity);
   const HorzMesh *M = r->R->Mesh;
   const int K       = r->R->NVertLayers;
   r->R->remapVelocity(levelView(layer_thickness, M->NCellsSize, K), levelView(normal_velocity, M->NEdgesSize, K),
                       (hipStream_t)stream);
   OMG_CATCH
}
int omg_vremap_adopt_target(omg_vremap *r, double *layer_thickness, void *stream) {
   OMG_TRY
   OMG_ARG(r && layer_thickness);
   r->R->adoptTarget(levelView(layer_thickness, r->R->Mesh->NCellsSize, r->R->NVertLayers), (hipStream_t)stream);
   OMG_CATCH
}
int omg_vremap_remap(omg_vremap *r, double *layer_thickness, double *normal_velocity, double *tracers, int ntracers,
                     void *stream) {
   OMG_TRY
   OMG_ARG(r && layer_thickness && normal_velocity && (tracers || ntracers <= 0));
   const HorzMesh *M = r->R->Mesh;
   const int K       = r->R->NVertLayers;
   const int NT      = ntracers > 0 ? ntracers : 0;
   r->R->remap(levelView(layer_thickness, M->NCellsSize, K), levelView(normal_velocity, M->NEdgesSize, K),
               tracerView(tracers, NT, M->NCellsSize, K), ntracers, (hipStream_t)stream);
   OMG_CATCH
}
int omg_vremap_launch_count(const omg_vremap *r, int64_t *n) {
   OMG_TRY
   OMG_ARG(r && n);
   *n = r->R->LaunchCount;
   OMG_CATCH
}
static ArrRef vremapLookup(const VertRemap &R, const char *Name) {
   return findNamed<ArrRef>({{"LayerThicknessTarget", arrRef(R.LayerThicknessTarget)}}, Name, "VertRemap: no array named ");
}
OMG_NAMED_ARRAYS(omg_vremap_copy_to_host, omg_vremap_copy_to_device, omg_vremap_device_ptr, omg_vremap, r,
                 vremapLookup(*r->R, name))
int omg_stepper_attach_vert_remap(omg_stepper *st, omg_vremap *r) {
   OMG_TRY
   OMG_ARG(st);
   splitExplicit(st, "attachVertRemap")->attachVertRemap(r ? r->R.get() : nullptr);
   OMG_CATCH
}

// ---- Kpp (Kpp.h)
int omg_kpp_config_default(omg_kpp_config *c) {
   OMG_TRY
   OMG_ARG(c);
   const KppConfig V;
   c->VonKarman            = V.VonKarman;
   c->CritBulkRichardson   = V.CritBulkRichardson;
   c->SurfaceLayerFraction = V.SurfaceLayerFraction;
   c->Cv                   = V.Cv;
   c->EntrainmentRatio     = V.EntrainmentRatio;
   c->CStar                = V.CStar;
   OMG_CATCH
}
int omg_kpp_create(const omg_mesh *m, const omg_vcoord *v, omg_vertmix *x, const omg_kpp_config *c, omg_kpp **out) {
   OMG_TRY
   OMG_ARG(m && out);
   KppConfig Cfg;
   if (c) {
      Cfg.VonKarman = c->VonKarman, Cfg.CritBulkRichardson = c->CritBulkRichardson;
      Cfg.SurfaceLayerFraction = c->SurfaceLayerFraction, Cfg.Cv = c->Cv;
      Cfg.EntrainmentRatio = c->EntrainmentRatio, Cfg.CStar = c->CStar;
   }
   newHandle(out, [&](omg_kpp &H) {
      H.K.reset(new Kpp("Default", m->M.get(), v ? v->V.get() : nullptr, x ? x->X.get() : nullptr, Cfg));
   });
   OMG_CATCH
}
int omg_kpp_destroy(omg_kpp *k) {
   delete k;
   return 0;
}
int omg_kpp_compute(omg_kpp *k, const double *normal_velocity, const double *tangential_velocity, void *stream) {
   OMG_TRY
   OMG_ARG(k && normal_velocity && tangential_velocity);
   const int NE = k->K->Mesh->NEdgesSize, K = k->K->NVertLayers;
   k->K->compute(levelView(normal_velocity, NE, K), levelView(tangential_velocity, NE, K), (hipStream_t)stream);
   OMG_CATCH
}
int omg_kpp_compute_arrays(omg_kpp *k, const double *normal_velocity, const double *tangential_velocity, const double *bvf,
                           const double *z_mid, const double *z_interface, double *vert_diff, double *vert_visc,
                           void *stream) {
   OMG_TRY
   OMG_ARG(k && normal_velocity && tangential_velocity && bvf && z_mid && z_interface && vert_diff && vert_visc);
   const int NE = k->K->Mesh->NEdgesSize, NC = k->K->Mesh->NCellsSize, K = k->K->NVertLayers;
   k->K->compute(levelView(normal_velocity, NE, K), levelView(tangential_velocity, NE, K), levelView(bvf, NC, K),
                 levelView(z_mid, NC, K), levelView(z_interface, NC, K + 1), levelView(vert_diff, NC, K),
                 levelView(vert_visc, NC, K), (hipStream_t)stream);
   OMG_CATCH
}
int omg_kpp_apply_non_local(omg_kpp *k, const double *layer_thickness, double *tracers, int ntracers, double dt,
                            const double *surface_flux, void *stream) {
   OMG_TRY
   OMG_ARG(k && layer_thickness && ntracers >= 0 && (tracers || ntracers == 0));
   const int NC = k->K->Mesh->NCellsSize, K = k->K->NVertLayers;
   k->K->applyNonLocalTracerFlux(levelView(layer_thickness, NC, K), tracerView(tracers, ntracers, NC, K), ntracers, dt,
                                 fluxView(surface_flux, ntracers, NC), (hipStream_t)stream);
   OMG_CATCH
}
int omg_kpp_constants(const omg_kpp *k, double *vt_coef, double *non_local_coeff) {
   OMG_TRY
   OMG_ARG(k && vt_coef && non_local_coeff);
   k->K->constants(*vt_coef, *non_local_coeff);
   OMG_CATCH
}
int omg_kpp_launch_count(const omg_kpp *k, int64_t *n) {
   OMG_TRY
   OMG_ARG(k && n);
   *n = k->K->LaunchCount;
   OMG_CATCH
}
static ArrRef kppLookup(const Kpp &P, const char *Name) {
   return findNamed<ArrRef>({{"FrictionVelocity", arrRef(P.FrictionVelocity)},
                             {"SurfaceBuoyancyFlux", arrRef(P.SurfaceBuoyancyFlux)},
                             {"BoundaryLayerDepth", arrRef(P.BoundaryLayerDepth)},
                             {"BulkRichardson", arrRef(P.BulkRichardson)},
                             {"NonLocalShape", arrRef(P.NonLocalShape)}},
                            Name, "Kpp: no array named ");
}
OMG_NAMED_ARRAYS(omg_kpp_copy_to_host, omg_kpp_copy_to_device, omg_kpp_device_ptr, omg_kpp, k, kppLookup(*k->K, name))
static const Array1DI4 &kppLookupI4(const Kpp &P, const char *Name) {
   return *findNamed<const Array1DI4 *>({{"BoundaryLayerIndex", &P.BoundaryLayerIndex}}, Name,
                                        "Kpp: no int array named ");
}
int omg_kpp_copy_to_host_i4(const omg_kpp *k, const char *name, int32_t *host, size_t n) {
   OMG_TRY
   OMG_ARG(k && name && host);
   const Array1DI4 &A = kppLookupI4(*k->K, name);
   if (n < A.size())
      OMEGA_ABORT(std::string("output buffer too small for ") + name);
   HIP_CHECK(hipDeviceSynchronize());
   copyToHost(host, A.Ptr, A.bytes());
   OMG_CATCH
}
int omg_kpp_copy_to_device_i4(omg_kpp *k, const char *name, const int32_t *host, size_t n) {
   OMG_TRY
   OMG_ARG(k && name && host);
   const Array1DI4 &A = kppLookupI4(*k->K, name);
   if (n != A.size())
      OMEGA_ABORT(std::string("size mismatch for ") + name);
   HIP_CHECK(hipDeviceSynchronize());
   copyToDevice(A.Ptr, host, A.bytes());
   HIP_CHECK(hipDeviceSynchronize());
   OMG_CATCH
}
int omg_vmix_step_attach_kpp(omg_vertmix_step *ms, omg_kpp *k) {
   OMG_TRY
   OMG_ARG(ms);
   ms->M->attachKpp(k ? k->K.get() : nullptr);
   OMG_CATCH
}

// ---- batched tridiagonal solvers (TriDiagSolvers.h)
/// a caller's [nbatch][nrow] device array of row pitch row_pitch (0: nrow) as the solvers' Array2DReal
static Array2DReal rowsView(const double *Dev, int NBatch, int NRow, int RowPitch) {
   Array2DReal A;
   A.Ptr    = const_cast<Real *>(Dev);
   A.Ext[0] = NBatch, A.Ext[1] = NRow;
   A.Pitch  = RowPitch == 0 ? NRow : RowPitch;
   return A;
}
int omg_tridiag_thomas_solve(const double *dl, const double *d, const double *du, double *x, int nbatch, int nrow,
                             int row_pitch, void *stream) {
   OMG_TRY
   OMG_ARG(row_pitch >= 0);
   ThomasSolver::solve(rowsView(dl, nbatch, nrow, row_pitch), rowsView(d, nbatch, nrow, row_pitch),
                       rowsView(du, nbatch, nrow, row_pitch), rowsView(x, nbatch, nrow, row_pitch),
                       (hipStream_t)stream);
   OMG_CATCH
}
int omg_tridiag_pcr_solve(const double *dl, const double *d, const double *du, double *x, int nbatch, int nrow,
                          int row_pitch, void *stream) {
   OMG_TRY
   OMG_ARG(row_pitch >= 0);
   PCRSolver::solve(rowsView(dl, nbatch, nrow, row_pitch), rowsView(d, nbatch, nrow, row_pitch),
                    rowsView(du, nbatch, nrow, row_pitch), rowsView(x, nbatch, nrow, row_pitch), (hipStream_t)stream);
   OMG_CATCH
}
int omg_tridiag_thomas_diff_solve(const double *g, const double *h, double *x, int nbatch, int nrow, int row_pitch,
                                  void *stream) {
   OMG_TRY
   OMG_ARG(row_pitch >= 0);
   ThomasDiffusionSolver::solve(rowsView(g, nbatch, nrow, row_pitch), rowsView(h, nbatch, nrow, row_pitch),
                                rowsView(x, nbatch, nrow, row_pitch), (hipStream_t)stream);
   OMG_CATCH
}
int omg_tridiag_pcr_diff_solve(const double *g, const double *h, double *x, int nbatch, int nrow, int row_pitch,
                               void *stream) {
   OMG_TRY
   OMG_ARG(row_pitch >= 0);
   PCRDiffusionSolver::solve(rowsView(g, nbatch, nrow, row_pitch), rowsView(h, nbatch, nrow, row_pitch),
                             rowsView(x, nbatch, nrow, row_pitch), (hipStream_t)stream);
   OMG_CATCH
}

} // extern "C"
