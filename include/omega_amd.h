/* omega_amd.h -- C ABI of libomega_amd.so, the MI355X-native compute backend for the
 * Omega ocean-dycore hot path (Tendencies + AuxiliaryState + TimeStepper + Halo).
 *
 * Omega has no FFI layer: its "operator API" for this path is a set of C++ classes
 * (O/ = components/omega/ in the reference tree).  Each entry point below names the
 * reference interface it replaces.  The same classes exist in C++ under omega_amd/csrc/
 * (namespace OMEGA, same class and method names) for a source-level drop-in; this C ABI
 * is the boundary a non-C++ host (or a test harness) binds.  See INTEGRATION.md.
 *
 * Conventions
 *  - every function returns 0 on success, non-zero on failure; omg_last_error() returns the
 *    message of the last failure on the calling thread (reference: int return codes of
 *    Halo/OceanState and the ABORT_ERROR macro, O/src/infra/Error.h:207-270);
 *  - arrays are LayoutRight doubles / int32, vertical index innermost, NXxSize = NXxAll+1
 *    rows with a zero sentinel row (O/src/base/DataTypes.h:58-94, O/src/base/Decomp.cpp:1082);
 *  - `stream` arguments are hipStream_t passed as void* (NULL = default stream); every
 *    compute call is asynchronous on that stream;
 *  - no function falls back to the CPU: without a HIP device every device call fails.
 */
#ifndef OMEGA_AMD_H
#define OMEGA_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct omg_decomp omg_decomp;   /* O/src/base/Decomp.h   class Decomp        */
typedef struct omg_halo omg_halo;       /* O/src/base/Halo.h     class Halo          */
typedef struct omg_mesh omg_mesh;       /* O/src/ocn/HorzMesh.h  class HorzMesh      */
typedef struct omg_state omg_state;     /* O/src/ocn/OceanState.h class OceanState   */
typedef struct omg_tracers omg_tracers; /* O/src/ocn/Tracers.h   class Tracers       */
typedef struct omg_aux omg_aux;         /* O/src/ocn/AuxiliaryState.h                */
typedef struct omg_tend omg_tend;       /* O/src/ocn/Tendencies.h                    */
typedef struct omg_stepper omg_stepper; /* O/src/timeStepping/TimeStepper.h          */
typedef struct omg_vcoord omg_vcoord;   /* O/src/ocn/VertCoord.h class VertCoord     */
typedef struct omg_eos omg_eos;         /* O/src/ocn/Eos.h       class Eos           */
typedef struct omg_vertmix omg_vertmix; /* O/doc/design/VerticalMixingCoeff.md (design only) */
typedef struct omg_pgrad omg_pgrad;     /* O/doc/design/OmegaV1GoverningEqns.md (design only) */
typedef struct omg_vertmix_step omg_vertmix_step; /* O/doc/design/OmegaV1GoverningEqns.md section 11 (design only) */
typedef struct omg_vertadv omg_vertadv; /* O/doc/design/OmegaV1GoverningEqns.md (design only) */
typedef struct omg_btr omg_btr;         /* O/doc/design/TimeStepping.md, OmegaV1GoverningEqns.md section 1 (design only) */
typedef struct omg_monoadv omg_monoadv; /* O/doc/design/Tracers.md, OmegaV0ShallowWater.md section 3.5.1 (design only) */

enum { OMG_ON_CELL = 0, OMG_ON_EDGE = 1, OMG_ON_VERTEX = 2 }; /* O/src/base/Halo.h:45 MeshElement */

const char *omg_last_error(void);

/* Row pitch of the library's own device arrays whose last index is the vertical level: every array the *_device_ptr
 * entry points return is [rows][omg_level_pitch(K)] doubles of which the first K per row are the levels (columns
 * of at least one 128-byte line are padded to whole lines: K = 60 -> 64; K a multiple of 16 or below 16: pitch = K).
 * Host arrays handed to / returned by the copy entry points and halo messages are always compact [rows][K].
 * Entry points that take RAW device arrays from the caller (omg_halo_exchange, omg_horz_*, omg_update_by_tend,
 * omg_local_weighted_sum_dd) have an explicit row_pitch argument (0 = compact). */
int omg_level_pitch(int nvertlayers);

/* ---- device / stream / event plumbing (Kokkos::initialize, Kokkos::fence, Pacer timers) ---- */
int omg_device_count(int *n);
int omg_device_init(int device_id);
int omg_device_synchronize(void);
int omg_stream_create(void **stream);
int omg_stream_destroy(void *stream);
int omg_stream_synchronize(void *stream);
int omg_event_create(void **event);
int omg_event_destroy(void *event);
int omg_event_record(void *event, void *stream);
int omg_event_elapsed_ms(void *start, void *stop, float *ms); /* synchronises on `stop` */

/* ---- global mesh as read from an MPAS mesh file (O/src/base/Decomp.cpp:108-395 readMesh,
 *      O/src/ocn/HorzMesh.cpp:424-523 read*).  Host pointers; indices 0-based, -1 = missing. ---- */
typedef struct omg_global_mesh {
   int32_t nCells, nEdges, nVertices, maxEdges, vertexDegree;
   const int32_t *cellsOnCell, *edgesOnCell, *verticesOnCell; /* [nCells][maxEdges]      */
   const int32_t *cellsOnEdge, *verticesOnEdge;               /* [nEdges][2]             */
   const int32_t *edgesOnEdge;                                /* [nEdges][2*maxEdges]    */
   const int32_t *cellsOnVertex, *edgesOnVertex;              /* [nVertices][vertexDegree] */
   const double *xCell, *yCell, *zCell, *lonCell, *latCell;
   const double *xEdge, *yEdge, *zEdge, *lonEdge, *latEdge;
   const double *xVertex, *yVertex, *zVertex, *lonVertex, *latVertex;
   const double *areaCell, *areaTriangle, *kiteAreasOnVertex; /* kite: [nVertices][vertexDegree] */
   const double *dcEdge, *dvEdge, *angleEdge, *weightsOnEdge; /* weights: [nEdges][2*maxEdges]   */
   const double *fCell, *fEdge, *fVertex, *bottomDepth;
} omg_global_mesh;

/* ---- raw device buffers for hosts without their own HIP runtime binding (Kokkos::View allocation / deep_copy) ---- */
/* number of device resources (buffers, streams, events) the library has created in this process: everything a time
 * step needs is created by the constructors / omg_stepper_create (O/src/timeStepping/RungeKutta4Stepper.cpp:43-64
 * allocates in finalizeInit), so the number does not move across omg_stepper_do_step calls */
int omg_device_resource_count(int64_t *n);
int omg_device_malloc(size_t bytes, void **ptr);
int omg_device_free(void *ptr);
int omg_copy_to_device(void *dst, const void *src, size_t bytes);
int omg_copy_to_host(void *dst, const void *src, size_t bytes);

/* ---- Reductions (O/src/base/Reductions.h:17-88 and the array forms :150-190, :262-310): sums in double-double.
 *      omg_local_sum_dd: sum a[i] (b == NULL) or sum a[i]*b[i] over n DEVICE values; omg_local_weighted_sum_dd:
 *      sum_r w[r] * sum_k a[r][k](*b[r][k]) over the first nrows rows of [rows][k] device arrays (w per row, e.g.
 *      AreaCell x layer thickness x tracer = tracer content).  hi_lo[0] + hi_lo[1] is the sum.
 *      omg_combine_dd: the reference's MPI_SUMDD operator applied in order to npairs (hi, lo) pairs -- how the
 *      per-rank partial sums are combined after an all-gather (globalSum). ---- */
int omg_local_sum_dd(const double *a, const double *b, size_t n, void *stream, double *hi_lo);
int omg_local_weighted_sum_dd(const double *w, const double *a, const double *b, int nrows, int k, int row_pitch,
                              void *stream, double *hi_lo); /* row_pitch of a and b in values, 0 = k */
int omg_combine_dd(const double *pairs, int npairs, double *hi_lo);

/* ---- MPAS mesh / initial-state file (O/src/base/Decomp.cpp:108-395 readMesh and O/src/ocn/HorzMesh.cpp:424-523
 *      read the same variables through SCORPIO): NetCDF classic CDF-1 / CDF-2 / CDF-5, both name conventions
 *      ("NCells" | "nCells", "CellsOnCell" | "cellsOnCell", ...), indices converted to 0-based / -1.
 *      omg_mesh_file_global_mesh fills `m` with pointers that stay valid until omg_mesh_file_close.
 *      omg_mesh_file_read_f64 reads any variable (e.g. layerThickness, normalVelocity, temperature of an initial
 *      state; record < 0 = all records) converted to double; omg_mesh_file_var_size = its element count
 *      (-1 if absent); omg_mesh_file_dim = a dimension length (-1 if absent). ---- */
typedef struct omg_mesh_file omg_mesh_file;
int omg_mesh_file_open(const char *path, omg_mesh_file **out);
int omg_mesh_file_close(omg_mesh_file *f);
int omg_mesh_file_global_mesh(const omg_mesh_file *f, omg_global_mesh *m);
int omg_mesh_file_dim(const omg_mesh_file *f, const char *name, int64_t *len);
int omg_mesh_file_var_size(const omg_mesh_file *f, const char *name, int64_t record, int64_t *n);
int omg_mesh_file_read_f64(const omg_mesh_file *f, const char *name, int64_t record, double *out, size_t n);

/* ---- Restart file (the RestartWrite / InitialState IOStreams of O/configs/Default.yml:91-127 go through SCORPIO;
 *      here one NetCDF CDF-5 file: layerThickness(nCells,nVertLevels), normalVelocity(nEdges,nVertLevels),
 *      tracers(nTracers,nCells,nVertLevels), simulationTime, stepsDone).  Rank 0 calls omg_restart_create; then
 *      every rank opens the file and writes / reads the rows of its own elements by 1-based global id (CellID /
 *      EdgeID of its Decomp) -- rows are [n][nVertLevels] host doubles; var = "layerThickness" | "normalVelocity" |
 *      "tracers" (plane = tracer index, else 0).  A restart may use a different partition. ---- */
typedef struct omg_restart_file omg_restart_file;
int omg_restart_create(const char *path, int64_t ncells_global, int64_t nedges_global, int nvertlevels, int ntracers,
                       double simulation_time, int64_t steps_done);
int omg_restart_open(const char *path, int write, omg_restart_file **out);
int omg_restart_close(omg_restart_file *f);
int omg_restart_info(const omg_restart_file *f, int64_t *ncells, int64_t *nedges, int *nvertlevels, int *ntracers,
                     double *simulation_time, int64_t *steps_done);
int omg_restart_write_rows(omg_restart_file *f, const char *var, int plane, const int32_t *global_id, int64_t n,
                           const double *rows);
int omg_restart_read_rows(const omg_restart_file *f, const char *var, int plane, const int32_t *global_id, int64_t n,
                          double *rows);

/* ---- History output (the "History" IOStream, O/configs/Default.yml:115-127: `Contents` lists fields and field groups;
 *      field names, long names and units as registered by the registerFields of O/src/ocn/auxiliaryVars/ (one .cpp per group) and
 *      O/src/ocn/OceanState.cpp:190-234).  contents: comma-separated field names ("SshCell", "KineticEnergyCell", ...)
 *      and groups ("State" = LayerThickness + NormalVelocity, "Tracers", "AuxiliaryState" = every auxiliary field).
 *      One CDF-5 file per dump (dimensions NCells / NEdges / NVertices / NVertLayers / NTracers); every rank writes
 *      the rows of its owned elements by global id.  create_file != 0 on exactly one rank (first, then a barrier of
 *      the caller's).  The whole AuxiliaryState is recomputed from the state / tracers at `time_level` before anything
 *      is copied (the fused RHS does not materialise most auxiliary arrays), on `stream`, which is synchronised. ---- */
int omg_history_write(const char *path, const omg_decomp *d, const omg_state *s, const omg_tracers *t, omg_aux *a,
                      const char *contents, double simulation_time, int time_level, int create_file, void *stream,
                      int *n_variables_written);

/* ---- Decomp (O/src/base/Decomp.cpp:444-745 constructor; Decomp.h:189-260 members).
 *      cell_task: optional [nCells] owner task of each cell (e.g. a METIS part file);
 *      NULL = built-in recursive coordinate bisection.  The global mesh arrays must stay
 *      alive until meshes / halos built from the decomp have been created. ---- */
int omg_decomp_create(const omg_global_mesh *mesh, int nparts, int mytask, int halo_width,
                      const int32_t *cell_task, omg_decomp **out);
/* local_order: 0 = the reference's numbering (owned cells in global-id order, every halo layer sorted by global id,
 * O/src/base/Decomp.cpp:1000-1080); 1 = every group ordered along a Morton curve through the cell centres, so that
 * consecutive local elements are spatial neighbours whatever order the mesh file uses; 2 = the same along a Hilbert
 * curve; 3 = k-d order: every group bisected recursively at the median of its widest axis, so that aligned runs of 8 /
 * 16 / 32 local cells -- the kernels' tiles -- are compact patches on the surface the cells live on (spheres: a tile
 * touches 35 distinct cell rows instead of 42 with the 3-D curves).  Edges / vertices follow the cells in every case.
 * Per global id the results of every computation are identical. */
int omg_decomp_create_ordered(const omg_global_mesh *mesh, int nparts, int mytask, int halo_width,
                              const int32_t *cell_task, int local_order, omg_decomp **out);
/* Built-in partitioners of the cell graph (the reference calls METIS_PartGraphKway, O/src/base/Decomp.cpp:868-1000):
 * method "rcb" = recursive coordinate bisection of the cell centres (what omg_decomp_create uses when cell_task is
 * NULL), "graph" = recursive graph bisection with Fiduccia-Mattheyses refinement + greedy k-way refinement on
 * CellsOnCell (no coordinates needed; minimises the edge cut = halo size within a 3 % imbalance tolerance).
 * cell_task_out[nCells] receives the owner task of every cell -- hand it to omg_decomp_create* as cell_task.
 * edge_cut (optional): number of cell-graph edges between different parts. */
int omg_partition_cells(const omg_global_mesh *mesh, int nparts, const char *method, int32_t *cell_task_out,
                        int64_t *edge_cut);
int omg_decomp_destroy(omg_decomp *d);
/* scalar members by reference name: "NCellsOwned", "NCellsAll", "NCellsSize", "NCellsGlobal",
 * "NEdges...", "NVertices...", "MaxEdges", "VertexDegree", "HaloWidth" */
int omg_decomp_get_int(const omg_decomp *d, const char *name, int32_t *out);
/* array members: "CellID" "EdgeID" "VertexID" (1-based global ids, [NXxSize]), "CellLoc"
 * "EdgeLoc" "VertexLoc" ([NXxSize][2]), "NCellsHalo" "NEdgesHalo" "NVerticesHalo"
 * ([HaloWidth]), "CellTask" ([NCellsGlobal]); n = capacity of out in elements */
int omg_decomp_get_array(const omg_decomp *d, const char *name, int32_t *out, size_t n);

/* ---- Halo (O/src/base/Halo.cpp:150-201 constructor, :455-600 exchange lists;
 *      Halo.h:767-915 exchangeFullArrayHalo) ---- */
typedef int (*omg_transport_fn)(void *ctx, int n_neighbors, const int *tasks, void *const *send_ptrs,
                                const size_t *send_bytes, void *const *recv_ptrs, const size_t *recv_bytes,
                                void *stream);
int omg_halo_create(const omg_decomp *d, omg_halo **out);
int omg_halo_destroy(omg_halo *h);
int omg_halo_num_neighbors(const omg_halo *h, int *n);
int omg_halo_neighbor_task(const omg_halo *h, int i, int *task);
int omg_halo_list_size(const omg_halo *h, int i, int elem, int recv, int *n);
int omg_halo_get_list(const omg_halo *h, int i, int elem, int recv, int32_t *out);
int omg_halo_required_bytes(const omg_halo *h, int i, size_t per_cell, size_t per_edge, size_t per_vertex,
                            size_t *bytes);
/* a caller-supplied wire (test rigs: messages staged through the host over gloo / MPI).  The pointers handed to
 * fn are slices of the Halo's own contiguous send / receive buffers in device memory. */
int omg_halo_set_transport(omg_halo *h, omg_transport_fn fn, void *ctx);
/* The production wire: RCCL send / recv over xGMI issued inside the library on the exchange's HIP stream
 * (ncclGroupStart, ncclRecv + ncclSend per neighbour, ncclGroupEnd) -- what the MPI_Irecv / MPI_Isend / MPI_Test
 * sequence of O/src/base/Halo.h:851-907, Halo.cpp:607-757 becomes.  One process per GPU, device selected with
 * omg_device_init first.  Rank 0 calls omg_rccl_get_unique_id and distributes the OMG_RCCL_ID_BYTES bytes by any side
 * channel; omg_rccl_create is collective over all nranks processes (ncclCommInitRank). */
enum { OMG_RCCL_ID_BYTES = 128 };
typedef struct omg_rccl omg_rccl;
int omg_rccl_get_unique_id(char *id /* [OMG_RCCL_ID_BYTES] */);
int omg_rccl_create(const char *id, int nranks, int rank, omg_rccl **out);
int omg_rccl_destroy(omg_rccl *c);
/* ncclCommAbort: give up a communicator (after an error, or when another rank could not create its own); every
 * later exchange on it fails.  An error inside an exchange aborts the communicator by itself. */
int omg_rccl_abort(omg_rccl *c);
/* what RCCL itself reports: communicator size, this rank, library version code, grouped exchanges issued so far */
int omg_rccl_info(const omg_rccl *c, int *nranks, int *rank, int *version, int64_t *exchanges);
/* one grouped exchange on raw device buffers (same argument meaning as omg_transport_fn) */
int omg_rccl_exchange(omg_rccl *c, int n, const int *peers, void *const *send_ptrs, const size_t *send_bytes,
                      void *const *recv_ptrs, const size_t *recv_bytes, void *stream);
/* route this Halo's exchanges through the communicator (which must outlive the Halo's exchanges) */
int omg_halo_use_rccl(omg_halo *h, omg_rccl *c);
/* The second stream-ordered wire: direct peer copies between the GPUs of the node (PeerWire.h).  Every rank owns a
 * mailbox (its receive buffer) and a block of flags in device memory, exported once with hipIpcGetMemHandle; an exchange
 * is pack kernel -> hipMemcpyAsync device-to-device into each neighbour's mailbox -> flag kernels (release store into
 * the peer's flags, bounded acquire wait on the local ones) -> unpack kernel, all on the exchange's stream: what the
 * MPI_Irecv / MPI_Isend / MPI_Test loop of O/src/base/Halo.h:851-907 becomes without any host wait.
 * omg_peer_create after omg_device_init; distribute the OMG_PEER_HANDLE_BYTES of omg_peer_local_handle to all ranks
 * by any side channel, pass all of them in rank order to omg_peer_connect, then omg_halo_use_peer.
 * mailbox_bytes >= omg_halo_recv_rows(...) * k * 8 of the largest exchange. */
enum { OMG_PEER_HANDLE_BYTES = 160 };
typedef struct omg_peer omg_peer;
int omg_peer_create(int nranks, int rank, size_t mailbox_bytes, omg_peer **out);
int omg_peer_destroy(omg_peer *p);
int omg_peer_local_handle(const omg_peer *p, char *out /* [OMG_PEER_HANDLE_BYTES] */);
int omg_peer_connect(omg_peer *p, const char *all_handles /* [nranks][OMG_PEER_HANDLE_BYTES] */);
/* exchanges issued so far; sticky status (0 = fine, else a wait on a peer gave up: 1 = my previous message was never
 * consumed, 2 = a neighbour's message never arrived, 4 = an all-gather of omg_halo_global_sum_dd never got a rank's
 * values; bits may combine); wait bound in seconds.
 * Lifetime: the wire and the Halo it serves (omg_halo_use_peer) may be destroyed in either order -- each releases the
 * other; a Halo whose wire has been destroyed has no wire (its next multi-rank exchange returns an error). */
int omg_peer_info(const omg_peer *p, int64_t *exchanges, int *status);
int omg_peer_set_timeout(omg_peer *p, double seconds);
int omg_halo_use_peer(omg_halo *h, omg_peer *p);
/* rows of k values this rank receives in one exchange of per_cell / per_edge / per_vertex arrays per element */
int omg_halo_recv_rows(const omg_halo *h, size_t per_cell, size_t per_edge, size_t per_vertex, size_t *rows);
/* Halo::exchangeFullArrayHalo on a raw device array [nt][rows_size][row_pitch] (nt = 1 for 2-D) of which the first
 * k values of every row are exchanged (row_pitch 0 = compact rows of k) */
int omg_halo_exchange(omg_halo *h, double *dev_array, int nt, int rows_size, int k, int row_pitch, int elem,
                      void *stream);
/* the same for the reference's other array types (O/src/base/Halo.h:304-351 rank 1, :324-760 I4 / I8 / R4 / R8, ranks
 * 1-5): values of elem_bytes bytes (4 or 8).  Rank 1: nt = 1, k = 1, row_pitch = 1; ranks 4 and 5: nt = the product of
 * the leading extents (the element index is the second-to-last, Halo.h:418-470).  omg_halo_exchange_i4 = elem_bytes 4. */
int omg_halo_exchange_bytes(omg_halo *h, void *dev_array, int elem_bytes, int nt, int rows_size, int k, int row_pitch,
                            int elem, void *stream);
int omg_halo_exchange_i4(omg_halo *h, int32_t *dev_array, int nt, int rows_size, int k, int row_pitch, int elem,
                         void *stream);
/* globalSum (O/src/base/Reductions.h:71-88 scalar, :150-190 array forms: MPI_Allreduce with the double-double operator
 * MPI_SUMDD) for npairs (<= 64) local partial sums at once: local_hi_lo[npairs][2] (from omg_local_sum_dd /
 * omg_local_weighted_sum_dd) is all-gathered over the Halo's wire -- ncclAllGather on the RCCL communicator, or the
 * peer wire's gather slots -- and combined in rank order with omg_combine_dd: hi_lo[npairs][2], the same bits on every
 * rank and for every partition.  Collective over all tasks of the decomposition; synchronises `stream`.  One task: the
 * combination alone.  Fails on a Halo whose wire is a caller-supplied transport. */
int omg_halo_global_sum_dd(omg_halo *h, const double *local_hi_lo, int npairs, double *hi_lo, void *stream);
/* h, u and the tracers of one exchange point as ONE message per neighbour: what the time steppers do after a stage
 * (RungeKutta4Stepper.cpp:95-101 calls OceanState::exchangeHalo and Tracers::exchangeHalo -- three rounds of messages;
 * here [h on cells][u on edges][tracers on cells] travel together).  `tracers` may be NULL.  Queued on `stream`. */
int omg_halo_exchange_state(omg_halo *h, omg_state *state, int state_time_level, omg_tracers *tracers,
                            int tracers_time_level, void *stream);
/* The wire's verdict, to be asked after the host has synchronised with an exchange's stream (the exchange calls return
 * when the work is queued): 0 = fine; fails (message: omg_last_error) when a peer-wire wait gave up -- the unpack
 * kernel of that exchange then copied nothing, the halo is stale.  The time steppers ask at the start of every step. */
int omg_halo_check(const omg_halo *h);

/* ---- Test options (omega_amd/csrc/Tuning.h).  The library never reads the environment.  Defaults are what production
 *      runs; every option forces a kernel / table structure that some mesh class reaches by itself (named in Tuning.h), so
 *      that tests can drive generated meshes through it -- no option can make a result wrong, and there is no measurement
 *      probe in the library.  Names: MergeL1 Pair TracerPatch (structure of the fused RHS; read at every launch); SendBand
 *      BandOnComm ShrinkSweeps (what a rank leaves out inside an RK4 step; read at every stage); ForceGeneric KeepMaxEdges
 *      NarrowTables (mesh tables; read when a HorzMesh is created); Graphs (-1 per object, 0 never, 1 default on).
 *      Unknown names fail.
 *      omg_set_timing_level: roctx ranges named after the reference's Pacer timers ("Tend:...", "AuxState:...",
 *      "RK4:haloExch"; share/pacer/Pacer.cpp:138-200) are emitted for timers up to this level (default 3 = all). ---- */
int omg_set_option(const char *name, int value);
int omg_get_option(const char *name, int *value);
int omg_set_timing_level(int level);

/* ---- HorzMesh (O/src/ocn/HorzMesh.cpp:44-140 constructor; HorzMesh.h:100-265 members).
 *      host_only != 0 builds the host arrays only (no device mirrors; compute calls fail). ---- */
int omg_mesh_create(const omg_decomp *d, int nvertlayers, int host_only, omg_mesh **out);
int omg_mesh_destroy(omg_mesh *m);
int omg_mesh_get_int(const omg_mesh *m, const char *name, int32_t *out);
int omg_mesh_get_array_i4(const omg_mesh *m, const char *name, int32_t *out, size_t n);
int omg_mesh_get_array_r8(const omg_mesh *m, const char *name, double *out, size_t n);
int omg_mesh_set_fvertex(omg_mesh *m, const double *host_values /* [NVerticesSize] */);

/* ---- HorzOperators (O/src/ocn/HorzOperators.h:9-187; constructors HorzOperators.cpp:7-28): the reference's
 *      reusable operators as sweeps over elements [0, n) (n < 0: all local elements) x nvertlayers levels of raw
 *      device arrays [NXxSize][row_pitch] (row_pitch 0 = compact rows of nvertlayers; input and output share it):
 *        divergence        DivCell(i,k)   = -sum_j DvEdge*EdgeSignOnCell(i,j)*VecEdge(e_j,k)/AreaCell(i)        :13-33
 *        gradient          GradEdge(e,k)  = (Scalar(c1,k) - Scalar(c0,k))/DcEdge(e)                             :47-60
 *        curl              CurlVertex(v,k)= sum_j DcEdge*EdgeSignOnVertex(v,j)*VecEdge(e_j,k)/AreaTriangle(v)   :71-93
 *        tangential_recon  ReconEdge(e,k) = sum_j WeightsOnEdge(e,j)*VecEdge(EdgesOnEdge(e,j),k)                :107-126
 *        interp_cell_to_edge (1-D arrays) isotropic != 0: kite-area weighted over the cells of the edge's two
 *                          vertices (:161-180), else the mean of its two cells (:153-159) ---- */
int omg_horz_divergence(const omg_mesh *m, const double *vec_edge_dev, double *div_cell_dev, int nvertlayers,
                        int row_pitch, int n, void *stream);
int omg_horz_gradient(const omg_mesh *m, const double *scalar_cell_dev, double *grad_edge_dev, int nvertlayers,
                      int row_pitch, int n, void *stream);
int omg_horz_curl(const omg_mesh *m, const double *vec_edge_dev, double *curl_vertex_dev, int nvertlayers,
                  int row_pitch, int n, void *stream);
int omg_horz_tangential_recon(const omg_mesh *m, const double *vec_edge_dev, double *recon_edge_dev, int nvertlayers,
                              int row_pitch, int n, void *stream);
int omg_horz_interp_cell_to_edge(const omg_mesh *m, const double *array_cell_dev, double *array_edge_dev,
                                 int isotropic, int n, void *stream);

/* ---- options (O/configs/Default.yml:25-52; Tendencies::readTendConfig O/src/ocn/Tendencies.cpp:123-213;
 *      AuxiliaryState::readConfigOptions O/src/ocn/AuxiliaryState.cpp:259-308) ---- */
typedef struct omg_tend_config {
   int32_t ThicknessFluxTendencyEnable, PVTendencyEnable, KETendencyEnable, SSHTendencyEnable,
       VelDiffTendencyEnable, VelHyperDiffTendencyEnable, WindForcingTendencyEnable, BottomDragTendencyEnable,
       TracerHorzAdvTendencyEnable, TracerDiffTendencyEnable, TracerHyperDiffTendencyEnable;
   int32_t FluxThicknessUpwind, FluxTracerUpwind, WindInterpIsotropic;
   double ViscDel2, ViscDel4, DivFactor, EddyDiff2, EddyDiff4, Density0, BottomDragCoeff;
} omg_tend_config;
void omg_tend_config_default(omg_tend_config *c);

/* ---- OceanState (O/src/ocn/OceanState.h:100-149; OceanState.cpp:247-407).  time_level:
 *      1 = new, 0 = current, -1 = previous.  halo may be NULL on a single rank. ---- */
int omg_state_create(const omg_mesh *m, omg_halo *halo, int nvertlayers, int ntimelevels, omg_state **out);
int omg_state_destroy(omg_state *s);
int omg_state_copy_to_device(omg_state *s, int time_level, const double *h_host, const double *u_host);
int omg_state_copy_to_host(const omg_state *s, int time_level, double *h_host, double *u_host);
int omg_state_device_ptr(const omg_state *s, int time_level, int which /*0 h, 1 u*/, double **dev);
int omg_state_exchange_halo(omg_state *s, int time_level, void *stream);
int omg_state_update_time_levels(omg_state *s, void *stream);

/* ---- Tracers (O/src/ocn/Tracers.cpp:269 getAll, :457-496 exchangeHalo/updateTimeLevels) ---- */
int omg_tracers_create(const omg_mesh *m, omg_halo *halo, int nvertlayers, int ntracers, int ntimelevels,
                       omg_tracers **out);
int omg_tracers_destroy(omg_tracers *t);
int omg_tracers_copy_to_device(omg_tracers *t, int time_level, const double *host);
int omg_tracers_copy_to_host(const omg_tracers *t, int time_level, double *host);
int omg_tracers_device_ptr(const omg_tracers *t, int time_level, double **dev);
int omg_tracers_exchange_halo(omg_tracers *t, int time_level, void *stream);
int omg_tracers_update_time_levels(omg_tracers *t, void *stream);

/* ---- AuxiliaryState (O/src/ocn/AuxiliaryState.h:49-82; AuxiliaryState.cpp:60-191) ---- */
int omg_aux_create(const omg_mesh *m, omg_halo *halo, int nvertlayers, int ntracers, omg_aux **out);
int omg_aux_destroy(omg_aux *a);
int omg_aux_set_options(omg_aux *a, int flux_thickness_upwind, int flux_tracer_upwind, int wind_interp_isotropic);
int omg_aux_compute_mom_aux(omg_aux *a, const omg_state *s, int thick_time_level, int vel_time_level, void *stream);
int omg_aux_compute_all(omg_aux *a, const omg_state *s, const omg_tracers *t, int tracer_time_level,
                        int thick_time_level, int vel_time_level, void *stream);
/* array by reference member name ("KineticEnergyCell", "VelocityDivCell", "FluxLayerThickEdge",
 * "MeanLayerThickEdge", "SshCell", "RelVortVertex", "NormRelVortVertex", "NormPlanetVortVertex",
 * "NormRelVortEdge", "NormPlanetVortEdge", "Del2Edge", "Del2DivCell", "Del2RelVortVertex",
 * "HTracersEdge", "Del2TracersCell", "NormalStressEdge", "ZonalStressCell", "MeridStressCell") */
int omg_aux_copy_to_host(const omg_aux *a, const char *name, double *host, size_t n);
int omg_aux_copy_to_device(omg_aux *a, const char *name, const double *host, size_t n);
int omg_aux_device_ptr(const omg_aux *a, const char *name, double **dev, size_t *n);

/* ---- Tendencies (O/src/ocn/Tendencies.h:73-102; Tendencies.cpp:257-600) ---- */
/* omg_tend_create FAILS (message: omg_last_error, naming the limit) for a mesh outside the fused RHS: an array plane of
 * 4 GiB or more (32-bit buffer offsets: ~ 2.2 M cells x 80 levels per rank -- several ranks may share a GPU) or MaxEdges
 * outside 5..8.  omg_tend_create_reference_structured accepts such a mesh: computeAllTendencies then takes the
 * reference-structured 23-launch path (~ 5 x the time) -- the caller's decision, not a surprise.
 * omg_tend_fused_limit asks beforehand, on sizes alone (rows incl. the sentinel; no mesh, no device): *supported = 1, or 0
 * with the reason in `why`. */
int omg_tend_create(const omg_mesh *m, int nvertlayers, int ntracers, const omg_tend_config *c, omg_tend **out);
int omg_tend_create_reference_structured(const omg_mesh *m, int nvertlayers, int ntracers, const omg_tend_config *c,
                                         omg_tend **out);
int omg_tend_fused_limit(int64_t ncells_size, int64_t nedges_size, int64_t nvertices_size, int max_edges, int nvertlayers,
                         int *supported, char *why, size_t why_bytes);
int omg_tend_destroy(omg_tend *t);
int omg_tend_set_fused(omg_tend *t, int use_fused_rhs);
/* HIP-graph replay of launch-bound sequences (default off: measured without gain on MI355X; OMEGA_GRAPHS=1 or these
 * switches turn it on): the fused RHS (omg_tend_compute_all) and, on one rank, the
 * stage-fused RK4 step (omg_stepper_do_step; option "UseGraphs") are captured the second time they are called with
 * the same arrays on the same NON-default stream and replayed afterwards with one host call.  Kernel timing and
 * custom tendencies switch it off.  *_graph_stats: graphs captured / replays so far. */
int omg_tend_set_graphs(omg_tend *t, int use_graphs);
int omg_tend_graph_stats(const omg_tend *t, int64_t *captures, int64_t *replays);
int omg_stepper_graph_stats(const omg_stepper *st, int64_t *captures, int64_t *replays);
int omg_tend_compute_all(omg_tend *t, const omg_state *s, omg_aux *a, const omg_tracers *tr, int tracer_time_level,
                         int thick_time_level, int vel_time_level, void *stream);
int omg_tend_compute_thickness(omg_tend *t, const omg_state *s, omg_aux *a, int thick_time_level,
                               int vel_time_level, void *stream);
int omg_tend_compute_velocity(omg_tend *t, const omg_state *s, omg_aux *a, int thick_time_level, int vel_time_level,
                              void *stream);
int omg_tend_compute_tracer(omg_tend *t, const omg_state *s, omg_aux *a, const omg_tracers *tr,
                            int tracer_time_level, int thick_time_level, int vel_time_level, void *stream);
/* Tendencies::computeTransportTendencies (omega_amd/csrc/Tendencies.h): the transport half of the RHS in two launches.
 * LayerThicknessTend and TracerTend end up, bit for bit on every row < NCellsAll, as omg_tend_compute_thickness followed
 * by omg_tend_compute_tracer with the same arguments leave them (attached VertAdv terms included); the edge-located
 * auxiliary arrays FluxLayerThickEdge, MeanLayerThickEdge and HTracersEdge are not written, Del2TracersCell only with
 * TracerHyperDiffTendencyEnable.  With a custom thickness tendency installed the two group calls run instead.  Fails
 * for a NULL handle and for a time level out of range. */
int omg_tend_compute_transport(omg_tend *t, const omg_state *s, omg_aux *a, const omg_tracers *tr,
                               int tracer_time_level, int thick_time_level, int vel_time_level, void *stream);
/* Tendencies::computeTransportTendenciesAndUpdate: omg_tend_compute_transport with the two updates that follow it in a
 * step folded into its kernels.  On every row < NCellsAll and level < NVertLayers the thickness of
 * next_thick_time_level and the tracers of next_tracer_time_level hold, bit for bit, what omg_tend_compute_transport
 * followed by next_h = h + coeff*LayerThicknessTend (omg_update_by_tend) and
 * next_tracers = (tracers*h + coeff*TracerTend)/next_h (omg_update_tracers_by_tend) leave there; their level padding is not written.  With
 * keep_tendencies the two tendency arrays hold what omg_tend_compute_transport leaves, without it their contents on
 * those rows are unspecified.  With a VertAdv attached, a custom thickness tendency installed, or an output level equal
 * to its input level the sequence itself runs.  Fails for a NULL handle and for a time level out of range. */
int omg_tend_compute_transport_update(omg_tend *t, omg_state *s, omg_aux *a, omg_tracers *tr, int tracer_time_level,
                                      int thick_time_level, int vel_time_level, int next_thick_time_level,
                                      int next_tracer_time_level, double coeff, int keep_tendencies, void *stream);
/* Tendencies::computeMomentumTendencies: the fused RHS without its tracer half.  NormalVelocityTend (rows < NEdgesAll)
 * and LayerThicknessTend (rows < NCellsAll) end up, bit for bit, as omg_tend_compute_all with the same arguments leaves
 * them, attached PressureGrad / VertAdv terms included; TracerTend and Del2TracersCell are not written.  With a custom
 * tendency installed, or off the fused RHS, omg_tend_compute_all itself runs (TracerTend is then written too).  Fails
 * for a NULL handle and for a time level out of range. */
int omg_tend_compute_momentum(omg_tend *t, const omg_state *s, omg_aux *a, const omg_tracers *tr, int tracer_time_level,
                              int thick_time_level, int vel_time_level, void *stream);
int omg_tend_compute_thickness_only(omg_tend *t, const omg_state *s, omg_aux *a, int thick_time_level,
                                    int vel_time_level, void *stream);
int omg_tend_compute_velocity_only(omg_tend *t, const omg_state *s, omg_aux *a, int thick_time_level,
                                   int vel_time_level, void *stream);
int omg_tend_compute_tracer_only(omg_tend *t, const omg_state *s, omg_aux *a, const omg_tracers *tr,
                                 int tracer_time_level, int thick_time_level, int vel_time_level, void *stream);
/* per-kernel timing of the fused RHS with HIP events on the launch stream (Pacer "Tend:*" timers,
 * O/src/ocn/Tendencies.cpp:280-481).  names[i] / ms_sum[i] for i < *n_kernels (<= 8). */
/* Custom tendencies (O/src/ocn/Tendencies.h:51-53; Tendencies.cpp:41-64 UseCustomTendency +
 * ManufacturedSolutionTendency): attach the manufactured-solution source terms of
 * O/src/ocn/CustomTendencyTerms.cpp:18-208 (wavelengths / amplitude = the ManufacturedSolution config group,
 * Default.yml:143-146; H0 = BottomDepth of the first cell; del2 / del4 switches and viscosities from this
 * Tendencies' options).  omg_tend_set_time = the TimeInstant argument of the compute* calls, in seconds
 * since the reference time (the time steppers set it per stage). */
int omg_tend_use_manufactured_solution(omg_tend *t, const omg_mesh *m, double wavelength_x, double wavelength_y,
                                       double amplitude);
/* Custom tendencies as a caller-supplied function (Tendencies::CustomTendencyType, O/src/ocn/Tendencies.h:51-53:
 * std::function<void(Array2DReal Tend, const OceanState*, const AuxiliaryState*, int ThickTimeLevel,
 * int VelTimeLevel, TimeInstant)>, called at the end of the thickness / velocity group, Tendencies.cpp:288-291,
 * 416-419).  The callback ADDS its term to tend_dev ([n_rows_size][row_pitch] device doubles, the first
 * nvertlayers values of rows [0, n_rows_all) are to be written) on `stream`; it is handed the state the tendencies
 * are evaluated on as raw device arrays of the same row pitch (layer thickness [NCellsSize][row_pitch] at the
 * thickness time level, normal velocity [NEdgesSize][row_pitch] at the velocity time level) and the model time.  which: 0 thickness, 1 velocity.  fn == NULL clears
 * that hook.  With a custom hook set the Runge-Kutta stage updates run as separate kernels. */
typedef int (*omg_custom_tend_fn)(void *ctx, double *tend_dev, const double *layer_thickness_dev,
                                  const double *normal_velocity_dev, int n_rows_all, int n_rows_size, int nvertlayers,
                                  int row_pitch, double time_seconds, void *stream);
int omg_tend_set_custom_tendency(omg_tend *t, int which, omg_custom_tend_fn fn, void *ctx);
int omg_tend_clear_custom_tendencies(omg_tend *t);
int omg_tend_set_time(omg_tend *t, double seconds);
int omg_tend_kernel_timing(omg_tend *t, int enable);
int omg_tend_collect_kernel_times(omg_tend *t, double *ms_sum, int *n_kernels, int *n_samples);
const char *omg_tend_kernel_name(int i);
/* which: 0 LayerThicknessTend [NCellsSize][K], 1 NormalVelocityTend [NEdgesSize][K],
 *        2 TracerTend [NT][NCellsSize][K] */
int omg_tend_copy_to_host(const omg_tend *t, int which, double *host, size_t n);
int omg_tend_device_ptr(const omg_tend *t, int which, double **dev, size_t *n);

/* ---- TimeStepper (O/src/timeStepping/TimeStepper.h:57-139 create/doStep;
 *      RungeKutta4Stepper.cpp:68-137, RungeKutta2Stepper.cpp:27-73, ForwardBackwardStepper.cpp:27-82).
 *      type: "Forward-Backward" | "RungeKutta4" | "RungeKutta2" (TimeStepper.h:64-75), or this library's
 *      "Split-Explicit" (omg_stepper_attach_barotropic) ---- */
int omg_stepper_create(const char *type, double time_step_seconds, omg_tend *t, omg_aux *a, const omg_mesh *m,
                       omg_halo *halo, omg_tracers *tr, omg_stepper **out);
int omg_stepper_destroy(omg_stepper *st);
int omg_stepper_do_step(omg_stepper *st, omg_state *s, void *stream);
/* model time in seconds since the reference time (the reference's SimTime / StepClock); doStep hands the
 * stage times to the custom tendencies */
int omg_stepper_set_start_time(omg_stepper *st, double seconds);
int omg_stepper_get_time(const omg_stepper *st, double *seconds);
/* RungeKutta4 only: "FuseStageUpdates" (default 1: the stage updates of TimeStepper.cpp:378-524 run in the
 * epilogue of the RHS kernels, same arithmetic) and "StoreStageTendencies" (default 0: with fused stages the
 * Tendencies arrays are not written), "OverlapHaloExchange" (default 1: with fused stages and neighbours, each
 * exchange starts when the band of cells whose values travel is final and runs on a communication stream
 * while the stage's interior cells are computed), "UseGraphs" (default 0, see omg_tend_set_graphs).  0 / 1. */
int omg_stepper_set_option(omg_stepper *st, const char *name, int value);
/* TimeStepper::changeTimeStep (O/src/timeStepping/TimeStepper.h:141-143) */
int omg_stepper_change_time_step(omg_stepper *st, double time_step_seconds);
/* the update kernel of TimeStepper::updateThicknessByTend / updateVelocityByTend (O/src/timeStepping/
 * TimeStepper.cpp:378-441) on raw device arrays: out[r][k] = in[r][k] + coeff * tend[r][k] for r < n_rows
 * (out may alias in) */
int omg_update_by_tend(double *out_dev, const double *in_dev, const double *tend_dev, double coeff, int n_rows,
                       int nvertlayers, void *stream);
/* the update kernel of TimeStepper::updateTracersByTend (O/src/timeStepping/TimeStepper.cpp:447-469) on raw device
 * arrays: next[l][r][k] = (cur[l][r][k]*h_cur[r][k] + coeff*tend[l][r][k]) / h_next[r][k] for l < n_tracers, r < n_rows
 * and every k < row_length, the ROW LENGTH of the arrays (omg_level_pitch(K) for the library's own); the tracer planes
 * are rows_size rows apart.  omg_update_by_tend's nvertlayers is a row length in the same sense. */
int omg_update_tracers_by_tend(double *next_dev, const double *cur_dev, const double *h_next_dev, const double *h_cur_dev,
                               const double *tend_dev, double coeff, int n_tracers, int n_rows, int rows_size,
                               int row_length, void *stream);
int omg_stepper_coeff_seconds(double mult, double time_step_seconds, double *out);

/* ---- VertCoord (O/src/ocn/VertCoord.h:28-209, VertCoord.cpp:484-864) and Eos (O/src/ocn/Eos.h:278-328,
 * Eos.cpp:113-176).  Numerical contract: omega_amd/csrc/VertCoord.h and Eos.h.  Level-indexed device arrays are
 * [NCellsSize][omg_level_pitch(K)] (interface arrays: omg_level_pitch(K + 1)); per-cell arrays [NCellsSize]; a NULL
 * per-cell array reads as zero. ---- */
/* VertCoord::VertCoord (VertCoord.cpp:50-127): min/max_level_cell are the mesh file's global 1-based
 * minLevelCell / maxLevelCell [nCells] gathered through d (both NULL: every layer active; d may then be NULL);
 * movement_weight_type "Uniform" or "Fixed" (VertCoord.cpp:614-650; anything else fails).  Fails for a host-only
 * mesh.  The edge and vertex layer ranges are computed here. */
int omg_vcoord_create(const omg_mesh *m, const omg_decomp *d, int nvertlayers, double rho0,
                      const char *movement_weight_type, const int32_t *min_level_cell, const int32_t *max_level_cell,
                      omg_vcoord **out);
int omg_vcoord_destroy(omg_vcoord *v);
/* VertCoord::minMaxLayerEdge (VertCoord.cpp:484-535) / minMaxLayerVertex (VertCoord.cpp:539-610), from the current
 * MinLayerCell / MaxLayerCell */
int omg_vcoord_min_max_layer_edge(omg_vcoord *v, void *stream);
int omg_vcoord_min_max_layer_vertex(omg_vcoord *v, void *stream);
/* VertCoord::computePressure (VertCoord.cpp:654-696) */
int omg_vcoord_compute_pressure(omg_vcoord *v, const double *layer_thickness_dev, const double *surface_pressure_dev,
                                void *stream);
/* VertCoord::computeZHeight (VertCoord.cpp:700-739) */
int omg_vcoord_compute_zheight(omg_vcoord *v, const double *layer_thickness_dev, const double *spec_vol_dev,
                               void *stream);
/* VertCoord::computeGeopotential (VertCoord.cpp:743-781) */
int omg_vcoord_compute_geopotential(omg_vcoord *v, const double *tidal_potential_dev,
                                    const double *self_attraction_loading_dev, void *stream);
/* VertCoord::computeTargetThickness (VertCoord.cpp:785-838) */
int omg_vcoord_compute_target_thickness(omg_vcoord *v, void *stream);
/* the fused column pass (VertCoord::computeColumn): one launch equal, bit for bit, to computePressure ->
 * Eos::computeSpecVol(T, S, PressureMid * 1.0e-4) -> computeZHeight -> computeGeopotential, with the thickness of
 * s at thick_time_level and T, S = tracers temp_index, salt_index of t at tracer_time_level (TracerDefs.inc: 0, 1);
 * displaced != 0 also writes SpecVolDisplaced at displacement kdisp (Eos.cpp:144-176) */
int omg_vcoord_compute_column(omg_vcoord *v, const omg_state *s, int thick_time_level, const omg_tracers *t,
                              int tracer_time_level, const omg_eos *e, int temp_index, int salt_index,
                              const double *surface_pressure_dev, const double *tidal_potential_dev,
                              const double *self_attraction_loading_dev, int displaced, int kdisp, void *stream);
/* arrays by reference member name (VertCoord.h:71-120): real "PressureInterface", "PressureMid", "ZInterface",
 * "ZMid", "GeopotentialMid", "LayerThicknessTarget", "RefLayerThickness", "VertCoordMovementWeights",
 * "BottomDepth"; int32 "MinLayerCell", "MaxLayerCell", "Min/MaxLayerEdgeTop/Bot", "Min/MaxLayerVertexTop/Bot" */
int omg_vcoord_copy_to_host(const omg_vcoord *v, const char *name, double *host, size_t n);
int omg_vcoord_copy_to_device(omg_vcoord *v, const char *name, const double *host, size_t n);
int omg_vcoord_device_ptr(const omg_vcoord *v, const char *name, double **dev, size_t *n);
int omg_vcoord_copy_to_host_i4(const omg_vcoord *v, const char *name, int32_t *host, size_t n);
int omg_vcoord_copy_to_device_i4(omg_vcoord *v, const char *name, const int32_t *host, size_t n);
/* "Rho0", "Gravity" (VertCoord's own g = 9.80616, VertCoord.cpp:659) */
int omg_vcoord_get_real(const omg_vcoord *v, const char *name, double *value);

/* Eos::init (Eos.cpp:60-110): eos_type "Linear" / "linear" or "teos10" / "teos-10" / "TEOS-10" (anything else
 * fails); the linear parameters DRhoDT, DRhoDS, RhoT0S0 (Eos.h:247-249; defaults -0.2, 0.8, 1000).  Fails for a
 * host-only mesh. */
int omg_eos_create(const omg_mesh *m, int nvertlayers, const char *eos_type, double drhodt, double drhods,
                   double rhot0s0, omg_eos **out);
int omg_eos_destroy(omg_eos *e);
/* Eos::computeSpecVol (Eos.cpp:113-140) / computeSpecVolDisp (Eos.cpp:144-176); the pressure used is
 * pressure * p_scale (1.0: dbar as given; 1.0e-4: a Pa array such as VertCoord's PressureMid) */
int omg_eos_compute_spec_vol(omg_eos *e, const double *conserv_temp_dev, const double *abs_salinity_dev,
                             const double *pressure_dev, double p_scale, void *stream);
int omg_eos_compute_spec_vol_disp(omg_eos *e, const double *conserv_temp_dev, const double *abs_salinity_dev,
                                  const double *pressure_dev, int kdisp, double p_scale, void *stream);
/* "SpecVol", "SpecVolDisplaced" (Eos.h:281-282) */
int omg_eos_copy_to_host(const omg_eos *e, const char *name, double *host, size_t n);
int omg_eos_copy_to_device(omg_eos *e, const char *name, const double *host, size_t n);
int omg_eos_device_ptr(const omg_eos *e, const char *name, double **dev, size_t *n);

/* ---- VertMix: vertical mixing coefficients and implicit vertical diffusion.  The reference specifies it in
 * O/doc/design/VerticalMixingCoeff.md only (no code yet).  Numerical contract and the stated deviations (N2 form,
 * Ri >= 0 clamp, integer exponents): omega_amd/csrc/VertMix.h.  Arrays are level-indexed device arrays as above;
 * edge arrays are [NEdgesSize][omg_level_pitch(K)].  Every call is asynchronous on stream and allocates nothing. ---- */
/* VerticalMixingCoeff.md section 4.1.1: the configuration, with its defaults */
typedef struct omg_vertmix_config {
   double BackgroundViscosity;   /* 1.0e-4 */
   double BackgroundDiffusivity; /* 1.0e-5 */
   int32_t EnableShearMix;       /* 1 */
   double ShearNuZero;           /* 0.005 */
   double ShearAlpha;            /* 5 */
   double ShearExponent;         /* 2 */
   int32_t EnableConvectiveMix;  /* 1 */
   double ConvectiveDiffusivity; /* 1.0 */
   double ConvectiveTriggerBVF;  /* 0.0 */
} omg_vertmix_config;
int omg_vertmix_config_default(omg_vertmix_config *c);
/* VerticalMixingCoeff.md section 4.1 (construction): fails for negative viscosities or diffusivities, more than 1024
 * layers (the tridiagonal limit), a host-only mesh, or a VertCoord of another mesh.  c NULL: the defaults. */
int omg_vertmix_create(const omg_mesh *m, const omg_vcoord *v, const omg_vertmix_config *c, omg_vertmix **out);
int omg_vertmix_destroy(omg_vertmix *x);
/* VerticalMixingCoeff.md section 4.2 (Brunt-Vaisala frequency, here on VertMix): BruntVaisalaFreqSq from e's SpecVol
 * and SpecVolDisplaced (after omg_vcoord_compute_column with displaced = 1, kdisp = 1) and the VertCoord's ZMid */
int omg_vertmix_compute_bvf(omg_vertmix *x, const omg_eos *e, void *stream);
/* VerticalMixingCoeff.md section 4.2 (background, shear and convective coefficients): VertVisc and VertDiff from the
 * edge velocities and bvf_dev (NULL: the object's own BruntVaisalaFreqSq) */
int omg_vertmix_compute(omg_vertmix *x, const double *normal_velocity_dev, const double *tangential_velocity_dev,
                        const double *bvf_dev, void *stream);
/* VerticalMixingCoeff.md section 4.3 (coefficients feeding TriDiagDiffSolver, no-flux boundaries): backward-Euler
 * diffusion with VertDiff of tracers_dev [ntracers][NCellsSize][pitch] in place, all tracers in one pass */
int omg_vertmix_apply_tracers(omg_vertmix *x, const double *layer_thickness_dev, double *tracers_dev, int ntracers,
                              double dt, void *stream);
/* VerticalMixingCoeff.md section 4.3: backward-Euler diffusion with VertVisc of the normal velocity in place */
int omg_vertmix_apply_velocity(omg_vertmix *x, const double *layer_thickness_dev, double *normal_velocity_dev,
                               double dt, void *stream);
/* "VertDiff", "VertVisc", "BruntVaisalaFreqSq" ([NCellsSize][K]) */
int omg_vertmix_copy_to_host(const omg_vertmix *x, const char *name, double *host, size_t n);
int omg_vertmix_copy_to_device(omg_vertmix *x, const char *name, const double *host, size_t n);
int omg_vertmix_device_ptr(const omg_vertmix *x, const char *name, double **dev, size_t *n);

/* The forced solves (O/doc/design/OmegaV1GoverningEqns.md section 11, "Forcing at the top and bottom of the ocean";
 * contract in omega_amd/csrc/VertMix.h).  surface_flux_dev: ntracers x NCellsSize values, tracer-major, tracer units *
 * m/s, positive into the ocean, added to the top row's right-hand side (NULL: no flux). */
int omg_vertmix_apply_tracers_forced(omg_vertmix *x, const double *layer_thickness_dev, double *tracers_dev, int ntracers,
                                     double dt, const double *surface_flux_dev, void *stream);
/* Wind stress normal_stress_dev [NEdgesSize] (Pa; NULL: none) as the top boundary condition, the linearised quadratic
 * bottom drag bottom_drag_coeff * |u| with the speed from the edge's own normal and tangential velocity as the bottom
 * one (tangential_velocity_dev [NEdgesSize][pitch], required iff bottom_drag_coeff != 0) and Rayleigh drag
 * rayleigh_drag_coeff (1/s) on every level.  A negative coefficient fails; a zero one skips its term; with every
 * term skipped the result is omg_vertmix_apply_velocity's bit for bit. */
int omg_vertmix_apply_velocity_forced(omg_vertmix *x, const double *layer_thickness_dev, double *normal_velocity_dev,
                                      double dt, double bottom_drag_coeff, double rayleigh_drag_coeff,
                                      const double *normal_stress_dev, const double *tangential_velocity_dev,
                                      void *stream);

/* ---- VertMixStep: the whole mixing sequence of a step as one call (omega_amd/csrc/VertMixStep.h): the displaced column
 * pass (temperature at tracer 0, salinity at 1), N2, the tangential velocity, the coefficients, the forced tracer solve
 * and the forced velocity solve, equal bit for bit to those six calls made one by one.  The object keeps pointers to x,
 * v and e: destroy it before them.  It allocates in create only. ---- */
/* fails for a host-only mesh, x / v / e NULL or of another mesh or layer count, ntracers < 2 and more than 1008 layers
 * (the fused column pass's limit) */
int omg_vertmix_step_create(const omg_mesh *m, omg_vertmix *x, omg_vcoord *v, omg_eos *e, int ntracers,
                            omg_vertmix_step **out);
int omg_vertmix_step_destroy(omg_vertmix_step *ms);
/* the coefficients of the velocity solve (>= 0; both 0 at creation) and whether NormalStressEdge is applied (off) */
int omg_vertmix_step_set_boundary(omg_vertmix_step *ms, double bottom_drag_coeff, double rayleigh_drag_coeff,
                                  int use_wind_stress);
/* layer_thickness_dev [NCellsSize][pitch]; normal_velocity_dev [NEdgesSize][pitch] and tracers_dev
 * [ntracers][NCellsSize][pitch] are mixed in place */
int omg_vertmix_step_apply(omg_vertmix_step *ms, const double *layer_thickness_dev, double *normal_velocity_dev,
                           double *tracers_dev, double dt, void *stream);
/* the same on time level time_level of s and tracer_time_level of t */
int omg_vertmix_step_apply_state(omg_vertmix_step *ms, const omg_state *s, int time_level, const omg_tracers *t,
                                 int tracer_time_level, double dt, void *stream);
/* "TangentialVelocity" ([NEdgesSize][K]), "NormalStressEdge" ([NEdgesSize]), "SurfaceTracerFlux" ([ntracers][NCellsSize]),
 * "SurfacePressure", "TidalPotential", "SelfAttractionLoading" ([NCellsSize]); all zero at creation */
int omg_vertmix_step_copy_to_host(const omg_vertmix_step *ms, const char *name, double *host, size_t n);
int omg_vertmix_step_copy_to_device(omg_vertmix_step *ms, const char *name, const double *host, size_t n);
int omg_vertmix_step_device_ptr(const omg_vertmix_step *ms, const char *name, double **dev, size_t *n);
/* TimeStepper::attachVertMix: every omg_stepper_do_step runs the sequence on the new time level with dt = the time step,
 * immediately before the time levels rotate (ms NULL: detach).  Fails for another mesh, layer or tracer count, and for
 * a stepper whose halo has neighbours: multi-rank mixing needs the halo of the new level before and after the solve and
 * is not built.  While attached RungeKutta4 runs its plain stage sequence and nothing is replayed as a graph.  Detach
 * before destroying ms. */
int omg_stepper_attach_vert_mix(omg_stepper *st, omg_vertmix_step *ms);

/* ---- PressureGrad: the layered-ocean pressure-gradient force on edges, -(grad Phi) - alpha grad p along the layers
 * (O/doc/design/OmegaV1GoverningEqns.md, discrete momentum equation; the reference has no code for it).  Numerical
 * contract: omega_amd/csrc/PressureGrad.h.  Arrays are level-indexed device arrays as above.  Every call is
 * asynchronous on stream and allocates nothing.  The object keeps pointers to v and e: destroy it before them. ---- */
/* fails for a host-only mesh and for a VertCoord or Eos of another mesh or layer count */
int omg_pgrad_create(const omg_mesh *m, omg_vcoord *v, omg_eos *e, omg_pgrad **out);
int omg_pgrad_destroy(omg_pgrad *p);
/* the fused column pass (omg_vcoord_compute_column) from raw arrays: layer_thickness_dev [NCellsSize][pitch],
 * tracers_dev [ntracers >= 2][NCellsSize][pitch] with temperature at index 0 and salinity at 1, no displaced volume,
 * and the object's SurfacePressure / TidalPotential / SelfAttractionLoading */
int omg_pgrad_update_column(omg_pgrad *p, const double *layer_thickness_dev, const double *tracers_dev, int ntracers,
                            void *stream);
/* tend_dev [NEdgesSize][pitch] -= the term, from the VertCoord's PressureMid / GeopotentialMid and the Eos's SpecVol as
 * they stand */
int omg_pgrad_compute(omg_pgrad *p, double *tend_dev, void *stream);
/* the same from the caller's [NCellsSize][pitch] arrays (PressureMid in Pa) */
int omg_pgrad_compute_arrays(omg_pgrad *p, double *tend_dev, const double *pressure_mid_dev,
                             const double *geopotential_mid_dev, const double *spec_vol_dev, void *stream);
/* "SurfacePressure", "TidalPotential", "SelfAttractionLoading" ([NCellsSize], zero at creation) */
int omg_pgrad_device_ptr(const omg_pgrad *p, const char *name, double **dev, size_t *n);
int omg_pgrad_copy_to_device(omg_pgrad *p, const char *name, const double *host, size_t n);
int omg_pgrad_copy_to_host(const omg_pgrad *p, const char *name, double *host, size_t n);
/* Tendencies::attachPressureGrad: the term becomes an opt-in velocity term of t (p NULL: detach).  Fails while
 * SSHTendencyEnable is on.  While attached omg_tend_compute_all runs the column pass on the stage's thickness and
 * tracers first; the velocity-only calls use the column fields as they stand; the Runge-Kutta stage updates run as
 * separate kernels and nothing is replayed as a graph.  Detach before destroying p. */
int omg_tend_attach_pressure_grad(omg_tend *t, omg_pgrad *p);

/* ---- VertAdv: vertical transport through the layer interfaces and the vertical advection of thickness, tracers and
 * momentum (O/doc/design/OmegaV1GoverningEqns.md, discrete-mass / -tracer / -momentum; the reference has no code for
 * them).  Numerical contract: omega_amd/csrc/VertAdv.h.  Arrays are level-indexed device arrays as above.  Every call
 * is asynchronous on stream and allocates nothing.  The object keeps a pointer to v: destroy it before v. ---- */
/* tracer_flux_order: 1 upwind, 2 centred.  Fails for another order, a host-only mesh, a VertCoord of another mesh or
 * layer count, and more layers than omg_vertadv_max_layers */
int omg_vertadv_create(const omg_mesh *m, const omg_vcoord *v, int tracer_flux_order, omg_vertadv **out);
int omg_vertadv_destroy(omg_vertadv *a);
int omg_vertadv_max_layers(int *n);
/* VertAdv::TracerTermEnable (default on).  Off: a Tendencies that a is attached to leaves a's tracer term out of
 * omg_tend_compute_all, omg_tend_compute_transport and the tracer group call, for a MonotoneAdv that limits the vertical
 * flux itself (omg_monoadv_attach_vert_adv); the thickness and velocity terms stay.  omg_vertadv_add_tracers ignores it */
int omg_vertadv_set_tracer_term(omg_vertadv *a, int on);
/* VerticalTransport from thickness_tend_dev [NCellsSize][pitch] (the horizontal part); add_thickness != 0 also applies
 * omg_vertadv_add_thickness to thickness_tend_dev in the same launch */
int omg_vertadv_compute_transport(omg_vertadv *a, double *thickness_tend_dev, int add_thickness, void *stream);
/* thickness_tend_dev [NCellsSize][pitch] += VerticalTransport[K+1] - VerticalTransport[K] */
int omg_vertadv_add_thickness(omg_vertadv *a, double *thickness_tend_dev, void *stream);
/* tracer_tend_dev, tracers_dev [ntracers][NCellsSize][pitch]; layer_thickness_dev [NCellsSize][pitch] */
int omg_vertadv_add_tracers(omg_vertadv *a, double *tracer_tend_dev, const double *layer_thickness_dev,
                            const double *tracers_dev, int ntracers, void *stream);
/* velocity_tend_dev, normal_velocity_dev [NEdgesSize][pitch]; layer_thickness_dev [NCellsSize][pitch] */
int omg_vertadv_add_velocity(omg_vertadv *a, double *velocity_tend_dev, const double *layer_thickness_dev,
                             const double *normal_velocity_dev, void *stream);
/* "VerticalTransport" ([NCellsSize][NVertLayers], zero at creation) */
int omg_vertadv_device_ptr(const omg_vertadv *a, const char *name, double **dev, size_t *n);
int omg_vertadv_copy_to_device(omg_vertadv *a, const char *name, const double *host, size_t n);
int omg_vertadv_copy_to_host(const omg_vertadv *a, const char *name, double *host, size_t n);
/* Tendencies::attachVertAdv: the terms become opt-in terms of t (a NULL: detach).  While attached omg_tend_compute_all
 * adds them after the built-in terms and before an attached PressureGrad and the custom hooks; the velocity and tracer
 * group calls use VerticalTransport as it stands; the Runge-Kutta stage updates run as separate kernels and nothing is
 * replayed as a graph.  Detach before destroying a. */
int omg_tend_attach_vert_adv(omg_tend *t, omg_vertadv *a);

/* ---- BarotropicMode: the vertical split of the edge velocity into its thickness-weighted mean and the baroclinic
 * remainder, and forward-backward sub-cycling of the 2-D (SSH, barotropic velocity) system (O/doc/design/
 * TimeStepping.md names the scheme, OmegaV1GoverningEqns.md section 1 the split step; the reference has no code for
 * them).  Numerical contract: omega_amd/csrc/BarotropicMode.h.  Arrays are level-indexed device arrays as above.  Every
 * call is asynchronous on stream and allocates nothing.  The object keeps a pointer to v: destroy it before v. ---- */
/* gravity: 9.80616 is VertCoord's.  Fails for a host-only mesh, a VertCoord that is NULL or of another mesh or layer
 * count, and more layers than omg_btr_max_layers */
int omg_btr_create(const omg_mesh *m, const omg_vcoord *v, double gravity, omg_btr **out);
int omg_btr_destroy(omg_btr *b);
int omg_btr_max_layers(int *n);
/* BtrThickEdge, BtrVelocity, BclVelocity from layer_thickness_dev [NCellsSize][pitch] and normal_velocity_dev
 * [NEdgesSize][pitch]; with_ssh != 0 also runs omg_btr_compute_ssh in the same launch */
int omg_btr_split_velocity(omg_btr *b, const double *layer_thickness_dev, const double *normal_velocity_dev, int with_ssh,
                           void *stream);
/* BtrForcing: the thickness-weighted vertical mean of velocity_tend_dev [NEdgesSize][pitch] */
int omg_btr_compute_forcing(omg_btr *b, const double *layer_thickness_dev, const double *velocity_tend_dev, void *stream);
/* SSH = column sum of layer_thickness_dev - BottomDepth (the VertCoord's) */
int omg_btr_compute_ssh(omg_btr *b, const double *layer_thickness_dev, void *stream);
/* normal_velocity_dev [NEdgesSize][pitch] = BclVelocity + BtrVelocity on each edge's level range */
int omg_btr_recombine(omg_btr *b, double *normal_velocity_dev, void *stream);
/* nsub forward-backward sub-steps of dt_btr seconds on SSH and BtrVelocity under BtrForcing; BtrFluxMean is the mean
 * edge flux of the sub-steps.  Fails for nsub < 1 and a dt_btr that is not finite and positive */
int omg_btr_subcycle(omg_btr *b, int nsub, double dt_btr, void *stream);
/* The three calls of a split-explicit step (omega_amd/csrc/BarotropicMode.h has the contract).
 * BtrTendMean = the thickness-weighted vertical mean of velocity_tend_dev; BtrForcing = BtrTendMean less the bracket of
 * a sub-step (Coriolis sum and surface-height gradient) at SSH and BtrVelocity as they stand */
int omg_btr_compute_residual_forcing(omg_btr *b, const double *layer_thickness_dev, const double *velocity_tend_dev,
                                     void *stream);
/* velocity_out_dev = BclVelocity + BtrFluxMean/BtrThickEdge on each edge's level range, velocity_old_dev on the other
 * levels; all [NEdgesSize][pitch] */
int omg_btr_transport_velocity(omg_btr *b, const double *velocity_old_dev, double *velocity_out_dev, void *stream);
/* velocity_out_dev = (BclVelocity + dt*(velocity_tend_dev - BtrTendMean)) + BtrVelocity on each edge's level range,
 * velocity_old_dev + dt*velocity_tend_dev on the other levels; velocity_out_dev may be velocity_old_dev.  Fails for a dt
 * that is not finite and positive */
int omg_btr_advance_velocity(omg_btr *b, const double *velocity_old_dev, const double *velocity_tend_dev, double dt,
                             double *velocity_out_dev, void *stream);
/* SplitExplicitStepper::attachBarotropic (omega_amd/csrc/SplitExplicitStepper.h): required before the first
 * omg_stepper_do_step of a "Split-Explicit" stepper, which then carries the 2-D system through nsub sub-steps of
 * BarotropicMode per step.  Fails for any other stepper type, a null b, one of another mesh or layer count, nsub < 1 and
 * a stepper whose halo has neighbours (the sub-cycle knows no halo exchange).  The stepper keeps a pointer to b. */
int omg_stepper_attach_barotropic(omg_stepper *st, omg_btr *b, int nsub);
/* SplitExplicitStepper::UseFusedTransport (default on): the thickness and tracer tendencies of a step through
 * omg_tend_compute_transport (two launches) instead of the two group calls (five); the step's result is the same bit
 * for bit either way.  Fails for any other stepper type. */
int omg_stepper_set_fused_transport(omg_stepper *st, int on);
/* SplitExplicitStepper::UseMomentumRHS: the first evaluation of a step through omg_tend_compute_momentum instead of
 * omg_tend_compute_all.  SplitExplicitStepper::FoldUpdates: with the fused transport on, the transport tendencies and
 * the thickness and tracer updates through omg_tend_compute_transport_update (keep_tendencies = 1) instead of three
 * calls (with tracers and TracerHyperDiffTendencyEnable off the three calls run: the folded call is no faster there).
 * The step's result is the same bit for bit under every combination.  Both fail for any other stepper type. */
int omg_stepper_set_momentum_rhs(omg_stepper *st, int on);
int omg_stepper_set_folded_updates(omg_stepper *st, int on);
/* "BtrVelocity", "BtrThickEdge", "BtrForcing", "BtrFluxMean", "BtrTendMean" ([NEdgesSize]), "SSH" ([NCellsSize]), "BclVelocity"
 * ([NEdgesSize][NVertLayers]); all zero at creation */
int omg_btr_device_ptr(const omg_btr *b, const char *name, double **dev, size_t *n);
int omg_btr_copy_to_device(omg_btr *b, const char *name, const double *host, size_t n);
int omg_btr_copy_to_host(const omg_btr *b, const char *name, double *host, size_t n);

/* ---- MonotoneAdv: flux-corrected (Zalesak) horizontal tracer advection, the centred edge flux limited against the
 * upwind one so that a forward update over dt creates no new extremum (O/doc/design/Tracers.md asks for a monotone
 * scheme; the reference has no code for one).  Numerical contract: omega_amd/csrc/MonotoneAdv.h.  Arrays are
 * level-indexed device arrays as above.  The call is asynchronous on stream and allocates nothing. ---- */
/* flux_thickness_upwind: the edge thickness of the mass flux, 0 centred, else upwind; it must be the AuxiliaryState's
 * choice.  Fails for a host-only mesh, nvertlayers < 1 and max_tracers < 1 */
int omg_monoadv_create(const omg_mesh *m, int nvertlayers, int max_tracers, int flux_thickness_upwind, omg_monoadv **out);
int omg_monoadv_destroy(omg_monoadv *a);
/* tracer_tend_dev [ntracers][NCellsSize][pitch] += the limited flux divergence of tracers_dev (same shape) over the step
 * h_old_dev -> h_new_dev ([NCellsSize][pitch]) of length dt by normal_velocity_dev ([NEdgesSize][pitch]); "ScaleIn" and
 * "ScaleOut" are overwritten.  Fails for ntracers outside 1 .. max_tracers and a dt that is not finite and positive.
 * Two launches; three after omg_monoadv_set_horz_order(a, 3 or 4, ...), which also overwrites "Hess" */
int omg_monoadv_add_tracers(omg_monoadv *a, double *tracer_tend_dev, const double *h_old_dev, const double *h_new_dev,
                            const double *normal_velocity_dev, const double *tracers_dev, int ntracers, double dt,
                            void *stream);
/* MonotoneAdv::attachVertAdv: while v is attached (NULL: detach) omg_monoadv_add_tracers runs the 3-D form, which limits
 * the vertical tracer flux of v's VerticalTransport, as it stands, together with the horizontal ones on the layer ranges
 * of v's VertCoord: the same arguments, two launches.  Fails for a v of another mesh or layer count.  a keeps a pointer
 * to v: detach before destroying it. */
int omg_monoadv_attach_vert_adv(omg_monoadv *a, omg_vertadv *v);
/* MonotoneAdv::setHorzOrder: the order of the horizontal flux under the limiter.  2 (the state at creation): the centred
 * flux, two launches.  4 and 3: the centred edge value corrected by the second derivative of the tracer along the line
 * between the two cells, from a least-squares quadratic at each cell (Skamarock and Gassmann 2011); order 3 adds the
 * upwind-biased term times coef3rd (in (0, 1]; MPAS's default 0.25; unused at the other orders).  The first such call
 * allocates "Hess" and the tables; it builds the tables on the host from the mesh's cell positions with sphere_radius
 * (0: a planar mesh) and the periods of a planar mesh (0: not periodic) and uploads them.  omg_monoadv_add_tracers then
 * makes three launches and still allocates nothing; order 2 frees nothing and gives the bits of an object never
 * configured.  Fails for an order outside {2, 3, 4}, coef3rd outside (0, 1] at order 3 and a negative or non-finite
 * radius or period.  A halo of at least 3 cell layers gives the global mesh's result on owned cells */
int omg_monoadv_set_horz_order(omg_monoadv *a, int order, double coef3rd, double sphere_radius, double x_period,
                               double y_period);
/* The tables omg_monoadv_set_horz_order(a, 3 or 4, ...) builds for an object on m, on the host alone (m may be
 * host-only): fit_cell [NCellsSize], the other three [NCellsSize][MaxEdges][3].  Order 2 writes nothing.  Fails as
 * omg_monoadv_set_horz_order does */
int omg_monoadv_high_order_tables(const omg_mesh *m, int order, double coef3rd, double sphere_radius, double x_period,
                                  double y_period, double *fit_cell, double *hess_weight, double *edge_dir_own,
                                  double *edge_dir_across);
/* kernel launches omg_monoadv_add_tracers has issued on a so far (two per call, three at order 3 or 4) */
int omg_monoadv_launch_count(const omg_monoadv *a, int64_t *n);
/* "ScaleIn", "ScaleOut" ([max_tracers][NCellsSize][NVertLayers], zero at creation); after
 * omg_monoadv_set_horz_order(3 or 4) also "Hess" ([max_tracers][3: xx, xy, yy][NCellsSize][NVertLayers]), "HessWeight",
 * "EdgeDirOwn", "EdgeDirAcross" ([NCellsSize][MaxEdges][3]) and "FitCell" ([NCellsSize], 1.0 or 0.0); before it these
 * five names fail */
int omg_monoadv_device_ptr(const omg_monoadv *a, const char *name, double **dev, size_t *n);
int omg_monoadv_copy_to_device(omg_monoadv *a, const char *name, const double *host, size_t n);
int omg_monoadv_copy_to_host(const omg_monoadv *a, const char *name, double *host, size_t n);
/* SplitExplicitStepper::attachMonotoneAdv (omega_amd/csrc/SplitExplicitStepper.h): the horizontal tracer advection of
 * every step of a "Split-Explicit" stepper through a (NULL: detach); the step then runs the transport tendencies, the
 * thickness update, omg_monoadv_add_tracers and the tracer update as four calls.  Fails for any other stepper type, an a
 * of another mesh or layer count, max_tracers below the stepper's tracer count, a flux_thickness_upwind that differs
 * from the AuxiliaryState's option, and while TracerHorzAdvTendencyEnable of the Tendencies is on (omg_stepper_do_step
 * checks the last three again).  An a with a VertAdv attached (omg_monoadv_attach_vert_adv) is also refused, at the
 * attachment and in every step, unless that VertAdv is the one attached to the Tendencies and its tracer term is off
 * (omg_vertadv_set_tracer_term): the step's VerticalTransport is the Tendencies', and the vertical term would be applied
 * twice.  The stepper keeps a pointer to a: detach before destroying it. */
int omg_stepper_attach_monotone_adv(omg_stepper *st, omg_monoadv *a);

/* ---- GentMcWilliams: the eddy-induced (bolus) velocity of the Gent-McWilliams closure on the edges, in the
 * boundary-value form of Ferrari et al. (2010) -- one symmetric tridiagonal system per edge column (the reference has no
 * code for it).  Numerical contract: omega_amd/csrc/GentMcWilliams.h.  Arrays are level-indexed device arrays as above.
 * Every call is asynchronous on stream and allocates nothing.  The object keeps pointers to v and e: destroy it before
 * them. ---- */
typedef struct omg_gm omg_gm;
/* kappa: the diffusivity every entry of "Kappa" starts with (m^2 s^-1, the class's default is 600); grav_wave_speed: c
 * of the boundary-value problem (m s^-1, default 0.3).  Fails for a host-only mesh, a VertCoord or Eos of another mesh
 * or layer count, more than 1024 layers, a kappa that is negative or not finite and a grav_wave_speed that is not
 * finite or <= 0 */
int omg_gm_create(const omg_mesh *m, omg_vcoord *v, omg_eos *e, double kappa, double grav_wave_speed, omg_gm **out);
int omg_gm_destroy(omg_gm *g);
/* the fused column pass (omg_vcoord_compute_column) from raw arrays: layer_thickness_dev [NCellsSize][pitch],
 * tracers_dev [ntracers >= 2][NCellsSize][pitch] with temperature at index 0 and salinity at 1, the displaced volume at
 * kdisp = 1, and the object's SurfacePressure / TidalPotential / SelfAttractionLoading */
int omg_gm_update_column(omg_gm *g, const double *layer_thickness_dev, const double *tracers_dev, int ntracers,
                         void *stream);
/* "BolusVelocity" and "StreamFunction" on every edge's level range, from the Eos's SpecVol / SpecVolDisplaced and the
 * VertCoord's ZMid as they stand; transport_dev [NEdgesSize][pitch] += BolusVelocity there (NULL: no term).  One launch */
int omg_gm_compute(omg_gm *g, const double *layer_thickness_dev, double *transport_dev, void *stream);
/* the same from the caller's [NCellsSize][pitch] arrays */
int omg_gm_compute_arrays(omg_gm *g, const double *layer_thickness_dev, const double *spec_vol_dev,
                          const double *spec_vol_displaced_dev, const double *z_mid_dev, double *transport_dev,
                          void *stream);
/* "Kappa" ([NEdgesSize], kappa at creation), "BolusVelocity", "StreamFunction" ([NEdgesSize][K], zero at creation; row K
 * of StreamFunction is the interface at the top of layer K), "SurfacePressure", "TidalPotential",
 * "SelfAttractionLoading" ([NCellsSize], zero at creation) */
int omg_gm_device_ptr(const omg_gm *g, const char *name, double **dev, size_t *n);
int omg_gm_copy_to_device(omg_gm *g, const char *name, const double *host, size_t n);
int omg_gm_copy_to_host(const omg_gm *g, const char *name, double *host, size_t n);
/* SplitExplicitStepper::attachGentMcWilliams (omega_amd/csrc/SplitExplicitStepper.h): every step of a "Split-Explicit"
 * stepper adds the bolus velocity of the current level's stratification to its transporting velocity (g NULL: detach):
 * omg_gm_update_column and omg_gm_compute on the current thickness and tracers between the transport velocity and the
 * transport tendencies.  The prognostic velocity never sees it.  Fails for any other stepper type, a g of another mesh
 * or layer count, a stepper with fewer than 2 tracers, and, while a PressureGrad is attached to the Tendencies, a g on
 * another VertCoord or Eos than that PressureGrad's (omg_stepper_do_step checks again); the caller keeps the forcing
 * arrays of the two objects equal.  The stepper keeps a pointer to g: detach before destroying it. */
int omg_stepper_attach_gm(omg_stepper *st, omg_gm *g);

/* ---- Redi: isoneutral diffusion of the tracers, the partner of GentMcWilliams -- the small-slope tensor with the
 * isopycnal slope relative to the layers on the edge interfaces, its two cross terms explicit on the tracer tendency and
 * its slope-squared part a vertical diffusivity for the implicit tracer solve of VertMix (the reference has no code for
 * it).  Numerical contract: omega_amd/csrc/Redi.h.  Arrays are level-indexed device arrays as above.  Every call is
 * asynchronous on stream and allocates nothing.  The object keeps pointers to v and e: destroy it before them. ---- */
typedef struct omg_redi omg_redi;
/* max_tracers: the most tracers omg_redi_add_tracer_tend takes (>= 1); kappa: the diffusivity every entry of "Kappa"
 * starts with (m^2 s^-1, the class's default is 600, >= 0 and finite); slope_max: the bound of |slope| (default 0.01,
 * finite and > 0); n2_floor: the least N^2 the slope is divided by (s^-2, default 1e-10, finite and > 0).  Fails also
 * for a host-only mesh, a VertCoord or Eos of another mesh or layer count and more than 1024 layers */
int omg_redi_create(const omg_mesh *m, omg_vcoord *v, omg_eos *e, int max_tracers, double kappa, double slope_max,
                    double n2_floor, omg_redi **out);
int omg_redi_destroy(omg_redi *r);
/* the fused column pass exactly as omg_gm_update_column runs it, with this object's SurfacePressure / TidalPotential /
 * SelfAttractionLoading */
int omg_redi_update_column(omg_redi *r, const double *layer_thickness_dev, const double *tracers_dev, int ntracers,
                           void *stream);
/* "SlopeInterface" on every edge's level range (row K: the interface at the top of layer K; 0 at the top of the range),
 * from the Eos's SpecVol / SpecVolDisplaced and the VertCoord's ZMid as they stand.  layer_thickness_dev is required
 * and not read (the slope does not depend on it).  One launch */
int omg_redi_compute_slope(omg_redi *r, const double *layer_thickness_dev, void *stream);
/* the same from the caller's [NCellsSize][pitch] arrays */
int omg_redi_compute_slope_arrays(omg_redi *r, const double *layer_thickness_dev, const double *spec_vol_dev,
                                  const double *spec_vol_displaced_dev, const double *z_mid_dev, void *stream);
/* tracer_tend_dev [ntracers][NCellsSize][pitch] += the divergence of the horizontal isoneutral flux and of the vertical
 * cross flux of tracers_dev [ntracers][NCellsSize][pitch], on every cell's layer range, from "SlopeInterface" and "Kappa"
 * as they stand; z_mid_dev NULL: the VertCoord's ZMid.  Fails for ntracers outside 1 .. max_tracers.  One launch */
int omg_redi_add_tracer_tend(omg_redi *r, double *tracer_tend_dev, const double *layer_thickness_dev,
                             const double *tracers_dev, int ntracers, const double *z_mid_dev, void *stream);
/* "VertDiffusivity" (Kappa times the squared slope, averaged to the cell interfaces); vert_diff_dev [NCellsSize][pitch]
 * += VertDiffusivity there (NULL: no term).  One launch */
int omg_redi_compute_vert_diffusivity(omg_redi *r, double *vert_diff_dev, void *stream);
/* kernel launches the three compute calls have issued on this object so far */
int omg_redi_launch_count(const omg_redi *r, int64_t *n);
/* "Kappa" ([NEdgesSize], kappa at creation), "SlopeInterface" ([NEdgesSize][K], zero at creation), "VertDiffusivity"
 * ([NCellsSize][K], zero at creation), "SurfacePressure", "TidalPotential", "SelfAttractionLoading" ([NCellsSize], zero
 * at creation) */
int omg_redi_device_ptr(const omg_redi *r, const char *name, double **dev, size_t *n);
int omg_redi_copy_to_device(omg_redi *r, const char *name, const double *host, size_t n);
int omg_redi_copy_to_host(const omg_redi *r, const char *name, double *host, size_t n);
/* VertMixStep::attachRedi (omega_amd/csrc/VertMixStep.h): omg_vertmix_step_apply adds "VertDiffusivity", from the slopes
 * r last computed, to the VertMix's VertDiff between the coefficients and the tracer solve (r NULL: detach).  Fails for
 * an r of another mesh, layer count, VertCoord or Eos.  ms keeps a pointer to r: detach before destroying it. */
int omg_vertmixstep_attach_redi(omg_vertmix_step *ms, omg_redi *r);
/* SplitExplicitStepper::attachRedi (omega_amd/csrc/SplitExplicitStepper.h): every step of a "Split-Explicit" stepper
 * computes the slopes of the current level (after the column pass: the GentMcWilliams's if one is attached, else
 * omg_redi_update_column) and adds omg_redi_add_tracer_tend to the tracer tendency before the tracer update (r NULL:
 * detach).  Fails for any other stepper type, an r of another mesh or layer count, max_tracers below the stepper's
 * tracer count, fewer than 2 tracers, an r on another VertCoord or Eos than an attached GentMcWilliams's or
 * PressureGrad's, a stepper without omg_stepper_attach_vert_mix and one whose VertMixStep does not have this r attached
 * (omg_stepper_do_step checks again).  The stepper keeps a pointer to r: detach before destroying it. */
int omg_stepper_attach_redi(omg_stepper *st, omg_redi *r);

/* ---- VertRemap (omega_amd/csrc/VertRemap.h; O/doc/design/VertCoord.md sections 2.6, 2.7, design only): vertical
 * Lagrangian remapping -- the target thickness of the VertCoord from the column totals of a thickness, and the
 * conservative PCM / PLM / PPM remap of tracers and velocity from that thickness onto the target.  Level-indexed device
 * arrays are [rows][pitch] with pitch = omg_level_pitch(NVertLayers).  Every call is asynchronous on stream, allocates
 * nothing and writes nothing outside the layer ranges.  The object keeps a pointer to v: destroy it before v. ---- */
typedef struct omg_vremap omg_vremap;
/* order: 1 PCM, 2 PLM, 3 PPM; max_tracers: the most tracers a call takes (>= 0).  Fails for another order, a negative
 * max_tracers, a host-only mesh, a VertCoord that is NULL or of another mesh or layer count, and more layers than
 * omg_vremap_max_layers */
int omg_vremap_create(const omg_mesh *m, const omg_vcoord *v, int order, int max_tracers, omg_vremap **out);
int omg_vremap_destroy(omg_vremap *r);
int omg_vremap_max_layers(int *n);
/* "LayerThicknessTarget" from layer_thickness_dev [NCellsSize][pitch] and the VertCoord's RefLayerThickness and
 * VertCoordMovementWeights.  One launch */
int omg_vremap_compute_target(omg_vremap *r, const double *layer_thickness_dev, void *stream);
/* tracers_dev [ntracers][NCellsSize][pitch] in place, from layer_thickness_dev onto "LayerThicknessTarget" as it stands.
 * Fails for ntracers outside 0 .. max_tracers.  One launch whatever ntracers (none for 0) */
int omg_vremap_remap_tracers(omg_vremap *r, const double *layer_thickness_dev, double *tracers_dev, int ntracers,
                             void *stream);
/* normal_velocity_dev [NEdgesSize][pitch] in place, between the means of the two cells' thicknesses and targets on every
 * edge's level range.  One launch */
int omg_vremap_remap_velocity(omg_vremap *r, const double *layer_thickness_dev, double *normal_velocity_dev, void *stream);
/* layer_thickness_dev = "LayerThicknessTarget" on the cells' ranges.  One launch */
int omg_vremap_adopt_target(omg_vremap *r, double *layer_thickness_dev, void *stream);
/* the four calls above in that order, in three launches, with the same bits */
int omg_vremap_remap(omg_vremap *r, double *layer_thickness_dev, double *normal_velocity_dev, double *tracers_dev,
                     int ntracers, void *stream);
/* kernel launches the five calls have issued on this object so far */
int omg_vremap_launch_count(const omg_vremap *r, int64_t *n);
/* "LayerThicknessTarget" ([NCellsSize][NVertLayers], zero at creation) */
int omg_vremap_device_ptr(const omg_vremap *r, const char *name, double **dev, size_t *n);
int omg_vremap_copy_to_device(omg_vremap *r, const char *name, const double *host, size_t n);
int omg_vremap_copy_to_host(const omg_vremap *r, const char *name, double *host, size_t n);
/* SplitExplicitStepper::attachVertRemap (omega_amd/csrc/SplitExplicitStepper.h): every step of a "Split-Explicit"
 * stepper runs omg_vremap_remap on the new time level between the velocity update and the vertical mixing (r NULL:
 * detach).  Fails for any other stepper type, an r of another mesh or layer count, max_tracers below the stepper's
 * tracer count, and while a VertAdv is attached to the Tendencies (omg_stepper_do_step checks again).  The stepper keeps
 * a pointer to r: detach before destroying it. */
int omg_stepper_attach_vert_remap(omg_stepper *st, omg_vremap *r);

/* ---- Kpp (omega_amd/csrc/Kpp.h; O/doc/design/OmegaV1GoverningEqns.md section 1 and VerticalMixingCoeff.md, design
 * only): K-profile boundary-layer mixing on top of a VertMix -- the boundary-layer depth from a bulk Richardson number,
 * the K-profile viscosity and diffusivity inside the layer over what omg_vertmix_compute wrote, and the non-local
 * redistribution of the surface tracer flux.  Level-indexed device arrays are [rows][pitch] with pitch =
 * omg_level_pitch(NVertLayers); z_interface_dev is [NCellsSize][omg_level_pitch(NVertLayers + 1)].  Every call is
 * asynchronous on stream and allocates nothing.  The object keeps pointers to v and x: destroy it before them. ---- */
typedef struct omg_kpp omg_kpp;
typedef struct omg_kpp_config {
   double VonKarman;            /* 0.4 */
   double CritBulkRichardson;   /* 0.3 */
   double SurfaceLayerFraction; /* 0.1 */
   double Cv;                   /* 1.7 */
   double EntrainmentRatio;     /* 0.2 */
   double CStar;                /* 10 */
} omg_kpp_config;
int omg_kpp_config_default(omg_kpp_config *c);
/* c NULL: the defaults.  Fails for a VonKarman or CritBulkRichardson that is not positive, a SurfaceLayerFraction
 * outside (0, 1), a negative Cv, EntrainmentRatio or CStar, a host-only mesh, a VertCoord or VertMix that is NULL or of
 * another mesh or layer count, and NVertLayers outside 1 .. 1024 */
int omg_kpp_create(const omg_mesh *m, const omg_vcoord *v, omg_vertmix *x, const omg_kpp_config *c, omg_kpp **out);
int omg_kpp_destroy(omg_kpp *k);
/* "BoundaryLayerDepth", "BoundaryLayerIndex", "BulkRichardson", "NonLocalShape" and, inside the boundary layer, the
 * VertMix's "VertDiff" / "VertVisc", from the edge velocities [NEdgesSize][pitch], the VertMix's "BruntVaisalaFreqSq",
 * the VertCoord's "ZMid" / "ZInterface" and this object's "FrictionVelocity" / "SurfaceBuoyancyFlux".  One launch */
int omg_kpp_compute(omg_kpp *k, const double *normal_velocity_dev, const double *tangential_velocity_dev, void *stream);
/* the same on the caller's cell arrays; vert_diff_dev and vert_visc_dev are rewritten inside the boundary layer only */
int omg_kpp_compute_arrays(omg_kpp *k, const double *normal_velocity_dev, const double *tangential_velocity_dev,
                           const double *bvf_dev, const double *z_mid_dev, const double *z_interface_dev,
                           double *vert_diff_dev, double *vert_visc_dev, void *stream);
/* tracers_dev [ntracers][NCellsSize][pitch] in place on owned cells: the counter-gradient part of surface_flux_dev
 * [ntracers][NCellsSize] (positive into the ocean; NULL: nothing is done) on "NonLocalShape" as it stands.  One launch */
int omg_kpp_apply_non_local(omg_kpp *k, const double *layer_thickness_dev, double *tracers_dev, int ntracers, double dt,
                            const double *surface_flux_dev, void *stream);
/* the two constants formed at creation (Kpp.h): VtCoef and NonLocalCoeff */
int omg_kpp_constants(const omg_kpp *k, double *vt_coef, double *non_local_coeff);
/* kernel launches the three calls have issued on this object so far */
int omg_kpp_launch_count(const omg_kpp *k, int64_t *n);
/* "FrictionVelocity", "SurfaceBuoyancyFlux", "BoundaryLayerDepth" ([NCellsSize]), "BulkRichardson", "NonLocalShape"
 * ([NCellsSize][NVertLayers]); all zero at creation */
int omg_kpp_device_ptr(const omg_kpp *k, const char *name, double **dev, size_t *n);
int omg_kpp_copy_to_device(omg_kpp *k, const char *name, const double *host, size_t n);
int omg_kpp_copy_to_host(const omg_kpp *k, const char *name, double *host, size_t n);
/* "BoundaryLayerIndex" ([NCellsSize] int32, zero at creation; -1 on land after a compute) */
int omg_kpp_copy_to_host_i4(const omg_kpp *k, const char *name, int32_t *host, size_t n);
int omg_kpp_copy_to_device_i4(omg_kpp *k, const char *name, const int32_t *host, size_t n);
/* VertMixStep::attachKpp (omega_amd/csrc/VertMixStep.h): omg_vertmix_step_apply runs omg_kpp_compute_arrays after the
 * coefficients and omg_kpp_apply_non_local with the step's "SurfaceTracerFlux" before the tracer solve (k NULL:
 * detach).  Fails for a k of another mesh or layer count or on another VertCoord or VertMix.  The VertMixStep keeps a
 * pointer to k: detach before destroying it. */
int omg_vmix_step_attach_kpp(omg_vertmix_step *ms, omg_kpp *k);

/* ---- Batched tridiagonal solvers (O/src/base/TriDiagSolvers.h).  Numerical contract: omega_amd/csrc/TriDiagSolvers.h.
 * nbatch systems of nrow rows (1 <= nrow <= 1024; anything else fails naming the limit), row i of every array at
 * dev + i * row_pitch (row_pitch 0: nrow).  x holds the right-hand side on entry and the solution on return; only
 * x[0:nbatch][0:nrow] is written, the coefficient arrays are left unchanged, nothing is allocated.  Asynchronous on
 * stream (NULL: the null stream). ---- */
/* ThomasSolver::solve (TriDiagSolvers.h:97-134): DL x(k-1) + D x(k) + DU x(k+1) = x */
int omg_tridiag_thomas_solve(const double *dl_dev, const double *d_dev, const double *du_dev, double *x_dev, int nbatch,
                             int nrow, int row_pitch, void *stream);
/* PCRSolver::solve (TriDiagSolvers.h:217-244) */
int omg_tridiag_pcr_solve(const double *dl_dev, const double *d_dev, const double *du_dev, double *x_dev, int nbatch,
                          int nrow, int row_pitch, void *stream);
/* ThomasDiffusionSolver::solve (TriDiagSolvers.h:324-359): -G(k-1) x(k-1) + (H(k) + G(k-1) + G(k)) x(k) - G(k) x(k+1) = x */
int omg_tridiag_thomas_diff_solve(const double *g_dev, const double *h_dev, double *x_dev, int nbatch, int nrow,
                                  int row_pitch, void *stream);
/* PCRDiffusionSolver::solve (TriDiagSolvers.h:458-483) */
int omg_tridiag_pcr_diff_solve(const double *g_dev, const double *h_dev, double *x_dev, int nbatch, int nrow,
                               int row_pitch, void *stream);

#ifdef __cplusplus
}
#endif
#endif
