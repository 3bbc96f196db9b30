// GMKernels.hip -- the eddy bolus-velocity kernel behind GentMcWilliams (GentMcWilliams.h) on gfx950.
//
// One launch, the edge geometry of the implicit vertical-mixing solves (kernels/VertMixKernels.hip): lanes along the
// layers of an edge column (layer Lo + I on lane I) in the packed-column shape (kernels/PackedColumns.h).  A lane reads
// its layer of the two cells once -- SpecVol, SpecVolDisplaced, ZMid, thickness: coalesced along the levels -- and hands
// the seven values the interface below it needs (the six of PackedColumns.h's edge layer and the edge thickness) to the
// next lane through LDS: no row is fetched from HBM twice by one column.  Lane I >= 1 then holds row I - 1 of the
// column's system (the interface at the top of its layer, edgeInterface of PackedColumns.h, which the slope kernel of
// kernels/RediKernels.hip shares) in registers and solves it with pcrDiffSolveRowRagged (kernels/TriDiagKernels.h),
// which lets columns of different depth share a workgroup; G, H and X go through the levels together, one barrier per
// level (the multi-right-hand-side body takes two).  The exchange area and the solver's workspace are the same LDS (7
// and 6 arrays of one double per lane); the stream function goes through it once more, to the lane above, for the
// vertical difference.  No scratch, no global atomics; the column tile of LevelTile.h (lanes along the columns) does
// not fit a solve that has its rows on the lanes.
#include "GMKernels.h"

namespace OMEGA {

namespace {

constexpr int GMArrays = EdgeLayerArrays + 1; // LDS doubles per lane: the exchange and HE cover the solver's workspace (2 x 3)

__global__ void __launch_bounds__(TriDiagMaxRows) bolusVelocityKernel(GMArgs A, int Pitch, PackedShape P) {
   extern __shared__ Real Lds[];
   const int T        = threadIdx.x;
   const PackedLane L = packedLane(P, A.K, A.NEdgesAll);
   const int I = L.I, Rows = P.Rows; // layer I of the column: level E.Lo + I
   const long Col     = L.Col;
   const EdgeColumn E = edgeColumn(A, L);
   const int N        = E.N;
   const int NLevWg   = packedLevels(L.InSys && I == 0, N - 1);
   const bool Act     = L.InSys && I < N;
   const int Lev      = E.Lo + I;

   // ---- this lane's layer of the two cells, and what the interface below it needs of it
   EdgeLayer V;
   Real HE = 1;
   if (Act) {
      const size_t C0 = (size_t)E.C0 * Pitch + Lev, C1 = (size_t)E.C1 * Pitch + Lev;
      HE = 0.5 * (A.LayerThickness[C0] + A.LayerThickness[C1]); // (first: not behind the branch on the bottom layer)
      V  = loadEdgeLayer(A, Col, C0, C1, I == N - 1);
      storeEdgeLayer(V, Lds, Rows, T);
      Lds[EdgeLayerArrays * Rows + T] = HE;
   }
   __syncthreads();

   // ---- row I - 1 of the system: the interface between layer Lev - 1 (the lane above) and layer Lev
   const bool Row = Act && I >= 1;
   const int NRow = N - 1, R = I - 1;
   Real G = 0, H = 1, X = 0;
   if (Row) {
      const Real GR         = A.GOverRho0;
      const EdgeInterface F = edgeInterface(V, Lds, Rows, T - 1, GR);
      const Real HEu        = Lds[EdgeLayerArrays * Rows + T - 1];
      const Real DzMid      = 0.5 * (HEu + HE);
      G = R < NRow - 1 ? A.C2 / HE : 0.0;
      H = F.N2E * DzMid;
      if (R == 0)
         H = H + A.C2 / HEu;
      if (R == NRow - 1)
         H = H + A.C2 / HE;
      X = DzMid * ((A.Kappa[Col] * GR) * F.GradRhoZ);
   }
   __syncthreads(); // the exchange has been read: the solver takes the LDS over

   Real Psi = pcrDiffSolveRowRagged(Row, R, NRow, NLevWg, G, H, X, Lds + L.S * A.K, Rows);
   if (!Row)
      Psi = 0; // the surface, and the lanes without a layer
   __syncthreads(); // the solver's last step has read its workspace

   // ---- u* = -(d Psi / dz) over the layer: the interface below is the next lane's
   if (Act)
      Lds[T] = Psi; // 0 on lane 0: the surface
   __syncthreads();
   if (Act) {
      const Real Top = I == 0 ? 0.0 : Psi;
      const Real Bot = I == N - 1 ? 0.0 : Lds[T + 1];
      const Real Ub  = (Bot - Top) / HE;
      const size_t Pe = (size_t)Col * Pitch + Lev;
      A.StreamFunction[Pe] = Top;
      A.BolusVelocity[Pe]  = Ub;
      if (A.Transport != nullptr)
         A.Transport[Pe] = A.Transport[Pe] + Ub;
   }
}

} // namespace

void launchBolusVelocity(const GMArgs &A, hipStream_t S) {
   requirePackedLayers("GentMcWilliams", A.K);
   if (A.NEdgesAll <= 0)
      return;
   const PackedShape P(A.K);
   const size_t Bytes = (size_t)GMArrays * P.Rows * sizeof(Real);
   hipLaunchKernelGGL(bolusVelocityKernel, P.grid(A.NEdgesAll), dim3(P.Threads), Bytes, S, A, levelPitch(A.K), P);
   HIP_CHECK(hipGetLastError());
}

} // namespace OMEGA
