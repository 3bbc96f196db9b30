// RediKernels.hip -- the three kernels behind Redi (Redi.h) on gfx950.
//
// Launch 1, the slope: the edge-column geometry of the bolus-velocity kernel (kernels/GMKernels.hip) without its solve
// -- lanes along the layers of an edge column (layer Lo + I on lane I) in the packed-column shape, and the edge layer
// and edge interface of kernels/PackedColumns.h, which both kernels use.  A lane reads its layer of the two cells once
// (SpecVol, SpecVolDisplaced, ZMid: coalesced along the levels) and hands the six values the interface below it needs
// -- the two densities, the two heights, the two displaced densities -- to the next lane through LDS; lane I >= 1 then
// forms the slope of the interface at the top of its layer in registers and stores it.  One barrier, no solve, one
// array written.
//
// Launches 2 and 3, the tracer tendency and the S.S diffusivity: gather stencils over cells with the levels innermost.
// A workgroup owns a tile of cells; its lanes run along the levels of a cell (LanesK = the power of two that holds
// min(K, 16): one 128-byte line of a row, the tile kernels' choice; longer columns are walked in strides of 16, which
// the row pitch is a multiple of) and along the cells of the tile (RediTileCells at most, 256 lanes at most).  The tile's connectivity is staged in LDS once, one lane per (cell, slot): the edge, its two cells,
// its level range, and the per-slot factors of the contract (InvDc, Kappa, Dv, the sign, F_J), so that the level loop
// reads no mesh table.  Level K's stencil takes K - 1 and K + 1 of the same rows: those are the adjacent lanes' own
// levels, fetched by the same wave from the same cache lines, so a row comes from HBM once per tile that touches it.
// The tracers go through in pairs (the slot loop's geometry, thickness and slopes are formed once per pair) with a
// single-tracer pass for an odd count: the accumulators have compile-time indices, nothing is indexed at run time.
// Tiles are dealt out through xcdRemap so that neighbouring tiles share an XCD's L2.  No scratch, no global atomics,
// no grid-wide synchronisation.
#include "RediKernels.h"
#include "KernelCommon.h"

namespace OMEGA {

namespace {

constexpr int RediTileCells = 32;  // most cells per workgroup of the cell launches
constexpr int RediMaxLanesK = 16;  // most lanes along one cell's levels: one 128-byte line of a row

__global__ void __launch_bounds__(TriDiagMaxRows) rediSlopeKernel(RediSlopeArgs A, int Pitch, PackedShape P) {
   extern __shared__ Real Lds[];
   const int T        = threadIdx.x;
   const PackedLane L = packedLane(P, A.K, A.NEdgesAll);
   const EdgeColumn E = edgeColumn(A, L);
   const bool Act     = L.InSys && L.I < E.N;
   const int Lev      = E.Lo + L.I;

   // ---- this lane's layer of the two cells, and what the interface below it needs of it
   EdgeLayer V;
   if (Act) {
      V = loadEdgeLayer(A, L.Col, (size_t)E.C0 * Pitch + Lev, (size_t)E.C1 * Pitch + Lev, L.I == E.N - 1);
      storeEdgeLayer(V, Lds, P.Rows, T);
   }
   __syncthreads();
   if (!Act)
      return;

   // ---- the interface between layer Lev - 1 (the lane above) and layer Lev
   Real Slope = 0.0; // the surface of the column
   if (L.I >= 1) {
      const Real GR         = A.GOverRho0;
      const EdgeInterface F = edgeInterface(V, Lds, P.Rows, T - 1, GR);
      const Real Den        = F.N2E < A.N2Floor ? A.N2Floor : F.N2E;
      const Real SIso       = (GR * F.GradRhoZ) / Den;
      Real SRel             = SIso - F.GradZE;
      SRel                  = SRel > A.SlopeMax ? A.SlopeMax : SRel;
      SRel                  = SRel < -A.SlopeMax ? -A.SlopeMax : SRel;
      Slope                 = SRel;
   }
   A.SlopeInterface[(size_t)L.Col * Pitch + Lev] = Slope;
}

/// What the cell launches keep in LDS per (cell of the tile, slot): carved from the dynamic LDS, doubles first
struct RediTileLds {
   Real *InvDc, *Kappa, *Dv, *Sign, *F; ///< [Tile * MaxEdges]
   Real *InvArea;                       ///< [Tile]
   int *Edge, *C0, *C1, *Lo, *Hi;       ///< [Tile * MaxEdges]; an unused or invalid slot has the empty range [K, -1]
   int *KMin, *KMax;                    ///< [Tile]; a cell without layers has the empty range [K, -1]
};
__host__ __device__ inline size_t rediTileBytes(int Tile, int MaxEdges) {
   return ((size_t)5 * Tile * MaxEdges + Tile) * sizeof(Real) + ((size_t)5 * Tile * MaxEdges + 2 * Tile) * sizeof(int);
}
__device__ inline RediTileLds rediCarve(void *Base, int Tile, int MaxEdges) {
   RediTileLds L;
   const int TM = Tile * MaxEdges;
   Real *R      = reinterpret_cast<Real *>(Base);
   L.InvDc = R, L.Kappa = R + TM, L.Dv = R + 2 * TM, L.Sign = R + 3 * TM, L.F = R + 4 * TM, L.InvArea = R + 5 * TM;
   int *Q = reinterpret_cast<int *>(R + 5 * TM + Tile);
   L.Edge = Q, L.C0 = Q + TM, L.C1 = Q + 2 * TM, L.Lo = Q + 3 * TM, L.Hi = Q + 4 * TM, L.KMin = Q + 5 * TM;
   L.KMax = Q + 5 * TM + Tile;
   return L;
}

/// Stage the connectivity of the Cnt cells from cell First, one lane per (cell, slot); ends with the one barrier
__device__ inline void rediStage(const RediCellArgs &A, const RediTileLds &L, int First, int Cnt, int Tid, int NThr) {
   const int ME = A.MaxEdges;
   for (int Idx = Tid; Idx < Cnt * ME; Idx += NThr) {
      const int Lc = Idx / ME, J = Idx - Lc * ME;
      const int C  = First + Lc;
      int E = 0, C0 = 0, C1 = 0, Lo = A.K, Hi = -1;
      Real InvDc = 0, Kap = 0, Dv = 0, Sg = 0, F = 0;
      if (J < A.NEdgesOnCell[C]) {
         E = A.EdgesOnCell[(size_t)C * ME + J];
         if (E >= 0 && E < A.NEdgesAll) {
            C0 = A.CellsOnEdge[2 * (size_t)E], C1 = A.CellsOnEdge[2 * (size_t)E + 1];
            const int El = A.MinLayerEdgeBot[E], Eh = A.MaxLayerEdgeTop[E];
            if (El >= 0 && El <= Eh && Eh < A.K && C0 >= 0 && C0 < A.NCellsSize && C1 >= 0 && C1 < A.NCellsSize) {
               Lo = El, Hi = Eh;
               const Real Dc = A.DcEdge[E];
               Dv            = A.DvEdge[E];
               InvDc         = 1.0 / Dc;
               Kap           = A.Kappa[E];
               Sg            = A.EdgeSignOnCell[(size_t)C * ME + J];
               F             = ((0.5 * Dc) * Dv) * (1.0 / A.AreaCell[C]);
            } else {
               E = 0, C0 = 0, C1 = 0;
            }
         } else {
            E = 0;
         }
      }
      L.Edge[Idx] = E, L.C0[Idx] = C0, L.C1[Idx] = C1, L.Lo[Idx] = Lo, L.Hi[Idx] = Hi;
      L.InvDc[Idx] = InvDc, L.Kappa[Idx] = Kap, L.Dv[Idx] = Dv, L.Sign[Idx] = Sg, L.F[Idx] = F;
   }
   for (int Lc = Tid; Lc < Cnt; Lc += NThr) {
      const int C  = First + Lc;
      const int Kl = A.MinLayerCell[C], Kh = A.MaxLayerCell[C];
      const bool Ok = Kl >= 0 && Kl <= Kh && Kh < A.K;
      L.KMin[Lc]    = Ok ? Kl : A.K;
      L.KMax[Lc]    = Ok ? Kh : -1;
      L.InvArea[Lc] = 1.0 / A.AreaCell[C];
   }
   __syncthreads();
}

/// NB tracers from tracer L0 of cell C (tile-local Lc), layer K: the slot loop of the contract
template <int NB>
__device__ __forceinline__ void rediTendPass(const RediCellArgs &A, const RediTileLds &L, int Pitch, int Lc, int C, int K,
                                             int L0) {
   const int ME       = A.MaxEdges;
   const size_t TrPl  = (size_t)A.TrRows * Pitch;
   const Real *Phi    = A.Tracers + (size_t)L0 * TrPl;
   Real Acc[NB], WTop[NB], WBot[NB];
#pragma unroll
   for (int B = 0; B < NB; ++B)
      Acc[B] = 0.0, WTop[B] = 0.0, WBot[B] = 0.0;
   for (int J = 0; J < ME; ++J) {
      const int Sl = Lc * ME + J;
      const int Lo = L.Lo[Sl], Hi = L.Hi[Sl];
      if (K < Lo || K > Hi)
         continue;
      const size_t P0 = (size_t)L.C0[Sl] * Pitch + K, P1 = (size_t)L.C1[Sl] * Pitch + K;
      const size_t Pe = (size_t)L.Edge[Sl] * Pitch + K;
      const Real InvDc = L.InvDc[Sl], Kap = L.Kappa[Sl], Dv = L.Dv[Sl], Sg = L.Sign[Sl], F = L.F[Sl];
      const bool HasUp = K > Lo, HasDn = K < Hi;
      const Real HE    = 0.5 * (A.LayerThickness[P0] + A.LayerThickness[P1]);
      const Real Z0 = A.ZMid[P0], Z1 = A.ZMid[P1];
      Real DzU0 = 1, DzU1 = 1, DzD0 = 1, DzD1 = 1, SUp = 0, SDn = 0;
      if (HasUp) {
         DzU0 = A.ZMid[P0 - 1] - Z0, DzU1 = A.ZMid[P1 - 1] - Z1;
         SUp  = A.SlopeInterface[Pe];
      }
      if (HasDn) {
         DzD0 = Z0 - A.ZMid[P0 + 1], DzD1 = Z1 - A.ZMid[P1 + 1];
         SDn  = A.SlopeInterface[Pe + 1];
      }
#pragma unroll
      for (int B = 0; B < NB; ++B) {
         const Real *Ph   = Phi + (size_t)B * TrPl;
         const Real Ph0 = Ph[P0], Ph1 = Ph[P1];
         const Real Grad  = (Ph1 - Ph0) * InvDc;
         Real Up = 0.0, Dn = 0.0;
         if (HasUp) {
            const Real Pu0 = Ph[P0 - 1], Pu1 = Ph[P1 - 1];
            const Real PhiZ0 = (Pu0 - Ph0) / DzU0, PhiZ1 = (Pu1 - Ph1) / DzU1;
            const Real PhiZE = 0.5 * (PhiZ0 + PhiZ1);
            const Real GradU = (Pu1 - Pu0) * InvDc;
            const Real GInt  = 0.5 * (GradU + Grad);
            Up               = SUp * PhiZE;
            WTop[B]          = WTop[B] + F * ((Kap * SUp) * GInt);
         }
         if (HasDn) {
            const Real Pd0 = Ph[P0 + 1], Pd1 = Ph[P1 + 1];
            const Real PhiZ0 = (Ph0 - Pd0) / DzD0, PhiZ1 = (Ph1 - Pd1) / DzD1;
            const Real PhiZE = 0.5 * (PhiZ0 + PhiZ1);
            const Real GradD = (Pd1 - Pd0) * InvDc;
            const Real GInt  = 0.5 * (Grad + GradD);
            Dn               = SDn * PhiZE;
            WBot[B]          = WBot[B] + F * ((Kap * SDn) * GInt);
         }
         const Real FluxE = (Kap * HE) * (Grad + 0.5 * (Up + Dn));
         Acc[B]           = Acc[B] - Sg * (Dv * FluxE);
      }
   }
   const Real InvA   = L.InvArea[Lc];
   const size_t TdPl = (size_t)A.TendRows * Pitch;
#pragma unroll
   for (int B = 0; B < NB; ++B) {
      Real *Td = A.Tend + (size_t)(L0 + B) * TdPl + (size_t)C * Pitch + K;
      *Td      = *Td + (Acc[B] * InvA + (WTop[B] - WBot[B]));
   }
}

__global__ void __launch_bounds__(256) rediTracerTendKernel(RediCellArgs A, int Pitch, int LanesK, int Tile, int NTiles) {
   extern __shared__ __align__(16) unsigned char RediLds[];
   const RediTileLds L = rediCarve(RediLds, Tile, A.MaxEdges);
   const int Tid       = threadIdx.x;
   const int First     = xcdRemap(blockIdx.x, NTiles) * Tile;
   int Cnt             = A.NCellsAll - First;
   Cnt                 = Cnt > Tile ? Tile : Cnt;
   rediStage(A, L, First, Cnt, Tid, blockDim.x);
   const int Lc = Tid / LanesK, Kl = Tid - Lc * LanesK;
   if (Lc >= Cnt)
      return;
   const int C = First + Lc;
   const int KMin = L.KMin[Lc], KMax = L.KMax[Lc];
   for (int K = Kl; K <= KMax; K += LanesK) {
      if (K < KMin)
         continue;
      int L0 = 0;
      for (; L0 + 2 <= A.NTracers; L0 += 2)
         rediTendPass<2>(A, L, Pitch, Lc, C, K, L0);
      if (L0 < A.NTracers)
         rediTendPass<1>(A, L, Pitch, Lc, C, K, L0);
   }
}

__global__ void __launch_bounds__(256) rediVertDiffKernel(RediCellArgs A, int Pitch, int LanesK, int Tile, int NTiles) {
   extern __shared__ __align__(16) unsigned char RediLds[];
   const RediTileLds L = rediCarve(RediLds, Tile, A.MaxEdges);
   const int Tid       = threadIdx.x;
   const int First     = xcdRemap(blockIdx.x, NTiles) * Tile;
   int Cnt             = A.NCellsAll - First;
   Cnt                 = Cnt > Tile ? Tile : Cnt;
   rediStage(A, L, First, Cnt, Tid, blockDim.x);
   const int Lc = Tid / LanesK, Kl = Tid - Lc * LanesK;
   if (Lc >= Cnt)
      return;
   const int C  = First + Lc;
   const int ME = A.MaxEdges;
   const int KMin = L.KMin[Lc], KMax = L.KMax[Lc];
   for (int K = Kl; K <= KMax; K += LanesK) {
      if (K <= KMin) // interfaces KMin + 1 .. KMax
         continue;
      Real D = 0.0;
      for (int J = 0; J < ME; ++J) {
         const int Sl = Lc * ME + J;
         if (K <= L.Lo[Sl] || K > L.Hi[Sl])
            continue;
         const Real Sv = A.SlopeInterface[(size_t)L.Edge[Sl] * Pitch + K];
         D             = D + L.F[Sl] * (L.Kappa[Sl] * (Sv * Sv));
      }
      const size_t P       = (size_t)C * Pitch + K;
      A.VertDiffusivity[P] = D;
      if (A.VertDiff != nullptr)
         A.VertDiff[P] = A.VertDiff[P] + D;
   }
}

/// The shape of a cell launch: lanes along the levels, cells per workgroup, workgroups
struct RediCellShape {
   int LanesK, Tile, Threads, NTiles;
};
inline RediCellShape rediCellShape(int NCellsAll, int K) {
   RediCellShape G;
   G.LanesK = 1;
   while (G.LanesK < K && G.LanesK < RediMaxLanesK)
      G.LanesK *= 2;
   G.Tile    = 256 / G.LanesK < RediTileCells ? 256 / G.LanesK : RediTileCells;
   G.Threads = G.Tile * G.LanesK;
   G.NTiles  = (NCellsAll + G.Tile - 1) / G.Tile;
   return G;
}

void requireRediLayers(int K) { requirePackedLayers("Redi", K); }

} // namespace

void launchRediSlope(const RediSlopeArgs &A, hipStream_t S) {
   requireRediLayers(A.K);
   if (A.NEdgesAll <= 0)
      return;
   const PackedShape P(A.K);
   const size_t Bytes = (size_t)EdgeLayerArrays * P.Rows * sizeof(Real);
   hipLaunchKernelGGL(rediSlopeKernel, P.grid(A.NEdgesAll), dim3(P.Threads), Bytes, S, A, levelPitch(A.K), P);
   HIP_CHECK(hipGetLastError());
}

void launchRediTracerTend(const RediCellArgs &A, hipStream_t S) {
   requireRediLayers(A.K);
   if (A.NCellsAll <= 0 || A.NTracers <= 0)
      return;
   const RediCellShape G = rediCellShape(A.NCellsAll, A.K);
   hipLaunchKernelGGL(rediTracerTendKernel, dim3(G.NTiles), dim3(G.Threads), rediTileBytes(G.Tile, A.MaxEdges), S, A,
                      levelPitch(A.K), G.LanesK, G.Tile, G.NTiles);
   HIP_CHECK(hipGetLastError());
}

void launchRediVertDiffusivity(const RediCellArgs &A, hipStream_t S) {
   requireRediLayers(A.K);
   if (A.NCellsAll <= 0)
      return;
   const RediCellShape G = rediCellShape(A.NCellsAll, A.K);
   hipLaunchKernelGGL(rediVertDiffKernel, dim3(G.NTiles), dim3(G.Threads), rediTileBytes(G.Tile, A.MaxEdges), S, A,
                      levelPitch(A.K), G.LanesK, G.Tile, G.NTiles);
   HIP_CHECK(hipGetLastError());
}

} // namespace OMEGA
