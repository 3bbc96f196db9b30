// BarotropicKernels.hip -- the kernels behind BarotropicMode (BarotropicMode.h) on gfx950.
//
// Column launch: the column tile of LevelTile.h, over edges and / or over cells -- the first NEdgeTiles workgroups of a
// launch own `Tile` consecutive edges each, the others `Tile` consecutive cells, so splitVelocity and computeSSH can
// share one launch (the two halves touch no common output: the bits are those of the two launches).
//   edges: the edge field's tile is one contiguous run, staged with loadTile; the thickness rows of the two cells of
//          every edge are read with the lanes along the levels (forLevelRuns: one 16-byte load per lane and row where
//          the pitch is even) and their mean goes to LDS; one lane per edge then runs the two ascending sums out of LDS
//          (odd LDS pitch: distinct banks); the baroclinic remainder is written back with the lanes along the flat run
//          (store2).  Per edge-level: h read twice, the field once, BclVelocity written once.
//   cells: the thickness tile staged with loadTile, one lane per column sums it.
// Level-row launch (recombine, transportVelocity, advanceVelocity): the level-row tile over edges, one lane per level
// pair; one kernel body, the operation a template parameter.  Recombine visits the runs that overlap the ranges; the
// other two visit every run below level K, and read the old velocity only where a run leaves its range.
//
// Sub-step launches (2-D): one thread per cell, then one thread per edge.  All per-(element, slot) tables are
// slot-major, so consecutive lanes read consecutive table entries; what is gathered are the 8-byte field values.  The
// cell kernel recomputes the flux of its own edges from the old fields (no third launch, no flux array between the
// launches); the edge kernel owns the flux sum.  Both read the old buffers and write the other ones: the sub-steps are
// ordered by the stream alone.
//
// No atomics, no scratch, no waiting on another workgroup anywhere.
#include "BarotropicKernels.h"
#include "LevelTile.h"

namespace OMEGA {

namespace {

static_assert(RowBlock == ColThreads, "the column launch walks thickness rows with forLevelRuns");

// ---------------------------------------------------------------------------------------------------- column launch
/// doubles of LDS for a tile of T edges: the edge field, the edge thickness, and per edge the mean, the level range
/// and the two cells (4 ints).  The cell half needs one of the level buffers and the ranges only.
inline size_t btrLdsDoubles(int T, int LP) { return (size_t)T * (2 * (size_t)LP + 3); }

template <class T, int Mode, bool Cells>
__global__ void __launch_bounds__(ColThreads) btrColumnKernel(BtrColumnArgs A, int P, int Tile, int NEdgeTiles) {
   extern __shared__ Real Lds[];
   const int K = A.K, LP = ldsPitch(P);
   Real *LU = Lds, *LH = LU + Tile * LP, *LB = LH + Tile * LP;
   I4 *Lo = reinterpret_cast<I4 *>(LB + Tile), *Hi = Lo + Tile, *Cell0 = Hi + Tile, *Cell1 = Cell0 + Tile;
   const int Tid = threadIdx.x;

   if (Mode != BtrEdgeNone && (int)blockIdx.x < NEdgeTiles) {
      const int E0 = blockIdx.x * Tile;
      const int Ne = min(Tile, A.NEdgesAll - E0);
      if (Tid < Ne) {
         const int E  = E0 + Tid;
         const int C0 = A.CellsOnEdge[2 * (size_t)E], C1 = A.CellsOnEdge[2 * (size_t)E + 1];
         int L = A.MinLayerEdgeBot[E], H = A.MaxLayerEdgeTop[E];
         // an invalid range, or (never with ranges derived from the cells') a cell that is no row: the empty range
         if (!(L >= 0 && L <= H && H < K) || C0 < 0 || C0 >= A.NCellsSize || C1 < 0 || C1 >= A.NCellsSize)
            L = 1, H = -1;
         Lo[Tid] = L, Hi[Tid] = H, Cell0[Tid] = C0, Cell1[Tid] = C1;
      }
      __syncthreads();
      const InRange Active{Lo, Hi};
      loadTile(A.EdgeField, P, E0, Ne, LU, LP, Active);
      forLevelRuns<T>(Ne, P, Lo, Hi, [&](int Le, int K0, int, int) {
         const T H0 = *reinterpret_cast<const T *>(A.LayerThick + (size_t)Cell0[Le] * P + K0);
         const T H1 = *reinterpret_cast<const T *>(A.LayerThick + (size_t)Cell1[Le] * P + K0);
#pragma unroll
         for (int J = 0; J < VecW<T>::W; ++J)
            LH[Le * LP + K0 + J] = 0.5 * (getc(H0, J) + getc(H1, J));
      });
      __syncthreads();
      if (Tid < Ne) {
         const int L = Lo[Tid], H = Hi[Tid];
         const Real *HE = LH + Tid * LP, *U = LU + Tid * LP;
         Real Sum = 0.0, SumHU = 0.0, Mean = 0.0;
         if (L <= H) {
            for (int Kk = L; Kk <= H; ++Kk) {
               Sum   = Sum + HE[Kk];
               SumHU = SumHU + HE[Kk] * U[Kk];
            }
            Mean = L == H ? U[L] : SumHU / Sum; // (the mean of one level is that level, not (hE*u)/hE)
         }
         if (Mode == BtrEdgeSplit)
            A.BtrThickEdge[E0 + Tid] = Sum;
         A.BtrOut[E0 + Tid] = Mean;
         LB[Tid]            = Mean;
      }
      if (Mode == BtrEdgeSplit) {
         __syncthreads();
         Real *G = A.BclVelocity + (size_t)E0 * P;
         forPairs(Ne * P, [&](int I, bool Two) {
            const Pos2 Q(I, P);
            const bool W0 = Active(Q.C0, Q.K0), W1 = Two && Active(Q.C1, Q.K1);
            store2(G + I, W0, W1, W0 ? LU[Q.C0 * LP + Q.K0] - LB[Q.C0] : 0.0, W1 ? LU[Q.C1 * LP + Q.K1] - LB[Q.C1] : 0.0);
         });
      }
      return;
   }

   if (Cells) {
      const int C0 = ((int)blockIdx.x - NEdgeTiles) * Tile;
      const int Nc = min(Tile, A.NCellsAll - C0);
      stageRanges(A.MinLayerCell, A.MaxLayerCell, C0, Nc, K, Lo, Hi);
      loadTile(A.LayerThick, P, C0, Nc, LH, LP, AllLevels());
      __syncthreads();
      if (Tid < Nc && Lo[Tid] <= Hi[Tid]) {
         const Real *Hc = LH + Tid * LP;
         Real Sum       = 0.0;
         for (int Kk = Lo[Tid]; Kk <= Hi[Tid]; ++Kk)
            Sum = Sum + Hc[Kk];
         A.SSH[C0 + Tid] = Sum - A.BottomDepth[C0 + Tid];
      }
   }
}

// ------------------------------------------------------------------------------------------------ level-row launch
template <class T, int Op> __global__ void __launch_bounds__(RowBlock) btrLevelKernel(BtrLevelArgs A, int Pitch) {
   __shared__ int Lo[RowTile], Hi[RowTile], VisLo[RowTile], VisHi[RowTile];
   __shared__ Real Btr[RowTile], Mean[RowTile];
   constexpr int W = VecW<T>::W;
   const int First = blockIdx.x * RowTile;
   int Cnt         = A.NEdgesAll - First;
   if (Cnt > RowTile)
      Cnt = RowTile;
   stageRanges(A.MinLayerEdgeBot, A.MaxLayerEdgeTop, First, Cnt, A.K, Lo, Hi);
   if ((int)threadIdx.x < Cnt) {
      const int Le = threadIdx.x, E = First + Le;
      // the runs to visit: recombine those of the range, the others every run that holds a level below K
      VisLo[Le] = Op == BtrLevelRecombine ? Lo[Le] : 0;
      VisHi[Le] = Op == BtrLevelRecombine ? Hi[Le] : A.K - 1;
      // (an empty range has BtrThickEdge 0: the quotient is then never used)
      Btr[Le] = Op == BtrLevelTransport ? A.BtrFluxMean[E] / A.BtrThickEdge[E] : A.BtrVelocity[E];
      if (Op == BtrLevelAdvance)
         Mean[Le] = A.BtrTendMean[E];
   }
   __syncthreads();
   forLevelRuns<T>(Cnt, Pitch, VisLo, VisHi, [&](int Le, int K0, int, int KLast) {
      const int L = Lo[Le], H = Hi[Le];
      const size_t R  = (size_t)(First + Le) * Pitch + K0;
      const bool Some = K0 + W - 1 >= L && K0 <= H, All = K0 >= L && K0 + W - 1 <= H;
      T Bc = T(), Old = T(), Td = T(), Res;
      if (Some)
         Bc = *reinterpret_cast<const T *>(A.BclVelocity + R);
      if (Op == BtrLevelAdvance)
         Td = *reinterpret_cast<const T *>(A.VelTend + R);
      if (Op != BtrLevelRecombine && !All)
         Old = *reinterpret_cast<const T *>(A.VelOld + R);
#pragma unroll
      for (int J = 0; J < W; ++J) {
         const bool In = K0 + J >= L && K0 + J <= H;
         if (Op == BtrLevelAdvance)
            setc(Res, J, In ? (getc(Bc, J) + A.Dt * (getc(Td, J) - Mean[Le])) + Btr[Le] : getc(Old, J) + A.Dt * getc(Td, J));
         else
            setc(Res, J, In ? getc(Bc, J) + Btr[Le] : getc(Old, J));
      }
      // (recombine: KLast = H and the run overlaps [L, H]; the others: every level 0 .. K - 1 of the run)
      storeRanged<T>(A.VelOut + R, Res, K0, Op == BtrLevelRecombine ? L : 0, KLast);
   });
}

// -------------------------------------------------------------------------------------------------------- sub-steps
constexpr int SubThreads = 256;

__global__ void __launch_bounds__(SubThreads) btrCellKernel(BtrSubArgs A) {
   const int C = blockIdx.x * SubThreads + threadIdx.x;
   if (C >= A.NCellsAll)
      return;
   const size_t NC  = (size_t)A.NCellsAll;
   const Real Eta   = A.SSH[C];
   const Real Depth = Eta + A.BottomDepth[C];
   const Real InvA  = A.InvAreaCell[C];
   const int N      = min(A.NEdgesOnCell[C], A.MaxEdges);
   Real Div         = 0.0;
   for (int J = 0; J < N; ++J) {
      const int E = A.EdgeSlot[J * NC + C], Nb = A.NbrSlot[J * NC + C];
      Real F      = 0.0;
      // (the sum of the two depths commutes: the edge kernel adds its first cell first; EdgeMask is 1.0 here, and the
      // product with it exact)
      if (Nb >= 0)
         F = (0.5 * (Depth + (A.SSH[Nb] + A.BottomDepth[Nb]))) * A.Vel[E];
      Div = Div - (A.DvSignSlot[J * NC + C] * F) * InvA;
   }
   A.SSHNew[C] = Eta - A.Dt * Div;
}

/// Cor - Gravity*((Eta[c1] - Eta[c0])*InvDcEdge[e]) of edge E with the cells Cc, the Coriolis sum over the slots of E in
/// slot order from A.Vel (holes skipped): the bracket of a sub-step (Eta = SSHNew) and of the residual forcing (Eta = SSH)
__device__ inline Real btrBracket(const BtrSubArgs &A, int E, int2 Cc, const Real *Eta) {
   const size_t NE = (size_t)A.NEdgesAll;
   const int N     = min(A.NEdgesOnEdge[E], A.MaxEdges2);
   Real Cor        = 0.0;
   for (int J = 0; J < N; ++J) {
      const int Ej = A.EoESlot[J * NE + E];
      if (Ej >= 0)
         Cor = Cor + A.CorSlot[J * NE + E] * A.Vel[Ej];
   }
   return Cor - A.Gravity * ((Eta[Cc.y] - Eta[Cc.x]) * A.InvDcEdge[E]);
}

__device__ inline bool btrOpenEdge(const BtrSubArgs &A, Real M, int2 Cc) {
   return M != 0.0 && Cc.x >= 0 && Cc.x < A.NCellsAll && Cc.y >= 0 && Cc.y < A.NCellsAll;
}

__global__ void __launch_bounds__(SubThreads) btrEdgeKernel(BtrSubArgs A) {
   const int E = blockIdx.x * SubThreads + threadIdx.x;
   if (E >= A.NEdgesAll)
      return;
   const Real U  = A.Vel[E];
   const Real M  = A.EdgeMask[E];
   const int2 Cc = *reinterpret_cast<const int2 *>(A.CellsOnEdge + 2 * (size_t)E);
   Real F = 0.0, Un = U;
   if (btrOpenEdge(A, M, Cc)) {
      F  = M * ((0.5 * ((A.SSH[Cc.x] + A.BottomDepth[Cc.x]) + (A.SSH[Cc.y] + A.BottomDepth[Cc.y]))) * U);
      Un = U + A.Dt * (M * (btrBracket(A, E, Cc, A.SSHNew) + A.Forcing[E]));
   }
   A.FluxSum[E] = A.FluxSum[E] + F;
   A.VelNew[E]  = Un;
}

__global__ void __launch_bounds__(SubThreads) btrResidualKernel(BtrSubArgs A, const Real *TendMean, Real *Forcing) {
   const int E = blockIdx.x * SubThreads + threadIdx.x;
   if (E >= A.NEdgesAll)
      return;
   const Real M  = A.EdgeMask[E];
   const int2 Cc = *reinterpret_cast<const int2 *>(A.CellsOnEdge + 2 * (size_t)E);
   Real G        = TendMean[E];
   if (btrOpenEdge(A, M, Cc))
      G = G - M * btrBracket(A, E, Cc, A.SSH);
   Forcing[E] = G;
}

__global__ void __launch_bounds__(SubThreads) btrDivideKernel(Real *X, int N, Real Div) {
   const int I = blockIdx.x * SubThreads + threadIdx.x;
   if (I < N)
      X[I] = X[I] / Div;
}

template <int Mode, bool Cells> void columnLaunchAs(const BtrColumnArgs &A, int P, int Tile, int NEdgeTiles, int NTiles,
                                                    size_t Bytes, hipStream_t S) {
   withLaneType(P, [&](auto Lane) {
      hipLaunchKernelGGL((btrColumnKernel<decltype(Lane), Mode, Cells>), dim3(NTiles), dim3(ColThreads), Bytes, S, A, P,
                         Tile, NEdgeTiles);
   });
}

} // namespace

int btrColumnTile(int K) {
   const int LP = ldsPitch(levelPitch(K));
   return pickColumnTile([&](int T) { return btrLdsDoubles(T, LP); });
}

void launchBtrColumn(const BtrColumnArgs &A, BtrEdgeMode Edges, bool Cells, hipStream_t S) {
   if (A.K <= 0)
      return;
   const bool Forcing = Edges == BtrEdgeForcing || Edges == BtrEdgeTendMean; // one kernel: A.BtrOut tells them apart
   OMEGA_REQUIRE(!(Forcing && Cells),
                 "BarotropicMode column kernel: the forcing sweep has no cell half (only the split shares its launch)");
   const int Tile = btrColumnTile(A.K);
   OMEGA_REQUIRE(Tile >= 2,
                 "BarotropicMode column kernel: NVertLayers " + std::to_string(A.K) + " is too long for the LDS tile");
   const int P          = levelPitch(A.K);
   const size_t Bytes   = btrLdsDoubles(Tile, ldsPitch(P)) * sizeof(Real);
   const int NEdgeTiles = Edges != BtrEdgeNone && A.NEdgesAll > 0 ? (A.NEdgesAll + Tile - 1) / Tile : 0;
   const int NCellTiles = Cells && A.NCellsAll > 0 ? (A.NCellsAll + Tile - 1) / Tile : 0;
   const int NTiles     = NEdgeTiles + NCellTiles;
   if (NTiles == 0)
      return;
   if (NEdgeTiles == 0)
      columnLaunchAs<BtrEdgeNone, true>(A, P, Tile, 0, NTiles, Bytes, S);
   else if (Forcing)
      columnLaunchAs<BtrEdgeForcing, false>(A, P, Tile, NEdgeTiles, NEdgeTiles, Bytes, S);
   else if (NCellTiles > 0)
      columnLaunchAs<BtrEdgeSplit, true>(A, P, Tile, NEdgeTiles, NTiles, Bytes, S);
   else
      columnLaunchAs<BtrEdgeSplit, false>(A, P, Tile, NEdgeTiles, NTiles, Bytes, S);
   HIP_CHECK(hipGetLastError());
}

void launchBtrLevels(const BtrLevelArgs &A, BtrLevelOp Op, hipStream_t S) {
   if (A.NEdgesAll <= 0 || A.K <= 0)
      return;
   const int Pitch = levelPitch(A.K);
   const dim3 Grid((A.NEdgesAll + RowTile - 1) / RowTile), Block(RowBlock);
   withLaneType(Pitch, [&](auto Lane) {
      using T = decltype(Lane);
      if (Op == BtrLevelRecombine)
         hipLaunchKernelGGL((btrLevelKernel<T, BtrLevelRecombine>), Grid, Block, 0, S, A, Pitch);
      else if (Op == BtrLevelTransport)
         hipLaunchKernelGGL((btrLevelKernel<T, BtrLevelTransport>), Grid, Block, 0, S, A, Pitch);
      else
         hipLaunchKernelGGL((btrLevelKernel<T, BtrLevelAdvance>), Grid, Block, 0, S, A, Pitch);
   });
   HIP_CHECK(hipGetLastError());
}

void launchBtrCells(const BtrSubArgs &A, hipStream_t S) {
   if (A.NCellsAll <= 0)
      return;
   hipLaunchKernelGGL(btrCellKernel, dim3((A.NCellsAll + SubThreads - 1) / SubThreads), dim3(SubThreads), 0, S, A);
   HIP_CHECK(hipGetLastError());
}

void launchBtrEdges(const BtrSubArgs &A, hipStream_t S) {
   if (A.NEdgesAll <= 0)
      return;
   hipLaunchKernelGGL(btrEdgeKernel, dim3((A.NEdgesAll + SubThreads - 1) / SubThreads), dim3(SubThreads), 0, S, A);
   HIP_CHECK(hipGetLastError());
}

void launchBtrResidual(const BtrSubArgs &A, const Real *TendMean, Real *Forcing, hipStream_t S) {
   if (A.NEdgesAll <= 0)
      return;
   hipLaunchKernelGGL(btrResidualKernel, dim3((A.NEdgesAll + SubThreads - 1) / SubThreads), dim3(SubThreads), 0, S, A,
                      TendMean, Forcing);
   HIP_CHECK(hipGetLastError());
}

void launchBtrDivide(Real *X, int N, Real Div, hipStream_t S) {
   if (N <= 0)
      return;
   hipLaunchKernelGGL(btrDivideKernel, dim3((N + SubThreads - 1) / SubThreads), dim3(SubThreads), 0, S, X, N, Div);
   HIP_CHECK(hipGetLastError());
}

} // namespace OMEGA
