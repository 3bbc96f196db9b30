// LevelTile.h -- the two workgroup shapes of the kernels over level-indexed arrays ([rows][Pitch], Pitch =
// levelPitch(K)), written once: ColumnKernels.hip, VertAdvKernels.hip and PressureGradKernels.hip are built on them.
//
// Column tile: a workgroup of ColThreads threads owns `Tile` consecutive cells.  The tile of one array is one
// contiguous run of Tile*Pitch values: it is staged into LDS with 16-byte-per-lane loads (loadTile) and written back
// with 16-byte-per-lane stores (storeTile, store2) whatever the column length; point-wise work runs with the lanes along
// the flat run (forPairs, Pos2), sequential work one lane per column out of LDS.  The LDS rows have an odd pitch
// (ldsPitch) so that the one-lane-per-column scans read distinct banks.  The host picks the largest tile whose LDS fits
// (pickColumnTile).
//
// Level-row tile: a workgroup of RowBlock threads owns RowTile consecutive rows (cells or edges), the lanes run along
// the levels of a row, two levels per lane as one 16-byte access when the row pitch is even (withLaneType: dv2 or
// double).  The per-row level range is staged in LDS (stageRanges, or stageEdgeTile with the edge's two cells and its
// mask); forLevelRuns visits the level runs that overlap their row's range and storeRanged writes a run's values inside
// it, one value wide where a pair straddles its end, so nothing outside the ranges is written.
//
// Everything here is inline: no kernel, no launch and no barrier of its own except the one stageEdgeTile ends with.
#ifndef OMEGA_AMD_LEVELTILE_H
#define OMEGA_AMD_LEVELTILE_H

#include "KernelCommon.h"

namespace OMEGA {

// ------------------------------------------------------------------------------------------------------ column tile
constexpr int ColThreads  = 256;
constexpr int ColLdsBytes = 65536;

/// LDS row pitch of a column of `P` values: odd, so that lanes c and c+1 of a scan sit on different banks
__host__ __device__ inline int ldsPitch(int P) { return P | 1; }

/// Columns per workgroup of a column-tile launch: the largest of 16, 8, 4, 2 whose LDS -- Doubles(T) doubles for a
/// tile of T columns -- fits 64 KiB; 0 if none does
template <class F> inline int pickColumnTile(F &&Doubles) {
   for (int T = 16; T >= 2; T /= 2)
      if ((size_t)Doubles(T) * sizeof(Real) <= (size_t)ColLdsBytes)
         return T;
   return 0;
}

__device__ inline bool aligned16(const void *P) { return ((uintptr_t)P & 15) == 0; }

/// Visit the flat run [0, N) in pairs (i, i+1), lanes along the run: F(i, Two) with Two = (i+1 < N)
template <class F> __device__ inline void forPairs(int N, F &&Fn) {
   for (int I = 2 * (int)threadIdx.x; I < N; I += 2 * ColThreads)
      Fn(I, I + 1 < N);
}

__device__ inline void load2(const Real *P, bool Two, Real &V0, Real &V1) {
   if (Two && aligned16(P)) {
      const double2 V = *reinterpret_cast<const double2 *>(P);
      V0 = V.x, V1 = V.y;
   } else {
      V0 = P[0];
      V1 = Two ? P[1] : 0.0;
   }
}

__device__ inline void store2(Real *P, bool W0, bool W1, Real V0, Real V1) {
   if (W0 && W1 && aligned16(P)) {
      *reinterpret_cast<double2 *>(P) = make_double2(V0, V1);
   } else {
      if (W0)
         P[0] = V0;
      if (W1)
         P[1] = V1;
   }
}

/// (cell, level) of flat position I of a run of rows of pitch P, and of I + 1
struct Pos2 {
   int C0, K0, C1, K1;
   __device__ Pos2(int I, int P) {
      C0 = I / P;
      K0 = I - C0 * P;
      C1 = C0, K1 = K0 + 1;
      if (K1 == P)
         C1 += 1, K1 = 0;
   }
};

/// Stage the active level ranges of the Nc rows from row R0 into LDS, one lane per row (the caller's next barrier
/// publishes them).  Null MinLayer / MaxLayer mean all K levels.  A row outside 0 <= KMin <= KMax < K (land) gets the
/// empty range [1, -1]: no level is inside it and Lo <= Hi fails.
__device__ inline void stageRanges(const I4 *MinLayer, const I4 *MaxLayer, int R0, int Nc, int K, int *Lo, int *Hi) {
   const int Tid = threadIdx.x;
   if (Tid < Nc) {
      const I4 KMin = MinLayer ? MinLayer[R0 + Tid] : 0, KMax = MaxLayer ? MaxLayer[R0 + Tid] : K - 1;
      const bool Ok = KMin >= 0 && KMin <= KMax && KMax < K;
      Lo[Tid] = Ok ? KMin : 1;
      Hi[Tid] = Ok ? KMax : -1;
   }
}

/// The predicates of loadTile / storeTile: every (column, level), or the levels of a column's staged range, widened by
/// `Below` levels at its bottom (1: the interfaces of the range)
struct AllLevels {
   __device__ bool operator()(int, int) const { return true; }
};
struct InRange {
   const int *Lo, *Hi;
   int Below = 0;
   __device__ bool operator()(int C, int Kk) const { return Kk >= Lo[C] && Kk <= Hi[C] + Below; }
};

/// Stage Nc columns of a [cell][P] array starting at row C0 into LDS rows of pitch LP.  Want(c, k) selects the values
/// to keep (the loads are issued for whole pairs: both are inside the rows being read).
template <class W>
__device__ inline void loadTile(const Real *G, int P, int C0, int Nc, Real *L, int LP, W &&Want) {
   const Real *Gt = G + (size_t)C0 * P;
   forPairs(Nc * P, [&](int I, bool Two) {
      const Pos2 Q(I, P);
      Real V0, V1;
      load2(Gt + I, Two, V0, V1);
      if (Want(Q.C0, Q.K0))
         L[Q.C0 * LP + Q.K0] = V0;
      if (Two && Want(Q.C1, Q.K1))
         L[Q.C1 * LP + Q.K1] = V1;
   });
}

/// Write the LDS values (c, k) with Want(c, k) back to a [cell][P] array
template <class W>
__device__ inline void storeTile(Real *G, int P, int C0, int Nc, const Real *L, int LP, W &&Want) {
   Real *Gt = G + (size_t)C0 * P;
   forPairs(Nc * P, [&](int I, bool Two) {
      const Pos2 Q(I, P);
      const bool W0 = Want(Q.C0, Q.K0), W1 = Two && Want(Q.C1, Q.K1);
      store2(Gt + I, W0, W1, W0 ? L[Q.C0 * LP + Q.K0] : 0.0, W1 ? L[Q.C1 * LP + Q.K1] : 0.0);
   });
}

// --------------------------------------------------------------------------------------------------- level-row tile
constexpr int RowBlock = 256;
constexpr int RowTile  = 32; // rows per workgroup

/// Launch with the lane type of a level-row kernel: Fn(dv2()) for an even row pitch (two levels per lane, one 16-byte
/// access), Fn(double()) for an odd one
template <class F> inline void withLaneType(int Pitch, F &&Fn) {
   if (Pitch % 2 == 0)
      Fn(dv2());
   else
      Fn(double());
}

/// What stageEdgeTile leaves in LDS for the Cnt edges from edge First: the two cells, the level range and the mask
struct EdgeTile {
   int First, Cnt;
   const int *Cell0, *Cell1, *Lo, *Hi;
   const Real *Mask;
};

/// The prologue of an edge kernel (Args: NEdgesAll, NCellsSize, K, CellsOnEdge, MinLayerEdgeBot, MaxLayerEdgeTop,
/// EdgeMask).  Tiles are dealt out through xcdRemap.  An edge with an invalid range or a cell outside
/// [0, NCellsSize) gets the empty range [K, -1]: it is left alone.  Also(Le, E) stages what else the kernel keeps per
/// edge, before the one barrier.
template <class Args, class F> __device__ inline EdgeTile stageEdgeTile(const Args &A, int NTiles, F &&Also) {
   __shared__ int Cell0[RowTile], Cell1[RowTile], Lo[RowTile], Hi[RowTile];
   __shared__ Real Mask[RowTile];
   const int First = xcdRemap(blockIdx.x, NTiles) * RowTile;
   int Cnt         = A.NEdgesAll - First;
   if (Cnt > RowTile)
      Cnt = RowTile;
   const int Tid = threadIdx.x;
   if (Tid < Cnt) {
      const int E  = First + Tid;
      const int C0 = A.CellsOnEdge[2 * (size_t)E], C1 = A.CellsOnEdge[2 * (size_t)E + 1];
      int L = A.MinLayerEdgeBot[E], H = A.MaxLayerEdgeTop[E];
      if (!(L >= 0 && L <= H && H < A.K) || C0 < 0 || C0 >= A.NCellsSize || C1 < 0 || C1 >= A.NCellsSize)
         L = A.K, H = -1;
      Cell0[Tid] = C0, Cell1[Tid] = C1, Lo[Tid] = L, Hi[Tid] = H;
      Mask[Tid]  = A.EdgeMask[E];
      Also(Tid, E);
   }
   __syncthreads();
   return {First, Cnt, Cell0, Cell1, Lo, Hi, Mask};
}

/// Lanes along the levels of the tile's Cnt rows, VecW<T>::W levels per lane: Fn(Le, K0, L, H) for every run
/// K0 .. K0 + W - 1 of row Le that overlaps the row's range [L, H] = [Lo[Le], Hi[Le]]
template <class T, class F>
__device__ inline void forLevelRuns(int Cnt, int Pitch, const int *Lo, const int *Hi, F &&Fn) {
   constexpr int W = VecW<T>::W;
   const int Lanes = Pitch / W; // lanes along one row
   for (int Idx = threadIdx.x; Idx < Cnt * Lanes; Idx += RowBlock) {
      const int Le = Idx / Lanes;
      const int K0 = (Idx - Le * Lanes) * W;
      const int L = Lo[Le], H = Hi[Le];
      if (K0 + W - 1 < L || K0 > H)
         continue;
      Fn(Le, K0, L, H);
   }
}

/// Store the values of the run K0 .. K0 + W - 1 that lie inside [L, H] (the run overlaps the range: K0 <= H and
/// K0 + W - 1 >= L); Out points at level K0
template <class T> __device__ inline void storeRanged(Real *Out, T Res, int K0, int L, int H) {
   if constexpr (VecW<T>::W == 2) {
      const bool In0 = K0 >= L, In1 = K0 + 1 <= H;
      if (In0 && In1)
         *reinterpret_cast<T *>(Out) = Res;
      else if (In0)
         Out[0] = getc(Res, 0);
      else
         Out[1] = getc(Res, 1);
   } else {
      *reinterpret_cast<T *>(Out) = Res;
   }
}

} // namespace OMEGA
#endif
