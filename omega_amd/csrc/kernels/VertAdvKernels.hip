// VertAdvKernels.hip -- the three kernels behind VertAdv (VertAdv.h) on gfx950.
//
// Column launch (transport scan, thickness update, or both): the column tile of LevelTile.h.  The tendency, the
// reference thickness (or, without the scan, the transport) are staged into LDS; the scan runs one lane per column; the
// point-wise thickness update and the write-back run with the lanes along the flat run again, 16-byte stores where both
// values of a pair are inside their column's range.  Land columns have an empty range; rows >= NCellsAll are never
// part of a tile.
//
// Tracer launch: the level-row tile of LevelTile.h over cells.  A lane keeps the thickness and the transport of its levels and of
// the two neighbouring ones in registers and sweeps every tracer with them: the tracer loop is inside the kernel.  The
// neighbouring levels K-1 and K+W of a tracer are loaded from the same 128-byte lines that the lanes next to it load
// at the same instant (one coalesced run per row), so they cost L1 requests, not HBM traffic.
//
// Edge launch: the level-row tile over edges, as in PressureGradKernels.hip -- the two cells, the level range and the
// mask staged in LDS (stageEdgeTile), tiles dealt out per XCD so that the cell rows neighbouring edges share come from
// that XCD's L2.  One thread owns (edge, level).
//
// No atomics and no scratch anywhere; a level pair that straddles the end of a range is computed whole and stored one
// value wide, so nothing outside the ranges is written.
#include "LevelTile.h"
#include "VertAdvKernels.h"

namespace OMEGA {

namespace {

// ---------------------------------------------------------------------------------------------------- column launch
/// doubles of LDS for a tile of T columns: tendency, reference thickness or nothing, transport, and the ranges
inline size_t colLdsDoubles(int T, int LP) { return (size_t)T * (3 * (size_t)LP + 1); }

template <bool Scan, bool Thick>
__global__ void __launch_bounds__(ColThreads) vertAdvColumnKernel(VertAdvColumnArgs A, int P, int Tile) {
   extern __shared__ Real Lds[];
   const int C0 = blockIdx.x * Tile;
   const int Nc = min(Tile, A.NCellsAll - C0);
   const int K = A.K, LP = ldsPitch(P);
   Real *LD = Lds, *LR = LD + Tile * LP, *LW = LR + Tile * LP;
   I4 *Lo = reinterpret_cast<I4 *>(LW + Tile * LP), *Hi = Lo + Tile;
   const int Tid = threadIdx.x;

   // per-column active range; a column outside 0 <= KMin <= KMax < K (land) gets an empty one
   stageRanges(A.MinLayerCell, A.MaxLayerCell, C0, Nc, K, Lo, Hi);
   const AllLevels All;
   loadTile(A.Tend, P, C0, Nc, LD, LP, All);
   if (Scan)
      loadTile(A.RefThick, P, C0, Nc, LR, LP, All);
   else
      loadTile(A.Transport, P, C0, Nc, LW, LP, All);
   __syncthreads();
   const InRange Active{Lo, Hi};

   if (Scan) {
      if (Tid < Nc && Lo[Tid] <= Hi[Tid]) {
         const int C = Tid, KMin = Lo[C], KMax = Hi[C];
         const Real *D = LD + C * LP, *R = LR + C * LP;
         Real *Wt = LW + C * LP;
         Real SumD = 0.0, SumWh = 0.0;
         for (int Kk = KMin; Kk <= KMax; ++Kk) {
            SumD  = SumD + D[Kk];
            SumWh = SumWh + A.MoveWeights[Kk] * R[Kk];
         }
         Real Acc = 0.0;
         for (int Kk = KMax; Kk >= KMin; --Kk) {
            const Real TT = ((A.MoveWeights[Kk] * R[Kk]) / SumWh) * SumD;
            Acc           = Acc + (D[Kk] - TT);
            Wt[Kk]        = Acc;
         }
         Wt[KMin] = 0.0;
      }
      __syncthreads();
      storeTile(A.Transport, P, C0, Nc, LW, LP, Active);
   }

   if (Thick) {
      Real *G    = A.Tend + (size_t)C0 * P;
      auto Value = [&](int C, int Kk) {
         const Real Wb = Kk < Hi[C] ? LW[C * LP + Kk + 1] : 0.0;
         return (LD[C * LP + Kk] - LW[C * LP + Kk]) + Wb;
      };
      forPairs(Nc * P, [&](int I, bool Two) {
         const Pos2 Q(I, P);
         const bool W0 = Active(Q.C0, Q.K0), W1 = Two && Active(Q.C1, Q.K1);
         store2(G + I, W0, W1, W0 ? Value(Q.C0, Q.K0) : 0.0, W1 ? Value(Q.C1, Q.K1) : 0.0);
      });
   }
}

// ---------------------------------------------------------------------------------------------------- tracer launch
template <class T, int Order>
__global__ void __launch_bounds__(RowBlock) vertAdvTracerKernel(VertAdvTracerArgs A, int Pitch) {
   constexpr int W = VecW<T>::W;
   __shared__ int Lo[RowTile], Hi[RowTile];
   const int First = blockIdx.x * RowTile;
   int Cnt         = A.NCellsAll - First;
   if (Cnt > RowTile)
      Cnt = RowTile;
   stageRanges(A.MinLayerCell, A.MaxLayerCell, First, Cnt, A.K, Lo, Hi);
   __syncthreads();
   const size_t Plane = (size_t)A.NCellsSize * Pitch;
   forLevelRuns<T>(Cnt, Pitch, Lo, Hi, [&](int Le, int K0, int L, int H) {
      const size_t R = (size_t)(First + Le) * Pitch + K0;
      // interface J is the top of level K0 + J: a flux passes it when KMin < K0 + J <= KMax
      bool Int[W + 1];
#pragma unroll
      for (int J = 0; J <= W; ++J)
         Int[J] = K0 + J > L && K0 + J <= H;
      // thickness of the levels K0 - 1 .. K0 + W and transport of the interfaces K0 .. K0 + W, held for all tracers
      Real Hh[W + 2], Wt[W + 1];
      {
         const T Hv = *reinterpret_cast<const T *>(A.LayerThick + R);
         const T Wv = *reinterpret_cast<const T *>(A.Transport + R);
#pragma unroll
         for (int J = 0; J < W; ++J)
            Hh[J + 1] = getc(Hv, J), Wt[J] = getc(Wv, J);
         Hh[0]     = Int[0] ? A.LayerThick[R - 1] : 1.0;
         Hh[W + 1] = Int[W] ? A.LayerThick[R + W] : 1.0;
         Wt[W]     = Int[W] ? A.Transport[R + W] : 0.0;
      }
      Real Den[W + 1];
#pragma unroll
      for (int J = 0; J <= W; ++J)
         Den[J] = Hh[J] + Hh[J + 1];
      for (int Tr = 0; Tr < A.NTracers; ++Tr) {
         const Real *Phi = A.Tracers + Tr * Plane + R;
         Real *Out       = A.Tend + Tr * Plane + R;
         const T Pv      = *reinterpret_cast<const T *>(Phi);
         const T In      = *reinterpret_cast<const T *>(Out);
         Real Ph[W + 2];
#pragma unroll
         for (int J = 0; J < W; ++J)
            Ph[J + 1] = getc(Pv, J);
         Ph[0]     = Int[0] ? Phi[-1] : 0.0;
         Ph[W + 1] = Int[W] ? Phi[W] : 0.0;
         Real F[W + 1];
#pragma unroll
         for (int J = 0; J <= W; ++J) {
            Real Top;
            if constexpr (Order == 2)
               Top = ((Hh[J] * Ph[J + 1]) + (Hh[J + 1] * Ph[J])) / Den[J];
            else
               Top = Wt[J] > 0.0 ? Ph[J + 1] : Ph[J];
            F[J] = Int[J] ? Wt[J] * Top : 0.0;
         }
         T Res;
#pragma unroll
         for (int J = 0; J < W; ++J)
            setc(Res, J, (getc(In, J) - F[J]) + F[J + 1]);
         storeRanged<T>(Out, Res, K0, L, H);
      }
   });
}

// ------------------------------------------------------------------------------------------------------ edge launch
template <class T>
__global__ void __launch_bounds__(RowBlock) vertAdvEdgeKernel(VertAdvEdgeArgs A, int Pitch, int NTiles) {
   constexpr int W = VecW<T>::W;
   const EdgeTile E = stageEdgeTile(A, NTiles, [](int, int) {});
   forLevelRuns<T>(E.Cnt, Pitch, E.Lo, E.Hi, [&](int Le, int K0, int L, int H) {
      const size_t R0 = (size_t)E.Cell0[Le] * Pitch + K0, R1 = (size_t)E.Cell1[Le] * Pitch + K0;
      const size_t Re = (size_t)(E.First + Le) * Pitch + K0;
      const T H0 = *reinterpret_cast<const T *>(A.LayerThick + R0), H1 = *reinterpret_cast<const T *>(A.LayerThick + R1);
      const T W0 = *reinterpret_cast<const T *>(A.Transport + R0), W1 = *reinterpret_cast<const T *>(A.Transport + R1);
      const T Uv = *reinterpret_cast<const T *>(A.NormalVelocity + Re);
      Real *Out  = A.Tend + Re;
      const T In = *reinterpret_cast<const T *>(Out);
      // u of the levels K0 - 1 .. K0 + W, the edge's transport at the interfaces K0 .. K0 + W; the neighbours outside
      // the pair are read only where a flux of the range needs them
      const bool Up = K0 > L && K0 <= H, Down = K0 + W - 1 >= L && K0 + W <= H;
      Real Uu[W + 2], We[W + 1];
#pragma unroll
      for (int J = 0; J < W; ++J) {
         Uu[J + 1] = getc(Uv, J);
         We[J]     = 0.5 * (getc(W0, J) + getc(W1, J));
      }
      Uu[0]     = Up ? A.NormalVelocity[Re - 1] : 0.0;
      Uu[W + 1] = Down ? A.NormalVelocity[Re + W] : 0.0;
      We[W]     = Down ? 0.5 * (A.Transport[R0 + W] + A.Transport[R1 + W]) : 0.0;
      const Real M = E.Mask[Le];
      T Res;
#pragma unroll
      for (int J = 0; J < W; ++J) {
         const int Kk    = K0 + J;
         const Real U    = Uu[J + 1];
         const Real HE   = 0.5 * (getc(H0, J) + getc(H1, J));
         const Real UTop = 0.5 * (Uu[J] + U), UBot = 0.5 * (U + Uu[J + 2]);
         const Real FTop = Kk == L ? 0.0 : We[J] * (UTop - U);
         const Real FBot = Kk == H ? 0.0 : We[J + 1] * (UBot - U);
         setc(Res, J, getc(In, J) - M * ((FTop - FBot) / HE));
      }
      storeRanged<T>(Out, Res, K0, L, H);
   });
}

} // namespace

int vertAdvColumnTile(int K) {
   const int LP = ldsPitch(levelPitch(K));
   return pickColumnTile([&](int T) { return colLdsDoubles(T, LP); });
}

void launchVertAdvColumn(const VertAdvColumnArgs &A, bool Scan, bool Thick, hipStream_t S) {
   if (A.NCellsAll <= 0 || A.K <= 0 || !(Scan || Thick))
      return;
   const int Tile = vertAdvColumnTile(A.K);
   OMEGA_REQUIRE(Tile >= 2, "VertAdv column kernel: NVertLayers " + std::to_string(A.K) + " is too long for the LDS tile");
   const int P        = levelPitch(A.K);
   const size_t Bytes = colLdsDoubles(Tile, ldsPitch(P)) * sizeof(Real);
   const dim3 Grid((A.NCellsAll + Tile - 1) / Tile), Block(ColThreads);
   if (Scan && Thick)
      hipLaunchKernelGGL((vertAdvColumnKernel<true, true>), Grid, Block, Bytes, S, A, P, Tile);
   else if (Scan)
      hipLaunchKernelGGL((vertAdvColumnKernel<true, false>), Grid, Block, Bytes, S, A, P, Tile);
   else
      hipLaunchKernelGGL((vertAdvColumnKernel<false, true>), Grid, Block, Bytes, S, A, P, Tile);
   HIP_CHECK(hipGetLastError());
}

void launchVertAdvTracer(const VertAdvTracerArgs &A, hipStream_t S) {
   if (A.NCellsAll <= 0 || A.K <= 0 || A.NTracers <= 0)
      return;
   const int Pitch = levelPitch(A.K);
   const dim3 Grid((A.NCellsAll + RowTile - 1) / RowTile), Block(RowBlock);
   withLaneType(Pitch, [&](auto Lane) {
      using T = decltype(Lane);
      if (A.Order == 2)
         hipLaunchKernelGGL((vertAdvTracerKernel<T, 2>), Grid, Block, 0, S, A, Pitch);
      else
         hipLaunchKernelGGL((vertAdvTracerKernel<T, 1>), Grid, Block, 0, S, A, Pitch);
   });
   HIP_CHECK(hipGetLastError());
}

void launchVertAdvEdge(const VertAdvEdgeArgs &A, hipStream_t S) {
   if (A.NEdgesAll <= 0 || A.K <= 0)
      return;
   const int Pitch  = levelPitch(A.K);
   const int NTiles = (A.NEdgesAll + RowTile - 1) / RowTile;
   withLaneType(Pitch, [&](auto Lane) {
      hipLaunchKernelGGL(vertAdvEdgeKernel<decltype(Lane)>, dim3(NTiles), dim3(RowBlock), 0, S, A, Pitch, NTiles);
   });
   HIP_CHECK(hipGetLastError());
}

} // namespace OMEGA
