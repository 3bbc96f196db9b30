// VertAdvKernels.hip -- the three kernels behind VertAdv (VertAdv.h) on gfx950.
//
// Column launch (transport scan, thickness update, or both): the shape of ColumnKernels.hip.  A workgroup of 256 threads
// owns a tile of consecutive cells; because the arrays are [cell][Pitch] rows the tile of one array is one contiguous
// run, staged into LDS with 16-byte-per-lane loads whatever the column length.  LDS rows are padded to an odd number of
// doubles so that the one-lane-per-column scan reads distinct banks.  The point-wise thickness update and the
// write-back run with the lanes along the flat run again, 16-byte stores where both values of a pair are inside their
// column's range.  Land columns have an empty range; rows >= NCellsAll are never part of a tile.
//
// Tracer launch: a workgroup owns 32 consecutive cells, the lanes run along the levels of a row, two levels per lane
// as one 16-byte access when the row pitch is even.  A lane keeps the thickness and the transport of its levels and of
// the two neighbouring ones in registers and sweeps every tracer with them: the tracer loop is inside the kernel.  The
// neighbouring levels K-1 and K+W of a tracer are loaded from the same 128-byte lines that the lanes next to it load
// at the same instant (one coalesced run per row), so they cost L1 requests, not HBM traffic.
//
// Edge launch: the tile shape of PressureGradKernels.hip -- 32 edges per workgroup, the two cells, the level range and
// the mask staged in LDS, the lanes along the levels with two levels per 16-byte access, tiles dealt out per XCD
// (xcdRemap) so that the cell rows neighbouring edges share come from that XCD's L2.  One thread owns (edge, level).
//
// No atomics and no scratch anywhere; a level pair that straddles the end of a range is computed whole and stored one
// value wide, so nothing outside the ranges is written.
#include "KernelCommon.h"
#include "VertAdvKernels.h"

namespace OMEGA {

namespace {

// ---------------------------------------------------------------------------------------------------- column launch
constexpr int ColThreads = 256;
constexpr int ColLdsBytes = 65536;

/// LDS row pitch of a column of `P` values: odd, so that lanes c and c+1 of a scan sit on different banks
__host__ __device__ inline int ldsPitch(int P) { return P | 1; }
/// doubles of LDS for a tile of T columns: tendency, reference thickness or nothing, transport, and the ranges
__host__ __device__ inline size_t colLdsDoubles(int T, int LP) { return (size_t)T * (3 * (size_t)LP + 1); }

__device__ inline bool aligned16(const void *P) { return ((uintptr_t)P & 15) == 0; }

/// Visit the flat run [0, N) in pairs (i, i+1), lanes along the run: F(i, Two) with Two = (i+1 < N)
template <class F> __device__ inline void forPairs(int N, F &&Fn) {
   for (int I = 2 * (int)threadIdx.x; I < N; I += 2 * ColThreads)
      Fn(I, I + 1 < N);
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

/// Stage Nc whole rows of a [cell][P] array starting at row C0 into LDS rows of pitch LP
__device__ inline void loadTile(const Real *G, int P, int C0, int Nc, Real *L, int LP) {
   const Real *Gt = G + (size_t)C0 * P;
   forPairs(Nc * P, [&](int I, bool Two) {
      const Pos2 Q(I, P);
      if (Two && aligned16(Gt + I)) {
         const double2 V        = *reinterpret_cast<const double2 *>(Gt + I);
         L[Q.C0 * LP + Q.K0] = V.x;
         L[Q.C1 * LP + Q.K1] = V.y;
      } else {
         L[Q.C0 * LP + Q.K0] = Gt[I];
         if (Two)
            L[Q.C1 * LP + Q.K1] = Gt[I + 1];
      }
   });
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
   if (Tid < Nc) {
      const I4 KMin = A.MinLayerCell[C0 + Tid], KMax = A.MaxLayerCell[C0 + Tid];
      const bool Ok = KMin >= 0 && KMin <= KMax && KMax < K;
      Lo[Tid] = Ok ? KMin : 1;
      Hi[Tid] = Ok ? KMax : -1;
   }
   loadTile(A.Tend, P, C0, Nc, LD, LP);
   if (Scan)
      loadTile(A.RefThick, P, C0, Nc, LR, LP);
   else
      loadTile(A.Transport, P, C0, Nc, LW, LP);
   __syncthreads();
   auto Active = [&](int C, int Kk) { return Kk >= Lo[C] && Kk <= Hi[C]; };

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
      Real *G = A.Transport + (size_t)C0 * P;
      forPairs(Nc * P, [&](int I, bool Two) {
         const Pos2 Q(I, P);
         const bool W0 = Active(Q.C0, Q.K0), W1 = Two && Active(Q.C1, Q.K1);
         store2(G + I, W0, W1, W0 ? LW[Q.C0 * LP + Q.K0] : 0.0, W1 ? LW[Q.C1 * LP + Q.K1] : 0.0);
      });
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
constexpr int TrBlock = 256;
constexpr int TrTile  = 32; // cells per workgroup

template <class T, int Order>
__global__ void __launch_bounds__(TrBlock) vertAdvTracerKernel(VertAdvTracerArgs A, int Pitch) {
   constexpr int W = VecW<T>::W;
   __shared__ int Lo[TrTile], Hi[TrTile];
   const int First = blockIdx.x * TrTile;
   int Cnt         = A.NCellsAll - First;
   if (Cnt > TrTile)
      Cnt = TrTile;
   const int Tid = threadIdx.x;
   if (Tid < Cnt) {
      const I4 KMin = A.MinLayerCell[First + Tid], KMax = A.MaxLayerCell[First + Tid];
      const bool Ok = KMin >= 0 && KMin <= KMax && KMax < A.K;
      Lo[Tid] = Ok ? KMin : A.K;
      Hi[Tid] = Ok ? KMax : -1;
   }
   __syncthreads();
   const int Lanes    = Pitch / W; // lanes along one row
   const size_t Plane = (size_t)A.NCellsSize * Pitch;
   for (int Idx = Tid; Idx < Cnt * Lanes; Idx += TrBlock) {
      const int Le = Idx / Lanes;
      const int K0 = (Idx - Le * Lanes) * W;
      const int L = Lo[Le], H = Hi[Le];
      if (K0 + W - 1 < L || K0 > H)
         continue;
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
         if constexpr (W == 2) {
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
   }
}

// ------------------------------------------------------------------------------------------------------ edge launch
constexpr int EdgeBlock = 256;
constexpr int EdgeTile  = 32; // edges per workgroup

template <class T>
__global__ void __launch_bounds__(EdgeBlock) vertAdvEdgeKernel(VertAdvEdgeArgs A, int Pitch, int NTiles) {
   constexpr int W = VecW<T>::W;
   __shared__ int Cell0[EdgeTile], Cell1[EdgeTile], Lo[EdgeTile], Hi[EdgeTile];
   __shared__ Real Mask[EdgeTile];
   const int First = xcdRemap(blockIdx.x, NTiles) * EdgeTile;
   int Cnt         = A.NEdgesAll - First;
   if (Cnt > EdgeTile)
      Cnt = EdgeTile;
   const int Tid = threadIdx.x;
   if (Tid < Cnt) {
      const int E  = First + Tid;
      const int C0 = A.CellsOnEdge[2 * (size_t)E], C1 = A.CellsOnEdge[2 * (size_t)E + 1];
      int L = A.MinLayerEdgeBot[E], H = A.MaxLayerEdgeTop[E];
      if (!(L >= 0 && L <= H && H < A.K) || C0 < 0 || C0 >= A.NCellsSize || C1 < 0 || C1 >= A.NCellsSize)
         L = A.K, H = -1; // an empty range: the edge is left alone
      Cell0[Tid] = C0, Cell1[Tid] = C1, Lo[Tid] = L, Hi[Tid] = H;
      Mask[Tid]  = A.EdgeMask[E];
   }
   __syncthreads();
   const int Lanes = Pitch / W; // lanes along one row
   for (int Idx = Tid; Idx < Cnt * Lanes; Idx += EdgeBlock) {
      const int Le = Idx / Lanes;
      const int K0 = (Idx - Le * Lanes) * W;
      const int L = Lo[Le], H = Hi[Le];
      if (K0 + W - 1 < L || K0 > H)
         continue;
      const size_t R0 = (size_t)Cell0[Le] * Pitch + K0, R1 = (size_t)Cell1[Le] * Pitch + K0;
      const size_t Re = (size_t)(First + Le) * Pitch + K0;
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
      const Real M = Mask[Le];
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
      if constexpr (W == 2) {
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
}

} // namespace

int vertAdvColumnTile(int K) {
   const int LP = ldsPitch(levelPitch(K));
   for (int Tile = 16; Tile >= 2; Tile /= 2)
      if (colLdsDoubles(Tile, LP) * sizeof(Real) <= (size_t)ColLdsBytes)
         return Tile;
   return 0;
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
   const dim3 Grid((A.NCellsAll + TrTile - 1) / TrTile), Block(TrBlock);
   const bool Two = Pitch % 2 == 0, Centred = A.Order == 2;
   if (Two && Centred)
      hipLaunchKernelGGL((vertAdvTracerKernel<dv2, 2>), Grid, Block, 0, S, A, Pitch);
   else if (Two)
      hipLaunchKernelGGL((vertAdvTracerKernel<dv2, 1>), Grid, Block, 0, S, A, Pitch);
   else if (Centred)
      hipLaunchKernelGGL((vertAdvTracerKernel<double, 2>), Grid, Block, 0, S, A, Pitch);
   else
      hipLaunchKernelGGL((vertAdvTracerKernel<double, 1>), Grid, Block, 0, S, A, Pitch);
   HIP_CHECK(hipGetLastError());
}

void launchVertAdvEdge(const VertAdvEdgeArgs &A, hipStream_t S) {
   if (A.NEdgesAll <= 0 || A.K <= 0)
      return;
   const int Pitch  = levelPitch(A.K);
   const int NTiles = (A.NEdgesAll + EdgeTile - 1) / EdgeTile;
   if (Pitch % 2 == 0)
      hipLaunchKernelGGL(vertAdvEdgeKernel<dv2>, dim3(NTiles), dim3(EdgeBlock), 0, S, A, Pitch, NTiles);
   else
      hipLaunchKernelGGL(vertAdvEdgeKernel<double>, dim3(NTiles), dim3(EdgeBlock), 0, S, A, Pitch, NTiles);
   HIP_CHECK(hipGetLastError());
}

} // namespace OMEGA
