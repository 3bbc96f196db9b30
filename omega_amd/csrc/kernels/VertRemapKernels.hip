// VertRemapKernels.hip -- the three kernels behind VertRemap (VertRemap.h) on gfx950.
//
// Cell launch (the target thickness, the tracer remap, or both): the column tile of LevelTile.h.  The thickness and the
// reference (or, without the target stage, the target) thickness are staged into LDS with 16-byte loads; the column
// sums of the target and the two interface scans run one lane per column out of odd-pitch LDS; everything else -- the
// target itself, the limited slopes, the interface values, the limited parabolas and the overlap sums -- runs with the
// lanes along the flat run, one (column, level) per lane and trip.  The overlap of a target layer with the source grid
// is data-dependent: a lane finds its first source cell by walking from its own level (the two grids are close) and then
// adds the pieces in ascending order, as the contract has it -- never as a difference of prefix sums.  The tracer loop is
// inside the kernel: a plane is staged, remapped and written back in place with 16-byte stores, the grids stay in LDS.
//
// Edge launch: the same tile over edges.  The edge's two cells and its range are staged first, the two thicknesses are
// formed from the two cells' rows (lanes along the levels of a row: one coalesced run per cell row), the velocity rows
// are staged like a tracer plane, and the column core is the cell launch's.
//
// Adoption: the level-row tile of LevelTile.h, a ranged copy.
//
// No atomics, no scratch, no grid-wide synchronisation; nothing outside the ranges is written (storeTile / storeRanged
// with the staged ranges).
#include "LevelTile.h"
#include "VertRemapKernels.h"

namespace OMEGA {

namespace {

/// LDS row pitch of the interfaces of a column of P levels (P + 1 of them): odd, like ldsPitch
__host__ __device__ inline int ifacePitch(int P) { return (P + 1) | 1; }

/// doubles of LDS for a tile of T columns: five level buffers, two interface buffers, two scalars per column, and per
/// column the range and the edge's two cells (4 x T ints = 2 x T doubles)
inline size_t remapLdsDoubles(int T, int LP, int LZ) { return (size_t)T * (5 * (size_t)LP + 2 * (size_t)LZ + 4); }

/// The buffers of a tile.  Three of them serve twice: T holds the target thickness until the interfaces are scanned,
/// then the right parabola value; D the limited slope, then the left parabola value; E the interface values, then the
/// result.
struct RemapTile {
   Real *H, *T, *A, *D, *E; ///< [Tile][LP]
   Real *Zs, *Zt;           ///< [Tile][LZ]: the source interfaces and the fitted target interfaces
   Real *Sc0, *Sc1;         ///< [Tile]
   int *Lo, *Hi, *Ca, *Cb;  ///< [Tile]
   int LP, LZ;
};
__device__ inline RemapTile carveTile(Real *Lds, int Tile, int P) {
   RemapTile B;
   B.LP = ldsPitch(P), B.LZ = ifacePitch(P);
   B.H   = Lds;
   B.T   = B.H + Tile * B.LP;
   B.A   = B.T + Tile * B.LP;
   B.D   = B.A + Tile * B.LP;
   B.E   = B.D + Tile * B.LP;
   B.Zs  = B.E + Tile * B.LP;
   B.Zt  = B.Zs + Tile * B.LZ;
   B.Sc0 = B.Zt + Tile * B.LZ;
   B.Sc1 = B.Sc0 + Tile;
   B.Lo  = reinterpret_cast<int *>(B.Sc1 + Tile);
   B.Hi  = B.Lo + Tile;
   B.Ca  = B.Hi + Tile;
   B.Cb  = B.Ca + Tile;
   return B;
}

/// Lanes along the flat run of the tile: Fn(C, Kk) for every (column, level) inside its column's range
template <class F> __device__ inline void forActive(const RemapTile &B, int Nc, int P, F &&Fn) {
   for (int I = threadIdx.x; I < Nc * P; I += ColThreads) {
      const int C = I / P, Kk = I - C * P;
      if (Kk >= B.Lo[C] && Kk <= B.Hi[C])
         Fn(C, Kk);
   }
}

/// zs and ZT of the contract from H and T, one lane per column; interface K is the top of level K
__device__ inline void scanInterfaces(const RemapTile &B, int Nc) {
   const int C = threadIdx.x;
   if (C < Nc && B.Lo[C] <= B.Hi[C]) {
      const int Lo = B.Lo[C], Hi = B.Hi[C];
      const Real *__restrict__ Hs = B.H + C * B.LP, *__restrict__ Ht = B.T + C * B.LP;
      Real *__restrict__ Zs = B.Zs + C * B.LZ, *__restrict__ Zt = B.Zt + C * B.LZ;
      // (four thicknesses are read ahead of the four dependent additions: the chain then waits for the adder, not for
      // an LDS round trip per level; the order of the additions is the contract's)
      Real Z = 0.0;
      Zs[Lo] = 0.0;
      int Kk = Lo;
      for (; Kk + 3 <= Hi; Kk += 4) {
         const Real A0 = Hs[Kk], A1 = Hs[Kk + 1], A2 = Hs[Kk + 2], A3 = Hs[Kk + 3];
         const Real Z1 = Z + A0, Z2 = Z1 + A1, Z3 = Z2 + A2;
         Z          = Z3 + A3;
         Zs[Kk + 1] = Z1, Zs[Kk + 2] = Z2, Zs[Kk + 3] = Z3, Zs[Kk + 4] = Z;
      }
      for (; Kk <= Hi; ++Kk) {
         Z          = Z + Hs[Kk];
         Zs[Kk + 1] = Z;
      }
      Real Y = 0.0;
      Zt[Lo] = 0.0;
      for (Kk = Lo; Kk + 3 < Hi; Kk += 4) {
         const Real A0 = Ht[Kk], A1 = Ht[Kk + 1], A2 = Ht[Kk + 2], A3 = Ht[Kk + 3];
         const Real Y1 = Y + A0, Y2 = Y1 + A1, Y3 = Y2 + A2;
         Y          = Y3 + A3;
         Zt[Kk + 1] = Y1 < Z ? Y1 : Z, Zt[Kk + 2] = Y2 < Z ? Y2 : Z, Zt[Kk + 3] = Y3 < Z ? Y3 : Z;
         Zt[Kk + 4] = Y < Z ? Y : Z;
      }
      for (; Kk < Hi; ++Kk) {
         Y          = Y + Ht[Kk];
         Zt[Kk + 1] = Y < Z ? Y : Z;
      }
      Zt[Hi + 1] = Z;
   }
}

/// d of the contract into D
__device__ inline void limitedSlopes(const RemapTile &B, int Nc, int P) {
   forActive(B, Nc, P, [&](int C, int Kk) {
      Real Dv = 0.0;
      if (Kk > B.Lo[C] && Kk < B.Hi[C]) {
         const Real *Hs = B.H + C * B.LP + Kk, *Av = B.A + C * B.LP + Kk;
         const Real Hm = Hs[-1], H0 = Hs[0], Hp = Hs[1];
         const Real Dm = Av[0] - Av[-1], Dp = Av[1] - Av[0];
         if (Dp * Dm > 0.0) {
            const Real Sl = (H0 / ((Hm + H0) + Hp)) *
                            ((((2.0 * Hm) + H0) / (Hp + H0)) * Dp + ((H0 + (2.0 * Hp)) / (Hm + H0)) * Dm);
            Real Tt = fabs(Sl), M = 2.0 * fabs(Dm);
            Tt = M < Tt ? M : Tt;
            M  = 2.0 * fabs(Dp);
            Tt = M < Tt ? M : Tt;
            Dv = Sl < 0.0 ? -Tt : Tt;
         }
      }
      B.D[C * B.LP + Kk] = Dv;
   });
}

/// e of the contract into E: entry K is the interface between levels K and K + 1
__device__ inline void interfaceValues(const RemapTile &B, int Nc, int P) {
   forActive(B, Nc, P, [&](int C, int Kk) {
      const int Lo = B.Lo[C], Hi = B.Hi[C];
      if (Kk >= Hi)
         return;
      const Real *Hs = B.H + C * B.LP + Kk, *Av = B.A + C * B.LP + Kk, *Dd = B.D + C * B.LP + Kk;
      const Real H0 = Hs[0], Hp = Hs[1];
      const Real Da = Av[1] - Av[0];
      Real Ev       = Av[0] + (H0 / (H0 + Hp)) * Da;
      if (Kk >= Lo + 1 && Kk + 2 <= Hi) {
         const Real Hm = Hs[-1], Hpp = Hs[2];
         const Real F1 = ((2.0 * Hp) * H0) / (H0 + Hp);
         const Real F2 = (Hm + H0) / ((2.0 * H0) + Hp);
         const Real F3 = (Hpp + Hp) / ((2.0 * Hp) + H0);
         const Real T1 = (F1 * (F2 - F3)) * Da;
         const Real T2 = ((H0 * (Hm + H0)) / ((2.0 * H0) + Hp)) * Dd[1];
         const Real T3 = ((Hp * (Hp + Hpp)) / (H0 + (2.0 * Hp))) * Dd[0];
         Ev            = Ev + (1.0 / (((Hm + H0) + Hp) + Hpp)) * ((T1 - T2) + T3);
      }
      B.E[C * B.LP + Kk] = Ev;
   });
}

/// aL into D and aR into T of the limited parabolas, from E
__device__ inline void limitedParabolas(const RemapTile &B, int Nc, int P) {
   forActive(B, Nc, P, [&](int C, int Kk) {
      const int O  = C * B.LP + Kk;
      const Real a = B.A[O];
      Real AL = a, AR = a;
      if (Kk > B.Lo[C] && Kk < B.Hi[C]) {
         AL = B.E[O - 1], AR = B.E[O];
         if ((AR - a) * (a - AL) <= 0.0) {
            AL = a, AR = a;
         } else {
            const Real Dl = AR - AL;
            const Real Q  = Dl * (a - 0.5 * (AL + AR));
            const Real S  = (Dl * Dl) / 6.0;
            if (Q > S)
               AL = (3.0 * a) - (2.0 * AR);
            else if (-S > Q)
               AR = (3.0 * a) - (2.0 * AL);
         }
      }
      B.D[O] = AL, B.T[O] = AR;
   });
}

/// aL, Dl = aR - aL and a6 of the cell at offset O of the level buffers
template <int Order> __device__ inline void cellCoeffs(const RemapTile &B, int O, Real &AL, Real &Dl, Real &A6) {
   const Real a = B.A[O];
   if constexpr (Order == 1) {
      AL = a, Dl = a - a, A6 = 0.0;
   } else if constexpr (Order == 2) {
      const Real Dd = B.D[O];
      AL            = a - 0.5 * Dd;
      const Real AR = a + 0.5 * Dd;
      Dl = AR - AL, A6 = 0.0;
   } else {
      AL            = B.D[O];
      const Real AR = B.T[O];
      Dl = AR - AL, A6 = 6.0 * (a - 0.5 * (AL + AR));
   }
}

/// The new mean of every target layer into E: each lane walks the source cells its layer overlaps, ascending
template <int Order> __device__ inline void overlapSums(const RemapTile &B, int Nc, int P) {
   forActive(B, Nc, P, [&](int C, int Kk) {
      const int Lo = B.Lo[C], Hi = B.Hi[C], Row = C * B.LP;
      const Real *Zs = B.Zs + C * B.LZ, *Hs = B.H + Row, *Av = B.A + Row;
      const Real Z0 = B.Zt[C * B.LZ + Kk], Z1 = B.Zt[C * B.LZ + Kk + 1];
      int J = Kk; // the largest J with Zs[J] <= Z0 (Zs[Lo] = 0 <= Z0)
      while (J > Lo && Zs[J] > Z0)
         --J;
      while (J < Hi && Zs[J + 1] <= Z0)
         ++J;
      const int J0  = J;
      const Real X0 = (Z0 - Zs[J0]) / Hs[J0];
      Real MinA = Av[J0], MaxA = Av[J0];
      auto Widen = [&](Real V) {
         MinA = V < MinA ? V : MinA;
         MaxA = V > MaxA ? V : MaxA;
      };
      if (J0 > Lo)
         Widen(Av[J0 - 1]);
      Real Res, AL, Dl, A6;
      if (Z1 <= Z0) { // no width: the point value
         cellCoeffs<Order>(B, Row + J0, AL, Dl, A6);
         Res = AL + X0 * (Dl + A6 * (1.0 - X0));
      } else {
         Real Sum   = 0.0;
         bool Whole = false;
         for (;; ++J) {
            const bool Last = J == Hi || !(Zs[J + 1] < Z1);
            const Real Xa   = J == J0 ? X0 : 0.0;
            const Real Xb   = Last ? (Z1 == Zs[J + 1] ? 1.0 : (Z1 - Zs[J]) / Hs[J]) : 1.0;
            Widen(Av[J]);
            Real Piece;
            if (Xa == 0.0 && Xb == 1.0) {
               Piece = Hs[J] * Av[J];
               Whole = J == J0 && Last;
            } else {
               cellCoeffs<Order>(B, Row + J, AL, Dl, A6);
               Piece = Hs[J] * ((AL * (Xb - Xa) + (0.5 * (Dl + A6)) * ((Xb * Xb) - (Xa * Xa))) -
                                (A6 / 3.0) * (((Xb * Xb) * Xb) - ((Xa * Xa) * Xa)));
            }
            Sum = Sum + Piece;
            if (Last)
               break;
         }
         Res = Whole ? Av[J0] : Sum / (Z1 - Z0);
      }
      if (J < Hi)
         Widen(Av[J + 1]);
      Res           = Res < MinA ? MinA : Res;
      Res           = Res > MaxA ? MaxA : Res;
      B.E[Row + Kk] = Res;
   });
}

/// The column core on the plane staged in A (published by a barrier), with the interfaces scanned: the result in E,
/// behind a barrier
template <int Order> __device__ inline void remapPlane(const RemapTile &B, int Nc, int P) {
   if constexpr (Order >= 2) {
      limitedSlopes(B, Nc, P);
      __syncthreads();
   }
   if constexpr (Order == 3) {
      interfaceValues(B, Nc, P);
      __syncthreads();
      limitedParabolas(B, Nc, P);
      __syncthreads();
   }
   overlapSums<Order>(B, Nc, P);
   __syncthreads();
}

// ------------------------------------------------------------------------------------------------------ cell launch
template <int Order, bool DoTarget>
__global__ void __launch_bounds__(ColThreads) vertRemapCellKernel(VertRemapCellArgs A, int P, int Tile) {
   extern __shared__ Real Lds[];
   const int C0      = blockIdx.x * Tile;
   const int Nc      = min(Tile, A.NCellsAll - C0);
   const RemapTile B = carveTile(Lds, Tile, P);

   stageRanges(A.MinLayerCell, A.MaxLayerCell, C0, Nc, A.K, B.Lo, B.Hi);
   const AllLevels All;
   loadTile(A.LayerThick, P, C0, Nc, B.H, B.LP, All);
   loadTile(DoTarget ? A.RefThick : A.Target, P, C0, Nc, B.T, B.LP, All);
   __syncthreads();
   const InRange Active{B.Lo, B.Hi};

   if (DoTarget) {
      const int C = threadIdx.x;
      if (C < Nc && B.Lo[C] <= B.Hi[C]) {
         const Real *Hs = B.H + C * B.LP, *R = B.T + C * B.LP;
         Real SumH = 0.0, SumRef = 0.0, SumWh = 0.0;
         for (int Kk = B.Lo[C]; Kk <= B.Hi[C]; ++Kk) {
            SumH   = SumH + Hs[Kk];
            SumWh  = SumWh + A.MoveWeights[Kk] * R[Kk];
            SumRef = SumRef + R[Kk];
         }
         B.Sc0[C] = SumH - SumRef;
         B.Sc1[C] = SumWh;
      }
      __syncthreads();
      forActive(B, Nc, P, [&](int Cc, int Kk) {
         const int O = Cc * B.LP + Kk;
         B.T[O]      = B.T[O] * (1.0 + (B.Sc0[Cc] * A.MoveWeights[Kk]) / B.Sc1[Cc]);
      });
      __syncthreads();
      storeTile(A.Target, P, C0, Nc, B.T, B.LP, Active);
   }
   if (A.NTracers <= 0)
      return;

   scanInterfaces(B, Nc); // (published by the barrier behind the first plane's load)
   const size_t Plane = (size_t)A.NCellsSize * P;
   for (int Tr = 0; Tr < A.NTracers; ++Tr) {
      Real *G = A.Tracers + Tr * Plane;
      loadTile(G, P, C0, Nc, B.A, B.LP, All);
      __syncthreads();
      remapPlane<Order>(B, Nc, P);
      storeTile(G, P, C0, Nc, B.E, B.LP, Active);
   }
}

// ------------------------------------------------------------------------------------------------------ edge launch
template <int Order>
__global__ void __launch_bounds__(ColThreads) vertRemapEdgeKernel(VertRemapEdgeArgs A, int P, int Tile) {
   extern __shared__ Real Lds[];
   const int E0      = blockIdx.x * Tile;
   const int Nc      = min(Tile, A.NEdgesAll - E0);
   const RemapTile B = carveTile(Lds, Tile, P);
   const int Tid     = threadIdx.x;

   // an edge with an invalid range or a cell outside [0, NCellsSize) gets the empty range [1, -1]: it is left alone
   if (Tid < Nc) {
      const size_t E = (size_t)E0 + Tid;
      int Ca = A.CellsOnEdge[2 * E], Cb = A.CellsOnEdge[2 * E + 1];
      int L = A.MinLayerEdgeBot[E], H = A.MaxLayerEdgeTop[E];
      if (!(L >= 0 && L <= H && H < A.K) || Ca < 0 || Ca >= A.NCellsSize || Cb < 0 || Cb >= A.NCellsSize)
         L = 1, H = -1, Ca = 0, Cb = 0;
      B.Lo[Tid] = L, B.Hi[Tid] = H, B.Ca[Tid] = Ca, B.Cb[Tid] = Cb;
   }
   __syncthreads();
   forActive(B, Nc, P, [&](int C, int Kk) {
      const size_t Ra = (size_t)B.Ca[C] * P + Kk, Rb = (size_t)B.Cb[C] * P + Kk;
      const int O = C * B.LP + Kk;
      B.H[O]      = 0.5 * (A.LayerThick[Ra] + A.LayerThick[Rb]);
      B.T[O]      = 0.5 * (A.Target[Ra] + A.Target[Rb]);
   });
   const AllLevels All;
   loadTile(A.NormalVelocity, P, E0, Nc, B.A, B.LP, All);
   __syncthreads();
   scanInterfaces(B, Nc);
   __syncthreads();
   remapPlane<Order>(B, Nc, P);
   storeTile(A.NormalVelocity, P, E0, Nc, B.E, B.LP, InRange{B.Lo, B.Hi});
}

// --------------------------------------------------------------------------------------------------------- adoption
template <class T>
__global__ void __launch_bounds__(RowBlock) vertRemapAdoptKernel(VertRemapAdoptArgs A, int Pitch) {
   __shared__ int Lo[RowTile], Hi[RowTile];
   const int First = blockIdx.x * RowTile;
   int Cnt         = A.NCellsAll - First;
   if (Cnt > RowTile)
      Cnt = RowTile;
   stageRanges(A.MinLayerCell, A.MaxLayerCell, First, Cnt, A.K, Lo, Hi);
   __syncthreads();
   forLevelRuns<T>(Cnt, Pitch, Lo, Hi, [&](int Le, int K0, int L, int H) {
      const size_t R = (size_t)(First + Le) * Pitch + K0;
      storeRanged<T>(A.LayerThick + R, *reinterpret_cast<const T *>(A.Target + R), K0, L, H);
   });
}

template <class F> void withOrder(int Order, F &&Fn) {
   if (Order == 1)
      Fn(std::integral_constant<int, 1>());
   else if (Order == 2)
      Fn(std::integral_constant<int, 2>());
   else
      Fn(std::integral_constant<int, 3>());
}

} // namespace

int vertRemapColumnTile(int K) {
   const int P = levelPitch(K);
   return pickColumnTile([&](int T) { return remapLdsDoubles(T, ldsPitch(P), ifacePitch(P)); });
}

void launchVertRemapCell(const VertRemapCellArgs &A, bool DoTarget, hipStream_t S) {
   if (A.NCellsAll <= 0 || A.K <= 0 || !(DoTarget || A.NTracers > 0))
      return;
   OMEGA_REQUIRE(A.Order >= 1 && A.Order <= 3, "VertRemap cell kernel: Order " + std::to_string(A.Order) + " is not 1 .. 3");
   const int Tile = vertRemapColumnTile(A.K);
   OMEGA_REQUIRE(Tile >= 2, "VertRemap cell kernel: NVertLayers " + std::to_string(A.K) + " is too long for the LDS tile");
   const int P        = levelPitch(A.K);
   const size_t Bytes = remapLdsDoubles(Tile, ldsPitch(P), ifacePitch(P)) * sizeof(Real);
   const dim3 Grid((A.NCellsAll + Tile - 1) / Tile), Block(ColThreads);
   withOrder(A.Order, [&](auto O) {
      constexpr int Order = decltype(O)::value;
      if (DoTarget)
         hipLaunchKernelGGL((vertRemapCellKernel<Order, true>), Grid, Block, Bytes, S, A, P, Tile);
      else
         hipLaunchKernelGGL((vertRemapCellKernel<Order, false>), Grid, Block, Bytes, S, A, P, Tile);
   });
   HIP_CHECK(hipGetLastError());
}

void launchVertRemapEdge(const VertRemapEdgeArgs &A, hipStream_t S) {
   if (A.NEdgesAll <= 0 || A.K <= 0)
      return;
   OMEGA_REQUIRE(A.Order >= 1 && A.Order <= 3, "VertRemap edge kernel: Order " + std::to_string(A.Order) + " is not 1 .. 3");
   const int Tile = vertRemapColumnTile(A.K);
   OMEGA_REQUIRE(Tile >= 2, "VertRemap edge kernel: NVertLayers " + std::to_string(A.K) + " is too long for the LDS tile");
   const int P        = levelPitch(A.K);
   const size_t Bytes = remapLdsDoubles(Tile, ldsPitch(P), ifacePitch(P)) * sizeof(Real);
   const dim3 Grid((A.NEdgesAll + Tile - 1) / Tile), Block(ColThreads);
   withOrder(A.Order, [&](auto O) {
      hipLaunchKernelGGL((vertRemapEdgeKernel<decltype(O)::value>), Grid, Block, Bytes, S, A, P, Tile);
   });
   HIP_CHECK(hipGetLastError());
}

void launchVertRemapAdopt(const VertRemapAdoptArgs &A, hipStream_t S) {
   if (A.NCellsAll <= 0 || A.K <= 0)
      return;
   const int Pitch = levelPitch(A.K);
   const dim3 Grid((A.NCellsAll + RowTile - 1) / RowTile), Block(RowBlock);
   withLaneType(Pitch, [&](auto Lane) {
      hipLaunchKernelGGL(vertRemapAdoptKernel<decltype(Lane)>, Grid, Block, 0, S, A, Pitch);
   });
   HIP_CHECK(hipGetLastError());
}

} // namespace OMEGA
