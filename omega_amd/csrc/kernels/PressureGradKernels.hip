// PressureGradKernels.hip -- the pressure-gradient kernel behind PressureGrad (PressureGrad.h) on gfx950.
//
// A workgroup owns a tile of PGradTile consecutive edges.  It stages the tile's per-edge scalars into LDS once -- the two
// cells, the level range, the mask and 1/Dc (the only division, once per edge) -- and then sweeps the tile's rows with
// the lanes along the levels: with an even row pitch a lane owns two adjacent levels and moves them as one 16-byte
// access, so 8 consecutive lanes cover one 128-byte line of a row and a wave reads whole runs of each gathered cell row
// (rows of K >= 16 levels start on line boundaries, Base.h: levelPitch).  An odd pitch (odd K < 16) takes the same code
// with one level per lane.  One thread owns (edge, level): no atomics.  A level pair that straddles the end of an
// edge's range is computed whole and stored one value wide, so nothing outside the range is written.
//
// Tiles are handed out through xcdRemap (KernelCommon.h): the workgroups that share an XCD walk one contiguous eighth
// of the edge numbering.  In the k-d order of the mesh consecutive edges lie next to each other, so the cell rows that
// neighbouring edges gather are re-read from that XCD's L2 instead of from HBM.
#include "KernelCommon.h"
#include "PressureGradKernels.h"

namespace OMEGA {

namespace {

constexpr int PGradBlock = 256;
constexpr int PGradTile  = 32; // edges per workgroup

template <class T>
__global__ void __launch_bounds__(PGradBlock) pressureGradKernel(PressureGradArgs A, int Pitch, int NTiles) {
   constexpr int W = VecW<T>::W;
   __shared__ int Cell0[PGradTile], Cell1[PGradTile], Lo[PGradTile], Hi[PGradTile];
   __shared__ Real Mask[PGradTile], InvDc[PGradTile];
   const int First = xcdRemap(blockIdx.x, NTiles) * PGradTile;
   int Cnt         = A.NEdgesAll - First;
   if (Cnt > PGradTile)
      Cnt = PGradTile;
   const int Tid = threadIdx.x;
   if (Tid < Cnt) {
      const int E  = First + Tid;
      const int C0 = A.CellsOnEdge[2 * (size_t)E], C1 = A.CellsOnEdge[2 * (size_t)E + 1];
      int L = A.MinLayerEdgeBot[E], H = A.MaxLayerEdgeTop[E];
      if (!(L >= 0 && L <= H && H < A.K) || C0 < 0 || C0 >= A.NCellsSize || C1 < 0 || C1 >= A.NCellsSize)
         L = A.K, H = -1; // an empty range: the edge is left alone
      Cell0[Tid] = C0, Cell1[Tid] = C1, Lo[Tid] = L, Hi[Tid] = H;
      Mask[Tid]  = A.EdgeMask[E];
      InvDc[Tid] = 1.0 / A.DcEdge[E];
   }
   __syncthreads();
   const int Lanes = Pitch / W; // lanes along one row
   for (int Idx = Tid; Idx < Cnt * Lanes; Idx += PGradBlock) {
      const int Le = Idx / Lanes;
      const int K0 = (Idx - Le * Lanes) * W;
      const int L = Lo[Le], H = Hi[Le];
      if (K0 + W - 1 < L || K0 > H)
         continue;
      const size_t R0 = (size_t)Cell0[Le] * Pitch + K0, R1 = (size_t)Cell1[Le] * Pitch + K0;
      const T Geo0 = *reinterpret_cast<const T *>(A.GeopotentialMid + R0);
      const T Geo1 = *reinterpret_cast<const T *>(A.GeopotentialMid + R1);
      const T P0   = *reinterpret_cast<const T *>(A.PressureMid + R0);
      const T P1   = *reinterpret_cast<const T *>(A.PressureMid + R1);
      const T Sv0  = *reinterpret_cast<const T *>(A.SpecVol + R0);
      const T Sv1  = *reinterpret_cast<const T *>(A.SpecVol + R1);
      Real *Out    = A.Tend + (size_t)(First + Le) * Pitch + K0;
      const T In   = *reinterpret_cast<const T *>(Out);
      const T Inv = splat<T>(InvDc[Le]), M = splat<T>(Mask[Le]);
      const T GradGeo = (Geo1 - Geo0) * Inv;
      const T GradP   = (P1 - P0) * Inv;
      const T AlphaE  = splat<T>(0.5) * (Sv0 + Sv1);
      const T Res     = In - M * (GradGeo + AlphaE * GradP);
      if constexpr (W == 2) {
         const bool In0 = K0 >= L, In1 = K0 + 1 <= H; // (the pair overlaps the range: K0 <= H and K0 + 1 >= L)
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

void launchPressureGrad(const PressureGradArgs &A, hipStream_t S) {
   if (A.NEdgesAll <= 0 || A.K <= 0)
      return;
   const int Pitch  = levelPitch(A.K);
   const int NTiles = (A.NEdgesAll + PGradTile - 1) / PGradTile;
   if (Pitch % 2 == 0)
      hipLaunchKernelGGL(pressureGradKernel<dv2>, dim3(NTiles), dim3(PGradBlock), 0, S, A, Pitch, NTiles);
   else
      hipLaunchKernelGGL(pressureGradKernel<double>, dim3(NTiles), dim3(PGradBlock), 0, S, A, Pitch, NTiles);
   HIP_CHECK(hipGetLastError());
}

} // namespace OMEGA
