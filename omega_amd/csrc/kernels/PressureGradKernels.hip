// PressureGradKernels.hip -- the pressure-gradient kernel behind PressureGrad (PressureGrad.h) on gfx950.
//
// The level-row tile of LevelTile.h over edges: a workgroup owns RowTile consecutive edges.  It stages the tile's
// per-edge scalars into LDS once -- the two cells, the level range, the mask (stageEdgeTile) and 1/Dc (the only division,
// once per edge) -- and then sweeps the tile's rows with the lanes along the levels: with an even row pitch a lane owns
// two adjacent levels and moves them as one 16-byte access, so 8 consecutive lanes cover one 128-byte line of a row and
// a wave reads whole runs of each gathered cell row (rows of K >= 16 levels start on line boundaries, Base.h:
// levelPitch).  An odd pitch (odd K < 16) takes the same code with one level per lane.  One thread owns (edge, level):
// no atomics.  A level pair that straddles the end of an edge's range is computed whole and stored one value wide, so
// nothing outside the range is written.
//
// Tiles are handed out through xcdRemap (KernelCommon.h): the workgroups that share an XCD walk one contiguous eighth
// of the edge numbering.  In the k-d order of the mesh consecutive edges lie next to each other, so the cell rows that
// neighbouring edges gather are re-read from that XCD's L2 instead of from HBM.
#include "LevelTile.h"
#include "PressureGradKernels.h"

namespace OMEGA {

namespace {

template <class T>
__global__ void __launch_bounds__(RowBlock) pressureGradKernel(PressureGradArgs A, int Pitch, int NTiles) {
   __shared__ Real InvDc[RowTile];
   const EdgeTile E = stageEdgeTile(A, NTiles, [&](int Le, int Edge) { InvDc[Le] = 1.0 / A.DcEdge[Edge]; });
   forLevelRuns<T>(E.Cnt, Pitch, E.Lo, E.Hi, [&](int Le, int K0, int L, int H) {
      const size_t R0 = (size_t)E.Cell0[Le] * Pitch + K0, R1 = (size_t)E.Cell1[Le] * Pitch + K0;
      const T Geo0 = *reinterpret_cast<const T *>(A.GeopotentialMid + R0);
      const T Geo1 = *reinterpret_cast<const T *>(A.GeopotentialMid + R1);
      const T P0   = *reinterpret_cast<const T *>(A.PressureMid + R0);
      const T P1   = *reinterpret_cast<const T *>(A.PressureMid + R1);
      const T Sv0  = *reinterpret_cast<const T *>(A.SpecVol + R0);
      const T Sv1  = *reinterpret_cast<const T *>(A.SpecVol + R1);
      Real *Out    = A.Tend + (size_t)(E.First + Le) * Pitch + K0;
      const T In   = *reinterpret_cast<const T *>(Out);
      const T Inv = splat<T>(InvDc[Le]), M = splat<T>(E.Mask[Le]);
      const T GradGeo = (Geo1 - Geo0) * Inv;
      const T GradP   = (P1 - P0) * Inv;
      const T AlphaE  = splat<T>(0.5) * (Sv0 + Sv1);
      const T Res     = In - M * (GradGeo + AlphaE * GradP);
      storeRanged<T>(Out, Res, K0, L, H);
   });
}

} // namespace

void launchPressureGrad(const PressureGradArgs &A, hipStream_t S) {
   if (A.NEdgesAll <= 0 || A.K <= 0)
      return;
   const int Pitch  = levelPitch(A.K);
   const int NTiles = (A.NEdgesAll + RowTile - 1) / RowTile;
   withLaneType(Pitch, [&](auto Lane) {
      hipLaunchKernelGGL(pressureGradKernel<decltype(Lane)>, dim3(NTiles), dim3(RowBlock), 0, S, A, Pitch, NTiles);
   });
   HIP_CHECK(hipGetLastError());
}

} // namespace OMEGA
