// PackedColumns.h -- what the kernels with "lanes along the rows of a column" share, inline like LevelTile.h and with no
// kernel of its own: the PCR array launcher (kernels/TriDiagKernels.hip), the implicit mixing solves
// (kernels/VertMixKernels.hip), the bolus-velocity kernel (kernels/GMKernels.hip) and the slope kernel
// (kernels/RediKernels.hip).
//
// The shape: row I of a column of at most K rows on lane I, floor(256 / K) columns side by side in a workgroup (one for
// K > 256, up to TriDiagMaxRows lanes), so a column's row of each array is one coalesced run.  Columns of one workgroup
// may differ in depth: packedLevels() agrees on the PCR level count the whole workgroup barriers for.
//
// The edge columns: the bolus-velocity and the slope kernel read the same stratification of the two cells of an edge
// and form the same interface quantities of GentMcWilliams.h's contract from it; the one copy here is what makes the
// slope's GradRhoZ and N2E the bits of the bolus velocity's.
#ifndef OMEGA_AMD_PACKEDCOLUMNS_H
#define OMEGA_AMD_PACKEDCOLUMNS_H

#include "TriDiagKernels.h"

#include <string>

namespace OMEGA {

constexpr int PackedLanes = 256; ///< lanes a workgroup of short columns fills

/// Columns per workgroup and the lanes they occupy, for columns of at most K rows; the kernels take it by value
struct PackedShape {
   int Sys, Rows, Threads;
   explicit PackedShape(int K) {
      Sys     = K <= PackedLanes ? PackedLanes / K : 1;
      Rows    = Sys * K;
      Threads = (Rows + 63) / 64 * 64;
   }
   /// workgroups for NCols columns
   dim3 grid(int NCols) const { return dim3((NCols + Sys - 1) / Sys); }
};

/// The launchers' refusal of a K the shape does not hold, under the calling class's name
inline void requirePackedLayers(const char *Class, int K) {
   OMEGA_REQUIRE(K >= 1 && K <= TriDiagMaxRows, std::string(Class) + ": NVertLayers = " + std::to_string(K) +
                                                    " is outside the supported 1 <= NVertLayers <= " +
                                                    std::to_string(TriDiagMaxRows));
}

/// A lane's place: row I of system S of its workgroup, column Col of all NCols; InSys: the lane has a column
struct PackedLane {
   int S, I;
   long Col;
   bool InSys;
};
__device__ inline PackedLane packedLane(const PackedShape &P, int K, int NCols) {
   const int T = threadIdx.x;
   PackedLane L;
   L.S     = T / K;
   L.I     = T - L.S * K;
   L.Col   = (long)blockIdx.x * P.Sys + L.S;
   L.InSys = T < P.Rows && L.Col < NCols;
   return L;
}

/// Rows of a column with the level range Lo .. Hi of K levels; 0 for a range that is not 0 <= Lo <= Hi < K
__device__ inline int packedRows(int Lo, int Hi, int K) { return (Lo >= 0 && Lo <= Hi && Hi < K) ? Hi - Lo + 1 : 0; }

/// The workgroup-uniform PCR level count: the largest pcrLevels(NRow) among the systems of the workgroup.  Every lane
/// calls it (two barriers); Lead: the lane of row 0 of a system, which reports its system's NRow.
__device__ inline int packedLevels(bool Lead, int NRow) {
   __shared__ int NLevShared;
   if (threadIdx.x == 0)
      NLevShared = 0;
   __syncthreads();
   if (Lead && NRow > 0)
      atomicMax(&NLevShared, pcrLevels(NRow));
   __syncthreads();
   return NLevShared;
}

// ---------------------------------------------------------------------------------------------------------------------
// edge columns: the stratification of the two cells of an edge (GentMcWilliams.h, Redi.h)
// ---------------------------------------------------------------------------------------------------------------------

/// What every launch over the edge columns reads (filled by ColumnPass::stratificationArgs)
struct EdgeColumnArgs {
   int NEdgesAll = 0, NCellsSize = 0, K = 0;
   const I4 *CellsOnEdge = nullptr;                                 ///< [edge][2]
   const I4 *MinLayerEdgeBot = nullptr, *MaxLayerEdgeTop = nullptr; ///< [edge] level range of the edge column
   const Real *DcEdge = nullptr;                                    ///< [edge]
   Real GOverRho0 = 0;                                              ///< g / Rho0, evaluated by the caller
   const Real *SpecVol = nullptr, *SpecVolDisplaced = nullptr, *ZMid = nullptr; ///< [cell][Pitch]
};

/// An edge column: layers Lo .. Lo + N - 1 between the cells C0 and C1.  N = 0 (the edge is left alone) without a
/// column, for a level range that is not 0 <= Lo <= Hi < K and for a cell outside [0, NCellsSize), as stageEdgeTile
/// (LevelTile.h) has it.
struct EdgeColumn {
   int Lo = 0, N = 0, C0 = 0, C1 = 0;
};
__device__ inline EdgeColumn edgeColumn(const EdgeColumnArgs &A, const PackedLane &L) {
   EdgeColumn E;
   if (L.InSys) {
      E.Lo         = A.MinLayerEdgeBot[L.Col];
      const int Hi = A.MaxLayerEdgeTop[L.Col];
      E.C0 = A.CellsOnEdge[2 * L.Col], E.C1 = A.CellsOnEdge[2 * L.Col + 1];
      // (the range first: the three loads are then issued together, none behind a branch on another)
      const int N = packedRows(E.Lo, Hi, A.K);
      if (N > 0 && E.C0 >= 0 && E.C0 < A.NCellsSize && E.C1 >= 0 && E.C1 < A.NCellsSize)
         E.N = N;
   }
   return E;
}

constexpr int EdgeLayerArrays = 6; ///< LDS doubles per lane of the exchange below

/// What the interface below a layer needs of it: the densities, heights and displaced densities of the two cells
struct EdgeLayer {
   Real Rho0 = 0, Rho1 = 0, Z0 = 0, Z1 = 0, Rd0 = 0, Rd1 = 0, InvDc = 0;
};
/// Layer Lev of the two cells, at P0 / P1 = cell * Pitch + Lev.  Bottom: the column's last layer, whose displaced
/// volume is not part of the contract (it may be unset) and is not read.
__device__ inline EdgeLayer loadEdgeLayer(const EdgeColumnArgs &A, long Col, size_t P0, size_t P1, bool Bottom) {
   EdgeLayer V;
   V.Rho0  = 1.0 / A.SpecVol[P0];
   V.Rho1  = 1.0 / A.SpecVol[P1];
   V.Z0    = A.ZMid[P0];
   V.Z1    = A.ZMid[P1];
   V.InvDc = 1.0 / A.DcEdge[Col];
   if (!Bottom) {
      V.Rd0 = 1.0 / A.SpecVolDisplaced[P0];
      V.Rd1 = 1.0 / A.SpecVolDisplaced[P1];
   }
   return V;
}
/// The hand-off to the lane below: lane T's six values into arrays 0 .. 5 of `Rows` doubles; the caller barriers
__device__ inline void storeEdgeLayer(const EdgeLayer &V, Real *Lds, int Rows, int T) {
   Lds[0 * Rows + T] = V.Rho0, Lds[1 * Rows + T] = V.Rho1, Lds[2 * Rows + T] = V.Z0, Lds[3 * Rows + T] = V.Z1;
   Lds[4 * Rows + T] = V.Rd0, Lds[5 * Rows + T] = V.Rd1;
}

/// The interface at the top of a layer, in the contract's order (GentMcWilliams.h)
struct EdgeInterface {
   Real GradRhoZ; ///< the density gradient at constant z
   Real N2E;      ///< clipped at 0
   Real GradZE;   ///< 0.5 * (GradZ[K-1] + GradZ[K]): the slope of the layer
};
/// From this lane's layer V and the layer above it, which lane U = T - 1 stored
__device__ inline EdgeInterface edgeInterface(const EdgeLayer &V, const Real *Lds, int Rows, int U, Real GR) {
   const Real Rho0u = Lds[0 * Rows + U], Rho1u = Lds[1 * Rows + U], Z0u = Lds[2 * Rows + U], Z1u = Lds[3 * Rows + U];
   const Real Rd0u = Lds[4 * Rows + U], Rd1u = Lds[5 * Rows + U];
   const Real GradRho = (V.Rho1 - V.Rho0) * V.InvDc, GradRhoU = (Rho1u - Rho0u) * V.InvDc;
   const Real GradZ = (V.Z1 - V.Z0) * V.InvDc, GradZU = (Z1u - Z0u) * V.InvDc;
   const Real Dz0 = Z0u - V.Z0, Dz1 = Z1u - V.Z1;
   const Real RhoZ0 = (Rho0u - V.Rho0) / Dz0, RhoZ1 = (Rho1u - V.Rho1) / Dz1;
   const Real N20 = (GR * (V.Rho0 - Rd0u)) / Dz0, N21 = (GR * (V.Rho1 - Rd1u)) / Dz1;
   const Real RhoZE = 0.5 * (RhoZ0 + RhoZ1);
   EdgeInterface F;
   F.N2E      = 0.5 * (N20 + N21);
   F.N2E      = F.N2E < 0.0 ? 0.0 : F.N2E;
   F.GradZE   = 0.5 * (GradZU + GradZ);
   F.GradRhoZ = 0.5 * (GradRhoU + GradRho) - RhoZE * F.GradZE;
   return F;
}

} // namespace OMEGA
#endif
