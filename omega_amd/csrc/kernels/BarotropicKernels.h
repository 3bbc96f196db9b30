// BarotropicKernels.h -- host-callable launchers of the kernels behind BarotropicMode (kernels/BarotropicKernels.hip).
// Asynchronous on the given stream, raw device pointers, allocate nothing.  Level-indexed arrays are [rows][Pitch] with
// Pitch = levelPitch(K).  The numerical contract is written down in BarotropicMode.h.
#ifndef OMEGA_AMD_BAROTROPICKERNELS_H
#define OMEGA_AMD_BAROTROPICKERNELS_H

#include "../Base.h"

namespace OMEGA {

/// What the edge part of a column launch computes
enum BtrEdgeMode : int {
   BtrEdgeNone    = 0,
   BtrEdgeSplit   = 1, ///< splitVelocity: BtrThickEdge, BtrVelocity (-> BtrOut) and BclVelocity
   BtrEdgeForcing = 2, ///< computeForcing: BtrForcing (-> BtrOut) and nothing else
};

/// The column launch: a sweep over the edges (the thickness-weighted vertical mean of an edge field) and / or one over
/// the cells (the column sum of the thickness), as workgroups of one launch.
struct BtrColumnArgs {
   int NEdgesAll = 0, NCellsAll = 0, NCellsSize = 0, K = 0;
   const I4 *CellsOnEdge = nullptr;                                 ///< [edge][2]
   const I4 *MinLayerEdgeBot = nullptr, *MaxLayerEdgeTop = nullptr; ///< [edge]
   const I4 *MinLayerCell = nullptr, *MaxLayerCell = nullptr;       ///< [cell]
   const Real *BottomDepth = nullptr;                               ///< [cell]
   const Real *LayerThick = nullptr;                                ///< [cell][Pitch]
   const Real *EdgeField = nullptr;                                 ///< [edge][Pitch]: u, or the velocity tendency
   Real *BtrThickEdge = nullptr, *BtrOut = nullptr;                 ///< [edge]
   Real *BclVelocity = nullptr;                                     ///< [edge][Pitch]
   Real *SSH = nullptr;                                             ///< [cell]
};
/// edges / cells per workgroup of the column launch at K levels (16, 8, 4 or 2), 0 if K is too long for the LDS tile
int btrColumnTile(int K);
/// Edges: what the edge half computes (BtrEdgeNone: no edge half); Cells: the SSH half.  BtrEdgeForcing with Cells is
/// not instantiated and is refused (OmegaError).
void launchBtrColumn(const BtrColumnArgs &A, BtrEdgeMode Edges, bool Cells, hipStream_t S);

struct BtrRecombineArgs {
   int NEdgesAll = 0, K = 0;
   const I4 *MinLayerEdgeBot = nullptr, *MaxLayerEdgeTop = nullptr; ///< [edge]
   const Real *BtrVelocity = nullptr;                               ///< [edge]
   const Real *BclVelocity = nullptr;                               ///< [edge][Pitch]
   Real *NormalVelocity = nullptr;                                  ///< [edge][Pitch]
};
void launchBtrRecombine(const BtrRecombineArgs &A, hipStream_t S);

/// One forward-backward sub-step: launchBtrCells (SSHNew from SSH and the old velocities), then launchBtrEdges (the new
/// velocities from the old ones and SSHNew; the flux sum).  The per-(element, slot) tables are slot-major --
/// [slot][NCellsAll] and [slot][NEdgesAll] -- so that lane i of a wavefront reads element i's entry of one slot: every
/// table is read once per sub-step in whole cache lines.
struct BtrSubArgs {
   int NCellsAll = 0, NEdgesAll = 0, MaxEdges = 0, MaxEdges2 = 0;
   Real Dt = 0, Gravity = 0;
   // cell tables
   const I4 *NEdgesOnCell = nullptr;  ///< [cell]
   const I4 *EdgeSlot = nullptr;      ///< [MaxEdges][NCellsAll]  EdgesOnCell(c, j)
   const I4 *NbrSlot = nullptr;       ///< [MaxEdges][NCellsAll]  the cell across that edge, -1 where EdgeMask is 0
   const Real *DvSignSlot = nullptr;  ///< [MaxEdges][NCellsAll]  DvEdge*EdgeSignOnCell
   const Real *InvAreaCell = nullptr; ///< [cell] 1/AreaCell
   // edge tables
   const I4 *CellsOnEdge = nullptr;   ///< [edge][2]
   const Real *EdgeMask = nullptr, *InvDcEdge = nullptr; ///< [edge]
   const I4 *NEdgesOnEdge = nullptr;  ///< [edge]
   const I4 *EoESlot = nullptr;       ///< [MaxEdges2][NEdgesAll]  EdgesOnEdge(e, j), -1 where it names no local edge
   const Real *CorSlot = nullptr;     ///< [MaxEdges2][NEdgesAll]  CorWeight(e, j)
   // fields
   const Real *BottomDepth = nullptr;                ///< [cell]
   const Real *SSH = nullptr, *Vel = nullptr;        ///< old values
   Real *SSHNew = nullptr, *VelNew = nullptr;        ///< new values (other buffers)
   const Real *Forcing = nullptr;                    ///< [edge]
   Real *FluxSum = nullptr;                          ///< [edge] accumulated
};
void launchBtrCells(const BtrSubArgs &A, hipStream_t S);
void launchBtrEdges(const BtrSubArgs &A, hipStream_t S);
/// X[i] = X[i]/Div for i < N
void launchBtrDivide(Real *X, int N, Real Div, hipStream_t S);

} // namespace OMEGA
#endif
