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
   /// computeResidualForcing: the forcing sweep with BtrTendMean as its BtrOut (the kernel of BtrEdgeForcing; the mode
   /// tells the caller's two outputs apart)
   BtrEdgeTendMean = 3,
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
/// Edges: what the edge half computes (BtrEdgeNone: no edge half); Cells: the SSH half.  BtrEdgeForcing /
/// BtrEdgeTendMean with Cells is not instantiated and is refused (OmegaError).
void launchBtrColumn(const BtrColumnArgs &A, BtrEdgeMode Edges, bool Cells, hipStream_t S);

/// The level-row launch over edges: what it writes into VelOut on each edge's range Lo .. Hi, and outside it
enum BtrLevelOp : int {
   BtrLevelRecombine = 0, ///< BclVelocity + BtrVelocity; nothing outside the range
   BtrLevelTransport = 1, ///< BclVelocity + BtrFluxMean/BtrThickEdge (one quotient per edge); VelOld outside
   /// (BclVelocity + Dt*(VelTend - BtrTendMean)) + BtrVelocity; VelOld + Dt*VelTend outside.  VelOut may be VelOld:
   /// a lane reads the levels it writes, and no others, before it writes them
   BtrLevelAdvance = 2,
};
/// "Outside" are the levels 0 <= K < A.K that are not in the range (all of them on an edge with an empty range); the
/// pitch padding is never written.  VelOld is read outside the ranges only: transport moves 16 B and advance 24 B per
/// edge-level inside them.
struct BtrLevelArgs {
   int NEdgesAll = 0, K = 0;
   Real Dt = 0;                                                     ///< advance
   const I4 *MinLayerEdgeBot = nullptr, *MaxLayerEdgeTop = nullptr; ///< [edge]
   const Real *BtrVelocity = nullptr;                               ///< [edge]  recombine, advance
   const Real *BtrFluxMean = nullptr, *BtrThickEdge = nullptr;      ///< [edge]  transport
   const Real *BtrTendMean = nullptr;                               ///< [edge]  advance
   const Real *BclVelocity = nullptr;                               ///< [edge][Pitch]
   const Real *VelOld = nullptr;                                    ///< [edge][Pitch]  transport, advance
   const Real *VelTend = nullptr;                                   ///< [edge][Pitch]  advance
   Real *VelOut = nullptr;                                          ///< [edge][Pitch]
};
void launchBtrLevels(const BtrLevelArgs &A, BtrLevelOp Op, hipStream_t S);

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
/// computeResidualForcing's edge half: Forcing[e] = TendMean[e] - EdgeMask[e]*(Cor - Gravity*((SSH[c1] - SSH[c0])*
/// InvDcEdge[e])), the bracket of launchBtrEdges at the fields A.SSH and A.Vel; TendMean[e] on an edge with EdgeMask 0,
/// which reads no cell and no neighbour.  Reads SSH, Vel and the edge tables of A; writes Forcing (not const here).
void launchBtrResidual(const BtrSubArgs &A, const Real *TendMean, Real *Forcing, hipStream_t S);
/// X[i] = X[i]/Div for i < N
void launchBtrDivide(Real *X, int N, Real Div, hipStream_t S);

} // namespace OMEGA
#endif
