// RediKernels.h -- host-callable launchers of the three kernels behind Redi (kernels/RediKernels.hip).  Asynchronous on
// the given stream, raw device pointers, allocate nothing.  Level-indexed arrays are [rows][Pitch] with Pitch =
// levelPitch(K).  The numerical contract is written down in Redi.h.
#ifndef OMEGA_AMD_REDIKERNELS_H
#define OMEGA_AMD_REDIKERNELS_H

#include "PackedColumns.h"

namespace OMEGA {

/// Everything one slope launch reads and writes (Redi::computeSlope)
struct RediSlopeArgs : EdgeColumnArgs {
   Real SlopeMax = 0, N2Floor = 0;
   Real *SlopeInterface = nullptr; ///< [edge][Pitch]
};
void launchRediSlope(const RediSlopeArgs &A, hipStream_t S);

/// The mesh tables and layer ranges the two cell launches stage (Redi::addTracerTend, Redi::computeVertDiffusivity).
struct RediCellArgs {
   int NCellsAll = 0, NCellsSize = 0, NEdgesAll = 0, K = 0, MaxEdges = 0;
   const I4 *NEdgesOnCell = nullptr, *EdgesOnCell = nullptr; ///< [cell], [cell][MaxEdges]
   const I4 *CellsOnEdge = nullptr;                          ///< [edge][2]
   const Real *EdgeSignOnCell = nullptr;                     ///< [cell][MaxEdges]
   const Real *AreaCell = nullptr, *DcEdge = nullptr, *DvEdge = nullptr, *Kappa = nullptr;
   const I4 *MinLayerCell = nullptr, *MaxLayerCell = nullptr;       ///< [cell]
   const I4 *MinLayerEdgeBot = nullptr, *MaxLayerEdgeTop = nullptr; ///< [edge]
   const Real *SlopeInterface = nullptr;                            ///< [edge][Pitch]
   // addTracerTend
   const Real *LayerThickness = nullptr, *ZMid = nullptr; ///< [cell][Pitch]
   const Real *Tracers = nullptr;                         ///< [tracer][TrRows][Pitch]
   Real *Tend = nullptr;                                  ///< [tracer][TendRows][Pitch], accumulated
   int NTracers = 0, TrRows = 0, TendRows = 0;
   // computeVertDiffusivity
   Real *VertDiffusivity = nullptr; ///< [cell][Pitch]
   Real *VertDiff = nullptr;        ///< [cell][Pitch], accumulated; null: no term
};
void launchRediTracerTend(const RediCellArgs &A, hipStream_t S);
void launchRediVertDiffusivity(const RediCellArgs &A, hipStream_t S);

} // namespace OMEGA
#endif
