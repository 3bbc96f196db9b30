// VertRemapKernels.h -- host-callable launchers of the kernels behind VertRemap (kernels/VertRemapKernels.hip).
// Asynchronous on the given stream, raw device pointers, allocate nothing.  Level-indexed arrays are [rows][Pitch] with
// Pitch = levelPitch(K).  The numerical contract is written down in VertRemap.h.
#ifndef OMEGA_AMD_VERTREMAPKERNELS_H
#define OMEGA_AMD_VERTREMAPKERNELS_H

#include "../Base.h"

namespace OMEGA {

/// columns per workgroup of the two column launches at K levels (16, 8, 4 or 2), 0 if K is too long for the LDS tile
int vertRemapColumnTile(int K);

/// The cell launch: the target thickness (DoTarget), the remap of NTracers tracer planes, or both in one launch
struct VertRemapCellArgs {
   int NCellsAll = 0, NCellsSize = 0, K = 0, NTracers = 0, Order = 3;
   const I4 *MinLayerCell = nullptr, *MaxLayerCell = nullptr; ///< [cell]
   const Real *MoveWeights = nullptr;                         ///< [K]
   const Real *RefThick = nullptr;                            ///< [cell][Pitch]
   const Real *LayerThick = nullptr;                          ///< [cell][Pitch]
   Real *Target = nullptr;  ///< [cell][Pitch]: written with DoTarget, read without
   Real *Tracers = nullptr; ///< [tracer][NCellsSize][Pitch], in place
};
void launchVertRemapCell(const VertRemapCellArgs &A, bool DoTarget, hipStream_t S);

struct VertRemapEdgeArgs {
   int NEdgesAll = 0, NCellsSize = 0, K = 0, Order = 3;
   const I4 *CellsOnEdge = nullptr;                                 ///< [edge][2]
   const I4 *MinLayerEdgeBot = nullptr, *MaxLayerEdgeTop = nullptr; ///< [edge] level range of the edge column
   const Real *LayerThick = nullptr, *Target = nullptr;             ///< [cell][Pitch]
   Real *NormalVelocity = nullptr;                                  ///< [edge][Pitch], in place
};
void launchVertRemapEdge(const VertRemapEdgeArgs &A, hipStream_t S);

struct VertRemapAdoptArgs {
   int NCellsAll = 0, K = 0;
   const I4 *MinLayerCell = nullptr, *MaxLayerCell = nullptr; ///< [cell]
   const Real *Target = nullptr;                              ///< [cell][Pitch]
   Real *LayerThick = nullptr;                                ///< [cell][Pitch]
};
void launchVertRemapAdopt(const VertRemapAdoptArgs &A, hipStream_t S);

} // namespace OMEGA
#endif
