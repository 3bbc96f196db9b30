// GMKernels.h -- host-callable launcher of the eddy bolus-velocity kernel behind GentMcWilliams (kernels/GMKernels.hip).
// Asynchronous on the given stream, raw device pointers, allocates nothing.  Level-indexed arrays are [rows][Pitch] with
// Pitch = levelPitch(K).  The numerical contract is written down in GentMcWilliams.h.
#ifndef OMEGA_AMD_GMKERNELS_H
#define OMEGA_AMD_GMKERNELS_H

#include "../Base.h"

namespace OMEGA {

/// Everything one bolus-velocity launch reads and writes (GentMcWilliams::computeBolusVelocity).
struct GMArgs {
   int NEdgesAll = 0, K = 0;
   const I4 *CellsOnEdge = nullptr;                                 ///< [edge][2]
   const I4 *MinLayerEdgeBot = nullptr, *MaxLayerEdgeTop = nullptr; ///< [edge] level range of the edge column
   const Real *DcEdge = nullptr, *Kappa = nullptr;                  ///< [edge]
   Real C2 = 0, GOverRho0 = 0; ///< GravWaveSpeed * GravWaveSpeed and g / Rho0, evaluated by the caller
   const Real *LayerThickness = nullptr, *SpecVol = nullptr, *SpecVolDisplaced = nullptr, *ZMid = nullptr; ///< [cell][Pitch]
   Real *BolusVelocity = nullptr, *StreamFunction = nullptr; ///< [edge][Pitch]
   Real *Transport = nullptr;                                ///< [edge][Pitch], accumulated; null: no term
};
void launchBolusVelocity(const GMArgs &A, hipStream_t S);

} // namespace OMEGA
#endif
