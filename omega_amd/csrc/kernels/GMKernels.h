// GMKernels.h -- host-callable launcher of the eddy bolus-velocity kernel behind GentMcWilliams (kernels/GMKernels.hip).
// Asynchronous on the given stream, raw device pointers, allocates nothing.  Level-indexed arrays are [rows][Pitch] with
// Pitch = levelPitch(K).  The numerical contract is written down in GentMcWilliams.h.
#ifndef OMEGA_AMD_GMKERNELS_H
#define OMEGA_AMD_GMKERNELS_H

#include "PackedColumns.h"

namespace OMEGA {

/// Everything one bolus-velocity launch reads and writes (GentMcWilliams::computeBolusVelocity)
struct GMArgs : EdgeColumnArgs {
   const Real *Kappa = nullptr;          ///< [edge]
   Real C2 = 0;                          ///< GravWaveSpeed * GravWaveSpeed, evaluated by the caller
   const Real *LayerThickness = nullptr; ///< [cell][Pitch]
   Real *BolusVelocity = nullptr, *StreamFunction = nullptr; ///< [edge][Pitch]
   Real *Transport = nullptr;                                ///< [edge][Pitch], accumulated; null: no term
};
void launchBolusVelocity(const GMArgs &A, hipStream_t S);

} // namespace OMEGA
#endif
