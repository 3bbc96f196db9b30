// PressureGradKernels.h -- host-callable launcher of the pressure-gradient kernel behind PressureGrad
// (kernels/PressureGradKernels.hip).  Asynchronous on the given stream, raw device pointers, allocates nothing.
// Level-indexed arrays are [rows][Pitch] with Pitch = levelPitch(K).  The numerical contract is written down in
// PressureGrad.h.
#ifndef OMEGA_AMD_PRESSUREGRADKERNELS_H
#define OMEGA_AMD_PRESSUREGRADKERNELS_H

#include "../Base.h"

namespace OMEGA {

/// Everything one pressure-gradient launch reads and writes (PressureGrad::computePressureGrad).
struct PressureGradArgs {
   int NEdgesAll = 0, NCellsSize = 0, K = 0;
   const I4 *CellsOnEdge = nullptr;          ///< [edge][2]
   const I4 *MinLayerEdgeBot = nullptr, *MaxLayerEdgeTop = nullptr; ///< [edge] level range of the term
   const Real *DcEdge = nullptr, *EdgeMask = nullptr;               ///< [edge]
   const Real *PressureMid = nullptr, *GeopotentialMid = nullptr, *SpecVol = nullptr; ///< [cell][Pitch]
   Real *Tend = nullptr;                                                               ///< [edge][Pitch], accumulated
};
void launchPressureGrad(const PressureGradArgs &A, hipStream_t S);

} // namespace OMEGA
#endif
