// MonotoneAdvKernels.h -- host-callable launcher of the kernels behind MonotoneAdv (kernels/MonotoneAdvKernels.hip).
// Asynchronous on the given stream, raw device pointers, allocates nothing.  Level-indexed arrays are [rows][Pitch] with
// Pitch = levelPitch(K).  The numerical contract is written down in MonotoneAdv.h.
#ifndef OMEGA_AMD_MONOTONEADVKERNELS_H
#define OMEGA_AMD_MONOTONEADVKERNELS_H

#include "../Base.h"
#include "../HorzMesh.h"

namespace OMEGA {

struct MonotoneAdvArgs {
   int K = 0, NTracers = 0;
   int FluxThicknessUpwind = 0;
   Real Dt                 = 0.0;
   const Real *HOld = nullptr, *HNew = nullptr;        ///< [NCellsSize][Pitch]
   const Real *NormalVelocity = nullptr;               ///< [NEdgesSize][Pitch]
   const Real *Tracers        = nullptr;               ///< [tracer][NCellsSize][Pitch]
   Real *ScaleIn = nullptr, *ScaleOut = nullptr;       ///< [tracer][NCellsSize][Pitch]: written by launch 1, read by 2
   Real *Tend = nullptr;                               ///< [tracer][NCellsSize][Pitch], accumulated by launch 2
   /// the 3-D form (MonotoneAdv::attachVertAdv): all three set, or all three null for the horizontal form
   const Real *VerticalTransport = nullptr;                   ///< [NCellsSize][Pitch]
   const I4 *MinLayerCell = nullptr, *MaxLayerCell = nullptr; ///< [cell]
   /// the high-order horizontal flux (MonotoneAdv::setHorzOrder(3 or 4)): all five set, or all five null
   Real *Hess = nullptr;                                      ///< [tracer*3 + t][NCellsSize][Pitch], written by pass 0
   const Real *HessWeight = nullptr;                          ///< [cell][MaxEdges][3]
   const Real *EdgeDirOwn = nullptr, *EdgeDirAcross = nullptr; ///< [cell][MaxEdges][3]
   const Real *FitCell = nullptr;                             ///< [cell] 1.0 / 0.0
   Real Beta           = 0.0;
};
/// the launches of MonotoneAdv::addTracerTend: with Hess set the Hessians of every cell first; the scale factors of every
/// cell, then the limited flux divergence (with VerticalTransport set, of the horizontal and the vertical fluxes).
/// Returns the number of launches issued.
int launchMonotoneAdv(const MeshView &M, const MonotoneAdvArgs &A, hipStream_t S);

} // namespace OMEGA
#endif
