// KppKernels.h -- host-callable launchers of the K-profile kernels behind Kpp (kernels/KppKernels.hip).  Both are
// asynchronous on the given stream, take raw device pointers and allocate nothing.  Level-indexed arrays are
// [rows][Pitch] with Pitch = levelPitch(K); ZInterface is [rows][levelPitch(K + 1)].  The numerical contract is written
// down in Kpp.h.
#ifndef OMEGA_AMD_KPPKERNELS_H
#define OMEGA_AMD_KPPKERNELS_H

#include "../Base.h"

namespace OMEGA {

/// Large et al. (1994): the constants of the unstable velocity scales, chosen so that the two branches of wS meet at
/// ZetaS and those of wM at ZetaM
constexpr Real KppCs = 98.96, KppCm = 8.38, KppAs = -28.86, KppAm = 1.26, KppZetaS = -1.0, KppZetaM = -0.2;

/// Everything the one launch of Kpp::compute reads and writes
struct KppComputeArgs {
   int NCellsAll = 0, NCellsSize = 0, K = 0, MaxEdges = 0;
   const I4 *MinLayer = nullptr, *MaxLayer = nullptr;
   const I4 *NEdgesOnCell = nullptr, *EdgesOnCell = nullptr; ///< [cell], [cell][MaxEdges]
   const Real *DcEdge = nullptr, *DvEdge = nullptr, *AreaCell = nullptr;
   const Real *Un = nullptr, *Ut = nullptr;                          ///< [edge][Pitch]
   const Real *N2 = nullptr, *ZMid = nullptr;                        ///< [cell][Pitch]
   const Real *ZInterface = nullptr;                                 ///< [cell][levelPitch(K + 1)]
   const Real *FrictionVelocity = nullptr, *SurfaceBuoyancyFlux = nullptr; ///< [cell]
   Real VonKarman = 0, CritBulkRichardson = 0, SurfaceLayerFraction = 0;
   Real VtCoef = 0, NonLocalCoeff = 0; ///< formed once on the host (Kpp.h)
   Real BackgroundViscosity = 0, BackgroundDiffusivity = 0;
   Real *VertVisc = nullptr, *VertDiff = nullptr;             ///< [cell][Pitch], rewritten inside the boundary layer
   Real *BulkRichardson = nullptr, *NonLocalShape = nullptr;  ///< [cell][Pitch]
   Real *BoundaryLayerDepth = nullptr;                        ///< [cell]
   I4 *BoundaryLayerIndex   = nullptr;                        ///< [cell]
};
void launchKppCompute(const KppComputeArgs &A, hipStream_t S);

/// Kpp::applyNonLocalTracerFlux: tracers [NTracers][TrRows][Pitch] in place on owned cells 0 .. NCellsOwned-1, every
/// tracer in the one launch; SurfaceFlux [NTracers][FluxStride]
void launchKppNonLocal(int NCellsOwned, int K, const I4 *MinLayer, const I4 *MaxLayer, const Real *H,
                       const Real *NonLocalShape, Real *Tracers, int NTracers, int TrRows, Real Dt,
                       const Real *SurfaceFlux, size_t FluxStride, hipStream_t S);

} // namespace OMEGA
#endif
