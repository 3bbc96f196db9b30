// VertMixKernels.h -- host-callable launchers of the vertical-mixing kernels behind VertMix (kernels/VertMixKernels.hip).
// Every launcher is asynchronous on the given stream, takes raw device pointers and allocates nothing.  Level-indexed
// arrays are [rows][Pitch] with Pitch = levelPitch(K).  The numerical contract is written down in VertMix.h.
#ifndef OMEGA_AMD_VERTMIXKERNELS_H
#define OMEGA_AMD_VERTMIXKERNELS_H

#include "../Base.h"

namespace OMEGA {

/// VertMix::computeBruntVaisalaFreqSq: rows 0 .. NCellsSize-1 of N2 (rows < NCellsAll computed on KMin < K <= KMax,
/// every other entry 0).  GOverRho0 = g / Rho0, evaluated by the caller.
void launchBruntVaisala(int NCellsAll, int NCellsSize, int K, const I4 *MinLayer, const I4 *MaxLayer, Real GOverRho0,
                        const Real *SpecVol, const Real *SpecVolDisp, const Real *ZMid, Real *N2, hipStream_t S);

/// Everything one coefficient launch reads and writes (VertMix::computeVertMix).
struct VertMixCoeffArgs {
   int NCellsAll = 0, NCellsSize = 0, K = 0, MaxEdges = 0;
   const I4 *MinLayer = nullptr, *MaxLayer = nullptr;
   const I4 *NEdgesOnCell = nullptr, *EdgesOnCell = nullptr; ///< [cell], [cell][MaxEdges]
   const Real *DcEdge = nullptr, *DvEdge = nullptr, *AreaCell = nullptr;
   const Real *Un = nullptr, *Ut = nullptr; ///< [edge][Pitch]
   const Real *N2 = nullptr, *ZMid = nullptr; ///< [cell][Pitch]
   Real BackgroundViscosity = 0, BackgroundDiffusivity = 0;
   int EnableShear = 0, EnableConvective = 0;
   Real ShearNuZero = 0, ShearAlpha = 0, ShearExponent = 0;
   Real ConvectiveDiffusivity = 0, ConvectiveTriggerBVF = 0;
   Real *VertVisc = nullptr, *VertDiff = nullptr; ///< [cell][Pitch]
};
void launchVertMixCoeffs(const VertMixCoeffArgs &A, hipStream_t S);

/// Backward-Euler diffusion of NTracers tracers ([NTracers][TrRows][Pitch]) in place on owned cells 0 .. NCellsOwned-1,
/// with the diffusivity VertDiff and thickness H: all tracers of a column in one pass (VertMix::applyTracerVertMix).
void launchTracerVertMix(int NCellsOwned, int K, const I4 *MinLayer, const I4 *MaxLayer, const Real *H,
                         const Real *VertDiff, Real *Tracers, int NTracers, int TrRows, Real Dt, hipStream_t S);

/// Backward-Euler diffusion of the normal velocity in place on owned edges 0 .. NEdgesOwned-1, levels
/// MinLayerEdgeBot .. MaxLayerEdgeTop, with cell values averaged to the edge (VertMix::applyVelocityVertMix).
void launchVelocityVertMix(int NEdgesOwned, int K, const I4 *CellsOnEdge, const I4 *MinLayerEdgeBot,
                           const I4 *MaxLayerEdgeTop, const Real *H, const Real *VertVisc, Real *U, Real Dt,
                           hipStream_t S);

} // namespace OMEGA
#endif
