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

/// launchTracerVertMix with a surface flux (VertMix.h, the forced tracer solve): row 0 of tracer L of column c takes
/// Dt * SurfaceFlux[L * FluxStride + c] on its right-hand side.  SurfaceFlux == nullptr: no term (the unforced bits).
void launchTracerVertMixForced(int NCellsOwned, int K, const I4 *MinLayer, const I4 *MaxLayer, const Real *H,
                               const Real *VertDiff, Real *Tracers, int NTracers, int TrRows, Real Dt,
                               const Real *SurfaceFlux, size_t FluxStride, hipStream_t S);

/// The boundary terms of one forced velocity solve (VertMix.h).  A zero coefficient or a null array skips its term.
struct VelocityForcingArgs {
   Real DtBottomDrag = 0, DtRayleigh = 0; ///< Dt * BottomDragCoeff, Dt * RayleighDragCoeff
   Real Rho0         = 1;
   const Real *Stress = nullptr, *EdgeMask = nullptr; ///< [edge]: NormalStressEdge (Pa), EdgeMask
   const Real *Ut     = nullptr;                      ///< [edge][Pitch]: read at the bottom row if DtBottomDrag != 0
};
/// launchVelocityVertMix with wind stress on the top row, linearised quadratic drag on the bottom row and Rayleigh drag
/// on every row (VertMix.h, the forced velocity solve)
void launchVelocityVertMixForced(int NEdgesOwned, int K, const I4 *CellsOnEdge, const I4 *MinLayerEdgeBot,
                                 const I4 *MaxLayerEdgeTop, const Real *H, const Real *VertVisc, Real *U, Real Dt,
                                 const VelocityForcingArgs &F, hipStream_t S);

} // namespace OMEGA
#endif
