// VertMix.h -- vertical mixing: background, Pacanowski-Philander shear and convective viscosity / diffusivity, and the
// implicit (backward-Euler) vertical diffusion of tracers and normal velocity with them.  The reference specifies the
// feature in its design document only (components/omega/doc/design/VerticalMixingCoeff.md: configuration section
// 4.1.1, coefficients 4.2, no-flux boundaries); the column solve is the reference's PCRDiffusionSolver
// (TriDiagSolvers.h), assembled as the reference's diffusion test does (test/base/TriDiagSolversTest.cpp:136-235:
// H = h, G = kappa * dt / mean(h), X = h * phi).
//
// Row K of VertDiff, VertVisc and BruntVaisalaFreqSq is the interface at the top of layer K.  Every array is
// [NCellsSize][levelPitch(NVertLayers)], allocated in the constructor; no call allocates.
//
// Numerical contract (FP64, -ffp-contract=off, IEEE divisions; a NumPy restatement in the same order is bit-identical,
// tests/vert_mix_reference.py).  g = VertCoord::Gravity (9.80616), Rho0 = the VertCoord's.  A column is a cell
// c < NCellsAll with 0 <= KMin <= KMax < NVertLayers.
//  - computeBruntVaisalaFreqSq(Eos): after VertCoord::computeColumn(..., Displaced = true, KDisp = 1, ...), so that
//    SpecVolDisplaced[K-1] is layer K-1's water at layer K's pressure, for KMin < K <= KMax:
//      N2[K] = ((g / Rho0) * ((1.0 / SpecVol[K]) - (1.0 / SpecVolDisplaced[K-1]))) / (ZMid[K-1] - ZMid[K])
//    Every other entry of rows 0 .. NCellsSize-1 is 0 (K = KMin, levels outside the range, land, the sentinel row).
//  - computeVertMix(Un, Ut, N2): edge arrays [NEdgesSize][pitch]; for KMin < K <= KMax, in this order:
//      visc = BackgroundViscosity; diff = BackgroundDiffusivity
//      shear:  S2 = 0; for J = 0 .. NEdgesOnCell-1 (e = EdgesOnCell[c][J]):
//                F = ((0.5 * DcEdge[e]) * DvEdge[e]) * (1.0 / AreaCell[c])
//                du = Un[e][K-1] - Un[e][K]; dv = Ut[e][K-1] - Ut[e][K]; S2 = S2 + F * ((du*du) + (dv*dv))
//              dz = ZMid[K-1] - ZMid[K]; S2 = S2 / (dz*dz); Ri = max(N2[K] / max(S2, 1.0e-12), 0.0)
//              D = 1.0 + ShearAlpha * Ri; visc = visc + ShearNuZero / D^n; diff = diff + visc / D
//      convective, if N2[K] < ConvectiveTriggerBVF: visc = visc + ConvectiveDiffusivity; diff = diff + ConvectiveDiffusivity
//    D^n is D*D*...*D left to right for an integer n = ShearExponent in 1 .. 8, else pow(D, n).  Every other entry of
//    rows 0 .. NCellsSize-1 is 0: the no-flux top interface K = KMin, levels outside the range, land, the sentinel row.
//    Edges are read as stored, also at levels where the neighbour cell is inactive.
//  - applyTracerVertMix(h, Tracers, NTracers, Dt): owned cells c < NCellsOwned, n = KMax-KMin+1, row i = level KMin+i:
//      H_i = h[k]; G_i = (VertDiff[k+1] * Dt) / ((h[k+1] + h[k]) / 2) for i < n-1, G_{n-1} = 0; X_i = h[k] * phi[k]
//      phi[k] <- PCRDiffusionSolver on (G, H, X) (tests/tridiag_reference.py: pcr_diff, NRow = 1 the 1x1 solve)
//    for every tracer; nothing else is written (not levels outside the range, land, halo or sentinel rows).
//  - applyVelocityVertMix(h, u, Dt): owned edges e < NEdgesOwned, c1, c2 = CellsOnEdge[e], levels
//    MinLayerEdgeBot[e] .. MaxLayerEdgeTop[e] (an empty range leaves the edge alone):
//      hE[k] = 0.5 * (h[c1][k] + h[c2][k]); nuE[k] = 0.5 * (VertVisc[c1][k] + VertVisc[c2][k])
//      H_i = hE[k]; G_i = (nuE[k+1] * Dt) / ((hE[k+1] + hE[k]) / 2), G_{n-1} = 0; X_i = hE[k] * u[k]
//
// The forced solves (the overloads with a VertMixBoundary / a SurfaceTracerFlux) put the reference's "forcing at the
// top and bottom of the ocean" (components/omega/doc/design/OmegaV1GoverningEqns.md section 11) into the same
// backward-Euler systems: wind stress as the top boundary condition, bottom drag as the bottom boundary condition,
// Rayleigh drag on every row, surface tracer fluxes on the top row.  Same precision rules (FP64, no contraction, IEEE
// division and sqrt, every chain in the order written); restated in tests/vert_mix_forcing_reference.py.
//  - applyVelocityVertMix(h, u, Dt, Boundary, NormalStressEdge, Ut): owned edges with a non-empty range Lo .. Hi,
//    n = Hi-Lo+1, row i = level k = Lo+i; hE[k], nuE[k] and G_i exactly as above:
//      D_i = hE[k]
//      if RayleighDragCoeff != 0:             D_i = D_i + (Dt*RayleighDragCoeff)*hE[k]
//      if i == n-1 and BottomDragCoeff != 0:  Speed = sqrt((u[e][Hi]*u[e][Hi]) + (Ut[e][Hi]*Ut[e][Hi]))   (u before the solve)
//                                             D_i = D_i + (Dt*BottomDragCoeff)*Speed
//      X_i = hE[k]*u[e][k]
//      if i == 0 and a stress array is given: X_i = X_i + (Dt*EdgeMask[e])*(NormalStressEdge[e]/Rho0)
//      u[e][Lo..Hi] <- the PCRDiffusionSolver arithmetic on (G, D, X): D stands where H stood
//    NormalStressEdge is [NEdgesSize] in Pa (an empty array: no stress); Ut is [NEdgesSize][pitch], required iff
//    BottomDragCoeff != 0.  n == 1 takes both boundary terms on its one row (the 1x1 solve).  A term whose
//    coefficient is zero, or whose array is absent, is skipped; with all terms skipped the result equals the unforced
//    call bit for bit.  Negative coefficients are refused.  An edge with an empty range is left alone whatever its
//    stress.
//  - applyTracerVertMix(h, Tracers, NTracers, Dt, SurfaceTracerFlux): SurfaceTracerFlux holds NTracers x NCellsSize
//    values, tracer-major, in tracer units * m/s, positive into the ocean (an empty array: no flux).  For an owned
//    cell, with rows as in applyTracerVertMix:
//      X_0 = (h[KMin]*phi[KMin]) + Dt*SurfaceTracerFlux[L][c]
//    Every other row, G and H are unchanged, so the once-per-column recursion is still shared by all tracers.
//  - Both write nothing outside what the unforced calls write.
//  - Freshwater as a mass flux (a thickness source) is out of scope: only tracer fluxes through a fixed surface.
//
// Deviations from the design document:
//  - Bottom drag: the linearised implicit form Cd |u^n| u^{n+1} on the bottom row's diagonal, stable for any Dt*Cd,
//    with the speed from the edge's own normal and tangential velocity (the governing-equation document's u|u|), not
//    from the cell kinetic energies that Omega-0's explicit BottomDragOnEdge averages to the edge.
//  - N2 form: the document writes N2 = g rho0 (rho_DD - rho) / (z(k-1) - z(k)), which has the wrong sign for stable
//    water and units other than s^-2; the form above is the document's with g / rho0 and the sign that makes N2 > 0
//    for stable water (lighter above), with rho = 1 / SpecVol.  It lives on VertMix, not in the equation of state.
//  - Ri clamp Ri >= 0: for N2 < 0 the literal formula divides by a 1 + alpha Ri that can be zero or negative;
//    Pacanowski-Philander is defined for Ri >= 0, and unstable water gets the convective term.
//  - Integer exponents by repeated multiplication: equal to a correctly rounded pow for these, and reproducible in
//    NumPy bit for bit; a non-integer exponent uses the device pow (a few ulp from NumPy's).
//
// The tracer pass solves every tracer of a column in one launch: G and H are assembled once, and everything of the
// PCR recursion that depends on them only (Alpha, Beta, the reduced G and H, the final determinants) is computed once
// per row and level (kernels/TriDiagKernels.h: pcrDiffSolveRowMulti).  Each tracer's result equals a separate
// PCRDiffusionSolver solve on the same G, H, X bit for bit.  Algorithmic traffic per active cell-level: 16 B (h,
// VertDiff) + 16 B per tracer (phi read and written), 112 B at 6 tracers.
#ifndef OMEGA_AMD_VERTMIX_H
#define OMEGA_AMD_VERTMIX_H

#include "Base.h"
#include "Eos.h"
#include "HorzMesh.h"
#include "OceanState.h"
#include "VertCoord.h"

namespace OMEGA {

/// The design document's configuration (VerticalMixingCoeff.md section 4.1.1), with its defaults
struct VertMixConfig {
   Real BackgroundViscosity   = 1.0e-4;
   Real BackgroundDiffusivity = 1.0e-5;
   bool EnableShearMix        = true;
   Real ShearNuZero           = 0.005;
   Real ShearAlpha            = 5;
   Real ShearExponent         = 2;
   bool EnableConvectiveMix   = true;
   Real ConvectiveDiffusivity = 1.0;
   Real ConvectiveTriggerBVF  = 0.0;
};

/// Coefficients of the forced velocity solve; both >= 0 (refused otherwise), 0 switches the term off
struct VertMixBoundary {
   Real BottomDragCoeff   = 0; ///< dimensionless Cd of the quadratic bottom drag
   Real RayleighDragCoeff = 0; ///< s^-1
};

class VertMix : public Registry<VertMix> {
 public:
   /// Refuses (OmegaError) negative viscosities or diffusivities, NVertLayers above the tridiagonal limit (1024), a
   /// host-only mesh and a VertCoord of another mesh.
   VertMix(const std::string &Name, const HorzMesh *Mesh, const VertCoord *VCoord, const VertMixConfig &Config);

   VertMixConfig Config;
   I4 NVertLayers;
   Array2DReal VertDiff, VertVisc, BruntVaisalaFreqSq; ///< [NCellsSize][levelPitch(NVertLayers)]
   HostArrayReal VertDiffH, VertViscH, BruntVaisalaFreqSqH;

   /// N2 into BruntVaisalaFreqSq from EqState's SpecVol / SpecVolDisplaced (KDisp = 1) and the VertCoord's ZMid
   void computeBruntVaisalaFreqSq(const Eos &EqState, hipStream_t S);
   /// VertVisc and VertDiff from the edge velocities and N2 (this object's BruntVaisalaFreqSq or the caller's)
   void computeVertMix(const Array2DReal &NormalVelocity, const Array2DReal &TangentialVelocity,
                       const Array2DReal &BruntVaisalaFreqSq, hipStream_t S);
   /// Tracers [>= NTracers][NCellsSize][levelPitch] are mixed in place; LayerThickness [NCellsSize][levelPitch]
   void applyTracerVertMix(const Array2DReal &LayerThickness, const Array3DReal &Tracers, int NTracers, Real Dt,
                           hipStream_t S);
   void applyTracerVertMix(const OceanState *State, int ThickLevel, const TracerStore *Tracers, int TrLevel, Real Dt,
                           hipStream_t S);
   /// NormalVelocity [NEdgesSize][levelPitch] is mixed in place
   void applyVelocityVertMix(const Array2DReal &LayerThickness, const Array2DReal &NormalVelocity, Real Dt,
                             hipStream_t S);
   /// thickness and normal velocity of State at time level Level
   void applyVelocityVertMix(const OceanState *State, int Level, Real Dt, hipStream_t S);
   /// The forced solves (contract above).  SurfaceTracerFlux [>= NTracers][NCellsSize]; NormalStressEdge [NEdgesSize];
   /// TangentialVelocity [NEdgesSize][levelPitch].  An empty array (Ptr == nullptr) is an absent one.
   void applyTracerVertMix(const Array2DReal &LayerThickness, const Array3DReal &Tracers, int NTracers, Real Dt,
                           const Array2DReal &SurfaceTracerFlux, hipStream_t S);
   void applyVelocityVertMix(const Array2DReal &LayerThickness, const Array2DReal &NormalVelocity, Real Dt,
                             const VertMixBoundary &Boundary, const Array1DReal &NormalStressEdge,
                             const Array2DReal &TangentialVelocity, hipStream_t S);
   /// Refuses (OmegaError) a negative coefficient
   static void requireBoundary(const VertMixBoundary &Boundary);

   // ---- the reference's style of signature: on this object's `Stream` (default: the null stream)
   hipStream_t Stream = nullptr;
   void computeBruntVaisalaFreqSq(const Eos &EqState) { computeBruntVaisalaFreqSq(EqState, Stream); }
   void computeVertMix(const Array2DReal &NormalVelocity, const Array2DReal &TangentialVelocity,
                       const Array2DReal &BruntVaisalaFreqSq) {
      computeVertMix(NormalVelocity, TangentialVelocity, BruntVaisalaFreqSq, Stream);
   }
   void applyTracerVertMix(const Array2DReal &LayerThickness, const Array3DReal &Tracers, int NTracers, Real Dt) {
      applyTracerVertMix(LayerThickness, Tracers, NTracers, Dt, Stream);
   }
   void applyVelocityVertMix(const Array2DReal &LayerThickness, const Array2DReal &NormalVelocity, Real Dt) {
      applyVelocityVertMix(LayerThickness, NormalVelocity, Dt, Stream);
   }

   void copyToHost();   ///< VertDiff, VertVisc, BruntVaisalaFreqSq -> the host mirrors
   void copyToDevice(); ///< the host mirrors -> VertDiff, VertVisc, BruntVaisalaFreqSq

   const HorzMesh *Mesh;
   const VertCoord *VCoord;
   std::string Name;
};

} // namespace OMEGA
#endif
