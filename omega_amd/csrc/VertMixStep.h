// VertMixStep.h -- the whole vertical-mixing sequence of one time step as one call: the displaced column pass, N^2, the
// tangential velocity, the mixing coefficients, and the forced implicit solves of the tracers and the normal velocity
// (VertMix.h), in the order a host would otherwise have to issue them after every step.  TimeStepper::attachVertMix
// makes the three schemes call it on the new time level at the end of a step.
//
// apply(LayerThickness, NormalVelocity, Tracers, Dt, S) runs on S, in this order:
//   1. VCoord->computeColumn(h, Tracers, Eos, SurfacePressure, TidalPotential, SelfAttractionLoading,
//      Displaced = true, KDisp = 1, S)                    (temperature at tracer index 0, salinity at 1)
//   2. VMix->computeBruntVaisalaFreqSq(Eos, S)
//   3. TangentialReconOnEdge: NormalVelocity -> TangentialVelocity (every edge < NEdgesAll)
//   4. VMix->computeVertMix(NormalVelocity, TangentialVelocity, VMix->BruntVaisalaFreqSq, S)
//  4a. with a Kpp attached (attachKpp; Kpp.h): P->compute(NormalVelocity, TangentialVelocity, VMix->BruntVaisalaFreqSq,
//      VCoord->ZMid, VCoord->ZInterface, VMix->VertDiff, VMix->VertVisc, S) -- the boundary-layer depth, and the
//      K-profile coefficients over what step 4 wrote inside it
//  4b. with a Redi attached (attachRedi; Redi.h): R->computeVertDiffusivity(VMix->VertDiff, S) -- the S.S part of the
//      isoneutral tensor, from the slopes the Redi last computed (inside a split-explicit step: those of level n, one set
//      per step as MPAS-Ocean keeps them), added to the diffusivity steps 4 and 4a have just written
//  4c. with a Kpp attached: P->applyNonLocalTracerFlux(h, Tracers, NTracers, Dt, SurfaceTracerFlux, S) -- the
//      counter-gradient redistribution of the surface flux, before the solve that applies the flux itself
//   5. VMix->applyTracerVertMix(h, Tracers, NTracers, Dt, SurfaceTracerFlux, S)
//   6. VMix->applyVelocityVertMix(h, u, Dt, Boundary, NormalStressEdge if UseWindStress, TangentialVelocity, S)
// The result equals these six (with a Redi: seven; with a Kpp: two more) public calls made by hand, bit for bit.  Step 6
// takes the bottom speed from the velocity before the solve and the tangential velocity of step 3.  As the hook of a
// split-explicit step the sequence -- with a Kpp, with a Redi and with both, in the order 4, 4a, 4b, 4c, 5 -- equals the
// host composition of tests/model_step_reference.py bit for bit, wherever the Kpp evaluates no cbrt (Kpp.h).
//
// One rank only as a stepper hook: the shear of step 4 and the tangential velocity read halo edges, so mixing inside a
// multi-rank step needs the halo of the new level before the sequence and again after the solves; that path is not
// built and TimeStepper::attachVertMix refuses a halo with neighbours.  A host that exchanges the halo itself may
// still call apply() on every rank.
#ifndef OMEGA_AMD_VERTMIXSTEP_H
#define OMEGA_AMD_VERTMIXSTEP_H

#include "ColumnPass.h"
#include "Kpp.h"
#include "OceanState.h"
#include "Redi.h"
#include "VertMix.h"

namespace OMEGA {

class VertMixStep : public Registry<VertMixStep>, public ColumnPass {
 public:
   /// The largest layer count of the fused column pass with the displaced volume (the LDS tile)
   static constexpr int MaxLayers = 1008;

   /// Refuses (OmegaError) a null or host-only mesh, a null VertMix / VertCoord / Eos or one of another mesh or layer
   /// count, NTracers < 2 (temperature and salinity) and more than MaxLayers layers.  Everything is allocated here;
   /// no call allocates.
   VertMixStep(const std::string &Name, const HorzMesh *Mesh, VertMix *VMix, VertCoord *VCoord, Eos *EqState,
               int NTracers);

   I4 NTracers;
   /// Zero at construction; the caller's to overwrite (as the column pass's forcing, ColumnPass.h)
   Array2DReal TangentialVelocity; ///< [NEdgesSize][levelPitch]: rewritten by apply
   Array1DReal NormalStressEdge;   ///< [NEdgesSize], Pa
   Array2DReal SurfaceTracerFlux;  ///< [NTracers][NCellsSize]

   VertMixBoundary Boundary;
   bool UseWindStress = false; ///< pass NormalStressEdge to the velocity solve

   void apply(const Array2DReal &LayerThickness, const Array2DReal &NormalVelocity, const Array3DReal &Tracers, Real Dt,
              hipStream_t S);
   /// thickness and normal velocity of State at time level Level, the tracers of Tracers at TrLevel
   void apply(const OceanState *State, int Level, const TracerStore *Tracers, int TrLevel, Real Dt, hipStream_t S);

   /// Opt-in: step 4b above through R; nullptr detaches.  Refuses (OmegaError) a Redi of another mesh or layer count and
   /// one on another VertCoord or Eos than this object's.  The object keeps the pointer.
   void attachRedi(Redi *R);
   Redi *redi() const { return RediTerm; }
   /// Opt-in: steps 4a and 4c above through P; nullptr detaches.  Refuses (OmegaError) a Kpp of another mesh or layer
   /// count and one on another VertCoord or VertMix than this object's.  The object keeps the pointer.
   void attachKpp(Kpp *P);
   Kpp *kpp() const { return KppTerm; }

   // ---- the reference's style of signature: on this object's `Stream` (default: the null stream)
   hipStream_t Stream = nullptr;
   void apply(const Array2DReal &LayerThickness, const Array2DReal &NormalVelocity, const Array3DReal &Tracers, Real Dt) {
      apply(LayerThickness, NormalVelocity, Tracers, Dt, Stream);
   }

   VertMix *VMix;
   std::string Name;

 protected:
   Redi *RediTerm = nullptr;
   Kpp *KppTerm   = nullptr;
};

} // namespace OMEGA
#endif
