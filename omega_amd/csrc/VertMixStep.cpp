// VertMixStep.cpp -- see VertMixStep.h.
#include "VertMixStep.h"
#include "HorzOperators.h"
#include "Pacer.h"

namespace OMEGA {

VertMixStep::VertMixStep(const std::string &Name_, const HorzMesh *Mesh_, VertMix *VMix_, VertCoord *VCoord_,
                         Eos *EqState_, int NTracers_)
    : ColumnPass(Mesh_, VCoord_, EqState_), NTracers(NTracers_), VMix(VMix_), Name(Name_) {
   OMEGA_REQUIRE(Mesh != nullptr, "VertMixStep: mesh is NULL");
   OMEGA_REQUIRE(NTracers >= 2, "VertMixStep: NTracers = " + std::to_string(NTracers) +
                                    " is below 2: the column pass needs temperature (0) and salinity (1)");
   OMEGA_REQUIRE(!Mesh->HostOnly,
                 "VertMixStep: the mesh was created host-only: no device arrays, compute is unavailable");
   OMEGA_REQUIRE(VMix != nullptr, "VertMixStep: VertMix is NULL");
   OMEGA_REQUIRE(VCoord != nullptr, "VertMixStep: VertCoord is NULL");
   OMEGA_REQUIRE(EqState != nullptr, "VertMixStep: Eos is NULL");
   OMEGA_REQUIRE(VMix->Mesh == Mesh && VMix->VCoord == VCoord && VCoord->Mesh == Mesh && EqState->Mesh == Mesh,
                 "VertMixStep: the VertMix, VertCoord or Eos was built for another mesh");
   OMEGA_REQUIRE(VMix->NVertLayers == VCoord->NVertLayers && EqState->NVertLayers == VCoord->NVertLayers,
                 "VertMixStep: the VertMix, VertCoord and Eos have different layer counts");
   NVertLayers = VCoord->NVertLayers;
   OMEGA_REQUIRE(NVertLayers <= MaxLayers, "VertMixStep: NVertLayers = " + std::to_string(NVertLayers) +
                                               " is above the fused column pass's limit of " +
                                               std::to_string(MaxLayers));
   TangentialVelocity = Array2DReal::levels("TangentialVelocity", Mesh->NEdgesSize, NVertLayers);
   NormalStressEdge   = Array1DReal("NormalStressEdge", Mesh->NEdgesSize);
   SurfaceTracerFlux  = Array2DReal("SurfaceTracerFlux", NTracers, Mesh->NCellsSize);
   allocateForcing();
}

void VertMixStep::attachRedi(Redi *R) {
   if (R != nullptr) {
      OMEGA_REQUIRE(R->Mesh == Mesh && R->NVertLayers == NVertLayers,
                    "VertMixStep::attachRedi: the Redi was built for another mesh or layer count");
      OMEGA_REQUIRE(R->VCoord == VCoord && R->EqState == EqState,
                    "VertMixStep::attachRedi: the Redi is on a different VertCoord or Eos than this VertMixStep");
   }
   RediTerm = R;
}

void VertMixStep::attachKpp(Kpp *P) {
   if (P != nullptr) {
      OMEGA_REQUIRE(P->Mesh == Mesh && P->NVertLayers == NVertLayers,
                    "VertMixStep::attachKpp: the Kpp was built for another mesh or layer count");
      OMEGA_REQUIRE(P->VCoord == VCoord && P->VMix == VMix,
                    "VertMixStep::attachKpp: the Kpp is on a different VertCoord or VertMix than this VertMixStep");
   }
   KppTerm = P;
}

void VertMixStep::apply(const Array2DReal &H, const Array2DReal &U, const Array3DReal &Tr, Real Dt, hipStream_t S) {
   requireLevelArray("VertMixStep", H, Mesh->NCellsSize, NVertLayers, "LayerThickness");
   requireLevelArray("VertMixStep", U, Mesh->NEdgesSize, NVertLayers, "NormalVelocity");
   requireLevelArray("VertMixStep", Tr, NTracers, Mesh->NCellsSize, NVertLayers, "Tracers", "NCellsSize");
   VertMix::requireBoundary(Boundary);
   Pacer::Range Timer("VertMixStep:apply", 1);
   updateColumn(H, Tr, true, S);
   VMix->computeBruntVaisalaFreqSq(*EqState, S);
   const TangentialReconOnEdge TangentialRecon(Mesh);
   TangentialRecon(TangentialVelocity, U, S);
   VMix->computeVertMix(U, TangentialVelocity, VMix->BruntVaisalaFreqSq, S);
   if (KppTerm) // the boundary layer: its depth, and the K-profile coefficients inside it
      KppTerm->compute(U, TangentialVelocity, VMix->BruntVaisalaFreqSq, VCoord->ZMid, VCoord->ZInterface, VMix->VertDiff,
                       VMix->VertVisc, S);
   if (RediTerm) // the S.S part of the isoneutral tensor joins the implicit tracer solve
      RediTerm->computeVertDiffusivity(VMix->VertDiff, S);
   if (KppTerm) // the counter-gradient part of the surface flux, before the solve applies the flux itself
      KppTerm->applyNonLocalTracerFlux(H, Tr, NTracers, Dt, SurfaceTracerFlux, S);
   VMix->applyTracerVertMix(H, Tr, NTracers, Dt, SurfaceTracerFlux, S);
   VMix->applyVelocityVertMix(H, U, Dt, Boundary, UseWindStress ? NormalStressEdge : Array1DReal(), TangentialVelocity,
                              S);
}

void VertMixStep::apply(const OceanState *State, int Level, const TracerStore *Tracers, int TrLevel, Real Dt,
                        hipStream_t S) {
   OMEGA_REQUIRE(State != nullptr && Tracers != nullptr, "VertMixStep::apply: state or tracers is NULL");
   OMEGA_REQUIRE(Tracers->NTracers == NTracers, "VertMixStep::apply: the tracer store has another tracer count");
   Array2DReal H, U;
   OMEGA_REQUIRE(State->getLayerThickness(H, Level) == 0 && State->getNormalVelocity(U, Level) == 0,
                 "VertMixStep::apply: bad time level");
   Array3DReal Tr;
   OMEGA_REQUIRE(Tracers->getAll(Tr, TrLevel) == 0, "VertMixStep::apply: bad tracer time level");
   apply(H, U, Tr, Dt, S);
}

} // namespace OMEGA
