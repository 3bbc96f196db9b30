// VertMix.cpp -- see VertMix.h.
#include "VertMix.h"
#include "Pacer.h"
#include "kernels/TriDiagKernels.h"
#include "kernels/VertMixKernels.h"

namespace OMEGA {

VertMix::VertMix(const std::string &Name_, const HorzMesh *Mesh_, const VertCoord *VCoord_, const VertMixConfig &C)
    : Config(C), NVertLayers(0), Mesh(Mesh_), VCoord(VCoord_), Name(Name_) {
   const std::pair<const char *, Real> NonNeg[] = {{"BackgroundViscosity", C.BackgroundViscosity},
                                                   {"BackgroundDiffusivity", C.BackgroundDiffusivity},
                                                   {"ShearNuZero", C.ShearNuZero},
                                                   {"ConvectiveDiffusivity", C.ConvectiveDiffusivity}};
   for (const auto &P : NonNeg)
      OMEGA_REQUIRE(P.second >= 0.0, std::string("VertMix: ") + P.first + " = " + std::to_string(P.second) +
                                         " is negative: viscosities and diffusivities must be >= 0");
   OMEGA_REQUIRE(Mesh != nullptr, "VertMix: mesh is NULL");
   NVertLayers = VCoord ? VCoord->NVertLayers : Mesh->NVertLayers;
   OMEGA_REQUIRE(NVertLayers >= 1 && NVertLayers <= TriDiagMaxRows,
                 "VertMix: NVertLayers = " + std::to_string(NVertLayers) +
                     " is outside the supported 1 <= NVertLayers <= " + std::to_string(TriDiagMaxRows) +
                     " (the tridiagonal solver limit)");
   OMEGA_REQUIRE(!Mesh->HostOnly, "VertMix: the mesh was created host-only: no device arrays, compute is unavailable");
   OMEGA_REQUIRE(VCoord != nullptr, "VertMix: VertCoord is NULL");
   OMEGA_REQUIRE(VCoord->Mesh == Mesh, "VertMix: the VertCoord was built for another mesh");
   const int NC = Mesh->NCellsSize, K = NVertLayers;
   VertDiff            = Array2DReal::levels("VertDiff", NC, K);
   VertVisc            = Array2DReal::levels("VertVisc", NC, K);
   BruntVaisalaFreqSq  = Array2DReal::levels("BruntVaisalaFreqSq", NC, K);
   VertDiffH           = HostArrayReal(NC, K);
   VertViscH           = HostArrayReal(NC, K);
   BruntVaisalaFreqSqH = HostArrayReal(NC, K);
}

void VertMix::computeBruntVaisalaFreqSq(const Eos &EqState, hipStream_t S) {
   OMEGA_REQUIRE(EqState.Mesh == Mesh && EqState.NVertLayers == NVertLayers,
                 "VertMix::computeBruntVaisalaFreqSq: the Eos was built for another mesh or layer count");
   Pacer::Range Timer("VertMix:computeBruntVaisalaFreqSq", 1);
   launchBruntVaisala(Mesh->NCellsAll, Mesh->NCellsSize, NVertLayers, VCoord->MinLayerCell.Ptr,
                      VCoord->MaxLayerCell.Ptr, VertCoord::Gravity / VCoord->Rho0, EqState.SpecVol.Ptr,
                      EqState.SpecVolDisplaced.Ptr, VCoord->ZMid.Ptr, BruntVaisalaFreqSq.Ptr, S);
}

void VertMix::computeVertMix(const Array2DReal &Un, const Array2DReal &Ut, const Array2DReal &N2, hipStream_t S) {
   requireLevelArray("VertMix", Un, Mesh->NEdgesSize, NVertLayers, "NormalVelocity");
   requireLevelArray("VertMix", Ut, Mesh->NEdgesSize, NVertLayers, "TangentialVelocity");
   requireLevelArray("VertMix", N2, Mesh->NCellsSize, NVertLayers, "BruntVaisalaFreqSq");
   Pacer::Range Timer("VertMix:computeVertMix", 1);
   VertMixCoeffArgs A;
   A.NCellsAll = Mesh->NCellsAll, A.NCellsSize = Mesh->NCellsSize, A.K = NVertLayers, A.MaxEdges = Mesh->MaxEdges;
   A.MinLayer = VCoord->MinLayerCell.Ptr, A.MaxLayer = VCoord->MaxLayerCell.Ptr;
   A.NEdgesOnCell = Mesh->NEdgesOnCell.Ptr, A.EdgesOnCell = Mesh->EdgesOnCell.Ptr;
   A.DcEdge = Mesh->DcEdge.Ptr, A.DvEdge = Mesh->DvEdge.Ptr, A.AreaCell = Mesh->AreaCell.Ptr;
   A.Un = Un.Ptr, A.Ut = Ut.Ptr, A.N2 = N2.Ptr, A.ZMid = VCoord->ZMid.Ptr;
   A.BackgroundViscosity   = Config.BackgroundViscosity;
   A.BackgroundDiffusivity = Config.BackgroundDiffusivity;
   A.EnableShear           = Config.EnableShearMix;
   A.EnableConvective      = Config.EnableConvectiveMix;
   A.ShearNuZero           = Config.ShearNuZero;
   A.ShearAlpha            = Config.ShearAlpha;
   A.ShearExponent         = Config.ShearExponent;
   A.ConvectiveDiffusivity = Config.ConvectiveDiffusivity;
   A.ConvectiveTriggerBVF  = Config.ConvectiveTriggerBVF;
   A.VertVisc = VertVisc.Ptr, A.VertDiff = VertDiff.Ptr;
   launchVertMixCoeffs(A, S);
}

void VertMix::applyTracerVertMix(const Array2DReal &H, const Array3DReal &Tr, int NTracers, Real Dt, hipStream_t S) {
   requireLevelArray("VertMix", H, Mesh->NCellsSize, NVertLayers, "LayerThickness");
   OMEGA_REQUIRE(NTracers >= 0 && NTracers <= Tr.Ext[0], "VertMix::applyTracerVertMix: NTracers = " +
                                                              std::to_string(NTracers) + " is outside 0 .. " +
                                                              std::to_string(Tr.Ext[0]));
   if (NTracers == 0)
      return;
   requireLevelArray("VertMix", Tr, NTracers, Mesh->NCellsSize, NVertLayers, "Tracers", "NCellsSize");
   Pacer::Range Timer("VertMix:applyTracerVertMix", 1);
   launchTracerVertMix(Mesh->NCellsOwned, NVertLayers, VCoord->MinLayerCell.Ptr, VCoord->MaxLayerCell.Ptr, H.Ptr,
                       VertDiff.Ptr, Tr.Ptr, NTracers, Tr.Ext[1], Dt, S);
}

void VertMix::applyTracerVertMix(const OceanState *State, int ThickLevel, const TracerStore *Tracers, int TrLevel,
                                 Real Dt, hipStream_t S) {
   OMEGA_REQUIRE(State != nullptr && Tracers != nullptr, "VertMix::applyTracerVertMix: state or tracers is NULL");
   Array2DReal H;
   OMEGA_REQUIRE(State->getLayerThickness(H, ThickLevel) == 0, "VertMix::applyTracerVertMix: bad thickness time level");
   Array3DReal Tr;
   OMEGA_REQUIRE(Tracers->getAll(Tr, TrLevel) == 0, "VertMix::applyTracerVertMix: bad tracer time level");
   applyTracerVertMix(H, Tr, Tracers->NTracers, Dt, S);
}

void VertMix::applyVelocityVertMix(const Array2DReal &H, const Array2DReal &U, Real Dt, hipStream_t S) {
   requireLevelArray("VertMix", H, Mesh->NCellsSize, NVertLayers, "LayerThickness");
   requireLevelArray("VertMix", U, Mesh->NEdgesSize, NVertLayers, "NormalVelocity");
   Pacer::Range Timer("VertMix:applyVelocityVertMix", 1);
   launchVelocityVertMix(Mesh->NEdgesOwned, NVertLayers, Mesh->CellsOnEdge.Ptr, VCoord->MinLayerEdgeBot.Ptr,
                         VCoord->MaxLayerEdgeTop.Ptr, H.Ptr, VertVisc.Ptr, U.Ptr, Dt, S);
}

void VertMix::applyVelocityVertMix(const OceanState *State, int Level, Real Dt, hipStream_t S) {
   OMEGA_REQUIRE(State != nullptr, "VertMix::applyVelocityVertMix: state is NULL");
   Array2DReal H, U;
   OMEGA_REQUIRE(State->getLayerThickness(H, Level) == 0 && State->getNormalVelocity(U, Level) == 0,
                 "VertMix::applyVelocityVertMix: bad time level");
   applyVelocityVertMix(H, U, Dt, S);
}

void VertMix::requireBoundary(const VertMixBoundary &B) {
   OMEGA_REQUIRE(B.BottomDragCoeff >= 0.0, "VertMix: BottomDragCoeff = " + std::to_string(B.BottomDragCoeff) +
                                               " is negative: drag coefficients must be >= 0");
   OMEGA_REQUIRE(B.RayleighDragCoeff >= 0.0, "VertMix: RayleighDragCoeff = " + std::to_string(B.RayleighDragCoeff) +
                                                 " is negative: drag coefficients must be >= 0");
}

void VertMix::applyTracerVertMix(const Array2DReal &H, const Array3DReal &Tr, int NTracers, Real Dt,
                                 const Array2DReal &Flux, hipStream_t S) {
   requireLevelArray("VertMix", H, Mesh->NCellsSize, NVertLayers, "LayerThickness");
   OMEGA_REQUIRE(NTracers >= 0 && NTracers <= Tr.Ext[0], "VertMix::applyTracerVertMix: NTracers = " +
                                                              std::to_string(NTracers) + " is outside 0 .. " +
                                                              std::to_string(Tr.Ext[0]));
   if (NTracers == 0)
      return;
   requireLevelArray("VertMix", Tr, NTracers, Mesh->NCellsSize, NVertLayers, "Tracers", "NCellsSize");
   OMEGA_REQUIRE(Flux.Ptr == nullptr ||
                     (Flux.Ext[0] >= NTracers && Flux.Ext[1] == Mesh->NCellsSize && Flux.Pitch == Mesh->NCellsSize),
                 "VertMix: SurfaceTracerFlux must be [NTracers][NCellsSize]");
   Pacer::Range Timer("VertMix:applyTracerVertMixForced", 1);
   launchTracerVertMixForced(Mesh->NCellsOwned, NVertLayers, VCoord->MinLayerCell.Ptr, VCoord->MaxLayerCell.Ptr, H.Ptr,
                             VertDiff.Ptr, Tr.Ptr, NTracers, Tr.Ext[1], Dt, Flux.Ptr, (size_t)Mesh->NCellsSize, S);
}

void VertMix::applyVelocityVertMix(const Array2DReal &H, const Array2DReal &U, Real Dt, const VertMixBoundary &B,
                                   const Array1DReal &Stress, const Array2DReal &Ut, hipStream_t S) {
   requireBoundary(B);
   requireLevelArray("VertMix", H, Mesh->NCellsSize, NVertLayers, "LayerThickness");
   requireLevelArray("VertMix", U, Mesh->NEdgesSize, NVertLayers, "NormalVelocity");
   OMEGA_REQUIRE(Stress.Ptr == nullptr || Stress.Ext[0] == Mesh->NEdgesSize,
                 "VertMix: NormalStressEdge must be [NEdgesSize]");
   if (B.BottomDragCoeff != 0.0) {
      OMEGA_REQUIRE(Ut.Ptr != nullptr, "VertMix: BottomDragCoeff != 0 needs the tangential velocity");
      requireLevelArray("VertMix", Ut, Mesh->NEdgesSize, NVertLayers, "TangentialVelocity");
   }
   Pacer::Range Timer("VertMix:applyVelocityVertMixForced", 1);
   VelocityForcingArgs F;
   F.DtBottomDrag = Dt * B.BottomDragCoeff, F.DtRayleigh = Dt * B.RayleighDragCoeff;
   F.Rho0   = VCoord->Rho0;
   F.Stress = Stress.Ptr, F.EdgeMask = Mesh->EdgeMask1D.Ptr;
   F.Ut     = B.BottomDragCoeff != 0.0 ? Ut.Ptr : nullptr;
   launchVelocityVertMixForced(Mesh->NEdgesOwned, NVertLayers, Mesh->CellsOnEdge.Ptr, VCoord->MinLayerEdgeBot.Ptr,
                               VCoord->MaxLayerEdgeTop.Ptr, H.Ptr, VertVisc.Ptr, U.Ptr, Dt, F, S);
}

void VertMix::copyToHost() {
   HIP_CHECK(hipDeviceSynchronize());
   OMEGA::copyToHost(VertDiffH.data(), VertDiff);
   OMEGA::copyToHost(VertViscH.data(), VertVisc);
   OMEGA::copyToHost(BruntVaisalaFreqSqH.data(), BruntVaisalaFreqSq);
}

void VertMix::copyToDevice() {
   OMEGA::copyToDevice(VertDiff, VertDiffH.data());
   OMEGA::copyToDevice(VertVisc, VertViscH.data());
   OMEGA::copyToDevice(BruntVaisalaFreqSq, BruntVaisalaFreqSqH.data());
}

} // namespace OMEGA
