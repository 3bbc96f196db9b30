// Kpp.cpp -- see Kpp.h.
#include "Kpp.h"
#include "Pacer.h"
#include "kernels/PackedColumns.h"

#include <cmath>

namespace OMEGA {

Kpp::Kpp(const std::string &Name_, const HorzMesh *Mesh_, const VertCoord *VCoord_, VertMix *VMix_, const KppConfig &C)
    : Config(C), NVertLayers(0), VtCoef(0), NonLocalCoeff(0), Mesh(Mesh_), VCoord(VCoord_), VMix(VMix_), Name(Name_) {
   const auto Text = [](const char *Field, Real V, const char *Rule) {
      return std::string("Kpp: ") + Field + " = " + std::to_string(V) + " " + Rule;
   };
   OMEGA_REQUIRE(std::isfinite(C.VonKarman) && C.VonKarman > 0.0,
                 Text("VonKarman", C.VonKarman, "is not finite or not positive"));
   OMEGA_REQUIRE(std::isfinite(C.CritBulkRichardson) && C.CritBulkRichardson > 0.0,
                 Text("CritBulkRichardson", C.CritBulkRichardson, "is not finite or not positive"));
   OMEGA_REQUIRE(C.SurfaceLayerFraction > 0.0 && C.SurfaceLayerFraction < 1.0,
                 Text("SurfaceLayerFraction", C.SurfaceLayerFraction, "is outside (0, 1)"));
   const std::pair<const char *, Real> NonNeg[] = {
       {"Cv", C.Cv}, {"EntrainmentRatio", C.EntrainmentRatio}, {"CStar", C.CStar}};
   for (const auto &P : NonNeg)
      OMEGA_REQUIRE(std::isfinite(P.second) && P.second >= 0.0, Text(P.first, P.second, "is negative or not finite"));
   OMEGA_REQUIRE(Mesh != nullptr, "Kpp: mesh is NULL");
   OMEGA_REQUIRE(!Mesh->HostOnly, "Kpp: the mesh was created host-only: no device arrays, compute is unavailable");
   OMEGA_REQUIRE(VCoord != nullptr, "Kpp: VertCoord is NULL");
   OMEGA_REQUIRE(VMix != nullptr, "Kpp: VertMix is NULL");
   OMEGA_REQUIRE(VCoord->Mesh == Mesh && VMix->Mesh == Mesh, "Kpp: the VertCoord or VertMix was built for another mesh");
   OMEGA_REQUIRE(VMix->NVertLayers == VCoord->NVertLayers, "Kpp: the VertCoord and VertMix have different layer counts");
   OMEGA_REQUIRE(VMix->VCoord == VCoord, "Kpp: the VertMix is on a different VertCoord");
   NVertLayers = VCoord->NVertLayers;
   requirePackedLayers("Kpp", NVertLayers);

   const Real Kappa = C.VonKarman, Ric = C.CritBulkRichardson, Eps = C.SurfaceLayerFraction;
   VtCoef        = (C.Cv * std::sqrt(C.EntrainmentRatio)) / ((Ric * (Kappa * Kappa)) * std::sqrt(KppCs * Eps));
   NonLocalCoeff = (C.CStar * Kappa) * std::cbrt((KppCs * Kappa) * Eps);

   const int NC = Mesh->NCellsSize, K = NVertLayers;
   FrictionVelocity     = Array1DReal("FrictionVelocity", NC);
   SurfaceBuoyancyFlux  = Array1DReal("SurfaceBuoyancyFlux", NC);
   BoundaryLayerDepth   = Array1DReal("BoundaryLayerDepth", NC);
   BoundaryLayerIndex   = Array1DI4("BoundaryLayerIndex", NC);
   BulkRichardson       = Array2DReal::levels("BulkRichardson", NC, K);
   NonLocalShape        = Array2DReal::levels("NonLocalShape", NC, K);
   FrictionVelocityH    = HostArrayReal(NC);
   SurfaceBuoyancyFluxH = HostArrayReal(NC);
   BoundaryLayerDepthH  = HostArrayReal(NC);
   BoundaryLayerIndexH  = HostArrayI4(NC);
   BulkRichardsonH      = HostArrayReal(NC, K);
   NonLocalShapeH       = HostArrayReal(NC, K);
}

void Kpp::compute(const Array2DReal &Un, const Array2DReal &Ut, const Array2DReal &N2, const Array2DReal &ZMid,
                  const Array2DReal &ZInt, const Array2DReal &VertDiff, const Array2DReal &VertVisc, hipStream_t S) const {
   const int K = NVertLayers;
   requireLevelArray("Kpp", Un, Mesh->NEdgesSize, K, "NormalVelocity");
   requireLevelArray("Kpp", Ut, Mesh->NEdgesSize, K, "TangentialVelocity");
   requireLevelArray("Kpp", N2, Mesh->NCellsSize, K, "BruntVaisalaFreqSq");
   requireLevelArray("Kpp", ZMid, Mesh->NCellsSize, K, "ZMid");
   OMEGA_REQUIRE(ZInt.Ptr != nullptr && ZInt.Ext[0] >= Mesh->NCellsSize && ZInt.Ext[1] == K + 1 &&
                     ZInt.Pitch == levelPitch(K + 1),
                 "Kpp: ZInterface must be [NCellsSize][NVertLayers + 1] with rows of levelPitch(NVertLayers + 1)");
   requireLevelArray("Kpp", VertDiff, Mesh->NCellsSize, K, "VertDiff");
   requireLevelArray("Kpp", VertVisc, Mesh->NCellsSize, K, "VertVisc");
   Pacer::Range Timer("Kpp:compute", 1);
   KppComputeArgs A;
   A.NCellsAll = Mesh->NCellsAll, A.NCellsSize = Mesh->NCellsSize, A.K = K, A.MaxEdges = Mesh->MaxEdges;
   A.MinLayer = VCoord->MinLayerCell.Ptr, A.MaxLayer = VCoord->MaxLayerCell.Ptr;
   A.NEdgesOnCell = Mesh->NEdgesOnCell.Ptr, A.EdgesOnCell = Mesh->EdgesOnCell.Ptr;
   A.DcEdge = Mesh->DcEdge.Ptr, A.DvEdge = Mesh->DvEdge.Ptr, A.AreaCell = Mesh->AreaCell.Ptr;
   A.Un = Un.Ptr, A.Ut = Ut.Ptr, A.N2 = N2.Ptr, A.ZMid = ZMid.Ptr, A.ZInterface = ZInt.Ptr;
   A.FrictionVelocity = FrictionVelocity.Ptr, A.SurfaceBuoyancyFlux = SurfaceBuoyancyFlux.Ptr;
   A.VonKarman = Config.VonKarman, A.CritBulkRichardson = Config.CritBulkRichardson;
   A.SurfaceLayerFraction = Config.SurfaceLayerFraction;
   A.VtCoef = VtCoef, A.NonLocalCoeff = NonLocalCoeff;
   A.BackgroundViscosity   = VMix->Config.BackgroundViscosity;
   A.BackgroundDiffusivity = VMix->Config.BackgroundDiffusivity;
   A.VertVisc = VertVisc.Ptr, A.VertDiff = VertDiff.Ptr;
   A.BulkRichardson = BulkRichardson.Ptr, A.NonLocalShape = NonLocalShape.Ptr;
   A.BoundaryLayerDepth = BoundaryLayerDepth.Ptr, A.BoundaryLayerIndex = BoundaryLayerIndex.Ptr;
   launchKppCompute(A, S);
   ++LaunchCount;
}

void Kpp::compute(const Array2DReal &Un, const Array2DReal &Ut, hipStream_t S) const {
   compute(Un, Ut, VMix->BruntVaisalaFreqSq, VCoord->ZMid, VCoord->ZInterface, VMix->VertDiff, VMix->VertVisc, S);
}

void Kpp::applyNonLocalTracerFlux(const Array2DReal &H, const Array3DReal &Tr, int NTracers, Real Dt,
                                  const Array2DReal &Flux, hipStream_t S) const {
   requireLevelArray("Kpp", H, Mesh->NCellsSize, NVertLayers, "LayerThickness");
   OMEGA_REQUIRE(NTracers >= 0 && NTracers <= Tr.Ext[0], "Kpp::applyNonLocalTracerFlux: NTracers = " +
                                                              std::to_string(NTracers) + " is outside 0 .. " +
                                                              std::to_string(Tr.Ext[0]));
   if (NTracers == 0 || Flux.Ptr == nullptr)
      return;
   requireLevelArray("Kpp", Tr, NTracers, Mesh->NCellsSize, NVertLayers, "Tracers", "NCellsSize");
   OMEGA_REQUIRE(Flux.Ext[0] >= NTracers && Flux.Ext[1] == Mesh->NCellsSize && Flux.Pitch == Mesh->NCellsSize,
                 "Kpp: SurfaceTracerFlux must be [NTracers][NCellsSize]");
   Pacer::Range Timer("Kpp:applyNonLocalTracerFlux", 1);
   launchKppNonLocal(Mesh->NCellsOwned, NVertLayers, VCoord->MinLayerCell.Ptr, VCoord->MaxLayerCell.Ptr, H.Ptr,
                     NonLocalShape.Ptr, Tr.Ptr, NTracers, Tr.Ext[1], Dt, Flux.Ptr, (size_t)Mesh->NCellsSize, S);
   ++LaunchCount;
}

void Kpp::copyToHost() {
   HIP_CHECK(hipDeviceSynchronize());
   OMEGA::copyToHost(FrictionVelocityH.data(), FrictionVelocity);
   OMEGA::copyToHost(SurfaceBuoyancyFluxH.data(), SurfaceBuoyancyFlux);
   OMEGA::copyToHost(BoundaryLayerDepthH.data(), BoundaryLayerDepth);
   OMEGA::copyToHost(BoundaryLayerIndexH.data(), BoundaryLayerIndex.Ptr, BoundaryLayerIndex.bytes());
   OMEGA::copyToHost(BulkRichardsonH.data(), BulkRichardson);
   OMEGA::copyToHost(NonLocalShapeH.data(), NonLocalShape);
}

void Kpp::copyToDevice() {
   OMEGA::copyToDevice(FrictionVelocity, FrictionVelocityH.data());
   OMEGA::copyToDevice(SurfaceBuoyancyFlux, SurfaceBuoyancyFluxH.data());
   OMEGA::copyToDevice(BoundaryLayerDepth, BoundaryLayerDepthH.data());
   OMEGA::copyToDevice(BoundaryLayerIndex.Ptr, BoundaryLayerIndexH.data(), BoundaryLayerIndex.bytes());
   OMEGA::copyToDevice(BulkRichardson, BulkRichardsonH.data());
   OMEGA::copyToDevice(NonLocalShape, NonLocalShapeH.data());
}

} // namespace OMEGA
