// GentMcWilliams.cpp -- see GentMcWilliams.h.
#include "GentMcWilliams.h"
#include "Pacer.h"
#include "kernels/GMKernels.h"
#include "kernels/TriDiagKernels.h"

#include <cmath>
#include <vector>

namespace OMEGA {

GentMcWilliams::GentMcWilliams(const std::string &Name_, const HorzMesh *Mesh_, VertCoord *VCoord_, Eos *EqState_,
                               Real GMKappa_, Real GravWaveSpeed_)
    : NVertLayers(0), GMKappa(GMKappa_), GravWaveSpeed(GravWaveSpeed_), Mesh(Mesh_), VCoord(VCoord_), EqState(EqState_),
      Name(Name_) {
   OMEGA_REQUIRE(Mesh != nullptr, "GentMcWilliams: mesh is NULL");
   OMEGA_REQUIRE(std::isfinite(GMKappa) && GMKappa >= 0.0,
                 "GentMcWilliams: GMKappa = " + std::to_string(GMKappa) + " is negative or not finite");
   OMEGA_REQUIRE(std::isfinite(GravWaveSpeed) && GravWaveSpeed > 0.0,
                 "GentMcWilliams: GravWaveSpeed = " + std::to_string(GravWaveSpeed) + " is not finite or not positive");
   OMEGA_REQUIRE(!Mesh->HostOnly,
                 "GentMcWilliams: the mesh was created host-only: no device arrays, compute is unavailable");
   OMEGA_REQUIRE(VCoord != nullptr, "GentMcWilliams: VertCoord is NULL");
   OMEGA_REQUIRE(EqState != nullptr, "GentMcWilliams: Eos is NULL");
   OMEGA_REQUIRE(VCoord->Mesh == Mesh, "GentMcWilliams: the VertCoord was built for another mesh");
   OMEGA_REQUIRE(EqState->Mesh == Mesh, "GentMcWilliams: the Eos was built for another mesh");
   OMEGA_REQUIRE(EqState->NVertLayers == VCoord->NVertLayers,
                 "GentMcWilliams: the VertCoord and the Eos have different layer counts");
   OMEGA_REQUIRE(VCoord->NVertLayers >= 1 && VCoord->NVertLayers <= TriDiagMaxRows,
                 "GentMcWilliams: NVertLayers = " + std::to_string(VCoord->NVertLayers) +
                     " is outside the supported 1 <= NVertLayers <= " + std::to_string(TriDiagMaxRows));
   NVertLayers           = VCoord->NVertLayers;
   Kappa                 = Array1DReal("Kappa", Mesh->NEdgesSize);
   BolusVelocity         = Array2DReal::levels("BolusVelocity", Mesh->NEdgesSize, NVertLayers);
   StreamFunction        = Array2DReal::levels("StreamFunction", Mesh->NEdgesSize, NVertLayers);
   SurfacePressure       = Array1DReal("SurfacePressure", Mesh->NCellsSize);
   TidalPotential        = Array1DReal("TidalPotential", Mesh->NCellsSize);
   SelfAttractionLoading = Array1DReal("SelfAttractionLoading", Mesh->NCellsSize);
   const std::vector<Real> Fill((size_t)Mesh->NEdgesSize, GMKappa);
   copyToDevice(Kappa, Fill.data());
}

void GentMcWilliams::updateColumn(const Array2DReal &LayerThickness, const Array3DReal &TracerArray,
                                  hipStream_t S) const {
   VCoord->computeColumn(LayerThickness, TracerArray, *EqState, SurfacePressure, TidalPotential, SelfAttractionLoading,
                         true, 1, S, 0, 1);
}

void GentMcWilliams::computeBolusVelocity(const Array2DReal &H, const Array2DReal &SpecVol, const Array2DReal &SpecVolDisp,
                                          const Array2DReal &ZMid, const Array2DReal &Transport, hipStream_t S) const {
   requireLevelArray("GentMcWilliams", H, Mesh->NCellsSize, NVertLayers, "LayerThickness");
   requireLevelArray("GentMcWilliams", SpecVol, Mesh->NCellsSize, NVertLayers, "SpecVol");
   requireLevelArray("GentMcWilliams", SpecVolDisp, Mesh->NCellsSize, NVertLayers, "SpecVolDisplaced");
   requireLevelArray("GentMcWilliams", ZMid, Mesh->NCellsSize, NVertLayers, "ZMid");
   if (Transport.Ptr != nullptr)
      requireLevelArray("GentMcWilliams", Transport, Mesh->NEdgesSize, NVertLayers, "Transport");
   Pacer::Range Timer("GentMcWilliams:computeBolusVelocity", 1);
   GMArgs A;
   A.NEdgesAll = Mesh->NEdgesAll, A.K = NVertLayers;
   A.CellsOnEdge     = Mesh->CellsOnEdge.Ptr;
   A.MinLayerEdgeBot = VCoord->MinLayerEdgeBot.Ptr, A.MaxLayerEdgeTop = VCoord->MaxLayerEdgeTop.Ptr;
   A.DcEdge = Mesh->DcEdge.Ptr, A.Kappa = Kappa.Ptr;
   A.C2        = GravWaveSpeed * GravWaveSpeed;
   A.GOverRho0 = VertCoord::Gravity / VCoord->Rho0;
   A.LayerThickness = H.Ptr, A.SpecVol = SpecVol.Ptr, A.SpecVolDisplaced = SpecVolDisp.Ptr, A.ZMid = ZMid.Ptr;
   A.BolusVelocity = BolusVelocity.Ptr, A.StreamFunction = StreamFunction.Ptr;
   A.Transport = Transport.Ptr;
   launchBolusVelocity(A, S);
}

void GentMcWilliams::computeBolusVelocity(const Array2DReal &H, const Array2DReal &Transport, hipStream_t S) const {
   computeBolusVelocity(H, EqState->SpecVol, EqState->SpecVolDisplaced, VCoord->ZMid, Transport, S);
}

} // namespace OMEGA
