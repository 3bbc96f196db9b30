// PressureGrad.cpp -- see PressureGrad.h.
#include "PressureGrad.h"
#include "Pacer.h"
#include "kernels/PressureGradKernels.h"

namespace OMEGA {

PressureGrad::PressureGrad(const std::string &Name_, const HorzMesh *Mesh_, VertCoord *VCoord_, Eos *EqState_)
    : NVertLayers(0), Mesh(Mesh_), VCoord(VCoord_), EqState(EqState_), Name(Name_) {
   OMEGA_REQUIRE(Mesh != nullptr, "PressureGrad: mesh is NULL");
   OMEGA_REQUIRE(!Mesh->HostOnly,
                 "PressureGrad: the mesh was created host-only: no device arrays, compute is unavailable");
   OMEGA_REQUIRE(VCoord != nullptr, "PressureGrad: VertCoord is NULL");
   OMEGA_REQUIRE(EqState != nullptr, "PressureGrad: Eos is NULL");
   OMEGA_REQUIRE(VCoord->Mesh == Mesh, "PressureGrad: the VertCoord was built for another mesh");
   OMEGA_REQUIRE(EqState->Mesh == Mesh, "PressureGrad: the Eos was built for another mesh");
   OMEGA_REQUIRE(EqState->NVertLayers == VCoord->NVertLayers,
                 "PressureGrad: the VertCoord and the Eos have different layer counts");
   NVertLayers           = VCoord->NVertLayers;
   SurfacePressure       = Array1DReal("SurfacePressure", Mesh->NCellsSize);
   TidalPotential        = Array1DReal("TidalPotential", Mesh->NCellsSize);
   SelfAttractionLoading = Array1DReal("SelfAttractionLoading", Mesh->NCellsSize);
}

void PressureGrad::computePressureGrad(const Array2DReal &Tend, const Array2DReal &PMid, const Array2DReal &GeoMid,
                                       const Array2DReal &SpecVol, hipStream_t S) const {
   requireLevelArray("PressureGrad", Tend, Mesh->NEdgesSize, NVertLayers, "Tend");
   requireLevelArray("PressureGrad", PMid, Mesh->NCellsSize, NVertLayers, "PressureMid");
   requireLevelArray("PressureGrad", GeoMid, Mesh->NCellsSize, NVertLayers, "GeopotentialMid");
   requireLevelArray("PressureGrad", SpecVol, Mesh->NCellsSize, NVertLayers, "SpecVol");
   Pacer::Range Timer("PressureGrad:computePressureGrad", 1);
   PressureGradArgs A;
   A.NEdgesAll = Mesh->NEdgesAll, A.NCellsSize = Mesh->NCellsSize, A.K = NVertLayers;
   A.CellsOnEdge     = Mesh->CellsOnEdge.Ptr;
   A.MinLayerEdgeBot = VCoord->MinLayerEdgeBot.Ptr, A.MaxLayerEdgeTop = VCoord->MaxLayerEdgeTop.Ptr;
   A.DcEdge = Mesh->DcEdge.Ptr, A.EdgeMask = Mesh->EdgeMask1D.Ptr;
   A.PressureMid = PMid.Ptr, A.GeopotentialMid = GeoMid.Ptr, A.SpecVol = SpecVol.Ptr;
   A.Tend = Tend.Ptr;
   launchPressureGrad(A, S);
}

void PressureGrad::computePressureGrad(const Array2DReal &Tend, hipStream_t S) const {
   computePressureGrad(Tend, VCoord->PressureMid, VCoord->GeopotentialMid, EqState->SpecVol, S);
}

void PressureGrad::updateColumn(const Array2DReal &LayerThickness, const Array3DReal &TracerArray, hipStream_t S) const {
   VCoord->computeColumn(LayerThickness, TracerArray, *EqState, SurfacePressure, TidalPotential, SelfAttractionLoading,
                         false, 0, S, 0, 1);
}

} // namespace OMEGA
