// PressureGrad.cpp -- see PressureGrad.h.
#include "PressureGrad.h"
#include "Pacer.h"
#include "kernels/PressureGradKernels.h"

namespace OMEGA {

PressureGrad::PressureGrad(const std::string &Name_, const HorzMesh *Mesh_, VertCoord *VCoord_, Eos *EqState_)
    : ColumnPass(Mesh_, VCoord_, EqState_), Name(Name_) {
   OMEGA_REQUIRE(Mesh != nullptr, "PressureGrad: mesh is NULL");
   requireFits("PressureGrad");
   allocateForcing();
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

} // namespace OMEGA
