// Redi.cpp -- see Redi.h.
#include "Redi.h"
#include "Pacer.h"
#include "kernels/RediKernels.h"

#include <cmath>
#include <vector>

namespace OMEGA {

Redi::Redi(const std::string &Name_, const HorzMesh *Mesh_, VertCoord *VCoord_, Eos *EqState_, int MaxTracers_,
           Real RediKappa_, Real SlopeMax_, Real N2Floor_)
    : ColumnPass(Mesh_, VCoord_, EqState_), MaxTracers(MaxTracers_), RediKappa(RediKappa_), SlopeMax(SlopeMax_),
      N2Floor(N2Floor_), Name(Name_) {
   OMEGA_REQUIRE(Mesh != nullptr, "Redi: mesh is NULL");
   OMEGA_REQUIRE(std::isfinite(RediKappa) && RediKappa >= 0.0,
                 "Redi: RediKappa = " + std::to_string(RediKappa) + " is negative or not finite");
   OMEGA_REQUIRE(std::isfinite(SlopeMax) && SlopeMax > 0.0,
                 "Redi: SlopeMax = " + std::to_string(SlopeMax) + " is not finite or not positive");
   OMEGA_REQUIRE(std::isfinite(N2Floor) && N2Floor > 0.0,
                 "Redi: N2Floor = " + std::to_string(N2Floor) + " is not finite or not positive");
   OMEGA_REQUIRE(MaxTracers >= 1, "Redi: MaxTracers = " + std::to_string(MaxTracers) + " is below 1");
   requireFits("Redi");
   requirePackedLayers("Redi", NVertLayers);
   Kappa           = Array1DReal("Kappa", Mesh->NEdgesSize);
   SlopeInterface  = Array2DReal::levels("SlopeInterface", Mesh->NEdgesSize, NVertLayers);
   VertDiffusivity = Array2DReal::levels("VertDiffusivity", Mesh->NCellsSize, NVertLayers);
   allocateForcing();
   const std::vector<Real> Fill((size_t)Mesh->NEdgesSize, RediKappa);
   copyToDevice(Kappa, Fill.data());
}

void Redi::computeSlope(const Array2DReal &H, const Array2DReal &SpecVol, const Array2DReal &SpecVolDisp,
                        const Array2DReal &ZMid, hipStream_t S) const {
   RediSlopeArgs A;
   stratificationArgs("Redi", A, H, SpecVol, SpecVolDisp, ZMid);
   Pacer::Range Timer("Redi:computeSlope", 1);
   A.SlopeMax = SlopeMax, A.N2Floor = N2Floor;
   A.SlopeInterface = SlopeInterface.Ptr;
   launchRediSlope(A, S);
   ++LaunchCount;
}

void Redi::computeSlope(const Array2DReal &H, hipStream_t S) const {
   computeSlope(H, EqState->SpecVol, EqState->SpecVolDisplaced, VCoord->ZMid, S);
}

/// the tables both cell launches stage
static RediCellArgs cellArgs(const Redi &R) {
   const HorzMesh *Mesh = R.Mesh;
   RediCellArgs A;
   A.NCellsAll = Mesh->NCellsAll, A.NCellsSize = Mesh->NCellsSize, A.NEdgesAll = Mesh->NEdgesAll;
   A.K = R.NVertLayers, A.MaxEdges = Mesh->MaxEdges;
   A.NEdgesOnCell = Mesh->NEdgesOnCell.Ptr, A.EdgesOnCell = Mesh->EdgesOnCell.Ptr;
   A.CellsOnEdge    = Mesh->CellsOnEdge.Ptr;
   A.EdgeSignOnCell = Mesh->EdgeSignOnCell.Ptr;
   A.AreaCell = Mesh->AreaCell.Ptr, A.DcEdge = Mesh->DcEdge.Ptr, A.DvEdge = Mesh->DvEdge.Ptr, A.Kappa = R.Kappa.Ptr;
   A.MinLayerCell = R.VCoord->MinLayerCell.Ptr, A.MaxLayerCell = R.VCoord->MaxLayerCell.Ptr;
   A.MinLayerEdgeBot = R.VCoord->MinLayerEdgeBot.Ptr, A.MaxLayerEdgeTop = R.VCoord->MaxLayerEdgeTop.Ptr;
   A.SlopeInterface = R.SlopeInterface.Ptr;
   return A;
}

void Redi::addTracerTend(const Array3DReal &Tend, const Array2DReal &H, const Array3DReal &Tracers, int NTracers,
                         const Array2DReal &ZMid, hipStream_t S) const {
   OMEGA_REQUIRE(NTracers >= 1 && NTracers <= MaxTracers, "Redi: NTracers = " + std::to_string(NTracers) +
                                                              " is outside 1 .. MaxTracers = " + std::to_string(MaxTracers));
   requireLevelArray("Redi", Tend, NTracers, Mesh->NCellsSize, NVertLayers, "TracerTend", "NCellsSize");
   requireLevelArray("Redi", H, Mesh->NCellsSize, NVertLayers, "LayerThickness");
   requireLevelArray("Redi", Tracers, NTracers, Mesh->NCellsSize, NVertLayers, "Tracers", "NCellsSize");
   requireLevelArray("Redi", ZMid, Mesh->NCellsSize, NVertLayers, "ZMid");
   Pacer::Range Timer("Redi:addTracerTend", 1);
   RediCellArgs A   = cellArgs(*this);
   A.LayerThickness = H.Ptr, A.ZMid = ZMid.Ptr;
   A.Tracers = Tracers.Ptr, A.Tend = Tend.Ptr;
   A.NTracers = NTracers, A.TrRows = Tracers.Ext[1], A.TendRows = Tend.Ext[1];
   launchRediTracerTend(A, S);
   ++LaunchCount;
}

void Redi::addTracerTend(const Array3DReal &Tend, const Array2DReal &H, const Array3DReal &Tracers, int NTracers,
                         hipStream_t S) const {
   addTracerTend(Tend, H, Tracers, NTracers, VCoord->ZMid, S);
}

void Redi::computeVertDiffusivity(const Array2DReal &VertDiff, hipStream_t S) const {
   if (VertDiff.Ptr != nullptr)
      requireLevelArray("Redi", VertDiff, Mesh->NCellsSize, NVertLayers, "VertDiff");
   Pacer::Range Timer("Redi:computeVertDiffusivity", 1);
   RediCellArgs A    = cellArgs(*this);
   A.VertDiffusivity = VertDiffusivity.Ptr;
   A.VertDiff        = VertDiff.Ptr;
   launchRediVertDiffusivity(A, S);
   ++LaunchCount;
}

} // namespace OMEGA
