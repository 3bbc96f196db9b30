// VertAdv.cpp -- see VertAdv.h.
#include "VertAdv.h"
#include "Pacer.h"
#include "kernels/VertAdvKernels.h"

namespace OMEGA {

int VertAdv::maxLayers() {
   // (levelPitch is monotone, so is the tile rule)
   int Lo = 1, Hi = 1 << 20;
   while (Lo < Hi) {
      const int Mid = Lo + (Hi - Lo + 1) / 2;
      if (vertAdvColumnTile(Mid) >= 2)
         Lo = Mid;
      else
         Hi = Mid - 1;
   }
   return Lo;
}

VertAdv::VertAdv(const std::string &Name_, const HorzMesh *Mesh_, const VertCoord *VCoord_, const VertAdvConfig &C)
    : NVertLayers(0), Config(C), Mesh(Mesh_), VCoord(VCoord_), Name(Name_) {
   OMEGA_REQUIRE(Mesh != nullptr, "VertAdv: mesh is NULL");
   OMEGA_REQUIRE(!Mesh->HostOnly, "VertAdv: the mesh was created host-only: no device arrays, compute is unavailable");
   OMEGA_REQUIRE(VCoord != nullptr, "VertAdv: VertCoord is NULL");
   OMEGA_REQUIRE(VCoord->Mesh == Mesh, "VertAdv: the VertCoord was built for another mesh");
   OMEGA_REQUIRE(VCoord->NVertLayers == Mesh->NVertLayers,
                 "VertAdv: the VertCoord has another layer count (" + std::to_string(VCoord->NVertLayers) +
                     ") than the mesh (" + std::to_string(Mesh->NVertLayers) + ")");
   OMEGA_REQUIRE(Config.TracerFluxOrder == 1 || Config.TracerFluxOrder == 2,
                 "VertAdv: TracerFluxOrder = " + std::to_string(Config.TracerFluxOrder) +
                     " is not supported: 1 (upwind) or 2 (centred)");
   NVertLayers = VCoord->NVertLayers;
   OMEGA_REQUIRE(NVertLayers >= 1 && vertAdvColumnTile(NVertLayers) >= 2,
                 "VertAdv: NVertLayers = " + std::to_string(NVertLayers) +
                     " is outside the supported 1 <= NVertLayers <= " + std::to_string(maxLayers()) +
                     " (what the column kernel's LDS tile holds)");
   VerticalTransport  = Array2DReal::levels("VerticalTransport", Mesh->NCellsSize, NVertLayers);
   VerticalTransportH = HostArrayReal(Mesh->NCellsSize, NVertLayers);
}

/// a tracer array of the kernel's plane stride: exactly NCellsSize rows per tracer
static void requirePlanes(const Array3DReal &A, int NT, int Rows, int K, const char *What) {
   requireLevelArray("VertAdv", A, NT, Rows, K, What);
   OMEGA_REQUIRE(A.Ext[1] == Rows, levelArrayText("VertAdv", What, "[NTracers][" + std::to_string(Rows) + "]"));
}

void VertAdv::columnLaunch(const Array2DReal &Tend, bool Scan, bool Thick, hipStream_t S) const {
   requireLevelArray("VertAdv", Tend, Mesh->NCellsSize, NVertLayers, "the thickness tendency");
   VertAdvColumnArgs A;
   A.NCellsAll = Mesh->NCellsAll, A.K = NVertLayers;
   A.MinLayerCell = VCoord->MinLayerCell.Ptr, A.MaxLayerCell = VCoord->MaxLayerCell.Ptr;
   A.MoveWeights = VCoord->VertCoordMovementWeights.Ptr, A.RefThick = VCoord->RefLayerThickness.Ptr;
   A.Tend = Tend.Ptr, A.Transport = VerticalTransport.Ptr;
   launchVertAdvColumn(A, Scan, Thick, S);
}

void VertAdv::computeVerticalTransport(const Array2DReal &ThickTend, hipStream_t S) const {
   Pacer::Range Timer("VertAdv:computeVerticalTransport", 1);
   columnLaunch(ThickTend, true, false, S);
}

void VertAdv::addThicknessTend(const Array2DReal &Tend, hipStream_t S) const {
   Pacer::Range Timer("VertAdv:addThicknessTend", 1);
   columnLaunch(Tend, false, true, S);
}

void VertAdv::computeAndAddThickness(const Array2DReal &Tend, hipStream_t S) const {
   Pacer::Range Timer("VertAdv:computeAndAddThickness", 1);
   columnLaunch(Tend, true, true, S);
}

void VertAdv::addTracerTend(const Array3DReal &Tend, const Array2DReal &H, const Array3DReal &Tracers, int NTracers,
                            hipStream_t S) const {
   OMEGA_REQUIRE(NTracers >= 0, "VertAdv: NTracers is negative");
   if (NTracers == 0)
      return;
   requirePlanes(Tend, NTracers, Mesh->NCellsSize, NVertLayers, "the tracer tendency");
   requirePlanes(Tracers, NTracers, Mesh->NCellsSize, NVertLayers, "Tracers");
   requireLevelArray("VertAdv", H, Mesh->NCellsSize, NVertLayers, "LayerThickness");
   Pacer::Range Timer("VertAdv:addTracerTend", 1);
   VertAdvTracerArgs A;
   A.NCellsAll = Mesh->NCellsAll, A.NCellsSize = Mesh->NCellsSize, A.K = NVertLayers, A.NTracers = NTracers;
   A.Order        = Config.TracerFluxOrder;
   A.MinLayerCell = VCoord->MinLayerCell.Ptr, A.MaxLayerCell = VCoord->MaxLayerCell.Ptr;
   A.Transport = VerticalTransport.Ptr, A.LayerThick = H.Ptr, A.Tracers = Tracers.Ptr, A.Tend = Tend.Ptr;
   launchVertAdvTracer(A, S);
}

void VertAdv::addVelocityTend(const Array2DReal &Tend, const Array2DReal &H, const Array2DReal &U, hipStream_t S) const {
   requireLevelArray("VertAdv", Tend, Mesh->NEdgesSize, NVertLayers, "the velocity tendency");
   requireLevelArray("VertAdv", H, Mesh->NCellsSize, NVertLayers, "LayerThickness");
   requireLevelArray("VertAdv", U, Mesh->NEdgesSize, NVertLayers, "NormalVelocity");
   Pacer::Range Timer("VertAdv:addVelocityTend", 1);
   VertAdvEdgeArgs A;
   A.NEdgesAll = Mesh->NEdgesAll, A.NCellsSize = Mesh->NCellsSize, A.K = NVertLayers;
   A.CellsOnEdge     = Mesh->CellsOnEdge.Ptr;
   A.MinLayerEdgeBot = VCoord->MinLayerEdgeBot.Ptr, A.MaxLayerEdgeTop = VCoord->MaxLayerEdgeTop.Ptr;
   A.EdgeMask  = Mesh->EdgeMask1D.Ptr;
   A.Transport = VerticalTransport.Ptr, A.LayerThick = H.Ptr, A.NormalVelocity = U.Ptr, A.Tend = Tend.Ptr;
   launchVertAdvEdge(A, S);
}

void VertAdv::copyToHost() {
   HIP_CHECK(hipDeviceSynchronize());
   OMEGA::copyToHost(VerticalTransportH.data(), VerticalTransport);
}

} // namespace OMEGA
