// VertRemap.cpp -- see VertRemap.h.
#include "VertRemap.h"
#include "Pacer.h"
#include "kernels/VertRemapKernels.h"

namespace OMEGA {

int VertRemap::maxLayers() {
   // (levelPitch is monotone, so is the tile rule)
   int Lo = 1, Hi = 1 << 20;
   while (Lo < Hi) {
      const int Mid = Lo + (Hi - Lo + 1) / 2;
      if (vertRemapColumnTile(Mid) >= 2)
         Lo = Mid;
      else
         Hi = Mid - 1;
   }
   return Lo;
}

VertRemap::VertRemap(const std::string &Name_, const HorzMesh *Mesh_, const VertCoord *VCoord_, int MaxTracers_,
                     const VertRemapConfig &C)
    : NVertLayers(0), MaxTracers(MaxTracers_), Config(C), Mesh(Mesh_), VCoord(VCoord_), Name(Name_) {
   OMEGA_REQUIRE(Mesh != nullptr, "VertRemap: mesh is NULL");
   OMEGA_REQUIRE(!Mesh->HostOnly, "VertRemap: the mesh was created host-only: no device arrays, compute is unavailable");
   OMEGA_REQUIRE(VCoord != nullptr, "VertRemap: VertCoord is NULL");
   OMEGA_REQUIRE(VCoord->Mesh == Mesh, "VertRemap: the VertCoord was built for another mesh");
   OMEGA_REQUIRE(VCoord->NVertLayers == Mesh->NVertLayers,
                 "VertRemap: the VertCoord has another layer count (" + std::to_string(VCoord->NVertLayers) +
                     ") than the mesh (" + std::to_string(Mesh->NVertLayers) + ")");
   OMEGA_REQUIRE(Config.Order >= 1 && Config.Order <= 3,
                 "VertRemap: Order = " + std::to_string(Config.Order) + " is not supported: 1 (PCM), 2 (PLM) or 3 (PPM)");
   OMEGA_REQUIRE(MaxTracers >= 0, "VertRemap: MaxTracers = " + std::to_string(MaxTracers) + " is negative");
   NVertLayers = VCoord->NVertLayers;
   OMEGA_REQUIRE(NVertLayers >= 1 && vertRemapColumnTile(NVertLayers) >= 2,
                 "VertRemap: NVertLayers = " + std::to_string(NVertLayers) +
                     " is outside the supported 1 <= NVertLayers <= " + std::to_string(maxLayers()) +
                     " (what the column kernel's LDS tile holds)");
   LayerThicknessTarget  = Array2DReal::levels("LayerThicknessTarget", Mesh->NCellsSize, NVertLayers);
   LayerThicknessTargetH = HostArrayReal(Mesh->NCellsSize, NVertLayers);
}

void VertRemap::cellLaunch(const Array2DReal &H, const Array3DReal *Tracers, int NTracers, bool Target,
                           hipStream_t S) const {
   requireLevelArray("VertRemap", H, Mesh->NCellsSize, NVertLayers, "LayerThickness");
   OMEGA_REQUIRE(NTracers >= 0 && NTracers <= MaxTracers, "VertRemap: NTracers = " + std::to_string(NTracers) +
                                                              " is outside 0 .. MaxTracers = " + std::to_string(MaxTracers));
   if (NTracers > 0) {
      // (the kernel's plane stride: exactly NCellsSize rows per tracer)
      requireLevelArray("VertRemap", *Tracers, NTracers, Mesh->NCellsSize, NVertLayers, "Tracers", "NCellsSize");
      OMEGA_REQUIRE(Tracers->Ext[1] == Mesh->NCellsSize, levelArrayText("VertRemap", "Tracers", "[NTracers][NCellsSize]"));
   }
   if (!Target && NTracers == 0)
      return;
   VertRemapCellArgs A;
   A.NCellsAll = Mesh->NCellsAll, A.NCellsSize = Mesh->NCellsSize, A.K = NVertLayers, A.NTracers = NTracers;
   A.Order        = Config.Order;
   A.MinLayerCell = VCoord->MinLayerCell.Ptr, A.MaxLayerCell = VCoord->MaxLayerCell.Ptr;
   A.MoveWeights = VCoord->VertCoordMovementWeights.Ptr, A.RefThick = VCoord->RefLayerThickness.Ptr;
   A.LayerThick = H.Ptr, A.Target = LayerThicknessTarget.Ptr;
   A.Tracers    = NTracers > 0 ? Tracers->Ptr : nullptr;
   launchVertRemapCell(A, Target, S);
   ++LaunchCount;
}

void VertRemap::computeTarget(const Array2DReal &H, hipStream_t S) const {
   Pacer::Range Timer("VertRemap:computeTarget", 1);
   cellLaunch(H, nullptr, 0, true, S);
}

void VertRemap::remapTracers(const Array2DReal &H, const Array3DReal &Tracers, int NTracers, hipStream_t S) const {
   Pacer::Range Timer("VertRemap:remapTracers", 1);
   cellLaunch(H, &Tracers, NTracers, false, S);
}

void VertRemap::remapVelocity(const Array2DReal &H, const Array2DReal &U, hipStream_t S) const {
   requireLevelArray("VertRemap", H, Mesh->NCellsSize, NVertLayers, "LayerThickness");
   requireLevelArray("VertRemap", U, Mesh->NEdgesSize, NVertLayers, "NormalVelocity");
   Pacer::Range Timer("VertRemap:remapVelocity", 1);
   VertRemapEdgeArgs A;
   A.NEdgesAll = Mesh->NEdgesAll, A.NCellsSize = Mesh->NCellsSize, A.K = NVertLayers, A.Order = Config.Order;
   A.CellsOnEdge     = Mesh->CellsOnEdge.Ptr;
   A.MinLayerEdgeBot = VCoord->MinLayerEdgeBot.Ptr, A.MaxLayerEdgeTop = VCoord->MaxLayerEdgeTop.Ptr;
   A.LayerThick = H.Ptr, A.Target = LayerThicknessTarget.Ptr, A.NormalVelocity = U.Ptr;
   launchVertRemapEdge(A, S);
   ++LaunchCount;
}

void VertRemap::adoptTarget(const Array2DReal &H, hipStream_t S) const {
   requireLevelArray("VertRemap", H, Mesh->NCellsSize, NVertLayers, "LayerThickness");
   Pacer::Range Timer("VertRemap:adoptTarget", 1);
   VertRemapAdoptArgs A;
   A.NCellsAll = Mesh->NCellsAll, A.K = NVertLayers;
   A.MinLayerCell = VCoord->MinLayerCell.Ptr, A.MaxLayerCell = VCoord->MaxLayerCell.Ptr;
   A.Target = LayerThicknessTarget.Ptr, A.LayerThick = H.Ptr;
   launchVertRemapAdopt(A, S);
   ++LaunchCount;
}

void VertRemap::remap(const Array2DReal &H, const Array2DReal &U, const Array3DReal &Tracers, int NTracers,
                      hipStream_t S) const {
   Pacer::Range Timer("VertRemap:remap", 1);
   // every refusal before the first launch: the edge launch's arrays are checked here too
   requireLevelArray("VertRemap", U, Mesh->NEdgesSize, NVertLayers, "NormalVelocity");
   cellLaunch(H, &Tracers, NTracers, true, S); // the target and the tracers: neither writes what the other two read
   remapVelocity(H, U, S);                     // reads h and the target
   adoptTarget(H, S);                          // h last
}

void VertRemap::copyToHost() {
   HIP_CHECK(hipDeviceSynchronize());
   OMEGA::copyToHost(LayerThicknessTargetH.data(), LayerThicknessTarget);
}

} // namespace OMEGA
