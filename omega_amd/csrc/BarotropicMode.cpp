// BarotropicMode.cpp -- see BarotropicMode.h.
#include "BarotropicMode.h"
#include "Pacer.h"
#include "kernels/BarotropicKernels.h"

#include <algorithm>
#include <cmath>

namespace OMEGA {

int BarotropicMode::maxLayers() {
   // the largest K whose two-edge tile fits the LDS, found once (levelPitch is monotone, so is the tile rule)
   static const int Limit = [] {
      int K = 1;
      while (btrColumnTile(K + 1) >= 2)
         ++K;
      return K;
   }();
   return Limit;
}

BarotropicMode::BarotropicMode(const std::string &Name_, const HorzMesh *Mesh_, const VertCoord *VCoord_,
                               const BarotropicConfig &C)
    : NVertLayers(0), Config(C), Mesh(Mesh_), VCoord(VCoord_), Name(Name_) {
   OMEGA_REQUIRE(Mesh != nullptr, "BarotropicMode: mesh is NULL");
   OMEGA_REQUIRE(!Mesh->HostOnly,
                 "BarotropicMode: the mesh was created host-only: no device arrays, compute is unavailable");
   OMEGA_REQUIRE(VCoord != nullptr, "BarotropicMode: VertCoord is NULL");
   OMEGA_REQUIRE(VCoord->Mesh == Mesh, "BarotropicMode: the VertCoord was built for another mesh");
   OMEGA_REQUIRE(VCoord->NVertLayers == Mesh->NVertLayers,
                 "BarotropicMode: the VertCoord has another layer count (" + std::to_string(VCoord->NVertLayers) +
                     ") than the mesh (" + std::to_string(Mesh->NVertLayers) + ")");
   NVertLayers = VCoord->NVertLayers;
   OMEGA_REQUIRE(NVertLayers >= 1 && btrColumnTile(NVertLayers) >= 2,
                 "BarotropicMode: NVertLayers = " + std::to_string(NVertLayers) +
                     " is outside the supported 1 <= NVertLayers <= " + std::to_string(maxLayers()) +
                     " (what the column kernel's LDS tile holds)");
   const int NE = Mesh->NEdgesSize, NC = Mesh->NCellsSize, NEA = Mesh->NEdgesAll, NCA = Mesh->NCellsAll;
   const int ME = Mesh->MaxEdges, ME2 = Mesh->MaxEdges2;
   BtrVelocity  = Array1DReal("BtrVelocity", NE);
   BtrThickEdge = Array1DReal("BtrThickEdge", NE);
   BtrForcing   = Array1DReal("BtrForcing", NE);
   BtrFluxMean  = Array1DReal("BtrFluxMean", NE);
   BtrTendMean  = Array1DReal("BtrTendMean", NE);
   SSH          = Array1DReal("SSH", NC);
   BclVelocity  = Array2DReal::levels("BclVelocity", NE, NVertLayers);
   BtrVelocityH = HostArrayReal(NE), BtrThickEdgeH = HostArrayReal(NE), BtrForcingH = HostArrayReal(NE);
   BtrFluxMeanH = HostArrayReal(NE), BtrTendMeanH = HostArrayReal(NE), SSHH = HostArrayReal(NC), BclVelocityH = HostArrayReal(NE, NVertLayers);
   SSHNext         = Array1DReal("SSHNext", NC);
   BtrVelocityNext = Array1DReal("BtrVelocityNext", NE);

   // the Coriolis weights, and the slot-major tables of the sub-step kernels
   CorWeightH      = HostArrayReal(NE, ME2, 1, 0.0);
   const int NSlotE = std::max(ME2 * NEA, 1), NSlotC = std::max(ME * NCA, 1);
   HostArrayReal CorT(NSlotE, 1, 1, 0.0);
   HostArrayI4 EoET(NSlotE, 1, 1, -1);
   for (int E = 0; E < NEA; ++E)
      for (int J = 0; J < ME2 && J < Mesh->NEdgesOnEdgeH(E); ++J) {
         const I4 Ej = Mesh->EdgesOnEdgeH(E, J);
         if (Ej < 0 || Ej >= NEA)
            continue; // a hole of a culled mesh: no weight, and the kernel skips the slot
         CorWeightH(E, J)           = Mesh->WeightsOnEdgeH(E, J) * Mesh->FEdgeH(Ej);
         CorT.V[(size_t)J * NEA + E] = CorWeightH(E, J);
         EoET.V[(size_t)J * NEA + E] = Ej;
      }
   HostArrayReal DvT(NSlotC, 1, 1, 0.0);
   HostArrayI4 EdgeT(NSlotC, 1, 1, 0), NbrT(NSlotC, 1, 1, -1);
   for (int Cl = 0; Cl < NCA; ++Cl)
      for (int J = 0; J < ME && J < Mesh->NEdgesOnCellH(Cl); ++J) {
         const I4 E = Mesh->EdgesOnCellH(Cl, J);
         if (E < 0 || E >= NEA)
            continue;
         const size_t At = (size_t)J * NCA + Cl;
         EdgeT.V[At]     = E;
         DvT.V[At]       = Mesh->DvEdgeH(E) * Mesh->EdgeSignOnCellH(Cl, J);
         const I4 C0 = Mesh->CellsOnEdgeH(E, 0), C1 = Mesh->CellsOnEdgeH(E, 1);
         if (Mesh->EdgeMask1DH(E) != 0.0 && (C0 == Cl || C1 == Cl))
            NbrT.V[At] = C0 == Cl ? C1 : C0;
      }
   CorSlot    = createDeviceMirrorCopy<Real, 1>("BtrCorSlot", CorT);
   EoESlot    = createDeviceMirrorCopy<I4, 1>("BtrEoESlot", EoET);
   DvSignSlot = createDeviceMirrorCopy<Real, 1>("BtrDvSignSlot", DvT);
   EdgeSlot   = createDeviceMirrorCopy<I4, 1>("BtrEdgeSlot", EdgeT);
   NbrSlot    = createDeviceMirrorCopy<I4, 1>("BtrNbrSlot", NbrT);
}

void BarotropicMode::columnLaunch(const Array2DReal &H, const Array2DReal *Field, int EdgeMode, bool Cells,
                                  hipStream_t S) const {
   requireLevelArray("BarotropicMode", H, Mesh->NCellsSize, NVertLayers, "LayerThickness");
   if (Field)
      requireLevelArray("BarotropicMode", *Field, Mesh->NEdgesSize, NVertLayers,
                        EdgeMode == BtrEdgeSplit ? "NormalVelocity" : "the velocity tendency");
   BtrColumnArgs A;
   A.NEdgesAll = Mesh->NEdgesAll, A.NCellsAll = Mesh->NCellsAll, A.NCellsSize = Mesh->NCellsSize, A.K = NVertLayers;
   A.CellsOnEdge     = Mesh->CellsOnEdge.Ptr;
   A.MinLayerEdgeBot = VCoord->MinLayerEdgeBot.Ptr, A.MaxLayerEdgeTop = VCoord->MaxLayerEdgeTop.Ptr;
   A.MinLayerCell = VCoord->MinLayerCell.Ptr, A.MaxLayerCell = VCoord->MaxLayerCell.Ptr;
   A.BottomDepth = VCoord->BottomDepth.Ptr;
   A.LayerThick = H.Ptr, A.EdgeField = Field ? Field->Ptr : nullptr;
   A.BtrThickEdge = BtrThickEdge.Ptr;
   A.BtrOut = EdgeMode == BtrEdgeForcing ? BtrForcing.Ptr : EdgeMode == BtrEdgeTendMean ? BtrTendMean.Ptr : BtrVelocity.Ptr;
   A.BclVelocity = BclVelocity.Ptr, A.SSH = SSH.Ptr;
   launchBtrColumn(A, (BtrEdgeMode)EdgeMode, Cells, S);
}

void BarotropicMode::splitVelocity(const Array2DReal &H, const Array2DReal &U, hipStream_t S) const {
   Pacer::Range Timer("BarotropicMode:splitVelocity", 1);
   columnLaunch(H, &U, BtrEdgeSplit, false, S);
}

void BarotropicMode::computeForcing(const Array2DReal &H, const Array2DReal &VelTend, hipStream_t S) const {
   Pacer::Range Timer("BarotropicMode:computeForcing", 1);
   columnLaunch(H, &VelTend, BtrEdgeForcing, false, S);
}

void BarotropicMode::computeSSH(const Array2DReal &H, hipStream_t S) const {
   Pacer::Range Timer("BarotropicMode:computeSSH", 1);
   columnLaunch(H, nullptr, BtrEdgeNone, true, S);
}

void BarotropicMode::splitVelocityAndSSH(const Array2DReal &H, const Array2DReal &U, hipStream_t S) const {
   Pacer::Range Timer("BarotropicMode:splitVelocityAndSSH", 1);
   columnLaunch(H, &U, BtrEdgeSplit, true, S);
}

void BarotropicMode::levelLaunch(int Op, const Array2DReal *VelOld, const Array2DReal *VelTend, Real Dt,
                                 const Array2DReal &VelOut, hipStream_t S) const {
   const char *OutName = Op == BtrLevelRecombine ? "NormalVelocity" : "the velocity written";
   requireLevelArray("BarotropicMode", VelOut, Mesh->NEdgesSize, NVertLayers, OutName);
   if (VelOld)
      requireLevelArray("BarotropicMode", *VelOld, Mesh->NEdgesSize, NVertLayers, "the old velocity");
   if (VelTend)
      requireLevelArray("BarotropicMode", *VelTend, Mesh->NEdgesSize, NVertLayers, "the velocity tendency");
   BtrLevelArgs A;
   A.NEdgesAll = Mesh->NEdgesAll, A.K = NVertLayers, A.Dt = Dt;
   A.MinLayerEdgeBot = VCoord->MinLayerEdgeBot.Ptr, A.MaxLayerEdgeTop = VCoord->MaxLayerEdgeTop.Ptr;
   A.BtrVelocity = BtrVelocity.Ptr, A.BtrFluxMean = BtrFluxMean.Ptr, A.BtrThickEdge = BtrThickEdge.Ptr;
   A.BtrTendMean = BtrTendMean.Ptr, A.BclVelocity = BclVelocity.Ptr;
   A.VelOld = VelOld ? VelOld->Ptr : nullptr, A.VelTend = VelTend ? VelTend->Ptr : nullptr, A.VelOut = VelOut.Ptr;
   launchBtrLevels(A, (BtrLevelOp)Op, S);
}

void BarotropicMode::recombine(const Array2DReal &U, hipStream_t S) const {
   Pacer::Range Timer("BarotropicMode:recombine", 1);
   levelLaunch(BtrLevelRecombine, nullptr, nullptr, 0.0, U, S);
}

void BarotropicMode::transportVelocity(const Array2DReal &UOld, const Array2DReal &UOut, hipStream_t S) const {
   Pacer::Range Timer("BarotropicMode:transportVelocity", 1);
   levelLaunch(BtrLevelTransport, &UOld, nullptr, 0.0, UOut, S);
}

void BarotropicMode::advanceVelocity(const Array2DReal &UOld, const Array2DReal &VelTend, Real Dt, const Array2DReal &UOut,
                                     hipStream_t S) const {
   OMEGA_REQUIRE(std::isfinite(Dt) && Dt > 0.0,
                 "BarotropicMode: advanceVelocity: Dt = " + std::to_string(Dt) + " is not a finite, positive time step");
   Pacer::Range Timer("BarotropicMode:advanceVelocity", 1);
   levelLaunch(BtrLevelAdvance, &UOld, &VelTend, Dt, UOut, S);
}

/// the mesh tables and constants of the sub-step kernels; the fields are the caller's to set
struct BarotropicMode::SubTables : BtrSubArgs {
   explicit SubTables(const BarotropicMode &B) {
      const HorzMesh *M = B.Mesh;
      const MeshView &V = M->view();
      NCellsAll = M->NCellsAll, NEdgesAll = M->NEdgesAll, MaxEdges = M->MaxEdges, MaxEdges2 = M->MaxEdges2;
      Gravity      = B.Config.Gravity;
      NEdgesOnCell = M->NEdgesOnCell.Ptr, EdgeSlot = B.EdgeSlot.Ptr, NbrSlot = B.NbrSlot.Ptr;
      DvSignSlot = B.DvSignSlot.Ptr, InvAreaCell = V.InvAreaCell;
      CellsOnEdge = M->CellsOnEdge.Ptr, EdgeMask = M->EdgeMask1D.Ptr, InvDcEdge = V.InvDcEdge;
      NEdgesOnEdge = M->NEdgesOnEdge.Ptr, EoESlot = B.EoESlot.Ptr, CorSlot = B.CorSlot.Ptr;
      BottomDepth = B.VCoord->BottomDepth.Ptr;
   }
};

void BarotropicMode::computeResidualForcing(const Array2DReal &H, const Array2DReal &VelTend, hipStream_t S) const {
   Pacer::Range Timer("BarotropicMode:computeResidualForcing", 1);
   columnLaunch(H, &VelTend, BtrEdgeTendMean, false, S);
   SubTables A(*this);
   A.SSH = SSH.Ptr, A.Vel = BtrVelocity.Ptr;
   launchBtrResidual(A, BtrTendMean.Ptr, BtrForcing.Ptr, S);
}

void BarotropicMode::subcycle(int NSub, Real DtBtr, hipStream_t S) const {
   OMEGA_REQUIRE(NSub >= 1, "BarotropicMode: NSub = " + std::to_string(NSub) + " is not a number of sub-steps (>= 1)");
   OMEGA_REQUIRE(std::isfinite(DtBtr) && DtBtr > 0.0,
                 "BarotropicMode: DtBtr = " + std::to_string(DtBtr) + " is not a finite, positive time step");
   Pacer::Range Timer("BarotropicMode:subcycle", 1);
   SubTables A(*this);
   A.Dt = DtBtr, A.Forcing = BtrForcing.Ptr, A.FluxSum = BtrFluxMean.Ptr;
   deviceFill0(BtrFluxMean.Ptr, (size_t)Mesh->NEdgesAll * sizeof(Real), S);
   // sub-step I reads one half of each double buffer and writes the other; an odd count ends in the second halves
   Real *Eta[2] = {SSH.Ptr, SSHNext.Ptr}, *Vel[2] = {BtrVelocity.Ptr, BtrVelocityNext.Ptr};
   for (int I = 0; I < NSub; ++I) {
      A.SSH = Eta[I & 1], A.SSHNew = Eta[(I + 1) & 1];
      A.Vel = Vel[I & 1], A.VelNew = Vel[(I + 1) & 1];
      launchBtrCells(A, S);
      launchBtrEdges(A, S);
   }
   if (NSub & 1) {
      deviceCopy(SSH.Ptr, SSHNext.Ptr, (size_t)Mesh->NCellsAll * sizeof(Real), S);
      deviceCopy(BtrVelocity.Ptr, BtrVelocityNext.Ptr, (size_t)Mesh->NEdgesAll * sizeof(Real), S);
   }
   launchBtrDivide(BtrFluxMean.Ptr, Mesh->NEdgesAll, (Real)NSub, S);
}

void BarotropicMode::copyToHost() {
   HIP_CHECK(hipDeviceSynchronize());
   OMEGA::copyToHost(BtrVelocityH.data(), BtrVelocity);
   OMEGA::copyToHost(BtrThickEdgeH.data(), BtrThickEdge);
   OMEGA::copyToHost(BtrForcingH.data(), BtrForcing);
   OMEGA::copyToHost(BtrFluxMeanH.data(), BtrFluxMean);
   OMEGA::copyToHost(BtrTendMeanH.data(), BtrTendMean);
   OMEGA::copyToHost(SSHH.data(), SSH);
   OMEGA::copyToHost(BclVelocityH.data(), BclVelocity);
}

} // namespace OMEGA
