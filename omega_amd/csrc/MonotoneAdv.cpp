// MonotoneAdv.cpp -- see MonotoneAdv.h.
#include "MonotoneAdv.h"
#include "Pacer.h"
#include "kernels/MonotoneAdvKernels.h"

#include <cmath>

namespace OMEGA {

MonotoneAdv::MonotoneAdv(const std::string &Name_, const HorzMesh *Mesh_, int K, int MaxTracers_, const MonotoneAdvConfig &C)
    : NVertLayers(K), MaxTracers(MaxTracers_), Config(C), Mesh(Mesh_), Name(Name_) {
   OMEGA_REQUIRE(Mesh != nullptr, "MonotoneAdv: mesh is NULL");
   OMEGA_REQUIRE(!Mesh->HostOnly, "MonotoneAdv: the mesh was created host-only: no device arrays, compute is unavailable");
   OMEGA_REQUIRE(NVertLayers >= 1, "MonotoneAdv: NVertLayers = " + std::to_string(NVertLayers) + " is not a layer count (>= 1)");
   OMEGA_REQUIRE(MaxTracers >= 1, "MonotoneAdv: MaxTracers = " + std::to_string(MaxTracers) + " is not a tracer count (>= 1)");
   ScaleIn   = Array3DReal::levels("ScaleIn", MaxTracers, Mesh->NCellsSize, NVertLayers);
   ScaleOut  = Array3DReal::levels("ScaleOut", MaxTracers, Mesh->NCellsSize, NVertLayers);
   ScaleInH  = HostArrayReal(MaxTracers, Mesh->NCellsSize, NVertLayers);
   ScaleOutH = HostArrayReal(MaxTracers, Mesh->NCellsSize, NVertLayers);
}

void MonotoneAdv::attachVertAdv(const VertAdv *V) {
   OMEGA_REQUIRE(V == nullptr || (V->Mesh == Mesh && V->NVertLayers == NVertLayers),
                 "MonotoneAdv::attachVertAdv: the VertAdv was built for another mesh or layer count");
   VAdv = V;
}

/// a tracer array of the kernel's plane stride: exactly NCellsSize rows per tracer
static void requirePlanes(const Array3DReal &A, int NT, int Rows, int K, const char *What) {
   requireLevelArray("MonotoneAdv", A, NT, Rows, K, What);
   OMEGA_REQUIRE(A.Ext[1] == Rows, levelArrayText("MonotoneAdv", What, "[NTracers][" + std::to_string(Rows) + "]"));
}

void MonotoneAdv::addTracerTend(const Array3DReal &Tend, const Array2DReal &HOld, const Array2DReal &HNew,
                                const Array2DReal &U, const Array3DReal &Tracers, int NTracers, Real Dt, hipStream_t S) const {
   OMEGA_REQUIRE(NTracers >= 1 && NTracers <= MaxTracers,
                 "MonotoneAdv: NTracers = " + std::to_string(NTracers) + " is outside 1 .. MaxTracers = " +
                     std::to_string(MaxTracers));
   OMEGA_REQUIRE(std::isfinite(Dt) && Dt > 0.0, "MonotoneAdv: Dt = " + std::to_string(Dt) + " is not finite and positive");
   requirePlanes(Tend, NTracers, Mesh->NCellsSize, NVertLayers, "the tracer tendency");
   requirePlanes(Tracers, NTracers, Mesh->NCellsSize, NVertLayers, "Tracers");
   requireLevelArray("MonotoneAdv", HOld, Mesh->NCellsSize, NVertLayers, "the old LayerThickness");
   requireLevelArray("MonotoneAdv", HNew, Mesh->NCellsSize, NVertLayers, "the new LayerThickness");
   requireLevelArray("MonotoneAdv", U, Mesh->NEdgesSize, NVertLayers, "NormalVelocity");
   Pacer::Range Timer("MonotoneAdv:addTracerTend", 1);
   MonotoneAdvArgs A;
   A.K = NVertLayers, A.NTracers = NTracers, A.FluxThicknessUpwind = Config.FluxThicknessUpwind ? 1 : 0, A.Dt = Dt;
   A.HOld = HOld.Ptr, A.HNew = HNew.Ptr, A.NormalVelocity = U.Ptr, A.Tracers = Tracers.Ptr;
   A.ScaleIn = ScaleIn.Ptr, A.ScaleOut = ScaleOut.Ptr, A.Tend = Tend.Ptr;
   if (VAdv) { // the 3-D form
      A.VerticalTransport = VAdv->VerticalTransport.Ptr;
      A.MinLayerCell = VAdv->VCoord->MinLayerCell.Ptr, A.MaxLayerCell = VAdv->VCoord->MaxLayerCell.Ptr;
   }
   launchMonotoneAdv(Mesh->view(), A, S);
}

void MonotoneAdv::copyToHost() {
   HIP_CHECK(hipDeviceSynchronize());
   OMEGA::copyToHost(ScaleInH.data(), ScaleIn);
   OMEGA::copyToHost(ScaleOutH.data(), ScaleOut);
}

} // namespace OMEGA
