// ColumnPass.h -- what the classes that run the fused column pass (VertCoord::computeColumn) on a VertCoord and an Eos
// of their mesh share: PressureGrad, GentMcWilliams and Redi (as a public base: P->Mesh, P->SurfacePressure and so on
// are the class's own members) and VertMixStep (the same, with its own checks).  The attached objects, the layer
// count, the per-cell forcing of the pass, the refusals of objects that do not fit together, and the pass itself.
// Every object has its own forcing arrays; keeping those of two objects on one VertCoord equal is the caller's.
#ifndef OMEGA_AMD_COLUMNPASS_H
#define OMEGA_AMD_COLUMNPASS_H

#include "Base.h"
#include "Eos.h"
#include "HorzMesh.h"
#include "VertCoord.h"
#include "kernels/PackedColumns.h"

namespace OMEGA {

struct ColumnPass {
   ColumnPass(const HorzMesh *Mesh_, VertCoord *VCoord_, Eos *EqState_) : Mesh(Mesh_), VCoord(VCoord_), EqState(EqState_) {}

   const HorzMesh *Mesh;
   VertCoord *VCoord;
   Eos *EqState;
   I4 NVertLayers = 0;
   /// The column pass's per-cell forcing, [NCellsSize], zero at construction; the caller may overwrite them
   Array1DReal SurfacePressure, TidalPotential, SelfAttractionLoading;

   /// Refuses (OmegaError, under the name Class) a host-only mesh and a VertCoord or Eos that is null, was built for
   /// another mesh or has another layer count; then takes the layer count.  The mesh is not null: the classes refuse
   /// that first, then their own parameters, then call this.
   void requireFits(const std::string &Class) {
      OMEGA_REQUIRE(!Mesh->HostOnly,
                    Class + ": the mesh was created host-only: no device arrays, compute is unavailable");
      OMEGA_REQUIRE(VCoord != nullptr, Class + ": VertCoord is NULL");
      OMEGA_REQUIRE(EqState != nullptr, Class + ": Eos is NULL");
      OMEGA_REQUIRE(VCoord->Mesh == Mesh, Class + ": the VertCoord was built for another mesh");
      OMEGA_REQUIRE(EqState->Mesh == Mesh, Class + ": the Eos was built for another mesh");
      OMEGA_REQUIRE(EqState->NVertLayers == VCoord->NVertLayers,
                    Class + ": the VertCoord and the Eos have different layer counts");
      NVertLayers = VCoord->NVertLayers;
   }
   void allocateForcing() {
      SurfacePressure       = Array1DReal("SurfacePressure", Mesh->NCellsSize);
      TidalPotential        = Array1DReal("TidalPotential", Mesh->NCellsSize);
      SelfAttractionLoading = Array1DReal("SelfAttractionLoading", Mesh->NCellsSize);
   }

   /// The fused column pass from raw arrays: thickness [NCellsSize][levelPitch(K)], tracers [>= 2][NCellsSize]
   /// [levelPitch(K)] with temperature at index 0 and salinity at 1, this object's forcing; Displaced: with the
   /// displaced volume of the layer above (KDisp = 1).
   void updateColumn(const Array2DReal &LayerThickness, const Array3DReal &TracerArray, bool Displaced,
                     hipStream_t S) const {
      VCoord->computeColumn(LayerThickness, TracerArray, *EqState, SurfacePressure, TidalPotential,
                            SelfAttractionLoading, Displaced, Displaced ? 1 : 0, S, 0, 1);
   }

   /// The edge columns of a launch on the stratification (SpecVol, SpecVolDisplaced, ZMid) of the two cells of an edge:
   /// refuses, under the name Class, a cell array that is not [NCellsSize][levelPitch(K)] -- the thickness first, as
   /// the callers list it -- and fills the fields of A.
   void stratificationArgs(const char *Class, EdgeColumnArgs &A, const Array2DReal &LayerThickness,
                           const Array2DReal &SpecVol, const Array2DReal &SpecVolDisplaced,
                           const Array2DReal &ZMid) const {
      requireLevelArray(Class, LayerThickness, Mesh->NCellsSize, NVertLayers, "LayerThickness");
      requireLevelArray(Class, SpecVol, Mesh->NCellsSize, NVertLayers, "SpecVol");
      requireLevelArray(Class, SpecVolDisplaced, Mesh->NCellsSize, NVertLayers, "SpecVolDisplaced");
      requireLevelArray(Class, ZMid, Mesh->NCellsSize, NVertLayers, "ZMid");
      A.NEdgesAll = Mesh->NEdgesAll, A.NCellsSize = Mesh->NCellsSize, A.K = NVertLayers;
      A.CellsOnEdge     = Mesh->CellsOnEdge.Ptr;
      A.MinLayerEdgeBot = VCoord->MinLayerEdgeBot.Ptr, A.MaxLayerEdgeTop = VCoord->MaxLayerEdgeTop.Ptr;
      A.DcEdge    = Mesh->DcEdge.Ptr;
      A.GOverRho0 = VertCoord::Gravity / VCoord->Rho0;
      A.SpecVol = SpecVol.Ptr, A.SpecVolDisplaced = SpecVolDisplaced.Ptr, A.ZMid = ZMid.Ptr;
   }
};

} // namespace OMEGA
#endif
