// VertCoord.h -- vertical coordinate: layer ranges, hydrostatic pressure, geometric height, geopotential and target
// thickness of every column.  Interface and array names after the reference (components/omega/src/ocn/VertCoord.h:
// 28-209; VertCoord.cpp:484-864).  Reading the configuration and the IO streams (the reference's init / completeSetup)
// is out of scope: the caller passes the options and the layer ranges.
//
// Numerical contract (FP64, -ffp-contract=off: a NumPy restatement in the same order is bit-identical,
// tests/column_reference.py).  g = 9.80616 (VertCoord's own gravity, VertCoord.cpp; NOT the 9.80665 of the
// tendencies), Rho0 = Density0 (default 1026).
//  - Layer ranges: MinLayerCell / MaxLayerCell are 0-based, sized NCellsSize, from the global 1-based
//    minLevelCell / maxLevelCell of a mesh file gathered through the Decomp (absent: 0 and NVertLayers-1); the
//    sentinel cell is -1 / -1.  Edges (2 cells) and vertices (VertexDegree cells), a cell with MaxLayerCell == -1
//    being land, top(c) = land ? NVertLayers+1 : Min(c), bot(c) = land ? 0 : Min(c):
//    MinLayer*Top = min(top), MinLayer*Bot = max(bot), MaxLayer*Top = min(Max), MaxLayer*Bot = max(Max); the
//    sentinel row is NVertLayers+1, NVertLayers+1, -1, -1.
//  - computePressure(h, Ps), cells 0 .. NCellsAll-1, sequential top-down over K = KMin .. KMax:
//      inc = (g*Rho0)*h[K]; acc += inc; PInt[K+1] = Ps + acc; PMid[K] = (Ps + acc) - 0.5*inc;  PInt[KMin] = Ps.
//  - computeZHeight(h, SpecVol), sequential bottom-up over K = KMax .. KMin:
//      dz = (Rho0*SpecVol[K])*h[K]; acc += dz; ZInt[K] = -Bot + acc; ZMid[K] = (-Bot + acc) - 0.5*dz;
//      ZInt[KMax+1] = -Bot.   (Bot = BottomDepth: the mesh's, overwritable.)
//  - computeGeopotential(Tidal, SAL): GeoMid[K] = ((g*ZMid[K]) + Tidal) + SAL on the active layers.
//  - computeTargetThickness(): ascending sequential sums over KMin .. KMax of W[K]*Ref[K] (SumWh) and of Ref[K]
//    (SumRef); Coeff = (PInt[KMax+1] - PInt[KMin])/(g*Rho0) - SumRef; Target[K] = Ref[K]*(1 + (Coeff*W[K])/SumWh).
//    W = VertCoordMovementWeights: 1 everywhere for "Uniform", 1 at level 0 and 0 elsewhere for "Fixed".
//  Entries outside a column's active range are not written, and a column whose range is not
//  0 <= KMin <= KMax < NVertLayers (land) is not touched at all.
//
// computeColumn is the per-step hot path: ONE launch whose result equals the sequence computePressure ->
// Eos::computeSpecVol(T, S, PMid*1.0e-4) -> computeZHeight -> computeGeopotential, bit for bit (the single-stage
// launches and the fused launch are instantiations of the same kernel code).  The equation of state takes pressure in
// dbar, VertCoord produces Pa: the factor 1.0e-4 (Pa -> dbar) is this library's convention -- the reference has no
// call site joining the two objects yet.  On inactive layers SpecVol is evaluated from whatever PressureMid holds
// there, as the sequence would.  Algorithmic traffic per cell-level: 72 B fused (reads h, T, S; writes PInt, PMid,
// SpecVol, ZInt, ZMid, GeoMid) against 104 B for the four launches.
#ifndef OMEGA_AMD_VERTCOORD_H
#define OMEGA_AMD_VERTCOORD_H

#include "Base.h"
#include "Decomp.h"
#include "Eos.h"
#include "HorzMesh.h"
#include "OceanState.h"

namespace OMEGA {

class VertCoord : public Registry<VertCoord> {
 public:
   /// MinLevelCellGlobal / MaxLevelCellGlobal: [NCellsGlobal] 1-based, as a mesh file holds them (nullable: every
   /// layer active); MeshDecomp is needed only to gather them.  MovementWeightType: "Uniform" or "Fixed".
   VertCoord(const std::string &Name, const HorzMesh *Mesh, const Decomp *MeshDecomp, int NVertLayers,
             Real Rho0 = 1026.0, const std::string &MovementWeightType = "Uniform",
             const I4 *MinLevelCellGlobal = nullptr, const I4 *MaxLevelCellGlobal = nullptr);

   static constexpr Real Gravity = 9.80616; ///< VertCoord.cpp: computePressure / computeGeopotential / ...

   I4 NVertLayers, NVertLayersP1;
   Real Rho0;
   std::string MovementWeightType;

   Array2DReal PressureInterface, PressureMid, ZInterface, ZMid, GeopotentialMid, LayerThicknessTarget;
   HostArrayReal PressureInterfaceH, PressureMidH, ZInterfaceH, ZMidH, GeopotentialMidH, LayerThicknessTargetH;

   Array1DI4 MinLayerCell, MaxLayerCell, MinLayerEdgeTop, MaxLayerEdgeTop, MinLayerEdgeBot, MaxLayerEdgeBot,
       MinLayerVertexTop, MaxLayerVertexTop, MinLayerVertexBot, MaxLayerVertexBot;
   HostArrayI4 MinLayerCellH, MaxLayerCellH, MinLayerEdgeTopH, MaxLayerEdgeTopH, MinLayerEdgeBotH, MaxLayerEdgeBotH,
       MinLayerVertexTopH, MaxLayerVertexTopH, MinLayerVertexBotH, MaxLayerVertexBotH;

   Array1DReal VertCoordMovementWeights; ///< [NVertLayers]
   Array2DReal RefLayerThickness;        ///< [NCellsSize][NVertLayers]
   HostArrayReal VertCoordMovementWeightsH, RefLayerThicknessH;

   Array1DReal BottomDepth; ///< [NCellsSize], the mesh's at construction
   HostArrayReal BottomDepthH;

   /// VertCoord::minMaxLayerEdge / minMaxLayerVertex (VertCoord.cpp:484-610), from the current Min/MaxLayerCell;
   /// the host mirrors are refreshed
   void minMaxLayerEdge(hipStream_t S);
   void minMaxLayerVertex(hipStream_t S);
   /// VertCoord::computePressure (VertCoord.cpp:654-696)
   void computePressure(const Array2DReal &LayerThickness, const Array1DReal &SurfacePressure, hipStream_t S);
   /// VertCoord::computeZHeight (VertCoord.cpp:700-739)
   void computeZHeight(const Array2DReal &LayerThickness, const Array2DReal &SpecVol, hipStream_t S);
   /// VertCoord::computeGeopotential (VertCoord.cpp:743-781)
   void computeGeopotential(const Array1DReal &TidalPotential, const Array1DReal &SelfAttractionLoading, hipStream_t S);
   /// VertCoord::computeTargetThickness (VertCoord.cpp:785-838)
   void computeTargetThickness(hipStream_t S);
   /// The fused column pass (see the contract above): thickness of State at ThickLevel, T and S = tracers TIndex and
   /// SIndex of Tracers at TrLevel (TracerDefs.inc: Temperature 0, Salinity 1); SpecVolDisplaced too when Displaced.
   void computeColumn(const OceanState *State, int ThickLevel, const TracerStore *Tracers, int TrLevel, const Eos &EqState,
                      const Array1DReal &SurfacePressure, const Array1DReal &TidalPotential,
                      const Array1DReal &SelfAttractionLoading, bool Displaced, I4 KDisp, hipStream_t S, I4 TIndex = 0,
                      I4 SIndex = 1);
   /// the same pass from raw arrays: LayerThickness [NCellsSize][levelPitch(K)], TracerArray
   /// [NTracers][NCellsSize][levelPitch(K)] (what the overload above forwards to; same kernel, same results)
   void computeColumn(const Array2DReal &LayerThickness, const Array3DReal &TracerArray, const Eos &EqState,
                      const Array1DReal &SurfacePressure, const Array1DReal &TidalPotential,
                      const Array1DReal &SelfAttractionLoading, bool Displaced, I4 KDisp, hipStream_t S, I4 TIndex = 0,
                      I4 SIndex = 1);

   // ---- the reference's signatures (VertCoord.h:180-206): on this object's `Stream` (default: the null stream)
   hipStream_t Stream = nullptr;
   void minMaxLayerEdge() { minMaxLayerEdge(Stream); }
   void minMaxLayerVertex() { minMaxLayerVertex(Stream); }
   void computePressure(const Array2DReal &LayerThickness, const Array1DReal &SurfacePressure) {
      computePressure(LayerThickness, SurfacePressure, Stream);
   }
   void computeZHeight(const Array2DReal &LayerThickness, const Array2DReal &SpecVol) {
      computeZHeight(LayerThickness, SpecVol, Stream);
   }
   void computeGeopotential(const Array1DReal &TidalPotential, const Array1DReal &SelfAttractionLoading) {
      computeGeopotential(TidalPotential, SelfAttractionLoading, Stream);
   }
   void computeTargetThickness() { computeTargetThickness(Stream); }

   void copyToHost();   ///< VertCoord.cpp:842-851: the seven real arrays -> their host mirrors
   void copyToDevice(); ///< VertCoord.cpp:855-864: the host mirrors -> the seven real arrays

   const HorzMesh *Mesh;
   std::string Name;

 private:
   ColumnArgs baseArgs() const;
};

} // namespace OMEGA
#endif
