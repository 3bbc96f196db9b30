// PressureGrad.h -- the pressure-gradient force of a layered (stratified) ocean on the edges: -(grad Phi) - alpha grad p
// along the layers, from the column fields of VertCoord (PressureMid, GeopotentialMid) and Eos (SpecVol).  It is what
// replaces Omega-0's SSHGradOnEdge (stacked shallow water, g grad(h - BottomDepth)) once the layers have their own
// density.  The reference names the term in its governing-equation document (components/omega/doc/design/
// OmegaV1GoverningEqns.md, discrete momentum equation) and has no code for it; its own pressure-gradient design
// document is still "forthcoming".
//
// Numerical contract (FP64, -ffp-contract=off, IEEE divisions; a NumPy restatement in the same order is bit-identical,
// tests/pressure_grad_reference.py).  For every edge e < NEdgesAll and level K in MinLayerEdgeBot[e] ..
// MaxLayerEdgeTop[e] of the VertCoord (an empty range leaves the edge alone), with c0, c1 = CellsOnEdge[e][0], [1]:
//      InvDc   = 1.0 / DcEdge[e]
//      GradGeo = (GeopotentialMid[c1][K] - GeopotentialMid[c0][K]) * InvDc
//      GradP   = (PressureMid[c1][K]     - PressureMid[c0][K])     * InvDc
//      AlphaE  = 0.5 * (SpecVol[c0][K] + SpecVol[c1][K])
//      Tend[e][K] = Tend[e][K] - EdgeMask[e] * (GradGeo + AlphaE * GradP)
//  - PressureMid is in Pa, as VertCoord produces it (SpecVol in m^3 kg^-1, GeopotentialMid in m^2 s^-2).
//  - Nothing else is written: levels outside the range, rows >= NEdgesAll, the sentinel row and the pitch padding
//    stay as they were.  The range MinLayerEdgeBot .. MaxLayerEdgeTop is the levels active in BOTH cells; an edge with
//    a land or missing neighbour has an empty range.
//  - Halo edges are swept like owned ones, as SSHGradOnEdge does.
//  - This is the centred form of -grad Phi - alpha grad p: the continuous limit of the three-term flux form of the
//    reference's discrete momentum equation, not that flux form itself.
//  - g enters through GeopotentialMid only and is VertCoord::Gravity (9.80616), NOT the 9.80665 of the tendencies'
//    SSHGradOnEdge.
//
// Algorithmic traffic: 24 B per cell-level (three cell arrays, each row ideally fetched once) + 16 B per edge-level
// (the tendency read and written), ~ 72 B per cell-level on a hexagon mesh (3 edges per cell).
#ifndef OMEGA_AMD_PRESSUREGRAD_H
#define OMEGA_AMD_PRESSUREGRAD_H

#include "ColumnPass.h"

namespace OMEGA {

class PressureGrad : public Registry<PressureGrad>, public ColumnPass {
 public:
   /// Refuses (OmegaError) a null or host-only mesh, and a VertCoord or Eos that is null, was built for another mesh or
   /// has another layer count.  Everything is allocated here; no call allocates.
   PressureGrad(const std::string &Name, const HorzMesh *Mesh, VertCoord *VCoord, Eos *EqState);

   /// The array form of the contract: Tend [NEdgesSize][levelPitch(K)] accumulated in place, the three cell arrays
   /// [NCellsSize][levelPitch(K)]
   void computePressureGrad(const Array2DReal &Tend, const Array2DReal &PressureMid, const Array2DReal &GeopotentialMid,
                            const Array2DReal &SpecVol, hipStream_t S) const;
   /// the same on the attached VertCoord's PressureMid / GeopotentialMid and the Eos's SpecVol as they stand
   void computePressureGrad(const Array2DReal &Tend, hipStream_t S) const;
   /// The fused column pass (VertCoord::computeColumn) from raw arrays: thickness [NCellsSize][levelPitch(K)], tracers
   /// [>= 2][NCellsSize][levelPitch(K)] with TIndex = 0, SIndex = 1, Displaced = false, and this object's
   /// SurfacePressure / TidalPotential / SelfAttractionLoading (ColumnPass.h).
   void updateColumn(const Array2DReal &LayerThickness, const Array3DReal &TracerArray, hipStream_t S) const {
      ColumnPass::updateColumn(LayerThickness, TracerArray, false, S);
   }

   // ---- the reference's style of signature: on this object's `Stream` (default: the null stream)
   hipStream_t Stream = nullptr;
   void computePressureGrad(const Array2DReal &Tend, const Array2DReal &PressureMid, const Array2DReal &GeopotentialMid,
                            const Array2DReal &SpecVol) const {
      computePressureGrad(Tend, PressureMid, GeopotentialMid, SpecVol, Stream);
   }
   void computePressureGrad(const Array2DReal &Tend) const { computePressureGrad(Tend, Stream); }
   void updateColumn(const Array2DReal &LayerThickness, const Array3DReal &TracerArray) const {
      updateColumn(LayerThickness, TracerArray, Stream);
   }

   std::string Name;
};

} // namespace OMEGA
#endif
