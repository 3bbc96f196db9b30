// Redi.h -- isoneutral (Redi 1982) diffusion of the tracers, the partner of GentMcWilliams: the tracer flux K grad(phi)
// with the small-slope tensor K = Kappa [[1, S], [S^T, S.S]] of the isopycnal slope S relative to the layers.  The two
// off-diagonal parts are explicit -- a horizontal edge flux that carries the vertical tracer gradient, and a vertical
// cross flux through the layer interfaces that carries the horizontal one -- and the S.S part is a vertical diffusivity
// that goes into VertMix's implicit tracer solve (VertMixStep::attachRedi).  The slope is the quotient of the two
// quantities GentMcWilliams already forms on the edge interfaces: the density gradient at constant z and N^2.  The
// reference has no code for it: the contract below is this library's.  DESIGN.md section 4.14.
//
// Numerical contract (FP64, -ffp-contract=off, IEEE divisions, every chain in the order written; a NumPy restatement in
// the same order is bit-identical, tests/redi_reference.py).  g = VertCoord::Gravity, Rho0 the VertCoord's, GR = g / Rho0.
//
// 1. computeSlope(h, [SpecVol, SpecVolDisplaced, ZMid,] S), one launch.  For every edge e < NEdgesAll with Lo =
//    MinLayerEdgeBot[e], Hi = MaxLayerEdgeTop[e], c0, c1 = CellsOnEdge[e][0], [1]; an edge whose range is not
//    0 <= Lo <= Hi < NVertLayers is left alone entirely:
//      InvDc = 1.0 / DcEdge[e]
//    layers K = Lo .. Hi, the expressions of GentMcWilliams.h:
//      Rho_c[K]   = 1.0 / SpecVol[c][K]                                   (c = c0, c1)
//      GradRho[K] = (Rho_c1[K] - Rho_c0[K]) * InvDc
//      GradZ[K]   = (ZMid[c1][K] - ZMid[c0][K]) * InvDc
//    interfaces K = Lo+1 .. Hi, again as GentMcWilliams.h has them:
//      per cell:  Dz_c   = ZMid[c][K-1] - ZMid[c][K]
//                 RhoZ_c = (Rho_c[K-1] - Rho_c[K]) / Dz_c
//                 N2_c   = (GR * (Rho_c[K] - (1.0 / SpecVolDisplaced[c][K-1]))) / Dz_c
//      RhoZE = 0.5 * (RhoZ_c0 + RhoZ_c1);  N2E = 0.5 * (N2_c0 + N2_c1);  N2E = N2E < 0.0 ? 0.0 : N2E
//      GradRhoZ = 0.5 * (GradRho[K-1] + GradRho[K]) - RhoZE * (0.5 * (GradZ[K-1] + GradZ[K]))
//    and then
//      Den  = N2E < N2Floor ? N2Floor : N2E
//      SIso = (GR * GradRhoZ) / Den                                       (the slope of the isopycnal surface)
//      SRel = SIso - 0.5 * (GradZ[K-1] + GradZ[K])                        (... relative to the layer)
//      SRel = SRel >  SlopeMax ?  SlopeMax : SRel
//      SRel = SRel < -SlopeMax ? -SlopeMax : SRel
//      SlopeInterface[e][K] = SRel
//    SlopeInterface[e][Lo] = 0.0
//  - Row K of SlopeInterface is the interface at the top of layer K.  Nothing else is written: the levels outside
//    Lo .. Hi, rows >= NEdgesAll, the sentinel row and the pitch padding stay as they were.  The slopes of the surface
//    and of the bottom are 0 by construction: no flux passes through either.
//  - The thickness does not enter the slope (hE of GentMcWilliams.h weighs the fluxes of 2. only): h is checked for its
//    shape like the other arrays and not read.
//
// 2. addTracerTend(Tend, h, Tracers, NTracers, [ZMid,] S), one launch.  For every cell c < NCellsAll, every layer K in
//    MinLayerCell[c] .. MaxLayerCell[c] (a cell whose range is not 0 <= KMin <= KMax < NVertLayers is left alone) and
//    every tracer L < NTracers, with phi = Tracers[L], InvAreaCell = 1.0 / AreaCell[c], Acc = WTop = WBot = 0.0:
//    slots J = 0 .. NEdgesOnCell[c]-1 in slot order, e = EdgesOnCell[c][J], c0, c1 = CellsOnEdge[e], Lo, Hi the edge's
//    range; a slot whose edge is not in 0 .. NEdgesAll-1, whose edge range is invalid or does not hold K contributes
//    nothing and reads nothing:
//      InvDc = 1.0 / DcEdge[e]
//      hE[K]      = 0.5 * (h[c0][K] + h[c1][K])
//      GradPhi[k] = (phi[c1][k] - phi[c0][k]) * InvDc                     (k = K-1, K, K+1 as needed, inside Lo .. Hi)
//      PhiZ_c[k]  = (phi[c][k-1] - phi[c][k]) / (ZMid[c][k-1] - ZMid[c][k])   (c = c0, c1; k = K, K+1 inside Lo+1 .. Hi)
//      PhiZE[k]   = 0.5 * (PhiZ_c0[k] + PhiZ_c1[k])
//      GInt[k]    = 0.5 * (GradPhi[k-1] + GradPhi[k])
//      Up = K > Lo ? SlopeInterface[e][K]   * PhiZE[K]   : 0.0
//      Dn = K < Hi ? SlopeInterface[e][K+1] * PhiZE[K+1] : 0.0
//      FluxE = (Kappa[e] * hE[K]) * (GradPhi[K] + 0.5 * (Up + Dn))
//      Acc   = Acc - EdgeSignOnCell[c][J] * (DvEdge[e] * FluxE)           (the sign convention of TracerDiffOnCell)
//      F_J = ((0.5 * DcEdge[e]) * DvEdge[e]) * InvAreaCell                (VertMix's edge-to-cell weight)
//      if K > Lo:  WTop = WTop + F_J * ((Kappa[e] * SlopeInterface[e][K])   * GInt[K])
//      if K < Hi:  WBot = WBot + F_J * ((Kappa[e] * SlopeInterface[e][K+1]) * GInt[K+1])
//    then  Tend[L][c][K] = Tend[L][c][K] + (Acc * InvAreaCell + (WTop - WBot))
//  - The two cells of an edge form FluxE from the same operands in the same order, and the layer below forms its WTop as
//    the layer above forms its WBot: the column integral telescopes and the domain integral cancels edge by edge.
//  - The inputs are not written; nothing of Tend but the entries named is.  Values outside a cell's layer range never
//    reach an output (every read above is inside both cells' ranges; the terms are selected, never multiplied by 0):
//    NaN there is legal input.
//
// 3. computeVertDiffusivity(VertDiff, S), one launch.  For every cell c < NCellsAll and interface K = MinLayerCell[c]+1
//    .. MaxLayerCell[c], D = 0.0, and in slot order over the slots whose edge is valid with Lo+1 <= K <= Hi:
//      D = D + F_J * (Kappa[e] * (SlopeInterface[e][K] * SlopeInterface[e][K]))
//    then VertDiffusivity[c][K] = D, and if VertDiff is given VertDiff[c][K] = VertDiff[c][K] + D (as GentMcWilliams
//    treats its Transport).  Every other entry is left alone.
//
// Deviations from other formulations:
//  - The layer thickness h stands for the metric dz (in hE and, through VertMix, in the implicit S.S term), as in
//    VertMix and GentMcWilliams.
//  - The vertical density derivative of the z-correction (RhoZ) is in-situ; only N^2 is locally referenced, as in
//    GentMcWilliams.
//  - The slope is clipped at SlopeMax; there is no Gerdes or Danabasoglu taper.
//  - The edge-normal weights F_J stand for the dot product of the horizontal vectors (S.S, S.grad phi): exact on a
//    planar Voronoi mesh, where sum_e F_e n n^T = I, an approximation on the sphere and at coasts.
//
// Algorithmic traffic: slope 24 B per cell-level (three cell arrays, each row ideally fetched once) + 8 B per edge-level
// written; tendency per tracer 8 B (phi) + 16 B (Tend read and written) per cell-level, plus once 16 B (h, ZMid) per
// cell-level and 8 B per edge-level (the slope); diffusivity 8 B per edge-level + 8 B per cell-level (24 B with VertDiff).
#ifndef OMEGA_AMD_REDI_H
#define OMEGA_AMD_REDI_H

#include "ColumnPass.h"

namespace OMEGA {

class Redi : public Registry<Redi>, public ColumnPass {
 public:
   /// Refuses (OmegaError) a null or host-only mesh; a VertCoord or Eos that is null, was built for another mesh or has
   /// another layer count; NVertLayers outside 1 .. TriDiagMaxRows; a RediKappa that is negative or not finite; a
   /// SlopeMax or N2Floor that is not finite or <= 0; MaxTracers < 1.  Everything is allocated here; no call allocates.
   Redi(const std::string &Name, const HorzMesh *Mesh, VertCoord *VCoord, Eos *EqState, int MaxTracers,
        Real RediKappa = 600.0, Real SlopeMax = 0.01, Real N2Floor = 1.0e-10);

   I4 MaxTracers;
   Real RediKappa, SlopeMax, N2Floor;
   /// [NEdgesSize], RediKappa at construction; the caller may overwrite it
   Array1DReal Kappa;
   /// [NEdgesSize][levelPitch(K)], zero at construction; row K: the interface at the top of layer K
   Array2DReal SlopeInterface;
   /// [NCellsSize][levelPitch(K)], zero at construction; the same row convention
   Array2DReal VertDiffusivity;
   mutable I8 LaunchCount = 0; ///< kernel launches issued by the three compute calls so far

   /// GentMcWilliams::updateColumn's pass (Displaced = true, KDisp = 1, temperature 0, salinity 1) with this object's
   /// forcing (ColumnPass.h)
   void updateColumn(const Array2DReal &LayerThickness, const Array3DReal &TracerArray, hipStream_t S) const {
      ColumnPass::updateColumn(LayerThickness, TracerArray, true, S);
   }
   /// 1. of the contract, the array form: the cell arrays [NCellsSize][levelPitch(K)]
   void computeSlope(const Array2DReal &LayerThickness, const Array2DReal &SpecVol, const Array2DReal &SpecVolDisplaced,
                     const Array2DReal &ZMid, hipStream_t S) const;
   /// the same on the attached Eos's SpecVol / SpecVolDisplaced and the VertCoord's ZMid as they stand
   void computeSlope(const Array2DReal &LayerThickness, hipStream_t S) const;
   /// 2. of the contract: Tend and Tracers [>= NTracers][NCellsSize][levelPitch(K)], on the SlopeInterface last computed.
   /// Refuses NTracers outside 1 .. MaxTracers and arrays of another shape.
   void addTracerTend(const Array3DReal &Tend, const Array2DReal &LayerThickness, const Array3DReal &Tracers,
                      int NTracers, const Array2DReal &ZMid, hipStream_t S) const;
   /// the same on the VertCoord's ZMid as it stands
   void addTracerTend(const Array3DReal &Tend, const Array2DReal &LayerThickness, const Array3DReal &Tracers,
                      int NTracers, hipStream_t S) const;
   /// 3. of the contract: VertDiff [NCellsSize][levelPitch(K)] accumulated in place, or empty (no term)
   void computeVertDiffusivity(const Array2DReal &VertDiff, hipStream_t S) const;

   // ---- the reference's style of signature: on this object's `Stream` (default: the null stream)
   hipStream_t Stream = nullptr;
   void updateColumn(const Array2DReal &LayerThickness, const Array3DReal &TracerArray) const {
      updateColumn(LayerThickness, TracerArray, Stream);
   }
   void computeSlope(const Array2DReal &LayerThickness, const Array2DReal &SpecVol, const Array2DReal &SpecVolDisplaced,
                     const Array2DReal &ZMid) const {
      computeSlope(LayerThickness, SpecVol, SpecVolDisplaced, ZMid, Stream);
   }
   void computeSlope(const Array2DReal &LayerThickness) const { computeSlope(LayerThickness, Stream); }
   void addTracerTend(const Array3DReal &Tend, const Array2DReal &LayerThickness, const Array3DReal &Tracers,
                      int NTracers, const Array2DReal &ZMid) const {
      addTracerTend(Tend, LayerThickness, Tracers, NTracers, ZMid, Stream);
   }
   void addTracerTend(const Array3DReal &Tend, const Array2DReal &LayerThickness, const Array3DReal &Tracers,
                      int NTracers) const {
      addTracerTend(Tend, LayerThickness, Tracers, NTracers, Stream);
   }
   void computeVertDiffusivity(const Array2DReal &VertDiff) const { computeVertDiffusivity(VertDiff, Stream); }

   std::string Name;
};

} // namespace OMEGA
#endif
