// GentMcWilliams.h -- the eddy-induced (bolus) velocity of the Gent-McWilliams closure on the edges, in the
// boundary-value form of Ferrari et al. (2010, Ocean Modelling 32) that MPAS-Ocean uses: the eddy stream function Psi
// of an edge column solves  c^2 Psi'' - N^2 Psi = -kappa (g / Rho0) grad_z rho  with Psi = 0 at the surface and at the
// bottom, and u* = -dPsi/dz.  One small symmetric positive-definite tridiagonal system per edge column; no slope
// tapering, and well posed in unstratified and unstable water (N^2 is clipped at 0, c^2 > 0 keeps the system definite).
// The reference has no code for it: the contract below is this library's.  DESIGN.md section 4.13.
//
// Numerical contract (FP64, -ffp-contract=off, IEEE divisions, every chain in the order written; a NumPy restatement in
// the same order is bit-identical, tests/gent_mcwilliams_reference.py).  g = VertCoord::Gravity, Rho0 the VertCoord's.
// For every edge e < NEdgesAll (halo edges are swept like owned ones, as PressureGrad does) with Lo = MinLayerEdgeBot[e],
// Hi = MaxLayerEdgeTop[e], c0, c1 = CellsOnEdge[e][0], [1]; an edge whose range is not 0 <= Lo <= Hi < NVertLayers is
// left alone entirely, and so is one with a cell outside [0, NCellsSize), as in Redi.h and the edge tiles of the other
// vertical kernels -- no mesh this library builds has one (Decomp maps every missing cell to the sentinel row):
//      InvDc = 1.0 / DcEdge[e];  C2 = GravWaveSpeed * GravWaveSpeed;  GR = g / Rho0
//    layers K = Lo .. Hi:
//      Rho_c[K]   = 1.0 / SpecVol[c][K]                                   (c = c0, c1)
//      hE[K]      = 0.5 * (h[c0][K] + h[c1][K])
//      GradRho[K] = (Rho_c1[K] - Rho_c0[K]) * InvDc
//      GradZ[K]   = (ZMid[c1][K] - ZMid[c0][K]) * InvDc
//    interfaces K = Lo+1 .. Hi, row i = K - Lo - 1 of n = Hi - Lo rows:
//      per cell:  Dz_c   = ZMid[c][K-1] - ZMid[c][K]
//                 RhoZ_c = (Rho_c[K-1] - Rho_c[K]) / Dz_c
//                 N2_c   = (GR * (Rho_c[K] - (1.0 / SpecVolDisplaced[c][K-1]))) / Dz_c   (VertMix.h's N2, same association)
//      RhoZE = 0.5 * (RhoZ_c0 + RhoZ_c1);  N2E = 0.5 * (N2_c0 + N2_c1);  N2E = N2E < 0.0 ? 0.0 : N2E
//      GradRhoZ = 0.5 * (GradRho[K-1] + GradRho[K]) - RhoZE * (0.5 * (GradZ[K-1] + GradZ[K]))
//                                                                 (the density gradient at constant z)
//      DzMid = 0.5 * (hE[K-1] + hE[K])
//      G_i = C2 / hE[K] for i < n-1;  G_{n-1} = 0
//      H_i = N2E * DzMid;  if i == 0: H_i = H_i + C2 / hE[Lo];  if i == n-1: H_i = H_i + C2 / hE[Hi]
//                                                                 (n == 1: both, in this order)
//      X_i = DzMid * ((Kappa[e] * GR) * GradRhoZ)
//      StreamFunction[e][K] = the PCRDiffusionSolver arithmetic on (G, H, X) (TriDiagSolvers.h; n == 1: the 1x1 solve)
//    StreamFunction[e][Lo] = 0.0
//    layers K = Lo .. Hi:  Top = (K == Lo) ? 0.0 : Psi[K];  Bot = (K == Hi) ? 0.0 : Psi[K+1]
//      BolusVelocity[e][K] = (Bot - Top) / hE[K]
//      if Transport is given:  Transport[e][K] = Transport[e][K] + BolusVelocity[e][K]
//  - The system is the equation above multiplied through by DzMid, which gives the symmetric diffusion form the solver
//    expects: -G_{i-1} Psi_{i-1} + (H_i + G_{i-1} + G_i) Psi_i - G_i Psi_{i+1} = X_i.  The Dirichlet ends are folded into
//    H: H_i >= 0 (0 on an interior row of unstratified water) and the diagonal H_i + G_{i-1} + G_i > 0 always.  Away
//    from the boundaries Psi tends to kappa times the isopycnal slope.
//  - Row K of StreamFunction is the interface at the top of layer K.
//  - Nothing else is written: the levels of BolusVelocity / StreamFunction / Transport outside Lo .. Hi, rows >=
//    NEdgesAll, the sentinel row and the pitch padding stay as they were.  Lo == Hi writes StreamFunction[e][Lo] = 0,
//    BolusVelocity[e][Lo] = 0 / hE and adds that to Transport.
//  - The bolus transport of a column telescopes: sum_K hE[K] * BolusVelocity[e][K] = 0 up to rounding.
//
// Deviations from the continuous closure:
//  - The layer thickness h stands for the metric dz (in the second difference and in u* = -dPsi/dz), as in VertMix.
//  - The vertical density derivative of the z-correction (RhoZ) is in-situ; only N^2 is locally referenced (the
//    displaced volume of the layer above).
//  - Redi (isopycnal) diffusion of the tracers is not part of this class: it is Redi.h, which forms the slope from the
//    same GradRhoZ and N2E.
//
// Algorithmic traffic: 32 B per cell-level (four cell arrays, each row ideally fetched once) + 16 B per edge-level
// (BolusVelocity and StreamFunction written) + 16 B per edge-level with Transport (read and written): ~ 128 B per
// cell-level on a hexagon mesh (3 edges per cell) with Transport, ~ 80 B without.
#ifndef OMEGA_AMD_GENTMCWILLIAMS_H
#define OMEGA_AMD_GENTMCWILLIAMS_H

#include "ColumnPass.h"

namespace OMEGA {

class GentMcWilliams : public Registry<GentMcWilliams>, public ColumnPass {
 public:
   /// Refuses (OmegaError) a null or host-only mesh; a VertCoord or Eos that is null, was built for another mesh or has
   /// another layer count; NVertLayers outside 1 .. TriDiagMaxRows; a GMKappa that is negative or not finite; a
   /// GravWaveSpeed that is not finite or <= 0.  Everything is allocated here; no call allocates.
   GentMcWilliams(const std::string &Name, const HorzMesh *Mesh, VertCoord *VCoord, Eos *EqState, Real GMKappa = 600.0,
                  Real GravWaveSpeed = 0.3);

   Real GMKappa, GravWaveSpeed;
   /// [NEdgesSize], GMKappa at construction; the caller may overwrite it (e.g. to scale with the resolution)
   Array1DReal Kappa;
   /// [NEdgesSize][levelPitch(K)], zero at construction
   Array2DReal BolusVelocity, StreamFunction;

   /// The fused column pass (VertCoord::computeColumn) from raw arrays: thickness [NCellsSize][levelPitch(K)], tracers
   /// [>= 2][NCellsSize][levelPitch(K)] with TIndex = 0, SIndex = 1, Displaced = true, KDisp = 1, and this object's
   /// SurfacePressure / TidalPotential / SelfAttractionLoading (ColumnPass.h).
   void updateColumn(const Array2DReal &LayerThickness, const Array3DReal &TracerArray, hipStream_t S) const {
      ColumnPass::updateColumn(LayerThickness, TracerArray, true, S);
   }
   /// The array form of the contract: the four cell arrays [NCellsSize][levelPitch(K)]; Transport
   /// [NEdgesSize][levelPitch(K)] accumulated in place, or empty (no term).  One launch.
   void computeBolusVelocity(const Array2DReal &LayerThickness, const Array2DReal &SpecVol,
                             const Array2DReal &SpecVolDisplaced, const Array2DReal &ZMid, const Array2DReal &Transport,
                             hipStream_t S) const;
   /// the same on the attached Eos's SpecVol / SpecVolDisplaced and the VertCoord's ZMid as they stand
   void computeBolusVelocity(const Array2DReal &LayerThickness, const Array2DReal &Transport, hipStream_t S) const;

   // ---- the reference's style of signature: on this object's `Stream` (default: the null stream)
   hipStream_t Stream = nullptr;
   void updateColumn(const Array2DReal &LayerThickness, const Array3DReal &TracerArray) const {
      updateColumn(LayerThickness, TracerArray, Stream);
   }
   void computeBolusVelocity(const Array2DReal &LayerThickness, const Array2DReal &SpecVol,
                             const Array2DReal &SpecVolDisplaced, const Array2DReal &ZMid,
                             const Array2DReal &Transport) const {
      computeBolusVelocity(LayerThickness, SpecVol, SpecVolDisplaced, ZMid, Transport, Stream);
   }
   void computeBolusVelocity(const Array2DReal &LayerThickness, const Array2DReal &Transport) const {
      computeBolusVelocity(LayerThickness, Transport, Stream);
   }

   std::string Name;
};

} // namespace OMEGA
#endif
