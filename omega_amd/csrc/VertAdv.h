// VertAdv.h -- vertical transport and vertical advection of a layered ocean: the thickness flux through the layer
// interfaces that holds the grid to the VertCoord's z-star ("Uniform" movement weights) or z-level ("Fixed") shape, and
// the terms it adds to the thickness, tracer and momentum tendencies.  The reference names the terms in its
// governing-equation document (components/omega/doc/design/OmegaV1GoverningEqns.md, discrete-mass, discrete-tracer,
// discrete-momentum) and has no code for them; the contract below is this library's.
//
// VerticalTransport is [NCellsSize][levelPitch(K)]: row K is the thickness flux (m/s) through the TOP of layer K,
// positive upward (the interface convention of VertMix).  The bottom interface of KMax is not stored and is zero.
//
// Numerical contract (FP64, -ffp-contract=off, IEEE divisions, every chain in the order written; a NumPy restatement in
// the same order is bit-identical, tests/vert_adv_reference.py).  A column is a cell c < NCellsAll with
// 0 <= KMin <= KMax < NVertLayers (the VertCoord's MinLayerCell / MaxLayerCell); W = VertCoordMovementWeights,
// Ref = RefLayerThickness of the VertCoord, D = the thickness tendency handed in.
//
//  computeVerticalTransport(D), D [NCellsSize][pitch], the horizontal part -div([h]_e u):
//      SumD = 0; SumWh = 0
//      for K = KMin .. KMax ascending:  SumD = SumD + D[K];  SumWh = SumWh + W[K]*Ref[c][K]
//      Acc = 0
//      for K = KMax .. KMin descending:
//          TT  = ((W[K]*Ref[c][K]) / SumWh) * SumD        (d/dt of VertCoord's LayerThicknessTarget[K])
//          Acc = Acc + (D[K] - TT)
//          VerticalTransport[c][K] = Acc
//      VerticalTransport[c][KMin] = 0.0
//    The surface is closed: what the sums leave at KMin is rounding residue of SumD - sum(TT) and is dropped.  Entries
//    outside the range, land columns, rows >= NCellsAll, the sentinel row and the pitch padding are not written.
//    "Fixed" weights give a z-level grid (all motion goes into the top layer), "Uniform" z-star.
//
//  addThicknessTend(Tend), cells < NCellsAll, K in KMin .. KMax, Wt = VerticalTransport[c]:
//      Wb = K < KMax ? Wt[K+1] : 0.0
//      Tend[c][K] = (Tend[c][K] - Wt[K]) + Wb
//
//  addTracerTend(Tend, h, Tracers, NTracers), Tend / Tracers [NTracers][NCellsSize][pitch], cells < NCellsAll, every
//  tracer L, Phi = Tracers[L][c].  The interface value at KMin < K <= KMax:
//      order 2:  PhiTop[K] = ((h[K-1]*Phi[K]) + (h[K]*Phi[K-1])) / (h[K-1] + h[K])
//      order 1:  PhiTop[K] = Wt[K] > 0.0 ? Phi[K] : Phi[K-1]
//    and the flux  F[K] = Wt[K]*PhiTop[K]  there;  F[KMin] = 0.0 and F[KMax+1] = 0.0, with no value read for them.
//      Tend[L][c][K] = (Tend[L][c][K] - F[K]) + F[K+1]
//    The tendency is that of h*phi, as everywhere in Tendencies.
//
//  addVelocityTend(Tend, h, u), edges e < NEdgesAll, c0, c1 = CellsOnEdge[e], K in Lo .. Hi = MinLayerEdgeBot[e] ..
//  MaxLayerEdgeTop[e] (the levels active in both cells; an empty range leaves the edge alone):
//      hE      = 0.5*(h[c0][K] + h[c1][K])
//      We[K]   = 0.5*(Wt[c0][K] + Wt[c1][K])
//      UTop[K] = 0.5*(u[e][K-1] + u[e][K])
//      FTop    = K == Lo ? 0.0 : We[K]  *(UTop[K]   - u[e][K])
//      FBot    = K == Hi ? 0.0 : We[K+1]*(UTop[K+1] - u[e][K])
//      Tend[e][K] = Tend[e][K] - EdgeMask[e]*((FTop - FBot)/hE)
//    Where one cell is deeper than the other no momentum passes the interface below the edge's last common level (nor
//    the one above its first): the edge's column is closed at both ends of its own range.
//
// Nothing but the stated entries is written by any call.  Halo cells and edges are swept like owned ones.
//
// Algorithmic traffic per cell-level: the transport 24 B (D, Ref read, VerticalTransport written), with the thickness
// update folded in 32 B; the thickness update alone 24 B; the tracer term 16 B + 24 B per tracer; the velocity term
// 16 B per cell-level (h, VerticalTransport, each row ideally once) + 24 B per edge-level (u read, Tend read and
// written).
#ifndef OMEGA_AMD_VERTADV_H
#define OMEGA_AMD_VERTADV_H

#include "Base.h"
#include "HorzMesh.h"
#include "VertCoord.h"

namespace OMEGA {

struct VertAdvConfig {
   int TracerFluxOrder = 2; ///< interface value of the tracer flux: 1 upwind, 2 centred (thickness-weighted)
};

class VertAdv : public Registry<VertAdv> {
 public:
   /// Refuses (OmegaError) a null or host-only mesh, a VertCoord that is null, was built for another mesh or has
   /// another layer count than the mesh, a TracerFluxOrder other than 1 or 2, and more layers than the column kernel's
   /// LDS tile holds (maxLayers()).  Everything is allocated here; no call allocates.
   VertAdv(const std::string &Name, const HorzMesh *Mesh, const VertCoord *VCoord, const VertAdvConfig &Config);
   /// the largest NVertLayers the column kernel accepts
   static int maxLayers();

   I4 NVertLayers;
   VertAdvConfig Config;
   Array2DReal VerticalTransport; ///< [NCellsSize][levelPitch(K)], zero at construction
   /// false: the Tendencies leave this object's tracer term out (the tracer group, computeTransportTendencies,
   /// computeAllTendencies), for a MonotoneAdv that limits the vertical flux itself (MonotoneAdv::attachVertAdv).
   /// addTracerTend called directly does not look at it; the thickness and velocity terms are not concerned.
   bool TracerTermEnable = true;
   HostArrayReal VerticalTransportH;

   void computeVerticalTransport(const Array2DReal &ThickTend, hipStream_t S) const;
   void addThicknessTend(const Array2DReal &Tend, hipStream_t S) const;
   /// computeVerticalTransport(Tend) and addThicknessTend(Tend) in one launch (the scan already holds the tendency);
   /// the same bits as the two calls
   void computeAndAddThickness(const Array2DReal &Tend, hipStream_t S) const;
   void addTracerTend(const Array3DReal &Tend, const Array2DReal &LayerThickness, const Array3DReal &Tracers,
                      int NTracers, hipStream_t S) const;
   void addVelocityTend(const Array2DReal &Tend, const Array2DReal &LayerThickness, const Array2DReal &NormalVelocity,
                        hipStream_t S) const;

   // ---- the reference's style of signature: on this object's `Stream` (default: the null stream)
   hipStream_t Stream = nullptr;
   void computeVerticalTransport(const Array2DReal &ThickTend) const { computeVerticalTransport(ThickTend, Stream); }
   void addThicknessTend(const Array2DReal &Tend) const { addThicknessTend(Tend, Stream); }
   void computeAndAddThickness(const Array2DReal &Tend) const { computeAndAddThickness(Tend, Stream); }
   void addTracerTend(const Array3DReal &Tend, const Array2DReal &LayerThickness, const Array3DReal &Tracers,
                      int NTracers) const {
      addTracerTend(Tend, LayerThickness, Tracers, NTracers, Stream);
   }
   void addVelocityTend(const Array2DReal &Tend, const Array2DReal &LayerThickness,
                        const Array2DReal &NormalVelocity) const {
      addVelocityTend(Tend, LayerThickness, NormalVelocity, Stream);
   }

   void copyToHost(); ///< VerticalTransport -> VerticalTransportH (synchronises the device)

   const HorzMesh *Mesh;
   const VertCoord *VCoord;
   std::string Name;

 private:
   void columnLaunch(const Array2DReal &Tend, bool Scan, bool Thick, hipStream_t S) const;
};

} // namespace OMEGA
#endif
