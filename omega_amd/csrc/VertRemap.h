// VertRemap.h -- vertical Lagrangian remapping: after a step in which the layers moved with the flow (a split-explicit
// step without a VertAdv: the thickness follows the horizontal divergence alone) the column is put back on the
// VertCoord's target grid by a conservative remap of the tracers and of the velocity -- piecewise constant (PCM), linear
// (PLM, van Leer limited) or parabolic (PPM, Colella and Woodward 1984 with their monotonicity limiter) reconstruction in
// the source cells, integrated exactly over each target layer.  The reference names the scheme as desired
// (components/omega/doc/design/VertCoord.md sections 2.6, 2.7) and has no code for it: the contract below is this
// library's.  DESIGN.md section 4.16.
//
// Numerical contract (FP64, -ffp-contract=off, IEEE divisions, every chain in the order written; a NumPy restatement in
// the same order is bit-identical, tests/vert_remap_reference.py).
//
// Column core, for cells and edges alike.  A column of N >= 1 rows j = 0 .. N-1: source thickness hs[j] > 0, target
// thickness ht[j] > 0, source means a[j].
//  - Interfaces, sequential:  zs[0] = 0.0;  zs[j+1] = zs[j] + hs[j];  zt likewise from ht.
//  - The target interfaces used:  ZT[0] = 0.0;  ZT[N] = zs[N];  ZT[k] = zt[k] < zs[N] ? zt[k] : zs[N]  for 0 < k < N.
//    The target column is fitted to the source column: a rounding residue of the two totals -- or, for edges, a real
//    mismatch (below) -- ends in the last layer or layers, never outside the data.  Where the target total is the smaller
//    one the last layer is widened to the source's bottom; where it is the larger one the layers past the source's bottom
//    have no width and take a point value (below).
//  - Limited slope, 0 < j < N-1, hm, h0, hp = hs[j-1], hs[j], hs[j+1], dm = a[j] - a[j-1], dp = a[j+1] - a[j]:
//      s = (h0 / ((hm + h0) + hp)) * ((((2.0*hm) + h0) / (hp + h0)) * dp + ((h0 + (2.0*hp)) / (hm + h0)) * dm)
//      if dp*dm > 0.0:  t = |s|;  m = 2.0*|dm|;  t = m < t ? m : t;  m = 2.0*|dp|;  t = m < t ? m : t;
//                       d[j] = s < 0.0 ? -t : t
//      else             d[j] = 0.0
//    d[0] = d[N-1] = 0.0.
//  - Reconstruction in cell j, xi in [0, 1] from its top:  R(xi) = aL + xi*(Dl + a6*(1.0 - xi)),  Dl = aR - aL.
//      Order 1:  aL = aR = a[j], a6 = 0.0.
//      Order 2:  aL = a[j] - 0.5*d[j];  aR = a[j] + 0.5*d[j];  a6 = 0.0.
//      Order 3:  the value e[j] at the interface between j and j+1 (0 <= j <= N-2), h0, hp = hs[j], hs[j+1],
//                da = a[j+1] - a[j]:
//                  b = a[j] + (h0 / (h0 + hp)) * da
//                where both cells have a neighbour on the far side (1 <= j and j+2 <= N-1), hm = hs[j-1], hpp = hs[j+2]:
//                  F1 = ((2.0*hp) * h0) / (h0 + hp)
//                  F2 = (hm + h0) / ((2.0*h0) + hp)
//                  F3 = (hpp + hp) / ((2.0*hp) + h0)
//                  T1 = (F1 * (F2 - F3)) * da
//                  T2 = ((h0 * (hm + h0)) / ((2.0*h0) + hp)) * d[j+1]
//                  T3 = ((hp * (hp + hpp)) / (h0 + (2.0*hp))) * d[j]
//                  e[j] = b + (1.0 / (((hm + h0) + hp) + hpp)) * ((T1 - T2) + T3)
//                elsewhere  e[j] = b.
//                Cells 0 and N-1 stay constant: aL = aR = a[j].  A cell 0 < j < N-1 takes aL = e[j-1], aR = e[j], then
//                  if (aR - a)*(a - aL) <= 0.0:  aL = aR = a
//                  else:  Dl = aR - aL;  Q = Dl * (a - 0.5*(aL + aR));  S = (Dl*Dl) / 6.0
//                         if Q > S:        aL = (3.0*a) - (2.0*aR)
//                         else if -S > Q:  aR = (3.0*a) - (2.0*aL)
//                a6 = 6.0 * (a - 0.5*(aL + aR))   (exactly 0.0 for a constant cell).
//  - Target layer k, z0 = ZT[k], z1 = ZT[k+1]:
//      j0 = the largest j <= N-1 with zs[j] <= z0;  j1 = the largest j <= N-1 with zs[j] < z1, and at least j0.
//      for j = j0 .. j1 ascending, Sum = 0.0 before the first:
//         x0 = j == j0 ? (z0 - zs[j]) / hs[j] : 0.0
//         x1 = j == j1 ? (z1 == zs[j+1] ? 1.0 : (z1 - zs[j]) / hs[j]) : 1.0
//           (an interface that equals the source cell's lower one bit for bit is its xi = 1: the quotient of the rounded
//           difference zs[j+1] - zs[j] by hs[j] need not be)
//         piece = hs[j]*a[j]                                                           if x0 == 0.0 and x1 == 1.0
//         piece = hs[j] * ((aL*(x1 - x0) + (0.5*(Dl + a6)) * ((x1*x1) - (x0*x0)))
//                          - (a6/3.0) * (((x1*x1)*x1) - ((x0*x0)*x0)))                 otherwise
//         Sum = Sum + piece
//      r = Sum / (z1 - z0)
//    with two exceptions: a target layer whose two interfaces are those of one source cell bit for bit (j0 == j1,
//    x0 == 0.0, x1 == 1.0) takes r = a[j0]; a layer without width (z1 <= z0) takes r = R(x0) of cell j0.  Then
//      lo, hi = the min, max of a[max(j0-1, 0) .. min(j1+1, N-1)];  r = r < lo ? lo : r;  r = r > hi ? hi : r
//    and r is the new mean of layer k.  The clamp only ever removes rounding: the limited reconstructions are monotone.
//
// The calls.  W = VertCoordMovementWeights, Ref = RefLayerThickness of the VertCoord.
//  computeTarget(h): cells c < NCellsAll with a range 0 <= KMin <= KMax < NVertLayers (MinLayerCell / MaxLayerCell):
//      SumH = SumRef = SumWh = 0.0
//      for K = KMin .. KMax ascending:  SumH = SumH + h[c][K];  SumWh = SumWh + W[K]*Ref[c][K];  SumRef = SumRef + Ref[c][K]
//      Coeff = SumH - SumRef
//      LayerThicknessTarget[c][K] = Ref[c][K] * (1.0 + (Coeff*W[K]) / SumWh)
//    VertCoord::computeTargetThickness's expression, with the column total taken from h itself instead of from the
//    pressure of a column pass.
//  remapTracers(h, Tracers, NTracers): the core on KMin .. KMax of every such cell, hs = h[c], ht = LayerThicknessTarget[c],
//    a = Tracers[L][c] for every L < NTracers, in place.  One launch whatever NTracers.
//  remapVelocity(h, u): edges e < NEdgesAll, c0, c1 = CellsOnEdge[e], on Lo .. Hi = MinLayerEdgeBot[e] ..
//    MaxLayerEdgeTop[e] (the levels active in both cells):
//      hs[K] = 0.5*(h[c0][K] + h[c1][K]);  ht[K] = 0.5*(LayerThicknessTarget[c0][K] + LayerThicknessTarget[c1][K])
//    a = u[e], in place.  An edge whose range is not 0 <= Lo <= Hi < NVertLayers or with a cell outside [0, NCellsSize) is
//    left alone (edgeColumn of kernels/PackedColumns.h).  Here the two totals genuinely differ where the two cells have
//    different ranges -- the target of each cell conserves that cell's own total, not the part of it inside the edge's
//    range -- and the ZT rule of the core is what decides those cases.
//  adoptTarget(h): h[c][K] = LayerThicknessTarget[c][K] on the cells' ranges.
//  remap(h, u, Tracers, NTracers): computeTarget, remapTracers, remapVelocity, adoptTarget, in three launches -- the
//    target and the tracers in one, the velocity, the thickness -- with the bits of the four calls.
// Nothing but the stated entries is written by any call: no other level, no land column, no row >= N*All, not the
// sentinel row, not the pitch padding.  Halo cells and edges are swept like owned ones.
//
// Algorithmic traffic per cell-level: the target 24 B (h, Ref read, target written); the tracers 16 B (h, target) + 16 B
// per tracer (read and written); the adoption 16 B; the velocity 16 B per cell-level (h and the target, each row ideally
// once) + 16 B per edge-level (u read and written).  remap: 24 B + 16 B per tracer per cell-level in its first launch,
// the velocity's in its second, 16 B in its last.
#ifndef OMEGA_AMD_VERTREMAP_H
#define OMEGA_AMD_VERTREMAP_H

#include "Base.h"
#include "HorzMesh.h"
#include "VertCoord.h"

namespace OMEGA {

struct VertRemapConfig {
   int Order = 3; ///< the reconstruction: 1 PCM, 2 PLM, 3 PPM
};

class VertRemap : public Registry<VertRemap> {
 public:
   /// Refuses (OmegaError) a null or host-only mesh, a VertCoord that is null, was built for another mesh or has another
   /// layer count than the mesh, an Order outside 1 .. 3, MaxTracers < 0, and more layers than the column kernel's LDS
   /// tile holds (maxLayers()).  Everything is allocated here; no call allocates.
   VertRemap(const std::string &Name, const HorzMesh *Mesh, const VertCoord *VCoord, int MaxTracers,
             const VertRemapConfig &Config = VertRemapConfig());
   /// the largest NVertLayers the column kernels accept
   static int maxLayers();

   I4 NVertLayers;
   I4 MaxTracers;
   VertRemapConfig Config;
   Array2DReal LayerThicknessTarget; ///< [NCellsSize][levelPitch(K)], zero at construction
   HostArrayReal LayerThicknessTargetH;
   mutable I8 LaunchCount = 0; ///< kernel launches issued by the five calls so far

   void computeTarget(const Array2DReal &LayerThickness, hipStream_t S) const;
   /// Tracers [>= NTracers][NCellsSize][levelPitch(K)].  Refuses NTracers outside 0 .. MaxTracers; 0 is no launch.
   void remapTracers(const Array2DReal &LayerThickness, const Array3DReal &Tracers, int NTracers, hipStream_t S) const;
   void remapVelocity(const Array2DReal &LayerThickness, const Array2DReal &NormalVelocity, hipStream_t S) const;
   void adoptTarget(const Array2DReal &LayerThickness, hipStream_t S) const;
   /// the four calls above in that order, in three launches; the same bits
   void remap(const Array2DReal &LayerThickness, const Array2DReal &NormalVelocity, const Array3DReal &Tracers,
              int NTracers, hipStream_t S) const;

   // ---- the reference's style of signature: on this object's `Stream` (default: the null stream)
   hipStream_t Stream = nullptr;
   void computeTarget(const Array2DReal &LayerThickness) const { computeTarget(LayerThickness, Stream); }
   void remapTracers(const Array2DReal &LayerThickness, const Array3DReal &Tracers, int NTracers) const {
      remapTracers(LayerThickness, Tracers, NTracers, Stream);
   }
   void remapVelocity(const Array2DReal &LayerThickness, const Array2DReal &NormalVelocity) const {
      remapVelocity(LayerThickness, NormalVelocity, Stream);
   }
   void adoptTarget(const Array2DReal &LayerThickness) const { adoptTarget(LayerThickness, Stream); }
   void remap(const Array2DReal &LayerThickness, const Array2DReal &NormalVelocity, const Array3DReal &Tracers,
              int NTracers) const {
      remap(LayerThickness, NormalVelocity, Tracers, NTracers, Stream);
   }

   void copyToHost(); ///< LayerThicknessTarget -> LayerThicknessTargetH (synchronises the device)

   const HorzMesh *Mesh;
   const VertCoord *VCoord;
   std::string Name;

 private:
   void cellLaunch(const Array2DReal &H, const Array3DReal *Tracers, int NTracers, bool Target, hipStream_t S) const;
};

} // namespace OMEGA
#endif
