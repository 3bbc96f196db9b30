// MonotoneAdv.h -- flux-corrected horizontal tracer advection: the centred (second-order) tracer flux of every edge,
// limited against the first-order upwind flux after Zalesak so that a forward-in-time update creates no new extremum.
// The reference asks for such a scheme in its design documents (components/omega/doc/design/Tracers.md: "many tracers
// will require monotonic or positive-definite advection schemes to prevent negative concentrations";
// OmegaV0ShallowWater.md section 3.5.1 names MPAS-Ocean's flux-corrected transport) and has no code for it: its
// TracerAuxVars offers FluxTracerEdgeOption::Center, which overshoots at every front, and Upwind, which is first order.
// The contract below is this library's.  A limiter needs a forward update with a known Dt: steps 6-7 of
// SplitExplicitStepper are one (SplitExplicitStepper::attachMonotoneAdv).
//
// Numerical contract (FP64, -ffp-contract=off, IEEE divisions, every chain in the order written; a NumPy restatement in
// the same order is bit-identical, tests/monotone_adv_reference.py).  max and min are comparisons,
//      max(a, b) = a < b ? b : a          min(a, b) = b < a ? b : a
// so they mean the same in C++ and in NumPy for every operand.  All levels K < NVertLayers are swept, as by the
// horizontal terms of Tendencies.  phi = Tracers[L], per tracer L < NTracers and level.
//
//  An edge e < NEdgesAll, c0, c1 = CellsOnEdge[e]:
//      EdgeMask[e] == 0:  Fm = 0.0 exactly; no cell is read; the edge enters no sum and no max/min
//      hE    = 0.5*(hOld[c0] + hOld[c1])
//              (FluxThicknessUpwind: u[e] > 0 ? hOld[c0] : u[e] < 0 ? hOld[c1] : max(hOld[c0], hOld[c1]),
//               the upwind flux thickness of LayerThicknessAuxVars)
//      Fm    = DvEdge[e]*(hE*u[e])
//      FLow  = Fm >= 0.0 ? Fm*phi[c0] : Fm*phi[c1]
//      FHigh = Fm*(0.5*(phi[c0] + phi[c1]))
//      A     = FHigh - FLow
//    A slot of EdgesOnCell that names no local edge (e >= NEdgesAll: the rim of the halo) counts as masked out.  DvEdge
//    of a local edge is positive.
//
//  Pass 1, cells c < NCellsAll, slots j < NEdgesOnCell[c] in slot order, masked-out slots skipped;
//  s = EdgeSignOnCell[c][j] (-1 where c is c0), n the cell across the edge, InvA = 1/AreaCell[c]; every sum starts at 0.0
//  and adds its terms one by one:
//      PMax = PMin = phi[c];  PMax = max(PMax, phi[n]);  PMin = min(PMin, phi[n])
//      DivLow = sum of s*FLow;            HTd  = hOld[c]*phi[c] + Dt*(DivLow*InvA)
//      PIn  = Dt*((sum of max(s*A, 0.0))*InvA);       POut = Dt*((sum of max(-(s*A), 0.0))*InvA)
//      QIn  = max(0.0, PMax*hNew[c] - HTd);           QOut = max(0.0, HTd - PMin*hNew[c])
//      ScaleIn[L][c]  = PIn  > 0.0 ? min(1.0, QIn/PIn)   : 1.0
//      ScaleOut[L][c] = POut > 0.0 ? min(1.0, QOut/POut) : 1.0
//    (s*X is X or -X: exact.)
//
//  Pass 2, cells c < NCellsAll, the same slots in the same order; both cells of an edge recompute the edge from the same
//  operands in the edge's orientation, so they agree on every bit:
//      Sc = A >= 0.0 ? min(ScaleOut[L][c0], ScaleIn[L][c1]) : min(ScaleIn[L][c0], ScaleOut[L][c1])
//      F  = FLow + Sc*A
//      Tend[L][c] = Tend[L][c] + (sum of s*F)*InvA
//    The tendency is that of h*phi, as everywhere in Tendencies.
//
// Only Tend[L < NTracers][c < NCellsAll][K < NVertLayers] and the same entries of ScaleIn / ScaleOut are written: no plane
// >= NTracers, no row >= NCellsAll, not the sentinel row, not the pitch padding.  The inputs are not written.
//
// Halo cells are swept like owned ones.  A cell of the outermost halo layer lacks the edges beyond the rim (they are
// masked out), so its sums are truncated and its scale factors are not those of the global mesh -- the truncation
// BarotropicMode.h describes for its rim.  Those scale factors enter the fluxes of the layer inside it, so the result on
// owned cells is that of the global mesh for a halo of at least 2 cell layers.
//
// What the limiter guarantees (Zalesak 1979; the horizontal case).  Given, on every cell-level,
//      hOld[c] - Dt*InvA*(sum over the edges with outflow of |Fm|) >= 0          (an outflow Courant number <= 1)
//      hNew[c] = hOld[c] - Dt*div(Fm)        up to rounding                      (the thickness the same fluxes give)
// the low-order update HTd/hNew is a convex combination of phi[c] and the upwind neighbours, hence inside
// [PMin, PMax]; ScaleIn caps the anti-diffusive inflow at what lifts the cell to PMax, ScaleOut the outflow at what
// lowers it to PMin, and an edge takes the smaller of the two factors that concern it, so the updated value
// (hOld*phi + Dt*Tend)/hNew lies in [PMin, PMax] up to rounding (tests/test_monotone_adv.py derives the margin).  A
// constant tracer has FHigh == FLow bit for bit on every edge (0.5*(p + p) == p), so A = 0 exactly and the update is
// the low-order one, which keeps a constant up to the rounding of hNew.  With a VertAdv attached to the Tendencies and
// none attached here the vertical term is added unlimited and the guarantee holds for the horizontal part only; the
// 3-D form below limits both.
//
// The 3-D form (attachVertAdv(V); same rules: FP64, -ffp-contract=off, every chain in the order written, the same max
// and min; a NumPy restatement in the same order is bit-identical, tests/monotone_adv_reference.py).  Everything
// about the horizontal edges stays as written above: Fm, FLow, FHigh, A, the slot order, the masking.
//
//  Interfaces of a cell c < NCellsAll with KMin .. KMax = MinLayerCell[c] .. MaxLayerCell[c] of V->VCoord,
//  Wt = V->VerticalTransport[c] as it stands, h = hOld[c].  Interface K is the top of layer K, Wt positive upward: a
//  positive flux leaves layer K and enters layer K-1.
//      Wv[K]    = (KMin < K && K <= KMax) ? Wt[K] : 0.0           (a select: Wt outside the range is never used)
//      VLow[K]  = Wv[K] > 0.0 ? Wv[K]*phi[K] : Wv[K]*phi[K-1]     (VertAdv's order-1 flux)
//      PhiT[K]  = phi[K-1] + (h[K-1]/(h[K-1] + h[K]))*(phi[K] - phi[K-1])
//      VHigh[K] = Wv[K]*PhiT[K]
//      AV[K]    = VHigh[K] - VLow[K]
//    PhiT is VertAdv's order-2 interface value, rearranged so that a constant tracer has AV == 0 bit for bit, the
//    property A has.  At an interface outside KMin < K <= KMax -- the bottom of KMax and everything at K >= NVertLayers
//    included -- VLow = AV = 0.0 exactly and no phi, h, ScaleIn or ScaleOut value from across it enters any arithmetic.
//    Levels outside KMin .. KMax and land columns (MaxLayerCell < MinLayerCell) so get the horizontal form only; they
//    are swept as above.
//
//  Pass 1, level K of cell c, after the horizontal slots:
//      PMax = max(PMax, phi[K-1]), PMin = min(PMin, phi[K-1])   if KMin < K <= KMax
//      PMax = max(PMax, phi[K+1]), PMin = min(PMin, phi[K+1])   if KMin <= K < KMax       (in this order)
//      HTd  = hOld*phi + Dt*(((DivLow*InvA) - VLow[K]) + VLow[K+1])
//      PIn  = Dt*((((sum of max(s*A, 0.0))*InvA)    + max(-AV[K], 0.0)) + max(AV[K+1], 0.0))
//      POut = Dt*((((sum of max(-(s*A), 0.0))*InvA) + max(AV[K], 0.0))  + max(-AV[K+1], 0.0))
//      QIn, QOut, ScaleIn, ScaleOut as above
//
//  Pass 2, the scale factors of the cell's own rows:
//      ScV[K] = AV[K] >= 0.0 ? min(ScaleOut[K], ScaleIn[K-1]) : min(ScaleIn[K], ScaleOut[K-1])
//      FV[K]  = VLow[K] + ScV[K]*AV[K]          (0.0 outside KMin < K <= KMax; no scale factor is read there)
//      Tend[L][c][K] = Tend[L][c][K] + ((((sum of s*F)*InvA) - FV[K]) + FV[K+1])
//    Layers K and K-1 evaluate interface K from the same operands, so the column telescopes exactly as the edges do.
//
//  The guarantee in 3-D.  Given, on every cell-level,
//      hOld - Dt*(InvA*(sum over the edges with outflow of |Fm|) + max(Wv[K], 0) + max(-Wv[K+1], 0)) >= 0
//      hNew = hOld + Dt*(-div(Fm) - Wv[K] + Wv[K+1])        up to rounding
//  the update (hOld*phi + Dt*Tend)/hNew lies between the smallest and the largest phi of the cell, its edge neighbours
//  and the levels above and below it inside the range, up to rounding (tests/test_monotone_adv_3d.py derives the margin).
//  The vertical part needs no other cell, so the halo rule stays at 2 cell layers.  The Tendencies must not add the
//  vertical tracer term as well: VertAdv::TracerTermEnable = false (SplitExplicitStepper::attachMonotoneAdv checks it).
//
//  Traffic of the 3-D form per cell-level of a hexagon mesh (the rows of the cell's own column count once per launch):
//  pass 1 adds VerticalTransport, 48 B + 24 B per tracer; pass 2 likewise, 40 B + 40 B per tracer; and 8 B per cell and
//  launch for the range.  DESIGN.md section 4.11.
//
// The high-order horizontal flux (setHorzOrder(3 or 4); same rules: FP64, -ffp-contract=off, every chain in the order
// written, the same max and min; a NumPy restatement in the same order that reads the tables from the object is
// bit-identical, tests/monotone_adv_reference.py).  OmegaV0ShallowWater.md section 3.5.1 describes MPAS-Ocean's
// transport as "fourth order under normal conditions, and reduces to third order to preserve monotonicity"
// (Skamarock and Gassmann 2011): the centred edge value is corrected by the second derivative of phi along the line
// between the two cells, taken from a least-squares quadratic at each of them.  Zalesak's argument holds for any FHigh,
// so Fm, FLow, A = FHigh - FLow, both passes, the vertical form and the masking are exactly as written above.
//
//  Tables, built once on the host by setHorzOrder (checked to a tolerance: a least-squares solve is not restated bit
//  for bit):
//    A cell c < NCellsAll is a fit cell (FitCell[c] = 1.0, else 0.0) when NEdgesOnCell[c] >= 5, every slot
//    j < NEdgesOnCell[c] names a local edge (e < NEdgesAll) with EdgeMask != 0 and a local cell across it
//    (n < NCellsAll), and the fit matrix below has full column rank (Householder QR: the smallest |R(k,k)| is above
//    1e-8 times the largest).  A coast cell and a cell of the outermost halo layer are never fit cells.
//    d_j: the offset from c to the cell across slot j.  Planar: X_n - X_c, the minimum image over a non-zero period.
//    Sphere: azimuthal equidistant -- the direction of the tangential part of X_n - X_c at c, the length
//    R*acos(r_c.r_n), evaluated as R*atan2(|r_c x r_n|, r_c.r_n): acos loses half the digits at these angles.
//    (e1, e2): an orthonormal frame of the tangent plane at c; the results do not depend on it beyond rounding, and the
//    library takes x, y on a plane and e1 = a x r_c/|a x r_c|, e2 = r_c x e1 on a sphere, a the z axis, or the x axis
//    where |r_c.z| >= 0.9.  (x_j, y_j): the components of d_j/L, L the mean |d_j|.  With P+ the pseudo-inverse of the
//    n x 5 matrix of rows (x, y, x^2, x*y, y^2) -- the least-squares quadratic through the centre value --
//      HessWeight[c][j] = (2*P+[2][j], P+[3][j], 2*P+[4][j])/L^2     (phi_xx, phi_xy, phi_yy per unit phi[n_j] - phi[c])
//    and zeros for a cell that is not a fit cell.  An edge is high when it is masked in and both its cells are fit
//    cells.  For slot j of c with edge e, (cs, sn) the unit direction of d_j in c's frame:
//      EdgeDirOwn[c][j]    = (DcEdge[e]^2/12)*(cs^2, 2*cs*sn, sn^2)
//      EdgeDirAcross[c][j] = a copy of EdgeDirOwn[n][j'], j' the slot of e in n (the same bits)
//    both 0.0 on a slot whose edge is not high.  EdgeDirOwn[c][j][0] and [2] are not both zero on a high edge, which is
//    how the kernels tell one.
//
//  Pass 0, cells c < NCellsAll, all levels, per tracer L and t in {xx, xy, yy}:
//      Hess[L][t][c] = the sum, started at 0.0, of HessWeight[c][j][t]*(phi[n_j] - phi[c]) over the slots in slot order
//    a cell that is not a fit cell stores 0.0 and reads no neighbour.
//
//  The edge, as evaluated by both its cells in passes 1 and 2, in the edge's orientation (Q0: the direction
//  coefficients on c0's side -- EdgeDirOwn of c0's slot, which is EdgeDirAcross of c1's):
//      D0    = (Q0[0]*Hxx[c0] + Q0[1]*Hxy[c0]) + Q0[2]*Hyy[c0]
//      D1    = (Q1[0]*Hxx[c1] + Q1[1]*Hxy[c1]) + Q1[2]*Hyy[c1]
//      S = D0 + D1;   T = D0 - D1;   B = Beta*T
//      Corr  = high edge ? S + (Fm >= 0.0 ? B : -B) : 0.0        (a select: nothing of Hess enters on another edge)
//      FHigh = Fm*(0.5*(phi[c0] + phi[c1]) - Corr)
//    Beta = 0.0 at order 4 and Coef3rdOrder at order 3 (MPAS's default 0.25; 1: the upwind-biased third order).  A
//    constant tracer has Hess == 0.0 exactly, so Corr = 0.0 and A = 0.0 bit for bit as before.
//
//  Only Hess[L < NTracers][t][c < NCellsAll][K < NVertLayers] is written besides the entries named above.  Hess of a
//  cell needs its neighbours, the scale factors need Hess of the cell and of the cells across, and the fluxes need the
//  scale factors of the cells across: the result on owned cells is that of the global mesh for a halo of at least 3
//  cell layers, the reference's default (Decomp.md gives higher-order tracer advection as one reason for it).
//
//  Three launches; traffic per cell-level of a hexagon mesh: pass 0 reads phi and writes three rows per tracer (32 B);
//  pass 1 adds the three Hess rows (40 B + 48 B per tracer), pass 2 likewise (32 B + 64 B per tracer): 72 B + 144 B per
//  tracer.  DESIGN.md section 4.12.
//
// Two launches per call, both tile sweeps over the cells (kernels/MonotoneAdvKernels.hip); no atomics and no
// edge-located array.  Algorithmic traffic per cell-level of a hexagon mesh (3 edge rows per cell), every row counted
// once per launch: pass 1 reads hOld, hNew and 3 u (40 B) and per tracer reads phi and writes the two scale factors
// (24 B); pass 2 reads hOld and 3 u (32 B) and per tracer reads phi and the two scale factors and updates Tend in place
// (40 B): 72 B + 64 B per tracer.  DESIGN.md section 4.10 has the measurement.
#ifndef OMEGA_AMD_MONOTONEADV_H
#define OMEGA_AMD_MONOTONEADV_H

#include "Base.h"
#include "HorzMesh.h"
#include "VertAdv.h"

namespace OMEGA {

struct MonotoneAdvConfig {
   bool FluxThicknessUpwind = false; ///< must match the AuxiliaryState's FluxThickEdgeChoice (Upwind: true)
};

/// The high-order horizontal flux of MonotoneAdv::setHorzOrder
struct MonoHighOrderConfig {
   int HorzOrder     = 2;    ///< 2: the centred flux; 4: Beta = 0.0; 3: Beta = Coef3rdOrder
   Real Coef3rdOrder = 0.25; ///< in (0, 1]; MPAS's default
   Real SphereRadius = 0.0;  ///< 0: planar
   Real XPeriod = 0.0, YPeriod = 0.0; ///< 0: not periodic
};

/// The tables of the high-order flux as setHorzOrder builds them, on the host alone (a host-only mesh will do): FitCell
/// [NCellsSize], HessWeight, EdgeDirOwn, EdgeDirAcross [NCellsSize][MaxEdges][3].  build refuses what setHorzOrder
/// refuses; at order 2 it builds nothing.
struct MonoHighOrderTables {
   HostArrayReal Fit, Weight, Own, Acr;
   void build(const HorzMesh &M, const MonoHighOrderConfig &C);
};

class MonotoneAdv : public Registry<MonotoneAdv> {
 public:
   /// Refuses (OmegaError) a null or host-only mesh, NVertLayers < 1 and MaxTracers < 1.  Everything is allocated here;
   /// no call allocates.
   MonotoneAdv(const std::string &Name, const HorzMesh *Mesh, int NVertLayers, int MaxTracers,
               const MonotoneAdvConfig &Config);

   I4 NVertLayers, MaxTracers;
   MonotoneAdvConfig Config;
   Array3DReal ScaleIn, ScaleOut; ///< [MaxTracers][NCellsSize][levelPitch(K)], zero at construction
   HostArrayReal ScaleInH, ScaleOutH;

   /// Tend += the limited flux divergence of Tracers[0 .. NTracers) over the step hOld -> hNew of length Dt by the
   /// velocity u.  Refuses NTracers outside 1 .. MaxTracers, a Dt that is not finite and positive, and arrays of another
   /// shape.  Two launches; three at order 3 or 4 (setHorzOrder).
   void addTracerTend(const Array3DReal &Tend, const Array2DReal &hOld, const Array2DReal &hNew, const Array2DReal &u,
                      const Array3DReal &Tracers, int NTracers, Real Dt, hipStream_t S) const;

   // ---- the reference's style of signature: on this object's `Stream` (default: the null stream)
   hipStream_t Stream = nullptr;
   void addTracerTend(const Array3DReal &Tend, const Array2DReal &hOld, const Array2DReal &hNew, const Array2DReal &u,
                      const Array3DReal &Tracers, int NTracers, Real Dt) const {
      addTracerTend(Tend, hOld, hNew, u, Tracers, NTracers, Dt, Stream);
   }

   /// While a VertAdv is attached addTracerTend runs the 3-D form: the same arguments, two launches, no allocation; it
   /// reads V->VerticalTransport as it stands and the layer ranges of V->VCoord.  nullptr detaches.  Refuses (OmegaError)
   /// a VertAdv of another mesh or layer count.
   void attachVertAdv(const VertAdv *V);
   const VertAdv *vertAdv() const { return VAdv; }

   /// Orders 3 and 4: builds the tables of the high-order flux on the host from the mesh's host arrays, uploads them and
   /// allocates Hess (the only allocation; addTracerTend still allocates nothing), and addTracerTend runs three launches.
   /// Order 2 frees nothing and switches the form off: two launches and the bits of an object never configured.
   /// Refuses (OmegaError) an order outside {2, 3, 4}, Coef3rdOrder outside (0, 1] at order 3 and a negative or
   /// non-finite radius or period.
   void setHorzOrder(const MonoHighOrderConfig &C);
   MonoHighOrderConfig HighOrder; ///< as last set
   Array3DReal Hess;              ///< [MaxTracers*3][NCellsSize][levelPitch(K)]: plane 3*L + t, t = xx, xy, yy
   Array3DReal HessWeight, EdgeDirOwn, EdgeDirAcross; ///< [NCellsSize][MaxEdges][3]
   Array1DReal FitCell;                               ///< [NCellsSize] 1.0 / 0.0
   mutable I8 LaunchCount = 0; ///< kernel launches issued by addTracerTend so far

   void copyToHost(); ///< ScaleIn, ScaleOut -> their host mirrors (synchronises the device)

   const HorzMesh *Mesh;
   std::string Name;

 private:
   const VertAdv *VAdv = nullptr;
};

} // namespace OMEGA
#endif
