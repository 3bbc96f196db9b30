// Eos.h -- equation of state: specific volume from conservative temperature, absolute salinity and pressure.
// Interface and array names after the reference (components/omega/src/ocn/Eos.h:278-328, Eos.cpp:113-176).
//
// Numerical contract (FP64, the library is built with -ffp-contract=off, so a NumPy restatement in the same order is
// bit-identical: tests/column_reference.py):
//  - SpecVol and SpecVolDisplaced are [NCellsSize][NVertLayers]; rows 0 .. NCellsAll-1 are computed on every level,
//    whatever the cell's active layer range; the sentinel row NCellsAll is 0 (the reference zero-fills the array
//    before computing it).
//  - Linear:  1 / (RhoT0S0 + (DRhoDT*T + DRhoDS*S)); defaults DRhoDT = -0.2, DRhoDS = 0.8, RhoT0S0 = 1000.
//  - TEOS-10: the 75-term polynomial of Roquet et al. (2015, Ocean Modelling 90, 29-43):
//      ss = sqrt((S + 24) / (40*35.16504/35)), tt = T / 40, pp = p / 1e4 (p in dbar),
//      v = v0(pp) + delta, delta = ((((c5*pp + c4)*pp + c3)*pp + c2)*pp + c1)*pp + c0,
//    with c0 .. c5 polynomials in (ss, tt) in nested form (kernels/ColumnKernels.hip: teos10Coeffs).
//  - Displaced (computeSpecVolDisp): the pressure of level clamp(K + KDisp, 0, NVertLayers-1) of the same cell.
//
// The reference keeps the six pressure coefficients of TEOS-10 in one shared device array (Teos10Eos::SpecVolPCoeffs,
// (6, VecLength)) that every (ICell, KChunk) iteration writes: on a GPU concurrent iterations overwrite each other's
// coefficients.  Here they live in registers, one set per lane and level, which is what the reference computes when
// it runs serially on a host -- that is the result the tests pin.
#ifndef OMEGA_AMD_EOS_H
#define OMEGA_AMD_EOS_H

#include "Base.h"
#include "HorzMesh.h"
#include "kernels/ColumnKernels.h"

namespace OMEGA {

enum class EosType {
   LinearEos, ///< linear equation of state
   Teos10Eos  ///< Roquet et al. 2015, 75-term expansion
};

/// The rows of tracer `Index` of a [NTracers][NCellsSize][NVertLayers] tracer array as a 2-D array (no copy: the
/// view shares the allocation, as a Kokkos subview does)
Array2DReal tracerRows(const Array3DReal &TracerArray, I4 Index);

class Eos : public Registry<Eos> {
 public:
   /// EosTypeStr: "Linear" / "linear" or "teos10" / "teos-10" / "TEOS-10" (Eos.cpp:70-107); anything else is refused.
   Eos(const std::string &Name, const HorzMesh *Mesh, int NVertLayers, const std::string &EosTypeStr = "teos10",
       Real DRhoDT = -0.2, Real DRhoDS = 0.8, Real RhoT0S0 = 1000.0);

   EosType EosChoice;
   Real DRhoDT, DRhoDS, RhoT0S0; ///< LinearEos parameters (Eos.h:247-249)
   Array2DReal SpecVol;          ///< [NCellsSize][NVertLayers]
   Array2DReal SpecVolDisplaced; ///< [NCellsSize][NVertLayers]
   HostArrayReal SpecVolH, SpecVolDisplacedH;

   /// Eos::computeSpecVol (Eos.cpp:113-140).  PScale multiplies the pressure before use (1.0: dbar as given).
   void computeSpecVol(const Array2DReal &ConservTemp, const Array2DReal &AbsSalinity, const Array2DReal &Pressure,
                       Real PScale, hipStream_t S) const;
   /// Eos::computeSpecVolDisp (Eos.cpp:144-176)
   void computeSpecVolDisp(const Array2DReal &ConservTemp, const Array2DReal &AbsSalinity, const Array2DReal &Pressure,
                           I4 KDisp, Real PScale, hipStream_t S) const;
   // ---- the reference's signatures: on this object's `Stream` (default: the null stream), pressure in dbar
   hipStream_t Stream = nullptr;
   void computeSpecVol(const Array2DReal &ConservTemp, const Array2DReal &AbsSalinity,
                       const Array2DReal &Pressure) const {
      computeSpecVol(ConservTemp, AbsSalinity, Pressure, 1.0, Stream);
   }
   void computeSpecVolDisp(const Array2DReal &ConservTemp, const Array2DReal &AbsSalinity, const Array2DReal &Pressure,
                           I4 KDisp) const {
      computeSpecVolDisp(ConservTemp, AbsSalinity, Pressure, KDisp, 1.0, Stream);
   }

   void copyToHost(); ///< SpecVol, SpecVolDisplaced -> the host mirrors
   EosParams params() const;

   const HorzMesh *Mesh;
   std::string Name;
   int NVertLayers;
};

} // namespace OMEGA
#endif
