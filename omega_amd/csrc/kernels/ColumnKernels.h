// ColumnKernels.h -- host-callable launchers of the vertical-column kernels behind VertCoord and Eos
// (kernels/ColumnKernels.hip).  Every launcher is asynchronous on the given stream and takes raw device pointers.
// The numerical contract is written down in VertCoord.h and Eos.h.
#ifndef OMEGA_AMD_COLUMNKERNELS_H
#define OMEGA_AMD_COLUMNKERNELS_H

#include "../Base.h"

namespace OMEGA {

/// Stages of the column kernel (one template over a compile-time mask of these).  Pressure, ZHeight and
/// TargetThickness are sequential per column; SpecVol, SpecVolDisp and Geopotential are point-wise.
enum ColumnStage : unsigned {
   StagePressure        = 1u << 0, ///< VertCoord::computePressure
   StageSpecVol         = 1u << 1, ///< Eos::computeSpecVol
   StageSpecVolDisp     = 1u << 2, ///< Eos::computeSpecVolDisp
   StageZHeight         = 1u << 3, ///< VertCoord::computeZHeight
   StageGeopotential    = 1u << 4, ///< VertCoord::computeGeopotential
   StageTargetThickness = 1u << 5, ///< VertCoord::computeTargetThickness
};

/// Equation of state parameters as the column kernel sees them.
struct EosParams {
   int Teos10     = 1;    ///< 1: TEOS-10 (Roquet et al. 2015), 0: linear
   Real DRhoDT    = -0.2; ///< linear: kg m^-3 degC^-1
   Real DRhoDS    = 0.8;  ///< linear: kg m^-3
   Real RhoT0S0   = 1000.0;
};

/// Everything one column launch reads and writes.  Level-indexed arrays are [cell][Pitch] (Pitch = levelPitch(K)),
/// interface arrays [cell][Pitch1] (Pitch1 = levelPitch(K + 1)).  Pointers a launch's stages do not use may be null;
/// the per-cell scalars Ps / Tidal / SAL read as 0 when null.
struct ColumnArgs {
   int NCells = 0;           ///< columns 0 .. NCells-1 are computed (NCellsAll); row NCells is the sentinel row
   int K = 0, Pitch = 0, Pitch1 = 0;
   const I4 *MinLayer = nullptr, *MaxLayer = nullptr; ///< [cell] 0-based active layer range
   Real Gravity = 0, Rho0 = 0;
   // inputs
   const Real *LayerThick = nullptr;  ///< Pressure, ZHeight
   const Real *ConservTemp = nullptr, *AbsSalinity = nullptr; ///< SpecVol(Disp)
   const Real *PressureIn = nullptr;  ///< SpecVol(Disp) without Pressure in the mask: pressure in dbar after PScale
   Real PScale = 1.0;                 ///< p = Pressure * PScale (1.0: as given; 1.0e-4: PressureMid in Pa -> dbar)
   int KDisp = 0;                     ///< SpecVolDisp: pressure taken at level clamp(K + KDisp, 0, K-1)
   const Real *SpecVolIn = nullptr;   ///< ZHeight without SpecVol in the mask
   const Real *ZMidIn = nullptr;      ///< Geopotential without ZHeight in the mask
   const Real *PIntIn = nullptr;      ///< TargetThickness
   const Real *RefThick = nullptr, *MoveWeights = nullptr; ///< TargetThickness ([cell][Pitch], [K])
   const Real *SurfPressure = nullptr, *Tidal = nullptr, *SAL = nullptr, *BottomDepth = nullptr; ///< [cell]
   EosParams Eos;
   // outputs
   Real *PInt = nullptr, *PMid = nullptr, *SpecVol = nullptr, *SpecVolDisp = nullptr;
   Real *ZInt = nullptr, *ZMid = nullptr, *GeoMid = nullptr, *Target = nullptr;
};

/// One launch of the column kernel for the stage combination `Mask` (the instantiated combinations: each single
/// stage, and Pressure|SpecVol|ZHeight|Geopotential with or without SpecVolDisp).  Fails (OmegaError) for a
/// combination that is not instantiated or a column too long for the LDS tile.
void launchColumn(unsigned Mask, const ColumnArgs &A, hipStream_t S);

/// VertCoord::minMaxLayerEdge / minMaxLayerVertex (VertCoord.cpp:484-610): one thread per edge / vertex over
/// NAll elements with NCellsOn cells each (2, VertexDegree), plus the sentinel row NAll.
void launchMinMaxLayer(int NAll, int NCellsOn, const I4 *CellsOn, const I4 *MinLayerCell, const I4 *MaxLayerCell,
                       int NVertLayers, I4 *MinTop, I4 *MinBot, I4 *MaxTop, I4 *MaxBot, hipStream_t S);

} // namespace OMEGA
#endif
