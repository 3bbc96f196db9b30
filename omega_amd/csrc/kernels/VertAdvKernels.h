// VertAdvKernels.h -- host-callable launchers of the kernels behind VertAdv (kernels/VertAdvKernels.hip).  Asynchronous
// on the given stream, raw device pointers, allocate nothing.  Level-indexed arrays are [rows][Pitch] with
// Pitch = levelPitch(K).  The numerical contract is written down in VertAdv.h.
#ifndef OMEGA_AMD_VERTADVKERNELS_H
#define OMEGA_AMD_VERTADVKERNELS_H

#include "../Base.h"

namespace OMEGA {

/// The column launch: the transport scan (Scan), the thickness update (Thick), or both in one launch.
struct VertAdvColumnArgs {
   int NCellsAll = 0, K = 0;
   const I4 *MinLayerCell = nullptr, *MaxLayerCell = nullptr; ///< [cell]
   const Real *MoveWeights = nullptr;                         ///< [K]
   const Real *RefThick = nullptr;                            ///< [cell][Pitch]
   Real *Tend = nullptr;      ///< [cell][Pitch]: the thickness tendency, read by Scan, updated by Thick
   Real *Transport = nullptr; ///< [cell][Pitch]: written by Scan, read by Thick alone
};
/// columns per workgroup of the column launch at K levels (16, 8, 4 or 2), 0 if K is too long for the LDS tile
int vertAdvColumnTile(int K);
void launchVertAdvColumn(const VertAdvColumnArgs &A, bool Scan, bool Thick, hipStream_t S);

struct VertAdvTracerArgs {
   int NCellsAll = 0, NCellsSize = 0, K = 0, NTracers = 0, Order = 2;
   const I4 *MinLayerCell = nullptr, *MaxLayerCell = nullptr; ///< [cell]
   const Real *Transport = nullptr, *LayerThick = nullptr;    ///< [cell][Pitch]
   const Real *Tracers = nullptr;                             ///< [tracer][NCellsSize][Pitch]
   Real *Tend = nullptr;                                      ///< [tracer][NCellsSize][Pitch], accumulated
};
void launchVertAdvTracer(const VertAdvTracerArgs &A, hipStream_t S);

struct VertAdvEdgeArgs {
   int NEdgesAll = 0, NCellsSize = 0, K = 0;
   const I4 *CellsOnEdge = nullptr;                                 ///< [edge][2]
   const I4 *MinLayerEdgeBot = nullptr, *MaxLayerEdgeTop = nullptr; ///< [edge] level range of the term
   const Real *EdgeMask = nullptr;                                  ///< [edge]
   const Real *Transport = nullptr, *LayerThick = nullptr;          ///< [cell][Pitch]
   const Real *NormalVelocity = nullptr;                            ///< [edge][Pitch]
   Real *Tend = nullptr;                                            ///< [edge][Pitch], accumulated
};
void launchVertAdvEdge(const VertAdvEdgeArgs &A, hipStream_t S);

} // namespace OMEGA
#endif
