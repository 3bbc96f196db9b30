// GentMcWilliams.cpp -- see GentMcWilliams.h.
#include "GentMcWilliams.h"
#include "Pacer.h"
#include "kernels/GMKernels.h"

#include <cmath>
#include <vector>

namespace OMEGA {

GentMcWilliams::GentMcWilliams(const std::string &Name_, const HorzMesh *Mesh_, VertCoord *VCoord_, Eos *EqState_,
                               Real GMKappa_, Real GravWaveSpeed_)
    : ColumnPass(Mesh_, VCoord_, EqState_), GMKappa(GMKappa_), GravWaveSpeed(GravWaveSpeed_), Name(Name_) {
   OMEGA_REQUIRE(Mesh != nullptr, "GentMcWilliams: mesh is NULL");
   OMEGA_REQUIRE(std::isfinite(GMKappa) && GMKappa >= 0.0,
                 "GentMcWilliams: GMKappa = " + std::to_string(GMKappa) + " is negative or not finite");
   OMEGA_REQUIRE(std::isfinite(GravWaveSpeed) && GravWaveSpeed > 0.0,
                 "GentMcWilliams: GravWaveSpeed = " + std::to_string(GravWaveSpeed) + " is not finite or not positive");
   requireFits("GentMcWilliams");
   requirePackedLayers("GentMcWilliams", NVertLayers);
   Kappa          = Array1DReal("Kappa", Mesh->NEdgesSize);
   BolusVelocity  = Array2DReal::levels("BolusVelocity", Mesh->NEdgesSize, NVertLayers);
   StreamFunction = Array2DReal::levels("StreamFunction", Mesh->NEdgesSize, NVertLayers);
   allocateForcing();
   const std::vector<Real> Fill((size_t)Mesh->NEdgesSize, GMKappa);
   copyToDevice(Kappa, Fill.data());
}

void GentMcWilliams::computeBolusVelocity(const Array2DReal &H, const Array2DReal &SpecVol, const Array2DReal &SpecVolDisp,
                                          const Array2DReal &ZMid, const Array2DReal &Transport, hipStream_t S) const {
   GMArgs A;
   stratificationArgs("GentMcWilliams", A, H, SpecVol, SpecVolDisp, ZMid);
   if (Transport.Ptr != nullptr)
      requireLevelArray("GentMcWilliams", Transport, Mesh->NEdgesSize, NVertLayers, "Transport");
   Pacer::Range Timer("GentMcWilliams:computeBolusVelocity", 1);
   A.Kappa = Kappa.Ptr, A.C2 = GravWaveSpeed * GravWaveSpeed;
   A.LayerThickness = H.Ptr;
   A.BolusVelocity = BolusVelocity.Ptr, A.StreamFunction = StreamFunction.Ptr;
   A.Transport = Transport.Ptr;
   launchBolusVelocity(A, S);
}

void GentMcWilliams::computeBolusVelocity(const Array2DReal &H, const Array2DReal &Transport, hipStream_t S) const {
   computeBolusVelocity(H, EqState->SpecVol, EqState->SpecVolDisplaced, VCoord->ZMid, Transport, S);
}

} // namespace OMEGA
