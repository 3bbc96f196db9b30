// Eos.cpp -- see Eos.h.
#include "Eos.h"

namespace OMEGA {

Array2DReal tracerRows(const Array3DReal &TracerArray, I4 Index) {
   OMEGA_REQUIRE(Index >= 0 && Index < TracerArray.Ext[0], "tracerRows: tracer index out of range");
   Array2DReal V;
   V.Ptr    = TracerArray.Ptr + (size_t)Index * TracerArray.Ext[1] * TracerArray.Pitch;
   V.Ext[0] = TracerArray.Ext[1];
   V.Ext[1] = TracerArray.Ext[2];
   V.Pitch  = TracerArray.Pitch;
   V.Label  = TracerArray.Label;
   V.Buf    = TracerArray.Buf;
   return V;
}

Eos::Eos(const std::string &Name_, const HorzMesh *Mesh_, int K, const std::string &EosTypeStr, Real DRhoDT_,
         Real DRhoDS_, Real RhoT0S0_)
    : DRhoDT(DRhoDT_), DRhoDS(DRhoDS_), RhoT0S0(RhoT0S0_), Mesh(Mesh_), Name(Name_), NVertLayers(K) {
   OMEGA_REQUIRE(Mesh != nullptr, "Eos: mesh is NULL");
   OMEGA_REQUIRE(K > 0, "Eos: NVertLayers must be positive");
   if (EosTypeStr == "Linear" || EosTypeStr == "linear")
      EosChoice = EosType::LinearEos;
   else if (EosTypeStr == "teos10" || EosTypeStr == "teos-10" || EosTypeStr == "TEOS-10")
      EosChoice = EosType::Teos10Eos;
   else
      OMEGA_ABORT("Eos: Unknown EosType requested: " + EosTypeStr);
   OMEGA_REQUIRE(!Mesh->HostOnly, "Eos: the mesh was created host-only: no device arrays, compute is unavailable");
   SpecVol          = Array2DReal::levels("SpecVol", Mesh->NCellsSize, K);
   SpecVolDisplaced = Array2DReal::levels("SpecVolDisplaced", Mesh->NCellsSize, K);
   SpecVolH          = HostArrayReal(Mesh->NCellsSize, K);
   SpecVolDisplacedH = HostArrayReal(Mesh->NCellsSize, K);
}

EosParams Eos::params() const {
   EosParams E;
   E.Teos10  = EosChoice == EosType::Teos10Eos;
   E.DRhoDT  = DRhoDT;
   E.DRhoDS  = DRhoDS;
   E.RhoT0S0 = RhoT0S0;
   return E;
}

void Eos::computeSpecVol(const Array2DReal &Ct, const Array2DReal &Sa, const Array2DReal &P, Real PScale,
                         hipStream_t S) const {
   requireLevelArray("Eos", Ct, Mesh->NCellsAll, NVertLayers, "ConservTemp", "NCellsSize");
   requireLevelArray("Eos", Sa, Mesh->NCellsAll, NVertLayers, "AbsSalinity", "NCellsSize");
   requireLevelArray("Eos", P, Mesh->NCellsAll, NVertLayers, "Pressure", "NCellsSize");
   ColumnArgs A;
   A.NCells = Mesh->NCellsAll, A.K = NVertLayers, A.Pitch = levelPitch(NVertLayers), A.Pitch1 = levelPitch(NVertLayers + 1);
   A.MinLayer = nullptr;
   A.ConservTemp = Ct.Ptr, A.AbsSalinity = Sa.Ptr, A.PressureIn = P.Ptr, A.PScale = PScale;
   A.Eos     = params();
   A.SpecVol = SpecVol.Ptr;
   launchColumn(StageSpecVol, A, S);
}

void Eos::computeSpecVolDisp(const Array2DReal &Ct, const Array2DReal &Sa, const Array2DReal &P, I4 KDisp, Real PScale,
                             hipStream_t S) const {
   requireLevelArray("Eos", Ct, Mesh->NCellsAll, NVertLayers, "ConservTemp", "NCellsSize");
   requireLevelArray("Eos", Sa, Mesh->NCellsAll, NVertLayers, "AbsSalinity", "NCellsSize");
   requireLevelArray("Eos", P, Mesh->NCellsAll, NVertLayers, "Pressure", "NCellsSize");
   ColumnArgs A;
   A.NCells = Mesh->NCellsAll, A.K = NVertLayers, A.Pitch = levelPitch(NVertLayers), A.Pitch1 = levelPitch(NVertLayers + 1);
   A.ConservTemp = Ct.Ptr, A.AbsSalinity = Sa.Ptr, A.PressureIn = P.Ptr, A.PScale = PScale, A.KDisp = KDisp;
   A.Eos         = params();
   A.SpecVolDisp = SpecVolDisplaced.Ptr;
   launchColumn(StageSpecVolDisp, A, S);
}

void Eos::copyToHost() {
   HIP_CHECK(hipDeviceSynchronize());
   OMEGA::copyToHost(SpecVolH.data(), SpecVol);
   OMEGA::copyToHost(SpecVolDisplacedH.data(), SpecVolDisplaced);
}

} // namespace OMEGA
