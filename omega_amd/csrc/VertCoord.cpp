// VertCoord.cpp -- see VertCoord.h.
#include "VertCoord.h"
#include "Pacer.h"

namespace OMEGA {

VertCoord::VertCoord(const std::string &Name_, const HorzMesh *Mesh_, const Decomp *MeshDecomp, int K, Real Rho0_,
                     const std::string &MoveType, const I4 *MinLevelGlobal, const I4 *MaxLevelGlobal)
    : NVertLayers(K), NVertLayersP1(K + 1), Rho0(Rho0_), MovementWeightType(MoveType), Mesh(Mesh_), Name(Name_) {
   OMEGA_REQUIRE(Mesh != nullptr, "VertCoord: mesh is NULL");
   OMEGA_REQUIRE(K > 0, "VertCoord: NVertLayers must be positive");
   OMEGA_REQUIRE(MoveType == "Fixed" || MoveType == "Uniform",
                 "VertCoord: Unknown MovementWeightType requested: " + MoveType);
   OMEGA_REQUIRE((MinLevelGlobal == nullptr) == (MaxLevelGlobal == nullptr),
                 "VertCoord: give both minLevelCell and maxLevelCell, or neither");
   OMEGA_REQUIRE(!Mesh->HostOnly,
                 "VertCoord: the mesh was created host-only: no device arrays, compute is unavailable");
   // VertCoord::initMovementWeights (VertCoord.cpp:614-650)
   VertCoordMovementWeightsH = HostArrayReal(K);
   for (int I = 0; I < K; ++I)
      VertCoordMovementWeightsH(I) = (MoveType == "Uniform" || I == 0) ? 1.0 : 0.0;

   const int NC = Mesh->NCellsSize, NAll = Mesh->NCellsAll;
   // layer ranges: global 1-based -> local 0-based (VertCoord.cpp:199-206), sentinel cell -1 / -1
   MinLayerCellH = HostArrayI4(NC, 1, 1, -1);
   MaxLayerCellH = HostArrayI4(NC, 1, 1, -1);
   if (MinLevelGlobal) {
      OMEGA_REQUIRE(MeshDecomp != nullptr, "VertCoord: a Decomp is needed to gather minLevelCell / maxLevelCell");
      OMEGA_REQUIRE(MeshDecomp->NCellsAll == NAll, "VertCoord: the Decomp does not match the mesh");
      for (int C = 0; C < NAll; ++C) {
         const I4 G        = MeshDecomp->CellIDH(C) - 1;
         MinLayerCellH(C) = MinLevelGlobal[G] - 1;
         MaxLayerCellH(C) = MaxLevelGlobal[G] - 1;
      }
   } else {
      for (int C = 0; C < NAll; ++C)
         MinLayerCellH(C) = 0, MaxLayerCellH(C) = K - 1;
   }
   MinLayerCell = createDeviceMirrorCopy<I4, 1>("MinLayerCell", MinLayerCellH);
   MaxLayerCell = createDeviceMirrorCopy<I4, 1>("MaxLayerCell", MaxLayerCellH);

   PressureInterface    = Array2DReal::levels("PressureInterface", NC, K + 1);
   PressureMid          = Array2DReal::levels("PressureMid", NC, K);
   ZInterface           = Array2DReal::levels("ZInterface", NC, K + 1);
   ZMid                 = Array2DReal::levels("ZMid", NC, K);
   GeopotentialMid      = Array2DReal::levels("GeopotentialMid", NC, K);
   LayerThicknessTarget = Array2DReal::levels("LayerThicknessTarget", NC, K);
   RefLayerThickness    = Array2DReal::levels("RefLayerThickness", NC, K);
   PressureInterfaceH    = HostArrayReal(NC, K + 1);
   PressureMidH          = HostArrayReal(NC, K);
   ZInterfaceH           = HostArrayReal(NC, K + 1);
   ZMidH                 = HostArrayReal(NC, K);
   GeopotentialMidH      = HostArrayReal(NC, K);
   LayerThicknessTargetH = HostArrayReal(NC, K);
   RefLayerThicknessH    = HostArrayReal(NC, K);
   VertCoordMovementWeights = createDeviceMirrorCopy<Real, 1>("VertCoordMovementWeights", VertCoordMovementWeightsH);
   BottomDepthH = Mesh->BottomDepthH;
   BottomDepth  = createDeviceMirrorCopy<Real, 1>("BottomDepth", BottomDepthH);

   const int NE = Mesh->NEdgesSize, NV = Mesh->NVerticesSize;
   MinLayerEdgeTop   = Array1DI4("MinLayerEdgeTop", NE);
   MaxLayerEdgeTop   = Array1DI4("MaxLayerEdgeTop", NE);
   MinLayerEdgeBot   = Array1DI4("MinLayerEdgeBot", NE);
   MaxLayerEdgeBot   = Array1DI4("MaxLayerEdgeBot", NE);
   MinLayerVertexTop = Array1DI4("MinLayerVertexTop", NV);
   MaxLayerVertexTop = Array1DI4("MaxLayerVertexTop", NV);
   MinLayerVertexBot = Array1DI4("MinLayerVertexBot", NV);
   MaxLayerVertexBot = Array1DI4("MaxLayerVertexBot", NV);
   minMaxLayerEdge(nullptr);
   minMaxLayerVertex(nullptr);
}

static HostArrayI4 mirror(const Array1DI4 &D, hipStream_t S) {
   HIP_CHECK(hipStreamSynchronize(S));
   HostArrayI4 H(D.Ext[0]);
   copyToHost(H.data(), D.Ptr, D.bytes());
   return H;
}

void VertCoord::minMaxLayerEdge(hipStream_t S) {
   launchMinMaxLayer(Mesh->NEdgesAll, 2, Mesh->CellsOnEdge.Ptr, MinLayerCell.Ptr, MaxLayerCell.Ptr, NVertLayers,
                     MinLayerEdgeTop.Ptr, MinLayerEdgeBot.Ptr, MaxLayerEdgeTop.Ptr, MaxLayerEdgeBot.Ptr, S);
   MinLayerEdgeTopH = mirror(MinLayerEdgeTop, S);
   MinLayerEdgeBotH = mirror(MinLayerEdgeBot, S);
   MaxLayerEdgeTopH = mirror(MaxLayerEdgeTop, S);
   MaxLayerEdgeBotH = mirror(MaxLayerEdgeBot, S);
}

void VertCoord::minMaxLayerVertex(hipStream_t S) {
   launchMinMaxLayer(Mesh->NVerticesAll, Mesh->VertexDegree, Mesh->CellsOnVertex.Ptr, MinLayerCell.Ptr,
                     MaxLayerCell.Ptr, NVertLayers, MinLayerVertexTop.Ptr, MinLayerVertexBot.Ptr,
                     MaxLayerVertexTop.Ptr, MaxLayerVertexBot.Ptr, S);
   MinLayerVertexTopH = mirror(MinLayerVertexTop, S);
   MinLayerVertexBotH = mirror(MinLayerVertexBot, S);
   MaxLayerVertexTopH = mirror(MaxLayerVertexTop, S);
   MaxLayerVertexBotH = mirror(MaxLayerVertexBot, S);
}

ColumnArgs VertCoord::baseArgs() const {
   ColumnArgs A;
   A.NCells   = Mesh->NCellsAll;
   A.K        = NVertLayers;
   A.Pitch    = levelPitch(NVertLayers);
   A.Pitch1   = levelPitch(NVertLayers + 1);
   A.MinLayer = MinLayerCell.Ptr;
   A.MaxLayer = MaxLayerCell.Ptr;
   A.Gravity  = Gravity;
   A.Rho0     = Rho0;
   return A;
}

static void requireCells(const Array1DReal &A, const HorzMesh *M, const char *What) {
   OMEGA_REQUIRE(A.Ptr == nullptr || A.Ext[0] >= M->NCellsAll,
                 std::string("VertCoord: ") + What + " must hold NCellsAll values (or be empty: zero)");
}

void VertCoord::computePressure(const Array2DReal &H, const Array1DReal &Ps, hipStream_t S) {
   requireLevelArray("VertCoord", H, Mesh->NCellsAll, NVertLayers, "LayerThickness", "NCellsSize");
   requireCells(Ps, Mesh, "SurfacePressure");
   Pacer::Range Timer("VertCoord:computePressure", 1);
   ColumnArgs A     = baseArgs();
   A.LayerThick     = H.Ptr;
   A.SurfPressure   = Ps.Ptr;
   A.PInt           = PressureInterface.Ptr;
   A.PMid           = PressureMid.Ptr;
   launchColumn(StagePressure, A, S);
}

void VertCoord::computeZHeight(const Array2DReal &H, const Array2DReal &SpecVol, hipStream_t S) {
   requireLevelArray("VertCoord", H, Mesh->NCellsAll, NVertLayers, "LayerThickness", "NCellsSize");
   requireLevelArray("VertCoord", SpecVol, Mesh->NCellsAll, NVertLayers, "SpecVol", "NCellsSize");
   Pacer::Range Timer("VertCoord:computeZHeight", 1);
   ColumnArgs A  = baseArgs();
   A.LayerThick  = H.Ptr;
   A.SpecVolIn   = SpecVol.Ptr;
   A.BottomDepth = BottomDepth.Ptr;
   A.ZInt        = ZInterface.Ptr;
   A.ZMid        = ZMid.Ptr;
   launchColumn(StageZHeight, A, S);
}

void VertCoord::computeGeopotential(const Array1DReal &Tidal, const Array1DReal &SAL, hipStream_t S) {
   requireCells(Tidal, Mesh, "TidalPotential");
   requireCells(SAL, Mesh, "SelfAttractionLoading");
   Pacer::Range Timer("VertCoord:computeGeopotential", 1);
   ColumnArgs A = baseArgs();
   A.ZMidIn     = ZMid.Ptr;
   A.Tidal      = Tidal.Ptr;
   A.SAL        = SAL.Ptr;
   A.GeoMid     = GeopotentialMid.Ptr;
   launchColumn(StageGeopotential, A, S);
}

void VertCoord::computeTargetThickness(hipStream_t S) {
   Pacer::Range Timer("VertCoord:computeTargetThickness", 1);
   ColumnArgs A  = baseArgs();
   A.PIntIn      = PressureInterface.Ptr;
   A.RefThick    = RefLayerThickness.Ptr;
   A.MoveWeights = VertCoordMovementWeights.Ptr;
   A.Target      = LayerThicknessTarget.Ptr;
   launchColumn(StageTargetThickness, A, S);
}

void VertCoord::computeColumn(const OceanState *State, int ThickLevel, const TracerStore *Tracers, int TrLevel,
                              const Eos &EqState, const Array1DReal &Ps, const Array1DReal &Tidal,
                              const Array1DReal &SAL, bool Displaced, I4 KDisp, hipStream_t S, I4 TIndex, I4 SIndex) {
   OMEGA_REQUIRE(State != nullptr && Tracers != nullptr, "VertCoord::computeColumn: state or tracers is NULL");
   OMEGA_REQUIRE(EqState.Mesh == Mesh && EqState.NVertLayers == NVertLayers,
                 "VertCoord::computeColumn: the Eos was built for another mesh or layer count");
   Array2DReal H;
   OMEGA_REQUIRE(State->getLayerThickness(H, ThickLevel) == 0, "VertCoord::computeColumn: bad thickness time level");
   Array3DReal Tr;
   OMEGA_REQUIRE(Tracers->getAll(Tr, TrLevel) == 0, "VertCoord::computeColumn: bad tracer time level");
   computeColumn(H, Tr, EqState, Ps, Tidal, SAL, Displaced, KDisp, S, TIndex, SIndex);
}

void VertCoord::computeColumn(const Array2DReal &H, const Array3DReal &Tr, const Eos &EqState, const Array1DReal &Ps,
                              const Array1DReal &Tidal, const Array1DReal &SAL, bool Displaced, I4 KDisp, hipStream_t S,
                              I4 TIndex, I4 SIndex) {
   OMEGA_REQUIRE(EqState.Mesh == Mesh && EqState.NVertLayers == NVertLayers,
                 "VertCoord::computeColumn: the Eos was built for another mesh or layer count");
   OMEGA_REQUIRE(Tr.Ptr != nullptr, "VertCoord::computeColumn: the tracer array is empty");
   const Array2DReal T = tracerRows(Tr, TIndex), Sa = tracerRows(Tr, SIndex);
   requireLevelArray("VertCoord", H, Mesh->NCellsAll, NVertLayers, "LayerThickness", "NCellsSize");
   requireLevelArray("VertCoord", T, Mesh->NCellsAll, NVertLayers, "tracer rows", "NCellsSize");
   requireCells(Ps, Mesh, "SurfacePressure");
   requireCells(Tidal, Mesh, "TidalPotential");
   requireCells(SAL, Mesh, "SelfAttractionLoading");
   Pacer::Range Timer("VertCoord:computeColumn", 1);
   ColumnArgs A    = baseArgs();
   A.LayerThick    = H.Ptr;
   A.ConservTemp   = T.Ptr;
   A.AbsSalinity   = Sa.Ptr;
   A.PScale        = 1.0e-4; // Pa -> dbar (VertCoord.h)
   A.KDisp         = KDisp;
   A.SurfPressure  = Ps.Ptr;
   A.Tidal         = Tidal.Ptr;
   A.SAL           = SAL.Ptr;
   A.BottomDepth   = BottomDepth.Ptr;
   A.Eos           = EqState.params();
   A.PInt          = PressureInterface.Ptr;
   A.PMid          = PressureMid.Ptr;
   A.SpecVol       = EqState.SpecVol.Ptr;
   A.SpecVolDisp   = Displaced ? EqState.SpecVolDisplaced.Ptr : nullptr;
   A.ZInt          = ZInterface.Ptr;
   A.ZMid          = ZMid.Ptr;
   A.GeoMid        = GeopotentialMid.Ptr;
   unsigned Mask   = StagePressure | StageSpecVol | StageZHeight | StageGeopotential;
   if (Displaced)
      Mask |= StageSpecVolDisp;
   launchColumn(Mask, A, S);
}

void VertCoord::copyToHost() {
   HIP_CHECK(hipDeviceSynchronize());
   OMEGA::copyToHost(PressureInterfaceH.data(), PressureInterface);
   OMEGA::copyToHost(PressureMidH.data(), PressureMid);
   OMEGA::copyToHost(ZInterfaceH.data(), ZInterface);
   OMEGA::copyToHost(ZMidH.data(), ZMid);
   OMEGA::copyToHost(GeopotentialMidH.data(), GeopotentialMid);
   OMEGA::copyToHost(LayerThicknessTargetH.data(), LayerThicknessTarget);
   OMEGA::copyToHost(RefLayerThicknessH.data(), RefLayerThickness);
}

void VertCoord::copyToDevice() {
   OMEGA::copyToDevice(PressureInterface, PressureInterfaceH.data());
   OMEGA::copyToDevice(PressureMid, PressureMidH.data());
   OMEGA::copyToDevice(ZInterface, ZInterfaceH.data());
   OMEGA::copyToDevice(ZMid, ZMidH.data());
   OMEGA::copyToDevice(GeopotentialMid, GeopotentialMidH.data());
   OMEGA::copyToDevice(LayerThicknessTarget, LayerThicknessTargetH.data());
   OMEGA::copyToDevice(RefLayerThickness, RefLayerThicknessH.data());
}

} // namespace OMEGA
