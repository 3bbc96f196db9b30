// Tendencies.h -- RHS tendencies of layer thickness, normal velocity and tracers.
// Interface after the reference (components/omega/src/ocn/Tendencies.h:73-144;
// Tendencies.cpp:217-600).  Every compute method exists in two forms: the native one takes the HIP
// stream (the `TimeInstant` of the reference is only forwarded to the custom-tendency hooks,
// Tendencies.cpp:288-293: here `ModelTime` seconds, set by the time steppers for every stage), and
// the REFERENCE'S OWN SIGNATURE (..., TimeInstant Time), which sets ModelTime from the instant and
// runs on the object's `Stream` -- a reference call site compiles unchanged.
#ifndef OMEGA_AMD_TENDENCIES_H
#define OMEGA_AMD_TENDENCIES_H

#include "AuxiliaryState.h"
#include "Base.h"
#include "GraphCache.h"
#include "TimeMgr.h"
#include "kernels/Kernels.h"

#include <functional>
#include <type_traits>

namespace OMEGA {

class PressureGrad;
class VertAdv;

/// A custom tendency hook (Tendencies.h:51-53): holds a callable of EITHER form --
///   native:     void(const Array2DReal &Tend, const OceanState *, const AuxiliaryState *, int ThickLvl, int VelLvl,
///                    R8 ModelTimeSeconds, hipStream_t S)                  (launch on S)
///   reference:  void(Array2DReal Tend, const OceanState *, const AuxiliaryState *, int ThickLvl, int VelLvl, TimeInstant Time)
/// A reference-form hook knows no stream: its work goes to the null stream as in the reference; when the tendencies run
/// on another stream the adapter orders the two by host synchronisation before and after the call.
class CustomTendencyType {
 public:
   using Native = std::function<void(const Array2DReal &, const OceanState *, const AuxiliaryState *, int, int, R8, hipStream_t)>;
   CustomTendencyType() = default;
   CustomTendencyType(std::nullptr_t) {}
   template <class C, std::enable_if_t<std::is_invocable_v<C &, const Array2DReal &, const OceanState *, const AuxiliaryState *,
                                                           int, int, R8, hipStream_t>, int> = 0>
   CustomTendencyType(C F_) : F(std::move(F_)) {}
   template <class C, std::enable_if_t<!std::is_invocable_v<C &, const Array2DReal &, const OceanState *, const AuxiliaryState *,
                                                            int, int, R8, hipStream_t> &&
                                           std::is_invocable_v<C &, Array2DReal, const OceanState *, const AuxiliaryState *, int,
                                                               int, TimeInstant>, int> = 0>
   CustomTendencyType(C G)
       : F([G](const Array2DReal &Tend, const OceanState *St, const AuxiliaryState *Aux, int ThickLvl, int VelLvl, R8 Seconds,
               hipStream_t S) mutable {
            if (S)
               HIP_CHECK(hipStreamSynchronize(S));
            G(Tend, St, Aux, ThickLvl, VelLvl, TimeInstant::fromSeconds(Seconds));
            if (S)
               HIP_CHECK(hipStreamSynchronize(nullptr));
         }) {}
   explicit operator bool() const { return (bool)F; }
   void operator()(const Array2DReal &Tend, const OceanState *St, const AuxiliaryState *Aux, int ThickLvl, int VelLvl, R8 Seconds,
                   hipStream_t S) const {
      F(Tend, St, Aux, ThickLvl, VelLvl, Seconds, S);
   }

 private:
   Native F;
};

class Tendencies : public Registry<Tendencies> {
 public:
   /// Fails (OmegaError naming the limit) when the mesh is outside the fused RHS -- an array plane of 4 GiB or more
   /// (32-bit buffer offsets: ~ 2.2 M cells x 80 levels PER RANK; several ranks may share a GPU) or MaxEdges outside
   /// 5..8 -- unless AllowReferenceStructured: then computeAllTendencies takes the reference-structured 23-launch path
   /// (~ 5 x the time) for good, a decision of the caller's instead of a surprise.
   Tendencies(const std::string &Name, const HorzMesh *Mesh, int NVertLayers, int NTracers, const TendParams &Options,
              bool AllowReferenceStructured = false);
   /// the test behind it, on sizes alone (no mesh, no device): "" if the fused RHS covers them, else the reason
   static std::string fusedLimit(size_t NCellsSize, size_t NEdgesSize, size_t NVerticesSize, int MaxEdges, int NVertLayers);

   Array2DReal LayerThicknessTend; ///< (NCellsSize, NVertLayers)
   Array2DReal NormalVelocityTend; ///< (NEdgesSize, NVertLayers)
   Array3DReal TracerTend;         ///< (NTracers, NCellsSize, NVertLayers)

   TendParams Params; ///< enable flags and coefficients (readTendConfig)
   /// Fused RHS for computeAllTendencies (default on); off = the reference's launch
   /// structure (every AuxiliaryState array materialised).
   bool UseFusedRHS = true;
   /// Replay the fused RHS as a HIP graph when it is called again with the same arrays on a non-default stream
   /// (GraphCache.h): one host call instead of 7 launches.  Default off (no gain measured); never used while
   /// kernel timing or custom tendencies are on.
   bool UseGraphs = false;
   GraphCache Graphs;
   /// the object's switch, or the option Graphs = 1 (read when asked, not when the object was made)
   bool graphsOn() const { return UseGraphs || GraphCache::defaultOn(); }

   /// Custom tendencies (Tendencies.h:51-53, 182-183): called at the end of the thickness / velocity
   /// group with the tendency array, the state / aux state, the two time levels and the model time
   /// (native form: ModelTime seconds + the stream; or the reference's form with a TimeInstant).
   using CustomTendencyType = OMEGA::CustomTendencyType;
   CustomTendencyType CustomThicknessTend, CustomVelocityTend;
   /// model time handed to the custom tendencies; the time steppers set it for every stage
   /// (RungeKutta4Stepper.cpp:87 StageTime, RungeKutta2Stepper.cpp:44,58, ForwardBackwardStepper.cpp:50,59,67)
   R8 ModelTime = 0.0;

   /// The layered-ocean pressure-gradient force (PressureGrad.h) as an opt-in velocity term; nullptr detaches.  Refused
   /// (OmegaError) while Params.SSHTendencyEnable is on -- two pressure forces must be a visible mistake -- and for an
   /// object of another mesh or layer count.  While attached:
   ///  - computeAllTendencies runs the column pass (PressureGrad::updateColumn) on the stage's layer thickness and the
   ///    TracerArray argument (tracer 0 = temperature, 1 = salinity), then subtracts the term from NormalVelocityTend
   ///    after the built-in velocity terms and before CustomVelocityTend, all on the same stream;
   ///  - computeVelocityTendenciesOnly / computeVelocityTendencies take no tracers: they add the term from the column
   ///    fields AS THEY STAND (the last updateColumn / VertCoord::computeColumn) -- the caller keeps them current;
   ///  - computeAllTendenciesStage returns false, as with custom hooks (the Runge-Kutta stage updates then run as
   ///    separate kernels), and the RHS is not replayed as a graph.
   /// With nothing attached every code path, launch count and result is what it was.
   void attachPressureGrad(PressureGrad *PGrad);
   PressureGrad *pressureGrad() const { return PGrad; }

   /// Vertical transport and vertical advection (VertAdv.h) as opt-in terms of all three tendencies; nullptr detaches.
   /// Refused (OmegaError) for an object of another mesh or layer count.  While attached:
   ///  - computeAllTendencies runs the existing RHS unchanged, then VertAdv::computeAndAddThickness on
   ///    LayerThicknessTend, addTracerTend with the stage's layer thickness and the TracerArray argument, and
   ///    addVelocityTend with the stage's thickness and velocity, all on the same stream, BEFORE an attached
   ///    PressureGrad and before both custom hooks: the transport is derived from the built-in thickness terms only,
   ///    not from what CustomThicknessTend adds;
   ///  - computeThicknessTendencies / ...Only do the thickness part (transport included) after the built-in terms and
   ///    before CustomThicknessTend;
   ///  - the velocity and tracer group methods add their term from VerticalTransport AS IT STANDS (the last thickness
   ///    evaluation) -- the caller keeps it current; the Forward-Backward stepper calls the thickness group first;
   ///  - computeAllTendenciesStage returns false (the Runge-Kutta stage updates then run as separate kernels), and
   ///    the RHS is not replayed as a graph.
   /// With nothing attached every code path, launch count, allocation and result is what it was.
   void attachVertAdv(VertAdv *VAdv);
   VertAdv *vertAdv() const { return VAdv; }

   /// Does anything add terms to the stored tendencies after the fused RHS (a custom hook, an attached PressureGrad or
   /// VertAdv)?  Then the stage-fused form does not apply and neither the RHS nor a step is replayed as a graph.  A new
   /// attachable term goes here.
   bool addsTermsAfterFusedRHS() const { return CustomThicknessTend || CustomVelocityTend || PGrad || VAdv; }

   void computeThicknessTendenciesOnly(const OceanState *State, const AuxiliaryState *AuxState, int ThickTimeLevel,
                                       int VelTimeLevel, hipStream_t S);
   void computeVelocityTendenciesOnly(const OceanState *State, const AuxiliaryState *AuxState, int ThickTimeLevel,
                                      int VelTimeLevel, hipStream_t S);
   void computeTracerTendenciesOnly(const OceanState *State, const AuxiliaryState *AuxState,
                                    const Array3DReal &TracerArray, int ThickTimeLevel, int VelTimeLevel,
                                    hipStream_t S);
   void computeThicknessTendencies(const OceanState *State, const AuxiliaryState *AuxState, int ThickTimeLevel,
                                   int VelTimeLevel, hipStream_t S);
   void computeVelocityTendencies(const OceanState *State, const AuxiliaryState *AuxState, int ThickTimeLevel,
                                  int VelTimeLevel, hipStream_t S);
   void computeTracerTendencies(const OceanState *State, const AuxiliaryState *AuxState,
                                const Array3DReal &TracerArray, int ThickTimeLevel, int VelTimeLevel, hipStream_t S);
   /// The transport half of the RHS -- thickness and tracer tendencies, with the velocity taken from a time level of
   /// the caller's choice (the Split-Explicit step passes the transporting velocity) -- in two launches instead of the
   /// five of the two group methods (kernels/TransportKernels.hip).  This library's own call:
   /// the reference has none.
   ///
   /// Contract: on every row < NCellsAll (halo included) LayerThicknessTend and TracerTend hold, BIT FOR BIT, what
   ///    computeThicknessTendencies(State, AuxState, ThickTimeLevel, VelTimeLevel, S);
   ///    computeTracerTendencies(State, AuxState, TracerArray, ThickTimeLevel, VelTimeLevel, S);
   /// leave there, attached terms included, in their documented order: the built-in thickness terms, an attached
   /// VertAdv's computeAndAddThickness, the built-in tracer terms, then VertAdv::addTracerTend with the transport just
   /// computed.  Nothing else of the tendency arrays is written: not the row padding, not the sentinel row, not
   /// NormalVelocityTend.  With no tracers the thickness tendency alone is computed.
   ///
   /// Deviation from the two group methods: the edge-located auxiliary arrays FluxLayerThickEdge, MeanLayerThickEdge
   /// and HTracersEdge are NOT materialised (as with the fused RHS: each cell recomputes the values of its own edges in
   /// registers), and Del2TracersCell is written only when Params.TracerHyperDiffTendencyEnable is set (the group
   /// method writes it always).
   ///
   /// Always valid: with a CustomThicknessTend hook installed -- it is handed the AuxiliaryState and may read those
   /// arrays -- the call runs the two group methods instead.  A time level out of range is refused with their error.
   void computeTransportTendencies(const OceanState *State, const AuxiliaryState *AuxState, const Array3DReal &TracerArray,
                                   int ThickTimeLevel, int VelTimeLevel, hipStream_t S);
   /// computeTransportTendencies with the thickness and tracer updates that follow it in a step folded into the
   /// epilogues of its two kernels: the tendencies go from the registers into the new values instead of making a round
   /// trip through HBM for the two streaming update kernels.  This library's own call.
   ///
   /// Contract: on every row < NCellsAll (halo included) and every level < NVertLayers, NextThick and NextTracers hold,
   /// BIT FOR BIT, what this sequence leaves there (Cur = the thickness of ThickTimeLevel and TracerArray):
   ///    computeTransportTendencies(State, AuxState, TracerArray, ThickTimeLevel, VelTimeLevel, S);
   ///    NextThick   = CurThick + Coeff*LayerThicknessTend                       (launchUpdateByTend)
   ///    NextTracers = (CurTracers*CurThick + Coeff*TracerTend)/NextThick        (launchUpdateTracersByTend)
   /// With KeepTendencies, LayerThicknessTend and TracerTend hold what computeTransportTendencies leaves.  Without it
   /// their contents on those rows are unspecified (the stores are skipped where no later kernel reads them).  Nothing
   /// outside those rows is written either way: not the row padding, not the sentinel row, not NormalVelocityTend.
   ///
   /// Deviation from the sequence: the LEVEL PADDING of NextThick and NextTracers (levels NVertLayers .. pitch-1) is
   /// NOT written.  The streaming kernels sweep whole rows and leave Cur's padding plus garbage there; nobody reads it.
   /// Del2TracersCell is written as by computeTransportTendencies.
   ///
   /// Always valid: with a VertAdv attached (it adds its terms to the stored tendencies after the kernels), with a
   /// CustomThicknessTend hook installed, or when an output aliases an input (NextThick is the thickness of
   /// ThickTimeLevel, or NextTracers is TracerArray: neighbouring cells still gather the inputs) the call runs the
   /// sequence above as written, level padding included.  NextThick and NextTracers must have the shape of the
   /// thickness and of TracerArray.  A time level out of range is refused with computeTransportTendencies' error.
   void computeTransportTendenciesAndUpdate(const OceanState *State, const AuxiliaryState *AuxState,
                                            const Array3DReal &TracerArray, int ThickTimeLevel, int VelTimeLevel,
                                            const Array2DReal &NextThick, const Array3DReal &NextTracers, R8 Coeff,
                                            bool KeepTendencies, hipStream_t S);
   /// The momentum half of the RHS: the fused RHS called without tracers, for a caller that computes the transport
   /// half elsewhere (the Split-Explicit step keeps only NormalVelocityTend of its first evaluation; DESIGN.md section
   /// 4.9).  This library's own call: the reference has none.
   ///
   /// Contract: on every row < NEdgesAll NormalVelocityTend holds, BIT FOR BIT, what
   ///    computeAllTendencies(State, AuxState, TracerArray, ThickTimeLevel, VelTimeLevel, S);
   /// leaves there, and so does LayerThicknessTend on every row < NCellsAll, attached terms included: an attached
   /// PressureGrad gets its column pass on TracerArray (the only use of TracerArray) and its term, an attached VertAdv
   /// its computeAndAddThickness and addVelocityTend.  LayerThicknessTend is not waste: the VertAdv derives its
   /// VerticalTransport from it.  TracerTend and Del2TracersCell are NOT written, and nothing else of the tendency
   /// arrays is: not the row padding, not the sentinel rows.  No graph replay and no kernel-timing events.
   ///
   /// Always valid: with a custom hook installed (either one), with UseFusedRHS off or on a mesh outside the fused RHS
   /// the call runs computeAllTendencies -- TracerTend (and the auxiliary state) is then written too.  A time level out
   /// of range is refused with computeAllTendencies' error.
   void computeMomentumTendencies(const OceanState *State, const AuxiliaryState *AuxState, const Array3DReal &TracerArray,
                                  int ThickTimeLevel, int VelTimeLevel, hipStream_t S);
   /// computeAllTendencies with a Runge-Kutta stage update folded into the kernels that produce the
   /// tendencies (kernels/Kernels.h: StageUpdate).  Returns false -- nothing launched -- when the
   /// stage-fused kernels do not cover this mesh / option set; the caller then uses the plain sequence.
   bool computeAllTendenciesStage(const OceanState *State, const AuxiliaryState *AuxState, const Array3DReal &TracerArray,
                                  int ThickTimeLevel, int VelTimeLevel, const StageUpdate &Stage, hipStream_t S);
   void computeAllTendencies(const OceanState *State, const AuxiliaryState *AuxState, const Array3DReal &TracerArray,
                             int ThickTimeLevel, int VelTimeLevel, hipStream_t S);

   // ---- the reference's signatures (Tendencies.h:73-102): ModelTime <- Time, launches on `Stream`
   hipStream_t Stream = nullptr; ///< stream of the reference-signature methods (default: the null stream, as Kokkos')
   void computeThicknessTendencies(const OceanState *State, const AuxiliaryState *AuxState, int ThickTimeLevel,
                                   int VelTimeLevel, TimeInstant Time) {
      ModelTime = Time.getSeconds();
      computeThicknessTendencies(State, AuxState, ThickTimeLevel, VelTimeLevel, Stream);
   }
   void computeVelocityTendencies(const OceanState *State, const AuxiliaryState *AuxState, int ThickTimeLevel,
                                  int VelTimeLevel, TimeInstant Time) {
      ModelTime = Time.getSeconds();
      computeVelocityTendencies(State, AuxState, ThickTimeLevel, VelTimeLevel, Stream);
   }
   void computeTracerTendencies(const OceanState *State, const AuxiliaryState *AuxState, const Array3DReal &TracerArray,
                                int ThickTimeLevel, int VelTimeLevel, TimeInstant Time) {
      ModelTime = Time.getSeconds();
      computeTracerTendencies(State, AuxState, TracerArray, ThickTimeLevel, VelTimeLevel, Stream);
   }
   void computeAllTendencies(const OceanState *State, const AuxiliaryState *AuxState, const Array3DReal &TracerArray,
                             int ThickTimeLevel, int VelTimeLevel, TimeInstant Time) {
      ModelTime = Time.getSeconds();
      computeAllTendencies(State, AuxState, TracerArray, ThickTimeLevel, VelTimeLevel, Stream);
   }
   void computeTransportTendencies(const OceanState *State, const AuxiliaryState *AuxState, const Array3DReal &TracerArray,
                                   int ThickTimeLevel, int VelTimeLevel, TimeInstant Time) {
      ModelTime = Time.getSeconds();
      computeTransportTendencies(State, AuxState, TracerArray, ThickTimeLevel, VelTimeLevel, Stream);
   }
   void computeTransportTendenciesAndUpdate(const OceanState *State, const AuxiliaryState *AuxState,
                                            const Array3DReal &TracerArray, int ThickTimeLevel, int VelTimeLevel,
                                            const Array2DReal &NextThick, const Array3DReal &NextTracers, R8 Coeff,
                                            bool KeepTendencies, TimeInstant Time) {
      ModelTime = Time.getSeconds();
      computeTransportTendenciesAndUpdate(State, AuxState, TracerArray, ThickTimeLevel, VelTimeLevel, NextThick, NextTracers,
                                          Coeff, KeepTendencies, Stream);
   }
   void computeMomentumTendencies(const OceanState *State, const AuxiliaryState *AuxState, const Array3DReal &TracerArray,
                                  int ThickTimeLevel, int VelTimeLevel, TimeInstant Time) {
      ModelTime = Time.getSeconds();
      computeMomentumTendencies(State, AuxState, TracerArray, ThickTimeLevel, VelTimeLevel, Stream);
   }
   void computeThicknessTendenciesOnly(const OceanState *State, const AuxiliaryState *AuxState, int ThickTimeLevel,
                                       int VelTimeLevel, TimeInstant Time) {
      ModelTime = Time.getSeconds();
      computeThicknessTendenciesOnly(State, AuxState, ThickTimeLevel, VelTimeLevel, Stream);
   }
   void computeVelocityTendenciesOnly(const OceanState *State, const AuxiliaryState *AuxState, int ThickTimeLevel,
                                      int VelTimeLevel, TimeInstant Time) {
      ModelTime = Time.getSeconds();
      computeVelocityTendenciesOnly(State, AuxState, ThickTimeLevel, VelTimeLevel, Stream);
   }
   void computeTracerTendenciesOnly(const OceanState *State, const AuxiliaryState *AuxState, const Array3DReal &TracerArray,
                                    int ThickTimeLevel, int VelTimeLevel, TimeInstant Time) {
      ModelTime = Time.getSeconds();
      computeTracerTendenciesOnly(State, AuxState, TracerArray, ThickTimeLevel, VelTimeLevel, Stream);
   }

   /// Per-kernel timing of the fused RHS with HIP events on the launch stream (bench.py's
   /// roofline leg): while enabled every computeAllTendencies call records 7 events.
   void enableKernelTiming(bool On);
   /// Sum of the recorded durations per kernel [FusedNumKernels] in ms and the number of
   /// recorded RHS evaluations; synchronises, then clears the recordings.
   int collectKernelTimes(double *MsSum);
   ~Tendencies();

   const HorzMesh *Mesh;
   int NVertLayers, NTracers;
   /// The fused RHS never materialises the edge-located auxiliary arrays; custom tendency hooks receive the
   /// AuxiliaryState and may read it (reference: computeAllTendencies computes the auxiliary state first,
   /// Tendencies.cpp:591): with this on (default) AuxiliaryState::computeAll runs before the hooks are called.
   bool MaterialiseAuxForCustom = true;

 private:
   PressureGrad *PGrad = nullptr;
   VertAdv *VAdv       = nullptr;
   void addPressureGrad(hipStream_t S); ///< NormalVelocityTend -= the attached term, from the column fields as they stand
   Array2DReal EdgeScratch; ///< running PV sums of the fused RHS (allocated by the constructor)
   bool TimingOn = false;
   std::vector<std::vector<hipEvent_t>> TimingEvents;
   /// AuxiliaryState options are read by AuxiliaryState::readConfigOptions in the reference;
   /// the kernels take them through TendParams, so sync them from the AuxState in use.
   TendParams paramsFor(const AuxiliaryState *AuxState) const;
};

} // namespace OMEGA
#endif
