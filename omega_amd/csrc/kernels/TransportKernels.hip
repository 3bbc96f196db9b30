// TransportKernels.hip -- Tendencies::computeTransportTendencies: the transport half of the RHS (thickness and tracer
// tendencies at a caller-chosen velocity level) in two launches.  The group calls run five (EdgeAux2Body,
// ThickTendBody, TracerEdgeBody, TracerCellBody, TracerTendBody) and pass FluxLayerThickEdge, MeanLayerThickEdge,
// HTracersEdge and Del2TracersCell through HBM; here a cell recomputes the edge values of its own slots in registers
// from CellsOnEdgeOnCell -- the expressions of those bodies, in their left-to-right order, so every bit of the result
// is theirs -- and only Del2TracersCell, which the hyperdiffusion term gathers from NEIGHBOURING cells, makes a round
// trip (and only when that term is enabled).  Compiled with -ffp-contract=off.
//
// Tendencies::computeTransportTendenciesAndUpdate runs the same two bodies with the template parameter Upd non-zero: the
// thickness and tracer updates of TendKernels.hip (UpdateFn, UpdateTracersFn) are then the epilogue of the kernel that
// finishes the tendency, on the register value, in the functors' expressions and operand order.  Both files are compiled
// with the same flags, so the FP64 division is the same instruction sequence in both.  The Upd = 0 / false instantiations
// are the kernels described below, unchanged: the update members live in a base class that is empty for them.
#include "KernelCommon.h"
#include "Kernels.h"

#include <type_traits>

namespace OMEGA {

struct NoUpdate {};
/// what the update epilogue of launch 1 needs beyond the body's own members
struct CellUpdate {
   Real *NextH, *NextTr;
   Real Coeff;
   int Keep; ///< store the tendencies too (LayerThicknessTend; TracerTend where no later launch reads it)
};
/// ... and that of launch 2, which has neither the thicknesses nor the tracers among its own inputs
struct HyperUpdate {
   const Real *H, *Tr, *NextH;
   Real *NextTr;
   Real Coeff;
   int Keep;
};

// ---------------------------------------------------------------------------------------
// Launch 1, one thread per (cell, level chunk): LayerThicknessTend (ThickTendBody with the flux of EdgeAux2Body), per
// tracer Del2TracersCell (TracerCellBody with the mean thickness of EdgeAux2Body) and TracerTend through the advection
// and del2 terms (TracerTendBody with the edge tracer of TracerEdgeBody).
//
// Registers: the edge values of all slots at once (h at both cells and u of 7 slots are 84 VGPRs with dv2) would leave
// nothing for the tracer loop, so nothing is kept per slot.  The tracers go in blocks of TrBlock: one pass over the
// slots loads h at the slot's two cells and u at its edge once and serves the block's tracers from them (7 gathers per
// slot for 2 tracers against 10 one by one); the next block loads them again, from L1/L2 -- the rows were fetched a
// moment ago by this workgroup.  The thickness tendency rides on the first block's pass.  Block 2 is the measured
// optimum at QU30 size with 6 tracers (dv2: 118 VGPRs, 4 waves per SIMD): 1 is 8 % slower, 3 (134 VGPRs, 3 waves) 7 %
// (profiles/EXPERIMENTS.md).
//
// Upd > 0: NextH = Hc + Coeff*TendV (UpdateFn) where the thickness tendency is finished, from the register value, Hc
// being the cell's own thickness.  Upd = 1 is the form for the hyperdiffusion term on: the tracer tendency is finished by
// launch 2, which does the tracer update, so TrTend is stored as ever and nothing is carried (dv2: 125 VGPRs, the 4 waves
// of the plain form).  Upd = 2 is the form for the term off: this launch finishes the tracer tendency too and
// NextTr = (CurTr*Hc + Coeff*TendV)/Hn (UpdateTracersFn) follows it, with Hc and the new Hn kept in registers across the
// tracer blocks (dv2: 147 VGPRs, 3 waves: the FP64 division of a block of two tracers).  LayerThicknessTend, and TrTend
// where launch 2 does not read it, are stored only if Keep is set.
template <int Upd> struct TransportCellBodyT : std::conditional_t<(Upd > 0), CellUpdate, NoUpdate> {
   static constexpr int TrBlock = 2;
   MeshView M;
   int K, NT;
   TendParams P;
   const Real *H, *U, *Tr;
   Real *HTend, *TrTend, *Del2Tr;
   struct Lds {
      Real *DvS, *MDvS, *Df2, *D2C, *InvA;
      int *Edge, *C0, *C1, *N;
   };
   template <class Cv> __host__ __device__ Lds layout(Cv &C, int Tile) const {
      const int ME = M.MaxEdges;
      Lds L;
      L.DvS  = C.template take<Real>(Tile * ME);
      L.MDvS = C.template take<Real>(Tile * ME);
      L.Df2  = C.template take<Real>(Tile * ME);
      L.D2C  = C.template take<Real>(Tile * ME);
      L.InvA = C.template take<Real>(Tile);
      L.Edge = C.template take<int>(Tile * ME);
      L.C0   = C.template take<int>(Tile * ME);
      L.C1   = C.template take<int>(Tile * ME);
      L.N    = C.template take<int>(Tile);
      return L;
   }
   __device__ void stage(const Lds &L, int First, int Cnt, int Tid, int NThr) const {
      const int ME = M.MaxEdges;
      for (int I = Tid; I < Cnt * ME; I += NThr) {
         const size_t G = (size_t)First * ME + I;
         L.DvS[I]       = M.DvSignOnCell[G];
         L.MDvS[I]      = M.MaskDvSignOnCell[G];
         L.Df2[I]       = M.Diff2CoefOnCell[G];
         L.D2C[I]       = M.Del2TrCoefOnCell[G];
         L.Edge[I]      = M.EdgesOnCell[G];
         L.C0[I]        = M.CellsOnEdgeOnCell[2 * G];
         L.C1[I]        = M.CellsOnEdgeOnCell[2 * G + 1];
      }
      for (int I = Tid; I < Cnt; I += NThr) {
         L.N[I]    = M.NEdgesOnCell[First + I];
         L.InvA[I] = M.InvAreaCell[First + I];
      }
   }
   /// one pass over the cell's slots for the tracers [Lt0, Lt0 + NB); Thick: the thickness tendency too.  Hc, Hn: the
   /// cell's own thickness and its new value (Upd = 2 only: the pass with Thick sets Hn, the later ones use it)
   template <class T, int NB>
   __device__ __forceinline__ void pass(const Lds &L, int Le, int ICell, int Kv, int Lt0, bool Thick, const T &Hc, T &Hn) const {
      constexpr int NA     = NB > 0 ? NB : 1;
      const int ME         = M.MaxEdges;
      const int N          = L.N[Le];
      const Real InvA      = L.InvA[Le];
      const size_t CStride = (size_t)M.NCellsSize * K;
      const bool Adv = P.TracerHorzAdvTendencyEnable, Diff = P.TracerDiffTendencyEnable, Hyp = P.TracerHyperDiffTendencyEnable;
      const bool DoFlux = Thick && P.ThicknessFluxTendencyEnable;
      const bool NeedU  = DoFlux || (NB > 0 && Adv);
      T DivTmp = splat<T>(0.0);
      T HAdvTmp[NA], DiffTmp[NA], D2Tmp[NA];
#pragma unroll
      for (int B = 0; B < NA; ++B)
         HAdvTmp[B] = DiffTmp[B] = D2Tmp[B] = splat<T>(0.0);
      for (int J = 0; J < N; ++J) {
         const int C0 = L.C0[Le * ME + J], C1 = L.C1[Le * ME + J];
         const T H0 = ldk<T>(H, C0, K, Kv), H1 = ldk<T>(H, C1, K, Kv);
         const T Mean = 0.5 * (H0 + H1); // MeanLayerThickEdge (EdgeAux2Body)
         T Ue         = splat<T>(0.0);
         if (NeedU)
            Ue = ldk<T>(U, L.Edge[Le * ME + J], K, Kv);
         if (DoFlux) { // FluxLayerThickEdge (EdgeAux2Body), ThicknessFluxDivOnCell (ThickTendBody)
            const T Flux = P.FluxThicknessUpwind ? upwind(Ue, H0, H1) : Mean;
            DivTmp -= L.DvS[Le * ME + J] * Flux * Ue * InvA;
         }
#pragma unroll
         for (int B = 0; B < NB; ++B) {
            const Real *TrL = Tr + (Lt0 + B) * CStride;
            const T T0 = ldk<T>(TrL, C0, K, Kv), T1 = ldk<T>(TrL, C1, K, Kv);
            if (Adv) { // HTracersEdge (TracerEdgeBody), TracerHorzAdvOnCell (TracerTendBody)
               const T HT0 = H0 * T0;
               const T HT1 = H1 * T1;
               T HTr;
               if (!P.FluxTracerUpwind)
                  HTr = 0.5 * (HT0 + HT1);
               else
                  HTr = upwind(Ue, HT0, HT1);
               HAdvTmp[B] -= L.MDvS[Le * ME + J] * HTr * Ue * InvA;
            }
            const T Grad = T1 - T0;
            if (Diff) // TracerDiffOnCell (TracerTendBody)
               DiffTmp[B] -= L.Df2[Le * ME + J] * Mean * Grad;
            if (Hyp) // Del2TracersCell (TracerCellBody)
               D2Tmp[B] -= L.D2C[Le * ME + J] * Mean * Grad;
         }
      }
      if (Thick) {
         T TendV = splat<T>(0.0);
         if (DoFlux)
            TendV -= DivTmp;
         if constexpr (Upd > 0) {
            if (this->Keep)
               stk<T>(HTend, ICell, K, Kv, TendV);
            if constexpr (Upd == 2) {
               Hn = Hc + this->Coeff * TendV; // UpdateFn
               stk<T>(this->NextH, ICell, K, Kv, Hn);
            } else // (launch 2 does the tracer update: nothing to carry)
               stk<T>(this->NextH, ICell, K, Kv, ldk<T>(H, ICell, K, Kv) + this->Coeff * TendV);
         } else
            stk<T>(HTend, ICell, K, Kv, TendV);
      }
#pragma unroll
      for (int B = 0; B < NB; ++B) {
         T TendV = splat<T>(0.0);
         if (Adv)
            TendV -= HAdvTmp[B];
         if (Diff)
            TendV += P.EddyDiff2 * DiffTmp[B] * InvA;
         if constexpr (Upd == 2) {
            if (this->Keep)
               stk<T>(TrTend + (Lt0 + B) * CStride, ICell, K, Kv, TendV);
            const T Cur = ldk<T>(Tr + (Lt0 + B) * CStride, ICell, K, Kv); // UpdateTracersFn
            stk<T>(this->NextTr + (Lt0 + B) * CStride, ICell, K, Kv, (Cur * Hc + this->Coeff * TendV) / Hn);
         } else
            stk<T>(TrTend + (Lt0 + B) * CStride, ICell, K, Kv, TendV);
         if (Hyp)
            stk<T>(Del2Tr + (Lt0 + B) * CStride, ICell, K, Kv, D2Tmp[B] * InvA);
      }
   }
   template <class T> __device__ void compute(const Lds &L, int Le, int ICell, int Kv) const {
      T Hc = splat<T>(0.0), Hn = splat<T>(0.0);
      if constexpr (Upd == 2)
         Hc = ldk<T>(H, ICell, K, Kv);
      if (NT <= 0) {
         pass<T, 0>(L, Le, ICell, Kv, 0, true, Hc, Hn);
         return;
      }
      int Lt = 0;
      for (; Lt + TrBlock <= NT; Lt += TrBlock)
         pass<T, TrBlock>(L, Le, ICell, Kv, Lt, Lt == 0, Hc, Hn);
      if (Lt < NT) // the odd one
         pass<T, 1>(L, Le, ICell, Kv, Lt, Lt == 0, Hc, Hn);
   }
};
using TransportCellBody = TransportCellBodyT<0>;

// ---------------------------------------------------------------------------------------
// Launch 2 (only with the hyperdiffusion term enabled): TracerHyperDiffOnCell (TracerTendBody).  The tendency launch 1
// stored is reloaded -- a stored double reloaded is the register value, the accumulation chain goes on exactly -- and
// the term is subtracted from the Del2TracersCell of the slots' cells.  EddyDiff4 == 0 is evaluated like any other
// value: a non-finite Del2 propagates as in the group call.
//
// Upd: the tracer tendency is final here, so NextTr = (CurTr*Hc + Coeff*TendV)/Hn (UpdateTracersFn) is this launch's
// epilogue, with Hc, the Hn launch 1 stored and CurTr read at the thread's own cell; the tendency is stored only if Keep.
template <bool Upd> struct TransportHyperBodyT : std::conditional_t<Upd, HyperUpdate, NoUpdate> {
   MeshView M;
   int K, NT;
   Real EddyDiff4;
   const Real *Del2Tr;
   Real *TrTend;
   struct Lds {
      Real *Df4, *InvA;
      int *C0, *C1, *N;
   };
   template <class Cv> __host__ __device__ Lds layout(Cv &C, int Tile) const {
      const int ME = M.MaxEdges;
      Lds L;
      L.Df4  = C.template take<Real>(Tile * ME);
      L.InvA = C.template take<Real>(Tile);
      L.C0   = C.template take<int>(Tile * ME);
      L.C1   = C.template take<int>(Tile * ME);
      L.N    = C.template take<int>(Tile);
      return L;
   }
   __device__ void stage(const Lds &L, int First, int Cnt, int Tid, int NThr) const {
      const int ME = M.MaxEdges;
      for (int I = Tid; I < Cnt * ME; I += NThr) {
         const size_t G = (size_t)First * ME + I;
         L.Df4[I]       = M.Diff4CoefOnCell[G];
         L.C0[I]        = M.CellsOnEdgeOnCell[2 * G];
         L.C1[I]        = M.CellsOnEdgeOnCell[2 * G + 1];
      }
      for (int I = Tid; I < Cnt; I += NThr) {
         L.N[I]    = M.NEdgesOnCell[First + I];
         L.InvA[I] = M.InvAreaCell[First + I];
      }
   }
   template <class T> __device__ void compute(const Lds &L, int Le, int ICell, int Kv) const {
      const int ME         = M.MaxEdges;
      const int N          = L.N[Le];
      const Real InvA      = L.InvA[Le];
      const size_t CStride = (size_t)M.NCellsSize * K;
      T Hc = splat<T>(0.0), Hn = splat<T>(0.0);
      if constexpr (Upd) {
         Hc = ldk<T>(this->H, ICell, K, Kv);
         Hn = ldk<T>(this->NextH, ICell, K, Kv);
      }
      for (int Lt = 0; Lt < NT; ++Lt) {
         T TendV         = ldk<T>(TrTend + Lt * CStride, ICell, K, Kv);
         T HypTmp        = splat<T>(0.0);
         const Real *D2L = Del2Tr + Lt * CStride;
         for (int J = 0; J < N; ++J) {
            const T Grad = ldk<T>(D2L, L.C1[Le * ME + J], K, Kv) - ldk<T>(D2L, L.C0[Le * ME + J], K, Kv);
            HypTmp -= L.Df4[Le * ME + J] * Grad;
         }
         TendV -= EddyDiff4 * HypTmp * InvA;
         if constexpr (Upd) {
            if (this->Keep)
               stk<T>(TrTend + Lt * CStride, ICell, K, Kv, TendV);
            const T Cur = ldk<T>(this->Tr + Lt * CStride, ICell, K, Kv);
            stk<T>(this->NextTr + Lt * CStride, ICell, K, Kv, (Cur * Hc + this->Coeff * TendV) / Hn);
         } else
            stk<T>(TrTend + Lt * CStride, ICell, K, Kv, TendV);
      }
   }
};
using TransportHyperBody = TransportHyperBodyT<false>;

void launchTransportTend(const MeshView &M, int K, int NT, const TendParams &P, const AuxPtrs &A, Real *HTend, Real *TrTend,
                         const Real *H, const Real *U, const Real *Tr, hipStream_t S) {
   if (NT < 0)
      NT = 0;
   TransportCellBody B{{}, M, K, NT, P, H, U, Tr, HTend, TrTend, A.Del2TracersCell};
   launchTile(B, M.NCellsAll, K, S);
   if (NT > 0 && P.TracerHyperDiffTendencyEnable) {
      TransportHyperBody Hb{{}, M, K, NT, P.EddyDiff4, A.Del2TracersCell, TrTend};
      launchTile(Hb, M.NCellsAll, K, S);
   }
}

void launchTransportTendUpdate(const MeshView &M, int K, int NT, const TendParams &P, const AuxPtrs &A, Real *HTend,
                               Real *TrTend, const Real *H, const Real *U, const Real *Tr, Real *NextH, Real *NextTr,
                               Real Coeff, bool KeepTend, hipStream_t S) {
   if (NT < 0)
      NT = 0;
   const int Keep = KeepTend ? 1 : 0;
   if (NT > 0 && !P.TracerHyperDiffTendencyEnable) { // the tracer tendency is final in launch 1
      TransportCellBodyT<2> B{{NextH, NextTr, Coeff, Keep}, M, K, NT, P, H, U, Tr, HTend, TrTend, A.Del2TracersCell};
      launchTile(B, M.NCellsAll, K, S);
      return;
   }
   TransportCellBodyT<1> B{{NextH, NextTr, Coeff, Keep}, M, K, NT, P, H, U, Tr, HTend, TrTend, A.Del2TracersCell};
   launchTile(B, M.NCellsAll, K, S);
   if (NT > 0) {
      TransportHyperBodyT<true> Hb{{H, Tr, NextH, NextTr, Coeff, Keep}, M, K, NT, P.EddyDiff4, A.Del2TracersCell, TrTend};
      launchTile(Hb, M.NCellsAll, K, S);
   }
}

} // namespace OMEGA
