// MonotoneAdvKernels.hip -- MonotoneAdv::addTracerTend: flux-corrected horizontal tracer advection in two cell-centric
// tile sweeps (the contract is MonotoneAdv.h's; compiled with -ffp-contract=off).  Like TransportCellBody a cell
// recomputes the edge values of its own slots in registers, so no edge-located array exists in HBM and nothing is
// accumulated across threads: both cells of an edge evaluate the edge's expressions from the same operands in the edge's
// own orientation (c0, c1 = CellsOnEdge), so they hold the same bits.
//
// What a thread holds of an edge is "this cell" and "the cell across" (CellsOnEdgeOnCell, staged as one index per slot);
// which of the two is c0 is the sign of the slot's MaskDvSignOnCell entry (EdgeMask*DvEdge*EdgeSignOnCell: negative where
// this cell is c0, zero on an edge that is masked out or is no local edge -- such a slot reads nothing).  The operands
// are put back into edge order by selects on that wave-uniform flag, which are exact, as is the multiplication by
// EdgeSignOnCell = +-1 written as a select between X and -X.  The cell's own values (h, phi, and in launch 2 its two
// scale factors) are loaded once, the neighbour's once per slot: launch 1 gathers 2 + NB rows per slot for a block of NB
// tracers, launch 2 2 + 3*NB.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; VGPRs / waves per SIMD of the dv2 and the one-level
// instantiation; scratch is 0 in every form) by the number of tracers that share one pass over the slots, and what
// addTracerTend takes at QU30 size with 6 tracers (profiles/r18_monotone_adv_block_ab_qu30.jsonl):
//                    block 1            block 2            block 3            block 4            block 6
//   MonoScaleBody   90 / 5,  63 / 8    118 / 4,  84 / 5   159 / 3, 102 / 4   163 / 3, 116 / 4   233 / 2, 144 / 3
//   MonoFluxBody    89 / 5,  60 / 8    122 / 4,  90 / 5   154 / 3, 108 / 4   162 / 3, 120 / 4   205 / 2, 116 / 4
//   ms              7.71 - 7.76        6.89 - 6.93        6.04 - 6.18        6.94 - 6.99        6.53 - 6.57
// The tracers go in blocks of TrBlock = 3: h of the cell across and u of the edge are loaded once per block, and the
// gathers of three tracers in flight per slot are worth more than the fourth wave that blocks of 2 keep (the transport
// body, with fewer gathers per tracer, settled on 2).  6 tracers are two blocks of 3; 4 + 2 is no better than 2 + 2 + 2.
// A remainder of 2 or 1 tracers takes a pass of that size.
//
// The 3-D form (Vert = true: MonotoneAdv::attachVertAdv) is a compile-time variant of the two bodies; the Vert = false
// instantiations are the ones above, register for register.  After the slots of a block each tracer adds the two
// interfaces of the thread's levels: the level above the first and below the last own level come as single values from
// the cell's own rows (lines the wavefront holds in L1: no new gather, no lane exchange, so nothing changes where an
// interface crosses a lane pair, a line or a level chunk of gridDim.y), and in the two-level lane type the interface
// between the two own levels is evaluated once, from registers alone (it is the top interface of the second level and
// the bottom interface of the first).  Both layers of an interface evaluate it from the same operands, so they agree on
// every bit.  The tracers of a block go one after the other behind a scheduling barrier: interleaved, the twelve
// divisions of a block's scale factors take the dv2 form of launch 1 to 198 VGPRs (2 waves); with the barrier and a
// 3-wave budget it needs 166 and no scratch, and the one-level form of launch 2 keeps its fourth wave (154 -> 118).
// Blocks stay at 3 (VGPRs / waves per SIMD of the dv2 and the one-level instantiation, scratch 0 in each):
//                    block 3, Vert = true
//   MonoScaleBody   166 / 3, 118 / 4
//   MonoFluxBody    160 / 3, 118 / 4
// At QU30 size with 6 tracers the 3-D call takes 8.67 ms where the 2-D one takes 6.27 (launch 1 +0.6 ms, launch 2
// +1.7 ms; profiles/r20_monotone_adv3d_diag_qu30.json).  Tried and not kept, DESIGN.md section 4.11: the neighbouring
// levels from the neighbouring lanes instead of loads (no gain: the loads are not what costs), VerticalTransport asked
// for above the slot loop (slower), launch 2 without the barrier in the dv2 form (slower).
//
// The high-order horizontal flux (High = true: MonotoneAdv::setHorzOrder(3 or 4)) is a second compile-time variant of the
// two bodies behind a launch of its own, MonoHessBody, which stores the three Hess rows of every cell and tracer; the
// High = false instantiations are the ones above, register for register.  The direction coefficients of a slot, on the
// cell's side and on the side of the cell across, are staged in the LDS tile (48 B per slot); the cell's own Hess rows
// are loaded once per tracer, those of the cell across per slot and tracer, under a branch on the slot's high flag, so
// that nothing of Hess enters on an edge that is not high.  Both cells of an edge put D of the two sides into the edge's
// order by selects, as they do with phi.  Blocks of 2 tracers (VGPRs / waves per SIMD of the dv2 and the one-level
// instantiation, scratch 0 in each; the 3-D scale body takes a 2-wave budget here: at 3 waves it spills 48 B):
//                    Vert = false         Vert = true          with blocks of 3
//   MonoScaleBody   182 / 2, 126 / 4     188 / 2, 136 / 3     224 / 2, 146 / 3;  168 / 3 + 236 B scratch, 158 / 3
//   MonoFluxBody    182 / 2, 122 / 4     188 / 2, 148 / 3     226 / 2, 148 / 3;  232 / 2, 174 / 2
//   MonoHessBody    110 / 4,  68 / 7     (blocks of 3)
// At QU30 size with 6 tracers the order-4 call takes 16.36 ms where the centred one takes 6.13 (pass 0 2.06 ms, pass 1
// 6.37 against 2.59, pass 2 7.99 against 3.56; profiles/r21_monotone_adv_ho_diag_qu30.json); blocks of 3 give 16.02 ms
// and cost the one-level forms a wave and the 3-D forms their registers.  DESIGN.md section 4.12.
#include "KernelCommon.h"
#include "MonotoneAdvKernels.h"

namespace OMEGA {

// max / min as the contract writes them: comparisons, so C++ and NumPy agree on every operand (signed zeros, NaN)
//   max(a, b) = a < b ? b : a        min(a, b) = b < a ? b : a
__device__ __forceinline__ double kmin(double A, double B) { return B < A ? B : A; }
__device__ __forceinline__ dv2 kmin(dv2 A, dv2 B) {
   dv2 R;
   R.x = kmin(A.x, B.x);
   R.y = kmin(A.y, B.y);
   return R;
}
/// FLow = Fm >= 0.0 ? Fm*P0 : Fm*P1
__device__ __forceinline__ double lowFlux(double Fm, double P0, double P1) { return Fm >= 0.0 ? Fm * P0 : Fm * P1; }
__device__ __forceinline__ dv2 lowFlux(dv2 Fm, dv2 P0, dv2 P1) {
   dv2 R;
   R.x = lowFlux(Fm.x, P0.x, P1.x);
   R.y = lowFlux(Fm.y, P0.y, P1.y);
   return R;
}
/// P > 0.0 ? min(1.0, Q/P) : 1.0
__device__ __forceinline__ double scaleOf(double P, double Q) { return P > 0.0 ? kmin(1.0, Q / P) : 1.0; }
__device__ __forceinline__ dv2 scaleOf(dv2 P, dv2 Q) {
   dv2 R;
   R.x = scaleOf(P.x, Q.x);
   R.y = scaleOf(P.y, Q.y);
   return R;
}
/// A >= 0.0 ? X : Y
__device__ __forceinline__ double selGe0(double A, double X, double Y) { return A >= 0.0 ? X : Y; }
__device__ __forceinline__ dv2 selGe0(dv2 A, dv2 X, dv2 Y) {
   dv2 R;
   R.x = selGe0(A.x, X.x, Y.x);
   R.y = selGe0(A.y, X.y, Y.y);
   return R;
}

/// the tables both launches stage: per slot the coefficient, the edge and the cell across; per cell the slot count and
/// 1/AreaCell
struct MonoLds {
   Real *MDvS, *InvA;
   int *Edge, *Nbr, *N;
};
struct MonoTables {
   using Lds = MonoLds;
   MeshView M;
   template <class Cv> __host__ __device__ MonoLds layout(Cv &C, int Tile) const {
      const int ME = M.MaxEdges;
      MonoLds L;
      L.MDvS = C.template take<Real>(Tile * ME);
      L.InvA = C.template take<Real>(Tile);
      L.Edge = C.template take<int>(Tile * ME);
      L.Nbr  = C.template take<int>(Tile * ME);
      L.N    = C.template take<int>(Tile);
      return L;
   }
   __device__ void stage(const MonoLds &L, int First, int Cnt, int Tid, int NThr) const {
      const int ME = M.MaxEdges;
      for (int I = Tid; I < Cnt * ME; I += NThr) {
         const size_t G = (size_t)First * ME + I;
         const Real Md  = M.MaskDvSignOnCell[G];
         L.MDvS[I]      = Md;
         L.Edge[I]      = M.EdgesOnCell[G];
         L.Nbr[I]       = M.CellsOnEdgeOnCell[2 * G + (Md < 0.0 ? 1 : 0)]; // this cell is c0: the cell across is c1
      }
      for (int I = Tid; I < Cnt; I += NThr) {
         L.N[I]    = M.NEdgesOnCell[First + I];
         L.InvA[I] = M.InvAreaCell[First + I];
      }
   }
};

/// The 3-D form (MonotoneAdv::attachVertAdv) adds the cell's layer range to the tables and VerticalTransport to the rows.
struct MonoLdsV : MonoLds {
   int *KMin, *KMax;
};
struct MonoTablesV : MonoTables {
   using Lds = MonoLdsV;
   int KLog; ///< NVertLayers (launchTile sets it): no interface at or below it carries flux
   const Real *Wt;
   const I4 *KMinCell, *KMaxCell;
   template <class Cv> __host__ __device__ MonoLdsV layout(Cv &C, int Tile) const {
      MonoLdsV L;
      static_cast<MonoLds &>(L) = MonoTables::layout(C, Tile);
      L.KMin                    = C.template take<int>(Tile);
      L.KMax                    = C.template take<int>(Tile);
      return L;
   }
   __device__ void stage(const MonoLdsV &L, int First, int Cnt, int Tid, int NThr) const {
      MonoTables::stage(L, First, Cnt, Tid, NThr);
      for (int I = Tid; I < Cnt; I += NThr) {
         L.KMin[I] = KMinCell[First + I];
         L.KMax[I] = KMaxCell[First + I];
      }
   }
};
/// The high-order horizontal flux (MonotoneAdv::setHorzOrder(3 or 4)) adds the direction coefficients of every slot, on
/// the cell's side and on the side of the cell across, to the tables (48 B per slot) and Hess to the rows.
template <class Base> struct MonoLdsH : Base::Lds {
   Real *QOwn, *QAcr;
};
template <class Base> struct MonoTablesH : Base {
   using Lds = MonoLdsH<Base>;
   const Real *DirOwn, *DirAcr, *Hess;
   Real Beta;
   template <class Cv> __host__ __device__ Lds layout(Cv &C, int Tile) const {
      Lds L;
      static_cast<typename Base::Lds &>(L) = Base::layout(C, Tile);
      L.QOwn                               = C.template take<Real>(Tile * this->M.MaxEdges * 3);
      L.QAcr                               = C.template take<Real>(Tile * this->M.MaxEdges * 3);
      return L;
   }
   __device__ void stage(const Lds &L, int First, int Cnt, int Tid, int NThr) const {
      Base::stage(L, First, Cnt, Tid, NThr);
      const int ME3 = this->M.MaxEdges * 3;
      for (int I = Tid; I < Cnt * ME3; I += NThr) {
         L.QOwn[I] = DirOwn[(size_t)First * ME3 + I];
         L.QAcr[I] = DirAcr[(size_t)First * ME3 + I];
      }
   }
};
template <bool Vert, bool High>
using MonoTablesOf = std::conditional_t<High, MonoTablesH<std::conditional_t<Vert, MonoTablesV, MonoTables>>,
                                        std::conditional_t<Vert, MonoTablesV, MonoTables>>;

/// tracers per pass over the slots of the two bodies with the high-order flux
constexpr int HighTrBlock = 2;
/// a slot's edge is high: its direction coefficients are set (cs^2 and sn^2 are not both zero)
__device__ __forceinline__ bool highSlot(const Real *Qo) { return Qo[0] != 0.0 || Qo[2] != 0.0; }
/// Corr of a high edge in edge orientation: D of this cell (its Hess Hc, its side's coefficients Qo) and of the cell
/// across (Hn, Qa) put into the order c0, c1; S + (Fm >= 0.0 ? B : -B)
template <class T>
__device__ __forceinline__ T highCorr(const Real *Qo, const Real *Qa, bool IsC0, Real Beta, const T &Fm, const T (&Hc)[3],
                                      const T (&Hn)[3]) {
   const T Dc = (Qo[0] * Hc[0] + Qo[1] * Hc[1]) + Qo[2] * Hc[2];
   const T Dn = (Qa[0] * Hn[0] + Qa[1] * Hn[1]) + Qa[2] * Hn[2];
   const T D0 = IsC0 ? Dc : Dn, D1 = IsC0 ? Dn : Dc;
   const T S = D0 + D1, Td = D0 - D1;
   const T B = Beta * Td;
   return S + selGe0(Fm, B, T(-B));
}

// The vertical part of a thread: its own levels are in registers; of the level above its first and the one below its
// last it loads single values from the cell's own rows (lines this wavefront has just fetched).  Interface K is the top
// of layer K and carries flux for KMin < K <= KMax; where it does not, the level across it is not read (the index is
// clamped to the thread's own level) and every value of the interface is selected to 0.0.
template <class T> struct VertSpan {
   static constexpr int W = VecW<T>::W;
   bool Top[W], Bot[W]; ///< the top / bottom interface of each own level carries flux
   int KUp, KDn;        ///< the level above the first own level, below the last; the own level where there is none
   __device__ __forceinline__ VertSpan(int Kv, int KMin, int KMax, int KLog) {
#pragma unroll
      for (int I = 0; I < W; ++I) {
         const int Lev = Kv * W + I;
         Top[I]        = KMin < Lev && Lev <= KMax && Lev > 0 && Lev < KLog; // (the last two: whatever the range says)
         Bot[I]        = KMin <= Lev && Lev < KMax && Lev + 1 < KLog;
      }
      KUp = Top[0] ? Kv * W - 1 : Kv * W;
      KDn = Bot[W - 1] ? Kv * W + W : Kv * W + W - 1;
   }
};
__device__ __forceinline__ double ld1(const double *P, int Row, int K, int Lev) { return P[(size_t)Row * K + Lev]; }
/// the values one level above / below each own level
__device__ __forceinline__ double above(double, double Up) { return Up; }
__device__ __forceinline__ dv2 above(dv2 Own, double Up) {
   dv2 R;
   R.x = Up;
   R.y = Own.x;
   return R;
}
__device__ __forceinline__ double below(double, double Dn) { return Dn; }
__device__ __forceinline__ dv2 below(dv2 Own, double Dn) {
   dv2 R;
   R.x = Own.y;
   R.y = Dn;
   return R;
}
/// the last own level
__device__ __forceinline__ double last(double Own) { return Own; }
__device__ __forceinline__ double last(dv2 Own) { return Own.y; }
/// M ? X : Y per level
__device__ __forceinline__ double selIn(const bool (&M)[1], double X, double Y) { return M[0] ? X : Y; }
__device__ __forceinline__ dv2 selIn(const bool (&M)[2], dv2 X, dv2 Y) {
   dv2 R;
   R.x = M[0] ? X.x : Y.x;
   R.y = M[1] ? X.y : Y.y;
   return R;
}
/// VLow = Wv > 0.0 ? Wv*PD : Wv*PU
__device__ __forceinline__ double lowFluxV(double Wv, double PU, double PD) { return Wv > 0.0 ? Wv * PD : Wv * PU; }
__device__ __forceinline__ dv2 lowFluxV(dv2 Wv, dv2 PU, dv2 PD) {
   dv2 R;
   R.x = lowFluxV(Wv.x, PU.x, PD.x);
   R.y = lowFluxV(Wv.y, PU.y, PD.y);
   return R;
}
/// VLow and AV of the interface between the layers U (above) and D (below), RU = hU/(hU + hD); 0.0 where In is false
template <class T, int W>
__device__ __forceinline__ void vertIface(const bool (&In)[W], const T &Wv, const T &PU, const T &PD, const T &RU, T &VLow,
                                          T &AV) {
   const T Z     = splat<T>(0.0);
   const T VL    = lowFluxV(Wv, PU, PD);
   const T PhiT  = PU + RU * (PD - PU);
   const T VHigh = Wv * PhiT;
   VLow          = selIn(In, VL, Z);
   AV            = selIn(In, T(VHigh - VL), Z);
}

/// the mass flux of a slot's edge in edge orientation: Fm = DvEdge*(hE*u)
template <class T>
__device__ __forceinline__ T massFlux(Real Dv, bool IsC0, bool Upwind, const T &Hc, const T &Hn, const T &Ue) {
   const T H0 = IsC0 ? Hc : Hn, H1 = IsC0 ? Hn : Hc;
   const T HE = Upwind ? upwind(Ue, H0, H1) : T(0.5 * (H0 + H1));
   return Dv * (HE * Ue);
}

// ---------------------------------------------------------------------------------------
// Launch 1, one thread per (cell, level chunk): ScaleIn, ScaleOut of the cell for every tracer.
// Vert: the 3-D form, which adds the two interfaces of every level to the sums after the slots.
// High: the high-order horizontal flux, which takes the cell's own three Hess rows once and gathers those of the cell
// across per slot and tracer.
template <bool Vert, bool High> struct MonoScaleBodyT : MonoTablesOf<Vert, High> {
   static constexpr int TrBlock  = High ? HighTrBlock : 3;
   static constexpr int MinWaves = Vert ? (High ? 2 : 3) : 1; // (1 is what a body without the member gets)
   using Lds                    = typename MonoTablesOf<Vert, High>::Lds;
   int K, NT, Upwind;
   Real Dt;
   const Real *HOld, *HNew, *U, *Tr;
   Real *SIn, *SOut;
   template <class T, int NB> __device__ __forceinline__ void pass(const Lds &L, int Le, int ICell, int Kv, int Lt0) const {
      const MeshView &M    = this->M;
      const int ME         = M.MaxEdges;
      const int N          = L.N[Le];
      const Real InvA      = L.InvA[Le];
      const size_t CStride = (size_t)M.NCellsSize * K;
      const T Hc           = ldk<T>(HOld, ICell, K, Kv);
      T Pc[NB], PMax[NB], PMin[NB], DivLow[NB], In[NB], Out[NB];
#pragma unroll
      for (int B = 0; B < NB; ++B) {
         Pc[B] = PMax[B] = PMin[B] = ldk<T>(Tr + (Lt0 + B) * CStride, ICell, K, Kv);
         DivLow[B] = In[B] = Out[B] = splat<T>(0.0);
      }
      T Hs[High ? NB : 1][3];
      if constexpr (High) {
#pragma unroll
         for (int B = 0; B < NB; ++B)
#pragma unroll
            for (int X = 0; X < 3; ++X)
               Hs[B][X] = ldk<T>(this->Hess + ((Lt0 + B) * 3 + X) * CStride, ICell, K, Kv);
      }
      for (int J = 0; J < N; ++J) {
         const Real Md = L.MDvS[Le * ME + J];
         if (Md == 0.0) // EdgeMask 0, or no local edge: Fm = 0.0 exactly, no cell is read
            continue;
         const bool IsC0 = Md < 0.0;
         const int Nb    = L.Nbr[Le * ME + J];
         const T Hn      = ldk<T>(HOld, Nb, K, Kv);
         const T Ue      = ldk<T>(U, L.Edge[Le * ME + J], K, Kv);
         const T Fm      = massFlux<T>(IsC0 ? -Md : Md, IsC0, Upwind != 0, Hc, Hn, Ue);
         [[maybe_unused]] const Real *Qo = nullptr;
         [[maybe_unused]] bool Hi        = false;
         if constexpr (High) {
            Qo = L.QOwn + (Le * ME + J) * 3;
            Hi = highSlot(Qo);
         }
#pragma unroll
         for (int B = 0; B < NB; ++B) {
            const T Pn = ldk<T>(Tr + (Lt0 + B) * CStride, Nb, K, Kv);
            const T P0 = IsC0 ? Pc[B] : Pn, P1 = IsC0 ? Pn : Pc[B];
            const T FLow  = lowFlux(Fm, P0, P1);
            T FHigh;
            if constexpr (High) {
               T Corr = splat<T>(0.0);
               if (Hi) {
                  T HnX[3];
#pragma unroll
                  for (int X = 0; X < 3; ++X)
                     HnX[X] = ldk<T>(this->Hess + ((Lt0 + B) * 3 + X) * CStride, Nb, K, Kv);
                  Corr = highCorr<T>(Qo, L.QAcr + (Le * ME + J) * 3, IsC0, this->Beta, Fm, Hs[B], HnX);
               }
               FHigh = Fm * (0.5 * (P0 + P1) - Corr);
            } else
               FHigh = Fm * (0.5 * (P0 + P1));
            const T A     = FHigh - FLow;
            PMax[B]       = kmax(PMax[B], Pn);
            PMin[B]       = kmin(PMin[B], Pn);
            const T SF = IsC0 ? T(-FLow) : FLow, SA = IsC0 ? T(-A) : A; // s*FLow, s*A
            DivLow[B]  = DivLow[B] + SF;
            In[B]      = In[B] + kmax(SA, splat<T>(0.0));
            Out[B]     = Out[B] + kmax(T(-SA), splat<T>(0.0));
         }
      }
      const T Hw = ldk<T>(HNew, ICell, K, Kv);
      if constexpr (Vert) {
         const T Z = splat<T>(0.0);
         const VertSpan<T> Sp(Kv, L.KMin[Le], L.KMax[Le], this->KLog);
         // the top interfaces of the own levels as T, the bottom interface of the last own level as one value (D); the
         // bottom interface of the first of two levels is the top interface of the second
         const bool BotD[1] = {Sp.Bot[VecW<T>::W - 1]};
         const T WvT     = selIn(Sp.Top, ldk<T>(this->Wt, ICell, K, Kv), Z);
         const double WvD = selIn(BotD, ld1(this->Wt, ICell, K, Sp.KDn), 0.0);
         const T HA      = above(Hc, ld1(HOld, ICell, K, Sp.KUp));
         const T RT      = HA / (HA + Hc); // h[K-1]/(h[K-1] + h[K])
         const double RD = last(Hc) / (last(Hc) + ld1(HOld, ICell, K, Sp.KDn));
#pragma unroll
         for (int B = 0; B < NB; ++B) {
            const Real *TrL  = Tr + (Lt0 + B) * CStride;
            const double PDn = ld1(TrL, ICell, K, Sp.KDn);
            const T PA = above(Pc[B], ld1(TrL, ICell, K, Sp.KUp)), PB = below(Pc[B], PDn);
            PMax[B] = selIn(Sp.Top, kmax(PMax[B], PA), PMax[B]);
            PMin[B] = selIn(Sp.Top, kmin(PMin[B], PA), PMin[B]);
            PMax[B] = selIn(Sp.Bot, kmax(PMax[B], PB), PMax[B]);
            PMin[B] = selIn(Sp.Bot, kmin(PMin[B], PB), PMin[B]);
            T VLt, AVt;
            double VLd, AVd;
            vertIface(Sp.Top, WvT, PA, Pc[B], RT, VLt, AVt);
            vertIface(BotD, WvD, last(Pc[B]), PDn, RD, VLd, AVd);
            const T VLb = below(VLt, VLd), AVb = below(AVt, AVd);
            const T HTd  = Hc * Pc[B] + Dt * (((DivLow[B] * InvA) - VLt) + VLb);
            const T PIn  = Dt * (((In[B] * InvA) + kmax(T(-AVt), Z)) + kmax(AVb, Z));
            const T POut = Dt * (((Out[B] * InvA) + kmax(AVt, Z)) + kmax(T(-AVb), Z));
            const T QIn  = kmax(Z, T(PMax[B] * Hw - HTd));
            const T QOut = kmax(Z, T(HTd - PMin[B] * Hw));
            stk<T>(SIn + (Lt0 + B) * CStride, ICell, K, Kv, scaleOf(PIn, QIn));
            stk<T>(SOut + (Lt0 + B) * CStride, ICell, K, Kv, scaleOf(POut, QOut));
            __builtin_amdgcn_sched_barrier(0);
         }
         return;
      }
#pragma unroll
      for (int B = 0; B < NB; ++B) {
         const T HTd  = Hc * Pc[B] + Dt * (DivLow[B] * InvA);
         const T PIn  = Dt * (In[B] * InvA);
         const T POut = Dt * (Out[B] * InvA);
         const T QIn  = kmax(splat<T>(0.0), T(PMax[B] * Hw - HTd));
         const T QOut = kmax(splat<T>(0.0), T(HTd - PMin[B] * Hw));
         stk<T>(SIn + (Lt0 + B) * CStride, ICell, K, Kv, scaleOf(PIn, QIn));
         stk<T>(SOut + (Lt0 + B) * CStride, ICell, K, Kv, scaleOf(POut, QOut));
      }
   }
   template <class T> __device__ void compute(const Lds &L, int Le, int ICell, int Kv) const {
      int Lt = 0;
      for (; Lt + TrBlock <= NT; Lt += TrBlock)
         pass<T, TrBlock>(L, Le, ICell, Kv, Lt);
      if constexpr (TrBlock > 2) {
         if (NT - Lt >= 2) {
            pass<T, 2>(L, Le, ICell, Kv, Lt);
            Lt += 2;
         }
      }
      if (Lt < NT) // the odd one
         pass<T, 1>(L, Le, ICell, Kv, Lt);
   }
};

// ---------------------------------------------------------------------------------------
// Launch 2, one thread per (cell, level chunk): Tend += (sum over the slots of s*(FLow + Sc*A))/AreaCell, with the scale
// factors launch 1 stored at the cell and at the cells across.
// Vert: the 3-D form, which adds the limited fluxes of the two interfaces of every level after the slots; an interface's
// scale factors are the cell's own, launch 1's of the levels on its two sides.
template <bool Vert, bool High> struct MonoFluxBodyT : MonoTablesOf<Vert, High> {
   static constexpr int TrBlock = High ? HighTrBlock : 3;
   using Lds                    = typename MonoTablesOf<Vert, High>::Lds;
   int K, NT, Upwind;
   const Real *HOld, *U, *Tr, *SIn, *SOut;
   Real *Tend;
   template <class T, int NB> __device__ __forceinline__ void pass(const Lds &L, int Le, int ICell, int Kv, int Lt0) const {
      const MeshView &M    = this->M;
      const int ME         = M.MaxEdges;
      const int N          = L.N[Le];
      const Real InvA      = L.InvA[Le];
      const size_t CStride = (size_t)M.NCellsSize * K;
      const T Hc           = ldk<T>(HOld, ICell, K, Kv);
      T Pc[NB], SIc[NB], SOc[NB], Sum[NB];
#pragma unroll
      for (int B = 0; B < NB; ++B) {
         Pc[B]  = ldk<T>(Tr + (Lt0 + B) * CStride, ICell, K, Kv);
         SIc[B] = ldk<T>(SIn + (Lt0 + B) * CStride, ICell, K, Kv);
         SOc[B] = ldk<T>(SOut + (Lt0 + B) * CStride, ICell, K, Kv);
         Sum[B] = splat<T>(0.0);
      }
      T Hs[High ? NB : 1][3];
      if constexpr (High) {
#pragma unroll
         for (int B = 0; B < NB; ++B)
#pragma unroll
            for (int X = 0; X < 3; ++X)
               Hs[B][X] = ldk<T>(this->Hess + ((Lt0 + B) * 3 + X) * CStride, ICell, K, Kv);
      }
      for (int J = 0; J < N; ++J) {
         const Real Md = L.MDvS[Le * ME + J];
         if (Md == 0.0)
            continue;
         const bool IsC0 = Md < 0.0;
         const int Nb    = L.Nbr[Le * ME + J];
         const T Hn      = ldk<T>(HOld, Nb, K, Kv);
         const T Ue      = ldk<T>(U, L.Edge[Le * ME + J], K, Kv);
         const T Fm      = massFlux<T>(IsC0 ? -Md : Md, IsC0, Upwind != 0, Hc, Hn, Ue);
         [[maybe_unused]] const Real *Qo = nullptr;
         [[maybe_unused]] bool Hi        = false;
         if constexpr (High) {
            Qo = L.QOwn + (Le * ME + J) * 3;
            Hi = highSlot(Qo);
         }
#pragma unroll
         for (int B = 0; B < NB; ++B) {
            const T Pn  = ldk<T>(Tr + (Lt0 + B) * CStride, Nb, K, Kv);
            const T SIn_ = ldk<T>(SIn + (Lt0 + B) * CStride, Nb, K, Kv);
            const T SOn = ldk<T>(SOut + (Lt0 + B) * CStride, Nb, K, Kv);
            const T P0 = IsC0 ? Pc[B] : Pn, P1 = IsC0 ? Pn : Pc[B];
            const T SI0 = IsC0 ? SIc[B] : SIn_, SI1 = IsC0 ? SIn_ : SIc[B];
            const T SO0 = IsC0 ? SOc[B] : SOn, SO1 = IsC0 ? SOn : SOc[B];
            const T FLow  = lowFlux(Fm, P0, P1);
            T FHigh;
            if constexpr (High) {
               T Corr = splat<T>(0.0);
               if (Hi) {
                  T HnX[3];
#pragma unroll
                  for (int X = 0; X < 3; ++X)
                     HnX[X] = ldk<T>(this->Hess + ((Lt0 + B) * 3 + X) * CStride, Nb, K, Kv);
                  Corr = highCorr<T>(Qo, L.QAcr + (Le * ME + J) * 3, IsC0, this->Beta, Fm, Hs[B], HnX);
               }
               FHigh = Fm * (0.5 * (P0 + P1) - Corr);
            } else
               FHigh = Fm * (0.5 * (P0 + P1));
            const T A     = FHigh - FLow;
            const T Sc    = selGe0(A, kmin(SO0, SI1), kmin(SI0, SO1));
            const T F     = FLow + Sc * A;
            Sum[B]        = Sum[B] + (IsC0 ? T(-F) : F); // s*F
         }
      }
      if constexpr (Vert) {
         const T Z = splat<T>(0.0);
         const VertSpan<T> Sp(Kv, L.KMin[Le], L.KMax[Le], this->KLog);
         const bool BotD[1] = {Sp.Bot[VecW<T>::W - 1]}; // (as in launch 1)
         const T WvT     = selIn(Sp.Top, ldk<T>(this->Wt, ICell, K, Kv), Z);
         const double WvD = selIn(BotD, ld1(this->Wt, ICell, K, Sp.KDn), 0.0);
         const T HA      = above(Hc, ld1(HOld, ICell, K, Sp.KUp));
         const T RT      = HA / (HA + Hc);
         const double RD = last(Hc) / (last(Hc) + ld1(HOld, ICell, K, Sp.KDn));
#pragma unroll
         for (int B = 0; B < NB; ++B) {
            const size_t Off = (Lt0 + B) * CStride;
            const T PA  = above(Pc[B], ld1(Tr + Off, ICell, K, Sp.KUp));
            const T SIA = above(SIc[B], ld1(SIn + Off, ICell, K, Sp.KUp)), SOA = above(SOc[B], ld1(SOut + Off, ICell, K, Sp.KUp));
            const double PDn = ld1(Tr + Off, ICell, K, Sp.KDn);
            const double SIDn = ld1(SIn + Off, ICell, K, Sp.KDn), SODn = ld1(SOut + Off, ICell, K, Sp.KDn);
            T VLt, AVt;
            double VLd, AVd;
            vertIface(Sp.Top, WvT, PA, Pc[B], RT, VLt, AVt);
            vertIface(BotD, WvD, last(Pc[B]), PDn, RD, VLd, AVd);
            // interface K: out of layer K into K-1 where AV >= 0
            const T ScT      = selGe0(AVt, kmin(SOc[B], SIA), kmin(SIc[B], SOA));
            const double ScD = selGe0(AVd, kmin(SODn, last(SIc[B])), kmin(SIDn, last(SOc[B])));
            const T FVt      = selIn(Sp.Top, T(VLt + ScT * AVt), Z);
            const T FVb      = below(FVt, selIn(BotD, VLd + ScD * AVd, 0.0));
            stk<T>(Tend + Off, ICell, K, Kv, ldk<T>(Tend + Off, ICell, K, Kv) + (((Sum[B] * InvA) - FVt) + FVb));
            __builtin_amdgcn_sched_barrier(0);
         }
         return;
      }
#pragma unroll
      for (int B = 0; B < NB; ++B) {
         Real *TendL = Tend + (Lt0 + B) * CStride;
         stk<T>(TendL, ICell, K, Kv, ldk<T>(TendL, ICell, K, Kv) + Sum[B] * InvA);
      }
   }
   template <class T> __device__ void compute(const Lds &L, int Le, int ICell, int Kv) const {
      int Lt = 0;
      for (; Lt + TrBlock <= NT; Lt += TrBlock)
         pass<T, TrBlock>(L, Le, ICell, Kv, Lt);
      if constexpr (TrBlock > 2) {
         if (NT - Lt >= 2) {
            pass<T, 2>(L, Le, ICell, Kv, Lt);
            Lt += 2;
         }
      }
      if (Lt < NT) // the odd one
         pass<T, 1>(L, Le, ICell, Kv, Lt);
   }
};

// ---------------------------------------------------------------------------------------
// Pass 0 of the high-order flux, one thread per (cell, level chunk): Hess[L][xx, xy, yy] of the cell for every tracer, the
// sum over the slots of HessWeight*(phi[n] - phi[c]).  A cell that is not a fit cell stores 0.0 and reads no neighbour.
struct MonoHessLds {
   Real *W;
   int *Nbr, *N, *Fit;
};
struct MonoHessBody {
   static constexpr int TrBlock = 3;
   using Lds                    = MonoHessLds;
   MeshView M;
   int K, NT;
   const Real *HessWeight, *FitCell, *Tr;
   Real *Hess;
   template <class Cv> __host__ __device__ MonoHessLds layout(Cv &C, int Tile) const {
      MonoHessLds L;
      L.W   = C.template take<Real>(Tile * M.MaxEdges * 3);
      L.Nbr = C.template take<int>(Tile * M.MaxEdges);
      L.N   = C.template take<int>(Tile);
      L.Fit = C.template take<int>(Tile);
      return L;
   }
   __device__ void stage(const MonoHessLds &L, int First, int Cnt, int Tid, int NThr) const {
      const int ME = M.MaxEdges;
      for (int I = Tid; I < Cnt * ME * 3; I += NThr)
         L.W[I] = HessWeight[(size_t)First * ME * 3 + I];
      for (int I = Tid; I < Cnt * ME; I += NThr) {
         const size_t G = (size_t)First * ME + I;
         L.Nbr[I]       = M.CellsOnEdgeOnCell[2 * G + (M.MaskDvSignOnCell[G] < 0.0 ? 1 : 0)]; // (as MonoTables::stage)
      }
      for (int I = Tid; I < Cnt; I += NThr) {
         L.N[I]   = M.NEdgesOnCell[First + I];
         L.Fit[I] = FitCell[First + I] != 0.0 ? 1 : 0;
      }
   }
   template <class T, int NB> __device__ __forceinline__ void pass(const Lds &L, int Le, int ICell, int Kv, int Lt0) const {
      const int ME         = M.MaxEdges;
      const size_t CStride = (size_t)M.NCellsSize * K;
      T H[NB][3];
#pragma unroll
      for (int B = 0; B < NB; ++B)
         H[B][0] = H[B][1] = H[B][2] = splat<T>(0.0);
      if (L.Fit[Le]) { // every slot of a fit cell has a local cell across a masked-in edge
         const int N = L.N[Le];
         T Pc[NB];
#pragma unroll
         for (int B = 0; B < NB; ++B)
            Pc[B] = ldk<T>(Tr + (Lt0 + B) * CStride, ICell, K, Kv);
         for (int J = 0; J < N; ++J) {
            const int Nb  = L.Nbr[Le * ME + J];
            const Real *W = L.W + (Le * ME + J) * 3;
#pragma unroll
            for (int B = 0; B < NB; ++B) {
               const T D = ldk<T>(Tr + (Lt0 + B) * CStride, Nb, K, Kv) - Pc[B];
#pragma unroll
               for (int X = 0; X < 3; ++X)
                  H[B][X] = H[B][X] + W[X] * D;
            }
         }
      }
#pragma unroll
      for (int B = 0; B < NB; ++B)
#pragma unroll
         for (int X = 0; X < 3; ++X)
            stk<T>(Hess + ((Lt0 + B) * 3 + X) * CStride, ICell, K, Kv, H[B][X]);
   }
   template <class T> __device__ void compute(const Lds &L, int Le, int ICell, int Kv) const {
      int Lt = 0;
      for (; Lt + TrBlock <= NT; Lt += TrBlock)
         pass<T, TrBlock>(L, Le, ICell, Kv, Lt);
      if (NT - Lt >= 2) {
         pass<T, 2>(L, Le, ICell, Kv, Lt);
         Lt += 2;
      }
      if (Lt < NT) // the odd one
         pass<T, 1>(L, Le, ICell, Kv, Lt);
   }
};

template <bool Vert, bool High> static int launchMonotoneAdvT(const MeshView &M, const MonotoneAdvArgs &A, hipStream_t S) {
   MonoScaleBodyT<Vert, High> B1{};
   MonoFluxBodyT<Vert, High> B2{};
   B1.M = B2.M = M;
   B1.K = B2.K = A.K, B1.NT = B2.NT = A.NTracers, B1.Upwind = B2.Upwind = A.FluxThicknessUpwind;
   B1.HOld = B2.HOld = A.HOld, B1.U = B2.U = A.NormalVelocity, B1.Tr = B2.Tr = A.Tracers;
   B1.SIn = A.ScaleIn, B1.SOut = A.ScaleOut, B2.SIn = A.ScaleIn, B2.SOut = A.ScaleOut;
   B1.Dt = A.Dt, B1.HNew = A.HNew, B2.Tend = A.Tend;
   if constexpr (Vert) {
      B1.Wt = B2.Wt = A.VerticalTransport;
      B1.KMinCell = B2.KMinCell = A.MinLayerCell, B1.KMaxCell = B2.KMaxCell = A.MaxLayerCell;
   }
   if constexpr (High) {
      MonoHessBody B0{};
      B0.M = M, B0.K = A.K, B0.NT = A.NTracers;
      B0.HessWeight = A.HessWeight, B0.FitCell = A.FitCell, B0.Tr = A.Tracers, B0.Hess = A.Hess;
      B1.DirOwn = B2.DirOwn = A.EdgeDirOwn, B1.DirAcr = B2.DirAcr = A.EdgeDirAcross;
      B1.Hess = B2.Hess = A.Hess, B1.Beta = B2.Beta = A.Beta;
      launchTile(B0, M.NCellsAll, A.K, S);
   }
   launchTile(B1, M.NCellsAll, A.K, S);
   launchTile(B2, M.NCellsAll, A.K, S);
   return High ? 3 : 2;
}

int launchMonotoneAdv(const MeshView &M, const MonotoneAdvArgs &A, hipStream_t S) {
   if (A.NTracers <= 0)
      return 0;
   const bool Vert = A.VerticalTransport != nullptr;
   if (A.Hess != nullptr)
      return Vert ? launchMonotoneAdvT<true, true>(M, A, S) : launchMonotoneAdvT<false, true>(M, A, S);
   return Vert ? launchMonotoneAdvT<true, false>(M, A, S) : launchMonotoneAdvT<false, false>(M, A, S);
}

} // namespace OMEGA
