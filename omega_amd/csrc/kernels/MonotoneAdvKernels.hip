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

/// the mass flux of a slot's edge in edge orientation: Fm = DvEdge*(hE*u)
template <class T>
__device__ __forceinline__ T massFlux(Real Dv, bool IsC0, bool Upwind, const T &Hc, const T &Hn, const T &Ue) {
   const T H0 = IsC0 ? Hc : Hn, H1 = IsC0 ? Hn : Hc;
   const T HE = Upwind ? upwind(Ue, H0, H1) : T(0.5 * (H0 + H1));
   return Dv * (HE * Ue);
}

// ---------------------------------------------------------------------------------------
// Launch 1, one thread per (cell, level chunk): ScaleIn, ScaleOut of the cell for every tracer.
struct MonoScaleBody : MonoTables {
   static constexpr int TrBlock = 3;
   using Lds                    = MonoLds;
   int K, NT, Upwind;
   Real Dt;
   const Real *HOld, *HNew, *U, *Tr;
   Real *SIn, *SOut;
   template <class T, int NB> __device__ __forceinline__ void pass(const Lds &L, int Le, int ICell, int Kv, int Lt0) const {
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
      for (int J = 0; J < N; ++J) {
         const Real Md = L.MDvS[Le * ME + J];
         if (Md == 0.0) // EdgeMask 0, or no local edge: Fm = 0.0 exactly, no cell is read
            continue;
         const bool IsC0 = Md < 0.0;
         const int Nb    = L.Nbr[Le * ME + J];
         const T Hn      = ldk<T>(HOld, Nb, K, Kv);
         const T Ue      = ldk<T>(U, L.Edge[Le * ME + J], K, Kv);
         const T Fm      = massFlux<T>(IsC0 ? -Md : Md, IsC0, Upwind != 0, Hc, Hn, Ue);
#pragma unroll
         for (int B = 0; B < NB; ++B) {
            const T Pn = ldk<T>(Tr + (Lt0 + B) * CStride, Nb, K, Kv);
            const T P0 = IsC0 ? Pc[B] : Pn, P1 = IsC0 ? Pn : Pc[B];
            const T FLow  = lowFlux(Fm, P0, P1);
            const T FHigh = Fm * (0.5 * (P0 + P1));
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
struct MonoFluxBody : MonoTables {
   static constexpr int TrBlock = 3;
   using Lds                    = MonoLds;
   int K, NT, Upwind;
   const Real *HOld, *U, *Tr, *SIn, *SOut;
   Real *Tend;
   template <class T, int NB> __device__ __forceinline__ void pass(const Lds &L, int Le, int ICell, int Kv, int Lt0) const {
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
      for (int J = 0; J < N; ++J) {
         const Real Md = L.MDvS[Le * ME + J];
         if (Md == 0.0)
            continue;
         const bool IsC0 = Md < 0.0;
         const int Nb    = L.Nbr[Le * ME + J];
         const T Hn      = ldk<T>(HOld, Nb, K, Kv);
         const T Ue      = ldk<T>(U, L.Edge[Le * ME + J], K, Kv);
         const T Fm      = massFlux<T>(IsC0 ? -Md : Md, IsC0, Upwind != 0, Hc, Hn, Ue);
#pragma unroll
         for (int B = 0; B < NB; ++B) {
            const T Pn  = ldk<T>(Tr + (Lt0 + B) * CStride, Nb, K, Kv);
            const T SIn_ = ldk<T>(SIn + (Lt0 + B) * CStride, Nb, K, Kv);
            const T SOn = ldk<T>(SOut + (Lt0 + B) * CStride, Nb, K, Kv);
            const T P0 = IsC0 ? Pc[B] : Pn, P1 = IsC0 ? Pn : Pc[B];
            const T SI0 = IsC0 ? SIc[B] : SIn_, SI1 = IsC0 ? SIn_ : SIc[B];
            const T SO0 = IsC0 ? SOc[B] : SOn, SO1 = IsC0 ? SOn : SOc[B];
            const T FLow  = lowFlux(Fm, P0, P1);
            const T FHigh = Fm * (0.5 * (P0 + P1));
            const T A     = FHigh - FLow;
            const T Sc    = selGe0(A, kmin(SO0, SI1), kmin(SI0, SO1));
            const T F     = FLow + Sc * A;
            Sum[B]        = Sum[B] + (IsC0 ? T(-F) : F); // s*F
         }
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

void launchMonotoneAdv(const MeshView &M, const MonotoneAdvArgs &A, hipStream_t S) {
   if (A.NTracers <= 0)
      return;
   MonoScaleBody B1{{M}, A.K, A.NTracers, A.FluxThicknessUpwind, A.Dt, A.HOld, A.HNew, A.NormalVelocity, A.Tracers,
                    A.ScaleIn, A.ScaleOut};
   launchTile(B1, M.NCellsAll, A.K, S);
   MonoFluxBody B2{{M}, A.K, A.NTracers, A.FluxThicknessUpwind, A.HOld, A.NormalVelocity, A.Tracers, A.ScaleIn, A.ScaleOut,
                   A.Tend};
   launchTile(B2, M.NCellsAll, A.K, S);
}

} // namespace OMEGA
