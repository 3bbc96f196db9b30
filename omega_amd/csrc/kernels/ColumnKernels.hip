// ColumnKernels.hip -- VertCoord (VertCoord.cpp:484-864) and Eos (Eos.h / Eos.cpp) on gfx950.
//
// One kernel template over a compile-time stage mask (ColumnKernels.h), on the column tile of LevelTile.h: a workgroup
// of 256 threads owns a tile of `Tile` consecutive cells, staged into LDS rows of odd pitch.  The sequential parts (the
// pressure and z-height scans, the target-thickness sums) run one lane per column out of LDS; the point-wise parts
// (equation of state, geopotential, target thickness) run with the lanes along the flat [cell][level] run.
//
// A single-stage instantiation (what VertCoord::computePressure, Eos::computeSpecVol, ... launch) and the fused
// instantiation (VertCoord::computeColumn) run the same stage code; the results agree bit for bit.
#include "ColumnKernels.h"
#include "LevelTile.h"

namespace OMEGA {

namespace {

/// Offsets (in doubles) of the LDS buffers a stage mask needs, for a tile of `T` columns:
///   H  LayerThickness (Pressure, ZHeight) or RefLayerThickness (TargetThickness)        [T][LP]
///   A  PressureInterface, then ZInterface (or the PressureInterface input of TargetThickness) [T][LP1]
///   B  PressureMid (or the pressure input of SpecVol), then ZMid (or the ZMid input of Geopotential) [T][LP]
///   S  SpecVol (ZHeight)                                                                 [T][LP]
///   then two per-column scalars [T] each and the per-column layer range (2 x T ints = T doubles)
struct ColLayout {
   int H, A, B, S, Sc, End;
   __host__ __device__ ColLayout(unsigned M, int T, int LP, int LP1) {
      const bool NeedH = M & (StagePressure | StageZHeight | StageTargetThickness);
      const bool NeedB = M & (StagePressure | StageSpecVol | StageSpecVolDisp | StageZHeight | StageGeopotential);
      const bool NeedS = M & StageZHeight;
      H   = 0;
      A   = H + (NeedH ? T * LP : 0);
      B   = A + (NeedH ? T * LP1 : 0);
      S   = B + (NeedB ? T * LP : 0);
      Sc  = S + (NeedS ? T * LP : 0);
      End = Sc + 3 * T;
   }
};

// ---- TEOS-10: the 75-term polynomial for specific volume of Roquet, Madec, McDougall and Barker (2015), "Accurate
// polynomial expressions for the density and specific volume of seawater using the TEOS-10 standard", Ocean
// Modelling 90, 29-43 (Appendix A.2, coefficients v_ijk; published data).  Reduced variables
//   ss = sqrt((SA + 24) / (40 * 35.16504 / 35)),  tt = CT / 40,  pp = p / 1e4 (p in dbar),
// v(SA, CT, p) = v0(pp) + delta(ss, tt, pp), delta = sum_k c_k(ss, tt) pp^k (k = 0..5), every polynomial evaluated
// in nested (Horner) form, innermost power first.
struct Teos10Coeffs {
   Real C0, C1, C2, C3, C4, C5;
};

__device__ inline Teos10Coeffs teos10Coeffs(Real Ct, Real Sa) {
   constexpr Real SAu = 40.0 * 35.16504 / 35.0, CTu = 40.0, DeltaS = 24.0;
   const Real Ss = sqrt((Sa + DeltaS) / SAu);
   const Real Tt = Ct / CTu;
   // v_ijk: i = power of ss, j = power of tt, k = power of pp
   constexpr Real V000 = 1.0769995862e-03, V100 = -3.1038981976e-04, V200 = 6.6928067038e-04,
                  V300 = -8.5047933937e-04, V400 = 5.8086069943e-04, V500 = -2.1092370507e-04,
                  V600 = 3.1932457305e-05, V010 = -1.5649734675e-05, V110 = 3.5009599764e-05,
                  V210 = -4.3592678561e-05, V310 = 3.4532461828e-05, V410 = -1.1959409788e-05,
                  V510 = 1.3864594581e-06, V020 = 2.7762106484e-05, V120 = -3.7435842344e-05,
                  V220 = 3.5907822760e-05, V320 = -1.8698584187e-05, V420 = 3.8595339244e-06,
                  V030 = -1.6521159259e-05, V130 = 2.4141479483e-05, V230 = -1.4353633048e-05,
                  V330 = 2.2863324556e-06, V040 = 6.9111322702e-06, V140 = -8.7595873154e-06,
                  V240 = 4.3703680598e-06, V050 = -8.0539615540e-07, V150 = -3.3052758900e-07,
                  V060 = 2.0543094268e-07;
   constexpr Real V001 = -1.6784136540e-05, V101 = 2.4262468747e-05, V201 = -3.4792460974e-05,
                  V301 = 3.7470777305e-05, V401 = -1.7322218612e-05, V501 = 3.0927427253e-06,
                  V011 = 1.8505765429e-05, V111 = -9.5677088156e-06, V211 = 1.1100834765e-05,
                  V311 = -9.8447117844e-06, V411 = 2.5909225260e-06, V021 = -1.1716606853e-05,
                  V121 = -2.3678308361e-07, V221 = 2.9283346295e-06, V321 = -4.8826139200e-07,
                  V031 = 7.9279656173e-06, V131 = -3.4558773655e-06, V231 = 3.1655306078e-07,
                  V041 = -3.4102187482e-06, V141 = 1.2956717783e-06, V051 = 5.0736766814e-07;
   constexpr Real V002 = 3.0623833435e-06, V102 = -5.8484432984e-07, V202 = -4.8122251597e-06,
                  V302 = 4.9263106998e-06, V402 = -1.7811974727e-06, V012 = -1.1736386731e-06,
                  V112 = -5.5699154557e-06, V212 = 5.4620748834e-06, V312 = -1.3544185627e-06,
                  V022 = 2.1305028740e-06, V122 = 3.9137387080e-07, V222 = -6.5731104067e-07,
                  V032 = -4.6132540037e-07, V132 = 7.7618888092e-09, V042 = -6.3352916514e-08;
   constexpr Real V003 = -3.8088938393e-07, V103 = 3.6310188515e-07, V203 = 1.6746303780e-08,
                  V013 = -3.6527006553e-07, V113 = -2.7295696237e-07, V023 = 2.8695905159e-07;
   constexpr Real V004 = 8.8302421514e-08, V104 = -1.1147125423e-07, V014 = 3.1454099902e-07;
   constexpr Real V005 = 4.2369007180e-09;
   Teos10Coeffs R;
   R.C5 = V005;
   R.C4 = V014 * Tt + V104 * Ss + V004;
   R.C3 = (V023 * Tt + V113 * Ss + V013) * Tt + (V203 * Ss + V103) * Ss + V003;
   R.C2 = (((V042 * Tt + V132 * Ss + V032) * Tt + (V222 * Ss + V122) * Ss + V022) * Tt +
           ((V312 * Ss + V212) * Ss + V112) * Ss + V012) * Tt +
          (((V402 * Ss + V302) * Ss + V202) * Ss + V102) * Ss + V002;
   R.C1 = ((((V051 * Tt + V141 * Ss + V041) * Tt + (V231 * Ss + V131) * Ss + V031) * Tt +
            ((V321 * Ss + V221) * Ss + V121) * Ss + V021) * Tt +
           (((V411 * Ss + V311) * Ss + V211) * Ss + V111) * Ss + V011) * Tt +
          ((((V501 * Ss + V401) * Ss + V301) * Ss + V201) * Ss + V101) * Ss + V001;
   R.C0 = (((((V060 * Tt + V150 * Ss + V050) * Tt + (V240 * Ss + V140) * Ss + V040) * Tt +
             ((V330 * Ss + V230) * Ss + V130) * Ss + V030) * Tt +
            (((V420 * Ss + V320) * Ss + V220) * Ss + V120) * Ss + V020) * Tt +
           ((((V510 * Ss + V410) * Ss + V310) * Ss + V210) * Ss + V110) * Ss + V010) * Tt +
          (((((V600 * Ss + V500) * Ss + V400) * Ss + V300) * Ss + V200) * Ss + V100) * Ss + V000;
   return R;
}

/// v(SA, CT, p) from the six pressure coefficients (held in registers: one set per lane and level)
__device__ inline Real teos10SpecVol(const Teos10Coeffs &Cf, Real P) {
   constexpr Real Pu = 1.0e4;
   // reference profile v0(pp) (Roquet et al. 2015, A.2)
   constexpr Real V00 = -4.4015007269e-05, V01 = 6.9232335784e-06, V02 = -7.5004675975e-07, V03 = 1.7009109288e-08,
                  V04 = -1.6884162004e-08, V05 = 1.9613503930e-09;
   const Real Pp    = P / Pu;
   const Real Ref   = (((((V05 * Pp + V04) * Pp + V03) * Pp + V02) * Pp + V01) * Pp + V00) * Pp;
   const Real Delta = ((((Cf.C5 * Pp + Cf.C4) * Pp + Cf.C3) * Pp + Cf.C2) * Pp + Cf.C1) * Pp + Cf.C0;
   return Ref + Delta;
}

__device__ inline Real linearSpecVol(const EosParams &E, Real Ct, Real Sa) {
   return 1.0 / (E.RhoT0S0 + (E.DRhoDT * Ct + E.DRhoDS * Sa));
}

template <unsigned M> __global__ __launch_bounds__(ColThreads) void columnKernel(ColumnArgs A, int Tile) {
   extern __shared__ Real Lds[];
   const int C0 = blockIdx.x * Tile;
   const int Nc = min(Tile, A.NCells - C0);
   const int K = A.K, P = A.Pitch, P1 = A.Pitch1;
   const int LP = ldsPitch(P), LP1 = ldsPitch(P1);
   const ColLayout L(M, Tile, LP, LP1);
   Real *LH = Lds + L.H, *LA = Lds + L.A, *LB = Lds + L.B, *LS = Lds + L.S;
   Real *Sc0 = Lds + L.Sc, *Sc1 = Sc0 + Tile;
   I4 *Lo = reinterpret_cast<I4 *>(Sc1 + Tile), *Hi = Lo + Tile;
   const int Tid = threadIdx.x;

   constexpr bool Press = M & StagePressure, SV = M & StageSpecVol, SVD = M & StageSpecVolDisp,
                  Zh = M & StageZHeight, Geo = M & StageGeopotential, Tgt = M & StageTargetThickness;

   // per-column active range (all levels without one: the equation of state); a column outside
   // 0 <= KMin <= KMax < K is left untouched by the range stages
   stageRanges(A.MinLayer, A.MaxLayer, C0, Nc, K, Lo, Hi);
   if (Geo && Tid < Nc) {
      Sc0[Tid] = A.Tidal ? A.Tidal[C0 + Tid] : 0.0;
      Sc1[Tid] = A.SAL ? A.SAL[C0 + Tid] : 0.0;
   }
   __syncthreads();
   const AllLevels All;
   const InRange Active{Lo, Hi}, ActiveP1{Lo, Hi, 1};

   // ---- stage the inputs
   if (Press || Zh)
      loadTile(A.LayerThick, P, C0, Nc, LH, LP, All);
   if (Press && (SV || SVD)) // the equation of state reads PressureMid on every level: keep what is there off the range
      loadTile(A.PMid, P, C0, Nc, LB, LP, [&](int C, int Kk) { return Kk < K && !Active(C, Kk); });
   if ((SV || SVD) && !Press)
      loadTile(A.PressureIn, P, C0, Nc, LB, LP, All);
   if (Zh && !SV)
      loadTile(A.SpecVolIn, P, C0, Nc, LS, LP, All);
   if (Geo && !Zh)
      loadTile(A.ZMidIn, P, C0, Nc, LB, LP, All);
   if (Tgt) {
      loadTile(A.PIntIn, P1, C0, Nc, LA, LP1, All);
      loadTile(A.RefThick, P, C0, Nc, LH, LP, All);
   }
   __syncthreads();

   // ---- computePressure (VertCoord.cpp:654-696): top-down sequential sum, one lane per column
   if (Press) {
      if (Tid < Nc && Lo[Tid] <= Hi[Tid]) {
         const int C = Tid, KMin = Lo[C], KMax = Hi[C];
         const Real Ps = A.SurfPressure ? A.SurfPressure[C0 + C] : 0.0;
         const Real GRho = A.Gravity * A.Rho0;
         Real Acc = 0.0;
         LA[C * LP1 + KMin] = Ps;
         for (int Kk = KMin; Kk <= KMax; ++Kk) {
            const Real Inc = GRho * LH[C * LP + Kk];
            Acc += Inc;
            const Real Pi = Ps + Acc;
            LA[C * LP1 + Kk + 1] = Pi;
            LB[C * LP + Kk]      = Pi - 0.5 * Inc;
         }
      }
      __syncthreads();
      storeTile(A.PInt, P1, C0, Nc, LA, LP1, ActiveP1);
      storeTile(A.PMid, P, C0, Nc, LB, LP, Active);
   }

   // ---- computeSpecVol / computeSpecVolDisp (Eos.cpp:113-176): every level of every column, lanes along the run
   if (SV || SVD) {
      const size_t Off = (size_t)C0 * P;
      const Real *Ct = A.ConservTemp + Off, *Sa = A.AbsSalinity + Off;
      const Real PScale = A.PScale;
      forPairs(Nc * P, [&](int I, bool Two) {
         const Pos2 Q(I, P);
         Real T0, T1, S0, S1;
         load2(Ct + I, Two, T0, T1);
         load2(Sa + I, Two, S0, S1);
         Real V[2] = {0.0, 0.0}, Vd[2] = {0.0, 0.0};
         const bool W[2] = {Q.K0 < K, Two && Q.K1 < K};
#pragma unroll
         for (int J = 0; J < 2; ++J) {
            const int C = J ? Q.C1 : Q.C0, Kk = J ? Q.K1 : Q.K0;
            const Real T = J ? T1 : T0, S = J ? S1 : S0;
            if (!W[J])
               continue;
            if (A.Eos.Teos10) {
               const Teos10Coeffs Cf = teos10Coeffs(T, S);
               if (SV)
                  V[J] = teos10SpecVol(Cf, LB[C * LP + Kk] * PScale);
               if (SVD) {
                  const int KD = max(0, min(Kk + A.KDisp, K - 1));
                  Vd[J] = teos10SpecVol(Cf, LB[C * LP + KD] * PScale);
               }
            } else {
               const Real Lin = linearSpecVol(A.Eos, T, S);
               V[J] = Lin, Vd[J] = Lin;
            }
            if (Zh)
               LS[C * LP + Kk] = V[J];
         }
         if (SV)
            store2(A.SpecVol + Off + I, W[0], W[1], V[0], V[1]);
         if (SVD)
            store2(A.SpecVolDisp + Off + I, W[0], W[1], Vd[0], Vd[1]);
      });
      if (blockIdx.x == 0) // the sentinel row (the reference zero-fills the whole array first)
         for (int Kk = Tid; Kk < K; Kk += ColThreads) {
            if (SV)
               A.SpecVol[(size_t)A.NCells * P + Kk] = 0.0;
            if (SVD)
               A.SpecVolDisp[(size_t)A.NCells * P + Kk] = 0.0;
         }
   }

   // ---- computeZHeight (VertCoord.cpp:700-739): bottom-up sequential sum, one lane per column
   if (Zh) {
      __syncthreads(); // LS complete; LA / LB no longer read by the stores above
      if (Tid < Nc && Lo[Tid] <= Hi[Tid]) {
         const int C = Tid, KMin = Lo[C], KMax = Hi[C];
         const Real NegBot = -A.BottomDepth[C0 + C];
         Real Acc = 0.0;
         LA[C * LP1 + KMax + 1] = NegBot;
         for (int Kk = KMax; Kk >= KMin; --Kk) {
            const Real Dz = (A.Rho0 * LS[C * LP + Kk]) * LH[C * LP + Kk];
            Acc += Dz;
            const Real Zi = NegBot + Acc;
            LA[C * LP1 + Kk] = Zi;
            LB[C * LP + Kk]  = Zi - 0.5 * Dz;
         }
      }
      __syncthreads();
      storeTile(A.ZInt, P1, C0, Nc, LA, LP1, ActiveP1);
      storeTile(A.ZMid, P, C0, Nc, LB, LP, Active);
   }

   // ---- computeGeopotential (VertCoord.cpp:743-781): point-wise on the active levels
   if (Geo) {
      Real *G = A.GeoMid + (size_t)C0 * P;
      const Real Grav = A.Gravity;
      forPairs(Nc * P, [&](int I, bool Two) {
         const Pos2 Q(I, P);
         const bool W0 = Active(Q.C0, Q.K0), W1 = Two && Active(Q.C1, Q.K1);
         const Real G0 = W0 ? ((Grav * LB[Q.C0 * LP + Q.K0]) + Sc0[Q.C0]) + Sc1[Q.C0] : 0.0;
         const Real G1 = W1 ? ((Grav * LB[Q.C1 * LP + Q.K1]) + Sc0[Q.C1]) + Sc1[Q.C1] : 0.0;
         store2(G + I, W0, W1, G0, G1);
      });
   }

   // ---- computeTargetThickness (VertCoord.cpp:785-838): two ascending sums per column, then point-wise
   if (Tgt) {
      if (Tid < Nc && Lo[Tid] <= Hi[Tid]) {
         const int C = Tid, KMin = Lo[C], KMax = Hi[C];
         Real SumWh = 0.0, SumRef = 0.0;
         for (int Kk = KMin; Kk <= KMax; ++Kk) {
            const Real R = LH[C * LP + Kk];
            SumWh += A.MoveWeights[Kk] * R;
            SumRef += R;
         }
         Sc0[C] = (LA[C * LP1 + KMax + 1] - LA[C * LP1 + KMin]) / (A.Gravity * A.Rho0) - SumRef;
         Sc1[C] = SumWh;
      }
      __syncthreads();
      Real *G = A.Target + (size_t)C0 * P;
      forPairs(Nc * P, [&](int I, bool Two) {
         const Pos2 Q(I, P);
         const bool W0 = Active(Q.C0, Q.K0), W1 = Two && Active(Q.C1, Q.K1);
         const Real T0 = W0 ? LH[Q.C0 * LP + Q.K0] * (1.0 + (Sc0[Q.C0] * A.MoveWeights[Q.K0]) / Sc1[Q.C0]) : 0.0;
         const Real T1 = W1 ? LH[Q.C1 * LP + Q.K1] * (1.0 + (Sc0[Q.C1] * A.MoveWeights[Q.K1]) / Sc1[Q.C1]) : 0.0;
         store2(G + I, W0, W1, T0, T1);
      });
   }
}

__global__ void minMaxLayerKernel(int NAll, int NCellsOn, const I4 *CellsOn, const I4 *MinLayerCell,
                                  const I4 *MaxLayerCell, int NVertLayersP1, I4 *MinTop, I4 *MinBot, I4 *MaxTop,
                                  I4 *MaxBot) {
   const int I = blockIdx.x * blockDim.x + threadIdx.x;
   if (I > NAll)
      return;
   if (I == NAll) { // sentinel row
      MinTop[I] = NVertLayersP1, MinBot[I] = NVertLayersP1, MaxTop[I] = -1, MaxBot[I] = -1;
      return;
   }
   I4 Top = 0, Bot = 0, MxTop = 0, MxBot = 0;
   for (int J = 0; J < NCellsOn; ++J) {
      const I4 C = CellsOn[(size_t)I * NCellsOn + J];
      const I4 Mn = MinLayerCell[C], Mx = MaxLayerCell[C];
      const bool Land = Mx == -1;
      const I4 T = Land ? NVertLayersP1 : Mn, B = Land ? 0 : Mn;
      Top   = J == 0 ? T : min(Top, T);
      Bot   = J == 0 ? B : max(Bot, B);
      MxTop = J == 0 ? Mx : min(MxTop, Mx);
      MxBot = J == 0 ? Mx : max(MxBot, Mx);
   }
   MinTop[I] = Top, MinBot[I] = Bot, MaxTop[I] = MxTop, MaxBot[I] = MxBot;
}

template <unsigned M> void launchMask(const ColumnArgs &A, int Tile, size_t Bytes, hipStream_t S) {
   hipLaunchKernelGGL(columnKernel<M>, dim3((A.NCells + Tile - 1) / Tile), dim3(ColThreads), Bytes, S, A, Tile);
}

constexpr unsigned FusedMask = StagePressure | StageSpecVol | StageZHeight | StageGeopotential;

} // namespace

void launchColumn(unsigned Mask, const ColumnArgs &A, hipStream_t S) {
   OMEGA_REQUIRE(A.NCells > 0 && A.K > 0, "column kernel: empty mesh or column");
   const int LP = ldsPitch(A.Pitch), LP1 = ldsPitch(A.Pitch1);
   const int Tile = pickColumnTile([&](int T) { return ColLayout(Mask, T, LP, LP1).End; });
   OMEGA_REQUIRE(Tile >= 2, "column kernel: NVertLayers " + std::to_string(A.K) + " is too long for the LDS tile");
   const size_t Bytes = (size_t)ColLayout(Mask, Tile, LP, LP1).End * sizeof(Real);
   switch (Mask) {
   case StagePressure: launchMask<StagePressure>(A, Tile, Bytes, S); break;
   case StageSpecVol: launchMask<StageSpecVol>(A, Tile, Bytes, S); break;
   case StageSpecVolDisp: launchMask<StageSpecVolDisp>(A, Tile, Bytes, S); break;
   case StageZHeight: launchMask<StageZHeight>(A, Tile, Bytes, S); break;
   case StageGeopotential: launchMask<StageGeopotential>(A, Tile, Bytes, S); break;
   case StageTargetThickness: launchMask<StageTargetThickness>(A, Tile, Bytes, S); break;
   case FusedMask: launchMask<FusedMask>(A, Tile, Bytes, S); break;
   case FusedMask | StageSpecVolDisp: launchMask<FusedMask | StageSpecVolDisp>(A, Tile, Bytes, S); break;
   default: OMEGA_ABORT("column kernel: stage combination " + std::to_string(Mask) + " is not instantiated");
   }
   HIP_CHECK(hipGetLastError());
}

void launchMinMaxLayer(int NAll, int NCellsOn, const I4 *CellsOn, const I4 *MinLayerCell, const I4 *MaxLayerCell,
                       int NVertLayers, I4 *MinTop, I4 *MinBot, I4 *MaxTop, I4 *MaxBot, hipStream_t S) {
   hipLaunchKernelGGL(minMaxLayerKernel, dim3((NAll + 1 + 255) / 256), dim3(256), 0, S, NAll, NCellsOn, CellsOn,
                      MinLayerCell, MaxLayerCell, NVertLayers + 1, MinTop, MinBot, MaxTop, MaxBot);
   HIP_CHECK(hipGetLastError());
}

} // namespace OMEGA
