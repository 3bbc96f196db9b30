// VertMixKernels.hip -- the vertical-mixing kernels behind VertMix (VertMix.h) on gfx950.
//
// N^2 and the coefficients: one lane per (cell, level), lanes along the levels, so rows K-1 and K of a cell or edge are
// neighbours in one row and a wave reads whole runs of each edge's row.  The shear gather loops over the cell's edges
// in ascending slot order.
//
// The implicit solves: lanes along the rows of a column (level KMin + i on lane i) in the packed-column shape
// (kernels/PackedColumns.h), as the PCR array launcher (kernels/TriDiagKernels.hip).  A lane assembles its row of G and H
// once and solves every right-hand side of the column with pcrDiffSolveRowMulti
// (kernels/TriDiagKernels.h): the G / H recursion, and with it every division except the last, is done once per
// column instead of once per tracer.  Columns of one workgroup have different depths: the workgroup loops to the
// largest level count among them (packedLevels) and each lane stops updating after its own.
//
// The forced solves (VertMix.h) are further instantiations of the same kernel: the boundary terms change one diagonal
// entry and one right-hand-side entry per column, read by the lane of row 0 or row N-1; nothing is added per level.
#include "PackedColumns.h"
#include "VertMixKernels.h"

namespace OMEGA {

namespace {

constexpr int MixLdsBytes = 65536; // workspace limit of one solve workgroup
constexpr int PointBlock  = 256;

/// D^N: D*D*...*D left to right for an integer N in 1 .. 8 (the correctly rounded pow for these), else pow(D, N)
__device__ inline Real shearPow(Real D, Real N) {
   if (N >= 1.0 && N <= 8.0 && (Real)(int)N == N) {
      Real P = D;
      for (int I = 1; I < (int)N; ++I)
         P = P * D;
      return P;
   }
   return pow(D, N);
}

__global__ void __launch_bounds__(PointBlock)
    bruntVaisalaKernel(int NCellsAll, int NCellsSize, int K, int Pitch, const I4 *MinLayer, const I4 *MaxLayer,
                       Real GOverRho0, const Real *SpecVol, const Real *SpecVolDisp, const Real *ZMid, Real *N2) {
   const long Idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
   if (Idx >= (long)NCellsSize * K)
      return;
   const int C   = (int)(Idx / K);
   const int Lev = (int)(Idx - (long)C * K);
   const size_t Row = (size_t)C * Pitch;
   Real V           = 0;
   if (C < NCellsAll) {
      const int KMin = MinLayer[C], KMax = MaxLayer[C];
      if (KMin >= 0 && KMin <= KMax && KMax < K && Lev > KMin && Lev <= KMax)
         V = (GOverRho0 * ((1.0 / SpecVol[Row + Lev]) - (1.0 / SpecVolDisp[Row + Lev - 1]))) /
             (ZMid[Row + Lev - 1] - ZMid[Row + Lev]);
   }
   N2[Row + Lev] = V;
}

__global__ void __launch_bounds__(PointBlock) vertMixCoeffKernel(VertMixCoeffArgs A, int Pitch) {
   const long Idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
   if (Idx >= (long)A.NCellsSize * A.K)
      return;
   const int C   = (int)(Idx / A.K);
   const int Lev = (int)(Idx - (long)C * A.K);
   const size_t Row = (size_t)C * Pitch;
   Real Visc = 0, Diff = 0;
   if (C < A.NCellsAll) {
      const int KMin = A.MinLayer[C], KMax = A.MaxLayer[C];
      if (KMin >= 0 && KMin <= KMax && KMax < A.K && Lev > KMin && Lev <= KMax) {
         const Real N2 = A.N2[Row + Lev];
         Visc          = A.BackgroundViscosity;
         Diff          = A.BackgroundDiffusivity;
         if (A.EnableShear) {
            Real S2           = 0;
            const Real InvA   = 1.0 / A.AreaCell[C];
            const int NEdges  = A.NEdgesOnCell[C];
            for (int J = 0; J < NEdges; ++J) {
               const int E      = A.EdgesOnCell[(size_t)C * A.MaxEdges + J];
               const Real F     = ((0.5 * A.DcEdge[E]) * A.DvEdge[E]) * InvA;
               const size_t Er  = (size_t)E * Pitch + Lev;
               const Real Du    = A.Un[Er - 1] - A.Un[Er];
               const Real Dv    = A.Ut[Er - 1] - A.Ut[Er];
               S2               = S2 + F * ((Du * Du) + (Dv * Dv));
            }
            const Real Dz = A.ZMid[Row + Lev - 1] - A.ZMid[Row + Lev];
            S2            = S2 / (Dz * Dz);
            const Real S2c = S2 < 1.0e-12 ? 1.0e-12 : S2;
            Real Ri        = N2 / S2c;
            Ri             = Ri < 0.0 ? 0.0 : Ri;
            const Real D   = 1.0 + A.ShearAlpha * Ri;
            Visc           = Visc + A.ShearNuZero / shearPow(D, A.ShearExponent);
            Diff           = Diff + Visc / D;
         }
         if (A.EnableConvective && N2 < A.ConvectiveTriggerBVF) {
            Visc = Visc + A.ConvectiveDiffusivity;
            Diff = Diff + A.ConvectiveDiffusivity;
         }
      }
   }
   A.VertVisc[Row + Lev] = Visc;
   A.VertDiff[Row + Lev] = Diff;
}

/// One implicit-mixing launch: NCols columns (owned cells or owned edges), NRhs right-hand sides of RhsStride values
struct MixArgs {
   int NCols = 0, K = 0, Pitch = 0;
   const I4 *Lo = nullptr, *Hi = nullptr; ///< [column] level range
   const I4 *CellsOnEdge = nullptr;       ///< edges: [edge][2]
   const Real *H = nullptr, *Coef = nullptr; ///< [cell][Pitch]: thickness, VertDiff / VertVisc
   Real *X = nullptr;                        ///< [rhs][column][Pitch], solved in place
   int NRhs = 0;
   size_t RhsStride = 0;
   Real Dt = 0;
   // ---- read by the Forced instantiations only
   const Real *Flux = nullptr; ///< cells: [rhs][FluxStride] surface flux, or null
   size_t FluxStride = 0;
   VelocityForcingArgs F;      ///< edges
};

/// Forced: the boundary terms of VertMix.h's forced solves -- one lane per column each (row 0: the surface flux or
/// the wind stress on X; row N-1: the bottom drag on the diagonal) and the Rayleigh drag on every row's diagonal.
/// The diagonal goes to the solver where H stood; X = Hr * value keeps the thickness.
template <int Chunk, bool OnEdge, bool Forced>
__global__ void __launch_bounds__(TriDiagMaxRows) implicitMixKernel(MixArgs A, PackedShape P) {
   extern __shared__ Real Lds[];
   const PackedLane L = packedLane(P, A.K, A.NCols);
   const int S = L.S, I = L.I, Rows = P.Rows; // row I of the column: level Lo + I
   const long Col = L.Col;
   int Lo = 0, N = 0;
   if (L.InSys) {
      Lo = A.Lo[Col];
      N  = packedRows(Lo, A.Hi[Col], A.K);
   }
   const int NLevWg = packedLevels(L.InSys && I == 0, N);
   const bool Act   = L.InSys && I < N;

   Real G = 0, Hr = 0;
   const int Lev = Lo + I;
   if (Act) {
      if (OnEdge) {
         const size_t C1 = (size_t)A.CellsOnEdge[2 * Col] * A.Pitch, C2 = (size_t)A.CellsOnEdge[2 * Col + 1] * A.Pitch;
         Hr = 0.5 * (A.H[C1 + Lev] + A.H[C2 + Lev]);
         if (I < N - 1) {
            const Real Hn = 0.5 * (A.H[C1 + Lev + 1] + A.H[C2 + Lev + 1]);
            const Real Nu = 0.5 * (A.Coef[C1 + Lev + 1] + A.Coef[C2 + Lev + 1]);
            G             = (Nu * A.Dt) / ((Hn + Hr) / 2);
         }
      } else {
         const size_t C = (size_t)Col * A.Pitch;
         Hr             = A.H[C + Lev];
         if (I < N - 1)
            G = (A.Coef[C + Lev + 1] * A.Dt) / ((A.H[C + Lev + 1] + Hr) / 2);
      }
   }
   Real *X        = A.X + (size_t)Col * A.Pitch + Lev;
   const size_t R = A.RhsStride;
   if constexpr (!Forced) {
      pcrDiffSolveRowMulti<Chunk>(
          Act, I, N, NLevWg, G, Hr, A.NRhs, [=](int Tr) { return Hr * X[Tr * R]; },
          [=](int Tr, Real V) { X[Tr * R] = V; }, Lds + S * A.K, Rows);
   } else if constexpr (OnEdge) {
      Real D = Hr, Top = 0;
      bool HasTop = false;
      if (Act) {
         if (A.F.DtRayleigh != 0)
            D = D + A.F.DtRayleigh * Hr;
         if (I == N - 1 && A.F.DtBottomDrag != 0) {
            const Real Ub = X[0], Vb = A.F.Ut[(size_t)Col * A.Pitch + Lev]; // u before the solve
            D             = D + A.F.DtBottomDrag * sqrt((Ub * Ub) + (Vb * Vb));
         }
         if (I == 0 && A.F.Stress != nullptr) {
            Top    = (A.Dt * A.F.EdgeMask[Col]) * (A.F.Stress[Col] / A.F.Rho0);
            HasTop = true;
         }
      }
      pcrDiffSolveRowMulti<Chunk>(
          Act, I, N, NLevWg, G, D, A.NRhs,
          [=](int Tr) {
             const Real V = Hr * X[Tr * R];
             return HasTop ? V + Top : V;
          },
          [=](int Tr, Real V) { X[Tr * R] = V; }, Lds + S * A.K, Rows);
   } else {
      // One lane per column (row 0) reads the flux, once per tracer.  The lane keeps the byte offset of its column in a
      // flux row (NoFlux: no term), added to the uniform row address: one VGPR and no 64-bit address arithmetic.
      constexpr unsigned NoFlux = ~0u;
      const unsigned FluxOff    = (Act && I == 0 && A.Flux != nullptr) ? (unsigned)Col * (unsigned)sizeof(Real) : NoFlux;
      const Real *const Flux    = A.Flux;
      const unsigned Fs         = (unsigned)A.FluxStride; // a row of cells: 32 bits hold it
      const Real Dt             = A.Dt;
      pcrDiffSolveRowMulti<Chunk>(
          Act, I, N, NLevWg, G, Hr, A.NRhs,
          [=](int Tr) {
             const Real V = Hr * X[Tr * R];
             if (FluxOff == NoFlux)
                return V;
             const char *Row = reinterpret_cast<const char *>(Flux + (size_t)((unsigned)Tr * Fs));
             return V + Dt * *reinterpret_cast<const Real *>(Row + FluxOff);
          },
          [=](int Tr, Real V) { X[Tr * R] = V; }, Lds + S * A.K, Rows);
   }
}

/// Right-hand sides per pass: the fewest of 1, 2, 4, 6, 8 that hold NRhs, within the LDS limit
int mixChunk(int NRhs, int Rows) {
   const int Cap      = (MixLdsBytes / (int)sizeof(Real) / Rows - 4) / 2;
   const int Opts[5]  = {1, 2, 4, 6, 8};
   int C              = 1;
   for (int O : Opts)
      if (O <= Cap && (C < NRhs))
         C = O;
   return C;
}

template <bool OnEdge, bool Forced> void launchMix(const MixArgs &A, hipStream_t Str) {
   requirePackedLayers("VertMix", A.K);
   if (A.NCols <= 0 || A.NRhs <= 0)
      return;
   const PackedShape P(A.K);
   const int Chunk = mixChunk(A.NRhs, P.Rows);
   const dim3 Grid = P.grid(A.NCols);
   const size_t Bytes = (size_t)(4 + 2 * Chunk) * P.Rows * sizeof(Real);
   switch (Chunk) {
   case 1: hipLaunchKernelGGL((implicitMixKernel<1, OnEdge, Forced>), Grid, dim3(P.Threads), Bytes, Str, A, P); break;
   case 2: hipLaunchKernelGGL((implicitMixKernel<2, OnEdge, Forced>), Grid, dim3(P.Threads), Bytes, Str, A, P); break;
   case 4: hipLaunchKernelGGL((implicitMixKernel<4, OnEdge, Forced>), Grid, dim3(P.Threads), Bytes, Str, A, P); break;
   case 6: hipLaunchKernelGGL((implicitMixKernel<6, OnEdge, Forced>), Grid, dim3(P.Threads), Bytes, Str, A, P); break;
   default: hipLaunchKernelGGL((implicitMixKernel<8, OnEdge, Forced>), Grid, dim3(P.Threads), Bytes, Str, A, P);
   }
   HIP_CHECK(hipGetLastError());
}

} // namespace

void launchBruntVaisala(int NCellsAll, int NCellsSize, int K, const I4 *MinLayer, const I4 *MaxLayer, Real GOverRho0,
                        const Real *SpecVol, const Real *SpecVolDisp, const Real *ZMid, Real *N2, hipStream_t S) {
   const long N = (long)NCellsSize * K;
   if (N <= 0)
      return;
   hipLaunchKernelGGL(bruntVaisalaKernel, dim3((unsigned)((N + PointBlock - 1) / PointBlock)), dim3(PointBlock), 0, S,
                      NCellsAll, NCellsSize, K, levelPitch(K), MinLayer, MaxLayer, GOverRho0, SpecVol, SpecVolDisp,
                      ZMid, N2);
   HIP_CHECK(hipGetLastError());
}

void launchVertMixCoeffs(const VertMixCoeffArgs &A, hipStream_t S) {
   const long N = (long)A.NCellsSize * A.K;
   if (N <= 0)
      return;
   hipLaunchKernelGGL(vertMixCoeffKernel, dim3((unsigned)((N + PointBlock - 1) / PointBlock)), dim3(PointBlock), 0, S,
                      A, levelPitch(A.K));
   HIP_CHECK(hipGetLastError());
}

void launchTracerVertMix(int NCellsOwned, int K, const I4 *MinLayer, const I4 *MaxLayer, const Real *H,
                         const Real *VertDiff, Real *Tracers, int NTracers, int TrRows, Real Dt, hipStream_t S) {
   MixArgs A;
   A.NCols = NCellsOwned, A.K = K, A.Pitch = levelPitch(K);
   A.Lo = MinLayer, A.Hi = MaxLayer;
   A.H = H, A.Coef = VertDiff, A.X = Tracers;
   A.NRhs = NTracers, A.RhsStride = (size_t)TrRows * A.Pitch, A.Dt = Dt;
   launchMix<false, false>(A, S);
}

void launchVelocityVertMix(int NEdgesOwned, int K, const I4 *CellsOnEdge, const I4 *MinLayerEdgeBot,
                           const I4 *MaxLayerEdgeTop, const Real *H, const Real *VertVisc, Real *U, Real Dt,
                           hipStream_t S) {
   MixArgs A;
   A.NCols = NEdgesOwned, A.K = K, A.Pitch = levelPitch(K);
   A.Lo = MinLayerEdgeBot, A.Hi = MaxLayerEdgeTop, A.CellsOnEdge = CellsOnEdge;
   A.H = H, A.Coef = VertVisc, A.X = U;
   A.NRhs = 1, A.RhsStride = 0, A.Dt = Dt;
   launchMix<true, false>(A, S);
}

void launchTracerVertMixForced(int NCellsOwned, int K, const I4 *MinLayer, const I4 *MaxLayer, const Real *H,
                               const Real *VertDiff, Real *Tracers, int NTracers, int TrRows, Real Dt,
                               const Real *SurfaceFlux, size_t FluxStride, hipStream_t S) {
   MixArgs A;
   A.NCols = NCellsOwned, A.K = K, A.Pitch = levelPitch(K);
   A.Lo = MinLayer, A.Hi = MaxLayer;
   A.H = H, A.Coef = VertDiff, A.X = Tracers;
   A.NRhs = NTracers, A.RhsStride = (size_t)TrRows * A.Pitch, A.Dt = Dt;
   // the kernel addresses a flux row with 32-bit offsets (values across the tracers, bytes within a row)
   OMEGA_REQUIRE(SurfaceFlux == nullptr || ((size_t)NCellsOwned <= FluxStride && FluxStride <= 0x1FFFFFFFu &&
                                            (size_t)NTracers * FluxStride <= 0xFFFFFFFFu),
                 "VertMix: the surface flux array is too large for the forced tracer solve");
   A.Flux = SurfaceFlux, A.FluxStride = FluxStride;
   launchMix<false, true>(A, S);
}

void launchVelocityVertMixForced(int NEdgesOwned, int K, const I4 *CellsOnEdge, const I4 *MinLayerEdgeBot,
                                 const I4 *MaxLayerEdgeTop, const Real *H, const Real *VertVisc, Real *U, Real Dt,
                                 const VelocityForcingArgs &F, hipStream_t S) {
   OMEGA_REQUIRE(F.DtBottomDrag == 0 || F.Ut != nullptr, "VertMix: bottom drag needs the tangential velocity");
   OMEGA_REQUIRE(F.Stress == nullptr || F.EdgeMask != nullptr, "VertMix: a stress array needs the edge mask");
   MixArgs A;
   A.NCols = NEdgesOwned, A.K = K, A.Pitch = levelPitch(K);
   A.Lo = MinLayerEdgeBot, A.Hi = MaxLayerEdgeTop, A.CellsOnEdge = CellsOnEdge;
   A.H = H, A.Coef = VertVisc, A.X = U;
   A.NRhs = 1, A.RhsStride = 0, A.Dt = Dt;
   A.F = F;
   launchMix<true, true>(A, S);
}

} // namespace OMEGA
