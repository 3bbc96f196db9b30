// KppKernels.hip -- the K-profile kernels behind Kpp (Kpp.h) on gfx950.
//
// compute: lanes along the rows of a column (level KMin + i on lane i) in the packed-column shape
// (kernels/PackedColumns.h), one launch of two phases with the column held in registers and LDS between them.
//   phase 1: each lane forms its term of the buoyancy difference, its shear to the top layer (the cell's edge slots in
//            ascending order; a slot's row is one coalesced run along the lanes, its top-layer value one address per
//            column) and the unresolved shear; the Hillis-Steele scan of the contract runs in two LDS buffers, one
//            barrier per pass, as many passes as the deepest column of the workgroup needs (a pass whose shift reaches
//            past a shorter column changes nothing of it, so the extra passes keep its bits); the first level whose
//            bulk Richardson number exceeds the critical one is an LDS atomicMin per column.
//   phase 2: the bulk Richardson numbers and depths stay in the two buffers; every lane of a column reads the two pairs
//            around the crossing (one address per column: a broadcast) and interpolates the same boundary-layer
//            depth, then rewrites its own interface if it lies inside the layer.
// Lane i of a column also zeroes level i of the two level outputs where that level is outside the column's range, so
// every entry of a row is written exactly once.  The shifted scan reads are consecutive doubles along the lanes: no
// lane-group conflicts.  The velocity scales branch on the sign of the buoyancy flux and on the cbrt regime per column.
//
// applyNonLocalTracerFlux: one lane per (owned cell, level), every tracer in the one launch.
#include "KppKernels.h"
#include "PackedColumns.h"

namespace OMEGA {

namespace {

constexpr int PointBlock = 256;

/// The turbulent velocity scale w(Sig, H) of Kpp.h for a column with friction velocity Us and buoyancy flux Bf;
/// Momentum: wM, else wS
template <bool Momentum> __device__ inline Real kppScale(Real Kappa, Real Us, Real Bf, Real Sig, Real H) {
   const Real U3 = (Us * Us) * Us;
   const Real Z  = ((Kappa * Sig) * H) * Bf;
   if (Bf >= 0.0) {
      const Real Den = U3 + 5.0 * Z;
      return Den > 0.0 ? ((Kappa * Us) * U3) / Den : 0.0;
   }
   if (Momentum) {
      if (Z >= KppZetaM * U3)
         return (Kappa * Us) * sqrt(sqrt(1.0 - (16.0 * Z) / U3));
      return Kappa * cbrt(KppAm * U3 - KppCm * Z);
   }
   if (Z >= KppZetaS * U3)
      return (Kappa * Us) * sqrt(1.0 - (16.0 * Z) / U3);
   return Kappa * cbrt(KppAs * U3 - KppCs * Z);
}

/// Dynamic LDS of one workgroup: two buffers of Rows doubles, the crossing level of each column, the pass count
size_t kppLdsBytes(const PackedShape &P) { return 2 * (size_t)P.Rows * sizeof(Real) + ((size_t)P.Sys + 1) * sizeof(int); }

__global__ void __launch_bounds__(TriDiagMaxRows) kppComputeKernel(KppComputeArgs A, PackedShape P, int Pitch, int PitchI) {
   extern __shared__ __attribute__((aligned(16))) Real Lds[];
   const int Rows = P.Rows;
   Real *Buf0 = Lds, *Buf1 = Lds + Rows;
   int *Crossing = reinterpret_cast<int *>(Lds + 2 * Rows); // [Sys]: the smallest level above the critical number
   int *Passes   = Crossing + P.Sys;                        // scan passes of the deepest column of the workgroup

   const PackedLane L = packedLane(P, A.K, A.NCellsSize);
   const int T = threadIdx.x, I = L.I; // row I of the column: level KMin + I
   const long C = L.Col;
   int KMin = 0, N = 0;
   if (L.InSys && C < A.NCellsAll) {
      KMin = A.MinLayer[C];
      N    = packedRows(KMin, A.MaxLayer[C], A.K);
   }
   const int KMax = KMin + N - 1;
   if (T == 0)
      *Passes = 0;
   __syncthreads();
   if (L.InSys && I == 0) {
      Crossing[L.S] = KMax + 1;
      if (N > 0)
         atomicMax(Passes, pcrLevels(N)); // ceil(log2 N): the passes s = 1, 2, 4, ... < N
   }
   __syncthreads();
   const int NPass = *Passes;
   const bool Act  = L.InSys && I < N;
   const int Lev   = KMin + I;
   const size_t Row = (size_t)C * Pitch, RowI = (size_t)C * PitchI;
   const Real Kappa = A.VonKarman, Eps = A.SurfaceLayerFraction, Ric = A.CritBulkRichardson;

   // ---- phase 1: the terms of the bulk Richardson number
   Real Us = 0, Bf = 0, Zs = 0, D = 0, Db = 0, DV2 = 0, Vt2 = 0;
   if (Act) {
      Us            = A.FrictionVelocity[C];
      Bf            = A.SurfaceBuoyancyFlux[C];
      Zs            = A.ZInterface[RowI + KMin];
      const Real Zm = A.ZMid[Row + Lev];
      D             = Zs - Zm;
      const Real N2 = A.N2[Row + Lev];
      if (I >= 1)
         Db = N2 * (A.ZMid[Row + Lev - 1] - Zm);
      const Real N2Below = Lev < KMax ? A.N2[Row + Lev + 1] : 0.0;
      const Real NMid    = 0.5 * (N2 + N2Below);
      const Real Nk      = sqrt(NMid > 0.0 ? NMid : 0.0);
      const Real InvA    = 1.0 / A.AreaCell[C];
      const int NEdges   = A.NEdgesOnCell[C];
      for (int J = 0; J < NEdges; ++J) {
         const int E     = A.EdgesOnCell[(size_t)C * A.MaxEdges + J];
         const Real F    = ((0.5 * A.DcEdge[E]) * A.DvEdge[E]) * InvA;
         const size_t Er = (size_t)E * Pitch;
         const Real Du   = A.Un[Er + KMin] - A.Un[Er + Lev];
         const Real Dv   = A.Ut[Er + KMin] - A.Ut[Er + Lev];
         DV2             = DV2 + F * ((Du * Du) + (Dv * Dv));
      }
      Vt2 = ((A.VtCoef * D) * Nk) * kppScale<false>(Kappa, Us, Bf, Eps, D);
   }
   // the inclusive scan down the column, every row from the values before the pass
   for (int Pass = 0; Pass < NPass; ++Pass) {
      Real *B = (Pass & 1) ? Buf1 : Buf0;
      if (T < Rows)
         B[T] = Db;
      __syncthreads();
      const int Shift = 1 << Pass;
      if (Act && I >= Shift)
         Db = Db + B[T - Shift];
   }
   Real Rib = 0;
   if (Act)
      Rib = (Db * D) / ((DV2 + Vt2) + 1.0e-10);
   __syncthreads(); // the last pass has been read: the buffers now hold Rib and d
   if (T < Rows) {
      Buf0[T] = Rib;
      Buf1[T] = D;
   }
   if (Act && I >= 1 && Rib > Ric)
      atomicMin(&Crossing[L.S], Lev);
   __syncthreads();

   // ---- phase 2: the depth of the boundary layer, then the interfaces inside it
   Real Hbl = 0;
   int Kb   = -1;
   if (Act) {
      Kb = Crossing[L.S];
      if (Kb > KMax) {
         Hbl = Zs - A.ZInterface[RowI + KMax + 1];
      } else {
         const int R   = T - I + (Kb - KMin); // the lane of level Kb
         const Real Rm = Buf0[R - 1], Rk = Buf0[R], Dm = Buf1[R - 1], Dk = Buf1[R];
         Hbl           = Dm + ((Ric - Rm) / (Rk - Rm)) * (Dk - Dm);
      }
   }
   if (L.InSys) {
      if (N == 0 || I < KMin || I > KMax) { // level I of the row is outside the column
         A.BulkRichardson[Row + I] = 0.0;
         A.NonLocalShape[Row + I]  = 0.0;
      }
      if (I == 0) {
         A.BoundaryLayerDepth[C] = Hbl;
         A.BoundaryLayerIndex[C] = Kb;
      }
   }
   if (Act) {
      A.BulkRichardson[Row + Lev] = Rib;
      Real Shape                  = 0.0;
      if (I >= 1) {
         const Real DI = Zs - A.ZInterface[RowI + Lev];
         if (DI < Hbl) {
            const Real Sig = DI / Hbl;
            const Real Sw  = (Bf < 0.0 && Sig > Eps) ? Eps : Sig;
            const Real G   = Sig * ((1.0 - Sig) * (1.0 - Sig));
            A.VertVisc[Row + Lev] = A.BackgroundViscosity + (Hbl * kppScale<true>(Kappa, Us, Bf, Sw, Hbl)) * G;
            A.VertDiff[Row + Lev] = A.BackgroundDiffusivity + (Hbl * kppScale<false>(Kappa, Us, Bf, Sw, Hbl)) * G;
            Shape                 = Bf < 0.0 ? A.NonLocalCoeff * G : 0.0;
         }
      }
      A.NonLocalShape[Row + Lev] = Shape;
   }
}

__global__ void __launch_bounds__(PointBlock)
    kppNonLocalKernel(int NCellsOwned, int K, int Pitch, const I4 *MinLayer, const I4 *MaxLayer, const Real *H,
                      const Real *NonLocalShape, Real *Tracers, int NTracers, size_t TrStride, Real Dt,
                      const Real *Flux, size_t FluxStride) {
   const long Idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
   if (Idx >= (long)NCellsOwned * K)
      return;
   const int C    = (int)(Idx / K);
   const int Lev  = (int)(Idx - (long)C * K);
   const int KMin = MinLayer[C], KMax = MaxLayer[C];
   if (!(KMin >= 0 && KMin <= KMax && KMax < K && Lev >= KMin && Lev <= KMax))
      return;
   const size_t At  = (size_t)C * Pitch + Lev;
   const Real Below = Lev < KMax ? NonLocalShape[At + 1] : 0.0;
   const Real Diff  = NonLocalShape[At] - Below;
   const Real Hk    = H[At];
   for (int Tr = 0; Tr < NTracers; ++Tr) {
      Real *Phi = Tracers + (size_t)Tr * TrStride + At;
      *Phi      = *Phi + ((Dt * Flux[(size_t)Tr * FluxStride + C]) * Diff) / Hk;
   }
}

} // namespace

void launchKppCompute(const KppComputeArgs &A, hipStream_t S) {
   requirePackedLayers("Kpp", A.K);
   if (A.NCellsSize <= 0)
      return;
   const PackedShape P(A.K);
   hipLaunchKernelGGL(kppComputeKernel, P.grid(A.NCellsSize), dim3(P.Threads), kppLdsBytes(P), S, A, P, levelPitch(A.K),
                      levelPitch(A.K + 1));
   HIP_CHECK(hipGetLastError());
}

void launchKppNonLocal(int NCellsOwned, int K, const I4 *MinLayer, const I4 *MaxLayer, const Real *H,
                       const Real *NonLocalShape, Real *Tracers, int NTracers, int TrRows, Real Dt,
                       const Real *SurfaceFlux, size_t FluxStride, hipStream_t S) {
   const long N = (long)NCellsOwned * K;
   if (N <= 0 || NTracers <= 0)
      return;
   const int Pitch = levelPitch(K);
   hipLaunchKernelGGL(kppNonLocalKernel, dim3((unsigned)((N + PointBlock - 1) / PointBlock)), dim3(PointBlock), 0, S,
                      NCellsOwned, K, Pitch, MinLayer, MaxLayer, H, NonLocalShape, Tracers, NTracers,
                      (size_t)TrRows * Pitch, Dt, SurfaceFlux, FluxStride);
   HIP_CHECK(hipGetLastError());
}

} // namespace OMEGA
