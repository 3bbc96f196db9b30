// MonotoneAdv.cpp -- see MonotoneAdv.h.
#include "MonotoneAdv.h"
#include "Pacer.h"
#include "kernels/MonotoneAdvKernels.h"

#include <algorithm>
#include <cmath>

namespace OMEGA {

MonotoneAdv::MonotoneAdv(const std::string &Name_, const HorzMesh *Mesh_, int K, int MaxTracers_, const MonotoneAdvConfig &C)
    : NVertLayers(K), MaxTracers(MaxTracers_), Config(C), Mesh(Mesh_), Name(Name_) {
   OMEGA_REQUIRE(Mesh != nullptr, "MonotoneAdv: mesh is NULL");
   OMEGA_REQUIRE(!Mesh->HostOnly, "MonotoneAdv: the mesh was created host-only: no device arrays, compute is unavailable");
   OMEGA_REQUIRE(NVertLayers >= 1, "MonotoneAdv: NVertLayers = " + std::to_string(NVertLayers) + " is not a layer count (>= 1)");
   OMEGA_REQUIRE(MaxTracers >= 1, "MonotoneAdv: MaxTracers = " + std::to_string(MaxTracers) + " is not a tracer count (>= 1)");
   ScaleIn   = Array3DReal::levels("ScaleIn", MaxTracers, Mesh->NCellsSize, NVertLayers);
   ScaleOut  = Array3DReal::levels("ScaleOut", MaxTracers, Mesh->NCellsSize, NVertLayers);
   ScaleInH  = HostArrayReal(MaxTracers, Mesh->NCellsSize, NVertLayers);
   ScaleOutH = HostArrayReal(MaxTracers, Mesh->NCellsSize, NVertLayers);
}

void MonotoneAdv::attachVertAdv(const VertAdv *V) {
   OMEGA_REQUIRE(V == nullptr || (V->Mesh == Mesh && V->NVertLayers == NVertLayers),
                 "MonotoneAdv::attachVertAdv: the VertAdv was built for another mesh or layer count");
   VAdv = V;
}

// ---- the tables of the high-order flux (MonotoneAdv.h) ----
namespace {
struct V3 {
   Real X, Y, Z;
};
V3 operator-(V3 A, V3 B) { return {A.X - B.X, A.Y - B.Y, A.Z - B.Z}; }
V3 operator*(Real S, V3 A) { return {S * A.X, S * A.Y, S * A.Z}; }
Real dot(V3 A, V3 B) { return A.X * B.X + A.Y * B.Y + A.Z * B.Z; }
Real norm(V3 A) { return std::sqrt(dot(A, A)); }
V3 cross(V3 A, V3 B) { return {A.Y * B.Z - A.Z * B.Y, A.Z * B.X - A.X * B.Z, A.X * B.Y - A.Y * B.X}; }
Real minImage(Real D, Real Period) { return Period > 0.0 ? D - Period * std::nearbyint(D / Period) : D; }

/// The pseudo-inverse of the N x 5 matrix A (row-major, N >= 5) by Householder QR: Pinv [5][N] = R^-1 Q^T.  False if A
/// has not full column rank: the smallest |R(k,k)| is not above 1e-8 times the largest.
bool pseudoInverse5(std::vector<Real> A, int N, std::vector<Real> &Pinv) {
   constexpr int P = 5;
   std::vector<Real> Qt((size_t)N * N, 0.0); // Q^T, built by applying the reflections to the identity
   for (int I = 0; I < N; ++I)
      Qt[(size_t)I * N + I] = 1.0;
   for (int K = 0; K < P; ++K) {
      Real Nrm = 0.0;
      for (int I = K; I < N; ++I)
         Nrm += A[I * P + K] * A[I * P + K];
      Nrm = std::sqrt(Nrm);
      if (Nrm == 0.0)
         return false;
      const Real Alpha = A[K * P + K] > 0.0 ? -Nrm : Nrm;
      std::vector<Real> V(N, 0.0);
      for (int I = K; I < N; ++I)
         V[I] = A[I * P + K];
      V[K] -= Alpha;
      Real VV = 0.0;
      for (int I = K; I < N; ++I)
         VV += V[I] * V[I];
      if (VV == 0.0)
         continue;
      for (int J = K; J < P; ++J) { // A <- (I - 2 v v^T / v^T v) A
         Real S = 0.0;
         for (int I = K; I < N; ++I)
            S += V[I] * A[I * P + J];
         S = 2.0 * S / VV;
         for (int I = K; I < N; ++I)
            A[I * P + J] -= S * V[I];
      }
      for (int J = 0; J < N; ++J) {
         Real S = 0.0;
         for (int I = K; I < N; ++I)
            S += V[I] * Qt[(size_t)I * N + J];
         S = 2.0 * S / VV;
         for (int I = K; I < N; ++I)
            Qt[(size_t)I * N + J] -= S * V[I];
      }
   }
   Real RMin = std::abs(A[0]), RMax = RMin;
   for (int K = 1; K < P; ++K) {
      RMin = std::min(RMin, std::abs(A[K * P + K]));
      RMax = std::max(RMax, std::abs(A[K * P + K]));
   }
   if (!(RMin > 1.0e-8 * RMax))
      return false;
   Pinv.assign((size_t)P * N, 0.0);
   for (int J = 0; J < N; ++J) // back substitution of R x = (Q^T)[0 .. 5)[J]
      for (int K = P - 1; K >= 0; --K) {
         Real S = Qt[(size_t)K * N + J];
         for (int M = K + 1; M < P; ++M)
            S -= A[K * P + M] * Pinv[(size_t)M * N + J];
         Pinv[(size_t)K * N + J] = S / A[K * P + K];
      }
   return true;
}
} // namespace

void MonoHighOrderTables::build(const HorzMesh &M, const MonoHighOrderConfig &C) {
   OMEGA_REQUIRE(C.HorzOrder >= 2 && C.HorzOrder <= 4,
                 "MonotoneAdv::setHorzOrder: HorzOrder = " + std::to_string(C.HorzOrder) + " is not 2, 3 or 4");
   OMEGA_REQUIRE(C.HorzOrder != 3 || (C.Coef3rdOrder > 0.0 && C.Coef3rdOrder <= 1.0),
                 "MonotoneAdv::setHorzOrder: Coef3rdOrder = " + std::to_string(C.Coef3rdOrder) + " is outside (0, 1]");
   for (Real X : {C.SphereRadius, C.XPeriod, C.YPeriod})
      OMEGA_REQUIRE(std::isfinite(X) && X >= 0.0, "MonotoneAdv::setHorzOrder: a radius or period of " + std::to_string(X) +
                                                      " is negative or not finite");
   if (C.HorzOrder == 2)
      return;
   const int NC = M.NCellsAll, NE = M.NEdgesAll, ME = M.MaxEdges;
   const Real R = C.SphereRadius;
   auto pos     = [&](int I) { return V3{M.XCellH(I), M.YCellH(I), M.ZCellH(I)}; };
   auto across  = [&](int Cell, int E) { return M.CellsOnEdgeH(E, 0) == Cell ? M.CellsOnEdgeH(E, 1) : M.CellsOnEdgeH(E, 0); };
   Fit = HostArrayReal(M.NCellsSize, 1, 1, 0.0), Weight = HostArrayReal(M.NCellsSize, ME, 3, 0.0);
   Own = HostArrayReal(M.NCellsSize, ME, 3, 0.0), Acr = HostArrayReal(M.NCellsSize, ME, 3, 0.0);
   std::vector<Real> Dir((size_t)M.NCellsSize * ME * 2, 0.0); // (cs, sn) of every slot of a fit cell
   std::vector<Real> A, Pinv, DX(ME), DY(ME);
   for (int Cell = 0; Cell < NC; ++Cell) {
      const int N = M.NEdgesOnCellH(Cell);
      bool Ok     = N >= 5;
      for (int J = 0; J < N && Ok; ++J) {
         const int E = M.EdgesOnCellH(Cell, J);
         Ok          = E >= 0 && E < NE && M.EdgeMask1DH(E) != 0.0;
         if (Ok) {
            const int Nb = across(Cell, E);
            Ok           = Nb >= 0 && Nb < NC;
         }
      }
      if (!Ok)
         continue;
      // the frame of the tangent plane at the cell
      const V3 Xc = pos(Cell);
      V3 E1{1.0, 0.0, 0.0}, E2{0.0, 1.0, 0.0}, Rc{0.0, 0.0, 1.0};
      if (R > 0.0) {
         Rc            = (1.0 / norm(Xc)) * Xc;
         const V3 Axis = std::abs(Rc.Z) < 0.9 ? V3{0.0, 0.0, 1.0} : V3{1.0, 0.0, 0.0};
         E1            = cross(Axis, Rc);
         E1            = (1.0 / norm(E1)) * E1;
         E2            = cross(Rc, E1);
      }
      Real LSum = 0.0;
      for (int J = 0; J < N; ++J) {
         const V3 Xn = pos(across(Cell, M.EdgesOnCellH(Cell, J)));
         V3 D        = Xn - Xc;
         if (R > 0.0) { // azimuthal equidistant: the tangential direction, the arc's length
            const V3 Rn  = (1.0 / norm(Xn)) * Xn;
            const V3 Tan = D - dot(D, Rc) * Rc;
            const Real Arc = R * std::atan2(norm(cross(Rc, Rn)), dot(Rc, Rn)); // (acos(r_c.r_n), well conditioned)
            D              = (Arc / norm(Tan)) * Tan;
         } else {
            D.X = minImage(D.X, C.XPeriod), D.Y = minImage(D.Y, C.YPeriod), D.Z = 0.0;
         }
         DX[J] = dot(D, E1), DY[J] = dot(D, E2);
         LSum += std::hypot(DX[J], DY[J]);
      }
      const Real L = LSum / N;
      A.assign((size_t)N * 5, 0.0);
      for (int J = 0; J < N; ++J) {
         const Real X = DX[J] / L, Y = DY[J] / L;
         Real *Row    = &A[(size_t)J * 5];
         Row[0] = X, Row[1] = Y, Row[2] = X * X, Row[3] = X * Y, Row[4] = Y * Y;
      }
      if (!pseudoInverse5(A, N, Pinv))
         continue;
      Fit(Cell) = 1.0;
      for (int J = 0; J < N; ++J) {
         Real *W = &Weight.V[((size_t)Cell * ME + J) * 3];
         W[0] = 2.0 * Pinv[(size_t)2 * N + J] / (L * L), W[1] = Pinv[(size_t)3 * N + J] / (L * L);
         W[2]       = 2.0 * Pinv[(size_t)4 * N + J] / (L * L);
         const Real Len = std::hypot(DX[J], DY[J]);
         Dir[((size_t)Cell * ME + J) * 2] = DX[J] / Len, Dir[((size_t)Cell * ME + J) * 2 + 1] = DY[J] / Len;
      }
   }
   // the direction coefficients of the high edges: a cell's own, then the copies of the cell across
   auto high = [&](int E) {
      return M.EdgeMask1DH(E) != 0.0 && Fit(M.CellsOnEdgeH(E, 0)) != 0.0 && Fit(M.CellsOnEdgeH(E, 1)) != 0.0;
   };
   for (int Cell = 0; Cell < NC; ++Cell) {
      if (Fit(Cell) == 0.0)
         continue;
      for (int J = 0; J < M.NEdgesOnCellH(Cell); ++J) {
         const int E = M.EdgesOnCellH(Cell, J);
         if (!high(E))
            continue;
         const Real Cs = Dir[((size_t)Cell * ME + J) * 2], Sn = Dir[((size_t)Cell * ME + J) * 2 + 1];
         const Real F  = M.DcEdgeH(E) * M.DcEdgeH(E) / 12.0;
         Real *Q       = &Own.V[((size_t)Cell * ME + J) * 3];
         Q[0] = F * (Cs * Cs), Q[1] = F * (2.0 * Cs * Sn), Q[2] = F * (Sn * Sn);
      }
   }
   for (int Cell = 0; Cell < NC; ++Cell) {
      if (Fit(Cell) == 0.0)
         continue;
      for (int J = 0; J < M.NEdgesOnCellH(Cell); ++J) {
         const int E = M.EdgesOnCellH(Cell, J);
         if (!high(E))
            continue;
         const int Nb = across(Cell, E);
         for (int J2 = 0; J2 < M.NEdgesOnCellH(Nb); ++J2)
            if (M.EdgesOnCellH(Nb, J2) == E)
               for (int X = 0; X < 3; ++X)
                  Acr.V[((size_t)Cell * ME + J) * 3 + X] = Own.V[((size_t)Nb * ME + J2) * 3 + X];
      }
   }
}

void MonotoneAdv::setHorzOrder(const MonoHighOrderConfig &C) {
   MonoHighOrderTables T;
   T.build(*Mesh, C); // (refuses what the configuration must not be, at every order)
   HighOrder = C;
   if (C.HorzOrder == 2)
      return;
   const HorzMesh &M = *Mesh;
   if (HessWeight.Ptr == nullptr) { // the first time: the only allocation
      HessWeight    = Array3DReal("HessWeight", M.NCellsSize, M.MaxEdges, 3);
      EdgeDirOwn    = Array3DReal("EdgeDirOwn", M.NCellsSize, M.MaxEdges, 3);
      EdgeDirAcross = Array3DReal("EdgeDirAcross", M.NCellsSize, M.MaxEdges, 3);
      FitCell       = Array1DReal("FitCell", M.NCellsSize);
      Hess          = Array3DReal::levels("Hess", MaxTracers * 3, M.NCellsSize, NVertLayers);
   }
   HIP_CHECK(hipDeviceSynchronize()); // (a call in flight may still read the tables)
   OMEGA::copyToDevice(HessWeight, T.Weight.data());
   OMEGA::copyToDevice(EdgeDirOwn, T.Own.data());
   OMEGA::copyToDevice(EdgeDirAcross, T.Acr.data());
   OMEGA::copyToDevice(FitCell, T.Fit.data());
}

/// a tracer array of the kernel's plane stride: exactly NCellsSize rows per tracer
static void requirePlanes(const Array3DReal &A, int NT, int Rows, int K, const char *What) {
   requireLevelArray("MonotoneAdv", A, NT, Rows, K, What);
   OMEGA_REQUIRE(A.Ext[1] == Rows, levelArrayText("MonotoneAdv", What, "[NTracers][" + std::to_string(Rows) + "]"));
}

void MonotoneAdv::addTracerTend(const Array3DReal &Tend, const Array2DReal &HOld, const Array2DReal &HNew,
                                const Array2DReal &U, const Array3DReal &Tracers, int NTracers, Real Dt, hipStream_t S) const {
   OMEGA_REQUIRE(NTracers >= 1 && NTracers <= MaxTracers,
                 "MonotoneAdv: NTracers = " + std::to_string(NTracers) + " is outside 1 .. MaxTracers = " +
                     std::to_string(MaxTracers));
   OMEGA_REQUIRE(std::isfinite(Dt) && Dt > 0.0, "MonotoneAdv: Dt = " + std::to_string(Dt) + " is not finite and positive");
   requirePlanes(Tend, NTracers, Mesh->NCellsSize, NVertLayers, "the tracer tendency");
   requirePlanes(Tracers, NTracers, Mesh->NCellsSize, NVertLayers, "Tracers");
   requireLevelArray("MonotoneAdv", HOld, Mesh->NCellsSize, NVertLayers, "the old LayerThickness");
   requireLevelArray("MonotoneAdv", HNew, Mesh->NCellsSize, NVertLayers, "the new LayerThickness");
   requireLevelArray("MonotoneAdv", U, Mesh->NEdgesSize, NVertLayers, "NormalVelocity");
   Pacer::Range Timer("MonotoneAdv:addTracerTend", 1);
   MonotoneAdvArgs A;
   A.K = NVertLayers, A.NTracers = NTracers, A.FluxThicknessUpwind = Config.FluxThicknessUpwind ? 1 : 0, A.Dt = Dt;
   A.HOld = HOld.Ptr, A.HNew = HNew.Ptr, A.NormalVelocity = U.Ptr, A.Tracers = Tracers.Ptr;
   A.ScaleIn = ScaleIn.Ptr, A.ScaleOut = ScaleOut.Ptr, A.Tend = Tend.Ptr;
   if (VAdv) { // the 3-D form
      A.VerticalTransport = VAdv->VerticalTransport.Ptr;
      A.MinLayerCell = VAdv->VCoord->MinLayerCell.Ptr, A.MaxLayerCell = VAdv->VCoord->MaxLayerCell.Ptr;
   }
   if (HighOrder.HorzOrder != 2) {
      A.Hess = Hess.Ptr, A.HessWeight = HessWeight.Ptr, A.FitCell = FitCell.Ptr;
      A.EdgeDirOwn = EdgeDirOwn.Ptr, A.EdgeDirAcross = EdgeDirAcross.Ptr;
      A.Beta = HighOrder.HorzOrder == 4 ? 0.0 : HighOrder.Coef3rdOrder;
   }
   LaunchCount += launchMonotoneAdv(Mesh->view(), A, S);
}

void MonotoneAdv::copyToHost() {
   HIP_CHECK(hipDeviceSynchronize());
   OMEGA::copyToHost(ScaleInH.data(), ScaleIn);
   OMEGA::copyToHost(ScaleOutH.data(), ScaleOut);
}

} // namespace OMEGA
