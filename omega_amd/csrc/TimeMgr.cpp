// TimeMgr.cpp -- see TimeMgr.h.
#include "TimeMgr.h"

#include <cfloat>
#include <cmath>
#include <cstdlib>

namespace OMEGA {

// ---- TimeFrac arithmetic of the reference's TimeMgr (TimeMgr.h) ----
namespace {
I8 fracGCD(I8 A, I8 B) {
   A = std::llabs(A);
   B = std::llabs(B);
   if (A == 0)
      return B ? B : 1;
   if (B == 0)
      return A;
   while (B) {
      I8 T = A % B;
      A    = B;
      B    = T;
   }
   return A;
}
} // namespace
// TimeFrac::simplify (TimeMgr.cpp:956-1000)
void TimeFrac::simplify() {
   OMEGA_REQUIRE(Denom != 0, "TimeFrac: zero denominator");
   I8 W;
   if (std::llabs((W = Numer / Denom)) >= 1) {
      Whole += W;
      Numer %= Denom;
   }
   if (Whole > 0 && ((Numer < 0 && Denom > 0) || (Denom < 0 && Numer > 0))) {
      Whole--;
      Numer += Denom;
   } else if ((Whole < 0 && (Numer > 0 && Denom > 0)) || (Denom < 0 && Numer < 0)) {
      Whole++;
      Numer -= Denom;
   }
   if (Denom < 0) {
      Denom *= -1;
      Numer *= -1;
   }
   const I8 G = fracGCD(Numer, Denom);
   Numer /= G;
   Denom /= G;
}
// TimeFrac::setSeconds (TimeMgr.cpp:193-283): continued-fraction conversion
TimeFrac TimeFrac::fromSeconds(R8 Seconds) {
   TimeFrac F;
   const R8 Rabs = std::fabs(Seconds);
   OMEGA_REQUIRE(!((Rabs > 0.0 && Rabs < 1e-17) || Rabs > 1e18), "TimeStepper: time value out of range");
   const int Sign = (Seconds < 0) ? -1 : 1;
   R8 Target      = Rabs;
   if (Target == 0.0)
      return F;
   if (Target >= 1.0) {
      const I8 W = (I8)Rabs;
      Target -= (R8)W;
      F.Whole = Sign * W;
      if (Target < 1e-17)
         return F;
   }
   const R8 P = std::pow(10.0, -(DBL_DIG - (int)std::log10(Rabs)));
   R8 R       = Target;
   I8 Npp = 0, Np = 1, Dpp = 1, Dp = 0, A, N, D;
   for (;;) {
      A = (I8)R;
      N = A * Np + Npp;
      D = A * Dp + Dpp;
      if (std::fabs((R8)N / (R8)D - Target) < P)
         break;
      const R8 Fr = R - (R8)A;
      if (Fr < 1e-17)
         break;
      R   = 1.0 / Fr;
      Npp = Np;
      Np  = N;
      Dpp = Dp;
      Dp  = D;
   }
   F.Numer = N * Sign;
   F.Denom = D;
   F.simplify();
   return F;
}
// TimeFrac::operator+ / operator- (TimeMgr.cpp:625-679): over the least common denominator
TimeFrac TimeFrac::operator+(const TimeFrac &O) const {
   TimeFrac S;
   S.Denom = Denom / fracGCD(Denom, O.Denom) * O.Denom;
   S.Numer = Numer * (S.Denom / Denom) + O.Numer * (S.Denom / O.Denom);
   S.Whole = Whole + O.Whole;
   S.simplify();
   return S;
}
TimeFrac TimeFrac::operator-(const TimeFrac &O) const {
   TimeFrac S;
   S.Denom = Denom / fracGCD(Denom, O.Denom) * O.Denom;
   S.Numer = Numer * (S.Denom / Denom) - O.Numer * (S.Denom / O.Denom);
   S.Whole = Whole - O.Whole;
   S.simplify();
   return S;
}
// TimeFrac::operator*(R8) (TimeMgr.cpp:747-767)
TimeFrac TimeFrac::operator*(R8 Multiplier) const {
   const TimeFrac M = fromSeconds(Multiplier);
   TimeFrac P;
   P.Denom = Denom * M.Denom;
   P.Numer = (Whole * Denom + Numer) * (M.Whole * M.Denom + M.Numer);
   P.simplify();
   return P;
}
TimeFrac TimeFrac::operator*(I4 Multiplier) const {
   TimeFrac P;
   P.Whole = Whole * Multiplier;
   P.Numer = Numer * Multiplier;
   P.Denom = Denom;
   P.simplify();
   return P;
}
void TimeInterval::set(R8 Length, TimeUnits Units) {
   OMEGA_REQUIRE(Units == TimeUnits::Seconds || Units == TimeUnits::Minutes || Units == TimeUnits::Hours,
                 "TimeInterval: only non-calendar units (seconds, minutes, hours) are supported");
   Interval = TimeFrac::fromSeconds(Length);
   if (Units == TimeUnits::Minutes)
      Interval = Interval * (I4)60;
   else if (Units == TimeUnits::Hours)
      Interval = Interval * (I4)3600;
}
void TimeInterval::get(R8 &Length, TimeUnits Units) const {
   OMEGA_REQUIRE(Units == TimeUnits::Seconds || Units == TimeUnits::Minutes || Units == TimeUnits::Hours,
                 "TimeInterval: only non-calendar units (seconds, minutes, hours) are supported");
   Length = Interval.getSeconds();
   if (Units == TimeUnits::Minutes)
      Length /= 60.0;
   else if (Units == TimeUnits::Hours)
      Length /= 3600.0;
}

} // namespace OMEGA
