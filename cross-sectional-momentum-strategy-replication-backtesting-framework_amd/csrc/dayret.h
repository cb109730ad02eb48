// dayret.h -- rule V1's daily return with a gap bound, as the kernels that walk day rows with an
// asset's last priced price in registers take it: k_daily_market, k_daily_sums and k_daily_fsums
// (dailymkt.hip, rules V2, V3, MF6), k_liq_sums (liquidity.hip, rule Q2) and k_asym_sums (asym.hip,
// rule AS2).
#pragma once
#include "csm_common.h"

#define DM_MAXGAP 32

// One asset's last priced price (NaN: none within reach) and the rows since it, saturated at
// DM_MAXGAP (one more is past every max_gap).
struct DrLane {
  double lp;
  int age;
};

// Row d's return: x / lp - 1.0 when x is priced and the last priced row is at most max_gap rows
// back, else NaN.  A NaN x or lp makes the quotient NaN by itself; the division's operands are a
// loaded value and a select of loaded values.
__device__ __forceinline__ double dr_step(DrLane& s, double x, int max_gap) {
  const bool ok = !isnan_d(x);
  const int g = s.age + 1;
  const double r = g <= max_gap ? x / s.lp - 1.0 : qnan();
  s.lp = ok ? x : s.lp;
  s.age = ok ? 0 : (g > DM_MAXGAP ? DM_MAXGAP : g);
  return r;
}

// The lead-in of a chunk that starts at row d0: each asset's latest priced row among the max_gap
// rows before d0 (clipped at row 0).  An older one books no return in the chunk.  col(k) is the
// k-th asset's column, or -1.  Only the lanes still searching load; the walk ends when no lane of
// the wave is.
template <int CNT, class Col>
__device__ __forceinline__ void dr_lead_in(DrLane (&s)[CNT], const double* __restrict__ P,
                                           int64_t N, int64_t d0, int max_gap, Col col) {
#pragma unroll
  for (int k = 0; k < CNT; ++k) {
    s[k].lp = qnan();
    s[k].age = DM_MAXGAP;
  }
  for (int g = 1; g <= max_gap && d0 - g >= 0; ++g) {
    bool searching = false;
#pragma unroll
    for (int k = 0; k < CNT; ++k) {
      const int64_t a = col(k);
      if (a >= 0 && isnan_d(s[k].lp)) {
        const double x = P[(d0 - g) * N + a];
        if (!isnan_d(x)) {
          s[k].lp = x;
          s[k].age = g - 1;
        } else {
          searching = true;
        }
      }
    }
    if (!__any(searching)) break;
  }
}
