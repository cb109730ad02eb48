// daytrip.h -- the day-row trips of the kernels that walk a chunk of consecutive months of the
// daily panel with a lane per asset (or two adjacent ones): k_month_stats (signals.hip, rule D1)
// and k_daily_sums (dailymkt.hip, rule V3); k_liq_sums (liquidity.hip, rule Q2) takes the block size
// and the clip and loads trips of its own length.
#pragma once
#include "csm_common.h"

#define MS_THREADS 256
#define MS_TRIP 8        // day rows per trip: two trips of two assets are 64 VGPRs of buffers

__device__ __forceinline__ int64_t ms_clip(int64_t d, int64_t lo, int64_t hi) {
  return d < lo ? lo : (d > hi ? hi : d);
}

// Rows [d, d + MS_TRIP) of the lane's assets; rows from dB on are ABSENT placeholders, which
// change nothing.
template <int VEC>
__device__ __forceinline__ void ms_load(double (&x)[MS_TRIP][VEC], const double* __restrict__ P,
                                        int64_t N, int64_t a, int64_t d, int64_t dB) {
  const double* p = P + d * N + a;
  auto row = [&](int i) {
    if (VEC == 2) {
      const double2 t = *reinterpret_cast<const double2*>(p + (int64_t)i * N);
      x[i][0] = t.x;
      x[i][VEC - 1] = t.y;
    } else {
      x[i][0] = p[(int64_t)i * N];
    }
  };
  if (d + MS_TRIP <= dB) {   // (uniform) a whole trip: no predicate on any load
#pragma unroll
    for (int i = 0; i < MS_TRIP; ++i) row(i);
  } else {
#pragma unroll
    for (int i = 0; i < MS_TRIP; ++i) {
      if (d + i < dB) {
        row(i);
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) x[i][k] = absent_val();
      }
    }
  }
}

static inline bool aligned8(const void* p) { return ((uintptr_t)p & 7u) == 0; }
