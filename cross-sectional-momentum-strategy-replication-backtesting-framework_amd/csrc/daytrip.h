// daytrip.h -- the month walk of the kernels that sum the daily panels by (month, asset):
// k_month_stats (signals.hip, rule D1), k_daily_sums and k_daily_fsums (dailymkt.hip, rules V3 and
// MF6), k_liq_sums (liquidity.hip, rule Q2), k_range_sums (range.hip, rules HL1..HL5) and
// k_asym_sums (asym.hip, rule AS2).
//
// The grid is (slice of MS_THREADS lanes) x (chunk of consecutive months, scan.h chunk_range); a
// lane owns one asset, or two adjacent ones (16-B loads and stores), and walks the day rows of its
// chunk in trips of TRIP rows, the next trip's loads in flight while this one is reduced.  A
// month's values are stored as the walk passes its end; no month needs anything from another but
// what the lead-in of its chunk reads again, so there is no barrier, no LDS, no atomic and no state
// in memory, and the chunk count only decides how many workgroups the launch has: every count
// gives the same bits.
//
// month_walk is that walk and nothing of a signal.  A kernel gives it a walker:
//   Rows                 one trip's rows of the kernel's panels, in registers
//   begin(dA)            the lead-in of a chunk that starts at row dA; resets the accumulators
//   load(r, d, dB)       rows [d, d + TRIP) into r, a trip ahead; rows from dB on are placeholders
//                        that change nothing (trip_load's fill)
//   own(r, d, dB)        what trip d loads for itself into r, if anything (k_daily_fsums)
//   step(r, i)           row i of the trip
//   flush(m)             month m is complete: stores it and resets the accumulators; the lane's
//                        running state (a last priced row) runs on
#pragma once
#include "csm_common.h"
#include "scan.h"

#define MS_THREADS 256
#define MS_TRIP 8        // day rows per trip: two trips of two assets are 64 VGPRs of buffers

__device__ __forceinline__ int64_t ms_clip(int64_t d, int64_t lo, int64_t hi) {
  return d < lo ? lo : (d > hi ? hi : d);
}

// Rows [d, d + TRIP) of the lane's VEC assets from column a of panel X; rows from dB on are `fill`.
template <int TRIP, int VEC>
__device__ __forceinline__ void trip_load(double (&x)[TRIP][VEC], const double* __restrict__ X,
                                          int64_t N, int64_t a, int64_t d, int64_t dB,
                                          double fill) {
  const double* p = X + d * N + a;
  auto row = [&](int i) {
    if (VEC == 2) {
      const double2 t = *reinterpret_cast<const double2*>(p + (int64_t)i * N);
      x[i][0] = t.x;
      x[i][VEC - 1] = t.y;
    } else {
      x[i][0] = p[(int64_t)i * N];
    }
  };
  if (d + TRIP <= dB) {   // (uniform) a whole trip: no predicate on any load
#pragma unroll
    for (int i = 0; i < TRIP; ++i) row(i);
  } else {
#pragma unroll
    for (int i = 0; i < TRIP; ++i) {
      if (d + i < dB) {
        row(i);
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) x[i][k] = fill;
      }
    }
  }
}

// Chunk blockIdx.y of G (G <= T_m: at least one month) of the calendar ms[0 .. T_m] over a panel
// of T_d day rows.  The chunk's day rows [dA, dB) are clipped to the panel and every month end to
// them in turn, so no calendar makes the walk read outside [dA, dB) or flush a month outside the
// chunk; months may be shorter than a trip or empty, several in a row.  The walker comes by value:
// by reference k_range_sums without CS and AR took 98 VGPRs for 95, four waves a SIMD for five.
template <int TRIP, class Walker>
__device__ __forceinline__ void month_walk(Walker w, const int64_t* __restrict__ ms, int T_m,
                                           int G, int64_t T_d) {
  int m0, m1;
  chunk_range(T_m, G, (int)blockIdx.y, m0, m1);
  const int64_t dA = ms_clip(ms[m0], 0, T_d), dB = ms_clip(ms[m1], dA, T_d);
  int m = m0;
  int64_t nb = ms_clip(ms[m0 + 1], dA, dB);   // end of month m
  w.begin(dA);
  auto next_month = [&]() {   // (uniform) month m is complete
    w.flush(m);
    ++m;
    nb = m < m1 ? ms_clip(ms[m + 1], dA, dB) : dB;
  };
  typename Walker::Rows cur, nxt;
  w.load(cur, dA, dB);
  for (int64_t d = dA; d < dB; d += TRIP) {
    w.load(nxt, d + TRIP, dB);
    w.own(cur, d, dB);
    if (d + TRIP <= nb) {   // (uniform) the trip lies inside month m: one straight block
#pragma unroll
      for (int i = 0; i < TRIP; ++i) w.step(cur, i);
    } else {
#pragma unroll
      for (int i = 0; i < TRIP; ++i) {
        while (m < m1 && d + i >= nb) next_month();   // (zero-length months: several)
        w.step(cur, i);
      }
    }
    cur = nxt;
  }
  while (m < m1) next_month();   // the last month, and whatever zero-length months follow it
}

static inline bool aligned8(const void* p) { return ((uintptr_t)p & 7u) == 0; }
