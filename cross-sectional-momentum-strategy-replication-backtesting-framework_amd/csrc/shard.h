// shard.h -- what the date-shard and time-chunk kernels of shards.hip, scans.hip, signal.hip and
// signal_tc.hip share: the exchange record and its fold, and the month prices of a shard.
//
// The exchange record of one asset over one shard (or chunk) of months, T = J + skip + 1; rows
// are N (or the column list's length) apart, [SUM_SCALARS + T] rows per shard:
//   0  n      present months of the shard
//   1  fv     index among them of the first with a valid price (-1: none)
//   2  lvi    index among them of the last with a valid price (-1: none)
//   3  lv     that last valid price (NaN: none)
//   4  head   the last valid price among the present rows before the tail, rows [0, n - T) (NaN)
//   5  first  the first present row's price (ABSENT: no present month)
//   6 ..      tail: the last T present month prices, oldest first, ABSENT-padded at the front
// An asset with no present month has the neutral record (0, -1, -1, NaN, NaN, ABSENT, ABSENT ...),
// which fold_body passes over.
#pragma once
#include "scan.h"

#define SUM_SCALARS 6
// Month loads in batches of SUM_U (independent loads issued together; the walks were one
// dependent round trip per month: C2 summary 15.5 us, fold 28.3 us).
#define SUM_U 8

#define MJ_MAX 4   // look-backs of one multi-J scan (scans.hip MJSet)
// psq (csm_momentum_multi_chunked): also the subset-ffilled price of every look-back jq.J[q]
// of the multi-J scan (the ranked subset starts J + skip present rows after the first valid
// price), [G][MJ_MAX][N]; the ring and pff are J's own for J = max(J) and shared by the others.
struct FoldJs {
  int n;
  int J[MJ_MAX];
};
// The fold of k_fold_carry for asset (column) a: the scan state at shard g's first month from
// the exchange records of shards < g (ring factors oldest first, then pff, psff: rows 0..W + 1
// through store(row, value)), and the first present price after shard g (returned).
template <class Store>
__device__ __forceinline__ double fold_body(const double* __restrict__ sm, int G, int g,
                                            int64_t N, int64_t a, int J, int skip,
                                            const double* __restrict__ tail_pm, Store store,
                                            const FoldJs& jq, double* __restrict__ psq) {
  const int W = J + skip, T = W + 1, S = SUM_SCALARS + T;
  const double NaN = qnan();
  // the neighbours' scalars in one round trip (the walks below start there and usually end
  // there): chunk g - 1's record scalars, chunk g + 1's count and first price
  double pg[SUM_SCALARS], ng0 = 0.0, ng5 = absent_val();
#pragma unroll
  for (int r = 0; r < SUM_SCALARS; ++r) pg[r] = g > 0 ? sm[((int64_t)(g - 1) * S + r) * N + a] : NaN;
  if (g + 1 < G) {
    ng0 = sm[((int64_t)(g + 1) * S) * N + a];
    ng5 = sm[((int64_t)(g + 1) * S + 5) * N + a];
  }
  auto at = [&](int h, int r) -> double { return sm[((int64_t)h * S + r) * N + a]; };
  // a record scalar (r a constant < SUM_SCALARS): chunk g - 1's from registers
  auto sc = [&](int h, int r) -> double { return h == g - 1 ? pg[r] : at(h, r); };
  // next_pm: first present row after shard g
  double npm = (tail_pm && g == G - 1) ? tail_pm[a] : absent_val();
  if (g + 1 < G) {
    if (ng0 > 0.0) npm = ng5;
    else for (int h = g + 2; h < G; ++h) if (sc(h, 0) > 0.0) { npm = sc(h, 5); break; }
  }
  if (tail_pm && g < G - 1 && is_absent(npm)) npm = tail_pm[a];
  // locate the oldest of the last T present rows of shards < g
  int nv = 0, src_h = -1, src_j = -1;
  for (int h = g - 1; h >= 0 && nv < T; --h) {
    const int k = (int)fmin(sc(h, 0), (double)T);
    const int take = k < T - nv ? k : T - nv;
    if (take > 0) { nv += take; src_h = h; src_j = T - take; }
  }
  double pff_before = NaN;
  if (nv > 0) {
    const int k0 = (int)fmin(sc(src_h, 0), (double)T);
    for (int j = src_j - 1; j > T - 1 - k0; --j) { const double x = at(src_h, SUM_SCALARS + j); if (!isnan_d(x)) { pff_before = x; break; } }
    if (isnan_d(pff_before)) pff_before = sc(src_h, 4);
    if (isnan_d(pff_before))
      for (int h = src_h - 1; h >= 0; --h) if (!isnan_d(sc(h, 3))) { pff_before = sc(h, 3); break; }
  }
  // replay oldest -> newest; the newest W rets become the ring (as factors fl(1+ret))
  double pff = pff_before;
  for (int k = 0; k < W; ++k) store(k, NaN);
  int c = 0;
  for (int h = src_h; h >= 0 && h < g; ++h) {
    const int kh = (int)fmin(sc(h, 0), (double)T);
    for (int jb = (h == src_h) ? src_j : T - kh; jb < T; jb += SUM_U) {   // SUM_U rows in flight
      double xs[SUM_U];
#pragma unroll
      for (int u = 0; u < SUM_U; ++u) xs[u] = jb + u < T ? at(h, SUM_SCALARS + jb + u) : NaN;
#pragma unroll
      for (int u = 0; u < SUM_U; ++u) {
        if (jb + u >= T) break;
        const double ret = price_step(xs[u], pff);
        const int pos = c - (nv - W);
        if (pos >= 0) store(pos, 1.0 + ret);
        ++c;
      }
    }
  }
  double lastv = NaN;
  for (int h = g - 1; h >= 0; --h) if (!isnan_d(sc(h, 3))) { lastv = sc(h, 3); break; }
  store(W, lastv);
  int64_t off = 0, f = -1;
  for (int hb = 0; hb < g; hb += SUM_U) {   // every earlier chunk's counts, SUM_U in flight
    double cn[SUM_U], fi[SUM_U];
#pragma unroll
    for (int u = 0; u < SUM_U; ++u) {
      cn[u] = hb + u < g ? at(hb + u, 0) : 0.0;
      fi[u] = hb + u < g ? at(hb + u, 1) : -1.0;
    }
#pragma unroll
    for (int u = 0; u < SUM_U; ++u) {
      if (hb + u >= g) break;
      if (f < 0 && fi[u] >= 0.0) f = off + (int64_t)fi[u];
      off += (int64_t)cn[u];
    }
  }
  // last valid price among the ranked rows of look-back Jq (rows >= f + Jq + skip)
  auto psff_of = [&](int Jq) {
    double ps = NaN;
    if (f >= 0) {
      int64_t offh = off;
      for (int h = g - 1; h >= 0; --h) {
        offh -= (int64_t)sc(h, 0);
        if (sc(h, 2) >= 0.0) {
          const int64_t li = offh + (int64_t)sc(h, 2);
          if (li >= f + Jq + skip) ps = sc(h, 3);
          break;
        }
      }
    }
    return ps;
  };
  store(W + 1, psff_of(J));
  if (psq)
    for (int q = 0; q < jq.n; ++q) psq[((int64_t)g * MJ_MAX + q) * N + a] = psff_of(jq.J[q]);
  return npm;
}

#define HALO_WALK 24   // a business month's day rows in one batch of loads
#define HALO_MAXG 64

// Month-end of asset a over day rows [d0, d1) (k_signal's reduction: last valid price, NaN if
// the month has rows but no price, ABSENT if none), walked back from the last row: one load for
// the usual month whose last row holds a price, else rows HALO_WALK at a time in flight.
__device__ __forceinline__ double halo_month_price(const double* __restrict__ P, int64_t d0,
                                                   int64_t d1, int64_t N, int64_t a) {
  if (d1 <= d0) return absent_val();
  const double xl = P[(d1 - 1) * N + a];
  if (xl == xl) return xl;
  bool p = !is_absent(xl);
  for (int64_t d = d1 - 2; d >= d0; d -= HALO_WALK) {
    double xs[HALO_WALK];
#pragma unroll
    for (int u = 0; u < HALO_WALK; ++u) xs[u] = d - u >= d0 ? P[(d - u) * N + a] : absent_val();
#pragma unroll
    for (int u = 0; u < HALO_WALK; ++u) {
      if (xs[u] == xs[u]) return xs[u];
      p |= !is_absent(xs[u]);
    }
  }
  return p ? qnan() : absent_val();
}

// Speculative shards keep PM only for the first and last W + SHARD_PM_EDGE months (what the
// summary walks and the repair read for a dense asset); other months are re-derived from the
// daily panel for the rare asset that needs them (shard_pm_at).
#define SHARD_PM_EDGE 8
__device__ __forceinline__ bool shard_pm_kept(int m, int T_m, int W) {
  return m < W + SHARD_PM_EDGE || m >= T_m - (W + SHARD_PM_EDGE);
}

#ifndef WALK_CHUNK
#define WALK_CHUNK 8   // months per load round of the summary / repair walks
#endif

// Month price of asset a in month m of a speculative shard: PM where k_signal<SH> kept it,
// else the month-end of the daily rows (k_signal's reduction: last valid price, NaN if the
// month has rows but no price, ABSENT if none).
__device__ __forceinline__ double shard_pm_at(const double* __restrict__ PM,
                                              const double* __restrict__ P,
                                              const int64_t* __restrict__ ms, int m, int T_m,
                                              int W, int64_t N, int64_t a) {
  if (shard_pm_kept(m, T_m, W)) return PM[(int64_t)m * N + a];
  // the month's day rows are loaded together (one latency per month, not one per day)
  constexpr int KD = 24;
  const int64_t d0 = ms[m], d1 = ms[m + 1];
  double last = 0.0;
  bool p = false, v = false;
  double xs[KD];
#pragma unroll
  for (int k = 0; k < KD; ++k) xs[k] = (d0 + k < d1) ? P[(d0 + k) * N + a] : absent_val();
#pragma unroll
  for (int k = 0; k < KD; ++k) {
    const double x = xs[k];
    const bool ok = x == x;
    p |= !is_absent(x);
    v |= ok;
    last = ok ? x : last;
  }
  for (int64_t d = d0 + KD; d < d1; ++d) {
    const double x = P[d * N + a];
    const bool ok = x == x;
    p |= !is_absent(x);
    v |= ok;
    last = ok ? x : last;
  }
  return p ? (v ? last : qnan()) : absent_val();
}

// WALK_CHUNK month prices of asset a, months m0, m0 + dm, m0 + 2 dm, ... within [lo, hi]
// (ABSENT outside): the kept months' PM loads are issued together first, the rare months PM
// does not keep are re-derived after them -- one memory round trip per chunk, not per month.
__device__ __forceinline__ void shard_pm_chunk(const double* __restrict__ PM,
                                               const double* __restrict__ P,
                                               const int64_t* __restrict__ ms, int m0, int dm,
                                               int lo, int hi, int T_m, int W, int64_t N,
                                               int64_t a, double (&buf)[WALK_CHUNK]) {
#pragma unroll
  for (int q = 0; q < WALK_CHUNK; ++q) {
    const int m = m0 + q * dm;
    const bool in = m >= lo && m <= hi;
    buf[q] = (in && shard_pm_kept(m, T_m, W)) ? PM[(int64_t)m * N + a] : absent_val();
  }
#pragma unroll
  for (int q = 0; q < WALK_CHUNK; ++q) {
    const int m = m0 + q * dm;
    if (m >= lo && m <= hi && !shard_pm_kept(m, T_m, W)) buf[q] = shard_pm_at(PM, P, ms, m, T_m, W, N, a);
  }
}
