// signals.hip -- signals that need every day row of the panel (rules D1..D6 in DESIGN.md 7): the
// 52-week high and volatility-scaled momentum, with the realised volatility the cost model takes
// as SIG.
//
//   k_month_stats     D1.  One pass over P: the month walk of daytrip.h, one or two assets per lane,
//                     no lead-in (csm_tune "stats_chunks").  Per priced cell: one division that
//                     depends on loaded values only, and one add on the SSW chain.
//   k_window_signals  D2..D6.  A lane per asset walks the months: the stitch (the month's first
//                     return, added last), the Jh / Jv windows on slot-major per-lane LDS rings
//                     (the column layout of scan.h's ScanLane ring), each window summed again
//                     oldest first every month, and the next return of each requested signal by
//                     scan.h's rank_step / pending_finish on a (psff, prev) pair of its own.
#include "csm_common.h"
#include "daytrip.h"
#include "scan.h"

#define WS_THREADS 64
#define WS_MAXJ 36

// the month chunks of k_month_stats: 0 auto, one month per chunk | n >= 1 that many (clamped to
// T_m).  Finer chunks measured faster at every step on both widths tried: C4 (100,000 assets,
// 461 months) 1 / 11 / 88 / 461 chunks 3.30 / 1.99 / 1.87 / 1.83 ms; 5,000 assets x 300 months
// 1 / 13 / 103 / 300 chunks 2.00 / 0.181 / 0.071 / 0.069 ms (profiles/r10/bench_signals.log)
static int g_tune_stats_chunks = 0;
static const TuneKnob g_knobs[] = {
    {"stats_chunks", &g_tune_stats_chunks, [](int v) { return v >= 0; }},
};

// ------------------------------------------------------------------------------- D1
// One asset's running statistics of the month being walked.
struct MsAcc {
  double last;   // last priced row's price (NaN: none yet)
  double p1;     // first priced row's price
  double hi;     // maximum over the priced rows
  double ss;     // sum of squared returns between consecutive priced rows, in day order
  int nd;        // their number
  bool anyp;     // the month has a row (a cell that is not ABSENT)
};

__device__ __forceinline__ void ms_reset(MsAcc& s) {
  s.last = qnan();
  s.p1 = qnan();
  s.hi = qnan();
  s.ss = 0.0;
  s.nd = 0;
  s.anyp = false;
}

// One day row.  Selects only: a row without a price (NaN or ABSENT) changes nothing but anyp, and
// the division's operands are loaded values, so the divisions of a trip do not wait for each other.
__device__ __forceinline__ void ms_step(MsAcc& s, double x) {
  const bool ok = !isnan_d(x);
  const bool have = ok && !isnan_d(s.last);
  const double r = x / s.last - 1.0;
  s.anyp |= !is_absent(x);
  s.ss = have ? s.ss + r * r : s.ss;
  s.nd += have ? 1 : 0;
  s.hi = (ok && !(x <= s.hi)) ? x : s.hi;   // (NaN hi: the first priced row)
  s.p1 = have ? s.p1 : (ok ? x : s.p1);
  s.last = ok ? x : s.last;
}

// k_month_stats's walker (daytrip.h): one panel, no lead-in; rows past the chunk are ABSENT.
template <int VEC>
struct MsWalker {
  const double* __restrict__ P;
  int64_t N, a;
  double* __restrict__ PM;
  double* __restrict__ P1;
  double* __restrict__ HI;
  double* __restrict__ SSW;
  int32_t* __restrict__ NDW;
  MsAcc acc[VEC];
  struct Rows {
    double x[MS_TRIP][VEC];
  };

  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int k = 0; k < VEC; ++k) ms_reset(acc[k]);
  }
  __device__ __forceinline__ void begin(int64_t) { reset(); }
  __device__ __forceinline__ void load(Rows& r, int64_t d, int64_t dB) const {
    trip_load<MS_TRIP, VEC>(r.x, P, N, a, d, dB, absent_val());
  }
  __device__ __forceinline__ void own(Rows&, int64_t, int64_t) const {}
  __device__ __forceinline__ void step(const Rows& r, int i) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) ms_step(acc[k], r.x[i][k]);
  }
  __device__ __forceinline__ void flush(int m) {
    const int64_t o = (int64_t)m * N + a;
    double pm[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) pm[k] = acc[k].anyp ? acc[k].last : absent_val();
    if (VEC == 2) {
      if (PM) store_pair(PM + o, pm[0], pm[VEC - 1]);
      store_pair(P1 + o, acc[0].p1, acc[VEC - 1].p1);
      store_pair(HI + o, acc[0].hi, acc[VEC - 1].hi);
      store_pair(SSW + o, acc[0].ss, acc[VEC - 1].ss);
      *reinterpret_cast<int2*>(NDW + o) = make_int2(acc[0].nd, acc[VEC - 1].nd);
    } else {
      if (PM) PM[o] = pm[0];
      P1[o] = acc[0].p1;
      HI[o] = acc[0].hi;
      SSW[o] = acc[0].ss;
      NDW[o] = acc[0].nd;
    }
    reset();
  }
};

template <int VEC>
__global__ __launch_bounds__(MS_THREADS) void k_month_stats(
    const double* __restrict__ P, int64_t T_d, int64_t N, const int64_t* __restrict__ ms, int T_m,
    int G, double* __restrict__ PM, double* __restrict__ P1, double* __restrict__ HI,
    double* __restrict__ SSW, int32_t* __restrict__ NDW) {
  const int64_t a = ((int64_t)blockIdx.x * MS_THREADS + threadIdx.x) * VEC;
  if (a >= N) return;   // (no barrier anywhere below)
  MsWalker<VEC> w{P, N, a, PM, P1, HI, SSW, NDW};
  month_walk<MS_TRIP>(w, ms, T_m, G, T_d);
}

// ---------------------------------------------------------------------------- D2..D6
struct WsRow {
  double pm, p1, hi, ssw, mom;
  int ndw;
};

__device__ __forceinline__ void ws_load(WsRow& r, int64_t o, const double* __restrict__ PM,
                                        const double* __restrict__ P1,
                                        const double* __restrict__ HI,
                                        const double* __restrict__ SSW,
                                        const int32_t* __restrict__ NDW,
                                        const double* __restrict__ M) {
  r.pm = PM[o];
  r.p1 = P1[o];
  r.hi = HI[o];
  r.ssw = SSW[o];
  r.ndw = NDW[o];
  r.mom = M ? M[o] : qnan();
}

// D6 on one (psff, prev) pair: month t's price x (ABSENT: no step) and the signal's value s.
__device__ __forceinline__ void ws_next_ret(double x, double s, int t, int64_t N, int64_t a,
                                            double& psff, int& prev, double* __restrict__ NR) {
  const int64_t o = (int64_t)t * N + a;
  if (is_absent(x)) {
    NR[o] = qnan();
    return;
  }
  if (rank_step(x, s, t, psff, prev, [&](int row, double nr) { NR[(int64_t)row * N + a] = nr; }))
    NR[o] = qnan();
}

// f(v) for the J entries of a lane's ring column from slot idx on (wrapping at J), oldest first:
// four reads in flight, then their f in order (one LDS latency per four entries, not per entry).
template <class T, class F>
__device__ __forceinline__ void ws_ring_walk(const T* ring, int J, int idx, F f) {
  int k = 0;
  for (; k + 4 <= J; k += 4) {
    T v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      v[u] = ring[idx * WS_THREADS];
      idx = (idx + 1 == J) ? 0 : idx + 1;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) f(v[u]);
  }
  for (; k < J; ++k) {
    f(ring[idx * WS_THREADS]);
    idx = (idx + 1 == J) ? 0 : idx + 1;
  }
}

// LDS (dynamic): HI ring [Jh][WS_THREADS] doubles, SS ring [Jv][WS_THREADS] doubles, ND ring
// [Jv][WS_THREADS] ints; a lane's column, so a wave's accesses hit every bank once.
static inline size_t ws_lds_bytes(int Jh, int Jv) {
  return (size_t)(Jh + Jv) * WS_THREADS * sizeof(double) + (size_t)Jv * WS_THREADS * sizeof(int);
}

__global__ __launch_bounds__(WS_THREADS) void k_window_signals(
    const double* __restrict__ PM, const double* __restrict__ P1, const double* __restrict__ HI,
    const double* __restrict__ SSW, const int32_t* __restrict__ NDW, const double* __restrict__ M,
    int T_m, int64_t N, int Jh, int Jv, int min_obs, double* __restrict__ SS,
    int32_t* __restrict__ ND, double* __restrict__ H52, double* __restrict__ RV,
    double* __restrict__ MS, double* __restrict__ NRH, double* __restrict__ NRM) {
  extern __shared__ __attribute__((aligned(16))) double ws_lds[];
  const int tid = threadIdx.x;
  const int64_t a = (int64_t)blockIdx.x * WS_THREADS + tid;
  if (a >= N) return;   // (no barrier: a lane reads only its own column)
  constexpr int RS = WS_THREADS;
  double* rh = ws_lds + tid;
  double* rs = ws_lds + Jh * RS + tid;
  int* rn = reinterpret_cast<int*>(ws_lds + (Jh + Jv) * RS) + tid;
  const double NaN = qnan();
  double q = NaN;    // last priced month price of the months before t
  int first = -1;    // first month with a priced row
  int hh = 0, hv = 0;   // the rings' next slots = their oldest entries once they are full
  double psff_h = NaN, psff_m = NaN;
  int prev_h = -1, prev_m = -1;
  const bool need_h = H52 || NRH, need_v = RV || MS || NRM;   // (uniform) windows somebody reads
  WsRow cur, nxt;
  ws_load(cur, a, PM, P1, HI, SSW, NDW, M);
  nxt = cur;
  for (int t = 0; t < T_m; ++t) {
    if (t + 1 < T_m) ws_load(nxt, (int64_t)(t + 1) * N + a, PM, P1, HI, SSW, NDW, M);
    const int64_t o = (int64_t)t * N + a;
    const bool priced = !isnan_d(cur.pm);
    if (first < 0 && priced) first = t;
    // D2: the return from the last priced month-end before t to the month's first price, last
    const bool stitch = !isnan_d(cur.p1) && !isnan_d(q);
    const double r0 = cur.p1 / q - 1.0;
    const double ss = stitch ? cur.ssw + r0 * r0 : cur.ssw;
    const int nd = cur.ndw + (stitch ? 1 : 0);
    if (SS) SS[o] = ss;
    if (ND) ND[o] = nd;
    rh[hh * RS] = cur.hi;
    hh = (hh + 1 == Jh) ? 0 : hh + 1;
    rs[hv * RS] = ss;
    rn[hv * RS] = nd;
    hv = (hv + 1 == Jv) ? 0 : hv + 1;
    // D3
    double h52 = NaN;
    if (need_h && priced && t - Jh + 1 >= 0 && first <= t - Jh + 1) {
      double hmax = NaN;
      ws_ring_walk(rh, Jh, hh, [&](double h) {
        hmax = (!isnan_d(h) && !(h <= hmax)) ? h : hmax;
      });
      h52 = cur.pm / hmax;
    }
    // D4: the window summed again, oldest month first
    double rv = NaN;
    if (need_v && first >= 0 && t - Jv + 1 >= 0 && first <= t - Jv + 1) {
      double s = 0.0;
      int n = 0;
      ws_ring_walk(rs, Jv, hv, [&](double x) { s += x; });
      ws_ring_walk(rn, Jv, hv, [&](int x) { n += x; });
      if (n >= min_obs) rv = sqrt(s / (double)n);
    }
    // D5
    const double msig = (!isnan_d(cur.mom) && rv > 0.0) ? cur.mom / rv : NaN;
    if (H52) H52[o] = h52;
    if (RV) RV[o] = rv;
    if (MS) MS[o] = msig;
    // D6
    if (NRH) ws_next_ret(cur.pm, h52, t, N, a, psff_h, prev_h, NRH);
    if (NRM) ws_next_ret(cur.pm, msig, t, N, a, psff_m, prev_m, NRM);
    q = priced ? cur.pm : q;
    cur = nxt;
  }
  // whole panels only: no later month settles the pending rows
  if (NRH && prev_h >= 0) NRH[(int64_t)prev_h * N + a] = pending_finish(absent_val(), psff_h);
  if (NRM && prev_m >= 0) NRM[(int64_t)prev_m * N + a] = pending_finish(absent_val(), psff_m);
}

extern "C" {

int csm_tune_signals(const char* key, int value) { return tune_set(g_knobs, key, value); }

int csm_month_stats(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N,
                    const int64_t* month_start, int32_t T_m, int32_t max_month_days, double* PM,
                    double* P1, double* HI, double* SSW, int32_t* NDW) {
  int r = prep(ctx);
  if (r) return r;
  if (!P || !month_start || !P1 || !HI || !SSW || !NDW || T_d < 1 || N < 1 || T_m < 1 ||
      T_d > ((int64_t)1 << 40) / N)
    return set_err(ctx, CSM_E_INVAL, "csm_month_stats: bad arguments (T_d=%lld N=%lld T_m=%d)",
                   (long long)T_d, (long long)N, T_m);
  if (max_month_days < 1 || max_month_days > 32)
    return set_err(ctx, CSM_E_INVAL, "csm_month_stats: max_month_days=%d is outside [1, 32]",
                   max_month_days);
  const bool v2 = (N % 2 == 0) && aligned16(P) && (!PM || aligned16(PM)) && aligned16(P1) &&
                  aligned16(HI) && aligned16(SSW) && aligned8(NDW);
  const int vec = v2 ? 2 : 1;
  // month chunks: T_m x slices workgroups fill the chip whatever the panel's width
  const dim3 grid = month_grid(ctx, N, MS_THREADS * vec,
                               g_tune_stats_chunks > 0 ? g_tune_stats_chunks : T_m, 0, T_m);
  const int g = (int)grid.y;
  if (v2)
    hipLaunchKernelGGL(k_month_stats<2>, grid, dim3(MS_THREADS), 0, ctx->stream, P, T_d, N,
                       month_start, T_m, g, PM, P1, HI, SSW, NDW);
  else
    hipLaunchKernelGGL(k_month_stats<1>, grid, dim3(MS_THREADS), 0, ctx->stream, P, T_d, N,
                       month_start, T_m, g, PM, P1, HI, SSW, NDW);
  LAUNCH_CHECK(ctx, "k_month_stats");
  return CSM_OK;
}

int csm_window_signals(csm_ctx* ctx, const double* PM, const double* P1, const double* HI,
                       const double* SSW, const int32_t* NDW, const double* M, int32_t T_m,
                       int64_t N, int32_t Jh, int32_t Jv, int32_t min_obs, double* SS, int32_t* ND,
                       double* H52, double* RV, double* MS, double* NR_H52, double* NR_MS) {
  int r = prep(ctx);
  if (r) return r;
  if (!PM || !P1 || !HI || !SSW || !NDW || T_m < 1 || N < 1)
    return set_err(ctx, CSM_E_INVAL, "csm_window_signals: bad arguments (T_m=%d N=%lld)", T_m,
                   (long long)N);
  if (Jh < 1 || Jh > WS_MAXJ || Jv < 1 || Jv > WS_MAXJ)
    return set_err(ctx, CSM_E_INVAL, "csm_window_signals: Jh=%d / Jv=%d is outside [1, %d]", Jh,
                   Jv, WS_MAXJ);
  if (min_obs < 1)
    return set_err(ctx, CSM_E_INVAL, "csm_window_signals: min_obs=%d must be at least 1", min_obs);
  if (!M && (MS || NR_MS))
    return set_err(ctx, CSM_E_INVAL, "csm_window_signals: MS and NR_MS need M");
  const unsigned blocks = (unsigned)((N + WS_THREADS - 1) / WS_THREADS);
  hipLaunchKernelGGL(k_window_signals, dim3(blocks), dim3(WS_THREADS), ws_lds_bytes(Jh, Jv),
                     ctx->stream, PM, P1, HI, SSW, NDW, M, T_m, N, Jh, Jv, min_obs, SS, ND, H52,
                     RV, MS, NR_H52, NR_MS);
  LAUNCH_CHECK(ctx, "k_window_signals");
  return CSM_OK;
}

}  // extern "C"
