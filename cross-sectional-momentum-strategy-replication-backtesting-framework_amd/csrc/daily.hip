// daily.hip -- daily return series of the decile and long-short portfolios (rule E7 in
// DESIGN.md 7, an extension of E1 / E2 to the days of the holding month), and per-series daily
// statistics.
//
//   k_daily        one workgroup per slice of DY_COLS adjacent assets, a lane per asset.  The
//                  workgroup walks the months in order: a lane carries its asset's forward-filled
//                  price and the month's base (the fill on the day before the month) in
//                  registers, the next month's day rows, labels and next_ret are loaded while
//                  this month is worked on, and P is read once whatever K is.  Per month the
//                  lanes' value relatives v = pff / base go to an LDS tile [asset][day]; the
//                  members of every (age, bin) cohort are listed by a stable counting sort of the
//                  slice (ascending asset within a bin), and a half-wave per (age, bin) -- a lane
//                  per day -- adds w * v over the bin's list in list order.  Out: the slice's
//                  partial sums [slice][age][bin][day] and, per month, its weight sums and member
//                  counts.
//   k_daily_finish one workgroup per month: slice partials added in ascending slice order,
//                  cohort values C = sum / weight, V = mean over the non-empty cohorts,
//                  DR = V[d] / V[d-1] - 1 (V = 1 on the day before the month), DLS, DCNT; NaN on
//                  every day without a portfolio.
//   k_series_stats one workgroup per series: count, mean, Sharpe, annualised volatility, maximum
//                  drawdown and final value of cumprod(1 + x), NaN entries dropped.
//
// Every sum has a fixed order (list order, slice order, shuffle trees), and there are no
// floating-point atomics: two calls on the same inputs give the same bits.
#include "csm_common.h"

#define DY_COLS 256              // assets per slice = threads per workgroup
#define DY_WAVES (DY_COLS / 64)
#define DY_HALF (DY_COLS / 32)   // half-waves: one (age, bin) list at a time each
#define DY_MAXK 12
#define DY_MAXNB 30
#define DY_MAXD 32

static inline int64_t dy_slices(int64_t N) { return (N + DY_COLS - 1) / DY_COLS; }
static inline size_t dy_up16(size_t x) { return (x + 15) & ~(size_t)15; }

// workspace: Sp [slices][K * n_bins][T_d] doubles, SWp [slices][T_m][K * n_bins] doubles,
// CNp [slices][T_m][K * n_bins] int32
struct DyWs {
  double* Sp;
  double* SWp;
  int32_t* CNp;
  size_t bytes;
};
static inline DyWs dy_layout(void* ws, int64_t T_d, int64_t N, int T_m, int n_bins, int K) {
  const size_t S = (size_t)dy_slices(N), KQ = (size_t)K * n_bins;
  const size_t b0 = dy_up16(S * KQ * (size_t)T_d * 8), b1 = dy_up16(S * (size_t)T_m * KQ * 8);
  const size_t b2 = dy_up16(S * (size_t)T_m * KQ * 4);
  char* p = (char*)ws;
  return DyWs{(double*)p, (double*)(p + b0), (int32_t*)(p + b0 + b1), b0 + b1 + b2};
}

// One month's inputs of a lane's asset: the day rows, next_ret of the held label row and the
// labels / weights of the K formation rows.
template <int MAXD, int KC, bool VW>
struct DyMonth {
  double p[MAXD];
  double nr;
  int lab[KC];
  double w[VW ? KC : 1];
};

// the day range of month m, clipped to the panel and to MAXD rows
__device__ __forceinline__ void dy_days(const int64_t* __restrict__ ms, int m, int64_t T_d,
                                        int maxd, int64_t& d0, int& nd) {
  int64_t a = ms[m], b = ms[m + 1];
  a = a < 0 ? 0 : (a > T_d ? T_d : a);
  b = b < a ? a : (b > T_d ? T_d : b);
  d0 = a;
  nd = (int)(b - a < (int64_t)maxd ? b - a : (int64_t)maxd);
}

template <int MAXD, int KC, bool VW>
__device__ __forceinline__ void dy_load(DyMonth<MAXD, KC, VW>& x, const double* __restrict__ P,
                                        const int64_t* __restrict__ ms, int m, int T_m,
                                        int64_t T_d, int64_t N, const int8_t* __restrict__ L,
                                        const double* __restrict__ NR,
                                        const double* __restrict__ W, int K, int64_t a,
                                        bool live) {
  const bool on = live && m < T_m;
  int64_t d0 = 0;
  int nd = 0;
  if (m < T_m) dy_days(ms, m, T_d, MAXD, d0, nd);
#pragma unroll
  for (int i = 0; i < MAXD; ++i) x.p[i] = (on && i < nd) ? P[(d0 + i) * N + a] : qnan();
  const int t = m - 1;   // the label row held over month m
  x.nr = (on && t >= 0) ? NR[(int64_t)t * N + a] : qnan();
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    const bool ok = on && k < K && t - k >= 0;
    x.lab[k] = ok ? (int)L[(int64_t)(t - k) * N + a] : -1;
    if (VW) x.w[k] = ok ? W[(int64_t)(t - k) * N + a] : 0.0;
  }
}

// LDS (dynamic): tile [DY_COLS][DP] doubles, then (VW) sorted weights [K][DY_COLS] doubles, then
// ints: cnt [K][DY_WAVES][NB], tot [K][NB], wb [K][DY_WAVES][NB], off [K][NB + 1], then the
// member lists perm [K][DY_COLS] bytes.
static inline size_t dy_lds_bytes(int maxd, int K, int n_bins, bool vw) {
  const size_t DP = (size_t)maxd | 1;
  size_t b = (size_t)DY_COLS * DP * 8;
  if (vw) b += (size_t)K * DY_COLS * 8;
  b += (size_t)K * (2 * DY_WAVES * n_bins + n_bins + n_bins + 1) * 4;
  b += (size_t)K * DY_COLS;
  return dy_up16(b);
}

template <int MAXD, int KC, bool VW>
__global__ __launch_bounds__(DY_COLS) void k_daily(
    const double* __restrict__ P, int64_t T_d, int64_t N, const int64_t* __restrict__ ms, int T_m,
    const int8_t* __restrict__ L, const double* __restrict__ NR, const double* __restrict__ W,
    int NB, int K, double* __restrict__ Sp, double* __restrict__ SWp, int32_t* __restrict__ CNp) {
  constexpr int DP = MAXD | 1;   // odd row stride: a wave's tile stores and reads hit every bank
  extern __shared__ __attribute__((aligned(16))) double dy_lds[];
  double* tile = dy_lds;
  double* wsrt = tile + DY_COLS * DP;
  int* cnt = reinterpret_cast<int*>(wsrt + (VW ? K * DY_COLS : 0));
  int* tot = cnt + K * DY_WAVES * NB;
  int* wb = tot + K * NB;
  int* off = wb + K * DY_WAVES * NB;
  uint8_t* perm = reinterpret_cast<uint8_t*>(off + K * (NB + 1));

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t slice = blockIdx.x;
  const int64_t a = slice * DY_COLS + tid;
  const bool live = a < N;
  const int KQ = K * NB;
  const uint64_t lt = (1ull << lane) - 1ull;
  const int hw = tid >> 5, day = tid & 31;

  for (int i = tid; i < K * DY_WAVES * NB; i += DY_COLS) cnt[i] = 0;
  double last = qnan();   // the asset's forward-filled price
  DyMonth<MAXD, KC, VW> cur, nxt;
  dy_load(cur, P, ms, 0, T_m, T_d, N, L, NR, W, K, a, live);
  __syncthreads();

  for (int m = 0; m < T_m; ++m) {   // (block-uniform)
    dy_load(nxt, P, ms, m + 1, T_m, T_d, N, L, NR, W, K, a, live);
    int64_t d0;
    int nd;
    dy_days(ms, m, T_d, MAXD, d0, nd);
    const double base = last;
    const bool okb = base > 0.0 && base < INFINITY;
    if (m == 0) {   // no portfolio yet: only the fill moves on
#pragma unroll
      for (int i = 0; i < MAXD; ++i) {
        const double x = cur.p[i];   // NaN beyond the month's rows
        last = x == x ? x : last;
      }
    } else {
      const int t = m - 1;
      const int kmax = t + 1 < K ? t + 1 : K;
      const bool elig = live && okb && cur.nr == cur.nr;
      // ---- A: rank of each lane among its wave's lanes of the same (age, bin), from
      // bit-sliced ballots; the last lane of a group leaves the group's size
      int lab[KC], rank[KC];
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        int l = (k < kmax && elig) ? cur.lab[k] : -1;
        if (l >= NB) l = -1;
        if (VW) {
          if (!(cur.w[k] > 0.0 && cur.w[k] < INFINITY)) l = -1;   // NaN fails w > 0
        }
        lab[k] = l;
        rank[k] = 0;
        if (k < kmax) {   // (block-uniform)
          uint64_t same = __ballot(l >= 0);
#pragma unroll
          for (int bb = 0; bb < 5; ++bb) {
            const bool bit = (l >> bb) & 1;
            const uint64_t mk = __ballot(bit);
            same &= bit ? mk : ~mk;
          }
          if (l >= 0) {
            rank[k] = __popcll(same & lt);
            if (rank[k] == __popcll(same) - 1) cnt[(k * DY_WAVES + wid) * NB + l] = rank[k] + 1;
          }
        }
      }
      __syncthreads();
      // ---- B: members per (age, bin)
      for (int i = tid; i < kmax * NB; i += DY_COLS) {
        const int k = i / NB, q = i - k * NB;
        int s = 0;
        for (int w2 = 0; w2 < DY_WAVES; ++w2) s += cnt[(k * DY_WAVES + w2) * NB + q];
        tot[i] = s;
      }
      __syncthreads();
      // ---- C: list offsets of each (age, bin) and of each wave's run inside it
      for (int i = tid; i < kmax * NB; i += DY_COLS) {
        const int k = i / NB, q = i - k * NB;
        int run = 0;
        for (int q2 = 0; q2 < q; ++q2) run += tot[k * NB + q2];
        off[k * (NB + 1) + q] = run;
        if (q == NB - 1) off[k * (NB + 1) + NB] = run + tot[i];
        for (int w2 = 0; w2 < DY_WAVES; ++w2) {
          wb[(k * DY_WAVES + w2) * NB + q] = run;
          run += cnt[(k * DY_WAVES + w2) * NB + q];
        }
      }
      __syncthreads();
      // ---- D: the lane's value relatives (the row of a lane that is no member of anything is
      // never read), the lists (ascending asset inside a bin), counters back to zero
#pragma unroll
      for (int i = 0; i < MAXD; ++i) {
        const double x = cur.p[i];   // NaN beyond the month's rows
        last = x == x ? x : last;
        if (i < nd) tile[tid * DP + i] = last / base;
      }
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        if (k < kmax && lab[k] >= 0) {
          const int pos = wb[(k * DY_WAVES + wid) * NB + lab[k]] + rank[k];
          perm[k * DY_COLS + pos] = (uint8_t)tid;
          if (VW) wsrt[k * DY_COLS + pos] = cur.w[k];
          if (rank[k] == 0) cnt[(k * DY_WAVES + wid) * NB + lab[k]] = 0;   // one lane per group
        }
      }
      __syncthreads();
      // ---- E: a half-wave per (age, bin), a lane per day: w * v added in list order
      for (int pr = hw; pr < kmax * NB; pr += DY_HALF) {
        const int k = pr / NB, q = pr - k * NB;
        const int j0 = off[k * (NB + 1) + q], j1 = off[k * (NB + 1) + q + 1];
        const uint8_t* pl = perm + k * DY_COLS;
        const double* wl = wsrt + k * DY_COLS;
        const int dd = day < nd ? day : 0;
        double s = 0.0, sw = 0.0;
        int j = j0;
        for (; j + 4 <= j1; j += 4) {
          double x[4], wt[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            x[u] = tile[(int)pl[j + u] * DP + dd];
            wt[u] = VW ? wl[j + u] : 1.0;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            s += VW ? wt[u] * x[u] : x[u];
            sw += wt[u];
          }
        }
        for (; j < j1; ++j) {
          const double x = tile[(int)pl[j] * DP + dd];
          const double wt = VW ? wl[j] : 1.0;
          s += VW ? wt * x : x;
          sw += wt;
        }
        if (day < nd) Sp[(slice * KQ + pr) * T_d + d0 + day] = s;
        if (day == 0) {
          const int64_t o = (slice * T_m + t) * KQ + pr;
          SWp[o] = sw;
          CNp[o] = j1 - j0;
        }
      }
      // (no barrier here: the next month writes tile / perm / off / wsrt only after its own
      // barriers, which no lane passes before every half-wave is done with this month)
    }
    cur = nxt;
  }
}

// LDS: sw [K * NB] doubles, cn [K * NB] ints, V [(DY_MAXD + 1)][NB] doubles
__global__ __launch_bounds__(256) void k_daily_finish(
    int64_t T_d, int64_t N, const int64_t* __restrict__ ms, int T_m, int maxd, int NB, int K,
    const double* __restrict__ Sp, const double* __restrict__ SWp,
    const int32_t* __restrict__ CNp, int64_t S, double* __restrict__ DR,
    double* __restrict__ DLS, int32_t* __restrict__ DCNT) {
  __shared__ double sh_sw[DY_MAXK * DY_MAXNB];
  __shared__ int sh_cn[DY_MAXK * DY_MAXNB];
  __shared__ double sh_v[(DY_MAXD + 1) * DY_MAXNB];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int KQ = K * NB;
  const double nan = qnan();
  // days without a portfolio: month 0 (and anything before it), whatever follows the last
  // month, and the days of a month beyond maxd rows
  int64_t f0 = 0, f1 = 0;
  int64_t d0 = 0;
  int nd = 0;
  if (m == T_m) {
    int64_t e = ms[T_m];
    f0 = e < 0 ? 0 : (e > T_d ? T_d : e);
    f1 = T_d;
  } else {
    dy_days(ms, m, T_d, maxd, d0, nd);
    int64_t e = ms[m + 1];
    e = e < d0 ? d0 : (e > T_d ? T_d : e);
    if (m == 0) { f0 = 0; f1 = e; nd = 0; }
    else { f0 = d0 + nd; f1 = e; }
  }
  for (int64_t i = f0 * NB + tid; i < f1 * NB; i += 256) DR[i] = nan;
  for (int64_t i = f0 + tid; i < f1; i += 256) DLS[i] = nan;
  if (m == 0) return;
  const int t = m - 1;   // DCNT row; holding month m (none for m == T_m)
  const int kmax = m == T_m ? 0 : (t + 1 < K ? t + 1 : K);
  for (int i = tid; i < KQ; i += 256) {
    const int k = i / NB;
    double sw = 0.0;
    int cn = 0;
    if (k < kmax)
      for (int64_t s = 0; s < S; ++s) {
        sw += SWp[(s * T_m + t) * KQ + i];
        cn += CNp[(s * T_m + t) * KQ + i];
      }
    sh_sw[i] = sw;
    sh_cn[i] = cn;
    if (DCNT) DCNT[(int64_t)t * KQ + i] = cn;
  }
  if (m == T_m) return;
  for (int q = tid; q < NB; q += 256) sh_v[q] = 1.0;   // the day before the month
  __syncthreads();
  for (int i = tid; i < nd * NB; i += 256) {
    const int q = i / nd, d = i - q * nd;
    double vs = 0.0;
    int nc = 0;
    for (int k = 0; k < kmax; ++k) {
      if (sh_cn[k * NB + q] <= 0) continue;
      const double* sp = Sp + (int64_t)(k * NB + q) * T_d + d0 + d;
      const int64_t st = (int64_t)KQ * T_d;
      double s = 0.0;
      int64_t sl = 0;
      for (; sl + 8 <= S; sl += 8) {   // 8 slices' partials in flight, added in slice order
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = sp[(sl + u) * st];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += x[u];
      }
      for (; sl < S; ++sl) s += sp[sl * st];
      vs += s / sh_sw[k * NB + q];
      ++nc;
    }
    sh_v[(d + 1) * NB + q] = nc > 0 ? vs / (double)nc : nan;
  }
  __syncthreads();
  for (int i = tid; i < nd * NB; i += 256) {
    const int d = i / NB, q = i - d * NB;
    DR[(d0 + d) * NB + q] = sh_v[(d + 1) * NB + q] / sh_v[d * NB + q] - 1.0;
  }
  for (int d = tid; d < nd; d += 256) {
    const double top = sh_v[(d + 1) * NB + NB - 1] / sh_v[d * NB + NB - 1] - 1.0;
    const double bot = sh_v[(d + 1) * NB] / sh_v[d * NB] - 1.0;
    DLS[d0 + d] = top - bot;   // NaN if either leg is
  }
}

// ------------------------------------------------------------------------- series statistics
#define ST_THREADS 256
#define ST_CHUNK 1024
#define ST_FIELDS 6
__device__ __forceinline__ double st_block_sum(double v, double* scr) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) scr[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < ST_THREADS / 64; ++w) s += scr[w];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(ST_THREADS) void k_series_stats(const double* __restrict__ X, int T,
                                                             int64_t stride, double freq,
                                                             double* __restrict__ out) {
  __shared__ double scr[ST_THREADS / 64];
  __shared__ double buf[ST_CHUNK];
  const int s = blockIdx.x, tid = threadIdx.x;
  const double* xs = X + s;
  double n = 0.0, sum = 0.0;
  for (int i = tid; i < T; i += ST_THREADS) {
    const double x = xs[(int64_t)i * stride];
    if (x == x) { n += 1.0; sum += x; }
  }
  n = st_block_sum(n, scr);
  sum = st_block_sum(sum, scr);
  const double mean = sum / n;   // NaN for an empty series
  double v = 0.0;
  for (int i = tid; i < T; i += ST_THREADS) {
    const double x = xs[(int64_t)i * stride];
    if (x == x) v += (x - mean) * (x - mean);
  }
  v = st_block_sum(v, scr);
  // the curve is a sequential product (cumprod's own order): chunks staged in LDS by the
  // workgroup, walked by one lane
  double cum = 1.0, peak = 1.0, mdd = 0.0;
  for (int c0 = 0; c0 < T; c0 += ST_CHUNK) {
    const int nc = T - c0 < ST_CHUNK ? T - c0 : ST_CHUNK;
    for (int i = tid; i < nc; i += ST_THREADS) buf[i] = xs[(int64_t)(c0 + i) * stride];
    __syncthreads();
    if (tid == 0) {
      for (int i = 0; i < nc; ++i) {
        const double x = buf[i];
        if (x == x) {
          cum *= 1.0 + x;
          peak = cum > peak ? cum : peak;
          const double dd = 1.0 - cum / peak;
          mdd = dd > mdd ? dd : mdd;
        }
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double sd = sqrt(v / (n - 1.0));
    const double rf = sqrt(freq);
    double* o = out + (int64_t)s * ST_FIELDS;
    const bool any = n > 0.0;
    o[0] = n;
    o[1] = mean;
    o[2] = sd > 0.0 ? mean * freq / (sd * rf) : qnan();
    o[3] = any ? sd * rf : qnan();
    o[4] = any ? mdd : qnan();
    o[5] = any ? cum : qnan();
  }
}

static bool dy_nbins_ok(int n_bins) {   // the set csm_portfolio accepts
  return nb_dispatch<2, 3, 4, 5, 10, 20, 30>(n_bins, [](auto) {});
}

template <int MAXD, int KC>
static const void* dy_kernel(bool vw) {
  return vw ? (const void*)k_daily<MAXD, KC, true> : (const void*)k_daily<MAXD, KC, false>;
}
template <int MAXD>
static const void* dy_kernel_k(int K, bool vw) {
  return K == 1 ? dy_kernel<MAXD, 1>(vw) : K <= 6 ? dy_kernel<MAXD, 6>(vw)
                                                  : dy_kernel<MAXD, DY_MAXK>(vw);
}

extern "C" {

int64_t csm_daily_workspace(int64_t T_d, int64_t N, int32_t T_m, int32_t n_bins, int32_t K) {
  if (T_d < 1 || N < 1 || T_m < 1 || n_bins < 1 || K < 1) return 0;
  return (int64_t)dy_layout(nullptr, T_d, N, T_m, n_bins, K).bytes;
}

int csm_daily_returns(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N,
                      const int64_t* month_start, int32_t T_m, int32_t max_month_days,
                      const int8_t* L, const double* NR, const double* W, int32_t n_bins,
                      int32_t K, double* DR, double* DLS, int32_t* DCNT, void* workspace) {
  int r = prep(ctx);
  if (r) return r;
  if (!P || !month_start || !L || !NR || !DR || !DLS || !workspace || T_d < 1 || N < 1 ||
      T_m < 1 || T_d > ((int64_t)1 << 40) / N)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_returns: bad arguments (T_d=%lld N=%lld T_m=%d)",
                   (long long)T_d, (long long)N, T_m);
  if (!dy_nbins_ok(n_bins))
    return set_err(ctx, CSM_E_INVAL, "csm_daily_returns: n_bins=%d is not one of 2,3,4,5,10,20,30",
                   n_bins);
  if (K < 1 || K > DY_MAXK)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_returns: K=%d is outside [1, %d]", K, DY_MAXK);
  if (max_month_days < 1 || max_month_days > DY_MAXD)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_returns: max_month_days=%d is outside [1, %d]",
                   max_month_days, DY_MAXD);
  const DyWs ws = dy_layout(workspace, T_d, N, T_m, n_bins, K);
  const int64_t S = dy_slices(N);
  const bool vw = W != nullptr;
  const int maxd = max_month_days <= 23 ? 23 : 32;   // the compiled month lengths
  const void* kern = maxd == 23 ? dy_kernel_k<23>(K, vw) : dy_kernel_k<32>(K, vw);
  const size_t lds = dy_lds_bytes(maxd, K, n_bins, vw);
  HIP_CHECK(ctx, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  int nb = n_bins, k = K, tm = T_m;
  double* Sp = ws.Sp;
  double* SWp = ws.SWp;
  int32_t* CNp = ws.CNp;
  void* args[] = {(void*)&P, (void*)&T_d, (void*)&N, (void*)&month_start, (void*)&tm, (void*)&L,
                  (void*)&NR, (void*)&W, (void*)&nb, (void*)&k, (void*)&Sp, (void*)&SWp,
                  (void*)&CNp};
  HIP_CHECK(ctx, hipLaunchKernel(kern, dim3((unsigned)S), dim3(DY_COLS), args, lds, ctx->stream));
  hipLaunchKernelGGL(k_daily_finish, dim3((unsigned)T_m + 1), dim3(256), 0, ctx->stream, T_d, N,
                     month_start, T_m, maxd, n_bins, K, (const double*)ws.Sp,
                     (const double*)ws.SWp, (const int32_t*)ws.CNp, S, DR, DLS, DCNT);
  LAUNCH_CHECK(ctx, "k_daily_finish");
  return CSM_OK;
}

int csm_series_stats(csm_ctx* ctx, const double* X, int32_t nS, int32_t T, int64_t stride,
                     double freq, double* out) {
  int r = prep(ctx);
  if (r) return r;
  if (!X || !out || nS < 1 || T < 0 || stride < 1 || !(freq > 0.0))
    return set_err(ctx, CSM_E_INVAL, "csm_series_stats: bad arguments (nS=%d T=%d stride=%lld)",
                   nS, T, (long long)stride);
  hipLaunchKernelGGL(k_series_stats, dim3((unsigned)nS), dim3(ST_THREADS), 0, ctx->stream, X, T,
                     stride, freq, out);
  LAUNCH_CHECK(ctx, "k_series_stats");
  return CSM_OK;
}

}  // extern "C"
