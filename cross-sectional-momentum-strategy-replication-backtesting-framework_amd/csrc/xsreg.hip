// xsreg.hip -- Fama-MacBeth cross-sectional regressions on the signal panels (rules R1..R6 in
// DESIGN.md 7): each month's regression of Y on K signals across the assets (OLS, WLS, ridge on
// z-scores), and the time-series mean of any series with its Newey-West t-statistic.
//
//   k_xs_mean      R1, R2.  The grid is (slice of XS_SLICE assets) x (month), k_market_factor's;
//                  a lane owns XS_PER assets of its slice, XS_THREADS apart, and sums w, w y and
//                  w s_k over them in that order from 0.0.  Each wave is reduced by the halving
//                  tree of __shfl_down over 64 lanes, the four wave sums are added in wave order
//                  and the workgroup leaves one partial per sum and slice.
//   k_xs_totals    R2.  A lane per (month, sum) adds the slices' partials in slice order from
//                  0.0: the month's sw, sy, ss_k and n.  (Summed by every workgroup of
//                  k_xs_moments instead, the 49 loads in a row cost far more than this launch:
//                  1.33 against 0.80 ms at 100,000 x 461, K = 4.)
//   k_xs_moments   R3.  my = sy / sw and ms_k = ss_k / sw by K + 1 lanes of each workgroup, then
//                  its partials of the (K + 1)(K + 2) / 2 centred moments, left as k_xs_mean's.
//   k_xs_solve     R3..R5.  A lane per month adds the slices' moment partials in slice order,
//                  scales, adds the ridge and solves by Cholesky.
//   k_newey_west   R6.  A wave per column: the column is staged and its NaNs closed up in LDS
//                  (a series longer than NW_LDS_MAX in a device workspace), lane 0 sums it in
//                  time order, then lane l sums lag l's products in time order and lane 0 adds the
//                  lags' terms in lag order -- each sum sequential, as R6 states it.
//
// The order of every sum is a function of N alone: no float atomic, no knob, nothing that depends
// on the launch.  Launching the two passes over chunks of 12 or 30 months, so that the second
// finds the first one's rows in the last-level cache, measured slower at every K
// and is not kept.
#include "csm_common.h"

#define XS_THREADS 256
#define XS_PER 8          // assets per lane: their loads of every row are issued before any sum
#define XS_SLICE (XS_THREADS * XS_PER)
#define XS_WAVES (XS_THREADS / 64)
#define XS_MAXK 8
#define XS_PIVOT 0x1p-40  // R5: a pivot must keep this much of its diagonal

#define NW_THREADS 64
#define NW_LDS_MAX 8000   // entries of a column that k_newey_west stages in LDS (62.5 KiB)

struct XsIn {
  const double* Y;
  const double* W;   // NULL: w = 1.0
  const double* S[XS_MAXK];
};

constexpr int xs_n1(int K) { return K + 2; }                    // sw, sy, ss_k
constexpr int xs_n2(int K) { return (K + 1) * (K + 2) / 2; }    // C_jk (j <= k), c_k, cyy

// The lane sums acc[NS] of a workgroup -> one partial per sum at out[0..NS): R1's tree per wave,
// then the wave sums in wave order from 0.0.  s_part is [XS_WAVES][NS] of LDS; the trailing
// barrier lets the next month reuse it.
template <int NS>
__device__ __forceinline__ void block_partials(double (&acc)[NS], double* s_part,
                                               double* __restrict__ out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int q = 0; q < NS; ++q) {
    const double v = wave_tree(acc[q]);
    if (lane == 0) s_part[wave * NS + q] = v;
  }
  __syncthreads();
  if (tid < NS) {
    double r = 0.0;
#pragma unroll
    for (int w = 0; w < XS_WAVES; ++w) r = r + s_part[w * NS + tid];
    out[tid] = r;
  }
  __syncthreads();
}

// One lane's XS_PER cells of month t: y, w and the K signals, every load issued before any use;
// ok[k] = the cell is an observation (R2).  A cell past N is loaded as NaN.
template <int K>
__device__ __forceinline__ void xs_load(const XsIn& in, int64_t row, int64_t a0, int64_t N,
                                        double (&y)[XS_PER], double (&w)[XS_PER],
                                        double (&s)[K][XS_PER], bool (&ok)[XS_PER]) {
#pragma unroll
  for (int k = 0; k < XS_PER; ++k) {
    const int64_t a = a0 + (int64_t)k * XS_THREADS;
    const bool live = a < N;
    y[k] = live ? in.Y[row + a] : qnan();
    w[k] = (live && in.W) ? in.W[row + a] : 1.0;
#pragma unroll
    for (int q = 0; q < K; ++q) s[q][k] = live ? in.S[q][row + a] : qnan();
  }
#pragma unroll
  for (int k = 0; k < XS_PER; ++k) {
    bool o = !isnan_d(y[k]) && w[k] > 0.0;   // (a NaN weight is not > 0)
#pragma unroll
    for (int q = 0; q < K; ++q) o = o && !isnan_d(s[q][k]);
    ok[k] = o;
  }
}

// ------------------------------------------------------------------------------- R1, R2
template <int K>
__global__ __launch_bounds__(XS_THREADS) void k_xs_mean(XsIn in, int T_m, int64_t N,
                                                        double* __restrict__ p1,
                                                        int32_t* __restrict__ pcnt) {
  constexpr int NS = xs_n1(K);
  __shared__ double s_part[XS_WAVES * NS];
  __shared__ int s_cnt[XS_WAVES];
  const int tid = threadIdx.x;
  const int64_t a0 = (int64_t)blockIdx.x * XS_SLICE + tid;
  for (int t = (int)blockIdx.y; t < T_m; t += (int)gridDim.y) {   // (uniform)
    double y[XS_PER], w[XS_PER], s[K][XS_PER];
    bool ok[XS_PER];
    xs_load<K>(in, (int64_t)t * N, a0, N, y, w, s, ok);
    double acc[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) acc[q] = 0.0;
    int c = 0;
#pragma unroll
    for (int k = 0; k < XS_PER; ++k) {
      const double wk = ok[k] ? w[k] : 0.0;
      acc[0] = acc[0] + wk;
      acc[1] = acc[1] + (ok[k] ? wk * y[k] : 0.0);
#pragma unroll
      for (int q = 0; q < K; ++q) acc[2 + q] = acc[2 + q] + (ok[k] ? wk * s[q][k] : 0.0);
      c += ok[k] ? 1 : 0;
    }
    const int64_t cell = (int64_t)t * gridDim.x + blockIdx.x;
    c = wave_tree(c);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = c;
    block_partials<NS>(acc, s_part, p1 + cell * NS);   // (its barriers order s_cnt too)
    if (tid == 0) pcnt[cell] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    __syncthreads();   // s_cnt is read before the next month's counts land
  }
}

// The slices' partials of month t, added in slice order from 0.0: tot [T_m][n1] and n [T_m].
// Lane (t, q) owns sum q of month t; q = n1 is the count.
__global__ __launch_bounds__(64) void k_xs_totals(const double* __restrict__ p1,
                                                  const int32_t* __restrict__ pcnt, int T_m,
                                                  int slices, int n1, double* __restrict__ tot,
                                                  int32_t* __restrict__ cnt) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)T_m * (n1 + 1)) return;
  const int t = (int)(id / (n1 + 1)), q = (int)(id % (n1 + 1));
  if (q == n1) {
    int c = 0;
    for (int i = 0; i < slices; ++i) c += pcnt[(int64_t)t * slices + i];
    cnt[t] = c;
  } else {
    double s = 0.0;
    for (int i = 0; i < slices; ++i) s = s + p1[((int64_t)t * slices + i) * n1 + q];
    tot[(int64_t)t * n1 + q] = s;
  }
}

// --------------------------------------------------------------------------------- R3
template <int K>
__global__ __launch_bounds__(XS_THREADS) void k_xs_moments(XsIn in, int T_m, int64_t N,
                                                           const double* __restrict__ tot,
                                                           double* __restrict__ p2) {
  constexpr int N1 = xs_n1(K), NS = xs_n2(K);
  __shared__ double s_part[XS_WAVES * NS];
  __shared__ double s_mean[K + 1];   // my, ms_k
  const int tid = threadIdx.x;
  const int slices = (int)gridDim.x;
  const int64_t a0 = (int64_t)blockIdx.x * XS_SLICE + tid;
  for (int t = (int)blockIdx.y; t < T_m; t += (int)gridDim.y) {   // (uniform)
    double y[XS_PER], w[XS_PER], s[K][XS_PER];
    bool ok[XS_PER];
    xs_load<K>(in, (int64_t)t * N, a0, N, y, w, s, ok);
    if (tid < K + 1) s_mean[tid] = tot[(int64_t)t * N1 + 1 + tid] / tot[(int64_t)t * N1];
    __syncthreads();
    const double my = s_mean[0];
    double ms[K];
#pragma unroll
    for (int q = 0; q < K; ++q) ms[q] = s_mean[1 + q];
    double acc[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) acc[q] = 0.0;
#pragma unroll
    for (int k = 0; k < XS_PER; ++k) {
      const double dy = y[k] - my, wdy = w[k] * dy;
      double d[K], wd[K];
#pragma unroll
      for (int q = 0; q < K; ++q) {
        d[q] = s[q][k] - ms[q];
        wd[q] = w[k] * d[q];
      }
      int u = 0;
#pragma unroll
      for (int j = 0; j < K; ++j)
#pragma unroll
        for (int q = j; q < K; ++q, ++u) acc[u] = acc[u] + (ok[k] ? wd[j] * d[q] : 0.0);
#pragma unroll
      for (int q = 0; q < K; ++q, ++u) acc[u] = acc[u] + (ok[k] ? wd[q] * dy : 0.0);
      acc[u] = acc[u] + (ok[k] ? wdy * dy : 0.0);
    }
    const int64_t cell = (int64_t)t * slices + blockIdx.x;
    block_partials<NS>(acc, s_part, p2 + cell * NS);   // (its last barrier covers s_mean too)
  }
}

// ------------------------------------------------------------------------------ R3..R5
template <int K>
__global__ __launch_bounds__(64) void k_xs_solve(const double* __restrict__ tot,
                                                 const int32_t* __restrict__ cnt,
                                                 const double* __restrict__ p2, int T_m,
                                                 int slices, int standardize, double ridge,
                                                 int min_obs, double* __restrict__ GAMMA,
                                                 double* __restrict__ R2,
                                                 int32_t* __restrict__ NOBS) {
  constexpr int N1 = xs_n1(K), NS = xs_n2(K);
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= T_m) return;
  const double NaN = qnan();
  double m1[N1], m2[NS];
#pragma unroll
  for (int q = 0; q < N1; ++q) m1[q] = tot[(int64_t)t * N1 + q];
#pragma unroll
  for (int q = 0; q < NS; ++q) m2[q] = 0.0;
  const int n = cnt[t];
  for (int i = 0; i < slices; ++i) {
    const int64_t cell = (int64_t)t * slices + i;
#pragma unroll
    for (int q = 0; q < NS; ++q) m2[q] = m2[q] + p2[cell * NS + q];
  }
  if (NOBS) NOBS[t] = n;
  double out[K + 1];
#pragma unroll
  for (int q = 0; q <= K; ++q) out[q] = NaN;
  double r2 = NaN;
  // R3's moments into a full symmetric matrix
  double C[K][K], c[K];
  {
    int u = 0;
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
      for (int q = j; q < K; ++q, ++u) C[j][q] = C[q][j] = m2[u];
#pragma unroll
    for (int q = 0; q < K; ++q, ++u) c[q] = m2[u];
  }
  const double cyy = m2[NS - 1];
  bool def = n >= min_obs && cyy > 0.0;
#pragma unroll
  for (int q = 0; q < K; ++q) def = def && C[q][q] > 0.0;
  if (def) {
    const double sw = m1[0], my = m1[1] / sw;
    // R4
    double A0[K][K], b[K];
    if (standardize) {
      double sd[K];
#pragma unroll
      for (int q = 0; q < K; ++q) sd[q] = sqrt(C[q][q] / sw);
#pragma unroll
      for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int q = 0; q < K; ++q) A0[j][q] = C[j][q] / (sd[j] * sd[q]);
        b[j] = c[j] / sd[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int q = 0; q < K; ++q) A0[j][q] = C[j][q];
        b[j] = c[j];
      }
    }
    // R5: Cholesky of A = A0 + ridge on the diagonal
    double L[K][K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const double ajj = A0[j][j] + ridge;
      double d = ajj;
#pragma unroll
      for (int p = 0; p < j; ++p) d = d - L[j][p] * L[j][p];
      def = def && d > ajj * XS_PIVOT;
      L[j][j] = sqrt(d);
#pragma unroll
      for (int i = j + 1; i < K; ++i) {
        double v = A0[i][j];
#pragma unroll
        for (int p = 0; p < j; ++p) v = v - L[i][p] * L[j][p];
        L[i][j] = v / L[j][j];
      }
    }
    if (def) {
      double z[K], g[K];
#pragma unroll
      for (int j = 0; j < K; ++j) {
        double sm = 0.0;
#pragma unroll
        for (int p = 0; p < j; ++p) sm = sm + L[j][p] * z[p];
        z[j] = (b[j] - sm) / L[j][j];
      }
#pragma unroll
      for (int j = K - 1; j >= 0; --j) {
        double sm = 0.0;
#pragma unroll
        for (int p = j + 1; p < K; ++p) sm = sm + L[p][j] * g[p];
        g[j] = (z[j] - sm) / L[j][j];
      }
      double g0 = my;
      if (!standardize) {
#pragma unroll
        for (int q = 0; q < K; ++q) g0 = g0 - g[q] * (m1[2 + q] / sw);
      }
      double gb = 0.0, gAg = 0.0;
#pragma unroll
      for (int j = 0; j < K; ++j) gb = gb + g[j] * b[j];
#pragma unroll
      for (int j = 0; j < K; ++j) {
        double r = 0.0;
#pragma unroll
        for (int q = 0; q < K; ++q) r = r + A0[j][q] * g[q];
        gAg = gAg + g[j] * r;
      }
      const double rss = (cyy - 2.0 * gb) + gAg;
      r2 = 1.0 - rss / cyy;
      out[0] = g0;
#pragma unroll
      for (int q = 0; q < K; ++q) out[1 + q] = g[q];
    }
  }
#pragma unroll
  for (int q = 0; q <= K; ++q) GAMMA[(int64_t)t * (K + 1) + q] = out[q];
  if (R2) R2[t] = r2;
}

// --------------------------------------------------------------------------------- R6
__global__ __launch_bounds__(NW_THREADS) void k_newey_west(const double* __restrict__ G, int T,
                                                           int64_t ld, int lags, double* ws,
                                                           double* __restrict__ MEAN,
                                                           double* __restrict__ SE,
                                                           double* __restrict__ TSTAT,
                                                           int32_t* __restrict__ NT) {
  extern __shared__ __attribute__((aligned(16))) double nw_lds[];
  __shared__ double s_a[NW_THREADS];
  __shared__ double s_mean;
  __shared__ int s_n;
  const int col = (int)blockIdx.x, lane = threadIdx.x;
  const double* __restrict__ g = G + col;
  double* u = ws ? ws + (int64_t)col * T : nw_lds;   // the column, then its u_i, gaps closed
  for (int i = lane; i < T; i += NW_THREADS) u[i] = g[(int64_t)i * ld];
  __syncthreads();
  if (lane == 0) {   // close the gaps in place (n <= i) and sum in time order
    int n = 0;
    double sm = 0.0;
    for (int i = 0; i < T; ++i) {
      const double x = u[i];
      if (!isnan_d(x)) {
        sm = sm + x;
        u[n++] = x;
      }
    }
    s_n = n;
    s_mean = n > 0 ? sm / (double)n : qnan();
  }
  __syncthreads();
  const int n = s_n;
  const double mean = s_mean;
  for (int i = lane; i < n; i += NW_THREADS) u[i] = u[i] - mean;
  __syncthreads();
  double var = 0.0;   // (lane 0's)
  const bool def = n >= 2 && lags <= n - 2;   // (uniform)
  if (def) {
    for (int l0 = 0; l0 <= lags; l0 += NW_THREADS) {
      const int l = l0 + lane;
      if (l <= lags) {
        double a = 0.0;
        for (int i = l; i < n; ++i) a = a + u[i] * u[i - l];
        s_a[lane] = a / (double)n;
      }
      __syncthreads();
      if (lane == 0) {
        for (int k = 0; k < NW_THREADS && l0 + k <= lags; ++k) {
          const int L = l0 + k;
          var = L == 0 ? s_a[0]
                       : var + (2.0 * (1.0 - (double)L / ((double)lags + 1.0))) * s_a[k];
        }
      }
      __syncthreads();   // s_a is read before the next lags land
    }
  }
  if (lane == 0) {
    double se = qnan(), ts = qnan();
    if (def && var > 0.0) {
      se = sqrt(var / (double)n);
      ts = mean / se;
    }
    MEAN[col] = mean;
    if (SE) SE[col] = se;
    if (TSTAT) TSTAT[col] = ts;
    if (NT) NT[col] = n;
  }
}

struct XsWs {
  double* p1;      // [T_m][slices][n1] k_xs_mean's partials
  int32_t* pcnt;   // [T_m][slices] its counts
  double* p2;      // [T_m][slices][n2] k_xs_moments's partials
  double* tot;     // [T_m][n1] the months' totals of p1
  int32_t* cnt;    // [T_m] and of pcnt
};

template <int K>
static int xs_launch(csm_ctx* ctx, const XsIn& in, int T_m, int64_t N, int slices, int standardize,
                     double ridge, int min_obs, const XsWs& w, double* GAMMA, double* R2,
                     int32_t* NOBS) {
  const dim3 grid((unsigned)slices, (unsigned)(T_m < 65535 ? T_m : 65535));
  hipLaunchKernelGGL(k_xs_mean<K>, grid, dim3(XS_THREADS), 0, ctx->stream, in, T_m, N, w.p1,
                     w.pcnt);
  LAUNCH_CHECK(ctx, "k_xs_mean");
  const int64_t lanes = (int64_t)T_m * (xs_n1(K) + 1);
  hipLaunchKernelGGL(k_xs_totals, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, ctx->stream,
                     w.p1, w.pcnt, T_m, slices, xs_n1(K), w.tot, w.cnt);
  LAUNCH_CHECK(ctx, "k_xs_totals");
  hipLaunchKernelGGL(k_xs_moments<K>, grid, dim3(XS_THREADS), 0, ctx->stream, in, T_m, N, w.tot,
                     w.p2);
  LAUNCH_CHECK(ctx, "k_xs_moments");
  hipLaunchKernelGGL(k_xs_solve<K>, dim3((unsigned)((T_m + 63) / 64)), dim3(64), 0, ctx->stream,
                     w.tot, w.cnt, w.p2, T_m, slices, standardize, ridge, min_obs, GAMMA, R2,
                     NOBS);
  LAUNCH_CHECK(ctx, "k_xs_solve");
  return CSM_OK;
}

extern "C" {

int csm_xs_regress(csm_ctx* ctx, const double* Y, const double* const* S, int32_t K,
                   const double* W, int32_t T_m, int64_t N, int32_t standardize, double ridge,
                   int32_t min_obs, double* GAMMA, double* R2, int32_t* NOBS) {
  int r = prep(ctx);
  if (r) return r;
  if (!Y || !S || !GAMMA || bad_panel(T_m, N))
    return set_err(ctx, CSM_E_INVAL, "csm_xs_regress: bad arguments (T_m=%d N=%lld)", T_m,
                   (long long)N);
  if (K < 1 || K > XS_MAXK)
    return set_err(ctx, CSM_E_INVAL, "csm_xs_regress: K=%d is outside [1, %d]", K, XS_MAXK);
  if (min_obs < K + 2)
    return set_err(ctx, CSM_E_INVAL, "csm_xs_regress: min_obs=%d must be at least K + 2 = %d",
                   min_obs, K + 2);
  if (!(ridge >= 0.0) || isinf(ridge))
    return set_err(ctx, CSM_E_INVAL, "csm_xs_regress: ridge=%g must be finite and >= 0", ridge);
  XsIn in{};
  in.Y = Y;
  in.W = W;
  for (int q = 0; q < K; ++q) {
    if (!S[q]) return set_err(ctx, CSM_E_INVAL, "csm_xs_regress: S[%d] is NULL", q);
    in.S[q] = S[q];
  }
  const int64_t slices = (N + XS_SLICE - 1) / XS_SLICE;
  const size_t cells = (size_t)T_m * (size_t)slices;
  const size_t n1 = (size_t)xs_n1(K), n2 = (size_t)xs_n2(K);
  r = ctx_reserve(ctx, "csm_xs_regress", "the partial-sum workspace", &ctx->xs_ws,
                  &ctx->xs_ws_bytes,
                  (cells * (n1 + n2) + (size_t)T_m * n1) * sizeof(double) +
                      (cells + (size_t)T_m) * sizeof(int32_t));
  if (r) return r;
  XsWs w;
  w.p1 = (double*)ctx->xs_ws;
  w.p2 = w.p1 + cells * n1;
  w.tot = w.p2 + cells * n2;
  w.pcnt = (int32_t*)(w.tot + (size_t)T_m * n1);
  w.cnt = w.pcnt + cells;
  r = CSM_E_INVAL;
  nb_dispatch<1, 2, 3, 4, 5, 6, 7, 8>(K, [&](auto k) {
    r = xs_launch<decltype(k)::value>(ctx, in, T_m, N, (int)slices, standardize != 0, ridge,
                                      min_obs, w, GAMMA, R2, NOBS);
  });
  return r;
}

int csm_newey_west(csm_ctx* ctx, const double* G, int32_t T, int32_t C, int64_t ld, int32_t lags,
                   double* MEAN, double* SE, double* TSTAT, int32_t* NT) {
  int r = prep(ctx);
  if (r) return r;
  if (!G || !MEAN || T < 1 || C < 1 || ld < C || lags < 0 || (int64_t)T > ((int64_t)1 << 40) / ld)
    return set_err(ctx, CSM_E_INVAL,
                   "csm_newey_west: bad arguments (T=%d C=%d ld=%lld lags=%d)", T, C,
                   (long long)ld, lags);
  double* ws = nullptr;
  if (T > NW_LDS_MAX) {   // (stream order keeps it apart from csm_xs_regress's use)
    r = ctx_reserve(ctx, "csm_newey_west", "the series workspace", &ctx->xs_ws, &ctx->xs_ws_bytes,
                    (size_t)T * (size_t)C * sizeof(double));
    if (r) return r;
    ws = (double*)ctx->xs_ws;
  }
  hipLaunchKernelGGL(k_newey_west, dim3((unsigned)C), dim3(NW_THREADS),
                     ws ? 0 : (size_t)T * sizeof(double), ctx->stream, G, T, ld, lags, ws, MEAN, SE,
                     TSTAT, NT);
  LAUNCH_CHECK(ctx, "k_newey_west");
  return CSM_OK;
}

}  // extern "C"
