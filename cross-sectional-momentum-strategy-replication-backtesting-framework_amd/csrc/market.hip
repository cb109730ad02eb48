// market.hip -- signals of the monthly cross-section (rules B1..B6 in DESIGN.md 7): the
// equal-weight market return, the market model of each asset on it (beta, alpha, idiosyncratic
// volatility, residual momentum) and the next return of any signal.
//
//   k_market_factor   B1, B2.  The grid is (slice of MF_SLICE assets) x (month); a lane owns
//                     MF_PER assets of its slice, MF_THREADS apart, and sums their x in that order
//                     from 0.0; the workgroup's lanes are summed by a halving tree in LDS.  A row
//                     of one slice is finished by its workgroup; a wider row leaves one (sum,
//                     count) pair per slice and k_market_finish adds them in slice order.  The
//                     order is a function of N alone: no atomic, no knob.
//   k_market_model    B1, B3..B5.  The grid is (64 assets) x (chunk of consecutive months); a lane
//                     owns one asset and keeps the window's Wb month returns in a slot-major LDS
//                     ring (the column layout of scan.h's ScanLane ring), next to one ring of the
//                     factor that the workgroup's lanes share.  A chunk starts cold Wb - 1 months
//                     before its first month and every window is summed again from its oldest
//                     month, so the chunk count (csm_tune "mm_chunks") only decides how many
//                     workgroups the launch has: every count gives the same bits.
//   k_factor_model    MF1..MF5.  k_market_model's shape on KF factors (a template on KF = 1..4):
//                     the shared factor ring holds a month's KF values side by side, pass 2
//                     gathers the packed normal equations, fsolve.h solves them per asset-month.
//                     At KF = 1 every operation is k_market_model's (rule MF8).
//   k_next_ret        B6.  A lane per asset walks the months with scan.h's rank_step /
//                     pending_finish on one (psff, prev) pair.
#include "csm_common.h"
#include "fsolve.h"
#include "scan.h"

#define MF_THREADS 256
#define MF_PER 8         // assets per lane: their loads of both rows are issued before any sum
#define MF_SLICE (MF_THREADS * MF_PER)
#define MM_THREADS 64
#define MM_MAXW 60
#define MM_BATCH 4       // ring entries a walk reads ahead of their use (6 measured the same, 12
                         // 3 % faster at Wb = 36 and no help to windows it does not divide)
#define NX_THREADS 64
#define NX_TRIP 4        // months per trip of k_next_ret: the next trip's loads are in flight

// the month chunks of k_market_model: 0 auto (scan.h auto_chunks) | n >= 1 that many (clamped to
// T_m); the month chunks of k_factor_model, the same values ("fm_chunks")
static int g_tune_mm_chunks = 0;
static int g_tune_fm_chunks = 0;
static const TuneKnob g_knobs[] = {
    {"mm_chunks", &g_tune_mm_chunks, [](int v) { return v >= 0; }},
    {"fm_chunks", &g_tune_fm_chunks, [](int v) { return v >= 0; }},
};

// B1: the month return over two calendar-adjacent month prices p (month t) and q (month t - 1).
__device__ __forceinline__ double month_ret(double p, double q) {
  return (!isnan_d(p) && !isnan_d(q)) ? p / q - 1.0 : qnan();
}

// ------------------------------------------------------------------------------- B1, B2
__device__ __forceinline__ void mf_finish(double s, int c, int min_assets, int t,
                                          double* __restrict__ MKT, int32_t* __restrict__ NMK) {
  MKT[t] = c >= min_assets ? s / (double)c : qnan();
  if (NMK) NMK[t] = c;
}

__global__ __launch_bounds__(MF_THREADS) void k_market_factor(
    const double* __restrict__ PM, int T_m, int64_t N, int min_assets, double* __restrict__ X,
    double* __restrict__ MKT, int32_t* __restrict__ NMK, double* __restrict__ psum,
    int32_t* __restrict__ pcnt) {
  __shared__ double s_sum[MF_THREADS];
  __shared__ int s_cnt[MF_THREADS];
  const int tid = threadIdx.x;
  const int64_t a0 = (int64_t)blockIdx.x * MF_SLICE + tid;
  for (int t = (int)blockIdx.y; t < T_m; t += (int)gridDim.y) {   // (uniform: T_m > grid.y)
    const double* __restrict__ row = PM + (int64_t)t * N;
    double p[MF_PER], q[MF_PER];
#pragma unroll
    for (int k = 0; k < MF_PER; ++k) {
      const int64_t a = a0 + (int64_t)k * MF_THREADS;
      const bool live = a < N;
      p[k] = live ? row[a] : qnan();
      q[k] = (live && t > 0) ? row[a - N] : qnan();
    }
    double s = 0.0;
    int c = 0;
#pragma unroll
    for (int k = 0; k < MF_PER; ++k) {
      const int64_t a = a0 + (int64_t)k * MF_THREADS;
      const double x = month_ret(p[k], q[k]);
      if (X && a < N) X[(int64_t)t * N + a] = x;
      const bool ok = !isnan_d(x);
      s = ok ? s + x : s;
      c += ok ? 1 : 0;
    }
    s_sum[tid] = s;
    s_cnt[tid] = c;
    __syncthreads();
    for (int h = MF_THREADS / 2; h > 0; h >>= 1) {
      if (tid < h) {
        s_sum[tid] = s_sum[tid] + s_sum[tid + h];
        s_cnt[tid] = s_cnt[tid] + s_cnt[tid + h];
      }
      __syncthreads();
    }
    if (tid == 0) {
      if (gridDim.x == 1) {
        mf_finish(s_sum[0], s_cnt[0], min_assets, t, MKT, NMK);
      } else {
        psum[(int64_t)t * gridDim.x + blockIdx.x] = s_sum[0];
        pcnt[(int64_t)t * gridDim.x + blockIdx.x] = s_cnt[0];
      }
    }
    __syncthreads();   // s_sum[0] is read before the next month's sums land
  }
}

// The slices' partial sums of month t, added in slice order from 0.0.
__global__ __launch_bounds__(64) void k_market_finish(const double* __restrict__ psum,
                                                      const int32_t* __restrict__ pcnt, int T_m,
                                                      int slices, int min_assets,
                                                      double* __restrict__ MKT,
                                                      int32_t* __restrict__ NMK) {
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= T_m) return;
  double s = 0.0;
  int c = 0;
  for (int i = 0; i < slices; ++i) {
    s += psum[(int64_t)t * slices + i];
    c += pcnt[(int64_t)t * slices + i];
  }
  mf_finish(s, c, min_assets, t, MKT, NMK);
}

// ---------------------------------------------------------------------------- B3..B5
struct MmOut {
  double* BETA;
  double* ALPHA;
  double* IVOL;
  double* RESMOM;
  int32_t* NOBS;
};

// f(x, fac) for cnt entries of the lane's x column and the shared factor ring from slot idx on
// (wrapping at W), oldest first: MM_BATCH reads of each in flight, then their f in order.
template <class Fn>
__device__ __forceinline__ void mm_walk(const double* rx, const double* fr, int W, int idx, int cnt,
                                        Fn f) {
  int k = 0;
  for (; k + MM_BATCH <= cnt; k += MM_BATCH) {
    double x[MM_BATCH], g[MM_BATCH];
#pragma unroll
    for (int u = 0; u < MM_BATCH; ++u) {
      x[u] = rx[idx * MM_THREADS];
      g[u] = fr[idx];
      idx = (idx + 1 == W) ? 0 : idx + 1;
    }
#pragma unroll
    for (int u = 0; u < MM_BATCH; ++u) f(x[u], g[u]);
  }
  for (; k < cnt; ++k) {
    f(rx[idx * MM_THREADS], fr[idx]);
    idx = (idx + 1 == W) ? 0 : idx + 1;
  }
}

// LDS (dynamic): the x ring [Wb][MM_THREADS] doubles, a lane's column, so a wave's accesses hit
// every bank once; then the factor ring [Wb], read by every lane at one address (a broadcast).
static inline size_t mm_lds_bytes(int Wb) {
  return ((size_t)Wb * MM_THREADS + (size_t)Wb) * sizeof(double);
}

__global__ __launch_bounds__(MM_THREADS) void k_market_model(
    const double* __restrict__ PM, const double* __restrict__ F, int T_m, int64_t N, int Wb, int J,
    int skip, int min_obs, int G, MmOut o) {
  extern __shared__ __attribute__((aligned(16))) double mm_lds[];
  const int tid = threadIdx.x;
  const int64_t a = (int64_t)blockIdx.x * MM_THREADS + tid;
  if (a >= N) return;   // (no barrier: a lane reads what it wrote itself)
  double* rx = mm_lds + tid;
  double* fr = mm_lds + Wb * MM_THREADS;
  const double NaN = qnan();
  int m0, m1;
  chunk_range(T_m, G, (int)blockIdx.y, m0, m1);   // G <= T_m: at least one month
  // the chunk starts cold: the first window it needs begins at j0, whose x needs month j0 - 1
  const int j0 = m0 - Wb + 1 > 0 ? m0 - Wb + 1 : 0;
  double prev = j0 > 0 ? PM[(int64_t)(j0 - 1) * N + a] : NaN;
  double cur = PM[(int64_t)j0 * N + a];
  double fcur = F[j0];
  int head = 0;   // the rings' next slot = their oldest entry once they are full
  const int kf = Wb - skip - J;   // the formation months' first position in the window (RESMOM)
  for (int j = j0; j < m1; ++j) {
    double nxt = cur, fnxt = fcur;
    if (j + 1 < m1) {
      nxt = PM[(int64_t)(j + 1) * N + a];
      fnxt = F[j + 1];
    }
    // an observation needs x and f: a month without f is stored as a month without x, so the
    // walks test one value
    rx[head * MM_THREADS] = isnan_d(fcur) ? NaN : month_ret(cur, prev);
    fr[head] = fcur;   // every lane stores the same value
    head = (head + 1 == Wb) ? 0 : head + 1;
    if (j >= m0) {
      double beta = NaN, alpha = NaN, ivol = NaN, resmom = NaN;
      int n = 0;
      if (j - Wb + 1 >= 0) {   // (uniform) a whole window: both rings are full
        // B3, pass 1
        double sx = 0.0, sf = 0.0;
        mm_walk(rx, fr, Wb, head, Wb, [&](double x, double f) {
          const bool ok = !isnan_d(x);
          sx = ok ? sx + x : sx;
          sf = ok ? sf + f : sf;
          n += ok ? 1 : 0;
        });
        const double mx = sx / (double)n, mf = sf / (double)n;
        // pass 2
        double sff = 0.0, sfx = 0.0;
        mm_walk(rx, fr, Wb, head, Wb, [&](double x, double f) {
          const bool ok = !isnan_d(x);
          const double df = f - mf, dx = x - mx;
          sff = ok ? sff + df * df : sff;
          sfx = ok ? sfx + df * dx : sfx;
        });
        const bool def = n >= min_obs && sff > 0.0;
        if (def) {
          beta = sfx / sff;
          alpha = mx - beta * mf;
        }
        // B4: the residuals on month j's own coefficients
        if (o.IVOL && def && n >= 3) {
          double se2 = 0.0;
          mm_walk(rx, fr, Wb, head, Wb, [&](double x, double f) {
            const bool ok = !isnan_d(x);
            const double e = x - (alpha + beta * f);
            se2 = ok ? se2 + e * e : se2;
          });
          ivol = sqrt(se2 / ((double)n - 2.0));
        }
        // B5: the residuals again over the J formation months
        if (o.RESMOM && def) {
          int h = head + kf;
          h = h >= Wb ? h - Wb : h;
          bool all = true;
          double se = 0.0;
          mm_walk(rx, fr, Wb, h, J, [&](double x, double f) {
            all = all && !isnan_d(x);
            se += x - (alpha + beta * f);
          });
          if (all) {
            const double me = se / (double)J;
            double sv = 0.0;
            mm_walk(rx, fr, Wb, h, J, [&](double x, double f) {
              const double d = (x - (alpha + beta * f)) - me;
              sv += d * d;
            });
            if (sv > 0.0) resmom = se / sqrt(sv / (double)(J - 1));
          }
        }
      }
      const int64_t oo = (int64_t)j * N + a;
      if (o.BETA) o.BETA[oo] = beta;
      if (o.ALPHA) o.ALPHA[oo] = alpha;
      if (o.IVOL) o.IVOL[oo] = ivol;
      if (o.RESMOM) o.RESMOM[oo] = resmom;
      if (o.NOBS) o.NOBS[oo] = n;
    }
    prev = cur;
    cur = nxt;
    fcur = fnxt;
  }
}

// ---------------------------------------------------------------------------- MF1..MF5
struct FmOut {
  double* BETA;   // [KF][T_m][N]
  double* ALPHA;
  double* IVOL;
  double* RESMOM;
  double* R2;
  int32_t* NOBS;
};

// mm_walk on KF factors: f(x, fac[KF]) for cnt entries of the lane's x column and the shared
// factor ring [W][KF] from slot idx on (wrapping at W), oldest first, MM_BATCH reads in flight.
template <int KF, class Fn>
__device__ __forceinline__ void fm_walk(const double* rx, const double* fr, int W, int idx, int cnt,
                                        Fn f) {
  int k = 0;
  for (; k + MM_BATCH <= cnt; k += MM_BATCH) {
    double x[MM_BATCH], g[MM_BATCH][KF];
#pragma unroll
    for (int u = 0; u < MM_BATCH; ++u) {
      x[u] = rx[idx * MM_THREADS];
#pragma unroll
      for (int c = 0; c < KF; ++c) g[u][c] = fr[idx * KF + c];
      idx = (idx + 1 == W) ? 0 : idx + 1;
    }
#pragma unroll
    for (int u = 0; u < MM_BATCH; ++u) f(x[u], g[u]);
  }
  for (; k < cnt; ++k) {
    double g[KF];
#pragma unroll
    for (int c = 0; c < KF; ++c) g[c] = fr[idx * KF + c];
    f(rx[idx * MM_THREADS], g);
    idx = (idx + 1 == W) ? 0 : idx + 1;
  }
}

// LDS (dynamic): the x ring [Wb][MM_THREADS], then the factor ring [Wb][KF] every lane reads at
// one address; at most 60 * (64 + 4) * 8 = 32,640 B.
static inline size_t fm_lds_bytes(int Wb, int KF) {
  return ((size_t)Wb * MM_THREADS + (size_t)Wb * KF) * sizeof(double);
}

template <int KF>
__global__ __launch_bounds__(MM_THREADS) void k_factor_model(
    const double* __restrict__ PM, const double* __restrict__ F, int T_m, int64_t N, int Wb, int J,
    int skip, int min_obs, int G, FmOut o) {
  constexpr int NP = fs_pairs(KF);
  extern __shared__ __attribute__((aligned(16))) double mm_lds[];
  const int tid = threadIdx.x;
  const int64_t a = (int64_t)blockIdx.x * MM_THREADS + tid;
  if (a >= N) return;   // (no barrier: a lane reads what it wrote itself)
  double* rx = mm_lds + tid;
  double* fr = mm_lds + Wb * MM_THREADS;
  const double NaN = qnan();
  int m0, m1;
  chunk_range(T_m, G, (int)blockIdx.y, m0, m1);   // G <= T_m: at least one month
  const int j0 = m0 - Wb + 1 > 0 ? m0 - Wb + 1 : 0;   // the chunk starts cold, as k_market_model's
  double prev = j0 > 0 ? PM[(int64_t)(j0 - 1) * N + a] : NaN;
  double cur = PM[(int64_t)j0 * N + a];
  double fcur[KF], fnxt[KF];
#pragma unroll
  for (int c = 0; c < KF; ++c) fcur[c] = F[(int64_t)j0 * KF + c];
  int head = 0;
  const int kf = Wb - skip - J;   // the formation months' first position in the window (RESMOM)
  const int64_t plane = (int64_t)T_m * N;
  for (int j = j0; j < m1; ++j) {
    double nxt = cur;
#pragma unroll
    for (int c = 0; c < KF; ++c) fnxt[c] = fcur[c];
    if (j + 1 < m1) {
      nxt = PM[(int64_t)(j + 1) * N + a];
#pragma unroll
      for (int c = 0; c < KF; ++c) fnxt[c] = F[(int64_t)(j + 1) * KF + c];
    }
    // MF1: a month with a NaN in any factor column has no factor row, and is stored as a month
    // without x, so the walks test one value
    bool frow = true;
#pragma unroll
    for (int c = 0; c < KF; ++c) frow = frow && !isnan_d(fcur[c]);
    rx[head * MM_THREADS] = frow ? month_ret(cur, prev) : NaN;
#pragma unroll
    for (int c = 0; c < KF; ++c) fr[head * KF + c] = fcur[c];   // every lane: the same values
    head = (head + 1 == Wb) ? 0 : head + 1;
    if (j >= m0) {
      double beta[KF], alpha = NaN, ivol = NaN, resmom = NaN, r2 = NaN;
#pragma unroll
      for (int c = 0; c < KF; ++c) beta[c] = NaN;
      int n = 0;
      if (j - Wb + 1 >= 0) {   // (uniform) a whole window: both rings are full
        // MF2, pass 1
        double sx = 0.0, sf[KF];
#pragma unroll
        for (int c = 0; c < KF; ++c) sf[c] = 0.0;
        fm_walk<KF>(rx, fr, Wb, head, Wb, [&](double x, const double (&f)[KF]) {
          const bool ok = !isnan_d(x);
          sx = ok ? sx + x : sx;
#pragma unroll
          for (int c = 0; c < KF; ++c) sf[c] = ok ? sf[c] + f[c] : sf[c];
          n += ok ? 1 : 0;
        });
        const double mx = sx / (double)n;
        double mf[KF];
#pragma unroll
        for (int c = 0; c < KF; ++c) mf[c] = sf[c] / (double)n;
        // pass 2
        double A[NP], b[KF], cxx = 0.0;
#pragma unroll
        for (int p = 0; p < NP; ++p) A[p] = 0.0;
#pragma unroll
        for (int c = 0; c < KF; ++c) b[c] = 0.0;
        fm_walk<KF>(rx, fr, Wb, head, Wb, [&](double x, const double (&f)[KF]) {
          const bool ok = !isnan_d(x);
          const double dx = x - mx;
          double d[KF];
#pragma unroll
          for (int c = 0; c < KF; ++c) d[c] = f[c] - mf[c];
#pragma unroll
          for (int c = 0; c < KF; ++c) {
#pragma unroll
            for (int e = c; e < KF; ++e) {
              const int p = fs_pair(KF, c, e);
              A[p] = ok ? A[p] + d[c] * d[e] : A[p];
            }
            b[c] = ok ? b[c] + d[c] * dx : b[c];
          }
          cxx = ok ? cxx + dx * dx : cxx;
        });
        // MF3, MF4
        double g[KF];
        const bool solved = fs_solve<KF>(A, b, g);
        const bool def = n >= min_obs && solved;
        if (def) {
          alpha = mx;
#pragma unroll
          for (int c = 0; c < KF; ++c) {
            beta[c] = g[c];
            alpha = alpha - g[c] * mf[c];
          }
        }
        auto resid = [&](double x, const double (&f)[KF]) {
          double fit = alpha;
#pragma unroll
          for (int c = 0; c < KF; ++c) fit = fit + beta[c] * f[c];
          return x - fit;
        };
        // MF5: the residuals on month j's own coefficients
        if ((o.IVOL || o.R2) && def && (n >= KF + 2 || cxx > 0.0)) {
          double se2 = 0.0;
          fm_walk<KF>(rx, fr, Wb, head, Wb, [&](double x, const double (&f)[KF]) {
            const bool ok = !isnan_d(x);
            const double e = resid(x, f);
            se2 = ok ? se2 + e * e : se2;
          });
          if (n >= KF + 2) ivol = sqrt(se2 / ((double)n - (KF + 1.0)));
          if (cxx > 0.0) r2 = 1.0 - se2 / cxx;
        }
        // the residuals again over the J formation months (B5's words)
        if (o.RESMOM && def) {
          int h = head + kf;
          h = h >= Wb ? h - Wb : h;
          bool all = true;
          double se = 0.0;
          fm_walk<KF>(rx, fr, Wb, h, J, [&](double x, const double (&f)[KF]) {
            all = all && !isnan_d(x);
            se += resid(x, f);
          });
          if (all) {
            const double me = se / (double)J;
            double sv = 0.0;
            fm_walk<KF>(rx, fr, Wb, h, J, [&](double x, const double (&f)[KF]) {
              const double d = resid(x, f) - me;
              sv += d * d;
            });
            if (sv > 0.0) resmom = se / sqrt(sv / (double)(J - 1));
          }
        }
      }
      const int64_t oo = (int64_t)j * N + a;
      if (o.BETA) {
#pragma unroll
        for (int c = 0; c < KF; ++c) o.BETA[c * plane + oo] = beta[c];
      }
      if (o.ALPHA) o.ALPHA[oo] = alpha;
      if (o.IVOL) o.IVOL[oo] = ivol;
      if (o.RESMOM) o.RESMOM[oo] = resmom;
      if (o.R2) o.R2[oo] = r2;
      if (o.NOBS) o.NOBS[oo] = n;
    }
    prev = cur;
    cur = nxt;
#pragma unroll
    for (int c = 0; c < KF; ++c) fcur[c] = fnxt[c];
  }
}

template <int KF>
static inline void fm_launch(csm_ctx* ctx, dim3 grid, const double* PM, const double* F, int T_m,
                             int64_t N, int Wb, int J, int skip, int min_obs, int G,
                             const FmOut& o) {
  hipLaunchKernelGGL(k_factor_model<KF>, grid, dim3(MM_THREADS), fm_lds_bytes(Wb, KF),
                     ctx->stream, PM, F, T_m, N, Wb, J, skip, min_obs, G, o);
}

// --------------------------------------------------------------------------------- B6
__device__ __forceinline__ void nx_load(double (&x)[NX_TRIP], double (&s)[NX_TRIP],
                                        const double* __restrict__ PM,
                                        const double* __restrict__ S, int64_t N, int64_t a, int t,
                                        int T_m) {
#pragma unroll
  for (int i = 0; i < NX_TRIP; ++i) {
    const bool in = t + i < T_m;
    x[i] = in ? PM[(int64_t)(t + i) * N + a] : absent_val();
    s[i] = in ? S[(int64_t)(t + i) * N + a] : qnan();
  }
}

__global__ __launch_bounds__(NX_THREADS) void k_next_ret(const double* __restrict__ PM,
                                                         const double* __restrict__ S, int T_m,
                                                         int64_t N, double* __restrict__ NR) {
  const int64_t a = (int64_t)blockIdx.x * NX_THREADS + threadIdx.x;
  if (a >= N) return;
  double psff = qnan();
  int prev = -1;
  double x[NX_TRIP], s[NX_TRIP], xn[NX_TRIP], sn[NX_TRIP];
  nx_load(x, s, PM, S, N, a, 0, T_m);
  for (int t = 0; t < T_m; t += NX_TRIP) {
    nx_load(xn, sn, PM, S, N, a, t + NX_TRIP, T_m);
#pragma unroll
    for (int i = 0; i < NX_TRIP; ++i) {
      if (t + i >= T_m) break;
      const int64_t o = (int64_t)(t + i) * N + a;
      if (is_absent(x[i])) {   // no step at all
        NR[o] = qnan();
      } else if (rank_step(x[i], s[i], t + i, psff, prev,
                           [&](int row, double nr) { NR[(int64_t)row * N + a] = nr; })) {
        NR[o] = qnan();
      }
    }
#pragma unroll
    for (int i = 0; i < NX_TRIP; ++i) {
      x[i] = xn[i];
      s[i] = sn[i];
    }
  }
  // whole panels only: no later month settles the pending row
  if (prev >= 0) NR[(int64_t)prev * N + a] = pending_finish(absent_val(), psff);
}

extern "C" {

int csm_tune_market(const char* key, int value) { return tune_set(g_knobs, key, value); }

int csm_market_factor(csm_ctx* ctx, const double* PM, int32_t T_m, int64_t N, int32_t min_assets,
                      double* X, double* MKT, int32_t* NMK) {
  int r = prep(ctx);
  if (r) return r;
  if (!PM || !MKT || bad_panel(T_m, N))
    return set_err(ctx, CSM_E_INVAL, "csm_market_factor: bad arguments (T_m=%d N=%lld)", T_m,
                   (long long)N);
  if (min_assets < 1)
    return set_err(ctx, CSM_E_INVAL, "csm_market_factor: min_assets=%d must be at least 1",
                   min_assets);
  const int64_t slices = (N + MF_SLICE - 1) / MF_SLICE;
  double* psum = nullptr;
  int32_t* pcnt = nullptr;
  if (slices > 1) {
    const size_t cells = (size_t)T_m * (size_t)slices;
    r = ctx_reserve(ctx, "csm_market_factor", "the partial-sum workspace", &ctx->mkt_ws,
                    &ctx->mkt_ws_bytes, cells * (sizeof(double) + sizeof(int32_t)));
    if (r) return r;
    psum = (double*)ctx->mkt_ws;
    pcnt = (int32_t*)(psum + cells);
  }
  const dim3 grid((unsigned)slices, (unsigned)(T_m < 65535 ? T_m : 65535));
  hipLaunchKernelGGL(k_market_factor, grid, dim3(MF_THREADS), 0, ctx->stream, PM, T_m, N,
                     min_assets, X, MKT, NMK, psum, pcnt);
  LAUNCH_CHECK(ctx, "k_market_factor");
  if (slices > 1) {
    hipLaunchKernelGGL(k_market_finish, dim3((unsigned)((T_m + 63) / 64)), dim3(64), 0,
                       ctx->stream, psum, pcnt, T_m, (int)slices, min_assets, MKT, NMK);
    LAUNCH_CHECK(ctx, "k_market_finish");
  }
  return CSM_OK;
}

int csm_market_model(csm_ctx* ctx, const double* PM, const double* F, int32_t T_m, int64_t N,
                     int32_t Wb, int32_t J, int32_t skip, int32_t min_obs, double* BETA,
                     double* ALPHA, double* IVOL, double* RESMOM, int32_t* NOBS) {
  int r = prep(ctx);
  if (r) return r;
  if (!PM || !F || bad_panel(T_m, N))
    return set_err(ctx, CSM_E_INVAL, "csm_market_model: bad arguments (T_m=%d N=%lld)", T_m,
                   (long long)N);
  if (!BETA && !ALPHA && !IVOL && !RESMOM && !NOBS)
    return set_err(ctx, CSM_E_INVAL, "csm_market_model: no output requested");
  if (Wb < 2 || Wb > MM_MAXW)
    return set_err(ctx, CSM_E_INVAL, "csm_market_model: Wb=%d is outside [2, %d]", Wb, MM_MAXW);
  if (min_obs < 2 || min_obs > Wb)
    return set_err(ctx, CSM_E_INVAL, "csm_market_model: min_obs=%d is outside [2, Wb=%d]",
                   min_obs, Wb);
  if (RESMOM && (J < 2 || skip < 0 || (int64_t)J + skip > Wb))
    return set_err(ctx, CSM_E_INVAL,
                   "csm_market_model: RESMOM needs J >= 2, skip >= 0 and J + skip <= Wb "
                   "(J=%d skip=%d Wb=%d)", J, skip, Wb);
  if (!RESMOM) {   // not read
    J = 2;
    skip = 0;
  }
  // Auto chunk count: about 64 workgroups per CU (scan.h auto_chunks).  The kernel is bound by
  // fp64 VALU issue (five walks of the window per asset-month), not by bytes, and a workgroup's
  // ring (18 KiB at Wb = 36) leaves a CU eight of them, so what the chunks buy is an even fill and
  // a short tail; past that, the Wb - 1 months a chunk warms up on cost more than they return.
  // MI355X, Wb = 36, all outputs, before a month without f was stored as a month without x
  // (profiles/r11/bench_market_*_sweep.log; after it, 3.23 and 0.168 ms at the auto counts of 11
  // and 100, bench_market_*.log): 100,000 assets x 461 months 1 / 2 / 12 / 46 / 461 chunks 4.62 /
  // 4.13 / 3.17 / 3.14 / 6.27 ms; 5,000 assets x 300 months 1 / 8 / 30 / 100 / 300 chunks 1.76 /
  // 0.308 / 0.185 / 0.167 / 0.212 ms
  const dim3 grid = month_grid(ctx, N, MM_THREADS, g_tune_mm_chunks, 64, T_m);
  const MmOut o{BETA, ALPHA, IVOL, RESMOM, NOBS};
  hipLaunchKernelGGL(k_market_model, grid, dim3(MM_THREADS), mm_lds_bytes(Wb), ctx->stream, PM, F,
                     T_m, N, Wb, J, skip, min_obs, (int)grid.y, o);
  LAUNCH_CHECK(ctx, "k_market_model");
  return CSM_OK;
}

int csm_factor_model(csm_ctx* ctx, const double* PM, const double* F, int32_t T_m, int64_t N,
                     int32_t KF, int32_t Wb, int32_t J, int32_t skip, int32_t min_obs,
                     double* BETA, double* ALPHA, double* IVOL, double* RESMOM, double* R2,
                     int32_t* NOBS) {
  int r = prep(ctx);
  if (r) return r;
  if (!PM || !F || bad_panel(T_m, N))
    return set_err(ctx, CSM_E_INVAL, "csm_factor_model: bad arguments (T_m=%d N=%lld)", T_m,
                   (long long)N);
  if (KF < 1 || KF > FS_MAXKF)
    return set_err(ctx, CSM_E_INVAL, "csm_factor_model: KF=%d is outside [1, %d]", KF, FS_MAXKF);
  if ((int64_t)T_m * KF > ((int64_t)1 << 40) / N)
    return set_err(ctx, CSM_E_INVAL, "csm_factor_model: bad arguments (T_m=%d N=%lld KF=%d)", T_m,
                   (long long)N, KF);
  if (!BETA && !ALPHA && !IVOL && !RESMOM && !R2 && !NOBS)
    return set_err(ctx, CSM_E_INVAL, "csm_factor_model: no output requested");
  if (Wb < KF + 1 || Wb > MM_MAXW)
    return set_err(ctx, CSM_E_INVAL, "csm_factor_model: Wb=%d is outside [KF+1=%d, %d]", Wb,
                   KF + 1, MM_MAXW);
  if (min_obs < KF + 1 || min_obs > Wb)
    return set_err(ctx, CSM_E_INVAL, "csm_factor_model: min_obs=%d is outside [KF+1=%d, Wb=%d]",
                   min_obs, KF + 1, Wb);
  if (RESMOM && (J < 2 || skip < 0 || (int64_t)J + skip > Wb))
    return set_err(ctx, CSM_E_INVAL,
                   "csm_factor_model: RESMOM needs J >= 2, skip >= 0 and J + skip <= Wb "
                   "(J=%d skip=%d Wb=%d)", J, skip, Wb);
  if (!RESMOM) {   // not read
    J = 2;
    skip = 0;
  }
  // Auto chunk count: k_market_model's.  The kernel has its shape, warm-up cost and LDS footprint
  // (plus Wb * KF doubles), and the sweep has its shape too.  MI355X, Wb = 36, all outputs, KF = 1 /
  // KF = 4 (profiles/r15/bench_factor_sweep.log): 100,000 assets x 461 months 2 / 11 (auto) / 12 /
  // 46 / 150 chunks 4.52 / 3.51 / 3.55 / 3.43 / 4.10 ms and 10.60 / 7.80 / 8.03 / 7.49 / 8.16 ms;
  // 5,000 assets x 300 months 2 / 12 / 46 / 100 (auto) / 150 chunks 1.100 / 0.240 / 0.179 /
  // 0.177 / 0.187 ms and 2.023 / 0.483 / 0.373 / 0.349 / 0.356 ms
  const dim3 grid = month_grid(ctx, N, MM_THREADS, g_tune_fm_chunks, 64, T_m);
  const int G = (int)grid.y;
  const FmOut o{BETA, ALPHA, IVOL, RESMOM, R2, NOBS};
  switch (KF) {
    case 1: fm_launch<1>(ctx, grid, PM, F, T_m, N, Wb, J, skip, min_obs, G, o); break;
    case 2: fm_launch<2>(ctx, grid, PM, F, T_m, N, Wb, J, skip, min_obs, G, o); break;
    case 3: fm_launch<3>(ctx, grid, PM, F, T_m, N, Wb, J, skip, min_obs, G, o); break;
    default: fm_launch<4>(ctx, grid, PM, F, T_m, N, Wb, J, skip, min_obs, G, o); break;
  }
  LAUNCH_CHECK(ctx, "k_factor_model");
  return CSM_OK;
}

int csm_next_ret(csm_ctx* ctx, const double* PM, const double* S, int32_t T_m, int64_t N,
                 double* NR) {
  int r = prep(ctx);
  if (r) return r;
  if (!PM || !S || !NR || bad_panel(T_m, N))
    return set_err(ctx, CSM_E_INVAL, "csm_next_ret: bad arguments (T_m=%d N=%lld)", T_m,
                   (long long)N);
  hipLaunchKernelGGL(k_next_ret, dim3((unsigned)((N + NX_THREADS - 1) / NX_THREADS)),
                     dim3(NX_THREADS), 0, ctx->stream, PM, S, T_m, N, NR);
  LAUNCH_CHECK(ctx, "k_next_ret");
  return CSM_OK;
}

}  // extern "C"
