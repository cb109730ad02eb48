// breakpoints.hip -- reference-universe breakpoints and universe screens (rules U1..U6 in
// DESIGN.md 7): qcut edges taken from a subset of each date's cells (NYSE-style breakpoints),
// every ranked cell of the date labelled against them, the decile means of those labels; and the
// price / size screen that NaNs cells out of a signal panel.
//
//   U1  the ranked set of date t: the cells whose M[t][a] is not NaN (the ABSENT payload is a
//       NaN).  The breakpoint set: the ranked cells with BP[t * bp_ld + a] != 0 (uint8; bp_ld = N
//       one row per month, bp_ld = 0 one static row; every byte value is data).
//   U2  edges: rule S5 on the breakpoint set's values (the caller's qtable, the fp64 lerp without
//       FMA), the distinct ones in order -- EDGES[t] = the NE[t] distinct edges, NaN up to
//       n_bins + 1; NVB[t] the size of the breakpoint set.  -0.0 and 0.0 are equal.
//   U3  NE[t] < 2 (an empty, one-value or all-equal subset): every label of the date is -1.
//       Otherwise a ranked cell's label is #{k in 1..NE-2 : e_k < x}, in [0, NE - 2]: cells below
//       e_0 fall in bin 0, cells above the last edge in bin NE - 2.  Non-ranked cells get -1.
//   U4  with NR: EW[t][d] the mean of NR over the cells with label d and a non-NaN NR, CNT their
//       count, NV[t] the ranked cells.  The sum's order: lane l of 1024 adds its cells l,
//       l + 1024, ... in ascending order from 0.0, each of the 16 waves adds its lanes by the
//       halving tree (h = 32..1: element j < h += element j + h), the wave sums are added in wave
//       order from 0.0 -- a function of N alone.  No floating-point atomic: two calls give the
//       same bits.
//   U5  the screen: a cell of M is kept iff M is not NaN, PM is NULL or PM >= min_price (a NaN or
//       ABSENT PM fails), and CAP is NULL or CAP >= CAPMIN[t] (a NaN on either side fails);
//       MS = M where kept, NaN elsewhere; KEPT[t] the kept cells.
//   U6  NR is the caller's (rule N6); the screen never changes it.
//
//   k_bppart   U1.  One workgroup per date, each wave one contiguous chunk of the row: the
//              breakpoint set's values, in asset order, to the packed row SK; NVB[t] (gsort.h's
//              pack_row).
//   k_bpedges  U2.  One workgroup per date sorts the NVB[t] packed keys only -- gsort.h's
//              sort_segment, as k_gdec: in LDS up to the "gdec_small_cap" knob's keys (4,096),
//              tiled past that; only keys are sorted, so the edges do not depend on the knob --
//              and takes the n_bins + 1 order statistics with their upper neighbours from the
//              sorted keys.  The distinct edges are kept in order, NaN after them: this
//              kernel's own rule, not k_gdec's duplicates='drop'.
//   k_bplabel  U3, U4.  One workgroup per date: one sweep of the whole row against the at most 19
//              interior edges (LDS), fused with the decile sums (per-lane registers per label).
//   k_screen   U5.  One workgroup per date, elementwise, the row's count by an integer block_sum.
#include "gsort.h"

#define BP_THREADS 1024
#define BP_WAVES (BP_THREADS / 64)
#define BP_U 4   // steps of BP_THREADS cells whose loads a lane issues together

// ------------------------------------------------------------------------------------ U1
__global__ __launch_bounds__(BP_THREADS) void k_bppart(const double* __restrict__ M,
                                                       const uint8_t* __restrict__ BP,
                                                       int64_t bp_ld, int64_t N,
                                                       double* __restrict__ SK,
                                                       int32_t* __restrict__ NVB) {
  __shared__ int s_cnt[BP_WAVES];
  const int t = blockIdx.x;
  const double* __restrict__ row = M + (int64_t)t * N;
  const uint8_t* __restrict__ bp = BP + (int64_t)t * bp_ld;
  double* __restrict__ sk = SK + (int64_t)t * N;
  double x;   // the cell's value, from the predicate to the emit
  const int tot = pack_row<BP_THREADS>(
      N, s_cnt,
      [&](int64_t i) {
        x = row[i];
        return x == x && bp[i] != 0;
      },
      [&](int64_t, int pos) { sk[pos] = x; });
  if (threadIdx.x == 0) NVB[t] = tot;
}

// ------------------------------------------------------------------------------------ U2
template <bool SMALL>
__global__ __launch_bounds__(SMALL ? GD_SMALL_THREADS : GD_LONG_THREADS) void k_bpedges(
    int64_t N, int n_bins, QTab qt, int cap, int tile, const int32_t* __restrict__ NVB, double* SK,
    double* __restrict__ EDGES, int32_t* __restrict__ NE) {
  constexpr int NT = SMALL ? GD_SMALL_THREADS : GD_LONG_THREADS;
  __shared__ double s_key[GD_TILE];
  __shared__ double s_edge[MAXQ];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int n = NVB[t];
  if (not_mine<SMALL>(n, cap)) return;
  if (n > 0) {
    const double* srt = sort_segment<SMALL, NT>(SK + (int64_t)t * N, s_key, n, tile);
    if (tid <= n_bins) s_edge[tid] = qcut_edge(srt, n, qt.q[tid]);
  }
  __syncthreads();
  if (tid == 0) {   // the distinct edges in order, NaN after them
    double* e = EDGES + (int64_t)t * (n_bins + 1);
    int nu = 0;
    if (n > 0)
      for (int k = 0; k <= n_bins; ++k) {
        const double v = s_edge[k];
        bool seen = false;
        for (int j = 0; j < nu; ++j) seen |= e[j] == v;
        if (!seen) e[nu++] = v;
      }
    for (int k = nu; k <= n_bins; ++k) e[k] = qnan();
    NE[t] = nu;
  }
}

// -------------------------------------------------------------------------------- U3, U4
template <int NB>
__global__ __launch_bounds__(BP_THREADS) void k_bplabel(
    const double* __restrict__ M, const double* __restrict__ NR, int64_t N, int n_bins,
    const double* __restrict__ EDGES, const int32_t* __restrict__ NE, int8_t* __restrict__ L,
    double* __restrict__ EW, int32_t* __restrict__ CNT, int32_t* __restrict__ NV) {
  constexpr int NBS = NB > 0 ? NB : 1;
  __shared__ double s_e[MAXQ];
  __shared__ double s_sum[BP_WAVES][NBS];
  __shared__ int s_c[BP_WAVES][NBS + 1];   // the labels' counts, then the ranked cells
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ne = NE[t];
  if (tid <= n_bins) s_e[tid] = EDGES[(int64_t)t * (n_bins + 1) + tid];
  __syncthreads();
  const int hi = ne - 2;   // interior edges s_e[1..hi]; ne < 2: no label at all
  const double* __restrict__ row = M + (int64_t)t * N;
  const double* __restrict__ nr = NB > 0 ? NR + (int64_t)t * N : nullptr;
  int8_t* __restrict__ lrow = L ? L + (int64_t)t * N : nullptr;
  double s[NBS];
  int c[NBS], nv = 0;
#pragma unroll
  for (int d = 0; d < NBS; ++d) {
    s[d] = 0.0;
    c[d] = 0;
  }
  for (int64_t b = 0; b < N; b += (int64_t)BP_THREADS * BP_U) {
    double xv[BP_U], rv[BP_U];
#pragma unroll
    for (int u = 0; u < BP_U; ++u) {
      const int64_t i = b + (int64_t)u * BP_THREADS + tid;
      xv[u] = i < N ? row[i] : qnan();
      rv[u] = (NB > 0 && i < N) ? nr[i] : qnan();
    }
#pragma unroll
    for (int u = 0; u < BP_U; ++u) {
      const int64_t i = b + (int64_t)u * BP_THREADS + tid;
      const double x = xv[u];
      const bool ranked = x == x;
      int lab = -1;
      if (ranked && ne >= 2) {
        lab = 0;
        for (int k = 1; k <= hi; ++k) lab += (s_e[k] < x) ? 1 : 0;
      }
      nv += ranked ? 1 : 0;
      if (lrow && i < N) lrow[i] = (int8_t)lab;
      if (NB > 0) {
        const double r = rv[u];
        const bool ok = lab >= 0 && r == r;
#pragma unroll
        for (int d = 0; d < NBS; ++d) {
          const bool h = ok && lab == d;
          s[d] = s[d] + (h ? r : 0.0);
          c[d] += h ? 1 : 0;
        }
      }
    }
  }
  if (NB > 0) {
#pragma unroll
    for (int d = 0; d < NBS; ++d) {
      const double sd = wave_tree(s[d]);
      const int cd = wave_tree(c[d]);
      if (lane == 0) {
        s_sum[wave][d] = sd;
        s_c[wave][d] = cd;
      }
    }
  }
  nv = wave_tree(nv);
  if (lane == 0) s_c[wave][NBS] = nv;
  __syncthreads();
  if (NB > 0 && tid < NB) {
    double a = 0.0;
    int k = 0;
    for (int w = 0; w < BP_WAVES; ++w) {
      a = a + s_sum[w][tid];
      k += s_c[w][tid];
    }
    if (EW) EW[(int64_t)t * NB + tid] = k > 0 ? a / (double)k : qnan();
    if (CNT) CNT[(int64_t)t * NB + tid] = k;
  }
  if (NV && tid == 0) {
    int k = 0;
    for (int w = 0; w < BP_WAVES; ++w) k += s_c[w][NBS];
    NV[t] = k;
  }
}

// ------------------------------------------------------------------------------------ U5
__global__ __launch_bounds__(BP_THREADS) void k_screen(
    const double* __restrict__ M, const double* __restrict__ PM, double min_price,
    const double* __restrict__ CAP, const double* __restrict__ CAPMIN, int64_t N,
    double* __restrict__ MS, int32_t* __restrict__ KEPT) {
  __shared__ int s_k[BP_WAVES];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int64_t o = (int64_t)t * N;
  const double cmin = CAP ? CAPMIN[t] : 0.0;
  int kept = 0;
  for (int64_t b = 0; b < N; b += (int64_t)BP_THREADS * BP_U) {
    double xv[BP_U], pv[BP_U], cv[BP_U];
#pragma unroll
    for (int u = 0; u < BP_U; ++u) {
      const int64_t i = b + (int64_t)u * BP_THREADS + tid;
      xv[u] = i < N ? M[o + i] : qnan();
      pv[u] = (PM && i < N) ? PM[o + i] : min_price;
      cv[u] = (CAP && i < N) ? CAP[o + i] : cmin;
    }
#pragma unroll
    for (int u = 0; u < BP_U; ++u) {
      const int64_t i = b + (int64_t)u * BP_THREADS + tid;
      const double x = xv[u];
      // (a NaN on either side of a comparison fails it)
      const bool keep = x == x && (!PM || pv[u] >= min_price) && (!CAP || cv[u] >= cmin);
      if (i < N) MS[o + i] = keep ? x : qnan();
      kept += (keep && i < N) ? 1 : 0;
    }
  }
  if (!KEPT) return;
  kept = block_sum<int, BP_THREADS>(kept, s_k);
  if (tid == 0) KEPT[t] = kept;
}

// ----------------------------------------------------------------------------------- host
extern "C" {

int csm_deciles_bp(csm_ctx* ctx, const double* M, const double* NR, const uint8_t* BP,
                   int64_t bp_ld, int32_t T_m, int64_t N, int32_t n_bins, const double* qtable,
                   int8_t* L, double* EW, int32_t* CNT, int32_t* NV, int32_t* NVB, double* EDGES,
                   int32_t* NE) {
  const char* who = "csm_deciles_bp";
  int r = prep(ctx);
  if (r) return r;
  if (!M || !BP || !qtable) return set_err(ctx, CSM_E_INVAL, "%s: M, BP or qtable is NULL", who);
  if (bad_panel(T_m, N, INT32_MAX))
    return set_err(ctx, CSM_E_INVAL, "%s: bad arguments (T_m=%d N=%lld)", who, T_m, (long long)N);
  if (bp_ld != 0 && bp_ld != N)
    return set_err(ctx, CSM_E_INVAL, "%s: bp_ld=%lld must be 0 (one static row) or N=%lld", who,
                   (long long)bp_ld, (long long)N);
  r = check_n_bins(ctx, who, n_bins, NR != nullptr);
  if (r) return r;
  if (!L && !EDGES) return set_err(ctx, CSM_E_INVAL, "%s: L and EDGES are both NULL", who);
  // the packed keys (8 B per cell), and the edges / counts the caller does not take
  const size_t b_sk = up16((size_t)T_m * (size_t)N * sizeof(double));
  const size_t b_e = up16((size_t)T_m * MAXQ * sizeof(double));
  const size_t b_i = up16((size_t)T_m * sizeof(int32_t));
  r = ctx_reserve(ctx, who, "the group partition workspace", &ctx->grp_ws, &ctx->grp_ws_bytes,
                  b_sk + b_e + 2 * b_i);
  if (r) return r;
  char* p = (char*)ctx->grp_ws;
  double* sk = (double*)p;
  double* edges = EDGES ? EDGES : (double*)(p + b_sk);
  int32_t* ne = NE ? NE : (int32_t*)(p + b_sk + b_e);
  int32_t* nvb = NVB ? NVB : (int32_t*)(p + b_sk + b_e + b_i);
  const QTab q = qtab_fill(qtable, n_bins);
  const SortPlan sp = sort_plan();
  const dim3 grid((unsigned)T_m);
  hipLaunchKernelGGL(k_bppart, grid, dim3(BP_THREADS), 0, ctx->stream, M, BP, bp_ld, N, sk, nvb);
  LAUNCH_CHECK(ctx, "k_bppart");
  LAUNCH_PAIR(ctx, k_bpedges, grid, N, n_bins, q, sp.cap, sp.tile, nvb, sk, edges, ne);
  if (!L && !NV && !(NR && (EW || CNT))) return CSM_OK;   // the edges alone
  nb_dispatch<0, 2, 3, 4, 5, 10, 20>(NR ? n_bins : 0, [&](auto nb) {
    hipLaunchKernelGGL(k_bplabel<decltype(nb)::value>, grid, dim3(BP_THREADS), 0, ctx->stream, M,
                       NR, N, n_bins, edges, ne, L, EW, CNT, NV);
  });
  LAUNCH_CHECK(ctx, "k_bplabel");
  return CSM_OK;
}

int csm_screen(csm_ctx* ctx, const double* M, const double* PM, double min_price,
               const double* CAP, const double* CAPMIN, int32_t T_m, int64_t N, double* MS,
               int32_t* KEPT) {
  const char* who = "csm_screen";
  int r = prep(ctx);
  if (r) return r;
  if (!M || !MS) return set_err(ctx, CSM_E_INVAL, "%s: M or MS is NULL", who);
  if (bad_panel(T_m, N, INT32_MAX))
    return set_err(ctx, CSM_E_INVAL, "%s: bad arguments (T_m=%d N=%lld)", who, T_m, (long long)N);
  if (CAP && !CAPMIN) return set_err(ctx, CSM_E_INVAL, "%s: CAP is given and CAPMIN is NULL", who);
  hipLaunchKernelGGL(k_screen, dim3((unsigned)T_m), dim3(BP_THREADS), 0, ctx->stream, M, PM,
                     min_price, CAP, CAPMIN, N, MS, KEPT);
  LAUNCH_CHECK(ctx, "k_screen");
  return CSM_OK;
}

}  // extern "C"
