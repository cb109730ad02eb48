// deciles_wide.hip -- the decile entry points and their dispatch, with the two kernels that no
// other source holds.  Reference behaviour restated (file:line into the reference):
//   deciles           run_demo.py:18-29,46    (pd.qcut(q=n, labels=False, duplicates='drop'))
//   decile means      run_demo.py:49-55       (dropna; groupby(date, decile).mean())
//   long-short        run_demo.py:57-67
//
//   k_deciles (dec_wide)   deciles.inc for wide rows read from M: a workgroup per date row.
//   k_long_short           the long-short series from the decile means and counts, one workgroup.
// deciles_dispatch picks, by row width, ids and the "dec_*" knobs, between these and the launchers
// of deciles_narrow.hip, deciles_pre.hip and deciles_npre.hip (csm_common.h).  csm_pipeline is
// here too: signal_launch (signal.hip), then this dispatch.
#include "csm_common.h"

// =====================================================================================
#define DEC_THREADS 512
#define HB 8192
#define CAP 4096
// label pass: 8 x 32 B of M / NR in flight per lane (128 VGPRs: still two 512-thread
// workgroups per CU): labels 117 -> 110 us per row at C4.  Row sweeps keep ROW_U = 8 (10 made
// the histogram pass 3 us slower; profiles/r01/experiments/dec_unroll_ab.log)
#ifndef DEC_LU
#define DEC_LU 8
#endif
namespace dec_wide {
#include "deciles.inc"
}  // namespace dec_wide
using dec_wide::k_deciles;
#undef DEC_THREADS
#undef HB
#undef CAP
#undef DEC_LU

// =====================================================================================
// Kernel E: long-short series (one workgroup; T_m * n_bins is tiny).  LS_THREADS threads: a
// thread's first month's counts and means are loaded before the leg-presence barrier and kept
// for its long-short (one round trip where T_m <= LS_THREADS, instead of a flag pass and a
// second pass over the months).
// =====================================================================================
#define LS_THREADS 512
__global__ __launch_bounds__(LS_THREADS) void k_long_short(const double* __restrict__ EW,
                                                           const int32_t* __restrict__ CNT,
                                                           int T_m, int nb,
                                                           double* __restrict__ LS) {
  __shared__ int has_lo, has_hi;
  const int t0 = threadIdx.x;
  int cv[MAXQ - 1];
  double ev[MAXQ - 1];
  auto load_row = [&](int t) {
    const double* e = EW + (int64_t)t * nb;
    const int32_t* c = CNT + (int64_t)t * nb;
#pragma unroll
    for (int d = 0; d < MAXQ - 1; ++d) {   // the row's counts and means, all loads in flight
      cv[d] = d < nb ? c[d] : 0;
      ev[d] = d < nb ? e[d] : 0.0;
    }
  };
  auto legs_of = [&](int& lo_c, int& hi_c) {   // the row's decile-0 / decile-(nb-1) counts
#pragma unroll
    for (int d = 0; d < MAXQ - 1; ++d) {
      if (d == 0) lo_c = cv[d];
      if (d == nb - 1) hi_c = cv[d];
    }
  };
  auto ls_of = [&](bool both) {
    bool any = false;
    double mx = -INFINITY, mn = INFINITY, lo = 0.0, hi = 0.0;
#pragma unroll
    for (int d = 0; d < MAXQ - 1; ++d) {
      if (cv[d] > 0) { any = true; mx = fmax(mx, ev[d]); mn = fmin(mn, ev[d]); }
      if (d == 0) lo = ev[d];
      if (d == nb - 1) hi = ev[d];
    }
    double v = qnan();
    if (any) v = both ? (hi - lo) : (mx - mn);
    return v;
  };
  if (t0 < T_m) load_row(t0);
  if (t0 == 0) { has_lo = 0; has_hi = 0; }
  __syncthreads();
  if (t0 < T_m) {
    int lc = 0, hc = 0;
    legs_of(lc, hc);
    if (lc > 0) atomicOr(&has_lo, 1);
    if (hc > 0) atomicOr(&has_hi, 1);
  }
  for (int t = t0 + LS_THREADS; t < T_m; t += LS_THREADS) {
    if (CNT[(int64_t)t * nb] > 0) atomicOr(&has_lo, 1);
    if (CNT[(int64_t)t * nb + nb - 1] > 0) atomicOr(&has_hi, 1);
  }
  __syncthreads();
  const bool both = has_lo && has_hi;
  if (t0 < T_m) LS[t0] = ls_of(both);
  for (int t = t0 + LS_THREADS; t < T_m; t += LS_THREADS) {
    load_row(t);
    LS[t] = ls_of(both);
  }
}

static int64_t* g_dec_timing = nullptr;   // csm_tune_ptr "dec_timing" (csm_common.h dec_mark)
// PRE decile pass (csm_deciles_ids): 1 the merged sweep, then the general kernel for the rows it
// leaves | 0 the general kernel only
static int g_tune_dec_merge = 1;
// wide rows on ids: 2 (auto) the split decile pass (plan, chunked sweep, finish; deciles.inc) for
// launches of fewer rows than half the CUs (short date shards), else the merged
// one-workgroup-per-row pass | 1 always split | 0 never.  Same labels and counts; decile means in
// another fixed order
static int g_tune_dec_split = 2;
static int g_tune_dec_split_cells = SPLIT_CELLS;   // cells per split-sweep chunk
// the split sweep: 0 the two-workgroups-per-CU variant (no prefetch) | 1 the prefetching one
// workgroup per CU | 2 prefetch when the launch has no more (chunk, date) pairs than CUs.
// C4 rank rehearsals, deciles_ids ms: 4-way 0.1162 / 0.1338 / 0.1165, 8-way 0.0998 / 0.1019 /
// 0.1014 (profiles/r06/experiments/split_pf)
static int g_tune_dec_split_pf = 0;
// rows with at most this many assets take the narrow-row decile kernels
static int g_tune_dec_narrow_max = 16384;
static const TuneKnob g_knobs[] = {
    {"dec_merge", &g_tune_dec_merge, [](int v) { return v == 0 || v == 1; }},
    {"dec_narrow_max", &g_tune_dec_narrow_max, [](int v) { return v >= 0; }},
    {"dec_split", &g_tune_dec_split, [](int v) { return v >= 0 && v <= 2; }},
    {"dec_split_pf", &g_tune_dec_split_pf, [](int v) { return v >= 0 && v <= 2; }},
    {"dec_split_cells", &g_tune_dec_split_cells,
     [](int v) { return v >= SPLIT_TRIP && v % SPLIT_TRIP == 0; }},
};
int csm_tune_deciles(const char* key, int value) { return tune_set(g_knobs, key, value); }
int csm_tune_ptr_deciles(const char* key, void* p) {
  if (!key || strcmp(key, "dec_timing")) return CSM_E_INVAL;
  g_dec_timing = (int64_t*)p;
  return CSM_OK;
}

// The split decile pass's workspace for T_m rows of N cells (csm_common.h DecSplit), carved
// from one context buffer; sized for n_bins up to MAXQ so one buffer serves every NB.
static size_t dsplit_layout(int32_t T_m, int64_t N, DecSplit* sp, char* base) {
  const int64_t CC = g_tune_dec_split_cells;
  const int64_t C = (N + CC - 1) / CC;
  auto al = [](size_t x) { return (x + 255) / 256 * 256; };
  size_t o = 0;
  const size_t plan = o; o = al(o + (size_t)T_m * DSPLAN_BYTES);
  const size_t tab = o;  o = al(o + (size_t)T_m * CSM_FB_BUCKETS);
  const size_t lp = o;   o = al(o + (size_t)T_m * C * (MAXQ - 1) * SPLIT_THREADS * 8);
  const size_t pc = o;   o = al(o + (size_t)T_m * C * MAXQ * 4);
  const size_t uc = o;   o = al(o + (size_t)T_m * C * SPLIT_WAVES * 4);
  const size_t ul = o;   o = al(o + (size_t)T_m * C * SPLIT_WAVES * SPLIT_FL * 4);
  if (sp) {
    sp->plan = base + plan;
    sp->tab = (int8_t*)(base + tab);
    sp->lp = (double*)(base + lp);
    sp->pc = (int32_t*)(base + pc);
    sp->ucnt = (int32_t*)(base + uc);
    sp->ulist = (uint32_t*)(base + ul);
    sp->C = (int)C;
    sp->cells = CC;
  }
  return o;
}

// What every decile entry point does first: prep, the checks they share, and the launch
// arguments with the quantile table filled in.  The caller adds its own checks, returns CSM_OK
// for T_m == 0 and hands *a to deciles_dispatch.
static int dec_args(csm_ctx* ctx, const char* who, const double* M, const double* NR,
                    const uint16_t* ids, int32_t T_m, int64_t N, int32_t n_bins,
                    const double* qtable, int8_t* L, double* EW, int32_t* CNT, int32_t* NV,
                    double* LS, DecLaunch* a) {
  int r = prep(ctx);
  if (r) return r;
  if (!M || !L || !qtable || N <= 0 || T_m < 0 || n_bins < 1 || n_bins > MAXQ - 1 || N > 0x7FFFFFFFLL)
    return set_err(ctx, CSM_E_INVAL, "%s: bad arguments (N=%lld T_m=%d n_bins=%d)", who,
                   (long long)N, T_m, n_bins);
  const bool v2 = (N % 2 == 0) && aligned16(M) && (!NR || aligned16(NR)) && (((uintptr_t)L & 1u) == 0);
  *a = DecLaunch{T_m, ctx->stream, M, NR, N, n_bins, QTab{}, L, NR ? EW : nullptr,
                 NR ? CNT : nullptr, NV, g_dec_timing, const_cast<uint16_t*>(ids), nullptr, LS,
                 nullptr, v2};
  for (int i = 0; i < MAXQ; ++i) a->q.q[i] = i <= n_bins ? qtable[i] : 1.0;
  return CSM_OK;
}

// One decile pass: picks the kernels for the row width, the ids (a.ids: the PRE kernels) and the
// tune knobs, and fills in a.flg and a.ticket.  a.LS: narrow rows on ids form the long-short in
// the decile launch (its last workgroup), and so does the split pass; every other pass with
// k_long_short after it -- measured the same on C4's wide rows (1.968 vs 1.971 ms/step), and
// the general kernel stays free of the per-workgroup fence
static int deciles_dispatch(csm_ctx* ctx, const char* who, DecLaunch a) {
  const bool pre = a.ids != nullptr, wide = a.N > g_tune_dec_narrow_max;
  double* LSw = (wide || !pre) ? a.LS : nullptr;
  if (LSw) a.LS = nullptr;
  bool ok;
  if (pre) {   // ids written by csm_signal_ids / csm_momentum_multi_ids: M is read only for a few cells
    int r = ctx_reserve(ctx, who, "the context's row-flag buffer", &ctx->dec_flg,
                        &ctx->dec_flg_bytes, (size_t)a.T_m * sizeof(int32_t));
    if (r) return r;
    a.flg = g_tune_dec_merge ? ctx->dec_flg : nullptr;
    // wide rows of a short date shard (fewer rows than half the CUs: one workgroup per row
    // leaves most of the chip idle): the split pass (plan, chunked sweep over the whole chip,
    // finish with the fused long-short) when the row's (chunk, wave) lists fit the finish
    // launch's merge.  Same labels and counts as the merged pass; means in another fixed order.
    const int64_t C = (a.N + g_tune_dec_split_cells - 1) / g_tune_dec_split_cells;
    const bool split = g_tune_dec_split == 1 ||
                       (g_tune_dec_split == 2 && (int64_t)a.T_m * 2 <= (int64_t)ctx->n_cu);
    if (split && a.flg && !a.q.legs && wide && C * SPLIT_WAVES <= DSPLIT_MAXL) {
      r = ctx_reserve(ctx, who, "the split decile workspace", &ctx->dsplit, &ctx->dsplit_bytes,
                      dsplit_layout(a.T_m, a.N, nullptr, nullptr));
      if (r) return r;
      DecSplit sp;
      dsplit_layout(a.T_m, a.N, &sp, (char*)ctx->dsplit);
      sp.pf = g_tune_dec_split_pf == 2 ? (C * a.T_m <= (int64_t)ctx->n_cu) : g_tune_dec_split_pf;
      a.LS = LSw;
      LSw = nullptr;
      a.ticket = a.LS ? ctx->ticket : nullptr;
      ok = launch_deciles_split(a, sp);
    } else {
      a.ticket = a.LS ? ctx->ticket : nullptr;
      // sweep rows: 2048 buckets (the fixed map's ids >> 2)
      ok = wide ? launch_deciles_pre(a, g_tune_dec_split_cells) : launch_deciles_pre_narrow(a);
    }
  } else if (!wide) {   // rows of a few thousand assets (C2/C3/C5)
    ok = launch_deciles_narrow(a);
  } else {
    ok = dec_nb_dispatch(a, [&](auto nb) {
      constexpr int NB = decltype(nb)::value;
      dec_launch(a.v2 ? k_deciles<NB, true> : k_deciles<NB, false>, dec_wide::kThreads, a, nullptr,
                 nullptr, nullptr);
    });
  }
  if (!ok)
    return set_err(ctx, CSM_E_INVAL, "%s: n_bins=%d unsupported with NR (use 2,3,4,5,10,20)", who,
                   a.n_bins);
  LAUNCH_CHECK(ctx, who);
  if (LSw) {
    hipLaunchKernelGGL(k_long_short, dim3(1), dim3(LS_THREADS), 0, ctx->stream, a.EW, a.CNT, a.T_m,
                       a.n_bins, LSw);
    LAUNCH_CHECK(ctx, "k_long_short");
  }
  return CSM_OK;
}

// the ids entry points' own check (NR may be NULL)
static int ids_check(csm_ctx* ctx, const char* who, const DecLaunch& a) {
  if (a.ids && (a.N % 4) == 0 && ((uintptr_t)a.ids & 7u) == 0 && aligned16(a.M) &&
      (!a.NR || aligned16(a.NR)) && (((uintptr_t)a.L & 3u) == 0))
    return CSM_OK;
  return set_err(ctx, CSM_E_INVAL, "%s: needs N %% 4 == 0, 8-B aligned ids, 16-B aligned M / NR, "
                 "4-B aligned L (N=%lld)", who, (long long)a.N);
}

extern "C" {

int csm_deciles(csm_ctx* ctx, const double* M, const double* NR, int32_t T_m, int64_t N,
                int32_t n_bins, const double* qtable, int8_t* L, double* EW, int32_t* CNT,
                int32_t* NV) {
  DecLaunch a;
  int r = dec_args(ctx, "csm_deciles", M, NR, nullptr, T_m, N, n_bins, qtable, L, EW, CNT, NV,
                   nullptr, &a);
  if (r) return r;
  if (NR && (!EW || !CNT))
    return set_err(ctx, CSM_E_INVAL, "csm_deciles: EW and CNT are required when NR is given");
  if (T_m == 0) return CSM_OK;
  return deciles_dispatch(ctx, "csm_deciles", a);
}

int csm_long_short(csm_ctx* ctx, const double* EW, const int32_t* CNT, int32_t T_m,
                   int32_t n_bins, double* LS) {
  int r = prep(ctx);
  if (r) return r;
  if (!EW || !CNT || !LS || T_m < 0 || n_bins < 1)
    return set_err(ctx, CSM_E_INVAL, "csm_long_short: bad arguments");
  if (T_m == 0) return CSM_OK;
  hipLaunchKernelGGL(k_long_short, dim3(1), dim3(LS_THREADS), 0, ctx->stream, EW, CNT, T_m, n_bins, LS);
  LAUNCH_CHECK(ctx, "k_long_short");
  return CSM_OK;
}

int csm_deciles_ids(csm_ctx* ctx, const double* M, const double* NR, const uint16_t* ids,
                    int32_t T_m, int64_t N, int32_t n_bins, const double* qtable, int8_t* L,
                    double* EW, int32_t* CNT, int32_t* NV) {
  DecLaunch a;
  int r = dec_args(ctx, "csm_deciles_ids", M, NR, ids, T_m, N, n_bins, qtable, L, EW, CNT, NV,
                   nullptr, &a);
  if (r) return r;
  if (NR && (!EW || !CNT))
    return set_err(ctx, CSM_E_INVAL, "csm_deciles_ids: EW and CNT are required when NR is given");
  if ((r = ids_check(ctx, "csm_deciles_ids", a))) return r;
  if (T_m == 0) return CSM_OK;
  return deciles_dispatch(ctx, "csm_deciles_ids", a);
}

int csm_deciles_ids_legs(csm_ctx* ctx, const double* M, const uint16_t* ids, int32_t T_m,
                         int64_t N, int32_t n_bins, const double* qtable, int8_t* L, int32_t* NV) {
  DecLaunch a;
  int r = dec_args(ctx, "csm_deciles_ids_legs", M, nullptr, ids, T_m, N, n_bins, qtable, L,
                   nullptr, nullptr, NV, nullptr, &a);
  if (r || (r = ids_check(ctx, "csm_deciles_ids_legs", a))) return r;
  if (T_m == 0) return CSM_OK;
  a.q.legs = 1;
  return deciles_dispatch(ctx, "csm_deciles_ids_legs", a);
}

int csm_deciles_ids_ls(csm_ctx* ctx, const double* M, const double* NR, const uint16_t* ids,
                       int32_t T_m, int64_t N, int32_t n_bins, const double* qtable, int8_t* L,
                       double* EW, int32_t* CNT, int32_t* NV, double* LS) {
  DecLaunch a;
  int r = dec_args(ctx, "csm_deciles_ids_ls", M, NR, ids, T_m, N, n_bins, qtable, L, EW, CNT, NV,
                   LS, &a);
  if (r) return r;
  if (!NR || !EW || !CNT || !LS)
    return set_err(ctx, CSM_E_INVAL, "csm_deciles_ids_ls: NR, EW, CNT and LS are required");
  if ((r = ids_check(ctx, "csm_deciles_ids_ls", a))) return r;
  if (T_m == 0) return CSM_OK;
  return deciles_dispatch(ctx, "csm_deciles_ids_ls", a);
}

int csm_pipeline(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N, const int64_t* month_start,
                 int32_t T_m, int32_t max_month_days, int32_t min_month_days, int32_t J,
                 int32_t skip, int32_t n_bins,
                 const double* qtable, double* PM, double* R, double* M, double* NR, int8_t* L,
                 double* EW, int32_t* CNT, int32_t* NV, double* LS) {
  DecLaunch a;
  int r = dec_args(ctx, "csm_pipeline", M, NR, nullptr, T_m, N, n_bins, qtable, L, EW, CNT, NV,
                   LS, &a);
  if (r) return r;
  if (!P || !month_start || !NR || !EW || !CNT || !LS)
    return set_err(ctx, CSM_E_INVAL, "csm_pipeline: bad arguments (N=%lld T_m=%d n_bins=%d)",
                   (long long)N, T_m, n_bins);
  if (T_m == 0) return CSM_OK;
  // the id path needs 4-aligned rows and the wide decile kernel; otherwise signal + deciles
  const bool want_ids = (N % 4) == 0 && N > g_tune_dec_narrow_max && aligned16(P) && aligned16(M) &&
                        aligned16(NR) && (((uintptr_t)L & 3u) == 0) && (!PM || aligned16(PM)) &&
                        (!R || aligned16(R));
  if (want_ids) {
    r = ctx_reserve(ctx, "csm_pipeline", "the bucket-id scratch", &ctx->scratch,
                    &ctx->scratch_bytes, (size_t)T_m * (size_t)N * sizeof(uint16_t));
    if (r) return r;
    a.ids = (uint16_t*)ctx->scratch;
  }
  (void)min_month_days;
  r = signal_launch(ctx, "csm_pipeline", P, T_d, N, month_start, T_m, max_month_days, J,
                    skip, PM, R, M, NR, nullptr, nullptr, nullptr, false, a.ids);
  if (r) return r;
  // the id path: labels, decile means and the long-short in one launch
  return deciles_dispatch(ctx, "csm_pipeline", a);
}

}  // extern "C"
