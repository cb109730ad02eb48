// liquidity.hip -- liquidity signals from the daily price and volume panels (rules Q1..Q6 in
// DESIGN.md 7): each (month, asset)'s day counts, volume, dollar volume and Amihud (2002) sums, and
// the window model on them -- ILLIQ, dollar average daily volume, turnover, and the shares of
// zero-return (Lesmond, Ogden and Trzcinka 1999) and zero-volume days.
//
//   k_liq_sums        Q2.  The month walk of daytrip.h on two panels: the V1 lead-in walks P only;
//                     then trips of TRIP day rows of P and V (csm_tune "lsums_chunks").
//                     Two panels double k_daily_sums's trip buffers, and the registers decide the
//                     shape.  The gfx950 compile (no scratch in any) and, on MI355X, 100,000 x
//                     10,000 days / 5,000 x 6,522 days at each one's best chunk count
//                     (profiles/r16/bench_liq_sweep.log; k_daily_sums 2.38 / 0.125 ms there):
//                       TRIP, per lane   VGPRs           waves per SIMD   ms
//                       8, one           133             3                3.65 / 0.147
//                       4, one            92             5                3.70 / 0.152
//                       4, two           179             2                3.76 / 0.154
//                       8, two           256 + 56 AGPR   1                4.54 / 0.184
//                     One asset per lane with TRIP 8 is the kernel every panel takes.  Two per
//                     lane (16-B loads of both panels, store_pair / int2 stores) with TRIP 4 stays
//                     behind csm_tune "lsums_pair" for even N with aligned panels: it issues half
//                     the load instructions and measured 2 to 5 % slower in both runs (bench_liq.log:
//                     3.46 / 0.162 ms against 3.38 / 0.155), two waves a SIMD hiding less than
//                     three.  The other two are not in the library.  (On daytrip.h's month_walk
//                     the first takes 159 VGPRs, still three waves a SIMD, and measures 0.5 to
//                     0.8 % slower: profiles/r18/walk_speed.md.)
//   k_liq_model       Q3.  k_daily_model's shape: a lane per asset over (64 assets) x (chunk of
//                     consecutive months); every window's sums are added again from its oldest
//                     month, read from the Q2 panels a requested output depends on (csm_tune
//                     "lmodel_chunks").
#include "csm_common.h"
#include "dayret.h"
#include "daytrip.h"
#include "scan.h"

#define LQM_THREADS 64
#define LQM_MAXW 12

// "lsums_chunks":  month chunks of k_liq_sums, 0 auto (scan.h auto_chunks) | n >= 1 that many
// "lmodel_chunks": month chunks of k_liq_model, 0 auto, one month per chunk | n >= 1 that many
// (both clamped to T_m)
// "lsums_pair":    0 auto, one asset per lane | 1 two per lane where the panels allow
// Every value gives the same bits.
static int g_tune_lsums_chunks = 0;
static int g_tune_lmodel_chunks = 0;
static int g_tune_lsums_pair = 0;
static const TuneKnob g_knobs[] = {
    {"lsums_chunks", &g_tune_lsums_chunks, [](int v) { return v >= 0; }},
    {"lmodel_chunks", &g_tune_lmodel_chunks, [](int v) { return v >= 0; }},
    {"lsums_pair", &g_tune_lsums_pair, [](int v) { return v == 0 || v == 1; }},
};

#define LQ_TRIP 8        // day rows per trip, one asset per lane
#define LQ_TRIP_PAIR 4   // and two per lane

// ------------------------------------------------------------------------------- Q2
// One asset's counts and sums of the month being walked.
struct LqAcc {
  double sv, sdv, sil;
  int np, nd, na, nzr, nzv;
};

__device__ __forceinline__ void lq_reset(LqAcc& s) {
  s.sv = s.sdv = s.sil = 0.0;
  s.np = s.nd = s.na = s.nzr = s.nzv = 0;
}

// One day row: price x, volume w (NaN is 0.0; whatever it is on an unpriced day, it is not
// taken).  r not NaN implies x priced, so an Amihud day's dv is a product of a price.
__device__ __forceinline__ void lq_step(LqAcc& s, DrLane& l, double x, double w, int max_gap) {
  const double r = dr_step(l, x, max_gap);
  const bool priced = !isnan_d(x), ret = !isnan_d(r);
  const double v = isnan_d(w) ? 0.0 : w;
  const double dv = x * v;
  const bool ami = ret && dv > 0.0;
  const double q = fabs(r) / dv;
  s.np += priced ? 1 : 0;
  s.sv = priced ? s.sv + v : s.sv;
  s.sdv = priced ? s.sdv + dv : s.sdv;
  s.nzv += (priced && v == 0.0) ? 1 : 0;
  s.nd += ret ? 1 : 0;
  s.nzr += (ret && r == 0.0) ? 1 : 0;
  s.na += ami ? 1 : 0;
  s.sil = ami ? s.sil + q : s.sil;
}

struct LqOut {
  int32_t *NP, *ND, *NA, *NZR, *NZV;
  double *SV, *SDV, *SIL;
};

template <int VEC>
__device__ __forceinline__ void lq_flush(const LqAcc (&s)[VEC], int64_t o, const LqOut& out) {
  if (VEC == 2) {
    *reinterpret_cast<int2*>(out.NP + o) = make_int2(s[0].np, s[VEC - 1].np);
    *reinterpret_cast<int2*>(out.ND + o) = make_int2(s[0].nd, s[VEC - 1].nd);
    *reinterpret_cast<int2*>(out.NA + o) = make_int2(s[0].na, s[VEC - 1].na);
    if (out.NZR) *reinterpret_cast<int2*>(out.NZR + o) = make_int2(s[0].nzr, s[VEC - 1].nzr);
    if (out.NZV) *reinterpret_cast<int2*>(out.NZV + o) = make_int2(s[0].nzv, s[VEC - 1].nzv);
    if (out.SV) store_pair(out.SV + o, s[0].sv, s[VEC - 1].sv);
    store_pair(out.SDV + o, s[0].sdv, s[VEC - 1].sdv);
    store_pair(out.SIL + o, s[0].sil, s[VEC - 1].sil);
  } else {
    out.NP[o] = s[0].np;
    out.ND[o] = s[0].nd;
    out.NA[o] = s[0].na;
    if (out.NZR) out.NZR[o] = s[0].nzr;
    if (out.NZV) out.NZV[o] = s[0].nzv;
    if (out.SV) out.SV[o] = s[0].sv;
    out.SDV[o] = s[0].sdv;
    out.SIL[o] = s[0].sil;
  }
}

// k_liq_sums's walker (daytrip.h): the V1 lead-in on P, then P's and V's rows; rows past the chunk
// are NaN: unpriced days, which change nothing.
template <int TRIP, int VEC>
struct LqWalker {
  const double* __restrict__ P;
  const double* __restrict__ V;
  int64_t N, a;
  int max_gap;
  LqOut out;
  DrLane lane[VEC];
  LqAcc acc[VEC];
  struct Rows {
    double p[TRIP][VEC], v[TRIP][VEC];
  };

  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int k = 0; k < VEC; ++k) lq_reset(acc[k]);
  }
  __device__ __forceinline__ void begin(int64_t dA) {
    dr_lead_in<VEC>(lane, P, N, dA, max_gap, [&](int k) { return a + k; });
    reset();
  }
  __device__ __forceinline__ void load(Rows& r, int64_t d, int64_t dB) const {
    trip_load<TRIP, VEC>(r.p, P, N, a, d, dB, qnan());
    trip_load<TRIP, VEC>(r.v, V, N, a, d, dB, qnan());
  }
  __device__ __forceinline__ void own(Rows&, int64_t, int64_t) const {}
  __device__ __forceinline__ void step(const Rows& r, int i) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) lq_step(acc[k], lane[k], r.p[i][k], r.v[i][k], max_gap);
  }
  __device__ __forceinline__ void flush(int m) {   // the V1 state runs on
    lq_flush<VEC>(acc, (int64_t)m * N + a, out);
    reset();
  }
};

template <int TRIP, int VEC>
__global__ __launch_bounds__(MS_THREADS) void k_liq_sums(
    const double* __restrict__ P, const double* __restrict__ V, int64_t T_d, int64_t N,
    const int64_t* __restrict__ ms, int T_m, int G, int max_gap, LqOut out) {
  const int64_t a = ((int64_t)blockIdx.x * MS_THREADS + threadIdx.x) * VEC;
  if (a >= N) return;   // (no barrier anywhere below; VEC == 2 has N even, so a + 1 < N)
  LqWalker<TRIP, VEC> w{P, V, N, a, max_gap, out};
  month_walk<TRIP>(w, ms, T_m, G, T_d);
}

// ------------------------------------------------------------------------------- Q3
struct LqmIn {
  const int32_t *NP, *ND, *NA, *NZR, *NZV;
  const double *SV, *SDV, *SIL, *SH;
};
struct LqmOut {
  double *ILLIQ, *DVOL, *TURN, *ZRET, *ZVOL;
  int32_t* NOBS;
};

__global__ __launch_bounds__(LQM_THREADS) void k_liq_model(LqmIn in, int T_m, int64_t N, int Wm,
                                                          int min_obs, double scale, int G,
                                                          LqmOut o) {
  const int64_t a = (int64_t)blockIdx.x * LQM_THREADS + threadIdx.x;
  if (a >= N) return;
  int m0, m1;
  chunk_range(T_m, G, (int)blockIdx.y, m0, m1);   // G <= T_m: at least one month
  const double NaN = qnan();
  // (uniform) the panels somebody reads: a panel no requested output depends on is not loaded
  // (its sum stays zero and feeds nothing written)
  const bool needa = o.ILLIQ || o.NOBS;                // NA
  const bool needil = o.ILLIQ != nullptr;              // SIL
  const bool needp = o.DVOL || o.TURN || o.ZVOL;       // NP
  const bool needdv = o.DVOL != nullptr;               // SDV
  const bool needv = o.TURN != nullptr;                // SV, SH
  const bool needr = o.ZRET != nullptr;                // ND, NZR
  const bool needzv = o.ZVOL != nullptr;               // NZV
  for (int t = m0; t < m1; ++t) {
    double illiq = NaN, dvol = NaN, turn = NaN, zret = NaN, zvol = NaN;
    int na = 0;
    if (t - Wm + 1 >= 0) {   // (uniform) a whole window, added oldest month first
      int np = 0, nd = 0, nzr = 0, nzv = 0;
      double sv = 0.0, sdv = 0.0, sil = 0.0;
#pragma unroll 4
      for (int j = t - Wm + 1; j <= t; ++j) {
        const int64_t oj = (int64_t)j * N + a;
        if (needa) na += in.NA[oj];
        if (needil) sil += in.SIL[oj];
        if (needp) np += in.NP[oj];
        if (needdv) sdv += in.SDV[oj];
        if (needv) sv += in.SV[oj];
        if (needr) {
          nd += in.ND[oj];
          nzr += in.NZR[oj];
        }
        if (needzv) nzv += in.NZV[oj];
      }
      const double naf = (double)na, npf = (double)np, ndf = (double)nd;
      if (na >= min_obs) illiq = (sil / naf) * scale;
      if (np >= min_obs) {
        dvol = sdv / npf;
        zvol = (double)nzv / npf;
        if (needv) {
          const double sh = in.SH[(int64_t)t * N + a];
          if (sh > 0.0) turn = (sv / npf) / sh;
        }
      }
      if (nd >= min_obs) zret = (double)nzr / ndf;
    }
    const int64_t ot = (int64_t)t * N + a;
    if (o.ILLIQ) o.ILLIQ[ot] = illiq;
    if (o.DVOL) o.DVOL[ot] = dvol;
    if (o.TURN) o.TURN[ot] = turn;
    if (o.ZRET) o.ZRET[ot] = zret;
    if (o.ZVOL) o.ZVOL[ot] = zvol;
    if (o.NOBS) o.NOBS[ot] = na;
  }
}


extern "C" {

int csm_tune_liq(const char* key, int value) { return tune_set(g_knobs, key, value); }

int csm_liq_sums(csm_ctx* ctx, const double* P, const double* V, int64_t T_d, int64_t N,
                 const int64_t* month_start, int32_t T_m, int32_t max_month_days, int32_t max_gap,
                 int32_t* NP, int32_t* ND, int32_t* NA, int32_t* NZR, int32_t* NZV, double* SV,
                 double* SDV, double* SIL) {
  int r = prep(ctx);
  if (r) return r;
  if (!P || !V || !month_start || !NP || !ND || !NA || !SDV || !SIL || T_d < 1 || N < 1 ||
      T_m < 1 || T_d > ((int64_t)1 << 40) / N)
    return set_err(ctx, CSM_E_INVAL, "csm_liq_sums: bad arguments (T_d=%lld N=%lld T_m=%d)",
                   (long long)T_d, (long long)N, T_m);
  if (max_month_days < 1 || max_month_days > 32)
    return set_err(ctx, CSM_E_INVAL, "csm_liq_sums: max_month_days=%d is outside [1, 32]",
                   max_month_days);
  if (max_gap < 1 || max_gap > DM_MAXGAP)
    return set_err(ctx, CSM_E_INVAL, "csm_liq_sums: max_gap=%d is outside [1, %d]", max_gap,
                   DM_MAXGAP);
  const bool v2 = g_tune_lsums_pair == 1 && (N % 2 == 0) && aligned16(P) && aligned16(V) &&
                  aligned8(NP) && aligned8(ND) && aligned8(NA) && (!NZR || aligned8(NZR)) &&
                  (!NZV || aligned8(NZV)) && (!SV || aligned16(SV)) && aligned16(SDV) &&
                  aligned16(SIL);
  // Auto chunk count: k_daily_fsums's, about 32 workgroups per CU (scan.h auto_chunks).  MI355X
  // (profiles/r16/bench_liq_sweep.log), one asset per lane, TRIP 8: 100,000 assets x 461 months
  // 3 / 6 / 11 / 22 / 44 / 88 chunks 3.91 / 3.95 / 3.75 / 3.72 / 3.69 / 3.65 ms (auto 21; eight
  // per CU would give 6); 5,000 assets x 300 months 13 / 25 / 50 / 100 / 150 / 300 chunks 0.214 /
  // 0.147 / 0.167 / 0.158 / 0.161 / 0.180 ms (auto 100).  Two per lane, TRIP 4: 5.25 / 4.10 /
  // 3.98 / 3.80 / 3.80 / 3.76 ms and 0.295 / 0.180 / 0.154 / 0.165 / 0.171 / 0.195 ms.
  const dim3 grid = month_grid(ctx, N, MS_THREADS * (v2 ? 2 : 1), g_tune_lsums_chunks, 32, T_m);
  const int g = (int)grid.y;
  const LqOut out{NP, ND, NA, NZR, NZV, SV, SDV, SIL};
  if (v2)
    hipLaunchKernelGGL((k_liq_sums<LQ_TRIP_PAIR, 2>), grid, dim3(MS_THREADS), 0, ctx->stream, P, V,
                       T_d, N, month_start, T_m, g, max_gap, out);
  else
    hipLaunchKernelGGL((k_liq_sums<LQ_TRIP, 1>), grid, dim3(MS_THREADS), 0, ctx->stream, P, V, T_d,
                       N, month_start, T_m, g, max_gap, out);
  LAUNCH_CHECK(ctx, "k_liq_sums");
  return CSM_OK;
}

int csm_liq_model(csm_ctx* ctx, const int32_t* NP, const int32_t* ND, const int32_t* NA,
                  const int32_t* NZR, const int32_t* NZV, const double* SV, const double* SDV,
                  const double* SIL, const double* SH, int32_t T_m, int64_t N, int32_t Wm,
                  int32_t min_obs, double scale, double* ILLIQ, double* DVOL, double* TURN,
                  double* ZRET, double* ZVOL, int32_t* NOBS) {
  int r = prep(ctx);
  if (r) return r;
  if (!NP || !ND || !NA || !SDV || !SIL || bad_panel(T_m, N))
    return set_err(ctx, CSM_E_INVAL, "csm_liq_model: bad arguments (T_m=%d N=%lld)", T_m,
                   (long long)N);
  if (!ILLIQ && !DVOL && !TURN && !ZRET && !ZVOL && !NOBS)
    return set_err(ctx, CSM_E_INVAL, "csm_liq_model: no output requested");
  if (Wm < 1 || Wm > LQM_MAXW)
    return set_err(ctx, CSM_E_INVAL, "csm_liq_model: Wm=%d is outside [1, %d]", Wm, LQM_MAXW);
  if (min_obs < 1)
    return set_err(ctx, CSM_E_INVAL, "csm_liq_model: min_obs=%d must be at least 1", min_obs);
  if (!(scale > 0.0) || scale > 1.7976931348623157e308)
    return set_err(ctx, CSM_E_INVAL, "csm_liq_model: scale=%g must be finite and positive", scale);
  if ((TURN && (!SV || !SH)) || (ZRET && !NZR) || (ZVOL && !NZV))
    return set_err(ctx, CSM_E_INVAL,
                   "csm_liq_model: TURN needs SV and SH, ZRET needs NZR and ZVOL needs NZV");
  const int64_t slices = (N + LQM_THREADS - 1) / LQM_THREADS;
  // auto is one month per chunk, csm_daily_model's rule: a chunk needs no warm-up
  int64_t G = g_tune_lmodel_chunks;
  if (G < 1 || G > T_m) G = T_m;
  if (G > 65535) G = 65535;   // (grid.y)
  const LqmIn in{NP, ND, NA, NZR, NZV, SV, SDV, SIL, SH};
  const LqmOut o{ILLIQ, DVOL, TURN, ZRET, ZVOL, NOBS};
  hipLaunchKernelGGL(k_liq_model, dim3((unsigned)slices, (unsigned)G), dim3(LQM_THREADS), 0,
                     ctx->stream, in, T_m, N, Wm, min_obs, scale, (int)G, o);
  LAUNCH_CHECK(ctx, "k_liq_model");
  return CSM_OK;
}

}  // extern "C"
