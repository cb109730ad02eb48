// asym.hip -- asymmetry signals of the daily returns (rules AS1..AS7 in DESIGN.md 7): each (month,
// asset)'s day counts and squared-return sums by the sign of the return, its market-model sums
// over the days on one side of a daily series, and the window model on them -- the information
// discreteness of Da, Gurun and Warachka (2014), the signed jump variation RSJ, the downside
// semi-volatility and the downside (or upside) beta.
//
//   k_asym_sums       AS2.  A walker of daytrip.h's month_walk shaped like k_daily_sums's: the V1
//                     lead-in, trips of MS_TRIP rows of P, FD's rows uniform and only when the
//                     call has an FD (HASF); one or two assets per lane (csm_tune "asums_pair",
//                     "asums_chunks").  The side of a row is a property of the row, so it is one
//                     scalar compare per row; every add is a select, no branch on a lane's data.
//                     The gfx950 compile (no scratch in any) and, on MI355X, 100,000 x 10,000
//                     days / 5,000 x 6,522 days at each one's best chunk count (scripts/
//                     bench_asym.py; k_daily_sums 2.23 / 0.110 ms in the same process, 2.35 /
//                     0.125 at its own auto count):
//                       per lane, HASF   VGPRs   waves per SIMD   ms
//                       one, no           79     6
//                       one, yes         102     4                2.24 / 0.119
//                       two, no          141     3                1.88 / 0.096 (11 / 100 chunks)
//                       two, yes         185     2                2.38 / 0.121
//                     One asset per lane is what every panel takes: with the six side sums two
//                     per lane leave a SIMD two waves for four, and measured slower at every
//                     chunk count of both runs.  Two per lane (16-B loads, int2 /
//                     store_pair stores) stays behind csm_tune "asums_pair" = 2 for even N with
//                     aligned panels.
//   k_asym_model      AS3.  k_liq_model's shape: a lane per asset over (64 assets) x (chunk of
//                     consecutive months); every window's sums are added again from its oldest
//                     month, read from the AS2 panels a requested output depends on (csm_tune
//                     "amodel_chunks").  The window ends `skip` months back.  48 VGPRs, no scratch.
//                     Window 12, every output: 5.42 / 0.215 ms beside k_liq_model's 3.21 / 0.147
//                     (eleven panels read for eight).
#include "csm_common.h"
#include "dayret.h"
#include "daytrip.h"
#include "scan.h"

#define ASM_THREADS 64
#define ASM_MAXW 36
#define ASM_MAXSKIP 12

// "asums_chunks":  month chunks of k_asym_sums, 0 auto (scan.h auto_chunks) | n >= 1 that many
// "amodel_chunks": month chunks of k_asym_model, 0 auto, one month per chunk | n >= 1 that many
// (both clamped to T_m)
// "asums_pair":    0 auto, one asset per lane | 1 one per lane | 2 two where the panels allow
// Every value gives the same bits.
static int g_tune_asums_chunks = 0;
static int g_tune_amodel_chunks = 0;
static int g_tune_asums_pair = 0;
static const TuneKnob g_knobs[] = {
    {"asums_chunks", &g_tune_asums_chunks, [](int v) { return v >= 0; }},
    {"amodel_chunks", &g_tune_amodel_chunks, [](int v) { return v >= 0; }},
    {"asums_pair", &g_tune_asums_pair, [](int v) { return v >= 0 && v <= 2; }},
};

// ------------------------------------------------------------------------------- AS2
// One asset's counts and sums of the month being walked.
struct AsAcc {
  double sup, sdn, br, bf, bff, brf;
  int nd, nup, ndn, nb;
};

__device__ __forceinline__ void as_reset(AsAcc& s) {
  s.sup = s.sdn = s.br = s.bf = s.bff = s.brf = 0.0;
  s.nd = s.nup = s.ndn = s.nb = 0;
}

// One day row: price x, the row's f and whether f lies on the side (uniform; false for a NaN f).
// The V1 state moves whatever f is.  A zero return counts in nd only.
template <bool HASF>
__device__ __forceinline__ void as_step(AsAcc& s, DrLane& l, double x, double f, bool on,
                                        int max_gap) {
  const double r = dr_step(l, x, max_gap);
  const bool ret = !isnan_d(r), up = r > 0.0, dn = r < 0.0;   // (NaN r: neither)
  const double rr = r * r;
  s.nd += ret ? 1 : 0;
  s.nup += up ? 1 : 0;
  s.sup = up ? s.sup + rr : s.sup;
  s.ndn += dn ? 1 : 0;
  s.sdn = dn ? s.sdn + rr : s.sdn;
  if (HASF) {
    const bool b = ret && on;
    s.nb += b ? 1 : 0;
    s.br = b ? s.br + r : s.br;
    s.bf = b ? s.bf + f : s.bf;
    s.bff = b ? s.bff + f * f : s.bff;
    s.brf = b ? s.brf + r * f : s.brf;
  }
}

struct AsOut {
  int32_t *ND, *NUP, *NDN;
  double *SUP, *SDN;
  int32_t* NB;   // the five side panels: all or none (HASF)
  double *BR, *BF, *BFF, *BRF;
};

template <int VEC, bool HASF>
__device__ __forceinline__ void as_flush(const AsAcc (&s)[VEC], int64_t o, const AsOut& out) {
  if (VEC == 2) {
    *reinterpret_cast<int2*>(out.ND + o) = make_int2(s[0].nd, s[VEC - 1].nd);
    *reinterpret_cast<int2*>(out.NUP + o) = make_int2(s[0].nup, s[VEC - 1].nup);
    *reinterpret_cast<int2*>(out.NDN + o) = make_int2(s[0].ndn, s[VEC - 1].ndn);
    store_pair(out.SUP + o, s[0].sup, s[VEC - 1].sup);
    store_pair(out.SDN + o, s[0].sdn, s[VEC - 1].sdn);
    if (HASF) {
      *reinterpret_cast<int2*>(out.NB + o) = make_int2(s[0].nb, s[VEC - 1].nb);
      store_pair(out.BR + o, s[0].br, s[VEC - 1].br);
      store_pair(out.BF + o, s[0].bf, s[VEC - 1].bf);
      store_pair(out.BFF + o, s[0].bff, s[VEC - 1].bff);
      store_pair(out.BRF + o, s[0].brf, s[VEC - 1].brf);
    }
  } else {
    out.ND[o] = s[0].nd;
    out.NUP[o] = s[0].nup;
    out.NDN[o] = s[0].ndn;
    out.SUP[o] = s[0].sup;
    out.SDN[o] = s[0].sdn;
    if (HASF) {
      out.NB[o] = s[0].nb;
      out.BR[o] = s[0].br;
      out.BF[o] = s[0].bf;
      out.BFF[o] = s[0].bff;
      out.BRF[o] = s[0].brf;
    }
  }
}

// k_asym_sums's walker (daytrip.h): the V1 lead-in, P's rows and, with HASF, FD's, which are
// uniform; rows past the chunk are ABSENT prices and NaN f: they change nothing.
template <int VEC, bool HASF>
struct AsWalker {
  const double* __restrict__ P;
  const double* __restrict__ FD;
  int64_t N, a;
  int max_gap;
  bool neg;   // side -1: the side days have f < 0; +1: f > 0
  AsOut out;
  DrLane lane[VEC];
  AsAcc acc[VEC];
  struct Rows {
    double x[MS_TRIP][VEC];
    double f[HASF ? MS_TRIP : 1] = {};
  };

  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int k = 0; k < VEC; ++k) as_reset(acc[k]);
  }
  __device__ __forceinline__ void begin(int64_t dA) {
    dr_lead_in<VEC>(lane, P, N, dA, max_gap, [&](int k) { return a + k; });
    reset();
  }
  __device__ __forceinline__ void load(Rows& r, int64_t d, int64_t dB) const {
    trip_load<MS_TRIP, VEC>(r.x, P, N, a, d, dB, absent_val());
    if (HASF) {
#pragma unroll
      for (int i = 0; i < MS_TRIP; ++i) r.f[HASF ? i : 0] = d + i < dB ? FD[d + i] : qnan();
    }
  }
  __device__ __forceinline__ void own(Rows&, int64_t, int64_t) const {}
  __device__ __forceinline__ void step(const Rows& r, int i) {
    const double f = r.f[HASF ? i : 0];
    const bool on = HASF && (neg ? f < 0.0 : f > 0.0);   // (uniform)
#pragma unroll
    for (int k = 0; k < VEC; ++k) as_step<HASF>(acc[k], lane[k], r.x[i][k], f, on, max_gap);
  }
  __device__ __forceinline__ void flush(int m) {   // the V1 state runs on
    as_flush<VEC, HASF>(acc, (int64_t)m * N + a, out);
    reset();
  }
};

template <int VEC, bool HASF>
__global__ __launch_bounds__(MS_THREADS) void k_asym_sums(
    const double* __restrict__ P, const double* __restrict__ FD, int64_t T_d, int64_t N,
    const int64_t* __restrict__ ms, int T_m, int G, int max_gap, int neg, AsOut out) {
  const int64_t a = ((int64_t)blockIdx.x * MS_THREADS + threadIdx.x) * VEC;
  if (a >= N) return;   // (no barrier anywhere below; VEC == 2 has N even, so a + 1 < N)
  AsWalker<VEC, HASF> w{P, FD, N, a, max_gap, neg != 0, out};
  month_walk<MS_TRIP>(w, ms, T_m, G, T_d);
}

template <int VEC, bool HASF>
static inline void as_launch(csm_ctx* ctx, dim3 grid, const double* P, const double* FD,
                             int64_t T_d, int64_t N, const int64_t* ms, int T_m, int max_gap,
                             int neg, const AsOut& out) {
  hipLaunchKernelGGL((k_asym_sums<VEC, HASF>), grid, dim3(MS_THREADS), 0, ctx->stream, P, FD, T_d,
                     N, ms, T_m, (int)grid.y, max_gap, neg, out);
}

// ------------------------------------------------------------------------------- AS3
struct AsmIn {
  const int32_t *ND, *NUP, *NDN;
  const double *SUP, *SDN;
  const int32_t* NB;
  const double *BR, *BF, *BFF, *BRF, *M;
};
struct AsmOut {
  double *ID, *RSJ, *DSVOL, *DNBETA;
  int32_t *NOBS, *NSIDE;
};

__global__ __launch_bounds__(ASM_THREADS) void k_asym_model(AsmIn in, int T_m, int64_t N, int Wm,
                                                           int skip, int min_obs, int min_side,
                                                           int G, AsmOut o) {
  const int64_t a = (int64_t)blockIdx.x * ASM_THREADS + threadIdx.x;
  if (a >= N) return;
  int m0, m1;
  chunk_range(T_m, G, (int)blockIdx.y, m0, m1);   // G <= T_m: at least one month
  const double NaN = qnan();
  // (uniform) the panels somebody reads: a panel no requested output depends on is not loaded
  // (its sum stays zero and feeds nothing written)
  const bool needd = o.ID || o.RSJ || o.DSVOL || o.NOBS;   // ND
  const bool needc = o.ID != nullptr;                       // NUP, NDN
  const bool needup = o.RSJ != nullptr;                     // SUP
  const bool needdn = o.RSJ || o.DSVOL;                     // SDN
  const bool neednb = o.DNBETA || o.NSIDE;                  // NB
  const bool needb = o.DNBETA != nullptr;                   // BR, BF, BFF, BRF
  for (int t = m0; t < m1; ++t) {
    double id = NaN, rsj = NaN, dsvol = NaN, dnbeta = NaN;
    int nd = 0, nb = 0;
    const int j0 = t - skip - Wm + 1;
    if (j0 >= 0) {   // (uniform) a whole window, added oldest month first
      int nup = 0, ndn = 0;
      double sup = 0.0, sdn = 0.0, br = 0.0, bf = 0.0, bff = 0.0, brf = 0.0;
#pragma unroll 4
      for (int j = j0; j <= t - skip; ++j) {
        const int64_t oj = (int64_t)j * N + a;
        if (needd) nd += in.ND[oj];
        if (needc) {
          nup += in.NUP[oj];
          ndn += in.NDN[oj];
        }
        if (needup) sup += in.SUP[oj];
        if (needdn) sdn += in.SDN[oj];
        if (neednb) nb += in.NB[oj];
        if (needb) {
          br += in.BR[oj];
          bf += in.BF[oj];
          bff += in.BFF[oj];
          brf += in.BRF[oj];
        }
      }
      const double ndf = (double)nd, nbf = (double)nb;
      if (nd >= min_obs) {
        if (needc) {
          const double q = (double)(ndn - nup) / ndf;
          const double m = in.M[(int64_t)t * N + a];
          id = m > 0.0 ? q : (m < 0.0 ? -q : (m == 0.0 ? 0.0 : NaN));
        }
        const double tot = sup + sdn;
        if (tot > 0.0) rsj = (sup - sdn) / tot;
        dsvol = sqrt(sdn / ndf);
      }
      const double mf = bf / nbf;
      const double cff = bff - bf * mf, crf = brf - br * mf;
      if (nb >= min_side && cff > 0.0) dnbeta = crf / cff;
    }
    const int64_t ot = (int64_t)t * N + a;
    if (o.ID) o.ID[ot] = id;
    if (o.RSJ) o.RSJ[ot] = rsj;
    if (o.DSVOL) o.DSVOL[ot] = dsvol;
    if (o.DNBETA) o.DNBETA[ot] = dnbeta;
    if (o.NOBS) o.NOBS[ot] = nd;
    if (o.NSIDE) o.NSIDE[ot] = nb;
  }
}


extern "C" {

int csm_tune_asym(const char* key, int value) { return tune_set(g_knobs, key, value); }

int csm_asym_sums(csm_ctx* ctx, const double* P, const double* FD, int64_t T_d, int64_t N,
                  const int64_t* month_start, int32_t T_m, int32_t max_month_days, int32_t max_gap,
                  int32_t side, int32_t* ND, int32_t* NUP, int32_t* NDN, double* SUP, double* SDN,
                  int32_t* NB, double* BR, double* BF, double* BFF, double* BRF) {
  int r = prep(ctx);
  if (r) return r;
  if (!P || !month_start || !ND || !NUP || !NDN || !SUP || !SDN || T_d < 1 || N < 1 || T_m < 1 ||
      T_d > ((int64_t)1 << 40) / N)
    return set_err(ctx, CSM_E_INVAL, "csm_asym_sums: bad arguments (T_d=%lld N=%lld T_m=%d)",
                   (long long)T_d, (long long)N, T_m);
  if (max_month_days < 1 || max_month_days > 32)
    return set_err(ctx, CSM_E_INVAL, "csm_asym_sums: max_month_days=%d is outside [1, 32]",
                   max_month_days);
  if (max_gap < 1 || max_gap > DM_MAXGAP)
    return set_err(ctx, CSM_E_INVAL, "csm_asym_sums: max_gap=%d is outside [1, %d]", max_gap,
                   DM_MAXGAP);
  if (side != -1 && side != 1)
    return set_err(ctx, CSM_E_INVAL, "csm_asym_sums: side=%d must be -1 or +1", side);
  const bool hasf = FD != nullptr;
  const int given = (NB != nullptr) + (BR != nullptr) + (BF != nullptr) + (BFF != nullptr) +
                    (BRF != nullptr);
  if (given != (hasf ? 5 : 0))
    return set_err(ctx, CSM_E_INVAL,
                   "csm_asym_sums: NB, BR, BF, BFF and BRF are given if and only if FD is");
  const bool v2 = g_tune_asums_pair == 2 && (N % 2 == 0) && aligned16(P) && aligned8(ND) &&
                  aligned8(NUP) && aligned8(NDN) && aligned16(SUP) && aligned16(SDN) &&
                  (!hasf || (aligned8(NB) && aligned16(BR) && aligned16(BF) && aligned16(BFF) &&
                             aligned16(BRF)));
  // Auto chunk count: k_liq_sums's, about 32 workgroups per CU (scan.h auto_chunks), not
  // k_daily_sums's eight: at one asset per lane four waves a SIMD are resident and finer chunks
  // keep them fed.  MI355X (scripts/bench_asym.py), one per lane / two per lane: 100,000 assets x
  // 461 months 3 / 6 / 11 / 22 / 44 / 88 chunks 2.59 / 2.49 / 2.28 / 2.26 / 2.24 / 2.27 ms and
  // 3.13 / 2.59 / 2.48 / 2.38 / 2.42 / 2.53 ms (auto 21; eight per CU gave 6); 5,000 assets x 300
  // months 13 / 25 / 50 / 100 / 150 / 300 chunks 0.203 / 0.129 / 0.119 / 0.122 / 0.125 / 0.137 ms
  // and 0.238 / 0.147 / 0.121 / 0.131 / 0.139 / 0.166 ms (auto 100).
  const dim3 grid = month_grid(ctx, N, MS_THREADS * (v2 ? 2 : 1), g_tune_asums_chunks, 32, T_m);
  const AsOut out{ND, NUP, NDN, SUP, SDN, NB, BR, BF, BFF, BRF};
  const int neg = side < 0;
  if (v2 && hasf)
    as_launch<2, true>(ctx, grid, P, FD, T_d, N, month_start, T_m, max_gap, neg, out);
  else if (v2)
    as_launch<2, false>(ctx, grid, P, FD, T_d, N, month_start, T_m, max_gap, neg, out);
  else if (hasf)
    as_launch<1, true>(ctx, grid, P, FD, T_d, N, month_start, T_m, max_gap, neg, out);
  else
    as_launch<1, false>(ctx, grid, P, FD, T_d, N, month_start, T_m, max_gap, neg, out);
  LAUNCH_CHECK(ctx, "k_asym_sums");
  return CSM_OK;
}

int csm_asym_model(csm_ctx* ctx, const int32_t* ND, const int32_t* NUP, const int32_t* NDN,
                   const double* SUP, const double* SDN, const int32_t* NB, const double* BR,
                   const double* BF, const double* BFF, const double* BRF, const double* M,
                   int32_t T_m, int64_t N, int32_t Wm, int32_t skip, int32_t min_obs,
                   int32_t min_side, double* ID, double* RSJ, double* DSVOL, double* DNBETA,
                   int32_t* NOBS, int32_t* NSIDE) {
  int r = prep(ctx);
  if (r) return r;
  if (!ND || !NUP || !NDN || !SUP || !SDN || bad_panel(T_m, N))
    return set_err(ctx, CSM_E_INVAL, "csm_asym_model: bad arguments (T_m=%d N=%lld)", T_m,
                   (long long)N);
  if (!ID && !RSJ && !DSVOL && !DNBETA && !NOBS && !NSIDE)
    return set_err(ctx, CSM_E_INVAL, "csm_asym_model: no output requested");
  if (Wm < 1 || Wm > ASM_MAXW)
    return set_err(ctx, CSM_E_INVAL, "csm_asym_model: Wm=%d is outside [1, %d]", Wm, ASM_MAXW);
  if (skip < 0 || skip > ASM_MAXSKIP)
    return set_err(ctx, CSM_E_INVAL, "csm_asym_model: skip=%d is outside [0, %d]", skip,
                   ASM_MAXSKIP);
  if (min_obs < 1)
    return set_err(ctx, CSM_E_INVAL, "csm_asym_model: min_obs=%d must be at least 1", min_obs);
  if (min_side < 2)
    return set_err(ctx, CSM_E_INVAL, "csm_asym_model: min_side=%d must be at least 2", min_side);
  const int given = (NB != nullptr) + (BR != nullptr) + (BF != nullptr) + (BFF != nullptr) +
                    (BRF != nullptr);
  if (given != 0 && given != 5)
    return set_err(ctx, CSM_E_INVAL, "csm_asym_model: NB, BR, BF, BFF and BRF go together");
  if ((ID && !M) || ((DNBETA || NSIDE) && given != 5))
    return set_err(ctx, CSM_E_INVAL,
                   "csm_asym_model: ID needs M, DNBETA and NSIDE need the five side panels");
  const int64_t slices = (N + ASM_THREADS - 1) / ASM_THREADS;
  // auto is one month per chunk, csm_liq_model's rule: a chunk needs no warm-up
  int64_t G = g_tune_amodel_chunks;
  if (G < 1 || G > T_m) G = T_m;
  if (G > 65535) G = 65535;   // (grid.y)
  const AsmIn in{ND, NUP, NDN, SUP, SDN, NB, BR, BF, BFF, BRF, M};
  const AsmOut o{ID, RSJ, DSVOL, DNBETA, NOBS, NSIDE};
  hipLaunchKernelGGL(k_asym_model, dim3((unsigned)slices, (unsigned)G), dim3(ASM_THREADS), 0,
                     ctx->stream, in, T_m, N, Wm, skip, min_obs, min_side, (int)G, o);
  LAUNCH_CHECK(ctx, "k_asym_model");
  return CSM_OK;
}

}  // extern "C"
