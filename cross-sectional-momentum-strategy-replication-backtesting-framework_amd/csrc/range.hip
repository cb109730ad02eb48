// range.hip -- range-based signals from the daily high, low and close panels (rules HL1..HL6 in
// DESIGN.md 7): each (month, asset)'s Parkinson (1980) sum of squared log ranges, its sum of
// Corwin-Schultz (2012) two-day high-low spreads and of Abdi-Ranaldo (2017) close-high-low terms,
// and the window model on them -- Parkinson volatility and the two bid-ask spread estimates.
//
//   k_range_sums      HL1..HL5.  The month walk of daytrip.h on three panels, one asset per lane:
//                     the lead-in walks the max_gap rows before the chunk for each asset's latest
//                     ranged row; then trips of TRIP day rows of H, L and C (csm_tune
//                     "rsums_chunks").  The first kernel here with
//                     log / exp: OCML's bodies are inlined, five logs (three without the overnight
//                     shift), one exp, three square roots and three divisions a pair, so the walk
//                     is bound by fp64 arithmetic, not by HBM; CS / AR are template flags, so a
//                     call without Corwin-Schultz carries none of its code.
//                     The gfx950 compile (no scratch in any), one asset per lane, VGPRs / waves
//                     per SIMD with CS and AR | CS | AR | neither:
//                       TRIP 2   133 / 3 | 123 / 4 |  85 / 5 |  71 / 7
//                       TRIP 4   157 / 3 | 147 / 3 | 110 / 4 |  95 / 5
//                       TRIP 8   206 / 2 | 195 / 2 | 158 / 3 | 143 / 3
//                     Each unrolled day step carries its own log bodies, so the registers grow
//                     faster with TRIP than k_liq_sums's did.  TRIP 4 keeps three waves a SIMD,
//                     as TRIP 2 does, with twice the loads in flight; TRIP 8 falls to two.
//                     On MI355X (profiles/r17/bench_range_trips.log, CS and AR on, 100,000 x
//                     10,000 days / 5,000 x 6,522 days; k_liq_sums 3.4 - 3.6 / 0.15 - 0.16 ms
//                     there) trips of 2 / 4 / 8 take 18.76 / 18.65 / 18.73 ms and 0.653 / 0.663 /
//                     0.662 ms: the trip length does not show, the arithmetic bounds the walk.
//                     TRIP 4 is the kernel in the library; the other two are not.
//   k_range_model     HL6.  k_liq_model's shape: a lane per asset over (64 assets) x (chunk of
//                     consecutive months); every window's sums are added again from its oldest
//                     month, read from the panels a requested output depends on (csm_tune
//                     "rmodel_chunks").
#include "csm_common.h"
#include "dayret.h"
#include "daytrip.h"
#include "scan.h"

#define RGM_THREADS 64
#define RGM_MAXW 12

// "rsums_chunks":  month chunks of k_range_sums, 0 auto (scan.h auto_chunks) | n >= 1 that many
// "rmodel_chunks": month chunks of k_range_model, 0 auto, one month per chunk | n >= 1 that many
// (both clamped to T_m).  Every value gives the same bits.
static int g_tune_rsums_chunks = 0;
static int g_tune_rmodel_chunks = 0;
static const TuneKnob g_knobs[] = {
    {"rsums_chunks", &g_tune_rsums_chunks, [](int v) { return v >= 0; }},
    {"rmodel_chunks", &g_tune_rmodel_chunks, [](int v) { return v >= 0; }},
};

#define RG_TRIP 4        // day rows per trip

// ------------------------------------------------------------------------------- HL1..HL5
// One asset's latest ranged row: its high, low and close, their logs, and the rows since it,
// saturated at DM_MAXGAP (one more is past every max_gap; the start: no such row).
struct RgLane {
  double H, L, C, h, l, c;
  int age;
};

// One asset's counts and sums of the month being walked.
struct RgAcc {
  double spk, scs, sar;
  int nrg, npr, ncs;
};

__device__ __forceinline__ void rg_reset(RgAcc& s) {
  s.spk = s.scs = s.sar = 0.0;
  s.nrg = s.npr = s.ncs = 0;
}

// HL1.  Every comparison is false on a NaN, so a NaN (or ABSENT) H, L or C is not ranged.
__device__ __forceinline__ bool rg_ranged(double H, double L, double C) {
  return L > 0.0 && H >= L && L <= C && C <= H;
}

// HL4's spread of the pair (p, day d): day d's range shifted by the overnight move, day p's raw.
// h, l are day d's logs, which a zero shift leaves as they are.
__device__ __forceinline__ double rg_cs(const RgLane& p, double H, double L, double h, double l) {
  const double s = L > p.C ? L - p.C : (H < p.C ? H - p.C : 0.0);
  const double Hs = H - s, Ls = L - s;
  double hs = h, ls = l;
  if (s != 0.0) {
    hs = log(Hs);
    ls = log(Ls);
  }
  const double up = p.h - p.l, us = hs - ls;
  const double beta = up * up + us * us;
  const double hh = p.H >= Hs ? p.h : hs;
  const double ll = p.L <= Ls ? p.l : ls;
  const double gamma = (hh - ll) * (hh - ll);
  const double k = 3.0 - 2.0 * 1.4142135623730951;   // 3 - 2 sqrt(2), sqrt(2) rounded to fp64
  const double alpha = (sqrt(2.0 * beta) - sqrt(beta)) / k - sqrt(gamma / k);
  const double e = exp(alpha);
  return 2.0 * (e - 1.0) / (1.0 + e);
}

// One day row (HL1..HL4).
template <bool CS, bool AR>
__device__ __forceinline__ void rg_step(RgAcc& s, RgLane& p, double H, double L, double C,
                                        int max_gap) {
  const int g = p.age + 1;
  if (!rg_ranged(H, L, C)) {
    p.age = g > DM_MAXGAP ? DM_MAXGAP : g;
    return;
  }
  const double h = log(H), l = log(L);
  const double c = AR ? log(C) : 0.0;
  const double u = h - l;
  s.nrg += 1;
  s.spk += u * u;
  if (g <= max_gap) {
    s.npr += 1;
    if (CS) {
      const double S = rg_cs(p, H, L, h, l);
      if (!isnan_d(S)) {
        s.ncs += 1;
        s.scs += S < 0.0 ? 0.0 : S;
      }
    }
    if (AR) {
      const double etap = (p.h + p.l) * 0.5, eta = (h + l) * 0.5;
      s.sar += (p.c - etap) * (p.c - eta);
    }
  }
  p.H = H;
  p.L = L;
  p.C = C;
  p.h = h;
  p.l = l;
  p.c = c;
  p.age = 0;
}

// The lead-in of a chunk that starts at row d0 (dr_lead_in's walk on three panels): the asset's
// latest ranged row among the max_gap rows before d0, clipped at row 0.  An older one makes no
// pair in the chunk.  Only the lanes still searching load; the walk ends when no lane of the wave
// is.
template <bool AR>
__device__ __forceinline__ void rg_lead_in(RgLane& p, const double* __restrict__ Hp,
                                           const double* __restrict__ Lp,
                                           const double* __restrict__ Cp, int64_t N, int64_t a,
                                           int64_t d0, int max_gap) {
  p.H = p.L = p.C = p.h = p.l = p.c = qnan();
  p.age = DM_MAXGAP;
  bool found = false;
  for (int g = 1; g <= max_gap && d0 - g >= 0; ++g) {
    if (!found) {
      const int64_t o = (d0 - g) * N + a;
      const double H = Hp[o], L = Lp[o], C = Cp[o];
      if (rg_ranged(H, L, C)) {
        p.H = H;
        p.L = L;
        p.C = C;
        p.h = log(H);
        p.l = log(L);
        p.c = AR ? log(C) : 0.0;
        p.age = g - 1;
        found = true;
      }
    }
    if (!__any(!found)) break;
  }
}

struct RgOut {
  int32_t *NRG, *NPR, *NCS;
  double *SPK, *SCS, *SAR;
};

template <bool CS, bool AR>
__device__ __forceinline__ void rg_flush(const RgAcc& s, int64_t o, const RgOut& out) {
  out.NRG[o] = s.nrg;
  out.NPR[o] = s.npr;
  out.SPK[o] = s.spk;
  if (CS) {
    out.NCS[o] = s.ncs;
    out.SCS[o] = s.scs;
  }
  if (AR) out.SAR[o] = s.sar;
}

// k_range_sums's walker (daytrip.h): the lead-in on three panels, then H's, L's and C's rows; rows
// past the chunk are NaN: days that are not ranged, which change nothing.
template <int TRIP, bool CS, bool AR>
struct RgWalker {
  const double* __restrict__ H;
  const double* __restrict__ L;
  const double* __restrict__ C;
  int64_t N, a;
  int max_gap;
  RgOut out;
  RgLane lane;
  RgAcc acc;
  struct Rows {
    double h[TRIP][1], l[TRIP][1], c[TRIP][1];
  };

  __device__ __forceinline__ void begin(int64_t dA) {
    rg_lead_in<AR>(lane, H, L, C, N, a, dA, max_gap);
    rg_reset(acc);
  }
  __device__ __forceinline__ void load(Rows& r, int64_t d, int64_t dB) const {
    trip_load<TRIP, 1>(r.h, H, N, a, d, dB, qnan());
    trip_load<TRIP, 1>(r.l, L, N, a, d, dB, qnan());
    trip_load<TRIP, 1>(r.c, C, N, a, d, dB, qnan());
  }
  __device__ __forceinline__ void own(Rows&, int64_t, int64_t) const {}
  __device__ __forceinline__ void step(const Rows& r, int i) {
    rg_step<CS, AR>(acc, lane, r.h[i][0], r.l[i][0], r.c[i][0], max_gap);
  }
  __device__ __forceinline__ void flush(int m) {   // the pair state runs on
    rg_flush<CS, AR>(acc, (int64_t)m * N + a, out);
    rg_reset(acc);
  }
};

template <int TRIP, bool CS, bool AR>
__global__ __launch_bounds__(MS_THREADS) void k_range_sums(
    const double* __restrict__ H, const double* __restrict__ L, const double* __restrict__ C,
    int64_t T_d, int64_t N, const int64_t* __restrict__ ms, int T_m, int G, int max_gap,
    RgOut out) {
  const int64_t a = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
  if (a >= N) return;   // (no barrier anywhere below)
  RgWalker<TRIP, CS, AR> w{H, L, C, N, a, max_gap, out};
  month_walk<TRIP>(w, ms, T_m, G, T_d);
}

// ------------------------------------------------------------------------------- HL6
struct RgmIn {
  const int32_t *NRG, *NPR, *NCS;
  const double *SPK, *SCS, *SAR;
};
struct RgmOut {
  double *PKVOL, *CSSPR, *ARSPR;
  int32_t* NOBS;
};

__global__ __launch_bounds__(RGM_THREADS) void k_range_model(RgmIn in, int T_m, int64_t N, int Wm,
                                                            int min_obs, double c4, int G,
                                                            RgmOut o) {
  const int64_t a = (int64_t)blockIdx.x * RGM_THREADS + threadIdx.x;
  if (a >= N) return;
  int m0, m1;
  chunk_range(T_m, G, (int)blockIdx.y, m0, m1);   // G <= T_m: at least one month
  const double NaN = qnan();
  // (uniform) the panels somebody reads: a panel no requested output depends on is not loaded
  // (its sum stays zero and feeds nothing written)
  const bool needpk = o.PKVOL != nullptr;              // NRG, SPK
  const bool needcs = o.CSSPR != nullptr;              // NCS, SCS
  const bool needar = o.ARSPR != nullptr;              // SAR
  const bool neednp = o.ARSPR || o.NOBS;               // NPR
  for (int t = m0; t < m1; ++t) {
    double pkvol = NaN, csspr = NaN, arspr = NaN;
    int npr = 0;
    if (t - Wm + 1 >= 0) {   // (uniform) a whole window, added oldest month first
      int nrg = 0, ncs = 0;
      double spk = 0.0, scs = 0.0, sar = 0.0;
#pragma unroll 4
      for (int j = t - Wm + 1; j <= t; ++j) {
        const int64_t oj = (int64_t)j * N + a;
        if (needpk) {
          nrg += in.NRG[oj];
          spk += in.SPK[oj];
        }
        if (needcs) {
          ncs += in.NCS[oj];
          scs += in.SCS[oj];
        }
        if (needar) sar += in.SAR[oj];
        if (neednp) npr += in.NPR[oj];
      }
      if (nrg >= min_obs) pkvol = sqrt(spk / (c4 * (double)nrg));
      if (ncs >= min_obs) csspr = scs / (double)ncs;
      if (npr >= min_obs) {
        const double mm = sar / (double)npr;
        arspr = mm > 0.0 ? 2.0 * sqrt(mm) : 0.0;
      }
    }
    const int64_t ot = (int64_t)t * N + a;
    if (o.PKVOL) o.PKVOL[ot] = pkvol;
    if (o.CSSPR) o.CSSPR[ot] = csspr;
    if (o.ARSPR) o.ARSPR[ot] = arspr;
    if (o.NOBS) o.NOBS[ot] = npr;
  }
}


extern "C" {

int csm_tune_range(const char* key, int value) { return tune_set(g_knobs, key, value); }

int csm_range_sums(csm_ctx* ctx, const double* H, const double* L, const double* C, int64_t T_d,
                   int64_t N, const int64_t* month_start, int32_t T_m, int32_t max_month_days,
                   int32_t max_gap, int32_t* NRG, int32_t* NPR, int32_t* NCS, double* SPK,
                   double* SCS, double* SAR) {
  int r = prep(ctx);
  if (r) return r;
  if (!H || !L || !C || !month_start || !NRG || !NPR || !SPK || T_d < 1 || N < 1 || T_m < 1 ||
      T_d > ((int64_t)1 << 40) / N)
    return set_err(ctx, CSM_E_INVAL, "csm_range_sums: bad arguments (T_d=%lld N=%lld T_m=%d)",
                   (long long)T_d, (long long)N, T_m);
  if ((NCS == nullptr) != (SCS == nullptr))
    return set_err(ctx, CSM_E_INVAL, "csm_range_sums: NCS and SCS go together");
  if (max_month_days < 1 || max_month_days > 32)
    return set_err(ctx, CSM_E_INVAL, "csm_range_sums: max_month_days=%d is outside [1, 32]",
                   max_month_days);
  if (max_gap < 1 || max_gap > DM_MAXGAP)
    return set_err(ctx, CSM_E_INVAL, "csm_range_sums: max_gap=%d is outside [1, %d]", max_gap,
                   DM_MAXGAP);
  // Auto chunk count: k_liq_sums's, about 32 workgroups per CU (scan.h auto_chunks)
  const dim3 grid = month_grid(ctx, N, MS_THREADS, g_tune_rsums_chunks, 32, T_m);
  const int g = (int)grid.y;
  const RgOut out{NRG, NPR, NCS, SPK, SCS, SAR};
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(MS_THREADS), 0, ctx->stream, H, L, C, T_d, N,
                       month_start, T_m, g, max_gap, out);
  };
  if (SCS && SAR)
    launch(k_range_sums<RG_TRIP, true, true>);
  else if (SCS)
    launch(k_range_sums<RG_TRIP, true, false>);
  else if (SAR)
    launch(k_range_sums<RG_TRIP, false, true>);
  else
    launch(k_range_sums<RG_TRIP, false, false>);
  LAUNCH_CHECK(ctx, "k_range_sums");
  return CSM_OK;
}

int csm_range_model(csm_ctx* ctx, const int32_t* NRG, const int32_t* NPR, const int32_t* NCS,
                    const double* SPK, const double* SCS, const double* SAR, int32_t T_m, int64_t N,
                    int32_t Wm, int32_t min_obs, double c4, double* PKVOL, double* CSSPR,
                    double* ARSPR, int32_t* NOBS) {
  int r = prep(ctx);
  if (r) return r;
  if (!NRG || !NPR || !SPK || bad_panel(T_m, N))
    return set_err(ctx, CSM_E_INVAL, "csm_range_model: bad arguments (T_m=%d N=%lld)", T_m,
                   (long long)N);
  if (!PKVOL && !CSSPR && !ARSPR && !NOBS)
    return set_err(ctx, CSM_E_INVAL, "csm_range_model: no output requested");
  if (Wm < 1 || Wm > RGM_MAXW)
    return set_err(ctx, CSM_E_INVAL, "csm_range_model: Wm=%d is outside [1, %d]", Wm, RGM_MAXW);
  if (min_obs < 1)
    return set_err(ctx, CSM_E_INVAL, "csm_range_model: min_obs=%d must be at least 1", min_obs);
  if (!(c4 > 0.0) || c4 > 1.7976931348623157e308)
    return set_err(ctx, CSM_E_INVAL, "csm_range_model: c4=%g must be finite and positive", c4);
  if ((CSSPR && (!NCS || !SCS)) || (ARSPR && !SAR))
    return set_err(ctx, CSM_E_INVAL,
                   "csm_range_model: CSSPR needs NCS and SCS and ARSPR needs SAR");
  const int64_t slices = (N + RGM_THREADS - 1) / RGM_THREADS;
  // auto is one month per chunk, csm_liq_model's rule: a chunk needs no warm-up
  int64_t G = g_tune_rmodel_chunks;
  if (G < 1 || G > T_m) G = T_m;
  if (G > 65535) G = 65535;   // (grid.y)
  const RgmIn in{NRG, NPR, NCS, SPK, SCS, SAR};
  const RgmOut o{PKVOL, CSSPR, ARSPR, NOBS};
  hipLaunchKernelGGL(k_range_model, dim3((unsigned)slices, (unsigned)G), dim3(RGM_THREADS), 0,
                     ctx->stream, in, T_m, N, Wm, min_obs, c4, (int)G, o);
  LAUNCH_CHECK(ctx, "k_range_model");
  return CSM_OK;
}

}  // extern "C"
