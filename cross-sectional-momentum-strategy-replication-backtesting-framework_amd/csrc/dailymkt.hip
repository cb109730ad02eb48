// dailymkt.hip -- signals of the daily returns against a daily market (rules V1..V6 in DESIGN.md
// 7): the equal-weight daily market return, each (month, asset)'s raw moment sums of its daily
// returns and the factor, and the window model on them -- daily beta, idiosyncratic and total
// volatility, skewness and the largest daily return (MAX).
//
//   k_daily_market    V1, V2.  The grid is (slice of DM_SLICE assets) x (chunk of consecutive day
//                     rows); a lane owns DM_PER assets of its slice, DM_THREADS apart (rule R1's
//                     layout, so a wave's loads of a row are contiguous), and carries each one's
//                     last priced price and its age in registers.  A chunk starts with the V1
//                     lead-in: a walk back over at most max_gap rows that only the lanes still
//                     without a price load.  Rows go in trips of DM_TRIP, the next trip's loads in
//                     flight; a lane adds its assets' returns in k order, the wave trees of a
//                     trip's days run together, and lane 0 of each wave leaves one (sum, count)
//                     pair per (day, slice, wave).  No barrier, no LDS, no atomic.
//   k_daily_market_finish  one thread per day adds the pairs in R1's order: a slice's four waves
//                     from 0.0, then the slices from 0.0.  The order is a function of N alone; the
//                     chunk length (csm_tune "dmkt_chunk_days") only decides how many workgroups
//                     there are.
//   k_daily_sums      V3.  k_month_stats's shape (daytrip.h): (slice of assets, one or two per
//                     lane) x (chunk of consecutive months), the same lead-in, FD[d] a uniform
//                     load, a month's sums flushed as the walk passes its end.  No barrier, no LDS,
//                     no state in memory (csm_tune "dsums_chunks").
//   k_daily_model     V4.  A lane per asset over (64 assets) x (chunk of consecutive months); every
//                     window's sums are added again from its oldest month, read from the V3 panels
//                     (a window is at most 12 months and its rows are L2 hits after the first
//                     read: an LDS ring of 12 x 60 B per lane would leave a CU three waves).  The
//                     chunk count (csm_tune "dmodel_chunks") only decides how many workgroups
//                     there are.
#include "csm_common.h"
#include "daytrip.h"
#include "scan.h"

#define DM_THREADS 256
#define DM_PER 8         // assets per lane (R1)
#define DM_SLICE (DM_THREADS * DM_PER)
#define DM_WAVES (DM_THREADS / 64)
#define DM_TRIP 4        // day rows per trip: two trips of eight assets are 128 VGPRs of buffers
#define DM_MAXGAP 32
#define DMD_THREADS 64
#define DMD_MAXW 12

// "dmkt_chunk_days": day rows per chunk of k_daily_market, 0 auto (dm_auto_chunk_days) | n >= 1
// "dsums_chunks":    month chunks of k_daily_sums, 0 auto (ds_auto_chunks) | n >= 1 that many
// "dmodel_chunks":   month chunks of k_daily_model, 0 auto, one month per chunk | n >= 1 that many
// (both clamped to T_m).  Every value gives the same bits.
static int g_tune_dmkt_chunk_days = 0;
static int g_tune_dsums_chunks = 0;
static int g_tune_dmodel_chunks = 0;
static const TuneKnob g_knobs[] = {
    {"dmkt_chunk_days", &g_tune_dmkt_chunk_days, [](int v) { return v >= 0; }},
    {"dsums_chunks", &g_tune_dsums_chunks, [](int v) { return v >= 0; }},
    {"dmodel_chunks", &g_tune_dmodel_chunks, [](int v) { return v >= 0; }},
};

// ------------------------------------------------------------------------------- V1
// One asset's last priced price (NaN: none within reach) and the rows since it, saturated at
// DM_MAXGAP (one more is past every max_gap).
struct DrLane {
  double lp;
  int age;
};

// Row d's return: x / lp - 1.0 when x is priced and the last priced row is at most max_gap rows
// back, else NaN.  A NaN x or lp makes the quotient NaN by itself; the division's operands are a
// loaded value and a select of loaded values.
__device__ __forceinline__ double dr_step(DrLane& s, double x, int max_gap) {
  const bool ok = !isnan_d(x);
  const int g = s.age + 1;
  const double r = g <= max_gap ? x / s.lp - 1.0 : qnan();
  s.lp = ok ? x : s.lp;
  s.age = ok ? 0 : (g > DM_MAXGAP ? DM_MAXGAP : g);
  return r;
}

// The lead-in of a chunk that starts at row d0: each asset's latest priced row among the max_gap
// rows before d0 (clipped at row 0).  An older one books no return in the chunk.  col(k) is the
// k-th asset's column, or -1.  Only the lanes still searching load; the walk ends when no lane of
// the wave is.
template <int CNT, class Col>
__device__ __forceinline__ void dr_lead_in(DrLane (&s)[CNT], const double* __restrict__ P,
                                           int64_t N, int64_t d0, int max_gap, Col col) {
#pragma unroll
  for (int k = 0; k < CNT; ++k) {
    s[k].lp = qnan();
    s[k].age = DM_MAXGAP;
  }
  for (int g = 1; g <= max_gap && d0 - g >= 0; ++g) {
    bool searching = false;
#pragma unroll
    for (int k = 0; k < CNT; ++k) {
      const int64_t a = col(k);
      if (a >= 0 && isnan_d(s[k].lp)) {
        const double x = P[(d0 - g) * N + a];
        if (!isnan_d(x)) {
          s[k].lp = x;
          s[k].age = g - 1;
        } else {
          searching = true;
        }
      }
    }
    if (!__any(searching)) break;
  }
}

// ------------------------------------------------------------------------------- V2
// Rows [d, d + DM_TRIP) of the lane's DM_PER assets; rows from dB on and columns from N on are NaN.
__device__ __forceinline__ void dm_load(double (&x)[DM_TRIP][DM_PER], const double* __restrict__ P,
                                        int64_t N, int64_t a0, int64_t d, int64_t dB) {
#pragma unroll
  for (int i = 0; i < DM_TRIP; ++i) {
#pragma unroll
    for (int k = 0; k < DM_PER; ++k) {
      const int64_t a = a0 + (int64_t)k * DM_THREADS;
      x[i][k] = (d + i < dB && a < N) ? P[(d + i) * N + a] : qnan();
    }
  }
}

__global__ __launch_bounds__(DM_THREADS) void k_daily_market(
    const double* __restrict__ P, int64_t T_d, int64_t N, int max_gap, int64_t chunk,
    double* __restrict__ psum, int32_t* __restrict__ pcnt) {
  const int tid = threadIdx.x;
  const int64_t a0 = (int64_t)blockIdx.x * DM_SLICE + tid;
  const int64_t dA = (int64_t)blockIdx.y * chunk;   // (the host keeps dA < T_d)
  const int64_t dB = dA + chunk < T_d ? dA + chunk : T_d;
  DrLane s[DM_PER];
  dr_lead_in<DM_PER>(s, P, N, dA, max_gap, [&](int k) {
    const int64_t a = a0 + (int64_t)k * DM_THREADS;
    return a < N ? a : (int64_t)-1;
  });
  double cur[DM_TRIP][DM_PER], nxt[DM_TRIP][DM_PER];
  dm_load(cur, P, N, a0, dA, dB);
  for (int64_t d = dA; d < dB; d += DM_TRIP) {
    dm_load(nxt, P, N, a0, d + DM_TRIP, dB);
    double sm[DM_TRIP];
    int c[DM_TRIP];
#pragma unroll
    for (int i = 0; i < DM_TRIP; ++i) {
      sm[i] = 0.0;
      c[i] = 0;
#pragma unroll
      for (int k = 0; k < DM_PER; ++k) {
        const double r = dr_step(s[k], cur[i][k], max_gap);
        const bool ok = !isnan_d(r);
        sm[i] = ok ? sm[i] + r : sm[i];
        c[i] += __popcll(__ballot(ok));   // (uniform) the wave's count
      }
    }
    // the wave's halving tree (csm_common.h wave_tree's order), the trip's days side by side
#pragma unroll
    for (int h = 32; h > 0; h >>= 1) {
#pragma unroll
      for (int i = 0; i < DM_TRIP; ++i) sm[i] = sm[i] + __shfl_down(sm[i], h, 64);
    }
    if ((tid & 63) == 0) {
#pragma unroll
      for (int i = 0; i < DM_TRIP; ++i) {
        if (d + i < dB) {
          const int64_t o = ((d + i) * gridDim.x + blockIdx.x) * DM_WAVES + (tid >> 6);
          psum[o] = sm[i];
          pcnt[o] = c[i];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < DM_TRIP; ++i) {
#pragma unroll
      for (int k = 0; k < DM_PER; ++k) cur[i][k] = nxt[i][k];
    }
  }
}

// Day d's partial sums: each slice's waves in order from 0.0, then the slices in order from 0.0.
__global__ __launch_bounds__(64) void k_daily_market_finish(
    const double* __restrict__ psum, const int32_t* __restrict__ pcnt, int64_t T_d, int slices,
    int min_assets, double* __restrict__ MKTD, int32_t* __restrict__ NMD) {
  const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= T_d) return;
  double tot = 0.0;
  int c = 0;
  for (int i = 0; i < slices; ++i) {
    double sl = 0.0;
#pragma unroll
    for (int w = 0; w < DM_WAVES; ++w) {
      const int64_t o = (d * slices + i) * DM_WAVES + w;
      sl += psum[o];
      c += pcnt[o];
    }
    tot += sl;
  }
  MKTD[d] = c >= min_assets ? tot / (double)c : qnan();
  if (NMD) NMD[d] = c;
}

// The workspace: psum [T_d][slices][DM_WAVES] doubles, then pcnt the same ints.
static inline int64_t dm_slices(int64_t N) { return (N + DM_SLICE - 1) / DM_SLICE; }

// Auto chunk length: about eight (slice, chunk) workgroups per CU, no chunk shorter than 32 rows
// (a chunk's lead-in is one more dependent row load for most lanes, up to max_gap for a few).
// MI355X (profiles/r14/bench_dailymkt_sweep.log): 100,000 assets x 10,000 days 16 / 64 / 128 /
// 239 / 512 / 2,048 rows 3.32 / 2.05 / 1.87 / 1.90 / 1.82 / 2.50 ms (auto 239); 5,000 assets x
// 6,522 days 8 / 16 / 32 / 64 / 128 / 512 rows 0.188 / 0.139 / 0.126 / 0.131 / 0.178 / 0.586 ms
// (auto 32)
static inline int64_t dm_auto_chunk_days(const csm_ctx* ctx, int64_t slices, int64_t T_d) {
  const int64_t want = (int64_t)8 * (ctx->n_cu > 0 ? ctx->n_cu : 256);
  const int64_t chunks = (want + slices - 1) / slices;
  const int64_t days = (T_d + chunks - 1) / chunks;
  return days < 32 ? 32 : days;
}

// ------------------------------------------------------------------------------- V3
// One asset's sums of the month being walked.
struct DsAcc {
  double sr, sf, srr, sff, srf, sr3, rmax;
  int no;
};

__device__ __forceinline__ void ds_reset(DsAcc& s) {
  s.sr = s.sf = s.srr = s.sff = s.srf = s.sr3 = 0.0;
  s.rmax = qnan();
  s.no = 0;
}

// One day row: the V1 state moves whatever f is; the sums take the row iff r and f are not NaN.
__device__ __forceinline__ void ds_step(DsAcc& s, DrLane& l, double x, double f, int max_gap) {
  const double r = dr_step(l, x, max_gap);
  const bool obs = !isnan_d(r) && !isnan_d(f);
  const double rr = r * r;
  s.no += obs ? 1 : 0;
  s.sr = obs ? s.sr + r : s.sr;
  s.sf = obs ? s.sf + f : s.sf;
  s.srr = obs ? s.srr + rr : s.srr;
  s.sff = obs ? s.sff + f * f : s.sff;
  s.srf = obs ? s.srf + r * f : s.srf;
  s.sr3 = obs ? s.sr3 + rr * r : s.sr3;
  s.rmax = (obs && !(r <= s.rmax)) ? r : s.rmax;   // (NaN rmax: the first observation)
}

struct DsOut {
  int32_t* NO;
  double *SR, *SF, *SRR, *SFF, *SRF, *SR3, *RMAX;
};

template <int VEC>
__device__ __forceinline__ void ds_flush(const DsAcc (&s)[VEC], int64_t o, const DsOut& out) {
  if (VEC == 2) {
    *reinterpret_cast<int2*>(out.NO + o) = make_int2(s[0].no, s[VEC - 1].no);
    store_pair(out.SR + o, s[0].sr, s[VEC - 1].sr);
    store_pair(out.SF + o, s[0].sf, s[VEC - 1].sf);
    store_pair(out.SRR + o, s[0].srr, s[VEC - 1].srr);
    store_pair(out.SFF + o, s[0].sff, s[VEC - 1].sff);
    store_pair(out.SRF + o, s[0].srf, s[VEC - 1].srf);
    if (out.SR3) store_pair(out.SR3 + o, s[0].sr3, s[VEC - 1].sr3);
    if (out.RMAX) store_pair(out.RMAX + o, s[0].rmax, s[VEC - 1].rmax);
  } else {
    out.NO[o] = s[0].no;
    out.SR[o] = s[0].sr;
    out.SF[o] = s[0].sf;
    out.SRR[o] = s[0].srr;
    out.SFF[o] = s[0].sff;
    out.SRF[o] = s[0].srf;
    if (out.SR3) out.SR3[o] = s[0].sr3;
    if (out.RMAX) out.RMAX[o] = s[0].rmax;
  }
}

// FD[d .. d + MS_TRIP) (uniform); NaN from dB on.
__device__ __forceinline__ void ds_fload(double (&f)[MS_TRIP], const double* __restrict__ FD,
                                         int64_t d, int64_t dB) {
#pragma unroll
  for (int i = 0; i < MS_TRIP; ++i) f[i] = d + i < dB ? FD[d + i] : qnan();
}

template <int VEC>
__global__ __launch_bounds__(MS_THREADS) void k_daily_sums(
    const double* __restrict__ P, const double* __restrict__ FD, int64_t T_d, int64_t N,
    const int64_t* __restrict__ ms, int T_m, int G, int max_gap, DsOut out) {
  const int64_t a = ((int64_t)blockIdx.x * MS_THREADS + threadIdx.x) * VEC;
  if (a >= N) return;   // (no barrier anywhere below)
  int m0, m1;
  chunk_range(T_m, G, (int)blockIdx.y, m0, m1);   // G <= T_m: at least one month
  // the chunk's day rows and month ends, clipped as k_month_stats clips them
  const int64_t dA = ms_clip(ms[m0], 0, T_d), dB = ms_clip(ms[m1], dA, T_d);
  int m = m0;
  int64_t nb = ms_clip(ms[m0 + 1], dA, dB);   // end of month m
  DrLane lane[VEC];
  dr_lead_in<VEC>(lane, P, N, dA, max_gap, [&](int k) { return a + k; });
  DsAcc acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) ds_reset(acc[k]);
  auto next_month = [&]() {   // (uniform) month m is complete; the V1 state runs on
    ds_flush<VEC>(acc, (int64_t)m * N + a, out);
#pragma unroll
    for (int k = 0; k < VEC; ++k) ds_reset(acc[k]);
    ++m;
    nb = m < m1 ? ms_clip(ms[m + 1], dA, dB) : dB;
  };
  double cur[MS_TRIP][VEC], nxt[MS_TRIP][VEC], fc[MS_TRIP], fn[MS_TRIP];
  ms_load<VEC>(cur, P, N, a, dA, dB);
  ds_fload(fc, FD, dA, dB);
  for (int64_t d = dA; d < dB; d += MS_TRIP) {
    ms_load<VEC>(nxt, P, N, a, d + MS_TRIP, dB);
    ds_fload(fn, FD, d + MS_TRIP, dB);
    if (d + MS_TRIP <= nb) {   // (uniform) the trip lies inside month m: one straight block
#pragma unroll
      for (int i = 0; i < MS_TRIP; ++i) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) ds_step(acc[k], lane[k], cur[i][k], fc[i], max_gap);
      }
    } else {
#pragma unroll
      for (int i = 0; i < MS_TRIP; ++i) {
        while (m < m1 && d + i >= nb) next_month();   // (zero-length months: several)
#pragma unroll
        for (int k = 0; k < VEC; ++k) ds_step(acc[k], lane[k], cur[i][k], fc[i], max_gap);
      }
    }
#pragma unroll
    for (int i = 0; i < MS_TRIP; ++i) {
      fc[i] = fn[i];
#pragma unroll
      for (int k = 0; k < VEC; ++k) cur[i][k] = nxt[i][k];
    }
  }
  while (m < m1) next_month();   // the last month, and whatever zero-length months follow it
}

// Auto chunk count: about eight (slice, chunk) workgroups per CU and no chunk shorter than three
// months.  Unlike k_month_stats, whose finest chunking is its fastest, a chunk here pays a lead-in
// (a dependent row load before its first trip) and fills a deeper pipeline (192 VGPRs with two
// assets per lane, two waves per SIMD).  MI355X (profiles/r14/bench_dailymkt_sweep.log):
// 100,000 assets x 461 months 1 / 11 / 88 / 461 chunks 3.94 / 2.37 / 2.55 / 3.62 ms (auto 11);
// 5,000 assets x 300 months 1 / 13 / 103 / 300 chunks 2.17 / 0.212 / 0.128 / 0.160 ms (auto 100)
static inline int ds_auto_chunks(const csm_ctx* ctx, int64_t slices, int T_m) {
  const int64_t want = (int64_t)8 * (ctx->n_cu > 0 ? ctx->n_cu : 256);
  int64_t G = (want + slices - 1) / slices;
  const int64_t most = T_m / 3 > 0 ? T_m / 3 : 1;
  if (G > most) G = most;
  return (int)G;
}

// ------------------------------------------------------------------------------- V4
struct DmdIn {
  const int32_t* NO;
  const double *SR, *SF, *SRR, *SFF, *SRF, *SR3, *RMAX;
};
struct DmdOut {
  double *DBETA, *DIVOL, *DTVOL, *DSKEW, *DMAX;
  int32_t* NOBS;
};

__global__ __launch_bounds__(DMD_THREADS) void k_daily_model(DmdIn in, int T_m, int64_t N, int Wm,
                                                            int min_obs, int G, DmdOut o) {
  const int64_t a = (int64_t)blockIdx.x * DMD_THREADS + threadIdx.x;
  if (a >= N) return;
  int m0, m1;
  chunk_range(T_m, G, (int)blockIdx.y, m0, m1);   // G <= T_m: at least one month
  const double NaN = qnan();
  // (uniform) the sums somebody reads: a window is re-read from L2 every month, so a panel no
  // requested output depends on is not loaded (its sum stays 0.0 and feeds nothing written)
  const bool needb = o.DBETA || o.DIVOL;                       // SF, SFF, SRF
  const bool needrr = o.DIVOL || o.DTVOL || o.DSKEW;           // SRR
  const bool needr = needb || needrr;                          // SR
  const bool need3 = o.DSKEW != nullptr, needx = o.DMAX != nullptr;
  for (int t = m0; t < m1; ++t) {
    double beta = NaN, ivol = NaN, tvol = NaN, skew = NaN, dmax = NaN;
    int n = 0;
    if (t - Wm + 1 >= 0) {   // (uniform) a whole window, added oldest month first
      double sr = 0.0, sf = 0.0, srr = 0.0, sff = 0.0, srf = 0.0, sr3 = 0.0, mx = NaN;
#pragma unroll 4
      for (int j = t - Wm + 1; j <= t; ++j) {
        const int64_t oj = (int64_t)j * N + a;
        n += in.NO[oj];
        if (needr) sr += in.SR[oj];
        if (needrr) srr += in.SRR[oj];
        if (needb) {
          sf += in.SF[oj];
          sff += in.SFF[oj];
          srf += in.SRF[oj];
        }
        if (need3) sr3 += in.SR3[oj];
        if (needx) {
          const double x = in.RMAX[oj];
          mx = (!isnan_d(x) && !(x <= mx)) ? x : mx;
        }
      }
      const double nf = (double)n;
      const double mr = sr / nf, mf = sf / nf;
      const double cff = sff - sf * mf, crf = srf - sr * mf, crr = srr - sr * mr;
      const bool enough = n >= min_obs;
      const bool def = enough && cff > 0.0;
      if (def) {
        beta = crf / cff;
        if (n >= 3) {
          const double q = crr - beta * crf;
          ivol = sqrt((q < 0.0 ? 0.0 : q) / (nf - 2.0));
        }
      }
      if (enough && n >= 2 && crr >= 0.0) tvol = sqrt(crr / (nf - 1.0));
      if (need3 && enough && n >= 3) {
        const double v = crr / nf;
        const double m3 = (sr3 - (3.0 * mr) * srr + ((2.0 * sr) * mr) * mr) / nf;
        if (v > 0.0) skew = m3 / (v * sqrt(v));
      }
      if (enough) dmax = mx;
    }
    const int64_t ot = (int64_t)t * N + a;
    if (o.DBETA) o.DBETA[ot] = beta;
    if (o.DIVOL) o.DIVOL[ot] = ivol;
    if (o.DTVOL) o.DTVOL[ot] = tvol;
    if (o.DSKEW) o.DSKEW[ot] = skew;
    if (o.DMAX) o.DMAX[ot] = dmax;
    if (o.NOBS) o.NOBS[ot] = n;
  }
}


extern "C" {

int csm_tune_dailymkt(const char* key, int value) { return tune_set(g_knobs, key, value); }

int64_t csm_daily_market_workspace(int64_t T_d, int64_t N) {
  if (T_d < 1 || N < 1 || T_d > INT32_MAX || T_d > ((int64_t)1 << 40) / N) return 0;
  return T_d * dm_slices(N) * DM_WAVES * (int64_t)(sizeof(double) + sizeof(int32_t));
}

int csm_daily_market(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N, int32_t max_gap,
                     int32_t min_assets, double* MKTD, int32_t* NMD, void* workspace) {
  int r = prep(ctx);
  if (r) return r;
  if (!P || !MKTD || !workspace || T_d < 1 || N < 1 || T_d > INT32_MAX ||
      T_d > ((int64_t)1 << 40) / N || !aligned8(workspace))
    return set_err(ctx, CSM_E_INVAL, "csm_daily_market: bad arguments (T_d=%lld N=%lld)",
                   (long long)T_d, (long long)N);
  if (max_gap < 1 || max_gap > DM_MAXGAP)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_market: max_gap=%d is outside [1, %d]", max_gap,
                   DM_MAXGAP);
  if (min_assets < 1)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_market: min_assets=%d must be at least 1",
                   min_assets);
  const int64_t slices = dm_slices(N);
  int64_t chunk = g_tune_dmkt_chunk_days > 0 ? g_tune_dmkt_chunk_days
                                              : dm_auto_chunk_days(ctx, slices, T_d);
  if (chunk > T_d) chunk = T_d;
  if ((T_d + chunk - 1) / chunk > 65535) chunk = (T_d + 65534) / 65535;   // (grid.y)
  const int64_t chunks = (T_d + chunk - 1) / chunk;
  double* psum = (double*)workspace;
  int32_t* pcnt = (int32_t*)(psum + T_d * slices * DM_WAVES);
  hipLaunchKernelGGL(k_daily_market, dim3((unsigned)slices, (unsigned)chunks), dim3(DM_THREADS),
                     0, ctx->stream, P, T_d, N, max_gap, chunk, psum, pcnt);
  LAUNCH_CHECK(ctx, "k_daily_market");
  hipLaunchKernelGGL(k_daily_market_finish, dim3((unsigned)((T_d + 63) / 64)), dim3(64), 0,
                     ctx->stream, psum, pcnt, T_d, (int)slices, min_assets, MKTD, NMD);
  LAUNCH_CHECK(ctx, "k_daily_market_finish");
  return CSM_OK;
}

int csm_daily_sums(csm_ctx* ctx, const double* P, const double* FD, int64_t T_d, int64_t N,
                   const int64_t* month_start, int32_t T_m, int32_t max_month_days,
                   int32_t max_gap, int32_t* NO, double* SR, double* SF, double* SRR, double* SFF,
                   double* SRF, double* SR3, double* RMAX) {
  int r = prep(ctx);
  if (r) return r;
  if (!P || !FD || !month_start || !NO || !SR || !SF || !SRR || !SFF || !SRF || T_d < 1 ||
      N < 1 || T_m < 1 || T_d > ((int64_t)1 << 40) / N)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_sums: bad arguments (T_d=%lld N=%lld T_m=%d)",
                   (long long)T_d, (long long)N, T_m);
  if (max_month_days < 1 || max_month_days > 32)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_sums: max_month_days=%d is outside [1, 32]",
                   max_month_days);
  if (max_gap < 1 || max_gap > DM_MAXGAP)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_sums: max_gap=%d is outside [1, %d]", max_gap,
                   DM_MAXGAP);
  const bool v2 = (N % 2 == 0) && aligned16(P) && aligned8(NO) && aligned16(SR) &&
                  aligned16(SF) && aligned16(SRR) && aligned16(SFF) && aligned16(SRF) &&
                  (!SR3 || aligned16(SR3)) && (!RMAX || aligned16(RMAX));
  const int vec = v2 ? 2 : 1;
  const int64_t slices = (N + (int64_t)MS_THREADS * vec - 1) / ((int64_t)MS_THREADS * vec);
  int64_t G = g_tune_dsums_chunks > 0 ? g_tune_dsums_chunks : ds_auto_chunks(ctx, slices, T_m);
  if (G > T_m) G = T_m;
  if (G > 65535) G = 65535;   // (grid.y)
  const int g = (int)G;
  const dim3 grid((unsigned)slices, (unsigned)g);
  const DsOut out{NO, SR, SF, SRR, SFF, SRF, SR3, RMAX};
  if (v2)
    hipLaunchKernelGGL(k_daily_sums<2>, grid, dim3(MS_THREADS), 0, ctx->stream, P, FD, T_d, N,
                       month_start, T_m, g, max_gap, out);
  else
    hipLaunchKernelGGL(k_daily_sums<1>, grid, dim3(MS_THREADS), 0, ctx->stream, P, FD, T_d, N,
                       month_start, T_m, g, max_gap, out);
  LAUNCH_CHECK(ctx, "k_daily_sums");
  return CSM_OK;
}

int csm_daily_model(csm_ctx* ctx, const int32_t* NO, const double* SR, const double* SF,
                    const double* SRR, const double* SFF, const double* SRF, const double* SR3,
                    const double* RMAX, int32_t T_m, int64_t N, int32_t Wm, int32_t min_obs,
                    double* DBETA, double* DIVOL, double* DTVOL, double* DSKEW, double* DMAX,
                    int32_t* NOBS) {
  int r = prep(ctx);
  if (r) return r;
  if (!NO || !SR || !SF || !SRR || !SFF || !SRF || bad_panel(T_m, N))
    return set_err(ctx, CSM_E_INVAL, "csm_daily_model: bad arguments (T_m=%d N=%lld)", T_m,
                   (long long)N);
  if (!DBETA && !DIVOL && !DTVOL && !DSKEW && !DMAX && !NOBS)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_model: no output requested");
  if (Wm < 1 || Wm > DMD_MAXW)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_model: Wm=%d is outside [1, %d]", Wm, DMD_MAXW);
  if (min_obs < 2)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_model: min_obs=%d must be at least 2", min_obs);
  if ((DSKEW && !SR3) || (DMAX && !RMAX))
    return set_err(ctx, CSM_E_INVAL, "csm_daily_model: DSKEW needs SR3 and DMAX needs RMAX");
  const int64_t slices = (N + DMD_THREADS - 1) / DMD_THREADS;
  // a chunk needs no warm-up, and finer measured faster or equal at every step on both widths
  // (DESIGN.md 7, V-rules): auto is one month per chunk
  int64_t G = g_tune_dmodel_chunks;
  if (G < 1 || G > T_m) G = T_m;
  if (G > 65535) G = 65535;   // (grid.y)
  const DmdIn in{NO, SR, SF, SRR, SFF, SRF, SR3, RMAX};
  const DmdOut o{DBETA, DIVOL, DTVOL, DSKEW, DMAX, NOBS};
  hipLaunchKernelGGL(k_daily_model, dim3((unsigned)slices, (unsigned)G), dim3(DMD_THREADS), 0,
                     ctx->stream, in, T_m, N, Wm, min_obs, (int)G, o);
  LAUNCH_CHECK(ctx, "k_daily_model");
  return CSM_OK;
}

}  // extern "C"
