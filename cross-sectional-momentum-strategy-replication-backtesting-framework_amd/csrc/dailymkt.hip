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
//   k_daily_sums      V3.  The month walk of daytrip.h, one or two assets per lane: k_daily_market's
//                     lead-in at each chunk's start, FD[d] a uniform load (csm_tune
//                     "dsums_chunks").
//   k_daily_fsums     MF6.  The same on KF factors (a template on KF = 1..4): a day row's KF factor
//                     values and their pair products are uniform, computed once per row; two
//                     assets per lane up to DF_PAIR_MAXKF factors, one past it (csm_tune
//                     "dfsums_chunks").
//   k_daily_fmodel    MF7.  k_daily_model's shape on the MF6 panels; fsolve.h solves each
//                     window's normal equations (csm_tune "dfmodel_chunks").
//   k_daily_model     V4.  A lane per asset over (64 assets) x (chunk of consecutive months); every
//                     window's sums are added again from its oldest month, read from the V3 panels
//                     (a window is at most 12 months and its rows are L2 hits after the first
//                     read: an LDS ring of 12 x 60 B per lane would leave a CU three waves).  The
//                     chunk count (csm_tune "dmodel_chunks") only decides how many workgroups
//                     there are.
#include "csm_common.h"
#include "dayret.h"
#include "daytrip.h"
#include "fsolve.h"
#include "scan.h"

#define DM_THREADS 256
#define DM_PER 8         // assets per lane (R1)
#define DM_SLICE (DM_THREADS * DM_PER)
#define DM_WAVES (DM_THREADS / 64)
#define DM_TRIP 4        // day rows per trip: two trips of eight assets are 128 VGPRs of buffers
#define DMD_THREADS 64
#define DMD_MAXW 12
// k_daily_fsums: the largest KF that takes two assets per lane and loads its factor rows a trip
// ahead, as k_daily_sums does.  Past it the 3 + 2 KF + KF (KF + 1) / 2 accumulators per asset, twice
// over, and two trips of KF factor rows fill the 256 VGPRs and leave a SIMD one wave, so a lane
// takes one asset and a trip loads its own factor rows.  MI355X, 100,000 x 10,000 days / 5,000 x
// 6,522 days, ms (profiles/r15/bench_fsums_*.log; k_daily_sums on six panels 2.19 / 0.120):
//   KF  paired, ahead   paired, own rows   one per lane, ahead   one per lane, own rows
//   1   2.15 / 0.110    --                 2.28 / 0.110          --
//   2   2.86 / 0.136    --                 3.15 / 0.122          --
//   3   6.20 / 0.275    4.95 / 0.232       4.24 / 0.168          3.91 / 0.158
//   4   8.18 / 0.331    7.12 / 0.286       6.47 / 0.254          5.10 / 0.211
#define DF_PAIR_MAXKF 2

// "dmkt_chunk_days": day rows per chunk of k_daily_market, 0 auto (dm_auto_chunk_days) | n >= 1
// "dsums_chunks":    month chunks of k_daily_sums, 0 auto (scan.h auto_chunks) | n >= 1 that many
// "dmodel_chunks":   month chunks of k_daily_model, 0 auto, one month per chunk | n >= 1 that many
// (both clamped to T_m).  Every value gives the same bits.
// "dfsums_chunks" / "dfmodel_chunks": the same two for k_daily_fsums and k_daily_fmodel.
static int g_tune_dmkt_chunk_days = 0;
static int g_tune_dsums_chunks = 0;
static int g_tune_dmodel_chunks = 0;
static int g_tune_dfsums_chunks = 0;
static int g_tune_dfmodel_chunks = 0;
static const TuneKnob g_knobs[] = {
    {"dmkt_chunk_days", &g_tune_dmkt_chunk_days, [](int v) { return v >= 0; }},
    {"dsums_chunks", &g_tune_dsums_chunks, [](int v) { return v >= 0; }},
    {"dmodel_chunks", &g_tune_dmodel_chunks, [](int v) { return v >= 0; }},
    {"dfsums_chunks", &g_tune_dfsums_chunks, [](int v) { return v >= 0; }},
    {"dfmodel_chunks", &g_tune_dfmodel_chunks, [](int v) { return v >= 0; }},
};

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

// k_daily_sums's walker (daytrip.h): the V1 lead-in, P's rows and FD's, which are uniform.
template <int VEC>
struct DsWalker {
  const double* __restrict__ P;
  const double* __restrict__ FD;
  int64_t N, a;
  int max_gap;
  DsOut out;
  DrLane lane[VEC];
  DsAcc acc[VEC];
  struct Rows {
    double x[MS_TRIP][VEC], f[MS_TRIP];
  };

  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int k = 0; k < VEC; ++k) ds_reset(acc[k]);
  }
  __device__ __forceinline__ void begin(int64_t dA) {
    dr_lead_in<VEC>(lane, P, N, dA, max_gap, [&](int k) { return a + k; });
    reset();
  }
  __device__ __forceinline__ void load(Rows& r, int64_t d, int64_t dB) const {
    trip_load<MS_TRIP, VEC>(r.x, P, N, a, d, dB, absent_val());
    ds_fload(r.f, FD, d, dB);
  }
  __device__ __forceinline__ void own(Rows&, int64_t, int64_t) const {}
  __device__ __forceinline__ void step(const Rows& r, int i) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) ds_step(acc[k], lane[k], r.x[i][k], r.f[i], max_gap);
  }
  __device__ __forceinline__ void flush(int m) {   // the V1 state runs on
    ds_flush<VEC>(acc, (int64_t)m * N + a, out);
    reset();
  }
};

template <int VEC>
__global__ __launch_bounds__(MS_THREADS) void k_daily_sums(
    const double* __restrict__ P, const double* __restrict__ FD, int64_t T_d, int64_t N,
    const int64_t* __restrict__ ms, int T_m, int G, int max_gap, DsOut out) {
  const int64_t a = ((int64_t)blockIdx.x * MS_THREADS + threadIdx.x) * VEC;
  if (a >= N) return;   // (no barrier anywhere below)
  DsWalker<VEC> w{P, FD, N, a, max_gap, out};
  month_walk<MS_TRIP>(w, ms, T_m, G, T_d);
}

// ------------------------------------------------------------------------------- MF6
// One asset's sums of the month being walked, on KF factors.
template <int KF>
struct DfAcc {
  double sr, srr, sf[KF], srf[KF], sff[KF * (KF + 1) / 2];
  int no;
};

template <int KF>
__device__ __forceinline__ void df_reset(DfAcc<KF>& s) {
  s.sr = s.srr = 0.0;
#pragma unroll
  for (int c = 0; c < KF; ++c) s.sf[c] = s.srf[c] = 0.0;
#pragma unroll
  for (int p = 0; p < fs_pairs(KF); ++p) s.sff[p] = 0.0;
  s.no = 0;
}

// One day row's factor values, whether all KF are there, and their pair products: the same for
// every asset, so computed once per row.
template <int KF>
struct DfRow {
  double f[KF], ff[KF * (KF + 1) / 2];
  bool ok;
};

template <int KF>
__device__ __forceinline__ DfRow<KF> df_row(const double (&f)[KF]) {
  DfRow<KF> w;
  w.ok = true;
#pragma unroll
  for (int c = 0; c < KF; ++c) {
    w.f[c] = f[c];
    w.ok = w.ok && !isnan_d(f[c]);
  }
#pragma unroll
  for (int c = 0; c < KF; ++c) {
#pragma unroll
    for (int e = c; e < KF; ++e) w.ff[fs_pair(KF, c, e)] = f[c] * f[e];
  }
  return w;
}

// One day row of one asset: the V1 state moves whatever the factor row is; the sums take the row
// iff r is not NaN and the day has a factor row.
template <int KF>
__device__ __forceinline__ void df_step(DfAcc<KF>& s, DrLane& l, double x, const DfRow<KF>& w,
                                        int max_gap) {
  const double r = dr_step(l, x, max_gap);
  const bool obs = !isnan_d(r) && w.ok;
  s.no += obs ? 1 : 0;
  s.sr = obs ? s.sr + r : s.sr;
  s.srr = obs ? s.srr + r * r : s.srr;
#pragma unroll
  for (int c = 0; c < KF; ++c) {
    s.sf[c] = obs ? s.sf[c] + w.f[c] : s.sf[c];
    s.srf[c] = obs ? s.srf[c] + r * w.f[c] : s.srf[c];
  }
#pragma unroll
  for (int p = 0; p < fs_pairs(KF); ++p) s.sff[p] = obs ? s.sff[p] + w.ff[p] : s.sff[p];
}

struct DfOut {
  int32_t* NO;
  double *SR, *SRR;   // [T_m][N]
  double *SF, *SRF;   // [KF][T_m][N]
  double* SFF;        // [KF (KF + 1) / 2][T_m][N]
};

template <int VEC>
__device__ __forceinline__ void df_store(double* p, double lo, double hi) {
  if (VEC == 2)
    store_pair(p, lo, hi);
  else
    p[0] = lo;
}

// o: the (month, asset) cell; plane: T_m * N, the stride between a panel's factor planes.
template <int KF, int VEC>
__device__ __forceinline__ void df_flush(const DfAcc<KF> (&s)[VEC], int64_t o, int64_t plane,
                                         const DfOut& out) {
  if (VEC == 2)
    *reinterpret_cast<int2*>(out.NO + o) = make_int2(s[0].no, s[VEC - 1].no);
  else
    out.NO[o] = s[0].no;
  df_store<VEC>(out.SR + o, s[0].sr, s[VEC - 1].sr);
  df_store<VEC>(out.SRR + o, s[0].srr, s[VEC - 1].srr);
#pragma unroll
  for (int c = 0; c < KF; ++c) {
    df_store<VEC>(out.SF + c * plane + o, s[0].sf[c], s[VEC - 1].sf[c]);
    df_store<VEC>(out.SRF + c * plane + o, s[0].srf[c], s[VEC - 1].srf[c]);
  }
#pragma unroll
  for (int p = 0; p < fs_pairs(KF); ++p)
    df_store<VEC>(out.SFF + p * plane + o, s[0].sff[p], s[VEC - 1].sff[p]);
}

// FD[d .. d + MS_TRIP)[KF] (uniform); NaN from dB on.
template <int KF>
__device__ __forceinline__ void df_fload(double (&f)[MS_TRIP][KF], const double* __restrict__ FD,
                                         int64_t d, int64_t dB) {
#pragma unroll
  for (int i = 0; i < MS_TRIP; ++i) {
#pragma unroll
    for (int c = 0; c < KF; ++c) f[i][c] = d + i < dB ? FD[(d + i) * KF + c] : qnan();
  }
}

// k_daily_fsums's walker (daytrip.h): k_daily_sums's on KF factors.  Up to DF_PAIR_MAXKF factors
// the factor rows are loaded a trip ahead with the prices; past it a trip loads its own.
template <int KF, int VEC>
struct DfWalker {
  static constexpr bool AHEAD = KF <= DF_PAIR_MAXKF;
  const double* __restrict__ P;
  const double* __restrict__ FD;
  int64_t N, a, plane;   // plane: T_m * N
  int max_gap;
  DfOut out;
  DrLane lane[VEC];
  DfAcc<KF> acc[VEC];
  struct Rows {
    double x[MS_TRIP][VEC];
    double f[MS_TRIP][KF] = {};   // (own() writes them when load() does not)
  };

  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int k = 0; k < VEC; ++k) df_reset<KF>(acc[k]);
  }
  __device__ __forceinline__ void begin(int64_t dA) {
    dr_lead_in<VEC>(lane, P, N, dA, max_gap, [&](int k) { return a + k; });
    reset();
  }
  __device__ __forceinline__ void load(Rows& r, int64_t d, int64_t dB) const {
    trip_load<MS_TRIP, VEC>(r.x, P, N, a, d, dB, absent_val());
    if (AHEAD) df_fload<KF>(r.f, FD, d, dB);
  }
  __device__ __forceinline__ void own(Rows& r, int64_t d, int64_t dB) const {
    if (!AHEAD) df_fload<KF>(r.f, FD, d, dB);
  }
  __device__ __forceinline__ void step(const Rows& r, int i) {
    const DfRow<KF> w = df_row<KF>(r.f[i]);
#pragma unroll
    for (int k = 0; k < VEC; ++k) df_step<KF>(acc[k], lane[k], r.x[i][k], w, max_gap);
  }
  __device__ __forceinline__ void flush(int m) {   // the V1 state runs on
    df_flush<KF, VEC>(acc, (int64_t)m * N + a, plane, out);
    reset();
  }
};

template <int KF, int VEC>
__global__ __launch_bounds__(MS_THREADS) void k_daily_fsums(
    const double* __restrict__ P, const double* __restrict__ FD, int64_t T_d, int64_t N,
    const int64_t* __restrict__ ms, int T_m, int G, int max_gap, DfOut out) {
  const int64_t a = ((int64_t)blockIdx.x * MS_THREADS + threadIdx.x) * VEC;
  if (a >= N) return;   // (no barrier anywhere below)
  DfWalker<KF, VEC> w{P, FD, N, a, (int64_t)T_m * N, max_gap, out};
  month_walk<MS_TRIP>(w, ms, T_m, G, T_d);
}

template <int KF>
static inline void df_launch(csm_ctx* ctx, bool v2, dim3 grid, const double* P, const double* FD,
                             int64_t T_d, int64_t N, const int64_t* ms, int T_m, int G,
                             int max_gap, const DfOut& out) {
  if constexpr (KF <= DF_PAIR_MAXKF) {
    if (v2) {
      hipLaunchKernelGGL((k_daily_fsums<KF, 2>), grid, dim3(MS_THREADS), 0, ctx->stream, P, FD,
                         T_d, N, ms, T_m, G, max_gap, out);
      return;
    }
  }
  hipLaunchKernelGGL((k_daily_fsums<KF, 1>), grid, dim3(MS_THREADS), 0, ctx->stream, P, FD, T_d,
                     N, ms, T_m, G, max_gap, out);
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

// ------------------------------------------------------------------------------- MF7
struct DfmIn {
  const int32_t* NO;
  const double *SR, *SRR, *SF, *SRF, *SFF;
};
struct DfmOut {
  double* DBETA;   // [KF][T_m][N]
  double *DALPHA, *DIVOL, *DR2;
  int32_t* NOBS;
};

// k_daily_model's shape on KF factors.
template <int KF>
__global__ __launch_bounds__(DMD_THREADS) void k_daily_fmodel(DfmIn in, int T_m, int64_t N, int Wm,
                                                             int min_obs, int G, DfmOut o) {
  constexpr int NP = fs_pairs(KF);
  const int64_t a = (int64_t)blockIdx.x * DMD_THREADS + threadIdx.x;
  if (a >= N) return;
  int m0, m1;
  chunk_range(T_m, G, (int)blockIdx.y, m0, m1);   // G <= T_m: at least one month
  const double NaN = qnan();
  const int64_t plane = (int64_t)T_m * N;
  // (uniform) the sums somebody reads: NOBS alone needs NO only
  const bool needrr = o.DIVOL || o.DR2;                       // SRR
  const bool needb = o.DBETA || o.DALPHA || needrr;           // SR, SF, SRF, SFF
  for (int t = m0; t < m1; ++t) {
    double beta[KF], alpha = NaN, ivol = NaN, r2 = NaN;
#pragma unroll
    for (int c = 0; c < KF; ++c) beta[c] = NaN;
    int n = 0;
    if (t - Wm + 1 >= 0) {   // (uniform) a whole window, added oldest month first
      double sr = 0.0, srr = 0.0, sf[KF], srf[KF], sff[NP];
#pragma unroll
      for (int c = 0; c < KF; ++c) sf[c] = srf[c] = 0.0;
#pragma unroll
      for (int p = 0; p < NP; ++p) sff[p] = 0.0;
#pragma unroll 2
      for (int j = t - Wm + 1; j <= t; ++j) {
        const int64_t oj = (int64_t)j * N + a;
        n += in.NO[oj];
        if (needrr) srr += in.SRR[oj];
        if (needb) {
          sr += in.SR[oj];
#pragma unroll
          for (int c = 0; c < KF; ++c) {
            sf[c] += in.SF[c * plane + oj];
            srf[c] += in.SRF[c * plane + oj];
          }
#pragma unroll
          for (int p = 0; p < NP; ++p) sff[p] += in.SFF[p * plane + oj];
        }
      }
      const double nf = (double)n;
      const double mr = sr / nf;
      double mf[KF], A[NP], b[KF], g[KF];
#pragma unroll
      for (int c = 0; c < KF; ++c) mf[c] = sf[c] / nf;
#pragma unroll
      for (int c = 0; c < KF; ++c) {
#pragma unroll
        for (int e = c; e < KF; ++e)
          A[fs_pair(KF, c, e)] = sff[fs_pair(KF, c, e)] - sf[c] * mf[e];
        b[c] = srf[c] - sr * mf[c];
      }
      const double crr = srr - sr * mr;
      const bool solved = fs_solve<KF>(A, b, g);
      if (n >= min_obs && solved) {
        alpha = mr;
        double q = crr;
#pragma unroll
        for (int c = 0; c < KF; ++c) {
          beta[c] = g[c];
          alpha = alpha - g[c] * mf[c];
          q = q - g[c] * b[c];
        }
        q = q < 0.0 ? 0.0 : q;
        if (n >= KF + 2) ivol = sqrt(q / (nf - (KF + 1.0)));
        if (crr > 0.0) r2 = 1.0 - q / crr;
      }
    }
    const int64_t ot = (int64_t)t * N + a;
    if (o.DBETA) {
#pragma unroll
      for (int c = 0; c < KF; ++c) o.DBETA[c * plane + ot] = beta[c];
    }
    if (o.DALPHA) o.DALPHA[ot] = alpha;
    if (o.DIVOL) o.DIVOL[ot] = ivol;
    if (o.DR2) o.DR2[ot] = r2;
    if (o.NOBS) o.NOBS[ot] = n;
  }
}

template <int KF>
static inline void dfm_launch(csm_ctx* ctx, dim3 grid, const DfmIn& in, int T_m, int64_t N, int Wm,
                              int min_obs, int G, const DfmOut& o) {
  hipLaunchKernelGGL(k_daily_fmodel<KF>, grid, dim3(DMD_THREADS), 0, ctx->stream, in, T_m, N, Wm,
                     min_obs, G, o);
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
  // Auto chunk count: about eight workgroups per CU (scan.h auto_chunks).  Unlike k_month_stats,
  // whose finest chunking is its fastest, a chunk here pays a lead-in (a dependent row load
  // before its first trip) and fills a deeper pipeline (two assets per lane leave a SIMD two
  // waves).  MI355X (profiles/r14/bench_dailymkt_sweep.log): 100,000 assets x 461 months 1 / 11 /
  // 88 / 461 chunks 3.94 / 2.37 / 2.55 / 3.62 ms (auto 11); 5,000 assets x 300 months 1 / 13 /
  // 103 / 300 chunks 2.17 / 0.212 / 0.128 / 0.160 ms (auto 100)
  const dim3 grid = month_grid(ctx, N, MS_THREADS * (v2 ? 2 : 1), g_tune_dsums_chunks, 8, T_m);
  const int g = (int)grid.y;
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

int csm_daily_fsums(csm_ctx* ctx, const double* P, const double* FD, int64_t T_d, int64_t N,
                    int32_t KF, const int64_t* month_start, int32_t T_m, int32_t max_month_days,
                    int32_t max_gap, int32_t* NO, double* SR, double* SRR, double* SF, double* SRF,
                    double* SFF) {
  int r = prep(ctx);
  if (r) return r;
  if (!P || !FD || !month_start || !NO || !SR || !SRR || !SF || !SRF || !SFF || T_d < 1 ||
      N < 1 || T_m < 1 || T_d > ((int64_t)1 << 40) / N)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_fsums: bad arguments (T_d=%lld N=%lld T_m=%d)",
                   (long long)T_d, (long long)N, T_m);
  if (KF < 1 || KF > FS_MAXKF)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_fsums: KF=%d is outside [1, %d]", KF, FS_MAXKF);
  if ((int64_t)T_m * fs_pairs(KF) > ((int64_t)1 << 40) / N)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_fsums: bad arguments (T_m=%d N=%lld KF=%d)", T_m,
                   (long long)N, KF);
  if (max_month_days < 1 || max_month_days > 32)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_fsums: max_month_days=%d is outside [1, 32]",
                   max_month_days);
  if (max_gap < 1 || max_gap > DM_MAXGAP)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_fsums: max_gap=%d is outside [1, %d]", max_gap,
                   DM_MAXGAP);
  const bool v2 = KF <= DF_PAIR_MAXKF && (N % 2 == 0) && aligned16(P) && aligned8(NO) &&
                  aligned16(SR) && aligned16(SRR) && aligned16(SF) && aligned16(SRF) &&
                  aligned16(SFF);
  // Auto chunk count: about 32 workgroups per CU in place of k_daily_sums's eight: the deeper
  // accumulator set leaves a CU fewer resident waves, and more, shorter chunks even the fill out.
  // MI355X (profiles/r15/bench_fsums_sweep.log), KF = 1 / KF = 4: 100,000 assets x 461 months 3 /
  // 6 / 12 / 30 / 100 chunks 2.65 / 2.14 / 2.06 / 1.97 / 2.16 ms and 5.26 / 5.09 / 4.65 / 4.48 /
  // 4.61 ms (auto 42 and 21: 2.21 and 4.57 ms in bench_factor.log, k_daily_sums 2.43 there; eight
  // per CU gave 11 and 6 chunks, 2.06 and 5.00 ms in the sweep's run); 5,000 assets x 300 months
  // 3 / 6 / 12 / 30 / 100 chunks 0.703 / 0.370 / 0.207 / 0.135 / 0.114 ms and 1.023 / 0.532 /
  // 0.288 / 0.259 / 0.216 ms (auto 100)
  const dim3 grid = month_grid(ctx, N, MS_THREADS * (v2 ? 2 : 1), g_tune_dfsums_chunks, 32, T_m);
  const int g = (int)grid.y;
  const DfOut out{NO, SR, SRR, SF, SRF, SFF};
  switch (KF) {
    case 1: df_launch<1>(ctx, v2, grid, P, FD, T_d, N, month_start, T_m, g, max_gap, out); break;
    case 2: df_launch<2>(ctx, v2, grid, P, FD, T_d, N, month_start, T_m, g, max_gap, out); break;
    case 3: df_launch<3>(ctx, v2, grid, P, FD, T_d, N, month_start, T_m, g, max_gap, out); break;
    default: df_launch<4>(ctx, v2, grid, P, FD, T_d, N, month_start, T_m, g, max_gap, out); break;
  }
  LAUNCH_CHECK(ctx, "k_daily_fsums");
  return CSM_OK;
}

int csm_daily_fmodel(csm_ctx* ctx, const int32_t* NO, const double* SR, const double* SRR,
                     const double* SF, const double* SRF, const double* SFF, int32_t T_m,
                     int64_t N, int32_t KF, int32_t Wm, int32_t min_obs, double* DBETA,
                     double* DALPHA, double* DIVOL, double* DR2, int32_t* NOBS) {
  int r = prep(ctx);
  if (r) return r;
  if (!NO || !SR || !SRR || !SF || !SRF || !SFF || bad_panel(T_m, N))
    return set_err(ctx, CSM_E_INVAL, "csm_daily_fmodel: bad arguments (T_m=%d N=%lld)", T_m,
                   (long long)N);
  if (KF < 1 || KF > FS_MAXKF)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_fmodel: KF=%d is outside [1, %d]", KF, FS_MAXKF);
  if ((int64_t)T_m * fs_pairs(KF) > ((int64_t)1 << 40) / N)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_fmodel: bad arguments (T_m=%d N=%lld KF=%d)", T_m,
                   (long long)N, KF);
  if (!DBETA && !DALPHA && !DIVOL && !DR2 && !NOBS)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_fmodel: no output requested");
  if (Wm < 1 || Wm > DMD_MAXW)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_fmodel: Wm=%d is outside [1, %d]", Wm, DMD_MAXW);
  if (min_obs < KF + 1)
    return set_err(ctx, CSM_E_INVAL, "csm_daily_fmodel: min_obs=%d must be at least KF+1=%d",
                   min_obs, KF + 1);
  const int64_t slices = (N + DMD_THREADS - 1) / DMD_THREADS;
  // auto is one month per chunk, csm_daily_model's rule: a chunk needs no warm-up.  MI355X
  // (profiles/r15/bench_factor_sweep.log), KF = 4, Wm = 1 / Wm = 12, 16 / 100 / T_m chunks:
  // 100,000 assets 1.75 / 1.69 / 1.67 ms and 14.18 / 12.14 / 12.01 ms; 5,000 assets 0.084 / 0.068 /
  // 0.073 ms and 0.480 / 0.486 / 0.464 ms
  int64_t G = g_tune_dfmodel_chunks;
  if (G < 1 || G > T_m) G = T_m;
  if (G > 65535) G = 65535;   // (grid.y)
  const DfmIn in{NO, SR, SRR, SF, SRF, SFF};
  const DfmOut o{DBETA, DALPHA, DIVOL, DR2, NOBS};
  const dim3 grid((unsigned)slices, (unsigned)G);
  switch (KF) {
    case 1: dfm_launch<1>(ctx, grid, in, T_m, N, Wm, min_obs, (int)G, o); break;
    case 2: dfm_launch<2>(ctx, grid, in, T_m, N, Wm, min_obs, (int)G, o); break;
    case 3: dfm_launch<3>(ctx, grid, in, T_m, N, Wm, min_obs, (int)G, o); break;
    default: dfm_launch<4>(ctx, grid, in, T_m, N, Wm, min_obs, (int)G, o); break;
  }
  LAUNCH_CHECK(ctx, "k_daily_fmodel");
  return CSM_OK;
}

}  // extern "C"
