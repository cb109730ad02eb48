// groups.hip -- within-group sorts (rules N1..N6 in DESIGN.md 7): exact qcut labels per (date,
// group), the groups' and the pooled decile means, and the groups' mean / standard deviation with
// the adjusted signals.  The work per date is a fixed number of sweeps of the row whatever
// n_groups is.
//
//   k_gpart    N1.  One workgroup per date; each of its GP_WAVES waves owns one contiguous chunk
//              of the row (gsort.h's wave_chunk).  First sweep: per-wave, per-group member counts in LDS (integer adds).
//              An exclusive prefix over (group, wave) gives the segment offsets SEG[t][g] and each
//              wave's first slot in each segment.  Second sweep: the members' values and asset
//              indices go to the packed row SK / SI, group-major and ascending asset inside a
//              group.  A wave ranks its 64 cells by peeling the groups present in them: the first
//              unhandled lane's id, the ballot of the lanes that share it, mbcnt for the rank --
//              as many trips as there are distinct groups in the 64 cells.  Cells outside every
//              group get their -1 / NaN outputs here.
//   k_gdec     N2, N3.  One workgroup per (date, group).  The segment's keys are sorted by
//              gsort.h's sort_segment, which k_rank, k_ic and breakpoints.hip's k_bpedges call
//              too: a bitonic network on exactly n keys (every exchange moves the smaller key down, an
//              exchange whose upper index is past n is skipped: the network of the next power of
//              two with +inf above n).  SMALL: a segment of at most `cap` keys, sorted in LDS.
//              Otherwise: tiles of `tile` keys sorted in LDS, the exchanges wider than a tile made
//              in the packed row itself.  Each launch returns at once on the other's segments
//              (not_mine; sort_plan and LAUNCH_PAIR on the host).  Edges are NumPy's lerp on the
//              sorted keys as deciles.inc computes them, deduped;
//              a member's label is the count of edges below its value.  Only keys are sorted, so
//              labels and sums do not depend on which kernel took the segment.  The sums: label
//              d's wave adds NR over the packed positions lane, lane + 64, ... from 0.0 (0.0
//              for a position of another label), then the halving tree over the lanes: an order
//              that depends on the segment's length alone.
//   k_gpool    N3.  A lane per (date, label) adds the groups' sums and counts, g ascending.
//   k_gstats   N4, N5.  One workgroup per (date, group): lane sums over positions tid, tid + 256,
//              ..., the halving tree per wave, the waves in wave order (gsort.h's block_sum);
//              then the members' adjusted signals through SI.
//
// Ranks and information coefficients (rules I1..I6) stand on the same partition and sort:
//   k_rank     I1, I2.  One workgroup per (date, group), k_gpart's segments (a NULL GID: one group
//              of every non-NaN cell).  The keys are sorted as k_gdec sorts them; a member's lt /
//              le are a lower- and an upper-bound search in the sorted keys, its rank goes out
//              through SI.  Non-members got their NaN from k_gpart.
//   k_icpart   I3.  One workgroup per month: the assets with S[t] and Y[t + lead] both not NaN,
//              in asset order, to an index list and two packed value rows (gsort.h's pack_row).
//   k_icpearson I5.  k_gstats's sums on the packed values: the means, then the three centred sums.
//   k_ic       I4.  One workgroup per month.  LDS: S's keys sorted, each position's centred
//              doubled rank kept as int32, then Y's keys sorted in the same buffer.  Past the cap
//              both packed rows are sorted in place and the values re-read through the index
//              list.  The three sums are int64: exact in any order.
//
// No floating-point atomic anywhere: two calls give the same bits.
#include "gsort.h"   // block_sum, pack_row / wave_chunk, sort_segment, qcut_edge

#define GP_THREADS 1024
#define GP_WAVES (GP_THREADS / 64)
#define GP_MAXG 256        // n_groups <= 256
#define GP_U 4             // steps of 64 cells whose loads a wave issues together
#define GS_THREADS 256

// segments of at most this many keys take the LDS kernels, here and in breakpoints.hip
static int g_tune_gdec_small_cap = GD_TILE;

static const TuneKnob g_knobs[] = {
    {"gdec_small_cap", &g_tune_gdec_small_cap, [](int v) { return v >= 1 && v <= GD_TILE; }},
};

SortPlan sort_plan() {
  const int cap = g_tune_gdec_small_cap;
  int tile = 2;
  while (tile < 2 * cap && tile < GD_TILE) tile <<= 1;
  return {cap, tile};
}

// ------------------------------------------------------------------------------------ N1
// the group of cell i of the row, -1 for none
__device__ __forceinline__ int cell_group(double x, int id, int n_groups) {
  return (x == x && id >= 0 && id < n_groups) ? id : -1;
}

__global__ __launch_bounds__(GP_THREADS) void k_gpart(
    const double* __restrict__ S, const int16_t* __restrict__ GID, int64_t g_ld, int64_t N,
    int n_groups, int32_t* __restrict__ SEG, uint32_t* __restrict__ SI, double* __restrict__ SK,
    int8_t* __restrict__ L, int32_t* __restrict__ NVG, int32_t* __restrict__ NV,
    double* __restrict__ SA, double* __restrict__ SZ, double* __restrict__ SB) {
  __shared__ int s_cnt[GP_WAVES][GP_MAXG];   // counts, then each wave's next slot per group
  __shared__ int s_tot[GP_MAXG];
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* __restrict__ row = S + (int64_t)t * N;
  // (GID NULL: csm_xs_rank's one group of every non-NaN cell)
  const int16_t* __restrict__ gid = GID ? GID + (int64_t)t * g_ld : nullptr;
  const Chunk ch = wave_chunk<GP_THREADS>(N);
  const int64_t i0 = ch.i0, i1 = ch.i1;
  for (int k = tid; k < GP_WAVES * GP_MAXG; k += GP_THREADS) (&s_cnt[0][0])[k] = 0;
  __syncthreads();
  for (int64_t b = i0; b < i1; b += 64 * GP_U) {   // GP_U steps of 64 cells, their loads together
    double xv[GP_U];
    int gv[GP_U];
#pragma unroll
    for (int u = 0; u < GP_U; ++u) {
      const int64_t i = b + u * 64 + lane;
      xv[u] = i < i1 ? row[i] : qnan();
      gv[u] = i < i1 ? (gid ? (int)gid[i] : 0) : -1;
    }
#pragma unroll
    for (int u = 0; u < GP_U; ++u) {
      const int g = cell_group(xv[u], gv[u], n_groups);
      if (g >= 0) atomicAdd(&s_cnt[wave][g], 1);
    }
  }
  __syncthreads();
  if (tid < GP_MAXG) {
    int c = 0;
    if (tid < n_groups)
      for (int w = 0; w < GP_WAVES; ++w) c += s_cnt[w][tid];
    s_tot[tid] = c;
  }
  __syncthreads();
  if (wave == 0) {   // exclusive prefix over the groups, four per lane
    int v[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = s_tot[4 * lane + k];
      s += v[k];
    }
    int inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(inc, o, 64);
      if (lane >= o) inc += u;
    }
    int off = inc - s;
    int32_t* seg = SEG + (int64_t)t * (n_groups + 1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int g = 4 * lane + k;
      s_tot[g] = off;
      if (g < n_groups) {
        seg[g] = off;
        if (NVG) NVG[(int64_t)t * n_groups + g] = v[k];
      }
      off += v[k];
    }
    if (lane == 63) {
      seg[n_groups] = inc;
      if (NV) NV[t] = inc;
    }
  }
  __syncthreads();
  if (tid < n_groups) {
    int run = s_tot[tid];
    for (int w = 0; w < GP_WAVES; ++w) {
      const int c = s_cnt[w][tid];
      s_cnt[w][tid] = run;
      run += c;
    }
  }
  __syncthreads();
  uint32_t* __restrict__ si = SI + (int64_t)t * N;
  double* __restrict__ sk = SK + (int64_t)t * N;
  const double NaN = qnan();
  for (int64_t b0 = i0; b0 < i1; b0 += 64 * GP_U) {   // (wave-uniform trips)
    double xv[GP_U];
    int gv[GP_U];
#pragma unroll
    for (int u = 0; u < GP_U; ++u) {
      const int64_t i = b0 + u * 64 + lane;
      xv[u] = i < i1 ? row[i] : NaN;
      gv[u] = i < i1 ? (gid ? (int)gid[i] : 0) : -1;
    }
#pragma unroll
    for (int u = 0; u < GP_U; ++u) {
      const int64_t i = b0 + u * 64 + lane;
      const double x = xv[u];
      int g = -1;
      if (i < i1) {
        g = cell_group(x, gv[u], n_groups);
        if (g < 0) {
          if (L) L[(int64_t)t * N + i] = -1;
          if (SA) SA[(int64_t)t * N + i] = NaN;
          if (SZ) SZ[(int64_t)t * N + i] = NaN;
          if (SB) SB[(int64_t)t * N + i] = NaN;
        }
      }
      uint64_t rem = __ballot(g >= 0);
      while (rem) {   // (wave-uniform)
        const int leader = __ffsll((unsigned long long)rem) - 1;
        const int gl = __builtin_amdgcn_readlane(g, leader);
        const uint64_t m = __ballot(g == gl);
        if (g == gl) {
          const int pos = s_cnt[wave][gl] + lane_prefix(m);
          si[pos] = (uint32_t)i;
          sk[pos] = x;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane == leader) s_cnt[wave][gl] += __popcll(m);
        __builtin_amdgcn_wave_barrier();
        rem &= ~m;
      }
    }
  }
}

// ------------------------------------------------------------------------------------ N2
template <bool SMALL>
__global__ __launch_bounds__(SMALL ? GD_SMALL_THREADS : GD_LONG_THREADS) void k_gdec(
    const double* __restrict__ S, const double* __restrict__ NR, int64_t N, int n_groups,
    int n_bins, QTab qt, int min_group, int cap, int tile, const int32_t* __restrict__ SEG,
    const uint32_t* __restrict__ SI, double* SK, int8_t* SL, int8_t* __restrict__ L,
    double* __restrict__ SUMG, int32_t* __restrict__ CNTG, double* __restrict__ EWG) {
  constexpr int NT = SMALL ? GD_SMALL_THREADS : GD_LONG_THREADS;
  __shared__ double s_key[GD_TILE];
  __shared__ int8_t s_lab[SMALL ? GD_TILE : 16];
  __shared__ double s_edge[MAXQ], s_bins[MAXQ];
  __shared__ int s_nb;
  const int64_t cell = blockIdx.x;
  const int t = (int)(cell / n_groups), g = (int)(cell % n_groups);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int seg0 = SEG[(int64_t)t * (n_groups + 1) + g];
  const int n = SEG[(int64_t)t * (n_groups + 1) + g + 1] - seg0;
  if (not_mine<SMALL>(n, cap)) return;
  double* gk = SK + (int64_t)t * N + seg0;   // the segment's keys in the packed row
  const uint32_t* __restrict__ si = SI + (int64_t)t * N + seg0;
  const bool ranked = n >= min_group && n > 0;
  if (ranked) {
    // edges: NumPy's lerp on the sorted keys, as deciles.inc
    const double* srt = sort_segment<SMALL, NT>(gk, s_key, n, tile);
    if (tid <= n_bins) s_edge[tid] = qcut_edge(srt, n, qt.q[tid]);
    __syncthreads();
    if (tid == 0) {   // duplicates='drop'
      int nu = 0;
      const int ne = n_bins + 1;
      for (int k = 0; k < ne; ++k) {
        bool seen = false;
        for (int j = 0; j < nu; ++j) seen |= s_bins[j] == s_edge[k];
        if (!seen) s_bins[nu++] = s_edge[k];
      }
      if (!(nu < ne && ne != 2)) {
        for (int k = 0; k < ne; ++k) s_bins[k] = s_edge[k];
        nu = ne;
      }
      s_nb = nu;
    }
  } else if (tid == 0) {
    s_nb = 0;
  }
  __syncthreads();
  // labels; with NR each position's label and next return are staged where the keys were
  const int nb = s_nb;
  double* rr = SMALL ? s_key : gk;
  int8_t* lb = SMALL ? s_lab : SL + (int64_t)t * N + seg0;
  for (int p = tid; p < n; p += NT) {
    const int64_t idx = (int64_t)t * N + si[p];
    const double x = SMALL ? gk[p] : S[idx];   // (the LDS kernel leaves the packed keys unsorted)
    int ids = 0;
    for (int j = 0; j < nb; ++j) ids += (s_bins[j] < x) ? 1 : 0;
    if (nb > 0 && x == s_bins[0]) ids = 1;
    const int lab = (nb == 0 || ids == 0 || ids == nb) ? -1 : ids - 1;
    L[idx] = (int8_t)lab;
    if (NR) {
      const double r = NR[idx];
      const bool ok = lab >= 0 && r == r;
      rr[p] = ok ? r : 0.0;
      lb[p] = (int8_t)(ok ? lab : -1);
    }
  }
  if (!NR) return;
  __syncthreads();
  for (int d = wave; d < n_bins; d += NT / 64) {   // (wave-uniform)
    double s = 0.0;
    int c = 0;
    for (int p = lane; p < n; p += 64) {
      const bool h = lb[p] == d;
      s = s + (h ? rr[p] : 0.0);
      c += h ? 1 : 0;
    }
    s = wave_tree(s);
    c = wave_tree(c);
    if (lane == 0) {
      const int64_t o = cell * n_bins + d;
      SUMG[o] = s;
      CNTG[o] = c;
      if (EWG) EWG[o] = c > 0 ? s / (double)c : qnan();
    }
  }
}

// ------------------------------------------------------------------------------------ N3
__global__ __launch_bounds__(64) void k_gpool(const double* __restrict__ SUMG,
                                              const int32_t* __restrict__ CNTG, int T_m,
                                              int n_groups, int n_bins, double* __restrict__ EW,
                                              int32_t* __restrict__ CNT) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)T_m * n_bins) return;
  const int64_t t = id / n_bins;
  const int d = (int)(id % n_bins);
  double s = 0.0;
  int c = 0;
  for (int g = 0; g < n_groups; ++g) {
    const int64_t o = (t * n_groups + g) * n_bins + d;
    s = s + SUMG[o];
    c += CNTG[o];
  }
  if (EW) EW[id] = c > 0 ? s / (double)c : qnan();
  if (CNT) CNT[id] = c;
}

// -------------------------------------------------------------------------------- N4, N5
__global__ __launch_bounds__(GS_THREADS) void k_gstats(
    int64_t N, int n_groups, const int32_t* __restrict__ SEG, const uint32_t* __restrict__ SI,
    const double* __restrict__ SK, double* __restrict__ GMEAN, double* __restrict__ GSD,
    int32_t* __restrict__ GCNT, double* __restrict__ SA, double* __restrict__ SZ,
    double* __restrict__ SB) {
  __shared__ double s_part[GS_THREADS / 64];
  const int64_t cell = blockIdx.x;
  const int t = (int)(cell / n_groups), g = (int)(cell % n_groups);
  const int tid = threadIdx.x;
  const int seg0 = SEG[(int64_t)t * (n_groups + 1) + g];
  const int n = SEG[(int64_t)t * (n_groups + 1) + g + 1] - seg0;
  const double* __restrict__ sk = SK + (int64_t)t * N + seg0;
  const uint32_t* __restrict__ si = SI + (int64_t)t * N + seg0;
  double a = 0.0;
  for (int p = tid; p < n; p += GS_THREADS) a = a + sk[p];
  const double sum = block_sum<double, GS_THREADS>(a, s_part);
  const double mean = n > 0 ? sum / (double)n : qnan();
  double q = 0.0;
  for (int p = tid; p < n; p += GS_THREADS) {
    const double d = sk[p] - mean;
    q = q + d * d;
  }
  const double ss = block_sum<double, GS_THREADS>(q, s_part);
  const double sd = n >= 2 ? sqrt(ss / (double)(n - 1)) : qnan();
  if (tid == 0) {
    if (GMEAN) GMEAN[cell] = mean;
    if (GSD) GSD[cell] = sd;
    if (GCNT) GCNT[cell] = n;
  }
  if (!SA && !SZ && !SB) return;
  const bool zok = sd == sd && sd != 0.0;
  for (int p = tid; p < n; p += GS_THREADS) {
    const int64_t idx = (int64_t)t * N + si[p];
    const double sa = sk[p] - mean;
    if (SA) SA[idx] = sa;
    if (SZ) SZ[idx] = zok ? sa / sd : qnan();
    if (SB) SB[idx] = mean;
  }
}

// -------------------------------------------------------------------------------- I1, I2
// the number of srt[0..n) (ascending) below x (LE: not above x), known to lie in [lo, hi]
template <bool LE>
__device__ __forceinline__ int count_to(const double* srt, int lo, int hi, double x) {
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    const double v = srt[mid];
    if (LE ? v <= x : v < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}
// Past the LDS cap the sorted keys are in the packed row; every stride-th of them is staged in
// LDS (s[j] = srt[j * stride], at most cap samples), so a search makes its first steps in LDS and
// the last log2(stride) in the row.
struct Samples {
  int m, stride;
};
template <int NT>
__device__ __forceinline__ Samples stage_samples(const double* srt, int n, double* s, int cap) {
  Samples sp;
  sp.stride = (n + cap - 1) / cap;
  sp.m = (n + sp.stride - 1) / sp.stride;
  for (int j = threadIdx.x; j < sp.m; j += NT) s[j] = srt[(int64_t)j * sp.stride];
  return sp;
}
template <bool LE>
__device__ __forceinline__ int count_to(const double* srt, int n, const double* s, Samples sp,
                                        double x) {
  const int c = count_to<LE>(s, 0, sp.m, x);   // sample c - 1 counts, sample c does not
  return count_to<LE>(srt, c > 0 ? (c - 1) * sp.stride + 1 : 0, c < sp.m ? c * sp.stride : n, x);
}

template <bool SMALL>
__global__ __launch_bounds__(SMALL ? GD_SMALL_THREADS : GD_LONG_THREADS) void k_rank(
    const double* __restrict__ S, int64_t N, int n_groups, int method, int pct, int cap, int tile,
    const int32_t* __restrict__ SEG, const uint32_t* __restrict__ SI, double* SK,
    double* __restrict__ RANK) {
  constexpr int NT = SMALL ? GD_SMALL_THREADS : GD_LONG_THREADS;
  __shared__ double s_key[GD_TILE];
  const int64_t cell = blockIdx.x;
  const int t = (int)(cell / n_groups), g = (int)(cell % n_groups);
  const int tid = threadIdx.x;
  const int seg0 = SEG[(int64_t)t * (n_groups + 1) + g];
  const int n = SEG[(int64_t)t * (n_groups + 1) + g + 1] - seg0;
  if (not_mine<SMALL>(n, cap)) return;
  double* gk = SK + (int64_t)t * N + seg0;
  const uint32_t* __restrict__ si = SI + (int64_t)t * N + seg0;
  sort_segment<SMALL, NT>(gk, s_key, n, tile);
  Samples sp{};
  if (!SMALL) {
    sp = stage_samples<NT>(gk, n, s_key, GD_TILE);
    __syncthreads();
  }
  for (int p = tid; p < n; p += NT) {
    const int64_t idx = (int64_t)t * N + si[p];
    const double x = SMALL ? gk[p] : S[idx];   // (the LDS kernel leaves the packed keys unsorted)
    const int lt = SMALL ? count_to<false>(s_key, 0, n, x) : count_to<false>(gk, n, s_key, sp, x);
    const int le = SMALL ? count_to<true>(s_key, 0, n, x) : count_to<true>(gk, n, s_key, sp, x);
    double r = method == 0 ? (double)(lt + le + 1) / 2.0 : (double)(method == 1 ? lt + 1 : le);
    if (pct) r = r / (double)n;
    RANK[idx] = r;
  }
}

// -------------------------------------------------------------------------------- I3..I6
#define IC_THREADS 1024

// I3.  One workgroup per month; each wave owns one contiguous chunk of the row.  The assets with
// S[t] and Y[t + lead] both not NaN go, in asset order, to IX (their indices) and KS / KY (their
// values); CN[t] is their number.
__global__ __launch_bounds__(IC_THREADS) void k_icpart(
    const double* __restrict__ S, const double* __restrict__ Y, int T_m, int64_t N, int lead,
    uint32_t* __restrict__ IX, double* __restrict__ KS, double* __restrict__ KY,
    int32_t* __restrict__ CN, int32_t* __restrict__ NOBS) {
  __shared__ int s_cnt[IC_THREADS / 64];
  const int t = blockIdx.x, tid = threadIdx.x;
  if ((int64_t)t + lead >= T_m) {   // (block-uniform)
    if (tid == 0) {
      CN[t] = 0;
      if (NOBS) NOBS[t] = 0;
    }
    return;
  }
  const double* __restrict__ rs = S + (int64_t)t * N;
  const double* __restrict__ ry = Y + ((int64_t)t + lead) * N;
  uint32_t* __restrict__ ix = IX + (int64_t)t * N;
  double* __restrict__ ks = KS + (int64_t)t * N;
  double* __restrict__ ky = KY + (int64_t)t * N;
  double s, y;   // the cell's values, from the predicate to the emit
  const int tot = pack_row<IC_THREADS>(
      N, s_cnt,
      [&](int64_t i) {
        s = rs[i];
        y = ry[i];
        return s == s && y == y;
      },
      [&](int64_t i, int pos) {
        ix[pos] = (uint32_t)i;
        ks[pos] = s;
        ky[pos] = y;
      });
  if (tid == 0) {
    CN[t] = tot;
    if (NOBS) NOBS[t] = tot;
  }
}

// I5, on the packed values in asset order (before k_ic sorts them)
__global__ __launch_bounds__(GS_THREADS) void k_icpearson(
    int64_t N, int min_obs, const int32_t* __restrict__ CN, const double* __restrict__ KS,
    const double* __restrict__ KY, double* __restrict__ PIC) {
  __shared__ double s_part[GS_THREADS / 64];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int n = CN[t];
  if (n < min_obs) {   // (block-uniform)
    if (tid == 0) PIC[t] = qnan();
    return;
  }
  const double* __restrict__ ks = KS + (int64_t)t * N;
  const double* __restrict__ ky = KY + (int64_t)t * N;
  double a = 0.0, b = 0.0;
  for (int p = tid; p < n; p += GS_THREADS) {
    a = a + ks[p];
    b = b + ky[p];
  }
  const double ms = block_sum<double, GS_THREADS>(a, s_part) / (double)n;
  const double my = block_sum<double, GS_THREADS>(b, s_part) / (double)n;
  double qss = 0.0, qyy = 0.0, qsy = 0.0;
  for (int p = tid; p < n; p += GS_THREADS) {
    const double ds = ks[p] - ms, dy = ky[p] - my;
    qss = qss + ds * ds;
    qyy = qyy + dy * dy;
    qsy = qsy + ds * dy;
  }
  const double css = block_sum<double, GS_THREADS>(qss, s_part);
  const double cyy = block_sum<double, GS_THREADS>(qyy, s_part);
  const double csy = block_sum<double, GS_THREADS>(qsy, s_part);
  if (tid == 0) PIC[t] = (css > 0.0 && cyy > 0.0) ? csy / sqrt(css * cyy) : qnan();
}

// I4.  One workgroup per month.  SMALL: at most `cap` observations -- S's keys sorted in LDS, each
// position's centred doubled rank a kept as int32, then Y's keys sorted in the same buffer.
// Otherwise both packed rows are sorted in place (seg_sort) and each position's values are re-read
// from S and Y through IX.  The three sums are integers: exact in any order.
template <bool SMALL>
__global__ __launch_bounds__(SMALL ? GD_SMALL_THREADS : GD_LONG_THREADS) void k_ic(
    const double* __restrict__ S, const double* __restrict__ Y, int64_t N, int lead, int min_obs,
    int cap, int tile, const int32_t* __restrict__ CN, const uint32_t* __restrict__ IX, double* KS,
    double* KY, double* __restrict__ RIC) {
  constexpr int NT = SMALL ? GD_SMALL_THREADS : GD_LONG_THREADS;
  __shared__ double s_key[GD_TILE];
  __shared__ int32_t s_a[SMALL ? GD_TILE : 1];
  __shared__ long long s_red[NT / 64];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int n = CN[t];
  if (not_mine<SMALL>(n, cap)) return;
  if (n < min_obs) {
    if (tid == 0) RIC[t] = qnan();
    return;
  }
  double* ks = KS + (int64_t)t * N;
  double* ky = KY + (int64_t)t * N;
  long long sab = 0, saa = 0, sbb = 0;
  if (SMALL) {
    sort_segment<SMALL, NT>(ks, s_key, n, tile);
    for (int p = tid; p < n; p += NT) {
      const double x = ks[p];
      s_a[p] = count_to<false>(s_key, 0, n, x) + count_to<true>(s_key, 0, n, x) - n;
    }
    __syncthreads();
    sort_segment<SMALL, NT>(ky, s_key, n, tile);
    for (int p = tid; p < n; p += NT) {
      const double y = ky[p];
      const long long a = s_a[p];
      const long long b = count_to<false>(s_key, 0, n, y) + count_to<true>(s_key, 0, n, y) - n;
      sab += a * b;
      saa += a * a;
      sbb += b * b;
    }
  } else {
    sort_segment<SMALL, NT>(ks, s_key, n, tile);
    sort_segment<SMALL, NT>(ky, s_key, n, tile);
    double* s_ys = s_key + GD_TILE / 2;   // half of the buffer for each row's samples
    const Samples ps = stage_samples<NT>(ks, n, s_key, GD_TILE / 2);
    const Samples py = stage_samples<NT>(ky, n, s_ys, GD_TILE / 2);
    __syncthreads();
    const uint32_t* __restrict__ ix = IX + (int64_t)t * N;
    const double* __restrict__ rs = S + (int64_t)t * N;
    const double* __restrict__ ry = Y + ((int64_t)t + lead) * N;
    for (int p = tid; p < n; p += NT) {
      const double x = rs[ix[p]], y = ry[ix[p]];
      const long long a =
          count_to<false>(ks, n, s_key, ps, x) + count_to<true>(ks, n, s_key, ps, x) - n;
      const long long b =
          count_to<false>(ky, n, s_ys, py, y) + count_to<true>(ky, n, s_ys, py, y) - n;
      sab += a * b;
      saa += a * a;
      sbb += b * b;
    }
  }
  const long long ab = block_sum<long long, NT>(sab, s_red);
  const long long aa = block_sum<long long, NT>(saa, s_red);
  const long long bb = block_sum<long long, NT>(sbb, s_red);
  if (tid == 0) RIC[t] = (aa > 0 && bb > 0) ? (double)ab / sqrt((double)aa * (double)bb) : qnan();
}

// ----------------------------------------------------------------------------------- host
struct GrpWs {
  int32_t* seg;    // [T_m][n_groups + 1] segment offsets in the packed row
  uint32_t* si;    // [T_m][N] the members' asset indices, group-major
  double* sk;      // [T_m][N] their values (k_gdec: sorted keys, then staged next returns)
  int8_t* sl;      // [T_m][N] k_gdec's staged labels (segments past the LDS cap)
  double* sumg;    // [T_m][n_groups][n_bins]
  int32_t* cntg;   // [T_m][n_groups][n_bins]
};

static int grp_reserve(csm_ctx* ctx, const char* who, int32_t T_m, int64_t N, int32_t n_groups,
                       int32_t n_bins, GrpWs* w) {
  const size_t cells = (size_t)T_m * (size_t)N, tg = (size_t)T_m * (size_t)n_groups;
  const size_t b_seg = up16(((size_t)T_m * (size_t)(n_groups + 1)) * sizeof(int32_t));
  const size_t b_si = up16(cells * sizeof(uint32_t)), b_sk = up16(cells * sizeof(double));
  const size_t b_sl = up16(cells), b_sum = up16(tg * (size_t)n_bins * sizeof(double));
  const size_t b_cnt = up16(tg * (size_t)n_bins * sizeof(int32_t));
  int r = ctx_reserve(ctx, who, "the group partition workspace", &ctx->grp_ws, &ctx->grp_ws_bytes,
                      b_seg + b_si + b_sk + b_sl + b_sum + b_cnt);
  if (r) return r;
  char* p = (char*)ctx->grp_ws;
  w->sk = (double*)p;
  p += b_sk;
  w->sumg = (double*)p;
  p += b_sum;
  w->si = (uint32_t*)p;
  p += b_si;
  w->seg = (int32_t*)p;
  p += b_seg;
  w->cntg = (int32_t*)p;
  p += b_cnt;
  w->sl = (int8_t*)p;
  return CSM_OK;
}

// the checks the grouped entry points share (gid_opt: a NULL GID is the caller's to judge)
static int grp_check(csm_ctx* ctx, const char* who, const double* S, const int16_t* GID,
                     int64_t g_ld, int32_t T_m, int64_t N, int32_t n_groups,
                     bool gid_opt = false) {
  if (!S || (!GID && !gid_opt) || bad_panel(T_m, N, INT32_MAX))
    return set_err(ctx, CSM_E_INVAL, "%s: bad arguments (T_m=%d N=%lld)", who, T_m, (long long)N);
  if (n_groups < 1 || n_groups > GP_MAXG)
    return set_err(ctx, CSM_E_INVAL, "%s: n_groups=%d is outside [1, %d]", who, n_groups, GP_MAXG);
  if (g_ld != 0 && g_ld != N)
    return set_err(ctx, CSM_E_INVAL, "%s: g_ld=%lld must be 0 (one static row) or N=%lld", who,
                   (long long)g_ld, (long long)N);
  if ((int64_t)T_m * n_groups > 0x7FFFFFFFLL)
    return set_err(ctx, CSM_E_INVAL, "%s: T_m * n_groups = %lld segments exceed one launch", who,
                   (long long)T_m * n_groups);
  return CSM_OK;
}

extern "C" {

int csm_tune_groups(const char* key, int value) { return tune_set(g_knobs, key, value); }

int csm_group_deciles(csm_ctx* ctx, const double* S, const double* NR, const int16_t* GID,
                      int64_t g_ld, int32_t T_m, int64_t N, int32_t n_groups, int32_t n_bins,
                      const double* qtable, int32_t min_group, int8_t* L, double* EW, int32_t* CNT,
                      int32_t* NV, double* EWG, int32_t* CNTG, int32_t* NVG) {
  const char* who = "csm_group_deciles";
  int r = prep(ctx);
  if (r) return r;
  r = grp_check(ctx, who, S, GID, g_ld, T_m, N, n_groups);
  if (r) return r;
  if (!L || !qtable) return set_err(ctx, CSM_E_INVAL, "%s: L or qtable is NULL", who);
  if (min_group < 1)
    return set_err(ctx, CSM_E_INVAL, "%s: min_group=%d must be at least 1", who, min_group);
  r = check_n_bins(ctx, who, n_bins, NR != nullptr);
  if (r) return r;
  GrpWs w;
  r = grp_reserve(ctx, who, T_m, N, n_groups, n_bins, &w);
  if (r) return r;
  const QTab q = qtab_fill(qtable, n_bins);
  const SortPlan sp = sort_plan();
  hipLaunchKernelGGL(k_gpart, dim3((unsigned)T_m), dim3(GP_THREADS), 0, ctx->stream, S, GID, g_ld,
                     N, n_groups, w.seg, w.si, w.sk, L, NVG, NV, (double*)nullptr,
                     (double*)nullptr, (double*)nullptr);
  LAUNCH_CHECK(ctx, "k_gpart");
  const unsigned segs = (unsigned)((int64_t)T_m * n_groups);
  int32_t* cntg = CNTG ? CNTG : w.cntg;
  LAUNCH_PAIR(ctx, k_gdec, segs, S, NR, N, n_groups, n_bins, q, min_group, sp.cap, sp.tile, w.seg,
              w.si, w.sk, w.sl, L, w.sumg, cntg, EWG);
  if (NR && (EW || CNT)) {
    const int64_t lanes = (int64_t)T_m * n_bins;
    hipLaunchKernelGGL(k_gpool, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, ctx->stream,
                       w.sumg, cntg, T_m, n_groups, n_bins, EW, CNT);
    LAUNCH_CHECK(ctx, "k_gpool");
  }
  return CSM_OK;
}

int csm_group_stats(csm_ctx* ctx, const double* S, const int16_t* GID, int64_t g_ld, int32_t T_m,
                    int64_t N, int32_t n_groups, double* GMEAN, double* GSD, int32_t* GCNT,
                    double* SA, double* SZ, double* SB) {
  const char* who = "csm_group_stats";
  int r = prep(ctx);
  if (r) return r;
  r = grp_check(ctx, who, S, GID, g_ld, T_m, N, n_groups);
  if (r) return r;
  GrpWs w;
  r = grp_reserve(ctx, who, T_m, N, n_groups, 1, &w);
  if (r) return r;
  hipLaunchKernelGGL(k_gpart, dim3((unsigned)T_m), dim3(GP_THREADS), 0, ctx->stream, S, GID, g_ld,
                     N, n_groups, w.seg, w.si, w.sk, (int8_t*)nullptr, (int32_t*)nullptr,
                     (int32_t*)nullptr, SA, SZ, SB);
  LAUNCH_CHECK(ctx, "k_gpart");
  hipLaunchKernelGGL(k_gstats, dim3((unsigned)((int64_t)T_m * n_groups)), dim3(GS_THREADS), 0,
                     ctx->stream, N, n_groups, w.seg, w.si, w.sk, GMEAN, GSD, GCNT, SA, SZ, SB);
  LAUNCH_CHECK(ctx, "k_gstats");
  return CSM_OK;
}

int csm_xs_rank(csm_ctx* ctx, const double* S, const int16_t* GID, int64_t g_ld, int32_t T_m,
                int64_t N, int32_t n_groups, int32_t method, int32_t pct, double* RANK,
                int32_t* NVG) {
  const char* who = "csm_xs_rank";
  int r = prep(ctx);
  if (r) return r;
  r = grp_check(ctx, who, S, GID, g_ld, T_m, N, n_groups, true);
  if (r) return r;
  if (!RANK) return set_err(ctx, CSM_E_INVAL, "%s: RANK is NULL", who);
  if (!GID && n_groups != 1)
    return set_err(ctx, CSM_E_INVAL, "%s: GID is NULL with n_groups=%d (one group only)", who,
                   n_groups);
  if (method < 0 || method > 2)
    return set_err(ctx, CSM_E_INVAL, "%s: method=%d is not 0 (average), 1 (min) or 2 (max)", who,
                   method);
  GrpWs w;
  r = grp_reserve(ctx, who, T_m, N, n_groups, 1, &w);
  if (r) return r;
  const SortPlan sp = sort_plan();
  hipLaunchKernelGGL(k_gpart, dim3((unsigned)T_m), dim3(GP_THREADS), 0, ctx->stream, S, GID, g_ld,
                     N, n_groups, w.seg, w.si, w.sk, (int8_t*)nullptr, NVG, (int32_t*)nullptr, RANK,
                     (double*)nullptr, (double*)nullptr);
  LAUNCH_CHECK(ctx, "k_gpart");
  LAUNCH_PAIR(ctx, k_rank, (unsigned)((int64_t)T_m * n_groups), S, N, n_groups, method, pct,
              sp.cap, sp.tile, w.seg, w.si, w.sk, RANK);
  return CSM_OK;
}

int csm_rank_ic(csm_ctx* ctx, const double* S, const double* Y, int32_t T_m, int64_t N,
                int32_t lead, int32_t min_obs, double* RIC, double* PIC, int32_t* NOBS) {
  const char* who = "csm_rank_ic";
  int r = prep(ctx);
  if (r) return r;
  if (!S || !Y || bad_panel(T_m, N) || lead < 0)
    return set_err(ctx, CSM_E_INVAL, "%s: bad arguments (T_m=%d N=%lld lead=%d)", who, T_m,
                   (long long)N, lead);
  if (N > ((int64_t)1 << 20))   // |a| < n <= 2^20: the int64 sums of I4 stay below 2^60
    return set_err(ctx, CSM_E_INVAL, "%s: N=%lld exceeds 2^20", who, (long long)N);
  if (min_obs < 2)
    return set_err(ctx, CSM_E_INVAL, "%s: min_obs=%d must be at least 2", who, min_obs);
  if (!RIC && !PIC) return set_err(ctx, CSM_E_INVAL, "%s: RIC and PIC are both NULL", who);
  // the index list and two key rows (20 B per cell), the months' counts
  const size_t cells = (size_t)T_m * (size_t)N;
  const size_t b_k = up16(cells * sizeof(double)), b_ix = up16(cells * sizeof(uint32_t));
  r = ctx_reserve(ctx, who, "the group partition workspace", &ctx->grp_ws, &ctx->grp_ws_bytes,
                  2 * b_k + b_ix + up16((size_t)T_m * sizeof(int32_t)));
  if (r) return r;
  char* p = (char*)ctx->grp_ws;
  double* ks = (double*)p;
  double* ky = (double*)(p + b_k);
  uint32_t* ix = (uint32_t*)(p + 2 * b_k);
  int32_t* cn = (int32_t*)(p + 2 * b_k + b_ix);
  const SortPlan sp = sort_plan();
  hipLaunchKernelGGL(k_icpart, dim3((unsigned)T_m), dim3(IC_THREADS), 0, ctx->stream, S, Y, T_m, N,
                     lead, ix, ks, ky, cn, NOBS);
  LAUNCH_CHECK(ctx, "k_icpart");
  if (PIC) {
    hipLaunchKernelGGL(k_icpearson, dim3((unsigned)T_m), dim3(GS_THREADS), 0, ctx->stream, N,
                       min_obs, cn, ks, ky, PIC);
    LAUNCH_CHECK(ctx, "k_icpearson");
  }
  if (RIC)
    LAUNCH_PAIR(ctx, k_ic, (unsigned)T_m, S, Y, N, lead, min_obs, sp.cap, sp.tile, cn, ix, ks, ky,
                RIC);
  return CSM_OK;
}

}  // extern "C"
