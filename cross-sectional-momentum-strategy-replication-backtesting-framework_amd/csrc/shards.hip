// shards.hip -- date shards (multi-GPU date sharding): the exchange records of
// shard.h, their fold into a shard's carry, and the speculative and halo passes around k_signal.
//
//   k_shard_summary_chunked   the record of every (month chunk, asset) of a month-price panel;
//                             one chunk is a rank's whole shard (csm_shard_summary).
//   k_fold_carry              fold_body per asset: the all-gathered records of the earlier shards
//                             into the scan state at a shard's first month.
//   k_shard_summary_state     the record from the end state k_signal<SH> left, with short walks
//   k_shard_summary_cols      from both ends of PM; _cols for a column list, a workgroup each.
//   k_shard_repair(_cols)     replays an asset from the true carry beside the speculative
//                             trajectory until the two states agree.
//   k_shard_fix_cols          fold and replay of the listed columns in one launch (halo pass).
//   k_halo_pm, k_shard_halo   the halo months' prices and the scan state they leave, with the
//                             flags of the assets for which that state may not be exact.
//   k_shard_need, k_shard_union   the flagged assets as bit masks, and the ranks' union as a
//                             column list.
#include <algorithm>

#include "csm_common.h"
#include "scan.h"
#include "shard.h"

// =====================================================================================
// Date-shard exchange records (shard.h).
// =====================================================================================
__global__ __launch_bounds__(256) void k_shard_summary_chunked(const double* __restrict__ PM,
                                                               int T_m, int64_t N, int T, int G,
                                                               double* __restrict__ out) {
  const int g = blockIdx.y;
  int m0, m1;
  chunk_range(T_m, G, g, m0, m1);
  const int S = SUM_SCALARS + T;
  // chunk g through pointer offsets (grid.x covers the assets)
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= N) return;
  const double* pm = PM + (int64_t)m0 * N;
  double* o = out + (int64_t)g * S * N;
  const int tm = m1 - m0;
  int64_t n = 0, fv = -1, lvi = -1;
  double lv = qnan(), first = absent_val();
  for (int mb = 0; mb < tm; mb += SUM_U) {
    double xs[SUM_U];
#pragma unroll
    for (int u = 0; u < SUM_U; ++u) xs[u] = mb + u < tm ? pm[(int64_t)(mb + u) * N + a] : absent_val();
#pragma unroll
    for (int u = 0; u < SUM_U; ++u) {
      const double x = xs[u];
      if (is_absent(x)) continue;
      if (n == 0) first = x;
      if (!isnan_d(x)) { if (fv < 0) fv = n; lvi = n; lv = x; }
      ++n;
    }
  }
  const int k = (int)(n < T ? n : T);
  int got = 0;
  double head = qnan();
  for (int j = 0; j < T - k; ++j) o[(int64_t)(SUM_SCALARS + j) * N + a] = absent_val();
  // backward: the last k present rows (oldest first in the record), then the last valid price
  // before them
  bool done = false;
  for (int mb = tm - 1; mb >= 0 && !done; mb -= SUM_U) {
    double xs[SUM_U];
#pragma unroll
    for (int u = 0; u < SUM_U; ++u) xs[u] = mb - u >= 0 ? pm[(int64_t)(mb - u) * N + a] : absent_val();
#pragma unroll
    for (int u = 0; u < SUM_U; ++u) {
      const double x = xs[u];
      if (done || mb - u < 0 || is_absent(x)) continue;
      if (got < k) {
        o[(int64_t)(SUM_SCALARS + T - 1 - got) * N + a] = x;
        ++got;
      } else if (!isnan_d(x)) {
        head = x;
        done = true;
      }
    }
  }
  o[0 * N + a] = (double)n;
  o[1 * N + a] = (double)fv;
  o[2 * N + a] = (double)lvi;
  o[3 * N + a] = lv;
  o[4 * N + a] = head;
  o[5 * N + a] = first;
}

__global__ __launch_bounds__(256) void k_fold_carry(const double* __restrict__ sm, int G, int g,
                                                    int64_t N, int J, int skip,
                                                    double* __restrict__ carry,
                                                    double* __restrict__ next_pm,
                                                    const double* __restrict__ tail_pm,
                                                    FoldJs jq, double* __restrict__ psq) {
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= N) return;
  const int W = J + skip;
  if (g < 0) {  // batched over all chunks: chunk blockIdx.y, outputs stacked per chunk
    g = blockIdx.y;
    carry += (int64_t)g * (W + 2) * N;
    next_pm += (int64_t)g * N;
  }
  next_pm[a] = fold_body(sm, G, g, N, a, J, skip, tail_pm,
                         [&](int k, double v) { carry[(int64_t)k * N + a] = v; }, jq, psq);
}

// =====================================================================================
// Speculative date shards (the fused multi-GPU pass).  A rank runs k_signal<SH>
// on its month range from an EMPTY scan state (trajectory F) before the earlier shards' carry
// is known, writing PM and a [5][N] end-state record (present months, pending row, its psff,
// first / last present month).  k_shard_summary_state builds the exchange record from PM with
// short walks from both ends (no full pass).  After the all-gather and k_fold_carry,
// k_shard_repair replays each asset from the true carry (trajectory T) beside F, rewriting
// R / M / NR, until the two states are bit-identical -- from then on every output k_signal
// wrote is T's -- or the asset has no present month left; then it finishes the pending ranked
// row with next_pm (k_signal ran without it).  A dense asset converges after its first
// J + skip + 1 present months.  Bit-identical to the unfused k_month_end ->
// k_shard_summary_chunked -> k_fold_carry -> k_momentum(carry) pass.
// =====================================================================================
#define REPAIR_THREADS 64
#define REPAIR_CHUNK WALK_CHUNK

// The record body over a month source: chunk(m0, dm, lo, hi, buf) fills WALK_CHUNK month
// prices (ABSENT outside [lo, hi]) and one(m) gives one month's price.
template <class Chunk, class One>
__device__ __forceinline__ void shard_summary_body(Chunk chunk, One one, int64_t n, int fm, int lm,
                                                   int T, int64_t os, double* __restrict__ out) {
  int64_t fv = -1, lvi = -1;
  double lv = qnan(), head = qnan(), first = absent_val();
  const int k = (int)(n < T ? n : T);
  for (int q = 0; q < T - k; ++q) out[(int64_t)(SUM_SCALARS + q) * os] = absent_val();
  if (n > 0) {
    // forward from the first present month: first price, index of the first valid row
    first = one(fm);
    int64_t ix = 0;
    bool found = false;
    for (int m0 = fm; m0 <= lm && !found; m0 += WALK_CHUNK) {
      double buf[WALK_CHUNK];
      chunk(m0, 1, fm, lm, buf);
#pragma unroll
      for (int q = 0; q < WALK_CHUNK; ++q) {
        const double x = buf[q];
        if (found || is_absent(x)) continue;
        if (!isnan_d(x)) { fv = ix; found = true; }
        ++ix;
      }
    }
    // backward from the last present month: tail, last valid (lv, lvi), head
    int got = 0;
    int64_t seen = 0;          // present rows passed, newest first
    bool have_lv = false, done = false;
    for (int m0 = lm; m0 >= fm && !done; m0 -= WALK_CHUNK) {
      double buf[WALK_CHUNK];
      chunk(m0, -1, fm, lm, buf);
#pragma unroll
      for (int q = 0; q < WALK_CHUNK; ++q) {
        const double x = buf[q];
        if (done || is_absent(x)) continue;
        const bool valid = !isnan_d(x);
        if (valid && !have_lv) { lv = x; lvi = n - 1 - seen; have_lv = true; }
        if (got < k) {
          out[(int64_t)(SUM_SCALARS + T - 1 - got) * os] = x;
          ++got;
        } else if (valid) {
          head = x;
          done = true;
        }
        ++seen;
      }
    }
  }
  out[0 * os] = (double)n;
  out[1 * os] = (double)fv;
  out[2 * os] = (double)lvi;
  out[3 * os] = lv;
  out[4 * os] = head;
  out[5 * os] = first;
}

// The exchange record (shard.h), as k_shard_summary_chunked builds it, from the SH state's n /
// first / last month.
// idx (the halo pass's fallback columns): output column j < ncol is asset idx[j] (record rows
// ncol apart); columns past the list's length *cnt get the record of an asset with no present
// month (a neutral column for k_fold_carry).
__global__ __launch_bounds__(256) void k_shard_summary_state(const double* __restrict__ PM,
                                                             const double* __restrict__ P,
                                                             const int64_t* __restrict__ ms,
                                                             int T_m, int64_t N, int T,
                                                             const double* __restrict__ st,
                                                             double* __restrict__ out,
                                                             const int32_t* __restrict__ idx,
                                                             const int32_t* __restrict__ cnt,
                                                             int64_t ncol) {
  const int W = T - 1;
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= (idx ? ncol : N)) return;
  const int64_t os = idx ? ncol : N;   // output row stride
  const bool listed = !idx || j < (int64_t)*cnt;
  const int64_t a = idx ? (listed ? (int64_t)idx[j] : 0) : j;
  const int64_t n = listed ? (int64_t)st[a] : 0;
  const int fm = listed ? (int)st[3 * N + a] : -1, lm = listed ? (int)st[4 * N + a] : -1;
  shard_summary_body(
      [&](int m0, int dm, int lo, int hi, double (&buf)[WALK_CHUNK]) {
        shard_pm_chunk(PM, P, ms, m0, dm, lo, hi, T_m, W, N, a, buf);
      },
      [&](int m) { return shard_pm_at(PM, P, ms, m, T_m, W, N, a); }, n, fm, lm, T, os, out + j);
}

// The listed columns of the halo pass, ONE WORKGROUP PER COLUMN (COLS_THREADS): its threads
// derive the column's T_m month prices together (PM where kept, else the month-end of the
// daily rows: one round trip for all months instead of one per re-derived month), into LDS; one
// lane then builds the record from LDS exactly as k_shard_summary_state does.  The grid is
// min(ncol, 2 n_CU) workgroups striding over the ncol columns (the listed count is on the
// device): a listed column as above, a column past the list gets the neutral record (no present
// month: k_shard_summary_state's, its T + SUM_SCALARS rows written by the workgroup's lanes).
#define COLS_THREADS 64
__global__ __launch_bounds__(COLS_THREADS) void k_shard_summary_cols(
    const double* __restrict__ PM, const double* __restrict__ P, const int64_t* __restrict__ ms,
    int T_m, int64_t N, int T, const double* __restrict__ st, double* __restrict__ out,
    const int32_t* __restrict__ idx, const int32_t* __restrict__ cnt, int64_t ncol) {
  extern __shared__ __attribute__((aligned(16))) double pmc[];   // [T_m]
  const int W = T - 1;
  const int64_t nl = *cnt;
  for (int64_t j = blockIdx.x; j < ncol; j += gridDim.x) {   // (workgroup-uniform)
    if (j >= nl) {   // the neutral record: shard_summary_body with n = 0
      for (int r = threadIdx.x; r < SUM_SCALARS + T; r += COLS_THREADS) {
        double v = absent_val();   // the tail rows and `first`
        if (r == 0) v = 0.0;
        else if (r == 1 || r == 2) v = -1.0;
        else if (r == 3 || r == 4) v = qnan();
        out[(int64_t)r * ncol + j] = v;
      }
      continue;
    }
    const int64_t a = (int64_t)idx[j];
    __syncthreads();   // (the previous column's lane 0 is done with pmc)
    for (int m = threadIdx.x; m < T_m; m += COLS_THREADS) pmc[m] = shard_pm_at(PM, P, ms, m, T_m, W, N, a);
    __syncthreads();
    if (threadIdx.x != 0) continue;
    const int64_t n = (int64_t)st[a];
    const int fm = (int)st[3 * N + a], lm = (int)st[4 * N + a];
    shard_summary_body(
        [&](int m0, int dm, int lo, int hi, double (&buf)[WALK_CHUNK]) {
#pragma unroll
          for (int q = 0; q < WALK_CHUNK; ++q) {
            const int m = m0 + q * dm;
            buf[q] = (m >= lo && m <= hi) ? pmc[m] : absent_val();
          }
        },
        [&](int m) { return pmc[m]; }, n, fm, lm, T, ncol, out + j);
  }
}

__device__ __forceinline__ bool same_bits(double x, double y) {
  return __double_as_longlong(x) == __double_as_longlong(y);
}

// fcarry: F's initial state (the halo pass's carry, [W+2][N]); NULL = empty (the speculative
// pass).  idx (the halo pass's fallback columns): thread j repairs asset idx[j] for j < *cnt,
// with carry / next_pm column j (rows ncol apart); NULL = every asset, carry / next_pm [.][N].
// The repair body for asset a over a month source chunk(m0, buf) (REPAIR_CHUNK months from m0,
// ABSENT past T_m - 1); rt / rf: T's and F's rings (stride RS).
template <class Chunk>
__device__ __forceinline__ void shard_repair_body(
    Chunk chunk, int T_m, int64_t N, int J, int skip, const double* __restrict__ carry,
    const double* __restrict__ next_pm, const double* __restrict__ st, double* __restrict__ R,
    double* __restrict__ M, double* __restrict__ NR, uint16_t* __restrict__ IDS,
    const double* __restrict__ fcarry, int64_t a, int64_t cs, int64_t cj, double* rt,
    double* rf, int RS) {
  const int W = J + skip;
  ScanLane t, f;
  scan_init(t, rt, RS, W, carry, cs, cj, true);
  scan_init(f, rf, RS, W, fcarry, N, a, true);
  auto same = [&]() -> bool {
    if (!same_bits(t.pff, f.pff) || !same_bits(t.psff, f.psff) || t.prev != f.prev) return false;
    for (int k = 0; k < W; ++k)
      if (!same_bits(rt[k * RS], rf[k * RS])) return false;
    return true;
  };
  const int64_t npres = (int64_t)st[a];
  const int fm = (int)st[3 * N + a];  // months before the first present one change no state
  int64_t seen = 0;
  bool conv = same();
  bool done = conv || npres == 0;
  static_assert(REPAIR_CHUNK == WALK_CHUNK, "the repair walks months in shard_pm_chunk's batches");
  for (int m0 = fm < 0 ? 0 : fm; m0 < T_m && !done; m0 += REPAIR_CHUNK) {
    double buf[REPAIR_CHUNK];
    chunk(m0, buf);
#pragma unroll
    for (int q = 0; q < REPAIR_CHUNK; ++q) {
      const int m = m0 + q;
      if (m >= T_m || done) break;
      const double x = buf[q];
      const double mom = scan_step(t, x, m, rt, RS, W, J, N, a, R, M, NR);
      if (IDS) IDS[(int64_t)m * N + a] = (uint16_t)csm_fid(mom);   // the rewritten cell's bucket id
      scan_shadow(f, x, m, rf, RS, W, J);
      if (!is_absent(x)) ++seen;
      conv = same();
      done = conv || seen >= npres;
    }
  }
  // the pending ranked row at the shard's end: F's (= T's once converged) or T's own
  const int prev = conv ? (int)st[N + a] : t.prev;
  const double psff = conv ? st[2 * N + a] : t.psff;
  if (prev >= 0) NR[(int64_t)prev * N + a] = pending_finish(next_pm[cj], psff);
}

__global__ __launch_bounds__(REPAIR_THREADS) void k_shard_repair(
    const double* __restrict__ PM, const double* __restrict__ P, const int64_t* __restrict__ ms,
    int T_m, int64_t N, int J, int skip,
    const double* __restrict__ carry, const double* __restrict__ next_pm,
    const double* __restrict__ st, double* __restrict__ R, double* __restrict__ M,
    double* __restrict__ NR, uint16_t* __restrict__ IDS, const double* __restrict__ fcarry,
    const int32_t* __restrict__ idx, const int32_t* __restrict__ cnt, int64_t ncol) {
  extern __shared__ __attribute__((aligned(16))) double lds[];  // [2][W][REPAIR_THREADS]
  const int W = J + skip, RS = REPAIR_THREADS;
  const int tid = threadIdx.x;
  const int64_t j = (int64_t)blockIdx.x * REPAIR_THREADS + tid;
  if (idx ? (j >= ncol || j >= (int64_t)*cnt) : j >= N) return;  // no barriers below
  const int64_t a = idx ? (int64_t)idx[j] : j;
  const int64_t cs = idx ? ncol : N, cj = idx ? j : a;   // carry / next_pm stride and column
  shard_repair_body(
      [&](int m0, double (&buf)[REPAIR_CHUNK]) {
        shard_pm_chunk(PM, P, ms, m0, 1, 0, T_m - 1, T_m, W, N, a, buf);
      },
      T_m, N, J, skip, carry, next_pm, st, R, M, NR, IDS, fcarry, a, cs, cj, lds + tid,
      lds + W * RS + tid, RS);
}

// The listed columns of the halo pass, one workgroup per column (k_shard_summary_cols' month
// prices into LDS by all its threads, then one lane repairs from them; rings in LDS too).
__global__ __launch_bounds__(COLS_THREADS) void k_shard_repair_cols(
    const double* __restrict__ PM, const double* __restrict__ P, const int64_t* __restrict__ ms,
    int T_m, int64_t N, int J, int skip,
    const double* __restrict__ carry, const double* __restrict__ next_pm,
    const double* __restrict__ st, double* __restrict__ R, double* __restrict__ M,
    double* __restrict__ NR, uint16_t* __restrict__ IDS, const double* __restrict__ fcarry,
    const int32_t* __restrict__ idx, const int32_t* __restrict__ cnt, int64_t ncol) {
  extern __shared__ __attribute__((aligned(16))) double lds[];  // pm [T_m], rings [2][W]
  const int W = J + skip;
  const int64_t j = blockIdx.x;
  if (j >= (int64_t)*cnt) return;   // (workgroup-uniform: before the barrier)
  const int64_t a = (int64_t)idx[j];
  double* pmc = lds;
  for (int m = threadIdx.x; m < T_m; m += COLS_THREADS) pmc[m] = shard_pm_at(PM, P, ms, m, T_m, W, N, a);
  __syncthreads();
  if (threadIdx.x != 0) return;
  shard_repair_body(
      [&](int m0, double (&buf)[REPAIR_CHUNK]) {
#pragma unroll
        for (int q = 0; q < REPAIR_CHUNK; ++q) buf[q] = m0 + q < T_m ? pmc[m0 + q] : absent_val();
      },
      T_m, N, J, skip, carry, next_pm, st, R, M, NR, IDS, fcarry, a, ncol, j, lds + T_m,
      lds + T_m + W, 1);
}

// The halo pass's listed columns after collective 1b, in ONE launch: a workgroup per listed
// column (a grid-stride loop over the device-side count, so an empty list costs one wave per
// workgroup) folds the column's exchange records (fold_body, k_fold_carry's walk) into the
// true scan state at the shard's first month and the first present price after the shard,
// derives the column's month prices into LDS (shard_pm_at, all lanes), and one lane replays
// every month from that state -- the sequential scan itself, so every output of the column is
// the unsharded pass's (no convergence test against the halo trajectory: nothing the halo
// state wrote is trusted).  Replaces k_fold_carry + k_shard_repair_cols.
template <int WR, int JC>
__global__ __launch_bounds__(COLS_THREADS) void k_shard_fix_cols(
    const double* __restrict__ PM, const double* __restrict__ P, const int64_t* __restrict__ ms,
    int T_m, int64_t N, int J, int skip, const double* __restrict__ recs, int G, int g,
    double* __restrict__ R, double* __restrict__ M, double* __restrict__ NR,
    uint16_t* __restrict__ IDS, const int32_t* __restrict__ idx, const int32_t* __restrict__ cnt,
    int64_t ncol) {
  // LDS: pm [T_m], carry [W + 2], ring [W] (runtime W), the column's records [G][S]
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int W = J + skip, S = SUM_SCALARS + W + 1;
  double* pmc = lds;
  double* cy = lds + T_m;
  double* ring = cy + W + 2;
  double* rec = ring + W;
  const int64_t n = (int64_t)*cnt < ncol ? (int64_t)*cnt : ncol;
  for (int64_t j = blockIdx.x; j < n; j += gridDim.x) {   // (workgroup-uniform)
    const int64_t a = (int64_t)idx[j];
    for (int q = threadIdx.x; q < G * S; q += COLS_THREADS) rec[q] = recs[(int64_t)q * ncol + j];
    for (int m = threadIdx.x; m < T_m; m += COLS_THREADS) pmc[m] = shard_pm_at(PM, P, ms, m, T_m, W, N, a);
    __syncthreads();
    if (threadIdx.x == 0) {
      const double npm = fold_body(rec, G, g, 1, 0, J, skip, (const double*)nullptr,
                                   [&](int k, double v) { cy[k] = v; }, FoldJs{0, {0, 0, 0, 0}},
                                   (double*)nullptr);
      ScanLane t;
      if constexpr (WR > 0) {   // the ring in registers, oldest first (k_signal_tc's scan)
        double fr[WR];
#pragma unroll
        for (int k = 0; k < WR; ++k) fr[k] = cy[k];
        t.pff = cy[WR];
        t.psff = cy[WR + 1];
        t.head = 0;
        t.prev = -1;
        double xn = pmc[0];
        for (int m = 0; m < T_m; ++m) {
          const double x = xn;
          if (m + 1 < T_m) xn = pmc[m + 1];
          const double mom = scan_step_reg<WR, JC>(t, x, m, fr, J, N, a, R, M, NR);
          if (IDS) IDS[(int64_t)m * N + a] = (uint16_t)csm_fid(mom);
        }
      } else {
        scan_init(t, ring, 1, W, cy, 1, 0, true);
        for (int m = 0; m < T_m; ++m) {
          const double mom = scan_step(t, pmc[m], m, ring, 1, W, J, N, a, R, M, NR);
          if (IDS) IDS[(int64_t)m * N + a] = (uint16_t)csm_fid(mom);
        }
      }
      // the pending ranked row at the shard's end (scan_finish)
      if (t.prev >= 0) NR[(int64_t)t.prev * N + a] = pending_finish(npm, t.psff);
    }
    __syncthreads();   // (the LDS is the next column's)
  }
}

// =====================================================================================
// Halo date shards (the default multi-GPU pass; north_star's "J + skip lookback
// halo").  A rank holds its shard's daily rows plus H calendar months before it and the first
// month after it.  k_shard_halo builds the scan state the halo months leave (from an empty
// state) and the forward month's price; the state is EXACT -- equal to the one the whole
// history leaves -- whenever the halo holds two valid prices W = J + skip present months apart
// (fv, lv below): the ring's W factors then all follow a valid price, and the last valid price
// is a ranked row in both histories.  k_signal<SH> starts from that state and the forward
// price, so a dense asset's outputs are final after one pass and no record is exchanged for
// it.  The other assets (listed inside the halo or the shard, long gaps, a forward month with
// no row) are flagged; only they take the exchange-and-repair path, over a column list.
// =====================================================================================
#define HALO_THREADS 256
#define HALO_U 8
// The halo months' and the forward months' prices, one thread per (asset, month): PMh[j][N],
// j < H halo month j, j = H + f forward month f < F.  A wave whose lanes walk a month back (no
// price on its last day: listings, delistings, absent months) does not hold up the others.
__global__ __launch_bounds__(HALO_THREADS) void k_halo_pm(const double* __restrict__ P,
                                                          const int64_t* __restrict__ ms, int H,
                                                          int T_m, int64_t N,
                                                          double* __restrict__ PMh) {
  const int64_t a = (int64_t)blockIdx.x * HALO_THREADS + threadIdx.x;
  const int j = blockIdx.y;
  if (a >= N) return;
  const int m = j < H ? j : j + T_m;
  PMh[(int64_t)j * N + a] = halo_month_price(P, ms[m], ms[m + 1], N, a);
}

// months [0, H) of ms are the halo, [H, H + T_m) the shard, [H + T_m, H + T_m + F) the forward
// months, their prices in PMh (k_halo_pm).  before: the panel has months before the halo (else
// the halo is the whole history and its state exact); after: the panel has months after the
// forward months (else an asset with no row in them has next_pm ABSENT, exactly).  carry
// [W+2][N] (csm_signal's layout), next_pm [N] (the first forward month with a row), flags [N]:
// bit 0 the carry may differ from the whole history's, bit 1 next_pm may.
__global__ __launch_bounds__(HALO_THREADS) void k_shard_halo(
    const double* __restrict__ PMh, int H, int F, int before, int after, int64_t N, int J,
    int skip, double* __restrict__ carry, double* __restrict__ next_pm,
    uint8_t* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) double hring[];  // [W][HALO_THREADS]
  const int W = J + skip, RS = HALO_THREADS;
  const int64_t a = (int64_t)blockIdx.x * HALO_THREADS + threadIdx.x;
  if (a >= N) return;  // no barriers below
  double* ring = hring + threadIdx.x;
  ScanLane s;
  scan_init(s, ring, RS, W, nullptr, N, a, true);
  int n = 0, fv = -1, lv = -1;
  for (int m0 = 0; m0 < H; m0 += HALO_U) {
    double xs[HALO_U];   // HALO_U month prices in flight
#pragma unroll
    for (int u = 0; u < HALO_U; ++u)
      xs[u] = m0 + u < H ? PMh[(int64_t)(m0 + u) * N + a] : absent_val();
#pragma unroll
    for (int u = 0; u < HALO_U; ++u) {
      const double x = xs[u];
      if (m0 + u >= H || is_absent(x)) continue;
      if (!isnan_d(x)) { if (fv < 0) fv = n; lv = n; }
      ++n;
      scan_shadow(s, x, m0 + u, ring, RS, W, J);
    }
  }
  int ix = s.head;
  for (int k = 0; k < W; ++k) {   // ring factors, oldest first (scan_finish's carry_out)
    carry[(int64_t)k * N + a] = ring[ix * RS];
    ix = (ix + 1 == W) ? 0 : ix + 1;
  }
  carry[(int64_t)W * N + a] = s.pff;
  carry[(int64_t)(W + 1) * N + a] = s.psff;
  uint8_t fl = 0;
  if (before && !(fv >= 0 && lv - fv >= W)) fl |= 1;
  double npm = absent_val();
  for (int f = 0; f < F && is_absent(npm); ++f) npm = PMh[(int64_t)(H + f) * N + a];
  if (after && is_absent(npm)) fl |= 2;
  next_pm[a] = npm;
  flags[a] = fl;
}

// This rank's exchange bits, one per asset, 64 per word (a wave's ballot), rows of nw words:
// 0 an uncertain carry and a present month in the shard; 1 an uncertain forward price and a
// pending ranked row at the shard's end; 2 a present month in the shard; 3 a present month
// before the shard's last Hn months (those in the next rank's halo).  The union below decides
// from every rank's rows which assets really need the exchange.
__global__ __launch_bounds__(256) void k_shard_need(const uint8_t* __restrict__ flags,
                                                    const double* __restrict__ st, int64_t N,
                                                    int T_m, int Hn, int64_t nw,
                                                    uint64_t* __restrict__ mask) {
  const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool c0 = false, c1 = false, pa = false, ph = false;
  if (a < N) {
    const uint8_t f = flags[a];
    pa = st[a] > 0.0;
    c0 = (f & 1) && pa;
    c1 = (f & 2) && st[N + a] >= 0.0;
    const double fm = st[3 * N + a];
    ph = fm >= 0.0 && fm < (double)(T_m - Hn);
  }
  const uint64_t b0 = __ballot(c0), b1 = __ballot(c1), b2 = __ballot(pa), b3 = __ballot(ph);
  if ((threadIdx.x & 63) == 0 && a < N) {
    const int64_t w = a >> 6;
    mask[w] = b0;
    mask[nw + w] = b1;
    mask[2 * nw + w] = b2;
    mask[3 * nw + w] = b3;
  }
}

// The assets that need the exchange on some rank, from every rank's k_shard_need rows
// [G][4][nw]: rank g needs asset a when its carry is uncertain and the asset has a row before
// g's halo (a row in a shard before g - 1, or in shard g - 1 before its last H months), or its
// forward price is uncertain and a later shard has a row -- otherwise the halo's state / ABSENT
// IS the whole history's.  The union as an ascending list of asset indices (the same on every
// rank): idx[0 .. min(count, cap)), *count = its full length (> cap: the list overflowed and
// the pass must take the all-gather path).  One workgroup.
#define UNION_THREADS 1024
__global__ __launch_bounds__(UNION_THREADS) void k_shard_union(const uint64_t* __restrict__ masks,
                                                               int G, int64_t nw, int64_t cap,
                                                               int32_t* __restrict__ idx,
                                                               int32_t* __restrict__ count) {
  __shared__ int32_t wsum[UNION_THREADS / 64];
  __shared__ int64_t base;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid == 0) base = 0;
  __syncthreads();
  auto row = [&](int g, int r, int64_t w) -> uint64_t { return masks[((int64_t)g * 4 + r) * nw + w]; };
  for (int64_t w0 = 0; w0 < nw; w0 += UNION_THREADS) {
    const int64_t w = w0 + tid;
    uint64_t u = 0;
    if (w < nw) {
      uint64_t later[HALO_MAXG];   // a row in a shard after g
      uint64_t suf = 0;
      for (int g = G - 1; g >= 0; --g) { later[g] = suf; suf |= row(g, 2, w); }
      uint64_t A = 0, B = 0, hp = 0;   // rows in shards < g - 1 / in g - 1 / in g - 1's head
      for (int g = 0; g < G; ++g) {
        const uint64_t hist = A | hp;   // a row before g's halo
        u |= (row(g, 0, w) & hist) | (row(g, 1, w) & later[g]);
        A |= B;
        B = row(g, 2, w);
        hp = row(g, 3, w);
      }
    }
    const int c = __popcll(u);
    int inc = c;   // wave inclusive scan, then the waves in order
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(inc, o, 64);
      if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[wid] = inc;
    __syncthreads();
    int64_t off = base + inc - c;
    for (int q = 0; q < wid; ++q) off += wsum[q];
    while (u) {
      const int b = __builtin_ctzll(u);
      u &= u - 1;
      if (off < cap) idx[off] = (int32_t)(w * 64 + b);
      ++off;
    }
    __syncthreads();
    if (tid == UNION_THREADS - 1) base = off;
    __syncthreads();
  }
  if (tid == 0) *count = (int32_t)(base < 0x7FFFFFFF ? base : 0x7FFFFFFF);
}

static int g_tune_cols_wg = 1;          // halo pass's listed columns: one workgroup per column (month prices into LDS) | 0 one thread per column
static const TuneKnob g_knobs[] = {
    {"cols_wg", &g_tune_cols_wg, [](int v) { return v == 0 || v == 1; }},
};
int csm_tune_shards(const char* key, int value) { return tune_set(g_knobs, key, value); }

void launch_shard_summary_chunked(hipStream_t st, const double* PM, int T_m, int64_t N, int T,
                                  int G, double* out) {
  hipLaunchKernelGGL(k_shard_summary_chunked, dim3((unsigned)((N + 255) / 256), (unsigned)G),
                     dim3(256), 0, st, PM, T_m, N, T, G, out);
}

void launch_fold_carry(hipStream_t st, const double* sm, int G, int g, int64_t N, int J, int skip,
                       double* carry, double* next_pm, const double* tail_pm, const FoldJs& jq,
                       double* psq) {
  hipLaunchKernelGGL(k_fold_carry, dim3((unsigned)((N + 255) / 256), (unsigned)(g < 0 ? G : 1)),
                     dim3(256), 0, st, sm, G, g, N, J, skip, carry, next_pm, tail_pm, jq, psq);
}

extern "C" {

int csm_shard_summary(csm_ctx* ctx, const double* PM, int32_t T_m, int64_t N, int32_t J,
                      int32_t skip, double* out) {
  int r = prep(ctx);
  if (r) return r;
  if (!PM || !out || N <= 0 || T_m < 0 || J < 1 || skip < 0 || J + skip > 256)
    return set_err(ctx, CSM_E_INVAL, "csm_shard_summary: bad arguments");
  // the whole shard as one chunk (T_m = 0: an empty chunk, the record with no present month)
  launch_shard_summary_chunked(ctx->stream, PM, T_m, N, J + skip + 1, 1, out);
  LAUNCH_CHECK(ctx, "k_shard_summary_chunked");
  return CSM_OK;
}

int csm_fold_carry(csm_ctx* ctx, const double* summaries, int32_t G, int32_t g, int64_t N,
                   int32_t J, int32_t skip, double* carry, double* next_pm) {
  int r = prep(ctx);
  if (r) return r;
  if (!summaries || !carry || !next_pm || N <= 0 || G < 1 || g < 0 || g >= G || J < 1 ||
      skip < 0 || J + skip > 256)
    return set_err(ctx, CSM_E_INVAL, "csm_fold_carry: bad arguments");
  launch_fold_carry(ctx->stream, summaries, G, g, N, J, skip, carry, next_pm, nullptr,
                    FoldJs{0, {0, 0, 0, 0}}, nullptr);
  LAUNCH_CHECK(ctx, "k_fold_carry");
  return CSM_OK;
}

int csm_shard_summary_state(csm_ctx* ctx, const double* P, const int64_t* month_start,
                            const double* PM, int32_t T_m, int64_t N, int32_t J, int32_t skip,
                            const double* state, double* out) {
  int r = prep(ctx);
  if (r) return r;
  if (!P || !month_start || !PM || !state || !out || N <= 0 || T_m < 1 || J < 1 || skip < 0 ||
      J + skip > 256)
    return set_err(ctx, CSM_E_INVAL, "csm_shard_summary_state: bad arguments");
  hipLaunchKernelGGL(k_shard_summary_state, dim3((unsigned)((N + 255) / 256)), dim3(256), 0,
                     ctx->stream, PM, P, month_start, T_m, N, J + skip + 1, state, out,
                     (const int32_t*)nullptr, (const int32_t*)nullptr, (int64_t)0);
  LAUNCH_CHECK(ctx, "k_shard_summary_state");
  return CSM_OK;
}

static int shard_repair(csm_ctx* ctx, const double* P, const int64_t* month_start, const double* PM,
                     int32_t T_m, int64_t N, int32_t J, int32_t skip, const double* carry,
                     const double* next_pm, const double* state, double* R, double* M,
                     double* NR, uint16_t* ids) {
  int r = prep(ctx);
  if (r) return r;
  if (!P || !month_start || !PM || !carry || !next_pm || !state || !M || !NR || N <= 0 ||
      T_m < 1 || J < 1 ||
      skip < 0 || J + skip > 128)
    return set_err(ctx, CSM_E_INVAL, "csm_shard_repair: bad arguments (J + skip <= 128)");
  const int W = J + skip;
  const size_t lds = (size_t)2 * W * REPAIR_THREADS * sizeof(double);
  if (lds > 65536)
    HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k_shard_repair,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_shard_repair, dim3((unsigned)((N + REPAIR_THREADS - 1) / REPAIR_THREADS)),
                     dim3(REPAIR_THREADS), lds, ctx->stream, PM, P, month_start, T_m, N, J, skip,
                     carry, next_pm, state, R, M, NR, ids, (const double*)nullptr,
                     (const int32_t*)nullptr, (const int32_t*)nullptr, (int64_t)0);
  LAUNCH_CHECK(ctx, "k_shard_repair");
  return CSM_OK;
}

int csm_shard_repair(csm_ctx* ctx, const double* P, const int64_t* month_start, const double* PM,
                     int32_t T_m, int64_t N, int32_t J, int32_t skip, const double* carry,
                     const double* next_pm, const double* state, double* R, double* M,
                     double* NR) {
  return shard_repair(ctx, P, month_start, PM, T_m, N, J, skip, carry, next_pm, state, R, M, NR,
                      nullptr);
}

int csm_shard_repair_ids(csm_ctx* ctx, const double* P, const int64_t* month_start,
                         const double* PM, int32_t T_m, int64_t N, int32_t J, int32_t skip,
                         const double* carry, const double* next_pm, const double* state,
                         double* R, double* M, double* NR, uint16_t* ids) {
  if (!ids) return set_err(ctx, CSM_E_INVAL, "csm_shard_repair_ids: ids is NULL");
  return shard_repair(ctx, P, month_start, PM, T_m, N, J, skip, carry, next_pm, state, R, M, NR,
                      ids);
}

// ---- halo date shards (k_shard_halo above; include/csmom.h) -------------------------------
int csm_shard_halo(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N,
                   const int64_t* month_start, int32_t H, int32_t T_m, int32_t F,
                   int32_t before, int32_t after, int32_t J, int32_t skip, double* halo_pm,
                   double* carry, double* next_pm, uint8_t* flags) {
  int r = prep(ctx);
  if (r) return r;
  if (!P || !month_start || !carry || !next_pm || !flags || (H + F > 0 && !halo_pm) || N <= 0 ||
      T_d <= 0 || H < 0 || T_m < 1 || F < 0 || F > 8 || J < 1 || skip < 0 || J + skip > 64)
    return set_err(ctx, CSM_E_INVAL, "csm_shard_halo: bad arguments (H >= 0, T_m >= 1, 0 <= F <= 8, "
                   "J + skip <= 64, halo_pm [H + F][N])");
  const int W = J + skip;
  const unsigned bx = (unsigned)((N + HALO_THREADS - 1) / HALO_THREADS);
  if (H + F > 0) {
    hipLaunchKernelGGL(k_halo_pm, dim3(bx, (unsigned)(H + F)), dim3(HALO_THREADS), 0, ctx->stream,
                       P, month_start, H, T_m, N, halo_pm);
    LAUNCH_CHECK(ctx, "k_halo_pm");
  }
  const size_t lds = (size_t)W * HALO_THREADS * sizeof(double);
  if (lds > 65536)
    HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k_shard_halo,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_shard_halo, dim3(bx), dim3(HALO_THREADS), lds, ctx->stream,
                     (const double*)halo_pm, H, F, before ? 1 : 0, after ? 1 : 0, N, J, skip, carry,
                     next_pm, flags);
  LAUNCH_CHECK(ctx, "k_shard_halo");
  return CSM_OK;
}

int csm_shard_need(csm_ctx* ctx, const uint8_t* flags, const double* state, int64_t N,
                   int32_t T_m, int32_t H, uint64_t* mask) {
  int r = prep(ctx);
  if (r) return r;
  if (!flags || !state || !mask || N <= 0 || T_m < 1 || H < 0)
    return set_err(ctx, CSM_E_INVAL, "csm_shard_need: bad arguments");
  hipLaunchKernelGGL(k_shard_need, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream,
                     flags, state, N, T_m, H, (N + 63) / 64, mask);
  LAUNCH_CHECK(ctx, "k_shard_need");
  return CSM_OK;
}

int csm_shard_union(csm_ctx* ctx, const uint64_t* masks, int32_t G, int64_t N, int64_t cap,
                    int32_t* idx, int32_t* count) {
  int r = prep(ctx);
  if (r) return r;
  if (!masks || !idx || !count || G < 1 || G > HALO_MAXG || N <= 0 || cap < 1 ||
      N > 0x7FFFFFFFLL)
    return set_err(ctx, CSM_E_INVAL, "csm_shard_union: bad arguments (1 <= G <= %d)", HALO_MAXG);
  hipLaunchKernelGGL(k_shard_union, dim3(1), dim3(UNION_THREADS), 0, ctx->stream, masks, G,
                     (N + 63) / 64, cap, idx, count);
  LAUNCH_CHECK(ctx, "k_shard_union");
  return CSM_OK;
}

int csm_shard_summary_cols(csm_ctx* ctx, const double* P, const int64_t* month_start,
                           const double* PM, int32_t T_m, int64_t N, int32_t J, int32_t skip,
                           const double* state, const int32_t* idx, const int32_t* count,
                           int64_t cap, double* out) {
  int r = prep(ctx);
  if (r) return r;
  if (!P || !month_start || !PM || !state || !idx || !count || !out || N <= 0 || T_m < 1 ||
      cap < 1 || J < 1 || skip < 0 || J + skip > 256)
    return set_err(ctx, CSM_E_INVAL, "csm_shard_summary_cols: bad arguments");
  // one workgroup per listed column, its month prices derived together into LDS
  if (g_tune_cols_wg && (size_t)T_m * sizeof(double) <= 65536 && cap <= 0x7FFFFFFF) {
    const int64_t grid = std::min<int64_t>(cap, 2 * (int64_t)ctx->n_cu);
    hipLaunchKernelGGL(k_shard_summary_cols, dim3((unsigned)grid), dim3(COLS_THREADS),
                       (size_t)T_m * sizeof(double), ctx->stream, PM, P, month_start, T_m, N,
                       J + skip + 1, state, out, idx, count, cap);
    LAUNCH_CHECK(ctx, "k_shard_summary_cols");
    return CSM_OK;
  }
  hipLaunchKernelGGL(k_shard_summary_state, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0,
                     ctx->stream, PM, P, month_start, T_m, N, J + skip + 1, state, out, idx,
                     count, cap);
  LAUNCH_CHECK(ctx, "k_shard_summary_state (columns)");
  return CSM_OK;
}

int csm_shard_repair_cols(csm_ctx* ctx, const double* P, const int64_t* month_start,
                          const double* PM, int32_t T_m, int64_t N, int32_t J, int32_t skip,
                          const double* carry, const double* next_pm, const double* fcarry,
                          const double* state, const int32_t* idx, const int32_t* count,
                          int64_t cap, double* R, double* M, double* NR, uint16_t* ids) {
  int r = prep(ctx);
  if (r) return r;
  if (!P || !month_start || !PM || !carry || !next_pm || !fcarry || !state || !idx || !count ||
      !M || !NR || N <= 0 || T_m < 1 || cap < 1 || J < 1 || skip < 0 || J + skip > 128)
    return set_err(ctx, CSM_E_INVAL, "csm_shard_repair_cols: bad arguments (J + skip <= 128)");
  const int W = J + skip;
  const size_t ldsc = (size_t)(T_m + 2 * W) * sizeof(double);
  if (g_tune_cols_wg && ldsc <= 65536 && cap <= 0x7FFFFFFF) {
    hipLaunchKernelGGL(k_shard_repair_cols, dim3((unsigned)cap), dim3(COLS_THREADS), ldsc,
                       ctx->stream, PM, P, month_start, T_m, N, J, skip, carry, next_pm, state,
                       R, M, NR, ids, fcarry, idx, count, cap);
    LAUNCH_CHECK(ctx, "k_shard_repair_cols");
    return CSM_OK;
  }
  const size_t lds = (size_t)2 * W * REPAIR_THREADS * sizeof(double);
  if (lds > 65536)
    HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k_shard_repair,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_shard_repair, dim3((unsigned)((cap + REPAIR_THREADS - 1) / REPAIR_THREADS)),
                     dim3(REPAIR_THREADS), lds, ctx->stream, PM, P, month_start, T_m, N, J, skip,
                     carry, next_pm, state, R, M, NR, ids, fcarry, idx, count, cap);
  LAUNCH_CHECK(ctx, "k_shard_repair (columns)");
  return CSM_OK;
}

int csm_shard_fix_cols(csm_ctx* ctx, const double* P, const int64_t* month_start,
                       const double* PM, int32_t T_m, int64_t N, int32_t J, int32_t skip,
                       const double* records, int32_t G, int32_t g, const int32_t* idx,
                       const int32_t* count, int64_t cap, double* R, double* M, double* NR,
                       uint16_t* ids) {
  int r = prep(ctx);
  if (r) return r;
  const int W = J + skip;
  const size_t lds = (size_t)(T_m + 2 * W + 2 + (size_t)G * (SUM_SCALARS + W + 1)) * sizeof(double);
  if (!P || !month_start || !PM || !records || !idx || !count || !M || !NR || N <= 0 ||
      T_m < 1 || cap < 1 || cap > 0x7FFFFFFF || G < 1 || g < 0 || g >= G || J < 1 || skip < 0 ||
      W > 128 || G > HALO_MAXG || lds > 65536)
    return set_err(ctx, CSM_E_INVAL, "csm_shard_fix_cols: bad arguments (J + skip <= 128, "
                   "0 <= g < G <= %d, months, rings and records within 64 KB of LDS)", HALO_MAXG);
  // a workgroup per listed column, at most two per CU (the list is short; the rest exit at once)
  const int64_t grid = cap < 2 * (int64_t)ctx->n_cu ? cap : 2 * (int64_t)ctx->n_cu;
  // (C4's look-back J = 12, skip = 1: the ring in registers and the product length fixed)
  const void* fn = (J == 12 && skip == 1) ? (const void*)k_shard_fix_cols<13, 12>
                                          : (const void*)k_shard_fix_cols<0, 0>;
  {
    int T_m_ = T_m, J_ = J, skip_ = skip, G_ = G, g_ = g;
    int64_t N_ = N, cap_ = cap;
    void* args[] = {(void*)&PM, (void*)&P, (void*)&month_start, &T_m_, &N_, &J_, &skip_,
                    (void*)&records, &G_, &g_, (void*)&R, (void*)&M, (void*)&NR, (void*)&ids,
                    (void*)&idx, (void*)&count, &cap_};
    HIP_CHECK(ctx, hipLaunchKernel(fn, dim3((unsigned)grid), dim3(COLS_THREADS), args, lds,
                                   ctx->stream));
  }
  LAUNCH_CHECK(ctx, "k_shard_fix_cols");
  return CSM_OK;
}

}  // extern "C"
