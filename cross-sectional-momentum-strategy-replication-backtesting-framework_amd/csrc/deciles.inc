// deciles.inc -- the per-date qcut kernel (k_deciles), included by deciles_wide.hip (wide rows:
// DEC_THREADS 512, HB 8192 buckets, CAP 4096 candidates; 8192 rather than 4096 buckets halves
// the target-bucket populations and cut C4's selection + gather time by a third) and by
// deciles_narrow.hip (rows of a few thousand assets: 256 threads, 1024 buckets, 2048
// candidates -- a sixth of the LDS, so several times the workgroups per CU).  The includer defines DEC_THREADS, HB, CAP and wraps
// the include in its own namespace.
constexpr int kThreads = DEC_THREADS;
#ifndef DEC_MLU
#define DEC_MLU 4   // PRE merged sweep: 4-cell groups of ids + next_ret in flight per lane
#endif
#ifndef DEC_SCH
#define DEC_SCH 32   // pass 0 samples: DEC_SCH chunks of 64 consecutive assets
#endif
// DEC_CHUNK_ORDER (wide rows on ids, deciles_pre.hip): the merged pass restarts each lane's
// next_ret sums at every chunk of sp.cells cells (whole sweep trips) and adds the lane's chunk
// partials in chunk order -- exactly what a split-pass sweep lane writes per chunk and the split
// finish adds up.  The two passes then sum every row in one order: a date shard of a few dozen
// rows (split pass) and the one-GPU pass (merged) give the same decile means bit for bit, on any
// CU count.
#ifndef DEC_CHUNK_ORDER
#define DEC_CHUNK_ORDER 0
#endif
constexpr int kHbBits = __builtin_ctz(HB);   // key-space refinement splits into HB sub-buckets
// PRE: the fixed map's ids (CSM_FB_BUCKETS buckets) coarsened to HB buckets by a right shift
// (monotone), NaN ids kept
constexpr int kFbs = HB <= CSM_FB_BUCKETS ? __builtin_ctz(CSM_FB_BUCKETS) - kHbBits : 0;
template <bool PRE>
__device__ __forceinline__ uint32_t dec_uid(uint32_t v) {
  return (!PRE || kFbs == 0 || v == 0xFFFFu) ? v : (v >> kFbs);
}
__device__ __forceinline__ int pre_bucket(double x) { return csm_fbucket(x) >> kFbs; }
static_assert((1 << kHbBits) == HB, "HB must be a power of two");
// =====================================================================================
// Kernel C: per-date qcut labels + fused equal-weight decile means (K = 1).
// One workgroup per date.  Exact order statistics by bucket-select:
//   pass 0  bucketing range from a 2048-value sample (0.2 % / 99.8 % order statistics)
//   pass 1  HB-bucket histogram, linear in value over that range (monotone: out-of-range
//           values clamp into the end buckets) + exact count / min / max
//   (rare)  oversized target buckets are refined in key space (order-preserving u64 keys)
//   pass 3  gather the target buckets' members into LDS; counting selection (bitonic sort
//           for big slots) gives the order statistics
//   pass 4  edges (NumPy lerp) -> dedupe -> bucket->label table -> labels; next_ret summed
//           per label in a fixed order
// =====================================================================================


__device__ __forceinline__ uint64_t dkey(double x) {
  const uint64_t b = (uint64_t)__double_as_longlong(x + 0.0);  // -0.0 -> +0.0
  return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
__device__ __forceinline__ double dval(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFULL) : ~k;
  return __longlong_as_double((long long)b);
}

struct Slot {
  uint64_t klo, khi;  // key interval (inclusive) inside value bucket b0
  int b0;
  int count;          // members
  int off;            // candidate offset
  int resolved;       // all members share one key -> value known
  double value;
};

struct DecShared {
  uint32_t hist[HB];
  double cand[CAP];
  Slot slots[MAXT];
  int64_t trank[MAXT];  // target ranks (sorted, distinct)
  int64_t tres[MAXT];   // residual rank inside its slot
  int tslot[MAXT];
  double tval[MAXT];
  int nslot, ntgt, total;
  double vmin, vmax, scale;
  uint64_t kmin_r, kmax_r;
  double bins[MAXQ];
  int nbins;
  int64_t n;
  int fill[MAXT];
  union {
    struct {              // key-space refinement scratch
      Slot slots2[MAXT];
      int remap[MAXT];
    } rf;
    struct {              // PRE merged pass (never runs with a refinement)
      int rlo[MAXQ], rhi[MAXQ];   // bucket range of each edge's order statistics
      int plo[MAXQ], phi[MAXQ];   // buckets of ranks floor(v_k), floor(v_k) + 1 (targets pass)
      double fh[MAXQ], fl[MAXQ];  // certain cells' next_ret totals per label
      int fcn[MAXQ];
    } mg;
  } x;
  int vbe[MAXQ];          // bucket of each bin edge
  alignas(16) int8_t blab[HB];   // bucket -> label (-1 NaN label, -2 bucket holds an edge: compare exactly)
  // reduction scratch
  double red_d[DEC_THREADS / 64][2];
  double red_d2[DEC_THREADS / 64][2];
  unsigned long long red_k[DEC_THREADS / 64][2];
  int64_t red_n[DEC_THREADS / 64];
  int red_n2[DEC_THREADS / 64][2];
  int tpre[MAXT + 1];   // prefix of unresolved member counts over the targets
  int sel_count;        // 1: counting selection, 0: bitonic sort
  int bext[2];          // PRE: lowest / highest non-empty bucket (they hold the min / max)
  int fast, ovf;        // PRE merged pass: taken / a wave's uncertain-cell list overflowed
};

// Monotone non-decreasing in x for any lo / scale (values outside [lo, lo + HB/scale)
// clamp into the end buckets), so bucket order never contradicts value order.  Branch-free:
// fmax/fmin clamp (NaN -> bucket 0; callers never count NaN), truncation = floor on [0, HB).
__device__ __forceinline__ int vbucket(double x, double lo, double scale) {
  const double f = fmin(fmax((x - lo) * scale, 0.0), (double)(HB - 1));
  return (int)f;
}

// Row sweep with ROW_U independent 16-B (or 8-B) loads issued per lane before use, so a
// 512-thread block keeps ROW_U KiB x 8 waves in flight.
#ifndef ROW_U
#define ROW_U 8
#endif
// label pass: V2 pairs of M and NR loaded per lane before use
#ifndef DEC_LU
#define DEC_LU 4
#endif
// REV walks the row's blocks from the end: a pass right after a forward pass then re-reads
// the most recently touched part of the row first, while it is still in the Infinity Cache
// (all dates' rows together exceed its 256 MB at C4, so the row's head has been evicted).
template <bool V2, bool REV = false, typename F>
__device__ __forceinline__ void for_row(const double* __restrict__ row, int64_t N, F&& f) {
  if (REV) {
    const int64_t step = (V2 ? 2 : 1) * DEC_THREADS;
    const int64_t blk = ROW_U * step;
    const int64_t i0 = (V2 ? 2 : 1) * (int64_t)threadIdx.x;
    for (int64_t b = (N + blk - 1) / blk - 1; b >= 0; --b) {
      const int64_t base = b * blk + i0;
      if (V2) {
        double2 v[ROW_U];
#pragma unroll
        for (int u = 0; u < ROW_U; ++u) {
          const int64_t i = base + u * step;
          v[u] = i < N ? *reinterpret_cast<const double2*>(row + i) : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int u = 0; u < ROW_U; ++u) {
          const int64_t i = base + u * step;
          if (i < N) { f(i, v[u].x); f(i + 1, v[u].y); }
        }
      } else {
        double v[ROW_U];
#pragma unroll
        for (int u = 0; u < ROW_U; ++u) {
          const int64_t i = base + u * step;
          v[u] = i < N ? row[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < ROW_U; ++u) {
          const int64_t i = base + u * step;
          if (i < N) f(i, v[u]);
        }
      }
    }
    return;
  }
  if (V2) {
    const int64_t step = 2 * DEC_THREADS;
    int64_t i = 2 * (int64_t)threadIdx.x;
    for (; i + (ROW_U - 1) * step < N; i += ROW_U * step) {
      double2 v[ROW_U];
#pragma unroll
      for (int u = 0; u < ROW_U; ++u) v[u] = *reinterpret_cast<const double2*>(row + i + u * step);
#pragma unroll
      for (int u = 0; u < ROW_U; ++u) { f(i + u * step, v[u].x); f(i + u * step + 1, v[u].y); }
    }
    for (; i < N; i += step) {
      const double2 t = *reinterpret_cast<const double2*>(row + i);
      f(i, t.x);
      f(i + 1, t.y);
    }
  } else {
    const int64_t step = DEC_THREADS;
    int64_t i = threadIdx.x;
    for (; i + (ROW_U - 1) * step < N; i += ROW_U * step) {
      double v[ROW_U];
#pragma unroll
      for (int u = 0; u < ROW_U; ++u) v[u] = row[i + u * step];
#pragma unroll
      for (int u = 0; u < ROW_U; ++u) f(i + u * step, v[u]);
    }
    for (; i < N; i += step) f(i, row[i]);
  }
}

__device__ __forceinline__ double wave_sum_d(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// Block-wide (min, max) and (sum, sum) over DEC_THREADS; every thread gets the results.
// Two barriers each (the scratch is reusable on return).
__device__ __forceinline__ void block_minmax(double mn, double mx, double& gmn, double& gmx,
                                             double (*scr)[2]) {
  for (int o = 32; o > 0; o >>= 1) {
    mn = fmin(mn, __shfl_down(mn, o, 64));
    mx = fmax(mx, __shfl_down(mx, o, 64));
  }
  if ((threadIdx.x & 63) == 0) { scr[threadIdx.x >> 6][0] = mn; scr[threadIdx.x >> 6][1] = mx; }
  __syncthreads();
  gmn = INFINITY; gmx = -INFINITY;
#pragma unroll
  for (int w = 0; w < DEC_THREADS / 64; ++w) { gmn = fmin(gmn, scr[w][0]); gmx = fmax(gmx, scr[w][1]); }
  __syncthreads();
}
__device__ __forceinline__ void block_sum2(int a, int b, int& ga, int& gb, int (*scr)[2]) {
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o, 64); b += __shfl_down(b, o, 64); }
  if ((threadIdx.x & 63) == 0) { scr[threadIdx.x >> 6][0] = a; scr[threadIdx.x >> 6][1] = b; }
  __syncthreads();
  ga = 0; gb = 0;
#pragma unroll
  for (int w = 0; w < DEC_THREADS / 64; ++w) { ga += scr[w][0]; gb += scr[w][1]; }
  __syncthreads();
}

// Exclusive scan of hist[HB] in place (hist[b] becomes the count of buckets < b): per-thread
// sums of 8 consecutive buckets, a wave scan by shuffles, then the wave totals.  Two barriers.
__device__ void block_exclusive_scan_hist(uint32_t* hist) {
  __shared__ uint32_t wtot[DEC_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  constexpr int per = HB / DEC_THREADS;  // 8
  uint32_t loc[per];
  uint32_t s = 0;
#pragma unroll
  for (int j = 0; j < per; ++j) { loc[j] = hist[tid * per + j]; s += loc[j]; }
  uint32_t inc = s;  // inclusive wave scan
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) wtot[wid] = inc;
  __syncthreads();
  uint32_t run = inc - s;
  for (int w = 0; w < wid; ++w) run += wtot[w];
#pragma unroll
  for (int j = 0; j < per; ++j) { hist[tid * per + j] = run; run += loc[j]; }
  __syncthreads();
}

// member test for a slot (value bucket b0 and key interval)
__device__ __forceinline__ bool slot_member(const Slot& s, int b, uint64_t k) {
  return b == s.b0 && k >= s.klo && k <= s.khi;
}

// =====================================================================================
// The split decile pass on ids (wide rows; deciles_pre.hip): the merged pass's work as three
// launches so that the bandwidth-bound part is balanced over the whole chip and no row's
// serial phases hold a CU's share of the sweep:
//   plan   (k_deciles<.., MG, SPLIT = 1>, one workgroup per date): id histogram, target
//          ranks, the edges' bucket ranges, the bucket -> label table; stores the table and the
//          row's slots / targets (DsPlan) -- or leaves the row to the general kernel (FLG = 1)
//   sweep  (k_dsplit_sweep, one workgroup per (sp.cells-cell chunk, date)): ids + next_ret
//          of the chunk -> labels of the certain cells, each lane's next_ret sums per label
//          (the merged pass's lane of that index sweeps the same cells in the same order), and
//          the uncertain cells (those in a target bucket) listed per (chunk, wave)
//   finish (k_deciles<.., SPLIT = 2>, one workgroup per date): each wave's lists in chunk order
//          (the merged pass's wave list), the listed cells' mom_J into the slots, selection,
//          exact edges; every lane's chunk partials in chunk order and the listed cells summed
//          as the merged pass sums them -> EW / CNT.  Rows with FLG = 1 (or a wave list longer
//          than the merged pass's) run the general kernel there instead.
// Chunks are fixed by N alone and the merged pass sums in the same order (DEC_CHUNK_ORDER), so
// a row's means do not depend on which pass, or how many rows a launch holds (date shards
// equal the one-GPU pass bit for bit).
// =====================================================================================
struct DsPlan {
  int64_t n;
  int nslot, ntgt, total, pad_;
  Slot slots[MAXT];
  int64_t trank[MAXT];
  int64_t tres[MAXT];
  int tslot[MAXT];
};
static_assert(sizeof(DsPlan) <= DSPLAN_BYTES, "DsPlan outgrew its slot in the workspace");

// plan: the table and the row's selection state for the finish launch
__device__ __forceinline__ void dsplit_store(const DecShared& S, int t, int64_t n, const DecSplit& sp) {
  const int tid = threadIdx.x;
  const uint4* src = reinterpret_cast<const uint4*>(S.blab);
  uint4* dst = reinterpret_cast<uint4*>(sp.tab + (int64_t)t * HB);
  for (int i = tid; i < HB / 16; i += DEC_THREADS) dst[i] = src[i];
  DsPlan* P = reinterpret_cast<DsPlan*>(sp.plan + (int64_t)t * DSPLAN_BYTES);
  if (tid == 0) { P->n = n; P->nslot = S.nslot; P->ntgt = S.ntgt; P->total = S.total; }
  if (tid < MAXT) {
    P->slots[tid] = S.slots[tid];
    P->trank[tid] = S.trank[tid];
    P->tres[tid] = S.tres[tid];
    P->tslot[tid] = S.tslot[tid];
  }
}

// finish: everything of the merged pass after its sweep, for one row whose sweep ran as chunks
// (the same arithmetic in the same order: see DEC_CHUNK_ORDER).  Returns false -- the general
// path takes the row -- when a wave's lists outgrow the merged pass's per-wave list, as the
// merged pass then gives the row up too.
template <int NB>
__device__ __forceinline__ bool dsplit_finish(DecShared& S, int t, const double* __restrict__ row,
                                              const double* __restrict__ nrow, int n_bins,
                                              const QTab& qt, int8_t* __restrict__ lrow,
                                              double* __restrict__ EW, int32_t* __restrict__ CNT,
                                              const DecSplit& sp) {
  constexpr int NBA = NB > 0 ? NB : 1;
  static_assert(DEC_THREADS == SPLIT_THREADS, "the finish's waves are the sweep's");
  constexpr int FL = HB / (DEC_THREADS / 64);   // the merged pass's per-wave list
  static_assert(FL == SPLIT_FL, "a sweep wave's chunk list fits the merged pass's wave list");
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const DsPlan* P = reinterpret_cast<const DsPlan*>(sp.plan + (int64_t)t * DSPLAN_BYTES);
  const int64_t n = P->n;
  const int C = sp.C;
  __shared__ int fovf;
  if (tid == 0) { S.nslot = P->nslot; S.ntgt = P->ntgt; fovf = 0; }
  if (tid < MAXT) {
    S.slots[tid] = P->slots[tid];
    S.trank[tid] = P->trank[tid];
    S.tres[tid] = P->tres[tid];
    S.tslot[tid] = P->tslot[tid];
    S.fill[tid] = 0;
  }
  {
    const uint4* src = reinterpret_cast<const uint4*>(sp.tab + (int64_t)t * HB);
    uint4* dst = reinterpret_cast<uint4*>(S.blab);
    for (int i = tid; i < HB / 16; i += DEC_THREADS) dst[i] = src[i];
  }
  // the certain cells' lane partials of the first chunks, loaded now (their latency under the
  // list and selection work below); summed per lane in chunk order further down
  constexpr int LPB = 4;   // chunks per batch of partial loads
  double lpp[LPB][NBA];
  auto lp_load = [&](int c0) {
#pragma unroll
    for (int cc = 0; cc < LPB; ++cc) {
      const double* lp = sp.lp + ((int64_t)t * C + c0 + cc) * (MAXQ - 1) * SPLIT_THREADS + tid;
#pragma unroll
      for (int d = 0; d < NBA; ++d) lpp[cc][d] = (NB > 0 && nrow && EW && c0 + cc < C) ? lp[d * SPLIT_THREADS] : 0.0;
    }
  };
  lp_load(0);
  // wave w's list: its (chunk, w) lists in chunk order (the merged pass's wave-w list); the
  // wave's C counts in one load (lane c: chunk c), their prefix by shuffles
  uint32_t* flist = S.hist + wid * FL;
  int fc = 0;   // wave-uniform
  for (int c0 = 0; c0 < C; c0 += 64) {
    const int c = c0 + lane;
    const int cnt = c < C ? sp.ucnt[((int64_t)t * C + c) * SPLIT_WAVES + wid] : 0;
    int inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(inc, o, 64);
      if (lane >= o) inc += v;
    }
    const int tot = __shfl(inc, 63, 64);
    const int nc = C - c0 < 64 ? C - c0 : 64;
    for (int k = 0; k < nc; ++k) {   // (wave-uniform) chunk c0 + k's list at its offset
      const int ck = __shfl(cnt, k, 64), ok = fc + __shfl(inc, k, 64) - ck;
      if (ok + ck <= FL) {
        const uint32_t* src = sp.ulist + (((int64_t)t * C + c0 + k) * SPLIT_WAVES + wid) * SPLIT_FL;
        for (int j = lane; j < ck; j += 64) flist[ok + j] = src[j];
      }
    }
    fc += tot;
  }
  if (fc > FL && lane == 0) fovf = 1;
  __syncthreads();
  if (fovf) return false;   // (block-uniform)
  // the listed cells' values into their slots (the merged pass's gather); their mom_J and
  // next_ret stay in registers for the labels below (a wave lists at most FL = 8 trips of 128)
  constexpr int FT = FL / 128;
  double xa[FT][2], ra[FT][2];
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int q = 0; q < FT; ++q) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = q * 128 + lane + 64 * h;
      const int ci = j < fc ? (int)flist[j] : 0;
      xa[q][h] = j < fc ? row[ci] : 0.0;
      ra[q][h] = (j < fc && NB > 0 && nrow && EW) ? nrow[ci] : 0.0;
    }
  }
#pragma unroll
  for (int q = 0; q < FT; ++q) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (q * 128 + lane + 64 * h >= fc) continue;
      const double x = xa[q][h];
      const int sl = -3 - (int)S.blab[pre_bucket(x)];
      if (sl >= 0) {
        const int pos = atomicAdd(&S.fill[sl], 1);
        S.cand[S.slots[sl].off + pos] = x;
      }
    }
  }
  __syncthreads();
  int nb = 0;
  {   // (block-uniform) order statistics inside the slots: counting selection or a bitonic sort
    if (wid == 0) {
      const int ntg = S.ntgt;
      int c = 0;
      if (lane < ntg) {
        const Slot& sl = S.slots[S.tslot[lane]];
        c = sl.resolved ? 0 : sl.count;
      }
      int inc = c;
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
      }
      if (lane < ntg) S.tpre[lane + 1] = inc;
      int64_t work = (int64_t)c * c;
      for (int o = 32; o > 0; o >>= 1) work += __shfl_xor(work, o, 64);
      if (lane == 0) { S.tpre[0] = 0; S.sel_count = work <= (int64_t)DEC_THREADS * 512; }
    }
    __syncthreads();
    if (S.sel_count) {
      const int ntg = S.ntgt, tot = S.tpre[ntg];
      for (int p = tid; p < tot; p += DEC_THREADS) {
        int t2 = 0, hi3 = ntg - 1;
        while (t2 < hi3) {
          const int mid = (t2 + hi3 + 1) >> 1;
          if (S.tpre[mid] <= p) t2 = mid; else hi3 = mid - 1;
        }
        const Slot& sl = S.slots[S.tslot[t2]];
        const int i = p - S.tpre[t2];
        const double* c = S.cand + sl.off;
        const double x = c[i];
        int rank = 0;
        for (int j = 0; j < sl.count; ++j) {
          const double y = c[j];
          rank += (y < x || (y == x && j < i)) ? 1 : 0;
        }
        if (rank == S.tres[t2]) S.tval[t2] = x;
      }
      if (tid < ntg) {
        const Slot& sl = S.slots[S.tslot[tid]];
        if (sl.resolved) S.tval[tid] = sl.value;
      }
    } else {
      int tot = 0;
      for (int i = 0; i < S.nslot; ++i) tot += S.slots[i].resolved ? 0 : S.slots[i].count;
      int P2 = 1;
      while (P2 < tot) P2 <<= 1;
      for (int i = tot + tid; i < P2; i += DEC_THREADS) S.cand[i] = INFINITY;
      __syncthreads();
      for (int k = 2; k <= P2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int i = tid; i < P2; i += DEC_THREADS) {
            const int ixj = i ^ j;
            if (ixj > i) {
              const double x = S.cand[i], y = S.cand[ixj];
              const bool up = (i & k) == 0;
              if ((x > y) == up) { S.cand[i] = y; S.cand[ixj] = x; }
            }
          }
          __syncthreads();
        }
      }
      if (tid < S.ntgt) {
        const Slot& sl = S.slots[S.tslot[tid]];
        S.tval[tid] = sl.resolved ? sl.value : S.cand[sl.off + S.tres[tid]];
      }
    }
    __syncthreads();
    // edges (NumPy _lerp) by wave 0; the first / last edge are placeholders (-DBL_MAX /
    // DBL_MAX): every listed cell lies strictly between the extreme buckets.  The plan took the
    // row only with pairwise disjoint edge ranges, so no two edges are equal (nothing dropped).
    if (wid == 0) {
      const double vmin = -__DBL_MAX__, vmax = __DBL_MAX__;
      auto order_stat = [&](int64_t r) -> double {
        if (r <= 0) return vmin;
        if (r >= n - 1) return vmax;
        int lo2 = 0, hi2 = S.ntgt - 1;
        while (lo2 < hi2) { const int mid = (lo2 + hi2) >> 1; if (S.trank[mid] < r) lo2 = mid + 1; else hi2 = mid; }
        return S.tval[lo2];
      };
      const int k = lane;
      if (k <= n_bins) {
        double ek;
        const double v = (double)(n - 1) * qt.q[k];
        if (v >= (double)(n - 1)) {
          ek = vmax;
        } else {
          const double p = floor(v);
          const double g = v - p;
          const int64_t pi = (int64_t)p;
          const double a = order_stat(pi);
          const double b = (g != 0.0) ? order_stat(pi + 1) : a;
          const double d = b - a;
          ek = (g >= 0.5) ? (b - d * (1.0 - g)) : (a + d * g);
        }
        S.bins[k] = ek;
      }
      if (lane == 0) S.nbins = n_bins + 1;
    }
    __syncthreads();
    nb = S.nbins;
  }
  const double* bins = S.bins;
  auto exact = [&](double x) {
    int ids = 0;
    for (int j = 0; j < nb; ++j) ids += (bins[j] < x) ? 1 : 0;
    return (ids == 0 || ids == nb) ? -1 : ids - 1;
  };
  if (NB == 0 || !nrow || !EW) {   // labels only: the listed cells' exact labels
#pragma unroll
    for (int q = 0; q < FT; ++q) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int j = q * 128 + lane + 64 * h;
        if (j < fc) lrow[flist[j]] = (int8_t)exact(xa[q][h]);
      }
    }
    return true;
  }
  // deterministic block reduction (the merged pass's block_sums): wave shfl_down trees, then the
  // waves in order (two-sum); thread d < NB gets label d's (high, low, count)
  __shared__ double fwh[DEC_THREADS / 64][NBA], fwl[DEC_THREADS / 64][NBA];
  __shared__ int fwc[DEC_THREADS / 64][NBA];
  double hs[NBA];
  int cn[NBA];
  auto bsum = [&](double& oh, double& ol, int& oc) {
#pragma unroll
    for (int d = 0; d < NB; ++d) {
      double h = hs[d], l = 0.0;
      int c = cn[d];
      for (int o = 32; o > 0; o >>= 1) {
        const double h2 = __shfl_down(h, o, 64), l2 = __shfl_down(l, o, 64);
        const int c2 = __shfl_down(c, o, 64);
        const double s2 = h + h2;
        const double bb = s2 - h;
        const double err = (h - (s2 - bb)) + (h2 - bb);
        h = s2; l = (l + l2) + err; c += c2;
      }
      if (lane == 0) { fwh[wid][d] = h; fwl[wid][d] = l; fwc[wid][d] = c; }
    }
    __syncthreads();
    if (tid < NB) {
      const int d = tid;
      double h = 0.0, l = 0.0;
      int c = 0;
      for (int w = 0; w < DEC_THREADS / 64; ++w) {
        const double h2 = fwh[w][d];
        const double s2 = h + h2;
        const double bb = s2 - h;
        const double err = (h - (s2 - bb)) + (h2 - bb);
        h = s2; l = (l + fwl[w][d]) + err; c += fwc[w][d];
      }
      oh = h; ol = l; oc = c;
    }
    __syncthreads();
  };
  // the certain cells: each lane's chunk partials in chunk order (the merged lane's sum)
#pragma unroll
  for (int d = 0; d < NBA; ++d) { hs[d] = 0.0; cn[d] = 0; }
  for (int c0 = 0; c0 < C; c0 += LPB) {
    if (c0 > 0) lp_load(c0);
#pragma unroll
    for (int cc = 0; cc < LPB; ++cc) {
      if (c0 + cc >= C) break;
#pragma unroll
      for (int d = 0; d < NB; ++d) hs[d] += lpp[cc][d];
    }
  }
  double ch = 0.0, cl = 0.0;
  int cc = 0;
  bsum(ch, cl, cc);
  if (tid < NB) {
    cc = 0;   // (integer counts: the chunks' totals)
    for (int c = 0; c < C; ++c) cc += sp.pc[((int64_t)t * C + c) * MAXQ + tid];
  }
  // the listed cells: exact labels, next_ret per wave in list order (the merged pass's tail:
  // entries j0 + lane, then j0 + 64 + lane, trips of 128)
#pragma unroll
  for (int d = 0; d < NBA; ++d) { hs[d] = 0.0; cn[d] = 0; }
  auto accumulate = [&](int lab, double r) {
    const bool ok = lab >= 0 && !isnan_d(r);
#pragma unroll
    for (int d = 0; d < NB; ++d) {
      const bool h = ok && lab == d;
      hs[d] += h ? r : 0.0;
      cn[d] += h ? 1 : 0;
    }
  };
#pragma unroll
  for (int q = 0; q < FT; ++q) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = q * 128 + lane + 64 * h;
      if (j >= fc) continue;
      const int l = exact(xa[q][h]);
      lrow[flist[j]] = (int8_t)l;
      accumulate(l, ra[q][h]);
    }
  }
  double fh = 0.0, fl = 0.0;
  int fcn = 0;
  bsum(fh, fl, fcn);
  if (tid < NB) {
    const int d = tid;
    double h = fh, l = fl;
    int c = fcn;
    {   // the certain cells' totals after the listed cells' (the merged pass's order)
      const double h2 = ch;
      const double s2 = h + h2;
      const double bb = s2 - h;
      const double err = (h - (s2 - bb)) + (h2 - bb);
      h = s2; l = (l + cl) + err; c += cc;
    }
    const double sum = (h - h == 0.0) ? h + l : h;   // inf sums stay inf (pandas' mean)
    EW[(int64_t)t * NB + d] = c > 0 ? sum / (double)c : qnan();
    if (CNT) CNT[(int64_t)t * NB + d] = c;
  }
  return true;
}

// sweep: one workgroup per (chunk, date).  The merged pass's sweep on sp.cells cells: the
// row's table staged in LDS, ids + next_ret with DEC_MLU 4-cell groups in flight per lane,
// labels of the certain cells written, their next_ret summed per lane and label (lane tid sweeps
// the cells lane tid of the merged pass sweeps there, in the same order), the uncertain cells
// (table <= -2) listed per wave.  A wave list overflow leaves the row to the general kernel.
// PF: the next trip's loads in flight while this trip is labelled (one workgroup per CU: the
// launch has no more (chunk, date) pairs than CUs); !PF: no prefetch, <= 128 VGPRs, two
// workgroups per CU for the launches with more pairs than CUs (4-way C4 shards: 115 rows x 4
// chunks; the prefetching kernel's 153 VGPRs run those in two rounds)
template <int NB, bool PF>
__global__ __launch_bounds__(SPLIT_THREADS) __attribute__((amdgpu_waves_per_eu(PF ? 1 : 4)))
void k_dsplit_sweep(
    const double* __restrict__ NRx, const uint16_t* __restrict__ IDSx, int64_t N,
    int8_t* __restrict__ L, int32_t* __restrict__ FLG, DecSplit sp) {
  static_assert(SPLIT_THREADS == DEC_THREADS && 4 * DEC_MLU * DEC_THREADS == SPLIT_TRIP,
                "a sweep lane is the merged pass's lane, a chunk whole merged-sweep trips");
  constexpr int NBA = NB > 0 ? NB : 1;
  const int c = blockIdx.x, t = blockIdx.y;
  if (FLG[t] != 0) return;   // the plan left the row to the general kernel
  __shared__ __attribute__((aligned(16))) int8_t tab[HB];
  __shared__ uint32_t lst[SPLIT_WAVES][SPLIT_FL];
  __shared__ int swc[SPLIT_WAVES][NBA];
  __shared__ int ovf;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  {
    const uint4* src = reinterpret_cast<const uint4*>(sp.tab + (int64_t)t * HB);
    uint4* dst = reinterpret_cast<uint4*>(tab);
    for (int i = tid; i < HB / 16; i += SPLIT_THREADS) dst[i] = src[i];
  }
  if (tid == 0) ovf = 0;
  __syncthreads();
  const int64_t a0 = (int64_t)c * sp.cells;
  const int64_t a1 = a0 + sp.cells < N ? a0 + sp.cells : N;
  const uint16_t* irow = IDSx + (int64_t)t * N;
  const double* nrow = NRx ? NRx + (int64_t)t * N : nullptr;
  int8_t* lrow = L + (int64_t)t * N;
  double hs[NBA];
  int cn[NBA];
#pragma unroll
  for (int d = 0; d < NBA; ++d) { hs[d] = 0.0; cn[d] = 0; }
  uint32_t* flist = lst[wid];
  int fc = 0;            // wave-uniform
  bool fovf = false;     // wave-uniform
  const int64_t step = 4 * SPLIT_THREADS;
  constexpr int LU4 = DEC_MLU;
  // the next trip's ids + next_ret are loaded while this trip's are labelled and summed (a
  // sweep workgroup is alone on its CU: registers to spare, and its loads in flight are what
  // bound it); the lane's cells and their order are the merged pass's
  auto load_trip = [&](int64_t base, uint2 (&pk)[LU4], double2 (&ra)[LU4], double2 (&rb)[LU4]) {
    const int64_t i0 = base + 4 * (int64_t)tid;
#pragma unroll
    for (int u = 0; u < LU4; ++u) {
      const int64_t i = i0 + u * step;
      pk[u] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
      ra[u] = make_double2(0.0, 0.0);
      rb[u] = make_double2(0.0, 0.0);
      if (i < a1) {
        pk[u] = *reinterpret_cast<const uint2*>(irow + i);
        if (NB > 0 && nrow) {
          ra[u] = *reinterpret_cast<const double2*>(nrow + i);
          rb[u] = *reinterpret_cast<const double2*>(nrow + i + 2);
        }
      }
    }
  };
  uint2 pk[LU4];
  double2 ra[LU4], rb[LU4];
  if (PF) load_trip(a0, pk, ra, rb);
  for (int64_t base = a0; base < a1; base += LU4 * step) {   // block-uniform trips
    const int64_t i0 = base + 4 * (int64_t)tid;
    uint2 pkn[LU4];
    double2 ran[LU4], rbn[LU4];
    if (PF)
      load_trip(base + LU4 * step, pkn, ran, rbn);   // (past the chunk: nothing loaded)
    else
      load_trip(base, pk, ra, rb);
    static_assert(4 * LU4 < 64, "6-bit packed label counts per batch");
    uint64_t pc = 0;
    uint32_t lw[LU4];
    uint32_t um = 0;
#pragma unroll
    for (int u = 0; u < LU4; ++u) {
      asm volatile("" ::: "memory");
      const uint32_t id[4] = {dec_uid<true>(pk[u].x & 0xFFFFu), dec_uid<true>(pk[u].x >> 16),
                              dec_uid<true>(pk[u].y & 0xFFFFu), dec_uid<true>(pk[u].y >> 16)};
      uint32_t w = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        int l = id[k] == 0xFFFFu ? -1 : (int)tab[id[k]];
        const bool un = l <= -2;
        um |= (un ? 1u : 0u) << (4 * u + k);
        l = un ? -3 : l;
        w |= (uint32_t)(uint8_t)(int8_t)l << (8 * k);
      }
      lw[u] = w;
    }
    const int nh = __popc(um);
    int inc = nh;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(inc, o, 64);
      if (lane >= o) inc += v;
    }
    const int tot = __shfl(inc, 63, 64);
    if (tot) {   // wave-uniform
      if (fc + tot > SPLIT_FL) fovf = true;
      if (!fovf) {
        int pos = fc + inc - nh;
        uint32_t m = um;
        while (m) {
          const int j = __builtin_ctz(m);
          m &= m - 1;
          flist[pos++] = (uint32_t)(i0 + (j >> 2) * step + (j & 3));
        }
        fc += tot;
      }
    }
#pragma unroll
    for (int u = 0; u < LU4; ++u) {
      asm volatile("" ::: "memory");
      const int64_t i = i0 + u * step;
      const uint32_t w = lw[u];
      if ((um >> (4 * u)) & 0xFu) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (((w >> (8 * k)) & 0xFFu) != 0xFDu) lrow[i + k] = (int8_t)(w >> (8 * k));
      } else if (i < a1) {
        *reinterpret_cast<uint32_t*>(lrow + i) = w;
      }
      if (NB > 0 && nrow) {
        const double rs[4] = {ra[u].x, ra[u].y, rb[u].x, rb[u].y};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int lk = (int)(int8_t)(w >> (8 * k));
          const bool ok = lk >= 0 && rs[k] == rs[k];
          const int lb = ok ? lk : -1;
          const double r = ok ? rs[k] : 0.0;
          if (NB <= 10) pc += (uint64_t)(ok ? 1u : 0u) << (6 * (ok ? lb : 0));
#pragma unroll
          for (int d = 0; d < NB; ++d) {
            const bool h = lb == d;
            hs[d] = hs[d] + (h ? r : 0.0);   // (not fma(0, r, s): 0 * inf poisons)
            if (NB > 10) cn[d] += h ? 1 : 0;
          }
        }
      }
    }
    if (NB <= 10) {
#pragma unroll
      for (int d = 0; d < NB; ++d) cn[d] += (int)((pc >> (6 * d)) & 63u);
    }
    if (PF) {
#pragma unroll
      for (int u = 0; u < LU4; ++u) { pk[u] = pkn[u]; ra[u] = ran[u]; rb[u] = rbn[u]; }
    }
  }
  if (fovf && lane == 0) ovf = 1;
  __syncthreads();
  if (ovf) {   // block-uniform: the general kernel rewrites the whole row
    if (tid == 0) FLG[t] = 1;
    return;
  }
  if (NB > 0 && nrow) {
    // each lane's partial sums (the finish adds them per lane in chunk order); counts per chunk
    double* lp = sp.lp + ((int64_t)t * sp.C + c) * (MAXQ - 1) * SPLIT_THREADS + tid;
#pragma unroll
    for (int d = 0; d < NB; ++d) lp[d * SPLIT_THREADS] = hs[d];
#pragma unroll
    for (int d = 0; d < NB; ++d) {
      int cc = cn[d];
      for (int o = 32; o > 0; o >>= 1) cc += __shfl_down(cc, o, 64);
      if (lane == 0) swc[wid][d] = cc;
    }
    __syncthreads();
    if (tid < NB) {
      int cc = 0;
      for (int w = 0; w < SPLIT_WAVES; ++w) cc += swc[w][tid];
      sp.pc[((int64_t)t * sp.C + c) * MAXQ + tid] = cc;
    }
  }
  const int64_t li = ((int64_t)t * sp.C + c) * SPLIT_WAVES + wid;
  for (int j = lane; j < fc; j += 64) sp.ulist[li * SPLIT_FL + j] = flist[j];
  if (lane == 0) sp.ucnt[li] = fc;
}

// PRE (N % 4 == 0): the ids are INPUT -- written by csm_signal_ids with the fixed
// map csm_fbucket -- so M is not streamed at all: the histogram, gather and label passes read
// 2 B per cell, and M only for the cells of target / edge buckets and of the two extreme
// buckets (the exact min / max come out of the gather pass).
// MG (PRE only): the merged pass.  A row it cannot take (ties across edges, tiny rows,
// oversized target buckets, an uncertain-cell list overflow) is given up: dec_row returns
// false (and sets FLG[t] = 1 when FLG is given), and the same workgroup runs the general PRE
// path on it (k_deciles<.., MG, FB>), or -- FLG given -- the general kernel launched next with
// the same FLG takes the rows with FLG[t] = 1.
// SPLIT (PRE, wide rows of short date shards): 1 = the split pass's plan launch (with MG),
// 2 = its finish launch (without MG: rows the plan or a sweep chunk left, FLG = 1, run the
// general path).
// One date row; returns false when the merged pass gave the row up (block-uniform).
#ifndef DEC_MINB
#define DEC_MINB 4
#endif
#ifndef DEC_MINB_MG0
#define DEC_MINB_MG0 DEC_MINB   // the merged pass without decile sums (sweep ranking)
#endif
template <int NB, bool V2, bool PRE, bool MG, int SPLIT = 0>
__device__ __forceinline__ bool dec_row(DecShared& S, const double* __restrict__ Mx,
                                        const double* __restrict__ NRx, int64_t N, int n_bins,
                                        const QTab& qt, int8_t* __restrict__ L,
                                        double* __restrict__ EW, int32_t* __restrict__ CNT,
                                        int32_t* __restrict__ NV, int64_t* __restrict__ tim,
                                        uint16_t* __restrict__ IDSx, int32_t* __restrict__ FLG,
                                        const DecSplit& sp = DecSplit{}) {
  static_assert(!PRE || HB <= CSM_FB_BUCKETS, "PRE reads the fixed-map ids");
  static_assert(!MG || PRE, "the merged pass reads the fixed-map ids");
  static_assert(SPLIT == 0 || (PRE && (SPLIT == 1) == MG), "split: plan = MG, finish = general");
  const int t = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const double* row = Mx + (int64_t)t * N;
  const double* nrow = NRx ? NRx + (int64_t)t * N : nullptr;
  int8_t* lrow = L + (int64_t)t * N;
  if (PRE && !MG && FLG && FLG[t] == 0) {   // the merged pass / the split sweep took this row
    if constexpr (SPLIT == 2) {
      if (dsplit_finish<NB>(S, t, row, nrow, n_bins, qt, lrow, EW, CNT, sp)) return true;
      __syncthreads();   // (a wave list the merged pass would overflow: the general path below)
    } else {
      return true;
    }
  }

  dec_mark(tim, t, 0);
  // ---------------- pass 0: robust bucketing range from a coalesced sample.
  // The histogram below is monotone for ANY [lo, hi] (values outside clamp into the end
  // buckets), so lo/hi need not be the exact extremes: a 0.2 %..99.8 % range of a sample
  // keeps heavy momentum tails from squeezing the bulk into a few buckets.  The exact
  // count / min / max come out of the histogram pass itself.
  double blo = 0.0, bscale = 0.0;
  if (PRE) {
    for (int b2 = tid; b2 < HB; b2 += DEC_THREADS) S.hist[b2] = 0;
    __syncthreads();
  } else {
    // 32 chunks x 64 consecutive assets, PER samples per thread held in registers.  Each wave
    // trims 0.2 % off both ends of its own samples by extracting the distinct minima /
    // maxima in rounds (every copy of a value per round; wave shuffles and ballots only, no
    // block barrier); the range is the widest of the waves' trimmed ranges.
    constexpr int SCH = DEC_SCH, PER = SCH * 64 / DEC_THREADS;
    double xs[PER];
    int nloc = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int c = (tid >> 6) + k * (DEC_THREADS / 64);
      const int64_t start = (N <= SCH * 64) ? (int64_t)c * 64 : ((int64_t)c * (N - 64)) / (SCH - 1);
      const int64_t i = start + lane;
      xs[k] = (i < N) ? row[i] : qnan();
      nloc += (xs[k] == xs[k]) ? 1 : 0;
    }
    int nsw = nloc;
    for (int o = 32; o > 0; o >>= 1) nsw += __shfl_xor(nsw, o, 64);
    double lo_w = INFINITY, hi_w = -INFINITY;
    if (nsw >= 1) {   // wave-uniform
      const int idx = (nsw * 2) / 1000;
      double cur_lo = -INFINITY, cur_hi = INFINITY;
      int below = 0, above = 0;
      bool lo_done = false, hi_done = false;
      while (!(lo_done && hi_done)) {
        double mn = INFINITY, mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
          const double x = xs[k];
          if (x > cur_lo) mn = fmin(mn, x);
          if (x < cur_hi) mx = fmax(mx, x);
        }
        for (int o = 32; o > 0; o >>= 1) {
          mn = fmin(mn, __shfl_xor(mn, o, 64));
          mx = fmax(mx, __shfl_xor(mx, o, 64));
        }
        int g1 = 0, g2 = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
          g1 += __popcll(__ballot(xs[k] == mn));
          g2 += __popcll(__ballot(xs[k] == mx));
        }
        if (!lo_done) { if (below + g1 > idx) { lo_w = mn; lo_done = true; } else { below += g1; cur_lo = mn; } }
        if (!hi_done) { if (above + g2 > idx) { hi_w = mx; hi_done = true; } else { above += g2; cur_hi = mx; } }
      }
    }
    if (lane == 0) { S.red_d[wid][0] = lo_w; S.red_d[wid][1] = hi_w; }
    for (int b2 = tid; b2 < HB; b2 += DEC_THREADS) S.hist[b2] = 0;
    __syncthreads();
    double lo = INFINITY, hi = -INFINITY;
#pragma unroll
    for (int w = 0; w < DEC_THREADS / 64; ++w) { lo = fmin(lo, S.red_d[w][0]); hi = fmax(hi, S.red_d[w][1]); }
    const double rng = hi - lo;
    const bool ok = lo <= hi && rng > 0.0 && rng <= 1.0e300;
    blo = ok ? lo : 0.0;
    bscale = ok ? (double)HB / rng : 0.0;
  }
  // the bucket of a value: the sampled linear map, or the fixed map of the precomputed ids
  auto BK = [&](double x) -> int { return PRE ? pre_bucket(x) : vbucket(x, blo, bscale); };
  dec_mark(tim, t, 1);
  // ---------------- pass 1: value-bucket histogram + exact count / min / max
  int64_t n;
  double vmin, vmax;
  {
    int64_t cnt = 0;
    double lo = INFINITY, hi = -INFINITY;
    if (PRE) {
      // ids only: 8 B (four ids) per lane per load, HU loads in flight
      const uint16_t* irow = IDSx + (int64_t)t * N;
      const int64_t step = 4 * DEC_THREADS;
      constexpr int HU = 8;
      for (int64_t i0 = 4 * (int64_t)tid; i0 < N; i0 += HU * step) {
        uint2 pk[HU];
#pragma unroll
        for (int u = 0; u < HU; ++u) {
          const int64_t i = i0 + u * step;
          pk[u] = i < N ? *reinterpret_cast<const uint2*>(irow + i) : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        }
#pragma unroll
        for (int u = 0; u < HU; ++u) {
          const uint32_t id[4] = {dec_uid<PRE>(pk[u].x & 0xFFFFu), dec_uid<PRE>(pk[u].x >> 16),
                                  dec_uid<PRE>(pk[u].y & 0xFFFFu), dec_uid<PRE>(pk[u].y >> 16)};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const bool ok = id[k] != CSM_FB_NAN;
            cnt += ok ? 1 : 0;
            if (ok) atomicAdd(&S.hist[id[k] & (HB - 1)], 1u);
          }
        }
      }
    } else {
      for_row<V2>(row, N, [&](int64_t, double x) {
        const bool ok = x == x;
        cnt += ok ? 1 : 0;
        lo = fmin(lo, x);  // fmin / fmax ignore a NaN operand
        hi = fmax(hi, x);
        atomicAdd(&S.hist[vbucket(x, blo, bscale)], ok ? 1u : 0u);
      });
    }
    for (int o = 32; o > 0; o >>= 1) {
      cnt += __shfl_down(cnt, o, 64);
      lo = fmin(lo, __shfl_down(lo, o, 64));
      hi = fmax(hi, __shfl_down(hi, o, 64));
    }
    // (the sample range above was read from red_d before the barrier that precedes this
    // pass, so red_d can be rewritten here)
    if (lane == 0) { S.red_n[wid] = cnt; S.red_d2[wid][0] = lo; S.red_d2[wid][1] = hi; }
    __syncthreads();
    int64_t c = 0; double l = INFINITY, h = -INFINITY;
#pragma unroll
    for (int w = 0; w < DEC_THREADS / 64; ++w) { c += S.red_n[w]; l = fmin(l, S.red_d2[w][0]); h = fmax(h, S.red_d2[w][1]); }
    n = c; vmin = l; vmax = h;
  }
  dec_mark(tim, t, 2);
  if (NV && tid == 0) NV[t] = (int32_t)n;
  constexpr int NBA = NB > 0 ? NB : 1;
  double hs[NBA], ls[NBA];
  int cn[NBA];
#pragma unroll
  for (int d = 0; d < NBA; ++d) { hs[d] = 0.0; ls[d] = 0.0; cn[d] = 0; }
  auto accumulate = [&](int lab, double r) {
    if (NB > 0) {
      const bool ok = lab >= 0 && !isnan_d(r);
#pragma unroll
      for (int d = 0; d < NB; ++d) {
        const bool h = ok && lab == d;
        hs[d] += h ? r : 0.0;
        cn[d] += h ? 1 : 0;
      }
    }
  };
  // deterministic block reduction of (hs, ls, cn): wave shfl_down tree, then the waves in
  // order; thread d < NB gets label d's (high, low, count).  Two-sum, |error| ~ 1e-16 sum |r|.
  __shared__ double wh[DEC_THREADS / 64][NBA], wl[DEC_THREADS / 64][NBA];
  __shared__ int wc[DEC_THREADS / 64][NBA];
  auto block_sums = [&](double& oh, double& ol, int& oc) {
#pragma unroll
    for (int d = 0; d < NB; ++d) {
      double h = hs[d], l = ls[d];
      int c = cn[d];
      for (int o = 32; o > 0; o >>= 1) {
        const double h2 = __shfl_down(h, o, 64), l2 = __shfl_down(l, o, 64);
        const int c2 = __shfl_down(c, o, 64);
        const double s2 = h + h2;
        const double bb = s2 - h;
        const double err = (h - (s2 - bb)) + (h2 - bb);
        h = s2; l = (l + l2) + err; c += c2;
      }
      if (lane == 0) { wh[wid][d] = h; wl[wid][d] = l; wc[wid][d] = c; }
    }
    __syncthreads();
    if (tid < NB) {
      const int d = tid;
      double h = 0.0, l = 0.0;
      int c = 0;
      for (int w = 0; w < DEC_THREADS / 64; ++w) {
        const double h2 = wh[w][d];
        const double s2 = h + h2;
        const double bb = s2 - h;
        const double err = (h - (s2 - bb)) + (h2 - bb);
        h = s2; l = (l + wl[w][d]) + err; c += wc[w][d];
      }
      oh = h; ol = l; oc = c;
    }
    __syncthreads();
  };
  // PRE merged pass: per-wave list of the row's uncertain cells (those in the buckets of an
  // interior edge's order statistics), kept in the histogram's LDS from the sweep to the end
  constexpr int FL = HB / (DEC_THREADS / 64);   // 1024 indices per wave
  uint32_t* flist = reinterpret_cast<uint32_t*>(S.hist) + wid * FL;
  int fc = 0;            // wave-uniform list length
  constexpr bool fast = MG;
  const bool lg = MG && NB == 0 && qt.legs != 0 && n_bins >= 4;   // block-uniform
  auto give_up = [&]() {   // block-uniform: leave the row to the general path
    if (FLG && tid == 0) FLG[t] = 1;
  };
  // PRE: min / max are not known yet (the gather pass finds them); n == 0 is degenerate, an
  // all-equal row is detected after the gather
  const bool degenerate = PRE ? (n == 0) : ((n == 0) || !(vmin < vmax));
  if (MG && degenerate) {   // no ranked cell (n == 0): every label NaN, no decile means
    if constexpr (SPLIT == 1) {   // the sweep writes the labels (NaN ids), finish the NaN means
      if (tid == 0) {
        S.nslot = 0; S.ntgt = 0; S.total = 0;
      }
      __syncthreads();
      if (tid < MAXT) S.slots[tid].off = 0;
      dsplit_store(S, t, n, sp);
      if (tid == 0) FLG[t] = 0;
      return true;
    }
    for (int64_t i = 4 * (int64_t)tid; i < N; i += 4 * DEC_THREADS)
      *reinterpret_cast<uint32_t*>(lrow + i) = 0xFFFFFFFFu;
    if (NB > 0 && nrow && EW && tid < NB) {
      EW[(int64_t)t * NB + tid] = qnan();
      if (CNT) CNT[(int64_t)t * NB + tid] = 0;
    }
    if (FLG && tid == 0) FLG[t] = 0;
    return true;
  }

  if (!degenerate) {
    // ---------------- target ranks (interior order statistics; min / max are known) and
    // their slots, all by wave 0 in registers: lane 2k (2k+1) holds floor(v_k) (floor + 1),
    // a 64-lane bitonic sort orders them, ballots drop duplicates and number the slots.
    block_exclusive_scan_hist(S.hist);
    if (wid == 0) {
      int64_t cv = INT64_MAX;
      const int k = lane >> 1;
      if (k <= n_bins) {
        const double v = (double)(n - 1) * qt.q[k];
        if (v < (double)(n - 1)) {   // else the edge is the max
          const double p = floor(v);
          const int64_t pi = (int64_t)p;
          if ((lane & 1) == 0) { if (pi > 0) cv = pi; }
          else if (v - p != 0.0 && pi + 1 < n - 1) cv = pi + 1;
        }
      }
      // ONE binary search for every lane (last bucket b with prefix[b] <= rank): the targets,
      // and (PRE) lanes 62 / 63 -- which hold no target -- the extreme ranks 0 and n - 1; the
      // buckets then travel with their ranks through the sort (the merged pass reads each
      // edge's pre-sort pair too), instead of three searches one after another
      int64_t sr = cv;
      if (PRE && lane == 62) sr = 0;
      if (PRE && lane == 63) sr = n - 1;
      int bk = 0;
      if (sr != INT64_MAX) {
        int lo2 = 0, hi2 = HB - 1;
        while (lo2 < hi2) {
          const int mid = (lo2 + hi2 + 1) >> 1;
          if ((int64_t)S.hist[mid] <= sr) lo2 = mid; else hi2 = mid - 1;
        }
        bk = lo2;
      }
      if (PRE && lane >= 62) S.bext[lane - 62] = bk;
      if constexpr (MG) {   // edge k: buckets of ranks floor(v_k) (lane 2k) and floor + 1 (2k + 1)
        const int bo = __shfl_down(bk, 1, 64);
        if ((lane & 1) == 0 && k <= n_bins) { S.x.mg.plo[k] = bk; S.x.mg.phi[k] = bo; }
        // legs mode: every edge's buckets are checked below (same rows merged as the full
        // pass), but only edges 1 and n_bins - 1 get slots and an exact selection
        if (lg && k != 1 && k != n_bins - 1) cv = INT64_MAX;
      }
#pragma unroll
      for (int kk = 2; kk <= 64; kk <<= 1) {
#pragma unroll
        for (int j = kk >> 1; j > 0; j >>= 1) {
          const int64_t o = __shfl_xor(cv, j, 64);
          const int ob = __shfl_xor(bk, j, 64);
          const bool up = (lane & kk) == 0, lower = (lane & j) == 0;
          const bool take = (lower == up) ? (o < cv) : (o > cv);
          cv = take ? o : cv;
          bk = take ? ob : bk;
        }
      }
      const int64_t prev = __shfl_up(cv, 1, 64);
      const bool keep = cv != INT64_MAX && (lane == 0 || prev != cv);
      const uint64_t lt = (1ull << lane) - 1ull;
      const uint64_t mk = __ballot(keep);
      const int pos = __popcll(mk & lt);
      if (keep) {   // (bk: the bucket of rank cv, from the search above)
        S.trank[pos] = cv;
        S.tres[pos] = cv - (int64_t)S.hist[bk];
      }
      const uint64_t before = mk & lt;
      const int plane = before ? 63 - __clzll((long long)before) : lane;   // previous kept lane
      const int pbk = __shfl(bk, plane, 64);
      const bool nsl = keep && (before == 0 || pbk != bk);
      const uint64_t ms = __ballot(nsl);
      const int sidx = __popcll(ms & (lt | (1ull << lane))) - 1;
      int cnt = 0;
      if (nsl) {
        Slot& sl = S.slots[sidx];
        sl.b0 = bk; sl.klo = 0; sl.khi = ~0ULL; sl.resolved = 0; sl.value = 0.0;
        const uint32_t next = (bk + 1 < HB) ? S.hist[bk + 1] : (uint32_t)n;
        cnt = (int)(next - S.hist[bk]);
        sl.count = cnt;
      }
      if (keep) S.tslot[pos] = sidx;
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
      if (lane == 0) { S.ntgt = __popcll(mk); S.nslot = __popcll(ms); S.total = cnt; }
      if constexpr (MG) {
        // the merged pass never refines or resolves a slot, so the candidate offsets and the
        // selection's per-target prefix are known now (this wave's LDS writes above are in
        // order): the gather and selection below need no wave-0 step and barrier of their own
        const int nsl2 = __popcll(ms), ntg2 = __popcll(mk);
        const int c1 = lane < nsl2 ? (int)S.slots[lane].count : 0;
        int inc = c1;
        for (int o = 1; o < 64; o <<= 1) {
          const int v = __shfl_up(inc, o, 64);
          if (lane >= o) inc += v;
        }
        if (lane < nsl2) { S.slots[lane].off = inc - c1; S.fill[lane] = 0; }
        const int c2 = lane < ntg2 ? (int)S.slots[S.tslot[lane]].count : 0;
        int inc2 = c2;
        for (int o = 1; o < 64; o <<= 1) {
          const int v = __shfl_up(inc2, o, 64);
          if (lane >= o) inc2 += v;
        }
        if (lane < ntg2) S.tpre[lane + 1] = inc2;
        int64_t work = (int64_t)c2 * c2;
        for (int o = 32; o > 0; o >>= 1) work += __shfl_xor(work, o, 64);
        if (lane == 0) { S.tpre[0] = 0; S.sel_count = work <= (int64_t)DEC_THREADS * 512; }
      }
    }
    __syncthreads();

    dec_mark(tim, t, 3);
    // ---------------- PRE merged pass (the common case).  Edge k lies between the order
    // statistics of ranks floor(v_k) and floor(v_k) + 1, so between their buckets; a bucket
    // strictly between them is empty.  When the edges' bucket ranges (edge 0: the minimum's
    // bucket, edge n_bins: the maximum's) are pairwise disjoint, every cell outside them has a
    // label fixed by its bucket alone (the map is monotone), no two edges can be equal (no
    // duplicates to drop), and the cells inside them are exactly the candidates of the
    // selection.  So ONE sweep over ids + next_ret labels and sums the certain cells and lists
    // the uncertain ones; the selection runs on the listed cells, which are then labelled
    // exactly.  This replaces the gather sweep, the label table and a pass over the ids.
    // Otherwise (ties across edges, tiny rows, oversized target buckets, a list overflow) the
    // general path below runs from here.
    if constexpr (MG) {
      if (tid == 0) { S.fast = 0; S.ovf = 0; }
      if (wid == 0) {
        const int k = lane;
        bool ok = S.total <= CAP;
        int rl = 0, rh = 0;
        if (k <= n_bins) {
          if (k == 0) { rl = rh = S.bext[0]; }
          else if (k == n_bins) { rl = rh = S.bext[1]; }
          else {
            const double v = (double)(n - 1) * qt.q[k];
            if (!(v < (double)(n - 1))) {
              ok = false;
            } else {
              const double p = floor(v);
              const int64_t pi = (int64_t)p;
              const int64_t ph = (v - p != 0.0) ? pi + 1 : pi;
              // (ranks pi >= 1 and ph <= n - 2 are targets: the targets pass searched them)
              if (pi < 1 || ph > n - 2) ok = false;
              else { rl = S.x.mg.plo[k]; rh = ph != pi ? S.x.mg.phi[k] : rl; }
            }
          }
        }
        const int nl = __shfl_down(rl, 1, 64);
        if (k < n_bins && !(rh < nl)) ok = false;
        const uint64_t bad = __ballot(k <= n_bins && !ok);
        if (k <= n_bins) { S.x.mg.rlo[k] = rl; S.x.mg.rhi[k] = rh; }
        if (lane == 0) S.fast = bad == 0 ? 1 : 0;
      }
      __syncthreads();
      if (!S.fast) { give_up(); return false; }
      {
        // pre-selection bucket -> label table: the label of a bucket outside every range is
        // (ranges below it) - 1; the extreme ranges hold labels 0 / n_bins - 1; the buckets of
        // the interior ranges are marked -2 (empty between-buckets) or -3 - slot
        {
          // the ranges are sorted and disjoint: walk them beside the thread's PT buckets
          constexpr int PT = HB / DEC_THREADS;
          const int nr = n_bins + 1;
          const int b0 = tid * PT;
          int j = 0;   // ranges entirely below the current bucket
          while (j < nr && S.x.mg.rhi[j] < b0) ++j;
          uint32_t w = 0;
          for (int o = 0; o < PT; ++o) {
            const int b2 = b0 + o;
            while (j < nr && S.x.mg.rhi[j] < b2) ++j;
            int lab = j - 1;
            if (j < nr && S.x.mg.rlo[j] <= b2)   // (legs mode: an interior range is a middle label)
              lab = j == 0 ? 0 : (j == nr - 1 ? n_bins - 1 : ((lg && j != 1 && j != nr - 2) ? j - 1 : -2));
            w |= (uint32_t)(uint8_t)(int8_t)lab << (8 * (o & 3));
            if ((o & 3) == 3) { reinterpret_cast<uint32_t*>(S.blab + b0)[o >> 2] = w; w = 0; }
          }
        }
        __syncthreads();
        if (tid < S.nslot) S.blab[S.slots[tid].b0] = (int8_t)(-3 - tid);
        __syncthreads();
        if constexpr (SPLIT == 1) {   // plan: candidate offsets, then table + plan out
          if (wid == 0) {
            const int nsl = S.nslot;
            const int c = lane < nsl ? S.slots[lane].count : 0;
            int inc = c;
            for (int o = 1; o < 64; o <<= 1) {
              const int v = __shfl_up(inc, o, 64);
              if (lane >= o) inc += v;
            }
            if (lane < nsl) S.slots[lane].off = inc - c;
          }
          __syncthreads();
          dsplit_store(S, t, n, sp);
          if (tid == 0) FLG[t] = 0;
          return true;
        }
        dec_mark(tim, t, 4);
        // the merged sweep (the general path's label pass, with the uncertain cells kept)
        const uint16_t* irow = IDSx + (int64_t)t * N;
        const int64_t step = 4 * DEC_THREADS;
        constexpr int LU4 = DEC_MLU;
        bool fovf = false;   // wave-uniform
        // DEC_CHUNK_ORDER: the lane's sums restart at every chunk (whole trips) and its chunk
        // partials are added in chunk order, as the split pass's sweep lanes and finish do
        constexpr bool CHK = DEC_CHUNK_ORDER && NB > 0 && SPLIT == 0;
        static_assert(!CHK || 4 * LU4 * DEC_THREADS == SPLIT_TRIP, "chunks are whole trips");
        // the chunk partials' running sums: labels d < QL in the candidate buffer (free until
        // the gather after the sweep; one slot per lane), the rest in registers
        constexpr int QL = CHK ? (NB < CAP / DEC_THREADS ? NB : CAP / DEC_THREADS) : 0;
        constexpr int QR = CHK ? NBA - QL : 0;
        double* qs = S.cand + tid;
        double q[QR > 0 ? QR : 1];
#pragma unroll
        for (int d = 0; d < QR; ++d) q[d] = 0.0;
#pragma unroll
        for (int d = 0; d < QL; ++d) qs[d * DEC_THREADS] = 0.0;
        int64_t cend = CHK ? sp.cells : 0;   // (block-uniform) end of the current chunk
        for (int64_t base = 0; base < N; base += LU4 * step) {
          const int64_t i0 = base + 4 * (int64_t)tid;
          uint2 pk[LU4];
          double2 ra[LU4], rb[LU4];
#pragma unroll
          for (int u = 0; u < LU4; ++u) {
            const int64_t i = i0 + u * step;
            pk[u] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
            ra[u] = make_double2(0.0, 0.0);
            rb[u] = make_double2(0.0, 0.0);
            if (i < N) {
              pk[u] = *reinterpret_cast<const uint2*>(irow + i);
              if (NB > 0 && nrow) {
                ra[u] = *reinterpret_cast<const double2*>(nrow + i);
                rb[u] = *reinterpret_cast<const double2*>(nrow + i + 2);
              }
            }
          }
          // labels of the batch (packed 4 per word, -3 = uncertain) and its uncertain-cell mask
          static_assert(4 * LU4 < 64, "6-bit packed label counts per batch");
          uint64_t pc = 0;   // NB <= 10: the batch's per-label counts, 6-bit fields
          uint32_t lw[LU4];
          uint32_t um = 0;
#pragma unroll
          for (int u = 0; u < LU4; ++u) {
            asm volatile("" ::: "memory");   // bound the table lookups in flight (register pressure)
            const uint32_t id[4] = {dec_uid<PRE>(pk[u].x & 0xFFFFu), dec_uid<PRE>(pk[u].x >> 16),
                                  dec_uid<PRE>(pk[u].y & 0xFFFFu), dec_uid<PRE>(pk[u].y >> 16)};
            uint32_t w = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              int l = id[k] == 0xFFFFu ? -1 : (int)S.blab[id[k]];
              const bool un = l <= -2;
              um |= (un ? 1u : 0u) << (4 * u + k);
              l = un ? -3 : l;
              w |= (uint32_t)(uint8_t)(int8_t)l << (8 * k);
            }
            lw[u] = w;
          }
          // one wave prefix scan places every lane's uncertain cells in the wave's list
          const int nh = __popc(um);
          int inc = nh;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(inc, o, 64);
            if (lane >= o) inc += v;
          }
          const int tot = __shfl(inc, 63, 64);
          if (tot) {   // wave-uniform
            if (fc + tot > FL) fovf = true;
            if (!fovf) {
              int pos = fc + inc - nh;
              uint32_t m = um;
              while (m) {
                const int j = __builtin_ctz(m);
                m &= m - 1;
                flist[pos++] = (uint32_t)(i0 + (j >> 2) * step + (j & 3));
              }
              fc += tot;
            }
          }
#pragma unroll
          for (int u = 0; u < LU4; ++u) {
            asm volatile("" ::: "memory");
            const int64_t i = i0 + u * step;
            const uint32_t w = lw[u];
            if ((um >> (4 * u)) & 0xFu) {
#pragma unroll
              for (int k = 0; k < 4; ++k)
                if (((w >> (8 * k)) & 0xFFu) != 0xFDu) lrow[i + k] = (int8_t)(w >> (8 * k));
            } else if (i < N) {
              *reinterpret_cast<uint32_t*>(lrow + i) = w;
            }
            if (NB > 0 && nrow) {
              const double rs[4] = {ra[u].x, ra[u].y, rb[u].x, rb[u].y};
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                const int lk = (int)(int8_t)(w >> (8 * k));
                const bool ok = lk >= 0 && rs[k] == rs[k];
                const int lb = ok ? lk : -1;
                const double r = ok ? rs[k] : 0.0;
                if (NB <= 10) pc += (uint64_t)(ok ? 1u : 0u) << (6 * (ok ? lb : 0));   // shift + add
#pragma unroll
                for (int d = 0; d < NB; ++d) {
                  const bool h = lb == d;
                  hs[d] = hs[d] + (h ? r : 0.0);   // (not fma(0, r, s): 0 * inf poisons)
                  if (NB > 10) cn[d] += h ? 1 : 0;
                }
              }
            }
          }
          if (NB <= 10) {   // the batch's counts (<= 4 * LU4 < 64 per field) into the counters
#pragma unroll
            for (int d = 0; d < NB; ++d) cn[d] += (int)((pc >> (6 * d)) & 63u);
          }
          if constexpr (CHK) {
            if (base + LU4 * step >= cend || base + LU4 * step >= N) {   // the chunk's last trip
#pragma unroll
              for (int d = 0; d < NB; ++d) {
                if (d < QL) qs[d * DEC_THREADS] += hs[d];
                else q[d - QL] += hs[d];
                hs[d] = 0.0;
              }
              cend += sp.cells;
            }
          }
        }
        if constexpr (CHK) {
#pragma unroll
          for (int d = 0; d < NB; ++d) hs[d] = d < QL ? qs[d * DEC_THREADS] : q[d - QL];
        }
        if (fovf && lane == 0) S.ovf = 1;
        __syncthreads();
        dec_mark(tim, t, 5);
        if (S.ovf) { give_up(); return false; }   // the general path rewrites every label
        if (NB > 0 && nrow && EW) {
          // the certain cells' totals now (the accumulators are free during the selection);
          // the listed cells' sums are reduced at the end and added to these
          double h, l;
          int c;
          block_sums(h, l, c);
          if (tid < NB) { S.x.mg.fh[tid] = h; S.x.mg.fl[tid] = l; S.x.mg.fcn[tid] = c; }
#pragma unroll
          for (int d = 0; d < NBA; ++d) { hs[d] = 0.0; ls[d] = 0.0; cn[d] = 0; }
        }
      }
    }
    // ---------------- (rare) key-space refinement of the largest slot until all fit.
    // Each refinement shrinks a slot's key range >= HB x (<= 7 per target before it is a
    // single key), so the bound below is never reached on consistent state.
    for (int guard = 0; !MG && S.total > CAP && guard < 8 * MAXT; ++guard) {
      __shared__ int rs;
      if (tid == 0) {
        int best = -1;
        for (int i = 0; i < S.nslot; ++i)
          if (!S.slots[i].resolved && (best < 0 || S.slots[i].count > S.slots[best].count)) best = i;
        rs = best;
      }
      __syncthreads();
      const Slot sl = S.slots[rs];
      // key min / max of the members
      unsigned long long kl = ~0ULL, kh = 0ULL;
      for_row<V2>(row, N, [&](int64_t, double x) {
        if (!isnan_d(x)) {
          const uint64_t k = dkey(x);
          if (slot_member(sl, BK(x), k)) { kl = k < kl ? k : kl; kh = k > kh ? k : kh; }
        }
      });
      for (int o = 32; o > 0; o >>= 1) {
        unsigned long long a2 = __shfl_down(kl, o, 64), b2 = __shfl_down(kh, o, 64);
        kl = a2 < kl ? a2 : kl; kh = b2 > kh ? b2 : kh;
      }
      if (lane == 0) { S.red_k[wid][0] = kl; S.red_k[wid][1] = kh; }
      for (int b = tid; b < HB; b += DEC_THREADS) S.hist[b] = 0;
      __syncthreads();
      if (tid == 0) {
        unsigned long long l2 = ~0ULL, h2 = 0ULL;
        for (int w = 0; w < DEC_THREADS / 64; ++w) { l2 = S.red_k[w][0] < l2 ? S.red_k[w][0] : l2; h2 = S.red_k[w][1] > h2 ? S.red_k[w][1] : h2; }
        S.kmin_r = l2; S.kmax_r = h2;
      }
      __syncthreads();
      const uint64_t kmin = S.kmin_r, kmax = S.kmax_r;
      if (kmin == kmax) {
        if (tid == 0) {
          Slot& s = S.slots[rs];
          s.resolved = 1; s.value = dval(kmin); s.klo = kmin; s.khi = kmax;
          S.total -= s.count;
        }
        __syncthreads();
        continue;
      }
      const uint64_t range = kmax - kmin;
      const int bits = 64 - __clzll((long long)range);
      const int shift = bits > kHbBits ? bits - kHbBits : 0;
      for_row<V2>(row, N, [&](int64_t, double x) {
        if (!isnan_d(x)) {
          const uint64_t k = dkey(x);
          if (slot_member(sl, BK(x), k)) atomicAdd(&S.hist[(k - kmin) >> shift], 1u);
        }
      });
      __syncthreads();
      // hist[b] -> members in sub-buckets < b, so each target's sub-bucket is a binary search
      // (a serial walk over HB buckets by one thread dominated heavy-tailed rows)
      const uint32_t hlast = S.hist[HB - 1];   // read before the scan's first barrier
      block_exclusive_scan_hist(S.hist);
      if (tid == 0) {
        // split slot rs by the sub-buckets of its targets; rebuild the slot list in order
        Slot old = S.slots[rs];
        Slot* ns_list = S.x.rf.slots2;
        int nn = 0;
        int* remap = S.x.rf.remap;
        for (int i = 0; i < S.nslot; ++i) remap[i] = -1;
        for (int i = 0; i < S.nslot; ++i) {
          if (i != rs) { ns_list[nn] = S.slots[i]; remap[i] = nn++; continue; }
          // targets of this slot (contiguous in target order)
          for (int ti = 0; ti < S.ntgt; ++ti) {
            if (S.tslot[ti] != rs) continue;
            int64_t r = S.tres[ti];
            int j = 0, hi2 = HB - 1;   // last sub-bucket with prefix <= r
            while (j < hi2) {
              const int mid = (j + hi2 + 1) >> 1;
              if ((int64_t)S.hist[mid] <= r) j = mid; else hi2 = mid - 1;
            }
            const int64_t acc = S.hist[j];
            const int cntj = (int)((j + 1 < HB ? (int64_t)S.hist[j + 1]
                                               : (int64_t)S.hist[HB - 1] + hlast) - acc);
            const uint64_t klo = kmin + ((uint64_t)j << shift);
            uint64_t khi = klo + (((uint64_t)1 << shift) - 1);
            if (khi > kmax || khi < klo) khi = kmax;
            if (nn == 0 || ns_list[nn - 1].b0 != old.b0 || ns_list[nn - 1].klo != klo) {
              Slot& s = ns_list[nn++];
              s = old; s.klo = klo; s.khi = khi; s.count = cntj; s.resolved = 0;
            }
            S.tres[ti] = r - acc;
            S.tslot[ti] = -(nn - 1) - 2;  // mark as remapped (new index encoded)
          }
        }
        for (int ti = 0; ti < S.ntgt; ++ti) {
          if (S.tslot[ti] <= -2) S.tslot[ti] = -S.tslot[ti] - 2;
          else S.tslot[ti] = remap[S.tslot[ti]];
        }
        int tot = 0;
        for (int i = 0; i < nn; ++i) { S.slots[i] = ns_list[i]; if (!ns_list[i].resolved) tot += ns_list[i].count; }
        S.nslot = nn;
        S.total = tot;
      }
      __syncthreads();
    }

    if (!MG) dec_mark(tim, t, 4);
    // ---------------- pass 3: gather candidates of unresolved slots
    if constexpr (!MG) {   // (the merged pass set the offsets in the targets step)
    if (wid == 0) {   // candidate offsets: exclusive scan of unresolved counts over slots
      const int nsl = S.nslot;
      const int c = (lane < nsl && !S.slots[lane].resolved) ? S.slots[lane].count : 0;
      int inc = c;
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
      }
      if (lane < nsl) { S.slots[lane].off = inc - c; S.fill[lane] = 0; }
      if (lane == 63) S.total = inc;
    }
    // bucket -> first slot index map (reuses hist; the merged pass keeps its lists there and
    // has the slot of each uncertain bucket in its label table)
    if (!fast) for (int b = tid; b < HB; b += DEC_THREADS) S.hist[b] = 0xFFFFFFFFu;
    __syncthreads();
    if (!fast && tid < S.nslot && (tid == 0 || S.slots[tid - 1].b0 != S.slots[tid].b0))
      S.hist[S.slots[tid].b0] = (uint32_t)tid;   // slots are ordered by bucket
    __syncthreads();
    }
    double pmn = INFINITY, pmx = -INFINITY;   // PRE: exact min / max of the extreme buckets
    if (fast) {
      // the listed cells' values into their slots (M read for a whole list at once)
      __builtin_amdgcn_wave_barrier();
      for (int j0 = 0; j0 < fc; j0 += 128) {
        const int j1 = j0 + lane, j2 = j1 + 64;
        const double x1 = j1 < fc ? row[flist[j1]] : 0.0;
        const double x2 = j2 < fc ? row[flist[j2]] : 0.0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if ((h ? j2 : j1) >= fc) continue;
          const double x = h ? x2 : x1;
          const int sl = -3 - (int)S.blab[pre_bucket(x)];
          if (sl >= 0) {
            const int pos = atomicAdd(&S.fill[sl], 1);
            S.cand[S.slots[sl].off + pos] = x;
          }
        }
      }
    } else {
      const double lo = blo, sc = bscale;
      const int nsl = S.nslot;
      auto offer = [&](double x, int b) {
        const uint64_t k = dkey(x);
        for (int i = (int)S.hist[b]; i < nsl && S.slots[i].b0 == b; ++i) {
          const Slot& s = S.slots[i];
          if (k >= s.klo && k <= s.khi) {
            if (!s.resolved) {
              const int pos = atomicAdd(&S.fill[i], 1);
              S.cand[s.off + pos] = x;
            }
            break;
          }
        }
      };
      if (PRE) {
        // ids only.  The cells of target / extreme buckets (~1 % of the row, spread over all
        // lanes) are appended to a per-wave index list in LDS (the label table's bytes, unused
        // until after this pass) and M is read for a whole list at once, 2 loads per lane in
        // flight: one memory latency per 256 hits instead of one per batch with a hit.
        const uint16_t* irow = IDSx + (int64_t)t * N;
        const int64_t step = 4 * DEC_THREADS;
        constexpr int GU = 8, GL = HB / 4 / (DEC_THREADS / 64);   // 256 indices per wave
        uint32_t* glist = reinterpret_cast<uint32_t*>(S.blab) + wid * GL;
        const int be0 = S.bext[0], be1 = S.bext[1];
        int gc = 0;   // wave-uniform list length
        auto take = [&](double x) {
          const int b = pre_bucket(x);
          if (b == be0 || b == be1) { pmn = fmin(pmn, x); pmx = fmax(pmx, x); }
          if (S.hist[b] != 0xFFFFFFFFu) offer(x, b);
        };
        auto gflush = [&]() {   // wave-uniform
          __builtin_amdgcn_wave_barrier();
          for (int j0 = 0; j0 < gc; j0 += 128) {
            const int j1 = j0 + lane, j2 = j1 + 64;
            const double x1 = j1 < gc ? row[glist[j1]] : qnan();
            const double x2 = j2 < gc ? row[glist[j2]] : qnan();
            if (j1 < gc) take(x1);
            if (j2 < gc) take(x2);
          }
          __builtin_amdgcn_wave_barrier();
          gc = 0;
        };
        // the trip count is block-uniform (no lane leaves the loop early): the ballots and the
        // list length must stay wave-uniform
        for (int64_t base = 0; base < N; base += GU * step) {
          const int64_t i0 = base + 4 * (int64_t)tid;
          uint2 pk[GU];
#pragma unroll
          for (int u = 0; u < GU; ++u) {
            const int64_t i = i0 + u * step;
            pk[u] = i < N ? *reinterpret_cast<const uint2*>(irow + i) : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
          }
          // the batch's hit flags first (LDS reads only, all in flight), then one wave prefix
          // scan places every lane's hits in the list
          uint32_t hits = 0;
#pragma unroll
          for (int u = 0; u < GU; ++u) {
            const uint32_t id[4] = {dec_uid<PRE>(pk[u].x & 0xFFFFu), dec_uid<PRE>(pk[u].x >> 16),
                                  dec_uid<PRE>(pk[u].y & 0xFFFFu), dec_uid<PRE>(pk[u].y >> 16)};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const bool hit = id[k] != 0xFFFFu &&
                               (S.hist[id[k]] != 0xFFFFFFFFu || (int)id[k] == be0 || (int)id[k] == be1);
              hits |= (hit ? 1u : 0u) << (4 * u + k);
            }
          }
          const int nh = __popc(hits);
          int inc = nh;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(inc, o, 64);
            if (lane >= o) inc += v;
          }
          const int tot = __shfl(inc, 63, 64);
          if (tot == 0) continue;   // wave-uniform
          if (gc + tot > GL) gflush();
          if (tot <= GL) {
            int pos = gc + inc - nh;
#pragma unroll
            for (int j = 0; j < 4 * GU; ++j)
              if ((hits >> j) & 1u) glist[pos++] = (uint32_t)(i0 + (j >> 2) * step + (j & 3));
            gc += tot;
          } else {   // more hits in one batch than the list holds (pathological rows)
#pragma unroll
            for (int j = 0; j < 4 * GU; ++j) {
              if (gc > GL - 64) gflush();
              const bool hit = (hits >> j) & 1u;
              const uint64_t mk = __ballot(hit);
              if (hit) glist[gc + lane_prefix(mk)] = (uint32_t)(i0 + (j >> 2) * step + (j & 3));
              gc += __popcll(mk);
            }
          }
        }
        gflush();
      } else {
        for_row<V2, true>(row, N, [&](int64_t, double x) {
          const uint32_t si = S.hist[vbucket(x, lo, sc)];
          if (si == 0xFFFFFFFFu || !(x == x)) return;  // common case: not a target bucket
          offer(x, vbucket(x, lo, sc));
        });
      }
    }
    __syncthreads();
    // placeholders (finite, so edge 0's lerp stays -DBL_MAX): every listed cell lies strictly
    // between the extreme buckets, so it is above the first edge and below the last
    if (PRE && fast) { vmin = -__DBL_MAX__; vmax = __DBL_MAX__; }
    else if (PRE) block_minmax(pmn, pmx, vmin, vmax, S.red_d);
    dec_mark(tim, t, MG ? 6 : 5);   // MG: 4 pre-table, 5 merged sweep (below)
    if (vmin < vmax) {   // block-uniform; PRE: an all-equal row is degenerate (labels NaN)
    // ---------------- order statistics inside the slots.  Small slots (the usual case: a
    // few dozen members each) use counting selection: the member whose rank inside its slot
    // (ties broken by position) equals the target's residual rank is the order statistic --
    // one pass, no barriers.  Large slots fall back to a bitonic sort of all candidates.
    if constexpr (!MG) {   // (the merged pass set these in the targets step)
    if (wid == 0) {   // per-target prefix of unresolved member counts, selection work
      const int ntg = S.ntgt;
      int c = 0;
      if (lane < ntg) {
        const Slot& sl = S.slots[S.tslot[lane]];
        c = sl.resolved ? 0 : sl.count;
      }
      int inc = c;
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
      }
      if (lane < ntg) S.tpre[lane + 1] = inc;
      int64_t work = (int64_t)c * c;
      for (int o = 32; o > 0; o >>= 1) work += __shfl_xor(work, o, 64);
      if (lane == 0) { S.tpre[0] = 0; S.sel_count = work <= (int64_t)DEC_THREADS * 512; }
    }
    __syncthreads();
    }
    if (S.sel_count) {
      const int ntg = S.ntgt, tot = S.tpre[ntg];
      for (int p = tid; p < tot; p += DEC_THREADS) {
        int t2 = 0, hi3 = ntg - 1;   // the target t2 with tpre[t2] <= p < tpre[t2 + 1]
        while (t2 < hi3) {
          const int mid = (t2 + hi3 + 1) >> 1;
          if (S.tpre[mid] <= p) t2 = mid; else hi3 = mid - 1;
        }
        const Slot& sl = S.slots[S.tslot[t2]];
        const int i = p - S.tpre[t2];
        const double* c = S.cand + sl.off;
        const double x = c[i];
        int rank = 0;
        for (int j = 0; j < sl.count; ++j) {
          const double y = c[j];
          rank += (y < x || (y == x && j < i)) ? 1 : 0;
        }
        if (rank == S.tres[t2]) S.tval[t2] = x;
      }
      if (tid < ntg) {
        const Slot& sl = S.slots[S.tslot[tid]];
        if (sl.resolved) S.tval[tid] = sl.value;
      }
    } else {
      const int tot = S.total;
      int P2 = 1;
      while (P2 < tot) P2 <<= 1;
      for (int i = tot + tid; i < P2; i += DEC_THREADS) S.cand[i] = INFINITY;
      __syncthreads();
      for (int k = 2; k <= P2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int i = tid; i < P2; i += DEC_THREADS) {
            const int ixj = i ^ j;
            if (ixj > i) {
              const double x = S.cand[i], y = S.cand[ixj];
              const bool up = (i & k) == 0;
              if ((x > y) == up) { S.cand[i] = y; S.cand[ixj] = x; }
            }
          }
          __syncthreads();
        }
      }
      if (tid < S.ntgt) {
        const Slot& sl = S.slots[S.tslot[tid]];
        S.tval[tid] = sl.resolved ? sl.value : S.cand[sl.off + S.tres[tid]];
      }
    }
    __syncthreads();
    if (!MG) dec_mark(tim, t, 6);
    // ---------------- edges (NumPy _lerp) and duplicates='drop', by wave 0: lane k computes
    // edge k (its order statistics by binary search over the sorted target ranks), keeps it
    // unless an earlier edge has the same value, and the kept edges are compacted by ballot.
    if (wid == 0) {
      auto order_stat = [&](int64_t r) -> double {
        if (r <= 0) return vmin;
        if (r >= n - 1) return vmax;
        int lo2 = 0, hi2 = S.ntgt - 1;
        while (lo2 < hi2) { const int mid = (lo2 + hi2) >> 1; if (S.trank[mid] < r) lo2 = mid + 1; else hi2 = mid; }
        return S.tval[lo2];
      };
      const int k = lane;
      const bool valid = k <= n_bins;
      double ek = 0.0;
      if (valid) {
        const double v = (double)(n - 1) * qt.q[k];
        if (v >= (double)(n - 1)) {
          ek = vmax;
        } else {
          const double p = floor(v);
          const double g = v - p;
          const int64_t pi = (int64_t)p;
          const double a = order_stat(pi);
          const double b = (g != 0.0) ? order_stat(pi + 1) : a;
          const double d = b - a;
          ek = (g >= 0.5) ? (b - d * (1.0 - g)) : (a + d * g);
        }
      }
      // legs mode: the interior edges (no order statistics selected) stand at edge 1's value,
      // so a listed cell of edge 1's range gets 0 or n_bins - 2 and one of edge n_bins - 1's
      // range n_bins - 2 or n_bins - 1 (the edges are distinct: no duplicates to drop)
      const double e1 = __shfl(ek, 1, 64);
      if (lg && k >= 2 && k <= n_bins - 2) ek = e1;
      bool seen = false;
      for (int j = 0; j < n_bins; ++j) {
        const double ej = __shfl(ek, j, 64);
        seen |= (j < k) && (ej == ek);
      }
      const bool keep = valid && !seen;
      const uint64_t mk = __ballot(keep);
      const int nu = __popcll(mk), ne = n_bins + 1;
      const bool drop = !lg && nu < ne && ne != 2;
      const int pos = drop ? lane_prefix(mk) : k;
      if (drop ? keep : valid) {
        S.bins[pos] = ek;
        S.vbe[pos] = BK(ek);
      }
      if (lane == 0) S.nbins = drop ? nu : ne;
    }
    __syncthreads();
    if (!fast)
    // bucket -> label table: a bucket holding no edge has one label for all its values
    // (the map is monotone: b(e) < b(x) implies e < x, b(e) > b(x) implies e > x).  So has a
    // bucket whose only edge is the first one (bins[0] = the row minimum: every x there has
    // ids 1) or the last one (the maximum: ids nbe - 1); only buckets holding an interior
    // edge, or two edges, compare values against the edges exactly.
    {
      // the edges' buckets in registers (LDS broadcast reads, once), then ALU-only compares
      // each thread owns PT consecutive buckets; most hold no edge (<= 21 edges in HB
      // buckets) and take one label, written 4 buckets per store
      const int nbe = S.nbins;
      constexpr int PT = HB / DEC_THREADS;
      static_assert(PT % 4 == 0, "4-bucket stores");
      int vbr[MAXQ];
#pragma unroll
      for (int j = 0; j < MAXQ; ++j) vbr[j] = j < nbe ? S.vbe[j] : 0x7FFFFFFF;
      const int b0 = tid * PT;
      int c0 = 0, c1 = 0;
#pragma unroll
      for (int j = 0; j < MAXQ; ++j) { c0 += vbr[j] < b0 ? 1 : 0; c1 += vbr[j] < b0 + PT ? 1 : 0; }
      if (c0 == c1) {
        const uint32_t lab = (uint32_t)(uint8_t)(int8_t)((c0 == 0 || c0 == nbe) ? -1 : c0 - 1);
#pragma unroll
        for (int w = 0; w < PT / 4; ++w)
          reinterpret_cast<uint32_t*>(S.blab + b0)[w] = lab * 0x01010101u;
      } else {
        for (int b2 = b0; b2 < b0 + PT; ++b2) {
          int c = 0, in = 0;
          bool inner = false, first = false;
#pragma unroll
          for (int j = 0; j < MAXQ; ++j) {
            c += vbr[j] < b2 ? 1 : 0;
            const bool eq = vbr[j] == b2;
            in += eq ? 1 : 0;
            inner |= eq && j > 0 && j < nbe - 1;
            first |= eq && j == 0;
          }
          const int ids = c + (first ? 1 : 0);
          S.blab[b2] = (int8_t)((inner || in > 1) ? -2 : ((ids == 0 || ids == nbe) ? -1 : ids - 1));
        }
      }
    }
    if (!fast) __syncthreads();   // (block-uniform; the merged pass built no table here)
    } else {   // all-equal row (PRE): every label NaN
      if (tid == 0) S.nbins = 0;
      __syncthreads();
    }
  } else {
    if (tid == 0) S.nbins = 0;
    __syncthreads();
  }

  dec_mark(tim, t, 7);
  // ---------------- pass 4: labels + equal-weight accumulation
  // Labels come from the bucket table; only values in a bucket that holds an edge are
  // compared against the edges.  Per lane the next_ret sums are plain fp64 (a few dozen
  // terms per label), then combined across lanes and waves with a fixed-order
  // double-double tree (deterministic; |error| ~ 1e-16 * sum |r|).
  const int nb = S.nbins;
  const double* bins = S.bins;  // LDS, every lane reads the same word: broadcast
  auto label_of = [&](double x) -> int {
    int lab = (nb == 0) ? -1 : (int)S.blab[BK(x)];
    lab = (x == x) ? lab : -1;
    if (lab != -2) return lab;
    int ids = 0;
    for (int j = 0; j < nb; ++j) ids += (bins[j] < x) ? 1 : 0;
    if (x == bins[0]) ids = 1;
    return (ids == 0 || ids == nb) ? -1 : ids - 1;
  };
  if (fast) {
    // merged pass, last step: the uncertain cells get their labels from the exact edges (the
    // first / last edge are -DBL_MAX / DBL_MAX placeholders: every listed cell lies inside)
    // and their next_ret is added after the certain cells', in list order (deterministic)
    __builtin_amdgcn_wave_barrier();
    for (int j0 = 0; j0 < fc; j0 += 128) {
      const int j1 = j0 + lane, j2 = j1 + 64;
      const int c1 = j1 < fc ? (int)flist[j1] : 0, c2 = j2 < fc ? (int)flist[j2] : 0;
      const double x1 = row[c1], x2 = row[c2];
      const double r1 = (NB > 0 && nrow) ? nrow[c1] : 0.0, r2 = (NB > 0 && nrow) ? nrow[c2] : 0.0;
      auto exact = [&](double x) {
        int ids = 0;
        for (int j = 0; j < nb; ++j) ids += (bins[j] < x) ? 1 : 0;
        return (ids == 0 || ids == nb) ? -1 : ids - 1;
      };
      if (j1 < fc) { const int l = exact(x1); lrow[c1] = (int8_t)l; accumulate(l, r1); }
      if (j2 < fc) { const int l = exact(x2); lrow[c2] = (int8_t)l; accumulate(l, r2); }
    }
  } else if (PRE) {
    // label from the bucket id; exact comparison (re-reading M) only in edge buckets.  The
    // decile sums use a one-hot select per label (s + r for the hit, s + 0 otherwise: an inf
    // next_ret stays in its own decile's sum, as in pandas' mean) and integer counts.
    const uint16_t* irow = IDSx + (int64_t)t * N;
    const int64_t step = 4 * DEC_THREADS;
    constexpr int LU4 = 4;
    // PRE: cells of edge buckets (label -2) are deferred -- appended to a per-wave index list
    // in LDS (the candidate buffer, free after the selection), their label byte written and
    // next_ret added after one batched read of their M / NR -- so the sweep never waits on a
    // dependent load.  List order, and so each lane's share, is fixed: deterministic sums.
    constexpr int DL = PRE ? CAP * 2 / (DEC_THREADS / 64) : 1;   // 1024 indices per wave
    uint32_t* dlist = reinterpret_cast<uint32_t*>(S.cand) + wid * DL;
    int dc = 0;   // wave-uniform list length
    auto dflush = [&]() {   // wave-uniform
      __builtin_amdgcn_wave_barrier();
      for (int j0 = 0; j0 < dc; j0 += 128) {
        const int j1 = j0 + lane, j2 = j1 + 64;
        const int c1 = j1 < dc ? (int)dlist[j1] : 0, c2 = j2 < dc ? (int)dlist[j2] : 0;
        const double x1 = row[c1], x2 = row[c2];
        const double r1 = (NB > 0 && nrow) ? nrow[c1] : 0.0, r2 = (NB > 0 && nrow) ? nrow[c2] : 0.0;
        if (j1 < dc) { const int l = label_of(x1); lrow[c1] = (int8_t)l; accumulate(l, r1); }
        if (j2 < dc) { const int l = label_of(x2); lrow[c2] = (int8_t)l; accumulate(l, r2); }
      }
      __builtin_amdgcn_wave_barrier();
      dc = 0;
    };
    // block-uniform trip count, cells past N predicated off (ids NaN, no store): no lane leaves
    // the loop early, so the PRE list length stays wave-uniform
    for (int64_t base = 0; base < N; base += LU4 * step) {
      const int64_t i0 = base + 4 * (int64_t)tid;
      uint2 pk[LU4];
      double2 ra[LU4], rb[LU4];
#pragma unroll
      for (int u = 0; u < LU4; ++u) {
        const int64_t i = i0 + u * step;
        pk[u] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        ra[u] = make_double2(0.0, 0.0);
        rb[u] = make_double2(0.0, 0.0);
        if (i < N) {
          pk[u] = *reinterpret_cast<const uint2*>(irow + i);
          if (NB > 0 && nrow) {
            ra[u] = *reinterpret_cast<const double2*>(nrow + i);
            rb[u] = *reinterpret_cast<const double2*>(nrow + i + 2);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < LU4; ++u) {
        const int64_t i = i0 + u * step;
        const bool in = i < N;
        const uint32_t id[4] = {dec_uid<PRE>(pk[u].x & 0xFFFFu), dec_uid<PRE>(pk[u].x >> 16),
                                  dec_uid<PRE>(pk[u].y & 0xFFFFu), dec_uid<PRE>(pk[u].y >> 16)};
        if (PRE && dc > DL - 4 * 64) dflush();   // room for this group (wave-uniform test)
        int lab[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          int l = (id[k] == 0xFFFFu || nb == 0) ? -1 : (int)S.blab[id[k]];
          if (PRE) {
            const bool df = l == -2;
            const uint64_t mk = __ballot(df);
            if (df) dlist[dc + lane_prefix(mk)] = (uint32_t)(i + k);
            dc += __popcll(mk);
            if (df) l = -3;   // excluded from the sums here; its byte is written by dflush only
          }
          lab[k] = l;
        }
        if (PRE && (lab[0] == -3 || lab[1] == -3 || lab[2] == -3 || lab[3] == -3)) {
#pragma unroll
          for (int k = 0; k < 4; ++k)   // bytes of the other cells (dflush owns the deferred ones)
            if (lab[k] != -3) lrow[i + k] = (int8_t)lab[k];
        } else if (in) {
          char4 lv;
          lv.x = (char)lab[0]; lv.y = (char)lab[1]; lv.z = (char)lab[2]; lv.w = (char)lab[3];
          *reinterpret_cast<char4*>(lrow + i) = lv;
        }
        if (NB > 0 && nrow) {
          const double rs[4] = {ra[u].x, ra[u].y, rb[u].x, rb[u].y};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const bool ok = lab[k] >= 0 && rs[k] == rs[k];
            const int lb = ok ? lab[k] : -1;
            const double r = ok ? rs[k] : 0.0;
#pragma unroll
            for (int d = 0; d < NB; ++d) {
              const bool h = lb == d;
              hs[d] = hs[d] + (h ? r : 0.0);   // (not fma(0, r, s): 0 * inf poisons)
              cn[d] += h ? 1 : 0;
            }
          }
        }
      }
    }
    if (PRE) dflush();
  } else if (V2) {
    const int64_t step = 2 * DEC_THREADS;
    int64_t i = 2 * (int64_t)tid;
    constexpr int LU = DEC_LU;
    for (; i + (LU - 1) * step < N; i += LU * step) {
      double2 x[LU], r[LU];
#pragma unroll
      for (int u = 0; u < LU; ++u) x[u] = *reinterpret_cast<const double2*>(row + i + u * step);
      if (NB > 0 && nrow) {
#pragma unroll
        for (int u = 0; u < LU; ++u) r[u] = *reinterpret_cast<const double2*>(nrow + i + u * step);
      }
#pragma unroll
      for (int u = 0; u < LU; ++u) {
        const int l0 = label_of(x[u].x), l1 = label_of(x[u].y);
        char2 lv; lv.x = (char)l0; lv.y = (char)l1;
        *reinterpret_cast<char2*>(lrow + i + u * step) = lv;
        if (NB > 0 && nrow) { accumulate(l0, r[u].x); accumulate(l1, r[u].y); }
      }
    }
    for (; i < N; i += step) {
      const double2 x = *reinterpret_cast<const double2*>(row + i);
      const int l0 = label_of(x.x), l1 = label_of(x.y);
      char2 lv; lv.x = (char)l0; lv.y = (char)l1;
      *reinterpret_cast<char2*>(lrow + i) = lv;
      if (NB > 0 && nrow && (l0 >= 0 || l1 >= 0)) {
        const double2 r = *reinterpret_cast<const double2*>(nrow + i);
        accumulate(l0, r.x);
        accumulate(l1, r.y);
      }
    }
  } else {
    for (int64_t i = tid; i < N; i += DEC_THREADS) {
      const int l0 = label_of(row[i]);
      lrow[i] = (int8_t)l0;
      if (NB > 0 && nrow && l0 >= 0) accumulate(l0, nrow[i]);
    }
  }
  dec_mark(tim, t, 8);
  if (NB > 0 && nrow && EW) {
    double fh = 0.0, fl = 0.0;
    int fcn = 0;
    block_sums(fh, fl, fcn);
    if (tid < NB) {
      const int d = tid;
      double h = fh, l = fl;
      int c = fcn;
      if (fast) {   // the merged pass's certain-cell totals, reduced before the selection
        const double h2 = S.x.mg.fh[d];
        const double s2 = h + h2;
        const double bb = s2 - h;
        const double err = (h - (s2 - bb)) + (h2 - bb);
        h = s2; l = (l + S.x.mg.fl[d]) + err; c += S.x.mg.fcn[d];
      }
      const double sum = (h - h == 0.0) ? h + l : h;   // inf sums stay inf (pandas' mean)
      EW[(int64_t)t * NB + d] = c > 0 ? sum / (double)c : qnan();
      if (CNT) CNT[(int64_t)t * NB + d] = c;
    }
  }
  if (MG && FLG && tid == 0) FLG[t] = 0;   // done: the general kernel skips this row
  return true;
}

// The long-short of every date (k_long_short's rule, run_demo.py:55-67) by the launch's last
// workgroup: each workgroup releases its row's EW / CNT and takes a ticket; the one that takes
// the last ticket reads every row.  The ticket wraps by itself (atomicInc with limit T_m - 1
// stores 0 on the last increment), so no reset store follows and a launch leaves it at 0.  One
// stream per context (csm_create): two launches sharing the ticket at once are out of contract.
template <int NB>
__device__ __forceinline__ void dec_ls_tail(const double* __restrict__ EW,
                                            const int32_t* __restrict__ CNT, int T_m,
                                            double* __restrict__ LS, int32_t* __restrict__ ticket) {
  constexpr int nb = NB;
  __shared__ int last, has_lo, has_hi;
  __syncthreads();   // this workgroup's EW / CNT stores are issued
  if (threadIdx.x == 0) {
    __threadfence();   // release them to every XCD
    last = atomicInc((unsigned*)ticket, (unsigned)(T_m - 1)) == (unsigned)(T_m - 1);
    has_lo = 0;
    has_hi = 0;
  }
  __syncthreads();
  if (!last) return;   // block-uniform
  __threadfence();     // acquire every other workgroup's rows (plain loads after the fence)
  for (int t = threadIdx.x; t < T_m; t += DEC_THREADS) {
    if (CNT[(int64_t)t * nb] > 0) atomicOr(&has_lo, 1);
    if (CNT[(int64_t)t * nb + nb - 1] > 0) atomicOr(&has_hi, 1);
  }
  __syncthreads();
  const bool both = has_lo && has_hi;
  for (int t = threadIdx.x; t < T_m; t += DEC_THREADS) {
    int c[NB];
    double e[NB];
#pragma unroll
    for (int d = 0; d < NB; ++d) {   // the row's counts and means, all loads in flight
      c[d] = CNT[(int64_t)t * nb + d];
      e[d] = EW[(int64_t)t * nb + d];
    }
    bool any = false;
    double mx = -INFINITY, mn = INFINITY;
#pragma unroll
    for (int d = 0; d < NB; ++d) {
      if (c[d] > 0) { any = true; mx = fmax(mx, e[d]); mn = fmin(mn, e[d]); }
    }
    double v = qnan();
    if (any) v = both ? (e[nb - 1] - e[0]) : (mx - mn);
    LS[t] = v;
  }
}

// FB (with MG): a row the merged pass gives up runs the general path in the same workgroup
// (no second launch).  LSo (NB > 0, needs ticket): the long-short of every date by the last
// workgroup (no k_long_short launch).
template <int NB, bool V2, bool PRE = false, bool MG = false, bool FB = false, int SPLIT = 0>
// (NB > 10: the per-label sums need more than the 128 VGPRs of two workgroups per CU)
__global__ __launch_bounds__(DEC_THREADS, (NB > 10 ? 1 : SPLIT == 2 ? 2 : (MG && NB == 0) ? DEC_MINB_MG0 : DEC_MINB)) void k_deciles(
    const double* __restrict__ Mx, const double* __restrict__ NRx, int64_t N, int n_bins,
    QTab qt, int8_t* __restrict__ L, double* __restrict__ EW, int32_t* __restrict__ CNT,
    int32_t* __restrict__ NV, int64_t* __restrict__ tim, uint16_t* __restrict__ IDSx,
    int32_t* __restrict__ FLG = nullptr, double* __restrict__ LSo = nullptr,
    int32_t* __restrict__ ticket = nullptr, DecSplit sp = DecSplit{}) {
  static_assert(!FB || MG, "the fallback follows the merged pass");
  static_assert(SPLIT == 0 || !FB, "the split pass leaves given-up rows to its finish launch");
  __shared__ DecShared S;
  const bool done = dec_row<NB, V2, PRE, MG, SPLIT>(S, Mx, NRx, N, n_bins, qt, L, EW, CNT, NV, tim,
                                                     IDSx, FB ? nullptr : FLG, sp);
  if constexpr (FB) {
    if (!done) {   // block-uniform
      __syncthreads();
      dec_row<NB, V2, PRE, false>(S, Mx, NRx, N, n_bins, qt, L, EW, CNT, NV, tim, IDSx, nullptr);
    }
  }
  if constexpr (NB > 0) {
    if (LSo) dec_ls_tail<NB>(EW, CNT, (int)gridDim.x, LSo, ticket);
  }
}
