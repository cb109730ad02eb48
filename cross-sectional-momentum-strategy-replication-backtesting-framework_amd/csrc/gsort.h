// gsort.h -- the sort-and-pack core groups.hip and breakpoints.hip share.
//   device: the block sum (csm_common.h's wave tree, then the waves in order), the predicate pack
//           of a row in asset order (pack_row), the bitonic sort of exactly n keys in LDS
//           (tile_sort) or in a packed global row (seg_sort) behind sort_segment, and NumPy's lerp
//           for one qcut edge on sorted keys.
//   host:   the LDS / tiled hand-over (sort_plan) and the launch of a kernel's two instantiations,
//           and the qtable and n_bins checks.
#pragma once
#include "csm_common.h"

#define GD_TILE 4096       // keys of one LDS sort (32 KiB)
#define GD_SMALL_THREADS 256
#define GD_LONG_THREADS 1024

// ----------------------------------------------------------------------------------- host
static inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// Segments of at most cap keys are sorted in LDS, longer ones in tiles of `tile` keys: csm_tune
// "gdec_small_cap" lowers cap from GD_TILE, the tile is then twice the next power of two, GD_TILE
// at most (groups.hip holds the knob).
struct SortPlan {
  int cap, tile;
};
SortPlan sort_plan();

// K<true> (LDS) and K<false> (tiled) over the same grid; each returns at once on the other's
// segments (not_mine).
#define LAUNCH_PAIR(ctx, K, grid, ...)                                                     \
  do {                                                                                     \
    hipLaunchKernelGGL(K<true>, dim3(grid), dim3(GD_SMALL_THREADS), 0, (ctx)->stream,      \
                       __VA_ARGS__);                                                       \
    LAUNCH_CHECK(ctx, #K " (LDS)");                                                        \
    hipLaunchKernelGGL(K<false>, dim3(grid), dim3(GD_LONG_THREADS), 0, (ctx)->stream,      \
                       __VA_ARGS__);                                                       \
    LAUNCH_CHECK(ctx, #K " (tiled)");                                                      \
  } while (0)

static inline QTab qtab_fill(const double* qtable, int n_bins) {
  QTab q{};
  for (int i = 0; i < MAXQ; ++i) q.q[i] = i <= n_bins ? qtable[i] : 1.0;
  return q;
}

// n_bins fits a QTab and, with NR, is a bin count the decile sums are compiled for
static inline int check_n_bins(csm_ctx* ctx, const char* who, int32_t n_bins, bool with_nr) {
  if (n_bins < 1 || n_bins > MAXQ - 1)
    return set_err(ctx, CSM_E_INVAL, "%s: n_bins=%d is outside [1, %d]", who, n_bins, MAXQ - 1);
  if (with_nr && !nb_dispatch<2, 3, 4, 5, 10, 20>(n_bins, [](auto) {}))
    return set_err(ctx, CSM_E_INVAL, "%s: n_bins=%d unsupported with NR (use 2,3,4,5,10,20)", who,
                   n_bins);
  return CSM_OK;
}

// --------------------------------------------------------------------------------- device
// Lane values -> their sum, in every lane: the tree per wave, then the waves in wave order from
// zero.  s_part: NT / 64 entries of LDS; the first barrier waits for its last readers, so one
// buffer serves sums in a row.
template <typename T, int NT>
__device__ __forceinline__ T block_sum(T v, T* s_part) {
  const int tid = threadIdx.x;
  v = wave_tree(v);
  __syncthreads();
  if ((tid & 63) == 0) s_part[tid >> 6] = v;
  __syncthreads();
  T r = T(0);
#pragma unroll 4   // (unrolled fully, 16 waves' int64 partials at once take k_ic from 8 waves per
                   // SIMD to 5)
  for (int w = 0; w < NT / 64; ++w) r = r + s_part[w];
  return r;
}

// The cells [i0, i1) of an N-cell row that this thread's wave, one of NT / 64, sweeps: contiguous
// chunks of a whole number of 64-cell steps, in wave order.
struct Chunk {
  int64_t i0, i1;
};
template <int NT>
__device__ __forceinline__ Chunk wave_chunk(int64_t N) {
  const int64_t per = ((N + NT - 1) / NT) * 64;
  const int64_t i0 = (int64_t)(threadIdx.x >> 6) * per;
  return {i0, i0 + per < N ? i0 + per : N};
}

// Packs the cells i of an N-cell row with in(i), in asset order: emit(i, pos) for each of them,
// pos its position among them, right after the lane's own in(i) -- what in loaded it may leave
// for emit.  Returns their number.  Each wave counts its chunk by ballot, an exclusive prefix over
// the waves (s_cnt: NT / 64 ints of LDS) gives its first position, a second sweep places the
// cells by lane_prefix.
template <int NT, typename In, typename Emit>
__device__ __forceinline__ int pack_row(int64_t N, int* s_cnt, In in, Emit emit) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Chunk ch = wave_chunk<NT>(N);
  int c = 0;
  for (int64_t b = ch.i0; b < ch.i1; b += 64) {   // (wave-uniform trips)
    const int64_t i = b + lane;
    c += __popcll(__ballot(i < ch.i1 && in(i)));
  }
  if (lane == 0) s_cnt[wave] = c;
  __syncthreads();
  int base = 0, tot = 0;
  for (int w = 0; w < NT / 64; ++w) {
    const int v = s_cnt[w];
    base += w < wave ? v : 0;
    tot += v;
  }
  for (int64_t b = ch.i0; b < ch.i1; b += 64) {
    const int64_t i = b + lane;
    const bool ok = i < ch.i1 && in(i);
    const uint64_t m = __ballot(ok);
    if (ok) emit(i, base + lane_prefix(m));
    base += __popcll(m);
  }
  return tot;
}

__device__ __forceinline__ void cmpx(double* a, uint32_t lo, uint32_t hi) {
  const double x = a[lo], y = a[hi];
  if (x > y) {
    a[lo] = y;
    a[hi] = x;
  }
}
// the first exchange of the merge of width k: lo with lo ^ (k - 1), over a[0..len)
template <int NT>
__device__ __forceinline__ void bit_flip(double* a, uint32_t len, uint32_t k) {
  const uint32_t h = k >> 1;
  for (uint32_t q = threadIdx.x;; q += NT) {
    const uint32_t lo = ((q & ~(h - 1)) << 1) | (q & (h - 1));
    if (lo >= len) break;
    const uint32_t hi = lo ^ (k - 1);
    if (hi < len) cmpx(a, lo, hi);
  }
}
// a later exchange of a merge: lo with lo + j
template <int NT>
__device__ __forceinline__ void bit_step(double* a, uint32_t len, uint32_t j) {
  for (uint32_t q = threadIdx.x;; q += NT) {
    const uint32_t lo = ((q & ~(j - 1)) << 1) | (q & (j - 1));
    if (lo >= len) break;
    const uint32_t hi = lo + j;
    if (hi < len) cmpx(a, lo, hi);
  }
}
// sorts s[0..len) (LDS), len <= GD_TILE
template <int NT>
__device__ __forceinline__ void tile_sort(double* s, uint32_t len) {
  for (uint32_t k = 2; (k >> 1) < len; k <<= 1) {
    bit_flip<NT>(s, len, k);
    __syncthreads();
    for (uint32_t j = k >> 2; j > 0; j >>= 1) {
      bit_step<NT>(s, len, j);
      __syncthreads();
    }
  }
}

// sorts gk[0..un) (the packed row), un past the LDS cap: tiles of tl keys sorted in s (LDS), the
// exchanges wider than a tile made in gk itself
template <int NT>
__device__ __forceinline__ void seg_sort(double* gk, double* s, uint32_t un, uint32_t tl) {
  const uint32_t tid = threadIdx.x;
  for (uint32_t tb = 0; tb < un; tb += tl) {
    const uint32_t len = un - tb < tl ? un - tb : tl;
    for (uint32_t p = tid; p < len; p += NT) s[p] = gk[tb + p];
    __syncthreads();
    tile_sort<NT>(s, len);
    for (uint32_t p = tid; p < len; p += NT) gk[tb + p] = s[p];
    __syncthreads();
  }
  for (uint32_t k = 2 * tl; k != 0 && (k >> 1) < un; k <<= 1) {
    bit_flip<NT>(gk, un, k);
    __syncthreads();
    for (uint32_t j = k >> 2; j >= tl; j >>= 1) {
      bit_step<NT>(gk, un, j);
      __syncthreads();
    }
    for (uint32_t tb = 0; tb < un; tb += tl) {   // the exchanges narrower than a tile
      const uint32_t len = un - tb < tl ? un - tb : tl;
      for (uint32_t p = tid; p < len; p += NT) s[p] = gk[tb + p];
      __syncthreads();
      for (uint32_t j = tl >> 1; j > 0; j >>= 1) {
        bit_step<NT>(s, len, j);
        __syncthreads();
      }
      for (uint32_t p = tid; p < len; p += NT) gk[tb + p] = s[p];
      __syncthreads();
    }
  }
}

// A sort kernel is launched twice over the same grid: SMALL takes the segments of at most cap
// keys, the other launch the longer ones.  True on the other launch's segment (block-uniform).
template <bool SMALL>
__device__ __forceinline__ bool not_mine(int n, int cap) {
  return SMALL ? n > cap : n <= cap;
}
// Sorts the n keys gk[0..n) of a packed row and returns the sorted keys: SMALL in s_key (LDS,
// GD_TILE doubles; gk keeps its asset order), otherwise in gk itself by tiles through s_key.
template <bool SMALL, int NT>
__device__ __forceinline__ const double* sort_segment(double* gk, double* s_key, int n, int tile) {
  if (SMALL) {
    for (int p = threadIdx.x; p < n; p += NT) s_key[p] = gk[p];
    __syncthreads();
    tile_sort<NT>(s_key, (uint32_t)n);
    return s_key;
  }
  seg_sort<NT>(gk, s_key, (uint32_t)n, (uint32_t)tile);
  return gk;
}

// edge q of the n sorted keys srt: NumPy's percentile(method='linear') lerp, as deciles.inc
__device__ __forceinline__ double qcut_edge(const double* srt, int n, double q) {
  const double v = (double)(n - 1) * q;
  if (v >= (double)(n - 1)) return srt[n - 1];
  const double p = floor(v);
  const double gm = v - p;
  const int pi = (int)p;
  const double a = srt[pi];
  const double b = (gm != 0.0) ? srt[pi + 1] : a;
  const double d = b - a;
  return (gm >= 0.5) ? (b - d * (1.0 - gm)) : (a + d * gm);
}
