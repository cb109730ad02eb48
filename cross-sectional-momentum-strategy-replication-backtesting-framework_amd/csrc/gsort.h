// gsort.h -- the device helpers groups.hip and breakpoints.hip share: the wave halving tree, the
// bitonic sort of exactly n keys in LDS (tile_sort) or in a packed global row (seg_sort), and
// NumPy's lerp for one qcut edge on sorted keys.
#pragma once
#include "csm_common.h"

#define GD_TILE 4096       // keys of one LDS sort (32 KiB)
#define GD_SMALL_THREADS 256
#define GD_LONG_THREADS 1024

static inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

__device__ __forceinline__ double gwave_tree(double v) {
#pragma unroll
  for (int h = 32; h > 0; h >>= 1) v = v + __shfl_down(v, h, 64);
  return v;
}
__device__ __forceinline__ int gwave_tree(int v) {
#pragma unroll
  for (int h = 32; h > 0; h >>= 1) v = v + __shfl_down(v, h, 64);
  return v;
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
