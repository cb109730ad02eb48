// fsolve.h -- rule MF3: the sequential LDL^T solve of the KF x KF normal equations
// of a factor model, shared by k_factor_model (market.hip) and k_daily_fmodel (dailymkt.hip).
// Every loop bound is a compile-time constant and every loop is unrolled, so A, b, L, D, z and g
// are registers: nothing is indexed at run time and nothing goes to scratch.
#pragma once
#include "csm_common.h"

#define FS_MAXKF 4

// The packed index of the symmetric pair (j, k), j <= k < KF: row-major upper triangle.
__host__ __device__ constexpr int fs_pair(int KF, int j, int k) {
  return j * KF - j * (j - 1) / 2 + (k - j);
}
__host__ __device__ constexpr int fs_pairs(int KF) { return KF * (KF + 1) / 2; }

// A (packed, fs_pair) g = b.  Returns whether the system is defined: every A_jj > 0 and every
// pivot D_j > A_jj * 2^-40 (a factor that is a combination of earlier ones fails, as R5's
// Cholesky pivot test does).  g is written either way; an undefined system's g is not to be used.
// At KF = 1, g_0 = b_0 / A_00 exactly.
template <int KF>
__device__ __forceinline__ bool fs_solve(const double (&A)[KF * (KF + 1) / 2],
                                         const double (&b)[KF], double (&g)[KF]) {
  double L[KF][KF], D[KF], z[KF];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < KF; ++j) {
    const double ajj = A[fs_pair(KF, j, j)];
    double d = ajj;
#pragma unroll
    for (int p = 0; p < j; ++p) d = d - (L[j][p] * L[j][p]) * D[p];
    ok = ok && ajj > 0.0 && d > ajj * 0x1p-40;
    D[j] = d;
#pragma unroll
    for (int i = j + 1; i < KF; ++i) {
      double v = A[fs_pair(KF, j, i)];
#pragma unroll
      for (int p = 0; p < j; ++p) v = v - (L[i][p] * L[j][p]) * D[p];
      L[i][j] = v / d;
    }
  }
#pragma unroll
  for (int j = 0; j < KF; ++j) {
    double v = b[j];
#pragma unroll
    for (int p = 0; p < j; ++p) v = v - L[j][p] * z[p];
    z[j] = v;
  }
#pragma unroll
  for (int j = KF - 1; j >= 0; --j) {
    double v = z[j] / D[j];
#pragma unroll
    for (int p = j + 1; p < KF; ++p) v = v - L[p][j] * g[p];
    g[j] = v;
  }
  return ok;
}
