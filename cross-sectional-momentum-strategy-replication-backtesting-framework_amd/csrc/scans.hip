// scans.hip -- the unfused month-end and momentum scans over [T][N] panels.  HBM- or latency-
// bound fp64 work, nothing is a contraction, so no MFMA.  Built with -ffp-contract=off: the fp64
// products and quotients must round exactly like NumPy / pandas.
// Reference behaviour restated (file:line into the reference):
//   month-end         src/features.py:34-39   (groupby ticker x Grouper('ME'): last / sum)
//   ret/mom scan      src/features.py:44-52   (pct_change ffill; shift(skip).rolling(J) prod)
//   next_ret          run_demo.py:48          (pct_change within the ranked subset, shift(-1))
//
//   k_month_end             a thread per (month, VEC assets): the month's last valid price and
//                           the Kahan sum of its volumes, days walked in order.
//   k_momentum              a thread per asset walks the month prices with scan.h's step, the
//                           J + skip ring in LDS; carry in and out for date shards.
//   k_momentum_chunked      the same scan with the months split into chunks, each from the carry
//                           that shards.hip's k_fold_carry rebuilt for it (small N).
//   k_momentum_multi        several look-backs in one scan over one ring of max(J) + skip
//   k_momentum_multi_reg    factors: the ring in LDS, as a register shift ring, and the register
//   k_momentum_multi_reg2   ring with two assets per lane, which is also the chunked form.
#include "csm_common.h"
#include "scan.h"
#include "shard.h"

// =====================================================================================
// Kernel A: month-end aggregation.  One thread per (month, VEC assets); a wave streams
// 64*VEC*8 contiguous bytes per day row (1 KiB at VEC=2).  Days of a month are walked in
// order so the Kahan volume sum matches pandas' group_sum bit for bit.
// =====================================================================================
template <int VEC, bool WITH_VOL>
__global__ __launch_bounds__(256) void k_month_end(const double* __restrict__ P,
                                                   const double* __restrict__ V,
                                                   const int64_t* __restrict__ month_start,
                                                   int64_t N, double* __restrict__ PM,
                                                   double* __restrict__ VOL) {
  const int m = blockIdx.y;
  const int64_t a = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
  if (a >= N) return;
  const int64_t d0 = month_start[m], d1 = month_start[m + 1];
  double last[VEC];
  bool anyp[VEC], anyv[VEC];
  double s[VEC], c[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    last[k] = 0.0; anyp[k] = false; anyv[k] = false; s[k] = 0.0; c[k] = 0.0;
  }
  const double* p = P + d0 * N + a;
  const double* v = WITH_VOL ? V + d0 * N + a : nullptr;
  int64_t d = d0;
  // prices only, a business month (<= 24 rows): every row load in flight at once, one round
  // trip per thread (the 8-row batches and the serial tail below took three to eight); rows
  // past the month are ABSENT placeholders, which change nothing
  constexpr int MD = 24;
  if (!WITH_VOL && d1 - d0 <= MD) {
    const int nd = (int)(d1 - d0);
    double x[MD][VEC];
#pragma unroll
    for (int j = 0; j < MD; ++j) {
      if (j < nd) {
        if (VEC == 2) {
          const double2 t = *reinterpret_cast<const double2*>(p + (int64_t)j * N);
          x[j][0] = t.x; x[j][VEC - 1] = t.y;
        } else {
          x[j][0] = p[(int64_t)j * N];
        }
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) x[j][k] = absent_val();
      }
    }
#pragma unroll
    for (int j = 0; j < MD; ++j) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const bool pr = !is_absent(x[j][k]);
        const bool ok = pr && !isnan_d(x[j][k]);
        anyp[k] |= pr;
        anyv[k] |= ok;
        last[k] = ok ? x[j][k] : last[k];
      }
    }
    d = d1;
  }
  // 8-day batches keep 8 row loads in flight per lane before the dependent selects.
  for (; d + 8 <= d1; d += 8) {
    double x[8][VEC];
    double y[WITH_VOL ? 8 : 1][VEC];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (VEC == 2) {
        double2 t = *reinterpret_cast<const double2*>(p + j * N);
        x[j][0] = t.x; x[j][VEC - 1] = t.y;
        if (WITH_VOL) { double2 u = *reinterpret_cast<const double2*>(v + j * N); y[j][0] = u.x; y[j][VEC - 1] = u.y; }
      } else {
        x[j][0] = p[j * N];
        if (WITH_VOL) y[j][0] = v[j * N];
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const bool pr = !is_absent(x[j][k]);
        const bool ok = pr && !isnan_d(x[j][k]);
        anyp[k] |= pr;
        anyv[k] |= ok;
        last[k] = ok ? x[j][k] : last[k];
        if (WITH_VOL && pr) {
          double val = y[j][k];
          val = isnan_d(val) ? 0.0 : val;
          const double yy = val - c[k];
          const double tt = s[k] + yy;
          double cc = (tt - s[k]) - yy;
          c[k] = isnan_d(cc) ? 0.0 : cc;
          s[k] = tt;
        }
      }
    }
    p += 8 * N;
    if (WITH_VOL) v += 8 * N;
  }
  for (; d < d1; ++d) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const double xv = p[k];
      const bool pr = !is_absent(xv);
      const bool ok = pr && !isnan_d(xv);
      anyp[k] |= pr;
      anyv[k] |= ok;
      last[k] = ok ? xv : last[k];
      if (WITH_VOL && pr) {
        double val = v[k];
        val = isnan_d(val) ? 0.0 : val;
        const double yy = val - c[k];
        const double tt = s[k] + yy;
        double cc = (tt - s[k]) - yy;
        c[k] = isnan_d(cc) ? 0.0 : cc;
        s[k] = tt;
      }
    }
    p += N;
    if (WITH_VOL) v += N;
  }
  double out[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) out[k] = anyp[k] ? (anyv[k] ? last[k] : qnan()) : absent_val();
  double* o = PM + (int64_t)m * N + a;
  if (VEC == 2) {
    *reinterpret_cast<double2*>(o) = make_double2(out[0], out[VEC - 1]);
  } else {
    o[0] = out[0];
  }
  if (WITH_VOL) {
    double* w = VOL + (int64_t)m * N + a;
#pragma unroll
    for (int k = 0; k < VEC; ++k) w[k] = anyp[k] ? s[k] : 0.0;
  }
}

// =====================================================================================
// Kernel B: per-asset scan over month prices (present rows only).  One thread per asset;
// PM rows prefetched SCAN_CHUNK months ahead (SCAN_CHUNK * 512 B in flight per wave).
// =====================================================================================
#define SCAN_THREADS 128
#define SCAN_CHUNK 16

__device__ __forceinline__ void momentum_body(
    double* ring_lds, const double* __restrict__ PM, int T_m, int64_t N, int J, int skip,
    double* __restrict__ R, double* __restrict__ M, double* __restrict__ NR,
    const double* __restrict__ carry, const double* __restrict__ next_pm,
    double* __restrict__ carry_out, uint16_t* __restrict__ IDS = nullptr);

__global__ __launch_bounds__(256) void k_momentum(
    const double* __restrict__ PM, int T_m, int64_t N, int J, int skip, double* __restrict__ R,
    double* __restrict__ M, double* __restrict__ NR, const double* __restrict__ carry,
    const double* __restrict__ next_pm, double* __restrict__ carry_out) {
  extern __shared__ __attribute__((aligned(16))) double ring_lds[];
  momentum_body(ring_lds, PM, T_m, N, J, skip, R, M, NR, carry, next_pm, carry_out);
}

// Time-chunked scan (small N): chunk blockIdx.y scans its month range from the carry that
// k_fold_carry rebuilt for it -- C x more waves in flight, same results bit for bit.
__global__ __launch_bounds__(256) void k_momentum_chunked(
    const double* __restrict__ PM, int T_m, int G, int64_t N, int J, int skip,
    double* __restrict__ R, double* __restrict__ M, double* __restrict__ NR,
    const double* __restrict__ carry, const double* __restrict__ next_pm,
    uint16_t* __restrict__ IDS) {
  extern __shared__ __attribute__((aligned(16))) double ring_lds[];
  const int g = blockIdx.y;
  int m0, m1;
  chunk_range(T_m, G, g, m0, m1);
  const int W = J + skip;
  const int64_t off = (int64_t)m0 * N;
  momentum_body(ring_lds, PM + off, m1 - m0, N, J, skip, R ? R + off : nullptr, M + off,
                NR + off, g > 0 ? carry + (int64_t)g * (W + 2) * N : nullptr,
                next_pm + (int64_t)g * N, nullptr, IDS ? IDS + off : nullptr);
}

__device__ __forceinline__ void momentum_body(
    double* ring_lds, const double* __restrict__ PM, int T_m, int64_t N, int J, int skip,
    double* __restrict__ R, double* __restrict__ M, double* __restrict__ NR,
    const double* __restrict__ carry, const double* __restrict__ next_pm,
    double* __restrict__ carry_out, uint16_t* __restrict__ IDS) {
  const int W = J + skip;
  const int tid = threadIdx.x;
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + tid;
  const bool live = a < N;
  const int RS = blockDim.x;
  double* ring = ring_lds + tid;
  ScanLane s;
  scan_init(s, ring, RS, W, carry, N, a, live);
  if (!live) return;
  for (int m0 = 0; m0 < T_m; m0 += SCAN_CHUNK) {
    double buf[SCAN_CHUNK];
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j)
      buf[j] = (m0 + j < T_m) ? PM[(int64_t)(m0 + j) * N + a] : absent_val();
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) {
      const int m = m0 + j;
      if (m >= T_m) break;
      const double mom = scan_step(s, buf[j], m, ring, RS, W, J, N, a, R, M, NR);
      if (IDS) IDS[(int64_t)m * N + a] = (uint16_t)csm_fid(mom);   // the decile pass's bucket id
    }
  }
  scan_finish(s, ring, RS, W, N, a, NR, next_pm, carry_out);
}

// Several look-backs in one scan (parameter sweeps, C3 / C5): one read of PM, one ring of
// Jmax + skip factors fl(1 + ret), and per J the sequential product over the oldest J of its
// last J + skip factors -- the same factors in the same order as k_momentum with a ring of
// exactly J + skip, so M and NR are bit-identical to per-J k_momentum calls.  NR is kept per
// J: the ranked subset (and so next_ret's subset-ffill, run_demo.py:48) starts J + skip
// present months after the first price.  No carry / next_pm (whole panels only).
struct MJSet {
  int J[MJ_MAX];
  double* M[MJ_MAX];
  double* NR[MJ_MAX];
  uint16_t* IDS[MJ_MAX];   // nullable: fixed-map bucket ids of M (csm_momentum_multi_ids)
};

__global__ __launch_bounds__(256) void k_momentum_multi(const double* __restrict__ PM, int T_m,
                                                        int64_t N, int nJ, int skip, int W,
                                                        MJSet mj) {
  extern __shared__ __attribute__((aligned(16))) double ring_lds[];
  const int tid = threadIdx.x;
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + tid;
  if (a >= N) return;   // no barriers below
  const int RS = blockDim.x;
  double* ring = ring_lds + tid;
  const double NaN = qnan();
  for (int k = 0; k < W; ++k) ring[k * RS] = NaN;
  int head = 0;
  double pff = NaN;
  double psff[MJ_MAX];
  int prev[MJ_MAX];
#pragma unroll
  for (int q = 0; q < MJ_MAX; ++q) { psff[q] = NaN; prev[q] = -1; }
  for (int m0 = 0; m0 < T_m; m0 += SCAN_CHUNK) {
    double buf[SCAN_CHUNK];
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j)
      buf[j] = (m0 + j < T_m) ? PM[(int64_t)(m0 + j) * N + a] : absent_val();
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) {
      const int m = m0 + j;
      if (m >= T_m) break;
      const double x = buf[j];
      const int64_t o = (int64_t)m * N + a;
      if (is_absent(x)) {
#pragma unroll
        for (int q = 0; q < MJ_MAX; ++q)
          if (q < nJ) {
            mj.M[q][o] = NaN; mj.NR[q][o] = NaN;
            if (mj.IDS[q]) mj.IDS[q][o] = (uint16_t)CSM_FB_NAN;
          }
        continue;
      }
      const double ret = price_step(x, pff);
      lds_push(ring, RS, W, head, 1.0 + ret);
#pragma unroll
      for (int q = 0; q < MJ_MAX; ++q) {
        if (q >= nJ) break;
        const int J = mj.J[q];
        int idx = head + (W - J - skip);      // oldest of this J's window
        if (idx >= W) idx -= W;
        const double mom = lds_prod(ring, RS, W, J, idx) - 1.0;
        double* NRq = mj.NR[q];
        if (rank_step(x, mom, m, psff[q], prev[q],
                      [&](int row, double nr) { NRq[(int64_t)row * N + a] = nr; }))
          NRq[o] = NaN;
        mj.M[q][o] = mom;
        if (mj.IDS[q]) mj.IDS[q][o] = (uint16_t)csm_fid(mom);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < MJ_MAX; ++q)
    if (q < nJ && prev[q] >= 0) mj.NR[q][(int64_t)prev[q] * N + a] = NaN;
}

// Register-ring variant for max(J) + skip <= RW: the last RW factors live in registers as a
// shift register (f[RW-1] newest), and J's product runs over all RW slots with the slots
// outside its window predicated off.  acc starts at 1.0 and 1.0 * x == x exactly, so the
// product is still oldest-first over the same factors: bit-identical, no LDS round trips.
template <int RW>
__global__ __launch_bounds__(256) void k_momentum_multi_reg(const double* __restrict__ PM,
                                                            int T_m, int64_t N, int nJ, int skip,
                                                            MJSet mj) {
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= N) return;
  const double NaN = qnan();
  double f[RW];
#pragma unroll
  for (int k = 0; k < RW; ++k) f[k] = NaN;
  double pff = NaN;
  double psff[MJ_MAX];
  int prev[MJ_MAX], lo[MJ_MAX];
#pragma unroll
  for (int q = 0; q < MJ_MAX; ++q) {
    psff[q] = NaN; prev[q] = -1;
    lo[q] = RW - mj.J[q] - skip;   // window = slots [lo, RW - skip)
  }
  const int hi = RW - skip;
  for (int m0 = 0; m0 < T_m; m0 += SCAN_CHUNK) {
    double buf[SCAN_CHUNK];
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j)
      buf[j] = (m0 + j < T_m) ? PM[(int64_t)(m0 + j) * N + a] : absent_val();
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) {
      const int m = m0 + j;
      if (m >= T_m) break;
      const double x = buf[j];
      const int64_t o = (int64_t)m * N + a;
      if (is_absent(x)) {
#pragma unroll
        for (int q = 0; q < MJ_MAX; ++q)
          if (q < nJ) {
            mj.M[q][o] = NaN; mj.NR[q][o] = NaN;
            if (mj.IDS[q]) mj.IDS[q][o] = (uint16_t)CSM_FB_NAN;
          }
        continue;
      }
      const double ret = price_step(x, pff);
      reg_push(f, 1.0 + ret);
#pragma unroll
      for (int q = 0; q < MJ_MAX; ++q) {
        if (q >= nJ) break;
        const double mom = mj_window<RW, false>(f, q, lo[q], hi) - 1.0;
        double* NRq = mj.NR[q];
        if (rank_step(x, mom, m, psff[q], prev[q],
                      [&](int row, double nr) { NRq[(int64_t)row * N + a] = nr; }))
          NRq[o] = NaN;
        mj.M[q][o] = mom;
        if (mj.IDS[q]) mj.IDS[q][o] = (uint16_t)csm_fid(mom);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < MJ_MAX; ++q)
    if (q < nJ && prev[q] >= 0) mj.NR[q][(int64_t)prev[q] * N + a] = NaN;
}
// Two adjacent assets per lane (a0 even): 16-B PM loads, mom_J / next_ret as one 16-B store
// per row when both assets write the same row (as k_signal's scan_step_pair), ids as one 4-B
// store: a wave moves 1 KiB per load / store instruction.  Same arithmetic per asset in the
// same order as k_momentum_multi_reg: bit-identical outputs.  N even, 16-B aligned buffers.
#define MJ2_CHUNK 8
// CH (csm_momentum_multi_chunked): chunk blockIdx.y of G scans its month range [ms, me) from
// the carry k_fold_carry rebuilt for max(J) (the last max(J) + skip factors, the month price
// pff) plus each J's subset-ffilled price psf[g][q] -- a smaller J's ring is the newest J + skip
// of the same factors -- and finishes its pending rows with npm[g] (the next chunk's first
// present price), as k_momentum_chunked does per J: the same bits.
// FIX: the default grid J = 3, 6, 9, 12 (in that order), skip 1, in a 13-slot ring with
// compile-time windows (J - 1 multiplies each, no predicated slots): the same oldest-first
// product (1.0 * x == x), about half the code -- the predicated chunked kernel was 85 KB, past
// the instruction cache (mj_window).
// The step's pieces run on every row with the state kept by selects on the absent predicate,
// not a branch: an absent row's x is a NaN, so price_step leaves pff as it is by itself.
template <int RW, bool CH = false, bool FIX = false>
__global__ __launch_bounds__(256) void k_momentum_multi_reg2(const double* __restrict__ PM,
                                                             int T_m, int64_t N, int nJ, int skip,
                                                             MJSet mj, int G = 1,
                                                             const double* __restrict__ carry = nullptr,
                                                             const double* __restrict__ npm = nullptr,
                                                             const double* __restrict__ psf = nullptr) {
  const int64_t a0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
  if (a0 >= N) return;
  const double NaN = qnan();
  double f[2][RW];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int k = 0; k < RW; ++k) f[c][k] = NaN;
  double pff[2] = {NaN, NaN};
  double psff[2][MJ_MAX];
  int prev[2][MJ_MAX], lo[MJ_MAX];
  int Wmax = 0;
#pragma unroll
  for (int q = 0; q < MJ_MAX; ++q) {
    psff[0][q] = psff[1][q] = NaN;
    prev[0][q] = prev[1][q] = -1;
    lo[q] = RW - mj.J[q] - skip;   // window = slots [lo, RW - skip)
    if (q < nJ && mj.J[q] + skip > Wmax) Wmax = mj.J[q] + skip;
  }
  const int hi = RW - skip;
  int ms = 0, me = T_m;
  const int g = CH ? (int)blockIdx.y : 0;
  if (CH) {
    chunk_range(T_m, G, g, ms, me);
    if (g > 0) {   // the carried state: ring slots [RW - Wmax, RW) oldest first, pff, psff per J
      const double* cg = carry + (int64_t)g * (Wmax + 2) * N + a0;
#pragma unroll
      for (int k = 0; k < RW; ++k)
        if (k >= RW - Wmax) {
          const double2 v = *reinterpret_cast<const double2*>(cg + (int64_t)(k - (RW - Wmax)) * N);
          f[0][k] = v.x;
          f[1][k] = v.y;
        }
      const double2 pv = *reinterpret_cast<const double2*>(cg + (int64_t)Wmax * N);
      pff[0] = pv.x;
      pff[1] = pv.y;
#pragma unroll
      for (int q = 0; q < MJ_MAX; ++q)
        if (q < nJ) {
          const double2 v = *reinterpret_cast<const double2*>(psf + ((int64_t)g * MJ_MAX + q) * N + a0);
          psff[0][q] = v.x;
          psff[1][q] = v.y;
        }
    }
  }
  for (int m0 = ms; m0 < me; m0 += MJ2_CHUNK) {
    double2 buf[MJ2_CHUNK];
#pragma unroll
    for (int j = 0; j < MJ2_CHUNK; ++j)
      buf[j] = (m0 + j < me) ? *reinterpret_cast<const double2*>(PM + (int64_t)(m0 + j) * N + a0)
                             : make_double2(absent_val(), absent_val());
#pragma unroll
    for (int j = 0; j < MJ2_CHUNK; ++j) {
      const int m = m0 + j;
      if (m >= me) break;
      const double xs[2] = {buf[j].x, buf[j].y};
      const int64_t o = (int64_t)m * N + a0;
      bool ab[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        ab[c] = is_absent(xs[c]);
        const double ret = price_step(xs[c], pff[c]);   // (an absent x is a NaN: pff stays)
        // reg_push restated with selects on the absent predicate (through the shared function the
        // chunked FIX instantiation grows 4 % and C3's scan stage 3 %)
#pragma unroll
        for (int k = 0; k + 1 < RW; ++k) f[c][k] = ab[c] ? f[c][k] : f[c][k + 1];
        f[c][RW - 1] = ab[c] ? f[c][RW - 1] : 1.0 + ret;
      }
#pragma unroll
      for (int q = 0; q < MJ_MAX; ++q) {
        if (q >= nJ) break;
        double mom[2], vp[2];
        int wp[2];
        bool wc[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const double acc = mj_window<RW, FIX>(f[c], q, lo[q], hi);
          mom[c] = ab[c] ? NaN : acc - 1.0;
          // rank_step restated with selects on the absent predicate (no branch in this kernel)
          const double ps_new = ffill(xs[c], psff[c][q]);
          wp[c] = (!ab[c] && prev[c][q] >= 0) ? prev[c][q] : -1;
          vp[c] = subset_ret(ps_new, psff[c][q]);
          const bool ranked = mom[c] == mom[c];
          wc[c] = !ranked;
          psff[c][q] = ranked ? ps_new : psff[c][q];
          prev[c][q] = ranked ? m : (ab[c] ? prev[c][q] : -1);
        }
        store_pair(mj.M[q] + o, mom[0], mom[1]);
        store_next_ret_pair(mj.NR[q], N, a0, o, wp, vp, wc);
        if (mj.IDS[q])
          *reinterpret_cast<uint32_t*>(mj.IDS[q] + o) = csm_fid(mom[0]) | (csm_fid(mom[1]) << 16);
      }
    }
  }
  // pending ranked rows: next_ret from the next chunk's first present price (CH), else NaN
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const double x = CH ? npm[(int64_t)g * N + a0 + c] : absent_val();
#pragma unroll
    for (int q = 0; q < MJ_MAX; ++q)
      if (q < nJ && prev[c][q] >= 0)
        mj.NR[q][(int64_t)prev[c][q] * N + a0 + c] = pending_finish(x, psff[c][q]);
  }
}

#define MJ_REG_W 16

// csm_momentum_multi: 2 register shift ring, two assets per lane (even N, aligned) | 1 one asset
// per lane | 0 the shared-memory ring (max(J) + skip > 16 always takes it)
static int g_tune_mj_reg = 2;
static const TuneKnob g_knobs[] = {
    {"mj_reg", &g_tune_mj_reg, [](int v) { return v >= 0 && v <= 2; }},
};
int csm_tune_scans(const char* key, int value) { return tune_set(g_knobs, key, value); }

extern "C" {

int csm_month_end(csm_ctx* ctx, const double* P, const double* V, int64_t T_d, int64_t N,
                  const int64_t* month_start, int32_t T_m, double* PM, double* VOL) {
  int r = prep(ctx);
  if (r) return r;
  if (!P || !month_start || !PM || N <= 0 || T_d < 0 || T_m < 0 || T_m > 65535)
    return set_err(ctx, CSM_E_INVAL, "csm_month_end: bad arguments (N=%lld T_d=%lld T_m=%d)",
                   (long long)N, (long long)T_d, T_m);
  if ((V == nullptr) != (VOL == nullptr))
    return set_err(ctx, CSM_E_INVAL, "csm_month_end: V and VOL must both be given or both NULL");
  if (T_m == 0) return CSM_OK;
  const bool v2 = (N % 2 == 0) && aligned16(P) && aligned16(PM) && (!V || aligned16(V));
  const int vec = v2 ? 2 : 1;
  dim3 grid((unsigned)((N + 256LL * vec - 1) / (256LL * vec)), (unsigned)T_m);
  if (v2) {
    if (V) hipLaunchKernelGGL((k_month_end<2, true>), grid, dim3(256), 0, ctx->stream, P, V, month_start, N, PM, VOL);
    else hipLaunchKernelGGL((k_month_end<2, false>), grid, dim3(256), 0, ctx->stream, P, V, month_start, N, PM, VOL);
  } else {
    if (V) hipLaunchKernelGGL((k_month_end<1, true>), grid, dim3(256), 0, ctx->stream, P, V, month_start, N, PM, VOL);
    else hipLaunchKernelGGL((k_month_end<1, false>), grid, dim3(256), 0, ctx->stream, P, V, month_start, N, PM, VOL);
  }
  LAUNCH_CHECK(ctx, "k_month_end");
  return CSM_OK;
}

int csm_momentum(csm_ctx* ctx, const double* PM, int32_t T_m, int64_t N, int32_t J, int32_t skip,
                 double* R, double* M, double* NR, const double* carry, const double* next_pm,
                 double* carry_out) {
  int r = prep(ctx);
  if (r) return r;
  if (!PM || !M || !NR || N <= 0 || T_m < 0 || J < 1 || skip < 0 || J + skip > 256)
    return set_err(ctx, CSM_E_INVAL, "csm_momentum: bad arguments (N=%lld T_m=%d J=%d skip=%d)",
                   (long long)N, T_m, J, skip);
  const int W = J + skip;
  const int tpb = W <= 64 ? SCAN_THREADS : 64;  // ring = W * tpb doubles of LDS (<= 128 KiB)
  const size_t lds = (size_t)W * tpb * sizeof(double);
  const unsigned blocks = (unsigned)((N + tpb - 1) / tpb);
  if (lds > 65536)
    HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k_momentum,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_momentum, dim3(blocks), dim3(tpb), lds, ctx->stream, PM, T_m, N, J,
                     skip, R, M, NR, carry, next_pm, carry_out);
  LAUNCH_CHECK(ctx, "k_momentum");
  return CSM_OK;
}

static bool mj_fixed_grid(const int32_t* Js, int nJ, int skip) {
  return nJ == 4 && skip == 1 && Js[0] == 3 && Js[1] == 6 && Js[2] == 9 && Js[3] == 12;
}

static int momentum_multi(csm_ctx* ctx, const double* PM, int32_t T_m, int64_t N,
                          const int32_t* Js, int32_t nJ, int32_t skip, double* const* M,
                          double* const* NR, uint16_t* const* IDS) {
  int r = prep(ctx);
  if (r) return r;
  if (!PM || !Js || !M || !NR || N <= 0 || T_m < 0 || nJ < 1 || nJ > MJ_MAX || skip < 0)
    return set_err(ctx, CSM_E_INVAL, "csm_momentum_multi: bad arguments (N=%lld T_m=%d nJ=%d "
                   "skip=%d; 1 <= nJ <= %d)", (long long)N, T_m, nJ, skip, MJ_MAX);
  MJSet mj;
  int Jmax = 0;
  for (int q = 0; q < MJ_MAX; ++q) {
    mj.J[q] = q < nJ ? Js[q] : 1;
    mj.M[q] = q < nJ ? M[q] : nullptr;
    mj.NR[q] = q < nJ ? NR[q] : nullptr;
    mj.IDS[q] = (q < nJ && IDS) ? IDS[q] : nullptr;
    if (q < nJ && IDS && !IDS[q])
      return set_err(ctx, CSM_E_INVAL, "csm_momentum_multi_ids: ids[%d] is NULL", q);
    if (q < nJ && (Js[q] < 1 || !M[q] || !NR[q]))
      return set_err(ctx, CSM_E_INVAL, "csm_momentum_multi: J[%d]=%d or its outputs invalid", q,
                     q < nJ ? Js[q] : 0);
    if (q < nJ && Js[q] > Jmax) Jmax = Js[q];
  }
  const int W = Jmax + skip;
  if (W > 64)
    return set_err(ctx, CSM_E_INVAL, "csm_momentum_multi: max(J) + skip = %d > 64", W);
  if (T_m == 0) return CSM_OK;
  const int tpb = SCAN_THREADS;
  const unsigned blocks = (unsigned)((N + tpb - 1) / tpb);
  bool al = (N % 2) == 0 && aligned16(PM);
  for (int q = 0; q < nJ; ++q)
    al = al && aligned16(M[q]) && aligned16(NR[q]) && (!IDS || ((uintptr_t)IDS[q] & 3u) == 0);
  if (W <= MJ_REG_W && g_tune_mj_reg == 2 && al) {   // register shift ring, two assets per lane
    if (mj_fixed_grid(Js, nJ, skip))
      hipLaunchKernelGGL((k_momentum_multi_reg2<13, false, true>), dim3((unsigned)((N / 2 + tpb - 1) / tpb)),
                         dim3(tpb), 0, ctx->stream, PM, T_m, N, nJ, skip, mj, 1,
                         (const double*)nullptr, (const double*)nullptr, (const double*)nullptr);
    else
      hipLaunchKernelGGL(k_momentum_multi_reg2<MJ_REG_W>, dim3((unsigned)((N / 2 + tpb - 1) / tpb)),
                         dim3(tpb), 0, ctx->stream, PM, T_m, N, nJ, skip, mj, 1,
                         (const double*)nullptr, (const double*)nullptr, (const double*)nullptr);
    LAUNCH_CHECK(ctx, "k_momentum_multi_reg2");
    return CSM_OK;
  }
  if (W <= MJ_REG_W && g_tune_mj_reg) {   // register shift ring
    hipLaunchKernelGGL(k_momentum_multi_reg<MJ_REG_W>, dim3(blocks), dim3(tpb), 0, ctx->stream,
                       PM, T_m, N, nJ, skip, mj);
    LAUNCH_CHECK(ctx, "k_momentum_multi_reg");
    return CSM_OK;
  }
  const size_t lds = (size_t)W * tpb * sizeof(double);   // <= 64 KiB
  hipLaunchKernelGGL(k_momentum_multi, dim3(blocks), dim3(tpb), lds, ctx->stream, PM, T_m, N,
                     nJ, skip, W, mj);
  LAUNCH_CHECK(ctx, "k_momentum_multi");
  return CSM_OK;
}

int csm_momentum_multi(csm_ctx* ctx, const double* PM, int32_t T_m, int64_t N,
                       const int32_t* Js, int32_t nJ, int32_t skip, double* const* M,
                       double* const* NR) {
  return momentum_multi(ctx, PM, T_m, N, Js, nJ, skip, M, NR, nullptr);
}

int csm_momentum_multi_ids(csm_ctx* ctx, const double* PM, int32_t T_m, int64_t N,
                           const int32_t* Js, int32_t nJ, int32_t skip, double* const* M,
                           double* const* NR, uint16_t* const* IDS) {
  if (!IDS) return set_err(ctx, CSM_E_INVAL, "csm_momentum_multi_ids: ids is NULL");
  return momentum_multi(ctx, PM, T_m, N, Js, nJ, skip, M, NR, IDS);
}

int64_t csm_momentum_chunked_workspace(int32_t T_m, int64_t N, int32_t J, int32_t skip,
                                       int32_t C) {
  if (N <= 0 || C < 1 || J < 1 || skip < 0) return 0;
  const int64_t S = SUM_SCALARS + J + skip + 1, W = J + skip;
  (void)T_m;
  return (int64_t)C * (S + (W + 2) + 1) * N * (int64_t)sizeof(double);
}

static int momentum_chunked(csm_ctx* ctx, const double* PM, int32_t T_m, int64_t N, int32_t J,
                            int32_t skip, int32_t C, double* R, double* M, double* NR,
                            const double* next_pm, void* workspace, uint16_t* IDS) {
  int r = prep(ctx);
  if (r) return r;
  if (!PM || !M || !NR || !workspace || N <= 0 || T_m < 0 || J < 1 || skip < 0 ||
      J + skip > 256 || C < 1 || C > 65535)
    return set_err(ctx, CSM_E_INVAL, "csm_momentum_chunked: bad arguments (N=%lld T_m=%d C=%d)",
                   (long long)N, T_m, C);
  if (T_m == 0) return CSM_OK;
  if (C > T_m) C = T_m;
  const int W = J + skip, T = W + 1, S = SUM_SCALARS + T;
  double* sm = (double*)workspace;
  double* carry = sm + (int64_t)C * S * N;
  double* npm = carry + (int64_t)C * (W + 2) * N;
  launch_shard_summary_chunked(ctx->stream, PM, T_m, N, T, C, sm);
  LAUNCH_CHECK(ctx, "k_shard_summary_chunked");
  launch_fold_carry(ctx->stream, sm, C, -1, N, J, skip, carry, npm, next_pm,
                    FoldJs{0, {0, 0, 0, 0}}, nullptr);
  LAUNCH_CHECK(ctx, "k_fold_carry");
  const int tpb = W <= 64 ? SCAN_THREADS : 64;
  const size_t lds = (size_t)W * tpb * sizeof(double);
  if (lds > 65536)
    HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k_momentum_chunked,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_momentum_chunked, dim3((unsigned)((N + tpb - 1) / tpb), C), dim3(tpb), lds,
                     ctx->stream, PM, T_m, C, N, J, skip, R, M, NR, (const double*)carry,
                     (const double*)npm, IDS);
  LAUNCH_CHECK(ctx, "k_momentum_chunked");
  return CSM_OK;
}

int csm_momentum_chunked(csm_ctx* ctx, const double* PM, int32_t T_m, int64_t N, int32_t J,
                         int32_t skip, int32_t C, double* R, double* M, double* NR,
                         const double* next_pm, void* workspace) {
  return momentum_chunked(ctx, PM, T_m, N, J, skip, C, R, M, NR, next_pm, workspace, nullptr);
}

int64_t csm_momentum_multi_chunked_workspace(int32_t T_m, int64_t N, int32_t Jmax, int32_t skip,
                                             int32_t C) {
  if (N <= 0 || C < 1 || Jmax < 1 || skip < 0) return 0;
  const int64_t W = Jmax + skip, S = SUM_SCALARS + W + 1;
  (void)T_m;
  return (int64_t)C * (S + (W + 2) + 1 + MJ_MAX) * N * (int64_t)sizeof(double);
}

int csm_momentum_multi_chunked(csm_ctx* ctx, const double* PM, int32_t T_m, int64_t N,
                               const int32_t* Js, int32_t nJ, int32_t skip, int32_t C,
                               double* const* M, double* const* NR, uint16_t* const* IDS,
                               void* workspace) {
  int r = prep(ctx);
  if (r) return r;
  if (!PM || !Js || !M || !NR || !workspace || N <= 0 || T_m < 0 || nJ < 1 || nJ > MJ_MAX ||
      skip < 0 || C < 1 || C > 65535)
    return set_err(ctx, CSM_E_INVAL, "csm_momentum_multi_chunked: bad arguments (N=%lld T_m=%d "
                   "nJ=%d C=%d; 1 <= nJ <= %d)", (long long)N, T_m, nJ, C, MJ_MAX);
  MJSet mj;
  FoldJs fj;
  fj.n = nJ;
  int Jmax = 0;
  bool al = (N % 2) == 0 && aligned16(PM) && aligned16(workspace);
  for (int q = 0; q < MJ_MAX; ++q) {
    const bool on = q < nJ;
    mj.J[q] = fj.J[q] = on ? Js[q] : 1;
    mj.M[q] = on ? M[q] : nullptr;
    mj.NR[q] = on ? NR[q] : nullptr;
    mj.IDS[q] = (on && IDS) ? IDS[q] : nullptr;
    if (on && (Js[q] < 1 || !M[q] || !NR[q] || (IDS && !IDS[q])))
      return set_err(ctx, CSM_E_INVAL, "csm_momentum_multi_chunked: J[%d]=%d or its outputs invalid",
                     q, on ? Js[q] : 0);
    if (on) {
      al = al && aligned16(M[q]) && aligned16(NR[q]) && (!IDS || ((uintptr_t)IDS[q] & 3u) == 0);
      Jmax = Js[q] > Jmax ? Js[q] : Jmax;
    }
  }
  const int W = Jmax + skip;
  if (W > MJ_REG_W || !al)
    return set_err(ctx, CSM_E_INVAL, "csm_momentum_multi_chunked: needs max(J) + skip <= %d, even N "
                   "and 16-B aligned PM / M / NR / workspace, 4-B aligned ids (W=%d N=%lld)",
                   MJ_REG_W, W, (long long)N);
  if (T_m == 0) return CSM_OK;
  if (C > T_m) C = T_m;
  const int T = W + 1, S = SUM_SCALARS + T;
  double* sm = (double*)workspace;
  double* carry = sm + (int64_t)C * S * N;
  double* npm = carry + (int64_t)C * (W + 2) * N;
  double* psq = npm + (int64_t)C * N;
  launch_shard_summary_chunked(ctx->stream, PM, T_m, N, T, C, sm);
  LAUNCH_CHECK(ctx, "k_shard_summary_chunked");
  launch_fold_carry(ctx->stream, sm, C, -1, N, Jmax, skip, carry, npm, nullptr, fj, psq);
  LAUNCH_CHECK(ctx, "k_fold_carry");
  const int tpb = SCAN_THREADS;
  const dim3 grid((unsigned)((N / 2 + tpb - 1) / tpb), (unsigned)C);
  if (mj_fixed_grid(Js, nJ, skip))
    hipLaunchKernelGGL((k_momentum_multi_reg2<13, true, true>), grid, dim3(tpb), 0, ctx->stream,
                       PM, T_m, N, nJ, skip, mj, C, (const double*)carry, (const double*)npm,
                       (const double*)psq);
  else
    hipLaunchKernelGGL((k_momentum_multi_reg2<MJ_REG_W, true>), grid, dim3(tpb), 0, ctx->stream,
                       PM, T_m, N, nJ, skip, mj, C, (const double*)carry, (const double*)npm,
                       (const double*)psq);
  LAUNCH_CHECK(ctx, "k_momentum_multi_reg2 (chunked)");
  return CSM_OK;
}

int csm_momentum_chunked_ids(csm_ctx* ctx, const double* PM, int32_t T_m, int64_t N, int32_t J,
                             int32_t skip, int32_t C, double* R, double* M, double* NR,
                             const double* next_pm, uint16_t* ids, void* workspace) {
  if (!ids || (N % 4) != 0 || ((uintptr_t)ids & 7u) != 0)
    return set_err(ctx, CSM_E_INVAL, "csm_momentum_chunked_ids: ids must be non-NULL and 8-B "
                   "aligned, N %% 4 == 0 (N=%lld)", (long long)N);
  return momentum_chunked(ctx, PM, T_m, N, J, skip, C, R, M, NR, next_pm, workspace, ids);
}

}  // extern "C"
