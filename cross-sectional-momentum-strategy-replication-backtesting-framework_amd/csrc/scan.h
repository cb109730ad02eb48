// scan.h -- the per-asset momentum scan's month step, stated once (oracle/csmom_oracle.py,
// momentum_scan) in pieces that the scan kernels of scans.hip, signal.hip, signal_tc.hip,
// shards.hip and sweep_boot.hip compose:
//   price_step            forward-fill + one-month return of a present row
//   lds_push / lds_prod   the J + skip ring of factors fl(1 + ret) in LDS
//   reg_push / reg_prod   the same ring as a register shift ring, oldest first
//   mj_window             one look-back's window of a longer register ring (multi-J scans)
//   rank_step             is the row ranked, and the pending ranked row's next_ret
//   scan_step_on          the whole step of one asset with its stores, on a given ring policy
//   pending_finish        the last pending row's next_ret at the end of a scan
//   store_pair / store_next_ret_pair   two adjacent assets' outputs as 16-B stores
//   scan_step / scan_step_pair / scan_step_reg   scan_step_on at its sites: the LDS ring, two
//                         adjacent assets with paired stores, the register ring
//   scan_shadow           the step's state transition alone, no output
// Every product runs oldest factor first, left to right, then - 1.0: every composition gives the
// same bits.  Absent rows (no step at all) and the output stores stay with the sites and with
// scan_step_on.
#pragma once
#include "csm_common.h"

// =====================================================================================
// Per-asset scan state (shared by k_momentum and k_signal).
// The J+skip ring of factors fl(1+ret) lives in LDS, slot-major with a per-lane column
// (stride RS doubles), so a wave's ring accesses are conflict-free.
// mom = (prod over the J oldest ring entries of fl(1+ret), left to right) - 1.
// =====================================================================================
struct ScanLane {
  double pff;   // last valid month price (features.py:44 grouped ffill)
  double psff;  // last valid price among ranked rows (run_demo.py:48 subset ffill)
  int head;     // index of the oldest ring entry
  int prev;     // month of the pending ranked row (its next_ret waits for the next row)
};

__device__ __forceinline__ void scan_init(ScanLane& s, double* ring, int RS, int W,
                                          const double* __restrict__ carry, int64_t N,
                                          int64_t a, bool live) {
  if (live && carry) {
    for (int k = 0; k < W; ++k) ring[k * RS] = carry[(int64_t)k * N + a];
    s.pff = carry[(int64_t)W * N + a];
    s.psff = carry[(int64_t)(W + 1) * N + a];
  } else {
    for (int k = 0; k < W; ++k) ring[k * RS] = qnan();
    s.pff = qnan();
    s.psff = qnan();
  }
  s.head = 0;
  s.prev = -1;
}

// Forward-fill: x, or the last valid value when x is NaN.
__device__ __forceinline__ double ffill(double x, double last) { return isnan_d(x) ? last : x; }

// Price step of a present row x (a price or NaN): forward-fills it from pff, returns the
// one-month return and leaves the filled price in pff.
__device__ __forceinline__ double price_step(double x, double& pff) {
  const double nx = ffill(x, pff);
  const double ret = nx / pff - 1.0;
  pff = nx;
  return ret;
}

// LDS ring: push overwrites the oldest entry and advances head.
__device__ __forceinline__ void lds_push(double* ring, int RS, int W, int& head, double fct) {
  ring[head * RS] = fct;
  head = (head + 1 == W) ? 0 : head + 1;
}

// Product of the J ring entries from slot idx on (wrapping at W), oldest first.
template <int JC = 0>   // JC > 0: J fixed at compile time (the product's ring reads unrolled)
__device__ __forceinline__ double lds_prod(const double* ring, int RS, int W, int J, int idx) {
  double acc = ring[idx * RS];
  if constexpr (JC > 0) {
    double f[JC];   // the ring reads all issued before the product
#pragma unroll
    for (int k = 1; k < JC; ++k) {
      idx = (idx + 1 == W) ? 0 : idx + 1;
      f[k] = ring[idx * RS];
    }
#pragma unroll
    for (int k = 1; k < JC; ++k) acc = acc * f[k];
  } else {
    for (int k = 1; k < J; ++k) {
      idx = (idx + 1 == W) ? 0 : idx + 1;
      acc = acc * ring[idx * RS];
    }
  }
  return acc;
}

// Register shift ring, oldest first (f[RW - 1] newest).  on = false leaves the ring as it is
// (the predicated kernels' absent rows: selects, not a branch).
template <int RW>
__device__ __forceinline__ void reg_push(double (&f)[RW], double fct, bool on = true) {
#pragma unroll
  for (int k = 0; k + 1 < RW; ++k) f[k] = on ? f[k + 1] : f[k];
  f[RW - 1] = on ? fct : f[RW - 1];
}

// Product of a register ring's J oldest factors (the ring holds exactly J + skip).
template <int RW>
__device__ __forceinline__ double reg_prod(const double (&f)[RW], int J) {
  double acc = f[0];
#pragma unroll
  for (int k = 1; k < RW; ++k)
    if (k < J) acc = acc * f[k];
  return acc;
}

// Window product of one look-back of a multi-J scan: slots [lo, hi) of an RW-slot register ring
// that holds max(J) + skip factors or more, with the slots outside the window predicated off.
// acc starts at 1.0 and 1.0 * x == x exactly, so the product is still oldest-first over the same
// factors: bit-identical to a ring of exactly J + skip.
// FIX: the default grid J = 3, 6, 9, 12 (in that order), skip 1, in a 13-slot ring with
// compile-time windows (J - 1 multiplies each, no predicated slots): the same oldest-first
// product, about half the code -- the predicated chunked kernel was 85 KB, past the instruction
// cache.
template <int RW, bool FIX>
__device__ __forceinline__ double mj_window(const double (&f)[RW], int q, int lo, int hi) {
  if constexpr (FIX) {
    constexpr int Jq[4] = {3, 6, 9, 12};
    double acc = 0.0;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      if (qq != q) continue;
      const int l = RW - Jq[qq] - 1;
      double a = f[l];
#pragma unroll
      for (int k = l + 1; k < RW - 1; ++k) a = a * f[k];
      acc = a;
    }
    return acc;
  }
  double acc = 1.0;
#pragma unroll
  for (int k = 0; k < RW; ++k) acc = (k >= lo && k < hi) ? acc * f[k] : acc;
  return acc;
}

// next_ret of a ranked row whose subset-forward-filled price is psff, given the next present
// row's subset-forward-filled price ps_new.
__device__ __forceinline__ double subset_ret(double ps_new, double psff) {
  return ps_new / psff - 1.0;
}

// Rank step of a present row x of month m with momentum mom, on one (psff, prev) pair.  The
// pending ranked row prev (if any) is settled first: settle(row, next_ret) with the return over
// the subset-forward-filled price.  Then the pair moves on: the row is ranked when mom is
// defined and becomes the pending one; else its own next_ret is NaN (returns true).
// settle is a callback, not a returned struct or out-parameters: the division stays under
// prev >= 0 and ahead of the update; with the value computed up front the one-wave
// k_signal<24,2,4,1,*> variants spill.
template <class Settle>
__device__ __forceinline__ bool rank_step(double x, double mom, int m, double& psff, int& prev,
                                          Settle settle) {
  const bool ranked = !isnan_d(mom);
  const double ps_new = ffill(x, psff);
  if (prev >= 0) settle(prev, subset_ret(ps_new, psff));
  if (ranked) {
    psff = ps_new;
    prev = m;
    return false;
  }
  prev = -1;
  return true;
}

// next_ret of the pending ranked row at the end of a scan: x is the next present month price
// (NaN: no valid price that month), or ABSENT when no later month is present.
__device__ __forceinline__ double pending_finish(double x, double psff) {
  return is_absent(x) ? qnan() : subset_ret(ffill(x, psff), psff);
}

__device__ __forceinline__ void scan_finish(ScanLane& s, double* ring, int RS, int W, int64_t N,
                                            int64_t a, double* __restrict__ NR,
                                            const double* __restrict__ next_pm,
                                            double* __restrict__ carry_out) {
  if (s.prev >= 0)
    NR[(int64_t)s.prev * N + a] = next_pm ? pending_finish(next_pm[a], s.psff) : qnan();
  if (carry_out) {
    int idx = s.head;
    for (int k = 0; k < W; ++k) {  // carry rows hold the ring's factors, oldest first
      carry_out[(int64_t)k * N + a] = ring[idx * RS];
      idx = (idx + 1 == W) ? 0 : idx + 1;
    }
    carry_out[(int64_t)W * N + a] = s.pff;
    carry_out[(int64_t)(W + 1) * N + a] = s.psff;
  }
}

// The LDS ring policy of one lane: push, then the product of the J oldest factors, - 1.
template <int JC = 0>   // JC > 0: J fixed at compile time (the product's ring reads unrolled)
__device__ __forceinline__ double lds_push_mom(ScanLane& s, double* ring, int RS, int W, int J,
                                               double fct) {
  lds_push(ring, RS, W, s.head, fct);
  return lds_prod<JC>(ring, RS, W, J, s.head) - 1.0;
}

// The whole month step of asset a with its stores: consumes month m's price x and returns mom
// (NaN when absent / undefined).  push_prod is the ring policy, a callable taking the new factor
// fl(1 + ret) and returning mom: lds_push_mom for the LDS ring, reg_push + reg_prod for the
// register ring.  An absent row changes no state and stores NaN in every output.
template <class Ring>
__device__ __forceinline__ double scan_step_on(ScanLane& s, double x, int m, int64_t N, int64_t a,
                                               double* __restrict__ R, double* __restrict__ M,
                                               double* __restrict__ NR, Ring push_prod) {
  const double NaN = qnan();
  const int64_t o = (int64_t)m * N + a;
  if (is_absent(x)) {
    if (R) R[o] = NaN;
    M[o] = NaN;
    NR[o] = NaN;
    return NaN;
  }
  const double ret = price_step(x, s.pff);
  const double mom = push_prod(1.0 + ret);
  if (rank_step(x, mom, m, s.psff, s.prev,
                [&](int row, double nr) { NR[(int64_t)row * N + a] = nr; }))
    NR[o] = NaN;
  if (R) R[o] = ret;
  M[o] = mom;
  return mom;
}

// Two adjacent assets' values of one row as one 16-B store (p 16-B aligned).
__device__ __forceinline__ void store_pair(double* p, double v0, double v1) {
  *reinterpret_cast<double2*>(p) = make_double2(v0, v1);
}

// next_ret of two adjacent assets a0, a0 + 1 (a0 even) after one month step, row stride N:
// the settled pending rows wp (-1: none) with values vp as one 16-B store when both assets
// settle the same row (the steady state), else split; the same for the NaN at this month's row
// (offset o) of the assets flagged in wc.  A wave issues half the store instructions.
__device__ __forceinline__ void store_next_ret_pair(double* __restrict__ NR, int64_t N,
                                                    int64_t a0, int64_t o, const int (&wp)[2],
                                                    const double (&vp)[2], const bool (&wc)[2]) {
  const double NaN = qnan();
  if (wp[0] >= 0 && wp[0] == wp[1]) {
    store_pair(NR + (int64_t)wp[0] * N + a0, vp[0], vp[1]);
  } else {
    if (wp[0] >= 0) NR[(int64_t)wp[0] * N + a0] = vp[0];
    if (wp[1] >= 0) NR[(int64_t)wp[1] * N + a0 + 1] = vp[1];
  }
  if (wc[0] && wc[1]) {
    store_pair(NR + o, NaN, NaN);
  } else {
    if (wc[0]) NR[o] = NaN;
    if (wc[1]) NR[o + 1] = NaN;
  }
}

// Month range of chunk g when T_m months are split into G contiguous chunks (earlier
// chunks take the remainder) -- the same split as distributed.month_partition.
__device__ __forceinline__ void chunk_range(int T_m, int G, int g, int& m0, int& m1) {
  const int base = T_m / G, rem = T_m % G;
  m0 = g * base + (g < rem ? g : rem);
  m1 = m0 + base + (g < rem ? 1 : 0);
}

// Auto chunk count of a kernel over (slice of assets) x (chunk of consecutive months) whose chunks
// pay for their start (a lead-in, a window's warm-up): about per_cu (slice, chunk) workgroups per
// CU, and no chunk shorter than three months.  per_cu is measured per kernel, at its caller.
static inline int auto_chunks(const csm_ctx* ctx, int64_t slices, int T_m, int per_cu) {
  const int64_t want = (int64_t)per_cu * (ctx->n_cu > 0 ? ctx->n_cu : 256);
  int64_t G = (want + slices - 1) / slices;
  const int64_t most = T_m / 3 > 0 ? T_m / 3 : 1;
  if (G > most) G = most;
  return (int)G;
}

// That kernel's grid: slices of per_slice assets x G chunks, G the tune value when it is >= 1,
// else auto_chunks at per_cu, clamped to T_m and to what grid.y takes.
static inline dim3 month_grid(const csm_ctx* ctx, int64_t N, int per_slice, int tune, int per_cu,
                              int T_m) {
  const int64_t slices = (N + per_slice - 1) / per_slice;
  int64_t G = tune > 0 ? tune : auto_chunks(ctx, slices, T_m, per_cu);
  if (G > T_m) G = T_m;
  if (G > 65535) G = 65535;   // (grid.y)
  return dim3((unsigned)slices, (unsigned)G);
}

// =====================================================================================
// The month step's sites with an LDS ring (shared by k_momentum and k_signal): scan_step_on
// with the LDS ring policy, and its form for two adjacent assets.
// =====================================================================================
template <int JC = 0>
__device__ __forceinline__ double scan_step(ScanLane& s, double x, int m, double* ring, int RS,
                                            int W, int J, int64_t N, int64_t a,
                                            double* __restrict__ R, double* __restrict__ M,
                                            double* __restrict__ NR) {
  return scan_step_on(s, x, m, N, a, R, M, NR,
                      [&](double fct) { return lds_push_mom<JC>(s, ring, RS, W, J, fct); });
}

// scan_step for two adjacent assets a0, a0 + 1 (a0 even) with their stores paired: mom_J
// (and ret_1m) as one 16-B store per row, next_ret as one 16-B store when both assets write
// the same row (the steady state), so a wave issues half the store instructions.  Same
// arithmetic in the same order as two scan_step calls: bit-identical outputs.
template <int JC = 0>
__device__ __forceinline__ void scan_step_pair(ScanLane (&s)[2], const double (&x)[2], int m,
                                               double* ring0, int RS, int W, int J, int64_t N,
                                               int64_t a0, double* __restrict__ R,
                                               double* __restrict__ M, double* __restrict__ NR,
                                               double (&mom)[2]) {
  const double NaN = qnan();
  double ret[2];
  int wp[2];          // next_ret row of the pending ranked row (-1: none)
  double vp[2];
  bool wc[2];         // NaN next_ret at row m
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    wp[c] = -1;
    vp[c] = NaN;
    if (is_absent(x[c])) {
      ret[c] = NaN; mom[c] = NaN; wc[c] = true;
      continue;
    }
    ret[c] = price_step(x[c], s[c].pff);
    mom[c] = lds_push_mom<JC>(s[c], ring0 + c, RS, W, J, 1.0 + ret[c]);
    // rank_step's update restated at the site (its arithmetic, ffill and subset_ret, is shared):
    // through any function form the 512-VGPR one-wave k_signal variants spill more than they do
    // with these statements inline
    const bool ranked = !isnan_d(mom[c]);
    const double ps_new = ffill(x[c], s[c].psff);
    if (s[c].prev >= 0) { wp[c] = s[c].prev; vp[c] = subset_ret(ps_new, s[c].psff); }
    if (ranked) {
      s[c].psff = ps_new;
      s[c].prev = m;
      wc[c] = false;
    } else {
      s[c].prev = -1;
      wc[c] = true;
    }
  }
  const int64_t o = (int64_t)m * N + a0;
  if (R) store_pair(R + o, ret[0], ret[1]);
  store_pair(M + o, mom[0], mom[1]);
  store_next_ret_pair(NR, N, a0, o, wp, vp, wc);
}

// scan_step without outputs (the state transition only): the step of a trajectory that is
// followed but not written, such as the speculative one (F) beside k_shard_repair's true one.
__device__ __forceinline__ void scan_shadow(ScanLane& s, double x, int m, double* ring, int RS,
                                            int W, int J) {
  if (is_absent(x)) return;
  const double ret = price_step(x, s.pff);
  const double mom = lds_push_mom(s, ring, RS, W, J, 1.0 + ret);
  rank_step(x, mom, m, s.psff, s.prev, [](int, double) {});
}

// A lane's row value of VEC adjacent assets (one double, or a double2 of a 16-B load) and its
// component k.
template <int VEC> struct RowT;
template <> struct RowT<1> { typedef double T; };
template <> struct RowT<2> { typedef double2 T; };
__device__ __forceinline__ double comp(double v, int) { return v; }
__device__ __forceinline__ double comp(double2 v, int k) { return k == 0 ? v.x : v.y; }

// scan_step with the ring in registers, oldest first (the same factors, product order and
// stores as scan_step's LDS ring).  JC > 0: J is the compile-time JC (the product's factor
// count folds: no per-factor select).
template <int WR, int JC = 0>
__device__ __forceinline__ double scan_step_reg(ScanLane& s, double x, int m, double (&fr)[WR],
                                                int J, int64_t N, int64_t a,
                                                double* __restrict__ R, double* __restrict__ M,
                                                double* __restrict__ NR) {
  return scan_step_on(s, x, m, N, a, R, M, NR, [&](double fct) {
    reg_push(fr, fct);
    return reg_prod(fr, JC > 0 ? JC : J) - 1.0;
  });
}
