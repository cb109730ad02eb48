// signal.hip -- the fused signal: month-end aggregation and momentum scan in one stream over the
// daily panel, so the month prices never go through HBM unless PM is asked for.  signal_launch
// picks the kernel; every csm_signal* entry point and csm_pipeline goes through it.
//
//   k_signal        every day row streamed: a wave reduces month m of its assets while the rows
//                   of the next months are in flight in register buffers, then steps the scan.
//                   Its variants: one-wave blocks or four barrier-free waves, the date-shard pass
//                   (SH: an end-state record instead of a carry) and the halo prologue (HALO).
//   k_signal_tail   the whole-panel pass on even N: a month's last day row alone, a walk back
//                   only where it holds no price; months in batches through LDS.
// With "signal_tail" 2 both are launched on wide panels and each wave samples the panel
// (tail_probe) to decide which of the two is the launch's kernel.
#include "csm_common.h"
#include "scan.h"
#include "shard.h"

// =====================================================================================
// Kernel AB (fused): month-end aggregation + scan in one stream over the daily panel, for
// large N.  One wave per block, two assets per lane (16-B row loads, 1 KiB per wave-
// instruction).  While month m is reduced and scanned, the MAXD day rows of months m+1..m+3
// are already in flight (four register buffers).  Months shorter than MAXD re-load their last
// row into the spare slots: those loads hit L1/L2 (no extra HBM bytes), keep the load count
// fixed so vmcnt waits stay counted, and do not change "last non-NaN" / "any present".
// The month prices never round-trip through HBM unless PM is requested.
// =====================================================================================
// VEC assets per lane (VEC = 2: 16-B row loads, 1 KiB per wave-instruction; VEC = 1: twice
// the waves, 8-B loads), NBUF month buffers (NBUF - 1 months in flight).
// P is row-major [T_d][N]: consecutive day rows of a wave are N * 8 B apart.
// BW > 1: BW waves cover 64 * VEC * BW adjacent assets and walk them independently (no
// barrier), so a CU's loads of a day row are one BW-KiB span.

// The launch-level choice of "signal_tail" 2.  Where the panel has few gaps k_signal_tail reads a
// fraction of k_signal's bytes; where a quarter of the cells have no price on the month's last
// day its walks move about the stream's bytes in dependent trips and k_signal is 4-10 % faster
// at C4's width.  Both kernels are launched, and every wave of both first
// samples the same cells -- the last day row of PROBE_M months spread over the calendar at 128
// columns spread over the panel, all loads in flight at once, cached after the first wave --
// so all reach the same answer without sharing anything: k_signal_tail is the launch's kernel
// where at most one sampled cell in PROBE_DEN holds no price, and the other kernel's waves
// return.  No host round trip, no device state, the same choice for the same panel.
#define PROBE_M 8
#define PROBE_DEN 8
__device__ __forceinline__ bool tail_probe(const double* __restrict__ P,
                                           const int64_t* __restrict__ month_start, int T_m,
                                           int64_t N, int64_t T_d) {
  static_assert(PROBE_M == 8, "the month spacing is a shift");
  const int lane = threadIdx.x & 63;
  const int64_t cs = N / 128;   // column spacing (probed launches have N >= SIGNAL_BWF_MIN_N)
  double x[PROBE_M][2];
  bool in[PROBE_M];
#pragma unroll
  for (int i = 0; i < PROBE_M; ++i) {
    const int m = (int)(((int64_t)(2 * i + 1) * T_m) >> 4);   // (/ (2 * PROBE_M))
    const int64_t d0 = month_start[m] < 0 ? 0 : month_start[m];
    const int64_t d1 = month_start[m + 1] < T_d ? month_start[m + 1] : T_d;
    in[i] = d1 > d0;   // wave-uniform
#pragma unroll
    for (int j = 0; j < 2; ++j)
      x[i][j] = in[i] ? P[(d1 - 1) * N + (2 * lane + j) * cs] : 0.0;
  }
  int gaps = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < PROBE_M; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      gaps += __popcll(__ballot(in[i] && !(x[i][j] == x[i][j])));
      tot += in[i] ? 64 : 0;
    }
  return gaps * PROBE_DEN <= tot;
}

// SH (speculative date shard): carry_out is instead a [5][N] end-state record -- present
// months of the shard, the pending ranked row (month index, -1 none), its subset-ffilled
// price, and the first / last present month (-1 none) -- for k_shard_summary_state and
// k_shard_repair.
// BL (VEC 2): day rows by raw buffer loads (see load_month).
// HALO (with SH, the halo date-shard pass): month_start holds ha.H halo months, the shard's
// T_m months and ha.F forward months; a prologue does k_halo_pm + k_shard_halo's work for the
// lane's assets -- the halo months' and forward months' prices (the month's last day row, a walk
// back where it holds no price), the scan state the halo leaves from an empty state, its flags
// (ha.flags) -- and the shard's scan continues from that state in the same registers / LDS ring,
// the forward price finishing the pending ranked row: the same state, so the same outputs, as
// k_shard_halo -> k_signal<SH> (csm_signal_shard_halo), without two launches and their
// dependent walks between them.
struct HaloArgs {
  int H, F, before, after;
  uint8_t* flags;
};
#define HALO_BATCH 8   // halo / forward months per prologue batch (LDS: [8][RS] prices + lists)
template <int MAXD, int VEC, int NBUF, int BW, bool SH, bool BL, int JC = 0, bool HALO = false>
__global__ __launch_bounds__(64 * BW) void k_signal(
    const double* __restrict__ P, const int64_t* __restrict__ month_start, int T_m, int64_t N,
    int J, int skip, double* __restrict__ PMo, double* __restrict__ R, double* __restrict__ M,
    double* __restrict__ NR, const double* __restrict__ carry, const double* __restrict__ next_pm,
    double* __restrict__ carry_out, int64_t T_d, uint16_t* __restrict__ IDS, HaloArgs ha,
    int probe) {
  static_assert(!HALO || (SH && VEC == 2), "the halo prologue: shard passes, paired lanes");
  // (launch-uniform: k_signal_tail is this panel's kernel)
  if (probe && tail_probe(P, month_start, T_m, N, T_d)) return;
  typedef typename RowT<VEC>::T VT;
  extern __shared__ __attribute__((aligned(16))) double ring_lds[];  // [W][64 * VEC * BW]
  const int W = J + skip;
  const int tid = threadIdx.x;
  const int64_t a0 = ((int64_t)blockIdx.x * 64 * BW + tid) * VEC;
  const bool live = a0 < N;
  const int RS = 64 * VEC * BW;
  ScanLane sl[VEC];
  // SH counters live in LDS after the ring ([3][RS] ints: present months, first, last present
  // month): the kernel already holds ~500 registers, and these are touched once per month
  int* shc = reinterpret_cast<int*>(ring_lds + W * RS);
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    scan_init(sl[k], ring_lds + VEC * tid + k, RS, W, HALO ? nullptr : carry, N, a0 + k, live);
    if (SH) {
      shc[VEC * tid + k] = 0;
      shc[RS + VEC * tid + k] = -1;
      shc[2 * RS + VEC * tid + k] = -1;
    }
  }
  double npmh[VEC];   // HALO: the forward price of each asset (csm_shard_halo's next_pm)
  if constexpr (HALO) {
    // Months in batches of HU: each lane loads its two assets' last day row of every month of
    // the batch (one 16-B load a month, all in flight); the cells whose last day holds no price
    // (a missing day, a listing, a delisting, an absent month) are listed per wave and walked
    // back by the wave's lanes in parallel, a cell per lane (halo_month_price); then each lane
    // scans its halo months from an empty state (k_shard_halo's scan_shadow) and takes the first
    // forward month with a row as the forward price.  LDS after the ring and the SH counters:
    // the batch's month prices [HU][RS] and each wave's list of cells to walk.
    constexpr int HU = HALO_BATCH;
    const int64_t* ms = month_start;
    const int H = ha.H, F = ha.F, HF = H + F;
    const int64_t as = live ? a0 : 0;
    const int lane = tid & 63, wv = tid >> 6;
    const int64_t aw = a0 - 2 * lane;   // the wave's first asset
    double* hpw = ring_lds + (size_t)W * RS + (size_t)(3 * RS) / 2;
    uint16_t* wl = reinterpret_cast<uint16_t*>(hpw + HU * RS) + wv * (HU * 128);
    int nh[VEC], fv[VEC], lv[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) { nh[c] = 0; fv[c] = -1; lv[c] = -1; npmh[c] = absent_val(); }
    for (int j0 = 0; j0 < HF; j0 += HU) {   // (block-uniform)
      double2 xl[HU];
#pragma unroll
      for (int u = 0; u < HU; ++u) {
        const int j = j0 + u;
        const int m = j < H ? j : j + T_m;   // halo month j, or forward month j - H
        xl[u] = make_double2(absent_val(), absent_val());
        if (j < HF) {
          const int64_t d0 = ms[m], d1 = ms[m + 1];
          if (d1 > d0) xl[u] = *reinterpret_cast<const double2*>(P + (d1 - 1) * N + as);
        }
      }
      int nit = 0;   // wave-uniform
#pragma unroll
      for (int u = 0; u < HU; ++u) {
        *reinterpret_cast<double2*>(hpw + u * RS + 2 * tid) = xl[u];
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
          const double x = comp(xl[u], c);
          const bool need = live && j0 + u < HF && !(x == x);
          const uint64_t mk = __ballot(need);
          if (need) wl[nit + lane_prefix(mk)] = (uint16_t)(u * 128 + 2 * lane + c);
          nit += __popcll(mk);
        }
      }
      __builtin_amdgcn_wave_barrier();
      // the walks, a cell per lane and two cells per lane at once: the month's day rows before
      // its last (known to hold no price) in one batch of loads per cell, all in flight
      for (int it0 = 0; it0 < nit; it0 += 128) {   // (wave-uniform)
        int item[2], u[2];
        int64_t d0[2], d1[2];
        double xs[2][HALO_WALK];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int it = it0 + 64 * h + lane;
          item[h] = it < nit ? (int)wl[it] : -1;
          u[h] = item[h] >> 7;
          const int j = j0 + (item[h] < 0 ? 0 : u[h]);
          const int m = j < H ? j : j + T_m;
          d0[h] = ms[m];
          d1[h] = ms[m + 1];
          const int64_t a = aw + (item[h] & 127);
#pragma unroll
          for (int k = 0; k < HALO_WALK; ++k) {
            const int64_t d = d1[h] - 2 - k;
            xs[h][k] = (item[h] >= 0 && d >= d0[h]) ? P[d * N + a] : absent_val();
          }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (item[h] < 0) continue;
          const int64_t a = aw + (item[h] & 127);
          const double xlast = hpw[u[h] * RS + 128 * wv + (item[h] & 127)];
          bool p = !is_absent(xlast), got = false;
          double x = 0.0;
#pragma unroll
          for (int k = 0; k < HALO_WALK; ++k) {
            if (!got && xs[h][k] == xs[h][k]) { x = xs[h][k]; got = true; }
            p |= !is_absent(xs[h][k]);
          }
          if (!got && d1[h] - 1 - HALO_WALK > d0[h]) {   // months longer than the batch (rare)
            const double y = halo_month_price(P, d0[h], d1[h] - 1 - HALO_WALK, N, a);
            if (y == y) { x = y; got = true; }
            p |= !is_absent(y);
          }
          hpw[u[h] * RS + 128 * wv + (item[h] & 127)] = got ? x : (p ? qnan() : absent_val());
        }
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < HU; ++u) {
        const int j = j0 + u;
        if (j >= HF) break;
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
          const double x = hpw[u * RS + 2 * tid + c];
          if (j < H) {
            if (live && !is_absent(x)) {
              if (!isnan_d(x)) { if (fv[c] < 0) fv[c] = nh[c]; lv[c] = nh[c]; }
              ++nh[c];
              scan_shadow(sl[c], x, j, ring_lds + VEC * tid + c, RS, W, J);
            }
          } else if (is_absent(npmh[c])) {
            npmh[c] = x;
          }
        }
      }
      __syncthreads();   // (the batch's LDS is the next batch's)
    }
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      sl[c].prev = -1;   // (the halo's pending row is the previous rank's: scan_init's state)
      uint8_t fl = 0;
      if (ha.before && !(fv[c] >= 0 && lv[c] - fv[c] >= W)) fl |= 1;
      if (ha.after && is_absent(npmh[c])) fl |= 2;
      if (live && ha.flags) ha.flags[a0 + c] = fl;
    }
    month_start += H;   // the shard's months from here on
  }
  const double* base = P + (live ? a0 : 0);
  const int64_t rstride = N;
  // Loads are issued unconditionally (months past the end re-load the last month: cache
  // hits) so every wait is a counted vmcnt; only the processing is guarded.
  // BL: raw buffer loads over a per-month resource that ends at the month's last day row, so
  // the padding loads past it are out of range: counted by vmcnt like any load, but they return
  // 0 without a memory request (process masks them by the wave-uniform row count).
  static_assert(!BL || VEC == 2, "buffer loads: paired lanes");
  const int voff = (int)((live ? a0 : 0) * 8);
  auto load_month = [&](VT (&buf)[MAXD], int mm) {
    mm = mm < T_m ? mm : T_m - 1;
    const int64_t f0 = month_start[mm], nn = month_start[mm + 1] - f0;
    if constexpr (BL) {
      typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(P + f0 * N), (short)0, (int)(nn * N * 8), 0x00020000);
#pragma unroll
      for (int k = 0; k < MAXD; ++k) {
        const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(rs, voff + k * (int)(N * 8), 0, 0);
        buf[k] = *reinterpret_cast<const VT*>(&w);
      }
    } else {
      // (a zero-length month re-loads a row of the panel too; process masks all of it)
      const int64_t pad = nn > 0 ? nn - 1 : (f0 > 0 ? -1 : 0);
#pragma unroll
      for (int k = 0; k < MAXD; ++k)
        buf[k] = *reinterpret_cast<const VT*>(base + (f0 + (k < nn ? k : pad)) * rstride);
    }
  };
  auto process = [&](const VT (&X)[MAXD], int m) {
    double pm[VEC];
    const int nnm = (int)(month_start[m + 1] - month_start[m]);
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      double last = 0.0;
      bool p = false, v = false;
#pragma unroll
      for (int k = 0; k < MAXD; ++k) {
        const double x = comp(X[k], c);
        const bool in = BL ? k < nnm : nnm > 0;   // wave-uniform (no row: a zero-length month)
        const bool ok = in && x == x;  // a valid price (ABSENT and missing are NaN)
        p |= in && !is_absent(x);
        v |= ok;
        last = ok ? x : last;
      }
      pm[c] = p ? (v ? last : qnan()) : absent_val();
      if (SH && p) {
        int* q = shc + VEC * tid + c;
        q[0] += 1;
        if (q[RS] < 0) q[RS] = m;
        q[2 * RS] = m;
      }
    }
    if (live) {
      if (PMo && (!SH || shard_pm_kept(m, T_m, W))) {
        if (VEC == 2) *reinterpret_cast<double2*>(PMo + (int64_t)m * N + a0) = make_double2(pm[0], pm[VEC - 1]);
        else PMo[(int64_t)m * N + a0] = pm[0];
      }
      double mom[VEC];
      if constexpr (VEC == 2) {   // paired 16-B stores (R / M / NR are 16-B aligned)
        scan_step_pair<JC>(reinterpret_cast<ScanLane (&)[2]>(sl), reinterpret_cast<const double (&)[2]>(pm),
                       m, ring_lds + VEC * tid, RS, W, J, N, a0, R, M, NR,
                       reinterpret_cast<double (&)[2]>(mom));
      } else {
#pragma unroll
        for (int c = 0; c < VEC; ++c)
          mom[c] = scan_step(sl[c], pm[c], m, ring_lds + VEC * tid + c, RS, W, J, N, a0 + c, R, M, NR);
      }
      if (IDS) {   // fixed-map bucket ids for the decile pass (csm_signal_ids)
        if (VEC == 2)
          *reinterpret_cast<uint32_t*>(IDS + (int64_t)m * N + a0) =
              csm_fid(mom[0]) | (csm_fid(mom[VEC - 1]) << 16);
        else
          IDS[(int64_t)m * N + a0] = (uint16_t)csm_fid(mom[0]);
      }
    }
  };
  static_assert(NBUF == 2 || NBUF == 4, "two or four month buffers");
  VT A[MAXD], B[MAXD];
  if (NBUF == 2) {
    // month m+1 in flight while month m is reduced (half the registers: two waves per SIMD)
    load_month(A, 0);
    for (int m = 0; m < T_m; m += 2) {
      load_month(B, m + 1);
      process(A, m);
      load_month(A, m + 2);
      if (m + 1 < T_m) process(B, m + 1);
    }
  } else {
    // months m+1..m+3 in flight (the whole-history-per-wave pattern needs ~3 months in
    // flight to approach the row-stream rate, see scripts/mb)
    VT C[MAXD], D[MAXD];
    load_month(A, 0);
    load_month(B, 1);
    load_month(C, 2);
    for (int m = 0; m < T_m; m += 4) {
      load_month(D, m + 3);
      process(A, m);
      load_month(A, m + 4);
      if (m + 1 < T_m) process(B, m + 1);
      load_month(B, m + 5);
      if (m + 2 < T_m) process(C, m + 2);
      load_month(C, m + 6);
      if (m + 3 < T_m) process(D, m + 3);
    }
  }
  if (live) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if constexpr (HALO) {   // scan_finish's pending row, with the prologue's forward price
        if (sl[k].prev >= 0)
          NR[(int64_t)sl[k].prev * N + a0 + k] = pending_finish(npmh[k], sl[k].psff);
      } else {
        scan_finish(sl[k], ring_lds + VEC * tid + k, RS, W, N, a0 + k, NR, next_pm,
                    SH ? nullptr : carry_out);
      }
      if (SH) {
        const int* q = shc + VEC * tid + k;
        carry_out[a0 + k] = (double)q[0];
        carry_out[N + a0 + k] = (double)sl[k].prev;
        carry_out[2 * N + a0 + k] = sl[k].psff;
        carry_out[3 * N + a0 + k] = (double)q[RS];
        carry_out[4 * N + a0 + k] = (double)q[2 * RS];
      }
    }
  }
}

// =====================================================================================
// Kernel AB, tail first (the one-GPU default for even N): the month-end needs the month's last
// valid price and whether any row is present, so a cell whose LAST day row holds a price needs
// no other row.  Months in batches of TAIL_U; a lane loads its asset's last day row of every
// month of the batch (one coalesced load a month, the next batch's already in flight), the
// cells whose last row holds no price (a missing day, a listing, a delisting, an absent month)
// are listed per wave in LDS and walked back by the wave's lanes, a cell per lane, in two lists.
// A missing day (a NaN that is not ABSENT) loads TAIL_BACK rows before the last and almost
// always finds its price there.  ABSENT in the last row (a listing, a delisting, an absent
// month) is almost always a month without a price, which needs every row, so the cell loads
// them all at once, two cells per lane and trip where the list is long; the rare missing day
// still open after TAIL_BACK rows joins that list.  The first trips of both lists are in flight
// together.  Then the batch's month prices are scanned from LDS.  The lists are in (month,
// column) order, so where gaps are dense neighbouring lanes walk neighbouring columns of the
// same rows and their requests coalesce.
// One asset per lane: the scan is a chain of dependent LDS reads and FP64 products that nothing
// hides once the row stream is gone, and paired lanes (k_signal's layout) give C4 782 waves for
// 1,024 SIMDs; single lanes give twice the waves (paired: 25-60 % slower).
// Same ring, same arithmetic as k_signal's one-asset-per-lane form: bit-identical PM / R / M /
// NR / ids.  Every wave works alone on its 64 assets (no block barrier, no global state).
// =====================================================================================
#define TAIL_U 8        // months per batch
#define TAIL_BACK 3     // day rows before the last that a cell with a missing last day loads first

template <int MAXD, int BW, int JC>
__global__ __launch_bounds__(64 * BW) void k_signal_tail(
    const double* __restrict__ P, const int64_t* __restrict__ month_start, int T_m, int64_t N,
    int J, int skip, double* __restrict__ PMo, double* __restrict__ R, double* __restrict__ M,
    double* __restrict__ NR, const double* __restrict__ carry, const double* __restrict__ next_pm,
    double* __restrict__ carry_out, int64_t T_d, uint16_t* __restrict__ IDS,
    int probe) {
  // (launch-uniform: k_signal is this panel's kernel)
  if (probe && !tail_probe(P, month_start, T_m, N, T_d)) return;
  // LDS: the ring [W][RS], the batch's month prices [TAIL_U][RS], each wave's two lists of cells
  extern __shared__ __attribute__((aligned(16))) double ring_lds[];
  constexpr int U = TAIL_U, RS = 64 * BW, WA = 64;
  const int W = J + skip;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t a0 = (int64_t)blockIdx.x * RS + tid;
  const bool live = a0 < N;
  const int64_t as = live ? a0 : 0;
  const int64_t aw = a0 - lane;         // the wave's first asset
  const int64_t* ms = month_start;
  double* hp = ring_lds + (size_t)W * RS;
  double* hpw = hp + WA * wv;           // the wave's columns of a month row
  uint16_t* wl = reinterpret_cast<uint16_t*>(hp + U * RS) + wv * (2 * U * WA);
  uint16_t* wl2 = wl + U * WA;          // wl: missing last days; wl2: absent last rows
  ScanLane sl;
  scan_init(sl, ring_lds + tid, RS, W, carry, N, a0, live);
  if (aw >= N) return;   // (wave-uniform; no wave waits for another)

  // day rows [d0, d1) of month m, inside the panel
  auto month_rows = [&](int m, int64_t& d0, int64_t& d1) {
    d0 = ms[m];
    d1 = ms[m + 1];
    d0 = d0 < 0 ? 0 : d0;
    d1 = d1 < T_d ? d1 : T_d;
  };
  auto load_last = [&](double (&xl)[U], int m0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      xl[u] = absent_val();
      if (m0 + u < T_m) {   // (block-uniform)
        int64_t d0, d1;
        month_rows(m0 + u, d0, d1);
        if (d1 > d0) xl[u] = P[(d1 - 1) * N + as];
      }
    }
  };
  // one more row of a listed cell, walking back: the latest valid price, and presence
  auto fold = [&](double y, double& x, bool& got, bool& p) {
    if (!got && y == y) { x = y; got = true; }
    p |= !is_absent(y);
  };
  // A trip of a walk: 64 listed cells, a cell per lane.  issue() puts the cell's KK rows before
  // its last in flight, finish_*() folds them into the month price.
  constexpr int K = MAXD - 1;
  struct Walk {
    int item, u, col;
    int64_t d0, d1;
    bool act;
  };
  auto issue = [&](auto& xs, Walk& w, const uint16_t* list, int it, int n, int m0) {
    constexpr int KK = sizeof(xs) / sizeof(double);
    w.act = it < n;
    w.item = w.act ? (int)list[it] : 0;
    w.u = w.item / WA;     // the batch's month
    w.col = w.item % WA;   // the wave's column
    month_rows(m0 + w.u, w.d0, w.d1);
    const int64_t a = aw + w.col;
#pragma unroll
    for (int k = 0; k < KK; ++k) {
      const int64_t d = w.d1 - 2 - k;
      xs[k] = (w.act && d >= w.d0) ? P[d * N + a] : absent_val();
    }
  };
  // a missing last day: the price TAIL_BACK rows back, or on to the list of whole months
  auto finish_back = [&](const double (&xs)[TAIL_BACK], const Walk& w, int& nb) {
    bool p = true, got = false;   // (a last row that is not ABSENT is a present row)
    double x = 0.0;
#pragma unroll
    for (int k = 0; k < TAIL_BACK; ++k) fold(xs[k], x, got, p);
    const bool more = w.act && !got && w.d1 - 2 - TAIL_BACK >= w.d0;
    if (w.act && !more) hpw[w.u * RS + w.col] = got ? x : qnan();
    const uint64_t mk = __ballot(more);
    if (more) wl2[nb + lane_prefix(mk)] = (uint16_t)w.item;
    nb += __popcll(mk);
  };
  auto finish_month = [&](const double (&xs)[K], const Walk& w) {
    bool p = !is_absent(hpw[w.u * RS + w.col]), got = false;
    double x = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) fold(xs[k], x, got, p);
    if (w.act) hpw[w.u * RS + w.col] = got ? x : (p ? qnan() : absent_val());
  };
  // up to 128 cells of the whole-month list from index i0: both halves' rows in flight at once
  auto walk_months = [&](int i0, int n, int m0) {
    double XS[K], XT[K];
    Walk wb, wc;
    const bool two = i0 + 64 < n;   // wave-uniform
    issue(XS, wb, wl2, i0 + lane, n, m0);
    if (two) issue(XT, wc, wl2, i0 + 64 + lane, n, m0);
    finish_month(XS, wb);
    if (two) finish_month(XT, wc);
  };

  double xa[U], xb[U];
  load_last(xa, 0);
  for (int m0 = 0; m0 < T_m; m0 += U) {
    load_last(xb, m0 + U);
    int na = 0, nb = 0;   // wave-uniform: the listed missing days, the listed absent last rows
    // ---- the batch's last rows into LDS, the cells without a price listed ----
#pragma unroll
    for (int u = 0; u < U; ++u) {
      hp[u * RS + tid] = xa[u];
      bool in = false;
      if (m0 + u < T_m) {
        int64_t d0, d1;
        month_rows(m0 + u, d0, d1);
        in = d1 > d0;   // (a zero-length month is ABSENT: nothing to walk)
      }
      const double x = xa[u];
      const bool need = live && in && !(x == x);
      const bool nb_ = need && is_absent(x), na_ = need && !nb_;
      const uint64_t mka = __ballot(na_), mkb = __ballot(nb_);
      const int item = u * WA + lane;
      if (na_) wl[na + lane_prefix(mka)] = (uint16_t)item;
      if (nb_) wl2[nb + lane_prefix(mkb)] = (uint16_t)item;
      na += __popcll(mka);
      nb += __popcll(mkb);
    }
    __builtin_amdgcn_wave_barrier();
    // ---- the walks, a cell per lane ----
    if (na + nb > 0) {
      double xs[TAIL_BACK];
      Walk wa;
      int db = nb < 128 ? nb : 128;   // whole months walked so far (the back walks append more)
      issue(xs, wa, wl, lane, na, m0);
      walk_months(0, db, m0);
      finish_back(xs, wa, nb);
      for (int it0 = 64; it0 < na; it0 += 64) {
        issue(xs, wa, wl, it0 + lane, na, m0);
        finish_back(xs, wa, nb);
      }
      __builtin_amdgcn_wave_barrier();
      for (; db < nb; db += 128) walk_months(db, nb, m0);
    }
    __builtin_amdgcn_wave_barrier();
    // ---- the scan of the batch's month prices (k_signal's process() from pm on) ----
#pragma unroll 1
    for (int u = 0; u < U; ++u) {
      const int m = m0 + u;
      if (m >= T_m) break;
      if (!live) continue;
      const double pm = hp[u * RS + tid];   // (the walks wrote the canonical NaN / ABSENT)
      if (PMo) PMo[(int64_t)m * N + a0] = pm;
      const double mom = scan_step<JC>(sl, pm, m, ring_lds + tid, RS, W, J, N, a0, R, M, NR);
      if (IDS) IDS[(int64_t)m * N + a0] = (uint16_t)csm_fid(mom);
    }
    __builtin_amdgcn_wave_barrier();   // (the batch's LDS is the next batch's)
#pragma unroll
    for (int u = 0; u < U; ++u) xa[u] = xb[u];
  }
  if (live) scan_finish(sl, ring_lds + tid, RS, W, N, a0, NR, next_pm, carry_out);
}

static int g_tune_signal_vec = 2;      // k_signal assets per lane: 2 (paired 16-B rows) | 1 (odd N)
static int g_tune_signal_bwf = 0;      // k_signal blocks: 0 auto | 1 one wave | 4 four barrier-free waves x 2 month buffers (buffer loads)
// the one-GPU fused signal (even N, aligned buffers): 0 k_signal, every day row streamed | 1
// k_signal_tail, last day rows and walks | 2 (auto) k_signal_tail below SIGNAL_BWF_MIN_N assets;
// from there on both are launched and each samples the panel's last day rows (tail_probe):
// k_signal_tail runs where at most 1 sampled cell in 8 holds no price, k_signal elsewhere
static int g_tune_signal_tail = 2;
static int g_tune_signal_j12 = 1;      // wide shard k_signal: J = 12 with its product length fixed at compile time (0: runtime J)
#define SIGNAL_BWF_MIN_N (180 * 512)   // auto: 4-wave blocks once the grid still covers >= 180 CUs
static const TuneKnob g_knobs[] = {
    {"signal_vec", &g_tune_signal_vec, [](int v) { return v == 1 || v == 2; }},
    {"signal_bwf", &g_tune_signal_bwf, [](int v) { return v == 0 || v == 1 || v == 4; }},
    {"signal_j12", &g_tune_signal_j12, [](int v) { return v == 0 || v == 1; }},
    {"signal_tail", &g_tune_signal_tail, [](int v) { return v >= 0 && v <= 2; }},
};
int csm_tune_signal(const char* key, int value) { return tune_set(g_knobs, key, value); }

int signal_launch(csm_ctx* ctx, const char* who, const double* P, int64_t T_d, int64_t N,
                  const int64_t* month_start, int32_t T_m, int32_t max_month_days, int32_t J,
                  int32_t skip, double* PM, double* R, double* M, double* NR, const double* carry,
                  const double* next_pm, double* carry_out, bool sh, uint16_t* ids,
                  const HaloArgs* halo) {
  int r = prep(ctx);
  if (r) return r;
  // (a shard pass starts from an empty state, or -- the halo pass -- from the halo's carry
  // and forward price)
  if (sh && (!PM || !carry_out || T_m < 1))
    return set_err(ctx, CSM_E_INVAL, "%s: a shard pass needs PM and state, and at least one month",
                   who);
  if (!P || !month_start || !M || !NR || N <= 0 || T_d < 0 || T_m < 0 || J < 1 || skip < 0 ||
      J + skip > 256 || max_month_days < 1)
    return set_err(ctx, CSM_E_INVAL, "%s: bad arguments (N=%lld T_m=%d J=%d skip=%d)", who,
                   (long long)N, T_m, J, skip);
  if (max_month_days > 32)
    return set_err(ctx, CSM_E_INVAL, "%s: months longer than 32 days are not supported "
                   "(use csm_month_end + csm_momentum)", who);
  if (T_m == 0) return CSM_OK;
  if (T_d == 0)
    return set_err(ctx, CSM_E_INVAL, "%s: %d months and no day row", who, T_m);
  const int W = J + skip;
  const bool can2 = (N % 2 == 0) && aligned16(P) && (!PM || aligned16(PM)) && aligned16(M) &&
                    aligned16(NR) && (!R || aligned16(R));
  const int vec = (g_tune_signal_vec == 1 || !can2) ? 1 : 2;
  // Tail first (k_signal_tail): the whole-panel pass on even N and aligned buffers, two
  // independent waves of 64 assets per block; ring, batch and lists in LDS (the CU's 160 KiB
  // bound J + skip).  J = 12 with its product length fixed at compile time: the scan's chain
  // is this kernel's critical path.  signal_tail 2: both kernels launched, tail_probe's choice
  // made by each.
  const size_t tlds = (size_t)(W + TAIL_U) * 128 * sizeof(double) + (size_t)2 * TAIL_U * 128 * sizeof(uint16_t);
  // (auto below SIGNAL_BWF_MIN_N: k_signal is one wave per 128 assets there, its time set by the
  // 461-month chain whatever N, and k_signal_tail measured 0.55-0.65 x even on the gap-heavy
  // panel at 32,768 and 65,536 assets: no probe)
  int tail = (!sh && !halo && can2 && tlds <= 160 * 1024) ? g_tune_signal_tail : 0;
  if (tail == 2 && N < (int64_t)SIGNAL_BWF_MIN_N) tail = 1;
  int probe_ = tail == 2;
  if (tail != 0) {
    const bool d23 = max_month_days <= 23, j12 = J == 12;
    const void* fn =
        d23 ? (j12 ? (const void*)k_signal_tail<23, 2, 12> : (const void*)k_signal_tail<23, 2, 0>)
            : (j12 ? (const void*)k_signal_tail<32, 2, 12> : (const void*)k_signal_tail<32, 2, 0>);
    if (tlds > 65536)
      HIP_CHECK(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tlds));
    const unsigned blocks = (unsigned)((N + 127) / 128);
    int T_m_ = T_m, J_ = J, skip_ = skip;
    int64_t N_ = N, T_d_ = T_d;
    void* args[] = {(void*)&P, (void*)&month_start, &T_m_, &N_, &J_, &skip_, (void*)&PM, (void*)&R,
                    (void*)&M, (void*)&NR, (void*)&carry, (void*)&next_pm, (void*)&carry_out, &T_d_,
                    (void*)&ids, &probe_};
    HIP_CHECK(ctx, hipLaunchKernel(fn, dim3(blocks), dim3(128), args, tlds, ctx->stream));
    LAUNCH_CHECK(ctx, who);
    if (tail == 1) return CSM_OK;
  }
  // Barrier-free 4-wave blocks (adjacent 1-KiB column slices walked independently, 2 month
  // buffers, raw buffer loads with the padding rows out of range): the wide-panel default
  // (C4 1.75-1.85 -> 1.63-1.78 ms, then buffer loads 1.695 -> 1.674, profiles/r02/experiments).
  // Rows of at most 2 GiB / 32 (buffer offsets), months of at most 23 days.
  const bool fits4 = vec == 2 && max_month_days <= 23 && N * 8 * 32 < ((int64_t)1 << 31);
  const bool wide4 = fits4 && (g_tune_signal_bwf == 4 ||
                               (g_tune_signal_bwf == 0 && N >= (int64_t)SIGNAL_BWF_MIN_N));
  const int bw = wide4 ? 4 : 1;
  const size_t lds = (size_t)W * 64 * vec * bw * sizeof(double) +
                     (sh ? (size_t)3 * 64 * vec * bw * sizeof(int) : 0) +
                     (halo ? (size_t)HALO_BATCH * 64 * vec * bw * sizeof(double) +
                             (size_t)bw * HALO_BATCH * 128 * sizeof(uint16_t) : 0);
  const unsigned blocks = (unsigned)((N / vec + 64 * bw - 1) / (64 * bw));
  const void* fn = nullptr;
  // one-wave blocks, four month buffers: 23 / 24 / 32 day rows (the longest month)
#define SIG1(V, SH_)                                                                            \
  (max_month_days <= 23 && V == 2 ? (const void*)k_signal<23, V, 4, 1, SH_, false>              \
   : max_month_days <= 24         ? (const void*)k_signal<24, V, 4, 1, SH_, false>              \
                                  : (const void*)k_signal<32, V, 4, 1, SH_, false>)
  // date shards: the default look-back J = 12 with its product length fixed at compile time
  // (8-way halo rank: shard kernel 0.237 -> 0.231 ms; the full C4 pass measured 0.3 % slower
  // with it, so the one-GPU kernel keeps the runtime J)
  const bool j12 = sh && J == 12 && g_tune_signal_j12;
  if (halo && !(sh && wide4))
    return set_err(ctx, CSM_E_INVAL, "%s: the fused halo prologue runs in the wide shard kernel "
                   "(even N >= %d, months of <= 23 days); use csm_shard_halo + "
                   "csm_signal_shard_halo", who, SIGNAL_BWF_MIN_N);
  if (halo)
    fn = j12 ? (const void*)k_signal<23, 2, 2, 4, true, true, 12, true>
             : (const void*)k_signal<23, 2, 2, 4, true, true, 0, true>;
  else if (wide4 && j12)
    fn = (const void*)k_signal<23, 2, 2, 4, true, true, 12>;
  else if (wide4)
    fn = sh ? (const void*)k_signal<23, 2, 2, 4, true, true> : (const void*)k_signal<23, 2, 2, 4, false, true>;
  else if (vec == 2)
    fn = sh ? SIG1(2, true) : SIG1(2, false);
  else
    fn = sh ? SIG1(1, true) : SIG1(1, false);
#undef SIG1
  if (lds > 65536)
    HIP_CHECK(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  {
    int T_m_ = T_m, J_ = J, skip_ = skip;
    int64_t N_ = N, T_d_ = T_d;
    HaloArgs ha = halo ? *halo : HaloArgs{0, 0, 0, 0, nullptr};
    void* args[] = {(void*)&P, (void*)&month_start, &T_m_, &N_, &J_, &skip_, (void*)&PM, (void*)&R,
                    (void*)&M, (void*)&NR, (void*)&carry, (void*)&next_pm, (void*)&carry_out, &T_d_,
                    (void*)&ids, (void*)&ha, &probe_};
    HIP_CHECK(ctx, hipLaunchKernel(fn, dim3(blocks), dim3(64 * bw), args, lds, ctx->stream));
  }
  LAUNCH_CHECK(ctx, who);
  return CSM_OK;
}

extern "C" {

int csm_signal(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N, const int64_t* month_start,
               int32_t T_m, int32_t max_month_days, int32_t J, int32_t skip, double* PM, double* R,
               double* M, double* NR, const double* carry, const double* next_pm,
               double* carry_out) {
  return signal_launch(ctx, "csm_signal", P, T_d, N, month_start, T_m, max_month_days, J,
                       skip, PM, R, M, NR, carry, next_pm, carry_out);
}

int csm_signal_ids(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N,
                   const int64_t* month_start, int32_t T_m, int32_t max_month_days,
                   int32_t min_month_days, int32_t J, int32_t skip, double* PM, double* R,
                   double* M, double* NR, uint16_t* ids) {
  if (!ids || (N % 4) != 0 || ((uintptr_t)ids & 7u) != 0)
    return set_err(ctx, CSM_E_INVAL, "csm_signal_ids: ids must be non-NULL and 8-B aligned, N %% 4 == 0 "
                   "(N=%lld)", (long long)N);
  (void)min_month_days;   // kept in the ABI (host hint for fixed day batches; no kernel uses it)
  return signal_launch(ctx, "csm_signal_ids", P, T_d, N, month_start, T_m, max_month_days, J,
                       skip, PM, R, M, NR, nullptr, nullptr, nullptr, false, ids);
}

int csm_signal_shard(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N,
                     const int64_t* month_start, int32_t T_m, int32_t max_month_days, int32_t J,
                     int32_t skip, double* PM, double* R, double* M, double* NR, double* state) {
  return signal_launch(ctx, "csm_signal_shard", P, T_d, N, month_start, T_m,
                       max_month_days, J, skip, PM, R, M, NR, nullptr, nullptr, state, true);
}

int csm_signal_shard_ids(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N,
                         const int64_t* month_start, int32_t T_m, int32_t max_month_days,
                         int32_t J, int32_t skip, double* PM, double* R, double* M, double* NR,
                         double* state, uint16_t* ids) {
  if (!ids || (N % 4) != 0 || ((uintptr_t)ids & 7u) != 0)
    return set_err(ctx, CSM_E_INVAL, "csm_signal_shard_ids: needs ids, N %% 4 == 0, 8-B aligned ids");
  return signal_launch(ctx, "csm_signal_shard_ids", P, T_d, N, month_start, T_m,
                       max_month_days, J, skip, PM, R, M, NR, nullptr, nullptr, state, true, ids);
}

int csm_signal_halo(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N,
                    const int64_t* month_start, int32_t H, int32_t T_m, int32_t F, int32_t before,
                    int32_t after, int32_t max_month_days, int32_t J, int32_t skip, double* PM,
                    double* R, double* M, double* NR, double* state, uint16_t* ids,
                    uint8_t* flags) {
  if (!flags || H < 0 || F < 0 || F > 8 || J + skip > 64)
    return set_err(ctx, CSM_E_INVAL, "csm_signal_halo: bad arguments (flags [N], H >= 0, "
                   "0 <= F <= 8, J + skip <= 64)");
  if (ids && ((N % 4) != 0 || ((uintptr_t)ids & 7u) != 0))
    return set_err(ctx, CSM_E_INVAL, "csm_signal_halo: ids need N %% 4 == 0, 8-B alignment");
  const HaloArgs ha{H, F, before ? 1 : 0, after ? 1 : 0, flags};
  return signal_launch(ctx, "csm_signal_halo", P, T_d, N, month_start, T_m, max_month_days, J,
                       skip, PM, R, M, NR, nullptr, nullptr, state, true, ids, &ha);
}

int csm_signal_shard_halo(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N,
                          const int64_t* month_start, int32_t T_m, int32_t max_month_days,
                          int32_t J, int32_t skip, const double* carry, const double* next_pm,
                          double* PM, double* R, double* M, double* NR, double* state,
                          uint16_t* ids) {
  if (!carry || !next_pm)
    return set_err(ctx, CSM_E_INVAL, "csm_signal_shard_halo: needs the halo's carry and next_pm");
  if (ids && ((N % 4) != 0 || ((uintptr_t)ids & 7u) != 0))
    return set_err(ctx, CSM_E_INVAL, "csm_signal_shard_halo: ids need N %% 4 == 0, 8-B alignment");
  return signal_launch(ctx, "csm_signal_shard_halo", P, T_d, N, month_start, T_m, max_month_days,
                       J, skip, PM, R, M, NR, carry, next_pm, state, true, ids);
}

}  // extern "C"
