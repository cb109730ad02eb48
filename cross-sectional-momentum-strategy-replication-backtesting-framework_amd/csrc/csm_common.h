// csm_common.h -- shared by the engine's translation units: the NaN-payload presence
// encoding, the context object and the status/error plumbing of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "../../include/csmom.h"

#define ABSENT_BITS 0x7FF4000000000001ULL
#define ABSENT_MASK 0x7FF7FFFFFFFFFFFFULL

__device__ __forceinline__ bool is_absent(double x) {
  return (((uint64_t)__double_as_longlong(x)) & ABSENT_MASK) == ABSENT_BITS;
}
__device__ __forceinline__ double absent_val() { return __longlong_as_double((long long)ABSENT_BITS); }
__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7FF8000000000000LL); }
__device__ __forceinline__ bool isnan_d(double x) { return x != x; }

// The halving tree over a wave's 64 lanes (h = 32..1: lane j += lane j + h); lane 0 holds the sum.
// Rules R1, N3, N4, U4 and I5 name this order.
template <typename T>
__device__ __forceinline__ T wave_tree(T v) {
#pragma unroll
  for (int h = 32; h > 0; h >>= 1) v = v + __shfl_down(v, h, 64);
  return v;
}

// A [T_m][N] panel an entry point refuses: an empty side, more than 2^40 cells, or a row of more
// than n_max cells (the calls that keep 32-bit positions in a row pass 2^31 - 1).
static inline bool bad_panel(int32_t T_m, int64_t N, int64_t n_max = INT64_MAX) {
  return T_m < 1 || N < 1 || N > n_max || (int64_t)T_m > ((int64_t)1 << 40) / N;
}

struct csm_ctx {
  int device;
  hipStream_t stream;
  char err[512];
  void* scratch;          // context-owned device workspace (k_deciles bucket ids), grown lazily
  size_t scratch_bytes;
  int n_cu;               // compute units of the device (decile kernel choice)
  int32_t* dec_flg;       // one int per row the merged decile pass left to the general kernel
  size_t dec_flg_bytes;   // (allocated at create, so a captured pipeline never allocates)
  int32_t* ticket;        // the fused long-short's arrival counter (zeroed at create; it wraps
                          // back to 0 on each decile launch's last increment)
  void* dsplit;           // the split decile pass's workspace (DecSplit), grown lazily
  size_t dsplit_bytes;
  void* comm;             // RCCL communicator of csm_allgather_init (collective.hip), or NULL
  int comm_rank, comm_size;
  // portfolio workspaces and what their last cohort pass wrote (portfolio.hip): bit 0 the leg
  // bitplanes -- the turnover pass reads bitplanes only from a workspace recorded here, whatever
  // the tune knobs say by then (a knob changed between the two calls falls back to the label
  // bytes) -- bit 1 legs-only cohort partials in the two-leg layout ([rows][K][C][2])
  void* planes_ws[32];
  unsigned char planes_bits[32];
  int planes_next;
  void* mkt_ws;           // csm_market_factor's per-slice partial sums and counts (market.hip),
  size_t mkt_ws_bytes;    // grown lazily
  void* xs_ws;            // csm_xs_regress's per-slice partial sums and counts, or a series too
  size_t xs_ws_bytes;     // long for csm_newey_west's LDS (xsreg.hip), grown lazily
  void* grp_ws;           // csm_group_deciles / csm_group_stats: the packed rows, segment offsets
  size_t grp_ws_bytes;    // and per-group sums; csm_xs_rank's the same, csm_rank_ic's index list
                          // and key rows (groups.hip), csm_deciles_bp's packed keys and edges
                          // (breakpoints.hip), grown lazily
};

static inline int set_err(csm_ctx* c, int code, const char* fmt, ...) {
  if (c) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(c->err, sizeof(c->err), fmt, ap);
    va_end(ap);
  }
  return code;
}

#define HIP_CHECK(ctx, call)                                                               \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return set_err(ctx, CSM_E_HIP, "%s: %s", #call, hipGetErrorString(e_));              \
  } while (0)

#define LAUNCH_CHECK(ctx, name)                                                            \
  do {                                                                                     \
    hipError_t e_ = hipGetLastError();                                                     \
    if (e_ != hipSuccess) return set_err(ctx, CSM_E_HIP, "%s launch: %s", name, hipGetErrorString(e_)); \
  } while (0)

static inline int prep(csm_ctx* c) {
  if (!c) return CSM_E_INVAL;
  c->err[0] = 0;
  HIP_CHECK(c, hipSetDevice(c->device));
  return CSM_OK;
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// One csm_tune knob: its key, the variable it sets and the values it accepts.  tune_set stores
// value into the table's knob named key; CSM_E_INVAL for a NULL or unknown key or a value the
// knob does not accept.
struct TuneKnob {
  const char* key;
  int* var;
  bool (*ok)(int);
};
template <size_t n>
static inline int tune_set(const TuneKnob (&tab)[n], const char* key, int value) {
  if (!key) return CSM_E_INVAL;
  for (const TuneKnob& k : tab)
    if (!strcmp(key, k.key) && k.ok(value)) {
      *k.var = value;
      return CSM_OK;
    }
  return CSM_E_INVAL;
}

// Whether the context's stream is being captured into a hipGraph.  Context-owned buffers are
// baked into a captured graph by address, so they are never (re)allocated while capturing.
static inline bool capturing(csm_ctx* c) {
  hipStreamCaptureStatus s = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(c->stream, &s) == hipSuccess && s != hipStreamCaptureStatusNone;
}
// Grows the context-owned buffer *ptr (*have bytes) to at least `need` bytes; its contents are
// not kept.
template <typename T>
static inline int ctx_reserve(csm_ctx* c, const char* who, const char* what, T** ptr,
                              size_t* have, size_t need) {
  if (*have >= need) return CSM_OK;
  if (capturing(c))   // a captured graph would keep the freed buffer's address
    return set_err(c, CSM_E_INVAL, "%s: %s (%zu B) must grow to %zu B during stream capture; "
                   "run the call once before capturing", who, what, *have, need);
  if (*ptr) HIP_CHECK(c, hipFree(*ptr));
  *ptr = nullptr;
  *have = 0;
  HIP_CHECK(c, hipMalloc(ptr, need));
  *have = need;
  return CSM_OK;
}

// Device counters / flags the library resets before a launch that accumulates into them are
// zeroed by a kernel, not by hipMemsetAsync: a kernel node replays the same way in a captured
// graph as eagerly (the turnover work-list counter, the boot-scan domain flag).
static __global__ void k_zero_i32(int32_t* __restrict__ p, int n) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < n) p[i] = 0;
}
static inline hipError_t zero_i32_async(int32_t* p, int n, hipStream_t st) {
  hipLaunchKernelGGL(k_zero_i32, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, p, n);
  return hipGetLastError();
}

// ---- calls between the engine's sources -------------------------------------------------------
// A kernel is defined in one source, beside every host function that takes its address; another
// source launches it through one of these.
// Each stage's csm_tune table (the knob variables are static in the stage's source); csm_tune and
// csm_tune_ptr (context.hip) try them in turn.
int csm_tune_scans(const char* key, int value);       // scans.hip
int csm_tune_signal(const char* key, int value);      // signal.hip
int csm_tune_signal_tc(const char* key, int value);   // signal_tc.hip
int csm_tune_deciles(const char* key, int value);     // deciles_wide.hip
int csm_tune_ptr_deciles(const char* key, void* p);
int csm_tune_shards(const char* key, int value);      // shards.hip
extern "C" {   // (these are among the library's exported symbols)
int csm_tune_portfolio(const char* key, int value);   // portfolio.hip
int csm_tune_ptr_portfolio(const char* key, void* p);
int csm_tune_signals(const char* key, int value);     // signals.hip
int csm_tune_market(const char* key, int value);      // market.hip
int csm_tune_groups(const char* key, int value);      // groups.hip
int csm_tune_dailymkt(const char* key, int value);    // dailymkt.hip
int csm_tune_liq(const char* key, int value);         // liquidity.hip
int csm_tune_range(const char* key, int value);       // range.hip
int csm_tune_asym(const char* key, int value);        // asym.hip
}
// The fused month-end + scan launch behind every csm_signal* entry point and csm_pipeline
// (signal.hip): k_signal_tail or k_signal for the panel's width and alignment and the signal
// knobs.  sh: a date-shard pass (carry_out is the shard's end-state record); ids: the decile
// pass's bucket ids, or NULL; halo: the fused halo prologue's arguments, or NULL.
struct HaloArgs;
int signal_launch(csm_ctx* ctx, const char* who, const double* P, int64_t T_d, int64_t N,
                  const int64_t* month_start, int32_t T_m, int32_t max_month_days, int32_t J,
                  int32_t skip, double* PM, double* R, double* M, double* NR, const double* carry,
                  const double* next_pm, double* carry_out, bool sh = false,
                  uint16_t* ids = nullptr, const HaloArgs* halo = nullptr);
// The exchange records of G month chunks of a [T_m][N] month-price panel, out [G][6 + T][N], and
// their fold into each chunk's carry (g < 0: every chunk, outputs stacked per chunk; else chunk g
// alone) -- shards.hip's k_shard_summary_chunked and k_fold_carry, which the time-chunked scans
// of scans.hip launch too.  The caller checks the launch (LAUNCH_CHECK).
struct FoldJs;
void launch_shard_summary_chunked(hipStream_t st, const double* PM, int T_m, int64_t N, int T,
                                  int G, double* out);
void launch_fold_carry(hipStream_t st, const double* sm, int G, int g, int64_t N, int J, int skip,
                       double* carry, double* next_pm, const double* tail_pm, const FoldJs& jq,
                       double* psq);

// ---- shared by the decile kernels (deciles_wide.hip and deciles_narrow.hip) ------------------
#define MAXQ 21  // n_bins + 1 <= 21
#define MAXT 42  // distinct target ranks (2 per interior quantile + min + max)
// Phase timestamps (profiling aid, csm_tune_ptr("dec_timing", buf)): per date row, wall-clock
// ticks at DEC_NPH phase boundaries, written by thread 0 when the pointer is set.
#define DEC_NPH 9
__device__ __forceinline__ void dec_mark(int64_t* tim, int t, int ph) {
  if (tim && threadIdx.x == 0) tim[(int64_t)t * DEC_NPH + ph] = (int64_t)wall_clock64();
}
struct QTab {
  double q[MAXQ];
  // legs mode (csm_deciles_ids_legs; labels-only merged pass, n_bins >= 4): only the first and
  // last decile are exact -- every other ranked cell gets some label in [1, n_bins - 2]
  int legs = 0;
};

// Fixed bucket map of the fused pipeline (csm_signal_ids writes one u16 id per asset-month,
// the decile pass histograms the ids instead of re-reading mom_J): y = fl(1 + x), 1024
// buckets per octave of y over [1/16, 16), clamped at both ends (x <= -15/16 -> 0, x >= 15
// -> 8191).  fl(1 + x) is monotone in x and so are the bits of a positive double, so the map is
// monotone non-decreasing: bucket order never contradicts value order, and the decile pass
// stays exact for ANY data -- the map only decides how many values share a bucket.  12-month
// momentum cross-sections (log-normal-ish in y) put ~5-10 of 100k values in a bulk bucket and
// almost none in the clamped end buckets (2048 per octave over [1/4, 4) halved the target
// buckets but left ~600-3000 values in the end buckets, whose exact min / max the pass needs);
// a row the map fits badly falls back to key-space refinement (slower, same labels).
#define CSM_FB_BUCKETS 8192
#define CSM_FB_NAN 0xFFFFu
// (bits >> 42 of the double, taken as the high word's arithmetic >> 10: the same value with
// 32-bit operations -- the id is computed for every asset-month by the VALU-bound scans)
__device__ __forceinline__ int csm_fbucket(double x) {
  const int b = __double2hiint(1.0 + x) >> 10;
  const int k = b - (0x3FB00000 >> 10);   // bits(1/16) >> 42
  return k < 0 ? 0 : (k > CSM_FB_BUCKETS - 1 ? CSM_FB_BUCKETS - 1 : k);
}
// set bits of a wave mask below this lane (v_mbcnt_lo / hi: 2 ops; the popcount of the masked
// ballot is 4)
__device__ __forceinline__ int lane_prefix(uint64_t m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
__device__ __forceinline__ uint32_t csm_fid(double x) {
  return x == x ? (uint32_t)csm_fbucket(x) : CSM_FB_NAN;
}

// The split decile pass on ids (deciles.inc, wide rows): device workspace of the plan / sweep /
// finish launches, carved from the context's split buffer (deciles_wide.hip dsplit_layout).  A chunk is
// a whole number of the merged pass's sweep trips (SPLIT_TRIP cells: 512 lanes x 4 groups x 4
// cells), and a sweep workgroup's lane owns the cells the merged pass's lane of that index owns
// there, so both passes sum next_ret in the same order (deciles.inc DEC_CHUNK_ORDER).
#define SPLIT_CELLS 32768   // default cells per sweep chunk (csm_tune "dec_split_cells"; the
                            // chunking depends on N and that knob only, never on the launch)
#define SPLIT_TRIP 8192     // cells of one merged-sweep trip: chunks are multiples of it
#define SPLIT_THREADS 512
#define SPLIT_WAVES (SPLIT_THREADS / 64)
#define SPLIT_FL 1024       // uncertain cells a sweep wave can list per chunk
#define DSPLAN_BYTES 4096   // one row's DsPlan
#define DSPLIT_MAXL 512     // (chunk, wave) lists per row the finish launch merges
struct DecSplit {
  char* plan;        // [T_m] DsPlan (slots, targets, ranked count)
  int8_t* tab;       // [T_m][8192] bucket -> label (-1 NaN, >= 0 certain, <= -2 uncertain)
  double* lp;        // [T_m][C][MAXQ - 1][SPLIT_THREADS] each lane's certain-cell next_ret sum
                     //   per label, per chunk (the merged pass's per-lane chunk partials)
  int32_t* pc;       // [T_m][C][MAXQ] certain-cell counts per label, per chunk
  int32_t* ucnt;     // [T_m][C][SPLIT_WAVES] uncertain cells listed per (chunk, wave)
  uint32_t* ulist;   // [T_m][C][SPLIT_WAVES][SPLIT_FL] their cell indices
  int C;             // chunks per row: ceil(N / cells)
  int64_t cells;     // cells per chunk (a multiple of SPLIT_TRIP)
  int pf;            // the sweep's prefetching variant (no more (chunk, date) pairs than CUs)
};


// Calls f(std::integral_constant<int, NB>{}) for the NB of the list that equals n_bins (the
// kernels take the bin count as a template parameter); false, and no call, when none does.
template <int... NBs, typename F>
static inline bool nb_dispatch(int n_bins, F&& f) {
  return ((n_bins == NBs && (f(std::integral_constant<int, NBs>{}), true)) || ...);
}

// The arguments of one decile pass, filled once by deciles_wide.hip's deciles_dispatch and unpacked
// into k_deciles's parameters at each launch (dec_launch).  A field the pass does not use is NULL.
struct DecLaunch {
  int T_m;            // date rows: one workgroup each
  hipStream_t st;
  const double* M;
  const double* NR;   // NULL: labels only (NB = 0)
  int64_t N;
  int n_bins;
  QTab q;
  int8_t* L;
  double* EW;
  int32_t* CNT;
  int32_t* NV;
  int64_t* tim;
  uint16_t* ids;      // the fixed map's bucket ids (the PRE kernels); NULL: the kernels that read M
  int32_t* flg;       // [T_m] ints: the merged pass first, then the general kernel for the rows it
                      // left (flg[t] = 1); NULL: the general kernel only
  double* LS;         // with ticket (NB > 0): the long-short by the pass's last workgroup
  int32_t* ticket;
  bool v2;            // paired loads (the kernels that read M: even N, aligned M / NR / L)
};

// every k_deciles instantiation of deciles.inc; NB in {0, 2, 3, 4, 5, 10, 20}, 0 without NR
using DecKernel = void (*)(const double*, const double*, int64_t, int, QTab, int8_t*, double*,
                           int32_t*, int32_t*, int64_t*, uint16_t*, int32_t*, double*, int32_t*,
                           DecSplit);
template <typename F>
static inline bool dec_nb_dispatch(const DecLaunch& a, F&& f) {
  return nb_dispatch<0, 2, 3, 4, 5, 10, 20>(a.NR ? a.n_bins : 0, f);
}
// one workgroup of `threads` per row; flg / LS / ticket are the launch's own (a pass of several
// launches gives them to some and NULL to others)
static inline void dec_launch(DecKernel k, unsigned threads, const DecLaunch& a, int32_t* flg,
                              double* LS, int32_t* ticket, DecSplit sp = DecSplit{}) {
  void* args[] = {(void*)&a.M,  (void*)&a.NR,  (void*)&a.N,   (void*)&a.n_bins, (void*)&a.q,
                  (void*)&a.L,  (void*)&a.EW,  (void*)&a.CNT, (void*)&a.NV,     (void*)&a.tim,
                  (void*)&a.ids, &flg,         &LS,           &ticket,          &sp};
  (void)hipLaunchKernel((const void*)k, dim3(a.T_m), dim3(threads), args, 0, a.st);
}

// The decile launchers; each returns false, having launched nothing, when n_bins is not a
// compiled NB (dec_nb_dispatch).
// rows of a few thousand assets reading M (deciles_narrow.hip)
bool launch_deciles_narrow(const DecLaunch& a);
// the fused pipeline's wide rows on ids (deciles_pre.hip); the merged pass sums in the split
// pass's order, its chunks of `cells` cells
bool launch_deciles_pre(const DecLaunch& a, int64_t cells);
// the split pass (plan, chunked sweep, finish + the general path for the rows it leaves) on
// wide rows of short date shards; a.flg required
bool launch_deciles_split(const DecLaunch& a, const DecSplit& sp);
// narrow rows on ids (deciles_npre.hip: 2048 buckets = the fixed map's ids >> 2); a.flg with
// decile sums: ONE launch, a row the merged pass gives up taking the general path in the same
// workgroup
bool launch_deciles_pre_narrow(const DecLaunch& a);
