/*
 * csmom.h -- C ABI of libcsmom.so, the MI355X (gfx950) engine for the cross-sectional
 * momentum backtest hot path of
 * AkshayJha22/Cross-Sectional-Momentum-Strategy-Replication-Backtesting-Framework.
 *
 * The reference has no FFI: its boundary is plain Python functions on pandas objects
 * (SURVEY.md section 8(b)).  Each entry point below replaces the arithmetic of one of
 * those functions; the Python layer in the package keeps the reference's signatures and
 * calls these through ctypes.
 *
 * Conventions
 *   - Every array argument is a DEVICE pointer (hipMalloc / torch ROCm tensor) unless it
 *     is documented as a host pointer.  Buffers are caller-owned.
 *   - Dense row-major [T][N] layouts, assets fastest, float64 throughout.
 *   - A cell with no daily row ("absent") holds the NaN payload CSM_ABSENT_BITS; a present
 *     row with a missing price holds an ordinary NaN.
 *   - Calls are asynchronous on the context's stream (csm_set_stream); csm_sync waits.
 *   - Every call returns CSM_OK (0) or a negative status; csm_last_error() describes it.
 *   - A context is not thread-safe; separate contexts may be used concurrently.
 */
#ifndef CSMOM_H
#define CSMOM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSM_ABI_VERSION 3
#define CSM_ABSENT_BITS 0x7FF4000000000001ULL

#define CSM_OK 0
#define CSM_E_INVAL (-1)   /* bad argument (null pointer, size, unsupported parameter) */
#define CSM_E_HIP (-2)     /* HIP runtime / launch failure */
#define CSM_E_RCCL (-3)    /* RCCL missing or a collective failed */
#define CSM_E_TIMEOUT (-4) /* an in-launch hand-off gave up a wait: that launch's outputs are invalid */
#define CSM_UNIQUE_ID_BYTES 128

typedef struct csm_ctx csm_ctx;

int csm_abi_version(void);

/* Process-wide knobs that select between PRODUCT paths with identical results (so tests can
 * drive the fallbacks on inputs that would not reach them): "signal_vec" (2 paired 16-B rows |
 * 1 one asset per lane, the odd-N path), "signal_bwf" (0 auto | 1 one-wave blocks | 4 the wide
 * panels' four barrier-free waves with buffer loads), "signal_j12" (1 the wide date-shard kernel's
 * J = 12 with the product length fixed at compile time | 0 runtime J), "signal_tail" (the
 * one-GPU fused signal on even N and 16-B aligned buffers: 0 the streaming kernel, every day row
 * read | 1 the tail-first kernel -- each month's last day row, then a walk back, a cell per
 * lane, only where that row holds no price | 2 auto, the default: the tail-first kernel below
 * 92,160 assets; from there on both kernels are launched and every wave of both first samples
 * the same 1,024 last-day cells over the calendar and the panel: the tail-first kernel runs
 * where at most one sampled cell in eight holds no price, the streaming kernel elsewhere, and
 * the other returns at once -- no host round trip, no state on the device or between calls),
 * "cols_wg" (1 the halo pass's listed
 * columns summarised / repaired one workgroup per column, month prices derived together in LDS |
 * 0 one thread per column), "dec_merge" (1 the merged decile sweep on
 * ids, the general kernel for the rows it leaves | 0 the general kernel only), "dec_split" (2
 * auto: wide rows on ids take the split pass -- plan, chunked sweep, finish -- in launches of
 * fewer rows than half the CUs (short date shards) | 1 always | 0 the merged pass with one
 * workgroup per row; the same labels, counts and means bit for bit), "mj_reg"
 * (csm_momentum_multi: 2 register ring, two assets per lane | 1 one asset | 0 the LDS ring),
 * "dec_narrow_max" (widest row for the narrow-row decile kernels), "cohort_seg" / "cohort_lds"
 * (portfolio cohort-sum kernel: label-sorted segments (rows <= 7168) | per-wave LDS sums |
 * register sums; "cohort_seg" changes the chunk plan, so set it before sizing the portfolio
 * workspace), "turn_want" (turnover workgroups per launch, default 4096; set before sizing
 * the portfolio workspace), "turn_gen_grid" (workgroups of the general-row turnover launch,
 * default 8192), "overlap_rows" (1 one thread per (month, panel, decile) for single-chunk
 * plans | 0 one per (K, month, panel, decile)), "gen_reset" (1 the turnover work-list counter
 * reset by a kernel | 0 by hipMemsetAsync, round 3's form, kept for the graph-replay diagnosis
 * of tests/test_gpu_capture.py), "turn_vwg" (1 a grouped batch's steady value-weight turnover
 * rows by one workgroup per weight panel | 0 one per row), "turn_mask" (1 steady equal-weight
 * legs turnover rows counted from the legs label sort's leg bitplanes | 0 from the label
 * bytes), "ls_opt" (1 the one-wave legs label sort's prefix ranks by v_mbcnt | 0 masked
 * popcounts), "dec_split_cells" (cells per chunk of the split decile sweep, default 32768, a
 * multiple of 8192 -- the merged pass's sweep trip -- so the merged and split passes sum every
 * row's decile means in the same order; the split workspace is the context's), "dec_split_pf"
 * (the split sweep: 0 two workgroups per CU, the default | 1 one prefetching workgroup per CU |
 * 2 the prefetching one when the launch has no more (chunk, date) pairs than CUs; the same
 * bits either way), "tc_spins" (polling trips a
 * csm_signal_chunked workgroup makes before it gives up a wait, default 2^21; 0 gives up at
 * once, which only the tests of the CSM_E_TIMEOUT report set), "stats_chunks" (csm_month_stats's
 * month chunks: 0 auto, one month each | n >= 1 that many, clamped to T_m), "mm_chunks"
 * (csm_market_model's month chunks: 0 auto | n >= 1 that many, clamped to T_m; the same bits),
 * "dmkt_chunk_days" / "dsums_chunks" / "dmodel_chunks" (csm_daily_market's day rows per
 * workgroup, csm_daily_sums's and csm_daily_model's month chunks: 0 auto; the same bits),
 * "fm_chunks" / "dfsums_chunks" / "dfmodel_chunks" (csm_factor_model's, csm_daily_fsums's and
 * csm_daily_fmodel's month chunks: 0 auto | n >= 1 that many, clamped to T_m; the same bits),
 * "lsums_chunks" / "lmodel_chunks" (csm_liq_sums's and csm_liq_model's month chunks: 0 auto |
 * n >= 1 that many, clamped to T_m), "lsums_pair" (csm_liq_sums: 0 one asset per lane | 1 two
 * where the panels allow; the same bits from all three), "rsums_chunks" / "rmodel_chunks"
 * (csm_range_sums's and csm_range_model's month chunks: 0 auto | n >= 1 that many, clamped to
 * T_m; the same bits), "asums_chunks" / "amodel_chunks" (csm_asym_sums's and csm_asym_model's month
 * chunks: 0 auto | n >= 1 that many, clamped to T_m), "asums_pair" (csm_asym_sums: 0 auto, one
 * asset per lane | 1 one per lane | 2 two where the panels allow; the same bits from all).
 * Returns CSM_E_INVAL for an unknown key or value. */
int csm_tune(const char* key, int value);
/* Profiling aids: "dec_timing" = device int64 buffer [T_m][9] that k_deciles fills with
 * wall-clock ticks (100 MHz) at its phase boundaries; "gen_probe" = device int32 that receives
 * the turnover work-list length the general-row launch read (NULL switches either off). */
int csm_tune_ptr(const char* key, void* p);

/* Create a context bound to HIP device `device` (stream = the null stream). */
int csm_create(int device, csm_ctx** out);
int csm_destroy(csm_ctx* ctx);
const char* csm_last_error(const csm_ctx* ctx);
/* Launch subsequent work on `stream` (a hipStream_t; NULL = the null stream). */
int csm_set_stream(csm_ctx* ctx, void* stream);
int csm_sync(csm_ctx* ctx);

/*
 * Month-end aggregation.  Replaces the `groupby(['ticker', Grouper(freq='ME')])
 * .agg(adj_close=last, monthly_volume=sum)` of src/features.py:34-39.
 *   P[T_d][N]        daily adj_close (ABSENT / NaN encoded)
 *   V[T_d][N]        daily volume, nullable (NaN counts as 0, features.py:31)
 *   month_start[T_m+1] int64 day offsets of each month (device)
 *   PM[T_m][N]       out: last non-NaN price; NaN if the month has rows but no price;
 *                    ABSENT if it has no row
 *   VOL[T_m][N]      out, nullable: pandas-Kahan sum of volume over present days
 */
int csm_month_end(csm_ctx* ctx, const double* P, const double* V, int64_t T_d, int64_t N,
                  const int64_t* month_start, int32_t T_m, double* PM, double* VOL);

/*
 * ret_1m / mom_J / next_ret scan over present rows of each asset.  Replaces
 * src/features.py:44-52 (pct_change with ffill; shift(skip).rolling(J).apply(prod))
 * and run_demo.py:48 (next-row return within the ranked subset).
 *   PM[T_m][N]   month prices from csm_month_end
 *   R, M, NR     out [T_m][N]; R nullable.  NaN where undefined or absent.
 *   carry        nullable [(J+skip)+2][N]: inherited scan state for a date shard
 *                (rows 0..J+skip-1: ring of factors fl(1+ret), oldest first;
 *                row J+skip: pff (last valid price); row J+skip+1: psff)
 *   next_pm      nullable [N]: month price of the first present row after the panel
 *                (ABSENT if none)
 *   carry_out    nullable [(J+skip)+2][N]: scan state after the panel
 * J >= 1, skip >= 0, J + skip <= 256.
 */
int csm_momentum(csm_ctx* ctx, const double* PM, int32_t T_m, int64_t N, int32_t J,
                 int32_t skip, double* R, double* M, double* NR, const double* carry,
                 const double* next_pm, double* carry_out);

/*
 * Several look-backs in one scan (parameter sweeps): Js[nJ] (1 <= nJ <= 4, host array),
 * M[q] / NR[q] host arrays of device [T_m][N] outputs.  One read of PM; each (M[q], NR[q])
 * equals csm_momentum(PM, Js[q], skip) bit for bit.  max(J) + skip <= 64; no carry.
 * Replaces, per sweep batch, the per-J `compute_monthly_momentum_from_daily(...,
 * lookback_months=J)` calls (src/features.py:47-52, run_demo.py:48).
 */
int csm_momentum_multi(csm_ctx* ctx, const double* PM, int32_t T_m, int64_t N,
                       const int32_t* Js, int32_t nJ, int32_t skip, double* const* M,
                       double* const* NR);
/*
 * csm_momentum_multi that also writes, per look-back, ids[q][T_m][N] (uint16, host array of
 * device pointers): each mom_J's fixed-map bucket id (as csm_signal_ids; 0xFFFF = NaN), so the
 * sweep's decile pass (csm_deciles_ids on the [T_m * B][N] rows of a batch) reads 2-B ids and M
 * only near the bin edges.  Same M / NR bits as csm_momentum_multi.
 */
int csm_momentum_multi_ids(csm_ctx* ctx, const double* PM, int32_t T_m, int64_t N,
                           const int32_t* Js, int32_t nJ, int32_t skip, double* const* M,
                           double* const* NR, uint16_t* const* ids);

/*
 * Time-chunked scan for panels with few assets: the months are split into C contiguous
 * chunks that are scanned concurrently from exactly rebuilt boundary states (the date-shard
 * summary/fold of csm_shard_summary / csm_fold_carry, inside one GPU).  Same outputs as
 * csm_momentum (no carry input).  workspace: device buffer of
 * csm_momentum_chunked_workspace(T_m, N, J, skip, C) bytes.
 */
int64_t csm_momentum_chunked_workspace(int32_t T_m, int64_t N, int32_t J, int32_t skip,
                                       int32_t C);
int csm_momentum_chunked(csm_ctx* ctx, const double* PM, int32_t T_m, int64_t N, int32_t J,
                         int32_t skip, int32_t C, double* R, double* M, double* NR,
                         const double* next_pm, void* workspace);
/*
 * csm_momentum_chunked that also writes ids[T_m][N] (uint16): each mom_J's fixed-map bucket id
 * (as csm_signal_ids), so a narrow panel's decile pass (csm_deciles_ids, C2) reads 2-B ids and
 * mom_J only near the bin edges.  Same R / M / NR bits.  N % 4 == 0, 8-B aligned ids.
 */
int csm_momentum_chunked_ids(csm_ctx* ctx, const double* PM, int32_t T_m, int64_t N, int32_t J,
                             int32_t skip, int32_t C, double* R, double* M, double* NR,
                             const double* next_pm, uint16_t* ids, void* workspace);
/*
 * Month-end + time-chunked scan in ONE launch for narrow panels (C2; replaces csm_month_end ->
 * csm_momentum_chunked_ids, four launches): a workgroup reduces one chunk's daily rows of 256
 * assets to month prices in LDS, publishes the chunk's exchange record, folds the records of
 * the earlier chunks of its columns (in-launch hand-off, bounded spins) and scans its months.
 * The same R / M / NR / ids bits as csm_month_end -> csm_momentum (month_start / P as
 * csm_signal; no carry, no next_pm: whole panels).  R and ids nullable.  Even N, months of at
 * most 23 day rows (max_month_days), J + skip <= 32, 1 <= C <= 64 chunks of at most 32
 * months, 16-B aligned P / M / NR / R, 4-B aligned ids.  workspace:
 * csm_signal_chunked_workspace(T_m, N, J, skip, C) bytes, 256-B aligned and ZERO-FILLED before
 * its first use (a launch leaves its sync words zero again; word 2 is set if a wait gave up,
 * which no correct launch does).  One launch at a time per workspace: two launches in flight
 * on different streams must not share one (their tickets and flags would mix).
 * A give-up is never silent: csm_signal_chunked_status reports it.
 */
int64_t csm_signal_chunked_workspace(int32_t T_m, int64_t N, int32_t J, int32_t skip, int32_t C);
int csm_signal_chunked(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N,
                       const int64_t* month_start, int32_t T_m, int32_t max_month_days,
                       int32_t J, int32_t skip, int32_t C, double* R, double* M, double* NR,
                       uint16_t* ids, void* workspace);
/*
 * Synchronises the context's stream and reads the workspace's give-up mark: CSM_OK, or
 * CSM_E_TIMEOUT when a csm_signal_chunked launch on it since the last check gave up a wait (its
 * outputs are invalid); the mark is then cleared.  CSM_E_INVAL while the stream is capturing
 * (check after the graph's replay).
 */
int csm_signal_chunked_status(csm_ctx* ctx, void* workspace);
/*
 * The two together for narrow sweep panels (C3): every look-back Js[q] (1 <= nJ <= 4, host
 * arrays as csm_momentum_multi) from ONE time-chunked scan -- one summary / fold for max(J) (plus
 * each J's subset-ffilled price) and one chunked multi-J scan instead of three launches per J.
 * Each (M[q], NR[q], ids[q]) equals csm_momentum(PM, Js[q], skip) (+ its ids) bit for bit.  ids
 * nullable (else a host array of device uint16 [T_m][N]).  max(J) + skip <= 16, even N, 16-B
 * aligned PM / M / NR / workspace.  workspace: csm_momentum_multi_chunked_workspace(T_m, N,
 * max(J), skip, C) bytes.
 */
int64_t csm_momentum_multi_chunked_workspace(int32_t T_m, int64_t N, int32_t Jmax, int32_t skip,
                                             int32_t C);
int csm_momentum_multi_chunked(csm_ctx* ctx, const double* PM, int32_t T_m, int64_t N,
                               const int32_t* Js, int32_t nJ, int32_t skip, int32_t C,
                               double* const* M, double* const* NR, uint16_t* const* ids,
                               void* workspace);

/*
 * Fused month-end aggregation + scan in one pass over the daily panel (csm_month_end then
 * csm_momentum without the PM round trip).  Same outputs and carry contract as
 * csm_momentum; PM and R nullable; no volume.  max_month_days (HOST value: the longest
 * month in days) must be <= 32.  Even N with 16-B aligned P takes 16-B row loads.
 */
int csm_signal(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N, const int64_t* month_start,
               int32_t T_m, int32_t max_month_days, int32_t J, int32_t skip, double* PM,
               double* R, double* M, double* NR, const double* carry, const double* next_pm,
               double* carry_out);

/*
 * csm_signal (no carry) that also writes ids[T_m][N] (uint16, 8-B aligned, N % 4 == 0): each
 * mom_J's bucket under the fixed monotone map of csm_deciles_ids (0xFFFF = NaN), so the decile
 * pass reads 2 B per cell instead of 8.  min_month_days (HOST value: the shortest interior
 * month in days; 0 = unknown) is accepted for ABI stability and not used by this build.
 */
int csm_signal_ids(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N,
                   const int64_t* month_start, int32_t T_m, int32_t max_month_days,
                   int32_t min_month_days, int32_t J, int32_t skip, double* PM, double* R,
                   double* M, double* NR, uint16_t* ids);

/*
 * Per-date qcut labels, fused with the equal-weight decile means.  Replaces
 * run_demo.py:18-29 (assign_deciles_per_date via pd.qcut(duplicates='drop')),
 * run_demo.py:46 (groupby('date').transform) and run_demo.py:49-55 (dropna +
 * groupby(['date','decile']).next_ret.mean()).
 *   M[T_m][N]     signal (NaN = not ranked)
 *   NR[T_m][N]    nullable: next-row returns; when NULL, EW/CNT are not produced
 *   qtable        HOST pointer, n_bins+1 quantile levels as NumPy's percentile sees them
 *                 ((linspace(0,1,n+1)*100)/100)
 *   L[T_m][N]     out int8 labels, -1 = NaN
 *   EW[T_m][n_bins]  out, nullable: mean next_ret per (date, label), NaN if empty
 *   CNT[T_m][n_bins] out, nullable: row counts per (date, label)
 *   NV[T_m]       out, nullable: ranked rows per date
 * n_bins in {2,3,4,5,10,20} (any n_bins in [1,20] when NR == NULL).
 */
int csm_deciles(csm_ctx* ctx, const double* M, const double* NR, int32_t T_m, int64_t N,
                int32_t n_bins, const double* qtable, int8_t* L, double* EW, int32_t* CNT,
                int32_t* NV);

/*
 * csm_deciles with the ids of csm_signal_ids: the same labels / EW / CNT / NV bit for bit;
 * M is read only for the cells whose bucket holds an order statistic, an interior edge, or
 * the row's min / max.  N % 4 == 0, 16-B aligned M / NR, 4-B aligned L.
 */
int csm_deciles_ids(csm_ctx* ctx, const double* M, const double* NR, const uint16_t* ids,
                    int32_t T_m, int64_t N, int32_t n_bins, const double* qtable, int8_t* L,
                    double* EW, int32_t* CNT, int32_t* NV);

/*
 * csm_deciles_ids + csm_long_short in one call (run_demo.py:46-67).  Narrow rows (N <= 16384,
 * C2): one launch, the decile pass's last workgroup forms LS[T_m] from every date's EW / CNT
 * (the context's arrival counter; concurrent calls of one context on two streams are not
 * supported).  Wider rows: the long-short kernel follows the decile pass.  NR, EW, CNT and LS
 * are required; the same labels / EW / CNT / NV / LS bits as the two calls.
 */
int csm_deciles_ids_ls(csm_ctx* ctx, const double* M, const double* NR, const uint16_t* ids,
                       int32_t T_m, int64_t N, int32_t n_bins, const double* qtable, int8_t* L,
                       double* EW, int32_t* CNT, int32_t* NV, double* LS);

/*
 * csm_deciles_ids without decile sums, for legs-only accounting (csm_cohort_sums_legs /
 * csm_portfolio_from_cohorts_legs, sweep.SweepConfig.legs_only): with n_bins >= 4 the labels
 * 0 and n_bins - 1 and the NaN label (-1) are exactly csm_deciles_ids's, every other ranked
 * cell gets SOME label in [1, n_bins - 2] (the interior edges' order statistics are not
 * selected).  n_bins < 4: exactly csm_deciles_ids.  NV as there (nullable).
 */
int csm_deciles_ids_legs(csm_ctx* ctx, const double* M, const uint16_t* ids, int32_t T_m,
                         int64_t N, int32_t n_bins, const double* qtable, int8_t* L, int32_t* NV);

/*
 * The whole K = 1 path of run_demo.py:31-67 in one call: fused month-end + scan (csm_signal,
 * with ids when N % 4 == 0 and the row is wide), per-date labels fused with the decile means
 * (csm_deciles / csm_deciles_ids), long-short (csm_long_short).  Arguments as in those calls
 * (min_month_days as in csm_signal_ids);
 * PM, R, NV nullable; qtable HOST.  The ids live in a context-owned workspace (T_m * N * 2 B,
 * grown on first use).
 */
int csm_pipeline(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N, const int64_t* month_start,
                 int32_t T_m, int32_t max_month_days, int32_t min_month_days, int32_t J,
                 int32_t skip, int32_t n_bins,
                 const double* qtable, double* PM, double* R, double* M, double* NR, int8_t* L,
                 double* EW, int32_t* CNT, int32_t* NV, double* LS);

/*
 * Long-short series.  Replaces run_demo.py:57-67: top minus bottom label mean when both
 * columns occur anywhere in the panel, else per-date max minus min; NaN = dropped date.
 *   EW, CNT [T_m][n_bins] from csm_deciles;  LS[T_m] out.
 */
int csm_long_short(csm_ctx* ctx, const double* EW, const int32_t* CNT, int32_t T_m,
                   int32_t n_bins, double* LS);

/*
 * Date-shard summary of a shard's month prices (prefix-independent), [S][N] float64 with
 * S = 6 + J + skip + 1 (layout in DESIGN.md / oracle shard_summary).  No reference
 * counterpart: it is the exchange record of the multi-GPU date sharding.
 */
int csm_shard_summary(csm_ctx* ctx, const double* PM, int32_t T_m, int64_t N, int32_t J,
                      int32_t skip, double* out);

/*
 * Fold the all-gathered summaries [G][S][N] into shard g's inherited scan state
 * (carry [(J+skip)+2][N]) and next_pm[N], bit-exactly equal to an unsharded scan.
 */
int csm_fold_carry(csm_ctx* ctx, const double* summaries, int32_t G, int32_t g, int64_t N,
                   int32_t J, int32_t skip, double* carry, double* next_pm);

/*
 * Speculative date shards (the fused multi-GPU pass; no reference counterpart).
 * csm_signal_shard: csm_signal over this rank's months from an EMPTY scan state, before the
 *   earlier shards' carry is known (no carry / next_pm).  PM [T_m][N] is required but only its
 *   first and last J + skip + 8 months are written (the calls below re-derive other months
 *   from P where an asset needs them); state [5][N] out: present months, pending ranked row
 *   (-1 none), its subset-ffilled price, first and last present month (-1 none).  T_m >= 1.
 * csm_shard_summary_state: the csm_shard_summary record of the shard's month prices, bit for
 *   bit, from short walks at both ends of each asset's present months.
 * csm_shard_repair: with carry / next_pm from csm_fold_carry, rewrites R (nullable) / M / NR
 *   where the true carry changes them and finishes the pending rows, so the result equals
 *   csm_momentum(month prices, carry, next_pm) bit for bit.  J + skip <= 128.
 * P / month_start / PM / state are the csm_signal_shard call's.
 */
int csm_signal_shard(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N,
                     const int64_t* month_start, int32_t T_m, int32_t max_month_days, int32_t J,
                     int32_t skip, double* PM, double* R, double* M, double* NR, double* state);
int csm_shard_summary_state(csm_ctx* ctx, const double* P, const int64_t* month_start,
                            const double* PM, int32_t T_m, int64_t N, int32_t J, int32_t skip,
                            const double* state, double* out);
int csm_shard_repair(csm_ctx* ctx, const double* P, const int64_t* month_start, const double* PM,
                     int32_t T_m, int64_t N, int32_t J, int32_t skip, const double* carry,
                     const double* next_pm, const double* state, double* R, double* M,
                     double* NR);
/*
 * The speculative shard pass with bucket ids (for csm_deciles_ids): csm_signal_shard that also
 * writes ids[T_m][N] like csm_signal_ids (N % 4 == 0, 8-B aligned), and csm_shard_repair that
 * rewrites the id of every cell it rewrites.  Same M / NR / R bits as the plain calls.
 */
int csm_signal_shard_ids(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N,
                         const int64_t* month_start, int32_t T_m, int32_t max_month_days,
                         int32_t J, int32_t skip, double* PM, double* R, double* M, double* NR,
                         double* state, uint16_t* ids);
int csm_shard_repair_ids(csm_ctx* ctx, const double* P, const int64_t* month_start,
                         const double* PM, int32_t T_m, int64_t N, int32_t J, int32_t skip,
                         const double* carry, const double* next_pm, const double* state,
                         double* R, double* M, double* NR, uint16_t* ids);

/*
 * Halo date shards (the default multi-GPU pass; no reference counterpart, SURVEY 8(e) and
 * north_star's "J + skip lookback halo").  A rank holds the daily rows of H calendar months
 * before its shard, its T_m shard months and F (0..8) months after it, month_start[H + T_m + F
 * + 1] (day offsets into P, the 'ME' groups of features.py:38).
 * csm_shard_halo: the scan state the halo months leave from an empty state (carry
 *   [(J+skip)+2][N], csm_signal's layout), next_pm[N] = the price of the first forward month
 *   with a row (ABSENT if none), and flags[N]: bit 0 the carry may differ from the one the
 *   whole history leaves (before != 0 -- the panel has months before the halo -- and the halo
 *   lacks two valid prices J + skip present months apart), bit 1 next_pm may differ (after !=
 *   0 -- the panel has months after the forward months -- and no forward row).  halo_pm:
 *   workspace [H + F][N] (the halo and forward months' prices).
 * csm_signal_shard_halo: csm_signal_shard from that carry and next_pm (month_start = the
 *   shard's T_m + 1 offsets, still into P); unflagged assets' outputs are final.
 * csm_shard_need: this rank's exchange bits mask[4][ceil(N / 64)] (bit a % 64 of word a / 64):
 *   row 0 flag bit 0 and a present month in the shard, row 1 flag bit 1 and a pending ranked
 *   row at its end, row 2 a present month, row 3 a present month before the shard's last H
 *   months (the part outside the next rank's halo).
 * csm_shard_union: from every rank's rows [G][4][ceil(N / 64)], the assets some rank needs --
 *   an uncertain carry and a row before that rank's halo, or an uncertain forward price and a
 *   row in a later shard -- as the ascending list idx[min(*count, cap)]; *count its full
 *   length (> cap: overflow -- take the all-gather path).  Same list on every rank.
 * csm_shard_summary_cols: csm_shard_summary_state's record for the listed assets only,
 *   out[S][cap] (columns past *count: an asset with no present month).  All-gather it, fold it
 *   with csm_fold_carry (N = cap), and:
 * csm_shard_repair_cols: csm_shard_repair of the listed assets, their carry / next_pm columns
 *   from that fold ([.][cap]); fcarry = this rank's halo carry (the state the pass started from).
 * csm_shard_fix_cols: the fold and the repair of the listed columns in ONE launch (the halo
 *   pass's default): records = the all-gathered [G][S][cap] records, g = this rank; each listed
 *   column's true carry and forward price are folded from them and every month of the column
 *   is replayed from that carry (the sequential scan: the unsharded pass's R / M / NR / ids).
 */
int csm_shard_halo(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N,
                   const int64_t* month_start, int32_t H, int32_t T_m, int32_t F,
                   int32_t before, int32_t after, int32_t J, int32_t skip, double* halo_pm,
                   double* carry, double* next_pm, uint8_t* flags);
/*
 * csm_signal_halo: csm_shard_halo + csm_signal_shard_halo in ONE launch (the wide shard kernel:
 * even N >= 92160, months of <= 23 day rows; else CSM_E_INVAL -- take the two calls): P and
 * month_start [H + T_m + F + 1] as csm_shard_halo's; the halo state, the forward price and
 * flags [N] (csm_shard_halo's) come from the kernel's prologue, the shard's PM / R / M / NR /
 * state / ids are csm_signal_shard_halo's, bit for bit.
 */
int csm_signal_halo(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N,
                    const int64_t* month_start, int32_t H, int32_t T_m, int32_t F, int32_t before,
                    int32_t after, int32_t max_month_days, int32_t J, int32_t skip, double* PM,
                    double* R, double* M, double* NR, double* state, uint16_t* ids,
                    uint8_t* flags);
int csm_signal_shard_halo(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N,
                          const int64_t* month_start, int32_t T_m, int32_t max_month_days,
                          int32_t J, int32_t skip, const double* carry, const double* next_pm,
                          double* PM, double* R, double* M, double* NR, double* state,
                          uint16_t* ids);
int csm_shard_need(csm_ctx* ctx, const uint8_t* flags, const double* state, int64_t N,
                   int32_t T_m, int32_t H, uint64_t* mask);
int csm_shard_union(csm_ctx* ctx, const uint64_t* masks, int32_t G, int64_t N, int64_t cap,
                    int32_t* idx, int32_t* count);
int csm_shard_summary_cols(csm_ctx* ctx, const double* P, const int64_t* month_start,
                           const double* PM, int32_t T_m, int64_t N, int32_t J, int32_t skip,
                           const double* state, const int32_t* idx, const int32_t* count,
                           int64_t cap, double* out);
int csm_shard_repair_cols(csm_ctx* ctx, const double* P, const int64_t* month_start,
                          const double* PM, int32_t T_m, int64_t N, int32_t J, int32_t skip,
                          const double* carry, const double* next_pm, const double* fcarry,
                          const double* state, const int32_t* idx, const int32_t* count,
                          int64_t cap, double* R, double* M, double* NR, uint16_t* ids);
int csm_shard_fix_cols(csm_ctx* ctx, const double* P, const int64_t* month_start,
                       const double* PM, int32_t T_m, int64_t N, int32_t J, int32_t skip,
                       const double* records, int32_t G, int32_t g, const int32_t* idx,
                       const int32_t* count, int64_t cap, double* R, double* M, double* NR,
                       uint16_t* ids);

/*
 * Portfolio accounting beyond the reference's K = 1 equal-weight case (SURVEY 8(f) rank 2;
 * rules E1..E5 in DESIGN.md section 8 / oracle/portfolio_oracle.py).  The reference counterpart
 * is run_demo.py:49-67 (K = 1, equal weight, no costs), which this collapses to.
 * Panels are batched [T_m][B][N] (B cross-sections per month row; B = 1 for one panel).
 *   L         int8 labels from csm_deciles (-1 = not ranked)
 *   NR        next-row returns (the return held over (t, t+1])
 *   W         nullable: formation weights (value weighting, e.g. market cap); NULL = equal
 *   K         holding months: month t averages the cohorts formed at t-K+1 .. t
 *   half_spread, k_impact, aum, ADV (nullable [T_m][B][N] dollar ADV), SIG (nullable
 *             volatility, NaN/NULL -> 0.02): the cost model of src/execution_models.py:4-12
 *   PR [T_m][B][n_bins]  overlapped decile returns;  LS [T_m][B] long-short (NaN = dropped)
 *   TURN, COST, NET [T_m][B] nullable: long-short turnover (1/2 sum |dw|), cost, LS - COST
 *   workspace: device buffer of csm_portfolio_workspace(T_m, B, N, n_bins, K) bytes
 * n_bins in {2,3,4,5,10,20,30}.
 */
int64_t csm_portfolio_workspace(int32_t T_m, int32_t B, int64_t N, int32_t n_bins, int32_t K);
int csm_portfolio(csm_ctx* ctx, const int8_t* L, const double* NR, const double* W, int32_t T_m,
                  int32_t B, int64_t N, int32_t n_bins, int32_t K, double half_spread,
                  double k_impact, double aum, const double* ADV, const double* SIG, double* PR,
                  double* LS, double* TURN, double* COST, double* NET, void* workspace);

/*
 * The two halves of csm_portfolio, for sweeps over K: cohort sums do not depend on the
 * holding period, so one csm_cohort_sums pass with Kmax cohorts (workspace of
 * csm_portfolio_workspace(T_m, B, N, n_bins, Kmax) bytes) serves csm_portfolio_from_cohorts
 * for every K <= Kmax (same L / W; outputs as csm_portfolio).
 */
int csm_cohort_sums(csm_ctx* ctx, const int8_t* L, const double* NR, const double* W, int32_t T_m,
                    int32_t B, int64_t N, int32_t n_bins, int32_t Kmax, void* workspace);
int csm_portfolio_from_cohorts(csm_ctx* ctx, const int8_t* L, const double* W, int32_t T_m,
                               int32_t B, int64_t N, int32_t n_bins, int32_t Kmax, int32_t K,
                               double half_spread, double k_impact, double aum, const double* ADV,
                               const double* SIG, double* PR, double* LS, double* TURN,
                               double* COST, double* NET, void* workspace);
/* Several holding periods at once (Ks: HOST array of nK values <= Kmax): outputs stacked
 * over K -- PR [nK][T_m][B][n_bins], LS / TURN / COST / NET [nK][T_m][B]; the turnover pass
 * loads each cell's labels once for up to 4 K values. */
int csm_portfolio_from_cohorts_multi(csm_ctx* ctx, const int8_t* L, const double* W,
                                     int32_t T_m, int32_t B, int64_t N, int32_t n_bins,
                                     int32_t Kmax, int32_t nK, const int32_t* Ks,
                                     double half_spread, double k_impact, double aum,
                                     const double* ADV, const double* SIG, double* PR, double* LS,
                                     double* TURN, double* COST, double* NET, void* workspace);

/*
 * Legs-only accounting for sweeps whose outputs are the long-short statistics (SweepRunner:
 * LS / TURN / COST / NET per strategy): csm_cohort_sums_legs sorts and sums only the two legs
 * (deciles 0 and n_bins - 1; rows of <= 7168 assets), csm_portfolio_from_cohorts_legs takes the
 * multi-K accounting from them -- LS, TURN, COST and NET equal the full path's bit for bit, PR
 * holds the two legs (NaN elsewhere).  The reference's long-short rule needs every decile only
 * when a panel lacks one leg's column (run_demo.py:60-65): then *need_full (device int32, set to
 * 0 by the caller) becomes 1 and the caller reruns the full csm_cohort_sums /
 * csm_portfolio_from_cohorts_multi.  The legs pass stores its partials in a two-leg layout and
 * records the layout in the workspace (the accounting reads it there): a full
 * csm_portfolio_from_cohorts* needs the full cohort sums, as before.
 */
/*
 * Equal-weight cohort sums of nJ (<= 4) label panels L[q] that share one next_ret panel NR (the
 * bootstrap sweep's shared next_ret, csm_boot_scan): each workspace[q] (csm_portfolio_workspace
 * bytes) ends up as csm_cohort_sums(_legs)(L[q], NR, NULL, ..., workspace[q]) leaves it, bit for
 * bit, but each month's return row is read once for every J (one launch) where the segment path
 * applies.  legs: 1 = csm_cohort_sums_legs.  Then csm_portfolio_from_cohorts_* per J.
 */
int csm_cohort_sums_js(csm_ctx* ctx, int32_t nJ, const int8_t* const* L, const double* NR,
                       int32_t T_m, int32_t B, int64_t N, int32_t n_bins, int32_t Kmax,
                       int32_t legs, void* const* workspaces);
int csm_cohort_sums_legs(csm_ctx* ctx, const int8_t* L, const double* NR, const double* W,
                         int32_t T_m, int32_t B, int64_t N, int32_t n_bins, int32_t Kmax,
                         void* workspace);
int csm_portfolio_from_cohorts_legs(csm_ctx* ctx, const int8_t* L, const double* W,
                                    int32_t T_m, int32_t B, int64_t N, int32_t n_bins,
                                    int32_t Kmax, int32_t nK, const int32_t* Ks,
                                    double half_spread, double k_impact, double aum,
                                    const double* ADV, const double* SIG, double* PR, double* LS,
                                    double* TURN, double* COST, double* NET, void* workspace,
                                    int32_t* need_full);

/*
 * The cohort sums and accounting of B = G * Bg panels whose labels / next_ret are stored
 * group-major -- L, NR [G][T_m][Bg][N]: G blocks, e.g. G look-backs' label panels as one decile
 * pass over the stacked rows writes them -- and whose weights / ADV / vol are shared by the G
 * groups -- W, ADV, SIG [T_m][Bg][N] (nullable as above).  Each call equals its plain-layout
 * counterpart (csm_cohort_sums(_legs), csm_portfolio_from_cohorts_multi / _legs) on the
 * side-by-side panels ([T_m][G * Bg][N], panel g * Bg + p = group g's panel p, weights repeated
 * per group) bit for bit, outputs and workspace included (csm_portfolio_workspace(T_m, G * Bg,
 * N, n_bins, Kmax) bytes; outputs [nK][T_m][G * Bg]), without those copies.  legs: 1 = the
 * legs-only forms (rows of <= 7168 assets; need_full as csm_portfolio_from_cohorts_legs).
 */
int csm_cohort_sums_grouped(csm_ctx* ctx, int32_t G, const int8_t* L, const double* NR,
                            const double* W, int32_t T_m, int32_t Bg, int64_t N, int32_t n_bins,
                            int32_t Kmax, int32_t legs, void* workspace);

/*
 * csm_cohort_sums_js for label panels stored group-major, L int8 [nJ][T_m][B * N] (the look-backs'
 * panels as one stacked decile pass writes them), into ONE workspace laid out for nJ * B panels
 * (csm_portfolio_workspace(T_m, nJ * B, ...); J q's panel b is panel q * B + b, as
 * csm_cohort_sums_grouped lays it out): one label-sort launch for every J and each month's
 * return row staged once for every J.  csm_portfolio_from_cohorts_grouped(G = nJ, Bg = B) then
 * accounts every J in one launch set.  Where csm_portfolio_plan(T_m, B, ...) equals
 * csm_portfolio_plan(T_m, nJ * B, ...), every J's results are csm_cohort_sums_js's bit for bit.
 */
int csm_cohort_sums_js_grouped(csm_ctx* ctx, int32_t nJ, const int8_t* L, const double* NR,
                               int32_t T_m, int32_t B, int64_t N, int32_t n_bins, int32_t Kmax,
                               int32_t legs, void* workspace);

/*
 * The chunk plan of a portfolio call on (T_m, B, N, n_bins, K): cohort chunks C in the low 32
 * bits, turnover chunks Ct in the high ones (-1 on bad arguments).  Two calls with the same plan
 * give each panel the same partial sums, so their per-panel results are the same bits.
 */
int64_t csm_portfolio_plan(int32_t T_m, int32_t B, int64_t N, int32_t n_bins, int32_t K);
int csm_portfolio_from_cohorts_grouped(csm_ctx* ctx, int32_t G, const int8_t* L, const double* W,
                                       int32_t T_m, int32_t Bg, int64_t N, int32_t n_bins,
                                       int32_t Kmax, int32_t nK, const int32_t* Ks,
                                       double half_spread, double k_impact, double aum,
                                       const double* ADV, const double* SIG, double* PR,
                                       double* LS, double* TURN, double* COST, double* NET,
                                       void* workspace, int32_t legs, int32_t* need_full);

/*
 * Performance summary per (strategy, panel) of stacked long-short series (LS, and the
 * nullable-together TURN / COST / NET, each [nS][T_m][B]): out [nS][B][7] = months, mean,
 * Sharpe (src/utils.py:8-16 at `freq` periods a year, ddof = 1), mean turnover, mean cost,
 * net mean, net Sharpe; NaN months dropped (run_demo.py:67).
 */
int csm_summary(csm_ctx* ctx, const double* LS, const double* TURN, const double* COST,
                const double* NET, int32_t nS, int32_t T_m, int32_t B, double freq,
                double* out);

/*
 * Daily return series of the decile and long-short portfolios (rule E7 in DESIGN.md section 7,
 * E1 / E2 carried to the days of the holding month; no reference counterpart -- the reference
 * stops at monthly numbers).  Label row t is held over the days d of calendar month t+1,
 * [month_start[t+1], month_start[t+2]).  With pff[d][a] the last non-NaN price of column a in
 * rows <= d (the ABSENT payload counts as NaN) and the base b[t][a] = pff[month_start[t+1]-1][a],
 * a member's value relative is v[d][a] = pff[d][a] / b[t][a].  The cohort of age k (formed at
 * t-k >= 0) and bin q takes the members of E1 -- L[t-k][a] == q, weight 1 or W[t-k][a] when that
 * is finite and > 0, NR[t][a] not NaN -- that also have a finite base > 0; its value is
 * C[d] = sum w v[d] / sum w, V_q[d] is the mean of C[d] over the non-empty cohorts (E2), V_q = 1
 * on the day before the month, and DR[d][q] = V_q[d] / V_q[d-1] - 1.
 *   P [T_d][N], month_start [T_m+1]: the daily panel of csm_month_end / csm_signal
 *   max_month_days: an upper bound of the months' lengths in rows, <= 32
 *   L [T_m][N] int8 labels (-1 = not ranked), NR [T_m][N] next-row returns, W nullable [T_m][N]
 *   n_bins in {2,3,4,5,10,20,30};  1 <= K <= 12;  any N >= 1
 *   DR [T_d][n_bins] out: NaN on the days of month 0 (no portfolio yet), on days outside
 *     [month_start[0], month_start[T_m]) and where the month has no non-empty cohort of the bin
 *   DLS [T_d] out: DR[d][n_bins-1] - DR[d][0], NaN if either leg is (E3's max-minus-min
 *     fallback is not carried over)
 *   DCNT nullable [T_m][K][n_bins] int32 out: the member counts (row T_m-1, never held, is 0)
 *   workspace: device buffer of csm_daily_workspace(T_d, N, T_m, n_bins, K) bytes (0 for
 *     arguments csm_daily_returns refuses)
 * Within a month prod_d (1 + DR[d][q]) = V_q[last day]; on a panel where every cell is priced
 * that is 1 + PR[t][q] of csm_portfolio for the same (L, NR, W, K).  Where prices are missing
 * the monthly engine books a multi-month return at one row while this series carries the
 * position flat until a price appears.  P is read once for any K; every sum has a fixed order,
 * so two calls on the same inputs give the same bits.  +-inf and zero prices are out of contract.
 */
int64_t csm_daily_workspace(int64_t T_d, int64_t N, int32_t T_m, int32_t n_bins, int32_t K);
int csm_daily_returns(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N,
                      const int64_t* month_start, int32_t T_m, int32_t max_month_days,
                      const int8_t* L, const double* NR, const double* W, int32_t n_bins,
                      int32_t K, double* DR, double* DLS, int32_t* DCNT, void* workspace);

/*
 * Statistics of nS series of T entries, element i of series s at X[s + i * stride] (a column of
 * DR: stride = n_bins; DLS: nS = 1, stride = 1).  NaN entries are dropped.  out [nS][6] = count,
 * mean, Sharpe (src/utils.py:8-16 at `freq` periods a year, ddof = 1; NaN when the deviation is
 * 0 or not defined), annualised volatility sd * sqrt(freq), the maximum drawdown of
 * cumprod(1 + x) as a positive fraction of a running peak that starts at 1, and the final
 * cumulative value.  An empty series gives count 0 and NaN elsewhere.
 */
int csm_series_stats(csm_ctx* ctx, const double* X, int32_t nS, int32_t T, int64_t stride,
                     double freq, double* out);

/*
 * Signals that need every day row of the panel (rules D1..D6 in DESIGN.md section 7; no
 * reference counterpart): the 52-week high and volatility-scaled momentum.  A row d of column a
 * is priced when P[d][a] is not NaN (the ABSENT payload counts as NaN); month t covers the rows
 * [month_start[t], month_start[t+1]).  fp64 throughout, every sum sequential in the stated order
 * from 0.0, so two calls, and every launch shape, give the same bits.
 *
 * csm_month_stats (D1): one pass over P; per (month, asset), independent of every other month:
 *   PM  [T_m][N] nullable out: csm_month_end's value -- the last priced row's price, NaN when the
 *       month has a row but no price, ABSENT when it has no row (or no day at all)
 *   P1  [T_m][N] out: the first priced row's price, NaN if none
 *   HI  [T_m][N] out: the maximum over the priced rows, NaN if none
 *   SSW [T_m][N] out, NDW [T_m][N] int32 out: over each pair of consecutive priced rows d' < d of
 *       the month, in day order, r = P[d] / P[d'] - 1, SSW += r * r, NDW += 1 (rows without a
 *       price in between are crossed: one return, booked where the price reappears)
 *   max_month_days: an upper bound of the months' lengths in rows, in [1, 32] (the bound
 *       csm_signal and csm_daily_returns take; a longer month is the caller's breach)
 * Any N >= 1; even N with 16-B aligned P / PM / P1 / HI / SSW and 8-B aligned NDW takes two
 * assets per lane, the same bits.  The launch is (asset slices) x (chunks of consecutive months);
 * "stats_chunks" (csm_tune: 0 auto, one month per chunk | n >= 1 that many chunks, clamped to T_m)
 * only changes how many workgroups there are.  Rows outside
 * [month_start[0], month_start[T_m]) are never read.
 *
 * csm_window_signals (D2..D6): a scan over the months of csm_month_stats's outputs, per asset:
 *   q = the last priced PM of the months before t.  When P1[t] is priced and q is not NaN:
 *       r0 = P1[t] / q - 1, SS[t] = SSW[t] + r0 * r0, ND[t] = NDW[t] + 1 (the month's first
 *       return, added last); else SS = SSW, ND = NDW.  first = the asset's first priced month.
 *   H52[t] = PM[t] / max{HI[j] : t-Jh+1 <= j <= t, HI[j] not NaN}: defined iff PM[t] is priced,
 *       t-Jh+1 >= 0 and first <= t-Jh+1; always <= 1
 *   RV[t] = sqrt(S / n), S = sum SS[j], n = sum ND[j] over j = t-Jv+1 .. t, oldest first: defined
 *       iff t-Jv+1 >= 0, first <= t-Jv+1 and n >= min_obs (month t itself may have no row); the
 *       realised daily volatility, and the SIG input of csm_portfolio's cost model
 *   MS[t] = M[t] / RV[t]: defined iff both are not NaN and RV[t] > 0
 *   NR_H52 / NR_MS: the next return of the signal S = H52 / MS under csm_momentum's rule --
 *       ranked = (PM not ABSENT) and (S not NaN), return over the prices forward-filled within
 *       the ranked subset, settled by the asset's next present row; whole panels only (the last
 *       ranked row's is NaN)
 *   M nullable [T_m][N]: the momentum to scale (csm_momentum's M of any J, skip)
 *   1 <= Jh, Jv <= 36;  min_obs >= 1;  T_m >= 1;  any N >= 1
 *   SS, H52, RV, MS, NR_H52, NR_MS [T_m][N] out, ND [T_m][N] int32 out: NaN where not defined;
 *       every one nullable; MS and NR_MS need M
 * +-inf and zero or negative prices are out of contract.
 */
int csm_month_stats(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N,
                    const int64_t* month_start, int32_t T_m, int32_t max_month_days, double* PM,
                    double* P1, double* HI, double* SSW, int32_t* NDW);
int csm_window_signals(csm_ctx* ctx, const double* PM, const double* P1, const double* HI,
                       const double* SSW, const int32_t* NDW, const double* M, int32_t T_m,
                       int64_t N, int32_t Jh, int32_t Jv, int32_t min_obs, double* SS, int32_t* ND,
                       double* H52, double* RV, double* MS, double* NR_H52, double* NR_MS);

/*
 * Signals of the monthly cross-section (rules B1..B6 in DESIGN.md section 7; no reference
 * counterpart): the equal-weight market return, each asset's market model on it -- beta, alpha,
 * idiosyncratic volatility and residual momentum (Blitz, Huij and Martens 2011) -- and the next
 * return of any signal.  A month price is priced when it is not NaN (the ABSENT payload counts as
 * NaN).  fp64 throughout; every per-asset sum is sequential in the stated order from 0.0, so two
 * calls, and every launch shape, give the same bits.
 *
 * csm_market_factor (B1, B2), PM [T_m][N] (csm_month_end's or csm_month_stats's):
 *   X   [T_m][N] nullable out: x[t] = PM[t] / PM[t-1] - 1 when both calendar-adjacent month
 *       prices are priced, else NaN (x[0] is NaN).  Not csm_momentum's R, which forward-fills over
 *       gaps; on a panel with every cell priced the two are equal bit for bit.
 *   NMK [T_m] int32 nullable out: the assets with an observation in month t
 *   MKT [T_m] out: (sum of x[t] over those assets) / NMK[t] when NMK[t] >= min_assets (>= 1), else
 *       NaN.  The sum's order is a function of N alone (lanes a fixed stride apart, a halving
 *       tree, then slices of 2048 assets in index order): no atomic, and no csm_tune knob
 *       changes it.  |MKT - exact| <= 2^-53 * (sum |x| + |MKT|).
 *
 * csm_market_model (B3..B5) over the Wb calendar months j = t-Wb+1 .. t (t-Wb+1 >= 0), x as above
 * (computed from PM), f = F[j] (F [T_m] on the device: MKT, or any series of the caller's):
 *   observations: the window's months where x[j] and f[j] are both not NaN; n their number
 *   pass 1, oldest first: sx += x, sf += f; mx = sx / n, mf = sf / n
 *   pass 2, oldest first: df = f - mf, dx = x - mx, sff += df * df, sfx += df * dx
 *   BETA[t] = sfx / sff, ALPHA[t] = mx - BETA * mf: defined iff n >= min_obs and sff > 0
 *   NOBS[t] = n (int32; 0 before the first whole window)
 *   e[j] = x[j] - (ALPHA + BETA * f[j]) on the observations, with month t's coefficients
 *   IVOL[t] = sqrt((sum e[j]^2, oldest first) / (n - 2)): defined iff BETA is and n >= 3
 *   RESMOM[t]: over the formation months j = t-skip-J+1 .. t-skip, se = sum e[j] oldest first,
 *       me = se / J, sv = sum (e[j] - me)^2 oldest first, RESMOM = se / sqrt(sv / (J - 1)):
 *       defined iff BETA is, all J formation months are observations, and sv > 0
 *   2 <= Wb <= 60;  min_obs in [2, Wb];  J >= 2, skip >= 0 and J + skip <= Wb, checked only when
 *   RESMOM is requested;  T_m >= 1 (T_m < Wb: nothing is defined);  any N >= 1
 *   BETA, ALPHA, IVOL, RESMOM [T_m][N] out, NOBS [T_m][N] int32 out: NaN where not defined; every
 *       one nullable, at least one given
 * The launch is (64 assets) x (chunks of consecutive months), each chunk starting cold Wb - 1
 * months before its first; "mm_chunks" (csm_tune: 0 auto | n >= 1 that many, clamped to T_m) only
 * changes how many workgroups there are.
 *
 * csm_next_ret (B6): NR [T_m][N] out, the next return of the signal S [T_m][N] under
 * csm_momentum's rule -- ranked = (PM not ABSENT) and (S not NaN), return over the prices
 * forward-filled within the ranked subset, settled by the asset's next present row; whole panels
 * only (the last ranked row's is NaN).  With it csm_deciles and csm_portfolio rank any signal.
 * +-inf and zero or negative prices are out of contract.
 */
int csm_market_factor(csm_ctx* ctx, const double* PM, int32_t T_m, int64_t N, int32_t min_assets,
                      double* X, double* MKT, int32_t* NMK);
int csm_market_model(csm_ctx* ctx, const double* PM, const double* F, int32_t T_m, int64_t N,
                     int32_t Wb, int32_t J, int32_t skip, int32_t min_obs, double* BETA,
                     double* ALPHA, double* IVOL, double* RESMOM, int32_t* NOBS);
int csm_next_ret(csm_ctx* ctx, const double* PM, const double* S, int32_t T_m, int64_t N,
                 double* NR);

/*
 * Signals of the daily returns against a daily market (rules V1..V6 in DESIGN.md section 7; no
 * reference counterpart): the equal-weight daily market, and from each asset's daily market model
 * the daily beta (Frazzini and Pedersen 2014), idiosyncratic volatility (Ang, Hodrick, Xing and
 * Zhang 2006), total volatility, skewness and MAX, the largest daily return (Bali, Cakici and
 * Whitelaw 2011).  Not csm_market_model's BETA / IVOL, which come from monthly returns.  A row is
 * priced when P[d][a] is not NaN (the ABSENT payload counts as NaN).  fp64 throughout, every sum
 * sequential in the stated order from 0.0, so two calls, and every launch shape, give the same
 * bits.
 *
 * The daily return (V1): with d' the latest priced row before d, r[d][a] = P[d][a] / P[d'][a] - 1
 * iff P[d][a] is priced, d' exists and d - d' <= max_gap (panel rows, ABSENT rows included); else
 * there is no observation.  max_gap in [1, 32].  Never month-bounded: a month's first priced day
 * takes its return from the previous month's rows.  On a panel with every cell priced r is
 * pandas' pct_change bit for bit.
 *
 * csm_daily_market (V2), all T_d rows:
 *   NMD  [T_d] int32 nullable out: the assets with an observation on day d
 *   MKTD [T_d] out: (sum of r[d] over those assets) / NMD[d] when NMD[d] >= min_assets (>= 1),
 *        else NaN.  The sum is csm_market_factor's: slices of 2048 assets, a lane's assets 256
 *        apart in order, a 64-wide halving tree, the four waves, then the slices -- a function of
 *        N alone.  |MKTD - exact| <= 2^-53 * (sum |r| + |MKTD|).
 *   workspace: device buffer of csm_daily_market_workspace(T_d, N) bytes (0 for arguments the
 *        call refuses), 8-B aligned, the caller's; T_d <= 2^31 - 1
 *   "dmkt_chunk_days" (csm_tune: 0 auto | n >= 1 day rows per workgroup) only changes how many
 *   workgroups there are.
 *
 * csm_daily_sums (V3): per (month t, asset), over the days d of [month_start[t], month_start[t+1])
 * where r[d][a] and f = FD[d] are both not NaN, in day order from 0:
 *   NO += 1, SR += r, SF += f, SRR += r * r, SFF += f * f, SRF += r * f, SR3 += (r * r) * r,
 *   RMAX = the largest r (NaN if none).  A month without a day gives zeros and a NaN RMAX.
 *   FD [T_d] on the device: MKTD, or any series of the caller's
 *   NO [T_m][N] int32 out; SR, SF, SRR, SFF, SRF [T_m][N] out; SR3, RMAX [T_m][N] nullable out
 *   max_month_days in [1, 32], csm_month_stats's bound
 * Any N >= 1; even N with 16-B aligned P and outputs (8-B NO) takes two assets per lane, the same
 * bits.  "dsums_chunks" (csm_tune: 0 auto | n >= 1 month chunks, clamped to T_m)
 * only changes how many workgroups there are.  No row before month_start[0] - max_gap (clipped to
 * 0) and none at or past month_start[T_m] is read.
 *
 * csm_daily_model (V4) over the Wm calendar months j = t-Wm+1 .. t (t-Wm+1 >= 0): each V3 sum
 * added over j oldest first from 0.0, n the summed NO, nf = (double)n, one rounding per operation:
 *   mr = SR / nf, mf = SF / nf, cff = SFF - SF * mf, crf = SRF - SR * mf, crr = SRR - SR * mr
 *   DBETA = crf / cff: defined iff n >= min_obs and cff > 0
 *   DIVOL = sqrt(max(q, 0) / (nf - 2)), q = crr - DBETA * crf: defined iff DBETA is and n >= 3
 *   DTVOL = sqrt(crr / (nf - 1)): defined iff n >= min_obs, n >= 2 and crr >= 0
 *   DSKEW = m3 / (v * sqrt(v)), v = crr / nf,
 *           m3 = (SR3 - (3 * mr) * SRR + ((2 * SR) * mr) * mr) / nf: defined iff n >= min_obs,
 *           n >= 3 and v > 0
 *   DMAX  = the largest non-NaN RMAX[j] of the window: defined iff n >= min_obs
 *   NOBS  = n (int32; 0 before the first whole window)
 *   1 <= Wm <= 12;  min_obs >= 2 (days);  T_m >= 1;  any N >= 1
 *   DBETA, DIVOL, DTVOL, DSKEW, DMAX [T_m][N] out, NOBS [T_m][N] int32 out: NaN where not
 *       defined; every one nullable, at least one given; DSKEW needs SR3 and DMAX needs RMAX
 *       (nullable inputs otherwise)
 * "dmodel_chunks" (csm_tune: 0 auto, one month per chunk | n >= 1 that many, clamped to T_m) only
 * changes how many workgroups there are; only the sums a requested output depends on are read.  The next return of any of these signals is csm_next_ret's.
 * +-inf and zero or negative prices are out of contract.
 */
int64_t csm_daily_market_workspace(int64_t T_d, int64_t N);
int csm_daily_market(csm_ctx* ctx, const double* P, int64_t T_d, int64_t N, int32_t max_gap,
                     int32_t min_assets, double* MKTD, int32_t* NMD, void* workspace);
int csm_daily_sums(csm_ctx* ctx, const double* P, const double* FD, int64_t T_d, int64_t N,
                   const int64_t* month_start, int32_t T_m, int32_t max_month_days,
                   int32_t max_gap, int32_t* NO, double* SR, double* SF, double* SRR, double* SFF,
                   double* SRF, double* SR3, double* RMAX);
int csm_daily_model(csm_ctx* ctx, const int32_t* NO, const double* SR, const double* SF,
                    const double* SRR, const double* SFF, const double* SRF, const double* SR3,
                    const double* RMAX, int32_t T_m, int64_t N, int32_t Wm, int32_t min_obs,
                    double* DBETA, double* DIVOL, double* DTVOL, double* DSKEW, double* DMAX,
                    int32_t* NOBS);

/*
 * Multi-factor rolling models (rules MF1..MF8 in DESIGN.md section 7; no reference counterpart):
 * the KF-factor form of csm_market_model and of csm_daily_sums / csm_daily_model, 1 <= KF <= 4 --
 * three-factor residual momentum (Blitz, Huij and Martens 2011), idiosyncratic volatility on the
 * three Fama-French factors (Ang, Hodrick, Xing and Zhang 2006), four-factor alphas, and Dimson
 * betas (a regression on the market and its lags).  fp64 throughout; every sum is sequential in the
 * stated order from 0.0 with one rounding per written operation, so two calls, and every launch
 * shape, give the same bits.  Factor panels are row-major with a date's factors adjacent: F
 * [T_m][KF] (monthly), FD [T_d][KF] (daily).  A date where any of the KF values is NaN has no
 * factor row and gives no observation for any asset.
 *
 * The solve (MF3) of A g = b, A symmetric KF x KF (A_ij for i > j means A_ji), sequential LDL^T:
 *   for j = 0 .. KF-1:  d = A_jj, then d = d - (L_jp * L_jp) * D_p for p = 0 .. j-1 ascending;
 *       the cell is undefined unless A_jj > 0 and d > A_jj * 2^-40;  D_j = d;
 *       for i = j+1 .. KF-1:  v = A_ji, then v = v - (L_ip * L_jp) * D_p for p < j ascending,
 *       L_ij = v / D_j
 *   forward: z_j = b_j, then z_j = z_j - L_jp * z_p for p < j ascending
 *   back, j = KF-1 .. 0: g_j = z_j / D_j, then g_j = g_j - L_pj * g_p for p = j+1 .. KF-1 ascending
 *   (KF = 1: g_0 = b_0 / A_00)
 *
 * csm_factor_model (MF1..MF5) over the Wb calendar months j = t-Wb+1 .. t (t-Wb+1 >= 0), x[j] the
 * month return of csm_market_factor's X (computed from PM), f_k = F[j][k]:
 *   observations: the window's months where x[j] is not NaN and month j has a factor row; n their
 *       number;  NOBS[t] = n (int32; 0 before the first whole window)
 *   pass 1, oldest first: sx += x, sf_k += f_k;  mx = sx / n, mf_k = sf_k / n
 *   pass 2, oldest first: dx = x - mx, d_k = f_k - mf_k;  A_jk += d_j * d_k (j <= k),
 *       b_k += d_k * dx, cxx += dx * dx
 *   BETA_k[t] = g_k (MF3);  ALPHA[t] = mx, then ALPHA = ALPHA - g_k * mf_k for k ascending: both
 *       defined iff n >= min_obs and MF3 is defined
 *   fit = ALPHA, then fit = fit + g_k * f_k[j] for k ascending;  e[j] = x[j] - fit, with month t's
 *       coefficients;  se2 = sum e[j]^2 over the observations, oldest first
 *   IVOL[t] = sqrt(se2 / (n - (KF + 1))): defined iff the coefficients are and n >= KF + 2
 *   R2[t] = 1 - se2 / cxx: defined iff the coefficients are and cxx > 0
 *   RESMOM[t]: csm_market_model's RESMOM on these residuals (formation months t-skip-J+1 ..
 *       t-skip, all J observed, sv > 0)
 *   KF + 1 <= Wb <= 60;  min_obs in [KF + 1, Wb];  J >= 2, skip >= 0 and J + skip <= Wb, checked
 *   only when RESMOM is requested;  T_m >= 1;  any N >= 1
 *   BETA [KF][T_m][N] out; ALPHA, IVOL, RESMOM, R2 [T_m][N] out; NOBS [T_m][N] int32 out: NaN where
 *       not defined; every one nullable, at least one given
 * The launch is csm_market_model's; "fm_chunks" (csm_tune: 0 auto | n >= 1 month chunks, clamped to
 * T_m) only changes how many workgroups there are.
 *
 * csm_daily_fsums (MF6): per (month t, asset), over the days d of [month_start[t],
 * month_start[t+1]) where csm_daily_market's r[d][a] is not NaN and day d has a factor row, in day
 * order from 0:  NO += 1, SR += r, SRR += r * r, SF_k += f_k, SRF_k += r * f_k,
 * SFF_p += f_j * f_k for j <= k with p(j, k) = j * KF - j * (j - 1) / 2 + (k - j).
 *   NO [T_m][N] int32 out; SR, SRR [T_m][N] out; SF, SRF [KF][T_m][N] out;
 *   SFF [KF (KF + 1) / 2][T_m][N] out; none nullable.  A month without a day gives zeros.
 *   max_gap, max_month_days and the rows read are csm_daily_sums's.  At KF <= 2 even N with 16-B
 *   aligned P and outputs (8-B NO) takes two assets per lane, as csm_daily_sums; KF >= 3 takes one
 *   (the accumulators of two would leave a SIMD one wave); the same bits either way.
 *   "dfsums_chunks" (csm_tune: 0 auto | n >= 1 month chunks, clamped to T_m) only changes how many
 *   workgroups there are.
 *
 * csm_daily_fmodel (MF7) over the Wm calendar months j = t-Wm+1 .. t (t-Wm+1 >= 0): each MF6 sum
 * added over j oldest first from 0.0, n the summed NO, nf = (double)n:
 *   mr = SR / nf, mf_k = SF_k / nf;  A_jk = SFF_p(j,k) - SF_j * mf_k (j <= k),
 *   b_k = SRF_k - SR * mf_k, crr = SRR - SR * mr
 *   DBETA_k = g_k (MF3): defined iff n >= min_obs and MF3 is defined
 *   DALPHA = mr, then DALPHA = DALPHA - g_k * mf_k for k ascending: defined iff DBETA is
 *   q = crr, then q = q - g_k * b_k for k ascending;  q+ = q < 0 ? 0 : q
 *   DIVOL = sqrt(q+ / (nf - (KF + 1))): defined iff DBETA is and n >= KF + 2
 *   DR2 = 1 - q+ / crr: defined iff DBETA is and crr > 0
 *   NOBS = n (int32; 0 before the first whole window)
 *   1 <= Wm <= 12;  min_obs >= KF + 1 (days);  T_m >= 1;  any N >= 1
 *   DBETA [KF][T_m][N] out; DALPHA, DIVOL, DR2 [T_m][N] out; NOBS [T_m][N] int32 out: NaN where not
 *       defined; every one nullable, at least one given; every input required
 * "dfmodel_chunks" (csm_tune: 0 auto, one month per chunk | n >= 1 that many, clamped to T_m) only
 * changes how many workgroups there are; only the sums a requested output depends on are read.
 *
 * MF8: at KF = 1 with the same F / FD, csm_factor_model gives csm_market_model's BETA, ALPHA, IVOL,
 * RESMOM and NOBS, csm_daily_fsums gives csm_daily_sums's NO, SR, SF, SRR, SFF and SRF, and
 * csm_daily_fmodel gives csm_daily_model's DBETA, DIVOL and NOBS, all bit for bit.
 * +-inf and zero or negative prices are out of contract.
 */
int csm_factor_model(csm_ctx* ctx, const double* PM, const double* F, int32_t T_m, int64_t N,
                     int32_t KF, int32_t Wb, int32_t J, int32_t skip, int32_t min_obs,
                     double* BETA, double* ALPHA, double* IVOL, double* RESMOM, double* R2,
                     int32_t* NOBS);
int csm_daily_fsums(csm_ctx* ctx, const double* P, const double* FD, int64_t T_d, int64_t N,
                    int32_t KF, const int64_t* month_start, int32_t T_m, int32_t max_month_days,
                    int32_t max_gap, int32_t* NO, double* SR, double* SRR, double* SF, double* SRF,
                    double* SFF);
int csm_daily_fmodel(csm_ctx* ctx, const int32_t* NO, const double* SR, const double* SRR,
                     const double* SF, const double* SRF, const double* SFF, int32_t T_m,
                     int64_t N, int32_t KF, int32_t Wm, int32_t min_obs, double* DBETA,
                     double* DALPHA, double* DIVOL, double* DR2, int32_t* NOBS);

/*
 * Liquidity signals from the daily price and volume panels (rules Q1..Q6 in DESIGN.md section 7; no
 * reference counterpart): Amihud's (2002) ILLIQ, the mean of |daily return| / daily dollar volume;
 * the dollar average daily volume csm_portfolio's ADV takes; turnover; and the shares of
 * zero-return days (Lesmond, Ogden and Trzcinka 1999) and zero-volume days.  fp64 throughout, every
 * sum sequential in day (then month) order from 0.0 with one rounding per written operation, so two
 * calls, and every launch shape, give the same bits.
 *
 * Q1: P, V [T_d][N].  v[d][a] = V[d][a], a NaN taken as 0.0 (csm_month_end's rule).  A day is
 * priced when P[d][a] is not NaN (the ABSENT payload counts as NaN); on a priced day dv = P * v, one
 * multiply.  r[d][a] is csm_daily_market's daily return (V1) with max_gap in [1, 32].  Volume on an
 * unpriced day is ignored.  Negative or +-inf volume and +-inf or non-positive prices are out of
 * contract.
 *
 * csm_liq_sums (Q2): per (month t, asset), over the days d of [month_start[t], month_start[t+1]) in
 * day order from 0:
 *   priced day:                       NP += 1, SV += v, SDV += dv, NZV += (v == 0)
 *   return day (r not NaN):           ND += 1, NZR += (r == 0.0)
 *   Amihud day (r not NaN, dv > 0):   NA += 1, SIL += fabs(r) / dv
 *   NP, ND, NA [T_m][N] int32 out; SDV, SIL [T_m][N] out; NZR, NZV [T_m][N] int32 and SV [T_m][N]
 *   nullable out.  A month without a day gives zeros.
 *   max_month_days in [1, 32], csm_month_stats's bound
 * Any N >= 1, one asset per lane; under csm_tune "lsums_pair" = 1 even N with 16-B aligned P, V and
 * f64 outputs and 8-B aligned int32 outputs takes two assets per lane (it measured a few per cent
 * slower, so it is not the default), the same bits.  "lsums_chunks" (csm_tune: 0 auto | n >= 1
 * month chunks, clamped to T_m) only changes how many workgroups there are.  No row before month_start[0] - max_gap
 * (clipped to 0) and none at or past month_start[T_m] is read, from either panel; the rows before
 * month_start[0] are read from P only.
 *
 * csm_liq_model (Q3) over the Wm calendar months j = t-Wm+1 .. t (t-Wm+1 >= 0): each Q2 value added
 * over j oldest first from zero into np, nd, na, nzr, nzv, sv, sdv, sil; counts enter the
 * arithmetic as (double):
 *   ILLIQ = (sil / na) * scale: defined iff na >= min_obs;  scale finite and positive
 *   DVOL  = sdv / np: defined iff np >= min_obs (the dollar ADV of csm_portfolio's ADV)
 *   TURN  = (sv / np) / SH[t][a]: defined iff np >= min_obs and SH[t][a] > 0
 *   ZRET  = nzr / nd: defined iff nd >= min_obs
 *   ZVOL  = nzv / np: defined iff np >= min_obs
 *   NOBS  = na (int32; 0 before the first whole window)
 *   1 <= Wm <= 12;  min_obs >= 1 (days);  T_m >= 1;  any N >= 1
 *   SH [T_m][N] nullable in: shares outstanding (csm_turnover_features' SH, for instance)
 *   ILLIQ, DVOL, TURN, ZRET, ZVOL [T_m][N] out, NOBS [T_m][N] int32 out: NaN where not defined;
 *       every one nullable, at least one given; TURN needs SV and SH, ZRET needs NZR and ZVOL needs
 *       NZV (nullable inputs otherwise)
 * "lmodel_chunks" (csm_tune: 0 auto, one month per chunk | n >= 1 that many, clamped to T_m) only
 * changes how many workgroups there are; only the panels a requested output depends on are read.
 * There is no log(1 + ILLIQ) output: ranks do not change under it.  The next return of any of these
 * signals is csm_next_ret's (Q4).
 */
int csm_liq_sums(csm_ctx* ctx, const double* P, const double* V, int64_t T_d, int64_t N,
                 const int64_t* month_start, int32_t T_m, int32_t max_month_days, int32_t max_gap,
                 int32_t* NP, int32_t* ND, int32_t* NA, int32_t* NZR, int32_t* NZV, double* SV,
                 double* SDV, double* SIL);
int csm_liq_model(csm_ctx* ctx, const int32_t* NP, const int32_t* ND, const int32_t* NA,
                  const int32_t* NZR, const int32_t* NZV, const double* SV, const double* SDV,
                  const double* SIL, const double* SH, int32_t T_m, int64_t N, int32_t Wm,
                  int32_t min_obs, double scale, double* ILLIQ, double* DVOL, double* TURN,
                  double* ZRET, double* ZVOL, int32_t* NOBS);

/*
 * Range-based signals from the daily high, low and close panels (rules HL1..HL6 in DESIGN.md
 * section 7; no reference counterpart): Parkinson's (1980) range volatility, Corwin and Schultz's
 * (2012) high-low bid-ask spread, zero-floored per pair, and Abdi and Ranaldo's (2017)
 * close-high-low spread.  fp64 without contraction, every sum sequential in day (then month) order
 * from 0.0, so two calls, and every launch shape, give the same bits.  log and exp are the device
 * library's (OCML), so the sums are not bit-comparable with another libm's.
 *
 * HL1: H, L, C [T_d][N], raw (unadjusted) prices on one scale.  Row d of asset a is ranged iff
 * H, L, C are all not NaN (the ABSENT payload counts as NaN), L > 0, H >= L and L <= C <= H; any
 * other row is skipped and changes no state.  +-inf prices are out of contract.
 * HL2: h = log(H), l = log(L), c = log(C), u = h - l, eta = (h + l) * 0.5.
 * HL3: d' = the asset's previous ranged row; (d', d) is a pair iff d - d' <= max_gap (panel rows,
 * max_gap in [1, 32]), booked in the month that holds d; never month-bounded.
 * HL4, per pair: s = L_d > C_d' ? L_d - C_d' : (H_d < C_d' ? H_d - C_d' : 0.0); H* = H_d - s,
 * L* = L_d - s, h* = log(H*), l* = log(L*); beta = u_d' u_d' + (h* - l*)(h* - l*);
 * hh = H_d' >= H* ? h_d' : h*, ll = L_d' <= L* ? l_d' : l*, gamma = (hh - ll)(hh - ll);
 * k = 3.0 - 2.0 sqrt(2.0); alpha = (sqrt(2.0 beta) - sqrt(beta)) / k - sqrt(gamma / k);
 * e = exp(alpha); S = 2.0 (e - 1.0) / (1.0 + e).  A NaN S (L* <= 0) contributes nothing.
 *
 * csm_range_sums (HL5): per (month t, asset), over the days d of [month_start[t], month_start[t+1])
 * in day order from 0:
 *   ranged day:            NRG += 1, SPK += u * u
 *   pair:                  NPR += 1, SAR += (c_d' - eta_d') * (c_d' - eta_d)
 *   pair with S not NaN:   NCS += 1, SCS += S < 0 ? 0.0 : S
 *   NRG, NPR [T_m][N] int32 out; SPK [T_m][N] out; NCS [T_m][N] int32 and SCS [T_m][N] nullable
 *   out, together (without them no pair's two logs, exp and three square roots are computed); SAR
 *   [T_m][N] nullable out.  A month without a day gives zeros.
 *   max_month_days in [1, 32], csm_month_stats's bound
 * Any N >= 1, one asset per lane.  "rsums_chunks" (csm_tune: 0 auto | n >= 1 month chunks, clamped
 * to T_m) only changes how many workgroups there are.  No row before month_start[0] - max_gap
 * (clipped to 0) and none at or past month_start[T_m] is read.
 *
 * csm_range_model (HL6) over the Wm calendar months j = t-Wm+1 .. t (t-Wm+1 >= 0): each HL5 value
 * added over j oldest first from zero into nrg, npr, ncs, spk, scs, sar; counts enter the
 * arithmetic as (double):
 *   PKVOL = sqrt(spk / (c4 * nrg)): defined iff nrg >= min_obs; the daily volatility, c4 = 4 ln 2
 *           from the caller (finite and positive)
 *   CSSPR = scs / ncs: defined iff ncs >= min_obs
 *   ARSPR = m > 0 ? 2.0 * sqrt(m) : 0.0, m = sar / npr: defined iff npr >= min_obs
 *   NOBS  = npr (int32; 0 before the first whole window)
 *   1 <= Wm <= 12;  min_obs >= 1 (days);  T_m >= 1;  any N >= 1
 *   PKVOL, CSSPR, ARSPR [T_m][N] out, NOBS [T_m][N] int32 out: NaN where not defined; every one
 *       nullable, at least one given; CSSPR needs NCS and SCS and ARSPR needs SAR (nullable inputs
 *       otherwise)
 * "rmodel_chunks" (csm_tune: 0 auto, one month per chunk | n >= 1 that many, clamped to T_m) only
 * changes how many workgroups there are; only the panels a requested output depends on are read.
 * The next return of any of these signals is csm_next_ret's.
 */
int csm_range_sums(csm_ctx* ctx, const double* H, const double* L, const double* C, int64_t T_d,
                   int64_t N, const int64_t* month_start, int32_t T_m, int32_t max_month_days,
                   int32_t max_gap, int32_t* NRG, int32_t* NPR, int32_t* NCS, double* SPK,
                   double* SCS, double* SAR);
int csm_range_model(csm_ctx* ctx, const int32_t* NRG, const int32_t* NPR, const int32_t* NCS,
                    const double* SPK, const double* SCS, const double* SAR, int32_t T_m, int64_t N,
                    int32_t Wm, int32_t min_obs, double c4, double* PKVOL, double* CSSPR,
                    double* ARSPR, int32_t* NOBS);

/*
 * Asymmetry signals of the daily returns (rules AS1..AS7 in DESIGN.md section 7; no reference
 * counterpart): the information discreteness of Da, Gurun and Warachka (2014), the signed jump
 * variation RSJ and the downside semi-volatility (Barndorff-Nielsen, Kinnebrock and Shephard 2010;
 * Bollerslev, Li and Zhao 2020), and the downside (or upside) beta (Bawa and Lindenberg 1977; Ang,
 * Chen and Xing 2006).  fp64 without contraction, every sum sequential in day (then month) order
 * from zero with one rounding per written operation, so two calls, and every launch shape, give the
 * same bits.
 *
 * AS1: P [T_d][N]; r[d][a] is csm_daily_market's daily return (V1) with max_gap in [1, 32].
 * FD [T_d] nullable in: f = FD[d], which may be NaN (csm_daily_market's MKTD, or any series).
 * side is -1 or +1: day d is on the side iff f < 0 (side -1) or f > 0 (side +1).
 *
 * csm_asym_sums (AS2): per (month t, asset), over the days d of [month_start[t], month_start[t+1])
 * in day order from zero, rr = r * r:
 *   return day (r not NaN):                    ND += 1
 *   r > 0:                                     NUP += 1, SUP += rr
 *   r < 0:                                     NDN += 1, SDN += rr   (a zero return: ND only)
 *   side day (r, f not NaN, f on the side):    NB += 1, BR += r, BF += f, BFF += f * f, BRF += r * f
 *   ND, NUP, NDN [T_m][N] int32 out; SUP, SDN [T_m][N] out.  NB [T_m][N] int32 and BR, BF, BFF, BRF
 *   [T_m][N] out are given if and only if FD is (CSM_E_INVAL otherwise).  A month without a day
 *   gives zeros.
 *   max_month_days in [1, 32], csm_month_stats's bound
 * Any N >= 1, one asset per lane; under csm_tune "asums_pair" = 2 even N with a 16-B aligned P and
 * f64 outputs and 8-B aligned int32 outputs takes two assets per lane (it measured slower, so it is
 * not the default), the same bits.  "asums_chunks" (csm_tune: 0 auto | n >= 1 month chunks, clamped to T_m) only changes how
 * many workgroups there are.  No row before month_start[0] - max_gap (clipped to 0) and none at or
 * past month_start[T_m] is read.
 *
 * csm_asym_model (AS3) over the Wm calendar months j = t-skip-Wm+1 .. t-skip (t-skip-Wm+1 >= 0):
 * each AS2 value added over j oldest first from zero into nd, nup, ndn, sup, sdn, nb, br, bf, bff,
 * brf; counts enter the arithmetic as (double):
 *   ID     = q if m > 0, -q if m < 0, 0.0 if m == 0, NaN if m is NaN, with q = (ndn - nup) / nd and
 *            m = M[t][a], the caller's formation return (mom_J with J = Wm and the same skip):
 *            defined iff nd >= min_obs
 *   RSJ    = (sup - sdn) / (sup + sdn): defined iff nd >= min_obs and sup + sdn > 0
 *   DSVOL  = sqrt(sdn / nd): defined iff nd >= min_obs
 *   DNBETA = crf / cff, mf = bf / nb, cff = bff - bf * mf, crf = brf - br * mf (csm_daily_model's
 *            form): defined iff nb >= min_side and cff > 0
 *   NOBS   = nd, NSIDE = nb (int32; 0 before the first whole window)
 *   1 <= Wm <= 36;  0 <= skip <= 12;  min_obs >= 1, min_side >= 2 (days);  T_m >= 1;  any N >= 1
 *   M [T_m][N] nullable in; NB, BR, BF, BFF, BRF nullable in, together
 *   ID, RSJ, DSVOL, DNBETA [T_m][N] out, NOBS, NSIDE [T_m][N] int32 out: NaN where not defined;
 *       every one nullable, at least one given; ID needs M, DNBETA and NSIDE need the five side
 *       panels
 * "amodel_chunks" (csm_tune: 0 auto, one month per chunk | n >= 1 that many, clamped to T_m) only
 * changes how many workgroups there are; only the panels a requested output depends on are read.
 * The next return of any of these signals is csm_next_ret's (AS4).
 */
int csm_asym_sums(csm_ctx* ctx, const double* P, const double* FD, int64_t T_d, int64_t N,
                  const int64_t* month_start, int32_t T_m, int32_t max_month_days, int32_t max_gap,
                  int32_t side, int32_t* ND, int32_t* NUP, int32_t* NDN, double* SUP, double* SDN,
                  int32_t* NB, double* BR, double* BF, double* BFF, double* BRF);
int csm_asym_model(csm_ctx* ctx, const int32_t* ND, const int32_t* NUP, const int32_t* NDN,
                   const double* SUP, const double* SDN, const int32_t* NB, const double* BR,
                   const double* BF, const double* BFF, const double* BRF, const double* M,
                   int32_t T_m, int64_t N, int32_t Wm, int32_t skip, int32_t min_obs,
                   int32_t min_side, double* ID, double* RSJ, double* DSVOL, double* DNBETA,
                   int32_t* NOBS, int32_t* NSIDE);

/*
 * Fama-MacBeth (1973) cross-sectional regressions (rules R1..R6 in DESIGN.md section 7; the
 * reference's StandardScaler + Ridge, src/models.py:8-22, is the standardize = 1, ridge > 0 case
 * applied to one month's cross-section).  fp64 throughout, every sum in a stated order, so two
 * calls, and every launch shape, give the same bits.
 *
 * csm_xs_regress: month t's regression of Y[t] on S_0[t] .. S_{K-1}[t] across the assets.
 *   Y [T_m][N]; S a HOST array of K device pointers, each [T_m][N] (1 <= K <= 8); W [T_m][N]
 *   nullable weights.  Asset a is an observation of month t iff Y and every S_k are not NaN (the
 *   ABSENT payload counts as NaN) and, with W, W is not NaN and > 0.  Months are independent.
 *   R1  every sum over the assets: non-observations add 0.0; slices of 2048 assets; lane l of 256
 *       adds assets 2048 i + l + 256 k, k = 0..7, in k order from 0.0; each 64 consecutive lanes by
 *       a halving tree (h = 32..1: element j < h += element j + h); the four wave sums in order
 *       from 0.0; the slice sums in order from 0.0.  A function of N alone: no atomic, no knob.
 *   R2  w = 1.0 without W.  n = observations = NOBS[t] (int32, nullable, written for every month);
 *       sw = sum w, sy = sum w * y, ss_k = sum w * s_k; my = sy / sw, ms_k = ss_k / sw.
 *       n < min_obs (min_obs >= K + 2): every float output of the month is NaN.
 *   R3  dy = y - my, d_k = s_k - ms_k; C_jk = sum (w * d_j) * d_k (j <= k), c_k = sum (w * d_k) * dy,
 *       cyy = sum (w * dy) * dy.  The month is undefined unless every C_kk > 0 and cyy > 0.
 *   R4  standardize: sd_k = sqrt(C_kk / sw), A0_jk = C_jk / (sd_j * sd_k), b_k = c_k / sd_k (the
 *       population z-score); else A0 = C, b = c.  A = A0 with A_kk = A0_kk + ridge (ridge >= 0).
 *   R5  one lane, sequentially.  Cholesky, j = 0..K-1: d = A_jj, d = d - L_jp * L_jp (p < j
 *       ascending); undefined unless d > A_jj * 2^-40; L_jj = sqrt(d); for i > j: v = A_ij,
 *       v = v - L_ip * L_jp (p < j ascending), L_ij = v / L_jj.  Forward: z_j = (b_j - s) / L_jj,
 *       s = sum_{p<j} L_jp * z_p ascending from 0.0.  Back, j = K-1..0: g_j = (z_j - s) / L_jj,
 *       s = sum_{p>j} L_pj * g_p ascending from 0.0.  Intercept: g0 = my standardised, else
 *       g0 = my, g0 = g0 - g_k * ms_k in k order.  Fit: gb = sum g_j * b_j, gAg = sum_j g_j *
 *       (sum_k A0_jk * g_k), each ascending from 0.0; rss = (cyy - 2.0 * gb) + gAg;
 *       R2 = 1.0 - rss / cyy.
 *   GAMMA [T_m][K + 1] out = (g0, g_0 .. g_{K-1}); R2 [T_m] nullable out; NaN where undefined.
 *   CSM_E_INVAL: K outside [1, 8], min_obs < K + 2, ridge < 0 or not finite, a NULL Y / S / S[k] /
 *   GAMMA, T_m < 1, N < 1, T_m * N > 2^40.  +-inf in the data is out of contract.
 * *
 * csm_newey_west (R6): per column c of G (entry i at G[i * ld + c], ld >= C), the non-NaN entries
 * in time order x_1 .. x_n (gaps closed): NT = n (int32); MEAN = (sum x in order from 0.0) / n
 * (NaN when n = 0); u_i = x_i - MEAN; a_l = (sum_{i>l} u_i * u_{i-l}, i ascending) / n for
 * l = 0..lags; var = a_0, then var += (2.0 * (1.0 - l / (lags + 1.0))) * a_l, l ascending (the
 * Bartlett kernel, 1/n scaling, no small-sample correction); SE = sqrt(var / n), TSTAT = MEAN / SE,
 * both defined iff n >= lags + 2 and var > 0.  MEAN [C] out; SE, TSTAT [C], NT [C] int32 nullable.
 * T, C >= 1; lags >= 0.
 */
int csm_xs_regress(csm_ctx* ctx, const double* Y, const double* const* S, int32_t K,
                   const double* W, int32_t T_m, int64_t N, int32_t standardize, double ridge,
                   int32_t min_obs, double* GAMMA, double* R2, int32_t* NOBS);
int csm_newey_west(csm_ctx* ctx, const double* G, int32_t T, int32_t C, int64_t ld, int32_t lags,
                   double* MEAN, double* SE, double* TSTAT, int32_t* NT);

/*
 * Within-group sorts (rules N1..N6 in DESIGN.md section 7): the reference's
 * groupby(['date', 'group'])['mom_J'].transform(assign_deciles_per_date) -- sector-neutral deciles
 * (Moskowitz-Grinblatt 1999), and with a first sort's labels as the groups the dependent double
 * sort -- and the groups' statistics with the industry-adjusted signals.  The cost per date is a
 * fixed number of sweeps of the row, whatever n_groups is.
 *   S [T_m][N] the signal (NaN, the ABSENT payload included: not ranked);  GID int16, row t at
 *   GID + t * g_ld: g_ld = N one row per month, g_ld = 0 one static row;  1 <= n_groups <= 256.
 *   N1  cell (t, a) is a member of group g = GID[t * g_ld + a] iff 0 <= g < n_groups and S[t][a]
 *       is not NaN; any other id means no group (ids are device data: never an error).
 *   N2  L [T_m][N] int8 out: per (t, g) csm_deciles's rule (qtable, n_bins as there: 1..20 without
 *       NR, 2/3/4/5/10/20 with) on the members' values alone; -1 outside every group and for every
 *       member of a group with fewer than min_group (>= 1) members at t.  A group of one value or
 *       of equal values is all -1; two distinct values get 0 and n_bins - 1.
 *   N3  with NR [T_m][N] (nullable): SUMG[t][g][d] = the sum of NR over the members of (t, g) with
 *       label d and a non-NaN NR, CNTG their count.  The members of a segment stand in asset
 *       order at positions 0..n-1; lane l of 64 adds positions l, l + 64, ... from 0.0 (0.0 for a
 *       position of another label), the lanes by a halving tree (h = 32..1: element j < h +=
 *       element j + h): a function of the group's size alone.  EWG [T_m][n_groups][n_bins] = SUMG
 *       / CNTG (NaN where empty); EW [T_m][n_bins] = (SUMG added over g ascending from 0.0) /
 *       (CNTG added over g) = CNT; NV [T_m] the members of the date, NVG [T_m][n_groups] of the
 *       group, labelled or not.  EW, CNT, NV, EWG, CNTG, NVG nullable; csm_long_short on EW / CNT
 *       gives the neutral long-short.
 *   N6  NR is the caller's: the next return of S itself (csm_signal, csm_next_ret) is the right
 *       one -- the reference computes next_ret on the rows with a valid signal and drops the rows
 *       without a decile afterwards (run_demo.py:41-49), so cells without a group simply drop out
 *       of the means.
 * "gdec_small_cap" (csm_tune, 1..4096) moves the segment length at which the LDS sort hands over
 * to the tiled one, here, in csm_xs_rank, csm_rank_ic and csm_deciles_bp; labels, counts, sums,
 * ranks and edges do not depend on it.
 *
 * csm_group_stats: N4  GCNT [T_m][n_groups] int32 the member count n; GMEAN = (sum of S over the
 *       members) / n, NaN for n = 0: lane l of 256 adds positions l, l + 256, ... from 0.0, each
 *       wave by the halving tree, the four wave sums in order from 0.0;  GSD = sqrt((sum of
 *       (s - GMEAN)^2, the same order) / (n - 1)), NaN for n < 2.
 *   N5  per member cell SA = S - GMEAN, SZ = SA / GSD (NaN where GSD is NaN or 0), SB = GMEAN;
 *       NaN in every other cell.  GMEAN, GSD, GCNT, SA, SZ, SB nullable: only those given are
 *       written.
 * CSM_E_INVAL: n_groups outside [1, 256], g_ld not 0 or N, min_group < 1, a NULL S / GID / L /
 * qtable, an n_bins csm_deciles refuses, T_m < 1, N < 1 or N >= 2^31, T_m * N > 2^40.  Scratch
 * (13 B per cell) is the context's.
 */
int csm_group_deciles(csm_ctx* ctx, const double* S, const double* NR, const int16_t* GID,
                      int64_t g_ld, int32_t T_m, int64_t N, int32_t n_groups, int32_t n_bins,
                      const double* qtable, int32_t min_group, int8_t* L, double* EW, int32_t* CNT,
                      int32_t* NV, double* EWG, int32_t* CNTG, int32_t* NVG);
int csm_group_stats(csm_ctx* ctx, const double* S, const int16_t* GID, int64_t g_ld, int32_t T_m,
                    int64_t N, int32_t n_groups, double* GMEAN, double* GSD, int32_t* GCNT,
                    double* SA, double* SZ, double* SB);

/*
 * Cross-sectional ranks and information coefficients (rules I1..I6 in DESIGN.md section 7):
 * pandas' rank(axis=1, method='average' | 'min' | 'max', pct=...) per date or per (date, group),
 * and the per-month Spearman and Pearson correlation of a signal with a later return (scipy's
 * spearmanr, pandas' corr(method='spearman')).  Ranks are integers or half-integers and the
 * Spearman sums are integers, so both are functions of the data alone: no tolerance.
 * method='first' and 'dense' are not offered: a stable order needs a (key, index) pair sort and
 * dense ranks a distinct-count scan, neither is needed for the IC, and the reference's 'first'
 * fallback (run_demo.py:25-29) is unreachable for finite input.
 *
 * csm_xs_rank:  S [T_m][N]; GID, g_ld, n_groups as csm_group_deciles.
 *   I1  membership is rule N1.  GID == NULL is allowed with n_groups == 1 only: every non-NaN
 *       cell is a member of group 0.  Non-members get NaN in RANK [T_m][N]; NVG [T_m][n_groups]
 *       int32 (nullable) receives the member counts.
 *   I2  a member with value x in a segment of n members: lt = the members with value < x, le =
 *       those with value <= x (-0.0 and 0.0 tie).  method 0 (average) = (lt + le + 1) / 2.0,
 *       1 (min) = lt + 1, 2 (max) = le; with pct != 0 that rank divided by (double)n, one fp64
 *       division (pandas' rank(pct=True)).
 *   CSM_E_INVAL as csm_group_stats, plus: a method outside 0..2, a NULL S or RANK, GID == NULL with
 *   n_groups != 1.  "gdec_small_cap" moves the LDS / tiled hand-over here too; the output does not
 *   depend on it.
 *
 * csm_rank_ic:  S, Y [T_m][N].
 *   I3  month t pairs S[t][a] with Y[t + lead][a], lead >= 0; asset a is an observation iff both
 *       are not NaN; n = NOBS[t] their number.  Months with t + lead >= T_m have NOBS = 0 and NaN
 *       outputs.  Ranks are taken inside the joint observation set, not over S alone.
 *   I4  with lt, le as in I2 over the observations, a = lt_s + le_s - n (= 2 rank - (n + 1), an
 *       integer) and b likewise from Y; Sab = sum a * b, Saa = sum a * a, Sbb = sum b * b in
 *       int64 (|a| < n <= 2^20: exact in any order).  RIC = (double)Sab / sqrt((double)Saa *
 *       (double)Sbb), each conversion rounding once; defined iff n >= min_obs, Saa > 0, Sbb > 0.
 *   I5  the observations stand in asset order at positions 0..n-1; every sum in N4's order (lane l
 *       of 256 adds positions l, l + 256, ... from 0.0, each wave by the halving tree, the four
 *       wave sums in order from 0.0).  ms = (sum s) / n, my = (sum y) / n; ds = s - ms, dy = y - my;
 *       css = sum ds * ds, cyy = sum dy * dy, csy = sum ds * dy; PIC = csy / sqrt(css * cyy),
 *       defined iff n >= min_obs, css > 0, cyy > 0.  A function of n alone: no atomic.
 *   I6  RIC, PIC [T_m] out, NOBS [T_m] int32 out, each nullable, RIC or PIC required; NOBS is
 *       written for every month.  Scratch (20 B per cell) is the context's.
 *   CSM_E_INVAL: a NULL S or Y, RIC and PIC both NULL, T_m < 1, N < 1, N > 2^20, lead < 0,
 *   min_obs < 2.  +-inf in the data is out of contract.
 */
int csm_xs_rank(csm_ctx* ctx, const double* S, const int16_t* GID, int64_t g_ld, int32_t T_m,
                int64_t N, int32_t n_groups, int32_t method, int32_t pct, double* RANK,
                int32_t* NVG);
int csm_rank_ic(csm_ctx* ctx, const double* S, const double* Y, int32_t T_m, int64_t N,
                int32_t lead, int32_t min_obs, double* RIC, double* PIC, int32_t* NOBS);

/*
 * Reference-universe breakpoints and universe screens (rules U1..U6 in DESIGN.md section 7): the
 * qcut edges of each date taken from a subset of its cells -- NYSE breakpoints -- and every ranked
 * cell of the date (NYSE, AMEX, Nasdaq) assigned to those bins; the edges themselves; and the
 * price / size screen of the momentum papers (Jegadeesh-Titman 2001: no stock under $5, none under
 * the smallest NYSE size decile).
 *
 * csm_deciles_bp:  M [T_m][N] the signal, NR [T_m][N] (nullable), BP uint8 with row t at
 *   BP + t * bp_ld: bp_ld = N one row per month, bp_ld = 0 one static row.
 *   U1  the ranked set of date t is the cells whose M[t][a] is not NaN (the ABSENT payload is a
 *       NaN); the breakpoint set is the ranked cells with BP[t * bp_ld + a] != 0.  Every byte value
 *       is data, never an error.
 *   U2  edges: csm_deciles's rule (qtable, the fp64 lerp without FMA) on the breakpoint set's values
 *       alone, the distinct edges kept in order.  EDGES [T_m][n_bins + 1]: the NE[t] distinct edges
 *       first, NaN after them; NE [T_m] int32; NVB [T_m] int32 the size of the breakpoint set.
 *       -0.0 and 0.0 count as equal.
 *   U3  NE[t] < 2 (the subset is empty, has one value, or all its values are equal): every label
 *       of the date is -1.  Otherwise a ranked cell with value x gets #{k in 1..NE-2 : e_k < x},
 *       an int8 in [0, NE - 2] -- pandas' cut(x, edges, include_lowest=True) inside [e_0, e_last],
 *       bin 0 below e_0 and bin NE - 2 above e_last.  Non-ranked cells get -1.  With BP all ones
 *       and n_bins >= 2 the labels are csm_deciles's.
 *   U4  with NR: EW [T_m][n_bins] the mean of NR over the cells with label d and a non-NaN NR,
 *       CNT their count, NV [T_m] the ranked cells.  Lane l of 1024 adds its cells l, l + 1024, ...
 *       in ascending order from 0.0; each of the 16 waves adds its lanes by the halving tree
 *       (h = 32..1: element j < h += element j + h); the wave sums are added in wave order from
 *       0.0: a function of N alone.  No floating-point atomic: two calls give the same bits.
 *   U6  NR is the caller's, as rule N6: the next return of the signal itself.  A screened-out cell
 *       simply drops from the means.
 *   n_bins 1..20 without NR, 2/3/4/5/10/20 with.  L, EW, CNT, NV, NVB, EDGES, NE are each
 *   nullable; L or EDGES is required; with L, NV, EW and CNT all NULL only the edges are computed.
 *   CSM_E_INVAL: a NULL M, BP or qtable, L and EDGES both NULL, bp_ld not 0 or N, an n_bins
 *   csm_deciles refuses, T_m < 1, N < 1 or N >= 2^31, T_m * N > 2^40.  Scratch (8 B per cell) is
 *   the context's group workspace.  "gdec_small_cap" moves the LDS / tiled hand-over of the
 *   breakpoint set's sort too; the edges do not depend on it.
 *
 * csm_screen:  U5  a cell of M [T_m][N] is kept iff M[t][a] is not NaN, and PM is NULL or
 *   PM[t][a] >= min_price (a NaN or ABSENT PM fails), and CAP is NULL or CAP[t][a] >= CAPMIN[t]
 *   (a NaN on either side fails the cell).  MS [T_m][N] = M where kept, NaN elsewhere; KEPT [T_m]
 *   int32 (nullable) the kept cells.  The screen never changes NR.  CSM_E_INVAL: a NULL M or MS,
 *   CAP given with a NULL CAPMIN, the size limits above.
 * +-inf in the data is out of contract.
 */
int csm_deciles_bp(csm_ctx* ctx, const double* M, const double* NR, const uint8_t* BP,
                   int64_t bp_ld, int32_t T_m, int64_t N, int32_t n_bins, const double* qtable,
                   int8_t* L, double* EW, int32_t* CNT, int32_t* NV, int32_t* NVB, double* EDGES,
                   int32_t* NE);
int csm_screen(csm_ctx* ctx, const double* M, const double* PM, double min_price,
               const double* CAP, const double* CAPMIN, int32_t T_m, int64_t N, double* MS,
               int32_t* KEPT);

/*
 * Stationary month bootstrap (BASELINE config C5; rule E6): panels b0 .. b0+B-1 of the base
 * month-return panel R[T_m][N] (csm_momentum's R; NaN = no row).  src[B][T_m] int32 out: the
 * source months; PMb[T_m][B][N] out: month prices p0 * prod(1 + r) over the resampled months,
 * ABSENT where the source return is NaN.  The random stream is splitmix64 keyed by
 * (seed, panel, month), so panel b is the same on every device and shard.
 */
int csm_bootstrap(csm_ctx* ctx, const double* R, int32_t T_m, int64_t N, int32_t B, int64_t b0,
                  uint64_t seed, double mean_block, double p0, int32_t* src, double* PMb);

/*
 * csm_bootstrap fused into csm_momentum_multi_ids for the bootstrap sweep (C5): the resampled
 * prices are generated in registers from R (csm_bootstrap's arithmetic, never written), scanned
 * for every J of Js in one pass, and written as M[nJ] (+ IDS[nJ], nullable) equal bit for bit to
 * csm_momentum_multi_ids on csm_bootstrap's panel, plus ONE next_ret panel NR [T_m][B][N] shared
 * by every J: equal to each J's next_ret on every row that J ranks (all the portfolio reads).
 *   src [B][T_m] out (as csm_bootstrap);  M[q] / IDS[q] / NR [T_m][B][N] out;
 *   bad: device int32, set to 1 when a generated price is not finite and non-zero (the shared
 *   next_ret is then not exact: rerun the batch on the csm_bootstrap path).
 * N even, 1 <= nJ <= 4, J + skip <= 16, 16-B aligned R / M / NR, 4-B aligned ids.
 */
int csm_boot_scan(csm_ctx* ctx, const double* R, int32_t T_m, int64_t N, int32_t B, int64_t b0,
                  uint64_t seed, double mean_block, double p0, const int32_t* Js, int32_t nJ,
                  int32_t skip, int32_t* src, double* const* M, uint16_t* const* IDS, double* NR,
                  int32_t* bad);

/*
 * Share-turnover features, replacing src/features.py:60-107 (compute_monthly_turnover) on the
 * dense monthly layout (rule T1): per present row adv = VOL / 21, shares = so[a] when not NaN
 * else trunc(mcap[a] / PM) when mcap != 0 and PM > 0 (NaN when that is not finite),
 * turnover = adv / shares when shares > 0, and turn_avg = pandas' rolling(lookback,
 * min_periods=1).mean() over the asset's present rows (bit-exact restatement).
 *   PM, VOL [T_m][N] from csm_month_end;  so, mcap [N] (NaN = not given)
 *   ADV, SH, TURN, TAVG [T_m][N] out (NaN where the asset has no row); lookback in [1, 48]
 */
int csm_turnover_features(csm_ctx* ctx, const double* PM, const double* VOL, const double* so,
                          const double* mcap, int32_t T_m, int64_t N, int32_t lookback,
                          double* ADV, double* SH, double* TURN, double* TAVG);

/*
 * Momentum x volume double sort helpers (LeSw00 section II; rule T2):
 *   Xm = X where M is valid, NaN elsewhere (the tercile universe; nullable)
 *   Lc = n_vol * Lm + Lv where both labels are valid, -1 elsewhere (nullable)
 * The cell returns then come from csm_portfolio with n_bins = n_mom * n_vol (30 supported).
 */
int csm_double_sort_labels(csm_ctx* ctx, const double* M, const double* X, const int8_t* Lm,
                           const int8_t* Lv, int32_t T_m, int64_t N, int32_t n_vol, double* Xm,
                           int8_t* Lc);

/*
 * The date-shard collectives over RCCL (xGMI on one node), for hosts that shard
 * run_demo.py:31-67 without torch.distributed: csm_comm_unique_id fills CSM_UNIQUE_ID_BYTES
 * (host memory) on ONE rank; the bytes reach the other ranks out of band; every rank calls
 * csm_allgather_init with them (one communicator per context, on the context's device); then
 * csm_allgather gathers `bytes` from every rank into recv (device, nranks * bytes, rank order)
 * on the context's stream -- collective 1 (the [S][N] shard summaries for csm_fold_carry) and
 * collective 2 (the per-date decile means / counts for csm_long_short).  csm_allgather_free
 * (also done by csm_destroy) releases the communicator.  RCCL is loaded at first use;
 * CSM_E_RCCL when it is missing or a call fails.
 */
int csm_comm_unique_id(void* unique_id);
int csm_allgather_init(csm_ctx* ctx, const void* unique_id, int32_t rank, int32_t nranks);
int csm_allgather(csm_ctx* ctx, const void* send, void* recv, int64_t bytes);
int csm_allgather_free(csm_ctx* ctx);

#ifdef __cplusplus
}
#endif

#endif /* CSMOM_H */
