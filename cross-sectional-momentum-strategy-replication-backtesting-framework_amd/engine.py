"""Device engine: the momentum hot path on dense HBM-resident panels.

`Engine` owns one csm context per device and launches on torch's current HIP stream, so
torch events, graphs and allocations compose with it.  Tensors are torch ROCm tensors:
  P[T_d][N] f64 daily prices (ABSENT payload = no row, NaN = missing price),
  month_start[T_m+1] int64, everything else as in include/csmom.h.

Reference mapping (file:line):
  month_end   -> src/features.py:34-39      momentum   -> src/features.py:44-52, run_demo.py:48
  deciles     -> run_demo.py:18-29,46,49-55  long_short -> run_demo.py:57-67
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch

from ._lib import ABSENT_BITS, check, load_library

QTABLE_CACHE: dict[int, np.ndarray] = {}
FUSED_MIN_N = 32768  # below this the fused kernel has too few waves to fill 256 CUs
DEC_NARROW_MAX = 16384   # widest row of the narrow-row decile kernels (libcsmom's default)
LEGS_MAX_N = 7168        # widest row of the legs-only portfolio accounting (SEG_MAXN)


def quantile_table(n_bins: int) -> np.ndarray:
    """qcut's quantile grid as NumPy's percentile sees it ((linspace*100)/100)."""
    q = QTABLE_CACHE.get(n_bins)
    if q is None:
        q = np.ascontiguousarray((np.linspace(0.0, 1.0, n_bins + 1) * 100.0) / 100.0)
        QTABLE_CACHE[n_bins] = q
    return q


def absent_tensor(shape, device) -> torch.Tensor:
    return torch.full(shape, ABSENT_BITS, dtype=torch.int64, device=device).view(torch.float64)


def is_absent(x: torch.Tensor) -> torch.Tensor:
    b = x.contiguous().view(torch.int64)
    return (b & 0x7FF7FFFFFFFFFFFF) == ABSENT_BITS


def _ptr(t: torch.Tensor | None):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _qptr(n_bins: int):
    """The quantile table as the C calls take it (a table of one entry for an n_bins they refuse)."""
    q = quantile_table(n_bins) if n_bins >= 1 else np.zeros(1)
    return q.ctypes.data_as(ctypes.c_void_p)


def _need(t: torch.Tensor, name: str, dtype, shape, device):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if t.device != device:
        raise ValueError(f"{name} must live on {device}, got {t.device}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


@dataclass
class PipelineOut:
    PM: torch.Tensor
    M: torch.Tensor
    NR: torch.Tensor
    L: torch.Tensor
    EW: torch.Tensor
    CNT: torch.Tensor
    LS: torch.Tensor
    R: torch.Tensor | None = None
    VOL: torch.Tensor | None = None
    NV: torch.Tensor | None = None
    # run_universe only: the breakpoint set's size, the screen's kept cells (None without a
    # screen), the distinct edges and their number per date (rules U2, U5)
    NVB: torch.Tensor | None = None
    KEPT: torch.Tensor | None = None
    EDGES: torch.Tensor | None = None
    NE: torch.Tensor | None = None


@dataclass
class PortfolioOut:
    PR: torch.Tensor                 # [T_m][B][n_bins] overlapped decile returns
    LS: torch.Tensor                 # [T_m][B] long-short (NaN = dropped month)
    TURN: torch.Tensor | None = None  # [T_m][B] long-short turnover
    COST: torch.Tensor | None = None  # [T_m][B] transaction cost
    NET: torch.Tensor | None = None   # [T_m][B] LS - COST
    legs_only: bool = False           # PR holds deciles 0 and n_bins - 1 only (NaN elsewhere)


@dataclass
class DailyOut:
    DR: torch.Tensor                  # [T_d][n_bins] daily returns of the bins (NaN = no portfolio)
    DLS: torch.Tensor                 # [T_d] top minus bottom (NaN if either leg is)
    DCNT: torch.Tensor | None = None  # [T_m][K][n_bins] int32 member counts


class MonthStats(NamedTuple):
    """csm_month_stats (rule D1), each [T_m][N]; unpacks into window_signals' first arguments."""
    PM: torch.Tensor    # month-end price, csm_month_end's value (ABSENT = the month has no row)
    P1: torch.Tensor    # first priced row's price
    HI: torch.Tensor    # maximum over the priced rows
    SSW: torch.Tensor   # sum of squared daily returns inside the month
    NDW: torch.Tensor   # int32, their number


@dataclass
class SignalsOut:
    """csm_window_signals (rules D2..D6), each [T_m][N]; None = not asked for."""
    SS: torch.Tensor | None = None       # SSW plus the month's first return, squared
    ND: torch.Tensor | None = None       # int32, NDW plus one where that return exists
    H52: torch.Tensor | None = None      # month-end price over the Jh-month high
    RV: torch.Tensor | None = None       # realised daily volatility over Jv months (the SIG input)
    MS: torch.Tensor | None = None       # M / RV
    NR_H52: torch.Tensor | None = None   # next return of the H52 ranking
    NR_MS: torch.Tensor | None = None    # next return of the MS ranking


@dataclass
class MarketModelOut:
    """csm_market_model (rules B3..B5), each [T_m][N]; None = not asked for."""
    BETA: torch.Tensor | None = None     # slope of the asset's month returns on the factor
    ALPHA: torch.Tensor | None = None    # intercept
    IVOL: torch.Tensor | None = None     # residual standard deviation, n - 2 degrees of freedom
    RESMOM: torch.Tensor | None = None   # residual momentum: sum of residuals over their deviation
    NOBS: torch.Tensor | None = None     # int32, observations in the window
    F: torch.Tensor | None = None        # [T_m] the factor regressed on (MKT when none was given)


class DailySums(NamedTuple):
    """csm_daily_sums (rule V3), each [T_m][N]: a month's raw moment sums over the days where the
    asset's daily return r and the factor f both exist; daily_model's input."""
    NO: torch.Tensor                     # int32, the observations
    SR: torch.Tensor                     # sum of r
    SF: torch.Tensor                     # sum of f
    SRR: torch.Tensor                    # sum of r * r
    SFF: torch.Tensor                    # sum of f * f
    SRF: torch.Tensor                    # sum of r * f
    SR3: torch.Tensor | None = None      # sum of (r * r) * r
    RMAX: torch.Tensor | None = None     # the largest r (NaN = no observation)


@dataclass
class DailyModelOut:
    """csm_daily_model (rule V4), each [T_m][N]; None = not asked for."""
    DBETA: torch.Tensor | None = None    # slope of the daily returns on the factor
    DIVOL: torch.Tensor | None = None    # residual standard deviation, n - 2 degrees of freedom
    DTVOL: torch.Tensor | None = None    # standard deviation of the daily returns, n - 1
    DSKEW: torch.Tensor | None = None    # their skewness (population moments)
    DMAX: torch.Tensor | None = None     # the window's largest daily return
    NOBS: torch.Tensor | None = None     # int32, observations in the window


@dataclass
class FactorModelOut:
    """csm_factor_model (rules MF1..MF5); None = not asked for."""
    BETA: torch.Tensor | None = None     # [KF][T_m][N] slopes on the KF factors
    ALPHA: torch.Tensor | None = None    # [T_m][N] intercept
    IVOL: torch.Tensor | None = None     # residual standard deviation, n - (KF + 1) degrees
    RESMOM: torch.Tensor | None = None   # residual momentum on the KF-factor residuals
    R2: torch.Tensor | None = None       # 1 - residual over total sum of squares
    NOBS: torch.Tensor | None = None     # int32, observations in the window
    F: torch.Tensor | None = None        # [T_m][KF] the factors regressed on


class DailyFSums(NamedTuple):
    """csm_daily_fsums (rule MF6): a month's raw moment sums over the days where the asset's
    daily return r and all KF factors exist; daily_fmodel's input."""
    NO: torch.Tensor                     # [T_m][N] int32, the observations
    SR: torch.Tensor                     # [T_m][N] sum of r
    SRR: torch.Tensor                    # [T_m][N] sum of r * r
    SF: torch.Tensor                     # [KF][T_m][N] sum of f_k
    SRF: torch.Tensor                    # [KF][T_m][N] sum of r * f_k
    SFF: torch.Tensor                    # [KF (KF + 1) / 2][T_m][N] sum of f_j * f_k, j <= k


@dataclass
class DailyFModelOut:
    """csm_daily_fmodel (rule MF7); None = not asked for."""
    DBETA: torch.Tensor | None = None    # [KF][T_m][N] slopes of the daily returns on the factors
    DALPHA: torch.Tensor | None = None   # [T_m][N] intercept
    DIVOL: torch.Tensor | None = None    # residual standard deviation, n - (KF + 1) degrees
    DR2: torch.Tensor | None = None      # 1 - residual over total sum of squares
    NOBS: torch.Tensor | None = None     # int32, observations in the window


class LiqSums(NamedTuple):
    """csm_liq_sums (rule Q2), each [T_m][N]: a month's day counts and its volume, dollar volume
    and Amihud sums; liq_model's input."""
    NP: torch.Tensor                     # int32, priced days
    ND: torch.Tensor                     # int32, days with a return (rule V1)
    NA: torch.Tensor                     # int32, days with a return and a positive dollar volume
    NZR: torch.Tensor | None             # int32, return days with r == 0
    NZV: torch.Tensor | None             # int32, priced days with zero volume
    SV: torch.Tensor | None              # sum of the volume over the priced days
    SDV: torch.Tensor                    # sum of price * volume over the priced days
    SIL: torch.Tensor                    # sum of |r| / (price * volume) over the Amihud days


@dataclass
class LiqModelOut:
    """csm_liq_model (rule Q3), each [T_m][N]; None = not asked for."""
    ILLIQ: torch.Tensor | None = None    # Amihud (2002): mean |r| / dollar volume, times scale
    DVOL: torch.Tensor | None = None     # dollar average daily volume (portfolio's ADV)
    TURN: torch.Tensor | None = None     # average daily volume over shares outstanding
    ZRET: torch.Tensor | None = None     # share of the return days with a zero return
    ZVOL: torch.Tensor | None = None     # share of the priced days with zero volume
    NOBS: torch.Tensor | None = None     # int32, Amihud days in the window


class RangeSums(NamedTuple):
    """csm_range_sums (rule HL5), each [T_m][N]: a month's ranged days and pairs and its
    Parkinson, Corwin-Schultz and Abdi-Ranaldo sums; range_model's input."""
    NRG: torch.Tensor                    # int32, ranged days (rule HL1)
    NPR: torch.Tensor                    # int32, pairs of ranged days (rule HL3)
    NCS: torch.Tensor | None             # int32, pairs with a Corwin-Schultz spread
    SPK: torch.Tensor                    # sum of the squared log ranges
    SCS: torch.Tensor | None             # sum of the zero-floored Corwin-Schultz spreads
    SAR: torch.Tensor | None             # sum of the Abdi-Ranaldo terms


@dataclass
class RangeModelOut:
    """csm_range_model (rule HL6), each [T_m][N]; None = not asked for."""
    PKVOL: torch.Tensor | None = None    # Parkinson (1980) daily volatility
    CSSPR: torch.Tensor | None = None    # Corwin-Schultz (2012) high-low spread
    ARSPR: torch.Tensor | None = None    # Abdi-Ranaldo (2017) close-high-low spread
    NOBS: torch.Tensor | None = None     # int32, pairs in the window


class AsymSums(NamedTuple):
    """csm_asym_sums (rule AS2), each [T_m][N]: a month's return days by the sign of the return,
    their squared returns, and the market-model sums over the days on one side of FD; asym_model's
    input.  The five side panels are None when no FD was given."""
    ND: torch.Tensor                     # int32, days with a return (rule V1)
    NUP: torch.Tensor                    # int32, days with r > 0
    NDN: torch.Tensor                    # int32, days with r < 0
    SUP: torch.Tensor                    # sum of r * r over the days with r > 0
    SDN: torch.Tensor                    # sum of r * r over the days with r < 0
    NB: torch.Tensor | None = None       # int32, return days with f on the side
    BR: torch.Tensor | None = None       # sum of r over them
    BF: torch.Tensor | None = None       # sum of f
    BFF: torch.Tensor | None = None      # sum of f * f
    BRF: torch.Tensor | None = None      # sum of r * f


@dataclass
class AsymModelOut:
    """csm_asym_model (rule AS3), each [T_m][N]; None = not asked for."""
    ID: torch.Tensor | None = None       # information discreteness (Da, Gurun and Warachka 2014)
    RSJ: torch.Tensor | None = None      # signed jump variation over the realised variance
    DSVOL: torch.Tensor | None = None    # downside semi-volatility, daily
    DNBETA: torch.Tensor | None = None   # slope of the daily returns on f over the side days
    NOBS: torch.Tensor | None = None     # int32, return days in the window
    NSIDE: torch.Tensor | None = None    # int32, side days in the window


@dataclass
class XsRegressOut:
    """csm_xs_regress (rules R1..R5): one cross-sectional regression per month."""
    GAMMA: torch.Tensor                  # [T_m][K + 1] intercept, then one slope per signal
    R2: torch.Tensor                     # [T_m]
    NOBS: torch.Tensor                   # [T_m] int32, the month's observations


@dataclass
class NeweyWestOut:
    """csm_newey_west (rule R6), each [C] (0-d for a [T] series)."""
    MEAN: torch.Tensor                   # time-series mean of the non-NaN entries
    SE: torch.Tensor                     # its Newey-West standard error
    T: torch.Tensor                      # MEAN / SE
    NT: torch.Tensor                     # int32, the non-NaN entries


@dataclass
class FamaMacBethOut(XsRegressOut):
    """Engine.fama_macbeth: the per-month regressions and the summary of their coefficients."""
    MEAN: torch.Tensor | None = None     # [K + 1] time-series means of GAMMA's columns
    SE: torch.Tensor | None = None       # [K + 1]
    T: torch.Tensor | None = None        # [K + 1]
    NT: torch.Tensor | None = None       # [K + 1] int32, months behind each
    R2_MEAN: torch.Tensor | None = None  # 0-d, the mean of the months' R2
    lags: int = 0                        # Newey-West lags used


@dataclass
class GroupStatsOut:
    """csm_group_stats (rules N4, N5); None = not asked for."""
    GMEAN: torch.Tensor | None = None    # [T_m][n_groups] mean of the signal over the group's members
    GSD: torch.Tensor | None = None      # [T_m][n_groups] its standard deviation, n - 1 (NaN for n < 2)
    GCNT: torch.Tensor | None = None     # [T_m][n_groups] int32, the members
    SA: torch.Tensor | None = None       # [T_m][N] signal minus its group's mean
    SZ: torch.Tensor | None = None       # [T_m][N] SA over the group's deviation
    SB: torch.Tensor | None = None       # [T_m][N] the group's mean at its members: the industry signal


@dataclass
class RankICOut:
    """csm_rank_ic (rules I3..I6), each [T_m]."""
    RIC: torch.Tensor                    # Spearman rank IC of S[t] with Y[t + lead] (NaN = undefined)
    PIC: torch.Tensor | None             # Pearson IC on the same observations; None = not asked for
    NOBS: torch.Tensor                   # int32, the month's observations


@dataclass
class ICDecayOut:
    """Engine.ic_decay: rank_ic per horizon and the Newey-West summary of each horizon's series."""
    RIC: torch.Tensor                    # [H][T_m]
    PIC: torch.Tensor                    # [H][T_m]
    NOBS: torch.Tensor                   # [H][T_m] int32
    MEAN: torch.Tensor                   # [H] time-series mean of RIC's rows
    SE: torch.Tensor                     # [H] its Newey-West standard error
    T: torch.Tensor                      # [H]
    NT: torch.Tensor                     # [H] int32, the months behind each
    horizons: tuple = ()
    lags: int = 0


@dataclass
class ShardState:
    """signal_shard's end-state record [5][N] (present months, pending ranked row, its
    subset-ffilled price, first / last present month) with the daily panel it came from
    (shard_summary / shard_repair re-derive months PM does not keep from it)."""
    t: torch.Tensor
    P: torch.Tensor
    month_start: torch.Tensor


class Engine:
    """Signal (J, skip) -> per-date n_bins labels -> equal-weight long-short, on one GPU."""

    shard_ids = True   # the fused date-shard pass writes bucket ids and ranks from them

    def __init__(self, device: int | str | torch.device = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("csmom.Engine needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = load_library()
        self.cus = int(torch.cuda.get_device_properties(self.device).multi_processor_count)
        h = ctypes.c_void_p()
        st = self.lib.csm_create(self.device.index, ctypes.byref(h))
        if st != 0:
            raise RuntimeError(f"csm_create(device={self.device.index}) failed with {st}")
        self.ctx = h

    def __del__(self):
        lib = getattr(self, "lib", None)
        if lib is not None and getattr(self, "ctx", None):
            lib.csm_destroy(self.ctx)
            self.ctx = None

    # ------------------------------------------------------------------ plumbing
    def _bind_stream(self):
        s = torch.cuda.current_stream(self.device).cuda_stream
        if s != getattr(self, "_bound_stream", None):   # one ctypes call per stream change
            self.lib.csm_set_stream(self.ctx, ctypes.c_void_p(s))
            self._bound_stream = s

    def _call(self, name, *args):
        self._bind_stream()
        check(self.lib, self.ctx, getattr(self.lib, name)(self.ctx, *args), name)

    def empty(self, shape, dtype=torch.float64):
        return torch.empty(shape, dtype=dtype, device=self.device)

    # ------------------------------------------------------------------ stages
    def month_end(self, P, month_start, V=None, PM=None, VOL=None):
        T_d, N = P.shape
        T_m = month_start.numel() - 1
        _need(P, "P", torch.float64, (T_d, N), self.device)
        _need(month_start, "month_start", torch.int64, (T_m + 1,), self.device)
        PM = self.empty((T_m, N)) if PM is None else PM
        _need(PM, "PM", torch.float64, (T_m, N), self.device)
        if V is not None:
            _need(V, "V", torch.float64, (T_d, N), self.device)
            VOL = self.empty((T_m, N)) if VOL is None else VOL
            _need(VOL, "VOL", torch.float64, (T_m, N), self.device)
        else:
            VOL = None
        self._call("csm_month_end", _ptr(P), _ptr(V), T_d, N, _ptr(month_start), T_m,
                   _ptr(PM), _ptr(VOL))
        return PM, VOL

    def momentum(self, PM, J=12, skip=1, with_ret=False, carry=None, next_pm=None,
                 carry_out=None, out=None, chunked="auto"):
        """csm_momentum.  chunked="auto": panels too narrow to fill the chip (few assets)
        take the time-chunked scan (csm_momentum_chunked, the same bits) when no carry is
        involved."""
        T_m, N = PM.shape
        if (chunked == "auto" and carry is None and next_pm is None and carry_out is None
                and self.default_chunks(T_m, N, J, skip) > 1):
            return self.momentum_chunked(PM, J, skip, with_ret=with_ret, out=out)
        _need(PM, "PM", torch.float64, (T_m, N), self.device)
        W = J + skip
        if carry is not None:
            _need(carry, "carry", torch.float64, (W + 2, N), self.device)
        if next_pm is not None:
            _need(next_pm, "next_pm", torch.float64, (N,), self.device)
        if carry_out is not None:
            _need(carry_out, "carry_out", torch.float64, (W + 2, N), self.device)
        if out is None:
            R = self.empty((T_m, N)) if with_ret else None
            M = self.empty((T_m, N))
            NR = self.empty((T_m, N))
        else:
            R, M, NR = out
        self._call("csm_momentum", _ptr(PM), T_m, N, int(J), int(skip), _ptr(R), _ptr(M),
                   _ptr(NR), _ptr(carry), _ptr(next_pm), _ptr(carry_out))
        return R, M, NR

    def momentum_multi(self, PM, Js, skip=1, with_ids=False, chunks=1, stacked=False):
        """csm_momentum_multi: one scan for several look-backs (up to 4 per launch).  Returns
        [(M, NR)] in the order of Js, each equal bit for bit to momentum(PM, J, skip).
        with_ids (csm_momentum_multi_ids): [(M, NR, IDS)], IDS the fixed-map bucket id of
        every mom_J (uint16 [T_m][N], read by deciles_ids on rows of any width).  chunks > 1
        (narrow panels; max(J) + skip <= 16, even N): the time-chunked multi-J scan
        (csm_momentum_multi_chunked), the same bits.  stacked: each launch group's M / NR / IDS
        are consecutive [T_m][N] blocks of one allocation (the joined sweep reads them as one
        [nJ][T_m][N] tensor, no copy); otherwise one allocation per output, freed one by one."""
        T_m, N = PM.shape
        _need(PM, "PM", torch.float64, (T_m, N), self.device)
        Js = [int(J) for J in Js]
        outs = []
        for q0 in range(0, len(Js), 4):
            grp = Js[q0:q0 + 4]
            if stacked:
                Ms = list(self.empty((len(grp), T_m, N)))
                NRs = list(self.empty((len(grp), T_m, N)))
            else:
                Ms = [self.empty((T_m, N)) for _ in grp]
                NRs = [self.empty((T_m, N)) for _ in grp]
            new_ids = ((lambda: list(self.empty((len(grp), T_m, N), torch.int16))) if stacked
                       else (lambda: [self.empty((T_m, N), torch.int16) for _ in grp]))
            jarr = (ctypes.c_int32 * len(grp))(*grp)
            marr = (ctypes.c_void_p * len(grp))(*[t.data_ptr() for t in Ms])
            narr = (ctypes.c_void_p * len(grp))(*[t.data_ptr() for t in NRs])
            if chunks > 1:
                IDs = new_ids() if with_ids else None
                iarr = ((ctypes.c_void_p * len(grp))(*[t.data_ptr() for t in IDs])
                        if with_ids else None)
                nbytes = int(self.lib.csm_momentum_multi_chunked_workspace(
                    T_m, N, max(grp), int(skip), int(chunks)))
                ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=self.device)
                self._call("csm_momentum_multi_chunked", _ptr(PM), T_m, N, jarr, len(grp),
                           int(skip), int(chunks), marr, narr, iarr, _ptr(ws))
                outs.extend(zip(Ms, NRs, IDs) if with_ids else zip(Ms, NRs))
            elif with_ids:
                IDs = new_ids()
                iarr = (ctypes.c_void_p * len(grp))(*[t.data_ptr() for t in IDs])
                self._call("csm_momentum_multi_ids", _ptr(PM), T_m, N, jarr, len(grp), int(skip),
                           marr, narr, iarr)
                outs.extend(zip(Ms, NRs, IDs))
            else:
                self._call("csm_momentum_multi", _ptr(PM), T_m, N, jarr, len(grp), int(skip),
                           marr, narr)
                outs.extend(zip(Ms, NRs))
        return outs

    @staticmethod
    def default_chunks(T_m, N, J=12, skip=1):
        """Chunks for the time-chunked scan: enough (chunk, asset) lanes to fill the chip
        (~2^17), chunks no shorter than one window (C2, 300 months: 20 chunks, scan 0.078 ->
        0.068 ms against 10 chunks of two windows; the fold chains through any number of
        earlier chunks, so the outputs are the same bits)."""
        if T_m <= 0:
            return 1
        want = max(1, -(-131072 // max(N, 1)))
        return int(max(1, min(want, T_m // max(J + skip + 1, 1), 256)))

    def momentum_chunked(self, PM, J=12, skip=1, chunks=None, with_ret=False, next_pm=None,
                         out=None, workspace=None, ids=None):
        """csm_momentum_chunked: the scan split into `chunks` concurrent month ranges.  ids
        (int16 [T_m][N], N % 4 == 0): also each mom_J's fixed-map bucket id
        (csm_momentum_chunked_ids, for deciles_ids)."""
        T_m, N = PM.shape
        _need(PM, "PM", torch.float64, (T_m, N), self.device)
        C = self.default_chunks(T_m, N, J, skip) if chunks is None else int(chunks)
        if next_pm is not None:
            _need(next_pm, "next_pm", torch.float64, (N,), self.device)
        if out is None:
            R = self.empty((T_m, N)) if with_ret else None
            M, NR = self.empty((T_m, N)), self.empty((T_m, N))
        else:
            R, M, NR = out
        nbytes = int(self.lib.csm_momentum_chunked_workspace(T_m, N, int(J), int(skip), C))
        if workspace is None or workspace.numel() * workspace.element_size() < nbytes:
            workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=self.device)
        if ids is not None:
            _need(ids, "ids", torch.int16, (T_m, N), self.device)
            self._call("csm_momentum_chunked_ids", _ptr(PM), T_m, N, int(J), int(skip), C, _ptr(R),
                       _ptr(M), _ptr(NR), _ptr(next_pm), _ptr(ids), _ptr(workspace))
        else:
            self._call("csm_momentum_chunked", _ptr(PM), T_m, N, int(J), int(skip), C, _ptr(R),
                       _ptr(M), _ptr(NR), _ptr(next_pm), _ptr(workspace))
        return R, M, NR

    @staticmethod
    def signal_default_chunks(T_m, N, J=12, skip=1, cus=256):
        """Chunks for csm_signal_chunked: as many as keep the grid (chunks x ceil(N / 256)
        workgroups) within one workgroup per CU, chunks no shorter than one window, and never
        fewer than the 32-months-per-chunk limit needs.  A second workgroup on a CU waits for
        the first to leave (each holds ~80 KB of LDS and its month-end stream saturates the
        CU), so the grid beyond the CU count serialises: C2 (20 column blocks) at 12 / 13 / 21
        chunks 0.130 / 0.152 / 0.140 ms per step (profiles/r05/experiments/tc_chunks/)."""
        if T_m <= 0:
            return 1
        nbx = max(1, -(-N // 256))
        c = min(max(1, cus // nbx), max(1, T_m // max(J + skip + 1, 1)), 64)
        return int(min(max(c, -(-T_m // 32)), 64))

    def signal_chunked(self, P, month_start, max_month_days, J=12, skip=1, chunks=None,
                       with_ret=False, with_ids=True, out=None, workspace=None, check=True):
        """csm_signal_chunked: month-end + time-chunked scan in one launch (narrow panels, C2):
        the same R / M / NR / ids bits as month_end -> momentum_chunked(_ids).  Even N, months
        of <= 23 day rows.  workspace: a zero-filled uint8 buffer of
        csm_signal_chunked_workspace bytes (kept by the caller across calls: each launch leaves
        its sync words zero).  check (default): unless the stream is capturing, read the
        launch's give-up mark (csm_signal_chunked_status; synchronises) and raise CsmError
        (CSM_E_TIMEOUT) if a workgroup gave up a wait.  check=False (timed loops, graph capture):
        the caller calls signal_chunked_status(workspace) itself afterwards.
        Returns (R, M, NR, IDS, workspace)."""
        T_d, N = P.shape
        T_m = month_start.numel() - 1
        _need(P, "P", torch.float64, (T_d, N), self.device)
        _need(month_start, "month_start", torch.int64, (T_m + 1,), self.device)
        C = (self.signal_default_chunks(T_m, N, J, skip, self.cus) if chunks is None
             else int(chunks))
        C = max(1, min(C, 64, max(T_m, 1)))
        if out is None:
            R = self.empty((T_m, N)) if with_ret else None
            M, NR = self.empty((T_m, N)), self.empty((T_m, N))
            IDS = self.empty((T_m, N), torch.int16) if with_ids else None
        else:
            R, M, NR, IDS = out
        if IDS is not None:
            _need(IDS, "IDS", torch.int16, (T_m, N), self.device)
        nbytes = int(self.lib.csm_signal_chunked_workspace(T_m, N, int(J), int(skip), C))
        if workspace is None or workspace.numel() * workspace.element_size() < nbytes:
            workspace = torch.zeros(max(nbytes, 256), dtype=torch.uint8, device=self.device)
        if R is not None:
            _need(R, "R", torch.float64, (T_m, N), self.device)
        _need(M, "M", torch.float64, (T_m, N), self.device)
        _need(NR, "NR", torch.float64, (T_m, N), self.device)
        self._call("csm_signal_chunked", _ptr(P), T_d, N, _ptr(month_start), T_m,
                   int(max_month_days), int(J), int(skip), C, _ptr(R), _ptr(M), _ptr(NR),
                   _ptr(IDS), _ptr(workspace))
        if check and not torch.cuda.is_current_stream_capturing():
            self.signal_chunked_status(workspace)
        return R, M, NR, IDS, workspace

    def signal_chunked_status(self, workspace):
        """csm_signal_chunked_status: synchronise, raise CsmError (CSM_E_TIMEOUT) if a
        csm_signal_chunked launch on this workspace gave up a wait since the last check (its
        outputs are invalid; the mark is cleared)."""
        self._call("csm_signal_chunked_status", _ptr(workspace))

    @staticmethod
    def signal_chunked_timed_out(workspace):
        """Whether the workspace holds an unreported give-up mark (sync word 2; never set by a
        correct launch).  Synchronises; does not clear it."""
        return bool(workspace[8:12].view(torch.int32).item() != 0)

    def signal(self, P, month_start, max_month_days, J=12, skip=1, with_pm=False,
               with_ret=False, carry=None, next_pm=None, carry_out=None, out=None):
        """Fused month-end + scan (csm_signal): one pass over the daily panel, no PM round
        trip.  Needs even N and months of <= 32 days."""
        T_d, N = P.shape
        T_m = month_start.numel() - 1
        _need(P, "P", torch.float64, (T_d, N), self.device)
        _need(month_start, "month_start", torch.int64, (T_m + 1,), self.device)
        W = J + skip
        for t, nm, shp in ((carry, "carry", (W + 2, N)), (next_pm, "next_pm", (N,)),
                           (carry_out, "carry_out", (W + 2, N))):
            if t is not None:
                _need(t, nm, torch.float64, shp, self.device)
        if out is None:
            PM = self.empty((T_m, N)) if with_pm else None
            R = self.empty((T_m, N)) if with_ret else None
            M, NR = self.empty((T_m, N)), self.empty((T_m, N))
        else:
            PM, R, M, NR = out
        self._call("csm_signal", _ptr(P), T_d, N, _ptr(month_start), T_m, int(max_month_days),
                   int(J), int(skip), _ptr(PM), _ptr(R), _ptr(M), _ptr(NR), _ptr(carry),
                   _ptr(next_pm), _ptr(carry_out))
        return PM, R, M, NR

    def signal_ids(self, P, month_start, max_month_days, J=12, skip=1, with_pm=False,
                   with_ret=False, out=None, min_month_days=0):
        """csm_signal_ids: csm_signal (no carry) that also writes the fixed-map bucket id of
        every mom_J (uint16 [T_m][N], read by deciles_ids).  N % 4 == 0.
        Returns (PM, R, M, NR, IDS)."""
        T_d, N = P.shape
        T_m = month_start.numel() - 1
        _need(P, "P", torch.float64, (T_d, N), self.device)
        _need(month_start, "month_start", torch.int64, (T_m + 1,), self.device)
        if out is None:
            PM = self.empty((T_m, N)) if with_pm else None
            R = self.empty((T_m, N)) if with_ret else None
            M, NR = self.empty((T_m, N)), self.empty((T_m, N))
            IDS = self.empty((T_m, N), torch.int16)
        else:
            PM, R, M, NR, IDS = out
        _need(IDS, "IDS", torch.int16, (T_m, N), self.device)
        self._call("csm_signal_ids", _ptr(P), T_d, N, _ptr(month_start), T_m, int(max_month_days),
                   int(min_month_days), int(J), int(skip), _ptr(PM), _ptr(R), _ptr(M), _ptr(NR),
                   _ptr(IDS))
        return PM, R, M, NR, IDS

    def deciles_ids(self, M, NR, IDS, n_bins=10, out=None, with_nv=False, LS=None, legs=False):
        """csm_deciles_ids: deciles() from the ids of signal_ids / momentum_multi(with_ids=True)
        (same labels / counts).  Rows of <= 16384 assets take the narrow kernel (2048 buckets:
        the fixed map's ids >> 2), wider rows the 8192-bucket merged pass; needs N % 4 == 0.
        LS (float64 [T_m], needs NR): also the long-short of every date, in the same launch
        (csm_deciles_ids_ls; equal to long_short(EW, CNT) bit for bit).
        legs=True (NR None; for legs-only accounting): csm_deciles_ids_legs -- labels 0,
        n_bins - 1 and NaN exact, every other ranked cell SOME label in [1, n_bins - 2]."""
        T_m, N = M.shape
        _need(M, "M", torch.float64, (T_m, N), self.device)
        _need(IDS, "IDS", torch.int16, (T_m, N), self.device)
        if NR is not None:
            _need(NR, "NR", torch.float64, (T_m, N), self.device)
        if out is None:
            L = self.empty((T_m, N), torch.int8)
            EW = self.empty((T_m, n_bins)) if NR is not None else None
            CNT = self.empty((T_m, n_bins), torch.int32) if NR is not None else None
            NV = self.empty((T_m,), torch.int32) if with_nv else None
        else:
            L, EW, CNT, NV = out
        q = quantile_table(n_bins)
        if LS is not None:
            if NR is None:
                raise ValueError("deciles_ids(LS=...) needs NR")
            _need(LS, "LS", torch.float64, (T_m,), self.device)
            self._call("csm_deciles_ids_ls", _ptr(M), _ptr(NR), _ptr(IDS), T_m, N, int(n_bins),
                       q.ctypes.data_as(ctypes.c_void_p), _ptr(L), _ptr(EW), _ptr(CNT), _ptr(NV),
                       _ptr(LS))
            return L, EW, CNT, NV
        if legs:
            if NR is not None:
                raise ValueError("deciles_ids(legs=True) takes no NR (labels only)")
            self._call("csm_deciles_ids_legs", _ptr(M), _ptr(IDS), T_m, N, int(n_bins),
                       q.ctypes.data_as(ctypes.c_void_p), _ptr(L), _ptr(NV))
            return L, EW, CNT, NV
        self._call("csm_deciles_ids", _ptr(M), _ptr(NR), _ptr(IDS), T_m, N, int(n_bins),
                   q.ctypes.data_as(ctypes.c_void_p), _ptr(L), _ptr(EW), _ptr(CNT), _ptr(NV))
        return L, EW, CNT, NV

    @staticmethod
    def month_days(month_start):
        """(longest month, shortest interior month) in days, one device sync; the first and
        the last month may be partial (csm_signal_ids' min_month_days excepts them)."""
        if month_start.numel() < 2:
            return 1, 0
        d = month_start[1:] - month_start[:-1]
        inner = d[1:-1] if d.numel() > 2 else d[:0]
        mn = inner.min() if inner.numel() else torch.full_like(d[0], 1 << 30)
        mx, mn = torch.stack([d.max(), mn]).tolist()
        return int(mx), int(mn)

    def pipeline(self, P, month_start, J=12, skip=1, n_bins=10, max_month_days=None,
                 with_pm=True, with_ret=False, out=None, min_month_days=None) -> PipelineOut:
        """csm_pipeline: the whole K = 1 pass in one C call (fused signal with bucket ids,
        labels + decile means, long-short)."""
        T_d, N = P.shape
        T_m = month_start.numel() - 1
        _need(P, "P", torch.float64, (T_d, N), self.device)
        _need(month_start, "month_start", torch.int64, (T_m + 1,), self.device)
        if max_month_days is None or min_month_days is None:
            mx, mn = self.month_days(month_start)
            max_month_days = mx if max_month_days is None else max_month_days
            min_month_days = mn if min_month_days is None else min_month_days
        if out is None:
            PM = self.empty((T_m, N)) if with_pm else None
            R = self.empty((T_m, N)) if with_ret else None
            M, NR = self.empty((T_m, N)), self.empty((T_m, N))
            L = self.empty((T_m, N), torch.int8)
            EW, CNT = self.empty((T_m, n_bins)), self.empty((T_m, n_bins), torch.int32)
            NV, LS = self.empty((T_m,), torch.int32), self.empty((T_m,))
        else:
            PM, R, M, NR, L, EW, CNT, NV, LS = out
        q = quantile_table(n_bins)
        self._call("csm_pipeline", _ptr(P), T_d, N, _ptr(month_start), T_m, int(max_month_days),
                   int(min_month_days), int(J), int(skip), int(n_bins),
                   q.ctypes.data_as(ctypes.c_void_p), _ptr(PM),
                   _ptr(R), _ptr(M), _ptr(NR), _ptr(L), _ptr(EW), _ptr(CNT), _ptr(NV), _ptr(LS))
        return PipelineOut(PM=PM, M=M, NR=NR, L=L, EW=EW, CNT=CNT, LS=LS, R=R, NV=NV)

    def deciles(self, M, NR=None, n_bins=10, out=None, with_nv=False):
        T_m, N = M.shape
        _need(M, "M", torch.float64, (T_m, N), self.device)
        if NR is not None:
            _need(NR, "NR", torch.float64, (T_m, N), self.device)
        if out is None:
            L = self.empty((T_m, N), torch.int8)
            EW = self.empty((T_m, n_bins)) if NR is not None else None
            CNT = self.empty((T_m, n_bins), torch.int32) if NR is not None else None
            NV = self.empty((T_m,), torch.int32) if with_nv else None
        else:
            L, EW, CNT, NV = out
        q = quantile_table(n_bins)
        self._call("csm_deciles", _ptr(M), _ptr(NR), T_m, N, int(n_bins),
                   q.ctypes.data_as(ctypes.c_void_p), _ptr(L), _ptr(EW), _ptr(CNT), _ptr(NV))
        return L, EW, CNT, NV

    def long_short(self, EW, CNT, LS=None):
        T_m, nb = EW.shape
        _need(EW, "EW", torch.float64, (T_m, nb), self.device)
        _need(CNT, "CNT", torch.int32, (T_m, nb), self.device)
        LS = self.empty((T_m,)) if LS is None else LS
        self._call("csm_long_short", _ptr(EW), _ptr(CNT), T_m, nb, _ptr(LS))
        return LS

    def portfolio(self, L, NR, n_bins=10, K=1, W=None, B=1, half_spread=0.0005, k_impact=0.1,
                  aum=0.0, ADV=None, SIG=None, with_costs=True, out=None, workspace=None):
        """csm_portfolio: K-overlapping cohorts, equal (W None) or value weights, long-short
        turnover and costs (rules E1..E5).  L/NR/W/ADV/SIG are [T_m][B*N] (B panels side by
        side, the sweep layout) or [T_m][N] with B = 1.  Returns a PortfolioOut."""
        T_m, BN = L.shape
        if B < 1 or BN % B:
            raise ValueError(f"row width {BN} is not B={B} panels")
        N = BN // B
        _need(L, "L", torch.int8, (T_m, BN), self.device)
        _need(NR, "NR", torch.float64, (T_m, BN), self.device)
        for t, nm in ((W, "W"), (ADV, "ADV"), (SIG, "SIG")):
            if t is not None:
                _need(t, nm, torch.float64, (T_m, BN), self.device)
        if out is None:
            PR = self.empty((T_m, B, n_bins))
            LS = self.empty((T_m, B))
            TURN = self.empty((T_m, B)) if with_costs else None
            COST = self.empty((T_m, B)) if with_costs else None
            NET = self.empty((T_m, B)) if with_costs else None
        else:
            PR, LS, TURN, COST, NET = out
        nbytes = int(self.lib.csm_portfolio_workspace(T_m, B, N, int(n_bins), int(K)))
        if workspace is None or workspace.numel() * workspace.element_size() < nbytes:
            workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=self.device)
        self._call("csm_portfolio", _ptr(L), _ptr(NR), _ptr(W), T_m, int(B), N, int(n_bins),
                   int(K), float(half_spread), float(k_impact), float(aum), _ptr(ADV), _ptr(SIG),
                   _ptr(PR), _ptr(LS), _ptr(TURN), _ptr(COST), _ptr(NET), _ptr(workspace))
        return PortfolioOut(PR=PR, LS=LS, TURN=TURN, COST=COST, NET=NET)

    def _cohort_pass(self, T_m, BN, B, panels, n_bins, Ks, legs_only, need_full, run, bname="B"):
        """What the portfolio_multi* wrappers share.  Rows of BN cells are B panels of N assets
        (ValueError otherwise); legs_only holds only for rows of <= LEGS_MAX_N assets (wider
        rows: every decile).  run(N, Ks, Kmax, ws, legs_only, flag) checks its tensors, makes the
        cohort pass and its accounting, and returns the wrapper's result; ws(given=None) is a
        workspace for `panels` panels (`given` when it is large enough).  legs_only with
        need_full None: the pass gets a flag of its own, the flag is read back (the one device
        sync), and when it is set -- a panel lacks a leg's column -- run is repeated without
        legs."""
        if B < 1 or BN % B:
            raise ValueError(f"row width {BN} is not {bname}={B} panels")
        N = BN // B
        Ks = [int(k) for k in Ks]
        Kmax = max(Ks)
        legs_only = bool(legs_only) and N <= LEGS_MAX_N

        def ws(given=None):
            nbytes = int(self.lib.csm_portfolio_workspace(T_m, int(panels), N, int(n_bins), Kmax))
            if given is None or given.numel() * given.element_size() < nbytes:
                given = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=self.device)
            return given

        flag = need_full
        if legs_only and need_full is None:
            flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        out = run(N, Ks, Kmax, ws, legs_only, flag)
        if legs_only and need_full is None and int(flag.item()):
            out = run(N, Ks, Kmax, ws, False, None)
        return out

    def portfolio_multi(self, L, NR, n_bins=10, Ks=(1,), W=None, B=1, half_spread=0.0005,
                        k_impact=0.1, aum=0.0, ADV=None, SIG=None, with_costs=True,
                        workspace=None, return_stacked=False, legs_only=False, need_full=None):
        """One cohort-sum pass (csm_cohort_sums, Kmax = max(Ks)) shared by the accounting of
        every holding period K in Ks (csm_portfolio_from_cohorts).  Returns {K: PortfolioOut}.
        legs_only (rows of <= 7168 assets): sort and sum only deciles 0 and n_bins - 1
        (csm_cohort_sums_legs / csm_portfolio_from_cohorts_legs): LS / TURN / COST / NET bit for
        bit the full path's, PR NaN outside the legs.  When a panel lacks one leg's column (the
        long-short rule then needs every decile) the full path is rerun (one device sync); with
        need_full (device int32 [1], caller-zeroed) the flag is left there instead, no sync, and
        the caller reruns with legs_only=False when it is set."""
        T_m, BN = L.shape

        def run(N, Ks, Kmax, ws, legs, flag):
            _need(L, "L", torch.int8, (T_m, BN), self.device)
            _need(NR, "NR", torch.float64, (T_m, BN), self.device)
            for t, nm in ((W, "W"), (ADV, "ADV"), (SIG, "SIG")):
                if t is not None:
                    _need(t, nm, torch.float64, (T_m, BN), self.device)
            w = ws(workspace)
            self._call("csm_cohort_sums_legs" if legs else "csm_cohort_sums", _ptr(L), _ptr(NR),
                       _ptr(W), T_m, int(B), N, int(n_bins), Kmax, _ptr(w))
            return self._from_cohorts(L, W, T_m, B, N, n_bins, Ks, half_spread, k_impact, aum,
                                      ADV, SIG, with_costs, w, legs, flag)

        res, stacked = self._cohort_pass(T_m, BN, B, B, n_bins, Ks, legs_only, need_full, run)
        return (res, stacked) if return_stacked else res

    def portfolio_multi_js(self, Ls, NR, n_bins=10, Ks=(1,), B=1, half_spread=0.0005,
                           k_impact=0.1, aum=0.0, with_costs=True, legs_only=False, need_full=None):
        """portfolio_multi (equal weights) for several label panels Ls that share ONE next_ret
        panel NR (the bootstrap sweep's, boot_scan): one cohort pass for every J
        (csm_cohort_sums_js: each month's return row read once), then each J's accounting.
        Returns [(res, stacked)] per J, each equal bit for bit to portfolio_multi(L, NR, ...,
        return_stacked=True)."""
        T_m, BN = NR.shape
        nJ = len(Ls)

        def run(N, Ks, Kmax, ws, legs, flag):
            _need(NR, "NR", torch.float64, (T_m, BN), self.device)
            for L in Ls:
                _need(L, "L", torch.int8, (T_m, BN), self.device)
            wss = [ws() for _ in Ls]
            self._call("csm_cohort_sums_js", nJ, (ctypes.c_void_p * nJ)(*[L.data_ptr() for L in Ls]),
                       _ptr(NR), T_m, int(B), N, int(n_bins), Kmax, 1 if legs else 0,
                       (ctypes.c_void_p * nJ)(*[w.data_ptr() for w in wss]))
            return [self._from_cohorts(L, None, T_m, B, N, n_bins, Ks, half_spread, k_impact, aum,
                                       None, None, with_costs, w, legs, flag)
                    for L, w in zip(Ls, wss)]

        return self._cohort_pass(T_m, BN, B, B, n_bins, Ks, legs_only, need_full, run)

    def portfolio_plan(self, T_m, B, N, n_bins=10, K=1):
        """csm_portfolio_plan: (cohort chunks, turnover chunks) of a portfolio call; calls with
        the same plan give each panel the same bits."""
        v = int(self.lib.csm_portfolio_plan(int(T_m), int(B), int(N), int(n_bins), int(K)))
        if v < 0:
            raise ValueError("csm_portfolio_plan: bad arguments")
        return v & 0xFFFFFFFF, v >> 32

    def portfolio_multi_js_grouped(self, Lg, NR, n_bins=10, Ks=(1,), B=1, half_spread=0.0005,
                                   k_impact=0.1, aum=0.0, with_costs=True, legs_only=False,
                                   need_full=None, return_stacked=False):
        """portfolio_multi_js with the look-backs' label panels stored group-major, Lg int8
        [nJ][T_m][B * N] (as one stacked decile pass writes them): one cohort pass over the shared
        next_ret NR [T_m][B * N] into one workspace of nJ * B panels (csm_cohort_sums_js_grouped),
        then ONE accounting launch set for every J (csm_portfolio_from_cohorts_grouped: panel
        q * B + b = J q's panel b).  Where portfolio_plan(T_m, B) == portfolio_plan(T_m, nJ * B),
        each J's outputs equal portfolio_multi_js's bit for bit."""
        if Lg.dim() != 3:
            raise ValueError("Lg must be [nJ][T_m][B * N]")
        nJ, T_m, BN = Lg.shape

        def run(N, Ks, Kmax, ws, legs, flag):
            _need(Lg, "Lg", torch.int8, (nJ, T_m, BN), self.device)
            _need(NR, "NR", torch.float64, (T_m, BN), self.device)
            w = ws()
            self._call("csm_cohort_sums_js_grouped", nJ, _ptr(Lg), _ptr(NR), T_m, int(B), N,
                       int(n_bins), Kmax, 1 if legs else 0, _ptr(w))
            return self._from_cohorts(Lg, None, T_m, nJ * B, N, n_bins, Ks, half_spread, k_impact,
                                      aum, None, None, with_costs, w, legs, flag, groups=(nJ, B))

        res, stacked = self._cohort_pass(T_m, BN, B, nJ * B, n_bins, Ks, legs_only, need_full, run)
        return (res, stacked) if return_stacked else res

    def portfolio_multi_grouped(self, Lg, NRg, n_bins=10, Ks=(1,), W=None, Bg=1,
                                half_spread=0.0005, k_impact=0.1, aum=0.0, ADV=None, SIG=None,
                                with_costs=True, workspace=None, return_stacked=False,
                                legs_only=False, need_full=None):
        """portfolio_multi of B = G * Bg panels stored group-major (csm_cohort_sums_grouped ->
        csm_portfolio_from_cohorts_grouped): Lg int8 / NRg f64 [G][T_m][Bg * N] (G blocks, e.g.
        the look-backs' label panels as one stacked decile pass writes them) and W / ADV / SIG
        [T_m][Bg * N] shared by the groups.  Outputs (panel g * Bg + p = group g's panel p) equal
        portfolio_multi(cat(Lg, 1), cat(NRg, 1), ..., W.repeat(1, G), B=G * Bg) bit for bit,
        without building those side-by-side copies."""
        if Lg.dim() != 3:
            raise ValueError("Lg must be [G][T_m][Bg * N]")
        G, T_m, BgN = Lg.shape

        def run(N, Ks, Kmax, ws, legs, flag):
            _need(Lg, "Lg", torch.int8, (G, T_m, BgN), self.device)
            _need(NRg, "NRg", torch.float64, (G, T_m, BgN), self.device)
            for t, nm in ((W, "W"), (ADV, "ADV"), (SIG, "SIG")):
                if t is not None:
                    _need(t, nm, torch.float64, (T_m, BgN), self.device)
            w = ws(workspace)
            self._call("csm_cohort_sums_grouped", G, _ptr(Lg), _ptr(NRg), _ptr(W), T_m, int(Bg), N,
                       int(n_bins), Kmax, 1 if legs else 0, _ptr(w))
            return self._from_cohorts(Lg, W, T_m, G * Bg, N, n_bins, Ks, half_spread, k_impact,
                                      aum, ADV, SIG, with_costs, w, legs, flag, groups=(G, Bg))

        res, stacked = self._cohort_pass(T_m, BgN, Bg, G * Bg, n_bins, Ks, legs_only, need_full,
                                         run, bname="Bg")
        return (res, stacked) if return_stacked else res

    def _from_cohorts(self, L, W, T_m, B, N, n_bins, Ks, half_spread, k_impact, aum, ADV, SIG,
                      with_costs, workspace, legs_only, need_full, groups=None):
        """The accounting half of portfolio_multi on a workspace holding the cohort sums ->
        (res {K: PortfolioOut}, stacked PortfolioOut).  groups=(G, Bg): the group-major layout
        of portfolio_multi_grouped."""
        nK = len(Ks)
        Kmax = max(Ks)
        PR, LS = self.empty((nK, T_m, B, n_bins)), self.empty((nK, T_m, B))
        TURN = self.empty((nK, T_m, B)) if with_costs else None
        COST = self.empty((nK, T_m, B)) if with_costs else None
        NET = self.empty((nK, T_m, B)) if with_costs else None
        ks = (ctypes.c_int32 * nK)(*Ks)
        args = (_ptr(L), _ptr(W), T_m, int(B), N, int(n_bins), Kmax, nK,
                ctypes.cast(ks, ctypes.c_void_p), float(half_spread), float(k_impact), float(aum),
                _ptr(ADV), _ptr(SIG), _ptr(PR), _ptr(LS), _ptr(TURN), _ptr(COST), _ptr(NET),
                _ptr(workspace))
        if groups is not None:
            G, Bg = groups
            gargs = (_ptr(L), _ptr(W), T_m, int(Bg)) + args[4:]
            self._call("csm_portfolio_from_cohorts_grouped", int(G), *gargs,
                       1 if legs_only else 0, _ptr(need_full) if legs_only else None)
        elif legs_only:
            self._call("csm_portfolio_from_cohorts_legs", *args, _ptr(need_full))
        else:
            self._call("csm_portfolio_from_cohorts_multi", *args)
        pick = lambda x, q: None if x is None else x[q]
        res = {K: PortfolioOut(PR=PR[q], LS=LS[q], TURN=pick(TURN, q), COST=pick(COST, q),
                               NET=pick(NET, q), legs_only=legs_only) for q, K in enumerate(Ks)}
        return res, PortfolioOut(PR=PR, LS=LS, TURN=TURN, COST=COST, NET=NET, legs_only=legs_only)

    def summary(self, LS, TURN=None, COST=None, NET=None, freq=12.0):
        """csm_summary: [nS][B][7] (months, mean, Sharpe, turnover, cost, net mean, net
        Sharpe) from stacked [nS][T_m][B] series (or one [T_m][B] series: nS = 1)."""
        if LS.dim() == 2:
            LS = LS.unsqueeze(0)
            TURN, COST, NET = (None if x is None else x.unsqueeze(0) for x in (TURN, COST, NET))
        nS, T_m, B = LS.shape
        for t, nm in ((LS, "LS"), (TURN, "TURN"), (COST, "COST"), (NET, "NET")):
            if t is not None:
                _need(t, nm, torch.float64, (nS, T_m, B), self.device)
        out = self.empty((nS, B, 7))
        self._call("csm_summary", _ptr(LS), _ptr(TURN), _ptr(COST), _ptr(NET), nS, T_m, B,
                   float(freq), _ptr(out))
        return out

    def _refuse_capture(self, what):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{what} is not supported under stream capture")

    def daily_returns(self, P, month_start, L, NR, n_bins=10, K=1, W=None, max_month_days=None,
                      out=None, workspace=None) -> DailyOut:
        """csm_daily_returns (rule E7): the daily return series of the n_bins portfolios and of
        top minus bottom for the labels L / next returns NR of the same panel (K overlapping
        cohorts, equal weights or W), one pass over P.  out = (DR, DLS, DCNT)."""
        self._refuse_capture("Engine.daily_returns")
        T_d, N = P.shape
        T_m = month_start.numel() - 1
        _need(P, "P", torch.float64, (T_d, N), self.device)
        _need(month_start, "month_start", torch.int64, (T_m + 1,), self.device)
        _need(L, "L", torch.int8, (T_m, N), self.device)
        _need(NR, "NR", torch.float64, (T_m, N), self.device)
        if W is not None:
            _need(W, "W", torch.float64, (T_m, N), self.device)
        if max_month_days is None:
            max_month_days, _ = self.month_days(month_start)
        if out is None:
            DR, DLS = self.empty((T_d, n_bins)), self.empty((T_d,))
            DCNT = self.empty((T_m, K, n_bins), torch.int32)
        else:
            DR, DLS, DCNT = out
            _need(DR, "DR", torch.float64, (T_d, n_bins), self.device)
            _need(DLS, "DLS", torch.float64, (T_d,), self.device)
            if DCNT is not None:
                _need(DCNT, "DCNT", torch.int32, (T_m, K, n_bins), self.device)
        nbytes = int(self.lib.csm_daily_workspace(T_d, N, T_m, int(n_bins), int(K)))
        if workspace is None or workspace.numel() * workspace.element_size() < nbytes:
            workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=self.device)
        self._call("csm_daily_returns", _ptr(P), T_d, N, _ptr(month_start), T_m,
                   int(max_month_days), _ptr(L), _ptr(NR), _ptr(W), int(n_bins), int(K), _ptr(DR),
                   _ptr(DLS), _ptr(DCNT), _ptr(workspace))
        return DailyOut(DR=DR, DLS=DLS, DCNT=DCNT)

    def series_stats(self, X, freq=252.0):
        """csm_series_stats: [nS][6] (count, mean, Sharpe, annualised volatility, maximum
        drawdown, final cumulative value) of the columns of X [T][nS] (or of one series [T]),
        NaN entries dropped."""
        self._refuse_capture("Engine.series_stats")
        if X.dim() == 1:
            X = X.unsqueeze(1)
        T, nS = X.shape
        _need(X, "X", torch.float64, (T, nS), self.device)
        out = self.empty((nS, 6))
        self._call("csm_series_stats", _ptr(X), nS, T, nS, float(freq), _ptr(out))
        return out

    def month_stats(self, P, month_start, max_month_days=None, out=None) -> MonthStats:
        """csm_month_stats (rule D1): one pass over P for each month's last, first and highest
        price and its sum of squared daily returns.  out = (PM, P1, HI, SSW, NDW)."""
        T_d, N = P.shape
        T_m = month_start.numel() - 1
        _need(P, "P", torch.float64, (T_d, N), self.device)
        _need(month_start, "month_start", torch.int64, (T_m + 1,), self.device)
        if max_month_days is None:
            max_month_days, _ = self.month_days(month_start)
        if out is None:
            PM, P1, HI, SSW = (self.empty((T_m, N)) for _ in range(4))
            NDW = self.empty((T_m, N), torch.int32)
        else:
            PM, P1, HI, SSW, NDW = out
            for t, name in ((PM, "PM"), (P1, "P1"), (HI, "HI"), (SSW, "SSW")):
                _need(t, name, torch.float64, (T_m, N), self.device)
            _need(NDW, "NDW", torch.int32, (T_m, N), self.device)
        self._call("csm_month_stats", _ptr(P), T_d, N, _ptr(month_start), T_m,
                   int(max_month_days), _ptr(PM), _ptr(P1), _ptr(HI), _ptr(SSW), _ptr(NDW))
        return MonthStats(PM, P1, HI, SSW, NDW)

    SIGNAL_OUTPUTS = ("SS", "ND", "H52", "RV", "MS", "NR_H52", "NR_MS")

    def window_signals(self, PM, P1, HI, SSW, NDW, M=None, Jh=12, Jv=12, min_obs=None,
                       outputs=None) -> SignalsOut:
        """csm_window_signals (rules D2..D6) on month_stats' outputs: the 52-week high H52 over
        Jh months, the realised daily volatility RV over Jv months (portfolio's SIG), MS = M / RV
        for a momentum M, and the next returns of the H52 and MS rankings.  min_obs (daily
        returns a window needs) defaults to 10 * Jv.  outputs: the SignalsOut fields to compute
        (default: all; MS and NR_MS only with M)."""
        T_m, N = PM.shape
        for t, name in ((PM, "PM"), (P1, "P1"), (HI, "HI"), (SSW, "SSW")):
            _need(t, name, torch.float64, (T_m, N), self.device)
        _need(NDW, "NDW", torch.int32, (T_m, N), self.device)
        if M is not None:
            _need(M, "M", torch.float64, (T_m, N), self.device)
        if outputs is None:
            outputs = tuple(k for k in self.SIGNAL_OUTPUTS
                            if M is not None or k not in ("MS", "NR_MS"))
        unknown = set(outputs) - set(self.SIGNAL_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        min_obs = 10 * int(Jv) if min_obs is None else int(min_obs)
        o = {k: self.empty((T_m, N), torch.int32 if k == "ND" else torch.float64)
             for k in outputs}
        self._call("csm_window_signals", _ptr(PM), _ptr(P1), _ptr(HI), _ptr(SSW), _ptr(NDW),
                   _ptr(M), T_m, N, int(Jh), int(Jv), min_obs,
                   *(_ptr(o.get(k)) for k in self.SIGNAL_OUTPUTS))
        return SignalsOut(**o)

    def market_factor(self, PM, min_assets=1, with_x=False):
        """csm_market_factor (rules B1, B2): the equal-weight market return MKT [T_m] of the
        month returns x over calendar-adjacent priced months, and NMK [T_m] (int32) the assets
        behind each.  Returns (MKT, NMK), or (MKT, NMK, X) with_x."""
        T_m, N = PM.shape
        _need(PM, "PM", torch.float64, (T_m, N), self.device)
        MKT = self.empty((T_m,))
        NMK = self.empty((T_m,), torch.int32)
        X = self.empty((T_m, N)) if with_x else None
        self._call("csm_market_factor", _ptr(PM), T_m, N, int(min_assets), _ptr(X), _ptr(MKT),
                   _ptr(NMK))
        return (MKT, NMK, X) if with_x else (MKT, NMK)

    MARKET_OUTPUTS = ("BETA", "ALPHA", "IVOL", "RESMOM", "NOBS")

    def market_model(self, PM, F=None, window=36, J=12, skip=1, min_obs=None,
                     outputs=None) -> MarketModelOut:
        """csm_market_model (rules B3..B5): each asset's month returns regressed on the factor F
        [T_m] over `window` calendar months -- BETA, ALPHA, the idiosyncratic volatility IVOL, the
        residual momentum RESMOM over the J months that end `skip` months back, and NOBS.  F None:
        market_factor's MKT.  min_obs defaults to max(2, ceil(2 * window / 3)).  outputs: the
        MarketModelOut fields to compute (default: all)."""
        T_m, N = PM.shape
        _need(PM, "PM", torch.float64, (T_m, N), self.device)
        if F is None:
            F, _ = self.market_factor(PM)
        _need(F, "F", torch.float64, (T_m,), self.device)
        outputs = self.MARKET_OUTPUTS if outputs is None else tuple(outputs)
        unknown = set(outputs) - set(self.MARKET_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        window = int(window)
        min_obs = max(2, -(-2 * window // 3)) if min_obs is None else int(min_obs)
        o = {k: self.empty((T_m, N), torch.int32 if k == "NOBS" else torch.float64)
             for k in outputs}
        self._call("csm_market_model", _ptr(PM), _ptr(F), T_m, N, window, int(J), int(skip),
                   min_obs, *(_ptr(o.get(k)) for k in self.MARKET_OUTPUTS))
        return MarketModelOut(F=F, **o)

    def next_ret(self, PM, S, out=None):
        """csm_next_ret (rule B6): the next return NR [T_m][N] of any signal S [T_m][N], which
        deciles and portfolio then rank on."""
        T_m, N = PM.shape
        _need(PM, "PM", torch.float64, (T_m, N), self.device)
        _need(S, "S", torch.float64, (T_m, N), self.device)
        NR = self.empty((T_m, N)) if out is None else out
        _need(NR, "NR", torch.float64, (T_m, N), self.device)
        self._call("csm_next_ret", _ptr(PM), _ptr(S), T_m, N, _ptr(NR))
        return NR

    def daily_market(self, P, max_gap=10, min_assets=1, workspace=None):
        """csm_daily_market (rules V1, V2): the equal-weight market return MKTD [T_d] of the daily
        returns (a return reaches back over at most max_gap rows without a price) and NMD [T_d]
        (int32), the assets behind each.  Returns (MKTD, NMD)."""
        T_d, N = P.shape
        _need(P, "P", torch.float64, (T_d, N), self.device)
        MKTD = self.empty((T_d,))
        NMD = self.empty((T_d,), torch.int32)
        nbytes = int(self.lib.csm_daily_market_workspace(T_d, N))
        if workspace is None or workspace.numel() * workspace.element_size() < nbytes:
            workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=self.device)
        self._call("csm_daily_market", _ptr(P), T_d, N, int(max_gap), int(min_assets), _ptr(MKTD),
                   _ptr(NMD), _ptr(workspace))
        return MKTD, NMD

    def daily_sums(self, P, month_start, FD, max_gap=10, max_month_days=None,
                   with_sr3=True, with_rmax=True) -> DailySums:
        """csm_daily_sums (rule V3): one pass over P for each (month, asset)'s raw moment sums of
        its daily returns and the factor FD [T_d] (daily_market's MKTD, or any series)."""
        T_d, N = P.shape
        T_m = month_start.numel() - 1
        _need(P, "P", torch.float64, (T_d, N), self.device)
        _need(month_start, "month_start", torch.int64, (T_m + 1,), self.device)
        _need(FD, "FD", torch.float64, (T_d,), self.device)
        if max_month_days is None:
            max_month_days, _ = self.month_days(month_start)
        NO = self.empty((T_m, N), torch.int32)
        SR, SF, SRR, SFF, SRF = (self.empty((T_m, N)) for _ in range(5))
        SR3 = self.empty((T_m, N)) if with_sr3 else None
        RMAX = self.empty((T_m, N)) if with_rmax else None
        self._call("csm_daily_sums", _ptr(P), _ptr(FD), T_d, N, _ptr(month_start), T_m,
                   int(max_month_days), int(max_gap), _ptr(NO), _ptr(SR), _ptr(SF), _ptr(SRR),
                   _ptr(SFF), _ptr(SRF), _ptr(SR3), _ptr(RMAX))
        return DailySums(NO, SR, SF, SRR, SFF, SRF, SR3, RMAX)

    DAILY_OUTPUTS = ("DBETA", "DIVOL", "DTVOL", "DSKEW", "DMAX", "NOBS")

    def daily_model(self, sums: DailySums, window=1, min_obs=None, outputs=None) -> DailyModelOut:
        """csm_daily_model (rule V4) on daily_sums' panels over `window` calendar months (1..12):
        the daily beta DBETA, idiosyncratic volatility DIVOL, total volatility DTVOL, skewness
        DSKEW, the largest daily return DMAX and NOBS.  min_obs counts days (default 15 * window).
        outputs: the DailyModelOut fields to compute (default: all the sums given allow)."""
        T_m, N = sums.SR.shape
        _need(sums.NO, "NO", torch.int32, (T_m, N), self.device)
        for k in ("SR", "SF", "SRR", "SFF", "SRF", "SR3", "RMAX"):
            t = getattr(sums, k)
            if t is not None:
                _need(t, k, torch.float64, (T_m, N), self.device)
        if outputs is None:
            outputs = tuple(k for k in self.DAILY_OUTPUTS
                            if not (k == "DSKEW" and sums.SR3 is None)
                            and not (k == "DMAX" and sums.RMAX is None))
        unknown = set(outputs) - set(self.DAILY_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        window = int(window)
        min_obs = 15 * window if min_obs is None else int(min_obs)
        o = {k: self.empty((T_m, N), torch.int32 if k == "NOBS" else torch.float64)
             for k in outputs}
        self._call("csm_daily_model", *(_ptr(t) for t in sums), T_m, N, window, min_obs,
                   *(_ptr(o.get(k)) for k in self.DAILY_OUTPUTS))
        return DailyModelOut(**o)

    FACTOR_OUTPUTS = ("BETA", "ALPHA", "IVOL", "RESMOM", "R2", "NOBS")

    def _factors(self, F, T, name):
        """A [T] or [T][KF] factor panel as [T][KF] (a 1-D series means KF = 1)."""
        if F.dim() == 1:
            F = F.unsqueeze(1)
        if F.dim() != 2 or not 1 <= F.shape[1] <= 4:
            raise ValueError(f"{name} must be [{T}] or [{T}][KF] with 1 <= KF <= 4, "
                             f"got {tuple(F.shape)}")
        _need(F, name, torch.float64, (T, F.shape[1]), self.device)
        return F

    def factor_model(self, PM, F, window=36, J=12, skip=1, min_obs=None,
                     outputs=None) -> FactorModelOut:
        """csm_factor_model (rules MF1..MF5): each asset's month returns regressed on the KF
        factors F [T_m][KF] (1 <= KF <= 4; a 1-D F means KF = 1) over `window` calendar months --
        BETA [KF][T_m][N], ALPHA, the idiosyncratic volatility IVOL, the residual momentum RESMOM
        over the J months that end `skip` months back, R2 and NOBS.  A month with a NaN in any
        factor column is no observation.  min_obs defaults to max(KF + 1, ceil(2 * window / 3)).
        outputs: the FactorModelOut fields to compute (default: all).  At KF = 1 the shared
        outputs are market_model's bit for bit."""
        T_m, N = PM.shape
        _need(PM, "PM", torch.float64, (T_m, N), self.device)
        F = self._factors(F, T_m, "F")
        KF = F.shape[1]
        outputs = self.FACTOR_OUTPUTS if outputs is None else tuple(outputs)
        unknown = set(outputs) - set(self.FACTOR_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        window = int(window)
        min_obs = max(KF + 1, -(-2 * window // 3)) if min_obs is None else int(min_obs)
        o = {k: self.empty((KF, T_m, N) if k == "BETA" else (T_m, N),
                           torch.int32 if k == "NOBS" else torch.float64) for k in outputs}
        self._call("csm_factor_model", _ptr(PM), _ptr(F), T_m, N, KF, window, int(J), int(skip),
                   min_obs, *(_ptr(o.get(k)) for k in self.FACTOR_OUTPUTS))
        return FactorModelOut(F=F, **o)

    def daily_fsums(self, P, month_start, FD, max_gap=10, max_month_days=None) -> DailyFSums:
        """csm_daily_fsums (rule MF6): one pass over P for each (month, asset)'s raw moment sums
        of its daily returns and the KF daily factors FD [T_d][KF] (a 1-D FD means KF = 1)."""
        T_d, N = P.shape
        T_m = month_start.numel() - 1
        _need(P, "P", torch.float64, (T_d, N), self.device)
        _need(month_start, "month_start", torch.int64, (T_m + 1,), self.device)
        FD = self._factors(FD, T_d, "FD")
        KF = FD.shape[1]
        if max_month_days is None:
            max_month_days, _ = self.month_days(month_start)
        NO = self.empty((T_m, N), torch.int32)
        SR, SRR = self.empty((T_m, N)), self.empty((T_m, N))
        SF, SRF = self.empty((KF, T_m, N)), self.empty((KF, T_m, N))
        SFF = self.empty((KF * (KF + 1) // 2, T_m, N))
        self._call("csm_daily_fsums", _ptr(P), _ptr(FD), T_d, N, KF, _ptr(month_start), T_m,
                   int(max_month_days), int(max_gap), _ptr(NO), _ptr(SR), _ptr(SRR), _ptr(SF),
                   _ptr(SRF), _ptr(SFF))
        return DailyFSums(NO, SR, SRR, SF, SRF, SFF)

    DAILY_FACTOR_OUTPUTS = ("DBETA", "DALPHA", "DIVOL", "DR2", "NOBS")

    def daily_fmodel(self, sums: DailyFSums, window=1, min_obs=None,
                     outputs=None) -> DailyFModelOut:
        """csm_daily_fmodel (rule MF7) on daily_fsums' panels over `window` calendar months
        (1..12): the slopes DBETA [KF][T_m][N], the intercept DALPHA, the idiosyncratic volatility
        DIVOL, DR2 and NOBS.  min_obs counts days (default max(15 * window, KF + 1)).  outputs:
        the DailyFModelOut fields to compute (default: all).  The Dimson beta is DBETA.sum(0) of
        a model on lagged(MKTD, lags)."""
        T_m, N = sums.SR.shape
        KF = sums.SF.shape[0]
        _need(sums.NO, "NO", torch.int32, (T_m, N), self.device)
        for k, lead in (("SR", ()), ("SRR", ()), ("SF", (KF,)), ("SRF", (KF,)),
                        ("SFF", (KF * (KF + 1) // 2,))):
            _need(getattr(sums, k), k, torch.float64, (*lead, T_m, N), self.device)
        outputs = self.DAILY_FACTOR_OUTPUTS if outputs is None else tuple(outputs)
        unknown = set(outputs) - set(self.DAILY_FACTOR_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        window = int(window)
        min_obs = max(15 * window, KF + 1) if min_obs is None else int(min_obs)
        o = {k: self.empty((KF, T_m, N) if k == "DBETA" else (T_m, N),
                           torch.int32 if k == "NOBS" else torch.float64) for k in outputs}
        self._call("csm_daily_fmodel", *(_ptr(t) for t in sums), T_m, N, KF, window, min_obs,
                   *(_ptr(o.get(k)) for k in self.DAILY_FACTOR_OUTPUTS))
        return DailyFModelOut(**o)

    def liq_sums(self, P, V, month_start, max_gap=10, max_month_days=None, with_sv=True,
                 with_nzr=True, with_nzv=True) -> LiqSums:
        """csm_liq_sums (rules Q1, Q2): one pass over the daily prices P and volumes V for each
        (month, asset)'s priced, return and Amihud day counts, its volume and dollar volume sums
        and its sum of |r| / dollar volume."""
        T_d, N = P.shape
        T_m = month_start.numel() - 1
        _need(P, "P", torch.float64, (T_d, N), self.device)
        _need(V, "V", torch.float64, (T_d, N), self.device)
        _need(month_start, "month_start", torch.int64, (T_m + 1,), self.device)
        if max_month_days is None:
            max_month_days, _ = self.month_days(month_start)
        NP, ND, NA = (self.empty((T_m, N), torch.int32) for _ in range(3))
        NZR = self.empty((T_m, N), torch.int32) if with_nzr else None
        NZV = self.empty((T_m, N), torch.int32) if with_nzv else None
        SV = self.empty((T_m, N)) if with_sv else None
        SDV, SIL = self.empty((T_m, N)), self.empty((T_m, N))
        self._call("csm_liq_sums", _ptr(P), _ptr(V), T_d, N, _ptr(month_start), T_m,
                   int(max_month_days), int(max_gap), _ptr(NP), _ptr(ND), _ptr(NA), _ptr(NZR),
                   _ptr(NZV), _ptr(SV), _ptr(SDV), _ptr(SIL))
        return LiqSums(NP, ND, NA, NZR, NZV, SV, SDV, SIL)

    LIQ_OUTPUTS = ("ILLIQ", "DVOL", "TURN", "ZRET", "ZVOL", "NOBS")

    def liq_model(self, sums: LiqSums, window=12, min_obs=None, scale=1e6, SH=None,
                  outputs=None) -> LiqModelOut:
        """csm_liq_model (rule Q3) on liq_sums' panels over `window` calendar months (1..12):
        Amihud's ILLIQ (times scale), the dollar average daily volume DVOL (portfolio's ADV), the
        turnover TURN on the shares outstanding SH [T_m][N], the shares of zero-return and
        zero-volume days ZRET and ZVOL, and NOBS.  min_obs counts days (default 15 * window).
        outputs: the LiqModelOut fields to compute (default: all the sums and SH given allow)."""
        T_m, N = sums.SDV.shape
        for k in ("NP", "ND", "NA", "NZR", "NZV"):
            t = getattr(sums, k)
            if t is not None:
                _need(t, k, torch.int32, (T_m, N), self.device)
        for k in ("SV", "SDV", "SIL"):
            t = getattr(sums, k)
            if t is not None:
                _need(t, k, torch.float64, (T_m, N), self.device)
        if SH is not None:
            _need(SH, "SH", torch.float64, (T_m, N), self.device)
        if outputs is None:
            outputs = tuple(k for k in self.LIQ_OUTPUTS
                            if not (k == "TURN" and (SH is None or sums.SV is None))
                            and not (k == "ZRET" and sums.NZR is None)
                            and not (k == "ZVOL" and sums.NZV is None))
        unknown = set(outputs) - set(self.LIQ_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        window = int(window)
        min_obs = 15 * window if min_obs is None else int(min_obs)
        o = {k: self.empty((T_m, N), torch.int32 if k == "NOBS" else torch.float64)
             for k in outputs}
        self._call("csm_liq_model", *(_ptr(t) for t in sums), _ptr(SH), T_m, N, window, min_obs,
                   float(scale), *(_ptr(o.get(k)) for k in self.LIQ_OUTPUTS))
        return LiqModelOut(**o)

    def range_sums(self, H, L, C, month_start, max_gap=1, max_month_days=None, with_cs=True,
                   with_ar=True) -> RangeSums:
        """csm_range_sums (rules HL1..HL5): one pass over the daily high, low and close panels
        for each (month, asset)'s ranged days and pairs, its sum of squared log ranges and, with
        with_cs / with_ar, its Corwin-Schultz and Abdi-Ranaldo sums."""
        T_d, N = H.shape
        T_m = month_start.numel() - 1
        for t, k in ((H, "H"), (L, "L"), (C, "C")):
            _need(t, k, torch.float64, (T_d, N), self.device)
        _need(month_start, "month_start", torch.int64, (T_m + 1,), self.device)
        if max_month_days is None:
            max_month_days, _ = self.month_days(month_start)
        NRG, NPR = self.empty((T_m, N), torch.int32), self.empty((T_m, N), torch.int32)
        NCS = self.empty((T_m, N), torch.int32) if with_cs else None
        SPK = self.empty((T_m, N))
        SCS = self.empty((T_m, N)) if with_cs else None
        SAR = self.empty((T_m, N)) if with_ar else None
        self._call("csm_range_sums", _ptr(H), _ptr(L), _ptr(C), T_d, N, _ptr(month_start), T_m,
                   int(max_month_days), int(max_gap), _ptr(NRG), _ptr(NPR), _ptr(NCS), _ptr(SPK),
                   _ptr(SCS), _ptr(SAR))
        return RangeSums(NRG, NPR, NCS, SPK, SCS, SAR)

    RANGE_OUTPUTS = ("PKVOL", "CSSPR", "ARSPR", "NOBS")

    def range_model(self, sums: RangeSums, window=1, min_obs=None, outputs=None) -> RangeModelOut:
        """csm_range_model (rule HL6) on range_sums' panels over `window` calendar months
        (1..12): Parkinson's daily volatility PKVOL (portfolio's SIG), the Corwin-Schultz and
        Abdi-Ranaldo spreads CSSPR and ARSPR, and NOBS.  min_obs counts days (default 15 *
        window).  outputs: the RangeModelOut fields to compute (default: all the sums given
        allow)."""
        T_m, N = sums.SPK.shape
        for k in ("NRG", "NPR", "NCS"):
            t = getattr(sums, k)
            if t is not None:
                _need(t, k, torch.int32, (T_m, N), self.device)
        for k in ("SPK", "SCS", "SAR"):
            t = getattr(sums, k)
            if t is not None:
                _need(t, k, torch.float64, (T_m, N), self.device)
        if outputs is None:
            outputs = tuple(k for k in self.RANGE_OUTPUTS
                            if not (k == "CSSPR" and (sums.NCS is None or sums.SCS is None))
                            and not (k == "ARSPR" and sums.SAR is None))
        unknown = set(outputs) - set(self.RANGE_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        window = int(window)
        min_obs = 15 * window if min_obs is None else int(min_obs)
        o = {k: self.empty((T_m, N), torch.int32 if k == "NOBS" else torch.float64)
             for k in outputs}
        self._call("csm_range_model", *(_ptr(t) for t in sums), T_m, N, window, min_obs,
                   4.0 * math.log(2.0), *(_ptr(o.get(k)) for k in self.RANGE_OUTPUTS))
        return RangeModelOut(**o)

    def asym_sums(self, P, month_start, FD=None, side=-1, max_gap=10,
                  max_month_days=None) -> AsymSums:
        """csm_asym_sums (rules AS1, AS2): one pass over the daily prices P for each (month,
        asset)'s return days by the sign of the return and their squared returns and, with a
        daily series FD [T_d] (daily_market's, or any other), the market-model sums over the days
        with FD < 0 (side -1) or FD > 0 (side +1)."""
        T_d, N = P.shape
        T_m = month_start.numel() - 1
        _need(P, "P", torch.float64, (T_d, N), self.device)
        _need(month_start, "month_start", torch.int64, (T_m + 1,), self.device)
        if FD is not None:
            _need(FD, "FD", torch.float64, (T_d,), self.device)
        if max_month_days is None:
            max_month_days, _ = self.month_days(month_start)
        ND, NUP, NDN = (self.empty((T_m, N), torch.int32) for _ in range(3))
        SUP, SDN = self.empty((T_m, N)), self.empty((T_m, N))
        NB = BR = BF = BFF = BRF = None
        if FD is not None:
            NB = self.empty((T_m, N), torch.int32)
            BR, BF, BFF, BRF = (self.empty((T_m, N)) for _ in range(4))
        self._call("csm_asym_sums", _ptr(P), _ptr(FD), T_d, N, _ptr(month_start), T_m,
                   int(max_month_days), int(max_gap), int(side), _ptr(ND), _ptr(NUP), _ptr(NDN),
                   _ptr(SUP), _ptr(SDN), _ptr(NB), _ptr(BR), _ptr(BF), _ptr(BFF), _ptr(BRF))
        return AsymSums(ND, NUP, NDN, SUP, SDN, NB, BR, BF, BFF, BRF)

    ASYM_OUTPUTS = ("ID", "RSJ", "DSVOL", "DNBETA", "NOBS", "NSIDE")

    def asym_model(self, sums: AsymSums, window=12, skip=0, M=None, min_obs=None, min_side=None,
                   outputs=None) -> AsymModelOut:
        """csm_asym_model (rule AS3) on asym_sums' panels over the `window` calendar months
        (1..36) that end `skip` months back (0..12): the information discreteness ID, signed by
        the formation return M [T_m][N] (mom_J with J = window and the same skip), the signed
        jump variation RSJ, the downside semi-volatility DSVOL, the side beta DNBETA, NOBS and
        NSIDE.  min_obs counts return days (default 15 * window), min_side side days (default
        max(2, 5 * window)).  outputs: the AsymModelOut fields to compute (default: all the sums
        and M given allow)."""
        T_m, N = sums.SUP.shape
        for k in ("ND", "NUP", "NDN", "NB"):
            t = getattr(sums, k)
            if t is not None:
                _need(t, k, torch.int32, (T_m, N), self.device)
        for k in ("SUP", "SDN", "BR", "BF", "BFF", "BRF"):
            t = getattr(sums, k)
            if t is not None:
                _need(t, k, torch.float64, (T_m, N), self.device)
        if M is not None:
            _need(M, "M", torch.float64, (T_m, N), self.device)
        if outputs is None:
            outputs = tuple(k for k in self.ASYM_OUTPUTS
                            if not (k == "ID" and M is None)
                            and not (k in ("DNBETA", "NSIDE") and sums.NB is None))
        unknown = set(outputs) - set(self.ASYM_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        window = int(window)
        min_obs = 15 * window if min_obs is None else int(min_obs)
        min_side = max(2, 5 * window) if min_side is None else int(min_side)
        o = {k: self.empty((T_m, N), torch.int32 if k in ("NOBS", "NSIDE") else torch.float64)
             for k in outputs}
        self._call("csm_asym_model", *(_ptr(t) for t in sums), _ptr(M), T_m, N, window, int(skip),
                   min_obs, min_side, *(_ptr(o.get(k)) for k in self.ASYM_OUTPUTS))
        return AsymModelOut(**o)

    @staticmethod
    def lagged(F, lags):
        """[T][1 + lags]: column k is the series F [T] shifted down k rows, NaN in its first k
        rows.  The Dimson (1979) beta with `lags` lags is DBETA.sum(0) of
        daily_fmodel(daily_fsums(P, month_start, lagged(MKTD, lags)))."""
        lags = int(lags)
        if F.dim() != 1 or lags < 0:
            raise ValueError("lagged takes a 1-D series and lags >= 0")
        out = torch.full((F.shape[0], 1 + lags), float("nan"), dtype=F.dtype, device=F.device)
        for k in range(1 + lags):
            out[k:, k] = F[:F.shape[0] - k]
        return out

    def xs_regress(self, Y, signals, W=None, standardize=False, ridge=0.0,
                   min_obs=None) -> XsRegressOut:
        """csm_xs_regress (rules R1..R5): each month's regression of Y [T_m][N] on the K signals
        (a sequence of [T_m][N] tensors, 1 <= K <= 8) across the assets -- OLS, WLS with weights
        W, and with standardize / ridge the reference's StandardScaler + Ridge on the month's
        cross-section.  min_obs defaults to K + 2."""
        signals = list(signals)
        T_m, N = Y.shape
        _need(Y, "Y", torch.float64, (T_m, N), self.device)
        for k, S in enumerate(signals):
            _need(S, f"signals[{k}]", torch.float64, (T_m, N), self.device)
        if W is not None:
            _need(W, "W", torch.float64, (T_m, N), self.device)
        K = len(signals)
        min_obs = K + 2 if min_obs is None else int(min_obs)
        GAMMA = self.empty((T_m, K + 1))
        R2 = self.empty((T_m,))
        NOBS = self.empty((T_m,), torch.int32)
        ptrs = (ctypes.c_void_p * max(K, 1))(*[S.data_ptr() for S in signals])
        self._call("csm_xs_regress", _ptr(Y), ptrs, K, _ptr(W), T_m, N, int(bool(standardize)),
                   float(ridge), min_obs, _ptr(GAMMA), _ptr(R2), _ptr(NOBS))
        return XsRegressOut(GAMMA=GAMMA, R2=R2, NOBS=NOBS)

    @staticmethod
    def default_lags(T):
        """The Newey-West lag rule floor(4 (T / 100)^(2/9))."""
        return int(np.floor(4.0 * (T / 100.0) ** (2.0 / 9.0)))

    def newey_west(self, G, lags=None) -> NeweyWestOut:
        """csm_newey_west (rule R6): the time-series mean of each column of G [T][C] (or of one
        series [T]) over its non-NaN entries, its Newey-West standard error (Bartlett kernel) and
        t-statistic.  lags defaults to floor(4 (T / 100)^(2/9)).  G is any per-month series:
        xs_regress's GAMMA, PipelineOut.EW / LS, PortfolioOut.LS."""
        one = G.dim() == 1
        G2 = G.unsqueeze(1) if one else G
        T, C = G2.shape
        _need(G2, "G", torch.float64, (T, C), self.device)
        lags = self.default_lags(T) if lags is None else int(lags)
        MEAN, SE, TS = (self.empty((C,)) for _ in range(3))
        NT = self.empty((C,), torch.int32)
        self._call("csm_newey_west", _ptr(G2), T, C, C, lags, _ptr(MEAN), _ptr(SE), _ptr(TS),
                   _ptr(NT))
        if one:
            MEAN, SE, TS, NT = MEAN[0], SE[0], TS[0], NT[0]
        return NeweyWestOut(MEAN=MEAN, SE=SE, T=TS, NT=NT)

    def fama_macbeth(self, Y, signals, W=None, standardize=True, ridge=0.0, min_obs=None,
                     lags=None) -> FamaMacBethOut:
        """Fama-MacBeth: xs_regress per month, then newey_west over GAMMA's K + 1 columns and the
        mean of R2, chained on the device."""
        r = self.xs_regress(Y, signals, W, standardize, ridge, min_obs)
        lags = self.default_lags(Y.shape[0]) if lags is None else int(lags)
        nw = self.newey_west(r.GAMMA, lags)
        r2 = self.newey_west(r.R2, lags)
        return FamaMacBethOut(GAMMA=r.GAMMA, R2=r.R2, NOBS=r.NOBS, MEAN=nw.MEAN, SE=nw.SE, T=nw.T,
                              NT=nw.NT, R2_MEAN=r2.MEAN, lags=lags)

    # ------------------------------------------------------------------ ranks and ICs
    RANK_METHODS = {"average": 0, "min": 1, "max": 2}

    def xs_rank(self, S, GID=None, n_groups=1, method="average", pct=False, out=None,
                with_nvg=False):
        """csm_xs_rank (rules I1, I2): the rank of S [T_m][N] inside each date, or with GID (int16
        [T_m][N] or a static [N]) inside each (date, group) -- pandas' rank(method='average' |
        'min' | 'max', pct=pct); NaN outside every group.  with_nvg: returns (RANK, NVG) with the
        member counts [T_m][n_groups]."""
        T_m, N = S.shape
        _need(S, "S", torch.float64, (T_m, N), self.device)
        if method not in self.RANK_METHODS:
            raise ValueError(f"method must be one of {tuple(self.RANK_METHODS)}, got {method!r}")
        g_ld = 0
        if GID is not None:
            GID, g_ld = self._group_ids(GID, T_m, N)
        G = int(n_groups)
        RANK = self.empty((T_m, N)) if out is None else out
        _need(RANK, "out", torch.float64, (T_m, N), self.device)
        NVG = self.empty((T_m, max(G, 1)), torch.int32) if with_nvg else None
        self._call("csm_xs_rank", _ptr(S), _ptr(GID), g_ld, T_m, N, G, self.RANK_METHODS[method],
                   int(bool(pct)), _ptr(RANK), _ptr(NVG))
        return (RANK, NVG) if with_nvg else RANK

    def rank_ic(self, S, Y, lead=0, min_obs=10, pearson=True) -> RankICOut:
        """csm_rank_ic (rules I3..I6): per month t the Spearman rank correlation RIC, and with
        pearson the Pearson correlation PIC, of S[t] with Y[t + lead] across the assets where
        both are not NaN; NaN with fewer than min_obs of them or no variation."""
        T_m, N = S.shape
        _need(S, "S", torch.float64, (T_m, N), self.device)
        _need(Y, "Y", torch.float64, (T_m, N), self.device)
        RIC = self.empty((T_m,))
        PIC = self.empty((T_m,)) if pearson else None
        NOBS = self.empty((T_m,), torch.int32)
        self._call("csm_rank_ic", _ptr(S), _ptr(Y), T_m, N, int(lead), int(min_obs), _ptr(RIC),
                   _ptr(PIC), _ptr(NOBS))
        return RankICOut(RIC=RIC, PIC=PIC, NOBS=NOBS)

    def ic_decay(self, S, X, horizons=(1, 2, 3, 6, 12), min_obs=10, lags=None) -> ICDecayOut:
        """The IC of S at each horizon h: rank_ic(S, X, lead=h), stacked [H][T_m], and one
        newey_west over the H series.  With X the month return (rule B1) horizon h is the return
        of the h-th month after formation."""
        hs = tuple(int(h) for h in horizons)
        if not hs:
            raise ValueError("horizons is empty")
        r = [self.rank_ic(S, X, lead=h, min_obs=min_obs) for h in hs]
        RIC = torch.stack([o.RIC for o in r])
        lags = self.default_lags(S.shape[0]) if lags is None else int(lags)
        nw = self.newey_west(RIC.t().contiguous(), lags)
        return ICDecayOut(RIC=RIC, PIC=torch.stack([o.PIC for o in r]),
                          NOBS=torch.stack([o.NOBS for o in r]), MEAN=nw.MEAN, SE=nw.SE, T=nw.T,
                          NT=nw.NT, horizons=hs, lags=lags)

    # ------------------------------------------------------------------ within-group sorts
    def _side_panel(self, X, name, dtypes, T_m, N, what):
        """A side panel of a [T_m][N] call: [T_m][N] (one row per month) or [N] (static), of one
        of dtypes; returns (X, its leading dimension: N or 0)."""
        if not isinstance(X, torch.Tensor) or X.dtype not in dtypes:
            raise TypeError(f"{name} must be {what}")
        static = X.dim() == 1
        _need(X, name, X.dtype, (N,) if static else (T_m, N), self.device)
        return X, 0 if static else N

    def _group_ids(self, GID, T_m, N):
        """GID as csm_group_* takes it: int16 [T_m][N] or [N]; returns (GID, g_ld)."""
        return self._side_panel(GID, "GID", (torch.int16,), T_m, N,
                                "an int16 torch tensor (labels: L.to(torch.int16))")

    def deciles_within(self, S, NR, GID, n_groups, n_bins=10, min_group=1, with_groups=False,
                       with_nv=False):
        """csm_group_deciles (rules N1..N3): the qcut labels of S inside each group of each date
        -- sector-neutral deciles; with a first sort's labels as GID the dependent double sort --
        and, with NR, the pooled decile means.  GID: int16 [T_m][N] or a static [N]; an id outside
        [0, n_groups) means no group; a group with fewer than min_group members is not ranked.
        Returns (L, EW, CNT[, NV][, EWG, CNTG, NVG]); EW / CNT / EWG / CNTG are None without NR."""
        T_m, N = S.shape
        _need(S, "S", torch.float64, (T_m, N), self.device)
        if NR is not None:
            _need(NR, "NR", torch.float64, (T_m, N), self.device)
        GID, g_ld = self._group_ids(GID, T_m, N)
        G, nb = int(n_groups), int(n_bins)
        L = self.empty((T_m, N), torch.int8)
        EW = self.empty((T_m, nb)) if NR is not None else None
        CNT = self.empty((T_m, nb), torch.int32) if NR is not None else None
        NV = self.empty((T_m,), torch.int32) if with_nv else None
        grp = with_groups and NR is not None and G >= 1
        EWG = self.empty((T_m, G, nb)) if grp else None
        CNTG = self.empty((T_m, G, nb), torch.int32) if grp else None
        NVG = self.empty((T_m, max(G, 1)), torch.int32) if with_groups else None
        self._call("csm_group_deciles", _ptr(S), _ptr(NR), _ptr(GID), g_ld, T_m, N, G, nb,
                   _qptr(nb), int(min_group), _ptr(L), _ptr(EW), _ptr(CNT), _ptr(NV), _ptr(EWG),
                   _ptr(CNTG), _ptr(NVG))
        out = (L, EW, CNT)
        if with_nv:
            out += (NV,)
        if with_groups:
            out += (EWG, CNTG, NVG)
        return out

    GROUP_OUTPUTS = ("GMEAN", "GSD", "GCNT", "SA", "SZ", "SB")

    def group_stats(self, S, GID, n_groups, outputs=None) -> GroupStatsOut:
        """csm_group_stats (rules N4, N5): each group's mean, standard deviation and member count
        per date, and per member the demeaned signal SA, the z-score SZ and the group's mean SB.
        outputs: the GroupStatsOut fields to compute (default: all)."""
        T_m, N = S.shape
        _need(S, "S", torch.float64, (T_m, N), self.device)
        GID, g_ld = self._group_ids(GID, T_m, N)
        outputs = self.GROUP_OUTPUTS if outputs is None else tuple(outputs)
        unknown = set(outputs) - set(self.GROUP_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        G = int(n_groups)
        o = {k: self.empty((T_m, max(G, 1)) if k[0] == "G" else (T_m, N),
                           torch.int32 if k == "GCNT" else torch.float64) for k in outputs}
        self._call("csm_group_stats", _ptr(S), _ptr(GID), g_ld, T_m, N, G,
                   *(_ptr(o.get(k)) for k in self.GROUP_OUTPUTS))
        return GroupStatsOut(**o)

    def _signal_panels(self, P, month_start, signal, J, skip, n_bins, window, min_obs, V=None,
                       HLC=None):
        """(PM, S, NR) of a signal name: "mom" as run builds it, the others as run_signal does."""
        if signal == "mom":
            PM, _ = self.month_end(P, month_start)
            T_m, N = PM.shape
            if self.default_chunks(T_m, N, J, skip) > 1:
                _, S, NR = self.momentum_chunked(PM, J, skip)
            else:
                _, S, NR = self.momentum(PM, J, skip)
        else:
            r = self.run_signal(P, month_start, signal, J, skip, n_bins, window, min_obs, V=V,
                                HLC=HLC)
            PM, S, NR = r.PM, r.M, r.NR
        return PM, S, NR

    def run_neutral(self, P, month_start, GID, n_groups, signal="mom", adjust=None, J=12, skip=1,
                    n_bins=10, min_group=1, window=12, min_obs=None, V=None,
                    HLC=None) -> PipelineOut:
        """One full pass ranked inside groups (Moskowitz-Grinblatt 1999).  The signal is built as
        run (signal "mom") or run_signal (its names) build it.  adjust None: labels by
        deciles_within, the decile means pooled over the groups.  adjust "demean" / "zscore": the
        signal minus its group's mean (over its deviation), rule N5, then a plain deciles on it.
        M is the signal ranked and NR the signal's next return (rule N6).  V: the daily volume
        panel, for run_signal's liquidity names; HLC: the daily high, low and close panels, for its
        range names."""
        if adjust not in (None, "demean", "zscore"):
            raise ValueError(f"adjust must be None, 'demean' or 'zscore', got {adjust!r}")
        PM, S, NR = self._signal_panels(P, month_start, signal, J, skip, n_bins, window, min_obs,
                                        V, HLC)
        if adjust is None:
            L, EW, CNT, NV = self.deciles_within(S, NR, GID, n_groups, n_bins, min_group,
                                                 with_nv=True)
        else:
            field = "SA" if adjust == "demean" else "SZ"
            S = getattr(self.group_stats(S, GID, n_groups, outputs=(field,)), field)
            L, EW, CNT, NV = self.deciles(S, NR, n_bins, with_nv=True)
        LS = self.long_short(EW, CNT)
        return PipelineOut(PM=PM, M=S, NR=NR, L=L, EW=EW, CNT=CNT, LS=LS, NV=NV)

    # ------------------------------------------- reference-universe breakpoints and screens
    def _bp_mask(self, BP, T_m, N):
        """BP as csm_deciles_bp takes it: uint8 (or bool, reinterpreted) [T_m][N] (one row per
        month) or [N] (static); returns (BP, bp_ld)."""
        BP, ld = self._side_panel(BP, "BP", (torch.uint8, torch.bool), T_m, N,
                                  "a uint8 or bool torch tensor")
        return (BP.view(torch.uint8) if BP.dtype == torch.bool else BP), ld

    def deciles_bp(self, M, NR, BP, n_bins=10, with_nv=False, with_edges=False):
        """csm_deciles_bp (rules U1..U4): the qcut edges of each date from the cells with a
        non-zero BP byte (NYSE breakpoints), every non-NaN cell of M labelled against them (below
        the first edge: bin 0, above the last: the top bin), and with NR the decile means.  BP:
        uint8 or bool [T_m][N] or a static [N].
        Returns (L, EW, CNT[, NV, NVB][, EDGES, NE]); EW / CNT are None without NR."""
        T_m, N = M.shape
        _need(M, "M", torch.float64, (T_m, N), self.device)
        if NR is not None:
            _need(NR, "NR", torch.float64, (T_m, N), self.device)
        BP, ld = self._bp_mask(BP, T_m, N)
        nb = int(n_bins)
        L = self.empty((T_m, N), torch.int8)
        EW = self.empty((T_m, nb)) if NR is not None else None
        CNT = self.empty((T_m, nb), torch.int32) if NR is not None else None
        NV = self.empty((T_m,), torch.int32) if with_nv else None
        NVB = self.empty((T_m,), torch.int32) if with_nv else None
        EDGES = self.empty((T_m, max(nb, 0) + 1)) if with_edges else None
        NE = self.empty((T_m,), torch.int32) if with_edges else None
        self._call("csm_deciles_bp", _ptr(M), _ptr(NR), _ptr(BP), ld, T_m, N, nb, _qptr(nb),
                   _ptr(L), _ptr(EW), _ptr(CNT), _ptr(NV), _ptr(NVB), _ptr(EDGES), _ptr(NE))
        out = (L, EW, CNT)
        if with_nv:
            out += (NV, NVB)
        if with_edges:
            out += (EDGES, NE)
        return out

    def breakpoints(self, S, BP, n_bins=10):
        """The edges of csm_deciles_bp alone (rule U2, L = NULL): (EDGES [T_m][n_bins + 1], the
        NE[t] distinct edges first and NaN after them, NE, NVB).  breakpoints(CAP, nyse, 10)[0][:, 1]
        is the NYSE 10th-percentile size per month, the CAPMIN screen takes."""
        T_m, N = S.shape
        _need(S, "S", torch.float64, (T_m, N), self.device)
        BP, ld = self._bp_mask(BP, T_m, N)
        nb = int(n_bins)
        EDGES = self.empty((T_m, max(nb, 0) + 1))
        NE = self.empty((T_m,), torch.int32)
        NVB = self.empty((T_m,), torch.int32)
        self._call("csm_deciles_bp", _ptr(S), None, _ptr(BP), ld, T_m, N, nb, _qptr(nb), None,
                   None, None, None, _ptr(NVB), _ptr(EDGES), _ptr(NE))
        return EDGES, NE, NVB

    def screen(self, M, PM=None, min_price=None, CAP=None, CAPMIN=None, with_kept=False):
        """csm_screen (rule U5): M where the cell passes the price screen (PM >= min_price) and
        the size screen (CAP >= CAPMIN[t]), NaN elsewhere; a NaN PM, CAP or CAPMIN fails the cell.
        A screen whose panel is None is not applied.  Returns MS, or (MS, KEPT) with with_kept."""
        T_m, N = M.shape
        _need(M, "M", torch.float64, (T_m, N), self.device)
        if (PM is None) != (min_price is None):
            raise ValueError("PM and min_price go together")
        if (CAP is None) != (CAPMIN is None):
            raise ValueError("CAP and CAPMIN go together")
        if PM is not None:
            _need(PM, "PM", torch.float64, (T_m, N), self.device)
        if CAP is not None:
            _need(CAP, "CAP", torch.float64, (T_m, N), self.device)
            _need(CAPMIN, "CAPMIN", torch.float64, (T_m,), self.device)
        MS = self.empty((T_m, N))
        KEPT = self.empty((T_m,), torch.int32) if with_kept else None
        self._call("csm_screen", _ptr(M), _ptr(PM), 0.0 if min_price is None else float(min_price),
                   _ptr(CAP), _ptr(CAPMIN), T_m, N, _ptr(MS), _ptr(KEPT))
        return (MS, KEPT) if with_kept else MS

    def run_universe(self, P, month_start, BP=None, min_price=None, CAP=None, min_size_pct=None,
                     signal="mom", J=12, skip=1, n_bins=10, window=12, min_obs=None) -> PipelineOut:
        """One full pass on a screened universe with reference breakpoints (Jegadeesh-Titman
        2001).  The signal is built as run_neutral builds it; cells whose formation-month price is
        under min_price, or whose CAP [T_m][N] is under the min_size_pct percentile of the BP
        subset's CAP that month, are screened out (rule U5); the rest are ranked by deciles_bp on
        the BP subset's edges.  BP None: every cell is a breakpoint cell.  min_size_pct: a
        percentage p with 100 / p one of 2, 3, 4, 5, 10, 20 (10: the smallest decile, 20: the
        smallest quintile).  M is the screened signal and NR the signal's next return (rule U6)."""
        if (CAP is None) != (min_size_pct is None):
            raise ValueError("CAP and min_size_pct go together")
        PM, S, NR = self._signal_panels(P, month_start, signal, J, skip, n_bins, window, min_obs)
        T_m, N = S.shape
        if BP is None:
            BP = torch.ones((N,), dtype=torch.uint8, device=self.device)
        CAPMIN = None
        if CAP is not None:
            nq = self.size_bins(min_size_pct)
            CAPMIN = self.breakpoints(CAP, BP, nq)[0][:, 1].contiguous()
        KEPT = None
        if min_price is not None or CAP is not None:
            S, KEPT = self.screen(S, PM if min_price is not None else None, min_price, CAP,
                                  CAPMIN, with_kept=True)
        L, EW, CNT, NV, NVB, EDGES, NE = self.deciles_bp(S, NR, BP, n_bins, with_nv=True,
                                                         with_edges=True)
        LS = self.long_short(EW, CNT)
        return PipelineOut(PM=PM, M=S, NR=NR, L=L, EW=EW, CNT=CNT, LS=LS, NV=NV, NVB=NVB,
                           KEPT=KEPT, EDGES=EDGES, NE=NE)

    @staticmethod
    def size_bins(min_size_pct):
        """The n_bins whose edge 1 is the min_size_pct percentile: 100 / p, one of 2/3/4/5/10/20."""
        for nq in (2, 3, 4, 5, 10, 20):
            if abs(100.0 / nq - float(min_size_pct)) < 1e-9:
                return nq
        raise ValueError(f"min_size_pct={min_size_pct!r}: 100 / p must be one of 2, 3, 4, 5, 10, 20")

    def turnover_features(self, PM, VOL, so, mcap, lookback=3):
        """csm_turnover_features (src/features.py:60-107, rule T1): (ADV, SH, TURN, TAVG)."""
        T_m, N = PM.shape
        _need(PM, "PM", torch.float64, (T_m, N), self.device)
        _need(VOL, "VOL", torch.float64, (T_m, N), self.device)
        _need(so, "so", torch.float64, (N,), self.device)
        _need(mcap, "mcap", torch.float64, (N,), self.device)
        outs = [self.empty((T_m, N)) for _ in range(4)]
        self._call("csm_turnover_features", _ptr(PM), _ptr(VOL), _ptr(so), _ptr(mcap), T_m, N,
                   int(lookback), *[_ptr(o) for o in outs])
        return tuple(outs)

    def mask_by(self, M, X):
        """X where M is valid, NaN elsewhere (csm_double_sort_labels)."""
        T_m, N = M.shape
        _need(X, "X", torch.float64, (T_m, N), self.device)
        Xm = self.empty((T_m, N))
        self._call("csm_double_sort_labels", _ptr(M), _ptr(X), None, None, T_m, N, 1, _ptr(Xm),
                   None)
        return Xm

    def combine_labels(self, Lm, Lv, n_vol):
        """n_vol * Lm + Lv where both are valid, else -1 (csm_double_sort_labels)."""
        T_m, N = Lm.shape
        _need(Lv, "Lv", torch.int8, (T_m, N), self.device)
        Lc = self.empty((T_m, N), torch.int8)
        dummy = self.empty((1,))
        self._call("csm_double_sort_labels", _ptr(dummy), None, _ptr(Lm), _ptr(Lv), T_m, N,
                   int(n_vol), None, _ptr(Lc))
        return Lc

    def bootstrap(self, R, B, b0=0, seed=5000, mean_block=6.0, p0=100.0, out=None):
        """csm_bootstrap: B stationary-bootstrap month panels of the base month-return panel
        R[T_m][N] (rule E6) -> (src [B][T_m] int32, PMb [T_m][B*N] month prices)."""
        T_m, N = R.shape
        _need(R, "R", torch.float64, (T_m, N), self.device)
        if out is None:
            src = self.empty((B, T_m), torch.int32)
            PMb = self.empty((T_m, B * N))
        else:
            src, PMb = out
        self._call("csm_bootstrap", _ptr(R), T_m, N, int(B), int(b0), ctypes.c_uint64(int(seed)),
                   float(mean_block), float(p0), _ptr(src), _ptr(PMb))
        return src, PMb

    def boot_scan(self, R, B, Js, skip=1, b0=0, seed=5000, mean_block=6.0, p0=100.0,
                  with_ids=True):
        """csm_boot_scan: bootstrap(R, B, ...) and momentum_multi(with_ids) in one pass, the panel
        never written -> (src [B][T_m], [(M, IDS)] per J (IDS None without ids), NR [T_m][B*N]
        next_ret shared by every J, bad [1] int32).  M / IDS equal momentum_multi's on
        bootstrap's panel bit for bit; NR equals each J's next_ret on every row J ranks unless
        bad is set (include/csmom.h)."""
        T_m, N = R.shape
        _need(R, "R", torch.float64, (T_m, N), self.device)
        Js = [int(J) for J in Js]
        nJ = len(Js)
        BN = B * N
        src = self.empty((B, T_m), torch.int32)
        # (the Js' panels back to back: a caller may rank them as one stacked decile pass)
        Ms = list(self.empty((len(Js), T_m, BN)))
        IDS = list(self.empty((len(Js), T_m, BN), torch.int16)) if with_ids else None
        NR = self.empty((T_m, BN))
        bad = torch.empty(1, dtype=torch.int32, device=self.device)
        arr = lambda ts: (ctypes.c_void_p * nJ)(*[t.data_ptr() for t in ts])
        self._call("csm_boot_scan", _ptr(R), T_m, N, int(B), int(b0), ctypes.c_uint64(int(seed)),
                   float(mean_block), float(p0), (ctypes.c_int32 * nJ)(*Js), nJ, int(skip),
                   _ptr(src), arr(Ms), arr(IDS) if with_ids else None, _ptr(NR), _ptr(bad))
        return src, list(zip(Ms, IDS if with_ids else [None] * nJ)), NR, bad

    def shard_summary(self, PM, J, skip, out=None, state=None):
        """csm_shard_summary (one pass over PM), or csm_shard_summary_state (short walks,
        the same record) when `state` from signal_shard is given."""
        T_m, N = PM.shape
        _need(PM, "PM", torch.float64, (T_m, N), self.device)
        S = 6 + J + skip + 1
        out = self.empty((S, N)) if out is None else out
        _need(out, "summary", torch.float64, (S, N), self.device)
        if state is not None:
            _need(state.t, "state", torch.float64, (5, N), self.device)
            self._call("csm_shard_summary_state", _ptr(state.P), _ptr(state.month_start),
                       _ptr(PM), T_m, N, int(J), int(skip), _ptr(state.t), _ptr(out))
        else:
            self._call("csm_shard_summary", _ptr(PM), T_m, N, int(J), int(skip), _ptr(out))
        return out

    def fold_carry(self, summaries, g, J, skip, carry=None, next_pm=None):
        G, S, N = summaries.shape
        if S != 6 + J + skip + 1:
            raise ValueError(f"summaries have {S} rows, expected {6 + J + skip + 1}")
        _need(summaries, "summaries", torch.float64, (G, S, N), self.device)
        carry = self.empty((J + skip + 2, N)) if carry is None else carry
        next_pm = self.empty((N,)) if next_pm is None else next_pm
        self._call("csm_fold_carry", _ptr(summaries), G, int(g), N, int(J), int(skip),
                   _ptr(carry), _ptr(next_pm))
        return carry, next_pm

    def signal_shard(self, P, month_start, max_month_days, J=12, skip=1, with_ret=False,
                     out=None, ids=None):
        """csm_signal_shard: the fused pass over this date shard from an empty scan state
        (speculative; shard_repair fixes it once the carry is known).  Returns
        (PM, R, M, NR, ShardState); PM holds only the shard's first / last J + skip + 8
        months (the rest are re-derived from P where needed).  ids (int16 [T_m][N], N % 4 ==
        0): also the fixed-map bucket id of every mom_J (csm_signal_shard_ids)."""
        T_d, N = P.shape
        T_m = month_start.numel() - 1
        _need(P, "P", torch.float64, (T_d, N), self.device)
        _need(month_start, "month_start", torch.int64, (T_m + 1,), self.device)
        if out is None:
            PM, M, NR = self.empty((T_m, N)), self.empty((T_m, N)), self.empty((T_m, N))
            R = self.empty((T_m, N)) if with_ret else None
            state = self.empty((5, N))
        else:
            PM, R, M, NR, state = out
        if ids is not None:
            _need(ids, "ids", torch.int16, (T_m, N), self.device)
            self._call("csm_signal_shard_ids", _ptr(P), T_d, N, _ptr(month_start), T_m,
                       int(max_month_days), int(J), int(skip), _ptr(PM), _ptr(R), _ptr(M),
                       _ptr(NR), _ptr(state), _ptr(ids))
        else:
            self._call("csm_signal_shard", _ptr(P), T_d, N, _ptr(month_start), T_m,
                       int(max_month_days), int(J), int(skip), _ptr(PM), _ptr(R), _ptr(M),
                       _ptr(NR), _ptr(state))
        return PM, R, M, NR, ShardState(state, P, month_start)

    def shard_repair(self, PM, carry, next_pm, state, M, NR, J, skip, R=None, ids=None):
        """csm_shard_repair: turn the outputs of signal_shard (M, NR, R rewritten in place)
        into those of the scan from `carry`, and finish the pending rows with `next_pm` (both
        from fold_carry)."""
        T_m, N = PM.shape
        W = J + skip
        _need(PM, "PM", torch.float64, (T_m, N), self.device)
        _need(carry, "carry", torch.float64, (W + 2, N), self.device)
        _need(next_pm, "next_pm", torch.float64, (N,), self.device)
        _need(state.t, "state", torch.float64, (5, N), self.device)
        for t, nm in ((M, "M"), (NR, "NR"), (R, "R")):
            if t is not None:
                _need(t, nm, torch.float64, (T_m, N), self.device)
        if ids is not None:   # rewrite the ids of the rewritten cells too
            _need(ids, "ids", torch.int16, (T_m, N), self.device)
            self._call("csm_shard_repair_ids", _ptr(state.P), _ptr(state.month_start), _ptr(PM),
                       T_m, N, int(J), int(skip), _ptr(carry), _ptr(next_pm), _ptr(state.t),
                       _ptr(R), _ptr(M), _ptr(NR), _ptr(ids))
        else:
            self._call("csm_shard_repair", _ptr(state.P), _ptr(state.month_start), _ptr(PM),
                       T_m, N, int(J), int(skip), _ptr(carry), _ptr(next_pm), _ptr(state.t),
                       _ptr(R), _ptr(M), _ptr(NR))
        return M, NR

    # ------------------------------------------------------------ halo date shards
    def shard_halo(self, P, month_start, H, F, J=12, skip=1, before=True, after=True, out=None):
        """csm_shard_halo: P holds H halo months, the shard and F (0..8) forward months
        (month_start [H + T_m + F + 1], day offsets into P); before / after: the panel has
        months before the halo / after the forward months.  Returns (carry [J+skip+2][N],
        next_pm [N], flags uint8 [N]; bit 0 carry uncertain, bit 1 next_pm uncertain)."""
        T_d, N = P.shape
        T_m = month_start.numel() - 1 - H - F
        _need(P, "P", torch.float64, (T_d, N), self.device)
        _need(month_start, "month_start", torch.int64, (H + T_m + F + 1,), self.device)
        if out is None:
            carry, npm = self.empty((J + skip + 2, N)), self.empty((N,))
            flags = self.empty((N,), torch.uint8)
        else:
            carry, npm, flags = out
        hpm = self.empty((max(H + F, 1), N))
        self._call("csm_shard_halo", _ptr(P), T_d, N, _ptr(month_start), int(H), int(T_m),
                   int(F), int(bool(before)), int(bool(after)), int(J), int(skip), _ptr(hpm),
                   _ptr(carry), _ptr(npm), _ptr(flags))
        return carry, npm, flags

    def signal_shard_halo(self, P, month_start, max_month_days, J, skip, carry, next_pm,
                          with_ret=False, out=None, ids=None):
        """csm_signal_shard_halo: signal_shard from the halo's carry / next_pm (month_start =
        the shard's T_m + 1 offsets into P).  Returns (PM, R, M, NR, ShardState)."""
        T_d, N = P.shape
        T_m = month_start.numel() - 1
        W = J + skip
        _need(P, "P", torch.float64, (T_d, N), self.device)
        _need(month_start, "month_start", torch.int64, (T_m + 1,), self.device)
        _need(carry, "carry", torch.float64, (W + 2, N), self.device)
        _need(next_pm, "next_pm", torch.float64, (N,), self.device)
        if out is None:
            PM, M, NR = self.empty((T_m, N)), self.empty((T_m, N)), self.empty((T_m, N))
            R = self.empty((T_m, N)) if with_ret else None
            state = self.empty((5, N))
        else:
            PM, R, M, NR, state = out
        if ids is not None:
            _need(ids, "ids", torch.int16, (T_m, N), self.device)
        self._call("csm_signal_shard_halo", _ptr(P), T_d, N, _ptr(month_start), T_m,
                   int(max_month_days), int(J), int(skip), _ptr(carry), _ptr(next_pm), _ptr(PM),
                   _ptr(R), _ptr(M), _ptr(NR), _ptr(state), _ptr(ids))
        return PM, R, M, NR, ShardState(state, P, month_start)

    @staticmethod
    def halo_fused_ok(N, max_month_days):
        """Whether csm_signal_halo (the halo prologue inside the wide shard kernel) takes this
        panel: even N >= 92160 (the four-wave blocks), months of <= 23 day rows."""
        return N % 2 == 0 and 92160 <= N < (1 << 31) // 256 and max_month_days <= 23

    def signal_halo(self, P, month_start, H, F, max_month_days, J, skip, before=True, after=True,
                    with_ret=False, ids=None):
        """csm_signal_halo: shard_halo + signal_shard_halo in one launch (halo_fused_ok
        panels).  month_start [H + T_m + F + 1] as shard_halo's.  Returns (PM, R, M, NR,
        ShardState, flags) -- ShardState on the shard's month offsets, flags shard_halo's."""
        T_d, N = P.shape
        T_m = month_start.numel() - 1 - H - F
        _need(P, "P", torch.float64, (T_d, N), self.device)
        _need(month_start, "month_start", torch.int64, (H + T_m + F + 1,), self.device)
        PM, M, NR = self.empty((T_m, N)), self.empty((T_m, N)), self.empty((T_m, N))
        R = self.empty((T_m, N)) if with_ret else None
        state = self.empty((5, N))
        flags = self.empty((N,), torch.uint8)
        if ids is not None:
            _need(ids, "ids", torch.int16, (T_m, N), self.device)
        self._call("csm_signal_halo", _ptr(P), T_d, N, _ptr(month_start), int(H), int(T_m), int(F),
                   int(bool(before)), int(bool(after)), int(max_month_days), int(J), int(skip),
                   _ptr(PM), _ptr(R), _ptr(M), _ptr(NR), _ptr(state), _ptr(ids), _ptr(flags))
        return PM, R, M, NR, ShardState(state, P, month_start[H:H + T_m + 1]), flags

    def shard_need(self, flags, state, H, out=None):
        """csm_shard_need -> int64 [4][ceil(N / 64)]: this rank's exchange bits (H = the halo
        length the next rank holds)."""
        N = flags.numel()
        T_m = state.month_start.numel() - 1
        mask = self.empty((4, (N + 63) // 64), torch.int64) if out is None else out
        self._call("csm_shard_need", _ptr(flags), _ptr(state.t), N, T_m, int(H), _ptr(mask))
        return mask

    def shard_union(self, masks, N, cap, out=None):
        """csm_shard_union over the gathered bits [G][4][ceil(N / 64)] -> (idx int32 [cap],
        count int32 [1]) on the device (no sync)."""
        G = masks.shape[0]
        _need(masks, "masks", torch.int64, (G, 4, (N + 63) // 64), self.device)
        idx, cnt = ((self.empty((cap,), torch.int32), self.empty((1,), torch.int32))
                    if out is None else out)
        self._call("csm_shard_union", _ptr(masks), G, N, int(cap), _ptr(idx), _ptr(cnt))
        return idx, cnt

    def shard_summary_cols(self, PM, state, idx, cnt, J, skip, out=None):
        """csm_shard_summary_cols: the exchange record [S][cap] of the listed assets."""
        T_m, N = PM.shape
        cap = idx.numel()
        S = 6 + J + skip + 1
        out = self.empty((S, cap)) if out is None else out
        _need(out, "summary", torch.float64, (S, cap), self.device)
        self._call("csm_shard_summary_cols", _ptr(state.P), _ptr(state.month_start), _ptr(PM),
                   T_m, N, int(J), int(skip), _ptr(state.t), _ptr(idx), _ptr(cnt), cap,
                   _ptr(out))
        return out

    def shard_repair_cols(self, PM, carry, next_pm, fcarry, state, idx, cnt, M, NR, J, skip,
                          R=None, ids=None):
        """csm_shard_repair_cols: repair the listed assets from their folded carry / next_pm
        columns ([.][cap]); fcarry = the halo carry the pass started from."""
        T_m, N = PM.shape
        cap = idx.numel()
        W = J + skip
        _need(carry, "carry", torch.float64, (W + 2, cap), self.device)
        _need(next_pm, "next_pm", torch.float64, (cap,), self.device)
        _need(fcarry, "fcarry", torch.float64, (W + 2, N), self.device)
        self._call("csm_shard_repair_cols", _ptr(state.P), _ptr(state.month_start), _ptr(PM),
                   T_m, N, int(J), int(skip), _ptr(carry), _ptr(next_pm), _ptr(fcarry),
                   _ptr(state.t), _ptr(idx), _ptr(cnt), cap, _ptr(R), _ptr(M), _ptr(NR),
                   _ptr(ids))
        return M, NR

    def shard_fix_cols(self, PM, records, g, state, idx, cnt, M, NR, J, skip, R=None, ids=None):
        """csm_shard_fix_cols: fold the listed columns' all-gathered records [G][S][cap] (this
        rank g) and replay every month of each listed column from its true carry, in one launch
        (the halo pass's fold_carry + shard_repair_cols)."""
        T_m, N = PM.shape
        G, S, cap = records.shape
        if S != 6 + J + skip + 1:
            raise ValueError(f"records have {S} rows, expected {6 + J + skip + 1}")
        _need(records, "records", torch.float64, (G, S, cap), self.device)
        _need(idx, "idx", torch.int32, (cap,), self.device)
        _need(M, "M", torch.float64, (T_m, N), self.device)
        _need(NR, "NR", torch.float64, (T_m, N), self.device)
        if ids is not None:
            _need(ids, "ids", torch.int16, (T_m, N), self.device)
        self._call("csm_shard_fix_cols", _ptr(state.P), _ptr(state.month_start), _ptr(PM),
                   T_m, N, int(J), int(skip), _ptr(records), G, int(g), _ptr(idx), _ptr(cnt), cap,
                   _ptr(R), _ptr(M), _ptr(NR), _ptr(ids))
        return M, NR

    def sync(self):
        self._call("csm_sync")

    # ------------------------------------------------------------------ pipeline
    def use_fused(self, P, V=None, max_month_days=None) -> bool:
        T_d, N = P.shape
        return (V is None and N >= FUSED_MIN_N and max_month_days is not None
                and max_month_days <= 32)

    def run(self, P, month_start, J=12, skip=1, n_bins=10, V=None, with_ret=False,
            max_month_days=None, fused=None):
        """One full pass: month-end -> signal -> labels + EW decile means -> long-short.
        Large panels take the fused month-end + scan kernel (no PM round trip)."""
        T_m, N = month_start.numel() - 1, P.shape[1]
        min_month_days = None
        if max_month_days is None and T_m > 0:
            max_month_days, min_month_days = self.month_days(month_start)
        if fused is None:
            fused = self.use_fused(P, V, max_month_days)
        if fused:   # one C call: signal (+ bucket ids for wide rows) -> deciles -> long-short
            return self.pipeline(P, month_start, J, skip, n_bins, max_month_days, with_pm=True,
                                 with_ret=with_ret, min_month_days=min_month_days)
        else:
            PM, VOL = self.month_end(P, month_start, V)
            if self.default_chunks(T_m, N, J, skip) > 1:
                R, M, NR = self.momentum_chunked(PM, J, skip, with_ret=with_ret)
            else:
                R, M, NR = self.momentum(PM, J, skip, with_ret=with_ret)
        L, EW, CNT, NV = self.deciles(M, NR, n_bins, with_nv=True)
        LS = self.long_short(EW, CNT)
        return PipelineOut(PM=PM, M=M, NR=NR, L=L, EW=EW, CNT=CNT, LS=LS, R=R, VOL=VOL, NV=NV)

    MARKET_SIGNALS = {"resid_mom": "RESMOM", "beta": "BETA", "ivol": "IVOL"}
    DAILY_SIGNALS = {"dbeta": "DBETA", "divol": "DIVOL", "dskew": "DSKEW", "max": "DMAX"}
    LIQ_SIGNALS = {"illiq": "ILLIQ", "dvol": "DVOL", "zret": "ZRET"}
    RANGE_SIGNALS = {"pkvol": "PKVOL", "cs_spread": "CSSPR", "ar_spread": "ARSPR"}
    ASYM_SIGNALS = {"info_disc": "ID", "rsj": "RSJ", "dsvol": "DSVOL", "dnbeta": "DNBETA"}
    RUN_SIGNALS = ("high52", "mom_vol", *MARKET_SIGNALS, *DAILY_SIGNALS, *ASYM_SIGNALS,
                   *RANGE_SIGNALS, *LIQ_SIGNALS)

    def daily_signals(self, P, month_start, names, window=None, min_obs=None, max_gap=10):
        """{name: [T_m][N]} for names of DAILY_SIGNALS (rules V1..V4): the daily market, one pass
        for the month sums on it, and one model call per window.  window None: 12 months for
        "dbeta", 1 for the others; min_obs counts days (default 15 * window)."""
        MKTD, _ = self.daily_market(P, max_gap)
        sums = self.daily_sums(P, month_start, MKTD, max_gap, with_sr3="dskew" in names,
                               with_rmax="max" in names)
        by_window = {}
        for n in names:
            w = (12 if n == "dbeta" else 1) if window is None else int(window)
            by_window.setdefault(w, []).append(n)
        out = {}
        for w, group in by_window.items():
            dm = self.daily_model(sums, w, min_obs,
                                  outputs=tuple(self.DAILY_SIGNALS[n] for n in group))
            for n in group:
                out[n] = getattr(dm, self.DAILY_SIGNALS[n])
        return out

    def liq_signals(self, P, V, month_start, names, window=None, min_obs=None, max_gap=10,
                    scale=1e6):
        """{name: [T_m][N]} for names of LIQ_SIGNALS (rules Q1..Q3): one pass over both panels
        for the month sums and one model call.  window None: 12 months; min_obs counts days
        (default 15 * window)."""
        sums = self.liq_sums(P, V, month_start, max_gap, with_sv=False,
                             with_nzr="zret" in names, with_nzv=False)
        lm = self.liq_model(sums, 12 if window is None else int(window), min_obs, scale,
                            outputs=tuple(self.LIQ_SIGNALS[n] for n in names))
        return {n: getattr(lm, self.LIQ_SIGNALS[n]) for n in names}

    def range_signals(self, H, L, C, month_start, names, window=None, min_obs=None, max_gap=1):
        """{name: [T_m][N]} for names of RANGE_SIGNALS (rules HL1..HL6): one pass over the three
        panels for the month sums and one model call.  window None: 1 month; min_obs counts days
        (default 15 * window)."""
        sums = self.range_sums(H, L, C, month_start, max_gap, with_cs="cs_spread" in names,
                               with_ar="ar_spread" in names)
        rm = self.range_model(sums, 1 if window is None else int(window), min_obs,
                              outputs=tuple(self.RANGE_SIGNALS[n] for n in names))
        return {n: getattr(rm, self.RANGE_SIGNALS[n]) for n in names}

    def asym_signals(self, P, month_start, names, J=12, skip=1, window=None, min_obs=None,
                     max_gap=10, PM=None):
        """{name: [T_m][N]} for names of ASYM_SIGNALS (rules AS1..AS3): one pass over P for the
        month sums and one model call per window.  "info_disc" always covers the J months that
        end `skip` months back, signed by momentum(PM, J, skip)'s mom_J (PM None: month_end's);
        `window` does not apply to it.  window None: 1 month for "rsj" and "dsvol", 12 for
        "dnbeta", whose factor is daily_market(P, max_gap)'s series and whose side is -1; these
        three end at the month itself.  min_obs counts return days (default 15 * window); for
        "dnbeta" it counts the down-market return days (default max(2, 5 * window), and at least
        2 when given)."""
        FD = self.daily_market(P, max_gap)[0] if "dnbeta" in names else None
        sums = self.asym_sums(P, month_start, FD, -1, max_gap)
        calls = {}
        for n in names:
            if n == "info_disc":
                key = (int(J), int(skip))
            else:
                key = ((12 if n == "dnbeta" else 1) if window is None else int(window), 0)
            calls.setdefault(key, []).append(n)
        out = {}
        for (w, s), group in calls.items():
            M = None
            if "info_disc" in group:
                if PM is None:
                    PM, _ = self.month_end(P, month_start)
                _, M, _ = self.momentum(PM, J, skip)
            am = self.asym_model(sums, w, s, M, min_obs,
                                 None if min_obs is None else max(2, int(min_obs)),
                                 outputs=tuple(self.ASYM_SIGNALS[n] for n in group))
            for n in group:
                out[n] = getattr(am, self.ASYM_SIGNALS[n])
        return out

    DAILY_FACTOR_SIGNALS = {"dbeta": "DBETA", "divol": "DIVOL"}   # the daily signals factors= serves

    def run_signal(self, P, month_start, signal, J=12, skip=1, n_bins=10, window=12,
                   min_obs=None, factors=None, V=None, HLC=None) -> PipelineOut:
        """One full pass ranked on a signal of the daily panel: "high52", the month-end price
        over the highest daily price of the last `window` months (no momentum scan), or
        "mom_vol", mom_J over the realised daily volatility of the last `window` months.
        M is the signal and NR its next return (rules D1..D6).
        Or on a signal of the monthly cross-section (rules B1..B6), from the market model of each
        asset's month returns on the equal-weight market over `window` months: "resid_mom", the
        residual momentum of the J months that end `skip` months back, "beta" or "ivol".  For
        these three a `window` left at its default of 12 means 36, and min_obs counts months
        (default max(2, ceil(2 * window / 3))).
        Or on a signal of the daily returns against the equal-weight daily market (rules
        V1..V6): "dbeta", "divol", "dskew" or "max".  For these a `window` left at its default
        means 12 months for "dbeta" and 1 month for the other three, and min_obs counts days
        (default 15 * window).
        factors (rules MF1..MF8): a [T_m][KF] tensor with "resid_mom" / "beta" / "ivol", or a
        [T_d][KF] tensor with "dbeta" / "divol", replaces the equal-weight market by the caller's
        KF factors (1 <= KF <= 4); "beta" and "dbeta" rank on column 0's slope, and min_obs
        defaults to factor_model's / daily_fmodel's.  Any other signal with factors raises.
        Or on a liquidity signal of the daily prices and the daily volume panel V [T_d][N] (rules
        Q1..Q6): "illiq", "dvol" or "zret" over `window` months, min_obs counting days (default
        15 * window).  These three need V; V with factors raises.
        Or on a range signal of the daily high, low and close panels HLC = (H, L, C), each
        [T_d][N] (rules HL1..HL6): "pkvol", "cs_spread" or "ar_spread".  For these a `window`
        left at its default means 1 month, min_obs counts days (default 15 * window), and NR is
        the next return of P's month-end prices.  These three need HLC; HLC with V or factors
        raises.
        Or on an asymmetry signal of the daily returns (rules AS1..AS7): "info_disc", the
        information discreteness of the J months that end `skip` months back, signed by mom_J
        (`window` does not apply), "rsj" or "dsvol" (a `window` left at its default means 1
        month), or "dnbeta", the beta on the down days of the equal-weight daily market (12
        months).  min_obs counts days as in asym_signals.  factors, V or HLC with one of these
        raises."""
        if signal not in self.RUN_SIGNALS:
            raise ValueError(f"signal must be one of {self.RUN_SIGNALS}, got {signal!r}")
        if signal in self.ASYM_SIGNALS and not (factors is None and V is None and HLC is None):
            raise ValueError(f"signal {signal!r} takes no factors, V or HLC")
        if signal in self.LIQ_SIGNALS and V is None:
            raise ValueError(f"signal {signal!r} needs the daily volume panel V")
        if V is not None and factors is not None:
            raise ValueError("V and factors do not go together")
        if signal in self.RANGE_SIGNALS and HLC is None:
            raise ValueError(f"signal {signal!r} needs the daily panels HLC = (H, L, C)")
        if HLC is not None and (V is not None or factors is not None):
            raise ValueError("HLC does not go with V or factors")
        if factors is not None and signal not in (*self.MARKET_SIGNALS,
                                                  *self.DAILY_FACTOR_SIGNALS):
            raise ValueError(f"factors go with {(*self.MARKET_SIGNALS, *self.DAILY_FACTOR_SIGNALS)}"
                             f", got {signal!r}")
        st = self.month_stats(P, month_start)
        if factors is not None and signal in self.MARKET_SIGNALS:
            field = self.MARKET_SIGNALS[signal]
            fm = self.factor_model(st.PM, factors, window=36 if window == 12 else window, J=J,
                                   skip=skip, min_obs=min_obs, outputs=(field,))
            S = getattr(fm, field)
            S = S[0] if S.dim() == 3 else S          # "beta": column 0's slope
            NR = self.next_ret(st.PM, S)
        elif factors is not None:
            field = self.DAILY_FACTOR_SIGNALS[signal]
            w = (12 if signal == "dbeta" else 1) if window == 12 else int(window)
            dm = self.daily_fmodel(self.daily_fsums(P, month_start, factors), w, min_obs,
                                   outputs=(field,))
            S = getattr(dm, field)
            S = S[0] if S.dim() == 3 else S          # "dbeta": column 0's slope
            NR = self.next_ret(st.PM, S)
        elif signal in self.DAILY_SIGNALS:
            S = self.daily_signals(P, month_start, (signal,), None if window == 12 else window,
                                   min_obs)[signal]
            NR = self.next_ret(st.PM, S)
        elif signal in self.ASYM_SIGNALS:
            S = self.asym_signals(P, month_start, (signal,), J, skip,
                                  None if window == 12 else window, min_obs, PM=st.PM)[signal]
            NR = self.next_ret(st.PM, S)
        elif signal in self.LIQ_SIGNALS:
            S = self.liq_signals(P, V, month_start, (signal,), window, min_obs)[signal]
            NR = self.next_ret(st.PM, S)
        elif signal in self.RANGE_SIGNALS:
            S = self.range_signals(*HLC, month_start, (signal,), None if window == 12 else window,
                                   min_obs)[signal]
            NR = self.next_ret(st.PM, S)
        elif signal in self.MARKET_SIGNALS:
            field = self.MARKET_SIGNALS[signal]
            mm = self.market_model(st.PM, window=36 if window == 12 else window, J=J, skip=skip,
                                   min_obs=min_obs, outputs=(field,))
            S = getattr(mm, field)
            NR = self.next_ret(st.PM, S)
        elif signal == "high52":
            sig = self.window_signals(*st, Jh=window, Jv=window, min_obs=min_obs,
                                      outputs=("H52", "NR_H52"))
            S, NR = sig.H52, sig.NR_H52
        else:
            _, M, _ = self.momentum(st.PM, J, skip)
            sig = self.window_signals(*st, M=M, Jh=window, Jv=window, min_obs=min_obs,
                                      outputs=("MS", "NR_MS"))
            S, NR = sig.MS, sig.NR_MS
        L, EW, CNT, NV = self.deciles(S, NR, n_bins, with_nv=True)
        LS = self.long_short(EW, CNT)
        return PipelineOut(PM=st.PM, M=S, NR=NR, L=L, EW=EW, CNT=CNT, LS=LS, NV=NV)
