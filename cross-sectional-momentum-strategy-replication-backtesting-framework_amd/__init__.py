"""csmom -- MI355X-native engine for the cross-sectional momentum backtest hot path of
AkshayJha22/Cross-Sectional-Momentum-Strategy-Replication-Backtesting-Framework.

Import it as ``csmom`` (the repo-root ``csmom.py`` aliases this directory, whose name is not
a Python identifier).  Public API (reference file:line it replaces):

  compute_monthly_momentum_from_daily   src/features.py:5-57       (GPU)
  compute_monthly_turnover              src/features.py:60-107     (host; unused by the path)
  assign_deciles_per_date               run_demo.py:18-29          (GPU)
  monthly_replication                   run_demo.py:31-79          (GPU + host summary)
  sharpe / ensure_dir / save_plot       src/utils.py:5-21          (host)
  fetch_daily / normalize_daily_columns src/data_io.py:23-73,131-180 (host, cached CSVs only)
  Engine                                dense device pipeline (bench / multi-GPU)
  Engine.portfolio / Engine.bootstrap   K-overlap, value weights, turnover, costs, bootstrap
                                        (beyond run_demo.py:49-67)
  Engine.daily_returns / series_stats   daily return series of the portfolios + their statistics
  daily_portfolio_returns               the same from a daily frame (rule E7; beyond the reference)
  Engine.month_stats / window_signals   52-week high, realised volatility and volatility-scaled
  Engine.run_signal                     momentum from every day row (rules D1..D6; beyond the reference)
  Engine.market_factor / market_model   equal-weight market, beta, idiosyncratic volatility and
  Engine.next_ret                       residual momentum; the next return of any signal (B1..B6)
  Engine.daily_market / daily_sums      equal-weight daily market; daily beta, idiosyncratic and total
  Engine.daily_model / daily_signals    volatility, skewness and MAX from daily returns (rules V1..V6)
  Engine.xs_regress / newey_west        per-month cross-sectional regressions (OLS, WLS, ridge) and
  Engine.fama_macbeth / fama_macbeth    Newey-West t-statistics of any monthly series (R1..R6)
  Engine.deciles_within / group_stats   qcut inside groups (sector-neutral deciles, dependent sorts)
  Engine.run_neutral / neutral_momentum and industry-adjusted signals (rules N1..N6)
  dependent_double_sort                 n1 bins of one signal, n2 bins of another inside each
  Engine.xs_rank / rank_ic / ic_decay   cross-sectional ranks, per-month Spearman and Pearson ICs
  information_coefficient               and their decay over horizons (rules I1..I6)
  Engine.deciles_bp / breakpoints       qcut edges from a subset of each date (NYSE breakpoints) applied
  Engine.screen / run_universe          to every cell, the edges themselves, price and size screens
  universe_momentum                     (rules U1..U6)
  Engine.factor_model / daily_fsums     KF-factor rolling models, KF = 1..4: FF3-style betas, alphas,
  Engine.daily_fmodel / lagged          idiosyncratic volatility, residual momentum, Dimson betas
  residual_momentum / align_factors     (rules MF1..MF8)
  Engine.liq_sums / liq_model           Amihud illiquidity, dollar average daily volume, turnover,
  liquidity_signals                     zero-return and zero-volume days from the daily price and
                                        volume panels (rules Q1..Q6)
  Engine.range_sums / range_model       Parkinson volatility, Corwin-Schultz and Abdi-Ranaldo bid-ask
  range_signals                         spreads from the daily high, low and close (rules HL1..HL6)
  Engine.asym_sums / asym_model         information discreteness, signed jump variation, downside
  asymmetry_signals / frog_in_the_pan   semi-volatility and downside beta from the daily returns; momentum
                                        inside information-discreteness bins (rules AS1..AS7)
  SweepRunner                           (J, K) grids over panels / bootstrap panels (C3, C5)
  Engine.turnover_features              src/features.py:60-107 on the device (bit-exact)
  momentum_volume_double_sort           LeSw00 10 x 3 momentum x turnover sort
"""
from ._lib import ABSENT_BITS, CsmError, CsmUnavailable, lib_path, load_library
from .engine import (AsymModelOut, AsymSums, DailyFModelOut, DailyFSums, DailyModelOut, DailyOut, DailySums, Engine, FactorModelOut, FamaMacBethOut, GroupStatsOut, ICDecayOut, LiqModelOut, LiqSums,
                     MarketModelOut,
                     MonthStats, NeweyWestOut, PipelineOut, PortfolioOut, RangeModelOut, RangeSums,
                     RankICOut, SignalsOut,
                     XsRegressOut, absent_tensor, is_absent, quantile_table)
from .data import fetch_daily, load_daily_panel, normalize_daily_columns
from .features import compute_monthly_momentum_from_daily, compute_monthly_turnover, get_engine
from .lesw import (DependentSortResult, DoubleSortResult, dependent_double_sort,
                   momentum_volume_double_sort)
from .neutral import NeutralResult, group_ids, neutral_momentum
from .universe import UniverseResult, breakpoint_mask, shares_row, universe_momentum
from .factors import ResidualMomentumResult, align_factors, residual_momentum
from .regress import FamaMacBethResult, fama_macbeth
from .ic import ICResult, information_coefficient
from .liquidity import LIQUIDITY_COLUMNS, liquidity_signals
from .ranges import RANGE_COLUMNS, range_signals
from .asym import ASYMMETRY_COLUMNS, FipResult, asymmetry_signals, frog_in_the_pan
from .panel import DensePanel, from_long, month_offsets, monthly_frame, range_from_long
from .replication import (ReplicationResult, assign_deciles_per_date, daily_portfolio_returns,
                          monthly_replication)
from .sweep import SUMMARY_FIELDS, SweepConfig, SweepRunner, strategy_grid
from .utils import ensure_dir, save_plot, sharpe

__all__ = [
    "ABSENT_BITS", "CsmError", "CsmUnavailable", "lib_path", "load_library", "Engine",
    "PipelineOut", "PortfolioOut", "SweepConfig", "SweepRunner", "SUMMARY_FIELDS",
    "strategy_grid", "DoubleSortResult", "momentum_volume_double_sort", "fetch_daily", "load_daily_panel", "normalize_daily_columns",
    "absent_tensor", "is_absent", "quantile_table",
    "compute_monthly_momentum_from_daily", "compute_monthly_turnover", "get_engine",
    "DensePanel", "from_long", "month_offsets", "monthly_frame", "ReplicationResult",
    "assign_deciles_per_date", "monthly_replication", "ensure_dir", "save_plot", "sharpe",
    "DailyOut", "daily_portfolio_returns", "MonthStats", "SignalsOut", "DailySums", "DailyModelOut",
    "MarketModelOut", "XsRegressOut", "NeweyWestOut", "FamaMacBethOut", "FamaMacBethResult",
    "fama_macbeth", "GroupStatsOut", "DependentSortResult", "dependent_double_sort",
    "NeutralResult", "group_ids", "neutral_momentum",
    "RankICOut", "ICDecayOut", "ICResult", "information_coefficient",
    "UniverseResult", "breakpoint_mask", "shares_row", "universe_momentum",
    "FactorModelOut", "DailyFSums", "DailyFModelOut", "ResidualMomentumResult", "align_factors",
    "residual_momentum", "LiqSums", "LiqModelOut", "LIQUIDITY_COLUMNS", "liquidity_signals",
    "RangeSums", "RangeModelOut", "RANGE_COLUMNS", "range_signals", "range_from_long",
    "AsymSums", "AsymModelOut", "ASYMMETRY_COLUMNS", "FipResult", "asymmetry_signals",
    "frog_in_the_pan",
]
