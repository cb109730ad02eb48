"""Factor-adjusted signals from a daily frame and a frame of monthly factor returns (rules
MF1..MF8 in DESIGN.md section 7; Engine.factor_model): residual momentum on the three Fama-French
factors (Blitz, Huij and Martens 2011), or on any one to four factor series of the caller's.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import pandas as pd
import torch

from .features import get_engine, upload_panel
from .panel import from_long
from .utils import sharpe


@dataclass
class ResidualMomentumResult:
    long_short: pd.Series      # the long-short per month-end date (undefined months left out)
    deciles: pd.DataFrame      # the decile means, one column per bin
    factors: pd.DataFrame      # the factor rows the panel's months were matched to (NaN: none)
    mean: float                # of the long-short months
    sharpe: float              # annualised over 12 periods
    t_nw: float                # Newey-West t-statistic of the mean (Engine.newey_west)
    lags: int


def align_factors(factors_df, month_index):
    """The rows of factors_df (one row per month, a DatetimeIndex or a "date" column, one column
    per factor, in any order) matched to the calendar months of month_index by (year, month):
    a float64 frame indexed by month_index, a NaN row for a month factors_df lacks; months it has
    and the panel lacks are dropped.  Two rows of one month raise ValueError."""
    df = factors_df
    if "date" in getattr(df, "columns", ()):
        df = df.set_index("date")
    dates = pd.DatetimeIndex(pd.to_datetime(df.index))
    key = dates.year * 12 + dates.month
    if pd.Index(key).has_duplicates:
        dup = dates[pd.Index(key).duplicated()][0]
        raise ValueError(f"factors_df has more than one row for {dup.year}-{dup.month:02d}")
    month_index = pd.DatetimeIndex(month_index)
    want = month_index.year * 12 + month_index.month
    vals = df.to_numpy(dtype=np.float64)
    out = pd.DataFrame(vals, index=pd.Index(key), columns=list(df.columns)).reindex(want)
    out.index = month_index
    return out


def residual_momentum(daily_df, factors_df, window=36, J=12, skip=1, n_bins=10, min_obs=None,
                      device=None):
    """Long-short of residual momentum: each stock's month returns regressed on the factors of
    factors_df (align_factors; one to four columns) over `window` months, ranked on the sum of
    the J residuals that end `skip` months back over their deviation
    (Engine.run_signal("resid_mom", factors=...); as there, a window of 12 means 36).  Returns a
    ResidualMomentumResult, or None when the frame holds no month."""
    panel = from_long(daily_df)
    if panel.P.size == 0 or panel.T_m == 0:
        return None
    idx = pd.DatetimeIndex(panel.month_end, name="date")
    fac = align_factors(factors_df, idx)
    eng = get_engine(device)
    P, _, ms = upload_panel(panel, eng, with_volume=False)
    F = torch.from_numpy(np.ascontiguousarray(fac.to_numpy())).to(eng.device)
    out = eng.run_signal(P, ms, "resid_mom", J=J, skip=skip, n_bins=n_bins, window=window,
                         min_obs=min_obs, factors=F)
    nw = eng.newey_west(out.LS)
    ls = pd.Series(out.LS.cpu().numpy(), index=idx, name="long_short").dropna()
    return ResidualMomentumResult(
        long_short=ls,
        deciles=pd.DataFrame(out.EW.cpu().numpy(), index=idx, columns=list(range(n_bins))),
        factors=fac, mean=float(nw.MEAN), sharpe=float(sharpe(ls.values, 12)),
        t_nw=float(nw.T), lags=eng.default_lags(out.LS.shape[0]))


__all__ = ["ResidualMomentumResult", "align_factors", "residual_momentum"]
