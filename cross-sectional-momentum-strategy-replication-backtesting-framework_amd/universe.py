"""Momentum on a screened universe with reference breakpoints, from a daily frame (Jegadeesh-
Titman 2001): stocks under a minimum price or under a size percentile of the breakpoint tickers
are dropped, the decile edges come from the breakpoint tickers alone (NYSE breakpoints) and every
remaining stock is assigned to those bins (rules U1..U6 in DESIGN.md section 7;
Engine.run_universe).
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
class UniverseResult:
    long_short: pd.Series      # the long-short per month-end date (dropped months left out)
    deciles: pd.DataFrame      # the decile means, one column per bin
    breakpoints: pd.DataFrame  # date x edge: the distinct edges first, NaN after them (rule U2)
    counts: pd.DataFrame       # per date: ranked cells, breakpoint-set cells, cells kept by the screen
    mean: float                # of the long-short months
    sharpe: float              # annualised over 12 periods
    t_nw: float                # Newey-West t-statistic of the mean (Engine.newey_west)
    lags: int


def breakpoint_mask(tickers, breakpoint_tickers):
    """uint8 [N]: 1 for the tickers of the panel that are breakpoint tickers; None means all."""
    if breakpoint_tickers is None:
        return np.ones(len(tickers), dtype=np.uint8)
    known = set(breakpoint_tickers)
    return np.array([1 if tk in known else 0 for tk in tickers], dtype=np.uint8)


def shares_row(tickers, shares):
    """float64 [N]: shares outstanding per ticker of the panel from a mapping or Series ticker ->
    shares; NaN for a ticker that is missing or whose value is None or NaN."""
    get = shares.get if hasattr(shares, "get") else dict(shares).get
    out = np.full(len(tickers), np.nan)
    for i, tk in enumerate(tickers):
        v = get(tk)
        if v is not None and v is not pd.NA:
            out[i] = float(v)
    return out


def universe_momentum(daily_df, breakpoint_tickers=None, min_price=None, shares=None,
                      min_size_pct=None, J=12, skip=1, n_bins=10, K=1, signal="mom", device=None):
    """Long-short of a signal of the daily frame on a screened universe.  breakpoint_tickers: the
    tickers whose values set the decile edges and the size percentile (None: all).  min_price:
    drop cells whose formation month-end price is below it.  shares: ticker -> shares
    outstanding; cap = month price x shares, and cells with a cap under the min_size_pct
    percentile of the breakpoint tickers' caps that month are dropped (Engine.run_universe).
    K > 1 holds the cohorts K months (Engine.portfolio).  Returns a UniverseResult, or None when
    the frame holds no month."""
    if (shares is None) != (min_size_pct is None):
        raise ValueError("shares and min_size_pct go together")
    panel = from_long(daily_df)
    if panel.P.size == 0 or panel.T_m == 0:
        return None
    mask = breakpoint_mask(panel.tickers, breakpoint_tickers)
    if not mask.any():
        raise ValueError("no ticker of the frame is a breakpoint ticker")
    eng = get_engine(device)
    P, _, ms = upload_panel(panel, eng, with_volume=False)
    BP = torch.from_numpy(mask).to(eng.device)
    CAP = None
    if shares is not None:
        PM, _ = eng.month_end(P, ms)
        CAP = PM * torch.from_numpy(shares_row(panel.tickers, shares)).to(eng.device)
    out = eng.run_universe(P, ms, BP, min_price=min_price, CAP=CAP, min_size_pct=min_size_pct,
                           signal=signal, J=J, skip=skip, n_bins=n_bins)
    EW, LS = out.EW, out.LS
    if K > 1:
        pf = eng.portfolio(out.L, out.NR, n_bins, K=K, with_costs=False)
        EW, LS = pf.PR[:, 0, :].contiguous(), pf.LS[:, 0].contiguous()
    nw = eng.newey_west(LS)
    idx = pd.DatetimeIndex(panel.month_end, name="date")
    ls = pd.Series(LS.cpu().numpy(), index=idx, name="long_short").dropna()
    kept = out.NV if out.KEPT is None else out.KEPT
    counts = pd.DataFrame({"ranked": out.NV.cpu().numpy(), "breakpoint": out.NVB.cpu().numpy(),
                           "kept": kept.cpu().numpy()}, index=idx)
    return UniverseResult(
        long_short=ls,
        deciles=pd.DataFrame(EW.cpu().numpy(), index=idx, columns=list(range(n_bins))),
        breakpoints=pd.DataFrame(out.EDGES.cpu().numpy(), index=idx,
                                 columns=list(range(n_bins + 1))),
        counts=counts, mean=float(nw.MEAN), sharpe=float(sharpe(ls.values, 12)),
        t_nw=float(nw.T), lags=eng.default_lags(LS.shape[0]))


__all__ = ["UniverseResult", "breakpoint_mask", "shares_row", "universe_momentum"]
