"""Information coefficients from a daily frame: each month's Spearman rank correlation of the
engine's signals with the return of the h-th month after formation, its mean, Newey-West
t-statistic, ICIR and hit rate per (signal, horizon) (rules I1..I6 in DESIGN.md section 7;
Engine.rank_ic / ic_decay).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import pandas as pd

from .engine import Engine
from .features import get_engine, upload_panel, upload_range
from .panel import from_long
from .regress import build_signals


@dataclass
class ICResult:
    table: pd.DataFrame       # one row per (signal, horizon): mean, se, t (Newey-West), icir, hit, months
    ic: pd.DataFrame          # the per-month rank ICs, indexed by month-end date, columns (signal, horizon)
    pearson: pd.DataFrame     # the per-month Pearson ICs, the same layout
    nobs: pd.DataFrame        # the per-month observations, the same layout
    lags: int


def ic_stats(x):
    """(icir, hit) of one IC series: mean / std(ddof=1) of the non-NaN months and the share of
    them above 0; NaN where undefined."""
    v = np.asarray(x, dtype=np.float64)
    v = v[~np.isnan(v)]
    if len(v) == 0:
        return float("nan"), float("nan")
    sd = v.std(ddof=1) if len(v) > 1 else float("nan")
    icir = float(v.mean() / sd) if sd == sd and sd > 0 else float("nan")
    return icir, float((v > 0).mean())


def information_coefficient(daily_df, signals=("mom", "high52", "beta", "ivol"),
                            horizons=(1, 3, 6, 12), J=12, skip=1, window=None, min_obs=10,
                            lags=None, device=None):
    """Rank ICs of the named signals (build_signals' names) with the month return (rule B1) of
    the h-th month after formation, for each h of horizons.  Returns an ICResult, or None when the
    frame holds no month."""
    names = tuple(signals)
    panel = from_long(daily_df)
    if panel.P.size == 0 or panel.T_m == 0:
        return None
    eng = get_engine(device)
    P, V, ms = upload_panel(panel, eng, with_volume=any(n in Engine.LIQ_SIGNALS for n in names))
    HLC = upload_range(daily_df, panel, eng) if any(n in Engine.RANGE_SIGNALS
                                                    for n in names) else None
    S, X = build_signals(eng, P, ms, names, J, skip, window, V=V, HLC=HLC)
    idx = pd.DatetimeIndex(panel.month_end, name="date")
    cols, ric, pic, nobs, rows = [], [], [], [], []
    used = 0
    for name, s in zip(names, S):
        d = eng.ic_decay(s, X, horizons, min_obs, lags)
        used = d.lags
        r = d.RIC.cpu().numpy()
        mean, se, t, nt = (v.cpu().numpy() for v in (d.MEAN, d.SE, d.T, d.NT))
        for k, h in enumerate(d.horizons):
            icir, hit = ic_stats(r[k])
            cols.append((name, h))
            rows.append(dict(mean=mean[k], se=se[k], t=t[k], icir=icir, hit=hit, months=int(nt[k])))
        ric.append(r)
        pic.append(d.PIC.cpu().numpy())
        nobs.append(d.NOBS.cpu().numpy())
    mi = pd.MultiIndex.from_tuples(cols, names=["signal", "horizon"])

    def frame(parts):
        return pd.DataFrame(np.concatenate(parts).T, index=idx, columns=mi)

    return ICResult(table=pd.DataFrame(rows, index=mi), ic=frame(ric), pearson=frame(pic),
                    nobs=frame(nobs), lags=used)


__all__ = ["ICResult", "ic_stats", "information_coefficient"]
