"""Fama-MacBeth (1973) regressions from a daily frame: next month's return regressed each month
on the engine's signals across the assets, the monthly slopes averaged over time and judged by
Newey-West t-statistics (rules R1..R6 in DESIGN.md section 7; Engine.fama_macbeth).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import pandas as pd
import torch

from .engine import Engine
from .features import get_engine, upload_panel, upload_range
from .panel import from_long

SIGNAL_NAMES = ("mom", "rev", *Engine.RUN_SIGNALS)


@dataclass
class FamaMacBethResult:
    table: pd.DataFrame       # one row per coefficient ('const', then the signals): mean, se, t, months
    gammas: pd.DataFrame      # the per-month coefficients, indexed by month-end date
    r2: pd.Series             # the per-month R2
    nobs: pd.Series           # the per-month observations
    r2_mean: float
    lags: int


def build_signals(eng: Engine, P, month_start, names, J=12, skip=1, window=None, V=None,
                  HLC=None):
    """The named signals of a daily panel on the device, each [T_m][N], with the B1 month return
    X: "mom" (mom_J), "rev" (the month's own return) and Engine.RUN_SIGNALS' names, built by the
    calls run_signal makes.  window None: 12 months for "high52" / "mom_vol" and "dbeta", 36 for
    the monthly market model's, 1 for "divol", "dskew" and "max", 12 for the liquidity names
    "illiq", "dvol" and "zret", which need the daily volume panel V [T_d][N], and 1 for the range
    names "pkvol", "cs_spread" and "ar_spread", which need the daily high, low and close panels
    HLC = (H, L, C).  The asymmetry names follow Engine.asym_signals: "info_disc" covers the J
    months that end `skip` months back whatever `window` is, "rsj" and "dsvol" default to 1 month
    and "dnbeta" to 12."""
    unknown = [n for n in names if n not in SIGNAL_NAMES]
    if unknown:
        raise ValueError(f"signals must be among {SIGNAL_NAMES}, got {unknown}")
    liq = [n for n in names if n in Engine.LIQ_SIGNALS]
    if liq and V is None:
        raise ValueError(f"signals {liq} need the daily volume panel V")
    rng = [n for n in names if n in Engine.RANGE_SIGNALS]
    if rng and HLC is None:
        raise ValueError(f"signals {rng} need the daily panels HLC = (H, L, C)")
    st = eng.month_stats(P, month_start)
    _, _, X = eng.market_factor(st.PM, with_x=True)
    out = {}
    if "rev" in names:
        out["rev"] = X
    if "mom" in names or "mom_vol" in names:
        _, M, _ = eng.momentum(st.PM, J, skip)
        out["mom"] = M
    daily = [n for n in ("high52", "mom_vol") if n in names]
    if daily:
        wd = 12 if window is None else int(window)
        fields = {"high52": "H52", "mom_vol": "MS"}
        sig = eng.window_signals(*st, M=out.get("mom"), Jh=wd, Jv=wd,
                                 outputs=tuple(fields[n] for n in daily))
        for n in daily:
            out[n] = getattr(sig, fields[n])
    market = [n for n in names if n in Engine.MARKET_SIGNALS]
    if market:
        mm = eng.market_model(st.PM, window=36 if window is None else int(window), J=J, skip=skip,
                              outputs=tuple(Engine.MARKET_SIGNALS[n] for n in market))
        for n in market:
            out[n] = getattr(mm, Engine.MARKET_SIGNALS[n])
    dsig = [n for n in names if n in Engine.DAILY_SIGNALS]
    if dsig:
        out.update(eng.daily_signals(P, month_start, dsig, window))
    asym = [n for n in names if n in Engine.ASYM_SIGNALS]
    if asym:
        out.update(eng.asym_signals(P, month_start, asym, J, skip, window, PM=st.PM))
    if liq:
        out.update(eng.liq_signals(P, V, month_start, liq, window))
    if rng:
        out.update(eng.range_signals(*HLC, month_start, rng, window))
    return [out[n] for n in names], X


def fama_macbeth(daily_df, signals=("mom", "high52", "beta", "ivol"), J=12, skip=1, window=None,
                 weights=None, standardize=True, ridge=0.0, lags=None, device=None,
                 transform=None):
    """Fama-MacBeth regressions of next month's return on the named signals.  Y[t] is the month
    return (rule B1) of month t + 1; weights, when given, is a [T_m][N] array or tensor in the
    dense panel's layout (from_long).  transform "rank" replaces each signal by its
    cross-sectional percentile rank (Engine.xs_rank(pct=True), rules I1, I2) before the
    regressions.  Returns a FamaMacBethResult, or None when the frame holds no month."""
    names = tuple(signals)
    if transform not in (None, "rank"):
        raise ValueError(f"transform must be None or 'rank', got {transform!r}")
    panel = from_long(daily_df)
    if panel.P.size == 0 or panel.T_m == 0:
        return None
    eng = get_engine(device)
    P, V, ms = upload_panel(panel, eng, with_volume=any(n in Engine.LIQ_SIGNALS for n in names))
    HLC = upload_range(daily_df, panel, eng) if any(n in Engine.RANGE_SIGNALS
                                                    for n in names) else None
    S, X = build_signals(eng, P, ms, names, J, skip, window, V=V, HLC=HLC)
    if transform == "rank":
        S = [eng.xs_rank(s, pct=True) for s in S]
    Y = torch.cat([X[1:], torch.full_like(X[:1], float("nan"))])
    W = None
    if weights is not None:
        W = torch.as_tensor(np.ascontiguousarray(weights) if isinstance(weights, np.ndarray)
                            else weights, dtype=torch.float64).to(eng.device).contiguous()
    out = eng.fama_macbeth(Y, S, W, standardize, ridge, lags=lags)
    idx = pd.DatetimeIndex(panel.month_end, name="date")
    cols = ["const", *names]
    table = pd.DataFrame({"mean": out.MEAN.cpu().numpy(), "se": out.SE.cpu().numpy(),
                          "t": out.T.cpu().numpy(), "months": out.NT.cpu().numpy()},
                         index=pd.Index(cols, name="coefficient"))
    return FamaMacBethResult(
        table=table, gammas=pd.DataFrame(out.GAMMA.cpu().numpy(), index=idx, columns=cols),
        r2=pd.Series(out.R2.cpu().numpy(), index=idx, name="r2"),
        nobs=pd.Series(out.NOBS.cpu().numpy(), index=idx, name="nobs"),
        r2_mean=float(out.R2_MEAN), lags=out.lags)


__all__ = ["FamaMacBethResult", "SIGNAL_NAMES", "build_signals", "fama_macbeth"]
