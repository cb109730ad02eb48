"""Liquidity signals from a daily frame: Amihud's (2002) illiquidity, the dollar average daily
volume, and the shares of zero-return and zero-volume days per (ticker, month) (rules Q1..Q6 in
DESIGN.md section 7; Engine.liq_sums / liq_model).
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from ._lib import ABSENT_BITS
from .features import get_engine, upload_panel
from .panel import from_long

LIQUIDITY_COLUMNS = ["ticker", "date", "illiq", "dvol", "zret", "zvol", "nobs"]


def liquidity_signals(daily_df, window=12, min_obs=None, scale=1e6, device=None):
    """The liquidity signals of the daily frame's `adj_close` and `volume` columns over `window`
    calendar months: illiq (mean |daily return| / dollar volume, times scale), dvol (mean dollar
    volume of the priced days), zret and zvol (shares of zero-return and zero-volume days) and
    nobs (the days behind illiq).  min_obs counts days (default 15 * window); a cell short of it
    is NaN.  Returns a DataFrame of LIQUIDITY_COLUMNS, one row per (ticker, calendar month) with
    at least one daily row, sorted by (ticker, date), or None when the frame holds no month."""
    panel = from_long(daily_df)
    if panel.P.size == 0 or panel.T_m == 0:
        return None
    eng = get_engine(device)
    P, V, ms = upload_panel(panel, eng)
    PM, _ = eng.month_end(P, ms)
    lm = eng.liq_model(eng.liq_sums(P, V, ms, with_sv=False), window, min_obs, scale,
                       outputs=("ILLIQ", "DVOL", "ZRET", "ZVOL", "NOBS"))
    pm = PM.cpu().numpy()
    pres = (pm.view(np.uint64) & np.uint64(0x7FF7FFFFFFFFFFFF)) != np.uint64(ABSENT_BITS)
    aa, mm = np.nonzero(pres.T)
    host = {k: getattr(lm, k).cpu().numpy()[mm, aa] for k in ("ILLIQ", "DVOL", "ZRET", "ZVOL",
                                                              "NOBS")}
    return pd.DataFrame({"ticker": panel.tickers[aa], "date": panel.month_end[mm],
                         "illiq": host["ILLIQ"], "dvol": host["DVOL"], "zret": host["ZRET"],
                         "zvol": host["ZVOL"], "nobs": host["NOBS"]})


__all__ = ["LIQUIDITY_COLUMNS", "liquidity_signals"]
