"""Range-based signals from a daily frame: Parkinson's (1980) volatility, the Corwin-Schultz
(2012) high-low spread and the Abdi-Ranaldo (2017) close-high-low spread per (ticker, month)
(rules HL1..HL6 in DESIGN.md section 7; Engine.range_sums / range_model).
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from ._lib import ABSENT_BITS
from .features import get_engine, upload_panel, upload_range
from .panel import from_long

RANGE_COLUMNS = ["ticker", "date", "pkvol", "cs_spread", "ar_spread", "nobs"]


def range_signals(daily_df, window=1, min_obs=None, max_gap=1, device=None):
    """The range signals of the daily frame's raw `high`, `low` and `close` columns over `window`
    calendar months: pkvol (Parkinson's daily volatility), cs_spread and ar_spread (the
    Corwin-Schultz and Abdi-Ranaldo bid-ask spread estimates, as fractions of the price) and nobs
    (the pairs of ranged days behind ar_spread).  A pair is two ranged days at most max_gap panel
    rows apart.  min_obs counts days (default 15 * window); a cell short of it is NaN.  Returns a
    DataFrame of RANGE_COLUMNS, one row per (ticker, calendar month) with at least one daily row,
    sorted by (ticker, date), or None when the frame holds no month."""
    panel = from_long(daily_df)
    if panel.P.size == 0 or panel.T_m == 0:
        return None
    eng = get_engine(device)
    P, _, ms = upload_panel(panel, eng, with_volume=False)
    H, L, C = upload_range(daily_df, panel, eng)
    PM, _ = eng.month_end(P, ms)
    rm = eng.range_model(eng.range_sums(H, L, C, ms, max_gap), window, min_obs)
    pm = PM.cpu().numpy()
    pres = (pm.view(np.uint64) & np.uint64(0x7FF7FFFFFFFFFFFF)) != np.uint64(ABSENT_BITS)
    aa, mm = np.nonzero(pres.T)
    host = {k: getattr(rm, k).cpu().numpy()[mm, aa] for k in eng.RANGE_OUTPUTS}
    return pd.DataFrame({"ticker": panel.tickers[aa], "date": panel.month_end[mm],
                         "pkvol": host["PKVOL"], "cs_spread": host["CSSPR"],
                         "ar_spread": host["ARSPR"], "nobs": host["NOBS"]})


__all__ = ["RANGE_COLUMNS", "range_signals"]
