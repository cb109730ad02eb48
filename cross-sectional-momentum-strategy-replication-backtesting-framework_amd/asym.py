"""Asymmetry signals from a daily frame: the information discreteness of Da, Gurun and Warachka
(2014), the signed jump variation and downside semi-volatility, and the downside beta, per
(ticker, month); and the "frog in the pan" double sort of momentum inside information-discreteness
bins (rules AS1..AS7 in DESIGN.md section 7; Engine.asym_sums / asym_model).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import pandas as pd
import torch

from ._lib import ABSENT_BITS
from .features import get_engine, upload_panel
from .lesw import dependent_double_sort
from .panel import from_long

ASYMMETRY_COLUMNS = ["ticker", "date", "info_disc", "rsj", "dsvol", "dnbeta", "nobs"]


def asymmetry_signals(daily_df, J=12, skip=1, min_obs=None, device=None):
    """The asymmetry signals of the daily frame's `adj_close` column: info_disc over the J months
    that end `skip` months back, signed by mom_J; rsj and dsvol of the month itself; dnbeta, the
    beta on the down days of the equal-weight daily market over 12 months; and nobs, the return
    days behind info_disc.  min_obs counts days as in Engine.asym_signals; a cell short of it is
    NaN.  Returns a DataFrame of ASYMMETRY_COLUMNS, one row per (ticker, calendar month) with at
    least one daily row, sorted by (ticker, date), or None when the frame holds no month."""
    panel = from_long(daily_df)
    if panel.P.size == 0 or panel.T_m == 0:
        return None
    eng = get_engine(device)
    P, _, ms = upload_panel(panel, eng, with_volume=False)
    PM, _ = eng.month_end(P, ms)
    sums = eng.asym_sums(P, ms, eng.daily_market(P)[0])
    _, M, _ = eng.momentum(PM, J, skip)
    min_side = None if min_obs is None else max(2, int(min_obs))
    form = eng.asym_model(sums, J, skip, M, min_obs, outputs=("ID", "NOBS"))
    month = eng.asym_model(sums, 1, 0, min_obs=min_obs, outputs=("RSJ", "DSVOL"))
    year = eng.asym_model(sums, 12, 0, min_side=min_side, outputs=("DNBETA",))
    pm = PM.cpu().numpy()
    pres = (pm.view(np.uint64) & np.uint64(0x7FF7FFFFFFFFFFFF)) != np.uint64(ABSENT_BITS)
    aa, mm = np.nonzero(pres.T)
    cols = {"info_disc": form.ID, "rsj": month.RSJ, "dsvol": month.DSVOL, "dnbeta": year.DNBETA,
            "nobs": form.NOBS}
    out = {"ticker": panel.tickers[aa], "date": panel.month_end[mm]}
    out.update({k: t.cpu().numpy()[mm, aa] for k, t in cols.items()})
    return pd.DataFrame(out)


@dataclass
class FipResult:
    long_short: pd.DataFrame  # winners minus losers inside each ID bin, indexed by month-end date
    spread: pd.Series         # ID bin 0 (continuous) minus ID bin n_id - 1 (discrete)
    cells: torch.Tensor       # [T_m][n_id][n_mom] cell returns (K-overlapped)
    table: pd.DataFrame       # mean, se, t, months of each bin's series and of the spread
    lags: int


def frog_in_the_pan(daily_df, J=12, skip=1, n_id=5, n_mom=5, K=1, min_obs=None, lags=None,
                    device=None):
    """Da, Gurun and Warachka's (2014) dependent double sort: n_id bins of the information
    discreteness each month, n_mom bins of mom_J inside each, the cells held K months, and the
    winners-minus-losers series of every ID bin with its Newey-West summary.  Momentum is
    expected to be strongest in bin 0, where information arrived in many small steps.  Returns a
    FipResult, or None when the frame holds no month."""
    panel = from_long(daily_df)
    if panel.P.size == 0 or panel.T_m == 0:
        return None
    eng = get_engine(device)
    P, _, ms = upload_panel(panel, eng, with_volume=False)
    PM, _ = eng.month_end(P, ms)
    _, M, _ = eng.momentum(PM, J, skip)
    ID = eng.asym_signals(P, ms, ("info_disc",), J, skip, None, min_obs, PM=PM)["info_disc"]
    Mx = eng.mask_by(ID, M)
    ds = dependent_double_sort(eng, ID, Mx, eng.next_ret(PM, Mx), n1=n_id, n2=n_mom, K=K)
    series = torch.cat([ds.LS, (ds.LS[:, 0] - ds.LS[:, n_id - 1]).unsqueeze(1)], dim=1)
    lags = eng.default_lags(panel.T_m) if lags is None else int(lags)
    nw = eng.newey_west(series.contiguous(), lags)
    idx = pd.DatetimeIndex(panel.month_end, name="date")
    host = series.cpu().numpy()
    table = pd.DataFrame({"mean": nw.MEAN.cpu().numpy(), "se": nw.SE.cpu().numpy(),
                          "t": nw.T.cpu().numpy(), "months": nw.NT.cpu().numpy()},
                         index=pd.Index([*range(n_id), "spread"], name="id_bin"))
    return FipResult(long_short=pd.DataFrame(host[:, :n_id], index=idx, columns=range(n_id)),
                     spread=pd.Series(host[:, n_id], index=idx, name="spread"), cells=ds.PR,
                     table=table, lags=lags)


__all__ = ["ASYMMETRY_COLUMNS", "FipResult", "asymmetry_signals", "frog_in_the_pan"]
