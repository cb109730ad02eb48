"""Sector-neutral momentum from a daily frame (Moskowitz-Grinblatt 1999): deciles formed inside
each group of each month and the legs pooled, or a plain sort of the group-adjusted signal (rules
N1..N6 in DESIGN.md section 7; Engine.run_neutral).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import pandas as pd
import torch

from .features import get_engine, upload_panel, upload_range
from .panel import from_long
from .utils import sharpe


@dataclass
class NeutralResult:
    long_short: pd.Series      # the neutral long-short per month-end date (dropped months left out)
    deciles: pd.DataFrame      # the pooled decile means, one column per bin
    group_long_short: pd.DataFrame | None   # EWG[:, g, n - 1] - EWG[:, g, 0], one column per group
    groups: list               # the group names, sorted: column g of the frames above is groups[g]
    mean: float                # of the long-short months
    sharpe: float              # annualised over 12 periods
    t_nw: float                # Newey-West t-statistic of the mean (Engine.newey_west)
    lags: int


def group_ids(tickers, groups):
    """The group id of each ticker: `groups` is a mapping or Series ticker -> label; a ticker that
    is missing, or whose label is None or NaN, gets -1 (no group).  The distinct labels, sorted,
    take the ids 0..G-1.  Returns (int16 [N], the sorted labels)."""
    get = groups.get if hasattr(groups, "get") else dict(groups).get
    labels = []
    for tk in tickers:
        lab = get(tk)
        if lab is None or (isinstance(lab, float) and lab != lab) or lab is pd.NA:
            lab = None
        labels.append(lab)
    names = sorted({lab for lab in labels if lab is not None})
    if len(names) > 256:
        raise ValueError(f"{len(names)} groups: at most 256")
    idx = {lab: i for i, lab in enumerate(names)}
    gid = np.array([-1 if lab is None else idx[lab] for lab in labels], dtype=np.int16)
    return gid, names


def neutral_momentum(daily_df, groups, J=12, skip=1, n_bins=10, K=1, min_group=None,
                     signal="mom", adjust=None, device=None):
    """Group-neutral long-short of a signal of the daily frame.  groups: ticker -> label (see
    group_ids); min_group None means n_bins; K > 1 holds the cohorts K months (Engine.portfolio).
    adjust None ranks inside the groups, "demean" / "zscore" rank the group-adjusted signal over
    the whole cross-section.  Returns a NeutralResult, or None when the frame holds no month."""
    panel = from_long(daily_df)
    if panel.P.size == 0 or panel.T_m == 0:
        return None
    gid, names = group_ids(panel.tickers, groups)
    if not names:
        raise ValueError("no ticker of the frame has a group")
    eng = get_engine(device)
    P, V, ms = upload_panel(panel, eng, with_volume=signal in eng.LIQ_SIGNALS)
    HLC = upload_range(daily_df, panel, eng) if signal in eng.RANGE_SIGNALS else None
    GID = torch.from_numpy(gid).to(eng.device)
    G = len(names)
    mg = int(n_bins) if min_group is None else int(min_group)
    out = eng.run_neutral(P, ms, GID, G, signal=signal, adjust=adjust, J=J, skip=skip,
                          n_bins=n_bins, min_group=mg, V=V, HLC=HLC)
    EW, LS = out.EW, out.LS
    if K > 1:
        pf = eng.portfolio(out.L, out.NR, n_bins, K=K, with_costs=False)
        EW, LS = pf.PR[:, 0, :].contiguous(), pf.LS[:, 0].contiguous()
    gls = None
    if adjust is None:
        _, _, _, EWG, _, _ = eng.deciles_within(out.M, out.NR, GID, G, n_bins, mg,
                                                with_groups=True)
        gls = EWG[:, :, n_bins - 1] - EWG[:, :, 0]
    nw = eng.newey_west(LS)
    idx = pd.DatetimeIndex(panel.month_end, name="date")
    ls = pd.Series(LS.cpu().numpy(), index=idx, name="long_short").dropna()
    return NeutralResult(
        long_short=ls,
        deciles=pd.DataFrame(EW.cpu().numpy(), index=idx, columns=list(range(n_bins))),
        group_long_short=None if gls is None else pd.DataFrame(gls.cpu().numpy(), index=idx,
                                                               columns=names),
        groups=names, mean=float(nw.MEAN), sharpe=float(sharpe(ls.values, 12)),
        t_nw=float(nw.T), lags=eng.default_lags(LS.shape[0]))


__all__ = ["NeutralResult", "group_ids", "neutral_momentum"]
