"""Rules U1..U6 restated in NumPy on top of oracle.csmom_oracle.qcut_edges /
quantile_table: the edges of each date from the breakpoint subset, every ranked cell's label
against them, the decile means (Kahan sums in asset order, oracle.portfolio_ew's), and the screen.
The CPU tests pin it to the reference's assign_deciles_per_date on the subset and to pandas'
qcut(retbins=True) / cut(include_lowest=True) (tests/golden/breakpoints.npz); the GPU tests compare
the engine against it.
"""
from __future__ import annotations

import numpy as np

from oracle.csmom_oracle import portfolio_ew, qcut_edges, quantile_table


def bp_rows(BP, T_m):
    """[T_m][N] view of the mask: a static [N] row is used for every month (bp_ld = 0)."""
    BP = np.asarray(BP)
    return np.broadcast_to(BP, (T_m, BP.shape[-1])) if BP.ndim == 1 else BP


def distinct_edges(values, n_bins, qtable=None):
    """U2 on one breakpoint set (no NaN in `values`): the distinct qcut edges in order."""
    if len(values) == 0:
        return np.empty(0)
    qt = quantile_table(n_bins) if qtable is None else qtable
    uniq = []
    for e in qcut_edges(np.sort(np.asarray(values, dtype=np.float64), kind="stable"), qt):
        if not any(e == u for u in uniq):   # (-0.0 == 0.0)
            uniq.append(e)
    return np.array(uniq)


def labels_row(x, e):
    """U3 on one date: x the row (NaN = not ranked), e its distinct edges."""
    lab = np.full(len(x), -1, dtype=np.int8)
    if len(e) < 2:
        return lab
    ok = ~np.isnan(x)
    inner = e[1:len(e) - 1]
    lab[ok] = (inner[None, :] < x[ok][:, None]).sum(axis=1).astype(np.int8)
    return lab


def breakpoints(M, BP, n_bins=10, qtable=None):
    """U1, U2: (EDGES [T_m][n_bins + 1] NaN-padded, NE, NVB)."""
    T_m, N = M.shape
    bp = bp_rows(BP, T_m)
    EDGES = np.full((T_m, n_bins + 1), np.nan)
    NE = np.zeros(T_m, dtype=np.int32)
    NVB = np.zeros(T_m, dtype=np.int32)
    for t in range(T_m):
        sel = ~np.isnan(M[t]) & (bp[t] != 0)
        e = distinct_edges(M[t, sel], n_bins, qtable)
        NVB[t] = int(sel.sum())
        NE[t] = len(e)
        EDGES[t, :len(e)] = e
    return EDGES, NE, NVB


def deciles_bp(M, NR, BP, n_bins=10, qtable=None):
    """U1..U4: dict(L, EDGES, NE, NVB, NV[, EW, CNT, LS])."""
    T_m, N = M.shape
    EDGES, NE, NVB = breakpoints(M, BP, n_bins, qtable)
    L = np.stack([labels_row(M[t], EDGES[t, :NE[t]]) for t in range(T_m)])
    out = dict(L=L, EDGES=EDGES, NE=NE, NVB=NVB, NV=(~np.isnan(M)).sum(axis=1).astype(np.int32))
    if NR is not None:
        EW, CNT, LS = portfolio_ew(L, NR, n_bins)
        out.update(EW=EW, CNT=CNT.astype(np.int32), LS=LS)
    return out


def screen(M, PM=None, min_price=None, CAP=None, CAPMIN=None):
    """U5: (MS, KEPT)."""
    keep = ~np.isnan(M)
    with np.errstate(invalid="ignore"):
        if PM is not None:
            keep &= PM >= min_price
        if CAP is not None:
            keep &= CAP >= np.asarray(CAPMIN)[:, None]
    return np.where(keep, M, np.nan), keep.sum(axis=1).astype(np.int32)
