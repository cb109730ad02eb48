"""Rules I1..I5 restated in NumPy: cross-sectional ranks per date or per
(date, group) -- pandas' rank(method='average' | 'min' | 'max', pct=...) -- and the per-month
Spearman and Pearson information coefficients on the joint observation set.  The CPU tests pin it
to pandas and scipy (tests/golden/rank_ic.npz); the GPU tests compare the engine against it.
"""
from __future__ import annotations

import math

import numpy as np

from group_ref import membership

METHODS = {"average": 0, "min": 1, "max": 2}


def lt_le(v):
    """I2: per value of v, the number of values below it and the number not above it."""
    srt = np.sort(v)
    return np.searchsorted(srt, v, side="left"), np.searchsorted(srt, v, side="right")


def rank_values(v, method="average", pct=False):
    """I2 on one segment's values (no NaN)."""
    n = len(v)
    lt, le = lt_le(v)
    m = METHODS[method]
    if m == 0:
        r = (lt + le + 1).astype(np.float64) / 2.0
    elif m == 1:
        r = (lt + 1).astype(np.float64)
    else:
        r = le.astype(np.float64)
    return r / float(n) if pct else r


def xs_rank(S, GID=None, n_groups=1, method="average", pct=False):
    """I1, I2: (RANK [T_m][N], NVG [T_m][n_groups] int32).  GID None: one group of every non-NaN
    cell."""
    T_m, N = S.shape
    if GID is None:
        assert n_groups == 1
        GID = np.zeros(N, dtype=np.int16)
    mem = membership(S, GID, n_groups)
    R = np.full((T_m, N), np.nan)
    NVG = np.zeros((T_m, n_groups), dtype=np.int32)
    for t in range(T_m):
        for g in np.unique(mem[t]):
            if g < 0:
                continue
            idx = np.nonzero(mem[t] == g)[0]
            NVG[t, g] = len(idx)
            R[t, idx] = rank_values(S[t, idx], method, pct)
    return R, NVG


def spearman_ints(s, y):
    """I4: (Sab, Saa, Sbb) as Python ints from the centred doubled ranks a = lt + le - n."""
    n = len(s)
    a = [int(l) + int(r) - n for l, r in zip(*lt_le(s))]
    b = [int(l) + int(r) - n for l, r in zip(*lt_le(y))]
    assert sum(a) == 0 and sum(b) == 0
    return (sum(p * q for p, q in zip(a, b)), sum(p * p for p in a), sum(q * q for q in b))


def pearson(s, y):
    """I5's two passes; the sums here are fsum (the device's order is within 1e-10 of any)."""
    n = len(s)
    ms, my = math.fsum(s) / n, math.fsum(y) / n
    ds, dy = s - ms, y - my
    css, cyy, csy = math.fsum(ds * ds), math.fsum(dy * dy), math.fsum(ds * dy)
    return csy / math.sqrt(css * cyy) if css > 0.0 and cyy > 0.0 else math.nan


def rank_ic(S, Y, lead=0, min_obs=10):
    """I3..I5: (RIC [T_m], PIC [T_m], NOBS [T_m] int32)."""
    T_m, N = S.shape
    RIC, PIC = np.full(T_m, np.nan), np.full(T_m, np.nan)
    NOBS = np.zeros(T_m, dtype=np.int32)
    for t in range(T_m):
        if t + lead >= T_m:
            continue
        ok = ~np.isnan(S[t]) & ~np.isnan(Y[t + lead])
        n = int(ok.sum())
        NOBS[t] = n
        if n < min_obs:
            continue
        s, y = S[t, ok], Y[t + lead, ok]
        sab, saa, sbb = spearman_ints(s, y)
        if saa > 0 and sbb > 0:
            RIC[t] = float(sab) / math.sqrt(float(saa) * float(sbb))
        PIC[t] = pearson(s, y)
    return RIC, PIC, NOBS
