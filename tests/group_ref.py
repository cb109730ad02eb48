"""Rules N1..N5 restated in NumPy: the reference's
groupby(['date', 'group'])['mom_J'].transform(assign_deciles_per_date), the groups' and the pooled
decile means, and the groups' statistics with the adjusted signals.  The CPU tests pin it to the
reference's own output (tests/golden/group_sorts.npz); the GPU tests compare the engine against it.
"""
from __future__ import annotations

import math

import numpy as np

from oracle.csmom_oracle import long_short, qcut_labels, quantile_table


def gid_rows(GID, T_m):
    """[T_m][N] view of the ids: a static [N] row is used for every month (g_ld = 0)."""
    GID = np.asarray(GID)
    return np.broadcast_to(GID, (T_m, GID.shape[-1])) if GID.ndim == 1 else GID


def membership(S, GID, n_groups):
    """N1: the group of every cell, -1 for none."""
    T_m, N = S.shape
    g = gid_rows(GID, T_m).astype(np.int64)
    ok = (g >= 0) & (g < n_groups) & ~np.isnan(S)
    return np.where(ok, g, -1)


def group_labels(S, GID, n_groups, n_bins=10, min_group=1, qtable=None):
    """N2: int8 [T_m][N], qcut_labels per (date, group) on the members' values alone."""
    T_m, N = S.shape
    qt = quantile_table(n_bins) if qtable is None else qtable
    mem = membership(S, GID, n_groups)
    L = np.full((T_m, N), -1, dtype=np.int8)
    for t in range(T_m):
        for g in np.unique(mem[t]):
            if g < 0:
                continue
            idx = np.nonzero(mem[t] == g)[0]
            if len(idx) < min_group:
                continue
            lab = qcut_labels(S[t, idx], n_bins, qt)
            L[t, idx] = np.where(np.isnan(lab), -1, lab).astype(np.int8)
    return L


def kahan(vals):
    """pandas' group_mean sum of `vals` in order (oracle.portfolio_ew's)."""
    s = c = 0.0
    for v in vals:
        y = v - c
        t = s + y
        cn = (t - s) - y
        c = 0.0 if math.isnan(cn) else cn
        s = t
    return s


def group_means(L, NR, mem, n_groups, n_bins):
    """N3 with Kahan sums in asset order.  Returns dict(SUMG, CNTG, EWG, EW, CNT, LS, NV, NVG)."""
    T_m, N = L.shape
    SUMG = np.zeros((T_m, n_groups, n_bins))
    CNTG = np.zeros((T_m, n_groups, n_bins), dtype=np.int32)
    NVG = np.zeros((T_m, n_groups), dtype=np.int32)
    keep = (L >= 0) & ~np.isnan(NR) & (mem >= 0)
    for t in range(T_m):
        for g in range(n_groups):
            inb = mem[t] == g
            NVG[t, g] = int(inb.sum())
            for d in range(n_bins):
                sel = np.nonzero(inb & keep[t] & (L[t] == d))[0]
                CNTG[t, g, d] = len(sel)
                SUMG[t, g, d] = kahan(NR[t, sel])
    with np.errstate(invalid="ignore", divide="ignore"):
        EWG = np.where(CNTG > 0, SUMG / np.maximum(CNTG, 1), np.nan)
        CNT = CNTG.sum(axis=1).astype(np.int32)
        tot = np.zeros((T_m, n_bins))
        for g in range(n_groups):
            tot = tot + SUMG[:, g, :]
        EW = np.where(CNT > 0, tot / np.maximum(CNT, 1), np.nan)
    return dict(SUMG=SUMG, CNTG=CNTG, EWG=EWG, EW=EW, CNT=CNT, LS=long_short(EW, CNT),
                NV=NVG.sum(axis=1).astype(np.int32), NVG=NVG)


def group_stats(S, GID, n_groups):
    """N4 with exactly rounded sums (math.fsum): GCNT, GMEAN = fsum / n, GSD."""
    T_m, N = S.shape
    mem = membership(S, GID, n_groups)
    GCNT = np.zeros((T_m, n_groups), dtype=np.int32)
    GMEAN = np.full((T_m, n_groups), np.nan)
    GSD = np.full((T_m, n_groups), np.nan)
    for t in range(T_m):
        for g in range(n_groups):
            v = S[t, mem[t] == g]
            n = len(v)
            GCNT[t, g] = n
            if n > 0:
                GMEAN[t, g] = math.fsum(v) / n
            if n > 1:
                GSD[t, g] = math.sqrt(math.fsum((v - GMEAN[t, g]) ** 2) / (n - 1))
    return GCNT, GMEAN, GSD


def adjusted(S, GID, n_groups, GMEAN, GSD):
    """N5 evaluated with the given GMEAN / GSD: (SA, SZ, SB), NaN outside every group."""
    T_m, N = S.shape
    mem = membership(S, GID, n_groups)
    rows = np.arange(T_m)[:, None]
    ok = mem >= 0
    m = np.where(ok, GMEAN[rows, np.maximum(mem, 0)], np.nan)
    sd = np.where(ok, GSD[rows, np.maximum(mem, 0)], np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        SA = np.where(ok, S - m, np.nan)
        SZ = np.where(ok & ~np.isnan(sd) & (sd != 0.0), SA / sd, np.nan)
    return SA, SZ, m
