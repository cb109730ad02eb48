"""Generate tests/golden/breakpoints.npz: breakpoints taken from a subset of a cross-section and
applied to all of it, by the REFERENCE's own ranking and by pandas (run once, in the build
container; the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_bp_golden.py

The reference is imported the way make_golden.py imports it.  For every (date, subset) the file
records, as data only:

* `assign_deciles_per_date` on the subset's values alone (the reference's labels of the subset);
* the `retbins` of `pd.qcut(subset, n_bins, retbins=True, duplicates='drop')`;
* `pd.cut(row, bins=retbins, labels=False, include_lowest=True)` on the whole row, NaN where
  pandas puts a cell out of range (and everywhere when there are fewer than two bins).

Cases: the edge panel's 12-1 momentum (edge.npz J12s1_M) with a static subset (mask bytes 0, 1 and
200) and a subset that moves over time (one date with a single member, one with two); synthetic
rows of sizes 1-500, n_bins 2 / 3 / 5 / 10 / 20, values rounded to cents (ties), all-equal subsets,
+-0.0.

Layout: panel cases `<name>_bp` uint8, `<name>_Lsub` int8 [T_m][N] (-1 = NaN or not in the
subset), `<name>_edges` [T_m][11] NaN-padded with `<name>_ne`, `<name>_cut` float [T_m][N];
synthetic cases flat: `xs_values`, `xs_bp`, `xs_sub` (float labels, NaN kept), `xs_cut`, with
`xs_offsets` [cases + 1], `xs_nbins`, `xs_edges` [cases][21] and `xs_ne`.
"""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

import numpy as np
import pandas as pd

OUT = Path(__file__).resolve().parent
_spec = importlib.util.spec_from_file_location("make_golden", OUT / "make_golden.py")
make_golden = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_golden)


def one_row(rd, x, bp, n_bins):
    """(sub labels [n] float, retbins, cut [n] float) of one cross-section x with mask bp."""
    n = len(x)
    sub = np.full(n, np.nan)
    cut = np.full(n, np.nan)
    sel = ~np.isnan(x) & (bp != 0)
    if not sel.any():
        return sub, np.empty(0), cut
    s = pd.Series(x[sel])
    sub[sel] = rd.assign_deciles_per_date(s, n=n_bins).to_numpy(dtype=np.float64)
    _, bins = pd.qcut(s, n_bins, labels=False, retbins=True, duplicates="drop")
    bins = np.asarray(bins, dtype=np.float64)
    if len(bins) >= 2:
        cut = pd.cut(pd.Series(x), bins=bins, labels=False,
                     include_lowest=True).to_numpy(dtype=np.float64)
    return sub, bins, cut


def panel_case(rd, M, BP, n_bins=10):
    T_m, N = M.shape
    bp = np.broadcast_to(BP, (T_m, N))
    Lsub = np.full((T_m, N), -1, dtype=np.int8)
    cut = np.full((T_m, N), np.nan)
    edges = np.full((T_m, n_bins + 1), np.nan)
    ne = np.zeros(T_m, dtype=np.int32)
    for t in range(T_m):
        sub, bins, cut[t] = one_row(rd, M[t], bp[t], n_bins)
        Lsub[t] = np.where(np.isnan(sub), -1, sub).astype(np.int8)
        edges[t, :len(bins)] = bins
        ne[t] = len(bins)
    return dict(Lsub=Lsub, cut=cut, edges=edges, ne=ne)


def panel_masks(M, rng):
    T_m, N = M.shape
    static = rng.choice(np.array([0, 1, 200], dtype=np.uint8), size=N, p=[0.6, 0.3, 0.1])
    row = (rng.random(N) < 0.4).astype(np.uint8)
    moving = np.empty((T_m, N), dtype=np.uint8)
    for t in range(T_m):
        flip = rng.random(N) < 0.1
        row = np.where(flip, 1 - row, row).astype(np.uint8)
        moving[t] = row
    full = np.nonzero((~np.isnan(M)).sum(axis=1) > 10)[0]
    for t, k in ((full[1], 1), (full[2], 2)):   # a date with one member, a date with two
        ok = np.nonzero(~np.isnan(M[t]))[0]
        moving[t] = 0
        moving[t, ok[:k]] = 1
    return {"static": static, "moving": moving}


def synthetic(rd, rng, cases=40):
    vals, bps, subs, cuts, offs, nbs, ne = [], [], [], [], [0], [], []
    edges = np.full((cases, 21), np.nan)
    sizes = [1, 2, 3, 500] + [int(rng.integers(4, 500)) for _ in range(cases - 4)]
    for c in range(cases):
        n, n_bins = sizes[c], (2, 3, 5, 10, 20)[c % 5]
        kind = c % 4
        if kind == 0:
            x = np.round(rng.normal(0.0, 0.05, size=n), 2)               # cent ties
        elif kind == 1:
            x = rng.choice(np.array([0.0, -0.0, 0.01, -0.01, 0.02]), size=n)   # +-0.0 and ties
        elif kind == 2:
            x = rng.normal(0.0, 0.3, size=n)
        else:
            x = np.round(rng.normal(0.0, 0.1, size=n), 2)
            x[rng.random(n) < 0.1] = -0.0
        bp = (rng.random(n) < (0.3 if c % 3 else 0.6)).astype(np.uint8)
        if c % 9 == 5:                                                   # an all-equal subset
            x[bp != 0] = float(np.round(rng.normal(), 2))
        sub, bins, cut = one_row(rd, x, bp, n_bins)
        vals.append(x)
        bps.append(bp)
        subs.append(sub)
        cuts.append(cut)
        offs.append(offs[-1] + n)
        nbs.append(n_bins)
        edges[c, :len(bins)] = bins
        ne.append(len(bins))
    return dict(xs_values=np.concatenate(vals), xs_bp=np.concatenate(bps),
                xs_sub=np.concatenate(subs), xs_cut=np.concatenate(cuts),
                xs_offsets=np.array(offs, dtype=np.int64), xs_nbins=np.array(nbs, dtype=np.int32),
                xs_edges=edges, xs_ne=np.array(ne, dtype=np.int32))


def main():
    edge = np.load(OUT / "edge.npz", allow_pickle=False)
    M = edge["J12s1_M"].copy()
    rd, *_ = make_golden.load_reference()
    rng = np.random.default_rng(20261020)
    out = {"pandas_version": np.array(pd.__version__), "numpy_version": np.array(np.__version__)}
    for name, bp in panel_masks(M, rng).items():
        out[f"{name}_bp"] = bp
        for k, v in panel_case(rd, M, bp).items():
            out[f"{name}_{k}"] = v
    out.update(synthetic(rd, rng))
    np.savez_compressed(OUT / "breakpoints.npz", **out)
    print("wrote", OUT / "breakpoints.npz", (OUT / "breakpoints.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    sys.exit(main())
