"""Generate tests/golden/group_sorts.npz by running the REFERENCE's own ranking inside groups
(run once, in the build container; the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_group_golden.py

The reference is imported the way make_golden.py imports it (its load_reference: a `yfinance`
stub, a scratch working directory, plotting disabled).  Every case runs

    df.groupby(['date', 'group'])['mom_J'].transform(assign_deciles_per_date)

and stores inputs and labels as data only:

* the edge panel's 12-1 momentum (edge.npz J12s1_M) under three group maps -- one group; four
  uneven groups with one single-ticker group and some tickers unmapped; a map that moves assets
  between groups over time;
* synthetic cross-sections: group sizes 1-400, values rounded to cents (ties), all-equal groups,
  +-0.0, n_bins 2, 3, 5, 10.

Layout: panel cases `<name>_gid` int16 [T_m][N] (the signal is edge.npz's) and `<name>_L` int8
(-1 = NaN); synthetic cases flat: `xs_values`, `xs_gid`, `xs_labels` (float, NaN kept) with
`xs_offsets` [cases + 1] and `xs_nbins` [cases].
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


def ref_labels(rd, values, dates, groups, n_bins):
    """The reference's transform on a long frame; rows without a group are left out (NaN)."""
    df = pd.DataFrame({"date": dates, "group": groups, "mom_J": values})
    has = df["group"] >= 0
    out = np.full(len(df), np.nan)
    sub = df[has]
    if len(sub):
        lab = sub.groupby(["date", "group"])["mom_J"].transform(
            lambda s: rd.assign_deciles_per_date(s, n=n_bins))
        out[np.nonzero(has.to_numpy())[0]] = lab.to_numpy(dtype=np.float64)
    return out


def panel_case(rd, M, gid, n_bins=10):
    T_m, N = M.shape
    dates = np.repeat(np.arange(T_m), N)
    lab = ref_labels(rd, M.ravel(), dates, gid.ravel().astype(np.int64), n_bins).reshape(T_m, N)
    return np.where(np.isnan(lab), -1, lab).astype(np.int8)


def panel_maps(T_m, N, rng):
    one = np.zeros((T_m, N), dtype=np.int16)
    row = rng.choice(np.array([0, 1, 2, -1], dtype=np.int16), size=N, p=[0.55, 0.25, 0.1, 0.1])
    row[7] = 3   # a group of a single ticker
    four = np.broadcast_to(row, (T_m, N)).copy()
    moving = rng.integers(0, 5, size=N).astype(np.int16)
    mv = np.empty((T_m, N), dtype=np.int16)
    for t in range(T_m):
        move = rng.random(N) < 0.08
        moving = np.where(move, rng.integers(-1, 5, size=N), moving).astype(np.int16)
        mv[t] = moving
    return {"one": (one, 1), "four": (four, 4), "moving": (mv, 5)}


def synthetic(rd, rng, cases=300):
    vals, gids, labs, offs, nbs = [], [], [], [0], []
    for c in range(cases):
        n_bins = (2, 3, 5, 10)[c % 4]
        n_groups = int(rng.integers(1, 6))
        sizes = [int(rng.integers(1, 401)) if rng.random() < 0.25 else int(rng.integers(1, 41))
                 for _ in range(n_groups)]
        v, g = [], []
        for k, n in enumerate(sizes):
            kind = rng.random()
            if kind < 0.12:
                x = np.full(n, float(np.round(rng.normal(), 2)))      # all-equal group
            elif kind < 0.24:
                x = rng.choice(np.array([0.0, -0.0, 0.01, -0.01]), size=n)   # +-0.0 and ties
            elif kind < 0.7:
                x = np.round(rng.normal(0.0, 0.05, size=n), 2)        # cent ties
            else:
                x = rng.normal(0.0, 0.3, size=n)
            v.append(x)
            g.append(np.full(n, k, dtype=np.int16))
        v, g = np.concatenate(v), np.concatenate(g)
        perm = rng.permutation(len(v))
        v, g = v[perm], g[perm]
        lab = ref_labels(rd, v, np.zeros(len(v), dtype=np.int64), g.astype(np.int64), n_bins)
        vals.append(v)
        gids.append(g)
        labs.append(lab)
        offs.append(offs[-1] + len(v))
        nbs.append(n_bins)
    return dict(xs_values=np.concatenate(vals), xs_gid=np.concatenate(gids),
                xs_labels=np.concatenate(labs), xs_offsets=np.array(offs, dtype=np.int64),
                xs_nbins=np.array(nbs, dtype=np.int32))


def main():
    edge = np.load(OUT / "edge.npz", allow_pickle=False)
    M = edge["J12s1_M"].copy()
    rd, *_ = make_golden.load_reference()
    rng = np.random.default_rng(20260113)
    out = {"pandas_version": np.array(pd.__version__), "numpy_version": np.array(np.__version__)}
    for name, (gid, n_groups) in panel_maps(*M.shape, rng).items():
        out[f"{name}_gid"] = gid
        out[f"{name}_ngroups"] = np.array(n_groups, dtype=np.int32)
        out[f"{name}_L"] = panel_case(rd, M, gid)
    out.update(synthetic(rd, rng))
    np.savez_compressed(OUT / "group_sorts.npz", **out)
    print("wrote", OUT / "group_sorts.npz", (OUT / "group_sorts.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    sys.exit(main())
