"""Generate tests/golden/rank_ic.npz: inputs with pandas' and scipy's own ranks and correlations
(run once, where pandas and scipy are installed):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_rank_golden.py

Data only.  Layout:

* `row_S` [T][N] cents-rounded rows with NaN, `row_gid` [T][N] int16 (ids -1..3), and per method m
  of average / min / max and p of 0 / 1: `row_<m>_<p>` = DataFrame.rank(axis=1, method=m, pct=p),
  `grp_<m>_<p>` = the long frame's groupby(['date', 'group']).rank(method=m, pct=p) (NaN where the
  id is negative);
* flat cross-sections of 3..400 values (ties, all-equal, +-0.0): `xs_values`, `xs_offsets`
  [cases + 1], `xs_<m>_<p>` = Series.rank;
* IC pairs `ic_S`, `ic_Y` flat with `ic_offsets` (NaN in both, ties in both): `ic_spearman`
  (scipy.stats.spearmanr on the joint non-NaN set), `ic_spearman_pd` (pandas corr(method=
  'spearman')), `ic_pearson` (np.corrcoef), `ic_n` the observations.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pandas as pd
import scipy
from scipy.stats import spearmanr

OUT = Path(__file__).resolve().parent
METHODS = ("average", "min", "max")


def rows(rng, T=6, N=97):
    S = np.round(rng.normal(0.0, 0.05, (T, N)), 2)
    S[rng.random((T, N)) < 0.2] = np.nan
    S[T - 1] = np.nan                      # an all-NaN row
    S[T - 2, 1:] = np.nan                  # n = 1
    gid = rng.integers(-1, 4, (T, N)).astype(np.int16)
    out = {"row_S": S, "row_gid": gid}
    df = pd.DataFrame(S)
    long = pd.DataFrame({"date": np.repeat(np.arange(T), N), "group": gid.ravel().astype(np.int64),
                         "v": S.ravel()})
    has = (long["group"] >= 0).to_numpy()
    for m in METHODS:
        for p in (0, 1):
            out[f"row_{m}_{p}"] = df.rank(axis=1, method=m, pct=bool(p)).to_numpy()
            g = np.full(T * N, np.nan)
            g[has] = long[has].groupby(["date", "group"])["v"].rank(method=m, pct=bool(p)).to_numpy()
            out[f"grp_{m}_{p}"] = g.reshape(T, N)
    return out


def draw(rng, n):
    kind = rng.random()
    if kind < 0.1:
        return np.full(n, float(np.round(rng.normal(), 2)))
    if kind < 0.2:
        return rng.choice(np.array([0.0, -0.0, 0.01, -0.01]), size=n)
    if kind < 0.7:
        return np.round(rng.normal(0.0, 0.05, size=n), 2)
    return rng.normal(0.0, 0.3, size=n)


def sections(rng, cases=60):
    vals, offs = [], [0]
    res = {f"xs_{m}_{p}": [] for m in METHODS for p in (0, 1)}
    for _ in range(cases):
        n = int(rng.integers(3, 401)) if rng.random() < 0.2 else int(rng.integers(3, 41))
        v = draw(rng, n)
        vals.append(v)
        offs.append(offs[-1] + n)
        for m in METHODS:
            for p in (0, 1):
                res[f"xs_{m}_{p}"].append(pd.Series(v).rank(method=m, pct=bool(p)).to_numpy())
    out = {k: np.concatenate(v) for k, v in res.items()}
    out["xs_values"] = np.concatenate(vals)
    out["xs_offsets"] = np.array(offs, dtype=np.int64)
    return out


def pairs(rng, cases=60):
    ss, ys, offs, sp, spd, pe, ns = [], [], [0], [], [], [], []
    for c in range(cases):
        n = int(rng.integers(12, 401)) if c % 3 == 0 else int(rng.integers(12, 61))
        s = np.round(rng.normal(0.0, 0.1, n), 2)
        y = 0.3 * s + rng.normal(0.0, 0.1, n)
        if c % 2 == 0:
            y = np.round(y, 2)
        s[rng.random(n) < 0.15] = np.nan
        y[rng.random(n) < 0.15] = np.nan
        ok = ~np.isnan(s) & ~np.isnan(y)
        ss.append(s)
        ys.append(y)
        offs.append(offs[-1] + n)
        ns.append(int(ok.sum()))
        sp.append(float(spearmanr(s[ok], y[ok])[0]))
        spd.append(float(pd.Series(s).corr(pd.Series(y), method="spearman")))
        pe.append(float(np.corrcoef(s[ok], y[ok])[0, 1]))
    return dict(ic_S=np.concatenate(ss), ic_Y=np.concatenate(ys),
                ic_offsets=np.array(offs, dtype=np.int64), ic_spearman=np.array(sp),
                ic_spearman_pd=np.array(spd), ic_pearson=np.array(pe),
                ic_n=np.array(ns, dtype=np.int32))


def main():
    rng = np.random.default_rng(20261020)
    out = {"pandas_version": np.array(pd.__version__), "numpy_version": np.array(np.__version__),
           "scipy_version": np.array(scipy.__version__)}
    out.update(rows(rng))
    out.update(sections(rng))
    out.update(pairs(rng))
    np.savez_compressed(OUT / "rank_ic.npz", **out)
    print("wrote", OUT / "rank_ic.npz", (OUT / "rank_ic.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    sys.exit(main())
