"""CPU: pins tests/dailymkt_ref.py, the NumPy restatement of rules V1..V4 that the
GPU tests compare against, to independent computations: pandas' pct_change, np.polyfit, np.std,
a centred third moment, math.fsum, and a hand-built column of gaps."""
import math

import numpy as np
import pandas as pd
import pytest

import dailymkt_ref as DR
from conftest import bits_equal
from oracle import csmom_oracle as O
from oracle.synth_np import make_panel

T_DAYS = 782
GAPPY = dict(late=0.2, delist=0.2, nan_day=0.01, absent_month=0.01, nan_month=0.01)
DENSE = dict(late=0, delist=0, nan_day=0, absent_month=0, nan_month=0)


@pytest.fixture(scope="module")
def dense():
    pan = make_panel(40, T_DAYS, seed=140, cents=True, with_volume=False, **DENSE)
    assert not np.isnan(pan["P"]).any()
    out = DR.daily(pan["P"], pan["month_start"])
    out["P"], out["ms"] = pan["P"], pan["month_start"]
    return out


def test_dense_returns_are_pct_change(dense):
    want = pd.DataFrame(dense["P"]).pct_change(fill_method=None).to_numpy()
    assert bits_equal(dense["R"], want)
    assert np.isnan(dense["R"][0]).all() and not np.isnan(dense["R"][1:]).any()
    assert (dense["NMD"][1:] == 40).all() and dense["NMD"][0] == 0 and np.isnan(dense["MKTD"][0])


def _rel(got, want):
    return abs(got - want) / max(abs(want), 1e-300)


def test_model_against_polyfit_std_and_centred_moments(dense):
    Wm = 3
    R, F, ms = dense["R"], dense["MKTD"], dense["ms"]
    mod = DR.daily_model(dense, Wm)
    T_m = len(ms) - 1
    worst = dict.fromkeys(("DBETA", "DIVOL", "DTVOL", "DSKEW", "DMAX"), 0.0)
    for t in range(Wm - 1, T_m):
        lo, hi = int(ms[t - Wm + 1]), int(ms[t + 1])
        f = F[lo:hi]
        for a in range(R.shape[1]):
            r = R[lo:hi, a]
            ok = ~np.isnan(r) & ~np.isnan(f)
            x, y = f[ok], r[ok]
            n = len(y)
            assert mod["NOBS"][t, a] == n >= 15 * Wm
            b, c = np.polyfit(x, y, 1)
            e = y - (c + b * x)
            dev = y - y.mean()
            want = dict(DBETA=b, DIVOL=math.sqrt((e * e).sum() / (n - 2)), DTVOL=np.std(y, ddof=1),
                        DSKEW=(dev ** 3).mean() / (dev ** 2).mean() ** 1.5, DMAX=y.max())
            for k, w in want.items():
                worst[k] = max(worst[k], _rel(mod[k][t, a], w))
    print(worst)
    assert worst["DMAX"] == 0.0
    assert max(worst.values()) <= 1e-10, worst
    assert np.isnan(mod["DBETA"][:Wm - 1]).all() and (mod["NOBS"][:Wm - 1] == 0).all()


@pytest.mark.parametrize("N", [63, 2050])
def test_market_sum_is_within_b2s_bound_of_the_exact_mean(N):
    pan = make_panel(N, T_DAYS, seed=200 + N, cents=True, with_volume=False, **GAPPY)
    mk = DR.daily_market(pan["P"])
    days = 0
    for d in range(T_DAYS):
        r = mk["R"][d]
        r = r[~np.isnan(r)]
        assert mk["NMD"][d] == len(r)
        if len(r) == 0:
            assert np.isnan(mk["MKTD"][d])
            continue
        exact = math.fsum(r) / len(r)
        assert abs(mk["MKTD"][d] - exact) <= 2.0 ** -53 * (np.abs(r).sum() + abs(mk["MKTD"][d]))
        days += 1
    assert days >= T_DAYS - 5
    low = DR.daily_market(pan["P"], min_assets=N + 1)
    assert np.isnan(low["MKTD"]).all() and np.array_equal(low["NMD"], mk["NMD"])


@pytest.mark.parametrize("max_gap", [2, 3, 10])
def test_hand_built_gaps(max_gap):
    pan = make_panel(3, T_DAYS, seed=7, cents=True, with_volume=False, **DENSE)
    P, ms = pan["P"], pan["month_start"]
    col, cases = DR.gap_column(T_DAYS, max_gap, int(ms[8]), O.absent_scalar())
    P[:, 1] = col
    out = DR.daily(P, ms, max_gap)
    r = out["R"][:, 1]
    assert [c[2] for c in cases].count(False) == 2 and len(cases) >= 5
    for d, dp, booked in cases:
        assert not np.isnan(col[d]) and not np.isnan(col[dp]) and np.isnan(col[dp + 1:d]).all()
        assert d - dp in (max_gap - 1, max_gap, max_gap + 1)
        if booked:
            assert r[d] == col[d] / col[dp] - 1.0, (d, dp)
        else:
            assert np.isnan(r[d]), (d, dp)
        assert r[d + 1] == col[d + 1] / col[d] - 1.0
    # the straddling gap's return belongs to the month its priced row is in
    d, dp, _ = cases[-1]
    assert dp < ms[8] < d
    days8 = np.arange(int(ms[8]), int(ms[9]))
    assert out["NO"][8, 1] == (~np.isnan(r[days8])).sum() == len(days8) - 1
    assert out["RMAX"][8, 1] == np.nanmax(r[days8]) and d in days8 and not np.isnan(r[d])
    # every row that is not the end of a case's gap or row 0 has a price one row back
    booked_rows = (~np.isnan(r)).sum()
    holes = int(np.isnan(col).sum())
    assert booked_rows == T_DAYS - 1 - holes - 2


def test_one_asset_is_its_own_market():
    pan = make_panel(1, T_DAYS, seed=11, cents=True, with_volume=False, **DENSE)
    P, ms = pan["P"], pan["month_start"]
    P[np.arange(30, T_DAYS, 37), 0] = np.nan
    out = DR.daily(P, ms, 3)
    assert bits_equal(out["MKTD"], out["R"][:, 0])
    for Wm, mo in ((1, 15), (3, 45)):
        mod = DR.daily_model(out, Wm, mo)
        ok = ~np.isnan(mod["DBETA"])
        assert ok.sum() >= 30 - Wm
        assert (mod["DBETA"][ok] == 1.0).all() and (mod["DIVOL"][ok] == 0.0).all()
        assert np.array_equal(ok, ~np.isnan(mod["DIVOL"]))


def test_factor_gaps_remove_observations_and_zero_length_months():
    pan = make_panel(7, T_DAYS, seed=207, cents=True, with_volume=False, **GAPPY)
    P, ms = pan["P"], pan["month_start"]
    ms0 = np.concatenate([ms[:5], ms[4:]])   # month 4 has no day
    base = DR.daily(P, ms0)
    assert (base["NO"][4] == 0).all() and (base["SR"][4] == 0.0).all()
    assert np.isnan(base["RMAX"][4]).all()
    for k in DR.SUMS:
        assert bits_equal(np.delete(base[k], 4, axis=0), DR.daily(P, ms)[k]), k
    FD = base["MKTD"].copy()
    cut = np.arange(3, T_DAYS, 11)
    FD[cut] = np.nan
    own = DR.daily(P, ms0, FD=FD)
    lost = ~np.isnan(base["R"][cut]) & ~np.isnan(base["MKTD"][cut])[:, None]
    assert base["NO"].sum() - own["NO"].sum() == lost.sum() > 0
