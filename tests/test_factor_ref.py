"""CPU: pins tests/factor_ref.py, the NumPy restatement of rules MF1..MF7 that the
GPU tests compare against: its collapse onto market_ref / dailymkt_ref at KF = 1 (rule MF8, bit
for bit), its coefficients against np.linalg.lstsq at KF = 2, 3, 4, a collinear pair, NaN factor
rows; and csmom.factors.align_factors.

Least squares.  The figure is max_k |coefficient_k - lstsq_k| / max_k |lstsq_k| over the KF
slopes and the intercept of a cell.  Largest values measured over the sampled cells: monthly
3.836e-14 (KF = 3), daily 9.169e-14 (KF = 3; the daily model works on raw moment sums, which
cancel more than the monthly model's centred ones); both are printed by the tests, and each bar
is one decade above its figure.  The interpolating window Wb = KF + 1 is not compared with lstsq
(its error is its matrix's conditioning: up to 1.1e-11 on these factors);
test_smallest_window_interpolates holds it to R2 = 1 instead.
"""
import numpy as np
import pandas as pd
import pytest

import dailymkt_ref as DR
import factor_ref as FR
import market_ref as MR
from conftest import bits_equal
from oracle.synth_np import make_panel

LSTSQ_TOL = FR.LSTSQ_TOL
# (Wb, J, skip, min_obs) of the multi-factor tests (test_gpu_factor_model.py's)
CASES = [(24, 11, 1, 18), (12, 6, 1, 10), (8, 2, 0, 8), (36, 12, 1, 24), (60, 12, 1, 40)]
DAILY_CASES = [(1, 15), (3, 45), (12, 180), (1, 3)]
_M, _D = {}, {}


def _monthly():
    if not _M:
        PM = MR.panel(130, "gappy")["PM"]
        _M.update(PM=PM, MKT=MR.market_factor(PM)["MKT"])
    return _M


def _daily():
    if not _D:
        pan = make_panel(130, 320, seed=430, cents=True, with_volume=False, **MR.GAPPY)
        out = DR.daily(pan["P"], pan["month_start"])
        assert len(pan["month_start"]) - 1 == 15
        _D.update(ms=pan["month_start"], R=out["R"], MKTD=out["MKTD"], sums=out, fs={})
    return _D


def _fsums(KF, nan_at=(100, 1)):
    d = _daily()
    key = (KF, nan_at)
    if key not in d["fs"]:
        FD = FR.seeded_factors(d["MKTD"], 77, KF, 0.01, nan_at)
        d["fs"][key] = (FD, FR.daily_fsums(d["R"], FD, d["ms"]))
    return d["fs"][key]


# ------------------------------------------------------------------------------- MF8
@pytest.mark.parametrize("case", MR.CASES)
def test_one_factor_is_the_market_model(case):
    m = _monthly()
    want = MR.market_model(m["PM"], m["MKT"], *case)
    got = FR.factor_model(m["PM"], m["MKT"], *case)
    assert got["BETA"].shape == (1, 60, 130)
    assert bits_equal(got["BETA"][0], want["BETA"])
    for k in ("ALPHA", "IVOL", "RESMOM"):
        assert bits_equal(got[k], want[k]), k
    assert np.array_equal(got["NOBS"], want["NOBS"])
    if case[0] < 60:
        assert (~np.isnan(want["BETA"])).mean() >= 0.2


def test_one_factor_is_the_daily_model():
    d = _daily()
    got = FR.daily_fsums(d["R"], d["MKTD"], d["ms"])
    assert np.array_equal(got["NO"], d["sums"]["NO"])
    for k in ("SR", "SRR"):
        assert bits_equal(got[k], d["sums"][k]), k
    for k in ("SF", "SRF", "SFF"):
        assert got[k].shape[0] == 1 and bits_equal(got[k][0], d["sums"][k]), k
    for Wm, mo in DAILY_CASES:
        want = DR.daily_model(d["sums"], Wm, mo)
        mod = FR.daily_fmodel(got, Wm, mo)
        assert bits_equal(mod["DBETA"][0], want["DBETA"]), (Wm, mo)
        assert bits_equal(mod["DIVOL"], want["DIVOL"]), (Wm, mo)
        assert np.array_equal(mod["NOBS"], want["NOBS"])
        assert (~np.isnan(want["DBETA"])).mean() >= 0.2


# --------------------------------------------------------------------- least squares
def _coef_diff(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


@pytest.mark.parametrize("KF", [2, 3, 4])
def test_monthly_coefficients_vs_lstsq(KF):
    m = _monthly()
    F = FR.seeded_factors(m["MKT"], 31, KF, 0.03, (33, 1))
    worst, cells = 0.0, 0
    for case in CASES:
        Wb = case[0]
        ref = FR.factor_model(m["PM"], F, *case)
        for t in range(Wb - 1, 60, 5 if Wb < 60 else 1):
            for a in range(0, 130, 7):
                if np.isnan(ref["ALPHA"][t, a]):
                    continue
                x, f = FR.window_obs(m["PM"], F, Wb, t, a)
                assert len(x) == ref["NOBS"][t, a] >= case[3]
                A = np.concatenate([f, np.ones((len(x), 1))], axis=1)
                want = np.linalg.lstsq(A, x, rcond=None)[0]
                got = np.append(ref["BETA"][:, t, a], ref["ALPHA"][t, a])
                worst = max(worst, _coef_diff(got, want))
                cells += 1
                e = x - A @ want     # R2 and IVOL from the independent residuals
                r2 = 1.0 - (e @ e) / ((x - x.mean()) @ (x - x.mean()))
                assert abs(ref["R2"][t, a] - r2) <= 1e-9
                iv = np.sqrt((e @ e) / (len(x) - (KF + 1.0)))
                assert abs(ref["IVOL"][t, a] - iv) <= 1e-9 * iv
    print(f"KF={KF}: worst monthly coefficient difference {worst:.3e} over {cells} cells")
    assert cells >= 300 and worst <= LSTSQ_TOL["monthly"]


@pytest.mark.parametrize("KF", [2, 3, 4])
def test_daily_coefficients_vs_lstsq(KF):
    d = _daily()
    FD, sums = _fsums(KF)
    frow = ~np.isnan(FD).any(axis=1)
    worst, cells = 0.0, 0
    for Wm, mo in DAILY_CASES[:3] + [(1, KF + 1)]:
        ref = FR.daily_fmodel(sums, Wm, mo)
        for t in range(Wm - 1, 15):
            lo, hi = int(d["ms"][t - Wm + 1]), int(d["ms"][t + 1])
            for a in range(0, 130, 9):
                if np.isnan(ref["DALPHA"][t, a]):
                    continue
                ok = ~np.isnan(d["R"][lo:hi, a]) & frow[lo:hi]
                y, f = d["R"][lo:hi, a][ok], FD[lo:hi][ok]
                assert len(y) == ref["NOBS"][t, a] >= mo
                A = np.concatenate([f, np.ones((len(y), 1))], axis=1)
                want = np.linalg.lstsq(A, y, rcond=None)[0]
                got = np.append(ref["DBETA"][:, t, a], ref["DALPHA"][t, a])
                worst = max(worst, _coef_diff(got, want))
                cells += 1
                if len(y) >= 15:
                    e = y - A @ want
                    iv = np.sqrt((e @ e) / (len(y) - (KF + 1.0)))
                    assert abs(ref["DIVOL"][t, a] - iv) <= 1e-7 * iv
                    r2 = 1.0 - (e @ e) / ((y - y.mean()) @ (y - y.mean()))
                    assert abs(ref["DR2"][t, a] - r2) <= 1e-7
    print(f"KF={KF}: worst daily coefficient difference {worst:.3e} over {cells} cells")
    assert cells >= 300 and worst <= LSTSQ_TOL["daily"]


# -------------------------------------------------------- collinear pairs and NaN rows
def test_exactly_collinear_pair_defines_nothing():
    m = _monthly()
    F = np.stack([m["MKT"], 2.0 * m["MKT"]], axis=1)
    ref = FR.factor_model(m["PM"], F, 24, 11, 1, 18)
    for k in ("BETA", "ALPHA", "IVOL", "RESMOM", "R2"):
        assert np.isnan(ref[k]).all(), k
    assert np.array_equal(ref["NOBS"], MR.market_model(m["PM"], m["MKT"], 24, 11, 1, 18)["NOBS"])
    d = _daily()
    FD = np.stack([d["MKTD"], 2.0 * d["MKTD"]], axis=1)
    mod = FR.daily_fmodel(FR.daily_fsums(d["R"], FD, d["ms"]), 1, 15)
    for k in ("DBETA", "DALPHA", "DIVOL", "DR2"):
        assert np.isnan(mod[k]).all(), k
    assert (mod["NOBS"] >= 15).mean() >= 0.5


def test_a_nan_in_one_column_removes_the_date_for_every_asset():
    m = _monthly()
    case = (12, 6, 1, 10)
    F = FR.seeded_factors(m["MKT"], 31, 3, 0.03)
    base = FR.factor_model(m["PM"], F, *case)
    F2 = F.copy()
    F2[33, 2] = np.nan
    got = FR.factor_model(m["PM"], F2, *case)
    X = MR.month_returns(m["PM"])
    hit = np.zeros(60, dtype=bool)
    hit[33:45] = True
    lost = ~np.isnan(X[33]) & ~np.isnan(F[33]).any()
    assert lost.sum() >= 60
    assert (got["NOBS"][hit] == base["NOBS"][hit] - lost).all()
    assert np.array_equal(got["NOBS"][~hit], base["NOBS"][~hit])
    assert bits_equal(got["BETA"][:, ~hit], base["BETA"][:, ~hit])
    # the formation months of t = 34 .. 39 hold month 33: no residual momentum there
    assert np.isnan(got["RESMOM"][34:40]).all() and not np.isnan(base["RESMOM"][34:40]).all()
    d = _daily()
    FD, sums = _fsums(3, None)
    FD2, sums2 = _fsums(3, (100, 1))
    t = int(np.searchsorted(d["ms"], 100, side="right") - 1)
    gone = (~np.isnan(d["R"][100]) & ~np.isnan(FD[100]).any()).astype(np.int32)
    assert gone.sum() >= 60 and np.isnan(FD2[100, 1]) and not np.isnan(FD2[100, 0])
    assert np.array_equal(sums["NO"][t] - sums2["NO"][t], gone)
    other = np.arange(15) != t
    for k in FR.FSUMS:
        assert bits_equal(sums[k][..., other, :], sums2[k][..., other, :]), k


def test_an_all_nan_column_defines_nothing():
    m = _monthly()
    F = FR.seeded_factors(m["MKT"], 31, 3, 0.03)
    F[:, 1] = np.nan
    ref = FR.factor_model(m["PM"], F, 12, 6, 1, 10)
    assert (ref["NOBS"] == 0).all()
    for k in ("BETA", "ALPHA", "IVOL", "RESMOM", "R2"):
        assert np.isnan(ref[k]).all(), k
    d = _daily()
    FD = FR.seeded_factors(d["MKTD"], 77, 2, 0.01)
    FD[:, 1] = np.nan
    sums = FR.daily_fsums(d["R"], FD, d["ms"])
    assert all((sums[k] == 0).all() for k in FR.FSUMS)
    mod = FR.daily_fmodel(sums, 1, 15)
    assert (mod["NOBS"] == 0).all() and np.isnan(mod["DBETA"]).all() and np.isnan(mod["DR2"]).all()


def test_smallest_window_interpolates():
    """Wb = n = KF + 1: IVOL is NaN by rule MF5 and the fit passes through every observation."""
    m = _monthly()
    for KF in (1, 2, 3):
        F = FR.seeded_factors(m["MKT"], 31, KF, 0.03)
        ref = FR.factor_model(m["PM"], F, KF + 1, 2, 0, KF + 1)
        assert np.isnan(ref["IVOL"]).all()
        ok = ~np.isnan(ref["ALPHA"])
        assert ok.mean() >= 0.2 and (ref["NOBS"][ok] == KF + 1).all()
        assert np.nanmin(ref["R2"]) >= 1.0 - 1e-6


# ------------------------------------------------------------------------ align_factors
def test_align_factors():
    from csmom.factors import align_factors
    idx = pd.to_datetime(["2000-01-31", "2000-02-29", "2000-03-31", "2000-04-28", "2000-05-31",
                          "2000-06-30"])                    # the panel's business month ends
    days = pd.to_datetime(["2000-03-01", "2000-01-15", "2000-06-30", "2000-02-29", "1999-12-31",
                           "2000-07-31", "2000-05-02"])    # unordered; no April; two extra months
    df = pd.DataFrame({"MKT": np.arange(7.0), "SMB": 10.0 + np.arange(7.0)}, index=days)
    got = align_factors(df, idx)
    assert list(got.columns) == ["MKT", "SMB"] and got.index.equals(idx)
    assert got.to_numpy().dtype == np.float64
    want = np.array([[1.0, 11.0], [3.0, 13.0], [0.0, 10.0], [np.nan, np.nan], [6.0, 16.0],
                     [2.0, 12.0]])
    assert bits_equal(got.to_numpy(), want)
    # a "date" column is the index; an integer column is converted
    df2 = df.reset_index().rename(columns={"index": "date"})
    df2["MKT"] = df2["MKT"].astype(int)
    assert bits_equal(align_factors(df2, idx).to_numpy(), want)
    dup = pd.concat([df, df.iloc[[3]].set_axis(pd.to_datetime(["2000-02-01"]))])
    with pytest.raises(ValueError, match="2000-02"):
        align_factors(dup, idx)
    assert align_factors(df.iloc[:0], idx).isna().all().all()


def test_public_names():
    import csmom
    for name in ("align_factors", "residual_momentum", "FactorModelOut", "DailyFSums",
                 "DailyFModelOut", "ResidualMomentumResult"):
        assert name in csmom.__all__ and hasattr(csmom, name)
    for name in ("factor_model", "daily_fsums", "daily_fmodel", "lagged"):
        assert callable(getattr(csmom.Engine, name))
    import torch
    lag = csmom.Engine.lagged(torch.arange(5, dtype=torch.float64), 2).numpy()
    want = np.array([[0, np.nan, np.nan], [1, 0, np.nan], [2, 1, 0], [3, 2, 1], [4, 3, 2.0]])
    assert bits_equal(lag, want)
