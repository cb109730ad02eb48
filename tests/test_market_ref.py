"""CPU: tests/market_ref.py, the restatement of rules B1..B6 the GPU tests compare against --
its month return against the oracle's on dense and gappy panels, its market model against
np.linalg.lstsq, the properties the rules imply, and the C boundary of the three new calls."""
import re
from pathlib import Path

import numpy as np
import pytest

import market_ref as MR
from conftest import bits_equal
from oracle import csmom_oracle as O

ROOT = Path(__file__).resolve().parents[1]
# four times the worst relative difference measured in test_market_model_vs_lstsq (its docstring)
TOL = dict(BETA=4 * 1.842e-12, IVOL=4 * 1.732e-13, RESMOM=4 * 8.910e-11)
_REF = {}


def _dense():
    """The dense panel's PM, x, market and per-case market model, computed once."""
    if not _REF:
        PM = MR.panel(65, "dense")["PM"]
        mf = MR.market_factor(PM)
        _REF.update(PM=PM, X=mf["X"], F=mf["MKT"], NMK=mf["NMK"], mm={})
    return _REF


def _model(case):
    d = _dense()
    if case not in d["mm"]:
        d["mm"][case] = MR.market_model(d["PM"], d["F"], *case)
    return d["mm"][case]


def _rel(got, want):
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~ok)
    return float(np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok]))) if ok.any() else 0.0


def test_dense_month_return_is_the_scans():
    d = _dense()
    R = O.momentum_scan(d["PM"], 12, 1)[0]
    assert not np.isnan(d["PM"]).any()
    assert bits_equal(d["X"], R)
    assert np.isnan(d["X"][0]).all() and not np.isnan(d["X"][1:]).any()
    assert (d["NMK"][1:] == 65).all() and d["NMK"][0] == 0 and np.isnan(d["F"][0])


def test_gappy_month_return_does_not_fill_gaps():
    PM = MR.panel(130, "gappy")["PM"]
    X = MR.month_returns(PM)
    R = O.momentum_scan(PM, 12, 1)[0]
    nx, nr = np.isnan(X), np.isnan(R)
    assert not np.array_equal(nx, nr)
    assert (nx & ~nr).sum() >= 50          # returns the scan carries over a gap
    both = ~nx & ~nr & ~np.isnan(np.vstack([PM[:1], PM[:-1]]))
    assert bits_equal(X[both], R[both])    # where the months are adjacent: the same quotient
    mf = MR.market_factor(PM, min_assets=60)
    assert np.array_equal(mf["NMK"], (~nx).sum(axis=1))
    assert np.isnan(mf["MKT"][mf["NMK"] < 60]).all() and (mf["NMK"] < 60).sum() >= 1
    assert not np.isnan(mf["MKT"][mf["NMK"] >= 60]).any()


@pytest.mark.parametrize("case", MR.CASES)
def test_market_model_vs_lstsq(case):
    """Every fully observed window of the dense panel (N = 65) against np.linalg.lstsq: beta,
    IVOL, and RESMOM as sum(e) / std(e, ddof=1) over the formation slice.  The two sides differ by
    conditioning only.  Worst relative differences measured over the five cases: beta 1.842e-12
    (Wb = 36), IVOL 1.732e-13 and RESMOM 8.910e-11 (both at Wb = 3, where two or three residuals of
    1e-3 are what is left of returns of 1e-1); the test holds four times each."""
    Wb, J, skip, _ = case
    d = _dense()
    ref = _model(case)
    X, F = d["X"], d["F"]
    worst = dict(BETA=0.0, IVOL=0.0, RESMOM=0.0)
    windows = 0
    for t in range(Wb, 60):   # window t-Wb+1 .. t without month 0, whose x is NaN
        w = slice(t - Wb + 1, t + 1)
        A = np.stack([np.ones(Wb), F[w]], axis=1)
        coef = np.linalg.lstsq(A, X[w], rcond=None)[0]
        E = X[w] - A @ coef
        fs = E[Wb - skip - J:Wb - skip]
        want = dict(BETA=coef[1], RESMOM=fs.sum(axis=0) / fs.std(axis=0, ddof=1))
        if Wb >= 3:
            want["IVOL"] = np.sqrt((E * E).sum(axis=0) / (Wb - 2))
        for k, v in want.items():
            assert not np.isnan(ref[k][t]).any(), (k, t)
            worst[k] = max(worst[k], _rel(v, ref[k][t]))
        assert (ref["NOBS"][t] == Wb).all()
        windows += 1
    print(case, windows, worst)
    assert windows == 60 - Wb
    for k in worst:
        assert worst[k] <= TOL[k], (k, worst[k])
    # the window that holds month 0 has Wb - 1 observations; before it nothing is defined
    assert (ref["NOBS"][:Wb - 1] == 0).all() and np.isnan(ref["BETA"][:Wb - 1]).all()
    if Wb < 60:
        assert (ref["NOBS"][Wb - 1] == Wb - 1).all()


def test_affine_factor_scales_beta():
    case = (24, 11, 1, 18)
    d = _dense()
    ref = _model(case)
    c, dd = 2.5, 0.01
    F2 = c * d["F"] + dd
    got = MR.market_model(d["PM"], F2, *case)
    assert _rel(got["BETA"] * c, ref["BETA"]) <= TOL["BETA"]
    assert _rel(got["IVOL"], ref["IVOL"]) <= TOL["IVOL"]
    assert np.array_equal(got["NOBS"], ref["NOBS"])


def test_asset_that_is_the_factor():
    """An asset whose x equals the factor: dx = df bit for bit, so sfx = sff and BETA is exactly
    1; ALPHA = mx - 1 * mf = 0, every residual is exactly 0, sv = 0, and RESMOM is NaN by the
    rule's sv > 0.  IVOL is 0."""
    case = (12, 6, 1, 10)
    d = _dense()
    PM = d["PM"].copy()
    F = d["X"][:, 0].copy()          # the factor is asset 0's own return
    got = MR.market_model(PM, F, *case)
    t = slice(12, 60)
    assert (got["BETA"][t, 0] == 1.0).all() and (got["ALPHA"][t, 0] == 0.0).all()
    assert (got["IVOL"][t, 0] == 0.0).all() and np.isnan(got["RESMOM"][t, 0]).all()
    assert not np.isnan(got["RESMOM"][t, 1:]).any()


def test_nan_in_the_factor_removes_the_month():
    case = (12, 6, 1, 10)
    d = _dense()
    ref = _model(case)
    F = d["F"].copy()
    F[30] = np.nan
    got = MR.market_model(d["PM"], F, *case)
    hit = np.zeros(60, dtype=bool)
    hit[30:42] = True                                  # windows t-11 .. t that hold month 30
    full = np.arange(60) >= 12
    assert (got["NOBS"][hit] == 11).all() and (got["NOBS"][full & ~hit] == 12).all()
    for k in ("BETA", "ALPHA", "IVOL", "RESMOM"):
        assert bits_equal(got[k][~hit], ref[k][~hit]), k
    assert not np.isnan(got["BETA"][hit]).any()        # 11 >= min_obs
    form = (np.arange(60) - 1 >= 30) & (np.arange(60) - 6 <= 30)   # formation t-6 .. t-1
    assert np.isnan(got["RESMOM"][form]).all() and not np.isnan(got["RESMOM"][hit & ~form]).any()
    F[31] = np.nan                                     # two gone: 10 observations still do
    assert not np.isnan(MR.market_model(d["PM"], F, *case)["BETA"][31:42]).any()
    F[32] = np.nan                                     # three gone: below min_obs
    assert np.isnan(MR.market_model(d["PM"], F, *case)["BETA"][32:42]).all()


def test_next_ret_is_rule_d6():
    PM = MR.panel(130, "gappy")["PM"]
    _, M, NR, _ = O.momentum_scan(PM, 6, 1)
    assert bits_equal(MR.next_ret(PM, M), NR) and (~np.isnan(NR)).sum() > 1000


def test_c_boundary_declares_the_three_calls():
    from csmom import _lib
    hdr = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "csmom.h").read_text(), flags=re.S)
    want = {"csm_market_factor": 8, "csm_market_model": 14, "csm_next_ret": 6}
    for name, n in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/csmom.h"
        assert len(m.group(1).split(",")) == n
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n
    assert "#define CSM_ABI_VERSION 3" in (ROOT / "include" / "csmom.h").read_text()
