"""CPU: tests/xsreg_ref.py, the restatement of rules R1..R6 the GPU tests compare against -- its
monthly regressions against np.linalg.lstsq (OLS, and WLS through sqrt(w) scaling), its
standardised ridge against the normal-equation closed form on StandardScaler-ed columns, its R2
against the directly computed one, its Newey-West numbers against a direct evaluation of R6's
formula, the properties the rules imply, and the C boundary of the two new calls.  This checks the
rules, not the kernel.

Bars: four times the worst difference measured on these panels (market_ref.panel(N, "gappy"),
60 months, regressors mom_12,1, BETA and IVOL at case (24, 11, 1, 18), Y the momentum ranking's
next return).  A coefficient difference is scaled by the larger of the other side's coefficient
and 1e-3.  Measured:
  OLS vs lstsq          3.250e-13 (N = 5), at most 8.809e-14 at N = 63, 257, 2049
  WLS vs lstsq          1.900e-12 (N = 5, 22 months), at most 5.052e-14 at N = 63, 257, 2049
  standardised ridge    1.010e-14 (ridge 0, N = 257) and 9.216e-15 (ridge 5.0) against the closed
                        form, scaled the same way
  R2                    6.772e-15 (N = 5), at most 5.551e-16 at N >= 63, absolute
  Newey-West            8.04e-16 relative over MEAN, SE and T at lags 0, 1 and 4
"""
import math
import re
from pathlib import Path

import numpy as np
import pytest

import xsreg_ref as XR
from conftest import bits_equal

ROOT = Path(__file__).resolve().parents[1]
SIZES = (5, 63, 257, 2049)
TOL = dict(OLS=4 * 3.250e-13, WLS=4 * 1.900e-12, RIDGE=4 * 1.010e-14, R2=4 * 6.772e-15,
           NW=4 * 8.04e-16)
_REF = {}


def _ols(N):
    if N not in _REF:
        d = XR.real_inputs(N)
        _REF[N] = XR.xs_regress(d["Y"], d["S"])
    return _REF[N]


def _weights(N):
    """Seeded positive weights with NaN, zero and negative cells."""
    rng = np.random.default_rng(900 + N)
    W = rng.uniform(0.5, 2.0, size=(60, N))
    r = rng.random((60, N))
    W[r < 0.03] = np.nan
    W[(r >= 0.03) & (r < 0.06)] = 0.0
    W[(r >= 0.06) & (r < 0.09)] = -1.0
    return W


def _design(d, t, W=None):
    """The month's observations: (obs mask, A = [1, S], y, w)."""
    obs = ~np.isnan(d["Y"][t])
    for s in d["S"]:
        obs &= ~np.isnan(s[t])
    if W is not None:
        obs &= ~np.isnan(W[t]) & (W[t] > 0.0)
    A = np.stack([np.ones(int(obs.sum()))] + [s[t][obs] for s in d["S"]], axis=1)
    return obs, A, d["Y"][t][obs], (None if W is None else W[t][obs])


def _scaled(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-3)))


def test_months_defined_on_the_real_signals():
    """The coverage the GPU tests rely on: at least half the months are defined."""
    for N, want in ((1, 0), (5, 35), (63, 36), (64, 36), (65, 36), (257, 36), (2048, 36),
                    (2049, 36), (4500, 36)):
        d = XR.real_inputs(N)
        r = XR.xs_regress(d["Y"], d["S"])
        defined = ~np.isnan(r["GAMMA"][:, 0])
        assert int(defined.sum()) == want, (N, int(defined.sum()))
        assert np.array_equal(defined, ~np.isnan(r["GAMMA"]).any(axis=1))
        assert np.array_equal(defined, ~np.isnan(r["R2"]))
    w = XR.wide_inputs()
    r = XR.xs_regress(w["Y"], w["S"])
    assert int((~np.isnan(r["GAMMA"][:, 0])).sum()) == 9 and w["Y"].shape == (14, 20001)


@pytest.mark.parametrize("N", SIZES)
def test_ols_and_r2_vs_lstsq(N):
    d = XR.real_inputs(N)
    r = _ols(N)
    worst = worst_r2 = 0.0
    months = 0
    for t in range(60):
        obs, A, y, _ = _design(d, t)
        assert r["NOBS"][t] == obs.sum()
        if np.isnan(r["GAMMA"][t, 0]):
            continue
        coef = np.linalg.lstsq(A, y, rcond=None)[0]
        worst = max(worst, _scaled(r["GAMMA"][t], coef))
        e = y - A @ coef
        dy = y - y.mean()
        worst_r2 = max(worst_r2, abs(r["R2"][t] - (1.0 - (e @ e) / (dy @ dy))))
        months += 1
    print(f"OLS N={N}: {months} months, gamma {worst:.3e}, R2 {worst_r2:.3e}")
    assert months >= 30
    assert worst <= TOL["OLS"] and worst_r2 <= TOL["R2"]


@pytest.mark.parametrize("N", SIZES)
def test_wls_vs_lstsq(N):
    d = XR.real_inputs(N)
    W = _weights(N)
    r = XR.xs_regress(d["Y"], d["S"], W=W)
    worst = 0.0
    months = 0
    for t in range(60):
        obs, A, y, w = _design(d, t, W)
        assert r["NOBS"][t] == obs.sum()
        if np.isnan(r["GAMMA"][t, 0]):
            continue
        rt = np.sqrt(w)
        coef = np.linalg.lstsq(A * rt[:, None], y * rt, rcond=None)[0]
        worst = max(worst, _scaled(r["GAMMA"][t], coef))
        months += 1
    print(f"WLS N={N}: {months} months, gamma {worst:.3e}")
    assert months >= (20 if N == 5 else 30)
    assert (r["NOBS"] <= _ols(N)["NOBS"]).all() and (r["NOBS"] < _ols(N)["NOBS"]).any()
    assert worst <= TOL["WLS"]
    # unit weights are no weights
    ones = XR.xs_regress(d["Y"], d["S"], W=np.ones((60, N)))
    for k in ("GAMMA", "R2"):
        assert bits_equal(ones[k], _ols(N)[k])


@pytest.mark.parametrize("N", SIZES[1:])
@pytest.mark.parametrize("ridge", [0.0, 5.0])
def test_standardised_ridge_vs_closed_form(N, ridge):
    """StandardScaler + Ridge(alpha) on the month's cross-section: z-scores with the population
    deviation, (Z'Z + alpha I) beta = Z'(y - mean y), intercept mean y."""
    d = XR.real_inputs(N)
    r = XR.xs_regress(d["Y"], d["S"], standardize=True, ridge=ridge)
    worst = 0.0
    months = 0
    for t in range(60):
        if np.isnan(r["GAMMA"][t, 0]):
            continue
        _, A, y, _ = _design(d, t)
        X = A[:, 1:]
        Z = (X - X.mean(axis=0)) / X.std(axis=0)
        beta = np.linalg.solve(Z.T @ Z + ridge * np.eye(3), Z.T @ (y - y.mean()))
        worst = max(worst, _scaled(r["GAMMA"][t], np.concatenate([[y.mean()], beta])))
        assert r["GAMMA"][t, 0] == r["MY"][t]
        months += 1
    print(f"ridge={ridge} N={N}: {months} months, gamma {worst:.3e}")
    assert months >= 30 and worst <= TOL["RIDGE"]
    if ridge > 0.0:   # shrinkage: the fit can only lose R2
        assert (r["R2"][~np.isnan(r["R2"])] <= XR.xs_regress(
            d["Y"], d["S"], standardize=True)["R2"][~np.isnan(r["R2"])] + 1e-12).all()


def test_standardising_leaves_the_ols_fit():
    d = XR.real_inputs(257)
    z = XR.xs_regress(d["Y"], d["S"], standardize=True)
    ok = ~np.isnan(z["R2"])
    assert np.array_equal(ok, ~np.isnan(_ols(257)["R2"]))
    assert np.max(np.abs(z["R2"][ok] - _ols(257)["R2"][ok])) <= 1e-12


def test_min_obs_and_degenerate_regressors():
    d = XR.real_inputs(5)
    full = _ols(5)
    r = XR.xs_regress(d["Y"], d["S"], min_obs=5)
    defined = ~np.isnan(r["GAMMA"][:, 0])
    assert np.array_equal(defined, ~np.isnan(full["GAMMA"][:, 0]) & (full["NOBS"] == 5))
    assert defined.sum() >= 5 and (full["NOBS"] < 5).sum() >= 5
    assert np.array_equal(r["NOBS"], full["NOBS"])
    assert bits_equal(r["GAMMA"][defined], full["GAMMA"][defined])
    # a constant regressor in one month: that month is undefined, the others are untouched
    d = XR.real_inputs(257)
    S = [s.copy() for s in d["S"]]
    S[1][40] = np.where(np.isnan(S[1][40]), np.nan, 0.25)
    r = XR.xs_regress(d["Y"], S)
    base = _ols(257)
    assert np.isnan(r["GAMMA"][40]).all() and not np.isnan(base["GAMMA"][40]).any()
    keep = np.arange(60) != 40
    assert bits_equal(r["GAMMA"][keep], base["GAMMA"][keep])
    assert r["NOBS"][40] == base["NOBS"][40]
    # a regressor twice, and an affine copy of one: the pivot rule leaves nothing
    for extra in (d["S"][0], 2.0 * d["S"][0] + 1.0):
        r = XR.xs_regress(d["Y"], d["S"] + [extra])
        assert np.isnan(r["GAMMA"]).all() and np.isnan(r["R2"]).all()
        assert np.array_equal(r["NOBS"], base["NOBS"])
    # enough ridge makes the copy solvable again
    r = XR.xs_regress(d["Y"], d["S"] + [d["S"][0]], standardize=True, ridge=5.0)
    assert (~np.isnan(r["GAMMA"][:, 0])).sum() == 36


def test_r1_sum_is_a_sum():
    """R1 against math.fsum within the bound of any order, and its reshape: one asset in the second
    slice is added last."""
    rng = np.random.default_rng(3)
    for N in (1, 63, 64, 65, 257, 2048, 2049, 4500):
        v = rng.normal(size=N)
        exact = math.fsum(v)
        assert abs(XR.r1_sum(v) - exact) <= 2.0 ** -53 * N * math.fsum(np.abs(v))
    v = rng.normal(size=2049)
    assert XR.r1_sum(v) == XR.r1_sum(v[:2048]) + v[2048]
    # lanes 256 apart are added first: assets 0 and 256 meet before asset 1 joins
    v = np.zeros(512)
    v[0], v[256], v[1] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert XR.r1_sum(v) == 1.0 and (1.0 + (v[256] + v[1])) > 1.0


def _nw_direct(x, L):
    x = x[~np.isnan(x)]
    n = len(x)
    u = x - x.mean()
    var = (u @ u) / n
    for l in range(1, L + 1):
        var += 2.0 * (1.0 - l / (L + 1.0)) * (u[l:] @ u[:-l]) / n
    se = math.sqrt(var / n)
    return x.mean(), se, x.mean() / se, n


@pytest.mark.parametrize("lags", [0, 1, 4])
def test_newey_west_vs_the_formula(lags):
    rng = np.random.default_rng(21)
    G = rng.normal(0.01, 0.05, size=(60, 5))
    for t in range(1, 60):
        G[t] += 0.4 * (G[t - 1] - 0.01)           # serial correlation for the lags to see
    G[[3, 17, 18, 44]] = np.nan
    G[:, 2] = np.nan
    keep = [0, 1, 2, 5, 6][:lags + 1]             # n = lags + 1: a mean and nothing else
    col = np.full(60, np.nan)
    col[keep] = G[keep, 4]
    G[:, 4] = col
    nw = XR.newey_west(G, lags)
    worst = 0.0
    for c in (0, 1, 3):
        mean, se, ts, n = _nw_direct(G[:, c], lags)
        assert nw["NT"][c] == n == 56
        for got, want in ((nw["MEAN"][c], mean), (nw["SE"][c], se), (nw["T"][c], ts)):
            worst = max(worst, abs(got - want) / abs(want))
    print(f"lags={lags}: worst relative difference {worst:.2e}")
    assert worst <= TOL["NW"]
    assert nw["NT"][2] == 0 and all(np.isnan(nw[k][2]) for k in ("MEAN", "SE", "T"))
    n4 = int((~np.isnan(G[:, 4])).sum())
    assert n4 == nw["NT"][4] == lags + 1
    assert not np.isnan(nw["MEAN"][4]) and np.isnan(nw["SE"][4]) and np.isnan(nw["T"][4])
    one = XR.newey_west(G[:, 0], lags)
    assert one["MEAN"] == nw["MEAN"][0] and one["T"] == nw["T"][0] and one["NT"] == 56
    if lags == 0:      # no lag: the plain standard error with the 1 / n variance
        x = G[:, 0][~np.isnan(G[:, 0])]
        assert abs(nw["SE"][0] - x.std() / math.sqrt(56)) <= 1e-15


def test_default_lags():
    assert [XR.default_lags(T) for T in (14, 60, 100, 300, 461)] == [2, 3, 4, 5, 5]


def test_fama_macbeth_chains_the_two():
    d = XR.real_inputs(63)
    fm = XR.fama_macbeth(d["Y"], d["S"])
    r = XR.xs_regress(d["Y"], d["S"], standardize=True)
    assert fm["lags"] == 3 and bits_equal(fm["GAMMA"], r["GAMMA"])
    nw = XR.newey_west(r["GAMMA"], 3)
    for k in ("MEAN", "SE", "T"):
        assert bits_equal(fm["nw"][k], nw[k]) and not np.isnan(nw[k]).any()
    assert (nw["NT"] == 36).all() and fm["R2_MEAN"] == XR.newey_west(r["R2"], 3)["MEAN"]


def test_c_boundary_declares_the_two_calls():
    from csmom import _lib
    hdr = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "csmom.h").read_text(), flags=re.S)
    for name, n in {"csm_xs_regress": 13, "csm_newey_west": 10}.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/csmom.h"
        assert len(m.group(1).split(",")) == n
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n
    import csmom
    for name in ("XsRegressOut", "NeweyWestOut", "FamaMacBethOut", "FamaMacBethResult",
                 "fama_macbeth"):
        assert name in csmom.__all__ and hasattr(csmom, name)
    for name in ("xs_regress", "newey_west", "fama_macbeth"):
        assert hasattr(csmom.Engine, name)
