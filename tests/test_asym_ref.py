"""CPU: the NumPy restatement of rules AS1..AS3 (tests/asym_ref.py) against independent
formulations on a dense panel, the restatements of the kernels it shares days with (liq_ref,
dailymkt_ref), hand-built cells for the sign rules, the skip identity, and the ABI table's
csm_asym_sums / csm_asym_model entries.

Bars.  Counts are exact.  DSVOL agrees within 1e-12 relative and RSJ within 1e-12 absolute (it
lies in [-1, 1] and is a difference of two sums: a sum of up to 276 positive terms differs between
summation orders by at most 276 * 2^-53 = 3.1e-14 relative).  DNBETA agrees with np.polyfit on the
side days within 1e-10 relative.  The maxima found are printed.
"""
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

import asym_ref as AR
import dailymkt_ref as DR
import liq_ref as LR
from conftest import bits_equal, max_rel
from oracle.synth_np import make_panel

DENSE = dict(late=0, delist=0, nan_day=0, absent_month=0, nan_month=0)
N = 40


@pytest.fixture(scope="module")
def dense():
    pan = make_panel(N, 782, seed=77, cents=True, with_volume=True, **DENSE)
    P, V, ms = pan["P"], pan["V"], pan["month_start"]
    assert not np.isnan(P).any()
    FD = DR.daily_market(P)["MKTD"]
    assert (FD[1:] < 0).sum() > 200 and (FD[1:] > 0).sum() > 200
    return dict(P=P, V=V, ms=ms, FD=FD, sums=AR.asym_sums(P, ms, FD),
                mon=np.repeat(np.arange(len(ms) - 1), np.diff(ms)))


def test_counts_exact_vs_pandas(dense):
    r = pd.DataFrame(dense["P"]).pct_change()
    f = pd.Series(dense["FD"])
    g = lambda x: x.groupby(dense["mon"]).sum().to_numpy()
    s = dense["sums"]
    assert np.array_equal(s["ND"], g(r.notna()))
    assert np.array_equal(s["NUP"], g(r > 0))
    assert np.array_equal(s["NDN"], g(r < 0))
    assert np.array_equal(s["NB"], g(r.notna().mul(f < 0, axis=0)))
    up = AR.asym_sums(dense["P"], dense["ms"], dense["FD"], side=1)
    assert np.array_equal(up["NB"], g(r.notna().mul(f > 0, axis=0)))
    assert np.array_equal(up["NB"] + s["NB"], g(r.notna().mul(f != 0, axis=0)))
    assert (s["NB"] < s["ND"]).all() and s["NB"].sum() > 5000
    for k in AR.COUNTS + AR.FSUMS:      # the side changes nothing else
        assert bits_equal(up[k], s[k]), k


def test_nd_is_liq_refs_and_zero_returns_close_the_count(dense):
    lq = LR.liq_sums(dense["P"], dense["V"], dense["ms"])
    s = dense["sums"]
    assert np.array_equal(s["ND"], lq["ND"])
    assert np.array_equal(s["NUP"] + s["NDN"] + lq["NZR"], s["ND"])
    assert lq["NZR"].sum() > 0


def _window_rows(dense, t, Wm, skip):
    ms = dense["ms"]
    return int(ms[t - skip - Wm + 1]), int(ms[t - skip + 1])


@pytest.mark.parametrize("Wm,skip", [(1, 0), (12, 0), (6, 2)])
def test_model_vs_masked_sums_and_polyfit(dense, Wm, skip):
    P, FD, R = dense["P"], dense["FD"], dense["sums"]["R"]
    T_m = len(dense["ms"]) - 1
    rng = np.random.default_rng(3)
    M = rng.standard_normal((T_m, N))
    got = AR.asym_model(dense["sums"], Wm, skip, M, min_obs=15 * Wm, min_side=max(2, 5 * Wm))
    want = {k: np.full((T_m, N), np.nan) for k in ("ID", "RSJ", "DSVOL", "DNBETA")}
    for t in range(skip + Wm - 1, T_m):
        a, b = _window_rows(dense, t, Wm, skip)
        r, f = R[a:b], FD[a:b]
        ok = ~np.isnan(r)
        nd = ok.sum(axis=0)
        r0 = np.where(ok, r, 0.0)
        sup = np.sum(np.where(r0 > 0, r0 * r0, 0.0), axis=0)
        sdn = np.sum(np.where(r0 < 0, r0 * r0, 0.0), axis=0)
        en = nd >= 15 * Wm
        with np.errstate(invalid="ignore", divide="ignore"):
            want["RSJ"][t] = np.where(en, (sup - sdn) / (sup + sdn), np.nan)
            want["DSVOL"][t] = np.where(en, np.sqrt(sdn / nd), np.nan)
            share = ((r0 < 0).sum(axis=0) - (r0 > 0).sum(axis=0)) / nd
            want["ID"][t] = np.where(en, np.sign(M[t]) * share, np.nan)
        for c in range(N):
            side = ok[:, c] & (f < 0)
            if side.sum() >= max(2, 5 * Wm):
                want["DNBETA"][t, c] = np.polyfit(f[side], r[side, c], 1)[0]
    for k in want:
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
    ok = ~np.isnan(want["RSJ"])
    e = dict(ID=float(np.abs(got["ID"][ok] - want["ID"][ok]).max()),
             RSJ=float(np.abs(got["RSJ"][ok] - want["RSJ"][ok]).max()),
             DSVOL=max_rel(got["DSVOL"], want["DSVOL"]), DNBETA=max_rel(got["DNBETA"], want["DNBETA"]))
    print(f"Wm={Wm} skip={skip}: " + ", ".join(f"{k} {v:.3e}" for k, v in e.items()))
    assert e["ID"] == 0.0 and e["RSJ"] <= 1e-12 and e["DSVOL"] <= 1e-12 and e["DNBETA"] <= 1e-10
    first = skip + Wm - 1
    assert (~np.isnan(got["RSJ"][first:])).mean() >= 0.5
    assert (~np.isnan(got["DNBETA"][first:])).mean() >= 0.5
    assert np.isnan(got["RSJ"][:first]).all() and (got["NOBS"][:first] == 0).all()
    assert (got["NSIDE"][:first] == 0).all()


def test_all_negative_factor_gives_daily_sums_bits(dense):
    """With every f below zero a side day is an observation of rule V3: the same sums."""
    FD2 = -np.abs(dense["FD"]) - 1e-9            # NaN kept (row 0 of a dense panel has no market)
    assert np.isnan(FD2).sum() >= 1 and (FD2[~np.isnan(FD2)] < 0).all()
    s = AR.asym_sums(dense["P"], dense["ms"], FD2)
    d = DR.daily_sums(s["R"], FD2, dense["ms"])
    assert np.array_equal(s["NB"], d["NO"])
    for a, b in (("BR", "SR"), ("BF", "SF"), ("BFF", "SFF"), ("BRF", "SRF")):
        assert bits_equal(s[a], d[b]), a
    for W in (1, 12):
        m = AR.asym_model(s, W, 0, min_side=15 * W)
        assert bits_equal(m["DNBETA"], DR.daily_model(d, W, 15 * W)["DBETA"])
    up = AR.asym_sums(dense["P"], dense["ms"], -FD2, side=1)
    assert np.array_equal(up["NB"], s["NB"]) and bits_equal(up["BR"], s["BR"])
    assert bits_equal(up["BF"], -s["BF"]) and bits_equal(up["BRF"], -s["BRF"])
    assert bits_equal(up["BFF"], s["BFF"])


@pytest.mark.parametrize("Wm,skip", [(3, 1), (6, 2), (1, 12)])
def test_skip_shifts_the_window(dense, Wm, skip):
    T_m = len(dense["ms"]) - 1
    M = np.random.default_rng(4).standard_normal((T_m, N))
    M0 = np.full_like(M, np.nan)
    M0[:T_m - skip] = M[skip:]                   # M0[t - skip] = M[t]
    a = AR.asym_model(dense["sums"], Wm, skip, M, min_obs=1, min_side=2)
    b = AR.asym_model(dense["sums"], Wm, 0, M0, min_obs=1, min_side=2)
    for k in AR.MODEL:
        assert bits_equal(a[k][skip:], b[k][:T_m - skip]), k
        head = a[k][:Wm + skip - 1]
        assert (head == 0).all() if head.dtype == np.int32 else np.isnan(head).all(), k
    assert not np.isnan(a["ID"][Wm + skip - 1:]).any()


def _hand():
    """Two months of 10 rows (max_gap 3); column 0: +, -, 0 returns; column 1: a gap."""
    ms = np.array([0, 10, 20], dtype=np.int64)
    P = np.full((20, 3), 100.0)
    P[:, 0] = [100, 101, 101, 100, 102, 102, 102, 99, 100, 101,
               101, 100, 99, 98, 97, 97, 98, 96, 95, 94]
    P[2:6, 1] = np.nan                           # rows 1 -> 6: a gap of 5, no return at row 6
    P[6:, 1] = 90.0
    FD = np.array([np.nan, .01, -.01, -.02, .03, 0.0, -.01, -.03, np.nan, .02] * 2)
    return P, ms, FD


def test_hand_cells():
    P, ms, FD = _hand()
    s = AR.asym_sums(P, ms, FD, max_gap=3)
    R = s["R"]
    # column 0, month 0: rows 1..9 have returns: + 0 - + 0 0 - + +
    assert (s["ND"][0, 0], s["NUP"][0, 0], s["NDN"][0, 0]) == (9, 4, 2)
    sup = 0.0
    for d in (1, 4, 8, 9):
        sup = sup + R[d, 0] * R[d, 0]
    assert s["SUP"][0, 0] == sup and s["SDN"][0, 0] == R[3, 0] * R[3, 0] + R[7, 0] * R[7, 0]
    # side days: f < 0 at rows 2, 3, 6, 7 (f == 0 and NaN f are on neither side)
    assert s["NB"][0, 0] == 4 and s["BF"][0, 0] == ((-.01 + -.02) + -.01) + -.03
    assert s["BR"][0, 0] == ((R[2, 0] + R[3, 0]) + R[6, 0]) + R[7, 0]
    up = AR.asym_sums(P, ms, FD, side=1, max_gap=3)
    assert up["NB"][0, 0] == 3                    # rows 1, 4, 9
    # month 1: the first row's return reaches back into month 0; every move but one is down
    assert (s["ND"][1, 0], s["NUP"][1, 0], s["NDN"][1, 0]) == (10, 1, 7)
    # column 1: the gap books no return at row 6, then zeros: ND only
    assert np.isnan(R[6, 1]) and (s["ND"][0, 1], s["NUP"][0, 1], s["NDN"][0, 1]) == (4, 0, 0)
    assert s["SUP"][0, 1] == 0.0 and s["SDN"][0, 1] == 0.0
    # the sign rule of ID: M > 0, M < 0, +0.0, -0.0, NaN
    for m, want in ((2.0, (2 - 4) / 9.0), (-2.0, -((2 - 4) / 9.0)), (0.0, 0.0), (-0.0, 0.0)):
        got = AR.asym_model(s, 1, 0, np.full((2, 3), m), min_obs=1)["ID"][0, 0]
        assert got == want and np.signbit(got) == (want < 0), m      # either zero gives +0.0
    assert np.isnan(AR.asym_model(s, 1, 0, np.full((2, 3), np.nan), min_obs=1)["ID"]).all()
    # no move at all: RSJ undefined, DSVOL 0.0, ID 0 shares
    m = AR.asym_model(s, 1, 0, np.ones((2, 3)), min_obs=1)
    assert np.isnan(m["RSJ"][0, 1]) and m["DSVOL"][0, 1] == 0.0 and m["ID"][0, 1] == 0.0
    assert m["RSJ"][0, 0] == (s["SUP"][0, 0] - s["SDN"][0, 0]) / (s["SUP"][0, 0] + s["SDN"][0, 0])
    # min_obs counts return days, min_side side days
    assert np.isnan(AR.asym_model(s, 1, 0, min_obs=10)["RSJ"][0, 0])
    assert not np.isnan(AR.asym_model(s, 1, 0, min_obs=9)["RSJ"][0, 0])
    assert np.isnan(AR.asym_model(s, 1, 0, min_side=5)["DNBETA"][0, 0])
    assert not np.isnan(AR.asym_model(s, 1, 0, min_side=4)["DNBETA"][0, 0])
    # without FD: no side panels, DNBETA undefined
    bare = AR.asym_sums(P, ms, max_gap=3)
    assert all(bare[k] is None for k in AR.SIDE)
    mb = AR.asym_model(bare, 1, 0, min_obs=1)
    assert np.isnan(mb["DNBETA"]).all() and (mb["NSIDE"] == 0).all()
    assert bits_equal(mb["RSJ"], AR.asym_model(s, 1, 0, min_obs=1)["RSJ"])


def test_names_and_abi():
    from csmom import Engine, _lib
    from csmom.regress import SIGNAL_NAMES
    assert Engine.ASYM_SIGNALS == {"info_disc": "ID", "rsj": "RSJ", "dsvol": "DSVOL",
                                   "dnbeta": "DNBETA"}
    assert set(Engine.ASYM_SIGNALS) < set(Engine.RUN_SIGNALS) < set(SIGNAL_NAMES)
    assert Engine.RUN_SIGNALS[-6:] == ("pkvol", "cs_spread", "ar_spread", "illiq", "dvol", "zret")
    assert Engine.ASYM_OUTPUTS == AR.MODEL
    header = (Path(__file__).resolve().parents[1] / "include" / "csmom.h").read_text()
    for name, nargs in (("csm_asym_sums", 20), ("csm_asym_model", 24)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert f"int {name}(csm_ctx* ctx" in header
