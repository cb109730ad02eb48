"""CPU: the NumPy restatement of rules Q1..Q3 (tests/liq_ref.py) against an independent pandas
expression on a dense panel, hand-built cells for each branch of the rules, and the ABI table's
csm_liq_sums / csm_liq_model entries.

Bars.  Counts are exact.  ILLIQ, DVOL, TURN and ZRET agree within 1e-12 relative at Wm 1 and 12: a
sum of up to 276 positive terms differs between summation orders by at most 276 * 2^-53 = 3.1e-14
relative, and the quotients add a few roundings.  The maximum found is printed (DESIGN.md 7 records
it).
"""
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

import liq_ref as LR
from conftest import max_rel
from oracle import csmom_oracle as O
from oracle.synth_np import make_panel

DENSE = dict(late=0, delist=0, nan_day=0, absent_month=0, nan_month=0)
REL = 1e-12


@pytest.fixture(scope="module")
def dense():
    pan = make_panel(40, 782, seed=77, cents=True, with_volume=True, **DENSE)
    P, V, ms = pan["P"], pan["V"].copy(), pan["month_start"]
    assert not np.isnan(P).any() and (V > 0).all()
    rng = np.random.default_rng(5)
    V[rng.random(V.shape) < 0.05] = 0.0          # zero-volume days: priced, not Amihud days
    SH = np.round(rng.lognormal(17.0, 1.0, (len(ms) - 1, 40)))
    return dict(P=P, V=V, ms=ms, SH=SH, sums=LR.liq_sums(P, V, ms))


def _pandas_months(d):
    """Month sums and counts by groupby(month) of the frames' own expressions."""
    P, V = pd.DataFrame(d["P"]), pd.DataFrame(d["V"])
    mon = np.repeat(np.arange(len(d["ms"]) - 1), np.diff(d["ms"]))
    r = P.pct_change()
    dv = P * V
    il = (r.abs() / dv).where(dv > 0)
    g = lambda f: f.groupby(mon)
    return dict(il_sum=g(il).sum(), il_mean=g(il).mean(), NA=g(il).count(), ND=g(r).count(),
                NP=g(P).count(), NZR=g(r == 0).sum(), NZV=g(V == 0).sum(),
                SDV=g(dv).sum(), dv_mean=g(dv).mean(), SV=g(V).sum(), v_mean=g(V).mean())


def test_counts_exact_vs_pandas(dense):
    m = _pandas_months(dense)
    for k in LR.COUNTS:
        assert np.array_equal(dense["sums"][k], m[k].to_numpy()), k
    assert dense["sums"]["NZV"].sum() > 1000 and dense["sums"]["NZR"].sum() > 0
    assert (dense["sums"]["NA"] < dense["sums"]["ND"]).any()


@pytest.mark.parametrize("Wm", [1, 12])
def test_model_vs_pandas(dense, Wm):
    m = _pandas_months(dense)
    SH = dense["SH"]
    mo = 15 * Wm
    got = LR.liq_model(dense["sums"], Wm, None, 1e6, SH)
    roll = lambda f: f.rolling(Wm).sum()
    na, npd, nd = roll(m["NA"]), roll(m["NP"]), roll(m["ND"])
    if Wm == 1:   # the month's own .mean()
        illiq, dvol, adv = m["il_mean"] * 1e6, m["dv_mean"], m["v_mean"]
    else:
        illiq, dvol, adv = roll(m["il_sum"]) / na * 1e6, roll(m["SDV"]) / npd, roll(m["SV"]) / npd
    want = dict(ILLIQ=illiq.where(na >= mo), DVOL=dvol.where(npd >= mo),
                TURN=(adv / SH).where(npd >= mo), ZRET=(roll(m["NZR"]) / nd).where(nd >= mo),
                ZVOL=(roll(m["NZV"]) / npd).where(npd >= mo))
    worst = 0.0
    for k, w in want.items():
        w = w.to_numpy(dtype=np.float64)
        assert np.array_equal(np.isnan(got[k]), np.isnan(w)), k
        e = max_rel(got[k], w)
        print(f"Wm={Wm} {k}: max relative difference {e:.3e}")
        worst = max(worst, e)
        assert e <= REL, k
    assert np.array_equal(got["NOBS"][Wm - 1:], na.to_numpy()[Wm - 1:].astype(np.int32))
    assert (got["NOBS"][:Wm - 1] == 0).all()
    assert (~np.isnan(got["ILLIQ"][Wm - 1:])).mean() >= 0.5
    print(f"Wm={Wm}: max relative difference over the outputs {worst:.3e}")


def _hand():
    """Three months of 20 rows, one column per case (max_gap 3)."""
    T, N = 60, 8
    ms = np.array([0, 20, 40, 60], dtype=np.int64)
    P = np.tile((50.0 + 0.5 * np.arange(T))[:, None], (1, N))
    V = np.full((T, N), 1000.0)
    V[5, 0] = 0.0                     # 0: a zero-volume day
    V[6, 1] = np.nan                  # 1: a NaN volume
    P[7, 2] = np.nan                  # 2: volume on an unpriced day
    V[7, 2] = 123456.0
    P[8:12, 3] = P[8, 3]              # 3: a constant-price run, three zero returns
    V[20:40, 4] = 0.0                 # 4: a month of all-zero volume
    P[3:5, 5] = np.nan                # 5: gaps d - d' of 3 (rows 2 -> 5: booked) ...
    P[6:9, 5] = O.absent_scalar()     #    ... of 4 (rows 5 -> 9: refused) and of 2 (9 -> 11)
    P[10, 5] = np.nan
    return P, V, ms


def test_hand_cells():
    P, V, ms = _hand()
    s = LR.liq_sums(P, V, ms, max_gap=3)
    full = dict(NP=20, ND=19, NA=19, NZR=0, NZV=0)     # month 0 of an untouched column
    for k, v in full.items():
        assert s[k][0, 7] == v and s[k][1, 7] == (20 if k in ("NP", "ND", "NA") else 0), k
    # a zero-volume day and a NaN volume: priced days, no Amihud days, nothing added to SV
    for c in (0, 1):
        assert (s["NP"][0, c], s["ND"][0, c], s["NA"][0, c], s["NZV"][0, c]) == (20, 19, 18, 1)
        assert s["SV"][0, c] == 19 * 1000.0 and s["SIL"][0, c] < s["SIL"][0, 7]
    # volume on an unpriced day is ignored; the next day's return reaches over it
    assert (s["NP"][0, 2], s["ND"][0, 2], s["NA"][0, 2], s["NZV"][0, 2]) == (19, 18, 18, 0)
    assert s["SV"][0, 2] == 19 * 1000.0
    sdv = 0.0
    for d in range(20):
        sdv = sdv + P[d, 2] * 1000.0 if d != 7 else sdv
    assert s["SDV"][0, 2] == sdv
    assert s["R"][8, 2] == P[8, 2] / P[6, 2] - 1.0
    # a constant-price run
    assert s["NZR"][0, 3] == 3 and s["ND"][0, 3] == 19 and s["NA"][0, 3] == 19
    # a month of all-zero volume
    assert (s["NP"][1, 4], s["ND"][1, 4], s["NA"][1, 4], s["NZV"][1, 4]) == (20, 20, 0, 20)
    assert s["SDV"][1, 4] == 0.0 and s["SIL"][1, 4] == 0.0
    m = LR.liq_model(s, 1, 1)
    assert np.isnan(m["ILLIQ"][1, 4]) and m["DVOL"][1, 4] == 0.0 and m["ZVOL"][1, 4] == 1.0
    assert m["NOBS"][1, 4] == 0 and not np.isnan(m["ILLIQ"][0, 4])
    # gaps one under, at and one over max_gap = 3
    r = s["R"][:, 5]
    assert not np.isnan(r[5]) and r[5] == P[5, 5] / P[2, 5] - 1.0       # d - d' = 3: at
    assert np.isnan(r[9])                                               # 4: over
    assert not np.isnan(r[11]) and r[11] == P[11, 5] / P[9, 5] - 1.0    # 2: under
    assert s["NP"][0, 5] == 20 - 6 and s["ND"][0, 5] == 20 - 6 - 2 and s["NA"][0, 5] == 12
    # the window adds months oldest first and NOBS is 0 before a whole window
    m3 = LR.liq_model(s, 3, 1)
    assert (m3["NOBS"][:2] == 0).all() and np.isnan(m3["DVOL"][:2]).all()
    assert m3["NOBS"][2, 7] == 59 and m3["NOBS"][2, 4] == 39
    sil = (s["SIL"][0, 7] + s["SIL"][1, 7]) + s["SIL"][2, 7]
    assert m3["ILLIQ"][2, 7] == (sil / 59.0) * 1e6


def test_shares_zero_or_nan_leave_turn_undefined():
    P, V, ms = _hand()
    s = LR.liq_sums(P, V, ms, max_gap=3)
    SH = np.full((3, 8), 5e6)
    SH[0, 0] = 0.0
    SH[1, 1] = np.nan
    SH[2, 2] = -1.0
    m = LR.liq_model(s, 1, 1, SH=SH)
    assert np.isnan(m["TURN"][0, 0]) and np.isnan(m["TURN"][1, 1]) and np.isnan(m["TURN"][2, 2])
    assert np.isnan(m["TURN"]).sum() == 3
    assert m["TURN"][0, 7] == (20 * 1000.0 / 20.0) / 5e6
    assert np.isnan(LR.liq_model(s, 1, 1)["TURN"]).all()


def test_min_obs_counts_days():
    P, V, ms = _hand()
    s = LR.liq_sums(P, V, ms, max_gap=3)
    m = LR.liq_model(s, 1, 19)
    assert not np.isnan(m["ILLIQ"][0, 7]) and np.isnan(m["ILLIQ"][0, 0])   # 19 and 18 Amihud days
    m = LR.liq_model(s, 1, 20)
    assert not np.isnan(m["DVOL"][0, 0]) and np.isnan(m["DVOL"][0, 2])     # 20 and 19 priced days
    assert np.isnan(LR.liq_model(s, 1)["ILLIQ"][0, 5])                     # default 15 > 12


def test_abi_table_and_header_carry_the_calls():
    from csmom import _lib
    header = (Path(__file__).resolve().parents[1] / "include" / "csmom.h").read_text()
    for name, nargs in (("csm_liq_sums", 17), ("csm_liq_model", 21)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert f"int {name}(csm_ctx* ctx" in header
