"""CPU: tests/signals_ref.py, the restatement of rules D1..D6 the GPU tests compare against --
a hand-worked panel with every output written out, its PM and D6 against the oracle's month_end
and momentum_scan, and the C boundary of the two new calls."""
import re
from pathlib import Path

import numpy as np

import signals_ref as SR
from conftest import bits_equal
from oracle import csmom_oracle as O
from oracle.synth_np import make_panel

ROOT = Path(__file__).resolve().parents[1]
NAN = np.nan
A = O.absent_scalar()


def _hand_panel():
    """3 assets x 4 months of 3 rows.  Asset 0: a NaN gap across the boundary of months 0 / 1.
    Asset 1: an ABSENT row crossed inside month 0, month 2 wholly ABSENT.  Asset 2: rows without
    a price in month 0, no row in month 1, first priced in month 2."""
    cols = [
        [1, 2, NAN, NAN, 4, 2, 2, 8, 4, 4, 4, 5],
        [10, A, 20, 20, 10, NAN, A, A, A, 5, 10, 10],
        [NAN, NAN, NAN, A, A, A, NAN, 3, 6, 6, 3, A],
    ]
    P = np.ascontiguousarray(np.array(cols, dtype=np.float64).T)
    assert O.is_absent(P).sum() == 8
    return P, np.array([0, 3, 6, 9, 12], dtype=np.int64)


def _eq(got, want):
    return bits_equal(got, np.array(want, dtype=np.float64))


def test_hand_worked_month_stats():
    P, ms = _hand_panel()
    st = SR.month_stats(P, ms)
    assert _eq(st["PM"], [[2, 20, NAN], [2, 10, NAN], [4, NAN, 6], [5, 10, 3]])
    assert np.array_equal(O.is_absent(st["PM"]), [[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 0, 0]])
    assert _eq(st["P1"], [[1, 10, NAN], [4, 20, NAN], [2, NAN, 3], [4, 5, 6]])
    assert _eq(st["HI"], [[2, 20, NAN], [4, 20, NAN], [8, NAN, 6], [5, 10, 6]])
    # asset 0, month 2: (8/2 - 1)^2 + (4/8 - 1)^2; month 3: 0 + (5/4 - 1)^2
    assert _eq(st["SSW"], [[1, 1, 0], [0.25, 0.25, 0], [9.25, 0, 1], [0.0625, 1, 0.25]])
    assert np.array_equal(st["NDW"], [[1, 1, 0], [1, 1, 0], [2, 0, 1], [2, 2, 1]])
    assert st["NDW"].dtype == np.int32


def test_hand_worked_window_signals():
    P, ms = _hand_panel()
    M = np.array([[NAN, NAN, NAN], [0.5, NAN, 1.0], [1.0, 2.0, NAN], [-0.25, 0.5, 1.5]])
    out = SR.signals(P, ms, M=M, Jh=2, Jv=2, min_obs=3)
    # stitches: asset 0 month 1 (4/2 - 1)^2 = 1, months 2 and 3 a zero return; asset 1 month 1
    # zero, month 3 (5/10 - 1)^2 against month 1's price; asset 2 month 3 zero
    assert _eq(out["SS"], [[1, 1, 0], [1.25, 0.25, 0], [9.25, 0, 1], [0.0625, 1.25, 0.25]])
    assert np.array_equal(out["ND"], [[1, 1, 0], [2, 2, 0], [3, 0, 1], [3, 3, 2]])
    assert _eq(out["H52"], [[NAN, NAN, NAN], [0.5, 0.5, NAN], [0.5, NAN, NAN], [0.625, 1.0, 0.5]])
    rv = [[NAN, NAN, NAN],
          [np.sqrt(2.25 / 3), np.sqrt(1.25 / 3), NAN],
          [np.sqrt(10.5 / 5), NAN, NAN],            # asset 1: 2 returns < min_obs
          [np.sqrt(9.3125 / 6), np.sqrt(1.25 / 3), np.sqrt(1.25 / 3)]]
    assert _eq(out["RV"], rv)
    ms_ = [[NAN, NAN, NAN], [0.5 / rv[1][0], NAN, NAN], [1.0 / rv[2][0], NAN, NAN],
           [-0.25 / rv[3][0], 0.5 / rv[3][1], 1.5 / rv[3][2]]]
    assert _eq(out["MS"], ms_)
    assert _eq(out["NR_H52"], [[NAN, NAN, NAN], [1.0, 0.0, NAN], [0.25, NAN, NAN],
                               [NAN, NAN, NAN]])
    assert _eq(out["NR_MS"], [[NAN, NAN, NAN], [1.0, NAN, NAN], [0.25, NAN, NAN],
                              [NAN, NAN, NAN]])


def test_min_obs_defaults_to_ten_per_month_and_m_is_optional():
    P, ms = _hand_panel()
    out = SR.signals(P, ms, Jh=2, Jv=2)
    assert np.isnan(out["RV"]).all() and out["MS"] is None and out["NR_MS"] is None
    assert not np.isnan(out["H52"]).all()


def _gappy():
    pan = make_panel(130, 782, seed=330, late=0.2, delist=0.2, nan_day=0.01, absent_month=0.01,
                     nan_month=0.01, cents=True, with_volume=False)
    return pan["P"], pan["month_start"]


def test_pm_is_the_oracles_month_end():
    P, ms = _gappy()
    PM = SR.month_stats(P, ms)["PM"]
    ref, _ = O.month_end(P, ms)
    assert bits_equal(PM, ref)
    assert np.array_equal(O.is_absent(PM), O.is_absent(ref))
    assert O.is_absent(PM).sum() > 100 and (np.isnan(PM) & ~O.is_absent(PM)).sum() > 10


def test_next_ret_of_momentum_is_the_oracles():
    P, ms = _gappy()
    PM, _ = O.month_end(P, ms)
    for J, skip in ((6, 1), (12, 0)):
        _, M, NR, _ = O.momentum_scan(PM, J, skip)
        assert (~np.isnan(NR)).sum() > 1000
        assert bits_equal(SR.next_ret(PM, M), NR)


def test_h52_is_at_most_one_and_often_one():
    P, ms = _gappy()
    out = SR.signals(P, ms)
    h = out["H52"][~np.isnan(out["H52"])]
    assert len(h) > 0.5 * out["H52"].size and (h <= 1.0).all() and (h > 0.0).all()
    assert (h == 1.0).sum() >= 50
    rv = out["RV"][~np.isnan(out["RV"])]
    assert len(rv) > 0.5 * out["RV"].size and (rv > 0).all()
    assert (out["ND"] >= out["NDW"]).all() and (out["ND"] <= out["NDW"] + 1).all()
    assert (out["SS"] >= out["SSW"]).all()


def test_window_of_one_month_and_zero_length_month():
    P, ms = _gappy()
    ms0 = np.concatenate([ms[:5], ms[4:]])   # month 4 has no day
    st = SR.month_stats(P, ms0)
    assert O.is_absent(st["PM"][4]).all() and np.isnan(st["HI"][4]).all()
    assert (st["SSW"][4] == 0).all() and (st["NDW"][4] == 0).all()
    ref, _ = O.month_end(P, ms0)
    assert bits_equal(st["PM"], ref)
    out = SR.window_signals(**st, Jh=1, Jv=1, min_obs=1)
    ok = ~np.isnan(out["H52"])
    assert bits_equal(out["H52"][ok], st["PM"][ok] / st["HI"][ok])
    assert np.array_equal(ok, ~np.isnan(st["PM"]))


def test_c_boundary_declares_both_calls():
    from csmom import _lib
    hdr = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "csmom.h").read_text(), flags=re.S)
    want = {"csm_month_stats": 12, "csm_window_signals": 19}
    for name, n in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/csmom.h"
        assert len(m.group(1).split(",")) == n
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n
    assert "#define CSM_ABI_VERSION 3" in (ROOT / "include" / "csmom.h").read_text()
