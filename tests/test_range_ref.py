"""CPU: tests/range_ref.py, the restatement of rules HL1..HL6 the GPU tests compare
against, pinned to hand cells, to a second evaluation straight from the papers' expressions and to
a simulated path; panel.range_from_long on a hand-built frame; the names the feature declares.

Bar for values that two evaluations give (ratio form log(H / L) against h - l): 1e-10 of the
reference's scale for that sum, the bar tests/test_gpu_range.py holds the device to.
"""
import math

import numpy as np
import pandas as pd
import pytest

import dailymkt_ref as DR
import range_ref as RR
from oracle import csmom_oracle as O

BAR = 1e-10
K = 3.0 - 2.0 * math.sqrt(2.0)


def _cols(*rows):
    """(H, L, C) [T_d][1] from rows of (H, L, C)."""
    a = np.array(rows, dtype=np.float64)
    return a[:, 0:1].copy(), a[:, 1:2].copy(), a[:, 2:3].copy()


def _one(rows, max_gap=1, ms=None):
    H, L, C = _cols(*rows)
    ms = np.array([0, len(rows)]) if ms is None else np.asarray(ms)
    return RR.range_sums(H, L, C, ms, max_gap)


def _same(a, b, keys=RR.SUMS + RR.SCALES):
    return all(np.array_equal(a[k].view(np.int64) if a[k].dtype == np.float64 else a[k],
                              b[k].view(np.int64) if b[k].dtype == np.float64 else b[k])
               for k in keys)


def test_constant_prices_give_exact_zeros():
    T_d = 44
    H = np.full((T_d, 3), 25.5)
    ms = np.array([0, 21, 44])
    s = RR.range_sums(H, H.copy(), H.copy(), ms)
    assert (s["NRG"] == [[21] * 3, [23] * 3]).all() and (s["NPR"] == [[20] * 3, [23] * 3]).all()
    assert (s["NCS"] == s["NPR"]).all()
    for k in RR.FSUMS + RR.SCALES:
        assert (s[k] == 0.0).all() and not np.signbit(s[k]).any(), k
    m = RR.range_model(s, 1)
    assert (m["PKVOL"] == 0.0).all() and (m["CSSPR"] == 0.0).all() and (m["ARSPR"] == 0.0).all()


def _paper_cs(H1, L1, H2, L2):
    """Corwin-Schultz (2012) eqs. 14, 18 on a pair with no overnight move, ratio form."""
    beta = math.log(H1 / L1) ** 2 + math.log(H2 / L2) ** 2
    gamma = math.log(max(H1, H2) / min(L1, L2)) ** 2
    alpha = (math.sqrt(2 * beta) - math.sqrt(beta)) / K - math.sqrt(gamma / K)
    return 2 * (math.exp(alpha) - 1) / (1 + math.exp(alpha))


def test_hand_worked_pair_against_the_papers():
    d1, d2 = (101.0, 99.0, 100.0), (101.5, 99.5, 101.0)     # C1 inside day 2: no overnight shift
    s = _one([d1, d2])
    assert s["NRG"][0, 0] == 2 and s["NPR"][0, 0] == 1 and s["NCS"][0, 0] == 1
    pk = math.log(101.0 / 99.0) ** 2 + math.log(101.5 / 99.5) ** 2
    cs = _paper_cs(101.0, 99.0, 101.5, 99.5)
    assert cs > 0
    ar = (math.log(100.0) - math.log(101.0 * 99.0) / 2) * (math.log(100.0)
                                                          - math.log(101.5 * 99.5) / 2)
    for k, want in (("SPK", pk), ("SCS", cs), ("SAR", ar)):
        err = abs(s[k][0, 0] - want) / s[k + "_scale"][0, 0]
        print(k, s[k][0, 0], want, err)
        assert err <= BAR, k
    assert s["SAR_scale"][0, 0] == abs(s["SAR"][0, 0]) and s["SPK_scale"][0, 0] == s["SPK"][0, 0]
    assert s["SCS_scale"][0, 0] > 10 * s["SCS"][0, 0]          # the magnitudes cancel in alpha
    m = RR.range_model(s, 1, 1)
    assert m["PKVOL"][0, 0] == math.sqrt(s["SPK"][0, 0] / (RR.C4 * 2.0))
    assert m["CSSPR"][0, 0] == s["SCS"][0, 0] and m["NOBS"][0, 0] == 1
    assert m["ARSPR"][0, 0] == (2.0 * math.sqrt(s["SAR"][0, 0]) if ar > 0 else 0.0)


def test_overnight_shift_branches():
    """Up, down and none, on prices whose shifted range is exact: the pair's S is the S of the
    pair with day d moved by hand, bit for bit; the Abdi-Ranaldo term takes the raw day."""
    p = (101.0, 99.0, 100.0)
    none, _ = RR.cs_pair(*p, 102.0, 100.0)
    up, _ = RR.cs_pair(*p, 104.0, 102.0)         # L > C': s = 2, the range comes down to 102 / 100
    down, _ = RR.cs_pair(*p, 97.0, 95.0)         # H < C': s = -3, the range goes up to 100 / 98
    assert up == none and down == RR.cs_pair(*p, 100.0, 98.0)[0]
    assert none == pytest.approx(_paper_cs(101.0, 99.0, 102.0, 100.0), rel=1e-9)
    assert down == pytest.approx(_paper_cs(101.0, 99.0, 100.0, 98.0), rel=1e-9)
    inside, _ = RR.cs_pair(*p, 100.5, 99.5)      # C' inside the day's range: no shift
    assert inside == pytest.approx(_paper_cs(101.0, 99.0, 100.5, 99.5), rel=1e-9)
    raw = _one([p, (104.0, 102.0, 103.0)])
    moved = _one([p, (102.0, 100.0, 101.0)])
    assert raw["SCS"][0, 0] == moved["SCS"][0, 0] and raw["SAR"][0, 0] != moved["SAR"][0, 0]
    eta1, eta2 = (math.log(101.0) + math.log(99.0)) * 0.5, (math.log(104.0) + math.log(102.0)) * 0.5
    assert raw["SAR"][0, 0] == (math.log(100.0) - eta1) * (math.log(100.0) - eta2)


def test_negative_spread_is_floored_per_pair():
    a, b = (101.0, 99.0, 101.0), (103.0, 100.5, 102.0)     # a wide two-day range, no shift
    S, _ = RR.cs_pair(*a, b[0], b[1])
    assert S < 0
    s = _one([a, b])
    assert s["NCS"][0, 0] == 1 and s["SCS"][0, 0] == 0.0 and s["SCS_scale"][0, 0] > 0


def test_shifted_low_at_zero_counts_as_a_pair_without_a_spread():
    """L* = L - (L - C') is C' up to rounding, so it is <= 0 only when C' is under half an ulp
    of L: a close of 1e-18 before a day at 0.02."""
    rows = [(2e-18, 1e-18, 1e-18), (0.03, 0.02, 0.02), (0.03, 0.02, 0.03)]
    S, _ = RR.cs_pair(*rows[0], 0.03, 0.02)
    assert S != S and 0.02 - (0.02 - 1e-18) == 0.0
    s = _one(rows)
    assert s["NRG"][0, 0] == 3 and s["NPR"][0, 0] == 2 and s["NCS"][0, 0] == 1
    one = _one(rows[1:])
    assert s["SCS"][0, 0] == one["SCS"][0, 0] and s["SCS_scale"][0, 0] == one["SCS_scale"][0, 0]
    assert s["SAR"][0, 0] != one["SAR"][0, 0]               # the Abdi-Ranaldo term is booked


REJECTED = {
    "H NaN": (np.nan, 99.0, 100.0), "L NaN": (101.0, np.nan, 100.0),
    "C NaN": (101.0, 99.0, np.nan), "H ABSENT": (O.absent_scalar(), 99.0, 100.0),
    "L ABSENT": (101.0, O.absent_scalar(), 100.0), "C ABSENT": (101.0, 99.0, O.absent_scalar()),
    "L zero": (101.0, 0.0, 100.0), "L negative": (101.0, -1.0, 100.0),
    "H < L": (99.0, 101.0, 100.0), "C > H": (101.0, 99.0, 101.5), "C < L": (101.0, 99.0, 98.5),
}


@pytest.mark.parametrize("why", sorted(REJECTED))
def test_rejected_row_changes_no_state(why):
    a, b = (101.0, 99.0, 100.0), (102.5, 100.5, 101.0)
    assert not RR.ranged(*REJECTED[why]) and RR.ranged(*a) and RR.ranged(*b)
    want = _one([a, b])
    got = _one([a, REJECTED[why], b], max_gap=2)           # the pair holds across the row
    assert _same(got, want) and got["NPR"][0, 0] == 1
    cut = _one([a, REJECTED[why], b], max_gap=1)           # and is out of reach at max_gap 1
    assert cut["NRG"][0, 0] == 2 and cut["NPR"][0, 0] == 0 and cut["SCS"][0, 0] == 0.0
    assert cut["SPK"][0, 0] == want["SPK"][0, 0]


T_DAYS = 782


def _gap_panel(max_gap):
    col, cases = DR.gap_column(T_DAYS, max(max_gap, 2), 170, O.absent_scalar())
    with np.errstate(invalid="ignore"):      # (the ABSENT payload is a signalling NaN)
        C = np.round(col, 2)[:, None]
        return np.round(C * 1.01, 2), np.round(C * 0.99, 2), C, cases


@pytest.mark.parametrize("max_gap", [1, 3, 10])
def test_max_gap_on_the_gap_column(max_gap):
    H, L, C, cases = _gap_panel(max_gap)
    days = np.arange(T_DAYS + 1)                           # a month a day: NPR[d] is row d's pair
    npr = RR.range_sums(H, L, C, days, max_gap)["NPR"][:, 0]
    ok = ~np.isnan(C[:, 0])
    if max_gap == 1:
        assert np.array_equal(npr[1:] == 1, ok[1:] & ok[:-1]) and npr[0] == 0
    else:
        assert [int(npr[d]) for d, _, _ in cases] == [int(b) for _, _, b in cases]
        assert {b for _, _, b in cases} == {True, False}
    assert npr.sum() >= 700


def _months():
    return np.concatenate([np.arange(0, T_DAYS, 21), [T_DAYS]]).astype(np.int64)


def test_zero_length_month():
    H, L, C, _ = _gap_panel(3)
    ms = _months()
    base = RR.range_sums(H, L, C, ms, 3)
    ms0 = np.concatenate([ms[:5], ms[4:]])                 # month 4 has no day
    got = RR.range_sums(H, L, C, ms0, 3)
    for k in RR.SUMS:
        assert (got[k][4] == 0).all(), k
        assert np.array_equal(np.delete(got[k], 4, axis=0), base[k]), k


@pytest.mark.parametrize("max_gap", [1, 3, 10])
def test_month_chunks_give_the_same_bits(max_gap):
    """Runs on month ranges with their lead-in equal the whole run; the gap column's gaps cross
    7-row chunk starts, and a 21-row month start lies inside several."""
    H, L, C, _ = _gap_panel(max_gap)
    rng = np.random.default_rng(7)
    H = np.concatenate([H, np.round(H * 1.5, 2)], axis=1)
    L = np.concatenate([L, np.round(L * 1.5, 2)], axis=1)
    C = np.concatenate([C, np.round(C * 1.5, 2)], axis=1)
    H[rng.random(H.shape) < 0.05] = np.nan
    for ms in (_months(), np.concatenate([np.arange(0, T_DAYS, 7), [T_DAYS]])):
        whole = RR.range_sums(H, L, C, ms, max_gap)
        T_m = len(ms) - 1
        for G in (2, 5, T_m):
            cuts = [T_m * g // G for g in range(G + 1)]
            parts = [RR.range_sums(H, L, C, ms, max_gap, cuts[g], cuts[g + 1]) for g in range(G)]
            got = {k: np.concatenate([p[k] for p in parts]) for k in RR.SUMS + RR.SCALES}
            assert _same(got, whole), (G, T_m)
        assert whole["NPR"].sum() > 1000 and (whole["NCS"] == whole["NPR"]).all()


def test_window_model_on_hand_made_sums():
    z = lambda *v: np.array(v, dtype=np.float64)[:, None]      # noqa: E731
    i = lambda *v: np.array(v, dtype=np.int32)[:, None]        # noqa: E731
    sums = dict(NRG=i(10, 12, 8), NPR=i(9, 12, 7), NCS=i(9, 11, 6), SPK=z(0.004, 0.006, 0.002),
                SCS=z(0.09, 0.11, 0.03), SAR=z(0.0009, -0.0030, 0.0007))
    m = RR.range_model(sums, 2, 20)
    assert np.isnan(m["PKVOL"][0]) and np.isnan(m["CSSPR"][0]) and np.isnan(m["ARSPR"][0])
    assert m["NOBS"][:, 0].tolist() == [0, 21, 19]
    # month 1: nrg 22, ncs 20, npr 21 -- every count at or over min_obs = 20
    assert m["PKVOL"][1, 0] == math.sqrt((0.004 + 0.006) / (RR.C4 * 22.0))
    assert m["CSSPR"][1, 0] == (0.09 + 0.11) / 20.0
    assert m["ARSPR"][1, 0] == 0.0                            # m = -0.0021 / 21 <= 0
    # month 2: nrg 20 (at the edge), ncs 17 and npr 19 (under it)
    assert m["PKVOL"][2, 0] == math.sqrt((0.006 + 0.002) / (RR.C4 * 20.0))
    assert np.isnan(m["CSSPR"][2, 0]) and np.isnan(m["ARSPR"][2, 0])
    m = RR.range_model(sums, 1, 7)
    assert m["ARSPR"][0, 0] == 2.0 * math.sqrt(0.0009 / 9.0) and m["ARSPR"][1, 0] == 0.0
    assert m["ARSPR"][2, 0] == 2.0 * math.sqrt(0.0007 / 7.0)   # npr == min_obs
    assert np.isnan(m["CSSPR"][2, 0]) and m["CSSPR"][1, 0] == 0.11 / 11.0
    m = RR.range_model(sums, 1)                                # the default: 15 days
    assert np.isnan(m["PKVOL"]).all() and np.isnan(m["ARSPR"]).all()
    zero = dict(sums, SAR=z(0.0, 0.0, 0.0))
    assert (RR.range_model(zero, 1, 1)["ARSPR"] == 0.0).all()
    assert RR.C4 == 4.0 * math.log(2.0)


def test_simulated_path_recovers_the_volatility_and_sees_the_spread():
    """A seeded driftless log-price path, 780 steps a day, sigma 1 % a day, 8 assets x 504 days in
    months of 21 (192 cells), through the reference on the CPU.  Without a spread the discrete
    range understates the continuous one a little and a month of 21 ranges estimates sigma to about
    7 %: this run's PKVOL / sigma has mean 0.9767 and cells in 0.7616 .. 1.1603.  Asserted: the
    mean in [0.95, 1.00] (the 2 % understatement, and four standard errors of 0.5 % either side)
    and every cell in [0.70, 1.25] (four of its own standard deviations).  With a half-spread of
    0.5 % on every trade, bought or sold at random, the mean spreads measured are CSSPR 0.01086
    (0.00410 without a spread: the zero floor's bias) and ARSPR 0.00949 (0.00214); asserted: each
    within 0.007 .. 0.014 of the 1 % quoted and more than twice its zero-spread mean."""
    rng = np.random.default_rng(2012)
    N, T_d, n, sigma, half = 8, 504, 780, 0.01, 0.005
    ms = np.arange(0, T_d + 1, 21)
    lp = np.cumsum(rng.standard_normal((T_d * n, N)) * (sigma / math.sqrt(n)), axis=0)
    mid = 50.0 * np.exp(lp)
    side = np.where(rng.random(mid.shape) < 0.5, 1.0 - half, 1.0 + half)
    out = {}
    for tag, px in (("mid", mid), ("trade", mid * side)):
        d = px.reshape(T_d, n, N)
        s = RR.range_sums(d.max(axis=1), d.min(axis=1), d[:, -1, :].copy(), ms)
        out[tag] = RR.range_model(s, 1)
        assert (s["NRG"] == 21).all() and (s["NCS"] == s["NPR"]).all()
    ratio = out["mid"]["PKVOL"] / sigma
    print("PKVOL / sigma:", ratio.min(), ratio.mean(), ratio.max())
    assert 0.95 <= ratio.mean() <= 1.00 and 0.70 <= ratio.min() and ratio.max() <= 1.25
    cs0, cs1 = out["mid"]["CSSPR"].mean(), out["trade"]["CSSPR"].mean()
    ar0, ar1 = out["mid"]["ARSPR"].mean(), out["trade"]["ARSPR"].mean()
    print("CSSPR", cs0, cs1, "ARSPR", ar0, ar1)
    assert cs0 < 0.5 * cs1 and 0.007 <= cs1 <= 0.014
    assert ar0 < 0.5 * ar1 and 0.007 <= ar1 <= 0.014


def test_range_from_long_on_a_hand_built_frame():
    import csmom
    from csmom.panel import from_long, range_from_long
    rows = [("2024-01-02", "AAA", 10.0, 10.5, 9.5, 10.2),
            ("2024-01-03", "AAA", 10.2, 10.6, 10.0, 10.4),
            ("2024-01-03", "AAA", 10.2, np.nan, 10.1, 10.5),   # a duplicate: last non-NaN wins
            ("2024-01-04", "AAA", 10.4, "n/a", 10.3, 10.6),    # not numeric
            ("2024-01-02", "BBB", 20.0, 20.5, 19.5, 20.2),
            ("2024-01-04", "BBB", 20.4, 20.8, None, 20.6)]     # BBB has no row on 01-03
    df = pd.DataFrame(rows, columns=["date", "ticker", "adj_close", "high", "low", "close"])
    with pytest.warns(RuntimeWarning):
        panel = from_long(df)
    H, L, C = range_from_long(df, panel)
    assert H.shape == panel.P.shape == (3, 2) and list(panel.tickers) == ["AAA", "BBB"]
    ab = O.is_absent
    assert ab(H[1, 1]) and ab(L[1, 1]) and ab(C[1, 1]) and ab(H).sum() == 1
    assert H[:, 0].tolist()[:2] == [10.5, 10.6] and np.isnan(H[2, 0]) and not ab(H[2, 0])
    assert L[:, 0].tolist() == [9.5, 10.1, 10.3] and C[:, 0].tolist() == [10.2, 10.5, 10.6]
    assert H[0, 1] == 20.5 and H[2, 1] == 20.8 and np.isnan(L[2, 1]) and not ab(L[2, 1])
    assert C[2, 1] == 20.6
    for missing in ("high", "low", "close"):
        with pytest.raises(ValueError):
            range_from_long(df.drop(columns=[missing]), panel)
    assert csmom.range_from_long is range_from_long


def test_names_exports_and_abi():
    import csmom
    from csmom import Engine
    from csmom.regress import SIGNAL_NAMES
    assert Engine.RANGE_SIGNALS == {"pkvol": "PKVOL", "cs_spread": "CSSPR", "ar_spread": "ARSPR"}
    assert set(Engine.RANGE_SIGNALS) <= set(Engine.RUN_SIGNALS)
    assert Engine.RUN_SIGNALS[-3:] == ("illiq", "dvol", "zret")
    assert Engine.RUN_SIGNALS[-6:-3] == ("pkvol", "cs_spread", "ar_spread")
    assert set(Engine.RANGE_SIGNALS) <= set(SIGNAL_NAMES)
    assert Engine.RANGE_OUTPUTS == RR.MODEL
    assert csmom.RANGE_COLUMNS == ["ticker", "date", "pkvol", "cs_spread", "ar_spread", "nobs"]
    for name in ("RangeSums", "RangeModelOut", "RANGE_COLUMNS", "range_signals"):
        assert name in csmom.__all__ and hasattr(csmom, name), name
    assert csmom.RangeSums._fields == RR.SUMS
    lib = csmom.load_library()
    assert lib.csm_abi_version() == 3
    assert hasattr(lib, "csm_range_sums") and hasattr(lib, "csm_range_model")
    for key in (b"rsums_chunks", b"rmodel_chunks"):
        assert lib.csm_tune(key, 3) == 0 and lib.csm_tune(key, 0) == 0 and lib.csm_tune(key, -1) != 0
