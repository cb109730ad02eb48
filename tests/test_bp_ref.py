"""CPU: tests/bp_ref.py, the restatement of rules U1..U6 the GPU tests compare against -- its
labels against the reference's assign_deciles_per_date on the subset alone and pandas'
cut(include_lowest=True) on the whole row, its edges against pandas' retbins
(tests/golden/breakpoints.npz), BP all ones against assign_deciles, the screen on a hand-written
case -- the C boundary of the two new calls, and universe_momentum's ticker -> mask mapping.  This
checks the rules, not the kernel.
"""
import re
from pathlib import Path

import numpy as np
import pytest

import bp_ref as BR
from conftest import load_golden
from oracle import csmom_oracle as O

ROOT = Path(__file__).resolve().parents[1]
NAN = np.nan


@pytest.fixture(scope="module")
def golden():
    return load_golden("breakpoints")


@pytest.fixture(scope="module")
def edge():
    return load_golden("edge")


def check_row(L, e, x, bp, sub, cut):
    """One date of the ref against the fixture: subset members, in-range and out-of-range cells."""
    ranked = ~np.isnan(x)
    mem = ranked & (bp != 0)
    want = np.where(np.isnan(sub), -1, sub).astype(np.int8)
    assert np.array_equal(L[mem], want[mem])            # the reference on the subset alone
    assert (L[~ranked] == -1).all()
    if len(e) < 2:
        assert (L == -1).all() and np.isnan(cut).all()
        return 0
    inr = ~np.isnan(cut)
    assert np.array_equal(L[inr], cut[inr].astype(np.int8))   # pandas' cut inside [e_0, e_m]
    below, above = ranked & (x < e[0]), ranked & (x > e[-1])
    assert np.array_equal(ranked & ~inr, below | above)
    assert (L[below] == 0).all() and (L[above] == len(e) - 2).all()
    return int(below.sum() + above.sum())


@pytest.mark.parametrize("name", ["static", "moving"])
def test_panel_matches_reference_and_pandas(golden, edge, name):
    M, bp = edge["J12s1_M"], golden[f"{name}_bp"]
    r = BR.deciles_bp(M, None, bp, 10)
    rows = BR.bp_rows(bp, M.shape[0])
    outside = 0
    for t in range(M.shape[0]):
        ne = int(golden[f"{name}_ne"][t])
        assert r["NE"][t] == ne
        # retbins, compared with == (the sign of a zero is free); NaN padding after them
        assert (r["EDGES"][t, :ne] == golden[f"{name}_edges"][t, :ne]).all()
        assert np.isnan(r["EDGES"][t, ne:]).all()
        lsub = golden[f"{name}_Lsub"][t]
        outside += check_row(r["L"][t], r["EDGES"][t, :ne], M[t], rows[t],
                             np.where(lsub < 0, NAN, lsub.astype(np.float64)),
                             golden[f"{name}_cut"][t])
    assert outside > 20                                  # cells beyond the subset's range exist
    assert (r["L"] >= 0).mean() > 0.2 and (golden[f"{name}_Lsub"] >= 0).mean() > 0.05
    assert np.array_equal(r["NVB"], ((rows != 0) & ~np.isnan(M)).sum(axis=1))


def test_fixture_covers_the_named_shapes(golden, edge):
    assert set(np.unique(golden["static_bp"]).tolist()) == {0, 1, 200}
    assert (np.diff(golden["moving_bp"].astype(np.int64), axis=0) != 0).any()
    nvb = ((golden["moving_bp"] != 0) & ~np.isnan(edge["J12s1_M"])).sum(axis=1)
    assert {0, 1, 2} <= set(nvb.tolist())                # empty, one-member, two-member subsets
    sizes = np.diff(golden["xs_offsets"])
    assert sizes.min() == 1 and sizes.max() == 500 and len(sizes) >= 40
    assert set(golden["xs_nbins"].tolist()) == {2, 3, 5, 10, 20}
    v = golden["xs_values"]
    assert (np.signbit(v) & (v == 0.0)).any() and ((~np.signbit(v)) & (v == 0.0)).any()
    assert (golden["xs_ne"] < 2).any() and (golden["xs_ne"] == golden["xs_nbins"] + 1).any()


def test_synthetic_rows_match_reference_and_pandas(golden):
    off = golden["xs_offsets"]
    outside = 0
    for c in range(len(off) - 1):
        sl = slice(off[c], off[c + 1])
        nb, ne = int(golden["xs_nbins"][c]), int(golden["xs_ne"][c])
        x, bp = golden["xs_values"][sl], golden["xs_bp"][sl]
        r = BR.deciles_bp(x[None], None, bp, nb)
        assert r["NE"][0] == ne, c
        assert (r["EDGES"][0, :ne] == golden["xs_edges"][c, :ne]).all(), c
        assert np.isnan(r["EDGES"][0, ne:]).all()
        outside += check_row(r["L"][0], r["EDGES"][0, :ne], x, bp, golden["xs_sub"][sl],
                             golden["xs_cut"][sl])
    # a random share p of a row leaves about 2 (1 - p) / p of its cells beyond the subset's range
    # (1.3 to 4.7 here, fewer with ties): at least one per two rows
    assert outside >= (len(off) - 1) // 2


def test_two_value_subset_gives_every_edge():
    x = np.array([[0.5, 1.0, 2.0, 3.0, NAN, -1.0]])
    bp = np.array([0, 1, 1, 0, 1, 0], dtype=np.uint8)
    for nb in (2, 3, 5, 10, 20):
        r = BR.deciles_bp(x, None, bp, nb)
        assert r["NE"][0] == nb + 1 and r["NVB"][0] == 2
        assert r["L"][0].tolist() == [0, 0, nb - 1, nb - 1, -1, 0]


def test_all_ones_is_assign_deciles(edge):
    M = edge["J12s1_M"]
    for nb in (2, 3, 10, 20):
        r = BR.deciles_bp(M, None, np.ones(M.shape[1], dtype=np.uint8), nb)
        assert np.array_equal(r["L"], O.assign_deciles(M, nb))
        r2 = BR.deciles_bp(M, None, np.full(M.shape, 255, dtype=np.uint8), nb)
        assert np.array_equal(r2["L"], r["L"])


def test_means_are_portfolio_ew_on_the_labels(golden, edge):
    M, NR = edge["J12s1_M"], edge["J12s1_NR"]
    r = BR.deciles_bp(M, NR, golden["static_bp"], 10)
    EW, CNT, LS = O.portfolio_ew(r["L"], NR, 10)
    assert np.array_equal(r["CNT"], CNT) and r["CNT"].dtype == np.int32
    assert np.array_equal(r["EW"], EW, equal_nan=True) and np.array_equal(r["LS"], LS, equal_nan=True)
    assert np.array_equal(r["NV"], (~np.isnan(M)).sum(axis=1))
    assert CNT.sum() > 500


def test_screen_rule_by_hand():
    A = O.absent_scalar()
    M = np.array([[0.1, 0.2, NAN, 0.4, 0.5, 0.6],
                  [1.1, 1.2, 1.3, 1.4, A, 1.6],
                  [2.1, 2.2, 2.3, 2.4, 2.5, 2.6]])
    PM = np.array([[5.0, 4.99, 9.0, NAN, 6.0, 7.0],
                   [9.0, 9.0, A, 9.0, 9.0, 1.0],
                   [9.0, 9.0, 9.0, 9.0, 9.0, 9.0]])
    CAP = np.array([[10.0, 10.0, 10.0, 10.0, 2.0, NAN],
                    [3.0, 2.99, 5.0, 5.0, 5.0, 5.0],
                    [9.0, 9.0, 9.0, 9.0, 9.0, 9.0]])
    CAPMIN = np.array([2.0, 3.0, NAN])
    MS, KEPT = BR.screen(M, PM, 5.0, CAP, CAPMIN)
    want = np.array([[0.1, NAN, NAN, NAN, 0.5, NAN],
                     [1.1, NAN, NAN, 1.4, NAN, NAN],
                     [NAN] * 6])
    assert np.array_equal(MS, want, equal_nan=True) and KEPT.tolist() == [2, 2, 0]
    MS, KEPT = BR.screen(M, PM, 5.0)                     # the price screen alone
    assert KEPT.tolist() == [3, 3, 6] and np.isnan(MS[0, 1]) and MS[0, 5] == 0.6
    MS, KEPT = BR.screen(M, None, None, CAP, CAPMIN)     # the size screen alone
    assert KEPT.tolist() == [4, 4, 0] and MS[1, 5] == 1.6 and np.isnan(MS[1, 1])
    MS, KEPT = BR.screen(M)
    assert KEPT.tolist() == [5, 5, 6] and np.array_equal(MS, np.where(np.isnan(M), NAN, M),
                                                         equal_nan=True)


# ------------------------------------------------------------------------------ C boundary
def _header():
    return (ROOT / "include" / "csmom.h").read_text()


@pytest.mark.parametrize("name,nparams", [("csm_deciles_bp", 16), ("csm_screen", 10)])
def test_header_declares(name, nparams):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} is not declared in include/csmom.h"
    assert len([p for p in m.group(1).split(",") if p.strip()]) == nparams


def test_abi_version_unchanged():
    assert re.search(r"#define\s+CSM_ABI_VERSION\s+3\b", _header())


def test_lib_lists_both():
    import csmom
    from csmom import _lib
    assert len(_lib.SIGNATURES["csm_deciles_bp"][1]) == 16
    assert len(_lib.SIGNATURES["csm_screen"][1]) == 10
    assert {"csm_deciles_bp", "csm_screen"} <= set(_lib.EXPORTS)
    for name in ("deciles_bp", "breakpoints", "screen", "run_universe"):
        assert callable(getattr(csmom.Engine, name))
    assert callable(csmom.universe_momentum) and "UniverseResult" in csmom.__all__
    assert [csmom.Engine.size_bins(p) for p in (50, 25, 20, 10, 5)] == [2, 4, 5, 10, 20]
    with pytest.raises(ValueError):
        csmom.Engine.size_bins(30)


# --------------------------------------------------------------------- ticker -> mask mapping
def test_mask_and_shares_mapping_on_real_tickers():
    import pandas as pd
    import csmom
    tickers = load_golden("real_data")["tickers"].tolist()
    nyse = [tk for i, tk in enumerate(tickers) if i % 3 == 0] + ["NOT_IN_THE_FRAME"]
    mask = csmom.breakpoint_mask(tickers, nyse)
    assert mask.dtype == np.uint8 and mask.shape == (len(tickers),)
    assert mask.tolist() == [1 if i % 3 == 0 else 0 for i in range(len(tickers))]
    assert csmom.breakpoint_mask(tickers, None).tolist() == [1] * len(tickers)
    assert csmom.breakpoint_mask(tickers, set(nyse)).tolist() == mask.tolist()
    shares = {tk: 1e6 * (i + 1) for i, tk in enumerate(tickers)}
    shares[tickers[1]] = None
    shares[tickers[2]] = float("nan")
    del shares[tickers[3]]
    row = csmom.shares_row(tickers, shares)
    assert row.dtype == np.float64 and np.isnan(row[1:4]).all() and row[0] == 1e6
    assert np.array_equal(row[4:], 1e6 * (np.arange(4, len(tickers)) + 1))
    assert np.array_equal(csmom.shares_row(tickers, pd.Series(shares)), row, equal_nan=True)
