"""CPU: the synthetic panels of tests/portfolio_cases.py contain what they claim, and the
thresholds the K lists are derived from are the ones csrc/portfolio.hip compiles with.  Oracle
only (PO.member_weights / PO.portfolio); no GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

import portfolio_cases as PC

HIP = (Path(__file__).resolve().parents[1]
       / "cross-sectional-momentum-strategy-replication-backtesting-framework_amd" / "csrc" / "portfolio.hip")
DEFINES = ("TP_U", "AC_MAXKD", "SEG_MAXKD", "TO_MAXQ", "TO_MAXK", "OV_TRIP", "TO_GEN_TB", "LS_PB",
           "SEG_MAXN", "PF_CHUNK_MIN")


def parse_thresholds(text):
    """{name: value} of the #defines in DEFINES plus BM_MAXK (the `kq <= 31` of the general
    equal-weight kernel choice); a missing one raises."""
    out = {}
    for name in DEFINES:
        m = re.findall(rf"^\s*#define\s+{name}\s+(\d+)\b", text, flags=re.M)
        assert len(m) == 1, f"{name}: {len(m)} definitions in portfolio.hip"
        out[name] = int(m[0])
    m = re.findall(r"\bkq\s*<=\s*(\d+)\s*&&\s*\(N\s*&\s*3\)\s*==\s*0", text)
    assert len(m) == 1, f"BM_MAXK: {len(m)} `kq <= ..` choices in portfolio.hip"
    out["BM_MAXK"] = int(m[0])
    return out


def test_thresholds_match_the_source():
    got = parse_thresholds(HIP.read_text())
    for name, v in got.items():
        assert v == getattr(PC, name), (name, v, getattr(PC, name))


def test_threshold_parser_notices_a_change():
    """The parity check has teeth: a moved or missing threshold in the source text is seen."""
    text = HIP.read_text()
    moved = re.sub(r"#define AC_MAXKD 384", "#define AC_MAXKD 256", text)
    assert parse_thresholds(moved)["AC_MAXKD"] == 256 != PC.AC_MAXKD
    with pytest.raises(AssertionError):
        parse_thresholds(text.replace("#define TP_U ", "#define TP_V "))
    with pytest.raises(AssertionError):
        parse_thresholds(text.replace("kq <= 31", "kq < 32"))


def test_k_lists_are_the_issue_lists():
    """The derived lists are the ones the thresholds were read off; when a constant moves, the
    lists move with it and this test names the new ones."""
    assert PC.k_lists() == {
        10: [8, 9, 13, 15, 16, 17, 31, 32, 33, 38, 39, 46, 47, 64, 240],
        30: [12, 13, 16, 17],
        2: [170, 171, 192, 193]}
    assert PC.k_all_costs() == (31, 32, 240)
    assert PC.k_odd_widths() == (17, 33, 47)
    assert PC.k_forced_modes() == (17, 47)
    assert PC.F1_KS == ((3, 11), (3, 12)) and PC.F3_KS == ((3, 32), (3, 33))
    # each K list entry sits where the table says it does
    for nb, Ks in PC.k_lists().items():
        assert any(K * nb <= PC.AC_MAXKD < (K + 1) * nb for K in Ks)
        assert any(K * (nb + 1) <= PC.SEG_MAXKD < (K + 1) * (nb + 1) for K in Ks)
        assert all(1 <= K <= PC.TO_MAXK for K in Ks)


def test_case_list_shapes():
    ids = [g[0] for g in PC.group_a()]
    assert len(ids) == len(set(ids))
    for grp in (PC.group_b(), PC.group_c(), PC.group_d(), PC.group_e()):
        names = [g[0] for g in grp]
        assert len(names) == len(set(names))
    for _, c, _, _ in PC.group_a():
        assert c.T_m == c.K + 9 and c.B == 2 and c.N in (260, 259, 258)
        assert c.N > PC.PF_CHUNK_MIN   # two turnover chunks
    assert max(c.B for _, c, _, _ in PC.group_b()) >= PC.LS_PB


def test_make_case_fractions_and_plants():
    a = PC.make_case(60, 3, 400, 10, 7, True, plant=PC.ALL_PLANTS)
    pm = PC.plant_months(60)
    L, NR, W, ADV, SIG = a["L"], a["NR"], a["W"], a["ADV"], a["SIG"]
    assert L.dtype == np.int8 and L.shape == NR.shape == W.shape == ADV.shape == SIG.shape == (60, 3, 400)
    assert L.min() == -1 and L.max() == 9
    cnt = np.bincount(L[:, 2].ravel() + 1, minlength=11) / L[:, 2].size
    assert np.abs(cnt - 1 / 11).max() < 0.01                      # uniform in [-1, n_bins)
    assert 0.04 < np.isnan(NR[:, 2]).mean() < 0.06
    assert 0.005 < np.isnan(W[:, 2]).mean() < 0.015 and 0.005 < (W[:, 2] == -1.0).mean() < 0.015
    assert 0.01 < np.isnan(SIG).mean() < 0.03
    assert 0 < (ADV == 0.0).sum() < 0.01 * ADV.size
    for t in pm["empty_top"]:
        assert not (L[t, 0] == 9).any() and (L[t, 2] == 9).any()
    assert max(pm["empty_top"]) == 59 and min(pm["empty_top"]) >= 1
    assert (L[pm["blank_month"], 0] == -1).all()
    assert np.isnan(NR[pm["nan_month"], 0]).all()
    w = W[pm["dead_weights"], 0]
    assert not (np.isfinite(w) & (w > 0)).any()
    assert not (L[:, 1] == 9).any() and (L[:, 0] == 9).any()
    assert PC.make_case(60, 3, 400, 10, 7, False)["W"] is None
    # the same seed gives the same panel; another label seed changes the labels only
    b = PC.make_case(60, 3, 400, 10, 7, True, plant=PC.ALL_PLANTS, label_seed=8)
    assert np.array_equal(b["NR"], NR, equal_nan=True) and not np.array_equal(b["L"], L)


CASES = PC.all_cases()


def _cid(c):
    return (f"T{c.T_m}-B{c.B}-N{c.N}-nb{c.n_bins}-K{c.K}-s{c.seed}"
            f"{'' if c.label_seed is None else '-l%d' % c.label_seed}-{'vw' if c.vw else 'ew'}")


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_case_contains_what_it_claims(case):
    a = PC.arrays(case)
    K, nb = case.K, case.n_bins
    ref = PC.oracle_ref(case, K, False)
    PR, LS, TURN = ref["PR"], ref["LS"], ref["TURN"]
    steady, nonfull = PC.row_classes(case, K)
    known = {"steady", "nonfull", "no_row_ge_K", "pr_nan", "pr_finite", "turn_finite", "turn0",
             "ls_fallback"}
    assert set(case.claims) <= known
    for claim in case.claims:
        if claim == "steady":
            assert steady.any(), "no row with t >= K and every window full"
        elif claim == "nonfull":
            assert nonfull.any(), "no row with t >= K and a window that is not full"
        elif claim == "no_row_ge_K":
            assert case.T_m <= K and not steady.any() and not nonfull.any()
        elif claim == "pr_nan":
            assert np.isnan(PR).any()
        elif claim == "pr_finite":
            assert np.isfinite(PR).any()
        elif claim == "turn_finite":
            assert np.isfinite(TURN).all()
        elif claim == "turn0":
            both = PC.leg_nonempty(case)[0].all(axis=1)          # [B]: month 0 has both legs
            assert both.any()
            assert np.allclose(TURN[0][both], 1.0, rtol=0, atol=1e-12)
        elif claim == "ls_fallback":
            assert "no_top_ever" in case.plant and not (a["L"][:, 1] == nb - 1).any()
            pr = PR[:, 1, :]
            assert np.isnan(pr[:, nb - 1]).all()
            ok = ~np.isnan(pr).all(axis=1)
            assert ok.any()
            want = np.nanmax(pr[ok], axis=1) - np.nanmin(pr[ok], axis=1)
            assert np.array_equal(LS[ok, 1], want) and np.isnan(LS[~ok, 1]).all()
    if "empty_top" in case.plant and case.T_m > K:
        assert max(PC.plant_months(case.T_m)["empty_top"]) >= K
        # a top-less month inside the window keeps rows with t >= K on the general launch
        assert nonfull[:, 0].any()
    # the planted months leave the oracle's conventions intact: NET = LS - COST
    assert np.array_equal(np.isnan(ref["NET"]), np.isnan(LS))
