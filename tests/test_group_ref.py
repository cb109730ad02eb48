"""CPU: tests/group_ref.py, the restatement of rules N1..N5 the GPU tests compare against -- its
labels against the reference's own groupby(['date', 'group']) transform (group_sorts.npz), its
pooled means against oracle.portfolio_ew on the same labels, n_groups = 1 against assign_deciles
-- the C boundary of the two new calls, and neutral_momentum's ticker -> group id mapping.  This
checks the rules, not the kernel.
"""
import re
from pathlib import Path

import numpy as np
import pytest

import group_ref as GR
from conftest import load_golden, max_rel
from oracle import csmom_oracle as O

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def golden():
    return load_golden("group_sorts")


@pytest.fixture(scope="module")
def edge():
    return load_golden("edge")


@pytest.mark.parametrize("name", ["one", "four", "moving"])
def test_panel_labels_match_reference(golden, edge, name):
    M = edge["J12s1_M"]
    L = GR.group_labels(M, golden[f"{name}_gid"], int(golden[f"{name}_ngroups"]))
    want = golden[f"{name}_L"]
    assert (want >= 0).mean() > 0.3   # the fixture ranks something
    assert np.array_equal(L, want)


def test_fixture_covers_the_named_group_shapes(golden, edge):
    gid = golden["four_gid"]
    assert (gid[0] == 3).sum() == 1 and (gid[0] == -1).sum() > 0
    assert (np.diff(golden["moving_gid"].astype(np.int64), axis=0) != 0).any()
    sizes = np.diff(golden["xs_offsets"])
    assert sizes.min() >= 1 and sizes.max() > 400
    assert set(golden["xs_nbins"].tolist()) == {2, 3, 5, 10}
    v = golden["xs_values"]
    assert (np.signbit(v) & (v == 0.0)).any() and ((~np.signbit(v)) & (v == 0.0)).any()


def test_synthetic_labels_match_reference(golden):
    off = golden["xs_offsets"]
    for c in range(len(off) - 1):
        sl = slice(off[c], off[c + 1])
        nb = int(golden["xs_nbins"][c])
        L = GR.group_labels(golden["xs_values"][sl][None], golden["xs_gid"][sl][None], 5, nb)
        ref = golden["xs_labels"][sl]
        want = np.where(np.isnan(ref), -1, ref).astype(np.int8)
        assert np.array_equal(L[0], want), (c, nb)


def test_small_group_rules(golden):
    """A group of one value or of equal values is NaN; two distinct values get 0 and n - 1."""
    S = np.array([[1.0, 2.0, 5.0, 5.0, 5.0, 3.0, np.nan]])
    gid = np.array([0, 0, 1, 1, 1, 2, 0], dtype=np.int16)
    for nb in (2, 3, 5, 10):
        L = GR.group_labels(S, gid, 3, nb)
        assert L.tolist() == [[0, nb - 1, -1, -1, -1, -1, -1]]
    assert GR.group_labels(S, gid, 3, 10, min_group=3).tolist() == [[-1] * 7]


def test_one_group_is_assign_deciles(edge):
    M = edge["J12s1_M"]
    for nb in (3, 10):
        L = GR.group_labels(M, np.zeros(M.shape[1], dtype=np.int16), 1, nb)
        assert np.array_equal(L, O.assign_deciles(M, nb))


@pytest.mark.parametrize("name", ["four", "moving"])
def test_pooled_means_match_portfolio_ew(golden, edge, name):
    M, NR = edge["J12s1_M"], edge["J12s1_NR"]
    gid, ng = golden[f"{name}_gid"], int(golden[f"{name}_ngroups"])
    L = GR.group_labels(M, gid, ng)
    r = GR.group_means(L, NR, GR.membership(M, gid, ng), ng, 10)
    EW, CNT, LS = O.portfolio_ew(L, NR, 10)
    assert np.array_equal(r["CNT"], CNT)
    assert np.array_equal(np.isnan(r["EW"]), np.isnan(EW))
    assert max_rel(r["EW"], EW) <= 1e-10
    assert np.array_equal(np.isnan(r["LS"]), np.isnan(LS)) and max_rel(r["LS"], LS) <= 1e-10
    assert np.array_equal(r["NV"], (GR.membership(M, gid, ng) >= 0).sum(axis=1))
    assert np.array_equal(r["CNTG"].sum(axis=1), CNT)


def test_group_stats_and_adjusted_signals(golden, edge):
    M = edge["J12s1_M"]
    gid, ng = golden["four_gid"], 4
    GCNT, GMEAN, GSD = GR.group_stats(M, gid, ng)
    mem = GR.membership(M, gid, ng)
    t = int(np.argmax(GCNT[:, 0]))
    v = M[t, mem[t] == 0]
    assert GCNT[t, 0] == len(v) > 2
    assert abs(GMEAN[t, 0] - v.mean()) <= 1e-15 * max(1.0, abs(v).max())
    assert abs(GSD[t, 0] - v.std(ddof=1)) <= 1e-14 * v.std(ddof=1)
    one = GCNT == 1
    assert one.any() and np.isnan(GSD[one]).all() and not np.isnan(GMEAN[one]).any()
    SA, SZ, SB = GR.adjusted(M, gid, ng, GMEAN, GSD)
    assert np.array_equal(np.isnan(SA), mem < 0) and np.array_equal(np.isnan(SB), mem < 0)
    assert np.isnan(SZ[mem == 3]).all()   # the single-ticker group has no deviation
    assert np.array_equal(SA[t, mem[t] == 0], v - GMEAN[t, 0])


# ------------------------------------------------------------------------------ C boundary
def _header():
    return (ROOT / "include" / "csmom.h").read_text()


@pytest.mark.parametrize("name,nparams", [("csm_group_deciles", 18), ("csm_group_stats", 13)])
def test_header_declares(name, nparams):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} is not declared in include/csmom.h"
    assert len([p for p in m.group(1).split(",") if p.strip()]) == nparams


def test_abi_version_unchanged():
    assert re.search(r"#define\s+CSM_ABI_VERSION\s+3\b", _header())


def test_lib_lists_both():
    import csmom
    from csmom import _lib
    assert len(_lib.SIGNATURES["csm_group_deciles"][1]) == 18
    assert len(_lib.SIGNATURES["csm_group_stats"][1]) == 13
    assert {"csm_group_deciles", "csm_group_stats"} <= set(_lib.EXPORTS)
    assert callable(csmom.neutral_momentum) and callable(csmom.dependent_double_sort)


# ------------------------------------------------------------------- ticker -> id mapping
def test_group_id_mapping_on_real_tickers():
    import csmom
    tickers = load_golden("real_data")["tickers"].tolist()
    sectors = ["tech", "energy", "banks", None, float("nan")]
    groups = {tk: sectors[i % 5] for i, tk in enumerate(tickers)}
    del groups[tickers[0]]   # a ticker the mapping does not know
    gid, names = csmom.group_ids(tickers, groups)
    assert names == ["banks", "energy", "tech"]
    assert gid.dtype == np.int16 and gid.shape == (len(tickers),)
    for i, tk in enumerate(tickers):
        lab = groups.get(tk)
        want = names.index(lab) if isinstance(lab, str) else -1
        assert gid[i] == want, (tk, lab)
    assert gid[0] == -1 and (gid == -1).sum() >= 2 * (len(tickers) // 5)
    import pandas as pd
    gid2, names2 = csmom.group_ids(tickers, pd.Series(groups))
    assert names2 == names and np.array_equal(gid2, gid)
