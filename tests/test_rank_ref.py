"""CPU: tests/rank_ref.py, the restatement of rules I1..I5 the GPU tests compare against -- its
ranks bit for bit against pandas' own (live, and as recorded in rank_ic.npz), its Spearman IC
against scipy's spearmanr and pandas' corr(method='spearman'), its Pearson IC against np.corrcoef
(1e-10 absolute: |IC| <= 1), the named degenerate rows, and the C boundary of the two new calls.
This checks the rules, not the kernel.
"""
import math
import re
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

import rank_ref as RR
from conftest import bits_equal, load_golden

ROOT = Path(__file__).resolve().parents[1]
METHODS = ("average", "min", "max")
TOL = 1e-10


@pytest.fixture(scope="module")
def golden():
    return load_golden("rank_ic")


def _rows(seed, T=5, N=211):
    rng = np.random.default_rng(seed)
    S = np.round(rng.normal(0.0, 0.05, (T, N)), 2)
    S[rng.random((T, N)) < 0.2] = np.nan
    gid = rng.integers(-1, 5, (T, N)).astype(np.int16)   # -1 and 4 are out of range for 4 groups
    return S, gid


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("pct", [False, True])
def test_row_ranks_equal_pandas(method, pct):
    S, _ = _rows(1)
    R, NVG = RR.xs_rank(S, None, 1, method, pct)
    want = pd.DataFrame(S).rank(axis=1, method=method, pct=pct).to_numpy()
    assert (~np.isnan(want)).mean() > 0.5
    assert bits_equal(R, want)
    assert np.array_equal(NVG[:, 0], (~np.isnan(S)).sum(axis=1))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("pct", [False, True])
def test_grouped_ranks_equal_pandas_groupby(method, pct):
    S, gid = _rows(2)
    T, N = S.shape
    R, NVG = RR.xs_rank(S, gid, 4, method, pct)
    long = pd.DataFrame({"date": np.repeat(np.arange(T), N), "group": gid.ravel().astype(np.int64),
                         "v": S.ravel()})
    has = ((long["group"] >= 0) & (long["group"] < 4)).to_numpy()
    want = np.full(T * N, np.nan)
    want[has] = long[has].groupby(["date", "group"])["v"].rank(method=method, pct=pct).to_numpy()
    assert (~np.isnan(want)).mean() > 0.4
    assert bits_equal(R, want.reshape(T, N))
    assert NVG.sum() == (~np.isnan(want)).sum()


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("pct", [0, 1])
def test_ranks_equal_the_fixture(golden, method, pct):
    """The pin: pandas' recorded output, so it holds wherever the tests run."""
    S, gid = golden["row_S"], golden["row_gid"]
    assert bits_equal(RR.xs_rank(S, None, 1, method, bool(pct))[0], golden[f"row_{method}_{pct}"])
    assert bits_equal(RR.xs_rank(S, gid, 4, method, bool(pct))[0], golden[f"grp_{method}_{pct}"])
    off, v = golden["xs_offsets"], golden["xs_values"]
    want = golden[f"xs_{method}_{pct}"]
    for c in range(len(off) - 1):
        sl = slice(off[c], off[c + 1])
        assert bits_equal(RR.rank_values(v[sl], method, bool(pct)), want[sl]), c
    assert (np.signbit(v) & (v == 0.0)).any() and ((~np.signbit(v)) & (v == 0.0)).any()


def _ic_cases(golden):
    off = golden["ic_offsets"]
    for c in range(len(off) - 1):
        sl = slice(off[c], off[c + 1])
        yield c, golden["ic_S"][sl][None], golden["ic_Y"][sl][None]


def test_ic_equals_the_fixture(golden):
    n_def = 0
    for c, s, y in _ic_cases(golden):
        RIC, PIC, NOBS = RR.rank_ic(s, y, 0, 2)
        assert NOBS[0] == golden["ic_n"][c] >= 2
        for got, key in ((RIC[0], "ic_spearman"), (RIC[0], "ic_spearman_pd"), (PIC[0], "ic_pearson")):
            want = golden[key][c]
            assert math.isnan(got) == math.isnan(want), (c, key)
            if not math.isnan(want):
                assert abs(got - want) <= TOL, (c, key, got, want)
        n_def += not math.isnan(RIC[0])
    assert n_def >= 50


def test_ic_equals_scipy_and_pandas_live(golden):
    stats = pytest.importorskip("scipy.stats")
    worst = 0.0
    for c, s, y in _ic_cases(golden):
        ok = ~np.isnan(s[0]) & ~np.isnan(y[0])
        RIC, PIC, _ = RR.rank_ic(s, y, 0, 2)
        sp = float(stats.spearmanr(s[0, ok], y[0, ok])[0])
        pdv = float(pd.Series(s[0]).corr(pd.Series(y[0]), method="spearman"))
        pe = float(np.corrcoef(s[0, ok], y[0, ok])[0, 1])
        for got, want in ((RIC[0], sp), (RIC[0], pdv), (PIC[0], pe)):
            assert math.isnan(got) == math.isnan(want), c
            if not math.isnan(want):
                worst = max(worst, abs(got - want))
    print(f"worst |IC - scipy / pandas / corrcoef| = {worst:.2e}")
    assert worst <= TOL


def test_ranks_are_inside_the_joint_set():
    """I3: an asset whose Y is NaN does not count in S's ranks."""
    s = np.array([[1.0, 2.0, 3.0, 4.0, 100.0]])
    y = np.array([[4.0, 3.0, 2.0, 1.0, np.nan]])
    RIC, PIC, NOBS = RR.rank_ic(s, y, 0, 2)
    assert NOBS[0] == 4 and RIC[0] == -1.0 and abs(PIC[0] + 1.0) <= 1e-15


def test_degenerate_rows():
    nan = np.nan
    S = np.array([[nan, nan, nan, nan],
                  [nan, 0.5, nan, nan],
                  [0.25, 0.25, 0.25, 0.25],
                  [0.0, -0.0, 1.0, -1.0]])
    for pct in (False, True):
        R, NVG = RR.xs_rank(S, None, 1, "average", pct)
        assert np.isnan(R[0]).all() and NVG[:, 0].tolist() == [0, 1, 4, 4]
        assert R[1, 1] == 1.0 and np.isnan(R[1, [0, 2, 3]]).all()      # n = 1: rank 1.0, pct 1.0
        d = 4.0 if pct else 1.0
        assert R[2].tolist() == [2.5 / d] * 4                          # all equal: (n + 1) / 2
        assert R[3].tolist() == [2.5 / d, 2.5 / d, 4.0 / d, 1.0 / d]   # -0.0 ties 0.0
    assert RR.xs_rank(S, None, 1, "min")[0][3].tolist() == [2.0, 2.0, 4.0, 1.0]
    assert RR.xs_rank(S, None, 1, "max")[0][3].tolist() == [3.0, 3.0, 4.0, 1.0]
    # the IC of an all-equal signal is NaN; so is a month under min_obs; n == min_obs is defined
    Y = np.array([[0.1, 0.2, 0.3, 0.4]] * 4)
    RIC, PIC, NOBS = RR.rank_ic(S, Y, 0, 4)
    assert NOBS.tolist() == [0, 1, 4, 4] and np.isnan(RIC[:3]).all() and np.isnan(PIC[:3]).all()
    assert not math.isnan(RIC[3]) and not math.isnan(PIC[3])
    RIC, PIC, NOBS = RR.rank_ic(S, Y, 0, 5)                            # n == min_obs - 1
    assert NOBS.tolist() == [0, 1, 4, 4] and np.isnan(RIC).all() and np.isnan(PIC).all()
    RIC, PIC, NOBS = RR.rank_ic(S, Y, 4, 2)                            # lead >= T_m
    assert NOBS.tolist() == [0] * 4 and np.isnan(RIC).all() and np.isnan(PIC).all()
    RIC, _, NOBS = RR.rank_ic(S, Y, 1, 2)                              # row 2 pairs with Y[3]
    assert NOBS.tolist() == [0, 1, 4, 0] and np.isnan(RIC).all()


# ------------------------------------------------------------------------------ C boundary
def _header():
    return (ROOT / "include" / "csmom.h").read_text()


@pytest.mark.parametrize("name,nparams", [("csm_xs_rank", 11), ("csm_rank_ic", 10)])
def test_header_declares(name, nparams):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} is not declared in include/csmom.h"
    assert len([p for p in m.group(1).split(",") if p.strip()]) == nparams


def test_abi_version_unchanged():
    assert re.search(r"#define\s+CSM_ABI_VERSION\s+3\b", _header())


def test_lib_lists_both():
    import csmom
    from csmom import _lib
    assert len(_lib.SIGNATURES["csm_xs_rank"][1]) == 11
    assert len(_lib.SIGNATURES["csm_rank_ic"][1]) == 10
    assert {"csm_xs_rank", "csm_rank_ic"} <= set(_lib.EXPORTS)
    assert callable(csmom.information_coefficient)
    for name in ("xs_rank", "rank_ic", "ic_decay"):
        assert callable(getattr(csmom.Engine, name))


def test_ic_stats_host_summary():
    from csmom.ic import ic_stats
    x = np.array([0.1, np.nan, -0.05, 0.2, 0.0])
    v = x[~np.isnan(x)]
    icir, hit = ic_stats(x)
    assert icir == v.mean() / v.std(ddof=1) and hit == 0.5
    assert all(math.isnan(k) for k in ic_stats(np.array([np.nan])))
