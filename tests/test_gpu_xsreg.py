"""GPU: csm_xs_regress / csm_newey_west / Engine.fama_macbeth / csmom.fama_macbeth (rules R1..R6 in
DESIGN.md 7) against the NumPy restatement in tests/xsreg_ref.py.

Bars.  Every step of R1..R6 has a stated order and ends in correctly rounded operations, and the
restatement reproduces R1's order (lanes, wave tree, waves, slices), so everything is bit for bit
(conftest.bits_equal; NOBS and NT exact).  A mismatch is a bug in one of the two sides, not a
tolerance to widen.

Coverage: in every case that is not an edge case by construction at least half the months have a
defined GAMMA row (asserted), so nothing passes on NaNs; tests/test_xsreg_ref.py pins the counts
(36 of 60 months on the real signals at N >= 63, 35 at N = 5, 0 at N = 1, 9 of 14 on the wide
panel).
"""
import numpy as np
import pandas as pd
import pytest
import torch

import market_ref as MR
import xsreg_ref as XR
from conftest import bits_equal

pytestmark = pytest.mark.gpu
_DEV = {}


def _up(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _raw(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else t.dtype)


def _same_bits(a, b):
    return torch.equal(_raw(a), _raw(b))


def _dev(key, arrays):
    """Device copies of a list of host arrays, uploaded once per key."""
    if key not in _DEV:
        _DEV[key] = [_up(a) for a in arrays]
    return _DEV[key]


def _check(engine, key, Y, S, W=None, half=True, **kw):
    """engine.xs_regress against the restatement, bit for bit -> (out, ref)."""
    ref = XR.xs_regress(Y, S, W, **kw)
    d = _dev(key, [Y, *S])
    out = engine.xs_regress(d[0], d[1:], None if W is None else _up(W), **kw)
    assert out.NOBS.dtype == torch.int32
    assert np.array_equal(out.NOBS.cpu().numpy(), ref["NOBS"]), key
    assert bits_equal(out.GAMMA.cpu().numpy(), ref["GAMMA"]), key
    assert bits_equal(out.R2.cpu().numpy(), ref["R2"]), key
    assert out.GAMMA.shape == (Y.shape[0], len(S) + 1)
    defined = ~np.isnan(ref["GAMMA"]).any(axis=1)
    assert np.array_equal(defined, ~np.isnan(ref["GAMMA"][:, 0]))
    if half:
        assert 2 * int(defined.sum()) >= Y.shape[0], (key, int(defined.sum()))
    return out, ref


def _normal(K, N=257):
    """Y of the real signals at N with K seeded normal regressors with holes."""
    return XR.real_inputs(N)["Y"], XR.normal_panel(60, N, K, seed=40 + K)


# ------------------------------------------------------------------------ csm_xs_regress
@pytest.mark.parametrize("N", [1, 5, 63, 64, 65, 257, 2048, 2049, 4500])
def test_width(engine, N):
    d = XR.real_inputs(N)
    _, ref = _check(engine, ("real", N), d["Y"], d["S"], half=N > 1)
    if N == 1:      # no month can have K + 2 observations
        assert np.isnan(ref["GAMMA"]).all() and (ref["NOBS"] <= 1).all()


def test_wide(engine):
    w = XR.wide_inputs()
    assert w["Y"].shape == (14, 20001)       # ten slices
    _, ref = _check(engine, "wide", w["Y"], w["S"])
    assert (ref["NOBS"][~np.isnan(ref["R2"])] >= 10000).all()
    _check(engine, "wide", w["Y"], w["S"], standardize=True, ridge=5.0)


@pytest.mark.parametrize("K", [1, 3, 8])
def test_k(engine, K):
    Y, S = _normal(K)
    _check(engine, ("normal", K), Y, S)
    _check(engine, ("normal", K), Y, S, standardize=True, ridge=5.0)


def test_bad_arguments_are_refused(engine):
    import csmom
    from csmom.engine import _ptr
    Y, S = _normal(8)
    d = _dev(("normal", 8), [Y, *S])
    for kw in (dict(signals=d[1:] + d[1:2]), dict(signals=[]), dict(signals=d[1:4], min_obs=4),
               dict(signals=d[1:4], ridge=-1.0), dict(signals=d[1:4], ridge=float("nan"))):
        with pytest.raises(csmom.CsmError) as e:
            engine.xs_regress(d[0], **kw)
        assert e.value.status == -1   # CSM_E_INVAL
    import ctypes
    gamma = torch.full((60, 2), 12345.0, dtype=torch.float64, device="cuda:0")
    one = (ctypes.c_void_p * 1)(d[1].data_ptr())
    for args in ((None, one, 1, None, 60, 257, 0, 0.0, 3, _ptr(gamma), None, None),
                 (_ptr(d[0]), None, 1, None, 60, 257, 0, 0.0, 3, _ptr(gamma), None, None),
                 (_ptr(d[0]), one, 1, None, 60, 257, 0, 0.0, 3, None, None, None),
                 (_ptr(d[0]), one, 1, None, 0, 257, 0, 0.0, 3, _ptr(gamma), None, None),
                 (_ptr(d[0]), one, 1, None, 60, 0, 0, 0.0, 3, _ptr(gamma), None, None),
                 (_ptr(d[0]), (ctypes.c_void_p * 1)(None), 1, None, 60, 257, 0, 0.0, 3,
                  _ptr(gamma), None, None)):
        with pytest.raises(csmom.CsmError) as e:
            engine._call("csm_xs_regress", *args)
        assert e.value.status == -1
    torch.cuda.synchronize()
    assert (gamma == 12345.0).all()      # nothing was launched
    with pytest.raises(ValueError):      # a non-contiguous view
        engine.xs_regress(d[0], [d[1].t().contiguous().t()])
    for args in ((None, 60, 2, 2, 1), (_ptr(gamma), 0, 2, 2, 1), (_ptr(gamma), 60, 2, 1, 1),
                 (_ptr(gamma), 60, 2, 2, -1)):
        with pytest.raises(csmom.CsmError) as e:
            engine._call("csm_newey_west", *args, _ptr(gamma), None, None, None)
        assert e.value.status == -1


def test_min_obs(engine):
    d = XR.real_inputs(5)
    base = XR.xs_regress(d["Y"], d["S"])
    out, ref = _check(engine, ("real", 5), d["Y"], d["S"], half=False, min_obs=5)
    defined = ~np.isnan(ref["GAMMA"][:, 0])
    assert np.array_equal(defined, ~np.isnan(base["GAMMA"][:, 0]) & (base["NOBS"] == 5))
    assert defined.sum() >= 5
    below = (base["NOBS"] < 5) & (base["NOBS"] > 0)
    assert below.sum() >= 1                     # a month that keeps its true NOBS and nothing else
    got = out.GAMMA.cpu().numpy()
    assert np.isnan(got[below]).all() and np.isnan(out.R2.cpu().numpy()[below]).all()
    assert np.array_equal(out.NOBS.cpu().numpy()[below], base["NOBS"][below])
    # a wider row, the bar above about half of the months' counts
    d = XR.real_inputs(63)
    base = XR.xs_regress(d["Y"], d["S"])
    k = int(np.median(base["NOBS"][base["NOBS"] > 0])) + 1
    out, ref = _check(engine, ("real", 63), d["Y"], d["S"], half=False, min_obs=k)
    defined = ~np.isnan(ref["GAMMA"][:, 0])
    assert np.array_equal(defined, ~np.isnan(base["GAMMA"][:, 0]) & (base["NOBS"] >= k))
    below = (base["NOBS"] < k) & ~np.isnan(base["GAMMA"][:, 0])
    assert defined.sum() >= 5 and below.sum() >= 5
    assert np.isnan(out.GAMMA.cpu().numpy()[below]).all()
    assert bits_equal(out.GAMMA.cpu().numpy()[defined], base["GAMMA"][defined])


def test_degenerate_regressors(engine):
    d = XR.real_inputs(257)
    base = XR.xs_regress(d["Y"], d["S"])
    S = [s.copy() for s in d["S"]]
    S[1][40] = np.where(np.isnan(S[1][40]), np.nan, 0.25)      # C_11 = 0 in month 40
    out, ref = _check(engine, "constant", d["Y"], S)
    assert np.isnan(ref["GAMMA"][40]).all() and not np.isnan(base["GAMMA"][40]).any()
    keep = np.arange(60) != 40
    assert bits_equal(out.GAMMA.cpu().numpy()[keep], base["GAMMA"][keep])
    assert ref["NOBS"][40] == base["NOBS"][40] > 100
    # the same tensor twice, and an affine copy: the pivot rule leaves no month
    dev = _dev(("real", 257), [d["Y"], *d["S"]])
    twice = engine.xs_regress(dev[0], [dev[1], dev[2], dev[3], dev[1]])
    assert torch.isnan(twice.GAMMA).all() and torch.isnan(twice.R2).all()
    assert np.array_equal(twice.NOBS.cpu().numpy(), base["NOBS"])
    for key, extra in (("twice", d["S"][0]), ("affine", 2.0 * d["S"][0] + 1.0)):
        _, ref = _check(engine, key, d["Y"], d["S"] + [extra], half=False)
        assert np.isnan(ref["GAMMA"]).all()
    # enough ridge makes the copy solvable again
    _check(engine, "twice", d["Y"], d["S"] + [d["S"][0]], standardize=True, ridge=5.0)


def test_weights(engine):
    d = XR.real_inputs(257)
    rng = np.random.default_rng(1157)
    W = rng.uniform(0.5, 2.0, size=(60, 257))
    r = rng.random((60, 257))
    W[r < 0.03] = np.nan
    W[(r >= 0.03) & (r < 0.06)] = 0.0
    W[(r >= 0.06) & (r < 0.09)] = -1.0
    base = XR.xs_regress(d["Y"], d["S"])
    for std in (False, True):
        _, ref = _check(engine, ("real", 257), d["Y"], d["S"], W=W, standardize=std)
        live = base["NOBS"] > 0
        assert (ref["NOBS"][live] < base["NOBS"][live]).all()     # those cells are excluded
        assert not bits_equal(ref["GAMMA"], XR.xs_regress(d["Y"], d["S"],
                                                          standardize=std)["GAMMA"])
    dev = _dev(("real", 257), [d["Y"], *d["S"]])
    ones = engine.xs_regress(dev[0], dev[1:], torch.ones_like(dev[0]))
    none = engine.xs_regress(dev[0], dev[1:])
    for k in ("GAMMA", "R2", "NOBS"):
        assert _same_bits(getattr(ones, k), getattr(none, k)), k


@pytest.mark.parametrize("standardize", [False, True])
@pytest.mark.parametrize("ridge", [0.0, 5.0])
def test_options(engine, standardize, ridge):
    for N in (65, 2049):
        d = XR.real_inputs(N)
        out, ref = _check(engine, ("real", N), d["Y"], d["S"], standardize=standardize,
                          ridge=ridge)
        if standardize:     # the intercept is the month's mean of Y
            assert bits_equal(out.GAMMA.cpu().numpy()[:, 0],
                              np.where(np.isnan(ref["R2"]), np.nan, ref["MY"]))


def test_layout(engine):
    from csmom.engine import _ptr
    import ctypes
    d = XR.real_inputs(257)
    dev = _dev(("real", 257), [d["Y"], *d["S"]])
    base = engine.xs_regress(dev[0], dev[1:])
    views = []
    for t in dev:       # an odd N through a base address 8 B past a 16-B boundary
        flat = torch.empty(t.numel() + 1, dtype=torch.float64, device="cuda:0")
        v = flat[1:].view(t.shape)
        v.copy_(t)
        assert t.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 8 and v.is_contiguous()
        views.append(v)
    for out in (engine.xs_regress(views[0], views[1:]), engine.xs_regress(dev[0], dev[1:])):
        for k in ("GAMMA", "R2", "NOBS"):
            assert _same_bits(getattr(out, k), getattr(base, k)), k
    # R2 and NOBS are optional at the C boundary
    gamma = torch.empty_like(base.GAMMA)
    ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in dev[1:]])
    engine._call("csm_xs_regress", _ptr(dev[0]), ptrs, 3, None, 60, 257, 0, 0.0, 5, _ptr(gamma),
                 None, None)
    assert _same_bits(gamma, base.GAMMA)


# ------------------------------------------------------------------------ csm_newey_west
def _series():
    rng = np.random.default_rng(21)
    G = rng.normal(0.01, 0.05, size=(60, 5))
    for t in range(1, 60):
        G[t] += 0.4 * (G[t - 1] - 0.01)
    G[[3, 17, 18, 44]] = np.nan
    G[:, 2] = np.nan
    return G


def _check_nw(engine, G, lags):
    ref = XR.newey_west(G, lags)
    out = engine.newey_west(_up(G), lags)
    assert out.NT.dtype == torch.int32
    assert np.array_equal(out.NT.cpu().numpy(), ref["NT"])
    for k in ("MEAN", "SE", "T"):
        assert bits_equal(getattr(out, k).cpu().numpy(), ref[k]), (k, lags)
    return out, ref


@pytest.mark.parametrize("lags", [0, 1, 4])
def test_newey_west(engine, lags):
    G = _series()
    keep = [0, 1, 2, 5, 6][:lags + 1]            # column 4: n = lags + 1
    col = np.full(60, np.nan)
    col[keep] = G[keep, 4]
    G[:, 4] = col
    out, ref = _check_nw(engine, G, lags)
    assert (ref["NT"] == [56, 56, 0, 56, lags + 1]).all()
    assert not np.isnan(ref["T"][[0, 1, 3]]).any()
    assert np.isnan(ref["MEAN"][2]) and np.isnan(ref["T"][2])
    assert not np.isnan(ref["MEAN"][4]) and np.isnan(ref["SE"][4]) and np.isnan(ref["T"][4])
    # a [T] vector
    one, r1 = _check_nw(engine, np.ascontiguousarray(G[:, 1]), lags)
    assert one.MEAN.dim() == 0 and _same_bits(one.T, out.T[1]) and int(one.NT) == 56


def test_newey_west_of_a_long_series(engine):
    """More entries than a workgroup stages in LDS (8000): the same rule through the workspace."""
    rng = np.random.default_rng(5)
    G = rng.normal(0.0005, 0.01, size=(8500, 2))
    G[rng.random(G.shape) < 0.02] = np.nan
    _, ref = _check_nw(engine, G, 2)
    assert (ref["NT"] > 8000).all() and not np.isnan(ref["T"]).any()


def test_newey_west_of_the_decile_series(engine):
    host = MR.panel(257)
    res = engine.run(_up(host["P"]), _up(host["ms"]), J=12, skip=1, n_bins=10)
    for G in (res.EW, res.LS):
        ref = XR.newey_west(G.cpu().numpy(), XR.default_lags(60))
        out = engine.newey_west(G)          # default lags: floor(4 (60 / 100)^(2/9)) = 3
        for k in ("MEAN", "SE", "T"):
            assert bits_equal(getattr(out, k).cpu().numpy(), ref[k]), k
        assert np.array_equal(out.NT.cpu().numpy(), ref["NT"])
        assert (np.asarray(ref["NT"]) >= 30).all() and not np.isnan(ref["T"]).any()


# -------------------------------------------------------------------------- fama_macbeth
def test_engine_fama_macbeth_is_the_two_calls(engine):
    d = XR.real_inputs(257)
    dev = _dev(("real", 257), [d["Y"], *d["S"]])
    fm = engine.fama_macbeth(dev[0], dev[1:])
    r = engine.xs_regress(dev[0], dev[1:], standardize=True)
    nw = engine.newey_west(r.GAMMA, 3)
    assert fm.lags == 3
    for k in ("GAMMA", "R2", "NOBS"):
        assert _same_bits(getattr(fm, k), getattr(r, k)), k
    for k in ("MEAN", "SE", "T", "NT"):
        assert _same_bits(getattr(fm, k), getattr(nw, k)), k
    assert _same_bits(fm.R2_MEAN, engine.newey_west(r.R2, 3).MEAN)
    ref = XR.fama_macbeth(d["Y"], d["S"])
    for k in ("MEAN", "SE", "T"):
        assert bits_equal(getattr(fm, k).cpu().numpy(), ref["nw"][k]), k
        assert not np.isnan(ref["nw"][k]).any()
    assert (ref["nw"]["NT"] == 36).all() and float(fm.R2_MEAN) == float(ref["R2_MEAN"])
    fm2 = engine.fama_macbeth(dev[0], dev[1:], standardize=False, ridge=0.5, lags=1)
    ref2 = XR.fama_macbeth(d["Y"], d["S"], standardize=False, ridge=0.5, lags=1)
    assert bits_equal(fm2.T.cpu().numpy(), ref2["nw"]["T"]) and fm2.lags == 1


def test_fama_macbeth_from_a_daily_frame(engine):
    import csmom
    from csmom.regress import build_signals
    host = MR.panel(63)
    P = host["P"]
    days = pd.bdate_range("2000-01-03", periods=P.shape[0])
    pres = (P.view(np.uint64) & np.uint64(0x7FF7FFFFFFFFFFFF)) != np.uint64(0x7FF4000000000001)
    dd, aa = np.nonzero(pres)
    df = pd.DataFrame({"date": days[dd], "ticker": np.array([f"T{a:03d}" for a in range(63)])[aa],
                       "adj_close": P[dd, aa]})
    names = ("mom", "high52", "beta", "ivol", "rev")
    res = csmom.fama_macbeth(df, signals=names)
    panel = csmom.from_long(df)
    assert np.array_equal(panel.month_start, host["ms"]) and panel.P.shape == P.shape
    assert res.gammas.index.equals(pd.DatetimeIndex(panel.month_end)) and len(res.gammas) == 60
    assert list(res.table.index) == ["const", *names] == list(res.gammas.columns)
    assert list(res.table.columns) == ["mean", "se", "t", "months"]
    # the restatement on the engine's own signals
    S, X = build_signals(engine, _up(P), _up(host["ms"]), names)
    Xh = X.cpu().numpy()
    assert bits_equal(Xh, MR.month_returns(host["PM"]))
    Y = np.vstack([Xh[1:], np.full((1, 63), np.nan)])
    ref = XR.fama_macbeth(Y, [s.cpu().numpy() for s in S])
    assert ref["lags"] == res.lags == 3
    assert bits_equal(res.gammas.to_numpy(), ref["GAMMA"])
    assert bits_equal(res.r2.to_numpy(), ref["R2"])
    assert np.array_equal(res.nobs.to_numpy(), ref["NOBS"])
    for col, k in (("mean", "MEAN"), ("se", "SE"), ("t", "T")):
        assert bits_equal(res.table[col].to_numpy(), ref["nw"][k]), col
        assert not np.isnan(ref["nw"][k]).any()
    assert np.array_equal(res.table["months"].to_numpy(), ref["nw"]["NT"])
    assert (ref["nw"]["NT"] >= 20).all() and res.r2_mean == float(ref["R2_MEAN"])
    with pytest.raises(ValueError):
        csmom.fama_macbeth(df, signals=("mom", "alpha"))
