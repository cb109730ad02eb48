"""GPU: csm_xs_rank / csm_rank_ic and what is built on them (rules I1..I6 in DESIGN.md 7) against
the NumPy restatement in tests/rank_ref.py, which the CPU tests pin to pandas and scipy.

Inputs are made as test_gpu_groups.make_case makes them: normal draws rounded to cents (ties),
20 % NaN, 1 % ABSENT, 5 % ids out of range; Y is correlated with S, 10 % NaN, rounded to cents in
every other case (ties on both sides).

Bars.  RANK, NVG, RIC and NOBS are exact: ranks are half-integers or one quotient, and the
Spearman sums are integers (I4), so RIC is three conversions, one product, one root and one
quotient, each correctly rounded, on both sides.  PIC is within 1e-10 absolute (|IC| <= 1) of the
restatement's fsum.  Two calls give the same bits, and so do the tuned and the untuned
small-segment cap.

Every parametrised IC case asserts that the reference IC is defined in at least half of the months
with t + lead < T_m, so nothing passes on NaNs; the named degenerate cases assert exactly their
degenerate output.
"""
import ctypes

import numpy as np
import pytest
import torch

import rank_ref as RR
from conftest import bits_equal
from oracle import csmom_oracle as O

pytestmark = pytest.mark.gpu

METHODS = ("average", "min", "max")
TOL = 1e-10


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def make_case(T_m, N, G, static, seed, weights=None, nan=0.2, bad=0.05):
    """S [T_m][N], GID [N] or [T_m][N] int16.  weights: the groups' shares of the assets."""
    rng = np.random.default_rng(seed)
    S = np.round(rng.normal(0.0, 0.1, (T_m, N)), 2)
    S[rng.random((T_m, N)) < nan] = np.nan
    if nan > 0:
        S[rng.random((T_m, N)) < 0.01] = O.absent_scalar()
    shape = (N,) if static else (T_m, N)
    p = None if weights is None else np.asarray(weights, dtype=np.float64) / np.sum(weights)
    gid = rng.choice(G, size=shape, p=p).astype(np.int16)
    out = rng.random(shape) < bad
    gid[out] = np.where(rng.random(shape) < 0.5, -1 - rng.integers(0, 3, shape),
                        G + rng.integers(0, 3, shape))[out].astype(np.int16)
    return S, gid


def make_y(S, seed, cents):
    rng = np.random.default_rng(seed)
    Y = 0.3 * np.where(np.isnan(S), 0.0, S) + rng.normal(0.0, 0.08, S.shape)
    if cents:
        Y = np.round(Y, 2)
    Y[rng.random(S.shape) < 0.1] = np.nan
    return Y


def check_ranks(engine, S, gid, G):
    """Every method and both pct against the restatement; returns the device outputs."""
    Sd, Gd = _up(S), (None if gid is None else _up(gid))
    outs = []
    for method in METHODS:
        for pct in (False, True):
            want, nvg = RR.xs_rank(S, gid, G, method, pct)
            R, NVG = engine.xs_rank(Sd, Gd, G, method, pct, with_nvg=True)
            assert bits_equal(R.cpu().numpy(), want), (method, pct)
            assert np.array_equal(NVG.cpu().numpy(), nvg)
            assert _bits(R, engine.xs_rank(Sd, Gd, G, method, pct))     # two calls, the same bits
            outs.append(R)
    return outs, nvg


# (T_m, N, n_groups, static ids, the groups' shares, NaN share)
RANK_CASES = [
    (3, 63, 1, True, None, 0.2),
    (3, 64, 2, False, None, 0.2),
    (1, 65, 2, True, [0.9, 0.1], 0.2),
    (3, 257, 11, False, None, 0.2),
    (3, 1000, 49, True, None, 0.2),
    (2, 4099, 256, False, None, 0.2),
    (2, 4099, 1, True, None, 0.0),       # one segment just past the LDS cap
    (1, 8200, 1, True, None, 0.0),       # three tiles: the merges wider than a tile run
]


@pytest.mark.parametrize("T_m,N,G,static,weights,nan", RANK_CASES)
def test_xs_rank_vs_ref(engine, T_m, N, G, static, weights, nan):
    S, gid = make_case(T_m, N, G, static, seed=N + G, weights=weights, nan=nan,
                       bad=0.05 if nan else 0.0)
    _, nvg = check_ranks(engine, S, gid, G)
    assert nvg.sum() >= 0.5 * T_m * N
    if nan == 0.0:
        assert nvg.min() == N > 4096


def test_no_gid_equals_a_row_of_zeros(engine):
    S, _ = make_case(3, 1000, 1, True, seed=4)
    Sd = _up(S)
    zeros = torch.zeros(1000, dtype=torch.int16, device=Sd.device)
    for method in METHODS:
        a = engine.xs_rank(Sd, None, 1, method, True)
        assert _bits(a, engine.xs_rank(Sd, zeros, 1, method, True))
        assert bits_equal(a.cpu().numpy(), RR.xs_rank(S, None, 1, method, True)[0])
    assert (~torch.isnan(a)).float().mean().item() > 0.5


def test_small_cap_knob_moves_segments_not_results(engine):
    """gdec_small_cap = 64: segments and months of more than 64 values take the tiled kernels
    (tiles of 128).  Same bits as untuned, for the ranks and for the IC."""
    T_m, N, G = 3, 1000, 4
    S, _ = make_case(T_m, N, G, True, seed=3, nan=0.0, bad=0.0)
    gid = np.repeat(np.arange(4, dtype=np.int16), [300, 64, 65, 571])
    gid = gid[np.random.default_rng(1).permutation(N)]
    Y = make_y(S, 5, True)
    base, nvg = check_ranks(engine, S, gid, G)
    assert nvg[0].tolist() == [300, 64, 65, 571]
    ic0 = check_ic(engine, S, Y, 1, 10)
    assert engine.lib.csm_tune(b"gdec_small_cap", 64) == 0
    try:
        tuned, _ = check_ranks(engine, S, gid, G)
        ic1 = check_ic(engine, S, Y, 1, 10)
    finally:
        assert engine.lib.csm_tune(b"gdec_small_cap", 4096) == 0
    for a, b in zip(base, tuned):
        assert _bits(a, b)
    for k in ("RIC", "PIC", "NOBS"):
        assert _bits(getattr(ic0, k), getattr(ic1, k))


# ---------------------------------------------------------------------------------- rank_ic
def check_ic(engine, S, Y, lead, min_obs, need_defined=True):
    T_m = S.shape[0]
    RIC, PIC, NOBS = RR.rank_ic(S, Y, lead, min_obs)
    live = max(T_m - lead, 0)
    if need_defined:
        assert (~np.isnan(RIC)).sum() >= 0.5 * live > 0 and (~np.isnan(PIC)).sum() >= 0.5 * live
    Sd, Yd = _up(S), _up(Y)
    o = engine.rank_ic(Sd, Yd, lead, min_obs)
    torch.cuda.synchronize()
    assert np.array_equal(o.NOBS.cpu().numpy(), NOBS)
    assert bits_equal(o.RIC.cpu().numpy(), RIC), (o.RIC.cpu().numpy(), RIC)
    pic = o.PIC.cpu().numpy()
    assert np.array_equal(np.isnan(pic), np.isnan(PIC))
    m = ~np.isnan(PIC)
    err = float(np.abs(pic[m] - PIC[m]).max()) if m.any() else 0.0
    print(f"rank_ic {S.shape} lead={lead}: max |PIC - ref| = {err:.2e}")
    assert err <= TOL
    again = engine.rank_ic(Sd, Yd, lead, min_obs)
    for k in ("RIC", "PIC", "NOBS"):
        assert _bits(getattr(o, k), getattr(again, k))
    only = engine.rank_ic(Sd, Yd, lead, min_obs, pearson=False)
    assert only.PIC is None and _bits(only.RIC, o.RIC) and _bits(only.NOBS, o.NOBS)
    return o


@pytest.mark.parametrize("lead", [0, 1, 3])
@pytest.mark.parametrize("N", [63, 64, 65, 257, 1000, 4099, 8200])
def test_rank_ic_vs_ref(engine, N, lead):
    S, _ = make_case(4, N, 1, True, seed=N + lead)
    Y = make_y(S, 7 * N + lead, cents=(N + lead) % 2 == 0)
    o = check_ic(engine, S, Y, lead, 10)
    if N == 8200:
        assert o.NOBS[: 4 - lead].min().item() > 4096     # past the LDS cap


def test_rank_ic_lead_past_the_panel(engine):
    S, _ = make_case(4, 257, 1, True, seed=2)
    o = check_ic(engine, S, make_y(S, 3, True), 4, 10, need_defined=False)
    assert (o.NOBS == 0).all() and torch.isnan(o.RIC).all() and torch.isnan(o.PIC).all()


def test_degenerate_rows(engine):
    nan = np.nan
    S = np.array([[nan, nan, nan, nan],
                  [nan, 0.5, nan, nan],
                  [0.25, 0.25, 0.25, 0.25],
                  [0.0, -0.0, 1.0, -1.0]])
    Sd = _up(S)
    for pct in (False, True):
        R, NVG = engine.xs_rank(Sd, pct=pct, with_nvg=True)
        R = R.cpu().numpy()
        d = 4.0 if pct else 1.0
        assert np.isnan(R[0]).all() and NVG[:, 0].tolist() == [0, 1, 4, 4]
        assert R[1, 1] == 1.0 and np.isnan(R[1, [0, 2, 3]]).all()
        assert R[2].tolist() == [2.5 / d] * 4
        assert R[3].tolist() == [2.5 / d, 2.5 / d, 4.0 / d, 1.0 / d]
    assert engine.xs_rank(Sd, method="min")[3].tolist() == [2.0, 2.0, 4.0, 1.0]
    assert engine.xs_rank(Sd, method="max")[3].tolist() == [3.0, 3.0, 4.0, 1.0]
    Y = np.array([[0.1, 0.2, 0.3, 0.4]] * 4)
    Yd = _up(Y)
    o = engine.rank_ic(Sd, Yd, 0, 4)                       # n == min_obs is defined
    want = RR.rank_ic(S, Y, 0, 4)
    assert o.NOBS.tolist() == [0, 1, 4, 4]
    assert torch.isnan(o.RIC[:3]).all() and torch.isnan(o.PIC[:3]).all()
    assert bits_equal(o.RIC.cpu().numpy(), want[0]) and not np.isnan(want[0][3])
    assert abs(o.PIC[3].item() - want[1][3]) <= TOL
    o = engine.rank_ic(Sd, Yd, 0, 5)                       # n == min_obs - 1
    assert o.NOBS.tolist() == [0, 1, 4, 4] and torch.isnan(o.RIC).all() and torch.isnan(o.PIC).all()
    o = engine.rank_ic(Sd, Yd, 4, 2)                       # lead >= T_m
    assert o.NOBS.tolist() == [0] * 4 and torch.isnan(o.RIC).all() and torch.isnan(o.PIC).all()
    o = engine.rank_ic(Sd, Yd, 1, 2)
    assert o.NOBS.tolist() == [0, 1, 4, 0] and torch.isnan(o.RIC).all()


def test_argument_checks(engine):
    S, gid = make_case(2, 64, 3, True, seed=1)
    Sd, Gd = _up(S), _up(gid)
    R = torch.empty_like(Sd)
    lib, p = engine.lib, lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def rank(S_=Sd, G_=Gd, g_ld=0, T_m=2, N=64, G=3, method=0, R_=R):
        st = lib.csm_xs_rank(engine.ctx, p(S_), p(G_), g_ld, T_m, N, G, method, 0, p(R_), None)
        return st, lib.csm_last_error(engine.ctx).decode()

    assert rank()[0] == 0 and rank(G_=None, G=1)[0] == 0
    for kw, word in ((dict(G_=None), "GID is NULL"), (dict(method=3), "method"),
                     (dict(method=-1), "method"), (dict(R_=None), "RANK"),
                     (dict(S_=None), "bad arguments"), (dict(G=0), "n_groups"),
                     (dict(G=257), "n_groups"), (dict(g_ld=7), "g_ld"), (dict(T_m=0), "bad arguments")):
        st, msg = rank(**kw)
        assert st == -1 and word in msg, (kw, st, msg)

    out = torch.empty(2, dtype=torch.float64, device=Sd.device)

    def ic(S_=Sd, Y_=Sd, T_m=2, N=64, lead=0, min_obs=2, RIC=out, PIC=out):
        st = lib.csm_rank_ic(engine.ctx, p(S_), p(Y_), T_m, N, lead, min_obs, p(RIC), p(PIC), None)
        return st, lib.csm_last_error(engine.ctx).decode()

    assert ic()[0] == 0 and ic(PIC=None)[0] == 0 and ic(RIC=None)[0] == 0
    for kw, word in ((dict(N=(1 << 20) + 1), "2^20"), (dict(min_obs=1), "min_obs"),
                     (dict(RIC=None, PIC=None), "both NULL"), (dict(S_=None), "bad arguments"),
                     (dict(Y_=None), "bad arguments"), (dict(lead=-1), "bad arguments"),
                     (dict(T_m=0), "bad arguments")):
        st, msg = ic(**kw)
        assert st == -1 and word in msg, (kw, st, msg)
    with pytest.raises(ValueError):
        engine.xs_rank(Sd, method="dense")


# --------------------------------------------------------------------------------- ic_decay
def test_ic_decay_is_the_stacked_calls(engine):
    S, _ = make_case(30, 257, 1, True, seed=8)
    X = make_y(S, 9, False)
    Sd, Xd = _up(S), _up(X)
    hs = (1, 2, 3, 6, 12)
    d = engine.ic_decay(Sd, Xd, hs, min_obs=10, lags=2)
    calls = [engine.rank_ic(Sd, Xd, h, 10) for h in hs]
    for k in ("RIC", "PIC", "NOBS"):
        assert _bits(getattr(d, k), torch.stack([getattr(c, k) for c in calls])), k
    nw = engine.newey_west(d.RIC.t().contiguous(), 2)
    for k in ("MEAN", "SE", "T", "NT"):
        assert _bits(getattr(d, k), getattr(nw, k)), k
    assert d.horizons == hs and d.lags == 2 and d.NT.tolist() == [30 - h for h in hs]
    assert not torch.isnan(d.T).any()
    for k, h in enumerate(hs):
        assert bits_equal(d.RIC[k].cpu().numpy(), RR.rank_ic(S, X, h, 10)[0])
    assert engine.ic_decay(Sd, Xd, (1,)).lags == engine.default_lags(30)


# ------------------------------------------------------------------------- from a daily frame
@pytest.fixture(scope="module")
def daily():
    import csmom
    from oracle.synth_np import make_panel, to_long
    panel = make_panel(40, 1300, seed=9, nan_day=0.01, absent_month=0.01, nan_month=0.01,
                       cents=True)
    df = to_long(panel)
    return df, csmom.from_long(df)


def test_information_coefficient_api(engine, daily):
    import csmom
    from csmom.regress import build_signals
    df, dense = daily
    names, hs = ("mom", "ivol"), (1, 3)
    res = csmom.information_coefficient(df, signals=names, horizons=hs, J=6, window=12,
                                        min_obs=10, device=0)
    S, X = build_signals(engine, _up(dense.P), _up(dense.month_start.astype(np.int64)), names,
                         6, 1, 12)
    Xh = X.cpu().numpy()
    assert res.ic.index.equals(pd_index(dense)) and len(res.ic) == dense.T_m >= 55
    assert list(res.table.index) == [(n, h) for n in names for h in hs] == list(res.ic.columns)
    assert list(res.table.columns) == ["mean", "se", "t", "icir", "hit", "months"]
    assert res.lags == engine.default_lags(dense.T_m)
    for n, s in zip(names, S):
        for h in hs:
            RIC, PIC, NOBS = RR.rank_ic(s.cpu().numpy(), Xh, h, 10)
            got = res.ic[(n, h)].to_numpy()
            assert (~np.isnan(RIC)).sum() >= 20
            assert bits_equal(got, RIC), (n, h)
            assert np.array_equal(res.nobs[(n, h)].to_numpy(), NOBS)
            pe = res.pearson[(n, h)].to_numpy()
            assert np.array_equal(np.isnan(pe), np.isnan(PIC))
            assert np.nanmax(np.abs(pe - PIC)) <= TOL
            v = got[~np.isnan(got)]
            row = res.table.loc[(n, h)]
            acc = 0.0
            for x in v:        # rule R6's mean: the sum in time order from 0.0
                acc += x
            assert row["mean"] == acc / len(v) and row["months"] == len(v)
            assert row["icir"] == v.mean() / v.std(ddof=1) and row["hit"] == (v > 0).mean()
            nw = engine.newey_west(_up(got), res.lags)
            assert row["se"] == nw.SE.item() and row["t"] == nw.T.item()
    assert csmom.information_coefficient(df.iloc[:0]) is None


def pd_index(dense):
    import pandas as pd
    return pd.DatetimeIndex(dense.month_end, name="date")


def test_fama_macbeth_rank_transform(engine, daily):
    import csmom
    from csmom.regress import build_signals
    df, dense = daily
    names = ("mom", "ivol")
    res = csmom.fama_macbeth(df, signals=names, J=6, window=12, transform="rank", device=0)
    S, X = build_signals(engine, _up(dense.P), _up(dense.month_start.astype(np.int64)), names,
                         6, 1, 12)
    ranked = [engine.xs_rank(s, pct=True) for s in S]
    for s, r in zip(S, ranked):
        assert bits_equal(r.cpu().numpy(), RR.xs_rank(s.cpu().numpy(), None, 1, "average", True)[0])
    Y = torch.cat([X[1:], torch.full_like(X[:1], float("nan"))])
    fm = engine.fama_macbeth(Y, ranked)
    assert (~torch.isnan(fm.GAMMA[:, 1])).sum().item() >= 20
    assert bits_equal(res.gammas.to_numpy(), fm.GAMMA.cpu().numpy())
    for col, k in (("mean", "MEAN"), ("se", "SE"), ("t", "T")):
        assert bits_equal(res.table[col].to_numpy(), getattr(fm, k).cpu().numpy()), col
    plain = csmom.fama_macbeth(df, signals=names, J=6, window=12, device=0)
    assert not bits_equal(plain.gammas.to_numpy(), res.gammas.to_numpy())
    with pytest.raises(ValueError):
        csmom.fama_macbeth(df, signals=names, transform="zscore")
