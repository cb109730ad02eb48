"""GPU: csm_daily_returns / csm_series_stats (rule E7) against the NumPy restatement in
tests/daily_ref.py, with the engine's own labels and next returns as members.

Bar: |DR_gpu - DR_ref| <= 1e-10 (1 + |DR_ref|), the same for DLS.  DR is a gross ratio minus 1;
the worst-case reordering error of a 20,000-term positive sum is 2 n eps ~ 4e-12 on the ratio,
and 1e-10 -- the project's EW / LS bar -- covers it with margin.  NaN positions and the member
counts are exact.  The statistics kernel is held to k_summary's bar, 1e-12 relative."""
import numpy as np
import pytest
import torch

import daily_ref as DRF
from conftest import bits_equal
from oracle import portfolio_oracle as PO
from oracle.synth_np import make_panel

pytestmark = pytest.mark.gpu
REL = 1e-10
T_DAYS = 782            # 36 whole business-day months of 19..23 rows from 2000-01-03
J, SKIP = 6, 1
_CACHE = {}


def _up(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _weights(shape, seed):
    """Formation weights with zeros and NaNs (either drops the member's weight)."""
    rng = np.random.default_rng(seed)
    W = rng.lognormal(0.0, 1.0, shape)
    u = rng.random(shape)
    W[u < 0.05] = 0.0
    W[u > 0.95] = np.nan
    return W


def _panel(engine, N, dense=False):
    """Host panel + the engine's labels / next returns for it (computed once per panel)."""
    key = (N, dense)
    if key not in _CACHE:
        if dense:
            pan = make_panel(N, T_DAYS, seed=100 + N, late=0, delist=0, nan_day=0, absent_month=0,
                             nan_month=0, with_volume=False)
        else:
            pan = make_panel(N, T_DAYS, seed=200 + N, late=0.2, delist=0.2, nan_day=0.01,
                             absent_month=0.01, nan_month=0.01, with_volume=False)
        P, ms = pan["P"], pan["month_start"]
        if not dense:   # NaN days at the start of some months: base and fill cross the boundary
            rng = np.random.default_rng(300 + N)
            for m in range(2, len(ms) - 1, 3):
                cols = rng.random(N) < 0.1
                P[ms[m]:ms[m] + 2, cols] = np.nan
        d = np.diff(ms)
        assert len(ms) - 1 == 36 and d.min() >= 19 and d.max() <= 23
        Pd, msd = _up(P), _up(ms)
        run = engine.run(Pd, msd, J=J, skip=SKIP, n_bins=10)
        _CACHE[key] = dict(P=P, ms=ms, Pd=Pd, msd=msd, L=run.L, NR=run.NR, M=run.M,
                           Lh=run.L.cpu().numpy(), NRh=run.NR.cpu().numpy(), ref={})
    return _CACHE[key]


def _ref(pan, n_bins, K, W, Lh=None, tag=None):
    key = (n_bins, K, tag)
    if key not in pan["ref"]:
        pan["ref"][key] = DRF.daily_returns(pan["P"], pan["ms"], pan["Lh"] if Lh is None else Lh,
                                            pan["NRh"], n_bins, K, W)
    return pan["ref"][key]


def _close(got, ref, what):
    g = got.cpu().numpy()
    assert np.array_equal(np.isnan(g), np.isnan(ref)), what
    m = ~np.isnan(ref)
    err = np.abs(g[m] - ref[m]) / (1.0 + np.abs(ref[m]))
    print(what, "max err / (1 + |ref|):", float(err.max()) if m.any() else 0.0)
    assert (err <= REL).all(), (what, float(err.max()))


@pytest.mark.parametrize("N,K,vw", [(7, 1, False), (7, 3, True), (130, 1, False), (130, 6, True),
                                    (1027, 1, False), (1027, 3, True), (20000, 1, False),
                                    (20000, 3, False), (20000, 2, True)])
def test_daily_vs_ref_gappy(engine, N, K, vw):
    pan = _panel(engine, N)
    W = _weights(pan["Lh"].shape, 400 + N) if vw else None
    out = engine.daily_returns(pan["Pd"], pan["msd"], pan["L"], pan["NR"], 10, K,
                               W=None if W is None else _up(W))
    DR, DLS, DCNT = _ref(pan, 10, K, W, tag=vw)
    _close(out.DR, DR, "DR")
    _close(out.DLS, DLS, "DLS")
    assert np.array_equal(out.DCNT.cpu().numpy(), DCNT)
    ms = pan["ms"]
    assert np.isnan(DR[:ms[1]]).all() and (~np.isnan(DR[ms[J + SKIP + 2]:])).any()
    if N == 7 and K == 1:   # ten bins over seven assets: a held day has empty bins, NaN there
        got = out.DR.cpu().numpy()
        held = (~np.isnan(got)).sum(axis=1)
        assert held.max() <= 7 and (held > 0).sum() > 200


@pytest.mark.parametrize("K", [1, 3, 6])
@pytest.mark.parametrize("n_bins", [3, 10])
@pytest.mark.parametrize("vw", [False, True])
def test_dense_monthly_product_is_portfolio_return(engine, K, n_bins, vw):
    """Every cell priced: the month's product of 1 + DR is 1 + PR of csm_portfolio, and the
    member counts are the oracle's E1 counts."""
    pan = _panel(engine, 130, dense=True)
    L = pan["L"] if n_bins == 10 else engine.deciles(pan["M"], None, n_bins)[0]
    Lh = L.cpu().numpy()
    W = _weights(Lh.shape, 500) if vw else None
    Wd = None if W is None else _up(W)
    out = engine.daily_returns(pan["Pd"], pan["msd"], L, pan["NR"], n_bins, K, W=Wd)
    DR, DLS, DCNT = _ref(pan, n_bins, K, W, Lh=Lh, tag=vw)
    _close(out.DR, DR, "DR")
    _close(out.DLS, DLS, "DLS")
    got_cnt = out.DCNT.cpu().numpy()
    assert np.array_equal(got_cnt, DCNT)
    CNT = PO.cohort_returns(Lh, pan["NRh"], n_bins, K, W)[3][:, :, 0, :]
    assert np.array_equal(got_cnt, CNT)
    PR = engine.portfolio(L, pan["NR"], n_bins, K, W=Wd, with_costs=False).PR.cpu().numpy()[:, 0, :]
    gross = DRF.monthly_gross(out.DR.cpu().numpy(), pan["ms"])
    assert (~np.isnan(PR)).sum() > 20 * n_bins
    for t in range(len(pan["ms"]) - 2):
        g, r = gross[t + 1], 1.0 + PR[t]
        assert np.array_equal(np.isnan(g), np.isnan(r)), t
        ok = ~np.isnan(r)
        assert (np.abs(g[ok] - r[ok]) <= REL * np.abs(r[ok])).all(), (t, g, r)


def test_two_calls_give_identical_bits(engine):
    pan = _panel(engine, 20000)
    a = engine.daily_returns(pan["Pd"], pan["msd"], pan["L"], pan["NR"], 10, 3)
    b = engine.daily_returns(pan["Pd"], pan["msd"], pan["L"], pan["NR"], 10, 3)
    assert bits_equal(a.DR.cpu().numpy(), b.DR.cpu().numpy())
    assert bits_equal(a.DLS.cpu().numpy(), b.DLS.cpu().numpy())
    assert np.array_equal(a.DCNT.cpu().numpy(), b.DCNT.cpu().numpy())


def test_out_buffers_get_nan_where_there_is_no_portfolio(engine):
    pan = _panel(engine, 130)
    T_d, T_m = pan["P"].shape[0], len(pan["ms"]) - 1
    DR = torch.full((T_d, 10), 12345.0, dtype=torch.float64, device="cuda:0")
    DLS = torch.full((T_d,), -777.0, dtype=torch.float64, device="cuda:0")
    DCNT = torch.full((T_m, 1, 10), -5, dtype=torch.int32, device="cuda:0")
    out = engine.daily_returns(pan["Pd"], pan["msd"], pan["L"], pan["NR"], 10, 1,
                               out=(DR, DLS, DCNT))
    assert out.DR is DR and out.DLS is DLS
    ref = _ref(pan, 10, 1, None, tag=False)
    d1 = pan["ms"][1]
    assert np.isnan(DR.cpu().numpy()[:d1]).all() and np.isnan(DLS.cpu().numpy()[:d1]).all()
    _close(DR, ref[0], "DR")
    _close(DLS, ref[1], "DLS")
    assert np.array_equal(DCNT.cpu().numpy(), ref[2])


def test_unranked_last_rows_give_nan_month(engine):
    """No label in the last held row (nor the one after it): the last month has no portfolio."""
    pan = _panel(engine, 1027)
    Lh = pan["Lh"].copy()
    Lh[-2:] = -1
    out = engine.daily_returns(pan["Pd"], pan["msd"], _up(Lh), pan["NR"], 10, 1)
    DR, DLS, DCNT = DRF.daily_returns(pan["P"], pan["ms"], Lh, pan["NRh"], 10, 1, None)
    got = out.DR.cpu().numpy()
    ms = pan["ms"]
    assert np.isnan(got[ms[-2]:]).all() and np.isnan(out.DLS.cpu().numpy()[ms[-2]:]).all()
    assert not np.isnan(got[ms[-3]:ms[-2]]).all()
    _close(out.DR, DR, "DR")
    assert (out.DCNT.cpu().numpy()[-2:] == 0).all()


def _stats_ref(x, freq):
    """dropna; mean; std(ddof=1); cumprod; running peak floored at 1."""
    x = x[~np.isnan(x)]
    n = len(x)
    if n == 0:
        return np.array([0.0] + [np.nan] * 5)
    mean = x.mean()
    sd = x.std(ddof=1) if n > 1 else np.nan
    cum = np.cumprod(1.0 + x)
    peak = np.maximum(np.maximum.accumulate(cum), 1.0)
    return np.array([n, mean, mean * freq / (sd * np.sqrt(freq)) if sd > 0 else np.nan,
                     sd * np.sqrt(freq), np.max(1.0 - cum / peak), cum[-1]])


def test_series_stats(engine):
    pan = _panel(engine, 1027)
    out = engine.daily_returns(pan["Pd"], pan["msd"], pan["L"], pan["NR"], 10, 1)
    X = torch.stack([out.DR[:, 0], out.DR[:, 4], out.DR[:, 9], out.DLS], dim=1).contiguous()
    got = engine.series_stats(X, freq=252.0).cpu().numpy()
    Xh = X.cpu().numpy()
    assert got.shape == (4, 6)
    for s in range(4):
        ref = _stats_ref(Xh[:, s], 252.0)
        assert ref[0] > 400 and ref[4] > 0
        assert not np.isnan(ref).any() and not np.isnan(got[s]).any()
        err = np.abs(got[s] - ref) / np.abs(ref)
        print("series", s, "max rel err:", float(err.max()))
        assert (err <= 1e-12).all(), (s, got[s], ref)
    one = engine.series_stats(out.DLS).cpu().numpy()
    assert bits_equal(one[0], got[3])


def test_series_stats_all_nan(engine):
    X = torch.full((300, 2), float("nan"), dtype=torch.float64, device="cuda:0")
    X[:, 1] = 0.25   # a constant series with exact sums: deviation 0 -> Sharpe NaN
    got = engine.series_stats(X).cpu().numpy()
    assert got[0, 0] == 0 and np.isnan(got[0, 1:]).all()
    assert got[1, 0] == 300 and np.isnan(got[1, 2]) and got[1, 4] == 0.0
    assert got[1, 5] == np.cumprod(np.full(300, 1.25))[-1]


@pytest.mark.parametrize("K,n_bins", [(0, 10), (13, 10), (1, 7)])
def test_bad_arguments_are_refused(engine, K, n_bins):
    import csmom
    pan = _panel(engine, 130)
    with pytest.raises(csmom.CsmError) as e:
        engine.daily_returns(pan["Pd"], pan["msd"], pan["L"], pan["NR"], n_bins, K)
    assert e.value.status == -1   # CSM_E_INVAL
