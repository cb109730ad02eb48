"""GPU: csm_month_stats / csm_window_signals / Engine.run_signal (rules D1..D6 in DESIGN.md 7)
against the NumPy restatement in tests/signals_ref.py.

Bars.  PM, P1, HI, SSW, NDW, SS, ND, H52, NR_H52 and NR_MS are sequential fp64 sums, maxima and
single correctly rounded quotients in the order the rules state: bit for bit.  RV = sqrt(S / n)
and MS = M / RV take S and n exact.  fp64 sqrt and / are correctly rounded in this build: the
bar was 2 ulp (one for the root, one for the quotient that consumes it), every case below
measured 0 on an MI355X (the maximum found is still printed), and so both are held to bit
equality as well.  Labels and counts of the ranking are exact, EW / LS within the
project's 1e-10.
"""
import ctypes

import numpy as np
import pytest
import torch

import signals_ref as SR
from conftest import bits_equal, max_rel
from oracle import csmom_oracle as O
from oracle.synth_np import make_panel

pytestmark = pytest.mark.gpu
T_DAYS = 782            # 36 whole business-day months of 19..23 rows from 2000-01-03
GAPPY = dict(late=0.2, delist=0.2, nan_day=0.01, absent_month=0.01, nan_month=0.01)
DENSE = dict(late=0, delist=0, nan_day=0, absent_month=0, nan_month=0)
MAX_ULP = 0             # see the module docstring
J_MOM, SKIP = 6, 1
_CACHE = {}


def _up(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _host_panel(N, kind):
    if kind == "dense":
        pan = make_panel(N, T_DAYS, seed=100 + N, cents=True, with_volume=False, **DENSE)
        return pan["P"], pan["month_start"]
    if kind == "calendar":   # calendar-day months of 28..31 rows: 2000-01 .. 2002-12
        pan = make_panel(N, 1096, seed=200 + N, cents=True, with_volume=False, **GAPPY)
        lens = [31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31] + 2 * [31, 28, 31, 30, 31, 30, 31,
                                                                       31, 30, 31, 30, 31]
        ms = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        assert ms[-1] == 1096 and min(lens) == 28 and max(lens) == 31
        return pan["P"], ms
    pan = make_panel(N, T_DAYS, seed=200 + N, cents=True, with_volume=False, **GAPPY)
    P, ms = pan["P"], pan["month_start"]
    d = np.diff(ms)
    assert len(ms) - 1 == 36 and d.min() >= 19 and d.max() <= 23
    if kind == "zero":       # month 4 has no day
        ms = np.concatenate([ms[:5], ms[4:]])
    if kind == "columns":    # a column without any price, and one without any row
        P[:, 3] = np.nan
        P[:, 4] = O.absent_like(P.shape[0])
    return P, ms


def _panel(N, kind="gappy"):
    """Host panel, its device copy, the momentum the MS signal scales and the D1 reference;
    computed once per panel and left unchanged."""
    key = (N, kind)
    if key not in _CACHE:
        P, ms = _host_panel(N, kind)
        st = SR.month_stats(P, ms)
        M = O.momentum_scan(st["PM"], J_MOM, SKIP)[1]
        _CACHE[key] = dict(P=P, ms=ms, Pd=_up(P), msd=_up(ms), st=st, M=M, Md=_up(M), ref={})
    return _CACHE[key]


def _ref(pan, Jh, Jv):
    if (Jh, Jv) not in pan["ref"]:
        st = pan["st"]
        pan["ref"][(Jh, Jv)] = SR.window_signals(st["PM"], st["P1"], st["HI"], st["SSW"],
                                                 st["NDW"], pan["M"], Jh, Jv)
    return pan["ref"][(Jh, Jv)]


def _ulps(got, ref, what):
    """Largest distance in ulp between two arrays with the same NaN pattern."""
    g, r = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert np.array_equal(np.isnan(g), np.isnan(r)), f"{what}: NaN pattern"
    ok = ~np.isnan(r)
    assert (np.signbit(g[ok]) == np.signbit(r[ok])).all(), what
    d = np.abs(g[ok].view(np.int64) - r[ok].view(np.int64))
    worst = int(d.max()) if d.size else 0
    print(f"{what}: max {worst} ulp over {int(ok.sum())} cells")
    return worst


def _check_stats(engine, pan, st):
    ref = pan["st"]
    for k in ("PM", "P1", "HI", "SSW"):
        assert bits_equal(getattr(st, k).cpu().numpy(), ref[k]), k
    assert np.array_equal(st.NDW.cpu().numpy(), ref["NDW"]), "NDW"
    # the ABSENT payload exactly where csm_month_end puts it
    pme, _ = engine.month_end(pan["Pd"], pan["msd"])
    import csmom
    assert torch.equal(csmom.is_absent(st.PM), csmom.is_absent(pme))
    assert np.array_equal(csmom.is_absent(st.PM).cpu().numpy(), O.is_absent(ref["PM"]))


def _check_signals(pan, sig, Jh, Jv):
    ref = _ref(pan, Jh, Jv)
    for k in ("SS", "H52", "NR_H52", "NR_MS"):
        assert bits_equal(getattr(sig, k).cpu().numpy(), ref[k]), (k, Jh, Jv)
    assert np.array_equal(sig.ND.cpu().numpy(), ref["ND"]), "ND"
    assert _ulps(sig.RV.cpu().numpy(), ref["RV"], f"RV({Jv})") <= MAX_ULP
    assert _ulps(sig.MS.cpu().numpy(), ref["MS"], f"MS({Jv})") <= MAX_ULP
    h = ref["H52"]
    assert (h[~np.isnan(h)] <= 1.0).all()


def _run(engine, pan, Jh=12, Jv=12, Pd=None):
    st = engine.month_stats(pan["Pd"] if Pd is None else Pd, pan["msd"])
    _check_stats(engine, pan, st)
    sig = engine.window_signals(*st, M=pan["Md"], Jh=Jh, Jv=Jv)
    _check_signals(pan, sig, Jh, Jv)
    return st, sig


@pytest.mark.parametrize("N", [1, 7, 130, 1027, 4098, 20000])
def test_signals_vs_ref_gappy(engine, N):
    pan = _panel(N)
    _run(engine, pan)
    ref = _ref(pan, 12, 12)
    if N >= 7:   # nothing passes on empty outputs
        for k in ("H52", "RV", "MS"):
            assert (~np.isnan(ref[k])).mean() >= 0.5, (k, float((~np.isnan(ref[k])).mean()))
    if N == 130:
        assert (ref["H52"] == 1.0).sum() >= 50
        assert (~np.isnan(ref["NR_H52"])).mean() >= 0.4 and (~np.isnan(ref["NR_MS"])).mean() >= 0.4


@pytest.mark.parametrize("N", [130, 4098])
def test_signals_vs_ref_dense(engine, N):
    pan = _panel(N, "dense")
    _run(engine, pan)
    ref = _ref(pan, 12, 12)
    for k in ("H52", "RV", "MS"):
        assert (~np.isnan(ref[k])).mean() >= 0.5, k
    assert (ref["ND"][1:] == np.diff(pan["ms"])[1:, None]).all()   # a return every day


@pytest.mark.parametrize("Jh,Jv", [(3, 6), (1, 1), (36, 36)])
def test_windows(engine, Jh, Jv):
    pan = _panel(130)
    _run(engine, pan, Jh, Jv)
    ref = _ref(pan, Jh, Jv)
    assert (~np.isnan(ref["H52"])).sum() > 0 and (~np.isnan(ref["RV"])).sum() > 0
    if (Jh, Jv) == (36, 36):   # one month has 36 months of history
        assert np.isnan(ref["H52"][:35]).all() and np.isnan(ref["RV"][:35]).all()


def test_unaligned_panel_takes_the_one_asset_path(engine):
    """Even N through a view 8 B past a 16-B boundary: the same bits as the paired path."""
    pan = _panel(130)
    T_d, N = pan["P"].shape
    flat = torch.empty(T_d * N + 1, dtype=torch.float64, device="cuda:0")
    view = flat[1:].view(T_d, N)
    view.copy_(pan["Pd"])
    assert pan["Pd"].data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8
    _run(engine, pan, Pd=view)


@pytest.mark.parametrize("kind", ["zero", "calendar", "columns"])
def test_calendars_and_empty_columns(engine, kind):
    pan = _panel(130, kind)
    st, sig = _run(engine, pan)
    if kind == "zero":
        import csmom
        assert csmom.is_absent(st.PM[4]).all() and (st.NDW[4] == 0).all()
    if kind == "calendar":
        assert int(engine.month_days(pan["msd"])[0]) == 31
    if kind == "columns":
        h = sig.H52.cpu().numpy()
        assert np.isnan(h[:, 3:5]).all() and not np.isnan(h[:, 5]).all()
        assert np.isnan(sig.RV.cpu().numpy()[:, 3:5]).all()
        assert (sig.ND.cpu().numpy()[:, 3:5] == 0).all()


def _tune(key, value):
    import csmom
    assert csmom.load_library().csm_tune(key.encode(), ctypes.c_int(value)) == 0


def _raw(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else t.dtype)


@pytest.mark.parametrize("N", [130, 1027])
def test_chunk_count_changes_no_bit(engine, N):
    pan = _panel(N)
    try:
        outs = {}
        for chunks in (0, 1, 5, 36):
            _tune("stats_chunks", chunks)
            st = engine.month_stats(pan["Pd"], pan["msd"])
            _check_stats(engine, pan, st)
            outs[chunks] = st
        for chunks in (1, 5, 36):   # NaN payloads included
            for a, b in zip(outs[0], outs[chunks]):
                assert torch.equal(_raw(a), _raw(b)), chunks
    finally:
        _tune("stats_chunks", 0)


@pytest.mark.parametrize("N", [7, 130])
def test_ranking_on_the_52_week_high(engine, N):
    pan = _panel(N)
    ref = _ref(pan, 12, 12)
    st = engine.month_stats(pan["Pd"], pan["msd"])
    sig = engine.window_signals(*st, Jh=12, Jv=12)
    assert sig.MS is None and sig.NR_MS is None
    L, EW, CNT, _ = engine.deciles(sig.H52, sig.NR_H52, 10)
    LS = engine.long_short(EW, CNT)
    Lr = O.assign_deciles(ref["H52"], 10)
    EWr, CNTr, LSr = O.portfolio_ew(Lr, ref["NR_H52"], 10)
    assert np.array_equal(L.cpu().numpy(), Lr)
    assert np.array_equal(CNT.cpu().numpy(), CNTr)
    for got, want in ((EW, EWr), (LS, LSr)):
        g = got.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(want))
        assert max_rel(g, want) <= 1e-10
    ranked = (Lr >= 0).any(axis=1)
    assert ranked.sum() >= 20
    if N == 7:    # fewer values than bins, and ties at 1.0: qcut drops duplicate edges
        assert all(len(np.unique(Lr[t][Lr[t] >= 0])) < 10 for t in np.nonzero(ranked)[0])
    else:
        assert (~np.isnan(LSr)).sum() >= 20


def _same(a, b):
    for k in ("PM", "M", "NR", "L", "EW", "CNT", "LS", "NV"):
        x, y = getattr(a, k), getattr(b, k)
        if not torch.equal(_raw(x), _raw(y)):
            return False
    return True


def test_run_signal_is_the_step_by_step_calls(engine):
    pan = _panel(1027)
    st = engine.month_stats(pan["Pd"], pan["msd"])
    sig = engine.window_signals(*st, Jh=12, Jv=12)
    L, EW, CNT, NV = engine.deciles(sig.H52, sig.NR_H52, 10, with_nv=True)
    LS = engine.long_short(EW, CNT)
    out = engine.run_signal(pan["Pd"], pan["msd"], "high52")
    for got, want in ((out.PM, st.PM), (out.M, sig.H52), (out.NR, sig.NR_H52), (out.L, L),
                      (out.EW, EW), (out.CNT, CNT), (out.LS, LS), (out.NV, NV)):
        assert torch.equal(_raw(got), _raw(want))
    assert (~torch.isnan(out.LS)).sum() >= 20

    _, M, _ = engine.momentum(st.PM, 6, 1)
    assert bits_equal(M.cpu().numpy(), pan["M"])
    sig = engine.window_signals(*st, M=M, Jh=12, Jv=12)
    L, EW, CNT, NV = engine.deciles(sig.MS, sig.NR_MS, 10, with_nv=True)
    LS = engine.long_short(EW, CNT)
    out = engine.run_signal(pan["Pd"], pan["msd"], "mom_vol", J=6)
    for got, want in ((out.PM, st.PM), (out.M, sig.MS), (out.NR, sig.NR_MS), (out.L, L),
                      (out.EW, EW), (out.CNT, CNT), (out.LS, LS), (out.NV, NV)):
        assert torch.equal(_raw(got), _raw(want))
    assert (~torch.isnan(out.LS)).sum() >= 20
    assert _same(out, engine.run_signal(pan["Pd"], pan["msd"], "mom_vol", J=6))
    a = engine.run_signal(pan["Pd"], pan["msd"], "high52", window=6)
    assert _same(a, engine.run_signal(pan["Pd"], pan["msd"], "high52", window=6))
    assert not torch.equal(_raw(a.M), _raw(engine.run_signal(pan["Pd"], pan["msd"], "high52").M))
    with pytest.raises(ValueError):
        engine.run_signal(pan["Pd"], pan["msd"], "low52")


def test_rv_feeds_the_cost_model(engine):
    """RV is the SIG input of csm_portfolio: NaN cells fall back to the constant, as before."""
    pan = _panel(130)
    out = engine.run_signal(pan["Pd"], pan["msd"], "high52")
    st = engine.month_stats(pan["Pd"], pan["msd"])
    rv = engine.window_signals(*st, outputs=("RV",)).RV
    adv = torch.full_like(rv, 1e6)
    a = engine.portfolio(out.L, out.NR, 10, 3, aum=1e8, ADV=adv, SIG=rv)
    b = engine.portfolio(out.L, out.NR, 10, 3, aum=1e8, ADV=adv,
                         SIG=torch.full_like(rv, float("nan")))
    assert torch.equal(_raw(a.LS), _raw(b.LS))
    ca, cb = a.COST.cpu().numpy(), b.COST.cpu().numpy()
    assert np.array_equal(np.isnan(ca), np.isnan(cb)) and (~np.isnan(ca)).sum() >= 15
    assert not np.array_equal(ca[~np.isnan(ca)], cb[~np.isnan(cb)])


SENTINEL = 12345.0


def _refused(engine, name, args, outs):
    import csmom
    with pytest.raises(csmom.CsmError) as e:
        engine._call(name, *args)
    assert e.value.status == -1   # CSM_E_INVAL
    torch.cuda.synchronize()
    for t in outs:                # nothing was launched
        assert (t == (SENTINEL if t.dtype == torch.float64 else 77)).all()


def test_bad_arguments_are_refused(engine):
    import csmom
    from csmom.engine import _ptr
    pan = _panel(130)
    Pd, msd = pan["Pd"], pan["msd"]
    T_d, N = Pd.shape
    T_m = msd.numel() - 1
    f = [torch.full((T_m, N), SENTINEL, dtype=torch.float64, device="cuda:0") for _ in range(4)]
    ndw = torch.full((T_m, N), 77, dtype=torch.int32, device="cuda:0")
    outs = f + [ndw]

    def stats(P=Pd, ms=msd, tm=T_m, mmd=23, o=(0, 1, 2, 3)):
        ptrs = [_ptr(f[i]) if i in o else None for i in range(4)]
        return (_ptr(P), T_d, N, _ptr(ms), tm, mmd, *ptrs, _ptr(ndw))

    for args in (stats(mmd=0), stats(mmd=33), stats(tm=0), stats(P=None), stats(ms=None),
                 stats(o=(0, 2, 3)), stats(o=(0, 1, 3)), stats(o=(0, 1, 2))):
        _refused(engine, "csm_month_stats", args, outs)
    for kw in (dict(max_month_days=33), dict(max_month_days=0)):
        with pytest.raises(csmom.CsmError):
            engine.month_stats(Pd, msd, **kw)
    with pytest.raises(csmom.CsmError):
        engine.month_stats(Pd, msd[:1])   # no month

    st = engine.month_stats(Pd, msd)
    ins = [_ptr(t) for t in st]
    g = [torch.full((T_m, N), SENTINEL, dtype=torch.float64, device="cuda:0") for _ in range(6)]
    nd = torch.full((T_m, N), 77, dtype=torch.int32, device="cuda:0")
    outs = g + [nd]

    def win(Jh=12, Jv=12, mo=120, M=pan["Md"], tm=T_m, ins=ins):
        return (*ins, _ptr(M), tm, N, Jh, Jv, mo, _ptr(g[0]), _ptr(nd), *(_ptr(t) for t in g[1:]))

    bad = [win(Jh=37), win(Jh=0), win(Jv=37), win(Jv=0), win(mo=0), win(tm=0), win(M=None)]
    bad += [win(ins=ins[:i] + [None] + ins[i + 1:]) for i in range(5)]
    for args in bad:
        _refused(engine, "csm_window_signals", args, outs)
    for kw in (dict(Jh=37), dict(Jv=37), dict(Jh=0), dict(min_obs=0)):
        with pytest.raises(csmom.CsmError) as e:
            engine.window_signals(*st, **kw)
        assert e.value.status == -1
    with pytest.raises(ValueError):
        engine.window_signals(*st, outputs=("H52", "XX"))
    # NR_MS alone without M
    _refused(engine, "csm_window_signals",
             (*ins, None, T_m, N, 12, 12, 120, None, None, None, None, None, None, _ptr(g[5])),
             outs)
