"""GPU: csm_daily_market / csm_daily_sums / csm_daily_model and Engine.run_signal's "dbeta",
"divol", "dskew", "max" (rules V1..V6 in DESIGN.md 7) against the NumPy restatement in
tests/dailymkt_ref.py.

Bars.  MKTD is rule R1's sum and one quotient, NMD, NO and the V3 sums are sequential fp64 sums and
maxima in the order the rules state: bit for bit.  The V4 outputs are chains of single correctly
rounded + - * / sqrt on those sums; fp64 sqrt and / are correctly rounded in this build (as
test_gpu_signals.py records), so they are held to bit equality too: MAX_ULP = 0, and the maximum
found is printed.  Labels and counts of the ranking are exact, EW / LS within the project's 1e-10.
"""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

import dailymkt_ref as DR
import signals_ref as SR
from conftest import bits_equal, load_golden, max_rel
from oracle import csmom_oracle as O
from oracle.synth_np import make_panel

pytestmark = pytest.mark.gpu
T_DAYS = 782            # 36 whole business-day months of 19..23 rows from 2000-01-03
GAPPY = dict(late=0.2, delist=0.2, nan_day=0.01, absent_month=0.01, nan_month=0.01)
DENSE = dict(late=0, delist=0, nan_day=0, absent_month=0, nan_month=0)
MAX_ULP = 0             # see the module docstring
GAP_COL = 5             # the hand-built column of the "gaps" panels
_CACHE = {}


def _up(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _host_panel(N, kind, max_gap):
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
    if kind == "gaps":       # dailymkt_ref.gap_column: gaps around max_gap, across chunk starts
        P[:, GAP_COL], _ = DR.gap_column(T_DAYS, max_gap, int(ms[8]), O.absent_scalar())
    return P, ms


def _panel(N, kind="gappy", max_gap=10):
    """Host panel, its device copy and the V1..V3 reference; computed once and left unchanged."""
    key = (N, kind, max_gap)
    if key not in _CACHE:
        P, ms = _host_panel(N, kind, max_gap)
        ref = DR.daily(P, ms, max_gap)
        _CACHE[key] = dict(P=P, ms=ms, Pd=_up(P), msd=_up(ms), ref=ref, mod={}, max_gap=max_gap)
    return _CACHE[key]


def _model_ref(pan, Wm, min_obs):
    if (Wm, min_obs) not in pan["mod"]:
        pan["mod"][(Wm, min_obs)] = DR.daily_model(pan["ref"], Wm, min_obs)
    return pan["mod"][(Wm, min_obs)]


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


def _check_market(pan, MKTD, NMD):
    ref = pan["ref"]
    assert np.array_equal(NMD.cpu().numpy(), ref["NMD"]), "NMD"
    assert bits_equal(MKTD.cpu().numpy(), ref["MKTD"]), "MKTD"


def _check_sums(sums, ref):
    assert np.array_equal(sums.NO.cpu().numpy(), ref["NO"]), "NO"
    for k in DR.SUMS[1:]:
        assert bits_equal(getattr(sums, k).cpu().numpy(), ref[k]), k


def _check_model(mod, ref, tag):
    assert np.array_equal(mod.NOBS.cpu().numpy(), ref["NOBS"]), "NOBS"
    for k in DR.MODEL[:5]:
        assert _ulps(getattr(mod, k).cpu().numpy(), ref[k], f"{k}{tag}") <= MAX_ULP, k


def _run(engine, pan, Pd=None, models=((1, 15), (3, None))):
    Pd = pan["Pd"] if Pd is None else Pd
    MKTD, NMD = engine.daily_market(Pd, pan["max_gap"])
    _check_market(pan, MKTD, NMD)
    sums = engine.daily_sums(Pd, pan["msd"], MKTD, pan["max_gap"])
    _check_sums(sums, pan["ref"])
    for Wm, mo in models:
        mod = engine.daily_model(sums, Wm, mo)
        _check_model(mod, _model_ref(pan, Wm, mo), f"(Wm={Wm})")
    return MKTD, NMD, sums


def _defined(pan):
    """Share of the (t, asset) cells with every Wm = 1, min_obs = 15 output defined."""
    ref = _model_ref(pan, 1, 15)
    return min(float((~np.isnan(ref[k])).mean()) for k in DR.MODEL[:5])


@pytest.mark.parametrize("N", [1, 2, 63, 257, 2050, 4097])
def test_vs_ref_gappy(engine, N):
    pan = _panel(N)
    _run(engine, pan)
    assert _defined(pan) >= 0.5
    if N >= 63:   # the gaps bite: some returns reach over rows without a price, some are refused
        r = pan["ref"]["R"]
        priced = ~np.isnan(pan["P"])
        assert (priced[1:] & ~priced[:-1] & ~np.isnan(r[1:])).sum() >= 10
        assert (pan["ref"]["NMD"] < N).any() and (pan["ref"]["NMD"] > 0).sum() >= T_DAYS - 2


@pytest.mark.parametrize("N", [63, 2050])
def test_vs_ref_dense(engine, N):
    pan = _panel(N, "dense")
    _run(engine, pan)
    assert _defined(pan) == 1.0
    assert (pan["ref"]["NMD"][1:] == N).all()
    assert (pan["ref"]["NO"][1:] == np.diff(pan["ms"])[1:, None]).all()   # a return every day


@pytest.mark.parametrize("max_gap", [1, 3, 10])
def test_max_gap(engine, max_gap):
    """The bound itself (gappy rows), and for max_gap >= 2 the hand-built column whose gaps are
    one under, at and one over the bound."""
    pan = _panel(257, "gappy" if max_gap == 1 else "gaps", max_gap)
    _run(engine, pan)
    assert _defined(pan) >= 0.5
    if max_gap > 1:
        _, cases = DR.gap_column(T_DAYS, max_gap, int(pan["ms"][8]), O.absent_scalar())
        r = pan["ref"]["R"][:, GAP_COL]
        assert [not np.isnan(r[d]) for d, _, _ in cases] == [b for _, _, b in cases]
    else:   # a return needs the row before it
        priced = ~np.isnan(pan["P"])
        assert np.array_equal(~np.isnan(pan["ref"]["R"][1:]), priced[1:] & priced[:-1])
    other = _panel(257, "gappy", 10)["ref"]["NMD"] if max_gap == 1 else None
    assert other is None or (other >= pan["ref"]["NMD"]).all() and (other > pan["ref"]["NMD"]).any()


@pytest.mark.parametrize("kind", ["zero", "calendar", "columns"])
def test_calendars_and_empty_columns(engine, kind):
    pan = _panel(130, kind)
    _, _, sums = _run(engine, pan)
    assert _defined(pan) >= 0.5
    if kind == "zero":
        assert (sums.NO[4] == 0).all() and (sums.SR[4] == 0).all() and (sums.SRF[4] == 0).all()
        assert torch.isnan(sums.RMAX[4]).all()
    if kind == "calendar":
        assert int(engine.month_days(pan["msd"])[0]) == 31
    if kind == "columns":
        assert (sums.NO[:, 3:5] == 0).all() and torch.isnan(sums.RMAX[:, 3:5]).all()
        mod = engine.daily_model(sums, 1, 15)
        assert torch.isnan(mod.DIVOL[:, 3:5]).all() and not torch.isnan(mod.DIVOL[:, 5]).all()


def test_unaligned_panel_takes_the_one_asset_path(engine):
    """Even N through a view 8 B past a 16-B boundary: the same bits as the paired path."""
    pan = _panel(2050)
    T_d, N = pan["P"].shape
    flat = torch.empty(T_d * N + 1, dtype=torch.float64, device="cuda:0")
    view = flat[1:].view(T_d, N)
    view.copy_(pan["Pd"])
    assert pan["Pd"].data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8
    _run(engine, pan, Pd=view)


def _tune(key, value):
    import csmom
    assert csmom.load_library().csm_tune(key.encode(), ctypes.c_int(value)) == 0


def _raw(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else t.dtype)


def _same(xs, ys):
    return all(torch.equal(_raw(a), _raw(b)) for a, b in zip(xs, ys))


@pytest.mark.parametrize("N,kind", [(257, "gaps"), (2050, "gappy")])
def test_launch_shape_changes_no_bit(engine, N, kind):
    pan = _panel(N, kind)
    T_m = len(pan["ms"]) - 1
    try:
        base = _run(engine, pan)
        for days in (T_DAYS, 7, 64):   # 7: every gap of the hand-built column crosses a chunk start
            _tune("dmkt_chunk_days", days)
            got = engine.daily_market(pan["Pd"], pan["max_gap"])
            assert _same(got, base[:2]), days
        for chunks in (1, 5, T_m):
            _tune("dsums_chunks", chunks)
            got = engine.daily_sums(pan["Pd"], pan["msd"], base[0], pan["max_gap"])
            assert _same(got, base[2]), chunks
        for Wm in (1, 3, 12):
            _tune("dmodel_chunks", 0)
            want = engine.daily_model(base[2], Wm)
            _check_model(want, _model_ref(pan, Wm, None), f"(Wm={Wm})")
            for chunks in (1, 4, T_m):
                _tune("dmodel_chunks", chunks)
                got = engine.daily_model(base[2], Wm)
                assert _same([getattr(got, k) for k in DR.MODEL],
                             [getattr(want, k) for k in DR.MODEL]), (Wm, chunks)
    finally:
        for k in ("dmkt_chunk_days", "dsums_chunks", "dmodel_chunks"):
            _tune(k, 0)


def test_twice_the_same_bits_and_min_assets(engine):
    pan = _panel(4097)
    a, b = _run(engine, pan, models=((1, 15),)), _run(engine, pan, models=((1, 15),))
    assert _same(a[:2], b[:2]) and _same(a[2], b[2])
    MKTD, NMD = engine.daily_market(pan["Pd"], min_assets=3000)
    ref = DR.daily_market(pan["P"], min_assets=3000)
    assert bits_equal(MKTD.cpu().numpy(), ref["MKTD"]) and torch.equal(NMD, a[1])
    assert 0 < int(torch.isnan(MKTD).sum()) < T_DAYS


def test_a_factor_of_the_callers(engine):
    """FD = MKTD with some days NaN removes exactly those days' observations."""
    pan = _panel(257)
    FD = pan["ref"]["MKTD"].copy()
    cut = np.arange(3, T_DAYS, 11)
    FD[cut] = np.nan
    sums = engine.daily_sums(pan["Pd"], pan["msd"], _up(FD))
    ref = DR.daily_sums(pan["ref"]["R"], FD, pan["ms"])
    _check_sums(sums, ref)
    lost = ~np.isnan(pan["ref"]["R"][cut]) & ~np.isnan(pan["ref"]["MKTD"][cut])[:, None]
    assert int(pan["ref"]["NO"].sum() - sums.NO.sum().item()) == lost.sum() > 0
    slim = engine.daily_sums(pan["Pd"], pan["msd"], _up(FD), with_sr3=False, with_rmax=False)
    assert slim.SR3 is None and slim.RMAX is None and _same(slim[:6], sums[:6])
    mod = engine.daily_model(slim, 1, 15)
    assert mod.DSKEW is None and mod.DMAX is None
    _check_model_some(mod, DR.daily_model(ref, 1, 15), ("DBETA", "DIVOL", "DTVOL"))


def _check_model_some(mod, ref, keys):
    for k in keys:
        assert _ulps(getattr(mod, k).cpu().numpy(), ref[k], k) <= MAX_ULP, k


@pytest.mark.parametrize("signal", ["divol", "max", "dbeta", "dskew"])
def test_run_signal(engine, signal):
    pan = _panel(257)
    Wm = 12 if signal == "dbeta" else 1
    ref = _model_ref(pan, Wm, None)[engine.DAILY_SIGNALS[signal]]
    if "PM" not in pan:
        pan["PM"] = SR.month_stats(pan["P"], pan["ms"])["PM"]
    out = engine.run_signal(pan["Pd"], pan["msd"], signal)
    assert bits_equal(out.PM.cpu().numpy(), pan["PM"])
    assert _ulps(out.M.cpu().numpy(), ref, signal) <= MAX_ULP
    NRr = SR.next_ret(pan["PM"], ref)
    assert bits_equal(out.NR.cpu().numpy(), NRr)
    Lr = O.assign_deciles(ref, 10)
    EWr, CNTr, LSr = O.portfolio_ew(Lr, NRr, 10)
    assert np.array_equal(out.L.cpu().numpy(), Lr)
    assert np.array_equal(out.CNT.cpu().numpy(), CNTr)
    for got, want in ((out.EW, EWr), (out.LS, LSr)):
        g = got.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(want))
        assert max_rel(g, want) <= 1e-10
    assert (~np.isnan(LSr)).sum() >= 36 - Wm - 1
    if signal == "divol":   # an explicit window and min_obs reach the model
        o3 = engine.run_signal(pan["Pd"], pan["msd"], signal, window=3, min_obs=40)
        assert bits_equal(o3.M.cpu().numpy(), _model_ref(pan, 3, 40)["DIVOL"])


def _real_frame():
    z = load_golden("real_data")
    P = z["P"]
    dd, aa = np.nonzero(~O.is_absent(P))
    return pd.DataFrame({"date": pd.to_datetime(z["day_ns"])[dd], "ticker": z["tickers"][aa],
                         "adj_close": P[dd, aa]})


def test_tables_from_a_daily_frame(engine):
    import csmom
    df = _real_frame()
    fm = csmom.fama_macbeth(df, signals=("mom", "divol", "max"), device=0)
    assert list(fm.table.index) == ["const", "mom", "divol", "max"]
    assert np.isfinite(fm.table[["mean", "se", "t"]].to_numpy()).all()
    assert (fm.table["months"] >= 20).all()
    ic = csmom.information_coefficient(df, signals=("divol",), device=0)
    assert np.isfinite(ic.table[["mean", "se", "t"]].to_numpy()).all() and len(ic.table) >= 1
    assert set(engine.DAILY_SIGNALS) <= set(csmom.regress.SIGNAL_NAMES)


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
    pan = _panel(63)
    Pd, msd = pan["Pd"], pan["msd"]
    T_d, N = Pd.shape
    T_m = msd.numel() - 1
    lib = csmom.load_library()
    assert lib.csm_daily_market_workspace(T_d, N) == T_d * 4 * 12
    assert lib.csm_daily_market_workspace(T_d, 4097) == T_d * 3 * 4 * 12
    assert lib.csm_daily_market_workspace(0, N) == 0 and lib.csm_daily_market_workspace(T_d, 0) == 0
    ws = torch.empty(T_d * 4 * 12, dtype=torch.uint8, device="cuda:0")
    mk = torch.full((T_d,), SENTINEL, dtype=torch.float64, device="cuda:0")
    nm = torch.full((T_d,), 77, dtype=torch.int32, device="cuda:0")

    def market(P=Pd, gap=10, ma=1, out=mk, w=ws, td=T_d):
        return (_ptr(P), td, N, gap, ma, _ptr(out), _ptr(nm), _ptr(w))

    for args in (market(gap=0), market(gap=33), market(ma=0), market(P=None), market(out=None),
                 market(w=None), market(td=0)):
        _refused(engine, "csm_daily_market", args, [mk, nm])

    f = [torch.full((T_m, N), SENTINEL, dtype=torch.float64, device="cuda:0") for _ in range(7)]
    no = torch.full((T_m, N), 77, dtype=torch.int32, device="cuda:0")
    FD = _up(pan["ref"]["MKTD"])

    def sums(P=Pd, F=FD, ms=msd, tm=T_m, mmd=23, gap=10, o=range(7), n=no):
        ptrs = [_ptr(f[i]) if i in o else None for i in range(7)]
        return (_ptr(P), _ptr(F), T_d, N, _ptr(ms), tm, mmd, gap, _ptr(n), *ptrs)

    bad = [sums(gap=0), sums(gap=33), sums(mmd=0), sums(mmd=33), sums(tm=0), sums(P=None),
           sums(F=None), sums(ms=None), sums(n=None)]
    bad += [sums(o=[j for j in range(7) if j != i]) for i in range(5)]
    for args in bad:
        _refused(engine, "csm_daily_sums", args, f + [no])
    for kw in (dict(max_gap=0), dict(max_gap=33)):
        with pytest.raises(csmom.CsmError):
            engine.daily_market(Pd, **kw)
        with pytest.raises(csmom.CsmError):
            engine.daily_sums(Pd, msd, FD, **kw)

    s = engine.daily_sums(Pd, msd, FD)
    ins = [_ptr(t) for t in s]
    g = [torch.full((T_m, N), SENTINEL, dtype=torch.float64, device="cuda:0") for _ in range(5)]
    nobs = torch.full((T_m, N), 77, dtype=torch.int32, device="cuda:0")

    def model(ins=ins, tm=T_m, Wm=1, mo=15, o=range(6)):
        ptrs = [_ptr(t) if i in o else None for i, t in enumerate(g + [nobs])]
        return (*ins, tm, N, Wm, mo, *ptrs)

    bad = [model(Wm=0), model(Wm=13), model(mo=1), model(tm=0), model(o=()),
           model(ins=ins[:6] + [None, ins[7]]),            # DSKEW without SR3
           model(ins=ins[:7] + [None]),                    # DMAX without RMAX
           model(ins=ins[:6] + [None, ins[7]], o=(3,))]
    bad += [model(ins=ins[:i] + [None] + ins[i + 1:]) for i in range(6)]
    for args in bad:
        _refused(engine, "csm_daily_model", args, g + [nobs])
    # without the nullable inputs the other outputs are served
    engine._call("csm_daily_model", *ins[:6], None, None, T_m, N, 1, 15, _ptr(g[0]), None, None,
                 None, None, None)
    assert bits_equal(g[0].cpu().numpy(), _model_ref(pan, 1, 15)["DBETA"])
    for kw in (dict(window=0), dict(window=13), dict(min_obs=1)):
        with pytest.raises(csmom.CsmError) as e:
            engine.daily_model(s, **kw)
        assert e.value.status == -1
    with pytest.raises(ValueError):
        engine.daily_model(s, outputs=("DBETA", "XX"))
    with pytest.raises(ValueError):
        engine.run_signal(Pd, msd, "dmax")
