"""GPU: csm_liq_sums / csm_liq_model, Engine.run_signal's "illiq", "dvol", "zret" and the host
entries on them (rules Q1..Q6 in DESIGN.md 7) against the NumPy restatement in tests/liq_ref.py.

Bars.  The Q2 counts and sums and NOBS are sequential sums in the order the rules state: bit for
bit.  The Q3 outputs are chains of single correctly rounded + * / on those sums; fp64 / is
correctly rounded in this build (as test_gpu_signals.py records), so they are held to bit equality
too: MAX_ULP = 0, and the maximum found is printed.  Labels and counts of the ranking are exact,
EW / LS within the project's 1e-10.

make_panel's volumes are never zero or NaN (checked in _host), so the panels get zero-volume days
(about 5 % of the cells) and NaN-volume days (about 1 %) from a seeded rng here.
"""
import ctypes

import numpy as np
import pytest
import torch

import dailymkt_ref as DR
import liq_ref as LR
import signals_ref as SR
from conftest import bits_equal, max_rel
from oracle import csmom_oracle as O
from oracle.synth_np import make_panel, to_long

pytestmark = pytest.mark.gpu
T_DAYS = 782            # 36 whole business-day months of 19..23 rows from 2000-01-03
GAPPY = dict(late=0.2, delist=0.2, nan_day=0.01, absent_month=0.01, nan_month=0.01)
DENSE = dict(late=0, delist=0, nan_day=0, absent_month=0, nan_month=0)
MAX_ULP = 0             # see the module docstring
GAP_COL = 5             # the hand-built column of the "gaps" panels
SIZES = [1, 2, 63, 130, 257, 514]   # odd and even, a partial wave, a second workgroup at
                                    # one (257) and at two (514) assets per lane
PAIR = (0, 1)           # csm_tune "lsums_pair": one asset per lane | two where the panels allow
_CACHE = {}


def _up(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _host(N, kind="gappy", max_gap=10):
    """Host panels, shares and the Q1, Q2 reference; computed once and left unchanged."""
    key = (N, kind, max_gap)
    if key in _CACHE:
        return _CACHE[key]
    if kind == "calendar":   # calendar-day months of 28..31 rows: 2000-01 .. 2002-12
        pan = make_panel(N, 1096, seed=300 + N, cents=True, with_volume=True, **GAPPY)
        lens = [31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31] + 2 * [31, 28, 31, 30, 31, 30, 31,
                                                                       31, 30, 31, 30, 31]
        ms = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        assert ms[-1] == 1096
    else:
        pan = make_panel(N, T_DAYS, seed=300 + N, cents=True, with_volume=True,
                         **(DENSE if kind == "dense" else GAPPY))
        ms = pan["month_start"]
        d = np.diff(ms)
        assert len(ms) - 1 == 36 and d.min() >= 19 and d.max() <= 23
    P, V = pan["P"], pan["V"]
    assert (V > 0).all()                       # never zero, never NaN: the cases come from here
    rng = np.random.default_rng(900 + N)
    u = rng.random(V.shape)
    V[u < 0.05] = 0.0
    V[u > 0.99] = np.nan
    if kind == "zero":       # month 4 has no day
        ms = np.concatenate([ms[:5], ms[4:]])
    if kind == "columns":    # a column without any price, and one without any row
        P[:, 3] = np.nan
        P[:, 4] = O.absent_like(P.shape[0])
    if kind == "gaps":       # dailymkt_ref.gap_column: gaps around max_gap, across chunk starts
        P[:, GAP_COL], _ = DR.gap_column(T_DAYS, max_gap, int(ms[8]), O.absent_scalar())
    T_m = len(ms) - 1
    SH = np.round(rng.lognormal(17.0, 1.0, (T_m, N)))
    SH[rng.random((T_m, N)) < 0.03] = 0.0
    SH[rng.random((T_m, N)) < 0.03] = np.nan
    _CACHE[key] = dict(P=P, V=V, ms=ms, SH=SH, ref=LR.liq_sums(P, V, ms, max_gap), mod={},
                       max_gap=max_gap, days=pan["days"], tickers=pan["tickers"])
    return _CACHE[key]


def _panel(N, kind="gappy", max_gap=10):
    pan = _host(N, kind, max_gap)
    if "Pd" not in pan:
        pan.update(Pd=_up(pan["P"]), Vd=_up(pan["V"]), msd=_up(pan["ms"]), SHd=_up(pan["SH"]))
    return pan


def _model_ref(pan, Wm, min_obs, sh=True):
    key = (Wm, min_obs, sh)
    if key not in pan["mod"]:
        pan["mod"][key] = LR.liq_model(pan["ref"], Wm, min_obs, 1e6, pan["SH"] if sh else None)
    return pan["mod"][key]


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


def _check_sums(sums, ref):
    for k in LR.COUNTS:
        assert np.array_equal(getattr(sums, k).cpu().numpy(), ref[k]), k
    for k in LR.FSUMS:
        assert bits_equal(getattr(sums, k).cpu().numpy(), ref[k]), k


def _check_model(mod, ref, tag, keys=LR.MODEL[:5]):
    if mod.NOBS is not None:
        assert np.array_equal(mod.NOBS.cpu().numpy(), ref["NOBS"]), "NOBS"
    for k in keys:
        assert _ulps(getattr(mod, k).cpu().numpy(), ref[k], f"{k}{tag}") <= MAX_ULP, k


MODELS = ((1, None), (3, None), (12, None), (3, 1))


def _tune(key, value):
    import csmom
    assert csmom.load_library().csm_tune(key.encode(), ctypes.c_int(value)) == 0


def _run(engine, pan, Pd=None, Vd=None, models=MODELS):
    """liq_sums at one and at two assets per lane, then the models on the default's panels."""
    Pd = pan["Pd"] if Pd is None else Pd
    Vd = pan["Vd"] if Vd is None else Vd
    try:
        for pair in reversed(PAIR):
            _tune("lsums_pair", pair)
            sums = engine.liq_sums(Pd, Vd, pan["msd"], pan["max_gap"])
            _check_sums(sums, pan["ref"])
    finally:
        _tune("lsums_pair", 0)
    for Wm, mo in models:
        mod = engine.liq_model(sums, Wm, mo, SH=pan["SHd"])
        _check_model(mod, _model_ref(pan, Wm, mo), f"(Wm={Wm}, min_obs={mo})")
    return sums


def _defined(pan, Wm):
    """Share of the cells from month Wm - 1 on with ILLIQ defined at the default min_obs."""
    return float((~np.isnan(_model_ref(pan, Wm, None)["ILLIQ"][Wm - 1:])).mean())


def _classes(pan):
    """Cells of each class the rules tell apart, on the reference arrays."""
    P, V, R = pan["P"], pan["V"], pan["ref"]["R"]
    priced = ~np.isnan(P)
    return dict(zero_return=int((R == 0.0).sum()),
                zero_volume_priced=int((priced & (V == 0.0)).sum()),
                nan_volume_priced=int((priced & np.isnan(V)).sum()),
                volume_unpriced=int((~priced & (V > 0.0)).sum()))


@pytest.mark.parametrize("N", SIZES)
def test_vs_ref_gappy(engine, N):
    pan = _panel(N)
    _run(engine, pan)
    if N >= 2:
        for Wm in (1, 3, 12):
            assert _defined(pan, Wm) >= 0.5, Wm
    if N >= 63:
        c = _classes(pan)
        print(c)
        assert min(c.values()) >= 1, c
        ref = pan["ref"]
        assert (ref["NA"] < ref["ND"]).any() and (ref["ND"] < ref["NP"]).any()


@pytest.mark.parametrize("N", [63, 130])
def test_vs_ref_dense(engine, N):
    pan = _panel(N, "dense")
    _run(engine, pan)
    assert _defined(pan, 1) >= 0.5 and _defined(pan, 12) >= 0.5
    assert (pan["ref"]["NP"] == np.diff(pan["ms"])[:, None]).all()       # every day priced
    assert (pan["ref"]["ND"][1:] == np.diff(pan["ms"])[1:, None]).all()  # and a return every day


@pytest.mark.parametrize("max_gap", [1, 3, 10])
def test_max_gap(engine, max_gap):
    """The bound itself (gappy rows), and for max_gap >= 2 the hand-built column whose gaps are
    one under, at and one over the bound."""
    pan = _panel(257, "gappy" if max_gap == 1 else "gaps", max_gap)
    _run(engine, pan)
    assert _defined(pan, 1) >= 0.5
    r = pan["ref"]["R"]
    if max_gap > 1:
        _, cases = DR.gap_column(T_DAYS, max_gap, int(pan["ms"][8]), O.absent_scalar())
        assert [not np.isnan(r[d, GAP_COL]) for d, _, _ in cases] == [b for _, _, b in cases]
    else:   # a return needs the row before it
        priced = ~np.isnan(pan["P"])
        assert np.array_equal(~np.isnan(r[1:]), priced[1:] & priced[:-1])


@pytest.mark.parametrize("kind", ["zero", "calendar", "columns"])
def test_calendars_and_empty_columns(engine, kind):
    pan = _panel(130, kind)
    sums = _run(engine, pan)
    assert _defined(pan, 1) >= 0.5
    if kind == "zero":
        for k in LR.SUMS:
            assert (getattr(sums, k)[4] == 0).all(), k
    if kind == "calendar":
        assert int(engine.month_days(pan["msd"])[0]) == 31
    if kind == "columns":
        assert (sums.NP[:, 3:5] == 0).all() and (sums.SV[:, 3:5] == 0).all()
        mod = engine.liq_model(sums, 1, 1)
        assert torch.isnan(mod.DVOL[:, 3:5]).all() and not torch.isnan(mod.DVOL[:, 5]).all()


@pytest.mark.parametrize("which", ["P", "V"])
def test_unaligned_panel_takes_the_one_asset_path(engine, which):
    """Even N with one panel through a view 8 B past a 16-B boundary: under "lsums_pair" = 1 too
    the call takes one asset per lane, and the bits are the paired path's."""
    pan = _panel(514)
    T_d, N = pan["P"].shape
    flat = torch.empty(T_d * N + 1, dtype=torch.float64, device="cuda:0")
    view = flat[1:].view(T_d, N)
    view.copy_(pan["Pd" if which == "P" else "Vd"])
    assert pan["Pd"].data_ptr() % 16 == 0 and pan["Vd"].data_ptr() % 16 == 0
    assert view.data_ptr() % 16 == 8
    _run(engine, pan, **{which + "d": view}, models=((1, None),))


def _raw(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else t.dtype)


def _same(xs, ys):
    return all(torch.equal(_raw(a), _raw(b)) for a, b in zip(xs, ys))


@pytest.mark.parametrize("N,kind", [(257, "gaps"), (514, "gappy"), (130, "zero")])
def test_launch_shape_changes_no_bit(engine, N, kind):
    pan = _panel(N, kind)
    T_m = len(pan["ms"]) - 1
    try:
        base = _run(engine, pan, models=())
        for pair in PAIR:
            _tune("lsums_pair", pair)
            for chunks in (1, 5, T_m, 0):
                _tune("lsums_chunks", chunks)
                got = engine.liq_sums(pan["Pd"], pan["Vd"], pan["msd"], pan["max_gap"])
                assert _same(got, base), (pair, chunks)
        for Wm in (1, 3, 12):
            _tune("lmodel_chunks", 0)
            want = engine.liq_model(base, Wm, SH=pan["SHd"])
            _check_model(want, _model_ref(pan, Wm, None), f"(Wm={Wm})")
            for chunks in (1, 5, T_m):
                _tune("lmodel_chunks", chunks)
                got = engine.liq_model(base, Wm, SH=pan["SHd"])
                assert _same([getattr(got, k) for k in LR.MODEL],
                             [getattr(want, k) for k in LR.MODEL]), (Wm, chunks)
    finally:
        for k in ("lsums_pair", "lsums_chunks", "lmodel_chunks"):
            _tune(k, 0)


def test_twice_the_same_bits(engine):
    pan = _panel(514)
    a, b = _run(engine, pan, models=((12, None),)), _run(engine, pan, models=((12, None),))
    assert _same(a, b)


def test_nullable_outputs_and_subsets(engine):
    pan = _panel(257)
    full = _run(engine, pan, models=())
    slim = engine.liq_sums(pan["Pd"], pan["Vd"], pan["msd"], with_sv=False, with_nzr=False,
                           with_nzv=False)
    assert slim.SV is None and slim.NZR is None and slim.NZV is None
    keep = ("NP", "ND", "NA", "SDV", "SIL")
    assert _same([getattr(slim, k) for k in keep], [getattr(full, k) for k in keep])
    mod = engine.liq_model(slim, 3, SH=pan["SHd"])   # the default: what the sums given allow
    assert mod.TURN is None and mod.ZRET is None and mod.ZVOL is None
    _check_model(mod, _model_ref(pan, 3, None), "(slim)", keys=("ILLIQ", "DVOL"))
    # without SH: no TURN by default, and the other outputs do not move
    mod = engine.liq_model(full, 3)
    assert mod.TURN is None
    _check_model(mod, _model_ref(pan, 3, None, sh=False), "(no SH)",
                 keys=("ILLIQ", "DVOL", "ZRET", "ZVOL"))
    # subsets, one output at a time
    ref = _model_ref(pan, 12, None)
    for k in LR.MODEL:
        one = engine.liq_model(full, 12, SH=pan["SHd"], outputs=(k,))
        assert [f for f in LR.MODEL if getattr(one, f) is not None] == [k]
        if k == "NOBS":
            assert np.array_equal(one.NOBS.cpu().numpy(), ref["NOBS"])
        else:
            assert _ulps(getattr(one, k).cpu().numpy(), ref[k], f"{k} alone") <= MAX_ULP
    # TURN's cells without shares are undefined, the others are not
    turn = _model_ref(pan, 1, 1)["TURN"]
    bad = ~(pan["SH"] > 0)
    assert bad.sum() >= 10 and np.isnan(turn[bad]).all() and not np.isnan(turn[~bad]).all()
    # scale multiplies once
    two = engine.liq_model(full, 12, scale=2e6, outputs=("ILLIQ",)).ILLIQ.cpu().numpy()
    assert bits_equal(two, LR.liq_model(pan["ref"], 12, None, 2e6)["ILLIQ"])


def _ranking(out, ref, PM):
    NRr = SR.next_ret(PM, ref)
    assert bits_equal(out.NR.cpu().numpy(), NRr)
    Lr = O.assign_deciles(ref, 10)
    EWr, CNTr, LSr = O.portfolio_ew(Lr, NRr, 10)
    assert np.array_equal(out.L.cpu().numpy(), Lr)
    assert np.array_equal(out.CNT.cpu().numpy(), CNTr)
    for got, want in ((out.EW, EWr), (out.LS, LSr)):
        g = got.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(want))
        assert max_rel(g, want) <= 1e-10
    return LSr


@pytest.mark.parametrize("signal", ["illiq", "dvol", "zret"])
def test_run_signal(engine, signal):
    pan = _panel(257)
    ref = _model_ref(pan, 12, None)[engine.LIQ_SIGNALS[signal]]
    if "PM" not in pan:
        pan["PM"] = SR.month_stats(pan["P"], pan["ms"])["PM"]
    out = engine.run_signal(pan["Pd"], pan["msd"], signal, V=pan["Vd"])
    assert bits_equal(out.PM.cpu().numpy(), pan["PM"])
    assert _ulps(out.M.cpu().numpy(), ref, signal) <= MAX_ULP
    LSr = _ranking(out, ref, pan["PM"])
    assert (~np.isnan(LSr)).sum() >= 36 - 12 - 1
    if signal == "illiq":   # an explicit window and min_obs reach the model
        o3 = engine.run_signal(pan["Pd"], pan["msd"], signal, window=3, min_obs=40, V=pan["Vd"])
        assert bits_equal(o3.M.cpu().numpy(), _model_ref(pan, 3, 40)["ILLIQ"])


def test_run_signal_refusals_and_old_calls(engine):
    pan = _panel(63)
    Pd, msd, Vd = pan["Pd"], pan["msd"], pan["Vd"]
    for signal in ("illiq", "dvol", "zret"):
        with pytest.raises(ValueError):
            engine.run_signal(Pd, msd, signal)
    FD = torch.zeros((Pd.shape[0], 1), dtype=torch.float64, device="cuda:0")
    with pytest.raises(ValueError):
        engine.run_signal(Pd, msd, "illiq", V=Vd, factors=FD)
    with pytest.raises(ValueError):
        engine.run_signal(Pd, msd, "dbeta", V=Vd, factors=FD)
    with pytest.raises(ValueError):
        engine.run_signal(Pd, msd, "amihud", V=Vd)
    a, b = engine.run_signal(Pd, msd, "divol"), engine.run_signal(Pd, msd, "divol", V=Vd)
    assert _same([a.M, a.NR, a.EW], [b.M, b.NR, b.EW])       # V changes no other signal
    assert engine.RUN_SIGNALS[-3:] == ("illiq", "dvol", "zret")


def test_build_signals(engine):
    from csmom.regress import SIGNAL_NAMES, build_signals
    pan = _panel(257)
    names = ("illiq", "rev", "zret", "dvol")
    S, X = build_signals(engine, pan["Pd"], pan["msd"], names, V=pan["Vd"])
    ref = _model_ref(pan, 12, None)
    for n, s in zip(names, S):
        if n != "rev":
            assert bits_equal(s.cpu().numpy(), ref[engine.LIQ_SIGNALS[n]]), n
    assert torch.equal(_raw(S[1]), _raw(X))
    S3, _ = build_signals(engine, pan["Pd"], pan["msd"], ("dvol",), window=3, V=pan["Vd"])
    assert bits_equal(S3[0].cpu().numpy(), _model_ref(pan, 3, None)["DVOL"])
    with pytest.raises(ValueError):
        build_signals(engine, pan["Pd"], pan["msd"], ("illiq",))
    assert set(engine.LIQ_SIGNALS) <= set(SIGNAL_NAMES)


def _frame(pan):
    return to_long(dict(P=pan["P"], V=pan["V"], days=pan["days"], tickers=pan["tickers"]))


def test_liquidity_signals_from_a_daily_frame(engine):
    import csmom
    from csmom.panel import from_long
    pan = _panel(63)
    df = _frame(pan)
    dense = from_long(df)        # the frame's own dense layout: no row is volume 0, NaN volume is 0
    ref = LR.liq_model(LR.liq_sums(dense.P, dense.V, dense.month_start), 3, 30, 1e6)
    got = csmom.liquidity_signals(df, window=3, min_obs=30, device=0)
    assert list(got.columns) == csmom.LIQUIDITY_COLUMNS
    PM = SR.month_stats(dense.P, dense.month_start)["PM"]
    aa, mm = np.nonzero(~O.is_absent(PM).T)
    assert len(got) == len(aa) and (got["ticker"].to_numpy() == dense.tickers[aa]).all()
    assert (got["date"].to_numpy() == dense.month_end[mm].to_numpy()).all()
    for col, k in (("illiq", "ILLIQ"), ("dvol", "DVOL"), ("zret", "ZRET"), ("zvol", "ZVOL")):
        assert bits_equal(got[col].to_numpy(), ref[k][mm, aa]), col
    assert np.array_equal(got["nobs"].to_numpy(), ref["NOBS"][mm, aa])
    assert got["illiq"].notna().mean() >= 0.5
    assert csmom.liquidity_signals(df.iloc[:0], device=0) is None


def test_tables_from_a_daily_frame(engine):
    """fama_macbeth, information_coefficient and neutral_momentum take the liquidity names."""
    import csmom
    pan = _panel(130)
    df = _frame(pan)
    fm = csmom.fama_macbeth(df, signals=("rev", "illiq", "zret"), device=0)
    assert list(fm.table.index) == ["const", "rev", "illiq", "zret"]
    assert np.isfinite(fm.table[["mean", "se", "t"]].to_numpy()).all()
    assert (fm.table["months"] >= 20).all()
    ic = csmom.information_coefficient(df, signals=("dvol",), horizons=(1, 3), device=0)
    assert np.isfinite(ic.table[["mean", "se", "t"]].to_numpy()).all() and len(ic.table) == 2
    groups = {t: i % 3 for i, t in enumerate(pan["tickers"])}
    nm = csmom.neutral_momentum(df, groups, n_bins=5, signal="illiq", device=0)
    assert len(nm.long_short) >= 20 and np.isfinite(nm.mean)
    base = csmom.neutral_momentum(df, groups, n_bins=5, device=0)    # "mom": no volume needed
    assert len(base.long_short) >= 20


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
    Pd, Vd, msd = pan["Pd"], pan["Vd"], pan["msd"]
    T_d, N = Pd.shape
    T_m = msd.numel() - 1
    ints = [torch.full((T_m, N), 77, dtype=torch.int32, device="cuda:0") for _ in range(5)]
    f = [torch.full((T_m, N), SENTINEL, dtype=torch.float64, device="cuda:0") for _ in range(3)]

    def sums(P=Pd, V=Vd, ms=msd, tm=T_m, mmd=23, gap=10, o=range(8), td=T_d):
        ptrs = [_ptr(t) if i in o else None for i, t in enumerate(ints + f)]
        return (_ptr(P), _ptr(V), td, N, _ptr(ms), tm, mmd, gap, *ptrs)

    bad = [sums(gap=0), sums(gap=33), sums(mmd=0), sums(mmd=33), sums(tm=0), sums(td=0),
           sums(P=None), sums(V=None), sums(ms=None)]
    bad += [sums(o=[j for j in range(8) if j != i]) for i in (0, 1, 2, 6, 7)]   # the required ones
    for args in bad:
        _refused(engine, "csm_liq_sums", args, ints + f)
    for kw in (dict(max_gap=0), dict(max_gap=33)):
        with pytest.raises(csmom.CsmError):
            engine.liq_sums(Pd, Vd, msd, **kw)

    s = engine.liq_sums(Pd, Vd, msd)
    ins = [_ptr(t) for t in s] + [_ptr(pan["SHd"])]
    g = [torch.full((T_m, N), SENTINEL, dtype=torch.float64, device="cuda:0") for _ in range(5)]
    nobs = torch.full((T_m, N), 77, dtype=torch.int32, device="cuda:0")

    def model(ins=ins, tm=T_m, Wm=1, mo=15, scale=1e6, o=range(6)):
        ptrs = [_ptr(t) if i in o else None for i, t in enumerate(g + [nobs])]
        return (*ins, tm, N, Wm, mo, scale, *ptrs)

    def without(i):
        return ins[:i] + [None] + ins[i + 1:]

    bad = [model(Wm=0), model(Wm=13), model(mo=0), model(tm=0), model(o=()), model(scale=0.0),
           model(scale=-1.0), model(scale=float("inf")), model(scale=float("nan")),
           model(ins=without(5)), model(ins=without(8)),       # TURN without SV, without SH
           model(ins=without(3)), model(ins=without(4)),       # ZRET without NZR, ZVOL without NZV
           model(ins=without(8), o=(2,))]
    bad += [model(ins=without(i)) for i in (0, 1, 2, 6, 7)]
    for args in bad:
        _refused(engine, "csm_liq_model", args, g + [nobs])
    # without the nullable inputs the other outputs are served
    engine._call("csm_liq_model", *ins[:3], None, None, None, *ins[6:8], None, T_m, N, 1, 15, 1e6,
                 _ptr(g[0]), _ptr(g[1]), None, None, None, None)
    ref = _model_ref(pan, 1, 15)
    assert bits_equal(g[0].cpu().numpy(), ref["ILLIQ"]) and bits_equal(g[1].cpu().numpy(),
                                                                      ref["DVOL"])
    for kw in (dict(window=0), dict(window=13), dict(min_obs=0), dict(scale=0.0)):
        with pytest.raises(csmom.CsmError) as e:
            engine.liq_model(s, **kw)
        assert e.value.status == -1
    with pytest.raises(ValueError):
        engine.liq_model(s, outputs=("ILLIQ", "XX"))
    with pytest.raises(csmom.CsmError):
        engine.liq_model(s, outputs=("TURN",))     # no SH
