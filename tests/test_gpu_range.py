"""GPU: csm_range_sums / csm_range_model, Engine.run_signal's "pkvol", "cs_spread", "ar_spread" and
the host entries on them (rules HL1..HL6 in DESIGN.md 7) against the restatement in
tests/range_ref.py.

Bars.  The counts NRG, NPR, NCS, NOBS and every NaN pattern are exact.  The float sums cannot be
bit-exact against the host: the device's log / exp are OCML's, the reference's are the host
libm's, and h - l and c - eta cancel.  They are held to |got - ref| <= 1e-10 * scale with the
reference's scale for that sum (range_ref's docstring); 1e-10 is the project's bar for values that
are not bit-exact, and two logs of about 1 ulp each on log-prices of order 5 against ranges of
order 1e-2 put the expected worst near 1e-13 of the scale.  The largest |got - ref| / scale per sum
is printed.  Any chunk count and any lead-in give the same device bits as one chunk (device against
device).  range_model is + * / sqrt only, correctly rounded in this build (as test_gpu_signals.py
records): on the device's own sums, downloaded, it equals range_ref.range_model bit for bit
(MAX_ULP = 0, the maximum found is printed).  Labels and counts of the ranking are exact, EW / LS
within 1e-10.

Panels: C is make_panel's price panel with its ABSENT / NaN cells; H = C exp(sigma |z1|) and
L = C exp(-sigma |z2|) rounded to cents from a seeded rng; about 1 % more NaN in each of H and L;
about 0.5 % of the rows with L > C and as many with H < C; a few rows with L = 0; about 2 % of the
rows with a range of 0.1 % around the close, so that the day lies wholly above or below the close
before it (overnight moves of both signs; many more arise by themselves).  Column TINY trades
near 0.02.  That alone cannot drive the shifted low to zero -- L* = L - (L - C') is C' up to
rounding -- so every 40th row of the column closes at 1e-18, under half an ulp of the next low:
those pairs have L* = 0, a NaN spread, and count in NPR and not in NCS.
"""
import ctypes
import tarfile

import numpy as np
import pytest
import torch

import dailymkt_ref as DR
import range_ref as RR
import signals_ref as SR
from conftest import GOLDEN, bits_equal, max_rel
from oracle import csmom_oracle as O
from oracle.synth_np import make_panel

pytestmark = pytest.mark.gpu
T_DAYS = 782            # 36 whole business-day months of 19..23 rows from 2000-01-03
GAPPY = dict(late=0.2, delist=0.2, nan_day=0.01, absent_month=0.01, nan_month=0.01)
DENSE = dict(late=0, delist=0, nan_day=0, absent_month=0, nan_month=0)
BAR = 1e-10             # see the module docstring
MAX_ULP = 0
TINY = 2                # the column near 0.02
GAP_COL = 5             # the hand-built column of the "gaps" panels
SIZES = [1, 2, 63, 130, 257]   # odd and even, a partial wave, a second workgroup
CHUNKS = (1, 3, 7, 36)
MODELS = ((1, None), (3, None), (12, None), (3, 1))
_CACHE = {}


def _up(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _tune(key, value):
    import csmom
    assert csmom.load_library().csm_tune(key.encode(), ctypes.c_int(value)) == 0


def _hlc(P, seed, sigma=0.015):
    """(H, L, C) as the module docstring describes them."""
    rng = np.random.default_rng(seed)
    T_d, N = P.shape
    C = P.copy()
    with np.errstate(invalid="ignore"):
        H = np.round(C * np.exp(sigma * np.abs(rng.standard_normal(P.shape))), 2)
        L = np.round(C * np.exp(-sigma * np.abs(rng.standard_normal(P.shape))), 2)
        tight = rng.random(P.shape) < 0.02
        H[tight], L[tight] = np.round(C * 1.001, 2)[tight], np.round(C * 0.999, 2)[tight]
        low_over = rng.random(P.shape) < 0.005
        L[low_over] = np.round(C * 1.01 + 0.01, 2)[low_over]
        high_under = rng.random(P.shape) < 0.005
        H[high_under] = np.round(C * 0.99 - 0.01, 2)[high_under]
    H[rng.random(P.shape) < 0.01] = np.nan
    L[rng.random(P.shape) < 0.01] = np.nan
    L[rng.integers(0, T_d, 6), rng.integers(0, N, 6)] = 0.0
    if N > TINY:
        d = np.arange(T_d)
        c = 0.02 + 0.01 * (d % 3)
        C[:, TINY], H[:, TINY], L[:, TINY] = c, c + 0.01, np.maximum(c - 0.01, 0.01)
        C[::40, TINY], H[::40, TINY], L[::40, TINY] = 1e-18, 2e-18, 1e-18
    return H, L, C


def _host(N, kind="gappy", max_gap=1):
    """Host panels and the HL1..HL5 reference; computed once and left unchanged."""
    key = (N, kind, max_gap)
    if key in _CACHE:
        return _CACHE[key]
    pan = make_panel(N, T_DAYS, seed=400 + N, cents=True, with_volume=False,
                     **(DENSE if kind == "dense" else GAPPY))
    ms = pan["month_start"]
    d = np.diff(ms)
    assert len(ms) - 1 == 36 and d.min() >= 19 and d.max() <= 23
    H, L, C = _hlc(pan["P"], 700 + N)
    if kind == "zero":       # month 4 has no day
        ms = np.concatenate([ms[:5], ms[4:]])
    if kind == "columns":    # a column that is never ranged, and one without any row
        H[:, 3] = np.nan
        for X in (H, L, C):
            X[:, 4] = O.absent_like(T_DAYS)
    if kind == "gaps":       # dailymkt_ref.gap_column: gaps around max_gap, one across month 12's
        col, _ = DR.gap_column(T_DAYS, max_gap, int(ms[12]), O.absent_scalar())   # start
        with np.errstate(invalid="ignore"):
            C[:, GAP_COL] = np.round(col, 2)
            H[:, GAP_COL] = np.round(C[:, GAP_COL] * 1.01, 2)
            L[:, GAP_COL] = np.round(C[:, GAP_COL] * 0.99, 2)
    _CACHE[key] = dict(P=pan["P"], H=H, L=L, C=C, ms=ms, max_gap=max_gap, mod={},
                       ref=RR.range_sums(H, L, C, ms, max_gap))
    return _CACHE[key]


def _panel(N, kind="gappy", max_gap=1):
    pan = _host(N, kind, max_gap)
    if "Hd" not in pan:
        pan.update(Hd=_up(pan["H"]), Ld=_up(pan["L"]), Cd=_up(pan["C"]), msd=_up(pan["ms"]),
                   Pd=_up(pan["P"]))
    return pan


def _np(sums):
    return {k: getattr(sums, k).cpu().numpy() for k in RR.SUMS if getattr(sums, k) is not None}


def _check_sums(sums, ref, tag, keys=RR.SUMS):
    got = _np(sums)
    worst = {}
    for k in keys:
        if k in RR.COUNTS:
            assert np.array_equal(got[k], ref[k]), k
            continue
        assert not np.isnan(got[k]).any(), k
        scale = ref[k + "_scale"]
        err = np.abs(got[k] - ref[k])
        assert (err[scale == 0.0] == 0.0).all(), k
        rel = float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0
        print(f"{k}{tag}: max |got - ref| / scale = {rel:.3e}")
        worst[k] = rel
        assert rel <= BAR, (k, rel)
    return worst


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


def _check_model(mod, ref, tag, keys=RR.MODEL[:3]):
    if mod.NOBS is not None:
        assert np.array_equal(mod.NOBS.cpu().numpy(), ref["NOBS"]), "NOBS"
    for k in keys:
        assert _ulps(getattr(mod, k).cpu().numpy(), ref[k], f"{k}{tag}") <= MAX_ULP, k


def _run(engine, pan, views=None, models=MODELS, tag=""):
    """range_sums against the reference, then the models on the device's own sums."""
    Hd, Ld, Cd = views or (pan["Hd"], pan["Ld"], pan["Cd"])
    sums = engine.range_sums(Hd, Ld, Cd, pan["msd"], pan["max_gap"])
    _check_sums(sums, pan["ref"], tag)
    own = _np(sums)
    for Wm, mo in models:
        mod = engine.range_model(sums, Wm, mo)
        _check_model(mod, RR.range_model(own, Wm, mo), f"(Wm={Wm}, min_obs={mo})")
    return sums


def _classes(pan):
    """Cells of each class the rules tell apart, on the host arrays."""
    H, L, C = pan["H"], pan["L"], pan["C"]
    with np.errstate(invalid="ignore"):
        rg = (L > 0) & (H >= L) & (L <= C) & (C <= H)
        both = rg[1:] & rg[:-1]
        return dict(h_nan=int((np.isnan(H) & ~np.isnan(L) & ~np.isnan(C)).sum()),
                    l_nan=int((np.isnan(L) & ~np.isnan(H) & ~np.isnan(C)).sum()),
                    c_nan=int(np.isnan(C).sum()), c_absent=int(O.is_absent(C).sum()),
                    low_over_close=int((L > C).sum()), high_under_close=int((H < C).sum()),
                    high_under_low=int((H < L).sum()), low_zero=int((L == 0.0).sum()),
                    shift_up=int((both & (L[1:] > C[:-1])).sum()),
                    shift_down=int((both & (H[1:] < C[:-1])).sum()),
                    no_shift=int((both & (L[1:] <= C[:-1]) & (H[1:] >= C[:-1])).sum()),
                    spread_nan=int((pan["ref"]["NPR"] - pan["ref"]["NCS"]).sum()),
                    spread_floored=int((pan["ref"]["SCS"] == 0.0).sum()))


def _defined(pan, Wm, k="CSSPR"):
    """Share of the cells from month Wm - 1 on with k defined at the default min_obs."""
    if Wm not in pan["mod"]:
        pan["mod"][Wm] = RR.range_model(pan["ref"], Wm)
    return float((~np.isnan(pan["mod"][Wm][k][Wm - 1:])).mean())


@pytest.mark.parametrize("N", SIZES)
def test_vs_ref_gappy(engine, N):
    pan = _panel(N)
    _run(engine, pan)
    if N >= 63:
        for Wm in (1, 3, 12):
            assert _defined(pan, Wm) >= 0.4, Wm
        c = _classes(pan)
        print(c)
        assert min(c.values()) >= 1, c
        assert c["shift_up"] >= 0.02 * pan["C"].size / 4 and c["shift_down"] >= 0.02 * pan["C"].size / 4
        ref = pan["ref"]
        assert (ref["NCS"][:, TINY] < ref["NPR"][:, TINY]).any()
        assert (ref["NPR"] < ref["NRG"]).any()


@pytest.mark.parametrize("kind", ["dense", "columns", "zero"])
def test_kinds(engine, kind):
    pan = _panel(130, kind)
    sums = _run(engine, pan, models=((1, None), (12, 1)))
    assert _defined(pan, 1) >= 0.4
    if kind == "zero":
        for k in RR.SUMS:
            assert (getattr(sums, k)[4] == 0).all(), k
    if kind == "columns":
        assert (sums.NRG[:, 3:5] == 0).all() and (sums.NPR[:, 3:5] == 0).all()
        assert (sums.SPK[:, 3:5] == 0).all() and (sums.SAR[:, 3:5] == 0).all()
        mod = engine.range_model(sums, 1, 1)
        assert torch.isnan(mod.PKVOL[:, 3:5]).all() and not torch.isnan(mod.PKVOL[:, 5]).all()
        assert (mod.NOBS[:, 3:5] == 0).all()


@pytest.mark.parametrize("max_gap", [1, 3, 10])
def test_max_gap(engine, max_gap):
    """The bound itself (gappy rows), and for max_gap >= 2 the hand-built column whose gaps are
    one under, at and one over the bound."""
    pan = _panel(130, "gappy" if max_gap == 1 else "gaps", max_gap)
    _run(engine, pan, models=((1, None),))
    if max_gap > 1:
        _, cases = DR.gap_column(T_DAYS, max_gap, int(pan["ms"][12]), O.absent_scalar())
        cols = [pan[k][:, GAP_COL:GAP_COL + 1] for k in "HLC"]
        npr = RR.range_sums(*cols, np.arange(T_DAYS + 1), max_gap)["NPR"][:, 0]   # a month a day
        assert [int(npr[d]) for d, _, _ in cases] == [int(b) for _, _, b in cases]


def _raw(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else t.dtype)


def _same(xs, ys):
    return all(torch.equal(_raw(a), _raw(b)) for a, b in zip(xs, ys))


@pytest.mark.parametrize("N,kind,max_gap", [(257, "gaps", 3), (130, "gaps", 10), (130, "zero", 1),
                                            (63, "gappy", 1)])
def test_launch_shape_changes_no_bit(engine, N, kind, max_gap):
    """Every chunk count, and so every lead-in, against one chunk: device against device.  With 36
    chunks month 12's start, which the gap column's last gap lies across, is a chunk start; with 3
    it is one too."""
    pan = _panel(N, kind, max_gap)
    T_m = len(pan["ms"]) - 1
    args = (pan["Hd"], pan["Ld"], pan["Cd"], pan["msd"], max_gap)
    try:
        _tune("rsums_chunks", 1)
        base = engine.range_sums(*args)
        _check_sums(base, pan["ref"], "(one chunk)")
        for chunks in CHUNKS + (T_m, 0):
            _tune("rsums_chunks", chunks)
            assert _same(engine.range_sums(*args), base), chunks
        for Wm in (1, 3, 12):
            _tune("rmodel_chunks", 0)
            want = engine.range_model(base, Wm)
            for chunks in (1, 5, T_m):
                _tune("rmodel_chunks", chunks)
                got = engine.range_model(base, Wm)
                assert _same([getattr(got, k) for k in RR.MODEL],
                             [getattr(want, k) for k in RR.MODEL]), (Wm, chunks)
    finally:
        for k in ("rsums_chunks", "rmodel_chunks"):
            _tune(k, 0)


def test_twice_the_same_bits_and_unaligned_views(engine):
    """The panels through views 8 B past a 16-B boundary give the aligned call's bits."""
    pan = _panel(130)
    a, b = _run(engine, pan, models=()), _run(engine, pan, models=())
    assert _same(a, b)
    T_d, N = pan["H"].shape
    views = []
    for k in ("Hd", "Ld", "Cd"):
        flat = torch.empty(T_d * N + 1, dtype=torch.float64, device="cuda:0")
        v = flat[1:].view(T_d, N)
        v.copy_(pan[k])
        assert pan[k].data_ptr() % 16 == 0 and v.data_ptr() % 16 == 8
        views.append(v)
    assert _same(_run(engine, pan, views=views, models=()), a)


def test_nullable_outputs_and_subsets(engine):
    pan = _panel(257)
    full = _run(engine, pan, models=())
    args = (pan["Hd"], pan["Ld"], pan["Cd"], pan["msd"])
    no_cs = engine.range_sums(*args, with_cs=False)
    assert no_cs.NCS is None and no_cs.SCS is None and no_cs.SAR is not None
    no_ar = engine.range_sums(*args, with_ar=False)
    assert no_ar.SAR is None and no_ar.SCS is not None
    slim = engine.range_sums(*args, with_cs=False, with_ar=False)
    assert slim.NCS is None and slim.SCS is None and slim.SAR is None
    for part, keys in ((no_cs, ("NRG", "NPR", "SPK", "SAR")), (slim, ("NRG", "NPR", "SPK")),
                       (no_ar, ("NRG", "NPR", "NCS", "SPK", "SCS"))):
        assert _same([getattr(part, k) for k in keys], [getattr(full, k) for k in keys]), keys
    own = _np(full)
    ref = RR.range_model(own, 3)
    mod = engine.range_model(slim, 3)            # the default: what the sums given allow
    assert mod.CSSPR is None and mod.ARSPR is None
    _check_model(mod, ref, "(slim)", keys=("PKVOL",))
    mod = engine.range_model(no_cs, 3)
    assert mod.CSSPR is None
    _check_model(mod, ref, "(no cs)", keys=("PKVOL", "ARSPR"))
    for k in RR.MODEL:                            # subsets, one output at a time
        one = engine.range_model(full, 3, outputs=(k,))
        assert [f for f in RR.MODEL if getattr(one, f) is not None] == [k]
        if k == "NOBS":
            assert np.array_equal(one.NOBS.cpu().numpy(), ref["NOBS"])
        else:
            assert _ulps(getattr(one, k).cpu().numpy(), ref[k], f"{k} alone") <= MAX_ULP
    ar = ref["ARSPR"]
    assert (ar == 0.0).any() and (ar > 0.0).any()          # m <= 0 gives 0.0, not NaN


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


@pytest.mark.parametrize("signal", ["pkvol", "cs_spread", "ar_spread"])
def test_run_signal(engine, signal):
    pan = _panel(257)
    HLC = (pan["Hd"], pan["Ld"], pan["Cd"])
    field = engine.RANGE_SIGNALS[signal]
    sums = engine.range_sums(*HLC, pan["msd"])
    want = getattr(engine.range_model(sums, 1), field)
    if "PM" not in pan:
        pan["PM"] = SR.month_stats(pan["P"], pan["ms"])["PM"]
    out = engine.run_signal(pan["Pd"], pan["msd"], signal, HLC=HLC)
    assert bits_equal(out.PM.cpu().numpy(), pan["PM"])
    assert torch.equal(_raw(out.M), _raw(want))
    M = out.M.cpu().numpy()
    assert bits_equal(M, RR.range_model(_np(sums), 1)[field])
    LSr = _ranking(out, M, pan["PM"])
    assert (~np.isnan(LSr)).sum() >= 30
    o3 = engine.run_signal(pan["Pd"], pan["msd"], signal, window=3, min_obs=40, HLC=HLC)
    assert torch.equal(_raw(o3.M), _raw(getattr(engine.range_model(sums, 3, 40), field)))


def test_run_signal_refusals_and_old_calls(engine):
    pan = _panel(63)
    Pd, msd = pan["Pd"], pan["msd"]
    HLC = (pan["Hd"], pan["Ld"], pan["Cd"])
    for signal in ("pkvol", "cs_spread", "ar_spread"):
        with pytest.raises(ValueError):
            engine.run_signal(Pd, msd, signal)
    FD = torch.zeros((Pd.shape[0], 1), dtype=torch.float64, device="cuda:0")
    V = torch.ones_like(Pd)
    with pytest.raises(ValueError):
        engine.run_signal(Pd, msd, "pkvol", HLC=HLC, factors=FD)
    with pytest.raises(ValueError):
        engine.run_signal(Pd, msd, "dbeta", HLC=HLC, factors=FD)
    with pytest.raises(ValueError):
        engine.run_signal(Pd, msd, "cs_spread", HLC=HLC, V=V)
    with pytest.raises(ValueError):
        engine.run_signal(Pd, msd, "parkinson", HLC=HLC)
    a, b = engine.run_signal(Pd, msd, "divol"), engine.run_signal(Pd, msd, "divol", HLC=HLC)
    assert _same([a.M, a.NR, a.EW], [b.M, b.NR, b.EW])      # HLC changes no other signal
    from csmom.regress import build_signals
    with pytest.raises(ValueError):
        build_signals(engine, Pd, msd, ("pkvol",))
    S, X = build_signals(engine, Pd, msd, ("ar_spread", "rev", "pkvol"), HLC=HLC)
    rm = engine.range_model(engine.range_sums(*HLC, msd), 1)
    assert _same([S[0], S[2], S[1]], [rm.ARSPR, rm.PKVOL, X])
    GID = torch.from_numpy((np.arange(Pd.shape[1]) % 3).astype(np.int16)).to("cuda:0")
    nt = engine.run_neutral(Pd, msd, GID, 3, signal="cs_spread", n_bins=5, HLC=HLC)
    assert torch.equal(_raw(nt.M), _raw(rm.CSSPR))


TICKERS = ["AAPL", "MSFT", "AMZN", "GOOGL", "NVDA", "TSLA", "META", "JPM", "BAC", "WMT", "PG",
           "KO", "DIS", "CSCO", "ORCL", "INTC", "AMD", "NFLX", "C", "GS"]


@pytest.fixture(scope="module")
def real_frame(tmp_path_factory):
    import csmom.data as D
    tmp = tmp_path_factory.mktemp("daily_csv")
    with tarfile.open(GOLDEN / "daily_csv.tar.xz") as tar:
        for n in tar.getnames():
            (tmp / n).write_bytes(tar.extractfile(n).read())
    return D.fetch_daily(TICKERS, data_dir=str(tmp), verbose=False)


def test_range_signals_on_the_real_fixture(engine, real_frame):
    import csmom
    df = real_frame
    dense = csmom.from_long(df)
    H, L, C = csmom.range_from_long(df, dense)
    assert H.shape == dense.P.shape and dense.P.shape[1] == 19
    sums = RR.range_sums(H, L, C, dense.month_start)
    got = csmom.range_signals(df, window=3, min_obs=30, device=0)
    assert list(got.columns) == csmom.RANGE_COLUMNS
    PM = SR.month_stats(dense.P, dense.month_start)["PM"]
    aa, mm = np.nonzero(~O.is_absent(PM).T)
    assert len(got) == len(aa) and (got["ticker"].to_numpy() == dense.tickers[aa]).all()
    assert (got["date"].to_numpy() == dense.month_end[mm].to_numpy()).all()
    assert not got.duplicated(["ticker", "date"]).any()
    assert got.equals(got.sort_values(["ticker", "date"], kind="stable"))
    # the sums under the bars above, on the device's own upload of the same panels
    dsums = engine.range_sums(_up(H), _up(L), _up(C), _up(dense.month_start))
    _check_sums(dsums, sums, "(fixture)")
    own = RR.range_model(_np(dsums), 3, 30)
    for col, k in (("pkvol", "PKVOL"), ("cs_spread", "CSSPR"), ("ar_spread", "ARSPR")):
        assert bits_equal(got[col].to_numpy(), own[k][mm, aa]), col
    assert np.array_equal(got["nobs"].to_numpy(), own["NOBS"][mm, aa])
    # the counts are the reference's, so every cell is defined where the reference's is
    ref = RR.range_model(sums, 3, 30)
    for col, k in (("pkvol", "PKVOL"), ("cs_spread", "CSSPR"), ("ar_spread", "ARSPR")):
        assert np.array_equal(got[col].isna().to_numpy(), np.isnan(ref[k][mm, aa])), col
    assert got["pkvol"].notna().mean() >= 0.9 and 0.005 < got["pkvol"].mean() < 0.05
    assert 0.001 < got["cs_spread"].mean() < 0.02
    assert csmom.range_signals(df.iloc[:0], device=0) is None


def test_tables_and_portfolio_on_the_real_fixture(engine, real_frame):
    import csmom
    from csmom.features import upload_panel, upload_range
    df = real_frame
    fm = csmom.fama_macbeth(df, signals=("mom", "cs_spread"), device=0)
    assert list(fm.table.index) == ["const", "mom", "cs_spread"]
    assert np.isfinite(fm.table[["mean", "se", "t"]].to_numpy()).all()
    ic = csmom.information_coefficient(df, signals=("pkvol",), horizons=(1, 3), device=0)
    assert np.isfinite(ic.table[["mean", "se", "t"]].to_numpy()).all() and len(ic.table) == 2
    groups = {t: i % 2 for i, t in enumerate(sorted(set(df["ticker"])))}
    nm = csmom.neutral_momentum(df, groups, n_bins=3, signal="ar_spread", device=0)
    assert len(nm.long_short) >= 20 and np.isfinite(nm.mean)
    dense = csmom.from_long(df)
    P, _, ms = upload_panel(dense, engine, with_volume=False)
    HLC = upload_range(df, dense, engine)
    out = engine.run(P, ms, J=12, skip=1, n_bins=5)
    PKVOL = engine.range_model(engine.range_sums(*HLC, ms, with_cs=False, with_ar=False), 1).PKVOL
    pf = engine.portfolio(out.L, out.NR, 5, K=3, aum=1e8, SIG=PKVOL)
    assert np.isfinite(pf.LS.cpu().numpy()).sum() >= 40


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
    Hd, Ld, Cd, msd = pan["Hd"], pan["Ld"], pan["Cd"], pan["msd"]
    T_d, N = Hd.shape
    T_m = msd.numel() - 1
    ints = [torch.full((T_m, N), 77, dtype=torch.int32, device="cuda:0") for _ in range(3)]
    f = [torch.full((T_m, N), SENTINEL, dtype=torch.float64, device="cuda:0") for _ in range(3)]

    def sums(H=Hd, L=Ld, C=Cd, ms=msd, tm=T_m, mmd=23, gap=1, o=range(6), td=T_d):
        ptrs = [_ptr(t) if i in o else None for i, t in enumerate(ints + f)]
        return (_ptr(H), _ptr(L), _ptr(C), td, N, _ptr(ms), tm, mmd, gap, *ptrs)

    bad = [sums(gap=0), sums(gap=33), sums(mmd=0), sums(mmd=33), sums(tm=0), sums(td=0),
           sums(H=None), sums(L=None), sums(C=None), sums(ms=None)]
    bad += [sums(o=[j for j in range(6) if j != i]) for i in (0, 1, 3)]   # the required ones
    bad += [sums(o=(0, 1, 3, 4, 5)), sums(o=(0, 1, 2, 3, 5))]             # NCS and SCS go together
    for args in bad:
        _refused(engine, "csm_range_sums", args, ints + f)
    for kw in (dict(max_gap=0), dict(max_gap=33)):
        with pytest.raises(csmom.CsmError):
            engine.range_sums(Hd, Ld, Cd, msd, **kw)

    s = engine.range_sums(Hd, Ld, Cd, msd)
    ins = [_ptr(t) for t in s]
    g = [torch.full((T_m, N), SENTINEL, dtype=torch.float64, device="cuda:0") for _ in range(3)]
    nobs = torch.full((T_m, N), 77, dtype=torch.int32, device="cuda:0")
    c4 = 4.0 * np.log(2.0)

    def model(ins=ins, tm=T_m, Wm=1, mo=15, c4=c4, o=range(4)):
        ptrs = [_ptr(t) if i in o else None for i, t in enumerate(g + [nobs])]
        return (*ins, tm, N, Wm, mo, c4, *ptrs)

    def without(i):
        return ins[:i] + [None] + ins[i + 1:]

    bad = [model(Wm=0), model(Wm=13), model(mo=0), model(tm=0), model(o=()), model(c4=0.0),
           model(c4=-1.0), model(c4=float("inf")), model(c4=float("nan")),
           model(ins=without(2)), model(ins=without(4)),       # CSSPR without NCS, without SCS
           model(ins=without(5))]                              # ARSPR without SAR
    bad += [model(ins=without(i)) for i in (0, 1, 3)]
    for args in bad:
        _refused(engine, "csm_range_model", args, g + [nobs])
    # without the nullable inputs the other outputs are served
    engine._call("csm_range_model", *ins[:2], None, ins[3], None, None, T_m, N, 1, 15, c4,
                 _ptr(g[0]), None, None, _ptr(nobs))
    ref = RR.range_model(_np(s), 1, 15)
    assert bits_equal(g[0].cpu().numpy(), ref["PKVOL"])
    assert np.array_equal(nobs.cpu().numpy(), ref["NOBS"])
    for kw in (dict(window=0), dict(window=13), dict(min_obs=0)):
        with pytest.raises(csmom.CsmError) as e:
            engine.range_model(s, **kw)
        assert e.value.status == -1
    with pytest.raises(ValueError):
        engine.range_model(s, outputs=("PKVOL", "XX"))
