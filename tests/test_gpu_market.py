"""GPU: csm_market_factor / csm_market_model / csm_next_ret / Engine.run_signal on the market-model
signals (rules B1..B6 in DESIGN.md 7) against the NumPy restatement in tests/market_ref.py.

Bars.  X, NMK, BETA, ALPHA, NOBS and every next return are sequential fp64 sums and single
correctly rounded quotients in the order the rules state: bit for bit.  MKT is a sum whose order
the rule leaves to the kernel: |MKT - fsum / n| <= 2^-53 (sum |x| + |MKT|), which holds for every
order ((n - 1) u sum |x| for the sum, over n, plus the quotient's rounding), and two calls give
the same bits.  The market model is therefore given the device's own MKT on both sides.  IVOL and
RESMOM end in one square root and one quotient, both correctly rounded in this build: the bar
was 2 ulp (the D4 / D5 precedent), every case below measured 0 on an MI355X (the maximum found is
still printed), and so both are held to bit equality as well.  Labels and counts of the ranking
are exact, EW / LS within the project's 1e-10.

Coverage: in every parameter case but Wb = 60 (one whole window, the last month) at least 20 % of
the cells of each output are defined, so nothing passes on NaNs -- except RESMOM at N = 1, where
the one asset is the market (x = f bit for bit, every residual 0, sv = 0) and rule B5 itself
leaves every cell NaN; that case asserts exactly that.
"""
import ctypes

import numpy as np
import pytest
import torch

import market_ref as MR
import signals_ref as SR
from conftest import bits_equal, max_rel
from oracle import csmom_oracle as O
from oracle.synth_np import make_panel

pytestmark = pytest.mark.gpu
MAX_ULP = 0             # see the module docstring
FLOAT_OUT = ("BETA", "ALPHA", "IVOL", "RESMOM")
_CACHE = {}


def _up(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _raw(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else t.dtype)


def _same_bits(a, b):
    return torch.equal(_raw(a), _raw(b))


def _tune(key, value):
    import csmom
    assert csmom.load_library().csm_tune(key.encode(), ctypes.c_int(value)) == 0


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


def _host_pm(N, kind):
    if kind == "wide":       # 20,001 assets x 14 months: more than one slice of the row sum
        pan = make_panel(N, 320, seed=300 + N, cents=True, with_volume=False, **MR.GAPPY)
        return O.month_end(pan["P"], pan["month_start"])[0][:14].copy()
    if kind == "columns":    # a column without any price, and one without any row
        PM = MR.panel(N, "gappy")["PM"].copy()
        PM[:, 3] = np.nan
        PM[:, 4] = O.absent_like(PM.shape[0])
        return PM
    return MR.panel(N, kind)["PM"]


def _pan(engine, N, kind="gappy"):
    """Host PM, its device copy, the B1 / B2 reference and the device's own market (host and
    device); computed once per panel and left unchanged."""
    key = (N, kind)
    if key not in _CACHE:
        PM = _host_pm(N, kind)
        PMd = _up(PM)
        MKTd, _ = engine.market_factor(PMd)
        _CACHE[key] = dict(PM=PM, PMd=PMd, mf=MR.market_factor(PM), Fd=MKTd,
                           F=MKTd.cpu().numpy(), mm={})
    return _CACHE[key]


def _ref(pan, case):
    if case not in pan["mm"]:
        pan["mm"][case] = MR.market_model(pan["PM"], pan["F"], *case)
    return pan["mm"][case]


def _model(engine, pan, case, PMd=None, Fd=None, outputs=None):
    Wb, J, skip, mo = case
    return engine.market_model(pan["PMd"] if PMd is None else PMd, pan["Fd"] if Fd is None else Fd,
                               window=Wb, J=J, skip=skip, min_obs=mo, outputs=outputs)


def _check_model(out, ref, what):
    for k in ("BETA", "ALPHA"):
        assert bits_equal(getattr(out, k).cpu().numpy(), ref[k]), (k, what)
    assert np.array_equal(out.NOBS.cpu().numpy(), ref["NOBS"]), ("NOBS", what)
    assert out.NOBS.dtype == torch.int32
    for k in ("IVOL", "RESMOM"):
        assert _ulps(getattr(out, k).cpu().numpy(), ref[k], f"{k}{what}") <= MAX_ULP


def _equal_outputs(a, b, fields=FLOAT_OUT + ("NOBS",)):
    return all(_same_bits(getattr(a, k), getattr(b, k)) for k in fields)


# ------------------------------------------------------------------- csm_market_factor
def _check_factor(engine, pan, min_assets=1):
    ref = pan["mf"]
    MKT, NMK, X = engine.market_factor(pan["PMd"], min_assets=min_assets, with_x=True)
    assert bits_equal(X.cpu().numpy(), ref["X"])
    assert NMK.dtype == torch.int32 and np.array_equal(NMK.cpu().numpy(), ref["NMK"])
    got = MKT.cpu().numpy()
    want = np.where(ref["NMK"] >= min_assets, ref["MKT"], np.nan)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    bound = 2.0 ** -53 * (ref["SABS"][ok] + np.abs(got[ok]))
    print(f"MKT: worst error / bound {float(np.max(err / bound)) if ok.any() else 0.0:.3f} "
          f"over {int(ok.sum())} months")
    assert (err <= bound).all()
    # two calls, and a call without X or NMK: the same bits
    again, nmk2 = engine.market_factor(pan["PMd"], min_assets=min_assets)
    assert _same_bits(MKT, again) and torch.equal(NMK, nmk2)
    T_m, N = pan["PM"].shape
    from csmom.engine import _ptr
    alone = torch.empty(T_m, dtype=torch.float64, device="cuda:0")
    engine._call("csm_market_factor", _ptr(pan["PMd"]), T_m, N, min_assets, None, _ptr(alone),
                 None)
    assert _same_bits(MKT, alone)
    return got


@pytest.mark.parametrize("N", [1, 2, 63, 65, 257, 1030])
def test_market_factor(engine, N):
    pan = _pan(engine, N)
    got = _check_factor(engine, pan)
    assert np.isnan(got[0]) and pan["mf"]["NMK"][0] == 0
    if N >= 63:
        assert (~np.isnan(got)).sum() == 59 and (pan["mf"]["NMK"][1:] >= 0.5 * N).all()


def test_market_factor_wide_row(engine):
    pan = _pan(engine, 20001, "wide")
    assert pan["PM"].shape == (14, 20001)
    got = _check_factor(engine, pan)
    assert (~np.isnan(got)).sum() == 13 and (pan["mf"]["NMK"][1:] >= 10000).all()


def test_min_assets(engine):
    pan = _pan(engine, 130)
    nmk = pan["mf"]["NMK"]
    k = int(np.sort(nmk)[len(nmk) // 2]) + 1      # above about half of the months' counts
    got = _check_factor(engine, pan, min_assets=k)
    assert np.isnan(got[nmk < k]).all() and (nmk < k).sum() >= 20
    assert not np.isnan(got[nmk >= k]).any() and (nmk >= k).sum() >= 5


# -------------------------------------------------------------------- csm_market_model
@pytest.mark.parametrize("N", [1, 65, 130, 257])
@pytest.mark.parametrize("kind", ["gappy", "dense"])
@pytest.mark.parametrize("case", MR.CASES)
def test_market_model_vs_ref(engine, case, kind, N):
    pan = _pan(engine, N, kind)
    ref = _ref(pan, case)
    out = _model(engine, pan, case)
    _check_model(out, ref, f"{case} {kind} N={N}")
    assert _same_bits(out.F, pan["Fd"])
    if case[0] == 60:     # one whole window: bit equality only
        assert (ref["NOBS"][:59] == 0).all() and (ref["NOBS"][59] > 0).any()
        return
    for k in FLOAT_OUT:
        cover = float((~np.isnan(ref[k])).mean())
        if N == 1 and k == "RESMOM":   # the asset is the market: B5 defines nothing
            assert cover == 0.0 and (ref["BETA"][~np.isnan(ref["BETA"])] == 1.0).all()
        else:
            assert cover >= 0.2, (k, cover)


def test_columns_without_price_or_row(engine):
    pan = _pan(engine, 130, "columns")
    case = (24, 11, 1, 18)
    out = _model(engine, pan, case)
    _check_model(out, _ref(pan, case), " columns")
    for k in FLOAT_OUT:
        g = getattr(out, k).cpu().numpy()
        assert np.isnan(g[:, 3:5]).all() and not np.isnan(g[:, 5]).all()
    assert (out.NOBS.cpu().numpy()[:, 3:5] == 0).all()


def test_caller_factor_with_nan_months(engine):
    pan = _pan(engine, 130)
    case = (12, 6, 1, 10)
    rng = np.random.default_rng(7)
    F = rng.normal(0.01, 0.05, 60)
    F[[20, 41]] = np.nan
    ref = MR.market_model(pan["PM"], F, *case)
    out = _model(engine, pan, case, Fd=_up(F))
    _check_model(out, ref, " caller F")
    base = _ref(pan, case)["NOBS"]
    hit = np.zeros(60, dtype=bool)
    hit[20:32] = hit[41:53] = True
    assert (ref["NOBS"][hit] <= 11).all() and (ref["NOBS"][hit] < base[hit]).any()
    assert (~np.isnan(ref["BETA"])).mean() >= 0.2


def test_fewer_months_than_the_window(engine):
    pan = _pan(engine, 130)
    PMd = pan["PMd"][:10].contiguous()
    out = engine.market_model(PMd, pan["Fd"][:10].contiguous(), window=12, J=6, skip=1, min_obs=10)
    for k in FLOAT_OUT:
        assert torch.isnan(getattr(out, k)).all(), k
    assert (out.NOBS == 0).all()
    out = engine.market_model(PMd[:1].contiguous(), window=2, J=2, skip=0, min_obs=2)   # T_m = 1
    assert torch.isnan(out.BETA).all() and (out.NOBS == 0).all() and torch.isnan(out.F).all()


@pytest.mark.parametrize("N,case", [(130, (24, 11, 1, 18)), (257, (3, 2, 0, 3)),
                                    (65, (60, 12, 1, 40))])
def test_chunk_count_changes_no_bit(engine, N, case):
    pan = _pan(engine, N)
    ref = _ref(pan, case)
    base = _model(engine, pan, case)
    try:
        for chunks in (1, 3, 7, 60):
            _tune("mm_chunks", chunks)
            out = _model(engine, pan, case)
            assert _equal_outputs(base, out), chunks   # NaN payloads included
            _check_model(out, ref, f" chunks={chunks}")
    finally:
        _tune("mm_chunks", 0)


def test_unaligned_view_and_odd_width(engine):
    """An even-N panel through a view 8 B past a 16-B boundary, and an odd-N panel that is the
    first 129 columns of the 130-column one: the same bits per column."""
    pan = _pan(engine, 130)
    case = (24, 11, 1, 18)
    base = _model(engine, pan, case)
    T_m, N = pan["PM"].shape
    flat = torch.empty(T_m * N + 1, dtype=torch.float64, device="cuda:0")
    view = flat[1:].view(T_m, N)
    view.copy_(pan["PMd"])
    assert pan["PMd"].data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8
    assert _equal_outputs(base, _model(engine, pan, case, PMd=view))
    _, _, x0 = engine.market_factor(pan["PMd"], with_x=True)
    mkt1, _, x1 = engine.market_factor(view, with_x=True)
    assert _same_bits(x0, x1) and _same_bits(mkt1, pan["Fd"])
    odd = _model(engine, pan, case, PMd=pan["PMd"][:, :129].contiguous())
    for k in FLOAT_OUT + ("NOBS",):
        assert _same_bits(getattr(odd, k), getattr(base, k)[:, :129]), k
    nr0 = engine.next_ret(pan["PMd"], base.BETA)
    assert _same_bits(nr0, engine.next_ret(view, base.BETA))
    assert _same_bits(nr0[:, :129], engine.next_ret(pan["PMd"][:, :129].contiguous(), odd.BETA))


def test_a_subset_of_outputs_has_the_same_bits(engine):
    pan = _pan(engine, 257)
    case = (36, 12, 1, 24)
    base = _model(engine, pan, case)
    for sub in (("RESMOM",), ("BETA",), ("IVOL", "NOBS"), ("ALPHA", "RESMOM")):
        out = _model(engine, pan, case, outputs=sub)
        assert _equal_outputs(base, out, sub), sub
        for k in set(FLOAT_OUT + ("NOBS",)) - set(sub):
            assert getattr(out, k) is None
    # J and skip are read for RESMOM only
    Wb, J, skip, mo = case
    out = engine.market_model(pan["PMd"], pan["Fd"], window=Wb, J=99, skip=-3, min_obs=mo,
                              outputs=("BETA", "IVOL"))
    assert _equal_outputs(base, out, ("BETA", "IVOL"))
    with pytest.raises(ValueError):
        _model(engine, pan, case, outputs=("BETA", "XX"))


def test_market_model_default_factor_and_min_obs(engine):
    pan = _pan(engine, 130)
    a = engine.market_model(pan["PMd"])                       # window 36, min_obs 24, own MKT
    b = engine.market_model(pan["PMd"], pan["Fd"], window=36, J=12, skip=1, min_obs=24)
    assert _equal_outputs(a, b) and _same_bits(a.F, pan["Fd"])
    c = engine.market_model(pan["PMd"], pan["Fd"], window=10, outputs=("BETA",))   # ceil(20/3) = 7
    d = engine.market_model(pan["PMd"], pan["Fd"], window=10, min_obs=7, outputs=("BETA",))
    e = engine.market_model(pan["PMd"], pan["Fd"], window=10, min_obs=8, outputs=("BETA",))
    assert _same_bits(c.BETA, d.BETA) and not _same_bits(c.BETA, e.BETA)


# ------------------------------------------------------------------------ csm_next_ret
def test_next_ret_of_any_signal(engine):
    pan = _pan(engine, 257)
    PM = pan["PM"]
    out = _model(engine, pan, (24, 11, 1, 18))
    rng = np.random.default_rng(11)
    rnd = rng.normal(size=PM.shape)
    rnd[rng.random(PM.shape) < 0.3] = np.nan
    for name, Sd in (("BETA", out.BETA), ("RESMOM", out.RESMOM), ("random", _up(rnd))):
        ref = SR.next_ret(PM, Sd.cpu().numpy())
        assert (~np.isnan(ref)).mean() >= 0.2, name
        assert bits_equal(engine.next_ret(pan["PMd"], Sd).cpu().numpy(), ref), name
    nan = torch.full_like(out.BETA, float("nan"))     # nothing ranked: nothing settled
    assert torch.isnan(engine.next_ret(pan["PMd"], nan)).all()


def test_next_ret_of_h52_is_window_signals(engine):
    host = MR.panel(257)
    Pd, msd = _up(host["P"]), _up(host["ms"])
    st = engine.month_stats(Pd, msd)
    sig = engine.window_signals(*st, outputs=("H52", "NR_H52"))
    assert (~torch.isnan(sig.NR_H52)).float().mean() >= 0.2
    assert _same_bits(engine.next_ret(st.PM, sig.H52), sig.NR_H52)


# ------------------------------------------------------------------- Engine.run_signal
@pytest.mark.parametrize("signal,field", [("resid_mom", "RESMOM"), ("beta", "BETA"),
                                          ("ivol", "IVOL")])
def test_run_signal_on_the_market_model(engine, signal, field):
    host = MR.panel(257)
    pan = _pan(engine, 257)
    Pd, msd = _up(host["P"]), _up(host["ms"])
    out = engine.run_signal(Pd, msd, signal)
    assert bits_equal(out.PM.cpu().numpy(), host["PM"])
    # the step-by-step calls: window 36 (the default of 12 means 36 here), min_obs 24
    mm = engine.market_model(out.PM, window=36, J=12, skip=1, outputs=(field,))
    S = getattr(mm, field)
    assert _same_bits(out.M, S) and _same_bits(out.NR, engine.next_ret(out.PM, S))
    assert _same_bits(out.M, engine.run_signal(Pd, msd, signal, window=36, min_obs=24).M)
    assert not _same_bits(out.M, engine.run_signal(Pd, msd, signal, window=24).M)
    # against the restatement (on the device's own market) and the oracle's decile routine
    ref = _ref(pan, (36, 12, 1, 24))
    Sr = ref[field]
    assert _ulps(out.M.cpu().numpy(), Sr, f"run_signal {field}") <= MAX_ULP
    NRr = MR.next_ret(host["PM"], Sr)
    Lr = O.assign_deciles(Sr, 10)
    EWr, CNTr, LSr = O.portfolio_ew(Lr, NRr, 10)
    assert np.array_equal(out.L.cpu().numpy(), Lr)
    assert np.array_equal(out.CNT.cpu().numpy(), CNTr)
    for got, want in ((out.EW, EWr), (out.LS, LSr)):
        g = got.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(want))
        assert max_rel(g, want) <= 1e-10
    assert (~np.isnan(LSr)).sum() >= 15 and (Lr >= 0).mean() >= 0.2


def test_run_signal_keeps_the_daily_signals(engine):
    host = MR.panel(257)
    Pd, msd = _up(host["P"]), _up(host["ms"])
    st = engine.month_stats(Pd, msd)
    sig = engine.window_signals(*st, Jh=12, Jv=12, outputs=("H52", "NR_H52"))
    out = engine.run_signal(Pd, msd, "high52")
    assert _same_bits(out.M, sig.H52) and _same_bits(out.NR, sig.NR_H52)
    _, M, _ = engine.momentum(st.PM, 12, 1)
    sig = engine.window_signals(*st, M=M, Jh=12, Jv=12, outputs=("MS", "NR_MS"))
    out = engine.run_signal(Pd, msd, "mom_vol")
    assert _same_bits(out.M, sig.MS) and _same_bits(out.NR, sig.NR_MS)
    assert (~torch.isnan(out.LS)).sum() >= 20
    with pytest.raises(ValueError):
        engine.run_signal(Pd, msd, "alpha")


# --------------------------------------------------------------------- argument errors
SENTINEL = 12345.0


def test_bad_arguments_are_refused(engine):
    import csmom
    from csmom.engine import _ptr
    pan = _pan(engine, 130)
    PMd, Fd = pan["PMd"], pan["Fd"]
    T_m, N = PMd.shape
    f = [torch.full((T_m, N), SENTINEL, dtype=torch.float64, device="cuda:0") for _ in range(4)]
    nobs = torch.full((T_m, N), 77, dtype=torch.int32, device="cuda:0")

    def refused(name, args):
        with pytest.raises(csmom.CsmError) as e:
            engine._call(name, *args)
        assert e.value.status == -1   # CSM_E_INVAL
        torch.cuda.synchronize()
        for t in f:                   # nothing was launched
            assert (t == SENTINEL).all()
        assert (nobs == 77).all()

    def model(Wb=12, J=6, skip=1, mo=10, o=(0, 1, 2, 3), n=True, PM=PMd, F=Fd, tm=T_m):
        ptrs = [_ptr(f[i]) if i in o else None for i in range(4)]
        return (_ptr(PM), _ptr(F), tm, N, Wb, J, skip, mo, *ptrs, _ptr(nobs) if n else None)

    for args in (model(Wb=1, mo=2), model(Wb=61, mo=40), model(J=12), model(J=6, skip=7),
                 model(J=1), model(skip=-1), model(mo=1), model(mo=13), model(o=(), n=False),
                 model(PM=None), model(F=None), model(tm=0)):
        refused("csm_market_model", args)
    # J + skip > Wb is fine when RESMOM is not asked for
    engine._call("csm_market_model", *model(J=12, o=(0,), n=False))
    assert not (f[0] == SENTINEL).any()
    f[0].fill_(SENTINEL)
    for kw in (dict(window=1), dict(window=61), dict(window=12, J=12, skip=1),
               dict(window=12, J=6, min_obs=1)):
        with pytest.raises(csmom.CsmError) as e:
            engine.market_model(PMd, Fd, **kw)
        assert e.value.status == -1
    mkt = f[0][0]
    for args in ((None, T_m, N, 1, None, _ptr(mkt), None), (_ptr(PMd), T_m, N, 0, None, _ptr(mkt), None),
                 (_ptr(PMd), T_m, N, 1, None, None, None), (_ptr(PMd), 0, N, 1, None, _ptr(mkt), None)):
        refused("csm_market_factor", args)
    for args in ((None, _ptr(f[1]), T_m, N, _ptr(f[0])), (_ptr(PMd), None, T_m, N, _ptr(f[0])),
                 (_ptr(PMd), _ptr(f[1]), T_m, N, None), (_ptr(PMd), _ptr(f[1]), T_m, 0, _ptr(f[0]))):
        refused("csm_next_ret", args)
    assert csmom.load_library().csm_tune(b"mm_chunks", ctypes.c_int(-1)) == -1
