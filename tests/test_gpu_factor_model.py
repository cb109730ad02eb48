"""GPU: csm_factor_model / Engine.factor_model / Engine.run_signal(..., factors=) on monthly factors
(rules MF1..MF5, MF8 in DESIGN.md 7) against the NumPy restatement in tests/factor_ref.py.

Factors.  Column 0 is the device's own MKT, given to both sides; columns 1..3 are seeded normal
series (sigma 0.03); one value of one row is NaN (month 20 of 60: inside the formation months
of the Wb = 24 and Wb = 12 cases, inside the window only at Wb = 36 and 60).

Bars.  NOBS, BETA, ALPHA and R2 are sequences of correctly rounded + - * / in a stated order: bit
for bit.  IVOL and RESMOM end in one square root and one quotient, both correctly rounded in this
build: the bar was the project's 2 ulp (the D4 / D5 / B4 precedent), every case below measured 0
on an MI355X (the largest distance found is still printed), and so both are held to bit equality
as well: MAX_ULP = 0.  Labels and counts of the ranking are exact, EW / LS within the project's
1e-10.

Coverage, asserted on the reference: in every case but Wb = 60 (one whole window, the last month)
at least 20 % of each output's cells are defined, so nothing passes on NaNs.  The exceptions are
by rule: IVOL at Wb = KF + 1 (n - (KF + 1) = 0 degrees of freedom; every cell NaN, asserted), and
RESMOM at N = 1, where the one asset is factor column 0 itself, every residual is 0 or rounding
noise and sv > 0 decides cell by cell (the cells are still compared).
"""
import ctypes

import numpy as np
import pytest
import torch

import factor_ref as FR
import market_ref as MR
from conftest import bits_equal, load_golden, max_rel
from oracle import csmom_oracle as O
from oracle.synth_np import make_panel

pytestmark = pytest.mark.gpu
MAX_ULP = 0             # see the module docstring
FLOAT_OUT = ("BETA", "ALPHA", "IVOL", "RESMOM", "R2")
ALL_OUT = FLOAT_OUT + ("NOBS",)
CASES = [(24, 11, 1, 18), (12, 6, 1, 10), (8, 2, 0, 8), (36, 12, 1, 24), (60, 12, 1, 40)]
KFS = (1, 2, 3, 4)
SENTINEL = 12345.0
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
    if kind == "wide":       # 20,001 assets x 14 months: grid.x > 1 at an odd N
        pan = make_panel(N, 320, seed=300 + N, cents=True, with_volume=False, **MR.GAPPY)
        return O.month_end(pan["P"], pan["month_start"])[0][:14].copy()
    if kind == "columns":    # a column without any price, and one without any row
        PM = MR.panel(N, "gappy")["PM"].copy()
        PM[:, 3] = np.nan
        PM[:, 4] = O.absent_like(PM.shape[0])
        return PM
    return MR.panel(N, kind)["PM"]


def _pan(engine, N, kind="gappy"):
    """Host PM, its device copy and the device's own market; made once, left unchanged."""
    key = (N, kind)
    if key not in _CACHE:
        PM = _host_pm(N, kind)
        PMd = _up(PM)
        MKTd, _ = engine.market_factor(PMd)
        _CACHE[key] = dict(PM=PM, PMd=PMd, MKTd=MKTd, MKT=MKTd.cpu().numpy(), fac={}, ref={})
    return _CACHE[key]


def _fac(pan, KF):
    """(host, device) factors [T_m][KF]: the device's MKT, seeded columns, one NaN."""
    if KF not in pan["fac"]:
        T_m = len(pan["MKT"])
        F = FR.seeded_factors(pan["MKT"], 31, KF, 0.03, (T_m // 3, min(1, KF - 1)))
        assert np.isnan(F[T_m // 3]).sum() == 1
        pan["fac"][KF] = (F, _up(F))
    return pan["fac"][KF]


def _ref(pan, KF, case):
    if (KF, case) not in pan["ref"]:
        pan["ref"][(KF, case)] = FR.factor_model(pan["PM"], _fac(pan, KF)[0], *case)
    return pan["ref"][(KF, case)]


def _model(engine, pan, KF, case, PMd=None, Fd=None, outputs=None):
    Wb, J, skip, mo = case
    return engine.factor_model(pan["PMd"] if PMd is None else PMd,
                               _fac(pan, KF)[1] if Fd is None else Fd,
                               window=Wb, J=J, skip=skip, min_obs=mo, outputs=outputs)


def _check(out, ref, what):
    assert out.NOBS.dtype == torch.int32
    assert np.array_equal(out.NOBS.cpu().numpy(), ref["NOBS"]), ("NOBS", what)
    for k in ("BETA", "ALPHA", "R2"):
        got = getattr(out, k).cpu().numpy()
        assert got.shape == ref[k].shape and bits_equal(got, ref[k]), (k, what)
    for k in ("IVOL", "RESMOM"):
        assert _ulps(getattr(out, k).cpu().numpy(), ref[k], f"{k} {what}") <= MAX_ULP


def coverage(ref, KF, case, N):
    """The module docstring's condition on the inputs, on the reference's result."""
    if case[0] == 60:     # one whole window: bit equality only
        assert (ref["NOBS"][:59] == 0).all() and (ref["NOBS"][59] > 0).any()
        return
    for k in FLOAT_OUT:
        cover = float((~np.isnan(ref[k])).mean())
        if k == "IVOL" and case[0] == KF + 1:
            assert cover == 0.0
        elif not (k == "RESMOM" and N == 1):
            assert cover >= 0.2, (k, cover)


def _equal_outputs(a, b, fields=ALL_OUT):
    return all(_same_bits(getattr(a, k), getattr(b, k)) for k in fields)


# ------------------------------------------------------------------------ against the ref
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("KF", KFS)
def test_factor_model_vs_ref(engine, KF, case, N):
    pan = _pan(engine, N)
    ref = _ref(pan, KF, case)
    out = _model(engine, pan, KF, case)
    _check(out, ref, f"KF={KF} {case} N={N}")
    assert _same_bits(out.F, _fac(pan, KF)[1])
    coverage(ref, KF, case, N)


@pytest.mark.parametrize("kind", ["dense", "columns"])
@pytest.mark.parametrize("case", [(24, 11, 1, 18), (36, 12, 1, 24)])
@pytest.mark.parametrize("KF", KFS)
def test_dense_panel_and_empty_columns(engine, KF, case, kind):
    pan = _pan(engine, 130, kind)
    ref = _ref(pan, KF, case)
    out = _model(engine, pan, KF, case)
    _check(out, ref, f"KF={KF} {case} {kind}")
    coverage(ref, KF, case, 130)
    if kind == "columns":
        for k in FLOAT_OUT:
            g = getattr(out, k).cpu().numpy()
            assert np.isnan(g[..., 3:5]).all() and not np.isnan(g[..., 5]).all()
        assert (out.NOBS.cpu().numpy()[:, 3:5] == 0).all()


@pytest.mark.parametrize("KF", KFS)
def test_smallest_window(engine, KF):
    """Wb = min_obs = KF + 1: IVOL is NaN by rule, the coefficients interpolate."""
    pan = _pan(engine, 130)
    case = (KF + 1, 2, 0, KF + 1)
    ref = _ref(pan, KF, case)
    out = _model(engine, pan, KF, case)
    _check(out, ref, f"KF={KF} {case}")
    coverage(ref, KF, case, 130)
    assert torch.isnan(out.IVOL).all()


@pytest.mark.parametrize("KF", KFS)
def test_wide_row(engine, KF):
    case = (12, 6, 1, 10)
    pan = _pan(engine, 20001, "wide")
    assert pan["PM"].shape == (14, 20001)
    ref = _ref(pan, KF, case)
    _check(_model(engine, pan, KF, case), ref, f"KF={KF} wide")
    for k in FLOAT_OUT:       # of the three months with a whole window
        assert (~np.isnan(ref[k][..., case[0] - 1:, :])).mean() >= 0.2, k


# -------------------------------------------------------------------------------- MF8
@pytest.mark.parametrize("N,kind,cases", [(130, "gappy", CASES + [(2, 2, 0, 2)]),
                                          (20001, "wide", [(12, 6, 1, 10), (3, 2, 0, 3)])])
def test_one_factor_is_market_model(engine, N, kind, cases):
    pan = _pan(engine, N, kind)
    Fd = _fac(pan, 1)[1]
    for Wb, J, skip, mo in cases:
        want = engine.market_model(pan["PMd"], Fd[:, 0].contiguous(), window=Wb, J=J, skip=skip,
                                   min_obs=mo)
        for F in (Fd, Fd[:, 0].contiguous()):        # [T_m][1], and a 1-D series
            got = engine.factor_model(pan["PMd"], F, window=Wb, J=J, skip=skip, min_obs=mo)
            assert got.BETA.shape == (1, *want.BETA.shape)
            assert _same_bits(got.BETA[0], want.BETA), (Wb, "BETA")
            for k in ("ALPHA", "IVOL", "RESMOM", "NOBS"):
                assert _same_bits(getattr(got, k), getattr(want, k)), (Wb, k)
        if Wb < pan["PM"].shape[0]:     # of the months with a whole window
            assert (~torch.isnan(want.BETA[Wb - 1:])).float().mean() >= 0.2


# ------------------------------------------------------------------------ launch shape
@pytest.mark.parametrize("N,KF,case", [(130, 3, (24, 11, 1, 18)), (65, 4, (5, 2, 0, 5)),
                                       (65, 2, (60, 12, 1, 40))])
def test_chunk_count_changes_no_bit(engine, N, KF, case):
    pan = _pan(engine, N)
    base = _model(engine, pan, KF, case)
    assert _equal_outputs(base, _model(engine, pan, KF, case))      # two calls
    try:
        for chunks in (1, 7, 60):
            _tune("fm_chunks", chunks)
            out = _model(engine, pan, KF, case)
            assert _equal_outputs(base, out), chunks   # NaN payloads included
    finally:
        _tune("fm_chunks", 0)
    _check(base, _ref(pan, KF, case), f"KF={KF} {case} chunks")


def test_unaligned_view_and_odd_width(engine):
    pan = _pan(engine, 130)
    KF, case = 3, (24, 11, 1, 18)
    base = _model(engine, pan, KF, case)
    T_m, N = pan["PM"].shape
    flat = torch.empty(T_m * N + 1, dtype=torch.float64, device="cuda:0")
    view = flat[1:].view(T_m, N)
    view.copy_(pan["PMd"])
    assert pan["PMd"].data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8
    assert _equal_outputs(base, _model(engine, pan, KF, case, PMd=view))
    odd = _model(engine, pan, KF, case, PMd=pan["PMd"][:, :129].contiguous())
    for k in ALL_OUT:
        assert _same_bits(getattr(odd, k), getattr(base, k)[..., :129]), k


# ----------------------------------------------------------------------------- outputs
def test_a_subset_of_outputs_has_the_same_bits(engine):
    pan = _pan(engine, 130)
    KF, case = 3, (36, 12, 1, 24)
    base = _model(engine, pan, KF, case)
    for sub in (("RESMOM",), ("BETA",), ("IVOL", "NOBS"), ("R2",), ("ALPHA", "RESMOM"),
                ("NOBS",)):
        out = _model(engine, pan, KF, case, outputs=sub)
        assert _equal_outputs(base, out, sub), sub
        for k in set(ALL_OUT) - set(sub):
            assert getattr(out, k) is None
    # J and skip are read for RESMOM only
    Wb, J, skip, mo = case
    out = engine.factor_model(pan["PMd"], _fac(pan, KF)[1], window=Wb, J=99, skip=-3, min_obs=mo,
                              outputs=("BETA", "IVOL"))
    assert _equal_outputs(base, out, ("BETA", "IVOL"))
    with pytest.raises(ValueError):
        _model(engine, pan, KF, case, outputs=("BETA", "XX"))
    # the default min_obs: max(KF + 1, ceil(2 * window / 3))
    a = engine.factor_model(pan["PMd"], _fac(pan, KF)[1], window=10, outputs=("BETA",))
    b = engine.factor_model(pan["PMd"], _fac(pan, KF)[1], window=10, min_obs=7, outputs=("BETA",))
    c = engine.factor_model(pan["PMd"], _fac(pan, KF)[1], window=10, min_obs=8, outputs=("BETA",))
    assert _same_bits(a.BETA, b.BETA) and not _same_bits(a.BETA, c.BETA)
    d = engine.factor_model(pan["PMd"], _fac(pan, KF)[1], window=4, outputs=("BETA",))
    e = engine.factor_model(pan["PMd"], _fac(pan, KF)[1], window=4, min_obs=4, outputs=("BETA",))
    assert _same_bits(d.BETA, e.BETA)


def _buffers(KF, T_m, N):
    f = {k: torch.full((KF, T_m, N) if k == "BETA" else (T_m, N), SENTINEL, dtype=torch.float64,
                       device="cuda:0") for k in FLOAT_OUT}
    f["NOBS"] = torch.full((T_m, N), 77, dtype=torch.int32, device="cuda:0")
    return f


def _untouched(f, keys):
    torch.cuda.synchronize()
    return all(bool((f[k] == (77 if k == "NOBS" else SENTINEL)).all()) for k in keys)


def test_buffers_not_requested_are_untouched(engine):
    from csmom.engine import _ptr
    pan = _pan(engine, 130)
    KF, case = 2, (12, 6, 1, 10)
    base = _model(engine, pan, KF, case)
    T_m, N = pan["PM"].shape
    for sub in (("ALPHA",), ("BETA", "R2"), ("RESMOM", "NOBS"), ("IVOL",)):
        f = _buffers(KF, T_m, N)
        engine._call("csm_factor_model", _ptr(pan["PMd"]), _ptr(_fac(pan, KF)[1]), T_m, N, KF,
                     *case, *(_ptr(f[k]) if k in sub else None for k in ALL_OUT))
        assert _untouched(f, set(ALL_OUT) - set(sub)), sub
        for k in sub:
            assert _same_bits(f[k], getattr(base, k)), (sub, k)


# --------------------------------------------------------- factors that define nothing
def test_collinear_pair_and_all_nan_column(engine):
    pan = _pan(engine, 130)
    case = (24, 11, 1, 18)
    mkt = pan["MKT"]
    F = np.stack([mkt, 2.0 * mkt], axis=1)
    ref = FR.factor_model(pan["PM"], F, *case)
    out = _model(engine, pan, 2, case, Fd=_up(F))
    for k in FLOAT_OUT:
        assert np.isnan(ref[k]).all() and torch.isnan(getattr(out, k)).all(), k
    assert np.array_equal(out.NOBS.cpu().numpy(), ref["NOBS"]) and (ref["NOBS"] >= 18).mean() >= 0.2
    F = FR.seeded_factors(mkt, 31, 3, 0.03)
    F[:, 2] = np.nan
    out = _model(engine, pan, 3, case, Fd=_up(F))
    for k in FLOAT_OUT:
        assert torch.isnan(getattr(out, k)).all(), k
    assert (out.NOBS == 0).all() and (FR.factor_model(pan["PM"], F, *case)["NOBS"] == 0).all()


def test_fewer_months_than_the_window(engine):
    pan = _pan(engine, 130)
    out = engine.factor_model(pan["PMd"][:10].contiguous(), _fac(pan, 3)[1][:10].contiguous(),
                              window=12, J=6, skip=1, min_obs=10)
    for k in FLOAT_OUT:
        assert torch.isnan(getattr(out, k)).all(), k
    assert (out.NOBS == 0).all()


# --------------------------------------------------------------------- argument errors
def test_bad_arguments_are_refused(engine):
    import csmom
    from csmom.engine import _ptr
    pan = _pan(engine, 130)
    PMd = pan["PMd"]
    T_m, N = PMd.shape
    Fd = _fac(pan, 4)[1]        # [T_m][4] serves every KF <= 4 here: only refusals are tried
    f = _buffers(4, T_m, N)

    def model(KF=2, Wb=12, J=6, skip=1, mo=10, o=ALL_OUT, PM=PMd, F=Fd, tm=T_m):
        return (_ptr(PM), _ptr(F), tm, N, KF, Wb, J, skip, mo,
                *(_ptr(f[k]) if k in o else None for k in ALL_OUT))

    for args in (model(KF=0), model(KF=5), model(KF=-1), model(KF=3, Wb=3, mo=3),
                 model(Wb=61, mo=40), model(mo=2), model(mo=13), model(J=12), model(J=6, skip=7),
                 model(J=1), model(skip=-1), model(o=()), model(PM=None), model(F=None),
                 model(tm=0)):
        with pytest.raises(csmom.CsmError) as e:
            engine._call("csm_factor_model", *args)
        assert e.value.status == -1   # CSM_E_INVAL
        assert _untouched(f, ALL_OUT)  # nothing was launched
    # J + skip > Wb is fine when RESMOM is not asked for
    engine._call("csm_factor_model", *model(J=12, o=("ALPHA",)))
    assert not _untouched(f, ("ALPHA",)) and _untouched(f, set(ALL_OUT) - {"ALPHA"})
    F3 = _fac(pan, 3)[1]
    for kw in (dict(window=3), dict(window=61), dict(window=12, J=12, skip=1),
               dict(window=12, J=6, min_obs=3), dict(window=12, J=6, min_obs=13)):
        with pytest.raises(csmom.CsmError) as e:
            engine.factor_model(PMd, F3, **kw)
        assert e.value.status == -1
    for bad in (torch.zeros((T_m, 5), dtype=torch.float64, device="cuda:0"),
                torch.zeros((T_m - 1, 2), dtype=torch.float64, device="cuda:0"),
                torch.zeros((T_m, 2, 1), dtype=torch.float64, device="cuda:0")):
        with pytest.raises(ValueError):
            engine.factor_model(PMd, bad)
    lib = csmom.load_library()
    assert lib.csm_tune(b"fm_chunks", ctypes.c_int(-1)) == -1


# ------------------------------------------------------------------- Engine.run_signal
def _ranking_matches_oracle(out, PM, Sr):
    NRr = MR.next_ret(PM, Sr)
    assert bits_equal(out.NR.cpu().numpy(), NRr)
    Lr = O.assign_deciles(Sr, 10)
    EWr, CNTr, LSr = O.portfolio_ew(Lr, NRr, 10)
    assert np.array_equal(out.L.cpu().numpy(), Lr)
    assert np.array_equal(out.CNT.cpu().numpy(), CNTr)
    for got, want in ((out.EW, EWr), (out.LS, LSr)):
        g = got.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(want))
        assert max_rel(g, want) <= 1e-10
    return Lr, LSr


@pytest.mark.parametrize("signal,field", [("resid_mom", "RESMOM"), ("beta", "BETA"),
                                          ("ivol", "IVOL")])
def test_run_signal_with_factors(engine, signal, field):
    host = MR.panel(257)
    pan = _pan(engine, 257)
    Pd, msd = _up(host["P"]), _up(host["ms"])
    F3, F3d = _fac(pan, 3)
    out = engine.run_signal(Pd, msd, signal, factors=F3d)
    assert bits_equal(out.PM.cpu().numpy(), host["PM"])
    # the step-by-step call: window 36 (the default of 12 means 36 here), min_obs 24
    fm = engine.factor_model(out.PM, F3d, window=36, J=12, skip=1, outputs=(field,))
    S = getattr(fm, field)
    S = S[0] if field == "BETA" else S           # "beta": column 0's slope
    assert _same_bits(out.M, S) and _same_bits(out.NR, engine.next_ret(out.PM, S))
    assert _same_bits(out.M, engine.run_signal(Pd, msd, signal, window=36, min_obs=24,
                                               factors=F3d).M)
    assert not _same_bits(out.M, engine.run_signal(Pd, msd, signal, window=24, factors=F3d).M)
    ref = _ref(pan, 3, (36, 12, 1, 24))[field]
    ref = ref[0] if field == "BETA" else ref
    assert _ulps(out.M.cpu().numpy(), ref, f"run_signal {field}") <= (0 if field == "BETA"
                                                                      else MAX_ULP)
    Lr, LSr = _ranking_matches_oracle(out, host["PM"], out.M.cpu().numpy())
    assert (~np.isnan(LSr)).sum() >= 15 and (Lr >= 0).mean() >= 0.2


def test_run_signal_without_factors_is_unchanged(engine):
    host = MR.panel(257)
    Pd, msd = _up(host["P"]), _up(host["ms"])
    out = engine.run_signal(Pd, msd, "resid_mom")
    mm = engine.market_model(out.PM, window=36, J=12, skip=1, outputs=("RESMOM",))
    assert _same_bits(out.M, mm.RESMOM) and _same_bits(out.NR, engine.next_ret(out.PM, mm.RESMOM))
    assert _same_bits(out.M, engine.run_signal(Pd, msd, "resid_mom", factors=None).M)
    F3d = _fac(_pan(engine, 257), 3)[1]
    for signal in ("max", "high52", "mom_vol", "dskew"):
        with pytest.raises(ValueError):
            engine.run_signal(Pd, msd, signal, factors=F3d)
    with pytest.raises(ValueError):
        engine.run_signal(Pd, msd, "alpha", factors=F3d)


def test_residual_momentum_from_a_daily_frame(engine):
    """csmom.residual_momentum: frame -> panel -> align_factors -> run_signal -> newey_west."""
    import pandas as pd

    import csmom
    from csmom.features import upload_panel
    z = load_golden("real_data")
    dd, aa = np.nonzero(~O.is_absent(z["P"]))
    df = pd.DataFrame({"date": pd.to_datetime(z["day_ns"])[dd], "ticker": z["tickers"][aa],
                       "adj_close": z["P"][dd, aa]})
    panel = csmom.from_long(df)
    idx = pd.DatetimeIndex(panel.month_end)
    assert panel.T_m == 84
    rng = np.random.default_rng(9)
    fac = pd.DataFrame(rng.normal(0.0, 0.03, (84, 3)), columns=["MKT", "SMB", "HML"],
                       index=idx - pd.Timedelta(days=2)).drop(idx[40] - pd.Timedelta(days=2))
    fac = fac.sample(frac=1.0, random_state=3)                  # unordered, one month missing
    res = csmom.residual_momentum(df, fac, window=24, J=6, skip=1, n_bins=5, device=0)
    assert list(res.factors.columns) == ["MKT", "SMB", "HML"] and res.factors.index.equals(idx)
    assert res.factors.iloc[40].isna().all() and res.factors.drop(idx[40]).notna().all().all()
    P, _, ms = upload_panel(panel, engine, with_volume=False)
    out = engine.run_signal(P, ms, "resid_mom", J=6, skip=1, n_bins=5, window=24,
                            factors=_up(res.factors.to_numpy()))
    ls = out.LS.cpu().numpy()
    assert bits_equal(res.long_short.to_numpy(), ls[~np.isnan(ls)]) and len(res.long_short) >= 40
    assert res.deciles.shape == (84, 5) and bits_equal(res.deciles.to_numpy(), out.EW.cpu().numpy())
    nw = engine.newey_west(out.LS)
    assert res.mean == float(nw.MEAN) and res.t_nw == float(nw.T) and np.isfinite(res.t_nw)
    ref = FR.factor_model(out.PM.cpu().numpy(), res.factors.to_numpy(), 24, 6, 1, 16)["RESMOM"]
    assert _ulps(out.M.cpu().numpy(), ref, "frame RESMOM") <= MAX_ULP
    assert (~np.isnan(ref[23:])).mean() >= 0.2


def test_lagged(engine):
    x = np.random.default_rng(5).normal(size=40)
    for lags in (0, 1, 2, 5):
        want = np.full((40, 1 + lags), np.nan)
        for k in range(1 + lags):
            want[k:, k] = x[:40 - k]
        got = engine.lagged(_up(x), lags)
        assert got.is_contiguous() and got.device.type == "cuda"
        assert bits_equal(got.cpu().numpy(), want), lags
    with pytest.raises(ValueError):
        engine.lagged(_up(x).view(8, 5), 1)
