"""GPU: csm_daily_fsums / csm_daily_fmodel, Engine.lagged and Engine.run_signal(..., factors=) on
daily factors (rules MF6..MF8 in DESIGN.md 7) against the NumPy restatement in tests/factor_ref.py.

Factors.  Column 0 is the device's own MKTD, given to both sides; columns 1..3 are seeded normal
series (sigma 0.01); one value of one row is NaN.

Bars.  NO, every MF6 sum, NOBS, DBETA, DALPHA and DR2 are sequences of correctly rounded + - * /
in a stated order: bit for bit.  DIVOL ends in one square root, correctly rounded in this build:
the bar was the project's 2 ulp (the D4 / D5 / B4 precedent), every case below measured 0 on an
MI355X (the largest distance found is still printed), and so it is held to bit equality as well:
MAX_ULP = 0.  Labels and counts of the ranking are exact, EW / LS within the project's 1e-10.

Coverage, asserted on the reference: in every case at least 20 % of each output's cells are
defined (Wm = 12 leaves 4 of the 15 months a whole window), so nothing passes on NaNs.
"""
import ctypes

import numpy as np
import pytest
import torch

import dailymkt_ref as DR
import factor_ref as FR
import signals_ref as SR
from conftest import bits_equal, max_rel
from oracle import csmom_oracle as O
from oracle.synth_np import make_panel

pytestmark = pytest.mark.gpu
T_DAYS = 320            # 15 whole business-day months from 2000-01-03
T_M = 15
GAPPY = dict(late=0.2, delist=0.2, nan_day=0.01, absent_month=0.01, nan_month=0.01)
DENSE = dict(late=0, delist=0, nan_day=0, absent_month=0, nan_month=0)
MAX_ULP = 0             # see the module docstring
MAX_GAP = 10
GAP_COL = 5             # the hand-built column of the "gaps" panel
KFS = (1, 2, 3, 4)
FLOAT_OUT = ("DBETA", "DALPHA", "DIVOL", "DR2")
SENTINEL = 12345.0
_CACHE = {}


def models(KF):
    """(Wm, min_obs) of the tests."""
    return [(1, 15), (3, 45), (12, 180), (1, KF + 1)]


def _up(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _raw(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else t.dtype)


def _same(xs, ys):
    return all(torch.equal(_raw(a), _raw(b)) for a, b in zip(xs, ys))


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


def host_panel(N, kind):
    pan = make_panel(N, T_DAYS, seed=300 + N, cents=True, with_volume=False,
                     **(DENSE if kind == "dense" else GAPPY))
    P, ms = pan["P"], pan["month_start"]
    assert len(ms) - 1 == T_M
    if kind == "zero":       # month 4 has no day
        ms = np.concatenate([ms[:5], ms[4:]])
    if kind == "gaps":       # dailymkt_ref.gap_column: gaps around max_gap, across chunk starts
        P[:, GAP_COL], _ = DR.gap_column(T_DAYS, MAX_GAP, int(ms[8]), O.absent_scalar())
    return P, ms


def _panel(engine, N, kind="gappy"):
    """Host panel, its V1 returns, the device copy and the device's own daily market; made once
    and left unchanged."""
    key = (N, kind)
    if key not in _CACHE:
        P, ms = host_panel(N, kind)
        Pd = _up(P)
        MKTDd, _ = engine.daily_market(Pd, MAX_GAP)
        _CACHE[key] = dict(P=P, ms=ms, Pd=Pd, msd=_up(ms), R=DR.daily_ret(P, MAX_GAP),
                           MKTDd=MKTDd, MKTD=MKTDd.cpu().numpy(), fac={}, sums={}, mod={})
    return _CACHE[key]


def host_factors(MKTD, KF):
    FD = FR.seeded_factors(MKTD, 77, KF, 0.01, (100, min(1, KF - 1)))
    assert np.isnan(FD[100]).sum() == 1
    return FD


def _fac(pan, KF):
    if KF not in pan["fac"]:
        FD = host_factors(pan["MKTD"], KF)
        pan["fac"][KF] = (FD, _up(FD))
    return pan["fac"][KF]


def _sums_ref(pan, KF):
    if KF not in pan["sums"]:
        pan["sums"][KF] = FR.daily_fsums(pan["R"], _fac(pan, KF)[0], pan["ms"])
    return pan["sums"][KF]


def _model_ref(pan, KF, Wm, mo):
    if (KF, Wm, mo) not in pan["mod"]:
        pan["mod"][(KF, Wm, mo)] = FR.daily_fmodel(_sums_ref(pan, KF), Wm, mo)
    return pan["mod"][(KF, Wm, mo)]


def _check_sums(sums, ref):
    assert sums.NO.dtype == torch.int32
    assert np.array_equal(sums.NO.cpu().numpy(), ref["NO"]), "NO"
    for k in FR.FSUMS[1:]:
        got = getattr(sums, k).cpu().numpy()
        assert got.shape == ref[k].shape and bits_equal(got, ref[k]), k


def _check_model(mod, ref, tag):
    assert mod.NOBS.dtype == torch.int32
    assert np.array_equal(mod.NOBS.cpu().numpy(), ref["NOBS"]), "NOBS"
    for k in ("DBETA", "DALPHA", "DR2"):
        got = getattr(mod, k).cpu().numpy()
        assert got.shape == ref[k].shape and bits_equal(got, ref[k]), (k, tag)
    assert _ulps(mod.DIVOL.cpu().numpy(), ref["DIVOL"], f"DIVOL {tag}") <= MAX_ULP


def coverage(ref):
    for k in FLOAT_OUT:
        cover = float((~np.isnan(ref[k])).mean())
        assert cover >= 0.2, (k, cover)


def _run(engine, pan, KF, Pd=None, cover=True):
    sums = engine.daily_fsums(pan["Pd"] if Pd is None else Pd, pan["msd"], _fac(pan, KF)[1],
                              MAX_GAP)
    _check_sums(sums, _sums_ref(pan, KF))
    for Wm, mo in models(KF):
        ref = _model_ref(pan, KF, Wm, mo)
        _check_model(engine.daily_fmodel(sums, Wm, mo), ref, f"KF={KF} Wm={Wm} min_obs={mo}")
        if cover:
            coverage(ref)
    return sums


# ------------------------------------------------------------------------ against the ref
@pytest.mark.parametrize("N", [1, 64, 129, 130, 2050])
@pytest.mark.parametrize("KF", KFS)
def test_vs_ref_gappy(engine, KF, N):
    _run(engine, _panel(engine, N), KF)


@pytest.mark.parametrize("kind", ["zero", "gaps", "dense"])
@pytest.mark.parametrize("KF", KFS)
def test_calendars_gaps_and_dense(engine, KF, kind):
    pan = _panel(engine, 130, kind)
    sums = _run(engine, pan, KF, cover=kind != "zero")   # 16 months, one of them empty
    if kind == "zero":
        assert len(pan["ms"]) - 1 == T_M + 1
        for t in sums:
            assert (t[..., 4, :] == 0).all()
        coverage(_model_ref(pan, KF, 1, 15))
    if kind == "gaps":
        _, cases = DR.gap_column(T_DAYS, MAX_GAP, int(pan["ms"][8]), O.absent_scalar())
        r = pan["R"][:, GAP_COL]
        assert [not np.isnan(r[d]) for d, _, _ in cases] == [b for _, _, b in cases]


@pytest.mark.parametrize("KF", KFS)
def test_unaligned_panel_takes_the_one_asset_path(engine, KF):
    """Even N through a view 8 B past a 16-B boundary: the same bits as the paired path."""
    pan = _panel(engine, 130)
    T_d, N = pan["P"].shape
    flat = torch.empty(T_d * N + 1, dtype=torch.float64, device="cuda:0")
    view = flat[1:].view(T_d, N)
    view.copy_(pan["Pd"])
    assert pan["Pd"].data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8
    a = engine.daily_fsums(view, pan["msd"], _fac(pan, KF)[1], MAX_GAP)
    _check_sums(a, _sums_ref(pan, KF))
    assert _same(a, engine.daily_fsums(pan["Pd"], pan["msd"], _fac(pan, KF)[1], MAX_GAP))


# -------------------------------------------------------------------------------- MF8
@pytest.mark.parametrize("N", [130, 2050])
def test_one_factor_is_the_daily_model(engine, N):
    pan = _panel(engine, N)
    FD1 = _fac(pan, 1)[1]
    s1 = engine.daily_sums(pan["Pd"], pan["msd"], FD1[:, 0].contiguous(), MAX_GAP)
    for FD in (FD1, FD1[:, 0].contiguous()):           # [T_d][1], and a 1-D series
        f = engine.daily_fsums(pan["Pd"], pan["msd"], FD, MAX_GAP)
        assert f.SF.shape == (1, T_M, N) and f.SFF.shape == (1, T_M, N)
        assert _same((f.NO, f.SR, f.SF[0], f.SRR, f.SFF[0], f.SRF[0]), s1[:6])
    for Wm, mo in [(1, 15), (3, 45), (12, 180), (1, 3)]:
        want = engine.daily_model(s1, Wm, mo, outputs=("DBETA", "DIVOL", "NOBS"))
        got = engine.daily_fmodel(f, Wm, mo)
        assert _same((got.DBETA[0], got.DIVOL, got.NOBS), (want.DBETA, want.DIVOL, want.NOBS)), Wm
        assert (~torch.isnan(want.DBETA)).float().mean() >= 0.2


# ------------------------------------------------------------------------ launch shape
@pytest.mark.parametrize("N,kind,KF", [(130, "gaps", 3), (2050, "gappy", 4), (129, "gappy", 2)])
def test_launch_shape_changes_no_bit(engine, N, kind, KF):
    pan = _panel(engine, N, kind)
    FDd = _fac(pan, KF)[1]
    base = _run(engine, pan, KF, cover=False)
    assert _same(base, engine.daily_fsums(pan["Pd"], pan["msd"], FDd, MAX_GAP))     # two calls
    try:
        for chunks in (1, 4, T_M):
            _tune("dfsums_chunks", chunks)
            assert _same(base, engine.daily_fsums(pan["Pd"], pan["msd"], FDd, MAX_GAP)), chunks
        for Wm in (1, 3, 12):
            _tune("dfmodel_chunks", 0)
            want = engine.daily_fmodel(base, Wm)
            assert _same(_fields(want), _fields(engine.daily_fmodel(base, Wm)))      # two calls
            for chunks in (1, 4, T_M):
                _tune("dfmodel_chunks", chunks)
                assert _same(_fields(want), _fields(engine.daily_fmodel(base, Wm))), (Wm, chunks)
    finally:
        for k in ("dfsums_chunks", "dfmodel_chunks"):
            _tune(k, 0)


def _fields(mod):
    return [getattr(mod, k) for k in FR.FMODEL]


# ----------------------------------------------------------------------------- outputs
def _buffers(KF, N):
    f = {k: torch.full((KF, T_M, N) if k == "DBETA" else (T_M, N), SENTINEL, dtype=torch.float64,
                       device="cuda:0") for k in FLOAT_OUT}
    f["NOBS"] = torch.full((T_M, N), 77, dtype=torch.int32, device="cuda:0")
    return f


def _untouched(f, keys):
    torch.cuda.synchronize()
    return all(bool((f[k] == (77 if k == "NOBS" else SENTINEL)).all()) for k in keys)


def test_a_subset_of_outputs_has_the_same_bits_and_touches_nothing_else(engine):
    from csmom.engine import _ptr
    pan = _panel(engine, 130)
    KF, N = 3, 130
    sums = engine.daily_fsums(pan["Pd"], pan["msd"], _fac(pan, KF)[1], MAX_GAP)
    base = engine.daily_fmodel(sums, 3, 45)
    for sub in (("DBETA",), ("DALPHA", "NOBS"), ("DIVOL",), ("DR2",), ("NOBS",)):
        out = engine.daily_fmodel(sums, 3, 45, outputs=sub)
        for k in FR.FMODEL:
            if k in sub:
                assert _same([getattr(out, k)], [getattr(base, k)]), (sub, k)
            else:
                assert getattr(out, k) is None
        f = _buffers(KF, N)
        engine._call("csm_daily_fmodel", *(_ptr(t) for t in sums), T_M, N, KF, 3, 45,
                     *(_ptr(f[k]) if k in sub else None for k in FR.FMODEL))
        assert _untouched(f, set(FR.FMODEL) - set(sub)), sub
        assert _same([f[k] for k in sub], [getattr(base, k) for k in sub]), sub
    with pytest.raises(ValueError):
        engine.daily_fmodel(sums, outputs=("DBETA", "XX"))
    # the default min_obs: max(15 * window, KF + 1)
    assert _same(_fields(engine.daily_fmodel(sums, 3)), _fields(base))


# --------------------------------------------------------- factors that define nothing
def test_collinear_pair_and_all_nan_column(engine):
    pan = _panel(engine, 130)
    FD = np.stack([pan["MKTD"], 2.0 * pan["MKTD"]], axis=1)
    sref = FR.daily_fsums(pan["R"], FD, pan["ms"])
    sums = engine.daily_fsums(pan["Pd"], pan["msd"], _up(FD), MAX_GAP)
    _check_sums(sums, sref)
    ref = FR.daily_fmodel(sref, 1, 15)
    mod = engine.daily_fmodel(sums, 1, 15)
    for k in FLOAT_OUT:
        assert np.isnan(ref[k]).all() and torch.isnan(getattr(mod, k)).all(), k
    assert np.array_equal(mod.NOBS.cpu().numpy(), ref["NOBS"]) and (ref["NOBS"] >= 15).mean() >= 0.5
    FD = FR.seeded_factors(pan["MKTD"], 77, 3, 0.01)
    FD[:, 1] = np.nan
    sums = engine.daily_fsums(pan["Pd"], pan["msd"], _up(FD), MAX_GAP)
    for t in sums:
        assert (t == 0).all()
    mod = engine.daily_fmodel(sums, 1, 15)
    for k in FLOAT_OUT:
        assert torch.isnan(getattr(mod, k)).all(), k
    assert (mod.NOBS == 0).all()


# --------------------------------------------------------------------- argument errors
def test_bad_arguments_are_refused(engine):
    import csmom
    from csmom.engine import _ptr
    pan = _panel(engine, 64)
    Pd, msd = pan["Pd"], pan["msd"]
    T_d, N = Pd.shape
    FDd = _fac(pan, 4)[1]       # [T_d][4] serves every KF <= 4 here: only refusals are tried
    s = dict(NO=torch.full((T_M, N), 77, dtype=torch.int32, device="cuda:0"))
    for k, lead in (("SR", ()), ("SRR", ()), ("SF", (4,)), ("SRF", (4,)), ("SFF", (10,))):
        s[k] = torch.full((*lead, T_M, N), SENTINEL, dtype=torch.float64, device="cuda:0")

    def clean():
        torch.cuda.synchronize()
        return all(bool((t == (77 if k == "NO" else SENTINEL)).all()) for k, t in s.items())

    def sums(KF=2, P=Pd, F=FDd, ms=msd, tm=T_M, mmd=23, gap=10, drop=None, td=T_d):
        return (_ptr(P), _ptr(F), td, N, KF, _ptr(ms), tm, mmd, gap,
                *(None if k == drop else _ptr(s[k]) for k in FR.FSUMS))

    bad = [sums(KF=0), sums(KF=5), sums(gap=0), sums(gap=33), sums(mmd=0), sums(mmd=33),
           sums(tm=0), sums(td=0), sums(P=None), sums(F=None), sums(ms=None)]
    bad += [sums(drop=k) for k in FR.FSUMS]
    for args in bad:
        with pytest.raises(csmom.CsmError) as e:
            engine._call("csm_daily_fsums", *args)
        assert e.value.status == -1 and clean()   # CSM_E_INVAL, nothing launched
    for kw in (dict(max_gap=0), dict(max_gap=33)):
        with pytest.raises(csmom.CsmError):
            engine.daily_fsums(Pd, msd, FDd, **kw)
    for badF in (torch.zeros((T_d, 5), dtype=torch.float64, device="cuda:0"),
                 torch.zeros((T_d - 1, 2), dtype=torch.float64, device="cuda:0")):
        with pytest.raises(ValueError):
            engine.daily_fsums(Pd, msd, badF)

    real = engine.daily_fsums(Pd, msd, _fac(pan, 2)[1], MAX_GAP)
    ins = [_ptr(t) for t in real]
    f = _buffers(2, N)

    def model(ins=ins, tm=T_M, KF=2, Wm=1, mo=15, o=FR.FMODEL):
        return (*ins, tm, N, KF, Wm, mo, *(_ptr(f[k]) if k in o else None for k in FR.FMODEL))

    bad = [model(KF=0), model(KF=5), model(Wm=0), model(Wm=13), model(mo=2), model(tm=0),
           model(o=())]
    bad += [model(ins=ins[:i] + [None] + ins[i + 1:]) for i in range(6)]
    for args in bad:
        with pytest.raises(csmom.CsmError) as e:
            engine._call("csm_daily_fmodel", *args)
        assert e.value.status == -1 and _untouched(f, FR.FMODEL)
    engine._call("csm_daily_fmodel", *model(mo=3, o=("DALPHA",)))     # min_obs = KF + 1 is served
    assert not _untouched(f, ("DALPHA",)) and _untouched(f, set(FR.FMODEL) - {"DALPHA"})
    for kw in (dict(window=0), dict(window=13), dict(min_obs=2)):
        with pytest.raises(csmom.CsmError) as e:
            engine.daily_fmodel(real, **kw)
        assert e.value.status == -1
    lib = csmom.load_library()
    for key in (b"dfsums_chunks", b"dfmodel_chunks"):
        assert lib.csm_tune(key, ctypes.c_int(-1)) == -1


# ------------------------------------------------------------------- Engine.run_signal
@pytest.mark.parametrize("signal,field,Wm", [("divol", "DIVOL", 1), ("dbeta", "DBETA", 12)])
def test_run_signal_with_daily_factors(engine, signal, field, Wm):
    pan = _panel(engine, 130)
    FD3, FD3d = _fac(pan, 3)
    if "PM" not in pan:
        pan["PM"] = SR.month_stats(pan["P"], pan["ms"])["PM"]
    out = engine.run_signal(pan["Pd"], pan["msd"], signal, factors=FD3d)
    assert bits_equal(out.PM.cpu().numpy(), pan["PM"])
    # the step-by-step calls: window 12 months for "dbeta", 1 for "divol"; min_obs 15 * window
    sums = engine.daily_fsums(pan["Pd"], pan["msd"], FD3d, MAX_GAP)
    S = getattr(engine.daily_fmodel(sums, Wm, outputs=(field,)), field)
    S = S[0] if field == "DBETA" else S            # "dbeta": column 0's slope
    assert _same([out.M, out.NR], [S, engine.next_ret(out.PM, S)])
    ref = _model_ref(pan, 3, Wm, 15 * Wm)[field]
    ref = ref[0] if field == "DBETA" else ref
    assert _ulps(out.M.cpu().numpy(), ref, signal) <= (0 if field == "DBETA" else MAX_ULP)
    Sr = out.M.cpu().numpy()
    NRr = SR.next_ret(pan["PM"], Sr)
    assert bits_equal(out.NR.cpu().numpy(), NRr)
    Lr = O.assign_deciles(Sr, 10)
    EWr, CNTr, LSr = O.portfolio_ew(Lr, NRr, 10)
    assert np.array_equal(out.L.cpu().numpy(), Lr)
    assert np.array_equal(out.CNT.cpu().numpy(), CNTr)
    for got, want in ((out.EW, EWr), (out.LS, LSr)):
        g = got.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(want))
        assert max_rel(g, want) <= 1e-10
    assert (~np.isnan(LSr)).sum() >= T_M - Wm - 1
    if signal == "divol":   # an explicit window and min_obs reach the model
        o3 = engine.run_signal(pan["Pd"], pan["msd"], signal, window=3, min_obs=40, factors=FD3d)
        assert _ulps(o3.M.cpu().numpy(), _model_ref(pan, 3, 3, 40)["DIVOL"], "divol 3") <= MAX_ULP
        # without factors: today's path, the single-factor kernels
        base = engine.run_signal(pan["Pd"], pan["msd"], signal)
        want = engine.daily_signals(pan["Pd"], pan["msd"], (signal,))[signal]
        assert _same([base.M], [want]) and not _same([base.M], [out.M])
    for other in ("max", "dskew", "high52"):
        with pytest.raises(ValueError):
            engine.run_signal(pan["Pd"], pan["msd"], other, factors=FD3d)


# ------------------------------------------------------------------------ Dimson betas
def test_dimson_beta_through_lagged(engine):
    """Every asset's return is 0.5 mkt[d] + 0.25 mkt[d-1] plus noise on a dense panel: the sum of
    the slopes on lagged(mkt, 2) is the least-squares answer (within factor_ref's daily lstsq bar,
    scaled by the cell's largest coefficient) and near 0.75; the columns are lags 0, 1, 2."""
    rng = np.random.default_rng(2024)
    N, Wm = 64, 3
    _, ms = host_panel(N, "dense")
    mkt = rng.normal(0.0, 0.01, T_DAYS)
    lag1 = np.concatenate([[0.0], mkt[:-1]])
    r = 0.5 * mkt[:, None] + 0.25 * lag1[:, None] + rng.normal(0.0, 0.001, (T_DAYS, N))
    P = 50.0 * np.cumprod(1.0 + r, axis=0)
    Pd, msd, mktd = _up(P), _up(ms), _up(mkt)
    FDd = engine.lagged(mktd, 2)
    FD = FDd.cpu().numpy()
    assert FD.shape == (T_DAYS, 3) and np.isnan(FD[:2]).sum() == 3
    sums = engine.daily_fsums(Pd, msd, FDd, MAX_GAP)
    mod = engine.daily_fmodel(sums, Wm)
    R = DR.daily_ret(P, MAX_GAP)
    _check_sums(sums, FR.daily_fsums(R, FD, ms))
    dimson = mod.DBETA.sum(0).cpu().numpy()
    beta = mod.DBETA.cpu().numpy()
    frow = ~np.isnan(FD).any(axis=1)
    worst, cells = 0.0, 0
    for t in range(Wm - 1, T_M):
        lo, hi = int(ms[t - Wm + 1]), int(ms[t + 1])
        ok = frow[lo:hi].copy()
        ok[0] &= lo > 0                               # row 0 has no return
        A = np.concatenate([FD[lo:hi][ok], np.ones((int(ok.sum()), 1))], axis=1)
        for a in range(N):
            want = np.linalg.lstsq(A, R[lo:hi, a][ok], rcond=None)[0]
            worst = max(worst, abs(dimson[t, a] - want[:3].sum()) / np.abs(want).max())
            cells += 1
            assert abs(beta[0, t, a] - 0.5) < 0.1 and abs(beta[1, t, a] - 0.25) < 0.1
            assert abs(beta[2, t, a]) < 0.1 and abs(dimson[t, a] - 0.75) < 0.15
    print(f"Dimson sum vs lstsq: worst {worst:.3e} over {cells} cells")
    assert cells == (T_M - Wm + 1) * N and worst <= FR.LSTSQ_TOL["daily"]
    assert np.isnan(dimson[:Wm - 1]).all()
