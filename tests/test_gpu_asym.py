"""GPU: csm_asym_sums / csm_asym_model, Engine.run_signal's "info_disc", "rsj", "dsvol", "dnbeta"
and the host entries on them (rules AS1..AS7 in DESIGN.md 7) against the NumPy restatement in
tests/asym_ref.py, and against the kernels that walk the same days (csm_liq_sums, csm_daily_sums,
csm_daily_model) with no reference in the loop.

Bars.  The AS2 counts and sums, NOBS and NSIDE are sequential sums in the order the rules state:
bit for bit.  The AS3 outputs are chains of single correctly rounded + - * / sqrt on those sums;
fp64 / and sqrt are correctly rounded in this build (as test_gpu_signals.py records), so they are
held to bit equality too: MAX_ULP = 0, and the maximum found is printed.  Labels and counts of the
rankings are exact, EW / LS and the double sort's cells within the project's 1e-10.
"""
import ctypes

import numpy as np
import pytest
import torch

import asym_ref as AR
import dailymkt_ref as DR
import group_ref as GR
import signals_ref as SR
import xsreg_ref as XR
from conftest import bits_equal, max_rel
from oracle import csmom_oracle as O
from oracle import portfolio_oracle as PO
from oracle.synth_np import make_panel, to_long

pytestmark = pytest.mark.gpu
T_DAYS = 782            # 36 whole business-day months of 19..23 rows from 2000-01-03
GAPPY = dict(late=0.2, delist=0.2, nan_day=0.01, absent_month=0.01, nan_month=0.01)
DENSE = dict(late=0, delist=0, nan_day=0, absent_month=0, nan_month=0)
MAX_ULP = 0             # see the module docstring
GAP_COL = 5             # the hand-built column of the "gaps" panels
SIZES = [1, 2, 63, 130, 257, 514]   # odd and even, a partial wave, a second workgroup at
                                    # one (257) and at two (514) assets per lane
PAIR = (1, 2)           # csm_tune "asums_pair": one asset per lane | two where the panels allow
MODELS = ((1, 0, None), (3, 0, None), (12, 1, None), (6, 2, None), (36, 0, None), (3, 0, 1),
          (12, 1, 1))   # (Wm, skip, min_obs); min_obs 1 goes with min_side 2
_CACHE = {}


def _up(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _host(N, kind="gappy", max_gap=10):
    """Host panels and the AS1, AS2 reference; computed once and left unchanged."""
    key = (N, kind, max_gap)
    if key in _CACHE:
        return _CACHE[key]
    if kind == "calendar":   # calendar-day months of 28..31 rows: 2000-01 .. 2002-12
        pan = make_panel(N, 1096, seed=300 + N, cents=True, **GAPPY)
        lens = [31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31] + 2 * [31, 28, 31, 30, 31, 30, 31,
                                                                       31, 30, 31, 30, 31]
        ms = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        assert ms[-1] == 1096
    else:
        pan = make_panel(N, T_DAYS, seed=300 + N, cents=True,
                         **(DENSE if kind == "dense" else GAPPY))
        ms = pan["month_start"]
        d = np.diff(ms)
        assert len(ms) - 1 == 36 and d.min() >= 19 and d.max() <= 23
    P = pan["P"]
    if kind == "zero":       # month 4 has no day
        ms = np.concatenate([ms[:5], ms[4:]])
    if kind == "columns":    # a column without any price, and one without any row
        P[:, 3] = np.nan
        P[:, 4] = O.absent_like(P.shape[0])
    if kind == "gaps":       # dailymkt_ref.gap_column: gaps around max_gap, across chunk starts
        P[:, GAP_COL], _ = DR.gap_column(T_DAYS, max_gap, int(ms[8]), O.absent_scalar())
    FD = DR.daily_market(P, max_gap)["MKTD"]
    T_m = len(ms) - 1
    PM = SR.month_stats(P, ms)["PM"]
    rng = np.random.default_rng(700 + N)
    M = rng.standard_normal((T_m, N))            # a formation return of every sign rule's class
    M[rng.random((T_m, N)) < 0.1] = np.nan
    ref = AR.asym_sums(P, ms, FD, -1, max_gap)
    hand = int(np.argmax(ref["ND"].sum(axis=0)))   # the column with the most return days
    M[1::7, hand] = 0.0
    M[2::7, hand] = -0.0
    M[3::7, hand] = np.nan
    _CACHE[key] = dict(P=P, V=pan["V"], ms=ms, FD=FD, M=M, PM=PM, mod={}, mom={}, ref=ref,
                       hand=hand, max_gap=max_gap,
                       days=pan["days"], tickers=pan["tickers"])
    return _CACHE[key]


def _panel(N, kind="gappy", max_gap=10):
    pan = _host(N, kind, max_gap)
    if "Pd" not in pan:
        pan.update(Pd=_up(pan["P"]), msd=_up(pan["ms"]), FDd=_up(pan["FD"]), Md=_up(pan["M"]))
    return pan


def _model_ref(pan, Wm, skip=0, mo=None, M="M", ms=None):
    """The AS3 reference; min_obs 1 goes with min_side 2.  M: a key of pan, or an array."""
    key = (Wm, skip, mo, M if isinstance(M, str) else id(M), ms)
    if key not in pan["mod"]:
        Mh = pan[M] if isinstance(M, str) else M
        side = ms if ms is not None else (None if mo is None else max(2, mo))
        pan["mod"][key] = AR.asym_model(pan["ref"], Wm, skip, Mh, mo, side)
    return pan["mod"][key]


def _mom(pan, J, skip):
    if (J, skip) not in pan["mom"]:
        pan["mom"][(J, skip)] = O.momentum_scan(pan["PM"], J, skip)[1]
    return pan["mom"][(J, skip)]


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
    for k in AR.COUNTS + AR.SIDE_COUNTS:
        assert np.array_equal(getattr(sums, k).cpu().numpy(), ref[k]), k
    for k in AR.FSUMS + AR.SIDE_FSUMS:
        assert bits_equal(getattr(sums, k).cpu().numpy(), ref[k]), k


def _check_model(mod, ref, tag, keys=AR.MODEL[:4]):
    for k in ("NOBS", "NSIDE"):
        if getattr(mod, k) is not None:
            assert np.array_equal(getattr(mod, k).cpu().numpy(), ref[k]), k
    for k in keys:
        assert _ulps(getattr(mod, k).cpu().numpy(), ref[k], f"{k}{tag}") <= MAX_ULP, k


def _tune(key, value):
    import csmom
    assert csmom.load_library().csm_tune(key.encode(), ctypes.c_int(value)) == 0


def _model(engine, sums, pan, Wm, skip=0, mo=None, **kw):
    return engine.asym_model(sums, Wm, skip, pan["Md"], mo, None if mo is None else max(2, mo),
                             **kw)


def _run(engine, pan, Pd=None, models=MODELS):
    """asym_sums at one and at two assets per lane, then the models on the default's panels."""
    Pd = pan["Pd"] if Pd is None else Pd
    T_m = len(pan["ms"]) - 1
    try:
        for pair in (*PAIR, 0):
            _tune("asums_pair", pair)
            sums = engine.asym_sums(Pd, pan["msd"], pan["FDd"], -1, pan["max_gap"])
            _check_sums(sums, pan["ref"])
    finally:
        _tune("asums_pair", 0)
    for Wm, skip, mo in models:
        if Wm + skip <= T_m:
            _check_model(_model(engine, sums, pan, Wm, skip, mo), _model_ref(pan, Wm, skip, mo),
                         f"(Wm={Wm}, skip={skip}, min_obs={mo})")
    return sums


def _defined(pan, Wm, skip=0):
    """Shares of the cells from the first whole window on with RSJ, ID's day count and DNBETA
    defined at the default minimums."""
    ref = _model_ref(pan, Wm, skip)
    first = Wm + skip - 1
    return min(float((~np.isnan(ref["RSJ"][first:])).mean()),
               float((ref["NOBS"][first:] >= 15 * Wm).mean()),
               float((~np.isnan(ref["DNBETA"][first:])).mean()))


@pytest.mark.parametrize("N", SIZES)
def test_vs_ref_gappy(engine, N):
    pan = _panel(N)
    _run(engine, pan)
    if N >= 2:
        for Wm, skip in ((1, 0), (3, 0), (12, 1)):
            assert _defined(pan, Wm, skip) >= 0.5, (Wm, skip)
    if N >= 63:
        ref, M = pan["ref"], pan["M"]
        zero = int((ref["R"] == 0.0).sum())
        print(f"zero-return days {zero}")
        assert zero >= 1 and (ref["NUP"] + ref["NDN"] < ref["ND"]).any()
        assert (M > 0).any() and (M < 0).any() and np.isnan(M).any()
        assert (ref["NB"] < ref["ND"]).any()
        idr = _model_ref(pan, 1, 0, 1)["ID"][:, pan["hand"]]   # the hand-made cells of M
        days = ref["ND"][:, pan["hand"]] >= 1
        for first, zero_m in ((1, True), (2, True), (3, False)):
            hit = np.zeros(len(days), dtype=bool)
            hit[first::7] = days[first::7]
            assert hit.sum() >= 1, first
            if zero_m:                                # either zero of M gives +0.0
                assert (idr[hit] == 0.0).all() and not np.signbit(idr[hit]).any()
            else:
                assert np.isnan(idr[hit]).all()


@pytest.mark.parametrize("N", [63, 130])
def test_vs_ref_dense(engine, N):
    pan = _panel(N, "dense")
    _run(engine, pan)
    assert _defined(pan, 1) >= 0.5 and _defined(pan, 12, 1) >= 0.5
    assert (pan["ref"]["ND"][1:] == np.diff(pan["ms"])[1:, None]).all()   # a return every day


@pytest.mark.parametrize("max_gap", [1, 3, 10])
def test_max_gap(engine, max_gap):
    """The bound itself (gappy rows), and for max_gap >= 2 the hand-built column whose gaps are
    one under, at and one over the bound."""
    pan = _panel(257, "gappy" if max_gap == 1 else "gaps", max_gap)
    _run(engine, pan, models=((1, 0, None), (3, 0, None)))
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
        for k in AR.SUMS:
            assert (getattr(sums, k)[4] == 0).all(), k
    if kind == "calendar":
        assert int(engine.month_days(pan["msd"])[0]) == 31
    if kind == "columns":
        assert (sums.ND[:, 3:5] == 0).all() and (sums.SUP[:, 3:5] == 0).all()
        mod = engine.asym_model(sums, 1, 0, min_obs=1, min_side=2)
        assert torch.isnan(mod.DSVOL[:, 3:5]).all() and not torch.isnan(mod.DSVOL[:, 5]).all()
        assert torch.isnan(mod.DNBETA[:, 3:5]).all() and (mod.NSIDE[:, 3:5] == 0).all()


def test_unaligned_panel_takes_the_one_asset_path(engine):
    """Even N with P through a view 8 B past a 16-B boundary: under "asums_pair" = 2 too the call
    takes one asset per lane, and the bits are the paired path's."""
    pan = _panel(514)
    T_d, N = pan["P"].shape
    flat = torch.empty(T_d * N + 1, dtype=torch.float64, device="cuda:0")
    view = flat[1:].view(T_d, N)
    view.copy_(pan["Pd"])
    assert pan["Pd"].data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8
    _run(engine, pan, Pd=view, models=((1, 0, None),))


def _raw(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else t.dtype)


def _same(xs, ys):
    xs, ys = list(xs), list(ys)
    return len(xs) == len(ys) and all(torch.equal(_raw(a), _raw(b)) for a, b in zip(xs, ys))


def _fields(mod, keys=AR.MODEL):
    return [getattr(mod, k) for k in keys]


@pytest.mark.parametrize("N,kind", [(257, "gaps"), (514, "gappy"), (130, "zero")])
def test_launch_shape_changes_no_bit(engine, N, kind):
    pan = _panel(N, kind)
    T_m = len(pan["ms"]) - 1
    try:
        base = _run(engine, pan, models=())
        bare = engine.asym_sums(pan["Pd"], pan["msd"], max_gap=pan["max_gap"])
        for pair in PAIR:
            _tune("asums_pair", pair)
            for chunks in (1, 5, T_m, 0):
                _tune("asums_chunks", chunks)
                got = engine.asym_sums(pan["Pd"], pan["msd"], pan["FDd"], -1, pan["max_gap"])
                assert _same(got, base), (pair, chunks)
                got = engine.asym_sums(pan["Pd"], pan["msd"], max_gap=pan["max_gap"])
                assert _same(got[:5], bare[:5]) and _same(got[:5], base[:5]), (pair, chunks)
        for Wm, skip in ((1, 0), (3, 0), (12, 1)):
            _tune("amodel_chunks", 0)
            want = _model(engine, base, pan, Wm, skip)
            _check_model(want, _model_ref(pan, Wm, skip), f"(Wm={Wm}, skip={skip})")
            for chunks in (1, 5, T_m):
                _tune("amodel_chunks", chunks)
                got = _model(engine, base, pan, Wm, skip)
                assert _same(_fields(got), _fields(want)), (Wm, skip, chunks)
    finally:
        for k in ("asums_pair", "asums_chunks", "amodel_chunks"):
            _tune(k, 0)


def test_twice_the_same_bits(engine):
    pan = _panel(514)
    a, b = _run(engine, pan, models=((12, 1, None),)), _run(engine, pan, models=((12, 1, None),))
    assert _same(a, b)


# ------------------------------------------------- against the kernels that walk the same days
@pytest.mark.parametrize("N,kind", [(257, "gappy"), (130, "zero"), (514, "gappy")])
def test_day_counts_against_liq_sums(engine, N, kind):
    pan = _panel(N, kind)
    s = engine.asym_sums(pan["Pd"], pan["msd"], max_gap=pan["max_gap"])
    lq = engine.liq_sums(pan["Pd"], torch.ones_like(pan["Pd"]), pan["msd"], pan["max_gap"])
    assert torch.equal(s.ND, lq.ND)
    assert torch.equal(s.NUP + s.NDN, lq.ND - lq.NZR)
    assert int(lq.NZR.sum()) >= 1 and int(s.ND.sum()) > 1000


@pytest.mark.parametrize("N", [257, 514])
def test_side_sums_against_daily_sums(engine, N):
    """With every f below zero a side day is an observation of rule V3: the same bits."""
    pan = _panel(N)
    FD2 = -pan["FDd"].abs() - 1e-9               # NaN kept
    assert bool(torch.isnan(FD2).any()) and bool((FD2[~torch.isnan(FD2)] < 0).all())
    s = engine.asym_sums(pan["Pd"], pan["msd"], FD2, -1, pan["max_gap"])
    d = engine.daily_sums(pan["Pd"], pan["msd"], FD2, pan["max_gap"])
    assert _same([s.NB, s.BR, s.BF, s.BFF, s.BRF], [d.NO, d.SR, d.SF, d.SFF, d.SRF])
    assert int(s.NB.sum()) > 1000
    for W in (1, 3, 12):
        m = 15 * W
        a = engine.asym_model(s, window=W, skip=0, min_side=m, outputs=("DNBETA", "NSIDE"))
        b = engine.daily_model(d, window=W, min_obs=m, outputs=("DBETA", "NOBS"))
        assert _same([a.DNBETA, a.NSIDE], [b.DBETA, b.NOBS]), W
        assert float((~torch.isnan(a.DNBETA[W - 1:])).double().mean()) >= 0.5


def test_the_other_side_mirrors(engine):
    pan = _panel(257)
    dn = engine.asym_sums(pan["Pd"], pan["msd"], pan["FDd"], -1)
    up = engine.asym_sums(pan["Pd"], pan["msd"], -pan["FDd"], +1)
    assert _same([up.NB, up.BR, up.BFF], [dn.NB, dn.BR, dn.BFF])
    assert _same([up.BF, up.BRF], [0.0 - dn.BF, 0.0 - dn.BRF])   # (0.0 - x: a month's +0.0 stays)
    assert _same(up[:5], dn[:5])
    real_up = engine.asym_sums(pan["Pd"], pan["msd"], pan["FDd"], +1)
    ref_up = AR.asym_sums(pan["P"], pan["ms"], pan["FD"], +1)
    _check_sums(real_up, ref_up)
    assert not torch.equal(real_up.NB, dn.NB)
    both = real_up.NB + dn.NB
    assert bool((both <= dn.ND).all()) and int(both.sum()) > 1000


@pytest.mark.parametrize("W,s", [(1, 1), (3, 2), (12, 1), (6, 12)])
def test_skip_shifts_the_window(engine, W, s):
    pan = _panel(257)
    T_m = len(pan["ms"]) - 1
    sums = engine.asym_sums(pan["Pd"], pan["msd"], pan["FDd"])
    M0 = torch.full_like(pan["Md"], float("nan"))
    M0[:T_m - s] = pan["Md"][s:]                 # M0[t - s] = M[t]
    a = engine.asym_model(sums, W, s, pan["Md"], min_obs=10 * W, min_side=3 * W)
    b = engine.asym_model(sums, W, 0, M0, min_obs=10 * W, min_side=3 * W)
    _check_model(a, AR.asym_model(pan["ref"], W, s, pan["M"], 10 * W, 3 * W), f"(W={W}, s={s})")
    first = W + s - 1
    for k in AR.MODEL:
        x, y = getattr(a, k), getattr(b, k)
        assert _same([x[s:]], [y[:T_m - s]]), k
        head = x[:first]
        assert bool((head == 0).all() if head.dtype == torch.int32 else torch.isnan(head).all()), k
    assert float((~torch.isnan(a.RSJ[first:])).double().mean()) >= 0.5


# ------------------------------------------------------------------ nullable outputs and the API
def test_nullable_outputs_and_subsets(engine):
    import csmom
    pan = _panel(257)
    full = _run(engine, pan, models=())
    bare = engine.asym_sums(pan["Pd"], pan["msd"])
    assert all(getattr(bare, k) is None for k in AR.SIDE)
    assert _same(bare[:5], full[:5])
    ref = _model_ref(pan, 12, 1)
    mod = engine.asym_model(bare, 12, 1, pan["Md"])      # the default: what the sums and M allow
    assert mod.DNBETA is None and mod.NSIDE is None
    _check_model(mod, ref, "(no FD)", keys=("ID", "RSJ", "DSVOL"))
    mod = engine.asym_model(full, 12, 1)                 # no M: no ID, the others do not move
    assert mod.ID is None
    _check_model(mod, ref, "(no M)", keys=("RSJ", "DSVOL", "DNBETA"))
    with pytest.raises(csmom.CsmError) as e:
        engine.asym_model(bare, 12, 1, pan["Md"], outputs=("DNBETA",))
    assert e.value.status == -1
    with pytest.raises(csmom.CsmError):
        engine.asym_model(bare, 12, 1, outputs=("NSIDE",))
    with pytest.raises(csmom.CsmError) as e:
        engine.asym_model(full, 12, 1, outputs=("ID",))
    assert e.value.status == -1
    for k in AR.MODEL:                                   # one output at a time
        one = _model(engine, full, pan, 12, 1, outputs=(k,))
        assert [f for f in AR.MODEL if getattr(one, f) is not None] == [k]
        if k in ("NOBS", "NSIDE"):
            assert np.array_equal(getattr(one, k).cpu().numpy(), ref[k])
        else:
            assert _ulps(getattr(one, k).cpu().numpy(), ref[k], f"{k} alone") <= MAX_ULP
    # ID alone on the sums without side panels, RSJ alone without M
    one = engine.asym_model(bare, 12, 1, pan["Md"], outputs=("ID",))
    assert bits_equal(one.ID.cpu().numpy(), ref["ID"])
    # explicit minimums reach the kernel separately
    m = engine.asym_model(full, 3, 0, pan["Md"], min_obs=40, min_side=25)
    _check_model(m, _model_ref(pan, 3, 0, 40, ms=25), "(40, 25)")


def _ranking(out, ref, PM, n_bins=10):
    NRr = SR.next_ret(PM, ref)
    assert bits_equal(out.NR.cpu().numpy(), NRr)
    Lr = O.assign_deciles(ref, n_bins)
    EWr, CNTr, LSr = O.portfolio_ew(Lr, NRr, n_bins)
    assert np.array_equal(out.L.cpu().numpy(), Lr)
    assert np.array_equal(out.CNT.cpu().numpy(), CNTr)
    for got, want in ((out.EW, EWr), (out.LS, LSr)):
        g = got.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(want))
        assert max_rel(g, want) <= 1e-10
    return LSr


def _signal_ref(pan, signal, J=12, skip=1, window=None, mo=None):
    if signal == "info_disc":
        return _model_ref(pan, J, skip, mo, M=_mom(pan, J, skip))["ID"]
    w = (12 if signal == "dnbeta" else 1) if window is None else window
    return _model_ref(pan, w, 0, mo)[{"rsj": "RSJ", "dsvol": "DSVOL", "dnbeta": "DNBETA"}[signal]]


@pytest.mark.parametrize("signal", ["info_disc", "rsj", "dsvol", "dnbeta"])
def test_run_signal(engine, signal):
    pan = _panel(257)
    ref = _signal_ref(pan, signal)
    out = engine.run_signal(pan["Pd"], pan["msd"], signal)
    assert bits_equal(out.PM.cpu().numpy(), pan["PM"])
    assert _ulps(out.M.cpu().numpy(), ref, signal) <= MAX_ULP
    LSr = _ranking(out, ref, pan["PM"])
    assert (~np.isnan(LSr)).sum() >= 36 - 12 - 2
    if signal == "info_disc":     # J and skip reach the model and the formation return
        m = _mom(pan, 12, 1)
        assert (m > 0).any() and (m < 0).any() and np.isnan(m).any()
        o6 = engine.run_signal(pan["Pd"], pan["msd"], signal, J=6, skip=2)
        r6 = _signal_ref(pan, signal, 6, 2)
        assert bits_equal(o6.M.cpu().numpy(), r6) and not bits_equal(r6[20:], ref[20:])
        _ranking(o6, r6, pan["PM"])
        ow = engine.run_signal(pan["Pd"], pan["msd"], signal, window=3)    # window does not apply
        assert _same([ow.M], [out.M])
        om = engine.run_signal(pan["Pd"], pan["msd"], signal, min_obs=200)
        assert bits_equal(om.M.cpu().numpy(), _signal_ref(pan, signal, mo=200))
    else:                         # an explicit window and min_obs reach the model
        o3 = engine.run_signal(pan["Pd"], pan["msd"], signal, window=3, min_obs=20)
        assert bits_equal(o3.M.cpu().numpy(), _signal_ref(pan, signal, window=3, mo=20))
        assert not bits_equal(o3.M.cpu().numpy()[12:], ref[12:])


def test_run_signal_refusals_and_old_calls(engine):
    pan = _panel(63)
    Pd, msd = pan["Pd"], pan["msd"]
    FD = torch.zeros((Pd.shape[0], 1), dtype=torch.float64, device="cuda:0")
    V = torch.ones_like(Pd)
    for signal in engine.ASYM_SIGNALS:
        for kw in (dict(V=V), dict(HLC=(Pd, Pd, Pd)), dict(factors=FD)):
            with pytest.raises(ValueError):
                engine.run_signal(Pd, msd, signal, **kw)
    with pytest.raises(ValueError):
        engine.run_signal(Pd, msd, "frog")
    assert set(engine.ASYM_SIGNALS) < set(engine.RUN_SIGNALS)
    assert engine.RUN_SIGNALS[-6:] == ("pkvol", "cs_spread", "ar_spread", "illiq", "dvol", "zret")
    # an old signal is the calls it was before: daily_market, daily_sums, daily_model
    a = engine.run_signal(Pd, msd, "dbeta")
    MKTD, _ = engine.daily_market(Pd, 10)
    dm = engine.daily_model(engine.daily_sums(Pd, msd, MKTD, 10, with_sr3=False, with_rmax=False),
                            12, outputs=("DBETA",))
    assert _same([a.M], [dm.DBETA]) and bool((~torch.isnan(a.M)).any())


def test_build_signals(engine):
    from csmom.regress import SIGNAL_NAMES, build_signals
    pan = _panel(257)
    names = ("rsj", "rev", "info_disc", "dnbeta", "mom", "dsvol")
    S, X = build_signals(engine, pan["Pd"], pan["msd"], names)
    for n, s in zip(names, S):
        if n in engine.ASYM_SIGNALS:
            assert bits_equal(s.cpu().numpy(), _signal_ref(pan, n)), n
    assert torch.equal(_raw(S[1]), _raw(X))
    S3, _ = build_signals(engine, pan["Pd"], pan["msd"], ("dsvol", "info_disc"), J=6, skip=2,
                          window=3)
    assert bits_equal(S3[0].cpu().numpy(), _signal_ref(pan, "dsvol", window=3))
    assert bits_equal(S3[1].cpu().numpy(), _signal_ref(pan, "info_disc", 6, 2))
    assert set(engine.ASYM_SIGNALS) <= set(SIGNAL_NAMES)


def _frame(pan):
    return to_long(dict(P=pan["P"], V=pan["V"], days=pan["days"], tickers=pan["tickers"]))


def _dense_ref(df, max_gap=10):
    from csmom.panel import from_long
    dense = from_long(df)        # the frame's own dense layout
    FD = DR.daily_market(dense.P, max_gap)["MKTD"]
    PM = SR.month_stats(dense.P, dense.month_start)["PM"]
    return dense, AR.asym_sums(dense.P, dense.month_start, FD, -1, max_gap), PM


def test_asymmetry_signals_from_a_daily_frame(engine):
    import csmom
    pan = _panel(63)
    df = _frame(pan)
    dense, sums, PM = _dense_ref(df)
    M = O.momentum_scan(PM, 6, 2)[1]
    form = AR.asym_model(sums, 6, 2, M, 60, 60)
    month, year = AR.asym_model(sums, 1, 0, None, 60, 60), AR.asym_model(sums, 12, 0, None, 60, 60)
    got = csmom.asymmetry_signals(df, J=6, skip=2, min_obs=60, device=0)
    assert list(got.columns) == csmom.ASYMMETRY_COLUMNS
    aa, mm = np.nonzero(~O.is_absent(PM).T)
    assert len(got) == len(aa) and (got["ticker"].to_numpy() == dense.tickers[aa]).all()
    assert (got["date"].to_numpy() == dense.month_end[mm].to_numpy()).all()
    for col, ref in (("info_disc", form["ID"]), ("rsj", month["RSJ"]), ("dsvol", month["DSVOL"]),
                     ("dnbeta", year["DNBETA"])):
        assert bits_equal(got[col].to_numpy(), ref[mm, aa]), col
    assert np.array_equal(got["nobs"].to_numpy(), form["NOBS"][mm, aa])
    assert np.isnan(got["rsj"]).all()            # no month has 60 return days ...
    assert got["info_disc"].notna().mean() >= 0.5 and got["dnbeta"].notna().mean() >= 0.5
    dflt = csmom.asymmetry_signals(df, device=0)  # ... and the defaults are asym_signals'
    assert bits_equal(dflt["rsj"].to_numpy(), AR.asym_model(sums, 1, 0)["RSJ"][mm, aa])
    assert dflt["rsj"].notna().mean() >= 0.5
    assert csmom.asymmetry_signals(df.iloc[:0], device=0) is None


def test_tables_from_a_daily_frame(engine):
    """fama_macbeth and information_coefficient take the asymmetry names."""
    import csmom
    pan = _panel(130)
    df = _frame(pan)
    fm = csmom.fama_macbeth(df, signals=("mom", "info_disc", "rsj"), device=0)
    assert list(fm.table.index) == ["const", "mom", "info_disc", "rsj"]
    assert np.isfinite(fm.table[["mean", "se", "t"]].to_numpy()).all()
    assert (fm.table["months"] >= 20).all()
    ic = csmom.information_coefficient(df, signals=("dnbeta",), horizons=(1, 3), device=0)
    assert np.isfinite(ic.table[["mean", "se", "t"]].to_numpy()).all() and len(ic.table) == 2


def test_frog_in_the_pan(engine):
    import csmom
    pan = _panel(257)
    df = _frame(pan)
    n_id, n_mom = 3, 5
    dense, sums, PM = _dense_ref(df)
    T_m = PM.shape[0]
    M = O.momentum_scan(PM, 12, 1)[1]
    ID = AR.asym_model(sums, 12, 1, M)["ID"]
    Mx = np.where(np.isnan(ID), np.nan, M)
    NR = SR.next_ret(PM, Mx)
    L1 = O.assign_deciles(ID, n_id)
    L2 = GR.group_labels(Mx, L1.astype(np.int16), n_id, n_mom)
    Lc = np.where((L1 >= 0) & (L2 >= 0), n_mom * L1.astype(np.int64) + L2, -1).astype(np.int8)
    assert (Lc[13:-1] >= 0).mean() >= 0.5
    want = PO.portfolio(Lc, NR, n_id * n_mom, K=1)["PR"][:, 0, :].reshape(T_m, n_id, n_mom)
    # the labels, through the engine calls frog_in_the_pan makes
    Pd, msd = _up(dense.P), _up(dense.month_start)
    PMd, _ = engine.month_end(Pd, msd)
    IDd = engine.asym_signals(Pd, msd, ("info_disc",), 12, 1, PM=PMd)["info_disc"]
    assert bits_equal(IDd.cpu().numpy(), ID)
    Mxd = engine.mask_by(IDd, engine.momentum(PMd, 12, 1)[1])
    ds = csmom.dependent_double_sort(engine, IDd, Mxd, engine.next_ret(PMd, Mxd), n1=n_id,
                                     n2=n_mom, K=1)
    assert np.array_equal(ds.Lm.cpu().numpy(), L1) and np.array_equal(ds.Lv.cpu().numpy(), L2)
    assert np.array_equal(ds.Lc.cpu().numpy(), Lc)
    # 15 cells are more than one csm_portfolio call takes: the ID bins are accounted one at a
    # time, which gives the cells of the joint call where both can run (2 x 5, K = 1 and 3)
    from csmom.lesw import PORTFOLIO_BINS, cell_returns
    assert n_id * n_mom not in PORTFOLIO_BINS and 2 * n_mom in PORTFOLIO_BINS
    L1b, _, _, _ = engine.deciles(IDd, None, 2)
    L2b, _, _ = engine.deciles_within(Mxd, None, L1b.to(torch.int16), 2, n_mom)
    NRd = engine.next_ret(PMd, Mxd)
    for K in (1, 3):
        one = cell_returns(engine, L1b, L2b, NRd, 2, n_mom, K, joint=True).cpu().numpy()
        per = cell_returns(engine, L1b, L2b, NRd, 2, n_mom, K, joint=False).cpu().numpy()
        assert np.array_equal(np.isnan(one), np.isnan(per)) and (~np.isnan(one)).mean() >= 0.5
        assert max_rel(per, one) <= 1e-10, K
    r = csmom.frog_in_the_pan(df, J=12, skip=1, n_id=n_id, n_mom=n_mom, K=1, device=0)
    assert _same([r.cells], [ds.PR])
    cells = r.cells.cpu().numpy()
    assert np.array_equal(np.isnan(cells), np.isnan(want))
    ok = ~np.isnan(want)
    assert (np.abs(cells[ok] - want[ok]) <= 1e-10 * np.maximum(np.abs(want[ok]), 1e-12)
            + 1e-15).all(), max_rel(cells, want)
    ls = r.long_short.to_numpy()
    assert list(r.long_short.columns) == list(range(n_id)) and ls.shape == (T_m, n_id)
    assert (r.long_short.index == dense.month_end).all()
    assert bits_equal(ls, cells[:, :, n_mom - 1] - cells[:, :, 0])
    assert bits_equal(r.spread.to_numpy(), ls[:, 0] - ls[:, n_id - 1])
    assert (~np.isnan(r.spread.to_numpy())).sum() >= 36 - 12 - 2
    series = np.concatenate([ls, r.spread.to_numpy()[:, None]], axis=1)
    assert r.lags == XR.default_lags(T_m)
    nw = XR.newey_west(series, r.lags)
    assert list(r.table.index) == [*range(n_id), "spread"]
    for col, k in (("mean", "MEAN"), ("se", "SE"), ("t", "T")):
        assert bits_equal(r.table[col].to_numpy(), nw[k]), col
    assert np.array_equal(r.table["months"].to_numpy(), nw["NT"])
    assert np.isfinite(r.table[["mean", "se", "t"]].to_numpy()).all()
    r5 = csmom.frog_in_the_pan(df, K=3, device=0)             # the default 5 x 5, held 3 months
    assert tuple(r5.cells.shape) == (T_m, 5, 5) and list(r5.table.index) == [*range(5), "spread"]
    assert np.isfinite(r5.table[["mean", "se", "t"]].to_numpy()).all()
    assert (r5.table["months"] >= 36 - 12 - 2).all()
    assert csmom.frog_in_the_pan(df.iloc[:0], device=0) is None


SENTINEL = 12345.0


def _refused(engine, name, args, outs):
    import csmom
    with pytest.raises(csmom.CsmError) as e:
        engine._call(name, *args)
    assert e.value.status == -1   # CSM_E_INVAL
    torch.cuda.synchronize()
    for t in outs:                # nothing was launched
        assert (t == (SENTINEL if t.dtype == torch.float64 else 77)).all()


def _filled(T_m, N, dtypes):
    return [torch.full((T_m, N), 77 if d == torch.int32 else SENTINEL, dtype=d, device="cuda:0")
            for d in dtypes]


def test_bad_arguments_are_refused(engine):
    import csmom
    from csmom.engine import _ptr
    pan = _panel(63)
    Pd, FDd, msd = pan["Pd"], pan["FDd"], pan["msd"]
    T_d, N = Pd.shape
    T_m = msd.numel() - 1
    i32, f64 = torch.int32, torch.float64
    outs = _filled(T_m, N, [i32, i32, i32, f64, f64, i32, f64, f64, f64, f64])   # AR.SUMS' order

    def sums(P=Pd, FD=FDd, ms=msd, tm=T_m, mmd=23, gap=10, side=-1, o=range(10), td=T_d):
        ptrs = [_ptr(t) if i in o else None for i, t in enumerate(outs)]
        return (_ptr(P), _ptr(FD), td, N, _ptr(ms), tm, mmd, gap, side, *ptrs)

    bad = [sums(gap=0), sums(gap=33), sums(mmd=0), sums(mmd=33), sums(tm=0), sums(td=0),
           sums(P=None), sums(ms=None), sums(side=0), sums(side=2), sums(side=-2),
           sums(o=range(5)),                       # FD without the side panels
           sums(FD=None),                          # the side panels without FD
           sums(FD=None, o=(0, 1, 2, 3, 4, 5))]    # one of them without FD
    bad += [sums(o=[j for j in range(10) if j != i]) for i in range(10)]   # any one missing
    for args in bad:
        _refused(engine, "csm_asym_sums", args, outs)
    for kw in (dict(max_gap=0), dict(max_gap=33), dict(side=0)):
        with pytest.raises(csmom.CsmError):
            engine.asym_sums(Pd, msd, FDd, **kw)
    engine._call("csm_asym_sums", *sums(FD=None, o=range(5)))    # without FD: the first five
    assert _same(outs[:5], engine.asym_sums(Pd, msd)[:5])
    assert all(bool((t == (SENTINEL if t.dtype == f64 else 77)).all()) for t in outs[5:])

    s = engine.asym_sums(Pd, msd, FDd)
    ins = [_ptr(t) for t in s] + [_ptr(pan["Md"])]
    g = _filled(T_m, N, [f64, f64, f64, f64, i32, i32])                          # AR.MODEL's order

    def model(ins=ins, tm=T_m, Wm=1, skip=0, mo=15, side=5, o=range(6)):
        ptrs = [_ptr(t) if i in o else None for i, t in enumerate(g)]
        return (*ins, tm, N, Wm, skip, mo, side, *ptrs)

    def without(*idx):
        return [None if i in idx else p for i, p in enumerate(ins)]

    bad = [model(Wm=0), model(Wm=37), model(skip=-1), model(skip=13), model(mo=0), model(side=1),
           model(tm=0), model(o=()),
           model(ins=without(10)),                 # ID without M
           model(ins=without(10), o=(0,)),
           model(ins=without(5, 6, 7, 8, 9)),      # DNBETA and NSIDE without the side panels
           model(ins=without(5, 6, 7, 8, 9), o=(3,)), model(ins=without(5, 6, 7, 8, 9), o=(5,)),
           model(ins=without(7)), model(ins=without(7), o=(1,))]   # a side panel on its own
    bad += [model(ins=without(i)) for i in range(5)]
    for args in bad:
        _refused(engine, "csm_asym_model", args, g)
    # without the nullable inputs the other outputs are served
    engine._call("csm_asym_model", *model(ins=without(5, 6, 7, 8, 9, 10), o=(1, 2, 4)))
    ref = _model_ref(pan, 1, 0, 15, ms=5)
    assert bits_equal(g[1].cpu().numpy(), ref["RSJ"]) and bits_equal(g[2].cpu().numpy(),
                                                                    ref["DSVOL"])
    assert np.array_equal(g[4].cpu().numpy(), ref["NOBS"])
    for kw in (dict(window=0), dict(window=37), dict(skip=-1), dict(skip=13), dict(min_obs=0),
               dict(min_side=1)):
        with pytest.raises(csmom.CsmError) as e:
            engine.asym_model(s, **kw)
        assert e.value.status == -1
    with pytest.raises(ValueError):
        engine.asym_model(s, outputs=("RSJ", "XX"))
