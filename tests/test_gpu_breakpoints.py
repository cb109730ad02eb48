"""GPU: csm_deciles_bp / csm_screen and what is built on them (rules U1..U6 in DESIGN.md 7)
against the NumPy restatement in tests/bp_ref.py, which the CPU tests pin to the reference and to
pandas.

Inputs are synthetic signals made directly: normal draws rounded to cents (ties), 20 % NaN, 1 %
ABSENT, next returns with 10 % NaN, masks whose non-zero bytes are 1, 2, 128 and 255.

Bars.  L, CNT, NV, NVB and NE are exact.  EDGES equal the ref with == (the sign of a zero is free)
and the NaN padding matches.  EW and the long-short are within the project's 1e-10 relative of the
ref's Kahan sums in asset order.  Two calls give the same bits.

The kernels have one hand-over length: a breakpoint set of at most 4,096 values is sorted in LDS,
a larger one in tiles; test_handover_lengths puts sets of 4,095, 4,096, 4,097 and 8,193 values on
its dates.  csm_tune "gdec_small_cap" lowers that length; test_lowered_cap runs the tiled sort
with several tiles on 1,000-asset rows at a cap of 64.

Every parametrised case asserts that at least half of its ranked cells carry a label >= 0 in the
ref, so nothing passes on -1s; the named degenerate cases assert exactly their degenerate output.
"""
import ctypes

import numpy as np
import pytest
import torch

import bp_ref as BR
from conftest import bits_equal, max_rel
from oracle import csmom_oracle as O

pytestmark = pytest.mark.gpu

REL = 1e-10
_CACHE = {}
NAN = np.nan


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def make_case(T_m, N, static, seed, frac=0.3, nan=0.2):
    """M, NR [T_m][N], BP uint8 [N] or [T_m][N] with a share `frac` of non-zero bytes."""
    rng = np.random.default_rng(seed)
    M = np.round(rng.normal(0.0, 0.1, (T_m, N)), 2)
    M[rng.random((T_m, N)) < nan] = NAN
    if nan > 0:
        M[rng.random((T_m, N)) < 0.01] = O.absent_scalar()
    NR = rng.normal(0.01, 0.08, (T_m, N))
    NR[rng.random((T_m, N)) < 0.1] = NAN
    shape = (N,) if static else (T_m, N)
    BP = np.where(rng.random(shape) < frac,
                  rng.choice(np.array([1, 2, 128, 255], dtype=np.uint8), size=shape), 0)
    return M, NR, BP.astype(np.uint8)


def ref_case(key, M, NR, BP, nb):
    if key not in _CACHE:
        _CACHE[key] = BR.deciles_bp(M, NR, BP, nb)
    return _CACHE[key]


def _close(got, ref, what):
    g = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert np.array_equal(np.isnan(g), np.isnan(ref)), what
    m = ~np.isnan(ref)
    scale = np.maximum(np.abs(ref[m]), 1e-12)
    assert (np.abs(g[m] - ref[m]) <= REL * scale + 1e-15).all(), (what, max_rel(g, ref))


def _edges_equal(got, ref):
    g = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert np.array_equal(np.isnan(g), np.isnan(ref))
    assert (g[~np.isnan(ref)] == ref[~np.isnan(ref)]).all()


def half_labelled(ref, M):
    ranked = ~np.isnan(M)
    return (ref["L"][ranked] >= 0).mean() >= 0.5


def check_bp(engine, M, NR, BP, nb, ref):
    Md, NRd, Bd = _up(M), _up(NR), _up(BP)
    out = engine.deciles_bp(Md, NRd, Bd, nb, with_nv=True, with_edges=True)
    L, EW, CNT, NV, NVB, EDGES, NE = out
    LS = engine.long_short(EW, CNT)
    torch.cuda.synchronize()
    assert np.array_equal(L.cpu().numpy(), ref["L"])
    assert np.array_equal(CNT.cpu().numpy(), ref["CNT"])
    assert np.array_equal(NV.cpu().numpy(), ref["NV"])
    assert np.array_equal(NVB.cpu().numpy(), ref["NVB"])
    assert np.array_equal(NE.cpu().numpy(), ref["NE"])
    _edges_equal(EDGES, ref["EDGES"])
    _close(EW, ref["EW"], "EW")
    _close(LS, ref["LS"], "LS")
    again = engine.deciles_bp(Md, NRd, Bd, nb, with_nv=True, with_edges=True)
    for a, b in zip(out, again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    L0, _, _ = engine.deciles_bp(Md, None, Bd, nb)          # labels only
    assert torch.equal(L0, L)
    E1, NE1, NVB1 = engine.breakpoints(Md, Bd, nb)          # the edges alone
    assert torch.equal(E1.view(torch.int64), EDGES.view(torch.int64))
    assert torch.equal(NE1, NE) and torch.equal(NVB1, NVB)
    return out


# (T_m, N, static mask, n_bins, the mask's share of the assets)
CASES = [
    (3, 63, True, 10, 0.3),
    (3, 64, False, 5, 0.5),
    (2, 65, True, 3, 0.3),
    (3, 257, False, 10, 0.3),
    (12, 1000, True, 10, 0.3),
    (3, 1000, False, 20, 0.5),
    (3, 1000, True, 2, 0.1),
    (3, 1000, False, 4, 0.3),
    (3, 20000, True, 10, 0.3),      # about 4,700 breakpoint values per date: the tiled sort
    (2, 20000, False, 5, 0.1),      # about 1,600: the LDS sort
]


@pytest.mark.parametrize("T_m,N,static,nb,frac", CASES)
def test_deciles_bp_vs_ref(engine, T_m, N, static, nb, frac):
    M, NR, BP = make_case(T_m, N, static, seed=N + nb, frac=frac)
    ref = ref_case((T_m, N, static, nb, frac), M, NR, BP, nb)
    assert half_labelled(ref, M)
    assert set(np.unique(BP).tolist()) - {0, 1} or N < 100   # bytes other than 0 and 1
    if N == 20000:
        assert (ref["NVB"] > 4096).all() if static else (ref["NVB"] < 4096).all()
    check_bp(engine, M, NR, BP, nb, ref)


@pytest.mark.parametrize("N", [2, 3])
def test_tiny_rows(engine, N):
    rng = np.random.default_rng(N)
    M = rng.normal(0.0, 0.1, (4, N))
    NR = rng.normal(0.01, 0.08, (4, N))
    BP = np.full(N, 7, dtype=np.uint8)
    BP[N - 1] = 0 if N == 3 else 7
    ref = ref_case(("tiny", N), M, NR, BP, 2)
    assert half_labelled(ref, M) and (ref["NE"] == 3).all()
    check_bp(engine, M, NR, BP, 2, ref)


def test_handover_lengths(engine):
    """Breakpoint sets of 4,095 / 4,096 (LDS) and 4,097 / 8,193 (tiled) values, per-month mask."""
    T_m, N, nb = 4, 20000, 10
    M, NR, _ = make_case(T_m, N, False, seed=41)
    BP = np.zeros((T_m, N), dtype=np.uint8)
    rng = np.random.default_rng(42)
    for t, k in enumerate((4095, 4096, 4097, 8193)):
        ok = np.nonzero(~np.isnan(M[t]))[0]
        BP[t, rng.choice(ok, size=k, replace=False)] = 255
        BP[t, np.nonzero(np.isnan(M[t]))[0][:50]] = 1       # NaN cells never join the set
    ref = ref_case("handover", M, NR, BP, nb)
    assert ref["NVB"].tolist() == [4095, 4096, 4097, 8193] and half_labelled(ref, M)
    check_bp(engine, M, NR, BP, nb, ref)


def lowered_cap_cases():
    """(name, M, NR, BP, n_bins) of test_lowered_cap."""
    M, NR, BP = make_case(3, 1000, True, seed=7, nan=0.1)    # about 270 breakpoint cells a date
    yield "static", M, NR, BP, 10
    T_m, N = 4, 1000
    M, NR, _ = make_case(T_m, N, False, seed=6)
    BP = np.zeros((T_m, N), dtype=np.uint8)
    rng = np.random.default_rng(7)
    for t, k in enumerate((64, 65, 128, 129)):
        BP[t, rng.choice(np.nonzero(~np.isnan(M[t]))[0], size=k, replace=False)] = 255
    yield "handover", M, NR, BP, 10


def test_lowered_cap(engine):
    """gdec_small_cap = 64: k_bpedges follows the knob, so about 270 breakpoint cells a date are
    three 128-key tiles merged through the packed row, and sets of 64 / 65 / 128 / 129 cells are
    the hand-over, a one-tile and a two-tile tiled sort.  Exact against the ref, and every output
    bit for bit what the default cap gives."""
    for name, M, NR, BP, nb in lowered_cap_cases():
        ref = ref_case(("cap64", name), M, NR, BP, nb)
        assert half_labelled(ref, M)
        if name == "handover":
            assert ref["NVB"].tolist() == [64, 65, 128, 129]
        else:
            assert ((ref["NVB"] > 256) & (ref["NVB"] <= 384)).all()
        at_default = check_bp(engine, M, NR, BP, nb, ref)
        assert engine.lib.csm_tune(b"gdec_small_cap", 64) == 0
        try:
            at_64 = check_bp(engine, M, NR, BP, nb, ref)
        finally:
            assert engine.lib.csm_tune(b"gdec_small_cap", 4096) == 0
        for a, b in zip(at_64, at_default):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_inner_subset_leaves_both_tails_outside(engine):
    """The subset: the cells whose |M| is below the date's median |M|.  A quarter of the ranked
    cells lies below e_0 and a quarter above e_m; they get bin 0 and the top bin."""
    T_m, N, nb = 3, 1000, 10
    M, NR, _ = make_case(T_m, N, True, seed=77)
    med = np.nanmedian(np.abs(M), axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        BP = (np.abs(M) < med).astype(np.uint8)
    ref = ref_case("inner", M, NR, BP, nb)
    assert half_labelled(ref, M)
    for t in range(T_m):
        ranked = ~np.isnan(M[t])
        e = ref["EDGES"][t, :ref["NE"][t]]
        below, above = ranked & (M[t] < e[0]), ranked & (M[t] > e[-1])
        assert below.sum() >= 0.1 * ranked.sum() and above.sum() >= 0.1 * ranked.sum()
        assert (ref["L"][t][below] == 0).all() and (ref["L"][t][above] == len(e) - 2).all()
    check_bp(engine, M, NR, BP, nb, ref)


@pytest.mark.parametrize("N", [1000, 20000])
def test_all_ones_equals_plain_deciles(engine, N):
    M, NR, _ = make_case(3, N, True, seed=N)
    Md, NRd = _up(M), _up(NR)
    ones = torch.ones(N, dtype=torch.bool, device=Md.device)     # (a bool mask is taken as bytes)
    L, EW, CNT, NV, NVB = engine.deciles_bp(Md, NRd, ones, 10, with_nv=True)
    L0, EW0, CNT0, NV0 = engine.deciles(Md, NRd, 10, with_nv=True)
    assert (L0 >= 0).float().mean().item() >= 0.5
    assert torch.equal(L, L0) and torch.equal(CNT, CNT0) and torch.equal(NV, NV0)
    assert torch.equal(NVB, NV0)
    _close(EW, EW0.cpu().numpy(), "EW")


def test_degenerate_cases(engine):
    T_m, N, nb = 6, 257, 10
    M, NR, _ = make_case(T_m, N, False, seed=11)
    ok = [np.nonzero(~np.isnan(M[t]))[0] for t in range(T_m)]
    BP = np.zeros((T_m, N), dtype=np.uint8)
    # 0: an empty subset (its only set bytes sit on NaN cells)   1: a one-value subset
    BP[0, np.nonzero(np.isnan(M[0]))[0]] = 1
    BP[1, ok[1][3]] = 1
    # 2: an all-equal subset   3: a date with all NaN   4: a two-value subset   5: ranked as usual
    M[2, ok[2][:40]] = 0.25
    BP[2, ok[2][:40]] = 9
    M[3, :] = NAN
    M[3, ::7] = O.absent_scalar()
    BP[3, :] = 1
    lo, hi = ok[4][0], ok[4][1]
    M[4, lo], M[4, hi] = -0.005, 0.015
    BP[4, [lo, hi]] = 1
    BP[5, ok[5][::3]] = 1
    ref = BR.deciles_bp(M, NR, BP, nb)
    L, EW, CNT, NV, NVB, EDGES, NE = check_bp(engine, M, NR, BP, nb, ref)
    L, EW, CNT, EDGES = L.cpu().numpy(), EW.cpu().numpy(), CNT.cpu().numpy(), EDGES.cpu().numpy()
    assert NVB.tolist() == [0, 1, 40, 0, 2, len(ok[5][::3])]
    assert NE.tolist()[:5] == [0, 1, 1, 0, nb + 1] and NE[5].item() > 5
    for t in (0, 1, 2, 3):
        assert (L[t] == -1).all() and (CNT[t] == 0).all() and np.isnan(EW[t]).all()
    assert np.isnan(EDGES[0]).all() and np.isnan(EDGES[3]).all()
    assert EDGES[1, 0] == M[1, ok[1][3]] and np.isnan(EDGES[1, 1:]).all()
    assert EDGES[2, 0] == 0.25 and np.isnan(EDGES[2, 1:]).all()
    assert NV.tolist() == (~np.isnan(M)).sum(axis=1).tolist() and NV[3].item() == 0
    # the two-value subset: n_bins + 1 distinct edges from -0.005 to 0.015, every ranked cell labelled
    assert not np.isnan(EDGES[4]).any() and (np.diff(EDGES[4]) > 0).all()
    assert EDGES[4, 0] == -0.005 and EDGES[4, nb] == 0.015
    r4 = ~np.isnan(M[4])
    assert (L[4][r4] >= 0).all() and L[4, lo] == 0 and L[4, hi] == nb - 1
    assert set(np.unique(L[4][r4]).tolist()) >= {0, nb - 1} and CNT[4].sum() > 100
    # N = 1: one value is never enough for two edges
    one = engine.deciles_bp(_up(np.array([[0.5], [NAN]])), _up(np.array([[0.1], [0.2]])),
                            _up(np.ones(1, dtype=np.uint8)), nb, with_nv=True, with_edges=True)
    assert one[0].tolist() == [[-1], [-1]] and one[2].sum().item() == 0
    assert torch.isnan(one[1]).all()
    assert one[3].tolist() == [1, 0] and one[4].tolist() == [1, 0] and one[6].tolist() == [1, 0]
    assert one[5][0, 0].item() == 0.5 and torch.isnan(one[5]).sum().item() == 2 * (nb + 1) - 1


def _screen_case(T_m, N, seed):
    M, _, _ = make_case(T_m, N, True, seed)
    rng = np.random.default_rng(seed + 1)
    PM = np.round(rng.lognormal(2.0, 1.0, (T_m, N)), 2)
    PM[rng.random((T_m, N)) < 0.05] = NAN
    PM[rng.random((T_m, N)) < 0.02] = O.absent_scalar()
    PM[0, :8] = 5.0                                          # on the floor: kept
    with np.errstate(invalid="ignore"):                      # (the ABSENT payload signals)
        CAP = PM * np.round(rng.lognormal(10.0, 2.0, N))
    CAP[rng.random((T_m, N)) < 0.03] = NAN
    return M, PM, CAP


@pytest.mark.parametrize("T_m,N", [(3, 65), (4, 1000), (2, 20000)])
def test_screen(engine, T_m, N):
    M, PM, CAP = _screen_case(T_m, N, seed=N)
    CAPMIN = np.nanquantile(CAP, 0.1, axis=1)
    if T_m > 3:
        CAPMIN[3] = NAN                                      # fails the whole date
    Md, PMd, Cd, CMd = _up(M), _up(PM), _up(CAP), _up(CAPMIN)
    for args, dev in (((PM, 5.0, CAP, CAPMIN), (PMd, 5.0, Cd, CMd)),
                      ((PM, 5.0, None, None), (PMd, 5.0, None, None)),
                      ((None, None, CAP, CAPMIN), (None, None, Cd, CMd)),
                      ((None, None, None, None), (None, None, None, None))):
        MS, KEPT = BR.screen(M, *args)
        got, kept = engine.screen(Md, *dev, with_kept=True)
        assert bits_equal(got.cpu().numpy(), MS)              # M's own bits where kept, NaN elsewhere
        assert np.array_equal(kept.cpu().numpy(), KEPT)
        assert torch.equal(engine.screen(Md, *dev).view(torch.int64), got.view(torch.int64))
    MS, KEPT = BR.screen(M, PM, 5.0, CAP, CAPMIN)
    ranked = (~np.isnan(M)).sum()
    assert 0.2 * ranked < KEPT.sum() < 0.9 * ranked           # the screens bite, and not everything
    assert np.isnan(PM[~np.isnan(M)]).any() and O.is_absent(PM).any()
    if T_m > 3:
        assert KEPT[3] == 0


def _daily_panel():
    from oracle.synth_np import make_panel
    return make_panel(60, 520, seed=9, nan_day=0.01, absent_month=0.01, nan_month=0.01,
                      cents=True)


def test_run_universe_is_the_composition_of_its_parts(engine):
    import csmom
    from oracle.synth_np import to_long
    dense = csmom.from_long(to_long(_daily_panel()))
    P, ms = _up(dense.P), _up(dense.month_start.astype(np.int64))
    N = dense.P.shape[1]
    rng = np.random.default_rng(3)
    bp = (rng.random(N) < 0.5).astype(np.uint8) * 200
    shares = np.round(rng.lognormal(3.0, 1.5, N))
    base = engine.run_neutral(P, ms, _up(np.zeros(N, dtype=np.int16)), 1, J=6, skip=1, n_bins=5)
    CAP = base.PM * _up(shares)
    floor = float(np.nanquantile(base.PM.cpu().numpy(), 0.15))
    out = engine.run_universe(P, ms, _up(bp), min_price=floor, CAP=CAP, min_size_pct=20, J=6,
                              skip=1, n_bins=5)
    E, NE, _ = engine.breakpoints(CAP, _up(bp), 5)
    CAPMIN = E[:, 1].contiguous()
    MS, KEPT = engine.screen(base.M, base.PM, floor, CAP, CAPMIN, with_kept=True)
    L, EW, CNT, NV, NVB, EDGES, NE = engine.deciles_bp(MS, base.NR, _up(bp), 5, with_nv=True,
                                                       with_edges=True)
    LS = engine.long_short(EW, CNT)
    for a, b in ((out.M, MS), (out.KEPT, KEPT), (out.L, L), (out.EW, EW), (out.CNT, CNT),
                 (out.NV, NV), (out.NVB, NVB), (out.EDGES, EDGES), (out.NE, NE), (out.LS, LS),
                 (out.NR, base.NR), (out.PM, base.PM)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    kept, sig = KEPT.sum().item(), (~torch.isnan(base.M)).sum().item()
    assert 0.3 * sig < kept < 0.95 * sig and (~torch.isnan(LS)).sum().item() >= 8
    assert torch.equal(KEPT, NV)
    # and against the ref on the device's own panels
    ms_ref, kept_ref = BR.screen(base.M.cpu().numpy(), base.PM.cpu().numpy(), floor,
                                 CAP.cpu().numpy(), CAPMIN.cpu().numpy())
    assert bits_equal(MS.cpu().numpy(), ms_ref) and np.array_equal(KEPT.cpu().numpy(), kept_ref)
    ref = BR.deciles_bp(ms_ref, base.NR.cpu().numpy(), bp, 5)
    assert np.array_equal(L.cpu().numpy(), ref["L"]) and half_labelled(ref, ms_ref)
    _close(EW, ref["EW"], "EW")
    with pytest.raises(ValueError):
        engine.run_universe(P, ms, _up(bp), CAP=CAP, min_size_pct=30)
    with pytest.raises(ValueError):
        engine.run_universe(P, ms, _up(bp), CAP=CAP)


def test_run_universe_without_screens_is_the_plain_sort(engine):
    import csmom
    from oracle.synth_np import to_long
    dense = csmom.from_long(to_long(_daily_panel()))
    P, ms = _up(dense.P), _up(dense.month_start.astype(np.int64))
    N = dense.P.shape[1]
    plain = engine.run_neutral(P, ms, _up(np.zeros(N, dtype=np.int16)), 1, J=6, skip=1, n_bins=5)
    out = engine.run_universe(P, ms, J=6, skip=1, n_bins=5)
    assert (plain.L >= 0).float().mean().item() > 0.3
    assert torch.equal(out.L, plain.L) and torch.equal(out.CNT, plain.CNT)
    assert torch.equal(out.M.view(torch.int64), plain.M.view(torch.int64)) and out.KEPT is None
    _close(out.EW, plain.EW.cpu().numpy(), "EW")
    _close(out.LS, plain.LS.cpu().numpy(), "LS")


def test_universe_momentum_api(engine):
    import csmom
    from oracle.synth_np import to_long
    df = to_long(_daily_panel())
    dense = csmom.from_long(df)
    tickers = list(dense.tickers)
    nyse = tickers[::2]
    shares = {tk: 1000.0 * (1 + (7 * i) % 13) for i, tk in enumerate(tickers)}
    res = csmom.universe_momentum(df, nyse, min_price=80.0, shares=shares, min_size_pct=20, J=6,
                                  skip=1, n_bins=5, device=0)
    P, ms = _up(dense.P), _up(dense.month_start.astype(np.int64))
    PM, _ = engine.month_end(P, ms)
    CAP = PM * _up(csmom.shares_row(tickers, shares))
    out = engine.run_universe(P, ms, _up(csmom.breakpoint_mask(tickers, nyse)), min_price=80.0,
                              CAP=CAP, min_size_pct=20, J=6, skip=1, n_bins=5)
    ls = out.LS.cpu().numpy()
    assert (~np.isnan(ls)).sum() >= 8
    assert bits_equal(res.long_short.to_numpy(), ls[~np.isnan(ls)])
    assert bits_equal(res.deciles.to_numpy(), out.EW.cpu().numpy())
    assert bits_equal(res.breakpoints.to_numpy(), out.EDGES.cpu().numpy())
    assert res.counts["ranked"].tolist() == out.NV.tolist()
    assert res.counts["breakpoint"].tolist() == out.NVB.tolist()
    assert res.counts["kept"].tolist() == out.KEPT.tolist()
    assert 0 < out.KEPT.sum().item() < (~torch.isnan(engine.run_universe(
        P, ms, J=6, skip=1, n_bins=5).M)).sum().item()
    assert np.isfinite(res.t_nw) and np.isfinite(res.mean)
    k3 = csmom.universe_momentum(df, nyse, J=6, skip=1, n_bins=5, K=3, device=0)
    pf = engine.portfolio(engine.run_universe(P, ms, _up(csmom.breakpoint_mask(tickers, nyse)),
                                              J=6, skip=1, n_bins=5).L, out.NR, 5, K=3,
                          with_costs=False)
    assert bits_equal(k3.deciles.to_numpy(), pf.PR[:, 0, :].cpu().numpy())


def _raw(engine, M, NR, BP, bp_ld, T_m, N, nb, L, EDGES, q=True):
    qt = O.quantile_table(max(nb, 1))
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = engine.lib.csm_deciles_bp(engine.ctx, p(M), p(NR), p(BP), bp_ld, T_m, N, nb,
                                   qt.ctypes.data_as(ctypes.c_void_p) if q else None, p(L), None,
                                   None, None, None, p(EDGES), None)
    return st, engine.lib.csm_last_error(engine.ctx).decode()


def test_argument_checks(engine):
    T_m, N = 2, 64
    M, NR, BP = make_case(T_m, N, True, seed=1)
    Md, NRd, Bd = _up(M), _up(NR), _up(BP)
    L = torch.empty((T_m, N), dtype=torch.int8, device=Md.device)
    E = torch.empty((T_m, 11), dtype=torch.float64, device=Md.device)
    ok = (Md, None, Bd, 0, T_m, N, 10, L, E)

    def bad(i, v, word, **kw):
        a = list(ok)
        a[i] = v
        st, msg = _raw(engine, *a, **kw)
        assert st == -1 and word in msg, (i, v, st, msg)

    assert _raw(engine, *ok)[0] == 0
    a = list(ok)
    a[8] = None
    assert _raw(engine, *a)[0] == 0                          # L alone
    a = list(ok)
    a[7] = None
    assert _raw(engine, *a)[0] == 0                          # EDGES alone
    a[8] = None
    st, msg = _raw(engine, *a)
    assert st == -1 and "both NULL" in msg
    bad(0, None, "NULL")
    bad(2, None, "NULL")
    bad(0, Md, "NULL", q=False)
    bad(3, 7, "bp_ld")
    bad(3, -N, "bp_ld")
    bad(6, 0, "n_bins")
    bad(6, 21, "n_bins")
    bad(4, 0, "bad arguments")
    bad(5, 0, "bad arguments")
    bad(5, 2 ** 31, "bad arguments")
    a = list(ok)
    a[1], a[6] = NRd, 7                                      # csm_deciles refuses 7 bins with NR
    st, msg = _raw(engine, *a)
    assert st == -1 and "n_bins=7" in msg
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    lib = engine.lib
    MS = torch.empty_like(Md)
    CM = torch.zeros(T_m, dtype=torch.float64, device=Md.device)
    assert lib.csm_screen(engine.ctx, p(Md), None, 0.0, None, None, T_m, N, p(MS), None) == 0
    for args, word in (((None, None, 0.0, None, None, T_m, N, p(MS), None), "NULL"),
                       ((p(Md), None, 0.0, None, None, T_m, N, None, None), "NULL"),
                       ((p(Md), None, 0.0, p(NRd), None, T_m, N, p(MS), None), "CAPMIN"),
                       ((p(Md), None, 0.0, None, p(CM), 0, N, p(MS), None), "bad arguments"),
                       ((p(Md), None, 0.0, None, None, T_m, 0, p(MS), None), "bad arguments")):
        st = lib.csm_screen(engine.ctx, *args)
        assert st == -1 and word in lib.csm_last_error(engine.ctx).decode(), args
    with pytest.raises(TypeError):
        engine.deciles_bp(Md, None, Bd.to(torch.int32), 10)
    with pytest.raises(ValueError):
        engine.screen(Md, PM=Md)
    with pytest.raises(ValueError):
        engine.screen(Md, CAP=Md)
