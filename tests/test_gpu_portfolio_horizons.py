"""GPU: the portfolio accounting (csm_portfolio*, csm_cohort_sums*) beyond the benchmark's K set
and shapes, against oracle.portfolio_oracle.portfolio on the synthetic panels of
tests/portfolio_cases.py: holding periods on both sides of every kernel-selection threshold of
csrc/portfolio.hip (groups A, E), K sets longer than one accounting batch (B), histories shorter
than the holding period (C), rows narrower than a wave (D), the shared-return cohort passes on
both sides of the segment limit (F) and the argument limits (G).

Bar: 1e-10 relative with equal NaN patterns against the oracle (tests/test_gpu_portfolio.py's
_close); bit-equality wherever the code or a docstring promises it.
tests/test_portfolio_cases_cpu.py proves that each panel contains what its test relies on."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import portfolio_cases as PC
from conftest import bits_equal
from oracle import portfolio_oracle as PO
from test_gpu_portfolio import REL, _close, _with_cohort_mode

pytestmark = pytest.mark.gpu
FIELDS = ("PR", "LS", "TURN", "COST", "NET")
assert REL == PC.REL == 1e-10


def _up(x):
    return torch.from_numpy(np.array(x, order="C")).to("cuda:0")   # (a copy: the cases are read-only)


@lru_cache(maxsize=4)
def _dev(case):
    """The case's arrays on the device in the engine's layout [T_m][B * N]."""
    a = PC.arrays(case)
    flat = lambda x: None if x is None else _up(x.reshape(case.T_m, case.B * case.N))
    return {k: flat(v) for k, v in a.items()}


def _kw(case, d, impact):
    kw = dict(W=d["W"], B=case.B)
    if impact:
        kw.update(aum=PC.AUM, ADV=d["ADV"], SIG=d["SIG"])
    return kw


def _np(x):
    return x.cpu().numpy()


def _check(out, ref, what, fields=FIELDS, q=None):
    """Every field of a PortfolioOut (slot q of a stacked one) within REL of the oracle."""
    for f in fields:
        g = _np(getattr(out, f))
        _close(g if q is None else g[q], ref[f], (what, f))


def _same(a, b, what, fields=FIELDS):
    for f in fields:
        assert bits_equal(_np(getattr(a, f)), _np(getattr(b, f))), (what, f)


# ------------------------------------------------------------------------------ A
_A = PC.group_a()


@pytest.mark.parametrize("name,case,impact,mode", _A, ids=[g[0] for g in _A])
def test_k_thresholds_vs_oracle(engine, name, case, impact, mode):
    """Holding periods on both sides of TP_U, the bitmask general-row limit, OV_TRIP, TO_GEN_TB,
    AC_MAXKD, SEG_MAXKD and at TO_MAXK (T_m = K + 9, B = 2, N = 260: two turnover chunks), on
    panels with top-less, blank and NaN-return months and a panel without a top decile: all five
    outputs against the oracle, for equal weights without impact and value weights with impact
    (every cost model at K = 31, 32, 240; N = 259 / 258 and the forced cohort kernels at the K
    portfolio_cases names)."""
    d = _dev(case)
    run = lambda: engine.portfolio(d["L"], d["NR"], case.n_bins, K=case.K, **_kw(case, d, impact))
    out = run() if mode is None else _with_cohort_mode(engine, mode, run)
    _check(out, PC.oracle_ref(case, case.K, impact), name)


# ------------------------------------------------------------------------------ B
_B = PC.group_b()


@pytest.mark.parametrize("name,case,Ks,opts", _B, ids=[g[0] for g in _B])
def test_k_sets_longer_than_a_batch(engine, name, case, Ks, opts):
    """More holding periods than one accounting batch (TO_MAXQ = 4; the turnover partials, the
    long-short flag words and the general-row work list are reused per batch and every output is
    offset by the batch): slot q of the stacked outputs equals the single call of Ks[q] bit for
    bit (the invariant of test_portfolio_multi_shares_cohort_pass) and the oracle within REL.
    Legs-only accounting over the same sets: LS / TURN / COST / NET bit for bit the full path's
    and PR on the two legs, with and without a panel that needs the full rerun."""
    impact, costs = opts.get("impact", False), opts.get("with_costs", True)
    d = _dev(case)
    nb = case.n_bins
    kw = dict(_kw(case, d, impact), with_costs=costs)
    fields = FIELDS if costs else ("PR", "LS")
    _, stk = engine.portfolio_multi(d["L"], d["NR"], nb, Ks=Ks, return_stacked=True, **kw)
    if not costs:
        assert stk.TURN is None and stk.COST is None and stk.NET is None
    for q, K in enumerate(Ks):
        one = engine.portfolio(d["L"], d["NR"], nb, K=K, **kw)
        for f in fields:
            assert bits_equal(_np(getattr(stk, f))[q], _np(getattr(one, f))), (name, q, K, f)
        _check(stk, PC.oracle_ref(case, K, impact), (name, q, K), fields, q=q)
    if not opts.get("legs_only"):
        return
    flag = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    engine.portfolio_multi(d["L"], d["NR"], nb, Ks=Ks, legs_only=True, need_full=flag, **kw)
    assert int(flag.item()) == (1 if opts["need_full"] else 0)
    _, legs = engine.portfolio_multi(d["L"], d["NR"], nb, Ks=Ks, legs_only=True,
                                     return_stacked=True, **kw)
    _same(legs, stk, name, ("LS", "TURN", "COST", "NET"))
    a, b = _np(legs.PR), _np(stk.PR)
    for dec in (0, nb - 1):
        assert bits_equal(a[..., dec], b[..., dec]), (name, dec)
    if not opts["need_full"]:
        assert np.isnan(a[..., 1:nb - 1]).all()


def test_k_set_grouped_equals_side_by_side(engine):
    """The nine-entry K set in the group-major layout (G = 2 groups of Bg = 2 panels, value
    weights / ADV / SIG shared by the groups): bit for bit the side-by-side call (as
    test_grouped_equals_side_by_side), and that one within REL of the oracle at the longest and
    the shortest K."""
    case = PC.group_b_grouped()
    a = PC.arrays(case)
    G, Bg, T_m, N, Ks = 2, 2, case.T_m, case.N, PC.KS_NINE
    grp = lambda x: np.stack([x[:, g * Bg:(g + 1) * Bg].reshape(T_m, Bg * N) for g in range(G)])
    shared = lambda x: np.ascontiguousarray(x[:, :Bg].reshape(T_m, Bg * N))
    Lg, NRg = grp(a["L"]), grp(a["NR"])
    Wh, ADVh, SIGh = shared(a["W"]), shared(a["ADV"]), shared(a["SIG"])
    _, g = engine.portfolio_multi_grouped(_up(Lg), _up(NRg), 10, Ks=Ks, W=_up(Wh), Bg=Bg,
                                          aum=PC.AUM, ADV=_up(ADVh), SIG=_up(SIGh),
                                          return_stacked=True)
    tile = lambda x: np.tile(x, (1, G))
    _, p = engine.portfolio_multi(_up(a["L"].reshape(T_m, -1)), _up(a["NR"].reshape(T_m, -1)), 10,
                                  Ks=Ks, W=_up(tile(Wh)), B=G * Bg, aum=PC.AUM, ADV=_up(tile(ADVh)),
                                  SIG=_up(tile(SIGh)), return_stacked=True)
    _same(g, p, "grouped")
    t3 = lambda x: tile(x).reshape(T_m, G * Bg, N)
    for K in (max(Ks), min(Ks)):
        ref = PO.portfolio(a["L"], a["NR"], 10, K=K, W=t3(Wh), aum=PC.AUM, ADV=t3(ADVh), SIG=t3(SIGh))
        _check(p, ref, ("side by side", K), q=Ks.index(K))


# ------------------------------------------------------------------------------ C
_C = PC.group_c()


@pytest.mark.parametrize("name,case,impact", _C, ids=[g[0] for g in _C])
def test_history_shorter_than_the_holding_period(engine, name, case, impact):
    """T_m in {1, 2, K - 1, K, K + 1}: no month t - K exists (no steady row) up to T_m = K."""
    d = _dev(case)
    out = engine.portfolio(d["L"], d["NR"], case.n_bins, K=case.K, **_kw(case, d, impact))
    _check(out, PC.oracle_ref(case, case.K, impact), name)


# ------------------------------------------------------------------------------ D
_D = PC.group_d()


@pytest.mark.parametrize("legs", [False, True])
@pytest.mark.parametrize("name,case", _D, ids=[g[0] for g in _D])
def test_narrow_rows(engine, name, case, legs):
    """Rows of 1 .. 65 assets (K = 3, T_m = 12, B = 3; equal weights, and value weights with
    impact costs): most deciles are empty, PR is mostly NaN and the long-short takes the
    fallback rule.  Legs-only accounting: LS / TURN / COST / NET and PR on the legs."""
    d = _dev(case)
    nb, impact = case.n_bins, case.vw
    ref = PC.oracle_ref(case, case.K, impact)
    kw = _kw(case, d, impact)
    if not legs:
        _check(engine.portfolio(d["L"], d["NR"], nb, K=case.K, **kw), ref, name)
        return
    out = engine.portfolio_multi(d["L"], d["NR"], nb, Ks=(case.K,), legs_only=True, **kw)[case.K]
    _check(out, ref, name, ("LS", "TURN", "COST", "NET"))
    pr = _np(out.PR)
    for dec in (0, nb - 1):
        _close(pr[..., dec], ref["PR"][..., dec], (name, "PR", dec))


# ------------------------------------------------------------------------------ E
_E = PC.group_e()


@pytest.mark.parametrize("name,case", _E, ids=[g[0] for g in _E])
def test_batched_value_weights_and_impact_vs_oracle(engine, name, case):
    """B = 3 and 16 panels with value weights (1 % NaN, 1 % negative, one month without a valid
    weight) and square-root impact costs (NaN volatilities, zero ADV cells)."""
    d = _dev(case)
    out = engine.portfolio(d["L"], d["NR"], case.n_bins, K=case.K, **_kw(case, d, True))
    _check(out, PC.oracle_ref(case, case.K, True), name)


# ------------------------------------------------------------------------------ F
def _shared_pass(engine, cases, Ks, legs):
    """portfolio_multi_js and portfolio_multi_js_grouped of the cases' label panels over their
    one next-return panel: every J bit for bit portfolio_multi's (their docstrings' promise)
    and within REL of the oracle."""
    c0, nJ = cases[0], len(cases)
    T_m, B, N, nb, Kmax = c0.T_m, c0.B, c0.N, c0.n_bins, max(Ks)
    assert engine.portfolio_plan(T_m, B, N, nb, Kmax)[0] == 1
    assert engine.portfolio_plan(T_m, B, N, nb, Kmax) == engine.portfolio_plan(T_m, nJ * B, N, nb, Kmax)
    NR = _dev(c0)["NR"]
    Ls = [_up(PC.arrays(c)["L"].reshape(T_m, B * N)) for c in cases]
    js = engine.portfolio_multi_js(Ls, NR, nb, Ks=Ks, B=B, legs_only=legs)
    _, jg = engine.portfolio_multi_js_grouped(torch.stack(Ls), NR, nb, Ks=Ks, B=B, legs_only=legs,
                                              return_stacked=True)
    for q, c in enumerate(cases):
        _, ref = engine.portfolio_multi(Ls[q], NR, nb, Ks=Ks, B=B, legs_only=legs,
                                        return_stacked=True)
        _same(js[q][1], ref, ("js", q))
        for f in FIELDS:
            assert bits_equal(_np(getattr(jg, f))[:, :, q * B:(q + 1) * B], _np(getattr(ref, f))), ("grouped", q, f)
        for i, K in enumerate(Ks):
            _check(ref, PC.oracle_ref(c, K, False), (q, K),
                   ("LS", "TURN", "COST", "NET") if legs else FIELDS, q=i)


@pytest.mark.parametrize("Ks", PC.F1_KS, ids=str)
def test_shared_return_pass_full_accounting(engine, Ks):
    """Four label panels, full accounting, B = 8, N = 64, T_m = 140 (one cohort chunk):
    Ks = (3, 11) takes the shared segment pass (4 * 11 * 11 <= SEG_MAXKD), (3, 12) the per-J
    passes."""
    _shared_pass(engine, PC.group_f1(Ks), Ks, False)


def test_shared_return_pass_legs_beyond_the_segment_limit(engine):
    """Legs-only at Kmax = 60, n_bins = 10: 60 * 11 > SEG_MAXKD, so portfolio_multi sums through
    the register kernel; two look-backs (2 * 60 * 4 <= SEG_MAXKD) must do the same to keep the
    promised bits."""
    _shared_pass(engine, PC.group_f2(), PC.F2_KS, True)


@pytest.mark.parametrize("Ks", PC.F3_KS, ids=str)
def test_shared_return_pass_legs_at_the_lds_bound(engine, Ks):
    """Legs-only, four look-backs: Kmax = 32 fills the shared pass's offset table
    (4 * 32 * 4 = SEG_MAXKD), 33 takes the per-J passes."""
    _shared_pass(engine, PC.group_f3(Ks), Ks, True)


@pytest.mark.parametrize("nb", [10, 30, 2])
def test_chunk_plan_follows_the_segment_limit(engine, nb):
    """The cohort chunk plan changes where the segment path ends, K * (n_bins + 1) = SEG_MAXKD:
    224 planned rows of 2600 assets get the segment path's ceil(1024 / 224) = 5 working chunks
    up to the limit and every ceil(2600 / PF_CHUNK_MIN) = 11 chunks past it; the turnover chunks
    do not depend on K."""
    K = PC.SEG_MAXKD // (nb + 1)
    assert K in PC.k_lists()[nb] and K + 1 in PC.k_lists()[nb]
    below, above = engine.portfolio_plan(56, 4, 2600, nb, K), engine.portfolio_plan(56, 4, 2600, nb, K + 1)
    assert below[0] == 5 and above[0] == -(-2600 // PC.PF_CHUNK_MIN) == 11
    assert below[1] == above[1] == engine.portfolio_plan(56, 1, 2600, nb, 1)[1]


# ------------------------------------------------------------------------------ G
def test_holding_period_limits(engine):
    """K = TO_MAXK + 1 is refused by the single and the multi entry (K = TO_MAXK runs in group
    A); the workspace of the largest accepted call has a size."""
    import csmom
    case = next(c for n, c, _ in PC.group_c() if n == "K6-T7-N260-ew")
    d = _dev(case)
    with pytest.raises(csmom.CsmError):
        engine.portfolio(d["L"], d["NR"], 10, K=PC.TO_MAXK + 1, B=case.B)
    with pytest.raises(csmom.CsmError):
        engine.portfolio_multi(d["L"], d["NR"], 10, Ks=(3, PC.TO_MAXK + 1), B=case.B)
    assert int(engine.lib.csm_portfolio_workspace(PC.TO_MAXK + 9, 2, 260, 30, PC.TO_MAXK)) > 0
    out = engine.portfolio(d["L"], d["NR"], 10, K=case.K, B=case.B)
    _check(out, PC.oracle_ref(case, case.K, False), "after the refused calls")
