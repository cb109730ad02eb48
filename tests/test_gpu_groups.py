"""GPU: csm_group_deciles / csm_group_stats and what is built on them (rules N1..N6 in DESIGN.md
7) against the NumPy restatement in tests/group_ref.py, which the CPU tests pin to the reference.

Inputs are synthetic signals made directly: normal draws rounded to cents (ties), 20 % NaN, 1 %
ABSENT, 5 % ids out of range (negative and >= n_groups), next returns with 10 % NaN.

Bars.  L, CNT, CNTG, NV, NVG and GCNT are exact.  EW, EWG and the long-short are within the
project's 1e-10 relative of the ref's Kahan sums in asset order.  Two calls give the same bits, and
so do the tuned and the untuned small-segment cap.

GMEAN is a sum whose order the rule leaves to the kernel.  With u = 2^-53 and g(k) = k u / (1 - k u),
any order of an n-term sum errs by at most g(n - 1) sum |x|; the quotient by n and the ref's own
fsum / n each round once.  So
    |GMEAN - fsum / n| <= g(n - 1) sum |x| / n + u (|GMEAN| + |fsum / n|).
GSD is compared with the ref evaluated at the DEVICE's GMEAN, so both sides sum the same
non-negative terms fl(fl(x - GMEAN)^2): the sums differ by at most g(n - 1) relative, plus one
rounding of fsum; each side then rounds one quotient (2 u) and, after the square root halves the
relative error, one root (2 u):
    |GSD - ref| <= (g(n - 1) / 2 + 4 u) ref
(4 u where 3.5 u is the first-order count, for the second-order terms).  SA, SZ and SB are single
correctly rounded operations on the device's own GMEAN / GSD: bit for bit.  Measured on an MI355X:
GMEAN at most 0.015 of its bound, GSD at most 0.089 (printed by the test).

Every parametrised case asserts that at least half of its cells carry a label >= 0 in the ref, so
nothing passes on -1s; the named degenerate cases assert exactly their degenerate output.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import group_ref as GR
from conftest import bits_equal, max_rel
from oracle import csmom_oracle as O
from oracle import portfolio_oracle as PO

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
REL = 1e-10
_CACHE = {}


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def make_case(T_m, N, G, static, seed, weights=None, nan=0.2, bad=0.05):
    """S, NR [T_m][N], GID [N] or [T_m][N] int16.  weights: the groups' shares of the assets."""
    rng = np.random.default_rng(seed)
    S = np.round(rng.normal(0.0, 0.1, (T_m, N)), 2)
    S[rng.random((T_m, N)) < nan] = np.nan
    if nan > 0:
        S[rng.random((T_m, N)) < 0.01] = O.absent_scalar()
    NR = rng.normal(0.01, 0.08, (T_m, N))
    NR[rng.random((T_m, N)) < 0.1] = np.nan
    shape = (N,) if static else (T_m, N)
    p = None if weights is None else np.asarray(weights, dtype=np.float64) / np.sum(weights)
    gid = rng.choice(G, size=shape, p=p).astype(np.int16)
    out = rng.random(shape) < bad
    gid[out] = np.where(rng.random(shape) < 0.5, -1 - rng.integers(0, 3, shape),
                        G + rng.integers(0, 3, shape))[out].astype(np.int16)
    return S, NR, gid


def ref_case(key, S, NR, gid, G, nb, min_group):
    if key not in _CACHE:
        L = GR.group_labels(S, gid, G, nb, min_group)
        mem = GR.membership(S, gid, G)
        _CACHE[key] = dict(L=L, mem=mem, **GR.group_means(L, NR, mem, G, nb))
    return _CACHE[key]


def _close(got, ref, what):
    g = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert np.array_equal(np.isnan(g), np.isnan(ref)), what
    m = ~np.isnan(ref)
    scale = np.maximum(np.abs(ref[m]), 1e-12)
    assert (np.abs(g[m] - ref[m]) <= REL * scale + 1e-15).all(), (what, max_rel(g, ref))


def check_deciles(engine, S, NR, gid, G, nb, min_group, ref):
    Sd, NRd, Gd = _up(S), _up(NR), _up(gid)
    L, EW, CNT, NV, EWG, CNTG, NVG = engine.deciles_within(Sd, NRd, Gd, G, nb, min_group,
                                                           with_groups=True, with_nv=True)
    LS = engine.long_short(EW, CNT)
    torch.cuda.synchronize()
    assert np.array_equal(L.cpu().numpy(), ref["L"])
    assert np.array_equal(CNT.cpu().numpy(), ref["CNT"])
    assert np.array_equal(CNTG.cpu().numpy(), ref["CNTG"])
    assert np.array_equal(NV.cpu().numpy(), ref["NV"])
    assert np.array_equal(NVG.cpu().numpy(), ref["NVG"])
    _close(EW, ref["EW"], "EW")
    _close(EWG, ref["EWG"], "EWG")
    _close(LS, ref["LS"], "LS")
    again = engine.deciles_within(Sd, NRd, Gd, G, nb, min_group, with_groups=True, with_nv=True)
    for a, b in zip((L, EW, CNT, NV, EWG, CNTG, NVG), again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    L0, _, _ = engine.deciles_within(Sd, None, Gd, G, nb, min_group)   # labels only
    assert torch.equal(L0, L)
    return L, EW, CNT, EWG, CNTG


# (T_m, N, n_groups, static ids, n_bins, min_group, the groups' shares of the assets)
SKEW11 = [40, 20, 10, 8, 6, 5, 4, 3, 2, 1.5, 0.5]
CASES = [
    (3, 63, 1, True, 10, 1, None),
    (3, 64, 2, False, 5, 1, None),
    (1, 65, 2, True, 3, 1, [0.9, 0.1]),
    (3, 257, 11, False, 10, 1, None),
    (24, 1000, 11, True, 10, 10, SKEW11),
    (3, 1000, 49, False, 2, 1, None),
    (3, 1000, 11, False, 3, 3, SKEW11),
    (3, 4099, 49, True, 20, 50, None),
    (3, 4099, 256, False, 5, 5, None),
    (1, 4099, 2, True, 10, 50, [0.999, 0.001]),
    (3, 4099, 11, False, 20, 20, [0] + [1] * 10),       # group 0 is empty
]


@pytest.mark.parametrize("T_m,N,G,static,nb,min_group,weights", CASES)
def test_group_deciles_vs_ref(engine, T_m, N, G, static, nb, min_group, weights):
    key = (T_m, N, G, static, nb, min_group)
    S, NR, gid = make_case(T_m, N, G, static, seed=N + G, weights=weights)
    ref = ref_case(key, S, NR, gid, G, nb, min_group)
    assert (ref["L"] >= 0).mean() >= 0.5
    check_deciles(engine, S, NR, gid, G, nb, min_group, ref)


def test_wide_rows_against_ref_and_the_loop_over_groups(engine):
    """20,000 x 6, 11 groups, group 0 with 40 % of the assets: its 6,000 or so members are past the LDS
    cap.  L also equals the loop over groups on Engine.deciles with masked signals bit for bit."""
    T_m, N, G, nb = 6, 20000, 11, 10
    S, NR, gid = make_case(T_m, N, G, True, seed=7, weights=SKEW11)
    ref = ref_case("wide", S, NR, gid, G, nb, 1)
    assert (ref["L"] >= 0).mean() >= 0.5 and ref["NVG"][:, 0].min() > 4096
    L, *_ = check_deciles(engine, S, NR, gid, G, nb, 1, ref)
    Sd = _up(S)
    loop = torch.full((T_m, N), -1, dtype=torch.int8, device=Sd.device)
    gd = _up(gid).expand(T_m, N)
    nan = torch.full_like(Sd, float("nan"))
    for g in range(G):
        Lg, _, _, _ = engine.deciles(torch.where(gd == g, Sd, nan), None, nb)
        loop = torch.where(gd == g, Lg, loop)
    assert torch.equal(loop, L)


@pytest.mark.parametrize("N", [1000, 20000])
def test_one_group_equals_plain_deciles(engine, N):
    S, NR, _ = make_case(3, N, 1, True, seed=N)
    gid = np.zeros(N, dtype=np.int16)
    Sd, NRd = _up(S), _up(NR)
    L, EW, CNT, NV = engine.deciles_within(Sd, NRd, _up(gid), 1, 10, with_nv=True)
    L0, EW0, CNT0, NV0 = engine.deciles(Sd, NRd, 10, with_nv=True)
    assert (L0 >= 0).float().mean().item() >= 0.5
    assert torch.equal(L, L0) and torch.equal(CNT, CNT0) and torch.equal(NV, NV0)
    _close(EW, EW0.cpu().numpy(), "EW")


def test_small_cap_knob_moves_segments_not_results(engine):
    """gdec_small_cap = 64: segments of 300 and 571 values take the tiled kernel (tiles of 128),
    64 stays in LDS, 65 does not.  Same labels, counts and bits of the means as untuned."""
    T_m, N, G, nb = 3, 1000, 4, 10
    S, NR, _ = make_case(T_m, N, G, True, seed=3, nan=0.0, bad=0.0)
    gid = np.repeat(np.arange(4, dtype=np.int16), [300, 64, 65, 571])
    gid = gid[np.random.default_rng(1).permutation(N)]
    ref = ref_case("knob", S, NR, gid, G, nb, 1)
    assert ref["NVG"][0].tolist() == [300, 64, 65, 571] and (ref["L"] >= 0).mean() >= 0.5
    base = check_deciles(engine, S, NR, gid, G, nb, 1, ref)
    assert engine.lib.csm_tune(b"gdec_small_cap", 64) == 0
    try:
        tuned = check_deciles(engine, S, NR, gid, G, nb, 1, ref)
    finally:
        assert engine.lib.csm_tune(b"gdec_small_cap", 4096) == 0
    for a, b in zip(base, tuned):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert engine.lib.csm_tune(b"gdec_small_cap", 0) != 0
    assert engine.lib.csm_tune(b"gdec_small_cap", 4097) != 0


def test_degenerate_cases(engine):
    T_m, N, nb = 3, 257, 10
    S, NR, gid = make_case(T_m, N, 4, False, seed=11)
    Sd, NRd = _up(S), _up(NR)
    nv = torch.zeros(T_m, dtype=torch.int32, device=Sd.device)
    # every id invalid
    bad = np.where(gid % 2 == 0, -1, 4).astype(np.int16)
    L, EW, CNT, NV, EWG, CNTG, NVG = engine.deciles_within(Sd, NRd, _up(bad), 4, nb,
                                                           with_groups=True, with_nv=True)
    assert (L == -1).all() and (CNT == 0).all() and (CNTG == 0).all() and (NVG == 0).all()
    assert torch.equal(NV, nv) and torch.isnan(EW).all() and torch.isnan(EWG).all()
    assert torch.isnan(engine.long_short(EW, CNT)).all()
    # every group under min_group
    mem = GR.membership(S, gid, 4)
    L, EW, CNT, NV = engine.deciles_within(Sd, NRd, _up(gid), 4, nb, min_group=N, with_nv=True)
    assert (L == -1).all() and (CNT == 0).all() and torch.isnan(EW).all()
    assert np.array_equal(NV.cpu().numpy(), (mem >= 0).sum(axis=1))
    # an all-equal group among ranked ones; a one-asset row
    S2 = S.copy()
    S2[:, gid[0] == 1] = 0.25
    g2 = np.ascontiguousarray(gid[0])
    ref = GR.group_labels(S2, g2, 4, nb)
    L, _, _ = engine.deciles_within(_up(S2), None, _up(g2), 4, nb)
    assert np.array_equal(L.cpu().numpy(), ref)
    assert (ref[:, g2 == 1] == -1).all() and (ref >= 0).mean() > 0.4
    one = engine.deciles_within(_up(np.array([[0.5], [np.nan]])), _up(np.array([[0.1], [0.2]])),
                                _up(np.zeros(1, dtype=np.int16)), 1, nb, with_nv=True)
    assert one[0].tolist() == [[-1], [-1]] and one[2].sum().item() == 0
    assert one[3].tolist() == [1, 0]


@pytest.mark.parametrize("T_m,N,G,static", [(3, 65, 2, True), (3, 1000, 11, False),
                                            (2, 4099, 49, True), (2, 20000, 3, True)])
def test_group_stats(engine, T_m, N, G, static):
    S, _, gid = make_case(T_m, N, G, static, seed=N + 1,
                          weights=[0.9, 0.08, 0.02] if G == 3 else None)
    GCNT, GMEAN, _ = GR.group_stats(S, gid, G)
    o = engine.group_stats(_up(S), _up(gid), G)
    torch.cuda.synchronize()
    assert np.array_equal(o.GCNT.cpu().numpy(), GCNT) and (GCNT > 0).mean() > 0.9
    gm, gsd = o.GMEAN.cpu().numpy(), o.GSD.cpu().numpy()
    mem = GR.membership(S, gid, G)
    worst_m = worst_s = 0.0
    for t in range(T_m):
        for g in range(G):
            v = S[t, mem[t] == g]
            n = len(v)
            if n == 0:
                assert np.isnan(gm[t, g]) and np.isnan(gsd[t, g])
                continue
            gam = (n - 1) * U / (1.0 - (n - 1) * U)
            bound = gam * float(np.abs(v).sum()) / n + U * (abs(gm[t, g]) + abs(GMEAN[t, g]))
            err = abs(gm[t, g] - GMEAN[t, g])
            assert err <= bound, (t, g, err, bound)
            worst_m = max(worst_m, err / bound if bound > 0 else 0.0)
            if n < 2:
                assert np.isnan(gsd[t, g])
                continue
            d = v - gm[t, g]
            want = math.sqrt(math.fsum(d * d) / (n - 1))
            sb = (gam / 2 + 4 * U) * want
            assert abs(gsd[t, g] - want) <= sb, (t, g, gsd[t, g], want)
            worst_s = max(worst_s, abs(gsd[t, g] - want) / sb if sb > 0 else 0.0)
    print(f"group_stats N={N} G={G}: worst GMEAN error / bound {worst_m:.3f}, GSD {worst_s:.3f}")
    SA, SZ, SB = GR.adjusted(S, gid, G, gm, gsd)
    assert bits_equal(o.SA.cpu().numpy(), SA)
    assert bits_equal(o.SZ.cpu().numpy(), SZ)
    assert bits_equal(o.SB.cpu().numpy(), SB)
    assert (~np.isnan(SZ)).mean() > 0.5
    again = engine.group_stats(_up(S), _up(gid), G)
    for k in engine.GROUP_OUTPUTS:
        assert torch.equal(getattr(o, k).view(torch.uint8), getattr(again, k).view(torch.uint8))
    part = engine.group_stats(_up(S), _up(gid), G, outputs=("SZ",))
    assert part.GMEAN is None and torch.equal(part.SZ.view(torch.int64), o.SZ.view(torch.int64))


def test_portfolio_on_neutral_labels(engine):
    T_m, N, G = 24, 1000, 11
    S, NR, gid = make_case(T_m, N, G, True, seed=N + G, weights=SKEW11)
    ref = ref_case((T_m, N, G, True, 10, 10), S, NR, gid, G, 10, 10)
    L, _, _ = engine.deciles_within(_up(S), None, _up(gid), G, 10, 10)
    out = engine.portfolio(L, _up(NR), 10, K=3, with_costs=False)
    want = PO.portfolio(ref["L"], NR, 10, K=3)
    _close(out.PR, want["PR"], "PR")
    _close(out.LS, want["LS"], "LS")


def test_dependent_double_sort(engine):
    import csmom
    T_m, N = 24, 1000
    S1, NR, _ = make_case(T_m, N, 1, True, seed=21)
    S2, _, _ = make_case(T_m, N, 1, True, seed=22)
    r = csmom.dependent_double_sort(engine, _up(S1), _up(S2), _up(NR), n1=3, n2=10, K=1)
    L1 = O.assign_deciles(S1, 3)
    L2 = GR.group_labels(S2, L1.astype(np.int16), 3, 10)
    Lc = np.where((L1 >= 0) & (L2 >= 0), 10 * L1.astype(np.int64) + L2, -1).astype(np.int8)
    assert (Lc >= 0).mean() >= 0.5
    assert np.array_equal(r.Lm.cpu().numpy(), L1) and np.array_equal(r.Lv.cpu().numpy(), L2)
    assert np.array_equal(r.Lc.cpu().numpy(), Lc)
    want = PO.portfolio(Lc, NR, 30, K=1)["PR"][:, 0, :].reshape(T_m, 3, 10)
    _close(r.PR, want, "PR")
    _close(r.LS, want[:, :, 9] - want[:, :, 0], "LS")


def test_industry_momentum(engine):
    """Industries ranked on their mean momentum: group_stats' GMEAN of M and of NR into deciles
    with N = n_groups."""
    T_m, N, G = 12, 4099, 49
    S, NR, gid = make_case(T_m, N, G, True, seed=5)
    NRm = np.where(np.isnan(S), np.nan, NR)
    IM = engine.group_stats(_up(S), _up(gid), G, outputs=("GMEAN",)).GMEAN
    INR = engine.group_stats(_up(NRm), _up(gid), G, outputs=("GMEAN",)).GMEAN
    L, EW, CNT, _ = engine.deciles(IM, INR, 5)
    im, inr = IM.cpu().numpy(), INR.cpu().numpy()
    Lr = O.assign_deciles(im, 5)
    EWr, CNTr, _ = O.portfolio_ew(Lr, inr, 5)
    assert (Lr >= 0).mean() >= 0.5
    assert np.array_equal(L.cpu().numpy(), Lr) and np.array_equal(CNT.cpu().numpy(), CNTr)
    _close(EW, EWr, "EW")


def _raw(engine, S, NR, GID, g_ld, T_m, N, G, nb, min_group, L, q=True):
    qt = O.quantile_table(max(nb, 1))
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = engine.lib.csm_group_deciles(engine.ctx, p(S), p(NR), p(GID), g_ld, T_m, N, G, nb,
                                      qt.ctypes.data_as(ctypes.c_void_p) if q else None,
                                      min_group, p(L), None, None, None, None, None, None)
    return st, engine.lib.csm_last_error(engine.ctx).decode()


def test_argument_checks(engine):
    T_m, N = 2, 64
    S, NR, gid = make_case(T_m, N, 3, True, seed=1)
    Sd, NRd, Gd = _up(S), _up(NR), _up(gid)
    L = torch.empty((T_m, N), dtype=torch.int8, device=Sd.device)
    ok = (Sd, None, Gd, 0, T_m, N, 3, 10, 1, L)

    def bad(i, v, word, **kw):
        a = list(ok)
        a[i] = v
        st, msg = _raw(engine, *a, **kw)
        assert st == -1 and word in msg, (i, v, st, msg)

    assert _raw(engine, *ok)[0] == 0
    bad(6, 0, "n_groups")
    bad(6, 257, "n_groups")
    bad(3, 7, "g_ld")
    bad(8, 0, "min_group")
    bad(0, None, "bad arguments")
    bad(2, None, "bad arguments")
    bad(9, None, "NULL")
    bad(7, 0, "n_bins")
    bad(7, 21, "n_bins")
    bad(4, 0, "bad arguments")
    bad(5, 0, "bad arguments")
    a = list(ok)
    a[1], a[7] = NRd, 7      # csm_deciles refuses 7 bins with NR
    st, msg = _raw(engine, *a)
    assert st == -1 and "n_bins=7" in msg
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    lib = engine.lib
    for args, word in (((None, p(Gd), 0, T_m, N, 3), "bad arguments"),
                       ((p(Sd), None, 0, T_m, N, 3), "bad arguments"),
                       ((p(Sd), p(Gd), 0, T_m, N, 300), "n_groups"),
                       ((p(Sd), p(Gd), 5, T_m, N, 3), "g_ld"),
                       ((p(Sd), p(Gd), 0, 0, N, 3), "bad arguments")):
        st = lib.csm_group_stats(engine.ctx, *args, None, None, None, None, None, None)
        assert st == -1 and word in lib.csm_last_error(engine.ctx).decode()
    with pytest.raises(TypeError):
        engine.deciles_within(Sd, None, Gd.to(torch.int32), 3)


def test_neutral_momentum_api(engine):
    import csmom
    from oracle.synth_np import make_panel, to_long
    panel = make_panel(40, 520, seed=9, nan_day=0.01, absent_month=0.01, nan_month=0.01,
                       cents=True)
    df = to_long(panel)
    tickers = sorted(df["ticker"].unique())
    groups = {tk: ("A", "B", "C", None)[i % 4] for i, tk in enumerate(tickers)}
    res = csmom.neutral_momentum(df, groups, J=6, skip=1, n_bins=3, min_group=3, device=0)
    dense = csmom.from_long(df)
    gid, names = csmom.group_ids(dense.tickers, groups)
    assert names == ["A", "B", "C"] and res.groups == names
    out = engine.run_neutral(_up(dense.P), _up(dense.month_start.astype(np.int64)), _up(gid), 3,
                             J=6, skip=1, n_bins=3, min_group=3)
    ls = out.LS.cpu().numpy()
    assert (~np.isnan(ls)).sum() >= 8
    assert bits_equal(res.long_short.to_numpy(), ls[~np.isnan(ls)])
    assert bits_equal(res.deciles.to_numpy(), out.EW.cpu().numpy())
    assert res.group_long_short.shape == (dense.T_m, 3) and np.isfinite(res.t_nw)
    # the labels are the ref's on the device's own signal
    M = out.M.cpu().numpy()
    assert np.array_equal(out.L.cpu().numpy(), GR.group_labels(M, gid, 3, 3, 3))
    for adjust, field in (("demean", "SA"), ("zscore", "SZ")):
        adj = engine.run_neutral(_up(dense.P), _up(dense.month_start.astype(np.int64)), _up(gid),
                                 3, adjust=adjust, J=6, skip=1, n_bins=3)
        want = getattr(engine.group_stats(out.M, _up(gid), 3, outputs=(field,)), field)
        assert torch.equal(adj.M.view(torch.int64), want.view(torch.int64))
        assert torch.equal(adj.L, engine.deciles(want, None, 3)[0])
