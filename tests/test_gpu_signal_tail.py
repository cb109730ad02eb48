"""GPU parity of the tail-first fused signal (k_signal_tail, the "signal_tail" knob): each month's
last day row, then a walk back only for the cells whose last row holds no price -- a cell per
lane.  "signal_tail" 1 always takes it; so does 2 below 92,160 assets; from there on 2 launches
both kernels, each samples the panel's last day rows, and it runs where at most one sampled cell
in eight holds no price, the streaming kernel elsewhere (the one not chosen returns at once).  PM, ret_1m, mom_J, next_ret and the
fixed-map ids must be

  (i)  the CPU oracle's (oracle.csmom_oracle.month_end + momentum_scan) as raw 64-bit words
       (ABSENT and the quiet NaN are different words);
  (ii) the streaming kernel's ("signal_tail" 0) as raw 64-bit words, NaN words and ids included.

The panels are the smallest that reach every branch of the kernel: a full 512-asset block plus a
partial one (N = 640) and a single partial wave (N = 132); a calendar with a 23-day, a 1-day and a
zero-length month cut to 1, 9 (one batch of 8 plus one) and 29 months; every kind of gap in both
parities of the column and at the edges of the 64-asset waves; a month in which a whole wave
walks and a batch whose list of cells is full; half the cells absent (lists of hundreds of
cells) and 2 % of them, also at the narrowest width that is probed (92,160 assets, three months),
where the probe's choice is the streaming kernel for the one and the tail-first kernel for the
other; and a row-slice view between finite poison rows, where a read outside the slice would
change a bit and not fault."""
import functools

import numpy as np
import pytest
import torch

from conftest import bits_equal, load_golden

pytestmark = pytest.mark.gpu

NPAT = 11          # column patterns of _panel (odd: every pattern lands on both lanes of a pair)
FULL_WAVE_MONTH = 10            # every cell of one wave walks in this month
FULL_BATCH = range(16, 24)      # ... and in every month of this batch (the list at capacity)


def _up(x, dev="cuda:0"):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _calendar(T_m):
    """The first T_m months of a 29-month calendar (about 620 days): month 3 has 23 days,
    month 5 one day, month 7 none."""
    lens = [21, 22, 20, 23, 19, 1, 22, 0, 21, 20, 22, 23, 21, 20, 22, 21, 23, 20, 19, 22, 21, 22,
            20, 23, 21, 22, 20, 21, 18]
    return np.concatenate([[0], np.cumsum(lens[:T_m])]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _panel(N, T_m=29, dense_gaps=False, sparse_gaps=False):
    """(P, month_start) with the gap patterns of the module docstring; the CPU side of the cases
    (every k of "last k days NaN", a full wave, a full list) is asserted here, before any launch."""
    from oracle.csmom_oracle import ABSENT_BITS
    ms = _calendar(T_m)
    T_d = int(ms[-1])
    rng = np.random.default_rng(1000 + N + T_m)
    P = 100.0 * np.exp(np.cumsum(rng.normal(0.0, 0.01, (T_d, N)), axis=0))
    P = np.round(P, 2)
    ABS = np.array([ABSENT_BITS], dtype=np.uint64).view(np.float64)[0]
    if dense_gaps or sparse_gaps:   # half / 2 % of the (asset, month) cells absent, a missing day here and there
        gone = rng.random((T_m, N)) < (0.5 if dense_gaps else 0.02)
        P[rng.random((T_d, N)) < 0.02] = np.nan
        for m in range(T_m):
            P[ms[m]:ms[m + 1], gone[m]] = ABS
        return P, ms
    ks = set()
    for a in range(N):
        pat, j = (a + a // 64) % NPAT, a // NPAT
        if a % 64 in (0, 63):
            pat = 2   # the edge columns of every 64-asset wave walk in every month
        for m in range(T_m):
            d0, d1 = int(ms[m]), int(ms[m + 1])
            n = d1 - d0
            if n == 0:
                continue
            col = P[d0:d1, a]
            if pat == 1:                       # the last day missing
                col[-1] = np.nan
            elif pat == 2:                     # the last k days missing, every k < n
                k = (m + j) % n
                col[n - k:] = np.nan
                ks.add((n, k))
            elif pat == 3 and (m + j) % 3 == 0:    # a month of missing days only -> quiet NaN
                col[:] = np.nan
            elif pat == 4 and (m + j) % 3 == 1:    # an absent month -> ABSENT
                col[:] = ABS
            elif pat == 5 and (m + j) % 2 == 0:    # absent at the end, only missing days before
                col[:] = np.nan
                col[n - 1 - (m + j) % n:] = ABS
            elif pat == 6:                     # absent on the last day, a price mid-month
                col[n // 2 + 1:] = np.nan
                col[-1] = ABS
            elif pat == 7:                     # listed mid-month ml, delisted mid-month md
                ml, md = min(2 + j % 3, T_m - 1), T_m - 4 - j % 3
                if m <= ml:
                    col[:n // 2 if m == ml else n] = ABS
                if md > ml and m >= md:
                    col[n // 2 if m == md else 0:] = ABS
            elif pat == 8:                     # never listed
                col[:] = ABS
            elif pat == 9 and m in (0, T_m - 1):   # gaps in the first and the last month
                if (j + (m > 0)) % 3 == 0:
                    col[-2:] = np.nan
                elif (j + (m > 0)) % 3 == 1:
                    col[:] = ABS
                else:
                    col[1:] = np.nan
            elif pat == 10:                    # scattered missing days
                col[rng.random(n) < 0.05] = np.nan
    w0 = 128 if N >= 256 else 0                # the wave of the capacity cases
    w1 = min(w0 + 128, N)
    if T_m > FULL_WAVE_MONTH:
        P[ms[FULL_WAVE_MONTH + 1] - 1, w0:w1] = np.nan
    if T_m > FULL_BATCH[-1]:
        for m in FULL_BATCH:
            P[ms[m + 1] - 1, w0:w1] = np.nan
    if T_m == 29:   # the cases are there (CPU side)
        lens = np.diff(ms)
        for n in set(int(x) for x in lens if x > 0):
            if N >= 640:
                assert {k for (nn, k) in ks if nn == n} == set(range(n)), n
        gap = np.isnan(P[ms[1:][lens > 0] - 1])          # last rows without a price
        assert gap[:, w0:w1].all(axis=1).sum() >= 9
        assert all(int(lens[m]) > 0 for m in FULL_BATCH)
    return P, ms


@functools.lru_cache(maxsize=None)
def _oracle(key, J, skip):
    """(PM, R, M, NR) of the CPU oracle for a panel key, computed once and shared."""
    from oracle import csmom_oracle as O
    P, ms = _inputs(key)
    PM, _ = O.month_end(P, ms)
    R, M, NR, _ = O.momentum_scan(PM, J, skip)
    for x in (PM, R, M, NR):
        x.setflags(write=False)
    return PM, R, M, NR


@functools.lru_cache(maxsize=None)
def _inputs(key):
    kind = key[0]
    if kind == "golden":
        z = load_golden(key[1])
        N = z["P"].shape[1]
        P = np.ascontiguousarray(z["P"][:, :N - N % 2])
        return P, z["month_start"].astype(np.int64)
    if kind == "built":
        return _panel(key[1], key[2])
    if kind == "dense":
        return _panel(640, 29, dense_gaps=True)
    if kind == "sparse":
        return _panel(640, 29, sparse_gaps=True)
    if kind == "wide":   # the narrowest probed width, three months
        return _panel(92_160, 3, dense_gaps=key[1] == "dense", sparse_gaps=key[1] == "sparse")
    raise KeyError(key)


def _same_words(a, b, what):
    a, b = _u64(a), _u64(b)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(bad)} cells differ, first (month, asset) {bad[:8].tolist()}")


def _tune(engine, **kn):
    for k, v in kn.items():
        assert engine.lib.csm_tune(k.encode(), int(v)) == 0, k


def _launch(engine, P, ms, mmd, J, skip):
    if P.shape[1] % 4 == 0:
        return engine.signal_ids(P, ms, mmd, J, skip, with_pm=True, with_ret=True)
    return engine.signal(P, ms, mmd, J, skip, with_pm=True, with_ret=True) + (None,)


def _check(engine, key, J, skip, tail, P=None, mmd=None, **knobs):
    """One launch with "signal_tail" = tail against the oracle and against "signal_tail" = 0."""
    from test_gpu_pipeline import fixed_ids
    Ph, ms_h = _inputs(key)
    Pd = _up(Ph) if P is None else P
    ms = _up(ms_h)
    mmd = int(np.diff(ms_h).max()) if mmd is None else mmd
    try:
        _tune(engine, signal_tail=tail, **knobs)
        got = _launch(engine, Pd, ms, mmd, J, skip)
        _tune(engine, signal_tail=0)
        base = _launch(engine, Pd, ms, mmd, J, skip)
        torch.cuda.synchronize()
    finally:
        _tune(engine, signal_tail=2)
    ref = _oracle(key, J, skip)
    assert np.array_equal(_u64(got[0]), ref[0].view(np.uint64)), "PM differs from the oracle"
    for nm, g, r in zip(("R", "M", "NR"), got[1:4], ref[1:]):
        assert bits_equal(g.cpu().numpy(), r), f"{nm} differs from the oracle"
        assert np.array_equal(_u64(g), r.view(np.uint64)), f"{nm}: NaN words differ from the oracle's"
    for nm, g, b in zip(("PM", "R", "M", "NR"), got[:4], base[:4]):
        _same_words(g, b, f"{nm} against the streaming kernel")
    if got[4] is not None:
        ids = got[4].cpu().numpy().view(np.uint16)
        assert np.array_equal(ids, base[4].cpu().numpy().view(np.uint16)), "ids differ"
        assert np.array_equal(ids, fixed_ids(got[2].cpu().numpy()))


@pytest.mark.parametrize("tail", [1, 2])
@pytest.mark.parametrize("J,skip", [(12, 1), (3, 0)])
@pytest.mark.parametrize("name", ["edge", "c1"])
def test_fixtures(engine, name, J, skip, tail):
    """The reference-generated fixtures (edge: 31 months of 10..23 days; c1: 360 one-day months),
    trimmed to even N."""
    _check(engine, ("golden", name), J, skip, tail)


@pytest.mark.parametrize("tail", [1, 2])
@pytest.mark.parametrize("N,T_m,J,skip", [(640, 29, 12, 1), (640, 29, 3, 0), (640, 9, 12, 1),
                                          (640, 1, 3, 0), (132, 29, 12, 1), (132, 9, 3, 0),
                                          (132, 1, 12, 1)])
def test_constructed_panel(engine, N, T_m, J, skip, tail):
    """Every gap pattern, the full wave and the full list (see _panel), 1 / 9 / 29 months."""
    _check(engine, ("built", N, T_m), J, skip, tail)


@pytest.mark.parametrize("tail", [1, 2])
@pytest.mark.parametrize("knobs", [dict(mmd=32)])
def test_constructed_panel_other_instantiations(engine, knobs, tail):
    """The 32-day instantiation (a looser bound on the longest month)."""
    _check(engine, ("built", 640, 29), 12, 1, tail, **knobs)


@pytest.mark.parametrize("tail", [1, 2])
def test_dense_gaps(engine, tail):
    """Half of the (asset, month) cells absent: every batch walks a list of ~250 cells a wave,
    in several trips."""
    _check(engine, ("dense",), 12, 1, tail)


@pytest.mark.parametrize("tail", [1, 2])
def test_sparse_gaps(engine, tail):
    """2 % of the cells absent and 2 % of the days missing: short lists, mostly one trip."""
    _check(engine, ("sparse",), 12, 1, tail)


@pytest.mark.parametrize("tail", [1, 2])
@pytest.mark.parametrize("gaps", ["sparse", "dense"])
def test_probed_width(engine, gaps, tail):
    """92,160 assets x 3 months, the narrowest launch "signal_tail" 2 probes: about 4 % (sparse)
    and 51 % (dense) of the last rows hold no price, on either side of the probe's one in eight,
    so the probed launch runs the tail-first kernel for the one and the streaming kernel for the
    other (the kernel not chosen returns without writing).  J = 1, skip = 0: mom_J is defined
    from the second month."""
    _check(engine, ("wide", gaps), 1, 0, tail)


@pytest.mark.parametrize("tail", [1, 2])
@pytest.mark.parametrize("N,T_m", [(640, 29), (132, 9)])
def test_row_slice_between_poison_rows(engine, N, T_m, tail):
    """P is a row-slice view into the middle of a larger tensor whose other rows hold finite
    prices; the slice has gaps (never-listed columns, absent and missing days) in its first and
    last months, so a walk that left the slice would find a price and change PM."""
    Ph, _ = _inputs(("built", N, T_m))
    T_d, pad = Ph.shape[0], 40
    big = torch.full((T_d + 2 * pad, N), 12345.678, dtype=torch.float64, device="cuda:0")
    big[pad:pad + T_d] = _up(Ph)
    _check(engine, ("built", N, T_m), 12, 1, tail, P=big[pad:pad + T_d])
    assert bool((big[:pad] == 12345.678).all()) and bool((big[pad + T_d:] == 12345.678).all())


def test_pipeline_equals_streaming(engine):
    """csm_pipeline and Engine.run(fused=True) on the edge fixture: labels, counts, decile means
    and long-short of "signal_tail" 0, as raw words."""
    Ph, ms_h = _inputs(("golden", "edge"))
    P, ms = _up(Ph), _up(ms_h)
    outs = {}
    try:
        for tail in (0, 1, 2):
            _tune(engine, signal_tail=tail)
            o = engine.pipeline(P, ms, 12, 1, 10, with_pm=True, with_ret=True)
            r = engine.run(P, ms, J=12, skip=1, n_bins=10, fused=True)
            torch.cuda.synchronize()
            outs[tail] = (o, r)
    finally:
        _tune(engine, signal_tail=2)
    for tail in (1, 2):
        for got, base in zip(outs[tail], outs[0]):
            for nm in ("M", "NR", "EW", "LS"):
                _same_words(getattr(got, nm), getattr(base, nm), f"{nm}, signal_tail {tail}")
            for nm in ("L", "CNT"):
                assert torch.equal(getattr(got, nm), getattr(base, nm)), (tail, nm)
