"""GPU: the month walk of daytrip.h under each of its five kernels -- k_month_stats, k_daily_sums,
k_daily_fsums, k_liq_sums and k_range_sums -- on one calendar built to take every branch of the
walk, at every chunk count.

The calendar has 16 months of 0, 0, 1, 7, 8, 9, 0, 15, 16, 17, 0, 0, 3, 24, 1, 0 day rows (101 rows):
empty months at the start, at the end and in a row; one-day months; months one row short of a trip
of 4 or 8 rows, exactly a trip and one row over; and a last partial trip.  Every chunk count from 1
to 16 puts a chunk start on every kind of month; 0 is the library's own count.

Bars: each file's own.  Counts are exact and sums bit for bit against the tests/*_ref.py
references, the range sums within test_gpu_range.py's 1e-10 of the reference's scale.  The panels
are make_panel's with about 10 % of the priced rows NaN; volumes and high / low / close are made
from them as test_gpu_liq.py and test_gpu_range.py make theirs.
"""
import ctypes

import numpy as np
import pytest
import torch

import dailymkt_ref as DR
import factor_ref as FR
import liq_ref as LR
import range_ref as RR
import signals_ref as SR
import test_gpu_range as TR
from conftest import bits_equal
from oracle.synth_np import make_panel

pytestmark = pytest.mark.gpu
LENS = [0, 0, 1, 7, 8, 9, 0, 15, 16, 17, 0, 0, 3, 24, 1, 0]
T_DAYS, T_M = 101, 16
SIZES = [1, 2, 257]     # one lane, two assets per lane, a second workgroup that is partly filled
CHUNKS = tuple(range(1, T_M + 1)) + (0,)
MAX_GAP = 3
GAPPY = dict(late=0.2, delist=0.2, nan_day=0.1, absent_month=0.01, nan_month=0.01)
_CACHE = {}


def _up(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _tune(key, value):
    import csmom
    assert csmom.load_library().csm_tune(key.encode(), ctypes.c_int(value)) == 0


def _panel(N):
    """Host panels, their device copies and the five references; made once and left unchanged."""
    if N in _CACHE:
        return _CACHE[N]
    assert sum(LENS) == T_DAYS and len(LENS) == T_M
    ms = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    pan = make_panel(N, T_DAYS, seed=500 + N, cents=True, with_volume=True, **GAPPY)
    P, V = pan["P"], pan["V"]
    rng = np.random.default_rng(600 + N)
    u = rng.random(V.shape)
    V[u < 0.05] = 0.0
    V[u > 0.99] = np.nan
    H, L, C = TR._hlc(P, 700 + N)
    R = DR.daily_ret(P, MAX_GAP)
    FD = FR.seeded_factors(rng.normal(0.0, 0.01, T_DAYS), 77, 4, 0.01, (50, 1))
    FD[20, 0] = np.nan
    fd = {1: np.ascontiguousarray(FD[:, :1]), 4: FD}
    ref = dict(stats=SR.month_stats(P, ms), dsums=DR.daily_sums(R, FD[:, 0], ms),
               fsums={KF: FR.daily_fsums(R, fd[KF], ms) for KF in fd},
               liq=LR.liq_sums(P, V, ms, MAX_GAP), range=RR.range_sums(H, L, C, ms, MAX_GAP))
    _CACHE[N] = dict(ref=ref, Pd=_up(P), Vd=_up(V), Hd=_up(H), Ld=_up(L), Cd=_up(C), msd=_up(ms),
                     FD0d=_up(FD[:, 0]), FDd={KF: _up(fd[KF]) for KF in fd})
    return _CACHE[N]


def _sweep(key, run, check):
    try:
        for chunks in CHUNKS:
            _tune(key, chunks)
            check(run(), chunks)
    finally:
        _tune(key, 0)


@pytest.mark.parametrize("N", SIZES)
def test_month_stats(engine, N):
    pan = _panel(N)
    ref = pan["ref"]["stats"]

    def check(st, chunks):
        for k in ("PM", "P1", "HI", "SSW"):
            assert bits_equal(getattr(st, k).cpu().numpy(), ref[k]), (k, chunks)
        assert np.array_equal(st.NDW.cpu().numpy(), ref["NDW"]), ("NDW", chunks)

    _sweep("stats_chunks", lambda: engine.month_stats(pan["Pd"], pan["msd"]), check)


@pytest.mark.parametrize("N", SIZES)
def test_daily_sums(engine, N):
    pan = _panel(N)
    ref = pan["ref"]["dsums"]

    def check(sums, chunks):
        assert np.array_equal(sums.NO.cpu().numpy(), ref["NO"]), ("NO", chunks)
        for k in DR.SUMS[1:]:
            assert bits_equal(getattr(sums, k).cpu().numpy(), ref[k]), (k, chunks)

    _sweep("dsums_chunks",
           lambda: engine.daily_sums(pan["Pd"], pan["msd"], pan["FD0d"], MAX_GAP), check)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("KF", [1, 4])   # factor rows loaded a trip ahead | a trip's own rows
def test_daily_fsums(engine, KF, N):
    pan = _panel(N)
    ref = pan["ref"]["fsums"][KF]

    def check(sums, chunks):
        assert np.array_equal(sums.NO.cpu().numpy(), ref["NO"]), ("NO", chunks)
        for k in FR.FSUMS[1:]:
            got = getattr(sums, k).cpu().numpy()
            assert got.shape == ref[k].shape and bits_equal(got, ref[k]), (k, chunks)

    _sweep("dfsums_chunks",
           lambda: engine.daily_fsums(pan["Pd"], pan["msd"], pan["FDd"][KF], MAX_GAP), check)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("pair", [0, 1])
def test_liq_sums(engine, pair, N):
    pan = _panel(N)
    ref = pan["ref"]["liq"]

    def check(sums, chunks):
        for k in LR.COUNTS:
            assert np.array_equal(getattr(sums, k).cpu().numpy(), ref[k]), (k, chunks)
        for k in LR.FSUMS:
            assert bits_equal(getattr(sums, k).cpu().numpy(), ref[k]), (k, chunks)

    try:
        _tune("lsums_pair", pair)
        _sweep("lsums_chunks",
               lambda: engine.liq_sums(pan["Pd"], pan["Vd"], pan["msd"], MAX_GAP), check)
    finally:
        _tune("lsums_pair", 0)


@pytest.mark.parametrize("N", SIZES)
def test_range_sums(engine, N):
    pan = _panel(N)
    ref = pan["ref"]["range"]
    _sweep("rsums_chunks",
           lambda: engine.range_sums(pan["Hd"], pan["Ld"], pan["Cd"], pan["msd"], MAX_GAP),
           lambda sums, chunks: TR._check_sums(sums, ref, f"(N={N}, {chunks} chunks)"))
