"""CPU: the E7 restatement (tests/daily_ref.py) against the portfolio oracle.  On a fully priced
panel the month's product of 1 + DR telescopes to the cohort-mean value on the last day, which
is 1 + PR of E1 / E2; the bar is 1e-10 relative on the gross return, the project's bar for EW /
PR (the telescoped product itself rounds at ~1e-15).  On a panel with gaps the daily series
carries a position flat, checked on hand-worked cells."""
import numpy as np
import pytest

import daily_ref as DRF
from oracle import csmom_oracle as O
from oracle import portfolio_oracle as PO
from oracle.synth_np import make_panel

REL = 1e-10
N_BINS = 5


@pytest.fixture(scope="module")
def dense():
    pan = make_panel(40, 14 * 21 + 6, seed=11, late=0, delist=0, nan_day=0, absent_month=0,
                     nan_month=0, with_volume=False)
    P, ms = pan["P"], pan["month_start"]
    assert len(ms) - 1 >= 14 and not np.isnan(P).any()
    ref = O.pipeline(P, ms, 3, 1, N_BINS)
    W = np.random.default_rng(12).lognormal(0.0, 1.0, ref["L"].shape)
    return P, ms, ref["L"], ref["NR"], W


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("vw", [False, True])
def test_monthly_product_is_the_oracle_return(dense, K, vw):
    P, ms, L, NR, W = dense
    W = W if vw else None
    DR, DLS, DCNT = DRF.daily_returns(P, ms, L, NR, N_BINS, K, W)
    ref = PO.portfolio(L, NR, N_BINS, K, W)
    PR, CNT = ref["PR"][:, 0, :], ref["CNT"][:, :, 0, :]
    gross = DRF.monthly_gross(DR, ms)
    T_m = len(ms) - 1
    assert np.isnan(gross[0]).all()                      # month 0 has no portfolio
    assert (~np.isnan(PR)).sum() > 5 * N_BINS
    for t in range(T_m - 1):
        g, r = gross[t + 1], 1.0 + PR[t]
        assert np.array_equal(np.isnan(g), np.isnan(r)), t
        ok = ~np.isnan(r)
        assert (np.abs(g[ok] - r[ok]) <= REL * np.abs(r[ok])).all(), (t, g, r)
    assert np.array_equal(DCNT, CNT)
    both = ~np.isnan(DR[:, 0]) & ~np.isnan(DR[:, -1])
    assert np.array_equal(np.isnan(DLS), ~both)


def test_gaps_are_carried_flat():
    """Four 3-day months, three assets, two bins.  Asset 0 has NaN days at the start of month
    1 (its base and fill cross the month boundary); asset 1 has no price from month 2 on (a
    two-month gap: the position stays at its last value); asset 2 alone is bin 0."""
    nan = np.nan
    ms = np.array([0, 3, 6, 9, 12])
    P = np.array([[10, 10, 10, nan, nan, 12, 12, 12, 12, 12, 12, 15],
                  [20, 20, 20, 22, 22, 22, nan, nan, nan, nan, nan, nan],
                  [5, 5, 5, 5, 6, 6, 6, 6, 3, 3, 3, 3]], dtype=np.float64).T.copy()
    P[6:9, 1] = np.array([O.ABSENT_BITS], dtype=np.uint64).view(np.float64)[0]
    L = np.tile(np.array([1, 1, 0], dtype=np.int8), (4, 1))
    NR = np.zeros((4, 3))
    NR[3] = nan
    DR, DLS, DCNT = DRF.daily_returns(P, ms, L, NR, 2, 1, None)
    assert np.isnan(DR[:3]).all() and np.isnan(DLS[:3]).all()
    # month 1, bin 1 = {0, 1}, bases (10, 20): values (1, 1.1), (1, 1.1), (1.2, 1.1)
    assert DR[3, 1] == 1.05 / 1.0 - 1.0 and DR[4, 1] == 0.0
    assert DR[5, 1] == ((12 / 10 + 22 / 20) / 2) / ((10 / 10 + 22 / 20) / 2) - 1.0
    # month 2, bases (12, 22): asset 1 has no price, its value stays 22 / 22 = 1
    assert (DR[6:9, 1] == 0.0).all()
    assert np.array_equal(DR[6:9, 0], [0.0, 0.0, 3 / 6 - 1.0])
    # month 3: still flat for asset 1 (base 22 from two months back); asset 0 ends at 15 / 12
    assert (DR[9:11, 1] == 0.0).all() and DR[11, 1] == (15 / 12 + 1.0) / 2 - 1.0
    assert DLS[8] == 0.0 - (3 / 6 - 1.0)
    assert np.array_equal(DCNT[:, 0, :], [[1, 2], [1, 2], [1, 2], [0, 0]])
    # a NaN next_ret takes the asset out of the month's cohort
    NR[1, 1] = nan
    DR2, _, DCNT2 = DRF.daily_returns(P, ms, L, NR, 2, 1, None)
    assert DCNT2[1, 0, 1] == 1 and np.array_equal(DR2[:6], DR[:6], equal_nan=True)
