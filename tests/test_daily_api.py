"""The public surface of the daily portfolio series (rule E7).  CPU: the C prototypes, their
ctypes entries and the Python entry points exist.  GPU: csmom.daily_portfolio_returns on the
cached daily CSVs of tests/golden/daily_csv.tar.xz -- a frame indexed by the fixture's trading
days whose legs, compounded over a month, are the legs of monthly_replication (1e-10 relative on
the gross return, on the months where every member has a month-end price on both sides)."""
import re
import tarfile

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

REF_DATA = GOLDEN / "daily_csv.tar.xz"
TICKERS = ["AAPL", "MSFT", "AMZN", "GOOGL", "NVDA", "TSLA", "META", "JPM", "BAC", "WMT", "PG",
           "KO", "DIS", "CSCO", "ORCL", "INTC", "AMD", "NFLX", "C", "GS"]
NEW = ("csm_daily_workspace", "csm_daily_returns", "csm_series_stats")


def test_prototypes_and_entry_points_exist():
    import csmom
    from csmom import _lib
    header = (ROOT / "include" / "csmom.h").read_text()
    for name in NEW:
        assert re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["csm_daily_returns"][1]) == 16
    assert callable(csmom.Engine.daily_returns) and callable(csmom.Engine.series_stats)
    assert callable(csmom.daily_portfolio_returns)
    assert [f for f in csmom.DailyOut.__dataclass_fields__] == ["DR", "DLS", "DCNT"]


@pytest.mark.gpu
def test_daily_frame_compounds_to_the_monthly_legs(engine, tmp_path):
    import csmom
    import csmom.data as D
    with tarfile.open(REF_DATA) as tar:
        for n in tar.getnames():
            (tmp_path / n).write_bytes(tar.extractfile(n).read())
    df = D.fetch_daily(TICKERS, data_dir=str(tmp_path), verbose=False)
    n_bins = 10
    frame = csmom.daily_portfolio_returns(df, lookback_months=12, skip_months=1, n_bins=n_bins)
    panel = csmom.from_long(df)
    assert frame.index.equals(panel.days) and len(frame) == len(panel.days)
    assert list(frame.columns) == list(range(n_bins)) + ["long_short"]
    both = frame[0].notna() & frame[n_bins - 1].notna()
    assert np.array_equal(frame["long_short"].notna().to_numpy(), both.to_numpy())
    d = (frame[n_bins - 1] - frame[0])[both]
    assert np.array_equal(frame["long_short"][both].to_numpy(), d.to_numpy())

    res = csmom.monthly_replication(df, n_bins=n_bins, plot_path=None, compute_turnover=False,
                                    keep_monthly=True, verbose=False)
    price = res.monthly.pivot(index="date", columns="ticker", values="adj_close")
    mom = res.monthly.pivot(index="date", columns="ticker", values="mom_J")
    price = price.reindex(panel.month_end)
    mom = mom.reindex(panel.month_end)
    ms = panel.month_start
    checked = 0
    for t in range(panel.T_m - 1):
        date = panel.month_end[t]
        members = mom.iloc[t].notna().to_numpy()
        if date not in res.ew.index or not members.any():
            continue
        if price.iloc[t].isna().to_numpy()[members].any() or \
                price.iloc[t + 1].isna().to_numpy()[members].any():
            continue   # a member without a month-end price: the monthly row spans the gap
        days = frame.iloc[ms[t + 1]:ms[t + 2]]
        for leg in (0, n_bins - 1):
            want = res.ew.loc[date].get(float(leg), np.nan)
            if np.isnan(want):
                continue
            got = float(np.prod(1.0 + days[leg].to_numpy()))
            assert abs(got - (1.0 + want)) <= 1e-10 * abs(1.0 + want), (date, leg, got, want)
            checked += 1
    assert checked >= 48, checked
