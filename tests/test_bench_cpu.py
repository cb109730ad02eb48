"""CPU: the bench's host plumbing -- the business-day calendar (pd.bdate_range on numpy days, so
weak-scaling calendars past pandas' Timestamp range work), the whole-month date shards of 2 / 4 /
8 ranks in both scaling modes, and `bench.py --gpus N`'s self-launch decision (the parent starts
the workers and never touches the GPU)."""
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


@pytest.mark.parametrize("start,n", [("1985-01-01", 10_000), ("2000-01-03", 6_522),
                                     ("1985-01-05", 1_100), ("2000-01-01", 1)])
def test_bday_calendar_is_pandas(start, n):
    from csmom.panel import month_offsets
    from csmom.synth import bday_calendar
    days, ms, mend = bday_calendar(start, n)
    ref = pd.bdate_range(start, periods=n)
    ms_r, mend_r = month_offsets(ref)
    assert days.equals(ref) and np.array_equal(ms, ms_r) and mend.equals(mend_r)


@pytest.mark.parametrize("G", [1, 2, 4, 8])
@pytest.mark.parametrize("scaling", ["strong", "weak"])
def test_shard_calendar_c4(G, scaling):
    """C4's calendar split over G ranks: strong = the fixed 10,000 bdays, weak = 10,000 per rank
    (8 ranks: 80,000 bdays from 1985, past 2262).  The shards are contiguous whole months that
    cover the calendar, and every rank agrees on the month counts."""
    from csmom.synth import bday_calendar, shard_calendar
    total = 10_000 * (G if scaling == "weak" else 1)
    days, ms, mend = bday_calendar("1985-01-01", total)
    T_m = len(ms) - 1
    got_days, parts = [], None
    for r in range(G):
        d, msl, me, months = shard_calendar("1985-01-01", total, G, r)
        parts = parts or months
        assert months == parts and sum(months) == T_m and len(msl) == months[r] + 1
        assert msl[0] == 0 and msl[-1] == len(d) and (np.diff(msl) > 0).all()
        got_days.append(np.asarray(d).astype("datetime64[D]"))
    assert np.array_equal(np.concatenate(got_days), np.asarray(days).astype("datetime64[D]"))
    assert max(parts) - min(parts) <= 1


def test_make_device_panel_past_pandas_range():
    """The weak-scaling 8-rank calendar's last shard (dates in the 2280s) builds a panel."""
    import torch
    from csmom.synth import make_device_panel, shard_calendar
    d, ms, _, _ = shard_calendar("1985-01-01", 80_000, 8, 7)
    assert np.asarray(d).astype("datetime64[D]")[-1] > np.datetime64("2262-04-11")
    k = 14                                      # its first 14 months
    pan = make_device_panel(8, d[:ms[k]], ms[:k + 1], seed=1, device="cpu",
                            shard=(7, 8, 4, 10_000.0))
    assert pan.P.shape[0] == ms[k] and pan.P.dtype == torch.float64
    assert len(pan.month_end) == len(pan.month_start_host) - 1


def test_dump_outputs_files(tmp_path):
    """--dump-outputs' writer: small arrays whole, the wide ones on one fixed seeded column sample
    that keeps the files within 64 MB, everything finite (a float array's NaN / inf cells are
    written as 0 and coded in <name>_nonfinite.npy) and the same from call to call."""
    import torch
    import bench
    assert bench.parse([]).full is False and bench.parse([]).dump_outputs is None
    assert bench.parse(["--full", "--dump-outputs", "x"]).dump_outputs == "x"
    rows, N = 461, 100_000                       # C4's months x assets (int8 keeps this small)
    L = (torch.arange(rows * N, dtype=torch.int64) % 11 - 1).to(torch.int8).reshape(rows, N)
    LS = torch.arange(rows, dtype=torch.float64)
    LS[:3] = torch.tensor([float("nan"), float("inf"), float("-inf")], dtype=torch.float64)
    small = dict(LS=LS, CNT=torch.ones(rows, 10, dtype=torch.int32))
    M = L.to(torch.float64)
    M[L < 0] = float("nan")
    wide = dict(M=M, NR=M, L=L)
    a, b = tmp_path / "a", tmp_path / "b" / "nested"
    bench.dump_outputs(a, small, wide)
    bench.dump_outputs(b, small, wide)
    fa = {f.name: np.load(f) for f in a.iterdir()}
    fb = {f.name: np.load(f) for f in b.iterdir()}
    assert sorted(fa) == ["CNT.npy", "L.npy", "LS.npy", "LS_nonfinite.npy", "M.npy",
                          "M_nonfinite.npy", "NR.npy", "NR_nonfinite.npy", "columns.npy"]
    assert sorted(fb) == sorted(fa) and all(np.array_equal(fa[k], fb[k]) for k in fa)
    assert all(v.dtype == (np.float32 if "_nonfinite" in k else np.float64) for k, v in fa.items())
    assert all(np.isfinite(v).all() for v in fa.values())
    assert sum(v.nbytes for v in fa.values()) <= 64 << 20
    cols = fa["columns.npy"].astype(np.int64)
    assert 1000 < len(cols) < N and (np.diff(cols) > 0).all() and cols[-1] < N
    assert np.array_equal(fa["L.npy"], L.numpy()[:, cols].astype(np.float64))
    assert np.array_equal(fa["LS.npy"][3:], np.arange(3.0, rows)) and not fa["LS.npy"][:3].any()
    assert fa["LS_nonfinite.npy"].tolist() == [1.0, 2.0, 3.0] + [0.0] * (rows - 3)
    Lc = L.numpy()[:, cols]
    assert np.array_equal(fa["M_nonfinite.npy"], (Lc < 0).astype(np.float32))
    assert np.array_equal(fa["M.npy"], np.where(Lc < 0, 0.0, Lc))
    # a narrow panel is written whole
    bench.dump_outputs(tmp_path / "c", {}, dict(M=M[:, :50]))
    assert np.array_equal(np.load(tmp_path / "c" / "columns.npy"), np.arange(50.0))
    assert np.load(tmp_path / "c" / "M.npy").shape == (rows, 50)


def test_gpus_n_self_launches(monkeypatch):
    """Without a torchrun environment `--gpus N > 1` hands the argv to spawn_workers (the parent
    imports no torch); with WORLD_SIZE set (a worker) it runs the bench itself."""
    import bench
    seen = []
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(bench, "spawn_workers", lambda argv: seen.append(argv) or 0)
    argv = ["--gpus", "8", "--steps", "5"]
    assert bench.main(argv) is None and seen == [argv]
    monkeypatch.setattr(bench, "spawn_workers", lambda argv: 3)
    with pytest.raises(SystemExit) as e:
        bench.main(argv)
    assert e.value.code == 3
    assert bench.parse([]).scaling == "strong" and bench.parse([]).gpus == 1
