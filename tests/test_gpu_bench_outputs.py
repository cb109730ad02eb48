"""bench.py on one GPU: the plain run (setup, warm-up, the timed steps, the line) against
`--full`, and `--dump-outputs DIR` -- what the last timed step computed, as finite .npy files
(NaN cells written as 0 and marked in <name>_nonfinite.npy), identical from run to run and equal
to the engine's own pipeline on the same seeded panel."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from conftest import bits_equal  # noqa: E402

pytestmark = pytest.mark.gpu
N, DAYS, SEED = 32_772, 700, 4      # wide enough for the benched path (ids: N > 16384, N % 4 == 0)
ARGS = ["--gpus", "1", "--assets", str(N), "--days", str(DAYS), "--seed", str(SEED)]


def _load(d):
    return {f.stem: np.load(f) for f in sorted(Path(d).glob("*.npy"))}


def _with_nan(got, name):
    """The dumped array with its marked cells back as NaN (the outputs here carry no inf)."""
    code = got[name + "_nonfinite"]
    assert set(np.unique(code).tolist()) <= {0.0, 1.0}
    return np.where(code == 1, np.nan, got[name])


@pytest.fixture(scope="module")
def plain(engine, tmp_path_factory):
    import bench
    d = tmp_path_factory.mktemp("dump_a")
    line = bench.main(ARGS + ["--steps", "3", "--warmup", "1", "--dump-outputs", str(d)])
    return line, _load(d)


def test_plain_line(plain):
    line, _ = plain
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "asset-days/s" and line["dtype"] == "f64" and line["higher_is_better"]
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - N * DAYS / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert line["engine_path"].startswith("fused k_signal (+ bucket ids)")
    # nothing that takes a run of its own
    assert line["cpu_baseline"] is None and line["decile_match_pct"] is None
    assert line["mom_bit_exact_pct"] is None and line["decile_check"] is None


def test_dump_is_the_pipeline(engine, plain):
    """The dumped arrays are the engine's pipeline on bench.py's N = 1 panel: the small ones whole,
    the (months, N) ones on the listed columns."""
    from csmom.synth import bday_calendar, make_device_panel
    _, got = plain
    assert sorted(got) == ["CNT", "EW", "EW_nonfinite", "L", "LS", "LS_nonfinite", "M",
                           "M_nonfinite", "NR", "NR_nonfinite", "columns"]
    assert all(a.dtype == (np.float32 if k.endswith("_nonfinite") else np.float64)
               for k, a in got.items())
    assert all(np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    days, ms_h, _ = bday_calendar("1985-01-01", DAYS)
    pan = make_device_panel(N, days, ms_h, seed=SEED * 1000, device=engine.device,
                            shard=(0, 1, SEED, float(DAYS)))
    one = engine.pipeline(pan.P, pan.month_start, 12, 1, 10)
    torch.cuda.synchronize()
    cols = got["columns"].astype(np.int64)
    assert len(cols) == len(set(cols.tolist())) and (np.diff(cols) > 0).all()
    assert 0 <= cols[0] and cols[-1] < N
    assert bits_equal(_with_nan(got, "LS"), one.LS.cpu().numpy())
    assert bits_equal(_with_nan(got, "EW"), one.EW.cpu().numpy())
    assert np.array_equal(got["CNT"], one.CNT.cpu().numpy().astype(np.float64))
    assert bits_equal(_with_nan(got, "M"), one.M.cpu().numpy()[:, cols])
    assert bits_equal(_with_nan(got, "NR"), one.NR.cpu().numpy()[:, cols])
    assert np.array_equal(got["L"], one.L.cpu().numpy()[:, cols].astype(np.float64))
    assert (got["LS_nonfinite"] == 0).any() and (got["LS_nonfinite"] == 1).any()
    assert (got["L"] >= 0).any()


def test_dump_repeats_and_full_checks(engine, plain, tmp_path):
    """A second run with other step counts and --full dumps the same bits (same inputs, same
    outputs), and --full's line carries the checks the plain line leaves out."""
    import bench
    line = bench.main(ARGS + ["--steps", "2", "--warmup", "0", "--full", "--cpu-assets", "200",
                              "--dump-outputs", str(tmp_path)])
    again = _load(tmp_path)
    _, got = plain
    assert sorted(again) == sorted(got)
    for k in got:
        assert bits_equal(again[k], got[k]), k
    assert line["steps"] == 2
    assert line["decile_match_pct"] == 100.0 and line["mom_bit_exact_pct"] == 100.0
    assert line["cpu_baseline"]["value"] > 0
    assert line["roofline"]["kernel"] == "k_signal" and line["stage_ms"]


def test_sweep_dump_and_full(engine, tmp_path):
    """C3 at a small size: the plain run dumps the summary table of its last step; --full adds
    the per-stage times and the decile match and dumps the same table."""
    import bench
    argv = ["--gpus", "1", "--config", "c3", "--assets", "1000", "--days", "2600", "--steps", "2",
            "--warmup", "1"]
    a, b = tmp_path / "a", tmp_path / "b"
    plain_line = bench.main(argv + ["--dump-outputs", str(a)])
    full_line = bench.main(argv + ["--full", "--no-cpu-baseline", "--dump-outputs", str(b)])
    ta, tb = np.load(a / "table.npy"), np.load(b / "table.npy")
    assert ta.dtype == np.float64 and ta.shape == (1, 16, 7) and bits_equal(ta, tb)
    assert np.isfinite(ta).all() and np.load(a / "table_nonfinite.npy").shape == ta.shape
    assert np.array_equal(np.load(a / "table_nonfinite.npy"), np.load(b / "table_nonfinite.npy"))
    assert plain_line["stage_ms"] is None and plain_line["roofline"] is None
    assert plain_line["cpu_baseline"] is None and "decile_match" not in plain_line
    assert plain_line["ms_per_step"] > 0 and plain_line["unit"] == "asset-day-strategies/s"
    assert full_line["stage_ms"] and full_line["roofline"]["kernel"] in full_line["stage_ms"]
    assert full_line["decile_match_pct"] == 100.0
