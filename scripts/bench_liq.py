#!/usr/bin/env python3
"""Time csm_liq_sums / csm_liq_model (rules Q1..Q3) and run_signal("illiq") against
csm_daily_sums on the same panel, in one process.

csm_daily_sums walks the price panel as csm_liq_sums does and reads half its bytes (8 B per
asset-day against 16 B), so k_daily_sums on the same box, back to back, is the yardstick: about
twice its time is the bandwidth-proportional figure.  Workload: the C4 panel (100,000 assets x
10,000 business days from 1985-01-01, csmom.synth.make_device_panel) with a seeded volume panel
beside it (rounded lognormal, about 5 % zero and 1 % NaN cells); run it with --assets 5000 --days
6522 for the C2 / C3 width.  HIP events around each call, the calls interleaved round by round,
median and range over the rounds.  Prints one line per call: ms, 16 N T_d / time in TB/s (8 N T_d
for daily_sums), and the ratio to k_daily_sums's time.

    python scripts/bench_liq.py [--assets N] [--days T] [--rounds R] [--warmup W]
                                [--sums-chunks C [C ...]] [--paired]
                                [--model-chunks C [C ...]]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def volume_panel(T_d, N, seed, device, block_days=512):
    """[T_d][N] rounded lognormal volumes, about 5 % zeros and 1 % NaN, built in HBM."""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(int(seed) * 31 + 7)
    V = torch.empty((T_d, N), dtype=torch.float64, device=device)
    for d0 in range(0, T_d, block_days):
        d1 = min(T_d, d0 + block_days)
        z = torch.randn(d1 - d0, N, generator=g, dtype=torch.float64, device=device)
        u = torch.rand(d1 - d0, N, generator=g, dtype=torch.float64, device=device)
        v = torch.exp(z + 13.0).round()
        v[u < 0.05] = 0.0
        v[u > 0.99] = float("nan")
        V[d0:d1] = v
    return V


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--assets", type=int, default=100_000)
    ap.add_argument("--days", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--sums-chunks", type=int, nargs="*", default=[],
                    help="also time csm_liq_sums with lsums_chunks forced to these values")
    ap.add_argument("--paired", action="store_true",
                    help="... and with lsums_pair = 1 (two assets per lane) as well")
    ap.add_argument("--model-chunks", type=int, nargs="*", default=[],
                    help="also time csm_liq_model with lmodel_chunks forced to these values")
    args = ap.parse_args()

    import torch

    import csmom
    from csmom.synth import bday_calendar, make_device_panel

    if not torch.cuda.is_available():
        sys.exit("bench_liq.py needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    eng = csmom.Engine(0)
    lib = eng.lib
    N, T_d = args.assets, args.days
    days, ms_host, _ = bday_calendar("1985-01-01", T_d)
    panel = make_device_panel(N, days, ms_host, seed=args.seed, device=dev)
    P, ms = panel.P, panel.month_start
    V = volume_panel(T_d, N, args.seed, dev)
    T_m = len(ms_host) - 1
    mmd, _ = eng.month_days(ms)

    def tuned(knobs, fn):
        def call():
            for k, v in knobs.items():
                lib.csm_tune(k, v)
            try:
                fn()
            finally:
                for k in knobs:
                    lib.csm_tune(k, 0)
        return call

    MKTD, _ = eng.daily_market(P)
    sums = eng.liq_sums(P, V, ms, max_month_days=mmd)
    dsums = lambda: eng.daily_sums(P, ms, MKTD, max_month_days=mmd)     # noqa: E731
    lsums = lambda: eng.liq_sums(P, V, ms, max_month_days=mmd)          # noqa: E731
    model1 = lambda: eng.liq_model(sums, 1)                             # noqa: E731
    model12 = lambda: eng.liq_model(sums, 12)                           # noqa: E731
    calls = {"daily_sums": dsums, "liq_sums": lsums}
    for pair in ([0, 1] if args.paired else [0]):
        if pair:
            calls["liq_sums per_lane=2"] = tuned({b"lsums_pair": 1}, lsums)
        for c in args.sums_chunks:
            calls[f"liq_sums per_lane={1 + pair} c={c}"] = tuned(
                {b"lsums_pair": pair, b"lsums_chunks": c}, lsums)
    calls["liq_model Wm=1"] = model1
    calls["liq_model Wm=12"] = model12
    for c in args.model_chunks:
        calls[f"liq_model Wm=1 c={c}"] = tuned({b"lmodel_chunks": c}, model1)
        calls[f"liq_model Wm=12 c={c}"] = tuned({b"lmodel_chunks": c}, model12)
    calls["run illiq"] = lambda: eng.run_signal(P, ms, "illiq", V=V)
    times = {k: [] for k in calls}
    for r in range(args.warmup + args.rounds):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    ref = statistics.median(times["daily_sums"])
    res = {}
    print(f"--- {N} assets x {T_d} days ({T_m} months)", flush=True)
    for name, ts in times.items():
        med = statistics.median(ts)
        per = 8.0 if name == "daily_sums" else 16.0
        res[name] = dict(ms=round(med, 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4),
                         tb_per_s=round(per * N * T_d / (med * 1e-3) / 1e12, 3),
                         ratio_to_daily_sums=round(med / ref, 3))
        print(f"{name:44s} {med:8.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})  "
              f"{res[name]['tb_per_s']:.2f} TB/s of {per:.0f} N T_d  {med / ref:.2f} x daily_sums",
              flush=True)
    print(json.dumps(dict(bench="liq", assets=N, days=T_d, months=T_m, rounds=args.rounds,
                          device=torch.cuda.get_device_name(0), results=res)))


if __name__ == "__main__":
    main()
