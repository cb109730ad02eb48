#!/usr/bin/env python3
"""Time csm_daily_market / csm_daily_sums / csm_daily_model (rules V1..V4) and
run_signal("divol") against csm_month_stats on the same panel, in one process.

csm_month_stats, csm_daily_market and csm_daily_sums each read every day row of the panel once
(8 B per asset-day), so k_month_stats on the same box, back to back, is the yardstick.  Workload:
the C4 panel (100,000 assets x 10,000 business days from 1985-01-01,
csmom.synth.make_device_panel); run it with --assets 5000 --days 6522 for the C2 / C3 width.  HIP
events around each call, the calls interleaved round by round, median and range over the rounds.
Prints one line per call: ms, 8 N T_d / time in TB/s, and the ratio to k_month_stats's time.

    python scripts/bench_dailymkt.py [--assets N] [--days T] [--rounds R] [--warmup W]
                                     [--chunk-days D [D ...]] [--sums-chunks C [C ...]]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--assets", type=int, default=100_000)
    ap.add_argument("--days", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--chunk-days", type=int, nargs="*", default=[],
                    help="also time csm_daily_market with dmkt_chunk_days forced to these values")
    ap.add_argument("--sums-chunks", type=int, nargs="*", default=[],
                    help="also time csm_daily_sums with dsums_chunks forced to these values")
    ap.add_argument("--model-chunks", type=int, nargs="*", default=[],
                    help="also time csm_daily_model with dmodel_chunks forced to these values")
    args = ap.parse_args()

    import torch

    import csmom
    from csmom.synth import bday_calendar, make_device_panel

    if not torch.cuda.is_available():
        sys.exit("bench_dailymkt.py needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    eng = csmom.Engine(0)
    lib = eng.lib
    N, T_d = args.assets, args.days
    days, ms_host, _ = bday_calendar("1985-01-01", T_d)
    panel = make_device_panel(N, days, ms_host, seed=args.seed, device=dev)
    P, ms = panel.P, panel.month_start
    T_m = len(ms_host) - 1
    mmd, _ = eng.month_days(ms)

    def tuned(key, value, fn):
        def call():
            lib.csm_tune(key, value)
            try:
                fn()
            finally:
                lib.csm_tune(key, 0)
        return call

    st_out = tuple(eng.empty((T_m, N)) for _ in range(4)) + (eng.empty((T_m, N), torch.int32),)
    ws = torch.empty(int(lib.csm_daily_market_workspace(T_d, N)), dtype=torch.uint8, device=dev)
    MKTD, _ = eng.daily_market(P, workspace=ws)
    sums = eng.daily_sums(P, ms, MKTD, max_month_days=mmd)
    market = lambda: eng.daily_market(P, workspace=ws)                  # noqa: E731
    dsums = lambda: eng.daily_sums(P, ms, MKTD, max_month_days=mmd)     # noqa: E731
    model1 = lambda: eng.daily_model(sums, 1)                           # noqa: E731
    model12 = lambda: eng.daily_model(sums, 12)                         # noqa: E731
    calls = {"month_stats": lambda: eng.month_stats(P, ms, mmd, out=st_out),
             "daily_market": market}
    for c in args.chunk_days:
        calls[f"daily_market d={c}"] = tuned(b"dmkt_chunk_days", c, market)
    calls["daily_sums"] = dsums
    for c in args.sums_chunks:
        calls[f"daily_sums c={c}"] = tuned(b"dsums_chunks", c, dsums)
    calls["daily_model Wm=1"] = model1
    calls["daily_model Wm=12"] = model12
    for c in args.model_chunks:
        calls[f"daily_model Wm=1 c={c}"] = tuned(b"dmodel_chunks", c, model1)
        calls[f"daily_model Wm=12 c={c}"] = tuned(b"dmodel_chunks", c, model12)
    calls["run divol"] = lambda: eng.run_signal(P, ms, "divol")
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
    bytes_read = 8.0 * N * T_d
    ref = statistics.median(times["month_stats"])
    res = {}
    for name, ts in times.items():
        med = statistics.median(ts)
        res[name] = dict(ms=round(med, 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4),
                         tb_per_s=round(bytes_read / (med * 1e-3) / 1e12, 3),
                         ratio_to_month_stats=round(med / ref, 3))
        print(f"{name:26s} {med:8.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})  "
              f"{res[name]['tb_per_s']:.2f} TB/s of 8 N T_d  {med / ref:.2f} x month_stats",
              flush=True)
    print(json.dumps(dict(bench="dailymkt", assets=N, days=T_d, months=T_m, rounds=args.rounds,
                          device=torch.cuda.get_device_name(0), results=res)))


if __name__ == "__main__":
    main()
