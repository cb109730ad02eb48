#!/usr/bin/env python3
"""Time csm_daily_returns (rule E7) against k_signal on the same panel, in one process.

Both kernels read the daily panel once (8 B per asset-day), so k_signal on the same box, back
to back, is the yardstick.  Workload: the C4 panel (100,000 assets x 10,000 business days from
1985-01-01, csmom.synth.make_device_panel), labels and next returns from Engine.run, K = 1 and
K = 6, equal weights.  HIP events around each call, the three calls interleaved round by round,
median and range over the rounds.  Prints one line per call: ms, 8 N T_d / time in TB/s, and
the ratio to k_signal's time.

    python scripts/bench_daily.py [--assets N] [--days T] [--rounds R] [--warmup W]
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
    args = ap.parse_args()

    import torch

    import csmom
    from csmom.synth import bday_calendar, make_device_panel

    if not torch.cuda.is_available():
        sys.exit("bench_daily.py needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    eng = csmom.Engine(0)
    N, T_d = args.assets, args.days
    days, ms_host, _ = bday_calendar("1985-01-01", T_d)
    panel = make_device_panel(N, days, ms_host, seed=args.seed, device=dev)
    P, ms = panel.P, panel.month_start
    T_m = len(ms_host) - 1
    mmd, _ = eng.month_days(ms)
    run = eng.run(P, ms, J=12, skip=1, n_bins=10, max_month_days=mmd)
    L, NR = run.L, run.NR
    sig_out = (None, None, eng.empty((T_m, N)), eng.empty((T_m, N)))
    calls = {"k_signal": lambda: eng.signal(P, ms, mmd, 12, 1, out=sig_out)}
    for K in (1, 6):
        nbytes = int(eng.lib.csm_daily_workspace(T_d, N, T_m, 10, K))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = (eng.empty((T_d, 10)), eng.empty((T_d,)), eng.empty((T_m, K, 10), torch.int32))
        calls[f"daily K={K}"] = (lambda K=K, ws=ws, out=out: eng.daily_returns(
            P, ms, L, NR, 10, K, max_month_days=mmd, out=out, workspace=ws))
        print(f"# daily K={K}: workspace {nbytes / 1e6:.0f} MB", flush=True)
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
    sig = statistics.median(times["k_signal"])
    res = {}
    for name, ts in times.items():
        med = statistics.median(ts)
        res[name] = dict(ms=round(med, 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4),
                         tb_per_s=round(bytes_read / (med * 1e-3) / 1e12, 3),
                         ratio_to_k_signal=round(med / sig, 3))
        print(f"{name:12s} {med:8.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})  "
              f"{res[name]['tb_per_s']:.2f} TB/s of 8 N T_d  {med / sig:.2f} x k_signal",
              flush=True)
    print(json.dumps(dict(bench="daily_returns", assets=N, days=T_d, months=T_m,
                          rounds=args.rounds, device=torch.cuda.get_device_name(0),
                          results=res)))


if __name__ == "__main__":
    main()
