#!/usr/bin/env python3
"""Time csm_asym_sums / csm_asym_model (rules AS1..AS3) and run_signal("info_disc") against
csm_daily_sums and csm_liq_model on the same panel, in one process.

csm_daily_sums reads what csm_asym_sums reads (P and the daily market, 8 B per asset-day) and
stores 60 B per asset-month against 64 B, so k_daily_sums on the same box, back to back, is the
yardstick.  csm_liq_model at window 12 stands beside csm_asym_model at window 12.  Workload: the
C4 panel (100,000 assets x 10,000 business days from 1985-01-01, csmom.synth.make_device_panel);
run it with --assets 5000 --days 6522 for the C2 / C3 width.  HIP events around each call, the
calls interleaved round by round, median and range over the rounds.  Prints one line per call:
ms, 8 N T_d / time in TB/s for the sums, and the ratio to k_daily_sums's time.

    python scripts/bench_asym.py [--assets N] [--days T] [--rounds R] [--warmup W]
                                 [--sums-chunks C [C ...]] [--model-chunks C [C ...]]
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
    ap.add_argument("--sums-chunks", type=int, nargs="*", default=[],
                    help="also time csm_asym_sums and csm_daily_sums with their chunk knobs "
                         "forced to these values, at one and at two assets per lane")
    ap.add_argument("--model-chunks", type=int, nargs="*", default=[],
                    help="also time csm_asym_model with amodel_chunks forced to these values")
    args = ap.parse_args()

    import torch

    import csmom
    from csmom.synth import bday_calendar, make_device_panel

    if not torch.cuda.is_available():
        sys.exit("bench_asym.py needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    eng = csmom.Engine(0)
    lib = eng.lib
    N, T_d = args.assets, args.days
    days, ms_host, _ = bday_calendar("1985-01-01", T_d)
    panel = make_device_panel(N, days, ms_host, seed=args.seed, device=dev)
    P, ms = panel.P, panel.month_start
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
    PM, _ = eng.month_end(P, ms)
    _, M, _ = eng.momentum(PM, 12, 1)
    sums = eng.asym_sums(P, ms, MKTD, max_month_days=mmd)
    lsums = eng.liq_sums(P, torch.ones_like(P), ms, max_month_days=mmd)
    dsums = lambda: eng.daily_sums(P, ms, MKTD, max_month_days=mmd)      # noqa: E731
    asums = lambda: eng.asym_sums(P, ms, MKTD, max_month_days=mmd)       # noqa: E731
    bare = lambda: eng.asym_sums(P, ms, max_month_days=mmd)              # noqa: E731
    model1 = lambda: eng.asym_model(sums, 1, outputs=("RSJ", "DSVOL"))   # noqa: E731
    model12 = lambda: eng.asym_model(sums, 12, 1, M)                     # noqa: E731
    calls = {"daily_sums": dsums, "asym_sums": asums}
    for pair in (1, 2):
        calls[f"asym_sums per_lane={pair}"] = tuned({b"asums_pair": pair}, asums)
    for c in args.sums_chunks:
        calls[f"daily_sums c={c}"] = tuned({b"dsums_chunks": c}, dsums)
        for pair in (1, 2):
            calls[f"asym_sums per_lane={pair} c={c}"] = tuned(
                {b"asums_pair": pair, b"asums_chunks": c}, asums)
    calls["asym_sums no FD"] = bare
    calls["liq_model Wm=12"] = lambda: eng.liq_model(lsums, 12)
    calls["asym_model Wm=1 (RSJ, DSVOL)"] = model1
    calls["asym_model Wm=12 skip=1 (all)"] = model12
    for c in args.model_chunks:
        calls[f"asym_model Wm=12 skip=1 (all) c={c}"] = tuned({b"amodel_chunks": c}, model12)
    calls["run info_disc"] = lambda: eng.run_signal(P, ms, "info_disc")
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
        res[name] = dict(ms=round(med, 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4),
                         ratio_to_daily_sums=round(med / ref, 3))
        line = f"{name:44s} {med:8.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})  "
        if "sums" in name:
            res[name]["tb_per_s"] = round(8.0 * N * T_d / (med * 1e-3) / 1e12, 3)
            line += f"{res[name]['tb_per_s']:.2f} TB/s of 8 N T_d  "
        print(line + f"{med / ref:.2f} x daily_sums", flush=True)
    print(json.dumps(dict(bench="asym", assets=N, days=T_d, months=T_m, rounds=args.rounds,
                          device=torch.cuda.get_device_name(0), results=res)))


if __name__ == "__main__":
    main()
