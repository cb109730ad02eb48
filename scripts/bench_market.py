#!/usr/bin/env python3
"""Time csm_market_factor / csm_market_model / csm_next_ret (rules B1..B6) beside
csm_window_signals on the same month panel, in one process.

Workload: the C4 panel (100,000 assets x 10,000 business days from 1985-01-01 = 461 months,
csmom.synth.make_device_panel) through csm_month_stats; run it with --assets 5000 --days 6522 for
the C2 / C3 width (300 months).  HIP events around each call, the calls interleaved round by
round, median and range over the rounds.  Each call is printed beside its byte floor: PM read once
(8 B per asset-month; csm_next_ret reads S as well) plus 8 B per requested output cell (4 for
NOBS), at 6.3 TB/s, the achievable HBM rate.  k_window_signals is context, not a yardstick: it
reads five month arrays and keeps two windows.

    python scripts/bench_market.py [--assets N] [--days T] [--rounds R] [--warmup W]
                                   [--window Wb] [--chunks C [C ...]]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

HBM_TBS = 6.3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--assets", type=int, default=100_000)
    ap.add_argument("--days", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--window", type=int, default=36)
    ap.add_argument("--chunks", type=int, nargs="*", default=[],
                    help="also time csm_market_model with mm_chunks forced to these values "
                         "(-1: one chunk per month)")
    args = ap.parse_args()

    import torch

    import csmom
    from csmom.synth import bday_calendar, make_device_panel

    if not torch.cuda.is_available():
        sys.exit("bench_market.py needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    eng = csmom.Engine(0)
    lib = eng.lib
    N, T_d = args.assets, args.days
    days, ms_host, _ = bday_calendar("1985-01-01", T_d)
    panel = make_device_panel(N, days, ms_host, seed=args.seed, device=dev)
    T_m = len(ms_host) - 1
    st = eng.month_stats(panel.P, panel.month_start)
    del panel
    torch.cuda.empty_cache()
    PM = st.PM
    M = eng.momentum(PM, 12, 1)[1]
    F, _ = eng.market_factor(PM)
    Wb = args.window
    cell = 8.0 * T_m * N

    def tuned(value, fn):
        def call():
            lib.csm_tune(b"mm_chunks", value)
            try:
                fn()
            finally:
                lib.csm_tune(b"mm_chunks", 0)
        return call

    model_all = lambda: eng.market_model(PM, F, window=Wb)                         # noqa: E731
    model_rm = lambda: eng.market_model(PM, F, window=Wb, outputs=("RESMOM",))      # noqa: E731
    nr_out = eng.empty((T_m, N))
    # name -> (call, bytes of the floor)
    calls = {"market_factor": (lambda: eng.market_factor(PM), cell),
             "market_factor +X": (lambda: eng.market_factor(PM, with_x=True), 2 * cell),
             "market_model": (model_all, cell + 4.5 * cell),
             "model RESMOM only": (model_rm, 2 * cell)}
    for c in args.chunks:
        c = T_m if c < 0 else c
        calls[f"market_model c={c}"] = (tuned(c, model_all), 5.5 * cell)
        calls[f"RESMOM only c={c}"] = (tuned(c, model_rm), 2 * cell)
    calls["next_ret"] = (lambda: eng.next_ret(PM, M, out=nr_out), 3 * cell)
    calls["window_signals"] = (lambda: eng.window_signals(*st, M=M), None)
    calls["window H52 only"] = (lambda: eng.window_signals(*st, outputs=("H52", "NR_H52")), None)
    times = {k: [] for k in calls}
    for r in range(args.warmup + args.rounds):
        for name, (fn, _) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    res = {}
    for name, ts in times.items():
        med = statistics.median(ts)
        floor = calls[name][1]
        res[name] = dict(ms=round(med, 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
        line = f"{name:24s} {med:8.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})"
        if floor is not None:
            fl = floor / (HBM_TBS * 1e12) * 1e3
            res[name].update(floor_ms=round(fl, 4), times_floor=round(med / fl, 2))
            line += f"  byte floor {fl:.3f} ms at {HBM_TBS} TB/s: {med / fl:.1f} x"
        print(line, flush=True)
    print(json.dumps(dict(bench="market", assets=N, days=T_d, months=T_m, window=Wb,
                          rounds=args.rounds, device=torch.cuda.get_device_name(0), results=res)))


if __name__ == "__main__":
    main()
