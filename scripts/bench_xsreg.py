#!/usr/bin/env python3
"""Time csm_xs_regress (rules R1..R5) and csm_newey_west (R6) at K = 1, 4 and 8 regressors, with
and without weights, in one process.

Workload: the C4 panel (100,000 assets x 10,000 business days from 1985-01-01 = 461 months,
csmom.synth.make_device_panel) through csm_month_stats; run it with --assets 5000 --days 6522 for
the C2 / C3 width (300 months).  Y is next month's B1 return, S_0 the 12-1 momentum, the other
regressors seeded normal panels with 5 % NaN holes, W uniform in [0.5, 2).  HIP events around each
call, the calls interleaved round by round, median and range over the rounds.  Each call is printed
beside its byte floor: Y, the K regressors (and W) read twice -- once for the means, once for the
centred moments -- at 6.3 TB/s, the achievable HBM rate.

    python scripts/bench_xsreg.py [--assets N] [--days T] [--rounds R] [--warmup W]
                                  [--ks K [K ...]]
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
    ap.add_argument("--ks", type=int, nargs="*", default=[1, 4, 8])
    args = ap.parse_args()

    import torch

    import csmom
    from csmom.synth import bday_calendar, make_device_panel

    if not torch.cuda.is_available():
        sys.exit("bench_xsreg.py needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    eng = csmom.Engine(0)
    N, T_d = args.assets, args.days
    days, ms_host, _ = bday_calendar("1985-01-01", T_d)
    panel = make_device_panel(N, days, ms_host, seed=args.seed, device=dev)
    T_m = len(ms_host) - 1
    PM = eng.month_stats(panel.P, panel.month_start).PM
    del panel
    torch.cuda.empty_cache()
    _, _, X = eng.market_factor(PM, with_x=True)
    Y = torch.cat([X[1:], torch.full_like(X[:1], float("nan"))])
    del X
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    S = [eng.momentum(PM, 12, 1)[1]]
    for _ in range(max(args.ks) - 1):
        s = torch.randn((T_m, N), dtype=torch.float64, device=dev, generator=gen)
        s[torch.rand((T_m, N), device=dev, generator=gen) < 0.05] = float("nan")
        S.append(s)
    W = torch.rand((T_m, N), dtype=torch.float64, device=dev, generator=gen) * 1.5 + 0.5
    cell = 8.0 * T_m * N

    # name -> (call, bytes of the floor)
    calls = {}
    gamma = None
    for K in args.ks:
        for w in (None, W):
            fn = (lambda K=K, w=w: eng.xs_regress(Y, S[:K], w, standardize=True))
            name = f"xs_regress K={K}" + (" +W" if w is not None else "")
            floor = 2.0 * (K + 1 + (w is not None)) * cell
            calls[name] = (fn, floor)
        gamma = eng.xs_regress(Y, S[:K], None, standardize=True).GAMMA
    calls["newey_west"] = (lambda: eng.newey_west(gamma), None)
    defined = int((~torch.isnan(gamma[:, 0])).sum())
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
        line = f"{name:28s} {med:8.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})"
        if floor is not None:
            fl = floor / (HBM_TBS * 1e12) * 1e3
            res[name].update(floor_ms=round(fl, 4), times_floor=round(med / fl, 2))
            line += f"  byte floor {fl:.3f} ms at {HBM_TBS} TB/s: {med / fl:.1f} x"
        print(line, flush=True)
    print(json.dumps(dict(bench="xsreg", assets=N, days=T_d, months=T_m, months_defined=defined,
                          rounds=args.rounds, device=torch.cuda.get_device_name(0), results=res)))


if __name__ == "__main__":
    main()
