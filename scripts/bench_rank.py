#!/usr/bin/env python3
"""Time csm_xs_rank and csm_rank_ic on the C4 monthly panel shape, in one process.

Workload: a synthetic signal panel made on the device ([months][assets] normal draws, 10 % NaN),
a later-return panel with 10 % NaN, static group ids drawn uniformly.  Candidates: xs_rank over
the whole cross-section (one segment per date, past the LDS cap: the tiled sort) and inside G
groups (LDS sorts), rank_ic with and without the Pearson pass, and for scale csm_group_deciles'
labels on the same segments (the same sort, no searches).  HIP events around each candidate, the
candidates interleaved round by round, median and range over the rounds.

    python scripts/bench_rank.py [--assets N] [--months T] [--groups G] [--rounds R]
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
    ap.add_argument("--months", type=int, default=461)
    ap.add_argument("--groups", type=int, default=49)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=4)
    args = ap.parse_args()

    import torch

    import csmom

    if not torch.cuda.is_available():
        sys.exit("bench_rank.py needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    eng = csmom.Engine(0)
    T_m, N, G = args.months, args.assets, args.groups
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    S = torch.randn((T_m, N), generator=gen, device=dev, dtype=torch.float64) * 0.3
    S[torch.rand((T_m, N), generator=gen, device=dev) < 0.1] = float("nan")
    Y = 0.1 * torch.nan_to_num(S) + torch.randn((T_m, N), generator=gen, device=dev,
                                                dtype=torch.float64) * 0.08
    Y[torch.rand((T_m, N), generator=gen, device=dev) < 0.1] = float("nan")
    gid = torch.randint(0, G, (N,), generator=gen, device=dev).to(torch.int16)
    zeros = torch.zeros(N, dtype=torch.int16, device=dev)
    out = torch.empty_like(S)

    calls = {
        "xs_rank G=1": lambda: eng.xs_rank(S, pct=True, out=out),
        f"xs_rank G={G}": lambda: eng.xs_rank(S, gid, G, pct=True, out=out),
        "rank_ic (RIC + PIC)": lambda: eng.rank_ic(S, Y, lead=1),
        "rank_ic (RIC only)": lambda: eng.rank_ic(S, Y, lead=1, pearson=False),
        "group_deciles labels G=1": lambda: eng.deciles_within(S, None, zeros, 1, 10),
        f"group_deciles labels G={G}": lambda: eng.deciles_within(S, None, gid, G, 10),
    }
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
    res = {}
    for name, ts in times.items():
        med = statistics.median(ts)
        res[name] = dict(ms=round(med, 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
        print(f"{name:30s} {med:9.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})", flush=True)
    ic = eng.rank_ic(S, Y, lead=1)
    print(f"mean rank IC {torch.nanmean(ic.RIC).item():.4f}, mean n {ic.NOBS.float().mean().item():.0f}")
    print(json.dumps(dict(bench="rank", assets=N, months=T_m, groups=G, rounds=args.rounds,
                          device=torch.cuda.get_device_name(0), results=res)))


if __name__ == "__main__":
    main()
