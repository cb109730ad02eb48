#!/usr/bin/env python3
"""Time csm_group_deciles (labels + pooled decile means) against what it replaces, the loop over
groups on existing calls -- mask the signal to one group, csm_deciles, merge the labels -- and
csm_group_stats alone, in one process.

Workload: a synthetic signal panel made on the device ([months][assets] normal draws, 10 % NaN,
its next returns, static group ids drawn uniformly).  HIP events around each candidate, the
candidates interleaved round by round, median and range over the rounds.  The ratio of the
49-group to the 11-group time of the new call is the claim that its cost does not grow with the
number of groups; the loop's grows in proportion.

    python scripts/bench_groups.py [--assets N] [--months T] [--groups G [G ...]] [--rounds R]
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
    ap.add_argument("--groups", type=int, nargs="+", default=[11, 49])
    ap.add_argument("--bins", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=4)
    args = ap.parse_args()

    import torch

    import csmom

    if not torch.cuda.is_available():
        sys.exit("bench_groups.py needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    eng = csmom.Engine(0)
    T_m, N, nb = args.months, args.assets, args.bins
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    S = torch.randn((T_m, N), generator=gen, device=dev, dtype=torch.float64) * 0.3
    S[torch.rand((T_m, N), generator=gen, device=dev) < 0.1] = float("nan")
    NR = torch.randn((T_m, N), generator=gen, device=dev, dtype=torch.float64) * 0.08
    nan = torch.full_like(S, float("nan"))

    def loop(gid2, G):
        L = torch.full((T_m, N), -1, dtype=torch.int8, device=dev)
        for g in range(G):
            m = gid2 == g
            Lg, _, _, _ = eng.deciles(torch.where(m, S, nan), NR, nb)
            L = torch.where(m, Lg, L)
        return L

    calls = {}
    gids = {}
    for G in args.groups:
        gid = torch.randint(0, G, (N,), generator=gen, device=dev).to(torch.int16)
        gids[G] = gid
        gid2 = gid.expand(T_m, N)
        calls[f"group_deciles G={G}"] = lambda gid=gid, G=G: eng.deciles_within(S, NR, gid, G, nb)
        calls[f"labels only G={G}"] = lambda gid=gid, G=G: eng.deciles_within(S, None, gid, G, nb)
        calls[f"loop over groups G={G}"] = lambda gid2=gid2, G=G: loop(gid2, G)
        calls[f"group_stats G={G}"] = lambda gid=gid, G=G: eng.group_stats(S, gid, G)
    calls["deciles (one sort)"] = lambda: eng.deciles(S, NR, nb)
    bp = torch.rand((N,), generator=gen, device=dev) < 0.3   # a static 30 % breakpoint subset
    calls["deciles_bp"] = lambda: eng.deciles_bp(S, NR, bp, nb)
    calls["breakpoints"] = lambda: eng.breakpoints(S, bp, nb)
    # the two routes agree before they are timed
    for G in args.groups:
        a = eng.deciles_within(S, NR, gids[G], G, nb)[0]
        assert torch.equal(a, loop(gids[G].expand(T_m, N), G)), f"labels differ at G={G}"
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
        print(f"{name:28s} {med:9.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})", flush=True)
    for G in args.groups:
        ratio = res[f"group_deciles G={G}"]["ms"] / res[f"loop over groups G={G}"]["ms"]
        res[f"new / loop G={G}"] = round(ratio, 3)
        print(f"group_deciles / loop at G={G}: {ratio:.3f}")
    if len(args.groups) >= 2:
        a, b = args.groups[0], args.groups[-1]
        ratio = res[f"group_deciles G={b}"]["ms"] / res[f"group_deciles G={a}"]["ms"]
        res[f"G={b} / G={a}"] = round(ratio, 3)
        print(f"group_deciles G={b} / G={a}: {ratio:.3f}")
    print(json.dumps(dict(bench="groups", assets=N, months=T_m, bins=nb, rounds=args.rounds,
                          device=torch.cuda.get_device_name(0), results=res)))


if __name__ == "__main__":
    main()
