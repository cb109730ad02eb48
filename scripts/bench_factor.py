#!/usr/bin/env python3
"""Time csm_factor_model / csm_daily_fsums / csm_daily_fmodel (rules MF1..MF7) at KF = 1..4
beside the single-factor csm_market_model / csm_daily_sums / csm_daily_model, in one process.

The single-factor kernels are the yardstick: the same panel, the same process, the calls
interleaved round by round.  Workloads: the C4 panel (100,000 assets x 10,000 business days from
1985-01-01, csmom.synth.make_device_panel) and the C2 / C3 width (5,000 x 6,522), one after the
other.  Factor column 0 is the panel's own equal-weight market, columns 1..3 seeded normal
series.  HIP events around each call, median and range over the rounds.  Prints one line per
call: ms, the bytes the call must move (its inputs once, its outputs once) over the time in TB/s,
and the ratio to its single-factor yardstick; then the KF = 1 ratio and the cost per added factor,
(t[KF=4] - t[KF=1]) / 3 as a share of the yardstick.  No threshold: the numbers are reported.

    python scripts/bench_factor.py [--panels NxT [NxT ...]] [--rounds R] [--warmup W]
                                   [--fm-chunks C [C ...]] [--fsums-chunks C [C ...]]
                                   [--fmodel-chunks C [C ...]] [--unaligned] [--only W [W ...]]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def bench_panel(args, eng, N, T_d):
    import torch

    from csmom.synth import bday_calendar, make_device_panel

    dev = eng.device
    lib = eng.lib
    days, ms_host, _ = bday_calendar("1985-01-01", T_d)
    panel = make_device_panel(N, days, ms_host, seed=args.seed, device=dev)
    P, ms = panel.P, panel.month_start
    T_m = len(ms_host) - 1
    mmd, _ = eng.month_days(ms)
    PM = eng.month_stats(P, ms, mmd).PM
    MKT, _ = eng.market_factor(PM)
    MKTD, _ = eng.daily_market(P)
    gen = torch.Generator(device="cpu").manual_seed(args.seed)
    F = torch.cat([MKT[:, None], (0.03 * torch.randn(T_m, 3, generator=gen,
                                                     dtype=torch.float64)).to(dev)], 1)
    FD = torch.cat([MKTD[:, None], (0.01 * torch.randn(T_d, 3, generator=gen,
                                                       dtype=torch.float64)).to(dev)], 1)
    Fk = {k: F[:, :k].contiguous() for k in (1, 2, 3, 4)}
    FDk = {k: FD[:, :k].contiguous() for k in (1, 2, 3, 4)}
    Wb = 36
    cell = 8.0 * N * T_m          # one [T_m][N] fp64 plane
    day_bytes = 8.0 * N * T_d     # the daily panel once

    def tuned(key, value, fn):
        def call():
            lib.csm_tune(key, value)
            try:
                fn()
            finally:
                lib.csm_tune(key, 0)
        return call

    calls = {}    # name -> (fn, bytes floor, yardstick name or None)
    calls["market_model"] = (lambda: eng.market_model(PM, MKT, window=Wb), cell + 4.5 * cell, None)
    calls["market_model RESMOM"] = (lambda: eng.market_model(PM, MKT, window=Wb,
                                                             outputs=("RESMOM",)), 2 * cell, None)
    for k in (1, 2, 3, 4):
        calls[f"factor_model KF={k}"] = (
            lambda k=k: eng.factor_model(PM, Fk[k], window=Wb), cell + (4.5 + k) * cell,
            "market_model")
        calls[f"factor_model KF={k} RESMOM"] = (
            lambda k=k: eng.factor_model(PM, Fk[k], window=Wb, outputs=("RESMOM",)), 2 * cell,
            "market_model RESMOM")
    for c in args.fm_chunks:
        for k in (1, 4):
            calls[f"factor_model KF={k} c={c}"] = (
                tuned(b"fm_chunks", c, lambda k=k: eng.factor_model(PM, Fk[k], window=Wb)),
                cell + (4.5 + k) * cell, "market_model")
    calls["daily_sums"] = (lambda: eng.daily_sums(P, ms, MKTD, max_month_days=mmd),
                           day_bytes + 7.5 * cell, None)
    calls["daily_sums 6 panels"] = (
        lambda: eng.daily_sums(P, ms, MKTD, max_month_days=mmd, with_sr3=False, with_rmax=False),
        day_bytes + 5.5 * cell, None)
    planes = {k: 0.5 + 2 + 2 * k + k * (k + 1) / 2 for k in (1, 2, 3, 4)}
    for k in (1, 2, 3, 4):
        calls[f"daily_fsums KF={k}"] = (
            lambda k=k: eng.daily_fsums(P, ms, FDk[k], max_month_days=mmd),
            day_bytes + planes[k] * cell, "daily_sums 6 panels")
    if args.unaligned:   # the one-asset-per-lane path: the panel through a view 8 B off 16
        flat = torch.empty(T_d * N + 1, dtype=torch.float64, device=dev)
        Pu = flat[1:].view(T_d, N)
        Pu.copy_(P)
        for k in (1, 2, 3, 4):
            calls[f"daily_fsums KF={k} one per lane"] = (
                lambda k=k: eng.daily_fsums(Pu, ms, FDk[k], max_month_days=mmd),
                day_bytes + planes[k] * cell, "daily_sums 6 panels")
    for c in args.fsums_chunks:
        for k in (1, 4):
            calls[f"daily_fsums KF={k} c={c}"] = (
                tuned(b"dfsums_chunks", c,
                      lambda k=k: eng.daily_fsums(P, ms, FDk[k], max_month_days=mmd)),
                day_bytes + planes[k] * cell, "daily_sums 6 panels")
    s1 = eng.daily_sums(P, ms, MKTD, max_month_days=mmd, with_sr3=False, with_rmax=False)
    fsk = {k: eng.daily_fsums(P, ms, FDk[k], max_month_days=mmd) for k in (1, 2, 3, 4)}
    shared = ("DBETA", "DIVOL", "NOBS")
    for Wm in (1, 12):
        # the floor counts a window's planes once (its other reads are L2 hits) plus the outputs
        calls[f"daily_model Wm={Wm}"] = (lambda Wm=Wm: eng.daily_model(s1, Wm, outputs=shared),
                                         (5.5 + 2.5) * cell, None)
        for k in (1, 2, 3, 4):
            fs = fsk[k]
            calls[f"daily_fmodel KF={k} Wm={Wm}"] = (
                lambda fs=fs, Wm=Wm: eng.daily_fmodel(fs, Wm, outputs=shared),
                (planes[k] + k + 1.5) * cell, f"daily_model Wm={Wm}")
            if k in (1, 4):
                for c in args.fmodel_chunks:
                    calls[f"daily_fmodel KF={k} Wm={Wm} c={c}"] = (
                        tuned(b"dfmodel_chunks", c,
                              lambda fs=fs, Wm=Wm: eng.daily_fmodel(fs, Wm, outputs=shared)),
                        (planes[k] + k + 1.5) * cell, f"daily_model Wm={Wm}")
    if args.only:        # the calls whose name holds one of the words, and their yardsticks
        keep = {n for n in calls if any(w in n for w in args.only)}
        keep |= {calls[n][2] for n in keep if calls[n][2]}
        calls = {n: v for n, v in calls.items() if n in keep}
    times = {k: [] for k in calls}
    for r in range(args.warmup + args.rounds):
        for name, (fn, _, _) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {}
    print(f"--- {N} assets x {T_d} days ({T_m} months), Wb = {Wb}", flush=True)
    for name, (_, floor, yard) in calls.items():
        ts = times[name]
        res[name] = dict(ms=round(med[name], 4), ms_min=round(min(ts), 4),
                         ms_max=round(max(ts), 4),
                         tb_per_s=round(floor / (med[name] * 1e-3) / 1e12, 3),
                         ratio=round(med[name] / med[yard], 3) if yard else None)
        tail = f"  {med[name] / med[yard]:.2f} x {yard}" if yard else ""
        print(f"{name:34s} {med[name]:8.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})  "
              f"{res[name]['tb_per_s']:.2f} TB/s of its floor{tail}", flush=True)
    for fam, yard in (("factor_model KF={}", "market_model"),
                      ("factor_model KF={} RESMOM", "market_model RESMOM"),
                      ("daily_fsums KF={}", "daily_sums 6 panels"),
                      ("daily_fmodel KF={} Wm=1", "daily_model Wm=1"),
                      ("daily_fmodel KF={} Wm=12", "daily_model Wm=12")):
        if fam.format(1) not in med or fam.format(4) not in med:
            continue
        t1, t4, ty = med[fam.format(1)], med[fam.format(4)], med[yard]
        res[fam.format("*")] = dict(kf1_ratio=round(t1 / ty, 3),
                                    per_added_factor=round((t4 - t1) / 3 / ty, 3))
        print(f"{fam.format('*'):34s} KF = 1 is {t1 / ty:.2f} x {yard}; each added factor "
              f"costs {(t4 - t1) / 3 / ty:.2f} x it", flush=True)
    return dict(assets=N, days=T_d, months=T_m, results=res)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--panels", nargs="*", default=["100000x10000", "5000x6522"],
                    help="assets x days of each workload")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--fm-chunks", type=int, nargs="*", default=[],
                    help="also time csm_factor_model (KF 1 and 4) with fm_chunks forced to these")
    ap.add_argument("--fsums-chunks", type=int, nargs="*", default=[],
                    help="also time csm_daily_fsums (KF 1 and 4) with dfsums_chunks forced")
    ap.add_argument("--fmodel-chunks", type=int, nargs="*", default=[],
                    help="also time csm_daily_fmodel (KF 1 and 4) with dfmodel_chunks forced")
    ap.add_argument("--unaligned", action="store_true",
                    help="also time csm_daily_fsums on an unaligned view of the panel, which "
                         "takes the one-asset-per-lane kernel")
    ap.add_argument("--only", nargs="*", default=[],
                    help="time only the calls whose name holds one of these words")
    args = ap.parse_args()

    import torch

    import csmom

    if not torch.cuda.is_available():
        sys.exit("bench_factor.py needs a GPU: there is no CPU path to time")
    eng = csmom.Engine(0)
    out = []
    for spec in args.panels:
        n, t = spec.lower().split("x")
        out.append(bench_panel(args, eng, int(n), int(t)))
        torch.cuda.empty_cache()
    print(json.dumps(dict(bench="factor", rounds=args.rounds,
                          device=torch.cuda.get_device_name(0), panels=out)))


if __name__ == "__main__":
    main()
