#!/usr/bin/env python3
"""Time csm_range_sums / csm_range_model (rules HL1..HL6) and run_signal("cs_spread") against
csm_liq_sums on the same panel, in one process.

csm_liq_sums walks two daily panels with the same trips and month flushes (16 B per asset-day
against 24 B here), so k_liq_sums on the same box, back to back, is the yardstick: 3/2 of its time
is the bandwidth-proportional figure.  What k_range_sums adds on top is arithmetic: three logs a
ranged day, and a pair's two logs, exp, three square roots and three divisions.  Workload: the C4
panel (100,000 assets x 10,000 business days from 1985-01-01, csmom.synth.make_device_panel) as the
close, H = C exp(sigma |z1|) and L = C exp(-sigma |z2|) rounded to cents from a seeded generator
(sigma 1.5 %, about 1 % NaN in each), and bench_liq.py's volume panel for the yardstick; run it
with --assets 5000 --days 6522 for the C2 / C3 width.  HIP events around each call, the calls
interleaved round by round, median and range over the rounds.  Prints one line per call: ms,
24 N T_d / time in GB/s (16 N T_d for liq_sums), and the ratio to k_liq_sums's time.

    python scripts/bench_range.py [--assets N] [--days T] [--rounds R] [--warmup W]
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
sys.path.insert(0, str(Path(__file__).resolve().parent))


def range_panels(C, seed, sigma=0.015, block_days=512):
    """(H, L) [T_d][N] around the close panel C, built in HBM block by block."""
    import torch
    g = torch.Generator(device=C.device)
    g.manual_seed(int(seed) * 37 + 11)
    H, L = torch.empty_like(C), torch.empty_like(C)
    for d0 in range(0, C.shape[0], block_days):
        c = C[d0:d0 + block_days]
        for X, sign in ((H, 1.0), (L, -1.0)):
            z = torch.randn(c.shape, generator=g, dtype=torch.float64, device=C.device).abs_()
            x = ((c * torch.exp(sign * sigma * z)) * 100.0).round_() / 100.0
            u = torch.rand(c.shape, generator=g, dtype=torch.float64, device=C.device)
            x[u < 0.01] = float("nan")
            X[d0:d0 + block_days] = x
    return H, L


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--assets", type=int, default=100_000)
    ap.add_argument("--days", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--sums-chunks", type=int, nargs="*", default=[],
                    help="also time csm_range_sums with rsums_chunks forced to these values")
    ap.add_argument("--model-chunks", type=int, nargs="*", default=[],
                    help="also time csm_range_model with rmodel_chunks forced to these values")
    args = ap.parse_args()

    import torch

    import csmom
    from bench_liq import volume_panel
    from csmom.synth import bday_calendar, make_device_panel

    if not torch.cuda.is_available():
        sys.exit("bench_range.py needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    eng = csmom.Engine(0)
    lib = eng.lib
    N, T_d = args.assets, args.days
    days, ms_host, _ = bday_calendar("1985-01-01", T_d)
    panel = make_device_panel(N, days, ms_host, seed=args.seed, device=dev)
    C, ms = panel.P, panel.month_start
    H, L = range_panels(C, args.seed)
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

    def rsums(**kw):
        return lambda: eng.range_sums(H, L, C, ms, max_month_days=mmd, **kw)

    sums = rsums()()
    share = {k: float(getattr(sums, k).sum()) / (N * T_d) for k in ("NRG", "NPR", "NCS")}
    model1 = lambda: eng.range_model(sums, 1)                           # noqa: E731
    model12 = lambda: eng.range_model(sums, 12)                         # noqa: E731
    calls = {"liq_sums": lambda: eng.liq_sums(C, V, ms, max_month_days=mmd),
             "range_sums": rsums(),
             "range_sums cs off": rsums(with_cs=False),
             "range_sums ar off": rsums(with_ar=False),
             "range_sums cs, ar off": rsums(with_cs=False, with_ar=False)}
    for c in args.sums_chunks:
        calls[f"range_sums c={c}"] = tuned({b"rsums_chunks": c}, rsums())
    calls["range_model Wm=1"] = model1
    calls["range_model Wm=12"] = model12
    for c in args.model_chunks:
        calls[f"range_model Wm=1 c={c}"] = tuned({b"rmodel_chunks": c}, model1)
        calls[f"range_model Wm=12 c={c}"] = tuned({b"rmodel_chunks": c}, model12)
    calls["run cs_spread"] = lambda: eng.run_signal(C, ms, "cs_spread", HLC=(H, L, C))
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
    ref = statistics.median(times["liq_sums"])
    res = {}
    print(f"--- {N} assets x {T_d} days ({T_m} months); of the asset-days "
          f"{share['NRG']:.3f} ranged, {share['NPR']:.3f} in a pair, {share['NCS']:.3f} with a "
          f"spread", flush=True)
    for name, ts in times.items():
        med = statistics.median(ts)
        per = 16.0 if name == "liq_sums" else 24.0
        res[name] = dict(ms=round(med, 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4),
                         gb_per_s=round(per * N * T_d / (med * 1e-3) / 1e9, 1),
                         ratio_to_liq_sums=round(med / ref, 3))
        print(f"{name:32s} {med:8.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})  "
              f"{res[name]['gb_per_s']:8.1f} GB/s of {per:.0f} N T_d  {med / ref:.2f} x liq_sums",
              flush=True)
    print(json.dumps(dict(bench="range", assets=N, days=T_d, months=T_m, rounds=args.rounds,
                          device=torch.cuda.get_device_name(0), shares=share, results=res)))


if __name__ == "__main__":
    main()
