#!/usr/bin/env python3
"""Time csm_month_stats / csm_window_signals (rules D1..D6) against k_signal on the same panel,
in one process.

csm_month_stats and the streaming k_signal (csm_tune "signal_tail" 0) both read every day row
of the panel once (8 B per asset-day), so the streaming k_signal on the same box, back to back,
is the yardstick; the default tail-first signal is timed for context.  Workload: the C4 panel
(100,000 assets x 10,000 business days from 1985-01-01, csmom.synth.make_device_panel); run it
with --assets 5000 --days 6522 for the C2 / C3 width.  HIP events around each call, the calls
interleaved round by round, median and range over the rounds.  Prints one line per call: ms,
8 N T_d / time in TB/s, and the ratio to the streaming k_signal's time.

    python scripts/bench_signals.py [--assets N] [--days T] [--rounds R] [--warmup W]
                                    [--chunks C [C ...]]
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
    ap.add_argument("--chunks", type=int, nargs="*", default=[],
                    help="also time csm_month_stats with stats_chunks forced to these values")
    args = ap.parse_args()

    import torch

    import csmom
    from csmom.synth import bday_calendar, make_device_panel

    if not torch.cuda.is_available():
        sys.exit("bench_signals.py needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    eng = csmom.Engine(0)
    lib = eng.lib
    N, T_d = args.assets, args.days
    days, ms_host, _ = bday_calendar("1985-01-01", T_d)
    panel = make_device_panel(N, days, ms_host, seed=args.seed, device=dev)
    P, ms = panel.P, panel.month_start
    T_m = len(ms_host) - 1
    mmd, _ = eng.month_days(ms)

    def tuned(key, value, default, fn):
        def call():
            lib.csm_tune(key, value)
            try:
                fn()
            finally:
                lib.csm_tune(key, default)
        return call

    sig_out = (None, None, eng.empty((T_m, N)), eng.empty((T_m, N)))
    signal = lambda: eng.signal(P, ms, mmd, 12, 1, out=sig_out)   # noqa: E731
    st_out = tuple(eng.empty((T_m, N)) for _ in range(4)) + (eng.empty((T_m, N), torch.int32),)
    stats = lambda: eng.month_stats(P, ms, mmd, out=st_out)       # noqa: E731
    st = eng.month_stats(P, ms, mmd)
    M = eng.momentum(st.PM, 12, 1)[1]
    calls = {"k_signal stream": tuned(b"signal_tail", 0, 2, signal),
             "k_signal default": signal,
             "month_stats": stats}
    for c in args.chunks:
        calls[f"month_stats c={c}"] = tuned(b"stats_chunks", c, 0, stats)
    calls["window_signals"] = lambda: eng.window_signals(*st, M=M)
    calls["window H52 only"] = lambda: eng.window_signals(*st, outputs=("H52", "NR_H52"))
    calls["run high52"] = lambda: eng.run_signal(P, ms, "high52")
    calls["run mom_vol"] = lambda: eng.run_signal(P, ms, "mom_vol")
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
    ref = statistics.median(times["k_signal stream"])
    res = {}
    for name, ts in times.items():
        med = statistics.median(ts)
        res[name] = dict(ms=round(med, 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4),
                         tb_per_s=round(bytes_read / (med * 1e-3) / 1e12, 3),
                         ratio_to_k_signal_stream=round(med / ref, 3))
        print(f"{name:18s} {med:8.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})  "
              f"{res[name]['tb_per_s']:.2f} TB/s of 8 N T_d  {med / ref:.2f} x k_signal stream",
              flush=True)
    print(json.dumps(dict(bench="signals", assets=N, days=T_d, months=T_m, rounds=args.rounds,
                          device=torch.cuda.get_device_name(0), results=res)))


if __name__ == "__main__":
    main()
