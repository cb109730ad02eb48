#!/usr/bin/env python3
"""Time csm_signal_ids with the streaming kernel ("signal_tail" 0) against the tail-first kernel
("signal_tail" 2, auto) on C4-shaped panels, in one process.

Panels (csmom.synth.make_device_panel, 100,000 assets x 10,000 business days from 1985-01-01):
  default  the generator's defaults (bench.py's C4 panel);
  gappy    late=0.5, delist=0.5: half the assets listed late, half delisted (gaps everywhere);
  full     no gap at all (late = delist = nan_day = nan_month = absent_month = 0).
HIP events around each call, the settings interleaved round by round, median and range over
the rounds; the range of the knob-0 repeats is the noise a difference has to clear.  --extra
adds settings, as name=knob:value[,knob:value...] (e.g. always=signal_tail:1).  Every setting's
M / NR / ids are compared with the knob-0 result (exact) before timing.

    python scripts/bench_signal_tail.py [--assets N] [--days T] [--rounds R] [--warmup W]
                                        [--panels default,gappy,full] [--extra ...]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

PANELS = {
    "default": {},
    "gappy": dict(late=0.5, delist=0.5),
    "full": dict(late=0.0, delist=0.0, nan_day=0.0, nan_month=0.0, absent_month=0.0),
    "absent30": dict(absent_month=0.3),   # (not in the default list) 30 % of the cells absent at random
}
DEFAULTS = dict(signal_tail=2, signal_vec=2)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--assets", type=int, default=100_000)
    ap.add_argument("--days", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--panels", default="default,gappy,full")
    ap.add_argument("--extra", nargs="*", default=[])
    args = ap.parse_args()

    import torch

    import csmom
    from csmom.synth import bday_calendar, make_device_panel

    if not torch.cuda.is_available():
        sys.exit("bench_signal_tail.py needs a GPU: there is no CPU path to time")
    settings = {"tail0": dict(signal_tail=0), "tail2": dict(signal_tail=2)}
    for spec in args.extra:
        name, kv = spec.split("=", 1)
        settings[name] = {k: int(v) for k, v in (p.split(":") for p in kv.split(","))}
    dev = torch.device("cuda", 0)
    eng = csmom.Engine(0)

    def tune(kn):
        for k, v in {**DEFAULTS, **kn}.items():
            if eng.lib.csm_tune(k.encode(), int(v)) != 0:
                sys.exit(f"csm_tune({k}, {v}) refused")

    N, T_d = args.assets, args.days
    days, ms_host, _ = bday_calendar("1985-01-01", T_d)
    T_m = len(ms_host) - 1
    results = {}
    try:
        for pname in args.panels.split(","):
            panel = make_device_panel(N, days, ms_host, seed=args.seed, device=dev, **PANELS[pname])
            P, ms = panel.P, panel.month_start
            mmd, mnd = eng.month_days(ms)
            out = (None, None, eng.empty((T_m, N)), eng.empty((T_m, N)),
                   eng.empty((T_m, N), torch.int16))
            ref = None
            for name, kn in settings.items():   # same bits first
                tune(kn)
                eng.signal_ids(P, ms, mmd, 12, 1, out=out, min_month_days=mnd)
                torch.cuda.synchronize()
                if ref is None:
                    ref = [t.clone() for t in out[2:]]
                else:
                    for a, b in zip(out[2:], ref):
                        if not torch.equal(a.view(torch.int16), b.view(torch.int16)):
                            sys.exit(f"{pname}/{name}: differs from signal_tail 0")
            del ref
            times = {k: [] for k in settings}
            for r in range(args.warmup + args.rounds):
                for name, kn in settings.items():
                    tune(kn)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    eng.signal_ids(P, ms, mmd, 12, 1, out=out, min_month_days=mnd)
                    e1.record()
                    e1.synchronize()
                    if r >= args.warmup:
                        times[name].append(e0.elapsed_time(e1))
            base = statistics.median(times["tail0"])
            spread = max(times["tail0"]) - min(times["tail0"])
            res = {}
            for name, ts in times.items():
                med = statistics.median(ts)
                res[name] = dict(ms=round(med, 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4),
                                 ratio_to_tail0=round(med / base, 3))
                print(f"{pname:8s} {name:10s} {med:8.4f} ms (min {min(ts):.4f}, max {max(ts):.4f})  "
                      f"{med / base:.3f} x tail0   [tail0 spread {spread:.4f} ms]", flush=True)
            results[pname] = dict(tail0_spread_ms=round(spread, 4), settings=res)
            del panel, P, out
            torch.cuda.empty_cache()
    finally:
        tune({})
    print(json.dumps(dict(bench="signal_tail", assets=N, days=T_d, months=T_m, rounds=args.rounds,
                          device=torch.cuda.get_device_name(0), results=results)))


if __name__ == "__main__":
    main()
