#!/usr/bin/env python3
"""Times the device heat equation (navsim_amd.generate_landscapes.diffuse) on GPU 0 and prints ONE JSON line.

    python tools/diffuse_time.py [--sizes 2000,500] [--steps 2000] [--sweep 96:8,96:12,64:8] [--no-series]

Per size: milliseconds (hipEvent pair around the enqueued launches, best of --reps after a warm-up run) of `steps` steps in the
plain and in the blocked form, the blocked form's tile B, steps per launch T and window side S, its bytes per cell and step
((S*S + B*B) * 8 / (B*B*T)) beside the plain form's 16, whether both forms gave the same bits, and the wall-clock seconds of a
ten-time diffuse_series up to `steps` against ten separate diffuse calls (upload, read-back and the host checks included).
--sweep S:T,... times the blocked form under other window sides / steps per launch (dv_diffuse_configure).
profiles/diffuse_time.json is this tool's line for the table of DESIGN 4."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "navigation-by-deja-vu_amd"))

from navsim_amd import generate_landscapes as G  # noqa: E402


def timed(field, steps, form, reps, window=None, steps_per_launch=None):
    """(best ms, result, info) of `steps` steps from `field` on a fresh context (DiffuseRun: the public face of dv_diffuse_*)."""
    run = G.DiffuseRun(field, window=window, steps_per_launch=steps_per_launch)
    try:
        run.advance(steps, form)                                  # warm-up (code load, clocks)
        best = None
        for _ in range(reps):
            run.restart(field)
            ms = run.timed_advance(steps, form)
            best = ms if best is None else min(best, ms)
        return best, run.read(), run.info()
    finally:
        run.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,500")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sweep", default="")
    ap.add_argument("--no-series", action="store_true")
    args = ap.parse_args()
    out = dict(steps=args.steps, sizes=[])
    for n in [int(x) for x in args.sizes.split(",")]:
        field = np.random.default_rng(n).random((n, n))
        plain_ms, plain, _ = timed(field, args.steps, "plain", args.reps)
        blocked_ms, blocked, info = timed(field, args.steps, "blocked", args.reps)
        auto_ms, auto, _ = timed(field, args.steps, "auto", args.reps)
        B, T = info["tile"], info["steps_per_launch"]
        S = B + 2 * T
        row = dict(n=n, plain_ms=round(plain_ms, 3), blocked_ms=round(blocked_ms, 3), auto_ms=round(auto_ms, 3), tile=B, steps_per_launch=T,
                   window=S, plain_bytes_per_cell_step=16, blocked_bytes_per_cell_step=round((S * S + B * B) * 8.0 / (B * B * T), 3),
                   same_bits=bool(np.array_equal(plain.view(np.uint64), blocked.view(np.uint64))
                                  and np.array_equal(plain.view(np.uint64), auto.view(np.uint64))),
                   ns_per_cell_step_plain=round(plain_ms * 1e6 / (n * n * args.steps), 5),
                   ns_per_cell_step_blocked=round(blocked_ms * 1e6 / (n * n * args.steps), 5))
        sweep = []
        for item in [x for x in args.sweep.split(",") if x]:
            s_, t_ = item.split(":")
            ms, res, inf = timed(field, args.steps, "blocked", args.reps, int(s_), int(t_))
            sweep.append(dict(window=int(s_), steps_per_launch=inf["steps_per_launch"], tile=inf["tile"], ms=round(ms, 3),
                              same_bits=bool(np.array_equal(res.view(np.uint64), plain.view(np.uint64)))))
        if sweep:
            row["sweep"] = sweep
        if not args.no_series:
            times = [args.steps * (k + 1) // 10 for k in range(10)]
            t0 = time.perf_counter()
            shots = G.diffuse_series(field, times)
            t1 = time.perf_counter()
            singles = [G.diffuse(field, t) for t in times]
            t2 = time.perf_counter()
            row.update(series_s=round(t1 - t0, 4), ten_calls_s=round(t2 - t1, 4),
                       series_same_bits=all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(shots, singles)))
        out["sizes"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
