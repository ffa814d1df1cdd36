#!/usr/bin/env python3
"""Time of reading an ensemble's scene_familiarity: ONE batched call that keeps the per-view minimum per agent
(dv_sense_step_batch_scene, 64/A agents per library pass) against one single-agent dv_sense_step(..., scene_fam) per agent for the same
poses on the same library -- the ensemble block's shape of bench.py: 32 agents x 16 headings, 100 000 views of 64x64.  The two forms
are timed in turns (interleaved), medians of --reps; the rows are checked bit for bit first.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "navigation-by-deja-vu_amd"))
import numpy as np                                   # noqa: E402
import navsim_amd                                    # noqa: E402
from navsim_amd import synth                         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=32)
    ap.add_argument("--headings", type=int, default=16)
    ap.add_argument("--views", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--seed", type=int, default=20261004)
    args = ap.parse_args()
    h = w = 64
    L = 2000
    land = synth.synth_landscape(args.seed, L, 4)
    path = synth.sin_training_path(0.5, 0.2 * L, 0.6 * L, arclen=8.0)
    nsf = navsim_amd.NavBySceneFamiliarity(land, (w, h), 0.5, n_test_angles=args.headings, n_sensor_levels=5,
                                           familiarity_model=navsim_amd.sads_familiarity(0.25), track_scene_familiarity=False)
    eng = nsf._engine
    try:
        eng.generate_library(args.seed, args.views, h, w, chem_weight=0.25)
        xs, ys, angs = [], [], []
        for i in np.linspace(5, len(path) - 5, args.agents).astype(int):
            dd = path[i + 1] - path[i]
            nsf.position = tuple(path[i] + np.array([1.0, -1.0]))
            nsf.angle = float(np.arctan2(dd[1], dd[0]) % (2 * np.pi))
            x, y, a = nsf.headings_to_test()
            xs.append(x); ys.append(y); angs.append(a)
        angs = np.stack(angs)

        def singles():
            return [eng.sense_step(xs[i], ys[i], angs[i], want_scene=True)["scene_familiarity"] for i in range(args.agents)]

        def batched():
            return eng.sense_step_batch_scene(xs, ys, angs).scene_familiarity

        for _ in range(3):                           # the first calls time the kernel forms and allocate the row buffers
            rows, ones = batched(), singles()
        for i in range(args.agents):
            if rows[i].tobytes() != ones[i].tobytes():
                raise RuntimeError("row %d of the batched call differs from the single-agent step" % i)
        tb, ts = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            batched()
            t1 = time.perf_counter()
            singles()
            t2 = time.perf_counter()
            tb.append(t1 - t0)
            ts.append(t2 - t1)
        mb, ms = float(np.median(tb)) * 1e3, float(np.median(ts)) * 1e3
        print(json.dumps(dict(agents=args.agents, headings=args.headings, views=args.views, reps=args.reps,
                              batched_scene_ms=mb, single_calls_ms=ms, ratio_single_over_batched=ms / mb)))
    finally:
        eng.close()


if __name__ == "__main__":
    main()
