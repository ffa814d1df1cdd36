#!/usr/bin/env python3
"""Per-agent chem_weight on the ensemble workload of tools/bench_ensemble.py (32 agents x 16 headings, 100 000 views of 64x64,
patches sensed on the device), in ms per ensemble step:

  uniform            32 agents, one weight, the unweighted call (dv_sense_step_batch)
  uniform_weighted   the same agents, the weighted call with every weight equal to the library's
  four_weights       eight starts x four weights (0, 0.25, 0.5, 1) in ONE weighted call on one library laid out for [0, 1]
  four_engines       the alternative without per-agent weights: four engines, each with the library ingested at one weight (its
                     own layout), eight agents each, stepped one after the other

The forms alternate within each of `rounds` rounds, so that the spread between rounds shows beside the differences.  Also the
library's HBM in each case (bytes of the byte tiles and of the bit-plane copy).

    python tools/bench_ensemble_weights.py [rounds] [steps]"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "navigation-by-deja-vu_amd"))
import navsim_amd                     # noqa: E402
from navsim_amd import synth          # noqa: E402

H = W = 64
A, N_VIEWS, SEED, N_STARTS = 16, 100000, 20261004, 8
WEIGHTS = (0.0, 0.25, 0.5, 1.0)


def lib_bytes(eng):
    info = eng.library_info()
    return int(info["tile_bytes"]) + int(info["bit_tile_bytes"])


def starts(nsf, n):
    L = nsf.landscape.shape[0]
    path = synth.sin_training_path(0.5, 0.2 * L, 0.6 * L, arclen=8.0)
    xs, ys, angs = [], [], []
    for i in np.linspace(5, len(path) - 5, n).astype(int):
        dd = path[i + 1] - path[i]
        nsf.position = tuple(path[i] + np.array([1.0, -1.0]))
        nsf.angle = float(np.arctan2(dd[1], dd[0]) % (2 * np.pi))
        x, y, a = nsf.headings_to_test()
        xs.append(x); ys.append(y); angs.append(a)
    return np.array(xs), np.array(ys), np.stack(angs)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    land = synth.synth_landscape(SEED, 2000, 4)

    def agent():
        return navsim_amd.NavBySceneFamiliarity(land, (W, H), 0.5, n_test_angles=A, n_sensor_levels=5,
                                                familiarity_model=navsim_amd.sads_familiarity(0.25), track_scene_familiarity=False)
    main_agent = agent()
    eng = main_agent._engine
    eng.set_weight_range(0.0, 1.0)
    eng.generate_library(SEED, N_VIEWS, H, W, chem_weight=0.25)
    xs8, ys8, an8 = starts(main_agent, N_STARTS)
    xs = np.repeat(xs8, len(WEIGHTS)); ys = np.repeat(ys8, len(WEIGHTS)); an = np.repeat(an8, len(WEIGHTS), axis=0)
    w4 = np.tile(np.array(WEIGHTS), N_STARTS)
    w_uni = np.full(len(xs), 0.25)
    others = []
    for cw in WEIGHTS:                              # the four-engine alternative: a library per weight, each in its own layout
        a = agent()
        a._engine.generate_library(SEED, N_VIEWS, H, W, chem_weight=cw)
        others.append(a)
    forms = {
        "uniform": lambda: eng.sense_step_batch(xs, ys, an),
        "uniform_weighted": lambda: eng.sense_step_batch(xs, ys, an, chem_weights=w_uni),
        "four_weights": lambda: eng.sense_step_batch(xs, ys, an, chem_weights=w4),
        "four_engines": lambda: [o._engine.sense_step_batch(xs8, ys8, an8) for o in others],
    }
    # the weighted call's records equal each weight's own engine's (same views, same sums, same weight)
    got = eng.sense_step_batch(xs, ys, an, chem_weights=w4)
    for k, o in enumerate(others):
        ref = o._engine.sense_step_batch(xs8, ys8, an8)
        for s in range(N_STARTS):
            r = got[s * len(WEIGHTS) + k]
            if (r["best_idex"], r["best_view"]) != (ref[s]["best_idex"], ref[s]["best_view"]):
                raise RuntimeError("weight %g, start %d: %r != %r" % (WEIGHTS[k], s, (r["best_idex"], r["best_view"]),
                                                                       (ref[s]["best_idex"], ref[s]["best_view"])))
    for f in forms.values():
        for _ in range(3):
            f()
    ms = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                f()
            ms[k].append((time.perf_counter() - t0) / steps * 1e3)
    out = dict(agents=len(xs), headings=A, views=N_VIEWS, sensor=[H, W], steps_per_round=steps,
               ms_per_ensemble_step={k: [round(x, 4) for x in v] for k, v in ms.items()},
               library_bytes=dict(one_range_library=lib_bytes(eng), four_engines=sum(lib_bytes(o._engine) for o in others)),
               kernel_form=eng.scoring_form())
    print(json.dumps(out))
    for o in others:
        o._engine.close()
    eng.close()


if __name__ == "__main__":
    main()
