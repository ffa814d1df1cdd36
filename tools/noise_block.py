#!/usr/bin/env python3
"""The `--blocks noise` block of tools/mushroom_time.py, tools/infomax_time.py and tools/rviews_time.py: what noise rows on the
landscape set (dv_noise_rows) cost a step of the model's banked, sensed call.

    python tools/noise_block.py mushroom|infomax|rviews [--sides 32,64] [--calls 30] [--reps 5]   (one JSON line; the three tools run it as a child)

Shape: the lands block's 4 landscapes x 4 banks (routes), 32 members x 16 headings and 8 members x 60 headings at side x side views;
member i in bank i % 4 on landscape 3 i % 4.  The engine's sensor has [1, 1] pixel blocks, 256 levels and no mask (the synthetic
landscapes' V lies on the reference's 5 levels, which an amplitude below 32 never leaves after a 5-level table).  The same poses are
stepped in alternating windows of one process, microseconds per step by a hipEvent pair, medians (and the spread) of --reps windows of
--calls steps:

  no_rows_us_per_step       no noise rows: the kernels as they were before there were rows (their code is untouched)
  zero_rows_us_per_step     rows of zero amplitude, set once before the window: the noise forms of the kernels with the draws' work and
                            the extra table read, no upload per step; the rows are checked to be the no-rows bits
  amp20_rows_us_per_step    rows of amplitude 20 on S and V, set once before the window
  fresh_rows_us_per_step    rows of amplitude 20 set again before EVERY step under new keys, as a route ensemble sets them (a member's
                            key counts its steps): the rows' check and upload per step on top

zero_over_no_rows, amp20_over_no_rows and fresh_over_no_rows are the ratios of the medians.  A window without a GPU fails; nothing here
falls back."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "navigation-by-deja-vu_amd"))
sys.path.insert(0, ROOT)

ENSEMBLES = ((32, 16), (8, 60))                                   # (members, headings)
N_BANKS = 4
LAND_SHAPES = ((600, 600), (560, 600), (600, 540), (600, 600))     # rows, cols: the poses lie inside all of them
MB = dict(n_kc=20000, fan_in=10, n_active=200)
ROUTE_VIEWS = 50
SEED, AMP = 11, 20


def spread(samples):
    return dict(median=round(float(np.median(samples)), 3), min=round(float(min(samples)), 3), max=round(float(max(samples)), 3))


def measure_side(model, side, n_calls, reps):
    import navsim_amd
    from navsim_amd import synth
    lands = [np.ascontiguousarray(synth.synth_landscape(3 + l, 600, 4)[:r, :c]) for l, (r, c) in enumerate(LAND_SHAPES)]
    L = len(lands)
    N = side * side
    out = dict(side=side, layouts=[])
    plug = dict(mushroom=lambda: navsim_amd.mushroom_familiarity(), infomax=lambda: navsim_amd.infomax_familiarity(learning_rate=1e-3),
                rviews=lambda: navsim_amd.sads_familiarity(0.25))[model]
    for n, A in ENSEMBLES:
        agent = navsim_amd.NavBySceneFamiliarity(lands[0], (side, side), 1.0, n_test_angles=A, n_sensor_levels=256, familiarity_model=plug())
        eng = agent._engine                                       # (landscape and sensor attached)
        eng.lands_set(lands)
        rng = np.random.default_rng(n * 100 + A)
        xs, ys = rng.uniform(150, 390, n), rng.uniform(150, 390, n)
        angs = (rng.uniform(0, 2 * np.pi, n)[:, None] + agent.angle_offsets[None, :]) % (2 * np.pi)
        banks = (np.arange(n) % N_BANKS).astype(np.int32)
        land_of = (3 * np.arange(n) % L).astype(np.int32)
        # four routes of ROUTE_VIEWS views, route r on landscape r, trained (or stored) without rows
        tx, ty, ta = rng.uniform(150, 390, L * ROUTE_VIEWS), rng.uniform(150, 390, L * ROUTE_VIEWS), rng.uniform(0, 2 * np.pi, L * ROUTE_VIEWS)
        route_of = np.repeat(np.arange(L, dtype=np.int32), ROUTE_VIEWS)
        if model == "mushroom":
            from navsim_amd.util import mushroom_connectivity
            eng.mb_begin(side, side, mushroom_connectivity(MB["n_kc"], N, MB["fan_in"], 0), MB["n_active"], 2)
            eng.mbank_set(N_BANKS)
            eng.mbank_train_from_poses(tx, ty, ta, route_of, want_views=False, land_of_view=route_of)
            step = lambda: eng.mbank_sense_step_batch(xs, ys, angs, banks, land_of_member=land_of)
        elif model == "infomax":
            from navsim_amd.util import infomax_initial_weights
            M = min(N, 1024)
            W0 = infomax_initial_weights(M, N, 0)
            eng.infomax_begin(side, side, W0, 2, 1e-3)
            eng.ibank_set(N_BANKS, W0)
            eng.ibank_train_from_poses(tx, ty, ta, route_of, want_views=False, land_of_view=route_of)
            step = lambda: eng.ibank_sense_step_batch(xs, ys, angs, banks, land_of_member=land_of)
        else:
            first = np.arange(L + 1, dtype=np.int64) * ROUTE_VIEWS
            eng.rviews_set_from_poses(tx, ty, ta, first, land_of_view=route_of, want_views=False)
            weights = np.full(n, 0.25)
            step = lambda: eng.rviews_sense_step(xs, ys, angs, banks, weights, land_of_member=land_of)
        streams = np.arange(n, dtype=np.uint64) << np.uint64(32)
        zeros, amps = np.zeros(n, dtype=np.int64), np.full(n, AMP, dtype=np.int64)
        count = [0]

        def window(which):
            if which == "no_rows":
                eng.noise_clear()
            elif which == "zero_rows":
                eng.noise_rows(SEED, streams, zeros, zeros)
            else:
                eng.noise_rows(SEED, streams, amps, amps)
            eng.timer_start()
            for _ in range(n_calls):
                if which == "fresh_rows":
                    count[0] += 1
                    eng.noise_rows(SEED, streams | np.uint64(count[0]), amps, amps)
                res = step()
            return eng.timer_stop() * 1e3 / n_calls, res

        kinds = ("no_rows", "zero_rows", "amp20_rows", "fresh_rows")
        rows = {k: window(k)[1] for k in kinds}                   # warm-up of every form (code load, clocks, the buffers)
        assert not any(r.flags.any() for r in rows.values())
        bits = lambda r: np.ascontiguousarray(r.angle_familiarity).view(np.uint64)
        assert np.array_equal(bits(rows["zero_rows"]), bits(rows["no_rows"])) and not np.array_equal(bits(rows["amp20_rows"]), bits(rows["no_rows"]))
        ts = {k: [] for k in kinds}
        for _ in range(reps):                                     # alternating windows
            for k in kinds:
                ts[k].append(window(k)[0])
        row = dict(members=n, headings=A)
        for k in kinds:
            row[k + "_us_per_step"] = spread(ts[k])
        for k in kinds[1:]:
            row[k.replace("_rows", "") + "_over_no_rows"] = round(float(np.median(ts[k]) / np.median(ts["no_rows"])), 3)
        out["layouts"].append(row)
        eng.close()
    return out


def measure(model, sides, n_calls, reps):
    return dict(model=model, n_banks=N_BANKS, n_lands=len(LAND_SHAPES), land_shapes=LAND_SHAPES, calls_per_window=n_calls, windows=reps,
                seed=SEED, amplitude=AMP, sizes=[measure_side(model, s, n_calls, reps) for s in sides])


def run_child(limit, sides, n_calls, reps, model):
    """The block in a process of its own under a time limit -> (status, row or None); what the three tools call."""
    import subprocess
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), model, "--sides", ",".join(str(s) for s in sides),
           "--calls", str(n_calls), "--reps", str(reps)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
    if p.returncode != 0:
        print("GPU measurement of the noise rows (%s) ended with status %d: nothing more is run" % (model, p.returncode), file=sys.stderr)
        return p.returncode, None
    return 0, json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model", choices=("mushroom", "infomax", "rviews"))
    ap.add_argument("--sides", default="32,64")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    print(json.dumps(measure(args.model, [int(s) for s in args.sides.split(",")], args.calls, args.reps)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
