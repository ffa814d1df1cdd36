#!/usr/bin/env python3
"""The `--blocks sensors` block of tools/mushroom_time.py, tools/infomax_time.py and tools/rviews_time.py: what a sensor table on the
landscape set (dv_sensors_set) costs a step of the model's banked, sensed call.

    python tools/sensors_block.py mushroom|infomax|rviews [--calls 30] [--reps 5]        (one JSON line; the three tools run it as a child)

Shape: the lands block's 4 landscapes x 4 banks (routes), 32 members x 16 headings and 8 members x 60 headings at 32 x 32 views; member i
in bank i % 4 on landscape 3 i % 4.  The engine's own sensor has [2, 2] pixel blocks, 5 levels, no mask.  The same poses are stepped
in alternating windows of one process, microseconds per step by a hipEvent pair, medians (and the spread) of --reps windows of --calls
steps:

  no_table_us_per_step      the set without a table: the kernels as they were before sensor tables (their code is untouched)
  equal_table_us_per_step   a table of four entries that all equal the engine's own sensor: the same pixels fetched per pose, so the
                            ratio equal_over_no_table is what reading the table costs; the rows are checked to be the no-table bits
  four_table_us_per_step    a table of four different entries, pixel blocks (1, 2), (2, 4), (3, 2), (2, 2) with their own levels and
                            masks: a pose's work is its entry's own pw * ph block (2, 8, 6 and 4 landscape pixels a sensor pixel
                            against 4 everywhere), so four_over_no_table has no mark to meet

A window without a GPU fails; nothing here falls back."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "navigation-by-deja-vu_amd"))
sys.path.insert(0, ROOT)

SIDE = 32
ENSEMBLES = ((32, 16), (8, 60))                                   # (members, headings)
N_BANKS = 4
LAND_SHAPES = ((600, 600), (560, 600), (600, 540), (600, 600))     # rows, cols: the poses lie inside all of them under every entry
OWN = dict(pixel=(2, 2), levels=5, mask=0)
FOUR = (dict(pixel=(1, 2), levels=5, mask=0), dict(pixel=(2, 4), levels=4, mask=1), dict(pixel=(3, 2), levels=256, mask=2),
        dict(pixel=(2, 2), levels=3, mask=1))
MB = dict(n_kc=20000, fan_in=10, n_active=200)
ROUTE_VIEWS = 50


def spread(samples):
    return dict(median=round(float(np.median(samples)), 3), min=round(float(min(samples)), 3), max=round(float(max(samples)), 3))


def measure(model, n_calls, reps):
    import copy
    import navsim_amd
    from navsim_amd import synth
    lands = [np.ascontiguousarray(synth.synth_landscape(3 + l, 600, 4)[:r, :c]) for l, (r, c) in enumerate(LAND_SHAPES)]
    L = len(lands)
    N = SIDE * SIDE
    out = dict(model=model, side=SIDE, n_banks=N_BANKS, n_lands=L, land_shapes=LAND_SHAPES, calls_per_window=n_calls, windows=reps,
               own_sensor=OWN, four_entries=FOUR, layouts=[])
    plug = dict(mushroom=lambda: navsim_amd.mushroom_familiarity(), infomax=lambda: navsim_amd.infomax_familiarity(learning_rate=1e-3),
                rviews=lambda: navsim_amd.sads_familiarity(0.25))[model]

    def table(entries, agent):
        luts = []
        for e in entries:
            probe = copy.copy(agent)
            probe.n_sensor_levels = (256, 256, e["levels"])
            luts.append(probe._level_tables())
        return [e["pixel"] for e in entries], np.stack(luts), [e["mask"] for e in entries]

    for n, A in ENSEMBLES:
        agent = navsim_amd.NavBySceneFamiliarity(lands[0], (SIDE, SIDE), 1.0, n_test_angles=A, sensor_pixel_dimensions=list(OWN["pixel"]),
                                                 n_sensor_levels=OWN["levels"], mask_middle_n=OWN["mask"], familiarity_model=plug())
        eng = agent._engine                                       # (landscape and sensor attached)
        eng.lands_set(lands)
        rng = np.random.default_rng(n * 100 + A)
        xs, ys = rng.uniform(150, 390, n), rng.uniform(150, 390, n)
        angs = (rng.uniform(0, 2 * np.pi, n)[:, None] + agent.angle_offsets[None, :]) % (2 * np.pi)
        banks = (np.arange(n) % N_BANKS).astype(np.int32)
        land_of = (3 * np.arange(n) % L).astype(np.int32)
        # four routes of ROUTE_VIEWS views, route r on landscape r, trained (or stored) without a table
        tx, ty, ta = rng.uniform(150, 390, L * ROUTE_VIEWS), rng.uniform(150, 390, L * ROUTE_VIEWS), rng.uniform(0, 2 * np.pi, L * ROUTE_VIEWS)
        route_of = np.repeat(np.arange(L, dtype=np.int32), ROUTE_VIEWS)
        if model == "mushroom":
            from navsim_amd.util import mushroom_connectivity
            eng.mb_begin(SIDE, SIDE, mushroom_connectivity(MB["n_kc"], N, MB["fan_in"], 0), MB["n_active"], 2)
            eng.mbank_set(N_BANKS)
            eng.mbank_train_from_poses(tx, ty, ta, route_of, want_views=False, land_of_view=route_of)
            step = lambda: eng.mbank_sense_step_batch(xs, ys, angs, banks, land_of_member=land_of)
        elif model == "infomax":
            from navsim_amd.util import infomax_initial_weights
            W0 = infomax_initial_weights(N, N, 0)
            eng.infomax_begin(SIDE, SIDE, W0, 2, 1e-3)
            eng.ibank_set(N_BANKS, W0)
            eng.ibank_train_from_poses(tx, ty, ta, route_of, want_views=False, land_of_view=route_of)
            step = lambda: eng.ibank_sense_step_batch(xs, ys, angs, banks, land_of_member=land_of)
        else:
            first = np.arange(L + 1, dtype=np.int64) * ROUTE_VIEWS
            eng.rviews_set_from_poses(tx, ty, ta, first, land_of_view=route_of, want_views=False)
            weights = np.full(n, 0.25)
            step = lambda: eng.rviews_sense_step(xs, ys, angs, banks, weights, land_of_member=land_of)
        tables = dict(no_table=None, equal_table=table([OWN] * L, agent), four_table=table(FOUR, agent))

        def window(which):
            if tables[which] is None:
                eng.sensors_clear()
            else:
                eng.sensors_set(*tables[which])
            eng.timer_start()
            for _ in range(n_calls):
                res = step()
            return eng.timer_stop() * 1e3 / n_calls, res

        rows = {k: window(k)[1] for k in tables}                  # warm-up of every form (code load, clocks, the buffers)
        assert not any(r.flags.any() for r in rows.values())
        bits = lambda r: np.ascontiguousarray(r.angle_familiarity).view(np.uint64)
        assert np.array_equal(bits(rows["equal_table"]), bits(rows["no_table"])) and not np.array_equal(bits(rows["four_table"]), bits(rows["no_table"]))
        ts = {k: [] for k in tables}
        for _ in range(reps):                                     # alternating windows
            for k in tables:
                ts[k].append(window(k)[0])
        row = dict(members=n, headings=A)
        for k in tables:
            row[k + "_us_per_step"] = spread(ts[k])
        for k in ("equal_table", "four_table"):
            row[k.replace("_table", "") + "_over_no_table"] = round(float(np.median(ts[k]) / np.median(ts["no_table"])), 3)
        out["layouts"].append(row)
        eng.close()
    return out


def run_child(limit, n_calls, reps, model):
    """The block in a process of its own under a time limit -> (status, row or None); what the three tools call."""
    import subprocess
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), model, "--calls", str(n_calls), "--reps", str(reps)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
    if p.returncode != 0:
        print("GPU measurement of the sensor tables (%s) ended with status %d: nothing more is run" % (model, p.returncode), file=sys.stderr)
        return p.returncode, None
    return 0, json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model", choices=("mushroom", "infomax", "rviews"))
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    print(json.dumps(measure(args.model, args.calls, args.reps)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
