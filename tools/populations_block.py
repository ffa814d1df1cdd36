#!/usr/bin/env python3
"""The populations block of tools/mushroom_time.py (--blocks populations): what a mushroom-body population table costs and what it
saves.  Same method as the banks and sensors blocks: 4 banks, 32 members x 16 headings and 8 members x 60 headings (member i in bank
i % 4), sides 32 and 64, medians of --reps alternating windows of --calls steps in ONE process, hipEvent pairs around a window.

The reference of every ratio is the banked step WITHOUT a table (dv_mbank_sense_step on dv_mbank_set(4) behind the model's own
20000 x 10 wiring) at the same poses in the same run.  Per side and layout:
  (a) same_as_model   a table of four populations equal to the model's (one per bank, each with its own copy of the wiring): what the
                      table itself costs; shared_by_four is the same four banks behind ONE population of the table, which leaves the
                      descriptor read alone and takes the four copies' cache footprint out
  (b) four_wirings    four populations of the model's size with wirings of their own (seeds 1..4)
  (c) three_sizes     5000 / 20000 / 80000 cells (n_active 1 %) in one table of three banks, member i in bank i % 3, against the
                      same members as three engines stepped in turn, each begun with one population and stepping its own members
and per side
  (d) train           one banked training call over four populations (the wirings of (b), --views views each), against four engines
                      with one dv_mb_train_from_poses call each
Not split further: a window's time is host and device together (table check, upload when it changed, launches, the one wait)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "navigation-by-deja-vu_amd"))
sys.path.insert(0, ROOT)

ENSEMBLES = ((32, 16), (8, 60))                                   # (members, headings)
K, FAN_IN, SPARSITY = 20000, 10, 0.01
N_BANKS = 4
SIZES = (5000, 20000, 80000)


def spread(samples):
    return dict(median=round(float(np.median(samples)), 3), min=round(float(min(samples)), 3), max=round(float(max(samples)), 3))


def measure(side, n_views, n_calls, reps):
    from navsim_amd import NavBySceneFamiliarity, mushroom_familiarity, synth
    from navsim_amd.util import mushroom_population
    N = side * side
    land = synth.synth_landscape(3, 600, 4)
    out = dict(side=side, N=N, n_kc=K, fan_in=FAN_IN, n_banks=N_BANKS, sizes=list(SIZES), calls_per_window=n_calls, views_per_route=n_views,
               layouts=[])
    own = mushroom_population(N, K, FAN_IN, SPARSITY, 0)
    wirings = [mushroom_population(N, K, FAN_IN, SPARSITY, seed) for seed in range(1, N_BANKS + 1)]
    sizes = [mushroom_population(N, k, FAN_IN, SPARSITY, 10 + j) for j, k in enumerate(SIZES)]

    def agent_engine(A):
        return NavBySceneFamiliarity(land, (side, side), 1.0, n_test_angles=A, familiarity_model=mushroom_familiarity())._engine

    def begin(eng, pop):
        eng.mb_begin(side, side, pop["conn"], pop["n_active"], pop["channel"])

    for n, A in ENSEMBLES:
        eng = agent_engine(A)
        lone = [agent_engine(A) for _ in SIZES]
        rng = np.random.default_rng(n * 100 + A)
        xs, ys = rng.uniform(150, 450, n), rng.uniform(150, 450, n)
        offsets = np.linspace(-np.pi / 2, np.pi / 2, A)
        angs = (rng.uniform(0, 2 * np.pi, n)[:, None] + offsets[None, :]) % (2 * np.pi)
        mid = angs[:, A // 2].copy()
        banks4 = (np.arange(n) % N_BANKS).astype(np.int32)
        banks3 = (np.arange(n) % len(SIZES)).astype(np.int32)
        each = list(range(N_BANKS))
        tables = {"no_table": None, "shared_by_four": ([own], [0] * N_BANKS, banks4), "same_as_model": ([own] * N_BANKS, each, banks4),
                  "four_wirings": (wirings, each, banks4), "three_sizes": (sizes, list(range(len(SIZES))), banks3)}

        def install(which):
            """(some weights at 0 in every bank, as on trained routes)"""
            begin(eng, own)
            if tables[which] is None:
                eng.mbank_set(N_BANKS)
                banks = banks4
            else:
                pops, of_bank, banks = tables[which]
                eng.mbpop_set(pops, of_bank)
            eng.mbank_train_from_poses(xs, ys, mid, banks, want_views=False)
            return banks

        def window(banks):
            eng.timer_start()
            for _ in range(n_calls):
                res = eng.mbank_sense_step_batch(xs, ys, angs, banks)
            return eng.timer_stop() * 1e3 / n_calls, res          # us per ensemble step

        members = [np.flatnonzero(banks3 == j) for j in range(len(SIZES))]
        for j, e in enumerate(lone):
            begin(e, sizes[j])
            e.mb_train_from_poses(xs[members[j]], ys[members[j]], mid[members[j]], want_views=False)

        def in_turn():
            t = 0.0
            for j, e in enumerate(lone):
                e.timer_start()
                for _ in range(n_calls):
                    e.mb_sense_step_batch(xs[members[j]], ys[members[j]], angs[members[j]])
                t += e.timer_stop() * 1e3 / n_calls
            return t

        # The table changes between windows (one engine, one process), so a window begins with its table installed and one untimed
        # step; every case is installed as often as every other.
        times = {which: [] for which in tables}
        times["three_engines_in_turn"] = []
        for rep in range(reps + 1):                               # (the first round is the warm-up: code load, clocks, the buffers)
            for which in tables:
                banks = install(which)
                _, res = window(banks)
                assert not res.flags.any() and res.angle_familiarity.max() == 0.0 and res.angle_familiarity.min() < 0
                t, _ = window(banks)
                if rep:
                    times[which].append(t)
            t = in_turn()
            if rep:
                times["three_engines_in_turn"].append(t)
        med = {which: float(np.median(v)) for which, v in times.items()}
        row = dict(members=n, headings=A)
        for which, v in times.items():
            row[which + "_us_per_step"] = spread(v)
        for which in ("shared_by_four", "same_as_model", "four_wirings", "three_sizes", "three_engines_in_turn"):
            row[which + "_over_no_table"] = round(med[which] / med["no_table"], 3)
        row["three_engines_over_one_table"] = round(med["three_engines_in_turn"] / med["three_sizes"], 3)
        out["layouts"].append(row)
        eng.close()
        for e in lone:
            e.close()
    # (d) training: four populations in one banked call on one engine, against one call per population on an engine each
    engines = [agent_engine(ENSEMBLES[0][1]) for _ in range(N_BANKS)]
    rng = np.random.default_rng(side + 7)
    total = N_BANKS * n_views
    xs, ys, angs = rng.uniform(150, 450, total), rng.uniform(150, 450, total), rng.uniform(0, 2 * np.pi, total)
    bank_of = np.repeat(np.arange(N_BANKS, dtype=np.int32), n_views)

    def one_call():
        eng = engines[0]
        begin(eng, own)
        eng.mbpop_set(wirings, list(range(N_BANKS)))
        eng.timer_start()
        eng.mbank_train_from_poses(xs, ys, angs, bank_of, want_views=False)
        return eng.timer_stop() * 1e3

    def call_per_population():
        t = 0.0
        for r, eng in enumerate(engines):
            begin(eng, wirings[r])
            sl = slice(r * n_views, (r + 1) * n_views)
            eng.timer_start()
            eng.mb_train_from_poses(xs[sl], ys[sl], angs[sl], want_views=False)
            t += eng.timer_stop() * 1e3
        return t

    one_call()
    zeros = engines[0].mbank_info()["n_depressed"].tolist()
    call_per_population()
    assert zeros == [e.mb_info()["n_depressed"] for e in engines] and all(0 < z <= K for z in zeros)
    t1, t4 = [], []
    for _ in range(reps):
        t1.append(one_call())
        t4.append(call_per_population())
    out["train"] = dict(populations=N_BANKS, views_per_population=n_views, one_banked_call_us=spread(t1), call_per_population_us=spread(t4),
                        per_population_over_banked=round(float(np.median(t4) / np.median(t1)), 3), n_depressed=zeros)
    for e in engines:
        e.close()
    return out


def run_child(limit, side, n_views, n_calls, reps):
    """One side in a process of its own under a time limit -> (status, row or None)."""
    import subprocess
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), str(side), "--views", str(n_views), "--calls", str(n_calls),
           "--reps", str(reps)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
    if p.returncode != 0:
        print("GPU measurement of the population tables of side %d ended with status %d: nothing more is run" % (side, p.returncode), file=sys.stderr)
        return p.returncode, None
    return 0, json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("side", type=int)
    ap.add_argument("--views", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    print(json.dumps(measure(args.side, args.views, args.calls, args.reps)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
