#!/usr/bin/env python3
"""The sets block of tools/mushroom_time.py (--blocks sets): what reading one selection of firing cells out through S banks costs
(dv_mbset_sense_step) beside what the same read-out costs without it.  Same method as the banks and populations blocks: the model's
20000 x 10 wiring, 32 members x 16 headings and 8 members x 60 headings, sides 32 and 64, medians of --reps alternating windows of
--calls steps in ONE process, hipEvent pairs around a window.

4 routes: banks 0..3 are their attractive memories, banks 4..7 a second memory each (8 banks, every one trained on poses of its own).
Member i's set of S entries is banks (i % 4 + 4 j) % 8, j < S, under coefficients +1, -1 in turn.  Per side and layout, in one run:
  banked          dv_mbank_sense_step, member i under bank i % 4: one selection and one read-out a column -- the reference of the ratios
  set_S           dv_mbset_sense_step at S = 1, 2 and 8 at the same poses
  banked_xS       dv_mbank_sense_step with every member entered S times (n S members, entry j under the j-th bank of its set): what the
                  read-out of S banks costs without sets -- S sensings and S selections a column; the host's pass that would combine
                  the S rows is not in it
Ratios are medians over the windows of the per-round ratio (round r of one case over round r of the other), with their min and max.
Not split further: a window's time is host and device together (table checks, uploads when a table changed, launches, the one wait)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "navigation-by-deja-vu_amd"))
sys.path.insert(0, ROOT)

ENSEMBLES = ((32, 16), (8, 60))                                   # (members, headings)
K, FAN_IN, N_ACTIVE = 20000, 10, 200
N_ROUTES = 4
SET_SIZES = (1, 2, 8)


def spread(samples):
    return dict(median=round(float(np.median(samples)), 3), min=round(float(min(samples)), 3), max=round(float(max(samples)), 3))


def measure(side, n_views, n_calls, reps):
    from navsim_amd import NavBySceneFamiliarity, mushroom_familiarity, synth
    from navsim_amd.util import mushroom_connectivity
    N = side * side
    land = synth.synth_landscape(3, 600, 4)
    out = dict(side=side, N=N, n_kc=K, fan_in=FAN_IN, n_active=N_ACTIVE, n_routes=N_ROUTES, n_banks=2 * N_ROUTES, set_sizes=list(SET_SIZES),
               calls_per_window=n_calls, views_per_bank=n_views, layouts=[])
    conn = mushroom_connectivity(K, N, FAN_IN, 0)
    for n, A in ENSEMBLES:
        agent = NavBySceneFamiliarity(land, (side, side), 1.0, n_test_angles=A, familiarity_model=mushroom_familiarity())
        eng = agent._engine                                       # (landscape and sensor attached)
        eng.mb_begin(side, side, conn, N_ACTIVE, 2)
        eng.mbank_set(2 * N_ROUTES)
        rng = np.random.default_rng(n * 100 + A)
        xs, ys = rng.uniform(150, 450, n), rng.uniform(150, 450, n)
        angs = (rng.uniform(0, 2 * np.pi, n)[:, None] + agent.angle_offsets[None, :]) % (2 * np.pi)
        total = 2 * N_ROUTES * n_views                            # (some weights at 0 in every bank, as on trained routes)
        eng.mbank_train_from_poses(rng.uniform(150, 450, total), rng.uniform(150, 450, total), rng.uniform(0, 2 * np.pi, total),
                                   np.repeat(np.arange(2 * N_ROUTES, dtype=np.int32), n_views), want_views=False)
        sets = {S: np.array([[(i % N_ROUTES + N_ROUTES * j) % (2 * N_ROUTES) for j in range(S)] for i in range(n)], dtype=np.int32)
                for S in SET_SIZES}
        coefs = {S: np.tile(np.array([1 if j % 2 == 0 else -1 for j in range(S)], dtype=np.int32), (n, 1)) for S in SET_SIZES}

        def banked(S):
            """The banked step with every member entered S times, entry j under the j-th bank of its set."""
            bx, by, ba = np.tile(xs, S), np.tile(ys, S), np.tile(angs, (S, 1))
            bb = np.ascontiguousarray(sets[S].T.reshape(-1))

            def window():
                eng.timer_start()
                for _ in range(n_calls):
                    res = eng.mbank_sense_step_batch(bx, by, ba, bb)
                return eng.timer_stop() * 1e3 / n_calls, res      # us per ensemble step
            return window

        def set_step(S):
            def window():
                eng.timer_start()
                for _ in range(n_calls):
                    res = eng.mbset_sense_step_batch(xs, ys, angs, sets[S], coefs[S])
                return eng.timer_stop() * 1e3 / n_calls, res
            return window

        cases = {"banked": banked(1)}
        for S in SET_SIZES:
            cases["set_%d" % S] = set_step(S)
            if S > 1:
                cases["banked_x%d" % S] = banked(S)
        times = {name: [] for name in cases}
        for rep in range(reps + 1):                               # (the first round is the warm-up: code load, clocks, the buffers)
            for name, window in cases.items():
                t, res = window()
                assert not res.flags.any()
                if rep:
                    times[name].append(t)
        # the read-outs agree: S = 1 is the banked step's bits, and the set's novelties are the S banked entries' rows
        one = cases["set_1"]()[1]
        assert np.array_equal(one.angle_familiarity, cases["banked"]()[1].angle_familiarity)
        for S in SET_SIZES[1:]:
            rows = -cases["banked_x%d" % S]()[1].angle_familiarity.reshape(S, n, A)
            assert np.array_equal(cases["set_%d" % S]()[1].bank_novelty, np.moveaxis(rows, 0, 2).astype(np.int32))
        row = dict(members=n, headings=A)
        for name, v in times.items():
            row[name + "_us_per_step"] = spread(v)

        def ratio(a, b):
            return spread([x / y for x, y in zip(times[a], times[b])])
        for S in SET_SIZES:
            row["set_%d_over_banked" % S] = ratio("set_%d" % S, "banked")
            if S > 1:
                row["banked_x%d_over_banked" % S] = ratio("banked_x%d" % S, "banked")
                row["set_%d_over_banked_x%d" % (S, S)] = ratio("set_%d" % S, "banked_x%d" % S)
        out["layouts"].append(row)
        eng.close()
    return out


def run_child(limit, side, n_views, n_calls, reps):
    """One side in a process of its own under a time limit -> (status, row or None)."""
    import subprocess
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), str(side), "--views", str(n_views), "--calls", str(n_calls),
           "--reps", str(reps)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
    if p.returncode != 0:
        print("GPU measurement of the bank sets of side %d ended with status %d: nothing more is run" % (side, p.returncode), file=sys.stderr)
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
