#!/usr/bin/env python3
"""The networks block of tools/infomax_time.py (--blocks networks): what an Infomax network table costs and what it saves.  Same
method as the banks and sensors blocks: 4 banks, 32 members x 16 headings and 8 members x 60 headings (member i in bank i % 4), sides
32 and 64 (N = side^2, the model's n_hidden = N), medians of --reps alternating windows of --calls steps in ONE process, hipEvent
pairs around a window.

The reference of every ratio is the banked step WITHOUT a table (dv_ibank_sense_step on dv_ibank_set(4) of the model's own N x N
weights) at the same poses in the same run.  Per side and layout:
  (a) same_as_model   a table of four networks equal to the model's (one per bank): what the table itself costs -- the descriptor read,
                      the ragged addresses, the bank's own row tiles in the decision
  (b) four_rates      four networks of the model's shape with learning rates of their own (the step does not read the rate: the
                      figure is (a)'s again, on weights trained at four rates)
  (c) three_sizes     n_hidden = N/4, N and 2N in one table of three banks, member i in bank i % 3 (grids sized for 2N; a workgroup
                      past its bank's rows leaves at once), against the same members as three engines stepped in turn, each begun
                      with one network and stepping its own members
and per side
  (d) train           one banked training call over four networks (the rates of (b), --views sensed views each), against four engines
                      with one dv_infomax_train_from_poses call each
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
N_BANKS = 4
RATES = (1e-3, 5e-4, 2.5e-4, 1.25e-4)                             # at most the rate the README gives as stable on 32 x 32 views


def spread(samples):
    return dict(median=round(float(np.median(samples)), 3), min=round(float(min(samples)), 3), max=round(float(max(samples)), 3))


def measure(side, n_views, n_calls, reps):
    from navsim_amd import NavBySceneFamiliarity, infomax_familiarity, synth
    from navsim_amd.util import infomax_network
    N = side * side
    sizes_m = (N // 4, N, 2 * N)
    land = synth.synth_landscape(3, 600, 4)
    out = dict(side=side, N=N, n_hidden=N, n_banks=N_BANKS, rates=list(RATES), sizes=list(sizes_m), calls_per_window=n_calls,
               views_per_route=n_views, layouts=[])
    own = infomax_network(N, None, RATES[0], 0)
    rates = [infomax_network(N, None, eta, 0) for eta in RATES]
    sizes = [infomax_network(N, m, RATES[0], 10 + j) for j, m in enumerate(sizes_m)]

    def agent_engine(A):
        return NavBySceneFamiliarity(land, (side, side), 1.0, n_test_angles=A, familiarity_model=infomax_familiarity(learning_rate=RATES[0]))._engine

    def begin(eng, net):
        eng.infomax_begin(side, side, net["w0"], net["channel"], net["learning_rate"])

    for n, A in ENSEMBLES:
        eng = agent_engine(A)
        lone = [agent_engine(A) for _ in sizes]
        rng = np.random.default_rng(n * 100 + A)
        xs, ys = rng.uniform(150, 450, n), rng.uniform(150, 450, n)
        offsets = np.linspace(-np.pi / 2, np.pi / 2, A)
        angs = (rng.uniform(0, 2 * np.pi, n)[:, None] + offsets[None, :]) % (2 * np.pi)
        mid = angs[:, A // 2].copy()
        banks4 = (np.arange(n) % N_BANKS).astype(np.int32)
        banks3 = (np.arange(n) % len(sizes)).astype(np.int32)
        each = list(range(N_BANKS))
        tables = {"no_table": None, "same_as_model": ([own] * N_BANKS, each, banks4), "four_rates": (rates, each, banks4),
                  "three_sizes": (sizes, list(range(len(sizes))), banks3)}

        def install(which):
            """(every bank trained on its members' middle views, as on short routes)"""
            begin(eng, own)
            if tables[which] is None:
                eng.ibank_set(N_BANKS, own["w0"])
                banks = banks4
            else:
                nets, of_bank, banks = tables[which]
                eng.inet_set(nets, of_bank)
            eng.ibank_train_from_poses(xs, ys, mid, banks, want_views=False)
            return banks

        def window(banks):
            eng.timer_start()
            for _ in range(n_calls):
                res = eng.ibank_sense_step_batch(xs, ys, angs, banks)
            return eng.timer_stop() * 1e3 / n_calls, res          # us per ensemble step

        members = [np.flatnonzero(banks3 == j) for j in range(len(sizes))]
        for j, e in enumerate(lone):
            begin(e, sizes[j])
            e.infomax_train_from_poses(xs[members[j]], ys[members[j]], mid[members[j]], want_views=False)

        def in_turn():
            t, rows = 0.0, []
            for j, e in enumerate(lone):
                e.timer_start()
                for _ in range(n_calls):
                    res = e.infomax_sense_step_batch(xs[members[j]], ys[members[j]], angs[members[j]])
                t += e.timer_stop() * 1e3 / n_calls
                rows.append(res.angle_familiarity)
            return t, rows

        # The table changes between windows (one engine, one process), so a window begins with its table installed and one untimed
        # step; every case is installed as often as every other.
        times = {which: [] for which in tables}
        times["three_engines_in_turn"] = []
        for rep in range(reps + 1):                               # (the first round is the warm-up: code load, clocks, the buffers)
            for which in tables:
                banks = install(which)
                _, res = window(banks)
                assert not res.flags.any() and np.isfinite(res.angle_familiarity).all() and res.angle_familiarity.max() < 0
                t, res = window(banks)
                if rep:
                    times[which].append(t)
            t, rows = in_turn()
            for j, m in enumerate(members):                       # (`res` is three_sizes': the three engines give its rows' bits)
                assert np.array_equal(rows[j].view(np.uint64), res.angle_familiarity[m].view(np.uint64)), j
            if rep:
                times["three_engines_in_turn"].append(t)
        med = {which: float(np.median(v)) for which, v in times.items()}
        row = dict(members=n, headings=A)
        for which, v in times.items():
            row[which + "_us_per_step"] = spread(v)
        for which in ("same_as_model", "four_rates", "three_sizes", "three_engines_in_turn"):
            row[which + "_over_no_table"] = round(med[which] / med["no_table"], 3)
        row["same_as_model_minus_no_table_us"] = round(med["same_as_model"] - med["no_table"], 3)
        row["three_engines_over_one_table"] = round(med["three_engines_in_turn"] / med["three_sizes"], 3)
        out["layouts"].append(row)
        eng.close()
        for e in lone:
            e.close()
    # (d) training: four networks in one banked call on one engine, against one call per network on an engine each
    engines = [agent_engine(ENSEMBLES[0][1]) for _ in range(N_BANKS)]
    rng = np.random.default_rng(side + 7)
    total = N_BANKS * n_views
    xs, ys, angs = rng.uniform(150, 450, total), rng.uniform(150, 450, total), rng.uniform(0, 2 * np.pi, total)
    bank_of = np.tile(np.arange(N_BANKS, dtype=np.int32), n_views)         # the routes' views interleaved: bank r's are xs[r::4]

    def one_call():
        eng = engines[0]
        begin(eng, own)
        eng.inet_set(rates, list(range(N_BANKS)))
        eng.timer_start()
        eng.ibank_train_from_poses(xs, ys, angs, bank_of, want_views=False)
        return eng.timer_stop() * 1e3

    def call_per_network():
        t = 0.0
        for r, eng in enumerate(engines):
            begin(eng, rates[r])
            eng.timer_start()
            eng.infomax_train_from_poses(xs[r::N_BANKS], ys[r::N_BANKS], angs[r::N_BANKS], want_views=False)
            t += eng.timer_stop() * 1e3
        return t

    one_call()
    banked = [engines[0].ibank_read_weights(r) for r in range(N_BANKS)]
    call_per_network()
    for r, e in enumerate(engines):                               # bank r of the one call against engine r's lone chain
        assert np.array_equal(banked[r].view(np.uint64), e.infomax_read_weights().view(np.uint64)), r
    del banked
    t1, t4 = [], []
    for _ in range(reps):
        t1.append(one_call())
        t4.append(call_per_network())
    out["train"] = dict(networks=N_BANKS, views_per_network=n_views, one_banked_call_us=spread(t1), call_per_network_us=spread(t4),
                        per_network_over_banked=round(float(np.median(t4) / np.median(t1)), 3))
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
        print("GPU measurement of the network tables of side %d ended with status %d: nothing more is run" % (side, p.returncode), file=sys.stderr)
        return p.returncode, None
    return 0, json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("side", type=int)
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    print(json.dumps(measure(args.side, args.views, args.calls, args.reps)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
