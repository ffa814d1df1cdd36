#!/usr/bin/env python3
"""Times the Infomax familiarity model (navsim_amd.infomax_familiarity; include/dejavu.h: dv_infomax_*) on GPU 0 and writes
profiles/infomax_time.json.

    python tools/infomax_time.py [--sides 32,64] [--views 400] [--calls 200] [--reps 5] [--blocks single,ensemble[,banks][,lands][,sensors][,networks][,noise]]
                                 [--out profiles/infomax_time.json]

Per sensor side s (views of s x s, N = M = s*s): microseconds per training view (a dv_infomax_train_u8 call over --views views, the
upload and the x preparation included, divided by the views) and per scoring call (dv_infomax_score_u8: upload, x preparation, the
pass over W and the read-back) for 16 and for 60 headings, each the median of --reps timed windows after a warm-up of the same
shape, from a hipEvent pair on the context's stream (dv_timer_start / dv_timer_stop) with the spread (min, max) beside it.  Beside
each figure its byte floor -- 3*8*M*N bytes per training view (W read twice, written once), 8*M*N per scoring call -- over the box's
own stream probe (dv_stream_read_gbps), and the fraction of that floor reached.  The same quantities for the NumPy restatement of
the model (tests/helpers_infomax.py) on the host's CPU, wall clock.

Ensemble block (--blocks ensemble): per side, 32 members x 16 headings and 8 members x 60 headings at poses spread over a synthetic
landscape -- microseconds per ensemble step of dv_batch_infomax_sense_step (one call for all members), and of the same poses as a
loop of dv_infomax_sense_step calls (one per member), the two taken in the same child process in alternating windows; median and
spread of --reps windows each, and the byte floor 8*M*N of one pass over W at the stream probe beside them.  (The matrix-time floor
from an fp64 MFMA rate probe is not part of the tool yet.)

Banks block (--blocks banks): per side, (a) training -- 4 routes of --route-views sensed views each (random poses on the synthetic
landscape) in ONE dv_ibank_train_from_poses call on one engine of 4 banks, against four dv_infomax_train_from_poses calls on four
engines (what there was before the banks), the two sides in alternating windows of one process, a window being one whole training;
microseconds from the hipEvent pair of each call (summed over the four) and, beside it, the wall clock around the calls; and (b) the
step -- the ensemble block's two layouts over 4 banks (dv_ibank_sense_step; member i in bank i % 4) against dv_batch_infomax_sense_step
at the same poses on one W.  Medians and spreads of --reps windows.  A block that is not measured keeps the rows the file holds.

Lands block (--blocks lands): per side, the two layouts over 4 banks AND 4 landscapes of three shapes held as a landscape set
(dv_lands_set; member i in bank i % 4 on landscape 3 i % 4) -- (a) dv_lands_ibank_sense_step against dv_ibank_sense_step at the same
poses on ONE landscape (the call as it was before landscape sets, in the SAME build of the library: its code path is untouched),
hipEvent pairs in alternating windows, ratio lands_over_one_landscape; (b) the same members as four engines of one landscape each, every engine stepping its landscape's members in
turn, against the one call, both WALL CLOCK, ratio four_engines_over_lands_wall (the four engines' rows are checked to be the one
call's bits); (c) 4 routes of --route-views views on the 4 landscapes trained in ONE dv_lands_ibank_train_from_poses call against four
dv_infomax_train_from_poses calls on four engines.

Networks block (--blocks networks): per side, the banks block's two layouts under network tables (dv_inet_set) against the banked step
without a table at the same poses -- a table equal to the model's, four learning rates, n_hidden = N/4, N and 2N in one table against
three engines stepped in turn -- and one banked training call over four networks against four engines (tools/networks_block.py).

Every GPU measurement runs in a child process of its own under a time limit, and nothing more is started on the GPU after one
that failed."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "navigation-by-deja-vu_amd"))
sys.path.insert(0, ROOT)

HEADINGS = (16, 60)                                               # 60: the reference's default n_test_angles


def views_of(side, n, seed=1):
    from tests import helpers_infomax as H
    return H.route_views(seed, n, side, side)


def spread(samples):
    return dict(median=round(float(np.median(samples)), 3), min=round(float(min(samples)), 3), max=round(float(max(samples)), 3))


def gpu_child(side, n_views, n_calls, reps, eta):
    """One size on the GPU -> one JSON line on stdout."""
    from navsim_amd import FamiliarityEngine
    from navsim_amd.util import infomax_initial_weights
    N = side * side
    eng = FamiliarityEngine(device=0)
    out = dict(side=side, N=N, M=N, weight_bytes=8 * N * N)
    out["stream_probe_gbps"] = round(eng.stream_read_gbps(1 << 30, 10), 1)
    views = views_of(side, n_views)
    W0 = infomax_initial_weights(N, N, 0)

    def train_once():
        eng.infomax_begin(side, side, W0, 2, eta)
        eng.timer_start()
        eng.infomax_train_u8(views)
        return eng.timer_stop() * 1e3 / n_views               # us per view

    train_once()                                                  # warm-up (code load, clocks, the staging buffers)
    out["train_us_per_view"] = spread([train_once() for _ in range(reps)])
    out["views_per_window"] = n_views
    assert eng.infomax_info()["finite"]
    for A in HEADINGS:
        patches = views_of(side, A, seed=2)
        fam = np.empty(A)

        def score_window():
            eng.timer_start()
            for _ in range(n_calls):
                eng.infomax_score_u8(patches, fam)
            return eng.timer_stop() * 1e3 / n_calls           # us per call
        score_window()
        out["score_us_per_call_A%d" % A] = spread([score_window() for _ in range(reps)])
    out["calls_per_window"] = n_calls
    eng.close()
    print(json.dumps(out))


ENSEMBLES = ((32, 16), (8, 60))                                   # (members, headings)


def ensemble_child(side, n_calls, reps, eta):
    """The ensemble block of one size on the GPU -> one JSON line on stdout."""
    from navsim_amd import NavBySceneFamiliarity, infomax_familiarity, synth
    from navsim_amd.util import infomax_initial_weights
    N = side * side
    land = synth.synth_landscape(3, 600, 4)
    out = dict(side=side, N=N, M=N, weight_bytes=8 * N * N, calls_per_window=n_calls, layouts=[])
    for n, A in ENSEMBLES:
        agent = NavBySceneFamiliarity(land, (side, side), 1.0, n_test_angles=A, familiarity_model=infomax_familiarity(learning_rate=eta))
        eng = agent._engine                                       # (landscape and sensor attached; the weights are the initial ones)
        if "stream_probe_gbps" not in out:
            out["stream_probe_gbps"] = round(eng.stream_read_gbps(1 << 30, 10), 1)
        eng.infomax_begin(side, side, infomax_initial_weights(N, N, 0), 2, eta)
        rng = np.random.default_rng(n * 100 + A)
        xs, ys = rng.uniform(150, 450, n), rng.uniform(150, 450, n)
        angs = (rng.uniform(0, 2 * np.pi, n)[:, None] + agent.angle_offsets[None, :]) % (2 * np.pi)
        fam = np.empty(A)

        def batched():
            eng.timer_start()
            for _ in range(n_calls):
                res = eng.infomax_sense_step_batch(xs, ys, angs)
            return eng.timer_stop() * 1e3 / n_calls, res          # us per ensemble step

        def looped():
            eng.timer_start()
            for _ in range(n_calls):
                for i in range(n):
                    eng.infomax_sense_step(xs[i], ys[i], angs[i], fam)
            return eng.timer_stop() * 1e3 / n_calls

        _, res = batched()                                        # warm-up of both (code load, clocks, the buffers)
        looped()
        assert not res.flags.any()
        tb, tl = [], []
        for _ in range(reps):                                     # alternating windows
            tb.append(batched()[0])
            tl.append(looped())
        out["layouts"].append(dict(members=n, headings=A, batched_us_per_step=spread(tb), loop_us_per_step=spread(tl),
                                   loop_over_batched=round(float(np.median(tl) / np.median(tb)), 3)))
        eng.close()
    print(json.dumps(out))


N_BANKS = 4


def banks_child(side, n_views, n_calls, reps, eta):
    """The banks block of one size on the GPU -> one JSON line on stdout."""
    from navsim_amd import NavBySceneFamiliarity, infomax_familiarity, synth
    from navsim_amd.util import infomax_initial_weights
    N = side * side
    land = synth.synth_landscape(3, 600, 4)
    W0 = infomax_initial_weights(N, N, 0)
    out = dict(side=side, N=N, M=N, weight_bytes=8 * N * N, n_banks=N_BANKS, calls_per_window=n_calls, layouts=[])

    def engine(A):
        agent = NavBySceneFamiliarity(land, (side, side), 1.0, n_test_angles=A, familiarity_model=infomax_familiarity(learning_rate=eta))
        return agent, agent._engine                              # (landscape and sensor attached)

    # (a) training: N_BANKS routes in one banked call on one engine, against one call per route on an engine each
    engines = [engine(HEADINGS[0])[1] for _ in range(N_BANKS)]
    rng = np.random.default_rng(side + 7)
    total = N_BANKS * n_views
    xs, ys, angs = rng.uniform(150, 450, total), rng.uniform(150, 450, total), rng.uniform(0, 2 * np.pi, total)
    bank_of = np.repeat(np.arange(N_BANKS, dtype=np.int32), n_views)

    def one_call():
        eng = engines[0]
        eng.infomax_begin(side, side, W0, 2, eta)
        eng.ibank_set(N_BANKS, W0)
        w0 = time.perf_counter()
        eng.timer_start()
        eng.ibank_train_from_poses(xs, ys, angs, bank_of, want_views=False)
        return eng.timer_stop() * 1e3, (time.perf_counter() - w0) * 1e6

    def call_per_route():
        t = wall = 0.0
        for r, eng in enumerate(engines):
            eng.infomax_begin(side, side, W0, 2, eta)
            sl = slice(r * n_views, (r + 1) * n_views)
            w0 = time.perf_counter()
            eng.timer_start()
            eng.infomax_train_from_poses(xs[sl], ys[sl], angs[sl], want_views=False)
            t += eng.timer_stop() * 1e3
            wall += (time.perf_counter() - w0) * 1e6
        return t, wall

    one_call()                                                    # warm-up of both (code load, clocks, the buffers)
    banked_w = [engines[0].ibank_read_weights(r) for r in range(N_BANKS)]
    call_per_route()
    assert all(np.array_equal(banked_w[r], engines[r].infomax_read_weights()) for r in range(N_BANKS))      # the same bits
    assert all(np.isfinite(w).all() for w in banked_w)
    t1, t4, w1, w4 = [], [], [], []
    for _ in range(reps):                                         # alternating windows
        a, b = one_call()
        t1.append(a)
        w1.append(b)
        a, b = call_per_route()
        t4.append(a)
        w4.append(b)
    out["train"] = dict(routes=N_BANKS, views_per_route=n_views, one_banked_call_us=spread(t1), call_per_route_us=spread(t4),
                        per_route_over_banked=round(float(np.median(t4) / np.median(t1)), 3),
                        one_banked_call_wall_us=spread(w1), call_per_route_wall_us=spread(w4),
                        per_route_over_banked_wall=round(float(np.median(w4) / np.median(w1)), 3),
                        banked_below_call_per_route=bool(np.median(t1) < np.median(t4)),
                        kernel_launches=dict(one_banked_call=3 * n_views + 4, call_per_route=N_BANKS * (3 * n_views + 4)))
    for e in engines:
        e.close()
    # (b) the step: the ensemble block's layouts over N_BANKS banks against the same poses on one W
    for n, A in ENSEMBLES:
        agent, eng = engine(A)
        eng.infomax_begin(side, side, W0, 2, eta)
        eng.ibank_set(N_BANKS, W0)
        rng = np.random.default_rng(n * 100 + A)
        xs, ys = rng.uniform(150, 450, n), rng.uniform(150, 450, n)
        angs = (rng.uniform(0, 2 * np.pi, n)[:, None] + agent.angle_offsets[None, :]) % (2 * np.pi)
        banks = (np.arange(n) % N_BANKS).astype(np.int32)

        def banked():
            eng.timer_start()
            for _ in range(n_calls):
                res = eng.ibank_sense_step_batch(xs, ys, angs, banks)
            return eng.timer_stop() * 1e3 / n_calls, res          # us per ensemble step

        def unbanked():
            eng.timer_start()
            for _ in range(n_calls):
                res = eng.infomax_sense_step_batch(xs, ys, angs)
            return eng.timer_stop() * 1e3 / n_calls, res

        _, res = banked()
        _, one = unbanked()
        assert not res.flags.any() and np.array_equal(res.angle_familiarity, one.angle_familiarity)       # (every bank holds W0)
        tb, tu = [], []
        for _ in range(reps):                                     # alternating windows
            tb.append(banked()[0])
            tu.append(unbanked()[0])
        out["layouts"].append(dict(members=n, headings=A, banked_us_per_step=spread(tb), unbanked_us_per_step=spread(tu),
                                   banked_over_unbanked=round(float(np.median(tb) / np.median(tu)), 3)))
        eng.close()
    print(json.dumps(out))


LAND_SHAPES = ((600, 600), (560, 600), (600, 540), (600, 600))     # rows, cols: the poses lie inside all of them


def lands_child(side, n_views, n_calls, reps, eta):
    """The lands block of one size on the GPU -> one JSON line on stdout."""
    from navsim_amd import NavBySceneFamiliarity, infomax_familiarity, synth
    from navsim_amd.util import infomax_initial_weights
    N = side * side
    lands = [np.ascontiguousarray(synth.synth_landscape(3 + l, 600, 4)[:r, :c]) for l, (r, c) in enumerate(LAND_SHAPES)]
    L = len(lands)
    W0 = infomax_initial_weights(N, N, 0)
    out = dict(side=side, N=N, M=N, weight_bytes=8 * N * N, n_banks=N_BANKS, n_lands=L, land_shapes=LAND_SHAPES, calls_per_window=n_calls,
               layouts=[])

    def engine(land, A, banks):
        agent = NavBySceneFamiliarity(land, (side, side), 1.0, n_test_angles=A, familiarity_model=infomax_familiarity(learning_rate=eta))
        agent._engine.infomax_begin(side, side, W0, 2, eta)
        if banks > 1:
            agent._engine.ibank_set(banks, W0)
        return agent, agent._engine                              # (landscape and sensor attached)

    # (c) training: L routes on L landscapes in one call on one engine, against one call per route on an engine each
    engines = [engine(lands[l], HEADINGS[0], 1)[1] for l in range(L)]
    engines[0].lands_set(lands)
    rng = np.random.default_rng(side + 7)
    total = L * n_views
    xs, ys, angs = rng.uniform(150, 390, total), rng.uniform(150, 390, total), rng.uniform(0, 2 * np.pi, total)
    route_of = np.repeat(np.arange(L, dtype=np.int32), n_views)

    def one_call():
        eng = engines[0]
        eng.infomax_begin(side, side, W0, 2, eta)
        eng.ibank_set(N_BANKS, W0)
        w0 = time.perf_counter()
        eng.timer_start()
        eng.ibank_train_from_poses(xs, ys, angs, route_of, want_views=False, land_of_view=route_of)
        return eng.timer_stop() * 1e3, (time.perf_counter() - w0) * 1e6

    def call_per_route():
        t = wall = 0.0
        for r, eng in enumerate(engines):
            eng.infomax_begin(side, side, W0, 2, eta)
            sl = slice(r * n_views, (r + 1) * n_views)
            w0 = time.perf_counter()
            eng.timer_start()
            eng.infomax_train_from_poses(xs[sl], ys[sl], angs[sl], want_views=False)
            t += eng.timer_stop() * 1e3
            wall += (time.perf_counter() - w0) * 1e6
        return t, wall

    one_call()                                                    # warm-up of both (code load, clocks, the buffers)
    trained = [engines[0].ibank_read_weights(r) for r in range(N_BANKS)]
    call_per_route()
    assert all(np.array_equal(trained[r], engines[r].infomax_read_weights()) for r in range(L))            # the same bits
    assert all(np.isfinite(w).all() for w in trained)
    t1, t4, w1, w4 = [], [], [], []
    for _ in range(reps):                                         # alternating windows
        a, b = one_call()
        t1.append(a)
        w1.append(b)
        a, b = call_per_route()
        t4.append(a)
        w4.append(b)
    out["train"] = dict(routes=L, views_per_route=n_views, one_lands_call_us=spread(t1), call_per_route_us=spread(t4),
                        per_route_over_lands=round(float(np.median(t4) / np.median(t1)), 3), one_lands_call_wall_us=spread(w1),
                        call_per_route_wall_us=spread(w4), per_route_over_lands_wall=round(float(np.median(w4) / np.median(w1)), 3))
    for e in engines:
        e.close()
    # (a), (b) the step, under the banks the training above left (four different W)
    for n, A in ENSEMBLES:
        agent, eng = engine(lands[0], A, N_BANKS)
        eng.lands_set(lands)
        four = [engine(lands[l], A, N_BANKS)[1] for l in range(L)]
        for e in four + [eng]:
            for r in range(N_BANKS):
                e.ibank_set_weights(r, trained[r])
        rng = np.random.default_rng(n * 100 + A)
        xs, ys = rng.uniform(150, 390, n), rng.uniform(150, 390, n)
        angs = (rng.uniform(0, 2 * np.pi, n)[:, None] + agent.angle_offsets[None, :]) % (2 * np.pi)
        banks = (np.arange(n) % N_BANKS).astype(np.int32)
        land_of = (3 * np.arange(n) % L).astype(np.int32)
        mine = [np.flatnonzero(land_of == l) for l in range(L)]
        parts = [(four[l], xs[m].copy(), ys[m].copy(), angs[m].copy(), banks[m].copy()) for l, m in enumerate(mine)]

        def on_set():
            w0 = time.perf_counter()
            eng.timer_start()
            for _ in range(n_calls):
                res = eng.ibank_sense_step_batch(xs, ys, angs, banks, land_of_member=land_of)
            return eng.timer_stop() * 1e3 / n_calls, (time.perf_counter() - w0) * 1e6 / n_calls, res

        def one_landscape():
            eng.timer_start()
            for _ in range(n_calls):
                eng.ibank_sense_step_batch(xs, ys, angs, banks)
            return eng.timer_stop() * 1e3 / n_calls

        def four_engines():
            w0 = time.perf_counter()
            for _ in range(n_calls):
                rows = [e.ibank_sense_step_batch(x, y, a, b) for e, x, y, a, b in parts]
            return (time.perf_counter() - w0) * 1e6 / n_calls, rows

        _, _, res = on_set()                                      # warm-up of all three
        one_landscape()
        _, rows = four_engines()
        assert not res.flags.any()
        for m, row in zip(mine, rows):                            # the same bits as an engine of that landscape alone
            assert np.array_equal(res.angle_familiarity[m], row.angle_familiarity) and np.array_equal(res.best_idex[m], row.best_idex)
        ts, ws, t1, w4 = [], [], [], []
        for _ in range(reps):                                     # alternating windows
            a, b, _ = on_set()
            ts.append(a)
            ws.append(b)
            t1.append(one_landscape())
            w4.append(four_engines()[0])
        out["layouts"].append(dict(members=n, headings=A, lands_us_per_step=spread(ts), one_landscape_us_per_step=spread(t1),
                                   lands_over_one_landscape=round(float(np.median(ts) / np.median(t1)), 3),
                                   lands_wall_us_per_step=spread(ws), four_engines_wall_us_per_step=spread(w4),
                                   four_engines_over_lands_wall=round(float(np.median(w4) / np.median(ws)), 3)))
        for e in four + [eng]:
            e.close()
    print(json.dumps(out))


def cpu_row(side, n_views, n_calls, eta):
    """The NumPy restatement on this host: wall clock."""
    from tests import helpers_infomax as H
    N = side * side
    views = views_of(side, n_views)
    W0 = H.initial_weights(N, N, 0)
    t0 = time.perf_counter()
    W = H.train(W0, views, eta=eta)
    t1 = time.perf_counter()
    row = dict(train_us_per_view=round((t1 - t0) * 1e6 / n_views, 1), views=n_views)
    for A in HEADINGS:
        patches = views_of(side, A, seed=2)
        t0 = time.perf_counter()
        for _ in range(n_calls):
            H.familiarity(W, patches)
        row["score_us_per_call_A%d" % A] = round((time.perf_counter() - t0) * 1e6 / n_calls, 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", default="32,64")
    ap.add_argument("--views", type=int, default=400)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--learning-rate", type=float, default=0.001,
                    help="the rule must stay finite on the tool's 5-level noise views: 0.01 overflows at 64x64 (the time does not depend on it)")
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed to each GPU child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infomax_time.json"))
    ap.add_argument("--blocks", default="single,ensemble", help="which blocks to measure: single (training and score_u8), ensemble, banks, lands, sensors (tools/sensors_block.py: dv_lands_ibank_sense_step without a sensor table, with one of equal entries and with one of four different entries), networks (tools/networks_block.py: network tables against the banked step without one), noise (tools/noise_block.py: dv_lands_ibank_sense_step without noise rows, under rows of zero amplitude and of amplitude 20, and with the rows set again before every step)")
    ap.add_argument("--route-views", type=int, default=200, help="sensed views of each of the banks block's 4 routes")
    ap.add_argument("--banks-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--lands-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--ensemble-calls", type=int, default=30, help="ensemble steps per timed window")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--ensemble-child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        gpu_child(args.child, args.views, args.calls, args.reps, args.learning_rate)
        return 0
    if args.ensemble_child:
        ensemble_child(args.ensemble_child, args.ensemble_calls, args.reps, args.learning_rate)
        return 0
    if args.banks_child:
        banks_child(args.banks_child, args.route_views, args.ensemble_calls, args.reps, args.learning_rate)
        return 0
    if args.lands_child:
        lands_child(args.lands_child, args.route_views, args.ensemble_calls, args.reps, args.learning_rate)
        return 0
    blocks = args.blocks.split(",")
    result = dict(tool="tools/infomax_time.py", timer="hipEvent pair (dv_timer_start/stop), median of %d windows after a warm-up" % args.reps,
                  learning_rate=args.learning_rate, blocks=blocks, sizes=[], ensembles=[], banks=[], lands=[], sensors=[], networks=[], noise=[])
    if os.path.exists(args.out):                                  # a block that is not measured keeps its rows
        with open(args.out) as f:
            kept = json.load(f)
        for block, key in (("single", "sizes"), ("ensemble", "ensembles"), ("banks", "banks"), ("lands", "lands"), ("sensors", "sensors"),
                           ("networks", "networks"), ("noise", "noise")):
            if block not in blocks:
                result[key] = kept.get(key, [])
        result["blocks"] = [b for b in kept.get("blocks", []) if b not in blocks] + blocks      # (every block whose rows the file holds)
    for side in [int(x) for x in args.sides.split(",")] if "banks" in blocks else []:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--banks-child", str(side),
               "--route-views", str(args.route_views), "--ensemble-calls", str(args.ensemble_calls), "--reps", str(args.reps),
               "--learning-rate", str(args.learning_rate)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if p.returncode != 0:
            print("GPU measurement of the banks of side %d ended with status %d: nothing more is run" % (side, p.returncode), file=sys.stderr)
            return p.returncode
        result["banks"].append(json.loads(p.stdout.strip().splitlines()[-1]))
    for side in [int(x) for x in args.sides.split(",")] if "lands" in blocks else []:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--lands-child", str(side),
               "--route-views", str(args.route_views), "--ensemble-calls", str(args.ensemble_calls), "--reps", str(args.reps),
               "--learning-rate", str(args.learning_rate)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if p.returncode != 0:
            print("GPU measurement of the landscape sets of side %d ended with status %d: nothing more is run" % (side, p.returncode), file=sys.stderr)
            return p.returncode
        result["lands"].append(json.loads(p.stdout.strip().splitlines()[-1]))
    if "sensors" in blocks:
        import sensors_block
        rc, row = sensors_block.run_child(args.limit, args.ensemble_calls, args.reps, "infomax")
        if rc != 0:
            return rc
        result["sensors"].append(row)
    if "noise" in blocks:
        import noise_block
        rc, row = noise_block.run_child(args.limit, [int(x) for x in args.sides.split(",")], args.ensemble_calls, args.reps, "infomax")
        if rc != 0:
            return rc
        result["noise"].append(row)
    for side in [int(x) for x in args.sides.split(",")] if "networks" in blocks else []:
        import networks_block
        rc, row = networks_block.run_child(args.limit, side, args.route_views, args.ensemble_calls, args.reps)
        if rc != 0:
            return rc
        result["networks"].append(row)
    for side in [int(x) for x in args.sides.split(",")] if "ensemble" in blocks else []:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--ensemble-child", str(side),
               "--ensemble-calls", str(args.ensemble_calls), "--reps", str(args.reps), "--learning-rate", str(args.learning_rate)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if p.returncode != 0:
            print("GPU measurement of the ensembles of side %d ended with status %d: nothing more is run" % (side, p.returncode), file=sys.stderr)
            return p.returncode
        row = json.loads(p.stdout.strip().splitlines()[-1])
        row["byte_floor_us_at_probe"] = round(8 * row["M"] * row["N"] / (row["stream_probe_gbps"] * 1e3), 3)
        result["ensembles"].append(row)
    for side in [int(x) for x in args.sides.split(",")] if "single" in blocks else []:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", str(side), "--views", str(args.views),
               "--calls", str(args.calls), "--reps", str(args.reps), "--learning-rate", str(args.learning_rate)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if p.returncode != 0:
            print("GPU measurement of side %d ended with status %d: nothing more is run" % (side, p.returncode), file=sys.stderr)
            return p.returncode
        row = json.loads(p.stdout.strip().splitlines()[-1])
        gbps = row["stream_probe_gbps"]
        M = N = row["N"]
        floors = dict(train=3 * 8 * M * N, score=8 * M * N)
        row["train_floor_bytes_per_view"] = floors["train"]
        row["score_floor_bytes_per_call"] = floors["score"]
        for key, kind in [("train_us_per_view", "train")] + [("score_us_per_call_A%d" % A, "score") for A in HEADINGS]:
            floor_us = floors[kind] / (gbps * 1e3)
            row[key]["floor_us_at_probe"] = round(floor_us, 3)
            row[key]["fraction_of_probe"] = round(floor_us / row[key]["median"], 4)
        row["numpy_cpu"] = cpu_row(side, min(args.views, 40), min(args.calls, 10), args.learning_rate)
        result["sizes"].append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
