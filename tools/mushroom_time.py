#!/usr/bin/env python3
"""Times the mushroom-body familiarity model (navsim_amd.mushroom_familiarity; include/dejavu.h: dv_mb_*) on GPU 0 and writes
profiles/mushroom_time.json.

    python tools/mushroom_time.py [--sides 32,64] [--views 1000] [--calls 200] [--reps 5] [--blocks single,ensemble[,banks][,metrics][,lands][,rows][,sensors][,populations][,noise][,sets]]
                                  [--out profiles/mushroom_time.json]

Per sensor side s (views of s x s) with K = 20000 Kenyon cells, fan-in 10 and 200 firing cells: microseconds per agent step
(dv_mb_sense_step: sensing, one scoring launch over all headings, the decision and the read-back) for 16 and for 60 headings, and
microseconds to train --views sensed views (dv_mb_train_from_poses without the views' read-back: sensing and one training launch),
each the median of --reps timed windows after a warm-up of the same shape, from a hipEvent pair on the context's stream
(dv_timer_start / dv_timer_stop) with the spread (min, max) beside it.  For context, from the same child process: the Infomax
model's step (dv_infomax_sense_step, N x N weights) at the same shapes; and from this host's CPU, wall clock: the NumPy statement
of the model (tests/helpers_mushroom.py) scoring the same number of patches.

Ensemble block (--blocks ensemble): per side, 32 members x 16 headings and 8 members x 60 headings at poses spread over the synthetic
landscape -- microseconds per ensemble step of dv_batch_mb_sense_step (one call for all members), and of the same poses as a loop of
dv_mb_sense_step calls, one per member, from the same child process in alternating windows of --ensemble-calls steps; their ratio is
loop_over_batched.

Banks block (--blocks banks): per side, the same two layouts over 4 memory banks (dv_mbank_set; member i in bank i % 4) --
microseconds per ensemble step of dv_mbank_sense_step and of dv_batch_mb_sense_step (every member under bank 0: the unbanked call, the
yardstick) at the same poses, alternating windows in the same child process; their ratio is banked_over_unbanked.  And training: 4
routes of --views views each in ONE dv_mbank_train_from_poses call on one engine, against four dv_mb_train_from_poses calls on four
engines (the sum of the four engines' own timers).

Metrics block (--blocks metrics): MushroomRouteEnsemble of 4 routes x 8 members x 16 headings at 32x32 views, made twice in one child
process -- from_routes_with(metrics="host"), every member's update_error a NumPy pass over its own route, and metrics="device", all
members' in one dv_path_routes_error call -- and stepped from the same starts, so both walk the same poses: WALL-CLOCK microseconds per
ens.step_forward(), Python included, in alternating windows of --ensemble-calls steps, for routes of about 3 500 points (a grid trial's)
and of about 50 000 (the sin path's arclen is set to reach the count); their ratio is host_over_device.  And the path_routes_error call
alone, at the members' last positions.

Lands block (--blocks lands): per side, the banks block's two layouts over 4 banks AND 4 landscapes of three shapes held as a
landscape set (dv_lands_set; member i in bank i % 4 on landscape 3 i % 4) -- (a) microseconds per ensemble step of
dv_lands_mbank_sense_step against dv_mbank_sense_step at the same poses on ONE landscape (the call as it was before landscape sets,
in the SAME build of the library: its code path is untouched),
hipEvent pairs in alternating windows, ratio lands_over_one_landscape; (b) the same members as four engines of one landscape each,
every engine stepping its landscape's members in turn -- what a user did before -- against the one call, both WALL CLOCK (four
streams have no common event pair), ratio four_engines_over_lands_wall; the four engines' rows are checked to be the one call's bits;
(c) 4 routes of --views views on the 4 landscapes trained in ONE dv_lands_mbank_train_from_poses call against four
dv_mb_train_from_poses calls on four engines (the sum of their timers, and wall clock).

Sensors block (--blocks sensors): the lands block's 32 x 32 layouts stepped by dv_lands_mbank_sense_step on the set without a sensor
table, with a table of four entries equal to the engine's sensor, and with a table of four different entries, in alternating windows
of one process (tools/sensors_block.py, which states the figures).

Noise block (--blocks noise): per side, the lands block's layouts stepped by dv_lands_mbank_sense_step without noise rows, under rows of
zero amplitude, under rows of amplitude 20, and with the rows set again before every step as a route ensemble sets them, in
alternating windows of one process (tools/noise_block.py, which states the figures).

Rows block (--blocks rows): the metrics block's MushroomRouteEnsemble with metrics="device" (4 routes x 8 members, both route sizes),
stepped --row-frames frames; then the three coverage columns of all members' result rows built two ways in alternating windows of the
same child process -- (a) every member's percent_recapitulated, percent_recapitulated_forgiving(0.05) and n_captures(0.05), as
run_ensemble built them before: three copies of the member's marks and two Python loops over them; (b) ens.coverage_summary(0.05): one
dv_marks_summary_routes call for all members -- WALL-CLOCK microseconds per build of all rows, Python included (a window is one build
of (a), 20 of (b)), their ratio methods_over_summary; and alone: the 3 x 32 path_routes_coverage copies of (a) without its loops (wall
clock), and the marks_summary_routes call between a hipEvent pair.  The two builds are checked to give equal rows.

Populations block (--blocks populations): per side, the banks block's two layouts under population tables (dv_mbpop_set) against the
banked step without a table at the same poses -- a table equal to the model's, four wirings, three sizes in one table against three
engines stepped in turn -- and one banked training call over four populations against four engines (tools/populations_block.py).

A block that is not measured keeps the rows it has in the output file.

Sets block (--blocks sets, tools/sets_block.py): per side, the banks block's two layouts over 4 routes of two memories each, stepped by
dv_mbset_sense_step at S = 1, 2 and 8 banks a member, by the banked step at the same poses, and by the banked step with every
member entered S times -- what the same read-out costs without sets.

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
ENSEMBLES = ((32, 16), (8, 60))                                   # (members, headings)
K, FAN_IN, N_ACTIVE = 20000, 10, 200


def spread(samples):
    return dict(median=round(float(np.median(samples)), 3), min=round(float(min(samples)), 3), max=round(float(max(samples)), 3))


def gpu_child(side, n_views, n_calls, reps):
    """One size on the GPU -> one JSON line on stdout."""
    from navsim_amd import NavBySceneFamiliarity, mushroom_familiarity, synth
    from navsim_amd.util import infomax_initial_weights, mushroom_connectivity
    N = side * side
    land = synth.synth_landscape(3, 600, 4)
    agent = NavBySceneFamiliarity(land, (side, side), 1.0, n_test_angles=HEADINGS[-1], familiarity_model=mushroom_familiarity())
    eng = agent._engine                                           # (landscape and sensor attached)
    out = dict(side=side, N=N, n_kc=K, fan_in=FAN_IN, n_active=N_ACTIVE, calls_per_window=n_calls, views_per_window=n_views)
    conn = mushroom_connectivity(K, N, FAN_IN, 0)
    rng = np.random.default_rng(side)
    xs, ys, angs = rng.uniform(150, 450, n_views), rng.uniform(150, 450, n_views), rng.uniform(0, 2 * np.pi, n_views)

    def train_window():
        eng.mb_begin(side, side, conn, N_ACTIVE, 2)
        eng.timer_start()
        eng.mb_train_from_poses(xs, ys, angs, want_views=False)
        return eng.timer_stop() * 1e3                             # us per n_views views

    train_window()                                                # warm-up (code load, clocks, the buffers)
    out["train_us_per_%d_views" % n_views] = spread([train_window() for _ in range(reps)])
    info = eng.mb_info()
    out["n_depressed_after_training"] = info["n_depressed"]
    assert info["views_trained"] == n_views and 0 < info["n_depressed"] <= K

    def step_windows(step, A):
        angles = (0.3 + np.linspace(-np.pi / 2, np.pi / 2, A)) % (2 * np.pi)
        fam = np.empty(A)

        def window():
            eng.timer_start()
            for _ in range(n_calls):
                step(300.0, 300.0, angles, fam)
            return eng.timer_stop() * 1e3 / n_calls               # us per step
        window()
        return spread([window() for _ in range(reps)])

    for A in HEADINGS:
        out["mb_sense_step_us_A%d" % A] = step_windows(eng.mb_sense_step, A)
    eng.mb_end()
    eng.infomax_begin(side, side, infomax_initial_weights(N, N, 0), 2, 0.001)
    for A in HEADINGS:
        out["infomax_sense_step_us_A%d" % A] = step_windows(eng.infomax_sense_step, A)
    eng.close()
    print(json.dumps(out))


def ensemble_child(side, n_calls, reps):
    """The ensemble block of one size on the GPU -> one JSON line on stdout."""
    from navsim_amd import NavBySceneFamiliarity, mushroom_familiarity, synth
    from navsim_amd.util import mushroom_connectivity
    N = side * side
    land = synth.synth_landscape(3, 600, 4)
    out = dict(side=side, N=N, n_kc=K, fan_in=FAN_IN, n_active=N_ACTIVE, calls_per_window=n_calls, layouts=[])
    conn = mushroom_connectivity(K, N, FAN_IN, 0)
    for n, A in ENSEMBLES:
        agent = NavBySceneFamiliarity(land, (side, side), 1.0, n_test_angles=A, familiarity_model=mushroom_familiarity())
        eng = agent._engine                                       # (landscape and sensor attached)
        eng.mb_begin(side, side, conn, N_ACTIVE, 2)
        rng = np.random.default_rng(n * 100 + A)
        xs, ys = rng.uniform(150, 450, n), rng.uniform(150, 450, n)
        angs = (rng.uniform(0, 2 * np.pi, n)[:, None] + agent.angle_offsets[None, :]) % (2 * np.pi)
        eng.mb_train_from_poses(xs, ys, angs[:, A // 2].copy(), want_views=False)   # (some weights at 0, as on a trained route)
        fam = np.empty(A)

        def batched():
            eng.timer_start()
            for _ in range(n_calls):
                res = eng.mb_sense_step_batch(xs, ys, angs)
            return eng.timer_stop() * 1e3 / n_calls, res          # us per ensemble step

        def looped():
            eng.timer_start()
            for _ in range(n_calls):
                for i in range(n):
                    eng.mb_sense_step(xs[i], ys[i], angs[i], fam)
            return eng.timer_stop() * 1e3 / n_calls

        _, res = batched()                                        # warm-up of both (code load, clocks, the buffers)
        looped()
        assert not res.flags.any() and res.angle_familiarity.max() == 0.0 and res.angle_familiarity.min() < 0
        tb, tl = [], []
        for _ in range(reps):                                     # alternating windows
            tb.append(batched()[0])
            tl.append(looped())
        out["layouts"].append(dict(members=n, headings=A, batched_us_per_step=spread(tb), loop_us_per_step=spread(tl),
                                   loop_over_batched=round(float(np.median(tl) / np.median(tb)), 3)))
        eng.close()
    print(json.dumps(out))


N_BANKS = 4


def banks_child(side, n_views, n_calls, reps):
    """The banks block of one size on the GPU -> one JSON line on stdout."""
    from navsim_amd import NavBySceneFamiliarity, mushroom_familiarity, synth
    from navsim_amd.util import mushroom_connectivity
    N = side * side
    land = synth.synth_landscape(3, 600, 4)
    out = dict(side=side, N=N, n_kc=K, fan_in=FAN_IN, n_active=N_ACTIVE, n_banks=N_BANKS, calls_per_window=n_calls,
               views_per_route=n_views, layouts=[])
    conn = mushroom_connectivity(K, N, FAN_IN, 0)
    for n, A in ENSEMBLES:
        agent = NavBySceneFamiliarity(land, (side, side), 1.0, n_test_angles=A, familiarity_model=mushroom_familiarity())
        eng = agent._engine                                       # (landscape and sensor attached)
        eng.mb_begin(side, side, conn, N_ACTIVE, 2)
        eng.mbank_set(N_BANKS)
        rng = np.random.default_rng(n * 100 + A)
        xs, ys = rng.uniform(150, 450, n), rng.uniform(150, 450, n)
        angs = (rng.uniform(0, 2 * np.pi, n)[:, None] + agent.angle_offsets[None, :]) % (2 * np.pi)
        banks = (np.arange(n) % N_BANKS).astype(np.int32)
        eng.mbank_train_from_poses(xs, ys, angs[:, A // 2].copy(), banks, want_views=False)   # (some weights at 0 in every bank)

        def banked():
            eng.timer_start()
            for _ in range(n_calls):
                res = eng.mbank_sense_step_batch(xs, ys, angs, banks)
            return eng.timer_stop() * 1e3 / n_calls, res          # us per ensemble step

        def unbanked():
            eng.timer_start()
            for _ in range(n_calls):
                eng.mb_sense_step_batch(xs, ys, angs)
            return eng.timer_stop() * 1e3 / n_calls

        _, res = banked()                                         # warm-up of both (code load, clocks, the buffers)
        unbanked()
        assert not res.flags.any() and res.angle_familiarity.max() == 0.0 and res.angle_familiarity.min() < 0
        tb, tu = [], []
        for _ in range(reps):                                     # alternating windows
            tb.append(banked()[0])
            tu.append(unbanked())
        out["layouts"].append(dict(members=n, headings=A, banked_us_per_step=spread(tb), unbanked_us_per_step=spread(tu),
                                   banked_over_unbanked=round(float(np.median(tb) / np.median(tu)), 3)))
        eng.close()
    # training: N_BANKS routes in one banked call on one engine, against one call per route on an engine each
    engines = [NavBySceneFamiliarity(land, (side, side), 1.0, n_test_angles=HEADINGS[0], familiarity_model=mushroom_familiarity())._engine
               for _ in range(N_BANKS)]
    rng = np.random.default_rng(side + 7)
    total = N_BANKS * n_views
    xs, ys, angs = rng.uniform(150, 450, total), rng.uniform(150, 450, total), rng.uniform(0, 2 * np.pi, total)
    bank_of = np.repeat(np.arange(N_BANKS, dtype=np.int32), n_views)

    def one_call():
        eng = engines[0]
        eng.mb_begin(side, side, conn, N_ACTIVE, 2)
        eng.mbank_set(N_BANKS)
        eng.timer_start()
        eng.mbank_train_from_poses(xs, ys, angs, bank_of, want_views=False)
        return eng.timer_stop() * 1e3

    def call_per_route():
        t = 0.0
        for r, eng in enumerate(engines):
            eng.mb_begin(side, side, conn, N_ACTIVE, 2)
            sl = slice(r * n_views, (r + 1) * n_views)
            eng.timer_start()
            eng.mb_train_from_poses(xs[sl], ys[sl], angs[sl], want_views=False)
            t += eng.timer_stop() * 1e3
        return t

    one_call()
    zeros = engines[0].mbank_info()["n_depressed"].tolist()
    call_per_route()
    assert zeros == [e.mb_info()["n_depressed"] for e in engines] and all(0 < z <= K for z in zeros)
    t1, t4 = [], []
    for _ in range(reps):
        t1.append(one_call())
        t4.append(call_per_route())
    out["train"] = dict(routes=N_BANKS, views_per_route=n_views, one_banked_call_us=spread(t1), call_per_route_us=spread(t4),
                        per_route_over_banked=round(float(np.median(t4) / np.median(t1)), 3), n_depressed=zeros)
    for e in engines:
        e.close()
    print(json.dumps(out))


LAND_SHAPES = ((600, 600), (560, 600), (600, 540), (600, 600))     # rows, cols: the poses lie inside all of them


def lands_child(side, n_views, n_calls, reps):
    """The lands block of one size on the GPU -> one JSON line on stdout."""
    from navsim_amd import NavBySceneFamiliarity, mushroom_familiarity, synth
    from navsim_amd.util import mushroom_connectivity
    N = side * side
    lands = [np.ascontiguousarray(synth.synth_landscape(3 + l, 600, 4)[:r, :c]) for l, (r, c) in enumerate(LAND_SHAPES)]
    L = len(lands)
    out = dict(side=side, N=N, n_kc=K, fan_in=FAN_IN, n_active=N_ACTIVE, n_banks=N_BANKS, n_lands=L, land_shapes=LAND_SHAPES,
               calls_per_window=n_calls, views_per_route=n_views, layouts=[])
    conn = mushroom_connectivity(K, N, FAN_IN, 0)

    def engine(land, A):
        agent = NavBySceneFamiliarity(land, (side, side), 1.0, n_test_angles=A, familiarity_model=mushroom_familiarity())
        agent._engine.mb_begin(side, side, conn, N_ACTIVE, 2)
        agent._engine.mbank_set(N_BANKS)
        return agent, agent._engine                              # (landscape and sensor attached)

    for n, A in ENSEMBLES:
        agent, eng = engine(lands[0], A)
        eng.lands_set(lands)
        rng = np.random.default_rng(n * 100 + A)
        xs, ys = rng.uniform(150, 390, n), rng.uniform(150, 390, n)
        angs = (rng.uniform(0, 2 * np.pi, n)[:, None] + agent.angle_offsets[None, :]) % (2 * np.pi)
        banks = (np.arange(n) % N_BANKS).astype(np.int32)
        land_of = (3 * np.arange(n) % L).astype(np.int32)
        eng.mbank_train_from_poses(xs, ys, angs[:, A // 2].copy(), banks, want_views=False, land_of_view=land_of)   # (some weights at 0)
        four = [engine(lands[l], A)[1] for l in range(L)]
        for e in four:
            for r in range(N_BANKS):
                e.mbank_set_weights(r, eng.mbank_read_weights(r))
        mine = [np.flatnonzero(land_of == l) for l in range(L)]
        parts = [(four[l], xs[m].copy(), ys[m].copy(), angs[m].copy(), banks[m].copy()) for l, m in enumerate(mine)]

        def on_set():
            w0 = time.perf_counter()
            eng.timer_start()
            for _ in range(n_calls):
                res = eng.mbank_sense_step_batch(xs, ys, angs, banks, land_of_member=land_of)
            return eng.timer_stop() * 1e3 / n_calls, (time.perf_counter() - w0) * 1e6 / n_calls, res

        def one_landscape():
            eng.timer_start()
            for _ in range(n_calls):
                eng.mbank_sense_step_batch(xs, ys, angs, banks)
            return eng.timer_stop() * 1e3 / n_calls

        def four_engines():
            w0 = time.perf_counter()
            for _ in range(n_calls):
                rows = [e.mbank_sense_step_batch(x, y, a, b) for e, x, y, a, b in parts]
            return (time.perf_counter() - w0) * 1e6 / n_calls, rows

        _, _, res = on_set()                                      # warm-up of all three (code load, clocks, the buffers)
        one_landscape()
        _, rows = four_engines()
        assert not res.flags.any() and res.angle_familiarity.min() < 0
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
    # training: L routes on L landscapes in one call on one engine, against one call per route on an engine each
    engines = [engine(lands[l], HEADINGS[0])[1] for l in range(L)]
    engines[0].lands_set(lands)
    rng = np.random.default_rng(side + 7)
    total = L * n_views
    xs, ys, angs = rng.uniform(150, 390, total), rng.uniform(150, 390, total), rng.uniform(0, 2 * np.pi, total)
    route_of = np.repeat(np.arange(L, dtype=np.int32), n_views)

    def one_call():
        eng = engines[0]
        eng.mbank_set(N_BANKS)
        w0 = time.perf_counter()
        eng.timer_start()
        eng.mbank_train_from_poses(xs, ys, angs, route_of, want_views=False, land_of_view=route_of)
        return eng.timer_stop() * 1e3, (time.perf_counter() - w0) * 1e6

    def call_per_route():
        t = wall = 0.0
        for r, eng in enumerate(engines):
            eng.mbank_set(1)
            sl = slice(r * n_views, (r + 1) * n_views)
            w0 = time.perf_counter()
            eng.timer_start()
            eng.mb_train_from_poses(xs[sl], ys[sl], angs[sl], want_views=False)
            t += eng.timer_stop() * 1e3
            wall += (time.perf_counter() - w0) * 1e6
        return t, wall

    one_call()
    zeros = engines[0].mbank_info()["n_depressed"].tolist()
    call_per_route()
    assert zeros == [e.mb_info()["n_depressed"] for e in engines] and all(0 < z <= K for z in zeros)
    t1, t4, w1, w4 = [], [], [], []
    for _ in range(reps):
        a, b = one_call()
        t1.append(a)
        w1.append(b)
        a, b = call_per_route()
        t4.append(a)
        w4.append(b)
    out["train"] = dict(routes=L, views_per_route=n_views, one_lands_call_us=spread(t1), call_per_route_us=spread(t4),
                        per_route_over_lands=round(float(np.median(t4) / np.median(t1)), 3), one_lands_call_wall_us=spread(w1),
                        call_per_route_wall_us=spread(w4), per_route_over_lands_wall=round(float(np.median(w4) / np.median(w1)), 3),
                        n_depressed=zeros)
    for e in engines:
        e.close()
    print(json.dumps(out))


METRIC_ROUTES, METRIC_MEMBERS, METRIC_HEADINGS, METRIC_SIDE = 4, 8, 16, 32
METRIC_POINTS = (3500, 50000)


def metrics_child(n_calls, reps):
    """The metrics block on the GPU -> one JSON line on stdout."""
    from navsim_amd import MushroomRouteEnsemble, NavBySceneFamiliarity, mushroom_familiarity, synth
    land = synth.synth_landscape(3, 600, 4)
    out = dict(side=METRIC_SIDE, routes=METRIC_ROUTES, members=METRIC_ROUTES * METRIC_MEMBERS, headings=METRIC_HEADINGS, n_kc=K,
               steps_per_window=n_calls, timer="wall clock (time.perf_counter) around ens.step_forward(), median of %d windows" % reps, sizes=[])
    for target in METRIC_POINTS:
        # the curve of curveness c over x in [100, 500] is 400 sqrt(2) long and a little more: arclen to reach `target` points
        routes = [synth.sin_training_path(c, 100, 400, arclen=400 * np.sqrt(2.0) / target) for c in (0.0, 0.2, 0.4, 0.6)]
        starts = []
        for r, route in enumerate(routes):
            for m in range(METRIC_MEMBERS):
                k = (1 + m) * len(route) // (4 * METRIC_MEMBERS)                        # along the route's first quarter
                d = route[k + 1] - route[k]
                starts.append((r, (float(route[k][0] + 0.3), float(route[k][1] - 0.2)), float(np.arctan2(d[1], d[0]) % (2 * np.pi))))
        ens = {}
        for mode in ("host", "device"):
            agent = NavBySceneFamiliarity(land, (METRIC_SIDE, METRIC_SIDE), 1.0, n_test_angles=METRIC_HEADINGS, familiarity_model=mushroom_familiarity())
            ens[mode] = MushroomRouteEnsemble.from_routes_with(agent, routes, starts, metrics=mode)

        def window(e):
            t0 = time.perf_counter()
            for _ in range(n_calls):
                e.step_forward()
            return (time.perf_counter() - t0) * 1e6 / n_calls                          # us per ensemble step

        for mode in ("host", "device"):                                                 # warm-up of both (code load, clocks, the buffers)
            window(ens[mode])
        t = dict(host=[], device=[])
        for _ in range(reps):                                                           # alternating windows, both at the same poses
            for mode in ("host", "device"):
                t[mode].append(window(ens[mode]))
        running = [len(ens[mode].active) for mode in ("host", "device")]
        same = all(a.position == b.position and a.navigation_error == b.navigation_error and a.percent_recapitulated == b.percent_recapitulated
                   for a, b in zip(ens["host"].agents, ens["device"].agents))
        assert same and running[0] == running[1], (same, running)                      # (both modes walked the same poses to the same marks)
        # the routed call alone, at the members' last positions (its marks are the ensemble's own: measured last)
        dev = ens["device"]
        slots = np.arange(len(starts), dtype=np.int32)
        xs = np.array([a.position[0] for a in dev.agents])
        ys = np.array([a.position[1] for a in dev.agents])
        reach = np.array([a.coverage_threshold_factor * a.step_size for a in dev.agents])

        def call_window():
            t0 = time.perf_counter()
            for _ in range(n_calls):
                dev.engine.path_routes_error(slots, xs, ys, reach)
            return (time.perf_counter() - t0) * 1e6 / n_calls

        call_window()
        tc = [call_window() for _ in range(reps)]
        out["sizes"].append(dict(route_points=[len(r) for r in routes], host_us_per_step=spread(t["host"]), device_us_per_step=spread(t["device"]),
                                 host_over_device=round(float(np.median(t["host"]) / np.median(t["device"])), 3),
                                 path_routes_error_us_per_call=spread(tc), members_running=running[1]))
        for e in ens.values():
            e.agents[0].clear_training()
            e.engine.close()
    print(json.dumps(out))


def rows_child(n_frames, reps):
    """The rows block on the GPU -> one JSON line on stdout."""
    from navsim_amd import MushroomRouteEnsemble, NavBySceneFamiliarity, mushroom_familiarity, synth
    from navsim_amd.experiment import N_CONSECUTIVE_SCENES as FRAC
    land = synth.synth_landscape(3, 600, 4)
    summary_builds = 20
    out = dict(side=METRIC_SIDE, routes=METRIC_ROUTES, members=METRIC_ROUTES * METRIC_MEMBERS, headings=METRIC_HEADINGS, n_kc=K,
               frames_stepped=n_frames, n_consecutive_scenes=FRAC,
               timer="wall clock (time.perf_counter) around the build of all members' coverage columns, median of %d windows; "
                     "a window is 1 build by the three methods, %d by coverage_summary" % (reps, summary_builds), sizes=[])
    for target in METRIC_POINTS:
        routes = [synth.sin_training_path(c, 100, 400, arclen=400 * np.sqrt(2.0) / target) for c in (0.0, 0.2, 0.4, 0.6)]
        starts = []
        for r, route in enumerate(routes):
            for m in range(METRIC_MEMBERS):
                k = (1 + m) * len(route) // (4 * METRIC_MEMBERS)                        # along the route's first quarter
                d = route[k + 1] - route[k]
                starts.append((r, (float(route[k][0] + 0.3), float(route[k][1] - 0.2)), float(np.arctan2(d[1], d[0]) % (2 * np.pi))))
        agent = NavBySceneFamiliarity(land, (METRIC_SIDE, METRIC_SIDE), 1.0, n_test_angles=METRIC_HEADINGS, familiarity_model=mushroom_familiarity())
        ens = MushroomRouteEnsemble.from_routes_with(agent, routes, starts, metrics="device")
        for _ in range(n_frames):
            ens.step_forward()
        eng = ens.engine

        def by_methods():
            t0 = time.perf_counter()
            rows = [{"path_coverage": a.percent_recapitulated, "percent_forgiving": a.percent_recapitulated_forgiving(n_consecutive_scenes=FRAC),
                     "n_captures": a.n_captures(n_consecutive_scenes=FRAC)} for a in ens.agents]
            return (time.perf_counter() - t0) * 1e6, rows

        def by_summary():
            t0 = time.perf_counter()
            for _ in range(summary_builds):
                rows = ens.coverage_summary(FRAC)
            return (time.perf_counter() - t0) * 1e6 / summary_builds, rows

        def copies():
            t0 = time.perf_counter()
            for a in ens.agents:
                for _ in range(3):
                    eng.path_routes_coverage(a._metric_slot, len(a.training_path))
            return (time.perf_counter() - t0) * 1e6

        slots = np.arange(len(ens.agents), dtype=np.int32)
        wins = np.array([a._window(FRAC) for a in ens.agents], dtype=np.int64)

        def call_alone():
            eng.timer_start()
            for _ in range(summary_builds):
                eng.marks_summary_routes(slots, wins)
            return eng.timer_stop() * 1e3 / summary_builds

        _, rows_a = by_methods()                                                        # warm-up of all (code load, clocks, the buffers)
        _, rows_b = by_summary()
        copies()
        call_alone()
        assert rows_a == rows_b, "the two builds differ"
        ta, tb, tc, td = [], [], [], []
        for _ in range(reps):                                                           # alternating windows, the same marks
            ta.append(by_methods()[0])
            tb.append(by_summary()[0])
            tc.append(copies())
            td.append(call_alone())
        covered = [r["path_coverage"] for r in rows_b]
        out["sizes"].append(dict(route_points=[len(r) for r in routes], windows=sorted(set(wins.tolist())),
                                 three_methods_us_per_build=spread(ta), coverage_summary_us_per_build=spread(tb),
                                 methods_over_summary=round(float(np.median(ta) / np.median(tb)), 1),
                                 coverage_copies_alone_us=spread(tc), marks_summary_routes_event_us_per_call=spread(td),
                                 path_coverage_min_max=[round(float(min(covered)), 4), round(float(max(covered)), 4)],
                                 members_running=len(ens.active), rows_equal=True))
        ens.agents[0].clear_training()
        eng.close()
    print(json.dumps(out))


def cpu_row(side, n_calls):
    """The NumPy statement on this host: wall clock, microseconds per call that scores A patches."""
    from tests import helpers_mushroom as H
    N = side * side
    conn = H.connectivity(K, N, FAN_IN, 0)
    wt = H.train(np.ones(K, np.uint8), H.route_views(1, 8, side, side), conn, N_ACTIVE)
    row = {}
    for A in HEADINGS:
        patches = H.route_views(2, A, side, side)
        t0 = time.perf_counter()
        for _ in range(n_calls):
            H.familiarity(wt, patches, conn, N_ACTIVE)
        row["score_us_per_call_A%d" % A] = round((time.perf_counter() - t0) * 1e6 / n_calls, 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", default="32,64")
    ap.add_argument("--views", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed to each GPU child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mushroom_time.json"))
    ap.add_argument("--blocks", default="single,ensemble", help="which blocks to measure: single (training and the agent step), ensemble, banks, metrics, lands, rows, sensors, populations, noise, sets")
    ap.add_argument("--ensemble-calls", type=int, default=30, help="ensemble steps per timed window")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--ensemble-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--banks-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--metrics-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--lands-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--rows-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--row-frames", type=int, default=300, help="frames the rows block steps its ensemble before it builds the rows")
    args = ap.parse_args()
    if args.child:
        gpu_child(args.child, args.views, args.calls, args.reps)
        return 0
    if args.ensemble_child:
        ensemble_child(args.ensemble_child, args.ensemble_calls, args.reps)
        return 0
    if args.banks_child:
        banks_child(args.banks_child, args.views, args.ensemble_calls, args.reps)
        return 0
    if args.metrics_child:
        metrics_child(args.ensemble_calls, args.reps)
        return 0
    if args.lands_child:
        lands_child(args.lands_child, args.views, args.ensemble_calls, args.reps)
        return 0
    if args.rows_child:
        rows_child(args.row_frames, args.reps)
        return 0
    blocks = args.blocks.split(",")
    result = dict(tool="tools/mushroom_time.py", timer="hipEvent pair (dv_timer_start/stop), median of %d windows after a warm-up" % args.reps,
                  sizes=[], ensembles=[], banks=[], metrics=[], lands=[], rows=[], sensors=[], populations=[], noise=[], sets=[])
    if os.path.exists(args.out):                                  # a block that is not measured keeps its rows
        with open(args.out) as f:
            kept = json.load(f)
        for block, key in (("single", "sizes"), ("ensemble", "ensembles"), ("banks", "banks"), ("metrics", "metrics"), ("lands", "lands"), ("rows", "rows"),
                           ("sensors", "sensors"), ("populations", "populations"), ("noise", "noise"), ("sets", "sets")):
            if block not in blocks:
                result[key] = kept.get(key, [])
    for side in [int(x) for x in args.sides.split(",")] if "ensemble" in blocks else []:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--ensemble-child", str(side),
               "--ensemble-calls", str(args.ensemble_calls), "--reps", str(args.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if p.returncode != 0:
            print("GPU measurement of the ensembles of side %d ended with status %d: nothing more is run" % (side, p.returncode), file=sys.stderr)
            return p.returncode
        result["ensembles"].append(json.loads(p.stdout.strip().splitlines()[-1]))
    for side in [int(x) for x in args.sides.split(",")] if "banks" in blocks else []:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--banks-child", str(side), "--views", str(args.views),
               "--ensemble-calls", str(args.ensemble_calls), "--reps", str(args.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if p.returncode != 0:
            print("GPU measurement of the banks of side %d ended with status %d: nothing more is run" % (side, p.returncode), file=sys.stderr)
            return p.returncode
        result["banks"].append(json.loads(p.stdout.strip().splitlines()[-1]))
    for side in [int(x) for x in args.sides.split(",")] if "lands" in blocks else []:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--lands-child", str(side), "--views", str(args.views),
               "--ensemble-calls", str(args.ensemble_calls), "--reps", str(args.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if p.returncode != 0:
            print("GPU measurement of the landscape sets of side %d ended with status %d: nothing more is run" % (side, p.returncode), file=sys.stderr)
            return p.returncode
        result["lands"].append(json.loads(p.stdout.strip().splitlines()[-1]))
    if "sensors" in blocks:
        import sensors_block
        rc, row = sensors_block.run_child(args.limit, args.ensemble_calls, args.reps, "mushroom")
        if rc != 0:
            return rc
        result["sensors"].append(row)
    if "noise" in blocks:
        import noise_block
        rc, row = noise_block.run_child(args.limit, [int(x) for x in args.sides.split(",")], args.ensemble_calls, args.reps, "mushroom")
        if rc != 0:
            return rc
        result["noise"].append(row)
    for side in [int(x) for x in args.sides.split(",")] if "populations" in blocks else []:
        import populations_block
        rc, row = populations_block.run_child(args.limit, side, args.views, args.ensemble_calls, args.reps)
        if rc != 0:
            return rc
        result["populations"].append(row)
    for side in [int(x) for x in args.sides.split(",")] if "sets" in blocks else []:
        import sets_block
        rc, row = sets_block.run_child(args.limit, side, args.views, args.ensemble_calls, args.reps)
        if rc != 0:
            return rc
        result["sets"].append(row)
    if "metrics" in blocks:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--metrics-child", "1",
               "--ensemble-calls", str(args.ensemble_calls), "--reps", str(args.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if p.returncode != 0:
            print("GPU measurement of the route ensembles' metrics ended with status %d: nothing more is run" % p.returncode, file=sys.stderr)
            return p.returncode
        result["metrics"].append(json.loads(p.stdout.strip().splitlines()[-1]))
    if "rows" in blocks:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--rows-child", "1",
               "--row-frames", str(args.row_frames), "--reps", str(args.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if p.returncode != 0:
            print("GPU measurement of the result rows ended with status %d: nothing more is run" % p.returncode, file=sys.stderr)
            return p.returncode
        result["rows"].append(json.loads(p.stdout.strip().splitlines()[-1]))
    for side in [int(x) for x in args.sides.split(",")] if "single" in blocks else []:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", str(side), "--views", str(args.views),
               "--calls", str(args.calls), "--reps", str(args.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if p.returncode != 0:
            print("GPU measurement of side %d ended with status %d: nothing more is run" % (side, p.returncode), file=sys.stderr)
            return p.returncode
        row = json.loads(p.stdout.strip().splitlines()[-1])
        row["numpy_cpu"] = cpu_row(side, 3)
        result["sizes"].append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
