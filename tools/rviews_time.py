#!/usr/bin/env python3
"""Times a step of the route view store (dv_rviews_sense_step, navsim_amd.SadsRouteEnsemble) at a slice of the reference's grid and
writes profiles/rviews_time.json.

    python tools/rviews_time.py [--sides 32,64] [--calls 30] [--reps 5] [--blocks routes[,sensors][,noise][,window][,reloc][,ssd][,ssdwin][,ncc]] [--out profiles/rviews_time.json]

Shape: 4 routes x 8 starts x 10 headings = 32 trials of 320 columns, views of side x side.  The routes have the grid's length:
synth.sin_training_path with arclen = step_size / n_test_angles (scripts/run_experiment.py:207) on a 900 x 900 landscape, one curve
a route.  Per side, medians (and the spread) of --reps alternating windows of --calls steps in one process:

  routed_call_us        the routed call alone (dv_rviews_sense_step for all 32 members at fixed poses), by a hipEvent pair
  routed_exact_call_us  the same call in its exact form (every view as the reference's sequential double sum)
  ensemble_step_wall_us SadsRouteEnsemble.step_forward(fake=True), wall clock: the call and the host's share of a step
  four_engines_wall_us  the same 32 trials as four NavEnsembles on four engines (a library a route) stepped in turn, wall clock --
                        what there was before the store; four streams have no common event pair
  four_engines_over_routed_wall   the ratio of the two wall-clock medians, whichever way it falls

The routed call's rows are checked against the four engines' rows before anything is timed (same best headings, scores within 1e-12
relative: the engines score in their default mode).  A window without a GPU fails; nothing here falls back.

Sensors block (--blocks sensors): dv_rviews_sense_step with a landscape per member on a set of 4 landscapes, without a sensor table,
with a table of four entries equal to the engine's sensor and with a table of four different entries, in alternating windows of one
process (tools/sensors_block.py, which states the shape and the figures); its rows are the file's "sensors".  A block that is not
measured keeps its rows.

Noise block (--blocks noise): dv_rviews_sense_step on the same set without noise rows, under rows of zero amplitude, under rows of
amplitude 20, and with the rows set again before every step as a route ensemble sets them, in alternating windows of one process
(tools/noise_block.py, which states the shape and the figures); its rows are the file's "noise".

Window block (--blocks window): the same slice with every member under a temporal window (dv_rvwin_sense_step: one fused scoring
launch), WINDOWS = (50, 50) and (255, 256) centred on each pose's nearest route point, against the unwindowed dv_rviews_sense_step at
the same poses, in alternating windows of one process: per side unwindowed_call_us and, per window, windowed_call_us /
windowed_exact_call_us (hipEvent pairs), ensemble_step_wall_us (SadsRouteEnsemble(window=...).step_forward(fake=True), wall clock) and
the two ratios; uncut_101_views_call_us is the 101-view call with the kernel's pixel cut switched off (DEJAVU_RVWIN_SPLIT=0).  The fast
and exact forms, and the cut and uncut kernels, are checked to agree on their bits before anything is timed.  The block is the file's
"window" key; measured alone it leaves every other key as it was.

Reloc block (--blocks reloc): the same slice under a window of 101 views with the loss test inside the call (dv_rvreloc_sense_step,
rvwin_sense_step(reloc_below=...)), in alternating windows of one process, hipEvent pairs: windowed_call_us (dv_rvwin_sense_step, no
thresholds), reloc_none_lost_call_us (every threshold -inf: the price of the planning launch and the empty worst-case grids),
reloc_4_lost_call_us (one member a route at +inf) and reloc_all_lost_call_us (all 32), against the host's way at the same poses --
host_4_lost_call_us / host_all_lost_call_us: the windowed call, then rviews_sense_step on the lost members (two enqueues, two waits, the
lost members sensed twice) -- and unwindowed_call_us.  The device's and the host's way are checked to agree on their bits before
anything is timed.  The block is the file's "reloc" key; measured alone it leaves every other key as it was.

SSD block (--blocks ssd): the same slice scored as exact SSD of one channel on the int8 matrix cores (dv_rvssd_sense_step) against the
perfect-memory call (dv_rviews_sense_step) at the same poses on the SAME engine and store, in alternating windows of one process, hipEvent
pairs: ssd_call_us and sads_call_us, their ratio, and ensemble_step_wall_us (SsdRouteEnsemble.step_forward(fake=True), wall clock).  Two
members' rows are checked against a NumPy int64 statement on the store's own views before anything is timed.  The block is the file's
"ssd" key; measured alone it leaves every other key as it was.

SSD window block (--blocks ssdwin): the same slice as exact SSD under a temporal window (dv_rvssdw_sense_step), SSDWIN_WINDOWS =
(50, 50) and (255, 256) centred on each pose's nearest route point, against the unwindowed dv_rvssd_sense_step at the same poses on the
same engine and store, in alternating windows of one process, hipEvent pairs: unwindowed_call_us and, per window, windowed_call_us and
its ratio; under the 101-view window the call with thresholds -- reloc_none_lost_call_us (every threshold -inf: the price of the
planning launch, the cleared keys and the empty worst-case grid), reloc_4_lost_call_us (one member a route at +inf) and
reloc_all_lost_call_us -- and ensemble_step_wall_us per window (SsdRouteEnsemble(window=...).step_forward(fake=True), wall clock) beside
the unwindowed ensemble's.  Whole-route windows on the shortest prefix, and the lost members' rows against the unwindowed call, are
checked on their bits before anything is timed.  The block is the file's "ssdwin" key; measured alone it leaves every other key as it
was.

NCC block (--blocks ncc): the same slice scored by the correlation coefficient (dv_rvncc_sense_step) against exact SSD
(dv_rvssd_sense_step) at the same poses on the SAME engine and store, in alternating windows of one process, hipEvent pairs:
ncc_call_us and ssd_call_us, their ratio, and ensemble_step_wall_us (NccRouteEnsemble.step_forward(fake=True), wall clock).  Two
members' rows are checked on their bits against the NumPy statement on the store's own views before anything is timed.  The two scoring
kernels' own times come from a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/rviews_time.py --ncc-trace-run --sides 32
    python tools/rviews_time.py --ncc-trace-stats DIR --sides 32   (the *kernel_stats.csv files under DIR -> the block's "kernel_trace" key,
                                                                     a side at a time: a trace's rows do not tell the sizes apart)
The block is the file's "ncc" key; measured alone it leaves every other key as it was."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "navigation-by-deja-vu_amd"))
sys.path.insert(0, ROOT)

CURVES = (0.0, 0.2, 0.35, 0.5)
STARTS_PER_ROUTE, HEADINGS, STEP_SIZE, CHEM_WEIGHT, LAND = 8, 10, 2.0, 0.25, 900


def spread(samples):
    return dict(median=round(float(np.median(samples)), 3), min=round(float(min(samples)), 3), max=round(float(max(samples)), 3))


def starts_of(routes):
    """8 starts a route: beside points spread along it, looking along the route with a small offset."""
    out = []
    for r, path in enumerate(routes):
        for k in range(STARTS_PER_ROUTE):
            i = (k + 1) * len(path) // (STARTS_PER_ROUTE + 2)
            d = path[i + 1] - path[i]
            out.append((r, (float(path[i][0] + 0.7 * (k % 3 - 1)), float(path[i][1] - 0.5 * (k % 2))), float(np.arctan2(d[1], d[0]) % (2 * np.pi)) + 0.05 * k))
    return out


def measure(side, n_calls, reps):
    import navsim_amd
    from navsim_amd import synth
    land = synth.synth_landscape(3, LAND, 4)
    routes = [synth.sin_training_path(c, 0.2 * LAND, 0.6 * LAND, arclen=STEP_SIZE / HEADINGS) for c in CURVES]
    starts = starts_of(routes)

    def agent():
        return navsim_amd.NavBySceneFamiliarity(land, (side, side), STEP_SIZE, n_test_angles=HEADINGS, track_scene_familiarity=False,
                                                familiarity_model=navsim_amd.sads_familiarity(CHEM_WEIGHT))

    t0 = time.perf_counter()
    ens = navsim_amd.SadsRouteEnsemble.from_routes_with(agent(), routes, starts, metrics="device")
    ens.engine.synchronize()
    train_routed_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    four = []
    for r, path in enumerate(routes):
        a = agent()
        a.train_from_path(path)
        four.append(navsim_amd.NavEnsemble.from_agent(a, [(pos, ang) for rr, pos, ang in starts if rr == r]))
        a._engine.synchronize()
    train_four_s = time.perf_counter() - t0
    eng = ens.engine
    n = len(starts)
    xs = np.array([p[0] for _, p, _ in starts])
    ys = np.array([p[1] for _, p, _ in starts])
    angs = (np.array([a for _, _, a in starts])[:, None] + ens.agents[0].angle_offsets[None, :]) % (2 * np.pi)
    route_of = np.array([r for r, _, _ in starts], dtype=np.int32)
    weights = np.full(n, CHEM_WEIGHT)
    mine = [np.flatnonzero(route_of == r) for r in range(len(routes))]

    def routed(exact=False):
        eng.timer_start()
        for _ in range(n_calls):
            res = eng.rviews_sense_step(xs, ys, angs, route_of, weights, exact=exact)
        return eng.timer_stop() * 1e3 / n_calls, res

    def ensemble_steps():
        w0 = time.perf_counter()
        for _ in range(n_calls):
            ens.step_forward(fake=True)
        return (time.perf_counter() - w0) * 1e6 / n_calls

    def four_engines():
        w0 = time.perf_counter()
        for _ in range(n_calls):
            for e in four:
                e.step_forward(fake=True)
        return (time.perf_counter() - w0) * 1e6 / n_calls

    _, res = routed()                                             # warm-up of every form (code load, clocks, the buffers)
    _, res_exact = routed(True)
    assert np.array_equal(res.angle_familiarity.view(np.uint64), res_exact.angle_familiarity.view(np.uint64))
    assert np.array_equal(res.angle_view, res_exact.angle_view) and np.array_equal(res.best_idex, res_exact.best_idex) and not res.flags.any()
    for r, m in enumerate(mine):                                  # the same decisions as an engine that holds that route's library alone
        got = four[r].engine.sense_step_batch(xs[m], ys[m], angs[m])
        assert np.array_equal(got.best_idex, res.best_idex[m])
        np.testing.assert_allclose(got.angle_familiarity, res.angle_familiarity[m], rtol=1e-12, atol=0)
    ensemble_steps()
    four_engines()
    assert len(ens.active) == n and all(len(e.active) == len(m) for e, m in zip(four, mine))
    tr, te, ws, w4 = [], [], [], []
    for _ in range(reps):                                         # alternating windows
        tr.append(routed()[0])
        te.append(routed(True)[0])
        ws.append(ensemble_steps())
        w4.append(four_engines())
    info = eng.rviews_info()
    out = dict(side=side, routes=len(routes), route_views=[len(r) for r in routes], members=n, headings=HEADINGS, columns=n * HEADINGS,
               chem_weight=CHEM_WEIGHT, calls_per_window=n_calls, windows=reps, store_bytes=info["bytes"],
               routed_call_us=spread(tr), routed_exact_call_us=spread(te), ensemble_step_wall_us=spread(ws),
               four_engines_wall_us=spread(w4), four_engines_over_routed_wall=round(float(np.median(w4) / np.median(ws)), 3),
               train_routed_s=round(train_routed_s, 3), train_four_engines_s=round(train_four_s, 3))
    for e in [ens] + four:
        e.engine.close()
    return out


WINDOWS = ((50, 50), (255, 256))


def measure_window(side, n_calls, reps):
    """The window block's row of one side: the routed call without a window against dv_rvwin_sense_step under WINDOWS, at the same
    poses, every window centred on its pose's nearest route point."""
    import navsim_amd
    from navsim_amd import synth
    land = synth.synth_landscape(3, LAND, 4)
    routes = [synth.sin_training_path(c, 0.2 * LAND, 0.6 * LAND, arclen=STEP_SIZE / HEADINGS) for c in CURVES]
    starts = starts_of(routes)
    centres = [int(np.argmin(np.linalg.norm(routes[r] - np.array(pos), axis=1))) for r, pos, _ in starts]

    def ensemble(window, split=True):
        if not split:
            os.environ["DEJAVU_RVWIN_SPLIT"] = "0"                # (read when the agent's engine is created)
        try:
            a = navsim_amd.NavBySceneFamiliarity(land, (side, side), STEP_SIZE, n_test_angles=HEADINGS, track_scene_familiarity=False,
                                                 familiarity_model=navsim_amd.sads_familiarity(CHEM_WEIGHT))
        finally:
            os.environ.pop("DEJAVU_RVWIN_SPLIT", None)
        return navsim_amd.SadsRouteEnsemble.from_routes_with(a, routes, starts, metrics="device", window=window,
                                                             window_centres=None if window is None else centres)

    plain = ensemble(None)
    windowed = [ensemble(w) for w in WINDOWS]
    uncut = ensemble(WINDOWS[0], split=False)
    n = len(starts)
    xs = np.array([p[0] for _, p, _ in starts])
    ys = np.array([p[1] for _, p, _ in starts])
    angs = (np.array([a for _, _, a in starts])[:, None] + plain.agents[0].angle_offsets[None, :]) % (2 * np.pi)
    route_of = np.array([r for r, _, _ in starts], dtype=np.int32)
    weights = np.full(n, CHEM_WEIGHT)
    lens = np.array([len(routes[r]) for r in route_of])
    bounds = [(np.maximum(0, np.array(centres) - b), np.minimum(lens, np.array(centres) + a + 1)) for b, a in WINDOWS]

    def call(eng, k=None, exact=False):
        eng.timer_start()
        for _ in range(n_calls):
            if k is None:
                res = eng.rviews_sense_step(xs, ys, angs, route_of, weights, exact=exact)
            else:
                res = eng.rvwin_sense_step(xs, ys, angs, route_of, weights, bounds[k][0], bounds[k][1], exact=exact)
        return eng.timer_stop() * 1e3 / n_calls, res

    def wall(ens):
        w0 = time.perf_counter()
        for _ in range(n_calls):
            ens.step_forward(fake=True)
        return (time.perf_counter() - w0) * 1e6 / n_calls

    call(plain.engine)                                            # warm-up of every form, and the forms agree
    for k, e in enumerate(windowed):
        _, fast = call(e.engine, k)
        _, exact = call(e.engine, k, exact=True)
        assert np.array_equal(fast.angle_familiarity.view(np.uint64), exact.angle_familiarity.view(np.uint64))
        assert np.array_equal(fast.angle_view, exact.angle_view) and np.array_equal(fast.best_idex, exact.best_idex) and not fast.flags.any()
        assert (fast.angle_view >= bounds[k][0][:, None]).all() and (fast.angle_view < bounds[k][1][:, None]).all()
    _, cut = call(windowed[0].engine, 0)
    _, whole = call(uncut.engine, 0)
    assert np.array_equal(cut.angle_familiarity.view(np.uint64), whole.angle_familiarity.view(np.uint64))
    for e in [plain, uncut] + windowed:
        wall(e)
    t_plain, t_uncut, w_plain = [], [], []
    t_win, t_exact, w_win = [[] for _ in WINDOWS], [[] for _ in WINDOWS], [[] for _ in WINDOWS]
    for _ in range(reps):                                         # alternating windows
        t_plain.append(call(plain.engine)[0])
        for k, e in enumerate(windowed):
            t_win[k].append(call(e.engine, k)[0])
            t_exact[k].append(call(e.engine, k, exact=True)[0])
        t_uncut.append(call(uncut.engine, 0)[0])
        w_plain.append(wall(plain))
        for k, e in enumerate(windowed):
            w_win[k].append(wall(e))
    rows = []
    for k, (b, a) in enumerate(WINDOWS):
        rows.append(dict(behind=b, ahead=a, views=int((bounds[k][1] - bounds[k][0]).max()), windowed_call_us=spread(t_win[k]),
                         windowed_exact_call_us=spread(t_exact[k]), ensemble_step_wall_us=spread(w_win[k]),
                         unwindowed_over_windowed_call=round(float(np.median(t_plain) / np.median(t_win[k])), 3),
                         unwindowed_over_windowed_wall=round(float(np.median(w_plain) / np.median(w_win[k])), 3),
                         members_running=len(windowed[k].active)))
    out = dict(side=side, routes=len(routes), route_views=[len(r) for r in routes], members=n, headings=HEADINGS, columns=n * HEADINGS,
               chem_weight=CHEM_WEIGHT, calls_per_window=n_calls, windows=reps, column_block=4, views_per_wave_chunk=64,
               unwindowed_call_us=spread(t_plain), unwindowed_ensemble_step_wall_us=spread(w_plain), members_running=len(plain.active),
               windowed=rows, uncut_101_views_call_us=spread(t_uncut))
    for e in [plain, uncut] + windowed:
        e.engine.close()
    return out


RELOC_WINDOW = (50, 50)


def measure_reloc(side, n_calls, reps):
    """The reloc block's row of one side."""
    import navsim_amd
    from navsim_amd import synth
    land = synth.synth_landscape(3, LAND, 4)
    routes = [synth.sin_training_path(c, 0.2 * LAND, 0.6 * LAND, arclen=STEP_SIZE / HEADINGS) for c in CURVES]
    starts = starts_of(routes)
    centres = np.array([int(np.argmin(np.linalg.norm(routes[r] - np.array(pos), axis=1))) for r, pos, _ in starts])
    a = navsim_amd.NavBySceneFamiliarity(land, (side, side), STEP_SIZE, n_test_angles=HEADINGS, track_scene_familiarity=False,
                                         familiarity_model=navsim_amd.sads_familiarity(CHEM_WEIGHT))
    ens = navsim_amd.SadsRouteEnsemble.from_routes_with(a, routes, starts, metrics="device", window=RELOC_WINDOW, window_centres=centres.tolist())
    eng = ens.engine
    n = len(starts)
    xs = np.array([p[0] for _, p, _ in starts])
    ys = np.array([p[1] for _, p, _ in starts])
    angs = (np.array([a for _, _, a in starts])[:, None] + ens.agents[0].angle_offsets[None, :]) % (2 * np.pi)
    route_of = np.array([r for r, _, _ in starts], dtype=np.int32)
    weights = np.full(n, CHEM_WEIGHT)
    lens = np.array([len(routes[r]) for r in route_of])
    lo, hi = np.maximum(0, centres - RELOC_WINDOW[0]), np.minimum(lens, centres + RELOC_WINDOW[1] + 1)
    four = np.arange(0, n, STARTS_PER_ROUTE)                     # one member a route
    taus = dict(none=np.full(n, -np.inf), four=np.where(np.isin(np.arange(n), four), np.inf, -np.inf), all=np.full(n, np.inf))
    lost_of = dict(four=four, all=np.arange(n))

    def device(which):
        eng.timer_start()
        for _ in range(n_calls):
            res = eng.rvwin_sense_step(xs, ys, angs, route_of, weights, lo, hi, reloc_below=None if which is None else taus[which])
        return eng.timer_stop() * 1e3 / n_calls, res

    def host(which):
        m = lost_of[which]
        eng.timer_start()
        for _ in range(n_calls):
            res = eng.rvwin_sense_step(xs, ys, angs, route_of, weights, lo, hi)
            again = eng.rviews_sense_step(xs[m], ys[m], angs[m], route_of[m], weights[m])
        return eng.timer_stop() * 1e3 / n_calls, res, again

    def unwindowed():
        eng.timer_start()
        for _ in range(n_calls):
            eng.rviews_sense_step(xs, ys, angs, route_of, weights)
        return eng.timer_stop() * 1e3 / n_calls

    _, plain = device(None)                                        # warm-up of every form, and the forms agree
    _, none = device("none")
    assert np.array_equal(none.angle_familiarity.view(np.uint64), plain.angle_familiarity.view(np.uint64)) and not none.flags.any()
    for which in ("four", "all"):
        _, got = device(which)
        _, win, again = host(which)
        m = lost_of[which]
        fam, view = win.angle_familiarity.copy(), win.angle_view.copy()
        fam[m], view[m] = again.angle_familiarity, again.angle_view
        assert np.array_equal(got.angle_familiarity.view(np.uint64), fam.view(np.uint64)) and np.array_equal(got.angle_view, view)
        assert np.array_equal(np.flatnonzero(got.relocalised), m)
    unwindowed()
    t = {k: [] for k in ("windowed", "none", "four", "all", "host_four", "host_all", "unwindowed")}
    for _ in range(reps):                                         # alternating windows
        t["windowed"].append(device(None)[0])
        for which in ("none", "four", "all"):
            t[which].append(device(which)[0])
        for which in ("four", "all"):
            t["host_" + which].append(host(which)[0])
        t["unwindowed"].append(unwindowed())
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = dict(side=side, routes=len(routes), route_views=[len(r) for r in routes], members=n, headings=HEADINGS, columns=n * HEADINGS,
               chem_weight=CHEM_WEIGHT, calls_per_window=n_calls, windows=reps, window_views=int((hi - lo).max()),
               windowed_call_us=spread(t["windowed"]), reloc_none_lost_call_us=spread(t["none"]), reloc_4_lost_call_us=spread(t["four"]),
               reloc_all_lost_call_us=spread(t["all"]), host_4_lost_call_us=spread(t["host_four"]), host_all_lost_call_us=spread(t["host_all"]),
               unwindowed_call_us=spread(t["unwindowed"]), none_lost_over_windowed=round(med["none"] / med["windowed"], 3),
               none_lost_minus_windowed_us=round(med["none"] - med["windowed"], 3),
               host_over_device_4_lost=round(med["host_four"] / med["four"], 3), host_over_device_all_lost=round(med["host_all"] / med["all"], 3))
    eng.close()
    return out


SSD_CHANNEL = 2


def measure_ssd(side, n_calls, reps):
    """The ssd block's row of one side."""
    import navsim_amd
    from navsim_amd import synth
    land = synth.synth_landscape(3, LAND, 4)
    routes = [synth.sin_training_path(c, 0.2 * LAND, 0.6 * LAND, arclen=STEP_SIZE / HEADINGS) for c in CURVES]
    starts = starts_of(routes)
    a = navsim_amd.NavBySceneFamiliarity(land, (side, side), STEP_SIZE, n_test_angles=HEADINGS, track_scene_familiarity=False,
                                         familiarity_model=navsim_amd.ssd_familiarity(SSD_CHANNEL))
    ens = navsim_amd.SsdRouteEnsemble.from_routes_with(a, routes, starts, metrics="device")
    eng = ens.engine
    n = len(starts)
    xs = np.array([p[0] for _, p, _ in starts])
    ys = np.array([p[1] for _, p, _ in starts])
    angs = (np.array([a for _, _, a in starts])[:, None] + ens.agents[0].angle_offsets[None, :]) % (2 * np.pi)
    route_of = np.array([r for r, _, _ in starts], dtype=np.int32)
    weights = np.full(n, CHEM_WEIGHT)

    def ssd():
        eng.timer_start()
        for _ in range(n_calls):
            res = eng.rvssd_sense_step(xs, ys, angs, route_of, SSD_CHANNEL)
        return eng.timer_stop() * 1e3 / n_calls, res

    def sads():
        eng.timer_start()
        for _ in range(n_calls):
            res = eng.rviews_sense_step(xs, ys, angs, route_of, weights)
        return eng.timer_stop() * 1e3 / n_calls, res

    def wall():
        w0 = time.perf_counter()
        for _ in range(n_calls):
            ens.step_forward(fake=True)
        return (time.perf_counter() - w0) * 1e6 / n_calls

    _, res = ssd()                                                # warm-up of both calls, and the SSD rows are the integers
    _, plain = sads()
    assert not res.flags.any() and not plain.flags.any()
    for i in (0, n - 1):
        lib = ens.agents[i].familiar_scenes[..., SSD_CHANNEL].reshape(len(routes[route_of[i]]), -1).astype(np.int64)
        pats = eng.sense(np.full(HEADINGS, xs[i]), np.full(HEADINGS, ys[i]), angs[i])[..., SSD_CHANNEL].reshape(HEADINGS, -1).astype(np.int64)
        rows = np.stack([((p[None, :] - lib) ** 2).sum(axis=1) for p in pats])
        assert np.array_equal(res.angle_ssd[i], rows.min(axis=1).astype(np.float64)) and np.array_equal(res.angle_view[i], rows.argmin(axis=1))
        assert res.best_idex[i] == int(np.argmin(rows.min(axis=1)))
    wall()
    assert len(ens.active) == n
    t_ssd, t_sads, w = [], [], []
    for _ in range(reps):                                         # alternating windows
        t_ssd.append(ssd()[0])
        t_sads.append(sads()[0])
        w.append(wall())
    info = eng.rviews_info()
    out = dict(side=side, routes=len(routes), route_views=[len(r) for r in routes], members=n, headings=HEADINGS, columns=n * HEADINGS,
               channel=SSD_CHANNEL, chem_weight=CHEM_WEIGHT, calls_per_window=n_calls, windows=reps, store_bytes=info["bytes"],
               tile_columns=32, view_groups_per_workgroup=4, ssd_call_us=spread(t_ssd), sads_call_us=spread(t_sads),
               ensemble_step_wall_us=spread(w), sads_over_ssd_call=round(float(np.median(t_sads) / np.median(t_ssd)), 3))
    eng.close()
    return out


def ncc_statement(lib, pats):
    """The correlation coefficient of every (patch, view) pair in NumPy: int64 sums, then one double product, one square root, one
    quotient and the clip; 0.0 where a plane is constant.  lib int64[L, P], pats int64[A, P] -> float64[A, L]."""
    P = lib.shape[1]
    sa, sb = pats.sum(axis=1), lib.sum(axis=1)
    num = P * (pats @ lib.T) - sa[:, None] * sb[None, :]
    va, vb = P * (pats * pats).sum(axis=1) - sa * sa, P * (lib * lib).sum(axis=1) - sb * sb
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.clip(num.astype(np.float64) / np.sqrt(va.astype(np.float64)[:, None] * vb.astype(np.float64)[None, :]), -1.0, 1.0)
    q[(va == 0)[:, None] | (vb == 0)[None, :]] = 0.0
    return q


def ncc_setup(side):
    """The ncc block's ensemble of one side and its step arguments."""
    import navsim_amd
    from navsim_amd import synth
    land = synth.synth_landscape(3, LAND, 4)
    routes = [synth.sin_training_path(c, 0.2 * LAND, 0.6 * LAND, arclen=STEP_SIZE / HEADINGS) for c in CURVES]
    starts = starts_of(routes)
    a = navsim_amd.NavBySceneFamiliarity(land, (side, side), STEP_SIZE, n_test_angles=HEADINGS, track_scene_familiarity=False,
                                         familiarity_model=navsim_amd.ncc_familiarity(SSD_CHANNEL))
    ens = navsim_amd.NccRouteEnsemble.from_routes_with(a, routes, starts, metrics="device")
    xs = np.array([p[0] for _, p, _ in starts])
    ys = np.array([p[1] for _, p, _ in starts])
    angs = (np.array([a for _, _, a in starts])[:, None] + ens.agents[0].angle_offsets[None, :]) % (2 * np.pi)
    route_of = np.array([r for r, _, _ in starts], dtype=np.int32)
    return ens, routes, xs, ys, angs, route_of


def measure_ncc(side, n_calls, reps):
    """The ncc block's row of one side."""
    ens, routes, xs, ys, angs, route_of = ncc_setup(side)
    eng = ens.engine
    n = len(xs)

    def ncc():
        eng.timer_start()
        for _ in range(n_calls):
            res = eng.rvncc_sense_step(xs, ys, angs, route_of, SSD_CHANNEL)
        return eng.timer_stop() * 1e3 / n_calls, res

    def ssd():
        eng.timer_start()
        for _ in range(n_calls):
            res = eng.rvssd_sense_step(xs, ys, angs, route_of, SSD_CHANNEL)
        return eng.timer_stop() * 1e3 / n_calls, res

    def wall():
        w0 = time.perf_counter()
        for _ in range(n_calls):
            ens.step_forward(fake=True)
        return (time.perf_counter() - w0) * 1e6 / n_calls

    _, res = ncc()                                                # warm-up of both calls, and the NCC rows are the statement's bits
    _, plain = ssd()
    assert not res.flags.any() and not plain.flags.any()
    for i in (0, n - 1):
        lib = ens.agents[i].familiar_scenes[..., SSD_CHANNEL].reshape(len(routes[route_of[i]]), -1).astype(np.int64)
        pats = eng.sense(np.full(HEADINGS, xs[i]), np.full(HEADINGS, ys[i]), angs[i])[..., SSD_CHANNEL].reshape(HEADINGS, -1).astype(np.int64)
        rows = ncc_statement(lib, pats)
        assert np.array_equal(res.angle_ncc[i].view(np.int64), rows.max(axis=1).view(np.int64)) and np.array_equal(res.angle_view[i], rows.argmax(axis=1))
        assert res.best_idex[i] == int(np.argmax(rows.max(axis=1)))
    wall()
    assert len(ens.active) == n
    t_ncc, t_ssd, w = [], [], []
    for _ in range(reps):                                         # alternating windows
        t_ncc.append(ncc()[0])
        t_ssd.append(ssd()[0])
        w.append(wall())
    info = eng.rviews_info()
    out = dict(side=side, routes=len(routes), route_views=[len(r) for r in routes], members=n, headings=HEADINGS, columns=n * HEADINGS,
               channel=SSD_CHANNEL, calls_per_window=n_calls, windows=reps, store_bytes=info["bytes"], tile_columns=32,
               view_groups_per_workgroup=4, ncc_call_us=spread(t_ncc), ssd_call_us=spread(t_ssd), ensemble_step_wall_us=spread(w),
               ncc_over_ssd_call=round(float(np.median(t_ncc) / np.median(t_ssd)), 3))
    eng.close()
    return out


def ncc_trace_run(sides, n_calls):
    """What the kernel trace watches: n_calls of each call a side, after a warm-up call of each."""
    for side in sides:
        ens, _, xs, ys, angs, route_of = ncc_setup(side)
        for _ in range(n_calls + 1):
            ens.engine.rvncc_sense_step(xs, ys, angs, route_of, SSD_CHANNEL)
            ens.engine.rvssd_sense_step(xs, ys, angs, route_of, SSD_CHANNEL)
        ens.engine.close()
    return 0


def ncc_trace_stats(directory, out, side):
    """The k_rvncc_* and k_rvssd_* rows of the trace's *kernel_stats.csv files under `directory`, a trace of --ncc-trace-run --sides
    `side` -> the ncc block's "kernel_trace" key, under that side."""
    import csv
    import glob
    rows = {}
    for path in sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r["Name"].split("(")[0].replace("void ", "").replace("dv::", "")
                if name.startswith(("k_rvncc_", "k_rvssd_")):
                    rows[name] = dict(calls=int(r["Calls"]), average_us=round(float(r["AverageNs"]) / 1e3, 3), min_us=round(float(r["MinNs"]) / 1e3, 3),
                                      max_us=round(float(r["MaxNs"]) / 1e3, 3))
    if not rows:
        print("no k_rvncc_* / k_rvssd_* rows under %s" % directory)
        return 1
    with open(out) as f:
        doc = json.load(f)
    trace = doc.setdefault("ncc", {}).setdefault("kernel_trace", dict(tool="rocprofv3 --kernel-trace --stats, a run of its own a side (--ncc-trace-run)",
                                                                      sides={}))
    score = {k: rows[k]["average_us"] for k in ("k_rvncc_score<0>", "k_rvssd_score<0>") if k in rows}
    trace["sides"][str(side)] = dict(kernels=rows, ncc_over_ssd_score=round(score["k_rvncc_score<0>"] / score["k_rvssd_score<0>"], 3)
                                     if len(score) == 2 else None)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["ncc"]["kernel_trace"]))
    return 0


SSDWIN_WINDOWS = ((50, 50), (255, 256))


def measure_ssdwin(side, n_calls, reps):
    """The ssdwin block's row of one side."""
    import navsim_amd
    from navsim_amd import synth
    land = synth.synth_landscape(3, LAND, 4)
    routes = [synth.sin_training_path(c, 0.2 * LAND, 0.6 * LAND, arclen=STEP_SIZE / HEADINGS) for c in CURVES]
    starts = starts_of(routes)
    centres = np.array([int(np.argmin(np.linalg.norm(routes[r] - np.array(pos), axis=1))) for r, pos, _ in starts])

    def ensemble(window):
        a = navsim_amd.NavBySceneFamiliarity(land, (side, side), STEP_SIZE, n_test_angles=HEADINGS, track_scene_familiarity=False,
                                             familiarity_model=navsim_amd.ssd_familiarity(SSD_CHANNEL))
        return navsim_amd.SsdRouteEnsemble.from_routes_with(a, routes, starts, metrics="device", window=window,
                                                            window_centres=None if window is None else centres.tolist())

    plain = ensemble(None)
    windowed = [ensemble(w) for w in SSDWIN_WINDOWS]
    eng = plain.engine
    n = len(starts)
    xs = np.array([p[0] for _, p, _ in starts])
    ys = np.array([p[1] for _, p, _ in starts])
    angs = (np.array([a for _, _, a in starts])[:, None] + plain.agents[0].angle_offsets[None, :]) % (2 * np.pi)
    route_of = np.array([r for r, _, _ in starts], dtype=np.int32)
    lens = np.array([len(routes[r]) for r in route_of])
    bounds = [(np.maximum(0, centres - b), np.minimum(lens, centres + a + 1)) for b, a in SSDWIN_WINDOWS]
    four = np.arange(0, n, STARTS_PER_ROUTE)                     # one member a route
    taus = dict(none=np.full(n, -np.inf), four=np.where(np.isin(np.arange(n), four), np.inf, -np.inf), all=np.full(n, np.inf))
    lost_of = dict(none=np.arange(0), four=four, all=np.arange(n))

    def call(k=None, which=None):
        eng.timer_start()
        for _ in range(n_calls):
            if k is None:
                res = eng.rvssd_sense_step(xs, ys, angs, route_of, SSD_CHANNEL)
            else:
                res = eng.rvssdw_sense_step(xs, ys, angs, route_of, bounds[k][0], bounds[k][1], SSD_CHANNEL,
                                            reloc_below=None if which is None else taus[which])
        return eng.timer_stop() * 1e3 / n_calls, res

    def wall(ens):
        w0 = time.perf_counter()
        for _ in range(n_calls):
            ens.step_forward(fake=True)
        return (time.perf_counter() - w0) * 1e6 / n_calls

    _, whole = call()                                             # warm-up of every form, and the forms agree
    assert not whole.flags.any()
    for k in range(len(SSDWIN_WINDOWS)):
        _, res = call(k)
        assert not res.flags.any() and (res.angle_view >= bounds[k][0][:, None]).all() and (res.angle_view < bounds[k][1][:, None]).all()
        assert (res.angle_ssd >= whole.angle_ssd).all()
        inside = (whole.angle_view >= bounds[k][0][:, None]) & (whole.angle_view < bounds[k][1][:, None])
        assert np.array_equal(res.angle_ssd[inside], whole.angle_ssd[inside]) and np.array_equal(res.angle_view[inside], whole.angle_view[inside])
    _, win = call(0)
    for which in ("none", "four", "all"):
        _, got = call(0, which)
        m = lost_of[which]
        ssd, view = win.angle_ssd.copy(), win.angle_view.copy()
        ssd[m], view[m] = whole.angle_ssd[m], whole.angle_view[m]
        assert np.array_equal(got.angle_ssd, ssd) and np.array_equal(got.angle_view, view) and np.array_equal(np.flatnonzero(got.relocalised), m)
    for e in [plain] + windowed:
        wall(e)
    t = {key: [] for key in ("unwindowed", "none", "four", "all", "wall_unwindowed")}
    t_win, w_win = [[] for _ in SSDWIN_WINDOWS], [[] for _ in SSDWIN_WINDOWS]
    for _ in range(reps):                                         # alternating windows
        t["unwindowed"].append(call()[0])
        for k in range(len(SSDWIN_WINDOWS)):
            t_win[k].append(call(k)[0])
        for which in ("none", "four", "all"):
            t[which].append(call(0, which)[0])
        t["wall_unwindowed"].append(wall(plain))
        for k, e in enumerate(windowed):
            w_win[k].append(wall(e))
    med = float(np.median(t["unwindowed"]))
    rows = []
    for k, (b, a) in enumerate(SSDWIN_WINDOWS):
        rows.append(dict(behind=b, ahead=a, views=int((bounds[k][1] - bounds[k][0]).max()), windowed_call_us=spread(t_win[k]),
                         ensemble_step_wall_us=spread(w_win[k]), unwindowed_over_windowed_call=round(med / float(np.median(t_win[k])), 3),
                         members_running=len(windowed[k].active)))
    m101 = float(np.median(t_win[0]))
    out = dict(side=side, routes=len(routes), route_views=[len(r) for r in routes], members=n, headings=HEADINGS, columns=n * HEADINGS,
               channel=SSD_CHANNEL, calls_per_window=n_calls, windows=reps, tile_columns=32, unwindowed_call_us=spread(t["unwindowed"]),
               unwindowed_ensemble_step_wall_us=spread(t["wall_unwindowed"]), members_running=len(plain.active), windowed=rows,
               reloc_window_views=rows[0]["views"], reloc_none_lost_call_us=spread(t["none"]), reloc_4_lost_call_us=spread(t["four"]),
               reloc_all_lost_call_us=spread(t["all"]), none_lost_minus_windowed_us=round(float(np.median(t["none"])) - m101, 3))
    for e in [plain] + windowed:
        e.engine.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", default="32,64")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rviews_time.json"))
    ap.add_argument("--blocks", default="routes", help="which blocks to measure: routes (the routed step against four engines), sensors, noise, window, reloc, ssd, ssdwin, ncc")
    ap.add_argument("--ncc-trace-run", action="store_true", help="the ncc block's calls alone, for a kernel trace (no timing, no output file)")
    ap.add_argument("--ncc-trace-stats", default=None, help="a kernel trace's output directory: its k_rvncc_* / k_rvssd_* rows go into the ncc block")
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed to the GPU child of the sensors block and of the noise block")
    args = ap.parse_args()
    if args.ncc_trace_run:
        return ncc_trace_run([int(s) for s in args.sides.split(",")], args.calls)
    if args.ncc_trace_stats:
        return ncc_trace_stats(args.ncc_trace_stats, args.out, int(args.sides.split(",")[0]))
    blocks = args.blocks.split(",")
    kept = {}
    if os.path.exists(args.out):                                  # a block that is not measured keeps its rows
        with open(args.out) as f:
            kept = json.load(f)
    sensors = kept.get("sensors", [])
    if "sensors" in blocks:                                       # (a child of its own, before this process opens the GPU)
        import sensors_block
        rc, row = sensors_block.run_child(args.limit, args.calls, args.reps, "rviews")
        if rc != 0:
            return rc
        sensors = [row]
    noise = kept.get("noise", [])
    if "noise" in blocks:                                         # (a child of its own, as the sensors block's)
        import noise_block
        rc, row = noise_block.run_child(args.limit, [int(s) for s in args.sides.split(",")], args.calls, args.reps, "rviews")
        if rc != 0:
            return rc
        noise = [row]
    rows = [measure(int(s), args.calls, args.reps) for s in args.sides.split(",")] if "routes" in blocks else kept.get("sizes", [])
    import torch                                                  # (after the windows: only to ask the device its name)
    doc = dict(tool="tools/rviews_time.py", device=torch.cuda.get_device_name(0), step_form="step_forward(fake=True)", note="medians of alternating windows in one process; wall-clock figures "
               "include the host's share of a step", sizes=rows, sensors=sensors, noise=noise)
    if "window" in blocks:                                        # a key of its own: the keys that were there stay as they were
        doc = dict(doc if ("routes" in blocks or "sensors" in blocks or "noise" in blocks or not kept) else kept, window=dict(device=torch.cuda.get_device_name(0), windows=[list(w) for w in WINDOWS],
                                            sizes=[measure_window(int(s), args.calls, args.reps) for s in args.sides.split(",")]))
    elif "window" in kept:
        doc["window"] = kept["window"]
    if "reloc" in blocks:                                         # a key of its own, as the window block's
        if not ({"routes", "sensors", "noise", "window"} & set(blocks)) and kept:
            doc = dict(kept)
        doc["reloc"] = dict(device=torch.cuda.get_device_name(0), window=list(RELOC_WINDOW),
                            sizes=[measure_reloc(int(s), args.calls, args.reps) for s in args.sides.split(",")])
    elif "reloc" in kept:
        doc["reloc"] = kept["reloc"]
    if "ssd" in blocks:                                           # a key of its own, as the window block's
        if not ({"routes", "sensors", "noise", "window", "reloc"} & set(blocks)) and kept:
            doc = dict(kept)
        doc["ssd"] = dict(device=torch.cuda.get_device_name(0), channel=SSD_CHANNEL,
                          sizes=[measure_ssd(int(s), args.calls, args.reps) for s in args.sides.split(",")])
    elif "ssd" in kept:
        doc["ssd"] = kept["ssd"]
    if "ssdwin" in blocks:                                        # a key of its own, as the window block's
        if not ({"routes", "sensors", "noise", "window", "reloc", "ssd"} & set(blocks)) and kept:
            doc = dict(kept)
        doc["ssdwin"] = dict(device=torch.cuda.get_device_name(0), channel=SSD_CHANNEL, windows=[list(w) for w in SSDWIN_WINDOWS],
                             sizes=[measure_ssdwin(int(s), args.calls, args.reps) for s in args.sides.split(",")])
    elif "ssdwin" in kept:
        doc["ssdwin"] = kept["ssdwin"]
    if "ncc" in blocks:                                           # a key of its own, as the window block's
        if not ({"routes", "sensors", "noise", "window", "reloc", "ssd", "ssdwin"} & set(blocks)) and kept:
            doc = dict(kept)
        doc["ncc"] = dict(device=torch.cuda.get_device_name(0), channel=SSD_CHANNEL,
                          sizes=[measure_ncc(int(s), args.calls, args.reps) for s in args.sides.split(",")])
    elif "ncc" in kept:
        doc["ncc"] = kept["ncc"]
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
