"""The coverage statistics of a result row on the device (dv_marks_*, k_marks_summary) against the reference's loops: np.array_equal on
int64[n, 3], no tolerances -- everything is integers.  The marks are planted through the existing metric calls and read back with the
existing coverage calls; what is read back is the tests' input (tests/helpers_marks_summary.py).  Then the ensembles, the lone agent and
the experiment loop against the agents' own three methods."""
import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import experiment, infomax_familiarity, mushroom_familiarity, synth
from tests import helpers_infomax_banks as HIB
from tests import helpers_marks_summary as HM
from tests import helpers_mushroom_banks as HMB
from tests import helpers_path_routes as HP

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -3


@pytest.fixture
def eng():
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


@pytest.fixture
def planted(eng):
    """The engine with HM's ten slots planted, and the marks read back from it."""
    eng.path_routes_set(HM.routes())
    eng.path_routes_slots(list(range(len(HM.LENGTHS))))
    eng.path_routes_error(*HM.plant_call())
    marks = [eng.path_routes_coverage(j, n) for j, n in enumerate(HM.LENGTHS)]
    for j, (got, want) in enumerate(zip(marks, HM.planned_marks())):
        assert np.array_equal(got, want), (j, np.flatnonzero(got != want)[:8])            # the planted runs are there
    return eng, marks


def _raw(eng, slots, windows, n=None):
    """dv_marks_summary_routes as the library takes it: (return code, out)."""
    slots, windows = np.ascontiguousarray(slots, dtype=np.int32), np.ascontiguousarray(windows, dtype=np.int64)
    out = np.full((len(slots), 3), -7, dtype=np.int64)
    rc = eng._lib.dv_marks_summary_routes(eng._ctx, slots.ctypes.data_as(N._i32p), N.i64ptr(windows), len(slots) if n is None else n, N.i64ptr(out))
    return rc, out


# ---- 1. the planted slots --------------------------------------------------------------------------------------------------------------------------
def test_planted_slots_under_all_their_windows_in_one_call(planted):
    eng, marks = planted
    slots, windows = HM.entries()
    got = eng.marks_summary_routes(slots, windows)
    want = HM.expected(marks, slots, windows)
    bad = np.flatnonzero((got != want).any(axis=1))
    print("%d entries over %d slots, %d differ" % (len(slots), len(HM.LENGTHS), len(bad)))
    assert got.dtype == np.int64 and got.shape == (len(slots), 3)
    assert np.array_equal(got, want), [(int(slots[e]), int(windows[e]), got[e].tolist(), want[e].tolist()) for e in bad[:8]]
    # the call only reads: the marks are as they were
    for j, n in enumerate(HM.LENGTHS):
        assert np.array_equal(eng.path_routes_coverage(j, n), marks[j]), j
    # one call of one entry; an empty call
    for e in (0, len(slots) // 2, len(slots) - 1):
        assert np.array_equal(eng.marks_summary_routes(slots[e:e + 1], windows[e:e + 1]), want[e:e + 1]), e
    assert eng.marks_summary_routes([], []).shape == (0, 3)


def test_refused_calls_and_reset(planted):
    eng, marks = planted
    slots, windows = HM.entries()
    want = HM.expected(marks, slots, windows)
    n_slots = len(HM.LENGTHS)
    for at, bad in ((3, n_slots), (0, -1), (len(slots) - 1, 1 << 20)):
        s = slots.copy()
        s[at] = bad
        rc, out = _raw(eng, s, windows)
        assert rc == INVALID and (out == -7).all() and ("slots[%d] = %d" % (at, bad)) in eng._lib.dv_last_error(eng._ctx).decode()
        with pytest.raises(ValueError, match=r"slots\[%d\]" % at):
            eng.marks_summary_routes(s, windows)
    w = windows.copy()
    w[5] = -1
    rc, out = _raw(eng, slots, w)
    assert rc == INVALID and (out == -7).all() and "window[5] = -1" in eng._lib.dv_last_error(eng._ctx).decode()
    with pytest.raises(ValueError, match=r"windows\[5\] = -1"):
        eng.marks_summary_routes(slots, w)
    assert _raw(eng, slots, windows, n=-1)[0] == INVALID
    rc, out = _raw(eng, slots, windows, n=0)
    assert rc == 0 and (out == -7).all()
    for j, n in enumerate(HM.LENGTHS):
        assert np.array_equal(eng.path_routes_coverage(j, n), marks[j]), j
    assert np.array_equal(eng.marks_summary_routes(slots, windows), want)
    # cleared marks: nothing covered; a window of 0 is met everywhere (furthest = n) and every mark is a clear one (captures = n)
    eng.path_routes_reset(-1)
    got = eng.marks_summary_routes(slots, windows)
    n = np.array(HM.LENGTHS, dtype=np.int64)[slots]
    cleared = np.stack([np.zeros_like(n), np.where(windows == 0, n, 0), np.where(windows == 0, n - windows, 0)], axis=1)
    assert np.array_equal(got, cleared)
    # without slots, and without routes: a state error
    eng.path_routes_slots(None)
    assert _raw(eng, [0], [1])[0] == STATE
    eng.path_routes_set(None)
    assert _raw(eng, [0], [1])[0] == STATE
    with pytest.raises(ValueError, match="no slots set"):
        eng.marks_summary_routes([0], [1])


# ---- 2. more entries than one launch takes ---------------------------------------------------------------------------------------------------------
def test_a_call_of_65537_entries_over_the_seven_slot_deal(eng):
    """helpers_path_routes' routes (curved, 1 to 263 200 points, dealt 4, 0, 2, 2, 0, 3, 1) marked by its calls one, b65 and c130; 65 537
    entries drawn over a palette of windows per slot: the second launch takes entries 65 535 and 65 536."""
    eng.path_routes_set(HP.routes())
    eng.path_routes_slots(HP.ROUTE_OF_SLOT)
    c, _ = HP.calls()
    for name in ("one", "b65", "c130"):
        eng.path_routes_error(*c[name])
    marks = [eng.path_routes_coverage(j, HP.ROUTE_POINTS[r]) for j, r in enumerate(HP.ROUTE_OF_SLOT)]
    assert sum(m.any() and not m.all() for m in marks) >= 4
    rng = np.random.default_rng(65537)
    palette = []
    for j, m in enumerate(marks):
        n = len(m)
        palette += [(j, w) for w in sorted({0, 1, 2, 3, n - 1, n, n + 5, int(0.05 * n), int(rng.integers(0, n + 1))})]
    pick = rng.integers(0, len(palette), 65537)
    pick[-2:] = [pick[-3] + 1, pick[-3] + 2]
    pick %= len(palette)                                                                 # (the second launch's two differ from their neighbours)
    slots = np.array([palette[k][0] for k in pick], dtype=np.int32)
    windows = np.array([palette[k][1] for k in pick], dtype=np.int64)
    want = HM.expected(marks, slots, windows)
    assert len(set(pick[-3:].tolist())) == 3
    got = eng.marks_summary_routes(slots, windows)
    bad = np.flatnonzero((got != want).any(axis=1))
    print("65537 entries over %d (slot, window) pairs: %d differ" % (len(palette), len(bad)))
    assert np.array_equal(got, want), [(int(e), int(slots[e]), int(windows[e]), got[e].tolist(), want[e].tolist()) for e in bad[:8]]


# ---- 3. the other two holders of marks ---------------------------------------------------------------------------------------------------------------
def test_the_one_paths_slots_and_the_lone_agents_marks(eng):
    n = HM.T + 37                                                                        # odd: slot 1 begins at an odd byte
    path = np.stack([np.arange(n, dtype=np.float64), np.zeros(n)], axis=1)
    assert eng._lib.dv_marks_summary(eng._ctx, 1, N.i64ptr(np.zeros(3, dtype=np.int64))) == STATE
    with pytest.raises(ValueError, match="no slots set"):
        eng.marks_summary_slots([0], [1])
    eng.set_training_path(path)
    eng.path_slots(3)
    # the slots' stretches are all 2 x 10 + 1 marks long (one reach per call): some overlap into longer runs, one crosses the trip edge
    centres = {0: [10.0, 25.0, 500.0], 1: [float(HM.T), 700.0, 721.0, n - 11.0], 2: []}
    pairs = [(j, x) for j in centres for x in centres[j]]
    eng.path_error_batch([j for j, _ in pairs], [x for _, x in pairs], [0.0] * len(pairs), 10.0)
    marks = [eng.path_coverage_slot(j, n) for j in range(3)]
    assert marks[0][:36].all() and not marks[0][36] and marks[1][HM.T - 10:HM.T + 11].all() and marks[1][-1] and not marks[2].any()
    slots = np.array([1, 0, 2, 1, 0, 1, 2, 0], dtype=np.int32)
    windows = np.array([21, 36, 0, 42, 21, n, 1, 0], dtype=np.int64)
    want = np.array([HM.loops(marks[j], w) for j, w in zip(slots.tolist(), windows.tolist())])      # (4 133 marks: the loops can walk them)
    assert np.array_equal(eng.marks_summary_slots(slots, windows), want)
    assert want[0].tolist() == [84, n, 3] and want[3].tolist() == [84, 732, 1]
    with pytest.raises(ValueError, match=r"slots\[0\] = 3"):
        eng.marks_summary_slots([3], [1])
    # the lone agent's marks, after the metrics enqueued beside the steps
    for x, reach in ((5.0, 5.0), (300.0, 7.0), (float(HM.T) + 1.0, 4.0), (n - 3.0, 2.0)):
        eng.path_error_enqueue(x, 0.0, reach)
        eng.path_error_wait()
    lone = eng.path_coverage(n)
    assert lone[:11].all() and lone[-1] and lone.sum() == 11 + 15 + 9 + 5
    for w in (0, 1, 5, 9, 10, 11, 15, 16, n):
        assert eng.marks_summary(w).tolist() == list(HM.loops(lone, w)), w
    assert eng.marks_summary(9).tolist() == [40, HM.T + 6, 2] and eng.marks_summary(5).tolist()[1:] == [n, 3]
    with pytest.raises(ValueError, match="window must be an integer >= 0"):
        eng.marks_summary(-1)
    assert eng._lib.dv_marks_summary(eng._ctx, -1, N.i64ptr(np.zeros(3, dtype=np.int64))) == INVALID
    # the slots' marks were not the lone agent's, nor the other way round
    assert np.array_equal(eng.path_coverage_slot(1, n), marks[1]) and np.array_equal(eng.marks_summary_slots(slots, windows), want)
    eng.set_training_path(None)


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------------------------
MODELS = {
    "mushroom": (navsim_amd.MushroomRouteEnsemble, HMB, (12, 10), lambda: mushroom_familiarity(n_kc=1043, fan_in=8, sparsity=0.02, seed=6)),
    "infomax": (navsim_amd.InfomaxRouteEnsemble, HIB, HIB.ENSEMBLE_SENSOR, lambda: infomax_familiarity(**HIB.ENSEMBLE_MODEL)),
}
KEYS = ("path_coverage", "percent_forgiving", "n_captures")


def _three(a, n_consecutive_scenes=0.05):
    return {"path_coverage": a.percent_recapitulated, "percent_forgiving": a.percent_recapitulated_forgiving(n_consecutive_scenes),
            "n_captures": a.n_captures(n_consecutive_scenes)}


def _same_rows(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w), i
        for k in g:
            assert (g[k] == w[k] or (g[k] != g[k] and w[k] != w[k])) and type(g[k]) is type(w[k]), (i, k, g[k], w[k])


def _counted(engine, name):
    calls, inner = [], getattr(engine, name)

    def call(*a):
        calls.append(a)
        return inner(*a)
    setattr(engine, name, call)
    return calls


@pytest.mark.parametrize("model", ["mushroom", "infomax"])
def test_route_ensembles_summary_equals_the_members_three_methods(model):
    cls, H, sensor, make = MODELS[model]
    paths = H.routes()[:2]
    starts = [s for s in H.starts(H.routes()) if s[0] < 2]
    agent = navsim_amd.NavBySceneFamiliarity(synth.synth_landscape(3, 300, 4), sensor, 1.0, n_test_angles=9, use_gpu_sensor=True,
                                             familiarity_model=make())
    ens = cls.from_routes_with(agent, paths, starts, metrics="device")
    try:
        assert len(ens.agents) == 4
        summaries = _counted(ens.engine, "marks_summary_routes")
        copies = _counted(ens.engine, "path_routes_coverage")
        rows = experiment.run_ensemble(ens, frames=15)
        assert len(summaries) == 1 and not copies                                        # one device call; no marks copied out
        assert list(summaries[0][1]) == [int(0.05 * len(a.training_path)) for a in ens.agents]
        want = [dict(_three(a), rmsd_error=a.navigation_error if a._n_navigation_error else float("nan"),
                     completed_frames=rows[i]["completed_frames"], stop_status=ens.stop_status[i]) for i, a in enumerate(ens.agents)]
        _same_rows(rows, want)
        trial = dict(step_size=1.0, n_test_angles=9)
        assert [experiment.csv_row(trial, r) for r in rows] == [experiment.csv_row(trial, w) for w in want]
        assert any(r["path_coverage"] > 0 for r in rows)
        for frac in (0.05, 0.0, 0.2, 1.0, 1.5):
            _same_rows(ens.coverage_summary(frac), [_three(a, frac) for a in ens.agents])
        _same_rows([a.coverage_summary(0.1) for a in ens.agents], [_three(a, 0.1) for a in ens.agents])
    finally:
        ens.agents[0].clear_training()


def test_nav_ensemble_and_lone_agent_summary_equal_the_three_methods():
    land = synth.synth_landscape(3, 300, 4)
    path = synth.sin_training_path(0.5, 60, 180, arclen=1.0)[:120]
    nsf = navsim_amd.NavBySceneFamiliarity(land, (32, 32), 1.0, n_test_angles=8, use_gpu_sensor=True,
                                           familiarity_model=navsim_amd.sads_familiarity(0.25))
    nsf.train_from_path(path)
    try:
        # the lone agent through run_experiment: its marks are on the device
        nsf.position, nsf.angle = (float(path[3][0]), float(path[3][1])), float(np.arctan2(*(path[4] - path[3])[::-1]) % (2 * np.pi))
        assert nsf._metrics_on_device
        summaries = _counted(nsf._engine, "marks_summary")
        row = experiment.run_experiment(nsf, frames=15)
        assert len(summaries) == 1 and summaries[0] == (int(0.05 * len(path)),)
        _same_rows([{k: row[k] for k in KEYS}], [_three(nsf)])
        assert row["path_coverage"] > 0 and row["rmsd_error"] == nsf.navigation_error
        for frac in (0.0, 0.05, 0.1, 2.0):
            _same_rows([nsf.coverage_summary(frac)], [_three(nsf, frac)])
        # three members on its path
        poses = [((float(path[k][0] + dx), float(path[k][1] + dy)), float(np.arctan2(*(path[k + 1] - path[k])[::-1]) % (2 * np.pi)))
                 for k, dx, dy in ((5, 0.0, 0.0), (40, 0.3, -0.2), (80, -0.4, 0.5))]
        ens = navsim_amd.NavEnsemble.from_agent(nsf, poses)
        assert all(a._metric_slot == j for j, a in enumerate(ens.agents))
        summaries = _counted(ens.engine, "marks_summary_slots")
        copies = _counted(ens.engine, "path_coverage_slot")
        rows = experiment.run_ensemble(ens, frames=15)
        assert len(summaries) == 1 and not copies and list(summaries[0][0]) == [0, 1, 2]
        _same_rows([{k: r[k] for k in KEYS} for r in rows], [_three(a) for a in ens.agents])
        assert any(r["path_coverage"] > 0 for r in rows)
        for frac in (0.0, 0.02, 0.3):
            _same_rows(ens.coverage_summary(frac), [_three(a, frac) for a in ens.agents])
    finally:
        nsf.clear_training()
