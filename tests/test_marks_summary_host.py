"""The coverage statistics of a result row without a device: the NumPy restatement (navsim_amd.agent.marks_summary_host) held to the
reference's loops, the binding surface of the dv_marks_* calls, the engine's argument checks (made before any library call), and the
ensembles' and the experiment loop's use of the summary call on a NumPy stand-in engine."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import experiment, mushroom_familiarity
from navsim_amd.agent import coverage_row, marks_summary_host
from tests import helpers_marks_summary as HM
from tests import helpers_mushroom_banks as HB
from tests import test_path_routes_host as TP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"dv_marks_summary": "marks_summary", "dv_marks_summary_slots": "marks_summary_slots", "dv_marks_summary_routes": "marks_summary_routes"}
PINNED_PREFIXES = ("dv_path_routes_", "dv_lands_", "dv_mb_", "dv_mbank_", "dv_ibank_", "dv_infomax", "dv_diffuse")


# ---- the restatement against the reference's loops -----------------------------------------------------------------------------------------------
def test_restatement_equals_the_loops_on_every_pattern_up_to_ten_marks():
    """Every mark pattern of length 1..10 under every window 0..n + 1: == on all three, and furthest / n == the forgiving loop's value
    (HM.loops asserts that one)."""
    cases = 0
    for n in range(1, 11):
        for bits in itertools.product((False, True), repeat=n):
            marks = np.array(bits, dtype=bool)
            for win in range(n + 2):
                assert marks_summary_host(marks, win) == HM.loops(marks, win), (bits, win)
                cases += 1
    assert cases == sum((n + 2) << n for n in range(1, 11))


def test_restatement_equals_the_loops_on_random_arrays():
    rng = np.random.default_rng(20250213)
    for k in range(2000):
        n = int(rng.integers(1, 301))
        marks = rng.random(n) < rng.uniform(0.5, 0.99)
        win = int(rng.integers(0, n + 2)) if k % 3 else int(0.05 * n)
        got = marks_summary_host(marks, win)
        assert got == HM.loops(marks, win), (k, n, win)
        assert all(type(v) is int for v in got)
    # uint8 marks of any non-zero value are marks; the row's types are the three methods'
    marks = np.array([0, 3, 1, 0, 255, 1, 1], dtype=np.uint8)
    assert marks_summary_host(marks, 2) == HM.loops(marks != 0, 2) == (5, 7, 2)
    bare = HM._Bare(marks != 0, 2)
    row = coverage_row(5, 7, 2, 7)
    for key, want in (("path_coverage", bare.percent_recapitulated), ("percent_forgiving", bare.percent_recapitulated_forgiving()),
                      ("n_captures", bare.n_captures())):
        assert row[key] == want and type(row[key]) is type(want), key
    assert type(coverage_row(0, 0, 0, 7)["percent_forgiving"]) is float                  # the loop's `0.`


def test_planted_slots_meet_their_conditions():
    """The GPU tests' planted runs are what helpers_marks_summary says they are."""
    C, T, W = HM.C, HM.T, HM.W
    assert T == 256 * C and HM.LENGTHS == (1, 2, C, 64 * C - 1, 64 * C + 1, T - 1, T, T + 1, 2 * T + 3, 263200)
    assert any(o % 2 for o in HM.offsets().tolist())                                     # a slot begins at an odd byte
    m = HM.planned_marks()
    assert m[0].all() and not m[2].any() and m[5].all() and len(m[5]) > 64 * C
    assert not m[1][0] and m[1][1] and HM.restated(m[1], 1) == (1, 2, 1)                 # clear at 0, a run of win: captured at p = win
    assert m[3][0] and m[3][C - 1] and m[3][C]                                           # from index 0; across a chunk edge
    assert HM.loops(m[3], 5)[2] == 4 and HM.loops(m[3], 6)[2] == 2 and HM.loops(m[3], 4)[2] == 5      # runs of win - 1, win, win + 1
    assert m[3][-1] and not m[3][-6] and HM.loops(m[3], 5)[1] == len(m[3])               # exactly win, ending at n - 1
    assert not m[4][0] and HM.loops(m[4], 7) == (13, 8, 1) and m[4][64 * C - 1] and m[4][64 * C] and m[4][-1]
    assert HM.restated(m[6], T - 3) == (T - 3, T, 1) and HM.restated(m[6], T - 2) == (T - 3, 0, 0)
    assert m[7][T - 1] and m[7][T] and m[7][:2001].all() and not m[7][2001]
    assert HM.restated(m[8], T + 5) == (2 * T + 2, T + 5, 0) and HM.restated(m[8], T - 3)[2] == 1
    assert W > T and [HM.restated(m[9], w)[2] for w in (W - 1, W, W + 1)] == [5, 4, 2]
    assert HM.restated(m[9], W)[1] == len(m[9]) and m[9][-W:].all() and not m[9][-W - 1]
    slots, windows = HM.entries()
    for j, n in enumerate(HM.LENGTHS):
        mine = set(windows[slots == j].tolist())
        assert {0, 1, n - 1, n, n + 5} <= mine and len(mine) >= 3


# ---- binding surface ---------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_engine_agree_on_the_marks_names():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    declared = set(re.findall(r"\bint\s+(dv_marks_[a-z0-9_]*)\s*\(", header))
    assert declared == set(NAMES) == {k for k in N.PROTOTYPES if k.startswith("dv_marks_")}
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert N.PROTOTYPES[name][0] is ctypes.c_int
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(N.PROTOTYPES[name][1]), name
        assert callable(getattr(navsim_amd.FamiliarityEngine, NAMES[name])), name
        assert not name.startswith(PINNED_PREFIXES), name
    assert N.PROTOTYPES["dv_marks_summary"][1] == [N._ctx_p, ctypes.c_int64, N._i64p]
    assert N.PROTOTYPES["dv_marks_summary_slots"][1] == [N._ctx_p, N._i32p, N._i64p, ctypes.c_int, N._i64p]
    assert N.PROTOTYPES["dv_marks_summary_routes"][1] == [N._ctx_p, N._i32p, N._i64p, ctypes.c_int64, N._i64p]
    # the kernel's trip, as the header states it and as the binding hands it to the tests
    defines = dict(re.findall(r"#define\s+(DV_MARKS_[A-Z_]+)\s+(\d+)", header))
    assert {k: int(v) for k, v in defines.items()} == dict(DV_MARKS_PER_THREAD=N.DV_MARKS_PER_THREAD, DV_MARKS_PER_TRIP=N.DV_MARKS_PER_TRIP)
    assert N.DV_MARKS_PER_TRIP == 256 * N.DV_MARKS_PER_THREAD


# ---- argument checks before the library --------------------------------------------------------------------------------------------------------
def test_marks_argument_checks_come_before_any_library_call():
    lib = TP._Recorder()
    e = TP._engine_without_a_device(lib)
    # no slots set: refused, whatever the arguments
    for call in (e.marks_summary_routes, e.marks_summary_slots):
        with pytest.raises(ValueError, match="no slots set"):
            call([0], [1])
    e.path_routes_set([np.zeros((3, 2)), np.ones((5, 2))])
    with pytest.raises(ValueError, match=r"no slots set \(path_routes_slots\)"):
        e.marks_summary_routes([0], [1])
    e.path_routes_slots([1, 0, 1])
    e.path_slots(4)
    del lib.calls[:]
    for call, n_slots in ((e.marks_summary_routes, 3), (e.marks_summary_slots, 4)):
        for slots, windows, what in (([0, n_slots], [1, 1], r"slots\[1\] = %d outside \[0, n_slots = %d\)" % (n_slots, n_slots)),
                                     ([-1, 0], [1, 1], r"slots\[0\] = -1 outside"),
                                     ([0.0, 1.0], [1, 1], "slots must hold integers"), ([[0, 1]], [1, 1], "slots must have one dimension"),
                                     ([0, 1], [1, -1], r"windows\[1\] = -1 < 0"), ([0, 1], [1.0, 2.0], "windows must hold integers"),
                                     ([0, 1], [[1, 2]], r"windows must have shape \(2,\)"), ([0, 1], [1], r"windows must have shape \(2,\)"),
                                     ([0, 1], 1, r"windows must have shape \(2,\)"), ([0], [1, 2], r"windows must have shape \(1,\)")):
            with pytest.raises(ValueError, match=what):
                call(slots, windows)
    for bad in (-1, 1.0, None, True, [1]):
        with pytest.raises(ValueError, match="window must be an integer >= 0"):
            e.marks_summary(bad)
    assert lib.calls == []
    # arguments that hold: each method reaches its own symbol, once, with the arguments the binding declares
    assert e.marks_summary(0).shape == (3,) and e.marks_summary(np.int64(7)).dtype == np.int64
    got = e.marks_summary_routes([2, 0, 2], [0, 5, 1 << 40])
    assert got.shape == (3, 3) and got.dtype == np.int64
    assert e.marks_summary_slots(np.array([3], dtype=np.int16), np.array([2], dtype=np.uint8)).shape == (1, 3)
    assert e.marks_summary_routes([], []).shape == (0, 3)
    assert lib.calls == [(s, len(N.PROTOTYPES[s][1])) for s in ("dv_marks_summary", "dv_marks_summary", "dv_marks_summary_routes",
                                                              "dv_marks_summary_slots", "dv_marks_summary_routes")]
    # the slots go with their routes, and with their path
    e.path_routes_set(None)
    e.set_training_path(None)
    for call in (e.marks_summary_routes, e.marks_summary_slots):
        with pytest.raises(ValueError, match="no slots set"):
            call([0], [1])


# ---- ensembles and the experiment loop on a NumPy stand-in engine ---------------------------------------------------------------------------------
class _WithoutSummary(TP._NumpyEngine):
    """The routed stand-in, as an engine that has no summary call (the stand-in itself answers every name with a call that fails)."""
    def __getattr__(self, name):
        if name.startswith("marks_summary"):
            raise AttributeError(name)
        return TP._NumpyEngine.__getattr__(self, name)


class _WithSummary(_WithoutSummary):
    def marks_summary_routes(self, slots, windows):
        self._note("marks_summary_routes", list(slots), list(windows))
        return np.array([marks_summary_host(self.marks[j], w) for j, w in zip(slots, windows)], dtype=np.int64).reshape(len(slots), 3)


def _ensemble(engine_cls, metrics="device"):
    """TP._ensemble's members (6, on 3 routes of 45, 40 and 35 points) on an engine of `engine_cls`."""
    agent = navsim_amd.NavBySceneFamiliarity(TP.LAND, (12, 10), 1.0, n_test_angles=9, use_gpu_sensor=False,
                                             familiarity_model=mushroom_familiarity(n_kc=300, fan_in=4, seed=3))
    agent._engine = engine_cls((10, 12))
    paths = HB.routes()
    return navsim_amd.MushroomRouteEnsemble.from_routes_with(agent, paths, HB.starts(paths), metrics=metrics)


def test_run_ensemble_takes_the_rows_from_one_summary_call():
    plain, summed = _ensemble(_WithoutSummary), _ensemble(_WithSummary)
    rows_plain = experiment.run_ensemble(plain, frames=12)
    n_cov = len(summed.engine.named("path_routes_coverage"))
    rows = experiment.run_ensemble(summed, frames=12)
    assert any(r["path_coverage"] > 0 for r in rows) and any(r["n_captures"] > 0 for r in rows)
    for r, p in zip(rows, rows_plain):
        assert sorted(r) == sorted(p)
        for k in ("path_coverage", "percent_forgiving", "n_captures", "completed_frames", "stop_status"):
            assert r[k] == p[k] and type(r[k]) is type(p[k]), k
    trial = dict(step_size=1.0)
    assert [experiment.csv_row(trial, r) for r in rows] == [experiment.csv_row(trial, p) for p in rows_plain]
    calls = summed.engine.named("marks_summary_routes")
    assert len(calls) == 1 and calls[0][1] == list(range(6))                             # ONE call, every member's slot
    assert calls[0][2] == [int(experiment.N_CONSECUTIVE_SCENES * len(a.training_path)) for a in summed.agents]
    assert len(set(calls[0][2])) > 1                                                     # ... each under its own route's window
    assert len(summed.engine.named("path_routes_coverage")) == n_cov                     # and no marks copied out
    assert len(plain.engine.named("path_routes_coverage")) == 3 * 6                      # (the three methods: one copy each, per member)
    # a member's own three methods still work afterwards, and its own summary equals them
    for a, r in zip(summed.agents, rows):
        assert (a.percent_recapitulated, a.percent_recapitulated_forgiving(0.05), a.n_captures(0.05)) == \
            (r["path_coverage"], r["percent_forgiving"], r["n_captures"])
        assert a.coverage_summary(0.05) == {k: r[k] for k in ("path_coverage", "percent_forgiving", "n_captures")}
    assert summed.coverage_summary(0.3) == plain.coverage_summary(0.3)
    for obj in (summed, summed.agents[0]):
        with pytest.raises(ValueError, match="n_consecutive_scenes must be >= 0"):
            obj.coverage_summary(-0.01)
    assert summed.agents[0].n_captures(-0.01) >= 0                                       # (the three methods are as they were)


def test_host_metric_members_are_answered_by_their_own_methods():
    ens = _ensemble(_WithSummary, metrics="host")
    rows = experiment.run_ensemble(ens, frames=5)
    assert not ens.engine.named("marks_summary_routes") and len(rows) == 6
    for a, r in zip(ens.agents, rows):
        assert r["path_coverage"] == a.percent_recapitulated and r["n_captures"] == a.n_captures(0.05)


class _OnlyThree(object):
    """What run_experiment asked of an agent before: stepping and the three methods."""
    training_path_length, step_size, stopped_with_exception = 10.0, 1.0, None
    percent_recapitulated, navigation_error = 0.25, 1.5

    def __init__(self):
        self.steps, self.asked = 0, []

    def step_forward(self):
        self.steps += 1
        if self.steps == 4:
            raise navsim_amd.ReachedEndOfTrainingPathException()

    def percent_recapitulated_forgiving(self, n_consecutive_scenes):
        self.asked.append(("forgiving", n_consecutive_scenes))
        return 0.5

    def n_captures(self, n_consecutive_scenes):
        self.asked.append(("captures", n_consecutive_scenes))
        return 3


def test_run_experiment_on_an_object_with_only_the_three_methods():
    a = _OnlyThree()
    row = experiment.run_experiment(a)
    assert row == dict(path_coverage=0.25, rmsd_error=1.5, completed_frames=3, stop_status=1, percent_forgiving=0.5, n_captures=3)
    assert a.asked == [("forgiving", 0.05), ("captures", 0.05)]


class _Stepped(HM._Bare):
    navigation_error = 0.0                                 # (a bare agent has stepped nowhere: no error to divide)


def test_run_experiment_takes_a_lone_agents_row_from_its_summary():
    marks = np.array([0, 1, 1, 0, 1, 1, 1, 0, 0, 1] * 4, dtype=bool)
    a = _Stepped(marks, 2)
    row = experiment.run_experiment(a, frames=0)
    assert (row["path_coverage"], row["percent_forgiving"], row["n_captures"]) == \
        (a.percent_recapitulated, a.percent_recapitulated_forgiving(), a.n_captures()) == (0.6, 0.925, 8)
    assert [type(row[k]) for k in ("path_coverage", "percent_forgiving", "n_captures")] == [np.float64, float, int]
