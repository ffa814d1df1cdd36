"""Windowed steps on the route view store, what needs no GPU: the binding surface of dv_rvwin_*, the Python-side checks (made before any
library call), SadsRouteEnsemble's window policy on a fake engine, and the facts about the GPU tests' inputs that keep them from being
vacuous."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import sads_familiarity
from navsim_amd.engine import RouteViewResults
from oracle import oracle
from tests import helpers_rviews as HR
from tests import helpers_rvwin as HW

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"dv_rvwin_step_u8": "rvwin_step_u8", "dv_rvwin_sense_step": "rvwin_sense_step"}
E = navsim_amd.SadsRouteEnsemble


# ---- bindings ----------------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_engine_agree_on_the_rvwin_names():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    declared = set(re.findall(r"\bint\s+(dv_rvwin_[a-z0-9_]*)\s*\(", header))
    assert declared == set(NAMES) == {k for k in N.PROTOTYPES if k.startswith("dv_rvwin_")}
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert N.PROTOTYPES[name][0] is ctypes.c_int
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(N.PROTOTYPES[name][1]), name
        assert callable(getattr(navsim_amd.FamiliarityEngine, NAMES[name])), name
    cap = int(re.search(r"#define DV_RVWIN_MAX_VIEWS (\d+)\b", header).group(1))
    assert cap == N.DV_RVWIN_MAX_VIEWS == navsim_amd.FamiliarityEngine.RVWIN_MAX_VIEWS == E.WINDOW_MAX_VIEWS == HW.MAX_VIEWS == 512
    # a windowed call is the unwindowed one with the two window tables in front of the flags
    for plain, win in (("dv_rviews_step_u8", "dv_rvwin_step_u8"), ("dv_rviews_sense_step", "dv_rvwin_sense_step")):
        p, w = N.PROTOTYPES[plain][1], N.PROTOTYPES[win][1]
        at = p.index(ctypes.c_uint32)
        assert w == p[:at] + [N._i32p, N._i32p] + p[at:]


# ---- refusals before any library call ------------------------------------------------------------------------------------------------------------
class _NoLibrary(object):
    def __getattr__(self, name):
        raise AssertionError("library call %s after an argument that must be refused" % name)


def _engine(first=(0, 3, 8, 1008), shape=(4, 4)):
    e = navsim_amd.FamiliarityEngine.__new__(navsim_amd.FamiliarityEngine)
    e._lib, e._ctx_raw, e._begun = _NoLibrary(), None, False
    e.n_lands, e.sensor_shape = 0, shape
    e.rviews_first = None if first is None else np.array(first, dtype=np.int64)
    e.rviews_shape = None if first is None else shape
    return e


@pytest.mark.parametrize("lo,hi,match", [([0, -1, 0], [3, 5, 9], r"member 1: window \[-1, 5\)"), ([0, 0, 0], [3, 6, 9], r"member 1: window \[0, 6\).*route 1 of 5 views"),
                                         ([2, 0, 0], [2, 5, 9], r"member 0: window \[2, 2\)"), ([2, 0, 0], [1, 5, 9], r"member 0: window \[2, 1\)"),
                                         ([0, 0, 100], [3, 5, 613], r"member 2: window \[100, 613\) must hold 1 to 512 views"),
                                         ([0, 0], [3, 5], r"win_lo must have shape \(3,\)"), ([0, 0, 0], [3, 5], r"win_hi must have shape \(3,\)"),
                                         ([0.0, 0.0, 0.0], [3, 5, 9], "win_lo must hold integers"), ([0, 0, 0], [3.0, 5.0, 9.0], "win_hi must hold integers")])
def test_refused_windows_never_reach_the_library(lo, hi, match):
    e = _engine()
    patches, z, angs = np.zeros((3, 2, 4, 4, 3), np.uint8), np.zeros(3), np.zeros((3, 2))
    routes, weights = [0, 1, 2], [0.0, 0.5, 1.0]
    for call in (lambda: e.rvwin_step_u8(patches, routes, weights, lo, hi), lambda: e.rvwin_sense_step(z, z, angs, routes, weights, lo, hi)):
        with pytest.raises(ValueError, match=match):
            call()


def test_the_unwindowed_calls_refusals_hold_for_the_windowed_calls():
    e = _engine()
    patches, z, angs = np.zeros((2, 3, 4, 4, 3), np.uint8), np.zeros(2), np.zeros((2, 3))
    for routes, weights, match in (([0, 3], [0.0, 0.0], r"route_of_member\[1\] = 3 outside"), ([0, 1], [0.0, 1.5], r"chem_weights\[1\] = 1.5")):
        with pytest.raises(ValueError, match=match):
            e.rvwin_step_u8(patches, routes, weights, [0, 0], [1, 1])
        with pytest.raises(ValueError, match=match):
            e.rvwin_sense_step(z, z, angs, routes, weights, [0, 0], [1, 1])
    with pytest.raises(ValueError, match=r"uint8\[n, A, 4, 4, 3\]"):
        e.rvwin_step_u8(np.zeros((2, 3, 4, 5, 3), np.uint8), [0, 1], [0.0, 0.0], [0, 0], [1, 1])
    with pytest.raises(N.EngineError, match="lands_set first"):
        e.rvwin_sense_step(z, z, angs, [0, 1], [0.0, 0.0], [0, 0], [1, 1], land_of_member=[0, 0])
    with pytest.raises(N.EngineError, match="no route views"):
        _engine(None).rvwin_step_u8(patches, [0, 1], [0.0, 0.0], [0, 0], [1, 1])
    with pytest.raises(N.EngineError, match="no route views"):
        _engine(None).rvwin_sense_step(z, z, angs, [0, 1], [0.0, 0.0], [0, 0], [1, 1])


# ---- the ensemble's policy on a fake engine -----------------------------------------------------------------------------------------------------
class FakeEngine(object):
    """Answers a step with angle_view[k, a] = (lo of member k, or 0) + 2 * a + 1 clipped to the window / route, best_idex 1, and flag
    16 for the members on route `flagged`."""

    def __init__(self, lengths, flagged=None):
        self.lengths, self.flagged, self.calls = lengths, flagged, []

    def _answer(self, routes, A, lo, hi):
        n = len(routes)
        view = np.minimum(np.asarray(lo)[:, None] + 2 * np.arange(A)[None, :] + 1, np.asarray(hi)[:, None] - 1).astype(np.int64)
        flags = np.array([16 if r == self.flagged else 0 for r in routes], dtype=np.uint32)
        fam = np.arange(n * A, dtype=np.float64).reshape(n, A) + np.asarray(lo)[:, None]
        return RouteViewResults(fam, view, np.where(flags > 0, -1, 1).astype(np.int32), flags)

    def rviews_sense_step(self, x, y, angs, routes, weights, land_of_member=None):
        self.calls.append(("rviews", list(routes), None, None))
        return self._answer(routes, np.asarray(angs).shape[1], [0] * len(routes), [self.lengths[r] for r in routes])

    def rvwin_sense_step(self, x, y, angs, routes, weights, win_lo, win_hi, land_of_member=None):
        self.calls.append(("rvwin", list(routes), list(win_lo), list(win_hi)))
        return self._answer(routes, np.asarray(angs).shape[1], win_lo, win_hi)


def fake_ensemble(lengths, routes, windows, centres, flagged=None):
    ens = object.__new__(E)
    ens.agents = [types.SimpleNamespace(training_path=np.zeros((lengths[r], 2)), memory_bank=r, window=w, memory_index=m)
                  for r, w, m in zip(routes, windows, centres)]
    ens.engine = FakeEngine(lengths, flagged)
    ens._banks = np.array(routes, dtype=np.int32)
    ens._weights = np.full(len(routes), 0.25)
    ens._lands = None
    return ens


def step(ens, idx):
    n = len(idx)
    return ens._device_step(idx, np.zeros(n), np.zeros(n), np.zeros((n, 3)))


def test_windows_clip_at_both_ends_and_the_centre_follows_the_chosen_headings_view():
    ens = fake_ensemble([30, 40], [0, 1, 1, 0], [(2, 3)] * 4, [1, 38, 20, None])
    r = step(ens, [0, 1, 2, 3])
    assert [c[0] for c in ens.engine.calls] == ["rvwin", "rviews"]                       # two calls: members 0-2 windowed, member 3 whole route
    assert ens.engine.calls[0][1:] == ([0, 1, 1], [0, 36, 18], [5, 40, 24]) and ens.engine.calls[1][1] == [0]
    assert ens._window_of(types.SimpleNamespace(window=(2, 3), memory_index=1, training_path=np.zeros((30, 2)))) == (0, 5)
    assert r.angle_view.shape == (4, 3) and r.best_idex.tolist() == [1, 1, 1, 1] and not r.flags.any()
    assert r.angle_view[:, 1].tolist() == [3, 39, 21, 3]                                  # merged in the caller's order
    assert r.angle_familiarity[3].tolist() == [0.0, 1.0, 2.0] and r.angle_familiarity[1].tolist() == [39.0, 40.0, 41.0]
    assert [a.memory_index for a in ens.agents] == [3, 39, 21, 3]                         # angle_view[best]
    step(ens, [3, 1])                                                                      # a later step of two of them, in another order
    assert ens.engine.calls[2:] == [("rvwin", [0, 1], [1, 37], [7, 40])]
    assert [a.memory_index for a in ens.agents] == [3, 39, 21, 4]                         # member 1's window [37, 40): view 40 is clipped to 39


def test_a_flagged_member_keeps_its_centre_and_relocalise_forgets_it():
    ens = fake_ensemble([30, 40], [0, 1, 0], [(2, 3), (2, 3), None], [10, 20, None], flagged=1)
    r = step(ens, [0, 1, 2])
    assert r.flags.tolist() == [0, 16, 0] and r.best_idex.tolist() == [1, -1, 1]
    assert [a.memory_index for a in ens.agents] == [11, 20, None]                         # member 2 has no window: it never has a centre
    ens.relocalise([0])
    assert [a.memory_index for a in ens.agents] == [None, 20, None]
    ens.engine.calls, ens.engine.flagged = [], None
    step(ens, [0, 1, 2])
    assert ens.engine.calls == [("rvwin", [1], [18], [24]), ("rviews", [0, 0], None, None)]
    assert [a.memory_index for a in ens.agents] == [3, 21, None]
    ens.relocalise()
    assert [a.memory_index for a in ens.agents] == [None, None, None]


def test_without_a_window_the_step_is_the_one_unwindowed_call():
    ens = fake_ensemble([30, 40], [0, 1, 0], [None] * 3, [None] * 3)

    def never(*a, **k):
        raise AssertionError("rvwin_sense_step without a window")
    ens.engine.rvwin_sense_step = never
    for _ in range(3):
        step(ens, [0, 1, 2])
    assert [c[0] for c in ens.engine.calls] == ["rviews"] * 3 and all(c[1] == [0, 1, 0] for c in ens.engine.calls)
    assert [a.memory_index for a in ens.agents] == [None] * 3
    plain = object.__new__(E)                                                               # members made without the new arguments at all
    plain.agents = [types.SimpleNamespace(training_path=np.zeros((30, 2)), memory_bank=0)]
    plain.engine, plain._banks, plain._weights, plain._lands = ens.engine, np.zeros(1, np.int32), np.zeros(1), None
    step(plain, [0])
    assert len(ens.engine.calls) == 4 and not hasattr(plain.agents[0], "memory_index")


def test_window_arguments():
    starts = [(0, (1.0, 1.0), 0.0), (1, (1.0, 1.0), 0.0), (0, (1.0, 1.0), 0.0)]
    lengths = [30, 40]
    assert E._windows_arg(None, None, starts, lengths) == ([None] * 3, [None] * 3)
    assert E._windows_arg(4, None, starts, lengths) == ([(4, 4)] * 3, [None] * 3)
    assert E._windows_arg((2, 3), [1, None, 29], starts, lengths) == ([(2, 3)] * 3, [1, None, 29])
    assert E._windows_arg([(2, 3), None, 5], [1, None, None], starts, lengths) == ([(2, 3), None, (5, 5)], [1, None, None])
    assert E._windows_arg((255, 256), None, starts, lengths)[0][0] == (255, 256) and E._windows_arg((0, 0), None, starts, lengths)[0][0] == (0, 0)
    for window, centres, match in (((600, 0), None, r"behind \+ ahead \+ 1 <= 512"), ((256, 256), None, "<= 512"), (-1, None, "int W >= 0"),
                                   ((1, 2, 3), None, "pair"), (2.5, None, "int W >= 0"), ([(2, 3), None], None, "2 entries for 3 starts"),
                                   ([(2, 3), None, (1, -1)], None, r"window\[2\]"), (None, [1, 1, 1], "window_centres without window"),
                                   ((2, 3), [1, 1], "2 entries for 3 starts"), ((2, 3), [30, 1, 1], r"window_centres\[0\] = 30 outside \[0, 30\)"),
                                   ((2, 3), [1, 40, 1], r"window_centres\[1\] = 40 outside \[0, 40\), the views of route 1"),
                                   ((2, 3), [1, -1, 1], r"window_centres\[1\] = -1"), ((2, 3), [1, 1.0, 1], r"window_centres\[1\] must be None or a view index"),
                                   ([(2, 3), None, 5], [1, 1, None], r"window_centres\[1\] = 1, but member 1 has no window")):
        with pytest.raises(ValueError, match=match):
            E._windows_arg(window, centres, starts, lengths)


def test_the_constructors_refuse_bad_windows_before_they_touch_the_engine():
    route = np.array([[50.0, 50.0], [51.0, 50.0], [52.0, 50.0]])
    starts = [(0, (50.0, 50.0), 0.0)]
    agent = types.SimpleNamespace(familiarity_model=sads_familiarity(0.25), _engine=_NoLibrary(), training_path=None, memory_bank=None)
    for kw, match in ((dict(window=(600, 0)), "<= 512"), (dict(window_centres=[1]), "window_centres without window"),
                      (dict(window=1, window_centres=[3]), r"window_centres\[0\] = 3 outside \[0, 3\)")):
        with pytest.raises(ValueError, match=match):
            E.from_routes_with(agent, [route], starts, **kw)
        with pytest.raises(ValueError, match=match):
            E.from_landscapes(agent, [np.zeros((9, 9, 3), np.uint8)], [(0, route)], starts, **kw)


# ---- facts that keep the GPU tests from being vacuous -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,n_differ", [((7, 5, 1, "random"), 4), ((7, 5, 70, "levels"), 6), ((19, 17, 10, "levels"), 6), ((32, 32, 16, "random"), 6)])
def test_the_windows_change_the_expected_rows(key, n_differ):
    case, (fam, view, best) = HW.expected_case(*key)
    assert case["routes"].tolist() == [4, 0, 2, 4, 1, 3, 2] and np.diff(case["first"])[case["routes"]].tolist() == [1043, 2, 64, 1043, 63, 65, 64]
    differ = [i for i in range(7) if fam[i].tobytes() != case["fam"][i].tobytes() or not np.array_equal(view[i], case["view"][i])]
    assert len(differ) == n_differ and 2 not in differ                                    # member 2's window is its whole route
    assert HW.WINDOWS[3][1] - HW.WINDOWS[3][0] == 512 and HW.WINDOWS[3][0] % 64 and HW.WINDOWS[0][0] // 64 != (HW.WINDOWS[0][1] - 1) // 64
    for i, (lo, hi) in enumerate(HW.WINDOWS):
        assert (view[i] >= lo).all() and (view[i] < hi).all()


def test_the_duplicate_views_first_maximum_depends_on_the_window():
    v, p = HW.duplicates()
    for (lo, hi), at in (((50, 200), 100), ((101, 200), 150), ((0, 200), 10)):
        f = oracle.sads_hsv(np.ascontiguousarray(v[lo:hi]), p, 0.3)
        assert lo + int(np.argmax(f)) == at and f.max() == 64.0
    assert oracle.sads_hsv(np.ascontiguousarray(v[11:100]), p, 0.3).max() < 64.0
    views, patches = HW.identical_run()
    s_hs, s_v = oracle.int_sums(views, patches[0])
    fast = oracle.fam_from_sums(s_hs, s_v, 64, 0.3)
    for lo, hi in ((50, 400), (0, 400)):                                                  # more candidates than the list holds: view 60 wins
        assert int(np.sum(fast[lo:hi] >= fast[lo:hi].max() - 2.0 * HR.delta(64))) >= 300 > HR.CAND_CAP
        assert lo + int(np.argmax(oracle.sads_hsv(np.ascontiguousarray(views[lo:hi]), patches[0], 0.3))) == 60


def test_the_scenarios_shadow_agents_show_the_window():
    win, whole = HW.scenario(True), HW.scenario(False)
    differ = [i for i in range(12) if win[i]["pos"] != whole[i]["pos"]]
    assert differ == [1, 5, 7, 9]
    assert all(r["spans"][0] == (0, r["length"]) and r["memory"][0] is not None for r in win)   # no centres: step 0 scores the whole route
    assert all(s is None or s[1] - s[0] <= 6 for r in win for s in r["spans"][1:])
    # member 9 meets a window clipped at its route's end, and member 11 reaches the end of its route (code 1) inside the fifteen steps
    assert any(s is not None and s[1] == win[9]["length"] and s[1] - s[0] < 6 for s in win[9]["spans"])
    assert [r["code"][-1] for r in win] == [0] * 11 + [1] and win[11]["code"][12:] == [0, 1, 1]
    assert win[11]["spans"][13] is not None and win[11]["spans"][14] is None              # the stopping step was sensed and applied
    assert all(s in (None, (0, r["length"])) for r in whole for s in r["spans"])
