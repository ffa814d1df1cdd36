"""Routed path metrics without a device: the conditions of tests/helpers_path_routes.py with their figures, the binding surface of the
dv_path_routes_* calls, the Python-side argument checks (made before any library call), and the route ensembles' metrics="device"
mode on a NumPy stand-in engine."""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import mushroom_familiarity, synth
from navsim_amd.engine import OneValueBatchResults
from tests import helpers_mushroom_banks as HB
from tests import helpers_path_routes as HP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"dv_path_routes_set": "path_routes_set", "dv_path_routes_slots": "path_routes_slots", "dv_path_routes_error": "path_routes_error",
         "dv_path_routes_coverage": "path_routes_coverage", "dv_path_routes_reset": "path_routes_reset",
         "dv_path_routes_info": "path_routes_info"}


# ---- the helper's conditions -------------------------------------------------------------------------------------------------------------------
def _planted(name):
    slot, pos, reach = HP.entry(name)
    dist = HP.distances(HP.slot_route(slot), pos)
    return slot, pos, reach, dist


def test_routes_and_slots_are_as_stated():
    R = HP.routes()
    assert tuple(len(r) for r in R) == (1, 2, 1025, 2500, 263200) and all(r.dtype == np.float64 and r.shape[1] == 2 for r in R)
    assert HP.ROUTE_OF_SLOT == (4, 0, 2, 2, 0, 3, 1) and HP.first().tolist() == [0, 1, 3, 1028, 3528, 266728]
    assert len(R[4]) > HP.TRIP == 262144                                                 # a second trip of 256 blocks x 1024 points
    c, _ = HP.calls()
    assert [len(c[k][0]) for k in HP.SEQUENCE] == [1, 65, 130, 65537]
    assert (c["wide"][0] == 6).all() and HP.ROUTE_OF_SLOT[6] == 1 and len(c["wide"][0]) > 65535      # the host loop's second launch
    for slots, xs, ys, reach in c.values():
        assert slots.dtype == np.int32 and slots.min() >= 0 and slots.max() < 7
        assert xs.dtype == ys.dtype == reach.dtype == np.float64 and len(xs) == len(ys) == len(reach) == len(slots)


def test_planted_entries_meet_their_conditions():
    slot, _, reach, dist = _planted("long_second_trip")
    print("long_second_trip: nearest point %d at %.6f, %d points within reach" % (dist.argmin(), dist.min(), (dist <= reach).sum()))
    assert slot == 0 and dist.argmin() == HP.TRIP + 500 >= 262144 and np.flatnonzero(dist <= reach).min() >= 262144
    slot, _, reach, dist = _planted("lone_point_block")
    assert slot == 2 and dist.argmin() == 1024 == len(dist) - 1 and dist.min() <= reach  # block 1 of the 1025-point route holds one point
    slot, _, reach, dist = _planted("partial_block")
    assert slot == 5 and dist.argmin() == 2400 >= 2048 and len(dist) % 1024 != 0 and dist.min() <= reach
    # the 3-4-5 position: its route's point at integer coordinates is the nearest one, at 5.0 exactly
    for name, covered in (("just_short", False), ("exact_reach", True)):
        slot, pos, reach, dist = _planted(name)
        pt = HP.routes()[3][HP.INTEGER_POINT]
        assert slot == 5 and np.array_equal(pt, np.round(pt)) and np.array_equal(pos - pt, [3.0, 4.0])
        assert dist.argmin() == HP.INTEGER_POINT and dist.min() == 5.0 == np.sqrt(9.0 + 16.0) and (dist == 5.0).sum() == 1
        assert bool(dist[HP.INTEGER_POINT] <= reach) is covered and (dist <= reach).sum() == int(covered)
    assert HP.entry("just_short")[2] == np.nextafter(5.0, 0.0) < 5.0 == HP.entry("exact_reach")[2]
    slot, pos, reach, dist = _planted("zero_reach")
    assert slot == 3 and reach == 0.0 and np.array_equal(pos, HP.routes()[2][77]) and np.flatnonzero(dist <= reach).tolist() == [77]
    slot, _, reach, dist = _planted("negative")
    assert slot == 1 and reach < 0 and dist.min() == 0.0 and not (dist <= reach).any()
    slot, _, reach, dist = _planted("everything")
    assert slot == 4 and reach == np.inf and dist.min() == 1000.0 and (dist <= reach).all()
    (sa, pa, ra, da), (sb, pb, rb, db) = _planted("twice_a"), _planted("twice_b")
    c, planted = HP.calls()
    assert sa == sb == 2 and planted["twice_a"][0] == planted["twice_b"][0] and not np.array_equal(pa, pb)
    a, b = da <= ra, db <= rb
    assert a.any() and b.any() and not (a & b).any()                                     # the OR is neither entry's own marks


def test_expected_marks_tell_the_slots_apart():
    want = HP.expected()
    c, planted = HP.calls()
    for name in HP.SEQUENCE:
        nearest, marks = want[name]
        assert nearest.shape == (HP.SIZES[name],) and (nearest >= 0).all() and len(marks) == 7
        assert [len(m) for m in marks] == [HP.ROUTE_POINTS[r] for r in HP.ROUTE_OF_SLOT]
    final = want[HP.SEQUENCE[-1]][1]
    print("marks after the sequence: %r of %r" % ([int(m.sum()) for m in final], [len(m) for m in final]))
    for j, m in enumerate(final):
        if len(m) > 1:                                                                   # (slots 1 and 4 have the one-point route)
            assert m.any() and not m.all(), j
    assert final[1].tolist() == [False] and final[4].tolist() == [True]                  # the pairs that share a route end differently
    assert not np.array_equal(final[2], final[3])
    # the point at distance 5.0: not marked by the call with the shorter reach, marked by the next
    assert not want["b65"][1][5][HP.INTEGER_POINT] and want["c130"][1][5][HP.INTEGER_POINT]
    # the second launch's entries are told by their nearest values: no two positions of the wide call are alike
    wide = c["wide"]
    assert len(set(zip(wide[1][-3:].tolist(), wide[2][-3:].tolist()))) == 3 and len(np.unique(HP.bits(want["wide"][0]))) > 65000
    assert final[6].tolist() == [True, False]
    # the marks past the first trip come from the long route's slot alone
    assert final[0][HP.TRIP:].any() and final[0][:HP.TRIP].any()


# ---- binding surface ---------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_engine_agree_on_the_routed_names():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    declared = set(re.findall(r"\bint\s+(dv_path_routes_[a-z0-9_]*)\s*\(", header))
    assert declared == set(NAMES) == {k for k in N.PROTOTYPES if k.startswith("dv_path_routes_")}
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert N.PROTOTYPES[name][0] is ctypes.c_int
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(N.PROTOTYPES[name][1]), name
        assert callable(getattr(navsim_amd.FamiliarityEngine, NAMES[name])), name
    # a reach per entry, where the one-path call has one for all
    assert N.PROTOTYPES["dv_path_routes_error"][1] == [N._ctx_p, N._i32p, N._f64p, N._f64p, N._f64p, ctypes.c_int64, N._f64p]
    assert N.PROTOTYPES["dv_path_routes_set"][1] == [N._ctx_p, N._f64p, N._i64p, ctypes.c_int]
    # the one-path calls are as they were
    assert N.PROTOTYPES["dv_path_error_batch"][1][-2:] == [ctypes.c_double, N._f64p] and len(N.PROTOTYPES["dv_path_slots"][1]) == 2
    assert len(N.PROTOTYPES["dv_set_training_path"][1]) == 3


# ---- argument checks before the library --------------------------------------------------------------------------------------------------------
class _Recorder(object):
    """Stands where the library does: every call succeeds and is noted as (symbol, number of arguments)."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, len(args)))
            return 0
        return call


def _engine_without_a_device(lib):
    e = navsim_amd.FamiliarityEngine.__new__(navsim_amd.FamiliarityEngine)
    e._lib, e._ctx_raw, e._begun = lib, None, False
    return e


def test_routed_argument_checks_come_before_any_library_call():
    lib = _Recorder()
    e = _engine_without_a_device(lib)
    a, b = np.zeros((3, 2)), np.ones((5, 2))
    for bad in ([a, np.zeros((0, 2))], [a, np.zeros((4, 3))], [a, np.zeros(4)], [a, np.zeros((4, 2), np.float32)], [a, [[1, 2]]], []):
        with pytest.raises(ValueError, match="routes"):
            e.path_routes_set(bad)
    both = np.concatenate([a, b])
    for first, what in (([1, 3, 8], r"first\[0\] must be 0"), ([0, 3, 3], "first must rise"), ([0, 5, 3, 8], "first must rise"),
                        ([0, 3, 7], r"first\[-1\] = 7, but there are 8 points"), ([0.0, 3.0, 8.0], "first must hold integers"),
                        ([0], "first must hold integers"), ([[0, 3, 8]], "first must hold integers")):
        with pytest.raises(ValueError, match=what):
            e.path_routes_set(both, first)
    with pytest.raises(ValueError, match="points must be float64"):
        e.path_routes_set(both.astype(np.float32), [0, 3, 8])
    assert lib.calls == [] and e._route_first is None
    e.path_routes_set([a, b])
    assert lib.calls == [("dv_path_routes_set", 4)] and e._route_first.tolist() == [0, 3, 8] and e._route_of_slot is None
    del lib.calls[:]
    # a route index outside [0, R)
    for bad in ([0, 2], [-1, 0], [0.0, 1.0], [[0, 1]], np.array([0, 1.5])):
        with pytest.raises(ValueError, match="route_of_slot"):
            e.path_routes_slots(bad)
    with pytest.raises(ValueError, match=r"route_of_slot\[1\] = 2 outside \[0, n_routes = 2\)"):
        e.path_routes_slots([0, 2])
    assert lib.calls == [] and e._route_of_slot is None
    e.path_routes_slots([1, 0, 1])
    assert lib.calls == [("dv_path_routes_slots", 3)] and e._route_of_slot.tolist() == [1, 0, 1]
    del lib.calls[:]
    # a slot outside range, a wrong dtype, a wrong length of reach
    ok = np.array([0.5, 1.5])
    for slots, xs, ys, reach, what in (([0, 3], ok, ok, ok, r"slots\[1\] = 3 outside \[0, n_slots = 3\)"), ([-1, 0], ok, ok, ok, "slots"),
                                       ([0.0, 1.0], ok, ok, ok, "slots must hold integers"), ([[0, 1]], ok, ok, ok, "slots must have one dimension"),
                                       ([0, 1], ok.astype(np.float32), ok, ok, "xs must be float64"), ([0, 1], ok, [1, 2], ok, "ys must be float64"),
                                       ([0, 1], ok, ok, np.array([1, 2]), "reach must be float64"),
                                       ([0, 1], ok, ok, np.array([0.5]), r"reach must have shape \(2,\)"), ([0, 1], ok, ok, 0.5, r"reach must have shape \(2,\)"),
                                       ([0, 1], ok[:1], ok, ok, r"xs must have shape \(2,\)"), ([0, 1], ok, np.zeros(3), ok, r"ys must have shape \(2,\)")):
        with pytest.raises(ValueError, match=what):
            e.path_routes_error(slots, xs, ys, reach)
    # n is not the slot's route length; slots that are none
    for slot, n, what in ((0, 3, "n must be 5, the length of slot 0's route"), (1, 5, "n must be 3"), (3, 5, "slot must be an integer in"),
                          (-1, 5, "slot must be an integer in"), (1.0, 3, "slot must be an integer in"), (True, 3, "slot must be an integer in"),
                          (1, 3.0, "n must be")):
        with pytest.raises(ValueError, match=what):
            e.path_routes_coverage(slot, n)
    for slot in (3, 1.0, None, True):
        with pytest.raises(ValueError, match="slot must be an integer"):
            e.path_routes_reset(slot)
    assert lib.calls == []
    # arguments that hold: each method reaches its own symbol, once, with the arguments the binding declares
    assert e.path_routes_error([2, 0], ok, ok, np.array([0.1, np.inf])).shape == (2,)
    assert e.path_routes_coverage(1, 3).shape == (3,)
    e.path_routes_reset(2)
    e.path_routes_reset()
    assert e.path_routes_info() == dict(n_routes=0, n_slots=0, n_points=0)               # (the stand-in writes nothing)
    assert lib.calls == [(s, len(N.PROTOTYPES[s][1])) for s in ("dv_path_routes_error", "dv_path_routes_coverage", "dv_path_routes_reset",
                                                              "dv_path_routes_reset", "dv_path_routes_info")]
    # the slots go with the routes; the routes go with None
    e.path_routes_set(both, [0, 3, 8])
    assert e._route_of_slot is None and e._route_first.tolist() == [0, 3, 8]
    e.path_routes_set(None)
    assert e._route_first is None


# ---- the ensembles' metrics="device" mode on a NumPy stand-in engine -----------------------------------------------------------------------------
class _NumpyEngine(object):
    """What a route ensemble asks of its engine, without a device: the model's calls answer with numbers drawn from a seed (the same for
    the same poses), the routed metric calls with the reference's expression; every call is noted by name."""
    def __init__(self, shape):
        self.calls, self.h, self.w = [], shape[0], shape[1]
        self.routes = self.route_of_slot = self.marks = None

    def _note(self, name, *what):
        self.calls.append((name,) + what)

    def named(self, name):
        return [c for c in self.calls if c[0] == name]

    # the model
    def mb_begin(self, *a):
        self._note("mb_begin")

    def mb_score_u8(self, *a):
        raise AssertionError("a member of a route ensemble steps with its ensemble")

    def mbank_set(self, n):
        self._note("mbank_set", n)

    def mbank_train_from_poses(self, x, y, angle, bank_of_view, want_views=True):
        self._note("mbank_train_from_poses", len(x))
        return np.zeros((len(x), self.h, self.w, 3), dtype=np.uint8)

    def mbank_sense_step_batch(self, x, y, angles, banks):
        self._note("mbank_sense_step_batch", len(x))
        seed = zlib.crc32(np.asarray(x).tobytes() + np.asarray(y).tobytes() + np.asarray(angles).tobytes())
        fam = -np.random.default_rng(seed).integers(0, 20, np.asarray(angles).shape).astype(np.float64)
        return OneValueBatchResults(fam, fam.argmax(axis=1).astype(np.int32), np.zeros(len(fam), dtype=np.uint32))

    # the routed metrics, by the reference's expression
    def path_routes_set(self, routes):
        self._note("path_routes_set", len(routes))
        self.routes, self.route_of_slot, self.marks = [np.array(r) for r in routes], None, None

    def path_routes_slots(self, route_of_slot):
        self._note("path_routes_slots", list(route_of_slot))
        self.route_of_slot = list(route_of_slot)
        self.marks = HP.clear_marks(self.route_of_slot, self.routes)

    def path_routes_error(self, slots, xs, ys, reach):
        self._note("path_routes_error", list(slots), np.asarray(reach).tolist())
        return HP.score(self.marks, list(slots), xs, ys, reach, self.route_of_slot, self.routes)

    def path_routes_coverage(self, slot, n):
        self._note("path_routes_coverage", slot)
        assert n == len(self.marks[slot])
        return self.marks[slot].copy()

    def path_routes_reset(self, slot=-1):
        self._note("path_routes_reset", slot)
        for j in (range(len(self.marks)) if slot < 0 else (slot,)):
            self.marks[j][:] = False

    def __getattr__(self, name):                           # path_error_batch, path_slots, set_training_path, ...: must not be asked
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*a, **k):
            self._note(name)
            raise AssertionError("the route ensemble asked its engine for %s" % name)
        return call


LAND = synth.synth_landscape(3, 300, 4)
ROUTED = ("path_routes_set", "path_routes_slots", "path_routes_error", "path_routes_coverage", "path_routes_reset")


def _ensemble(maker, **kw):
    agent = navsim_amd.NavBySceneFamiliarity(LAND, (12, 10), 1.0, n_test_angles=9, use_gpu_sensor=False,
                                             familiarity_model=mushroom_familiarity(n_kc=300, fan_in=4, seed=3))
    agent._engine = _NumpyEngine((10, 12))
    paths = HB.routes()
    return maker(agent, paths, HB.starts(paths), **kw), paths


def test_device_metrics_take_one_routed_call_a_step_with_every_members_own_reach():
    ens, paths = _ensemble(navsim_amd.MushroomRouteEnsemble.from_routes_with, metrics="device")
    host, _ = _ensemble(navsim_amd.MushroomRouteEnsemble.from_routes_with, metrics="host")
    eng = ens.engine
    assert ens.metrics == "device" and host.metrics == "host"
    assert eng.named("path_routes_set") == [("path_routes_set", 3)] and all(np.array_equal(r, p) for r, p in zip(eng.routes, paths))
    assert eng.named("path_routes_slots") == [("path_routes_slots", [0, 0, 1, 1, 2, 2])]  # a slot per member, in member order
    assert [m._metric_slot for m in ens.agents] == list(range(6)) and all(m._ens is ens and not m._metrics_on_device for m in ens.agents)
    # members with step sizes and factors of their own: every entry carries ITS member's reach
    for k, m in enumerate(ens.agents + host.agents):
        m.coverage_threshold_factor = 0.5 + 0.25 * (k % 6)
    ens.agents[3].max_distance_to_training_path = host.agents[3].max_distance_to_training_path = 2.0     # (above every member's reach)
    for t in range(12):
        before = list(ens.active)
        n_err = len(eng.named("path_routes_error"))
        ens.step_forward()
        host.step_forward()
        err = eng.named("path_routes_error")
        assert len(err) == n_err + 1, t                                                  # ONE routed call a step
        assert err[-1][1] == before and err[-1][2] == [ens.agents[i].coverage_threshold_factor * ens.agents[i].step_size for i in before]
        assert len(set(err[-1][2])) == len(before)
        assert ens.stop_status == host.stop_status, t                                    # "too far" falls in the same step
        for i, (m, a) in enumerate(zip(ens.agents, host.agents)):
            assert m.position == a.position and m.angle == a.angle, (t, i)
            if m._n_navigation_error:
                assert m.navigation_error == a.navigation_error, (t, i)
            assert m.percent_recapitulated == a.percent_recapitulated and m.n_captures() == a.n_captures(), (t, i)
            assert m.percent_recapitulated_forgiving() == a.percent_recapitulated_forgiving(), (t, i)
    assert ens.stop_status[3] == -1 and 0 in ens.stop_status
    assert any(m.percent_recapitulated > 0 for m in ens.agents)
    # reset_error reaches the member's routed slot, and no other
    marked = [j for j in range(6) if eng.marks[j].any()]
    assert len(marked) >= 2
    n_reset, j, others = len(eng.named("path_routes_reset")), marked[-1], [m.copy() for m in eng.marks]
    ens.agents[j].reset_error()
    assert eng.named("path_routes_reset")[n_reset:] == [("path_routes_reset", j)] and not eng.marks[j].any()
    assert all(np.array_equal(eng.marks[k], others[k]) for k in range(6) if k != j)
    assert {c[0] for c in eng.calls} <= set(ROUTED) | {"mb_begin", "mbank_set", "mbank_train_from_poses", "mbank_sense_step_batch"}
    assert not eng.named("path_error_batch") and not eng.named("path_slots") and not eng.named("set_training_path")


def test_a_limit_below_the_reach_marks_in_a_second_call_and_only_within_the_limit():
    """The reference stops a member that is too far before it marks anything: a member whose max_distance_to_training_path is below
    its reach sends a reach that marks nothing, and its marks follow once its distance is known."""
    ens, _ = _ensemble(navsim_amd.MushroomRouteEnsemble.from_routes_with, metrics="device")
    host, _ = _ensemble(navsim_amd.MushroomRouteEnsemble.from_routes_with, metrics="host")
    eng = ens.engine
    for e in (ens, host):
        for k in (1, 2, 5):
            e.agents[k].max_distance_to_training_path = (0.6, 0.75, 0.7)[k % 3]          # below the reach, 0.8
    second = 0
    for t in range(10):
        before = list(ens.active)
        n_err = len(eng.named("path_routes_error"))
        ens.step_forward()
        host.step_forward()
        err = eng.named("path_routes_error")[n_err:]
        late = [i for i in before if i in (1, 2, 5)]
        assert len(err) in ((1, 2) if late else (1,)) and err[0][1] == before, t
        assert err[0][2] == [-1.0 if i in late else 0.8 for i in before], t
        if len(err) == 2:
            second += 1
            assert set(err[1][1]) <= set(late) and err[1][2] == [0.8] * len(err[1][1]), t
            assert all(ens.stop_status[i] == 0 for i in err[1][1]), t                    # marked: within its limit
        assert ens.stop_status == host.stop_status, t
        for i, (m, a) in enumerate(zip(ens.agents, host.agents)):
            assert m.position == a.position and np.array_equal(m._coverage_array, a._coverage_array), (t, i)
            assert m._navigation_error == a._navigation_error and m._n_navigation_error == a._n_navigation_error, (t, i)
    assert second and [ens.stop_status[k] for k in (1, 2, 5)].count(-1) >= 1 and any(eng.marks[k].any() for k in (1, 2, 5))


@pytest.mark.parametrize("kw", [dict(), dict(metrics="host")])
def test_host_metrics_touch_none_of_the_routed_calls(kw):
    maker = navsim_amd.MushroomRouteEnsemble.from_routes if not kw else navsim_amd.MushroomRouteEnsemble.from_routes_with
    ens, _ = _ensemble(maker, **kw)
    for _ in range(4):
        ens.step_forward()
    for m in ens.agents:
        assert m._metric_slot is None and m._ens is None and not m._metrics_on_device
        assert m.navigation_error >= 0 and 0 <= m.percent_recapitulated <= 1
        m.reset_error()
    assert ens.metrics == "host" and not any(c[0].startswith("path_") or c[0] == "set_training_path" for c in ens.engine.calls)
    assert len(ens.engine.named("mbank_sense_step_batch")) == 4


def test_an_unknown_metrics_value_is_refused():
    for cls in (navsim_amd.MushroomRouteEnsemble, navsim_amd.InfomaxRouteEnsemble):
        for bad in ("gpu", "", None, True):
            with pytest.raises(ValueError, match="metrics must be one of"):
                cls.from_routes_with(object(), [], [], metrics=bad)
            with pytest.raises(ValueError, match="metrics must be one of"):
                cls([], metrics=bad)
