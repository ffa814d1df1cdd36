"""Routed path metrics on the device (dv_path_routes_*, k_path_error_routes) against the reference's NumPy expression on the inputs of
tests/helpers_path_routes.py: np.array_equal on the marks and on the uint64 view of `nearest`, no tolerances -- the square root and the
two products are correctly rounded on both sides.  Then the route ensembles with metrics="device" against lone agents whose metrics
run on the host."""
import csv
import io

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import infomax_familiarity, mushroom_familiarity, synth
from tests import helpers_infomax_banks as HIB
from tests import helpers_mushroom_banks as HMB
from tests import helpers_path_routes as HP

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -3


@pytest.fixture
def eng():
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


def _routed(e):
    e.path_routes_set(HP.routes())
    e.path_routes_slots(HP.ROUTE_OF_SLOT)
    return e


def _all_marks(e):
    return [e.path_routes_coverage(j, HP.ROUTE_POINTS[r]) for j, r in enumerate(HP.ROUTE_OF_SLOT)]


def _same_marks(e, want, note):
    for j, (got, w) in enumerate(zip(_all_marks(e), want)):
        assert got.dtype == np.bool_ and np.array_equal(got, w), (note, j, np.flatnonzero(got != w)[:8])


# ---- 1. the helper's calls ------------------------------------------------------------------------------------------------------------------------
def test_every_call_gives_numpys_bits_and_every_slots_whole_array(eng):
    """After EVERY call nearest has NumPy's bits and ALL seven slots' whole arrays are the host's: the slots lie back to back, so a store
    one byte past a slot's end shows in the next."""
    _routed(eng)
    assert eng.path_routes_info() == dict(n_routes=5, n_slots=7, n_points=sum(HP.ROUTE_POINTS))
    _same_marks(eng, HP.clear_marks(), "cleared")
    c, planted = HP.calls()
    want = HP.expected()
    for name in HP.SEQUENCE:
        slots, xs, ys, reach = c[name]
        nearest = eng.path_routes_error(slots, xs, ys, reach)
        bad = np.flatnonzero(HP.bits(nearest) != HP.bits(want[name][0]))
        print("%s: %d entries, %d differ" % (name, len(slots), len(bad)))
        assert nearest.dtype == np.float64 and not len(bad), (name, bad[:8], nearest[bad[:8]], want[name][0][bad[:8]])
        _same_marks(eng, want[name][1], name)
    call, e = planted["just_short"]
    assert call == "b65" and HP.bits(want[call][0][e:e + 1])[0] == HP.bits(np.array([5.0]))[0]


# ---- 2. reset, slots again, routes again -------------------------------------------------------------------------------------------------------------
def test_reset_clears_one_slot_or_all_and_new_routes_drop_the_slots(eng):
    _routed(eng)
    c, _ = HP.calls()
    want = HP.expected()
    for name in ("one", "b65"):
        eng.path_routes_error(*c[name])
    marks = [m.copy() for m in want["b65"][1]]
    assert marks[2].any() and marks[3].any() and marks[0].any()
    eng.path_routes_reset(2)                                                             # its neighbours 1 and 3 keep theirs
    marks[2][:] = False
    _same_marks(eng, marks, "reset(2)")
    eng.path_routes_reset(-1)
    _same_marks(eng, HP.clear_marks(), "reset(-1)")
    eng.path_routes_error(*c["one"])
    _same_marks(eng, want["one"][1], "after reset")
    # slots again: cleared, and made anew -- here three of them, in another order
    eng.path_routes_slots([2, 4, 2])
    assert eng.path_routes_info() == dict(n_routes=5, n_slots=3, n_points=sum(HP.ROUTE_POINTS))
    assert [len(eng.path_routes_coverage(j, n)) for j, n in enumerate((1025, 263200, 1025))] == [1025, 263200, 1025]
    assert not any(eng.path_routes_coverage(j, n).any() for j, n in enumerate((1025, 263200, 1025)))
    slot, pos, reach = HP.entry("long_second_trip")
    nearest = eng.path_routes_error([1], pos[:1], pos[1:], np.array([reach]))
    dist = HP.distances(HP.routes()[4], pos)
    assert HP.bits(nearest)[0] == HP.bits(dist[dist.argmin():][:1])[0] and np.array_equal(eng.path_routes_coverage(1, 263200), dist <= reach)
    assert not eng.path_routes_coverage(0, 1025).any() and not eng.path_routes_coverage(2, 1025).any()
    with pytest.raises(ValueError, match="slot must be an integer in"):
        eng.path_routes_coverage(3, 1025)
    # routes again: the slots are gone, and the metric call is a state error
    eng.path_routes_set(HP.routes()[:3])
    assert eng.path_routes_info() == dict(n_routes=3, n_slots=0, n_points=1028)
    one = np.zeros(1)
    slots = np.zeros(1, dtype=np.int32)
    assert eng._lib.dv_path_routes_error(eng._ctx, slots.ctypes.data_as(N._i32p), N.f64ptr(one), N.f64ptr(one), N.f64ptr(one), 1, N.f64ptr(one)) == STATE
    assert eng._lib.dv_path_routes_reset(eng._ctx, -1) == STATE
    with pytest.raises(N.EngineError, match="DV_ERR_STATE"):
        eng.path_routes_error([0], one, one, one)
    eng.path_routes_set(None)
    assert eng.path_routes_info() == dict(n_routes=0, n_slots=0, n_points=0)
    assert eng._lib.dv_path_routes_slots(eng._ctx, slots.ctypes.data_as(N._i32p), 1) == STATE
    with pytest.raises(N.EngineError, match="DV_ERR_STATE"):
        eng.path_routes_slots([0])


# ---- 3. refusals at the C level ------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_marks_and_state_as_they_were(eng):
    _routed(eng)
    c, _ = HP.calls()
    want = HP.expected()
    eng.path_routes_error(*c["one"])
    eng.path_routes_error(*c["b65"])
    lib, ctx, info = eng._lib, eng._ctx, eng.path_routes_info()
    slots, xs, ys, reach = [np.array(a) for a in c["c130"]]
    reach[:] = np.inf                                                                    # (were any entry to run, it would mark a whole route)
    nearest = np.full(len(slots), -7.0)
    for bad in (7, -1, 1 << 20):
        slots[64] = bad                                                                  # in the middle of the table
        assert lib.dv_path_routes_error(ctx, slots.ctypes.data_as(N._i32p), N.f64ptr(xs), N.f64ptr(ys), N.f64ptr(reach), len(slots),
                                        N.f64ptr(nearest)) == INVALID
        assert b"slots[64]" in lib.dv_last_error(ctx)
        assert (nearest == -7.0).all()
    out = np.full(2600, 9, dtype=np.uint8)
    for slot, n in ((5, 2499), (5, 2501), (5, 0), (6, 1), (7, 2500), (-1, 2500)):
        assert lib.dv_path_routes_coverage(ctx, slot, N.u8ptr(out), n) == INVALID, (slot, n)
    assert (out == 9).all()
    assert lib.dv_path_routes_reset(ctx, 7) == INVALID
    table = np.array([4, 0, 5, 1], dtype=np.int32)
    assert lib.dv_path_routes_slots(ctx, table.ctypes.data_as(N._i32p), 4) == INVALID and b"route_of_slot[2]" in lib.dv_last_error(ctx)
    first = np.array([0, 4, 4, 9], dtype=np.int64)
    pts = np.zeros((9, 2))
    assert lib.dv_path_routes_set(ctx, N.f64ptr(pts), N.i64ptr(first), 3) == INVALID
    first[:] = [1, 4, 6, 9]
    assert lib.dv_path_routes_set(ctx, N.f64ptr(pts), N.i64ptr(first), 3) == INVALID
    assert eng.path_routes_info() == info
    _same_marks(eng, want["b65"][1], "after the refusals")
    # ... and the next call goes on from there
    nearest = eng.path_routes_error(*c["c130"])
    assert np.array_equal(HP.bits(nearest), HP.bits(want["c130"][0]))
    _same_marks(eng, want["c130"][1], "c130")


# ---- 4. the one-path calls and the routed ones do not meet --------------------------------------------------------------------------------------------
def _one_path_calls(e):
    """set_training_path + path_slots + path_error_batch on a 300-point path, and what the single agent's calls give on it."""
    rng = np.random.default_rng(5)
    path = np.stack([40.0 + 0.9 * np.arange(300), 80.0 + 6.0 * np.sin(np.arange(300) / 9.0)], axis=1)
    e.set_training_path(path)
    e.path_slots(5)
    out = []
    for n in (3, 70):
        slots = rng.integers(0, 5, n)
        at = path[rng.integers(0, 300, n)] + rng.uniform(-1.0, 1.0, (n, 2))
        out.append(e.path_error_batch(slots, at[:, 0], at[:, 1], 1.3))
    out.extend(e.path_coverage_slot(j, 300) for j in range(5))
    e.path_error_enqueue(51.0, 82.0, 2.0)
    out.append(np.array([e.path_error_wait()]))
    out.append(e.path_coverage(300))
    return path, out


def test_the_one_path_calls_and_the_routed_calls_leave_each_other_alone(eng):
    fresh = navsim_amd.FamiliarityEngine(device=0)
    try:
        path, want_one = _one_path_calls(fresh)
    finally:
        fresh.close()
    assert want_one[0].shape == (3,) and want_one[2].shape == (300,) and any(w.any() for w in want_one[2:7])
    _routed(eng)
    c, _ = HP.calls()
    want = HP.expected()
    eng.path_routes_error(*c["one"])
    eng.path_routes_error(*c["b65"])
    _, got_one = _one_path_calls(eng)
    for k, (g, w) in enumerate(zip(got_one, want_one)):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g, w.view(np.uint64) if w.dtype == np.float64 else w), k
    _same_marks(eng, want["b65"][1], "after the one-path calls")
    nearest = eng.path_routes_error(*c["c130"])
    assert np.array_equal(HP.bits(nearest), HP.bits(want["c130"][0]))
    _same_marks(eng, want["c130"][1], "c130")
    assert np.array_equal(eng.path_coverage_slot(2, 300), want_one[4])                   # the one-path slots kept theirs meanwhile
    eng.path_routes_set(None)
    assert eng.path_routes_info()["n_routes"] == 0
    assert np.array_equal(eng.path_coverage_slot(2, 300), want_one[4]) and np.array_equal(eng.path_coverage(300), want_one[-1])
    eng.path_reset_slot(-1)
    eng.path_reset()
    _, again = _one_path_calls(eng)
    for k, (g, w) in enumerate(zip(again, want_one)):
        assert np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g, w.view(np.uint64) if w.dtype == np.float64 else w), k
    eng.set_training_path(None)


# ---- 5. the ensembles ------------------------------------------------------------------------------------------------------------------------------------
MODELS = {
    "mushroom": (navsim_amd.MushroomRouteEnsemble, HMB, (12, 10), lambda: mushroom_familiarity(n_kc=1043, fan_in=8, sparsity=0.02, seed=6)),
    "infomax": (navsim_amd.InfomaxRouteEnsemble, HIB, HIB.ENSEMBLE_SENSOR, lambda: infomax_familiarity(**HIB.ENSEMBLE_MODEL)),
}
TOO_FAR = 0.6        # the routes' points lie 1.0 apart and the steps are 1.0 long: a member half-way between two points is 0.5 from both,
                     # and the members that start beside their route start 0.78 from its nearest point


def _agent(model, max_distance, factor=0.8):
    return navsim_amd.NavBySceneFamiliarity(synth.synth_landscape(3, 300, 4), MODELS[model][2], 1.0, n_test_angles=9, use_gpu_sensor=True,
                                            max_distance_to_training_path=max_distance, coverage_threshold_factor=factor,
                                            familiarity_model=MODELS[model][3]())


def _lone(model, paths, starts, max_distance, host_metrics, factor=0.8):
    out = []
    for r, pos, ang in starts:
        a = _agent(model, max_distance, factor)
        a.train_from_path(paths[r])
        if host_metrics:
            a._engine.set_training_path(None)
            a._metrics_on_device = False                                                 # update_error's NumPy branch
            a.reset_error()
        a.position, a.angle = pos, ang
        out.append(a)
    return out


# (the reach is factor x step_size = factor: with 0.5 the limit TOO_FAR lies above it and a step takes ONE routed call; with 0.8 the limit
# lies below it, and the marks of a member found within its limit follow in a second call)
@pytest.mark.parametrize("model,max_distance,factor", [("mushroom", np.inf, 0.8), ("infomax", np.inf, 0.8), ("mushroom", TOO_FAR, 0.5),
                                                       ("mushroom", TOO_FAR, 0.8)])
def test_device_metric_members_equal_lone_agents_with_host_metrics(model, max_distance, factor):
    cls, H, _, _ = MODELS[model]
    paths = H.routes()
    starts = H.starts(paths)
    ens = cls.from_routes_with(_agent(model, max_distance, factor), paths, starts, metrics="device")
    alone = _lone(model, paths, starts, max_distance, True, factor)
    per_step = 1 if max_distance >= factor else 2
    calls = []
    inner = ens.engine.path_routes_error

    def counted(slots, xs, ys, reach):
        calls.append(list(slots))
        return inner(slots, xs, ys, reach)
    ens.engine.path_routes_error = counted
    try:
        assert len(ens.agents) == 6 and all(m._metric_slot == j and m._ens is ens and not m._metrics_on_device for j, m in enumerate(ens.agents))
        assert all(not a._metrics_on_device and a._metric_slot is None for a in alone)
        assert ens.engine.path_routes_info() == dict(n_routes=3, n_slots=6, n_points=sum(len(p) for p in paths))
        stopped_at = {}
        for t in range(15):
            before, n_calls = list(ens.active), len(calls)
            ens.step_forward()
            if per_step == 1:
                assert len(calls) == n_calls + (1 if before else 0), t                   # exactly ONE routed metrics call a step
            assert len(calls) <= n_calls + per_step and (not before or len(calls[n_calls]) <= len(before)), t
            for k, a in enumerate(alone):
                if a.stopped_with_exception is None:
                    try:
                        a.step_forward()
                    except navsim_amd.StopNavigationException as stop:
                        a.stopped_with_exception = stop
                        stopped_at[k] = (t, stop.get_code())
            for i, (m, a) in enumerate(zip(ens.agents, alone)):
                assert m.position == a.position and m.angle == a.angle, (t, i)
                code = a.stopped_with_exception.get_code() if a.stopped_with_exception is not None else 0
                assert ens.stop_status[i] == code, (t, i)                                # stopped in the same step, with the same code
                assert m.navigated_for_frames == a.navigated_for_frames and m._n_navigation_error == a._n_navigation_error, (t, i)
                if a._n_navigation_error:
                    assert m.navigation_error == a.navigation_error, (t, i)
                assert m.percent_recapitulated == a.percent_recapitulated, (t, i)
                assert m.percent_recapitulated_forgiving() == a.percent_recapitulated_forgiving() and m.n_captures() == a.n_captures(), (t, i)
                assert np.array_equal(m._coverage_array, a._coverage_array), (t, i)
        print("%s, max distance %r, reach %r: stops %r, routed calls %d" % (model, max_distance, factor, stopped_at, len(calls)))
        if np.isfinite(max_distance):
            assert -1 in [code for _, code in stopped_at.values()]
        assert any(m.percent_recapitulated > 0 for m in ens.agents)
    finally:
        ens.engine.path_routes_error = inner
        ens.agents[0].clear_training()
        for a in alone:
            a.clear_training()


def _csv(rows):
    out = io.StringIO()
    w = csv.DictWriter(out, fieldnames=sorted(rows[0]))
    w.writeheader()
    w.writerows(rows)
    return out.getvalue()


@pytest.mark.parametrize("model", ["mushroom", "infomax"])
def test_run_ensemble_rows_equal_host_metric_rows_and_lone_run_experiment_rows(model):
    cls, H, _, _ = MODELS[model]
    paths = H.routes()
    starts = H.starts(paths)
    texts = []
    for metrics in ("device", "host"):
        ens = cls.from_routes_with(_agent(model, np.inf), paths, starts, metrics=metrics)
        try:
            texts.append(_csv(navsim_amd.run_ensemble(ens)))
        finally:
            ens.agents[0].clear_training()
    wants = []
    for a in _lone(model, paths, starts, np.inf, host_metrics=False):
        try:
            wants.append(navsim_amd.run_experiment(a))
        finally:
            a.clear_training()
    assert texts[0] == texts[1] == _csv(wants)
