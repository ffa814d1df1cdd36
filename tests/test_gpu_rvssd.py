"""GPU tests of SSD on the route view store (dv_rvssd_*) and navsim_amd.SsdRouteEnsemble.  Every expected value is the NumPy int64
statement of tests/helpers_rvssd.py (held to oracle.ssds by tests/test_rvssd_host.py), the host sensor model's views, or a lone
NavBySceneFamiliarity(ssd_familiarity(channel)) agent with an engine and a route of its own.  Every comparison is np.array_equal on
integers or on the doubles that hold them: no tolerance anywhere."""
import csv
import io

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import ssd_familiarity
from tests import helpers_lands as HL
from tests import helpers_rviews as HR
from tests import helpers_rvssd as HV
from tests import helpers_sensors as HS

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture()
def eng():
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


def check_step(e, c, channel=2, want=None):
    ssd, view, best, scene = want or c["want"]
    r = e.rvssd_step_u8(c["patches"], c["routes"], channel)
    assert np.array_equal(r.angle_ssd, ssd), (channel, np.argwhere(r.angle_ssd != ssd)[:4].tolist())
    assert np.array_equal(r.angle_view, view) and np.array_equal(r.best_idex, best) and not r.flags.any(), channel
    assert np.array_equal(bits(r.angle_familiarity), bits(np.negative(ssd))), channel
    rows = e.rvssd_scene_u8(c["patches"], c["routes"], channel)
    assert [row.shape for row in rows] == [s.shape for s in scene]
    for i, (got, s) in enumerate(zip(rows, scene)):
        assert np.array_equal(got, s), (channel, i)
    return r


# ---- 1. pixel tails, byte range -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(3, 3), (7, 5), (8, 8)])
def test_pixel_tails_on_every_channel(eng, h, w):
    """P = 9 (one partial K-step), 35 (Pw = 9: a second K-step of 3 pixels, dwords past Pw), 64 (no tail)."""
    c = HV.tail_case(h, w)
    eng.rviews_set_u8(c["views"], c["first"])
    for channel in (0, 1, 2):
        check_step(eng, c, channel, c["want"][channel])


def test_sign_edges_of_the_bias_trick(eng):
    c = HV.edge_byte_case()
    eng.rviews_set_u8(c["views"], c["first"])
    check_step(eng, c)


def test_the_largest_value_and_a_random_pair_at_64x64(eng):
    c = HV.extreme_case()
    eng.rviews_set_u8(c["views"], c["first"])
    r = check_step(eng, c)
    assert r.angle_ssd[0, 0] == 266342400.0 and r.angle_view[0, 0] == 0


# ---- 2. route lengths, ties ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant_last", (False, True))
def test_padding_views_never_win(eng, plant_last):
    """Routes of 2, 33, 64, 65 and 130 views: an all-zero patch is closest to the zero bytes that pad a route's last group."""
    c = HV.lengths_case(plant_last)
    eng.rviews_set_u8(c["views"], c["first"])
    r = check_step(eng, c)
    lens = np.array(HV.LENGTHS)[c["routes"]]
    assert (r.angle_view < lens[:, None]).all()
    if plant_last:
        assert np.array_equal(r.angle_view[:, 0], lens - 1)


@pytest.mark.parametrize("second", (40, 70))
def test_ties_go_to_the_least_view_and_the_first_heading(eng, second):
    c = HV.tie_case(second)
    eng.rviews_set_u8(c["views"], c["first"])
    r = check_step(eng, c)
    assert r.angle_view[0].tolist()[1:] == [5, 5] and r.best_idex[0] == 1 and np.signbit(r.angle_familiarity[0, 1])


# ---- 3. column geometry -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HV.GEOMETRIES))
def test_column_geometry(eng, name):
    c = HV.geometry_case(name)
    eng.rviews_set_u8(c["views"], c["first"])
    check_step(eng, c)


def test_a_member_alone_and_among_seventy_gives_identical_rows(eng):
    c = HV.geometry_case("many")
    eng.rviews_set_u8(c["views"], c["first"])
    many = eng.rvssd_step_u8(c["patches"], c["routes"])
    alone = eng.rvssd_step_u8(c["patches"][37:38], c["routes"][37:38])
    assert np.array_equal(alone.angle_ssd[0], many.angle_ssd[37]) and np.array_equal(alone.angle_view[0], many.angle_view[37])
    assert alone.best_idex[0] == many.best_idex[37]
    rows_many = eng.rvssd_scene_u8(c["patches"], c["routes"])
    rows_alone = eng.rvssd_scene_u8(c["patches"][37:38], c["routes"][37:38])
    assert np.array_equal(rows_alone[0], rows_many[37])


# ---- 4. sensed calls ----------------------------------------------------------------------------------------------------------------------------
def test_sensed_calls_on_one_landscape_equal_the_u8_calls_on_the_host_models_views():
    name = "sq"
    t = HL.train_case(name)
    order = np.concatenate(t["first"])
    on0 = order[t["land_of"][order] == 0]                                                 # the route on landscape 0, and once more reversed
    x, y, ang = np.concatenate([t["x"][on0], t["x"][on0][::-1]]), np.concatenate([t["y"][on0], t["y"][on0][::-1]]), \
        np.concatenate([t["angle"][on0], t["angle"][on0][::-1] + 0.1])
    first = HV.first_of([len(on0), len(on0)])
    c = HL.SENSORS[name]
    e = navsim_amd.FamiliarityEngine(device=0)
    try:
        e.set_landscape(HL.lands()[0])
        e.configure_sensor(c["sensor"], c["pixel"], HL.level_tables(name), c["mask"])
        views = e.rviews_set_from_poses(x, y, ang, first)
        assert np.array_equal(views, HL.host_scenes(name, x, y, ang, [0] * len(x)))
        xs, ys = np.array([x[2], x[4] + 0.5, x[1]]), np.array([y[2], y[4] - 0.5, y[1] + 1.0])
        angs = (np.array([ang[2], ang[4], ang[1]])[:, None] + np.array([-0.3, 0.0, 0.2, 0.5])[None, :]) % (2 * np.pi)
        routes = [1, 0, 1]
        patches = np.stack([HL.host_scenes(name, [xs[i]] * 4, [ys[i]] * 4, angs[i], [0] * 4) for i in range(3)])
        for channel in (2, 0):
            want = HV.expected(views, first, patches, routes, channel)
            u8 = e.rvssd_step_u8(patches, routes, channel)
            s = e.rvssd_sense_step(xs, ys, angs, routes, channel)
            for r in (u8, s):
                assert np.array_equal(r.angle_ssd, want[0]) and np.array_equal(r.angle_view, want[1]) and np.array_equal(r.best_idex, want[2])
                assert not r.flags.any()
            rows, flags = e.rvssd_scene(xs, ys, angs, routes, channel, want_flags=True)
            assert not flags.any() and all(np.array_equal(got, w) for got, w in zip(rows, want[3]))
    finally:
        e.close()


def test_sensed_calls_on_a_landscape_set_with_a_sensor_table_and_a_member_off_its_landscape():
    """Two landscapes of different shapes (L0 300 x 300 under E0, L1 211 x 173 under E1), 16 x 8 views; member 2 is on L1 at a place
    that only L0 has: flagged 16 with best_idex -1, its scene row -inf, the others scored."""
    shape, pairs = "wide", ((0, "E0"), (1, "E1"))
    rng = np.random.default_rng(5)
    n_r = (9, 6)
    x, y, ang = rng.uniform(50, 120, 15), rng.uniform(50, 120, 15), rng.uniform(0, 2 * np.pi, 15)
    land_of_view = np.repeat([0, 1], n_r).astype(np.int32)
    first = HV.first_of(n_r)
    c = HS.ENTRIES["OWN"]
    e = navsim_amd.FamiliarityEngine(device=0)
    try:
        e.set_landscape(HL.lands()[0])
        e.configure_sensor(HS.SHAPES[shape], c["pixel"], HS.level_table(shape, "OWN"), c["mask"])
        e.lands_set([HL.lands()[l] for l, _ in pairs])
        e.sensors_set(*HS.table_args(shape, [n for _, n in pairs]))
        views = e.rviews_set_from_poses(x, y, ang, first, land_of_view=land_of_view)
        host = np.stack([HS.host_scene(shape, pairs[l][1], x[v], y[v], ang[v], pairs[l][0]) for v, l in enumerate(land_of_view)])
        assert np.array_equal(views, host)
        xs, ys = np.array([x[1] + 0.4, x[10], HL.ON_L2_OFF_L1[0], x[12] - 0.3]), np.array([y[1], y[10] + 0.6, HL.ON_L2_OFF_L1[1], y[12]])
        angs = (np.array([ang[1], ang[10], 0.3, ang[12]])[:, None] + np.array([0.0, 0.25, -0.25])[None, :]) % (2 * np.pi)
        routes, lands = [0, 1, 1, 1], [0, 1, 1, 1]
        assert all(HS.is_off(shape, "E1", xs[2], ys[2], a, 1) for a in angs[2])
        keep = [0, 1, 3]
        patches = np.stack([np.stack([HS.host_scene(shape, pairs[lands[i]][1], xs[i], ys[i], a, pairs[lands[i]][0]) for a in angs[i]]) for i in keep])
        for channel in (2, 1):
            want = HV.expected(views, first, patches, [routes[i] for i in keep], channel)
            s = e.rvssd_sense_step(xs, ys, angs, routes, channel, land_of_member=lands)
            assert s.flags.tolist() == [0, 0, HL.SENSE_ERROR, 0] and s.best_idex[2] == -1
            assert np.array_equal(s.angle_ssd[keep], want[0]) and np.array_equal(s.angle_view[keep], want[1])
            assert np.array_equal(s.best_idex[keep], want[2])
            rows, flags = e.rvssd_scene(xs, ys, angs, routes, channel, land_of_member=lands, want_flags=True)
            assert flags.tolist() == [0, 0, HL.SENSE_ERROR, 0] and rows[2].shape == (6,) and (rows[2] == -np.inf).all()
            assert all(np.array_equal(rows[i], w) for i, w in zip(keep, want[3]))
    finally:
        e.close()


# ---- 5. scene calls -----------------------------------------------------------------------------------------------------------------------------
def test_scene_rows_are_ragged_per_view_maxima_over_the_headings(eng):
    c = HV.geometry_case("straddle")                                                      # 70 headings: a member's columns in three tiles
    eng.rviews_set_u8(c["views"], c["first"])
    rows = eng.rvssd_scene_u8(c["patches"], c["routes"])
    assert [len(r) for r in rows] == [HV.GEOMETRY_LENGTHS[r] for r in c["routes"]] and len(set(len(r) for r in rows)) == 3
    for i, row in enumerate(rows):
        lib = c["views"][c["first"][c["routes"][i]]:c["first"][c["routes"][i] + 1]]
        assert np.array_equal(row, HV.ssd_rows(lib, c["patches"][i], 2).max(axis=0).astype(np.float64)), i
    n, A = c["patches"].shape[:2]
    out = np.empty(int(sum(len(r) for r in rows)) + 1)
    routes = np.ascontiguousarray(c["routes"])
    rc = eng._lib.dv_rvssd_scene_u8(eng._ctx, N.u8ptr(c["patches"]), n, A, routes.ctypes.data_as(N._i32p), 2, len(out), N.f64ptr(out))
    assert rc == INVALID and b"scene_ssd" in eng._lib.dv_last_error(eng._ctx)


# ---- 6. norm cache ------------------------------------------------------------------------------------------------------------------------------
def test_the_view_norms_follow_the_store_and_the_channel(eng):
    c = HV.tail_case(7, 5)
    other = HV.planes_u8(77, c["views"].shape)                                            # other views of the same shape and routes
    want_other = {ch: HV.expected(other, c["first"], c["patches"], c["routes"], ch) for ch in (0, 2)}
    assert not np.array_equal(want_other[2][0], c["want"][2][0])
    eng.rviews_set_u8(c["views"], c["first"])
    for channel in (2, 0, 2):
        check_step(eng, c, channel, c["want"][channel])
    eng.rviews_set_u8(other, c["first"])                                                  # replaced: the new numbers
    for channel in (2, 0):
        check_step(eng, dict(c, views=other), channel, want_other[channel])
    eng.rviews_clear()
    eng.rviews_set_u8(c["views"], c["first"])                                             # cleared and set: the first store's again
    for channel in (2, 0, 2):
        check_step(eng, c, channel, c["want"][channel])


# ---- 7. state -----------------------------------------------------------------------------------------------------------------------------------
def test_the_sads_step_is_untouched_and_no_store_is_a_state_error(eng):
    s = HR.step_case(7, 5, 70, "levels")
    eng.rviews_set_u8(s["views"], s["first"])
    before = eng.rviews_step_u8(s["patches"], s["routes"], s["weights"])
    assert np.array_equal(bits(before.angle_familiarity), bits(s["fam"]))
    want = HV.expected(s["views"], s["first"], s["patches"], s["routes"], 1)
    r = eng.rvssd_step_u8(s["patches"], s["routes"], 1)
    assert np.array_equal(r.angle_ssd, want[0]) and np.array_equal(r.angle_view, want[1]) and np.array_equal(r.best_idex, want[2])
    rows = eng.rvssd_scene_u8(s["patches"], s["routes"], 1)
    assert all(np.array_equal(got, w) for got, w in zip(rows, want[3]))
    after = eng.rviews_step_u8(s["patches"], s["routes"], s["weights"])
    assert np.array_equal(bits(after.angle_familiarity), bits(before.angle_familiarity)) and np.array_equal(after.angle_view, before.angle_view)
    assert np.array_equal(after.best_idex, before.best_idex)
    # refused tables change nothing, and name the entry
    n, A = s["patches"].shape[:2]
    ssd, view, best = np.empty((n, A)), np.empty((n, A), dtype=np.int64), np.empty(n, dtype=np.int32)

    def raw(routes, channel):
        routes = np.array(routes, dtype=np.int32)
        return eng._lib.dv_rvssd_step_u8(eng._ctx, N.u8ptr(s["patches"]), n, A, routes.ctypes.data_as(N._i32p), channel, N.f64ptr(ssd),
                                         N.i64ptr(view), best.ctypes.data_as(N._i32p))
    bad = s["routes"].copy()
    bad[3] = 6
    assert raw(bad, 2) == INVALID and b"route_of_member[3] = 6" in eng._lib.dv_last_error(eng._ctx)
    assert raw(s["routes"], 3) == INVALID and b"channel 3" in eng._lib.dv_last_error(eng._ctx)
    assert raw(s["routes"], -1) == INVALID
    r = eng.rvssd_step_u8(s["patches"], s["routes"], 1)
    assert np.array_equal(r.angle_ssd, want[0])
    eng.rviews_clear()
    assert raw(s["routes"], 2) == STATE
    eng.rviews_first, eng.rviews_shape = s["first"], (7, 5)                               # (past the engine's own check, to the library's)
    with pytest.raises(N.EngineError, match="no route views"):
        eng.rvssd_step_u8(s["patches"], s["routes"])
    eng.rviews_first = eng.rviews_shape = None
    with pytest.raises(N.EngineError, match="no route views"):
        eng.rvssd_step_u8(s["patches"], s["routes"])


# ---- 8. the ensemble ----------------------------------------------------------------------------------------------------------------------------
ENS_SENSOR, ENS_ANGLES, ENS_STEPS = (16, 16), 10, 25


def make_agent(land, channel):
    return navsim_amd.NavBySceneFamiliarity(np.array(land), ENS_SENSOR, 1.0, n_test_angles=ENS_ANGLES, use_gpu_sensor=True,
                                            familiarity_model=ssd_familiarity(channel))


def ens_routes(two_lands):
    """Three routes, [(landscape_index, path)]: on L0 alone, or routes 0 and 2 on L0 and route 1 on L1 (211 x 173)."""
    r = HL.ens_routes()
    paths = [r[0][1], r[2][1], r[1][1]]
    for p in paths:
        assert (p > 8).all() and (p[:, 0] < 173 - 8).all() and (p[:, 1] < 211 - 8).all()  # inside both landscapes' bounds at 16 x 16
    return [(1 if two_lands and k == 1 else 0, p) for k, p in enumerate(paths)]


def lone_agents(landscapes, routes, starts, channel):
    out = []
    for r, pos, ang in starts:
        l, path = routes[r]
        a = make_agent(landscapes[l], channel)
        a.train_from_path(path)
        a.position, a.angle = pos, ang
        out.append(a)
    return out


def build(two_lands, metrics, channel):
    landscapes = HL.lands()[:2]
    routes = ens_routes(two_lands)
    starts = HL.ens_starts(routes)
    assert len(starts) == 6
    agent = make_agent(landscapes[0], channel)
    if two_lands:
        ens = navsim_amd.SsdRouteEnsemble.from_landscapes(agent, list(landscapes), routes, starts, metrics=metrics)
    else:
        ens = navsim_amd.SsdRouteEnsemble.from_routes_with(agent, [p for _, p in routes], starts, metrics=metrics)
    return ens, landscapes, routes, starts


@pytest.mark.parametrize("two_lands,metrics,channel", [(False, "host", 2), (False, "device", 0), (True, "device", 2)])
def test_ensemble_members_equal_lone_agents(two_lands, metrics, channel):
    ens, landscapes, routes, starts = build(two_lands, metrics, channel)
    lone = lone_agents(landscapes, routes, starts, channel)
    calls = []
    inner = ens.engine.rvssd_sense_step

    def counted(*a, **k):
        calls.append(1)
        return inner(*a, **k)
    ens.engine.rvssd_sense_step = counted
    try:
        assert ens.channel == channel and [a.memory_bank for a in ens.agents] == [r for r, _, _ in starts]
        assert [a.landscape_index for a in ens.agents] == ([routes[r][0] for r, _, _ in starts] if two_lands else [None] * 6)
        for m, a in zip(ens.agents, lone):
            assert np.array_equal(m.training_path, a.training_path) and m.training_path_length == a.training_path_length
            assert np.array_equal(m.familiar_scenes, a.familiar_scenes)
        with pytest.raises(ValueError, match="SsdRouteEnsemble"):
            ens.agents[1].step_forward()
        with pytest.raises(ValueError, match="NavEnsemble does not take a member of a SsdRouteEnsemble"):
            navsim_amd.NavEnsemble(ens.agents)
        for t in range(ENS_STEPS):
            running = bool(ens.active)
            ens.step_forward()
            assert len(calls) == t + 1 or not running                                     # ONE device call a step
            for a in lone:
                if a.stopped_with_exception is None:
                    try:
                        a.step_forward()
                    except navsim_amd.StopNavigationException as stop:
                        a.stopped_with_exception = stop
            for i, (m, a) in enumerate(zip(ens.agents, lone)):
                assert m.position == a.position and m.angle == a.angle, (t, i)
                assert np.array_equal(bits(m.angle_familiarity), bits(a.angle_familiarity)), (t, i)
                code = a.stopped_with_exception.get_code() if a.stopped_with_exception is not None else 0
                assert ens.stop_status[i] == code, (t, i)
                assert m.navigation_error == a.navigation_error and m.percent_recapitulated == a.percent_recapitulated, (t, i)
                assert np.array_equal(m._coverage_array, a._coverage_array), (t, i)
            if t in (0, 9):
                rows = ens.scene_familiarity()
                for i, (m, a) in enumerate(zip(ens.agents, lone)):
                    assert np.array_equal(bits(rows[i]), bits(a.scene_familiarity)), (t, i)
                    assert np.array_equal(bits(m.scene_familiarity), bits(a.scene_familiarity)), (t, i)
        assert 1 in ens.stop_status                                                       # members reached the end of their route on the way
        cover = ens.coverage_summary(0.05)
        for c, a in zip(cover, lone):
            assert float(c["path_coverage"]) == a.percent_recapitulated
    finally:
        ens.engine.rvssd_sense_step = inner
        ens.engine.close()
        for a in lone:
            a.clear_training()
            a._engine.close()


def _csv(rows):
    out = io.StringIO()
    w = csv.DictWriter(out, fieldnames=sorted(rows[0]))
    w.writeheader()
    w.writerows(rows)
    return out.getvalue()


def test_run_ensemble_rows_equal_lone_run_experiment_rows():
    ens, landscapes, routes, starts = build(True, "device", 2)
    try:
        rows = navsim_amd.run_ensemble(ens)
    finally:
        ens.engine.close()
    wants = []
    for a in lone_agents(landscapes, routes, starts, 2):
        try:
            wants.append(navsim_amd.run_experiment(a))
        finally:
            a.clear_training()
            a._engine.close()
    assert _csv(rows) == _csv(wants)
