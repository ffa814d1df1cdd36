"""GPU tests of the route view store (dv_rviews_*) and navsim_amd.SadsRouteEnsemble against oracle.step / oracle.sads_hsv (pinned by
tests/golden/) on every member's OWN route's views, against the golden tie and trajectory fixtures, and against lone agents that each
have an engine, a landscape and a route of their own.  Familiarities are compared on their bits (np.array_equal) unless stated."""
import csv
import io

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import synth
from oracle import oracle
from tests import helpers_lands as HL
from tests import helpers_rviews as HR
from tests.helpers import engine_with, sha, step_case_inputs
from tests.test_host_logic import _run_trajectory

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture()
def eng():
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


def check_step(e, c, **kw):
    """The fast form and the exact form both give the oracle's record of every member."""
    for exact in (False, True):
        r = e.rviews_step_u8(c["patches"], c["routes"], c["weights"], exact=exact, **kw)
        assert np.array_equal(bits(r.angle_familiarity), bits(c["fam"])), exact
        assert np.array_equal(r.angle_view, c["view"]), exact
        assert np.array_equal(r.best_idex, c["best"]) and not r.flags.any(), exact


# ---- 1. rviews_step_u8 against oracle.step per member ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,A,kind", [(7, 5, 1, "random"), (7, 5, 70, "levels"), (19, 17, 10, "levels"), (19, 17, 70, "random"),
                                         (32, 32, 16, "random"), (32, 32, 10, "levels"), (5, 7, 260, "random")])
def test_step_equals_the_oracle_on_every_members_own_route(eng, h, w, A, kind):
    c = HR.step_case(h, w, A, kind)
    assert len(set(c["weights"].tolist())) == 3 and sorted(set(c["routes"].tolist())) == [0, 1, 2, 3, 4]
    eng.rviews_set_u8(c["views"], c["first"])
    info = eng.rviews_info()
    assert info["n_routes"] == 6 and np.array_equal(info["first"], c["first"]) and info["shape"] == (h, w)
    check_step(eng, c)
    sc = eng.rviews_scene_u8(c["patches"], c["routes"], c["weights"])
    for got, want in zip(sc, c["scene"]):
        assert np.array_equal(bits(got), bits(want))


def test_wide_views_tile_the_headings_in_lds(eng):
    """64 x 64: 12 KiB of planes a patch, four patches a tile; 60 headings on a route of 70 views (and a route of 3)."""
    c = HR.step_case(64, 64, 60, "random", lengths=(70, 3), routes=(1, 0, 0), weights=(0.3, 0.0, 1.0))
    eng.rviews_set_u8(c["views"], c["first"])
    check_step(eng, c)


@pytest.mark.parametrize("slab", ["37", "1"])
def test_columns_cross_a_slab_edge_inside_a_member(slab):
    """DEJAVU_RVIEWS_SLAB (read when the engine is created): 70 columns in slabs of 37 (an edge inside a member) and of 1."""
    c = HR.step_case(19, 17, 10, "levels")
    assert 37 % 10 and c["routes"][HR.sorted_member_at(c["routes"], 10, 37)] != c["routes"][0]
    e = engine_with({"DEJAVU_RVIEWS_SLAB": slab})
    try:
        e.rviews_set_u8(c["views"], c["first"])
        check_step(e, c)
    finally:
        e.close()


def test_columns_cross_the_default_slab_edge(eng):
    """30 members x 260 headings = 7 800 columns; the default slab holds 7 710 (the longest route has 1 043 views)."""
    routes, weights = HR.WIDE_ROUTES, HR.WIDE_WEIGHTS
    edge = HR.slab_columns(1043)
    assert edge == 7710 and edge % 260 and routes[HR.sorted_member_at(routes, 260, edge)] != routes[0]
    c = HR.step_case(7, 5, 260, "random", routes=routes, weights=weights)
    eng.rviews_set_u8(c["views"], c["first"])
    check_step(eng, c)


# ---- 2. ties -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s_ties_8x8", "s_ties_8x8_cw", "s_ties_4x4"])
def test_golden_tie_fixtures_behind_a_decoy_route(eng, manifest, golden, name):
    case = [c for c in manifest["t2_step"] if c["name"] == name][0]
    z = golden("t2_step.npz")
    lib, patches = step_case_inputs(case)
    decoy = synth.synth_views(5, 9, case["h"], case["w"])
    eng.rviews_set_u8(np.concatenate([decoy, lib]), [0, 9, 9 + len(lib)])
    for exact in (False, True):
        r = eng.rviews_step_u8(patches[None], [1], [case["chem_weight"]], exact=exact)
        assert np.array_equal(bits(r.angle_familiarity[0]), bits(z[name + "_angle"])), exact
        assert r.best_idex[0] == case["best_idex"] and r.angle_view[0, case["best_idex"]] == case["best_view"], exact
        assert r.angle_familiarity[0, case["best_idex"]] == case["step_familiarity"], exact
    sc = eng.rviews_scene_u8(patches[None], [1], [case["chem_weight"]])[0]
    assert np.array_equal(bits(sc), bits(z[name + "_scene"]))


def test_permuted_views_make_several_candidates_and_the_first_exact_maximum_wins(eng):
    views, patch = HR.permuted_route(8, 8, 40, 3)
    decoy = synth.random_hsv(9, (4, 8, 8, 3))
    patches = np.stack([patch, views[5]])[None]                                           # a tie of all 40, and a plain heading
    for cw in (0.3, 0.0, 1.0):
        fam, view, best, most = HR.statement(views, patches[0], cw)
        assert most == 40
        want = oracle.step(views, patches[0], cw)
        eng.rviews_set_u8(np.concatenate([decoy, views]), [0, 4, 44])
        for exact in (False, True):
            r = eng.rviews_step_u8(patches, [1], [cw], exact=exact)
            assert np.array_equal(bits(r.angle_familiarity[0]), bits(want["angle_familiarity"])) and r.best_idex[0] == want["best_idex"]
            assert np.array_equal(r.angle_view[0], view)


def test_five_thousand_identical_views_overflow_the_list_and_view_0_wins(eng):
    view = synth.random_hsv(4, (8, 8, 3))
    views = np.repeat(view[None], 5000, axis=0)
    other = synth.random_hsv(6, (300, 8, 8, 3))
    patches = synth.random_hsv(8, (2, 3, 8, 8, 3))
    eng.rviews_set_u8(np.concatenate([other, views]), [0, 300, 5300])
    routes, weights = [1, 0], [0.3, 0.3]                                                  # the overflowing member beside one that does not
    assert 5000 > HR.CAND_CAP
    for exact in (False, True):
        r = eng.rviews_step_u8(patches, routes, weights, exact=exact)
        want = oracle.step(views, patches[0], 0.3)
        assert np.array_equal(bits(r.angle_familiarity[0]), bits(want["angle_familiarity"])) and (r.angle_view[0] == 0).all()
        want = oracle.step(other, patches[1], 0.3)
        assert np.array_equal(bits(r.angle_familiarity[1]), bits(want["angle_familiarity"]))
        assert r.angle_view[1, want["best_idex"]] == want["best_view"] and r.best_idex[1] == want["best_idex"]


# ---- 3. sensing --------------------------------------------------------------------------------------------------------------------------------
def sensor_engine(name, land):
    c = HL.SENSORS[name]
    e = navsim_amd.FamiliarityEngine(device=0)
    e.set_landscape(land)
    e.configure_sensor(c["sensor"], c["pixel"], HL.level_tables(name), c["mask"])
    return e


@pytest.mark.parametrize("name", ["sq", "px"])
def test_set_from_poses_senses_every_route_on_its_own_landscape(name):
    t = HL.train_case(name)
    order = np.concatenate(t["first"])                                                    # the case interleaves its routes: route by route here
    x, y, ang, land_of = t["x"][order], t["y"][order], t["angle"][order], t["land_of"][order]
    first = HR.first_of([len(f) for f in t["first"]])
    e = sensor_engine(name, HL.lands()[0])
    try:
        e.lands_set(list(HL.lands()))
        views = e.rviews_set_from_poses(x, y, ang, first, land_of_view=land_of)
        assert np.array_equal(views, t["scenes"][order])
        # the store holds those views: a patch that is a view of route r scores h * w there, at that view
        w, h = HL.SENSORS[name]["sensor"]
        patches = np.stack([views[first[r] + 3] for r in range(3)])[:, None]
        r = e.rviews_step_u8(patches, [0, 1, 2], [0.3, 0.3, 0.3])
        assert (r.angle_familiarity == h * w).all() and (r.angle_view[:, 0] <= 3).all()
        # ... and sensed steps see each member's own landscape
        k = first[1] + 2
        s = e.rviews_sense_step([x[k], x[k]], [y[k], y[k]], [[ang[k]], [ang[k]]], [1, 1], [0.0, 0.0], land_of_member=[land_of[k], 0])
        assert s.angle_familiarity[0, 0] == h * w and s.angle_view[0, 0] <= 2 and s.angle_familiarity[1, 0] < h * w and not s.flags.any()
        # a view off its own landscape: IndexError names it, the store stays
        before = e.rviews_step_u8(patches, [0, 1, 2], [0.3, 0.0, 1.0])
        v, bx, by = HL.off_own_landscape_view(name)
        v = int(np.flatnonzero(order == v)[0])
        x2, y2 = x.copy(), y.copy()
        x2[v], y2[v] = bx, by
        with pytest.raises(IndexError, match="view %d " % v):
            e.rviews_set_from_poses(x2, y2, ang, first, land_of_view=land_of)
        after = e.rviews_step_u8(patches, [0, 1, 2], [0.3, 0.0, 1.0])
        assert np.array_equal(bits(after.angle_familiarity), bits(before.angle_familiarity)) and np.array_equal(e.rviews_info()["first"], first)
        # without a table: the engine's one landscape
        one = e.rviews_set_from_poses(x[:first[1]], y[:first[1]], ang[:first[1]], [0, first[1]])
        assert np.array_equal(one, HL.host_scenes(name, x[:first[1]], y[:first[1]], ang[:first[1]], [0] * int(first[1])))
    finally:
        e.close()


def test_sensed_scene_flags_the_member_off_its_landscape_and_checks_n_out_first():
    t = HL.train_case("sq")
    order = np.concatenate(t["first"])
    x, y, ang, land_of = t["x"][order], t["y"][order], t["angle"][order], t["land_of"][order]
    first = HR.first_of([len(f) for f in t["first"]])
    e = sensor_engine("sq", HL.lands()[0])
    try:
        e.lands_set(list(HL.lands()))
        views = e.rviews_set_from_poses(x, y, ang, first, land_of_view=land_of)
        at = [int(first[r]) + 4 for r in range(3)]
        xs, ys = x[at].copy(), y[at].copy()
        angs = (ang[at][:, None] + np.array([-0.4, 0.0, 0.3])[None, :]) % (2 * np.pi)
        lands, weights = land_of[at].copy(), [0.3, 0.0, 1.0]
        xs[1], ys[1] = HL.ON_L2_OFF_L1[:2]                                                  # member 1 (on L1) leaves its own landscape
        assert lands[1] == 1 and all(HL.is_off("sq", xs[1], ys[1], a, 1) for a in angs[1])
        rows, flags = e.rviews_scene(xs, ys, angs, [0, 1, 2], weights, land_of_member=lands, want_flags=True)
        assert flags.tolist() == [0, HL.SENSE_ERROR, 0] and np.isinf(rows[1]).all() and rows[1].shape == (int(first[2] - first[1]),)
        step = e.rviews_sense_step(xs, ys, angs, [0, 1, 2], weights, land_of_member=lands)
        assert step.flags.tolist() == [0, HL.SENSE_ERROR, 0] and step.best_idex[1] == -1
        for i in (0, 2):
            patches = HL.host_scenes("sq", [xs[i]] * 3, [ys[i]] * 3, angs[i], [lands[i]] * 3)
            want = oracle.step(views[first[i]:first[i + 1]], patches, weights[i])
            assert np.array_equal(bits(rows[i]), bits(want["scene_familiarity"]))
            assert np.array_equal(bits(step.angle_familiarity[i]), bits(want["angle_familiarity"])) and step.best_idex[i] == want["best_idex"]
        # a scene_fam of the wrong length is refused by name before anything is sensed
        routes, w = np.array([0, 1, 2], dtype=np.int32), np.array(weights)
        tab, out = lands.astype(np.int32), np.empty(int(first[3]) + 1)
        rc = e._lib.dv_rviews_scene(e._ctx, N.f64ptr(xs), N.f64ptr(ys), N.f64ptr(angs), 3, 3, routes.ctypes.data_as(N._i32p), N.f64ptr(w),
                                    tab.ctypes.data_as(N._i32p), len(out), N.f64ptr(out), None)
        assert rc == INVALID and b"scene_fam" in e._lib.dv_last_error(e._ctx)
    finally:
        e.close()


def test_8193_views_in_one_call():
    e = sensor_engine("sq", HL.lands()[0])
    try:
        rng = np.random.default_rng(5)
        n = 8193
        x, y, ang = rng.uniform(40, 260, n), rng.uniform(40, 260, n), rng.uniform(0, 2 * np.pi, n)
        views = e.rviews_set_from_poses(x, y, ang, [0, 4097, n])
        assert np.array_equal(views, e.sense(x, y, ang))
        for k in (0, 4096, 4097, 8192):
            assert np.array_equal(views[k], HL.host_scene("sq", x[k], y[k], ang[k], 0))
        r = e.rviews_step_u8(np.stack([views[8192], views[4096]])[:, None], [1, 0], [0.3, 0.3])
        assert (r.angle_familiarity == 1024).all() and r.angle_view[0, 0] <= 8192 - 4097 and r.angle_view[1, 0] <= 4096
    finally:
        e.close()


# ---- 4. ensembles ------------------------------------------------------------------------------------------------------------------------------
def test_one_ensemble_gives_both_golden_trajectories(manifest, golden):
    """traj_c0 (chem_weight 0) and traj_cw (0.5) share landscape, path, sensor and start: route 0 = route 1 = that path, member 0 on
    route 0 under weight 0, member 1 on route 1 under 0.5."""
    z = golden("t4_trajectory.npz")
    cases = {c["name"]: c for c in manifest["t4_trajectory"]}
    c0, cw = cases["traj_c0"], cases["traj_cw"]
    land = synth.synth_landscape(c0["landscape"]["seed"], c0["landscape"]["size"], c0["landscape"]["grain"])
    assert sha(land) == c0["landscape"]["sha"]
    path = synth.sin_training_path(0.5, 0.2 * c0["landscape"]["size"], 0.6 * c0["landscape"]["size"], arclen=1.0)[:c0["n_views"]]
    assert sha(path) == c0["path_sha"] == cw["path_sha"]
    nsf = navsim_amd.NavBySceneFamiliarity(land, c0["sensor_dimensions"], c0["step_size"], n_test_angles=c0["n_test_angles"],
                                           max_distance_to_training_path=450, familiarity_model=navsim_amd.sads_familiarity(0.25))
    d = path[2] - path[1]
    start = (tuple(path[1] + np.array(c0["start_offset"])), float(np.arctan2(d[1], d[0]) % (2 * np.pi)) + np.deg2rad(c0["start_angle_offset_deg"]))
    ens = navsim_amd.SadsRouteEnsemble.from_routes_with(nsf, [path, path.copy()], [(0,) + start, (1,) + start], metrics="device",
                                                        chem_weights=[0.0, 0.5])
    try:
        assert [a.chem_weight for a in ens.agents] == [0.0, 0.5] and [a.memory_bank for a in ens.agents] == [0, 1]
        assert sha(ens.agents[0].familiar_scenes) == bytes(z["traj_c0_scenes_sha"]).hex()
        rec = [([], [], [], []) for _ in ens.agents]
        for _ in range(c0["n_steps"]):
            ens.step_forward()
            for a, (best, pos, ang, fam) in zip(ens.agents, rec):
                best.append(a.last_best_idex)
                pos.append([a.position[0], a.position[1]])
                ang.append(a.angle)
                fam.append(a.step_familiarity)
        cover = ens.coverage_summary(0.05)
        for i, (a, case, (best, pos, ang, fam)) in enumerate(zip(ens.agents, (c0, cw), rec)):
            name = case["name"]
            assert ens.stop_status == [0, 0]
            assert np.array_equal(np.array(best), z[name + "_best"]), name
            assert np.array(pos).tobytes() == z[name + "_pos"].tobytes() and np.array(ang).tobytes() == z[name + "_angle"].tobytes(), name
            assert np.array_equal(bits(fam), bits(z[name + "_fam"])), name
            assert np.array_equal(bits(a.angle_familiarity), bits(z[name + "_last_angle_fam"])), name
            assert np.array_equal(bits(a.scene_familiarity), bits(z[name + "_last_scene_fam"])), name
            assert a.navigated_for_frames == case["navigated_for_frames"] and float(a.navigation_error) == case["navigation_error"], name
            assert float(cover[i]["path_coverage"]) == case["percent_recapitulated"], name
            assert float(cover[i]["percent_forgiving"]) == case["percent_forgiving"] and int(cover[i]["n_captures"]) == case["n_captures"], name
    finally:
        ens.engine.close()


def make_agent(land, exact=False, **kw):
    return navsim_amd.NavBySceneFamiliarity(np.array(land), HL.ENS_SENSOR, 1.0, n_test_angles=9, use_gpu_sensor=True,
                                            familiarity_model=navsim_amd.sads_familiarity(0.25, exact=exact), **kw)


WEIGHTS = (0.25, 0.0, 1.0, 0.25, 0.5, 0.25, 0.3, 0.25, 0.0, 0.75, 0.25, 1.0)


def lone_agents(landscapes, routes, starts, weights, exact):
    out = []
    for (r, pos, ang), w in zip(starts, weights):
        l, path = routes[r]
        a = navsim_amd.NavBySceneFamiliarity(np.array(landscapes[l]), HL.ENS_SENSOR, 1.0, n_test_angles=9, use_gpu_sensor=True,
                                             familiarity_model=navsim_amd.sads_familiarity(w, exact=exact))
        a.train_from_path(path)
        a.position, a.angle = pos, ang
        out.append(a)
    return out


@pytest.mark.parametrize("metrics", ("host", "device"))
@pytest.mark.parametrize("shapes", ("mixed", "same"))
def test_ensemble_members_equal_lone_agents_on_their_own_landscapes(shapes, metrics):
    landscapes = HL.lands()[:3] if shapes == "mixed" else HL.same_shape_lands()
    routes = HL.ens_routes()
    starts = HL.ens_starts(routes)
    ens = navsim_amd.SadsRouteEnsemble.from_landscapes(make_agent(landscapes[0]), list(landscapes), routes, starts, metrics=metrics,
                                                       chem_weights=WEIGHTS)
    exact = lone_agents(landscapes, routes, starts, WEIGHTS, True)
    plain = lone_agents(landscapes, routes, starts, WEIGHTS, False)
    calls = []
    inner = ens.engine.rviews_sense_step

    def counted(*a, **k):
        calls.append((list(a[3]), list(a[4]), list(k["land_of_member"])))
        return inner(*a, **k)
    ens.engine.rviews_sense_step = counted
    try:
        assert ens._uniform == (shapes == "same")
        assert [a.memory_bank for a in ens.agents] == [r for r, _, _ in starts]
        assert [a.landscape_index for a in ens.agents] == [routes[r][0] for r, _, _ in starts]
        for m, a in zip(ens.agents, exact):
            assert m.landscape is landscapes[m.landscape_index] and m._bounds_tuple() == a._bounds_tuple()
            assert np.array_equal(m.training_path, a.training_path) and m.training_path_length == a.training_path_length
            assert np.array_equal(m.familiar_scenes, a.familiar_scenes)
        with pytest.raises(ValueError, match="SadsRouteEnsemble"):
            ens.agents[1].step_forward()
        with pytest.raises(ValueError, match="NavEnsemble does not take a member of a SadsRouteEnsemble"):
            navsim_amd.NavEnsemble(ens.agents)
        worst = 0.0
        for t in range(15):
            before = list(ens.active)
            ens.step_forward()
            assert len(calls) == t + 1                                                    # ONE device call a step
            assert calls[-1] == ([ens.agents[i].memory_bank for i in before], [WEIGHTS[i] for i in before],
                                 [ens.agents[i].landscape_index for i in before])
            for a in exact + plain:
                if a.stopped_with_exception is None:
                    try:
                        a.step_forward()
                    except navsim_amd.StopNavigationException as stop:
                        a.stopped_with_exception = stop
            for i, (m, a, p) in enumerate(zip(ens.agents, exact, plain)):
                assert m.position == a.position == p.position and m.angle == a.angle == p.angle, (t, i)
                assert np.array_equal(bits(m.angle_familiarity), bits(a.angle_familiarity)), (t, i)
                if not np.isnan(p.angle_familiarity).any():
                    worst = max(worst, float(np.max(np.abs(m.angle_familiarity - p.angle_familiarity) / np.abs(m.angle_familiarity))))
                code = a.stopped_with_exception.get_code() if a.stopped_with_exception is not None else 0
                assert ens.stop_status[i] == code, (t, i)
                assert m.navigation_error == a.navigation_error and m.percent_recapitulated == a.percent_recapitulated, (t, i)
                assert np.array_equal(m._coverage_array, a._coverage_array), (t, i)
            if t in (0, 14):
                rows = ens.scene_familiarity()
                for i, (m, a) in enumerate(zip(ens.agents, exact)):
                    assert np.array_equal(bits(rows[i]), bits(a.scene_familiarity)), (t, i)
                    assert np.array_equal(bits(m.scene_familiarity), bits(a.scene_familiarity)), (t, i)
        print("default-mode lone agents: largest relative difference of angle_familiarity %.3e" % worst)
        assert worst <= 1e-12
    finally:
        ens.engine.rviews_sense_step = inner
        ens.agents[0].clear_training()
        for a in exact + plain:
            a.clear_training()
            a._engine.close()


def _csv(rows):
    out = io.StringIO()
    w = csv.DictWriter(out, fieldnames=sorted(rows[0]))
    w.writeheader()
    w.writerows(rows)
    return out.getvalue()


def test_run_ensemble_rows_equal_lone_run_experiment_rows():
    landscapes = HL.lands()[:3]
    routes = HL.ens_routes()
    starts = HL.ens_starts(routes)
    ens = navsim_amd.SadsRouteEnsemble.from_landscapes(make_agent(landscapes[0]), list(landscapes), routes, starts, metrics="device",
                                                       chem_weights=WEIGHTS)
    try:
        rows = navsim_amd.run_ensemble(ens)
    finally:
        ens.engine.close()
    wants = []
    for a in lone_agents(landscapes, routes, starts, WEIGHTS, True):
        try:
            wants.append(navsim_amd.run_experiment(a))
        finally:
            a.clear_training()
            a._engine.close()
    assert _csv(rows) == _csv(wants)


def test_a_member_past_the_edge_of_its_own_landscape_stops_and_the_others_go_on():
    L = HL.lands()
    landscapes = [L[0], L[1], L[3]]
    HL.ens_facts(L)
    routes = [(l, path) for l, (_, path) in zip((0, 1, 2), HL.ens_routes()[:3])]
    pos, ang = HL.EDGE_START
    HL.footprint_facts()
    starts = [(0, pos, ang), (1, pos, ang), (2, pos, ang), (1, tuple(routes[1][1][3]), 0.8), (1,) + HL.FOOTPRINT_START]
    ens = navsim_amd.SadsRouteEnsemble.from_landscapes(make_agent(L[0]), landscapes, routes, starts)
    try:
        assert not ens._uniform and ens._weights.tolist() == [0.25] * 5
        ens.step_forward()
        assert ens.stop_status == [0, -2, 0, 0, -3]
        assert isinstance(ens.agents[1].stopped_with_exception, navsim_amd.OutOfLandscapeBoundsException)
        assert isinstance(ens.agents[4].stopped_with_exception, IndexError) and ens.agents[4].position == HL.FOOTPRINT_START[0]
        assert np.isinf(ens.agents[4].scene_familiarity).all() and np.isfinite(ens.agents[0].scene_familiarity).all()
        ens.step_forward()
        assert ens.stop_status == [0, -2, 0, 0, -3] and ens.agents[0].position != pos and ens.agents[1].position == pos
    finally:
        ens.engine.close()


# ---- 5. coexistence and refusals ---------------------------------------------------------------------------------------------------------------
def test_the_library_and_a_lone_agent_work_beside_a_live_store_and_after_it_is_cleared():
    L = HL.lands()
    _, path = HL.ens_routes()[0]
    _, pos, ang = HL.ens_starts(HL.ens_routes())[1]
    plain, agent = make_agent(L[0]), make_agent(L[0])
    c = HR.step_case(19, 17, 10, "levels")
    lib, pats = synth.synth_views(3, 300, 32, 32), synth.synth_patches(3, 8, 32, 32)
    other = navsim_amd.FamiliarityEngine(device=0)
    try:
        for a in (plain, agent):
            a.train_from_path(path)
            a.position, a.angle = pos, ang
        eng = agent._engine
        other.set_library(lib, 0.25)
        want = other.step(pats, want_scene=True)
        for stage in range(4):
            if stage == 1:
                eng.rviews_set_u8(c["views"], c["first"])
                other.rviews_set_u8(c["views"][:70], [0, 30, 70])                          # two engines in turn, different stores
            elif stage == 2:
                check_step(eng, c)
                r = other.rviews_step_u8(c["patches"][:2], [1, 0], [0.3, 0.0])
                w0 = oracle.step(c["views"][30:70], c["patches"][0], 0.3)
                assert np.array_equal(bits(r.angle_familiarity[0]), bits(w0["angle_familiarity"]))
                check_step(eng, c)
            elif stage == 3:
                eng.rviews_clear()
                other.rviews_clear()
                assert eng.rviews_info()["n_routes"] == 0 and eng.rviews_info()["bytes"] == 0
            got = other.step(pats, want_scene=True)
            assert got["best_idex"] == want["best_idex"] and np.array_equal(bits(got["angle_familiarity"]), bits(want["angle_familiarity"]))
            assert np.array_equal(bits(got["scene_familiarity"]), bits(want["scene_familiarity"]))
            for t in range(3):
                plain.step_forward()
                agent.step_forward()
                assert agent.position == plain.position and agent.angle == plain.angle, (stage, t)
                assert np.array_equal(bits(agent.angle_familiarity), bits(plain.angle_familiarity)), (stage, t)
        with pytest.raises(N.EngineError, match="no route views"):
            eng.rviews_step_u8(c["patches"], c["routes"], c["weights"])
    finally:
        other.close()
        for a in (plain, agent):
            a.clear_training()
            a._engine.close()


def test_refused_tables_leave_everything_as_it_was(eng):
    c = HR.step_case(19, 17, 10, "levels")
    eng.rviews_set_u8(c["views"], c["first"])
    n, A = c["patches"].shape[:2]
    fam, view, best = np.empty((n, A)), np.empty((n, A), dtype=np.int64), np.empty(n, dtype=np.int32)

    def raw(routes, weights):
        routes, weights = np.array(routes, dtype=np.int32), np.array(weights, dtype=np.float64)
        return eng._lib.dv_rviews_step_u8(eng._ctx, N.u8ptr(c["patches"]), n, A, routes.ctypes.data_as(N._i32p), N.f64ptr(weights), 0,
                                          N.f64ptr(fam), N.i64ptr(view), best.ctypes.data_as(N._i32p))
    bad = c["routes"].copy()
    bad[3] = 6
    assert raw(bad, c["weights"]) == INVALID and b"route_of_member[3] = 6" in eng._lib.dv_last_error(eng._ctx)
    bad[3] = -1
    assert raw(bad, c["weights"]) == INVALID
    w = c["weights"].copy()
    w[5] = 1.5
    assert raw(c["routes"], w) == INVALID and b"chem_weights[5]" in eng._lib.dv_last_error(eng._ctx)
    w[5] = np.nan
    assert raw(c["routes"], w) == INVALID
    first = np.array([0, 5, 6, 9], dtype=np.int64)
    assert eng._lib.dv_rviews_set_u8(eng._ctx, N.u8ptr(c["views"]), N.i64ptr(first), 3, 19, 17) == INVALID
    assert b"first[2] = 6" in eng._lib.dv_last_error(eng._ctx)
    with pytest.raises(N.EngineError, match="lands_set first"):
        eng.rviews_sense_step([50.0] * n, [50.0] * n, np.zeros((n, A)), c["routes"], c["weights"], land_of_member=[0] * n)
    assert np.array_equal(eng.rviews_info()["first"], c["first"])
    check_step(eng, c)
