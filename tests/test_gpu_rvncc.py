"""GPU tests of NCC on the route view store (dv_rvncc_*), the ncc_familiarity plug-in, the lone agent and navsim_amd.NccRouteEnsemble.
Every expected value is the NumPy statement of tests/helpers_rvncc.py (held to np.corrcoef and to its exact values by
tests/test_rvncc_host.py), the host sensor model's views, or a lone agent with an engine and a route of its own.  Doubles are compared
by their bits (np.array_equal on .view(np.int64)): no tolerance anywhere."""
import csv
import io

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import ncc_familiarity, synth
from tests import helpers_lands as HL
from tests import helpers_noise as HZ
from tests import helpers_rvncc as HC
from tests import helpers_sensors as HS

pytestmark = pytest.mark.gpu

INVALID = -1
bits = HC.bits


def same_bits(got, want, what=None):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(bits(got), bits(want)), (what, np.argwhere(bits(got) != bits(want))[:4].tolist())


@pytest.fixture()
def eng():
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


def check_step(e, c, channel=2, scene=True):
    ncc, view, best, rows_want = c["want"][channel] if isinstance(c["want"], dict) else c["want"]
    r = e.rvncc_step_u8(c["patches"], c["routes"], channel)
    same_bits(r.angle_ncc, ncc, ("angle_ncc", channel))
    assert np.array_equal(r.angle_view, view), (channel, np.argwhere(r.angle_view != view)[:4].tolist())
    assert np.array_equal(r.best_idex, best) and not r.flags.any() and r.angle_familiarity is r.angle_ncc, channel
    if scene:
        rows = e.rvncc_scene_u8(c["patches"], c["routes"], channel)
        assert [row.shape for row in rows] == [s.shape for s in rows_want]
        for i, (got, s) in enumerate(zip(rows, rows_want)):
            same_bits(got, s, ("scene", channel, i))
    return r


# ---- 1. uploaded patches against the statement ---------------------------------------------------------------------------------------------------
def test_the_7x5_tail_on_every_channel(eng):
    """P = 35, Pw = 9: the partial last K-step."""
    c = HC.ncc_tail_case(7, 5)
    eng.rviews_set_u8(c["views"], c["first"])
    for channel in (0, 1, 2):
        check_step(eng, c, channel)


@pytest.mark.parametrize("h,w", [(33, 31), (32, 32)])
def test_1023_and_1024_pixels(eng, h, w):
    c = HC.ncc_tail_case(h, w)
    eng.rviews_set_u8(c["views"], c["first"])
    check_step(eng, c, 2)


def test_the_largest_sums_at_64x64_give_exactly_one_and_minus_one(eng):
    c = HC.ncc_extreme_case()
    eng.rviews_set_u8(c["views"], c["first"])
    r = check_step(eng, c)
    assert r.angle_ncc[0].tolist() == [1.0, 1.0, 0.0] and r.angle_view[0].tolist() == [0, 1, 0]
    rows = eng.rvncc_scene_u8(c["patches"][:, :2], c["routes"])
    assert rows[0][:2].tolist() == [-1.0, -1.0]


def test_the_bytes_0_127_128_and_255(eng):
    c = HC.ncc_edge_byte_case()
    eng.rviews_set_u8(c["views"], c["first"])
    check_step(eng, c)


# ---- 2. gain and offset ----------------------------------------------------------------------------------------------------------------------------
def test_a_view_under_a_gain_and_an_offset_is_found_with_exactly_one_where_ssd_reports_another(eng):
    c = HC.gain_case()
    eng.rviews_set_u8(c["views"], c["first"])
    r = check_step(eng, c)
    assert r.angle_ncc[0, 0] == 1.0 and r.angle_view[0, 0] == HC.GAIN_K
    ssd = eng.rvssd_step_u8(c["patches"], c["routes"])
    assert ssd.angle_view[0, 0] != HC.GAIN_K and ssd.angle_view[0, 0] == HC.ssd_first_min(c["views"], c["patches"][0], 2)[0]


# ---- 3. degenerates --------------------------------------------------------------------------------------------------------------------------------
def test_constant_planes_correlate_with_nothing(eng):
    c = HC.constant_case()
    eng.rviews_set_u8(c["views"], c["first"])
    r = check_step(eng, c)
    assert r.angle_ncc[0].tolist() == [0.0, 0.0] and r.angle_view[0].tolist() == [0, 4] and r.best_idex[0] == 0
    row = eng.rvncc_scene_u8(c["patches"][:, :1], c["routes"])[0]                          # the constant patch alone: a row of 0.0
    assert row.tolist() == [0.0] * 6 and not np.signbit(row).any()


def test_padding_views_do_not_win_where_every_view_correlates_negatively(eng):
    c = HC.negative_case()
    eng.rviews_set_u8(c["views"], c["first"])
    r = check_step(eng, c)
    assert r.angle_ncc[0, 0] < 0.0 and r.angle_view[0, 0] < 65


# ---- 4. geometry -----------------------------------------------------------------------------------------------------------------------------------
def test_routes_of_2_to_300_views_with_the_members_in_shuffled_route_order(eng):
    """2, 33, 64, 65, 130 and 300 views (300: a second block of four view groups); every route's best view is its LAST."""
    c = HC.ncc_lengths_case()
    eng.rviews_set_u8(c["views"], c["first"])
    r = check_step(eng, c)
    lens = np.array(HC.NCC_LENGTHS)[c["routes"]]
    assert np.array_equal(r.angle_view[:, 0], lens - 1) and (r.angle_ncc[:, 0] == 1.0).all() and (r.angle_view < lens[:, None]).all()


@pytest.mark.parametrize("n,A", [(7, 10), (1, 33), (2, 70), (1, 1)])
def test_column_geometry(eng, n, A):
    """7 x 10: tiles cut members; 33 and 70 headings: a member in several tiles; one member x one heading."""
    c = HC.members_case(n, A)
    eng.rviews_set_u8(c["views"], c["first"])
    check_step(eng, c)


def test_a_member_alone_and_among_seven_gives_identical_rows(eng):
    c = HC.members_case(7, 10)
    eng.rviews_set_u8(c["views"], c["first"])
    many = eng.rvncc_step_u8(c["patches"], c["routes"])
    alone = eng.rvncc_step_u8(c["patches"][3:4], c["routes"][3:4])
    same_bits(alone.angle_ncc[0], many.angle_ncc[3])
    assert np.array_equal(alone.angle_view[0], many.angle_view[3]) and alone.best_idex[0] == many.best_idex[3]
    same_bits(eng.rvncc_scene_u8(c["patches"][3:4], c["routes"][3:4])[0], eng.rvncc_scene_u8(c["patches"], c["routes"])[3])


# ---- 5. ties ---------------------------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_least_view_and_the_first_heading(eng):
    """One view at indices 5 and 290 of a route (other groups, other blocks); headings 1 and 2 are equal."""
    c = HC.ncc_tie_case()
    eng.rviews_set_u8(c["views"], c["first"])
    r = check_step(eng, c)
    assert r.angle_ncc[0].tolist()[1:] == [1.0, 1.0] and r.angle_view[0].tolist()[1:] == [5, 5] and r.best_idex[0] == 1


# ---- 6. launch edge --------------------------------------------------------------------------------------------------------------------------------
def test_32769_members_on_one_route(eng):
    c = HC.many_members_case()
    eng.rviews_set_u8(c["views"], c["first"])
    r = check_step(eng, c, scene=False)
    assert r.angle_ncc.shape == (32769, 1)
    rows = eng.rvncc_scene_u8(c["patches"][-40:], c["routes"][-40:])
    same_bits(np.stack(rows), c["want"][3][-40:])


def test_32769_tiles_the_last_in_a_launch_of_its_own(eng):
    c = HC.launch_edge_case()
    eng.rviews_set_u8(c["views"], c["first"])
    r = check_step(eng, c, scene=False)
    assert r.angle_ncc.shape == (32769, 1)
    rows = eng.rvncc_scene_u8(c["patches"], c["routes"])
    same_bits(np.stack(rows), c["want"][3])


# ---- 7. sensed calls -------------------------------------------------------------------------------------------------------------------------------
def same_as_twin(e, xs, ys, angs, routes, patches, channel, views, first, lands=None):
    want = HC.expected(views, first, patches, routes, channel)
    u8 = e.rvncc_step_u8(patches, routes, channel)
    s = e.rvncc_sense_step(xs, ys, angs, routes, channel, land_of_member=lands)
    for r in (u8, s):
        same_bits(r.angle_ncc, want[0], channel)
        assert np.array_equal(r.angle_view, want[1]) and np.array_equal(r.best_idex, want[2]) and not r.flags.any()
    rows, flags = e.rvncc_scene(xs, ys, angs, routes, channel, land_of_member=lands, want_flags=True)
    twin = e.rvncc_scene_u8(patches, routes, channel)
    assert not flags.any()
    for got, t, w in zip(rows, twin, want[3]):
        same_bits(got, w, channel)
        same_bits(t, w, channel)


def test_sensed_calls_on_the_engines_landscape_equal_the_u8_calls_on_the_host_models_views():
    name = "sq"
    t = HL.train_case(name)
    order = np.concatenate(t["first"])
    on0 = order[t["land_of"][order] == 0]                                                 # the route on landscape 0, and once more reversed
    x, y, ang = np.concatenate([t["x"][on0], t["x"][on0][::-1]]), np.concatenate([t["y"][on0], t["y"][on0][::-1]]), \
        np.concatenate([t["angle"][on0], t["angle"][on0][::-1] + 0.1])
    first = HC.first_of([len(on0), len(on0)])
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
            same_as_twin(e, xs, ys, angs, routes, patches, channel, views, first)
    finally:
        e.close()


def test_sensed_calls_on_a_landscape_set_under_a_sensor_table_with_a_member_off_its_landscape():
    """Two landscapes of different shapes (L0 300 x 300 under E0, L1 211 x 173 under E1), 16 x 8 views; member 2 is on L1 at a place
    that only L0 has: flagged 16 with best_idex -1, its scene row +inf, the others untouched."""
    shape, pairs = "wide", ((0, "E0"), (1, "E1"))
    rng = np.random.default_rng(5)
    n_r = (9, 6)
    x, y, ang = rng.uniform(50, 120, 15), rng.uniform(50, 120, 15), rng.uniform(0, 2 * np.pi, 15)
    land_of_view = np.repeat([0, 1], n_r).astype(np.int32)
    first = HC.first_of(n_r)
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
            want = HC.expected(views, first, patches, [routes[i] for i in keep], channel)
            s = e.rvncc_sense_step(xs, ys, angs, routes, channel, land_of_member=lands)
            assert s.flags.tolist() == [0, 0, HL.SENSE_ERROR, 0] and s.best_idex[2] == -1
            same_bits(s.angle_ncc[keep], want[0], channel)
            assert np.array_equal(s.angle_view[keep], want[1]) and np.array_equal(s.best_idex[keep], want[2])
            rows, flags = e.rvncc_scene(xs, ys, angs, routes, channel, land_of_member=lands, want_flags=True)
            assert flags.tolist() == [0, 0, HL.SENSE_ERROR, 0] and rows[2].shape == (6,) and (rows[2] == np.inf).all()
            for i, w in zip(keep, want[3]):
                same_bits(rows[i], w, (channel, i))
    finally:
        e.close()


def test_sensed_calls_under_noise_rows_equal_their_uploaded_twins():
    """helpers_noise.store_case: two routes sensed under training rows, three members on two landscapes under rows of their own."""
    s = HZ.store_case()
    e = navsim_amd.FamiliarityEngine(device=0)
    try:
        e.set_landscape(HZ.lands()[0])
        e.configure_sensor(HZ.THIN["sensor"], HZ.THIN["pixel"], HZ.level_table(HZ.THIN), HZ.THIN["mask"])
        e.lands_set(list(HZ.lands()))
        e.noise_rows(HZ.SEED, s["tkeys"], s["tamp_s"], s["tamp_v"])
        views = e.rviews_set_from_poses(s["x"], s["y"], s["angle"], s["first"], land_of_view=s["land_of_view"])
        assert np.array_equal(views, s["views"])
        e.noise_rows(HZ.SEED, s["keys"], s["amp_s"], s["amp_v"])
        for channel in (1, 2):
            same_as_twin(e, s["xs"], s["ys"], s["angs"], s["routes"], s["patches"], channel, s["views"], s["first"], lands=s["lands"])
        quiet = HZ.member_views(HZ.THIN, s["xs"], s["ys"], s["angs"], s["lands"], HZ.SEED, s["keys"], [0] * 3, [0] * 3)
        assert not np.array_equal(e.rvncc_step_u8(quiet, s["routes"], 2).angle_ncc, e.rvncc_step_u8(s["patches"], s["routes"], 2).angle_ncc)
    finally:
        e.close()


# ---- 8. scene calls --------------------------------------------------------------------------------------------------------------------------------
def test_scene_rows_are_ragged_and_a_wrong_length_is_refused_by_name(eng):
    c = HC.members_case(2, 70)                                                            # 70 headings: a member's columns in three tiles
    eng.rviews_set_u8(c["views"], c["first"])
    rows = eng.rvncc_scene_u8(c["patches"], c["routes"])
    assert [len(r) for r in rows] == [HC.GEOMETRY_LENGTHS[r] for r in c["routes"]]
    for i, row in enumerate(rows):
        lib = c["views"][c["first"][c["routes"][i]]:c["first"][c["routes"][i] + 1]]
        same_bits(row, HC.ncc_rows(lib, c["patches"][i], 2).min(axis=0), i)
    n, A = c["patches"].shape[:2]
    out = np.empty(int(sum(len(r) for r in rows)) + 1)
    routes = np.ascontiguousarray(c["routes"])
    rc = eng._lib.dv_rvncc_scene_u8(eng._ctx, N.u8ptr(c["patches"]), n, A, routes.ctypes.data_as(N._i32p), 2, len(out), N.f64ptr(out))
    assert rc == INVALID and b"scene_ncc" in eng._lib.dv_last_error(eng._ctx)
    rc = eng._lib.dv_rvncc_scene_u8(eng._ctx, N.u8ptr(c["patches"]), n, A, routes.ctypes.data_as(N._i32p), 3, len(out) - 1, N.f64ptr(out))
    assert rc == INVALID and b"channel 3" in eng._lib.dv_last_error(eng._ctx)


# ---- 9. caches -------------------------------------------------------------------------------------------------------------------------------------
def test_the_ssd_calls_are_untouched_by_an_ncc_call_between_them(eng):
    c = HC.ncc_tail_case(7, 5)
    eng.rviews_set_u8(c["views"], c["first"])
    before = eng.rvssd_step_u8(c["patches"], c["routes"], 1)
    scene_before = eng.rvssd_scene_u8(c["patches"], c["routes"], 1)
    check_step(eng, c, 1)
    after = eng.rvssd_step_u8(c["patches"], c["routes"], 1)
    scene_after = eng.rvssd_scene_u8(c["patches"], c["routes"], 1)
    assert np.array_equal(after.angle_ssd, before.angle_ssd) and np.array_equal(after.angle_view, before.angle_view)
    assert np.array_equal(after.best_idex, before.best_idex) and all(np.array_equal(a, b) for a, b in zip(scene_after, scene_before))
    from tests import helpers_rvssd as HV
    assert np.array_equal(after.angle_ssd, HV.tail_case(7, 5)["want"][1][0])


def test_the_view_statistics_follow_the_store_and_the_channel(eng):
    c = HC.ncc_tail_case(7, 5)
    other = dict(c, views=HC.planes_u8(77, c["views"].shape))                             # other views of the same shape and routes
    other["want"] = {ch: HC.expected(other["views"], c["first"], c["patches"], c["routes"], ch) for ch in (0, 2)}
    assert not np.array_equal(other["want"][2][0], c["want"][2][0])
    eng.rviews_set_u8(c["views"], c["first"])
    for channel in (2, 0, 2):                                                             # two channels in turn on one store
        check_step(eng, c, channel)
    eng.rviews_set_u8(other["views"], c["first"])                                         # replaced: a stale statistic would give other numbers
    for channel in (2, 0):
        check_step(eng, other, channel)
    eng.rviews_clear()
    eng.rviews_set_u8(c["views"], c["first"])
    for channel in (0, 2):
        check_step(eng, c, channel)


# ---- 10. the plug-in and the lone agent ------------------------------------------------------------------------------------------------------------
def test_model_and_func_against_the_statement():
    c = HC.ncc_tail_case(7, 5)
    scenes = c["views"][5:]                                                                # 70 views
    for channel in (0, 2):
        func = ncc_familiarity(channel)(scenes)
        try:
            assert func.max_familiarity == 1.0 and func.metric == "ncc" and func.channel == channel
            for scene in (c["patches"][0, 1], c["patches"][1, 0], np.full((7, 5, 3), 9, dtype=np.uint8)):
                fambuf = np.full(70, np.nan)
                func(scene, fambuf)
                same_bits(fambuf, HC.ncc_rows(scenes, scene[None], channel)[0], channel)
        finally:
            func.engine.close()


AGENT_SENSOR, AGENT_ANGLES, AGENT_STEPS = (16, 8), 9, 40


def agent_route():
    return synth.sin_training_path(0.2, 60, 180, arclen=1.0)[:60]


def make_agent(land, gpu=True, angles=AGENT_ANGLES, **kw):
    return navsim_amd.NavBySceneFamiliarity(np.array(land), AGENT_SENSOR, 1.0, n_test_angles=angles, use_gpu_sensor=gpu,
                                            familiarity_model=ncc_familiarity(2), **kw)


@pytest.mark.parametrize("lazy", (True, False))
def test_a_40_step_trajectory_of_the_lone_agent_equals_the_numpy_shadow(lazy):
    land, route = HL.lands()[0], agent_route()
    a, host = make_agent(land), make_agent(land, gpu=False)
    a.lazy_scene = lazy
    try:
        a.train_from_path(route)
        hd = HL.route_headings(route)
        views = np.stack([host.get_sensor_mat(route[v], hd[v]) for v in range(len(route))])
        assert np.array_equal(a.familiar_scenes, views)
        pos, ang = (float(route[3][0] + 0.4), float(route[3][1] - 0.3)), float(hd[3] + 0.2)
        a.position, a.angle = pos, ang
        for t in range(AGENT_STEPS):
            angles = (ang + a.angle_offsets) % (2 * np.pi)
            patches = np.stack([host.get_sensor_mat(pos, x) for x in angles])
            rows = HC.ncc_rows(views, patches, 2)
            fam = rows.max(axis=1)
            best = int(np.argmax(fam))
            ang = angles[best]
            pos = (pos[0] + 1.0 * np.cos(ang), pos[1] + 1.0 * np.sin(ang))
            a.step_forward()
            assert a.position == pos and a.angle == ang, t
            same_bits(a.angle_familiarity, fam, t)
            if lazy or t % 7 == 0:
                same_bits(a.scene_familiarity, rows.min(axis=0), t)
        assert a.navigated_for_frames == AGENT_STEPS
    finally:
        a.clear_training()
        a._engine.close()


def test_the_agent_with_the_host_sensor_model_goes_through_func_and_an_additional_path_ingests_everything_again():
    land, route = HL.lands()[0], agent_route()
    a, host, g = make_agent(land, gpu=False, angles=5), make_agent(land, gpu=False, angles=5), make_agent(land, angles=5)
    try:
        first, more = route[:20], route[25:40]
        for x in (a, g):
            x.train_from_path(first)
            x.train_additional_path(more)
            x.position, x.angle = (float(route[30][0]), float(route[30][1] + 0.5)), float(HL.route_headings(route)[30])
        views = np.stack([host.get_sensor_mat(p, h) for pts in (first, more) for p, h in zip(pts, HL.route_headings(pts))])
        assert np.array_equal(a.familiar_scenes, views) and np.array_equal(g.familiar_scenes, views)
        angles = (a.angle + a.angle_offsets) % (2 * np.pi)
        rows = HC.ncc_rows(views, np.stack([host.get_sensor_mat(a.position, x) for x in angles]), 2)
        assert rows[int(np.argmax(rows.max(axis=1)))].argmax() >= 20                        # the match lies on the added path
        for x in (a, g):
            x.step_forward(fake=True)
            same_bits(x.angle_familiarity, rows.max(axis=1))
            same_bits(x.scene_familiarity, rows.min(axis=0))
    finally:
        a._familiarity_func.engine.close()
        g._engine.close()


# ---- 11. the ensemble ------------------------------------------------------------------------------------------------------------------------------
def ens_setup():
    landscapes = HL.lands()[:2]
    routes = HL.ens_routes()[:4]                                                           # two routes on each of two landscapes
    assert [l for l, _ in routes] == [0, 0, 1, 1]
    starts = HL.ens_starts(routes)
    assert len(starts) == 8
    return landscapes, routes, starts


def lone_agents(landscapes, routes, starts):
    out = []
    for r, pos, ang in starts:
        l, path = routes[r]
        a = make_agent(landscapes[l], angles=10)
        a.train_from_path(path)
        a.position, a.angle = pos, ang
        out.append(a)
    return out


def _csv(rows):
    out = io.StringIO()
    w = csv.DictWriter(out, fieldnames=sorted(rows[0]))
    w.writeheader()
    w.writerows(rows)
    return out.getvalue()


@pytest.fixture(scope="module")
def lone_rows():
    landscapes, routes, starts = ens_setup()
    wants = []
    for a in lone_agents(landscapes, routes, starts):
        try:
            wants.append(navsim_amd.run_experiment(a))
        finally:
            a.clear_training()
            a._engine.close()
    return wants


@pytest.mark.parametrize("metrics", ("host", "device"))
def test_run_ensemble_rows_equal_lone_agents_rows(metrics, lone_rows):
    landscapes, routes, starts = ens_setup()
    ens = navsim_amd.NccRouteEnsemble.from_landscapes(make_agent(landscapes[0], angles=10), list(landscapes), routes, starts, metrics=metrics)
    try:
        assert ens.channel == 2 and [a.memory_bank for a in ens.agents] == [r for r, _, _ in starts]
        assert [a.landscape_index for a in ens.agents] == [routes[r][0] for r, _, _ in starts]
        with pytest.raises(ValueError, match="NccRouteEnsemble"):
            ens.agents[1].step_forward()
        rows = navsim_amd.run_ensemble(ens)
    finally:
        ens.engine.close()
    assert _csv(rows) == _csv(lone_rows)
    assert any(r["stop_status"] == 1 for r in rows)                                       # members reached the end of their route


def test_ensemble_steps_and_scene_familiarity_equal_lone_agents():
    landscapes, routes, starts = ens_setup()
    ens = navsim_amd.NccRouteEnsemble.from_routes_with(make_agent(landscapes[0], angles=10), [p for _, p in routes[:2]], starts[:4], metrics="device")
    lone = lone_agents(landscapes, routes, starts[:4])
    try:
        for m, a in zip(ens.agents, lone):
            assert np.array_equal(m.familiar_scenes, a.familiar_scenes) and m.training_path_length == a.training_path_length
        for t in range(4):
            ens.step_forward()
            for a in lone:
                a.step_forward()
            rows = ens.scene_familiarity() if t in (0, 3) else None
            for i, (m, a) in enumerate(zip(ens.agents, lone)):
                assert m.position == a.position and m.angle == a.angle, (t, i)
                same_bits(m.angle_familiarity, a.angle_familiarity, (t, i))
                assert m.navigation_error == a.navigation_error, (t, i)
                if rows is not None:
                    same_bits(rows[i], a.scene_familiarity, (t, i))
        cover = ens.coverage_summary(0.05)
        assert [float(c["path_coverage"]) for c in cover] == [a.percent_recapitulated for a in lone]
    finally:
        ens.engine.close()
        for a in lone:
            a.clear_training()
            a._engine.close()


def noise_build(members=None):
    c, noise, starts = HZ.ENS, HZ.ENS_NOISE, HZ.ens_starts()
    if members is not None:
        noise = dict(noise, amp_v=[noise["amp_v"][i] for i in members], streams=[noise["streams"][i] for i in members])
        starts = [starts[i] for i in members]
    agent = navsim_amd.NavBySceneFamiliarity(np.array(HZ.lands()[0]), c["sensor"], HZ.ENS_STEP, n_test_angles=HZ.ENS_ANGLES, use_gpu_sensor=True,
                                             n_sensor_levels=c["levels"], familiarity_model=ncc_familiarity(2))
    return navsim_amd.NccRouteEnsemble.from_landscapes(agent, list(HZ.lands()), HZ.ens_routes(), starts, noise=noise)


def test_under_noise_a_members_rows_are_those_of_a_one_member_ensemble_with_its_stream():
    ens = noise_build()
    ones = []
    try:
        for a, want in zip(ens.agents, [HZ.ens_train_views()[r] for r, _, _ in HZ.ens_starts()]):
            assert np.array_equal(a.familiar_scenes, want)                                # training under the routes' own keys
        ens.step_forward()
        first = [(a.angle_familiarity.copy(), tuple(a.position), float(a.angle)) for a in ens.agents]
        assert not np.array_equal(first[0][0], first[1][0])                               # one pose, two streams
        shadow = HZ.shadow(0, 1)[0]                                                       # the statement's patches of member 0's first step
        memory = HZ.ens_train_views()[0]
        same_bits(first[0][0], HC.ncc_rows(memory, shadow["patches"], 2).max(axis=1))
        scene = ens.scene_familiarity()
        same_bits(scene[0], HC.ncc_rows(memory, shadow["patches"], 2).min(axis=0))
        trace = [first]
        for _ in range(4):
            ens.step_forward()
            trace.append([(a.angle_familiarity.copy(), tuple(a.position), float(a.angle)) for a in ens.agents])
        for i in range(4):
            one = noise_build([i])
            ones.append(one)
            for t in range(5):
                one.step_forward()
                m = one.agents[0]
                same_bits(m.angle_familiarity, trace[t][i][0], (i, t))
                assert tuple(m.position) == trace[t][i][1] and float(m.angle) == trace[t][i][2], (i, t)
                if t == 0:
                    same_bits(one.scene_familiarity()[0], scene[i], i)
            assert one.stop_status[0] == ens.stop_status[i]
    finally:
        ens.engine.close()
        for one in ones:
            one.engine.close()
