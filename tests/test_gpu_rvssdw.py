"""GPU tests of windowed SSD on the route view store (dv_rvssdw_*) and of the windows of navsim_amd.SsdRouteEnsemble.  Every expected
value is the NumPy int64 statement of tests/helpers_rvssd.py on the slice of the member's route (tests/helpers_rvssdw.py), the
unwindowed call on the same patches, the host sensor model's views, or a shadow agent whose plug-in computes -SSD on the slice in NumPy.
Every comparison is np.array_equal on integers or on the doubles that hold them: no tolerance anywhere."""
import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import ssd_familiarity
from tests import helpers_lands as HL
from tests import helpers_rvssd as HV
from tests import helpers_rvssdw as H
from tests import helpers_sensors as HS

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -3
E = navsim_amd.SsdRouteEnsemble


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture()
def eng():
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


def lo_hi(windows):
    return [w[0] for w in windows], [w[1] for w in windows]


def same(r, want, flags=None):
    ssd, view, best = want[:3]
    assert np.array_equal(r.angle_ssd, ssd), np.argwhere(r.angle_ssd != ssd)[:4].tolist()
    assert np.array_equal(r.angle_view, view), np.argwhere(r.angle_view != view)[:4].tolist()
    assert np.array_equal(r.best_idex, best)
    assert np.array_equal(bits(r.angle_familiarity), bits(np.negative(ssd)))
    assert np.array_equal(r.flags, np.zeros(len(best), dtype=np.uint32) if flags is None else np.asarray(flags, dtype=np.uint32)), r.flags


def check_windowed(e, c, channel=2):
    e.rviews_set_u8(c["views"], c["first"])
    r = e.rvssdw_step_u8(c["patches"], c["routes"], *lo_hi(c["windows"]), channel=channel)
    same(r, c["want"])
    lo, hi = np.array(lo_hi(c["windows"]))
    assert (r.angle_view >= lo[:, None]).all() and (r.angle_view < hi[:, None]).all()
    return r


# ---- 1. window edges, planted matches -----------------------------------------------------------------------------------------------------------
def test_window_edges_nine_groups_and_the_routes_padding(eng):
    """[0,1), [63,65), [64,128), [63,575) (512 views over nine groups: wave 0 makes three trips) and a window that ends with a route of
    130 views, where a padding view would win the all-zero patch if it were not masked."""
    r = check_windowed(eng, H.edges_case())
    assert r.angle_view[0].tolist() == [0, 0] and (r.angle_ssd > 0).all()


def test_planted_matches_just_outside_the_window_never_win(eng):
    r = check_windowed(eng, H.planted_case())
    assert r.angle_ssd[0, 1] > 0 and 70 <= r.angle_view[0, 1] < 130


# ---- 2. pixel tails, byte range -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channel", (0, 1, 2))
def test_the_partial_last_k_step_on_every_channel(eng, channel):
    check_windowed(eng, H.tail_case(channel), channel)


def test_k_steps_issued_together_then_one_at_a_time_then_the_partial_one(eng):
    check_windowed(eng, H.ahead_case())


def test_sign_edges_of_the_bias_trick(eng):
    check_windowed(eng, H.edge_byte_case())


def test_the_largest_value_at_64x64(eng):
    r = check_windowed(eng, H.extreme_case())
    assert r.angle_ssd[0, 0] == 266342400.0 and r.angle_view[0, 0] == 1


# ---- 3. ties ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second", (40, 70))
@pytest.mark.parametrize("which", (0, 1, 2))
def test_ties_inside_the_window_go_to_the_least_view_and_the_first_heading(eng, second, which):
    r = check_windowed(eng, H.tie_case(second, which))
    if which < 2:
        assert r.angle_view[0].tolist()[1:] == [(5, second)[which]] * 2 and r.best_idex[0] == 1 and np.signbit(r.angle_familiarity[0, 1])


# ---- 4. tiles, members, the whole route, the launch bound -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", H.TILE_HEADINGS)
def test_heading_tiles_and_three_windows_on_one_route(eng, A):
    check_windowed(eng, H.tiles_case(A))


def test_whole_route_windows_equal_the_unwindowed_call_bit_for_bit(eng):
    c = HV.geometry_case("many")
    eng.rviews_set_u8(c["views"], c["first"])
    lens = np.diff(c["first"])[c["routes"]]
    assert lens.max() <= H.MAX_VIEWS
    whole = eng.rvssd_step_u8(c["patches"], c["routes"])
    r = eng.rvssdw_step_u8(c["patches"], c["routes"], np.zeros(len(lens), dtype=np.int64), lens)
    same(whole, c["want"])
    same(r, (whole.angle_ssd, whole.angle_view, whole.best_idex))
    again = eng.rvssd_step_u8(c["patches"], c["routes"])                                  # the two calls leave each other alone
    same(again, c["want"])


def test_one_member_more_than_a_launch_takes(eng):
    c = H.bound_case()
    r = check_windowed(eng, c)
    assert len(r.best_idex) == H.MEMBERS_PER_LAUNCH + 1 and 64 <= r.angle_view[-1, 0] < 70


# ---- 5. sensed calls ----------------------------------------------------------------------------------------------------------------------------------
def test_sensed_windowed_calls_on_one_landscape_equal_the_u8_call_on_the_host_models_views():
    name = "sq"
    t = HL.train_case(name)
    order = np.concatenate(t["first"])
    on0 = order[t["land_of"][order] == 0]
    x, y, ang = np.concatenate([t["x"][on0], t["x"][on0][::-1]]), np.concatenate([t["y"][on0], t["y"][on0][::-1]]), \
        np.concatenate([t["angle"][on0], t["angle"][on0][::-1] + 0.1])
    first = HV.first_of([len(on0), len(on0)])
    c = HL.SENSORS[name]
    e = navsim_amd.FamiliarityEngine(device=0)
    try:
        e.set_landscape(HL.lands()[0])
        e.configure_sensor(c["sensor"], c["pixel"], HL.level_tables(name), c["mask"])
        views = e.rviews_set_from_poses(x, y, ang, first)
        xs, ys = np.array([x[2], x[4] + 0.5, x[1]]), np.array([y[2], y[4] - 0.5, y[1] + 1.0])
        angs = (np.array([ang[2], ang[4], ang[1]])[:, None] + np.array([-0.3, 0.0, 0.2, 0.5])[None, :]) % (2 * np.pi)
        routes = [1, 0, 1]
        windows = [(1, len(on0)), (0, 2), (len(on0) - 1, len(on0))]
        patches = np.stack([HL.host_scenes(name, [xs[i]] * 4, [ys[i]] * 4, angs[i], [0] * 4) for i in range(3)])
        for channel in (2, 0):
            want = H.window_expected(views, first, patches, routes, windows, channel)
            u8 = e.rvssdw_step_u8(patches, routes, *lo_hi(windows), channel=channel)
            s = e.rvssdw_sense_step(xs, ys, angs, routes, *lo_hi(windows), channel=channel)
            same(u8, want)
            same(s, want)
    finally:
        e.close()


def test_sensed_windowed_calls_on_a_landscape_set_with_a_sensor_table_and_a_member_off_its_landscape():
    """Two landscapes of different shapes under a sensor entry each; member 2 is on L1 at a place that only L0 has: flagged 16 with
    best_idex -1 and never lost, whatever its threshold; the others are scored, member 3 re-localised."""
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
        xs, ys = np.array([x[1] + 0.4, x[10], HL.ON_L2_OFF_L1[0], x[12] - 0.3]), np.array([y[1], y[10] + 0.6, HL.ON_L2_OFF_L1[1], y[12]])
        angs = (np.array([ang[1], ang[10], 0.3, ang[12]])[:, None] + np.array([0.0, 0.25, -0.25])[None, :]) % (2 * np.pi)
        routes, lands = [0, 1, 1, 1], [0, 1, 1, 1]
        windows = [(2, 9), (0, 3), (1, 4), (4, 6)]
        assert all(HS.is_off(shape, "E1", xs[2], ys[2], a, 1) for a in angs[2])
        keep = [0, 1, 3]
        patches = np.stack([np.stack([HS.host_scene(shape, pairs[lands[i]][1], xs[i], ys[i], a, pairs[lands[i]][0]) for a in angs[i]]) for i in keep])
        for channel in (2, 1):
            want = H.window_expected(views, first, patches, [routes[i] for i in keep], [windows[i] for i in keep], channel)
            u8 = e.rvssdw_step_u8(patches, [routes[i] for i in keep], *lo_hi([windows[i] for i in keep]), channel=channel)
            same(u8, want)
            s = e.rvssdw_sense_step(xs, ys, angs, routes, *lo_hi(windows), channel=channel, land_of_member=lands)
            assert s.flags.tolist() == [0, 0, HL.SENSE_ERROR, 0] and s.best_idex[2] == -1
            assert np.array_equal(s.angle_ssd[keep], want[0]) and np.array_equal(s.angle_view[keep], want[1])
            assert np.array_equal(s.best_idex[keep], want[2])
            whole = HV.expected(views, first, patches, [routes[i] for i in keep], channel)
            taus = [-np.inf, H.stay(want[0][1]), np.inf, np.inf]
            t = e.rvssdw_sense_step(xs, ys, angs, routes, *lo_hi(windows), channel=channel, land_of_member=lands, reloc_below=taus)
            assert t.flags.tolist() == [0, 0, HL.SENSE_ERROR, H.RELOCALISED] and t.best_idex[2] == -1
            assert t.relocalised.tolist() == [False, False, False, True]
            assert np.array_equal(t.angle_ssd[[0, 1]], want[0][:2]) and np.array_equal(t.angle_view[[0, 1]], want[1][:2])
            assert np.array_equal(t.angle_ssd[3], whole[0][2]) and np.array_equal(t.angle_view[3], whole[1][2]) and t.best_idex[3] == whole[2][2]
    finally:
        e.close()


# ---- 6. re-localisation -----------------------------------------------------------------------------------------------------------------------------
def check_rule(e, c, taus, want):
    """The call with thresholds against (ssd, view, best, lost); the lost rows against the unwindowed call itself, the others against
    the call without thresholds."""
    ssd, view, best, lost = want
    r = e.rvssdw_step_u8(c["patches"], c["routes"], *lo_hi(c["windows"]), reloc_below=taus)
    same(r, (ssd, view, best), np.where(lost, H.RELOCALISED, 0))
    assert np.array_equal(r.relocalised, lost)
    whole = e.rvssd_step_u8(c["patches"], c["routes"])
    plain = e.rvssdw_step_u8(c["patches"], c["routes"], *lo_hi(c["windows"]))
    for i, gone in enumerate(lost):
        src = whole if gone else plain
        assert np.array_equal(bits(r.angle_ssd[i]), bits(src.angle_ssd[i])) and np.array_equal(r.angle_view[i], src.angle_view[i]), i
        assert r.best_idex[i] == src.best_idex[i], i
    return r


@pytest.mark.parametrize("A", H.TILE_HEADINGS)
def test_the_strict_rule_on_lost_members_of_several_routes(eng, A):
    """Thresholds exactly -min ssd (kept: the < is strict), the next double above (lost), -inf and +inf; the lost members lie on routes
    3, 1 and 3.  At 33 headings the two lost members of route 3 are 66 columns: a plan tile spans both."""
    c = H.tiles_case(A)
    eng.rviews_set_u8(c["views"], c["first"])
    taus, want = H.mixed_thresholds(c)
    check_rule(eng, c, taus, want)


def test_nobody_lost_and_everybody_lost(eng):
    c = H.tiles_case(33)
    eng.rviews_set_u8(c["views"], c["first"])
    n = len(c["routes"])
    none = check_rule(eng, c, np.full(n, -np.inf), H.apply_rule(c["want"], c["whole"], np.full(n, -np.inf)))
    assert not none.flags.any()
    every = check_rule(eng, c, np.full(n, np.inf), H.apply_rule(c["want"], c["whole"], np.full(n, np.inf)))
    assert every.flags.tolist() == [H.RELOCALISED] * n
    kept = check_rule(eng, c, [H.stay(row) for row in c["want"][0]], c["want"] + (np.zeros(n, dtype=bool),))
    assert not kept.flags.any()


def test_refused_calls_change_nothing(eng):
    c = H.tiles_case(33)
    n, A = c["patches"].shape[:2]
    ssd, view, best, flags = np.empty((n, A)), np.empty((n, A), dtype=np.int64), np.empty(n, dtype=np.int32), np.zeros(n, dtype=np.uint32)

    def raw(routes, windows, taus, channel):
        routes, (lo, hi) = np.array(routes, dtype=np.int32), [np.array(w, dtype=np.int32) for w in lo_hi(windows)]
        tau = None if taus is None else np.array(taus, dtype=np.float64)
        return eng._lib.dv_rvssdw_step_u8(eng._ctx, N.u8ptr(c["patches"]), n, A, routes.ctypes.data_as(N._i32p), lo.ctypes.data_as(N._i32p),
                                          hi.ctypes.data_as(N._i32p), None if tau is None else N.f64ptr(tau), channel, N.f64ptr(ssd),
                                          N.i64ptr(view), best.ctypes.data_as(N._i32p), flags.ctypes.data_as(N._u32p))
    assert raw(c["routes"], c["windows"], None, 2) == STATE
    eng.rviews_set_u8(c["views"], c["first"])
    before = eng.rvssdw_step_u8(c["patches"], c["routes"], *lo_hi(c["windows"]))
    bad = list(c["windows"])
    bad[2] = (0, 130)
    assert raw(c["routes"], bad, None, 2) == INVALID
    assert b"member 2: window [0, 130) must hold 1 to 512 views within its route 3 of 129 views" in eng._lib.dv_last_error(eng._ctx)
    bad[2] = (5, 5)
    assert raw(c["routes"], bad, None, 2) == INVALID and b"member 2: window [5, 5)" in eng._lib.dv_last_error(eng._ctx)
    assert raw(c["routes"], c["windows"], [0.0, 0.0, 0.0, np.nan, 0.0], 2) == INVALID
    assert b"member 3: reloc_below is NaN" in eng._lib.dv_last_error(eng._ctx)
    assert raw(c["routes"], c["windows"], None, 3) == INVALID and b"channel 3" in eng._lib.dv_last_error(eng._ctx)
    assert raw([3, 1, 5, 0, 3], c["windows"], None, 2) == INVALID and b"route_of_member[2] = 5" in eng._lib.dv_last_error(eng._ctx)
    assert raw(c["routes"], c["windows"], None, 2) == 0 and np.array_equal(ssd, before.angle_ssd) and np.array_equal(view, before.angle_view)


# ---- 7. the ensemble ----------------------------------------------------------------------------------------------------------------------------------
ENS_CHANNEL, ENS_STEPS = 2, 20


class Counted(object):
    """Counts the ensemble's two device calls."""

    def __init__(self, engine):
        self.engine, self.calls = engine, []
        self.inner = (engine.rvssd_sense_step, engine.rvssdw_sense_step)
        engine.rvssd_sense_step = lambda *a, **k: self._call("rvssd", 0, a, k)
        engine.rvssdw_sense_step = lambda *a, **k: self._call("rvssdw", 1, a, k)

    def _call(self, name, which, a, k):
        self.calls.append((name, len(a[0]), "reloc_below" in k))
        return self.inner[which](*a, **k)

    def take(self):
        out, self.calls = self.calls, []
        return out

    def restore(self):
        self.engine.rvssd_sense_step, self.engine.rvssdw_sense_step = self.inner


def make_agent(land):
    return navsim_amd.NavBySceneFamiliarity(np.array(land), HL.ENS_SENSOR, 1.0, n_test_angles=9, use_gpu_sensor=True,
                                            familiarity_model=ssd_familiarity(ENS_CHANNEL))


def scenario_inputs():
    landscapes = HL.lands()[:3]
    routes = HL.ens_routes()
    return landscapes, routes, HL.ens_starts(routes)


def shadow_agents(landscapes, routes, starts, windows, centres, thresholds):
    out = []
    for i, (r, pos, ang) in enumerate(starts):
        l, path = routes[r]
        plug = H.SsdShadow(ENS_CHANNEL, windows[i], centres[i], thresholds[i])
        a = navsim_amd.NavBySceneFamiliarity(np.array(landscapes[l]), HL.ENS_SENSOR, 1.0, n_test_angles=9, use_gpu_sensor=False,
                                             familiarity_model=plug)
        a.train_from_path(path)
        a.position, a.angle = pos, ang
        out.append((a, plug))
    return out


def scene_want(shadow_row):
    """A shadow's scene_familiarity is -inf where its plug-in scored nothing; the reference's value for views never scored is +inf."""
    return np.where(np.isneginf(shadow_row), np.inf, shadow_row)


def same_state(ens, shadows, t):
    for i, (m, (a, plug)) in enumerate(zip(ens.agents, shadows)):
        assert m.position == a.position and m.angle == a.angle, (t, i)
        assert np.array_equal(bits(m.angle_familiarity), bits(a.angle_familiarity)), (t, i)
        assert m.memory_index == plug.memory_index, (t, i)
        assert m.relocalised == plug.relocalised and m.n_relocalisations == plug.n_relocalisations, (t, i)
        assert ens.stop_status[i] == (0 if a.stopped_with_exception is None else a.stopped_with_exception.get_code()), (t, i)


def same_scenes(ens, shadows, spans, t):
    rows = ens.scene_familiarity()
    for i, (a, plug) in enumerate(shadows):
        assert np.array_equal(bits(rows[i]), bits(scene_want(np.array(a.scene_familiarity)))), (t, i)
        if spans[i] is not None:                                                          # (the whole route after a re-localised step)
            lo, hi = spans[i]
            assert np.isposinf(rows[i][:lo]).all() and np.isposinf(rows[i][hi:]).all() and np.isfinite(rows[i][lo:hi]).all(), (t, i)


def test_windowed_and_unwindowed_members_side_by_side_equal_their_shadow_agents():
    """Twelve members on three landscapes: every third without a window, the others under (2, 3) or (1, 1); centres for most, two of
    them at the far end of the route (mis-centred) -- one of these with a threshold, which finds itself again in its first step, one
    without, which stays where it believes itself; relocalise() half way."""
    landscapes, routes, starts = scenario_inputs()
    lens = [len(routes[r][1]) for r, _, _ in starts]
    windows = [None if i % 3 == 0 else ((2, 3) if i % 3 == 1 else 1) for i in range(12)]
    pairs = [None if w is None else ((w, w) if isinstance(w, int) else w) for w in windows]
    centres = [None if w is None or i == 4 else (3 if i % 2 == 0 else 10) for i, w in enumerate(windows)]
    centres[1], centres[8] = lens[1] - 1, lens[8] - 1                                     # mis-centred
    thresholds = [None if w is None or i in (8, 10) else -1500000.0 for i, w in enumerate(windows)]
    agent = make_agent(landscapes[0])
    with pytest.raises(ValueError, match=r"relocalise_below\[0\] = -1.0, but member 0 has no window"):
        E.from_landscapes(agent, list(landscapes), routes, starts, window=windows, relocalise_below=[-1.0] + [None] * 11)
    ens = E.from_landscapes(agent, list(landscapes), routes, starts, window=windows, window_centres=centres, relocalise_below=thresholds)
    shadows = shadow_agents(landscapes, routes, starts, pairs, centres, thresholds)
    count = Counted(ens.engine)
    try:
        assert [a.window for a in ens.agents] == pairs and [a.memory_index for a in ens.agents] == centres
        assert [a.relocalise_below for a in ens.agents] == thresholds and [a.n_relocalisations for a in ens.agents] == [0] * 12
        for t in range(ENS_STEPS):
            if t == 10:
                ens.relocalise([2, 5])
                for i in (2, 5):
                    shadows[i][1].memory_index = None
            active = list(ens.active)
            win = [i for i in active if ens._window_of(ens.agents[i]) is not None]
            n_win, with_tau = len(win), any(thresholds[i] is not None for i in win)
            ens.step_forward()
            spans = [plug.step(a) for a, plug in shadows]
            same_state(ens, shadows, t)
            want_calls = ([("rvssdw", n_win, with_tau)] if n_win else []) + ([("rvssd", len(active) - n_win, False)] if len(active) > n_win else [])
            assert count.take() == want_calls, t                                          # at most two device calls a step
            if t in (0, 1, 10, ENS_STEPS - 1):
                same_scenes(ens, shadows, spans, t)
        n_reloc = [plug.n_relocalisations for _, plug in shadows]
        assert n_reloc[1] >= 1 and n_reloc[8] == 0 and shadows[1][1].spans[0] is None      # the rule fired where it should, and only by a threshold
        assert sum(n_reloc) == sum(a.n_relocalisations for a in ens.agents)
    finally:
        count.restore()
        ens.engine.close()


def test_a_window_as_long_as_the_routes_gives_the_unwindowed_ensembles_steps():
    """Routes of at most 256 views under window=255 (and every centre given): step by step the unwindowed ensemble."""
    landscapes, routes, starts = scenario_inputs()
    assert max(len(p) for _, p in routes) <= 256
    plain = E.from_landscapes(make_agent(landscapes[0]), list(landscapes), routes, starts, metrics="device")
    wide = E.from_landscapes(make_agent(landscapes[0]), list(landscapes), routes, starts, metrics="device", window=255,
                             window_centres=[0] * len(starts))
    count = Counted(wide.engine)
    try:
        for t in range(ENS_STEPS):
            n_active = len(wide.active)
            plain.step_forward()
            wide.step_forward()
            assert count.take() == ([("rvssdw", n_active, False)] if n_active else []), t
            for i, (m, a) in enumerate(zip(wide.agents, plain.agents)):
                assert m.position == a.position and m.angle == a.angle, (t, i)
                assert np.array_equal(bits(m.angle_familiarity), bits(a.angle_familiarity)), (t, i)
                assert m.navigation_error == a.navigation_error and m.percent_recapitulated == a.percent_recapitulated, (t, i)
            assert wide.stop_status == plain.stop_status, t
            if t in (0, ENS_STEPS - 1):
                for i, (got, want) in enumerate(zip(wide.scene_familiarity(), plain.scene_familiarity())):
                    assert np.array_equal(bits(got), bits(want)), (t, i)
    finally:
        count.restore()
        wide.engine.close()
        plain.engine.close()
