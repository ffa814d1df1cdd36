"""GPU tests of the windowed steps on the route view store (dv_rvwin_*) and of SadsRouteEnsemble's windows: against oracle.step on every
member's slice of its own route (tests/helpers_rvwin.py), against the unwindowed calls where the window is the whole route, and against
shadow agents whose sensor model and plug-in run on the host.  Familiarities are compared on their bits."""
import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import synth
from oracle import oracle
from tests import helpers_lands as HL
from tests import helpers_rviews as HR
from tests import helpers_rvwin as HW
from tests import helpers_sensors as HS
from tests.helpers import step_case_inputs
from tests.test_gpu_rviews import _csv, bits, check_step, make_agent, sensor_engine
from tests.test_gpu_sensors import table_engine

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -3
E = navsim_amd.SadsRouteEnsemble


@pytest.fixture()
def eng():
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


def lo_hi(windows):
    return [w[0] for w in windows], [w[1] for w in windows]


def check_windowed(e, case, windows, want):
    """The fast form and the exact form both give the oracle's record of every member's slice."""
    fam, view, best = want
    lo, hi = lo_hi(windows)
    for exact in (False, True):
        r = e.rvwin_step_u8(case["patches"], case["routes"], case["weights"], lo, hi, exact=exact)
        assert np.array_equal(bits(r.angle_familiarity), bits(fam)), exact
        assert np.array_equal(r.angle_view, view), exact
        assert np.array_equal(r.best_idex, best) and not r.flags.any(), exact


# ---- 1. rvwin_step_u8 against oracle.step on every member's slice -------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,A,kind", HW.STEP_CASES + ((19, 17, 17, "levels"), (19, 17, 5, "levels")))
def test_windowed_step_equals_the_oracle_on_every_members_slice(eng, h, w, A, kind):
    """A = 17 and A = 5: column blocks of four with a one-column tail; A = 260: 65 blocks a member."""
    case, want = HW.expected_case(h, w, A, kind)
    eng.rviews_set_u8(case["views"], case["first"])
    check_windowed(eng, case, HW.WINDOWS, want)


def test_wide_views_fill_the_patch_planes_of_a_block(eng):
    """64 x 64: 12 KiB of planes a patch, 48 KiB a block, beside 16 KiB of scores."""
    case, want = HW.expected_case(64, 64, 10, "random", windows=HW.WIDE_WINDOWS, **HW.WIDE)
    eng.rviews_set_u8(case["views"], case["first"])
    check_windowed(eng, case, HW.WIDE_WINDOWS, want)


# ---- 2. a window that is the whole route ----------------------------------------------------------------------------------------------------------
def test_whole_route_windows_equal_the_unwindowed_step_and_the_two_leave_each_other_alone(eng):
    case = HR.step_case(19, 17, 10, "levels", lengths=(2, 63, 64, 65, 512, 5))
    eng.rviews_set_u8(case["views"], case["first"])
    whole = HW.whole_routes(case)
    assert max(hi for _, hi in whole) == 512
    lo, hi = lo_hi(whole)
    narrow = tuple((l // 2, max(l // 2 + 1, l - 3)) for _, l in whole)
    narrow_want = HW.expected(case, narrow)
    for exact in (False, True):
        u = eng.rviews_step_u8(case["patches"], case["routes"], case["weights"], exact=exact)
        assert np.array_equal(bits(u.angle_familiarity), bits(case["fam"])) and np.array_equal(u.angle_view, case["view"])
        r = eng.rvwin_step_u8(case["patches"], case["routes"], case["weights"], lo, hi, exact=exact)
        assert np.array_equal(bits(r.angle_familiarity), bits(u.angle_familiarity)), exact
        assert np.array_equal(r.angle_view, u.angle_view) and np.array_equal(r.best_idex, u.best_idex), exact
    # windowed calls between unwindowed ones and the other way round: everybody keeps their bits
    check_windowed(eng, case, narrow, narrow_want)
    check_step(eng, case)
    check_windowed(eng, case, narrow, narrow_want)
    check_windowed(eng, case, whole, (case["fam"], case["view"], case["best"]))
    check_step(eng, case)


# ---- 3. ties --------------------------------------------------------------------------------------------------------------------------------------
def slice_want(views, patches, cw, lo, hi):
    lib = np.ascontiguousarray(views[lo:hi])
    want = oracle.step(lib, patches, cw)
    view = np.array([lo + int(np.argmax(oracle.sads_hsv(lib, p, cw))) for p in patches])
    return want, view


def test_duplicate_views_the_first_one_inside_the_window_wins(eng):
    v, p = HW.duplicates()
    decoy = synth.random_hsv(9, (7, 8, 8, 3))
    eng.rviews_set_u8(np.concatenate([decoy, v]), [0, 7, 207])
    patches = np.stack([p, synth.random_hsv(13, (8, 8, 3))])[None].repeat(4, axis=0)
    windows = ((50, 200), (101, 200), (0, 200), (11, 100))
    lo, hi = lo_hi(windows)
    for exact in (False, True):
        r = eng.rvwin_step_u8(patches, [1] * 4, [0.3] * 4, lo, hi, exact=exact)
        assert r.angle_view[:, 0].tolist()[:3] == [100, 150, 10] and (r.angle_familiarity[:3, 0] == 64.0).all() and r.angle_familiarity[3, 0] < 64.0
        for i, (l, h) in enumerate(windows):
            want, view = slice_want(v, patches[i], 0.3, l, h)
            assert np.array_equal(bits(r.angle_familiarity[i]), bits(want["angle_familiarity"])) and np.array_equal(r.angle_view[i], view)
            assert r.best_idex[i] == want["best_idex"]


def test_permuted_views_are_all_candidates_and_the_first_exact_maximum_wins(eng):
    views, patch = HR.permuted_route(8, 8, 40, 3)
    decoy = synth.random_hsv(9, (4, 8, 8, 3))
    patches = np.stack([patch, views[5]])[None]
    eng.rviews_set_u8(np.concatenate([decoy, views]), [0, 4, 44])
    for cw in (0.3, 0.0, 1.0):
        assert HR.statement(np.ascontiguousarray(views[5:40]), patches[0], cw)[3] == 35
        want, view = slice_want(views, patches[0], cw, 5, 40)
        for exact in (False, True):
            r = eng.rvwin_step_u8(patches, [1], [cw], [5], [40], exact=exact)
            assert np.array_equal(bits(r.angle_familiarity[0]), bits(want["angle_familiarity"])) and r.best_idex[0] == want["best_idex"]
            assert np.array_equal(r.angle_view[0], view)


def test_three_hundred_identical_views_overflow_the_list_inside_the_launch_and_view_60_wins(eng):
    views, patches = HW.identical_run()
    decoy = synth.random_hsv(9, (5, 8, 8, 3))
    eng.rviews_set_u8(np.concatenate([decoy, views]), [0, 5, 405])
    windows = ((50, 400), (0, 400), (100, 200), (0, 60))
    lo, hi = lo_hi(windows)
    both = np.stack([patches] * 4)
    for exact in (False, True):
        r = eng.rvwin_step_u8(both, [1] * 4, [0.3, 0.3, 0.0, 1.0], lo, hi, exact=exact)
        assert r.angle_view[:3, 0].tolist() == [60, 60, 100]
        for i, ((l, h), cw) in enumerate(zip(windows, (0.3, 0.3, 0.0, 1.0))):
            want, view = slice_want(views, patches, cw, l, h)
            assert np.array_equal(bits(r.angle_familiarity[i]), bits(want["angle_familiarity"])) and np.array_equal(r.angle_view[i], view), (exact, i)


def test_the_golden_tie_library_under_windows_around_its_best_view(eng, manifest):
    case = [c for c in manifest["t2_step"] if c["name"] == "s_ties_8x8"][0]
    lib, patches = step_case_inputs(case)
    b = case["best_view"]
    assert len(lib) == 20000 and b == 11817
    decoy = synth.synth_views(5, 9, case["h"], case["w"])
    eng.rviews_set_u8(np.concatenate([decoy, lib]), [0, 9, 9 + len(lib)])
    windows = ((b, b + 512), (b - 511, b + 1), (12000, 12512))
    lo, hi = lo_hi(windows)
    wants = [slice_want(lib, patches, case["chem_weight"], l, h) for l, h in windows]
    for exact in (False, True):
        r = eng.rvwin_step_u8(np.stack([patches] * 3), [1] * 3, [case["chem_weight"]] * 3, lo, hi, exact=exact)
        for i, (want, view) in enumerate(wants):
            assert np.array_equal(bits(r.angle_familiarity[i]), bits(want["angle_familiarity"])), (exact, i)
            assert np.array_equal(r.angle_view[i], view) and r.best_idex[i] == want["best_idex"], (exact, i)
        for i in (0, 1):                                                                  # the library's own best view, at the window's first and last place
            assert r.best_idex[i] == case["best_idex"] and r.angle_view[i, case["best_idex"]] == b
            assert r.angle_familiarity[i, case["best_idex"]] == case["step_familiarity"]
        assert r.angle_familiarity[2, case["best_idex"]] <= case["step_familiarity"]


# ---- 4. members are independent -------------------------------------------------------------------------------------------------------------------
def test_members_are_independent(eng):
    case, (fam, view, best) = HW.expected_case(19, 17, 10, "levels")
    eng.rviews_set_u8(case["views"], case["first"])
    lo, hi = np.array(lo_hi(HW.WINDOWS))
    perm = np.array([3, 6, 0, 5, 1, 4, 2])
    for exact in (False, True):
        r = eng.rvwin_step_u8(case["patches"][perm], case["routes"][perm], case["weights"][perm], lo[perm], hi[perm], exact=exact)
        assert np.array_equal(bits(r.angle_familiarity), bits(fam[perm])) and np.array_equal(r.angle_view, view[perm])
        assert np.array_equal(r.best_idex, best[perm])
    # two members on one route (route 4, 1 043 views) with different windows, one patch set; then one window under three weights
    p = case["patches"][0]
    views4 = case["views"][case["first"][4]:case["first"][5]]
    for windows, weights in ((((0, 200), (150, 662), (1042, 1043)), (0.3, 0.3, 0.3)), (((100, 400),) * 3, (0.0, 0.3, 1.0))):
        l, h = lo_hi(windows)
        r = eng.rvwin_step_u8(np.stack([p] * 3), [4] * 3, weights, l, h)
        for i in range(3):
            want, wview = slice_want(views4, p, weights[i], *windows[i])
            assert np.array_equal(bits(r.angle_familiarity[i]), bits(want["angle_familiarity"])) and np.array_equal(r.angle_view[i], wview)
            assert r.best_idex[i] == want["best_idex"]
        assert not np.array_equal(bits(r.angle_familiarity[0]), bits(r.angle_familiarity[1]))


# ---- 5. sensing -----------------------------------------------------------------------------------------------------------------------------------
def sq_store():
    t = HL.train_case("sq")
    order = np.concatenate(t["first"])
    return t["scenes"][order], HR.first_of([len(f) for f in t["first"]])


def member_windows(first, routes):
    """A window per member inside its route, none of them the whole route."""
    lens = np.diff(first)[routes]
    lo = np.array([1 + i % 3 for i in range(len(routes))])
    hi = np.array([l - (i + 1) % 2 for i, l in enumerate(lens)])
    assert (lo < hi).all() and ((lo > 0) | (hi < lens)).all()
    return lo, hi


def same_results(a, b, rows=None):
    rows = np.arange(len(a.best_idex)) if rows is None else rows
    assert np.array_equal(bits(a.angle_familiarity[rows]), bits(b.angle_familiarity[rows])) and np.array_equal(a.angle_view[rows], b.angle_view[rows])
    assert np.array_equal(a.best_idex[rows], b.best_idex[rows])


def test_sensed_windowed_steps_equal_uploaded_ones_on_the_engines_landscape_and_on_a_set():
    c = HL.step_case("sq", 5, 13)
    views, first = sq_store()
    weights = np.array([0.25, 0.0, 1.0, 0.5, 0.3])
    lo, hi = member_windows(first, c["banks"])
    e = sensor_engine("sq", HL.lands()[0])
    try:
        e.rviews_set_u8(views, first)
        # the engine's one landscape: the host model's patches on L0
        on0 = np.stack([HL.host_scenes("sq", [c["xs"][i]] * 13, [c["ys"][i]] * 13, c["angs"][i], [0] * 13) for i in range(5)])
        for exact in (False, True):
            up = e.rvwin_step_u8(on0, c["banks"], weights, lo, hi, exact=exact)
            fam, view, best = HW.expected(dict(views=views, first=first, patches=on0, routes=c["banks"], weights=weights), list(zip(lo, hi)))
            assert np.array_equal(bits(up.angle_familiarity), bits(fam)) and np.array_equal(up.angle_view, view) and np.array_equal(up.best_idex, best)
            s = e.rvwin_sense_step(c["xs"], c["ys"], c["angs"], c["banks"], weights, lo, hi, exact=exact)
            same_results(s, up)
            assert not s.flags.any()
        # a landscape set: every member on its own landscape
        e.lands_set(list(HL.lands()))
        up = e.rvwin_step_u8(c["planes"], c["banks"], weights, lo, hi)
        s = e.rvwin_sense_step(c["xs"], c["ys"], c["angs"], c["banks"], weights, lo, hi, land_of_member=c["lands"])
        same_results(s, up)
        assert not s.flags.any() and not np.array_equal(c["planes"], on0)
        # member 2 off its own landscape: flag 16 for it, the others keep their rows
        xs, ys, land_of = HL.flag_case("sq")
        f = e.rvwin_sense_step(xs, ys, c["angs"], c["banks"], weights, lo, hi, land_of_member=land_of)
        assert f.flags.tolist() == [0, 0, HL.SENSE_ERROR, 0, 0] and f.best_idex[2] == -1
        same_results(f, up, rows=np.array([0, 1, 3, 4]))
    finally:
        e.close()


def test_sensed_windowed_steps_under_a_sensor_table():
    c = HS.step_case("wide", 5, 13)
    views, first = HS.route_views("wide")[:2]
    weights = np.array([0.25, 0.0, 1.0, 0.5, 0.3])
    lo, hi = member_windows(first, c["banks"])
    e = table_engine("wide")
    try:
        e.rviews_set_u8(views, first)
        up = e.rvwin_step_u8(c["planes"], c["banks"], weights, lo, hi)
        fam, view, best = HW.expected(dict(views=views, first=first, patches=c["planes"], routes=c["banks"], weights=weights), list(zip(lo, hi)))
        assert np.array_equal(bits(up.angle_familiarity), bits(fam)) and np.array_equal(up.angle_view, view)
        s = e.rvwin_sense_step(c["xs"], c["ys"], c["angs"], c["banks"], weights, lo, hi, land_of_member=c["lands"])
        same_results(s, up)
        assert not s.flags.any()
    finally:
        e.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refused_windows_leave_everything_as_it_was(eng):
    case, want = HW.expected_case(19, 17, 10, "levels")
    n, A = case["patches"].shape[:2]
    fam, view, best = np.empty((n, A)), np.empty((n, A), dtype=np.int64), np.empty(n, dtype=np.int32)
    flags = np.zeros(n, dtype=np.uint32)
    z, angs = np.full(n, 50.0), np.zeros((n, A))

    def raw(lo, hi, routes=case["routes"], sensed=False):
        lo, hi, routes = np.array(lo, dtype=np.int32), np.array(hi, dtype=np.int32), np.array(routes, dtype=np.int32)
        p = lambda a: a.ctypes.data_as(N._i32p)
        if sensed:
            return eng._lib.dv_rvwin_sense_step(eng._ctx, N.f64ptr(z), N.f64ptr(z), N.f64ptr(angs), n, A, p(routes), N.f64ptr(case["weights"]), None,
                                                p(lo), p(hi), 0, N.f64ptr(fam), N.i64ptr(view), p(best), flags.ctypes.data_as(N._u32p))
        return eng._lib.dv_rvwin_step_u8(eng._ctx, N.u8ptr(case["patches"]), n, A, p(routes), N.f64ptr(case["weights"]), p(lo), p(hi), 0,
                                         N.f64ptr(fam), N.i64ptr(view), p(best))
    lo, hi = lo_hi(HW.WINDOWS)
    assert raw(lo, hi) == STATE and b"no route views" in eng._lib.dv_last_error(eng._ctx)
    assert raw(lo, hi, sensed=True) == STATE
    eng.rviews_set_u8(case["views"], case["first"])
    check_step(eng, case)
    check_windowed(eng, case, HW.WINDOWS, want)
    for i, l, h, text in ((0, -1, 70, b"member 0: window [-1, 70)"), (5, 63, 66, b"member 5: window [63, 66)"), (6, 40, 40, b"member 6: window [40, 40)"),
                          (6, 41, 40, b"member 6"), (3, 530, 1043, b"member 3: window [530, 1043)"), (1, 2, 3, b"member 1")):
        blo, bhi = list(lo), list(hi)
        blo[i], bhi[i] = l, h
        for sensed in (False, True):
            assert raw(blo, bhi, sensed=sensed) == INVALID and text in eng._lib.dv_last_error(eng._ctx), (i, sensed)
    bad = case["routes"].copy()
    bad[3] = 6
    assert raw(lo, hi, routes=bad) == INVALID and b"route_of_member[3] = 6" in eng._lib.dv_last_error(eng._ctx)
    assert raw(lo, hi, sensed=True) == STATE and b"sensor" in eng._lib.dv_last_error(eng._ctx)   # (no sensor on this engine)
    with pytest.raises(ValueError, match="member 3"):
        eng.rvwin_step_u8(case["patches"], case["routes"], case["weights"], [0] * 7, [1, 1, 1, 1044, 1, 1, 1])
    assert np.array_equal(eng.rviews_info()["first"], case["first"])
    check_step(eng, case)
    check_windowed(eng, case, HW.WINDOWS, want)


# ---- 7. the ensemble ------------------------------------------------------------------------------------------------------------------------------
class Counted(object):
    """Counts the ensemble's two device calls."""

    def __init__(self, engine):
        self.engine, self.calls = engine, []
        self.inner = (engine.rviews_sense_step, engine.rvwin_sense_step)
        engine.rviews_sense_step = lambda *a, **k: self._call("rviews", 0, a, k)
        engine.rvwin_sense_step = lambda *a, **k: self._call("rvwin", 1, a, k)

    def _call(self, name, which, a, k):
        self.calls.append((name, len(a[0])))
        return self.inner[which](*a, **k)

    def take(self):
        out, self.calls = self.calls, []
        return out

    def restore(self):
        self.engine.rviews_sense_step, self.engine.rvwin_sense_step = self.inner


def scenario_inputs():
    landscapes = HL.lands()[:3]
    routes = HL.ens_routes()
    return landscapes, routes, HL.ens_starts(routes)


def scene_want(shadow_row):
    """A shadow's scene_familiarity is -inf where its plug-in scored nothing; the reference's value for views never scored is +inf."""
    return np.where(np.isneginf(shadow_row), np.inf, shadow_row)


def step_both(ens, shadows):
    ens.step_forward()
    for a, plug in shadows:
        plug.step(a)


def same_state(ens, shadows, t):
    for i, (m, (a, plug)) in enumerate(zip(ens.agents, shadows)):
        assert m.position == a.position and m.angle == a.angle, (t, i)
        assert np.array_equal(bits(m.angle_familiarity), bits(a.angle_familiarity)), (t, i)
        assert m.memory_index == plug.memory_index, (t, i)
        assert ens.stop_status[i] == (0 if a.stopped_with_exception is None else a.stopped_with_exception.get_code()), (t, i)


@pytest.mark.parametrize("metrics", ("host", "device"))
def test_windowed_members_equal_their_shadow_agents(metrics):
    landscapes, routes, starts = scenario_inputs()
    want = HW.scenario(True)
    ens = E.from_landscapes(make_agent(landscapes[0]), list(landscapes), routes, starts, metrics=metrics, chem_weights=HW.ENS_WEIGHTS,
                            window=HW.ENS_WINDOW)
    count = Counted(ens.engine)
    try:
        assert [a.window for a in ens.agents] == [HW.ENS_WINDOW] * 12 and [a.memory_index for a in ens.agents] == [None] * 12
        for t in range(HW.ENS_STEPS):
            n_active = len(ens.active)
            ens.step_forward()
            assert count.take() == [("rviews" if t == 0 else "rvwin", n_active)], t      # ONE device call a step
            for i, (m, w) in enumerate(zip(ens.agents, want)):
                assert m.position == w["pos"][t] and m.angle == w["ang"][t], (t, i)
                assert np.array_equal(bits(m.angle_familiarity), bits(w["fam"][t])), (t, i)
                assert m.memory_index == w["memory"][t] and ens.stop_status[i] == w["code"][t], (t, i)
            if t in (0, HW.ENS_STEPS - 1):
                rows = ens.scene_familiarity()
                for i, (m, w) in enumerate(zip(ens.agents, want)):
                    assert np.array_equal(bits(rows[i]), bits(scene_want(w["scene"][t]))), (t, i)
                    assert np.array_equal(bits(m.scene_familiarity), bits(rows[i])), (t, i)
                    if t and w["spans"][t] is not None:
                        lo, hi = w["spans"][t]
                        assert np.isposinf(rows[i][:lo]).all() and np.isposinf(rows[i][hi:]).all() and np.isfinite(rows[i][lo:hi]).all()
        assert ens.stop_status == [0] * 11 + [1]
        cover = ens.coverage_summary(0.05)
        for i, (m, w) in enumerate(zip(ens.agents, want)):
            assert m.navigation_error == w["error"] and m.percent_recapitulated == w["coverage"] == cover[i]["path_coverage"], i
    finally:
        count.restore()
        ens.engine.close()


def test_a_window_longer_than_the_routes_gives_the_unwindowed_ensembles_rows():
    landscapes, routes, starts = scenario_inputs()
    texts = []
    for window in (None, (255, 256)):
        agent = make_agent(landscapes[0])
        with pytest.raises(ValueError, match="<= 512"):                                   # refused before anything is made: the agent serves again
            E.from_landscapes(agent, list(landscapes), routes, starts, chem_weights=HW.ENS_WEIGHTS, window=(600, 0))
        ens = E.from_landscapes(agent, list(landscapes), routes, starts, metrics="device", chem_weights=HW.ENS_WEIGHTS, window=window)
        count = Counted(ens.engine)
        try:
            texts.append(_csv(navsim_amd.run_ensemble(ens)))
            names = set(name for name, _ in count.take())
            assert names == ({"rviews"} if window is None else {"rviews", "rvwin"})
        finally:
            count.restore()
            ens.engine.close()
    assert texts[0] == texts[1]


def test_windows_per_member_centres_and_relocalise():
    landscapes, routes, starts = scenario_inputs()
    windows = [None if i % 3 == 0 else ((2, 3) if i % 3 == 1 else 1) for i in range(12)]
    pairs = [None if w is None else ((w, w) if isinstance(w, int) else w) for w in windows]
    centres = [None if w is None or i == 4 else (3 if i % 2 == 0 else 10) for i, w in enumerate(windows)]
    n_win = sum(w is not None for w in windows)
    agent = make_agent(landscapes[0])
    with pytest.raises(ValueError, match=r"window_centres\[1\] = 30 outside \[0, 30\)"):
        E.from_landscapes(agent, list(landscapes), routes, starts, window=windows, window_centres=[None, 30] + [None] * 10)
    ens = E.from_landscapes(agent, list(landscapes), routes, starts, chem_weights=HW.ENS_WEIGHTS, window=windows, window_centres=centres)
    shadows = HW.shadow_agents(landscapes, routes, starts, HW.ENS_WEIGHTS, pairs, centres)
    count = Counted(ens.engine)
    try:
        assert [a.window for a in ens.agents] == pairs and [a.memory_index for a in ens.agents] == centres
        for t in range(4):
            step_both(ens, shadows)
            same_state(ens, shadows, t)
            # the members with a window and a centre in one call, the others (no window; member 4 in its first step) in the other
            first = sum(c is not None for c in centres)
            assert count.take() == [("rvwin", first if t == 0 else n_win), ("rviews", 12 - (first if t == 0 else n_win))], t
        assert all((a.memory_index is None) == (w is None) for a, w in zip(ens.agents, pairs))
        rows = ens.scene_familiarity()
        for i, (a, _) in enumerate(shadows):
            assert np.array_equal(bits(rows[i]), bits(scene_want(np.array(a.scene_familiarity)))), i
        ens.relocalise([1, 5])
        for i in (1, 5):
            shadows[i][1].memory_index = None
        assert [ens.agents[i].memory_index for i in (1, 5, 7)] == [None, None, shadows[7][1].memory_index]
        step_both(ens, shadows)
        same_state(ens, shadows, "relocalised")
        assert count.take() == [("rvwin", n_win - 2), ("rviews", 12 - n_win + 2)]
        assert shadows[1][1].spans[-1] == (0, len(ens.agents[1].training_path))
        ens.relocalise()
        assert all(a.memory_index is None for a in ens.agents)
        for _, plug in shadows:
            plug.memory_index = None
        step_both(ens, shadows)
        same_state(ens, shadows, "all relocalised")
        assert count.take() == [("rviews", 12)]
    finally:
        count.restore()
        ens.engine.close()
