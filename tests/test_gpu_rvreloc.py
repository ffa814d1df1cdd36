"""GPU tests of the re-localisation inside the windowed step (dv_rvreloc_*: FamiliarityEngine.rvwin_step_u8 / rvwin_sense_step with
reloc_below) and of SadsRouteEnsemble's relocalise_below.  Everything is held against oracle.step (tests/helpers_rvreloc.py): on every
member's window slice, and on its whole route where the rule triggers; thresholds come from the oracle's windowed rows, never from the
code under test.  Familiarities are compared on their bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from tests import helpers_lands as HL
from tests import helpers_rviews_edges as HE
from tests import helpers_rvreloc as H
from tests import helpers_rvwin as HW
from tests import helpers_sensors as HS
from tests.test_gpu_rviews import sensor_engine
from tests.test_gpu_rvwin import Counted, lo_hi, member_windows, scene_want, sq_store
from tests.test_gpu_sensors import table_engine

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = navsim_amd.SadsRouteEnsemble
bits = H.bits


@pytest.fixture()
def eng():
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


def step_u8(e, case, windows, taus, exact=False):
    lo, hi = lo_hi(windows)
    return e.rvwin_step_u8(case["patches"], case["routes"], case["weights"], lo, hi, exact=exact, reloc_below=taus)


# ---- 1. the basic case: mixed thresholds, both forms, fast and exact --------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", H.BASIC_SHAPES)
def test_mixed_thresholds_on_uploaded_patches(eng, h, w):
    """-inf, +inf, the windowed maximum itself (stays) and the next double above it (goes): routes of 2, 65 and 130 views, weights 0,
    0.25 and 1, six members x five headings."""
    case, windowed, whole = H.basic(h, w)
    want = H.apply_rule(windowed, whole, H.mixed_thresholds(windowed))
    eng.rviews_set_u8(case["views"], case["first"])
    for exact in (False, True):
        H.check(step_u8(eng, case, H.BASIC_WINDOWS, H.mixed_thresholds(windowed), exact=exact), want)
    eng.set_exact(True)                                                                    # dv_set_exact: the same results
    H.check(step_u8(eng, case, H.BASIC_WINDOWS, H.mixed_thresholds(windowed)), want)


def sensed_engine(h, w, lut):
    e = navsim_amd.FamiliarityEngine(device=0)
    e.set_landscape(HL.lands()[0])
    e.configure_sensor((w, h), (2, 2), lut, 0)
    return e


@pytest.mark.parametrize("h,w", H.BASIC_SHAPES)
def test_mixed_thresholds_on_sensed_patches_and_the_state_the_call_leaves(h, w):
    """The sensed form gives the oracle's rows on the host model's patches; plain unwindowed and windowed calls after it (and it after
    them) return what they return on a fresh engine: the oracle's rows."""
    s = H.sensed_basic(h, w)
    case, windowed, whole = s["case"], s["windowed"], s["whole"]
    taus = H.mixed_thresholds(windowed)
    want = H.apply_rule(windowed, whole, taus)
    assert want[3].any() and not want[3].all()
    lo, hi = lo_hi(H.BASIC_WINDOWS)
    none = np.zeros(6, dtype=bool)
    e = sensed_engine(h, w, s["lut"])
    try:
        e.rviews_set_u8(case["views"], case["first"])
        pose = (s["xs"], s["ys"], s["angs"], case["routes"], case["weights"])
        for exact in (False, True):
            H.check(e.rvwin_sense_step(*pose, lo, hi, exact=exact, reloc_below=taus), want)
            H.check(step_u8(e, case, H.BASIC_WINDOWS, taus, exact=exact), want)
            r = e.rviews_sense_step(*pose, exact=exact)
            assert np.array_equal(bits(r.angle_familiarity), bits(whole[0])) and np.array_equal(r.angle_view, whole[1]) and not r.flags.any()
            r = e.rvwin_sense_step(*pose, lo, hi, exact=exact)
            assert np.array_equal(bits(r.angle_familiarity), bits(windowed[0])) and np.array_equal(r.angle_view, windowed[1]) and not r.flags.any()
            H.check(e.rvwin_sense_step(*pose, lo, hi, exact=exact, reloc_below=taus), want)
            H.check(e.rvwin_sense_step(*pose, lo, hi, exact=exact, reloc_below=np.full(6, H.NEVER)), windowed + (none,))
        # a refused call (a NaN, named) changes nothing
        fam, view, best, flags = np.empty((6, 5)), np.empty((6, 5), dtype=np.int64), np.empty(6, dtype=np.int32), np.zeros(6, dtype=np.uint32)
        bad = taus.copy()
        bad[4] = np.nan
        p = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(N._i32p)
        rc = e._lib.dv_rvreloc_sense_step(e._ctx, N.f64ptr(s["xs"]), N.f64ptr(s["ys"]), N.f64ptr(s["angs"]), 6, 5, p(case["routes"]),
                                          N.f64ptr(case["weights"]), None, p(lo), p(hi), N.f64ptr(bad), 0, N.f64ptr(fam), N.i64ptr(view),
                                          p(best), flags.ctypes.data_as(N._u32p))
        assert rc == -1 and b"member 4: reloc_below is NaN" in e._lib.dv_last_error(e._ctx)
        rc = e._lib.dv_rvreloc_step_u8(e._ctx, N.u8ptr(case["patches"]), 6, 5, p(case["routes"]), N.f64ptr(case["weights"]), p(lo), p(hi),
                                       N.f64ptr(bad), 0, N.f64ptr(fam), N.i64ptr(view), p(best), flags.ctypes.data_as(N._u32p))
        assert rc == -1 and b"dv_rvreloc_step_u8: member 4: reloc_below is NaN" in e._lib.dv_last_error(e._ctx)
        H.check(e.rvwin_sense_step(*pose, lo, hi, reloc_below=taus), want)
    finally:
        e.close()


# ---- 2. nobody lost, everybody lost ----------------------------------------------------------------------------------------------------------
def test_nobody_lost_is_the_windowed_call_and_everybody_lost_the_unwindowed_one(eng):
    case, windowed, whole = H.basic(8, 8)
    eng.rviews_set_u8(case["views"], case["first"])
    lo, hi = lo_hi(H.BASIC_WINDOWS)
    for exact in (False, True):
        plain = eng.rvwin_step_u8(case["patches"], case["routes"], case["weights"], lo, hi, exact=exact)
        r = step_u8(eng, case, H.BASIC_WINDOWS, np.full(6, H.NEVER), exact=exact)
        assert np.array_equal(bits(r.angle_familiarity), bits(plain.angle_familiarity)) and np.array_equal(r.angle_view, plain.angle_view)
        assert np.array_equal(r.best_idex, plain.best_idex) and not r.flags.any() and not r.relocalised.any()
        H.check(r, windowed + (np.zeros(6, dtype=bool),))
        every = eng.rviews_step_u8(case["patches"], case["routes"], case["weights"], exact=exact)
        r = step_u8(eng, case, H.BASIC_WINDOWS, np.full(6, H.ALWAYS), exact=exact)
        assert np.array_equal(bits(r.angle_familiarity), bits(every.angle_familiarity)) and np.array_equal(r.angle_view, every.angle_view)
        assert np.array_equal(r.best_idex, every.best_idex) and r.relocalised.all()
        H.check(r, whole + (np.ones(6, dtype=bool),))


# ---- 3. lost counts per route: tiles of 16, 12, 8 and 4 columns --------------------------------------------------------------------------------
def test_lost_counts_per_route_give_every_tile_width(eng):
    """Route 0: 28 lost columns (two tiles, 16 and 12); route 1: nobody lost, between routes that have some; route 2: 8; route 3: 4;
    members not sorted by route, lost and kept ones mixed within a route."""
    case, windows, taus, want = H.counts_case()
    assert [(r, n) for _, n, r in H.device_plan(H.COUNTS_ROUTES, want[3], H.COUNTS_A, 16)[1]] == H.COUNTS_TILES
    eng.rviews_set_u8(case["views"], case["first"])
    for exact in (False, True):
        H.check(step_u8(eng, case, windows, taus, exact=exact), want)


def test_more_members_and_columns_than_one_pass_of_the_planning_workgroup(eng):
    """300 members x 2 headings on three routes, two in three lost: the prefix sums' running bases cross the passes of 256."""
    case, windows, taus, want = H.many_case()
    eng.rviews_set_u8(case["views"], case["first"])
    for exact in (False, True):
        H.check(step_u8(eng, case, windows, taus, exact=exact), want)


# ---- 4. more than 256 candidates ----------------------------------------------------------------------------------------------------------------
def test_a_lost_column_with_257_candidates_finishes_in_the_same_call(eng):
    """257 identical planted views: the lost members' heading 0 overflows k_rv_pick's list and goes through the exact-all pass; the
    member between them keeps its window."""
    c = HE.pick_case(257)
    windows = ((0, 10), (280, 300), (21, 150))
    windowed = HW.expected(c, windows)
    whole = (c["fam"], c["view"], c["best"])
    taus = np.array([H.go(windowed[0][0]), H.stay(windowed[0][1]), H.ALWAYS])
    want = H.apply_rule(windowed, whole, taus)
    assert want[3].tolist() == [True, False, True] and (want[1][[0, 2], 0] == HE.PICK_AT).all() and windowed[1][2, 0] == 21
    eng.rviews_set_u8(c["views"], c["first"])
    for exact in (False, True):
        H.check(step_u8(eng, c, windows, taus, exact=exact), want)


# ---- 5. 64 x 64 views ------------------------------------------------------------------------------------------------------------------------------
def test_wide_views_tile_limit_4_and_the_lds_above_64_kib(eng):
    """Routes of 70 and 3 views, three members x five headings: a lost member's five columns are tiles of 4 and 1."""
    case, windowed = HW.expected_case(64, 64, 5, "random", windows=HW.WIDE_WINDOWS, **HW.WIDE)
    whole = (case["fam"], case["view"], case["best"])
    taus = np.array([H.go(windowed[0][0]), H.stay(windowed[0][1]), H.ALWAYS])
    want = H.apply_rule(windowed, whole, taus)
    assert want[3].tolist() == [True, False, True] and HE.tile_width(64 * 64) == 4
    eng.rviews_set_u8(case["views"], case["first"])
    for exact in (False, True):
        H.check(step_u8(eng, case, HW.WIDE_WINDOWS, taus, exact=exact), want)
    H.check(step_u8(eng, case, HW.WIDE_WINDOWS, np.full(3, H.ALWAYS)), whole + (np.ones(3, dtype=bool),))


# ---- 6. a landscape set: the sense error, and a sensor table ------------------------------------------------------------------------------------
def test_a_member_off_its_landscape_is_not_relocalised_and_its_neighbours_are():
    c = HL.step_case("sq", 5, 13)
    views, first = sq_store()
    weights = np.array([0.25, 0.0, 1.0, 0.5, 0.3])
    lo, hi = member_windows(first, c["banks"])
    case = dict(views=views, first=first, patches=c["planes"], routes=c["banks"], weights=weights)
    windowed = HW.expected(case, list(zip(lo, hi)))
    fam, view, best, _ = H.HR.expected(views, first, c["planes"], c["banks"], weights)
    e = sensor_engine("sq", HL.lands()[0])
    try:
        e.rviews_set_u8(views, first)
        e.lands_set(list(HL.lands()))
        taus = np.array([H.ALWAYS, H.stay(windowed[0][1]), H.ALWAYS, H.go(windowed[0][3]), H.NEVER])
        want = H.apply_rule(windowed, (fam, view, best), taus)
        assert want[3].tolist() == [True, False, True, True, False]
        H.check(e.rvwin_sense_step(c["xs"], c["ys"], c["angs"], c["banks"], weights, lo, hi, land_of_member=c["lands"], reloc_below=taus), want)
        xs, ys, land_of = HL.flag_case("sq")                                              # member 2 off its own landscape, threshold +inf
        r = e.rvwin_sense_step(xs, ys, c["angs"], c["banks"], weights, lo, hi, land_of_member=land_of, reloc_below=taus)
        assert r.flags.tolist() == [32, 0, 16, 32, 0] and r.best_idex[2] == -1 and r.relocalised.tolist() == [True, False, False, True, False]
        H.check(r, want, flagged=(2,))
    finally:
        e.close()


def test_a_sensor_table_on_two_landscapes():
    c = HS.step_case("wide", 5, 13)
    views, first = HS.route_views("wide")[:2]
    keep = np.flatnonzero(c["lands"] < 2)                                                  # the members on landscapes 0 and 1
    assert keep.tolist() == [0, 1, 4] and sorted(set(c["lands"][keep].tolist())) == [0, 1]
    banks, weights, planes = c["banks"][keep], np.array([0.25, 0.0, 1.0]), np.ascontiguousarray(c["planes"][keep])
    lo, hi = member_windows(first, banks)
    case = dict(views=views, first=first, patches=planes, routes=banks, weights=weights)
    windowed = HW.expected(case, list(zip(lo, hi)))
    taus = np.array([H.go(windowed[0][0]), H.stay(windowed[0][1]), H.ALWAYS])
    want = H.apply_rule(windowed, H.HR.expected(views, first, planes, banks, weights)[:3], taus)
    e = table_engine("wide", pairs=((0, HS.TABLE[0]), (1, HS.TABLE[1])))
    try:
        e.rviews_set_u8(views, first)
        r = e.rvwin_sense_step(c["xs"][keep], c["ys"][keep], c["angs"][keep], banks, weights, lo, hi, land_of_member=c["lands"][keep], reloc_below=taus)
        H.check(r, want)
        assert want[3].tolist() == [True, False, True]
    finally:
        e.close()


# ---- 7. a small slab: the members fall into three groups -----------------------------------------------------------------------------------------
CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
from tests import helpers_rvreloc as H
from tests.helpers import engine_with
case, windowed, whole = H.basic(8, 8)
out = {}
for slab in ("10", "3"):
    e = engine_with({"DEJAVU_RVIEWS_SLAB": slab})
    e.rviews_set_u8(case["views"], case["first"])
    lo, hi = [w[0] for w in H.BASIC_WINDOWS], [w[1] for w in H.BASIC_WINDOWS]
    for name, taus in (("mixed", H.mixed_thresholds(windowed)), ("all", np.full(6, H.ALWAYS))):
        for exact in (False, True):
            r = e.rvwin_step_u8(case["patches"], case["routes"], case["weights"], lo, hi, exact=exact, reloc_below=taus)
            k = "%%s_%%s_%%d_" %% (slab, name, exact)
            out[k + "fam"], out[k + "view"], out[k + "best"], out[k + "flags"] = r.angle_familiarity, r.angle_view, r.best_idex, r.flags
    e.close()
np.savez(sys.argv[1], **out)
"""


def test_a_small_slab_cuts_the_members_into_three_groups(tmp_path):
    """A fresh process under DEJAVU_RVIEWS_SLAB = 10 (six members x five headings: three groups of two, a lost member in each) and = 3
    (less than a member's columns: a member a group): the results are those of one group, the oracle's."""
    assert H.groups(6, 5, 10) == [(0, 2), (2, 4), (4, 6)] and len(H.groups(6, 5, 3)) == 6
    path = str(tmp_path / "out.npz")
    env = {k: v for k, v in os.environ.items() if k != "DEJAVU_RVIEWS_SLAB"}
    done = subprocess.run([sys.executable, "-c", CHILD % (REPO, os.path.join(REPO, "navigation-by-deja-vu_amd")), path], env=env, timeout=120,
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    got = np.load(path)
    case, windowed, whole = H.basic(8, 8)
    wants = dict(mixed=H.apply_rule(windowed, whole, H.mixed_thresholds(windowed)), all=whole + (np.ones(6, dtype=bool),))
    for slab in ("10", "3"):
        for name, (fam, view, best, lost) in wants.items():
            for exact in (0, 1):
                k = "%s_%s_%d_" % (slab, name, exact)
                assert np.array_equal(bits(got[k + "fam"]), bits(fam)) and np.array_equal(got[k + "view"], view), k
                assert np.array_equal(got[k + "best"], best) and np.array_equal(got[k + "flags"], np.where(lost, 32, 0)), k


# ---- 8. the ensemble ------------------------------------------------------------------------------------------------------------------------------
def make_agent():
    return navsim_amd.NavBySceneFamiliarity(np.array(HL.lands()[0]), H.ENS_SENSOR, 1.0, n_test_angles=9, use_gpu_sensor=True,
                                            familiarity_model=navsim_amd.sads_familiarity(0.25))


@pytest.mark.parametrize("threshold", (H.ENS_THRESHOLD, None))
def test_mis_centred_members_find_themselves_again_as_their_shadows_do(threshold):
    """Two routes, four members on a 32 x 32 sensor, window (5, 5), members 1 and 3 centred on the far end of their routes.  With the
    threshold they relocalise in their first step and then track, as their shadow agents (host sensor model, the rule in Python); without
    it the ensemble gives what it gave before: they stay lost."""
    routes = H.ens_routes()
    starts = H.ens_starts(routes)
    want = H.scenario(threshold)
    ens = E.from_routes_with(make_agent(), routes, starts, chem_weights=H.ENS_WEIGHTS, window=H.ENS_WINDOW, window_centres=H.ens_centres(routes),
                             relocalise_below=threshold)
    count = Counted(ens.engine)
    try:
        assert [a.relocalise_below for a in ens.agents] == [threshold] * 4 and [a.n_relocalisations for a in ens.agents] == [0] * 4
        for t in range(H.ENS_STEPS):
            ens.step_forward()
            assert count.take() == [("rvwin", 4)], t                                      # ONE device call a step
            for i, (m, w) in enumerate(zip(ens.agents, want)):
                assert m.position == w["pos"][t] and m.angle == w["ang"][t], (t, i)
                assert np.array_equal(bits(m.angle_familiarity), bits(w["fam"][t])), (t, i)
                assert m.memory_index == w["memory"][t] and ens.stop_status[i] == w["code"][t], (t, i)
                assert m.relocalised == w["relocalised"][t] and m.n_relocalisations == w["n"][t], (t, i)
            if t in (0, 1, H.ENS_STEPS - 1):
                rows = ens.scene_familiarity()
                for i, w in enumerate(want):
                    assert np.array_equal(bits(rows[i]), bits(scene_want(w["scene"][t]))), (t, i)
        lost = [1, 3] if threshold is not None else []
        assert [a.n_relocalisations for a in ens.agents] == [int(i in lost) for i in range(4)]
    finally:
        count.restore()
        ens.engine.close()
