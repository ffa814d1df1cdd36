"""GPU tests of the branches of the route view store's kernels that the tests of their rule never enter (tests/helpers_rviews_edges.py;
tests/test_rviews_edges_host.py pins that the inputs reach them): the tile widths 12, 8 and 4 of k_rv_score, the list cap of k_rv_pick
at its value, the window lengths, empty pixel ranges, candidate counts and three-column tail of k_rvwin_score, DEJAVU_RVWIN_SPLIT=0,
and the second launch of calls with more than 32 768 members.  Everything is compared on its bits with oracle.step / oracle.sads_hsv
on every member's own route or slice, in the fast form and the exact form."""
import numpy as np
import pytest

import navsim_amd
from tests import helpers_rviews_edges as HE
from tests.helpers import engine_with
from tests.test_gpu_rviews import bits, check_step
from tests.test_gpu_rvwin import check_windowed

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng():
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


@pytest.fixture()
def flat():
    """An engine that does not cut short windows by pixels (the variable is read when the engine is created)."""
    e = engine_with({"DEJAVU_RVWIN_SPLIT": "0"})
    yield e
    e.close()


def win_want(case):
    return case["win_fam"], case["win_view"], case["win_best"]


# ---- A. tile widths of the unwindowed step ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", HE.TILE_SHAPES)
def test_tile_widths_12_8_and_4_equal_the_oracle(eng, h, w):
    """T = 12: three column blocks and an idle wave; T = 8: two column blocks x two view groups; T = 4: four view groups, on routes of
    2, 65 and 130 views -- the last workgroup of a route has view-group waves past its end."""
    c = HE.tile_case(h, w)
    eng.rviews_set_u8(c["views"], c["first"])
    check_step(eng, c)
    sc = eng.rviews_scene_u8(c["patches"], c["routes"], c["weights"])
    for got, want in zip(sc, c["scene"]):
        assert np.array_equal(bits(got), bits(want))


# ---- B. the list cap of k_rv_pick ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", HE.PICK_RUNS)
def test_a_full_list_and_one_candidate_more(eng, k):
    """256 identical views: the list is full and k_rv_pick scores it itself; 257: the column goes to the exact-all pass.  View 20, the
    first of the run, wins under each weight."""
    c = HE.pick_case(k)
    eng.rviews_set_u8(c["views"], c["first"])
    assert (c["view"][:, 0] == HE.PICK_AT).all() and (c["best"] == 0).all()
    check_step(eng, c)


def test_256_permuted_views_fill_the_list_and_the_first_exact_maximum_wins(eng):
    c = HE.permuted_case()
    eng.rviews_set_u8(c["views"], c["first"])
    check_step(eng, c)


# ---- C. window lengths -----------------------------------------------------------------------------------------------------------------------
def test_window_lengths_at_the_thresholds_of_the_pixel_cut(eng):
    """63 to 512 views at lo & 63 = 0, 1 and 63: where `parts` changes and where a wave takes a second chunk.  The near match of the
    window's last view wins; the exact copy of the view just outside the window does not."""
    c, windows = HE.window_case()
    eng.rviews_set_u8(c["views"], c["first"])
    P = HE.WIN_SHAPE[0] * HE.WIN_SHAPE[1]
    assert (c["win_best"] == 2).all() and (c["win_view"][:, 2] == np.array(windows)[:, 1] - 1).all() and (c["win_fam"][:, 0] < P).all()
    check_windowed(eng, c, windows, win_want(c))


# ---- D. tiny views ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", HE.TINY_SHAPES)
def test_tiny_views_leave_pixel_ranges_empty(eng, h, w):
    """Pw = 1, 2, 3 under cuts of 4 and 2 pixel ranges, column blocks with a three-column tail, and exact ties among the views."""
    for A in HE.TINY_A:
        c, windows = HE.tiny_case(h, w, A)
        eng.rviews_set_u8(c["views"], c["first"])
        check_windowed(eng, c, windows, win_want(c))


# ---- E. candidate counts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", HE.COUNT_RUNS)
def test_candidate_counts_at_the_two_thresholds(eng, k):
    """16 candidates: the wave scores them together; 17: a lane each; 256: still the candidates only; 257: every view of the window.
    View 100, the first of the run, wins; under a window that starts inside the run its own first view, 105."""
    c, windows = HE.count_case(k)
    eng.rviews_set_u8(c["views"], c["first"])
    assert (c["win_view"][:, 0] == HE.COUNT_AT).all()
    check_windowed(eng, c, windows, win_want(c))
    c, windows = HE.count_case(k, HE.COUNT_INSIDE)
    assert (c["win_view"][:, 0] == HE.COUNT_INSIDE[0]).all()
    check_windowed(eng, c, windows, win_want(c))


# ---- F. DEJAVU_RVWIN_SPLIT=0 -------------------------------------------------------------------------------------------------------------------
def same_bits_without_the_cut(eng, flat, cases):
    for c, windows in cases:
        lo, hi = [w[0] for w in windows], [w[1] for w in windows]
        for e in (eng, flat):
            e.rviews_set_u8(c["views"], c["first"])
        check_windowed(flat, c, windows, win_want(c))
        for exact in (False, True):
            a = eng.rvwin_step_u8(c["patches"], c["routes"], c["weights"], lo, hi, exact=exact)
            b = flat.rvwin_step_u8(c["patches"], c["routes"], c["weights"], lo, hi, exact=exact)
            assert np.array_equal(bits(a.angle_familiarity), bits(b.angle_familiarity)) and np.array_equal(a.angle_view, b.angle_view), exact
            assert np.array_equal(a.best_idex, b.best_idex) and not b.flags.any(), exact


def test_without_the_pixel_cut_the_window_lengths_give_the_same_bits(eng, flat):
    same_bits_without_the_cut(eng, flat, [HE.window_case()])


def test_without_the_pixel_cut_the_tiny_views_give_the_same_bits(eng, flat):
    same_bits_without_the_cut(eng, flat, [HE.tiny_case(h, w, A) for h, w in HE.TINY_SHAPES for A in HE.TINY_A])


# ---- G. more than 32 768 members -------------------------------------------------------------------------------------------------------------
MANY_ROWS = (0, 32767, 32768, 32770)


def test_32771_members_take_a_second_launch(eng):
    """The windowed step's and the scene call's second launch (members 32 768 - 32 770 differ from members 0 - 2), and the unwindowed
    step's 65 542 columns in three slabs cut by the cap on a slab's columns."""
    c, windows = HE.many_table()
    entry = HE.many_entry()
    n = len(entry)
    patches, routes, weights = c["patches"][entry], c["routes"][entry], c["weights"][entry]
    lo, hi = np.array(windows)[entry].T
    eng.rviews_set_u8(c["views"], c["first"])
    for exact in (False, True):
        r = eng.rvwin_step_u8(patches, routes, weights, lo, hi, exact=exact)
        for i in MANY_ROWS:
            assert np.array_equal(bits(r.angle_familiarity[i]), bits(c["win_fam"][i % 7])), (exact, i)
            assert np.array_equal(r.angle_view[i], c["win_view"][i % 7]) and r.best_idex[i] == c["win_best"][i % 7], (exact, i)
        assert np.array_equal(bits(r.angle_familiarity), bits(c["win_fam"][entry])), exact
        assert np.array_equal(r.angle_view, c["win_view"][entry]) and np.array_equal(r.best_idex, c["win_best"][entry]), exact
        assert r.angle_familiarity.shape == (n, HE.MANY_A) and not r.flags.any()
        u = eng.rviews_step_u8(patches, routes, weights, exact=exact)
        for i in MANY_ROWS:
            assert np.array_equal(bits(u.angle_familiarity[i]), bits(c["fam"][i % 7])), (exact, i)
            assert np.array_equal(u.angle_view[i], c["view"][i % 7]) and u.best_idex[i] == c["best"][i % 7], (exact, i)
        assert np.array_equal(bits(u.angle_familiarity), bits(c["fam"][entry])), exact
        assert np.array_equal(u.angle_view, c["view"][entry]) and np.array_equal(u.best_idex, c["best"][entry]), exact
        assert not u.flags.any()
    sc = eng.rviews_scene_u8(patches, routes, weights)
    assert len(sc) == n
    for i in MANY_ROWS:
        assert np.array_equal(bits(sc[i]), bits(c["scene"][i % 7])), i
    assert np.array_equal(bits(np.concatenate(sc)), bits(np.concatenate([c["scene"][k] for k in entry])))
