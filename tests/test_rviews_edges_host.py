"""The route-view edge tests' inputs, what needs no GPU: that every shape, route, window and run of tests/helpers_rviews_edges.py reaches
the branch of k_rv_score, k_rv_pick and k_rvwin_score it is named for.  The thresholds are read out of the two .inl files; the host's
arithmetic on them is restated in the helper."""
import numpy as np
import pytest

from tests import helpers_rviews as HR
from tests import helpers_rviews_edges as HE
from tests import helpers_rvwin as HW


def test_the_constants_are_the_sources():
    k = HE.constants()
    assert (k["kRvBlock"], k["kRvTileMax"], k["kRvLdsBytes"], k["kRvCandCap"], k["kRvWinCoop"]) == (4, 16, 48 * 1024, 256, 16)
    assert k["kRvCandCap"] == HR.CAND_CAP and k["slab_bytes"] == HR.SLAB_BYTES
    assert k["slab_cap"] == k["scene_launch"] == k["rvwin_launch"] == 32768
    assert HE.PICK_RUNS == (k["kRvCandCap"], k["kRvCandCap"] + 1)
    assert HE.COUNT_RUNS == (k["kRvWinCoop"], k["kRvWinCoop"] + 1, k["kRvCandCap"], k["kRvCandCap"] + 1)


# ---- A ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_tile_widths_of_the_shapes():
    for h, w, P, Pw, T in HE.TILE_TABLE:
        assert (h * w, (h * w + 3) // 4, HE.tile_width(h * w)) == (P, Pw, T), (h, w)
    assert sorted(set(t[4] for t in HE.TILE_TABLE[1:])) == [4, 8, 12] and HE.TILE_SHAPES == tuple(t[:2] for t in HE.TILE_TABLE if t[4] != 16)
    # the ranges of the two widths no other test enters, and their ends
    assert [HE.tile_width(P) for P in (1024, 1025, 1364, 1365, 2048, 2049, 4096)] == [16, 12, 12, 8, 8, 4, 4]
    assert [HE.wave_map(T) for T in (16, 12, 8, 4)] == [(4, 1), (3, 1), (2, 2), (1, 4)]
    # every existing shape of the unwindowed tests sits at T = 16, or at T = 4 with 4 096 pixels
    assert [HE.tile_width(h * w) for h, w in ((7, 5), (19, 17), (32, 32), (5, 7), (8, 8), (4, 4), (64, 64))] == [16] * 6 + [4]


@pytest.mark.parametrize("h,w", HE.TILE_SHAPES)
def test_the_tile_cases_fill_their_tiles_and_leave_waves_past_the_routes_end(h, w):
    T = HE.tile_width(h * w)
    ncb, vpw = HE.wave_map(T)
    c = HE.tile_case(h, w)
    assert c["first"].tolist() == [0, 2, 67, 197, 202] and c["patches"].shape == (5, 7, h, w, 3)
    got = HE.tiles(c["routes"], HE.TILE_A, T, 130)
    want = [(0, 4), (0, 3)] if T == 4 else [(0, 7)]                                         # route 0 has one member
    assert got == want + [(r, n) for r in (1, 2) for n in HE.TILE_SPLITS[T]]
    # the two members of routes 1 and 2 carry different weights, and at T >= 8 the first tile of the route holds columns of both
    order = np.argsort(c["routes"], kind="stable")
    assert c["routes"][order].tolist() == [0, 1, 1, 2, 2] and c["weights"][order].tolist() == [0.3, 0.3, 0.0, 0.0, 1.0]
    assert (HE.TILE_SPLITS[T][0] > HE.TILE_A) == (T >= 8)
    # groups of 64 views: 2 and 3; the last workgroup of a route has view-group waves past the route's end where vpw > 1
    groups = [-(-n // 64) for n in (65, 130)]
    assert groups == [2, 3]
    if vpw == 2:
        assert groups[1] % vpw == 1                                                       # a wave pair past 130 views
    if vpw == 4:
        assert vpw - groups[1] == 1 and vpw - groups[0] == 2                              # one wave past 130 views, two past 65
    if T == 12:
        assert ncb == 3 and vpw == 1                                                      # (the fourth wave idles)
    assert (c["fam"][:, 0] < h * w).all()                                                 # (the copy of another route's view found no equal)


# ---- B, E ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", HE.PICK_RUNS)
def test_the_pick_cases_have_the_candidates_they_are_named_for(k):
    c = HE.pick_case(k)
    cand = HE.candidates(c)
    assert cand[:, 0].tolist() == [k] * 3 and (cand[:, 1] <= 3).all()                      # under each of the three weights
    assert c["weights"].tolist() == [0.3, 0.0, 1.0] and c["first"].tolist() == [0, 5, 305]
    assert (c["view"][:, 0] == HE.PICK_AT).all() and (c["best"] == 0).all()
    assert np.array_equal(c["views"][5 + HE.PICK_AT], c["views"][5 + HE.PICK_AT + k - 1])
    assert not np.array_equal(c["views"][5 + HE.PICK_AT], c["views"][5 + HE.PICK_AT + k])


def test_the_permuted_route_fills_the_list_with_different_exact_values():
    c = HE.permuted_case()
    cand = HE.candidates(c)
    assert cand[:, 0].tolist() == [HE.constants()["kRvCandCap"]] * 3 and c["first"].tolist() == [0, 4, 260]
    # equal integer sums, different sequential doubles under a weight that mixes them: the first exact maximum is no list's first entry
    assert c["view"][0, 0] != 0 and len(set(c["view"][:, 0].tolist())) > 1 and (c["view"][:, 1] == 5).all()


@pytest.mark.parametrize("k", HE.COUNT_RUNS)
def test_the_count_cases_have_the_candidates_they_are_named_for(k):
    c, windows = HE.count_case(k)
    assert windows == ((90, 490),) * 3 and c["first"].tolist() == [0, 5, 525]
    cand = HE.candidates(c, windows)
    assert cand[:, 0].tolist() == [k] * 3 and (cand[:, 1] <= 3).all()
    assert (c["win_view"][:, 0] == HE.COUNT_AT).all() and (c["win_best"] == 0).all()
    # the window that starts inside the run: its first view wins
    c2, inside = HE.count_case(k, HE.COUNT_INSIDE)
    assert inside == ((105, 505),) * 3 and HE.COUNT_AT < 105 < HE.COUNT_AT + k
    assert HE.candidates(c2, inside)[:, 0].tolist() == [k - 5] * 3 and (c2["win_view"][:, 0] == 105).all()
    for (lo, hi), phase in ((HE.COUNT_WINDOW, 26), (HE.COUNT_INSIDE, 41)):
        assert (hi - lo, HE.parts(hi - lo), lo & 63) == (400, 1, phase)


# ---- C ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_windows_sit_on_the_thresholds_of_the_pixel_cut():
    c, windows = HE.window_case()
    assert len(windows) == len(HE.WIN_LENGTHS) * len(HE.WIN_LOS) == 42 == len(set(windows))
    assert sorted(set(hi - lo for lo, hi in windows)) == list(HE.WIN_LENGTHS) and sorted(set(lo & 63 for lo, _ in windows)) == [0, 1, 63]
    for lo, hi in windows:
        assert HE.parts(hi - lo) == HE.WIN_PARTS[hi - lo] and HE.parts(hi - lo, split=False) == 1 and hi < HE.WIN_ROUTE
        assert -(-(hi - lo) // 256) == (1 if hi - lo <= 256 else 2)                        # trips of the j0 += 256 loop
    assert [n for n in HE.WIN_LENGTHS if HE.parts(n) != HE.parts(n + 1)] == [64, 128]
    assert HE.WIN_LENGTHS[-1] == HW.MAX_VIEWS and c["weights"][:4].tolist() == [0.0, 0.3, 1.0, 0.0]
    # the near match of the window's last view wins, at that view; the copy of the view just outside finds no equal inside
    P = HE.WIN_SHAPE[0] * HE.WIN_SHAPE[1]
    for i, (lo, hi) in enumerate(windows):
        assert np.array_equal(c["patches"][i, 0], c["views"][HE.WIN_DECOY + hi])
        assert c["win_view"][i, 2] == hi - 1 and c["win_best"][i] == 2 and c["win_fam"][i, 0] < c["win_fam"][i, 2] <= P
    assert (c["win_view"] >= np.array(windows)[:, :1]).all() and (c["win_view"] < np.array(windows)[:, 1:]).all()


# ---- D ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_tiny_views_leave_pixel_ranges_empty_and_tie():
    assert [((h * w) + 3) // 4 for h, w in HE.TINY_SHAPES] == list(HE.TINY_PW)
    assert [(hi - lo, HE.parts(hi - lo), lo & 63) for lo, hi in HE.TINY_WINDOWS] == [(1, 4, 7), (40, 4, 7), (64, 4, 7), (100, 2, 7)]
    for Pw in set(HE.TINY_PW):
        for n_parts in (4, 2):
            ranges = HE.pixel_ranges(Pw, n_parts)
            assert sum(b - a for a, b in ranges) == Pw and ranges[0][0] == 0 and ranges[-1][1] == Pw
            assert any(a == b for a, b in ranges) == (Pw < n_parts)
    assert any(a == b for a, b in HE.pixel_ranges(1, 2)) and all(Pw < 4 for Pw in HE.TINY_PW)
    # a remainder the cut must not drop: 3 dwords in 2 and in 4 parts, 2 in 4, 1 in 2
    assert HE.pixel_ranges(3, 2) == [(0, 1), (1, 3)] and HE.pixel_ranges(3, 4) == [(0, 0), (0, 1), (1, 2), (2, 3)]
    # the last column block holds three live columns
    assert [A % HE.constants()["kRvBlock"] for A in HE.TINY_A] == [3, 3, 3]
    for h, w in HE.TINY_SHAPES:
        several = 0
        for A in HE.TINY_A:
            c, windows = HE.tiny_case(h, w, A)
            assert c["first"].tolist() == [0, 3, 203] and c["patches"].shape == (4, A, h, w, 3)
            several += int((HE.candidates(c, windows) > 1).sum())
        assert several >= 1, (h, w)


# ---- G ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_many_members_take_a_second_launch_and_a_capped_slab():
    k = HE.constants()
    n, A = HE.MANY_N, HE.MANY_A
    assert n > k["rvwin_launch"] and n > k["scene_launch"] and k["rvwin_launch"] % len(HE.MANY_TABLE)
    entry = HE.many_entry()
    assert entry[[32768, 32769, 32770]].tolist() != entry[[0, 1, 2]].tolist() and entry[32768:].tolist() == [1, 2, 3]
    # 65 542 columns: three slabs by the cap, not by the score buffer
    lmax = max(HE.MANY_LENGTHS)
    assert HR.slab_columns(lmax) > k["slab_cap"]
    assert HE.slabs(n * A, lmax) == [(0, 32768), (32768, 65536), (65536, 65542)]
    # the seven entries differ, sit on all three routes, and their windows are no whole routes (but entry 0's and 4's)
    c, windows = HE.many_table()
    assert len(set(HE.MANY_TABLE)) == 7 and sorted(set(c["routes"].tolist())) == [0, 1, 2] and len(set(c["weights"].tolist())) == 3
    whole = [w == (0, HE.MANY_LENGTHS[r]) for (r, w, _) in HE.MANY_TABLE]
    assert whole == [True, False, False, False, True, False, False]
    for i in range(7):
        same = c["win_fam"][i].tobytes() == c["fam"][i].tobytes() and np.array_equal(c["win_view"][i], c["view"][i])
        assert same or not whole[i]
    assert sum(c["win_fam"][i].tobytes() != c["fam"][i].tobytes() for i in range(7)) >= 4
    assert len(set(c["fam"][i].tobytes() for i in range(7))) == 7
    for _, (lo, hi), _ in HE.MANY_TABLE:
        assert HE.parts(hi - lo) == (4 if hi - lo <= 64 else 2) and lo & 63 == lo
