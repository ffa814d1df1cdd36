"""Inputs of the route-view edge tests (tests/test_rviews_edges_host.py, tests/test_gpu_rviews_edges.py): the shapes, route lengths,
windows and runs of identical views that reach the branches of k_rv_score, k_rv_pick and k_rvwin_score which the tests of the rule
(tests/test_gpu_rviews.py, tests/test_gpu_rvwin.py) never enter, and the expected values on them.

Nothing here comes from the device.  The thresholds are read out of csrc/dejavu_rviews.inl and csrc/dejavu_rvwin.inl (`constants`)
and the host's arithmetic on them is restated (`tile_width`, `tiles`, `parts`, `slabs`), so that the CPU test can pin that every input
reaches the branch it is named for.  Expected values are oracle.step's, through helpers_rviews.expected and helpers_rvwin.expected."""
import functools
import os
import re

import numpy as np

from navsim_amd import synth
from tests import helpers_rviews as HR
from tests import helpers_rvwin as HW

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "navigation-by-deja-vu_amd", "csrc")
CYCLE = (0.0, 0.3, 1.0)                         # the weights the members of a case cycle through


# ---- the sources' constants and the host's arithmetic on them -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def constants():
    """dict of the constexpr ints named below (a product of literals is multiplied out), the 64 MiB of a slab's scores, the cap on a
    slab's columns and the members of a launch of the windowed step and of the scene call."""
    rviews = open(os.path.join(CSRC, "dejavu_rviews.inl")).read()
    rvwin = open(os.path.join(CSRC, "dejavu_rvwin.inl")).read()
    out = {}
    for name, text in (("kRvBlock", rviews), ("kRvTileMax", rviews), ("kRvLdsBytes", rviews), ("kRvCandCap", rviews), ("kRvWinCoop", rvwin)):
        expr = re.search(r"constexpr int %s = ([0-9* ]+);" % name, text).group(1)
        out[name] = int(np.prod([int(f) for f in expr.split("*")]))
    out["slab_bytes"] = int(re.search(r"std::max\(1ll, \((\d+)ll << 20\) / \(lstride \* 8\)\)", rviews).group(1)) << 20
    out["slab_cap"] = int(re.search(r"std::min\(cols, (\d+)ll\)", rviews).group(1))
    out["scene_launch"] = int(re.search(r"for \(int i0 = 0; i0 < N; i0 \+= (\d+)\)", rviews).group(1))
    out["rvwin_launch"] = int(re.search(r"for \(int i0 = 0; i0 < N; i0 \+= (\d+)\)", rvwin).group(1))
    return out


def tile_width(P):
    """rviews_plan's T: the columns of a tile whose patches (three planes of Pw dwords each) fit the LDS budget, a multiple of kRvBlock."""
    k = constants()
    Pw = (P + 3) // 4
    return min(k["kRvTileMax"], k["kRvLdsBytes"] // (3 * Pw * 4) // k["kRvBlock"] * k["kRvBlock"])


def wave_map(T):
    """k_rv_score's (column blocks, view groups of a workgroup) at tile width T."""
    ncb = T // constants()["kRvBlock"]
    return ncb, max(1, 4 // ncb)


def slabs(n_columns, lmax):
    """rviews_plan's slabs of the sorted columns: [(s0, s1)]."""
    k = constants()
    lstride = (lmax + 63) // 64 * 64
    slab = min(n_columns, min(max(1, k["slab_bytes"] // (lstride * 8)), k["slab_cap"]))
    return [(s0, min(n_columns, s0 + slab)) for s0 in range(0, n_columns, slab)]


def tiles(routes, A, T, lmax):
    """rviews_plan's tiles: (route, columns) of every tile, the members sorted by route (stable), slab by slab."""
    col_route = np.repeat(np.asarray(routes)[np.argsort(np.asarray(routes), kind="stable")], A)
    out = []
    for s0, s1 in slabs(len(col_route), lmax):
        s = s0
        while s < s1:
            e = s + 1
            while e < s1 and e - s < T and col_route[e] == col_route[s]:
                e += 1
            out.append((int(col_route[s]), e - s))
            s = e
    return out


def parts(n_views, split=True):
    """k_rvwin_score's pixel cut of a window of n_views views."""
    nch = (n_views + 63) >> 6
    return 1 if not split else 4 if nch == 1 else 2 if nch == 2 else 1


def pixel_ranges(Pw, n_parts):
    return [(p * Pw // n_parts, (p + 1) * Pw // n_parts) for p in range(n_parts)]


def candidates(case, windows=None):
    """The fast path's candidates (helpers_rviews.statement) of every column -> int[n, A]; windows: on the members' slices."""
    views, first, patches = case["views"], case["first"], case["patches"]
    n, A = patches.shape[:2]
    out = np.empty((n, A), dtype=np.int64)
    for i in range(n):
        r = case["routes"][i]
        lo, hi = (0, int(first[r + 1] - first[r])) if windows is None else windows[i]
        lib = np.ascontiguousarray(views[first[r] + lo:first[r] + hi])
        for a in range(A):
            out[i, a] = HR.statement(lib, patches[i, a:a + 1], float(case["weights"][i]))[3]
    return out


def _frozen(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _case(views, lengths, patches, routes, weights, windows=None):
    """A case in the form check_step / check_windowed take: with the whole routes' expected values, or (windows) the slices'."""
    case = dict(views=views, first=HR.first_of(lengths), patches=np.ascontiguousarray(patches),
                routes=np.array(routes, dtype=np.int32), weights=np.array(weights, dtype=np.float64))
    if windows is None:
        case["fam"], case["view"], case["best"], case["scene"] = HR.expected(views, case["first"], case["patches"], case["routes"], case["weights"])
    else:
        case["win_fam"], case["win_view"], case["win_best"] = HW.expected(case, windows)
    return _frozen(case)


# ---- A. tile widths of the unwindowed step ---------------------------------------------------------------------------------------------------
TILE_TABLE = ((32, 32, 1024, 256, 16), (25, 41, 1025, 257, 12), (31, 44, 1364, 341, 12), (36, 38, 1368, 342, 8), (45, 45, 2025, 507, 8),
              (3, 683, 2049, 513, 4))                                                       # h, w, P, Pw, T
TILE_SHAPES = tuple(t[:2] for t in TILE_TABLE[1:])
TILE_LENGTHS = (2, 65, 130, 5)                  # 65 and 130 views: 2 and 3 groups of 64; route 3 is the one no member uses
TILE_ROUTES = (2, 1, 2, 0, 1)                   # the two members of routes 1 and 2 share tiles: 14 sorted columns a route
TILE_WEIGHTS = (0.0, 0.3, 1.0, 0.3, 0.0)        # ... under different weights
TILE_A = 7
TILE_SPLITS = {16: [14], 12: [12, 2], 8: [8, 6], 4: [4, 4, 4, 2]}                          # the tiles of a route's 14 columns


def tile_case(h, w):
    return HR.step_case(h, w, TILE_A, "random", lengths=TILE_LENGTHS, routes=TILE_ROUTES, weights=TILE_WEIGHTS)


# ---- B. the list cap of k_rv_pick, E. the candidate counts of k_rvwin_score --------------------------------------------------------------------
def _run_route(n, at, k, seed):
    """(views uint8[n, 8, 8, 3] of which [at, at + k) are one view, patches uint8[2, 8, 8, 3]: heading 0 near that view, heading 1
    random) -- helpers_rvwin.identical_run with the run's place and length as arguments."""
    views = synth.random_hsv(seed, (n, 8, 8, 3))
    views[at:at + k] = synth.random_hsv(seed + 1, (8, 8, 3))
    return views, np.stack([synth.near_match_patch(views[at], 5), synth.random_hsv(seed + 2, (8, 8, 3))])


PICK_RUNS = (256, 257)                          # kRvCandCap: the list is full; one more: the exact-all pass
PICK_AT, PICK_ROUTE = 20, 300


@functools.lru_cache(maxsize=None)
def pick_case(k):
    """Three members (weights 0.3, 0.0, 1.0) on a route of 300 views behind a 5-view decoy; views [20, 20 + k) are one view."""
    views, patches = _run_route(PICK_ROUTE, PICK_AT, k, 41)
    store = np.concatenate([synth.random_hsv(9, (5, 8, 8, 3)), views])
    return _case(store, (5, PICK_ROUTE), np.stack([patches] * 3), (1, 1, 1), (0.3, 0.0, 1.0))


@functools.lru_cache(maxsize=None)
def permuted_case(seed=3):
    """helpers_rviews.permuted_route with kRvCandCap views: every view is a candidate of heading 0, and the list is full."""
    views, patch = HR.permuted_route(8, 8, 256, seed)
    store = np.concatenate([synth.random_hsv(9, (4, 8, 8, 3)), views])
    return _case(store, (4, 256), np.stack([np.stack([patch, views[5]])] * 3), (1, 1, 1), (0.3, 0.0, 1.0))


COUNT_RUNS = (16, 17, 256, 257)                 # kRvWinCoop and one more, kRvCandCap and one more
COUNT_AT, COUNT_ROUTE = 100, 520
COUNT_WINDOW, COUNT_INSIDE = (90, 490), (105, 505)


@functools.lru_cache(maxsize=None)
def count_case(k, window=COUNT_WINDOW):
    """(case, windows): three members (weights 0.3, 0.0, 1.0) under one window of a route of 520 views (behind a 5-view decoy) whose
    views [100, 100 + k) are one view."""
    views, patches = _run_route(COUNT_ROUTE, COUNT_AT, k, 51)
    store = np.concatenate([synth.random_hsv(9, (5, 8, 8, 3)), views])
    windows = (window,) * 3
    return _case(store, (5, COUNT_ROUTE), np.stack([patches] * 3), (1, 1, 1), (0.3, 0.0, 1.0), windows), windows


# ---- C. window lengths -----------------------------------------------------------------------------------------------------------------------
WIN_LENGTHS = (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512)
WIN_LOS = (0, 1, 63)
WIN_PARTS = {63: 4, 64: 4, 65: 2, 127: 2, 128: 2, 129: 1, 191: 1, 192: 1, 193: 1, 255: 1, 256: 1, 257: 1, 511: 1, 512: 1}
WIN_ROUTE, WIN_DECOY, WIN_SHAPE, WIN_A = 1100, 3, (19, 17), 5


@functools.lru_cache(maxsize=None)
def window_case():
    """(case, windows): a member per (lo, length) on one route of 1 100 "levels" views behind a 3-view decoy.  Heading 2 of a member is
    a near match of the LAST view of its window, heading 0 an exact copy of the view just outside it."""
    h, w = WIN_SHAPE
    windows = tuple(dict.fromkeys((lo, lo + n) for n in WIN_LENGTHS for lo in WIN_LOS))
    views = synth.synth_views(1500, WIN_DECOY + WIN_ROUTE, h, w)
    n = len(windows)
    patches = synth.synth_views(2500, n * WIN_A, h, w).reshape(n, WIN_A, h, w, 3).copy()
    for i, (lo, hi) in enumerate(windows):
        patches[i, 2] = synth.near_match_patch(views[WIN_DECOY + hi - 1], 31 + i)
        patches[i, 0] = views[WIN_DECOY + hi]
    case = _case(views, (WIN_DECOY, WIN_ROUTE), patches, (1,) * n, tuple(CYCLE[i % 3] for i in range(n)), windows)
    return case, windows


# ---- D. tiny views ---------------------------------------------------------------------------------------------------------------------------
TINY_SHAPES = ((1, 1), (1, 2), (1, 3), (2, 2), (1, 5), (3, 3), (2, 6))
TINY_PW = (1, 1, 1, 1, 2, 3, 3)
TINY_A = (3, 7, 11)                             # column blocks of 3, 4 + 3 and 4 + 4 + 3 live columns
TINY_WINDOWS = ((7, 8), (7, 47), (7, 71), (7, 107))                                       # 1, 40 and 64 views (4 parts), 100 (2 parts)
TINY_ROUTE, TINY_DECOY = 200, 3
# The views' seeds, a shape each.  Random views of a few pixels tie exactly now and then, not always: these are the first seeds from
# 3000 on under which some column of the shape has more than one candidate (pinned by the host test).
TINY_SEEDS = {(1, 1): 3000, (1, 2): 3000, (1, 3): 3001, (2, 2): 3000, (1, 5): 3005, (3, 3): 3004, (2, 6): 3000}


@functools.lru_cache(maxsize=None)
def tiny_case(h, w, A):
    """(case, windows): a member per window of TINY_WINDOWS on a route of 200 "random" views behind a 3-view decoy."""
    views = synth.random_hsv(TINY_SEEDS[(h, w)], (TINY_DECOY + TINY_ROUTE, h, w, 3))
    n = len(TINY_WINDOWS)
    patches = synth.random_hsv(4000 + 16 * h + w + 256 * A, (n, A, h, w, 3))
    case = _case(views, (TINY_DECOY, TINY_ROUTE), patches, (1,) * n, tuple(CYCLE[i % 3] for i in range(n)), TINY_WINDOWS)
    return case, TINY_WINDOWS


# ---- G. more members than one launch takes ------------------------------------------------------------------------------------------------------
MANY_N, MANY_A, MANY_SHAPE = 32771, 2, (2, 2)
MANY_LENGTHS = (5, 70, 9)
MANY_TABLE = ((1, (0, 70), 0.3), (0, (0, 3), 0.0), (2, (4, 9), 1.0), (1, (30, 68), 0.0), (0, (0, 5), 0.3), (1, (60, 70), 1.0),
              (2, (0, 1), 0.3))                                                            # route, window, weight


@functools.lru_cache(maxsize=None)
def many_table():
    """The case of the seven entries (a member each), with the whole routes' and the windows' expected values, and the windows."""
    h, w = MANY_SHAPE
    views = synth.random_hsv(61, (sum(MANY_LENGTHS), h, w, 3))
    patches = synth.random_hsv(62, (len(MANY_TABLE), MANY_A, h, w, 3))
    routes, windows, weights = zip(*MANY_TABLE)
    whole = _case(views, MANY_LENGTHS, patches, routes, weights)
    win = _case(views, MANY_LENGTHS, patches, routes, weights, windows)
    return dict(whole, **{k: win[k] for k in ("win_fam", "win_view", "win_best")}), windows


def many_entry(n=MANY_N):
    """The table entry of every member: member i takes entry i % 7."""
    return np.arange(n) % len(MANY_TABLE)
