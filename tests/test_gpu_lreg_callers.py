"""The register-ring fp4 bodies (Body::LcRegCode8 forced with DEJAVU_LREG8=1, Body::LcRegCode with DEJAVU_LREG8=0, Body::LcReg with
DEJAVU_VCODE=0) under everything their callers send them that three random-heading files (test_gpu_libreg.py,
test_gpu_libreg_code.py, test_gpu_lreg8.py) do not: ties inside an item and across workgroups (fused_finish's lane-half, wave and
running-summary merges, its queue and the shared list's overflow), passes of several agents with and without weights, a second
heading tile as a pass of its own (a_off > 0), eight headings and one (APAD 8), the wide step, a grown library and first_view.

Every expectation is the CPU oracle's (oracle.sads_hsv rows, the reference's decision rule on them); the LDS-ring engine
(DEJAVU_VCODE=0, DEJAVU_LIBREG=0) is the bit-for-bit witness of the integer sums; scoring_form() must name the body a case is about
after every call.  tests/helpers_lreg.py:place only chooses where views are planted (layout of the eight-wave body: items of 16
view groups, waves 0-7; the same views tie across other waves and items in the four-consumer bodies).
"""
import numpy as np
import pytest

from navsim_amd import synth
from tests.helpers_lreg import (GROUPS_EIGHT_WAVES, GROUPS_FOUR_CONSUMERS, UNDER_TEST, assert_form, clear_headings, engine, fresh_view,
                                oracle_rows, place, step_of_rows, tied_pair)

pytestmark = pytest.mark.gpu

RTOL = 1e-9
F, H, W = 7000 + 19, 32, 32                   # 14 items of 15 or 16 view groups on 14 workgroups (eight waves); NK = 8 + 16
_STORED = 3000                                # a view of the library no case overwrites
_CACHE = {}


def _once(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def _lib0():
    return _once("lib0", lambda: synth.synth_views(91 + F, F, H, W))


def _pool():
    """96 random headings every case draws from (the oracle scores each against a library once)."""
    return _once("pool", lambda: synth.synth_patches(300 + 96, 96, H, W))


def _where(view):
    item, _, _, wave, t, half, _ = place(F, view, GROUPS_EIGHT_WAVES)
    return item, wave, t, half


# Copies of fresh views, lowest index first.  Item 1 holds view groups 15-30 (16 of them: waves 0-7 all live).
_G1 = 15 * 32
DUPS = {
    "lane_halves": (_G1 + 2 * 32 + 9, _G1 + 2 * 32 + 13),          # v and v + 4 of one view group: the two halves of a lane pair
    "t0_t1": (_G1 + 4 * 32 + 20, _G1 + 5 * 32 + 3),                # the two view groups of wave 2
    "waves_3_4": (_G1 + 7 * 32 + 30, _G1 + 8 * 32 + 1),            # rows 3 and 4 of sum_sc / sum_view
    "wave_7": (_G1 + 14 * 32 + 17, _G1 + 15 * 32 + 6),             # both view groups of the last wave
    "two_items": (_G1 + 10 * 32 + 11, 94 * 32 + 3 * 32 + 2),       # items 1 and 6: two workgroups, settled by k_fold
    "waves_0_1": (_G1 + 1 * 32 + 25, _G1 + 3 * 32 + 4),            # two waves of one item in the four-consumer bodies as well
}
_DUP_ORDER = list(DUPS)


def test_planted_views_are_where_the_cases_say():
    assert _where(DUPS["lane_halves"][0])[:3] == _where(DUPS["lane_halves"][1])[:3] == (1, 1, 0)
    assert (_where(DUPS["lane_halves"][0])[3], _where(DUPS["lane_halves"][1])[3]) == (0, 1)
    assert (_where(DUPS["t0_t1"][0])[:3], _where(DUPS["t0_t1"][1])[:3]) == ((1, 2, 0), (1, 2, 1))
    assert (_where(DUPS["waves_3_4"][0])[:3], _where(DUPS["waves_3_4"][1])[:3]) == ((1, 3, 1), (1, 4, 0))
    assert (_where(DUPS["wave_7"][0])[:3], _where(DUPS["wave_7"][1])[:3]) == ((1, 7, 0), (1, 7, 1))
    assert (_where(DUPS["two_items"][0])[:2], _where(DUPS["two_items"][1])[:2]) == ((1, 5), (6, 1))
    assert (_where(DUPS["waves_0_1"][0])[:3], _where(DUPS["waves_0_1"][1])[:3]) == ((1, 0, 1), (1, 1, 1))
    assert all(v[0] < v[1] for v in DUPS.values()) and _STORED not in sum(DUPS.values(), ())
    # the four-consumer bodies cut items of 8 view groups: the same copies are one lane pair, one wave's two view groups (t0_t1,
    # wave_7), two waves of one item (waves_0_1) and two items (waves_3_4, two_items) there
    four = {name: [place(F, v, GROUPS_FOUR_CONSUMERS)[:5:3] + place(F, v, GROUPS_FOUR_CONSUMERS)[4:5] for v in vs] for name, vs in DUPS.items()}
    assert four["lane_halves"] == [(2, 1, 0), (2, 1, 0)] and four["t0_t1"] == [(2, 2, 0), (2, 2, 1)] and four["wave_7"] == [(3, 3, 0), (3, 3, 1)]
    assert four["waves_0_1"] == [(2, 0, 1), (2, 1, 1)] and four["waves_3_4"] == [(2, 3, 1), (3, 0, 0)] and four["two_items"][1][0] == 12


def _lib_dups():
    def make():
        lib = _lib0().copy()
        for i, name in enumerate(_DUP_ORDER):
            for v in DUPS[name]:
                lib[v] = fresh_view(i)
        return lib
    return _once("lib_dups", make)


def _x(name):
    return fresh_view(_DUP_ORDER.index(name))


class _Pair:
    """The engine under test and the LDS-ring witness on one library."""

    def __init__(self, kind, lib, cw, first_view=0, second_tile_as_pass=False, one_chunk=True, weight_range=None):
        self.kind, self.first_view = kind, first_view
        self.engines = [engine(kind, one_chunk, second_tile_as_pass), engine("lds_ring", one_chunk, second_tile_as_pass)]
        for e in self.engines:
            if weight_range is not None:
                e.set_weight_range(*weight_range)
            if lib is not None:
                e.set_library(lib, cw, first_view=first_view)
        self.e, self.lds = self.engines

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for e in self.engines:
            e.close()

    def form(self, fused, fp4=True):
        return assert_form(self.e, self.kind, fused, fp4)


def _same_record(got, ref, what):
    assert (got["best_idex"], got["best_view"]) == (ref["best_idex"], ref["best_view"]), what
    assert np.array_equal(got["angle_familiarity"], ref["angle_familiarity"]), what
    assert np.array_equal(got["angle_view"], ref["angle_view"]), what


def _check_record(got, rows, what, tied=(), first_view=0, every_view=True):
    """One step's (or agent's) record against the oracle's rows of its headings: oracle.step's decision and familiarities, and each
    heading's first best view.  every_view=False (chem_weight 1.0 alone: value differences vanish and random headings meet equal
    integer sums, which the oracle's sequential doubles need not order by index): the views of the headings the oracle settles."""
    want = step_of_rows(rows)
    assert got["best_idex"] == want["best_idex"], (what, got["flags"], got["n_candidates"] if "n_candidates" in got else None)
    assert got["best_view"] == want["best_view"] + first_view, what
    np.testing.assert_allclose(got["angle_familiarity"], want["angle_familiarity"], rtol=RTOL, err_msg=str(what))
    sel = clear_headings(rows, tied)
    assert sel.all() or not every_view, what                # the oracle settles every heading's view: none is left out
    assert np.array_equal(np.asarray(got["angle_view"])[sel], want["angle_view"][sel] + first_view), what
    return want


def _check_ties(got, rows, want, what):
    """A step whose best is tied: the exact resolver settled it, and it saw at least the pairs the oracle has within the window."""
    assert got["flags"] & 1, (what, got["flags"])
    n_within = int((rows >= want["step_familiarity"] - got["delta"]).sum())
    assert 2 <= n_within <= 64, (what, n_within)           # (the resolver's business, not the overflow path's)
    assert got["n_candidates"] >= n_within, (what, got["n_candidates"], n_within)


# ------------------------------------------------------------------ a, i. duplicates and first-view rules
def _near(name, seed=7):
    """The copies' view with 3 % of its pixels replaced: every copy scores alike against it, some 15 below h * w."""
    return synth.near_match_patch(_x(name), seed, fraction=0.03)


def _duplicate_steps(A):
    """(name, patches, tied headings, best heading, best view, whether the step's best is tied) of every step of case a."""
    base = _pool()[:A]
    for name in _DUP_ORDER:
        lowest = DUPS[name][0]
        one = base.copy()
        one[A // 3] = _x(name)
        yield name + "/one heading", one, (A // 3,), A // 3, lowest, True
        if A >= 8:
            two = base.copy()
            two[1] = two[A - 2] = _x(name)
            yield name + "/two headings", two, (1, A - 2), 1, lowest, True
            # the tie is not the step's best: no resolver looks at it, the summaries alone must name the first view
            beside = base.copy()
            beside[A // 3], beside[A - 3] = _lib_dups()[_STORED], _near(name)
            yield name + "/beside the best", beside, (A - 3,), A // 3, _STORED, False
        if A > 1:
            every = np.repeat(_x(name)[None], A, axis=0)
            yield name + "/every heading", every, tuple(range(A)), 0, lowest, True


def _run_duplicates(kind, cw, first_view):
    lib = _lib_dups()
    with _Pair(kind, lib, cw, first_view) as p:
        assert (p.e.library_info()["code_tile_bytes"] > 0) == (kind != "thermometer_ring")
        for A in (1, 8, 13, 32):                                        # 1 and 8: APAD 8
            for name, pats, tied, best, view, best_tied in _duplicate_steps(A):
                what = (kind, cw, A, name)
                lowest = DUPS[name.split("/")[0]][0]
                rows = oracle_rows("dups", lib, pats, cw)
                got = p.e.step(pats, want_scene=False)
                p.form(fused=True)
                want = _check_record(got, rows, what, tied, first_view)
                assert (want["best_idex"], want["best_view"]) == (best, view) and got["best_view"] == view + first_view, what
                assert all(want["angle_view"][a] == lowest and got["angle_view"][a] == lowest + first_view for a in tied), what
                assert got["step_familiarity"] == H * W, what
                if best_tied:
                    _check_ties(got, rows, want, what)
                else:
                    assert not got["flags"] & 1 and all(want["angle_familiarity"][a] < H * W - 5 for a in tied), (what, got["flags"])
                _same_record(got, p.lds.step(pats, want_scene=False), what)
            # and the unfused form of the same body: every view's sum, stored
            pats = _pool()[:A].copy()
            pats[A // 3] = _x("waves_3_4")
            rows = oracle_rows("dups", lib, pats, cw)
            got = p.e.step(pats, want_scene=True)
            p.form(fused=False)
            _check_record(got, rows, (kind, cw, A, "scene"), (A // 3,), first_view)
            np.testing.assert_allclose(got["scene_familiarity"], rows.min(axis=0), rtol=RTOL)
            assert np.array_equal(got["scene_familiarity"], p.lds.step(pats, want_scene=True)["scene_familiarity"])


@pytest.mark.parametrize("cw", [0.25, 0.5])
@pytest.mark.parametrize("kind", UNDER_TEST)
def test_duplicates_report_the_first_view(kind, cw):
    """Copies of a view whose lowest index is not the first one the hardware meets: the other lane half, the wave's other view
    group, waves 3 and 4, wave 7, another workgroup; seen by one heading, by two (the first wins) and by every heading."""
    _run_duplicates(kind, cw, 0)


@pytest.mark.parametrize("kind", UNDER_TEST)
def test_duplicates_with_a_first_view(kind):
    """The same steps on a library whose view 0 is global view 1000: every reported view is first_view + local (dejavu.h)."""
    _run_duplicates(kind, 0.25, 1000)


# ------------------------------------------------------------------ b. equal scores from different sums
_PAIR_AT = (_G1 + 4 * 32 + 5, _G1 + 12 * 32 + 9)          # waves 2 and 6 of item 1


@pytest.mark.parametrize("z_first", [True, False])
@pytest.mark.parametrize("kind", UNDER_TEST)
def test_equal_scores_from_different_sums(kind, z_first):
    """Y (S_hs 254) and Z (S_v 127) score alike against X at chem_weight 0.5 and 0.249 apart at 0.25 (the control)."""
    assert (_where(_PAIR_AT[0])[:2], _where(_PAIR_AT[1])[:2]) == ((1, 2), (1, 6))
    x = fresh_view(20)
    y, z = tied_pair(x)
    lib = _lib0().copy()
    lib[_PAIR_AT[0]], lib[_PAIR_AT[1]] = (z, y) if z_first else (y, z)
    A = 13
    pats = _pool()[:A].copy()
    pats[A // 3] = x
    for cw in (0.5, 0.25):
        what = (kind, z_first, cw)
        rows = oracle_rows("pair%d" % z_first, lib, pats, cw)
        tie = rows[A // 3, _PAIR_AT[0]] == rows[A // 3, _PAIR_AT[1]]
        assert tie == (cw == 0.5), what
        with _Pair(kind, lib, cw) as p:
            got = p.e.step(pats, want_scene=False)
            p.form(fused=True)
            want = _check_record(got, rows, what, (A // 3,))
            assert want["best_idex"] == A // 3
            if cw == 0.5:
                assert got["best_view"] == _PAIR_AT[0] and got["flags"] & 1, (what, got["flags"])
                _check_ties(got, rows, want, what)
            else:                                                       # Y is the nearer at 0.25, wherever it is
                assert got["best_view"] == (_PAIR_AT[1] if z_first else _PAIR_AT[0]), what
            _same_record(got, p.lds.step(pats, want_scene=False), what)


# ------------------------------------------------------------------ c. queue and list overflow
@pytest.mark.parametrize("kind", UNDER_TEST)
def test_queue_and_list_overflow(kind):
    """400 copies of one view inside item 1 (512 views): one heading leaves 399 entries for the 256-entry LDS queue, 16 headings 6400
    pairs for the 4096-entry shared list."""
    cw = 0.25
    x = fresh_view(30)
    lib = _lib0().copy()
    lib[_G1:_G1 + 400] = x
    assert _where(_G1)[0] == _where(_G1 + 399)[0] == 1
    with _Pair(kind, lib, cw) as p:
        for A in (1, 16):
            what = (kind, A)
            pats = np.repeat(x[None], A, axis=0)
            rows = oracle_rows("copies", lib, pats, cw)
            got = p.e.step(pats, want_scene=False)
            p.form(fused=True)
            want = _check_record(got, rows, what, tuple(range(A)))
            assert (got["best_idex"], got["best_view"], got["step_familiarity"]) == (0, _G1, H * W), what
            assert got["flags"] & 3, (what, got["flags"])               # exact values decided
            if A == 1:
                assert got["n_candidates"] >= 400, (what, got["n_candidates"])
            else:
                assert got["n_candidates"] > 4096 or got["flags"] & 4, (what, got["n_candidates"], got["flags"])
            _same_record(got, p.lds.step(pats, want_scene=False), what)
        # the engine scores plain headings as before after the redo
        pats = _pool()[:13].copy()
        pats[4] = lib[_STORED]
        got = p.e.step(pats, want_scene=False)
        p.form(fused=True)
        _check_record(got, oracle_rows("copies", lib, pats, cw), (kind, "after"))
        assert (got["best_idex"], got["best_view"]) == (4, _STORED)


# ------------------------------------------------------------------ d. the workgroup's running summary, on a grown library
_FG, _NAPP, _SEED_D = 130900, 1600, 4242                    # generated on the device, then appended: 132 500 views, 259 items of 16 groups
_FD = _FG + _NAPP


@pytest.mark.parametrize("kind", UNDER_TEST)
def test_running_summary_of_a_workgroup_with_two_items(kind):
    """Workgroup 0 of the eight-wave body takes items 0 and 256.  X, generated view 100 (item 0), is copied into items 256, 257 and
    the last, partial item: the first item wins and the loser is listed.  U exists in item 256 only: the second item wins.  T is in
    items 256, 257 and the last real view group.  An exact copy scores h * w and nothing else can, so the lowest copy is the answer;
    the rest is held to the LDS-ring engine on the same generated-and-appended library."""
    cw, A = 0.25, 13
    c256, c257, c_last = 131008 + 5 * 32 + 7, 131520 + 9 * 32 + 30, _FD - 3
    u256 = 131008 + 11 * 32 + 2
    t256, t257, t_last = 131008 + 15 * 32 + 31, 131520 + 0 * 32 + 0, _FD - 20
    pl = lambda v: place(_FD, v, GROUPS_EIGHT_WAVES)
    assert (pl(100)[0], pl(100)[6]) == (0, 0) and pl(_FD - 1)[1] == 259
    assert [pl(v)[0] for v in (c256, c257, c_last)] == [256, 257, 258] and pl(c256)[6] == 0
    assert (pl(u256)[0], pl(u256)[6]) == (256, 0) and [pl(v)[0] for v in (t256, t257, t_last)] == [256, 257, 258]
    assert t_last // 32 == (_FD - 1) // 32 and _FD % 32 != 0 and _FG < 131008      # the last real view group, partial; all appended
    x = synth.synth_views(_SEED_D, 1, H, W, first_view=100)[0]
    u, t = fresh_view(40), fresh_view(41)
    more = synth.synth_views(_SEED_D, _NAPP, H, W, first_view=_FG)
    for v in (c256, c257, c_last):
        more[v - _FG] = x
    more[u256 - _FG] = u
    for v in (t256, t257, t_last):
        more[v - _FG] = t
    base = synth.synth_patches(_SEED_D, A, H, W)
    steps = []
    near = {1: (synth.near_match_patch(x, 3, fraction=0.03), 100), 12: (synth.near_match_patch(t, 4, fraction=0.03), t256)}
    for name, plant, beside in (("first item wins", {4: (x, 100)}, {}), ("second item wins", {6: (u, u256)}, {}),
                                ("later items", {2: (t, t256)}, {}), ("all three", {9: (x, 100), 3: (u, u256), 11: (t, t256)}, {}),
                                # ties that no resolver looks at: workgroup 0's two items (X) and three workgroups (T) name the first view
                                ("ties beside the best", {6: (u, u256)}, near)):
        pats = base.copy()
        for a, (patch, _) in list(plant.items()) + list(beside.items()):
            pats[a] = patch
        steps.append((name, pats, {a: v for a, (_, v) in plant.items()}, {a: v for a, (_, v) in beside.items()}))
    with _Pair(kind, None, cw, one_chunk=False) as p:
        for e in p.engines:
            e.generate_library(_SEED_D, _FG, H, W, cw)
            e.append_library(more)
            info = e.library_info()
            assert info["n_views"] == _FD == e.n_views, info
        assert (p.e.library_info()["code_tile_bytes"] > 0) == (kind != "thermometer_ring")
        for name, pats, planted, beside in steps:
            what = (kind, name)
            got = p.e.step(pats, want_scene=False)
            p.form(fused=True)
            first = min(planted)
            assert (got["best_idex"], got["best_view"], got["step_familiarity"]) == (first, planted[first], H * W), (what, got["flags"])
            for a, v in planted.items():
                assert got["angle_view"][a] == v and got["angle_familiarity"][a] == H * W, (what, a)
            for a, v in beside.items():
                assert got["angle_view"][a] == v and H * W - 40 < got["angle_familiarity"][a] < H * W - 5, (what, a, got["angle_view"][a])
            if len(planted) == 1 and u256 in planted.values():
                assert not got["flags"] & 1, (what, got["flags"])
            else:
                assert got["flags"] & 1, (what, got["flags"])
                assert got["n_candidates"] >= sum(4 if v == 100 else (1 if v == u256 else 3) for v in planted.values()), what
            _same_record(got, p.lds.step(pats, want_scene=False), what)
        # the stored sums of the grown library (the unfused form), bit for bit, and sampled against the oracle
        got = p.e.step(steps[3][1], want_scene=True)
        p.form(fused=False)
        ref = p.lds.step(steps[3][1], want_scene=True)
        _same_record(got, ref, (kind, "scene"))
        assert np.array_equal(got["scene_familiarity"], ref["scene_familiarity"])
        rows = oracle_rows("grown_tail", more, steps[3][1], cw)
        np.testing.assert_allclose(got["scene_familiarity"][_FG:], rows.min(axis=0), rtol=RTOL)


# ------------------------------------------------------------------ e. passes of several agents
def _agent_patches(n, A, off_level=False):
    """patches[n, A] out of the pool and what is planted: {agent: (tied headings, best heading, best view)}.  Every planted agent's
    best is tied, but agent 0's among more than two agents (a stored view alone)."""
    pats = _pool()[:n * A].reshape(n, A, H, W, 3).copy()
    dup, every = _x("waves_3_4"), _x("two_items")
    stored = _lib_dups()[_STORED]
    planted = {}
    pats[0, 5] = _near("t0_t1")                                         # a tie beside agent 0's best: the summaries alone name its view
    if n == 1:
        pats[0, 2], pats[0, A - 1] = stored, dup
        planted[0] = ((5, A - 1), 2, _STORED)
    else:
        a_dup, a_every = (0, 1) if n == 2 else (n - 2, n - 1)
        pats[0, 2] = stored
        pats[a_dup, A - 1] = dup
        pats[a_every, :] = every
        planted[0] = ((5, A - 1) if n == 2 else (5,), 2, _STORED)
        if n > 2:
            planted[a_dup] = ((A - 1,), A - 1, DUPS["waves_3_4"][0])
        planted[a_every] = (tuple(range(A)), 1 if off_level else 0, DUPS["two_items"][0])
    if off_level:                                                       # heading 0 of the last agent: both copies lose the same there
        levels = sorted(int(v) for v in synth.V_LEVELS)
        pats[n - 1, 0, 1, 1, 2] = (levels[1] + levels[2]) // 2          # strictly between two value levels: no fp4 coefficient
        assert levels[1] < pats[n - 1, 0, 1, 1, 2] < levels[2]
    return pats, planted


AGENT_SHAPES = [(2, 16), (3, 10), (2, 13), (6, 16), (1, 32)]       # (6, 16): a 64-heading pass on the two-tile body, then 32 here


@pytest.mark.parametrize("n,A", AGENT_SHAPES)
@pytest.mark.parametrize("kind", UNDER_TEST)
def test_passes_of_several_agents(kind, n, A):
    cw = 0.25
    lib = _lib_dups()
    with _Pair(kind, lib, cw) as p:
        for off_level in (False, True):
            pats, planted = _agent_patches(n, A, off_level)
            got = p.e.step_batch(pats)
            p.form(fused=True, fp4=not off_level)
            scene = p.e.step_batch_scene(pats)
            p.form(fused=False, fp4=not off_level)
            ref_scene = p.lds.step_batch_scene(pats)
            assert len(got) == len(scene) == n and scene.scene_familiarity.shape == (n, F)
            for i in range(n):
                what = (kind, n, A, off_level, i)
                rows = oracle_rows("dups", lib, pats[i], cw)
                tied, best, view = planted.get(i, ((), None, None))
                for rec in (got[i], scene[i]):
                    want = _check_record(rec, rows, what, tied)
                    if best is not None:
                        assert (rec["best_idex"], rec["best_view"]) == (best, view), what
                        if i == 0:
                            assert rec["angle_view"][5] == want["angle_view"][5] == DUPS["t0_t1"][0], what
                        if i != 0 or n <= 2:
                            _check_ties(rec, rows, want, what)
                    _same_record(rec, got[i], what)
                one = p.e.step(pats[i], want_scene=False)
                _same_record(got[i], one, what)
                np.testing.assert_allclose(scene.scene_familiarity[i], rows.min(axis=0), rtol=RTOL, err_msg=str(what))
                assert np.array_equal(scene.scene_familiarity[i], ref_scene.scene_familiarity[i]), what
                _same_record(scene[i], ref_scene[i], what)


# ------------------------------------------------------------------ f. per-agent weights
@pytest.mark.parametrize("kind", UNDER_TEST)
def test_agents_under_their_own_weights(kind):
    """Three agents x 10 headings under chem_weight 0.0, 0.5 and 1.0 in one pass, on a layout for every weight in [0, 1]."""
    lib, A = _lib_dups(), 10
    weights = [0.0, 0.5, 1.0]
    pats = _pool()[:3 * A].reshape(3, A, H, W, 3).copy()
    planted = {0: (3, _STORED), 1: (7, DUPS["wave_7"][0]), 2: (5, _STORED + 1)}
    pats[0, 3], pats[1, 7], pats[2, 5] = lib[_STORED], _x("wave_7"), lib[_STORED + 1]
    with _Pair(kind, lib, 0.5, weight_range=(0.0, 1.0)) as p:
        got = p.e.step_batch(pats, chem_weights=weights)
        p.form(fused=True)
        ref = p.lds.step_batch(pats, chem_weights=weights)
        for i, w in enumerate(weights):
            what = (kind, i, w)
            rows = oracle_rows("dups", lib, pats[i], w)
            n_within = int((rows >= rows.max() - got[i]["delta"]).sum())
            assert n_within <= 64, (what, n_within)                     # weight 1.0 hides every value difference: still few ties
            _check_record(got[i], rows, what, (planted[i][0],), every_view=w < 1.0)     # (all views: the LDS-ring engine's, below)
            assert (got[i]["best_idex"], got[i]["best_view"]) == planted[i], what
            _same_record(got[i], ref[i], what)
        # the same agent on a library ingested at its weight alone, where that layout takes the body (0.0 and 1.0 have no code tiles)
        p.e.set_weight_range(1.0, 0.0)
        p.e.set_library(lib, 0.5)
        one = p.e.step(pats[1], want_scene=False)
        p.form(fused=True)
        _same_record(got[1], one, (kind, "ingested at 0.5"))


# ------------------------------------------------------------------ g. the second heading tile as a pass of its own
@pytest.mark.parametrize("kind", UNDER_TEST)
def test_second_heading_tile_as_a_launch_of_its_own(kind):
    """DEJAVU_HT=1: 64 resident headings are two launches of the one-tile body, the second with a_off = 32."""
    cw = 0.25
    lib = _lib_dups()
    with _Pair(kind, lib, cw, second_tile_as_pass=True) as p:
        # one step of 64 headings: a best view for a heading of tile 1; a duplicate pair seen by one heading of each tile
        for name, plant, tied in (("tile 1 wins", {40: lib[_STORED], 12: _near("lane_halves"), 45: _near("wave_7")}, (12, 45)),
                                  ("a pair in both tiles", {5: _x("waves_3_4"), 50: _x("waves_3_4")}, (5, 50))):
            pats = _pool()[:64].copy()
            for a, patch in plant.items():
                pats[a] = patch
            rows = oracle_rows("dups", lib, pats, cw)
            got = p.e.step(pats, want_scene=False)
            p.form(fused=True)
            want = _check_record(got, rows, (kind, name), tied)
            if 40 in plant:                                             # ties beside the best, one in each tile: no resolver
                assert (want["best_idex"], want["best_view"]) == (40, _STORED) and not got["flags"] & 1, (name, got["flags"])
                assert (got["angle_view"][12], got["angle_view"][45]) == (DUPS["lane_halves"][0], DUPS["wave_7"][0]), name
            else:
                assert want["best_idex"] == 5 and got["best_view"] == DUPS["waves_3_4"][0] == got["angle_view"][50], name
                _check_ties(got, rows, want, (kind, name))
            _same_record(got, p.lds.step(pats, want_scene=False), (kind, name))
        # 6 agents x 10 (A_real 60; agent 3 holds headings 30-39: both tiles) and 4 x 16
        for n, A, a_every, a_dup in ((6, 10, 3, 5), (4, 16, 3, 2)):
            pats = _pool()[:n * A].reshape(n, A, H, W, 3).copy()
            pats[0, 2] = lib[_STORED]
            pats[a_every, :] = _x("two_items")
            # (a_dup: headings of tile 1; the two view groups of wave 2 are one item's in the four-consumer bodies too)
            pats[a_dup, 7], pats[a_dup, 2] = _x("t0_t1"), _near("wave_7")
            planted = {0: ((), 2, _STORED), a_every: (tuple(range(A)), 0, DUPS["two_items"][0]), a_dup: ((7, 2), 7, DUPS["t0_t1"][0])}
            got = p.e.step_batch(pats)
            p.form(fused=True)
            ref = p.lds.step_batch(pats)
            for i in range(n):
                what = (kind, n, A, i)
                tied, best, view = planted.get(i, ((), None, None))
                rows = oracle_rows("dups", lib, pats[i], cw)
                want = _check_record(got[i], rows, what, tied)
                if best is not None:
                    assert (got[i]["best_idex"], got[i]["best_view"]) == (best, view), what
                if i == a_dup:
                    assert got[i]["angle_view"][2] == want["angle_view"][2] == DUPS["wave_7"][0], what
                if i in (a_dup, a_every):
                    _check_ties(got[i], rows, want, what)
                _same_record(got[i], ref[i], what)


# ------------------------------------------------------------------ h. the wide step
@pytest.mark.parametrize("A", [77, 64 + 32])
@pytest.mark.parametrize("kind", UNDER_TEST)
def test_wide_step_ends_in_a_short_pass(kind, A):
    """More than 64 headings: a 64-heading pass on the two-tile body, then 13 or 32 headings on the body under test, enqueued back to
    back with result records of their own."""
    cw = 0.25
    lib = _lib_dups()
    late = 64 + (A - 64) // 2
    with _Pair(kind, lib, cw) as p:
        for name, plant in (("best in the last pass", (late,)), ("tied across the passes", (10, late))):
            pats = _pool()[:A].copy()
            for a in plant:
                pats[a] = lib[_STORED]
            rows = oracle_rows("dups", lib, pats, cw)
            for want_scene in (False, True):
                what = (kind, A, name, want_scene)
                got = p.e.step(pats, want_scene=want_scene)
                p.form(fused=None if want_scene else True)
                want = _check_record(got, rows, what)
                assert (want["best_idex"], want["best_view"]) == (plant[0], _STORED), what
                assert got["step_familiarity"] == H * W and got["n_passes"] == 2 and got["n_contending"] == len(plant), (what, got)
                ref = p.lds.step(pats, want_scene=want_scene)
                _same_record(got, ref, what)
                if want_scene:
                    np.testing.assert_allclose(got["scene_familiarity"], rows.min(axis=0), rtol=RTOL)
                    assert np.array_equal(got["scene_familiarity"], ref["scene_familiarity"]), what
