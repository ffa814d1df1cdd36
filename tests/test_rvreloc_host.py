"""Re-localisation inside the windowed step, what needs no GPU: the binding surface of dv_rvreloc_*, the Python-side checks (made before
any library call), SadsRouteEnsemble's routing, scene mask and bookkeeping on a fake engine (tests/helpers_rvreloc.py), the device's
plan restated in NumPy against rviews_plan's tiles, and the facts about the GPU tests' inputs that keep them from being vacuous."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import sads_familiarity
from tests import helpers_rviews_edges as HE
from tests import helpers_rvreloc as H
from tests import helpers_rvwin as HW

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = navsim_amd.SadsRouteEnsemble


# ---- bindings ----------------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_engine_agree_on_the_relocalising_calls():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    declared = set(re.findall(r"\bint\s+(dv_rvreloc_[a-z0-9_]*)\s*\(", header))
    assert declared == {"dv_rvreloc_step_u8", "dv_rvreloc_sense_step"} == {k for k in N.PROTOTYPES if k.startswith("dv_rvreloc_")}
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name), name
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(N.PROTOTYPES[name][1]), name
    # the two windowed calls with the thresholds behind win_hi, and member_flags as an output of the uploaded form too
    w, r = N.PROTOTYPES["dv_rvwin_step_u8"][1], N.PROTOTYPES["dv_rvreloc_step_u8"][1]
    at = w.index(ctypes.c_uint32)
    assert r == w[:at] + [N._f64p] + w[at:] + [N._u32p]
    w, r = N.PROTOTYPES["dv_rvwin_sense_step"][1], N.PROTOTYPES["dv_rvreloc_sense_step"][1]
    at = w.index(ctypes.c_uint32)
    assert r == w[:at] + [N._f64p] + w[at:]
    # a result bit no other DV_RES_* uses
    res = {k: int(v) for k, v in re.findall(r"#define (DV_RES_[A-Z_]+)\s+(\d+)u", header)}
    assert res["DV_RES_RELOCALISED"] == N.DV_RES_RELOCALISED == H.RELOCALISED == 32
    assert all(v & 32 == 0 for k, v in res.items() if k != "DV_RES_RELOCALISED") and len(set(res.values())) == len(res)
    assert not [k for k in dir(navsim_amd) if "reloc" in k.lower()]                        # nothing new is exported


# ---- refusals before any library call ------------------------------------------------------------------------------------------------------------
class _NoLibrary(object):
    def __getattr__(self, name):
        raise AssertionError("library call %s after an argument that must be refused" % name)


class _Recorder(object):
    """A library that records the names of the calls made and answers DV_OK."""

    def __init__(self):
        self.names = []

    def __getattr__(self, name):
        def call(*a):
            self.names.append(name)
            return 0
        return call


def _engine(lib, first=(0, 3, 8, 1008), shape=(4, 4)):
    e = navsim_amd.FamiliarityEngine.__new__(navsim_amd.FamiliarityEngine)
    e._lib, e._ctx_raw, e._begun = lib, None, False
    e.n_lands, e.sensor_shape = 0, shape
    e.rviews_first, e.rviews_shape = np.array(first, dtype=np.int64), shape
    return e


ARGS = dict(patches=np.zeros((3, 2, 4, 4, 3), np.uint8), z=np.zeros(3), angs=np.zeros((3, 2)), routes=[0, 1, 2], weights=[0.0, 0.5, 1.0],
            lo=[0, 0, 0], hi=[3, 5, 9])


def _both(e, **kw):
    a = ARGS
    return (lambda: e.rvwin_step_u8(a["patches"], a["routes"], a["weights"], a["lo"], a["hi"], **kw),
            lambda: e.rvwin_sense_step(a["z"], a["z"], a["angs"], a["routes"], a["weights"], a["lo"], a["hi"], **kw))


@pytest.mark.parametrize("tau,match", [([0.0, np.nan, 1.0], "member 1: reloc_below is NaN"), ([0.0, 1.0], r"reloc_below must have shape \(3,\)"),
                                       ([[0.0, 1.0, 2.0]], r"reloc_below must have shape \(3,\)"), (["a", "b", "c"], "reloc_below must hold numbers"),
                                       (5.0, r"reloc_below must have shape \(3,\)")])
def test_refused_thresholds_never_reach_the_library(tau, match):
    for call in _both(_engine(_NoLibrary()), reloc_below=tau):
        with pytest.raises(ValueError, match=match):
            call()
    # the windowed calls' own refusals hold with a threshold too
    e = _engine(_NoLibrary())
    with pytest.raises(ValueError, match=r"member 1: window \[0, 6\)"):
        e.rvwin_step_u8(ARGS["patches"], ARGS["routes"], ARGS["weights"], [0, 0, 0], [3, 6, 9], reloc_below=[0.0, 0.0, 0.0])


def test_none_takes_todays_call_and_an_array_the_new_one():
    lib = _Recorder()
    e = _engine(lib)
    for call in _both(e):
        call()
    for call in _both(e, reloc_below=None):
        r = call()
        assert not r.relocalised.any()
    assert lib.names == ["dv_rvwin_step_u8", "dv_rvwin_sense_step"] * 2
    lib.names = []
    for call in _both(e, reloc_below=[-np.inf, np.inf, 3]):                                # infinities and integers are thresholds
        call()
    assert lib.names == ["dv_rvreloc_step_u8", "dv_rvreloc_sense_step"]


def test_the_c_checks_that_run_before_the_device():
    """What the library refuses without a device: a NULL context, and (on a context that was never made) nothing else to reach --
    the entry points exist and answer DV_ERR_INVALID = -1 before they touch anything."""
    lib = N.load()
    for name in ("dv_rvreloc_step_u8", "dv_rvreloc_sense_step"):
        args = [None if t is not ctypes.c_int and t is not ctypes.c_uint32 else 0 for t in N.PROTOTYPES[name][1]]
        assert getattr(lib, name)(*args) == -1, name


# ---- the constructors ---------------------------------------------------------------------------------------------------------------------------
def test_threshold_arguments():
    wins = [(2, 3), None, (5, 5)]
    assert E._thresholds_arg(None, wins) == [None] * 3
    assert E._thresholds_arg([10.0, None, -np.inf], wins) == [10.0, None, -np.inf]
    assert E._thresholds_arg(7, [(1, 1)] * 3) == [7.0] * 3 and E._thresholds_arg(np.inf, [(1, 1)]) == [np.inf]
    for arg, w, match in ((7.0, wins, r"relocalise_below\[1\] = 7.0, but member 1 has no window"), ([1.0, 2.0], wins, "2 entries for 3 starts"),
                          (np.nan, [(1, 1)], "relocalise_below is NaN"), ([1.0, None, np.nan], wins, r"relocalise_below\[2\] is NaN"),
                          ("high", [(1, 1)], "must be a familiarity"), ([True, None, 1.0], wins, r"relocalise_below\[0\] must be a familiarity"),
                          (5.0, [None], "has no window")):
        with pytest.raises(ValueError, match=match):
            E._thresholds_arg(arg, w)


def test_the_constructors_refuse_bad_thresholds_before_they_touch_the_engine():
    route = np.array([[50.0, 50.0], [51.0, 50.0], [52.0, 50.0]])
    starts = [(0, (50.0, 50.0), 0.0)]
    agent = types.SimpleNamespace(familiarity_model=sads_familiarity(0.25), _engine=_NoLibrary(), training_path=None, memory_bank=None)
    for kw, match in ((dict(relocalise_below=5.0), "member 0 has no window"), (dict(window=1, relocalise_below=np.nan), "is NaN"),
                      (dict(window=1, relocalise_below=[1.0, 2.0]), "2 entries for 1 starts")):
        with pytest.raises(ValueError, match=match):
            E.from_routes_with(agent, [route], starts, **kw)
        with pytest.raises(ValueError, match=match):
            E.from_landscapes(agent, [np.zeros((9, 9, 3), np.uint8)], [(0, route)], starts, **kw)


# ---- routing, the scene mask and the bookkeeping on a fake engine -------------------------------------------------------------------------------
LENGTHS, LEVEL = [30, 40], {0: 50.0, 1: 10.0}   # the fake windowed rows: 50 + a on route 0, 10 + a on route 1 (a < 3: maxima 52 and 12)


def test_without_a_threshold_the_calls_are_the_ones_there_were():
    ens = H.fake_ensemble(LENGTHS, LEVEL, [0, 1, 0], [(2, 3)] * 3, [5, 20, None], [None] * 3)
    H.fake_step(ens, [0, 1, 2])
    assert ens.engine.calls == [("rvwin", [0, 1], [3, 18], [9, 24], None), ("rviews", [0])]   # no reloc_below argument at all
    assert [a.relocalised for a in ens.agents] == [False] * 3 and [a.n_relocalisations for a in ens.agents] == [0] * 3


def test_members_with_and_without_a_threshold_share_the_one_windowed_call():
    # member 0: threshold 52 = its maximum (stays); member 1: 12.5 > 12 (lost); member 2: no threshold; member 3: no window; member 4: no centre
    ens = H.fake_ensemble(LENGTHS, LEVEL, [0, 1, 1, 0, 1], [(2, 3), (2, 3), (2, 3), None, (2, 3)], [5, 20, 30, None, None],
                          [52.0, 12.5, None, None, 99.0])
    r = H.fake_step(ens, [0, 1, 2, 3, 4])
    assert ens.engine.calls == [("rvwin", [0, 1, 1], [3, 18, 28], [9, 24, 34], [52.0, 12.5, -np.inf]), ("rviews", [0, 1])]   # two calls at most
    assert r.flags.tolist() == [0, 32, 0, 0, 0]
    assert [a.relocalised for a in ens.agents] == [False, True, False, False, False]
    assert [a.n_relocalisations for a in ens.agents] == [0, 1, 0, 0, 0]
    # memory_index = angle_view[best]: the lost member's is the whole-route search's (2 * 2), the others' their windows'
    assert [a.memory_index for a in ens.agents] == [5, 4, 30, None, 4]
    assert r.angle_familiarity[1].tolist() == [100.0, 101.0, 102.0] and r.angle_familiarity[0].tolist() == [50.0, 51.0, 52.0]
    # the next step: member 1's window is centred on what the global search found; it is still below its threshold and lost again
    ens.engine.calls = []
    H.fake_step(ens, [1, 4])
    assert ens.engine.calls == [("rvwin", [1, 1], [2, 2], [8, 8], [12.5, 99.0])]
    assert [ens.agents[i].n_relocalisations for i in (1, 4)] == [2, 1] and ens.agents[4].relocalised
    # a step in which it is not lost clears `relocalised` and keeps the count
    ens.agents[1].relocalise_below = 12.0
    H.fake_step(ens, [1])
    assert not ens.agents[1].relocalised and ens.agents[1].n_relocalisations == 2


def test_a_flagged_member_is_not_relocalised_and_keeps_its_books():
    ens = H.fake_ensemble(LENGTHS, LEVEL, [0, 1], [(2, 3)] * 2, [5, 20], [np.inf, np.inf], flagged=1)
    r = H.fake_step(ens, [0, 1])
    assert r.flags.tolist() == [32, 16] and r.best_idex.tolist() == [2, -1]
    assert [a.relocalised for a in ens.agents] == [True, False] and [a.n_relocalisations for a in ens.agents] == [1, 0]
    assert [a.memory_index for a in ens.agents] == [4, 20]


def test_the_scene_mask_after_a_relocalised_step():
    ens = H.fake_ensemble(LENGTHS, LEVEL, [0, 1], [(2, 3)] * 2, [5, 20], [0.0, 12.5])
    H.fake_step(ens, [0, 1])
    rows = ens.scene_familiarity()
    assert ens.engine.calls[-1] == ("scene", [0, 1])
    assert np.isposinf(rows[0][:3]).all() and np.isposinf(rows[0][9:]).all() and (rows[0][3:9] == 7.0).all()   # member 0 kept its window
    assert (rows[1] == 7.0).all() and len(rows[1]) == 40                                    # member 1 was relocalised: nothing is masked
    # relocalise() and memory_index = None work as before: the step scores the whole route by the unwindowed call, and is no relocalisation
    ens.relocalise([1])
    ens.engine.calls = []
    H.fake_step(ens, [0, 1])
    assert [c[0] for c in ens.engine.calls] == ["rvwin", "rviews"] and not ens.agents[1].relocalised and ens.agents[1].n_relocalisations == 1
    assert (ens.scene_familiarity()[1] == 7.0).all()


# ---- the device's plan ------------------------------------------------------------------------------------------------------------------------------
def test_the_devices_plan_is_rviews_plans_for_the_lost_columns():
    rng = np.random.default_rng(5)
    cases = [(H.COUNTS_ROUTES, H.COUNTS_LOST, H.COUNTS_A, 16), (H.COUNTS_ROUTES, H.COUNTS_LOST, H.COUNTS_A, 4),
             ((1, 0, 0), (1, 1, 1), 5, 4), ((1, 0, 0), (0, 0, 0), 5, 4), ((0,), (1,), 1, 16)]
    for _ in range(40):
        n, A = int(rng.integers(1, 40)), int(rng.integers(1, 9))
        cases.append((tuple(rng.integers(0, 5, n).tolist()), tuple(rng.integers(0, 2, n).tolist()), A, int(rng.choice([4, 8, 12, 16]))))
    for routes, lost, A, T in cases:
        col_of, tiles = H.device_plan(routes, lost, A, T)
        want_cols, want_tiles = H.host_plan(routes, lost, A, T)
        assert np.array_equal(col_of, want_cols), (routes, lost, A, T)
        assert [(r, n) for _, n, r in tiles] == want_tiles and [s for s, _, _ in tiles] == np.concatenate([[0], np.cumsum([n for _, n in want_tiles])])[:-1].tolist()
        # never more tiles than the host's grid has: those of "every member lost"
        assert len(tiles) <= len(H.device_plan(routes, [1] * len(routes), A, T)[1])
    assert [(r, n) for _, n, r in H.device_plan(H.COUNTS_ROUTES, H.COUNTS_LOST, H.COUNTS_A, 16)[1]] == H.COUNTS_TILES
    assert H.groups(6, 5, 10) == [(0, 2), (2, 4), (4, 6)] and H.groups(6, 5, 3) == [(i, i + 1) for i in range(6)] and H.groups(3, 5, 7710) == [(0, 3)]
    assert HE.tile_width(64 * 64) == 4 and HE.tile_width(8 * 8) == HE.tile_width(35) == HE.tile_width(32 * 32) == 16


# ---- facts that keep the GPU tests from being vacuous -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", H.BASIC_SHAPES)
def test_the_basic_case_separates_the_window_from_the_whole_route(h, w):
    case, windowed, whole = H.basic(h, w)
    taus = H.mixed_thresholds(windowed)
    fam, view, best, lost = H.apply_rule(windowed, whole, taus)
    assert lost.tolist() == [False, True, False, True, False, True]
    assert np.diff(case["first"])[case["routes"]].tolist() == [130, 2, 65, 130, 65, 130]
    for i in range(6):
        differs = windowed[0][i].tobytes() != whole[0][i].tobytes() or not np.array_equal(windowed[1][i], whole[1][i])
        assert differs, i                                                                  # a wrong decision shows in every member's row
    assert ((h * w + 3) // 4, (h * w) % 4) in ((9, 3), (16, 0))


def test_the_counts_case_gives_the_four_tile_widths():
    case, windows, taus, (fam, view, best, lost) = H.counts_case()
    assert lost.astype(int).tolist() == list(H.COUNTS_LOST)
    by_route = [int(sum(l for l, r in zip(H.COUNTS_LOST, H.COUNTS_ROUTES) if r == k)) * H.COUNTS_A for k in range(4)]
    assert by_route == [28, 0, 8, 4] and list(H.COUNTS_ROUTES) != sorted(H.COUNTS_ROUTES)
    assert all(hi - lo < length for (lo, hi), length in zip(windows, np.diff(case["first"])[case["routes"]]))


def test_the_many_case_crosses_the_planning_workgroups_passes():
    case, windows, taus, (fam, view, best, lost) = H.many_case()
    order = np.argsort(case["routes"], kind="stable")
    assert len(lost) == 300 > 256 and lost[order][:256].sum() < lost.sum() - 10           # lost members in both passes of the member loop
    col_of, tiles = H.device_plan(case["routes"], lost, H.MANY_A, 16)
    assert len(col_of) == 2 * lost.sum() > 256 and len(tiles) > 16                        # lost columns and tiles in later passes of the column loop
    assert sorted(set(r for _, _, r in tiles)) == [0, 1, 2] and (col_of >= 0).all()
    assert any(n < 16 for _, n, _ in tiles) and [(r, n) for _, n, r in tiles] == H.host_plan(case["routes"], lost, H.MANY_A, 16)[1]


def test_the_scenarios_shadows_show_the_rule():
    plain, ruled = H.scenario(None), H.scenario(H.ENS_THRESHOLD)
    # without the loss test the two mis-centred members never leave the far end of their routes ...
    assert all(m >= 3 * H.ENS_LENGTHS[0] // 4 for m in plain[1]["memory"]) and all(m >= 3 * H.ENS_LENGTHS[1] // 4 for m in plain[3]["memory"])
    # ... and what they see in their windows lies below the threshold, what the others see at or above it
    assert max(max(plain[i]["best_windowed"]) for i in (1, 3)) < H.ENS_THRESHOLD <= min(min(plain[i]["best_windowed"]) for i in (0, 2))
    # with it they relocalise in their first step and then track their twins
    assert [r["n"][-1] for r in ruled] == [0, 1, 0, 1] and [r["relocalised"][0] for r in ruled] == [False, True, False, True]
    assert all(not any(r["relocalised"][1:]) for r in ruled) and all(set(r["code"]) == {0} for r in ruled)
    assert ruled[1]["memory"] == ruled[0]["memory"] and ruled[3]["memory"] == ruled[2]["memory"]
    assert ruled[0]["pos"] == plain[0]["pos"] and ruled[1]["pos"] != plain[1]["pos"]
    # the relocalised step's scene_familiarity is the whole route's row; the next step's is masked again
    assert np.isfinite(ruled[1]["scene"][0]).all() and np.isneginf(ruled[1]["scene"][1]).sum() == H.ENS_LENGTHS[0] - 9   # (views [0, 3 + 5 + 1))
    assert HW.MAX_VIEWS == 512
