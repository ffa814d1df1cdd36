"""Windowed SSD on the route view store without a device: the NumPy restatement of k_rvssdw_score held to the expected values of every
GPU case, the binding surface of the dv_rvssdw_* calls, the constants of csrc/dejavu_rvssdw.inl, the engine's refusals (raised before
any library call), the windows' arguments of SsdRouteEnsemble (SadsRouteEnsemble's, by its texts) and its routing on a recording
engine."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import ssd_familiarity
from navsim_amd.engine import RouteSsdResults
from tests import helpers_rvssd as HV
from tests import helpers_rvssdw as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"dv_rvssdw_step_u8": "rvssdw_step_u8", "dv_rvssdw_sense_step": "rvssdw_sense_step"}
E, SADS = navsim_amd.SsdRouteEnsemble, navsim_amd.SadsRouteEnsemble


# ---- the kernel's statement in NumPy --------------------------------------------------------------------------------------------------------------
def _statement_equals_expected(c, channel=2, members=None):
    for i in (range(len(c["routes"])) if members is None else members):
        r, (lo, hi) = c["routes"][i], c["windows"][i]
        ssd, view = H.window_statement(c["views"][c["first"][r]:c["first"][r + 1]], c["patches"][i], lo, hi, channel)
        assert np.array_equal(ssd, c["want"][0][i].astype(np.int64)) and np.array_equal(view, c["want"][1][i]), (i, channel)
        assert c["want"][2][i] == int(np.argmin(ssd)), i


def test_statement_on_the_window_edges_and_the_planted_matches():
    c = H.edges_case()
    _statement_equals_expected(c)
    # unmasked, a padding view of route 1's last group (zero bytes) would be the all-zero patch's best view
    lib = np.concatenate([c["views"][600:], np.zeros((62, 5, 5, 3), dtype=np.uint8)])
    ssd, view = H.window_statement(lib, c["patches"][4], 100, 192, 2)
    assert ssd[0] == 0 and view[0] == 130
    p = H.planted_case()
    _statement_equals_expected(p)
    lib = p["views"]
    assert H.window_statement(lib, p["patches"][0], 69, 130, 2)[1][1] == 69 and H.window_statement(lib, p["patches"][0], 70, 131, 2)[1][1] == 130


@pytest.mark.parametrize("channel", (0, 1, 2))
def test_statement_on_the_7x5_tail(channel):
    _statement_equals_expected(H.tail_case(channel), channel)


def test_statement_on_the_sign_edges_the_extremes_and_the_ties():
    _statement_equals_expected(H.ahead_case())
    _statement_equals_expected(H.edge_byte_case())
    _statement_equals_expected(H.extreme_case())
    for second in (40, 70):
        for which in (0, 1, 2):
            _statement_equals_expected(H.tie_case(second, which))


@pytest.mark.parametrize("A", H.TILE_HEADINGS)
def test_statement_on_the_tiles_and_what_the_rule_makes_of_them(A):
    c = H.tiles_case(A)
    _statement_equals_expected(c)
    taus, (ssd, view, best, lost) = H.mixed_thresholds(c)
    assert lost.tolist() == [True, True, True, False, False] and [int(c["routes"][i]) for i in np.flatnonzero(lost)] == [3, 1, 3]
    assert np.array_equal(ssd[:3], c["whole"][0][:3]) and np.array_equal(ssd[3:], c["want"][0][3:])
    assert taus[3] == -c["want"][0][3].min() and taus[0] > -c["want"][0][0].min() and np.nextafter(taus[0], -np.inf) == -c["want"][0][0].min()
    if A == 33:
        assert 2 * A > 2 * HV.TILE and A % HV.TILE                                        # route 3's lost columns: a tile spans both members


def test_statement_on_the_members_around_the_launch_bound():
    c = H.bound_case()
    n = len(c["routes"])
    assert n == H.MEMBERS_PER_LAUNCH + 1 and c["patches"].shape[:2] == (n, 1)
    _statement_equals_expected(c, members=(0, 1, H.MEMBERS_PER_LAUNCH - 1, H.MEMBERS_PER_LAUNCH))


def test_whole_route_windows_give_the_unwindowed_expected_values():
    c = HV.geometry_case("many")
    lens = np.diff(c["first"])[c["routes"]]
    got = H.window_expected(c["views"], c["first"], c["patches"], c["routes"], [(0, int(n)) for n in lens], 2)
    assert all(np.array_equal(g, w) for g, w in zip(got, c["want"][:3]))


# ---- binding surface --------------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_engine_agree_on_the_rvssdw_names():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    declared = set(re.findall(r"\bint\s+(dv_rvssdw_[a-z0-9_]*)\s*\(", header))
    assert declared == set(NAMES) == {k for k in N.PROTOTYPES if k.startswith("dv_rvssdw_")}
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert N.PROTOTYPES[name][0] is ctypes.c_int
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(N.PROTOTYPES[name][1]), name
        assert callable(getattr(navsim_amd.FamiliarityEngine, NAMES[name])), name
    P = N.PROTOTYPES
    # the unwindowed calls with the windows and the thresholds behind the tables, and the flag word at the end of both
    assert P["dv_rvssdw_step_u8"][1] == P["dv_rvssd_step_u8"][1][:5] + [N._i32p, N._i32p, N._f64p] + P["dv_rvssd_step_u8"][1][5:] + [N._u32p]
    assert P["dv_rvssdw_sense_step"][1] == P["dv_rvssd_sense_step"][1][:8] + [N._i32p, N._i32p, N._f64p] + P["dv_rvssd_sense_step"][1][8:]
    for name, order in (("dv_rvssdw_step_u8", "patches n_agents n_headings route_of_member win_lo win_hi reloc_below channel angle_ssd angle_view "
                                              "best_heading member_flags"),
                        ("dv_rvssdw_sense_step", "x y angles n_agents n_headings route_of_member land_of_member win_lo win_hi reloc_below channel "
                                                 "angle_ssd angle_view best_heading member_flags")):
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert [a.split()[-1].lstrip("*") for a in args.split(",")][1:] == order.split(), name
    FE = navsim_amd.FamiliarityEngine
    assert list(inspect.signature(FE.rvssdw_step_u8).parameters) == ["self", "patches", "route_of_member", "win_lo", "win_hi", "channel", "reloc_below"]
    assert list(inspect.signature(FE.rvssdw_sense_step).parameters) == ["self", "x", "y", "angles", "route_of_member", "win_lo", "win_hi", "channel",
                                                                         "land_of_member", "reloc_below"]
    for f in (FE.rvssdw_step_u8, FE.rvssdw_sense_step):
        assert inspect.signature(f).parameters["channel"].default == 2 and inspect.signature(f).parameters["reloc_below"].default is None


def test_the_constants_of_the_source_are_the_helpers():
    src = open(os.path.join(REPO, "navigation-by-deja-vu_amd", "csrc", "dejavu_rvssdw.inl")).read()
    got = {k: int(v) for k, v in re.findall(r"constexpr int (kRvssdw[A-Za-z]*) = (\d+);", src)}
    assert got == {"kRvssdwMembersPerLaunch": H.MEMBERS_PER_LAUNCH, "kRvssdwAhead": H.AHEAD} and H.MEMBERS_PER_LAUNCH <= 65535   # a grid's y
    assert "rvssd_group_acc<kRvssdwAhead>(" in src and H.AHEAD >= 1                       # (integer sums: the K-steps' order does not show)
    assert "for (int i0 = 0; i0 < N; i0 += kRvssdwMembersPerLaunch)" in src                # the launches loop over the bound
    assert "mins[4][kRvssdTile]" in src and HV.TILE == 32 and HV.GROUPS_PER_BLOCK == 4    # the tile and the four waves are dejavu_rvssd.inl's
    assert "reloc.T = kRvssdTile" in src and "kRvssdTilesPerLaunch" in src
    assert H.MAX_VIEWS == N.DV_RVWIN_MAX_VIEWS == navsim_amd.FamiliarityEngine.RVWIN_MAX_VIEWS == E.WINDOW_MAX_VIEWS
    assert H.covered_groups(63, 63 + H.MAX_VIEWS) == (0, 8)                               # nine groups at most: three trips of a wave
    assert "mfma" not in src                                                              # the K loop is shared, not copied


# ---- the engine's refusals come before the library ----------------------------------------------------------------------------------------------------
def _engine_without_a_device(lib, shape=(4, 4), first=(0, 3, 8, 1008)):
    e = navsim_amd.FamiliarityEngine.__new__(navsim_amd.FamiliarityEngine)
    e._lib, e._ctx_raw, e._begun, e.sensor_shape, e.n_lands = lib, None, False, shape, 0
    if first is not None:
        e.rviews_first, e.rviews_shape = np.array(first, dtype=np.int64), shape
    return e


ARGS = dict(patches=np.zeros((3, 2, 4, 4, 3), np.uint8), z=np.zeros(3), angs=np.zeros((3, 2)), routes=[0, 1, 2], lo=[0, 0, 100], hi=[3, 5, 612])


def _both(e, **kw):
    a = dict(ARGS, **kw)
    extra = {k: a[k] for k in ("channel", "reloc_below") if k in a}
    return (lambda: e.rvssdw_step_u8(a["patches"], a["routes"], a["lo"], a["hi"], **extra),
            lambda: e.rvssdw_sense_step(a["z"], a["z"], a["angs"], a["routes"], a["lo"], a["hi"], **extra))


@pytest.mark.parametrize("kw,match", [(dict(lo=[0, -1, 0], hi=[3, 5, 9]), r"member 1: window \[-1, 5\)"),
                                      (dict(lo=[0, 0, 0], hi=[3, 6, 9]), r"member 1: window \[0, 6\).*route 1 of 5 views"),
                                      (dict(lo=[2, 0, 0], hi=[2, 5, 9]), r"member 0: window \[2, 2\)"),
                                      (dict(lo=[0, 0, 100], hi=[3, 5, 613]), r"member 2: window \[100, 613\) must hold 1 to 512 views"),
                                      (dict(lo=[0, 0]), r"win_lo must have shape \(3,\)"), (dict(hi=[3.0, 5.0, 9.0]), "win_hi must hold integers"),
                                      (dict(reloc_below=[0.0, np.nan, -1.0]), "member 1: reloc_below is NaN"),
                                      (dict(reloc_below=[0.0, -1.0]), r"reloc_below must have shape \(3,\)"),
                                      (dict(reloc_below=["a", "b", "c"]), "reloc_below must hold numbers"),
                                      (dict(channel=3), "channel must be 0, 1 or 2"), (dict(channel=True), "channel must be 0, 1 or 2"),
                                      (dict(routes=[0, 3, 1]), r"route_of_member\[1\] = 3")])
def test_refusals_come_before_any_library_call(kw, match):
    lib = HV.Recorder()
    e = _engine_without_a_device(lib)
    for call in _both(e, **kw):
        with pytest.raises(ValueError, match=match):
            call()
    assert lib.calls == []


def test_no_store_is_refused_and_what_passes_reaches_the_one_symbol_of_its_call():
    lib = HV.Recorder()
    bare = _engine_without_a_device(lib, first=None)
    for call in _both(bare):
        with pytest.raises(N.EngineError, match="no route views"):
            call()
    with pytest.raises(ValueError, match=r"uint8\[n, A, 4, 4, 3\]"):
        _engine_without_a_device(lib).rvssdw_step_u8(np.zeros((3, 2, 4, 5, 3), np.uint8), [0, 1, 2], ARGS["lo"], ARGS["hi"])
    assert lib.calls == []
    e = _engine_without_a_device(lib)
    u8, sensed = _both(e)
    r = u8()
    assert lib.calls == ["dv_rvssdw_step_u8"] and isinstance(r, RouteSsdResults) and r.angle_ssd.shape == (3, 2) and r.angle_view.dtype == np.int64
    assert np.array_equal(r.angle_familiarity, np.negative(r.angle_ssd)) and not r.relocalised.any()
    sensed()
    u8, sensed = _both(e, reloc_below=[-np.inf, 0.0, np.inf], channel=0)
    u8()
    sensed()
    assert lib.calls == ["dv_rvssdw_step_u8", "dv_rvssdw_sense_step"] * 2               # with thresholds too: one symbol a call


# ---- the ensemble's arguments -------------------------------------------------------------------------------------------------------------------------
def test_the_windows_helpers_are_one_copy_on_both_ensembles():
    for name in ("_windows_arg", "_thresholds_arg", "_set_windows", "relocalise", "_window_of"):
        a, b = getattr(E, name), getattr(SADS, name)
        assert getattr(a, "__func__", a) is getattr(b, "__func__", b), name
    assert E.WINDOW_MAX_VIEWS == SADS.WINDOW_MAX_VIEWS == 512
    for name in ("from_routes_with", "from_landscapes"):
        for kw in ("window", "window_centres", "relocalise_below"):
            assert inspect.signature(getattr(E, name)).parameters[kw].default is None, (name, kw)


def test_the_constructors_refuse_bad_windows_by_the_sads_ensembles_texts_before_they_touch_the_engine():
    class _NoLibrary(object):
        def __getattr__(self, name):
            raise AssertionError("engine call %s after an argument that must be refused" % name)
    route = np.array([[50.0, 50.0], [51.0, 50.0], [52.0, 50.0]])
    starts = [(0, (50.0, 50.0), 0.0)]
    agent = types.SimpleNamespace(familiarity_model=ssd_familiarity(2), _engine=_NoLibrary(), training_path=None, memory_bank=None)
    for kw in (dict(window=(600, 0)), dict(window=(1, 2, 3)), dict(window_centres=[1]), dict(window=1, window_centres=[3]), dict(window=[None], window_centres=[1]),
               dict(relocalise_below=-5.0), dict(window=[None], relocalise_below=[-5.0]), dict(window=1, relocalise_below=float("nan")),
               dict(window=1, relocalise_below=[-1.0, -2.0]), dict(window=1, relocalise_below="low")):
        texts = []
        for ens, model in ((E, ssd_familiarity(2)), (SADS, navsim_amd.sads_familiarity(0.25))):
            agent.familiarity_model = model
            for make in (lambda: ens.from_routes_with(agent, [route], starts, **kw),
                         lambda: ens.from_landscapes(agent, [np.zeros((9, 9, 3), np.uint8)], [(0, route)], starts, **kw)):
                with pytest.raises(ValueError) as err:
                    make()
                texts.append(str(err.value))
        assert len(set(texts)) == 1, (kw, texts)
    agent.familiarity_model = ssd_familiarity(2)
    with pytest.raises(ValueError, match="but member 0 has no window: the threshold is a windowed member's loss test"):
        E.from_routes_with(agent, [route], starts, relocalise_below=-5.0)
    with pytest.raises(ValueError, match=r"window_centres\[0\] = 1, but member 0 has no window"):
        E.from_routes_with(agent, [route], starts, window=[None], window_centres=[1])
    with pytest.raises(ValueError, match="window_centres without window"):
        E.from_routes_with(agent, [route], starts, window_centres=[1])


# ---- the ensemble's routing on a recording engine -------------------------------------------------------------------------------------------------------
class RecordingEngine(object):
    """Answers a step with angle_view[k, a] = (lo of member k, or 0) + 2 * a + 1 clipped to the window / route, best_idex 1, flag 16
    for the members on route `flagged`, and flag 32 for the windowed members whose threshold is above `level`."""

    def __init__(self, lengths, level=-100.0, flagged=None):
        self.lengths, self.level, self.flagged, self.calls = lengths, level, flagged, []

    def _answer(self, routes, A, lo, hi, taus=None):
        n = len(routes)
        view = np.minimum(np.asarray(lo)[:, None] + 2 * np.arange(A)[None, :] + 1, np.asarray(hi)[:, None] - 1).astype(np.int64)
        lost = np.zeros(n, dtype=bool) if taus is None else self.level < np.asarray(taus)
        view[lost] = 0                                                                    # (a whole-route row: its best view is view 0)
        flags = np.array([16 if r == self.flagged else 32 if gone else 0 for r, gone in zip(routes, lost)], dtype=np.uint32)
        ssd = np.arange(n * A, dtype=np.float64).reshape(n, A) + np.asarray(lo)[:, None]
        return RouteSsdResults(ssd, view, np.where(flags == 16, -1, 1).astype(np.int32), flags)

    def rvssd_sense_step(self, x, y, angs, routes, channel=2, land_of_member=None):
        self.calls.append(("rvssd", list(routes), None, None, None, channel))
        return self._answer(routes, np.asarray(angs).shape[1], [0] * len(routes), [self.lengths[r] for r in routes])

    def rvssdw_sense_step(self, x, y, angs, routes, win_lo, win_hi, channel=2, land_of_member=None, reloc_below=None):
        self.calls.append(("rvssdw", list(routes), list(win_lo), list(win_hi), None if reloc_below is None else list(reloc_below), channel))
        return self._answer(routes, np.asarray(angs).shape[1], win_lo, win_hi, reloc_below)


def fake_ensemble(lengths, routes, windows, centres, thresholds=None, **kw):
    ens = object.__new__(E)
    ens.agents = [types.SimpleNamespace(training_path=np.zeros((lengths[r], 2)), memory_bank=r) for r in routes]
    ens._set_windows(windows, centres, thresholds)
    ens.engine, ens.channel = RecordingEngine(lengths, **kw), 1
    ens._banks, ens._lands = np.array(routes, dtype=np.int32), None
    return ens


def step(ens, idx):
    n = len(idx)
    return ens._device_step(idx, np.zeros(n), np.zeros(n), np.zeros((n, 3)))


def test_windowed_members_go_to_the_windowed_call_and_the_rest_to_the_unwindowed_one():
    ens = fake_ensemble([30, 40], [0, 1, 1, 0], [(2, 3)] * 3 + [None], [1, 38, None, None])
    r = step(ens, [0, 1, 2, 3])
    assert ens.engine.calls == [("rvssdw", [0, 1], [0, 36], [5, 40], None, 1), ("rvssd", [1, 0], None, None, None, 1)]   # no threshold: no table
    assert isinstance(r, RouteSsdResults) and r.angle_view[:, 1].tolist() == [3, 39, 3, 3] and not r.flags.any()       # merged in the caller's order
    assert np.array_equal(r.angle_familiarity, np.negative(r.angle_ssd)) and r.angle_ssd[1].tolist() == [39.0, 40.0, 41.0]
    assert [a.memory_index for a in ens.agents] == [3, 39, 3, None]                       # angle_view[best]; member 3 has no window
    ens.engine.calls = []
    step(ens, [2, 1])                                                                      # a later step of two of them, in another order
    assert ens.engine.calls == [("rvssdw", [1, 1], [1, 37], [7, 40], None, 1)]
    ens.relocalise([1])
    assert [a.memory_index for a in ens.agents] == [3, None, 4, None]


def test_the_threshold_table_travels_only_when_a_member_of_the_call_has_one():
    ens = fake_ensemble([30, 40], [0, 1, 1, 0], [(2, 3)] * 4, [10, 20, 20, None], [None, -50.0, -200.0, -50.0])
    r = step(ens, [0, 1, 2, 3])
    assert ens.engine.calls == [("rvssdw", [0, 1, 1], [8, 18, 18], [14, 24, 24], [-np.inf, -50.0, -200.0], 1), ("rvssd", [0], None, None, None, 1)]
    assert r.flags.tolist() == [0, 32, 0, 0] and r.relocalised.tolist() == [False, True, False, False]
    assert [a.relocalised for a in ens.agents] == [False, True, False, False] and [a.n_relocalisations for a in ens.agents] == [0, 1, 0, 0]
    assert [a.memory_index for a in ens.agents] == [11, 0, 21, 3]
    assert ens._step_windows[id(ens.agents[1])] is None and ens._step_windows[id(ens.agents[2])] == (18, 24)          # nothing masked after the search
    ens.engine.calls = []
    step(ens, [0])                                                                         # the one member of this call has no threshold
    assert ens.engine.calls == [("rvssdw", [0], [9], [15], None, 1)]


def test_a_flagged_member_is_never_relocalised_and_keeps_its_books():
    ens = fake_ensemble([30, 40], [0, 1], [(2, 3)] * 2, [10, 20], [-50.0, -50.0], flagged=1)
    r = step(ens, [0, 1])
    assert r.flags.tolist() == [32, 16] and r.best_idex.tolist() == [1, -1]
    assert [a.memory_index for a in ens.agents] == [0, 20] and [a.n_relocalisations for a in ens.agents] == [1, 0]


def test_without_a_window_anywhere_the_step_is_exactly_the_one_unwindowed_call():
    ens = fake_ensemble([30, 40], [0, 1, 0], [None] * 3, [None] * 3)

    def never(*a, **k):
        raise AssertionError("rvssdw_sense_step without a window")
    ens.engine.rvssdw_sense_step = never
    for _ in range(3):
        step(ens, [0, 1, 2])
    assert ens.engine.calls == [("rvssd", [0, 1, 0], None, None, None, 1)] * 3
    plain = object.__new__(E)                                                               # members made without the new arguments at all
    plain.agents = [types.SimpleNamespace(training_path=np.zeros((30, 2)), memory_bank=0)]
    plain.engine, plain.channel, plain._banks, plain._lands = ens.engine, 1, np.zeros(1, np.int32), None
    step(plain, [0])
    assert len(ens.engine.calls) == 4 and not hasattr(plain.agents[0], "memory_index")


def test_the_scene_row_is_masked_outside_the_window_and_unmasked_after_a_relocalised_step():
    ens = fake_ensemble([30, 40], [0, 1, 1], [(2, 3)] * 3, [10, 20, None], [None, -50.0, None])
    step(ens, [0, 1, 2])
    rows = [np.arange(30.0), np.arange(40.0), np.arange(40.0)]
    ens.engine.rvssd_scene = lambda x, y, angs, routes, channel, land_of_member=None: [rows[i] for i in range(len(routes))]
    for i, a in enumerate(ens.agents):
        a.track_scene_familiarity, a._scene_fam, a._scene_owner, a.landscape_index = True, np.empty(len(rows[i])), None, None
        a.scene_familiarity = a._scene_fam
        ens._note_scene(a, 0.0, 0.0, np.zeros(3), None)
        assert a._scene_stale[4] == ((8, 14), None, None)[i]
    got = ens.scene_familiarity()
    assert np.isposinf(got[0][:8]).all() and np.isposinf(got[0][14:]).all() and np.array_equal(got[0][8:14], -rows[0][8:14])
    assert np.array_equal(got[1], -rows[1]) and np.array_equal(got[2], -rows[2])           # re-localised; no centre: the whole rows
