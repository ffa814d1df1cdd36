"""NCC on the route view store without a device: the statement held to np.corrcoef and to its exact values, the NumPy restatement of the
scoring kernel on every case, the conditions the GPU cases rely on, the binding surface of the dv_rvncc_* calls, the engine's refusals
(raised before any library call), the constants of csrc/dejavu_rvssd.inl the cases are built on, and every ensemble's refusal."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import infomax_familiarity, mushroom_familiarity, ncc_familiarity, sads_familiarity, ssd_familiarity, synth
from tests import helpers_rvncc as HC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"dv_rvncc_step_u8": "rvncc_step_u8", "dv_rvncc_sense_step": "rvncc_sense_step", "dv_rvncc_scene_u8": "rvncc_scene_u8",
         "dv_rvncc_scene": "rvncc_scene"}
SHAPES = ((7, 5), (33, 31), (32, 32), (64, 64))             # P = 35, 1023, 1024, 4096


# ---- the statement ---------------------------------------------------------------------------------------------------------------------------
def test_the_statement_is_within_1e_12_of_corrcoef_wherever_both_variances_are_non_zero():
    rng = np.random.default_rng(3)
    for h, w in SHAPES:
        for _ in range(6):
            a, b = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)
            for x, y in ((a, b), (a, (a // 2 + rng.integers(0, 40, (h, w))).astype(np.uint8)), (a, 255 - a // 3)):
                want = np.corrcoef(x.reshape(-1).astype(np.float64), y.reshape(-1).astype(np.float64))[0, 1]
                assert abs(HC.ncc_pair(x, y) - want) <= 1e-12, (h, w)


def test_the_exact_values_of_the_statement():
    rng = np.random.default_rng(4)
    for h, w in SHAPES:
        for _ in range(4):
            a = rng.integers(0, 200, (h, w), dtype=np.uint8)
            assert HC.ncc_pair(a, a) == 1.0                                               # an identical view: sqrt(fl(x * x)) == x
            assert HC.ncc_pair(a, a + 55) == 1.0                                          # an offset without clipping
            assert HC.ncc_pair(a, 255 - a) == -1.0                                        # the complement
            five = (rng.integers(0, 5, (h, w)) * 63).astype(np.uint8)                     # a 5-level plane against a constant one
            assert HC.ncc_pair(five, np.full((h, w), 90, dtype=np.uint8)) == 0.0 == HC.ncc_pair(np.full((h, w), 255, dtype=np.uint8), five)
    alt = np.zeros((64, 64), dtype=np.uint8)
    alt[:, ::2] = 255                                                                     # the largest sums: num, Va, Vb = 2^38 - ...
    assert HC.ncc_pair(alt, alt) == 1.0 and HC.ncc_pair(alt, 255 - alt) == -1.0
    assert 4096 * int((alt.astype(np.int64) ** 2).sum()) > 2 ** 31                         # (P * Sab overflows int32 at 64 x 64)


def test_the_vectorised_statement_is_the_statement_pair_by_pair():
    for c in (HC.ncc_tail_case(7, 5), HC.ncc_edge_byte_case(), HC.constant_case(), HC.ncc_extreme_case()):
        for i, r in enumerate(c["routes"]):
            lib = c["views"][c["first"][r]:c["first"][r + 1]]
            rows = HC.ncc_rows(lib, c["patches"][i], 2)
            for a in range(min(2, rows.shape[0])):
                for f in range(0, rows.shape[1], 7):
                    want = HC.ncc_pair(c["patches"][i, a, :, :, 2], lib[f, :, :, 2])
                    assert np.array_equal(HC.bits(rows[a, f]), HC.bits(want)), (i, a, f)
    assert np.abs(HC.ncc_rows(HC.ncc_tail_case(7, 5)["views"], HC.ncc_tail_case(7, 5)["patches"][0], 2)).max() <= 1.0


# ---- the kernel's arithmetic in NumPy ----------------------------------------------------------------------------------------------------------
def _statement_equals_expected(c, channel=2):
    want = c["want"][channel]
    for i, r in enumerate(c["routes"]):
        lib = c["views"][c["first"][r]:c["first"][r + 1]]
        q, view, rows = HC.kernel_statement(lib, c["patches"][i], channel)
        assert np.array_equal(HC.bits(q), HC.bits(want[0][i])) and np.array_equal(view, want[1][i]), (i, channel)
        assert np.array_equal(HC.bits(rows.min(axis=0)), HC.bits(want[3][i])), (i, channel)


@pytest.mark.parametrize("channel", (0, 1, 2))
def test_kernel_statement_on_the_7x5_tail(channel):
    """P = 35, Pw = 9: the second K-step holds 3 real pixels, 1 byte of the store's zero padding and 7 dwords that are not loaded."""
    _statement_equals_expected(HC.ncc_tail_case(7, 5), channel)


def test_kernel_statement_on_every_other_case():
    for c in (HC.ncc_edge_byte_case(), HC.ncc_extreme_case(), HC.gain_case(), HC.constant_case(), HC.negative_case(), HC.ncc_lengths_case(),
              HC.ncc_tie_case(), HC.members_case(7, 10), HC.ncc_geometry_case("one")):
        _statement_equals_expected(c)
    for shape in ((33, 31), (32, 32)):
        _statement_equals_expected(HC.ncc_tail_case(*shape), 2)


def test_unmasked_a_padding_view_would_win_where_every_view_correlates_negatively():
    c = HC.negative_case()
    lib = np.concatenate([c["views"], np.zeros((63, 5, 5, 3), dtype=np.uint8)])           # the route's two groups, the padding as views
    q, view, _ = HC.kernel_statement(lib, c["patches"][0], 2)
    assert q[0] == 0.0 and view[0] == 65
    q, view, _ = HC.kernel_statement(c["views"], c["patches"][0], 2)
    assert q[0] < 0.0 and view[0] < 65


# ---- what the GPU cases rely on --------------------------------------------------------------------------------------------------------------
def test_the_cases_hold_what_the_gpu_tests_rely_on():
    c = HC.gain_case()
    ncc, view, best, _ = c["want"][2]
    assert ncc[0, 0] == 1.0 and view[0, 0] == HC.GAIN_K
    assert HC.ssd_first_min(c["views"], c["patches"][0], 2)[0] != HC.GAIN_K                # SSD reports another view
    assert c["views"].max() <= 120
    c = HC.constant_case()
    ncc, view, best, scene = c["want"][2]
    assert ncc[0].tolist() == [0.0, 0.0] and view[0].tolist() == [0, 4] and best[0] == 0
    rows = HC.ncc_rows(c["views"], c["patches"][0], 2)
    assert (rows[0] == 0.0).all() and (np.delete(rows[1], 4) < 0).all() and rows[1, 4] == 0.0
    c = HC.negative_case()
    assert c["want"][2][0][0, 0] < 0.0 and len(c["views"]) == 65                           # the expected maximum is below zero
    c = HC.ncc_lengths_case()
    lens = np.array(HC.NCC_LENGTHS)[c["routes"]]
    assert sorted(lens.tolist()) == [2, 33, 64, 65, 130, 300] and lens.tolist() != sorted(lens.tolist())
    assert (c["want"][2][0][:, 0] == 1.0).all() and np.array_equal(c["want"][2][1][:, 0], lens - 1)
    assert (300 + 63) // 64 > HC.GROUPS_PER_BLOCK                                          # a second block of four view groups
    c = HC.ncc_tie_case()
    ncc, view, best, _ = c["want"][2]
    assert ncc[0].tolist()[1:] == [1.0, 1.0] and ncc[0, 0] < 1.0 and view[0].tolist()[1:] == [5, 5] and best[0] == 1
    assert 5 // 64 != 290 // 64 and 5 // (64 * HC.GROUPS_PER_BLOCK) != 290 // (64 * HC.GROUPS_PER_BLOCK)
    c = HC.ncc_extreme_case()
    assert c["want"][2][0][0].tolist() == [1.0, 1.0, 0.0]
    c = HC.ncc_edge_byte_case()
    assert set(np.unique(c["views"]).tolist()) == set(HC.EDGE_BYTES)
    # 7 members x 10 headings: tiles cut members; 33 and 70 headings: more than a tile a member
    tiles = HC.plan_tiles(HC.members_case(7, 10)["routes"], 10)
    assert any((s + n) % 10 for s, n, _ in tiles)                                          # a tile ends inside a member
    assert len(HC.plan_tiles(HC.members_case(1, 33)["routes"], 33)) == 2 and len(HC.plan_tiles(HC.members_case(2, 70)["routes"], 70)) == 6


def test_the_launch_edge_cases_and_their_tiles():
    """The plan cuts tiles by route, not by member: 32 769 members of ONE route are 1025 tiles, one launch.  A launch of its own for the
    last tile needs 32 769 tiles: a route per member."""
    many = HC.many_members_case()
    assert many["patches"].shape[:2] == (32769, 1) and many["views"].shape == (3, 7, 5, 3)
    tiles = HC.plan_tiles(many["routes"], 1)
    assert len(tiles) == 1025 and tiles[-1][:2] == (32768, 1)
    edge = HC.launch_edge_case()
    tiles = HC.plan_tiles(edge["routes"], 1)
    assert len(tiles) == HC.TILES_PER_LAUNCH + 1 and all(n == 1 for _, n, _ in tiles)


# ---- binding surface -------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_engine_agree_on_the_rvncc_names():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    declared = set(re.findall(r"\bint\s+(dv_rvncc_[a-z0-9_]*)\s*\(", header))
    assert declared == set(NAMES) == {k for k in N.PROTOTYPES if k.startswith("dv_rvncc_")}
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert N.PROTOTYPES[name][0] is ctypes.c_int
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(N.PROTOTYPES[name][1]), name
        assert callable(getattr(navsim_amd.FamiliarityEngine, NAMES[name])), name
        # dv_rvssd_*'s call argument for argument, angle_ncc / scene_ncc in place of angle_ssd / scene_ssd
        twin = name.replace("rvncc", "rvssd")
        assert N.PROTOTYPES[name] == N.PROTOTYPES[twin], name
        twin_args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % twin, header).group(1)
        assert re.sub(r"\s+", " ", args) == re.sub(r"\s+", " ", twin_args.replace("_ssd", "_ncc")), name
    E = navsim_amd.FamiliarityEngine
    for call in NAMES.values():
        assert list(inspect.signature(getattr(E, call)).parameters) == list(inspect.signature(getattr(E, call.replace("rvncc", "rvssd"))).parameters)
        assert inspect.signature(getattr(E, call)).parameters["channel"].default == 2
    assert inspect.signature(E.rvncc_scene).parameters["want_flags"].default is False


def test_the_constants_of_the_source_are_the_helpers_and_the_only_atomics_are_integer_minima():
    csrc = os.path.join(REPO, "navigation-by-deja-vu_amd", "csrc")
    ssd = open(os.path.join(csrc, "dejavu_rvssd.inl")).read()
    got = {k: int(v) for k, v in re.findall(r"constexpr int (kRvssd[A-Za-z]*) = (\d+);", ssd)}
    assert got == {"kRvssdTile": HC.TILE, "kRvssdGroupsPerBlock": HC.GROUPS_PER_BLOCK, "kRvssdTilesPerLaunch": HC.TILES_PER_LAUNCH}
    code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "dejavu_rvncc.inl")).read())
    assert set(re.findall(r"atomic[A-Za-z]*", code)) == {"atomicMin"}                       # 64-bit integers, on the encoding of the double


# ---- the engine's refusals come before the library --------------------------------------------------------------------------------------------
def _engine_without_a_device(lib, shape=(7, 5), first=(0, 5, 9)):
    e = navsim_amd.FamiliarityEngine.__new__(navsim_amd.FamiliarityEngine)
    e._lib, e._ctx_raw, e._begun, e.sensor_shape = lib, None, False, shape
    if first is not None:
        e.rviews_first, e.rviews_shape = np.array(first, dtype=np.int64), shape
    return e


def test_refusals_come_before_any_library_call():
    lib = HC.Recorder()
    e = _engine_without_a_device(lib)
    patches = np.zeros((2, 3, 7, 5, 3), dtype=np.uint8)
    x, y, angs = [50.0, 60.0], [50.0, 60.0], np.zeros((2, 3))
    for channel in (3, -1, 1.0, True, None):
        for call in (lambda: e.rvncc_step_u8(patches, [0, 1], channel), lambda: e.rvncc_scene_u8(patches, [0, 1], channel),
                     lambda: e.rvncc_sense_step(x, y, angs, [0, 1], channel), lambda: e.rvncc_scene(x, y, angs, [0, 1], channel)):
            with pytest.raises(ValueError, match="channel must be 0, 1 or 2"):
                call()
    for bad in (np.zeros((2, 3, 5, 7, 3), dtype=np.uint8), np.zeros((2, 3, 7, 5), dtype=np.uint8), np.zeros((3, 7, 5, 3), dtype=np.uint8)):
        with pytest.raises(ValueError, match="patches must be uint8"):
            e.rvncc_step_u8(bad, [0, 1])
        with pytest.raises(ValueError, match="patches must be uint8"):
            e.rvncc_scene_u8(bad, [0, 1])
    for routes in ([0, 2], [-1, 0], [0], [0.0, 1.0]):
        for call in (lambda: e.rvncc_step_u8(patches, routes), lambda: e.rvncc_sense_step(x, y, angs, routes),
                     lambda: e.rvncc_scene_u8(patches, routes), lambda: e.rvncc_scene(x, y, angs, routes)):
            with pytest.raises(ValueError, match="route_of_member"):
                call()
    bare = _engine_without_a_device(lib, first=None)
    for call in (lambda: bare.rvncc_step_u8(patches, [0, 1]), lambda: bare.rvncc_sense_step(x, y, angs, [0, 1]),
                 lambda: bare.rvncc_scene_u8(patches, [0, 1]), lambda: bare.rvncc_scene(x, y, angs, [0, 1])):
        with pytest.raises(N.EngineError, match="no route views"):
            call()
    assert lib.calls == []
    # ... and what passes reaches the one symbol of its call
    r = e.rvncc_step_u8(patches, [0, 1], channel=0)
    assert lib.calls == ["dv_rvncc_step_u8"] and r.angle_ncc.shape == (2, 3) and r.angle_view.shape == (2, 3)
    assert r.angle_familiarity is r.angle_ncc
    rows = e.rvncc_scene_u8(patches, [1, 0])
    assert lib.calls[-1] == "dv_rvncc_scene_u8" and [len(row) for row in rows] == [4, 5]
    e.rvncc_sense_step(x, y, angs, [0, 1])
    rows, flags = e.rvncc_scene(x, y, angs, [0, 1], want_flags=True)
    assert lib.calls[-2:] == ["dv_rvncc_sense_step", "dv_rvncc_scene"] and flags.shape == (2,)
    with pytest.raises(ValueError, match="a route holds at least 2"):                      # (why no case has a route of one view)
        navsim_amd.FamiliarityEngine._rviews_first([0, 1, 3], 3)


def test_the_plug_in_has_the_references_two_stage_shape():
    model = ncc_familiarity(1)
    assert model.metric == "ncc" and model.channel == 1 and callable(model.make_engine) and callable(model.from_engine)
    func = model.from_engine(_engine_without_a_device(HC.Recorder()), None)
    assert func.max_familiarity == 1.0 and func.metric == "ncc" and func.channel == 1
    with pytest.raises(ValueError, match="channel must be 0"):
        ncc_familiarity(3)
    with pytest.raises(ValueError, match="expected 'double'"):
        func(np.zeros((7, 5, 3), dtype=np.uint8), np.zeros(9, dtype=np.float32))
    assert "ncc_familiarity" in navsim_amd.__all__ and "NccRouteEnsemble" in navsim_amd.__all__


# ---- the ensembles' refusals ------------------------------------------------------------------------------------------------------------------
class _Engine(object):
    """An agent's engine for the refusals that never reach it."""


def _agent(model):
    a = navsim_amd.NavBySceneFamiliarity(synth.synth_landscape(3, 120, 4), (8, 8), 1.0, n_test_angles=5, use_gpu_sensor=False,
                                         familiarity_model=model)
    a._engine = _Engine()
    return a


def _routes():
    path = synth.sin_training_path(0.2, 30, 60, arclen=1.0)[:12]
    return [path, path + 3.0], [(0, tuple(path[2]), 0.3), (1, tuple(path[3] + 3.0), 0.1)]


def test_ncc_route_ensemble_refuses_the_other_models_by_name():
    RE = navsim_amd.NccRouteEnsemble
    assert issubclass(RE, navsim_amd.NavEnsemble) and not hasattr(RE, "relocalise")
    assert list(inspect.signature(RE.from_routes_with).parameters) == ["agent", "routes", "starts", "metrics"]
    assert list(inspect.signature(RE.from_landscapes).parameters) == ["agent", "landscapes", "routes", "starts", "metrics", "sensors", "noise"]
    routes, starts = _routes()
    with pytest.raises(ValueError, match="NccRouteEnsemble does not take an Infomax model: navsim_amd.InfomaxRouteEnsemble"):
        RE.from_routes(_agent(infomax_familiarity(seed=3)), routes, starts)
    with pytest.raises(ValueError, match="NccRouteEnsemble does not take a mushroom-body model: navsim_amd.MushroomRouteEnsemble"):
        RE.from_routes(_agent(mushroom_familiarity(n_kc=50, fan_in=4, seed=3)), routes, starts)
    with pytest.raises(ValueError, match="NccRouteEnsemble does not take a perfect-memory model: navsim_amd.SadsRouteEnsemble"):
        RE.from_routes(_agent(sads_familiarity(0.25)), routes, starts)
    with pytest.raises(ValueError, match="NccRouteEnsemble does not take an SSD model: navsim_amd.SsdRouteEnsemble"):
        RE.from_routes(_agent(ssd_familiarity(2)), routes, starts)
    host = navsim_amd.NavBySceneFamiliarity(synth.synth_landscape(3, 120, 4), (8, 8), 1.0, n_test_angles=5, use_gpu_sensor=False,
                                            familiarity_model=ncc_familiarity(2))
    with pytest.raises(ValueError, match="use_gpu_sensor=True"):
        RE.from_routes(host, routes, starts)
    with pytest.raises(ValueError, match="made from routes"):
        RE.from_agent(_agent(ncc_familiarity(2)), [((40.0, 40.0), 0.0)])
    with pytest.raises(ValueError, match="metrics must be one of"):
        RE.from_routes_with(_agent(ncc_familiarity(2)), routes, starts, metrics="gpu")


ROUTED = ("SadsRouteEnsemble", "SsdRouteEnsemble", "MushroomRouteEnsemble", "InfomaxRouteEnsemble")


@pytest.mark.parametrize("name", ROUTED)
def test_every_other_route_ensemble_refuses_an_ncc_model_and_points_to_its_own(name):
    routes, starts = _routes()
    with pytest.raises(ValueError, match="%s does not take an NCC model.*navsim_amd.NccRouteEnsemble" % name):
        getattr(navsim_amd, name).from_routes(_agent(ncc_familiarity(1)), routes, starts)


def _member(channel, bank=0):
    """What from_routes leaves of a member, as far as the constructors' checks read it."""
    a = _agent(ncc_familiarity(channel))
    a.training_path = _routes()[0][0]
    a._familiarity_func = a.familiarity_model.from_engine(a._engine, None)
    a.memory_bank = bank
    return a


def test_members_of_mixed_channels_and_foreign_ensembles_are_refused_by_name():
    a, b = _member(2), _member(0, 1)
    b._engine = a._engine
    b._familiarity_func = b.familiarity_model.from_engine(a._engine, None)
    with pytest.raises(ValueError, match="NccRouteEnsemble: member 1 compares channel 0, member 0 channel 2.*share one channel"):
        navsim_amd.NccRouteEnsemble([a, b])
    for other in (navsim_amd.NavEnsemble, navsim_amd.InfomaxEnsemble, navsim_amd.MushroomEnsemble, navsim_amd.MushroomRouteEnsemble,
                  navsim_amd.InfomaxRouteEnsemble, navsim_amd.SsdRouteEnsemble):
        with pytest.raises(ValueError, match="%s does not take a member of a NccRouteEnsemble" % other.__name__):
            other([a])
    with pytest.raises(ValueError, match="NccRouteEnsemble"):
        navsim_amd.SadsRouteEnsemble([a])
    with pytest.raises(ValueError, match="route 0 of the view store it shares: step it with its NccRouteEnsemble"):
        a.step_forward()
    with pytest.raises(ValueError, match="route 0 of the view store it shares.*clear_training would replace every member's routes"):
        a.clear_training()
    with pytest.raises(ValueError, match="route 0 of the view store it shares.*train_additional_path would replace every member's routes"):
        a.train_additional_path(_routes()[0][1])
    # a trained lone agent of the NCC model (no memory_bank) in the one-route ensembles
    lone = _member(2)
    lone.memory_bank = None
    for other in (navsim_amd.NavEnsemble, navsim_amd.InfomaxEnsemble, navsim_amd.MushroomEnsemble):
        with pytest.raises(ValueError, match="%s does not take an NCC model.*navsim_amd.NccRouteEnsemble" % other.__name__):
            other([lone])
    for foreign, name in ((ssd_familiarity(2), "SsdRouteEnsemble"), (sads_familiarity(0.25), "SadsRouteEnsemble")):
        m = _agent(foreign)
        m.memory_bank = 1
        with pytest.raises(ValueError, match="NccRouteEnsemble does not take a member of a %s" % name):
            navsim_amd.NccRouteEnsemble([m])
