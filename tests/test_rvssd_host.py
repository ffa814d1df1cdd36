"""SSD on the route view store without a device: the helper's expected value held to oracle.ssds, the NumPy restatement of the scoring
kernel on the extreme cases, the binding surface of the dv_rvssd_* calls, the engine's refusals (raised before any library call), the
launch-bound constants of csrc/dejavu_rvssd.inl, and the refusals of SsdRouteEnsemble and of the other ensembles."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import infomax_familiarity, mushroom_familiarity, sads_familiarity, ssd_familiarity, synth
from oracle import oracle
from tests import helpers_rvssd as HV

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"dv_rvssd_step_u8": "rvssd_step_u8", "dv_rvssd_sense_step": "rvssd_sense_step", "dv_rvssd_scene_u8": "rvssd_scene_u8",
         "dv_rvssd_scene": "rvssd_scene"}


# ---- the expected value ----------------------------------------------------------------------------------------------------------------------
def test_the_helpers_statement_is_the_oracles_ssds_on_a_handful_of_pairs():
    rng = np.random.default_rng(3)
    pairs = [(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)) for h, w in ((3, 3), (7, 5), (8, 8), (64, 64))]
    pairs.append((np.zeros((64, 64), dtype=np.uint8), np.full((64, 64), 255, dtype=np.uint8)))
    pairs.append((np.array([[0, 127, 128, 255]], dtype=np.uint8), np.array([[255, 128, 127, 0]], dtype=np.uint8)))
    for a, b in pairs:
        want = oracle.ssds(a, b)
        assert want == float(int(want)) and HV.ssd_pair(a, b) == int(want) == HV.ssd_pair(b, a)
    assert HV.ssd_pair(*pairs[4]) == HV.MAX_SSD == 266342400 < 2 ** 31


def test_the_cases_hold_what_the_gpu_tests_rely_on():
    for h, w in ((3, 3), (7, 5), (8, 8)):
        HV.tail_case(h, w)
    c = HV.edge_byte_case()
    assert set(np.unique(c["views"]).tolist()) == set(np.unique(c["patches"]).tolist()) == set(HV.EDGE_BYTES)
    for plant in (False, True):
        HV.lengths_case(plant)
    for second in (40, 70):
        HV.tie_case(second)
    for name in HV.GEOMETRIES:
        HV.geometry_case(name)


# ---- the kernel's arithmetic in NumPy ----------------------------------------------------------------------------------------------------------
def _statement_equals_expected(c, channel):
    want = HV.expected(c["views"], c["first"], c["patches"], c["routes"], channel)
    for i, r in enumerate(c["routes"]):
        ssd, view = HV.kernel_statement(c["views"][c["first"][r]:c["first"][r + 1]], c["patches"][i], channel)
        assert np.array_equal(ssd, want[0][i].astype(np.int64)) and np.array_equal(view, want[1][i]), (i, channel)


@pytest.mark.parametrize("channel", (0, 1, 2))
def test_kernel_statement_on_the_7x5_tail(channel):
    """P = 35, Pw = 9: the second K-step holds 3 real pixels, 1 byte of the store's zero padding and 7 dwords that are not loaded."""
    _statement_equals_expected(HV.tail_case(7, 5), channel)


def test_kernel_statement_on_the_64x64_extremes_and_the_sign_edges():
    _statement_equals_expected(HV.extreme_case(), 2)
    _statement_equals_expected(HV.edge_byte_case(), 2)


def test_kernel_statement_masks_the_padding_views_and_keeps_the_least_index():
    c = HV.lengths_case(False)
    _statement_equals_expected(c, 2)
    # unmasked, a padding view (zero bytes) would be the all-zero patch's best view on every route that has padding
    lib = np.concatenate([c["views"][:2], np.zeros((62, 5, 5, 3), dtype=np.uint8)])
    ssd, view = HV.kernel_statement(lib, c["patches"][1], 2)
    assert ssd[0] == 0 and view[0] == 2 and HV.kernel_statement(lib[:2], c["patches"][1], 2)[1][0] < 2
    for second in (40, 70):
        _statement_equals_expected(HV.tie_case(second), 2)


# ---- binding surface -------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_engine_agree_on_the_rvssd_names():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    declared = set(re.findall(r"\bint\s+(dv_rvssd_[a-z0-9_]*)\s*\(", header))
    assert declared == set(NAMES) == {k for k in N.PROTOTYPES if k.startswith("dv_rvssd_")}
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert N.PROTOTYPES[name][0] is ctypes.c_int
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(N.PROTOTYPES[name][1]), name
        assert callable(getattr(navsim_amd.FamiliarityEngine, NAMES[name])), name
    P = N.PROTOTYPES
    # the SSD calls are the store's calls without the weights and the flag word, the channel behind the tables
    assert P["dv_rvssd_step_u8"][1] == P["dv_rviews_step_u8"][1][:5] + [ctypes.c_int] + P["dv_rviews_step_u8"][1][7:]
    assert P["dv_rvssd_sense_step"][1] == P["dv_rviews_sense_step"][1][:7] + [N._i32p, ctypes.c_int] + P["dv_rviews_sense_step"][1][10:]
    assert P["dv_rvssd_scene_u8"][1] == P["dv_rviews_scene_u8"][1][:5] + [ctypes.c_int] + P["dv_rviews_scene_u8"][1][6:]
    assert P["dv_rvssd_scene"][1] == P["dv_rviews_scene"][1][:7] + [N._i32p, ctypes.c_int] + P["dv_rviews_scene"][1][9:]
    # the u8 and the sensed forms agree on the order of what they share: counts, routes, (landscapes,) channel, outputs
    assert P["dv_rvssd_sense_step"][1][4:7] == P["dv_rvssd_step_u8"][1][2:5] and P["dv_rvssd_sense_step"][1][8:12] == P["dv_rvssd_step_u8"][1][5:9]
    assert P["dv_rvssd_scene"][1][4:7] == P["dv_rvssd_scene_u8"][1][2:5] and P["dv_rvssd_scene"][1][8:11] == P["dv_rvssd_scene_u8"][1][5:8]
    E = navsim_amd.FamiliarityEngine
    assert list(inspect.signature(E.rvssd_step_u8).parameters) == ["self", "patches", "route_of_member", "channel"]
    assert list(inspect.signature(E.rvssd_sense_step).parameters) == ["self", "x", "y", "angles", "route_of_member", "channel", "land_of_member"]
    assert inspect.signature(E.rvssd_step_u8).parameters["channel"].default == 2
    assert inspect.signature(E.rvssd_sense_step).parameters["channel"].default == 2


def test_the_launch_bounds_of_the_source_are_the_helpers():
    src = open(os.path.join(REPO, "navigation-by-deja-vu_amd", "csrc", "dejavu_rvssd.inl")).read()
    got = {k: int(v) for k, v in re.findall(r"constexpr int (kRvssd[A-Za-z]*) = (\d+);", src)}
    assert got == {"kRvssdTile": HV.TILE, "kRvssdGroupsPerBlock": HV.GROUPS_PER_BLOCK, "kRvssdTilesPerLaunch": HV.TILES_PER_LAUNCH}
    assert HV.TILE == 32 and HV.TILES_PER_LAUNCH <= 65535                                 # the MFMA's M; a grid's y
    assert "for (int t0 = 0; t0 < p.n_tiles; t0 += kRvssdTilesPerLaunch)" in src           # the launches loop over the bound


# ---- the engine's refusals come before the library --------------------------------------------------------------------------------------------
def _engine_without_a_device(lib, shape=(7, 5), first=(0, 5, 9)):
    e = navsim_amd.FamiliarityEngine.__new__(navsim_amd.FamiliarityEngine)
    e._lib, e._ctx_raw, e._begun, e.sensor_shape = lib, None, False, shape
    if first is not None:
        e.rviews_first, e.rviews_shape = np.array(first, dtype=np.int64), shape
    return e


def test_refusals_come_before_any_library_call():
    lib = HV.Recorder()
    e = _engine_without_a_device(lib)
    patches = np.zeros((2, 3, 7, 5, 3), dtype=np.uint8)
    x, y, angs = [50.0, 60.0], [50.0, 60.0], np.zeros((2, 3))
    for channel in (3, -1, 1.0, True, None):
        for call in (lambda: e.rvssd_step_u8(patches, [0, 1], channel), lambda: e.rvssd_scene_u8(patches, [0, 1], channel),
                     lambda: e.rvssd_sense_step(x, y, angs, [0, 1], channel), lambda: e.rvssd_scene(x, y, angs, [0, 1], channel)):
            with pytest.raises(ValueError, match="channel must be 0, 1 or 2"):
                call()
    for bad in (np.zeros((2, 3, 5, 7, 3), dtype=np.uint8), np.zeros((2, 3, 7, 5), dtype=np.uint8), np.zeros((3, 7, 5, 3), dtype=np.uint8)):
        with pytest.raises(ValueError, match="patches must be uint8"):
            e.rvssd_step_u8(bad, [0, 1])
        with pytest.raises(ValueError, match="patches must be uint8"):
            e.rvssd_scene_u8(bad, [0, 1])
    for routes in ([0, 2], [-1, 0], [0], [0.0, 1.0]):
        for call in (lambda: e.rvssd_step_u8(patches, routes), lambda: e.rvssd_sense_step(x, y, angs, routes),
                     lambda: e.rvssd_scene_u8(patches, routes), lambda: e.rvssd_scene(x, y, angs, routes)):
            with pytest.raises(ValueError, match="route_of_member"):
                call()
    bare = _engine_without_a_device(lib, first=None)
    for call in (lambda: bare.rvssd_step_u8(patches, [0, 1]), lambda: bare.rvssd_sense_step(x, y, angs, [0, 1]),
                 lambda: bare.rvssd_scene_u8(patches, [0, 1]), lambda: bare.rvssd_scene(x, y, angs, [0, 1])):
        with pytest.raises(N.EngineError, match="no route views"):
            call()
    assert lib.calls == []
    # ... and what passes reaches the one symbol of its call
    r = e.rvssd_step_u8(patches, [0, 1], channel=0)
    assert lib.calls == ["dv_rvssd_step_u8"] and r.angle_ssd.shape == (2, 3) and r.angle_view.shape == (2, 3)
    rows = e.rvssd_scene_u8(patches, [1, 0])
    assert lib.calls[-1] == "dv_rvssd_scene_u8" and [len(row) for row in rows] == [4, 5]


def test_angle_familiarity_is_the_negated_row_with_the_lone_agents_zero():
    from navsim_amd.engine import RouteSsdResults
    ssd = np.array([[0.0, 5.0]])
    r = RouteSsdResults(ssd, np.zeros((1, 2), dtype=np.int64), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.uint32))
    assert r.angle_ssd is ssd and r.angle_familiarity.tolist() == [[0.0, -5.0]] and np.signbit(r.angle_familiarity[0, 0])


# ---- the ensemble's refusals ------------------------------------------------------------------------------------------------------------------
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


def test_ssd_route_ensemble_is_exported_and_refuses_the_other_models_by_name():
    RE = navsim_amd.SsdRouteEnsemble
    assert "SsdRouteEnsemble" in navsim_amd.__all__ and issubclass(RE, navsim_amd.NavEnsemble)
    assert RE.from_routes.__func__ is navsim_amd.SadsRouteEnsemble.from_routes.__func__
    for name in ("from_routes", "from_routes_with", "from_landscapes"):
        assert callable(getattr(RE, name))
    assert "metrics" in inspect.signature(RE.from_routes_with).parameters and "sensors" in inspect.signature(RE.from_landscapes).parameters
    routes, starts = _routes()
    with pytest.raises(ValueError, match="SsdRouteEnsemble does not take an Infomax model: navsim_amd.InfomaxRouteEnsemble"):
        RE.from_routes(_agent(infomax_familiarity(seed=3)), routes, starts)
    with pytest.raises(ValueError, match="SsdRouteEnsemble does not take a mushroom-body model: navsim_amd.MushroomRouteEnsemble"):
        RE.from_routes(_agent(mushroom_familiarity(n_kc=50, fan_in=4, seed=3)), routes, starts)
    with pytest.raises(ValueError, match="SsdRouteEnsemble does not take a perfect-memory model: navsim_amd.SadsRouteEnsemble"):
        RE.from_routes(_agent(sads_familiarity(0.25)), routes, starts)
    host = navsim_amd.NavBySceneFamiliarity(synth.synth_landscape(3, 120, 4), (8, 8), 1.0, n_test_angles=5, use_gpu_sensor=False,
                                            familiarity_model=ssd_familiarity(2))
    with pytest.raises(ValueError, match="use_gpu_sensor=True"):
        RE.from_routes(host, routes, starts)
    with pytest.raises(ValueError, match="made from routes"):
        RE.from_agent(_agent(ssd_familiarity(2)), [((40.0, 40.0), 0.0)])


def test_sads_route_ensemble_still_refuses_ssd_and_names_the_ensemble_that_steps_it():
    routes, starts = _routes()
    with pytest.raises(ValueError, match="perfect-memory model.*SsdRouteEnsemble"):
        navsim_amd.SadsRouteEnsemble.from_routes(_agent(ssd_familiarity(1)), routes, starts)


def _member(channel, bank=0):
    """What from_routes leaves of a member, as far as the constructors' checks read it."""
    a = _agent(ssd_familiarity(channel))
    a.training_path = _routes()[0][0]
    a._familiarity_func = a.familiarity_model.from_engine(a._engine, None)
    a.memory_bank = bank
    return a


def test_members_of_mixed_channels_and_foreign_ensembles_are_refused_by_name():
    a, b = _member(2), _member(0, 1)
    b._engine = a._engine
    b._familiarity_func = b.familiarity_model.from_engine(a._engine, None)
    with pytest.raises(ValueError, match="member 1 compares channel 0, member 0 channel 2.*share one channel"):
        navsim_amd.SsdRouteEnsemble([a, b])
    for other in (navsim_amd.NavEnsemble, navsim_amd.InfomaxEnsemble, navsim_amd.MushroomEnsemble, navsim_amd.MushroomRouteEnsemble,
                  navsim_amd.InfomaxRouteEnsemble):
        with pytest.raises(ValueError, match="%s does not take a member of a SsdRouteEnsemble" % other.__name__):
            other([a])
    with pytest.raises(ValueError, match="SsdRouteEnsemble"):
        navsim_amd.SadsRouteEnsemble([a])
    with pytest.raises(ValueError, match="route 0 of the view store it shares: step it with its SsdRouteEnsemble"):
        a.step_forward()
    sads = _agent(sads_familiarity(0.25))
    sads.memory_bank = 1
    with pytest.raises(ValueError, match="SsdRouteEnsemble does not take a member of a SadsRouteEnsemble"):
        navsim_amd.SsdRouteEnsemble([sads])
