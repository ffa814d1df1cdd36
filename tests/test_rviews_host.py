"""The route view store, what needs no GPU: the binding surface of dv_rviews_*, the Python-side checks (made before any library call),
SadsRouteEnsemble's refusals, and the NumPy restatement of the fast path's rule against oracle.step."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import infomax_familiarity, mushroom_familiarity, sads_familiarity, ssd_familiarity, synth
from oracle import oracle
from tests import helpers_rviews as HR
from tests.helpers import step_case_inputs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"dv_rviews_set_u8": "rviews_set_u8", "dv_rviews_set_from_poses": "rviews_set_from_poses", "dv_rviews_step_u8": "rviews_step_u8",
         "dv_rviews_sense_step": "rviews_sense_step", "dv_rviews_scene_u8": "rviews_scene_u8", "dv_rviews_scene": "rviews_scene",
         "dv_rviews_info": "rviews_info", "dv_rviews_clear": "rviews_clear"}


def test_header_bindings_and_engine_agree_on_the_rviews_names():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    declared = set(re.findall(r"\bint\s+(dv_rviews_[a-z0-9_]*)\s*\(", header))
    assert declared == set(NAMES) == {k for k in N.PROTOTYPES if k.startswith("dv_rviews_")}
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert N.PROTOTYPES[name][0] is ctypes.c_int
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(N.PROTOTYPES[name][1]), name
        assert callable(getattr(navsim_amd.FamiliarityEngine, NAMES[name])), name
    assert int(re.search(r"#define DV_RVIEWS_EXACT (\d+)u", header).group(1)) == N.DV_RVIEWS_EXACT
    # the sensed step is the uploaded one with poses for patches, the landscape table behind the weights, and the members' flags
    u8, sensed = N.PROTOTYPES["dv_rviews_step_u8"][1], N.PROTOTYPES["dv_rviews_sense_step"][1]
    assert sensed == [u8[0], N._f64p, N._f64p, N._f64p] + u8[2:6] + [N._i32p] + u8[6:] + [N._u32p]


class _NoLibrary(object):
    def __getattr__(self, name):
        raise AssertionError("library call %s after an argument that must be refused" % name)


def _engine(first=(0, 3, 8), shape=(4, 4), n_lands=0):
    e = navsim_amd.FamiliarityEngine.__new__(navsim_amd.FamiliarityEngine)
    e._lib, e._ctx_raw, e._begun = _NoLibrary(), None, False
    e.n_lands, e.sensor_shape = n_lands, shape
    e.rviews_first = None if first is None else np.array(first, dtype=np.int64)
    e.rviews_shape = None if first is None else shape
    return e


@pytest.mark.parametrize("first,match", [([0, 3], r"first\[1\] = 3, but there are 8 views"), ([1, 8], r"first\[0\] = 1"),
                                         ([0, 7, 8], r"first\[2\] = 8: route 1 would hold 1 views"), ([0, 5, 4, 8], r"route 1 would hold -1"),
                                         ([0], "shape"), ([[0, 8]], "shape"), ([0.0, 8.0], "integers")])
def test_refused_route_tables_never_reach_the_library(first, match):
    e = _engine(None)
    z = np.zeros(8)
    with pytest.raises(ValueError, match=match):
        e.rviews_set_u8(np.zeros((8, 4, 4, 3), np.uint8), first)
    with pytest.raises(ValueError, match=match):
        e.rviews_set_from_poses(z, z, z, first)
    assert e.rviews_first is None


def test_refused_views_and_patches_never_reach_the_library():
    e = _engine(None)
    for bad, match in ((np.zeros((8, 4, 4), np.uint8), r"uint8\[n, h, w, 3\]"), (np.zeros((8, 4, 4, 3), np.float32), "dtype"),
                       (np.zeros((8, 65, 64, 3), np.uint8), "4096")):
        with pytest.raises(ValueError, match=match):
            e.rviews_set_u8(bad, [0, 8])
    with pytest.raises(N.EngineError, match="no route views"):
        e.rviews_step_u8(np.zeros((2, 3, 4, 4, 3), np.uint8), [0, 1], [0.0, 0.0])
    e = _engine()
    for bad, match in ((np.zeros((2, 3, 4, 5, 3), np.uint8), r"uint8\[n, A, 4, 4, 3\]"), (np.zeros((2, 3, 4, 4, 3), np.int8), "dtype"),
                       (np.zeros((0, 3, 4, 4, 3), np.uint8), "n, A >= 1")):
        with pytest.raises(ValueError, match=match):
            e.rviews_step_u8(bad, [0, 1], [0.0, 0.0])
        with pytest.raises(ValueError, match=match):
            e.rviews_scene_u8(bad, [0, 1], [0.0, 0.0])


@pytest.mark.parametrize("routes,weights,match", [([0, 2], [0.0, 0.0], r"route_of_member\[1\] = 2 outside"), ([-1, 0], [0.0, 0.0], r"\[0\] = -1"),
                                                  ([0, 1, 1], [0.0, 0.0], "shape"), ([0.0, 1.0], [0.0, 0.0], "integers"),
                                                  ([0, 1], [0.0, 1.5], r"chem_weights\[1\] = 1.5 outside \[0, 1\]"),
                                                  ([0, 1], [np.nan, 0.5], r"chem_weights\[0\]"), ([0, 1], [0.0], "shape"),
                                                  ([0, 1], ["a", "b"], "numbers")])
def test_refused_step_tables_never_reach_the_library(routes, weights, match):
    e = _engine()
    patches, z, angs = np.zeros((2, 3, 4, 4, 3), np.uint8), np.zeros(2), np.zeros((2, 3))
    for call in (lambda: e.rviews_step_u8(patches, routes, weights), lambda: e.rviews_scene_u8(patches, routes, weights),
                 lambda: e.rviews_sense_step(z, z, angs, routes, weights), lambda: e.rviews_scene(z, z, angs, routes, weights)):
        with pytest.raises(ValueError, match=match):
            call()
    with pytest.raises(N.EngineError, match="lands_set first"):
        e.rviews_sense_step(z, z, angs, [0, 1], [0.0, 0.0], land_of_member=[0, 0])
    with pytest.raises(ValueError, match=r"land_of_member\[1\] = 3"):
        _engine(n_lands=3).rviews_sense_step(z, z, angs, [0, 1], [0.0, 0.0], land_of_member=[0, 3])
    with pytest.raises(ValueError, match="angles"):
        e.rviews_sense_step(z, z, np.zeros(3), [0, 1], [0.0, 0.0])


# ---- the ensemble ------------------------------------------------------------------------------------------------------------------------------
def _agent(model, engine=object(), **kw):
    return types.SimpleNamespace(familiarity_model=model, _engine=engine, training_path=None, memory_bank=None, **kw)


def test_the_ensemble_is_exported_and_refuses_the_other_models_and_agents():
    assert "SadsRouteEnsemble" in navsim_amd.__all__ and issubclass(navsim_amd.SadsRouteEnsemble, navsim_amd.NavEnsemble)
    route = np.array([[50.0, 50.0], [51.0, 50.0], [52.0, 50.0]])
    starts = [(0, (50.0, 50.0), 0.0)]
    E = navsim_amd.SadsRouteEnsemble
    for model, match in ((infomax_familiarity(n_hidden=4), "InfomaxRouteEnsemble steps that one"),
                         (mushroom_familiarity(n_kc=100, fan_in=4, sparsity=0.1, seed=1), "MushroomRouteEnsemble steps that one"),
                         (ssd_familiarity(), "perfect-memory model"), (lambda scenes: None, "perfect-memory model")):
        with pytest.raises(ValueError, match=match):
            E.from_routes(_agent(model), [route], starts)
    sads = sads_familiarity(0.25)
    with pytest.raises(ValueError, match="GPU"):
        E.from_routes(_agent(sads, engine=None), [route], starts)
    with pytest.raises(ValueError, match="UNTRAINED"):
        E.from_routes(types.SimpleNamespace(familiarity_model=sads, _engine=object(), training_path=route, memory_bank=None), [route], starts)
    for weights, match in (([0.5, 0.5], "2 weights for 1 starts"), ([1.5], r"\[0, 1\]")):
        with pytest.raises(ValueError, match=match):
            E.from_routes_with(_agent(sads), [route], starts, chem_weights=weights)
        with pytest.raises(ValueError, match=match):
            E.from_landscapes(_agent(sads), [np.zeros((9, 9, 3), np.uint8)], [(0, route)], starts, chem_weights=weights)
    with pytest.raises(ValueError, match="route_index 1 outside"):
        E.from_routes(_agent(sads), [route], [(1, (50.0, 50.0), 0.0)])
    with pytest.raises(ValueError, match="metrics"):
        E.from_routes_with(_agent(sads), [route], starts, metrics="gpu")
    with pytest.raises(ValueError, match="from_routes"):
        E.from_agent(_agent(sads), [((1.0, 1.0), 0.0)])


def test_a_routed_member_steps_with_its_ensemble_only_and_the_other_ensembles_name_it():
    land = synth.synth_landscape(3, 120, 4)
    a = navsim_amd.NavBySceneFamiliarity(land, (8, 8), 1.0, n_test_angles=5, use_gpu_sensor=False, familiarity_model=sads_familiarity(0.25))
    a.memory_bank = 2
    with pytest.raises(ValueError, match="route 2 of the view store .*SadsRouteEnsemble"):
        a.step_forward()
    eng = object()
    member = types.SimpleNamespace(familiarity_model=sads_familiarity(0.25), _engine=eng, training_path=np.zeros((3, 2)), memory_bank=1,
                                   _familiarity_func=types.SimpleNamespace(engine=eng, chem_weight=0.25), track_scene_familiarity=False)
    for cls in (navsim_amd.NavEnsemble, navsim_amd.InfomaxEnsemble, navsim_amd.MushroomEnsemble):
        with pytest.raises(ValueError, match="%s does not take a member of a SadsRouteEnsemble: its route is route 1 of" % cls.__name__):
            cls._check_member(member)
    for cls in (navsim_amd.MushroomRouteEnsemble, navsim_amd.InfomaxRouteEnsemble):
        with pytest.raises(ValueError, match=cls.__name__ + " takes agents of the"):
            cls._check_member(member)
    navsim_amd.SadsRouteEnsemble._check_member(member)                                    # the one that takes it
    # the two banked models' names are what they were
    for metric, name in (("mushroom", "MushroomRouteEnsemble"), ("infomax", "InfomaxRouteEnsemble")):
        banked = types.SimpleNamespace(familiarity_model=types.SimpleNamespace(metric=metric), memory_bank=0)
        with pytest.raises(ValueError, match="NavEnsemble does not take a member of a %s: its route is kept in memory bank 0" % name):
            navsim_amd.NavEnsemble._check_member(banked)
        with pytest.raises(ValueError, match="SadsRouteEnsemble does not take"):
            navsim_amd.SadsRouteEnsemble._check_member(banked)


# ---- the rule of the fast path ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s_ties_8x8", "s_ties_8x8_cw", "s_ties_4x4"])
def test_the_statement_gives_the_tie_fixtures_record(manifest, golden, name):
    case = [c for c in manifest["t2_step"] if c["name"] == name][0]
    lib, patches = step_case_inputs(case)
    fam, view, best, most = HR.statement(lib, patches, case["chem_weight"])
    assert fam.tobytes() == golden("t2_step.npz")[name + "_angle"].tobytes() and best == case["best_idex"]
    assert view[best] == case["best_view"] and fam[best] == case["step_familiarity"] and most >= 1
    print("%s: most candidates of a column %d (the list holds %d)" % (name, most, HR.CAND_CAP))


def test_the_window_never_drops_the_true_maximum_on_2000_random_small_routes():
    rng = np.random.default_rng(77)
    several = 0
    for k in range(2000):
        h, w = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        F, A = int(rng.integers(2, 40)), int(rng.integers(1, 5))
        if k % 2:
            views, patches = synth.synth_views(k, F, h, w), synth.synth_patches(k, A, h, w)
        else:
            views, patches = synth.random_hsv(k, (F, h, w, 3)), synth.random_hsv(k + 5000, (A, h, w, 3))
        if k % 5 == 0:
            views[F // 2:] = views[:F - F // 2]                                           # repeated views: ties
        cw = (0.0, 0.3, 1.0, float(rng.uniform()))[k % 4]
        fam, view, best, most = HR.statement(views, patches, cw)
        want = oracle.step(views, patches, cw)
        assert fam.tobytes() == want["angle_familiarity"].tobytes() and best == want["best_idex"] and view[best] == want["best_view"], k
        several += most > 1
    assert several > 200


def test_the_step_inputs_are_what_the_gpu_tests_say():
    c = HR.step_case(19, 17, 10, "levels")
    assert c["first"].tolist() == [0, 2, 65, 129, 194, 1237, 1242] and 5 not in c["routes"]
    assert (np.argsort(c["routes"], kind="stable") != np.arange(7)).any() and (7 * 5) % 4 and (19 * 17) % 4
    assert HR.slab_columns(1043) == 7710 and 7710 % 260 and 30 * 260 > 7710
    assert HR.WIDE_ROUTES[HR.sorted_member_at(HR.WIDE_ROUTES, 260, 7710)] != HR.WIDE_ROUTES[0]
    assert c["routes"][HR.sorted_member_at(c["routes"], 10, 37)] != c["routes"][0]
    views, patch = HR.permuted_route(8, 8, 40, 3)
    s_hs, s_v = oracle.int_sums(views, patch)
    assert len(set(s_hs.tolist())) == 1 and len(set(s_v.tolist())) == 1
    assert len(set(oracle.sads_hsv(views, patch, 0.3).tolist())) > 1                      # equal integer sums, different sequential doubles
