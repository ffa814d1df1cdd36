"""Landscape sets, what needs no GPU: the conditions the inputs of tests/test_gpu_lands.py must meet (asserted on the host sensor model
and the NumPy statements, so that a passing GPU test cannot be vacuous), the binding surface of the new calls, and the Python-side
checks of the landscape tables, which are made before any library call."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from tests import helpers_infomax as HI
from tests import helpers_lands as HL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"dv_lands_set": "lands_set", "dv_lands_clear": "lands_clear", "dv_lands_info": "lands_info", "dv_lands_sense": "lands_sense",
         "dv_lands_mbank_train_from_poses": "mbank_train_from_poses", "dv_lands_ibank_train_from_poses": "ibank_train_from_poses",
         "dv_lands_mbank_sense_step": "mbank_sense_step_batch", "dv_lands_ibank_sense_step": "ibank_sense_step_batch"}


# ---- the inputs' conditions ------------------------------------------------------------------------------------------------------------------
def test_the_landscapes_have_the_shapes_and_the_odd_base():
    L = HL.lands()
    assert [l.shape[:2] for l in L] == [(300, 300), (211, 173), (173, 260), (300, 300)]
    assert (L[0].size + L[1].size) % 2 == 1                                               # L2's byte offset in the set
    assert np.array_equal(L[3], L[0][::-1, ::-1]) and L[3].flags.c_contiguous and not np.array_equal(L[3], L[0])
    assert len({l.shape for l in HL.same_shape_lands()}) == 1


@pytest.mark.parametrize("name", sorted(HL.SENSORS))
def test_sensed_poses_tell_the_landscapes_apart(name):
    s = HL.sense_case(name)
    assert s["land_of"].tolist() == list(HL.SENSE_PATTERN) * 2 and set(s["land_of"].tolist()) == {0, 1, 2, 3}
    assert s["scenes"].shape == (14,) + HL.SENSORS[name]["sensor"][::-1] + (3,)


def test_a_pose_on_the_wide_landscape_is_off_the_narrow_one_and_negative_indices_wrap_by_their_own_rows_and_columns():
    x, y, a = HL.ON_L2_OFF_L1
    assert not HL.is_off("sq", x, y, a, 2) and HL.is_off("sq", x, y, a, 1) and not HL.is_off("sq", x, y, a, 0)
    view = HL.wrap_facts("cols")
    assert not np.array_equal(view, HL.host_scene("sq", *HL.WRAP_POSE, 0))
    view = HL.wrap_facts("rows")
    assert not np.array_equal(view, HL.host_scene("sq", *HL.WRAP_ROW_POSE, 0))


@pytest.mark.parametrize("name", sorted(HL.SENSORS))
def test_training_inputs_interleave_routes_of_three_landscapes(name):
    t = HL.train_case(name)
    assert [len(f) for f in t["first"]] == list(HL.ROUTE_POINTS) and sorted(set(t["land_of"].tolist())) == [0, 1, 2]
    v, x, y = HL.off_own_landscape_view(name)
    assert t["land_of"][v] == 1 and 0 < v < len(t["x"]) - 1
    for channel in (0, 1, 2) if name == "px" else (2,):
        HL.mb_banks(name, channel)
        W0, Ws = HL.im_banks(name, channel)
        assert Ws.shape == (3,) + W0.shape
    if name == "sq":
        HL.mb_banks(name, 2, wide=True)                                                   # fan-in 16


@pytest.mark.parametrize("n,A", HL.LAYOUTS + (HL.WIDE_LAYOUT,))
def test_step_layouts_permute_under_a_sort_by_bank_and_straddle_the_slab_edge(n, A):
    c = HL.step_case("sq", n, A)
    assert c["banks"].tolist() == [HL.STEP_BANKS[i % 5] for i in range(n)] and c["lands"].tolist() == [HL.STEP_LANDS[i % 5] for i in range(n)]
    if (n, A) == HL.WIDE_LAYOUT:
        assert n * A == 8196 and 682 * A < 8192 < 683 * A and c["lands"][682] != c["lands"][0]
    mb, im = HL.mb_statement("sq", 2, c), HL.im_statement("sq", 2, c)
    assert mb.shape == im.shape == (n, A)
    assert len(np.unique(mb)) > 3 and mb.min() < 0
    # the landscape matters to the scores: member 1 (L1) scored on member 0's landscape (L0) would get other values
    if n >= 5:
        other = dict(c, planes=np.stack([HL.host_scenes("sq", [c["xs"][1]] * A, [c["ys"][1]] * A, c["angs"][1], [0] * A)]),
                     banks=c["banks"][1:2])
        assert not np.array_equal(HL.mb_statement("sq", 2, other)[0], mb[1])
        assert not np.array_equal(HL.im_statement("sq", 2, other)[0], im[1])
    if A > 1:
        print("lands %dx%d: least margin of an Infomax best heading %.2e" % (n, A, min(HI.best_margin(r) for r in im)))


def test_the_flagged_member_is_off_its_own_landscape_only():
    xs, ys, land_of = HL.flag_case("sq")
    assert land_of[2] == 1 and land_of.tolist() != list(HL.STEP_LANDS)


def test_ensemble_routes_lie_inside_their_own_landscapes():
    HL.ens_facts(HL.lands())
    HL.ens_facts(HL.same_shape_lands())
    routes = HL.ens_routes()
    assert [l for l, _ in routes] == [0, 0, 1, 1, 2, 2] and len(HL.ens_starts(routes)) == 12
    assert len(HL.footprint_facts()) == 9


# ---- binding surface -------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_engine_agree_on_the_lands_names():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    declared = set(re.findall(r"\bint\s+(dv_lands_[a-z0-9_]*)\s*\(", header))
    assert declared == set(NAMES) == {k for k in N.PROTOTYPES if k.startswith("dv_lands_")}
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert N.PROTOTYPES[name][0] is ctypes.c_int
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(N.PROTOTYPES[name][1]), name
        assert callable(getattr(navsim_amd.FamiliarityEngine, NAMES[name])), name
    # a call on a set is its twin with the landscape table behind the bank table
    for model in ("m", "i"):
        twin = N.PROTOTYPES["dv_%sbank_train_from_poses" % model][1]
        assert N.PROTOTYPES["dv_lands_%sbank_train_from_poses" % model][1] == twin[:6] + [N._i32p] + twin[6:]
        twin = N.PROTOTYPES["dv_%sbank_sense_step" % model][1]
        assert N.PROTOTYPES["dv_lands_%sbank_sense_step" % model][1] == twin[:7] + [N._i32p] + twin[7:]
    assert N.PROTOTYPES["dv_lands_sense"][1] == N.PROTOTYPES["dv_sense"][1][:4] + [N._i32p] + N.PROTOTYPES["dv_sense"][1][4:]


# ---- the Python-side checks: before any library call -------------------------------------------------------------------------------------
class _NoLibrary(object):
    def __getattr__(self, name):
        raise AssertionError("library call %s after a table that must be refused" % name)


def _engine(n_lands, banks=3):
    e = navsim_amd.FamiliarityEngine.__new__(navsim_amd.FamiliarityEngine)
    e._lib, e._ctx_raw, e._begun = _NoLibrary(), None, False
    e.n_lands, e.mb_banks, e.infomax_banks, e.sensor_shape = n_lands, banks, banks, (4, 4)
    return e


@pytest.mark.parametrize("table,match", [([0, -1, 0], r"\[1\] = -1 outside \[0, n_lands = 4\)"), ([0, 1, 4], r"\[2\] = 4 outside"),
                                         ([0, 1], "shape"), ([0, 1, 2, 3], "shape"), (np.array([0.0, 1.0, 2.0]), "integers"),
                                         ([[0, 1, 2]], "shape")])
def test_refused_landscape_tables_never_reach_the_library(table, match):
    e = _engine(4)
    z = np.zeros(3)
    for call in (lambda: e.mbank_train_from_poses(z, z, z, [0, 1, 2], land_of_view=table),
                 lambda: e.ibank_train_from_poses(z, z, z, [0, 1, 2], land_of_view=table),
                 lambda: e.mbank_sense_step_batch(z, z, np.zeros((3, 2)), [0, 1, 2], land_of_member=table),
                 lambda: e.ibank_sense_step_batch(z, z, np.zeros((3, 2)), [0, 1, 2], land_of_member=table),
                 lambda: e.lands_sense(z, z, z, table)):
        with pytest.raises(ValueError, match=match):
            call()
    with pytest.raises(N.EngineError, match="lands_set first"):
        _engine(0).lands_sense(z, z, z, [0, 0, 0])


def test_lands_set_refuses_what_is_no_list_of_hsv_landscapes():
    e = _engine(0)
    for bad, match in (([], "no landscapes"), ([np.zeros((4, 4), np.uint8)], r"uint8\[rows, cols, 3\]"),
                       ([np.zeros((4, 4, 3), np.float32)], "dtype"), ([np.zeros((4, 0, 3), np.uint8)], r"uint8\[rows, cols, 3\]")):
        with pytest.raises(ValueError, match=match):
            e.lands_set(bad)
    assert e.n_lands == 0


def test_from_landscapes_checks_its_arguments_before_it_trains():
    from navsim_amd import mushroom_familiarity
    agent = types.SimpleNamespace(familiarity_model=mushroom_familiarity(n_kc=100, fan_in=4, sparsity=0.1, seed=1), _engine=None,
                                  training_path=None, memory_bank=None)
    L = HL.lands()
    route = np.array([[50.0, 50.0], [51.0, 50.0], [52.0, 50.0]])
    for lands, routes, match in (([], [(0, route)], "landscapes"), ([L[0][..., 0]], [(0, route)], "landscapes"),
                                 (L, [route], r"routes\[0\] must be"), (L, [(4, route)], r"landscape_index 4 outside \[0, 4\)"),
                                 (L, [(True, route)], "landscape_index")):
        with pytest.raises(ValueError, match=match):
            navsim_amd.MushroomRouteEnsemble.from_landscapes(agent, lands, routes, [(0, (50.0, 50.0), 0.0)])
    with pytest.raises(ValueError, match="GPU"):                                           # (then the refusals of from_routes)
        navsim_amd.MushroomRouteEnsemble.from_landscapes(agent, L, [(1, route)], [(0, (50.0, 50.0), 0.0)])
    assert callable(navsim_amd.InfomaxRouteEnsemble.from_landscapes)
