"""Sensor tables, what needs no GPU: the conditions the inputs of tests/test_gpu_sensors.py must meet (asserted on the host sensor model
and the NumPy statements, so that a passing GPU test cannot be vacuous), the binding surface of the new calls, the Python-side checks,
which are made before any library call, and the resources of the new kernel forms."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from tests import helpers_lands as HL
from tests import helpers_sensors as HS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"dv_sensors_set": "sensors_set", "dv_sensors_clear": "sensors_clear", "dv_sensors_info": "sensors_info"}


# ---- the inputs' conditions ------------------------------------------------------------------------------------------------------------------
def test_the_engines_own_configuration_is_none_of_the_entries():
    own = HS.ENTRIES["OWN"]
    assert all(c != own for e, c in HS.ENTRIES.items() if e != "OWN")
    assert all(c["pixel"][1] % 2 == 0 for c in HS.ENTRIES.values())                       # the thin shape's extent 5 * ph is even
    e1, e3, e0, e4 = (HS.ENTRIES[k] for k in ("E1", "E3", "E0", "E4"))
    assert (e1["pixel"], e1["mask"]) == (e3["pixel"], e3["mask"]) and e1["levels"] != e3["levels"]
    assert (e0["pixel"], e0["levels"]) == (e4["pixel"], e4["levels"]) and e0["mask"] != e4["mask"]
    assert not np.array_equal(HS.level_table("wide", "E1"), HS.level_table("wide", "E3"))


@pytest.mark.parametrize("shape", sorted(HS.SHAPES))
def test_every_pair_of_configurations_gives_different_views_on_every_pose(shape):
    s = HS.sense_case(shape)                                                              # (asserts the pairwise differences)
    w, h = HS.SHAPES[shape]
    assert s["scenes"].shape == (14, h, w, 3) and s["land_of"].tolist() == list(HL.SENSE_PATTERN) * 2
    assert len(s["on0"]) == 4 and all(not np.array_equal(s["twice"][k], s["scenes"][v]) for k, v in enumerate(s["on0"]))
    if shape == "thin":
        assert (w * h) % 64 != 0 and 64 // (w * h) >= 2                                   # a wavefront spans poses of different entries


@pytest.mark.parametrize("shape", sorted(HS.SHAPES))
def test_the_footprint_pose_is_on_the_landscape_under_the_small_entry_and_off_it_under_the_large_one(shape):
    x, y, ang, land_of, scenes = HS.foot_case(shape)
    assert [s is None for s in scenes] == [False, False, True, False]
    assert HS.FOOT_SET[1][0] == HS.FOOT_SET[2][0] == 1 and HL.lands()[1].shape[:2] == (211, 173)
    with pytest.raises(IndexError):
        HS.host_scene(shape, "E2", x[2], y[2], ang[2], 1)


@pytest.mark.parametrize("shape", sorted(HS.SHAPES))
def test_training_and_step_inputs_are_sensed_under_their_own_entries(shape):
    t = HS.train_case(shape)
    assert sorted(set(t["land_of"].tolist())) == [0, 1, 2] and t["land_of"][:6].tolist() == [0, 1, 2, 0, 1, 2]
    HS.mb_banks(shape)
    W0, Ws = HS.im_banks(shape)
    assert Ws.shape == (3,) + W0.shape
    for n, A in HL.LAYOUTS + ((HL.WIDE_LAYOUT,) if shape == "wide" else ()):
        c = HS.step_case(shape, n, A)
        mb, im = HS.mb_statement(shape, c), HS.im_statement(shape, c)
        assert mb.shape == im.shape == (n, A) and len(np.unique(mb)) > 2
        if (n, A) == HL.WIDE_LAYOUT:
            assert 682 * A < 8192 < 683 * A and HS.TABLE[c["lands"][682]] != HS.TABLE[c["lands"][0]]


def test_ensemble_routes_and_starts_meet_their_own_entries_footprints():
    HS.ens_facts()
    assert len(HS.edge_facts()) == 9
    assert all((c or {}).get("sensor_pixel_dimensions", [1, 2])[1] % 2 == 0 for c in HS.ENS_SENSORS[1:])


# ---- binding surface -------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_engine_agree_on_the_sensors_names_and_the_lands_names_are_the_eight():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    declared = set(re.findall(r"\bint\s+(dv_sensors_[a-z0-9_]*)\s*\(", header))
    assert declared == set(NAMES) == {k for k in N.PROTOTYPES if k.startswith("dv_sensors_")}
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert N.PROTOTYPES[name][0] is ctypes.c_int
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(N.PROTOTYPES[name][1]), name
        assert callable(getattr(navsim_amd.FamiliarityEngine, NAMES[name])), name
    assert navsim_amd.FamiliarityEngine.n_sensors == 0
    lands = set(re.findall(r"\bint\s+(dv_lands_[a-z0-9_]*)\s*\(", header))
    assert len(lands) == 8 and lands == {k for k in N.PROTOTYPES if k.startswith("dv_lands_")}


# ---- the Python-side checks: before any library call -----------------------------------------------------------------------------------------
class _NoLibrary(object):
    def __getattr__(self, name):
        raise AssertionError("library call %s after arguments that must be refused" % name)


def _engine(n_lands, sensor=(16, 8)):
    e = navsim_amd.FamiliarityEngine.__new__(navsim_amd.FamiliarityEngine)
    e._lib, e._ctx_raw, e._begun = _NoLibrary(), None, False
    e.n_lands, e.sensor_shape = n_lands, (sensor[1], sensor[0])
    return e


def test_refused_sensor_tables_never_reach_the_library():
    px, luts, masks = HS.table_args("wide", HS.TABLE)
    e = _engine(4)
    for bad, match in (((px[:3], luts, masks), r"pixel_dimensions must have shape \(4, 2\)"),
                       ((px, luts[:3], masks), r"luts must have shape \(4, 3, 256\)"),
                       ((px, luts, masks[:3]), r"masks must have shape \(4,\)"),
                       ((np.array(px, dtype=np.float64), luts, masks), "pixel_dimensions must hold integers"),
                       ((px, luts.astype(np.int32), masks), "luts must be uint8"),
                       ((px, luts, np.array(masks, dtype=np.float32)), "masks must hold integers"),
                       (([(1, 2), (64, 65), (3, 2), (2, 4)], luts, masks), r"pixel_dimensions\[1\] = \(64, 65\)"),
                       (([(1, 2), (2, 4), (0, 2), (2, 4)], luts, masks), r"pixel_dimensions\[2\] = \(0, 2\)"),
                       ((px, luts, [0, 1, 9, 1]), r"masks\[2\] = 9 outside \[0, w / 2 = 8\]"),
                       ((px, luts, [0, -1, 2, 1]), r"masks\[1\] = -1 outside")):
        with pytest.raises(ValueError, match=match):
            e.sensors_set(*bad)
    assert e.n_sensors == 0
    with pytest.raises(N.EngineError, match="lands_set first"):
        _engine(0).sensors_set(px, luts, masks)


def _agent(**kw):
    from navsim_amd import mushroom_familiarity
    a = navsim_amd.NavBySceneFamiliarity(np.array(HL.lands()[0]), HL.ENS_SENSOR, 1.0, n_test_angles=9, use_gpu_sensor=False,
                                         familiarity_model=mushroom_familiarity(n_kc=100, fan_in=4, sparsity=0.1, seed=1), **kw)
    a._engine = _NoLibrary()                                                              # an engine that must never be called
    return a


def test_from_landscapes_refuses_bad_sensors_before_it_touches_the_engine():
    L = list(HL.lands()[:3])
    routes = HL.ens_routes()
    starts = HL.ens_starts(routes)
    good = list(HS.ENS_SENSORS)
    for cls in (navsim_amd.MushroomRouteEnsemble, navsim_amd.InfomaxRouteEnsemble, navsim_amd.SadsRouteEnsemble):
        for bad, match in ((good[:2], "sensors holds 2 entries for 3 landscapes"),
                           ([None, dict(sensor_dimensions=[12, 10]), None], "w × h is the engine's one"),
                           ([None, dict(sensor_pixel_dimensions=[1.0, 2.0]), None], r"sensors\[1\]: sensor_pixel_dimensions"),
                           ([None, None, dict(sensor_pixel_dimensions=[64, 66])], r"sensors\[2\]: sensor_pixel_dimensions"),
                           ([dict(mask_middle_n=7), None, None], r"sensors\[0\]: mask_middle_n 7 outside \[0, w / 2 = 6\]"),
                           ([None, dict(n_sensor_levels=1), None], r"sensors\[1\]: n_sensor_levels"),
                           ([None, dict(levels=4), None], r"sensors\[1\]: unknown keys"),
                           ([None, (1, 2), None], r"sensors\[1\] must be None or a dict")):
            with pytest.raises(ValueError, match=match):
                cls.from_landscapes(_agent(), L, routes, starts, sensors=bad)


def test_sensor_entries_take_the_agents_values_for_missing_keys_and_its_level_arithmetic():
    a = _agent(sensor_pixel_dimensions=[1, 2], n_sensor_levels=7, mask_middle_n=1)
    entries = navsim_amd.MushroomRouteEnsemble._sensor_entries(a, 3, HS.ENS_SENSORS)
    assert [e["index"] for e in entries] == [0, 1, 2]
    assert [e["sensor_pixel_dimensions"].tolist() for e in entries] == [[1, 2], [1, 2], [2, 2]]
    assert [e["n_sensor_levels"] for e in entries] == [(256, 256, 7), (256, 256, 4), (256, 256, 7)]
    assert [e["mask_middle_n"] for e in entries] == [1, 1, 2]
    assert np.array_equal(entries[0]["lut"], a._level_tables()) and not np.array_equal(entries[1]["lut"], entries[0]["lut"])
    b = _agent(n_sensor_levels=4)
    assert np.array_equal(entries[1]["lut"], b._level_tables()) and a.n_sensor_levels == (256, 256, 7)
    # a member carries its entry: its bounds are its own footprint's
    import copy
    m = navsim_amd.MushroomRouteEnsemble._on_landscape(copy.copy(a), HL.lands()[1], entries[2])
    assert m.sensor_index == 2 and m._sensor_r == 12.0 and m._bounds_tuple() == (12.0, 173 - 12.0, 211 - 12.0)
    assert a.sensor_index is None and a._sensor_r == 10.0 and a.sensor_pixel_dimensions.tolist() == [1, 2]


# ---- the new kernel forms ----------------------------------------------------------------------------------------------------------------------
def test_the_sensor_table_kernel_forms_use_no_scratch():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = {r["name"]: r for r in kernel_resources.kernel_table()}
    for name in ("k_sense_lands_sensors", "k_mb_pose_bank_lands_sensors", "k_sense_lands", "k_mb_pose_bank_lands"):
        assert name in rows, name
        assert rows[name]["scratch"] == 0 and rows[name]["vgpr_spills"] == 0, rows[name]
