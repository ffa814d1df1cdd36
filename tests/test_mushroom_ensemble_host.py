"""Ensembles of mushroom-body agents, host side (no GPU): the C ABI's two batch calls in the header, the binding and the library, who
MushroomEnsemble, NavEnsemble and InfomaxEnsemble refuse, the engine methods' shape checks (made before any device call), and the
conditions that the patch sets of the GPU tests must satisfy under the NumPy statement (tests/helpers_mushroom_ensemble.py)."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import infomax_familiarity, mushroom_familiarity, synth
from tests import helpers_mushroom as H
from tests import helpers_mushroom_ensemble as HE
from tests.conftest import REPO

LAND = synth.synth_landscape(5, 200, 4)
PATH = np.stack([np.linspace(50, 150, 40), np.full(40, 100.0)], axis=1)
POSES = [((60.0, 100.5), 0.1), ((80.0, 99.0), 6.1)]
BATCH = ("dv_batch_mb_step_u8", "dv_batch_mb_sense_step")


def _agent(model):
    return navsim_amd.NavBySceneFamiliarity(LAND, (8, 8), 2.0, n_test_angles=4, use_gpu_sensor=False, familiarity_model=model)


def _like(metric, engine, func_engine, trained=True):
    """What an ensemble class looks at in an agent, without a device."""
    return SimpleNamespace(_engine=engine, familiarity_model=SimpleNamespace(metric=metric), training_path=PATH if trained else None,
                           _familiarity_func=SimpleNamespace(engine=func_engine, metric=metric) if trained else None)


def test_batch_calls_are_declared_bound_and_exported():
    i32p, u32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32)
    assert N.PROTOTYPES["dv_batch_mb_step_u8"] == (ctypes.c_int, [N._ctx_p, N._u8p, ctypes.c_int, ctypes.c_int, N._f64p, i32p])
    assert N.PROTOTYPES["dv_batch_mb_sense_step"] == (ctypes.c_int, [N._ctx_p, N._f64p, N._f64p, N._f64p, ctypes.c_int, ctypes.c_int,
                                                                     N._f64p, i32p, u32p])
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    lib = N.load()
    for name in BATCH:
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(N.PROTOTYPES[name][1]), name                  # argument counts as the header declares them
        assert hasattr(lib, name), name
    for name in ("mb_step_batch_u8", "mb_sense_step_batch"):
        assert callable(getattr(navsim_amd.FamiliarityEngine, name)), name
    # the single-agent calls are as they were
    assert len(N.PROTOTYPES["dv_mb_sense_step"][1]) == 7 and len(N.PROTOTYPES["dv_mb_score_u8"][1]) == 4


def test_mushroom_ensemble_is_exported_and_is_a_nav_ensemble():
    assert "MushroomEnsemble" in navsim_amd.__all__
    assert issubclass(navsim_amd.MushroomEnsemble, navsim_amd.NavEnsemble)
    assert not issubclass(navsim_amd.MushroomEnsemble, navsim_amd.InfomaxEnsemble)
    for name in ("from_agent", "step_forward", "run", "scene_familiarity", "active"):
        assert hasattr(navsim_amd.MushroomEnsemble, name), name
    assert "chem_weights" not in inspect.signature(navsim_amd.MushroomEnsemble.from_agent).parameters


def test_mushroom_ensemble_refuses_other_models_untrained_agents_and_the_host_sensor():
    from oracle import oracle
    sads = _agent(oracle.sads_familiarity(0.25))
    sads.train_from_path(PATH)
    with pytest.raises(ValueError, match="MushroomEnsemble takes agents of the mushroom-body model.*NavEnsemble steps the library-based"):
        navsim_amd.MushroomEnsemble.from_agent(sads, POSES)
    with pytest.raises(ValueError, match="MushroomEnsemble takes agents of the mushroom-body model"):
        navsim_amd.MushroomEnsemble([sads])
    eng = object()
    for infomax in (_like("infomax", eng, eng), _agent(infomax_familiarity(seed=3))):
        with pytest.raises(ValueError, match="MushroomEnsemble does not take an Infomax model.*InfomaxEnsemble"):
            navsim_amd.MushroomEnsemble._check_member(infomax)
    # a mushroom-body agent with the host sensor model (no engine of its own)
    host = _agent(mushroom_familiarity(n_kc=300, fan_in=4, seed=3))
    with pytest.raises(ValueError, match="MushroomEnsemble needs agents whose sensor model runs on the GPU"):
        navsim_amd.MushroomEnsemble.from_agent(host, POSES)
    # ... with an engine, but untrained, or trained on another engine than its own
    with pytest.raises(ValueError, match="MushroomEnsemble needs trained agents"):
        navsim_amd.MushroomEnsemble.from_agent(_like("mushroom", eng, eng, trained=False), POSES)
    with pytest.raises(ValueError, match="MushroomEnsemble needs trained agents"):
        navsim_amd.MushroomEnsemble([_like("mushroom", eng, object())])
    navsim_amd.MushroomEnsemble._check_member(_like("mushroom", eng, eng))               # the one it takes
    with pytest.raises(ValueError, match="no agents"):
        navsim_amd.MushroomEnsemble([])


def test_the_other_ensembles_still_refuse_the_model_and_point_at_the_one_that_takes_it():
    eng = object()
    for agent in (_like("mushroom", eng, eng), _agent(mushroom_familiarity(n_kc=300, fan_in=4, seed=3))):
        with pytest.raises(ValueError, match="NavEnsemble does not take a mushroom-body model.*MushroomEnsemble"):
            navsim_amd.NavEnsemble._check_member(agent)
        with pytest.raises(ValueError, match="InfomaxEnsemble does not take a mushroom-body model.*MushroomEnsemble"):
            navsim_amd.InfomaxEnsemble._check_member(agent)
    navsim_amd.InfomaxEnsemble._check_member(_like("infomax", eng, eng))                 # (as before)


class _NoDevice(object):
    """Stands where the library does: any call through it is a test failure."""
    def __getattr__(self, name):
        raise AssertionError("%s reached the library" % name)


def _engine_without_a_device(shape):
    e = navsim_amd.FamiliarityEngine.__new__(navsim_amd.FamiliarityEngine)
    e._lib, e._ctx_raw, e._begun, e.mb_shape = _NoDevice(), None, False, shape
    return e


def test_shape_checks_come_before_any_device_call():
    e = _engine_without_a_device((3, 5))
    for planes in (np.zeros((2, 3, 5), np.uint8), np.zeros((2, 4, 5, 3), np.uint8), np.zeros((0, 4, 3, 5), np.uint8),
                   np.zeros((2, 0, 3, 5), np.uint8), np.zeros((2, 4, 3, 5, 1), np.uint8)):
        with pytest.raises(ValueError, match="planes must be uint8"):
            e.mb_step_batch_u8(planes)
    with pytest.raises((ValueError, TypeError)):
        e.mb_step_batch_u8(np.zeros((2, 4, 3, 5), np.float32))
    for x, y, ang in ((np.ones(2), np.ones(3), np.zeros((2, 4))), (np.ones(2), np.ones(2), np.zeros((3, 4))),
                      (np.ones(2), np.ones(2), np.zeros(8)), (np.ones(2), np.ones(2), np.zeros((2, 0))),
                      (np.ones(0), np.ones(0), np.zeros((0, 4))), (np.ones(2), np.ones(2), np.zeros((2, 2, 2)))):
        with pytest.raises(ValueError, match=r"x\[N\], y\[N\] and angles\[N, A\] expected"):
            e.mb_sense_step_batch(x, y, ang)
    # shapes that agree do reach the library
    with pytest.raises(AssertionError, match="dv_batch_mb_step_u8 reached the library"):
        e.mb_step_batch_u8(np.zeros((2, 4, 3, 5), np.uint8))
    with pytest.raises(AssertionError, match="dv_batch_mb_sense_step reached the library"):
        e.mb_sense_step_batch(np.ones(2), np.ones(2), np.zeros((2, 4)))


@pytest.mark.parametrize("key,n,A", HE.CASES)
def test_patch_sets_satisfy_the_helpers_conditions(key, n, A):
    """ensemble_data asserts the three conditions; here they are stated once more on what it returns, with the figures printed."""
    e = HE.ensemble_data(key, n, A)
    assert e["planes"].shape == (n, A, e["h"], e["w"]) and e["fam"].shape == (n, A) and e["best"].shape == (n,)
    assert np.array_equal(H.bits(e["fam"]), H.bits((-e["d"]).astype(np.float64))) and e["fam"].max() == 0.0
    assert e["best"].tolist() == np.argmax(e["fam"], axis=1).tolist()
    print("mushroom ensemble %s %dx%d: best %r, d in [%d, %d], columns with d > 0: %d of %d"
          % (key, n, A, e["best"].tolist(), e["d"].min(), e["d"].max(), int((e["d"] > 0).sum()), n * A))
    assert (e["d"] > 0).any()
    if A > 1:
        assert (e["best"] != 0).any()
    if A >= 8:
        i = e["planted"]
        a0, a1 = HE.planted_headings(A)
        assert i == n - 1 and 0 < a0 < a1 < A
        assert np.flatnonzero(e["d"][i] == 0).tolist() == [a0, a1] and e["best"][i] == a0
        assert np.array_equal(e["planes"][i, a0], e["planes"][i, a1])
        if A > 256:
            assert a1 - 256 < a0                                                         # the later heading sits in the lower thread
    else:
        assert e["planted"] is None
    for i in range(n):
        if i != e["planted"] and (A > 1 or i % 2 == 0):
            assert e["d"][i, (3 * i + 1) % A] == 0, i                                    # the member's trained view


def test_slab_inputs_cross_the_view_bound_and_the_byte_bound():
    views, stage = H.slab_views()
    s = HE.slab_data()
    assert s["pick"].shape == (3, 2731) and s["pick"].size == views + 1
    assert not np.array_equal(s["two"][0], s["two"][1]) and s["fam"].min() < 0 and s["fam"].max() == 0.0
    assert s["pick"].reshape(-1)[views] == 0 and s["pick"].reshape(-1)[views - 1] == 1   # the column behind the bound differs from the one before
    assert s["best"][2] == 2730
    b = HE.bytes_data()
    n = b["pick"].shape[1]
    assert (n - 1) * b["h"] * b["w"] == stage and n - 1 < views                           # the bytes, not the views, end the first launch
    assert b["best"].tolist() == [n - 1] and b["fam"][0, -1] == 0.0 and b["fam"][0, 0] < 0


def test_sensed_models_and_poses_distinguish():
    conn, n_active, wt = HE.sensed_model("c16")
    assert conn.shape[1] == 16 and 1024 + 4 * (255 * 16 + 1) * 4 + 64 == 66384 > 65536
    for A in (9, 13):
        xs, ys, centre = HE.sensed_poses(A)
        offsets = np.linspace(-np.pi / 2, np.pi / 2, A)
        angs = (centre[:, None] + offsets[None, :]) % (2 * np.pi)
        for name in HE.SENSED_MODELS:
            fam = HE.sensed_statement(name, xs, ys, angs)
            print("mushroom sensed %s A=%d: best %r, values %d" % (name, A, np.argmax(fam, axis=1).tolist(), len(np.unique(fam))))
            assert fam.shape == (5, A) and len(np.unique(fam)) > 3 and (np.argmax(fam, axis=1) != 0).any()
