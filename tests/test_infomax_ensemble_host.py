"""Ensembles of Infomax agents, host side (no GPU): who InfomaxEnsemble and NavEnsemble refuse, the C ABI's two batch calls in the
binding, the engine methods' shape checks (made before any device call), the symbols the two one-value models' shared engine code
reaches, and the margins of the patch sets the GPU tests use (tests/helpers_infomax_ensemble.py) under the NumPy restatement."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import infomax_familiarity, synth
from tests import helpers_infomax as H
from tests import helpers_infomax_ensemble as HE

LAND = synth.synth_landscape(5, 200, 4)
PATH = np.stack([np.linspace(50, 150, 40), np.full(40, 100.0)], axis=1)
POSES = [((60.0, 100.5), 0.1), ((80.0, 99.0), 6.1)]


def _agent(model):
    return navsim_amd.NavBySceneFamiliarity(LAND, (8, 8), 2.0, n_test_angles=4, use_gpu_sensor=False, familiarity_model=model)


def _infomax_like(engine, func_engine, trained=True):
    """What InfomaxEnsemble looks at in an agent, without a device."""
    return SimpleNamespace(_engine=engine, familiarity_model=SimpleNamespace(metric="infomax"), training_path=PATH if trained else None,
                           _familiarity_func=SimpleNamespace(engine=func_engine, metric="infomax") if trained else None)


def test_infomax_ensemble_is_exported_and_is_a_nav_ensemble():
    assert "InfomaxEnsemble" in navsim_amd.__all__
    assert issubclass(navsim_amd.InfomaxEnsemble, navsim_amd.NavEnsemble)
    for name in ("from_agent", "step_forward", "run", "scene_familiarity", "active"):
        assert hasattr(navsim_amd.InfomaxEnsemble, name), name
    import inspect
    assert "chem_weights" not in inspect.signature(navsim_amd.InfomaxEnsemble.from_agent).parameters


def test_infomax_ensemble_refuses_other_models_untrained_agents_and_the_host_sensor():
    from oracle import oracle
    sads = _agent(oracle.sads_familiarity(0.25))
    sads.train_from_path(PATH)
    with pytest.raises(ValueError, match="takes agents of the Infomax model"):
        navsim_amd.InfomaxEnsemble.from_agent(sads, POSES)
    with pytest.raises(ValueError, match="takes agents of the Infomax model"):
        navsim_amd.InfomaxEnsemble([sads])
    # an Infomax agent with the host sensor model (no engine of its own), trained or not
    host = _agent(infomax_familiarity(seed=3))
    with pytest.raises(ValueError, match="sensor model runs on the GPU"):
        navsim_amd.InfomaxEnsemble.from_agent(host, POSES)
    # ... with an engine, but untrained
    eng = object()
    with pytest.raises(ValueError, match="needs trained agents"):
        navsim_amd.InfomaxEnsemble.from_agent(_infomax_like(eng, eng, trained=False), POSES)
    with pytest.raises(ValueError, match="needs trained agents"):
        navsim_amd.InfomaxEnsemble([_infomax_like(eng, eng, trained=False)])
    navsim_amd.InfomaxEnsemble._check_member(_infomax_like(eng, eng))                    # the one it takes
    with pytest.raises(ValueError, match="no agents"):
        navsim_amd.InfomaxEnsemble([])


def test_nav_ensemble_still_refuses_infomax():
    eng = object()
    for agent in (_infomax_like(eng, eng), _agent(infomax_familiarity(seed=3))):
        with pytest.raises(ValueError, match="NavEnsemble does not take an Infomax model"):
            navsim_amd.NavEnsemble.from_agent(agent, POSES)
        with pytest.raises(ValueError, match="NavEnsemble does not take an Infomax model"):
            navsim_amd.NavEnsemble([agent])
    with pytest.raises(ValueError, match="InfomaxEnsemble"):                             # the message points at the class that does
        navsim_amd.NavEnsemble([_infomax_like(eng, eng)])


def test_batch_calls_are_bound_and_exported():
    i32p, u32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32)
    assert N.PROTOTYPES["dv_batch_infomax_step_u8"] == (ctypes.c_int, [N._ctx_p, N._u8p, ctypes.c_int, ctypes.c_int, N._f64p, i32p])
    assert N.PROTOTYPES["dv_batch_infomax_sense_step"] == (ctypes.c_int, [N._ctx_p, N._f64p, N._f64p, N._f64p, ctypes.c_int, ctypes.c_int,
                                                                          N._f64p, i32p, u32p])
    lib = N.load()
    for name in ("dv_batch_infomax_step_u8", "dv_batch_infomax_sense_step"):
        assert hasattr(lib, name), name
    for name in ("infomax_step_batch_u8", "infomax_sense_step_batch"):
        assert callable(getattr(navsim_amd.FamiliarityEngine, name)), name
    # the single-agent calls are as they were
    assert len(N.PROTOTYPES["dv_infomax_sense_step"][1]) == 7 and len(N.PROTOTYPES["dv_infomax_score_u8"][1]) == 4


class _NoDevice(object):
    """Stands where the library does: any call through it is a test failure."""
    def __getattr__(self, name):
        raise AssertionError("%s reached the library" % name)


def _engine_without_a_device(lib, shape):
    e = navsim_amd.FamiliarityEngine.__new__(navsim_amd.FamiliarityEngine)
    e._lib, e._ctx_raw, e._begun, e.infomax_shape, e.mb_shape, e.sensor_shape = lib, None, False, shape, shape, shape
    return e


def test_shape_checks_come_before_any_device_call():
    """The Infomax twin of the mushroom-body test of this name (tests/test_mushroom_ensemble_host.py): the same bad inputs."""
    e = _engine_without_a_device(_NoDevice(), (3, 5))
    for planes in (np.zeros((2, 3, 5), np.uint8), np.zeros((2, 4, 5, 3), np.uint8), np.zeros((0, 4, 3, 5), np.uint8),
                   np.zeros((2, 0, 3, 5), np.uint8), np.zeros((2, 4, 3, 5, 1), np.uint8)):
        with pytest.raises(ValueError, match="planes must be uint8"):
            e.infomax_step_batch_u8(planes)
    with pytest.raises((ValueError, TypeError)):
        e.infomax_step_batch_u8(np.zeros((2, 4, 3, 5), np.float32))
    for x, y, ang in ((np.ones(2), np.ones(3), np.zeros((2, 4))), (np.ones(2), np.ones(2), np.zeros((3, 4))),
                      (np.ones(2), np.ones(2), np.zeros(8)), (np.ones(2), np.ones(2), np.zeros((2, 0))),
                      (np.ones(0), np.ones(0), np.zeros((0, 4))), (np.ones(2), np.ones(2), np.zeros((2, 2, 2)))):
        with pytest.raises(ValueError, match=r"x\[N\], y\[N\] and angles\[N, A\] expected"):
            e.infomax_sense_step_batch(x, y, ang)
    # shapes that agree do reach the library
    with pytest.raises(AssertionError, match="dv_batch_infomax_step_u8 reached the library"):
        e.infomax_step_batch_u8(np.zeros((2, 4, 3, 5), np.uint8))
    with pytest.raises(AssertionError, match="dv_batch_infomax_sense_step reached the library"):
        e.infomax_sense_step_batch(np.ones(2), np.ones(2), np.zeros((2, 4)))


class _Recorder(object):
    """Stands where the library does: every call succeeds and is noted as (symbol, number of arguments)."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, len(args)))
            return 0
        return call


@pytest.mark.parametrize("prefix,single,batch", [("infomax", "dv_infomax", "dv_batch_infomax"), ("mb", "dv_mb", "dv_batch_mb")])
def test_each_shared_operation_reaches_its_own_models_symbol(prefix, single, batch):
    """The two one-value models share one implementation per engine operation, driven by a table of symbol prefixes: every public
    method must still reach the symbol its name promises, with as many arguments as the binding declares for that symbol."""
    h, w, n, A = 3, 5, 2, 4
    lib = _Recorder()
    e = _engine_without_a_device(lib, (h, w))
    views, xy = np.zeros((n, h, w), np.uint8), np.ones(n)
    for method, args, symbol in (("train_u8", (views,), single + "_train_u8"),
                                 ("train_from_poses", (xy, xy, xy), single + "_train_from_poses"),
                                 ("score_u8", (views,), single + "_score_u8"),
                                 ("sense_step", (1.0, 1.0, np.zeros(A)), single + "_sense_step"),
                                 ("step_batch_u8", (np.zeros((n, A, h, w), np.uint8),), batch + "_step_u8"),
                                 ("sense_step_batch", (xy, xy, np.zeros((n, A))), batch + "_sense_step")):
        del lib.calls[:]
        getattr(e, prefix + "_" + method)(*args)
        assert lib.calls == [(symbol, len(N.PROTOTYPES[symbol][1]))], (method, lib.calls)
    # ... and the accessor hands out the same model's methods
    model = e.one_value({"infomax": "infomax", "mb": "mushroom"}[prefix])
    for op in ("train_u8", "train_from_poses", "score_u8", "sense_step", "end"):
        assert getattr(model, op) == getattr(e, prefix + "_" + op), op


@pytest.mark.parametrize("n,A", HE.LAYOUTS)
@pytest.mark.parametrize("key", HE.KEYS)
def test_every_members_best_heading_is_clear_of_the_tolerance(key, n, A):
    """What lets the GPU tests demand the restatement's argmax of every member: its best heading leads the second best by more than
    1000 TOL relative; in the planted member the two copies are equal and lead every other patch by as much."""
    e = HE.ensemble_data(key, n, A)
    assert e["planes"].shape == (n, A, e["h"], e["w"]) and e["fam"].shape == (n, A) and np.all(e["fam"] < 0)
    for i in range(n):
        row = e["fam"][i]
        if i == e["planted"]:
            assert H.bits(row[2]) == H.bits(row[7]) and int(np.argmax(row)) == 2
            others = np.delete(row, [2, 7])
            assert (row[2] - others.max()) / abs(row[2]) > 1000 * H.TOL, (i, row[2], others.max())
        else:
            assert H.best_margin(row) > 1000 * H.TOL, (i, H.best_margin(row))
    if n == 7:
        assert e["planted"] is None
    else:
        assert e["planted"] == n - 1
