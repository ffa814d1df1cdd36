"""Population tables of the mushroom-body model without a device: the binding surface of the dv_mbpop_* calls, the engine's argument
checks (made before any library call), util.mushroom_population against the NumPy statement's own draws, and the populations=
plumbing of MushroomRouteEnsemble against a fake engine's call log (tests/helpers_mbpop.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import mushroom_familiarity
from navsim_amd.util import mushroom_population
from tests import helpers_mbpop as HP
from tests import helpers_mushroom as H
from tests import helpers_mushroom_banks as HB

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"dv_mbpop_set": "mbpop_set", "dv_mbpop_clear": "mbpop_clear", "dv_mbpop_info": "mbpop_info"}


# ---- binding surface -------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_engine_agree_on_the_mbpop_names():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    declared = set(re.findall(r"\bint\s+(dv_mbpop_[a-z0-9_]*)\s*\(", header))
    assert declared == set(NAMES) == {k for k in N.PROTOTYPES if k.startswith("dv_mbpop_")}
    assert not any(k.startswith(("dv_mb_", "dv_mbank_")) for k in declared)               # (the closed sets of the two older surfaces)
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert N.PROTOTYPES[name][0] is ctypes.c_int
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(N.PROTOTYPES[name][1]), name
        assert callable(getattr(navsim_amd.FamiliarityEngine, NAMES[name])), name
    # the banked calls serve the table with no new argument
    assert len(N.PROTOTYPES["dv_mbank_train_u8"][1]) == 4 and len(N.PROTOTYPES["dv_mbank_sense_step"][1]) == 10
    assert len(N.PROTOTYPES["dv_lands_mbank_sense_step"][1]) == 11 and len(N.PROTOTYPES["dv_mbank_read_weights"][1]) == 3
    for call in ("from_routes_with", "from_landscapes"):
        assert list(inspect.signature(getattr(navsim_amd.MushroomRouteEnsemble, call)).parameters)[-1] == "populations"
    assert list(inspect.signature(navsim_amd.MushroomRouteEnsemble.from_routes).parameters) == ["agent", "routes", "starts"]


def test_the_kernels_live_in_their_own_file_and_k_mb_is_read_not_copied():
    csrc = os.path.join(REPO, "navigation-by-deja-vu_amd", "csrc")
    new = open(os.path.join(csrc, "dejavu_mbpop.inl")).read()
    kernels = set(re.findall(r"\bvoid\s+(k_[a-z0-9_]+)\s*\(", new))
    assert kernels == {"k_mbpop_bank", "k_mbpop_pose_bank", "k_mbpop_pose_bank_lands", "k_mbpop_pose_bank_lands_sensors", "k_mbpop_count"}
    assert len(re.findall(r"^\s+mb_view<", new, re.M)) == 4 and "atomicAdd" not in new      # one statement of the selection: mb_view's
    old = open(os.path.join(csrc, "dejavu_mushroom.inl")).read()
    assert not re.findall(r"\bvoid\s+(k_mbpop[a-z0-9_]*)\s*\(", old)
    assert '#include "dejavu_mbpop.inl"' in open(os.path.join(csrc, "dejavu_hip.hip")).read()


# ---- mushroom_population -----------------------------------------------------------------------------------------------------------------------
def test_mushroom_population_draws_what_the_model_and_the_statement_draw():
    pop = mushroom_population(35, n_kc=257, fan_in=10, sparsity=0.013, seed=41, channel=1)
    assert sorted(pop) == ["channel", "conn", "fan_in", "n_active", "n_kc"]
    assert (pop["channel"], pop["n_kc"], pop["fan_in"], pop["n_active"]) == (1, 257, 10, 3)
    assert pop["conn"].dtype == np.int32 and np.array_equal(pop["conn"], H.connectivity(257, 35, 10, 41))
    model = mushroom_familiarity(channel=1, n_kc=257, fan_in=10, sparsity=0.013, seed=41)
    assert model.n_active == pop["n_active"] and (model.sparsity, model.seed) == (0.013, 41)
    assert mushroom_population(35, n_kc=10, sparsity=0.001)["n_active"] == 1              # max(1, round(0.01))
    d = mushroom_population(1024)
    assert (d["n_kc"], d["fan_in"], d["n_active"], d["channel"]) == (20000, 10, 200, 2) and d["conn"].shape == (20000, 10)
    # the statement's plug-in of the same arguments trains the same weights as the population's own numbers
    scenes = np.random.default_rng(3).integers(0, 5, (6, 5, 7, 3)).astype(np.uint8) * 60
    func = H.numpy_model(channel=1, n_kc=257, fan_in=10, sparsity=0.013, seed=41)(scenes)
    assert np.array_equal(func.wt, H.train(np.ones(257, np.uint8), scenes[..., 1], pop["conn"], pop["n_active"]))
    for bad in (dict(n_kc=0), dict(fan_in=17), dict(sparsity=0.0), dict(channel=3)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            mushroom_population(35, **bad)
    for bad in (0, -3, 2.5, None, True):
        with pytest.raises(ValueError, match="n_pixels"):
            mushroom_population(bad)


# ---- argument checks before the library -----------------------------------------------------------------------------------------------------
class _Recorder(object):
    """Stands where the library does: every call succeeds and is noted as (symbol, number of arguments)."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, len(args)))
            return 0
        return call


def _engine_without_a_device(lib, shape):
    e = navsim_amd.FamiliarityEngine.__new__(navsim_amd.FamiliarityEngine)
    e._lib, e._ctx_raw, e._begun, e.mb_shape, e.sensor_shape, e.mb_banks = lib, None, False, shape, shape, 1
    return e


def test_every_refusal_comes_before_any_library_call():
    h, w = 5, 7
    lib = _Recorder()
    e = _engine_without_a_device(lib, (h, w))
    good = HP.population(h * w, 63, 4, 7, 1)

    def but(**kw):
        keep = {k: v for k, v in good.items() if "conn" not in kw or k not in ("n_kc", "fan_in")}       # (another conn: its own shape)
        return dict(keep, **kw)

    conn = good["conn"]
    low, high = conn.copy(), conn.copy()
    low[5, 2], high[62, 3] = -1, h * w
    bad_pops = (
        (but(n_active=0), r"populations\[1\]: n_active 0 outside \[1, n_kc = 63\]"),
        (but(n_active=64), r"populations\[1\]: n_active 64 outside"),
        (but(n_active=7.0), r"populations\[1\]: n_active"),
        (but(channel=3), r"populations\[1\]: channel 3 outside \[0, 2\]"),
        (but(channel=-1), r"populations\[1\]: channel"),
        (but(conn=conn[:, :0]), r"populations\[1\]: fan_in 0 outside \[1, 16\]"),
        (but(conn=np.zeros((4, 17), np.int32)), r"populations\[1\]: fan_in 17 outside"),
        (but(conn=np.zeros((0, 4), np.int32)), r"populations\[1\]: n_kc 0 outside \[1, 16777216\]"),
        (but(conn=conn.astype(np.float64)), r"populations\[1\]: conn must hold integers"),
        (but(conn=conn.reshape(-1)), r"populations\[1\]: conn must be int32\[n_kc, fan_in\]"),
        (but(conn=low), r"populations\[1\]: conn\[5\]\[2\] = -1 outside \[0, 35\)"),
        (but(conn=high), r"populations\[1\]: conn\[62\]\[3\] = 35 outside \[0, 35\)"),
        (but(n_kc=64), r"populations\[1\]: n_kc = 64, but conn has shape \(63, 4\)"),
        (but(fan_in=5), r"populations\[1\]: fan_in = 5, but conn"),
        (but(weights=1), r"populations\[1\]: unknown keys \['weights'\]"),
        ({k: v for k, v in good.items() if k != "conn"}, r"populations\[1\] must be a dict with conn and n_active"),
        ([1, 2], r"populations\[1\] must be a dict"),
    )
    for pop, message in bad_pops:
        with pytest.raises(ValueError, match=message):
            e.mbpop_set([good, pop], [0, 1])
    for pops in ([], None, good, 3):
        with pytest.raises(ValueError, match="populations must be a list of one or more dicts"):
            e.mbpop_set(pops, [0])
    for table, message in (([0, 2], r"population_of_bank\[1\] = 2 outside \[0, n_pops = 2\)"), ([-1, 0], r"population_of_bank\[0\] = -1"),
                           ([0.0, 1.0], "population_of_bank must hold integers"), ([[0, 1]], "population_of_bank must have one dimension"),
                           ([], "population_of_bank must name the population of one or more banks")):
        with pytest.raises(ValueError, match=message):
            e.mbpop_set([good, good], table)
    assert lib.calls == [] and e.mb_pops is None and e.mb_banks == 1
    # a table that holds: one call, with the arguments the binding declares; the engine knows the ragged lengths from then on
    wide = HP.population(h * w, 257, 10, 3, 2, channel=0)
    e.mbpop_set([good, wide], np.array([1, 0, 1], dtype=np.int64))
    assert lib.calls == [("dv_mbpop_set", len(N.PROTOTYPES["dv_mbpop_set"][1]))] and e.mb_banks == 3
    assert [p["n_kc"] for p in e.mb_pops] == [63, 257] and e.mb_pop_of_bank.tolist() == [1, 0, 1] and "conn" not in e.mb_pops[0]
    del lib.calls[:]
    for bank, own, given in ((0, 257, 63), (1, 63, 257), (2, 257, 63)):                   # the bank's own length, before the library
        with pytest.raises(ValueError, match=r"weights must be uint8\[%d\]" % own):
            e.mbank_set_weights(bank, np.ones(given, np.uint8))
    for bank in (3, -1, 1.0, None, True):
        with pytest.raises(ValueError, match="bank must be an integer"):
            e.mbank_set_weights(bank, np.ones(63, np.uint8))
    for table in ([0, 1, 3, 0], [0, -1, 1, 2]):
        with pytest.raises(ValueError, match="bank_of_view"):
            e.mbank_train_u8(np.zeros((4, h, w), np.uint8), table)
    assert lib.calls == []
    got = e.mbank_read_weights()
    assert isinstance(got, list) and [len(g) for g in got] == [257, 63, 257] and all(g.dtype == np.uint8 for g in got)
    assert e.mbank_read_weights(1).shape == (63,)
    assert lib.calls == [("dv_mbank_read_weights", 3)] * 4
    e.mbank_set_weights(1, np.ones(63, np.uint8))
    assert lib.calls[-1] == ("dv_mbank_set_weights", 3)
    # mbpop_clear, mbank_set, mb_begin and mb_end each forget the table
    for drop in (lambda: e.mbpop_clear(), lambda: e.mbank_set(2), lambda: e.mb_begin(h, w, np.zeros((4, 2), np.int32), 1), lambda: e.mb_end()):
        e.mbpop_set([good], [0, 0])
        assert e.mb_pops is not None
        drop()
        assert e.mb_pops is None and e.mb_banks == (2 if lib.calls[-1][0] == "dv_mbank_set" else 1)
    e.mb_shape = None                                                                     # no model: the library answers DV_ERR_STATE
    del lib.calls[:]
    e.mbpop_set([but(conn=high)], [0])
    assert lib.calls == [("dv_mbpop_set", 9)]


# ---- the ensemble's plumbing -------------------------------------------------------------------------------------------------------------------
class _Agent(object):
    """An agent-shaped object on a fake engine: what _from_routes touches."""
    training_path = None
    memory_bank = None
    landscape_index = None
    n_test_angles = 9
    step_size = 1.0
    track_scene_familiarity = False
    stopped_with_exception = None

    def __init__(self, engine, model):
        self._engine, self.familiarity_model = engine, model
        self.sensor_dimensions = np.array([engine.w, engine.h])
        self.landscape = np.zeros((300, 300, 3), np.uint8)
        self._sensor_r = 6.0
        self.angle_offsets = np.zeros(9)

    def _check_bounds(self, pt):
        pass

    def reset_error(self):
        pass


MODEL = dict(channel=2, n_kc=300, fan_in=4, sparsity=0.02, seed=6)


def _from_routes(populations, metrics="host"):
    eng = HP.FakeEngine(10, 12)
    paths = HB.routes()
    agent = _Agent(eng, mushroom_familiarity(**MODEL))
    ens = navsim_amd.MushroomRouteEnsemble.from_routes_with(agent, paths, HB.starts(paths), metrics=metrics, populations=populations)
    return eng, ens, paths


def test_populations_none_logs_todays_calls():
    eng, ens, paths = _from_routes(None)
    assert eng.log == [("mb_begin", 10, 12, (300, 4), 6, 2), ("mbank_set", 3), ("mbank_train_from_poses", sum(len(p) for p in paths), [0, 1, 2])]
    assert all(a.population_index is None and a.population is None for a in ens.agents)
    info = ens.bank_info()
    assert eng.log[-1] == ("mbank_info",) and len(eng.log) == 4
    assert info["n_kc"].tolist() == [300] * 3 and info["n_active"].tolist() == [6] * 3 and info["population_of_bank"].tolist() == [0] * 3
    plain = navsim_amd.MushroomRouteEnsemble.from_routes(_Agent(HP.FakeEngine(10, 12), mushroom_familiarity(**MODEL)), paths, HB.starts(paths))
    assert plain.engine.log == eng.log[:3]


def test_equal_entries_share_one_population_and_members_carry_theirs():
    pops = [None, dict(n_kc=1043, seed=7), dict(seed=6)]                                  # the third equals the model's own: one population
    eng, ens, paths = _from_routes(pops)
    assert [c[0] for c in eng.log] == ["mb_begin", "mbpop_set", "mbank_train_from_poses"]
    _, sent, of_bank = eng.log[1]
    own = dict(channel=2, n_kc=300, fan_in=4, n_active=6, sparsity=0.02, seed=6)
    other = dict(channel=2, n_kc=1043, fan_in=4, n_active=21, sparsity=0.02, seed=7)
    assert sent == [own, other] and of_bank == [0, 1, 0]
    assert np.array_equal(eng.mb_pops[1]["conn"], H.connectivity(1043, 120, 4, 7)) and eng.mb_pops[1]["conn"].dtype == np.int32
    assert [a.memory_bank for a in ens.agents] == [0, 0, 1, 1, 2, 2] and [a.population_index for a in ens.agents] == [0, 0, 1, 1, 0, 0]
    assert ens.agents[2].population == other and ens.agents[5].population == own
    info = ens.bank_info()
    assert sorted(info) == ["n_active", "n_banks", "n_depressed", "n_kc", "population_of_bank", "views_trained"]
    assert info["n_kc"].tolist() == [300, 1043, 300] and info["n_active"].tolist() == [6, 21, 6] and info["population_of_bank"].tolist() == [0, 1, 0]
    # a route under two populations is entered twice
    paths = HB.routes()
    twice = [paths[0], paths[0], paths[1]]
    eng2 = HP.FakeEngine(10, 12)
    starts = [(0, (70.0, 70.0), 0.1), (1, (70.0, 70.0), 0.1), (2, (70.0, 70.0), 0.1)]
    ens2 = navsim_amd.MushroomRouteEnsemble.from_routes_with(_Agent(eng2, mushroom_familiarity(**MODEL)), twice, starts,
                                                             populations=[None, dict(sparsity=0.05, channel=0), None])
    assert eng2.log[1][2] == [0, 1, 0] and eng2.log[1][1][1]["n_active"] == 15 and eng2.log[1][1][1]["channel"] == 0
    assert ens2.agents[0].training_path is ens2.agents[1].training_path and ens2.agents[1].population_index == 1


def test_populations_are_refused_by_entry_before_the_engine_is_asked():
    for bad, message in (([None, None], "one entry per route \\(3\\)"), (dict(n_kc=3), "one entry per route"), ([None, 3, None], r"populations\[1\] must be None or a dict"),
                         ([None, None, dict(cells=5)], r"populations\[2\]: unknown keys \['cells'\]"),
                         ([dict(n_kc=0), None, None], r"populations\[0\]: n_kc must be a positive integer"),
                         ([None, dict(fan_in=17), None], r"populations\[1\]: fan_in"), ([None, dict(sparsity=2), None], r"populations\[1\]: sparsity"),
                         ([None, None, dict(channel=5)], r"populations\[2\]: channel")):
        eng = HP.FakeEngine(10, 12)
        with pytest.raises(ValueError, match=message):
            paths = HB.routes()
            navsim_amd.MushroomRouteEnsemble.from_routes_with(_Agent(eng, mushroom_familiarity(**MODEL)), paths, HB.starts(paths), populations=bad)
        assert eng.log == []
    # the other route ensembles have no populations to give
    with pytest.raises(ValueError, match="InfomaxRouteEnsemble has no populations"):
        navsim_amd.InfomaxRouteEnsemble._population_entries(None, None, 3, [None] * 3)
    assert "populations" not in inspect.signature(navsim_amd.SadsRouteEnsemble.from_routes_with).parameters
