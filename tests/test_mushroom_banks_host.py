"""Memory banks of the mushroom-body model without a device: the conditions of tests/helpers_mushroom_banks.py with their figures, the
binding surface of the dv_mbank_* calls, the Python-side checks of the bank tables (made before any library call), the refusals of
MushroomRouteEnsemble and of the other ensembles, and run_ensemble's per-member default frames."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import experiment, infomax_familiarity, mushroom_familiarity, synth
from tests import helpers_mushroom as H
from tests import helpers_mushroom_banks as HB

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"dv_mbank_set": "mbank_set", "dv_mbank_train_u8": "mbank_train_u8", "dv_mbank_train_from_poses": "mbank_train_from_poses",
         "dv_mbank_step_u8": "mbank_step_batch_u8", "dv_mbank_sense_step": "mbank_sense_step_batch",
         "dv_mbank_read_weights": "mbank_read_weights", "dv_mbank_set_weights": "mbank_set_weights", "dv_mbank_info": "mbank_info"}


# ---- the helpers' conditions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(set(HB.KEYS + HB.QUARTER_KEYS)))
def test_banks_differ_and_patches_tell_them_apart(key):
    b = HB.bank_data(key)
    print("banks %s: equal share %.2f, least pairwise weight difference %d, views %r, zeros %r"
          % (key, b["equal_share"], b["min_diff"], b["counts"].tolist(), b["zeros"].tolist()))
    assert b["wts"].shape == (HB.R, b["K"]) and b["counts"].sum() == b["F"]
    for r in range(HB.R):
        assert np.array_equal(b["wts"][r], H.train(np.ones(b["K"], np.uint8), b["views"][b["bank_of"] == r], b["conn"], b["n_active"]))
        for o in range(r + 1, HB.R):
            assert (b["wts"][r] != b["wts"][o]).any(), (r, o)
    if key in HB.QUARTER_KEYS:
        assert b["equal_share"] <= 0.25 and b["min_diff"] >= 100
    # the whole model's weights are the banks' weights multiplied: nothing trained is lost by dealing the views out
    assert np.array_equal(b["wts"].min(axis=0), b["wt"])


@pytest.mark.parametrize("n,A", HB.LAYOUTS + (HB.TIE_LAYOUT,))
@pytest.mark.parametrize("key", HB.KEYS)
def test_member_bank_tables_distinguish(key, n, A):
    d = HB.layout_data(key, n, A)
    assert d["banks"].shape == (n,) and d["banks"].min() >= 0 and d["banks"].max() < HB.R
    told = []
    for i in range(n):
        own, best = d["banks"][i], d["best"][i]
        assert np.array_equal(d["fam"][i], (-d["nov_all"][own, i]).astype(np.float64)) and best == int(np.argmax(d["fam"][i]))
        told.append(any(d["nov_all"][o, i, best] != d["nov_all"][own, i, best] for o in range(HB.R) if o != own))
    assert all(told) if A >= 8 else any(told), (key, n, A, told)
    if n > 1:
        assert len(set(d["banks"].tolist())) > 1
    if d["planted"] is not None:
        assert d["banks"][d["planted"]] == 0
    if (n, A) == HB.TIE_LAYOUT:
        assert d["best"][1] == 5 and H.bits(d["fam"][1, [5, 257]]).tolist() == [0, 0] and d["banks"][0] != d["banks"][1]


def test_bound_inputs_catch_a_table_read_at_the_launchs_own_column():
    views, stage = H.slab_views()
    v = HB.view_bound_data()
    assert len(v["pick"]) == views + 1 and v["bank_of"][views] != v["bank_of"][0] and v["pick"][views] == 1 and not v["pick"][:views].any()
    # read at column 0 of the second launch, view 8192 would go to bank 0: another bank 0 and another bank 2
    wrong = HB.train_banks(v["two"][v["pick"][[0, 1, 2, views]]], [0, 1, 2, 0], v["conn"], v["n_active"], v["K"])
    assert not np.array_equal(wrong[0], v["wts"][0]) and not np.array_equal(wrong[2], v["wts"][2])
    assert v["step_banks"][-1] != v["step_banks"][0] and v["step_pick"].size == views + 1
    nov0 = H.novelty(v["wts"][0], v["two"][1:], v["conn"], v["n_active"])[0]
    assert nov0 > 0 and v["fam"][2, -1] == 0.0                                           # column 8192 under bank 0 is not what is expected
    b = HB.byte_bound_data()
    assert (len(b["pick"]) - 1) * b["h"] * b["w"] == stage and len(b["pick"]) - 1 < views
    assert b["bank_of"][-1] == 1 and b["pick"][-1] == 1 and b["step_banks"][-1] != b["step_banks"][0]
    assert not np.array_equal(b["wts"][1], b["wts"][0]) and b["fam"].min() < 0


# ---- binding surface -------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_engine_agree_on_the_mbank_names():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    declared = set(re.findall(r"\bint\s+(dv_mbank_[a-z0-9_]*)\s*\(", header))
    assert declared == set(NAMES) == {k for k in N.PROTOTYPES if k.startswith("dv_mbank_")}
    assert not any(k.startswith("dv_mb_") for k in declared)
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert N.PROTOTYPES[name][0] is ctypes.c_int
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(N.PROTOTYPES[name][1]), name
        assert callable(getattr(navsim_amd.FamiliarityEngine, NAMES[name])), name
    # a banked call is its unbanked twin with the bank table behind the counts
    assert N.PROTOTYPES["dv_mbank_train_u8"][1] == N.PROTOTYPES["dv_mb_train_u8"][1] + [N._i32p]
    assert N.PROTOTYPES["dv_mbank_sense_step"][1] == N.PROTOTYPES["dv_batch_mb_sense_step"][1][:6] + [N._i32p] + N.PROTOTYPES["dv_batch_mb_sense_step"][1][6:]
    assert N.PROTOTYPES["dv_mbank_step_u8"][1] == N.PROTOTYPES["dv_batch_mb_step_u8"][1][:4] + [N._i32p] + N.PROTOTYPES["dv_batch_mb_step_u8"][1][4:]
    # ... and the twins are as they were
    assert len(N.PROTOTYPES["dv_mb_train_u8"][1]) == 3 and len(N.PROTOTYPES["dv_batch_mb_sense_step"][1]) == 9 and len(N.PROTOTYPES["dv_mb_info"][1]) == 8
    assert "MushroomRouteEnsemble" in navsim_amd.__all__ and issubclass(navsim_amd.MushroomRouteEnsemble, navsim_amd.NavEnsemble)
    assert not issubclass(navsim_amd.MushroomRouteEnsemble, navsim_amd.MushroomEnsemble)
    assert list(inspect.signature(navsim_amd.MushroomRouteEnsemble.from_routes).parameters) == ["agent", "routes", "starts"]


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


def _engine_without_a_device(lib, shape, banks):
    e = navsim_amd.FamiliarityEngine.__new__(navsim_amd.FamiliarityEngine)
    e._lib, e._ctx_raw, e._begun, e.mb_shape, e.sensor_shape, e.mb_banks = lib, None, False, shape, shape, banks
    return e


def test_bank_table_checks_come_before_any_library_call():
    h, w, n, A = 3, 5, 4, 2
    lib = _Recorder()
    e = _engine_without_a_device(lib, (h, w), 3)
    views, xy = np.zeros((n, h, w), np.uint8), np.ones(n)
    planes, angs = np.zeros((n, A, h, w), np.uint8), np.zeros((n, A))
    calls = {"mbank_train_u8": (lambda t: e.mbank_train_u8(views, t), "bank_of_view"),
             "mbank_train_from_poses": (lambda t: e.mbank_train_from_poses(xy, xy, xy, t), "bank_of_view"),
             "mbank_step_batch_u8": (lambda t: e.mbank_step_batch_u8(planes, t), "bank_of_member"),
             "mbank_sense_step_batch": (lambda t: e.mbank_sense_step_batch(xy, xy, angs, t), "bank_of_member")}
    bad = ([0, 1, 3, 0], [0, -1, 1, 2], [0, 1, 2], [0, 1, 2, 0, 1], [[0, 1], [2, 0]], [0.0, 1.0, 2.0, 0.0], np.array([0, 1, 2, 1.5]), None)
    for name, (call, what) in calls.items():
        for table in bad:
            with pytest.raises(ValueError, match=what):
                call(table)
        assert lib.calls == [], (name, lib.calls)
    with pytest.raises(ValueError, match=r"bank_of_view\[2\] = 3 outside \[0, n_banks = 3\)"):
        e.mbank_train_u8(views, [0, 1, 3, 0])
    for bank in (3, -1, 1.0, None, True):
        with pytest.raises(ValueError, match="bank must be an integer"):
            e.mbank_set_weights(bank, np.ones(7, np.uint8))
    for bank in (3, -1, 1.5):
        with pytest.raises(ValueError, match="bank must be an integer"):
            e.mbank_read_weights(bank)
    for nb in (0, -2, 1.5, None, True):
        with pytest.raises(ValueError, match="n_banks must be an integer >= 1"):
            e.mbank_set(nb)
    assert lib.calls == [] and e.mb_banks == 3
    # tables that hold: each method reaches its own symbol, once, with the arguments the binding declares
    good = np.array([2, 0, 1, 1], dtype=np.int64)
    for name, symbol in (("mbank_train_u8", "dv_mbank_train_u8"), ("mbank_train_from_poses", "dv_mbank_train_from_poses"),
                         ("mbank_step_batch_u8", "dv_mbank_step_u8"), ("mbank_sense_step_batch", "dv_mbank_sense_step")):
        del lib.calls[:]
        res = calls[name][0](good)
        assert lib.calls == [(symbol, len(N.PROTOTYPES[symbol][1]))], (name, lib.calls)
        if "step" in name:
            assert isinstance(res, navsim_amd.engine.OneValueBatchResults) and res.angle_familiarity.shape == (n, A)
    del lib.calls[:]
    e.mbank_set(5)
    assert lib.calls == [("dv_mbank_set", 2)] and e.mb_banks == 5
    # mb_begin and mb_end return to one bank
    e.mb_begin(h, w, np.zeros((4, 2), np.int32), 1)
    assert e.mb_banks == 1
    e.mb_banks = 4
    e.mb_end()
    assert e.mb_banks == 1


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
LAND = synth.synth_landscape(3, 300, 4)


def _agent(model, gpu=False):
    return navsim_amd.NavBySceneFamiliarity(LAND, (12, 10), 1.0, n_test_angles=9, use_gpu_sensor=gpu, familiarity_model=model)


class _Like(object):
    """An agent-shaped object: what the refusals look at."""
    training_path = None
    memory_bank = None

    def __init__(self, metric, engine=None):
        self.familiarity_model = type("M", (), {"metric": metric})()
        self._engine = engine


def test_from_routes_refuses_what_it_cannot_train():
    paths = HB.routes()
    st = HB.starts(paths)
    RE = navsim_amd.MushroomRouteEnsemble
    from oracle import oracle
    with pytest.raises(ValueError, match="MushroomRouteEnsemble takes agents of the mushroom-body model"):
        RE.from_routes(_agent(oracle.sads_familiarity(0.25)), paths, st)
    with pytest.raises(ValueError, match="does not take an Infomax model"):
        RE.from_routes(_agent(infomax_familiarity(seed=3)), paths, st)
    with pytest.raises(ValueError, match="MushroomRouteEnsemble needs agents whose sensor model runs on the GPU"):
        RE.from_routes(_agent(mushroom_familiarity(n_kc=300, fan_in=4, seed=3)), paths, st)      # the host sensor model
    eng = object()
    trained = _Like("mushroom", eng)
    trained.training_path = paths[0]
    with pytest.raises(ValueError, match="from_routes takes an UNTRAINED agent"):
        RE.from_routes(trained, paths, st)
    fresh = _Like("mushroom", eng)                       # (the checks below come before anything is asked of the engine: `eng` has no methods)
    for bad in ([(3, (70.0, 70.0), 0.1)], [(0, (70.0, 70.0), 0.1), (-1, (70.0, 70.0), 0.1)], [(1.0, (70.0, 70.0), 0.1)]):
        with pytest.raises(ValueError, match="route_index .* outside \\[0, 3\\)"):
            RE.from_routes(fresh, paths, bad)
    with pytest.raises(ValueError, match="no starts"):
        RE.from_routes(fresh, paths, [])
    with pytest.raises(ValueError, match="routes must be"):
        RE.from_routes(fresh, [], st)
    with pytest.raises(ValueError, match="made from routes"):
        RE.from_agent(fresh, [((70.0, 70.0), 0.1)])
    with pytest.raises(ValueError, match="takes the members MushroomRouteEnsemble.from_routes makes"):
        RE([fresh])


def test_a_banked_member_steps_with_its_ensemble_only():
    a = _agent(mushroom_familiarity(n_kc=300, fan_in=4, seed=3))
    a.memory_bank = 2
    with pytest.raises(ValueError, match="memory bank 2 .*MushroomRouteEnsemble"):
        a.step_forward()
    with pytest.raises(ValueError, match="MushroomRouteEnsemble"):
        navsim_amd.run_experiment(a, frames=3)
    eng = object()
    member = _Like("mushroom", eng)
    member.memory_bank, member.training_path = 1, HB.routes()[0]
    member._familiarity_func = type("F", (), {"engine": eng, "metric": "mushroom"})()
    for cls in (navsim_amd.MushroomEnsemble, navsim_amd.NavEnsemble, navsim_amd.InfomaxEnsemble):
        with pytest.raises(ValueError, match="%s does not take a member of a MushroomRouteEnsemble" % cls.__name__):
            cls._check_member(member)
        with pytest.raises(ValueError, match="does not take a member of a MushroomRouteEnsemble"):
            cls([member])
    navsim_amd.MushroomRouteEnsemble._check_member(member)                               # the one that takes it
    member.memory_bank = None
    navsim_amd.MushroomEnsemble._check_member(member)                                    # (as before)


# ---- frames ------------------------------------------------------------------------------------------------------------------------------------
class _Walker(object):
    """A member for NavEnsemble.run: counts its steps."""
    stopped_with_exception = None
    _n_navigation_error = 0
    percent_recapitulated = 0.0

    def __init__(self, length, step):
        self.training_path_length, self.step_size, self.steps = length, step, 0

    def percent_recapitulated_forgiving(self, n_consecutive_scenes):
        return 0.0

    def n_captures(self, n_consecutive_scenes):
        return 0


class _Ens(navsim_amd.NavEnsemble):
    def __init__(self, agents, stop_at=None):
        self.agents, self.stop_status, self.stop_at, self.seen = agents, [0] * len(agents), stop_at or {}, []

    def _step_forward(self, fake):
        act = self.active
        self.seen.append(list(act))
        for i in act:
            self.agents[i].steps += 1
            if self.stop_at.get(i) == self.agents[i].steps:
                self.stop_status[i] = -1
        return self.active


def test_run_takes_one_count_per_member():
    ens = _Ens([_Walker(10, 1.0) for _ in range(4)], stop_at={3: 2})
    done = ens.run([3, 0, 5, 9])
    assert done == [3, 0, 5, 1] and [a.steps for a in ens.agents] == [3, 0, 5, 2]
    assert ens.stop_status == [0, 0, 0, -1]                                              # out of frames is no stop
    assert ens.seen == [[0, 2, 3], [0, 2, 3], [0, 2], [2], [2]] and ens._frames_left is None
    assert ens.active == [0, 1, 2]
    with pytest.raises(ValueError, match="frames holds 2 counts for 4 members"):
        ens.run([1, 2])
    # an int is every member's count, as before
    ens = _Ens([_Walker(10, 1.0) for _ in range(3)], stop_at={1: 2})
    assert ens.run(4) == [4, 1, 4] and ens.seen == [[0, 1, 2], [0, 1, 2], [0, 2], [0, 2]]


def test_run_ensembles_default_frames_are_each_members_own():
    same = _Ens([_Walker(44.7, 1.5) for _ in range(3)])
    rows = experiment.run_ensemble(same)
    today = int(experiment.FRAME_FACTOR * 44.7 / 1.5)                                    # members on one path: the value used before
    assert [r["completed_frames"] for r in rows] == [today] * 3 and len(same.seen) == today
    mixed = _Ens([_Walker(44.0, 1.0), _Walker(39.2, 1.0), _Walker(34.0, 2.0)])
    rows = experiment.run_ensemble(mixed)
    assert [r["completed_frames"] for r in rows] == [132, 117, 51] and [r["stop_status"] for r in rows] == [0, 0, 0]
    assert [r["completed_frames"] for r in experiment.run_ensemble(_Ens([_Walker(44.0, 1.0), _Walker(10.0, 1.0)]), frames=7)] == [7, 7]
