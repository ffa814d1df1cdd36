"""Weight banks of the Infomax model without a device: the conditions of tests/helpers_infomax_banks.py with their figures (the tolerance
rule measured again on every bank's chain), the binding surface of the dv_ibank_* calls, the Python-side checks of the bank tables (made
before any library call) and the refusals of InfomaxRouteEnsemble and of the other ensembles."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import infomax_familiarity, mushroom_familiarity, synth
from tests import helpers_infomax as H
from tests import helpers_infomax_banks as HB

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"dv_ibank_set": "ibank_set", "dv_ibank_train_u8": "ibank_train_u8", "dv_ibank_train_from_poses": "ibank_train_from_poses",
         "dv_ibank_step_u8": "ibank_step_batch_u8", "dv_ibank_sense_step": "ibank_sense_step_batch",
         "dv_ibank_read_weights": "ibank_read_weights", "dv_ibank_set_weights": "ibank_set_weights", "dv_ibank_info": "ibank_info"}


# ---- the helpers' conditions ---------------------------------------------------------------------------------------------------------------
def test_the_pattern_deals_the_cases_as_the_tests_need_them():
    assert HB.PATTERN == (2, 0, 1, 1, 0, 2, 1) and HB.R == 3
    assert HB.bank_data("5x3_f2")["counts"].tolist() == [1, 0, 1]                         # one bank stays empty
    assert HB.bank_data("7x5_m1043")["counts"].tolist() == [1, 1, 1]                      # one view a bank
    assert HB.bank_data("33x31")["N"] % 4 != 0
    for key in HB.KEYS:
        b = HB.bank_data(key)
        assert b["counts"].sum() == b["F"] and len(b["Ws"]) == HB.R
        for r in range(HB.R):
            assert np.array_equal(b["Ws"][r], H.train(b["W0"], b["views"][b["bank_of"] == r]))
        if b["counts"][1] == 0:
            assert np.array_equal(H.bits(b["Ws"][1]), H.bits(b["W0"]))
    for key in ("40x1", "16x16_a16", "32x32_m1040"):                                     # chains of unequal length
        assert len(set(HB.bank_data(key)["counts"].tolist())) > 1, key
    # a 64-column block boundary inside a bank's run of columns: in (2, 65) a member's own 65 columns; in (5, 13) column 64 of the
    # caller's order lies inside member 4, whose bank also holds member 1 -- its run is cut from columns that are no neighbours
    assert (np.bincount(HB.deal(2), minlength=HB.R) * 65).tolist() == [65, 0, 65]
    assert (np.bincount(HB.deal(5), minlength=HB.R) * 13).tolist() == [26, 26, 13] and HB.deal(5)[4] == HB.deal(5)[1] == 0
    assert HB.deal(7).tolist() == list(HB.PATTERN)
    assert HB.LAYOUTS == ((1, 16), (7, 1), (5, 13), (3, 60), (2, 65))


@pytest.mark.parametrize("key", HB.KEYS)
def test_tolerance_rule_on_every_banks_chain(key):
    """1000 x the float64 statement's own discrepancy (against longdouble, against a permuted order) on every bank's chain stays under
    the bound the GPU tests use, H.TOL."""
    w, d = HB.bank_discrepancies(key)
    print("infomax banks %s: largest discrepancy of a bank's chain: weights %.2e, scores %.2e (1000 x under TOL %.1e)" % (key, w, d, H.TOL))
    assert 1000 * max(w, d) <= H.TOL


def test_tolerance_rule_on_the_sensed_routes():
    w = HB.sensed_discrepancy()
    print("infomax banks, sensed routes: largest discrepancy of a route's chain: weights %.2e (1000 x under TOL %.1e)" % (w, H.TOL))
    assert 1000 * w <= H.TOL
    x, y, ang, bank_of, first = HB.interleaved_poses()
    assert [len(f) for f in first] == list(HB.SENSED_POINTS) and len(set(HB.SENSED_POINTS)) == 3
    assert bank_of[:6].tolist() == [0, 1, 2, 0, 1, 2]                                    # interleaved
    for r, route in enumerate(HB.sensed_routes()):
        assert np.array_equal(x[first[r]], route[:, 0]) and np.array_equal(ang[first[r]], HB.route_headings(route))


@pytest.mark.parametrize("n,A", HB.LAYOUTS)
@pytest.mark.parametrize("key", HB.KEYS)
def test_the_banks_tell_the_members_apart_and_best_headings_are_clear(key, n, A):
    d = HB.layout_data(key, n, A)
    assert d["banks"].tolist() == [HB.PATTERN[i % 7] for i in range(n)]
    margins = []
    for i in range(n):
        assert np.array_equal(H.bits(d["fam"][i]), H.bits(d["fam_all"][d["banks"][i], i]))
        for r in range(HB.R):
            if r != d["banks"][i]:
                assert HB.wrong_bank_shows(d["fam_all"], d["banks"], i, r), (key, n, A, i, r)
        margins.append(H.best_margin(d["fam"][i]))
        assert margins[-1] > 1000 * H.TOL, (key, n, A, i, margins[-1])
    print("infomax banks %s %dx%d: least margin of a best heading %.2e" % (key, n, A, min(margins)))
    if n > 1:
        assert len(set(d["banks"].tolist())) > 1


# ---- steps past one launch -------------------------------------------------------------------------------------------------------------------
def test_the_slab_layout_under_banks_of_one_shape_cuts_a_member_and_a_wrong_index_would_show():
    from tests import helpers_inet as HN
    lay, d = HN.slab_layout(), HB.slab_step_data()
    A, c0, s = lay["A"], lay["c0"], lay["straddler"]
    assert (c0, lay["nc1"], lay["nc2"], lay["cut"]) == (8176, 8176, 80, 4) and [b[:3] for b in lay["launches"][1][2]] == [(1, 8176, 44), (2, 8220, 24), (3, 8244, 12)]
    assert d["Ws"][0].shape == (24, 1024) and np.bincount(d["bank_of"]).tolist() == list(HN.SLAB["trained"])
    assert np.array_equal(d["banks"], lay["banks"]) and (np.diff(d["banks"]) < 0).any()
    assert d["first"][s] < lay["cut"] <= d["second"][s] and d["margin"] > 1000 * H.TOL
    cols = d["planes"][lay["order"]].reshape((-1,) + d["planes"].shape[2:])
    bank, x = HN.wrong_index_margins(lay, cols, lambda b, planes: H.familiarity(d["Ws"][b], planes))
    told = ~np.isnan(x)
    print("%s, M = 24 a bank: maxima ahead by %.2e; launch 2 under the launch-local place's bank off by %.2e at least, X read at c %% slab by %.2e"
          % (HN.SLAB_NAME, d["margin"], bank.min(), x[told].min()))
    assert bank.min() > 1e-6 and x[told].min() > 1e-6 and told.sum() == 64
    w = max(H.chain_discrepancy(d["W0"], d["views"][d["bank_of"] == b], d["Ws"][b], HB.SLAB["eta"]) for b in range(4))
    sc = HN.score_discrepancy(lambda **kw: HB.slab_scores(d["Ws"], d["planes"], d["banks"], **kw), d["fam"])
    print("    largest discrepancy of the statement: weights %.2e, scores %.2e (1000 x under TOL %.1e)" % (w, sc, H.TOL))
    assert 1000 * max(w, sc) <= H.TOL


def test_the_blocks_layout_under_banks_of_one_shape_is_16384_blocks_and_one():
    from tests import helpers_inet as HN
    d = HB.blocks_data()
    B = HN.BLOCKS["banks"]
    assert [(c0, nc, len(b)) for c0, nc, b in d["launches"]] == [(0, 49152, 16384), (49152, 3, 1)] and d["W0"].shape == (15, 35)
    assert sorted(d["trained"]) == [0, B - 2, B - 1] and d["last"] != B - 1 and d["banks"][d["last"]] == B - 1
    i = d["last"]
    right = d["fam"][i]
    assert right.tolist() == H.familiarity(d["trained"][B - 1], d["planes"][i]).tolist()
    for W in (d["trained"][0], d["trained"][B - 2], d["W0"]):                             # the bank of sorted place 0, one block back, no bank's
        assert (np.abs(H.familiarity(W, d["planes"][i]) - right) / np.abs(right)).min() > 1e-6
    assert (np.abs(H.familiarity(d["trained"][B - 1], d["planes"][d["order"][0]]) - right) / np.abs(right)).min() > 1e-6
    w = max(H.chain_discrepancy(d["W0"], d["views"][d["bank_of"] == b], W, HB.BLOCKS["eta"]) for b, W in d["trained"].items())
    sc = HN.score_discrepancy(lambda **kw: HB.blocks_scores(d["W0"], d["trained"], **kw), d["fam"])
    print("%s, M = 15 a bank: largest discrepancy of the statement: weights %.2e, scores %.2e (1000 x under TOL %.1e)" % (HN.BLOCKS_NAME, w, sc, H.TOL))
    assert 1000 * max(w, sc) <= H.TOL


# ---- binding surface -------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_engine_agree_on_the_ibank_names():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    declared = set(re.findall(r"\bint\s+(dv_ibank_[a-z0-9_]*)\s*\(", header))
    assert declared == set(NAMES) == {k for k in N.PROTOTYPES if k.startswith("dv_ibank_")}
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert N.PROTOTYPES[name][0] is ctypes.c_int
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(N.PROTOTYPES[name][1]), name
        assert callable(getattr(navsim_amd.FamiliarityEngine, NAMES[name])), name
    # a banked call is its unbanked twin with the bank table behind the counts
    assert N.PROTOTYPES["dv_ibank_train_u8"][1] == N.PROTOTYPES["dv_infomax_train_u8"][1] + [N._i32p]
    assert N.PROTOTYPES["dv_ibank_train_from_poses"][1] == N.PROTOTYPES["dv_infomax_train_from_poses"][1][:5] + [N._i32p] + \
        N.PROTOTYPES["dv_infomax_train_from_poses"][1][5:]
    assert N.PROTOTYPES["dv_ibank_sense_step"][1] == N.PROTOTYPES["dv_batch_infomax_sense_step"][1][:6] + [N._i32p] + \
        N.PROTOTYPES["dv_batch_infomax_sense_step"][1][6:]
    assert N.PROTOTYPES["dv_ibank_step_u8"][1] == N.PROTOTYPES["dv_batch_infomax_step_u8"][1][:4] + [N._i32p] + \
        N.PROTOTYPES["dv_batch_infomax_step_u8"][1][4:]
    # ... and the twins are as they were
    assert len(N.PROTOTYPES["dv_infomax_train_u8"][1]) == 3 and len(N.PROTOTYPES["dv_batch_infomax_sense_step"][1]) == 9
    assert len(N.PROTOTYPES["dv_infomax_info"][1]) == 6
    assert "InfomaxRouteEnsemble" in navsim_amd.__all__ and issubclass(navsim_amd.InfomaxRouteEnsemble, navsim_amd.NavEnsemble)
    assert not issubclass(navsim_amd.InfomaxRouteEnsemble, navsim_amd.InfomaxEnsemble)
    assert list(inspect.signature(navsim_amd.InfomaxRouteEnsemble.from_routes).parameters) == ["agent", "routes", "starts"]
    # the two route ensembles share from_routes
    assert navsim_amd.InfomaxRouteEnsemble.from_routes.__func__ is navsim_amd.MushroomRouteEnsemble.from_routes.__func__


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
    e._lib, e._ctx_raw, e._begun, e.infomax_shape, e.sensor_shape, e.infomax_banks = lib, None, False, shape, shape, banks
    return e


def test_bank_table_checks_come_before_any_library_call():
    h, w, n, A = 3, 5, 4, 2
    lib = _Recorder()
    e = _engine_without_a_device(lib, (h, w), 3)
    e.mb_banks = 7                                                                       # (the other model's banks do not count here)
    views, xy = np.zeros((n, h, w), np.uint8), np.ones(n)
    planes, angs = np.zeros((n, A, h, w), np.uint8), np.zeros((n, A))
    calls = {"ibank_train_u8": (lambda t: e.ibank_train_u8(views, t), "bank_of_view"),
             "ibank_train_from_poses": (lambda t: e.ibank_train_from_poses(xy, xy, xy, t), "bank_of_view"),
             "ibank_step_batch_u8": (lambda t: e.ibank_step_batch_u8(planes, t), "bank_of_member"),
             "ibank_sense_step_batch": (lambda t: e.ibank_sense_step_batch(xy, xy, angs, t), "bank_of_member")}
    bad = ([0, 1, 3, 0], [0, -1, 1, 2], [0, 1, 2], [0, 1, 2, 0, 1], [[0, 1], [2, 0]], [0.0, 1.0, 2.0, 0.0], np.array([0, 1, 2, 1.5]), None)
    for name, (call, what) in calls.items():
        for table in bad:
            with pytest.raises(ValueError, match=what):
                call(table)
        assert lib.calls == [], (name, lib.calls)
    with pytest.raises(ValueError, match=r"bank_of_view\[2\] = 3 outside \[0, n_banks = 3\)"):
        e.ibank_train_u8(views, [0, 1, 3, 0])
    for bank in (3, -1, 1.0, None, True):
        with pytest.raises(ValueError, match="bank must be an integer"):
            e.ibank_set_weights(bank, np.ones((4, 15)))
    for bank in (3, -1, 1.5, None):
        with pytest.raises(ValueError, match="bank must be an integer"):
            e.ibank_read_weights(bank)
    for nb in (0, -2, 1.5, None, True):
        with pytest.raises(ValueError, match="n_banks must be an integer >= 1"):
            e.ibank_set(nb, np.ones((4, 15)))
    assert lib.calls == [] and e.infomax_banks == 3
    # tables that hold: each method reaches its own symbol, once, with the arguments the binding declares
    good = np.array([2, 0, 1, 1], dtype=np.int64)
    for name, symbol in (("ibank_train_u8", "dv_ibank_train_u8"), ("ibank_train_from_poses", "dv_ibank_train_from_poses"),
                         ("ibank_step_batch_u8", "dv_ibank_step_u8"), ("ibank_sense_step_batch", "dv_ibank_sense_step")):
        del lib.calls[:]
        res = calls[name][0](good)
        assert lib.calls == [(symbol, len(N.PROTOTYPES[symbol][1]))], (name, lib.calls)
        if "step" in name:
            assert isinstance(res, navsim_amd.engine.OneValueBatchResults) and res.angle_familiarity.shape == (n, A)
    e.ibank_train_u8(np.zeros((0, h, w), np.uint8), [])                                  # no views: legal
    del lib.calls[:]
    e.ibank_set(5, np.ones((4, 15)))
    assert ("dv_ibank_set", 3) in lib.calls and e.infomax_banks == 5
    # infomax_begin and infomax_end return to one bank
    e.infomax_begin(h, w, np.zeros((4, 15)))
    assert e.infomax_banks == 1
    e.infomax_banks = 4
    e.infomax_end()
    assert e.infomax_banks == 1


def test_a_banked_call_is_bounded_by_its_own_models_banks():
    """The two models' banked calls share one host path; what tells them apart is whose bank count bounds the table.  With 2 Infomax
    banks and 5 mushroom banks a table that names bank 4 reaches every dv_mbank_* symbol and no dv_ibank_* one, and with the counts
    exchanged the reverse."""
    h, w, A = 3, 5, 2
    table = [0, 4]
    views, xy = np.zeros((2, h, w), np.uint8), np.ones(2)
    planes, angs = np.zeros((2, A, h, w), np.uint8), np.zeros((2, A))
    ops = (("train_u8", "train_u8", (views,)), ("train_from_poses", "train_from_poses", (xy, xy, xy)),
           ("step_batch_u8", "step_u8", (planes,)), ("sense_step_batch", "sense_step", (xy, xy, angs)))
    for ibanks, mbanks in ((2, 5), (5, 2)):
        lib = _Recorder()
        e = _engine_without_a_device(lib, (h, w), ibanks)
        e.mb_shape, e.mb_banks = (h, w), mbanks
        for prefix, banks in (("ibank_", ibanks), ("mbank_", mbanks)):
            for method, op, args in ops:
                del lib.calls[:]
                if banks == 5:
                    getattr(e, prefix + method)(*args + (table,))
                    assert lib.calls == [("dv_" + prefix + op, len(N.PROTOTYPES["dv_" + prefix + op][1]))], (prefix, method, lib.calls)
                else:
                    with pytest.raises(ValueError, match=r"\[1\] = 4 outside \[0, n_banks = 2\)"):
                        getattr(e, prefix + method)(*args + (table,))
                    assert lib.calls == [], (prefix, method, lib.calls)


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
    RE = navsim_amd.InfomaxRouteEnsemble
    from oracle import oracle
    with pytest.raises(ValueError, match="InfomaxRouteEnsemble takes agents of the Infomax model"):
        RE.from_routes(_agent(oracle.sads_familiarity(0.25)), paths, st)
    with pytest.raises(ValueError, match="does not take a mushroom-body model"):
        RE.from_routes(_agent(mushroom_familiarity(n_kc=300, fan_in=4, seed=3)), paths, st)
    with pytest.raises(ValueError, match="InfomaxRouteEnsemble needs agents whose sensor model runs on the GPU"):
        RE.from_routes(_agent(infomax_familiarity(seed=3)), paths, st)                   # the host sensor model
    eng = object()
    trained = _Like("infomax", eng)
    trained.training_path = paths[0]
    with pytest.raises(ValueError, match="from_routes takes an UNTRAINED agent"):
        RE.from_routes(trained, paths, st)
    fresh = _Like("infomax", eng)                        # (the checks below come before anything is asked of the engine: `eng` has no methods)
    for bad in ([(3, (70.0, 70.0), 0.1)], [(0, (70.0, 70.0), 0.1), (-1, (70.0, 70.0), 0.1)], [(1.0, (70.0, 70.0), 0.1)]):
        with pytest.raises(ValueError, match="route_index .* outside \\[0, 3\\)"):
            RE.from_routes(fresh, paths, bad)
    with pytest.raises(ValueError, match="no starts"):
        RE.from_routes(fresh, paths, [])
    with pytest.raises(ValueError, match="routes must be"):
        RE.from_routes(fresh, [], st)
    with pytest.raises(ValueError, match="InfomaxRouteEnsemble is made from routes .*InfomaxEnsemble.from_agent"):
        RE.from_agent(fresh, [((70.0, 70.0), 0.1)])
    with pytest.raises(ValueError, match="takes the members InfomaxRouteEnsemble.from_routes makes"):
        RE([fresh])


def test_a_banked_member_steps_with_its_ensemble_only():
    a = _agent(infomax_familiarity(seed=3))
    a.memory_bank = 2
    with pytest.raises(ValueError, match="memory bank 2 .*InfomaxRouteEnsemble"):
        a.step_forward()
    with pytest.raises(ValueError, match="InfomaxRouteEnsemble"):
        navsim_amd.run_experiment(a, frames=3)
    eng = object()
    member = _Like("infomax", eng)
    member.memory_bank, member.training_path = 1, HB.routes()[0]
    member._familiarity_func = type("F", (), {"engine": eng, "metric": "infomax"})()
    for cls in (navsim_amd.InfomaxEnsemble, navsim_amd.NavEnsemble, navsim_amd.MushroomEnsemble):
        with pytest.raises(ValueError, match="%s does not take a member of a InfomaxRouteEnsemble" % cls.__name__):
            cls._check_member(member)
        with pytest.raises(ValueError, match="does not take a member of a InfomaxRouteEnsemble"):
            cls([member])
    navsim_amd.InfomaxRouteEnsemble._check_member(member)                                # the one that takes it
    with pytest.raises(ValueError, match="MushroomRouteEnsemble takes agents of the mushroom-body model|does not take an Infomax model"):
        navsim_amd.MushroomRouteEnsemble._check_member(member)                           # ... and its twin does not
    member.memory_bank = None
    navsim_amd.InfomaxEnsemble._check_member(member)                                     # (as before)
