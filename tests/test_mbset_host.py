"""CPU side of the bank-set tests: what tests/helpers_mbset.py's inputs must distinguish (so that no GPU test passes on a read-out that
takes a set's entries in another order, drops its last bank, or takes its table at the launch's own column), the binding surface, the
Python-side refusals, made before any library call, the overflow arithmetic, and the opponent ensemble's bank numbering and noise keys."""
import os
import re

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from tests import helpers_mbset as M
from tests import helpers_mushroom as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"dv_mbset_step_u8": "mbset_step_batch_u8", "dv_mbset_sense_step": "mbset_sense_step_batch",
         "dv_mbset_lands_sense_step": "mbset_sense_step_batch"}


# ---- the helpers' conditions, with their figures -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(M.SHAPES))
@pytest.mark.parametrize("S", M.SET_SIZES)
def test_uploaded_inputs_tell_order_and_last_bank(shape, S):
    m = M.model(shape)
    for name, c in (("layout", M.case(shape, S)), ("constant", M.constant_case(shape, S))):
        order, drop = M.conditions(c["mask"], m["wts"], c["banks"], c["coefs"], c["A"])
        print("%s %s S=%d: %d columns of %d change with the entries' order, %d without the last bank"
              % (shape, name, S, order, c["fam"].size, drop))
        assert order > 0 and drop > 0, (shape, name, S)
        assert c["nov"].shape == c["fam"].shape + (S,) and c["nov"].min() >= 0 and c["nov"].max() <= m["n_active"]
    c = M.case(shape, S)
    if S >= 2:
        assert (c["coefs"] < 0).any() and (c["coefs"] == 0).any() and (c["banks"][1::2, -1] == c["banks"][1::2, 0]).all()
    assert len(np.unique(c["fam"])) > 3


def test_the_small_model_has_empty_waves():
    K = M.SHAPES["7x5"]["K"]
    span = H.wave_span(K)
    assert span == 64 and K - 2 * span == 2 and 3 * span > K                              # wave 2 owns two cells, wave 3 none


def test_the_tie_is_decided_by_the_sum_and_not_by_the_first_bank():
    t = M.tie_case()
    assert t["best"].tolist() == [100, 5] and t["planes"].shape[:2] == M.TIE_LAYOUT
    assert t["nov"][1, 5].tolist() == [10, 4] and t["nov"][1, 257].tolist() == [8, 2]
    assert int(np.argmax(-t["nov"][1, :, 0])) == 257
    order, drop = M.conditions(H.fired_mask(t["planes"].reshape(-1, t["h"], t["w"]), t["conn"], t["n_active"])[0], t["wts"], t["banks"],
                               t["coefs"], M.TIE_LAYOUT[1])
    assert order > 0 and drop > 0


@pytest.mark.parametrize("which", ["uploaded", "sensed"])
def test_the_second_launch_begins_inside_a_member(which):
    c0, member, heading = M.second_launch()
    n, A = M.WIDE_LAYOUT
    assert n * A > c0 and member == n - 1 and 0 < heading < A                             # column 8192: member 682, heading 8
    w = M.wide_case() if which == "uploaded" else M.wide_sensed_case()
    assert not np.array_equal(w["banks"][member], w["banks"][0]) and not np.array_equal(w["coefs"][member], w["coefs"][0])
    print("683 x 12 %s: the launch's own column gives another value at columns %r" % (which, w["wrong"].tolist()))
    assert len(w["wrong"]) > 0 and w["wrong"].min() >= c0
    m = M.model("7x5")
    order, drop = M.conditions(w["mask"], m["wts"], w["banks"], w["coefs"], A)
    assert order > 0 and drop > 0


@pytest.mark.parametrize("kind", ["own", "lands", "table", "noise", "both"])
def test_sensed_inputs_tell_order_and_last_bank(kind):
    s = M.sensed_case(kind)
    mask, _ = H.fired_mask(s["planes"].reshape((-1,) + s["planes"].shape[2:]), s["conn"], M.SENSED["n_active"])
    order, drop = M.conditions(mask, s["wts"], s["banks"], s["coefs"], M.SENSED["headings"])
    print("sensed %s: %d of %d columns change with the order, %d without the last bank" % (kind, order, s["fam"].size, drop))
    assert order > 0 and drop > 0
    if kind in ("table", "both"):
        assert sorted(set(s["lands"].tolist())) == [0, 1] and [c["pixel"] for c in s["table"]] == [(2, 4), (1, 1)]
    if kind == "lands":                                                                 # a member's own landscape among several shows
        own = M.sensed_case("own")
        assert s["lands"].tolist() == [0, 1, 1, 0, 1] and s["table"] is None and s["keys"] is None
        moved = [i for i in range(len(s["lands"])) if not np.array_equal(s["planes"][i], own["planes"][i])]
        assert moved == [1, 2, 4] and not np.array_equal(s["fam"], own["fam"])


def test_one_heading_of_the_flag_member_leaves_its_landscape():
    x, y, off = M.off_facts()
    assert off == [False, False, True, False]


# ---- the binding surface -------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_engine_agree_on_the_mbset_names():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    declared = set(re.findall(r"\bint\s+(dv_mbset_[a-z0-9_]*)\s*\(", header))
    assert declared == set(NAMES) == {k for k in N.PROTOTYPES if k.startswith("dv_mbset_")}
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name), name
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(N.PROTOTYPES[name][1]), name
        assert callable(getattr(navsim_amd.FamiliarityEngine, NAMES[name])), name
    assert int(re.search(r"#define\s+DV_MBSET_MAX_BANKS\s+(\d+)", header).group(1)) == N.DV_MBSET_MAX_BANKS == M.MAX_BANKS
    # the landscape form is the other sensed form with the landscape table behind the coefficients
    p = N.PROTOTYPES["dv_mbset_sense_step"][1]
    assert N.PROTOTYPES["dv_mbset_lands_sense_step"][1] == p[:9] + [N._i32p] + p[9:]
    # ... and the landscape set's own calls are the eight they were (the set step on a landscape set is named with the set calls)
    assert len({k for k in N.PROTOTYPES if k.startswith("dv_lands_")}) == 8


# ---- Python-side refusals, before any library call ----------------------------------------------------------------------------------------
class _Recorder(object):
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, len(args)))
            return 0
        return call


def _engine_without_a_device(lib, shape, banks, n_active):
    e = navsim_amd.FamiliarityEngine.__new__(navsim_amd.FamiliarityEngine)
    e._lib, e._ctx_raw, e._begun, e.mb_shape, e.sensor_shape, e.mb_banks, e.mb_active = lib, None, False, shape, shape, banks, n_active
    e.n_lands = 2
    return e


def test_set_table_checks_come_before_any_library_call():
    h, w, n, A = 3, 5, 4, 2
    lib = _Recorder()
    e = _engine_without_a_device(lib, (h, w), 3, 7)
    planes, xy, angs = np.zeros((n, A, h, w), np.uint8), np.ones(n), np.zeros((n, A))
    good_b, good_c = np.array([[0, 1], [2, 2], [1, 0], [0, 2]]), np.array([[1, -1], [1, 0], [2, -3], [1, -1024]])
    bad = [(good_b.astype(float), good_c, "bank_sets must hold integers"),
           (good_b, good_c.astype(float), "coefs must hold integers"),
           (good_b[:3], good_c[:3], r"bank_sets must have shape \(4, S\)"),
           (good_b[:, 0], good_c[:, 0], r"bank_sets must have shape \(4, S\)"),
           (np.zeros((4, 0), int), np.zeros((4, 0), int), "1 <= S <= DV_MBSET_MAX_BANKS = 8"),
           (np.zeros((4, 9), int), np.zeros((4, 9), int), "1 <= S <= DV_MBSET_MAX_BANKS = 8"),
           (good_b, good_c[:, :1], "one shape"),
           (np.where(np.arange(8).reshape(4, 2) == 5, 3, good_b), good_c, r"bank_sets\[2\]\[1\] = 3 outside \[0, n_banks = 3\)"),
           (np.where(np.arange(8).reshape(4, 2) == 0, -1, good_b), good_c, r"bank_sets\[0\]\[0\] = -1 outside"),
           (good_b, np.where(np.arange(8).reshape(4, 2) == 3, 2 ** 31, good_c), r"coefs\[1\]\[1\] = 2147483648 does not fit an int32"),
           (good_b, np.where(np.arange(8).reshape(4, 2) == 6, 2 ** 29, good_c), "member 3: sum")]
    for banks, coefs, msg in bad:
        for call in (lambda: e.mbset_step_batch_u8(planes, banks, coefs), lambda: e.mbset_sense_step_batch(xy, xy, angs, banks, coefs),
                     lambda: e.mbset_sense_step_batch(xy, xy, angs, banks, coefs, land_of_member=[0, 1, 1, 0])):
            with pytest.raises(ValueError, match=msg):
                call()
    with pytest.raises(ValueError, match="land_of_member"):
        e.mbset_sense_step_batch(xy, xy, angs, good_b, good_c, land_of_member=[0, 1, 2, 0])
    with pytest.raises(ValueError, match="planes must be uint8"):
        e.mbset_step_batch_u8(planes[0], good_b, good_c)
    assert lib.calls == []
    # tables that hold: each method reaches its own symbol, once, with the arguments the binding declares
    for call, symbol in ((lambda: e.mbset_step_batch_u8(planes, good_b, good_c), "dv_mbset_step_u8"),
                         (lambda: e.mbset_sense_step_batch(xy, xy, angs, good_b, good_c), "dv_mbset_sense_step"),
                         (lambda: e.mbset_sense_step_batch(xy, xy, angs, good_b, good_c, land_of_member=[0, 1, 1, 0]), "dv_mbset_lands_sense_step")):
        del lib.calls[:]
        res = call()
        assert lib.calls == [(symbol, len(N.PROTOTYPES[symbol][1]))], lib.calls
        assert isinstance(res, navsim_amd.engine.MbSetBatchResults) and res.angle_familiarity.shape == (n, A)
        assert res.bank_novelty.shape == (n, A, 2) and res.bank_novelty.dtype == np.int32 and res.flags.shape == (n,)


def test_the_overflow_bound_is_exact():
    for n_active in (1, 7, 200, 1 << 24):
        top = M.overflow_bound(n_active)
        assert top * n_active <= 2 ** 31 - 1 < (top + 1) * n_active
        T = navsim_amd.FamiliarityEngine.mbset_tables
        rest = min(top, 5)
        T([[0, 0]], [[top - rest, -rest]], 1, 1, n_active)                                # at the bound
        with pytest.raises(ValueError, match="member 0: sum .coefs. = %d times n_active = %d exceeds" % (top + 1, n_active)):
            T([[0, 0]], [[top - rest, -rest - 1]], 1, 1, n_active)
    b, c = navsim_amd.FamiliarityEngine.mbset_tables([[0]], [[-2 ** 31]], 1, 1, None)      # (n_active unknown: the library's check)
    assert b.dtype == c.dtype == np.int32 and c[0, 0] == -2 ** 31


# ---- the opponent ensemble: bank numbering, training order and noise keys --------------------------------------------------------------------
class _TrainingEngine(object):
    """Stands where the engine does while an ensemble is built: records the calls and answers the training call with blank views."""
    n_lands = 0

    def __init__(self):
        self.calls = []

    def mb_begin(self, *a, **k):
        self.calls.append(("mb_begin",))

    def mbank_set(self, n):
        self.calls.append(("mbank_set", int(n)))

    def lands_set(self, lands):
        self.calls.append(("lands_set", len(lands)))

    def noise_rows(self, seed, keys, amp_s, amp_v):
        self.calls.append(("noise_rows", int(seed), np.array(keys, dtype=np.uint64), list(amp_s), list(amp_v)))

    def noise_clear(self):
        self.calls.append(("noise_clear",))

    def __getattr__(self, name):                                                         # (what the model and the ensemble look for and never call here)
        if name in ("mb_train_u8", "mb_score_u8", "mb_sense_step", "mb_train_from_poses", "mb_end", "sense_step_batch_scene"):
            return lambda *a, **k: None
        raise AttributeError(name)

    def mbank_train_from_poses(self, x, y, angle, bank_of_view, land_of_view=None):
        self.calls.append(("train", np.array(x), np.array(y), np.array(angle), np.array(bank_of_view), None if land_of_view is None else np.array(land_of_view)))
        return np.zeros((len(x), 6, 8, 3), np.uint8)


def _untrained_agent(engine):
    from navsim_amd import mushroom_familiarity
    from tests import helpers_noise as HZ
    a = navsim_amd.NavBySceneFamiliarity(np.array(HZ.lands()[0]), HZ.ENS["sensor"], HZ.ENS_STEP, n_test_angles=HZ.ENS_ANGLES, use_gpu_sensor=False,
                                         n_sensor_levels=HZ.ENS["levels"], familiarity_model=mushroom_familiarity(**HZ.ENS_MB))
    a._engine = engine
    return a


def test_the_opponent_ensembles_banks_training_order_and_keys():
    from tests import helpers_noise as HZ
    RE = navsim_amd.MushroomRouteEnsemble
    routes, starts = HZ.ens_routes(), HZ.ens_starts()
    n = [len(r) for _, r in routes]
    runs = {}
    for name, kw in (("plain", {}), ("opp", dict(opponent=dict(turn=[np.pi, 2.0], gain=[1, 2, 0, 3])))):
        eng = _TrainingEngine()
        ens = RE.from_landscapes(_untrained_agent(eng), list(HZ.lands()), routes, starts, noise=HZ.ENS_NOISE, **kw)
        runs[name] = (eng, ens)
    (pe, plain), (oe, opp) = runs["plain"], runs["opp"]
    assert [c[0] for c in pe.calls] == [c[0] for c in oe.calls] == ["mb_begin", "lands_set", "noise_rows", "mbank_set", "train", "noise_clear"]
    assert pe.calls[3] == ("mbank_set", 2) and oe.calls[3] == ("mbank_set", 4)
    total = sum(n)
    pt, ot = pe.calls[4], oe.calls[4]
    for k in (1, 2, 3, 4, 5):                                                             # the attractive views first, in today's order
        assert np.array_equal(ot[k][:total], pt[k]), k
    assert np.array_equal(ot[1][total:], pt[1]) and np.array_equal(ot[2][total:], pt[2]) and np.array_equal(ot[5][total:], pt[5])
    assert np.array_equal(ot[4][total:], pt[4] + 2)                                       # route r's repulsive bank is R + r
    turn = np.repeat([np.pi, 2.0], n)
    assert np.array_equal(ot[3][total:], pt[3] + turn)
    # the keys: the attractive ones unchanged, the repulsive ones (0xC0000000 | r) << 32 | v with the route's training amplitudes
    pk, ok = pe.calls[2], oe.calls[2]
    assert np.array_equal(ok[2][:total], pk[2]) and ok[3][:total] == pk[3] and ok[4][:total] == pk[4] and ok[1] == pk[1]
    want = np.array([M.repulsive_key(r, v) for r in range(2) for v in range(n[r])], dtype=np.uint64)
    assert np.array_equal(ok[2][total:], want) and ok[3][total:] == pk[3] and ok[4][total:] == pk[4]
    assert np.array_equal(RE._repulsive_keys(1, 3), want[n[0]:n[0] + 3])
    att = {int(k) for k in pk[2]} | {int(k) for r in range(2 ** 4) for k in RE._train_keys(r, 4)}
    rep = {int(k) for k in want} | {int(k) for r in range(2 ** 4) for k in RE._repulsive_keys(r, 4)}
    assert not att & rep and all(k >> 62 == 3 for k in rep) and all(k >> 62 == 2 for k in att)
    assert all(RE._step_key(s, c) >> 63 == 0 for s in (0, 5, 2 ** 31 - 1) for c in (0, 1, 2 ** 32 - 1))      # a step key's top bit is 0
    # the members
    assert [a.memory_bank for a in opp.agents] == [0, 0, 1, 1] and [a.repulsive_bank for a in opp.agents] == [2, 2, 3, 3]
    assert [a.opponent_gain for a in opp.agents] == [1, 2, 0, 3] and all(a.bank_novelty is None for a in opp.agents)
    assert [len(a.repulsive_scenes) for a in opp.agents] == [n[0], n[0], n[1], n[1]]
    assert opp._sets.tolist() == [[0, 2], [0, 2], [1, 3], [1, 3]] and opp._coefs.tolist() == [[1, -1], [1, -2], [1, 0], [1, -3]]
    assert all(a.repulsive_bank is None for a in plain.agents) and plain._sets is None


def test_opponent_arguments_are_refused_before_any_engine_call():
    from tests import helpers_noise as HZ
    RE = navsim_amd.MushroomRouteEnsemble
    routes, starts = HZ.ens_routes(), HZ.ens_starts()
    eng = HZ.FakeEngine()
    bad = [(3, "opponent must be None or a dict"), (dict(speed=1), "unknown keys"), (dict(gain=1.5), "a gain is an integer"),
           (dict(gain=1025), "a gain is an integer in \\[0, 1024\\]"), (dict(gain=-1), "a gain"), (dict(gain=True), "a gain"),
           (dict(gain=[1, 2]), "holds 2 values for 4 starts"), (dict(turn=[1.0]), "holds 1 values for 2 routes"),
           (dict(turn=float("nan")), "a turn is a finite angle"), (dict(turn="pi"), "a turn")]
    for opponent, msg in bad:
        with pytest.raises(ValueError, match=msg):
            RE.from_landscapes(_untrained_agent(eng), list(HZ.lands()), routes, starts, opponent=opponent)
        with pytest.raises(ValueError, match=msg):
            RE.from_routes_with(_untrained_agent(eng), [r for _, r in routes], starts, opponent=opponent)
    with pytest.raises(ValueError, match="opponent with populations"):
        RE.from_routes_with(_untrained_agent(eng), [r for _, r in routes], starts, opponent=dict(gain=1), populations=[None, None])
    assert eng.calls == []
    import inspect
    assert "opponent" not in inspect.signature(navsim_amd.InfomaxRouteEnsemble.from_routes_with).parameters
    assert "opponent" not in inspect.signature(navsim_amd.InfomaxRouteEnsemble.from_landscapes).parameters
    # a member with an opponent memory is a banked member: the other ensembles refuse it by name
    a = _untrained_agent(eng)
    a.memory_bank, a.repulsive_bank = 0, 2
    for E in (navsim_amd.MushroomEnsemble, navsim_amd.NavEnsemble):
        with pytest.raises(ValueError, match="MushroomRouteEnsemble"):
            E._check_member(a)
    # ... and it steps with its ensemble only: a step of its own would read the attractive bank alone
    with pytest.raises(ValueError, match="memory bank 0 .*MushroomRouteEnsemble"):
        a.step_forward()
    with pytest.raises(ValueError, match="MushroomRouteEnsemble"):
        navsim_amd.run_experiment(a, frames=3)
