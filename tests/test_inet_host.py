"""Network tables of the Infomax model without a device: the binding surface of the dv_inet_* calls, where the kernels live, the engine's
argument checks (made before any library call), util.infomax_network against the draws of infomax_familiarity's begin, and the networks=
plumbing of InfomaxRouteEnsemble against a fake engine's call log (tests/helpers_inet.py), and the layouts of the steps that run past one
launch: where the cut falls by the kernel file's constants, what a launch-local index would change, the tolerance rule on them."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import infomax_familiarity, infomax_network
from tests import helpers_inet as HN
from tests import helpers_infomax as H
from tests import helpers_infomax_banks as HB

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"dv_inet_set": "inet_set", "dv_inet_clear": "inet_clear", "dv_inet_info": "inet_info"}
KERNELS = {"k_inet_prep", "k_inet_gemv", "k_inet_upart", "k_inet_ureduce", "k_inet_update", "k_inet_finite", "k_inet_score_cols", "k_inet_decide"}
# the banked surface as it stood before there were tables: (return type, number of arguments)
IBANK = {"dv_ibank_set": 3, "dv_ibank_train_u8": 4, "dv_ibank_train_from_poses": 7, "dv_ibank_step_u8": 7, "dv_ibank_sense_step": 10,
         "dv_ibank_read_weights": 3, "dv_ibank_set_weights": 3, "dv_ibank_info": 4}


# ---- binding surface -------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_engine_agree_on_the_inet_names():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    declared = set(re.findall(r"\bint\s+(dv_inet_[a-z0-9_]*)\s*\(", header))
    assert declared == set(NAMES) == {k for k in N.PROTOTYPES if k.startswith("dv_inet_")}
    assert not any(k.startswith(("dv_ibank_", "dv_infomax")) for k in declared)           # (the closed sets of the two older surfaces)
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert N.PROTOTYPES[name][0] is ctypes.c_int
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(N.PROTOTYPES[name][1]), name
        assert callable(getattr(navsim_amd.FamiliarityEngine, NAMES[name])), name
    # the banked calls serve the table with no new argument
    assert {k: len(v[1]) for k, v in N.PROTOTYPES.items() if k.startswith("dv_ibank_")} == IBANK
    assert len(N.PROTOTYPES["dv_lands_ibank_train_from_poses"][1]) == 8 and len(N.PROTOTYPES["dv_lands_ibank_sense_step"][1]) == 11
    for name, n in IBANK.items():
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == n, name
    for call in ("from_routes_with", "from_landscapes"):
        assert list(inspect.signature(getattr(navsim_amd.InfomaxRouteEnsemble, call)).parameters)[-1] == "networks"
    assert list(inspect.signature(navsim_amd.InfomaxRouteEnsemble.from_routes).parameters) == ["agent", "routes", "starts"]
    assert "infomax_network" in navsim_amd.__all__


def test_the_kernels_live_in_their_own_file_and_the_bodies_are_read_not_copied():
    csrc = os.path.join(REPO, "navigation-by-deja-vu_amd", "csrc")
    new = open(os.path.join(csrc, "dejavu_inet.inl")).read()
    assert set(re.findall(r"\bvoid\s+(k_[a-z0-9_]+)\s*\(", new)) == KERNELS
    for body in ("im_prep_view", "im_gemv_rows", "im_upart_cols", "im_ureduce_cols", "im_update_rows", "im_any_not_finite", "im_decide_member"):
        assert len(re.findall(r"^\s+(?:if \()?%s\(" % body, new, re.M)) == 1, body       # one call each: the banked twin's own body
    assert len(re.findall(r"\bim_score_tile<[124], VEC>\(", new)) == 3
    assert "atomic" not in new and "asm" not in new and "__builtin_amdgcn_mfma" not in new
    old = open(os.path.join(csrc, "dejavu_infomax.inl")).read()
    assert not re.findall(r"\bvoid\s+(k_inet[a-z0-9_]*)\s*\(", old)
    assert '#include "dejavu_inet.inl"' in open(os.path.join(csrc, "dejavu_hip.hip")).read()
    assert "dejavu_inet.inl" in open(os.path.join(csrc, "Makefile")).read()


# ---- a step past one launch: the layouts of tests/test_gpu_inet.py reach the edges they are there for ---------------------------------------
def test_step_slabs_states_the_cut_of_the_kernel_files_constants():
    stage, cols_max, heads = HN.slab_constants()
    src = open(os.path.join(REPO, "navigation-by-deja-vu_amd", "csrc", "dejavu_infomax.inl")).read()
    for name in ("kImStageBytes", "kImSlabColsMax", "kImHeadings"):
        assert len(re.findall(r"constexpr\s+[a-z_ ]+\s+%s\s*=" % name, src)) == 1, name
    assert "nk < (size_t)(kImSlabColsMax / kImHeadings) && nc + blocks[k0 + nk].nc <= slab" in src        # the rule step_slabs restates
    assert heads == 64 and stage % (8 * heads) == 0 and cols_max % heads == 0
    slab = stage // (8 * 1024)
    # one bank: whole blocks fill the slab to its last column, and the next block begins the next launch
    assert [(c0, nc, len(b)) for c0, nc, b in HN.step_slabs([slab + 1], 1, 1024)] == [(0, slab, slab // heads), (slab, 1, 1)]
    # two banks: the first one's ragged block leaves the slab short, and no block mixes banks
    got = HN.step_slabs([3, slab], 1, 1024)
    assert [(c0, nc, len(b)) for c0, nc, b in got] == [(0, 3 + slab - heads, slab // heads), (3 + slab - heads, heads, 1)]
    assert got[0][2][0] == (0, 0, 3, 0) and got[0][2][1] == (1, 3, heads, heads) and got[1][2][0] == (1, 3 + slab - heads, heads, slab)
    # an empty bank has no block; a call within the slab is one launch
    assert HN.step_slabs([2, 0, 1], 70, 35) == [(0, 210, [(0, 0, 64, 0), (0, 64, 64, 64), (0, 128, 12, 128), (2, 140, 64, 192), (2, 204, 6, 256)])]
    # the widest step of the tests before these: 14 members x 70 headings at N = 35, one launch
    assert len(HN.step_slabs(np.bincount(HN.STEP_BANKS, minlength=7).tolist(), 70, 35)) == 1


def _own_bank_score(d):
    return lambda bank, planes: H.familiarity(d["Ws"][bank], planes)


def test_the_slab_layout_cuts_a_member_of_bank_1_and_a_wrong_index_would_show():
    lay, d = HN.slab_layout(), HN.slab_step_data()
    A, c0 = lay["A"], lay["c0"]
    assert (c0, lay["nc1"], lay["nc2"], lay["slab"], lay["cut"]) == (8176, 8176, 80, 8192, 4) and d["N"] % 4 == 0
    assert [b[:3] for b in lay["launches"][1][2]] == [(1, 8176, 44), (2, 8220, 24), (3, 8244, 12)]
    assert [len(b) for _, _, b in lay["launches"]] == [128, 3] and sorted(set(b[2] for b in lay["launches"][0][2])) == [48, 64]
    assert np.bincount(d["banks"]).tolist() == list(HN.SLAB["members"]) and (np.diff(d["banks"]) < 0).any()   # the caller's order is not sorted
    assert [net["n_hidden"] for net in d["nets"]] == [49, 17, 33, 5] and [net["channel"] for net in d["nets"]] == [2, 0, 1, 0]
    assert np.bincount(d["bank_of"]).tolist() == list(HN.SLAB["trained"]) and d["bank_of"][:4].tolist() == [0, 1, 2, 3]
    s = lay["straddler"]
    assert lay["place"][s] * A < c0 < (lay["place"][s] + 1) * A and d["first"][s] < lay["cut"] <= d["second"][s]
    print("%s: two equal maxima a member, ahead of the third by at least %.2e relative" % (HN.SLAB_NAME, d["margin"]))
    cols = d["planes"][lay["order"]].reshape((-1,) + d["planes"].shape[2:])
    bank, x = HN.wrong_index_margins(lay, cols, _own_bank_score(d))
    told = ~np.isnan(x)
    print("    launch 2 under the bank of the launch-local place: off by %.2e at least; X read at c %% slab: off by %.2e at least (%d of %d columns)"
          % (bank.min(), x[told].min(), told.sum(), len(x)))
    assert bank.min() > 1e-6 and x[told].min() > 1e-6 and told.sum() == lay["nc2"] - (lay["slab"] - c0)
    mine = slice(0, A - lay["cut"])                                                        # the straddling member's columns of launch 2
    assert bank[mine].min() > 1e-6 and np.isnan(x[mine]).all()                             # (X behind launch 1's columns: nothing of this call)
    # ... so for the straddling member: x_first taken at its member's first column, or at a whole block (X read `cut` or c0 % 64 columns on)
    right = d["fam"][s, lay["cut"]:]
    assert np.array_equal(right, H.familiarity(d["Ws"][1], cols[c0:c0 + A - lay["cut"]]))
    for shift in (lay["cut"], c0 % 64):
        held = cols[c0 + shift:c0 + shift + A - lay["cut"]]
        assert (np.abs(H.familiarity(d["Ws"][1], held) - right) / np.abs(right)).min() > 1e-6, shift


def test_the_tolerance_rule_on_the_slab_layouts_weights_and_scores():
    d = HN.slab_step_data()
    w = HN.weight_discrepancy(d["nets"], d["net_of_bank"], d["views"], d["bank_of"], d["Ws"])
    s = HN.score_discrepancy(lambda **kw: HN.scores(d["nets"], d["net_of_bank"], d["Ws"], d["planes"], d["banks"], **kw), d["fam"])
    print("%s, uploaded: largest discrepancy of the statement: weights %.2e, scores %.2e (1000 x under TOL %.1e)" % (HN.SLAB_NAME, w, s, H.TOL))
    assert 1000 * max(w, s) <= H.TOL


def test_the_sensed_slab_layout_mixes_channels_and_landscapes_across_the_cut():
    from tests import helpers_lands as HL
    lay, d = HN.slab_layout(), HN.slab_sense_data()
    A, c0, order = lay["A"], lay["c0"], lay["order"]
    assert HL.SENSORS["sq"]["sensor"] == (HN.SLAB["w"], HN.SLAB["h"])
    # the first column of launch 2: bank 1 reads channel 0, the bank of the launch-local place (bank 0) channel 2, and the planes differ
    s, a = lay["straddler"], lay["cut"]
    assert order[c0 // A] == s and d["banks"][order[0]] == 0 and (d["nets"][0]["channel"], d["nets"][1]["channel"]) == (2, 0)
    for scenes in (d["scenes_set"], d["scenes_one"]):
        assert not np.array_equal(scenes[s, a, ..., 0], scenes[s, a, ..., 2])
        wrong = H.familiarity(d["Ws"][1], scenes[s, a:a + 1, ..., 2])[0]
        right = H.familiarity(d["Ws"][1], scenes[s, a:a + 1, ..., 0])[0]
        assert abs(wrong - right) / abs(right) > 1e-6
    # every member of launch 2 stands on another landscape than the member at its launch-local place, and its view there is another
    behind = order[c0 // A:]
    local = order[:len(behind)]
    assert (d["lands"][behind] != d["lands"][local]).all() and len(set(d["lands"][behind].tolist())) > 1
    for i, j in zip(behind, local):
        assert not np.array_equal(d["scenes_set"][i, A - 1], HL.host_scene("sq", d["xs"][i], d["ys"][i], d["angs"][i, A - 1], d["lands"][j]))
    # the set's and the one landscape's steps differ where a member is not on landscape 0
    off0 = d["lands"] != 0
    assert (np.abs(d["fam_set"][off0] - d["fam_one"][off0]).max(axis=1) > 1e-6 * np.abs(d["fam_one"][off0]).max()).all()
    assert np.array_equal(d["fam_set"][~off0], d["fam_one"][~off0])
    # the member that is moved off its landscape lies behind c0 and is not the straddling one
    m = d["flagged"]
    assert lay["place"][m] * A >= c0 + A and m != s and lay["place"][m] != len(order) - 1
    x, y, l = HN.OFF_THE_SET
    assert all(HL.is_off("sq", x, y, ang, l) for ang in d["angs"][m]) and all(HL.is_off("sq", *HN.OFF_THE_ONE, ang, 0) for ang in d["angs"][m])
    worst = 0.0
    for scenes, fam in ((d["scenes_set"], d["fam_set"]), (d["scenes_one"], d["fam_one"])):
        worst = max(worst, HN.score_discrepancy(lambda **kw: HN.scores(d["nets"], d["net_of_bank"], d["Ws"], scenes, d["banks"], **kw), fam))
    print("%s, sensed: largest discrepancy of the statement's scores %.2e (1000 x under TOL %.1e)" % (HN.SLAB_NAME, worst, H.TOL))
    assert 1000 * worst <= H.TOL


def test_the_blocks_layout_is_16384_blocks_and_one_and_a_wrong_bank_would_show():
    d = HN.blocks_data()
    B, A = HN.BLOCKS["banks"], d["A"]
    assert [(c0, nc, len(b)) for c0, nc, b in d["launches"]] == [(0, 49152, 16384), (49152, 3, 1)] and d["N"] % 4 != 0 and A == 3
    assert sorted(d["banks"].tolist()) == list(range(B)) and d["last"] != B - 1 and d["banks"][d["last"]] == B - 1
    M = np.array([net["n_hidden"] for net in d["nets"]])
    assert M.tolist() == [1, 3, 17] and M[d["net_of_bank"][B - 1]] == 3 and M[d["net_of_bank"][B - 2]] == 17
    assert (d["net_of_bank"][:B - 2] == np.arange(B - 2) % 3).all() and sorted(d["trained"]) == [0, B - 2, B - 1]
    assert d["bank_of"].tolist() == [0, B - 2, B - 1] * 3
    # launch 2's row under the bank of sorted place 0 (bank 0) and under the bank one block back (bank 16383)
    i = d["last"]
    right = d["fam"][i]
    assert right.tolist() == H.familiarity(d["trained"][B - 1], d["planes"][i]).tolist()
    assert (np.abs(H.familiarity(d["trained"][0], d["planes"][i]) - right) / np.abs(right)).min() > 1e-6
    assert (np.abs(H.familiarity(d["trained"][B - 2], d["planes"][i]) - right) / np.abs(right)).min() > 1e-6
    j = int(d["order"][B - 2])
    assert d["fam"][j].tolist() == H.familiarity(d["trained"][B - 2], d["planes"][j]).tolist()
    # ... and read at the launch-local column of X, the planes of the member at place 0
    assert (np.abs(H.familiarity(d["trained"][B - 1], d["planes"][d["order"][0]]) - right) / np.abs(right)).min() > 1e-6
    lay = HN.blocks_layout()
    kinds, w0s = d["net_of_bank"], [net["w0"] for net in d["nets"]]
    s = HN.score_discrepancy(lambda **kw: HN.blocks_scores(lay, kinds, w0s, d["trained"], **kw), d["fam"])
    w = max(H.chain_discrepancy(d["nets"][kinds[b]]["w0"], d["views"][d["bank_of"] == b], W, d["nets"][kinds[b]]["learning_rate"])
            for b, W in d["trained"].items())
    print("%s: largest discrepancy of the statement: weights %.2e, scores %.2e (1000 x under TOL %.1e)" % (HN.BLOCKS_NAME, w, s, H.TOL))
    assert 1000 * max(w, s) <= H.TOL


# ---- infomax_network ---------------------------------------------------------------------------------------------------------------------------
class _Begun(object):
    """Stands where the engine does for a model's begin: keeps what infomax_begin is given."""
    def infomax_begin(self, h, w, weights, channel=2, learning_rate=0.01):
        self.got = (h, w, weights, channel, learning_rate)


def test_infomax_network_draws_what_the_models_begin_draws():
    net = infomax_network(35, n_hidden=63, learning_rate=0.005, seed=41, channel=1)
    assert sorted(net) == ["channel", "learning_rate", "n_hidden", "w0"]
    assert (net["channel"], net["n_hidden"], net["learning_rate"]) == (1, 63, 0.005)
    assert net["w0"].dtype == np.float64 and np.array_equal(net["w0"], H.initial_weights(63, 35, 41))
    e = _Begun()
    infomax_familiarity(channel=1, learning_rate=0.005, seed=41, n_hidden=63).begin(e, 5, 7)
    assert e.got[:2] == (5, 7) and e.got[3:] == (1, 0.005) and np.array_equal(e.got[2], net["w0"])
    d = infomax_network(120)                                                              # n_hidden None: as many rows as pixels
    infomax_familiarity().begin(e, 10, 12)
    assert (d["n_hidden"], d["learning_rate"], d["channel"]) == (120, 0.01, 2) and np.array_equal(e.got[2], d["w0"])
    model = infomax_familiarity(learning_rate=0.02, seed=5, n_hidden=9)
    assert (model.learning_rate, model.seed, model.n_hidden, model.channel) == (0.02, 5, 9, 2)
    for bad in (dict(n_hidden=0), dict(learning_rate=0.0), dict(learning_rate=np.inf), dict(channel=3)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            infomax_network(35, **bad)
    for bad in (0, -3, 2.5, None, True):
        with pytest.raises(ValueError, match="n_pixels"):
            infomax_network(bad)


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
    e._lib, e._ctx_raw, e._begun, e.infomax_shape, e.sensor_shape, e.infomax_banks = lib, None, False, shape, shape, 1
    return e


def test_every_refusal_comes_before_any_library_call():
    h, w = 5, 7
    lib = _Recorder()
    e = _engine_without_a_device(lib, (h, w))
    good = HN.network(h * w, 63, 0.005, 1)

    def but(**kw):
        keep = {k: v for k, v in good.items() if "w0" not in kw or k != "n_hidden"}      # (another w0: its own shape)
        return dict(keep, **kw)

    w0 = good["w0"]
    bad_nets = (
        (but(learning_rate=0.0), r"networks\[1\]: learning_rate 0.0 must be a positive number"),
        (but(learning_rate=-0.01), r"networks\[1\]: learning_rate"),
        (but(learning_rate=np.inf), r"networks\[1\]: learning_rate inf"),
        (but(learning_rate=np.nan), r"networks\[1\]: learning_rate nan"),
        (but(learning_rate="0.01"), r"networks\[1\]: learning_rate"),
        (but(learning_rate=True), r"networks\[1\]: learning_rate"),
        (but(channel=3), r"networks\[1\]: channel 3 outside \[0, 2\]"),
        (but(channel=-1), r"networks\[1\]: channel"),
        (but(channel=1.0), r"networks\[1\]: channel"),
        (but(w0=w0[:0]), r"networks\[1\]: n_hidden 0 outside \[1, 1048576\]"),
        (but(w0=w0.astype(np.float32)), r"networks\[1\]: w0 must be float64, got dtype float32"),
        (but(w0=w0.astype(np.int64)), r"networks\[1\]: w0 must be float64"),
        (but(w0=w0.reshape(-1)), r"networks\[1\]: w0 must be float64\[n_hidden, 35\], got shape \(2205,\)"),
        (but(w0=w0[:, :34]), r"networks\[1\]: w0 must be float64\[n_hidden, 35\], got shape \(63, 34\)"),
        (but(n_hidden=64), r"networks\[1\]: n_hidden = 64, but w0 has shape \(63, 35\)"),
        (but(weights=1), r"networks\[1\]: unknown keys \['weights'\]"),
        ({k: v for k, v in good.items() if k != "w0"}, r"networks\[1\] must be a dict with w0 and learning_rate"),
        ({k: v for k, v in good.items() if k != "learning_rate"}, r"networks\[1\] must be a dict with w0 and learning_rate"),
        ([1, 2], r"networks\[1\] must be a dict"),
    )
    for net, message in bad_nets:
        with pytest.raises(ValueError, match=message):
            e.inet_set([good, net], [0, 1])
    for nets in ([], None, good, 3):
        with pytest.raises(ValueError, match="networks must be a list of one or more dicts"):
            e.inet_set(nets, [0])
    for table, message in (([0, 2], r"network_of_bank\[1\] = 2 outside \[0, n_nets = 2\)"), ([-1, 0], r"network_of_bank\[0\] = -1"),
                           ([0.0, 1.0], "network_of_bank must hold integers"), ([[0, 1]], "network_of_bank must have one dimension"),
                           ([], "network_of_bank must name the network of 1 to 65535 banks, got 0"),
                           (np.zeros(65536, np.int32), "network_of_bank must name the network of 1 to 65535 banks, got 65536")):
        with pytest.raises(ValueError, match=message):
            e.inet_set([good, good], table)
    assert lib.calls == [] and e.infomax_nets is None and e.infomax_banks == 1
    # a table that holds: one call, with the arguments the binding declares; the engine knows the ragged shapes from then on
    lib.dv_infomax_info = lambda *args: 0                                                 # (n_hidden and n_pixels stay 0: the library's to say)
    tall = HN.network(h * w, 257, 0.01, 2, channel=0)
    e.inet_set([good, tall], np.array([1, 0, 1], dtype=np.int64))
    assert lib.calls == [("dv_inet_set", len(N.PROTOTYPES["dv_inet_set"][1]))] and e.infomax_banks == 3
    assert [p["n_hidden"] for p in e.infomax_nets] == [63, 257] and e.infomax_net_of_bank.tolist() == [1, 0, 1] and "w0" not in e.infomax_nets[0]
    assert [p["learning_rate"] for p in e.infomax_nets] == [0.005, 0.01] and [p["channel"] for p in e.infomax_nets] == [2, 0]
    del lib.calls[:]
    for bank in (3, -1, 1.0, None, True):
        with pytest.raises(ValueError, match="bank must be an integer"):
            e.ibank_set_weights(bank, w0)
    for table in ([0, 1, 3, 0], [0, -1, 1, 2]):
        with pytest.raises(ValueError, match="bank_of_view"):
            e.ibank_train_u8(np.zeros((4, h, w), np.uint8), table)
    assert lib.calls == []
    assert [e.ibank_read_weights(b).shape[0] for b in range(3)] == [257, 63, 257]         # the bank's own rows
    assert lib.calls == [("dv_ibank_read_weights", 3)] * 3
    # inet_clear, ibank_set, infomax_begin and infomax_end each forget the table
    for drop in (lambda: e.inet_clear(), lambda: e.ibank_set(2, w0), lambda: e.infomax_begin(h, w, w0), lambda: e.infomax_end()):
        e.infomax_shape = (h, w)
        e.inet_set([good], [0, 0])
        assert e.infomax_nets is not None
        drop()
        assert e.infomax_nets is None and e.infomax_net_of_bank is None and e.infomax_banks == (2 if lib.calls[-1][0] == "dv_ibank_set" else 1)
    e.infomax_shape = None                                                                # no model: the library answers DV_ERR_STATE
    del lib.calls[:]
    e.inet_set([but(w0=w0[:, :34])], [0])
    assert lib.calls == [("dv_inet_set", 8)]


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


MODEL = dict(channel=2, learning_rate=1e-3, seed=6, n_hidden=30)


def _from_routes(networks, metrics="host"):
    eng = HN.FakeEngine(10, 12)
    paths = HB.routes()
    agent = _Agent(eng, infomax_familiarity(**MODEL))
    ens = navsim_amd.InfomaxRouteEnsemble.from_routes_with(agent, paths, HB.starts(paths), metrics=metrics, networks=networks)
    return eng, ens, paths


def test_networks_none_logs_todays_calls():
    eng, ens, paths = _from_routes(None)
    assert eng.log == [("infomax_begin", 10, 12, (30, 120), 2, 1e-3), ("infomax_read_weights",), ("ibank_set", 3, (30, 120)),
                       ("ibank_train_from_poses", sum(len(p) for p in paths), [0, 1, 2])]
    assert all(a.network_index is None and a.network is None for a in ens.agents)
    info = ens.bank_info()
    assert eng.log[-1] == ("ibank_info",) and len(eng.log) == 5
    assert info["n_hidden"].tolist() == [30] * 3 and info["learning_rate"].tolist() == [1e-3] * 3 and info["network_of_bank"].tolist() == [0] * 3
    plain = navsim_amd.InfomaxRouteEnsemble.from_routes(_Agent(HN.FakeEngine(10, 12), infomax_familiarity(**MODEL)), paths, HB.starts(paths))
    assert plain.engine.log == eng.log[:4]


def test_equal_entries_share_one_network_and_members_carry_theirs():
    nets = [None, dict(n_hidden=70, seed=7), dict(seed=6, n_hidden=30)]                   # the third equals the model's own: one network
    eng, ens, paths = _from_routes(nets)
    assert [c[0] for c in eng.log] == ["infomax_begin", "inet_set", "ibank_train_from_poses"]
    _, sent, of_bank = eng.log[1]
    own = dict(channel=2, n_hidden=30, learning_rate=1e-3, seed=6)
    other = dict(channel=2, n_hidden=70, learning_rate=1e-3, seed=7)
    assert sent == [own, other] and of_bank == [0, 1, 0]
    assert np.array_equal(eng.infomax_nets[1]["w0"], H.initial_weights(70, 120, 7)) and np.array_equal(eng.infomax_nets[0]["w0"], H.initial_weights(30, 120, 6))
    assert [a.memory_bank for a in ens.agents] == [0, 0, 1, 1, 2, 2] and [a.network_index for a in ens.agents] == [0, 0, 1, 1, 0, 0]
    assert ens.agents[2].network == other and ens.agents[5].network == own
    info = ens.bank_info()
    assert sorted(info) == ["finite", "learning_rate", "n_banks", "n_hidden", "network_of_bank", "views_trained"]
    assert info["n_hidden"].tolist() == [30, 70, 30] and info["learning_rate"].tolist() == [1e-3] * 3 and info["network_of_bank"].tolist() == [0, 1, 0]
    # a model of as many rows as pixels (n_hidden None) equals an entry that says so in numbers
    eng3 = HN.FakeEngine(10, 12)
    model = infomax_familiarity(learning_rate=1e-3, seed=6)
    ens3 = navsim_amd.InfomaxRouteEnsemble.from_routes_with(_Agent(eng3, model), paths, HB.starts(paths),
                                                            networks=[None, dict(n_hidden=120), dict(learning_rate=5e-4, channel=0)])
    assert eng3.log[1][2] == [0, 0, 1] and [n["n_hidden"] for n in eng3.log[1][1]] == [120, 120]
    assert eng3.log[1][1][1] == dict(channel=0, n_hidden=120, learning_rate=5e-4, seed=6)
    # a route under two networks is entered twice
    twice = [paths[0], paths[0], paths[1]]
    eng2 = HN.FakeEngine(10, 12)
    starts = [(0, (70.0, 70.0), 0.1), (1, (70.0, 70.0), 0.1), (2, (70.0, 70.0), 0.1)]
    ens2 = navsim_amd.InfomaxRouteEnsemble.from_routes_with(_Agent(eng2, infomax_familiarity(**MODEL)), twice, starts,
                                                            networks=[None, dict(learning_rate=5e-4, channel=0), None])
    assert eng2.log[1][2] == [0, 1, 0] and eng2.log[1][1][1]["learning_rate"] == 5e-4 and eng2.log[1][1][1]["channel"] == 0
    assert ens2.agents[0].training_path is ens2.agents[1].training_path and ens2.agents[1].network_index == 1


def test_networks_are_refused_by_entry_before_the_engine_is_asked():
    for bad, message in (([None, None], "one entry per route \\(3\\)"), (dict(n_hidden=3), "one entry per route"), ([None, 3, None], r"networks\[1\] must be None or a dict"),
                         ([None, None, dict(rows=5)], r"networks\[2\]: unknown keys \['rows'\]"),
                         ([dict(n_hidden=0), None, None], r"networks\[0\]: n_hidden must be a positive integer"),
                         ([None, dict(learning_rate=0), None], r"networks\[1\]: learning_rate"), ([None, dict(learning_rate=np.nan), None], r"networks\[1\]: learning_rate"),
                         ([None, None, dict(channel=5)], r"networks\[2\]: channel"), ([None, None, dict(seed=-1)], r"networks\[2\]: ")):
        eng = HN.FakeEngine(10, 12)
        with pytest.raises(ValueError, match=message):
            paths = HB.routes()
            navsim_amd.InfomaxRouteEnsemble.from_routes_with(_Agent(eng, infomax_familiarity(**MODEL)), paths, HB.starts(paths), networks=bad)
        assert eng.log == []


def test_population_entries_still_refuses_for_infomax():
    with pytest.raises(ValueError, match="InfomaxRouteEnsemble has no populations.*networks="):
        navsim_amd.InfomaxRouteEnsemble._population_entries(None, None, 3, [None] * 3)
    for call in ("from_routes_with", "from_landscapes"):
        assert "populations" not in inspect.signature(getattr(navsim_amd.InfomaxRouteEnsemble, call)).parameters
        assert list(inspect.signature(getattr(navsim_amd.MushroomRouteEnsemble, call)).parameters)[-1] == "populations"
