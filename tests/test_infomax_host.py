"""Infomax familiarity model, host side: the factory's argument checks, the C ABI's surface, and the NumPy restatement the GPU tests
compare against -- its discrepancy against itself (the source of the GPU tolerance), its margins and its divergence."""
import os
import re
import warnings

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import infomax_familiarity
from navsim_amd.util import infomax_initial_weights, reject_infomax
from tests import helpers_infomax as H
from tests.conftest import REPO

NAMES = {"dv_infomax_begin", "dv_infomax_train_u8", "dv_infomax_train_from_poses", "dv_infomax_score_u8", "dv_infomax_sense_step",
         "dv_infomax_read_weights", "dv_infomax_set_weights", "dv_infomax_info", "dv_infomax_end"}


def test_header_and_bindings_agree_on_the_infomax_names():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    declared = set(re.findall(r"\bint\s+(dv_infomax[a-z0-9_]*)\s*\(", header))
    assert declared == NAMES
    assert declared == {k for k in N.PROTOTYPES if k.startswith("dv_infomax")}
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert N.PROTOTYPES[name][0].__name__ == "c_int"
    # argument counts as the header declares them
    for name in declared:
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(N.PROTOTYPES[name][1]), name
    for name in ("infomax_begin", "infomax_train_u8", "infomax_train_from_poses", "infomax_score_u8", "infomax_sense_step",
                 "infomax_read_weights", "infomax_set_weights", "infomax_info", "infomax_end"):
        assert callable(getattr(navsim_amd.FamiliarityEngine, name)), name
    assert "infomax_familiarity" in navsim_amd.__all__


def test_factory_checks_its_arguments():
    for bad in (3, -1, None, 1.5):
        with pytest.raises(ValueError, match="channel"):
            infomax_familiarity(channel=bad)
    for bad in (0, -0.01, float("nan"), float("inf"), "0.01"):
        with pytest.raises(ValueError, match="learning_rate"):
            infomax_familiarity(learning_rate=bad)
    for bad in (0, -4, 2.5):
        with pytest.raises(ValueError, match="n_hidden"):
            infomax_familiarity(n_hidden=bad)
    with pytest.raises(ValueError, match="one device"):
        infomax_familiarity(devices=[0, 1])
    model = infomax_familiarity(channel=1, learning_rate=0.02, seed=3, n_hidden=7)
    assert (model.metric, model.channel, model.learning_rate) == ("infomax", 1, 0.02)
    assert callable(model.make_engine) and callable(model.from_engine) and callable(model.begin)
    with pytest.raises(ValueError, match="uint8_t"):
        model(np.zeros((3, 4, 4, 3), dtype=np.float32))


def test_func_checks_fambuf_and_carries_the_extras():
    class Engine(object):
        def infomax_score_u8(self, planes):
            assert planes.dtype == np.uint8 and planes.shape == (4, 5)
            return np.array([-12.5])

    func = infomax_familiarity(channel=2).from_engine(Engine(), None)
    assert (func.max_familiarity, func.metric, func.channel) == (0.0, "infomax", 2)
    for bad in (np.zeros(3, dtype=np.float32), [0.0, 0.0], np.zeros(3, dtype=np.int64)):
        with pytest.raises(ValueError, match="Buffer dtype mismatch for fambuf, expected 'double'"):
            func(np.zeros((4, 5, 3), dtype=np.uint8), bad)
    buf = np.full(6, np.nan)
    func(np.zeros((4, 5, 3), dtype=np.uint8), buf)         # the ONE value in EVERY entry
    assert np.all(buf == -12.5)
    func(np.zeros((4, 5), dtype=np.uint8), buf)            # a single-channel scene as it is


def test_batched_and_sharded_forms_reject_the_model():
    from navsim_amd import sharded, util
    model = infomax_familiarity()
    with pytest.raises(ValueError, match="Infomax"):
        reject_infomax(model, "x")
    with pytest.raises(ValueError, match="FamiliarityGroup"):
        util.sads_familiarity(model, devices=[0])
    with pytest.raises(ValueError, match="sharded_sads_familiarity"):
        sharded.sharded_sads_familiarity(model, None, 0, 1)
    with pytest.raises(ValueError, match="device_sharded_sads_familiarity"):
        sharded.device_sharded_sads_familiarity(model, 0, 1, "cuda:0")
    reject_infomax(util.ssd_familiarity(), "x")
    reject_infomax(0.25, "x")


def test_initial_weights_are_the_restatements():
    W = infomax_initial_weights(24, 40, seed=13)
    assert W.tobytes() == H.initial_weights(24, 40, 13).tobytes()
    assert np.allclose(W.mean(axis=1), 0, atol=1e-15) and np.allclose(W.std(axis=1), 1, atol=1e-15)


@pytest.mark.parametrize("key", ["5x3_f1", "5x3_f2", "40x1", "16x16_a65", "20x13", "7x5_m1043", "33x31", "32x32_m1040"])
def test_restatement_against_itself_gives_the_gpu_tolerance(key):
    """float64 against longdouble and against a permuted summation order, at every GPU test shape: 1000 x the largest is the bound."""
    disc = H.discrepancies(key)
    print("infomax restatement %s: W/d vs longdouble %.2e %.2e, vs permuted order %.2e %.2e" % ((key,) + disc))
    assert 1000 * max(disc) <= H.TOL
    assert H.TOL <= 1e-11                                   # ... and the bound stays beside the 1e-12 score contract


@pytest.mark.parametrize("key", H.MEAN_KEYS)
def test_offset_weights_see_the_mean_and_keep_the_gpu_tolerance(key):
    """The cases whose rows of W sum to 1: the 1000 x rule holds under TOL as for the others, and -- what they are for -- a mean that
    misses one pixel moves their scores by far more than TOL, while the scores under the zero-sum weights of the plain case do not move."""
    d, plain = H.offset_case_data(key), H.case_data(key)
    assert d["N"] > 256 and np.isfinite(d["W"]).all() and np.abs(d["W"]).max() < 10
    disc = H.offset_discrepancies(key)
    print("infomax restatement %s from W0 + 1/N: W/d vs longdouble %.2e %.2e, vs permuted order %.2e %.2e" % ((key,) + disc))
    assert 1000 * max(disc) <= H.TOL
    assert np.abs(plain["W"].sum(axis=1)).max() < 1e-12 and np.abs(d["W"].sum(axis=1)).min() > 0.5
    moved = np.max(np.abs(H.familiarity_with_mean_off(d["W"], d["patches"], 1.0 / d["N"]) - d["fam"])) / np.max(np.abs(d["fam"]))
    blind = np.max(np.abs(H.familiarity_with_mean_off(plain["W"], plain["patches"], 1.0 / d["N"]) - plain["fam"])) / np.max(np.abs(plain["fam"]))
    print("    a mean one pixel short moves d by %.2e (zero-sum rows: %.2e)" % (moved, blind))
    assert moved > 1000 * H.TOL and blind < H.TOL
    assert H.best_margin(d["fam"]) > 1000 * H.TOL


def test_long_chain_has_a_bound_of_its_own_by_the_same_rule():
    """8197 views of 32x32 (the chain that crosses the training's staging slab): 1000 x its largest self-discrepancy is above TOL, and
    TOL_LONG_CHAIN is that figure rounded up to one digit.  Its cap is its own, not TOL's: within a factor of ten of the figure measured
    here, whichever NumPy measures it."""
    d = H.long_chain_data()
    assert d["F"] > (64 << 20) // (8 * d["N"]) and np.isfinite(d["W"]).all()
    disc = H.chain_discrepancy(d["W0"], d["views"], d["W"], H.ETA)
    print("infomax restatement, long chain: W vs longdouble / permuted order %.2e (max|W| %.3g)" % (disc, np.abs(d["W"]).max()))
    assert 1000 * disc > H.TOL                              # (why it is no member of CASES)
    assert 1000 * disc <= H.TOL_LONG_CHAIN <= 10000 * disc


def test_sensed_chain_is_held_to_the_gpu_tolerance():
    """The 45 sensed 32x32 views of the agent test at 1040 rows (host sensor model, a plug-in without an engine): the chain passes the
    1000 x rule under TOL, so the device's weights after train_from_path are held to TOL."""
    s = H.sensed_data()
    assert s["views"].shape == (45, 32, 32) and s["W"].shape == (1040, 1024) and np.isfinite(s["W"]).all()
    assert len(np.unique(s["views"])) > 1
    disc = H.chain_discrepancy(s["W0"], s["views"], s["W"], s["eta"])
    print("infomax restatement, sensed chain: W vs longdouble / permuted order %.2e (max|W| %.3g)" % (disc, np.abs(s["W"]).max()))
    assert 1000 * disc <= H.TOL


def test_restatement_separates_trained_from_novel_views():
    d = H.case_data("16x16_a16")
    assert np.isfinite(d["W"]).all() and np.abs(d["W"]).max() < 10
    trained = d["fam"][::3]
    novel = np.delete(d["fam"], np.s_[::3])
    assert trained.min() > novel.max()                      # every trained view is more familiar than every novel one
    # and the untrained network does not separate them like that
    f0 = H.familiarity(d["W0"], d["patches"])
    assert not (f0[::3].min() > np.delete(f0, np.s_[::3]).max())


@pytest.mark.parametrize("key", [k for k, c in H.CASES.items() if c["A"] > 1])
def test_best_heading_of_every_case_is_clear_of_the_tolerance(key):
    assert H.best_margin(H.case_data(key)["fam"]) > 1000 * H.TOL


def test_diverging_rate_overflows_the_restatement():
    d = H.case_data("16x16_a16")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        W = H.train(d["W0"], d["views"], eta=H.diverging_eta())
        W10 = H.train(d["W0"], d["views"], eta=H.diverging_eta() / 10)
    assert not np.isfinite(W).all() and not np.isfinite(W10).all()
    assert np.isfinite(d["W"]).all()                        # (ETA)
