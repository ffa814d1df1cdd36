"""Mushroom-body familiarity model, host side: the C ABI's surface, the factory's argument checks, the refusals of the batched and
sharded forms, and the properties of the NumPy restatement the GPU tests compare against (tests/helpers_mushroom.py) -- among them
what the inputs of the GPU tests must distinguish, so that a later change of a seed or a shape cannot hollow one out: the widest case
under 15-bit indices, the waves and trips that the long quotas choose their equals from, the two views of every slab test, and the
poses and headings of the sensed ones (taken here with the host sensor model, which is byte-equal to the device's)."""
import os
import re

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import mushroom_familiarity
from navsim_amd.util import mushroom_connectivity, reject_infomax, reject_mushroom
from tests import helpers_mushroom as H
from tests.conftest import REPO

NAMES = {"dv_mb_begin", "dv_mb_train_u8", "dv_mb_train_from_poses", "dv_mb_score_u8", "dv_mb_activity_u8", "dv_mb_sense_step",
         "dv_mb_read_weights", "dv_mb_set_weights", "dv_mb_info", "dv_mb_end"}


def test_header_and_bindings_agree_on_the_mb_names():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    declared = set(re.findall(r"\bint\s+(dv_mb_[a-z0-9_]*)\s*\(", header))
    assert declared == NAMES
    assert declared == {k for k in N.PROTOTYPES if k.startswith("dv_mb_")}
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert N.PROTOTYPES[name][0].__name__ == "c_int"
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(N.PROTOTYPES[name][1]), name      # argument counts as the header declares them
        assert callable(getattr(navsim_amd.FamiliarityEngine, name[3:])), name
    assert "mushroom_familiarity" in navsim_amd.__all__


def test_factory_checks_its_arguments():
    for bad in (3, -1, None, 1.5):
        with pytest.raises(ValueError, match="channel"):
            mushroom_familiarity(channel=bad)
    for bad in (0, -4, 2.5, None, "7"):
        with pytest.raises(ValueError, match="n_kc"):
            mushroom_familiarity(n_kc=bad)
    for bad in (0, 17, -1, 2.0, None):
        with pytest.raises(ValueError, match="fan_in"):
            mushroom_familiarity(fan_in=bad)
    for bad in (0, -0.1, 1.5, float("nan"), "0.01", None):
        with pytest.raises(ValueError, match="sparsity"):
            mushroom_familiarity(sparsity=bad)
    with pytest.raises(ValueError, match="one device"):
        mushroom_familiarity(devices=[0, 1])
    model = mushroom_familiarity(channel=1, n_kc=1043, fan_in=8, sparsity=0.02, seed=3)
    assert (model.metric, model.channel, model.n_kc, model.fan_in, model.n_active) == ("mushroom", 1, 1043, 8, 21)
    assert mushroom_familiarity(n_kc=10, sparsity=0.001).n_active == 1            # max(1, round(0.01))
    assert mushroom_familiarity().n_active == 200
    assert callable(model.make_engine) and callable(model.from_engine) and callable(model.begin)
    with pytest.raises(ValueError, match="Buffer dtype mismatch"):
        model(np.zeros((3, 4, 4, 3), dtype=np.float32))


def test_begin_hook_draws_the_public_connectivity():
    seen = {}

    class Engine(object):
        def mb_begin(self, h, w, conn, n_active, channel):
            seen.update(h=h, w=w, conn=conn, n_active=n_active, channel=channel)

    mushroom_familiarity(channel=0, n_kc=37, fan_in=10, sparsity=0.1, seed=37).begin(Engine(), 3, 5)
    assert (seen["h"], seen["w"], seen["n_active"], seen["channel"]) == (3, 5, 4, 0)
    assert seen["conn"].dtype == np.int32 and np.array_equal(seen["conn"], H.connectivity(37, 15, 10, 37))


def test_func_checks_fambuf_and_carries_the_extras():
    class Engine(object):
        def mb_score_u8(self, planes):
            assert planes.dtype == np.uint8 and planes.shape == (4, 5)
            return np.array([-12.0])

    func = mushroom_familiarity(channel=2).from_engine(Engine(), None)
    assert (func.max_familiarity, func.metric, func.channel) == (0.0, "mushroom", 2)
    assert isinstance(func.engine, Engine)
    for bad in (np.zeros(3, dtype=np.float32), [0.0, 0.0], np.zeros(3, dtype=np.int64)):
        with pytest.raises(ValueError, match="Buffer dtype mismatch for fambuf, expected 'double'"):
            func(np.zeros((4, 5, 3), dtype=np.uint8), bad)
    buf = np.full(6, np.nan)
    func(np.zeros((4, 5, 3), dtype=np.uint8), buf)         # the ONE value in EVERY entry
    assert np.all(buf == -12.0)
    func(np.zeros((4, 5), dtype=np.uint8), buf)            # a single-channel scene as it is


def test_batched_and_sharded_forms_reject_the_model():
    from navsim_amd import sharded, util

    class Agent(object):
        familiarity_model = mushroom_familiarity()
        _familiarity_func = None
        _engine = None
        training_path = None

    model = mushroom_familiarity()
    for refuse in (reject_mushroom, reject_infomax):
        with pytest.raises(ValueError, match="x does not take a mushroom-body model"):
            refuse(model, "x")
    with pytest.raises(ValueError, match="FamiliarityGroup does not take a mushroom-body model"):
        util.sads_familiarity(model, devices=[0])
    with pytest.raises(ValueError, match="sharded_sads_familiarity does not take a mushroom-body model"):
        sharded.sharded_sads_familiarity(model, None, 0, 1)
    with pytest.raises(ValueError, match="device_sharded_sads_familiarity does not take a mushroom-body model"):
        sharded.device_sharded_sads_familiarity(model, 0, 1, "cuda:0")
    with pytest.raises(ValueError, match="NavEnsemble does not take a mushroom-body model"):
        navsim_amd.NavEnsemble._check_member(Agent())
    with pytest.raises(ValueError, match="InfomaxEnsemble does not take a mushroom-body model"):
        navsim_amd.InfomaxEnsemble._check_member(Agent())
    # the Infomax message is as it was, and the other models pass
    with pytest.raises(ValueError, match="x does not take an Infomax model: it batches or shards a view library, and infomax_familiarity "
                                         "keeps none"):
        reject_infomax(navsim_amd.infomax_familiarity(), "x")
    reject_mushroom(navsim_amd.infomax_familiarity(), "x")
    reject_infomax(util.ssd_familiarity(), "x")
    reject_infomax(0.25, "x")


def test_connectivity_is_deterministic_in_the_seed():
    a, b = mushroom_connectivity(300, 40, 3, seed=32), mushroom_connectivity(300, 40, 3, seed=32)
    assert a.dtype == np.int32 and a.shape == (300, 3) and np.array_equal(a, b)
    assert a.min() >= 0 and a.max() < 40
    assert not np.array_equal(a, mushroom_connectivity(300, 40, 3, seed=33))
    assert np.array_equal(a, H.connectivity(300, 40, 3, 32))                 # the restatement's draw
    assert np.array_equal(mushroom_connectivity(5, 7, 2), mushroom_connectivity(5, 7, 2, seed=0))


# ---- the restatement's own properties --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(H.CASES))
def test_selection_is_the_stable_argsort_and_the_conditions_hold(key):
    """case_data asserts the three conditions of the helper; here the selection is rebuilt from the threshold and the quota -- the form
    the kernel computes it in -- and must be the stable argsort's set, and the tie rule must decide in every case."""
    d = H.case_data(key)
    a = H.activity(d["patches"], d["conn"])
    assert a.min() >= 0 and a.max() <= 255 * d["c"]
    for row, mask, thr in zip(a, d["mask"], d["thr"]):
        assert mask.sum() == d["n_active"]
        above = row > thr
        quota = d["n_active"] - int(above.sum())
        equals = np.flatnonzero(row == thr)
        assert 0 < quota <= len(equals)
        want = above.copy()
        want[equals[:quota]] = True
        assert np.array_equal(mask.astype(bool), want)
    ties = H.tie_counts(d["patches"], d["conn"], d["n_active"])
    print("mushroom %s: zero fraction %.2f, (above, at) the threshold of the first patch %r, d %r"
          % (key, float((d["wt"] == 0).mean()), ties[0], d["d"][:6].tolist()))
    if key != "20x13_all_fire":
        assert any(at > d["n_active"] - ab for ab, at in ties)               # more cells at the threshold than places left
    assert np.array_equal(H.bits(d["fam"]), H.bits((-d["d"]).astype(np.float64))) and d["fam"].max() == 0.0


@pytest.mark.parametrize("key", ["5x3_k37", "40x1_k300", "16x16_k1043", "20x13_k257_half"])
def test_training_has_no_order_and_is_idempotent(key):
    d = H.case_data(key)
    ones = np.ones(d["K"], np.uint8)
    args = (d["conn"], d["n_active"])
    assert np.array_equal(H.train(ones, d["views"][::-1], *args), d["wt"])
    cut = max(1, d["F"] // 3)
    assert np.array_equal(H.train(H.train(ones, d["views"][:cut], *args), d["views"][cut:], *args), d["wt"])
    assert np.array_equal(H.train(H.train(ones, d["views"][cut:], *args), d["views"][:cut], *args), d["wt"])
    assert np.array_equal(H.train(d["wt"], np.repeat(d["views"], 2, axis=0), *args), d["wt"])


@pytest.mark.parametrize("key", H.CONSTANT_KEYS)
def test_constant_planes_fire_the_first_cells(key):
    d, k = H.case_data(key), H.constant_data(key)
    assert k["planes"].shape == (3, d["h"], d["w"]) and k["mask"].sum(axis=1).tolist() == [d["n_active"]] * 3
    assert k["thr"][0] == 0 and k["thr"][1] == 255 * d["c"] and 0 <= k["thr"][2] <= 255 * d["c"]
    assert len(np.unique(H.activity(k["planes"][2:], d["conn"]))) > 2           # the two-level plane spreads the cells


def test_the_widest_case_needs_all_sixteen_index_bits():
    d = H.case_data("256x256_k1043_c16")
    assert d["N"] == 65536 and d["conn"].max() >= 65000 and 0.45 < float((d["conn"] >= 32768).mean()) < 0.55
    low_mask, low_thr = H.fired_mask(d["patches"], d["conn"] & 0x7fff, d["n_active"])
    print("mushroom 256x256: thresholds %r, with 15-bit indices %r" % (d["thr"].tolist(), low_thr.tolist()))
    assert (low_mask != d["mask"]).any(axis=1).all()                          # (case_data asserts it too)
    ties = H.tie_counts(d["patches"], d["conn"], d["n_active"])
    assert sum(at > d["n_active"] - ab for ab, at in ties) >= 2               # the tie rule decides on more than one patch
    assert d["d"].max() > 0 and d["d"][-1] == 0


@pytest.mark.parametrize("n_active", H.LONG_QUOTA["n_active"])
def test_long_quotas_choose_equals_beyond_the_first_wave(n_active):
    q = H.quota_data(n_active)
    span = H.wave_span(q["K"])
    assert span == 320 and q["K"] > 3 * span                                  # four waves, the last one ragged
    assert q["mask"].sum(axis=1).tolist() == [n_active] * 3
    for plane in q["planes"][:2]:                                             # constant: every cell an equal, the first n_active chosen
        assert np.array_equal(H.chosen_equals(plane, q["conn"], n_active), np.arange(n_active))
    chosen = H.chosen_equals(q["planes"][2], q["conn"], n_active)
    waves, trips = sorted(set((chosen // span).tolist())), sorted(set(((chosen % span) // 64).tolist()))
    print("mushroom long quota %d: halves plane, threshold %d, %d chosen equals in waves %r, trips %r"
          % (n_active, q["thr"][2], len(chosen), waves, trips))
    assert len(chosen) >= 1
    if n_active in (320, 321, 1000):
        assert waves == [0, 1, 2] and trips == [0, 1, 2, 3, 4]
    if n_active == 1042:
        assert waves == [2] and len(chosen) == 1
    assert n_active > 64                                                      # the constant planes' quota leaves wave 0's first trip
    # more equals than places: the rank decides
    a = H.activity(q["planes"][2:], q["conn"])[0]
    assert int((a == q["thr"][2]).sum()) > len(chosen)


def test_slab_inputs_are_two_views_that_differ():
    views, stage = H.slab_views()
    t = H.slab_train_data()
    slab = stage // t["N"]
    assert 1 < slab < views and (slab + 1) * t["N"] > stage                   # the bytes end a slab of 128x128 planes
    assert not np.array_equal(t["both"], t["first"])                          # the view behind the edge brings cells
    assert 0 < (t["both"] == 0).sum() <= t["K"] // 2
    fam = H.familiarity(t["first"], t["two"], t["conn"], t["n_active"])
    assert H.bits(fam[:1])[0] == 0 and fam[1] < 0
    d = H.case_data(H.SLAB_ACTIVITY["key"])
    assert 1 < stage // d["K"] < views and stage // d["K"] < stage // d["N"]  # the fired masks end a slab of the activity call
    assert not np.array_equal(d["mask"][0], d["mask"][1]) and d["thr"][0] != d["thr"][1]
    assert len({d["mask"][i].tobytes() for i in range(3)}) == 3               # (the three patches of the optional-output calls)


def test_slab_poses_and_headings_distinguish():
    from tests import helpers_infomax as HI
    m = H.SLAB_POSES
    conn = H.connectivity(m["K"], 1024, m["c"], m["seed"])
    ones = np.ones(m["K"], np.uint8)
    path = H.sensed_route()
    i0, i1 = m["poses"]
    head = H.route_headings(path)
    two = H.host_sensed_planes(path[[i0, i1], 0], path[[i0, i1], 1], head[[i0, i1]])
    assert np.array_equal(two, HI.sensed_data()["views"][[i0, i1]])            # (the agent's own training views)
    assert not np.array_equal(H.train(ones, two, conn, m["n_active"]), H.train(ones, two[:1], conn, m["n_active"]))
    x, y = H.step_xy()
    planes = H.host_sensed_planes(x, y, m["angles"])
    for trained in (0, 1):
        fam = H.familiarity(H.train(ones, planes[trained:trained + 1], conn, m["n_active"]), planes, conn, m["n_active"])
        assert H.bits(fam[trained:trained + 1])[0] == 0 and fam[1 - trained] < 0
    # the 300 headings of the decide test, under the route's weights: a best and a worst to plant
    angles = H.circle_angles(300)
    assert len(np.unique(angles)) == 300
    conn = H.connectivity(4100, 1024, 10, 41)
    wt = H.train(np.ones(4100, np.uint8), HI.sensed_data()["views"], conn, 41)
    want = H.familiarity(wt, H.host_sensed_planes(x, y, angles), conn, 41)
    print("mushroom decide: 300 headings score %g .. %g, %d values, first maximum at %d"
          % (want.min(), want.max(), len(np.unique(want)), int(np.argmax(want))))
    assert want.max() > want.min()


def test_slab_size_is_read_from_the_kernel_file():
    views, stage = H.slab_views()
    assert views >= 1 and stage >= 65536
    assert (views + 1) * 15 <= stage            # at 5x3 the view count, not the bytes, ends a slab
