"""Mushroom-body familiarity model on the device against its NumPy restatement (tests/helpers_mushroom.py): integers from pixel to score,
so every comparison is exact -- np.array_equal, floats through their uint64 view (H.bits).  No tolerance anywhere.

Shapes (H.CASES): K below one wave with c close to N; one winner taken from the tie bin; ragged K with more than 64 headings; the
default K = 20000 (many trips per wave) with N % 4 != 0; the widest histogram (c = 16: 4081 bins) with odd N; the largest plane that
fits in LDS (128 x 128) with K = 8 * 256 + 1; n_active = K; c = 1 with a tie bin far wider than the quota; 256 x 256, the widest plane
the model takes: pixel indices with the top bit of their uint16 set and the largest LDS request (130896 B), checked for content;
constant and two-level planes, where every cell ties and exactly the first n_active must fire across every wave's span -- also under
quotas that run past wave 0's first trip, past its span and into the third wave (H.LONG_QUOTA).

Beyond one launch and one trip: calls whose views cross the view bound of a launch (kMbSlabViews) and the byte bound (kMbStageBytes) --
training and scoring of planes, the activity call's per-slab copies, training from poses, the agent's step -- always two distinct views
repeated, so that the NumPy side stays two rows; k_mb_decide over more than 256 headings, with ties planted between its first and
second trip; two engines whose models need different amounts of LDS, used in turn."""
import ctypes

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import mushroom_familiarity, synth
from tests import helpers_infomax as HI
from tests import helpers_mushroom as H

pytestmark = pytest.mark.gpu

STATE, INVALID = -3, -1


@pytest.fixture(scope="module")
def eng():
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


def begin(e, d):
    e.mb_begin(d["h"], d["w"], d["conn"], d["n_active"], 2)


def describe(e, d, planes, mask, thr):
    """Why a comparison failed: is it the sum (threshold) or the selection (mask)?"""
    got_mask, got_thr = e.mb_activity_u8(planes)
    return "thresholds %s, masks %s (first differing patch %r)" % (
        "equal" if np.array_equal(got_thr, thr) else "differ: %r vs %r" % (got_thr[:8], thr[:8]),
        "equal" if np.array_equal(got_mask, mask) else "differ",
        int(np.argmax((got_mask != mask).any(axis=1))) if not np.array_equal(got_mask, mask) else None)


# ---- 1. selection and sum ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(H.CASES))
def test_fired_mask_threshold_and_scores(eng, key):
    d = H.case_data(key)
    begin(eng, d)
    mask, thr = eng.mb_activity_u8(d["patches"])
    assert mask.shape == (d["A"] + 1, d["K"]) and mask.dtype == np.uint8 and thr.dtype == np.int32
    assert np.array_equal(thr, d["thr"]), describe(eng, d, d["patches"], d["mask"], d["thr"])
    assert np.array_equal(mask, d["mask"]), describe(eng, d, d["patches"], d["mask"], d["thr"])
    # fresh weights: every firing cell counts
    fresh = eng.mb_score_u8(d["patches"])
    assert np.array_equal(H.bits(fresh), H.bits(np.full(d["A"] + 1, -float(d["n_active"]))))
    # the restatement's trained weights
    eng.mb_set_weights(d["wt"])
    fam = eng.mb_score_u8(d["patches"])
    assert fam.shape == (d["A"] + 1,) and fam.dtype == np.float64
    assert np.array_equal(H.bits(fam), H.bits(d["fam"])), (fam, d["fam"], describe(eng, d, d["patches"], d["mask"], d["thr"]))
    assert H.bits(fam[-1:])[0] == 0                                   # the trained view: +0.0, max_familiarity's bits
    # a patch scores the same alone as among the others
    alone = np.array([eng.mb_score_u8(p)[0] for p in d["patches"][:3]])
    assert np.array_equal(H.bits(alone), H.bits(fam[:3]))


@pytest.mark.parametrize("key", H.CONSTANT_KEYS)
def test_constant_and_two_level_planes(eng, key):
    d, k = H.case_data(key), H.constant_data(key)
    begin(eng, d)
    mask, thr = eng.mb_activity_u8(k["planes"])
    assert np.array_equal(thr, k["thr"]) and np.array_equal(mask, k["mask"])
    assert mask[0, :d["n_active"]].all() and not mask[0, d["n_active"]:].any()         # all 0: the cells 0 .. n_active-1
    assert mask[1, :d["n_active"]].all() and not mask[1, d["n_active"]:].any()         # all 255
    eng.mb_set_weights(d["wt"])
    assert np.array_equal(H.bits(eng.mb_score_u8(k["planes"])), H.bits(k["fam"]))


@pytest.mark.parametrize("n_active", H.LONG_QUOTA["n_active"])
def test_a_quota_that_runs_past_the_first_cells(eng, n_active):
    """Every cell ties and the quota is not used up inside wave 0's first trip: the wave's starting rank, the equals of its earlier
    trips and the ballot's lower lanes all decide (masks and fresh scores only: one such view would clear most of the weights)."""
    q = H.quota_data(n_active)
    eng.mb_begin(q["h"], q["w"], q["conn"], n_active, 2)
    mask, thr = eng.mb_activity_u8(q["planes"])
    assert np.array_equal(thr, q["thr"]), (thr, q["thr"])
    assert np.array_equal(mask, q["mask"]), [np.flatnonzero(m != w)[:8].tolist() for m, w in zip(mask, q["mask"])]
    for row in (0, 1):                                                   # all 0, all 255: the cells 0 .. n_active-1 and no others
        assert mask[row, :n_active].all() and not mask[row, n_active:].any()
    assert thr[0] == 0 and thr[1] == 255 * q["c"]
    assert np.array_equal(H.bits(eng.mb_score_u8(q["planes"])), H.bits(np.full(3, -float(n_active))))


# ---- 2. weights ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(H.CASES))
def test_weights_after_training(eng, key):
    d = H.case_data(key)
    begin(eng, d)
    info = eng.mb_info()
    assert info == dict(n_kc=d["K"], n_pixels=d["N"], fan_in=d["c"], n_active=d["n_active"], views_trained=0, n_depressed=0, bytes=d["K"])
    assert eng.mb_read_weights().tolist() == [1] * d["K"]
    eng.mb_train_u8(d["views"])
    wt = eng.mb_read_weights()
    assert wt.dtype == np.uint8 and np.array_equal(wt, d["wt"]), describe(eng, d, d["patches"], d["mask"], d["thr"])
    info = eng.mb_info()
    assert info["views_trained"] == d["F"] and info["n_depressed"] == int((d["wt"] == 0).sum())
    # every training view scores 0 on the device's own weights
    assert np.array_equal(H.bits(eng.mb_score_u8(d["views"])), H.bits(np.zeros(d["F"])))
    assert np.array_equal(H.bits(eng.mb_score_u8(d["patches"])), H.bits(d["fam"]))


# ---- 3. order-free training ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,cut", [("5x3_k37", 1), ("40x1_k300", 11), ("16x16_k1043", 5), ("7x5_k20000", 17), ("33x31_k4100_c16", 2)])
def test_training_has_no_order(eng, key, cut):
    d = H.case_data(key)
    v = d["views"]
    for name, calls in (("reversed", [v[::-1]]), ("cut", [v[:cut], v[cut:]]), ("cut, later part first", [v[cut:], v[:cut]]),
                        ("every view twice", [np.repeat(v, 2, axis=0)]), ("again", [v, v])):
        begin(eng, d)
        for part in calls:
            eng.mb_train_u8(np.ascontiguousarray(part))
        assert np.array_equal(eng.mb_read_weights(), d["wt"]), name
        assert eng.mb_info()["views_trained"] == sum(len(p) for p in calls), name


# ---- 4. more views than one launch takes -----------------------------------------------------------------------------------------
def test_training_across_the_slab():
    """kMbSlabViews copies of one view and then ONE other view: the second launch brings cells the first did not depress."""
    slab, stage = H.slab_views()
    d = H.case_data("5x3_k37")
    assert (slab + 1) * d["N"] <= stage                                  # the view count ends the slab at this shape
    two = HI.route_views(77, 2, d["h"], d["w"])
    views = np.ascontiguousarray(np.concatenate([np.repeat(two[:1], slab, axis=0), two[1:]]))
    ones = np.ones(d["K"], np.uint8)
    want = H.train(ones, two, d["conn"], d["n_active"])
    assert not np.array_equal(want, H.train(ones, two[:1], d["conn"], d["n_active"]))      # (the last view matters)
    e = navsim_amd.FamiliarityEngine(device=0)
    try:
        begin(e, d)
        e.mb_train_u8(views)
        assert np.array_equal(e.mb_read_weights(), want)
        assert e.mb_info()["views_trained"] == slab + 1 and e.mb_info()["n_depressed"] == int((want == 0).sum())
        # scoring crosses it too: the last patch is the other view
        fam = e.mb_score_u8(views)
        assert not fam.any() and fam.shape == (slab + 1,)
        e.mb_set_weights(H.train(ones, two[:1], d["conn"], d["n_active"]))
        fam = e.mb_score_u8(views)
        assert not fam[:slab].any() and fam[slab] == H.familiarity(e.mb_read_weights(), two[1:], d["conn"], d["n_active"])[0] < 0
    finally:
        e.close()


def test_training_and_scoring_across_the_byte_bound(eng):
    """128x128 planes: 64 MiB of them, not kMbSlabViews, end a launch.  `slab` copies of one view, then ONE other view."""
    views_bound, stage = H.slab_views()
    t = H.slab_train_data()
    slab = stage // t["N"]
    assert slab < views_bound and (slab + 1) * t["N"] > stage            # it is the bytes that end the slab
    views = np.ascontiguousarray(np.concatenate([np.repeat(t["two"][:1], slab, axis=0), t["two"][1:]]))
    assert not np.array_equal(t["both"], t["first"])                     # (the last view matters)
    eng.mb_begin(t["h"], t["w"], t["conn"], t["n_active"], 2)
    eng.mb_train_u8(views)
    assert np.array_equal(eng.mb_read_weights(), t["both"])
    assert eng.mb_info()["views_trained"] == slab + 1 and eng.mb_info()["n_depressed"] == int((t["both"] == 0).sum())
    fam = eng.mb_score_u8(views)
    assert fam.shape == (slab + 1,) and not H.bits(fam).any()            # every view trained: +0.0
    eng.mb_set_weights(t["first"])
    fam = eng.mb_score_u8(views)
    last = H.familiarity(t["first"], t["two"][1:], t["conn"], t["n_active"])
    assert last[0] < 0 and not H.bits(fam[:slab]).any() and H.bits(fam[slab:])[0] == H.bits(last)[0], (fam[slab - 2:], last)


def test_activity_across_the_byte_bound_and_its_optional_outputs(eng):
    """K = 20000: the fired masks (20000 bytes a view) end a launch of the activity call.  Copies of patch 0, then patch 1: the masks
    and thresholds of the second launch must land behind those of the first.  Then fired = NULL and threshold = NULL, one at a time."""
    views_bound, stage = H.slab_views()
    d = H.case_data(H.SLAB_ACTIVITY["key"])
    slab = stage // d["K"]
    assert slab < views_bound and slab < stage // d["N"]
    begin(eng, d)
    planes = np.ascontiguousarray(np.concatenate([np.repeat(d["patches"][:1], slab, axis=0), d["patches"][1:2]]))
    mask, thr = eng.mb_activity_u8(planes)
    assert mask.shape == (slab + 1, d["K"]) and thr.shape == (slab + 1,)
    assert not np.array_equal(d["mask"][0], d["mask"][1]) and d["thr"][0] != d["thr"][1]
    assert np.array_equal(thr[:slab], np.full(slab, d["thr"][0], np.int32)) and thr[slab] == d["thr"][1], (thr[:2], thr[slab - 2:])
    assert np.array_equal(mask[slab], d["mask"][1])
    assert np.array_equal(mask[slab - 1], d["mask"][0]) and np.array_equal(mask[0], d["mask"][0])
    assert (mask[:slab] == d["mask"][0]).all()
    # either output may be NULL
    three = np.ascontiguousarray(d["patches"][:3])
    full_mask, full_thr = eng.mb_activity_u8(three)
    assert np.array_equal(full_mask, d["mask"][:3]) and np.array_equal(full_thr, d["thr"][:3])
    only_thr = np.full(3, -7, dtype=np.int32)
    assert eng._lib.dv_mb_activity_u8(eng._ctx, N.u8ptr(three), 3, None, only_thr.ctypes.data_as(N._i32p)) == 0
    assert np.array_equal(only_thr, full_thr)
    only_mask = np.full((3, d["K"]), 7, dtype=np.uint8)
    assert eng._lib.dv_mb_activity_u8(eng._ctx, N.u8ptr(three), 3, N.u8ptr(only_mask), None) == 0
    assert np.array_equal(only_mask, full_mask)
    assert eng._lib.dv_mb_activity_u8(eng._ctx, N.u8ptr(three), 3, None, None) == 0
    # the engine goes on working
    eng.mb_set_weights(d["wt"])
    assert np.array_equal(H.bits(eng.mb_score_u8(d["patches"])), H.bits(d["fam"]))


# ---- 5. weights round trip -------------------------------------------------------------------------------------------------------
def test_set_weights_round_trip_and_a_second_engine(eng):
    d = H.case_data("16x16_k1043")
    begin(eng, d)
    eng.mb_train_u8(d["views"])
    wt = eng.mb_read_weights()
    fam = eng.mb_score_u8(d["patches"])
    eng.mb_set_weights(np.ones(d["K"], np.uint8))
    assert eng.mb_info()["n_depressed"] == 0
    eng.mb_set_weights(wt)
    assert np.array_equal(eng.mb_read_weights(), wt)
    with pytest.raises(ValueError, match="DV_ERR_INVALID"):
        eng.mb_set_weights(np.where(np.arange(d["K"]) == 700, 2, wt).astype(np.uint8))       # neither 0 nor 1
    assert np.array_equal(eng.mb_read_weights(), wt)
    other = navsim_amd.FamiliarityEngine(device=0)
    try:
        begin(other, d)
        other.mb_set_weights(wt)
        assert np.array_equal(H.bits(other.mb_score_u8(d["patches"])), H.bits(fam))
    finally:
        other.close()


def check_model(e, d):
    """The engine's model is `d`'s, trained: its weights, the scores and the activity of its patches are the restatement's."""
    assert np.array_equal(e.mb_read_weights(), d["wt"])
    assert np.array_equal(H.bits(e.mb_score_u8(d["patches"])), H.bits(d["fam"]))
    mask, thr = e.mb_activity_u8(d["patches"])
    assert np.array_equal(thr, d["thr"]) and np.array_equal(mask, d["mask"])


@pytest.mark.parametrize("key", ["33x31_k4100_c16", "256x256_k1043_c16"])
def test_two_engines_with_models_of_different_lds_size(key):
    """The cap on a kernel's dynamic LDS belongs to the function, not to an engine: the begin of a small model in one engine must not
    lower it under the launches of a model of more than 64 KB in another."""
    big, small = H.case_data(key), H.case_data("5x3_k37")
    a, b = navsim_amd.FamiliarityEngine(device=0), navsim_amd.FamiliarityEngine(device=0)
    try:
        begin(a, big)
        a.mb_train_u8(big["views"])
        begin(b, small)
        b.mb_train_u8(small["views"])
        check_model(b, small)
        check_model(a, big)
        check_model(b, small)
        assert np.array_equal(H.bits(a.mb_score_u8(big["views"])), H.bits(np.zeros(big["F"])))
    finally:
        a.close()
        b.close()


# ---- 6, 7. poses ---------------------------------------------------------------------------------------------------------------------
POSE_MODEL = dict(n_kc=4100, fan_in=10, sparsity=0.01, seed=41)


pose_headings = H.route_headings


@pytest.fixture(scope="module")
def sensed():
    """An agent with a 32x32 sensor on synth_landscape(3, 300, 4); its engine holds the landscape and the sensor."""
    model = mushroom_familiarity(**POSE_MODEL)
    agent = HI.sensed_agent(model, True)
    yield agent, model
    agent._engine.close()


def test_training_from_poses_is_training_on_its_own_views(sensed):
    agent, model = sensed
    e = agent._engine
    path = HI.sensed_route()
    x, y, ang = path[:, 0], path[:, 1], pose_headings(path)
    model.begin(e, 32, 32)
    views = e.mb_train_from_poses(x, y, ang)
    assert views.shape == (len(path), 32, 32, 3) and np.array_equal(views, e.sense(x, y, ang))
    wt = e.mb_read_weights()
    assert e.mb_info()["views_trained"] == len(path)
    planes = np.ascontiguousarray(views[..., 2])
    assert len(np.unique(planes)) > 1
    model.begin(e, 32, 32)
    e.mb_train_u8(planes)
    assert np.array_equal(e.mb_read_weights(), wt)
    conn = H.connectivity(4100, 1024, 10, POSE_MODEL["seed"])
    want = H.train(np.ones(4100, np.uint8), planes, conn, 41)
    assert 0 < (want == 0).sum() <= 2050 and np.array_equal(wt, want)
    # another channel is another plane
    mushroom_familiarity(channel=1, **POSE_MODEL).begin(e, 32, 32)
    e.mb_train_from_poses(x, y, ang, want_views=False)
    assert np.array_equal(e.mb_read_weights(), H.train(np.ones(4100, np.uint8), np.ascontiguousarray(views[..., 1]), conn, 41))


@pytest.mark.parametrize("n_headings", [9, 90])
def test_sense_step_is_score_on_the_sensed_planes(sensed, n_headings):
    agent, model = sensed
    e = agent._engine
    path = HI.sensed_route()
    model.begin(e, 32, 32)
    e.mb_train_from_poses(path[:, 0], path[:, 1], pose_headings(path), want_views=False)
    x, y = path[7] + np.array([0.6, -0.3])
    angles = (0.4 + np.linspace(-np.pi / 2, np.pi / 2, n_headings)) % (2 * np.pi)
    best, fam = e.mb_sense_step(x, y, angles)
    planes = np.ascontiguousarray(e.sense(np.full(n_headings, x), np.full(n_headings, y), angles)[..., 2])
    want = e.mb_score_u8(planes)
    assert np.array_equal(H.bits(fam), H.bits(want))
    assert best == int(np.argmax(want))                                   # integer scores tie: the first maximum
    assert len(np.unique(want)) > 1 and np.all(want <= 0)
    conn = H.connectivity(4100, 1024, 10, POSE_MODEL["seed"])
    assert np.array_equal(H.bits(want), H.bits(H.familiarity(e.mb_read_weights(), planes, conn, 41)))
    # every heading the same view: all scores tie and the first wins
    best, fam = e.mb_sense_step(x, y, np.full(n_headings, 0.4))
    assert best == 0 and len(np.unique(fam)) == 1


def v_planes(e, x, y, angles):
    angles = np.asarray(angles, dtype=np.float64)
    return np.ascontiguousarray(e.sense(np.full(len(angles), x), np.full(len(angles), y), angles)[..., 2])


def test_training_from_poses_across_the_view_bound(sensed):
    """kMbSlabViews copies of one pose and then ONE other pose: the second launch of dv_mb_train_from_poses reads behind the first's
    views and brings cells that the first did not depress."""
    e = sensed[0]._engine
    slab, _ = H.slab_views()
    m = H.SLAB_POSES
    conn = H.connectivity(m["K"], 1024, m["c"], m["seed"])
    ones = np.ones(m["K"], np.uint8)
    path = HI.sensed_route()
    p = path[list(m["poses"])]
    ang = pose_headings(path)[list(m["poses"])]
    two = np.ascontiguousarray(e.sense(p[:, 0], p[:, 1], ang)[..., 2])
    assert np.array_equal(two, H.host_sensed_planes(p[:, 0], p[:, 1], ang))
    want = H.train(ones, two, conn, m["n_active"])
    assert not np.array_equal(want, H.train(ones, two[:1], conn, m["n_active"]))        # (the last pose matters)
    e.mb_begin(32, 32, conn, m["n_active"], 2)
    rep = np.r_[np.zeros(slab, dtype=np.int64), 1]
    assert e.mb_train_from_poses(p[rep, 0], p[rep, 1], ang[rep], want_views=False) is None
    assert np.array_equal(e.mb_read_weights(), want)
    assert e.mb_info()["views_trained"] == slab + 1 and e.mb_info()["n_depressed"] == int((want == 0).sum())


def test_sense_step_across_the_view_bound(sensed):
    """kMbSlabViews copies of one heading and then ONE other: the second scoring launch writes its d behind the first's."""
    e = sensed[0]._engine
    slab, _ = H.slab_views()
    m = H.SLAB_POSES
    conn = H.connectivity(m["K"], 1024, m["c"], m["seed"])
    ones = np.ones(m["K"], np.uint8)
    x, y = H.step_xy()
    two = v_planes(e, x, y, m["angles"])
    assert np.array_equal(two, H.host_sensed_planes(x, y, m["angles"]))
    rep = np.r_[np.zeros(slab, dtype=np.int64), 1]
    angles = np.asarray(m["angles"])[rep]
    e.mb_begin(32, 32, conn, m["n_active"], 2)
    # trained on the LAST heading's view alone: it wins, at index kMbSlabViews
    wt = H.train(ones, two[1:], conn, m["n_active"])
    e.mb_set_weights(wt)
    best, fam = e.mb_sense_step(x, y, angles)
    want = H.familiarity(wt, two, conn, m["n_active"])[rep]
    assert fam.shape == (slab + 1,) and np.array_equal(H.bits(fam), H.bits(want)), (fam[:2], fam[slab - 2:], want[[0, -1]])
    assert H.bits(fam[-1:])[0] == 0 and fam[0] < 0 and len(np.unique(fam[:-1])) == 1
    assert best == slab
    # trained on the FIRST heading's view alone: heading 0 wins over its 8191 equals
    wt = H.train(ones, two[:1], conn, m["n_active"])
    e.mb_set_weights(wt)
    best, fam = e.mb_sense_step(x, y, angles)
    want = H.familiarity(wt, two, conn, m["n_active"])[rep]
    assert np.array_equal(H.bits(fam), H.bits(want)), (fam[:2], fam[slab - 2:], want[[0, -1]])
    assert best == 0 and fam[-1] < 0


def test_decide_beyond_its_first_trip(sensed):
    """k_mb_decide_batch (the step is an ensemble of one) strides 256 threads over the headings: 300 of them, then ties planted between a first-trip and a second-trip
    heading, inside one thread across trips, and a single maximum in the second trip."""
    agent, model = sensed
    e = agent._engine
    path = HI.sensed_route()
    model.begin(e, 32, 32)
    e.mb_train_from_poses(path[:, 0], path[:, 1], pose_headings(path), want_views=False)
    wt = e.mb_read_weights()
    conn = H.connectivity(4100, 1024, 10, POSE_MODEL["seed"])
    x, y = H.step_xy()

    def step(angles):
        best, fam = e.mb_sense_step(x, y, angles)
        want = H.familiarity(wt, v_planes(e, x, y, angles), conn, 41)
        assert np.array_equal(H.bits(fam), H.bits(want)), np.flatnonzero(fam != want)[:8]
        assert best == int(np.argmax(want)), (best, int(np.argmax(want)))
        return best, want

    angles = H.circle_angles(300)
    assert len(np.unique(angles)) == 300
    _, want = step(angles)
    assert want.max() > want.min() and np.all(want <= 0)
    b, m = angles[int(np.argmax(want))], angles[int(np.argmin(want))]
    for planted, winner in (((200, 257), 200), ((257,), 257), ((1, 257), 1), ((299, 257), 257)):
        arranged = np.where(want == want.max(), m, angles)
        arranged[list(planted)] = b
        best, got = step(arranged)
        assert np.flatnonzero(got == got.max()).tolist() == sorted(planted) and got.max() == want.max(), planted
        assert best == winner, (planted, best)


# ---- 8, 9. behind the agent ----------------------------------------------------------------------------------------------------------
SENSOR = (12, 10)                                                     # (w, h): N = 120
AGENT_MODEL = dict(n_kc=1043, fan_in=8, sparsity=0.02, seed=6)


def make_agent(model, gpu_sensor, n_test_angles=9):
    land = synth.synth_landscape(3, 300, 4)
    return navsim_amd.NavBySceneFamiliarity(land, SENSOR, 1.0, n_test_angles=n_test_angles, use_gpu_sensor=gpu_sensor,
                                            familiarity_model=model)


def route():
    return synth.sin_training_path(0.5, 60, 180, arclen=1.0)[:45]


def test_agent_trajectory_device_host_sensor_and_numpy_plug_in():
    path = route()
    model = mushroom_familiarity(**AGENT_MODEL)
    agents = [make_agent(model, True), make_agent(model, False), make_agent(H.numpy_model(**AGENT_MODEL), False)]
    try:
        for a in agents:
            a.train_from_path(path)
            a.position, a.angle = tuple(path[3] + np.array([0.7, -0.4])), 0.9
        assert agents[0]._familiarity_func.engine is agents[0]._engine              # the fused device step
        assert agents[1]._familiarity_func.metric == "mushroom" and agents[1]._engine is None
        assert not hasattr(agents[2]._familiarity_func, "engine")                   # the reference's loop over func
        assert agents[0].familiar_scenes.tobytes() == agents[2].familiar_scenes.tobytes()
        assert np.array_equal(agents[0]._engine.mb_read_weights(), agents[2]._familiarity_func.wt)
        assert np.array_equal(agents[1]._familiarity_func.engine.mb_read_weights(), agents[2]._familiarity_func.wt)
        seen = set()
        for step in range(40):
            for a in agents:
                a.step_forward(fake=True)
            a0 = agents[0]
            for a in agents[1:]:
                assert a.position == a0.position and a.angle == a0.angle, step
                assert np.array_equal(H.bits(a.angle_familiarity), H.bits(a0.angle_familiarity)), step
                assert np.array_equal(H.bits(a.scene_familiarity), H.bits(a0.scene_familiarity)), step
            assert a0.last_best_idex == int(np.argmax(a0.angle_familiarity))
            assert np.all(a0.angle_familiarity <= 0) and a0.step_familiarity == a0.angle_familiarity.max()
            assert a0.scene_familiarity.shape == (len(path),) and np.all(a0.scene_familiarity == a0.angle_familiarity.min())
            seen.update(a0.angle_familiarity.tolist())
        assert len(seen) > 3                                                         # (the walk met views of several novelties)
    finally:
        for a in agents[:2]:
            a.clear_training()


def test_additional_path_is_training_on_both_paths():
    path = route()
    more = route()[::-1][:20] + np.array([1.5, -2.0])
    model = mushroom_familiarity(**AGENT_MODEL)
    dev, host = make_agent(model, True), make_agent(model, False)
    try:
        for a in (dev, host):
            a.train_from_path(path)
        first = dev._engine.mb_read_weights()
        for a in (dev, host):
            a.train_additional_path(more)
        assert dev.familiar_scenes.tobytes() == host.familiar_scenes.tobytes() and len(dev.familiar_scenes) == 65
        conn = H.connectivity(1043, 120, 8, AGENT_MODEL["seed"])
        both = H.train(np.ones(1043, np.uint8), np.ascontiguousarray(dev.familiar_scenes[..., 2]), conn, 21)
        assert (both == 0).sum() > (first == 0).sum()                                # (the second path brought new cells)
        assert np.array_equal(dev._engine.mb_read_weights(), both)
        assert np.array_equal(host._familiarity_func.engine.mb_read_weights(), both)
        assert dev._engine.mb_info()["views_trained"] == 65
    finally:
        dev.clear_training()
        host.clear_training()


# ---- 10. errors --------------------------------------------------------------------------------------------------------------------
def test_every_call_before_begin_is_a_state_error():
    e = navsim_amd.FamiliarityEngine(device=0)
    try:
        lib, ctx = e._lib, e._ctx
        out, ang = np.zeros(2), np.zeros(2)
        planes = np.zeros((1, 3, 5), dtype=np.uint8)
        buf = np.zeros(64, dtype=np.uint8)
        thr = np.zeros(2, dtype=np.int32)
        best = ctypes.c_int32(0)
        assert lib.dv_mb_train_u8(ctx, N.u8ptr(planes), 1) == STATE
        assert lib.dv_mb_train_from_poses(ctx, N.f64ptr(out), N.f64ptr(out), N.f64ptr(ang), 2, None) == STATE
        assert lib.dv_mb_score_u8(ctx, N.u8ptr(planes), 1, N.f64ptr(out)) == STATE
        assert lib.dv_mb_activity_u8(ctx, N.u8ptr(planes), 1, N.u8ptr(buf), thr.ctypes.data_as(N._i32p)) == STATE
        assert lib.dv_mb_sense_step(ctx, 1.0, 1.0, N.f64ptr(ang), 2, N.f64ptr(out), ctypes.byref(best)) == STATE
        assert lib.dv_mb_read_weights(ctx, N.u8ptr(buf)) == STATE
        assert lib.dv_mb_set_weights(ctx, N.u8ptr(buf)) == STATE
        for call in (lambda: e.mb_score_u8(planes), lambda: e.mb_train_u8(planes), e.mb_read_weights, lambda: e.mb_activity_u8(planes)):
            with pytest.raises(navsim_amd.EngineError, match="DV_ERR_STATE"):
                call()
        assert e.mb_info() == dict(n_kc=0, n_pixels=0, fan_in=0, n_active=0, views_trained=0, n_depressed=0, bytes=0)
        e.mb_end()                                                                    # (harmless without a model)
        # ... and after end
        e.mb_begin(3, 5, H.connectivity(37, 15, 10, 1), 4)
        e.mb_end()
        assert lib.dv_mb_score_u8(ctx, N.u8ptr(planes), 1, N.f64ptr(out)) == STATE
    finally:
        e.close()


def test_begin_rejects_bad_arguments_one_by_one(eng):
    conn = H.connectivity(37, 15, 10, 1)
    good = dict(h=3, w=5, conn=conn, n_active=4, channel=2)
    eng.mb_begin(**good)
    for bad in (dict(channel=3), dict(channel=-1), dict(n_active=0), dict(n_active=38), dict(h=0), dict(w=0), dict(conn=conn[:, :0]),
                dict(conn=np.zeros((37, 17), np.int64)), dict(conn=conn[:0]), dict(h=257, w=256, conn=np.zeros((37, 10), np.int64)),
                dict(conn=np.where(np.arange(370).reshape(37, 10) == 369, 15, conn)),       # conn == N
                dict(conn=np.where(np.arange(370).reshape(37, 10) == 200, -1, conn)),       # conn < 0
                dict(h=2)):                                                                 # 10 pixels: conn reaches 14
        with pytest.raises(ValueError, match="DV_ERR_INVALID"):
            eng.mb_begin(**dict(good, **bad))
    assert eng._lib.dv_mb_begin(eng._ctx, 3, 5, 2, 37, 10, 4, None) == INVALID            # NULL conn
    # the model from before the refusals is still there; planes of another shape are refused
    assert eng.mb_info()["n_kc"] == 37
    with pytest.raises(ValueError):
        eng.mb_score_u8(np.zeros((2, 5, 3), dtype=np.uint8))
    # the limits themselves are taken: fan_in 16 and 65536 pixels
    eng.mb_begin(256, 256, np.full((5, 16), 65535), 5)
    assert eng.mb_activity_u8(np.zeros((1, 256, 256), np.uint8))[0].tolist() == [[1] * 5]


def test_sensor_of_another_shape_and_a_footprint_off_the_landscape():
    agent = make_agent(mushroom_familiarity(**AGENT_MODEL), True)
    try:
        e = agent._engine
        path = route()
        agent.train_from_path(path)
        wt = e.mb_read_weights()
        assert 0 < (wt == 0).sum() < 1043
        angles = (0.8 + np.pi / 2 + agent.angle_offsets) % (2 * np.pi)
        # a corner of the rotated footprint leaves the landscape: the reference's IndexError, and nothing is trained
        with pytest.raises(IndexError):
            e.mb_sense_step(297.5, 297.5, angles)
        with pytest.raises(IndexError):
            e.mb_train_from_poses(np.array([100.0, 297.5]), np.array([100.0, 297.5]), angles[:2])
        assert np.array_equal(e.mb_read_weights(), wt) and e.mb_info()["views_trained"] == len(path)
        best, fam = e.mb_sense_step(path[5][0], path[5][1], angles)                   # the engine goes on working
        assert 0 <= best < len(angles)
        # a model of another shape than the sensor's
        e.mb_begin(3, 5, H.connectivity(37, 15, 10, 1), 4)
        with pytest.raises(ValueError, match="the sensor is 12x10 but the model takes 5x3"):
            e.mb_sense_step(100.0, 100.0, angles)
        with pytest.raises(ValueError, match="the sensor is 12x10 but the model takes 5x3"):
            e.mb_train_from_poses(np.array([100.0]), np.array([100.0]), angles[:1])
        assert e.mb_info()["views_trained"] == 0
    finally:
        agent.clear_training()


def test_an_ensemble_of_mushroom_agents_is_refused():
    agent = make_agent(mushroom_familiarity(**AGENT_MODEL), True)
    try:
        agent.train_from_path(route())
        poses = [((100.0, 100.0), 0.3), ((110.0, 100.0), 0.4)]
        with pytest.raises(ValueError, match="NavEnsemble does not take a mushroom-body model"):
            navsim_amd.NavEnsemble.from_agent(agent, poses)
        with pytest.raises(ValueError, match="InfomaxEnsemble does not take a mushroom-body model"):
            navsim_amd.InfomaxEnsemble.from_agent(agent, poses)
    finally:
        agent.clear_training()
