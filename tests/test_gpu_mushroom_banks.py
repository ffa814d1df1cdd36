"""Memory banks of the mushroom-body model on the device (dv_mbank_*): several memories behind one connectivity, trained in shared
launches and scored member by member, against the NumPy statement (tests/helpers_mushroom.py through tests/helpers_mushroom_banks.py)
and against engines that hold one memory each -- bit for bit: every comparison is np.array_equal on integers or on the scores' uint64
views.  MushroomRouteEnsemble against lone agents, each trained on its own route alone on its own engine."""
import csv
import io

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import mushroom_familiarity, synth
from tests import helpers_infomax as HI
from tests import helpers_mushroom as H
from tests import helpers_mushroom_banks as HB
from tests import helpers_mushroom_ensemble as HE
from tests import helpers_sensed_models as HS

pytestmark = pytest.mark.gpu

STATE, INVALID, SENSE_ERROR = -3, -1, 16


@pytest.fixture(scope="module")
def eng():
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


def begin(e, d, wts=None, n_banks=HB.R):
    e.mb_begin(d["h"], d["w"], d["conn"], d["n_active"], 2)
    e.mbank_set(n_banks)
    if wts is not None:
        for r, w in enumerate(wts):
            e.mbank_set_weights(r, w)


def same(res, fam, best):
    assert res.angle_familiarity.shape == fam.shape and res.angle_familiarity.dtype == np.float64
    bad = np.argwhere(H.bits(res.angle_familiarity) != H.bits(fam))
    assert len(bad) == 0, (bad[:6].tolist(), res.angle_familiarity[tuple(bad[0])], fam[tuple(bad[0])])
    assert res.best_idex.tolist() == np.asarray(best).tolist()


# ---- 1. training and scoring against the statement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", HB.KEYS)
def test_training_and_scoring_are_the_statement_bank_by_bank(eng, key):
    b = HB.bank_data(key)
    begin(eng, b)
    assert eng.mbank_info()["n_banks"] == HB.R and np.array_equal(eng.mbank_read_weights(), np.ones((HB.R, b["K"]), np.uint8))
    eng.mbank_train_u8(b["views"], b["bank_of"])
    got = eng.mbank_read_weights()
    assert got.shape == (HB.R, b["K"]) and got.dtype == np.uint8
    for r in range(HB.R):
        assert np.array_equal(got[r], b["wts"][r]), (r, np.flatnonzero(got[r] != b["wts"][r])[:8])
        assert np.array_equal(eng.mbank_read_weights(r), b["wts"][r])
    info = eng.mbank_info()
    assert info["views_trained"].tolist() == b["counts"].tolist() and info["n_depressed"].tolist() == b["zeros"].tolist()
    assert eng.mb_info()["views_trained"] == b["counts"][0] and eng.mb_info()["n_depressed"] == b["zeros"][0]      # bank 0
    for n, A in HB.LAYOUTS:
        d = HB.layout_data(key, n, A)
        res = eng.mbank_step_batch_u8(d["planes"], d["banks"])
        assert not res.flags.any()
        same(res, d["fam"], d["best"])
    # training again changes nothing (it has no order and is idempotent), whatever the order of the views
    order = np.random.default_rng(5).permutation(len(b["views"]))
    eng.mbank_train_u8(np.ascontiguousarray(b["views"][order]), b["bank_of"][order])
    assert np.array_equal(eng.mbank_read_weights(), b["wts"])
    assert eng.mbank_info()["views_trained"].tolist() == (2 * b["counts"]).tolist()


def test_the_devices_bank_table_follows_the_calls(eng):
    """The device holds ONE bank table, for views and for members alike, and the host sends it only when its content changes.  The
    smallest case (3 x 5 views, 37 cells), 4 members x 2 headings: a first table, the same again (nothing sent), another of the same
    length, a training call whose bank_of_view equals it (the members' table serves the views), the step after it, five members (the
    buffer grows), and back to the first table.  Every step is the statement under the weights as trained so far."""
    b = HB.bank_data("5x3_k37")
    h, w, args = b["h"], b["w"], (b["conn"], b["n_active"])
    first, more = HI.route_views(141, 3, h, w), HI.route_views(142, 4, h, w)
    planes = HI.route_views(143, 10, h, w).reshape(5, 2, h, w).copy()
    planes[:3, 0], planes[3, 1], planes[4, 0] = first, more[1], more[3]                  # what some bank was trained on, beside what none was
    T1, T2, T5 = np.array([0, 1, 2, 1], np.int32), np.array([2, 0, 1, 0], np.int32), np.array([1, 2, 0, 2, 1], np.int32)

    def want(wts, table):
        return np.stack([H.familiarity(wts[r], planes[i], *args) for i, r in enumerate(table)])

    w0 = HB.train_banks(first, [0, 1, 2], *args, b["K"])
    w1 = np.stack([H.train(w0[r], more[T2 == r], *args) for r in range(HB.R)])
    assert (w1 != w0).any(axis=1).all()                                                  # the training call shows in every bank
    rows = [want(w0, T1), want(w0, T2), want(w1, T2), want(w1, T1)]
    assert all(not np.array_equal(rows[a], rows[c]) for a in range(4) for c in range(a + 1, 4))     # so does a stale table, or a stale bank

    def step(table, wts):
        res = eng.mbank_step_batch_u8(planes[:len(table)], table)
        same(res, want(wts, table), np.argmax(want(wts, table), axis=1))

    begin(eng, b, w0)                                                                    # (mb_begin: the device's table is gone)
    step(T1, w0)
    step(T1.copy(), w0)
    step(T2, w0)
    eng.mbank_train_u8(more, T2.copy())
    assert np.array_equal(eng.mbank_read_weights(), w1)
    step(T2, w1)
    step(T5, w1)
    step(T1, w1)


# ---- 2. isolation ----------------------------------------------------------------------------------------------------------------------------
def test_banks_do_not_touch_one_another(eng):
    b = HB.bank_data("16x16_k1043")
    ones = np.ones(b["K"], np.uint8)
    begin(eng, b)
    eng.mbank_train_u8(b["views"], np.ones(len(b["views"]), dtype=np.int32))             # bank 1 alone
    got = eng.mbank_read_weights()
    assert np.array_equal(got[0], ones) and np.array_equal(got[2], ones) and np.array_equal(got[1], b["wt"])
    assert eng.mbank_info()["views_trained"].tolist() == [0, b["F"], 0]
    # the single model's calls work on bank 0 and on nothing else
    patches = b["patches"]
    assert np.array_equal(eng.mb_score_u8(patches), -np.full(len(patches), float(b["n_active"])))         # bank 0 is fresh: d = n_active
    mine = b["views"][b["bank_of"] == 0]
    eng.mb_train_u8(mine)
    got = eng.mbank_read_weights()
    assert np.array_equal(got[0], b["wts"][0]) and np.array_equal(got[1], b["wt"]) and np.array_equal(got[2], ones)
    assert np.array_equal(eng.mb_read_weights(), b["wts"][0])
    assert np.array_equal(H.bits(eng.mb_score_u8(patches)), H.bits((-b["nov"][0]).astype(np.float64)))
    assert eng.mbank_info()["views_trained"].tolist() == [len(mine), b["F"], 0]
    # set_weights of one bank round-trips and changes that row only
    before = eng.mbank_read_weights()
    eng.mbank_set_weights(2, b["wts"][2])
    after = eng.mbank_read_weights()
    assert np.array_equal(after[2], b["wts"][2]) and np.array_equal(after[:2], before[:2])
    with pytest.raises(ValueError, match="DV_ERR_INVALID"):
        eng.mbank_set_weights(1, np.full(b["K"], 2, np.uint8))
    assert np.array_equal(eng.mbank_read_weights(), after)
    # mb_begin after mbank_set is one bank again
    eng.mb_begin(b["h"], b["w"], b["conn"], b["n_active"], 2)
    info = eng.mbank_info()
    assert info["n_banks"] == 1 and info["views_trained"].tolist() == [0] and info["n_depressed"].tolist() == [0]
    assert eng.mbank_read_weights().shape == (1, b["K"])
    assert eng._lib.dv_mbank_read_weights(eng._ctx, 1, N.u8ptr(np.empty(b["K"], np.uint8))) == INVALID


def test_the_sensed_single_calls_use_bank_zero(sensed):
    e = sensed
    conn, n_active, wts, _ = HB.sensed_banks("c10")
    begin(e, dict(h=32, w=32, conn=conn, n_active=n_active), wts)
    xs, ys, centre = HE.sensed_poses(9)
    angs = (centre[:, None] + np.linspace(-np.pi / 2, np.pi / 2, 9)[None, :]) % (2 * np.pi)
    want = HB.sensed_statement("c10", xs, ys, angs, [0] * 5)
    same(e.mb_sense_step_batch(xs, ys, angs), want, np.argmax(want, axis=1))              # dv_batch_mb_sense_step
    assert not np.array_equal(want, HB.sensed_statement("c10", xs, ys, angs, [1] * 5))
    assert np.array_equal(e.mbank_read_weights(), wts)


# ---- 3. equivalence with engines of one memory each ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sensed():
    """An agent with a 32x32 sensor on synth_landscape(3, 300, 4); its engine holds the landscape and the sensor."""
    agent = HI.sensed_agent(mushroom_familiarity(**HE.SENSED_MODELS["c10"]), True)
    yield agent._engine
    agent._engine.close()


def test_one_banked_engine_equals_an_engine_per_route(sensed):
    conn, n_active, _ = HE.sensed_model("c10")
    paths = HB.routes()
    heads = [H.route_headings(p) for p in paths]
    xs, ys, centre = HE.sensed_poses(9)
    angs = (centre[:, None] + np.linspace(-np.pi / 2, np.pi / 2, 9)[None, :]) % (2 * np.pi)
    lone_w, lone_views, lone_fam = [], [], []
    for p, hd in zip(paths, heads):
        a = HI.sensed_agent(mushroom_familiarity(**HE.SENSED_MODELS["c10"]), True)
        try:
            a._engine.mb_begin(32, 32, conn, n_active, 2)
            lone_views.append(a._engine.mb_train_from_poses(p[:, 0], p[:, 1], hd))
            lone_w.append(a._engine.mb_read_weights())
            lone_fam.append(a._engine.mb_sense_step_batch(xs, ys, angs).angle_familiarity)
        finally:
            a._engine.close()
    assert all((lone_w[a] != lone_w[b]).any() for a in range(3) for b in range(a + 1, 3))
    e = sensed
    begin(e, dict(h=32, w=32, conn=conn, n_active=n_active))
    pts = np.concatenate(paths)
    bank_of = np.repeat(np.arange(3, dtype=np.int32), [len(p) for p in paths])
    views = e.mbank_train_from_poses(pts[:, 0], pts[:, 1], np.concatenate(heads), bank_of)
    assert np.array_equal(views, np.concatenate(lone_views))
    assert np.array_equal(e.mbank_read_weights(), np.stack(lone_w))
    assert e.mbank_info()["views_trained"].tolist() == [len(p) for p in paths]
    # (tables of one length in turn, one of them twice running: the library sends a table only when it differs from the device's)
    for banks in ([0, 1, 2, 1, 0], [0, 1, 2, 1, 0], [2, 2, 0, 1, 1], [0, 1, 2, 1, 0]):
        res = e.mbank_sense_step_batch(xs, ys, angs, banks)
        want = np.stack([lone_fam[r][i] for i, r in enumerate(banks)])
        same(res, want, np.argmax(want, axis=1))
    assert not np.array_equal(lone_fam[0], lone_fam[1]) and not np.array_equal(lone_fam[1], lone_fam[2])


# ---- 4. both bounds of a launch ------------------------------------------------------------------------------------------------------------
def test_views_and_columns_past_the_view_bound(eng):
    v = HB.view_bound_data()
    begin(eng, v)
    eng.mbank_train_u8(v["two"][v["pick"]], v["bank_of"])                                # 8193 views: view 8192 is bank 2's
    assert np.array_equal(eng.mbank_read_weights(), v["wts"])
    assert eng.mbank_info()["views_trained"].tolist() == [2731, 2731, 2731]
    res = eng.mbank_step_batch_u8(v["two"][v["step_pick"]], v["step_banks"])             # 8193 columns: column 8192 is bank 2's
    same(res, v["fam"], v["best"])


def test_planes_past_the_byte_bound(eng):
    b = HB.byte_bound_data()
    begin(eng, b)
    eng.mbank_train_u8(b["two"][b["pick"]], b["bank_of"])                                # 4097 planes of 128x128
    assert np.array_equal(eng.mbank_read_weights(), b["wts"])
    res = eng.mbank_step_batch_u8(b["two"][b["step_pick"]], b["step_banks"])
    same(res, b["fam"], b["best"])


def slab_pose_banks():
    """Two banks for H.SLAB_POSES' model: fresh, and trained on the second heading's view alone."""
    m = H.SLAB_POSES
    conn = H.connectivity(m["K"], 1024, m["c"], m["seed"])
    x, y = H.step_xy()
    two = H.host_sensed_planes(x, y, m["angles"])
    ones = np.ones(m["K"], np.uint8)
    return dict(conn=conn, n_active=m["n_active"], h=32, w=32), np.stack([ones, H.train(ones, two[1:], conn, m["n_active"])])


def test_sensed_columns_past_the_view_bound(sensed):
    """3 members x 2731 headings: the pose index crosses the launch bound inside member 2, whose bank is not member 0's.  Each member's
    row is a lone mb_sense_step's on an engine whose one memory holds the member's bank."""
    e = sensed
    model, wts = slab_pose_banks()
    x, y = H.step_xy()
    n, A = HE.SLAB_MEMBERS, HE.SLAB_HEADINGS
    xs, ys = x + np.array([0.0, 0.7, -0.5]), y + np.array([0.0, -0.4, 0.6])
    angs = np.stack([(shift + H.circle_angles(A)) % (2 * np.pi) for shift in (0.0, 0.01, 0.02)])
    banks = [0, 1, 1]
    lone = []
    e.mb_begin(32, 32, model["conn"], model["n_active"], 2)
    for i in range(n):
        e.mb_set_weights(wts[banks[i]])
        lone.append(e.mb_sense_step(xs[i], ys[i], angs[i]))
    other = e.mb_sense_step(xs[2], ys[2], angs[2])[1]                                    # (member 2 under bank 1, from the loop's end) ...
    e.mb_set_weights(wts[0])
    assert not np.array_equal(e.mb_sense_step(xs[2], ys[2], angs[2])[1], other)          # ... is not member 2 under bank 0
    begin(e, model, wts, n_banks=2)
    res = e.mbank_sense_step_batch(xs, ys, angs, banks)
    assert res.angle_familiarity.shape == (n, A) and not res.flags.any()
    for i, (best, fam) in enumerate(lone):
        assert np.array_equal(H.bits(res.angle_familiarity[i]), H.bits(fam)), i
        assert res.best_idex[i] == best, i


# ---- 5. more than 256 headings -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", HB.KEYS)
def test_members_of_260_headings_in_different_banks(eng, key):
    n, A = HB.TIE_LAYOUT
    d = HB.layout_data(key, n, A)
    begin(eng, d, d["wts"])
    res = eng.mbank_step_batch_u8(d["planes"], d["banks"])
    same(res, d["fam"], d["best"])
    assert res.best_idex[1] == 5 and H.bits(res.angle_familiarity[1, [5, 257]]).tolist() == [0, 0]       # the first of two equal +0.0


# ---- 6. LDS above 64 KB through the banked kernels -----------------------------------------------------------------------------------------
def test_the_widest_plane_through_the_banked_kernels(eng):
    n, A = HB.WIDE_LAYOUT
    d = HB.layout_data(HB.WIDE_KEY, n, A)                                                # 256x256, c = 16: 130 896 bytes of LDS
    begin(eng, d)
    eng.mbank_train_u8(d["views"], d["bank_of"])
    assert np.array_equal(eng.mbank_read_weights(), d["wts"])
    same(eng.mbank_step_batch_u8(d["planes"], d["banks"]), d["fam"], d["best"])


def _sensed_c16(e):
    conn, n_active, wts, bank_of = HB.sensed_banks("c16")                                # fan-in 16 on 32x32: 66 384 bytes of LDS
    begin(e, dict(h=32, w=32, conn=conn, n_active=n_active))
    path = HI.sensed_route()
    e.mbank_train_from_poses(path[:, 0], path[:, 1], H.route_headings(path), bank_of, want_views=False)
    assert np.array_equal(e.mbank_read_weights(), wts)


def test_a_sensed_model_above_64_kb_and_two_engines_in_turn(sensed):
    e1 = sensed
    _sensed_c16(e1)
    A = 9
    xs, ys, centre = HE.sensed_poses(A)
    angs = (centre[:, None] + np.linspace(-np.pi / 2, np.pi / 2, A)[None, :]) % (2 * np.pi)
    banks = np.array([2, 0, 1, 1, 0], dtype=np.int32)
    want1 = HB.sensed_statement("c16", xs, ys, angs, banks)
    same(e1.mbank_sense_step_batch(xs, ys, angs, banks), want1, np.argmax(want1, axis=1))
    assert not np.array_equal(want1, HB.sensed_statement("c16", xs, ys, angs, [0] * 5))
    # a second engine whose model is far smaller, used in turn with the first
    a2 = HI.sensed_agent(mushroom_familiarity(**HE.SENSED_MODELS["c10"]), True)
    e2 = a2._engine
    try:
        model, wts = slab_pose_banks()
        begin(e2, model, wts, n_banks=2)
        banks2 = [1, 0, 0, 1, 1]
        planes = H.host_sensed_planes(np.repeat(xs, A), np.repeat(ys, A), angs.reshape(-1)).reshape(5, A, 32, 32)
        want2 = np.stack([(-HE.novelty(wts[banks2[i]], planes[i], model["conn"], model["n_active"])).astype(np.float64) for i in range(5)])
        for _ in range(2):
            same(e1.mbank_sense_step_batch(xs, ys, angs, banks), want1, np.argmax(want1, axis=1))
            same(e2.mbank_sense_step_batch(xs, ys, angs, banks2), want2, np.argmax(want2, axis=1))
            same(e1.mbank_step_batch_u8(planes, banks), want1, np.argmax(want1, axis=1))
            same(e2.mbank_step_batch_u8(planes, banks2), want2, np.argmax(want2, axis=1))
    finally:
        e2.close()


# ---- 7. flags ----------------------------------------------------------------------------------------------------------------------------------
def test_a_member_off_the_landscape_is_flagged_and_the_others_keep_their_banks(sensed):
    e = sensed
    conn, n_active, wts, _ = HB.sensed_banks("c10")
    begin(e, dict(h=32, w=32, conn=conn, n_active=n_active), wts)
    HS.flag_facts("sq")
    x, y = HS.FLAG_AT["sq"]
    A = 9
    xs, ys, centre = HE.sensed_poses(A)
    angs = (centre[:, None] + np.linspace(-np.pi / 2, np.pi / 2, A)[None, :]) % (2 * np.pi)
    banks = np.array([2, 0, 1, 1, 0], dtype=np.int32)
    clean = e.mbank_sense_step_batch(xs, ys, angs, banks)
    want = HB.sensed_statement("c10", xs, ys, angs, banks)
    same(clean, want, np.argmax(want, axis=1))
    xs2, ys2, angs2 = xs.copy(), ys.copy(), angs.copy()
    xs2[2], ys2[2] = x, y
    angs2[2] = HS.safe_angles(A, 100)
    angs2[2, 3] = np.deg2rad(HS.OFF_DEG[0])                                              # one corner leaves the landscape
    assert HS.is_off("sq", x, y, angs2[2, 3]) and not any(HS.is_off("sq", x, y, a) for a in np.delete(angs2[2], 3))
    with pytest.raises(IndexError):
        HS.host_scenes("sq", x, y, angs2[2, 3])
    res = e.mbank_sense_step_batch(xs2, ys2, angs2, banks)
    assert res.flags.tolist() == [0, 0, SENSE_ERROR, 0, 0] and res.best_idex[2] == -1
    for i in (0, 1, 3, 4):
        assert np.array_equal(H.bits(res.angle_familiarity[i]), H.bits(want[i])), i
        assert res.best_idex[i] == int(np.argmax(want[i])), i
    same(e.mbank_sense_step_batch(xs, ys, angs, banks), want, np.argmax(want, axis=1))  # ... and the next call without it is as before


# ---- 8. refusals on the device side ----------------------------------------------------------------------------------------------------------
def test_a_bank_out_of_range_is_refused_and_nothing_changes(eng):
    v = HB.view_bound_data()
    begin(eng, v, v["wts"])
    before = eng.mbank_read_weights()
    views, _ = H.slab_views()
    planes = v["two"][v["pick"]]
    lib, ctx = eng._lib, eng._ctx
    fam, best = np.zeros(v["step_pick"].size), np.zeros(3, dtype=np.int32)
    step_planes = np.ascontiguousarray(v["two"][v["step_pick"]])
    for bad in (HB.R, -1):
        for at in (0, 100, views):                                                       # (views: beyond the first launch)
            table = v["bank_of"].copy()
            table[at] = bad
            assert lib.dv_mbank_train_u8(ctx, N.u8ptr(planes), len(planes), table.ctypes.data_as(N._i32p)) == INVALID
            assert ("bank_of_view[%d] = %d" % (at, bad)) in lib.dv_last_error(ctx).decode()
        for at in (0, 2):
            table = v["step_banks"].copy()
            table[at] = bad
            assert lib.dv_mbank_step_u8(ctx, N.u8ptr(step_planes), 3, HE.SLAB_HEADINGS, table.ctypes.data_as(N._i32p), N.f64ptr(fam),
                                        best.ctypes.data_as(N._i32p)) == INVALID
            assert ("bank_of_member[%d] = %d" % (at, bad)) in lib.dv_last_error(ctx).decode()
    assert lib.dv_mbank_train_u8(ctx, N.u8ptr(planes), len(planes), None) == INVALID
    assert lib.dv_mbank_set(ctx, 0) == INVALID and lib.dv_mbank_read_weights(ctx, HB.R, N.u8ptr(np.empty(v["K"], np.uint8))) == INVALID
    assert np.array_equal(eng.mbank_read_weights(), before) and eng.mbank_info()["views_trained"].tolist() == [0, 0, 0]
    # the engine's own check is the same refusal, before the library; a table the engine cannot know to be stale reaches the library's
    with pytest.raises(ValueError, match="bank_of_view"):
        eng.mbank_train_u8(planes[:4], [0, 1, 2, 3])
    eng.mb_banks = 4                                                                     # (what the engine believes; the library holds 3)
    try:
        with pytest.raises(ValueError, match="DV_ERR_INVALID"):
            eng.mbank_train_u8(planes[:4], [0, 1, 2, 3])
    finally:
        eng.mb_banks = HB.R
    assert np.array_equal(eng.mbank_read_weights(), before)
    same(eng.mbank_step_batch_u8(step_planes, v["step_banks"]), v["fam"], v["best"])


def test_mbank_calls_without_a_model_are_state_errors():
    e = navsim_amd.FamiliarityEngine(device=0)
    try:
        t = np.zeros(2, dtype=np.int32)
        planes, fam, best, flags = np.zeros((2, 3, 5), np.uint8), np.zeros(2), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.uint32)
        tp, bp = t.ctypes.data_as(N._i32p), best.ctypes.data_as(N._i32p)
        lib, ctx = e._lib, e._ctx
        assert lib.dv_mbank_set(ctx, 2) == STATE
        assert lib.dv_mbank_train_u8(ctx, N.u8ptr(planes), 2, tp) == STATE
        assert lib.dv_mbank_train_from_poses(ctx, N.f64ptr(fam), N.f64ptr(fam), N.f64ptr(fam), 2, tp, None) == STATE
        assert lib.dv_mbank_step_u8(ctx, N.u8ptr(planes), 2, 1, tp, N.f64ptr(fam), bp) == STATE
        assert lib.dv_mbank_sense_step(ctx, N.f64ptr(fam), N.f64ptr(fam), N.f64ptr(fam), 2, 1, tp, N.f64ptr(fam), bp,
                                       flags.ctypes.data_as(N._u32p)) == STATE
        assert lib.dv_mbank_read_weights(ctx, 0, N.u8ptr(planes)) == STATE and lib.dv_mbank_set_weights(ctx, 0, N.u8ptr(planes)) == STATE
        info = e.mbank_info()
        assert info["n_banks"] == 1 and info["views_trained"].tolist() == [0] and info["n_depressed"].tolist() == [0]
        e.mb_begin(3, 5, H.connectivity(37, 15, 10, 1), 4)
        e.mbank_set(2)
        assert lib.dv_mbank_sense_step(ctx, N.f64ptr(fam), N.f64ptr(fam), N.f64ptr(fam), 2, 1, tp, N.f64ptr(fam), bp,
                                       flags.ctypes.data_as(N._u32p)) == STATE            # a model but no sensor
        e.mb_end()
        assert e.mbank_info()["n_banks"] == 1 and lib.dv_mbank_set(ctx, 2) == STATE
    finally:
        e.close()


# ---- 9. the ensemble ---------------------------------------------------------------------------------------------------------------------------
SENSOR = (12, 10)
AGENT_MODEL = dict(n_kc=1043, fan_in=8, sparsity=0.02, seed=6)


def make_agent():
    return navsim_amd.NavBySceneFamiliarity(synth.synth_landscape(3, 300, 4), SENSOR, 1.0, n_test_angles=9, use_gpu_sensor=True,
                                            familiarity_model=mushroom_familiarity(**AGENT_MODEL))


def _lone(paths, starts):
    out = []
    for r, pos, ang in starts:
        a = make_agent()
        a.train_from_path(paths[r])
        a.position, a.angle = pos, ang
        out.append(a)
    return out


def test_route_ensemble_members_equal_lone_agents_trained_on_their_own_routes():
    paths = HB.routes()
    starts = HB.starts(paths)
    ens = navsim_amd.MushroomRouteEnsemble.from_routes(make_agent(), paths, starts)
    alone = _lone(paths, starts)
    calls = []
    inner = ens.engine.mbank_sense_step_batch

    def counted(*a, **k):
        calls.append(list(a[3]))
        return inner(*a, **k)
    ens.engine.mbank_sense_step_batch = counted
    try:
        assert len(ens.agents) == 6 and [a.memory_bank for a in ens.agents] == [0, 0, 1, 1, 2, 2]
        info = ens.bank_info()
        assert info["n_banks"] == 3 and info["views_trained"].tolist() == [len(p) for p in paths]
        for r in range(3):
            one = alone[2 * r]._engine.mb_info()
            assert (info["views_trained"][r], info["n_depressed"][r]) == (one["views_trained"], one["n_depressed"]), r
            assert np.array_equal(ens.engine.mbank_read_weights(r), alone[2 * r]._engine.mb_read_weights()), r
        for m, a in zip(ens.agents, alone):
            assert m._metric_slot is None and not m._metrics_on_device                   # the host's metrics
            assert np.array_equal(m.training_path, a.training_path) and m.training_path_length == a.training_path_length
            assert np.array_equal(m.familiar_scenes, a.familiar_scenes) and np.array_equal(m.scene_familiarity, a.scene_familiarity)
        with pytest.raises(ValueError, match="MushroomRouteEnsemble"):
            ens.agents[1].step_forward()
        seen = set()
        for t in range(15):
            before = list(ens.active)
            ens.step_forward()
            assert len(calls) == t + 1 and calls[-1] == [ens.agents[i].memory_bank for i in before]       # ONE device call a step
            for a in alone:
                if a.stopped_with_exception is None:
                    try:
                        a.step_forward()
                    except navsim_amd.StopNavigationException as stop:
                        a.stopped_with_exception = stop
            for i, (m, a) in enumerate(zip(ens.agents, alone)):
                assert m.position == a.position and m.angle == a.angle, (t, i)
                assert np.array_equal(H.bits(m.angle_familiarity), H.bits(a.angle_familiarity)), (t, i)
                assert np.array_equal(H.bits(m.scene_familiarity), H.bits(a.scene_familiarity)), (t, i)
                code = a.stopped_with_exception.get_code() if a.stopped_with_exception is not None else 0
                assert ens.stop_status[i] == code, (t, i)
                assert m.navigation_error == a.navigation_error and m.percent_recapitulated == a.percent_recapitulated, (t, i)
                seen.update(m.angle_familiarity.tolist())
        assert len(seen) > 3 and max(seen) == 0.0
    finally:
        ens.engine.mbank_sense_step_batch = inner
        ens.agents[0].clear_training()
        for a in alone:
            a.clear_training()


def _csv(rows):
    out = io.StringIO()
    w = csv.DictWriter(out, fieldnames=sorted(rows[0]))
    w.writeheader()
    w.writerows(rows)
    return out.getvalue()


def test_run_ensemble_rows_equal_lone_run_experiment_rows():
    paths = HB.routes()
    starts = HB.starts(paths)
    ens = navsim_amd.MushroomRouteEnsemble.from_routes(make_agent(), paths, starts)
    try:
        rows = navsim_amd.run_ensemble(ens)                                              # every member its own route's frames
    finally:
        ens.agents[0].clear_training()
    wants = []
    for a in _lone(paths, starts):
        try:
            wants.append(navsim_amd.run_experiment(a))
        finally:
            a.clear_training()
    assert _csv(rows) == _csv(wants)
    # a member that ran out of frames did so at ITS route's count, and the three routes' counts differ
    budget = [int(navsim_amd.experiment.FRAME_FACTOR * np.sum(np.linalg.norm(paths[r][1:] - paths[r][:-1], axis=1)) / 1.0) for r, _, _ in starts]
    assert len(set(budget)) == 3
    for row, frames in zip(rows, budget):
        assert row["completed_frames"] == frames if row["stop_status"] == 0 else row["completed_frames"] < frames, (row, frames)
