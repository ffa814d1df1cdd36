"""Weight banks of the Infomax model on the device (dv_ibank_*): several models of one shape in one context, their training chains
advanced in lockstep and their members scored in one call.  Device against device bit for bit -- every bank against an engine that holds
that bank's model alone (np.array_equal on the uint64 views) -- and against the NumPy statement (tests/helpers_infomax.py through
tests/helpers_infomax_banks.py) within H.TOL, the figure printed before it is asserted.  InfomaxRouteEnsemble against lone agents, each
trained on its own route alone on its own engine."""
import csv
import io

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import infomax_familiarity, synth
from tests import helpers_infomax as H
from tests import helpers_infomax_banks as HB
from tests import helpers_mushroom_ensemble as HE
from tests import helpers_sensed_models as HS

pytestmark = pytest.mark.gpu

STATE, INVALID, SENSE_ERROR = -3, -1, 16


@pytest.fixture(scope="module")
def eng():
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def lone():
    """The engine that holds one bank's model alone."""
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


def begin(e, d, n_banks=HB.R, eta=H.ETA, weights=None):
    e.infomax_begin(d["h"], d["w"], d["W0"], 2, eta)
    e.ibank_set(n_banks, d["W0"])
    if weights is not None:
        for r, W in enumerate(weights):
            e.ibank_set_weights(r, W)


def lone_chain(e, d, views, eta=H.ETA):
    """The weights of a model that trains on `views` alone from d's W0."""
    e.infomax_begin(d["h"], d["w"], d["W0"], 2, eta)
    if len(views):
        e.infomax_train_u8(views)
    return e.infomax_read_weights()


def same_bits(a, b, what=None):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.argwhere(H.bits(a) != H.bits(b))
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist())


# ---- 1. training ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", HB.KEYS)
def test_every_bank_trains_as_its_chain_alone(eng, lone, key):
    b = HB.bank_data(key)
    begin(eng, b)
    info = eng.ibank_info()
    assert info["n_banks"] == HB.R and info["views_trained"].tolist() == [0] * HB.R and info["finite"].tolist() == [True] * HB.R
    eng.ibank_train_u8(b["views"], b["bank_of"])
    got = [eng.ibank_read_weights(r) for r in range(HB.R)]
    worst = 0.0
    for r in range(HB.R):
        same_bits(got[r], lone_chain(lone, b, b["views"][b["bank_of"] == r]), (key, r))
        worst = max(worst, float(np.max(np.abs(got[r] - b["Ws"][r])) / np.max(np.abs(b["Ws"][r]))))
        if b["counts"][r] == 0:
            same_bits(got[r], b["W0"], (key, r, "the empty bank"))
    print("infomax banks, weights %s: relative error %.3e (bound %.1e)" % (key, worst, H.TOL))
    assert worst <= H.TOL
    info = eng.ibank_info()
    assert info["views_trained"].tolist() == b["counts"].tolist() and info["finite"].tolist() == [True] * HB.R
    assert eng.infomax_info()["views_trained"] == b["counts"][0]                          # bank 0
    # one banked call is two banked calls cut at any view
    cut = {2: 1, 3: 2}.get(b["F"], (2 * b["F"]) // 5)
    begin(eng, b)
    eng.ibank_train_u8(b["views"][:cut], b["bank_of"][:cut])
    eng.ibank_train_u8(b["views"][cut:], b["bank_of"][cut:])
    assert eng.ibank_info()["views_trained"].tolist() == b["counts"].tolist()
    for r in range(HB.R):
        same_bits(eng.ibank_read_weights(r), got[r], (key, r, "cut at %d" % cut))
    # no views: legal, and nothing moves
    eng.ibank_train_u8(b["views"][:0], b["bank_of"][:0])
    same_bits(eng.ibank_read_weights(2), got[2])


def test_single_model_calls_act_on_bank_0_and_touch_no_other(eng, lone):
    b = HB.bank_data("40x1")
    k = 9
    begin(eng, b)
    eng.infomax_train_u8(b["views"][:k])                                                 # before: bank 0's chain begins
    assert eng.ibank_info()["views_trained"].tolist() == [k, 0, 0] and eng.infomax_info()["views_trained"] == k
    same_bits(eng.ibank_read_weights(1), b["W0"])
    same_bits(eng.ibank_read_weights(2), b["W0"])
    eng.ibank_train_u8(b["views"], b["bank_of"])
    in0 = b["views"][b["bank_of"] == 0]
    w0 = lone_chain(lone, b, np.concatenate([b["views"][:k], in0]))
    same_bits(eng.ibank_read_weights(0), w0)
    same_bits(eng.infomax_read_weights(), w0)
    w12 = [eng.ibank_read_weights(r) for r in (1, 2)]
    for r in (1, 2):
        same_bits(w12[r - 1], lone_chain(lone, b, b["views"][b["bank_of"] == r]), r)
    # after: scoring, stepping, training and set_weights of the single model are bank 0's
    lone.infomax_begin(b["h"], b["w"], w0, 2, H.ETA)
    same_bits(eng.infomax_score_u8(b["patches"]), lone.infomax_score_u8(b["patches"]))
    d = HB.layout_data("40x1", 5, 13)
    same_bits(eng.infomax_step_batch_u8(d["planes"]).angle_familiarity, lone.infomax_step_batch_u8(d["planes"]).angle_familiarity)
    eng.infomax_train_u8(b["views"][:3])
    lone.infomax_train_u8(b["views"][:3])
    same_bits(eng.infomax_read_weights(), lone.infomax_read_weights())
    eng.infomax_set_weights(b["Ws"][0])
    same_bits(eng.ibank_read_weights(0), b["Ws"][0])
    for r in (1, 2):
        same_bits(eng.ibank_read_weights(r), w12[r - 1], r)
    assert eng.ibank_info()["views_trained"].tolist() == [k + b["counts"][0] + 3, b["counts"][1], b["counts"][2]]


def test_a_slab_edge_cuts_every_banks_chain_and_keeps_its_bits(eng, lone):
    """32x32 views, 4 rows: the x vectors are staged 8192 at a time over ALL banks, so 8192 + 5 views in two banks of unequal length end
    the first slab in the middle of both chains.  Each bank's bits are those of its chain alone (a device-against-device comparison)."""
    d = H.long_chain_data()
    assert d["F"] == 8192 + 5 and (64 << 20) // (8 * d["N"]) == 8192
    bank_of = (np.arange(d["F"]) % 3 == 1).astype(np.int32)                              # 5465 views in bank 0, 2732 in bank 1
    counts = np.bincount(bank_of).tolist()
    assert counts == [5465, 2732] and bank_of[:8192].sum() not in (0, counts[1])          # the edge cuts both chains
    begin(eng, d, n_banks=2)
    eng.ibank_train_u8(d["views"], bank_of)
    assert eng.ibank_info()["views_trained"].tolist() == counts
    for r in range(2):
        same_bits(eng.ibank_read_weights(r), lone_chain(lone, d, d["views"][bank_of == r]), r)


# ---- 2. the step on uploaded patches -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", HB.KEYS)
def test_step_scores_every_member_under_its_own_bank(eng, lone, key):
    b = HB.bank_data(key)
    begin(eng, b, weights=b["Ws"])
    results = {}
    for n, A in HB.LAYOUTS:
        d = HB.layout_data(key, n, A)
        res = eng.ibank_step_batch_u8(d["planes"], d["banks"])
        assert res.angle_familiarity.shape == (n, A) and not res.flags.any()
        results[(n, A)] = res
        err = float(np.max(np.abs(res.angle_familiarity - d["fam"]) / np.abs(d["fam"])))
        print("infomax banks, scores %s %dx%d: relative error %.3e (bound %.1e)" % (key, n, A, err, H.TOL))
        assert err <= H.TOL
        assert res.best_idex.tolist() == d["best"].tolist()                              # (margins above 1000 TOL: the host test)
        # members in another order: the results in that order, and no bit changes
        perm = np.random.default_rng(n * 100 + A).permutation(n)
        res2 = eng.ibank_step_batch_u8(np.ascontiguousarray(d["planes"][perm]), d["banks"][perm])
        same_bits(res2.angle_familiarity, res.angle_familiarity[perm], (key, n, A, "permuted"))
        assert res2.best_idex.tolist() == res.best_idex[perm].tolist()
    # every column is the single model's score of the patch on an engine that holds the bank's weights
    lone.infomax_begin(b["h"], b["w"], b["W0"], 2, H.ETA)
    for r in range(HB.R):
        lone.infomax_set_weights(b["Ws"][r])
        for n, A in HB.LAYOUTS:
            d = HB.layout_data(key, n, A)
            for i in np.flatnonzero(d["banks"] == r):
                same_bits(results[(n, A)].angle_familiarity[i], lone.infomax_score_u8(d["planes"][i]), (key, n, A, int(i), r))


@pytest.mark.parametrize("key", ("5x3_f2", "40x1"))                                      # 15 pixels and 40: N % 4 != 0 beside N % 4 == 0
def test_training_and_steps_take_turns_at_one_table_buffer(eng, lone, key):
    """A training call's chains and a step's column blocks go to the same device buffer, and a table is sent only when its content is
    not the one the buffer holds: train, step, train on the same tables, step on the same tables, then training twice running (the
    second finds its own table there).  Every bank is its chain alone and every row the single model's score, bit for bit."""
    b, d = HB.bank_data(key), HB.layout_data(key, 5, 13)
    begin(eng, b)
    for rounds in (1, 2, 4):
        for _ in range(1 if rounds < 4 else 2):
            eng.ibank_train_u8(b["views"], b["bank_of"].copy())
        res = eng.ibank_step_batch_u8(d["planes"], d["banks"].copy())
        assert eng.ibank_info()["views_trained"].tolist() == (rounds * b["counts"]).tolist()
        for r in range(HB.R):
            own = b["views"][b["bank_of"] == r]
            same_bits(eng.ibank_read_weights(r), lone_chain(lone, b, np.concatenate([own] * rounds)), (key, rounds, r))
            for i in np.flatnonzero(d["banks"] == r):                                    # (lone holds the chain's weights now)
                same_bits(res.angle_familiarity[i], lone.infomax_score_u8(d["planes"][i]), (key, rounds, int(i), r))
        assert res.best_idex.tolist() == np.argmax(res.angle_familiarity, axis=1).tolist()


# ---- 2b. steps past one launch: the byte bound and the block-count bound (layouts of tests/helpers_inet.py) ----------------------------------
def close(got, want, what):
    err = float(np.max(np.abs(np.asarray(got) - want)) / np.max(np.abs(want)))
    print("infomax banks, %s: relative error %.3e (bound %.1e)" % (what, err, H.TOL))
    assert err <= H.TOL, (what, err)


def test_a_step_past_the_slab_scores_its_second_launch_behind_an_uploaded_slab(eng, lone):
    """688 members x 12 headings of 32 x 32 views over four banks of M = 24: launch 2 begins at column 8176, inside a member of bank 1,
    with blocks of 44, 24 and 12 columns of banks 1, 2 and 3 -- k_im_score_cols_banks<true> at a non-zero x_first behind a slab of
    uploaded planes, and k_im_decide_banks over a member whose columns come from two launches."""
    from tests import helpers_inet as HN
    d, lay = HB.slab_step_data(), HN.slab_layout()
    begin(eng, d, n_banks=4, eta=HB.SLAB["eta"], weights=d["Ws"])
    res = eng.ibank_step_batch_u8(d["planes"], d["banks"])
    assert not res.flags.any()
    behind = lay["order"][lay["c0"] // lay["A"]:]
    close(res.angle_familiarity[behind], d["fam"][behind], "32x32 slab layout, the %d members of launch 2" % len(behind))
    close(res.angle_familiarity, d["fam"], "32x32 slab layout, %d members x %d headings" % d["fam"].shape)
    rows = np.arange(len(d["banks"]))
    same_bits(res.angle_familiarity[rows, d["first"]], res.angle_familiarity[rows, d["second"]], "equal patches")
    assert res.best_idex.tolist() == d["first"].tolist()                                  # the first of two equal maxima, across the cut too
    lone.infomax_begin(d["h"], d["w"], d["W0"], 2, HB.SLAB["eta"])
    for r in range(4):
        lone.infomax_set_weights(d["Ws"][r])
        for i in np.flatnonzero(d["banks"] == r):
            same_bits(res.angle_familiarity[i], lone.infomax_score_u8(d["planes"][i]), (int(i), r))
    again = eng.ibank_step_batch_u8(d["planes"], d["banks"])
    same_bits(again.angle_familiarity, res.angle_familiarity, "the second call")
    # ... and trained on the device, every bank is its chain alone
    begin(eng, d, n_banks=4, eta=HB.SLAB["eta"])
    eng.ibank_train_u8(d["views"], d["bank_of"])
    for r in range(4):
        close(eng.ibank_read_weights(r), d["Ws"][r], "32x32 slab layout, bank %d weights" % r)


def test_a_step_of_16385_blocks_scores_the_last_block_in_a_launch_of_its_own(eng, lone):
    """16385 banks of M = 15, one member x 3 headings of 7 x 5 views each, in a scrambled order: the scoring grid's y extent takes 16384
    blocks, launch 2 is bank 16384's one block at c0 = 49152 (k_im_score_cols_banks<false>).  Banks 0, 16383 and 16384 hold trained
    weights.  Device memory: X 67.1 MB (239616 columns x 35 x 8: the slab, far from full), dpart 8.4 MB (one row tile x 1048640 padded
    columns x 8), weights 68.8 MB (16385 x 15 x 35 x 8)."""
    d = HB.blocks_data()
    B = len(d["banks"])
    eng.infomax_begin(d["h"], d["w"], d["W0"], 2, HB.BLOCKS["eta"])
    eng.ibank_set(B, d["W0"])
    for b, W in d["trained"].items():
        eng.ibank_set_weights(b, W)
    res = eng.ibank_step_batch_u8(d["planes"], d["banks"])
    assert not res.flags.any()
    close(res.angle_familiarity[d["last"]], d["fam"][d["last"]], "7x5, 16385 blocks: the member of launch 2")
    close(res.angle_familiarity, d["fam"], "7x5, 16385 blocks")
    assert res.best_idex.tolist() == np.argmax(res.angle_familiarity, axis=1).tolist()
    lone.infomax_begin(d["h"], d["w"], d["W0"], 2, HB.BLOCKS["eta"])
    for b in (1, 2, 8191, 8192, B - 4, B - 3):                                            # banks at W0, up to the last blocks of launch 1
        i = d["order"][b]
        same_bits(res.angle_familiarity[i], lone.infomax_score_u8(d["planes"][i]), b)
    for b, W in d["trained"].items():                                                     # ... and both sides of block 16384
        lone.infomax_set_weights(W)
        i = d["order"][b]
        same_bits(res.angle_familiarity[i], lone.infomax_score_u8(d["planes"][i]), b)
    again = eng.ibank_step_batch_u8(d["planes"], d["banks"])
    same_bits(again.angle_familiarity, res.angle_familiarity, "the second call")
    # the three banks trained on the device, with 16385 as the training grids' extents
    eng.ibank_set(B, d["W0"])
    eng.ibank_train_u8(d["views"], d["bank_of"])
    counts = np.zeros(B, dtype=np.int64)
    counts[list(d["trained"])] = 3
    assert eng.ibank_info()["views_trained"].tolist() == counts.tolist()
    for b, W in d["trained"].items():
        close(eng.ibank_read_weights(b), W, "7x5 bank %d of 16385, weights" % b)
    same_bits(eng.ibank_read_weights(B - 3), d["W0"], "an untrained bank")


# ---- 3. sensed: three routes on the landscape of helpers_infomax.SENSED ----------------------------------------------------------------------
def _sensed_agent():
    return H.sensed_agent(infomax_familiarity(**HB.SENSED_MODEL), True)


@pytest.fixture(scope="module")
def sensed():
    """(the banked engine trained on the three routes in one call, the views it returned, the lone agents: one a route)."""
    s = HB.sensed_data()
    a = _sensed_agent()
    e = a._engine
    alone = []
    try:
        m = HB.SENSED_MODEL
        e.infomax_begin(32, 32, s["W0"], 2, m["learning_rate"])
        e.ibank_set(HB.R, s["W0"])
        x, y, ang, bank_of, _ = HB.interleaved_poses()
        views = e.ibank_train_from_poses(x, y, ang, bank_of)
        for route in HB.sensed_routes():
            alone.append(_sensed_agent())
            alone[-1].train_from_path(route)
        yield e, views, alone
    finally:
        e.close()
        for l in alone:
            l.clear_training()


def test_training_from_poses_is_every_routes_lone_training(sensed):
    e, views, alone = sensed
    s = HB.sensed_data()
    _, _, _, bank_of, first = HB.interleaved_poses()
    assert views.shape == (len(bank_of), 32, 32, 3) and e.ibank_info()["views_trained"].tolist() == list(HB.SENSED_POINTS)
    worst = 0.0
    for r in range(HB.R):
        assert views[first[r]].tobytes() == s["scenes"][r].tobytes(), r                  # out_views: the host sensor model's views
        assert alone[r].familiar_scenes.tobytes() == s["scenes"][r].tobytes(), r
        W = e.ibank_read_weights(r)
        same_bits(W, alone[r]._engine.infomax_read_weights(), r)
        worst = max(worst, float(np.max(np.abs(W - s["Ws"][r])) / np.max(np.abs(s["Ws"][r]))))
    print("infomax banks, sensed routes: relative error of the weights %.3e (bound %.1e)" % (worst, H.TOL))
    assert worst <= H.TOL


def _member_poses(A=9):
    xs, ys, centre = HE.sensed_poses(A)
    return xs, ys, (centre[:, None] + np.linspace(-np.pi / 2, np.pi / 2, A)[None, :]) % (2 * np.pi)


def test_sense_step_is_every_members_lone_step_and_a_member_off_the_landscape_is_flagged(sensed):
    e, _, alone = sensed
    xs, ys, angs = _member_poses()
    banks = np.array([2, 0, 1, 1, 0], dtype=np.int32)
    res = e.ibank_sense_step_batch(xs, ys, angs, banks)
    assert not res.flags.any()
    for i in range(5):
        best, fam = alone[banks[i]]._engine.infomax_sense_step(xs[i], ys[i], angs[i])
        same_bits(res.angle_familiarity[i], fam, i)
        assert res.best_idex[i] == best == int(np.argmax(fam)) and len(np.unique(fam)) > 1, i
    # under bank 0 everywhere the scores are others: the table is what tells the members apart
    all0 = e.ibank_sense_step_batch(xs, ys, angs, np.zeros(5, dtype=np.int32))
    for i in range(5):
        assert (H.bits(all0.angle_familiarity[i]) == H.bits(res.angle_familiarity[i])).all() == (banks[i] == 0), i
    # one member's footprint leaves the landscape at one heading
    HS.flag_facts("sq")
    x, y = HS.FLAG_AT["sq"]
    xs2, ys2, angs2 = xs.copy(), ys.copy(), angs.copy()
    xs2[2], ys2[2] = x, y
    angs2[2] = HS.safe_angles(angs.shape[1], 100)
    angs2[2, 3] = np.deg2rad(HS.OFF_DEG[0])
    assert HS.is_off("sq", x, y, angs2[2, 3]) and not any(HS.is_off("sq", x, y, a) for a in np.delete(angs2[2], 3))
    res2 = e.ibank_sense_step_batch(xs2, ys2, angs2, banks)
    assert res2.flags.tolist() == [0, 0, SENSE_ERROR, 0, 0] and res2.best_idex[2] == -1
    for i in (0, 1, 3, 4):
        same_bits(res2.angle_familiarity[i], res.angle_familiarity[i], i)
        assert res2.best_idex[i] == res.best_idex[i], i
    again = e.ibank_sense_step_batch(xs, ys, angs, banks)                                # ... and the next call without it is as before
    same_bits(again.angle_familiarity, res.angle_familiarity)
    assert again.best_idex.tolist() == res.best_idex.tolist() and not again.flags.any()


def test_a_route_that_leaves_the_landscape_trains_nothing(sensed):
    e, _, _ = sensed
    before = [e.ibank_read_weights(r) for r in range(HB.R)]
    counts = e.ibank_info()["views_trained"].tolist()
    x, y, ang, bank_of, _ = HB.interleaved_poses()
    x, y, ang = x.copy(), y.copy(), ang.copy()
    x[7], y[7], ang[7] = HS.FLAG_AT["sq"][0], HS.FLAG_AT["sq"][1], np.deg2rad(HS.OFF_DEG[0])
    with pytest.raises(IndexError):
        e.ibank_train_from_poses(x, y, ang, bank_of)
    assert e.ibank_info()["views_trained"].tolist() == counts
    for r in range(HB.R):
        same_bits(e.ibank_read_weights(r), before[r], r)


# ---- 4. divergence ---------------------------------------------------------------------------------------------------------------------------
def test_a_diverging_bank_is_named_and_the_others_go_on(eng, lone):
    b = HB.bank_data("16x16_a16")
    eta = H.diverging_eta()
    with np.errstate(all="ignore"):
        one_ok = bool(np.isfinite(H.train(b["W0"], b["views"][:1], eta=eta)).all())      # decided by the statement
        assert not np.isfinite(H.train(b["W0"], b["views"], eta=eta)).all()
    at = 5
    extra = b["views"][:1] if one_ok else b["views"][:0]
    planes = np.concatenate([b["views"][:at], extra, b["views"][at:]])
    table = np.ones(len(planes), dtype=np.int32)
    if one_ok:
        table[at] = 0                                                                    # bank 0's single view, in the middle of bank 1's
    begin(eng, b, eta=eta)
    with pytest.raises(navsim_amd.EngineError, match="DV_ERR_STATE") as ei:
        eng.ibank_train_u8(planes, table)
    assert "bank 1" in str(ei.value) and "learning_rate 1" in str(ei.value)
    info = eng.ibank_info()
    assert info["finite"].tolist() == [True, False, True]
    assert info["views_trained"].tolist() == [int(one_ok), len(b["views"]), 0]
    same_bits(eng.ibank_read_weights(0), lone_chain(lone, b, extra, eta=eta))             # the finite banks hold their own chains' bits
    same_bits(eng.ibank_read_weights(2), b["W0"])
    d = HB.layout_data("16x16_a16", 5, 13)
    ok = eng.ibank_step_batch_u8(d["planes"], np.array([0, 2, 0, 0, 2], dtype=np.int32))  # a step that names finite banks only
    assert np.isfinite(ok.angle_familiarity).all()
    with pytest.raises(navsim_amd.EngineError, match="DV_ERR_STATE") as ei:
        eng.ibank_step_batch_u8(d["planes"], np.array([0, 2, 1, 0, 2], dtype=np.int32))
    assert "bank_of_member[2]" in str(ei.value) and "not finite" in str(ei.value)
    with pytest.raises(navsim_amd.EngineError, match="DV_ERR_STATE"):
        eng.ibank_train_u8(b["views"][:2], [2, 1])
    assert eng.ibank_info()["views_trained"].tolist() == [int(one_ok), len(b["views"]), 0]     # (refused before anything was trained)
    eng.ibank_train_u8(b["views"][:1], [2])                                              # a call that names finite banks only works
    eng.ibank_set_weights(1, b["W0"])                                                    # finite weights heal the bank
    assert eng.ibank_info()["finite"][1]
    healed = eng.ibank_step_batch_u8(d["planes"], np.array([0, 2, 1, 0, 2], dtype=np.int32))
    assert np.isfinite(healed.angle_familiarity).all()
    lone.infomax_begin(b["h"], b["w"], b["W0"], 2, eta)
    same_bits(healed.angle_familiarity[2], lone.infomax_score_u8(d["planes"][2]))


# ---- 5. refusals on the device side, lifecycle -------------------------------------------------------------------------------------------
def test_a_bank_out_of_range_is_refused_and_nothing_changes(eng):
    b = HB.bank_data("40x1")
    begin(eng, b, weights=b["Ws"])
    d = HB.layout_data("40x1", 5, 13)
    lib, ctx = eng._lib, eng._ctx
    fam, best = np.zeros((5, 13)), np.zeros(5, dtype=np.int32)
    for bad in (HB.R, -1):
        for at in (0, 20, len(b["views"]) - 1):
            table = b["bank_of"].copy()
            table[at] = bad
            assert lib.dv_ibank_train_u8(ctx, N.u8ptr(b["views"]), len(b["views"]), table.ctypes.data_as(N._i32p)) == INVALID
            assert ("bank_of_view[%d] = %d" % (at, bad)) in lib.dv_last_error(ctx).decode()
        for at in (0, 4):
            table = d["banks"].copy()
            table[at] = bad
            assert lib.dv_ibank_step_u8(ctx, N.u8ptr(d["planes"]), 5, 13, table.ctypes.data_as(N._i32p), N.f64ptr(fam),
                                        best.ctypes.data_as(N._i32p)) == INVALID
            assert ("bank_of_member[%d] = %d" % (at, bad)) in lib.dv_last_error(ctx).decode()
    assert lib.dv_ibank_train_u8(ctx, N.u8ptr(b["views"]), len(b["views"]), None) == INVALID
    assert lib.dv_ibank_set(ctx, 0, N.f64ptr(b["W0"])) == INVALID and lib.dv_ibank_set(ctx, 2, None) == INVALID
    assert lib.dv_ibank_read_weights(ctx, HB.R, N.f64ptr(np.empty_like(b["W0"]))) == INVALID
    assert eng.ibank_info()["views_trained"].tolist() == [0, 0, 0] and eng.ibank_info()["n_banks"] == HB.R
    for r in range(HB.R):
        same_bits(eng.ibank_read_weights(r), b["Ws"][r], r)
    # the engine's own check is the same refusal, before the library; a table the engine cannot know to be stale reaches the library's
    with pytest.raises(ValueError, match="bank_of_view"):
        eng.ibank_train_u8(b["views"][:4], [0, 1, 2, 3])
    eng.infomax_banks = 4                                                                # (what the engine believes; the library holds 3)
    try:
        with pytest.raises(ValueError, match="DV_ERR_INVALID"):
            eng.ibank_train_u8(b["views"][:4], [0, 1, 2, 3])
    finally:
        eng.infomax_banks = HB.R
    res = eng.ibank_step_batch_u8(d["planes"], d["banks"])
    assert res.best_idex.tolist() == d["best"].tolist()


def test_ibank_calls_without_a_model_are_state_errors():
    e = navsim_amd.FamiliarityEngine(device=0)
    try:
        t = np.zeros(2, dtype=np.int32)
        planes, fam, best, flags = np.zeros((2, 3, 5), np.uint8), np.zeros(15 * 15), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.uint32)
        tp, bp = t.ctypes.data_as(N._i32p), best.ctypes.data_as(N._i32p)
        lib, ctx = e._lib, e._ctx
        assert lib.dv_ibank_set(ctx, 2, N.f64ptr(fam)) == STATE
        assert lib.dv_ibank_train_u8(ctx, N.u8ptr(planes), 2, tp) == STATE
        assert lib.dv_ibank_train_from_poses(ctx, N.f64ptr(fam), N.f64ptr(fam), N.f64ptr(fam), 2, tp, None) == STATE
        assert lib.dv_ibank_step_u8(ctx, N.u8ptr(planes), 2, 1, tp, N.f64ptr(fam), bp) == STATE
        assert lib.dv_ibank_sense_step(ctx, N.f64ptr(fam), N.f64ptr(fam), N.f64ptr(fam), 2, 1, tp, N.f64ptr(fam), bp,
                                       flags.ctypes.data_as(N._u32p)) == STATE
        assert lib.dv_ibank_read_weights(ctx, 0, N.f64ptr(fam)) == STATE and lib.dv_ibank_set_weights(ctx, 0, N.f64ptr(fam)) == STATE
        info = e.ibank_info()
        assert info["n_banks"] == 1 and info["views_trained"].tolist() == [0] and info["finite"].tolist() == [False]
        e.infomax_begin(3, 5, H.initial_weights(15, 15, 1))
        e.ibank_set(2, H.initial_weights(15, 15, 1))
        assert lib.dv_ibank_sense_step(ctx, N.f64ptr(fam), N.f64ptr(fam), N.f64ptr(fam), 2, 1, tp, N.f64ptr(fam), bp,
                                       flags.ctypes.data_as(N._u32p)) == STATE            # a model but no sensor
        e.infomax_end()
        assert e.ibank_info()["n_banks"] == 1 and lib.dv_ibank_set(ctx, 2, N.f64ptr(fam)) == STATE
    finally:
        e.close()


def test_two_engines_with_their_own_banks_and_set_drops_what_was_trained(eng, lone):
    b, c = HB.bank_data("40x1"), HB.bank_data("5x3_f2")
    begin(eng, b)
    begin(lone, c, n_banks=5)
    table5 = np.array([4, 3], dtype=np.int32)
    eng.ibank_train_u8(b["views"], b["bank_of"])
    lone.ibank_train_u8(c["views"], table5)
    assert eng.ibank_info()["n_banks"] == 3 and lone.ibank_info()["n_banks"] == 5
    assert lone.ibank_info()["views_trained"].tolist() == [0, 0, 0, 1, 1] and eng.ibank_info()["views_trained"].tolist() == b["counts"].tolist()
    for r in range(HB.R):
        err = float(np.max(np.abs(eng.ibank_read_weights(r) - b["Ws"][r])) / np.max(np.abs(b["Ws"][r])))
        assert err <= H.TOL, (r, err)
    for r, v in ((4, 0), (3, 1)):
        want = H.train(c["W0"], c["views"][v:v + 1])
        assert float(np.max(np.abs(lone.ibank_read_weights(r) - want)) / np.max(np.abs(want))) <= H.TOL, r
    same_bits(lone.ibank_read_weights(1), c["W0"])
    # ibank_set after training: every bank is the given weights again, the counts are 0, the number of banks is the new one
    trained = eng.ibank_read_weights(0)
    eng.ibank_set(2, b["Ws"][1])
    info = eng.ibank_info()
    assert info["n_banks"] == 2 and info["views_trained"].tolist() == [0, 0] and info["finite"].tolist() == [True, True]
    assert eng.infomax_info()["views_trained"] == 0
    for r in range(2):
        same_bits(eng.ibank_read_weights(r), b["Ws"][1], r)
    assert not np.array_equal(trained, b["Ws"][1])
    with pytest.raises(ValueError, match="bank must be an integer"):
        eng.ibank_read_weights(2)
    # infomax_begin returns to one bank
    eng.infomax_begin(b["h"], b["w"], b["W0"], 2, H.ETA)
    assert eng.ibank_info()["n_banks"] == 1 and eng.infomax_banks == 1
    assert lone.ibank_info()["n_banks"] == 5                                             # (the other engine's model is its own)


# ---- 6. the ensemble ---------------------------------------------------------------------------------------------------------------------------
def make_agent():
    return navsim_amd.NavBySceneFamiliarity(synth.synth_landscape(3, 300, 4), HB.ENSEMBLE_SENSOR, 1.0, n_test_angles=9, use_gpu_sensor=True,
                                            familiarity_model=infomax_familiarity(**HB.ENSEMBLE_MODEL))


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
    ens = navsim_amd.InfomaxRouteEnsemble.from_routes(make_agent(), paths, starts)
    alone = _lone(paths, starts)
    calls = []
    inner = ens.engine.ibank_sense_step_batch

    def counted(*a, **k):
        calls.append(list(a[3]))
        return inner(*a, **k)
    ens.engine.ibank_sense_step_batch = counted
    try:
        assert len(ens.agents) == 6 and [a.memory_bank for a in ens.agents] == [0, 0, 1, 1, 2, 2]
        info = ens.bank_info()
        assert info["n_banks"] == 3 and info["views_trained"].tolist() == [len(p) for p in paths] and info["finite"].all()
        for r in range(3):
            same_bits(ens.engine.ibank_read_weights(r), alone[2 * r]._engine.infomax_read_weights(), r)
        for m, a in zip(ens.agents, alone):
            assert m._metric_slot is None and not m._metrics_on_device                   # the host's metrics
            assert np.array_equal(m.training_path, a.training_path) and m.training_path_length == a.training_path_length
            assert np.array_equal(m.familiar_scenes, a.familiar_scenes)
        with pytest.raises(ValueError, match="InfomaxRouteEnsemble"):
            ens.agents[1].step_forward()
        with pytest.raises(ValueError, match="InfomaxEnsemble does not take a member of a InfomaxRouteEnsemble"):
            navsim_amd.InfomaxEnsemble(ens.agents)
        for t in range(12):
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
                same_bits(m.angle_familiarity, a.angle_familiarity, (t, i))
                same_bits(m.scene_familiarity, a.scene_familiarity, (t, i))
                code = a.stopped_with_exception.get_code() if a.stopped_with_exception is not None else 0
                assert ens.stop_status[i] == code, (t, i)
                assert m.navigation_error == a.navigation_error and m.percent_recapitulated == a.percent_recapitulated, (t, i)
    finally:
        ens.engine.ibank_sense_step_batch = inner
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
    ens = navsim_amd.InfomaxRouteEnsemble.from_routes(make_agent(), paths, starts)
    try:
        assert ens.bank_info()["views_trained"].tolist() == list(HB.ROUTE_POINTS)
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
