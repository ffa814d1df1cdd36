"""Network tables of the Infomax model on the device (dv_inet_*): banks with n_hidden, learning rate, W0 and channel of their own,
trained in shared lockstep launches and scored member by member.  Against lone engines begun with one network each: np.array_equal on
the doubles' uint64 views.  Against the NumPy statement run per bank with that bank's W0, rate and channel (tests/helpers_inet.py over
tests/helpers_infomax.py): within helpers_infomax.TOL, relative to max|W| and max|d|, every figure printed before it is asserted.
InfomaxRouteEnsemble(networks=...) against lone agents built with infomax_familiarity of the member's network and trained on its route
alone.  The steps of section 5b run past one launch (helpers_inet.SLAB: the staging slab's bytes; helpers_inet.BLOCKS: the scoring grid's
blocks); tests/test_inet_host.py asserts of their layouts that the second launch is reached and that an index local to it would show."""
import csv
import io

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import infomax_familiarity, synth
from tests import helpers_inet as HN
from tests import helpers_infomax as H
from tests import helpers_infomax_banks as HB
from tests import helpers_lands as HL
from tests import helpers_sensed_models as HS
from tests import helpers_sensors as HSN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def lone():
    """The engine that is begun with ONE network at a time."""
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


def same_bits(got, want, what=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape)
    bad = np.argwhere(H.bits(got) != H.bits(want))
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def close(got, want, what):
    r = HN.rel(got, want)
    print("%s: %.3g relative (TOL %g)" % (what, r, H.TOL))
    assert r <= H.TOL, (what, r)
    return r


def begin_lone(e, h, w, net):
    e.infomax_begin(h, w, net["w0"], net["channel"], net["learning_rate"])


def begin_table(e, h, w, nets, net_of_bank):
    begin_lone(e, h, w, nets[0])
    e.inet_set(nets, net_of_bank)


def check_against_lone_engines(lone, d, got, planes=None, banks=None, res=None):
    """Bank by bank: an engine begun with the bank's network alone and trained on the bank's views, in their order, gives the bank's
    weights; its score of a member's patches gives the member's row."""
    for b, p in enumerate(d["net_of_bank"]):
        begin_lone(lone, d["h"], d["w"], d["nets"][p])
        mine = np.ascontiguousarray(d["views"][np.asarray(d["bank_of"]) == b])
        if len(mine):
            lone.infomax_train_u8(mine)
        same_bits(lone.infomax_read_weights(), got[b], ("weights of bank", b))
        for i in np.flatnonzero(np.asarray(banks) == b) if banks is not None else ():
            same_bits(lone.infomax_score_u8(np.ascontiguousarray(planes[i])), res.angle_familiarity[i], ("member", int(i), "bank", b))


def train_table(eng, d):
    begin_table(eng, d["h"], d["w"], d["nets"], d["net_of_bank"])
    eng.ibank_train_u8(d["views"], d["bank_of"])
    return [eng.ibank_read_weights(b) for b in range(len(d["net_of_bank"]))]


# ---- 1. ragged M on the scalar-load path: five networks and seven banks on 7 x 5 views ---------------------------------------------------
def test_one_table_trains_every_bank_through_its_own_network(eng, lone):
    d = HN.table_data()
    nets, of_bank, B = d["nets"], d["net_of_bank"], len(d["net_of_bank"])
    assert d["N"] % 4 != 0
    begin_table(eng, d["h"], d["w"], nets, of_bank)
    info = eng.inet_info()
    assert (info["n_nets"], info["n_banks"]) == (5, 7) and info["network_of_bank"].tolist() == list(of_bank)
    assert info["n_hidden"].tolist() == [M for M, _ in HN.TABLE["nets"]] and info["learning_rate"].tolist() == [r for _, r in HN.TABLE["nets"]]
    assert info["channel"].tolist() == [2] * 5 and info["views_trained"].tolist() == [0] * B and info["finite"].all()
    rows = [nets[p]["n_hidden"] for p in of_bank]
    assert info["bytes"] >= 8 * d["N"] * sum(rows)
    for b in range(B):                                                                    # every bank starts as its network's W0
        same_bits(eng.ibank_read_weights(b), nets[of_bank[b]]["w0"], b)
    eng.ibank_train_u8(d["views"], d["bank_of"])                                          # 40 views, all banks and networks: one call
    got = [eng.ibank_read_weights(b) for b in range(B)]
    assert [g.shape for g in got] == [(M, d["N"]) for M in rows]
    worst = max(close(got[b], d["Ws"][b], "7x5 bank %d (M = %d) weights" % (b, rows[b])) for b in range(B))
    print("7x5 table: weights within %.3g of the statement" % worst)
    same_bits(got[5], nets[1]["w0"], "the bank without a view")
    counts = np.bincount(d["bank_of"], minlength=B).tolist()
    for info in (eng.ibank_info(), eng.inet_info()):
        assert info["n_banks"] == B and info["views_trained"].tolist() == counts and info["finite"].all()
    one = eng.infomax_info()                                                              # the begin's model; the two counts are bank 0's
    assert (one["n_hidden"], one["n_pixels"], one["views_trained"], one["finite"]) == (1, 35, counts[0], True)
    check_against_lone_engines(lone, d, got)


# ---- 2. the VEC loads: 8 x 8 views with M = 16, 17 and 1040 in one table ------------------------------------------------------------------
def test_the_vector_loads_under_three_row_counts_in_one_table(eng, lone):
    d = HN.vec_data()
    got = train_table(eng, d)
    for b in range(3):
        close(got[b], d["Ws"][b], "8x8 bank %d weights" % b)
    banks = np.array([2, 0, 1, 2], dtype=np.int32)
    planes = H.route_views(HN.VEC["seed"] + 9, 4 * 5, d["h"], d["w"]).reshape(4, 5, d["h"], d["w"]).copy()
    planes[:, 1] = d["views"][:4]
    res = eng.ibank_step_batch_u8(planes, banks)
    close(res.angle_familiarity, HN.scores(d["nets"], d["net_of_bank"], d["Ws"], planes, banks), "8x8 scores")
    assert res.best_idex.tolist() == np.argmax(res.angle_familiarity, axis=1).tolist() and not res.flags.any()
    check_against_lone_engines(lone, d, got, planes, banks, res)


# ---- 3. a step over the table of test 1 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", HN.STEP_HEADINGS)
def test_a_step_scores_every_member_under_its_own_bank(eng, lone, A):
    d, s = HN.table_data(), HN.step_data(A)
    got = train_table(eng, d)
    assert np.bincount(s["banks"]).max() * A > 64                                         # a bank's columns are cut into blocks
    res = eng.ibank_step_batch_u8(s["planes"], s["banks"])
    assert not res.flags.any()
    close(res.angle_familiarity, s["fam"], "7x5 step, %d headings" % A)
    rows = np.arange(len(s["banks"]))
    same_bits(res.angle_familiarity[rows, s["first"]], res.angle_familiarity[rows, s["second"]], "equal patches")
    assert res.best_idex.tolist() == s["first"].tolist()                                  # the first of the two maxima
    check_against_lone_engines(lone, d, got, s["planes"], s["banks"], res)


# ---- 4. channels: 33 x 31 views sensed from poses, one W0 under H, S and V -----------------------------------------------------------------
SENSED = dict(sensor=(33, 31), pixel=[2, 2], levels=5, M=20, eta=1e-3, seed=441)


def sensed_agent(gpu):
    model = infomax_familiarity(learning_rate=SENSED["eta"], seed=3, n_hidden=8) if gpu else HS._keep
    return navsim_amd.NavBySceneFamiliarity(synth.synth_landscape(*H.SENSED["land"]), SENSED["sensor"], 1.0, n_test_angles=9,
                                            sensor_pixel_dimensions=list(SENSED["pixel"]), n_sensor_levels=SENSED["levels"], mask_middle_n=0,
                                            use_gpu_sensor=gpu, familiarity_model=model)


def host_scenes(agent, x, y, angles):
    return np.stack([agent.get_sensor_mat((xi, yi), ai) for xi, yi, ai in zip(np.ravel(x), np.ravel(y), np.ravel(angles))])


def test_sensed_poses_train_and_score_each_bank_under_its_own_channel():
    w, h = SENSED["sensor"]
    nets = [HN.network(w * h, SENSED["M"], SENSED["eta"], SENSED["seed"], channel=ch) for ch in (0, 1, 2)]
    assert np.array_equal(nets[0]["w0"], nets[2]["w0"])                                   # one W0
    x, y, ang = HS.route_poses()
    F = len(x)
    host = sensed_agent(False)
    scenes = host_scenes(host, x, y, ang)
    bank_of = np.tile(np.arange(3, dtype=np.int32), F)                                    # every pose three times, once into every bank
    x3, y3, a3 = np.repeat(x, 3), np.repeat(y, 3), np.repeat(ang, 3)
    Ws = HN.train(nets, (0, 1, 2), np.repeat(scenes, 3, axis=0), bank_of)
    assert all(HN.rel(Ws[a], Ws[b]) > 1e-6 for a in range(3) for b in range(a + 1, 3))    # the three banks differ
    xs, ys, angs = HS.member_poses()
    banks = [0, 1, 2, 0, 1]
    member_scenes = host_scenes(host, np.repeat(xs, angs.shape[1]), np.repeat(ys, angs.shape[1]), angs).reshape(angs.shape + (h, w, 3))
    want = HN.scores(nets, (0, 1, 2), Ws, member_scenes, banks)
    a, b = sensed_agent(True), sensed_agent(True)
    try:
        e = a._engine
        begin_table(e, h, w, nets, (0, 1, 2))
        views = e.ibank_train_from_poses(x3, y3, a3, bank_of)
        assert np.array_equal(views, np.repeat(scenes, 3, axis=0))                        # the device's sensor is the host's
        got = [e.ibank_read_weights(ch) for ch in range(3)]
        for ch in range(3):
            close(got[ch], Ws[ch], "33x31 channel %d weights" % ch)
        assert e.ibank_info()["views_trained"].tolist() == [F] * 3
        res = e.ibank_sense_step_batch(xs, ys, angs, banks)
        assert not res.flags.any()
        close(res.angle_familiarity, want, "33x31 sensed scores")
        for call in (lambda: e.infomax_train_from_poses(x, y, ang), lambda: e.infomax_sense_step(xs[0], ys[0], angs[0]),
                     lambda: e.infomax_sense_step_batch(xs, ys, angs)):                   # bank 0 behind the begin's shape: refused
            with pytest.raises(N.EngineError, match="dv_inet_clear.*DV_ERR_STATE"):
                call()
        # one member off the landscape: flagged, and the others' rows and decisions are what they were
        xo, yo = xs.copy(), ys.copy()
        xo[3], yo[3] = 295.0, 295.0                                                         # (the footprint passes the landscape's high edges at any heading)
        off = e.ibank_sense_step_batch(xo, yo, angs, banks)
        assert off.flags.tolist() == [0, 0, 0, HS.SENSE_ERROR, 0] and off.best_idex[3] == -1
        keep = [0, 1, 2, 4]
        same_bits(off.angle_familiarity[keep], res.angle_familiarity[keep], "beside a flagged member")
        assert off.best_idex[keep].tolist() == res.best_idex[keep].tolist()
        lone = b._engine
        for ch in range(3):                                                               # a lone agent's engine under the channel's network
            begin_lone(lone, h, w, nets[ch])
            lone.infomax_train_from_poses(x, y, ang, want_views=False)
            same_bits(lone.infomax_read_weights(), got[ch], ch)
            rows = [i for i, bk in enumerate(banks) if bk == ch]
            one = lone.infomax_sense_step_batch(xs[rows], ys[rows], angs[rows])
            same_bits(one.angle_familiarity, res.angle_familiarity[rows], ch)
            assert one.best_idex.tolist() == res.best_idex[rows].tolist()
    finally:
        a._engine.close()
        b._engine.close()


# ---- 5. the slab edge: 8193 views of 32 x 32 into M = 4 and M = 5 ---------------------------------------------------------------------------
def test_the_last_view_past_a_slab_keeps_its_own_bank_and_a_cut_call_its_bits(eng, lone):
    d = HN.edge_data()
    n = len(d["views"])
    begin_table(eng, d["h"], d["w"], d["nets"], (0, 1))
    eng.ibank_train_u8(d["views"], d["bank_of"])                                          # the last view alone is bank 1's, in a slab of its own
    got = [eng.ibank_read_weights(b) for b in range(2)]
    assert eng.ibank_info()["views_trained"].tolist() == [n - 1, 1]
    close(got[1], d["W1"], "the one view of bank 1")
    for b in range(2):                                                                    # lone chains
        begin_lone(lone, d["h"], d["w"], d["nets"][b])
        lone.infomax_train_u8(np.ascontiguousarray(d["views"][d["bank_of"] == b]))
        same_bits(lone.infomax_read_weights(), got[b], b)
    cut = HN.EDGE["cut"]
    eng.inet_set(d["nets"], (0, 1))
    eng.ibank_train_u8(d["views"][:cut], d["bank_of"][:cut])
    eng.ibank_train_u8(d["views"][cut:], d["bank_of"][cut:])
    for b in range(2):
        same_bits(eng.ibank_read_weights(b), got[b], ("cut at", cut, b))


# ---- 5b. a step past one launch: the byte bound (8192 columns of 32 x 32 views) and the block-count bound (16384 blocks) --------------------
def launch_2(lay):
    """The caller's members with a column in launch 2."""
    return lay["order"][lay["c0"] // lay["A"]:]


def test_a_step_past_the_slab_scores_its_second_launch_under_the_blocks_own_banks(eng, lone):
    """helpers_inet.SLAB on uploaded patches: launch 2 begins at column 8176, inside a member of bank 1, and holds a block of 44, 24 and 12
    columns of banks 1, 2 and 3 (M = 17, 33 and 5 under a grid sized for bank 0's 49) -- k_inet_score_cols<true> behind a non-zero
    x_first, k_inet_decide over columns of two launches."""
    d, lay = HN.slab_step_data(), HN.slab_layout()
    got = train_table(eng, d)
    for b in range(4):
        close(got[b], d["Ws"][b], "32x32 slab layout, bank %d weights" % b)
    res = eng.ibank_step_batch_u8(d["planes"], d["banks"])
    assert not res.flags.any()
    behind = launch_2(lay)
    close(res.angle_familiarity[behind], d["fam"][behind], "32x32 slab layout, the %d members of launch 2" % len(behind))
    close(res.angle_familiarity, d["fam"], "32x32 slab layout, %d members x %d headings" % d["fam"].shape)
    rows = np.arange(len(d["banks"]))
    same_bits(res.angle_familiarity[rows, d["first"]], res.angle_familiarity[rows, d["second"]], "equal patches")
    assert res.best_idex.tolist() == d["first"].tolist()                                  # the first of the two maxima, across the cut too
    check_against_lone_engines(lone, d, got, d["planes"], d["banks"], res)
    again = eng.ibank_step_batch_u8(d["planes"], d["banks"])                              # the table and the stage buffers are reused
    same_bits(again.angle_familiarity, res.angle_familiarity, "the second call")
    assert again.best_idex.tolist() == res.best_idex.tolist() and not again.flags.any()


@pytest.fixture(scope="module")
def sensing():
    """An engine with helpers_lands' 32 x 32 sensor, landscape 0 as its one landscape and the four landscapes as a set."""
    c = HL.SENSORS["sq"]
    e = navsim_amd.FamiliarityEngine(device=0)
    e.set_landscape(HL.lands()[0])
    e.configure_sensor(c["sensor"], c["pixel"], HL.level_tables("sq"), c["mask"])
    e.lands_set(list(HL.lands()))
    yield e
    e.close()


@pytest.mark.parametrize("form", ("set", "one"))
def test_a_sensed_step_past_the_slab_reads_every_member_at_its_own_banks_channel(sensing, form):
    """helpers_inet.SLAB sensed from poses, bank 0 on channel 2 and banks 1, 2, 3 on 0, 1, 0.  set: every member on its own landscape of
    the set (lands_launch_sense at c0); one: all on the engine's one landscape (k_sense_each at d_poses + c0).  Then a member of launch
    2 is moved off its landscape: its flag alone is set (im_perr + c0)."""
    e = sensing
    d, lay = HN.slab_sense_data(), HN.slab_layout()
    begin_table(e, d["h"], d["w"], d["nets"], d["net_of_bank"])
    e.ibank_train_u8(d["views"], d["bank_of"])
    for b in range(4):
        close(e.ibank_read_weights(b), d["Ws"][b], "32x32 slab layout, sensed (%s), bank %d weights" % (form, b))
    table = dict(land_of_member=d["lands"]) if form == "set" else {}
    want = d["fam_" + form]
    res = e.ibank_sense_step_batch(d["xs"], d["ys"], d["angs"], d["banks"], **table)
    assert not res.flags.any()
    behind = launch_2(lay)
    close(res.angle_familiarity[behind], want[behind], "32x32 slab layout, sensed (%s), the %d members of launch 2" % (form, len(behind)))
    close(res.angle_familiarity, want, "32x32 slab layout, sensed (%s)" % form)
    assert res.best_idex.tolist() == np.argmax(res.angle_familiarity, axis=1).tolist()
    m = d["flagged"]
    xs, ys = d["xs"].copy(), d["ys"].copy()
    if form == "set":
        lands = d["lands"].copy()
        xs[m], ys[m], lands[m] = HN.OFF_THE_SET
        table = dict(land_of_member=lands)
    else:
        xs[m], ys[m] = HN.OFF_THE_ONE
    off = e.ibank_sense_step_batch(xs, ys, d["angs"], d["banks"], **table)
    keep = np.delete(np.arange(len(xs)), m)
    assert off.flags[m] == HS.SENSE_ERROR and off.best_idex[m] == -1 and not off.flags[keep].any()
    same_bits(off.angle_familiarity[keep], res.angle_familiarity[keep], "beside a flagged member of launch 2")
    assert off.best_idex[keep].tolist() == res.best_idex[keep].tolist()


def lone_rows(lone, d, net, W, members, res):
    begin_lone(lone, d["h"], d["w"], net)
    if W is not None:
        lone.infomax_set_weights(W)
    for i in members:
        same_bits(lone.infomax_score_u8(np.ascontiguousarray(d["planes"][i])), res.angle_familiarity[i], ("member", int(i), "bank", int(d["banks"][i])))


def test_a_step_of_16385_blocks_scores_the_last_block_in_a_launch_of_its_own(eng, lone):
    """helpers_inet.BLOCKS: 16385 banks of one member x 3 headings of 7 x 5 views in a scrambled order; the scoring grid's y extent takes
    16384 blocks, so launch 2 is bank 16384's one block at c0 = 49152 (k_inet_score_cols<false>; M = 3 under a grid sized for 17).
    Banks 0, 16383 and 16384 are trained in one call, with 16385 as the training grids' y and z extents.  Device memory: X 67.1 MB
    (239616 columns x 35 x 8: the slab, far from full), dpart 16.8 MB (2 row tiles x 1048640 padded columns x 8), the ragged weights
    32.1 MB (114 701 rows x 35 x 8), h, u and upart 11.0 MB."""
    d = HN.blocks_data()
    B = HN.BLOCKS["banks"]
    begin_table(eng, d["h"], d["w"], d["nets"], d["net_of_bank"])
    eng.ibank_train_u8(d["views"], d["bank_of"])
    info = eng.inet_info()
    counts = np.zeros(B, dtype=np.int64)
    counts[list(d["trained"])] = HN.BLOCKS["views"]
    assert info["n_banks"] == B and info["views_trained"].tolist() == counts.tolist() and info["finite"].all()
    got = {b: eng.ibank_read_weights(b) for b in d["trained"]}
    for b, W in d["trained"].items():
        close(got[b], W, "7x5 bank %d of 16385, weights" % b)
    res = eng.ibank_step_batch_u8(d["planes"], d["banks"])
    assert not res.flags.any()
    close(res.angle_familiarity[d["last"]], d["fam"][d["last"]], "7x5, 16385 blocks: the member of launch 2")
    close(res.angle_familiarity, d["fam"], "7x5, 16385 blocks")
    assert res.best_idex.tolist() == np.argmax(res.angle_familiarity, axis=1).tolist()
    clear = np.flatnonzero(np.sort(d["fam"], axis=1)[:, -1] - np.sort(d["fam"], axis=1)[:, -2] > 1000 * H.TOL * np.abs(d["fam"]).max())
    assert len(clear) > B // 2 and res.best_idex[clear].tolist() == np.argmax(d["fam"][clear], axis=1).tolist()
    for b in d["trained"]:                                                                # lone engines: the trained banks ...
        net = d["nets"][d["net_of_bank"][b]]
        begin_lone(lone, d["h"], d["w"], net)
        lone.infomax_train_u8(np.ascontiguousarray(d["views"][d["bank_of"] == b]))
        same_bits(lone.infomax_read_weights(), got[b], ("weights of bank", b))
        lone_rows(lone, d, net, got[b], [d["order"][b]], res)
    for b in (1, 2, 3, 8191, 8192, B - 4, B - 3):                                         # ... and a handful at their W0, up to the last blocks
        same_bits(eng.ibank_read_weights(b), d["nets"][d["net_of_bank"][b]]["w0"], b)
        lone_rows(lone, d, d["nets"][d["net_of_bank"][b]], None, [d["order"][b]], res)
    again = eng.ibank_step_batch_u8(d["planes"], d["banks"])
    same_bits(again.angle_familiarity, res.angle_familiarity, "the second call")


# ---- 6. divergence is a bank's own ------------------------------------------------------------------------------------------------------------
def test_one_banks_divergence_names_its_own_rate_and_leaves_the_others_working(eng, lone):
    d = HN.diverge_data()
    begin_table(eng, d["h"], d["w"], d["nets"], (0, 1, 2))
    with pytest.raises(N.EngineError, match=r"bank 1 are not finite \(learning_rate 1 is too large.*DV_ERR_STATE"):
        eng.ibank_train_u8(d["views"], d["bank_of"])
    info = eng.inet_info()
    assert info["finite"].tolist() == [True, False, True] and info["views_trained"].tolist() == [d["F"]] * 3
    close(eng.ibank_read_weights(0), d["W0"], "bank 0 beside a diverged bank")
    close(eng.ibank_read_weights(2), d["W2"], "bank 2 beside a diverged bank")
    planes = np.ascontiguousarray(np.stack([d["patches"][:5], d["patches"][5:10]]))
    res = eng.ibank_step_batch_u8(planes, [2, 0])                                         # they still score
    for b, net in ((0, 0), (2, 2)):
        begin_lone(lone, d["h"], d["w"], d["nets"][net])
        lone.infomax_train_u8(np.ascontiguousarray(d["views"][d["bank_of"] == b]))
        same_bits(lone.infomax_read_weights(), eng.ibank_read_weights(b), b)
        same_bits(lone.infomax_score_u8(planes[0 if b == 2 else 1]), res.angle_familiarity[0 if b == 2 else 1], b)
    # a table that names the diverged bank is refused before anything is trained or scored
    before = [eng.ibank_read_weights(b) for b in (0, 2)]
    with pytest.raises(N.EngineError, match=r"bank_of_view\[2\] names bank 1.*learning_rate 1 is too large.*DV_ERR_STATE"):
        eng.ibank_train_u8(d["views"][:4], [0, 2, 1, 0])
    with pytest.raises(N.EngineError, match=r"bank_of_member\[1\] names bank 1.*DV_ERR_STATE"):
        eng.ibank_step_batch_u8(planes, [2, 1])
    assert eng.inet_info()["views_trained"].tolist() == [d["F"]] * 3
    for b, w in zip((0, 2), before):
        same_bits(eng.ibank_read_weights(b), w, b)
    eng.ibank_set_weights(1, d["nets"][1]["w0"])                                          # finite weights heal the bank
    assert eng.inet_info()["finite"].all()
    res = eng.ibank_step_batch_u8(planes, [2, 1])
    begin_lone(lone, d["h"], d["w"], d["nets"][1])
    same_bits(lone.infomax_score_u8(planes[1]), res.angle_familiarity[1], "the healed bank")
    with pytest.raises(ValueError, match=r"weights must be float64\[24,256\]"):          # the bank's own shape
        eng.ibank_set_weights(1, d["nets"][0]["w0"])


# ---- 7. state: the bank-0 calls under a table, every way out of one, two engines ------------------------------------------------------------
def test_the_bank0_calls_are_refused_and_every_way_out_of_a_table_gives_todays_bits(eng, lone):
    d = HN.table_data()
    nets, of_bank, h, w = d["nets"], d["net_of_bank"], d["h"], d["w"]
    begin_lone(eng, h, w, nets[0])
    none = eng.inet_info()                                                                # a model, no table
    assert (none["n_nets"], none["n_banks"], none["bytes"]) == (0, 0, 0) and len(none["n_hidden"]) == 0 and len(none["finite"]) == 0
    got = train_table(eng, d)
    views, planes = d["views"], HN.step_data(9)["planes"]
    for call in (lambda: eng.infomax_train_u8(views), lambda: eng.infomax_score_u8(views), lambda: eng.infomax_step_batch_u8(planes),
                 lambda: eng.infomax_read_weights(), lambda: eng.infomax_set_weights(np.ones((1, 35)))):   # (the sensed ones: test 4)
        with pytest.raises(N.EngineError, match="dv_inet_clear.*DV_ERR_STATE"):
            call()
    for b in range(7):
        same_bits(eng.ibank_read_weights(b), got[b], b)
    # a refused table leaves the live one as it was
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(N._i32p)
    f64 = lambda a: N.f64ptr(np.ascontiguousarray(a, dtype=np.float64))
    w0 = np.concatenate([nets[0]["w0"].ravel(), nets[1]["w0"].ravel()])
    for rates, chans, of, msg in (([0.01, np.inf], [2, 2], [0], "network 1: learning_rate inf must be positive"),
                                  ([0.01, 0.02], [2, 3], [0], r"network 1: channel 3 outside \[0, 2\]"),
                                  ([0.01, 0.02], [2, 2], [0, 2], r"network_of_bank\[1\] = 2 outside \[0, n_nets = 2\)")):
        with pytest.raises(ValueError, match=msg):
            eng._check(eng._lib.dv_inet_set(eng._ctx, 2, i32([1, 3]), f64(rates), i32(chans), f64(w0), len(of), i32(of)), "dv_inet_set")
    with pytest.raises(ValueError, match=r"network 0: n_hidden 0 outside"):
        eng._check(eng._lib.dv_inet_set(eng._ctx, 1, i32([0]), f64([0.01]), i32([2]), f64(w0), 1, i32([0])), "dv_inet_set")
    assert eng.inet_info()["n_nets"] == 5
    for b in range(7):
        same_bits(eng.ibank_read_weights(b), got[b], b)
    # a second engine with another table: neither touches the other
    v = HN.vec_data()
    got_v = train_table(lone, v)
    assert (lone.inet_info()["n_nets"], eng.inet_info()["n_nets"]) == (3, 5)
    s = HN.step_data(9)
    res = eng.ibank_step_batch_u8(s["planes"], s["banks"])
    close(res.angle_familiarity, s["fam"], "beside another engine's table")
    for b in range(3):
        same_bits(lone.ibank_read_weights(b), got_v[b], b)
    # today's calls after a table: dv_ibank_set, dv_inet_clear, dv_infomax_begin and dv_infomax_end each drop it
    k = HB.bank_data("7x5_m1043")
    assert (k["h"], k["w"]) == (h, w)

    lay = HB.layout_data("7x5_m1043", 5, 13)

    def todays_bits(first=None):
        eng.ibank_set(HB.R, k["W0"])
        eng.ibank_train_u8(k["views"], k["bank_of"])
        out = [eng.ibank_read_weights(r) for r in range(HB.R)] + [eng.ibank_step_batch_u8(lay["planes"], lay["banks"]).angle_familiarity]
        out.append(eng.infomax_score_u8(k["patches"]))                                    # bank 0 again
        for r in range(HB.R):
            close(out[r], k["Ws"][r], "today's bank %d" % r)
        for a, b in zip(out, first or ()):
            same_bits(a, b, "after a table")
        return out

    eng.infomax_begin(h, w, k["W0"], 2, H.ETA)
    first = todays_bits()                                                                 # before any table of this model
    eng.inet_set(nets, of_bank)
    eng.ibank_set(HB.R, k["W0"])                                                          # dv_ibank_set drops the table
    assert eng.inet_info()["n_nets"] == 0 and eng.infomax_nets is None and eng.ibank_read_weights(1).shape == k["W0"].shape
    todays_bits(first)
    eng.inet_set(nets, of_bank)
    eng.inet_clear()                                                                      # one bank of the begin's network at its W0
    assert eng.inet_info()["n_nets"] == 0 and eng.ibank_info()["n_banks"] == 1 and eng.ibank_info()["views_trained"].tolist() == [0]
    same_bits(eng.infomax_read_weights(), k["W0"], "the begin's W0")
    todays_bits(first)
    eng.inet_set(nets, of_bank)
    eng.infomax_begin(h, w, k["W0"], 2, H.ETA)                                            # dv_infomax_begin drops it too
    assert eng.inet_info()["n_nets"] == 0 and eng.infomax_banks == 1
    todays_bits(first)
    eng.inet_set(nets, of_bank)
    eng.infomax_end()
    assert eng.inet_info()["n_nets"] == 0
    with pytest.raises(N.EngineError, match="DV_ERR_STATE"):                              # no model: no table
        eng.inet_set(nets, of_bank)


# ---- 8. landscape, sensor and network differ at once: the ensemble on a landscape set with a sensor table --------------------------------
AGENT_MODEL = dict(learning_rate=1e-3, seed=9, n_hidden=40)
SET_NETWORKS = (None, dict(n_hidden=70, learning_rate=2e-3, seed=11), dict(n_hidden=70, learning_rate=2e-3, seed=11), None)


def set_agent(land, model=None, **config):
    return navsim_amd.NavBySceneFamiliarity(np.array(land), HL.ENS_SENSOR, 1.0, n_test_angles=9, use_gpu_sensor=True,
                                            familiarity_model=infomax_familiarity(**dict(AGENT_MODEL, **(model or {}))),
                                            **dict(HSN.ENS_AGENT, **config))


def step_together(ens, alone, steps):
    for t in range(steps):
        ens.step_forward()
        for a in alone:
            if a.stopped_with_exception is None:
                try:
                    a.step_forward()
                except navsim_amd.StopNavigationException as stop:
                    a.stopped_with_exception = stop
        for i, (m, a) in enumerate(zip(ens.agents, alone)):
            assert m.position == a.position and m.angle == a.angle, (t, i)
            same_bits(m.angle_familiarity, a.angle_familiarity, (t, i))
            code = a.stopped_with_exception.get_code() if a.stopped_with_exception is not None else 0
            assert ens.stop_status[i] == code, (t, i)
            assert m.navigation_error == a.navigation_error and m.percent_recapitulated == a.percent_recapitulated, (t, i)


def test_banks_that_differ_in_landscape_sensor_and_network_equal_lone_agents():
    landscapes = HL.lands()[:2]
    routes = HL.ens_routes()[:4]                                                          # two routes on each of the two landscapes
    starts = HL.ens_starts(routes)
    ens = navsim_amd.InfomaxRouteEnsemble.from_landscapes(set_agent(landscapes[0]), list(landscapes), routes, starts, metrics="device",
                                                          sensors=list(HSN.ENS_SENSORS[:2]), networks=list(SET_NETWORKS))
    alone = []
    for r, pos, ang in starts:
        l, path = routes[r]
        a = set_agent(landscapes[l], SET_NETWORKS[r], **HSN.ens_config(l))
        a.train_from_path(path)
        a.position, a.angle = pos, ang
        alone.append(a)
    try:
        e = ens.engine
        assert e.n_sensors == 2 and e.n_lands == 2 and e.inet_info()["n_nets"] == 2      # routes 1 and 2 share a network, on two landscapes
        info = ens.bank_info()
        assert info["network_of_bank"].tolist() == [0, 1, 1, 0] and info["n_hidden"].tolist() == [40, 70, 70, 40]
        assert info["learning_rate"].tolist() == [1e-3, 2e-3, 2e-3, 1e-3] and info["finite"].all()
        for r in range(4):
            one = alone[2 * r]._engine
            same_bits(e.ibank_read_weights(r), one.infomax_read_weights(), r)
            assert info["views_trained"][r] == one.infomax_info()["views_trained"], r
        for m, a in zip(ens.agents, alone):
            assert m.network_index == info["network_of_bank"][m.memory_bank] and m.network["n_hidden"] == info["n_hidden"][m.memory_bank]
            assert np.array_equal(m.familiar_scenes, a.familiar_scenes)
        step_together(ens, alone, 8)
        print("after 8 steps: stop_status %r" % (ens.stop_status,))
        assert any(m.position != s[1] for m, s in zip(ens.agents, starts))
    finally:
        ens.agents[0].clear_training()
        ens.engine.close()
        for a in alone:
            a.clear_training()
            a._engine.close()


# ---- 9. InfomaxRouteEnsemble.from_routes_with(networks=...) under run_ensemble ---------------------------------------------------------------
ROUTE_NETWORKS = (None, dict(learning_rate=2e-3), dict(n_hidden=70, seed=7))


def route_agent(model=None):
    return navsim_amd.NavBySceneFamiliarity(synth.synth_landscape(3, 300, 4), HB.ENSEMBLE_SENSOR, 1.0, n_test_angles=9, use_gpu_sensor=True,
                                            familiarity_model=infomax_familiarity(**dict(HB.ENSEMBLE_MODEL, **(model or {}))))


def _csv(rows):
    out = io.StringIO()
    w = csv.DictWriter(out, fieldnames=sorted(rows[0]))
    w.writeheader()
    w.writerows(rows)
    return out.getvalue()


def test_run_ensemble_rows_equal_lone_run_experiment_rows_of_each_members_network():
    paths = HB.routes()
    starts = HB.starts(paths)
    ens = navsim_amd.InfomaxRouteEnsemble.from_routes_with(route_agent(), paths, starts, metrics="device", networks=list(ROUTE_NETWORKS))
    try:
        assert len(ens.agents) == 6 and ens.engine.inet_info()["n_nets"] == 3
        assert [a.network_index for a in ens.agents] == [0, 0, 1, 1, 2, 2]
        assert ens.agents[4].network == dict(channel=2, n_hidden=70, learning_rate=1e-3, seed=7)
        info = ens.bank_info()
        assert info["n_hidden"].tolist() == [256, 256, 70] and info["learning_rate"].tolist() == [1e-3, 2e-3, 1e-3]
        assert info["network_of_bank"].tolist() == [0, 1, 2] and info["views_trained"].tolist() == list(HB.ROUTE_POINTS)
        rows = navsim_amd.run_ensemble(ens, frames=40)
    finally:
        ens.agents[0].clear_training()
        ens.engine.close()
    wants = []
    for r, pos, ang in starts:
        a = route_agent(ROUTE_NETWORKS[r])
        try:
            a.train_from_path(paths[r])
            a.position, a.angle = pos, ang
            wants.append(navsim_amd.run_experiment(a, frames=40))
        finally:
            a.clear_training()
            a._engine.close()
    print("completed_frames %r stop_status %r" % ([r["completed_frames"] for r in rows], [r["stop_status"] for r in rows]))
    assert _csv(rows) == _csv(wants)


def test_without_networks_the_ensemble_makes_the_calls_it_made():
    paths = HB.routes()
    agent = route_agent()
    log = []
    e = agent._engine
    for name in ("ibank_set", "inet_set", "ibank_train_from_poses"):
        def note(*a, _inner=getattr(e, name), _name=name, **k):
            log.append(_name)
            return _inner(*a, **k)
        setattr(e, name, note)
    ens = navsim_amd.InfomaxRouteEnsemble.from_routes_with(agent, paths, HB.starts(paths), networks=None)
    try:
        assert log == ["ibank_set", "ibank_train_from_poses"] and e.inet_info()["n_nets"] == 0
        assert all(a.network_index is None and a.network is None for a in ens.agents)
        info = ens.bank_info()
        assert info["network_of_bank"].tolist() == [0, 0, 0] and info["n_hidden"].tolist() == [256] * 3
        assert info["learning_rate"].tolist() == [HB.ENSEMBLE_MODEL["learning_rate"]] * 3
    finally:
        ens.agents[0].clear_training()
        e.close()
