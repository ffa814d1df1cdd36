"""Landscape sets on the device (dv_lands_*): several landscapes resident together and a landscape per pose in the sensed calls of the
banked models.  Three oracles (tests/helpers_lands.py): the HOST sensor model on each pose's own landscape alone, the NumPy statements
of the two models on those views, and engines that hold ONE landscape each through set_landscape.  Everything integer is compared
with np.array_equal; Infomax weights and scores are bit-equal to the one-landscape engines (uint64 views) and within
helpers_infomax.TOL of the statement, the figure printed before it is asserted."""
import csv
import io

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import infomax_familiarity, mushroom_familiarity
from tests import helpers_infomax as HI
from tests import helpers_lands as HL
from tests import helpers_mushroom as H

pytestmark = pytest.mark.gpu

STATE, INVALID = -3, -1
MB_CASES = (("sq", 2, False), ("sq", 2, True), ("px", 0, False), ("px", 1, False), ("px", 2, False), ("odd", 2, False))
IM_CASES = (("sq", 2), ("px", 0), ("px", 1), ("px", 2), ("odd", 2))


def one_land_engine(name, land):
    """An engine that holds ONE landscape (set_landscape) and the sensor of `name`."""
    c = HL.SENSORS[name]
    e = navsim_amd.FamiliarityEngine(device=0)
    e.set_landscape(land)
    e.configure_sensor(c["sensor"], c["pixel"], HL.level_tables(name), c["mask"])
    return e


def set_engine(name, own=0):
    """... and, beside its one landscape, the four landscapes as a set."""
    e = one_land_engine(name, HL.lands()[own])
    e.lands_set(list(HL.lands()))
    return e


@pytest.fixture(scope="module")
def engines():
    """name -> (the engine with the set, [the one-landscape engine of every landscape]), made at first use."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = (set_engine(name), [one_land_engine(name, l) for l in HL.lands()])
        return made[name]
    yield get
    for e, ones in made.values():
        e.close()
        for o in ones:
            o.close()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    bad = np.argwhere(H.bits(a) != H.bits(b))
    assert len(bad) == 0, (bad[:6].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


def rel(got, want):
    return float(np.max(np.abs(np.asarray(got) - want)) / np.max(np.abs(want)))


# ---- 1. lands_sense ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HL.SENSORS))
def test_lands_sense_is_the_host_model_on_each_poses_own_landscape(engines, name):
    e, ones = engines(name)
    info = e.lands_info()
    assert info["n_lands"] == 4 and info["shapes"] == [l.shape[:2] for l in HL.lands()] and info["bytes"] == sum(l.size for l in HL.lands())
    s = HL.sense_case(name)
    got = e.lands_sense(s["x"], s["y"], s["angle"], s["land_of"])
    assert got.dtype == np.uint8 and np.array_equal(got, s["scenes"])
    for l in range(4):                                                                    # ... and the one-landscape engine's dv_sense
        m = s["land_of"] == l
        assert np.array_equal(got[m], ones[l].sense(s["x"][m], s["y"][m], s["angle"][m])), l
    x, y, a = HL.ON_L2_OFF_L1
    assert np.array_equal(e.lands_sense([x], [y], [a], [2])[0], HL.host_scene(name, x, y, a, 2))
    with pytest.raises(IndexError, match="pose 1 .*landscape 1 .211 x 173"):
        e.lands_sense([s["x"][0], x, x], [s["y"][0], y, y], [0.1, a, a], [0, 1, 1])
    assert np.array_equal(e.lands_sense(s["x"], s["y"], s["angle"], s["land_of"]), s["scenes"])


def test_a_negative_index_wraps_by_the_poses_own_rows_and_columns(engines):
    """A negative column on the 211 x 173 landscape and a negative row on the 173 x 260 one, in one call with the same poses on L0."""
    e, _ = engines("sq")
    (xc, yc, ac), lc = HL.WRAPS["cols"]
    (xr, yr, ar), lr = HL.WRAPS["rows"]
    cols, rows = HL.wrap_facts("cols"), HL.wrap_facts("rows")
    got = e.lands_sense([xc, xc, xr, xr, xc], [yc, yc, yr, yr, yc], [ac, ac, ar, ar, ac], [lc, 0, lr, 0, lc])
    assert np.array_equal(got[0], cols) and np.array_equal(got[4], cols) and np.array_equal(got[2], rows)
    assert np.array_equal(got[1], HL.host_scene("sq", xc, yc, ac, 0)) and not np.array_equal(got[0], got[1])
    assert np.array_equal(got[3], HL.host_scene("sq", xr, yr, ar, 0)) and not np.array_equal(got[2], got[3])


# ---- 2. the mushroom-body model ------------------------------------------------------------------------------------------------------------
def mb_begin(e, name, channel, wide, wts=None):
    conn, n_active, _ = HL.mb_banks(name, channel, wide)
    w, h = HL.SENSORS[name]["sensor"]
    e.mb_begin(h, w, conn, n_active, channel)
    e.mbank_set(HL.N_BANKS)
    if wts is not None:
        for r, wt in enumerate(wts):
            e.mbank_set_weights(r, wt)


@pytest.mark.parametrize("name,channel,wide", MB_CASES)
def test_mushroom_routes_on_three_landscapes_train_in_one_call(engines, name, channel, wide):
    e, ones = engines(name)
    t = HL.train_case(name)
    _, _, wts = HL.mb_banks(name, channel, wide)
    mb_begin(e, name, channel, wide)
    views = e.mbank_train_from_poses(t["x"], t["y"], t["angle"], t["bank_of"], land_of_view=t["land_of"])
    assert np.array_equal(views, t["scenes"])                                            # the host model, byte for byte
    got = e.mbank_read_weights()
    assert np.array_equal(got, wts)                                                       # the statement
    assert e.mbank_info()["views_trained"].tolist() == list(HL.ROUTE_POINTS)
    for r in range(3):                                                                    # an engine that trained that route alone on that landscape alone
        o = ones[HL.ROUTE_LANDS[r]]
        conn, n_active, _ = HL.mb_banks(name, channel, wide)
        o.mb_begin(views.shape[1], views.shape[2], conn, n_active, channel)
        i = t["first"][r]
        assert np.array_equal(o.mb_train_from_poses(t["x"][i], t["y"][i], t["angle"][i]), views[i])
        assert np.array_equal(o.mb_read_weights(), got[r]), r
    # one view off its own landscape (though on two others): IndexError, and every bank as it was
    v, x, y = HL.off_own_landscape_view(name)
    xs, ys = t["x"].copy(), t["y"].copy()
    xs[v], ys[v] = x, y
    with pytest.raises(IndexError, match="pose %d " % v):                                # (on the trained banks ...
        e.mbank_train_from_poses(xs, ys, t["angle"], t["bank_of"], land_of_view=t["land_of"])
    assert np.array_equal(e.mbank_read_weights(), got) and e.mbank_info()["views_trained"].tolist() == list(HL.ROUTE_POINTS)
    mb_begin(e, name, channel, wide)                                                      # ... and on fresh ones, where any training shows)
    with pytest.raises(IndexError, match="pose %d " % v):
        e.mbank_train_from_poses(xs, ys, t["angle"], t["bank_of"], land_of_view=t["land_of"])
    assert np.array_equal(e.mbank_read_weights(), np.ones_like(wts)) and e.mbank_info()["views_trained"].tolist() == [0, 0, 0]


def mb_check_step(e, ones, name, channel, wide, case):
    want = HL.mb_statement(name, channel, case, wide)
    res = e.mbank_sense_step_batch(case["xs"], case["ys"], case["angs"], case["banks"], land_of_member=case["lands"])
    assert not res.flags.any()
    same_bits(res.angle_familiarity, want)
    assert res.best_idex.tolist() == np.argmax(want, axis=1).tolist()
    for l in range(4):                                                                    # the one-landscape engine of that landscape and bank
        m = np.flatnonzero(case["lands"] == l)
        if len(m):
            one = ones[l].mbank_sense_step_batch(case["xs"][m], case["ys"][m], case["angs"][m], case["banks"][m])
            same_bits(res.angle_familiarity[m], one.angle_familiarity)
            assert res.best_idex[m].tolist() == one.best_idex.tolist()
    return res


@pytest.mark.parametrize("name,channel,wide", MB_CASES)
def test_mushroom_members_step_on_their_own_landscapes(engines, name, channel, wide):
    e, ones = engines(name)
    _, _, wts = HL.mb_banks(name, channel, wide)
    for eng in [e] + ones:
        mb_begin(eng, name, channel, wide, wts)
    for n, A in (HL.LAYOUTS if name == "sq" else ((5, 13),)):
        case = HL.step_case(name, n, A)
        res = mb_check_step(e, ones, name, channel, wide, case)
        if n > 1:                                                                         # permuting the members permutes the rows
            perm = np.random.default_rng(n * 100 + A).permutation(n)
            res2 = e.mbank_sense_step_batch(case["xs"][perm], case["ys"][perm], case["angs"][perm], case["banks"][perm],
                                            land_of_member=case["lands"][perm])
            same_bits(res2.angle_familiarity, res.angle_familiarity[perm])
            assert res2.best_idex.tolist() == res.best_idex[perm].tolist()
    assert np.array_equal(e.mbank_read_weights(), wts)


def test_mushroom_columns_past_the_launch_edge_keep_their_members_landscape(engines):
    """683 members x 12 headings = 8196 columns: the second launch begins inside member 682, whose landscape is not member 0's."""
    e, ones = engines("sq")
    _, _, wts = HL.mb_banks("sq", 2)
    for eng in [e] + ones:
        mb_begin(eng, "sq", 2, False, wts)
    mb_check_step(e, ones, "sq", 2, False, HL.step_case("sq", *HL.WIDE_LAYOUT))


def test_mushroom_training_past_8192_views_keeps_the_tables_in_step(engines):
    """8193 views in one call: view 8192, alone in the second training launch, is the only view of route 1 (landscape 1, bank 1); the
    others repeat two views of route 0.  Bank 1 is what route 1's view alone gives, bank 0 what the two views give."""
    e, _ = engines("sq")
    t = HL.train_case("sq")
    conn, n_active, _ = HL.mb_banks("sq", 2)
    n = 8193
    i0, i1 = t["first"][0][:2], t["first"][1][0]
    pick = np.concatenate([np.tile(i0, n // 2), [i1]])
    assert len(pick) == n and t["land_of"][i1] == 1
    mb_begin(e, "sq", 2, False)
    views = e.mbank_train_from_poses(t["x"][pick], t["y"][pick], t["angle"][pick], t["bank_of"][pick], land_of_view=t["land_of"][pick])
    assert np.array_equal(views[-1], t["scenes"][i1]) and np.array_equal(views[:2], t["scenes"][i0])
    ones = np.ones(HL.MB["n_kc"], np.uint8)
    want = np.stack([H.train(ones, t["scenes"][i0][..., 2], conn, n_active), H.train(ones, t["scenes"][i1:i1 + 1][..., 2], conn, n_active), ones])
    assert np.array_equal(e.mbank_read_weights(), want) and e.mbank_info()["views_trained"].tolist() == [8192, 1, 0]


def test_a_mushroom_member_off_its_own_landscape_is_flagged_and_its_neighbours_are_not(engines):
    e, ones = engines("sq")
    _, _, wts = HL.mb_banks("sq", 2)
    mb_begin(e, "sq", 2, False, wts)
    case = HL.step_case("sq", 5, 13)
    want = HL.mb_statement("sq", 2, case)
    xs, ys, land_of = HL.flag_case("sq")
    res = e.mbank_sense_step_batch(xs, ys, case["angs"], case["banks"], land_of_member=land_of)
    assert res.flags.tolist() == [0, 0, HL.SENSE_ERROR, 0, 0] and res.best_idex[2] == -1
    keep = [0, 1, 3, 4]
    same_bits(res.angle_familiarity[keep], want[keep])
    assert res.best_idex[keep].tolist() == np.argmax(want, axis=1)[keep].tolist()
    land_of[2] = 2                                                                        # the same place on the wide landscape: sensed
    assert not e.mbank_sense_step_batch(xs, ys, case["angs"], case["banks"], land_of_member=land_of).flags.any()


# ---- 3. the Infomax model ------------------------------------------------------------------------------------------------------------------
def im_begin(e, name, channel, Ws=None):
    W0, _ = HL.im_banks(name, channel)
    w, h = HL.SENSORS[name]["sensor"]
    e.infomax_begin(h, w, W0, channel=channel, learning_rate=HL.IM["eta"])
    e.ibank_set(HL.N_BANKS, W0)
    if Ws is not None:
        for r, W in enumerate(Ws):
            e.ibank_set_weights(r, W)


@pytest.mark.parametrize("name,channel", IM_CASES)
def test_infomax_routes_on_three_landscapes_train_in_one_call(engines, name, channel):
    e, ones = engines(name)
    t = HL.train_case(name)
    W0, Ws = HL.im_banks(name, channel)
    im_begin(e, name, channel)
    views = e.ibank_train_from_poses(t["x"], t["y"], t["angle"], t["bank_of"], land_of_view=t["land_of"])
    assert np.array_equal(views, t["scenes"])
    got = np.stack([e.ibank_read_weights(r) for r in range(3)])
    worst = max(rel(got[r], Ws[r]) for r in range(3))
    print("lands, infomax weights %s ch %d: relative error %.3e (bound %.1e)" % (name, channel, worst, HI.TOL))
    assert worst <= HI.TOL
    for r in range(3):
        o = ones[HL.ROUTE_LANDS[r]]
        o.infomax_begin(views.shape[1], views.shape[2], W0, channel=channel, learning_rate=HL.IM["eta"])
        i = t["first"][r]
        o.infomax_train_from_poses(t["x"][i], t["y"][i], t["angle"][i])
        same_bits(o.infomax_read_weights(), got[r])
    v, x, y = HL.off_own_landscape_view(name)
    xs, ys = t["x"].copy(), t["y"].copy()
    xs[v], ys[v] = x, y
    with pytest.raises(IndexError, match="pose %d " % v):
        e.ibank_train_from_poses(xs, ys, t["angle"], t["bank_of"], land_of_view=t["land_of"])
    for r in range(3):
        same_bits(e.ibank_read_weights(r), got[r])
    assert e.ibank_info()["views_trained"].tolist() == list(HL.ROUTE_POINTS)


def im_check_step(e, ones, name, channel, case):
    want = HL.im_statement(name, channel, case)
    res = e.ibank_sense_step_batch(case["xs"], case["ys"], case["angs"], case["banks"], land_of_member=case["lands"])
    assert not res.flags.any()
    err = rel(res.angle_familiarity, want)
    print("lands, infomax scores %s ch %d %dx%d: relative error %.3e (bound %.1e)" % ((name, channel) + want.shape + (err, HI.TOL)))
    assert err <= HI.TOL
    for l in range(4):
        m = np.flatnonzero(case["lands"] == l)
        if len(m):
            one = ones[l].ibank_sense_step_batch(case["xs"][m], case["ys"][m], case["angs"][m], case["banks"][m])
            same_bits(res.angle_familiarity[m], one.angle_familiarity)
            assert res.best_idex[m].tolist() == one.best_idex.tolist()
    return res


@pytest.mark.parametrize("name,channel", IM_CASES)
def test_infomax_members_step_on_their_own_landscapes(engines, name, channel):
    e, ones = engines(name)
    _, Ws = HL.im_banks(name, channel)
    for eng in [e] + ones:
        im_begin(eng, name, channel, Ws)
    for n, A in (HL.LAYOUTS if name == "sq" else ((5, 13),)):
        case = HL.step_case(name, n, A)
        res = im_check_step(e, ones, name, channel, case)
        if n > 1:
            perm = np.random.default_rng(n * 100 + A).permutation(n)
            res2 = e.ibank_sense_step_batch(case["xs"][perm], case["ys"][perm], case["angs"][perm], case["banks"][perm],
                                            land_of_member=case["lands"][perm])
            same_bits(res2.angle_familiarity, res.angle_familiarity[perm])
            assert res2.best_idex.tolist() == res.best_idex[perm].tolist()


def test_infomax_columns_past_the_slab_edge_keep_their_members_landscape(engines):
    e, ones = engines("sq")
    _, Ws = HL.im_banks("sq", 2)
    for eng in [e] + ones:
        im_begin(eng, "sq", 2, Ws)
    im_check_step(e, ones, "sq", 2, HL.step_case("sq", *HL.WIDE_LAYOUT))


def test_an_infomax_member_off_its_own_landscape_is_flagged_and_its_neighbours_are_not(engines):
    e, ones = engines("sq")
    _, Ws = HL.im_banks("sq", 2)
    im_begin(e, "sq", 2, Ws)
    case = HL.step_case("sq", 5, 13)
    clean = e.ibank_sense_step_batch(case["xs"], case["ys"], case["angs"], case["banks"], land_of_member=case["lands"])
    xs, ys, land_of = HL.flag_case("sq")
    res = e.ibank_sense_step_batch(xs, ys, case["angs"], case["banks"], land_of_member=land_of)
    assert res.flags.tolist() == [0, 0, HL.SENSE_ERROR, 0, 0] and res.best_idex[2] == -1
    keep = [0, 1, 3, 4]
    same_bits(res.angle_familiarity[keep], clean.angle_familiarity[keep])
    assert res.best_idex[keep].tolist() == clean.best_idex[keep].tolist()


# ---- 4. state --------------------------------------------------------------------------------------------------------------------------------
def test_refused_tables_leave_the_set_the_banks_and_the_buffers_as_they_were(engines):
    e, _ = engines("sq")
    _, _, wts = HL.mb_banks("sq", 2)
    mb_begin(e, "sq", 2, False, wts)
    case = HL.step_case("sq", 5, 13)
    before = e.mbank_sense_step_batch(case["xs"], case["ys"], case["angs"], case["banks"], land_of_member=case["lands"])
    t = HL.train_case("sq")
    n = len(t["x"])
    for bad in ([0, 1, -1, 0, 0], [0, 1, 4, 0, 0], [0, 1, 2], np.zeros(5)):
        with pytest.raises(ValueError):
            e.mbank_sense_step_batch(case["xs"], case["ys"], case["angs"], case["banks"], land_of_member=bad)
    with pytest.raises(ValueError):
        e.mbank_train_from_poses(t["x"], t["y"], t["angle"], t["bank_of"], land_of_view=[4] * n)
    # past the Python-side check: the library's own, before anything reaches the device
    lib, ctx = e._lib, e._ctx
    fam, best, flags = np.empty((5, 13)), np.empty(5, np.int32), np.empty(5, np.uint32)
    for entry in (-1, 4):
        tab = np.array([0, 1, entry, 0, 0], dtype=np.int32)
        rc = lib.dv_lands_mbank_sense_step(ctx, N.f64ptr(case["xs"]), N.f64ptr(case["ys"]), N.f64ptr(np.ascontiguousarray(case["angs"])), 5, 13,
                                           case["banks"].ctypes.data_as(N._i32p), tab.ctypes.data_as(N._i32p), N.f64ptr(fam),
                                           best.ctypes.data_as(N._i32p), flags.ctypes.data_as(N._u32p))
        assert rc == INVALID and ("land_of_member[2] = %d" % entry) in lib.dv_last_error(ctx).decode()
        out = np.empty((n,) + t["scenes"].shape[1:], np.uint8)
        tabv = np.full(n, entry, dtype=np.int32)
        rc = lib.dv_lands_mbank_train_from_poses(ctx, N.f64ptr(t["x"]), N.f64ptr(t["y"]), N.f64ptr(t["angle"]), n, t["bank_of"].ctypes.data_as(N._i32p),
                                                 tabv.ctypes.data_as(N._i32p), N.u8ptr(out))
        assert rc == INVALID and "land_of_view[0]" in lib.dv_last_error(ctx).decode()
    assert np.array_equal(e.mbank_read_weights(), wts) and e.lands_info()["n_lands"] == 4
    after = e.mbank_sense_step_batch(case["xs"], case["ys"], case["angs"], case["banks"], land_of_member=case["lands"])
    same_bits(after.angle_familiarity, before.angle_familiarity)


@pytest.mark.parametrize("model", ("mushroom", "infomax"))
def test_the_bank_table_and_the_landscape_table_change_apart(engines, model):
    """A set of two landscapes, five members: a step, a step with the same land_of_member under other banks, then a step with the same
    bank_of_member on other landscapes.  Each table is kept on the device by its own record (and Infomax sends the landscapes in bank
    order, so its landscape table changes with the banks).  Every row is the one-landscape engine's of that landscape and bank."""
    _, ones = engines("sq")
    case = HL.step_case("sq", 5, 13)
    xs, ys, angs = case["xs"], case["ys"], case["angs"]
    if model == "mushroom":
        begin, step = (lambda eng: mb_begin(eng, "sq", 2, False, HL.mb_banks("sq", 2)[2])), "mbank_sense_step_batch"
    else:
        begin, step = (lambda eng: im_begin(eng, "sq", 2, HL.im_banks("sq", 2)[1])), "ibank_sense_step_batch"
    lands_a, lands_b = np.array([0, 1, 1, 0, 1], np.int32), np.array([1, 0, 1, 1, 0], np.int32)
    banks_p, banks_q = np.array([1, 0, 2, 0, 1], np.int32), np.array([2, 2, 0, 1, 0], np.int32)
    e = one_land_engine("sq", HL.lands()[0])
    try:
        e.lands_set(list(HL.lands()[:2]))
        for eng in [e] + ones[:2]:
            begin(eng)
        rows = []
        for lands, banks in ((lands_a, banks_p), (lands_a, banks_q), (lands_b, banks_q)):
            want = np.empty((5, 13))
            for l in range(2):
                m = np.flatnonzero(lands == l)
                want[m] = getattr(ones[l], step)(xs[m], ys[m], angs[m], banks[m]).angle_familiarity
            res = getattr(e, step)(xs, ys, angs, banks.copy(), land_of_member=lands.copy())
            assert not res.flags.any()
            same_bits(res.angle_familiarity, want)
            assert res.best_idex.tolist() == np.argmax(want, axis=1).tolist()
            rows.append(want)
        # a table left over from the step before would show: every member whose entry changed has another row
        assert all(not np.array_equal(rows[0][i], rows[1][i]) for i in np.flatnonzero(banks_p != banks_q))
        assert all(not np.array_equal(rows[1][i], rows[2][i]) for i in np.flatnonzero(lands_a != lands_b))
    finally:
        e.close()


def test_the_one_landscape_calls_keep_their_bits_beside_a_set_and_after_it_is_cleared():
    name = "sq"
    plain = one_land_engine(name, HL.lands()[0])
    e = set_engine(name)
    try:
        _, _, wts = HL.mb_banks(name, 2)
        s = HL.sense_case(name)
        case = HL.step_case(name, 5, 13)
        for eng in (plain, e):
            mb_begin(eng, name, 2, False, wts)
        want_sense = plain.sense(s["x"], s["y"], s["angle"])
        want_step = plain.mb_sense_step_batch(case["xs"], case["ys"], case["angs"])
        want_bank = plain.mbank_sense_step_batch(case["xs"], case["ys"], case["angs"], case["banks"])

        def check():
            assert np.array_equal(e.sense(s["x"], s["y"], s["angle"]), want_sense)
            got = e.mb_sense_step_batch(case["xs"], case["ys"], case["angs"])
            same_bits(got.angle_familiarity, want_step.angle_familiarity)
            assert got.best_idex.tolist() == want_step.best_idex.tolist()
            same_bits(e.mbank_sense_step_batch(case["xs"], case["ys"], case["angs"], case["banks"]).angle_familiarity, want_bank.angle_familiarity)
        check()
        e.mbank_sense_step_batch(case["xs"], case["ys"], case["angs"], case["banks"], land_of_member=case["lands"])
        check()
        # the set again, with other shapes and another order: the tables now name other landscapes
        L = HL.lands()
        e.lands_set([L[2], L[1]])
        assert e.lands_info()["shapes"] == [(173, 260), (211, 173)]
        got = e.lands_sense(s["x"][:2], s["y"][:2], s["angle"][:2], [0, 1])
        assert np.array_equal(got[0], HL.host_scene(name, s["x"][0], s["y"][0], s["angle"][0], 2))
        assert np.array_equal(got[1], HL.host_scene(name, s["x"][1], s["y"][1], s["angle"][1], 1))
        with pytest.raises(ValueError, match="n_lands = 2"):
            e.lands_sense(s["x"][:2], s["y"][:2], s["angle"][:2], [0, 2])
        e.set_landscape(L[0])                                                             # a new one landscape leaves the set alone
        e.mb_end()
        assert e.lands_info()["n_lands"] == 2
        mb_begin(e, name, 2, False, wts)
        check()
        e.lands_clear()
        assert e.lands_info() == dict(n_lands=0, shapes=[], bytes=0)
        check()
        with pytest.raises(N.EngineError, match="lands_set first"):
            e.lands_sense(s["x"][:2], s["y"][:2], s["angle"][:2], [0, 0])
        tab = np.zeros(2, dtype=np.int32)
        out = np.empty((2, 32, 32, 3), np.uint8)
        assert e._lib.dv_lands_sense(e._ctx, N.f64ptr(s["x"]), N.f64ptr(s["y"]), N.f64ptr(s["angle"]), tab.ctypes.data_as(N._i32p), 2,
                                     N.u8ptr(out)) == STATE
    finally:
        plain.close()
        e.close()


def test_two_engines_with_different_sets_used_in_turn():
    L = HL.lands()
    a, b = one_land_engine("sq", L[0]), one_land_engine("sq", L[0])
    try:
        a.lands_set([L[0], L[1]])
        b.lands_set([L[1], L[2], L[0]])
        s = HL.sense_case("sq")
        x, y, ang = s["x"][:3], s["y"][:3], s["angle"][:3]
        for _ in range(2):
            ga, gb = a.lands_sense(x, y, ang, [1, 0, 1]), b.lands_sense(x, y, ang, [1, 0, 1])
            assert np.array_equal(ga, HL.host_scenes("sq", x, y, ang, [1, 0, 1]))
            assert np.array_equal(gb, HL.host_scenes("sq", x, y, ang, [2, 1, 2]))
    finally:
        a.close()
        b.close()


# ---- 5. the ensembles ------------------------------------------------------------------------------------------------------------------------
MODELS = {
    "mushroom": (lambda: mushroom_familiarity(n_kc=1043, fan_in=8, sparsity=0.02, seed=6), "MushroomRouteEnsemble", "mbank_sense_step_batch"),
    "infomax": (lambda: infomax_familiarity(learning_rate=1e-3, seed=9, n_hidden=18), "InfomaxRouteEnsemble", "ibank_sense_step_batch"),
}


def make_agent(model, land):
    return navsim_amd.NavBySceneFamiliarity(np.array(land), HL.ENS_SENSOR, 1.0, n_test_angles=9, use_gpu_sensor=True,
                                            familiarity_model=MODELS[model][0]())


def lone_agents(model, landscapes, routes, starts):
    """Every member's twin: an agent on an engine of its own, with its own landscape alone, trained on its route alone."""
    out = []
    for r, pos, ang in starts:
        l, path = routes[r]
        a = make_agent(model, landscapes[l])
        a.train_from_path(path)
        a.position, a.angle = pos, ang
        out.append(a)
    return out


@pytest.mark.parametrize("model", sorted(MODELS))
def test_an_agents_own_steps_keep_their_bits_beside_a_live_set_and_after_it_is_cleared(model):
    """Two agents trained alike walk from the same start, step for step.  One engine never holds a set; the other gets one after three
    steps, a step with a landscape per member on it after six, and loses it after nine: the lone steps (dv_mb_sense_step /
    dv_infomax_sense_step on the engine's one landscape) agree throughout, in position, heading and the bits of angle_familiarity."""
    L = HL.lands()
    _, path = HL.ens_routes()[0]
    _, pos, ang = HL.ens_starts(HL.ens_routes())[1]
    plain, agent = make_agent(model, L[0]), make_agent(model, L[0])
    try:
        for a in (plain, agent):
            a.train_from_path(path)
            a.position, a.angle = pos, ang
        eng = agent._engine
        xs, ys = np.array([pos[0], pos[0] + 2.0]), np.array([pos[1], pos[1] - 1.5])
        angs = (np.array([ang, ang + 0.4])[:, None] + agent.angle_offsets[None, :]) % (2 * np.pi)
        seen = set()

        def between(stage):
            if stage == 1:
                eng.lands_set([L[1], L[2], L[0]])
            elif stage == 2:
                res = getattr(eng, MODELS[model][2])(xs, ys, angs, [0, 0], land_of_member=[0, 1])
                one = getattr(eng, MODELS[model][2])(xs, ys, angs, [0, 0])                # (the same poses on the engine's one landscape)
                assert not res.flags.any() and not np.array_equal(res.angle_familiarity, one.angle_familiarity)
            elif stage == 3:
                eng.lands_clear()
            assert eng.lands_info()["n_lands"] == (3 if stage in (1, 2) else 0)

        for stage in range(4):
            between(stage)
            for t in range(3):
                plain.step_forward()
                agent.step_forward()
                assert agent.position == plain.position and agent.angle == plain.angle, (stage, t)
                assert np.array_equal(H.bits(agent.angle_familiarity), H.bits(plain.angle_familiarity)), (stage, t)
                assert agent.navigation_error == plain.navigation_error, (stage, t)
                seen.update(agent.angle_familiarity.tolist())
        assert len(seen) > 12 and agent.position != pos
    finally:
        for a in (plain, agent):
            a.clear_training()
            a._engine.close()


@pytest.mark.parametrize("metrics", ("host", "device"))
@pytest.mark.parametrize("shapes", ("mixed", "same"))
@pytest.mark.parametrize("model", sorted(MODELS))
def test_ensemble_members_equal_lone_agents_on_their_own_landscapes(model, shapes, metrics):
    landscapes = HL.lands()[:3] if shapes == "mixed" else HL.same_shape_lands()
    routes = HL.ens_routes()
    starts = HL.ens_starts(routes)
    cls = getattr(navsim_amd, MODELS[model][1])
    ens = cls.from_landscapes(make_agent(model, landscapes[0]), list(landscapes), routes, starts, metrics=metrics)
    alone = lone_agents(model, landscapes, routes, starts)
    calls = []
    inner = getattr(ens.engine, MODELS[model][2])

    def counted(*a, **k):
        calls.append((list(a[3]), list(k["land_of_member"])))
        return inner(*a, **k)
    setattr(ens.engine, MODELS[model][2], counted)
    try:
        assert ens._uniform == (shapes == "same")
        assert [a.memory_bank for a in ens.agents] == [r for r, _, _ in starts]
        assert [a.landscape_index for a in ens.agents] == [routes[r][0] for r, _, _ in starts]
        for m, a in zip(ens.agents, alone):
            assert m.landscape is landscapes[m.landscape_index] and m._bounds_tuple() == a._bounds_tuple()
            assert np.array_equal(m.training_path, a.training_path) and m.training_path_length == a.training_path_length
            assert np.array_equal(m.familiar_scenes, a.familiar_scenes)
        with pytest.raises(ValueError, match=MODELS[model][1]):
            ens.agents[1].step_forward()
        with pytest.raises(ValueError):
            navsim_amd.NavEnsemble(ens.agents)
        for t in range(15):
            before = list(ens.active)
            ens.step_forward()
            assert len(calls) == t + 1                                                    # ONE device call a step
            assert calls[-1] == ([ens.agents[i].memory_bank for i in before], [ens.agents[i].landscape_index for i in before])
            for a in alone:
                if a.stopped_with_exception is None:
                    try:
                        a.step_forward()
                    except navsim_amd.StopNavigationException as stop:
                        a.stopped_with_exception = stop
            for i, (m, a) in enumerate(zip(ens.agents, alone)):
                assert m.position == a.position and m.angle == a.angle, (t, i)
                assert np.array_equal(H.bits(m.angle_familiarity), H.bits(a.angle_familiarity)), (t, i)
                code = a.stopped_with_exception.get_code() if a.stopped_with_exception is not None else 0
                assert ens.stop_status[i] == code, (t, i)
                assert m.navigation_error == a.navigation_error and m.percent_recapitulated == a.percent_recapitulated, (t, i)
                assert np.array_equal(m._coverage_array, a._coverage_array), (t, i)
    finally:
        setattr(ens.engine, MODELS[model][2], inner)
        ens.agents[0].clear_training()
        for a in alone:
            a.clear_training()


def _csv(rows):
    out = io.StringIO()
    w = csv.DictWriter(out, fieldnames=sorted(rows[0]))
    w.writeheader()
    w.writerows(rows)
    return out.getvalue()


@pytest.mark.parametrize("model", sorted(MODELS))
def test_run_ensemble_rows_equal_lone_run_experiment_rows(model):
    landscapes = HL.lands()[:3]
    routes = HL.ens_routes()
    starts = HL.ens_starts(routes)
    ens = getattr(navsim_amd, MODELS[model][1]).from_landscapes(make_agent(model, landscapes[0]), list(landscapes), routes, starts)
    try:
        rows = navsim_amd.run_ensemble(ens)
    finally:
        ens.agents[0].clear_training()
    wants = []
    for a in lone_agents(model, landscapes, routes, starts):
        try:
            wants.append(navsim_amd.run_experiment(a))
        finally:
            a.clear_training()
    assert _csv(rows) == _csv(wants)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_a_member_past_the_edge_of_its_own_landscape_stops_and_the_others_go_on(model):
    """Three members at the same coordinates, past the bound of the 211 x 173 landscape and well inside the two 300 x 300 ones; a
    fourth on its route; a fifth inside the bounds of the 211 x 173 landscape where a corner of its footprint leaves it."""
    L = HL.lands()
    landscapes = [L[0], L[1], L[3]]
    HL.ens_facts(L)
    routes = [(l, path) for l, (_, path) in zip((0, 1, 2), HL.ens_routes()[:3])]
    pos, ang = HL.EDGE_START
    HL.footprint_facts()
    starts = [(0, pos, ang), (1, pos, ang), (2, pos, ang), (1, tuple(routes[1][1][3]), 0.8), (1,) + HL.FOOTPRINT_START]
    ens = getattr(navsim_amd, MODELS[model][1]).from_landscapes(make_agent(model, L[0]), landscapes, routes, starts)
    try:
        assert not ens._uniform
        ens.step_forward()
        assert ens.stop_status == [0, -2, 0, 0, -3]
        assert isinstance(ens.agents[1].stopped_with_exception, navsim_amd.OutOfLandscapeBoundsException)
        assert isinstance(ens.agents[4].stopped_with_exception, IndexError) and ens.agents[4].position == HL.FOOTPRINT_START[0]
        ens.step_forward()
        assert ens.stop_status == [0, -2, 0, 0, -3] and ens.agents[0].position != pos and ens.agents[1].position == pos
    finally:
        ens.agents[0].clear_training()
