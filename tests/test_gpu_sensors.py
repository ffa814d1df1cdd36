"""Sensor tables on the device (dv_sensors_*): a sensor configuration per landscape of the set, read per pose by the sensed calls that take
a landscape table.  Expected values never come from the device (tests/helpers_sensors.py): the HOST sensor model under each pose's own
entry on its own landscape alone, the NumPy statements of the two one-value models, and oracle.step for perfect memory.  Everything
integer is compared with np.array_equal; Infomax weights and scores are within helpers_infomax.TOL of the statement, the figure
printed before it is asserted, and bit-equal (uint64 views) to engines that hold that one sensor and that one route."""
import csv
import io

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import infomax_familiarity, mushroom_familiarity, sads_familiarity
from tests import helpers_infomax as HI
from tests import helpers_lands as HL
from tests import helpers_mushroom as H
from tests import helpers_mushroom_ensemble as HE
from tests import helpers_rviews as HR
from tests import helpers_sensors as HS

pytestmark = pytest.mark.gpu

STATE, INVALID = -3, -1
SHAPE_NAMES = sorted(HS.SHAPES)
CHEM = (0.25, 0.0, 1.0, 0.5, 0.3)                            # a perfect-memory member's weight: CHEM[i % 5]


def own_engine(shape, land):
    """An engine that holds ONE landscape (set_landscape) under the engine's OWN configuration, which is none of the entries."""
    c = HS.ENTRIES["OWN"]
    e = navsim_amd.FamiliarityEngine(device=0)
    e.set_landscape(land)
    e.configure_sensor(HS.SHAPES[shape], c["pixel"], HS.level_table(shape, "OWN"), c["mask"])
    return e


def entry_engine(shape, entry, land):
    """An engine whose ONE sensor is `entry` and whose one landscape is `land`: no set, no table."""
    c = HS.ENTRIES[entry]
    e = navsim_amd.FamiliarityEngine(device=0)
    e.set_landscape(land)
    e.configure_sensor(HS.SHAPES[shape], c["pixel"], HS.level_table(shape, entry), c["mask"])
    return e


def table_engine(shape, pairs=None):
    """own_engine with the landscapes of `pairs` ((landscape of lands(), entry), ...; default the four under TABLE) as a set and their
    entries as its sensor table."""
    pairs = pairs or tuple(enumerate(HS.TABLE))
    e = own_engine(shape, HL.lands()[0])
    e.lands_set([HL.lands()[l] for l, _ in pairs])
    e.sensors_set(*HS.table_args(shape, [n for _, n in pairs]))
    return e


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = table_engine(shape)
        return made[shape]
    yield get
    for e in made.values():
        e.close()


def same_bits(a, b, what=None):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    bad = np.argwhere(H.bits(a) != H.bits(b))
    assert len(bad) == 0, (what, bad[:6].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


def rel(got, want):
    return float(np.max(np.abs(np.asarray(got) - want)) / np.max(np.abs(want)))


def mb_begin(e, shape, wts=None):
    conn, n_active, _ = HS.mb_banks(shape)
    w, h = HS.SHAPES[shape]
    e.mb_begin(h, w, conn, n_active, 2)
    e.mbank_set(HS.N_BANKS)
    if wts is not None:
        for r, wt in enumerate(wts):
            e.mbank_set_weights(r, wt)


def im_begin(e, shape, Ws=None):
    W0, _ = HS.im_banks(shape)
    w, h = HS.SHAPES[shape]
    e.infomax_begin(h, w, W0, channel=2, learning_rate=HS.IM["eta"])
    e.ibank_set(HS.N_BANKS, W0)
    if Ws is not None:
        for r, W in enumerate(Ws):
            e.ibank_set_weights(r, W)


# ---- 1. lands_sense under a table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_lands_sense_is_the_host_model_under_each_poses_own_entry(shape):
    s = HS.sense_case(shape)
    e = table_engine(shape, HS.SET5)                                                      # L0 entered twice: under E0 and under E4
    try:
        assert e.n_sensors == 5
        info = e.sensors_info()
        px, luts, masks = HS.table_args(shape, [n for _, n in HS.SET5])
        assert info["n_sensors"] == 5 and info["pixel_dimensions"].tolist() == [list(p) for p in px] and info["masks"].tolist() == list(masks)
        assert np.array_equal(info["luts"], luts)
        got = e.lands_sense(s["x"], s["y"], s["angle"], s["land_of"])
        assert got.dtype == np.uint8 and np.array_equal(got, s["scenes"])
        on0 = s["on0"]                                                                    # the poses of landscape 0 once more, on its second entry
        both = e.lands_sense(np.concatenate([s["x"][on0], s["x"][on0]]), np.concatenate([s["y"][on0], s["y"][on0]]),
                             np.concatenate([s["angle"][on0], s["angle"][on0]]), [4] * len(on0) + [0] * len(on0))
        assert np.array_equal(both[:len(on0)], s["twice"]) and np.array_equal(both[len(on0):], s["scenes"][on0])
        # without a landscape table: the engine's landscape under the engine's sensor, table or not
        assert np.array_equal(e.sense(s["x"][on0], s["y"][on0], s["angle"][on0]), s["own"][on0])
        e.sensors_clear()
        assert e.n_sensors == 0 and e.sensors_info()["n_sensors"] == 0 and e.lands_info()["n_lands"] == 5
        assert np.array_equal(e.lands_sense(s["x"], s["y"], s["angle"], s["land_of"]), s["own"])   # the engine's configuration again
        e.sensors_set(px, luts, masks)
        assert np.array_equal(e.lands_sense(s["x"], s["y"], s["angle"], s["land_of"]), s["scenes"])
    finally:
        e.close()


# ---- 2. the footprint is the entry's own -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_a_pose_is_flagged_under_the_entry_whose_footprint_leaves_the_landscape_and_not_under_the_smaller_one(shape):
    x, y, ang, land_of, scenes = HS.foot_case(shape)
    e = table_engine(shape, HS.FOOT_SET)
    try:
        keep = [0, 1, 3]
        got = e.lands_sense(x[keep], y[keep], ang[keep], land_of[keep])
        assert all(np.array_equal(got[k], scenes[v]) for k, v in enumerate(keep))
        with pytest.raises(IndexError, match=r"pose 2 .*landscape 2 .211 x 173"):
            e.lands_sense(x, y, ang, land_of)
        # a step: the member's DV_RES_SENSE_ERROR, the others scored
        planes = np.stack([scenes[v] for v in keep])[:, None]                             # [3, 1, h, w, 3]
        banks = np.array([0, 1, 2, 1], dtype=np.int32)
        conn, n_active, wts = HS.mb_banks(shape)
        mb_begin(e, shape, wts)
        res = e.mbank_sense_step_batch(x, y, ang[:, None], banks, land_of_member=land_of)
        assert res.flags.tolist() == [0, 0, HS.SENSE_ERROR, 0] and res.best_idex.tolist() == [0, 0, -1, 0]
        want = [-float(HE.novelty(wts[banks[v]], planes[k, :, :, :, 2], conn, n_active)[0]) for k, v in enumerate(keep)]
        assert res.angle_familiarity[keep, 0].tolist() == want
        _, Ws = HS.im_banks(shape)
        im_begin(e, shape, Ws)
        res = e.ibank_sense_step_batch(x, y, ang[:, None], banks, land_of_member=land_of)
        assert res.flags.tolist() == [0, 0, HS.SENSE_ERROR, 0] and res.best_idex.tolist() == [0, 0, -1, 0]
        want = np.array([HI.familiarity(Ws[banks[v]], planes[k, :, :, :, 2])[0] for k, v in enumerate(keep)])
        err = rel(res.angle_familiarity[keep, 0], want)
        print("sensors, flagged step %s: infomax relative error %.3e (bound %.1e)" % (shape, err, HI.TOL))
        assert err <= HI.TOL
        views, first = HS.route_views(shape)[:2]
        e.rviews_set_u8(views, first)
        weights = [0.25, 0.0, 1.0, 0.5]
        res = e.rviews_sense_step(x, y, ang[:, None], banks, weights, land_of_member=land_of)
        assert res.flags.tolist() == [0, 0, HS.SENSE_ERROR, 0] and res.best_idex.tolist() == [0, 0, -1, 0]
        fam, view, _, scene = HR.expected(views, first, planes, banks[keep], np.array(weights)[keep])
        same_bits(res.angle_familiarity[keep], fam)
        assert np.array_equal(res.angle_view[keep], view)
        rows, flags = e.rviews_scene(x, y, ang[:, None], banks, weights, land_of_member=land_of, want_flags=True)
        assert flags.tolist() == [0, 0, HS.SENSE_ERROR, 0] and np.isinf(rows[2]).all()
        for k, v in enumerate(keep):
            same_bits(rows[v], scene[k], v)
    finally:
        e.close()


# ---- 3. training from poses ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_routes_on_three_landscapes_and_entries_train_in_one_call(engines, shape):
    e = engines(shape)
    t = HS.train_case(shape)
    w, h = HS.SHAPES[shape]
    # mushroom body
    conn, n_active, wts = HS.mb_banks(shape)
    mb_begin(e, shape)
    views = e.mbank_train_from_poses(t["x"], t["y"], t["angle"], t["bank_of"], land_of_view=t["land_of"])
    assert np.array_equal(views, t["scenes"])                                            # the host model, byte for byte
    assert np.array_equal(e.mbank_read_weights(), wts)                                    # the statement, bit for bit
    assert e.mbank_info()["views_trained"].tolist() == list(HL.ROUTE_POINTS)
    # Infomax
    W0, Ws = HS.im_banks(shape)
    im_begin(e, shape)
    views = e.ibank_train_from_poses(t["x"], t["y"], t["angle"], t["bank_of"], land_of_view=t["land_of"])
    assert np.array_equal(views, t["scenes"])
    got = np.stack([e.ibank_read_weights(r) for r in range(3)])
    worst = max(rel(got[r], Ws[r]) for r in range(3))
    print("sensors, infomax weights %s: relative error %.3e (bound %.1e)" % (shape, worst, HI.TOL))
    assert worst <= HI.TOL
    for r in range(3):                                                                    # an engine with that one sensor that trains that route alone
        o = entry_engine(shape, HS.TABLE[HL.ROUTE_LANDS[r]], HL.lands()[HL.ROUTE_LANDS[r]])
        try:
            o.infomax_begin(h, w, W0, channel=2, learning_rate=HS.IM["eta"])
            i = t["first"][r]
            assert np.array_equal(o.infomax_train_from_poses(t["x"][i], t["y"][i], t["angle"][i]), t["scenes"][i])
            same_bits(o.infomax_read_weights(), got[r], r)
        finally:
            o.close()
    # perfect memory: the store's views, route by route
    want, first, x, y, ang, land_of = HS.route_views(shape)
    views = e.rviews_set_from_poses(x, y, ang, first, land_of_view=land_of)
    assert np.array_equal(views, want) and np.array_equal(e.rviews_info()["first"], first)
    patches = np.stack([want[first[r] + 3] for r in range(3)])[:, None]                   # a view of route r scores h * w there
    r = e.rviews_step_u8(patches, [0, 1, 2], [0.3, 0.3, 0.3])
    assert (r.angle_familiarity == h * w).all()
    e.rviews_clear()


# ---- 4. steps --------------------------------------------------------------------------------------------------------------------------------
def check_steps(e, shape, n, A):
    case = HS.step_case(shape, n, A)
    w, h = HS.SHAPES[shape]
    planes = np.ascontiguousarray(case["planes"][..., 2])
    # mushroom body: the statement, bit for bit
    want = HS.mb_statement(shape, case)
    res = e.mbank_sense_step_batch(case["xs"], case["ys"], case["angs"], case["banks"], land_of_member=case["lands"])
    assert not res.flags.any()
    same_bits(res.angle_familiarity, want, "mushroom")
    assert res.best_idex.tolist() == np.argmax(want, axis=1).tolist()
    # Infomax: its statement, and infomax_score_u8 of an engine that holds that bank's W alone, on the host model's planes
    want = HS.im_statement(shape, case)
    res = e.ibank_sense_step_batch(case["xs"], case["ys"], case["angs"], case["banks"], land_of_member=case["lands"])
    assert not res.flags.any()
    err = rel(res.angle_familiarity, want)
    print("sensors, infomax scores %s %dx%d: relative error %.3e (bound %.1e)" % (shape, n, A, err, HI.TOL))
    assert err <= HI.TOL
    _, Ws = HS.im_banks(shape)
    lone = navsim_amd.FamiliarityEngine(device=0)
    try:
        for r in range(HS.N_BANKS):
            m = np.flatnonzero(case["banks"] == r)
            if len(m):
                lone.infomax_begin(h, w, Ws[r], channel=2, learning_rate=HS.IM["eta"])
                same_bits(res.angle_familiarity[m], lone.infomax_score_u8(planes[m].reshape(-1, h, w)).reshape(len(m), A), ("infomax", r))
    finally:
        lone.close()
    # perfect memory: oracle.step on the member's own route views (members repeat every 40: 8 places x 5 banks and landscapes)
    views, first = HS.route_views(shape)[:2]
    weights = np.array([CHEM[i % 5] for i in range(n)])
    k = min(n, 40)
    fam, view, best, scene = HR.expected(views, first, case["planes"][:k], case["banks"][:k], weights[:k])
    pick = np.arange(n) % k
    res = e.rviews_sense_step(case["xs"], case["ys"], case["angs"], case["banks"], weights, land_of_member=case["lands"])
    assert not res.flags.any()
    same_bits(res.angle_familiarity, fam[pick], "perfect memory")
    assert np.array_equal(res.angle_view, view[pick]) and res.best_idex.tolist() == best[pick].tolist()
    if n <= 5:
        rows = e.rviews_scene(case["xs"], case["ys"], case["angs"], case["banks"], weights, land_of_member=case["lands"])
        for i in range(n):
            same_bits(rows[i], scene[i], ("scene", i))


@pytest.fixture(scope="module")
def stepping(engines):
    """shape -> the table engine with the statement's banks and the host model's route views in place."""
    def get(shape):
        e = engines(shape)
        mb_begin(e, shape, HS.mb_banks(shape)[2])
        im_begin(e, shape, HS.im_banks(shape)[1])
        e.rviews_set_u8(*HS.route_views(shape)[:2])
        return e
    return get


@pytest.mark.parametrize("n,A", HL.LAYOUTS)
@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_members_step_on_their_own_landscapes_under_their_own_entries(stepping, shape, n, A):
    check_steps(stepping(shape), shape, n, A)


def test_columns_past_a_launch_and_a_slab_edge_keep_their_members_entry(stepping):
    """683 members x 12 headings = 8196 columns: column 8192 is inside member 682, whose entry is not member 0's."""
    n, A = HL.WIDE_LAYOUT
    case = HS.step_case("wide", n, A)
    assert HS.TABLE[case["lands"][n - 1]] != HS.TABLE[case["lands"][0]] and (n - 1) * A < 8192 < n * A
    check_steps(stepping("wide"), "wide", n, A)


# ---- 5. refusals leave everything as it was ----------------------------------------------------------------------------------------------------
def test_a_refused_table_leaves_the_old_one_the_set_the_banks_and_the_store_and_a_new_set_drops_the_table(stepping):
    shape = "wide"
    e = stepping(shape)
    case = HS.step_case(shape, 5, 13)
    weights = np.array([CHEM[i % 5] for i in range(5)])

    def snapshot():
        return (e.mbank_sense_step_batch(case["xs"], case["ys"], case["angs"], case["banks"], land_of_member=case["lands"]).angle_familiarity,
                e.ibank_sense_step_batch(case["xs"], case["ys"], case["angs"], case["banks"], land_of_member=case["lands"]).angle_familiarity,
                e.rviews_sense_step(case["xs"], case["ys"], case["angs"], case["banks"], weights, land_of_member=case["lands"]).angle_familiarity)
    before = snapshot()
    wts = e.mbank_read_weights()
    px, luts, masks = HS.table_args(shape, HS.TABLE)
    for bad in ((px[:3], luts[:3], masks[:3]), ([(1, 2), (2, 4), (64, 65), (2, 4)], luts, masks), (px, luts, [0, 1, 9, 1])):
        with pytest.raises(ValueError):
            e.sensors_set(*bad)
    # past the Python-side checks: the library's own, naming the entry, before anything reaches the device
    lib, ctx = e._lib, e._ctx

    def raw(pw, ph, mk, n):
        pw, ph, mk = (np.array(a, dtype=np.int32) for a in (pw, ph, mk))
        return lib.dv_sensors_set(ctx, pw.ctypes.data_as(N._i32p), ph.ctypes.data_as(N._i32p), mk.ctypes.data_as(N._i32p), N.u8ptr(luts), n)
    assert raw([1, 2, 3], [2, 4, 2], [0, 1, 2], 3) == INVALID and "n_lands = 4" in lib.dv_last_error(ctx).decode()
    assert raw([1, 2, 0, 2], [2, 4, 2, 4], [0, 1, 2, 1], 4) == INVALID and "entry 2" in lib.dv_last_error(ctx).decode()
    assert raw([1, 2, 3, 64], [2, 4, 2, 65], [0, 1, 2, 1], 4) == INVALID and "entry 3" in lib.dv_last_error(ctx).decode()
    assert raw([1, 2, 3, 2], [2, 4, 2, 4], [0, 9, 2, 1], 4) == INVALID and "entry 1" in lib.dv_last_error(ctx).decode()
    assert raw([1, 2, 3, 2], [2, 4, 2, 4], [0, -1, 2, 1], 4) == INVALID and "entry 1" in lib.dv_last_error(ctx).decode()
    info = e.sensors_info()
    assert info["n_sensors"] == 4 and info["pixel_dimensions"].tolist() == [list(p) for p in px] and np.array_equal(info["luts"], luts)
    assert e.lands_info()["n_lands"] == 4 and np.array_equal(e.mbank_read_weights(), wts) and e.rviews_info()["n_routes"] == 3
    for a, b in zip(snapshot(), before):
        same_bits(a, b)
    # a new set drops the table: its entries are gone
    s = HS.sense_case(shape)
    e.lands_set(list(HL.lands()))
    assert e.n_sensors == 0 and e.sensors_info()["n_sensors"] == 0
    assert np.array_equal(e.lands_sense(s["x"], s["y"], s["angle"], s["land_of"]), s["own"])
    e.sensors_set(px, luts, masks)
    e.lands_clear()
    assert e.n_sensors == 0 and e.sensors_info()["n_sensors"] == 0
    assert lib.dv_sensors_set(ctx, None, None, None, None, 4) == INVALID
    assert raw([1, 2, 3, 2], [2, 4, 2, 4], [0, 1, 2, 1], 4) == STATE
    with pytest.raises(N.EngineError, match="lands_set first"):
        e.sensors_set(px, luts, masks)
    e.lands_set(list(HL.lands()))
    e.sensors_set(px, luts, masks)                                                        # (as the module's other tests found it)
    for a, b in zip(snapshot(), before):
        same_bits(a, b)


# ---- 6. unchanged without a table --------------------------------------------------------------------------------------------------------------
def test_the_calls_without_a_table_keep_their_bits_beside_a_live_table_after_it_is_cleared_and_on_an_engine_that_never_had_one():
    shape = "wide"
    s = HS.sense_case(shape)
    case = HS.step_case(shape, 5, 13)
    weights = np.array([CHEM[i % 5] for i in range(5)])
    _, _, wts = HS.mb_banks(shape)
    _, Ws = HS.im_banks(shape)
    views, first = HS.route_views(shape)[:2]
    plain = own_engine(shape, HL.lands()[0])                                              # a set, never a table
    plain.lands_set(list(HL.lands()))
    e = table_engine(shape)
    try:
        for eng in (plain, e):
            mb_begin(eng, shape, wts)
            im_begin(eng, shape, Ws)
            eng.rviews_set_u8(views, first)

        def calls(eng, with_lands):
            k = dict(land_of_member=case["lands"]) if with_lands else {}
            out = [eng.mbank_sense_step_batch(case["xs"], case["ys"], case["angs"], case["banks"], **k).angle_familiarity,
                   eng.ibank_sense_step_batch(case["xs"], case["ys"], case["angs"], case["banks"], **k).angle_familiarity,
                   eng.rviews_sense_step(case["xs"], case["ys"], case["angs"], case["banks"], weights, **k).angle_familiarity]
            out += list(eng.rviews_scene(case["xs"], case["ys"], case["angs"], case["banks"], weights, **k))
            if with_lands:
                out.append(eng.lands_sense(s["x"], s["y"], s["angle"], s["land_of"]).astype(np.float64))
            else:
                out += [eng.sense(s["x"], s["y"], s["angle"]).astype(np.float64),
                        eng.mb_sense_step_batch(case["xs"], case["ys"], case["angs"]).angle_familiarity,
                        eng.infomax_sense_step_batch(case["xs"], case["ys"], case["angs"]).angle_familiarity]
            return out
        want_one, want_set = calls(plain, False), calls(plain, True)
        assert np.array_equal(want_set[-1], s["own"].astype(np.float64))                  # (the parent's path is the host model's under OWN)
        for a, b in zip(calls(e, False), want_one):                                       # beside a live table: the one-landscape calls
            same_bits(a, b)
        under = calls(e, True)
        assert not np.array_equal(under[0], want_set[0]) and np.array_equal(under[-1], s["scenes"].astype(np.float64))
        e.sensors_clear()
        for a, b in zip(calls(e, False) + calls(e, True), want_one + want_set):           # after it is cleared: everything
            same_bits(a, b)
    finally:
        plain.close()
        e.close()


# ---- 7. the ensembles --------------------------------------------------------------------------------------------------------------------------
MODELS = {
    "mushroom": (lambda w: mushroom_familiarity(n_kc=1043, fan_in=8, sparsity=0.02, seed=6), "MushroomRouteEnsemble"),
    "infomax": (lambda w: infomax_familiarity(learning_rate=1e-3, seed=9, n_hidden=18), "InfomaxRouteEnsemble"),
    "sads": (lambda w: sads_familiarity(w, exact=True), "SadsRouteEnsemble"),
}
WEIGHTS = (0.25, 0.0, 1.0, 0.25, 0.5, 0.25, 0.3, 0.25, 0.0, 0.75, 0.25, 1.0)


def make_agent(model, land, weight=0.25, **config):
    return navsim_amd.NavBySceneFamiliarity(np.array(land), HL.ENS_SENSOR, 1.0, n_test_angles=9, use_gpu_sensor=True,
                                            familiarity_model=MODELS[model][0](weight), **dict(HS.ENS_AGENT, **config))


def make_ensemble(model, landscapes, routes, starts, metrics="host", sensors=HS.ENS_SENSORS):
    cls = getattr(navsim_amd, MODELS[model][1])
    extra = dict(chem_weights=WEIGHTS[:len(starts)]) if model == "sads" else {}
    return cls.from_landscapes(make_agent(model, landscapes[0]), list(landscapes), routes, starts, metrics=metrics, sensors=list(sensors), **extra)


def lone_agents(model, landscapes, routes, starts):
    """Every member's twin: an agent with an engine, a landscape, a sensor configuration and a route of its own."""
    out = []
    for k, (r, pos, ang) in enumerate(starts):
        l, path = routes[r]
        a = make_agent(model, landscapes[l], WEIGHTS[k], **HS.ens_config(l))
        a.train_from_path(path)
        a.position, a.angle = pos, ang
        out.append(a)
    return out


def close_all(ens, alone):
    ens.agents[0].clear_training()
    ens.engine.close()
    for a in alone:
        a.clear_training()
        a._engine.close()


@pytest.mark.parametrize("metrics", ("host", "device"))
@pytest.mark.parametrize("model", sorted(MODELS))
def test_ensemble_members_equal_lone_agents_with_their_own_sensor(model, metrics):
    landscapes = HL.lands()[:3]
    routes = HL.ens_routes()
    starts = HL.ens_starts(routes)
    ens = make_ensemble(model, landscapes, routes, starts, metrics)
    alone = lone_agents(model, landscapes, routes, starts)
    try:
        assert len(ens.agents) == 12 and not ens._uniform and ens.engine.n_sensors == 3
        for m, a in zip(ens.agents, alone):
            l = m.landscape_index
            assert m.sensor_index == l and m.landscape is landscapes[l]
            assert m.sensor_pixel_dimensions.tolist() == a.sensor_pixel_dimensions.tolist() and m.n_sensor_levels == a.n_sensor_levels
            assert m.mask_middle_n == a.mask_middle_n and m._sensor_r == a._sensor_r == HS.ens_radius(l) and m._bounds_tuple() == a._bounds_tuple()
            assert np.array_equal(m.familiar_scenes, a.familiar_scenes)
            assert np.array_equal(m.get_sensor_mat(m.position, m.angle), a.get_sensor_mat(a.position, a.angle))
        for t in range(24):
            ens.step_forward()
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
        assert any(m.position != s[1] for m, s in zip(ens.agents, starts))
    finally:
        close_all(ens, alone)


def _csv(rows):
    out = io.StringIO()
    w = csv.DictWriter(out, fieldnames=sorted(rows[0]))
    w.writeheader()
    w.writerows(rows)
    return out.getvalue()


@pytest.mark.parametrize("model", sorted(MODELS))
def test_run_ensemble_rows_equal_lone_run_experiment_rows_under_their_own_sensors(model):
    landscapes = HL.lands()[:3]
    routes = HL.ens_routes()
    starts = HL.ens_starts(routes)
    ens = make_ensemble(model, landscapes, routes, starts, "device")
    alone = lone_agents(model, landscapes, routes, starts)
    try:
        rows = navsim_amd.run_ensemble(ens, 36)
        wants = [navsim_amd.run_experiment(a, 36) for a in alone]
        assert _csv(rows) == _csv(wants)
    finally:
        close_all(ens, alone)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_a_member_whose_larger_footprint_leaves_its_landscape_stops_as_its_lone_twin_and_the_others_go_on(model):
    """Five members: three at EDGE_START -- inside the bounds of every landscape under the agent's own footprint, past L1's under entry
    1's; one on its route; one at FOOTPRINT_START, inside entry 1's bounds on L1 where a corner of that footprint leaves the landscape."""
    HS.edge_facts()
    L = HL.lands()
    landscapes = [L[l] for l in HS.EDGE_LANDS]
    routes = HS.edge_routes()
    pos, ang = HS.EDGE_START
    starts = [(0, pos, ang), (1, pos, ang), (2, pos, ang), (1, tuple(routes[1][1][3]), 0.8), (1,) + HS.FOOTPRINT_START]
    ens = make_ensemble(model, landscapes, routes, starts)
    alone = lone_agents(model, landscapes, routes, starts)
    try:
        for t in range(2):
            ens.step_forward()
            codes = []
            for a in alone:
                if a.stopped_with_exception is None:
                    try:
                        a.step_forward()
                    except navsim_amd.StopNavigationException as stop:
                        a.stopped_with_exception = stop
                    except IndexError as stop:                                            # the footprint left the landscape: the trial ends (-3)
                        a.stopped_with_exception = stop
                s = a.stopped_with_exception
                codes.append(0 if s is None else s.get_code() if hasattr(s, "get_code") else -3)
            assert ens.stop_status == codes == [0, -2, 0, 0, -3], t
            for i in (0, 2, 3):
                assert ens.agents[i].position == alone[i].position and ens.agents[i].position != starts[i][1], (t, i)
                assert np.array_equal(H.bits(ens.agents[i].angle_familiarity), H.bits(alone[i].angle_familiarity)), (t, i)
        assert isinstance(ens.agents[1].stopped_with_exception, navsim_amd.OutOfLandscapeBoundsException) and ens.agents[1].position == pos
        assert isinstance(ens.agents[4].stopped_with_exception, IndexError) and ens.agents[4].position == HS.FOOTPRINT_START[0]
    finally:
        close_all(ens, alone)


def test_an_ensemble_made_without_sensors_gets_no_table_and_no_sensor_index():
    landscapes = HL.lands()[:3]
    routes = HL.ens_routes()
    starts = HL.ens_starts(routes)
    ens = navsim_amd.MushroomRouteEnsemble.from_landscapes(make_agent("mushroom", landscapes[0]), list(landscapes), routes, starts)
    try:
        assert ens.engine.n_sensors == 0 and ens.engine.sensors_info()["n_sensors"] == 0
        assert all(a.sensor_index is None and a._sensor_r == 6.0 for a in ens.agents)
    finally:
        ens.agents[0].clear_training()
        ens.engine.close()
