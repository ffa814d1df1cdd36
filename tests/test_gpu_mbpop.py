"""Population tables of the mushroom-body model on the device (dv_mbpop_*): banks with cells, wiring, quota and channel of their own,
trained in shared launches and scored member by member, against the NumPy statement run per bank with that bank's population
(tests/helpers_mbpop.py over tests/helpers_mushroom.py) and against lone engines begun with one population each -- bit for bit: every
comparison is np.array_equal on integers or on the scores' uint64 views.  MushroomRouteEnsemble(populations=...) against lone agents
built with mushroom_familiarity of the member's population and trained on its route alone."""
import csv
import io

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import mushroom_familiarity, synth
from tests import helpers_infomax as HI
from tests import helpers_lands as HL
from tests import helpers_mbpop as HP
from tests import helpers_mushroom as H
from tests import helpers_mushroom_banks as HB
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
    """The engine that is begun with ONE population at a time."""
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


def same(res, fam, best=None):
    assert res.angle_familiarity.shape == fam.shape and res.angle_familiarity.dtype == np.float64
    bad = np.argwhere(H.bits(res.angle_familiarity) != H.bits(fam))
    assert len(bad) == 0, (bad[:6].tolist(), res.angle_familiarity[tuple(bad[0])], fam[tuple(bad[0])])
    assert res.best_idex.tolist() == np.argmax(fam, axis=1).tolist()                       # the first maximum
    if best is not None:
        assert res.best_idex.tolist() == np.asarray(best).tolist()


def begin_table(e, h, w, pops, pop_of_bank):
    e.mb_begin(h, w, pops[0]["conn"], pops[0]["n_active"], pops[0]["channel"])
    e.mbpop_set(pops, pop_of_bank)


def begin_lone(e, h, w, pop):
    e.mb_begin(h, w, pop["conn"], pop["n_active"], pop["channel"])


def check_against_lone_engines(lone, h, w, pops, pop_of_bank, views, bank_of, got_wts, planes, banks, res):
    """Bank by bank: an engine begun with the bank's population alone, trained on the bank's views, gives the bank's weights, and its
    batched step on the bank's members gives their rows."""
    for b, p in enumerate(pop_of_bank):
        begin_lone(lone, h, w, pops[p])
        mine = np.ascontiguousarray(views[np.asarray(bank_of) == b])
        if len(mine):
            lone.mb_train_u8(mine)
        assert np.array_equal(lone.mb_read_weights(), got_wts[b]), b
        rows = np.flatnonzero(np.asarray(banks) == b)
        if len(rows):
            one = lone.mb_step_batch_u8(np.ascontiguousarray(planes[rows]))
            assert np.array_equal(H.bits(one.angle_familiarity), H.bits(res.angle_familiarity[rows])), b
            assert one.best_idex.tolist() == res.best_idex[rows].tolist(), b


# ---- 1. one table of five populations and seven banks on 7 x 5 views -------------------------------------------------------------------
def test_one_table_trains_and_scores_every_bank_through_its_own_population(eng, lone):
    d = HP.table_data()
    pops, of_bank, B = d["pops"], d["pop_of_bank"], len(d["pop_of_bank"])
    begin_table(eng, d["h"], d["w"], pops, of_bank)
    info = eng.mbpop_info()
    assert (info["n_pops"], info["n_banks"]) == (5, 7) and info["population_of_bank"].tolist() == list(of_bank)
    assert [info[k].tolist() for k in ("n_kc", "fan_in", "n_active")] == [list(col) for col in zip(*HP.TABLE["pops"])]
    assert info["channel"].tolist() == [2] * 5 and info["views_trained"].tolist() == [0] * B and info["n_depressed"].tolist() == [0] * B
    lengths = [pops[p]["n_kc"] for p in of_bank]
    assert info["bytes"] >= sum(lengths) + 2 * sum(K * c for K, c, _ in HP.TABLE["pops"])
    fresh = eng.mbank_read_weights()
    assert [len(f) for f in fresh] == lengths and all((f == 1).all() for f in fresh)
    eng.mbank_train_u8(d["views"], d["bank_of"])                                          # 40 views, all banks and populations: one call
    got = eng.mbank_read_weights()
    for b in range(B):
        assert np.array_equal(got[b], d["wts"][b]), (b, np.flatnonzero(got[b] != d["wts"][b])[:8])
        assert np.array_equal(eng.mbank_read_weights(b), d["wts"][b])
    zeros, counts = [int((w == 0).sum()) for w in d["wts"]], np.bincount(d["bank_of"], minlength=B).tolist()
    for info in (eng.mbank_info(), eng.mbpop_info()):
        assert info["n_banks"] == B and info["n_depressed"].tolist() == zeros and info["views_trained"].tolist() == counts
    one = eng.mb_info()                                                                   # the begin's model; the two counts are bank 0's
    assert (one["n_kc"], one["fan_in"], one["n_active"]) == HP.TABLE["pops"][0] and (one["views_trained"], one["n_depressed"]) == (counts[0], zeros[0])
    res = eng.mbank_step_batch_u8(d["planes"], d["banks"])                                # 2 members x 13 headings per bank
    assert not res.flags.any()
    same(res, d["fam"], d["best"])
    check_against_lone_engines(lone, d["h"], d["w"], pops, of_bank, d["views"], d["bank_of"], got, d["planes"], d["banks"], res)
    # training again, in another order, changes nothing
    order = np.random.default_rng(5).permutation(len(d["views"]))
    eng.mbank_train_u8(np.ascontiguousarray(d["views"][order]), d["bank_of"][order])
    assert all(np.array_equal(g, w) for g, w in zip(eng.mbank_read_weights(), d["wts"]))
    assert eng.mbank_info()["views_trained"].tolist() == [2 * c for c in counts]


# ---- 2. 33 x 31 views from sensed poses: one wiring under the three channels -------------------------------------------------------------
SENSED = dict(sensor=(33, 31), pixel=[2, 2], levels=5, K=1043, c=8, n_active=21, seed=331)


def sensed_agent(gpu):
    keep = mushroom_familiarity(n_kc=300, fan_in=4, seed=3) if gpu else HS._keep
    return navsim_amd.NavBySceneFamiliarity(synth.synth_landscape(*HI.SENSED["land"]), SENSED["sensor"], 1.0, n_test_angles=9,
                                            sensor_pixel_dimensions=list(SENSED["pixel"]), n_sensor_levels=SENSED["levels"], mask_middle_n=0,
                                            use_gpu_sensor=gpu, familiarity_model=keep)


def host_scenes(agent, x, y, angles):
    return np.stack([agent.get_sensor_mat((xi, yi), ai) for xi, yi, ai in zip(np.ravel(x), np.ravel(y), np.ravel(angles))])


def test_sensed_poses_train_and_score_each_bank_under_its_own_channel():
    w, h = SENSED["sensor"]
    assert (w * h) % 4 == 3
    pops = [HP.population(w * h, SENSED["K"], SENSED["c"], SENSED["n_active"], SENSED["seed"], channel=ch) for ch in (0, 1, 2)]
    assert np.array_equal(pops[0]["conn"], pops[2]["conn"])                               # one wiring
    x, y, ang = HS.route_poses()
    F = len(x)
    host = sensed_agent(False)
    scenes = host_scenes(host, x, y, ang)
    bank_of = np.repeat(np.arange(3, dtype=np.int32), F)                                  # every view into every bank
    wts = HP.train(pops, (0, 1, 2), np.concatenate([scenes] * 3), bank_of)
    assert all((wts[a] != wts[b]).any() for a in range(3) for b in range(a + 1, 3))       # the three banks differ
    xs, ys, angs = HS.member_poses()
    banks = [0, 1, 2, 0, 1]
    member_scenes = host_scenes(host, np.repeat(xs, angs.shape[1]), np.repeat(ys, angs.shape[1]), angs).reshape(angs.shape + (h, w, 3))
    want = HP.scores(pops, (0, 1, 2), wts, member_scenes, banks)
    assert not np.array_equal(want[0], HP.scores(pops, (0, 1, 2), wts, member_scenes, [1])[0]) and want.min() < 0
    a = sensed_agent(True)
    b = sensed_agent(True)
    try:
        e = a._engine
        begin_table(e, h, w, pops, (0, 1, 2))
        views = e.mbank_train_from_poses(np.tile(x, 3), np.tile(y, 3), np.tile(ang, 3), bank_of)
        assert np.array_equal(views, np.concatenate([scenes] * 3))                        # the device's sensor is the host's
        got = e.mbank_read_weights()
        for ch in range(3):
            assert np.array_equal(got[ch], wts[ch]), ch
        assert e.mbank_info()["views_trained"].tolist() == [F] * 3
        res = e.mbank_sense_step_batch(xs, ys, angs, banks)
        assert not res.flags.any()
        same(res, want)
        for call in (lambda: e.mb_train_from_poses(x, y, ang), lambda: e.mb_sense_step(xs[0], ys[0], angs[0]),
                     lambda: e.mb_sense_step_batch(xs, ys, angs)):                        # bank 0 behind the begin's wiring: refused
            with pytest.raises(N.EngineError, match="dv_mbpop_clear.*DV_ERR_STATE"):
                call()
        assert all(np.array_equal(g, wt) for g, wt in zip(e.mbank_read_weights(), wts))
        lone = b._engine
        for ch in range(3):                                                               # a lone engine begun with the channel's population
            begin_lone(lone, h, w, pops[ch])
            lone.mb_train_from_poses(x, y, ang, want_views=False)
            assert np.array_equal(lone.mb_read_weights(), got[ch]), ch
            rows = [i for i, bk in enumerate(banks) if bk == ch]
            one = lone.mb_sense_step_batch(xs[rows], ys[rows], angs[rows])
            assert np.array_equal(H.bits(one.angle_familiarity), H.bits(res.angle_familiarity[rows])), ch
    finally:
        a._engine.close()
        b._engine.close()


# ---- 3. constant planes: the quota among equals runs through the waves' spans ------------------------------------------------------------
def test_constant_planes_fire_the_first_cells_in_index_order_in_each_population(eng, lone):
    d = HP.constant_data()
    begin_table(eng, d["h"], d["w"], d["pops"], (0, 1))
    planes = np.ascontiguousarray(np.concatenate([d["planes"], d["planes"]]))
    bank_of = np.array([0, 0, 1, 1], dtype=np.int32)
    eng.mbank_train_u8(planes, bank_of)                                                   # K = 257 and K = 1043 in one launch
    got = eng.mbank_read_weights()
    for b in range(2):
        assert np.array_equal(got[b], d["want"][b]), (b, np.flatnonzero(got[b] != d["want"][b])[:8])
        assert eng.mbank_info()["n_depressed"][b] == d["pops"][b]["n_active"]
    members = np.ascontiguousarray(np.stack([d["planes"], d["planes"]]))                  # trained views: d = 0 in either bank
    res = eng.mbank_step_batch_u8(members, [0, 1])
    same(res, np.zeros((2, 2)))
    check_against_lone_engines(lone, d["h"], d["w"], d["pops"], (0, 1), planes, bank_of, got, members, [0, 1], res)


# ---- 4. launch edges: the bank is read at the CALL's column ------------------------------------------------------------------------------
def test_the_last_view_and_the_last_column_past_a_launch_keep_their_own_bank_and_population(eng, lone):
    d = HP.edge_data()
    begin_table(eng, d["h"], d["w"], d["pops"], (0, 1))
    views = d["two"][d["pick"]]
    eng.mbank_train_u8(views, d["bank_of"])                                               # 8193 views: the last alone is bank 1's
    got = eng.mbank_read_weights()
    assert np.array_equal(got[0], d["wts"][0]) and np.array_equal(got[1], d["wts"][1])
    assert eng.mbank_info()["views_trained"].tolist() == [len(views) - 1, 1]
    planes = d["two"][d["step_pick"]]
    res = eng.mbank_step_batch_u8(planes, d["step_banks"])                                # 8193 columns: the last is inside member 2, bank 1
    same(res, d["fam"], d["best"])
    for b in range(2):
        begin_lone(lone, d["h"], d["w"], d["pops"][b])
        lone.mb_train_u8(d["two"][b:b + 1])
        assert np.array_equal(lone.mb_read_weights(), got[b]), b
        rows = np.flatnonzero(d["step_banks"] == b)
        one = lone.mb_step_batch_u8(np.ascontiguousarray(planes[rows]))
        assert np.array_equal(H.bits(one.angle_familiarity), H.bits(res.angle_familiarity[rows])), b


# ---- 5. the widest launch: 256 x 256 views, c = 16 and c = 1 in one call -----------------------------------------------------------------
def test_the_widest_plane_under_two_fan_ins_and_two_engines_whose_tables_need_different_lds(eng, lone):
    h = w = 256
    pops = [HP.population(h * w, 1043, 16, 21, 341), HP.population(h * w, 300, 1, 5, 342)]
    views = H.route_views(343, 4, h, w)
    bank_of = np.array([0, 1, 1, 0], dtype=np.int32)
    wts = HP.train(pops, (0, 1), views, bank_of)
    planes = np.ascontiguousarray(np.stack([np.stack([views[0], views[1]]), np.stack([views[0], views[1]])]))
    banks = np.array([0, 1], dtype=np.int32)
    fam = HP.scores(pops, (0, 1), wts, planes, banks)
    assert fam[0, 0] == 0 and fam[0, 1] < 0 and fam[1, 0] < 0 and fam[1, 1] == 0
    begin_table(eng, h, w, pops, (0, 1))                                                  # 65536 + 4 * 4081 * 4 + 64 = 130 896 bytes a launch
    eng.mbank_train_u8(views, bank_of)
    got = eng.mbank_read_weights()
    assert np.array_equal(got[0], wts[0]) and np.array_equal(got[1], wts[1])
    t = HP.table_data()
    begin_table(lone, t["h"], t["w"], t["pops"][:2], (0, 1, 1))                           # a table of c = 1 and c = 4 on 35 pixels: 4.1 KB
    small_wts = HP.train(t["pops"][:2], (0, 1, 1), t["views"], np.minimum(t["bank_of"], 2))
    lone.mbank_train_u8(t["views"], np.minimum(t["bank_of"], 2))
    small_banks = np.minimum(t["banks"], 2)
    small_fam = HP.scores(t["pops"][:2], (0, 1, 1), small_wts, t["planes"], small_banks)
    for _ in range(2):                                                                    # stepped alternately
        same(eng.mbank_step_batch_u8(planes, banks), fam)
        same(lone.mbank_step_batch_u8(t["planes"], small_banks), small_fam)
    res = eng.mbank_step_batch_u8(planes, banks)
    check_against_lone_engines(lone, h, w, pops, (0, 1), views, bank_of, got, planes, banks, res)


# ---- 6. landscape, sensor and population differ at once: the ensemble on a landscape set with a sensor table --------------------------
AGENT_MODEL = dict(n_kc=1043, fan_in=8, sparsity=0.02, seed=6)
SET_POPULATIONS = (None, dict(n_kc=300, fan_in=4, seed=11), dict(channel=1), dict(n_kc=300, fan_in=4, seed=11), dict(sparsity=0.05, seed=12),
                   dict(n_kc=2003, fan_in=16, channel=0))


def set_agent(land, model=None, **config):
    return navsim_amd.NavBySceneFamiliarity(np.array(land), HL.ENS_SENSOR, 1.0, n_test_angles=9, use_gpu_sensor=True,
                                            familiarity_model=mushroom_familiarity(**dict(AGENT_MODEL, **(model or {}))),
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
            assert np.array_equal(H.bits(m.angle_familiarity), H.bits(a.angle_familiarity)), (t, i)
            code = a.stopped_with_exception.get_code() if a.stopped_with_exception is not None else 0
            assert ens.stop_status[i] == code, (t, i)
            assert m.navigation_error == a.navigation_error and m.percent_recapitulated == a.percent_recapitulated, (t, i)


def test_banks_that_differ_in_landscape_sensor_and_population_equal_lone_agents():
    landscapes = HL.lands()[:3]
    routes = HL.ens_routes()
    starts = HL.ens_starts(routes)
    ens = navsim_amd.MushroomRouteEnsemble.from_landscapes(set_agent(landscapes[0]), list(landscapes), routes, starts, metrics="device",
                                                           sensors=list(HSN.ENS_SENSORS), populations=list(SET_POPULATIONS))
    alone = []
    for r, pos, ang in starts:
        l, path = routes[r]
        a = set_agent(landscapes[l], SET_POPULATIONS[r], **HSN.ens_config(l))
        a.train_from_path(path)
        a.position, a.angle = pos, ang
        alone.append(a)
    try:
        e = ens.engine
        assert e.n_sensors == 3 and e.n_lands == 3 and e.mbpop_info()["n_pops"] == 5     # routes 1 and 3 share a population
        info = ens.bank_info()
        assert info["population_of_bank"].tolist() == [0, 1, 2, 1, 3, 4] and info["n_kc"].tolist() == [1043, 300, 1043, 300, 1043, 2003]
        assert info["n_active"].tolist() == [21, 6, 21, 6, 52, 40]
        for r in range(6):
            one = alone[2 * r]._engine
            assert np.array_equal(e.mbank_read_weights(r), one.mb_read_weights()), r
            assert (info["views_trained"][r], info["n_depressed"][r]) == (one.mb_info()["views_trained"], one.mb_info()["n_depressed"]), r
        for m, a in zip(ens.agents, alone):
            assert m.population_index == info["population_of_bank"][m.memory_bank] and m.population["n_kc"] == a.familiarity_model.n_kc
            assert np.array_equal(m.familiar_scenes, a.familiar_scenes)
        step_together(ens, alone, 10)
        print("after 10 steps: stop_status %r" % (ens.stop_status,))
        assert any(m.position != s[1] for m, s in zip(ens.agents, starts))
    finally:
        ens.agents[0].clear_training()
        ens.engine.close()
        for a in alone:
            a.clear_training()
            a._engine.close()


# ---- 7. MushroomRouteEnsemble.from_routes_with(populations=...): 3 routes x 2 populations entered as 6 routes ----------------------------
ROUTE_POPULATIONS = (None, dict(n_kc=2003, fan_in=10, sparsity=0.01, seed=21, channel=1))


def route_agent(model=None):
    return navsim_amd.NavBySceneFamiliarity(synth.synth_landscape(3, 300, 4), (12, 10), 1.0, n_test_angles=9, use_gpu_sensor=True,
                                            familiarity_model=mushroom_familiarity(**dict(AGENT_MODEL, **(model or {}))))


def _csv(rows):
    out = io.StringIO()
    w = csv.DictWriter(out, fieldnames=sorted(rows[0]))
    w.writeheader()
    w.writerows(rows)
    return out.getvalue()


@pytest.fixture(scope="module")
def lone_rows():
    """run_experiment of every member's lone twin, once for both metrics."""
    paths = HB.routes()
    rows = []
    for r, pos, ang in route_starts(paths):
        a = route_agent(ROUTE_POPULATIONS[r % 2])
        try:
            a.train_from_path(paths[r // 2])
            a.position, a.angle = pos, ang
            rows.append(navsim_amd.run_experiment(a, frames=40))
        finally:
            a.clear_training()
            a._engine.close()
    return rows


def route_starts(paths):
    """HB.starts on the routes entered twice: route 2 k under the agent's model, 2 k + 1 under the other population."""
    return [(2 * r + p, pos, ang) for r, pos, ang in HB.starts(paths) for p in range(2)]


@pytest.mark.parametrize("metrics", ("host", "device"))
def test_run_ensemble_rows_equal_lone_run_experiment_rows_of_each_members_population(lone_rows, metrics):
    paths = HB.routes()
    routes = [paths[k // 2] for k in range(6)]
    ens = navsim_amd.MushroomRouteEnsemble.from_routes_with(route_agent(), routes, route_starts(paths), metrics=metrics,
                                                            populations=[ROUTE_POPULATIONS[k % 2] for k in range(6)])
    try:
        assert len(ens.agents) == 12 and ens.engine.mbpop_info()["n_pops"] == 2
        assert [a.population_index for a in ens.agents] == [0, 1] * 6 and ens.bank_info()["n_kc"].tolist() == [1043, 2003] * 3
        rows = navsim_amd.run_ensemble(ens, frames=40)
    finally:
        ens.agents[0].clear_training()
        ens.engine.close()
    print("completed_frames %r stop_status %r" % ([r["completed_frames"] for r in rows], [r["stop_status"] for r in rows]))
    assert _csv(rows) == _csv(lone_rows)
    assert any(lone_rows[2 * k] != lone_rows[2 * k + 1] for k in range(6))               # the populations tell: twins of one start differ


# ---- 8. ragged weights round trip; leaving a table; the bank-0 calls under one ------------------------------------------------------------
def test_weights_round_trip_and_every_way_out_of_a_table_gives_todays_bits(eng):
    d = HP.table_data()
    pops, of_bank, h, w = d["pops"], d["pop_of_bank"], d["h"], d["w"]
    begin_table(eng, h, w, pops, of_bank)
    for b, wt in enumerate(d["wts"]):
        eng.mbank_set_weights(b, wt)
    got = eng.mbank_read_weights()
    assert all(np.array_equal(g, wt) for g, wt in zip(got, d["wts"]))
    same(eng.mbank_step_batch_u8(d["planes"], d["banks"]), d["fam"], d["best"])
    with pytest.raises(ValueError, match=r"weights must be uint8\[257\]"):
        eng.mbank_set_weights(3, np.ones(63, np.uint8))
    bad = np.ones(257, np.uint8)
    bad[256] = 2
    with pytest.raises(ValueError, match=r"weights\[256\] = 2 is neither 0 nor 1"):       # the 0 / 1 check runs on the bank's own length
        eng.mbank_set_weights(3, bad)
    assert eng._lib.dv_mbank_read_weights(eng._ctx, 7, N.u8ptr(np.empty(2000, np.uint8))) == -1
    assert all(np.array_equal(g, wt) for g, wt in zip(eng.mbank_read_weights(), d["wts"]))
    # the bank-0 calls assume the begin's wiring: refused, naming dv_mbpop_clear, and nothing changes
    views, planes = d["views"], d["planes"]
    for call in (lambda: eng.mb_train_u8(views), lambda: eng.mb_score_u8(views), lambda: eng.mb_activity_u8(views), lambda: eng.mb_step_batch_u8(planes),
                 lambda: eng.mb_read_weights(), lambda: eng.mb_set_weights(np.ones(1, np.uint8))):      # (the sensed ones: test 2)
        with pytest.raises(N.EngineError, match="dv_mbpop_clear.*DV_ERR_STATE"):
            call()
    assert all(np.array_equal(g, wt) for g, wt in zip(eng.mbank_read_weights(), d["wts"]))
    # a refused table leaves the live one as it was
    with pytest.raises(ValueError, match=r"population 1: conn\[62\]\[3\] = 35 outside \[0, 35\)"):
        conn = pops[1]["conn"].astype(np.int32)
        conn[62, 3] = 35
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(N._i32p)
        eng._check(eng._lib.dv_mbpop_set(eng._ctx, 2, i32([1, 63]), i32([1, 4]), i32([1, 7]), i32([2, 2]),
                                         i32(np.concatenate([pops[0]["conn"].ravel(), conn.ravel()])), 1, i32([0])), "dv_mbpop_set")
    assert eng.mbpop_info()["n_pops"] == 5 and all(np.array_equal(g, wt) for g, wt in zip(eng.mbank_read_weights(), d["wts"]))
    # today's calls after a table: dv_mbank_set, dv_mbpop_clear and dv_mb_begin each return to the begin's population
    b = HB.bank_data("7x5_k20000")
    assert (b["h"], b["w"]) == (h, w)

    def todays_bits():
        eng.mbank_train_u8(b["views"], b["bank_of"])
        assert np.array_equal(eng.mbank_read_weights(), b["wts"]) and eng.mbank_info()["n_depressed"].tolist() == b["zeros"].tolist()
        lay = HB.layout_data("7x5_k20000", 5, 13)
        res = eng.mbank_step_batch_u8(lay["planes"], lay["banks"])
        same(res, lay["fam"], lay["best"])
        assert np.array_equal(H.bits(eng.mb_score_u8(b["patches"])), H.bits((-b["nov"][0]).astype(np.float64)))     # bank 0 again

    eng.mb_begin(h, w, b["conn"], b["n_active"], 2)
    eng.mbpop_set(pops, of_bank)
    eng.mbank_set(HB.R)                                                                   # dv_mbank_set drops the table
    assert eng.mbpop_info()["n_pops"] == 0 and eng.mbank_read_weights().shape == (HB.R, b["K"])
    todays_bits()
    eng.mbpop_set(pops, of_bank)
    eng.mbpop_clear()                                                                     # one bank of the begin's population, weights 1
    assert eng.mbpop_info()["n_pops"] == 0 and np.array_equal(eng.mbank_read_weights(), np.ones((1, b["K"]), np.uint8))
    assert eng.mbank_info()["views_trained"].tolist() == [0]
    eng.mbank_set(HB.R)
    todays_bits()
    eng.mbpop_set(pops, of_bank)
    eng.mb_begin(h, w, b["conn"], b["n_active"], 2)                                       # dv_mb_begin drops it too
    assert eng.mbpop_info()["n_pops"] == 0 and eng.mb_banks == 1
    eng.mbank_set(HB.R)
    todays_bits()
    eng.mbpop_set(pops, of_bank)
    eng.mb_end()
    assert eng.mbpop_info()["n_pops"] == 0
    with pytest.raises(N.EngineError, match="DV_ERR_STATE"):                              # no model: no table
        eng.mbpop_set(pops, of_bank)
