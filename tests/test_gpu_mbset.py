"""Bank sets of the mushroom-body model on the device (dv_mbset_*): one selection of firing cells read out through several banks,
against the NumPy statement (tests/helpers_mbset.py on tests/helpers_mushroom.py's fired_mask) -- bit for bit: np.array_equal on the
integers, the scores on their uint64 views.  tests/test_mbset_host.py asserts of every input here that a read-out which takes the set's
entries in another order, drops the last bank or takes its table at the launch's own column gives other numbers."""
import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from tests import helpers_mbset as M
from tests import helpers_mushroom as H
from tests import helpers_noise as HZ

pytestmark = pytest.mark.gpu

STATE, INVALID, SENSE_ERROR = -3, -1, 16


@pytest.fixture(scope="module")
def eng():
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


def begin(e, m, wts):
    e.mb_begin(m["h"], m["w"], m["conn"], m["n_active"], 2)
    e.mbank_set(len(wts))
    for r, w in enumerate(wts):
        e.mbank_set_weights(r, w)


def same(res, want, what=None):
    assert res.angle_familiarity.shape == want["fam"].shape and res.angle_familiarity.dtype == np.float64
    assert res.bank_novelty.dtype == np.int32 and np.array_equal(res.bank_novelty, want["nov"]), what
    bad = np.argwhere(H.bits(res.angle_familiarity) != H.bits(want["fam"]))
    assert len(bad) == 0, (what, bad[:6].tolist(), res.angle_familiarity[tuple(bad[0])], want["fam"][tuple(bad[0])])
    assert res.best_idex.tolist() == np.asarray(want["best"]).tolist(), what


# ---- 1. uploaded planes against the statement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(M.SHAPES))
def test_uploaded_planes_are_the_statement(eng, shape):
    m = M.model(shape)
    begin(eng, m, m["wts"])
    for S in M.SET_SIZES:
        c = M.case(shape, S)
        res = eng.mbset_step_batch_u8(c["planes"], c["banks"], c["coefs"])
        assert not res.flags.any()
        same(res, c, (shape, S))


# ---- 2. the banked step's bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(M.SHAPES))
def test_one_bank_and_a_zero_coefficient_equal_the_banked_step(eng, shape):
    m = M.model(shape)
    begin(eng, m, m["wts"])
    planes = M.layout_planes(shape)
    banks = np.array([0, 3, 1, 4], dtype=np.int32)                                      # (each the bank of its member's planted view)
    want = eng.mbank_step_batch_u8(planes, banks)
    one = eng.mbset_step_batch_u8(planes, banks[:, None], np.ones((4, 1), np.int32))
    two = eng.mbset_step_batch_u8(planes, np.stack([banks, (banks + 1) % M.N_BANKS], axis=1), np.tile(np.array([1, 0], np.int32), (4, 1)))
    for got in (one, two):
        assert np.array_equal(H.bits(got.angle_familiarity), H.bits(want.angle_familiarity))
        assert got.best_idex.tolist() == want.best_idex.tolist() and not got.flags.any()
    assert np.array_equal(one.bank_novelty[..., 0], (-want.angle_familiarity).astype(np.int32))
    assert (want.angle_familiarity == 0).any() and not np.signbit(one.angle_familiarity[want.angle_familiarity == 0]).any()      # +0.0


# ---- 3. constant planes: the rank rule picks ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(M.SHAPES))
def test_constant_planes_count_the_first_cells_of_every_bank(eng, shape):
    m = M.model(shape)
    begin(eng, m, m["wts"])
    for S in M.SET_SIZES:
        c = M.constant_case(shape, S)
        same(eng.mbset_step_batch_u8(c["planes"], c["banks"], c["coefs"]), c, (shape, S))


# ---- 4. a tie across 260 headings, from different pairs ---------------------------------------------------------------------------------
def test_equal_values_from_different_pairs_go_to_the_lower_heading(eng):
    t = M.tie_case()
    begin(eng, t, t["wts"])
    res = eng.mbset_step_batch_u8(t["planes"], t["banks"], t["coefs"])
    same(res, t)
    assert res.best_idex.tolist() == [100, 5]
    assert res.bank_novelty[1, 5].tolist() == [10, 4] and res.bank_novelty[1, 257].tolist() == [8, 2]
    assert res.angle_familiarity[1, 5] == res.angle_familiarity[1, 257] == -6.0


# ---- 5. the second launch begins inside a member ------------------------------------------------------------------------------------------
def test_columns_past_the_launch_bound_uploaded(eng):
    m, w = M.model("7x5"), M.wide_case()
    begin(eng, m, m["wts"])
    res = eng.mbset_step_batch_u8(w["planes"], w["banks"], w["coefs"])
    same(res, w)


def sensed_engine(cfg, table=None):
    e = navsim_amd.FamiliarityEngine(device=0)
    e.set_landscape(HZ.lands()[0])
    e.configure_sensor(cfg["sensor"], cfg["pixel"], HZ.level_table(cfg), cfg["mask"])
    e.lands_set(list(HZ.lands()))
    if table is not None:
        e.sensors_set(*HZ.table_args(table))
    return e


def test_columns_past_the_launch_bound_sensed():
    m, w = M.model("7x5"), M.wide_sensed_case()
    e = sensed_engine(HZ.THIN)
    try:
        begin(e, m, m["wts"])
        res = e.mbset_sense_step_batch(w["xs"], w["ys"], w["angs"], w["banks"], w["coefs"])
        assert not res.flags.any()
        same(res, w)
        twin = e.mbset_step_batch_u8(w["planes"], w["banks"], w["coefs"])
        assert np.array_equal(H.bits(twin.angle_familiarity), H.bits(res.angle_familiarity)) and np.array_equal(twin.bank_novelty, res.bank_novelty)
    finally:
        e.close()


# ---- 6. the sensed calls against their uploaded twins on host-sensed views --------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["own", "lands", "table", "noise", "both"])
def test_sensed_calls_equal_their_uploaded_twins(kind):
    s = M.sensed_case(kind)
    e = sensed_engine(s["cfg"], s["table"])
    try:
        begin(e, dict(h=s["cfg"]["sensor"][1], w=s["cfg"]["sensor"][0], conn=s["conn"], n_active=M.SENSED["n_active"]), s["wts"])
        twin = e.mbset_step_batch_u8(s["planes"], s["banks"], s["coefs"])
        same(twin, s, kind)
        if s["keys"] is not None:
            e.noise_rows(HZ.SEED, s["keys"], s["amp_s"], s["amp_v"])
            with pytest.raises(N.EngineError, match="noise rows are live"):                # (a call without a landscape table: no noise)
                e.mbset_sense_step_batch(s["xs"], s["ys"], s["angs"], s["banks"], s["coefs"])
        res = e.mbset_sense_step_batch(s["xs"], s["ys"], s["angs"], s["banks"], s["coefs"], land_of_member=s["lands"])
        assert not res.flags.any()
        same(res, s, kind)
    finally:
        e.close()


def test_a_member_off_its_landscape_is_flagged_and_the_others_are_untouched():
    s = M.sensed_case("own")
    x, y, off = M.off_facts()
    e = sensed_engine(s["cfg"])
    try:
        begin(e, dict(h=8, w=16, conn=s["conn"], n_active=M.SENSED["n_active"]), s["wts"])
        xs, ys, angs = s["xs"].copy(), s["ys"].copy(), s["angs"].copy()
        xs[2], ys[2], angs[2] = x, y, M.OFF_ANGLES
        for lands in (None, np.zeros(len(xs), np.int32)):
            res = e.mbset_sense_step_batch(xs, ys, angs, s["banks"], s["coefs"], land_of_member=lands)
            assert res.flags.tolist() == [0, 0, SENSE_ERROR, 0, 0] and res.best_idex[2] == -1
            for i in (0, 1, 3, 4):
                assert np.array_equal(H.bits(res.angle_familiarity[i]), H.bits(s["fam"][i])) and res.best_idex[i] == s["best"][i], i
                assert np.array_equal(res.bank_novelty[i], s["nov"][i]), i
        same(e.mbset_sense_step_batch(s["xs"], s["ys"], s["angs"], s["banks"], s["coefs"]), s)      # the next call without it is as before
    finally:
        e.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def _raw(e, planes, banks, coefs, S=None):
    n, A = planes.shape[:2]
    banks, coefs = np.ascontiguousarray(banks, np.int32), np.ascontiguousarray(coefs, np.int32)
    fam, best, nov = np.zeros((n, A)), np.zeros(n, np.int32), np.zeros((n, A, max(banks.shape[1], 1)), np.int32)
    i32 = lambda a: a.ctypes.data_as(N._i32p)
    rc = e._lib.dv_mbset_step_u8(e._ctx, N.u8ptr(planes), n, A, banks.shape[1] if S is None else S, i32(banks), i32(coefs), N.f64ptr(fam),
                                 i32(best), i32(nov))
    return rc, e._lib.dv_last_error(e._ctx).decode()


def test_refusals_come_before_the_device(eng):
    m = M.model("7x5")
    begin(eng, m, m["wts"])
    c = M.case("7x5", 2)
    planes = np.ascontiguousarray(c["planes"])
    before = eng.mbank_read_weights()
    for S in (0, 9):
        rc, msg = _raw(eng, planes, np.zeros((4, 9), np.int32), np.ones((4, 9), np.int32), S)
        assert rc == INVALID and ("set_size %d" % S) in msg
    for bad in (M.N_BANKS, -1):
        banks = c["banks"].copy()
        banks[3, 1] = bad
        rc, msg = _raw(eng, planes, banks, c["coefs"])
        assert rc == INVALID and ("banks[3][1] = %d" % bad) in msg
        with pytest.raises(ValueError, match=r"bank_sets\[3\]\[1\] = %d outside" % bad):
            eng.mbset_step_batch_u8(planes, banks, c["coefs"])
    # the overflow bound: sum |coefs| n_active <= 2^31 - 1
    top = M.overflow_bound(m["n_active"])
    coefs = c["coefs"].copy()
    coefs[2] = (top - 5, -5)
    rc, _ = _raw(eng, planes, c["banks"], coefs)
    assert rc == 0
    coefs[2] = (top - 5, -6)
    rc, msg = _raw(eng, planes, c["banks"], coefs)
    assert rc == INVALID and "member 2" in msg and "2^31 - 1" in msg
    with pytest.raises(ValueError, match="member 2"):
        eng.mbset_step_batch_u8(planes, c["banks"], coefs)
    # a live population table: banks of different populations share no selection
    from navsim_amd.util import mushroom_population
    pop = mushroom_population(m["w"] * m["h"], n_kc=m["K"], fan_in=m["c"], sparsity=m["n_active"] / m["K"], seed=1, channel=2)
    eng.mbpop_set([pop], [0] * M.N_BANKS)
    try:
        rc, msg = _raw(eng, planes, c["banks"], c["coefs"])
        assert rc == STATE and "population table is live" in msg
    finally:
        eng.mbpop_clear()
    begin(eng, m, before)
    same(eng.mbset_step_batch_u8(planes, c["banks"], c["coefs"]), c)                      # ... and nothing has changed
    assert np.array_equal(eng.mbank_read_weights(), before)


def test_set_calls_without_a_model_are_state_errors():
    e = navsim_amd.FamiliarityEngine(device=0)
    try:
        rc, msg = _raw(e, np.zeros((2, 3, 5, 7), np.uint8), np.zeros((2, 2), np.int32), np.ones((2, 2), np.int32))
        assert rc == STATE and "no mushroom-body model" in msg
        z, t = np.zeros(2), np.zeros((2, 2), np.int32)
        best, flags = np.zeros(2, np.int32), np.zeros(2, np.uint32)
        i32 = lambda a: a.ctypes.data_as(N._i32p)
        assert e._lib.dv_mbset_sense_step(e._ctx, N.f64ptr(z), N.f64ptr(z), N.f64ptr(z), 2, 1, 2, i32(t), i32(t), N.f64ptr(z), i32(best),
                                          flags.ctypes.data_as(N._u32p), None) == STATE
        assert e._lib.dv_mbset_lands_sense_step(e._ctx, N.f64ptr(z), N.f64ptr(z), N.f64ptr(z), 2, 1, 2, i32(t), i32(t), i32(best), N.f64ptr(z),
                                                i32(best), flags.ctypes.data_as(N._u32p), None) == STATE
        m = M.model("7x5")
        begin(e, m, m["wts"])
        assert e._lib.dv_mbset_sense_step(e._ctx, N.f64ptr(z), N.f64ptr(z), N.f64ptr(z), 2, 1, 2, i32(t), i32(t), N.f64ptr(z), i32(best),
                                          flags.ctypes.data_as(N._u32p), None) == STATE       # a model but no sensor
    finally:
        e.close()


# ---- 8. two engines whose models need different LDS, in turn ----------------------------------------------------------------------------
def test_two_engines_of_different_lds_step_in_turn(eng):
    big, small = M.model("33x31"), M.model("7x5")
    begin(eng, big, big["wts"])
    e2 = navsim_amd.FamiliarityEngine(device=0)
    try:
        begin(e2, small, small["wts"])                                                   # the small model is begun last
        cb, cs = M.case("33x31", 8), M.case("7x5", 3)
        for _ in range(2):
            same(eng.mbset_step_batch_u8(cb["planes"], cb["banks"], cb["coefs"]), cb, "big")
            same(e2.mbset_step_batch_u8(cs["planes"], cs["banks"], cs["coefs"]), cs, "small")
    finally:
        e2.close()


# ---- 9. the opponent ensemble ---------------------------------------------------------------------------------------------------------------
from navsim_amd import mushroom_familiarity, synth  # noqa: E402
from tests import helpers_mushroom_banks as HB  # noqa: E402

RE = navsim_amd.MushroomRouteEnsemble
STEPS = 15


def make_agent(model=None, gpu=True):
    return navsim_amd.NavBySceneFamiliarity(synth.synth_landscape(3, 300, 4), M.ENS_SENSOR, 1.0, n_test_angles=M.ENS_ANGLES, use_gpu_sensor=gpu,
                                            familiarity_model=model or mushroom_familiarity(**M.ENS_MODEL))


def rows_of(ens):
    return [(H.bits(a.angle_familiarity).tolist(), tuple(a.position), float(a.angle)) for a in ens.agents], list(ens.stop_status)


def test_gain_zero_is_the_plain_ensemble_and_the_members_carry_their_banks():
    paths = HB.routes()
    starts = HB.starts(paths)
    plain = RE.from_routes_with(make_agent(), paths, starts)
    opp = RE.from_routes_with(make_agent(), paths, starts, opponent=dict(turn=np.pi, gain=0))
    calls = []
    inner = opp.engine.mbset_sense_step_batch
    opp.engine.mbset_sense_step_batch = lambda *a, **k: calls.append((np.array(a[3]).tolist(), np.array(a[4]).tolist())) or inner(*a, **k)
    try:
        R = len(paths)
        assert [a.memory_bank for a in opp.agents] == [0, 0, 1, 1, 2, 2] and [a.repulsive_bank for a in opp.agents] == [3, 3, 4, 4, 5, 5]
        assert [a.opponent_gain for a in opp.agents] == [0] * 6 and all(a.repulsive_bank is None for a in plain.agents)
        with pytest.raises(ValueError, match="MushroomRouteEnsemble"):                     # a member steps with its ensemble only
            opp.agents[1].step_forward()
        info = opp.bank_info()
        assert info["n_banks"] == 2 * R and info["views_trained"].tolist() == 2 * [len(p) for p in paths] and len(info["n_kc"]) == 2 * R
        for m, p in zip(opp.agents, plain.agents):
            assert np.array_equal(m.familiar_scenes, p.familiar_scenes) and m.bank_novelty is None
            route, hd = m.training_path, H.route_headings(m.training_path)
            assert np.array_equal(m.repulsive_scenes, opp.engine.sense(route[:, 0], route[:, 1], hd + np.pi))
            assert not np.array_equal(m.repulsive_scenes, m.familiar_scenes)
        for r in range(R):
            assert np.array_equal(opp.engine.mbank_read_weights(r), plain.engine.mbank_read_weights(r))
            assert not np.array_equal(opp.engine.mbank_read_weights(R + r), opp.engine.mbank_read_weights(r))
        for t in range(STEPS):
            before = list(opp.active)
            plain.step_forward()
            opp.step_forward()
            assert len(calls) == t + 1                                                   # ONE device call a step
            assert calls[-1] == ([[opp.agents[i].memory_bank, opp.agents[i].repulsive_bank] for i in before], [[1, 0]] * len(before))
            assert rows_of(opp) == rows_of(plain), t
        nov = opp.agents[0].bank_novelty
        assert nov.shape == (M.ENS_ANGLES, 2) and nov.dtype == np.int32
        assert np.array_equal(H.bits(opp.agents[0].angle_familiarity), H.bits((-nov[:, 0]).astype(np.float64)))
    finally:
        opp.engine.mbset_sense_step_batch = inner
        opp.agents[0].clear_training()
        plain.agents[0].clear_training()


def test_gain_one_equals_shadow_agents_whose_sensor_and_memories_run_in_numpy():
    paths = HB.routes()
    starts = HB.starts(paths)
    opp = RE.from_routes_with(make_agent(), paths, starts, opponent=dict(turn=np.pi, gain=1))
    shadows = []
    for r, pos, ang in starts:
        probe = make_agent(gpu=False)
        hd = H.route_headings(paths[r])
        rep = np.stack([probe.get_sensor_mat((x, y), a + np.pi) for (x, y), a in zip(paths[r], hd)])
        s = make_agent(M.numpy_opponent_model(rep, 1, **M.ENS_MODEL), gpu=False)
        s.train_from_path(paths[r])
        s.position, s.angle = pos, ang
        shadows.append(s)
    try:
        for m, s in zip(opp.agents, shadows):
            assert np.array_equal(opp.engine.mbank_read_weights(m.memory_bank), s._familiarity_func.wts[0])
            assert np.array_equal(opp.engine.mbank_read_weights(m.repulsive_bank), s._familiarity_func.wts[1])
        seen, both = set(), 0
        for t in range(STEPS):
            opp.step_forward()
            for s in shadows:
                if s.stopped_with_exception is None:
                    try:
                        s.step_forward()
                    except navsim_amd.StopNavigationException as stop:
                        s.stopped_with_exception = stop
            for i, (m, s) in enumerate(zip(opp.agents, shadows)):
                assert m.position == s.position and m.angle == s.angle, (t, i)
                assert np.array_equal(H.bits(m.angle_familiarity), H.bits(s.angle_familiarity)), (t, i, m.angle_familiarity, s.angle_familiarity)
                code = s.stopped_with_exception.get_code() if s.stopped_with_exception is not None else 0
                assert opp.stop_status[i] == code, (t, i)
                seen.update(m.angle_familiarity.tolist())
                both += int((m.bank_novelty[:, 1] > 0).any())
        assert len(seen) > 3 and both > 0                                                # the repulsive memory takes part
    finally:
        opp.agents[0].clear_training()


def noisy_agent():
    c = HZ.ENS
    return navsim_amd.NavBySceneFamiliarity(np.array(HZ.lands()[0]), c["sensor"], HZ.ENS_STEP, n_test_angles=HZ.ENS_ANGLES, use_gpu_sensor=True,
                                            n_sensor_levels=c["levels"], familiarity_model=mushroom_familiarity(**HZ.ENS_MB))


def noisy(members=None, **kw):
    starts, noise = HZ.ens_starts(), HZ.ENS_NOISE
    if members is not None:
        starts = [starts[i] for i in members]
        noise = dict(noise, amp_v=[noise["amp_v"][i] for i in members], streams=[noise["streams"][i] for i in members])
    return RE.from_landscapes(noisy_agent(), list(HZ.lands()), HZ.ens_routes(), starts, noise=noise, **kw)


def test_from_landscapes_under_noise_gain_zero_and_a_member_alone():
    plain, zero = noisy(), noisy(opponent=dict(gain=0))
    gains = [1, 2, 0, 3]
    opp = noisy(opponent=dict(turn=[np.pi, 2.0], gain=gains))
    try:
        for r, (l, route) in enumerate(HZ.ens_routes()):
            m = next(a for a in opp.agents if a.memory_bank == r)
            assert np.array_equal(m.familiar_scenes, HZ.ens_train_views()[r])              # the attractive keys are unchanged
            hd = HZ.route_headings(route) + (np.pi, 2.0)[r]
            want = np.stack([HZ.view(HZ.lands()[l], HZ.ENS, route[v][0], route[v][1], hd[v], HZ.ENS_NOISE["seed"], M.repulsive_key(r, v), 0,
                                     HZ.ENS_NOISE["train_amp_s"], HZ.ENS_NOISE["train_amp_v"][r]) for v in range(len(route))])
            assert np.array_equal(m.repulsive_scenes, want), r
        assert opp.engine.noise_info()["n_rows"] == 0
        traces, differs = [], False
        for t in range(6):
            for e in (plain, zero, opp):
                e.step_forward()
            assert rows_of(zero) == rows_of(plain), t
            traces.append(rows_of(opp))
            differs = differs or traces[-1][0] != rows_of(plain)[0]
        assert differs                                                                   # (the gains above 0 show)
        for i in (1, 3):
            one = noisy(members=[i], opponent=dict(turn=[np.pi, 2.0], gain=[gains[i]]))
            try:
                for t in range(6):
                    one.step_forward()
                    got, codes = rows_of(one)
                    assert got[0] == traces[t][0][i] and codes[0] == traces[t][1][i], (i, t)
            finally:
                one.agents[0].clear_training()
    finally:
        for e in (plain, zero, opp):
            e.agents[0].clear_training()


def test_run_ensemble_rows_come_out_of_an_opponent_ensemble():
    paths = HB.routes()
    starts = HB.starts(paths)
    opp = RE.from_routes_with(make_agent(), paths, starts, opponent=dict(gain=[1, 2, 1, 2, 1, 2]))
    try:
        rows = navsim_amd.run_ensemble(opp, frames=8)
        assert len(rows) == len(starts) and all(0 < r["completed_frames"] <= 8 for r in rows)
        assert [r["stop_status"] for r in rows] == list(opp.stop_status)
    finally:
        opp.agents[0].clear_training()
