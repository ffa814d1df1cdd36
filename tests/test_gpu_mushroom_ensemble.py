"""Ensembles of mushroom-body agents on the device: the batch calls (dv_batch_mb_step_u8 / dv_batch_mb_sense_step) against the NumPy
statement (tests/helpers_mushroom.py) and against the single-agent calls, bit for bit -- the model is integer arithmetic, so every
comparison is np.array_equal, floats through their uint64 view; MushroomEnsemble against agents stepping alone.

Shapes (tests/helpers_mushroom_ensemble.py): the small cases of helpers_mushroom under member layouts of one member, one heading per
member, ragged members, a member wider than a wave and one wider than k_mb_decide_batch's workgroup; the 256x256 plane (130 896 bytes
of LDS); 8193 columns (one more than a launch) and 4097 planes of 128x128 (one more than 64 MiB of staged bytes); the 32x32 sensor
with a fan-in of 10 and of 16 (66 384 bytes of LDS, over what a launch gets without the function's attribute)."""
import csv
import io

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import mushroom_familiarity, synth
from tests import helpers_infomax as HI
from tests import helpers_mushroom as H
from tests import helpers_mushroom_ensemble as HE

pytestmark = pytest.mark.gpu

STATE, INVALID, SENSE_ERROR = -3, -1, 16


@pytest.fixture(scope="module")
def eng():
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


def begin(e, d):
    e.mb_begin(d["h"], d["w"], d["conn"], d["n_active"], 2)
    e.mb_set_weights(d["wt"])


def same(res, fam, best):
    assert res.angle_familiarity.shape == fam.shape and res.angle_familiarity.dtype == np.float64
    bad = np.argwhere(H.bits(res.angle_familiarity) != H.bits(fam))
    assert len(bad) == 0, (bad[:6].tolist(), res.angle_familiarity[tuple(bad[0])], fam[tuple(bad[0])])
    assert res.best_idex.tolist() == np.asarray(best).tolist()


# ---- 1. uploaded planes against the statement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,n,A", HE.CASES)
def test_step_batch_u8_is_the_statement(eng, key, n, A):
    e = HE.ensemble_data(key, n, A)
    begin(eng, e)
    res = eng.mb_step_batch_u8(e["planes"])
    assert res.best_idex.shape == (n,) and res.flags.shape == (n,) and not res.flags.any()
    same(res, e["fam"], e["best"])
    flat = eng.mb_score_u8(e["planes"].reshape(n * A, e["h"], e["w"]))                   # ... and the single call, per column
    assert np.array_equal(H.bits(res.angle_familiarity).reshape(-1), H.bits(flat))
    if e["planted"] is not None:
        a0, a1 = HE.planted_headings(A)
        assert res.best_idex[e["planted"]] == a0                                         # the first of two equal maxima
        assert H.bits(res.angle_familiarity[e["planted"], [a0, a1]]).tolist() == [0, 0]  # +0.0
    again = eng.mb_step_batch_u8(e["planes"])
    same(again, e["fam"], e["best"])


# ---- 2. columns past one launch ------------------------------------------------------------------------------------------------------
def test_columns_past_the_view_bound_of_a_launch(eng):
    s = HE.slab_data()
    begin(eng, s)
    n, A = s["pick"].shape
    planes = s["two"][s["pick"]]                                                         # uint8[3, 2731, 3, 5]
    whole = eng.mb_step_batch_u8(planes)
    same(whole, s["fam"], s["best"])
    flat = planes.reshape(n * A, s["h"], s["w"])
    views, _ = H.slab_views()
    cut = [eng.mb_step_batch_u8(flat[None, :views]), eng.mb_step_batch_u8(flat[None, views:])]
    got = np.concatenate([c.angle_familiarity.reshape(-1) for c in cut])
    assert np.array_equal(H.bits(got), H.bits(whole.angle_familiarity).reshape(-1))
    assert cut[1].angle_familiarity.shape == (1, 1) and H.bits(cut[1].angle_familiarity)[0, 0] == 0 and cut[1].best_idex.tolist() == [0]
    for i in range(n):
        one = eng.mb_step_batch_u8(planes[i:i + 1])
        same(one, s["fam"][i:i + 1], s["best"][i:i + 1])


def test_columns_past_the_byte_bound_of_a_launch(eng):
    b = HE.bytes_data()
    begin(eng, b)
    res = eng.mb_step_batch_u8(b["two"][b["pick"]])                                      # uint8[1, 4097, 128, 128]
    same(res, b["fam"], b["best"])


# ---- 3. sensed columns -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sensed():
    """An agent with a 32x32 sensor on synth_landscape(3, 300, 4); its engine holds the landscape and the sensor."""
    agent = HI.sensed_agent(mushroom_familiarity(**HE.SENSED_MODELS["c10"]), True)
    yield agent._engine
    agent._engine.close()


def begin_sensed(e, name):
    conn, n_active, wt = HE.sensed_model(name)
    e.mb_begin(32, 32, conn, n_active, 2)
    path = HI.sensed_route()
    e.mb_train_from_poses(path[:, 0], path[:, 1], H.route_headings(path), want_views=False)
    assert np.array_equal(e.mb_read_weights(), wt)                                       # (the device's training is the statement's)


@pytest.mark.parametrize("name,A", [("c10", 9), ("c10", 13), ("c16", 9)])
def test_sense_step_batch_is_five_single_steps_and_the_statement(sensed, name, A):
    e = sensed
    begin_sensed(e, name)
    xs, ys, centre = HE.sensed_poses(A)
    angs = (centre[:, None] + np.linspace(-np.pi / 2, np.pi / 2, A)[None, :]) % (2 * np.pi)
    single = [e.mb_sense_step(xs[i], ys[i], angs[i]) for i in range(5)]
    res = e.mb_sense_step_batch(xs, ys, angs)
    assert not res.flags.any()
    for i, (best, fam) in enumerate(single):
        assert np.array_equal(H.bits(res.angle_familiarity[i]), H.bits(fam)), i
        assert res.best_idex[i] == best == int(np.argmax(fam)), i
    want = HE.sensed_statement(name, xs, ys, angs)
    same(res, want, np.argmax(want, axis=1))
    # member 2 moves to where a corner of the rotated footprint leaves the landscape: the sensor's defined error, flagged per member
    xs2, ys2, angs2 = xs.copy(), ys.copy(), angs.copy()
    xs2[2] = ys2[2] = 283.4                                                              # r = 16: inside the bounds test (x, y < 284)
    angs2[2] = (0.8 + np.pi / 2 + np.linspace(-np.pi / 2, np.pi / 2, A)) % (2 * np.pi)
    with pytest.raises(IndexError):
        e.mb_sense_step(xs2[2], ys2[2], angs2[2])
    res2 = e.mb_sense_step_batch(xs2, ys2, angs2)
    assert res2.flags.tolist() == [0, 0, SENSE_ERROR, 0, 0] and res2.best_idex[2] == -1
    for i in (0, 1, 3, 4):
        assert np.array_equal(H.bits(res2.angle_familiarity[i]), H.bits(res.angle_familiarity[i])), i
        assert res2.best_idex[i] == res.best_idex[i], i
    # ... and the next call without it is as before
    res3 = e.mb_sense_step_batch(xs, ys, angs)
    assert not res3.flags.any()
    same(res3, want, np.argmax(want, axis=1))


def slab_pose_model():
    m = H.SLAB_POSES
    conn = H.connectivity(m["K"], 1024, m["c"], m["seed"])
    x, y = H.step_xy()
    two = H.host_sensed_planes(x, y, m["angles"])
    wt = H.train(np.ones(m["K"], np.uint8), two[1:], conn, m["n_active"])                # trained on the second heading's view alone
    return dict(conn=conn, n_active=m["n_active"], wt=wt, h=32, w=32, two=two)


def test_sensed_columns_past_the_view_bound(sensed):
    """3 members x 2731 headings over the full circle with the SLAB_POSES model: the pose index crosses the launch bound inside
    member 2; each member's row is a lone mb_sense_step's."""
    e = sensed
    begin(e, slab_pose_model())
    x, y = H.step_xy()
    n, A = HE.SLAB_MEMBERS, HE.SLAB_HEADINGS
    xs = x + np.array([0.0, 0.7, -0.5])
    ys = y + np.array([0.0, -0.4, 0.6])
    angs = np.stack([(shift + H.circle_angles(A)) % (2 * np.pi) for shift in (0.0, 0.01, 0.02)])
    res = e.mb_sense_step_batch(xs, ys, angs)
    assert res.angle_familiarity.shape == (n, A) and not res.flags.any()
    for i in range(n):
        best, fam = e.mb_sense_step(xs[i], ys[i], angs[i])
        assert np.array_equal(H.bits(res.angle_familiarity[i]), H.bits(fam)), i
        assert res.best_idex[i] == best, i
        assert len(np.unique(fam)) > 1
    assert np.all(res.angle_familiarity <= 0)


# ---- 4. two engines ----------------------------------------------------------------------------------------------------------------------
def test_two_engines_take_turns():
    a1 = HI.sensed_agent(mushroom_familiarity(**HE.SENSED_MODELS["c16"]), True)
    a2 = HI.sensed_agent(mushroom_familiarity(**HE.SENSED_MODELS["c10"]), True)
    e1, e2 = a1._engine, a2._engine
    try:
        begin_sensed(e1, "c16")
        begin(e2, slab_pose_model())
        A = 9
        xs, ys, centre = HE.sensed_poses(A)
        angs = (centre[:, None] + np.linspace(-np.pi / 2, np.pi / 2, A)[None, :]) % (2 * np.pi)
        want1 = HE.sensed_statement("c16", xs, ys, angs)
        m = slab_pose_model()
        planes = H.host_sensed_planes(np.repeat(xs, A), np.repeat(ys, A), angs.reshape(-1))
        want2 = (-HE.novelty(m["wt"], planes, m["conn"], m["n_active"])).astype(np.float64).reshape(5, A)
        assert not np.array_equal(want1, want2)
        for _ in range(2):
            same(e1.mb_sense_step_batch(xs, ys, angs), want1, np.argmax(want1, axis=1))
            same(e2.mb_sense_step_batch(xs, ys, angs), want2, np.argmax(want2, axis=1))
            same(e1.mb_step_batch_u8(planes.reshape(5, A, 32, 32)), want1, np.argmax(want1, axis=1))
            same(e2.mb_step_batch_u8(planes.reshape(5, A, 32, 32)), want2, np.argmax(want2, axis=1))
    finally:
        e1.close()
        e2.close()


# ---- 5, 6. MushroomEnsemble against agents stepping alone ----------------------------------------------------------------------------
SENSOR = (12, 10)                                                     # (w, h): N = 120, as tests/test_gpu_mushroom.py
AGENT_MODEL = dict(n_kc=1043, fan_in=8, sparsity=0.02, seed=6)


def make_agent(track=True):
    land = synth.synth_landscape(3, 300, 4)
    return navsim_amd.NavBySceneFamiliarity(land, SENSOR, 1.0, n_test_angles=9, use_gpu_sensor=True, track_scene_familiarity=track,
                                            familiarity_model=mushroom_familiarity(**AGENT_MODEL))


def route():
    return synth.sin_training_path(0.5, 60, 180, arclen=1.0)[:45]


def _poses(path):
    """Six start poses: two on the route, two beside it, one within r of the landscape's edge, one a few steps before the path's end."""
    out = []
    for k, (dx, dy, da) in zip((3, 10, 18, 26), ((0.0, 0.0, 0.0), (-0.5, 0.6, -0.2), (0.0, 0.0, 0.0), (-0.8, -0.3, -0.1))):
        d = path[k + 1] - path[k]
        out.append(((float(path[k][0] + dx), float(path[k][1] + dy)), float((np.arctan2(d[1], d[0]) + da) % (2 * np.pi))))
    out.append(((4.0, 150.0), 0.3))
    d = path[-1] - path[-2]
    out.append(((float(path[-5][0]), float(path[-5][1])), float(np.arctan2(d[1], d[0]) % (2 * np.pi))))
    return out


def _trained(path, track=True):
    a = make_agent(track)
    a.train_from_path(path)
    return a


@pytest.mark.parametrize("track", [True, False])
def test_mushroom_ensemble_members_equal_lone_agents(track):
    path = route()
    poses = _poses(path)
    ens = navsim_amd.MushroomEnsemble.from_agent(_trained(path, track), poses)
    calls = []
    inner = ens.engine.mb_sense_step_batch

    def counted(*a, **k):
        calls.append(len(a[0]))
        return inner(*a, **k)
    ens.engine.mb_sense_step_batch = counted
    alone = []
    for pos, ang in poses:
        a = _trained(path, track)
        a.position, a.angle = pos, ang
        alone.append(a)
    try:
        assert isinstance(ens, navsim_amd.NavEnsemble) and len(ens.agents) == 6
        assert all(a._metric_slot == j for j, a in enumerate(ens.agents))                # the metrics' batched device path
        seen = set()
        for t in range(40):
            before = list(ens.active)
            n_calls = len(calls)
            ens.step_forward(fake=False)
            assert len(calls) == n_calls + (1 if before else 0), t                      # ONE batched engine call per step
            for a in alone:
                if a.stopped_with_exception is None:
                    try:
                        a.step_forward(fake=False)
                    except navsim_amd.StopNavigationException as stop:
                        a.stopped_with_exception = stop
            for i, (m, a) in enumerate(zip(ens.agents, alone)):
                assert m.position == a.position and m.angle == a.angle, (t, i)
                assert np.array_equal(H.bits(m.angle_familiarity), H.bits(a.angle_familiarity)), (t, i)
                if track:
                    assert np.array_equal(H.bits(m.scene_familiarity), H.bits(a.scene_familiarity)), (t, i)
                code = a.stopped_with_exception.get_code() if a.stopped_with_exception is not None else 0
                assert ens.stop_status[i] == code, (t, i)
                if a._n_navigation_error or m._n_navigation_error:
                    assert m.navigation_error == a.navigation_error and m.percent_recapitulated == a.percent_recapitulated, (t, i)
            for i in before:
                if ens.stop_status[i] != -2:                                             # (every member that was scored in this step)
                    m = ens.agents[i]
                    seen.update(m.angle_familiarity.tolist())
                    if track:
                        assert m.scene_familiarity.shape == (len(path),) and np.all(m.scene_familiarity == m.angle_familiarity.min()), (t, i)
        assert len(seen) > 3 and max(seen) == 0.0                                        # (views of several novelties, trained ones too)
        # the member inside the bounds margin never sensed; the one near the path's end reached it
        assert ens.stop_status[4] == -2 and np.isnan(ens.agents[4].angle_familiarity).all()
        assert ens.stop_status[5] == 1 and isinstance(ens.agents[5].stopped_with_exception, navsim_amd.ReachedEndOfTrainingPathException)
        assert calls[0] == 5                                                             # member 4 was not sent to the device
        if track:
            rows = ens.scene_familiarity()
            assert rows.shape == (6, len(path)) and np.isposinf(rows[4]).all()
            for i in (0, 1, 2, 3, 5):
                assert np.all(rows[i] == ens.agents[i].angle_familiarity.min()), i
        else:
            with pytest.raises(ValueError, match="track_scene_familiarity=True"):
                ens.scene_familiarity()
    finally:
        ens.engine.mb_sense_step_batch = inner
        ens.agents[0].clear_training()
        for a in alone:
            a.clear_training()


def _csv(rows):
    out = io.StringIO()
    w = csv.DictWriter(out, fieldnames=sorted(rows[0]))
    w.writeheader()
    w.writerows(rows)
    return out.getvalue()


def test_run_ensemble_rows_equal_run_experiment_rows():
    path = route()
    poses = _poses(path)
    ens = navsim_amd.MushroomEnsemble.from_agent(_trained(path), poses)
    try:
        rows = navsim_amd.run_ensemble(ens, frames=40)
    finally:
        ens.agents[0].clear_training()
    assert len(rows) == 6
    wants = []
    for i, (pos, ang) in enumerate(poses):
        a = _trained(path)
        try:
            a.position, a.angle = pos, ang
            if i == 4:
                # the agent that never stepped has no error yet: run_experiment's row divides 0 by 0 (run_ensemble reports NaN there);
                # the other keys are taken from the agent as run_experiment takes them
                with pytest.raises(ZeroDivisionError):
                    navsim_amd.run_experiment(a, frames=40)
                want = dict(path_coverage=a.percent_recapitulated, rmsd_error=float("nan"), completed_frames=0,
                            stop_status=a.stopped_with_exception.get_code(), n_captures=a.n_captures(n_consecutive_scenes=0.05),
                            percent_forgiving=a.percent_recapitulated_forgiving(n_consecutive_scenes=0.05))
            else:
                want = navsim_amd.run_experiment(a, frames=40)
        finally:
            a.clear_training()
        wants.append(want)
    assert _csv(rows) == _csv(wants)
    assert np.isnan(rows[4]["rmsd_error"]) and rows[4]["stop_status"] == -2 and rows[4]["completed_frames"] == 0
    assert rows[5]["stop_status"] == 1 and 0 < rows[5]["completed_frames"] < 10
    assert any(r["completed_frames"] == 40 for r in rows)


# ---- 7. state and argument errors ----------------------------------------------------------------------------------------------------
def _raw(e, planes, n, A, fam, best, flags, xy, ang):
    bp, fp = best.ctypes.data_as(N._i32p), flags.ctypes.data_as(N._u32p)
    return (e._lib.dv_batch_mb_step_u8(e._ctx, N.u8ptr(planes), n, A, N.f64ptr(fam), bp),
            e._lib.dv_batch_mb_sense_step(e._ctx, N.f64ptr(xy), N.f64ptr(xy), N.f64ptr(ang), n, A, N.f64ptr(fam), bp, fp))


def test_batch_calls_without_a_model_are_state_errors():
    e = navsim_amd.FamiliarityEngine(device=0)
    try:
        fam, best, flags = np.zeros(2), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.uint32)
        planes = np.zeros((1, 2, 3, 5), dtype=np.uint8)
        xy, ang = np.ones(1), np.zeros(2)
        assert _raw(e, planes, 1, 2, fam, best, flags, xy, ang) == (STATE, STATE)
        with pytest.raises(navsim_amd.EngineError, match="DV_ERR_STATE"):
            e.mb_step_batch_u8(planes)
        with pytest.raises(navsim_amd.EngineError, match="DV_ERR_STATE"):
            e.mb_sense_step_batch(xy, xy, ang[None])
        # a model but no sensor: the sensed call alone is a state error
        e.mb_begin(3, 5, H.connectivity(37, 15, 10, 1), 4)
        assert _raw(e, planes, 1, 2, fam, best, flags, xy, ang) == (0, STATE)
        # ... and after end
        e.mb_end()
        assert _raw(e, planes, 1, 2, fam, best, flags, xy, ang) == (STATE, STATE)
    finally:
        e.close()


def test_batch_calls_reject_bad_arguments_and_keep_the_model(sensed):
    e = sensed
    begin_sensed(e, "c10")
    xs, ys, centre = HE.sensed_poses(9)
    angs = (centre[:, None] + np.linspace(-np.pi / 2, np.pi / 2, 9)[None, :]) % (2 * np.pi)
    want = HE.sensed_statement("c10", xs, ys, angs)
    same(e.mb_sense_step_batch(xs, ys, angs), want, np.argmax(want, axis=1))
    planes = np.zeros((2, 3, 32, 32), dtype=np.uint8)
    fam, best, flags = np.zeros(6), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.uint32)
    xy, ang = np.full(2, 100.0), np.zeros(6)
    bp, fp = best.ctypes.data_as(N._i32p), flags.ctypes.data_as(N._u32p)
    lib, ctx = e._lib, e._ctx
    assert _raw(e, planes, 0, 3, fam, best, flags, xy, ang) == (INVALID, INVALID)
    assert _raw(e, planes, 2, 0, fam, best, flags, xy, ang) == (INVALID, INVALID)
    assert lib.dv_batch_mb_step_u8(ctx, None, 2, 3, N.f64ptr(fam), bp) == INVALID
    assert lib.dv_batch_mb_step_u8(ctx, N.u8ptr(planes), 2, 3, None, bp) == INVALID
    assert lib.dv_batch_mb_step_u8(ctx, N.u8ptr(planes), 2, 3, N.f64ptr(fam), None) == INVALID
    assert lib.dv_batch_mb_step_u8(ctx, N.u8ptr(planes), 65536, 65536, N.f64ptr(fam), bp) == INVALID      # columns that fit no int
    good = (N.f64ptr(xy), N.f64ptr(xy), N.f64ptr(ang), 2, 3, N.f64ptr(fam), bp, fp)
    for k in (0, 1, 2, 5, 6, 7):
        args = list(good)
        args[k] = None
        assert lib.dv_batch_mb_sense_step(ctx, *args) == INVALID, k
    assert lib.dv_batch_mb_sense_step(ctx, *good) == 0
    with pytest.raises(ValueError):
        e.mb_step_batch_u8(np.zeros((2, 3, 5, 3), dtype=np.uint8))                       # planes of another shape
    # the model that was there before the refusals still scores as before
    same(e.mb_sense_step_batch(xs, ys, angs), want, np.argmax(want, axis=1))
    # a model of another shape than the sensor's
    e.mb_begin(3, 5, H.connectivity(37, 15, 10, 1), 4)
    with pytest.raises(ValueError, match="the sensor is 32x32 but the model takes 5x3"):
        e.mb_sense_step_batch(xs, ys, angs)
    assert lib.dv_batch_mb_sense_step(e._ctx, *good) == INVALID
    assert e.mb_step_batch_u8(np.zeros((2, 3, 3, 5), dtype=np.uint8)).angle_familiarity.shape == (2, 3)
