"""Ensembles of Infomax agents on the device: the batch calls against the single-agent calls, bit for bit, and against the NumPy
restatement (tests/helpers_infomax.py) within its own tolerance; InfomaxEnsemble against agents stepping alone.

Shapes: the small cases of tests/helpers_infomax.py -- (20,13) with 70 rows (vector loads, a ragged row tile), (40,1) with 24 rows,
(5,3) (the scalar-load path), (16,16), and (7,5) with 1043 rows and (32,32) with 1040 (more than 64 row tiles: k_im_decide's sum over
a column's tiles takes a second trip, compared with k_im_dfinish's on the same wrapped loop) -- under member layouts that put a single member, one heading per member, a member across a
block of 64 columns, a ragged last block and a member wider than a block through the column grid (tests/helpers_infomax_ensemble.py)."""

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import infomax_familiarity, synth
from tests import helpers_infomax as H
from tests import helpers_infomax_ensemble as HE

pytestmark = pytest.mark.gpu

SENSOR = (12, 10)                                                     # (w, h): N = 120, as tests/test_gpu_infomax.py


@pytest.fixture(scope="module")
def eng():
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


def make_agent(model, n_test_angles=9):
    land = synth.synth_landscape(3, 300, 4)
    return navsim_amd.NavBySceneFamiliarity(land, SENSOR, 1.0, n_test_angles=n_test_angles, use_gpu_sensor=True, familiarity_model=model)


def route():
    return synth.sin_training_path(0.5, 60, 180, arclen=1.0)[:45]


# ---- 1. uploaded patches: the batch call against score_u8 and the restatement -------------------------------------------------------
@pytest.mark.parametrize("n,A", HE.LAYOUTS)
@pytest.mark.parametrize("key", HE.KEYS)
def test_step_batch_u8_is_score_u8_per_column(eng, key, n, A):
    e = HE.ensemble_data(key, n, A)
    eng.infomax_begin(e["h"], e["w"], e["W0"], 2, H.ETA)
    eng.infomax_set_weights(e["W"])
    res = eng.infomax_step_batch_u8(e["planes"])
    assert res.angle_familiarity.shape == (n, A) and res.best_idex.shape == (n,) and res.flags.shape == (n,)
    assert res.angle_familiarity.dtype == np.float64 and not res.flags.any()
    flat = eng.infomax_score_u8(e["planes"].reshape(n * A, e["h"], e["w"]))
    assert np.array_equal(H.bits(res.angle_familiarity).reshape(-1), H.bits(flat))
    err = np.max(np.abs(res.angle_familiarity - e["fam"])) / np.max(np.abs(e["fam"]))
    print("infomax ensemble %s %dx%d: relative error %.3e (bound %.1e)" % (key, n, A, err, H.TOL))
    assert err <= H.TOL
    assert res.best_idex.tolist() == np.argmax(e["fam"], axis=1).tolist()
    if e["planted"] is not None:
        i = e["planted"]
        assert res.best_idex[i] == 2                                                     # the first of two equal maxima
        assert H.bits(res.angle_familiarity[i, 2]) == H.bits(res.angle_familiarity[i, 7])
    again = eng.infomax_step_batch_u8(e["planes"])
    assert np.array_equal(H.bits(again.angle_familiarity), H.bits(res.angle_familiarity))
    assert again.best_idex.tolist() == res.best_idex.tolist()


def test_columns_past_one_staging_slab_keep_their_bits(eng):
    """2 members x 16163 headings at (20,13): 32326 columns of 2080 bytes are more than the 64 MiB the x vectors are staged in, so the
    call runs two slabs back to back (32256 columns, then 70); a column's value is score_u8's whichever slab it falls in."""
    d = H.case_data("20x13")
    n, A = 2, 16163
    assert n * A * d["N"] * 8 > 64 << 20
    planes = H.route_views(4242, n * A, d["h"], d["w"])
    eng.infomax_begin(d["h"], d["w"], d["W"], 2, H.ETA)
    res = eng.infomax_step_batch_u8(planes.reshape(n, A, d["h"], d["w"]))
    flat = eng.infomax_score_u8(planes)
    assert np.array_equal(H.bits(res.angle_familiarity).reshape(-1), H.bits(flat))
    assert res.best_idex.tolist() == np.argmax(flat.reshape(n, A), axis=1).tolist()


# ---- 2. sensed patches: the batch call against single steps ---------------------------------------------------------------------------
@pytest.mark.parametrize("A", [9, 13])
def test_sense_step_batch_is_five_single_steps(A):
    path = route()
    agent = make_agent(infomax_familiarity(seed=8), n_test_angles=A)
    try:
        agent.train_from_path(path)
        e = agent._engine
        rng = np.random.default_rng(A)
        xs = np.array([path[k][0] + rng.uniform(-1, 1) for k in (3, 11, 20, 29, 38)])
        ys = np.array([path[k][1] + rng.uniform(-1, 1) for k in (3, 11, 20, 29, 38)])
        angs = np.stack([(a + agent.angle_offsets) % (2 * np.pi) for a in (0.9, 0.2, 5.9, 1.4, 3.0)])
        single = [e.infomax_sense_step(xs[i], ys[i], angs[i]) for i in range(5)]
        res = e.infomax_sense_step_batch(xs, ys, angs)
        assert not res.flags.any()
        for i, (best, fam) in enumerate(single):
            assert np.array_equal(H.bits(res.angle_familiarity[i]), H.bits(fam)), i
            assert res.best_idex[i] == best == int(np.argmax(fam)), i
        # member 2 moves to where the bounds test passes (r = 6: x, y < 294) but a corner of the rotated footprint leaves the landscape
        xs2, ys2, angs2 = xs.copy(), ys.copy(), angs.copy()
        xs2[2] = ys2[2] = 293.4
        angs2[2] = (0.8 + np.pi / 2 + agent.angle_offsets) % (2 * np.pi)
        agent._check_bounds((xs2[2], ys2[2]))
        with pytest.raises(IndexError):
            e.infomax_sense_step(xs2[2], ys2[2], angs2[2])
        res2 = e.infomax_sense_step_batch(xs2, ys2, angs2)
        assert res2.flags.tolist() == [0, 0, 16, 0, 0] and res2.best_idex[2] == -1
        for i in (0, 1, 3, 4):
            assert np.array_equal(H.bits(res2.angle_familiarity[i]), H.bits(res.angle_familiarity[i])), i
            assert res2.best_idex[i] == res.best_idex[i], i
        # ... and the next call without it is as before
        res3 = e.infomax_sense_step_batch(xs, ys, angs)
        assert not res3.flags.any() and np.array_equal(H.bits(res3.angle_familiarity), H.bits(res.angle_familiarity))
    finally:
        agent.clear_training()


# ---- 3. InfomaxEnsemble against agents stepping alone -----------------------------------------------------------------------------------
def _poses(path):
    """Six start poses: four beside the route, one within r of the landscape's edge, one a few steps before the path's end."""
    out = []
    for k, (dx, dy, da) in zip((3, 10, 18, 26), ((0.7, -0.4, 0.1), (-0.5, 0.6, -0.2), (0.3, 0.9, 0.15), (-0.8, -0.3, -0.1))):
        d = path[k + 1] - path[k]
        out.append(((float(path[k][0] + dx), float(path[k][1] + dy)), float((np.arctan2(d[1], d[0]) + da) % (2 * np.pi))))
    out.append(((4.0, 150.0), 0.3))
    d = path[-1] - path[-2]
    out.append(((float(path[-5][0]), float(path[-5][1])), float(np.arctan2(d[1], d[0]) % (2 * np.pi))))
    return out


def _trained(path, seed=9):
    a = make_agent(infomax_familiarity(seed=seed))
    a.train_from_path(path)
    return a


def _same_row(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        assert x == y or (isinstance(x, float) and np.isnan(x) and np.isnan(y)), (k, x, y)


def test_infomax_ensemble_members_equal_lone_agents():
    path = route()
    poses = _poses(path)
    ens = navsim_amd.InfomaxEnsemble.from_agent(_trained(path), poses)
    calls = []
    inner = ens.engine.infomax_sense_step_batch

    def counted(*a, **k):
        calls.append(len(a[0]))
        return inner(*a, **k)
    ens.engine.infomax_sense_step_batch = counted
    alone = []
    for pos, ang in poses:
        a = _trained(path)
        a.position, a.angle = pos, ang
        alone.append(a)
    try:
        assert isinstance(ens, navsim_amd.NavEnsemble) and len(ens.agents) == 6
        assert all(a._metric_slot == j for j, a in enumerate(ens.agents))                # the metrics' batched device path
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
                assert np.array_equal(H.bits(m.scene_familiarity), H.bits(a.scene_familiarity)), (t, i)
            for i in before:
                if ens.stop_status[i] != -2:                                             # (every member that was scored in this step)
                    m = ens.agents[i]
                    assert m.scene_familiarity.shape == (len(path),) and np.all(m.scene_familiarity == m.angle_familiarity.min()), (t, i)
        # the member inside the bounds margin never sensed; the one near the path's end reached it
        assert ens.stop_status[4] == -2 and np.isnan(ens.agents[4].angle_familiarity).all() and np.isposinf(ens.agents[4].scene_familiarity).all()
        assert ens.stop_status[5] == 1 and isinstance(ens.agents[5].stopped_with_exception, navsim_amd.ReachedEndOfTrainingPathException)
        assert calls[0] == 5                                                             # member 4 was not sent to the device
        rows = ens.scene_familiarity()
        assert rows.shape == (6, len(path)) and np.isposinf(rows[4]).all()
        for i in (0, 1, 2, 3, 5):
            assert np.all(rows[i] == ens.agents[i].angle_familiarity.min()), i
    finally:
        ens.engine.infomax_sense_step_batch = inner
        ens.agents[0].clear_training()
        for a in alone:
            a.clear_training()


def test_run_ensemble_rows_equal_run_experiment_rows():
    path = route()
    poses = _poses(path)
    ens = navsim_amd.InfomaxEnsemble.from_agent(_trained(path), poses)
    try:
        rows = navsim_amd.run_ensemble(ens, frames=40)
    finally:
        ens.agents[0].clear_training()
    assert len(rows) == 6
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
        _same_row(rows[i], want)
    assert np.isnan(rows[4]["rmsd_error"]) and rows[4]["stop_status"] == -2 and rows[4]["completed_frames"] == 0
    assert rows[5]["stop_status"] == 1 and 0 < rows[5]["completed_frames"] < 10


# ---- 4. errors --------------------------------------------------------------------------------------------------------------------------
def test_batch_calls_before_begin_are_state_errors():
    e = navsim_amd.FamiliarityEngine(device=0)
    try:
        fam, best, flags = np.zeros(2), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.uint32)
        planes = np.zeros((1, 2, 3, 5), dtype=np.uint8)
        xy, ang = np.ones(1), np.zeros(2)
        bp, fp = best.ctypes.data_as(N._i32p), flags.ctypes.data_as(N._u32p)
        assert e._lib.dv_batch_infomax_step_u8(e._ctx, N.u8ptr(planes), 1, 2, N.f64ptr(fam), bp) == -3       # DV_ERR_STATE
        assert e._lib.dv_batch_infomax_sense_step(e._ctx, N.f64ptr(xy), N.f64ptr(xy), N.f64ptr(ang), 1, 2, N.f64ptr(fam), bp, fp) == -3
        with pytest.raises(navsim_amd.EngineError, match="DV_ERR_STATE"):
            e.infomax_step_batch_u8(planes)
        with pytest.raises(navsim_amd.EngineError, match="DV_ERR_STATE"):
            e.infomax_sense_step_batch(xy, xy, ang[None])
    finally:
        e.close()


def test_batch_calls_reject_bad_arguments_and_non_finite_weights(eng):
    d = H.case_data("16x16_a16")
    eng.infomax_begin(d["h"], d["w"], d["W"], 2, H.ETA)
    planes = np.ascontiguousarray(d["patches"][:6].reshape(2, 3, d["h"], d["w"]))
    fam, best, flags = np.zeros(6), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.uint32)
    xy, ang = np.ones(2), np.zeros(6)
    bp, fp = best.ctypes.data_as(N._i32p), flags.ctypes.data_as(N._u32p)
    lib, ctx = eng._lib, eng._ctx
    assert lib.dv_batch_infomax_step_u8(ctx, N.u8ptr(planes), 0, 3, N.f64ptr(fam), bp) == -1                   # DV_ERR_INVALID
    assert lib.dv_batch_infomax_step_u8(ctx, N.u8ptr(planes), 2, 0, N.f64ptr(fam), bp) == -1
    assert lib.dv_batch_infomax_step_u8(ctx, N.u8ptr(planes), 2, 3, None, bp) == -1
    assert lib.dv_batch_infomax_step_u8(ctx, N.u8ptr(planes), 2, 3, N.f64ptr(fam), None) == -1
    assert lib.dv_batch_infomax_step_u8(ctx, None, 2, 3, N.f64ptr(fam), bp) == -1
    assert lib.dv_batch_infomax_sense_step(ctx, N.f64ptr(xy), N.f64ptr(xy), N.f64ptr(ang), 0, 3, N.f64ptr(fam), bp, fp) == -1
    assert lib.dv_batch_infomax_sense_step(ctx, N.f64ptr(xy), N.f64ptr(xy), N.f64ptr(ang), 2, 3, None, bp, fp) == -1
    assert lib.dv_batch_infomax_sense_step(ctx, N.f64ptr(xy), N.f64ptr(xy), N.f64ptr(ang), 2, 3, N.f64ptr(fam), None, fp) == -1
    assert lib.dv_batch_infomax_sense_step(ctx, N.f64ptr(xy), N.f64ptr(xy), N.f64ptr(ang), 2, 3, N.f64ptr(fam), bp, None) == -1
    with pytest.raises(ValueError):
        eng.infomax_step_batch_u8(np.zeros((2, 3, 5, 3), dtype=np.uint8))                                      # patches of another shape
    assert np.isfinite(eng.infomax_step_batch_u8(planes).angle_familiarity).all()
    # a diverged training: the batch calls answer as the single ones do
    eng.infomax_begin(d["h"], d["w"], d["W0"], 2, H.diverging_eta())
    with pytest.raises(navsim_amd.EngineError, match="DV_ERR_STATE"):
        eng.infomax_train_u8(d["views"])
    with pytest.raises(navsim_amd.EngineError, match="not finite"):
        eng.infomax_step_batch_u8(planes)
    eng.infomax_set_weights(d["W"])
    assert np.isfinite(eng.infomax_step_batch_u8(planes).angle_familiarity).all()


def test_sense_step_batch_after_a_diverged_training_is_not_finite():
    d = H.case_data("16x16_a16")
    land = synth.synth_landscape(3, 300, 4)
    agent = navsim_amd.NavBySceneFamiliarity(land, (d["w"], d["h"]), 1.0, n_test_angles=3, familiarity_model=infomax_familiarity(seed=8))
    e = agent._engine                                                   # (landscape and sensor attached; the model is begun by hand)
    try:
        e.infomax_begin(d["h"], d["w"], d["W0"], 2, H.diverging_eta())
        with pytest.raises(navsim_amd.EngineError, match="learning_rate"):
            e.infomax_train_u8(d["views"])
        with pytest.raises(navsim_amd.EngineError, match="not finite"):
            e.infomax_sense_step_batch(np.full(2, 100.0), np.full(2, 100.0), np.zeros((2, 3)))
        e.infomax_set_weights(d["W"])
        res = e.infomax_sense_step_batch(np.full(2, 100.0), np.full(2, 100.0), np.zeros((2, 3)))
        assert np.isfinite(res.angle_familiarity).all() and not res.flags.any()
    finally:
        e.close()
