"""Infomax familiarity model on the device against its NumPy restatement (tests/helpers_infomax.py), within the tolerance that
restatement gives against itself (H.TOL); device against device, bit for bit.

Shapes (H.CASES): (5,3) with one and two views -- the first-h launch and the fused hand-over of the next h; (40,1) with 24 rows, the
shape of the reference's scripts/test.py; (16,16) with 130 views and 16 / 65 patches -- the steady state and the 64-heading chunk;
(20,13) with 70 rows -- ragged in every tile; (7,5) with 1043 rows, (33,31) with 20 and (32,32) with 1040 -- the smallest at which
the strided loops of the kernels take a further trip (66 and 65 row tiles for 64 lanes, 17 row blocks, 4 column blocks of 256, 64
chunks of scalar loads); 8197 views of (32,32) -- the chain that crosses the staging slab of the training."""
import ctypes

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import infomax_familiarity, synth
from tests import helpers_infomax as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = navsim_amd.FamiliarityEngine(device=0)
    yield e
    e.close()


def begin(e, d, weights=None, eta=H.ETA):
    e.infomax_begin(d["h"], d["w"], d["W0"] if weights is None else weights, 2, eta)


@pytest.mark.parametrize("key", ["5x3_f1", "5x3_f2", "40x1", "16x16_a16", "20x13", "7x5_m1043", "33x31", "32x32_m1040"])
def test_weights_after_training(eng, key):
    d = H.case_data(key)
    begin(eng, d)
    eng.infomax_train_u8(d["views"])
    W = eng.infomax_read_weights()
    info = eng.infomax_info()
    assert info == dict(n_hidden=d["M"], n_pixels=d["N"], views_trained=d["F"], finite=True, bytes=8 * d["M"] * d["N"])
    err = np.max(np.abs(W - d["W"])) / np.max(np.abs(d["W"]))
    print("infomax weights %s: relative error %.3e (bound %.1e)" % (key, err, H.TOL))
    assert err <= H.TOL
    # the same calls again: the same bits
    begin(eng, d)
    eng.infomax_train_u8(d["views"])
    assert np.array_equal(H.bits(eng.infomax_read_weights()), H.bits(W))


@pytest.mark.parametrize("key", list(H.CASES))
def test_scores_on_the_restatements_weights(eng, key):
    d = H.case_data(key)
    begin(eng, d, weights=d["W"])
    fam = eng.infomax_score_u8(d["patches"])
    assert fam.shape == (d["A"],) and np.all(fam < 0)
    err = np.max(np.abs(fam - d["fam"])) / np.max(np.abs(d["fam"]))
    print("infomax scores %s: relative error %.3e (bound %.1e)" % (key, err, H.TOL))
    assert err <= H.TOL
    if d["A"] > 1:
        assert H.best_margin(d["fam"]) > H.TOL                     # (chosen so on the CPU: tests/test_infomax_host.py)
        assert int(np.argmax(fam)) == int(np.argmax(d["fam"]))
    # a patch scores the same alone as among the others (any heading count takes the same sums)
    alone = np.array([eng.infomax_score_u8(p)[0] for p in d["patches"][:3]])
    assert np.array_equal(H.bits(alone), H.bits(fam[:3]))


@pytest.mark.parametrize("key", H.MEAN_KEYS)
def test_weights_whose_rows_do_not_sum_to_zero_see_the_views_mean(eng, key):
    """From W0 + 1/N: under every other W of these tests the rows sum to zero and W x does not depend on the mean k_im_prep takes off
    a view (tests/helpers_infomax.py: MEAN_KEYS); here a mean that misses one pixel moves the scores by 6e-6 and more."""
    d = H.offset_case_data(key)
    begin(eng, d)
    eng.infomax_train_u8(d["views"])
    W = eng.infomax_read_weights()
    err = np.max(np.abs(W - d["W"])) / np.max(np.abs(d["W"]))
    print("infomax weights %s from W0 + 1/N: relative error %.3e (bound %.1e)" % (key, err, H.TOL))
    assert err <= H.TOL
    eng.infomax_set_weights(d["W"])
    fam = eng.infomax_score_u8(d["patches"])
    err = np.max(np.abs(fam - d["fam"])) / np.max(np.abs(d["fam"]))
    print("infomax scores %s from W0 + 1/N: relative error %.3e (bound %.1e)" % (key, err, H.TOL))
    assert err <= H.TOL
    assert H.best_margin(d["fam"]) > H.TOL and int(np.argmax(fam)) == int(np.argmax(d["fam"]))


@pytest.mark.parametrize("key,cut", [("5x3_f2", 1), ("16x16_a16", 50), ("20x13", 32), ("7x5_m1043", 2), ("32x32_m1040", 5)])
def test_continued_training_is_the_uncut_chain(eng, key, cut):
    d = H.case_data(key)
    begin(eng, d)
    eng.infomax_train_u8(d["views"])
    whole = eng.infomax_read_weights()
    begin(eng, d)
    eng.infomax_train_u8(d["views"][:cut])
    eng.infomax_train_u8(d["views"][cut:])
    assert eng.infomax_info()["views_trained"] == d["F"]
    assert np.array_equal(H.bits(eng.infomax_read_weights()), H.bits(whole))


def test_chain_across_the_staging_slab_is_the_uncut_chain(eng):
    """8197 views of 32x32: the x vectors are staged 8192 at a time, so the training ends one slab without a next view and starts the
    next with a first h of its own.  Cut anywhere -- inside the first slab, or exactly where the slabs meet -- it carries the same
    bits, and they are the restatement's weights within the bound that chain's own rounding gives (H.TOL_LONG_CHAIN)."""
    d = H.long_chain_data()
    assert d["F"] == 8192 + 5 and (64 << 20) // (8 * d["N"]) == 8192
    got = []
    for cut in (None, 100, 8192):
        begin(eng, d)
        if cut is None:
            eng.infomax_train_u8(d["views"])
        else:
            eng.infomax_train_u8(d["views"][:cut])
            eng.infomax_train_u8(d["views"][cut:])
        assert eng.infomax_info()["views_trained"] == 8197, cut
        got.append(eng.infomax_read_weights())
    assert np.array_equal(H.bits(got[1]), H.bits(got[0]))
    assert np.array_equal(H.bits(got[2]), H.bits(got[0]))
    err = np.max(np.abs(got[0] - d["W"])) / np.max(np.abs(d["W"]))
    print("infomax weights, 8197-view chain: relative error %.3e (bound %.1e)" % (err, H.TOL_LONG_CHAIN))
    assert err <= H.TOL_LONG_CHAIN


def test_set_weights_round_trip_and_a_second_engine(eng):
    d = H.case_data("20x13")
    begin(eng, d)
    eng.infomax_train_u8(d["views"])
    W = eng.infomax_read_weights()
    fam = eng.infomax_score_u8(d["patches"])
    eng.infomax_set_weights(W)
    assert np.array_equal(H.bits(eng.infomax_read_weights()), H.bits(W))
    other = navsim_amd.FamiliarityEngine(device=0)
    try:
        other.infomax_begin(d["h"], d["w"], np.zeros_like(W), 2, H.ETA)
        other.infomax_set_weights(W)
        assert np.array_equal(H.bits(other.infomax_score_u8(d["patches"])), H.bits(fam))
    finally:
        other.close()


# ---- behind the agent -------------------------------------------------------------------------------------------------------
SENSOR = (12, 10)                                                     # (w, h): N = 120


def make_agent(model, gpu_sensor, n_test_angles=9):
    land = synth.synth_landscape(3, 300, 4)
    return navsim_amd.NavBySceneFamiliarity(land, SENSOR, 1.0, n_test_angles=n_test_angles, use_gpu_sensor=gpu_sensor,
                                            familiarity_model=model)


def route():
    return synth.sin_training_path(0.5, 60, 180, arclen=1.0)[:45]


def hide_engine(model):
    """The same model as a plug-in that shows the agent nothing but func(scene, fambuf): the reference's generic loop."""
    def plain(scenes):
        func = model(scenes)

        def only_func(scene, fambuf):
            func(scene, fambuf)
        only_func.max_familiarity = func.max_familiarity
        only_func.inner = func
        return only_func
    return plain


def test_training_from_poses_is_training_on_the_uploaded_views():
    path = route()
    dev = make_agent(infomax_familiarity(seed=5), True)
    host = make_agent(infomax_familiarity(seed=5), False)
    try:
        dev.train_from_path(path)
        host.train_from_path(path)
        assert dev.familiar_scenes.tobytes() == host.familiar_scenes.tobytes()       # out_views: the host sensor model's views
        W_dev = dev._engine.infomax_read_weights()
        W_host = host._familiarity_func.engine.infomax_read_weights()
        assert W_dev.shape == (120, 120) and np.array_equal(H.bits(W_dev), H.bits(W_host))
        assert dev._engine.infomax_info()["views_trained"] == len(path)
        # a further path continues the chain on both
        more = route()[::-1][:20] + np.array([1.5, -2.0])
        dev.train_additional_path(more)
        host.train_additional_path(more)
        assert dev.familiar_scenes.tobytes() == host.familiar_scenes.tobytes() and len(dev.familiar_scenes) == 65
        assert np.array_equal(H.bits(dev._engine.infomax_read_weights()), H.bits(host._familiarity_func.engine.infomax_read_weights()))
    finally:
        dev.clear_training()
        host.clear_training()


def test_agent_fused_step_is_the_generic_plug_in_path():
    path = route()
    model = infomax_familiarity(seed=6)
    agents = [make_agent(model, True), make_agent(model, False), make_agent(hide_engine(model), False)]
    try:
        for a in agents:
            a.train_from_path(path)
            a.position, a.angle = tuple(path[3] + np.array([0.7, -0.4])), 0.9
        assert agents[0]._familiarity_func.engine is agents[0]._engine              # the fused device step
        assert not hasattr(agents[2]._familiarity_func, "engine")                   # the reference's loop over func
        for step in range(40):
            for a in agents:
                a.step_forward(fake=True)
            a0 = agents[0]
            for a in agents[1:]:
                assert a.position == a0.position and a.angle == a0.angle, step
                assert np.array_equal(H.bits(a.angle_familiarity), H.bits(a0.angle_familiarity)), step
                assert np.array_equal(H.bits(a.scene_familiarity), H.bits(a0.scene_familiarity)), step
            assert a0.last_best_idex == int(np.argmax(a0.angle_familiarity))
            assert np.all(a0.angle_familiarity < 0) and a0.step_familiarity == a0.angle_familiarity.max()
            # no per-view memory: scene_familiarity is the least familiarity over the headings, at every view
            assert a0.scene_familiarity.shape == (len(path),)
            assert np.all(a0.scene_familiarity == a0.angle_familiarity.min())
    finally:
        agents[2]._familiarity_func.inner.engine.close()
        for a in agents[:2]:
            a.clear_training()


# ---- behind the agent, at a shape past one trip of the loops: 32x32 views, 1040 rows (65 row tiles) ----------------------------------
def sensed_agent(seed=H.SENSED["seed"]):
    a = H.sensed_agent(infomax_familiarity(learning_rate=H.SENSED["eta"], seed=seed, n_hidden=H.SENSED["M"]), True)
    a.train_from_path(H.sensed_route())
    return a


def test_sensed_training_at_1040_rows_gives_the_restatements_weights():
    s = H.sensed_data()
    agent = sensed_agent()
    try:
        assert agent.familiar_scenes.tobytes() == s["scenes"].tobytes()              # the host sensor model's views
        W = agent._engine.infomax_read_weights()
        assert agent._engine.infomax_info()["views_trained"] == s["n_poses"]
    finally:
        agent.clear_training()
    # s["W"]: H.train(H.initial_weights(1040, 1024, seed), familiar_scenes[..., 2], eta=0.001), computed once for both test modules
    want = s["W"]
    assert W.shape == want.shape == (1040, 1024)
    err = np.max(np.abs(W - want)) / np.max(np.abs(want))
    print("infomax weights, sensed 32x32 x 1040: relative error %.3e (bound %.1e)" % (err, H.TOL))
    assert err <= H.TOL                                    # (this chain passes the 1000 x rule under TOL: tests/test_infomax_host.py)


def test_sense_step_batch_at_1040_rows_is_five_single_steps():
    path = H.sensed_route()
    agent = sensed_agent()
    try:
        e = agent._engine
        rng = np.random.default_rng(9)
        xs = np.array([path[k][0] + rng.uniform(-1, 1) for k in (3, 11, 20, 29, 38)])
        ys = np.array([path[k][1] + rng.uniform(-1, 1) for k in (3, 11, 20, 29, 38)])
        angs = np.stack([(a + agent.angle_offsets) % (2 * np.pi) for a in (0.9, 0.2, 5.9, 1.4, 3.0)])
        assert angs.shape == (5, 9)
        single = [e.infomax_sense_step(xs[i], ys[i], angs[i]) for i in range(5)]
        res = e.infomax_sense_step_batch(xs, ys, angs)
        assert not res.flags.any()
        for i, (best, fam) in enumerate(single):
            assert np.all(fam < 0) and len(np.unique(fam)) > 1, i
            assert np.array_equal(H.bits(res.angle_familiarity[i]), H.bits(fam)), i
            assert res.best_idex[i] == best == int(np.argmax(fam)), i
    finally:
        agent.clear_training()


def test_infomax_ensemble_at_1040_rows_equals_lone_agents():
    path = H.sensed_route()
    poses = []
    for k, (dx, dy, da) in zip((3, 14, 27), ((0.7, -0.4, 0.1), (-0.5, 0.6, -0.2), (0.3, 0.9, 0.15))):
        step = path[k + 1] - path[k]
        poses.append(((float(path[k][0] + dx), float(path[k][1] + dy)), float((np.arctan2(step[1], step[0]) + da) % (2 * np.pi))))
    ens = navsim_amd.InfomaxEnsemble.from_agent(sensed_agent(), poses)
    alone = []
    try:
        for pos, ang in poses:
            a = sensed_agent()
            a.position, a.angle = pos, ang
            alone.append(a)
        for t in range(5):
            ens.step_forward(fake=False)
            for a in alone:
                a.step_forward(fake=False)
            for i, (m, a) in enumerate(zip(ens.agents, alone)):
                assert m.position == a.position and m.angle == a.angle, (t, i)
                assert np.array_equal(H.bits(m.angle_familiarity), H.bits(a.angle_familiarity)), (t, i)
        assert not any(ens.stop_status) and len(ens.active) == 3
    finally:
        ens.agents[0].clear_training()
        for a in alone:
            a.clear_training()


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_scoring_before_begin_is_a_state_error():
    e = navsim_amd.FamiliarityEngine(device=0)
    try:
        out = np.zeros(1)
        planes = np.zeros((1, 3, 5), dtype=np.uint8)
        assert e._lib.dv_infomax_score_u8(e._ctx, N.u8ptr(planes), 1, N.f64ptr(out)) == -3          # DV_ERR_STATE
        with pytest.raises(navsim_amd.EngineError, match="DV_ERR_STATE"):
            e.infomax_score_u8(planes)
        with pytest.raises(navsim_amd.EngineError, match="DV_ERR_STATE"):
            e.infomax_train_u8(planes)
        with pytest.raises(navsim_amd.EngineError, match="DV_ERR_STATE"):
            e.infomax_read_weights()
        best = ctypes.c_int32(0)
        ang = np.zeros(2)
        assert e._lib.dv_infomax_sense_step(e._ctx, 1.0, 1.0, N.f64ptr(ang), 2, N.f64ptr(out), ctypes.byref(best)) == -3
        assert e.infomax_info()["finite"] is False and e.infomax_info()["n_hidden"] == 0
    finally:
        e.close()


def test_begin_rejects_bad_arguments(eng):
    W0 = H.initial_weights(15, 15, 1)
    for kw in (dict(channel=3), dict(channel=-1), dict(learning_rate=0.0), dict(learning_rate=-1.0)):
        with pytest.raises(ValueError, match="DV_ERR_INVALID"):
            eng.infomax_begin(3, 5, W0, **kw)
    z = ctypes.c_double(0)
    assert eng._lib.dv_infomax_begin(eng._ctx, 3, 5, 2, 0, 0.01, ctypes.byref(z)) == -1              # n_hidden < 1
    with pytest.raises(ValueError):
        eng.infomax_begin(3, 4, W0)                                                               # 15 columns for 12 pixels
    eng.infomax_begin(3, 5, W0)
    with pytest.raises(ValueError):
        eng.infomax_score_u8(np.zeros((2, 5, 3), dtype=np.uint8))                                 # patches of another shape


def test_diverging_learning_rate_is_an_error_and_no_nans_come_back(eng):
    d = H.case_data("16x16_a16")
    begin(eng, d, eta=H.diverging_eta())                                 # a rate the CPU restatement overflows at
    with pytest.raises(navsim_amd.EngineError, match=r"DV_ERR_STATE") as ei:
        eng.infomax_train_u8(d["views"])
    assert "learning_rate 1" in str(ei.value)
    assert eng.infomax_info()["finite"] is False
    with pytest.raises(navsim_amd.EngineError, match="not finite"):
        eng.infomax_score_u8(d["patches"])
    # the model through the factory: the same error from training
    with pytest.raises(navsim_amd.EngineError, match="learning_rate"):
        infomax_familiarity(learning_rate=H.diverging_eta(), seed=14)(d["views"])
    # finite weights bring the model back
    eng.infomax_set_weights(d["W"])
    assert np.isfinite(eng.infomax_score_u8(d["patches"])).all()


def test_an_ensemble_of_infomax_agents_is_refused():
    agent = make_agent(infomax_familiarity(seed=7), True)
    try:
        agent.train_from_path(route())
        with pytest.raises(ValueError, match="NavEnsemble does not take an Infomax model"):
            navsim_amd.NavEnsemble.from_agent(agent, [((100.0, 100.0), 0.3), ((110.0, 100.0), 0.4)])
    finally:
        agent.clear_training()
