"""The sensor options under the learned models on the device: every sensed path of the Infomax and the mushroom-body model (training
from poses, the lone step, the ensemble's batched step, the per-member off-landscape flag, the agent and the two ensembles) against the
HOST sensor model's views and the NumPy statements on them (tests/helpers_sensed_models.py; its conditions and the Infomax tolerance
rule are held on the CPU by tests/test_sensed_models_host.py).

Reached here and nowhere else: channels 0 and 1 through the strided source of k_im_prep and k_mb and through k_mb_pose's own choice of
byte; the block branch of sense_pixel (hue argmax, saturation wrap, rounded mean V), the level table and the mask under k_mb_pose;
sensors that are not square, with pw != ph; N % 4 = 3 and a partial second trip of k_mb_pose's fill (odd: 323 pixels); a flag in a later
trip of k_mb_decide_batch (256 columns a trip) and of k_im_decide (64), in a member's last column, and from four different corners of
the footprint.

Mushroom comparisons are np.array_equal on the uint64 view; Infomax weights and scores are relative to max|W| and max|d| under
helpers_infomax.TOL, with the error printed."""
import numpy as np
import pytest

import navsim_amd
from navsim_amd import infomax_familiarity, mushroom_familiarity
from tests import helpers_infomax as HI
from tests import helpers_mushroom as H
from tests import helpers_sensed_models as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    """name -> the engine of an agent with use_gpu_sensor=True and the configuration's options (landscape and sensor attached; the
    models are begun by hand)."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = S.make_agent(name, mushroom_familiarity(n_kc=S.MB["n_kc"], fan_in=S.MB["fan_in"]), True)
            c = S.CONFIGS[name]
            assert made[name]._engine.sensor_shape == (c["sensor"][1], c["sensor"][0])
        return made[name]._engine
    yield get
    for agent in made.values():
        agent._engine.close()


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64, what
    bad = np.argwhere(H.bits(got) != H.bits(want))
    assert len(bad) == 0, (what, len(bad), bad[:6].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def within_tol(got, want, what):
    err = float(np.max(np.abs(np.asarray(got) - want)) / np.max(np.abs(want)))
    print("infomax %s: relative error %.3e (bound %.1e)" % (what, err, HI.TOL))
    assert err <= HI.TOL, what


# ---- 1. mushroom body, engine level ---------------------------------------------------------------------------------------------------
def begin_mb(e, d, trained=True):
    e.mb_begin(d["h"], d["w"], d["conn"], d["n_active"], d["channel"])
    if trained:
        e.mb_set_weights(d["wt"])


@pytest.mark.parametrize("name,channel", S.CASES)
def test_mb_train_from_poses_returns_the_host_views_and_the_statements_weights(engines, name, channel):
    d, e = S.data(name, channel), engines(name)
    begin_mb(e, d, trained=False)
    views = e.mb_train_from_poses(*S.route_poses())
    assert views.shape == d["scenes"].shape and views.dtype == np.uint8
    for ch in range(3):
        assert np.array_equal(views[..., ch], d["scenes"][..., ch]), ("channel", ch, int((views[..., ch] != d["scenes"][..., ch]).sum()))
    wt = e.mb_read_weights()
    assert np.array_equal(wt, d["wt"]), int((wt != d["wt"]).sum())
    assert e.mb_info()["views_trained"] == 45 and e.mb_info()["n_depressed"] == int((d["wt"] == 0).sum())


@pytest.mark.parametrize("name,channel", S.CASES)
def test_mb_sense_step_is_the_statement_on_the_host_planes(engines, name, channel):
    d, e = S.data(name, channel), engines(name)
    begin_mb(e, d)
    x, y, angs = S.lone_pose()
    best, fam = e.mb_sense_step(x, y, angs)
    same_bits(fam, d["mb_lone"], "lone step")
    assert best == int(np.argmax(d["mb_lone"]))


@pytest.mark.parametrize("name,channel", S.CASES)
def test_mb_sense_step_batch_is_the_statement_the_lone_steps_and_the_uploaded_planes(engines, name, channel):
    d, e = S.data(name, channel), engines(name)
    begin_mb(e, d)
    xs, ys, angs = S.member_poses()
    res = e.mb_sense_step_batch(xs, ys, angs)
    assert not res.flags.any()
    same_bits(res.angle_familiarity, d["mb_fam"], "batch")
    assert res.best_idex.tolist() == np.argmax(d["mb_fam"], axis=1).tolist()
    for i in range(S.N_MEMBERS):
        best, fam = e.mb_sense_step(xs[i], ys[i], angs[i])
        same_bits(fam, res.angle_familiarity[i], ("lone step of member", i))
        assert best == res.best_idex[i], i
    up = e.mb_step_batch_u8(d["members"])                                                # the host planes, uploaded
    same_bits(up.angle_familiarity, res.angle_familiarity, "uploaded planes")
    assert up.best_idex.tolist() == res.best_idex.tolist()


# ---- 2. Infomax, engine level ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,channel", S.CASES)
def test_infomax_train_from_poses_returns_the_host_views_and_the_restatements_weights(engines, name, channel):
    d, e = S.data(name, channel), engines(name)
    e.infomax_begin(d["h"], d["w"], d["W0"], channel, d["eta"])
    views = e.infomax_train_from_poses(*S.route_poses())
    for ch in range(3):
        assert np.array_equal(views[..., ch], d["scenes"][..., ch]), ("channel", ch, int((views[..., ch] != d["scenes"][..., ch]).sum()))
    W = e.infomax_read_weights()
    assert W.shape == d["W"].shape and e.infomax_info()["views_trained"] == 45
    within_tol(W, d["W"], "weights, sensed %s ch %d" % (name, channel))


@pytest.mark.parametrize("name,channel", S.CASES)
def test_infomax_sensed_steps_are_the_restatement_on_the_host_planes(engines, name, channel):
    d, e = S.data(name, channel), engines(name)
    e.infomax_begin(d["h"], d["w"], d["W"], channel, d["eta"])                           # the restatement's W: a score's error is not the chain's
    e.infomax_set_weights(d["W"])
    x, y, la = S.lone_pose()
    best, fam = e.infomax_sense_step(x, y, la)
    within_tol(fam, d["im_lone"], "lone step, %s ch %d" % (name, channel))
    assert best == int(np.argmax(d["im_lone"]))
    xs, ys, angs = S.member_poses()
    res = e.infomax_sense_step_batch(xs, ys, angs)
    assert not res.flags.any() and res.angle_familiarity.shape == (S.N_MEMBERS, S.N_HEADINGS)
    within_tol(res.angle_familiarity, d["im_fam"], "batch, %s ch %d" % (name, channel))
    assert res.best_idex.tolist() == np.argmax(d["im_fam"], axis=1).tolist()
    for i in range(S.N_MEMBERS):
        best, fam = e.infomax_sense_step(xs[i], ys[i], angs[i])
        same_bits(fam, res.angle_familiarity[i], ("lone step of member", i))
        assert best == res.best_idex[i], i


# ---- 3. the per-member off-landscape flag --------------------------------------------------------------------------------------------------
def begin_flag_model(e, name, model):
    """-> (batch call, lone call, compare(got, want, what)) with the group's channel-2 model on the engine."""
    d = S.data(name, 2)
    if model == "mb":
        begin_mb(e, d)
        return e.mb_sense_step_batch, e.mb_sense_step, same_bits
    e.infomax_begin(d["h"], d["w"], d["W"], 2, d["eta"])
    return e.infomax_sense_step_batch, e.infomax_sense_step, within_tol


def run_flag_layout(e, name, model, lay, alone):
    """The clean call, the flagged call and the clean call again; `alone`: the unflagged members whose row must be a lone step's and a
    call's without the other members."""
    batch, lone, compare = begin_flag_model(e, name, model)
    xs, ys = lay["xs"], lay["ys"]
    n, A = lay["angs"].shape
    tag = "%s %s %dx%d" % (name, model, n, A)
    first = batch(xs, ys, lay["clean"])
    assert not first.flags.any(), first.flags
    compare(first.angle_familiarity, lay[model + "_clean"], tag + " clean")
    assert first.best_idex.tolist() == lay[model + "_best_clean"].tolist()
    res = batch(xs, ys, lay["angs"])
    assert res.flags.tolist() == lay["flags"].tolist(), res.flags
    assert res.best_idex.tolist() == lay[model + "_best"].tolist(), res.best_idex
    keep = lay["keep"]
    compare(np.where(keep, res.angle_familiarity, 0.0), np.where(keep, lay[model + "_fam"], 0.0), tag + " flagged, the columns on the landscape")
    same_bits(np.where(keep, res.angle_familiarity, 0.0), np.where(keep, first.angle_familiarity, 0.0), tag + " flagged against clean")
    for i in range(n):
        if lay["flags"][i]:
            with pytest.raises(IndexError):
                lone(xs[i], ys[i], lay["angs"][i])
    for i in alone:
        best, fam = lone(xs[i], ys[i], lay["angs"][i])
        same_bits(res.angle_familiarity[i], fam, (tag, "lone step of member", i))
        assert res.best_idex[i] == best
        only = batch(xs[i:i + 1], ys[i:i + 1], lay["angs"][i:i + 1])
        same_bits(only.angle_familiarity[0], res.angle_familiarity[i], (tag, "member alone in a call", i))
        assert only.flags.tolist() == [0] and only.best_idex[0] == best
    after = batch(xs, ys, lay["clean"])
    assert not after.flags.any(), after.flags
    same_bits(after.angle_familiarity, first.angle_familiarity, tag + " clean again")
    assert after.best_idex.tolist() == first.best_idex.tolist()


@pytest.mark.parametrize("model", ["mb", "im"])
@pytest.mark.parametrize("name", S.FLAG_GROUPS)
def test_flag_from_each_corner_of_the_footprint(engines, name, model):
    """Four members at one place, each with ONE heading on another diagonal, so that another corner of the footprint is off the
    landscape: every one is flagged -- a workgroup-wide OR, not one thread's pixel -- and the fifth, on the route, is not."""
    S.flag_facts(name)
    lay = S.flag_layouts(name, model)["corners"]
    assert lay["flags"].tolist() == [16, 16, 16, 16, 0] and lay[model + "_best"][:4].tolist() == [-1] * 4
    run_flag_layout(engines(name), name, model, lay, alone=[4])


@pytest.mark.parametrize("model", ["mb", "im"])
@pytest.mark.parametrize("name", S.FLAG_GROUPS)
def test_flag_in_a_later_trip_and_in_a_members_last_column(engines, name, model):
    """Three members x 260 headings (mushroom) or 70 (Infomax): member 0 is off at its last heading only, member 2 at heading 257 (65)
    only -- columns of the decide kernel's second trip -- and member 1, between them, nowhere."""
    S.flag_facts(name)
    lay = S.flag_layouts(name, model)["trips"]
    assert lay["flags"].tolist() == [16, 0, 16] and lay[model + "_best"][1] == int(np.argmax(lay[model + "_fam"][1])) > 0
    run_flag_layout(engines(name), name, model, lay, alone=[1])


# ---- 4. agent level: px, channel 1 ----------------------------------------------------------------------------------------------------------
def _clear(agents):
    for a in agents:
        if getattr(a._familiarity_func, "engine", None) is not None:
            a.clear_training()


def test_mushroom_agent_device_host_sensor_and_numpy_plug_in_on_channel_1():
    path = S.route()
    cfg = S.AGENT
    model = mushroom_familiarity(channel=cfg["channel"], **cfg["mb"])
    agents = [S.make_agent(cfg["name"], model, True), S.make_agent(cfg["name"], model, False),
              S.make_agent(cfg["name"], H.numpy_model(channel=cfg["channel"], **cfg["mb"]), False)]
    try:
        for a in agents:
            a.train_from_path(path)
            a.position, a.angle = tuple(path[3] + np.array([0.7, -0.4])), 0.9
        assert agents[0]._familiarity_func.engine is agents[0]._engine and agents[0]._familiarity_func.channel == 1
        assert agents[1]._familiarity_func.metric == "mushroom" and agents[1]._engine is None
        assert not hasattr(agents[2]._familiarity_func, "engine")
        assert agents[0].familiar_scenes.tobytes() == agents[2].familiar_scenes.tobytes() == S.scenes(cfg["name"])["route"].tobytes()
        wt = agents[2]._familiarity_func.wt
        other = H.numpy_model(channel=2, **cfg["mb"])(agents[2].familiar_scenes).wt
        assert not np.array_equal(wt, other)                                             # (channel 2 is another model)
        assert np.array_equal(agents[0]._engine.mb_read_weights(), wt)
        assert np.array_equal(agents[1]._familiarity_func.engine.mb_read_weights(), wt)
        seen = set()
        for step in range(20):
            for a in agents:
                a.step_forward(fake=True)
            a0 = agents[0]
            for a in agents[1:]:
                assert a.position == a0.position and a.angle == a0.angle, step
                assert np.array_equal(H.bits(a.angle_familiarity), H.bits(a0.angle_familiarity)), step
                assert np.array_equal(H.bits(a.scene_familiarity), H.bits(a0.scene_familiarity)), step
            assert a0.last_best_idex == int(np.argmax(a0.angle_familiarity))
            seen.update(a0.angle_familiarity.tolist())
        assert len(seen) > 3
    finally:
        _clear(agents[:2])


def _ensemble_against_lone_agents(make_ens, model, steps=15):
    path = S.route()
    cfg = S.AGENT
    poses = S.start_poses(path)

    def trained(gpu_sensor=True):
        a = S.make_agent(cfg["name"], model, gpu_sensor)
        a.train_from_path(path)
        return a
    ens = make_ens(trained(), poses)
    alone = []
    try:
        for pos, ang in poses:
            a = trained()
            a.position, a.angle = pos, ang
            alone.append(a)
        host = trained(False)                                                            # member 0 once more, through the host sensor model
        host.position, host.angle = poses[0]
        alone.append(host)
        assert ens.agents[0]._familiarity_func.channel == 1 and ens.agents[0].familiar_scenes.tobytes() == host.familiar_scenes.tobytes()
        seen = set()
        for t in range(steps):
            ens.step_forward(fake=False)
            for a in alone:
                a.step_forward(fake=False)
            for i, (m, a) in enumerate(zip(list(ens.agents) + [ens.agents[0]], alone)):
                assert m.position == a.position and m.angle == a.angle, (t, i)
                assert np.array_equal(H.bits(m.angle_familiarity), H.bits(a.angle_familiarity)), (t, i)
                assert np.array_equal(H.bits(m.scene_familiarity), H.bits(a.scene_familiarity)), (t, i)
                seen.update(m.angle_familiarity.tolist())
        assert not any(ens.stop_status) and len(ens.active) == len(poses) and len(seen) > 3
    finally:
        ens.agents[0].clear_training()
        _clear(alone)


def test_mushroom_ensemble_on_channel_1_equals_lone_agents():
    model = mushroom_familiarity(channel=S.AGENT["channel"], **S.AGENT["mb"])
    _ensemble_against_lone_agents(navsim_amd.MushroomEnsemble.from_agent, model)


def test_infomax_ensemble_on_channel_1_equals_lone_agents():
    model = infomax_familiarity(channel=S.AGENT["channel"], **S.AGENT["im"])
    _ensemble_against_lone_agents(navsim_amd.InfomaxEnsemble.from_agent, model)
