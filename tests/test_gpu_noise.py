"""Sensor noise on the device (dv_noise_*): a reproducible integer draw per sensing in every sensed call that takes a landscape table.
Expected bytes never come from the device (tests/helpers_noise.py): agent.fill_sensor_from and agent.downscale_chem on the pose's own
landscape, the draws of synth.splitmix64, the agent's level tables, the NumPy statement of the mushroom body.  The scored calls are
compared with their uploaded-patch twins (*_u8) on the statement's patches.  Every comparison is np.array_equal (doubles: on their
uint64 views).  At helpers_inet.SLAB's size the sensor has 256 levels and no mask, and the noiseless lands_sense views are S and V."""
import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import infomax_familiarity, mushroom_familiarity, sads_familiarity, ssd_familiarity
from tests import helpers_mushroom as H
from tests import helpers_noise as HZ

pytestmark = pytest.mark.gpu

STATE, INVALID = -3, -1


def engine(cfg, table=None):
    """An engine under `cfg` with landscape 0 as its one landscape, helpers_noise.lands() as its set and `table` as its sensor table."""
    e = navsim_amd.FamiliarityEngine(device=0)
    e.set_landscape(HZ.lands()[0])
    e.configure_sensor(cfg["sensor"], cfg["pixel"], HZ.level_table(cfg), cfg["mask"])
    e.lands_set(list(HZ.lands()))
    if table is not None:
        e.sensors_set(*HZ.table_args(table))
    return e


def same_bits(a, b, what=None):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    bad = np.argwhere(H.bits(a) != H.bits(b))
    assert len(bad) == 0, (what, len(bad), bad[:6].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


def same_results(got, want, what, fields=("angle_familiarity", "best_idex")):
    for f in fields:
        same_bits(getattr(got, f), getattr(want, f), (what, f))


# ---- 1, 2. lands_sense under rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("thin", "wide"))
def test_lands_sense_under_rows_is_the_statement_byte_for_byte(name):
    s = HZ.sense_case(name)
    e = engine(HZ.THIN) if name == "thin" else engine(HZ.WIDE, table=s["cfgs"])
    try:
        plain = e.lands_sense(s["x"], s["y"], s["angle"], s["land_of"])
        assert np.array_equal(plain, s["plain"])
        assert e.noise_info()["n_rows"] == 0 and e.n_noise_rows == 0
        e.noise_rows(HZ.SEED, s["keys"], s["amp_s"], s["amp_v"])
        info = e.noise_info()
        assert info["n_rows"] == 11 == e.n_noise_rows and info["seed"] == HZ.SEED and np.array_equal(info["keys"], s["keys"])
        assert info["amp_s"].tolist() == s["amp_s"].tolist() and info["amp_v"].tolist() == s["amp_v"].tolist()
        got = e.lands_sense(s["x"], s["y"], s["angle"], s["land_of"])
        assert got.dtype == np.uint8 and np.array_equal(got, s["noisy"])
        zero = [v for v in range(11) if s["amp_s"][v] == 0 and s["amp_v"][v] == 0]
        assert zero and np.array_equal(got[zero], plain[zero])
        if name == "wide":
            for v in range(11):
                cfg = s["cfgs"][s["land_of"][v]]
                assert set(np.unique(got[v][..., 2]).tolist()) <= set(np.unique(HZ.level_table(cfg)[2]).tolist())
                if cfg["mask"]:
                    assert not got[v][:, 8 - cfg["mask"]:8 + cfg["mask"]].any()
        # the same rows again: the same bytes (nothing of a call's state enters a draw); another seed: other bytes
        assert np.array_equal(e.lands_sense(s["x"], s["y"], s["angle"], s["land_of"]), got)
        e.noise_rows(HZ.SEED + 1, s["keys"], s["amp_s"], s["amp_v"])
        other = e.lands_sense(s["x"], s["y"], s["angle"], s["land_of"])
        assert np.array_equal(other[zero], plain[zero]) and not np.array_equal(other, got)
        # a row's bytes do not depend on its place in the call, nor on who else is there
        pick = [7, 2, 9]
        e.noise_rows(HZ.SEED, s["keys"][pick], s["amp_s"][pick], s["amp_v"][pick])
        assert np.array_equal(e.lands_sense(s["x"][pick], s["y"][pick], s["angle"][pick], s["land_of"][pick]), s["noisy"][pick])
        # the sensor table may go and come under live rows; the set may be set again
        if name == "wide":
            e.sensors_clear()
            assert e.noise_info()["n_rows"] == 3
            e.lands_set(list(HZ.lands()))
            e.sensors_set(*HZ.table_args(s["cfgs"]))
            assert e.noise_info()["n_rows"] == 3
            assert np.array_equal(e.lands_sense(s["x"][pick], s["y"][pick], s["angle"][pick], s["land_of"][pick]), s["noisy"][pick])
    finally:
        e.close()


# ---- 3, 4. the mushroom body ---------------------------------------------------------------------------------------------------------------------
def mb_engine(shape, table):
    own, tab = HZ.MB_SHAPES[shape][:2]
    e = engine(own, table=tab if table else None)
    w, h = own["sensor"]
    e.mb_begin(h, w, HZ.mb_conn(shape), HZ.MB["n_active"], HZ.MB["channel"])
    e.mbank_set(HZ.N_BANKS)
    return e


@pytest.mark.parametrize("shape,table", [("thin", False), ("thin", True), ("big", False), ("big", True)])
def test_mushroom_training_and_banked_step_under_rows_equal_the_statement(shape, table):
    t, c = HZ.mb_train_case(shape, table), HZ.mb_step_case(shape, table)
    e = mb_engine(shape, table)
    try:
        e.noise_rows(HZ.SEED, t["keys"], t["amp_s"], t["amp_v"])
        got = e.mbank_train_from_poses(t["x"], t["y"], t["angle"], t["bank_of"], land_of_view=t["land_of"])
        assert np.array_equal(got, t["views"])
        for b in range(HZ.N_BANKS):
            assert np.array_equal(e.mbank_read_weights(b), t["wts"][b]), b
        e.noise_rows(HZ.SEED, c["keys"], c["amp_s"], c["amp_v"])
        res = e.mbank_sense_step_batch(c["xs"], c["ys"], c["angs"], c["banks"], land_of_member=c["lands"])
        assert not res.flags.any()
        same_bits(res.angle_familiarity, c["fam"], (shape, table))
        assert res.best_idex.tolist() == c["best"].tolist()
        twin = e.mbank_step_batch_u8(np.ascontiguousarray(c["planes"][..., HZ.MB["channel"]]), c["banks"])
        same_results(res, twin, (shape, table, "the uploaded twin"))
        e.noise_clear()
        quiet = e.mbank_sense_step_batch(c["xs"], c["ys"], c["angs"], c["banks"], land_of_member=c["lands"])
        same_bits(quiet.angle_familiarity, c["plain_fam"], (shape, table, "after noise_clear"))
    finally:
        e.close()


# ---- 5. Infomax ------------------------------------------------------------------------------------------------------------------------------------
def im_begin(e, cfg, n_banks, M=None):
    w, h = cfg["sensor"]
    Ws = HZ.im_weights(n_banks, w * h, M)
    e.infomax_begin(h, w, Ws[0], channel=HZ.IM["channel"], learning_rate=0.01)
    e.ibank_set(n_banks, Ws[0])
    for b in range(n_banks):
        e.ibank_set_weights(b, Ws[b])


def test_infomax_banked_step_under_rows_equals_the_uploaded_step_on_the_statements_patches():
    c = HZ.im_step_case()
    e = engine(HZ.THIN)
    try:
        im_begin(e, HZ.THIN, 3)
        want = e.ibank_step_batch_u8(np.ascontiguousarray(c["planes"][..., HZ.IM["channel"]]), c["banks"])
        e.noise_rows(HZ.SEED, c["keys"], c["amp_s"], c["amp_v"])
        got = e.ibank_sense_step_batch(c["xs"], c["ys"], c["angs"], c["banks"], land_of_member=c["lands"])
        assert not got.flags.any()
        same_results(got, want, "5 x 3 at 7 x 5")
        e.noise_clear()
        quiet = e.ibank_sense_step_batch(c["xs"], c["ys"], c["angs"], c["banks"], land_of_member=c["lands"])
        assert not np.array_equal(quiet.angle_familiarity, got.angle_familiarity)
    finally:
        e.close()


def test_infomax_step_past_the_slab_draws_by_the_calls_columns():
    """helpers_inet.SLAB's layout: the second launch begins at column 8176, heading 4 of a member at place 681 of the bank order.  A row
    or heading index counted from the launch's first column would give other bytes there."""
    c = HZ.slab_case()
    lay = c["lay"]
    n, A = len(c["banks"]), lay["A"]
    e = engine(HZ.PLAIN32)
    try:
        im_begin(e, HZ.PLAIN32, 4, M=5)
        plain = e.lands_sense(np.repeat(c["xs"], A), np.repeat(c["ys"], A), c["angs"].reshape(-1), np.repeat(c["lands"], A)).reshape(n, A, 32, 32, 3)
        patches = HZ.noise_on_views(plain, HZ.SEED, c["keys"], c["amp_s"], c["amp_v"])
        i = int(lay["straddler"])                             # spot checks of the vectorised statement against the pose-by-pose one
        for a in (0, lay["cut"], A - 1):
            assert np.array_equal(patches[i, a], HZ.view(HZ.lands()[c["lands"][i]], HZ.PLAIN32, c["xs"][i], c["ys"][i], c["angs"][i, a], HZ.SEED,
                                                         int(c["keys"][i]), a, c["amp_s"][i], c["amp_v"][i]))
        want = e.ibank_step_batch_u8(np.ascontiguousarray(patches[..., HZ.IM["channel"]]), c["banks"])
        e.noise_rows(HZ.SEED, c["keys"], c["amp_s"], c["amp_v"])
        got = e.ibank_sense_step_batch(c["xs"], c["ys"], c["angs"], c["banks"], land_of_member=c["lands"])
        assert not got.flags.any()
        behind = lay["order"][lay["c0"] // A:]
        same_bits(got.angle_familiarity[behind], want.angle_familiarity[behind], "the members of launch 2")
        same_results(got, want, "688 x 12 at 32 x 32")
    finally:
        e.close()


# ---- 6. the view store -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def store():
    s = HZ.store_case()
    e = engine(HZ.THIN)
    e.noise_rows(HZ.SEED, s["tkeys"], s["tamp_s"], s["tamp_v"])
    views = e.rviews_set_from_poses(s["x"], s["y"], s["angle"], s["first"], land_of_view=s["land_of_view"])
    e.noise_rows(HZ.SEED, s["keys"], s["amp_s"], s["amp_v"])
    yield e, s, views
    e.close()


def test_the_store_holds_the_statements_views(store):
    e, s, views = store
    assert np.array_equal(views, s["views"])
    assert e.rviews_info()["first"].tolist() == [0, 5, 75] and e.noise_info()["n_rows"] == 3


ROUTE_FIELDS = ("angle_familiarity", "angle_view", "best_idex")
LOST = np.array([-np.inf, 1e300, -np.inf])                   # member 1's windowed best is below its threshold: re-localised in the step


def test_the_sads_steps_and_scene_under_rows_equal_their_uploaded_twins(store):
    e, s, _ = store
    p, r, w, l = s["patches"], s["routes"], s["weights"], s["lands"]
    pose = (s["xs"], s["ys"], s["angs"])
    same_results(e.rviews_sense_step(*pose, r, w, land_of_member=l), e.rviews_step_u8(p, r, w), "rviews", ROUTE_FIELDS)
    same_results(e.rviews_sense_step(*pose, r, w, land_of_member=l, exact=True), e.rviews_step_u8(p, r, w, exact=True), "rviews exact", ROUTE_FIELDS)
    same_results(e.rvwin_sense_step(*pose, r, w, s["win_lo"], s["win_hi"], land_of_member=l),
                 e.rvwin_step_u8(p, r, w, s["win_lo"], s["win_hi"]), "rvwin", ROUTE_FIELDS)
    got = e.rvwin_sense_step(*pose, r, w, s["win_lo"], s["win_hi"], land_of_member=l, reloc_below=LOST)
    want = e.rvwin_step_u8(p, r, w, s["win_lo"], s["win_hi"], reloc_below=LOST)
    assert got.relocalised.tolist() == [False, True, False] == want.relocalised.tolist()
    same_results(got, want, "rvwin, re-localised", ROUTE_FIELDS)
    rows, twin = e.rviews_scene(*pose, r, w, land_of_member=l), e.rviews_scene_u8(p, r, w)
    assert [len(x) for x in rows] == [5, 70, 70]
    for i in range(3):
        same_bits(rows[i], twin[i], ("rviews_scene", i))


def test_the_ssd_steps_and_scene_under_rows_equal_their_uploaded_twins(store):
    e, s, _ = store
    p, r, l = s["patches"], s["routes"], s["lands"]
    pose = (s["xs"], s["ys"], s["angs"])
    fields = ROUTE_FIELDS + ("angle_ssd",)
    for ch in (1, 2):
        same_results(e.rvssd_sense_step(*pose, r, ch, land_of_member=l), e.rvssd_step_u8(p, r, ch), ("rvssd", ch), fields)
        same_results(e.rvssdw_sense_step(*pose, r, s["win_lo"], s["win_hi"], ch, land_of_member=l),
                     e.rvssdw_step_u8(p, r, s["win_lo"], s["win_hi"], ch), ("rvssdw", ch), fields)
        got = e.rvssdw_sense_step(*pose, r, s["win_lo"], s["win_hi"], ch, land_of_member=l, reloc_below=LOST)
        want = e.rvssdw_step_u8(p, r, s["win_lo"], s["win_hi"], ch, reloc_below=LOST)
        assert got.relocalised.tolist() == [False, True, False] == want.relocalised.tolist()
        same_results(got, want, ("rvssdw, re-localised", ch), fields)
        rows, twin = e.rvssd_scene(*pose, r, ch, land_of_member=l), e.rvssd_scene_u8(p, r, ch)
        for i in range(3):
            same_bits(rows[i], twin[i], ("rvssd_scene", ch, i))
    # the statement's patches differ from the noiseless ones in the compared channels: the equalities above are not the noiseless ones
    quiet = HZ.member_views(HZ.THIN, s["xs"], s["ys"], s["angs"], l, HZ.SEED, s["keys"], [0] * 3, [0] * 3)
    assert not np.array_equal(e.rvssd_step_u8(quiet, r, 2).angle_ssd, e.rvssd_step_u8(p, r, 2).angle_ssd)


# ---- 7. refusals and the way out -------------------------------------------------------------------------------------------------------------------
def test_refusals_while_rows_are_live_and_the_way_out():
    s = HZ.sense_case("thin")
    e = engine(HZ.THIN)
    try:
        e.noise_rows(HZ.SEED, s["keys"], s["amp_s"], s["amp_v"])
        # a row-count mismatch: refused before anything reaches the device, and the message names both counts
        with pytest.raises(ValueError, match=r"land_of_pose holds 10 entries, but 11 noise rows are live"):
            e.lands_sense(s["x"][:10], s["y"][:10], s["angle"][:10], s["land_of"][:10])
        x, y, a = (np.ascontiguousarray(v[:10]) for v in (s["x"], s["y"], s["angle"]))
        out = np.empty((10, 5, 7, 3), dtype=np.uint8)
        rc = e._lib.dv_lands_sense(e._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(a), np.ascontiguousarray(s["land_of"][:10]).ctypes.data_as(N._i32p), 10,
                                   N.u8ptr(out))
        assert rc == INVALID
        # sensed calls without a landscape table: DV_ERR_STATE
        w, h = HZ.THIN["sensor"]
        e.mb_begin(h, w, HZ.mb_conn("thin"), HZ.MB["n_active"], 2)
        e.mbank_set(2)
        angs = np.tile(s["angle"][:3], (11, 1))
        banks = np.zeros(11, dtype=np.int32)
        with pytest.raises(N.EngineError, match="noise rows are live, and a call without a landscape table senses without noise"):
            e.mbank_sense_step_batch(s["x"], s["y"], angs, banks)
        with pytest.raises(N.EngineError, match="without a landscape table"):
            e.mbank_train_from_poses(s["x"], s["y"], s["angle"], banks)
        with pytest.raises(N.EngineError, match="without a landscape table"):
            e.rviews_set_from_poses(s["x"], s["y"], s["angle"], np.array([0, 5, 11], dtype=np.int64))
        im_begin(e, HZ.THIN, 2)
        with pytest.raises(N.EngineError, match="without a landscape table"):
            e.ibank_sense_step_batch(s["x"], s["y"], angs, banks)
        # uploaded-patch calls are untouched
        planes = np.ascontiguousarray(np.broadcast_to(s["noisy"][:, None, :, :, 2], (11, 3, 5, 7)))
        assert not e.mbank_step_batch_u8(planes[:4], banks[:4]).flags.any()
        # get_sensor_mat's call stays noiseless
        assert np.array_equal(e.sense(s["x"][:2], s["y"][:2], s["angle"][:2]),
                              HZ.views(HZ.THIN, s["x"][:2], s["y"][:2], s["angle"][:2], [0, 0], 0, [0, 0], [0, 0], [0, 0]))
        # a sensor of another w x h drops the rows; the same w x h keeps them
        e.configure_sensor(HZ.THIN["sensor"], HZ.THIN["pixel"], HZ.level_table(HZ.THIN), 0)
        assert e.noise_info()["n_rows"] == 11
        e.configure_sensor((8, 6), (1, 1), HZ.level_table(HZ.THIN), 0)
        assert e.noise_info()["n_rows"] == 0 == e.n_noise_rows
        e.configure_sensor(HZ.THIN["sensor"], HZ.THIN["pixel"], HZ.level_table(HZ.THIN), 0)
        e.noise_rows(HZ.SEED, s["keys"], s["amp_s"], s["amp_v"])
        assert np.array_equal(e.lands_sense(s["x"], s["y"], s["angle"], s["land_of"]), s["noisy"])
        e.noise_clear()
        assert e.noise_info()["n_rows"] == 0
        assert np.array_equal(e.lands_sense(s["x"], s["y"], s["angle"], s["land_of"]), s["plain"])
        assert np.array_equal(e.lands_sense(s["x"][:10], s["y"][:10], s["angle"][:10], s["land_of"][:10]), s["plain"][:10])
    finally:
        e.close()


def test_a_sensed_call_without_a_landscape_table_returns_dv_err_state():
    s = HZ.sense_case("thin")
    e = engine(HZ.THIN)
    try:
        e.noise_rows(HZ.SEED, s["keys"], s["amp_s"], s["amp_v"])
        x, y, a = (np.ascontiguousarray(v) for v in (s["x"], s["y"], s["angle"]))
        first = np.array([0, 5, 11], dtype=np.int64)
        rc = e._lib.dv_rviews_set_from_poses(e._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(a), 11, N.i64ptr(first), 2, None, None)
        assert rc == STATE and b"noise rows are live" in e._lib.dv_last_error(e._ctx)
    finally:
        e.close()


# ---- 8, 9. ensembles -------------------------------------------------------------------------------------------------------------------------------
MODELS = {
    "ssd": (navsim_amd.SsdRouteEnsemble, lambda: ssd_familiarity(2), {}),
    "mushroom": (navsim_amd.MushroomRouteEnsemble, lambda: mushroom_familiarity(**HZ.ENS_MB), {}),
    "sads": (navsim_amd.SadsRouteEnsemble, lambda: sads_familiarity(0.25), dict(window=3)),
    "infomax": (navsim_amd.InfomaxRouteEnsemble, lambda: infomax_familiarity(n_hidden=6, learning_rate=0.01, seed=3), {}),
}
STEPS = 6


def make_agent(model):
    c = HZ.ENS
    return navsim_amd.NavBySceneFamiliarity(np.array(HZ.lands()[0]), c["sensor"], HZ.ENS_STEP, n_test_angles=HZ.ENS_ANGLES, use_gpu_sensor=True,
                                            n_sensor_levels=c["levels"], familiarity_model=model)


def build(name, members=None, noise=HZ.ENS_NOISE, **kw):
    """The ensemble of ens_starts() (members: a subset of them, with their own amplitudes and streams)."""
    E, model, more = MODELS[name]
    starts = HZ.ens_starts()
    if members is not None and noise is not None:
        noise = dict(noise, amp_v=[noise["amp_v"][i] for i in members], streams=[noise["streams"][i] for i in members])
    if members is not None:
        starts = [starts[i] for i in members]
    more = dict(more, **kw)
    if noise is not None:
        more["noise"] = noise
    return E.from_landscapes(make_agent(model()), list(HZ.lands()), HZ.ens_routes(), starts, **more)


def run(ens, steps=STEPS):
    """Per step: every member's (row, position, angle), then the stop codes."""
    out = []
    for _ in range(steps):
        ens.step_forward()
        out.append([(a.angle_familiarity.copy(), tuple(a.position), float(a.angle)) for a in ens.agents])
    return out, list(ens.stop_status)


def assert_member_equals(trace, codes, i, lone_trace, lone_codes, what):
    for t, (step, lone) in enumerate(zip(trace, lone_trace)):
        same_bits(step[i][0], lone[0][0], (what, i, t))
        assert step[i][1] == lone[0][1] and step[i][2] == lone[0][2], (what, i, t)
    assert codes[i] == lone_codes[0], (what, i)


def test_ssd_ensemble_replicates_equal_their_lone_ensembles_and_the_numpy_shadow():
    ens = build("ssd")
    lone = []
    try:
        assert [a.noise_stream for a in ens.agents] == HZ.ENS_NOISE["streams"] and [a.noise_count for a in ens.agents] == [0] * 4
        assert [a.noise_amp for a in ens.agents] == [(0, v) for v in HZ.ENS_NOISE["amp_v"]]
        for a, want in zip(ens.agents, [HZ.ens_train_views()[r] for r, _, _ in HZ.ens_starts()]):
            assert np.array_equal(a.familiar_scenes, want)                                # training under the routes' own keys
        assert ens.engine.noise_info()["n_rows"] == 0                                      # no rows between training and the first step
        # the first step, then its scene: the scene of the patches that step scored
        ens.step_forward()
        shadows = [HZ.shadow(i, 3) for i in range(4)]
        first_rows = [a.angle_familiarity.copy() for a in ens.agents]
        for i in range(4):
            same_bits(first_rows[i], shadows[i][0]["fam"], ("shadow", i, 0))
        assert not np.array_equal(first_rows[0], first_rows[1])                           # one pose, two streams
        patches = np.stack([shadows[i][0]["patches"] for i in range(4)])
        routes = [r for r, _, _ in HZ.ens_starts()]
        scene = ens.scene_familiarity()
        twin = ens.engine.rvssd_scene_u8(patches, routes, 2)
        for i in range(4):
            same_bits(scene[i], np.negative(twin[i]), ("scene", i))
        assert [a.noise_count for a in ens.agents] == [1] * 4                              # (the scene re-senses: it is no step)
        trace = [[(first_rows[i], tuple(a.position), float(a.angle)) for i, a in enumerate(ens.agents)]]
        more, codes = run(ens, STEPS - 1)
        trace += more
        for i in range(4):
            for t in range(3):
                same_bits(trace[t][i][0], shadows[i][t]["fam"], ("shadow", i, t))
                assert trace[t][i][1] == tuple(shadows[i][t]["position"]) and trace[t][i][2] == float(shadows[i][t]["angle"]), (i, t)
        assert [a.noise_count for a in ens.agents] == [STEPS] * 4
        for i in range(4):
            one = build("ssd", members=[i])
            lone.append(one)
            assert_member_equals(trace, codes, i, *run(one), "ssd")
    finally:
        ens.engine.close()
        for one in lone:
            one.engine.close()


def test_a_fake_run_does_not_repeat_its_draws():
    ens = build("ssd", members=[0])
    try:
        ens.step_forward(fake=True)
        a = ens.agents[0]
        assert a.noise_count == 1
        rows = [a.angle_familiarity.copy()]
        a.position, a.angle = HZ.ens_starts()[0][1], HZ.ens_starts()[0][2]                # back to the start: the same pose, the next draws
        ens.step_forward(fake=True)
        rows.append(a.angle_familiarity.copy())
        assert a.noise_count == 2 and not np.array_equal(rows[0], rows[1])
    finally:
        ens.engine.close()


@pytest.mark.parametrize("name", ("mushroom", "sads", "infomax"))
def test_the_other_ensembles_members_equal_their_lone_ensembles(name):
    ens = build(name)
    lone = []
    try:
        trace, codes = run(ens)
        if name == "mushroom":
            for i in range(4):
                same_bits(trace[0][i][0], HZ.mushroom_first_row(i), ("the mushroom statement", i))
            assert not np.array_equal(trace[0][0][0], trace[0][1][0])                     # one pose, two streams
        if name == "sads":
            assert all(a.window == (3, 3) for a in ens.agents) and all(a.memory_index is not None for a in ens.agents)
        for i in range(4):
            one = build(name, members=[i])
            lone.append(one)
            assert_member_equals(trace, codes, i, *run(one), name)
    finally:
        ens.engine.close()
        for one in lone:
            one.engine.close()


def test_a_windowed_ensembles_two_calls_each_get_their_own_members_rows():
    """Members 0 and 2 with a window and a centre, 1 and 3 without: two device calls a step, each under its own members' rows."""
    window = [2, None, (1, 4), None]
    centres = [3, None, 2, None]
    ens = build("ssd", window=window, window_centres=centres)
    lone = []
    try:
        trace, codes = run(ens, 3)
        for i in range(4):
            one = build("ssd", members=[i], window=[window[i]], window_centres=[centres[i]])
            lone.append(one)
            assert_member_equals(trace, codes, i, *run(one, 3), "windowed ssd")
    finally:
        ens.engine.close()
        for one in lone:
            one.engine.close()


@pytest.mark.parametrize("name", sorted(MODELS))
def test_noise_none_is_the_ensemble_built_without_the_argument(name):
    E, model, more = MODELS[name]
    with_none = E.from_landscapes(make_agent(model()), list(HZ.lands()), HZ.ens_routes(), HZ.ens_starts(), noise=None, **more)
    without = E.from_landscapes(make_agent(model()), list(HZ.lands()), HZ.ens_routes(), HZ.ens_starts(), **more)
    try:
        calls = []
        with_none.engine.noise_rows = lambda *a, **k: calls.append(a)
        a, ca = run(with_none, 3)
        b, cb = run(without, 3)
        assert calls == [] and with_none.engine.noise_info()["n_rows"] == 0
        assert [m.noise_stream for m in with_none.agents] == [None] * 4 and [m.noise_count for m in with_none.agents] == [0] * 4
        for t in range(3):
            for i in range(4):
                same_bits(a[t][i][0], b[t][i][0], (name, t, i))
                assert a[t][i][1:] == b[t][i][1:]
        assert ca == cb
        assert np.array_equal(a[0][0][0], a[0][1][0], equal_nan=True)                     # one pose, no noise: the same row
    finally:
        with_none.engine.close()
        without.engine.close()
