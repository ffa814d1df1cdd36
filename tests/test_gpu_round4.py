"""GPU parity tests added in round 4: the dense full-library check at BASELINE configs[2], steps of more than 64 headings,
the SSD familiarity plug-in behind the agent, ssd_f32 at configs[2]'s literal float32 size, the clean-up paths of the SSD
ingests and the kernel knobs a context reads at creation.  Everything calls libdejavu_hip.so through navsim_amd (ctypes);
the oracle (oracle/) is the checker only; nothing reads /root/reference.
"""
import ctypes

import numpy as np
import pytest

import navsim_amd
from navsim_amd import synth
from navsim_amd import _native as N
from oracle import oracle
from tests.helpers import ENGINE_MODES, engine_mode, engine_with

pytestmark = pytest.mark.gpu

RTOL = 1e-9


# ------------------------------------------------------------------ dense check at the size the headline is quoted on
def _dense_fam(seed, F, h, w, cw, patch, full_range_s=False):
    s_hs, s_v = oracle.synth_int_sums(seed, 0, F, h, w, patch, full_range_s=full_range_s)
    return oracle.fam_from_sums(s_hs, s_v, h * w, cw)


def test_dense_oracle_at_config_two():
    """BASELINE configs[2] (128x128 sensor, 500 000 views, 32 headings), EVERY view against the oracle.

    The sampled checks of test_large_library_properties see ~130 of the 500 000 views; the machinery that only exists at
    this size (7.63 view-group ranges per workgroup, loaders running through item boundaries, the partial eighth round, the
    accumulators changing hands at the segment boundary) deserves all of them.  The oracle's integer sums (util.pyx:48-56,69)
    are computed for every view of the synthetic library, each view regenerated inside the C loop (oracle_synth_int_sums,
    pinned to oracle_int_sums by tests/test_oracle_golden.py); fam = P - (0.5 cw S_hs + (1 - cw) S_v) / 255 is within 1e-12
    of the reference's sequential doubles, and one unit of either sum moves a score by >= 5e-4, so rtol 1e-9 on ~16 000 is
    a bit-level check of the sums.

    (a) one-heading steps with want_scene: scene_familiarity[f] = fam[0, f] for ALL f -- an on-level patch (fp4 body of the
        matrix-core kernel, unfused epilogue + k_finish) and an off-level one (its int8 body in the same launch);
    (b) the step as it ships (32 headings, fused epilogue, k_fold): three headings' maxima and first maximisers against the
        dense oracle's max / first argmax over all 500 000 views;
    (c) the mixed layout (saturation 0..127 kept as byte planes, value bits on the matrix cores): one heading, all views."""
    if not oracle.have_omp():
        pytest.skip("oracle/liboracle_omp.so is not built")
    F, h, w, A, seed, cw = 500000, 128, 128, 32, 777, 0.25
    eng = navsim_amd.FamiliarityEngine(device=0)
    try:
        eng.generate_library(seed, F, h, w, cw)
        patches = synth.synth_patches(seed, A, h, w)
        patches[30] = synth.near_match_patch(synth.synth_views(seed, 1, h, w, first_view=3)[0], 130, fraction=0.01)
        # (a) on-level patch: all 500 000 scores
        r = eng.step(patches[7:8], want_scene=True)
        form = eng.scoring_form()
        assert form["matrix_cores"] and form["fp4"] and not form["fused_finish"], form
        want = _dense_fam(seed, F, h, w, cw, patches[7])
        np.testing.assert_allclose(r["scene_familiarity"], want, rtol=RTOL)
        assert r["angle_view"][0] == int(np.argmax(want)) and r["best_view"] == int(np.argmax(want))
        # ... and an off-level patch (bytes strictly inside the library's gaps): the int8 body of the same kernel
        off = patches[7].copy()
        off[::3, ::5, 2] = 100                                       # between the levels 63 and 127
        off[1::4, 2::7, 1] = 50                                      # between the saturations 0 and 127
        r = eng.step(off[None], want_scene=True)
        form = eng.scoring_form()
        assert form["matrix_cores"] and not form["fp4"], form
        want = _dense_fam(seed, F, h, w, cw, off)
        np.testing.assert_allclose(r["scene_familiarity"], want, rtol=RTOL)
        assert r["angle_view"][0] == int(np.argmax(want))
        # (b) the shipped step: fused epilogue + k_fold, 32 headings; three of them against every view
        r = eng.step(patches, want_scene=False)
        form = eng.scoring_form()
        assert form["matrix_cores"] and form["fp4"] and form["fused_finish"], form
        assert r["best_idex"] == 30 and r["best_view"] == 3
        for a in (0, 13, 30):
            want = _dense_fam(seed, F, h, w, cw, patches[a])
            np.testing.assert_allclose(r["angle_familiarity"][a], want.max(), rtol=RTOL)
            assert r["angle_view"][a] == int(np.argmax(want)), a
        # (c) mixed layout
        eng.generate_library(seed, F, h, w, cw, full_range_s=True)
        assert eng.library_info()["mixed_layout"]
        pm = synth.synth_patches(seed, 2, h, w, full_range_s=True)
        r = eng.step(pm[1:2], want_scene=True)
        want = _dense_fam(seed, F, h, w, cw, pm[1], full_range_s=True)
        np.testing.assert_allclose(r["scene_familiarity"], want, rtol=RTOL)
        assert r["angle_view"][0] == int(np.argmax(want))
    finally:
        eng.close()


# ------------------------------------------------------------------ more than 64 headings
@pytest.fixture(scope="module", params=ENGINE_MODES)
def eng(request):
    e = engine_mode(request.param)
    e.mode = request.param
    yield e
    e.close()


@pytest.mark.parametrize("A,F,h,w,cw", [(65, 700, 8, 8, 0.0), (90, 3000, 8, 8, 0.25), (130, 257, 9, 7, 1.0), (200, 3000, 16, 16, 0.4)])
def test_wide_steps_match_the_reference(eng, A, F, h, w, cw):
    """The reference takes any n_test_angles (NavBySceneFamiliarity.py:62,87-88; loop :289, argmax :315): steps of more than
    DV_MAX_HEADINGS headings run as ceil(A / 64) library passes merged inside the library.  Small five-level sensors make
    equal integer sums with ulp-different doubles common, so the passes' near-ties go through the exact
    resolver; exact duplicates across passes must go to the first heading."""
    lib = synth.synth_views(91, F, h, w)
    patches = synth.synth_patches(91, A, h, w)
    eng.set_library(lib, cw)
    cases = []
    cases.append(("random", patches.copy()))
    p = patches.copy()
    p[A - 3] = lib[F // 3]                                          # an exact copy in the LAST pass: the strict winner
    cases.append(("winner in the last pass", p))
    p = patches.copy()
    p[A - 2] = lib[F // 2]
    p[5] = lib[F // 5]                                              # exact copies in the first and the last pass: both score h*w
    cases.append(("exact tie across passes", p))
    p = patches.copy()
    p[70 % A] = p[3]                                                # the same patch twice, one per pass
    p[64] = p[0]
    cases.append(("duplicate headings", p))
    for name, pats in cases:
        want = oracle.step(lib, pats, cw)
        got = eng.step(pats, want_scene=True)
        assert got["n_passes"] == (A + 63) // 64
        assert got["best_idex"] == want["best_idex"], (name, got["best_idex"], want["best_idex"], got["n_contending"])
        assert got["best_view"] == want["best_view"], name
        np.testing.assert_allclose(got["angle_familiarity"], want["angle_familiarity"], rtol=RTOL)
        np.testing.assert_allclose(got["scene_familiarity"], want["scene_familiarity"], rtol=RTOL)
        np.testing.assert_allclose(got["step_familiarity"], want["step_familiarity"], rtol=RTOL)
        fast = eng.step(pats, want_scene=False)                      # the passes enqueued back to back
        assert (fast["best_idex"], fast["best_view"]) == (want["best_idex"], want["best_view"]), name
        np.testing.assert_allclose(fast["angle_familiarity"], want["angle_familiarity"], rtol=RTOL)
        forced = eng.step(pats, want_scene=False, force_resolve=True)
        assert forced["best_idex"] == want["best_idex"] and forced["step_familiarity"] == want["step_familiarity"], name


def test_wide_step_on_the_tie_stress_fixture(manifest):
    """The golden tie-stress library (8x8 five-level views, 20 000 of them: hundreds of equal integer sums with different
    doubles) with its 8 patches repeated over 72 headings in a rotated order: every pass holds every patch, so the maximum is
    attained in both passes and the first heading must win on exact values."""
    from tests.helpers import step_case_inputs
    case = [c for c in manifest["t2_step"] if c["name"].startswith("s_ties")][0]
    lib, patches = step_case_inputs(case)
    A0 = patches.shape[0]
    order = [(3 * i + 1) % A0 for i in range(72)]
    pats = np.ascontiguousarray(patches[order])
    want = oracle.step(lib, pats, case["chem_weight"])
    for env in ({}, {"DEJAVU_SHAPE": "6", "DEJAVU_BITS": "2"}):
        e = engine_with(env)
        try:
            e.set_library(lib, case["chem_weight"])
            got = e.step(pats, want_scene=False)
            assert got["best_idex"] == want["best_idex"] and got["best_view"] == want["best_view"]
            assert got["n_contending"] == 2
            assert got["step_familiarity"] == want["step_familiarity"]         # exact after the forced resolve
        finally:
            e.close()


def test_agent_with_ninety_test_angles():
    """NavBySceneFamiliarity(n_test_angles=90) -- more than one library pass per step -- walks the trajectory of the same agent
    scored by the oracle plug-in with the host sensor model (the reference's loop, one model call per heading)."""
    land = synth.synth_landscape(8, 400, 4)
    path = synth.sin_training_path(0.5, 60, 260, arclen=1.0)[:200]
    kw = dict(n_test_angles=90, n_sensor_levels=5, saccade_degrees=180.)
    dev = navsim_amd.NavBySceneFamiliarity(land, (16, 16), 1.0, familiarity_model=navsim_amd.sads_familiarity(0.25),
                                           track_scene_familiarity=False, **kw)
    ref = navsim_amd.NavBySceneFamiliarity(land, (16, 16), 1.0, familiarity_model=oracle.sads_familiarity(0.25),
                                           use_gpu_sensor=False, **kw)
    for nsf in (dev, ref):
        nsf.train_from_path(path)
        nsf.position, nsf.angle = (path[2][0] + 0.6, path[2][1] - 0.3), 0.8
    assert np.array_equal(dev.familiar_scenes, ref.familiar_scenes)
    for t in range(40):
        dev.step_forward(fake=True)
        ref.step_forward(fake=True)
        assert dev.last_best_idex == ref.last_best_idex, t
        assert dev.position == ref.position and dev.angle == ref.angle, t
        np.testing.assert_allclose(dev.angle_familiarity, ref.angle_familiarity, rtol=RTOL)
    dev.track_scene_familiarity = True                               # and the per-view minimum over all 90 headings
    dev.step_forward(fake=True)
    ref.step_forward(fake=True)
    np.testing.assert_allclose(dev.scene_familiarity, ref.scene_familiarity, rtol=RTOL)
    dev.clear_training()


def test_wide_step_errors(eng):
    lib = synth.synth_views(3, 100, 8, 8)
    eng.set_library(lib, 0.0)
    with pytest.raises(ValueError):
        eng.step(np.zeros((N.DV_MAX_WIDE_HEADINGS + 1, 8, 8, 3), dtype=np.uint8))
    r = eng.step(np.repeat(lib[17:18], 64 * 3, axis=0), want_scene=False)      # 192 identical headings: the first wins
    assert (r["best_idex"], r["best_view"], r["n_passes"]) == (0, 17, 3)


# ------------------------------------------------------------------ SSD as the agent's familiarity plug-in
def _host_ssd_model(channel):
    """The reference-shaped plug-in with `ssds` (navsim/util.pyx:171-184) as its metric, on the host: the checker of the device
    plug-in.  uint8 differences squared and summed in float64 are exact integers, so NumPy's sum IS oracle.ssds' value (spot
    checks below call oracle.ssds itself, which tests/test_oracle_golden.py pins to the reference's)."""
    def model(scenes):
        planes = scenes[..., channel].astype(np.float64)

        def func(scene, fambuf):
            d = planes - scene[..., channel].astype(np.float64)
            fambuf[:] = -(d * d).sum(axis=(1, 2))
        func.max_familiarity = 0.0
        return func
    return model


@pytest.mark.parametrize("channel", [2, 1])
def test_ssd_plugin_pairs_against_the_reference_ssds(channel):
    """ssd_familiarity(channel)(scenes) -> func(scene, fambuf): the reference's two-stage plug-in shape (util.pyx:10-25) with the
    north star's literal metric; every pair is the exact integer oracle.ssds returns."""
    rng = np.random.default_rng(12)
    scenes = rng.integers(0, 256, (300, 12, 20, 3), dtype=np.uint8)
    func = navsim_amd.ssd_familiarity(channel)(scenes)
    assert func.max_familiarity == 0.0 and func.metric == "ssd_u8" and func.channel == channel
    scene = rng.integers(0, 256, (12, 20, 3), dtype=np.uint8)
    scene[3:9] = scenes[77, 3:9]
    fam = np.full(300, np.nan)
    func(scene, fam)
    for f in (0, 77, 150, 299):
        assert fam[f] == -oracle.ssds(scene[..., channel].astype(np.float64), scenes[f, ..., channel].astype(np.float64))
    want = np.empty(300)
    _host_ssd_model(channel)(scenes)(scene, want)
    assert np.array_equal(fam, want)
    with pytest.raises(ValueError):
        func(scene, np.empty(300, dtype=np.float32))                 # "Buffer dtype mismatch", like the reference's kernel
    with pytest.raises(ValueError):
        navsim_amd.ssd_familiarity(channel)(scenes.astype(np.int16))
    func.engine.close()
    # float32 scenes take the ssd_f32 metric: within 1e-6 relative of ssds on the upcast data
    fs = rng.random((200, 12, 20), dtype=np.float32)
    func = navsim_amd.ssd_familiarity(channel)(fs)
    assert func.metric == "ssd_f32"
    q = (fs[40] + 0.01 * rng.random((12, 20), dtype=np.float32)).astype(np.float32)
    fam = np.empty(200)
    func(q, fam)
    want = np.array([-oracle.ssds(q.astype(np.float64), v.astype(np.float64)) for v in fs])
    np.testing.assert_allclose(fam, want, rtol=1e-6)
    assert int(np.argmax(fam)) == 40
    func.engine.close()


def test_agent_with_the_ssd_plugin_walks_the_host_loops_trajectory():
    """step_forward with ssd_familiarity: sense -> score (int8 matrix cores) -> decide on the device (dv_sense_step_u8),
    against the same agent running the reference's loop -- one `func(scene, fambuf)` call per heading, host sensor model,
    host SSD -- over 250 steps: heading index, pose and every per-heading familiarity equal (the SSDs are exact integers)."""
    land = synth.synth_landscape(5, 500, 4)
    path = synth.sin_training_path(0.5, 60, 380, arclen=1.0)[:330]
    kw = dict(n_test_angles=12, n_sensor_levels=256, saccade_degrees=120.)
    dev = navsim_amd.NavBySceneFamiliarity(land, (32, 32), 1.0, familiarity_model=navsim_amd.ssd_familiarity(2), **kw)
    ref = navsim_amd.NavBySceneFamiliarity(land, (32, 32), 1.0, familiarity_model=_host_ssd_model(2), use_gpu_sensor=False, **kw)
    for nsf in (dev, ref):
        nsf.train_from_path(path)
        nsf.position, nsf.angle = (path[3][0] + 0.7, path[3][1] - 0.4), 0.9
    assert dev._familiarity_func.metric == "ssd_u8" and dev._familiarity_func.engine is dev._engine
    assert np.array_equal(dev.familiar_scenes, ref.familiar_scenes)
    for t in range(250):
        dev.step_forward(fake=(t % 2 == 0))
        ref.step_forward(fake=(t % 2 == 0))
        assert dev.last_best_idex == ref.last_best_idex, t
        assert dev.position == ref.position and dev.angle == ref.angle, t
        assert np.array_equal(dev.angle_familiarity, ref.angle_familiarity), t
        assert np.array_equal(dev.scene_familiarity, ref.scene_familiarity), t
    assert dev.navigation_error == ref.navigation_error
    assert dev.percent_recapitulated == ref.percent_recapitulated
    # off the landscape: the reference's stop exception, raised before anything is sensed
    dev.position = (3.0, 3.0)
    with pytest.raises(navsim_amd.OutOfLandscapeBoundsException):
        dev.step_forward()
    # a second training path: the SSD library is ingested again with the new views
    more = synth.sin_training_path(0.3, 80, 200, arclen=1.0)[:90]
    dev.train_additional_path(more)
    ref.train_additional_path(more)
    dev.position = ref.position = (more[5][0] + 0.3, more[5][1])
    dev.angle = ref.angle = 0.7
    dev.step_forward(fake=True)
    ref.step_forward(fake=True)
    assert dev.last_best_idex == ref.last_best_idex and np.array_equal(dev.angle_familiarity, ref.angle_familiarity)
    dev.clear_training()


def test_ssd_plugin_with_the_host_sensor_model():
    """The same plug-in under an agent that senses on the host (use_gpu_sensor=False): patches are uploaded, the step is
    step_u8 -- still one device step per step_forward."""
    land = synth.synth_landscape(6, 300, 4)
    path = synth.sin_training_path(0.5, 60, 180, arclen=1.0)[:120]
    kw = dict(n_test_angles=9, n_sensor_levels=5, use_gpu_sensor=False)
    dev = navsim_amd.NavBySceneFamiliarity(land, (16, 16), 1.0, familiarity_model=navsim_amd.ssd_familiarity(2), **kw)
    ref = navsim_amd.NavBySceneFamiliarity(land, (16, 16), 1.0, familiarity_model=_host_ssd_model(2), **kw)
    for nsf in (dev, ref):
        nsf.train_from_path(path)
        nsf.position, nsf.angle = (path[3][0] + 0.7, path[3][1] - 0.4), 0.9
    for t in range(30):
        dev.step_forward(fake=True)
        ref.step_forward(fake=True)
        assert dev.last_best_idex == ref.last_best_idex and dev.position == ref.position, t
        assert np.array_equal(dev.angle_familiarity, ref.angle_familiarity)
    dev.clear_training()


# ------------------------------------------------------------------ clean-up paths and small fixes of the round-3 review
@pytest.mark.parametrize("metric,n_allocs", [("u8", 6), ("f32", 10)])
def test_allocation_failure_leaves_no_library(metric, n_allocs):
    """A failed allocation inside an SSD ingest must not leave a half-built library behind (the step calls would launch kernels
    on null pointers): every allocation of the ingest is failed in turn (DEJAVU_TEST_FAIL_ALLOC), the call reports
    DV_ERR_OOM, the step answers DV_ERR_STATE, and the same context takes the library afterwards."""
    rng = np.random.default_rng(2)
    if metric == "u8":
        views = rng.integers(0, 256, (200, 10, 12), dtype=np.uint8)
        pats = rng.integers(0, 256, (4, 10, 12), dtype=np.uint8)
    else:
        views = rng.random((200, 10, 12), dtype=np.float32)
        pats = rng.random((4, 10, 12), dtype=np.float32)
    for k in range(1, n_allocs + 1):
        e = engine_with({"DEJAVU_TEST_FAIL_ALLOC": str(k)})
        try:
            with pytest.raises(navsim_amd.EngineError, match="DV_ERR_OOM"):
                (e.set_library_u8 if metric == "u8" else e.set_library_f32)(views)
            res = N.StepResult()                                     # (the C calls themselves: the Python face has no shape to check against)
            if metric == "u8":
                rc = e._lib.dv_step_u8(e._ctx, N.u8ptr(pats), 4, 0, ctypes.byref(res), None)
            else:
                rc = e._lib.dv_step_f32(e._ctx, pats.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 4, 0, ctypes.byref(res), None)
            assert rc == -3, rc                                      # DV_ERR_STATE: no library
            assert e._lib.dv_get_library_info(e._ctx, ctypes.byref(N.LibInfo())) == -3
        finally:
            e.close()
    e = engine_with({"DEJAVU_TEST_FAIL_ALLOC": str(n_allocs + 1)})      # past the ingest's allocations: nothing fails
    try:
        (e.set_library_u8 if metric == "u8" else e.set_library_f32)(views)
        r = (e.step_u8 if metric == "u8" else e.step_f32)(pats)
        assert 0 <= r["best_idex"] < 4
    finally:
        e.close()


def test_resolve_after_an_ssd_u8_step_is_a_no_op():
    """dv_resolve on an ssd_u8 step (every score exact already) must not reach the sads_hsv resolver, whose tiles do not exist."""
    rng = np.random.default_rng(4)
    views = rng.integers(0, 256, (300, 20, 24), dtype=np.uint8)
    views[200] = views[10]
    pats = rng.integers(0, 256, (5, 20, 24), dtype=np.uint8)
    pats[3] = views[10]
    e = navsim_amd.FamiliarityEngine(0)
    try:
        e.set_library_u8(views)
        r = e.step_u8(pats)
        assert (r["best_idex"], r["best_view"], r["step_ssd"]) == (3, 10, 0.0)
        r2 = e.resolve()
        assert (r2["best_idex"], r2["best_view"]) == (3, 10)
        r3 = e.step_u8(pats)                                         # and the engine is fine afterwards
        assert (r3["best_idex"], r3["best_view"]) == (3, 10)
    finally:
        e.close()


@pytest.mark.parametrize("env", [{"DEJAVU_LC": "0"}, {"DEJAVU_LC": "2"}, {"DEJAVU_HT": "1"}, {"DEJAVU_MIXED": "0"},
                                 {"DEJAVU_LC": "0", "DEJAVU_RING": "1"}, {"DEJAVU_LC": "0", "DEJAVU_RING": "2"}, {"DEJAVU_TUNE_ALL": "1"}])
def test_body_knobs_are_read_per_context(env):
    """DEJAVU_LC / DEJAVU_HT / DEJAVU_RING / DEJAVU_MIXED select kernel bodies; they are fields of the context read at
    dv_create (they used to be process-wide statics: a second engine silently ignored a changed value).  Each body on a small
    library with 33..64 resident headings (two heading tiles) and with 13, against the oracle and against the default body."""
    F, h, w, cw = 7000 + 19, 16, 12, 0.25
    full = env.get("DEJAVU_MIXED") is not None
    lib = synth.synth_views(71, F, h, w, full_range_s=full)
    base = {"DEJAVU_SHAPE": "6", "DEJAVU_BITS": "2", "DEJAVU_MFMA_CHUNK": "1"}     # one K chunk: the loader / consumer body even at this size
    e_def = engine_with(base)
    e_knob = engine_with(dict(base, **env))
    try:
        for e in (e_def, e_knob):
            e.set_library(lib, cw)
        if full:
            assert e_def.library_info()["mixed_layout"] and not e_knob.library_info()["mixed_layout"]
        for A in (13, 40, 64):
            pats = synth.synth_patches(200 + A, A, h, w, full_range_s=full)
            pats[A // 2] = synth.near_match_patch(lib[(A * 131) % F], A, fraction=0.03)
            want = oracle.step(lib, pats, cw)
            for e in (e_def, e_knob):
                for it in range(3):
                    got = e.step(pats, want_scene=(it == 1))
                    assert (got["best_idex"], got["best_view"]) == (want["best_idex"], want["best_view"]), (env, A)
                    np.testing.assert_allclose(got["angle_familiarity"], want["angle_familiarity"], rtol=RTOL)
                    if it == 1:
                        np.testing.assert_allclose(got["scene_familiarity"], want["scene_familiarity"], rtol=RTOL)
    finally:
        e_def.close()
        e_knob.close()


def test_fenced_ticket_is_the_default_on_long_passes():
    """The release / acquire pair around k_finish's arrival ticket is the default wherever the scoring pass is long (>= 200 us
    estimated): the byte path and the mixed layout at large sizes.  Checked through the decisions of both forms on a library
    large enough to take the fenced default (duplicated best views in far-apart blocks), and DEJAVU_FENCED still overrides."""
    F, h, w, A, cw = 120000, 32, 32, 16, 0.25                        # byte tiles 246 MB -> fenced by default; bit tiles 92 MB
    seen = {}
    for name, env in (("default bytes", {"DEJAVU_BITS": "0", "DEJAVU_FINISH": "2"}),
                      ("unfenced bytes", {"DEJAVU_BITS": "0", "DEJAVU_FINISH": "2", "DEJAVU_FENCED": "0"})):
        e = engine_with(env)
        try:
            e.generate_library(31, F, h, w, cw)
            pats = synth.synth_patches(31, A, h, w)
            pats[9] = synth.near_match_patch(synth.synth_views(31, 1, h, w, first_view=119999)[0], 4, fraction=0.02)
            for _ in range(5):
                r = e.step(pats, want_scene=True)
                assert (r["best_idex"], r["best_view"]) == (9, 119999), name
            seen[name] = (np.array(r["angle_familiarity"]), np.array(r["scene_familiarity"]))
        finally:
            e.close()
    assert np.array_equal(seen["default bytes"][0], seen["unfenced bytes"][0])
    assert np.array_equal(seen["default bytes"][1], seen["unfenced bytes"][1])


# ------------------------------------------------------------------ ssd_f32: device generator, configs[2] in its literal form
def test_generated_f32_library_equals_uploaded():
    F, h, w, A = 3000, 24, 20, 16
    lib = synth.synth_views_f32(9, F, h, w, first_view=50)
    rng = np.random.default_rng(1)
    pats = rng.random((A, h, w), dtype=np.float32)
    pats[6] = lib[1234] + np.float32(0.001) * rng.random((h, w), dtype=np.float32)
    a, b = navsim_amd.FamiliarityEngine(0), navsim_amd.FamiliarityEngine(0)
    try:
        a.set_library_f32(lib, first_view=50)
        b.generate_library_f32(9, F, h, w, first_view=50)
        ra, rb = a.step_f32(pats, want_scene=True), b.step_f32(pats, want_scene=True)
        assert (ra["best_idex"], ra["best_view"]) == (rb["best_idex"], rb["best_view"]) == (6, 50 + 1234)
        assert np.array_equal(ra["angle_ssd"], rb["angle_ssd"]) and np.array_equal(ra["scene_ssd"], rb["scene_ssd"])
    finally:
        a.close()
        b.close()


def test_ssd_f32_at_config_two_literal_size():
    """BASELINE configs[2] as BASELINE.json words it: 128x128 sensor, 500 000 stored views, 32 headings, fp32 -- 32.8 GB of
    float32 views generated on the device -- through size-independent properties: planted near-copies in the first, a middle
    and the last view group win at their headings, the closest wins the step; every reported minimum is the SSD of the
    reported view to 1e-6 relative of oracle.ssds (util.pyx:171-184) on that view regenerated on the host; no view of a fixed
    spread beats the reported minima; two half libraries reproduce the full library's minima and views."""
    F, h, w, A, seed = 500000, 128, 128, 32, 4242
    eng = navsim_amd.FamiliarityEngine(0)
    try:
        eng.generate_library_f32(seed, F, h, w)
        rng = np.random.default_rng(7)
        pats = rng.random((A, h, w), dtype=np.float32)
        targets = {4: (499999, 0.02), 19: (250001, 0.01), 27: (3, 0.03)}
        for a, (f, eps) in targets.items():
            v = synth.synth_views_f32(seed, 1, h, w, first_view=f)[0]
            pats[a] = v + np.float32(eps) * rng.random((h, w), dtype=np.float32)
        r = eng.step_f32(pats)
        for a, (f, _) in targets.items():
            assert r["angle_view"][a] == f, (a, r["angle_view"][a])
        assert r["best_idex"] == 19 and r["best_view"] == 250001
        spread = np.unique(np.concatenate([np.arange(0, F, F // 61), np.asarray(r["angle_view"], dtype=np.int64)]))
        views = {int(f): synth.synth_views_f32(seed, 1, h, w, first_view=int(f))[0].astype(np.float64) for f in spread}
        for a in range(A):
            pa = pats[a].astype(np.float64)
            want = oracle.ssds(pa, views[int(r["angle_view"][a])])
            np.testing.assert_allclose(r["angle_ssd"][a], want, rtol=1e-6)
            if a % 8 == 3:
                assert min(oracle.ssds(pa, v) for v in views.values()) >= want * (1 - 1e-6), a
        full_min, full_view = np.array(r["angle_ssd"]), np.array(r["angle_view"])
        halves = []
        for lo, hi in ((0, F // 2), (F // 2, F)):
            eng.generate_library_f32(seed, hi - lo, h, w, first_view=lo)
            halves.append(eng.step_f32(pats))
        merged = np.minimum(halves[0]["angle_ssd"], halves[1]["angle_ssd"])
        assert np.array_equal(merged, full_min)
        pick = np.where(halves[0]["angle_ssd"] <= halves[1]["angle_ssd"], halves[0]["angle_view"], halves[1]["angle_view"])
        assert np.array_equal(pick, full_view)
    finally:
        eng.close()


@pytest.mark.parametrize("F,h,w,A", [(1, 1, 1, 1), (130, 5, 7, 3), (300, 16, 16, 16), (64, 9, 31, 8), (257, 32, 32, 10), (200, 12, 12, 32),
                                     (150, 10, 14, 64), (90, 7, 9, 37), (4100, 64, 64, 17), (9000, 24, 24, 33), (700, 128, 128, 12)])
def test_ssd_f32_on_the_matrix_cores_reports_the_references_doubles(F, h, w, A):
    """step_f32 without per-view output takes the cross-term form on the fp32 matrix cores (k_ssd_f32_mfma: it only SELECTS, the
    listed pairs are re-scored in the reference's sequential double arithmetic): every per-heading minimum must be the double
    `ssds` (util.pyx:171-184, via the pinned oracle) returns for the reported view -- bit for bit -- and the view the true first
    minimiser; ragged shapes (pixels not a multiple of 4, 1..64 headings = the 16-wide and the 32-wide instruction, one and two
    passes, several pixel chunks per view group), near matches whose SSD is 1e-6 of the norms, exact duplicates.  The direct
    form (DEJAVU_SSD_MFMA=0: k_ssd_tiles) must agree to its 1e-6."""
    rng = np.random.default_rng(F * 13 + A)
    lib = rng.uniform(-3, 3, (F, h, w)).astype(np.float32)
    patches = rng.uniform(-3, 3, (A, h, w)).astype(np.float32)
    if F > 100:
        patches[A // 2] = lib[F // 3] + rng.normal(0, 0.001, (h, w)).astype(np.float32)    # a near match: SSD ~1e-6 of the norms
        lib[F - 1] = lib[F // 7]                                                             # an exact duplicate of a view ...
        patches[0] = lib[F // 7]                                                             # ... that a heading looks at: SSD 0 twice
    want = np.empty((A, F))
    l64 = lib.astype(np.float64)
    for a in range(A):
        d = l64 - patches[a].astype(np.float64)
        want[a] = (d * d).reshape(F, -1).sum(axis=1)                  # near the oracle's value: used to find the few pairs it scores
    e_new, e_old = engine_with({}), engine_with({"DEJAVU_SSD_MFMA": "0"})
    try:
        for e in (e_new, e_old):
            e.set_library_f32(lib)
        r = e_new.step_f32(patches)
        assert r["flags"] & 1                                         # decided on exact values
        for a in range(A):
            f = int(r["angle_view"][a])
            exact = oracle.ssds(patches[a].astype(np.float64), l64[f])
            assert r["angle_ssd"][a] == exact, (a, f)
            # the first true minimiser: no view scores lower, and none of a lower index ties with it
            near = np.flatnonzero(want[a] <= exact * (1 + 1e-9) + 1e-300)
            ex = np.array([oracle.ssds(patches[a].astype(np.float64), l64[k]) for k in near])
            assert ex.min() == exact and int(near[int(np.argmin(ex))]) == f, (a, f, near[:5])
        best = int(np.argmin(r["angle_ssd"]))
        assert r["best_idex"] == best and r["best_view"] == int(r["angle_view"][best]) and r["step_ssd"] == r["angle_ssd"][best]
        if F > 100:
            assert r["best_idex"] == 0 and r["best_view"] == F // 7 and r["step_ssd"] == 0.0
        r0 = e_old.step_f32(patches)
        assert (r0["best_idex"], r0["best_view"]) == (r["best_idex"], r["best_view"])
        np.testing.assert_allclose(r0["angle_ssd"], r["angle_ssd"], rtol=1e-6, atol=1e-12)
        for _ in range(3):                                            # repeatable
            again = e_new.step_f32(patches)
            assert np.array_equal(again["angle_ssd"], r["angle_ssd"]) and np.array_equal(again["angle_view"], r["angle_view"])
    finally:
        e_new.close()
        e_old.close()


@pytest.mark.parametrize("A,scale,noise", [(32, 1.0, 0.6), (40, 300.0, 0.5), (32, 1e-3, 0.8), (64, 5.0, 0.4), (16, 40.0, 0.5),
                                           (32, 1.0, 1e-3)])
def test_ssd_f32_selection_bound_under_cancellation(A, scale, noise):
    """The matrix-core forms only select (two-term bf16 products at 32 headings per pass, fp32 chains at up to 16): their error
    bound must keep every heading's true minimiser in the candidate list where the expansion cancels -- a library of noisy copies of
    one view on top of an offset twice its range (the norms are 10-30x the SSDs, and a planted exact copy makes one SSD zero), values
    far from 1.  With noise 1e-3 every view lies inside every heading's window (96 000 pairs > the 4096 the list holds): the step
    must then fall back to exact scores everywhere (flag 4) and still be right.  Every reported minimum is compared with the
    reference's `ssds` over ALL views (float64 NumPy finds the few pairs the oracle scores)."""
    rng = np.random.default_rng(A * 7 + int(scale))
    F, h, w = 3000, 24, 20
    base = (rng.uniform(-1, 1, (h, w)) * scale + 2 * scale).astype(np.float32)
    lib = (base[None] + (noise * scale) * rng.standard_normal((F, h, w))).astype(np.float32)
    patches = (base[None] + (noise * scale) * rng.standard_normal((A, h, w))).astype(np.float32)
    patches[3] = lib[777]                                              # an exact match among the near-duplicates
    l64 = lib.astype(np.float64)
    e = engine_with({})
    try:
        e.set_library_f32(lib)
        r = e.step_f32(patches)
        for a in range(A):
            d = l64 - patches[a].astype(np.float64)
            approx = (d * d).reshape(F, -1).sum(axis=1)
            near = np.flatnonzero(approx <= approx.min() * (1 + 1e-9) + 1e-300)
            ex = np.array([oracle.ssds(patches[a].astype(np.float64), l64[k]) for k in near])
            assert r["angle_ssd"][a] == ex.min(), (a, r["angle_ssd"][a], ex.min(), r["n_candidates"], r["flags"])
            assert int(r["angle_view"][a]) == int(near[int(np.argmin(ex))]), a
        assert r["best_idex"] == 3 and r["best_view"] == 777 and r["step_ssd"] == 0.0
        # noise 1e-3: every view lies inside every heading's window (96 000 pairs) -> the exact fallback; the others: the bound itself
        assert bool(r["flags"] & 4) == (noise < 1e-2), (r["flags"], r["n_candidates"])
        if noise > 1e-2:
            assert r["n_candidates"] < 40 * A
    finally:
        e.close()


# ------------------------------------------------------------------ the agent's next step begun before its book-keeping
def _walk(pipeline, script):
    land = synth.synth_landscape(12, 500, 4)
    path = synth.sin_training_path(0.5, 80, 330, arclen=1.0)[:260]
    nsf = navsim_amd.NavBySceneFamiliarity(land, (16, 16), 1.0, n_test_angles=12, n_sensor_levels=5,
                                           familiarity_model=navsim_amd.sads_familiarity(0.25), track_scene_familiarity=False)
    nsf.pipeline_steps = pipeline
    nsf.train_from_path(path)
    nsf.position, nsf.angle = (path[3][0] + 0.4, path[3][1] - 0.2), 0.6
    log, begun_used = [], 0
    try:
        for t in range(400):
            what = script(t)
            if what == "teleport":                                   # a pose nobody began a step for
                nsf.position, nsf.angle = (path[40][0] - 0.3, path[40][1] + 0.5), 1.1
            elif what == "engine":                                   # something else asked of the engine between two steps
                nsf._engine.library_info()
            elif what == "metrics":                                  # a metric read in mid-run (collects outstanding answers)
                log.append(("rmsd", float(nsf.navigation_error), float(nsf.percent_recapitulated)))
            elif what == "sense":
                log.append(("mat", nsf.get_sensor_mat(nsf.position, nsf.angle).tobytes()))
            had = nsf._spec is not None and nsf._engine._begun
            nsf.step_forward(fake=(what == "fake"))
            begun_used += int(had)
            log.append((nsf.last_best_idex, nsf.position, nsf.angle, nsf.angle_familiarity.tobytes(), nsf.navigated_for_frames))
    except navsim_amd.StopNavigationException as e:
        log.append(("stop", e.get_code()))
    log.append(("end", float(nsf.navigation_error), float(nsf.percent_recapitulated), nsf.percent_recapitulated_forgiving(),
                nsf.n_captures(), nsf.navigated_for_frames))
    nsf.clear_training()
    return log, begun_used


def test_pipelined_agent_steps_equal_call_per_step():
    """dv_agent_step_begin / _end: the agent begins its next step as soon as the new pose is known and ends it in the next
    step_forward().  Same decisions, poses, per-heading maxima, error metrics and stop as one call per step -- also when the pose
    is changed between steps, when other engine calls come in between (the begun step is superseded), with fake steps mixed
    in, and at the end of the path (a begun step nobody ends)."""
    def script(t):
        return {17: "teleport", 30: "engine", 31: "fake", 32: "fake", 50: "metrics", 51: "sense", 90: "teleport"}.get(t)
    piped, used = _walk(True, script)
    plain, used0 = _walk(False, script)
    assert used0 == 0 and used > len(piped) * 0.9, (used, len(piped))    # the pipelined run did end begun steps almost every time
    assert len(piped) == len(plain)
    for k, (a, b) in enumerate(zip(piped, plain)):
        assert a == b, k
    assert piped[-2][0] == "stop" or len(piped) > 400                    # (the walk reaches the end of the path)


def test_begun_agent_step_is_superseded_by_any_other_call():
    land = synth.synth_landscape(3, 300, 4)
    agent = None
    try:
        agent = navsim_amd.NavBySceneFamiliarity(land, (8, 8), 1.0, n_test_angles=6, n_sensor_levels=5,
                                                 familiarity_model=navsim_amd.sads_familiarity(0.0))
        agent.train_from_path(synth.sin_training_path(0.5, 60, 200, arclen=1.0)[:100])
        e2 = agent._engine
        fam = np.empty(6)
        offs = agent.angle_offsets
        assert e2.agent_step_end() is None                               # nothing begun
        assert e2.agent_step_begin(100.0, 130.0, 0.3, offs, fam, None, 0.0) is None
        best = e2.agent_step_end()
        want, _ = e2.agent_step(100.0, 130.0, 0.3, offs, np.empty(6), None, 0.0)
        assert best == want
        e2.agent_step_begin(100.0, 130.0, 0.3, offs, fam, None, 0.0)
        e2.library_info()
        assert e2.agent_step_end() is None                               # superseded: the caller steps again
        # end and the next begin in one call: nothing is begun for a pose the bounds test refuses; otherwise the step begun is the
        # one for the candidate of the heading chosen
        cand_angle = (0.3 + offs) % (2 * np.pi)
        bounds = np.array([4.0, 296.0, 296.0])
        e2.agent_step_begin(100.0, 130.0, 0.3, offs, fam, None, 0.0)
        got = e2.agent_step_end_begin((cand_angle, np.full(6, 1e6), np.full(6, 130.0)), bounds, False, 0.0)
        assert got == (want, False, None) and e2.agent_step_end() is None
        e2.agent_step_begin(100.0, 130.0, 0.3, offs, fam, None, 0.0)
        got = e2.agent_step_end_begin((cand_angle, np.full(6, 120.0), np.full(6, 131.0)), bounds, False, 0.0)
        assert got == (want, True, None)
        nxt = e2.agent_step_end()
        chk, _ = e2.agent_step(120.0, 131.0, cand_angle[want], offs, np.empty(6), None, 0.0)
        assert nxt == chk
        assert e2.agent_step_end_begin((cand_angle, np.full(6, 120.0), np.full(6, 131.0)), bounds, False, 0.0) is None      # nothing begun
        # the C ABI itself refuses an end with another step in between, and one without a begin
        lib = e2._lib
        best32 = ctypes.c_int32()
        e2.agent_step_begin(100.0, 130.0, 0.3, offs, fam, None, 0.0)
        e2.sense_step(100.0, 130.0, (0.3 + offs) % (2 * np.pi), want_scene=False)
        assert lib.dv_agent_step_end(e2._ctx_raw, N.f64ptr(fam), ctypes.byref(best32)) == -3
        assert lib.dv_agent_step_end(e2._ctx_raw, N.f64ptr(fam), ctypes.byref(best32)) == -3
    finally:
        if agent is not None:
            agent.clear_training()


# ------------------------------------------------------------------ passes of 64 headings: two view groups x two heading tiles per consumer
@pytest.mark.parametrize("cw", [0.25, 0.0, 1.0])
def test_passes_of_64_headings_with_shared_accumulators_match_the_oracle(cw):
    """k_sad_lc22 (ensemble passes of 64 headings on libraries of >= 1280 view-group ranges: two view groups and two heading tiles per
    consumer, the bit positions of one gap width in one accumulator, the saturation counts parked in LDS) against the oracle on EVERY
    view: agents on the library's levels (fp4 form), agents with off-level value bytes (the kernel's int8 body for the whole pass),
    exact duplicates across view groups (resolver), a short last pass -- and the records of the one-view-group body (DEJAVU_LC22=0)."""
    F, h, w, A, n_agents, seed = 41500, 16, 16, 16, 11, 77          # 11 agents x 16 headings: passes of 64, 64 and 48 headings
    lib = synth.synth_views(seed, F, h, w)
    lib[40000] = lib[123]                                            # duplicates in different ranges of view groups
    on = synth.synth_patches(seed + 3, n_agents * A, h, w).reshape(n_agents, A, h, w, 3)
    on[2, 5] = lib[123]
    on[7, 0] = synth.near_match_patch(lib[31000], 5, fraction=0.02)
    on[10, 15] = lib[41499]
    off = on.copy()
    off[..., 2] = synth.random_hsv(seed + 9, off.shape[:-1])         # value bytes between the levels: every pass takes the int8 body
    off[4, 3] = lib[777]
    got = {}
    for knob in ("1", "0"):
        eng = engine_with({"DEJAVU_LC22": knob})
        try:
            eng.set_library(lib, cw)
            for name, patches in (("on", on), ("off", off)):
                eng.step_batch(patches)                                  # (the first call times the kernel forms)
                got[knob, name] = eng.step_batch(patches)
                if knob == "1" and name == "on" and cw < 1.0 and eng.scoring_form()["matrix_cores"]:      # (a knob of the suite's A/B runs may
                    assert eng.scoring_form()["fp4"], eng.scoring_form()                                    #  have the timing pick a byte kernel here)
        finally:
            eng.close()
    for name, patches in (("on", on), ("off", off)):
        res, ref = got["1", name], got["0", name]
        for ag in range(n_agents):
            want = oracle.step(lib, patches[ag], cw, want_scene=False)
            assert res[ag]["best_idex"] == want["best_idex"], (name, ag, res[ag]["flags"], res[ag]["n_candidates"])
            assert res[ag]["best_view"] == want["best_view"], (name, ag)
            np.testing.assert_allclose(res[ag]["angle_familiarity"], want["angle_familiarity"], rtol=RTOL)
            np.testing.assert_allclose(res[ag]["step_familiarity"], want["step_familiarity"], rtol=RTOL)
            assert (ref[ag]["best_idex"], ref[ag]["best_view"]) == (res[ag]["best_idex"], res[ag]["best_view"])
            assert np.array_equal(ref[ag]["angle_familiarity"], res[ag]["angle_familiarity"])       # the same integer sums either way
    if cw < 1.0:
        assert (got["1", "on"][2]["best_idex"], got["1", "on"][2]["best_view"]) == (5, 123)      # the first of the two duplicates
    # the reference's default n_test_angles = 60 (NavBySceneFamiliarity.py:62) is ONE pass of 64 resident headings: a single agent's
    # step takes the same kernel
    eng = engine_with({})
    try:
        eng.set_library(lib, cw)
        p60 = on.reshape(-1, h, w, 3)[:60].copy()
        p60[41] = lib[40000 - 1]
        for _ in range(2):
            r = eng.step(p60, want_scene=False)
        want = oracle.step(lib, p60, cw, want_scene=False)
        assert (r["best_idex"], r["best_view"]) == (want["best_idex"], want["best_view"])
        np.testing.assert_allclose(r["angle_familiarity"], want["angle_familiarity"], rtol=RTOL)
        assert r["step_familiarity"] == pytest.approx(want["step_familiarity"], rel=RTOL)
    finally:
        eng.close()


@pytest.mark.parametrize("h,w,n_agents,A,F,cw,levels", [
    (8, 8, 4, 16, 41000, 0.25, None), (12, 20, 8, 8, 47001, 0.5, None), (32, 32, 2, 32, 41011, 0.1, None), (16, 16, 1, 64, 52000, 0.25, None),
    (16, 16, 3, 20, 41000, 0.0, None), (64, 64, 4, 16, 41000, 0.25, None),
    (16, 16, 4, 16, 41000, 0.25, (0, 50, 100, 150, 255)),               # value gaps 50, 50, 50, 105: the shared accumulator does not fit
    (16, 16, 4, 16, 41000, 0.25, (0, 100, 150, 200, 250)),              # 100, 50, 50, 50: it does (position 0 has its own)
    (16, 16, 4, 16, 41000, 0.25, (0, 85, 170, 255))])                   # three equal gaps
def test_two_group_body_equals_one_group_body(h, w, n_agents, A, F, cw, levels):
    """The records of passes of 64 headings are the same numbers whichever body scored them (DEJAVU_LC22=1 / 0): shapes, agents per
    pass, a last pixel block that is not whole, value level sets the shared accumulators fit and do not fit (lc22_fits decides)."""
    lib = synth.synth_views(5, F, h, w)
    patches = synth.synth_patches(6, n_agents * A, h, w).reshape(n_agents, A, h, w, 3)
    if levels is not None:                                           # re-map the five synthetic value levels
        lut = np.zeros(256, np.uint8)
        src = (0, 63, 127, 191, 255)
        for k, v in enumerate(src):
            lut[v] = levels[min(k, len(levels) - 1)]
        lib[..., 2] = lut[lib[..., 2]]
        patches[..., 2] = lut[patches[..., 2]]
    patches[n_agents // 2, A // 2] = lib[F - 7]
    recs = {}
    for knob in ("1", "0"):
        eng = engine_with({"DEJAVU_LC22": knob})
        try:
            eng.set_library(lib, cw)
            eng.step_batch(patches)
            r = eng.step_batch(patches)
            recs[knob] = [(x["best_idex"], x["best_view"], x["step_familiarity"], x["angle_familiarity"].tobytes(), x["angle_view"].tobytes()) for x in r]
        finally:
            eng.close()
    assert recs["1"] == recs["0"]
    assert recs["1"][n_agents // 2][:2] == (A // 2, F - 7)
    want = oracle.step(lib[F - 300:], patches[0], cw, want_scene=False)      # and a slice of the oracle for good measure
    got = engine_with({})
    try:
        got.set_library(lib[F - 300:], cw)
        r0 = got.step(patches[0], want_scene=False)
        assert r0["best_view"] == want["best_view"]
    finally:
        got.close()


@pytest.mark.parametrize("env", [{"DEJAVU_CHAIN_ORDER": "1"}, {"DEJAVU_CHAIN_ORDER": "2"}, {"DEJAVU_CHAINS": "3"}, {"DEJAVU_CHAINS": "1"},
                                 {"DEJAVU_CHAINS": "3", "DEJAVU_LC22": "0"}])
def test_ensemble_chain_knobs_leave_the_records_alone(env):
    """However the passes of an ensemble step are laid out on their streams (DEJAVU_CHAIN_ORDER, DEJAVU_CHAINS), every agent's record is
    the same -- uploaded and device-sensed patches, eight passes and a short ninth."""
    F, h, w, A, n_agents = 41000, 16, 16, 16, 34
    lib = synth.synth_views(9, F, h, w)
    patches = synth.synth_patches(10, n_agents * A, h, w).reshape(n_agents, A, h, w, 3)
    patches[33, 2] = lib[40999]
    patches[17, 9] = synth.near_match_patch(lib[12345], 4, fraction=0.02)
    recs = []
    for e in ({}, env):
        eng = engine_with(e)
        try:
            eng.set_library(lib, 0.25)
            eng.step_batch(patches)
            r = eng.step_batch(patches)
            recs.append([(x["best_idex"], x["best_view"], x["step_familiarity"], x["angle_familiarity"].tobytes()) for x in r])
        finally:
            eng.close()
    assert recs[0] == recs[1]
    assert recs[0][33][:2] == (2, 40999) and recs[0][17][:2] == (9, 12345)


def test_pipelined_agent_walks_out_of_the_landscape_like_the_plain_one():
    """The call that ends a step begins the next one only where the reference's bounds test lets it sense (dv_agent_step_end_begin): an
    agent heading for the edge stops at the same step, in the same state, as with one call per step -- fake and real steps."""
    land = synth.synth_landscape(3, 260, 4)
    path = np.stack([np.linspace(60, 200, 120), np.full(120, 130.0)], axis=1)
    logs = {}
    for pipe in (True, False):
        for fake in (True, False):
            nsf = navsim_amd.NavBySceneFamiliarity(land, (16, 16), 2.0, n_test_angles=8, n_sensor_levels=5, saccade_degrees=30.,
                                                   familiarity_model=navsim_amd.sads_familiarity(0.25), track_scene_familiarity=False)
            nsf.pipeline_steps = pipe
            nsf.train_from_path(path)
            nsf.position, nsf.angle = (150.0, 131.0), 0.02
            log = []
            try:
                for t in range(200):
                    nsf.step_forward(fake=fake)
                    log.append((nsf.last_best_idex, nsf.position, nsf.angle, nsf.navigated_for_frames))
            except (navsim_amd.StopNavigationException, IndexError) as e:      # (the rotated sensor's corners reach past the bounds test: the
                log.append(("stop", type(e).__name__, nsf.position, nsf.navigated_for_frames))      #  reference's trial may end in an IndexError first)
            if not fake:
                log.append(("rmsd", float(nsf.navigation_error), nsf.percent_recapitulated_forgiving()))
            logs[pipe, fake] = log
            nsf.clear_training()
    for fake in (True, False):
        assert logs[True, fake] == logs[False, fake], fake
    assert logs[True, True][-1][0] == "stop" and logs[True, True][-1][1] in ("OutOfLandscapeBoundsException", "IndexError")


@pytest.mark.parametrize("max_dist", [np.inf, 3.0])
def test_ensemble_metrics_on_the_device_equal_the_host_arithmetic(max_dist):
    """update_error (NavBySceneFamiliarity.py:252-276) of all members of an ensemble in one device call per step (dv_path_error_batch,
    a coverage array per member): RMSD, coverage, forgiving coverage, captures, frames and stop codes equal those of the same agents
    stepping one by one with the reference's NumPy arithmetic -- also where members stop for being too far from the path."""
    land = synth.synth_landscape(21, 500, 4)
    path = synth.sin_training_path(0.5, 80, 330, arclen=1.0)[:300]
    def trained():
        nsf = navsim_amd.NavBySceneFamiliarity(land, (16, 16), 1.0, n_test_angles=8, n_sensor_levels=5, max_distance_to_training_path=max_dist,
                                               familiarity_model=navsim_amd.sads_familiarity(0.25), track_scene_familiarity=False)
        nsf.train_from_path(path)
        return nsf
    rng = np.random.default_rng(8)
    poses = []
    for i in (3, 40, 90, 150, 220, 280):
        d = path[i + 1] - path[i]
        poses.append((path[i] + rng.uniform(-1.5, 1.5, 2), float((np.arctan2(d[1], d[0]) + rng.uniform(-0.3, 0.3)) % (2 * np.pi))))
    ens = navsim_amd.NavEnsemble.from_agent(trained(), poses)
    assert all(a._metric_slot == j for j, a in enumerate(ens.agents))
    done = ens.run(260)
    rows = []
    for j, a in enumerate(ens.agents):
        rows.append((done[j], ens.stop_status[j], a.navigated_for_frames, float(a.navigation_error) if a._n_navigation_error else None,
                     float(a.percent_recapitulated), a.percent_recapitulated_forgiving(), a.n_captures(), a.position, a.angle))
    ens.engine.close()
    # the same agents one by one, metrics on the host (the reference's NumPy expression)
    want = []
    for pos, ang in poses:
        nsf = trained()
        nsf._metrics_on_device = False
        nsf.pipeline_steps = False
        nsf.reset_error()
        nsf.position, nsf.angle = (float(pos[0]), float(pos[1])), float(ang)
        steps, code = 0, 0
        try:
            for _ in range(260):
                nsf.step_forward()
                steps += 1
        except navsim_amd.StopNavigationException as e:
            code = e.get_code()
        except IndexError:
            code = navsim_amd.NavEnsemble.SENSE_ERROR_STATUS
        want.append((steps, code, nsf.navigated_for_frames, float(nsf.navigation_error) if nsf._n_navigation_error else None,
                     float(nsf.percent_recapitulated), nsf.percent_recapitulated_forgiving(), nsf.n_captures(), nsf.position, nsf.angle))
        nsf._engine.close()
    assert rows == want
    if np.isfinite(max_dist):
        assert any(r[1] == navsim_amd.TooFarFromTrainingPathException().get_code() for r in rows)


def test_scene_familiarity_worked_out_when_read_equals_the_one_kept_every_step():
    """track_scene_familiarity=True (the reference's default): the agent takes its lean device step and works the per-view minimum of
    the last step out when scene_familiarity is read (lazy_scene) -- the array the eager agent keeps every step, bit for bit, at any
    step it is read, also right after the step that ends the run; in between, the two walk the same trajectory."""
    land = synth.synth_landscape(12, 500, 4)
    path = synth.sin_training_path(0.5, 80, 330, arclen=1.0)[:200]
    agents = []
    for lazy in (True, False):
        nsf = navsim_amd.NavBySceneFamiliarity(land, (16, 16), 1.0, n_test_angles=12, n_sensor_levels=5, familiarity_model=navsim_amd.sads_familiarity(0.25))
        nsf.lazy_scene = lazy
        nsf.train_from_path(path)
        nsf.position, nsf.angle = (path[3][0] + 0.4, path[3][1] - 0.2), 0.6
        agents.append(nsf)
    lazy_a, eager_a = agents
    assert lazy_a.track_scene_familiarity and np.array_equal(lazy_a.scene_familiarity, eager_a.scene_familiarity)      # zeros after training (:134)
    stopped = [None, None]
    reads = 0
    for t in range(400):
        for k, a in enumerate(agents):
            try:
                a.step_forward()
            except navsim_amd.StopNavigationException as e:
                stopped[k] = type(e).__name__
        assert lazy_a.position == eager_a.position and lazy_a.angle == eager_a.angle and stopped[0] == stopped[1], t
        if t % 7 == 3 or stopped[0]:
            reads += 1
            assert lazy_a._scene_stale is not None
            assert lazy_a.scene_familiarity.tobytes() == eager_a.scene_familiarity.tobytes(), t
            assert lazy_a._scene_stale is None and lazy_a.scene_familiarity is lazy_a.scene_familiarity
        if stopped[0]:
            break
    assert reads > 10
    # ... and right after the step that ends a run: both agents set down just before the end of the path
    d = path[-5] - path[-6]
    for a in agents:
        a.stopped_with_exception = None
        a.position, a.angle = (float(path[-6][0]), float(path[-6][1])), float(np.arctan2(d[1], d[0]) % (2 * np.pi))
    ended = [None, None]
    for t in range(40):
        for k, a in enumerate(agents):
            if ended[k] is None:
                try:
                    a.step_forward()
                except navsim_amd.StopNavigationException as e:
                    ended[k] = type(e).__name__
        if ended[0] or ended[1]:
            break
    assert ended[0] == ended[1] == "ReachedEndOfTrainingPathException"
    assert lazy_a._scene_stale is not None and lazy_a.scene_familiarity.tobytes() == eager_a.scene_familiarity.tobytes()
    for a in agents:
        a.clear_training()


@pytest.mark.parametrize("max_dist,start", [(2.5, (0.5, 1.8)), (3.0, (1.0, -2.0)), (6.0, (2.0, 3.0)), (450.0, (1.0, -1.0))])
def test_deferred_error_metrics_with_a_finite_max_distance_stop_in_the_very_step(max_dist, start):
    """With a finite max_distance_to_training_path the reference stops the run inside the step that gets too far (:264).  The lean agent
    collects a position's distance one step late only while the triangle inequality says that cannot happen, and waits for it at once
    otherwise: the step, exception and state at the stop -- and every metric -- equal those of an agent with the metrics in NumPy."""
    land = synth.synth_landscape(31, 500, 4)
    path = synth.sin_training_path(0.5, 80, 330, arclen=1.0)[:220]
    out = []
    deferred = 0
    for device in (True, False):
        nsf = navsim_amd.NavBySceneFamiliarity(land, (16, 16), 1.0, n_test_angles=8, n_sensor_levels=5, max_distance_to_training_path=max_dist,
                                               familiarity_model=navsim_amd.sads_familiarity(0.25), track_scene_familiarity=False)
        nsf.train_from_path(path)
        if not device:
            nsf._metrics_on_device = False
            nsf.pipeline_steps = False
            nsf.reset_error()
        nsf.position, nsf.angle = (path[5][0] + start[0], path[5][1] + start[1]), 0.9
        log = []
        try:
            for t in range(400):
                nsf.step_forward()
                if device:
                    deferred += int(nsf._pending_errors > 0)
                log.append((nsf.last_best_idex, nsf.position, nsf.angle))
        except navsim_amd.StopNavigationException as e:
            log.append(("stop", type(e).__name__, nsf.position, nsf.angle, nsf.navigated_for_frames))
        log.append((nsf.navigated_for_frames, float(nsf.navigation_error) if nsf._n_navigation_error else None, float(nsf.percent_recapitulated),
                    nsf.percent_recapitulated_forgiving(), nsf.n_captures()))
        out.append(log)
        nsf.clear_training()
    assert out[0] == out[1]
    if max_dist >= 6.0:
        assert deferred > 50                                            # far from the limit the answers did come a step late
    if max_dist <= 3.0:
        assert out[0][-2][0] == "stop"
