"""GPU tests of per-agent scene_familiarity in batched passes: dv_sense_step_batch_scene / dv_step_batch_scene and the ensembles of
reference-default agents (track_scene_familiarity=True) built on them.

Every comparison is bit for bit against the single-agent step with scene_fam on the same engine (which the suite holds to the
reference elsewhere), except where the oracle is named: there the project's contract for scores applies (1e-12 relative from the
integer sums, equal in exact mode)."""
import numpy as np
import pytest

import navsim_amd
from navsim_amd import synth
from oracle import oracle
from tests.helpers import ENGINE_MODES, engine_mode, sha
from tests.test_gpu_parity import SHAPES, make_inputs
from tests.test_host_logic import _run_trajectory

pytestmark = pytest.mark.gpu

KEYS = ("best_heading", "best_view", "best_fam", "flags", "n_candidates", "n_headings", "angle_fam", "angle_view")


def rec(r, i):
    return tuple(np.asarray(r.records[i][k]).tobytes() for k in KEYS)


@pytest.fixture(scope="module", params=ENGINE_MODES)
def eng(request):
    """Every test runs under each form of the scoring path (tests/helpers.py:ENGINE_MODES): both step endings, the
    bit-plane matrix-core kernel, and the product default."""
    e = engine_mode(request.param)
    e.mode = request.param
    yield e
    e.close()


def _attach_sensor(e, land, dims):
    host = navsim_amd.NavBySceneFamiliarity(land, dims, 1.0, n_test_angles=4, n_sensor_levels=5, use_gpu_sensor=False,
                                            familiarity_model=oracle.sads_familiarity())
    e.set_landscape(land)
    e.configure_sensor(host.sensor_dimensions, host.sensor_pixel_dimensions, host._level_tables(), host.mask_middle_n)


# ------------------------------------------------------------------ 1. sensed form: rows and records
@pytest.mark.parametrize("exact", [False, True])
def test_sensed_rows_equal_the_single_agent_step(eng, exact):
    """1, 3, 4, 5 and 9 agents x 8, 16, 60 and 64 headings (60: one agent per pass; 5 x 16: a partly filled last pass): every row is
    dv_sense_step's scene_fam of that pose, the records are dv_sense_step_batch's."""
    land = synth.synth_landscape(11, 420, 4)
    path = synth.sin_training_path(0.5, 0.2 * 420, 0.6 * 420, arclen=1.0)[:300]
    _attach_sensor(eng, land, (16, 12))
    d = path[1:] - path[:-1]
    head = np.arctan2(d[:, 1], d[:, 0])
    head = np.append(head, head[-1])
    eng.set_library_from_poses(path[:, 0], path[:, 1], head, 0.25)            # 300 views: not a multiple of 64
    eng.set_exact(exact)
    rng = np.random.default_rng(5)
    try:
        for A in (8, 16, 60, 64):
            for n in (1, 3, 4, 5, 9):
                k = rng.integers(3, len(path) - 3, n)
                xs, ys = path[k, 0] + rng.uniform(-0.7, 0.7, n), path[k, 1] + rng.uniform(-0.7, 0.7, n)
                angs = (head[k][:, None] + rng.uniform(-0.3, 0.3, (n, 1)) + np.linspace(-1.0, 1.0, A)[None, :]) % (2 * np.pi)
                got = eng.sense_step_batch_scene(xs, ys, angs)
                plain = eng.sense_step_batch(xs, ys, angs)
                assert got.scene_familiarity.shape == (n, 300) and got.scene_familiarity.dtype == np.float64
                for i in range(n):
                    one = eng.sense_step(xs[i], ys[i], angs[i], want_scene=True)
                    assert got.scene_familiarity[i].tobytes() == one["scene_familiarity"].tobytes(), (eng.mode, A, n, i)
                    assert rec(got, i) == rec(plain, i), (eng.mode, A, n, i)
                    assert got[i]["best_idex"] == one["best_idex"] and got[i]["best_view"] == one["best_view"]
                    assert got[i]["angle_familiarity"].tobytes() == one["angle_familiarity"].tobytes()
    finally:
        eng.set_exact(False)


# ------------------------------------------------------------------ 2. patch form on every layout
@pytest.mark.parametrize("F,h,w,A,cw,kind", SHAPES)
def test_patch_form_rows_on_every_layout(eng, F, h, w, A, cw, kind):
    """The shapes and layouts of test_ragged_shapes_against_oracle (five levels, mixed, three hues, signed, many hues, no saturation,
    F below 64 and not a multiple of 64) with five agents per call: every row is dv_step's scene_fam of that agent's patches, in
    both the integer and the exact mode, and within the contract of the oracle's."""
    n = 5
    lib, _ = make_inputs(F, h, w, A, kind, seed=F * 131 + A)
    patches = np.stack([make_inputs(F, h, w, A, kind, seed=F * 131 + A + 1000 * (i + 1))[1] for i in range(n)])
    patches[1, A // 2] = lib[F // 2]                                          # an agent that sees a stored view
    eng.set_library(lib, cw)
    try:
        for exact in (False, True):
            eng.set_exact(exact)
            got = eng.step_batch_scene(patches)
            plain = eng.step_batch(patches)
            assert got.scene_familiarity.shape == (n, F)
            for i in range(n):
                one = eng.step(patches[i], want_scene=True)
                assert got.scene_familiarity[i].tobytes() == one["scene_familiarity"].tobytes(), (eng.mode, kind, exact, i)
                assert rec(got, i) == rec(plain, i), (eng.mode, kind, exact, i)
                want = oracle.step(lib, patches[i], cw)
                assert got[i]["best_idex"] == want["best_idex"] and got[i]["best_view"] == want["best_view"]
                if exact:
                    assert got.scene_familiarity[i].tobytes() == want["scene_familiarity"].tobytes()
                else:
                    # (atol: the contract as test_ragged_shapes_against_oracle states it for these shapes, where a score may be 0)
                    np.testing.assert_allclose(got.scene_familiarity[i], want["scene_familiarity"], rtol=1e-12, atol=1e-12)
    finally:
        eng.set_exact(False)


def test_rows_on_a_library_the_matrix_cores_stream(eng):
    """41 500 views of 16x16 (the sizes at which the shipped engine ends its steps in k_finish and scores on the matrix cores), 9
    agents x 16 headings: passes of 64, 64 and 16 headings."""
    F, h, w, A, n, seed = 41500, 16, 16, 16, 9, 77
    lib = synth.synth_views(seed, F, h, w)
    patches = synth.synth_patches(seed + 3, n * A, h, w).reshape(n, A, h, w, 3)
    patches[2, 5] = lib[123]
    patches[8, A - 1] = lib[F - 1]
    patches[4, ..., 2] = synth.random_hsv(seed + 9, patches[4].shape[:-1])    # value bytes between the levels: the int8 body
    eng.set_library(lib, 0.25)
    eng.step_batch_scene(patches)                                             # (the first call times the kernel forms)
    got = eng.step_batch_scene(patches)
    plain = eng.step_batch(patches)
    for i in range(n):
        one = eng.step(patches[i], want_scene=True)
        assert got.scene_familiarity[i].tobytes() == one["scene_familiarity"].tobytes(), (eng.mode, i)
        assert rec(got, i) == rec(plain, i), (eng.mode, i)
    assert got.scene_familiarity[2, 123] <= 256.0 and got[2]["best_view"] == 123


# ------------------------------------------------------------------ 3. weighted members
@pytest.mark.parametrize("F", [3001, 41500])
def test_weighted_rows_equal_a_library_of_that_weight(eng, F):
    """chem_weights 0, 0.25, 0.5 and 1 in one call on a library laid out by set_weight_range: row i is the single-agent scene_fam of an
    engine whose library was ingested at weight w_i, and the oracle's per-view minimum at w_i within the contract for scores."""
    h, w, A, n, seed = 16, 16, 16, 8, 91
    lib = synth.synth_views(seed, F, h, w)
    patches = synth.synth_patches(seed + 3, n * A, h, w).reshape(n, A, h, w, 3)
    patches[3, 7] = lib[F // 3]
    patches[6, ..., 2] = synth.random_hsv(seed + 9, patches[6].shape[:-1])
    weights = [(0.0, 0.25, 0.5, 1.0)[i % 4] for i in range(n)]
    single = engine_mode(eng.mode)
    try:
        eng.set_weight_range(0.0, 1.0)
        eng.set_library(lib, 0.25)
        eng.set_weight_range(1.0, 0.0)
        for exact in (False, True):
            eng.set_exact(exact)
            single.set_exact(exact)
            got = eng.step_batch_scene(patches, chem_weights=weights)
            plain = eng.step_batch(patches, chem_weights=weights)
            for cw in sorted(set(weights)):
                single.set_library(lib, cw)
                for i in range(n):
                    if weights[i] != cw:
                        continue
                    one = single.step(patches[i], want_scene=True)
                    assert got.scene_familiarity[i].tobytes() == one["scene_familiarity"].tobytes(), (eng.mode, exact, i, cw)
                    assert rec(got, i) == rec(plain, i), (eng.mode, exact, i, cw)
                    if F <= 5000:
                        want = oracle.step(lib, patches[i], cw, want_scene=True)["scene_familiarity"]
                        if exact:
                            assert got.scene_familiarity[i].tobytes() == want.tobytes(), (eng.mode, i, cw)
                        else:
                            np.testing.assert_allclose(got.scene_familiarity[i], want, rtol=1e-12, atol=0)
    finally:
        eng.set_exact(False)
        single.close()


# ------------------------------------------------------------------ 4. an agent whose footprint leaves the landscape
def test_an_agent_off_the_landscape_gets_a_row_of_inf(eng):
    land = synth.synth_landscape(3, 120, 4)
    path = np.stack([np.linspace(40, 80, 70), np.full(70, 60.0)], axis=1)
    _attach_sensor(eng, land, (40, 40))
    eng.set_library_from_poses(path[:, 0], path[:, 1], np.zeros(70), 0.25)
    offs = np.linspace(-0.5, 0.5, 4)
    poses = [((60.0, 60.0), 0.0), ((99.4, 99.4), 0.8 + np.pi / 2), ((50.0, 61.0), 0.2), ((70.0, 58.0), 6.0)]
    xs, ys = [p[0][0] for p in poses], [p[0][1] for p in poses]
    angs = np.stack([(p[1] + offs) % (2 * np.pi) for p in poses])
    with pytest.raises(IndexError):
        eng.sense_step(xs[1], ys[1], angs[1], want_scene=True)
    got = eng.sense_step_batch_scene(xs, ys, angs)
    keep = [0, 2, 3]
    without = eng.sense_step_batch_scene([xs[i] for i in keep], [ys[i] for i in keep], angs[keep])
    assert got[1]["flags"] & 16 and np.isposinf(got.scene_familiarity[1]).all()
    for j, i in enumerate(keep):
        assert not got[i]["flags"] & 16
        assert np.isfinite(got.scene_familiarity[i]).all()
        assert got.scene_familiarity[i].tobytes() == without.scene_familiarity[j].tobytes(), i
        assert rec(got, i) == rec(without, j), i


def test_argument_errors_follow_the_weighted_batch(eng):
    lib = synth.synth_views(3, 500, 8, 8)
    patches = synth.synth_patches(4, 3 * 8, 8, 8).reshape(3, 8, 8, 8, 3)
    eng.set_library(lib, 0.0)
    with pytest.raises(ValueError, match="agent 1: chem_weight .* outside"):
        eng.step_batch_scene(patches, chem_weights=[0.0, 1.5, 0.0])
    with pytest.raises(navsim_amd.EngineError, match="agent 2: .*hue/saturation"):
        eng.step_batch_scene(patches, chem_weights=[0.0, 0.0, 0.5])
    with pytest.raises(ValueError, match="chem_weights"):
        eng.step_batch_scene(patches, chem_weights=[0.0, 0.0])
    got = eng.step_batch_scene(patches)                                       # and the library still serves the call
    assert got.scene_familiarity[0].tobytes() == eng.step(patches[0], want_scene=True)["scene_familiarity"].tobytes()


# ------------------------------------------------------------------ 5. ensembles of reference-default agents
class Recording(object):
    """The engine with every call made through it noted (name, arguments as bytes)."""

    def __init__(self, engine):
        self._engine, self.calls = engine, []

    def __getattr__(self, name):
        target = getattr(self._engine, name)
        if not callable(target):
            return target

        def call(*args, **kwargs):
            self.calls.append((name, tuple(np.asarray(a).tobytes() for a in args), tuple((k, np.asarray(v).tobytes()) for k, v in sorted(kwargs.items()))))
            return target(*args, **kwargs)
        return call


def test_default_agents_walk_a_golden_trajectory_as_an_ensemble(manifest, golden):
    """Agents as the constructor makes them (track_scene_familiarity left at its default), NavEnsemble.from_agent, 50 steps of the
    golden trajectory traj_cw: after steps 1, 10 and 50 every member's scene_familiarity is that of the same agent stepped alone
    from the same start, NavEnsemble.scene_familiarity()[i] is that array, member 0 is on the reference's trajectory; with nobody
    reading the attribute the engine sees the calls of an ensemble that tracks nothing; the result rows are the same either way."""
    z = golden("t4_trajectory.npz")
    case = {c["name"]: c for c in manifest["t4_trajectory"]}["traj_cw"]
    land = synth.synth_landscape(case["landscape"]["seed"], case["landscape"]["size"], case["landscape"]["grain"])
    assert sha(land) == case["landscape"]["sha"]
    zero = dict(case, n_steps=0)
    model = lambda: navsim_amd.sads_familiarity(case["chem_weight"])           # noqa: E731

    def trained(**kw):
        return _run_trajectory(zero, land, model(), **kw)[0]

    first = trained()
    assert first.track_scene_familiarity
    path = first.training_path
    start = ((first.position[0], first.position[1]), first.angle)
    poses = [start, start] + [((path[k][0] + 0.5, path[k][1] + 0.25 * j), first.angle + 0.1 * j) for j, k in enumerate((30, 90, 150))]
    ens = navsim_amd.NavEnsemble.from_agent(first, poses)
    assert all(a.track_scene_familiarity for a in ens.agents)
    ens.engine = Recording(ens.engine)
    plain = navsim_amd.NavEnsemble.from_agent(trained(track_scene_familiarity=False), poses)
    plain.engine = Recording(plain.engine)
    alone = []
    for pos, ang in poses:
        a = trained()
        a.position, a.angle = pos, ang
        alone.append(a)
    name = case["name"]
    try:
        assert not ens.scene_familiarity().any()                              # zeros, as after train_from_path
        for t in range(50):
            ens.step_forward()
            plain.step_forward()
            for a in alone:
                a.step_forward()
            assert ens.agents[0].last_best_idex == z[name + "_best"][t]
            assert np.array(ens.agents[1].position).tobytes() == z[name + "_pos"][t].tobytes(), t
            if t + 1 in (1, 10, 50):
                assert ens.engine.calls == plain.engine.calls                 # the step itself: exactly the calls of today
                assert {c[0] for c in ens.engine.calls} <= {"sense_step_batch", "path_error_batch"}
                n_calls = len(ens.engine.calls)
                rows = ens.scene_familiarity()
                assert [c[0] for c in ens.engine.calls[n_calls:]] == ["sense_step_batch_scene"]
                assert rows.shape == (len(poses), len(path))
                for i, (m, a) in enumerate(zip(ens.agents, alone)):
                    assert m.position == a.position and m.angle == a.angle, (t, i)
                    want = a.scene_familiarity
                    assert m.scene_familiarity.tobytes() == want.tobytes(), (t, i)
                    assert rows[i].tobytes() == want.tobytes(), (t, i)
                assert ens.scene_familiarity().tobytes() == rows.tobytes() and len(ens.engine.calls) == n_calls + 1
                del ens.engine.calls[n_calls:]
        np.testing.assert_allclose(ens.agents[0].scene_familiarity, alone[0].scene_familiarity, rtol=0)
        rows_t = navsim_amd.run_ensemble(ens, frames=30)
        rows_p = navsim_amd.run_ensemble(plain, frames=30)
        assert rows_t == rows_p and ens.stop_status == plain.stop_status
        assert [a.position for a in ens.agents] == [a.position for a in plain.agents]
    finally:
        for a in alone + [first, plain.agents[0]]:
            a._engine.close()


def test_weighted_members_read_their_rows(manifest):
    """Members under chem_weights of their own (from_agent(chem_weights=...)): each row is the scene_familiarity of an agent trained
    for that weight and stepped alone."""
    case = {c["name"]: c for c in manifest["t4_trajectory"]}["traj_c0"]
    land = synth.synth_landscape(case["landscape"]["seed"], case["landscape"]["size"], case["landscape"]["grain"])
    zero = dict(case, n_steps=0)
    weights = [0.0, 0.5, 1.0]
    first = _run_trajectory(zero, land, navsim_amd.sads_familiarity(0.0))[0]
    start = ((first.position[0], first.position[1]), first.angle)
    ens = navsim_amd.NavEnsemble.from_agent(first, [start] * 3, chem_weights=weights)
    alone = [_run_trajectory(zero, land, navsim_amd.sads_familiarity(w))[0] for w in weights]
    try:
        for t in range(12):
            ens.step_forward()
            for a in alone:
                a.step_forward()
        rows = ens.scene_familiarity()
        for i, a in enumerate(alone):
            assert ens.agents[i].position == a.position, i
            assert rows[i].tobytes() == a.scene_familiarity.tobytes(), i
    finally:
        for a in alone + [first]:
            a._engine.close()


# ------------------------------------------------------------------ 6. one agent's candidate list overflows
def test_an_overflowing_agent_leaves_its_neighbours_rows_alone(eng):
    """A library of 1000 near-identical views: agent 1's eight equal patches tie on every view (8000 candidates, more than a
    candidate list holds), so its pass is redone with exact scores.  Its row is then the exact one, as for a step of its own; agents
    0 and 2 of the same pass keep the rows of the integer pass, bit for bit what each gets alone."""
    base = synth.synth_views(3, 1, 8, 8)[0]
    lib = np.repeat(base[None], 1000, axis=0)
    lib[500, 2, 2, 2] ^= 0x40
    ties = np.repeat(base[None], 8, axis=0)
    ties[:, 0, 0, 2] ^= 0x80
    patches = np.stack([synth.synth_patches(21, 8, 8, 8), ties, synth.synth_patches(22, 8, 8, 8)])
    for k in range(8):                                                        # distinct maxima per heading: one heading's ties only
        patches[0, k, k, 0, 2] ^= 0xFF
        patches[2, k, 0, k, 2] ^= 0xFF
    for cw in (0.0, 0.5):
        eng.set_library(lib, cw)
        got = eng.step_batch_scene(patches)
        plain = eng.step_batch(patches)
        assert got[1]["flags"] & 4 and got[1]["n_candidates"] > 4096, got[1]["flags"]
        for i in range(3):
            one = eng.step(patches[i], want_scene=True)
            assert bool(one["flags"] & 4) == (i == 1), (eng.mode, cw, i, one["flags"], one["n_candidates"])
            assert bool(got[i]["flags"] & 4) == (i == 1), (eng.mode, cw, i, got[i]["flags"])
            assert got.scene_familiarity[i].tobytes() == one["scene_familiarity"].tobytes(), (eng.mode, cw, i)
            assert got[i]["best_idex"] == one["best_idex"] and got[i]["best_view"] == one["best_view"], (eng.mode, cw, i)
            assert got[i]["best_idex"] == plain[i]["best_idex"] and got[i]["best_view"] == plain[i]["best_view"], (eng.mode, cw, i)
        assert got.scene_familiarity[1].tobytes() == oracle.step(lib, patches[1], cw)["scene_familiarity"].tobytes()


# ------------------------------------------------------------------ 7. argument errors of the sensed form, other metrics
def test_argument_errors_of_the_sensed_form_and_other_metrics(eng):
    from navsim_amd import _native as N
    land = synth.synth_landscape(3, 120, 4)
    path = np.stack([np.linspace(40, 80, 70), np.full(70, 60.0)], axis=1)
    _attach_sensor(eng, land, (8, 8))
    eng.set_library_from_poses(path[:, 0], path[:, 1], np.zeros(70), 0.0)     # cw 0 alone: no saturation planes
    xs, ys = [50.0, 60.0, 70.0], [60.0, 60.5, 59.5]
    angs = np.stack([np.linspace(-0.5, 0.5, 4) % (2 * np.pi)] * 3)
    with pytest.raises(ValueError, match="agent 1: chem_weight .* outside"):  # DV_ERR_INVALID
        eng.sense_step_batch_scene(xs, ys, angs, chem_weights=[0.0, -0.1, 0.0])
    with pytest.raises(navsim_amd.EngineError, match="agent 2: .*hue/saturation"):      # DV_ERR_STATE
        eng.sense_step_batch_scene(xs, ys, angs, chem_weights=[0.0, 0.0, 0.5])
    with pytest.raises(ValueError, match="chem_weights"):
        eng.sense_step_batch_scene(xs, ys, angs, chem_weights=[0.0, 0.0])
    with pytest.raises(ValueError, match="angles"):
        eng.sense_step_batch_scene(xs, ys, angs[:2])
    x, y = np.array(xs), np.array(ys)
    res = (N.StepResult * 3)()
    scene = np.empty((3, 70))
    args = (eng._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angs), 3, 4, None, 0)
    assert eng._lib.dv_sense_step_batch_scene(*args, res, None) == -1         # scene_fam is not optional
    assert eng._lib.dv_sense_step_batch_scene(*args, None, N.f64ptr(scene)) == -1
    assert eng._lib.dv_sense_step_batch_scene(*args[:4], 0, 4, None, 0, res, N.f64ptr(scene)) == -1
    assert eng._lib.dv_sense_step_batch_scene(*args[:5], 65, None, 0, res, N.f64ptr(scene)) == -1
    got = eng.sense_step_batch_scene(xs, ys, angs, chem_weights=[0.0, 0.0, 0.0])          # the weight it was laid out for is served
    for i in range(3):
        assert got.scene_familiarity[i].tobytes() == eng.sense_step(xs[i], ys[i], angs[i], want_scene=True)["scene_familiarity"].tobytes()
    # an SSD library: both forms refuse (DV_ERR_STATE), as the header says
    views = np.random.default_rng(4).integers(0, 256, (70, 8, 8), dtype=np.uint8)
    eng.set_library_u8(views)
    try:
        assert eng._lib.dv_sense_step_batch_scene(*args, res, N.f64ptr(scene)) == -3
        patches = np.zeros((3, 4, 8, 8, 3), dtype=np.uint8)
        assert eng._lib.dv_step_batch_scene(eng._ctx, N.u8ptr(patches), 3, 4, None, 0, res, N.f64ptr(scene)) == -3
    finally:
        eng.clear_library()
