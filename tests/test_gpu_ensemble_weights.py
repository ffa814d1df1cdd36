"""GPU tests of per-agent chem_weight: dv_step_batch_weighted / dv_sense_step_batch_weighted, dv_set_weight_range and
NavEnsemble.from_agent(chem_weights=...).

The reference runs chem_weight as a variable of its experiment grid (scripts/run_experiment.py:61,218); a trial's training views
do not depend on it, so one library laid out for a range of weights serves every member of an ensemble under its own weight."""

import numpy as np
import pytest

import navsim_amd
from navsim_amd import synth
from oracle import oracle
from tests.helpers import engine_with, sha
from tests.test_host_logic import _run_trajectory

pytestmark = pytest.mark.gpu

RTOL = 1e-9
WEIGHTS = (0.0, 0.25, 0.3, 0.5, 1.0)


# ------------------------------------------------------------------ 1. the reference's trajectories of two weights from ONE ensemble
def test_two_weights_in_one_ensemble_follow_the_reference_trajectories(manifest, golden):
    """traj_c0 (chem_weight 0) and traj_cw (0.5) share landscape, path, sensor and start: one agent trained for cw 0, one ensemble of
    two members under [0.0, 0.5], 1000 steps -- each member is its fixture's trajectory, bit for bit, with the fixture's metrics."""
    z = golden("t4_trajectory.npz")
    cases = {c["name"]: c for c in manifest["t4_trajectory"]}
    c0, cw = cases["traj_c0"], cases["traj_cw"]
    for k in ("landscape", "path_sha", "n_views", "sensor_dimensions", "start_offset", "start_angle_offset_deg", "n_test_angles"):
        assert c0[k] == cw[k], k
    land = synth.synth_landscape(c0["landscape"]["seed"], c0["landscape"]["size"], c0["landscape"]["grain"])
    assert sha(land) == c0["landscape"]["sha"]
    zero = dict(c0, n_steps=0)                                       # trained and placed at the fixture's start, no step taken
    nsf = _run_trajectory(zero, land, navsim_amd.sads_familiarity(0.0), track_scene_familiarity=False)[0]
    assert nsf.familiarity_model.chem_weight == 0.0
    assert nsf._engine.library_info()["weight_range"] == (0.0, 0.0)       # ingested for cw 0 alone: from_agent lays it out again
    start = ((nsf.position[0], nsf.position[1]), nsf.angle)
    ens = navsim_amd.NavEnsemble.from_agent(nsf, [start, start], chem_weights=[0.0, 0.5])
    try:
        assert [a.chem_weight for a in ens.agents] == [0.0, 0.5]
        assert ens.engine.library_info()["weight_range"] == (0.0, 1.0)
        rec = [([], [], [], []) for _ in ens.agents]
        for _ in range(c0["n_steps"]):
            ens.step_forward()
            for a, (best, pos, ang, fam) in zip(ens.agents, rec):
                best.append(a.last_best_idex)
                pos.append([a.position[0], a.position[1]])
                ang.append(a.angle)
                fam.append(a.step_familiarity)
        for a, case, (best, pos, ang, fam) in zip(ens.agents, (c0, cw), rec):
            name = case["name"]
            assert case["stop_status"] == 0 and ens.stop_status == [0, 0]
            assert np.array_equal(np.array(best), z[name + "_best"]), name
            assert np.array(pos).tobytes() == z[name + "_pos"].tobytes(), name
            assert np.array(ang).tobytes() == z[name + "_angle"].tobytes(), name
            np.testing.assert_allclose(fam, z[name + "_fam"], rtol=RTOL, atol=0, err_msg=name)
            assert a.navigated_for_frames == case["navigated_for_frames"], name
            assert float(a.navigation_error) == case["navigation_error"], name
            assert float(a.percent_recapitulated) == case["percent_recapitulated"], name
            assert float(a.percent_recapitulated_forgiving(0.05)) == case["percent_forgiving"], name
            assert int(a.n_captures(0.05)) == case["n_captures"], name
        # the foreign-weight member refuses a step of its own (it would score under the library's weight)
        with pytest.raises(ValueError, match="chem_weight"):
            ens.agents[1].step_forward()
    finally:
        ens.engine.close()


# ------------------------------------------------------------------ 2. every scoring form against the oracle, per agent
MODES = {
    "default": ({}, False, False),
    "lc22=0": ({"DEJAVU_LC22": "0"}, False, False),
    "fuse=0": ({"DEJAVU_FUSE": "0"}, False, False),
    "fp4=0": ({"DEJAVU_FP4": "0"}, False, False),
    "exact": ({}, True, False),
    "force_resolve": ({}, False, True),
}


def _batch_inputs(seed, F, h, w, n_agents, A, lib):
    on = synth.synth_patches(seed + 3, n_agents * A, h, w).reshape(n_agents, A, h, w, 3)
    on[2, 5] = lib[123]                                              # a planted exact match
    on[7, 0] = synth.near_match_patch(lib[min(31000, F - 1)], 5, fraction=0.02)
    on[10, A - 1] = lib[F - 1]
    off = on.copy()
    off[..., 2] = synth.random_hsv(seed + 9, off.shape[:-1])         # value bytes between the levels: the int8 body
    off[4, 3] = lib[777]
    return (("on", on), ("off", off))


def _check_weighted(lib, cases, weights, modes, lib_cw=0.25, info_check=None):
    want = {name: [oracle.step(lib, p[ag], weights[ag], want_scene=False) for ag in range(len(p))] for name, p in cases}
    for mode in modes:
        env, exact, force = MODES[mode]
        eng = engine_with(env)
        try:
            eng.set_weight_range(0.0, 1.0)
            eng.set_library(lib, lib_cw)
            info = eng.library_info()
            assert info["weight_range"] == (0.0, 1.0) and info["chem_weight"] == lib_cw
            if info_check:
                info_check(info)
            eng.set_exact(exact)
            for name, patches in cases:
                eng.step_batch(patches, force_resolve=force, chem_weights=weights)     # (the first call times the kernel forms)
                res = eng.step_batch(patches, force_resolve=force, chem_weights=weights)
                for ag in range(len(patches)):
                    wnt = want[name][ag]
                    msg = (mode, name, ag, weights[ag], res[ag]["flags"], res[ag]["n_candidates"])
                    assert res[ag]["best_idex"] == wnt["best_idex"], msg
                    assert res[ag]["best_view"] == wnt["best_view"], msg
                    np.testing.assert_allclose(res[ag]["angle_familiarity"], wnt["angle_familiarity"], rtol=RTOL, err_msg=str(msg))
                    np.testing.assert_allclose(res[ag]["step_familiarity"], wnt["step_familiarity"], rtol=RTOL, err_msg=str(msg))
        finally:
            eng.close()


def test_weighted_passes_of_64_headings_match_the_oracle_per_agent():
    """11 agents x 16 headings (passes of 64, 64 and 48 headings) on 41 500 views of 16x16, the weights cycling over five values:
    on-level and off-level patches, duplicates across view groups, a planted exact match; every scoring form."""
    F, h, w, A, n_agents, seed = 41500, 16, 16, 16, 11, 77
    lib = synth.synth_views(seed, F, h, w)
    lib[40000] = lib[123]                                            # duplicates in different ranges of view groups
    weights = [WEIGHTS[i % len(WEIGHTS)] for i in range(n_agents)]
    _check_weighted(lib, _batch_inputs(seed, F, h, w, n_agents, A, lib), weights, MODES)


@pytest.mark.parametrize("kind", ["small", "generic", "full_range_s"])
def test_weighted_batches_on_other_layouts_match_the_oracle(kind):
    """The unfused finishing (a small library), the generic-hue layout (more than four hues) and the mixed layout (saturation from
    the whole 0..127 range): per-agent weights against the oracle."""
    h, w, A, n_agents, seed = 16, 16, 16, 11, 91
    F = 3001 if kind == "small" else 12000
    lib = synth.synth_views(seed, F, h, w, full_range_s=(kind == "full_range_s"))
    check = None
    if kind == "generic":                                            # sixteen hues with S > 0
        lib[..., 0] = synth.random_hsv(seed + 1, lib.shape[:-1]) & 0x0F
        check = lambda info: info["generic_hue"] or pytest.fail("expected the generic-hue layout")     # noqa: E731
    cases = _batch_inputs(seed, F, h, w, n_agents, A, lib)
    if kind == "generic":
        for i, (_, p) in enumerate(cases):
            p[..., 0] = synth.random_hsv(seed + 30 + i, p.shape[:-1]) & 0x0F
            p[2, 5], p[10, A - 1] = lib[123], lib[F - 1]
    if kind == "full_range_s":
        for i, (_, p) in enumerate(cases):
            p[..., 1] = synth.synth_patches(seed + 20 + i, n_agents * A, h, w, full_range_s=True).reshape(p.shape)[..., 1]
    weights = [WEIGHTS[(i + 2) % len(WEIGHTS)] for i in range(n_agents)]
    _check_weighted(lib, cases, weights, ("default", "exact", "force_resolve"), info_check=check)


# ------------------------------------------------------------------ 3. weighted equals uniform
def test_weighted_records_equal_uniform_records_at_each_weight():
    """Each agent's weighted record is bit for bit the unweighted batch's record of the same agents on a library ingested at that
    agent's weight (same range layout); weights all equal to the library's give the unweighted call's records."""
    F, h, w, A, n_agents, seed = 41500, 16, 16, 16, 10, 5
    lib = synth.synth_views(seed, F, h, w)
    patches = synth.synth_patches(seed + 1, n_agents * A, h, w).reshape(n_agents, A, h, w, 3)
    patches[3, 7] = lib[9001]
    patches[8] = lib[2000:2000 + A]                                  # an agent with an exact match on every heading
    weights = [WEIGHTS[i % len(WEIGHTS)] for i in range(n_agents)]
    keys = ("best_heading", "best_view", "best_fam", "flags", "angle_fam", "angle_view")

    def rec(r, ag):
        return tuple(np.asarray(r.records[ag][k]).tobytes() for k in keys)

    eng = engine_with({})
    try:
        eng.set_weight_range(0.0, 1.0)
        eng.set_library(lib, 0.25)
        eng.step_batch(patches, chem_weights=weights)
        got = eng.step_batch(patches, chem_weights=weights)
        mixed = [rec(got, ag) for ag in range(n_agents)]
        same = eng.step_batch(patches, chem_weights=[0.25] * n_agents)
        plain = eng.step_batch(patches)
        assert [rec(same, ag) for ag in range(n_agents)] == [rec(plain, ag) for ag in range(n_agents)]
        for cw in sorted(set(weights)):
            eng.set_library(lib, cw)                                 # same range, so the same layout: only the weight differs
            eng.step_batch(patches)
            uni = eng.step_batch(patches)
            for ag in range(n_agents):
                if weights[ag] == cw:
                    assert mixed[ag] == rec(uni, ag), (ag, cw)
    finally:
        eng.close()


# ------------------------------------------------------------------ 4. refusals
def test_weighted_calls_refuse_what_the_layout_cannot_serve():
    F, h, w, A, n_agents = 5000, 16, 16, 8, 3
    lib = synth.synth_views(3, F, h, w)
    patches = synth.synth_patches(4, n_agents * A, h, w).reshape(n_agents, A, h, w, 3)
    patches[1, 2] = lib[321]
    eng = engine_with({})
    try:
        eng.set_library(lib, 0.0)                                    # cw 0 alone: no saturation planes
        assert eng.library_info()["weight_range"] == (0.0, 0.0)
        for bad in ([0.0, -0.1, 0.0], [0.0, 1.5, 0.0]):              # DV_ERR_INVALID
            with pytest.raises(ValueError, match="agent 1: chem_weight .* outside"):
                eng.step_batch(patches, chem_weights=bad)
        with pytest.raises(navsim_amd.EngineError, match="agent 2: .*hue/saturation"):      # DV_ERR_STATE: no saturation planes
            eng.step_batch(patches, chem_weights=[0.0, 0.0, 0.5])
        with pytest.raises(ValueError, match="chem_weights"):
            eng.step_batch(patches, chem_weights=[0.0, 0.0])
        with pytest.raises(ValueError, match="weight range"):
            eng.set_weight_range(0.3, 1.0)
            eng.set_library(lib, 0.25)                               # the ingest's weight lies outside the range
        # the resident library still serves a correct unweighted step
        eng.set_weight_range(1.0, 0.0)
        eng.set_library(lib, 0.0)
        r = eng.step_batch(patches)
        for ag in range(n_agents):
            want = oracle.step(lib, patches[ag], 0.0, want_scene=False)
            assert (r[ag]["best_idex"], r[ag]["best_view"]) == (want["best_idex"], want["best_view"])
            np.testing.assert_allclose(r[ag]["angle_familiarity"], want["angle_familiarity"], rtol=RTOL)
        assert (r[1]["best_idex"], r[1]["best_view"]) == (2, 321)
        w0 = eng.step_batch(patches, chem_weights=[0.0] * n_agents)           # the weight it was laid out for is served
        assert [x["best_view"] for x in w0] == [x["best_view"] for x in r]
    finally:
        eng.close()
