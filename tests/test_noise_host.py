"""Sensor noise, what needs no GPU: the statement's own properties (tests/helpers_noise.py), the conditions the inputs of
tests/test_gpu_noise.py must meet (so that a passing GPU test cannot be vacuous), the binding surface of dv_noise_*, and the Python-side
checks of FamiliarityEngine.noise_rows and from_landscapes(noise=...), which are made before any library call."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import synth
from tests import helpers_noise as HZ

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"dv_noise_rows": "noise_rows", "dv_noise_clear": "noise_clear", "dv_noise_info": "noise_info"}
ENSEMBLES = (navsim_amd.MushroomRouteEnsemble, navsim_amd.InfomaxRouteEnsemble, navsim_amd.SadsRouteEnsemble, navsim_amd.SsdRouteEnsemble)


# ---- the statement -----------------------------------------------------------------------------------------------------------------------
def test_amplitude_one_reaches_both_ends_within_a_7x5_view_of_three_headings():
    n_s, n_v = zip(*(HZ.draws(HZ.SEED, 0xFEDCBA9876543210, a, 35, 1, 1) for a in range(3)))
    n_s, n_v = np.concatenate(n_s), np.concatenate(n_v)
    assert len(n_s) == 105 and set(n_s.tolist()) == {-1, 0, 1} and set(n_v.tolist()) == {-1, 0, 1}


def test_amplitude_255_reaches_both_ends_in_10240_draws_and_every_amplitude_stays_in_range():
    n_s, n_v = HZ.draws(HZ.SEED, 3, 0, 10240, 255, 255)
    assert n_s.min() == -255 and n_s.max() == 255 and n_v.min() == -255 and n_v.max() == 255
    for amp in (0, 1, 2, 20, 127, 254):
        s, v = HZ.draws(7, 11, 2, 4096, amp, 255 - amp)
        assert s.min() >= -amp and s.max() <= amp and v.min() >= amp - 255 and v.max() <= 255 - amp
        if amp:
            assert s.min() == -amp and s.max() == amp                                     # 4096 draws over at most 509 values
    zero_s, zero_v = HZ.draws(HZ.SEED, 5, 1, 1000, 0, 0)
    assert not zero_s.any() and not zero_v.any()


def test_two_keys_or_two_seeds_agree_at_the_chance_rate():
    """At amplitude 20 a draw takes 41 values: 10240 independent pairs agree 250 times on average (sigma 15.6)."""
    base = HZ.draws(1, 100, 0, 10240, 20, 20)
    for seed, key in ((1, 101), (2, 100), (1, 100 + (1 << 32)), (1, 100 | (1 << 63))):
        other = HZ.draws(seed, key, 0, 10240, 20, 20)
        for c in range(2):
            same = int((base[c] == other[c]).sum())
            assert 170 <= same <= 330, (seed, key, c, same)
    # S and V of one word are the word's two halves: independent of each other as well
    assert 170 <= int((base[0] == base[1]).sum()) <= 330


def test_the_counter_is_distinct_across_headings_and_the_draws_follow_it():
    P, A = 35, 5
    c = np.concatenate([HZ.counters(a, P) for a in range(A)])
    assert len(set(c.tolist())) == A * P and c.tolist() == list(range(A * P))
    # heading a of a member is the stream's pixels a P .. (a + 1) P: a launch that begins inside a member draws what one launch would
    whole = HZ.draws(9, 77, 0, A * P, 20, 20)
    for a in range(A):
        part = HZ.draws(9, 77, a, P, 20, 20)
        assert np.array_equal(part[0], whole[0][a * P:(a + 1) * P]) and np.array_equal(part[1], whole[1][a * P:(a + 1) * P])
    assert not np.array_equal(HZ.draws(9, 77, 0, P, 20, 20)[1], HZ.draws(9, 77, 1, P, 20, 20)[1])


def test_the_draw_is_the_statement_written_out_in_python_integers():
    M = (1 << 64) - 1

    def sm(z):
        z &= M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    seed, key, a, P, amp_s, amp_v = HZ.SEED, 0xF00DFACE12345678, 2, 35, 20, 3
    assert int(synth.splitmix64(np.uint64(12345))) == sm(12345)
    base = sm(key + seed * 0x9E3779B97F4A7C15)
    n_s, n_v = HZ.draws(seed, key, a, P, amp_s, amp_v)
    for j in (0, 1, 17, 34):
        word = sm(base + a * P + j)
        assert n_s[j] == (((word & 0xFFFFFFFF) * (2 * amp_s + 1)) >> 32) - amp_s
        assert n_v[j] == (((word >> 32) * (2 * amp_v + 1)) >> 32) - amp_v


def test_noise_clamps_at_both_ends_keeps_the_hue_and_the_zero_row_is_the_identity():
    raw = np.zeros((5, 7, 3), dtype=np.uint8)
    raw[..., 0] = 99
    raw[..., 1] = 0
    raw[..., 2] = 255
    out = HZ.add_noise(raw, 5, 6, 0, 255, 255)
    n_s, n_v = HZ.draws(5, 6, 0, 35, 255, 255)
    assert (out[..., 0] == 99).all()
    assert np.array_equal(out[..., 1].reshape(-1), np.maximum(n_s, 0)) and (n_s < 0).any()        # S = 0: every negative draw clamps
    assert np.array_equal(out[..., 2].reshape(-1), 255 + np.minimum(n_v, 0)) and (n_v > 0).any()  # V = 255: every positive draw clamps
    assert np.array_equal(HZ.add_noise(raw, 5, 6, 0, 0, 0), raw)
    # the vectorised form used at SLAB's size is the same statement
    views = np.random.default_rng(1).integers(0, 256, (4, 3, 5, 7, 3), dtype=np.uint8)
    keys, amp_s, amp_v = HZ.rows(2, 4)
    got = HZ.noise_on_views(views, 9, keys, amp_s, amp_v)
    for i in range(4):
        for a in range(3):
            assert np.array_equal(got[i, a], HZ.add_noise(views[i, a], 9, int(keys[i]), a, amp_s[i], amp_v[i]))


def test_the_key_layouts_of_training_and_steps():
    assert HZ.train_key(0, 0) == 0x80000000 << 32 and HZ.train_key(3, 7) == (0x80000003 << 32) | 7
    assert HZ.step_key(5, 0) == 5 << 32 and HZ.step_key(2 ** 31 - 1, 9) == ((2 ** 31 - 1) << 32) | 9
    # a step's key never is a training key: streams stay below 2**31
    assert HZ.step_key(2 ** 31 - 1, 2 ** 32 - 1) < HZ.train_key(0, 0)
    E = navsim_amd.MushroomRouteEnsemble
    assert E._train_keys(3, 4).dtype == np.uint64 and E._train_keys(3, 4).tolist() == [HZ.train_key(3, v) for v in range(4)]
    assert E._step_key(5, 9) == HZ.step_key(5, 9)


# ---- the inputs' conditions --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("thin", "wide"))
def test_the_sense_cases_rows_change_their_views_and_respect_levels_and_mask(name):
    s = HZ.sense_case(name)
    assert s["noisy"].shape == (11,) + {"thin": (5, 7, 3), "wide": (8, 16, 3)}[name]
    assert sorted(set(zip(s["amp_s"].tolist(), s["amp_v"].tolist()))) == sorted(HZ.ROWS5)
    assert int(s["keys"][0]) >> 63 == 1 and int(s["keys"].max()) > 2 ** 63 and len(set(s["keys"].tolist())) == 11
    assert sorted(set(s["land_of"].tolist())) == [0, 1] and [l.shape for l in HZ.lands()] == [(151, 131, 3), (140, 170, 3)]
    if name == "thin":
        assert 35 % 64 != 0 and 64 // 35 >= 1                                             # a wavefront spans poses of different rows
    else:
        for v in range(11):
            cfg = s["cfgs"][s["land_of"][v]]
            assert set(np.unique(s["noisy"][v][..., 2]).tolist()) <= set(np.unique(HZ.level_table(cfg)[2]).tolist())
            if cfg["mask"]:
                assert not s["noisy"][v][:, 8 - cfg["mask"]:8 + cfg["mask"]].any()
        masked_255 = [v for v in range(11) if s["amp_v"][v] == 255 and s["cfgs"][s["land_of"][v]]["mask"]]
        assert masked_255                                                                   # a masked entry meets amplitude 255


def test_the_footprints_of_every_configuration_stay_on_both_landscapes_in_the_box():
    """The half diagonal of the footprint, and a pixel for the rounding, fit between BOX and every edge: no heading leaves a landscape."""
    for cfg in (HZ.THIN_B, HZ.WIDE_A, HZ.BIG_B, HZ.PLAIN32, HZ.ENS):
        w, h = cfg["sensor"][0] * cfg["pixel"][0], cfg["sensor"][1] * cfg["pixel"][1]
        r = np.hypot(w / 2, h / 2) + 1
        for land in HZ.lands():
            assert r < HZ.BOX[0] and HZ.BOX[1] < land.shape[1] - r and r < HZ.BOX[2] and HZ.BOX[3] < land.shape[0] - r, (cfg, land.shape)


@pytest.mark.parametrize("table", (False, True))
def test_the_mushroom_cases_are_moved_by_the_noise(table):
    t = HZ.mb_train_case("thin", table)                       # (asserts that both banks differ from the noiseless training)
    assert sorted(set(t["bank_of"].tolist())) == [0, 1] and t["views"].shape == (9, 5, 7, 3)
    c = HZ.mb_step_case("thin", table)                        # (asserts that the scores differ from the noiseless ones)
    assert c["fam"].shape == (3, 3) and c["planes"].shape == (3, 3, 5, 7, 3)
    assert HZ.MB_SHAPES["big"][0]["sensor"][0] * HZ.MB_SHAPES["big"][0]["sensor"][1] > 256   # a thread senses more than one pixel


def test_the_slab_case_cuts_inside_a_member_and_launch_local_rows_would_show():
    c = HZ.slab_case()
    lay = c["lay"]
    A = lay["A"]
    assert (len(c["banks"]), A, lay["c0"]) == (688, 12, 8176) and lay["c0"] % A == 4
    order = lay["order"]
    behind = order[lay["c0"] // A:]
    local = order[:len(behind)]                               # the members a launch-local row index would read
    assert all(c["keys"][i] != c["keys"][j] for i, j in zip(behind, local))
    assert len(set(c["keys"].tolist())) == 688 and sorted(set(c["lands"].tolist())) == [0, 1]


def test_the_store_case_holds_two_routes_of_5_and_70_views():
    s = HZ.store_case()
    assert s["first"].tolist() == [0, 5, 75] and s["views"].shape == (75, 5, 7, 3) and s["patches"].shape == (3, 3, 5, 7, 3)
    assert (s["win_lo"] < s["win_hi"]).all() and s["win_hi"].tolist() <= [5, 70, 70]
    plain = HZ.member_views(HZ.THIN, s["xs"], s["ys"], s["angs"], s["lands"], HZ.SEED, s["keys"], [0] * 3, [0] * 3)
    assert all(not np.array_equal(plain[i], s["patches"][i]) for i in range(3))


def test_the_replicates_of_one_pose_see_different_rows_under_different_streams():
    """Test 8's condition: members 0 and 1 of the ensemble stand at one pose and differ in their stream alone; by the statement their
    first rows differ, and member 0's row is not the noiseless one."""
    starts = HZ.ens_starts()
    assert starts[0] == starts[1] and HZ.ENS_NOISE["streams"][0] != HZ.ENS_NOISE["streams"][1]
    assert HZ.ENS_NOISE["amp_v"][0] == HZ.ENS_NOISE["amp_v"][1]
    a, b = HZ.shadow(0, 1)[0], HZ.shadow(1, 1)[0]
    assert np.array_equal(a["angles"], b["angles"]) and not np.array_equal(a["patches"], b["patches"])
    assert not np.array_equal(a["fam"], b["fam"]), (a["fam"], b["fam"])
    plain = HZ.shadow(0, 1, noise=dict(HZ.ENS_NOISE, amp_v=[0, 0, 0, 0]))[0]
    assert not np.array_equal(plain["fam"], a["fam"])
    assert not np.array_equal(HZ.mushroom_first_row(0), HZ.mushroom_first_row(1))          # ... under the mushroom body as well
    # the routes lie inside their landscapes' bounds for the ensemble's sensor, and route 1's views carry training noise
    for l, route in HZ.ens_routes():
        rows_, cols = HZ.lands()[l].shape[:2]
        assert (route > 8).all() and (route[:, 0] < cols - 8).all() and (route[:, 1] < rows_ - 8).all()
    r1 = HZ.ens_routes()[1][1]
    hd = HZ.route_headings(r1)
    assert any(not np.array_equal(HZ.ens_train_views()[1][v], HZ.view(HZ.lands()[1], HZ.ENS, r1[v][0], r1[v][1], hd[v])) for v in range(len(r1)))


# ---- binding surface -----------------------------------------------------------------------------------------------------------------------
def test_header_bindings_engine_and_library_agree_on_the_noise_names():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    declared = set(re.findall(r"\bint\s+(dv_noise_[a-z0-9_]*)\s*\(", header))
    assert declared == set(NAMES) == {k for k in N.PROTOTYPES if k.startswith("dv_noise_")}
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert N.PROTOTYPES[name][0] is ctypes.c_int
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(N.PROTOTYPES[name][1]), name
        assert callable(getattr(navsim_amd.FamiliarityEngine, NAMES[name])), name
    assert navsim_amd.FamiliarityEngine.n_noise_rows == 0
    for E in ENSEMBLES:
        assert inspect.signature(E.from_landscapes).parameters["noise"].default is None
        assert "noise" not in inspect.signature(E.from_routes_with).parameters and "noise" not in inspect.signature(E.from_routes).parameters
        assert "from_landscapes([landscape]" in E.from_routes_with.__doc__ or "from_landscapes([landscape]" in navsim_amd.MushroomRouteEnsemble.from_routes_with.__doc__


def test_the_noise_kernel_forms_use_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    table = {r["name"]: r for r in kernel_resources.kernel_table()}
    for name in ("k_sense_lands_noise", "k_sense_lands_sensors_noise", "k_mb_pose_bank_lands_noise", "k_mb_pose_bank_lands_sensors_noise"):
        assert name in table, name
        assert table[name]["scratch"] == 0 and table[name]["vgpr_spills"] == 0, table[name]


# ---- the Python-side checks: before any library call -------------------------------------------------------------------------------------------
class _NoLibrary(object):
    def __getattr__(self, name):
        raise AssertionError("library call %s after arguments that must be refused" % name)


def test_refused_noise_rows_never_reach_the_library():
    e = navsim_amd.FamiliarityEngine.__new__(navsim_amd.FamiliarityEngine)
    e._lib, e._ctx_raw, e._begun = _NoLibrary(), None, False
    keys = np.array([1, 2, 3], dtype=np.uint64)
    for bad, match in (((-1, keys, [0] * 3, [0] * 3), r"seed must be an integer in \[0, 2\*\*64\)"),
                       ((2 ** 64, keys, [0] * 3, [0] * 3), "seed must be"),
                       ((1.5, keys, [0] * 3, [0] * 3), "seed must be"),
                       ((0, keys.astype(np.int64), [0] * 3, [0] * 3), "keys must be uint64"),
                       ((0, np.zeros((3, 1), dtype=np.uint64), [0] * 3, [0] * 3), "keys must be uint64"),
                       ((0, keys[:0], [], []), "keys must be uint64"),
                       ((0, keys, [0, 0], [0] * 3), r"amp_s must have shape \(3,\)"),
                       ((0, keys, [0] * 3, [0] * 4), r"amp_v must have shape \(3,\)"),
                       ((0, keys, [0, 256, 0], [0] * 3), r"amp_s\[1\] = 256 outside \[0, 255\]"),
                       ((0, keys, [0] * 3, [0, 0, -1]), r"amp_v\[2\] = -1 outside"),
                       ((0, keys, [0.0] * 3, [0] * 3), "amp_s must hold integers")):
        with pytest.raises(ValueError, match=match):
            e.noise_rows(*bad)
    assert e.n_noise_rows == 0


def _agent(model):
    a = navsim_amd.NavBySceneFamiliarity(np.array(HZ.lands()[0]), HZ.ENS["sensor"], 1.0, n_test_angles=5, use_gpu_sensor=False,
                                         familiarity_model=model)
    a._engine = HZ.FakeEngine()                                                          # an engine that must never be called
    return a


def test_from_landscapes_refuses_bad_noise_before_it_touches_the_engine():
    from navsim_amd import infomax_familiarity, mushroom_familiarity, sads_familiarity, ssd_familiarity
    models = (lambda: mushroom_familiarity(n_kc=100, fan_in=4, sparsity=0.1, seed=1), lambda: infomax_familiarity(n_hidden=4),
              lambda: sads_familiarity(0.25), lambda: ssd_familiarity(2))
    L, routes, starts = list(HZ.lands()), HZ.ens_routes(), HZ.ens_starts()
    for E, model in zip(ENSEMBLES, models):
        for bad, match in (((1, 2), "noise must be None or a dict"),
                           (dict(amp=3), r"noise: unknown keys \['amp'\]"),
                           (dict(seed=-1), r"noise\['seed'\] must be an integer in \[0, 2\*\*64\)"),
                           (dict(seed=1.0), r"noise\['seed'\]"),
                           (dict(amp_v=256), r"noise\['amp_v'\] = 256: an amplitude"),
                           (dict(amp_s=-1), r"noise\['amp_s'\] = -1"),
                           (dict(amp_v=2.0), r"noise\['amp_v'\] = 2.0"),
                           (dict(amp_v=[1, 2, 3]), r"noise\['amp_v'\] holds 3 values for 4 starts"),
                           (dict(amp_s=[1, 2, 3, 300]), r"noise\['amp_s'\]\[3\] = 300"),
                           (dict(train_amp_v=[1, 2, 3]), r"noise\['train_amp_v'\] holds 3 values for 2 routes"),
                           (dict(train_amp_s=[0, True]), r"noise\['train_amp_s'\]\[1\] = True"),
                           (dict(streams=[1, 2, 3]), r"noise\['streams'\] must be None or a list with one stream per start \(4\)"),
                           (dict(streams=[1, 2, 3, 2 ** 31]), r"noise\['streams'\]\[3\] = 2147483648"),
                           (dict(streams=[1, 2, -3, 4]), r"noise\['streams'\]\[2\] = -3"),
                           (dict(streams=[4, 2, 3, 2]), r"noise\['streams'\]\[3\] = 2 duplicates noise\['streams'\]\[1\]")):
            a = _agent(model())
            with pytest.raises(ValueError, match=match):
                E.from_landscapes(a, L, routes, starts, noise=bad)
            assert a._engine.calls == []
    with pytest.raises(ValueError, match="noise with populations"):
        navsim_amd.MushroomRouteEnsemble.from_landscapes(_agent(models[0]()), L, routes, starts, noise=dict(amp_v=1), populations=[None, None])


def test_the_noise_argument_as_the_ensembles_take_it():
    E = navsim_amd.SsdRouteEnsemble
    assert E._noise_arg(None, 4, 2) is None
    got = E._noise_arg(dict(amp_v=20), 4, 2)
    assert got == dict(seed=0, amp_s=[0] * 4, amp_v=[20] * 4, train_amp_s=[0, 0], train_amp_v=[0, 0], streams=[0, 1, 2, 3])
    got = E._noise_arg(HZ.ENS_NOISE, 4, 2)
    assert got["amp_v"] == [40, 40, 25, 60] and got["train_amp_v"] == [0, 12] and got["streams"] == [5, 9, 2, 7] and got["seed"] == 77
    assert E._noise_arg(dict(seed=2 ** 64 - 1, streams=np.array([3, 0, 2 ** 31 - 1, 1])), 4, 2)["streams"] == [3, 0, 2 ** 31 - 1, 1]
    assert E._noise_seed is None and set(E.NOISE_KEYS) == {"seed", "amp_s", "amp_v", "train_amp_s", "train_amp_v", "streams"}
