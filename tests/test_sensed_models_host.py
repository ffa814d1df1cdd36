"""What the sensed tests of the learned models must distinguish (tests/helpers_sensed_models.py), held on the CPU: the conditions on the
host sensor model's planes and the two NumPy statements, and the Infomax tolerance rule of tests/helpers_infomax.py applied to the new
chains and scores.  Nothing here touches the device."""
import numpy as np
import pytest

from tests import helpers_infomax as HI
from tests import helpers_mushroom as H
from tests import helpers_sensed_models as S


def test_configurations_are_what_they_are_for():
    shape = {name: (c["sensor"], tuple(c["pixel"]), c["levels"], c["mask"]) for name, c in S.CONFIGS.items()}
    assert shape["px"] == ((16, 8), (2, 4), 4, 1) and shape["odd"] == ((19, 17), (2, 2), 5, 2)
    assert shape["tall"] == ((6, 23), (3, 2), 7, 0) and shape["wide"] == ((34, 10), (1, 1), 5, 3)
    assert [S.n_pixels(k) for k in ("px", "odd", "tall", "wide")] == [128, 323, 138, 340]
    assert S.n_pixels("odd") % 4 == 3 and 256 < S.n_pixels("odd") < 512 and S.n_pixels("wide") % 256 != 0
    assert len(S.CASES) == 11 and ("wide", 1) not in S.CASES
    for name, c in S.CONFIGS.items():
        assert (c["sensor"][0] * c["pixel"][0]) % 2 == 0 and (c["sensor"][1] * c["pixel"][1]) % 2 == 0, name
    # the shared setup is helpers_infomax.SENSED's
    assert S.scenes("sq")["route"].tobytes() == HI.sensed_data()["scenes"].tobytes()
    xs, ys, angs = S.member_poses()
    assert angs.shape == (5, 13) and len(np.unique(angs)) == 65
    x, y, la = S.lone_pose()
    assert (x, y) == H.step_xy() and len(np.unique(la)) == 13


@pytest.mark.parametrize("name", ["px", "odd", "tall", "wide"])
def test_host_views_of_a_configuration(name):
    c = S.CONFIGS[name]
    w, h = c["sensor"]
    s = S.scenes(name)                                                                   # (asserts the mask's columns)
    assert s["route"].shape == (45, h, w, 3) and s["members"].shape == (5, 13, h, w, 3) and s["lone"].shape == (13, h, w, 3)
    every = np.concatenate([s["route"], s["members"].reshape(-1, h, w, 3), s["lone"]])
    # V takes the configuration's levels only; H and S keep all 256
    table = np.unique(np.rint(np.arange(256, dtype=np.float32) / 255 * (c["levels"] - 1)) / (c["levels"] - 1) * 255).astype(np.uint8)
    assert set(np.unique(every[..., 2])) <= set(table.tolist()) | {0}
    if c["pixel"] != (1, 1):
        assert len(np.unique(every[..., 2])) > 2                                         # (block means: levels between the landscape's two)
        # the block branch: saturations that a single landscape pixel cannot have (sums of a block, wrapped)
        from navsim_amd import synth
        land = synth.synth_landscape(*HI.SENSED["land"])
        assert not set(np.unique(every[..., 1])) <= set(np.unique(land[..., 1]))
    # no two channels are one plane
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not np.array_equal(every[..., a], every[..., b])


@pytest.mark.parametrize("name,channel", S.CASES)
def test_conditions_of_a_case(name, channel):
    d = S.data(name, channel)                                                            # (asserts the per-case conditions)
    K = S.MB["n_kc"]
    assert d["conn"].shape == (K, S.MB["fan_in"]) and d["conn"].max() < d["h"] * d["w"]
    zeros = int((d["wt"] == 0).sum())
    assert 0 < zeros <= K // 2
    assert d["mb_fam"].shape == d["im_fam"].shape == (5, 13) and d["mb_lone"].shape == d["im_lone"].shape == (13,)
    assert d["mb_fam"].min() < 0 and all(len(np.unique(r)) > 1 for r in d["mb_fam"]) and len(np.unique(d["mb_lone"])) > 1
    # the route's own views are familiar to the statement trained on them
    assert not H.novelty(d["wt"], d["views"], d["conn"], d["n_active"]).any()
    margins = [HI.best_margin(r) for r in list(d["im_fam"]) + [d["im_lone"]]]
    print("%s ch %d: %d of %d weights depressed; least Infomax margin %.2e" % (name, channel, zeros, K, min(margins)))
    assert min(margins) >= S.MARGIN > 1000 * HI.TOL
    assert (np.argmax(d["im_fam"], axis=1) != 0).any() and (np.argmax(d["mb_fam"], axis=1) != 0).any()
    assert d["W"].shape == (S.CONFIGS[name]["n_hidden"], d["h"] * d["w"]) and np.abs(d["W"]).max() < 10


@pytest.mark.parametrize("name", ["px", "odd", "tall", "wide"])
def test_channels_of_a_configuration_differ(name):
    S.assert_channels_differ(name)
    if name == "wide":
        # why wide has no channel 1: under [1, 1] pixels on this landscape S and V give the mushroom statement the same d
        s = S.scenes(name)
        conn, n_active = S.mb_model(name)
        fam = []
        for ch in (1, 2):
            wt = H.train(np.ones(S.MB["n_kc"], np.uint8), S.plane(s["route"], ch), conn, n_active)
            fam.append(S.mb_scores(wt, S.plane(s["members"], ch), conn, n_active))
        assert np.array_equal(fam[0], fam[1])


@pytest.mark.parametrize("name,channel", S.CASES + (("sq", 2),))
def test_new_chains_and_scores_keep_the_gpu_tolerance(name, channel):
    """The rule of tests/test_infomax_host.py: float64 against longdouble and against a permuted order, weights relative to max|W| and
    scores to max|d|; 1000 x the largest is under TOL, so the device is held to TOL on these chains and scores too."""
    chain, score = S.im_discrepancies(name, channel)
    top = np.abs(S.data(name, channel)["W"]).max()
    print("infomax restatement, sensed %s ch %d: W %.2e, d %.2e (max|W| %.3g)" % (name, channel, chain, score, top))
    assert 1000 * max(chain, score) <= HI.TOL


@pytest.mark.parametrize("name", S.FLAG_GROUPS)
def test_flag_positions_and_layouts(name):
    """On the axes' headings the footprint stays on the landscape at FLAG_AT, on the diagonals it leaves it (the host model's
    IndexError); the layouts flag whom they should and the statement decides every row that is compared."""
    S.flag_facts(name)
    for model, A, late in (("mb", 260, 257), ("im", 70, 65)):
        L = S.flag_layouts(name, model)
        c, t = L["corners"], L["trips"]
        assert c["angs"].shape == (5, 9) and c["flags"].tolist() == [16, 16, 16, 16, 0] and c["off"] == [(0, 1), (1, 3), (2, 5), (3, 7)]
        assert [round(float(np.rad2deg(c["angs"][i, a]))) for i, a in c["off"]] == [45, 135, 225, 315]
        assert t["angs"].shape == (3, A) and t["flags"].tolist() == [16, 0, 16] and t["off"] == [(0, A - 1), (2, late)]
        assert late >= (256 if model == "mb" else 64)                                    # a column of the decide kernel's second trip
        for lay in (c, t):
            assert int((~lay["keep"]).sum()) == len(lay["off"]) and not lay["clean"][~lay["keep"]].tolist() == lay["angs"][~lay["keep"]].tolist()
            assert np.array_equal(lay["clean"][lay["keep"]], lay["angs"][lay["keep"]])
            assert lay[model + "_best"].tolist() == [-1 if f else int(np.argmax(lay[model + "_fam"][i])) for i, f in enumerate(lay["flags"])]
            # the compared columns of a flagged call are the clean call's
            assert np.array_equal(lay[model + "_fam"][lay["keep"]], lay[model + "_clean"][lay["keep"]])
        # the unflagged member's best heading is not where a kernel that answers 0 would put it
        assert t[model + "_best"][1] > 0
        if model == "im":
            # the tolerance rule on the layouts' scores (same weights as data(name, 2), whose chain is measured above)
            W = S.data(name, 2)["W"]
            for lay in (c, t):
                planes, want = lay["planes_clean"].reshape((-1,) + lay["planes"].shape[2:]), lay["im_clean"].reshape(-1)
                disc = max(float(np.max(np.abs(HI.familiarity(W, planes, **kw) - want)) / np.max(np.abs(want)))
                           for kw in (dict(dtype=np.longdouble), dict(order_seed=99)))
                print("infomax restatement, flag layout %s %dx%d: d %.2e" % ((name,) + lay["angs"].shape + (disc,)))
                assert 1000 * disc <= HI.TOL
