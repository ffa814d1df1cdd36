"""The sensor options under the learned models: sensor configurations, poses and the expected values of the Infomax and mushroom-body
tests that sense (tests/test_sensed_models_host.py, tests/test_gpu_sensed_models.py).

Everything here comes from the HOST sensor model (an agent with use_gpu_sensor=False: get_sensor_mat, held to the reference's recorded
outputs by tests/test_host_logic.py) and the NumPy statements of the two models (tests/helpers_mushroom.py, tests/helpers_infomax.py);
nothing is derived from the device.  Computed once (functools.lru_cache) and read-only.

Shared setup, that of helpers_infomax.SENSED: synth.synth_landscape(3, 300, 4), the first 45 points of sin_training_path(0.5, 60, 180,
arclen=1.0), each view looking along helpers_mushroom.route_headings.  Scored poses: five members x 13 headings beside the route
(helpers_mushroom_ensemble.sensed_poses(13), each member's headings spread over half a circle about its centre) and a lone step of 13
headings at route[7] + (0.6, -0.3) about the route's heading there.

CONFIGS (the agent requires sw*pw and sh*ph to be even):

    name   sensor (w, h)  pixel dims  levels  mask  N     reaches
    px     (16, 8)        [2, 4]      4       1     128   the reference's traj_px sensor: block branch, S wrap, mask
    odd    (19, 17)       [2, 2]      5       2     323   N % 4 = 3; a second, partial trip of a 256-thread fill; odd width under the mask
    tall   (6, 23)        [3, 2]      7       0     138   h > w and pw != ph: a swapped sw/sh or pw/ph shows
    wide   (34, 10)       [1, 1]      5       3     340   the nblk == 1 branch with mask and levels; N % 256 != 0
    sq     (32, 32)       [1, 1]      5       0     1024  helpers_infomax.SENSED's sensor, for the flag tests only (channel 2)

Channels 0, 1 and 2 (H, S, V) for px, odd and tall; 0 and 2 for wide, where with [1, 1] pixels on this landscape the S and V planes are
monotone images of one another and the mushroom statement gives them identical d.  Models are small: n_kc=1043, fan_in=8, n_active=21
(16 for tall: MB_ACTIVE); n_hidden=20 (70 for odd), learning_rate=1e-3.

Conditions asserted in data(), on the CPU, so that no test passes on a kernel that reads the wrong channel or returns a constant:
every compared plane has more than one value and the masked columns are 0 in all three channels; the mushroom weights have
0 < zeros <= K/2; some scored column has d > 0 and no member's 13 scores are all equal; within a configuration the channels' mushroom
scores, trained weights and Infomax scores differ pairwise; every member's best Infomax heading leads by best_margin >= 1e-6 (far above
TOL) and some member's best heading is not 0.  A seed is changed if one fails, never a condition.

Flag layouts (flag_layouts): at FLAG_AT[name] the footprint stays on the landscape at headings of 0, 90, 180 and 270 degrees (and a few
degrees about them: SAFE_JITTER) and leaves it at 45, 135, 225 and 315 -- established by the host model's IndexError for every pose a
layout uses (flag_facts, _checked_planes), never assumed."""
import functools

import numpy as np

from tests import helpers_infomax as HI
from tests import helpers_mushroom as H
from tests import helpers_mushroom_ensemble as HE

CONFIGS = {
    "px": dict(sensor=(16, 8), pixel=(2, 4), levels=4, mask=1, channels=(0, 1, 2), n_hidden=20, mb_seed=61, im_seed=71),
    "odd": dict(sensor=(19, 17), pixel=(2, 2), levels=5, mask=2, channels=(0, 1, 2), n_hidden=70, mb_seed=62, im_seed=72),
    "tall": dict(sensor=(6, 23), pixel=(3, 2), levels=7, mask=0, channels=(0, 1, 2), n_hidden=20, mb_seed=63, im_seed=73),
    "wide": dict(sensor=(34, 10), pixel=(1, 1), levels=5, mask=3, channels=(0, 2), n_hidden=20, mb_seed=64, im_seed=74),
    # the flag tests' square sensor: no member of CASES
    "sq": dict(sensor=(32, 32), pixel=(1, 1), levels=5, mask=0, channels=(2,), n_hidden=20, mb_seed=65, im_seed=75),
}
CASES = tuple((name, ch) for name in ("px", "odd", "tall", "wide") for ch in CONFIGS[name]["channels"])
MB = dict(n_kc=1043, fan_in=8, n_active=21)
# tall's S plane alone: its 45 route views are so varied under 21 firing cells that they depress 574 .. 618 of the 1043 cells whatever
# the connectivity's seed (47 seeds tried), more than the K/2 the weights' condition allows.  The condition stays; tall's model fires 16.
MB_ACTIVE = {"tall": 16}
IM_ETA = 1e-3
N_MEMBERS, N_HEADINGS = 5, 13
MARGIN = 1e-6                                       # of every member's best Infomax heading: far above HI.TOL

# flag tests: where the footprint is on the landscape at the axes' headings and off it at the diagonals
FLAG_AT = {"sq": (281.0, 281.0), "odd": (278.0, 278.0)}
FLAG_GROUPS = tuple(FLAG_AT)
SAFE_DEG, OFF_DEG = (0.0, 90.0, 180.0, 270.0), (45.0, 135.0, 225.0, 315.0)
SAFE_JITTER = 4.0                                   # degrees about a safe heading that the layouts use
SENSE_ERROR = 16


def n_pixels(name):
    w, h = CONFIGS[name]["sensor"]
    return w * h


def _keep(scenes):
    def func(scene, fambuf):
        fambuf[...] = 0.0
    func.max_familiarity = 0.0
    return func


def make_agent(name, model, gpu_sensor, n_test_angles=9, **kw):
    """An agent on the shared landscape with the configuration's sensor options."""
    import navsim_amd
    from navsim_amd import synth
    c = CONFIGS[name]
    return navsim_amd.NavBySceneFamiliarity(synth.synth_landscape(*HI.SENSED["land"]), c["sensor"], 1.0, n_test_angles=n_test_angles,
                                            sensor_pixel_dimensions=list(c["pixel"]), n_sensor_levels=c["levels"], mask_middle_n=c["mask"],
                                            use_gpu_sensor=gpu_sensor, familiarity_model=model, **kw)


@functools.lru_cache(maxsize=None)
def _host_sensor(name):
    return make_agent(name, _keep, False)


def host_scenes(name, x, y, angles):
    """uint8[n,h,w,3]: what the HOST sensor model takes at (x[i], y[i], angles[i]) under the configuration.  IndexError where a
    footprint leaves the landscape, as the model raises it."""
    agent = _host_sensor(name)
    x, y, angles = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(angles, np.float64))
    return np.stack([agent.get_sensor_mat((xi, yi), ai) for xi, yi, ai in zip(x.reshape(-1), y.reshape(-1), angles.reshape(-1))])


def plane(scenes, channel):
    return np.ascontiguousarray(np.asarray(scenes)[..., channel])


def route():
    return HI.sensed_route()


def route_poses():
    path = route()
    return path[:, 0], path[:, 1], H.route_headings(path)


def member_poses():
    """(xs[5], ys[5], angs[5, 13]) of the batched step."""
    xs, ys, centre = HE.sensed_poses(N_HEADINGS)
    return xs, ys, (centre[:, None] + np.linspace(-np.pi / 2, np.pi / 2, N_HEADINGS)[None, :]) % (2 * np.pi)


def lone_pose():
    """(x, y, angs[13]) of the lone step."""
    path = route()
    at = H.SLAB_POSES["at"]
    x, y = path[at] + np.array(H.SLAB_POSES["xy_offset"])
    return float(x), float(y), (H.route_headings(path)[at] + np.linspace(-np.pi / 2, np.pi / 2, N_HEADINGS)) % (2 * np.pi)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def scenes(name):
    """The host sensor model's views of a configuration: dict(route uint8[45,h,w,3], members uint8[5,13,h,w,3], lone uint8[13,h,w,3])."""
    w, h = CONFIGS[name]["sensor"]
    rx, ry, ra = route_poses()
    xs, ys, angs = member_poses()
    lx, ly, la = lone_pose()
    out = dict(route=host_scenes(name, rx, ry, ra),
               members=host_scenes(name, np.repeat(xs, N_HEADINGS), np.repeat(ys, N_HEADINGS), angs.reshape(-1)).reshape(angs.shape + (h, w, 3)),
               lone=host_scenes(name, lx, ly, la))
    assert out["route"].shape == (45, h, w, 3) and out["route"].dtype == np.uint8
    mask = CONFIGS[name]["mask"]
    for s in out.values():
        flat = s.reshape(-1, h, w, 3)
        if mask:
            assert not flat[:, :, w // 2 - mask:w // 2 + mask, :].any(), name          # masked columns: 0 in all three channels
        # ... and nowhere else a whole column of zeros in all three channels of every view (the mask is what zeroed them)
        zero_cols = np.flatnonzero(~flat.any(axis=(0, 1, 3)))
        assert zero_cols.tolist() == list(range(w // 2 - mask, w // 2 + mask)), (name, zero_cols)
    _frozen(*out.values())
    return out


def mb_model(name):
    """(conn, n_active) of a configuration's mushroom model."""
    return H.connectivity(MB["n_kc"], n_pixels(name), MB["fan_in"], CONFIGS[name]["mb_seed"]), MB_ACTIVE.get(name, MB["n_active"])


def mb_scores(wt, planes, conn, n_active):
    """float64[...]: the statement's familiarity of uint8[..., h, w] planes."""
    planes = np.asarray(planes)
    lead = planes.shape[:-2]
    d = HE.novelty(wt, planes.reshape((-1,) + planes.shape[-2:]), conn, n_active)
    return (-d).astype(np.float64).reshape(lead)


def im_scores(W, planes, **kw):
    planes = np.asarray(planes)
    lead = planes.shape[:-2]
    return HI.familiarity(W, planes.reshape((-1,) + planes.shape[-2:]), **kw).reshape(lead)


@functools.lru_cache(maxsize=None)
def data(name, channel):
    """dict(scenes, views (the route's compared planes), members / lone (the scored planes), conn, n_active, wt, mb_fam [5,13], mb_lone
    [13], W0, W, im_fam [5,13], im_lone [13], h, w, M, eta) with the per-case conditions of the module docstring asserted."""
    c = CONFIGS[name]
    w, h = c["sensor"]
    s = scenes(name)
    views, members, lone = plane(s["route"], channel), plane(s["members"], channel), plane(s["lone"], channel)
    for p in np.concatenate([views, members.reshape(-1, h, w), lone]):
        assert len(np.unique(p)) > 1, (name, channel)                                 # no constant plane
    conn, n_active = mb_model(name)
    wt = H.train(np.ones(MB["n_kc"], np.uint8), views, conn, n_active)
    assert 0 < int((wt == 0).sum()) <= MB["n_kc"] // 2, (name, channel, int((wt == 0).sum()))
    mb_fam, mb_lone = mb_scores(wt, members, conn, n_active), mb_scores(wt, lone, conn, n_active)
    assert mb_fam.min() < 0 and mb_lone.min() < 0, (name, channel)                    # some column with d > 0
    for row in list(mb_fam) + [mb_lone]:
        assert len(np.unique(row)) > 1, (name, channel, row)
    M = c["n_hidden"]
    W0 = HI.initial_weights(M, h * w, c["im_seed"])
    W = HI.train(W0, views, eta=IM_ETA)
    assert np.isfinite(W).all()
    im_fam, im_lone = im_scores(W, members), im_scores(W, lone)
    for row in list(im_fam) + [im_lone]:
        assert HI.best_margin(row) >= MARGIN, (name, channel, HI.best_margin(row))
    assert (np.argmax(im_fam, axis=1) != 0).any() and (np.argmax(mb_fam, axis=1) != 0).any(), (name, channel)
    _frozen(views, members, lone, conn, wt, mb_fam, mb_lone, W0, W, im_fam, im_lone)
    return dict(scenes=s["route"], views=views, members=members, lone=lone, conn=conn, n_active=n_active, wt=wt, mb_fam=mb_fam,
                mb_lone=mb_lone, W0=W0, W=W, im_fam=im_fam, im_lone=im_lone, h=h, w=w, M=M, eta=IM_ETA, channel=channel)


def assert_channels_differ(name):
    """Within a configuration the channels' expected mushroom scores, trained weights and Infomax scores differ pairwise."""
    chans = CONFIGS[name]["channels"]
    for i, a in enumerate(chans):
        for b in chans[i + 1:]:
            da, db = data(name, a), data(name, b)
            assert not np.array_equal(da["mb_fam"], db["mb_fam"]) and not np.array_equal(da["mb_lone"], db["mb_lone"]), (name, a, b)
            assert not np.array_equal(da["wt"], db["wt"]), (name, a, b)
            assert not np.array_equal(da["im_fam"], db["im_fam"]) and not np.array_equal(da["im_lone"], db["im_lone"]), (name, a, b)
            assert not np.array_equal(da["W"], db["W"]), (name, a, b)


def im_discrepancies(name, channel):
    """(W, d) of the float64 restatement against longdouble and against a permuted order, the larger of each, relative -- the figures
    the tolerance rule of helpers_infomax takes (scores on the SAME weights, as the GPU test takes them)."""
    d = data(name, channel)
    chain = HI.chain_discrepancy(d["W0"], d["views"], d["W"], d["eta"])
    planes = np.concatenate([d["members"].reshape(-1, d["h"], d["w"]), d["lone"]])
    want = np.concatenate([d["im_fam"].reshape(-1), d["im_lone"]])
    score = max(float(np.max(np.abs(HI.familiarity(d["W"], planes, **kw) - want)) / np.max(np.abs(want)))
                for kw in (dict(dtype=np.longdouble), dict(order_seed=99)))
    return chain, score


# ---- flags -------------------------------------------------------------------------------------------------------------------------------
def is_off(name, x, y, angle):
    """Does the HOST sensor model raise IndexError at the pose?"""
    try:
        host_scenes(name, x, y, angle)
    except IndexError:
        return True
    return False


def flag_facts(name):
    """At FLAG_AT[name] the footprint stays on the landscape at 0, 90, 180 and 270 degrees and leaves it at the four diagonals."""
    x, y = FLAG_AT[name]
    _host_sensor(name)._check_bounds((x, y))                                            # (the agent's own bounds test passes there)
    assert [is_off(name, x, y, np.deg2rad(a)) for a in SAFE_DEG] == [False] * 4, name
    assert [is_off(name, x, y, np.deg2rad(a)) for a in OFF_DEG] == [True] * 4, name


def safe_angles(n, seed):
    """n headings within SAFE_JITTER degrees of the four safe ones, all distinct."""
    rng = np.random.default_rng(seed)
    deg = np.array(SAFE_DEG)[np.arange(n) % 4] + rng.uniform(-SAFE_JITTER, SAFE_JITTER, n)
    return np.deg2rad(deg % 360.0)


def _checked_planes(name, xs, ys, angs, off, channel=2):
    """uint8[n, A, h, w]: the host model's compared planes of a layout; the poses in `off` (a set of (member, heading)) must raise
    IndexError -- their plane stays 0 and is never compared -- and every other pose must not."""
    w, h = CONFIGS[name]["sensor"]
    n, A = angs.shape
    out = np.zeros((n, A, h, w), dtype=np.uint8)
    for i in range(n):
        for a in range(A):
            if (i, a) in off:
                assert is_off(name, xs[i], ys[i], angs[i, a]), (name, i, a)
            else:
                out[i, a] = host_scenes(name, xs[i], ys[i], angs[i, a])[0, ..., channel]
    return out


def clear_margin(row, planes):
    """best_margin of a row of Infomax scores whose equal maxima, if any, are byte-identical planes (nearest-neighbour sensing gives two
    headings a fraction of a degree apart the same bytes, and a column's score depends on its bytes alone): the lead over the best
    DIFFERENT value."""
    row = np.asarray(row)
    best = int(np.argmax(row))
    ties = row == row[best]
    assert all(np.array_equal(p, planes[best]) for p in np.asarray(planes)[ties])
    return float((row[best] - row[~ties].max()) / abs(row[best]))


def _layout(name, xs, ys, angs, off):
    """One flag layout: the poses, the same poses with every off heading replaced by a safe one (`clean`), the host planes of both (an
    off pose's plane is 0 and never compared), the statements on them, the expected flags and which columns are compared (`keep`)."""
    d = data(name, 2)
    n, A = angs.shape
    clean = angs.copy()
    for k, (i, a) in enumerate(sorted(off)):
        clean[i, a] = safe_angles(1, 900 + k)[0]
    planes, planes_clean = _checked_planes(name, xs, ys, angs, off), _checked_planes(name, xs, ys, clean, set())
    keep = np.ones((n, A), dtype=bool)
    for i, a in off:
        keep[i, a] = False
    flags = np.array([0 if keep[i].all() else SENSE_ERROR for i in range(n)], dtype=np.uint32)
    out = dict(xs=xs, ys=ys, angs=angs, clean=clean, keep=keep, flags=flags, off=sorted(off), planes=planes, planes_clean=planes_clean,
               mb_fam=mb_scores(d["wt"], planes, d["conn"], d["n_active"]), mb_clean=mb_scores(d["wt"], planes_clean, d["conn"], d["n_active"]),
               im_fam=im_scores(d["W"], planes), im_clean=im_scores(d["W"], planes_clean))
    for model in ("mb", "im"):
        fam = out[model + "_fam"]
        # the best heading of every unflagged member, and of every member of the clean call, is the statement's first maximum
        out[model + "_best"] = np.array([int(np.argmax(fam[i])) if flags[i] == 0 else -1 for i in range(n)])
        out[model + "_best_clean"] = np.argmax(out[model + "_clean"], axis=1)
        for i in range(n):
            assert len(np.unique(out[model + "_clean"][i])) > 1, (name, model, i)
    for i in range(n):
        for row, pl, need in ((out["im_clean"][i], planes_clean[i], True), (out["im_fam"][i], planes[i], flags[i] == 0)):
            if need:
                assert clear_margin(row, pl) >= MARGIN, (name, i, clear_margin(row, pl))
    _frozen(*[v for v in out.values() if isinstance(v, np.ndarray)])
    return out


@functools.lru_cache(maxsize=None)
def flag_layouts(name, model):
    """dict(corners, trips) of a flag group for `model` ("mb" / "im"; the layouts differ in the width of `trips` alone).

    corners: five members x 9 headings.  Members 0..3 stand at FLAG_AT, every heading safe but one, at the diagonal of 45 + 90 i degrees,
    in column 2 i + 1: four different corners of the footprint leave the landscape.  Member 4 stands on the route and is not flagged.
    trips: three members at FLAG_AT x 260 headings (mb: k_mb_decide_batch takes 256 a trip) or 70 (im: k_im_decide takes 64).  Member
    0: only its LAST heading is off (the column before member 1's first); member 1: none; member 2: only heading 257 (65) is off, a
    column of the second trip."""
    flag_facts(name)
    x, y = FLAG_AT[name]
    path = route()
    A = 9
    xs, ys = np.array([x] * 4 + [path[20][0] + 0.4]), np.array([y] * 4 + [path[20][1] - 0.7])
    angs = np.stack([safe_angles(A, 100 + i) for i in range(4)] + [(3.0 + np.linspace(-np.pi / 2, np.pi / 2, A)) % (2 * np.pi)])
    off = set()
    for i in range(4):
        angs[i, 2 * i + 1] = np.deg2rad(OFF_DEG[i])
        off.add((i, 2 * i + 1))
    corners = _layout(name, xs, ys, angs, off)
    assert corners["flags"].tolist() == [SENSE_ERROR] * 4 + [0]
    A, late = (260, 257) if model == "mb" else (70, 65)
    angs = np.stack([safe_angles(A, 200 + i) for i in range(3)])
    angs[0, A - 1] = np.deg2rad(OFF_DEG[1])
    angs[2, late] = np.deg2rad(OFF_DEG[2])
    trips = _layout(name, np.full(3, x), np.full(3, y), angs, {(0, A - 1), (2, late)})
    assert trips["flags"].tolist() == [SENSE_ERROR, 0, SENSE_ERROR] and len(np.unique(angs)) == 3 * A
    return dict(corners=corners, trips=trips)


# ---- agent level ---------------------------------------------------------------------------------------------------------------------------
AGENT = dict(name="px", channel=1, mb=dict(n_kc=1043, fan_in=8, sparsity=0.02, seed=6), im=dict(learning_rate=IM_ETA, seed=9, n_hidden=20))


def start_poses(path):
    """Four start poses beside the route."""
    out = []
    for k, (dx, dy, da) in zip((3, 10, 18, 26), ((0.7, -0.4, 0.1), (-0.5, 0.6, -0.2), (0.3, 0.9, 0.15), (-0.8, -0.3, -0.1))):
        d = path[k + 1] - path[k]
        out.append(((float(path[k][0] + dx), float(path[k][1] + dy)), float((np.arctan2(d[1], d[0]) + da) % (2 * np.pi))))
    return out
