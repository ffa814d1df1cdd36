"""NumPy restatement of the mushroom-body familiarity model (include/dejavu.h: dv_mb_*) and the inputs of its tests.

The model, literally.  N = h*w pixels; p = a view's uint8[h,w] plane flattened in C order; conn = int32[K, c] drawn as
np.random.default_rng(seed).integers(0, N, (K, c)) (a pixel repeated in a row counts twice); wt = uint8[K], all 1 at first.

    a_k   = sum_j p[conn[k, j]]                                  integers, at most 255 c
    fired = np.argsort(-a, kind="stable")[:n_active]             larger a first, then lower k
    train:  wt[fired] = 0          score:  d = sum(wt[fired])    familiarity = float64(-d): the INTEGER is negated, a trained view is +0.0

Everything is an integer, so the device is held to this file bit for bit: np.array_equal everywhere, floats through their uint64
view (bits), no tolerance.  The tie rule is the model, not a corner of it: route_views has five grey levels, so `a` takes a few dozen
values and in every case the threshold value is shared by more cells than there are places left (tests/test_mushroom_host.py).

CASES are the smallest shapes at which the kernels can still go wrong (see the column `reaches`), and one that is not small: 256x256,
the only plane whose pixel indices need all 16 bits of the device's connectivity.  Three conditions are asserted here,
on the CPU, so that no test passes on a kernel that zeroes everything or selects nothing: at most half the weights are 0 after training
(but for all_fire), every training view scores 0, and every case but 40x1_k300 (one winner: d is 0 or 1; it does score a 1) and all_fire
(one view depresses every cell, so every d is 0: the GPU test scores it on fresh weights too, where d = K) scores a patch with d > 0.
Zero fraction after training, measured with this file: 5x3_k37 0.19, 40x1_k300 0.12, 16x16_k1043 0.21, 7x5_k20000 0.25,
33x31_k4100_c16 0.06, 128x128_k2049 0.09, 20x13_k257_half 0.50 (128 of 257), 256x256_k1043_c16 0.06.  A fourth condition holds the
widest case to its purpose: with every index cut to 15 bits (conn & 0x7fff) each of its patches fires another set of cells.

Outside CASES, because the three conditions do not apply to them (they are for masks and fresh scores, or for two views repeated):
LONG_QUOTA -- constant and two-level planes under quotas that run past wave 0's first 64 cells and past its whole span; the SLAB_*
inputs -- two distinct views, repeated on the device's side only, that carry a call across the view bound and the byte bound of a
launch (slab_views); SLAB_POSES and circle_angles -- poses and headings for the same through the sensor (host_sensed_planes: the host
sensor model, byte-equal to the device's).  tests/test_mushroom_host.py asserts what each of them must distinguish.
"""
import functools
import os
import re

import numpy as np

from tests.helpers_infomax import route_views, bits, sensed_route  # noqa: F401  (shared inputs)

CASES = {
    # sensor (w, h), cells, fan-in, firing cells, views trained, patches scored                     reaches
    "5x3_k37": dict(w=5, h=3, K=37, c=10, n_active=4, F=2, A=1, seed=37),                          # K below one wave; c close to N: repeats
    "40x1_k300": dict(w=40, h=1, K=300, c=3, n_active=1, F=37, A=16, seed=32),                     # one winner, always from the tie bin
    "16x16_k1043": dict(w=16, h=16, K=1043, c=8, n_active=21, F=12, A=65, seed=33),                # ragged K; more than 64 headings
    "7x5_k20000": dict(w=7, h=5, K=20000, c=10, n_active=200, F=30, A=5, seed=34),                 # the default K: many trips; N % 4 != 0
    "33x31_k4100_c16": dict(w=33, h=31, K=4100, c=16, n_active=41, F=6, A=17, seed=35),            # the widest histogram (4081 bins); odd N
    "128x128_k2049": dict(w=128, h=128, K=2049, c=10, n_active=64, F=3, A=3, seed=36),             # the largest plane in LDS; K = 8*256 + 1
    "20x13_all_fire": dict(w=20, h=13, K=300, c=5, n_active=300, F=1, A=4, seed=39),               # n_active = K
    "20x13_k257_half": dict(w=20, h=13, K=257, c=1, n_active=128, F=1, A=9, seed=38),              # c = 1; tie bin far wider than the quota
    "256x256_k1043_c16": dict(w=256, h=256, K=1043, c=16, n_active=21, F=3, A=3, seed=40),         # 65536 pixels: 16-bit indices; most LDS
}
CONSTANT_KEYS = ("16x16_k1043", "33x31_k4100_c16")

# Quotas that are not used up inside wave 0's first trip, on 16x16_k1043's connectivity (K = 1043: a wave's span is 320 cells, five
# trips of 64): one past the first trip, a whole span, one past it, into the third wave, near K, and all but one cell.
LONG_QUOTA = dict(key="16x16_k1043", n_active=(65, 320, 321, 700, 1000, 1042))

# Two views repeated across a launch's bounds (slab_views).  SLAB_TRAIN: 128x128 planes, where the staged BYTES end a training or
# scoring launch (64 MiB / 16384 = 4096 views, below the view bound).  SLAB_ACTIVITY: 7x5_k20000's first two patches, where the fired
# masks (20000 bytes a view) end an activity launch.  SLAB_POSES: a small model on the 32x32 sensor of helpers_infomax.SENSED; two
# poses of sensed_route() for training from poses, two headings at `xy_offset` from the route's eighth point for the agent's step.
SLAB_TRAIN = dict(key="128x128_k2049", seed=78)
SLAB_ACTIVITY = dict(key="7x5_k20000")
SLAB_POSES = dict(K=300, c=4, n_active=6, seed=50, poses=(0, 30), angles=(0.4, 2.0), at=7, xy_offset=(0.6, -0.3))


def connectivity(K, N, c, seed):
    return np.random.default_rng(seed).integers(0, N, (K, c))


def activity(planes, conn):
    """int64[n, K]: a_k of each of uint8[n,h,w] planes."""
    planes = np.asarray(planes)
    p = planes.reshape(len(planes), int(np.prod(planes.shape[1:]))).astype(np.int32)
    return p[:, conn].sum(axis=-1, dtype=np.int64)


def fired_sets(planes, conn, n_active):
    """int64[n, n_active]: the firing cells of each plane, in the order of the model."""
    a = activity(planes, conn)
    return np.array([np.argsort(-row, kind="stable")[:n_active] for row in a], dtype=np.int64).reshape(len(a), n_active)


def fired_mask(planes, conn, n_active):
    """(uint8[n, K] with 1 where the cell fires, int32[n]: the least activity of a firing cell)."""
    a = activity(planes, conn)
    f = fired_sets(planes, conn, n_active)
    mask = np.zeros(a.shape, dtype=np.uint8)
    np.put_along_axis(mask, f, 1, axis=1)
    thr = np.take_along_axis(a, f, axis=1).min(axis=1).astype(np.int32)
    return mask, thr


def train(wt, planes, conn, n_active):
    """The weights after training on uint8[n,h,w] planes (a new array)."""
    wt = np.array(wt, dtype=np.uint8)
    for f in fired_sets(planes, conn, n_active):
        wt[f] = 0
    return wt


def novelty(wt, planes, conn, n_active):
    """int64[n]: d of each plane."""
    return np.array([int(np.asarray(wt)[f].sum()) for f in fired_sets(planes, conn, n_active)], dtype=np.int64)


def familiarity(wt, planes, conn, n_active):
    """float64[n]: -d, the integer negated and then converted (so 0 stays +0.0)."""
    return (-novelty(wt, planes, conn, n_active)).astype(np.float64)


def constant_planes(h, w):
    """uint8[3,h,w]: all 0, all 255, and 0 / 255 in halves of the flattened plane."""
    halves = np.zeros(h * w, dtype=np.uint8)
    halves[(h * w) // 2:] = 255
    return np.ascontiguousarray(np.stack([np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8), halves.reshape(h, w)]))


def tie_counts(planes, conn, n_active):
    """Per plane: (cells above the threshold, cells at it)."""
    a = activity(planes, conn)
    _, thr = fired_mask(planes, conn, n_active)
    return [(int((row > t).sum()), int((row == t).sum())) for row, t in zip(a, thr)]


@functools.lru_cache(maxsize=None)
def case_data(key):
    """The inputs of a case and the restatement on them, computed once: dict(views, patches, conn, wt, mask, thr, fam, d)."""
    c = CASES[key]
    N = c["w"] * c["h"]
    views = route_views(c["seed"], c["F"], c["h"], c["w"])
    patches = np.ascontiguousarray(np.concatenate([route_views(c["seed"] + 100, c["A"], c["h"], c["w"]), views[:1]]))
    conn = connectivity(c["K"], N, c["c"], c["seed"])
    wt = train(np.ones(c["K"], np.uint8), views, conn, c["n_active"])
    mask, thr = fired_mask(patches, conn, c["n_active"])
    d = novelty(wt, patches, conn, c["n_active"])
    fam = familiarity(wt, patches, conn, c["n_active"])
    for a in (views, patches, conn, wt, mask, thr, d, fam):
        a.setflags(write=False)
    # the three conditions (module docstring)
    if key != "20x13_all_fire":
        assert 0 < int((wt == 0).sum()) <= (c["K"] + 1) // 2, key
    assert not novelty(wt, views, conn, c["n_active"]).any(), key
    assert d[-1] == 0 and fam[-1] == 0.0 and not np.signbit(fam[-1]), key
    if key not in ("40x1_k300", "20x13_all_fire"):
        assert d.max() > 0, key
    if N > 32768:
        # the fourth: a 15-bit index is another model for every patch
        low, _ = fired_mask(patches, conn & 0x7fff, c["n_active"])
        assert (conn >= 32768).mean() > 0.4 and (low != mask).any(axis=1).all(), key
    return dict(c, N=N, views=views, patches=patches, conn=conn, wt=wt, mask=mask, thr=thr, d=d, fam=fam)


@functools.lru_cache(maxsize=None)
def constant_data(key):
    """CONSTANT_KEYS: the constant and two-level planes under the case's connectivity and trained weights."""
    d = case_data(key)
    planes = constant_planes(d["h"], d["w"])
    mask, thr = fired_mask(planes, d["conn"], d["n_active"])
    fam = familiarity(d["wt"], planes, d["conn"], d["n_active"])
    # a constant plane excites every cell alike: exactly the cells 0 .. n_active-1 fire
    first = np.zeros(d["K"], np.uint8)
    first[:d["n_active"]] = 1
    assert np.array_equal(mask[0], first) and np.array_equal(mask[1], first) and thr[0] == 0 and thr[1] == 255 * d["c"]
    for a in (planes, mask, thr, fam):
        a.setflags(write=False)
    return dict(planes=planes, mask=mask, thr=thr, fam=fam)


def wave_span(K):
    """Cells of one wave of k_mb: K / 4 rounded up, then up to a multiple of 64."""
    return (((K + 3) // 4) + 63) & ~63


@functools.lru_cache(maxsize=None)
def quota_data(n_active):
    """LONG_QUOTA: constant_planes under the case's connectivity with n_active firing cells: dict(planes, conn, mask, thr, K, c)."""
    d = case_data(LONG_QUOTA["key"])
    planes = constant_planes(d["h"], d["w"])
    mask, thr = fired_mask(planes, d["conn"], n_active)
    first = np.zeros(d["K"], np.uint8)
    first[:n_active] = 1
    assert np.array_equal(mask[0], first) and np.array_equal(mask[1], first) and thr[0] == 0 and thr[1] == 255 * d["c"]
    for a in (planes, mask, thr):
        a.setflags(write=False)
    return dict(planes=planes, conn=d["conn"], mask=mask, thr=thr, K=d["K"], c=d["c"], h=d["h"], w=d["w"], n_active=n_active)


def chosen_equals(plane, conn, n_active):
    """The cells of ONE plane that fire with a_k equal to the threshold -- those the rank arithmetic chooses -- in index order."""
    a = activity(plane[None], conn)[0]
    mask, thr = fired_mask(plane[None], conn, n_active)
    return np.flatnonzero((a == thr[0]) & (mask[0] == 1))


@functools.lru_cache(maxsize=None)
def slab_train_data():
    """SLAB_TRAIN: dict(two uint8[2,h,w], conn, n_active, K, N, h, w, both, first): the weights after both views and after view 0."""
    d = case_data(SLAB_TRAIN["key"])
    two = route_views(SLAB_TRAIN["seed"], 2, d["h"], d["w"])
    ones = np.ones(d["K"], np.uint8)
    both = train(ones, two, d["conn"], d["n_active"])
    first = train(ones, two[:1], d["conn"], d["n_active"])
    for a in (two, both, first):
        a.setflags(write=False)
    return dict(two=two, conn=d["conn"], n_active=d["n_active"], K=d["K"], N=d["N"], h=d["h"], w=d["w"], both=both, first=first)


@functools.lru_cache(maxsize=None)
def _host_sensor():
    from tests import helpers_infomax as HI

    def keep(scenes):
        def func(scene, fambuf):
            fambuf[...] = 0.0
        func.max_familiarity = 0.0
        return func
    return HI.sensed_agent(keep, False)


def host_sensed_planes(x, y, angles):
    """uint8[n,32,32]: the V planes the HOST sensor model takes at (x[i], y[i], angles[i]) on helpers_infomax.SENSED's landscape."""
    agent = _host_sensor()
    x, y, angles = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(angles, np.float64))
    return np.ascontiguousarray(np.stack([agent.get_sensor_mat((xi, yi), ai) for xi, yi, ai in zip(x, y, angles)])[..., 2])


def route_headings(path):
    """The heading of every view of a training path, as the agent takes them: towards the next point, the last one again."""
    steps = path[1:] - path[:-1]
    headings = np.arctan2(steps[:, 1], steps[:, 0])
    return headings[np.minimum(np.arange(len(path)), len(path) - 2)]


def step_xy():
    """Where the sense-step tests stand: off the route, beside its eighth point."""
    return tuple(sensed_route()[SLAB_POSES["at"]] + np.array(SLAB_POSES["xy_offset"]))


def circle_angles(n):
    """n distinct headings over the full circle."""
    return (0.4 + np.arange(n) * (2 * np.pi / n)) % (2 * np.pi)


def slab_views():
    """Views of one training launch, read from the kernel file (kMbSlabViews), and the bytes of planes it may stage."""
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(os.path.dirname(here), "navigation-by-deja-vu_amd", "csrc", "dejavu_mushroom.inl")).read()
    views = int(re.search(r"kMbSlabViews\s*=\s*(\d+)\s*;", src).group(1))
    stage = re.search(r"kMbStageBytes\s*=\s*(\d+)u\s*<<\s*(\d+)\s*;", src)
    return views, int(stage.group(1)) << int(stage.group(2))


def numpy_model(channel=2, n_kc=20000, fan_in=10, sparsity=0.01, seed=0):
    """The statement as a familiarity plug-in of the reference's shape, with no engine: the agent runs its generic loop over func."""
    n_active = max(1, int(round(sparsity * n_kc)))

    def model(scenes):
        planes = np.ascontiguousarray(np.asarray(scenes)[..., channel])
        conn = connectivity(n_kc, planes.shape[1] * planes.shape[2], fan_in, seed)
        wt = train(np.ones(n_kc, np.uint8), planes, conn, n_active)

        def func(scene, fambuf):
            fambuf[...] = familiarity(wt, np.asarray(scene)[None, ..., channel], conn, n_active)[0]
        func.max_familiarity = 0.0
        func.wt = wt
        return func
    return model
