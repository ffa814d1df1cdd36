"""Inputs of the sensor-noise tests (tests/test_noise_host.py, tests/test_gpu_noise.py) and the NumPy statement of the noise.

The statement (include/dejavu.h, "noise rows").  A sensed pose that belongs to noise row (key, amp_s, amp_v), heading a of its member,
sensor pixel j = bi w + bj, P = w h, uint64 arithmetic that wraps:
    base = splitmix64(key + seed GOLDEN)         word = splitmix64(base + (a P + j))
    d_S  = word & 0xFFFFFFFF, d_V = word >> 32   n_c = ((d_c (2 amp_c + 1)) >> 32) - amp_c
    S'   = clamp(S + n_S, 0, 255), V' likewise
on the sensor pixel's S and V after the pixel block's rule (agent.downscale_chem) and before the level tables; the hue is the noiseless
model's; the level tables and the mask follow.  Nothing here comes from the device: a view is agent.fill_sensor_from and
agent.downscale_chem on the pose's own landscape, the draws of synth.splitmix64, the agent's own _level_tables.  Where host sensing of
every pose would be slow (SLAB: 8256 poses of 32 x 32) the sensor has 256 levels and no mask, so the level tables are the identity and
the noiseless device views (lands_sense, held to the host model by tests/test_gpu_lands.py) are S and V: noise_on_views.

Landscapes (lands()): 151 x 131 and 140 x 170 parts of two synthetic landscapes -- different shapes, the first of an odd byte count.
Every pose lies in BOX, where the largest footprint of these tests (66 x 62 landscape pixels, 33 x 31 sensor pixels of 2 x 2) stays on
both landscapes at any heading.

What the CPU test asserts of these inputs (so that a passing GPU test is not vacuous) is stated beside each function."""
import functools
import types

import numpy as np

from navsim_amd import synth
from navsim_amd.agent import NavBySceneFamiliarity, downscale_chem, fill_sensor_from

GOLDEN = synth.GOLDEN
MASK32 = np.uint64(0xFFFFFFFF)
BOX = (47.0, 84.0, 47.0, 93.0)                              # x0, x1, y0, y1

# sensor configurations: sensor (w, h), pixel (pw, ph), the levels of V (H and S keep 256), mask_middle_n
THIN = dict(sensor=(7, 5), pixel=(1, 1), levels=16, mask=0)           # P = 35: a wavefront spans poses of different rows
THIN_A = dict(sensor=(7, 5), pixel=(1, 1), levels=4, mask=1)          # ... its two table entries
THIN_B = dict(sensor=(7, 5), pixel=(2, 2), levels=6, mask=0)
WIDE = dict(sensor=(16, 8), pixel=(1, 2), levels=3, mask=0)           # the engine's own configuration beside the table below
WIDE_A = dict(sensor=(16, 8), pixel=(2, 4), levels=4, mask=2)         # the reference's 16 x 8 sensor
WIDE_B = dict(sensor=(16, 8), pixel=(1, 1), levels=5, mask=0)
BIG = dict(sensor=(33, 31), pixel=(1, 1), levels=5, mask=0)           # 1023 pixels: a thread of the mushroom kernels senses four
BIG_A = dict(sensor=(33, 31), pixel=(1, 1), levels=7, mask=3)
BIG_B = dict(sensor=(33, 31), pixel=(2, 2), levels=4, mask=0)
PLAIN32 = dict(sensor=(32, 32), pixel=(1, 1), levels=256, mask=0)     # identity level tables, no mask (SLAB)
ROWS5 = ((0, 0), (1, 0), (0, 255), (255, 255), (20, 3))               # (amp_s, amp_v) of the rows, in turn
SEED = 0x1234_5678_9ABC_DEF1


@functools.lru_cache(maxsize=None)
def lands():
    a = np.ascontiguousarray(synth.synth_landscape(21, 300, 4)[:151, :131])
    b = np.ascontiguousarray(synth.synth_landscape(23, 300, 4)[:140, :170])
    assert a.shape == (151, 131, 3) and b.shape == (140, 170, 3) and a.size % 2 == 1
    for l in (a, b):
        l.setflags(write=False)
    return (a, b)


def level_table(cfg):
    """uint8[3, 256]: the agent's own level arithmetic on the configuration's levels."""
    return NavBySceneFamiliarity._level_tables(types.SimpleNamespace(n_sensor_levels=(256, 256, int(cfg["levels"]))))


def table_args(cfgs):
    """(pixel_dimensions, luts, masks) of FamiliarityEngine.sensors_set."""
    return [c["pixel"] for c in cfgs], np.stack([level_table(c) for c in cfgs]), [c["mask"] for c in cfgs]


# ---- the statement -----------------------------------------------------------------------------------------------------------------------
def train_key(route, view):
    """A route ensemble's key of training view `view` of route `route`."""
    return ((0x80000000 | int(route)) << 32) | int(view)


def step_key(stream, count):
    """... and of a member's device step number `count` (from 0)."""
    return (int(stream) << 32) | int(count)


def counters(a, P):
    """uint64[P]: the counters of heading a's pixels."""
    return np.uint64(a) * np.uint64(P) + np.arange(P, dtype=np.uint64)


def draws(seed, key, a, P, amp_s, amp_v):
    """(n_S, n_V) int64[P]: the integers added to S and V of the P pixels of heading `a` under (seed, key)."""
    with np.errstate(over="ignore"):
        base = synth.splitmix64(np.uint64(key) + np.uint64(seed) * GOLDEN)
        word = synth.splitmix64(base + counters(a, P))
        d_s, d_v = word & MASK32, word >> np.uint64(32)
        n_s = ((d_s * np.uint64(2 * int(amp_s) + 1)) >> np.uint64(32)).astype(np.int64) - int(amp_s)
        n_v = ((d_v * np.uint64(2 * int(amp_v) + 1)) >> np.uint64(32)).astype(np.int64) - int(amp_v)
    return n_s, n_v


def add_noise(raw, seed, key, a, amp_s, amp_v):
    """uint8[h, w, 3]: `raw` (a view before its level tables) with the draws added to S and V and clamped; the hue is raw's."""
    h, w = raw.shape[:2]
    n_s, n_v = draws(seed, key, a, h * w, amp_s, amp_v)
    out = raw.copy()
    out[..., 1] = np.clip(raw[..., 1].astype(np.int64) + n_s.reshape(h, w), 0, 255)
    out[..., 2] = np.clip(raw[..., 2].astype(np.int64) + n_v.reshape(h, w), 0, 255)
    return out


def raw_view(land, cfg, x, y, angle):
    """uint8[h, w, 3]: the sensor pixels after the block rule, before the level tables (IndexError where the footprint leaves `land`)."""
    (w, h), (pw, ph) = cfg["sensor"], cfg["pixel"]
    buf = np.empty((h * ph, w * pw, 3), dtype=np.uint8)
    fill_sensor_from(buf, float(x), float(y), float(angle), land)
    return downscale_chem(buf, ph, pw)


def finish(raw, cfg):
    """The level tables, then the mask."""
    lut = level_table(cfg)
    out = np.stack([lut[ch][raw[..., ch]] for ch in range(3)], axis=-1)
    mid = out.shape[1] // 2
    out[:, mid - cfg["mask"]:mid + cfg["mask"]] = 0
    return out


def view(land, cfg, x, y, angle, seed=0, key=0, a=0, amp_s=0, amp_v=0):
    """The statement for one pose."""
    return finish(add_noise(raw_view(land, cfg, x, y, angle), seed, key, a, amp_s, amp_v), cfg)


def views(cfgs, x, y, angle, land_of, seed, keys, amp_s, amp_v, per=1):
    """uint8[n per, h, w, 3]: the statement for the n per poses of a call, member-major: pose t belongs to row t // per (its landscape
    land_of[t // per], its configuration cfgs[land_of[...]] where cfgs is a list, else cfgs) and is heading t % per of it."""
    L = lands()
    out = []
    for t in range(len(x)):
        i, a = divmod(t, per)
        l = int(land_of[i])
        cfg = cfgs[l] if isinstance(cfgs, (list, tuple)) else cfgs
        out.append(view(L[l], cfg, x[t], y[t], angle[t], seed, int(keys[i]), a, int(amp_s[i]), int(amp_v[i])))
    return np.stack(out)


def member_views(cfgs, xs, ys, angs, land_of, seed, keys, amp_s, amp_v):
    """uint8[n, A, h, w, 3]: views() for n members at (xs[i], ys[i]) looking along angs[i, :]."""
    n, A = np.shape(angs)
    flat = views(cfgs, np.repeat(xs, A), np.repeat(ys, A), np.reshape(angs, -1), land_of, seed, keys, amp_s, amp_v, per=A)
    return flat.reshape((n, A) + flat.shape[1:])


def noise_on_views(noiseless, seed, keys, amp_s, amp_v):
    """uint8[n, A, h, w, 3]: the statement on noiseless views of a sensor whose level tables are the identity and that has no mask
    (its views ARE the raw S and V), vectorised over members and headings.  Asserted (CPU): equal to add_noise view by view."""
    v = np.asarray(noiseless)
    n, A, h, w = v.shape[:4]
    P = h * w
    with np.errstate(over="ignore"):
        base = synth.splitmix64(np.asarray(keys, dtype=np.uint64) + np.uint64(seed) * GOLDEN)
        word = synth.splitmix64(base[:, None, None] + (np.arange(A, dtype=np.uint64)[None, :, None] * np.uint64(P) +
                                                       np.arange(P, dtype=np.uint64)[None, None, :]))
        s_amp = np.asarray(amp_s, dtype=np.uint64)[:, None, None]
        v_amp = np.asarray(amp_v, dtype=np.uint64)[:, None, None]
        n_s = (((word & MASK32) * (np.uint64(2) * s_amp + np.uint64(1))) >> np.uint64(32)).astype(np.int64) - s_amp.astype(np.int64)
        n_v = (((word >> np.uint64(32)) * (np.uint64(2) * v_amp + np.uint64(1))) >> np.uint64(32)).astype(np.int64) - v_amp.astype(np.int64)
    out = v.copy()
    out[..., 1] = np.clip(v[..., 1].astype(np.int64) + n_s.reshape(n, A, h, w), 0, 255)
    out[..., 2] = np.clip(v[..., 2].astype(np.int64) + n_v.reshape(n, A, h, w), 0, 255)
    return out


# ---- poses and rows ----------------------------------------------------------------------------------------------------------------------
def poses(seed, n):
    """(x, y, angle) float64[n] inside BOX."""
    rng = np.random.default_rng(seed)
    return rng.uniform(BOX[0], BOX[1], n), rng.uniform(BOX[2], BOX[3], n), rng.uniform(0, 2 * np.pi, n)


def rows(seed, n):
    """(keys uint64[n] that use all 64 bits, amp_s, amp_v int[n]: ROWS5 in turn)."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    keys[0] |= np.uint64(1 << 63)
    if n > 1:
        keys[1] &= np.uint64((1 << 63) - 1)
    amp = [ROWS5[i % len(ROWS5)] for i in range(n)]
    return keys, np.array([a for a, _ in amp]), np.array([b for _, b in amp])


@functools.lru_cache(maxsize=None)
def sense_case(name):
    """Test 1 ("thin": THIN on both landscapes) and test 2 ("wide": the table WIDE_A, WIDE_B): 11 poses dealt over the two landscapes,
    rows ROWS5 in turn -> dict(cfgs, x, y, angle, land_of, keys, amp_s, amp_v, noisy, plain).
    Asserted: the rows of zero amplitude give the noiseless views, every other row changes its view; wide: the outputs lie on the
    entry's levels, and the masked columns are 0 in the rows of amplitude 255."""
    cfgs = {"thin": THIN, "wide": [WIDE_A, WIDE_B]}[name]
    n = 11
    x, y, ang = poses(101, n)
    land_of = np.array([0, 1, 1, 0, 1, 0, 0, 1, 0, 1, 1], dtype=np.int32)
    keys, amp_s, amp_v = rows(102, n)
    noisy = views(cfgs, x, y, ang, land_of, SEED, keys, amp_s, amp_v)
    plain = views(cfgs, x, y, ang, land_of, SEED, keys, np.zeros(n, int), np.zeros(n, int))
    for v in range(n):
        assert np.array_equal(noisy[v], plain[v]) == (amp_s[v] == 0 and amp_v[v] == 0), (name, v)
    for a in (x, y, ang, land_of, keys, amp_s, amp_v, noisy, plain):
        a.setflags(write=False)
    return dict(cfgs=cfgs, x=x, y=y, angle=ang, land_of=land_of, keys=keys, amp_s=amp_s, amp_v=amp_v, noisy=noisy, plain=plain)


# ---- the mushroom body: training and the banked step ----------------------------------------------------------------------------------------
MB = dict(n_kc=301, fan_in=4, n_active=7, seed=71, channel=2)
MB_SHAPES = {"thin": (THIN, [THIN_A, THIN_B], 3, 3), "big": (BIG, [BIG_A, BIG_B], 5, 2)}    # own, table, members, headings
N_BANKS = 2


def mb_conn(shape):
    from tests import helpers_mushroom as H
    w, h = MB_SHAPES[shape][0]["sensor"]
    return H.connectivity(MB["n_kc"], w * h, MB["fan_in"], MB["seed"])


@functools.lru_cache(maxsize=None)
def mb_train_case(shape, table):
    """Nine training views dealt over the two banks and the two landscapes, rows ROWS5 in turn -> dict(cfgs, x, y, angle, bank_of,
    land_of, keys, amp_s, amp_v, views (the statement), wts uint8[2, K] (the mushroom statement trained on them), plain_wts (trained on
    the noiseless views).  Asserted: the noise changes both banks."""
    from tests import helpers_mushroom as H
    own, tab = MB_SHAPES[shape][:2]
    cfgs = tab if table else own
    n = 9
    x, y, ang = poses(111, n)
    bank_of = np.array([0, 1, 1, 0, 1, 0, 0, 1, 0], dtype=np.int32)
    land_of = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1], dtype=np.int32)
    keys, amp_s, amp_v = rows(112, n)
    noisy = views(cfgs, x, y, ang, land_of, SEED, keys, amp_s, amp_v)
    plain = views(cfgs, x, y, ang, land_of, SEED, keys, np.zeros(n, int), np.zeros(n, int))
    conn = mb_conn(shape)
    ones = np.ones(MB["n_kc"], np.uint8)
    ch = MB["channel"]
    wts = np.stack([H.train(ones, np.ascontiguousarray(noisy[bank_of == b][..., ch]), conn, MB["n_active"]) for b in range(N_BANKS)])
    plain_wts = np.stack([H.train(ones, np.ascontiguousarray(plain[bank_of == b][..., ch]), conn, MB["n_active"]) for b in range(N_BANKS)])
    assert all((wts[b] != plain_wts[b]).any() for b in range(N_BANKS)), shape
    return dict(cfgs=cfgs, x=x, y=y, angle=ang, bank_of=bank_of, land_of=land_of, keys=keys, amp_s=amp_s, amp_v=amp_v, views=noisy, wts=wts,
                plain_wts=plain_wts, conn=conn)


@functools.lru_cache(maxsize=None)
def mb_step_case(shape, table):
    """MB_SHAPES' members x headings under mb_train_case's banks -> dict(xs, ys, angs, banks, lands, keys, amp_s, amp_v, planes (the
    statement's noised views), fam float64[n, A], best int[n]; plain_fam: the statement on the noiseless views).
    Asserted: the noise changes the scores."""
    from tests import helpers_mushroom_ensemble as HE
    own, tab, n, A = MB_SHAPES[shape]
    cfgs = tab if table else own
    t = mb_train_case(shape, table)
    xs, ys, _ = poses(121, n)
    angs = np.random.default_rng(122).uniform(0, 2 * np.pi, (n, A))
    banks = np.array([1, 0, 1, 1, 0][:n], dtype=np.int32)
    land_of = np.array([0, 1, 1, 0, 1][:n], dtype=np.int32)
    keys, amp_s, amp_v = rows(123, n)
    amp_s, amp_v = amp_s[::-1].copy(), amp_v[::-1].copy()      # (member 0 is not the zero row)
    ch = MB["channel"]

    def score(planes):
        d = np.stack([HE.novelty(t["wts"][banks[i]], np.ascontiguousarray(planes[i][..., ch]), t["conn"], MB["n_active"]) for i in range(n)])
        return (-d).astype(np.float64)
    planes = member_views(cfgs, xs, ys, angs, land_of, SEED, keys, amp_s, amp_v)
    plain = member_views(cfgs, xs, ys, angs, land_of, SEED, keys, np.zeros(n, int), np.zeros(n, int))
    fam, plain_fam = score(planes), score(plain)
    assert not np.array_equal(fam, plain_fam), shape
    return dict(cfgs=cfgs, xs=xs, ys=ys, angs=angs, banks=banks, lands=land_of, keys=keys, amp_s=amp_s, amp_v=amp_v, planes=planes, fam=fam,
                best=np.argmax(fam, axis=1), plain_fam=plain_fam)


# ---- Infomax: a small step, and helpers_inet.SLAB's layout ------------------------------------------------------------------------------------
IM = dict(n_hidden=6, seed=131, channel=2)


def im_weights(n_banks, N, M=None):
    """float64[n_banks, M, N]: distinct finite weights, bank by bank (the step is compared between two device paths, bit for bit)."""
    rng = np.random.default_rng(IM["seed"])
    return rng.normal(0.0, 1.0 / np.sqrt(N), (n_banks, M or IM["n_hidden"], N))


@functools.lru_cache(maxsize=None)
def im_step_case():
    """5 members x 3 headings at THIN under three banks whose order is not the members' -> dict(xs, ys, angs, banks, lands, keys, amp_s,
    amp_v, planes uint8[n, A, h, w, 3]: the statement).  Asserted: the sort by bank permutes the members."""
    n, A = 5, 3
    xs, ys, _ = poses(141, n)
    angs = np.random.default_rng(142).uniform(0, 2 * np.pi, (n, A))
    banks = np.array([2, 0, 1, 0, 2], dtype=np.int32)
    land_of = np.array([0, 1, 1, 0, 1], dtype=np.int32)
    assert (np.argsort(banks, kind="stable") != np.arange(n)).any()
    keys, amp_s, amp_v = rows(143, n)
    planes = member_views(THIN, xs, ys, angs, land_of, SEED, keys, amp_s, amp_v)
    return dict(xs=xs, ys=ys, angs=angs, banks=banks, lands=land_of, keys=keys, amp_s=amp_s, amp_v=amp_v, planes=planes)


@functools.lru_cache(maxsize=None)
def slab_case():
    """helpers_inet.SLAB's 688 members x 12 headings of 32 x 32 views in its scrambled caller's order: the second launch of the banked
    step begins at column 8176, inside a member -> dict(xs, ys, angs, banks, lands, keys, amp_s, amp_v, lay).  The members stand at 16
    places; every member has a key and amplitudes of its own.  Asserted (CPU): the cut, and that the rows of the members of launch 2
    differ from those of the members at their launch-local places."""
    from tests import helpers_inet as HN
    lay = HN.slab_layout()
    n, A = len(lay["banks"]), lay["A"]
    px, py, _ = poses(151, 16)
    heads = np.random.default_rng(152).uniform(0, 2 * np.pi, (16, A))
    at = np.arange(n) % 16
    rng = np.random.default_rng(153)
    keys = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    amp_s, amp_v = rng.integers(0, 256, n), rng.integers(0, 256, n)
    land_of = (np.arange(n) % 3 == 1).astype(np.int32)
    return dict(xs=px[at], ys=py[at], angs=heads[at], banks=lay["banks"], lands=land_of, keys=keys, amp_s=amp_s, amp_v=amp_v, lay=lay)


# ---- the view store ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def store_case():
    """Two routes of 5 and 70 views (route 0 on landscape 1, route 1 on landscape 0) at THIN, their views under rows of their own, and
    3 members x 3 headings -> dict(x, y, angle, first, land_of_view, tkeys, tamp_s, tamp_v, views (the statement); xs, ys, angs, routes,
    lands, weights, keys, amp_s, amp_v, patches (the statement), win_lo, win_hi).  Members 1 and 2 stand on views 20 and 50 of route 1,
    turned a little, so their windows hold their match."""
    n = 75
    x, y, ang = poses(161, n)
    first = np.array([0, 5, 75], dtype=np.int64)
    land_of_view = np.array([1] * 5 + [0] * 70, dtype=np.int32)
    tkeys, tamp_s, tamp_v = rows(162, n)
    tamp_s, tamp_v = np.minimum(tamp_s, 12), np.minimum(tamp_v, 12)
    v = views(THIN, x, y, ang, land_of_view, SEED, tkeys, tamp_s, tamp_v)
    routes = np.array([0, 1, 1], dtype=np.int32)
    lands_m = np.array([1, 0, 0], dtype=np.int32)
    at = [2, 5 + 20, 5 + 50]
    xs, ys = x[at] + 0.3, y[at] - 0.2
    angs = (ang[at][:, None] + np.array([-0.5, 0.0, 0.4])[None, :]) % (2 * np.pi)
    keys, amp_s, amp_v = rows(163, 3)
    amp_s, amp_v = np.array([20, 0, 3]), np.array([3, 30, 255])
    patches = member_views(THIN, xs, ys, angs, lands_m, SEED, keys, amp_s, amp_v)
    return dict(x=x, y=y, angle=ang, first=first, land_of_view=land_of_view, tkeys=tkeys, tamp_s=tamp_s, tamp_v=tamp_v, views=v, xs=xs, ys=ys,
                angs=angs, routes=routes, lands=lands_m, weights=np.array([0.25, 0.0, 0.5]), keys=keys, amp_s=amp_s, amp_v=amp_v,
                patches=patches, win_lo=np.array([0, 10, 30], dtype=np.int32), win_hi=np.array([5, 40, 70], dtype=np.int32))


# ---- ensembles ---------------------------------------------------------------------------------------------------------------------------------
ENS = dict(sensor=(8, 6), pixel=(1, 1), levels=16, mask=0)  # (V steps of 17: an amplitude above 8 shows after the level table)
ENS_ANGLES, ENS_STEP = 5, 1.0
ENS_NOISE = dict(seed=77, amp_s=0, amp_v=[40, 40, 25, 60], train_amp_s=0, train_amp_v=[0, 12], streams=[5, 9, 2, 7])


def ens_routes():
    """[(landscape_index, route)]: route 0 on landscape 0, route 1 on landscape 1, inside BOX."""
    k = np.arange(16, dtype=np.float64)
    r0 = np.stack([50.0 + k, 58.0 + 3.0 * np.sin(k / 4.0)], axis=1)
    k = np.arange(14, dtype=np.float64)
    r1 = np.stack([60.0 + 0.8 * k, 52.0 + 0.6 * k], axis=1)
    return [(0, r0), (1, r1)]


def ens_starts():
    """Four starts: members 0 and 1 are the SAME pose on route 0 (under different streams), members 2 and 3 stand on route 1."""
    routes = ens_routes()
    p0, p1 = routes[0][1], routes[1][1]
    return [(0, (float(p0[3][0]), float(p0[3][1] + 0.4)), 0.2), (0, (float(p0[3][0]), float(p0[3][1] + 0.4)), 0.2),
            (1, (float(p1[2][0] + 0.3), float(p1[2][1])), 0.7), (1, (float(p1[6][0]), float(p1[6][1] - 0.5)), 0.5)]


def route_headings(route):
    steps = route[1:] - route[:-1]
    h = np.arctan2(steps[:, 1], steps[:, 0])
    return h[np.minimum(np.arange(len(route)), len(route) - 2)]


@functools.lru_cache(maxsize=None)
def ens_train_views():
    """[uint8[n_r, h, w, 3]]: the statement's views of the routes under the training keys and ENS_NOISE's training amplitudes."""
    out = []
    for r, (l, route) in enumerate(ens_routes()):
        hd = route_headings(route)
        out.append(np.stack([view(lands()[l], ENS, route[v][0], route[v][1], hd[v], ENS_NOISE["seed"], train_key(r, v), 0,
                                  ENS_NOISE["train_amp_s"], ENS_NOISE["train_amp_v"][r]) for v in range(len(route))]))
    return out


def angle_offsets(n=ENS_ANGLES, saccade_degrees=180.0):
    half = saccade_degrees / 2
    return np.linspace(-(np.pi * half / 180.0), np.pi * half / 180.0, n)


def shadow(member, steps, channel=2, noise=None):
    """A NumPy agent of SsdRouteEnsemble's member `member` of ens_starts() under ENS_NOISE: the statement's patches at its headings,
    SSD in int64 against its route's statement views, the first maximum, the agent's move (noise: ENS_NOISE, or a dict of its shape
    with other recall amplitudes) -> a list per step of dict(x, y, angles,
    patches uint8[A, h, w, 3], fam float64[A], best, position, angle)."""
    noise = noise or ENS_NOISE
    r, pos, ang = ens_starts()[member]
    l = ens_routes()[r][0]
    memory = ens_train_views()[r][..., channel].astype(np.int64)
    out = []
    for t in range(steps):
        angles = (ang + angle_offsets()) % (2 * np.pi)
        key = step_key(noise["streams"][member], t)
        patches = np.stack([view(lands()[l], ENS, pos[0], pos[1], angles[a], noise["seed"], key, a, noise["amp_s"], noise["amp_v"][member])
                            for a in range(len(angles))])
        d = patches[:, None, :, :, channel].astype(np.int64) - memory[None]
        fam = -(d * d).sum(axis=(2, 3)).min(axis=1).astype(np.float64)
        best = int(np.argmax(fam))
        x, y = pos
        ang = angles[best]
        pos = (pos[0] + ENS_STEP * np.cos(ang), pos[1] + ENS_STEP * np.sin(ang))
        out.append(dict(x=x, y=y, angles=angles, patches=patches, fam=fam, best=best, position=pos, angle=ang))
    return out


ENS_MB = dict(n_kc=300, fan_in=4, sparsity=0.03, seed=5)    # MushroomRouteEnsemble's model in these tests


def mushroom_first_row(member):
    """float64[A]: the mushroom statement on the first step's statement patches of member `member` (shadow's: the patches of a step
    are the sensor's, whatever scores them), under its route's bank trained on the statement's views."""
    from navsim_amd.util import mushroom_connectivity
    from tests import helpers_mushroom as H
    r = ens_starts()[member][0]
    w, h = ENS["sensor"]
    conn = mushroom_connectivity(ENS_MB["n_kc"], w * h, ENS_MB["fan_in"], ENS_MB["seed"])
    n_active = max(1, int(round(ENS_MB["sparsity"] * ENS_MB["n_kc"])))
    wt = H.train(np.ones(ENS_MB["n_kc"], np.uint8), np.ascontiguousarray(ens_train_views()[r][..., 2]), conn, n_active)
    return H.familiarity(wt, np.ascontiguousarray(shadow(member, 1)[0]["patches"][..., 2]), conn, n_active)


# ---- a fake engine: the ensembles' arguments are refused before any of its calls ---------------------------------------------------------------
class FakeEngine(object):
    """Records noise_rows / noise_clear and refuses everything else: what from_landscapes must not reach with bad arguments."""

    def __init__(self):
        self.calls = []

    def noise_rows(self, seed, keys, amp_s, amp_v):
        self.calls.append(("noise_rows", int(seed), np.array(keys, dtype=np.uint64), list(amp_s), list(amp_v)))

    def noise_clear(self):
        self.calls.append(("noise_clear",))

    def __getattr__(self, name):
        raise AssertionError("engine call %s after arguments that must be refused" % name)
