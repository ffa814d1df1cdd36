"""Inputs of the bank-set tests of the mushroom-body model (tests/test_mbset_host.py, tests/test_gpu_mbset.py) and the statement of
the set read-out in NumPy, on tests/helpers_mushroom.py's fired_mask.  Nothing here comes from the device.

The statement (include/dejavu.h, "bank sets").  Member i of a step carries banks[i][0..S) and int32 coefs[i][0..S).  For its column a
with fired mask F (helpers_mushroom.fired_mask: the model's own selection),
    d_j = sum_k F[k] * wt[banks[i][j]][k]        v = sum_j coefs[i][j] * d_j        angle_familiarity[i][a] = float64(-v)
and best[i] is np.argmax of the row: the first maximum.  Integers, so every comparison is np.array_equal, the scores on their bits.

Models.  SHAPES["7x5"]: 130 cells at fan-in 3, 7 firing -- a wave's span is 64 cells, so wave 2 owns two cells and wave 3 none (the
hand-over of the wave totals has empty waves).  SHAPES["33x31"]: 20 000 cells at fan-in 10, 200 firing (79 trips a wave, odd N).
N_BANKS = 5 banks, bank b trained on the views v with v % 5 == b of a route of 10.

Sets (set_tables): for S in SET_SIZES the coefficients are COEF_POOL in turn from a member's own offset (negatives and 0 among them),
the banks walk the five banks with a member's own stride, and from S = 2 on every odd member enters its first bank again as its last.
conditions() is what tests/test_mbset_host.py asserts of every GPU input, so that no GPU test passes on a read-out that takes the
entries in another order, drops the last one, or (683 x 12) takes the table at the launch's own column.

The opponent ensemble's shadow (numpy_opponent_model) is an agent with the host sensor model whose familiarity plug-in holds two NumPy
memories; the agent's own generic loop moves it."""
import functools

import numpy as np

from tests import helpers_mushroom as H

N_BANKS = 5
MAX_BANKS = 8
SET_SIZES = (1, 2, 3, 8)
SHAPES = {"7x5": dict(w=7, h=5, K=130, c=3, n_active=7, seed=201), "33x31": dict(w=33, h=31, K=20000, c=10, n_active=200, seed=202)}
LAYOUT = (4, 5)                                             # members x headings of test 1
COEF_POOL = (3, -2, 1, 0, -1, 5, 2, -4, 7)
WIDE_LAYOUT = (683, 12)                                     # 8196 columns: the second launch begins at column 8192, inside member 682
TIE_LAYOUT = (2, 260)
TIE_KEY = "16x16_k1043"


def readout(mask, wts, banks, coefs, A):
    """(nov int64[n, A, S], v int64[n, A]) of fired masks uint8[n A, K] under weights uint8[n_banks, K]."""
    banks, coefs = np.asarray(banks, dtype=np.int64), np.asarray(coefs, dtype=np.int64)
    n, S = banks.shape
    d_all = mask.astype(np.int64) @ np.asarray(wts).astype(np.int64).T                  # [n A, n_banks]
    nov = np.take_along_axis(d_all.reshape(n, A, -1), np.broadcast_to(banks[:, None, :], (n, A, S)), axis=2)
    return nov, (nov * coefs[:, None, :]).sum(axis=2)


def statement(planes, wts, conn, n_active, banks, coefs):
    """dict(nov int32[n, A, S], fam float64[n, A], best int[n]) of uint8[n, A, h, w] planes."""
    n, A = planes.shape[:2]
    mask, _ = H.fired_mask(planes.reshape((n * A,) + planes.shape[2:]), conn, n_active)
    return finish(mask, wts, banks, coefs, A)


def finish(mask, wts, banks, coefs, A):
    nov, v = readout(mask, wts, banks, coefs, A)
    assert np.abs(v).max() < 2 ** 31
    fam = (-v).astype(np.float64)
    return dict(nov=nov.astype(np.int32), fam=fam, best=np.argmax(fam, axis=1))


def set_tables(n, S):
    """(banks, coefs) int32[n, S]."""
    banks = np.array([[(i + j * (1 + i % 3)) % N_BANKS for j in range(S)] for i in range(n)], dtype=np.int32)
    coefs = np.array([[COEF_POOL[(2 * i + j) % len(COEF_POOL)] for j in range(S)] for i in range(n)], dtype=np.int32)
    if S >= 2:
        banks[1::2, -1] = banks[1::2, 0]                                                 # a bank entered twice
    return banks, coefs


@functools.lru_cache(maxsize=None)
def model(shape):
    """dict(conn, wts uint8[5, K], views, + the shape's values): five banks trained on different views of one route."""
    m = SHAPES[shape]
    conn = H.connectivity(m["K"], m["w"] * m["h"], m["c"], m["seed"])
    views = H.route_views(m["seed"], 2 * N_BANKS, m["h"], m["w"])
    ones = np.ones(m["K"], np.uint8)
    wts = np.stack([H.train(ones, views[b::N_BANKS], conn, m["n_active"]) for b in range(N_BANKS)])
    assert all((wts[a] != wts[b]).any() for a in range(N_BANKS) for b in range(a + 1, N_BANKS)), shape
    for a in (conn, views, wts):
        a.setflags(write=False)
    return dict(m, conn=conn, wts=wts, views=views)


@functools.lru_cache(maxsize=None)
def layout_planes(shape):
    """uint8[4, 5, h, w]: novel views of another strip, with a trained view at one heading of every member."""
    m = model(shape)
    n, A = LAYOUT
    planes = H.route_views(m["seed"] + 100, n * A, m["h"], m["w"]).reshape(n, A, m["h"], m["w"]).copy()
    for i in range(n):
        planes[i, (2 * i + 1) % A] = m["views"][3 * i % len(m["views"])]
    planes.setflags(write=False)
    return planes


@functools.lru_cache(maxsize=None)
def case(shape, S):
    """Test 1's input and statement -> dict(planes, banks, coefs, nov, fam, best, mask)."""
    m = model(shape)
    planes = layout_planes(shape)
    n, A = LAYOUT
    banks, coefs = set_tables(n, S)
    mask, _ = H.fired_mask(planes.reshape(n * A, m["h"], m["w"]), m["conn"], m["n_active"])
    return dict(finish(mask, m["wts"], banks, coefs, A), planes=planes, banks=banks, coefs=coefs, mask=mask, A=A)


def conditions(mask, wts, banks, coefs, A):
    """What must differ from the statement at at least one column: the set's entries read in another order (the banks rolled by one
    under the same coefficients; S = 1: the next bank), and the last bank dropped -> (columns that differ) of each."""
    _, v = readout(mask, wts, banks, coefs, A)
    S = banks.shape[1]
    other = np.roll(banks, 1, axis=1) if S > 1 else (banks + 1) % N_BANKS
    _, v_order = readout(mask, wts, other, coefs, A)
    v_drop = readout(mask, wts, banks[:, :-1], coefs[:, :-1], A)[1] if S > 1 else np.zeros_like(v)
    return int((v_order != v).sum()), int((v_drop != v).sum())


@functools.lru_cache(maxsize=None)
def constant_case(shape, S):
    """helpers_mushroom.constant_planes (every cell ties at the threshold: the rank rule picks cells 0 .. n_active - 1) as one member
    of three headings."""
    m = model(shape)
    planes = H.constant_planes(m["h"], m["w"])[None]
    banks, coefs = set_tables(1, S)
    mask, thr = H.fired_mask(planes[0], m["conn"], m["n_active"])
    first = np.zeros(m["K"], np.uint8)
    first[:m["n_active"]] = 1
    assert np.array_equal(mask[0], first) and np.array_equal(mask[1], first)
    return dict(finish(mask, m["wts"], banks, coefs, 3), planes=planes, banks=banks, coefs=coefs, mask=mask, A=3)


@functools.lru_cache(maxsize=None)
def tie_case():
    """2 members x 260 headings, S = 2, coefficients (1, -1): an attractive and a repulsive memory at gain 1, their weights made by
    hand on three views P, Q, R so that (d_att, d_rep) is (10, 4) under P, (8, 2) under Q and (many, 0) under R.  Member 1 sees P at
    heading 5 and Q at heading 257, R elsewhere: v = 6 at both, from different pairs, and more elsewhere -- the answer is heading 5,
    and the first bank alone says 257.  Member 0 sees Q at heading 100 alone."""
    d = H.case_data(TIE_KEY)
    n, A = TIE_LAYOUT
    three = H.route_views(777, 40, d["h"], d["w"])[[0, 17, 39]]
    F = [set(f.tolist()) for f in H.fired_sets(three, d["conn"], d["n_active"])]
    only = [sorted(F[a] - F[(a + 1) % 3] - F[(a + 2) % 3]) for a in range(3)]
    assert len(only[0]) >= 10 and len(only[1]) >= 8 and len(only[2]) >= 7, [len(o) for o in only]
    att, rep = np.zeros(d["K"], np.uint8), np.zeros(d["K"], np.uint8)
    att[only[0][:10]], rep[only[0][:4]] = 1, 1
    att[only[1][:8]], rep[only[1][:2]] = 1, 1
    att[only[2]] = 1
    wts = np.stack([att, rep])
    pick = np.full((n, A), 2)
    pick[0, 100] = 1
    pick[1, 5], pick[1, 257] = 0, 1
    planes = np.ascontiguousarray(three[pick])
    banks, coefs = np.array([[0, 1], [0, 1]], np.int32), np.array([[1, -1], [1, -1]], np.int32)
    mask3, _ = H.fired_mask(three, d["conn"], d["n_active"])
    s = finish(mask3[pick.reshape(-1)], wts, banks, coefs, A)
    assert s["nov"][1, 5].tolist() == [10, 4] and s["nov"][1, 257].tolist() == [8, 2] and s["nov"][1, 0, 1] == 0 and s["nov"][1, 0, 0] > 6
    assert s["best"].tolist() == [100, 5] and np.flatnonzero(s["fam"][1] == -6.0).tolist() == [5, 257]
    assert int(np.argmin(s["nov"][1, :, 0])) == 257                                      # a decision on the first bank alone
    return dict(s, planes=planes, banks=banks, coefs=coefs, wts=wts, conn=d["conn"], n_active=d["n_active"], h=d["h"], w=d["w"], K=d["K"])


def wide_tables():
    """The 683 members' sets (S = 2) and coefficients: drawn per member, so those behind the launch's cut are not the first members'."""
    n = WIDE_LAYOUT[0]
    rng = np.random.default_rng(31)
    banks = rng.integers(0, N_BANKS, (n, 2)).astype(np.int32)
    coefs = rng.integers(-3, 4, (n, 2)).astype(np.int32)
    coefs[coefs == 0] = 2
    banks[682], coefs[682] = (4, 1), (1, -2)
    banks[0], coefs[0] = (0, 2), (3, 1)
    return banks, coefs


def second_launch():
    """(first column of the second launch, the member it lies in, its heading): by kMbSlabViews of dejavu_mushroom.inl."""
    views, _ = H.slab_views()
    return (views,) + divmod(views, WIDE_LAYOUT[1])


def launch_local(banks, coefs, A):
    """The per-column tables a kernel would use that took its table at the LAUNCH's own column: (banks, coefs) int32[n A, S]."""
    c0 = second_launch()[0]
    col = np.arange(len(banks) * A)
    member = np.where(col < c0, col // A, (col - c0) // A)
    return banks[member], coefs[member]


@functools.lru_cache(maxsize=None)
def wide_case():
    """Test 5, uploaded: 683 x 12 columns drawn from a pool of 8 views of the 7x5 model -> dict(planes, banks, coefs, nov, fam, best,
    wrong: columns at which the launch-local table gives another value)."""
    m = model("7x5")
    n, A = WIDE_LAYOUT
    pool = np.concatenate([H.route_views(m["seed"] + 300, 6, m["h"], m["w"]), m["views"][:2]])
    pick = np.random.default_rng(32).integers(0, len(pool), (n, A))
    banks, coefs = wide_tables()
    mask8, _ = H.fired_mask(pool, m["conn"], m["n_active"])
    mask = mask8[pick.reshape(-1)]
    s = finish(mask, m["wts"], banks, coefs, A)
    lb, lc = launch_local(banks, coefs, A)
    _, v_local = readout(mask, m["wts"], lb, lc, 1)
    wrong = np.flatnonzero(v_local.reshape(-1) != -s["fam"].reshape(-1).astype(np.int64))
    return dict(s, planes=np.ascontiguousarray(pool[pick]), banks=banks, coefs=coefs, mask=mask, A=A, wrong=wrong)


# ---- sensed calls: helpers_noise's landscapes, configurations and statement of the sensor ------------------------------------------------
SENSED = dict(n_kc=301, fan_in=4, n_active=7, seed=71, channel=2, members=5, headings=4, S=3)


@functools.lru_cache(maxsize=None)
def sensed_model(sensor):
    """(conn, wts uint8[5, K]) for a sensor of (w, h): five banks with hand-drawn weights (half of the cells depressed, each its own)."""
    w, h = sensor
    conn = H.connectivity(SENSED["n_kc"], w * h, SENSED["fan_in"], SENSED["seed"])
    wts = (np.random.default_rng(72).integers(0, 2, (N_BANKS, SENSED["n_kc"]))).astype(np.uint8)
    return conn, wts


@functools.lru_cache(maxsize=None)
def sensed_case(kind):
    """kind in ("own", "lands", "table", "noise", "both"; "lands": the landscape set without a sensor table or noise rows, every
    member on its own landscape) -> dict(cfg (the engine's own), table (None or the set's sensor table), xs, ys, angs,
    lands (None: the engine's one landscape, helpers_noise.lands()[0]), keys / amp_s / amp_v (None without noise), views (the host
    statement of the sensor, uint8[n, A, h, w, 3]), banks, coefs, nov, fam, best).  Asserted: noise changes the scores."""
    from tests import helpers_noise as HZ
    n, A, S = SENSED["members"], SENSED["headings"], SENSED["S"]
    cfg = HZ.WIDE
    table = [HZ.WIDE_A, HZ.WIDE_B] if kind in ("table", "both") else None
    xs, ys, _ = HZ.poses(221, n)
    angs = np.random.default_rng(222).uniform(0, 2 * np.pi, (n, A))
    lands = None if kind == "own" else np.array([0, 1, 1, 0, 1], dtype=np.int32)
    noisy = kind in ("noise", "both")
    keys, amp_s, amp_v = HZ.rows(223, n)
    amp_s, amp_v = amp_s[::-1].copy(), amp_v[::-1].copy()
    zeros = np.zeros(n, int)
    land_of = np.zeros(n, np.int32) if lands is None else lands
    cfgs = table if table else cfg
    plain = HZ.member_views(cfgs, xs, ys, angs, land_of, HZ.SEED, keys, zeros, zeros)
    views = HZ.member_views(cfgs, xs, ys, angs, land_of, HZ.SEED, keys, amp_s, amp_v) if noisy else plain
    conn, wts = sensed_model(cfg["sensor"])
    banks, coefs = set_tables(n, S)
    planes = np.ascontiguousarray(views[..., SENSED["channel"]])
    s = statement(planes, wts, conn, SENSED["n_active"], banks, coefs)
    if noisy:
        assert not np.array_equal(s["fam"], statement(np.ascontiguousarray(plain[..., 2]), wts, conn, SENSED["n_active"], banks, coefs)["fam"])
    return dict(s, cfg=cfg, table=table, xs=xs, ys=ys, angs=angs, lands=lands, keys=keys if noisy else None, amp_s=amp_s, amp_v=amp_v,
                planes=planes, banks=banks, coefs=coefs, conn=conn, wts=wts)


OFF_EDGE, OFF_Y = 9.5, 70.0                                 # the pose's distance from the last column of landscape 0 (151 x 131)
OFF_ANGLES = (0.0, np.pi / 2, np.pi / 4, np.pi)


@functools.lru_cache(maxsize=None)
def off_facts():
    """Under helpers_noise.WIDE (16 x 8 sensor pixels of 1 x 2: a footprint of 16 x 16 landscape pixels, half a side 8, half a diagonal
    11.3) at OFF_EDGE from the last column, the headings of OFF_ANGLES: which of them leave landscape 0 -> (x, y, list of bool).
    Asserted: exactly one does, the diagonal one."""
    from tests import helpers_noise as HZ
    land = HZ.lands()[0]
    x, y = land.shape[1] - OFF_EDGE, OFF_Y
    off = []
    for a in OFF_ANGLES:
        try:
            HZ.raw_view(land, HZ.WIDE, x, y, a)
            off.append(False)
        except IndexError:
            off.append(True)
    assert sum(off) == 1, off
    return x, y, off


@functools.lru_cache(maxsize=None)
def wide_sensed_case():
    """Test 5, sensed: 683 x 12 on helpers_noise.THIN (7 x 5) and landscape 0: member i stands at one of four places and looks along
    twelve headings (48 host-sensed views in all) -> dict(xs, ys, angs, planes uint8[683, 12, 5, 7], banks, coefs, nov, fam, best)."""
    from tests import helpers_noise as HZ
    m = model("7x5")
    n, A = WIDE_LAYOUT
    px, py, _ = HZ.poses(231, 4)
    twelve = H.circle_angles(A)
    four = HZ.member_views(HZ.THIN, px, py, np.tile(twelve, (4, 1)), np.zeros(4, np.int32), 0, np.zeros(4, np.uint64), np.zeros(4, int),
                           np.zeros(4, int))[..., 2]
    where = np.arange(n) % 4
    banks, coefs = wide_tables()
    mask4, _ = H.fired_mask(four.reshape(4 * A, m["h"], m["w"]), m["conn"], m["n_active"])
    mask = mask4.reshape(4, A, -1)[where].reshape(n * A, -1)
    s = finish(mask, m["wts"], banks, coefs, A)
    lb, lc = launch_local(banks, coefs, A)
    _, v_local = readout(mask, m["wts"], lb, lc, 1)
    wrong = np.flatnonzero(v_local.reshape(-1) != -s["fam"].reshape(-1).astype(np.int64))
    return dict(s, xs=px[where], ys=py[where], angs=np.tile(twelve, (n, 1)), planes=np.ascontiguousarray(four[where]), banks=banks, coefs=coefs,
                wrong=wrong, mask=mask, A=A)


def overflow_bound(n_active):
    """The largest sum of |coefs| a member may carry under n_active firing cells."""
    return (2 ** 31 - 1) // int(n_active)


# ---- the opponent ensemble: a shadow agent whose sensor model and two memories run in NumPy ---------------------------------------------------
ENS_SENSOR = (12, 10)
ENS_MODEL = dict(n_kc=1043, fan_in=8, sparsity=0.02, seed=6)
ENS_ANGLES = 9


def repulsive_key(route, view):
    """The noise key of view `view` of route `route`'s repulsive bank."""
    return ((0xC0000000 | int(route)) << 32) | int(view)


def numpy_opponent_model(repulsive_scenes, gain, channel=2, n_kc=20000, fan_in=10, sparsity=0.01, seed=0):
    """helpers_mushroom.numpy_model with a second memory: a familiarity plug-in of the reference's shape, with no engine, whose value
    is -(d_att - gain d_rep) -- the attractive memory trained on the agent's familiar scenes, the repulsive one on `repulsive_scenes`
    (the same points, host-sensed at the route's headings plus the turn)."""
    n_active = max(1, int(round(sparsity * n_kc)))

    def model(scenes):
        planes = np.ascontiguousarray(np.asarray(scenes)[..., channel])
        conn = H.connectivity(n_kc, planes.shape[1] * planes.shape[2], fan_in, seed)
        ones = np.ones(n_kc, np.uint8)
        wts = np.stack([H.train(ones, planes, conn, n_active),
                        H.train(ones, np.ascontiguousarray(np.asarray(repulsive_scenes)[..., channel]), conn, n_active)])

        def func(scene, fambuf):
            mask, _ = H.fired_mask(np.asarray(scene)[None, ..., channel], conn, n_active)
            _, v = readout(mask, wts, [[0, 1]], [[1, -int(gain)]], 1)
            fambuf[...] = float(-v[0, 0])
        func.max_familiarity = 0.0
        func.wts = wts
        return func
    return model
