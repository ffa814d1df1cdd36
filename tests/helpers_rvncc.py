"""Inputs of the NCC route-view tests (tests/test_rvncc_host.py, tests/test_gpu_rvncc.py), THE STATEMENT of the metric and the NumPy
restatement of what the scoring kernel does.

Nothing here comes from the device.  For a patch plane a and a stored view b of P uint8 pixels, in exact (Python) integers

    Sa = sum a   Sb = sum b   Saa = sum a^2   Sbb = sum b^2   Sab = sum a b
    num = P Sab - Sa Sb      Va = P Saa - Sa^2      Vb = P Sbb - Sb^2
    q   = 0.0                                                              if Va == 0 or Vb == 0
    q   = clip(float64(num) / sqrt(float64(Va) * float64(Vb)), -1.0, 1.0)  otherwise

one IEEE double product, one square root, one quotient, in that order.  A step keeps per heading the largest q over the views of the
member's route and the least view that attains it; a scene call per view the least q over the member's headings.

`kernel_statement` restates k_rvncc_score of csrc/dejavu_rvncc.inl: the operands a - 128 with an int32 GEMM accumulator, the sums over
P pixels only, the int64 epilogue, the padding views of a route masked by index and the order of the pairs (q, view)."""
import functools

import numpy as np

from tests.helpers_rvssd import (TILE, GROUPS_PER_BLOCK, TILES_PER_LAUNCH, EDGE_BYTES, GEOMETRIES, GEOMETRY_LENGTHS, first_of, planes_u8,  # noqa: F401
                                 _freeze, tail_case, edge_byte_case, extreme_case, lengths_case, tie_case, geometry_case, Recorder)
from tests import helpers_rvssd as HV


def ncc_pair(a, b):
    """THE STATEMENT on one pair of equally shaped uint8 arrays -> float (a Python float is an IEEE double)."""
    a = [int(v) for v in np.asarray(a).reshape(-1)]
    b = [int(v) for v in np.asarray(b).reshape(-1)]
    P = len(a)
    Sa, Sb = sum(a), sum(b)
    Saa, Sbb, Sab = sum(v * v for v in a), sum(v * v for v in b), sum(u * v for u, v in zip(a, b))
    num, Va, Vb = P * Sab - Sa * Sb, P * Saa - Sa * Sa, P * Sbb - Sb * Sb
    if Va == 0 or Vb == 0:
        return 0.0
    assert max(abs(num), Va, Vb) < 2 ** 53                                                # the conversions below are exact
    q = np.float64(num) / np.sqrt(np.float64(Va) * np.float64(Vb))
    return float(min(max(q, np.float64(-1.0)), np.float64(1.0)))


def ncc_rows(lib, pats, channel):
    """float64[A, L]: the statement on every (patch, view) of `channel`, vectorised in int64 (held to ncc_pair by the CPU test).
    lib uint8[L, h, w, 3], pats uint8[A, h, w, 3]."""
    L, A = len(lib), len(pats)
    v = lib[..., channel].reshape(L, -1).astype(np.int64)
    p = pats[..., channel].reshape(A, -1).astype(np.int64)
    P = v.shape[1]
    Sa, Saa, Sb, Sbb = p.sum(axis=1), (p * p).sum(axis=1), v.sum(axis=1), (v * v).sum(axis=1)
    num = P * (p @ v.T) - Sa[:, None] * Sb[None, :]
    Va, Vb = P * Saa - Sa * Sa, P * Sbb - Sb * Sb
    return _epilogue(num, Va, Vb)


def _epilogue(num, Va, Vb):
    """q float64[A, L] from int64 num[A, L], Va[A], Vb[L]: the product, the square root, the quotient, the clip, 0.0 where a variance is 0."""
    den = np.sqrt(Va.astype(np.float64)[:, None] * Vb.astype(np.float64)[None, :])
    dead = (Va == 0)[:, None] | (Vb == 0)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.clip(num.astype(np.float64) / den, -1.0, 1.0)
    q[dead] = 0.0
    return q


def expected(views, first, patches, routes, channel):
    """Per member on its own route's views -> (ncc float64[n, A] the largest q, view int64[n, A] the least index that attains it, best
    int32[n] the first largest heading, scene: list of float64[len] with the least q over the headings per view)."""
    n, A = patches.shape[:2]
    ncc, view, best, scene = np.empty((n, A)), np.empty((n, A), dtype=np.int64), np.empty(n, dtype=np.int32), []
    for i in range(n):
        rows = ncc_rows(views[first[routes[i]]:first[routes[i] + 1]], patches[i], channel)
        ncc[i], view[i] = rows.max(axis=1), rows.argmax(axis=1)                           # (argmax: the first, so the least index)
        best[i] = int(np.argmax(ncc[i]))
        scene.append(rows.min(axis=0))
    return ncc, view, best, scene


def kernel_statement(lib, pats, channel):
    """k_rvncc_score and k_rvncc_pick on one route in NumPy -> (q float64[A], view int64[A], rows float64[A, L]: every live pair's q).
    lib uint8[L, h, w, 3], pats uint8[A, h, w, 3]."""
    L, A = len(lib), len(pats)
    P = lib.shape[1] * lib.shape[2]
    Pw, Kp = (P + 3) // 4, (P + 31) // 32
    Lpad = (L + 63) // 64 * 64
    plane = np.zeros((Lpad, Pw * 4), dtype=np.uint8)                                      # the store's plane: 0 beyond P and beyond L
    plane[:L, :P] = lib[..., channel].reshape(L, P)
    b = np.zeros((Lpad, Kp * 32), dtype=np.int64)                                         # dwords q >= Pw are not loaded: 0
    b[:, :Pw * 4] = (plane ^ 0x80).view(np.int8)                                          # (a zero byte of the plane is -128 here)
    a = np.zeros((A, Kp * 32), dtype=np.int64)                                            # pixels past P are 0 in the patch operand
    a[:, :P] = (pats[..., channel].reshape(A, P) ^ 0x80).view(np.int8)
    acc = a @ b.T                                                                         # [A, Lpad]: the int8 GEMM, int32 on the device
    assert np.abs(acc).max() < 2 ** 31
    acc = acc.astype(np.int32).astype(np.int64)
    vs = plane[:, :P].astype(np.int64) - 128                                              # the sums over the P pixels only
    ps = pats[..., channel].reshape(A, P).astype(np.int64) - 128
    sb, sbb, sa, saa = vs.sum(axis=1), (vs * vs).sum(axis=1), ps.sum(axis=1), (ps * ps).sum(axis=1)
    assert max(np.abs(sb).max(), np.abs(sa).max()) < 2 ** 31 and max(sbb.max(), saa.max()) < 2 ** 32    # an int and an unsigned each
    num = P * acc - sa[:, None] * sb[None, :]                                             # int64 from here
    Va, Vb = P * saa - sa * sa, P * sbb - sb * sb
    q = _epilogue(num, Va, Vb)
    q[:, L:] = -np.inf                                                                    # the padding views, masked by index
    out_q, out_v = np.empty(A), np.empty(A, dtype=np.int64)
    for col in range(A):                                                                  # the pairs (q, view): larger q, then lesser view --
        bq, bv = -np.inf, 0x7fffffff                                                      # per view group first, then the groups in order
        for g in range(Lpad // 64):
            gq, gv = -np.inf, 0x7fffffff
            for f in range(64 * g, 64 * g + 64):
                if f < L and (q[col, f] > gq or (q[col, f] == gq and f < gv)):
                    gq, gv = q[col, f], f
            if gq > bq:
                bq, bv = gq, gv
        out_q[col], out_v[col] = bq, bv
    return out_q, out_v, q[:, :L]


def ssd_first_min(lib, pats, channel):
    """int64[A]: the SSD statement's first least view (helpers_rvssd.ssd_rows)."""
    return HV.ssd_rows(lib, pats, channel).argmin(axis=1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------
def with_want(c, channels=(2,)):
    """An SSD case's inputs with the NCC expectations per channel."""
    return dict(views=c["views"], first=c["first"], patches=c["patches"], routes=c["routes"],
                want={ch: expected(c["views"], c["first"], c["patches"], c["routes"], ch) for ch in channels})


@functools.lru_cache(maxsize=None)
def ncc_tail_case(h, w):
    return with_want(tail_case(h, w), (0, 1, 2))


@functools.lru_cache(maxsize=None)
def ncc_edge_byte_case():
    return with_want(edge_byte_case())


@functools.lru_cache(maxsize=None)
def ncc_geometry_case(name):
    return with_want(geometry_case(name))


@functools.lru_cache(maxsize=None)
def ncc_extreme_case():
    """64 x 64 (P = 4096, the store's limit), one route of 3 views: alternating 0 / 255, its complement, random bytes; one member with the
    alternating plane, its complement and a constant as headings.  The largest sums: exactly 1.0 and -1.0."""
    alt = np.zeros((64, 64, 3), dtype=np.uint8)
    alt[:, ::2] = 255
    views = np.stack([alt, 255 - alt, planes_u8(11, (64, 64, 3))])
    patches = np.stack([alt, 255 - alt, np.full((64, 64, 3), 255, dtype=np.uint8)])[None]
    first, routes = first_of((3,)), np.array([0], dtype=np.int32)
    want = expected(views, first, patches, routes, 2)
    assert want[0][0].tolist() == [1.0, 1.0, 0.0] and want[1][0].tolist() == [0, 1, 0] and want[2][0] == 0
    assert want[3][0][0] == -1.0 and want[3][0][1] == -1.0                                 # the scene's minima: each against its complement
    return _freeze(dict(views=views, first=first, patches=patches, routes=routes, want={2: want}))


GAIN_K, GAIN_SEED = 9, 273                                   # (the seed: the first of np.random.default_rng(0 ...) at which SSD misses view k)


@functools.lru_cache(maxsize=None)
def gain_case():
    """A route of 70 views at 7 x 5, random in [0, 120]; the patch is 2 * view_k + 7 (no clipping): NCC finds view k with exactly 1.0.
    The SSD statement's first minimum on the same store and patch is another view (the CPU test asserts it for GAIN_SEED)."""
    views = np.random.default_rng(GAIN_SEED).integers(0, 121, size=(70, 7, 5, 3), dtype=np.uint8)
    patches = (2 * views[GAIN_K].astype(np.int64) + 7).astype(np.uint8)[None, None]
    assert patches.max() <= 247
    first, routes = first_of((70,)), np.array([0], dtype=np.int32)
    want = expected(views, first, patches, routes, 2)
    return _freeze(dict(views=views, first=first, patches=patches, routes=routes, want={2: want}))


def _negative_route(seed, L, h=5, w=5):
    """L views that all correlate NEGATIVELY with the returned patch: view = 255 - (a noisy copy of the patch)."""
    rng = np.random.default_rng(seed)
    patch = rng.integers(40, 216, size=(h, w, 3), dtype=np.uint8)
    noise = rng.integers(-12, 13, size=(L, h, w, 3))
    views = (255 - np.clip(patch.astype(np.int64)[None] + noise, 0, 255)).astype(np.uint8)
    return patch, views


@functools.lru_cache(maxsize=None)
def constant_case():
    """One route of 6 views that all correlate negatively with heading 1's patch, view 4 constant; headings: a constant patch, that
    patch.  The constant patch: a row of 0.0, view 0.  The other: the constant view wins with 0.0 at its own index, 4."""
    patch, views = _negative_route(51, 6)
    views[4] = 77
    patches = np.stack([np.full_like(patch, 200), patch])[None]
    first, routes = first_of((6,)), np.array([0], dtype=np.int32)
    want = expected(views, first, patches, routes, 2)
    return _freeze(dict(views=views, first=first, patches=patches, routes=routes, want={2: want}))


@functools.lru_cache(maxsize=None)
def negative_case():
    """A route of 65 views (63 padding views in its second group) that all correlate negatively with the patch: the best q is < 0, and a
    padding view, whose Vb is 0, would score 0.0 and win."""
    patch, views = _negative_route(52, 65)
    patches = patch[None, None]
    first, routes = first_of((65,)), np.array([0], dtype=np.int32)
    want = expected(views, first, patches, routes, 2)
    return _freeze(dict(views=views, first=first, patches=patches, routes=routes, want={2: want}))


NCC_LENGTHS = (2, 33, 64, 65, 130, 300)                      # (a route holds at least 2 views: the store refuses 1)


@functools.lru_cache(maxsize=None)
def ncc_lengths_case():
    """Routes of NCC_LENGTHS views at 5 x 5 (300: a second block of four view groups), a member per route in shuffled route order, two
    headings; every route's last view is heading 0's patch under a gain and an offset: exactly 1.0 at the route's last view."""
    first = first_of(NCC_LENGTHS)
    views = planes_u8(61, (int(first[-1]), 5, 5, 3))
    patches = planes_u8(62, (len(NCC_LENGTHS), 2, 5, 5, 3))
    routes = np.array([3, 5, 0, 4, 1, 2], dtype=np.int32)
    for i, r in enumerate(routes):
        patches[i, 0] = patches[i, 0] // 4 + 20                                           # in [20, 83]
        views[first[r + 1] - 1] = 3 * patches[i, 0] + 2                                   # in [62, 251]: no clipping
    want = expected(views, first, patches, routes, 2)
    return _freeze(dict(views=views, first=first, patches=patches, routes=routes, want={2: want}))


@functools.lru_cache(maxsize=None)
def ncc_tie_case():
    """A route of 300 views at 6 x 6 with one view stored at indices 5 and 290 (another group and another block), behind a decoy route;
    headings: a worse patch, then the stored view twice.  The least view and the first heading win."""
    views = planes_u8(71, (4 + 300, 6, 6, 3))
    patch = planes_u8(72, (6, 6, 3))
    views[4 + 5] = views[4 + 290] = patch
    patches = np.stack([planes_u8(73, (6, 6, 3)), patch, patch])[None]
    first, routes = first_of((4, 300)), np.array([1], dtype=np.int32)
    want = expected(views, first, patches, routes, 2)
    return _freeze(dict(views=views, first=first, patches=patches, routes=routes, want={2: want}))


@functools.lru_cache(maxsize=None)
def members_case(n, A):
    """n members x A headings at 7 x 5 over geometry_case's routes (7, 70, 3, 129 and 40 views), the members' routes in shuffled order
    (7 members: five on route 1 and two on route 3, so that a tile of 32 columns ends inside a member)."""
    first = first_of(GEOMETRY_LENGTHS)
    views = planes_u8(41, (int(first[-1]), 7, 5, 3))
    patches = planes_u8(80 + n * A, (n, A, 7, 5, 3))
    routes = np.array([(1, 3, 1, 1, 3, 1, 1)[i % 7] if n == 7 else (3 * i + 1) % 5 for i in range(n)], dtype=np.int32)
    want = expected(views, first, patches, routes, 2)
    return _freeze(dict(views=views, first=first, patches=patches, routes=routes, want={2: want}))


LAUNCH_EDGE_MEMBERS = TILES_PER_LAUNCH + 1                   # 32 769


def plan_tiles(routes, A):
    """rvssd_plan of csrc/dejavu_rvssd.inl in NumPy -> [(first sorted column, columns, route)]: the members sorted by route (stable),
    their columns cut into tiles of at most TILE columns of ONE route (a tile may hold columns of several members)."""
    order = np.argsort(np.asarray(routes), kind="stable")
    col_route = np.repeat(np.asarray(routes)[order], A)
    tiles, s = [], 0
    while s < len(col_route):
        e = s + 1
        while e < len(col_route) and e - s < TILE and col_route[e] == col_route[s]:
            e += 1
        tiles.append((s, e - s, int(col_route[s])))
        s = e
    return tiles


@functools.lru_cache(maxsize=None)
def many_members_case():
    """32 769 members x 1 heading at 7 x 5 on a route of 3 views: 1025 tiles of one route, the last of ONE column."""
    n = LAUNCH_EDGE_MEMBERS
    views = planes_u8(90, (3, 7, 5, 3))
    patches = planes_u8(91, (n, 1, 7, 5, 3))
    first, routes = first_of((3,)), np.zeros(n, dtype=np.int32)
    rows = ncc_rows(views, patches[:, 0], 2)                                              # [n, 3]
    want = (rows.max(axis=1)[:, None], rows.argmax(axis=1)[:, None].astype(np.int64), np.zeros(n, dtype=np.int32), rows)
    return _freeze(dict(views=views, first=first, patches=patches, routes=routes, want=want))


@functools.lru_cache(maxsize=None)
def launch_edge_case():
    """32 769 members x 1 heading at 2 x 2, every member on a route of its own (32 769 routes of 2 views, in shuffled order): a tile is
    of one route, so there are 32 769 tiles and the last is a launch of its own -> want = (ncc[n, 1], view[n, 1], best[n], q[n, 2])."""
    n = LAUNCH_EDGE_MEMBERS
    rng = np.random.default_rng(92)
    views = rng.integers(0, 256, size=(2 * n, 2, 2, 3), dtype=np.uint8)
    first = first_of([2] * n)
    patches = rng.integers(0, 256, size=(n, 1, 2, 2, 3), dtype=np.uint8)
    routes = rng.permutation(n).astype(np.int32)
    p = patches[:, 0, :, :, 2].reshape(n, -1).astype(np.int64)
    P = p.shape[1]
    q = np.empty((n, 2))
    for k in range(2):
        v = views[2 * routes.astype(np.int64) + k][..., 2].reshape(n, -1).astype(np.int64)
        num = P * (p * v).sum(axis=1) - p.sum(axis=1) * v.sum(axis=1)
        Va, Vb = P * (p * p).sum(axis=1) - p.sum(axis=1) ** 2, P * (v * v).sum(axis=1) - v.sum(axis=1) ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            q[:, k] = np.clip(num.astype(np.float64) / np.sqrt(Va.astype(np.float64) * Vb.astype(np.float64)), -1.0, 1.0)
        q[(Va == 0) | (Vb == 0), k] = 0.0
    want = (q.max(axis=1)[:, None], q.argmax(axis=1)[:, None].astype(np.int64), np.zeros(n, dtype=np.int32), q)
    return _freeze(dict(views=views, first=first, patches=patches, routes=routes, want=want))
