"""Inputs of the SSD route-view tests (tests/test_rvssd_host.py, tests/test_gpu_rvssd.py), the expected values on them and the NumPy
restatement of what the scoring kernel does.

Nothing here comes from the device.  The expected value of a (patch, view) pair is `ssd_pair`: ((p.astype(np.int64) - v) ** 2).sum()
on the compared channel, the least view index on ties -- itself held to oracle.ssds (pinned by tests/golden/t6_ssds.npz) by the CPU
test.  `kernel_statement` restates k_rvssd_score of csrc/dejavu_rvssd.inl: the operands' order with the XOR, patch pixels past P zero,
norms over P pixels only, the key ssd << 32 | view, and the padding views of a route masked by index."""
import functools

import numpy as np

TILE = 32                                       # kRvssdTile: columns of a tile at most (the MFMA's M)
GROUPS_PER_BLOCK = 4                            # kRvssdGroupsPerBlock: view groups of a scoring workgroup
TILES_PER_LAUNCH = 32768                        # kRvssdTilesPerLaunch: tiles of a scoring launch at most
MAX_SSD = 255 * 255 * 4096                      # 266 342 400: all-0 views against an all-255 patch at 64 x 64


def ssd_pair(p, v):
    """The expected value of one pair of equally shaped uint8 arrays."""
    return int(((p.astype(np.int64) - v) ** 2).sum())


def first_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def ssd_rows(lib, pats, channel):
    """int64[A, L]: ssd_pair of every (patch, view) on `channel`; lib uint8[L, h, w, 3], pats uint8[A, h, w, 3]."""
    L, A = len(lib), len(pats)
    v = lib[..., channel].reshape(L, -1).astype(np.int64)
    p = pats[..., channel].reshape(A, -1).astype(np.int64)
    out = np.empty((A, L), dtype=np.int64)
    for a in range(A):
        out[a] = ((p[a][None, :] - v) ** 2).sum(axis=1)
    return out


def expected(views, first, patches, routes, channel):
    """Per member on its own route's views -> (ssd float64[n, A], view int64[n, A] the least index, best int32[n] the first least
    heading, scene: list of float64[len] with the largest value over the headings per view)."""
    n, A = patches.shape[:2]
    ssd, view, best, scene = np.empty((n, A)), np.empty((n, A), dtype=np.int64), np.empty(n, dtype=np.int32), []
    for i in range(n):
        rows = ssd_rows(views[first[routes[i]]:first[routes[i] + 1]], patches[i], channel)
        ssd[i], view[i] = rows.min(axis=1), rows.argmin(axis=1)                           # (argmin: the first, so the least index)
        best[i] = int(np.argmin(ssd[i]))
        scene.append(rows.max(axis=0).astype(np.float64))
    return ssd, view, best, scene


def kernel_statement(lib, pats, channel):
    """k_rvssd_score on one route in NumPy -> (ssd int64[A], view int64[A]).  lib uint8[L, h, w, 3], pats uint8[A, h, w, 3]."""
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
    vnorm = ((plane[:, :P].astype(np.int64) - 128) ** 2).sum(axis=1)                      # norms over the P pixels only
    pnorm = ((pats[..., channel].reshape(A, P).astype(np.int64) - 128) ** 2).sum(axis=1)
    acc = a @ b.T                                                                         # [A, Lpad]: the int8 GEMM, int32 on the device
    assert np.abs(acc).max() < 2 ** 31
    ssd = vnorm[None, :] + pnorm[:, None] - 2 * acc
    assert ssd.min() >= 0 and ssd.max() < 2 ** 31
    key = (ssd.astype(np.uint64) << np.uint64(32)) | np.arange(Lpad, dtype=np.uint64)[None, :]
    key[:, L:] = np.uint64(0xffffffffffffffff)                                            # the padding views, masked by index
    least = key.min(axis=1)
    return (least >> np.uint64(32)).astype(np.int64), (least & np.uint64(0xffffffff)).astype(np.int64)


def planes_u8(seed, shape):
    """Independent random bytes in every plane (reading the wrong plane gives other numbers)."""
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def tail_case(h, w):
    """Two routes (5 and 70 views), three members x 3 headings in unsorted route order; expected values per channel."""
    first = first_of((5, 70))
    views = planes_u8(100 + h * w, (75, h, w, 3))
    patches = planes_u8(200 + h * w, (3, 3, h, w, 3))
    patches[0, 1] = views[5 + 66]                                                         # an exact view of the own route: 0 at view 66
    routes = np.array([1, 0, 1], dtype=np.int32)
    want = {ch: expected(views, first, patches, routes, ch) for ch in range(3)}
    assert all(want[ch][0][0, 1] == 0 and want[ch][1][0, 1] == 66 for ch in range(3))
    assert not np.array_equal(want[0][0], want[1][0]) and not np.array_equal(want[1][0], want[2][0])
    return _freeze(dict(views=views, first=first, patches=patches, routes=routes, want=want))


EDGE_BYTES = (0, 127, 128, 255)


@functools.lru_cache(maxsize=None)
def edge_byte_case():
    """8 x 8 views and patches of the bias trick's sign edges only: every pair of (0, 127, 128, 255) meets in some pixel."""
    rng = np.random.default_rng(7)
    views = np.array(EDGE_BYTES, dtype=np.uint8)[rng.integers(0, 4, size=(9, 8, 8, 3))]
    patches = np.array(EDGE_BYTES, dtype=np.uint8)[rng.integers(0, 4, size=(1, 4, 8, 8, 3))]
    for k, b in enumerate(EDGE_BYTES):                                                    # constant views and patches: every pair, whole
        views[k], patches[0, k] = b, EDGE_BYTES[(k + 1) % 4]
    first, routes = first_of((9,)), np.array([0], dtype=np.int32)
    return _freeze(dict(views=views, first=first, patches=patches, routes=routes, want=expected(views, first, patches, routes, 2)))


@functools.lru_cache(maxsize=None)
def extreme_case():
    """64 x 64 (P = 4096, the store's limit): route 0 all-0 views against an all-255 patch (MAX_SSD), route 1 a random pair."""
    views = np.zeros((5, 64, 64, 3), dtype=np.uint8)
    views[2:] = planes_u8(11, (3, 64, 64, 3))
    patches = np.empty((2, 1, 64, 64, 3), dtype=np.uint8)
    patches[0] = 255
    patches[1] = planes_u8(12, (1, 64, 64, 3))
    first, routes = first_of((2, 3)), np.array([0, 1], dtype=np.int32)
    want = expected(views, first, patches, routes, 2)
    assert want[0][0, 0] == MAX_SSD and want[1][0, 0] == 0
    return _freeze(dict(views=views, first=first, patches=patches, routes=routes, want=want))


LENGTHS = (2, 33, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def lengths_case(plant_last):
    """Routes of LENGTHS views at 5 x 5, no all-zero view, a member per route with two headings: an all-zero patch and a random one.
    plant_last: the route's last view is the all-ones view, the closest of all to the all-zero patch."""
    first = first_of(LENGTHS)
    views = np.random.default_rng(21).integers(2, 256, size=(int(first[-1]), 5, 5, 3), dtype=np.uint8)
    if plant_last:
        views[first[1:] - 1] = 1
    patches = planes_u8(22, (5, 2, 5, 5, 3))
    patches[:, 0] = 0
    routes = np.array([3, 0, 4, 1, 2], dtype=np.int32)
    want = expected(views, first, patches, routes, 2)
    assert (want[1] < np.array(LENGTHS)[routes][:, None]).all()
    if plant_last:
        assert np.array_equal(want[1][:, 0], np.array(LENGTHS)[routes] - 1)
    return _freeze(dict(views=views, first=first, patches=patches, routes=routes, want=want))


@functools.lru_cache(maxsize=None)
def tie_case(second):
    """A route of 80 views at 6 x 6 with the patch itself at views 5 and `second` (40: the other half of the group; 70: the next group),
    behind a decoy route; two headings with the same patch and a third, worse one in front."""
    views = planes_u8(31, (4 + 80, 6, 6, 3))
    patch = planes_u8(32, (6, 6, 3))
    views[4 + 5] = views[4 + second] = patch
    patches = np.stack([planes_u8(33, (6, 6, 3)), patch, patch])[None]
    first, routes = first_of((4, 80)), np.array([1], dtype=np.int32)
    want = expected(views, first, patches, routes, 2)
    assert want[0][0].tolist()[1:] == [0.0, 0.0] and want[0][0, 0] > 0 and want[1][0].tolist()[1:] == [5, 5] and want[2][0] == 1
    return _freeze(dict(views=views, first=first, patches=patches, routes=routes, want=want))


GEOMETRY_LENGTHS = (7, 70, 3, 129, 40)
GEOMETRIES = {"one": (1, 1), "straddle": (3, 70), "many": (70, 1)}


@functools.lru_cache(maxsize=None)
def geometry_case(name):
    """n members x A headings at 7 x 5 over routes of GEOMETRY_LENGTHS views, the members' routes in unsorted order."""
    n, A = GEOMETRIES[name]
    first = first_of(GEOMETRY_LENGTHS)
    views = planes_u8(41, (int(first[-1]), 7, 5, 3))
    patches = planes_u8(42 + n, (n, A, 7, 5, 3))
    routes = np.array([(3 * i + 1) % 5 for i in range(n)], dtype=np.int32)
    if name == "straddle":
        assert A % TILE and (n * A) // TILE >= 2                                         # more than two tiles, a member's columns in two
    if name == "many":
        assert sorted(set(routes.tolist())) == [0, 1, 2, 3, 4] and routes.tolist() != sorted(routes.tolist())
    return _freeze(dict(views=views, first=first, patches=patches, routes=routes, want=expected(views, first, patches, routes, 2)))


class Recorder(object):
    """Stands where the library does: every call succeeds and is noted by its symbol."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            return 0
        return call
