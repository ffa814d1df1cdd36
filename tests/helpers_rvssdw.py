"""Inputs of the windowed SSD route-view tests (tests/test_rvssdw_host.py, tests/test_gpu_rvssdw.py), the expected values on them and
the NumPy restatement of what the windowed scoring kernel does.

Nothing here comes from the device.  The expected value of a member under the window [lo, hi) is tests/helpers_rvssd.py's `expected`
(ssd_rows, the least view, the first least heading) on the slice views[first[r] + lo : first[r] + hi] alone, with lo added to its view
indices.  `window_statement` restates k_rvssdw_score of csrc/dejavu_rvssdw.inl: the view groups lo >> 6 .. (hi - 1) >> 6 that the
workgroup covers, whole, the key ssd << 32 | view of every covered view, all ones outside [lo, hi), and the minimum of the key.  Every
case asserts what the GPU test relies on."""
import functools

import numpy as np

from tests import helpers_rvssd as HV

MEMBERS_PER_LAUNCH = 32768                       # kRvssdwMembersPerLaunch: members of a windowed scoring launch at most
AHEAD = 4                                        # kRvssdwAhead: K-steps whose loads the windowed kernel issues together
MAX_VIEWS = 512                                  # DV_RVWIN_MAX_VIEWS
RELOCALISED, SENSE_ERROR = 32, 16


def window_expected(views, first, patches, routes, windows, channel):
    """Per member on views [lo, hi) of its own route -> (ssd float64[n, A], view int64[n, A] counted from the route's first view,
    best int32[n])."""
    n, A = patches.shape[:2]
    ssd, view, best = np.empty((n, A)), np.empty((n, A), dtype=np.int64), np.empty(n, dtype=np.int32)
    for i, (lo, hi) in enumerate(windows):
        f = int(first[routes[i]])
        assert 0 <= lo < hi <= first[routes[i] + 1] - f and hi - lo <= MAX_VIEWS
        s, v, b, _ = HV.expected(views[f + lo:f + hi], HV.first_of((hi - lo,)), patches[i:i + 1], [0], channel)
        ssd[i], view[i], best[i] = s[0], v[0] + lo, b[0]
    return ssd, view, best


def covered_groups(lo, hi):
    """The store's groups of 64 views that a workgroup reads for the window [lo, hi): first and last."""
    return lo >> 6, (hi - 1) >> 6


def window_statement(lib, pats, lo, hi, channel):
    """k_rvssdw_score on one member in NumPy -> (ssd int64[A], view int64[A]).  lib uint8[L, h, w, 3]: the member's whole route."""
    L, A = len(lib), len(pats)
    P = lib.shape[1] * lib.shape[2]
    Pw, Kp = (P + 3) // 4, (P + 31) // 32
    Lpad = (L + 63) // 64 * 64
    g0, g1 = covered_groups(lo, hi)
    assert g1 - g0 + 1 <= 9 and (g1 + 1) * 64 <= Lpad
    f = np.arange(g0 * 64, (g1 + 1) * 64)                                                 # the covered views, padding views included
    plane = np.zeros((Lpad, Pw * 4), dtype=np.uint8)                                      # the store's plane: 0 beyond P and beyond L
    plane[:L, :P] = lib[..., channel].reshape(L, P)
    b = np.zeros((len(f), Kp * 32), dtype=np.int64)
    b[:, :Pw * 4] = (plane[f] ^ 0x80).view(np.int8)
    a = np.zeros((A, Kp * 32), dtype=np.int64)
    a[:, :P] = (pats[..., channel].reshape(A, P) ^ 0x80).view(np.int8)
    vnorm = ((plane[f, :P].astype(np.int64) - 128) ** 2).sum(axis=1)
    pnorm = ((pats[..., channel].reshape(A, P).astype(np.int64) - 128) ** 2).sum(axis=1)
    acc = a @ b.T
    assert np.abs(acc).max() < 2 ** 31
    ssd = vnorm[None, :] + pnorm[:, None] - 2 * acc
    assert ssd.min() >= 0 and ssd.max() < 2 ** 31
    key = (ssd.astype(np.uint64) << np.uint64(32)) | f.astype(np.uint64)[None, :]
    key[:, (f < lo) | (f >= hi)] = np.uint64(0xffffffffffffffff)                          # outside the window: the route's padding too
    least = key.min(axis=1)
    return (least >> np.uint64(32)).astype(np.int64), (least & np.uint64(0xffffffff)).astype(np.int64)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _case(views, first, patches, routes, windows, channel=2, **more):
    routes = np.array(routes, dtype=np.int32)
    want = window_expected(views, first, patches, routes, windows, channel)
    return _freeze(dict(views=views, first=first, patches=patches, routes=routes, windows=tuple(windows), want=want, **more))


EDGE_WINDOWS = ((0, 1), (63, 65), (64, 128), (63, 575), (100, 130))


@functools.lru_cache(maxsize=None)
def edges_case():
    """5 x 5 views without an all-zero view: route 0 of 600 views under [0,1), [63,65), [64,128) and [63,575) (512 views in 9 groups),
    route 1 of 130 views under a window that ends where the route does; heading 0 is the all-zero patch, closest to the zero bytes that
    pad route 1's last group."""
    first = HV.first_of((600, 130))
    views = np.random.default_rng(51).integers(2, 256, size=(730, 5, 5, 3), dtype=np.uint8)
    patches = HV.planes_u8(52, (5, 2, 5, 5, 3))
    patches[:, 0] = 0
    c = _case(views, first, patches, [0, 0, 0, 0, 1], EDGE_WINDOWS)
    assert covered_groups(63, 575) == (0, 8) and 575 - 63 == MAX_VIEWS                   # nine groups: wave 0 takes groups 0, 4 and 8
    assert covered_groups(100, 130) == (1, 2) and (c["want"][0] > 0).all()               # a padding view (ssd 0 at heading 0) would win
    return c


@functools.lru_cache(maxsize=None)
def planted_case():
    """A route of 300 views at 5 x 5 with the patch itself at views lo - 1 and hi of the window [70, 130): both lie in the groups the
    workgroup covers, neither may win."""
    lo, hi = 70, 130
    first = HV.first_of((300,))
    views = HV.planes_u8(53, (300, 5, 5, 3))
    patches = HV.planes_u8(54, (1, 3, 5, 5, 3))
    views[lo - 1] = views[hi] = patches[0, 1]
    c = _case(views, first, patches, [0], [(lo, hi)])
    rows = HV.ssd_rows(views, patches[0], 2)
    assert rows[1, lo - 1] == 0 and rows[1, hi] == 0 and (c["want"][0] > 0).all()
    assert covered_groups(lo, hi) == ((lo - 1) >> 6, hi >> 6)
    return c


TAIL_WINDOWS = ((3, 68), (1, 4), (60, 70))


@functools.lru_cache(maxsize=None)
def tail_case(channel):
    """helpers_rvssd.tail_case(7, 5) (P = 35: a partial last K-step; routes of 5 and 70 views) under windows."""
    t = HV.tail_case(7, 5)
    c = _case(t["views"], t["first"], t["patches"], t["routes"], TAIL_WINDOWS, channel)
    assert c["want"][0][0, 1] == 0 and c["want"][1][0, 1] == 66                          # the planted view 66 lies inside [3, 68)
    return c


@functools.lru_cache(maxsize=None)
def edge_byte_case():
    """helpers_rvssd.edge_byte_case (8 x 8, bytes 0, 127, 128 and 255 only) under the window [2, 9)."""
    t = HV.edge_byte_case()
    return _case(t["views"], t["first"], t["patches"], t["routes"], [(2, 9)])


@functools.lru_cache(maxsize=None)
def extreme_case():
    """helpers_rvssd.extreme_case (64 x 64): the all-255 patch against the all-0 view 1 of route 0 alone, a random pair on route 1."""
    t = HV.extreme_case()
    c = _case(t["views"], t["first"], t["patches"], t["routes"], [(1, 2), (0, 2)])
    assert c["want"][0][0, 0] == HV.MAX_SSD == 266342400 and c["want"][1][0, 0] == 1
    return c


@functools.lru_cache(maxsize=None)
def ahead_case():
    """14 x 14 views (P = 196, Pw = 49): six full K-steps -- one trip of AHEAD = 4 together, two one at a time -- and the partial
    seventh.  Two members x 3 headings on a route of 70 views."""
    P = 14 * 14
    assert (P + 3) // 4 // 8 == AHEAD + 2 and (P + 31) // 32 == AHEAD + 3
    first = HV.first_of((70,))
    views = HV.planes_u8(81, (70, 14, 14, 3))
    patches = HV.planes_u8(82, (2, 3, 14, 14, 3))
    patches[1, 2] = views[65]
    c = _case(views, first, patches, [0, 0], [(10, 70), (60, 66)])
    assert c["want"][0][1, 2] == 0 and c["want"][1][1, 2] == 65
    return c


def tie_windows(second):
    """(both matches, only the second, neither) for helpers_rvssd.tie_case(second): the patch lies at views 5 and `second`."""
    return (0, 80), (6, 80), (6, second)


@functools.lru_cache(maxsize=None)
def tie_case(second, which):
    t = HV.tie_case(second)
    c = _case(t["views"], t["first"], t["patches"], t["routes"], [tie_windows(second)[which]])
    ssd, view, best = c["want"]
    if which == 0:
        assert ssd[0].tolist()[1:] == [0.0, 0.0] and view[0].tolist()[1:] == [5, 5] and best[0] == 1          # the least view, the first heading
    elif which == 1:
        assert ssd[0].tolist()[1:] == [0.0, 0.0] and view[0].tolist()[1:] == [second, second] and best[0] == 1
    else:
        assert (ssd[0] > 0).all() and ssd[0, 1] == ssd[0, 2] and view[0, 1] == view[0, 2] and best[0] != 2
    return c


TILE_ROUTES = (3, 1, 3, 0, 3)                                                             # three members of route 3, in unsorted route order
TILE_WINDOWS = ((60, 129), (0, 70), (0, 64), (2, 7), (64, 65))
TILE_HEADINGS = (1, 33, 70)


@functools.lru_cache(maxsize=None)
def tiles_case(A):
    """Five members x A headings at 7 x 5 over helpers_rvssd's routes of 7, 70, 3, 129 and 40 views."""
    first = HV.first_of(HV.GEOMETRY_LENGTHS)
    views = HV.planes_u8(41, (int(first[-1]), 7, 5, 3))
    patches = HV.planes_u8(60 + A, (5, A, 7, 5, 3))
    c = _case(views, first, patches, TILE_ROUTES, TILE_WINDOWS)
    whole = HV.expected(views, first, patches, c["routes"], 2)
    assert not np.array_equal(whole[0][[0, 2, 4]], c["want"][0][[0, 2, 4]])               # the window matters
    if A > 1:
        assert len(set(map(bytes, c["want"][0][[0, 2, 4]]))) == 3                          # and the three windows of route 3 differ
    return dict(c, whole=whole[:3])


@functools.lru_cache(maxsize=None)
def bound_case():
    """32 769 members x 1 heading at 2 x 2: one more than a windowed scoring launch takes.  The last member alone is on route 1, under
    a window no other member has."""
    n = MEMBERS_PER_LAUNCH + 1
    first = HV.first_of((4, 70))
    views = HV.planes_u8(71, (74, 2, 2, 3))
    patches = HV.planes_u8(72, (n, 1, 2, 2, 3))
    routes = np.zeros(n, dtype=np.int32)
    routes[-1] = 1
    windows = [(1, 3)] * (n - 1) + [(64, 70)]
    rows = HV.ssd_rows(views[1:3], patches[:n - 1, 0], 2)                                 # members 0 .. n - 2: a column each
    last = window_expected(views, first, patches[-1:], [1], windows[-1:], 2)
    ssd = np.concatenate([rows.min(axis=1).astype(np.float64), last[0][0]])[:, None]
    view = np.concatenate([rows.argmin(axis=1) + 1, last[1][0]])[:, None]
    # a launch-local member index would score the last member as member 0: another patch, route and window
    as_first = window_expected(views, first, patches[:1], [0], windows[:1], 2)
    assert (as_first[0][0, 0], as_first[1][0, 0]) != (ssd[-1, 0], view[-1, 0]) and 64 <= view[-1, 0] < 70
    return _freeze(dict(views=views, first=first, patches=patches, routes=routes, windows=tuple(windows),
                        want=(ssd, view.astype(np.int64), np.zeros(n, dtype=np.int32))))


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------------
def stay(ssd_row):
    """The threshold that just does NOT re-localise a member whose windowed SSDs are `ssd_row`: -min ssd (the < is strict)."""
    return float(-np.min(ssd_row))


def go(ssd_row):
    """The least threshold that does: the next double above."""
    return float(np.nextafter(-np.min(ssd_row), np.inf))


def apply_rule(windowed, whole, taus):
    """windowed, whole: (ssd [n, A], view [n, A], best [n]); taus [n] -> (ssd, view, best, lost bool[n]) by the rule."""
    taus = np.asarray(taus, dtype=np.float64)
    lost = np.array([np.max(-windowed[0][i]) < taus[i] for i in range(len(taus))])
    out = [np.where(lost.reshape((-1,) + (1,) * (w.ndim - 1)), g, w) for w, g in zip(windowed, whole)]
    return out[0], out[1].astype(np.int64), out[2].astype(np.int32), lost


def mixed_thresholds(c):
    """For tiles_case: members 0 and 2 (route 3) lost by the next double above, member 1 (route 1) by +inf; member 3 kept by the exact
    value, member 4 by -inf.  The lost members lie on routes 3, 1, 3."""
    ssd = c["want"][0]
    taus = np.array([go(ssd[0]), np.inf, go(ssd[2]), stay(ssd[3]), -np.inf])
    want = apply_rule(c["want"], c["whole"], taus)
    assert want[3].tolist() == [True, True, True, False, False]
    return taus, want


# ---- the ensemble's shadow agents --------------------------------------------------------------------------------------------------------------
class SsdShadow(object):
    """The plug-in of a shadow agent (familiarity_model=SsdShadow(...)): -SSD of one channel in NumPy, with the window (behind, ahead)
    or None, and the rule: before a windowed step the shadow senses the agent's test headings on the host, takes the largest windowed
    familiarity over them, and where that is < `below` scores this step against the whole route."""

    def __init__(self, channel, window, memory_index=None, below=None):
        self.channel, self.window, self.memory_index, self.below = channel, window, memory_index, below
        self.relocalised, self.n_relocalisations, self._whole = False, 0, False
        self.seen, self.spans = [], []

    def span(self, n):
        if self._whole or self.window is None or self.memory_index is None:
            return 0, n
        return max(0, self.memory_index - self.window[0]), min(n, self.memory_index + self.window[1] + 1)

    def _fam(self, scenes, scene):
        return np.negative(HV.ssd_rows(np.asarray(scenes), np.asarray(scene)[None], self.channel)[0].astype(np.float64))

    def __call__(self, scenes):
        def func(scene, fambuf):
            lo, hi = self.span(len(scenes))
            fambuf[:] = -np.inf
            fambuf[lo:hi] = self._fam(scenes[lo:hi], scene)
            self.seen.append(int(np.argmax(fambuf)))
        func.max_familiarity = 0.0
        return func

    def step(self, agent):
        """One step of `agent` (whose plug-in this is) -> the span [lo, hi) it was scored under, or None where it sensed nothing."""
        import navsim_amd
        if agent.stopped_with_exception is not None:
            return None
        lost = False
        if self.window is not None and self.memory_index is not None and self.below is not None:
            lo, hi = self.span(len(agent.familiar_scenes))
            try:
                heads = (agent.angle + agent.angle_offsets) % (2 * np.pi)
                best = max(float(self._fam(agent.familiar_scenes[lo:hi], agent.get_sensor_mat(agent.position, h)).max()) for h in heads)
                lost = best < self.below
            except (navsim_amd.StopNavigationException, IndexError):
                lost = False                                                              # (the agent's own step stops it the same way)
        self._whole, self.seen = lost, []
        span = self.span(len(agent.familiar_scenes))
        try:
            agent.step_forward()
        except navsim_amd.StopNavigationException as stop:
            agent.stopped_with_exception = stop
        finally:
            self._whole = False
        if len(self.seen) != agent.n_test_angles:                                         # stopped before it sensed (or while sensing)
            return None
        if self.window is not None:
            self.memory_index = self.seen[agent.last_best_idex]
            self.relocalised = lost
            self.n_relocalisations += int(lost)
        self.spans.append(None if lost else span)
        return span
