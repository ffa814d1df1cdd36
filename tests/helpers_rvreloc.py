"""Inputs of the re-localisation tests (tests/test_rvreloc_host.py, tests/test_gpu_rvreloc.py) and the expected values on them.

Nothing here comes from the device.  THE RULE: a windowed member is lost iff the largest value of its windowed row (oracle.step on the
slice [lo, hi) of its own route, tests/helpers_rvwin.py) is < its threshold; a lost member's row is oracle.step on its whole route
(tests/helpers_rviews.py).  Thresholds are taken from the oracle's windowed rows: `stay` is the windowed maximum itself (a strict < does
not trigger), `go` the next double above it (it does).  `device_plan` restates what k_rvreloc_plan writes, in NumPy prefix sums; the
CPU test holds it against rviews_plan's tiles for the same columns.  FakeEngine answers SadsRouteEnsemble's device calls on the host;
RelocShadow is helpers_rvwin.Shadow with the rule applied in Python."""
import functools
import types

import numpy as np

import navsim_amd
from navsim_amd import synth
from navsim_amd.engine import RouteViewResults
from oracle import oracle
from tests import helpers_lands as HL
from tests import helpers_rviews as HR
from tests import helpers_rviews_edges as HE
from tests import helpers_rvwin as HW

RELOCALISED, SENSE_ERROR = 32, 16               # DV_RES_RELOCALISED, DV_RES_SENSE_ERROR
NEVER, ALWAYS = -np.inf, np.inf


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def stay(row):
    """The threshold that just does NOT relocalise a member whose windowed row is `row`."""
    return float(np.max(row))


def go(row):
    """The least threshold that relocalises it."""
    return float(np.nextafter(np.max(row), np.inf))


def apply_rule(windowed, whole, taus):
    """windowed, whole: (fam [n, A], view [n, A], best [n]); taus [n] -> (fam, view, best, lost bool[n]) by the rule."""
    taus = np.asarray(taus, dtype=np.float64)
    lost = np.array([np.max(windowed[0][i]) < taus[i] for i in range(len(taus))])
    out = [np.where(lost.reshape((-1,) + (1,) * (w.ndim - 1)), g, w) for w, g in zip(windowed, whole)]
    return out[0], out[1].astype(np.int64), out[2].astype(np.int32), lost


def check(r, want, flagged=()):
    """The results of a relocalising call against (fam, view, best, lost): bits, views, headings, flags."""
    fam, view, best, lost = want
    keep = np.array([i not in flagged for i in range(len(lost))])
    assert np.array_equal(bits(r.angle_familiarity[keep]), bits(fam[keep]))
    assert np.array_equal(r.angle_view[keep], view[keep]) and np.array_equal(r.best_idex[keep], best[keep])
    flags = np.where(keep, np.where(lost, RELOCALISED, 0), SENSE_ERROR)
    assert np.array_equal(r.flags, flags.astype(np.uint32)), (r.flags, flags)
    assert np.array_equal(r.relocalised, lost & keep)


# ---- the basic case: routes of 2, 65 and 130 views, six members x five headings ------------------------------------------------------------
BASIC_LENGTHS = (2, 65, 130)                    # the group edge at 64 views is crossed once and twice
BASIC_ROUTES = (2, 0, 1, 2, 1, 2)               # not in route order
BASIC_WEIGHTS = (0.0, 0.25, 1.0, 0.25, 0.0, 1.0)
BASIC_WINDOWS = ((60, 70), (0, 1), (3, 9), (100, 130), (60, 65), (0, 12))
BASIC_SHAPES = ((5, 7), (8, 8))                 # 35 pixels: Pw = 9, a ragged last dword


@functools.lru_cache(maxsize=None)
def basic(h, w, A=5, lengths=BASIC_LENGTHS, routes=BASIC_ROUTES, weights=BASIC_WEIGHTS, windows=BASIC_WINDOWS, kind="random"):
    """(case of helpers_rviews.step_case, windowed (fam, view, best), whole (fam, view, best))."""
    case = HR.step_case(h, w, A, kind, lengths=lengths, routes=routes, weights=weights)
    windowed = HW.expected(case, windows)
    return case, windowed, (case["fam"], case["view"], case["best"])


def mixed_thresholds(windowed):
    """-inf, +inf and the two edge values, in turn over the members: members 1, 3 and 5 are lost."""
    fam = windowed[0]
    kinds = ("never", "always", "stay", "go")
    return np.array([dict(never=NEVER, always=ALWAYS, stay=stay(fam[i]), go=go(fam[i]))[kinds[i % 4]] for i in range(len(fam))])


# ---- the basic case sensed: a sensor of the views' own shape on landscape L0 ------------------------------------------------------------------
def _host_agent(h, w):
    a = navsim_amd.NavBySceneFamiliarity(np.array(HL.lands()[0]), (w, h), 1.0, n_test_angles=9, sensor_pixel_dimensions=[2, 2], n_sensor_levels=5,
                                         mask_middle_n=0, use_gpu_sensor=False, familiarity_model=HL._keep)
    return a


@functools.lru_cache(maxsize=None)
def sensed_basic(h, w):
    """basic(h, w) with the members' patches sensed: dict(xs, ys, angs, lut, case, windowed, whole) -- the store's views are basic's, the
    patches the host sensor model's views of six poses x five headings on L0 (w x h pixels of 2 x 2, five levels, no mask)."""
    base = basic(h, w)[0]
    agent = _host_agent(h, w)
    rng = np.random.default_rng(7 * h + w)
    n, A = len(BASIC_ROUTES), 5
    xs, ys, angs = rng.uniform(60, 240, n), rng.uniform(60, 240, n), rng.uniform(0, 2 * np.pi, (n, A))
    patches = np.stack([np.stack([np.array(agent.get_sensor_mat((float(xs[i]), float(ys[i])), float(angs[i, a]))) for a in range(A)]) for i in range(n)])
    case = dict(views=base["views"], first=base["first"], patches=np.ascontiguousarray(patches), routes=base["routes"], weights=base["weights"])
    fam, view, best, _ = HR.expected(case["views"], case["first"], case["patches"], case["routes"], case["weights"])
    return dict(xs=xs, ys=ys, angs=angs, lut=agent._level_tables(), case=case, windowed=HW.expected(case, BASIC_WINDOWS), whole=(fam, view, best))


# ---- lost counts per route: tiles of 16, 12, 8 and 4 columns -------------------------------------------------------------------------------
# A = 4 headings; the lost members of a route give its lost columns: route 0 -> 7 members = 28 columns = tiles of 16 and 12 (two tiles of
# one route); route 1 -> nobody lost, between two routes that have some; route 2 -> 2 members = 8; route 3 -> 1 member = 4.  Members are
# given in an order that is not sorted by route, and some members of routes 0, 2 and 3 are not lost.
COUNTS_A = 4
COUNTS_LENGTHS = (65, 2, 70, 130)
COUNTS_ROUTES = (3, 0, 2, 0, 1, 0, 0, 2, 1, 0, 3, 0, 0, 2, 0, 0, 3)
COUNTS_LOST = (1, 1, 1, 1, 0, 1, 0, 0, 0, 1, 0, 1, 1, 1, 1, 0, 0)
COUNTS_TILES = [(0, 16), (0, 12), (2, 8), (3, 4)]


@functools.lru_cache(maxsize=None)
def counts_case():
    n = len(COUNTS_ROUTES)
    weights = tuple((0.0, 0.25, 1.0)[i % 3] for i in range(n))
    lens = [COUNTS_LENGTHS[r] for r in COUNTS_ROUTES]
    windows = tuple((l // 2, min(l, l // 2 + 1 + i % 5)) for i, l in enumerate(lens))
    case, windowed, whole = basic(8, 8, A=COUNTS_A, lengths=COUNTS_LENGTHS, routes=COUNTS_ROUTES, weights=weights, windows=windows)
    taus = np.array([go(windowed[0][i]) if COUNTS_LOST[i] else stay(windowed[0][i]) for i in range(n)])
    return case, windows, taus, apply_rule(windowed, whole, taus)


# ---- more members and columns than one pass of the planning workgroup ------------------------------------------------------------------------
# k_rvreloc_plan is one workgroup of 256 threads: 300 members are two passes of its member loop (the prefix's running base crosses from
# one to the next), their 600 columns three passes of its column loop (the tiles' running count does).
MANY_N, MANY_A = 300, 2


@functools.lru_cache(maxsize=None)
def many_case():
    rng = np.random.default_rng(17)
    routes = tuple(int(r) for r in rng.integers(0, 3, MANY_N))
    weights = tuple((0.0, 0.25, 1.0)[i % 3] for i in range(MANY_N))
    windows = tuple((l // 2, min(l, l // 2 + 1 + i % 7)) for i, l in enumerate(BASIC_LENGTHS[r] for r in routes))
    case, windowed, whole = basic(8, 8, A=MANY_A, routes=routes, weights=weights, windows=windows)
    lost = rng.integers(0, 3, MANY_N) > 0                                                  # two members in three
    taus = np.array([go(windowed[0][i]) if lost[i] else stay(windowed[0][i]) for i in range(MANY_N)])
    return case, windows, taus, apply_rule(windowed, whole, taus)


# ---- the device's plan in NumPy --------------------------------------------------------------------------------------------------------------
def groups(n, A, slab):
    """The consecutive groups of members whose columns fit a slab of `slab` columns (one member at least): [(m0, m1)]."""
    gm = min(n, max(1, slab // A))
    return [(g0, min(n, g0 + gm)) for g0 in range(0, n, gm)]


def device_plan(routes, lost, A, T):
    """What k_rvreloc_plan writes for ONE group: (col_of, tiles [(s0, n, route)]).  The host's part: the members sorted by route (stable)
    and each sorted place's run of its route; the device's: an exclusive prefix of the lost members in sorted order, a lost member's
    column a at prefix * A + a, a tile's start where the distance from the first lost column of the route is a multiple of T, and a
    second exclusive prefix that numbers the tiles."""
    routes, lost = np.asarray(routes), np.asarray(lost, dtype=bool)
    order = np.argsort(routes, kind="stable")
    sr = routes[order]
    run0 = np.array([np.flatnonzero(sr == r)[0] for r in sr])
    run1 = np.array([np.flatnonzero(sr == r)[-1] + 1 for r in sr])
    keep = lost[order].astype(np.int64)
    pm = np.concatenate([[0], np.cumsum(keep)])
    col_of = np.full(int(pm[-1]) * A, -1, dtype=np.int64)
    start = np.zeros(len(order) * A, dtype=np.int64)
    entry = {}
    for s in range(len(order) * A):
        m, a = divmod(s, A)
        if not keep[m]:
            continue
        k, ke = pm[m] * A + a, pm[run1[m]] * A
        col_of[k] = order[m] * A + a
        if (k - pm[run0[m]] * A) % T == 0:
            start[s] = 1
            entry[s] = (int(k), int(min(T, ke - k)), int(sr[m]))
    number = np.concatenate([[0], np.cumsum(start)])
    tiles = [None] * int(number[-1])
    for s, t in entry.items():
        tiles[number[s]] = t
    return col_of, tiles


def host_plan(routes, lost, A, T):
    """rviews_plan's column order and tiles (tests/helpers_rviews_edges.tiles) of a call that holds the lost members only."""
    members = np.flatnonzero(np.asarray(lost, dtype=bool))
    r = np.asarray(routes)[members]
    order = members[np.argsort(r, kind="stable")]
    col_of = (order[:, None] * A + np.arange(A)[None, :]).reshape(-1)
    if not len(members):
        return col_of, []
    return col_of, HE.tiles(r, A, T, 64)


# ---- a fake engine for the ensemble's routing, mask and bookkeeping -------------------------------------------------------------------------
class FakeEngine(object):
    """Answers SadsRouteEnsemble's device calls on the host.  A windowed row is fam[k, a] = level[route] + a, view = lo + a clipped to
    the window; a whole-route row is 100 + a, view = 2 * a.  With reloc_below the rule is applied: a lost member's row is the whole
    route's and its flag 32.  rviews_scene answers rows of 7.0."""

    def __init__(self, lengths, level, flagged=None):
        self.lengths, self.level, self.flagged, self.calls = lengths, level, flagged, []

    def _whole(self, routes, A):
        n = len(routes)
        fam = 100.0 + np.tile(np.arange(A, dtype=np.float64), (n, 1))
        view = np.minimum(2 * np.tile(np.arange(A), (n, 1)), np.array([self.lengths[r] for r in routes])[:, None] - 1).astype(np.int64)
        return fam, view

    def _flags(self, routes):
        return np.array([SENSE_ERROR if r == self.flagged else 0 for r in routes], dtype=np.uint32)

    def rviews_sense_step(self, x, y, angs, routes, weights, land_of_member=None):
        self.calls.append(("rviews", list(routes)))
        fam, view = self._whole(routes, np.asarray(angs).shape[1])
        flags = self._flags(routes)
        return RouteViewResults(fam, view, np.where(flags > 0, -1, fam.shape[1] - 1).astype(np.int32), flags)

    def rvwin_sense_step(self, x, y, angs, routes, weights, win_lo, win_hi, land_of_member=None, **more):
        assert set(more) <= {"reloc_below"}
        tau = more.get("reloc_below")
        self.calls.append(("rvwin", list(routes), list(win_lo), list(win_hi), None if tau is None else np.asarray(tau).tolist()))
        n, A = len(routes), np.asarray(angs).shape[1]
        fam = np.array([self.level[r] for r in routes], dtype=np.float64)[:, None] + np.arange(A)[None, :]
        view = np.minimum(np.asarray(win_lo)[:, None] + np.arange(A)[None, :], np.asarray(win_hi)[:, None] - 1).astype(np.int64)
        flags = self._flags(routes)
        if tau is not None:
            lost = (fam.max(axis=1) < np.asarray(tau)) & (flags == 0)
            wf, wv = self._whole(routes, A)
            fam, view = np.where(lost[:, None], wf, fam), np.where(lost[:, None], wv, view)
            flags = np.where(lost, RELOCALISED, flags).astype(np.uint32)
        return RouteViewResults(fam, view, np.where(flags & SENSE_ERROR, -1, A - 1).astype(np.int32), flags)

    def rviews_scene(self, x, y, angs, routes, weights, land_of_member=None):
        self.calls.append(("scene", list(routes)))
        return [np.full(self.lengths[r], 7.0) for r in routes]


class FakeMember(types.SimpleNamespace):
    @property
    def scene_familiarity(self):
        return self._scene_fam


def fake_ensemble(lengths, level, routes, windows, centres, thresholds, flagged=None):
    E = navsim_amd.SadsRouteEnsemble
    ens = object.__new__(E)
    ens.agents = [FakeMember(training_path=np.zeros((lengths[r], 2)), memory_bank=r, window=w, memory_index=m,
                             relocalise_below=t, relocalised=False, n_relocalisations=0, track_scene_familiarity=True,
                             _scene_fam=np.zeros(lengths[r]), _scene_stale=None, _scene_owner=None, _scene_is_inf=False)
                  for r, w, m, t in zip(routes, windows, centres, thresholds)]
    ens.engine = FakeEngine(lengths, level, flagged)
    ens._banks = np.array(routes, dtype=np.int32)
    ens._weights = np.full(len(routes), 0.25)
    ens._lands = None
    return ens


def fake_step(ens, idx, A=3):
    """_device_step for the members idx, and the scene notes step_forward leaves for those that apply the step."""
    n = len(idx)
    r = ens._device_step(idx, np.zeros(n), np.zeros(n), np.zeros((n, A)))
    for k, i in enumerate(idx):
        if not r.flags[k] & SENSE_ERROR:
            ens._note_scene(ens.agents[i], 0.0, 0.0, np.zeros(A), 0.25)
    return r


# ---- the ensemble's scenario on a 32 x 32 sensor and its shadow agents ---------------------------------------------------------------------
ENS_SENSOR = (32, 32)
ENS_WINDOW = (5, 5)
ENS_STEPS = 40
ENS_WEIGHTS = (0.25, 0.0, 0.25, 0.5)
ENS_THRESHOLD = 850.0                           # between what the mis-centred members see in their windows and what the others do (asserted)
ENS_LENGTHS = (75, 90)


def ens_routes():
    """Two routes on landscape L0 of helpers_lands."""
    return [synth.sin_training_path(0.2, 60, 180, arclen=1.0)[:ENS_LENGTHS[0]], synth.sin_training_path(0.3, 60, 180, arclen=1.0)[:ENS_LENGTHS[1]]]


def ens_starts(routes):
    """Two members a route, each ON its route at its fourth point: (route_index, (x, y), angle)."""
    out = []
    for r, path in enumerate(routes):
        d = path[4] - path[3]
        for _ in range(2):
            out.append((r, (float(path[3][0]), float(path[3][1])), float(np.arctan2(d[1], d[0]) % (2 * np.pi))))
    return out


def ens_centres(routes):
    """Members 0 and 2 know where they are; members 1 and 3 believe themselves at the far end of their route."""
    return [3, len(routes[0]) - 1, 3, len(routes[1]) - 1]


class RelocShadow(HW.Shadow):
    """helpers_rvwin.Shadow with the rule: before a windowed step the shadow senses the agent's test headings on the host, takes the
    largest windowed familiarity over them, and where that is < `below` scores this step against the whole route."""

    def __init__(self, chem_weight, window, memory_index=None, below=None):
        HW.Shadow.__init__(self, chem_weight, window, memory_index)
        self.below, self.relocalised, self.n_relocalisations, self._whole, self.best_windowed = below, False, 0, False, []

    def span(self, n):
        return (0, n) if self._whole else HW.Shadow.span(self, n)

    def step(self, agent):
        lost, best = False, None
        if agent.stopped_with_exception is None and self.window is not None and self.memory_index is not None:
            lo, hi = HW.Shadow.span(self, len(agent.familiar_scenes))
            lib = np.ascontiguousarray(agent.familiar_scenes[lo:hi])
            try:
                heads = (agent.angle + agent.angle_offsets) % (2 * np.pi)
                scenes = [np.array(agent.get_sensor_mat(agent.position, h)) for h in heads]
                best = max(float(oracle.sads_hsv(lib, np.ascontiguousarray(s), self.chem_weight).max()) for s in scenes)
            except (navsim_amd.StopNavigationException, IndexError):
                best = None                                                               # (the agent's own step stops it the same way)
            lost = best is not None and self.below is not None and best < self.below
        self._whole = lost
        try:
            span = HW.Shadow.step(self, agent)
        finally:
            self._whole = False
        if span is not None:
            self.relocalised = lost
            self.n_relocalisations += int(lost)
            self.best_windowed.append(best)
        return span


def shadow_agents(thresholds, centres=None):
    land = HL.lands()[0]
    routes = ens_routes()
    out = []
    for i, (r, pos, ang) in enumerate(ens_starts(routes)):
        plug = RelocShadow(ENS_WEIGHTS[i], ENS_WINDOW, (ens_centres(routes) if centres is None else centres)[i], thresholds[i])
        a = navsim_amd.NavBySceneFamiliarity(np.array(land), ENS_SENSOR, 1.0, n_test_angles=9, use_gpu_sensor=False, familiarity_model=plug)
        a.train_from_path(routes[r])
        a.position, a.angle = pos, ang
        out.append((a, plug))
    return out


@functools.lru_cache(maxsize=None)
def scenario(threshold):
    """The four shadow agents under `threshold` (None: no loss test) stepped ENS_STEPS times -> per member dict(pos, ang, fam, memory,
    relocalised, n, code: an entry per step; scene: {step: scene_familiarity, -inf where nothing was scored}; best_windowed)."""
    shadows = shadow_agents([threshold] * 4)
    rec = [dict(pos=[], ang=[], fam=[], memory=[], relocalised=[], n=[], code=[], scene={}) for _ in shadows]
    for t in range(ENS_STEPS):
        for (a, plug), r in zip(shadows, rec):
            plug.step(a)
            r["pos"].append(a.position)
            r["ang"].append(a.angle)
            r["fam"].append(a.angle_familiarity.copy())
            r["memory"].append(plug.memory_index)
            r["relocalised"].append(plug.relocalised)
            r["n"].append(plug.n_relocalisations)
            r["code"].append(0 if a.stopped_with_exception is None else a.stopped_with_exception.get_code())
            if t in (0, 1, ENS_STEPS - 1):
                r["scene"][t] = np.array(a.scene_familiarity)
    for (a, plug), r in zip(shadows, rec):
        r["best_windowed"] = list(plug.best_windowed)
    return rec
