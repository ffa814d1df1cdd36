"""Inputs of the windowed route-view tests (tests/test_rvwin_host.py, tests/test_gpu_rvwin.py) and the expected values on them.

Nothing here comes from the device.  A windowed member's expected row is oracle.step (pinned by tests/golden/) on the slice [lo, hi)
of its own route's views, with lo added to the view indices.  The ensemble's expected trajectories are those of SHADOW agents: the
project's own NavBySceneFamiliarity with the sensor model on the host and a plug-in that scores a scene against the slice of its
scenes with oracle.sads_hsv (-inf elsewhere), so that the agent's own loop, movement, error metrics and stop conditions run on it."""
import functools

import numpy as np

import navsim_amd
from navsim_amd import synth
from oracle import oracle
from tests import helpers_lands as HL
from tests import helpers_rviews as HR

MAX_VIEWS = 512                                 # DV_RVWIN_MAX_VIEWS
# helpers_rviews.step_case's seven members sit on routes 4, 0, 2, 4, 1, 3, 2 of lengths 1043, 2, 64, 1043, 63, 65, 64
WINDOWS = ((60, 70),                            # straddles a group edge
           (1, 2),                              # one view, the route's last
           (0, 64),                             # a whole route
           (531, 1043),                         # 512 views, unaligned, to the route's end
           (0, 1),
           (63, 65),                            # runs into the padded last group
           (10, 40))
STEP_CASES = ((7, 5, 1, "random"), (7, 5, 70, "levels"), (19, 17, 10, "levels"), (32, 32, 16, "random"), (5, 7, 260, "random"))
WIDE = dict(lengths=(70, 3), routes=(1, 0, 0), weights=(0.3, 0.0, 1.0))                 # the 64 x 64 case of helpers_rviews
WIDE_WINDOWS = ((0, 3), (3, 70), (63, 65))


def expected(case, windows):
    """oracle.step per member on views [lo, hi) of its own route -> (fam [n, A], view [n, A] (route-relative), best [n])."""
    views, first, patches = case["views"], case["first"], case["patches"]
    n, A = patches.shape[:2]
    fam, view, best = np.empty((n, A)), np.empty((n, A), dtype=np.int64), np.empty(n, dtype=np.int32)
    for i in range(n):
        r, (lo, hi) = case["routes"][i], windows[i]
        assert 0 <= lo < hi <= first[r + 1] - first[r] and hi - lo <= MAX_VIEWS
        lib = np.ascontiguousarray(views[first[r] + lo:first[r] + hi])
        got = oracle.step(lib, patches[i], float(case["weights"][i]))
        fam[i], best[i] = got["angle_familiarity"], got["best_idex"]
        for a in range(A):                                                                # (oracle.step keeps the best heading's view only)
            f = oracle.sads_hsv(lib, patches[i, a], float(case["weights"][i]))
            view[i, a] = lo + int(np.argmax(f))
            assert f[view[i, a] - lo] == fam[i, a]
    return fam, view, best


@functools.lru_cache(maxsize=None)
def expected_case(h, w, A, kind, windows=WINDOWS, **kw):
    """(case of helpers_rviews.step_case, (fam, view, best) under `windows`), computed once."""
    case = HR.step_case(h, w, A, kind, **kw)
    out = expected(case, windows)
    for v in out:
        v.setflags(write=False)
    return case, out


def whole_routes(case):
    return tuple((0, int(case["first"][r + 1] - case["first"][r])) for r in case["routes"])


def duplicates():
    """(views uint8[200, 8, 8, 3], patch): views 10, 100 and 150 are the patch."""
    v = synth.random_hsv(11, (200, 8, 8, 3))
    p = synth.random_hsv(12, (8, 8, 3))
    v[10], v[100], v[150] = p, p, p
    return v, p


def identical_run():
    """(views uint8[400, 8, 8, 3], patches uint8[2, 8, 8, 3]): views [60, 360) are one view; heading 0 is near it, heading 1 random."""
    views = synth.random_hsv(21, (400, 8, 8, 3))
    views[60:360] = synth.random_hsv(22, (8, 8, 3))
    patches = np.stack([synth.near_match_patch(views[60], 5), synth.random_hsv(23, (8, 8, 3))])
    return views, patches


# ---- the ensemble's scenario and its shadow agents ---------------------------------------------------------------------------------------------
ENS_WEIGHTS = (0.25, 0.0, 1.0, 0.25, 0.5, 0.25, 0.3, 0.25, 0.0, 0.75, 0.25, 1.0)         # the twelve of tests/test_gpu_rviews.py
ENS_WINDOW = (2, 3)
ENS_STEPS = 15


class Shadow(object):
    """The plug-in of a shadow agent (familiarity_model=Shadow(...)): perfect memory with the window (behind, ahead), or None."""

    def __init__(self, chem_weight, window, memory_index=None):
        self.chem_weight, self.window, self.memory_index = float(chem_weight), window, memory_index
        self.seen, self.spans = [], []

    def span(self, n):
        if self.window is None or self.memory_index is None:
            return 0, n
        return max(0, self.memory_index - self.window[0]), min(n, self.memory_index + self.window[1] + 1)

    def __call__(self, scenes):
        def func(scene, fambuf):
            lo, hi = self.span(len(scenes))
            fambuf[:] = -np.inf
            fambuf[lo:hi] = oracle.sads_hsv(np.ascontiguousarray(scenes[lo:hi]), np.ascontiguousarray(scene), self.chem_weight)
            self.seen.append(int(np.argmax(fambuf)))
        func.max_familiarity = float(scenes[0].shape[0] * scenes[0].shape[1])
        return func

    def step(self, agent):
        """One step of `agent` (whose plug-in this is) -> the window [lo, hi) it was scored under, or None where it sensed nothing.
        After a step the agent applied, memory_index is the view its chosen heading matched."""
        if agent.stopped_with_exception is not None:
            return None
        self.seen = []
        span = self.span(len(agent.familiar_scenes))
        try:
            agent.step_forward()
        except navsim_amd.StopNavigationException as stop:
            agent.stopped_with_exception = stop
        if len(self.seen) != agent.n_test_angles:                                         # stopped before it sensed (or while sensing)
            return None
        if self.window is not None:
            self.memory_index = self.seen[agent.last_best_idex]
        self.spans.append(span)
        return span


def shadow_agents(landscapes, routes, starts, weights, windows, centres=None):
    """A shadow agent per start, on its own landscape and route; windows / centres: an entry per start (None: whole route)."""
    out = []
    for i, ((r, pos, ang), w) in enumerate(zip(starts, weights)):
        l, path = routes[r]
        plug = Shadow(w, windows[i], None if centres is None else centres[i])
        a = navsim_amd.NavBySceneFamiliarity(np.array(landscapes[l]), HL.ENS_SENSOR, 1.0, n_test_angles=9, use_gpu_sensor=False,
                                             familiarity_model=plug)
        a.train_from_path(path)
        a.position, a.angle = pos, ang
        out.append((a, plug))
    return out


@functools.lru_cache(maxsize=None)
def scenario(windowed=True):
    """The shadow agents of the scenario (windowed: under ENS_WINDOW, no initial centres; else whole routes) stepped ENS_STEPS times ->
    per member dict(pos, ang, fam, memory, spans, code: a list with an entry per step; scene: {step: the agent's scene_familiarity
    after steps 0 and 14, -inf outside the window}; error, coverage, length)."""
    landscapes = HL.lands()[:3]
    routes = HL.ens_routes()
    starts = HL.ens_starts(routes)
    shadows = shadow_agents(landscapes, routes, starts, ENS_WEIGHTS, [ENS_WINDOW if windowed else None] * len(starts))
    rec = [dict(pos=[], ang=[], fam=[], memory=[], spans=[], code=[], scene={}) for _ in shadows]
    for t in range(ENS_STEPS):
        for (a, plug), r in zip(shadows, rec):
            span = plug.step(a)
            r["pos"].append(a.position)
            r["ang"].append(a.angle)
            r["fam"].append(a.angle_familiarity.copy())
            r["memory"].append(plug.memory_index)
            r["spans"].append(span)
            r["code"].append(0 if a.stopped_with_exception is None else a.stopped_with_exception.get_code())
            if t in (0, ENS_STEPS - 1):
                r["scene"][t] = np.array(a.scene_familiarity)
    for (a, _), r in zip(shadows, rec):
        r["error"], r["coverage"] = a.navigation_error, a.percent_recapitulated
        r["length"] = len(a.training_path)
    return rec
