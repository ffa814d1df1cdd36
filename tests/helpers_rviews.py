"""Inputs of the route-view tests (tests/test_rviews_host.py, tests/test_gpu_rviews.py) and the NumPy restatement of the step's rule.

Nothing here comes from the device.  The expected values are oracle.step's (pinned by tests/golden/) on every member's OWN route's
views; `statement` restates what the fast path does -- integer sums, fast score, every view within 2 delta of the fast maximum scored
again exactly, the first exact maximum -- so that the CPU test can pin that the window never drops the true maximum."""
import functools

import numpy as np

from navsim_amd import synth
from oracle import oracle

CAND_CAP = 256                                  # kRvCandCap of dejavu_rviews.inl
SLAB_BYTES = 64 << 20                           # a slab's score buffer
ROUTE_LENGTHS = (2, 63, 64, 65, 1043, 5)        # route 5 is the one no member uses
MEMBER_ROUTES = (4, 0, 2, 4, 1, 3, 2)           # not in route order; route 4 (the longest) twice, route 5 never
MEMBER_WEIGHTS = (0.0, 0.3, 1.0, 0.3, 0.0, 1.0, 0.3)
WIDE_ROUTES = tuple(MEMBER_ROUTES[(i + 1) % 7] for i in range(30))     # 30 members x 260 headings cross the default slab's edge ...
WIDE_WEIGHTS = tuple(MEMBER_WEIGHTS[(i + 1) % 7] for i in range(30))   # ... inside the last member of the sort by route (route 4; member 0: route 0)


def delta(P):
    """The project's bound on |fast score - sequential double| (dejavu_hip.hip c->delta)."""
    return 4.0 * (P + 8.0) * 2.0 ** -53 * P


def first_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def statement(views, patches, cw):
    """(angle_fam float64[A], angle_view int64[A], best, most candidates of a column): the fast path's rule in NumPy."""
    F, h, w, _ = views.shape
    A, P = patches.shape[0], h * w
    fam, view, most = np.empty(A), np.empty(A, dtype=np.int64), 0
    for a in range(A):
        s_hs, s_v = oracle.int_sums(views, patches[a])
        assert s_hs.max() <= 510 * P and s_v.max() <= 255 * P
        fast = oracle.fam_from_sums(s_hs, s_v, P, cw)
        cand = np.flatnonzero(fast >= fast.max() - 2.0 * delta(P))
        exact = oracle.sads_hsv(np.ascontiguousarray(views[cand]), patches[a], cw)
        k = int(np.argmax(exact))
        fam[a], view[a], most = exact[k], cand[k], max(most, len(cand))
    return fam, view, int(np.argmax(fam)), most


def expected(views, first, patches, routes, weights):
    """oracle.step per member on its own route's views -> (fam [n, A], view [n, A], best [n], scene: list of float64[len])."""
    n, A = patches.shape[:2]
    fam, view, best, scene = np.empty((n, A)), np.empty((n, A), dtype=np.int64), np.empty(n, dtype=np.int32), []
    for i in range(n):
        lib = views[first[routes[i]]:first[routes[i] + 1]]
        r = oracle.step(lib, patches[i], float(weights[i]))
        fam[i], best[i] = r["angle_familiarity"], r["best_idex"]
        scene.append(r["scene_familiarity"])
        for a in range(A):                                                                # (oracle.step keeps the best heading's view only)
            f = oracle.sads_hsv(lib, patches[i, a], float(weights[i]))
            view[i, a] = int(np.argmax(f))
            assert f[view[i, a]] == fam[i, a]
    return fam, view, best, scene


def _data(kind, seed, n, h, w):
    if kind == "random":                                                                  # any hue, S up to 255
        return synth.random_hsv(seed, (n, h, w, 3))
    return synth.synth_views(seed, n, h, w)                                               # the five-level synthetic views


@functools.lru_cache(maxsize=None)
def step_case(h, w, A, kind, lengths=ROUTE_LENGTHS, routes=MEMBER_ROUTES, weights=MEMBER_WEIGHTS):
    """dict(views, first, patches [n, A, h, w, 3], routes, weights, fam, view, best, scene).  A few patches are near copies of views of
    their own route and of ANOTHER route (a member scored on the wrong route gets another maximum)."""
    first = first_of(lengths)
    views = _data(kind, 1000 + h * w + A, int(first[-1]), h, w)
    n = len(routes)
    patches = _data(kind, 2000 + h * w + A, n * A, h, w).reshape(n, A, h, w, 3).copy()
    for i in range(n):
        r = routes[i]
        own = first[r] + (7 * i + 1) % lengths[r]
        patches[i, A // 2] = synth.near_match_patch(views[own], 31 + i)
        other = first[(r + 1) % len(lengths)]
        patches[i, 0] = views[other]                                                      # an exact copy of a view the member must not see
    routes_a, weights_a = np.array(routes, dtype=np.int32), np.array(weights, dtype=np.float64)
    fam, view, best, scene = expected(views, first, patches, routes_a, weights_a)
    for i in range(n):
        assert fam[i, 0] < h * w                                                          # (the foreign copy found no equal in the own route)
    out = dict(views=views, first=first, patches=patches, routes=routes_a, weights=weights_a, fam=fam, view=view, best=best, scene=scene)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def slab_columns(lmax):
    """The columns of a slab by default: what 64 MiB of doubles hold at a row stride of the longest route padded to 64 views."""
    return max(1, SLAB_BYTES // ((lmax + 63) // 64 * 64 * 8))


def sorted_member_at(routes, A, column):
    """The member whose columns hold sorted column `column` (members sorted by route, stable)."""
    order = np.argsort(np.asarray(routes), kind="stable")
    return int(order[column // A])


def permuted_route(h, w, n, seed):
    """n views that are pixel permutations of one random view (equal integer sums against a constant patch, different sequential
    doubles) and the constant patch."""
    rng = np.random.default_rng(seed)
    base = synth.random_hsv(seed, (h * w, 3))
    base[:, 0] = 7                                                                        # one hue: S differences, never sums
    views = np.stack([base[rng.permutation(h * w)] for _ in range(n)]).reshape(n, h, w, 3)
    patch = np.empty((h, w, 3), dtype=np.uint8)
    patch[...] = (7, 11, 3)
    return np.ascontiguousarray(views), patch
