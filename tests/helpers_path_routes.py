"""Inputs of the routed path-metric tests (tests/test_path_routes_host.py, tests/test_gpu_path_routes.py) and what NumPy makes of them,
computed once.  Nothing here comes from the device.

The expected values are the reference's expression (navsim/NavBySceneFamiliarity.py:252-276), entry by entry:
    delta = path - pos; delta *= delta; dist = np.sqrt(np.sum(delta, axis=1)); nearest = dist.min(); marks |= dist <= reach

Routes, in this order: 1, 2, 1025, 2500 and 263 200 points.  The last is longer than 256 blocks x 1024 points: its walk takes a second
grid-stride trip.  Seven slots dealt (4, 0, 2, 2, 0, 3, 1): not route order, and two pairs share a route.

The calls (CALLS: name -> slots, xs, ys, reach), in the order of SEQUENCE, with the entries planted in them (PLANTED: name -> (call,
entry)):
  one        1 entry   long_second_trip: slot 0 beside point 262 644 of the long route, reachable only in the second trip
  b65       65 entries lone_point_block: slot 2 beyond the end of the 1025-point route, nearest its point 1024 (a block holding one point)
                       partial_block: slot 5 beside point 2400 of the 2500-point route (the last, partial block)
                       just_short: slot 5, 3 to the right of and 4 above point 1234 of that route (integer coordinates), distance 5.0
                                   exactly, reach np.nextafter(5.0, 0): not covered
                       zero_reach: slot 3 ON point 77 of the 1025-point route, reach 0.0: that point only
                       negative: slot 1 ON the one point of route 0, reach -1.0: nothing
                       twice_a, twice_b: slot 2 at two different positions: its marks are the OR
  c130     130 entries exact_reach: `just_short` once more with reach 5.0: covered
                       everything: slot 4 far from the one point of route 0, reach inf: the whole route
  wide  65 537 entries all on slot 6 (the 2-point route), around its first point: the host's second launch takes entries 65 535 and 65 536
Every other entry is drawn from the seed: a slot among 0, 2, 3, 5, a position within 1.5 of a point of its route, a reach in [0, 2.5).
"""
import functools

import numpy as np

ROUTE_POINTS = (1, 2, 1025, 2500, 263200)
ROUTE_OF_SLOT = (4, 0, 2, 2, 0, 3, 1)
SEQUENCE = ("one", "b65", "c130", "wide")
SIZES = {"one": 1, "b65": 65, "c130": 130, "wide": 65537}
INTEGER_POINT = 1234                         # of route 3
TRIP = 256 * 1024                            # points of one trip of the widest grid


@functools.lru_cache(maxsize=None)
def routes():
    """The five routes, float64[n, 2] each (read-only)."""
    rng = np.random.default_rng(20240611)
    out = [np.array([[10.0, 20.0]]), np.array([[5.5, 7.25], [9.0, 3.0]])]
    i = np.arange(ROUTE_POINTS[2], dtype=np.float64)
    out.append(np.stack([30.0 + 0.7 * i, 60.0 + 10.0 * np.cos(i / 50.0) + rng.uniform(-0.05, 0.05, len(i))], axis=1))
    # route 3 runs along (4, -3), at right angles to the (3, 4) of the 3-4-5 position; its point INTEGER_POINT is left on the lattice
    k = np.arange(ROUTE_POINTS[3], dtype=np.float64)
    r3 = np.stack([100.0 + 4.0 * k, 9000.0 - 3.0 * k], axis=1)
    noise = rng.uniform(-0.3, 0.3, r3.shape)
    noise[INTEGER_POINT] = 0.0
    out.append(r3 + noise)
    i = np.arange(ROUTE_POINTS[4], dtype=np.float64)
    out.append(np.stack([20.0 + 0.05 * i, 500.0 + 40.0 * np.sin(i / 700.0) + rng.uniform(-0.01, 0.01, len(i))], axis=1))
    assert tuple(len(r) for r in out) == ROUTE_POINTS
    for r in out:
        r.setflags(write=False)
    return tuple(out)


def first():
    return np.cumsum((0,) + ROUTE_POINTS).astype(np.int64)


def slot_route(slot):
    return routes()[ROUTE_OF_SLOT[slot]]


@functools.lru_cache(maxsize=None)
def calls():
    """(CALLS, PLANTED): name -> (slots int32[n], xs, ys, reach float64[n]); planted name -> (call, entry)."""
    R = routes()
    rng = np.random.default_rng(77)
    out, planted = {}, {}

    def drawn(n):
        slots = rng.choice(np.array([0, 2, 3, 5]), size=n).astype(np.int32)
        xs, ys = np.empty(n), np.empty(n)
        for e, s in enumerate(slots):
            p = slot_route(s)[rng.integers(len(slot_route(s)))]
            xs[e], ys[e] = p[0] + rng.uniform(-1.5, 1.5), p[1] + rng.uniform(-1.5, 1.5)
        return slots, xs, ys, rng.uniform(0.0, 2.5, n)

    def plant(call, entry, name, slot, pos, reach):
        slots, xs, ys, rs = out[call]
        slots[entry], xs[entry], ys[entry], rs[entry] = slot, pos[0], pos[1], reach
        planted[name] = (call, entry)

    out["one"] = drawn(1)
    plant("one", 0, "long_second_trip", 0, R[4][TRIP + 500] + np.array([0.004, -0.003]), 0.12)
    out["b65"] = drawn(65)
    plant("b65", 3, "lone_point_block", 2, R[2][1024] + np.array([0.2, 0.1]), 1.0)
    plant("b65", 10, "partial_block", 5, R[3][2400] + np.array([0.3, 0.2]), 6.0)
    plant("b65", 17, "just_short", 5, R[3][INTEGER_POINT] + np.array([3.0, 4.0]), np.nextafter(5.0, 0.0))
    plant("b65", 30, "zero_reach", 3, R[2][77], 0.0)
    plant("b65", 41, "negative", 1, R[0][0], -1.0)
    plant("b65", 50, "twice_a", 2, R[2][300] + np.array([0.1, 0.3]), 1.2)
    plant("b65", 64, "twice_b", 2, R[2][640] + np.array([-0.2, 0.1]), 0.9)
    out["c130"] = drawn(130)
    plant("c130", 65, "exact_reach", 5, R[3][INTEGER_POINT] + np.array([3.0, 4.0]), 5.0)
    plant("c130", 129, "everything", 4, R[0][0] + np.array([600.0, -800.0]), np.inf)
    n = SIZES["wide"]
    out["wide"] = (np.full(n, 6, dtype=np.int32), R[1][0, 0] + rng.uniform(-3.0, 3.0, n) / np.sqrt(2.0),
                   R[1][0, 1] + rng.uniform(-3.0, 3.0, n) / np.sqrt(2.0), rng.uniform(0.0, 2.0, n))
    assert {k: len(v[0]) for k, v in out.items()} == SIZES
    for v in out.values():
        for a in v:
            a.setflags(write=False)
    return out, planted


def entry(name):
    """(slot, position float64[2], reach) of a planted entry."""
    c, planted = calls()
    call, e = planted[name]
    slots, xs, ys, rs = c[call]
    return int(slots[e]), np.array([xs[e], ys[e]]), float(rs[e])


def distances(path, pos):
    """The reference's expression: float64[n] of the distances from `pos` to every point of `path`."""
    delta = path - pos
    delta *= delta
    return np.sqrt(np.sum(delta, axis=1))


def score(marks, slots, xs, ys, reach, route_of_slot=ROUTE_OF_SLOT, all_routes=None):
    """One call by the reference's expression, entry by entry: float64[n] of nearest; `marks` (a list of bool arrays, one per slot)
    updated in place."""
    all_routes = routes() if all_routes is None else all_routes
    nearest = np.empty(len(slots))
    for e in range(len(slots)):
        dist = distances(all_routes[route_of_slot[slots[e]]], np.array([xs[e], ys[e]]))
        nearest[e] = dist.min()
        marks[slots[e]] |= dist <= reach[e]
    return nearest


def clear_marks(route_of_slot=ROUTE_OF_SLOT, all_routes=None):
    all_routes = routes() if all_routes is None else all_routes
    return [np.zeros(len(all_routes[r]), dtype=bool) for r in route_of_slot]


@functools.lru_cache(maxsize=None)
def expected():
    """name -> (nearest float64[n], marks after the call: a tuple of 7 bool arrays), the calls made in SEQUENCE on cleared slots."""
    c, _ = calls()
    marks = clear_marks()
    out = {}
    for name in SEQUENCE:
        nearest = score(marks, *c[name])
        nearest.setflags(write=False)
        snap = tuple(m.copy() for m in marks)
        for m in snap:
            m.setflags(write=False)
        out[name] = (nearest, snap)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
