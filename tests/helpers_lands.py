"""Inputs of the landscape-set tests (tests/test_lands_host.py, tests/test_gpu_lands.py) and the expected values on them, computed once.

Nothing here comes from the device: the views are the HOST sensor model's (navsim_amd.agent with use_gpu_sensor=False) on each pose's
own landscape alone, and the models' values are the NumPy statements of tests/helpers_mushroom.py and tests/helpers_infomax.py.

Landscapes (lands()): L0 = synth_landscape(3, 300, 4); L1 = the 211 x 173 top-left part of synth_landscape(5, 300, 4) -- rows != cols,
and 211 * 173 * 3 = 109 509 bytes is odd, so L2 begins at an odd byte of the set; L2 = the 173 x 260 part of synth_landscape(7, 300, 4);
L3 = L0[::-1, ::-1] made contiguous.  SAME_SHAPE are three 300 x 300 landscapes (L0, L3 and synth_landscape(9, 300, 4)).

Sensors (SENSORS): "sq" 32x32 plain; "px" and "odd" of tests/helpers_sensed_models.py (16x8 with [2, 4] blocks, 4 levels, mask 1;
19x17 with [2, 2] blocks, mask 2, N = 323).

Models: mushroom n_kc = 2003 with fan-in 10 (MB) and once fan-in 16 (MB16); Infomax n_hidden = 18 (20 for "px", 16 for "odd").

What the CPU test asserts of these inputs (so that a passing GPU test is not vacuous) is stated beside each function."""
import functools

import numpy as np

from tests import helpers_infomax as HI
from tests import helpers_mushroom as H
from tests import helpers_mushroom_ensemble as HE
from tests import helpers_sensed_models as HS

SENSORS = {
    "sq": dict(sensor=(32, 32), pixel=(1, 1), levels=5, mask=0),
    "px": {k: HS.CONFIGS["px"][k] for k in ("sensor", "pixel", "levels", "mask")},
    "odd": {k: HS.CONFIGS["odd"][k] for k in ("sensor", "pixel", "levels", "mask")},
}
MB = dict(n_kc=2003, fan_in=10, n_active=40, seed=81)
MB16 = dict(n_kc=2003, fan_in=16, n_active=40, seed=82)
IM = dict(n_hidden={"sq": 18, "px": 20, "odd": 16}, eta=1e-3, seed=83)
SENSE_PATTERN = (2, 0, 1, 3, 1, 0, 2)
STEP_BANKS, STEP_LANDS = (1, 0, 2, 0, 1), (0, 1, 2, 3, 1)
SENSE_ERROR = 16
N_BANKS = 3


@functools.lru_cache(maxsize=None)
def lands():
    from navsim_amd import synth
    L0 = synth.synth_landscape(3, 300, 4)
    L1 = np.ascontiguousarray(synth.synth_landscape(5, 300, 4)[:211, :173])
    L2 = np.ascontiguousarray(synth.synth_landscape(7, 300, 4)[:173, :260])
    L3 = np.ascontiguousarray(L0[::-1, ::-1])
    out = (L0, L1, L2, L3)
    assert [l.shape for l in out] == [(300, 300, 3), (211, 173, 3), (173, 260, 3), (300, 300, 3)]
    assert L1.size % 2 == 1                                   # L2's first byte in the set is odd
    for l in out:
        l.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def same_shape_lands():
    from navsim_amd import synth
    L = lands()
    out = (L[0], L[3], synth.synth_landscape(9, 300, 4))
    out[2].setflags(write=False)
    return out


def _keep(scenes):
    def func(scene, fambuf):
        fambuf[...] = 0.0
    func.max_familiarity = 0.0
    return func


@functools.lru_cache(maxsize=None)
def _host_agent(name, l):
    """An agent whose sensor model runs on the host, on landscape l of lands() alone."""
    import navsim_amd
    land = lands()[l]
    c = SENSORS[name]
    agent = navsim_amd.NavBySceneFamiliarity(np.array(land), c["sensor"], 1.0, n_test_angles=9, sensor_pixel_dimensions=list(c["pixel"]),
                                             n_sensor_levels=c["levels"], mask_middle_n=c["mask"], use_gpu_sensor=False, familiarity_model=_keep)
    # the sensor model alone: get_sensor_mat without the agent's own bounds test in front (dv_sense has none either), so that the
    # model's wrap of a negative index and its IndexError past the end are what a pose near an edge meets
    agent._check_bounds = lambda position: None
    return agent


def level_tables(name):
    return _host_agent(name, 0)._level_tables()


def host_scene(name, x, y, angle, land):
    """uint8[h,w,3]: the host model's view of one pose on landscape `land` alone; IndexError where the model raises it."""
    return _host_agent(name, int(land)).get_sensor_mat((float(x), float(y)), float(angle)).copy()


def host_scenes(name, x, y, angle, land_of):
    return np.stack([host_scene(name, xi, yi, ai, l) for xi, yi, ai, l in zip(x, y, angle, land_of)])


def is_off(name, x, y, angle, land):
    try:
        host_scene(name, x, y, angle, land)
    except IndexError:
        return True
    return False


def footprint_indices(name, x, y, angle):
    """(ix, iy) int64 arrays of the landscape pixels the footprint asks for, before any wrap (agent.fill_sensor_from's arithmetic)."""
    import math
    from navsim_amd.agent import _c_round
    c = SENSORS[name]
    n1, n0 = c["sensor"][0] * c["pixel"][0], c["sensor"][1] * c["pixel"][1]
    rot = -(0.5 * math.pi - angle)
    cs, sn = math.cos(rot), math.sin(rot)
    px = np.arange(n1, dtype=np.float64)[None, :] - 0.5 * n1
    py = np.arange(n0, dtype=np.float64)[:, None] - 0.5 * n0
    return _c_round(px * cs - py * sn + x).astype(np.int64), _c_round(px * sn + py * cs + y).astype(np.int64)


# ---- lands_sense ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sense_case(name):
    """14 poses inside every landscape, dealt over the four landscapes as SENSE_PATTERN twice -> dict(x, y, angle, land_of, scenes).
    Asserted: a pose's view on its own landscape differs from its view on every other landscape."""
    rng = np.random.default_rng(11)
    n = 2 * len(SENSE_PATTERN)
    x, y, ang = rng.uniform(45, 125, n), rng.uniform(45, 125, n), rng.uniform(0, 2 * np.pi, n)
    land_of = np.array(SENSE_PATTERN * 2, dtype=np.int32)
    scenes = host_scenes(name, x, y, ang, land_of)
    for v in range(n):
        for l in range(4):
            if l != land_of[v]:
                assert not np.array_equal(host_scene(name, x[v], y[v], ang[v], l), scenes[v]), (name, v, l)
    for a in (x, y, ang, land_of, scenes):
        a.setflags(write=False)
    return dict(x=x, y=y, angle=ang, land_of=land_of, scenes=scenes)


ON_L2_OFF_L1 = (200.0, 80.0, 0.3)                            # x = 200: inside L2's 260 columns, past L1's 173
WRAP_POSE = (10.0, 60.0, 0.0)                                # on L1: the 32 x 32 footprint reaches column -6 ...
WRAP_ROW_POSE = (60.0, 10.0, 0.0)                            # ... and on L2 row -6
WRAPS = {"cols": (WRAP_POSE, 1), "rows": (WRAP_ROW_POSE, 2)}


def wrap_facts(which="cols"):
    """The footprint at WRAPS[which]'s pose reaches a negative column (row) of its landscape, L1 (L2), and leaves it nowhere else; the
    host model wraps it by the landscape's OWN 173 columns (rows): its view there is the view of the pose 173 columns further right
    (rows further down) on the landscape laid beside (below) itself, where nothing wraps.  The wrapped pixels matter (they are not
    what the nearest column or row inside gives), and a wrap by another landscape's extent (300, 260 or 211) would read other pixels.
    Returns the view."""
    import navsim_amd
    (x, y, a), l = WRAPS[which]
    land = lands()[l]
    ix, iy = footprint_indices("sq", x, y, a)
    axis = 1 if which == "cols" else 0
    neg, other = (ix, iy) if which == "cols" else (iy, ix)
    assert land.shape[axis] == 173 and neg.min() < 0 and neg.max() < 173 and 0 <= other.min() and other.max() < land.shape[1 - axis]
    got = host_scene("sq", x, y, a, l)
    twice = navsim_amd.NavBySceneFamiliarity(np.concatenate([land, land], axis=axis), (32, 32), 1.0, n_test_angles=9, use_gpu_sensor=False,
                                             familiarity_model=_keep)
    assert np.array_equal(got, twice.get_sensor_mat((x + 173.0, y) if which == "cols" else (x, y + 173.0), a))
    pick = (lambda k: land[iy, k]) if which == "cols" else (lambda k: land[k, ix])
    assert not np.array_equal(pick(neg % 173), pick(np.clip(neg, 0, None)))
    return got


# ---- training ------------------------------------------------------------------------------------------------------------------------------
ROUTE_CURVES, ROUTE_POINTS, ROUTE_LANDS = (0.2, 0.5, 0.35), (15, 9, 12), (0, 1, 2)


def route_headings(route):
    return H.route_headings(route)


@functools.lru_cache(maxsize=None)
def train_case(name):
    """Three routes, route r on landscape ROUTE_LANDS[r] and into bank r, their views interleaved in the call's order (round robin until
    a route runs out) -> dict(x, y, angle, bank_of, land_of, first (the call's indices of every route), routes, scenes uint8[n,h,w,3]).
    Asserted: every route lies inside its landscape's bounds; the tables are interleaved; the routes' views differ."""
    from navsim_amd import synth
    routes = [synth.sin_training_path(c, 60, 180, arclen=1.0)[:k] for c, k in zip(ROUTE_CURVES, ROUTE_POINTS)]
    order = []
    for s in range(max(ROUTE_POINTS)):
        order += [(r, s) for r in range(3) if s < ROUTE_POINTS[r]]
    heads = [route_headings(r) for r in routes]
    x = np.array([routes[r][s][0] for r, s in order])
    y = np.array([routes[r][s][1] for r, s in order])
    ang = np.array([heads[r][s] for r, s in order])
    bank_of = np.array([r for r, _ in order], dtype=np.int32)
    land_of = np.array([ROUTE_LANDS[r] for r, _ in order], dtype=np.int32)
    first = [np.flatnonzero(bank_of == r) for r in range(3)]
    assert bank_of[:6].tolist() == [0, 1, 2, 0, 1, 2] and land_of[:6].tolist() == [0, 1, 2, 0, 1, 2]
    for r, route in enumerate(routes):
        a = _host_agent(name, ROUTE_LANDS[r])
        for pt in route:
            type(a)._check_bounds(a, pt)                                                  # (the agent's bounds test on the route's landscape)
    scenes = host_scenes(name, x, y, ang, land_of)
    assert not np.array_equal(scenes[0], scenes[1]) and not np.array_equal(scenes[1], scenes[2])
    for a in (x, y, ang, bank_of, land_of, scenes):
        a.setflags(write=False)
    return dict(x=x, y=y, angle=ang, bank_of=bank_of, land_of=land_of, first=first, routes=routes, heads=heads, scenes=scenes)


def off_own_landscape_view(name):
    """(index, x, y): view `index` of train_case moved to a point that is on L0 and L2 but off its own L1."""
    t = train_case(name)
    v = int(np.flatnonzero(t["land_of"] == 1)[2])
    x, y, a = ON_L2_OFF_L1[0], ON_L2_OFF_L1[1], float(t["angle"][v])
    assert is_off(name, x, y, a, 1) and not is_off(name, x, y, a, 0) and not is_off(name, x, y, a, 2)
    return v, x, y


def mb_model(name, spec=None):
    spec = spec or MB
    w, h = SENSORS[name]["sensor"]
    return H.connectivity(spec["n_kc"], w * h, spec["fan_in"], spec["seed"]), spec["n_active"]


@functools.lru_cache(maxsize=None)
def mb_banks(name, channel, wide=False):
    """(conn, n_active, wts uint8[3, K]): the statement, bank r trained on route r's host-sensed planes.  Asserted: banks differ."""
    spec = MB16 if wide else MB
    conn, n_active = mb_model(name, spec)
    t = train_case(name)
    ones = np.ones(spec["n_kc"], np.uint8)
    wts = np.stack([H.train(ones, np.ascontiguousarray(t["scenes"][t["first"][r]][..., channel]), conn, n_active) for r in range(3)])
    assert all((wts[a] != wts[b]).any() for a in range(3) for b in range(a + 1, 3)), (name, channel)
    wts.setflags(write=False)
    return conn, n_active, wts


@functools.lru_cache(maxsize=None)
def im_banks(name, channel):
    """(W0, Ws float64[3, M, N]): the statement, bank r trained from W0 on route r's host-sensed planes in the route's order."""
    w, h = SENSORS[name]["sensor"]
    W0 = HI.initial_weights(IM["n_hidden"][name], w * h, IM["seed"])
    t = train_case(name)
    Ws = np.stack([HI.train(W0, np.ascontiguousarray(t["scenes"][t["first"][r]][..., channel]), eta=IM["eta"]) for r in range(3)])
    assert np.isfinite(Ws).all() and not np.array_equal(Ws[0], Ws[1]) and not np.array_equal(Ws[1], Ws[2])
    W0.setflags(write=False)
    Ws.setflags(write=False)
    return W0, Ws


# ---- steps ---------------------------------------------------------------------------------------------------------------------------------
LAYOUTS = ((1, 16), (5, 13), (2, 260))
WIDE_LAYOUT = (683, 12)                                     # 8196 columns: column 8192, a launch's and a slab's edge, is inside member 682


@functools.lru_cache(maxsize=None)
def step_case(name, n, A):
    """n members x A headings -> dict(xs, ys, angs [n, A], banks, lands, planes uint8[n, A, h, w, 3] (host model, own landscape)).
    Members take STEP_BANKS / STEP_LANDS in turn: the banks' order is not the members', so a sort by bank permutes the landscapes.
    The members stand at a few places inside every landscape and look along a few headings, so that the host model senses each distinct
    (place, heading, landscape) once.
    Asserted: bank order differs from member order where n > 2; every plane differs between the member's landscape and the landscape
    of member 0 where those differ (so a table read at a launch-local index shows)."""
    rng = np.random.default_rng(100 * n + A)
    n_places = min(n, 8)
    place_x, place_y = rng.uniform(50, 120, n_places), rng.uniform(50, 120, n_places)
    heads = rng.uniform(0, 2 * np.pi, (n_places, A))
    place = np.arange(n) % n_places
    xs, ys, angs = place_x[place], place_y[place], heads[place]
    banks = np.array([STEP_BANKS[i % 5] for i in range(n)], dtype=np.int32)
    land_of = np.array([STEP_LANDS[i % 5] for i in range(n)], dtype=np.int32)
    if n == WIDE_LAYOUT[0]:
        assert land_of[n - 1] != land_of[0] and (n - 1) * A < 8192 < n * A
    if n > 2:
        assert (np.argsort(banks, kind="stable") != np.arange(n)).any()
    w, h = SENSORS[name]["sensor"]
    cache = {}
    planes = np.empty((n, A, h, w, 3), dtype=np.uint8)
    for i in range(n):
        for a in range(A):
            k = (int(place[i]), a, int(land_of[i]))
            if k not in cache:
                cache[k] = host_scene(name, xs[i], ys[i], angs[i, a], land_of[i])
            planes[i, a] = cache[k]
    i = n - 1
    if land_of[i] != land_of[0]:
        assert not np.array_equal(planes[i, A - 1], host_scene(name, xs[i], ys[i], angs[i, A - 1], land_of[0]))
    for a in (xs, ys, angs, banks, land_of, planes):
        a.setflags(write=False)
    return dict(xs=xs, ys=ys, angs=angs, banks=banks, lands=land_of, planes=planes)


def mb_statement(name, channel, case, wide=False):
    """float64[n, A]: the mushroom statement on the case's host-sensed planes, member i under bank banks[i]."""
    conn, n_active, wts = mb_banks(name, channel, wide)
    planes = case["planes"][..., channel]
    n, A = planes.shape[:2]
    flat, inv = np.unique(planes.reshape(n * A, -1), axis=0, return_inverse=True)
    flat = flat.reshape((-1,) + planes.shape[2:])
    nov = np.stack([HE.novelty(w, flat, conn, n_active) for w in wts])                # [bank, distinct plane]
    return (-nov[np.repeat(case["banks"], A), inv.reshape(-1)]).astype(np.float64).reshape(n, A)


def im_statement(name, channel, case):
    _, Ws = im_banks(name, channel)
    planes = case["planes"][..., channel]
    n, A = planes.shape[:2]
    flat, inv = np.unique(planes.reshape(n * A, -1), axis=0, return_inverse=True)
    flat = flat.reshape((-1,) + planes.shape[2:])
    fam = np.stack([HI.familiarity(W, flat) for W in Ws])
    return fam[np.repeat(case["banks"], A), inv.reshape(-1)].reshape(n, A)


def flag_case(name):
    """The 5 x 13 layout with member 2 moved to ON_L2_OFF_L1's place and put on L1: off its own landscape, though on L2 and L0."""
    c = step_case(name, 5, 13)
    xs, ys, land_of = c["xs"].copy(), c["ys"].copy(), c["lands"].copy()
    xs[2], ys[2], land_of[2] = ON_L2_OFF_L1[0], ON_L2_OFF_L1[1], 1
    for a in range(13):
        assert is_off(name, xs[2], ys[2], c["angs"][2, a], 1) and not is_off(name, xs[2], ys[2], c["angs"][2, a], 2)
    return xs, ys, land_of


# ---- ensembles -------------------------------------------------------------------------------------------------------------------------------
ENS_SENSOR = (12, 10)
ENS_CURVES, ENS_POINTS = ((0.2, 0.5), (0.3, 0.45), (0.25, 0.4)), ((30, 26), (24, 28), (22, 27))


def ens_routes():
    """[(landscape_index, route)]: two routes on each of three landscapes (six banks)."""
    from navsim_amd import synth
    return [(l, synth.sin_training_path(ENS_CURVES[l][k], 60, 180, arclen=1.0)[:ENS_POINTS[l][k]]) for l in range(3) for k in range(2)]


def ens_starts(routes):
    """Two starts a route: on it at its fourth point, and beside its eleventh: (route_index, (x, y), angle)."""
    out = []
    for r, (_, path) in enumerate(routes):
        for k, (dx, dy, da) in ((3, (0.0, 0.0, 0.0)), (10, (-0.5, 0.6, -0.2))):
            d = path[k + 1] - path[k]
            out.append((r, (float(path[k][0] + dx), float(path[k][1] + dy)), float((np.arctan2(d[1], d[0]) + da) % (2 * np.pi))))
    return out


EDGE_START = ((168.0, 100.0), 0.0)                          # past L1's bound (173 - 6 columns), well inside a 300 x 300 landscape


FOOTPRINT_START = ((166.7, 100.0), 0.0)                     # inside L1's bounds; a corner of the 12 x 10 footprint reaches past column 172


def footprint_facts():
    """At FOOTPRINT_START the agent's own bounds test on L1 passes, and the host model raises IndexError for some, not all, of the nine
    headings the agent tests there: the member is flagged by the device, not stopped by its bounds."""
    import navsim_amd
    a = navsim_amd.NavBySceneFamiliarity(np.array(lands()[1]), ENS_SENSOR, 1.0, n_test_angles=9, use_gpu_sensor=False, familiarity_model=_keep)
    pos, ang = FOOTPRINT_START
    a.position, a.angle = pos, ang
    _, _, headings = a.headings_to_test()                       # (raises where the bounds test stops the agent)
    off = []
    for h in headings:
        try:
            a.get_sensor_mat(pos, h)
            off.append(False)
        except IndexError:
            off.append(True)
    assert any(off) and not all(off), off
    return off


def ens_facts(landscapes):
    """Every route lies inside its own landscape's bounds for the ensemble's sensor; EDGE_START is out of L1's bounds and in L0's."""
    r = max(ENS_SENSOR) / 2
    for l, path in ens_routes():
        rows, cols = landscapes[l].shape[:2]
        assert (path[:, 0] > r).all() and (path[:, 1] > r).all() and (path[:, 0] < cols - r).all() and (path[:, 1] < rows - r).all(), l
    (x, y), _ = EDGE_START
    assert x >= 173 - r and r < x < 300 - r and r < y < 211 - r
