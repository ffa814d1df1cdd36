"""Inputs of the sensor-table tests (tests/test_sensors_host.py, tests/test_gpu_sensors.py) and the expected values on them, computed once.

Nothing here comes from the device: a view is the HOST sensor model's (navsim_amd.agent with use_gpu_sensor=False) under that pose's
own sensor entry on that pose's own landscape alone, and the models' values are the NumPy statements of tests/helpers_mushroom.py and
tests/helpers_infomax.py.  The landscapes are helpers_lands.lands().

Sensor shapes (SHAPES): "wide" 16 x 8 -- 128 pixels, half a wavefront of the sensing kernel a pose; "thin" 6 x 5 -- 30 pixels, so a
wavefront spans poses of different entries (the reference asserts that the pixel extent is even, so ph is even in every entry).

Entries (ENTRIES), one per landscape of a set: E0 (1, 2) 5 levels mask 0; E1 (2, 4) 4 levels mask 1; E2 (3, 2) 256 levels mask 2;
E3 (2, 4) 2 levels mask 1 -- E1 but for its level table; E4 (1, 2) 5 levels mask 1 -- E0 but for its mask.  OWN is the engine's one
configuration, pixel (2, 2), 3 levels, mask 0: it equals none of the entries, so a kernel that reads the context's configuration
where it should read the table fails on every pose.

What the CPU test asserts of these inputs (so that a passing GPU test is not vacuous) is stated beside each function."""
import functools

import numpy as np

from tests import helpers_infomax as HI
from tests import helpers_lands as HL
from tests import helpers_mushroom as H
from tests import helpers_mushroom_ensemble as HE

SHAPES = {"wide": (16, 8), "thin": (6, 5)}
ENTRIES = {
    "E0": dict(pixel=(1, 2), levels=5, mask=0),
    "E1": dict(pixel=(2, 4), levels=4, mask=1),
    "E2": dict(pixel=(3, 2), levels=256, mask=2),
    "E3": dict(pixel=(2, 4), levels=2, mask=1),
    "E4": dict(pixel=(1, 2), levels=5, mask=1),
    "OWN": dict(pixel=(2, 2), levels=3, mask=0),
}
TABLE = ("E0", "E1", "E2", "E3")                            # entry l of the four-landscape set
SET5 = ((0, "E0"), (1, "E1"), (2, "E2"), (3, "E3"), (0, "E4"))   # (landscape of helpers_lands.lands(), entry): L0 entered twice
MB = dict(n_kc=1003, n_active=30, seed=91)
MB_FAN_IN = {"wide": 10, "thin": 6}
IM = dict(n_hidden={"wide": 20, "thin": 12}, eta=1e-3, seed=93)
N_BANKS = 3
SENSE_ERROR = 16


@functools.lru_cache(maxsize=None)
def _host_agent(shape, entry, l):
    """An agent whose sensor model runs on the host, with entry `entry`'s configuration, on landscape l of helpers_lands.lands() alone."""
    import navsim_amd
    c = ENTRIES[entry]
    agent = navsim_amd.NavBySceneFamiliarity(np.array(HL.lands()[l]), SHAPES[shape], 1.0, n_test_angles=9, sensor_pixel_dimensions=list(c["pixel"]),
                                             n_sensor_levels=c["levels"], mask_middle_n=c["mask"], use_gpu_sensor=False, familiarity_model=HL._keep)
    agent._check_bounds = lambda position: None                # the sensor model alone (helpers_lands._host_agent)
    return agent


def level_table(shape, entry):
    return _host_agent(shape, entry, 0)._level_tables()


def table_args(shape, entries):
    """(pixel_dimensions, luts, masks) of FamiliarityEngine.sensors_set for a list of entry names."""
    return ([ENTRIES[e]["pixel"] for e in entries], np.stack([level_table(shape, e) for e in entries]), [ENTRIES[e]["mask"] for e in entries])


def host_scene(shape, entry, x, y, angle, land):
    """uint8[h, w, 3]: the host model's view of one pose under `entry` on landscape `land` alone; IndexError where the model raises it."""
    return _host_agent(shape, entry, int(land)).get_sensor_mat((float(x), float(y)), float(angle)).copy()


def is_off(shape, entry, x, y, angle, land):
    try:
        host_scene(shape, entry, x, y, angle, land)
    except IndexError:
        return True
    return False


# ---- lands_sense under a table ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sense_case(shape):
    """helpers_lands.sense_case's 14 poses and deal over the four landscapes -> dict(x, y, angle, land_of, scenes under TABLE, own: the
    same poses under OWN, twice: views of the poses on landscape 0 under E4).
    Asserted: on every pose, on its own landscape, the six configurations give six different views."""
    rng = np.random.default_rng(11)
    n = 2 * len(HL.SENSE_PATTERN)
    x, y, ang = rng.uniform(45, 125, n), rng.uniform(45, 125, n), rng.uniform(0, 2 * np.pi, n)
    land_of = np.array(HL.SENSE_PATTERN * 2, dtype=np.int32)
    per = {e: np.stack([host_scene(shape, e, x[v], y[v], ang[v], land_of[v]) for v in range(n)]) for e in ENTRIES}
    names = sorted(ENTRIES)
    for v in range(n):
        for i, a in enumerate(names):
            for b in names[i + 1:]:
                assert not np.array_equal(per[a][v], per[b][v]), (shape, v, a, b)
    scenes = np.stack([per[TABLE[land_of[v]]][v] for v in range(n)])
    on0 = np.flatnonzero(land_of == 0)
    twice = np.stack([per["E4"][v] for v in on0])
    for a in (x, y, ang, land_of, scenes, twice):
        a.setflags(write=False)
    return dict(x=x, y=y, angle=ang, land_of=land_of, scenes=scenes, own=per["OWN"], on0=on0, twice=twice)


# ---- the footprint is the entry's own --------------------------------------------------------------------------------------------------------
FOOT_POSE = {"wide": (160.0, 100.0, np.pi / 2), "thin": (166.0, 100.0, np.pi / 2)}
FOOT_SET = ((0, "E1"), (1, "E0"), (1, "E2"))                # L1 entered twice: under E0 the pose is on it, under E2's larger footprint off it
FOOT_INSIDE = (90.0, 90.0, 0.7)


def foot_case(shape):
    """Four poses on FOOT_SET: FOOT_INSIDE on entry 0, FOOT_POSE on entry 1 (L1 under E0: sensed) and on entry 2 (L1 under E2: off),
    FOOT_INSIDE on entry 2 -> (x, y, angle, land_of, scenes with None at the pose that is off).
    Asserted: exactly pose 2 raises IndexError in the host model."""
    fx, fy, fa = FOOT_POSE[shape]
    ix, iy, ia = FOOT_INSIDE
    x, y, ang = np.array([ix, fx, fx, ix]), np.array([iy, fy, fy, iy]), np.array([ia, fa, fa, ia])
    land_of = np.array([0, 1, 2, 2], dtype=np.int32)
    scenes = []
    for v in range(4):
        l, e = FOOT_SET[land_of[v]]
        off = is_off(shape, e, x[v], y[v], ang[v], l)
        assert off == (v == 2), (shape, v)
        scenes.append(None if off else host_scene(shape, e, x[v], y[v], ang[v], l))
    return x, y, ang, land_of, scenes


# ---- training --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def train_case(shape):
    """helpers_lands.train_case's three interleaved routes (route r on landscape r, into bank r), their views under entry TABLE[r].
    Asserted: every view is on its landscape under its entry; the views differ from what OWN gives."""
    t = HL.train_case("sq")
    n = len(t["x"])
    scenes = np.stack([host_scene(shape, TABLE[t["land_of"][v]], t["x"][v], t["y"][v], t["angle"][v], t["land_of"][v]) for v in range(n)])
    own = np.stack([host_scene(shape, "OWN", t["x"][v], t["y"][v], t["angle"][v], t["land_of"][v]) for v in range(n)])
    assert all(not np.array_equal(scenes[v], own[v]) for v in range(n))
    scenes.setflags(write=False)
    return dict(t, scenes=scenes)


def mb_model(shape):
    w, h = SHAPES[shape]
    return H.connectivity(MB["n_kc"], w * h, MB_FAN_IN[shape], MB["seed"]), MB["n_active"]


@functools.lru_cache(maxsize=None)
def mb_banks(shape, channel=2):
    """(conn, n_active, wts uint8[3, K]): the statement, bank r trained on route r's planes.  Asserted: the banks differ."""
    conn, n_active = mb_model(shape)
    t = train_case(shape)
    ones = np.ones(MB["n_kc"], np.uint8)
    wts = np.stack([H.train(ones, np.ascontiguousarray(t["scenes"][t["first"][r]][..., channel]), conn, n_active) for r in range(3)])
    assert all((wts[a] != wts[b]).any() for a in range(3) for b in range(a + 1, 3)), shape
    wts.setflags(write=False)
    return conn, n_active, wts


@functools.lru_cache(maxsize=None)
def im_banks(shape, channel=2):
    """(W0, Ws float64[3, M, N]): the statement, bank r trained from W0 on route r's planes in the route's order."""
    w, h = SHAPES[shape]
    W0 = HI.initial_weights(IM["n_hidden"][shape], w * h, IM["seed"])
    t = train_case(shape)
    Ws = np.stack([HI.train(W0, np.ascontiguousarray(t["scenes"][t["first"][r]][..., channel]), eta=IM["eta"]) for r in range(3)])
    assert np.isfinite(Ws).all() and not np.array_equal(Ws[0], Ws[1]) and not np.array_equal(Ws[1], Ws[2])
    W0.setflags(write=False)
    Ws.setflags(write=False)
    return W0, Ws


# ---- steps -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def step_case(shape, n, A):
    """helpers_lands.step_case's members, banks and landscapes for the layout, the planes under each member's own entry (TABLE of its
    landscape) -> dict(xs, ys, angs [n, A], banks, lands, planes uint8[n, A, h, w, 3]).
    Asserted: where the last member's entry differs from member 0's, its last plane is not what member 0's entry gives there (so a
    table read at a launch-local column shows); every plane differs from OWN's."""
    rng = np.random.default_rng(100 * n + A)
    n_places = min(n, 8)
    place_x, place_y = rng.uniform(50, 120, n_places), rng.uniform(50, 120, n_places)
    heads = rng.uniform(0, 2 * np.pi, (n_places, A))
    place = np.arange(n) % n_places
    xs, ys, angs = place_x[place], place_y[place], heads[place]
    banks = np.array([HL.STEP_BANKS[i % 5] for i in range(n)], dtype=np.int32)
    land_of = np.array([HL.STEP_LANDS[i % 5] for i in range(n)], dtype=np.int32)
    if n == HL.WIDE_LAYOUT[0]:
        assert land_of[n - 1] != land_of[0] and (n - 1) * A < 8192 < n * A
    w, h = SHAPES[shape]
    cache = {}
    planes = np.empty((n, A, h, w, 3), dtype=np.uint8)
    for i in range(n):
        for a in range(A):
            k = (int(place[i]), a, int(land_of[i]))
            if k not in cache:
                cache[k] = host_scene(shape, TABLE[land_of[i]], xs[i], ys[i], angs[i, a], land_of[i])
                assert not np.array_equal(cache[k], host_scene(shape, "OWN", xs[i], ys[i], angs[i, a], land_of[i]))
            planes[i, a] = cache[k]
    i = n - 1
    if land_of[i] != land_of[0]:
        assert not np.array_equal(planes[i, A - 1], host_scene(shape, TABLE[land_of[0]], xs[i], ys[i], angs[i, A - 1], land_of[i]))
    for a in (xs, ys, angs, banks, land_of, planes):
        a.setflags(write=False)
    return dict(xs=xs, ys=ys, angs=angs, banks=banks, lands=land_of, planes=planes)


def _distinct(planes):
    n, A = planes.shape[:2]
    flat, inv = np.unique(planes.reshape(n * A, -1), axis=0, return_inverse=True)
    return flat.reshape((-1,) + planes.shape[2:]), inv.reshape(-1)


def mb_statement(shape, case, channel=2):
    """float64[n, A]: the mushroom statement on the case's planes, member i under bank banks[i]."""
    conn, n_active, wts = mb_banks(shape, channel)
    flat, inv = _distinct(case["planes"][..., channel])
    nov = np.stack([HE.novelty(w, flat, conn, n_active) for w in wts])
    return (-nov[np.repeat(case["banks"], case["planes"].shape[1]), inv]).astype(np.float64).reshape(case["planes"].shape[:2])


def im_statement(shape, case, channel=2):
    _, Ws = im_banks(shape, channel)
    flat, inv = _distinct(case["planes"][..., channel])
    fam = np.stack([HI.familiarity(W, flat) for W in Ws])
    return fam[np.repeat(case["banks"], case["planes"].shape[1]), inv].reshape(case["planes"].shape[:2])


def route_views(shape):
    """(views uint8[n, h, w, 3] route by route, first int64[4], x, y, angle, land_of in that order): the store of train_case's routes."""
    t = train_case(shape)
    order = np.concatenate(t["first"])
    first = np.concatenate([[0], np.cumsum([len(f) for f in t["first"]])]).astype(np.int64)
    return t["scenes"][order], first, t["x"][order], t["y"][order], t["angle"][order], t["land_of"][order]


# ---- ensembles -------------------------------------------------------------------------------------------------------------------------------
ENS_SENSORS = (None, dict(sensor_pixel_dimensions=[1, 2], n_sensor_levels=4, mask_middle_n=1), dict(sensor_pixel_dimensions=[2, 2], mask_middle_n=2))
ENS_AGENT = dict(sensor_pixel_dimensions=[1, 1], n_sensor_levels=5, mask_middle_n=0)


def ens_config(l):
    """The keyword arguments of a lone agent with landscape l's sensor: the agent's own values where the entry leaves a key out."""
    return dict(ENS_AGENT, **(ENS_SENSORS[l] or {}))


def ens_radius(l):
    c = ens_config(l)
    return max(HL.ENS_SENSOR[0] * c["sensor_pixel_dimensions"][0], HL.ENS_SENSOR[1] * c["sensor_pixel_dimensions"][1]) / 2


def ens_facts():
    """helpers_lands' ensemble routes lie inside their own landscapes under their own entry's footprint; the three footprints differ."""
    L = HL.lands()
    assert [ens_radius(l) for l in range(3)] == [6.0, 10.0, 12.0]
    for l, path in HL.ens_routes():
        r = ens_radius(l)
        rows, cols = L[l].shape[:2]
        assert (path[:, 0] > r).all() and (path[:, 1] > r).all() and (path[:, 0] < cols - r).all() and (path[:, 1] < rows - r).all(), l


# A start on L1 (211 x 173) that the agent's own 12 x 10 footprint (r = 6) keeps inside the bounds and entry 1's 12 x 20 footprint
# (r = 10) does not: x = 165 < 173 - 6, x >= 173 - 10.
EDGE_START = ((165.0, 100.0), 0.0)
# ... and one inside entry 1's bounds (x < 163) where a corner of the 12 x 20 footprint leaves L1 for some headings
FOOTPRINT_START = ((162.5, 100.0), 0.0)


EDGE_LANDS = (0, 1, 3)                                      # helpers_lands.lands() indices of the edge case's set; entry k = ENS_SENSORS[k]


def edge_routes():
    """[(landscape_index, route)]: helpers_lands' first three ensemble routes, one on each landscape of EDGE_LANDS."""
    return [(k, path) for k, (_, path) in zip(range(3), HL.ens_routes()[:3])]


def edge_facts():
    """The edge case's routes lie inside their landscapes under their own entries' footprints.  EDGE_START is out of L1's bounds under entry 1's footprint and inside them under the agent's own; at FOOTPRINT_START the bounds
    test of entry 1 passes and the host model raises IndexError for some, not all, of the nine headings tested there."""
    import navsim_amd
    for k, path in edge_routes():
        r = ens_radius(k)
        rows, cols = HL.lands()[EDGE_LANDS[k]].shape[:2]
        assert (path[:, 0] > r).all() and (path[:, 1] > r).all() and (path[:, 0] < cols - r).all() and (path[:, 1] < rows - r).all(), k
    (x, y), _ = EDGE_START
    assert 173 - ens_radius(1) <= x < 173 - 6.0 and ens_radius(2) < x < 300 - ens_radius(2)
    a = navsim_amd.NavBySceneFamiliarity(np.array(HL.lands()[1]), HL.ENS_SENSOR, 1.0, n_test_angles=9, use_gpu_sensor=False,
                                         familiarity_model=HL._keep, **ens_config(1))
    pos, ang = FOOTPRINT_START
    a.position, a.angle = pos, ang
    _, _, headings = a.headings_to_test()
    off = []
    for h in headings:
        try:
            a.get_sensor_mat(pos, h)
            off.append(False)
        except IndexError:
            off.append(True)
    assert any(off) and not all(off), off
    return off
