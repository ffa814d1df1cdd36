"""Inputs of the weight-bank tests of the Infomax model (tests/test_infomax_banks_host.py, tests/test_gpu_infomax_banks.py) and the NumPy
statement (tests/helpers_infomax.py) on them, computed once.  Nothing here comes from the device.

Banks.  R = 3 models of one shape and one learning rate; bank r is H.train(W0, views[bank_of == r]): the statement of one model, applied to
the views dealt to the bank, in the order they have among all views.  The views of H.case_data(key) are dealt out by the repeating
PATTERN (2, 0, 1, 1, 0, 2, 1): view v -> bank PATTERN[v % 7], so that the banks' chains differ in length and interleave.  5x3_f2 has two
views: bank 1 stays empty and keeps W0.  7x5_m1043 has three: one view a bank.

Members.  A layout (n, A) is uint8[n, A, h, w]: windows of a random 5-level strip the case's models have not seen, and at heading
(3 i + 1) % A of member i one view that member's own bank was trained on (any view where the bank is empty).  Member i sits in bank
PATTERN[i % 7].  Columns go to the device in blocks of 64 that never mix banks.  In (2, 65) each member overflows a block of its own: a
block boundary inside a bank's run.  In (5, 13) column 64 of the caller's order lies inside member 4, whose bank 0 also holds member 1:
the bank's run is gathered from members that are no neighbours, as bank 1's (members 2, 3) and bank 2's (member 0, listed first) are.
(3, 60) has a ragged last tile in every block; in (7, 1) the banks have 2, 3 and 2 columns, far less than a 16-column tile.

Conditions, asserted in tests/test_infomax_banks_host.py on the CPU so that no GPU test can pass on the wrong bank or the wrong order:
  - under a wrong bank's W every member's best heading changes or one of its scores moves by more than 1000 TOL (relative);
  - every member's best heading leads its second best by more than 1000 TOL (relative) under its own bank;
  - every bank's chain of every case, in float64 against longdouble and against a permuted order of every sum: 1000 x the largest
    discrepancy stays under H.TOL (the rule TOL was made by; the chains here are parts of the chains it was measured on).
Measured (x86-64, OpenBLAS NumPy), the largest of a case's banks, weights / scores:

    5x3_f2       8.9e-17 / 4.1e-16        7x5_m1043    8.3e-16 / 1.2e-16
    40x1         3.7e-16 / 1.3e-16        33x31        1.1e-16 / 4.8e-16
    16x16_a16    8.3e-16 / 3.8e-16        32x32_m1040  3.7e-16 / 2.2e-16
    sensed routes (32x32, 70 rows, 15 / 9 / 12 views at 1e-3)   3.6e-16 (weights)

The largest is 8.3e-16, under the 1.37e-15 TOL was rounded up from.  The least margin of a best heading over all cases and layouts is
2.2e-3 (33x31, 3 x 60), far above 1000 TOL = 2e-9.
"""
import functools

import numpy as np

from tests import helpers_infomax as H

R = 3
PATTERN = (2, 0, 1, 1, 0, 2, 1)
KEYS = ("5x3_f2", "40x1", "16x16_a16", "7x5_m1043", "33x31", "32x32_m1040")
LAYOUTS = ((1, 16), (7, 1), (5, 13), (3, 60), (2, 65))
SEED = 7000                                                        # of the members' strips


def deal(n):
    """int32[n]: entry v -> bank PATTERN[v % 7]."""
    return np.array([PATTERN[v % len(PATTERN)] for v in range(n)], dtype=np.int32)


def train_banks(W0, views, bank_of, eta=H.ETA, n_banks=R, **kw):
    """[n_banks] arrays [M, N]: the statement, bank by bank (an empty bank keeps W0)."""
    views, bank_of = np.asarray(views), np.asarray(bank_of)
    return [H.train(W0, views[bank_of == r], eta=eta, **kw) for r in range(n_banks)]


@functools.lru_cache(maxsize=None)
def bank_data(key):
    """dict(views, bank_of, Ws [R] of float64[M, N], counts int[R], + case_data)."""
    d = H.case_data(key)
    bank_of = deal(len(d["views"]))
    Ws = train_banks(d["W0"], d["views"], bank_of)
    for a in Ws + [bank_of]:
        a.setflags(write=False)
    return dict(d, bank_of=bank_of, Ws=Ws, counts=np.bincount(bank_of, minlength=R))


def bank_discrepancies(key):
    """(weights, scores): the float64 statement of every bank's chain of a case against longdouble and against a permuted order of the
    sums -- the largest over the banks, relative (as H.discrepancies takes them for the one chain of a case)."""
    b = bank_data(key)
    worst_w = worst_d = 0.0
    for r in range(R):
        fam = H.familiarity(b["Ws"][r], b["patches"])
        for kw in (dict(dtype=np.longdouble), dict(order_seed=99)):
            W2 = H.train(b["W0"], b["views"][b["bank_of"] == r], **kw)
            worst_w = max(worst_w, float(np.max(np.abs(W2 - b["Ws"][r])) / np.max(np.abs(b["Ws"][r]))))
            f2 = H.familiarity(b["Ws"][r], b["patches"], **kw)
            worst_d = max(worst_d, float(np.max(np.abs(f2 - fam)) / np.max(np.abs(fam))))
    return worst_w, worst_d


@functools.lru_cache(maxsize=None)
def layout_data(key, n, A):
    """dict(planes uint8[n,A,h,w], banks int32[n], fam_all float64[R,n,A] (every member under every bank), fam float64[n,A] (member i
    under banks[i]), best int[n], Ws, h, w, W0)."""
    b = bank_data(key)
    h, w = b["h"], b["w"]
    planes = H.route_views(SEED + b["seed"] * 100 + n * 7 + A, n * A, h, w).reshape(n, A, h, w).copy()
    banks = deal(n)
    for i in range(n):
        own = b["views"][b["bank_of"] == banks[i]]
        planes[i, (3 * i + 1) % A] = own[(5 * i + 1) % len(own)] if len(own) else b["views"][0]
    flat = planes.reshape(n * A, h, w)
    fam_all = np.stack([H.familiarity(W, flat).reshape(n, A) for W in b["Ws"]])
    fam = fam_all[banks, np.arange(n)]
    best = np.argmax(fam, axis=1)
    for a in (planes, banks, fam_all, fam, best):
        a.setflags(write=False)
    return dict(planes=planes, banks=banks, fam_all=fam_all, fam=fam, best=best, Ws=b["Ws"], h=h, w=w, W0=b["W0"])


def wrong_bank_shows(fam_all, banks, i, r):
    """Does scoring member i under bank r instead of its own change its best heading or move a score by more than 1000 TOL, relative?"""
    own, other = fam_all[banks[i], i], fam_all[r, i]
    return bool(np.argmax(own) != np.argmax(other) or np.max(np.abs(own - other) / np.abs(own)) > 1000 * H.TOL)


# ---- steps past one launch, without a network table: the layouts of tests/helpers_inet.py under banks of one shape -------------------------
# SLAB: helpers_inet.SLAB's 688 members x 12 headings of 32 x 32 views over four banks (the byte bound: launch 2 begins at column 8176,
# inside a member of bank 1), every bank with M = 24 rows (a ragged second row tile) and trained weights of its own.
# BLOCKS: helpers_inet.BLOCKS' 16385 banks of one member x 3 headings of 7 x 5 views (the block-count bound: 16384 blocks and one), M = 15,
# banks 0, 16383 and 16384 trained.  Measured as the table above, weights / scores: SLAB 2.4e-16 / 6.5e-16, BLOCKS 1.7e-16 / 5.7e-16.
SLAB = dict(M=24, eta=0.02, seed=471)
BLOCKS = dict(M=15, eta=0.01, seed=481)


@functools.lru_cache(maxsize=None)
def slab_step_data():
    """dict(W0, Ws [4], views, bank_of, planes uint8[688,12,32,32], banks, fam, first, second, margin, h, w): helpers_inet.slab_members
    under four banks of one shape, bank b trained from W0 on the views helpers_inet.slab_deal() gives it."""
    from tests import helpers_inet as HN
    t = HN.SLAB
    W0 = H.initial_weights(SLAB["M"], t["w"] * t["h"], SLAB["seed"])
    views = H.route_views(SLAB["seed"] + 10, sum(t["trained"]), t["h"], t["w"])
    bank_of = HN.slab_deal()
    Ws = train_banks(W0, views, bank_of, eta=SLAB["eta"], n_banks=len(t["members"]))
    assert all(np.isfinite(W).all() for W in Ws)
    assert all(HN.rel(Ws[a], Ws[b]) > 1e-6 for a in range(4) for b in range(a + 1, 4)) and all(HN.rel(W, W0) > 1e-6 for W in Ws)
    banks = HN.slab_layout()["banks"]
    planes, fam, first, second, margin = HN.slab_members(lambda p: slab_scores(Ws, p, banks))
    for a in [W0, views, bank_of] + Ws:
        a.setflags(write=False)
    return dict(W0=W0, Ws=Ws, views=views, bank_of=bank_of, planes=planes, banks=banks, fam=fam, first=first, second=second, margin=margin,
                h=t["h"], w=t["w"])


def slab_scores(Ws, planes, banks, **kw):
    return np.stack([H.familiarity(Ws[b], planes[i], **kw) for i, b in enumerate(banks)])


@functools.lru_cache(maxsize=None)
def blocks_data():
    """dict(W0, trained {bank: W}, fam float64[16385, 3], + helpers_inet.blocks_layout()): every bank W0 but the three trained ones."""
    from tests import helpers_inet as HN
    lay = HN.blocks_layout()
    W0 = H.initial_weights(BLOCKS["M"], lay["N"], BLOCKS["seed"])
    trained = {b: H.train(W0, lay["views"][lay["bank_of"] == b], eta=BLOCKS["eta"]) for b in HN.BLOCKS["trained"]}
    assert all(np.isfinite(W).all() and HN.rel(W, W0) > 1e-6 for W in trained.values())
    fam = blocks_scores(W0, trained)
    for a in [W0, fam] + list(trained.values()):
        a.setflags(write=False)
    return dict(lay, W0=W0, trained=trained, fam=fam, h=HN.BLOCKS["h"], w=HN.BLOCKS["w"])


def blocks_scores(W0, trained, **kw):
    from tests import helpers_inet as HN
    lay = HN.blocks_layout()
    return HN.blocks_scores(lay, np.zeros(len(lay["banks"]), dtype=np.int32), [W0], trained, **kw)


# ---- sensed banks: three short routes of unequal length on helpers_infomax.SENSED's landscape, its 32x32 sensor -----------------------
CURVES = (0.2, 0.5, 0.8)
SENSED_POINTS = (15, 9, 12)
SENSED_MODEL = dict(learning_rate=H.SENSED["eta"], seed=23, n_hidden=70)


def sensed_routes():
    from navsim_amd import synth
    return [synth.sin_training_path(c, 60, 180, arclen=1.0)[:k] for c, k in zip(CURVES, SENSED_POINTS)]


def route_headings(route):
    """The heading of every view of a route, as train_from_path takes them: towards the next point, the last one once more."""
    steps = route[1:] - route[:-1]
    h = np.arctan2(steps[:, 1], steps[:, 0])
    return h[np.minimum(np.arange(len(route)), len(route) - 2)]


def interleaved_poses():
    """(x, y, angle, bank_of_view, first): the three routes' poses dealt into ONE call with their views interleaved (route r's k-th view
    keeps its place among r's views); first[r] = the places of r's views in the call."""
    routes = sensed_routes()
    order = sorted((k * R + r, r, k) for r, route in enumerate(routes) for k in range(len(route)))       # round-robin while they last
    x = np.array([routes[r][k][0] for _, r, k in order])
    y = np.array([routes[r][k][1] for _, r, k in order])
    heads = [route_headings(route) for route in routes]
    ang = np.array([heads[r][k] for _, r, k in order])
    bank_of = np.array([r for _, r, _ in order], dtype=np.int32)
    return x, y, ang, bank_of, [np.flatnonzero(bank_of == r) for r in range(R)]


@functools.lru_cache(maxsize=None)
def sensed_data():
    """dict(scenes [R] of uint8[n_r,32,32,3] as the HOST sensor model takes them, W0, Ws [R]): the statement on the routes' V planes."""
    def keep(scenes):
        def func(scene, fambuf):
            fambuf[...] = 0.0
        func.max_familiarity = 0.0
        return func

    scenes = []
    for route in sensed_routes():
        agent = H.sensed_agent(keep, False)
        agent.train_from_path(route)
        scenes.append(np.array(agent.familiar_scenes))
    m = SENSED_MODEL
    W0 = H.initial_weights(m["n_hidden"], 32 * 32, m["seed"])
    Ws = [H.train(W0, np.ascontiguousarray(s[..., 2]), eta=m["learning_rate"]) for s in scenes]
    for a in scenes + Ws + [W0]:
        a.setflags(write=False)
    return dict(scenes=scenes, W0=W0, Ws=Ws)


def sensed_discrepancy():
    s = sensed_data()
    return max(H.chain_discrepancy(s["W0"], np.ascontiguousarray(sc[..., 2]), W, SENSED_MODEL["learning_rate"])
               for sc, W in zip(s["scenes"], s["Ws"]))


# ---- routes of the ensemble tests: sin_training_path at three curves on the tests' synthetic landscape, a 16x16 sensor ----------------
ROUTE_POINTS = (45, 40, 35)                                                               # lengths differ: so do the members' frames
ENSEMBLE_SENSOR = (16, 16)
ENSEMBLE_MODEL = dict(learning_rate=1e-3, seed=9)


def routes():
    from navsim_amd import synth
    return [synth.sin_training_path(c, 60, 180, arclen=1.0)[:k] for c, k in zip(CURVES, ROUTE_POINTS)]


def starts(paths):
    """Two starts a route: on it at its fourth point, and beside its eleventh: (route_index, (x, y), angle)."""
    out = []
    for r, path in enumerate(paths):
        for k, (dx, dy, da) in ((3, (0.0, 0.0, 0.0)), (10, (-0.5, 0.6, -0.2))):
            d = path[k + 1] - path[k]
            out.append((r, (float(path[k][0] + dx), float(path[k][1] + dy)), float((np.arctan2(d[1], d[0]) + da) % (2 * np.pi))))
    return out
