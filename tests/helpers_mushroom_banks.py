"""Inputs of the memory-bank tests of the mushroom-body model (tests/test_mushroom_banks_host.py, tests/test_gpu_mushroom_banks.py) and
the NumPy statement (tests/helpers_mushroom.py) on them, computed once.  Nothing here comes from the device.

Banks.  R = 3 memories behind one connectivity; bank r is H.train(ones, views[bank_of == r]): the statement of one model, applied to
the views dealt to the bank.  The views of H.case_data(key) are dealt out as view v -> bank v % 3.

Conditions, asserted here on the CPU so that no GPU test can pass on the wrong bank:
  - the banks' weights differ pairwise (bank_data);
  - at most a quarter of a case's patches score equally under all banks (bank_data, for QUARTER_KEYS; 5x3_k37 has two views and two
    patches, and is not held to it);
  - every member of every planted layout (at least 8 headings; in 7x1, where a novel patch may fire no depressed cell of any bank, at
    least one member) sits in a bank under which its best heading's score differs from the score of the same patch under at least
    one other bank (layout_data).  The member -> bank table starts from PATTERN and a member for which the condition fails under its
    pattern bank moves to another bank for which it holds (bank 0 tried last) -- decided by the statement alone.  The planted member (the last
    one, helpers_mushroom_ensemble) always sits in bank 0, where its planted view (view 0 of the case) was trained, so that its two
    planted headings are its two equal maxima of +0.0 under its own bank.

Bounds of a launch.  VIEW_BOUND: 8193 views of a 7x5 plane under a model of 300 cells, two distinct views repeated; the views' banks
are v % 3, so view 8192 (the one view of the second launch) is in bank 2 and view 0 in bank 0, and view 8192 alone is the second
view: a table read at the launch's own column would train it into bank 0.  BYTE_BOUND: 4097 planes of 128x128 (one more than 64 MiB
hold), the last one alone being the second view, in bank 4096 % 3 = 1."""
import functools

import numpy as np

from tests import helpers_infomax as HI
from tests import helpers_mushroom as H
from tests import helpers_mushroom_ensemble as HE

R = 3
KEYS = ("16x16_k1043", "7x5_k20000", "33x31_k4100_c16", "5x3_k37")
QUARTER_KEYS = ("16x16_k1043", "7x5_k20000", "33x31_k4100_c16", "128x128_k2049")
LAYOUTS = ((1, 16), (7, 1), (5, 13), (2, 65))
TIE_LAYOUT = (2, 260)
PATTERN = (2, 0, 1, 1, 0, 2, 1)
WIDE_KEY, WIDE_LAYOUT = HE.WIDE_KEY, HE.WIDE_LAYOUT


def deal(n):
    """int32[n]: view v -> bank v % R."""
    return (np.arange(n) % R).astype(np.int32)


def train_banks(views, bank_of, conn, n_active, K, n_banks=R):
    """uint8[n_banks, K]: the statement, bank by bank."""
    views, bank_of = np.asarray(views), np.asarray(bank_of)
    ones = np.ones(K, np.uint8)
    return np.stack([H.train(ones, views[bank_of == r], conn, n_active) if (bank_of == r).any() else ones.copy() for r in range(n_banks)])


@functools.lru_cache(maxsize=None)
def bank_data(key):
    """dict(views, bank_of, wts uint8[R, K], counts int[R], zeros int[R], nov int64[R, patches], equal_share, min_diff, + case_data)."""
    d = H.case_data(key)
    bank_of = deal(len(d["views"]))
    wts = train_banks(d["views"], bank_of, d["conn"], d["n_active"], d["K"])
    nov = np.stack([H.novelty(w, d["patches"], d["conn"], d["n_active"]) for w in wts])
    equal_share = float(np.mean((nov == nov[0]).all(axis=0)))
    min_diff = min(int((wts[a] != wts[b]).sum()) for a in range(R) for b in range(a + 1, R))
    assert min_diff > 0, key
    if key in QUARTER_KEYS:
        assert equal_share <= 0.25, (key, equal_share)
    for a in (wts, nov, bank_of):
        a.setflags(write=False)
    return dict(d, bank_of=bank_of, wts=wts, counts=np.bincount(bank_of, minlength=R), zeros=(wts == 0).sum(axis=1), nov=nov,
                equal_share=equal_share, min_diff=min_diff)


@functools.lru_cache(maxsize=None)
def layout_data(key, n, A):
    """dict(planes uint8[n,A,h,w], banks int32[n], fam float64[n,A] (member i under banks[i]), best int[n], nov_all int64[R,n,A],
    planted, wts, ...) of a member layout of helpers_mushroom_ensemble under the case's three banks."""
    b = bank_data(key)
    e = HE.ensemble_data(key, n, A)
    flat = e["planes"].reshape(n * A, e["h"], e["w"])
    nov_all = np.stack([HE.novelty(w, flat, b["conn"], b["n_active"]).reshape(n, A) for w in b["wts"]])
    banks = np.zeros(n, dtype=np.int32)

    def distinguishes(r, i):
        best = int(np.argmin(nov_all[r, i]))                                              # (argmax of -d: the first of equals)
        return any(nov_all[o, i, best] != nov_all[r, i, best] for o in range(R) if o != r)

    for i in range(n):
        first = 0 if i == e["planted"] else PATTERN[i % len(PATTERN)]
        if e["planted"] is None:
            banks[i] = first                              # 7x1: a novel patch may fire no depressed cell of any bank; PATTERN as it is
            continue
        for r in ([first] if i == e["planted"] else [first] + sorted((r for r in range(R) if r != first), reverse=True)):   # (bank 0 last)
            if distinguishes(r, i):
                banks[i] = r
                break
        else:
            raise AssertionError("no bank distinguishes member %d of %s %dx%d" % (i, key, n, A))
    assert any(distinguishes(int(banks[i]), i) for i in range(n)), (key, n, A)
    nov = nov_all[banks, np.arange(n)]
    fam = (-nov).astype(np.float64)
    best = np.argmax(fam, axis=1)
    if e["planted"] is not None:
        p, (a0, a1) = e["planted"], HE.planted_headings(A)
        assert banks[p] == 0 and np.flatnonzero(fam[p] == fam[p].max()).tolist() == [a0, a1] and best[p] == a0, (key, n, A)
        assert H.bits(fam[p, a0:a0 + 1])[0] == 0                                          # +0.0
    if n > 1:
        assert len(set(banks.tolist())) > 1, (key, n, A)                                  # the members sit in different banks
    for a in (nov_all, banks, fam, best):
        a.setflags(write=False)
    return dict(planes=e["planes"], banks=banks, fam=fam, best=best, nov_all=nov_all, planted=e["planted"], wts=b["wts"], conn=b["conn"],
                n_active=b["n_active"], h=e["h"], w=e["w"], views=b["views"], bank_of=b["bank_of"])


# ---- the two bounds of a launch ----------------------------------------------------------------------------------------------------------
VIEW_BOUND = dict(w=7, h=5, K=300, c=4, n_active=6, seed=91)


@functools.lru_cache(maxsize=None)
def view_bound_data():
    """dict(two uint8[2,5,7], pick int[8193] (training: which of the two each view is), bank_of int32[8193], wts uint8[3,K],
    step_pick int[3, 2731], step_banks, fam float64[3, 2731], best, conn, n_active, h, w)."""
    m = VIEW_BOUND
    views, _ = H.slab_views()
    n = views + 1
    conn = H.connectivity(m["K"], m["w"] * m["h"], m["c"], m["seed"])
    two = H.route_views(m["seed"], 2, m["h"], m["w"])
    pick = np.zeros(n, dtype=np.int64)
    pick[-1] = 1
    bank_of = deal(n)
    assert bank_of[views] == 2 and bank_of[0] == 0
    ones = np.ones(m["K"], np.uint8)
    first, both = H.train(ones, two[:1], conn, m["n_active"]), H.train(ones, two, conn, m["n_active"])
    assert not np.array_equal(first, both)
    wts = np.stack([first, first, both])                                                  # (view 8192, the second view, is bank 2's)
    nov = np.stack([H.novelty(w, two, conn, m["n_active"]) for w in wts])                 # [bank, which view]
    assert nov[:, 0].tolist() == [0, 0, 0] and nov[0, 1] > 0 and nov[1, 1] > 0 and nov[2, 1] == 0
    # the step: members 0 and 1 as helpers_mushroom_ensemble.slab_data (novel but for one heading); member 2, in bank 2, sees the
    # second view everywhere: 0 under its own bank, d > 0 under bank 0 -- which column 8192 would get from a launch-local index
    step_pick = np.ones((HE.SLAB_MEMBERS, HE.SLAB_HEADINGS), dtype=np.int64)
    step_pick[0, -1] = 0
    step_pick[1, 1500] = 0
    step_banks = np.array([0, 1, 2], dtype=np.int32)
    fam = (-nov[step_banks[:, None], step_pick]).astype(np.float64)
    best = np.argmax(fam, axis=1)
    assert best.tolist() == [HE.SLAB_HEADINGS - 1, 1500, 0] and step_pick.size == n
    return dict(two=two, pick=pick, bank_of=bank_of, wts=wts, step_pick=step_pick, step_banks=step_banks, fam=fam, best=best, conn=conn,
                n_active=m["n_active"], h=m["h"], w=m["w"], K=m["K"])


BYTE_MEMBERS, BYTE_HEADINGS = 17, 241                                                     # 4097 columns


@functools.lru_cache(maxsize=None)
def byte_bound_data():
    """dict(two, pick int[4097], bank_of, wts, step_pick int[17, 241], step_banks, fam, best, ...): helpers_mushroom.SLAB_TRAIN's two
    128x128 views; the last plane alone is the second view, in bank 1.  In the step the last column (member 16, bank 1) is the second
    view, 0 under bank 1 and d > 0 under bank 0; member 5 (bank 2) sees it at heading 100, where it is novel."""
    t = H.slab_train_data()
    _, stage = H.slab_views()
    n = stage // t["N"] + 1
    assert n == BYTE_MEMBERS * BYTE_HEADINGS
    pick = np.zeros(n, dtype=np.int64)
    pick[-1] = 1
    bank_of = deal(n)
    assert bank_of[-1] == 1
    wts = np.stack([t["first"], t["both"], t["first"]])
    nov = np.stack([H.novelty(w, t["two"], t["conn"], t["n_active"]) for w in wts])
    assert nov[:, 0].tolist() == [0, 0, 0] and nov[0, 1] > 0 and nov[1, 1] == 0 and nov[2, 1] > 0
    step_pick = pick.reshape(BYTE_MEMBERS, BYTE_HEADINGS).copy()
    step_pick[5, 100] = 1
    step_banks = deal(BYTE_MEMBERS)
    assert step_banks[16] == 1 and step_banks[5] == 2 and step_banks[0] == 0
    fam = (-nov[step_banks[:, None], step_pick]).astype(np.float64)
    assert fam[16, -1] == 0.0 and fam[5, 100] < 0 and (np.delete(fam.reshape(-1), 5 * BYTE_HEADINGS + 100) == 0).all()
    return dict(two=t["two"], pick=pick, bank_of=bank_of, wts=wts, step_pick=step_pick, step_banks=step_banks, fam=fam,
                best=np.argmax(fam, axis=1), conn=t["conn"], n_active=t["n_active"], h=t["h"], w=t["w"], K=t["K"])


# ---- sensed banks: the 32x32 sensor of helpers_infomax.SENSED ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sensed_banks(name):
    """(conn, n_active, wts uint8[3, K], bank_of): HE.SENSED_MODELS[name] with the host-sensed views of the route dealt v % 3."""
    m = HE.SENSED_MODELS[name]
    conn, n_active, _ = HE.sensed_model(name)
    views = HI.sensed_data()["views"]
    bank_of = deal(len(views))
    wts = train_banks(views, bank_of, conn, n_active, m["n_kc"])
    assert all((wts[a] != wts[b]).any() for a in range(R) for b in range(a + 1, R))
    return conn, n_active, wts, bank_of


def sensed_statement(name, xs, ys, angs, banks):
    """float64[n, A]: the statement on the host sensor model's planes, member i under bank banks[i]."""
    conn, n_active, wts, _ = sensed_banks(name)
    n, A = angs.shape
    planes = H.host_sensed_planes(np.repeat(xs, A), np.repeat(ys, A), angs.reshape(-1)).reshape(n, A, 32, 32)
    return np.stack([(-HE.novelty(wts[banks[i]], planes[i], conn, n_active)).astype(np.float64) for i in range(n)])


# ---- routes of the ensemble tests: sin_training_path at three curves on the tests' synthetic landscape -------------------------------
CURVES = (0.2, 0.5, 0.8)
ROUTE_POINTS = (45, 40, 35)                                                               # lengths differ: so do the members' frames


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
