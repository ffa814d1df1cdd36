"""Inputs of the mushroom-body ensemble tests (tests/test_mushroom_ensemble_host.py, tests/test_gpu_mushroom_ensemble.py): the patch
sets of every case and member layout, and the NumPy statement (tests/helpers_mushroom.py) on them, computed once.

A patch set is uint8[n, A, h, w]: windows of a random 5-level strip that the case's model has not seen (novel), and in it
  - every ordinary member i carries ONE trained view, at heading (3 i + 1) % A, so that its best heading is decided by the model and
    not by the order of the patches (with one heading per member only the even members do: the odd ones keep their novel patch, or
    every column of the layout would score 0);
  - the planted member (the last one, in layouts of at least 8 headings) carries the SAME trained view at two headings (2 and 7; 5 and
    257 in the layout of 260 headings, which k_mb_decide_batch's threads 5 and 1 hold: the later heading in the lower thread) and,
    everywhere else, the first windows of a strip of its own that the statement scores with d > 0: two equal maxima of +0.0, of which
    np.argmax takes the first.
Three conditions are asserted here, on the CPU, so that no test can pass on a kernel that returns 0 everywhere or heading 0 always:
in every layout of more than one heading (with one heading there is only heading 0) at least one member's expected best heading is
not 0; the planted member's maximum is attained at exactly its two planted headings, the first of which is not heading 0; and every
case and layout has a column with d > 0.  SEED is chosen so that the statement alone satisfies all of this.

Outside the layouts: SLAB, two distinct 5x3 planes repeated over three members x 2731 headings = 8193 columns, one more than a launch
takes, so the statement is computed for two; BYTES, the same with tests/helpers_mushroom.SLAB_TRAIN's 128x128 planes, 4097 of them,
one more than 64 MiB of staged bytes hold; and the models of the sensed tests on the 32x32 sensor of helpers_infomax.SENSED."""
import functools

import numpy as np

from tests import helpers_infomax as HI
from tests import helpers_mushroom as H

KEYS = ("5x3_k37", "16x16_k1043", "7x5_k20000", "33x31_k4100_c16")
# (n_agents, A): a single member; one heading per member; members that are no multiple of anything; a member wider than a wave; a
# member wider than k_mb_decide_batch's workgroup
LAYOUTS = ((1, 16), (7, 1), (5, 13), (2, 65), (2, 260))
WIDE_KEY, WIDE_LAYOUT = "256x256_k1043_c16", (2, 3)              # 130 896 bytes of LDS a workgroup
CASES = tuple((k, n, A) for k in KEYS for n, A in LAYOUTS) + ((WIDE_KEY,) + WIDE_LAYOUT,)
SEED = 7000                                                       # of the novel strips

# sensed tests: a 32x32 sensor; the second model's fan-in of 16 takes 1024 + 4 * 4081 * 4 + 64 = 66 384 bytes of LDS
SENSED_MODELS = dict(c10=dict(n_kc=4100, fan_in=10, sparsity=0.01, seed=41), c16=dict(n_kc=2049, fan_in=16, sparsity=0.02, seed=43))
SLAB_MEMBERS, SLAB_HEADINGS = 3, 2731                             # 8193 columns


def planted_member(n, A):
    return n - 1 if A >= 8 else None


def planted_headings(A):
    return (5, 257) if A > 257 else (2, 7)


def novelty(wt, planes, conn, n_active, chunk=32):
    """H.novelty in chunks of planes (the statement's gather is planes x cells x fan-in integers at once)."""
    planes = np.asarray(planes)
    return np.concatenate([H.novelty(wt, planes[i:i + chunk], conn, n_active) for i in range(0, len(planes), chunk)])


@functools.lru_cache(maxsize=None)
def ensemble_data(key, n, A):
    """dict(planes uint8[n,A,h,w], d int64[n,A], fam float64[n,A], best int[n] (the statement's), planted (member or None), conn, wt,
    views, h, w, n_active)."""
    d = H.case_data(key)
    h, w = d["h"], d["w"]
    args = (d["conn"], d["n_active"])
    base = SEED + d["seed"] * 100 + n * 7 + A
    planes = H.route_views(base, n * A, h, w).reshape(n, A, h, w).copy()
    planted = planted_member(n, A)
    for i in range(n):
        if i == planted:
            pool = H.route_views(base + 1, 4 * A + 16, h, w)
            novel = pool[novelty(d["wt"], pool, *args) > 0][:A]
            assert len(novel) == A, (key, n, A, len(novel))
            planes[i] = novel
            for a in planted_headings(A):
                planes[i, a] = d["views"][0]
        elif A > 1 or i % 2 == 0:
            planes[i, (3 * i + 1) % A] = d["views"][(5 * i + 1) % d["F"]]
    nov = novelty(d["wt"], planes.reshape(n * A, h, w), *args).reshape(n, A)
    fam = (-nov).astype(np.float64)
    best = np.argmax(fam, axis=1)
    # the three conditions (module docstring)
    if A > 1:
        assert (best != 0).any(), (key, n, A)
    if planted is not None:
        a0, a1 = planted_headings(A)
        assert np.flatnonzero(fam[planted] == fam[planted].max()).tolist() == [a0, a1] and a0 != 0 and best[planted] == a0, (key, n, A)
        assert H.bits(fam[planted, a0:a0 + 1])[0] == 0                                   # +0.0
    assert nov.max() > 0, (key, n, A)
    for a in (planes, nov, fam, best):
        a.setflags(write=False)
    return dict(planes=planes, d=nov, fam=fam, best=best, planted=planted, conn=d["conn"], wt=d["wt"], views=d["views"], h=h, w=w,
                n_active=d["n_active"])


@functools.lru_cache(maxsize=None)
def slab_data():
    """SLAB: dict(two uint8[2,3,5], pick int[3, 2731] (which of the two each column is), fam float64[3, 2731], best, conn, wt, ...):
    5x3_k37's model; plane 0 is a trained view (d = 0), plane 1 a novel one (d > 0).  Member 0 is novel but for its last heading,
    member 1 but for heading 1500, and member 2 but for its LAST heading: column 8192, the one column of the second launch (the first
    launch ends with column 8191, member 2's heading 2729, a novel one)."""
    d = H.case_data("5x3_k37")
    pool = H.route_views(SEED + 99, 64, d["h"], d["w"])
    nov = H.novelty(d["wt"], pool, d["conn"], d["n_active"])
    two = np.ascontiguousarray(np.stack([d["views"][0], pool[int(np.argmax(nov > 0))]]))
    n2 = H.novelty(d["wt"], two, d["conn"], d["n_active"])
    assert n2[0] == 0 and n2[1] > 0
    pick = np.ones((SLAB_MEMBERS, SLAB_HEADINGS), dtype=np.int64)
    pick[0, SLAB_HEADINGS - 1] = 0
    pick[1, 1500] = 0
    pick[2, SLAB_HEADINGS - 1] = 0
    fam = (-n2).astype(np.float64)[pick]
    best = np.argmax(fam, axis=1)
    assert best.tolist() == [SLAB_HEADINGS - 1, 1500, SLAB_HEADINGS - 1]
    views, _ = H.slab_views()
    assert SLAB_MEMBERS * SLAB_HEADINGS == views + 1
    return dict(two=two, pick=pick, fam=fam, best=best, conn=d["conn"], wt=d["wt"], h=d["h"], w=d["w"], n_active=d["n_active"])


@functools.lru_cache(maxsize=None)
def bytes_data():
    """BYTES: one member x 4097 planes of 128x128_k2049 built as SLAB_TRAIN's: view 0 everywhere but the LAST column, which is view 1
    -- trained on view 1 alone, so the winner is the one column behind the byte bound of the first launch."""
    t = H.slab_train_data()
    _, stage = H.slab_views()
    n = stage // t["N"] + 1
    wt = H.train(np.ones(t["K"], np.uint8), t["two"][1:], t["conn"], t["n_active"])
    n2 = H.novelty(wt, t["two"], t["conn"], t["n_active"])
    assert n2[0] > 0 and n2[1] == 0
    pick = np.zeros((1, n), dtype=np.int64)
    pick[0, -1] = 1
    fam = (-n2).astype(np.float64)[pick]
    return dict(two=t["two"], pick=pick, fam=fam, best=np.array([n - 1]), conn=t["conn"], wt=wt, h=t["h"], w=t["w"], n_active=t["n_active"])


def sensed_model(name):
    """(conn, n_active, wt): SENSED_MODELS[name] on the 32x32 sensor, trained by the statement on the host-sensed views of the route."""
    return _sensed_model(name)


@functools.lru_cache(maxsize=None)
def _sensed_model(name):
    m = SENSED_MODELS[name]
    n_active = max(1, int(round(m["sparsity"] * m["n_kc"])))
    conn = H.connectivity(m["n_kc"], 1024, m["fan_in"], m["seed"])
    wt = H.train(np.ones(m["n_kc"], np.uint8), HI.sensed_data()["views"], conn, n_active)
    assert 0 < (wt == 0).sum() <= m["n_kc"] // 2
    return conn, n_active, wt


def sensed_poses(A):
    """Five members beside the route of helpers_infomax.SENSED: (xs, ys, centre headings)."""
    path = HI.sensed_route()
    rng = np.random.default_rng(A)
    at = (3, 11, 20, 29, 38)
    xs = np.array([path[k][0] + rng.uniform(-1, 1) for k in at])
    ys = np.array([path[k][1] + rng.uniform(-1, 1) for k in at])
    return xs, ys, np.array([0.9, 0.2, 5.9, 1.4, 3.0])


def sensed_statement(name, xs, ys, angs):
    """float64[n, A]: the statement on the host sensor model's planes at the members' poses."""
    conn, n_active, wt = sensed_model(name)
    n, A = angs.shape
    planes = H.host_sensed_planes(np.repeat(xs, A), np.repeat(ys, A), angs.reshape(-1))
    return (-novelty(wt, planes, conn, n_active)).astype(np.float64).reshape(n, A)
