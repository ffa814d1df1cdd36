"""Network tables of the Infomax model (include/dejavu.h: dv_inet_*): the NumPy statement of tests/helpers_infomax.py run bank by bank,
each bank with its own network (n_hidden, learning rate, W0, channel), and the inputs of tests/test_inet_host.py and
tests/test_gpu_inet.py.  Comparisons with the statement use helpers_infomax.TOL, relative to max|W| and max|d| as everywhere; comparisons
with lone engines are on the doubles' bits.

TABLE is the one table of the 7 x 5 tests (N = 35): networks (n_hidden, learning_rate) whose M each reach another corner of the ragged
grids -- 1: one wave of a 4-row block; 3: a ragged block; 63 and 65: one short of and one past the 64-row block of the u partial sums;
1043: 17 row blocks and 66 row tiles of 16, the decision's second trip.  Seven banks, networks 1 and 3 behind two banks each, 40 views
dealt unevenly (DEAL) with bank 5 left empty.  Every rate is checked here, on the CPU, to leave the statement finite on the views.

Steps past one launch.  step_slabs() states the cut ibank_batch makes of a step's columns, on the three constants read from the kernel
file; SLAB crosses the byte bound (8192 columns of 32 x 32 views) in the middle of a member, BLOCKS the block-count bound (16384 blocks).
tests/test_inet_host.py asserts of both what their comments say, that a launch-local bank, column or landscape index would move launch
2's values by more than 1e-6 relative, and the rule helpers_infomax.TOL was made by on these (shape, M, views), which its table does not
hold: the statement in float64 against longdouble and against a permuted order of every sum, the larger, relative to max|W| and max|d|
(x86-64, OpenBLAS NumPy):

    layout (w x h; M of the banks; views trained a bank)                       weights     scores
    SLAB   32x32; 49, 17, 33, 5; 3, 5, 4, 3   688 x 12 uploaded patches        2.8e-16     5.4e-16
    SLAB   the same banks; 688 x 12 sensed headings, set / one landscape                   5.5e-16
    BLOCKS 7x5; 1, 3, 17 in turn over 16385 banks; 3 in three banks            1.8e-16     2.6e-16

1000 x the largest, 5.5e-13, is under TOL = 2e-12: no layout needs a bound of its own.  (helpers_infomax_banks.py: the same two layouts
under banks of one shape.)"""
import functools
import os
import re

import numpy as np

from tests import helpers_infomax as H

TABLE = dict(w=7, h=5, nets=((1, 0.01), (3, 0.02), (63, 0.005), (65, 0.01), (1043, 0.002)), net_of_bank=(0, 1, 2, 3, 4, 1, 3), seed=401, views=40)
DEAL = (0, 3, 1, 6, 4, 2, 1, 1, 6, 3, 4)                     # bank of view v is DEAL[v % 11]: banks 1, 3, 4 and 6 get more; bank 5 none

# the VEC loads (N % 4 == 0): 8 x 8 views with a whole row tile, one row past it and 65 row tiles in one table
VEC = dict(w=8, h=8, nets=((16, 0.01), (17, 0.02), (1040, 0.005)), net_of_bank=(0, 1, 2), seed=411, views=17, deal=(2, 0, 1, 1, 2))

# the step's layouts over TABLE: 14 members in scrambled bank order, 8 of them in bank 1 (72 and 560 columns: more than one block)
STEP_BANKS = (1, 4, 1, 0, 6, 1, 2, 1, 5, 1, 3, 1, 1, 1)
STEP_HEADINGS = (9, 70)


def network(N, M, eta, seed, channel=2):
    """The dict FamiliarityEngine.inet_set takes, with the statement's own initial weights."""
    return dict(channel=channel, n_hidden=M, learning_rate=eta, w0=H.initial_weights(M, N, seed))


def deal(n, pattern=DEAL):
    return np.array([pattern[v % len(pattern)] for v in range(n)], dtype=np.int32)


def train(nets, net_of_bank, planes, bank_of, Ws=None):
    """[float64[M of bank b, N]]: every bank's weights after the views dealt to it, in their order, under its own network.  planes:
    uint8[n,h,w] of the compared plane already, or uint8[n,h,w,3] scenes, of which a bank reads its network's channel."""
    planes, bank_of = np.asarray(planes), np.asarray(bank_of)
    out = []
    for b, p in enumerate(net_of_bank):
        net = nets[p]
        mine = planes[bank_of == b]
        if planes.ndim == 4:
            mine = np.ascontiguousarray(mine[..., net["channel"]])
        start = net["w0"] if Ws is None else Ws[b]
        W = H.train(start, mine, eta=net["learning_rate"]) if len(mine) else np.array(start, dtype=np.float64)
        assert np.isfinite(W).all(), (b, net["learning_rate"])          # the rate is stable on these views
        out.append(W)
    return out


def scores(nets, net_of_bank, Ws, planes, banks, **kw):
    """float64[n, A]: member i's A planes (uint8[n,A,h,w], or [n,A,h,w,3] scenes) under bank banks[i] and that bank's channel.  kw: the
    dtype or order_seed of H.familiarity (the tolerance rule's other runs)."""
    planes = np.asarray(planes)
    rows = []
    for i, b in enumerate(banks):
        net = nets[net_of_bank[b]]
        mine = planes[i] if planes.ndim == 4 else np.ascontiguousarray(planes[i][..., net["channel"]])
        rows.append(H.familiarity(Ws[b], mine, **kw))
    return np.stack(rows)


def rel(got, want):
    """max|got - want| / max|want|."""
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want))) / np.max(np.abs(want)))


def _table(t, pattern):
    N = t["w"] * t["h"]
    nets = [network(N, M, eta, t["seed"] + p) for p, (M, eta) in enumerate(t["nets"])]
    views = H.route_views(t["seed"], t["views"], t["h"], t["w"])
    bank_of = deal(t["views"], pattern)
    Ws = train(nets, t["net_of_bank"], views, bank_of)
    for a in [views, bank_of] + Ws + [n["w0"] for n in nets]:
        a.setflags(write=False)
    return dict(nets=nets, net_of_bank=t["net_of_bank"], views=views, bank_of=bank_of, Ws=Ws, h=t["h"], w=t["w"], N=N)


@functools.lru_cache(maxsize=None)
def table_data():
    """TABLE's inputs and the statement on them: dict(nets, net_of_bank, views, bank_of, Ws, h, w, N)."""
    d = _table(TABLE, DEAL)
    counts = np.bincount(d["bank_of"], minlength=7).tolist()
    assert counts[5] == 0 and min(c for b, c in enumerate(counts) if b != 5) >= 3 and len(set(counts)) > 2, counts
    # what the test must tell apart: banks of one network differ, and the empty bank holds its network's W0
    assert rel(d["Ws"][1], d["Ws"][5]) > 1e-3 and rel(d["Ws"][3], d["Ws"][6]) > 1e-3 and np.array_equal(d["Ws"][5], d["nets"][1]["w0"])
    return d


@functools.lru_cache(maxsize=None)
def vec_data():
    d = _table(VEC, VEC["deal"])
    assert d["N"] % 4 == 0 and sorted(set(d["bank_of"].tolist())) == [0, 1, 2]
    return d


@functools.lru_cache(maxsize=None)
def step_data(A):
    """A step over TABLE's trained banks: 14 members of A headings in STEP_BANKS' order.  A member's patches are windows of a strip of its
    own, every third a trained view; member i's best patch (by the statement) is planted a second time at a LATER heading, so its row
    has two equal maxima and the first must win.  dict(planes uint8[14,A,h,w], banks, fam, first int[14], second int[14])."""
    d = table_data()
    banks = np.array(STEP_BANKS, dtype=np.int32)
    n = len(banks)
    planes = H.route_views(TABLE["seed"] + 70 + A, n * A, d["h"], d["w"]).reshape(n, A, d["h"], d["w"]).copy()
    for i in range(n):
        planes[i, ::3] = d["views"][(np.arange(len(planes[i, ::3])) + i) % len(d["views"])]
    fam = scores(d["nets"], d["net_of_bank"], d["Ws"], planes, banks)
    first, second = [], []
    for i in range(n):
        order = np.argsort(-fam[i], kind="stable")
        a = int(min(order[0], A - 2))                        # (the best heading, or the last but one where the best is the last)
        planes[i, a] = planes[i, order[0]]
        b = a + 1 + (i % (A - 1 - a))
        planes[i, b] = planes[i, a]
        first.append(a)
        second.append(b)
    fam = scores(d["nets"], d["net_of_bank"], d["Ws"], planes, banks)
    assert all(np.argmax(fam[i]) == first[i] and fam[i, first[i]] == fam[i, second[i]] for i in range(n))
    top = -np.sort(-fam, axis=1)
    assert ((top[:, 0] - top[:, 2]) / np.abs(top[:, 0])).min() > 1e-3                    # the pair leads the rest far above H.TOL
    # under another bank a member gets another row (bank 1 against its network's other bank, 5, too)
    other = scores(d["nets"], d["net_of_bank"], d["Ws"], planes, [{1: 5, 5: 1, 3: 6, 6: 3}.get(b, (b + 1) % 5) for b in banks])
    assert all(rel(other[i], fam[i]) > 1e-6 for i in range(n) if d["nets"][d["net_of_bank"][banks[i]]]["n_hidden"] > 1)
    for a in (planes, fam):
        a.setflags(write=False)
    return dict(planes=planes, banks=banks, fam=fam, first=np.array(first), second=np.array(second))


# ---- the slab edge: one more view than the x vectors of 32 x 32 views are staged at a time -------------------------------------------------
EDGE = dict(w=32, h=32, nets=((4, H.ETA), (5, H.ETA)), seed=421, cut=100)


@functools.lru_cache(maxsize=None)
def edge_data():
    """8193 views of 32 x 32 (helpers_infomax.LONG_CHAIN's: 8192 x vectors a slab), all in bank 0 (M = 4) but the last, alone in bank 1
    (M = 5): dict(nets, views, bank_of, W1: the statement on bank 1's one view).  A table read at the slab's own view index would train
    the last view into bank 0.  Bank 0's chain is held to lone engines' bits alone: along 8192 views the statement's own rounding is
    above TOL (helpers_infomax: LONG_CHAIN)."""
    t = EDGE
    n = 8192 + 1
    nets = [network(t["w"] * t["h"], M, eta, t["seed"] + p) for p, (M, eta) in enumerate(t["nets"])]
    views = H.long_chain_data()["views"][:n]
    bank_of = np.zeros(n, dtype=np.int32)
    bank_of[-1] = 1
    W1 = H.train(nets[1]["w0"], views[-1:], eta=nets[1]["learning_rate"])
    assert rel(W1, nets[1]["w0"]) > 1e-6
    return dict(nets=nets, views=views, bank_of=bank_of, W1=W1, h=t["h"], w=t["w"])


# ---- divergence: three banks on the 16 x 16 case's views, the middle one at helpers_infomax.diverging_eta() ---------------------------------
def diverge_data():
    c = H.case_data("16x16_a16")
    N = c["N"]
    nets = [network(N, 20, H.ETA, 431), network(N, 24, H.diverging_eta(), 432), network(N, 33, 0.005, 433)]
    views = np.ascontiguousarray(np.concatenate([c["views"]] * 3))
    bank_of = np.repeat(np.arange(3, dtype=np.int32), len(c["views"]))
    with np.errstate(all="ignore"):
        assert not np.isfinite(H.train(nets[1]["w0"], c["views"], eta=nets[1]["learning_rate"])).all()      # it does diverge, on the CPU
    Ws = train([nets[0], nets[2]], (0, 1), np.ascontiguousarray(np.concatenate([c["views"]] * 2)), bank_of[:2 * len(c["views"])])
    return dict(nets=nets, views=views, bank_of=bank_of, W0=Ws[0], W2=Ws[1], patches=c["patches"], h=c["h"], w=c["w"], F=len(c["views"]))


# ---- a step's launches: the cut ibank_batch (dejavu_infomax.inl) makes, stated again -------------------------------------------------------
def slab_constants():
    """(kImStageBytes, kImSlabColsMax, kImHeadings), read from the kernel file: a layout below that no longer reaches an edge after one of
    them changed fails its assertion on the CPU instead of passing on one launch."""
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(os.path.dirname(here), "navigation-by-deja-vu_amd", "csrc", "dejavu_infomax.inl")).read()
    stage = re.search(r"kImStageBytes\s*=\s*(\d+)u?\s*<<\s*(\d+)\s*;", src)
    cols = re.search(r"kImSlabColsMax\s*=\s*(\d+)\s*<<\s*(\d+)\s*;", src)
    heads = re.search(r"kImHeadings\s*=\s*(\d+)\s*;", src)
    return int(stage.group(1)) << int(stage.group(2)), int(cols.group(1)) << int(cols.group(2)), int(heads.group(1))


def step_slabs(members_per_bank, A, N):
    """The launches of a banked step as [(c0, nc, blocks)], blocks = [(bank, x0, nc, d0)]: the members sorted stably by bank, so bank b's
    run of members_per_bank[b] * A columns follows its predecessors'; a run cut into blocks of kImHeadings columns (the last ragged); d0
    counted in runs padded to whole blocks (cpad); a launch takes consecutive blocks while its columns stay within the slab --
    kImStageBytes / (8 N) rounded down to whole blocks, at least one block, at most kImSlabColsMax and cpad -- and its blocks stay under
    kImSlabColsMax / kImHeadings.  c0 is the first block's x0: where the launch's first column lies among the sorted columns."""
    stage, cols_max, heads = slab_constants()
    blocks, cpad, first = [], 0, 0
    for b, n in enumerate(members_per_bank):
        cols, x0 = int(n) * A, first * A
        for o in range(0, cols, heads):
            blocks.append((b, x0 + o, min(heads, cols - o), cpad + o))
        cpad += (cols + heads - 1) // heads * heads
        first += int(n)
    slab = min(max(stage // (8 * N) // heads * heads, heads), cols_max, cpad)
    out, k0 = [], 0
    while k0 < len(blocks):
        nc = nk = 0
        while k0 + nk < len(blocks) and nk < cols_max // heads and nc + blocks[k0 + nk][2] <= slab:
            nc += blocks[k0 + nk][2]
            nk += 1
        assert nk > 0, (k0, slab)
        out.append((blocks[k0][1], nc, blocks[k0:k0 + nk]))
        k0 += nk
    return out


def slab_columns(N):
    stage, cols_max, heads = slab_constants()
    return min(max(stage // (8 * N) // heads * heads, heads), cols_max)


def sorted_members(banks):
    """(order, place): order[p] the caller's member at place p of the bank order, place[i] the place of member i."""
    order = np.argsort(np.asarray(banks), kind="stable")
    place = np.empty(len(order), dtype=np.int64)
    place[order] = np.arange(len(order))
    return order, place


# ---- the byte bound: 688 members x 12 headings of 32 x 32 views over four banks --------------------------------------------------------------
# SLAB: 340, 345, 2 and 1 members in banks 0 .. 3 (runs of 4080, 4140, 24 and 12 columns), in a caller's order scrambled by SLAB's seed.
# The slab holds 64 MiB / (8 * 1024) = 8192 columns: launch 1 takes bank 0's 64 blocks (63 whole, one of 48) and 64 whole blocks of
# bank 1, 8176 columns; launch 2 begins at c0 = 8176 = 681 * 12 + 4, inside the member at place 681, with bank 1's last 44 columns,
# bank 2's 24 and bank 3's 12: one block of each im_score_tile<4 | 2 | 1> class.  nets: (n_hidden, learning_rate, channel) of bank b's
# network; bank 0 has the largest M, so the row tiles that leave early (banks 1 .. 3: 2, 3 and 1 tiles of 4) are launch 2's; 17, 33 and
# 5 are no multiples of 16.  trained: the views each bank is trained on, so that no bank is its W0.
SLAB = dict(w=32, h=32, A=12, members=(340, 345, 2, 1), nets=((49, 0.01, 2), (17, 0.005, 0), (33, 0.002, 1), (5, 0.01, 0)),
            trained=(3, 5, 4, 3), seed=451)
SLAB_NAME = "SLAB (340, 345, 2, 1 members x 12 headings of 32 x 32 views)"


@functools.lru_cache(maxsize=None)
def slab_layout():
    """dict(banks int32[688] in the caller's order, order, place, launches, c0, nc1, nc2, slab, straddler (the caller's member whose
    columns the cut divides), cut (its headings in launch 1), A, N).  Asserted: everything SLAB's comment says of the cut."""
    t = SLAB
    A, N, n = t["A"], t["w"] * t["h"], sum(t["members"])
    banks = np.random.default_rng(t["seed"]).permutation(np.repeat(np.arange(len(t["members"]), dtype=np.int32), t["members"])).astype(np.int32)
    order, place = sorted_members(banks)
    assert (order != np.arange(n)).sum() > n // 2, SLAB_NAME + ": the caller's order is the bank order"
    launches = step_slabs(t["members"], A, N)
    slab = slab_columns(N)
    said = "%s: the slab holds %d columns and step_slabs gives %r" % (SLAB_NAME, slab, [(c0, nc, len(b)) for c0, nc, b in launches])
    assert len(launches) == 2, said + ", not two launches"
    (c1, nc1, blocks1), (c0, nc2, blocks2) = launches
    assert c1 == 0 and c0 == nc1 and nc1 + nc2 == n * A, said
    assert c0 % 64 != 0 and c0 % A != 0, said + ": the first launch ends at a whole block or a whole member"
    assert [b[0] for b in blocks2] == [1, 2, 3] and blocks1[-1][0] == 1, said + ": launch 2 is not the end of bank 1, bank 2, bank 3"
    widths = [b[2] for b in blocks2]
    assert 32 < widths[0] < 64 and 16 < widths[1] <= 32 and widths[2] <= 16, said + ": launch 2 lacks a block of each tile class: %r" % (widths,)
    assert [b[1] - c0 for b in blocks2] == [0, widths[0], widths[0] + widths[1]] and widths[0] % 16 != 0, said
    assert any(b[2] < 64 for b in blocks1), said + ": launch 1 has no ragged block"
    straddler, cut = int(order[c0 // A]), c0 % A
    assert banks[straddler] == 1 and 2 <= cut <= A - 2, said
    M = [m for m, _, _ in t["nets"]]
    tiles = [(m + 15) // 16 for m in M]
    assert tiles[0] == max(tiles) and all(tiles[b] < tiles[0] for b in (1, 2, 3)) and any(M[b] % 16 for b in (1, 2, 3)), (SLAB_NAME, M)
    for a in (banks, order, place):
        a.setflags(write=False)
    return dict(banks=banks, order=order, place=place, launches=launches, c0=c0, nc1=nc1, nc2=nc2, slab=slab, straddler=straddler, cut=cut,
                A=A, N=N)


@functools.lru_cache(maxsize=None)
def slab_pool():
    """uint8[8256, 32, 32]: a distinct view for every column -- helpers_infomax.long_chain_data's 8197 and 59 windows of another strip."""
    t, n = SLAB, sum(SLAB["members"]) * SLAB["A"]
    have = H.long_chain_data()["views"]
    pool = np.ascontiguousarray(np.concatenate([have, H.route_views(t["seed"] + 20, n - len(have), t["h"], t["w"])]))
    assert len(pool) == n and len(np.unique(pool.reshape(n, -1), axis=0)) == n, SLAB_NAME + ": two columns share a view"
    pool.setflags(write=False)
    return pool


def slab_members(score):
    """The members' planes over slab_pool() in the caller's order, with every member's best patch (by score(planes) -> float64[n, A],
    the statement) planted a second time at a LATER heading -- the straddling member's two on the two sides of the cut -- so that a row
    has two equal maxima and the first must win.  -> (planes uint8[n,A,h,w], fam, first int[n], second int[n])."""
    t, lay = SLAB, slab_layout()
    A, cut, n = lay["A"], lay["cut"], len(lay["banks"])
    planes = slab_pool().reshape(n, A, t["h"], t["w"]).copy()
    fam = score(planes)
    first, second = [], []
    for i in range(n):
        best = int(np.argmax(fam[i]))
        if i == lay["straddler"]:
            a, b = (best, cut + 1 + i % (A - cut - 1)) if best < cut else (cut - 2, best)
        else:
            a = min(best, A - 2)
            b = a + 1 + (i % (A - 1 - a))
        planes[i, a] = planes[i, best]
        planes[i, b] = planes[i, a]
        first.append(a)
        second.append(b)
    fam = score(planes)
    first, second = np.array(first), np.array(second)
    rows = np.arange(n)
    assert (np.argmax(fam, axis=1) == first).all() and (fam[rows, first] == fam[rows, second]).all() and (first < second).all(), SLAB_NAME
    assert first[lay["straddler"]] < cut <= second[lay["straddler"]], SLAB_NAME + ": the straddling member's maxima lie on one side of the cut"
    top = -np.sort(-fam, axis=1)
    margin = float(((top[:, 0] - top[:, 2]) / np.abs(top[:, 0])).min())
    assert margin > 1000 * H.TOL, (SLAB_NAME, margin)                                      # the pair leads the rest far above H.TOL
    for a in (planes, fam, first, second):
        a.setflags(write=False)
    return planes, fam, first, second, margin


def slab_deal():
    """int32[15]: the bank of every trained view, the banks' views interleaved (round robin while they last)."""
    t = SLAB["trained"]
    return np.array([b for s in range(max(t)) for b in range(len(t)) if s < t[b]], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def slab_step_data():
    """The uploaded step under a table: dict(nets, net_of_bank, views, bank_of, Ws, h, w, N, planes, banks, fam, first, second, margin)."""
    t = SLAB
    N = t["w"] * t["h"]
    nets = [network(N, M, eta, t["seed"] + 1 + p, channel=ch) for p, (M, eta, ch) in enumerate(t["nets"])]
    of_bank = (0, 1, 2, 3)
    views = H.route_views(t["seed"] + 10, sum(t["trained"]), t["h"], t["w"])
    bank_of = slab_deal()
    Ws = train(nets, of_bank, views, bank_of)
    assert all(rel(Ws[b], nets[b]["w0"]) > 1e-6 for b in of_bank)                          # no bank is its W0
    banks = slab_layout()["banks"]
    planes, fam, first, second, margin = slab_members(lambda p: scores(nets, of_bank, Ws, p, banks))
    for a in [views, bank_of] + Ws:
        a.setflags(write=False)
    return dict(nets=nets, net_of_bank=of_bank, views=views, bank_of=bank_of, Ws=Ws, h=t["h"], w=t["w"], N=N, planes=planes, banks=banks,
                fam=fam, first=first, second=second, margin=margin)


def wrong_index_margins(lay, cols, score):
    """What a wrong index in launch 2 would give, on the CPU.  cols: the compared planes uint8[C,h,w] in the SORTED order (what X holds);
    score(bank, planes) -> the statement under that bank.  For every column c of launch 2 the relative distance of its right value to
      bank: its value under the bank of the launch-LOCAL place, sorted member (c - c0) / A instead of c / A;
      x:    the value of the column a kernel that forgot c0 reads, X[c % slab] instead of X[c - c0] -- X holds launch 2's columns, behind
            them what launch 1 left, and behind those nothing of this call (NaN here: such a column cannot be told).
    -> (bank float64[nc2], x float64[nc2])."""
    A, c0, nc1, nc2, slab = lay["A"], lay["c0"], lay["nc1"], lay["nc2"], lay["slab"]
    sorted_banks = lay["banks"][lay["order"]]
    bank, x = np.empty(nc2), np.full(nc2, np.nan)
    for k in range(nc2):
        c = c0 + k
        own, local = int(sorted_banks[c // A]), int(sorted_banks[k // A])
        right = score(own, cols[c:c + 1])[0]
        bank[k] = abs(score(local, cols[c:c + 1])[0] - right) / abs(right)
        q = c % slab
        held = c0 + q if q < nc2 else q if q < nc1 else None
        if held is not None:
            x[k] = abs(score(own, cols[held:held + 1])[0] - right) / abs(right)
    return bank, x


def score_discrepancy(score, fam):
    """The tolerance rule on a step's scores: score(**kw) -> the statement's array in longdouble and in a permuted order of every sum,
    against its float64 run `fam`; the larger, relative to max|fam| (as the GPU test compares)."""
    return max(float(np.max(np.abs(score(**kw) - fam)) / np.max(np.abs(fam))) for kw in (dict(dtype=np.longdouble), dict(order_seed=99)))


def weight_discrepancy(nets, net_of_bank, views, bank_of, Ws):
    """The tolerance rule on every bank's chain (H.chain_discrepancy): the largest."""
    return max(H.chain_discrepancy(nets[p]["w0"], views[np.asarray(bank_of) == b], Ws[b], nets[p]["learning_rate"])
               for b, p in enumerate(net_of_bank) if (np.asarray(bank_of) == b).any())


# ---- the byte bound, sensed: the same members at a few places of helpers_lands' landscapes, its 32 x 32 sensor --------------------------------
SLAB_LANDS = (0, 1, 2, 3, 1)                                  # member i stands on landscape SLAB_LANDS[i % 5] of the set


@functools.lru_cache(maxsize=None)
def slab_sense_data():
    """The sensed step: the members of slab_layout() at 8 places and 8 x 12 headings (as helpers_lands.step_case, so the host model senses
    every distinct (place, heading, landscape) once) -> dict(xs, ys, angs [n, A], banks, lands, scenes_set uint8[n,A,h,w,3] (every member
    on its own landscape of the set), scenes_one (every member on landscape 0: the engine's one landscape), fam_set, fam_one,
    flagged (a member of launch 2 that is not the straddling one), + slab_step_data()'s networks and weights).  Member i stands on
    landscape SLAB_LANDS[i % 5], but launch 2's members each on another one than the member at their launch-local place."""
    from tests import helpers_lands as HL
    d, lay = slab_step_data(), slab_layout()
    n, A = len(lay["banks"]), lay["A"]
    rng = np.random.default_rng(SLAB["seed"] + 30)
    place_x, place_y, heads = rng.uniform(50, 120, 8), rng.uniform(50, 120, 8), rng.uniform(0, 2 * np.pi, (8, A))
    at = np.arange(n) % 8
    xs, ys, angs = place_x[at], place_y[at], heads[at]
    lands = np.array([SLAB_LANDS[i % 5] for i in range(n)], dtype=np.int32)
    behind = lay["order"][lay["c0"] // A:]                    # launch 2's members: each on another landscape than the member at its
    for k, i in enumerate(behind):                            # launch-local place, so a landscape table read there shows
        lands[i] = (lands[lay["order"][k]] + 1 + k % 3) % 4
    cache = {}

    def scene(i, a, l):
        k = (int(at[i]), a, int(l))
        if k not in cache:
            cache[k] = HL.host_scene("sq", xs[i], ys[i], angs[i, a], l)
        return cache[k]

    scenes_set = np.stack([np.stack([scene(i, a, lands[i]) for a in range(A)]) for i in range(n)])
    scenes_one = np.stack([np.stack([scene(i, a, 0) for a in range(A)]) for i in range(n)])
    fam_set = scores(d["nets"], d["net_of_bank"], d["Ws"], scenes_set, lay["banks"])
    fam_one = scores(d["nets"], d["net_of_bank"], d["Ws"], scenes_one, lay["banks"])
    flagged = int(lay["order"][-2])                           # the last member but one of the bank order
    for a in (xs, ys, angs, lands, scenes_set, scenes_one, fam_set, fam_one):
        a.setflags(write=False)
    return dict(d, xs=xs, ys=ys, angs=angs, lands=lands, scenes_set=scenes_set, scenes_one=scenes_one, fam_set=fam_set, fam_one=fam_one,
                flagged=flagged)


OFF_THE_SET = (200.0, 80.0, 1)                                # helpers_lands.ON_L2_OFF_L1's place, put on L1: past its 173 columns
OFF_THE_ONE = (295.0, 295.0)                                  # past the high edges of the 300 x 300 landscape 0 at any heading


# ---- the block-count bound: 16385 banks of one member of 3 headings, 7 x 5 views -------------------------------------------------------------
# 16385 blocks of 3 columns: the scoring grid's y extent takes 16384 of them, launch 2 the last one at c0 = 49152; the staging slab
# (239616 columns at N = 35) is far from full.  Networks of M = 1, 3 and 17 in turn; bank 16383 (launch 1's last block) has M = 17 and
# bank 16384 (launch 2's lone block) M = 3, so its second row tile leaves early.  Banks 0, 16383 and 16384 are trained on three views each.
BLOCKS = dict(w=7, h=5, A=3, banks=16385, nets=((1, 0.01), (3, 0.02), (17, 0.005)), trained=(0, 16383, 16384), views=3, seed=461)
BLOCKS_NAME = "BLOCKS (16385 banks of one member x 3 headings of 7 x 5 views)"


@functools.lru_cache(maxsize=None)
def blocks_layout():
    """dict(banks int32[16385]: the bank of member i, a permutation; order, place, launches, c0, last (the caller's member of launch 2),
    planes uint8[16385,3,5,7], views uint8[9,5,7], bank_of int32[9]).  Asserted: the 16384 + 1 split and what BLOCKS' comment says."""
    t = BLOCKS
    B, A, N = t["banks"], t["A"], t["w"] * t["h"]
    launches = step_slabs([1] * B, A, N)
    said = "%s: the grid takes %d blocks, the slab %d columns, and step_slabs gives %r" % (
        BLOCKS_NAME, slab_constants()[1] // slab_constants()[2], slab_columns(N), [(c0, nc, len(b)) for c0, nc, b in launches])
    assert [len(b) for _, _, b in launches] == [B - 1, 1], said + ", not launches of 16384 blocks and 1"
    assert launches[1][0] == (B - 1) * A and launches[1][2][0][:3] == (B - 1, (B - 1) * A, A) and A > 1, said
    assert slab_columns(N) > B * A, said + ": the byte bound cuts this call too"
    banks = np.random.default_rng(t["seed"]).permutation(B).astype(np.int32)
    order, place = sorted_members(banks)
    assert (order != np.arange(B)).mean() > 0.99, BLOCKS_NAME + ": the caller's order is the bank order"
    last = int(order[-1])
    assert banks[last] == B - 1 and last != B - 1, BLOCKS_NAME + ": launch 2's member is the caller's last"
    planes = H.route_views(t["seed"] + 5, B * A, t["h"], t["w"]).reshape(B, A, t["h"], t["w"])
    views = H.route_views(t["seed"] + 6, t["views"] * len(t["trained"]), t["h"], t["w"])
    bank_of = np.array(t["trained"] * t["views"], dtype=np.int32)                          # interleaved
    for a in (banks, order, place, planes, views, bank_of):
        a.setflags(write=False)
    return dict(banks=banks, order=order, place=place, launches=launches, c0=launches[1][0], last=last, planes=planes, views=views,
                bank_of=bank_of, A=A, N=N)


def blocks_scores(lay, kind_of_bank, W_of_kind, W_of_trained, **kw):
    """float64[16385, 3]: H.familiarity once per kind of bank (banks that share weights) over the planes of that kind's members, the
    trained banks' members then under their own weights."""
    fam = np.empty(lay["planes"].shape[:2], dtype=kw.get("dtype", np.float64))
    kind_of_member = np.asarray(kind_of_bank)[lay["banks"]]
    for k, W in enumerate(W_of_kind):
        m = np.flatnonzero(kind_of_member == k)
        fam[m] = H.familiarity(W, lay["planes"][m].reshape((-1,) + lay["planes"].shape[2:]), **kw).reshape(len(m), -1)
    for b, W in W_of_trained.items():
        i = int(lay["order"][b])                             # (one member a bank: the member at place b)
        fam[i] = H.familiarity(W, lay["planes"][i], **kw)
    return fam


@functools.lru_cache(maxsize=None)
def blocks_data():
    """The table over blocks_layout(): dict(nets, net_of_bank int32[16385], trained {bank: W}, fam, + the layout)."""
    t, lay = BLOCKS, blocks_layout()
    B = t["banks"]
    nets = [network(lay["N"], M, eta, t["seed"] + 1 + p) for p, (M, eta) in enumerate(t["nets"])]
    of_bank = (np.arange(B) % 3).astype(np.int32)
    of_bank[B - 2] = 2                                        # launch 1's last block: the largest M
    M = [net["n_hidden"] for net in nets]
    assert M[of_bank[B - 1]] < max(M) and (M[of_bank[B - 1]] + 15) // 16 < (max(M) + 15) // 16, BLOCKS_NAME + ": launch 2's bank has every row tile"
    assert M[of_bank[B - 2]] == max(M) and of_bank[0] != of_bank[B - 1], BLOCKS_NAME
    trained = {}
    for b in t["trained"]:
        net = nets[of_bank[b]]
        trained[b] = H.train(net["w0"], lay["views"][lay["bank_of"] == b], eta=net["learning_rate"])
        assert np.isfinite(trained[b]).all() and rel(trained[b], net["w0"]) > 1e-6
    fam = blocks_scores(lay, of_bank, [net["w0"] for net in nets], trained)
    of_bank.setflags(write=False)
    fam.setflags(write=False)
    return dict(lay, nets=nets, net_of_bank=of_bank, trained=trained, fam=fam, h=t["h"], w=t["w"])


# ---- a fake engine: what the ensemble's plumbing asks of one ---------------------------------------------------------------------------------
class FakeEngine(object):
    """Stands where FamiliarityEngine does for InfomaxRouteEnsemble.from_routes_with: notes every call by name (and what the tests look
    at of its arguments) and answers with arrays of the right shape."""
    def __init__(self, h, w):
        self.log, self.h, self.w = [], h, w
        self.infomax_nets, self.infomax_net_of_bank, self.infomax_banks, self.infomax_hidden = None, None, 1, 0
        self.sensor_shape = (h, w)
        self._w0 = None

    def infomax_begin(self, h, w, weights, channel=2, learning_rate=0.01):
        self.log.append(("infomax_begin", h, w, weights.shape, channel, learning_rate))
        self.infomax_nets, self.infomax_banks, self.infomax_hidden, self._w0 = None, 1, weights.shape[0], weights

    def infomax_read_weights(self):
        self.log.append(("infomax_read_weights",))
        return self._w0

    def ibank_set(self, n_banks, weights):
        self.log.append(("ibank_set", n_banks, weights.shape))
        self.infomax_nets, self.infomax_banks = None, n_banks

    def inet_set(self, networks, network_of_bank):
        self.log.append(("inet_set", [{k: v for k, v in p.items() if k != "w0"} for p in networks], list(network_of_bank)))
        self.infomax_nets, self.infomax_net_of_bank, self.infomax_banks = list(networks), np.asarray(network_of_bank, np.int32), len(network_of_bank)

    def ibank_train_from_poses(self, x, y, angle, bank_of_view, want_views=True, land_of_view=None):
        self.log.append(("ibank_train_from_poses", len(x), list(np.unique(bank_of_view))))
        return np.zeros((len(x), self.h, self.w, 3), dtype=np.uint8)

    def infomax_score_u8(self, planes, out=None):            # (bound by the model's func; a banked member never calls it)
        self.log.append(("infomax_score_u8",))
        raise AssertionError("a bank-0 call under a route ensemble")

    def ibank_info(self):
        self.log.append(("ibank_info",))
        return dict(n_banks=self.infomax_banks, views_trained=np.zeros(self.infomax_banks, np.int64), finite=np.ones(self.infomax_banks, bool))
