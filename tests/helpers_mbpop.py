"""Population tables of the mushroom-body model (include/dejavu.h: dv_mbpop_*): the NumPy statement of tests/helpers_mushroom.py run
bank by bank, each bank with its own population (cells, wiring, quota, channel), and the inputs of tests/test_mbpop_host.py and
tests/test_gpu_mbpop.py.  Nothing here has a tolerance: integers from pixel to score, np.array_equal everywhere.

TABLE is the one table of the 7 x 5 test: populations (K, c, n_active) that each reach another corner of the kernel body --
(1, 1, 1): one cell, three waves without cells; (63, 4, 7): under one wave's trip; (65, 16, 65): every cell fires, the widest
histogram; (257, 10, 3): a wave's span is 128, so waves 0..2 hold 128 + 128 + 1 cells and the fourth owns none; (1043, 2, 11):
several trips a wave.  Seven banks, two populations behind two banks each, and 40 views dealt unevenly (DEAL)."""
import functools

import numpy as np

from tests import helpers_mushroom as H

TABLE = dict(w=7, h=5, pops=((1, 1, 1), (63, 4, 7), (65, 16, 65), (257, 10, 3), (1043, 2, 11)), pop_of_bank=(0, 1, 2, 3, 4, 1, 3), seed=301,
             views=40, members_per_bank=2, headings=13)
DEAL = (0, 3, 1, 6, 4, 2, 5, 1, 1, 6, 3)                     # bank of view v is DEAL[v % 11]: banks 1, 3 and 6 get more than the others


def population(N, K, c, n_active, seed, channel=2):
    """The dict FamiliarityEngine.mbpop_set takes, with the statement's own connectivity."""
    return dict(channel=channel, n_kc=K, fan_in=c, n_active=n_active, conn=H.connectivity(K, N, c, seed).astype(np.int32))


def deal(n, pattern=DEAL):
    return np.array([pattern[v % len(pattern)] for v in range(n)], dtype=np.int32)


def train(pops, pop_of_bank, planes, bank_of, wts=None):
    """[uint8[K of bank b]]: every bank's weights after the views dealt to it, under its own population.  planes: uint8[n,h,w] of the
    compared plane already, or uint8[n,h,w,3] scenes, of which a bank reads its population's channel."""
    planes, bank_of = np.asarray(planes), np.asarray(bank_of)
    out = []
    for b, p in enumerate(pop_of_bank):
        pop = pops[p]
        mine = planes[bank_of == b]
        if planes.ndim == 4:
            mine = np.ascontiguousarray(mine[..., pop["channel"]])
        start = np.ones(pop["n_kc"], np.uint8) if wts is None else wts[b]
        out.append(H.train(start, mine, pop["conn"], pop["n_active"]) if len(mine) else np.array(start, dtype=np.uint8))
    return out


def scores(pops, pop_of_bank, wts, planes, banks):
    """float64[n, A]: member i's A planes (uint8[n,A,h,w], or [n,A,h,w,3] scenes) under bank banks[i] and that bank's population."""
    planes = np.asarray(planes)
    rows = []
    for i, b in enumerate(banks):
        pop = pops[pop_of_bank[b]]
        mine = planes[i] if planes.ndim == 4 else np.ascontiguousarray(planes[i][..., pop["channel"]])
        rows.append(H.familiarity(wts[b], mine, pop["conn"], pop["n_active"]))
    return np.stack(rows)


@functools.lru_cache(maxsize=None)
def table_data():
    """TABLE's inputs and the statement on them: dict(pops, pop_of_bank, views, bank_of, wts, planes, banks, fam, best, h, w)."""
    t = TABLE
    N = t["w"] * t["h"]
    pops = [population(N, K, c, a, t["seed"] + p) for p, (K, c, a) in enumerate(t["pops"])]
    views = H.route_views(t["seed"], t["views"], t["h"], t["w"])
    bank_of = deal(t["views"])
    wts = train(pops, t["pop_of_bank"], views, bank_of)
    B, m, A = len(t["pop_of_bank"]), t["members_per_bank"], t["headings"]
    banks = np.repeat(np.arange(B, dtype=np.int32), m)
    planes = H.route_views(t["seed"] + 50, B * m * A, t["h"], t["w"]).reshape(B * m, A, t["h"], t["w"]).copy()
    for i, b in enumerate(banks):                            # a view the member's bank was trained on, at a heading that is not the first
        planes[i, 3 + i % 7] = views[bank_of == b][i % 2]
    fam = scores(pops, t["pop_of_bank"], wts, planes, banks)
    # what the test must tell apart: every bank was trained, no bank of the larger populations is empty or full, banks of one population
    # differ, and a member scored under the other bank of its population (or under bank 4) gets another row
    assert sorted(set(bank_of.tolist())) == list(range(B)) and len(set(np.bincount(bank_of).tolist())) > 1
    for b in (1, 3, 4, 5, 6):
        assert 0 < int((wts[b] == 0).sum()) < len(wts[b]), b
    assert not np.array_equal(wts[1], wts[5]) and not np.array_equal(wts[3], wts[6])
    assert (wts[2] == 0).all() and wts[0].tolist() == [0]                      # every cell fires; the one cell
    other = scores(pops, t["pop_of_bank"], wts, planes, [{1: 5, 5: 1, 3: 6, 6: 3}.get(b, b) for b in banks])
    for i, b in enumerate(banks):
        if b in (1, 3, 5, 6):
            assert not np.array_equal(other[i], fam[i]), i
    assert (fam.max(axis=1) == 0).all() and fam.min() < 0
    return dict(pops=pops, pop_of_bank=t["pop_of_bank"], views=views, bank_of=bank_of, wts=wts, planes=planes, banks=banks, fam=fam,
                best=np.argmax(fam, axis=1), h=t["h"], w=t["w"])


# ---- constant planes: the quota among equals through the waves' spans -----------------------------------------------------------------
CONSTANT = dict(w=16, h=16, pops=((257, 10, 200), (1043, 2, 700)), seed=311)


def constant_data():
    """Two populations whose quotas run through several waves' spans (257 cells: spans of 128, quota 200 ends in wave 1; 1043 cells:
    spans of 320, quota 700 ends in wave 2), one bank each, on an all-0 and an all-255 plane: every activity is equal, so exactly the
    first n_active cells in index order fire."""
    t = CONSTANT
    pops = [population(t["w"] * t["h"], K, c, a, t["seed"] + p) for p, (K, c, a) in enumerate(t["pops"])]
    planes = H.constant_planes(t["h"], t["w"])[:2]
    want = []
    for pop in pops:
        first = np.ones(pop["n_kc"], np.uint8)
        first[:pop["n_active"]] = 0
        assert np.array_equal(H.train(np.ones(pop["n_kc"], np.uint8), planes, pop["conn"], pop["n_active"]), first)
        assert H.wave_span(pop["n_kc"]) < pop["n_active"]
        want.append(first)
    return dict(pops=pops, planes=planes, want=want, h=t["h"], w=t["w"])


# ---- launch edges ------------------------------------------------------------------------------------------------------------------------------
EDGE = dict(w=7, h=5, pops=((300, 4, 6), (129, 3, 5)), seed=321)


@functools.lru_cache(maxsize=None)
def edge_data():
    """One more view, and one more column, than a launch holds (helpers_mushroom.slab_views), the last alone in bank 1, whose population
    is another than bank 0's.  Two views `two`: all training views are two[0] in bank 0 but the last, two[1] in bank 1.  A table read at
    the launch's own column would send the last view to bank 0 -- bank 0 would hold two[1] as well and bank 1 nothing -- and would score
    the last column under bank 0.  dict(pops, two, pick, bank_of, wts, step_pick int[3, 2731], step_banks, fam, best)."""
    from tests import helpers_mushroom_ensemble as HE
    t = EDGE
    n = H.slab_views()[0] + 1
    pops = [population(t["w"] * t["h"], K, c, a, t["seed"] + p) for p, (K, c, a) in enumerate(t["pops"])]
    two = H.route_views(t["seed"], 2, t["h"], t["w"])
    pick = np.zeros(n, dtype=np.int64)
    pick[-1] = 1
    bank_of = np.zeros(n, dtype=np.int32)
    bank_of[-1] = 1
    wts = train(pops, (0, 1), two[pick], bank_of)
    wrong = train(pops, (0, 1), two[pick], np.zeros(n, dtype=np.int32))
    assert not np.array_equal(wrong[0], wts[0]) and not np.array_equal(wrong[1], wts[1])
    # the step: members 0 and 1 in bank 0 see two[0] (trained there: 0) but for one heading each; member 2, in bank 1, sees two[1]
    # everywhere, 0 under its own bank
    step_pick = np.zeros((HE.SLAB_MEMBERS, HE.SLAB_HEADINGS), dtype=np.int64)
    assert step_pick.size == n
    step_pick[0, 7], step_pick[1, 1500] = 1, 1
    step_pick[2, :] = 1
    step_banks = np.array([0, 0, 1], dtype=np.int32)
    fam = scores(pops, (0, 1), wts, two[step_pick], step_banks)
    under0 = scores(pops, (0, 1), wts, two[step_pick], [0, 0, 0])
    assert fam[2, -1] == 0.0 and under0[2, -1] < 0 and fam[0, 7] < 0 and fam[1, 1500] < 0
    return dict(pops=pops, two=two, pick=pick, bank_of=bank_of, wts=wts, step_pick=step_pick, step_banks=step_banks, fam=fam,
                best=np.argmax(fam, axis=1), h=t["h"], w=t["w"])


# ---- a fake engine: what the ensemble's plumbing asks of one ---------------------------------------------------------------------------------
class FakeEngine(object):
    """Stands where FamiliarityEngine does for MushroomRouteEnsemble.from_routes_with: notes every call by name (and what the tests
    look at of its arguments) and answers with arrays of the right shape."""
    def __init__(self, h, w):
        self.log, self.h, self.w = [], h, w
        self.mb_pops, self.mb_pop_of_bank, self.mb_banks = None, None, 1
        self.sensor_shape = (h, w)

    def mb_begin(self, h, w, conn, n_active, channel=2):
        self.log.append(("mb_begin", h, w, conn.shape, n_active, channel))
        self.mb_pops, self.mb_banks = None, 1

    def mbank_set(self, n_banks):
        self.log.append(("mbank_set", n_banks))
        self.mb_pops, self.mb_banks = None, n_banks

    def mbpop_set(self, populations, population_of_bank):
        self.log.append(("mbpop_set", [{k: v for k, v in p.items() if k != "conn"} for p in populations], list(population_of_bank)))
        self.mb_pops, self.mb_pop_of_bank, self.mb_banks = list(populations), np.asarray(population_of_bank, np.int32), len(population_of_bank)

    def mbank_train_from_poses(self, x, y, angle, bank_of_view, want_views=True, land_of_view=None):
        self.log.append(("mbank_train_from_poses", len(x), list(np.unique(bank_of_view))))
        return np.zeros((len(x), self.h, self.w, 3), dtype=np.uint8)

    def mb_score_u8(self, planes, out=None):                 # (bound by the model's func; a banked member never calls it)
        self.log.append(("mb_score_u8",))
        raise AssertionError("a bank-0 call under a route ensemble")

    def mbank_info(self):
        self.log.append(("mbank_info",))
        return dict(n_banks=self.mb_banks, views_trained=np.zeros(self.mb_banks, np.int64), n_depressed=np.zeros(self.mb_banks, np.int64))
