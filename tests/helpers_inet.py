"""Network tables of the Infomax model (include/dejavu.h: dv_inet_*): the NumPy statement of tests/helpers_infomax.py run bank by bank,
each bank with its own network (n_hidden, learning rate, W0, channel), and the inputs of tests/test_inet_host.py and
tests/test_gpu_inet.py.  Comparisons with the statement use helpers_infomax.TOL, relative to max|W| and max|d| as everywhere; comparisons
with lone engines are on the doubles' bits.

TABLE is the one table of the 7 x 5 tests (N = 35): networks (n_hidden, learning_rate) whose M each reach another corner of the ragged
grids -- 1: one wave of a 4-row block; 3: a ragged block; 63 and 65: one short of and one past the 64-row block of the u partial sums;
1043: 17 row blocks and 66 row tiles of 16, the decision's second trip.  Seven banks, networks 1 and 3 behind two banks each, 40 views
dealt unevenly (DEAL) with bank 5 left empty.  Every rate is checked here, on the CPU, to leave the statement finite on the views."""
import functools

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


def scores(nets, net_of_bank, Ws, planes, banks):
    """float64[n, A]: member i's A planes (uint8[n,A,h,w], or [n,A,h,w,3] scenes) under bank banks[i] and that bank's channel."""
    planes = np.asarray(planes)
    rows = []
    for i, b in enumerate(banks):
        net = nets[net_of_bank[b]]
        mine = planes[i] if planes.ndim == 4 else np.ascontiguousarray(planes[i][..., net["channel"]])
        rows.append(H.familiarity(Ws[b], mine))
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
