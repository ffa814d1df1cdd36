"""NumPy restatement of the Infomax familiarity model (include/dejavu.h: dv_infomax_*), the inputs of its tests and the tolerance
the device is held to.

The model, literally.  N = h*w pixels; x = p/255 - mean(p/255) of a view's uint8[h,w] plane flattened in C order, the mean being the
sum of the N values divided by N; W is [M, N], drawn as standard_normal from np.random.default_rng(seed), every row then minus its
mean and divided by its standard deviation (ddof=0).  One training view:

    h = W x;  y = tanh(h);  u = h^T W;  W <- W + (eta / N) * (W - (y + h) u^T)

and a scored view: d = sum_i |(W x)_i|, familiarity = -d.

Tolerance.  The device differs from this file in the order of its sums and in tanh by a few ulp, so the contract is a relative bound,
and it comes from this restatement alone: at every shape of the GPU tests (CASES) the restatement is run in float64, in
np.longdouble, and in float64 with every sum taken over a permuted order (`order_seed`), and the float64 run is compared with the
other two -- weights relative to max|W|, scores relative to max|d|.  Measured (x86-64, OpenBLAS NumPy):

    case (w x h, M, F)      float64 vs longdouble (W, d)     float64 vs permuted float64 (W, d)
    5x3,   15,   1          7.9e-17  5.4e-17                 8.9e-17  0
    5x3,   15,   2          1.3e-16  8.9e-17                 4.5e-17  0
    40x1,  24,  37          4.9e-16  9.3e-17                 1.5e-16  1.4e-16
    16x16, 256, 130         1.4e-15  1.5e-16                 8.1e-16  2.2e-16
    20x13, 70,  33          5.2e-16  2.5e-16                 2.1e-16  3.0e-16

The largest is 1.37e-15; the bound is that times 1000 (the margin for the device's tanh and tree reductions; the rule is contractive
at the tested learning rate, so errors do not grow along the chain), rounded up to one digit: TOL = 2e-12, beside the project's 1e-12
score contract.  tests/test_infomax_host.py measures the table again and holds TOL to it; nothing here comes from the code under
test.  On the same data: max|W| after training 2.5 .. 4.3; the 16x16 case scores its trained views near -645 and novel ones near
-920; the best heading of every case leads the second by at least 3e-3 relative, far above TOL; at learning rates of 0.1 and more
the float64 restatement overflows on the 16x16 case's views within its 130 views (0.01 stays finite), which is where the
divergence test takes its rate from.
"""
import functools

import numpy as np

TOL = 2e-12
ETA = 0.01
LEVELS = np.array([0, 64, 128, 191, 255], dtype=np.uint8)

# sensor (w, h), rows of W, views trained, patches scored: the smallest shapes at which the kernels can still go wrong (ragged
# tiles, M != N, one view, two views, more than 64 headings)
CASES = {
    "5x3_f1": dict(w=5, h=3, M=15, F=1, A=1, seed=11),
    "5x3_f2": dict(w=5, h=3, M=15, F=2, A=1, seed=12),
    "40x1": dict(w=40, h=1, M=24, F=37, A=16, seed=13),
    "16x16_a16": dict(w=16, h=16, M=256, F=130, A=16, seed=14),
    "16x16_a65": dict(w=16, h=16, M=256, F=130, A=65, seed=14),
    "20x13": dict(w=20, h=13, M=70, F=33, A=60, seed=15),
}


def route_views(seed, n, h, w):
    """uint8[n,h,w]: overlapping windows of one random 5-level strip, one pixel apart -- a route's views."""
    rng = np.random.default_rng(seed)
    strip = LEVELS[rng.integers(0, len(LEVELS), (h, w + n))]
    return np.ascontiguousarray(np.stack([strip[:, f:f + w] for f in range(n)]))


def initial_weights(M, N, seed=0):
    W = np.random.default_rng(seed).standard_normal((M, N))
    W -= W.mean(axis=1, keepdims=True)
    W /= W.std(axis=1, keepdims=True)
    return W


class _Order(object):
    """The order every sum of one run is taken in: as stored, or permuted (the same permutations all along the run)."""

    def __init__(self, M, N, order_seed):
        if order_seed is None:
            self.cols = self.rows = None
        else:
            rng = np.random.default_rng(order_seed)
            self.cols, self.rows = rng.permutation(N), rng.permutation(M)

    def total(self, v, which):
        p = self.cols if which == "cols" else self.rows
        return np.sum(v if p is None else v[p])

    def wx(self, W, x):
        return W @ x if self.cols is None else W[:, self.cols] @ x[self.cols]

    def hw(self, h, W):
        return h @ W if self.rows is None else h[self.rows] @ W[self.rows, :]


def prepare(plane, dtype=np.float64, order=None):
    v = np.asarray(plane).reshape(-1).astype(dtype) / dtype(255)
    total = np.sum(v) if order is None else order.total(v, "cols")
    return v - total / dtype(v.size)


def train(W, planes, eta=ETA, dtype=np.float64, order_seed=None):
    """One pass of the rule over uint8[n,h,w] planes, in order; returns the new W (dtype)."""
    W = np.array(W, dtype=dtype)
    M, N = W.shape
    order = _Order(M, N, order_seed)
    rate = dtype(eta) / dtype(N)
    for p in planes:
        x = prepare(p, dtype, order)
        h = order.wx(W, x)
        y = np.tanh(h)
        u = order.hw(h, W)
        W = W + rate * (W - np.outer(y + h, u))
    return W


def familiarity(W, planes, dtype=np.float64, order_seed=None):
    """-d of each of uint8[n,h,w] planes."""
    W = np.asarray(W, dtype=dtype)
    order = _Order(W.shape[0], W.shape[1], order_seed)
    return np.array([-order.total(np.abs(order.wx(W, prepare(p, dtype, order))), "rows") for p in planes], dtype=dtype)


@functools.lru_cache(maxsize=None)
def case_data(key):
    """The inputs of a case and the float64 restatement on them, computed once: dict(views, patches, W0, W, fam)."""
    c = CASES[key]
    N = c["w"] * c["h"]
    views = route_views(c["seed"], c["F"], c["h"], c["w"])
    # patches: some trained views, the rest windows of another strip (novel)
    novel = route_views(c["seed"] + 1000, c["A"], c["h"], c["w"])
    patches = novel.copy()
    patches[::3] = views[np.arange(len(patches[::3])) % c["F"]]
    W0 = initial_weights(c["M"], N, c["seed"])
    W = train(W0, views)
    for a in (views, patches, W0, W):
        a.setflags(write=False)
    fam = familiarity(W, patches)
    fam.setflags(write=False)
    return dict(c, N=N, views=views, patches=patches, W0=W0, W=W, fam=fam)


def discrepancies(key):
    """(W vs longdouble, d vs longdouble, W vs permuted order, d vs permuted order) of the float64 restatement at a case, relative."""
    d = case_data(key)
    out = []
    for kw in (dict(dtype=np.longdouble), dict(order_seed=99)):
        W2 = train(d["W0"], d["views"], **kw)
        out.append(float(np.max(np.abs(W2 - d["W"])) / np.max(np.abs(d["W"]))))
        # scores on the SAME weights, as the GPU test takes them
        f2 = familiarity(d["W"], d["patches"], **kw)
        out.append(float(np.max(np.abs(f2 - d["fam"])) / np.max(np.abs(d["fam"]))))
    return tuple(out)


def best_margin(fam):
    """Gap between the best and the second-best value, relative to the best's size."""
    s = np.sort(np.asarray(fam, dtype=np.float64))
    return np.inf if len(s) < 2 else float((s[-1] - s[-2]) / abs(s[-1]))


def diverging_eta():
    """A learning rate at which this restatement overflows on the 16x16 case's views (found here, on the CPU; the host test checks
    it): ten times the smallest that did."""
    return 1.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
