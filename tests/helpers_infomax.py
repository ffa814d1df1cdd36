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
    7x5,   1043, 3          4.8e-16  1.1e-16                 8.8e-16  1.2e-16
    33x31, 20,   6          2.3e-16  2.9e-16                 2.2e-16  6.1e-16
    32x32, 1040, 11         5.5e-16  2.5e-16                 4.7e-16  3.7e-16

The largest is 1.37e-15; the bound is that times 1000 (the margin for the device's tanh and tree reductions; the rule is contractive
at the tested learning rate, so errors do not grow along the chain), rounded up to one digit: TOL = 2e-12, beside the project's 1e-12
score contract.  tests/test_infomax_host.py measures the table again and holds TOL to it; nothing here comes from the code under
test.  On the same data: max|W| after training 2.5 .. 4.3; the 16x16 case scores its trained views near -645 and novel ones near
-920; the best heading of every case leads the second by at least 3e-3 relative, far above TOL; at learning rates of 0.1 and more
the float64 restatement overflows on the 16x16 case's views within its 130 views (0.01 stays finite), which is where the
divergence test takes its rate from.  The last three cases are the smallest at which the kernels' strided loops take a further
trip (see CASES); max|W| 3.6 .. 4.8, best heading ahead by 0.33, 0.26 and 0.049.

The cases with more than 256 pixels a second time from W0 + 1/N (MEAN_KEYS, offset_case_data: rows that sum to 1, without which W x
does not depend on the mean taken off a view -- a mean that misses ONE pixel moves d by 3e-16 under the weights above and by 6e-6 ..
2e-4 under these):

    20x13, 70,  33          5.6e-16  2.9e-16                 2.6e-16  4.6e-16
    33x31, 20,   6          2.4e-16  2.2e-16                 2.2e-16  4.8e-16
    32x32, 1040, 11         5.0e-16  2.3e-16                 5.6e-16  3.7e-16

Two chains outside CASES, measured the same way (weights only):

    LONG_CHAIN  32x32, 4 rows, 8197 views at ETA       6.7e-15 vs longdouble, 1.1e-15 vs permuted order
    SENSED      32x32, 1040 rows, 45 sensed views, 1e-3  7.7e-16 vs longdouble, 3.8e-16 vs permuted order

Along 8197 views the rounding of the chain accumulates: 1000 x 6.75e-15 is above TOL, so that chain has a bound of its own by the
same rule, TOL_LONG_CHAIN = 7e-12 (1000 x its largest discrepancy, rounded up to one digit; no cap shared with TOL).  The sensed
chain passes the rule under TOL itself.  tests/test_infomax_host.py measures both again.

The sensed chains under the sensor's options (tests/helpers_sensed_models.py: 45 sensed views at 1e-3, 20 rows, 70 for odd; scores of
5 x 13 + 13 sensed headings on the trained weights), the larger of the two discrepancies each (vs longdouble, vs permuted order):

    configuration (w x h), channel     W         d
    px    16x8    H / S / V            6.3e-16 / 8.9e-16 / 5.7e-16     3.6e-16 / 2.3e-16 / 2.6e-16
    odd   19x17   H / S / V            8.8e-16 / 8.3e-16 / 8.6e-16     3.2e-16 / 4.1e-16 / 3.3e-16
    tall  6x23    H / S / V            8.6e-16 / 7.6e-16 / 6.4e-16     4.0e-16 / 3.1e-16 / 2.7e-16
    wide  34x10   H / V                7.3e-16 / 7.4e-16               4.5e-16 / 5.9e-16
    sq    32x32   V (flag tests)       6.6e-16                         4.9e-16

and the scores of the flag layouts (5 x 9 and 3 x 70 headings at the landscape's edge) 3.7e-16 .. 5.5e-16.  The largest is 8.9e-16:
all pass the rule under TOL.  tests/test_sensed_models_host.py measures them again.
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
    # the smallest shapes at which the kernels' strided loops take a further trip: more than 64 row tiles of 16 (M > 1024: the lanes
    # of k_im_dfinish / k_im_decide take a second tile; 17 row blocks of 64 in k_im_ureduce), more than one 16-column chunk with
    # N % 4 != 0 (the scalar loads), several elements per thread in k_im_prep and several column blocks of 256 (N > 256).  F is at
    # least ceil(A / 3): with fewer views two of the planted patches are one view and the best heading's margin is 0
    "7x5_m1043": dict(w=7, h=5, M=1043, F=3, A=5, seed=19),
    "33x31": dict(w=33, h=31, M=20, F=6, A=17, seed=17),
    "32x32_m1040": dict(w=32, h=32, M=1040, F=11, A=33, seed=18),
}

# Every W of CASES has rows that sum to zero: initial_weights takes each row's mean off and the rule keeps it so (u . 1 = h^T (W 1) = 0),
# and then W x = W v - mean(v) (W 1) does not depend on the mean that is taken off a view: no case above would notice a wrong one.
# These cases -- N > 256, where a thread of k_im_prep sums more than one pixel: 4 threads with two, 4 each with a ragged end, 4 each --
# are run a second time from W0 + 1/N, rows that sum to 1 (offset_case_data)
MEAN_KEYS = ("20x13", "33x31", "32x32_m1040")

# The chain that enters the slab loop of the training a second time: the x vectors of 32x32 views are staged 64 MiB / (8 * 1024) =
# 8192 at a time.  Too long for TOL (see the docstring), so it has a bound of its own and is no member of CASES.
LONG_CHAIN = dict(w=32, h=32, M=4, F=8192 + 5, seed=20)
TOL_LONG_CHAIN = 7e-12

# The sensed path at a wrapped shape: one agent with a 32x32 sensor on synth.synth_landscape, 1040 rows (65 row tiles), trained on 45
# poses at the rate the README gives as stable for such views.
SENSED = dict(sensor=(32, 32), M=1040, n_poses=45, eta=0.001, seed=21, land=(3, 300, 4))


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


def _discrepancies(d):
    out = []
    for kw in (dict(dtype=np.longdouble), dict(order_seed=99)):
        W2 = train(d["W0"], d["views"], **kw)
        out.append(float(np.max(np.abs(W2 - d["W"])) / np.max(np.abs(d["W"]))))
        # scores on the SAME weights, as the GPU test takes them
        f2 = familiarity(d["W"], d["patches"], **kw)
        out.append(float(np.max(np.abs(f2 - d["fam"])) / np.max(np.abs(d["fam"]))))
    return tuple(out)


def discrepancies(key):
    """(W vs longdouble, d vs longdouble, W vs permuted order, d vs permuted order) of the float64 restatement at a case, relative."""
    return _discrepancies(case_data(key))


@functools.lru_cache(maxsize=None)
def offset_case_data(key):
    """case_data(key) run again from W0 + 1/N -- rows that sum to 1 -- so that the mean of a view shows in W x (see MEAN_KEYS)."""
    d = case_data(key)
    W0 = d["W0"] + 1.0 / d["N"]
    W = train(W0, d["views"])
    fam = familiarity(W, d["patches"])
    for a in (W0, W, fam):
        a.setflags(write=False)
    return dict(d, W0=W0, W=W, fam=fam)


def offset_discrepancies(key):
    """discrepancies() of offset_case_data(key)."""
    return _discrepancies(offset_case_data(key))


def familiarity_with_mean_off(W, planes, by):
    """familiarity() with every view's mean taken too small by `by` (1/N: the mean that misses one pixel of value 255)."""
    W = np.asarray(W, dtype=np.float64)
    return np.array([-np.sum(np.abs(W @ (prepare(p) + by))) for p in planes])


def chain_discrepancy(W0, views, W, eta):
    """The float64 chain W = train(W0, views, eta) against the same chain in longdouble and in a permuted order: the larger, relative."""
    return max(float(np.max(np.abs(train(W0, views, eta=eta, **kw) - W)) / np.max(np.abs(W)))
               for kw in (dict(dtype=np.longdouble), dict(order_seed=99)))


@functools.lru_cache(maxsize=None)
def long_chain_data():
    """LONG_CHAIN's inputs and the float64 restatement on them, computed once: dict(views, W0, W)."""
    c = LONG_CHAIN
    views = route_views(c["seed"], c["F"], c["h"], c["w"])
    W0 = initial_weights(c["M"], c["w"] * c["h"], c["seed"])
    W = train(W0, views)
    for a in (views, W0, W):
        a.setflags(write=False)
    return dict(c, N=c["w"] * c["h"], views=views, W0=W0, W=W)


def sensed_route():
    from navsim_amd import synth
    return synth.sin_training_path(0.5, 60, 180, arclen=1.0)[:SENSED["n_poses"]]


def sensed_agent(model, gpu_sensor, n_test_angles=9):
    import navsim_amd
    from navsim_amd import synth
    return navsim_amd.NavBySceneFamiliarity(synth.synth_landscape(*SENSED["land"]), SENSED["sensor"], 1.0, n_test_angles=n_test_angles,
                                            use_gpu_sensor=gpu_sensor, familiarity_model=model)


@functools.lru_cache(maxsize=None)
def sensed_data():
    """SENSED's views as the host sensor model takes them (an agent without an engine: its plug-in only keeps the scenes) and the
    float64 restatement on their V planes, computed once: dict(scenes uint8[n,h,w,3], views uint8[n,h,w], W0, W)."""
    def keep(scenes):
        def func(scene, fambuf):
            fambuf[...] = 0.0
        func.max_familiarity = 0.0
        return func

    c = SENSED
    agent = sensed_agent(keep, False)
    agent.train_from_path(sensed_route())
    scenes = np.array(agent.familiar_scenes)
    views = np.ascontiguousarray(scenes[..., 2])
    W0 = initial_weights(c["M"], views.shape[1] * views.shape[2], c["seed"])
    W = train(W0, views, eta=c["eta"])
    for a in (scenes, views, W0, W):
        a.setflags(write=False)
    return dict(c, scenes=scenes, views=views, W0=W0, W=W)


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
