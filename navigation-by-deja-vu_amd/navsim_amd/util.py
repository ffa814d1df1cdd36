"""navsim.util counterpart: the familiarity-model plug-in, backed by the HIP engine.

Reference: navsim/util.pyx:10-25 (`sads_familiarity(chem_weight)` -> `internal(scenes)` -> `func`).
"""
import numpy as np

from .engine import FamiliarityEngine, one_value_prefix


def sads_familiarity(chem_weight=0.0, device=0, exact=False, devices=None):
    """Two-stage factory with the reference's shape.

    stage 1  sads_familiarity(chem_weight)          binds the weight          (util.pyx:10)
    stage 2  model(scenes: uint8[F,h,w,3]) -> func  uploads the library once  (util.pyx:11-13)
    func(scene: uint8[h,w,3], fambuf: float64[F])   writes fambuf in place    (util.pyx:14-20)
    func.max_familiarity = h*w                                                (util.pyx:22)

    Extras carried by `func` (used by the agent's fused step): func.engine, func.chem_weight.
    `exact=True` makes every fambuf value the reference's double bit for bit (slower fp64 kernel);
    the default integer-sum scores are within 1e-12 relative of it.
    `devices=[d0, d1, ...]`: ONE process, the library cut into contiguous blocks over these devices
    (navsim_amd.group.FamiliarityGroup over a dv_group); func.engine.step is then the merged, unsharded decision.  The agent
    senses its patches with the host sensor model in that form.
    """
    if devices is not None:
        return _group_sads_familiarity(chem_weight, list(devices))

    def bind(engine, scenes):
        maxfam = scenes[0].shape[0] * scenes[0].shape[1]

        def func(scene, fambuf):
            engine.score(scene, fambuf)

        func.max_familiarity = maxfam
        func.engine = engine
        func.chem_weight = chem_weight
        return func

    def sads_familiarity_internal(scenes):
        assert 0 <= chem_weight <= 1
        engine = FamiliarityEngine(device=device, exact=exact)
        engine.set_library(scenes, chem_weight)
        return bind(engine, scenes)

    # Hooks for navsim_amd.NavBySceneFamiliarity: it creates the engine early (landscape and sensor model live on
    # the GPU too), builds the library on the device and then binds `func` to that engine.
    def make_engine():
        assert 0 <= chem_weight <= 1
        return FamiliarityEngine(device=device, exact=exact)

    sads_familiarity_internal.make_engine = make_engine
    sads_familiarity_internal.from_engine = bind
    sads_familiarity_internal.chem_weight = chem_weight
    return sads_familiarity_internal


def _group_sads_familiarity(chem_weight, devices):
    reject_infomax(chem_weight, "FamiliarityGroup")
    def sads_familiarity_internal(scenes):
        assert 0 <= chem_weight <= 1
        from .group import FamiliarityGroup
        group = FamiliarityGroup(devices)
        group.set_library(scenes, chem_weight)

        def func(scene, fambuf):
            group.score(scene, fambuf)

        func.max_familiarity = scenes[0].shape[0] * scenes[0].shape[1]
        func.engine = group
        func.chem_weight = chem_weight
        return func

    sads_familiarity_internal.chem_weight = chem_weight
    return sads_familiarity_internal


hip_sads_familiarity = sads_familiarity


def ssd_familiarity(channel=2, device=0):
    """The north star's literal metric -- the pixel-wise sum of squared differences, the reference's `ssds`
    (navsim/util.pyx:171-184) -- as a familiarity plug-in of the reference's shape (util.pyx:10-25):

    stage 1  ssd_familiarity(channel)                  picks the compared channel of HSV scenes (0 H, 1 S, 2 V)
    stage 2  model(scenes) -> func                     uploads the library once:
                 uint8[F,h,w,3] / uint8[F,h,w]         -> the ssd_u8 metric: exact integer sums on the int8 matrix cores
                 float32[F,h,w]                        -> the ssd_f32 metric (within 1e-6 relative of ssds on the upcast data)
    func(scene, fambuf: float64[F])                    writes fambuf[f] = -SSD(scene, view f) in place: the most familiar view
                                                       is the one with the least SSD, as np.max / np.argmax of the agent's loop
                                                       (NavBySceneFamiliarity.py:313,315) expect
    func.max_familiarity = 0.0                         (an identical scene)

    Extras carried by `func` for the agent's fused step: func.engine, func.metric ("ssd_u8" / "ssd_f32"), func.channel.
    """
    if channel not in (0, 1, 2):
        raise ValueError("channel must be 0 (H), 1 (S) or 2 (V), got %r" % (channel,))

    def plane(a, lead):
        """The compared plane of a scene array: [.., h, w, 3] -> [.., h, w]; a single-channel array as it is."""
        a = np.asarray(a)
        if a.ndim == lead + 3:
            a = a[..., channel]
        if a.ndim != lead + 2:
            raise ValueError("scene array has shape %r" % (a.shape,))
        return np.ascontiguousarray(a)

    def bind(engine, metric):
        def func(scene, fambuf):
            if not (isinstance(fambuf, np.ndarray) and fambuf.dtype == np.float64):
                raise ValueError("Buffer dtype mismatch for fambuf, expected 'double'")
            p = plane(scene, 0)
            if metric == "ssd_u8":
                engine.score_u8(p, fambuf)
            else:
                engine.score_f32(p, fambuf)
            np.negative(fambuf, out=fambuf)

        func.max_familiarity = 0.0
        func.engine = engine
        func.metric = metric
        func.channel = channel
        return func

    def ssd_familiarity_internal(scenes):
        scenes = np.asarray(scenes)
        engine = FamiliarityEngine(device=device)
        if scenes.dtype == np.uint8:
            engine.set_library_u8(plane(scenes, 1))
            return bind(engine, "ssd_u8")
        if scenes.dtype == np.float32:
            engine.set_library_f32(plane(scenes, 1))
            return bind(engine, "ssd_f32")
        engine.close()
        raise ValueError("Buffer dtype mismatch, expected 'uint8_t' or 'float' but got '%s'" % scenes.dtype)

    # hooks for navsim_amd.NavBySceneFamiliarity (landscape, sensor model and library on the GPU: see sads_familiarity)
    ssd_familiarity_internal.make_engine = lambda: FamiliarityEngine(device=device)
    ssd_familiarity_internal.from_engine = lambda engine, scenes: bind(engine, "ssd_u8")
    ssd_familiarity_internal.metric = "ssd"
    ssd_familiarity_internal.channel = channel
    return ssd_familiarity_internal


def ncc_familiarity(channel=2, device=0):
    """The correlation coefficient (zero-mean normalised cross-correlation) of one channel, the third perfect-memory metric of the
    view-based navigation literature beside SADS and SSD, invariant to the gain and offset of a view -- as a familiarity plug-in of
    the reference's shape (util.pyx:10-25):

    stage 1  ncc_familiarity(channel)                  picks the compared channel of HSV scenes (0 H, 1 S, 2 V)
    stage 2  model(scenes: uint8[F,h,w,3]) -> func     puts the scenes into a one-route view store (rviews_set_u8)
    func(scene: uint8[h,w,3], fambuf: float64[F])      writes fambuf[f] = q(scene, view f) in place (rvncc_scene_u8 with one member and
                                                       one heading): in [-1, 1], 0.0 where a plane is constant
    func.max_familiarity = 1.0                         (an identical scene, or one that differs by a gain and an offset)

    Extras carried by `func` for the agent's fused step: func.engine, func.metric ("ncc"), func.channel.
    """
    if channel not in (0, 1, 2):
        raise ValueError("channel must be 0 (H), 1 (S) or 2 (V), got %r" % (channel,))

    def bind(engine, scenes=None):
        def func(scene, fambuf):
            if not (isinstance(fambuf, np.ndarray) and fambuf.dtype == np.float64):
                raise ValueError("Buffer dtype mismatch for fambuf, expected 'double'")
            scene = np.asarray(scene)
            fambuf[...] = engine.rvncc_scene_u8(scene.reshape((1, 1) + scene.shape), [0], channel)[0]

        func.max_familiarity = 1.0
        func.engine = engine
        func.metric = "ncc"
        func.channel = channel
        return func

    def ncc_familiarity_internal(scenes):
        scenes = np.asarray(scenes)
        if scenes.dtype != np.uint8:
            raise ValueError("Buffer dtype mismatch, expected 'uint8_t' but got '%s'" % scenes.dtype)
        engine = FamiliarityEngine(device=device)
        try:
            engine.rviews_set_u8(scenes, [0, len(scenes)])
        except Exception:
            engine.close()
            raise
        return bind(engine)

    # hooks for navsim_amd.NavBySceneFamiliarity (landscape, sensor model and view store on the GPU: see sads_familiarity)
    ncc_familiarity_internal.make_engine = lambda: FamiliarityEngine(device=device)
    ncc_familiarity_internal.from_engine = bind
    ncc_familiarity_internal.metric = "ncc"
    ncc_familiarity_internal.channel = channel
    return ncc_familiarity_internal


def reject_ncc(model, what):
    """Every ensemble but NccRouteEnsemble scores a view library, an Infomax matrix or a mushroom body: the NCC model's views lie in
    the route view store and only navsim_amd.NccRouteEnsemble's step scores them there.  Raises ValueError for an NCC model (the
    factory's product, its bound func, or an agent that carries one)."""
    for obj in (model, getattr(model, "familiarity_model", None), getattr(model, "_familiarity_func", None)):
        if getattr(obj, "metric", None) == "ncc":
            raise ValueError("%s does not take an NCC model: ncc_familiarity scores the views of the route view store, which only "
                             "navsim_amd.NccRouteEnsemble batches (or step each agent on its own engine)" % what)


def reject_infomax(model, what):
    """The batched and multi-device forms score a library; the Infomax model has none.  Raises ValueError for an Infomax model (the
    factory's product, its bound func, or an agent that carries one)."""
    for obj in (model, getattr(model, "familiarity_model", None), getattr(model, "_familiarity_func", None)):
        if getattr(obj, "metric", None) == "infomax":
            raise ValueError("%s does not take an Infomax model: it batches or shards a view library, and infomax_familiarity keeps "
                             "none (step each agent on its own engine, or use navsim_amd.InfomaxEnsemble)" % what)
    reject_mushroom(model, what)


def reject_mushroom(model, what):
    """The same refusal for the mushroom-body model (mushroom_familiarity): it keeps no library either; navsim_amd.MushroomEnsemble is
    the one batched form that takes it."""
    for obj in (model, getattr(model, "familiarity_model", None), getattr(model, "_familiarity_func", None)):
        if getattr(obj, "metric", None) == "mushroom":
            raise ValueError("%s does not take a mushroom-body model: it batches or shards a view library (or one Infomax weight "
                             "matrix), and mushroom_familiarity keeps neither (step each agent on its own engine, or use "
                             "navsim_amd.MushroomEnsemble)" % what)
    reject_ncc(model, what)


def route_ensemble_name(agent):
    """The ensemble that steps a banked member of `agent`'s model."""
    metrics = [getattr(obj, "metric", None) for obj in (agent, getattr(agent, "familiarity_model", None), getattr(agent, "_familiarity_func", None))]
    if "infomax" in metrics:
        return "InfomaxRouteEnsemble"
    if "ncc" in metrics:
        return "NccRouteEnsemble"
    if any(str(m).startswith("ssd") for m in metrics if m is not None):
        return "SsdRouteEnsemble"                                 # (ssd_familiarity: "ssd", its bound func "ssd_u8")
    if all(m is None for m in metrics) and getattr(getattr(agent, "familiarity_model", None), "chem_weight", None) is not None:
        return "SadsRouteEnsemble"                                # (the perfect-memory model's product carries a weight and no metric)
    return "MushroomRouteEnsemble"


def reject_banked(agent, what):
    """The refusal of every ensemble but the member's own route ensemble (navsim_amd.MushroomRouteEnsemble, InfomaxRouteEnsemble): the
    member's route is kept in a bank of its own (agent.memory_bank), and the other ensembles' steps score under the model's first bank."""
    if getattr(agent, "memory_bank", None) is not None:
        if route_ensemble_name(agent) in ("SadsRouteEnsemble", "SsdRouteEnsemble", "NccRouteEnsemble"):
            raise ValueError("%s does not take a member of a %s: its route is route %d of the engine's view store, "
                             "and only that ensemble's step scores it there" % (what, route_ensemble_name(agent), agent.memory_bank))
        raise ValueError("%s does not take a member of a %s: its route is kept in memory bank %d of the shared model, "
                         "and only that ensemble's step scores it there" % (what, route_ensemble_name(agent), agent.memory_bank))


def _one_value_familiarity(metric, channel, device, begin, **extras):
    """Stage 2 of a model that keeps no library (infomax_familiarity, mushroom_familiarity): `begin(engine, h, w)` makes a fresh model
    of h x w views; the engine's <prefix>_train_u8 / <prefix>_score_u8 are the ones of `metric`.  `extras` become attributes of the product."""
    prefix = one_value_prefix(metric)

    def plane(a, lead):
        a = np.asarray(a)
        if a.ndim == lead + 3:
            a = a[..., channel]
        if a.ndim != lead + 2:
            raise ValueError("scene array has shape %r" % (a.shape,))
        return np.ascontiguousarray(a)

    def bind(engine, scenes=None):
        score_u8 = getattr(engine, prefix + "score_u8")

        def func(scene, fambuf):
            if not (isinstance(fambuf, np.ndarray) and fambuf.dtype == np.float64):
                raise ValueError("Buffer dtype mismatch for fambuf, expected 'double'")
            fambuf[...] = score_u8(plane(scene, 0))[0]

        func.max_familiarity = 0.0
        func.engine = engine
        func.metric = metric
        func.channel = channel
        return func

    def internal(scenes):
        scenes = np.asarray(scenes)
        if scenes.dtype != np.uint8:
            raise ValueError("Buffer dtype mismatch, expected 'uint8_t' but got '%s'" % scenes.dtype)
        planes = plane(scenes, 1)
        engine = FamiliarityEngine(device=device)
        try:
            begin(engine, planes.shape[1], planes.shape[2])
            getattr(engine, prefix + "train_u8")(planes)
        except Exception:
            engine.close()
            raise
        return bind(engine)

    # hooks for navsim_amd.NavBySceneFamiliarity (landscape, sensor model and training on the GPU: see sads_familiarity)
    internal.__name__ = internal.__qualname__ = "%s_familiarity_internal" % metric
    internal.make_engine = lambda: FamiliarityEngine(device=device)
    internal.from_engine = bind
    internal.begin = begin
    internal.metric = metric
    internal.channel = channel
    for name, value in extras.items():
        setattr(internal, name, value)
    return internal


def infomax_initial_weights(n_hidden, n_pixels, seed=0):
    """The Infomax model's initial W, float64[n_hidden, n_pixels], drawn on the host: standard normal from
    np.random.default_rng(seed), then every row has its mean subtracted and is divided by its standard deviation (ddof=0)."""
    w = np.random.default_rng(seed).standard_normal((int(n_hidden), int(n_pixels)))
    w -= w.mean(axis=1, keepdims=True)
    w /= w.std(axis=1, keepdims=True)
    return w


def infomax_familiarity(channel=2, learning_rate=0.01, seed=0, n_hidden=None, device=0, devices=None):
    """The Infomax network of Baddeley, Graham, Husbands & Philippides (2012) as a familiarity plug-in of the reference's shape
    (util.pyx:10-25): a fixed-size memory -- one layer of weights W, float64[n_hidden, h*w], trained in one pass over the route's
    views -- where sads_familiarity and ssd_familiarity keep every view.

    stage 1  infomax_familiarity(channel, learning_rate, seed, n_hidden)   the compared channel of HSV scenes (0 H, 1 S, 2 V), the
                                                       rule's learning rate, the seed of the initial W and its number of rows
                                                       (None: as many as the view has pixels)
    stage 2  model(scenes) -> func                     trains on uint8[F,h,w,3] / uint8[F,h,w], in order, on the device
    func(scene, fambuf: float64[F])                    writes the ONE value -d(scene) = -sum|W x| into EVERY entry of fambuf: np.max
                                                       of it is the heading's familiarity, so the reference's loop
                                                       (NavBySceneFamiliarity.py:301-315) works unchanged -- and the agent's
                                                       scene_familiarity is therefore constant over the views (the least familiarity
                                                       over the headings): the model keeps no per-view memory
    func.max_familiarity = 0.0

    With x = p/255 - mean(p/255) of the view's plane, a training view does h = W x; y = tanh(h); u = h^T W;
    W <- W + (learning_rate / N) (W - (y + h) u^T).  A learning rate too large for the views makes the rule diverge: training then
    raises EngineError.  Extras carried by `func`: func.engine (engine.infomax_read_weights() / infomax_set_weights() save and restore
    the model), func.metric ("infomax"), func.channel.
    """
    if devices is not None:
        raise ValueError("infomax_familiarity runs on one device (device=...): FamiliarityGroup cuts a view library over several, and "
                         "this model keeps none")
    if channel not in (0, 1, 2):
        raise ValueError("channel must be 0 (H), 1 (S) or 2 (V), got %r" % (channel,))
    if not (isinstance(learning_rate, (int, float, np.floating, np.integer)) and learning_rate > 0 and np.isfinite(learning_rate)):
        raise ValueError("learning_rate must be a positive number, got %r" % (learning_rate,))
    if n_hidden is not None and not (isinstance(n_hidden, (int, np.integer)) and n_hidden >= 1):
        raise ValueError("n_hidden must be a positive integer or None, got %r" % (n_hidden,))

    def begin(engine, h, w):
        """A fresh model of h x w views on `engine` (the agent calls this before it trains from poses)."""
        n = int(h) * int(w)
        engine.infomax_begin(h, w, infomax_initial_weights(n if n_hidden is None else n_hidden, n, seed), channel, learning_rate)

    return _one_value_familiarity("infomax", channel, device, begin, learning_rate=learning_rate, seed=seed, n_hidden=n_hidden)


def infomax_network(n_pixels, n_hidden=None, learning_rate=0.01, seed=0, channel=2):
    """One network of an Infomax network table (FamiliarityEngine.inet_set) over views of n_pixels pixels:
    dict(channel, n_hidden, learning_rate, w0) with n_hidden = n_pixels where None is given and
    w0 = infomax_initial_weights(n_hidden, n_pixels, seed) -- what infomax_familiarity of the same arguments begins its engine with."""
    if isinstance(n_pixels, bool) or not isinstance(n_pixels, (int, np.integer)) or n_pixels < 1:
        raise ValueError("n_pixels must be a positive integer, got %r" % (n_pixels,))
    infomax_familiarity(channel=channel, learning_rate=learning_rate, seed=seed, n_hidden=n_hidden)      # (its argument checks)
    m = int(n_pixels) if n_hidden is None else int(n_hidden)
    return dict(channel=int(channel), n_hidden=m, learning_rate=float(learning_rate), w0=infomax_initial_weights(m, n_pixels, seed))


def mushroom_connectivity(n_kc, n_pixels, fan_in, seed=0):
    """The mushroom-body model's fan-in, int32[n_kc, fan_in], drawn on the host: the pixels each Kenyon cell listens to, from
    np.random.default_rng(seed).integers(0, n_pixels, (n_kc, fan_in)).  A pixel repeated in a row counts twice."""
    return np.random.default_rng(seed).integers(0, int(n_pixels), (int(n_kc), int(fan_in))).astype(np.int32)


def mushroom_population(n_pixels, n_kc=20000, fan_in=10, sparsity=0.01, seed=0, channel=2):
    """One population of a mushroom-body population table (FamiliarityEngine.mbpop_set) over views of n_pixels pixels:
    dict(channel, n_kc, fan_in, n_active, conn) with conn = mushroom_connectivity(n_kc, n_pixels, fan_in, seed) and
    n_active = max(1, round(sparsity * n_kc)) -- what mushroom_familiarity of the same arguments begins its engine with."""
    if isinstance(n_pixels, bool) or not isinstance(n_pixels, (int, np.integer)) or n_pixels < 1:
        raise ValueError("n_pixels must be a positive integer, got %r" % (n_pixels,))
    model = mushroom_familiarity(channel=channel, n_kc=n_kc, fan_in=fan_in, sparsity=sparsity, seed=seed)      # (its argument checks)
    return dict(channel=int(channel), n_kc=int(n_kc), fan_in=int(fan_in), n_active=model.n_active,
                conn=mushroom_connectivity(n_kc, n_pixels, fan_in, seed))


def mushroom_familiarity(channel=2, n_kc=20000, fan_in=10, sparsity=0.01, seed=0, device=0, devices=None):
    """The mushroom-body circuit of Ardin, Peng, Mangan, Lagogiannis & Webb (2016) as a familiarity plug-in of the reference's shape
    (util.pyx:10-25): a memory of fixed size and finite capacity -- one byte of output weight per Kenyon cell -- where sads_familiarity
    and ssd_familiarity keep every view and infomax_familiarity a float64 matrix.

    stage 1  mushroom_familiarity(channel, n_kc, fan_in, sparsity, seed)   the compared channel of HSV scenes (0 H, 1 S, 2 V), the number
                                                       of Kenyon cells, the pixels each listens to (1..16), the fraction of cells that
                                                       fire for a view (n_active = max(1, round(sparsity * n_kc))) and the seed of the
                                                       fan-in (mushroom_connectivity)
    stage 2  model(scenes) -> func                     trains on uint8[F,h,w,3] / uint8[F,h,w] on the device, all views in one launch
    func(scene, fambuf: float64[F])                    writes the ONE value -d(scene) into EVERY entry of fambuf, as infomax_familiarity
                                                       does: the model keeps no per-view memory
    func.max_familiarity = 0.0

    A cell's activity is the sum of its pixels; the n_active most excited fire (larger sum first, then lower index: the sensor's planes
    have five levels, so the tie rule decides at every view); training clears the weight of every cell that fired, and d is the number
    of a view's firing cells whose weight is intact: 0 for a trained view, n_active at most.  Integer from pixel to score, so exact.
    Extras carried by `func`: func.engine (engine.mb_read_weights() / mb_set_weights() save and restore the model,
    engine.mb_info()["n_depressed"] tells how full it is), func.metric ("mushroom"), func.channel.
    """
    if devices is not None:
        raise ValueError("mushroom_familiarity runs on one device (device=...): FamiliarityGroup cuts a view library over several, and "
                         "this model keeps none")
    if channel not in (0, 1, 2):
        raise ValueError("channel must be 0 (H), 1 (S) or 2 (V), got %r" % (channel,))
    if not (isinstance(n_kc, (int, np.integer)) and not isinstance(n_kc, bool) and n_kc >= 1):
        raise ValueError("n_kc must be a positive integer, got %r" % (n_kc,))
    if not (isinstance(fan_in, (int, np.integer)) and not isinstance(fan_in, bool) and 1 <= fan_in <= 16):
        raise ValueError("fan_in must be an integer in [1, 16], got %r" % (fan_in,))
    if not (isinstance(sparsity, (int, float, np.floating, np.integer)) and not isinstance(sparsity, bool) and 0 < sparsity <= 1):
        raise ValueError("sparsity must be a number in (0, 1], got %r" % (sparsity,))
    n_active = max(1, int(round(sparsity * n_kc)))

    def begin(engine, h, w):
        """A fresh model of h x w views on `engine` (the agent calls this before it trains from poses)."""
        engine.mb_begin(h, w, mushroom_connectivity(n_kc, int(h) * int(w), fan_in, seed), n_active, channel)

    return _one_value_familiarity("mushroom", channel, device, begin, n_kc=n_kc, fan_in=fan_in, n_active=n_active, sparsity=sparsity, seed=seed)
