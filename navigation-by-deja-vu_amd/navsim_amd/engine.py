"""FamiliarityEngine -- Python face of one dv_ctx (one GPU, one stored-view library shard)."""
import ctypes
from types import SimpleNamespace

import numpy as np

from . import _native as N


def agent_weights(chem_weights, n):
    """chem_weights of a weighted batch as float64[n] (None stays None: the unweighted call).  The range [0, 1] and the layout are
    the library's to check (dv_step_batch_weighted names the agent it refuses)."""
    if chem_weights is None:
        return None
    w = np.ascontiguousarray(chem_weights, dtype=np.float64).reshape(-1)
    if w.shape[0] != n:
        raise ValueError("chem_weights holds %d weights for %d agents" % (w.shape[0], n))
    return w


class BatchResults(object):
    """The records of an ensemble step (dv_step_batch / dv_sense_step_batch), one per agent.  A sequence of the per-agent result
    dictionaries step() returns -- made when asked for -- and, for callers that only move agents, the same numbers as arrays over
    the records' own memory: best_idex[n], best_view[n], step_familiarity[n], flags[n], n_candidates[n], angle_familiarity[n, A],
    angle_view[n, A].  (32 dictionaries per ensemble step cost the host 60-80 us beside a 0.8 ms device step.)
    scene_familiarity: float64[n, F] after sense_step_batch_scene / step_batch_scene (row i: the per-view minimum over agent i's own
    headings), else None."""
    _DTYPE = np.dtype(N.StepResult)

    def __init__(self, raw, n, A, scene=None):
        self._raw, self.n, self.A = raw, n, A
        self.scene_familiarity = scene
        rec = np.frombuffer(raw, dtype=self._DTYPE, count=n)
        self.records = rec
        self.best_idex, self.best_view, self.step_familiarity = rec["best_heading"], rec["best_view"], rec["best_fam"]
        self.flags, self.n_candidates = rec["flags"], rec["n_candidates"]
        self.angle_familiarity, self.angle_view = rec["angle_fam"][:, :A], rec["angle_view"][:, :A]

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self.n))]
        if i < 0:
            i += self.n
        if not 0 <= i < self.n:
            raise IndexError(i)
        return FamiliarityEngine._result_dict(self._raw[i], None)

    def __iter__(self):
        return (self[i] for i in range(self.n))


class OneValueBatchResults(object):
    """An ensemble step of the Infomax model (dv_batch_infomax_step_u8 / dv_batch_infomax_sense_step) or of the mushroom-body model
    (dv_batch_mb_step_u8 / dv_batch_mb_sense_step), in BatchResults' shape for
    callers that move agents: angle_familiarity[n, A] (float64), best_idex[n] (int32; -1 for a member whose footprint left the
    landscape) and flags[n] (uint32; DV_RES_SENSE_ERROR = 16 for such a member, whose row is unspecified)."""

    def __init__(self, angle_familiarity, best_idex, flags):
        self.n, self.A = angle_familiarity.shape
        self.angle_familiarity, self.best_idex, self.flags = angle_familiarity, best_idex, flags

    def __len__(self):
        return self.n


class RouteViewResults(OneValueBatchResults):
    """A step on the route view store (dv_rviews_step_u8 / dv_rviews_sense_step): OneValueBatchResults and angle_view[n, A] (int64),
    the first view of the member's own route that attains angle_familiarity."""

    def __init__(self, angle_familiarity, angle_view, best_idex, flags):
        OneValueBatchResults.__init__(self, angle_familiarity, best_idex, flags)
        self.angle_view = angle_view

    @property
    def relocalised(self):
        """bool[n]: the member's windowed best lay below its threshold, and its row is the whole-route step's (DV_RES_RELOCALISED)."""
        return (np.asarray(self.flags) & N.DV_RES_RELOCALISED) != 0


class RouteSsdResults(RouteViewResults):
    """An SSD step on the route view store (dv_rvssd_step_u8 / dv_rvssd_sense_step): angle_ssd[n, A] (float64 holding the exact
    integers), angle_view[n, A] the least view of the member's route that attains it, best_idex[n] the first least heading, and
    angle_familiarity = np.negative(angle_ssd): the lone SSD agent's bits, -0.0 included."""

    def __init__(self, angle_ssd, angle_view, best_idex, flags):
        RouteViewResults.__init__(self, np.negative(angle_ssd), angle_view, best_idex, flags)
        self.angle_ssd = angle_ssd


class RouteNccResults(RouteViewResults):
    """An NCC step on the route view store (dv_rvncc_step_u8 / dv_rvncc_sense_step): angle_ncc[n, A] (float64, the largest correlation
    coefficient over the member's route), angle_view[n, A] the least view that attains it, best_idex[n] the first largest heading;
    angle_familiarity IS angle_ncc (the same array)."""

    def __init__(self, angle_ncc, angle_view, best_idex, flags):
        RouteViewResults.__init__(self, angle_ncc, angle_view, best_idex, flags)
        self.angle_ncc = angle_ncc


class MbSetBatchResults(OneValueBatchResults):
    """A bank-set step of the mushroom-body model (dv_mbset_step_u8 / dv_mbset_sense_step / dv_mbset_lands_sense_step):
    OneValueBatchResults and bank_novelty[n, A, S] (int32), the column's novelty under each bank of its member's set."""

    def __init__(self, angle_familiarity, best_idex, flags, bank_novelty):
        OneValueBatchResults.__init__(self, angle_familiarity, best_idex, flags)
        self.bank_novelty = bank_novelty


InfomaxBatchResults = OneValueBatchResults    # the name it had while Infomax was the only such model

# The one-value models -- no library, ONE value per heading: metric -> (prefix of the single calls' symbols, of the batch calls', the
# engine attribute that holds the model's (h, w), prefix of the banked calls' symbols, of the banked calls on a landscape set, the
# engine attribute that holds the model's number of banks).
_ONE_VALUE = {"infomax": ("dv_infomax_", "dv_batch_infomax_", "infomax_shape", "dv_ibank_", "dv_lands_ibank_", "infomax_banks"),
              "mushroom": ("dv_mb_", "dv_batch_mb_", "mb_shape", "dv_mbank_", "dv_lands_mbank_", "mb_banks")}
ONE_VALUE_METRICS = tuple(_ONE_VALUE)


def one_value_prefix(metric):
    """"infomax_" / "mb_": what the names of the engine's methods for the one-value model `metric` begin with."""
    return _ONE_VALUE[metric][0][3:]


class FamiliarityEngine(object):
    """Scores sensor patches against a stored-view library resident in HBM.

    Replaces, behind the reference's interfaces, navsim/util.pyx:31-73 (the kernel) and the
    heading loop navsim/NavBySceneFamiliarity.py:283-316 (`step`).
    """

    def __init__(self, device=0, exact=False):
        self._lib = N.load()
        self._begun = False                    # an agent step was begun and not ended (agent_step_begin)
        self._ctx_raw = N._ctx_p()
        rc = self._lib.dv_create(ctypes.byref(self._ctx_raw), int(device))
        if rc != 0:
            msg = self._lib.dv_last_error(None)
            raise N.EngineError("dv_create(device=%d) failed: %s (%s)" % (
                device, msg.decode() if msg else "?", N.ERROR_NAMES.get(rc, rc)))
        self.device = int(device)
        self.n_views = 0
        self.shape = None
        self._step_state = None                  # sense_step_into's result record and angle buffer
        self._agent_state = None                 # agent_step's argument buffers
        self._err_out = ctypes.c_double()        # path_error_wait's answer
        self._err_out_ref = ctypes.byref(self._err_out)
        if exact:
            self.set_exact(True)

    # -- plumbing -------------------------------------------------------------------------------
    @property
    def _ctx(self):
        # Every call into the context goes through here, except agent_step_end: whatever it is, it supersedes an agent step that was
        # begun and not ended (the begun step's work stays harmlessly queued on the stream; its record is not read)
        self._begun = False
        return self._ctx_raw

    def _check(self, rc, what):
        if rc != 0:
            msg = self._lib.dv_last_error(self._ctx)
            text = "%s failed: %s (%s)" % (what, msg.decode() if msg else "?", N.ERROR_NAMES.get(rc, rc))
            if rc == -1:
                raise ValueError(text)
            raise N.EngineError(text)

    def close(self):
        if getattr(self, "_ctx_raw", None):
            self._lib.dv_destroy(self._ctx_raw)
            self._ctx_raw = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_exact(self, exact):
        """exact=True: every score is the reference's sequential-double value (fp64 kernel)."""
        self._check(self._lib.dv_set_exact(self._ctx, 1 if exact else 0), "dv_set_exact")

    def set_stream(self, hip_stream):
        self._check(self._lib.dv_set_stream(self._ctx, ctypes.c_void_p(hip_stream or 0)), "dv_set_stream")

    def synchronize(self):
        self._check(self._lib.dv_synchronize(self._ctx), "dv_synchronize")

    # -- library --------------------------------------------------------------------------------
    def set_library(self, scenes, chem_weight=0.0, first_view=0):
        """scenes: uint8[F,h,w,3] (NavBySceneFamiliarity.py:122).  Copied to the GPU and re-tiled."""
        scenes = N.as_u8(scenes, "familiar_scenes")
        if scenes.ndim != 4:
            raise ValueError("familiar_scenes must be uint8[F,h,w,3], got shape %r" % (scenes.shape,))
        F, h, w, ch = scenes.shape
        self._check(self._lib.dv_set_library(self._ctx, N.u8ptr(scenes), F, h, w, ch, float(chem_weight),
                                             int(first_view)), "dv_set_library")
        self.n_views, self.shape = F, (h, w)

    def generate_library(self, seed, n_views, h, w, chem_weight=0.0, first_view=0, full_range_s=False):
        """Same bytes as synth.synth_views(seed, n_views, h, w, first_view, full_range_s), generated in HBM."""
        self._check(self._lib.dv_generate_library_ex(self._ctx, int(seed), int(n_views), int(h), int(w), float(chem_weight),
                                                     int(first_view), 1 if full_range_s else 0), "dv_generate_library_ex")
        self.n_views, self.shape = int(n_views), (int(h), int(w))

    def append_library(self, scenes):
        """More views (uint8[n,h,w,3]) behind the resident ones; only the new view groups are re-tiled.  Raises
        EngineError (DV_ERR_STATE) when they do not fit the resident layout (a new hue, S > 127 on a signed plane)."""
        scenes = N.as_u8(scenes, "familiar_scenes")
        if scenes.ndim != 4 or scenes.shape[1:3] != tuple(self.shape):
            raise ValueError("appended views must be uint8[n,%d,%d,3], got shape %r" % (self.shape + (scenes.shape,)))
        self._check(self._lib.dv_append_library(self._ctx, N.u8ptr(scenes), scenes.shape[0], scenes.shape[3]), "dv_append_library")
        self.n_views += scenes.shape[0]

    def append_library_from_poses(self, x, y, angle, want_views=True):
        """dv_append_library with the views sensed on the device; returns them (uint8[n,h,w,3]) when want_views."""
        x, y, angle = self._pose_arrays(x, y, angle)
        h, w = self.sensor_shape
        out = np.empty((len(x), h, w, 3), dtype=np.uint8) if want_views else None
        self._check_sense(self._lib.dv_append_library_from_poses(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angle), len(x),
                                                                 N.u8ptr(out) if want_views else None), "dv_append_library_from_poses")
        self.n_views += len(x)
        return out

    def set_weight_range(self, lo, hi):
        """Lay later ingests (set_library, set_library_from_poses, generate_library) out for every chem_weight in [lo, hi], so that a
        weighted batch (step_batch / sense_step_batch with chem_weights) may score each agent under its own weight.  The ingest's own
        chem_weight must lie in the range.  lo > hi restores the default: the ingest's weight alone."""
        self._check(self._lib.dv_set_weight_range(self._ctx, float(lo), float(hi)), "dv_set_weight_range")

    def clear_library(self):
        self._check(self._lib.dv_clear_library(self._ctx), "dv_clear_library")
        self.n_views, self.shape = 0, None

    def library_info(self):
        info = N.LibInfo()
        self._check(self._lib.dv_get_library_info(self._ctx, ctypes.byref(info)), "dv_get_library_info")
        return dict(n_views=info.n_views, first_view=info.first_view, h=info.h, w=info.w,
                    n_planes=info.n_planes, n_hue_planes=info.n_hue_planes, generic_hue=bool(info.generic_hue),
                    has_value_plane=bool(info.has_value_plane), tile_bytes=info.tile_bytes,
                    chem_weight=info.chem_weight, delta=info.delta, hues=[int(x) for x in info.hues][:info.n_hues],
                    signed_saturation=bool(info.signed_saturation), has_bit_planes=bool(info.has_bit_planes),
                    bit_planes_hs=info.bit_planes_hs, bit_planes_v=info.bit_planes_v, bit_tile_bytes=info.bit_tile_bytes,
                    fp4_form=bool(info.fp4_form), code_tile_bytes=info.code_tile_bytes, mixed_layout=bool(info.mixed_layout),
                    weight_range=(info.weight_lo, info.weight_hi))

    def read_planes(self, v0, n):
        info = self.library_info()
        out = np.empty((n, info["n_planes"], info["h"] * info["w"]), dtype=np.uint8)
        self._check(self._lib.dv_read_planes(self._ctx, int(v0), int(n), N.u8ptr(out)), "dv_read_planes")
        return out

    # -- sensor model on the GPU ---------------------------------------------------------------
    def set_landscape(self, landscape):
        """landscape: uint8[rows, cols, 3] HSV (any strides; copied).  Kept resident in HBM."""
        landscape = N.as_u8(landscape, "landscape")
        if landscape.ndim != 3 or landscape.shape[2] != 3:
            raise ValueError("landscape must be uint8[rows, cols, 3], got shape %r" % (landscape.shape,))
        self._check(self._lib.dv_set_landscape(self._ctx, N.u8ptr(landscape), landscape.shape[0], landscape.shape[1], 3),
                    "dv_set_landscape")

    def configure_sensor(self, sensor_dimensions, sensor_pixel_dimensions, lut, mask_middle_n):
        lut = np.ascontiguousarray(lut, dtype=np.uint8)
        assert lut.shape == (3, 256)
        self._check(self._lib.dv_configure_sensor(self._ctx, int(sensor_dimensions[0]), int(sensor_dimensions[1]),
                                                  int(sensor_pixel_dimensions[0]), int(sensor_pixel_dimensions[1]),
                                                  N.u8ptr(lut), int(mask_middle_n)), "dv_configure_sensor")
        shape = (int(sensor_dimensions[1]), int(sensor_dimensions[0]))
        if getattr(self, "sensor_shape", shape) != shape:
            self.n_sensors = 0                                   # (a sensor table was checked against the old w x h: the library drops it)
            self.n_noise_rows = 0                                # (w h enters the noise rows' counters: the library drops them)
        self.sensor_shape = shape

    @staticmethod
    def _pose_arrays(x, y, angle):
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        angle = np.ascontiguousarray(angle, dtype=np.float64).reshape(-1)
        assert x.shape == y.shape == angle.shape
        return x, y, angle

    def _check_sense(self, rc, what):
        if rc == -5:
            msg = self._lib.dv_last_error(self._ctx)
            raise IndexError(msg.decode() if msg else "index out of bounds")     # what the reference raises
        self._check(rc, what)

    def sense(self, x, y, angle):
        """get_sensor_mat at n poses -> uint8[n, h, w, 3] (NavBySceneFamiliarity.py:151-192)."""
        x, y, angle = self._pose_arrays(x, y, angle)
        h, w = self.sensor_shape
        out = np.empty((len(x), h, w, 3), dtype=np.uint8)
        self._check_sense(self._lib.dv_sense(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angle), len(x), N.u8ptr(out)),
                          "dv_sense")
        return out

    def sense_patches(self, x, y, angles):
        """The heading patches of one position, sensed straight into the resident patches."""
        angles = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1)
        self._check_sense(self._lib.dv_sense_patches(self._ctx, float(x), float(y), N.f64ptr(angles), len(angles)),
                          "dv_sense_patches")

    def sense_step(self, x, y, angles, want_scene=True, force_resolve=False):
        """Sense the heading patches at (x, y) and score them: one call for an agent step's device work."""
        angles = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1)
        if len(angles) > N.DV_MAX_HEADINGS:
            return self._wide(lambda flags, res, fam, view, scene: self._lib.dv_sense_step_wide(
                self._ctx, float(x), float(y), N.f64ptr(angles), len(angles), flags, res, fam, view, scene),
                len(angles), want_scene, force_resolve, "dv_sense_step_wide")
        r = N.StepResult()
        scene = np.empty(self.n_views, dtype=np.float64) if want_scene else None
        self._check_sense(self._lib.dv_sense_step(self._ctx, float(x), float(y), N.f64ptr(angles), len(angles),
                                                  N.DV_STEP_FORCE_RESOLVE if force_resolve else 0, ctypes.byref(r),
                                                  N.f64ptr(scene) if want_scene else None), "dv_sense_step")
        return self._result_dict(r, scene)

    def sense_step_into(self, x, y, angle, offsets, out_fam):
        """The agent's step as it runs thousands of times per second: headings (angle + offsets) mod 2 pi, sensed and scored,
        per-heading familiarities written into out_fam; returns the chosen heading's index.  Same call as sense_step(...,
        want_scene=False) -- dv_sense_step -- through ONE result record and ONE angle buffer kept for the engine's lifetime
        (no per-step allocations, views or dictionaries on the host side)."""
        if len(offsets) > N.DV_MAX_HEADINGS:
            # more headings than one library pass holds: the wide step (passes merged in the library, same decision rule)
            res = self.sense_step(x, y, (angle + offsets) % (2 * np.pi), want_scene=False)
            out_fam[:] = res["angle_familiarity"]
            return res["best_idex"]
        if out_fam.shape != (len(offsets),):
            raise ValueError("out_fam has shape %r, expected (%d,)" % (out_fam.shape, len(offsets)))
        st = self._step_state
        if st is None or len(st[0]) != len(offsets):
            res = N.StepResult()
            buf = np.empty(len(offsets), dtype=np.float64)
            st = self._step_state = (buf, N.f64ptr(buf), res, ctypes.byref(res),
                                     np.frombuffer(res, dtype=np.float64, count=len(offsets), offset=N.RESULT_ARRAYS_OFFSET))
        buf, bufp, res, resp, fam = st
        np.add(offsets, angle, out=buf)
        np.mod(buf, 2 * np.pi, out=buf)
        rc = self._lib.dv_sense_step(self._ctx, x, y, bufp, len(buf), 0, resp, None)
        if rc:
            self._check_sense(rc, "dv_sense_step")
        out_fam[:] = fam
        return res.best_heading

    def _agent_args(self, offsets, out_fam):
        st = self._agent_state
        if st is None or st[0] is not offsets or st[1] is not out_fam:
            if not (out_fam.flags.c_contiguous and out_fam.dtype == np.float64 and out_fam.shape == (len(offsets),)):
                raise ValueError("out_fam must be a C-contiguous float64[%d]" % len(offsets))
            off = np.ascontiguousarray(offsets, dtype=np.float64)
            best, nearest, have = ctypes.c_int32(0), ctypes.c_double(0.0), ctypes.c_int32(0)
            st = self._agent_state = (offsets, out_fam, off, N.f64ptr(off), len(off), N.f64ptr(out_fam), best, ctypes.byref(best),
                                      nearest, ctypes.byref(nearest), have, ctypes.byref(have))
        return st

    def agent_step(self, x, y, angle, offsets, out_fam, error_pos, reach):
        """dv_agent_step: one agent step's device work and device-side book-keeping in one call.  The headings (angle + offsets)
        mod 2 pi are sensed at (x, y) and scored, out_fam (float64[A], C-contiguous: the agent's angle_familiarity) is written in
        place; error_pos = (ex, ey) asks for the error metrics of that position (or None), and an outstanding answer comes back.
        Returns (best heading, nearest distance or None)."""
        _, _, _, offp, A, famp, best, bestp, nearest, nearestp, have, havep = self._agent_args(offsets, out_fam)
        if error_pos is None:
            rc = self._lib.dv_agent_step(self._ctx, x, y, angle, offp, A, 0, 0.0, 0.0, 0.0, famp, bestp, nearestp, havep)
        else:
            rc = self._lib.dv_agent_step(self._ctx, x, y, angle, offp, A, 1, error_pos[0], error_pos[1], reach, famp, bestp, nearestp, havep)
        if rc:
            self._check_sense(rc, "dv_agent_step")
        return best.value, (nearest.value if have.value else None)

    def agent_step_begin(self, x, y, angle, offsets, out_fam, error_pos, reach):
        """First half of agent_step (dv_agent_step_begin): collects an outstanding error answer, launches the step, returns at once
        with that answer (or None).  agent_step_end() hands out the step's result -- unless anything else was asked of the engine in
        between, which supersedes the begun step."""
        _, _, _, offp, A, famp, best, bestp, nearest, nearestp, have, havep = self._agent_args(offsets, out_fam)
        if error_pos is None:
            rc = self._lib.dv_agent_step_begin(self._ctx, x, y, angle, offp, A, 0, 0.0, 0.0, 0.0, nearestp, havep)
        else:
            rc = self._lib.dv_agent_step_begin(self._ctx, x, y, angle, offp, A, 1, error_pos[0], error_pos[1], reach, nearestp, havep)
        if rc:
            self._check_sense(rc, "dv_agent_step_begin")
        self._begun = True
        return nearest.value if have.value else None

    def agent_step_end(self):
        """Second half: waits for the begun step, writes its per-heading maxima into the out_fam given to agent_step_begin and
        returns the best heading; None when the begun step was superseded (the caller takes the step again)."""
        if not self._begun:
            return None
        self._begun = False
        st = self._agent_state
        rc = self._lib.dv_agent_step_end(self._ctx_raw, st[5], st[7])
        if rc:
            self._check_sense(rc, "dv_agent_step_end")
        return st[6].value

    def agent_step_end_begin(self, cand, bounds, do_error, reach):
        """agent_step_end and the next agent_step_begin in one call (dv_agent_step_end_begin): cand = (angles[A], xs[A], ys[A]) of every
        candidate heading (float64, C-contiguous), bounds = float64[3] of the reference's bounds test.  Returns None when the begun step
        was superseded, else (best heading, whether the next step was begun, an outstanding error answer or None)."""
        if not self._begun:
            return None
        self._begun = False
        st = self._agent_state
        begun = ctypes.c_int32(0)
        rc = self._lib.dv_agent_step_end_begin(self._ctx_raw, st[5], st[7], N.f64ptr(cand[1]), N.f64ptr(cand[2]), N.f64ptr(cand[0]), st[3], st[4],
                                               N.f64ptr(bounds), 1 if do_error else 0, reach, ctypes.byref(begun), st[9], st[11])
        if rc:
            self._check_sense(rc, "dv_agent_step_end_begin")
        self._begun = bool(begun.value)
        return st[6].value, self._begun, (st[8].value if st[10].value else None)

    def sense_step_batch(self, x, y, angles, force_resolve=False, chem_weights=None):
        """Ensemble step on the device: agent i at (x[i], y[i]) looking along angles[i][0..A) -> BatchResults (a sequence of result dicts).
        chem_weights[N] (optional): agent i is scored under chem_weights[i] (the library's layout must serve it: set_weight_range)."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        angles = np.ascontiguousarray(angles, dtype=np.float64)
        if angles.ndim != 2 or len(x) != len(y) or angles.shape[0] != len(x):
            raise ValueError("x[N], y[N] and angles[N, A] expected")
        n, A = angles.shape
        w = agent_weights(chem_weights, n)
        res = (N.StepResult * n)()
        flags = N.DV_STEP_FORCE_RESOLVE if force_resolve else 0
        if w is None:
            self._check_sense(self._lib.dv_sense_step_batch(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angles), n, A, flags, res),
                              "dv_sense_step_batch")
        else:
            self._check_sense(self._lib.dv_sense_step_batch_weighted(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angles), n, A,
                                                                     N.f64ptr(w), flags, res), "dv_sense_step_batch_weighted")
        return BatchResults(res, n, A)

    def sense_step_batch_scene(self, x, y, angles, force_resolve=False, chem_weights=None):
        """sense_step_batch that also keeps every agent's per-view minimum (dv_sense_step_batch_scene): the same records, and
        BatchResults.scene_familiarity = float64[N, F], row i the minimum over agent i's OWN headings under its own weight -- what
        sense_step(x[i], y[i], angles[i], want_scene=True) returns, bit for bit; a row of +inf for an agent whose footprint left
        the landscape (flags & DV_RES_SENSE_ERROR).  The passes go through HBM one after the other: a call for reading the minimum
        of a step already taken (NavEnsemble.scene_familiarity), not for stepping."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        angles = np.ascontiguousarray(angles, dtype=np.float64)
        if angles.ndim != 2 or len(x) != len(y) or angles.shape[0] != len(x):
            raise ValueError("x[N], y[N] and angles[N, A] expected")
        n, A = angles.shape
        w = agent_weights(chem_weights, n)
        res = (N.StepResult * n)()
        scene = np.empty((n, int(self.n_views)), dtype=np.float64)
        self._check_sense(self._lib.dv_sense_step_batch_scene(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angles), n, A,
                                                              None if w is None else N.f64ptr(w),
                                                              N.DV_STEP_FORCE_RESOLVE if force_resolve else 0, res, N.f64ptr(scene)),
                          "dv_sense_step_batch_scene")
        return BatchResults(res, n, A, scene)

    def set_library_from_poses(self, x, y, angle, chem_weight=0.0, first_view=0, want_views=True):
        """train_from_path on the device: sense the poses and ingest them as the library; returns familiar_scenes."""
        x, y, angle = self._pose_arrays(x, y, angle)
        h, w = self.sensor_shape
        views = np.empty((len(x), h, w, 3), dtype=np.uint8) if want_views else None
        self._check_sense(self._lib.dv_set_library_from_poses(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angle), len(x),
                                                              float(chem_weight), int(first_view),
                                                              N.u8ptr(views) if want_views else None),
                          "dv_set_library_from_poses")
        self.n_views, self.shape = len(x), (h, w)
        return views

    # -- scoring --------------------------------------------------------------------------------
    def _patch_shape_ok(self, p, lead):
        h, w = self.shape if self.shape else (None, None)
        want = lead + (h, w, 3)
        if self.shape is None:
            raise N.EngineError("no library set")
        if tuple(p.shape) != want:
            raise ValueError("patch array has shape %r, expected %r" % (tuple(p.shape), want))

    def score(self, scene, fambuf):
        """util.pyx:14-20 func(scene, fambuf): writes float64[F] in place."""
        scene = N.as_u8(scene, "scene")
        self._patch_shape_ok(scene, ())
        if not (isinstance(fambuf, np.ndarray) and fambuf.dtype == np.float64):
            raise ValueError("Buffer dtype mismatch for fambuf, expected 'double'")
        if fambuf.shape != (self.n_views,):
            raise ValueError("fambuf has shape %r, expected (%d,)" % (fambuf.shape, self.n_views))
        if fambuf.flags.c_contiguous:
            self._check(self._lib.dv_score(self._ctx, N.u8ptr(scene), N.f64ptr(fambuf)), "dv_score")
        else:
            tmp = np.empty(self.n_views, dtype=np.float64)
            self._check(self._lib.dv_score(self._ctx, N.u8ptr(scene), N.f64ptr(tmp)), "dv_score")
            fambuf[:] = tmp
        return fambuf

    @staticmethod
    def _result_dict(r, scene):
        A = r.n_headings
        # views of the record's four per-heading arrays ([4][64] 8-byte values after the header); every step
        # has its own record, which the views keep alive
        M = N.DV_MAX_HEADINGS
        f64 = np.frombuffer(r, dtype=np.float64, count=4 * M, offset=N.RESULT_ARRAYS_OFFSET)
        i64 = f64.view(np.int64)
        return dict(best_idex=r.best_heading, best_view=r.best_view, step_familiarity=r.best_fam,
                    angle_familiarity=f64[:A], angle_view=i64[M:M + A],
                    exact_familiarity=f64[2 * M:2 * M + A], exact_view=i64[3 * M:3 * M + A],
                    approx_max=r.approx_max, delta=r.delta, n_candidates=r.n_candidates,
                    flags=r.flags, scene_familiarity=scene)

    def step(self, patches, want_scene=True, force_resolve=False):
        """Heading loop of step_forward (:283-316) on patches uint8[A,h,w,3]."""
        patches = N.as_u8(patches, "patches")
        if patches.ndim != 4:
            raise ValueError("patches must be uint8[A,h,w,3]")
        self._patch_shape_ok(patches, (patches.shape[0],))
        if patches.shape[0] > N.DV_MAX_HEADINGS:
            return self._wide(lambda flags, res, fam, view, scene: self._lib.dv_step_wide(
                self._ctx, N.u8ptr(patches), patches.shape[0], flags, res, fam, view, scene),
                patches.shape[0], want_scene, force_resolve, "dv_step_wide")
        r = N.StepResult()
        scene = np.empty(self.n_views, dtype=np.float64) if want_scene else None
        self._check(self._lib.dv_step(self._ctx, N.u8ptr(patches), patches.shape[0],
                                      N.DV_STEP_FORCE_RESOLVE if force_resolve else 0, ctypes.byref(r),
                                      N.f64ptr(scene) if want_scene else None), "dv_step")
        return self._result_dict(r, scene)

    def _wide(self, call, A, want_scene, force_resolve, what):
        """A step of more than DV_MAX_HEADINGS headings (the reference takes any n_test_angles, NavBySceneFamiliarity.py:62,289):
        ceil(A / 64) library passes merged inside the library; same keys as a single-pass step's result."""
        res = N.WideResult()
        fam = np.empty(A, dtype=np.float64)
        view = np.empty(A, dtype=np.int64)
        scene = np.empty(self.n_views, dtype=np.float64) if want_scene else None
        self._check_sense(call(N.DV_STEP_FORCE_RESOLVE if force_resolve else 0, ctypes.byref(res), N.f64ptr(fam), N.i64ptr(view),
                               N.f64ptr(scene) if want_scene else None), what)
        return dict(best_idex=res.best_heading, best_view=res.best_view, step_familiarity=res.best_fam, angle_familiarity=fam,
                    angle_view=view, flags=res.flags, n_passes=res.n_passes, n_contending=res.n_contending,
                    scene_familiarity=scene)

    def step_batch(self, patches, force_resolve=False, chem_weights=None):
        """Ensemble step: patches uint8[N, A, h, w, 3] -> BatchResults, a sequence of N result dicts (one library pass per 64/A agents).
        chem_weights[N] (optional): agent i is scored under chem_weights[i] (the library's layout must serve it: set_weight_range)."""
        patches = N.as_u8(patches, "patches")
        if patches.ndim != 5:
            raise ValueError("patches must be uint8[N,A,h,w,3]")
        n, A = patches.shape[0], patches.shape[1]
        self._patch_shape_ok(patches, (n, A))
        w = agent_weights(chem_weights, n)
        res = (N.StepResult * n)()
        flags = N.DV_STEP_FORCE_RESOLVE if force_resolve else 0
        if w is None:
            self._check(self._lib.dv_step_batch(self._ctx, N.u8ptr(patches), n, A, flags, res), "dv_step_batch")
        else:
            self._check(self._lib.dv_step_batch_weighted(self._ctx, N.u8ptr(patches), n, A, N.f64ptr(w), flags, res),
                        "dv_step_batch_weighted")
        return BatchResults(res, n, A)

    def step_batch_scene(self, patches, force_resolve=False, chem_weights=None):
        """step_batch that also keeps every agent's per-view minimum (dv_step_batch_scene): BatchResults.scene_familiarity =
        float64[N, F], row i what step(patches[i], want_scene=True) returns under agent i's weight."""
        patches = N.as_u8(patches, "patches")
        if patches.ndim != 5:
            raise ValueError("patches must be uint8[N,A,h,w,3]")
        n, A = patches.shape[0], patches.shape[1]
        self._patch_shape_ok(patches, (n, A))
        w = agent_weights(chem_weights, n)
        res = (N.StepResult * n)()
        scene = np.empty((n, int(self.n_views)), dtype=np.float64)
        self._check(self._lib.dv_step_batch_scene(self._ctx, N.u8ptr(patches), n, A, None if w is None else N.f64ptr(w),
                                                  N.DV_STEP_FORCE_RESOLVE if force_resolve else 0, res, N.f64ptr(scene)),
                    "dv_step_batch_scene")
        return BatchResults(res, n, A, scene)

    # -- ssd_f32 metric --------------------------------------------------------------------------
    @staticmethod
    def _f32(a, what):
        a = np.ascontiguousarray(a)
        if a.dtype != np.float32:
            raise ValueError("Buffer dtype mismatch for %s, expected 'float' but got '%s'" % (what, a.dtype))
        return a

    def set_library_f32(self, views, first_view=0):
        """views: float32[F,h,w]; scores are sums of squared differences (navsim/util.pyx:171-184)."""
        views = self._f32(views, "views")
        if views.ndim != 3:
            raise ValueError("views must be float32[F,h,w], got shape %r" % (views.shape,))
        F, h, w = views.shape
        fp = views.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        self._check(self._lib.dv_set_library_f32(self._ctx, fp, F, h, w, int(first_view)), "dv_set_library_f32")
        self.n_views, self.shape = F, (h, w)

    def generate_library_f32(self, seed, n_views, h, w, first_view=0):
        """Same values as synth.synth_views_f32(seed, n_views, h, w, first_view), generated in HBM."""
        self._check(self._lib.dv_generate_library_f32(self._ctx, int(seed), int(n_views), int(h), int(w), int(first_view)),
                    "dv_generate_library_f32")
        self.n_views, self.shape = int(n_views), (int(h), int(w))

    def score_f32(self, patch, ssdbuf=None):
        patch = self._f32(patch, "patch")
        if tuple(patch.shape) != self.shape:
            raise ValueError("patch has shape %r, expected %r" % (patch.shape, self.shape))
        if ssdbuf is None:
            ssdbuf = np.empty(self.n_views, dtype=np.float64)
        self._check(self._lib.dv_score_f32(self._ctx, patch.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                           N.f64ptr(ssdbuf)), "dv_score_f32")
        return ssdbuf

    def step_f32(self, patches, want_scene=False, force_resolve=False):
        """Least-SSD heading over float32 patches [A,h,w]: dict with angle_ssd, best_idex, best_view, step_ssd."""
        patches = self._f32(patches, "patches")
        if patches.ndim != 3 or tuple(patches.shape[1:]) != self.shape:
            raise ValueError("patches must be float32[A,%d,%d]" % self.shape)
        r = N.StepResult()
        scene = np.empty(self.n_views, dtype=np.float64) if want_scene else None
        self._check(self._lib.dv_step_f32(self._ctx, patches.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                          patches.shape[0], N.DV_STEP_FORCE_RESOLVE if force_resolve else 0,
                                          ctypes.byref(r), N.f64ptr(scene) if want_scene else None), "dv_step_f32")
        d = self._result_dict(r, scene)
        return dict(best_idex=d["best_idex"], best_view=d["best_view"], step_ssd=d["step_familiarity"],
                    angle_ssd=d["angle_familiarity"], angle_view=d["angle_view"], n_candidates=d["n_candidates"],
                    flags=d["flags"], scene_ssd=scene)

    # -- ssd_u8 metric: exact SSD of uint8 views on the int8 matrix cores -------------------------------
    def set_library_u8(self, views, first_view=0):
        """views: uint8[F,h,w]; scores are the exact integer sums of squared differences (navsim/util.pyx:171-184 on uint8 data)."""
        views = N.as_u8(views, "views")
        if views.ndim != 3:
            raise ValueError("views must be uint8[F,h,w], got shape %r" % (views.shape,))
        F, h, w = views.shape
        self._check(self._lib.dv_set_library_u8(self._ctx, N.u8ptr(views), F, h, w, int(first_view)), "dv_set_library_u8")
        self.n_views, self.shape = F, (h, w)

    def set_library_u8_from_poses(self, x, y, angle, channel=2, first_view=0, want_views=True):
        """train_from_path for the ssd_u8 plug-in on the device: sense the poses, ingest their `channel` bytes as the library;
        returns familiar_scenes (uint8[n,h,w,3]) when want_views."""
        x, y, angle = self._pose_arrays(x, y, angle)
        h, w = self.sensor_shape
        views = np.empty((len(x), h, w, 3), dtype=np.uint8) if want_views else None
        self._check_sense(self._lib.dv_set_library_u8_from_poses(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angle), len(x),
                                                                 int(channel), int(first_view),
                                                                 N.u8ptr(views) if want_views else None),
                          "dv_set_library_u8_from_poses")
        self.n_views, self.shape = len(x), (h, w)
        return views

    def sense_step_u8(self, x, y, angles, channel=2, want_scene=False):
        """dv_sense_step for an ssd_u8 library: the heading patches sensed at (x, y), their `channel` bytes scored on the int8
        matrix cores, the least-SSD heading decided on the device.  Result as step_u8's."""
        angles = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1)
        r = N.StepResult()
        scene = np.empty(self.n_views, dtype=np.float64) if want_scene else None
        self._check_sense(self._lib.dv_sense_step_u8(self._ctx, float(x), float(y), N.f64ptr(angles), len(angles), int(channel), 0,
                                                     ctypes.byref(r), N.f64ptr(scene) if want_scene else None), "dv_sense_step_u8")
        d = self._result_dict(r, scene)
        return dict(best_idex=d["best_idex"], best_view=d["best_view"], step_ssd=d["step_familiarity"],
                    angle_ssd=d["angle_familiarity"], angle_view=d["angle_view"], n_candidates=d["n_candidates"],
                    flags=d["flags"], scene_ssd=scene)

    def score_u8(self, patch, ssdbuf=None):
        patch = N.as_u8(patch, "patch")
        if tuple(patch.shape) != self.shape:
            raise ValueError("patch has shape %r, expected %r" % (patch.shape, self.shape))
        if ssdbuf is None:
            ssdbuf = np.empty(self.n_views, dtype=np.float64)
        self._check(self._lib.dv_score_u8(self._ctx, N.u8ptr(patch), N.f64ptr(ssdbuf)), "dv_score_u8")
        return ssdbuf

    def step_u8(self, patches, want_scene=False):
        """Least-SSD heading over uint8 patches [A,h,w]: dict with angle_ssd, best_idex, best_view, step_ssd (exact integers)."""
        patches = N.as_u8(patches, "patches")
        if patches.ndim != 3 or tuple(patches.shape[1:]) != self.shape:
            raise ValueError("patches must be uint8[A,%d,%d]" % self.shape)
        r = N.StepResult()
        scene = np.empty(self.n_views, dtype=np.float64) if want_scene else None
        self._check(self._lib.dv_step_u8(self._ctx, N.u8ptr(patches), patches.shape[0], 0, ctypes.byref(r),
                                         N.f64ptr(scene) if want_scene else None), "dv_step_u8")
        d = self._result_dict(r, scene)
        return dict(best_idex=d["best_idex"], best_view=d["best_view"], step_ssd=d["step_familiarity"],
                    angle_ssd=d["angle_familiarity"], angle_view=d["angle_view"], n_candidates=d["n_candidates"],
                    flags=d["flags"], scene_ssd=scene)

    def resolve(self):
        r = N.StepResult()
        self._check(self._lib.dv_resolve(self._ctx, ctypes.byref(r)), "dv_resolve")
        return self._result_dict(r, None)

    # -- resident form --------------------------------------------------------------------------
    def upload_patches(self, patches):
        patches = N.as_u8(patches, "patches")
        self._patch_shape_ok(patches, (patches.shape[0],))
        self._check(self._lib.dv_upload_patches(self._ctx, N.u8ptr(patches), patches.shape[0]), "dv_upload_patches")

    def generate_patches(self, seed, n_headings):
        self._check(self._lib.dv_generate_patches(self._ctx, int(seed), int(n_headings)), "dv_generate_patches")

    def step_enqueue(self, want_scene=False, force_resolve=False):
        flags = (N.DV_STEP_WANT_SCENE if want_scene else 0) | (N.DV_STEP_FORCE_RESOLVE if force_resolve else 0)
        self._check(self._lib.dv_step_enqueue(self._ctx, flags), "dv_step_enqueue")

    def step_wait(self, want_scene=False):
        r = N.StepResult()
        scene = np.empty(self.n_views, dtype=np.float64) if want_scene else None
        self._check_sense(self._lib.dv_step_wait(self._ctx, ctypes.byref(r), N.f64ptr(scene) if want_scene else None),
                          "dv_step_wait")
        return self._result_dict(r, scene)

    def step_record(self):
        """(device pointer, n_doubles) of the packed record of the last enqueued step (sharded exchange)."""
        ptr = ctypes.c_void_p()
        n = ctypes.c_int(0)
        self._check(self._lib.dv_step_record(self._ctx, ctypes.byref(ptr), ctypes.byref(n)), "dv_step_record")
        return int(ptr.value), int(n.value)

    def resolve_enqueue(self):
        self._check(self._lib.dv_resolve_enqueue(self._ctx), "dv_resolve_enqueue")

    def step_keys(self, rank, world, signed_order=False):
        """Enqueue the packing of the last step's keys for the all-reduce(max) exchange; (device pointer, n_words)."""
        ptr = ctypes.c_void_p()
        n = ctypes.c_int(0)
        self._check(self._lib.dv_step_keys(self._ctx, int(rank), int(world), 1 if signed_order else 0, ctypes.byref(ptr),
                                           ctypes.byref(n)), "dv_step_keys")
        return int(ptr.value), int(n.value)

    # -- measurement ----------------------------------------------------------------------------
    def timer_start(self):
        self._check(self._lib.dv_timer_start(self._ctx), "dv_timer_start")

    def timer_stop(self):
        ms = ctypes.c_float(0)
        self._check(self._lib.dv_timer_stop(self._ctx, ctypes.byref(ms)), "dv_timer_stop")
        return float(ms.value)

    def profile_kernel(self, enable, every=1):
        """Bracket every `every`-th scoring-kernel launch with hipEvents (an event pair costs stream time)."""
        self._check(self._lib.dv_profile_kernel(self._ctx, max(1, int(every)) if enable else 0), "dv_profile_kernel")

    def profile_read(self):
        tot = ctypes.c_double(0)
        n = ctypes.c_int64(0)
        self._check(self._lib.dv_profile_read(self._ctx, ctypes.byref(tot), ctypes.byref(n)), "dv_profile_read")
        return float(tot.value), int(n.value)

    def publish(self, device_ptr, n_doubles):
        """Enqueue the hand-over of a device buffer of doubles to the host (no stream wait), see dv_publish."""
        self._check(self._lib.dv_publish(self._ctx, ctypes.c_void_p(int(device_ptr)), int(n_doubles)), "dv_publish")

    def publish_wait(self, out):
        """Poll for the last publish and copy it into `out` (float64, C-contiguous)."""
        self._check(self._lib.dv_publish_wait(self._ctx, N.f64ptr(out), out.size), "dv_publish_wait")
        return out

    def set_mailbox(self, address, n_bytes, rank, world):
        """Attach (address = 0: detach) the node's shared host segment of the mailbox exchange, see dv_set_mailbox."""
        self._check(self._lib.dv_set_mailbox(self._ctx, ctypes.c_void_p(int(address) or None), int(n_bytes), int(rank), int(world)),
                    "dv_set_mailbox")

    def mailbox_post(self, slot, seq):
        self._check(self._lib.dv_mailbox_post(self._ctx, int(slot), int(seq)), "dv_mailbox_post")

    def mailbox_wait(self, slot, seq, rank_mask, records, timeout_ms=20000):
        self._check(self._lib.dv_mailbox_wait(self._ctx, int(slot), int(seq), int(rank_mask), N.f64ptr(records),
                                              records.shape[1], int(timeout_ms)), "dv_mailbox_wait")
        return records

    def workgroup_shape(self, n_headings):
        """Shape of the scoring kernel in use for this many headings (0: not timed yet / not applicable)."""
        v = ctypes.c_int(0)
        self._check(self._lib.dv_workgroup_shape(self._ctx, int(n_headings), ctypes.byref(v)), "dv_workgroup_shape")
        return int(v.value)

    # -- error / coverage metrics on the device (NavBySceneFamiliarity.py:252-276) ----------------
    def set_training_path(self, points):
        """points: float64[n, 2] (x, y), or None to detach.  Clears the coverage marks."""
        self._path_slot_count = None                             # (the library drops the slots with the path)
        if points is None:
            self._check(self._lib.dv_set_training_path(self._ctx, None, 0), "dv_set_training_path")
            return
        pts = np.ascontiguousarray(points, dtype=np.float64)
        assert pts.ndim == 2 and pts.shape[1] == 2
        self._check(self._lib.dv_set_training_path(self._ctx, N.f64ptr(pts), pts.shape[0]), "dv_set_training_path")

    def path_error_enqueue(self, x, y, reach):
        rc = self._lib.dv_path_error_enqueue(self._ctx, x, y, reach)
        if rc:
            self._check(rc, "dv_path_error_enqueue")

    def path_error_wait(self):
        out = self._err_out
        rc = self._lib.dv_path_error_wait(self._ctx, self._err_out_ref)
        if rc:
            self._check(rc, "dv_path_error_wait")
        return out.value

    def path_coverage(self, n):
        out = np.empty(int(n), dtype=np.uint8)
        self._check(self._lib.dv_path_coverage(self._ctx, N.u8ptr(out), int(n)), "dv_path_coverage")
        return out.astype(bool)

    def patches_on_level(self):
        """True when the resident patches allowed the fp4 form of the matrix-core kernel (dv_patches_on_level)."""
        rc = self._lib.dv_patches_on_level(self._ctx)
        if rc < 0:
            self._check(rc, "dv_patches_on_level")
        return bool(rc)

    def scoring_form(self):
        """Form of the last integer scoring pass (dv_scoring_form): matrix cores / fp4 coefficients / fused finishing / value rows
        read as 3-bit codes / those in the registers of all eight waves of a workgroup / the name of the kernel body the host
        launched for a matrix-core pass (`body`, None otherwise: include/dejavu.h, DV_FORM_BODY_NAMES)."""
        rc = self._lib.dv_scoring_form(self._ctx)
        if rc < 0:
            self._check(rc, "dv_scoring_form")
        body = (rc >> N.DV_FORM_BODY_SHIFT) & ((1 << N.DV_FORM_BODY_BITS) - 1)
        return dict(matrix_cores=bool(rc & 1), fp4=bool(rc & 2), fused_finish=bool(rc & 4), codes=bool(rc & 8), consumers8=bool(rc & 16),
                    body=N.DV_FORM_BODY_NAMES[body - 1] if body else None)

    def path_reset(self):
        self._check(self._lib.dv_path_reset(self._ctx), "dv_path_reset")

    # update_error for the agents of an ensemble: a coverage array per agent (slot) on the device
    def path_slots(self, n_slots):
        self._check(self._lib.dv_path_slots(self._ctx, int(n_slots)), "dv_path_slots")
        self._path_slot_count = int(n_slots) or None

    def path_error_batch(self, slots, xs, ys, reach):
        """nearest[i] of agent slots[i] at (xs[i], ys[i]) (NavBySceneFamiliarity.py:252-276 for all of them at once); its marks updated."""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        xs = np.ascontiguousarray(xs, dtype=np.float64)
        ys = np.ascontiguousarray(ys, dtype=np.float64)
        out = np.empty(len(slots), dtype=np.float64)
        self._check(self._lib.dv_path_error_batch(self._ctx, slots.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), N.f64ptr(xs), N.f64ptr(ys),
                                                  len(slots), float(reach), N.f64ptr(out)), "dv_path_error_batch")
        return out

    def path_coverage_slot(self, slot, n):
        out = np.empty(int(n), dtype=np.uint8)
        self._check(self._lib.dv_path_coverage_slot(self._ctx, int(slot), N.u8ptr(out), int(n)), "dv_path_coverage_slot")
        return out.astype(bool)

    def path_reset_slot(self, slot=-1):
        self._check(self._lib.dv_path_reset_slot(self._ctx, int(slot)), "dv_path_reset_slot")

    # -- the same metrics against several routes: a path per route, a coverage array per slot (include/dejavu.h: dv_path_routes_*) ----
    _route_first = None          # int64[R + 1]: the bounds of the routes set (path_routes_set); None: no routes
    _route_of_slot = None        # int32[n_slots]: the route of every slot (path_routes_slots); None: no slots

    @staticmethod
    def _index_table(table, what, hi, of, n=None, per=None):
        """`table` as int32[n] (n = None: of any length) with every entry in [0, hi), or ValueError naming `what`: checked before any
        library call.  `of` names hi, `per` what an entry stands for.  hi = None: there is nothing to index yet, and the library
        answers DV_ERR_STATE."""
        arr = np.asarray(table)
        if arr.shape == (0,):
            arr = arr.astype(np.int32)                           # (an empty list has no dtype to speak of)
        if arr.dtype.kind not in "iu":
            raise ValueError("%s must hold integers%s, got dtype %s" % (what, " (a %s per entry)" % per if per else "", arr.dtype))
        if n is None and arr.ndim != 1:
            raise ValueError("%s must have one dimension, got shape %r" % (what, arr.shape))
        if n is not None and arr.shape != (n,):
            raise ValueError("%s must have shape (%d,), got %r" % (what, n, arr.shape))
        if hi is not None and len(arr) and (arr.min() < 0 or arr.max() >= hi):
            bad = np.flatnonzero((arr < 0) | (arr >= hi))
            raise ValueError("%s[%d] = %d outside [0, %s = %d)" % (what, bad[0], arr[bad[0]], of, hi))
        return np.ascontiguousarray(arr, dtype=np.int32)

    def path_routes_set(self, routes, first=None):
        """routes: a sequence of R arrays float64[n_r, 2] (n_r >= 1) -- or, with `first` (integers [R + 1], rising from 0), all routes'
        points in one float64[first[-1], 2].  None detaches.  Drops the slots and their marks."""
        if routes is None:
            self._check(self._lib.dv_path_routes_set(self._ctx, None, None, 0), "dv_path_routes_set")
            self._route_first = self._route_of_slot = None
            return
        if first is None:
            parts = []
            for r, route in enumerate(routes):
                part = np.asarray(route)
                if part.dtype != np.float64 or part.ndim != 2 or part.shape[1] != 2 or len(part) < 1:
                    raise ValueError("routes[%d] must be float64[n, 2] with n >= 1, got %s%r" % (r, part.dtype, part.shape))
                parts.append(part)
            if not parts:
                raise ValueError("routes must hold at least one route")
            first = np.cumsum([0] + [len(p) for p in parts])
            pts = np.ascontiguousarray(np.concatenate(parts))
        else:
            pts = np.asarray(routes)
            if pts.dtype != np.float64 or pts.ndim != 2 or pts.shape[1] != 2:
                raise ValueError("the routes' points must be float64[n, 2], got %s%r" % (pts.dtype, pts.shape))
            pts = np.ascontiguousarray(pts)
        bounds = np.asarray(first)
        if bounds.dtype.kind not in "iu" or bounds.ndim != 1 or len(bounds) < 2:
            raise ValueError("first must hold integers [R + 1] with R >= 1, got %s%r" % (bounds.dtype, bounds.shape))
        bounds = np.ascontiguousarray(bounds, dtype=np.int64)
        if bounds[0] != 0:
            raise ValueError("first[0] must be 0, got %d" % bounds[0])
        if (np.diff(bounds) < 1).any():
            r = int(np.flatnonzero(np.diff(bounds) < 1)[0])
            raise ValueError("first must rise: first[%d] = %d after first[%d] = %d (a route has at least one point)"
                             % (r + 1, bounds[r + 1], r, bounds[r]))
        if bounds[-1] != len(pts):
            raise ValueError("first[-1] = %d, but there are %d points" % (bounds[-1], len(pts)))
        self._check(self._lib.dv_path_routes_set(self._ctx, N.f64ptr(pts), N.i64ptr(bounds), len(bounds) - 1), "dv_path_routes_set")
        self._route_first, self._route_of_slot = bounds, None

    def path_routes_slots(self, route_of_slot):
        """Slot j gets coverage marks of its own for route route_of_slot[j], cleared (what the slots held is dropped).  An empty table,
        or None, frees them."""
        table = self._index_table([] if route_of_slot is None else route_of_slot, "route_of_slot",
                                 None if self._route_first is None else len(self._route_first) - 1, "n_routes")
        self._check(self._lib.dv_path_routes_slots(self._ctx, table.ctypes.data_as(N._i32p), len(table)), "dv_path_routes_slots")
        self._route_of_slot = table if len(table) else None

    def path_routes_error(self, slots, xs, ys, reach):
        """update_error (NavBySceneFamiliarity.py:252-276) for n entries at once, each against ITS slot's route and with its OWN reach:
        float64[n] of the distances to the nearest point of each entry's route; the slots' marks updated."""
        slots = self._index_table(slots, "slots", None if self._route_of_slot is None else len(self._route_of_slot), "n_slots")
        n = len(slots)
        vals = []
        for name, v in (("xs", xs), ("ys", ys), ("reach", reach)):
            arr = np.asarray(v)
            if arr.shape == (0,):
                arr = arr.astype(np.float64)
            if arr.dtype != np.float64:
                raise ValueError("%s must be float64, got dtype %s" % (name, arr.dtype))
            if arr.shape != (n,):
                raise ValueError("%s must have shape (%d,), one per entry of slots, got %r" % (name, n, arr.shape))
            vals.append(np.ascontiguousarray(arr))
        out = np.empty(n, dtype=np.float64)
        self._check(self._lib.dv_path_routes_error(self._ctx, slots.ctypes.data_as(N._i32p), N.f64ptr(vals[0]), N.f64ptr(vals[1]),
                                                   N.f64ptr(vals[2]), n, N.f64ptr(out)), "dv_path_routes_error")
        return out

    def _route_slot(self, slot):
        n_slots = None if self._route_of_slot is None else len(self._route_of_slot)
        if isinstance(slot, bool) or not isinstance(slot, (int, np.integer)) or slot < 0 or (n_slots is not None and slot >= n_slots):
            raise ValueError("slot must be an integer in [0, n_slots%s), got %r" % ("" if n_slots is None else " = %d" % n_slots, slot))
        return int(slot)

    def path_routes_coverage(self, slot, n):
        """bool[n]: the marks of `slot`; n must be the length of the slot's route."""
        slot = self._route_slot(slot)
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
            raise ValueError("n must be the length of slot %d's route, got %r" % (slot, n))
        if self._route_of_slot is not None:
            r = self._route_of_slot[slot]
            length = int(self._route_first[r + 1] - self._route_first[r])
            if n != length:
                raise ValueError("n must be %d, the length of slot %d's route, got %r" % (length, slot, n))
        out = np.empty(int(n), dtype=np.uint8)
        self._check(self._lib.dv_path_routes_coverage(self._ctx, slot, N.u8ptr(out), int(n)), "dv_path_routes_coverage")
        return out.astype(bool)

    def path_routes_reset(self, slot=-1):
        """Clears the marks of one slot, or of all (slot < 0)."""
        if isinstance(slot, bool) or not isinstance(slot, (int, np.integer)):
            raise ValueError("slot must be an integer, got %r" % (slot,))
        slot = self._route_slot(slot) if slot >= 0 else -1
        self._check(self._lib.dv_path_routes_reset(self._ctx, slot), "dv_path_routes_reset")

    def path_routes_info(self):
        """dict(n_routes, n_slots, n_points), as the library counts them."""
        nr, ns, npts = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
        self._check(self._lib.dv_path_routes_info(self._ctx, ctypes.byref(nr), ctypes.byref(ns), ctypes.byref(npts)), "dv_path_routes_info")
        return dict(n_routes=nr.value, n_slots=ns.value, n_points=npts.value)

    # -- the coverage statistics of a result row, from the marks on the device (include/dejavu.h: dv_marks_*) ---------------------------
    _path_slot_count = None      # the slots of the one training path (path_slots); None: none made through this engine

    @staticmethod
    def _marks_window(window, what="window"):
        if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or window < 0:
            raise ValueError("%s must be an integer >= 0, got %r" % (what, window))
        return int(window)

    @staticmethod
    def _marks_windows(windows, n):
        arr = np.asarray(windows)
        if arr.shape == (0,):
            arr = arr.astype(np.int64)
        if arr.dtype.kind not in "iu":
            raise ValueError("windows must hold integers, got dtype %s" % arr.dtype)
        if arr.shape != (n,):
            raise ValueError("windows must have shape (%d,), one per entry of slots, got %r" % (n, arr.shape))
        if n and arr.min() < 0:
            bad = int(np.flatnonzero(arr < 0)[0])
            raise ValueError("windows[%d] = %d < 0" % (bad, arr[bad]))
        return np.ascontiguousarray(arr, dtype=np.int64)

    def marks_summary(self, window):
        """int64[3] = (covered, furthest, captures) of the agent's marks (those path_coverage copies out) under `window` marks:
        the set marks; the largest p + 1 such that the `window` marks ending at p are all set (0 without one); the runs of exactly
        `window` set marks behind a clear mark.  Over n marks they are percent_recapitulated * n, percent_recapitulated_forgiving * n
        and n_captures of the reference (NavBySceneFamiliarity.py:212-249)."""
        window = self._marks_window(window)
        out = np.empty(3, dtype=np.int64)
        self._check(self._lib.dv_marks_summary(self._ctx, window, N.i64ptr(out)), "dv_marks_summary")
        return out

    def _marks_summary_many(self, symbol, slots, windows, n_slots, made_by):
        if n_slots is None:
            raise ValueError("no slots set (%s)" % made_by)
        slots = self._index_table(slots, "slots", n_slots, "n_slots")
        n = len(slots)
        windows = self._marks_windows(windows, n)
        out = np.empty((n, 3), dtype=np.int64)
        self._check(getattr(self._lib, symbol)(self._ctx, slots.ctypes.data_as(N._i32p), N.i64ptr(windows), n, N.i64ptr(out)), symbol)
        return out

    def marks_summary_slots(self, slots, windows):
        """marks_summary for n entries at once over the slots of path_slots: int64[n, 3], entry i slot slots[i] under windows[i]."""
        return self._marks_summary_many("dv_marks_summary_slots", slots, windows, self._path_slot_count, "path_slots")

    def marks_summary_routes(self, slots, windows):
        """marks_summary for n entries at once over the slots of path_routes_slots, each as long as its own route: int64[n, 3]."""
        return self._marks_summary_many("dv_marks_summary_routes", slots, windows,
                                        None if self._route_of_slot is None else len(self._route_of_slot), "path_routes_slots")

    def stream_read_gbps(self, n_bytes=1 << 30, iters=10):
        g = ctypes.c_double(0)
        self._check(self._lib.dv_stream_read_gbps(self._ctx, int(n_bytes), int(iters), ctypes.byref(g)),
                    "dv_stream_read_gbps")
        return float(g.value)

    # -- the one-value models (Infomax, mushroom body): one implementation per operation, the model's symbols from _ONE_VALUE ----
    @staticmethod
    def _model_planes(shape, planes, what):
        """`planes` as uint8[n,h,w] of a model begun with shape (h, w); one uint8[h,w] counts as n = 1."""
        planes = N.as_u8(planes, what)
        if planes.ndim == 2:
            planes = planes[None]
        if shape is None:
            return planes if planes.ndim == 3 else planes.reshape(1, 1, -1)      # (no model: the library answers DV_ERR_STATE)
        if planes.ndim != 3 or tuple(planes.shape[1:]) != shape:
            raise ValueError("%s must be uint8[n,%d,%d], got shape %r" % ((what,) + shape + (planes.shape,)))
        return planes

    def _ov_planes(self, metric, planes):
        return self._model_planes(getattr(self, _ONE_VALUE[metric][2], None), planes, "planes")

    @staticmethod
    def _member_poses(x, y, angles):
        """An ensemble's poses as float64 x[N], y[N] and angles[N, A]."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        angles = np.ascontiguousarray(angles, dtype=np.float64)
        if angles.ndim != 2 or len(x) != len(y) or angles.shape[0] != len(x) or angles.shape[0] < 1 or angles.shape[1] < 1:
            raise ValueError("x[N], y[N] and angles[N, A] expected (N, A >= 1), got shapes %r, %r and %r" % (x.shape, y.shape, angles.shape))
        return x, y, angles

    @staticmethod
    def _member_planes(planes):
        """An ensemble's uploaded patches as uint8[n, A, ...]: member i's A headings in row i."""
        planes = N.as_u8(planes, "planes")
        if planes.ndim != 4 or planes.shape[0] < 1 or planes.shape[1] < 1:
            raise ValueError("planes must be uint8[n,A,h,w] with n, A >= 1, got shape %r" % (planes.shape,))
        return planes

    @staticmethod
    def _member_results(n, A):
        """The buffers a step of n members x A headings answers into: angle_familiarity, best_idex, flags."""
        return np.empty((n, A), dtype=np.float64), np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.uint32)

    def one_value(self, metric):
        """The bound train_u8, train_from_poses, score_u8, sense_step and end of the one-value model `metric` ("infomax" or
        "mushroom": ONE_VALUE_METRICS), so that a caller needs no branch per model."""
        prefix = one_value_prefix(metric)
        return SimpleNamespace(**{op: getattr(self, prefix + op) for op in ("train_u8", "train_from_poses", "score_u8", "sense_step", "end")})

    def _ov_train_u8(self, metric, planes):
        name = _ONE_VALUE[metric][0] + "train_u8"
        planes = self._ov_planes(metric, planes)
        self._check(getattr(self._lib, name)(self._ctx, N.u8ptr(planes), planes.shape[0]), name)

    def _ov_train_from_poses(self, metric, x, y, angle, want_views):
        name = _ONE_VALUE[metric][0] + "train_from_poses"
        x, y, angle = self._pose_arrays(x, y, angle)
        h, w = self.sensor_shape
        views = np.empty((len(x), h, w, 3), dtype=np.uint8) if want_views else None
        self._check_sense(getattr(self._lib, name)(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angle), len(x),
                                                   N.u8ptr(views) if want_views else None), name)
        return views

    def _ov_score_u8(self, metric, planes, out):
        name = _ONE_VALUE[metric][0] + "score_u8"
        planes = self._ov_planes(metric, planes)
        if out is None:
            out = np.empty(planes.shape[0], dtype=np.float64)
        assert out.dtype == np.float64 and out.flags.c_contiguous and out.size == planes.shape[0]
        self._check(getattr(self._lib, name)(self._ctx, N.u8ptr(planes), planes.shape[0], N.f64ptr(out)), name)
        return out

    def _ov_sense_step(self, metric, x, y, angles, out_fam):
        name = _ONE_VALUE[metric][0] + "sense_step"
        angles = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1)
        if out_fam is None:
            out_fam = np.empty(len(angles), dtype=np.float64)
        assert out_fam.dtype == np.float64 and out_fam.flags.c_contiguous and out_fam.size == len(angles)
        best = ctypes.c_int32(-1)
        self._check_sense(getattr(self._lib, name)(self._ctx, float(x), float(y), N.f64ptr(angles), len(angles), N.f64ptr(out_fam),
                                                   ctypes.byref(best)), name)
        return int(best.value), out_fam

    def _ov_step_batch_u8(self, metric, planes):
        name = _ONE_VALUE[metric][1] + "step_u8"
        planes = self._member_planes(planes)
        n, A = planes.shape[:2]
        flat = self._ov_planes(metric, planes.reshape((n * A,) + planes.shape[2:]))
        fam, best, flags = self._member_results(n, A)
        self._check(getattr(self._lib, name)(self._ctx, N.u8ptr(flat), n, A, N.f64ptr(fam), best.ctypes.data_as(N._i32p)), name)
        return OneValueBatchResults(fam, best, flags)

    def _ov_sense_step_batch(self, metric, x, y, angles):
        name = _ONE_VALUE[metric][1] + "sense_step"
        x, y, angles = self._member_poses(x, y, angles)
        n, A = angles.shape
        fam, best, flags = self._member_results(n, A)
        self._check(getattr(self._lib, name)(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angles), n, A, N.f64ptr(fam),
                                             best.ctypes.data_as(N._i32p), flags.ctypes.data_as(N._u32p)), name)
        return OneValueBatchResults(fam, best, flags)

    # -- ... and their banked calls (dv_ibank_*, dv_mbank_*): the same, with a bank per view or per member -------------------------
    def _bank_table(self, metric, table, n, what):
        return self._index_table(table, what, getattr(self, _ONE_VALUE[metric][5]), "n_banks", n, "bank")

    def _bank_symbol(self, metric, op, land_of, n, what):
        """The symbol of the banked call `op` and what follows the bank table in its arguments: nothing, or (land_of is not None: the
        call on the live landscape set) the landscape table, checked."""
        if land_of is None:
            return _ONE_VALUE[metric][3] + op, ()
        return _ONE_VALUE[metric][4] + op, (self._land_table(land_of, n, what).ctypes.data_as(N._i32p),)

    def _bank_train_u8(self, metric, planes, bank_of_view):
        name = _ONE_VALUE[metric][3] + "train_u8"
        planes = self._ov_planes(metric, planes)
        banks = self._bank_table(metric, bank_of_view, planes.shape[0], "bank_of_view")
        self._check(getattr(self._lib, name)(self._ctx, N.u8ptr(planes), planes.shape[0], banks.ctypes.data_as(N._i32p)), name)

    def _bank_train_from_poses(self, metric, x, y, angle, bank_of_view, want_views, land_of_view):
        x, y, angle = self._pose_arrays(x, y, angle)
        banks = self._bank_table(metric, bank_of_view, len(x), "bank_of_view")
        name, lands = self._bank_symbol(metric, "train_from_poses", land_of_view, len(x), "land_of_view")
        h, w = self.sensor_shape
        views = np.empty((len(x), h, w, 3), dtype=np.uint8) if want_views else None
        self._check_sense(getattr(self._lib, name)(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angle), len(x), banks.ctypes.data_as(N._i32p),
                                                   *lands, N.u8ptr(views) if want_views else None), name)
        return views

    def _bank_step_batch_u8(self, metric, planes, bank_of_member):
        name = _ONE_VALUE[metric][3] + "step_u8"
        planes = self._member_planes(planes)
        n, A = planes.shape[:2]
        banks = self._bank_table(metric, bank_of_member, n, "bank_of_member")
        flat = self._ov_planes(metric, planes.reshape((n * A,) + planes.shape[2:]))
        fam, best, flags = self._member_results(n, A)
        self._check(getattr(self._lib, name)(self._ctx, N.u8ptr(flat), n, A, banks.ctypes.data_as(N._i32p), N.f64ptr(fam),
                                             best.ctypes.data_as(N._i32p)), name)
        return OneValueBatchResults(fam, best, flags)

    def _bank_sense_step_batch(self, metric, x, y, angles, bank_of_member, land_of_member):
        x, y, angles = self._member_poses(x, y, angles)
        n, A = angles.shape
        banks = self._bank_table(metric, bank_of_member, n, "bank_of_member")
        name, lands = self._bank_symbol(metric, "sense_step", land_of_member, n, "land_of_member")
        fam, best, flags = self._member_results(n, A)
        self._check(getattr(self._lib, name)(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angles), n, A, banks.ctypes.data_as(N._i32p),
                                             *lands, N.f64ptr(fam), best.ctypes.data_as(N._i32p), flags.ctypes.data_as(N._u32p)), name)
        return OneValueBatchResults(fam, best, flags)

    # -- Infomax familiarity model: one layer of weights instead of a library (include/dejavu.h: dv_infomax_*) ----------------
    def infomax_begin(self, h, w, weights, channel=2, learning_rate=0.01):
        """weights: float64[n_hidden, h*w], the initial W (drawn by the caller: util.infomax_initial_weights).  Copied to the GPU."""
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.ndim != 2 or weights.shape[1] != int(h) * int(w):
            raise ValueError("weights must be float64[n_hidden, %d], got shape %r" % (int(h) * int(w), weights.shape))
        self._check(self._lib.dv_infomax_begin(self._ctx, int(h), int(w), int(channel), weights.shape[0], float(learning_rate),
                                               N.f64ptr(weights)), "dv_infomax_begin")
        self.infomax_shape = (int(h), int(w))
        self.infomax_hidden = weights.shape[0]
        self.infomax_banks = 1
        self.infomax_nets = self.infomax_net_of_bank = None

    def infomax_train_u8(self, planes):
        """One more pass of the learning rule over uint8[n,h,w] planes, in order, on the same W."""
        self._ov_train_u8("infomax", planes)

    def infomax_train_from_poses(self, x, y, angle, want_views=True):
        """train_from_path for the Infomax plug-in on the device: sense the poses, train on their compared plane; returns
        familiar_scenes (uint8[n,h,w,3]) when want_views."""
        return self._ov_train_from_poses("infomax", x, y, angle, want_views)

    def infomax_score_u8(self, planes, out=None):
        """familiarity = -sum|W x| of each of uint8[n,h,w] planes (or one uint8[h,w]) -> float64[n]."""
        return self._ov_score_u8("infomax", planes, out)

    def infomax_sense_step(self, x, y, angles, out_fam=None):
        """One agent step: sense the heading patches at (x, y), score them, first maximum -> (best_idex, angle_familiarity)."""
        return self._ov_sense_step("infomax", x, y, angles, out_fam)

    def infomax_step_batch_u8(self, planes):
        """An ensemble's step on uploaded patches: uint8[n, A, h, w] planes, member i's A headings in row i -> InfomaxBatchResults (every
        member's familiarities and first maximum from one device call; the flags are 0)."""
        return self._ov_step_batch_u8("infomax", planes)

    def infomax_sense_step_batch(self, x, y, angles):
        """An ensemble's step: member i at (x[i], y[i]) looking along angles[i][0..A) -> InfomaxBatchResults.  One enqueue and one wait
        for all members; a member whose footprint leaves the landscape is flagged (flags & 16, best_idex -1), the others are scored."""
        return self._ov_sense_step_batch("infomax", x, y, angles)

    def infomax_info(self):
        m, n, fin = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        views, nbytes = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._lib.dv_infomax_info(self._ctx, ctypes.byref(m), ctypes.byref(n), ctypes.byref(views), ctypes.byref(fin),
                                              ctypes.byref(nbytes)), "dv_infomax_info")
        return dict(n_hidden=m.value, n_pixels=n.value, views_trained=views.value, finite=bool(fin.value), bytes=nbytes.value)

    def infomax_read_weights(self):
        """float64[n_hidden, h*w]: what a user saves (np.save) and hands to infomax_set_weights or infomax_begin later."""
        info = self.infomax_info()
        out = np.empty((info["n_hidden"], info["n_pixels"]), dtype=np.float64)
        self._check(self._lib.dv_infomax_read_weights(self._ctx, N.f64ptr(out)), "dv_infomax_read_weights")
        return out

    def infomax_set_weights(self, weights):
        info = self.infomax_info()
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if info["n_hidden"] and weights.shape != (info["n_hidden"], info["n_pixels"]):
            raise ValueError("weights must be float64[%d,%d], got shape %r" % (info["n_hidden"], info["n_pixels"], weights.shape))
        self._check(self._lib.dv_infomax_set_weights(self._ctx, N.f64ptr(weights)), "dv_infomax_set_weights")

    def infomax_end(self):
        self._check(self._lib.dv_infomax_end(self._ctx), "dv_infomax_end")
        self.infomax_shape = None
        self.infomax_banks = 1
        self.infomax_nets = self.infomax_net_of_bank = None

    # -- weight banks of the Infomax model: several models of one shape in one context (include/dejavu.h: dv_ibank_*) ------------
    infomax_banks = 1            # banks of the model (ibank_set; 1 after infomax_begin)

    def _ibank_weights(self, weights, what, bank=None):
        info = self.infomax_info()
        if bank is not None and self.infomax_nets is not None:      # the bank's own shape under the live network table
            info = dict(info, n_hidden=self.infomax_nets[self.infomax_net_of_bank[bank]]["n_hidden"])
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if info["n_hidden"] and weights.shape != (info["n_hidden"], info["n_pixels"]):
            raise ValueError("%s must be float64[%d,%d], got shape %r" % (what, info["n_hidden"], info["n_pixels"], weights.shape))
        return weights

    def ibank_set(self, n_banks, weights):
        """n_banks banks, every one a copy of `weights` (float64[n_hidden, h*w]: the model's W0); what was trained is dropped.  The
        infomax_* calls keep acting on bank 0; infomax_begin and infomax_end return to one bank."""
        if isinstance(n_banks, bool) or not isinstance(n_banks, (int, np.integer)) or n_banks < 1:
            raise ValueError("n_banks must be an integer >= 1, got %r" % (n_banks,))
        weights = self._ibank_weights(weights, "weights")
        self._check(self._lib.dv_ibank_set(self._ctx, int(n_banks), N.f64ptr(weights)), "dv_ibank_set")
        self.infomax_banks = int(n_banks)
        self.infomax_nets = self.infomax_net_of_bank = None

    def ibank_train_u8(self, planes, bank_of_view):
        """infomax_train_u8 with view v trained into bank bank_of_view[v]: every bank's views in their order, the banks' chains in
        lockstep, three launches a step for all of them."""
        self._bank_train_u8("infomax", planes, bank_of_view)

    def ibank_train_from_poses(self, x, y, angle, bank_of_view, want_views=True, land_of_view=None):
        """infomax_train_from_poses with view v trained into bank bank_of_view[v] (the routes of a grid, trained in one call); returns
        the views (uint8[n,h,w,3]) when want_views."""
        return self._bank_train_from_poses("infomax", x, y, angle, bank_of_view, want_views, land_of_view)

    def ibank_step_batch_u8(self, planes, bank_of_member):
        """infomax_step_batch_u8 with member i scored under bank bank_of_member[i] -> OneValueBatchResults, in the caller's order."""
        return self._bank_step_batch_u8("infomax", planes, bank_of_member)

    def ibank_sense_step_batch(self, x, y, angles, bank_of_member, land_of_member=None):
        """infomax_sense_step_batch with member i scored under bank bank_of_member[i] -> OneValueBatchResults: one enqueue and one wait."""
        return self._bank_sense_step_batch("infomax", x, y, angles, bank_of_member, land_of_member)

    def ibank_read_weights(self, bank):
        """float64[n_hidden, h*w] of one bank; while a network table is live (inet_set), n_hidden is the bank's own network's."""
        bank = self._bank_index(bank, self.infomax_banks)
        info = self.infomax_info()
        if self.infomax_nets is not None:
            info = dict(info, n_hidden=self.infomax_nets[self.infomax_net_of_bank[bank]]["n_hidden"])
        out = np.empty((max(info["n_hidden"], 1), max(info["n_pixels"], 1)), dtype=np.float64)
        self._check(self._lib.dv_ibank_read_weights(self._ctx, bank, N.f64ptr(out)), "dv_ibank_read_weights")
        return out

    def ibank_set_weights(self, bank, weights):
        bank = self._bank_index(bank, self.infomax_banks)
        weights = self._ibank_weights(weights, "weights", bank)
        self._check(self._lib.dv_ibank_set_weights(self._ctx, bank, N.f64ptr(weights)), "dv_ibank_set_weights")

    def ibank_info(self):
        """dict(n_banks, views_trained int64[n_banks], finite bool[n_banks])."""
        nb = ctypes.c_int(0)
        self._check(self._lib.dv_ibank_info(self._ctx, ctypes.byref(nb), None, None), "dv_ibank_info")
        views = np.zeros(max(nb.value, 1), dtype=np.int64)
        finite = np.zeros(max(nb.value, 1), dtype=np.int32)
        self._check(self._lib.dv_ibank_info(self._ctx, None, views.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                            finite.ctypes.data_as(N._i32p)), "dv_ibank_info")
        return dict(n_banks=nb.value, views_trained=views, finite=finite.astype(bool))

    # -- network tables of the Infomax model: a bank's own n_hidden, learning rate, W0 and channel (include/dejavu.h: dv_inet_*) ----
    infomax_nets = None          # the live table's networks, dict(channel, n_hidden, learning_rate) each (inet_set; None: no table)
    infomax_net_of_bank = None   # int32[n_banks]: the network of every bank of the live table
    IM_MAX_HIDDEN = 1 << 20

    @classmethod
    def _network(cls, p, net, n_pixels):
        """networks[p] as (dict(channel, n_hidden, learning_rate), w0 float64[n_hidden, n_pixels]), or ValueError naming the entry.
        n_pixels: h * w of the model (None: no model yet, and the library answers DV_ERR_STATE)."""
        who = "networks[%d]" % p
        if not isinstance(net, dict) or "w0" not in net or "learning_rate" not in net:
            raise ValueError("%s must be a dict with w0 and learning_rate (util.infomax_network makes one)" % who)
        extra = sorted(set(net) - {"w0", "learning_rate", "channel", "n_hidden", "seed"})
        if extra:
            raise ValueError("%s: unknown keys %r" % (who, extra))
        w0 = np.asarray(net["w0"])
        if w0.dtype != np.float64:
            raise ValueError("%s: w0 must be float64, got dtype %s" % (who, w0.dtype))
        if w0.ndim != 2 or (n_pixels is not None and w0.shape[1] != n_pixels):
            raise ValueError("%s: w0 must be float64[n_hidden, %s], got shape %r" % (who, "h*w" if n_pixels is None else n_pixels, w0.shape))
        n_hidden = w0.shape[0]

        def whole(v):
            return isinstance(v, (int, np.integer)) and not isinstance(v, bool)

        if "n_hidden" in net and not (whole(net["n_hidden"]) and net["n_hidden"] == n_hidden):
            raise ValueError("%s: n_hidden = %r, but w0 has shape %r" % (who, net["n_hidden"], w0.shape))
        if not 1 <= n_hidden <= cls.IM_MAX_HIDDEN:
            raise ValueError("%s: n_hidden %d outside [1, %d]" % (who, n_hidden, cls.IM_MAX_HIDDEN))
        rate, channel = net["learning_rate"], net.get("channel", 2)
        if isinstance(rate, bool) or not isinstance(rate, (int, float, np.floating, np.integer)) or not (rate > 0 and np.isfinite(rate)):
            raise ValueError("%s: learning_rate %r must be a positive number" % (who, rate))
        if not (whole(channel) and 0 <= channel <= 2):
            raise ValueError("%s: channel %r outside [0, 2]" % (who, channel))
        return dict(channel=int(channel), n_hidden=int(n_hidden), learning_rate=float(rate)), np.ascontiguousarray(w0)

    def inet_set(self, networks, network_of_bank):
        """A network table: networks is a list of dicts (util.infomax_network: channel, n_hidden, learning_rate, w0 float64[n_hidden,
        h*w] over the model's pixels), network_of_bank names every bank's network (its length is the number of banks; several banks
        may share one).  Every bank starts as a copy of its network's w0; what was trained is dropped.  From here on the ibank_* calls
        train and score every view and member through its bank's own n_hidden, learning rate and channel, and the infomax_* calls
        (bank 0 behind the begin's shape) are refused until inet_clear, ibank_set, infomax_begin or infomax_end.  Every entry is
        checked here, before any library call; ValueError names it."""
        if isinstance(networks, dict) or not hasattr(networks, "__len__") or len(networks) < 1:
            raise ValueError("networks must be a list of one or more dicts (util.infomax_network), got %r" % (type(networks).__name__,))
        n_pixels = None if self.infomax_shape is None else self.infomax_shape[0] * self.infomax_shape[1]
        nets, w0s = zip(*[self._network(p, net, n_pixels) for p, net in enumerate(networks)])
        of_bank = self._index_table(network_of_bank, "network_of_bank", len(nets), "n_nets", per="network")
        if not 1 <= len(of_bank) <= 65535:
            raise ValueError("network_of_bank must name the network of 1 to 65535 banks, got %d" % len(of_bank))
        n_hidden = np.array([p["n_hidden"] for p in nets], dtype=np.int32)
        channel = np.array([p["channel"] for p in nets], dtype=np.int32)
        rate = np.array([p["learning_rate"] for p in nets], dtype=np.float64)
        concat = np.ascontiguousarray(np.concatenate([w.reshape(-1) for w in w0s]), dtype=np.float64)
        i32 = lambda a: a.ctypes.data_as(N._i32p)
        self._check(self._lib.dv_inet_set(self._ctx, len(nets), i32(n_hidden), N.f64ptr(rate), i32(channel), N.f64ptr(concat), len(of_bank),
                                          i32(of_bank)), "dv_inet_set")
        self.infomax_nets, self.infomax_net_of_bank, self.infomax_banks = list(nets), of_bank, len(of_bank)

    def inet_clear(self):
        """Back to one bank of the network infomax_begin made, at its initial weights."""
        self._check(self._lib.dv_inet_clear(self._ctx), "dv_inet_clear")
        self.infomax_nets, self.infomax_net_of_bank, self.infomax_banks = None, None, 1

    def inet_info(self):
        """dict(n_nets, n_banks, n_hidden / channel int32[n_nets], learning_rate float64[n_nets], network_of_bank int32[n_banks],
        views_trained int64[n_banks], finite bool[n_banks], bytes); n_nets = n_banks = 0 and empty arrays without a table."""
        P, B, nbytes = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
        self._check(self._lib.dv_inet_info(self._ctx, ctypes.byref(P), ctypes.byref(B), None, None, None, None, None, None, ctypes.byref(nbytes)),
                    "dv_inet_info")
        n_hidden, channel = np.zeros(P.value, dtype=np.int32), np.zeros(P.value, dtype=np.int32)
        rate = np.zeros(P.value, dtype=np.float64)
        of_bank, finite = np.zeros(B.value, dtype=np.int32), np.zeros(B.value, dtype=np.int32)
        views = np.zeros(B.value, dtype=np.int64)
        if P.value:
            i32 = lambda a: a.ctypes.data_as(N._i32p)
            self._check(self._lib.dv_inet_info(self._ctx, None, None, i32(n_hidden), N.f64ptr(rate), i32(channel), i32(of_bank),
                                               views.ctypes.data_as(N._i64p), i32(finite), None), "dv_inet_info")
        return dict(n_nets=P.value, n_banks=B.value, n_hidden=n_hidden, learning_rate=rate, channel=channel, network_of_bank=of_bank,
                    views_trained=views, finite=finite.astype(bool), bytes=nbytes.value)

    # -- mushroom-body familiarity model: a fixed fan-in and one byte of weight per Kenyon cell (include/dejavu.h: dv_mb_*) --------
    def mb_begin(self, h, w, conn, n_active, channel=2):
        """conn: int32[n_kc, fan_in], the pixels each Kenyon cell listens to (drawn by the caller: util.mushroom_connectivity).
        Copied to the GPU; the weights start at 1."""
        conn = np.ascontiguousarray(conn, dtype=np.int32)
        if conn.ndim != 2:
            raise ValueError("conn must be int32[n_kc, fan_in], got shape %r" % (conn.shape,))
        self._check(self._lib.dv_mb_begin(self._ctx, int(h), int(w), int(channel), conn.shape[0], conn.shape[1], int(n_active),
                                          conn.ctypes.data_as(N._i32p)), "dv_mb_begin")
        self.mb_shape = (int(h), int(w))
        self.mb_banks = 1
        self.mb_pops = None
        self.mb_active = int(n_active)

    def mb_train_u8(self, planes):
        """Depress the cells that fire for each of uint8[n,h,w] planes: one launch for all of them, in no order."""
        self._ov_train_u8("mushroom", planes)

    def mb_train_from_poses(self, x, y, angle, want_views=True):
        """train_from_path for the mushroom-body plug-in on the device: sense the poses, train on their compared plane; returns
        familiar_scenes (uint8[n,h,w,3]) when want_views."""
        return self._ov_train_from_poses("mushroom", x, y, angle, want_views)

    def mb_score_u8(self, planes, out=None):
        """familiarity = -(firing cells whose weight is intact) of each of uint8[n,h,w] planes (or one uint8[h,w]) -> float64[n]."""
        return self._ov_score_u8("mushroom", planes, out)

    def mb_activity_u8(self, planes):
        """Which cells each of uint8[n,h,w] planes excites -> (fired uint8[n, n_kc], threshold int32[n]: the least activity that fires)."""
        planes = self._ov_planes("mushroom", planes)
        fired = np.empty((planes.shape[0], self.mb_info()["n_kc"]), dtype=np.uint8)
        thr = np.empty(planes.shape[0], dtype=np.int32)
        self._check(self._lib.dv_mb_activity_u8(self._ctx, N.u8ptr(planes), planes.shape[0], N.u8ptr(fired), thr.ctypes.data_as(N._i32p)),
                    "dv_mb_activity_u8")
        return fired, thr

    def mb_sense_step(self, x, y, angles, out_fam=None):
        """One agent step: sense the heading patches at (x, y), score them, first maximum -> (best_idex, angle_familiarity)."""
        return self._ov_sense_step("mushroom", x, y, angles, out_fam)

    def mb_step_batch_u8(self, planes):
        """An ensemble's step on uploaded patches: uint8[n, A, h, w] planes, member i's A headings in row i -> InfomaxBatchResults (every
        member's familiarities and first maximum from one device call; the flags are 0)."""
        return self._ov_step_batch_u8("mushroom", planes)

    def mb_sense_step_batch(self, x, y, angles):
        """An ensemble's step: member i at (x[i], y[i]) looking along angles[i][0..A) -> InfomaxBatchResults.  One enqueue and one wait
        for all members; a member whose footprint leaves the landscape is flagged (flags & 16, best_idex -1), the others are scored."""
        return self._ov_sense_step_batch("mushroom", x, y, angles)

    def mb_info(self):
        k, n, c, act = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        views, zeros, nbytes = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._lib.dv_mb_info(self._ctx, ctypes.byref(k), ctypes.byref(n), ctypes.byref(c), ctypes.byref(act), ctypes.byref(views),
                                         ctypes.byref(zeros), ctypes.byref(nbytes)), "dv_mb_info")
        return dict(n_kc=k.value, n_pixels=n.value, fan_in=c.value, n_active=act.value, views_trained=views.value,
                    n_depressed=zeros.value, bytes=nbytes.value)

    def mb_read_weights(self):
        """uint8[n_kc], 1 or 0: what a user saves (np.save) and hands to mb_set_weights later."""
        out = np.empty(max(self.mb_info()["n_kc"], 1), dtype=np.uint8)
        self._check(self._lib.dv_mb_read_weights(self._ctx, N.u8ptr(out)), "dv_mb_read_weights")
        return out

    def mb_set_weights(self, weights):
        n_kc = self.mb_info()["n_kc"]
        weights = N.as_u8(weights, "weights")
        if n_kc and weights.shape != (n_kc,):
            raise ValueError("weights must be uint8[%d], got shape %r" % (n_kc, weights.shape))
        self._check(self._lib.dv_mb_set_weights(self._ctx, N.u8ptr(weights)), "dv_mb_set_weights")

    def mb_end(self):
        self._check(self._lib.dv_mb_end(self._ctx), "dv_mb_end")
        self.mb_shape = None
        self.mb_banks = 1
        self.mb_pops = None
        self.mb_active = None

    # -- memory banks of the mushroom-body model: several memories behind one connectivity (include/dejavu.h: dv_mbank_*) ---------
    mb_banks = 1                 # memories of the model (mbank_set; 1 after mb_begin)

    def _bank_index(self, bank, n_banks=None):
        n_banks = self.mb_banks if n_banks is None else n_banks
        if isinstance(bank, bool) or not isinstance(bank, (int, np.integer)) or not 0 <= bank < n_banks:
            raise ValueError("bank must be an integer in [0, n_banks = %d), got %r" % (n_banks, bank))
        return int(bank)

    def mbank_set(self, n_banks):
        """n_banks memories behind the model's connectivity, all weights 1 (what was trained is dropped).  The mb_* calls keep acting
        on bank 0; mb_begin and mb_end return to one bank."""
        if isinstance(n_banks, bool) or not isinstance(n_banks, (int, np.integer)) or n_banks < 1:
            raise ValueError("n_banks must be an integer >= 1, got %r" % (n_banks,))
        self._check(self._lib.dv_mbank_set(self._ctx, int(n_banks)), "dv_mbank_set")
        self.mb_banks = int(n_banks)
        self.mb_pops = None

    def mbank_train_u8(self, planes, bank_of_view):
        """mb_train_u8 with view v depressing bank bank_of_view[v]: the views of all banks in the same launches."""
        self._bank_train_u8("mushroom", planes, bank_of_view)

    def mbank_train_from_poses(self, x, y, angle, bank_of_view, want_views=True, land_of_view=None):
        """mb_train_from_poses with view v depressing bank bank_of_view[v] (the routes of a grid, trained in one call); returns the
        views (uint8[n,h,w,3]) when want_views."""
        return self._bank_train_from_poses("mushroom", x, y, angle, bank_of_view, want_views, land_of_view)

    def mbank_step_batch_u8(self, planes, bank_of_member):
        """mb_step_batch_u8 with member i scored under bank bank_of_member[i] -> OneValueBatchResults."""
        return self._bank_step_batch_u8("mushroom", planes, bank_of_member)

    def mbank_sense_step_batch(self, x, y, angles, bank_of_member, land_of_member=None):
        """mb_sense_step_batch with member i scored under bank bank_of_member[i] -> OneValueBatchResults: one enqueue and one wait."""
        return self._bank_sense_step_batch("mushroom", x, y, angles, bank_of_member, land_of_member)

    # -- bank sets: one selection of firing cells read out through several banks (include/dejavu.h: dv_mbset_*) ------------------
    mb_active = None             # n_active of the model mb_begin made (None: no model)

    @staticmethod
    def mbset_tables(bank_sets, coefs, n, n_banks, n_active):
        """`bank_sets` and `coefs` as int32[n, S] (1 <= S <= DV_MBSET_MAX_BANKS), or ValueError naming the entry: integers, one shape,
        banks in [0, n_banks), coefficients in int32, and per member sum |coefs| * n_active <= 2^31 - 1 (the member's value cannot
        wrap).  n_banks / n_active None: not known here, the library checks."""
        banks, cf = np.asarray(bank_sets), np.asarray(coefs)
        for arr, what in ((banks, "bank_sets"), (cf, "coefs")):
            if arr.dtype.kind not in "iu":
                raise ValueError("%s must hold integers, got dtype %s" % (what, arr.dtype))
            if arr.ndim != 2 or arr.shape[0] != n or not 1 <= arr.shape[1] <= N.DV_MBSET_MAX_BANKS:
                raise ValueError("%s must have shape (%d, S) with 1 <= S <= DV_MBSET_MAX_BANKS = %d, got %r"
                                 % (what, n, N.DV_MBSET_MAX_BANKS, arr.shape))
        if banks.shape != cf.shape:
            raise ValueError("bank_sets and coefs must have one shape, got %r and %r" % (banks.shape, cf.shape))
        if n_banks is not None and (banks.min() < 0 or banks.max() >= n_banks):
            i, j = np.argwhere((banks < 0) | (banks >= n_banks))[0]
            raise ValueError("bank_sets[%d][%d] = %d outside [0, n_banks = %d)" % (i, j, banks[i, j], n_banks))
        if cf.min() < -2 ** 31 or cf.max() > 2 ** 31 - 1:
            i, j = np.argwhere((cf < -2 ** 31) | (cf > 2 ** 31 - 1))[0]
            raise ValueError("coefs[%d][%d] = %d does not fit an int32" % (i, j, cf[i, j]))
        if n_active is not None:
            mag = np.abs(cf.astype(np.int64)).sum(axis=1)          # (every entry fits an int32: at most 2^34 a member, 2^58 with n_active)
            over = np.flatnonzero(mag * np.int64(n_active) > 2 ** 31 - 1)
            if len(over):
                raise ValueError("member %d: sum |coefs| = %d times n_active = %d exceeds 2^31 - 1" % (over[0], mag[over[0]], n_active))
        return np.ascontiguousarray(banks, dtype=np.int32), np.ascontiguousarray(cf, dtype=np.int32)

    def mbset_step_batch_u8(self, planes, bank_sets, coefs):
        """An ensemble's step on uploaded uint8[n, A, h, w] planes with member i read out through the banks bank_sets[i][0..S) from ONE
        selection of firing cells: angle_familiarity[i][a] = -(sum_j coefs[i][j] * d_j), d_j the column's novelty under bank
        bank_sets[i][j] -> MbSetBatchResults (bank_novelty int32[n, A, S] holds the d_j)."""
        planes = self._member_planes(planes)
        n, A = planes.shape[:2]
        banks, cf = self.mbset_tables(bank_sets, coefs, n, self.mb_banks if self.mb_shape else None, self.mb_active)
        flat = self._ov_planes("mushroom", planes.reshape((n * A,) + planes.shape[2:]))
        fam, best, flags = self._member_results(n, A)
        nov = np.empty((n, A, banks.shape[1]), dtype=np.int32)
        i32 = lambda a: a.ctypes.data_as(N._i32p)
        self._check(self._lib.dv_mbset_step_u8(self._ctx, N.u8ptr(flat), n, A, banks.shape[1], i32(banks), i32(cf), N.f64ptr(fam), i32(best),
                                               i32(nov)), "dv_mbset_step_u8")
        return MbSetBatchResults(fam, best, flags, nov)

    def mbset_sense_step_batch(self, x, y, angles, bank_sets, coefs, land_of_member=None):
        """mbset_step_batch_u8 from poses: member i at (x[i], y[i]) looking along angles[i][0..A), on the engine's landscape or
        (land_of_member) on its landscape of the live set, under the set's sensor table and noise rows where there are any.  One
        enqueue and one wait; a member whose footprint leaves its landscape is flagged (flags & 16, best_idex -1)."""
        x, y, angles = self._member_poses(x, y, angles)
        n, A = angles.shape
        banks, cf = self.mbset_tables(bank_sets, coefs, n, self.mb_banks if self.mb_shape else None, self.mb_active)
        lands = () if land_of_member is None else (self._land_table(land_of_member, n, "land_of_member").ctypes.data_as(N._i32p),)
        name = "dv_mbset_sense_step" if land_of_member is None else "dv_mbset_lands_sense_step"
        fam, best, flags = self._member_results(n, A)
        nov = np.empty((n, A, banks.shape[1]), dtype=np.int32)
        i32 = lambda a: a.ctypes.data_as(N._i32p)
        self._check(getattr(self._lib, name)(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angles), n, A, banks.shape[1], i32(banks), i32(cf),
                                             *lands, N.f64ptr(fam), i32(best), flags.ctypes.data_as(N._u32p), i32(nov)), name)
        return MbSetBatchResults(fam, best, flags, nov)

    def _bank_cells(self, bank):
        """n_kc of bank `bank` under the live population table."""
        return self.mb_pops[self.mb_pop_of_bank[bank]]["n_kc"]

    def mbank_read_weights(self, bank=None):
        """uint8[n_kc] of one bank; bank=None: all of them, uint8[n_banks, n_kc] -- or, while a population table is live (mbpop_set), a
        list of n_banks arrays, each uint8[n_kc of the bank's own population]: the banks are ragged."""
        if bank is not None:
            bank = self._bank_index(bank)
        if self.mb_pops is not None:
            out = []
            for b in (range(self.mb_banks) if bank is None else (bank,)):
                out.append(np.empty(self._bank_cells(b), dtype=np.uint8))
                self._check(self._lib.dv_mbank_read_weights(self._ctx, b, N.u8ptr(out[-1])), "dv_mbank_read_weights")
            return out if bank is None else out[0]
        n_kc = max(self.mb_info()["n_kc"], 1)
        out = np.empty((self.mb_banks if bank is None else 1, n_kc), dtype=np.uint8)
        for row, b in enumerate(range(self.mb_banks) if bank is None else (bank,)):
            self._check(self._lib.dv_mbank_read_weights(self._ctx, b, N.u8ptr(out[row])), "dv_mbank_read_weights")
        return out if bank is None else out[0]

    def mbank_set_weights(self, bank, weights):
        bank = self._bank_index(bank)
        n_kc = self._bank_cells(bank) if self.mb_pops is not None else self.mb_info()["n_kc"]
        weights = N.as_u8(weights, "weights")
        if n_kc and weights.shape != (n_kc,):
            raise ValueError("weights must be uint8[%d], got shape %r" % (n_kc, weights.shape))
        self._check(self._lib.dv_mbank_set_weights(self._ctx, bank, N.u8ptr(weights)), "dv_mbank_set_weights")

    def mbank_info(self):
        """dict(n_banks, views_trained int64[n_banks], n_depressed int64[n_banks])."""
        nb = ctypes.c_int(0)
        self._check(self._lib.dv_mbank_info(self._ctx, ctypes.byref(nb), None, None), "dv_mbank_info")
        views = np.zeros(max(nb.value, 1), dtype=np.int64)
        zeros = np.zeros(max(nb.value, 1), dtype=np.int64)
        i64p = ctypes.POINTER(ctypes.c_int64)
        self._check(self._lib.dv_mbank_info(self._ctx, None, views.ctypes.data_as(i64p), zeros.ctypes.data_as(i64p)), "dv_mbank_info")
        return dict(n_banks=nb.value, views_trained=views, n_depressed=zeros)

    # -- population tables of the mushroom-body model: a bank's own cells, wiring, quota and channel (include/dejavu.h: dv_mbpop_*) --
    mb_pops = None               # the live table's populations, dict(channel, n_kc, fan_in, n_active) each (mbpop_set; None: no table)
    mb_pop_of_bank = None        # int32[n_banks]: the population of every bank of the live table
    MB_MAX_CELLS, MB_MAX_FAN_IN = 1 << 24, 16

    @classmethod
    def _population(cls, p, pop, n_pixels):
        """populations[p] as (dict(channel, n_kc, fan_in, n_active), conn int32[n_kc, fan_in]), or ValueError naming the entry.
        n_pixels: h * w of the model (None: no model yet, and the library answers DV_ERR_STATE)."""
        who = "populations[%d]" % p
        if not isinstance(pop, dict) or "conn" not in pop or "n_active" not in pop:
            raise ValueError("%s must be a dict with conn and n_active (util.mushroom_population makes one)" % who)
        extra = sorted(set(pop) - {"conn", "n_active", "channel", "n_kc", "fan_in", "seed", "sparsity"})
        if extra:
            raise ValueError("%s: unknown keys %r" % (who, extra))
        conn = np.asarray(pop["conn"])
        if conn.dtype.kind not in "iu":
            raise ValueError("%s: conn must hold integers, got dtype %s" % (who, conn.dtype))
        if conn.ndim != 2:
            raise ValueError("%s: conn must be int32[n_kc, fan_in], got shape %r" % (who, conn.shape))
        n_kc, fan_in = conn.shape

        def whole(v):
            return isinstance(v, (int, np.integer)) and not isinstance(v, bool)

        for key, have in (("n_kc", n_kc), ("fan_in", fan_in)):
            if key in pop and not (whole(pop[key]) and pop[key] == have):
                raise ValueError("%s: %s = %r, but conn has shape %r" % (who, key, pop[key], conn.shape))
        if not 1 <= n_kc <= cls.MB_MAX_CELLS:
            raise ValueError("%s: n_kc %d outside [1, %d]" % (who, n_kc, cls.MB_MAX_CELLS))
        if not 1 <= fan_in <= cls.MB_MAX_FAN_IN:
            raise ValueError("%s: fan_in %d outside [1, %d]" % (who, fan_in, cls.MB_MAX_FAN_IN))
        n_active, channel = pop["n_active"], pop.get("channel", 2)
        if not (whole(n_active) and 1 <= n_active <= n_kc):
            raise ValueError("%s: n_active %r outside [1, n_kc = %d]" % (who, n_active, n_kc))
        if not (whole(channel) and 0 <= channel <= 2):
            raise ValueError("%s: channel %r outside [0, 2]" % (who, channel))
        if n_pixels is not None and (conn.min() < 0 or conn.max() >= n_pixels):
            k, j = np.argwhere((conn < 0) | (conn >= n_pixels))[0]
            raise ValueError("%s: conn[%d][%d] = %d outside [0, %d)" % (who, k, j, conn[k, j], n_pixels))
        return dict(channel=int(channel), n_kc=int(n_kc), fan_in=int(fan_in), n_active=int(n_active)), np.ascontiguousarray(conn, dtype=np.int32)

    def mbpop_set(self, populations, population_of_bank):
        """A population table: populations is a list of dicts (util.mushroom_population: channel, n_kc, fan_in, n_active, conn
        int32[n_kc, fan_in] over the model's h * w pixels), population_of_bank names every bank's population (its length is the number
        of banks; several banks may share one).  All weights 1; what was trained is dropped.  From here on the mbank_* calls train and
        score every view and member through its bank's own cells, wiring, quota and channel, and the mb_* calls (bank 0 behind the
        begin's wiring) are refused until mbpop_clear, mbank_set, mb_begin or mb_end.  Every entry is checked here, before any library
        call; ValueError names it."""
        if isinstance(populations, dict) or not hasattr(populations, "__len__") or len(populations) < 1:
            raise ValueError("populations must be a list of one or more dicts (util.mushroom_population), got %r" % (type(populations).__name__,))
        n_pixels = None if self.mb_shape is None else self.mb_shape[0] * self.mb_shape[1]
        pops, conns = zip(*[self._population(p, pop, n_pixels) for p, pop in enumerate(populations)])
        of_bank = self._index_table(population_of_bank, "population_of_bank", len(pops), "n_pops", per="population")
        if len(of_bank) < 1:
            raise ValueError("population_of_bank must name the population of one or more banks, got none")
        col = lambda key: np.array([p[key] for p in pops], dtype=np.int32)
        n_kc, fan_in, n_active, channel = col("n_kc"), col("fan_in"), col("n_active"), col("channel")
        concat = np.ascontiguousarray(np.concatenate([c.reshape(-1) for c in conns]), dtype=np.int32)
        i32 = lambda a: a.ctypes.data_as(N._i32p)
        self._check(self._lib.dv_mbpop_set(self._ctx, len(pops), i32(n_kc), i32(fan_in), i32(n_active), i32(channel), i32(concat), len(of_bank),
                                           i32(of_bank)), "dv_mbpop_set")
        self.mb_pops, self.mb_pop_of_bank, self.mb_banks = list(pops), of_bank, len(of_bank)

    def mbpop_clear(self):
        """Back to one bank of the population mb_begin made, weights 1."""
        self._check(self._lib.dv_mbpop_clear(self._ctx), "dv_mbpop_clear")
        self.mb_pops, self.mb_pop_of_bank, self.mb_banks = None, None, 1

    def mbpop_info(self):
        """dict(n_pops, n_banks, n_kc / fan_in / n_active / channel int32[n_pops], population_of_bank int32[n_banks], views_trained /
        n_depressed int64[n_banks], bytes); n_pops = n_banks = 0 and empty arrays without a table."""
        P, B, nbytes = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
        self._check(self._lib.dv_mbpop_info(self._ctx, ctypes.byref(P), ctypes.byref(B), None, None, None, None, None, None, None,
                                            ctypes.byref(nbytes)), "dv_mbpop_info")
        per_pop = [np.zeros(P.value, dtype=np.int32) for _ in range(4)]
        of_bank = np.zeros(B.value, dtype=np.int32)
        views, zeros = np.zeros(B.value, dtype=np.int64), np.zeros(B.value, dtype=np.int64)
        if P.value:
            self._check(self._lib.dv_mbpop_info(self._ctx, None, None, *([a.ctypes.data_as(N._i32p) for a in per_pop] +
                                                [of_bank.ctypes.data_as(N._i32p), views.ctypes.data_as(N._i64p), zeros.ctypes.data_as(N._i64p), None])),
                        "dv_mbpop_info")
        return dict(n_pops=P.value, n_banks=B.value, n_kc=per_pop[0], fan_in=per_pop[1], n_active=per_pop[2], channel=per_pop[3],
                    population_of_bank=of_bank, views_trained=views, n_depressed=zeros, bytes=nbytes.value)

    # -- landscape sets: several landscapes resident together, a landscape per pose (include/dejavu.h: dv_lands_*) -----------------
    n_lands = 0                  # landscapes of the set (lands_set; 0: none)

    def _land_table(self, table, n, what):
        """`table` as int32[n] with every entry in [0, n_lands), or ValueError naming `what`: checked before any library call."""
        if not self.n_lands:
            raise N.EngineError("%s given, but the engine holds no landscape set: lands_set first (DV_ERR_STATE)" % what)
        return self._index_table(table, what, self.n_lands, "n_lands", n, "landscape")

    def lands_set(self, landscapes):
        """landscapes: a list of uint8[rows, cols, 3] HSV of any shapes and strides (copied), kept resident together beside the engine's
        one landscape (set_landscape), which they leave alone.  The sensor configuration is the engine's one (configure_sensor) until
        sensors_set gives every landscape of the set its own; a new set drops that table."""
        lands = [N.as_u8(l, "landscapes[%d]" % i) for i, l in enumerate(landscapes)]
        if not lands:
            raise ValueError("no landscapes: a set holds at least one")
        for i, l in enumerate(lands):
            if l.ndim != 3 or l.shape[2] != 3 or l.shape[0] < 1 or l.shape[1] < 1:
                raise ValueError("landscapes[%d] must be uint8[rows, cols, 3], got shape %r" % (i, l.shape))
        flat = np.concatenate([l.reshape(-1) for l in lands])
        rows = np.array([l.shape[0] for l in lands], dtype=np.int32)
        cols = np.array([l.shape[1] for l in lands], dtype=np.int32)
        self._check(self._lib.dv_lands_set(self._ctx, N.u8ptr(flat), rows.ctypes.data_as(N._i32p), cols.ctypes.data_as(N._i32p), len(lands), 3),
                    "dv_lands_set")
        self.n_lands = len(lands)
        self.n_sensors = 0                                       # (a sensor table belonged to the old set's entries: the library drops it)

    def lands_clear(self):
        self._check(self._lib.dv_lands_clear(self._ctx), "dv_lands_clear")
        self.n_lands = 0
        self.n_sensors = 0

    def lands_info(self):
        """dict(n_lands, shapes: list of (rows, cols), bytes)."""
        nl, nbytes = ctypes.c_int(0), ctypes.c_int64(0)
        self._check(self._lib.dv_lands_info(self._ctx, ctypes.byref(nl), None, None, ctypes.byref(nbytes)), "dv_lands_info")
        rows = np.zeros(max(nl.value, 1), dtype=np.int32)
        cols = np.zeros(max(nl.value, 1), dtype=np.int32)
        self._check(self._lib.dv_lands_info(self._ctx, None, rows.ctypes.data_as(N._i32p), cols.ctypes.data_as(N._i32p), None), "dv_lands_info")
        return dict(n_lands=nl.value, shapes=[(int(r), int(c)) for r, c in zip(rows[:nl.value], cols[:nl.value])], bytes=nbytes.value)

    def lands_sense(self, x, y, angle, land_of_pose):
        """sense() with pose v on landscape land_of_pose[v] of the set -> uint8[n, h, w, 3].  IndexError names the first pose whose
        footprint leaves its own landscape."""
        x, y, angle = self._pose_arrays(x, y, angle)
        lands = self._land_table(land_of_pose, len(x), "land_of_pose")
        if len(x) < 1:
            raise ValueError("no poses")
        h, w = self.sensor_shape
        out = np.empty((len(x), h, w, 3), dtype=np.uint8)
        self._check_sense(self._lib.dv_lands_sense(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angle), lands.ctypes.data_as(N._i32p), len(x),
                                                   N.u8ptr(out)), "dv_lands_sense")
        return out

    # -- sensor tables: a sensor configuration per landscape of the set (include/dejavu.h: dv_sensors_*) ---------------------------
    n_sensors = 0                # entries of the set's sensor table (sensors_set; 0: the engine's one sensor for every landscape)
    SENSOR_MAX_BLOCK = 4096      # pw * ph of a sensor pixel, as dv_configure_sensor bounds it

    def sensors_set(self, pixel_dimensions, luts, masks):
        """A sensor per landscape of the live set: entry l is what landscape l is sensed with by every call that takes a landscape
        table.  pixel_dimensions: integers [n_lands, 2], (pw, ph) a row; luts: uint8[n_lands, 3, 256] level tables; masks: integers
        [n_lands] (mask_middle_n).  The sensor's w x h stays the engine's one (configure_sensor).  Dtype, shape and range are checked
        before any library call; ValueError names the entry."""
        if not self.n_lands:
            raise N.EngineError("sensors_set: the engine holds no landscape set: lands_set first (DV_ERR_STATE)")
        if getattr(self, "sensor_shape", None) is None:
            raise N.EngineError("sensors_set: no sensor configured: configure_sensor sets the w x h all entries share (DV_ERR_STATE)")
        n = self.n_lands
        px, mk, lt = np.asarray(pixel_dimensions), np.asarray(masks), np.asarray(luts)
        for arr, what, shape in ((px, "pixel_dimensions", (n, 2)), (mk, "masks", (n,))):
            if arr.dtype.kind not in "iu":
                raise ValueError("%s must hold integers, got dtype %s" % (what, arr.dtype))
            if arr.shape != shape:
                raise ValueError("%s must have shape %r (an entry per landscape of the set), got %r" % (what, shape, arr.shape))
        if lt.dtype != np.uint8:
            raise ValueError("luts must be uint8 level tables, got dtype %s" % lt.dtype)
        if lt.shape != (n, 3, 256):
            raise ValueError("luts must have shape %r (an entry per landscape of the set), got %r" % ((n, 3, 256), lt.shape))
        w = self.sensor_shape[1]
        for l in range(n):
            pw, ph, m = int(px[l, 0]), int(px[l, 1]), int(mk[l])
            if pw < 1 or ph < 1 or pw * ph > self.SENSOR_MAX_BLOCK:
                raise ValueError("pixel_dimensions[%d] = (%d, %d): pw, ph >= 1 and pw * ph <= %d" % (l, pw, ph, self.SENSOR_MAX_BLOCK))
            if not 0 <= m <= w // 2:
                raise ValueError("masks[%d] = %d outside [0, w / 2 = %d]" % (l, m, w // 2))
        pw = np.ascontiguousarray(px[:, 0], dtype=np.int32)
        ph = np.ascontiguousarray(px[:, 1], dtype=np.int32)
        mk = np.ascontiguousarray(mk, dtype=np.int32)
        lt = np.ascontiguousarray(lt)
        self._check(self._lib.dv_sensors_set(self._ctx, pw.ctypes.data_as(N._i32p), ph.ctypes.data_as(N._i32p), mk.ctypes.data_as(N._i32p),
                                             N.u8ptr(lt), n), "dv_sensors_set")
        self.n_sensors = n

    def sensors_clear(self):
        self._check(self._lib.dv_sensors_clear(self._ctx), "dv_sensors_clear")
        self.n_sensors = 0

    def sensors_info(self):
        """dict(n_sensors, pixel_dimensions int32[n, 2], masks int32[n], luts uint8[n, 3, 256]) of the live table (n = 0: none)."""
        n = ctypes.c_int(0)
        self._check(self._lib.dv_sensors_info(self._ctx, ctypes.byref(n), None, None, None, None), "dv_sensors_info")
        k = max(n.value, 1)
        pw, ph, mk = (np.zeros(k, dtype=np.int32) for _ in range(3))
        lt = np.zeros((k, 3, 256), dtype=np.uint8)
        self._check(self._lib.dv_sensors_info(self._ctx, None, pw.ctypes.data_as(N._i32p), ph.ctypes.data_as(N._i32p), mk.ctypes.data_as(N._i32p),
                                              N.u8ptr(lt)), "dv_sensors_info")
        self.n_sensors = n.value
        return dict(n_sensors=n.value, pixel_dimensions=np.stack([pw, ph], axis=1)[:n.value], masks=mk[:n.value], luts=lt[:n.value])

    # -- noise rows: a reproducible noise draw per sensing on a landscape set (include/dejavu.h: dv_noise_*) ---------------------------
    n_noise_rows = 0             # live noise rows (noise_rows; 0: every sensed call is the noiseless model)

    @staticmethod
    def _noise_args(seed, keys, amp_s, amp_v):
        """(seed, keys uint64[n], amp_s uint8[n], amp_v uint8[n]) checked, or ValueError naming the argument and the entry."""
        if isinstance(seed, (bool, float)) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise ValueError("seed must be an integer in [0, 2**64), got %r" % (seed,))
        k = np.asarray(keys)
        if k.dtype != np.uint64 or k.ndim != 1 or k.shape[0] < 1:
            raise ValueError("keys must be uint64[n] with n >= 1, got dtype %s and shape %r" % (k.dtype, k.shape))
        amps = []
        for a, what in ((amp_s, "amp_s"), (amp_v, "amp_v")):
            a = np.asarray(a)
            if a.dtype.kind not in "iu":
                raise ValueError("%s must hold integers, got dtype %s" % (what, a.dtype))
            if a.shape != k.shape:
                raise ValueError("%s must have shape %r (an amplitude per key), got %r" % (what, k.shape, a.shape))
            for i, v in enumerate(a.tolist()):
                if not 0 <= v <= 255:
                    raise ValueError("%s[%d] = %d outside [0, 255]" % (what, i, v))
            amps.append(np.ascontiguousarray(a, dtype=np.uint8))
        return int(seed), np.ascontiguousarray(k), amps[0], amps[1]

    def noise_rows(self, seed, keys, amp_s, amp_v):
        """Noise rows of the sensed calls that take a landscape table (land_of_*): row i = (keys[i], amp_s[i], amp_v[i]) belongs to
        member i of a step or scene call, or to view / pose i of a training, store or lands_sense call, which then add to the S and V
        of every sensor pixel an integer in [-amp, +amp] drawn from splitmix64 at a counter of (seed, key, heading, pixel) -- after
        the pixel block's rule, before the level tables; hue, mask and errors are the noiseless model's.  keys: uint64[n]; amplitudes:
        integers in [0, 255], one per key; seed in [0, 2**64).  Checked before any library call.  While rows are live a call whose
        landscape table has not n entries, or a sensed call without one, is refused; noise_clear ends that."""
        seed, k, s, v = self._noise_args(seed, keys, amp_s, amp_v)
        self._check(self._lib.dv_noise_rows(self._ctx, ctypes.c_uint64(seed), k.ctypes.data_as(N._u64p), N.u8ptr(s), N.u8ptr(v), len(k)),
                    "dv_noise_rows")
        self.n_noise_rows = len(k)

    def noise_clear(self):
        self._check(self._lib.dv_noise_clear(self._ctx), "dv_noise_clear")
        self.n_noise_rows = 0

    def noise_info(self):
        """dict(n_rows, seed, keys uint64[n], amp_s uint8[n], amp_v uint8[n]) of the live rows (n_rows = 0: none)."""
        n, seed = ctypes.c_int64(0), ctypes.c_uint64(0)
        self._check(self._lib.dv_noise_info(self._ctx, ctypes.byref(n), ctypes.byref(seed), None, None, None), "dv_noise_info")
        m = max(n.value, 1)
        k, s, v = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint8), np.zeros(m, dtype=np.uint8)
        self._check(self._lib.dv_noise_info(self._ctx, None, None, k.ctypes.data_as(N._u64p), N.u8ptr(s), N.u8ptr(v)), "dv_noise_info")
        self.n_noise_rows = n.value
        return dict(n_rows=n.value, seed=seed.value, keys=k[:n.value], amp_s=s[:n.value], amp_v=v[:n.value])

    # -- route view store: perfect-memory members scored on their own routes (include/dejavu.h: dv_rviews_*) ------------------------
    rviews_first = None          # int64[n_routes + 1] of the store (rviews_set_u8 / rviews_set_from_poses; None: no store)
    rviews_shape = None          # (h, w) of its views
    RVIEWS_MAX_PIXELS = 4096

    @staticmethod
    def _rviews_first(first, n):
        """`first` as int64[R + 1]: 0, ascending by at least 2, ending at n -- or ValueError naming the entry."""
        arr = np.asarray(first)
        if arr.ndim != 1 or arr.shape[0] < 2:
            raise ValueError("first must have shape (n_routes + 1,) with n_routes >= 1, got %r" % (arr.shape,))
        if arr.dtype.kind not in "iu":
            raise ValueError("first must hold integers (a route's first view), got dtype %s" % arr.dtype)
        arr = np.ascontiguousarray(arr, dtype=np.int64)
        if arr[0] != 0:
            raise ValueError("first[0] = %d, not 0" % arr[0])
        short = np.flatnonzero(np.diff(arr) < 2)
        if len(short):
            raise ValueError("first[%d] = %d: route %d would hold %d views (a route holds at least 2)"
                             % (short[0] + 1, arr[short[0] + 1], short[0], arr[short[0] + 1] - arr[short[0]]))
        if arr[-1] != n:
            raise ValueError("first[%d] = %d, but there are %d views" % (len(arr) - 1, arr[-1], n))
        return arr

    def _rviews_tables(self, n, route_of_member, chem_weights, land_of_member=None):
        """The tables of a step as (int32[n], float64[n], int32[n] or None), every entry in range -- checked before any library call."""
        if self.rviews_first is None:
            raise N.EngineError("no route views: rviews_set_u8 or rviews_set_from_poses first (DV_ERR_STATE)")
        routes = self._index_table(route_of_member, "route_of_member", len(self.rviews_first) - 1, "n_banks", n, "bank")
        w = np.asarray(chem_weights)
        if w.dtype.kind not in "fiu":
            raise ValueError("chem_weights must hold numbers, got dtype %s" % w.dtype)
        if w.shape != (n,):
            raise ValueError("chem_weights must have shape (%d,), got %r" % (n, w.shape))
        w = np.ascontiguousarray(w, dtype=np.float64)
        bad = np.flatnonzero(~((w >= 0.0) & (w <= 1.0)))
        if len(bad):
            raise ValueError("chem_weights[%d] = %r outside [0, 1]" % (bad[0], float(w[bad[0]])))
        lands = None if land_of_member is None else self._land_table(land_of_member, n, "land_of_member")
        return routes, w, lands

    def rviews_set_u8(self, views, first):
        """views: uint8[n, h, w, 3], route r = views[first[r]:first[r + 1]]: the store of the routes' views, for tests without a sensor."""
        views = N.as_u8(views, "views")
        if views.ndim != 4 or views.shape[3] != 3 or views.shape[1] < 1 or views.shape[2] < 1:
            raise ValueError("views must be uint8[n, h, w, 3], got shape %r" % (views.shape,))
        if views.shape[1] * views.shape[2] > self.RVIEWS_MAX_PIXELS:
            raise ValueError("views of %d x %d: h * w must be <= %d" % (views.shape[1], views.shape[2], self.RVIEWS_MAX_PIXELS))
        first = self._rviews_first(first, views.shape[0])
        self._check(self._lib.dv_rviews_set_u8(self._ctx, N.u8ptr(views), N.i64ptr(first), len(first) - 1, views.shape[1], views.shape[2]),
                    "dv_rviews_set_u8")
        self.rviews_first, self.rviews_shape = first, (views.shape[1], views.shape[2])

    def rviews_set_from_poses(self, x, y, angle, first, land_of_view=None, want_views=True):
        """Senses the views of all routes in one call into the store (view v on landscape land_of_view[v] of the live set; None: on the
        engine's landscape); returns them (uint8[n, h, w, 3]) when want_views.  IndexError names the first view whose footprint leaves
        its own landscape, and the store stays as it was."""
        x, y, angle = self._pose_arrays(x, y, angle)
        first = self._rviews_first(first, len(x))
        lands = None if land_of_view is None else self._land_table(land_of_view, len(x), "land_of_view")
        h, w = self.sensor_shape
        views = np.empty((len(x), h, w, 3), dtype=np.uint8) if want_views else None
        self._check_sense(self._lib.dv_rviews_set_from_poses(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angle), len(x), N.i64ptr(first),
                                                             len(first) - 1, None if lands is None else lands.ctypes.data_as(N._i32p),
                                                             N.u8ptr(views) if want_views else None), "dv_rviews_set_from_poses")
        self.rviews_first, self.rviews_shape = first, (h, w)
        return views

    def rviews_clear(self):
        self._check(self._lib.dv_rviews_clear(self._ctx), "dv_rviews_clear")
        self.rviews_first = self.rviews_shape = None

    def rviews_info(self):
        """dict(n_routes, first int64[n_routes + 1], shape (h, w), bytes)."""
        nr, h, w, nbytes = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
        self._check(self._lib.dv_rviews_info(self._ctx, ctypes.byref(nr), None, ctypes.byref(h), ctypes.byref(w), ctypes.byref(nbytes)),
                    "dv_rviews_info")
        first = np.zeros(nr.value + 1, dtype=np.int64)
        if nr.value:
            self._check(self._lib.dv_rviews_info(self._ctx, None, N.i64ptr(first), None, None, None), "dv_rviews_info")
        return dict(n_routes=nr.value, first=first, shape=(h.value, w.value), bytes=nbytes.value)

    def _rviews_patches(self, patches):
        patches = N.as_u8(patches, "patches")
        if self.rviews_first is None:
            raise N.EngineError("no route views: rviews_set_u8 or rviews_set_from_poses first (DV_ERR_STATE)")
        if patches.ndim != 5 or patches.shape[0] < 1 or patches.shape[1] < 1 or patches.shape[2:] != self.rviews_shape + (3,):
            raise ValueError("patches must be uint8[n, A, %d, %d, 3] with n, A >= 1, got shape %r" % (self.rviews_shape + (patches.shape,)))
        return patches

    def rviews_step_u8(self, patches, route_of_member, chem_weights, exact=False):
        """patches: uint8[n, A, h, w, 3]; member i is scored against the views of route route_of_member[i] under chem_weights[i] ->
        RouteViewResults: angle_familiarity[n, A] (the reference's bits), angle_view[n, A] (the first view of the route that attains
        it), best_idex[n] (np.argmax of the row), flags[n]."""
        patches = self._rviews_patches(patches)
        n, A = patches.shape[:2]
        routes, w, _ = self._rviews_tables(n, route_of_member, chem_weights)
        fam, best, flags = self._member_results(n, A)
        view = np.empty((n, A), dtype=np.int64)
        self._check(self._lib.dv_rviews_step_u8(self._ctx, N.u8ptr(patches), n, A, routes.ctypes.data_as(N._i32p), N.f64ptr(w),
                                                N.DV_RVIEWS_EXACT if exact else 0, N.f64ptr(fam), N.i64ptr(view), best.ctypes.data_as(N._i32p)),
                    "dv_rviews_step_u8")
        return RouteViewResults(fam, view, best, flags)

    def rviews_sense_step(self, x, y, angles, route_of_member, chem_weights, land_of_member=None, exact=False):
        """rviews_step_u8 with member i's patches sensed at (x[i], y[i]) along angles[i] (on landscape land_of_member[i] of the live
        set): one enqueue and one wait.  flags[i] carries DV_RES_SENSE_ERROR = 16 for a member whose footprint leaves its landscape."""
        x, y, angles = self._member_poses(x, y, angles)
        n, A = angles.shape
        routes, w, lands = self._rviews_tables(n, route_of_member, chem_weights, land_of_member)
        fam, best, flags = self._member_results(n, A)
        view = np.empty((n, A), dtype=np.int64)
        self._check(self._lib.dv_rviews_sense_step(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angles), n, A, routes.ctypes.data_as(N._i32p),
                                                   N.f64ptr(w), None if lands is None else lands.ctypes.data_as(N._i32p),
                                                   N.DV_RVIEWS_EXACT if exact else 0, N.f64ptr(fam), N.i64ptr(view),
                                                   best.ctypes.data_as(N._i32p), flags.ctypes.data_as(N._u32p)), "dv_rviews_sense_step")
        return RouteViewResults(fam, view, best, flags)

    # -- windowed steps on the store: perfect memory with a temporal window (include/dejavu.h: dv_rvwin_*) ---------------------------
    RVWIN_MAX_VIEWS = N.DV_RVWIN_MAX_VIEWS

    def _rvwin_windows(self, routes, win_lo, win_hi):
        """The windows of a step as two int32[n]: member i's [win_lo[i], win_hi[i]) holds 1 to RVWIN_MAX_VIEWS views of its route --
        or ValueError naming the member.  Checked before any library call."""
        n = len(routes)
        out = []
        for what, arr in (("win_lo", win_lo), ("win_hi", win_hi)):
            arr = np.asarray(arr)
            if arr.dtype.kind not in "iu":
                raise ValueError("%s must hold integers (a view of the member's route per entry), got dtype %s" % (what, arr.dtype))
            if arr.shape != (n,):
                raise ValueError("%s must have shape (%d,), got %r" % (what, n, arr.shape))
            out.append(arr.astype(np.int64))
        lo, hi = out
        lens = np.diff(self.rviews_first)[routes]
        bad = np.flatnonzero((lo < 0) | (lo >= hi) | (hi > lens) | (hi - lo > self.RVWIN_MAX_VIEWS))
        if len(bad):
            i = int(bad[0])
            raise ValueError("member %d: window [%d, %d) must hold 1 to %d views within its route %d of %d views"
                             % (i, lo[i], hi[i], self.RVWIN_MAX_VIEWS, routes[i], lens[i]))
        return np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(hi, dtype=np.int32)

    @staticmethod
    def _rvwin_thresholds(reloc_below, n):
        """reloc_below of a step as float64[n] (None: None), no NaN -- checked before any library call."""
        if reloc_below is None:
            return None
        t = np.asarray(reloc_below)
        if t.dtype.kind not in "fiu":
            raise ValueError("reloc_below must hold numbers (a familiarity per member; -inf: never), got dtype %s" % t.dtype)
        if t.shape != (n,):
            raise ValueError("reloc_below must have shape (%d,), got %r" % (n, t.shape))
        t = np.ascontiguousarray(t, dtype=np.float64)
        bad = np.flatnonzero(np.isnan(t))
        if len(bad):
            raise ValueError("member %d: reloc_below is NaN" % bad[0])
        return t

    def rvwin_step_u8(self, patches, route_of_member, chem_weights, win_lo, win_hi, exact=False, reloc_below=None):
        """rviews_step_u8 with member i scored against views [win_lo[i], win_hi[i]) of its route only (at most RVWIN_MAX_VIEWS), in one
        fused scoring launch -> RouteViewResults: what the unwindowed step gives on that slice of the route, angle_view counted from
        the route's first view.  reloc_below (float64[n]; None: the call as it ever was): member i whose largest windowed
        angle_familiarity is < reloc_below[i] is lost, and its row is rviews_step_u8's on its whole route, in the same enqueue
        (dv_rvreloc_step_u8); results.relocalised says which."""
        patches = self._rviews_patches(patches)
        n, A = patches.shape[:2]
        routes, w, _ = self._rviews_tables(n, route_of_member, chem_weights)
        lo, hi = self._rvwin_windows(routes, win_lo, win_hi)
        tau = self._rvwin_thresholds(reloc_below, n)
        fam, best, flags = self._member_results(n, A)
        view = np.empty((n, A), dtype=np.int64)
        if tau is not None:
            self._check(self._lib.dv_rvreloc_step_u8(self._ctx, N.u8ptr(patches), n, A, routes.ctypes.data_as(N._i32p), N.f64ptr(w),
                                                     lo.ctypes.data_as(N._i32p), hi.ctypes.data_as(N._i32p), N.f64ptr(tau),
                                                     N.DV_RVIEWS_EXACT if exact else 0, N.f64ptr(fam), N.i64ptr(view),
                                                     best.ctypes.data_as(N._i32p), flags.ctypes.data_as(N._u32p)), "dv_rvreloc_step_u8")
            return RouteViewResults(fam, view, best, flags)
        self._check(self._lib.dv_rvwin_step_u8(self._ctx, N.u8ptr(patches), n, A, routes.ctypes.data_as(N._i32p), N.f64ptr(w),
                                               lo.ctypes.data_as(N._i32p), hi.ctypes.data_as(N._i32p), N.DV_RVIEWS_EXACT if exact else 0,
                                               N.f64ptr(fam), N.i64ptr(view), best.ctypes.data_as(N._i32p)), "dv_rvwin_step_u8")
        return RouteViewResults(fam, view, best, flags)

    def rvwin_sense_step(self, x, y, angles, route_of_member, chem_weights, win_lo, win_hi, land_of_member=None, exact=False,
                         reloc_below=None):
        """rvwin_step_u8 with the patches sensed as rviews_sense_step senses them: one enqueue and one wait (with reloc_below too:
        dv_rvreloc_sense_step; a member flagged DV_RES_SENSE_ERROR is never lost)."""
        x, y, angles = self._member_poses(x, y, angles)
        n, A = angles.shape
        routes, w, lands = self._rviews_tables(n, route_of_member, chem_weights, land_of_member)
        lo, hi = self._rvwin_windows(routes, win_lo, win_hi)
        tau = self._rvwin_thresholds(reloc_below, n)
        fam, best, flags = self._member_results(n, A)
        view = np.empty((n, A), dtype=np.int64)
        if tau is not None:
            self._check(self._lib.dv_rvreloc_sense_step(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angles), n, A,
                                                        routes.ctypes.data_as(N._i32p), N.f64ptr(w),
                                                        None if lands is None else lands.ctypes.data_as(N._i32p), lo.ctypes.data_as(N._i32p),
                                                        hi.ctypes.data_as(N._i32p), N.f64ptr(tau), N.DV_RVIEWS_EXACT if exact else 0,
                                                        N.f64ptr(fam), N.i64ptr(view), best.ctypes.data_as(N._i32p),
                                                        flags.ctypes.data_as(N._u32p)), "dv_rvreloc_sense_step")
            return RouteViewResults(fam, view, best, flags)
        self._check(self._lib.dv_rvwin_sense_step(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angles), n, A, routes.ctypes.data_as(N._i32p),
                                                  N.f64ptr(w), None if lands is None else lands.ctypes.data_as(N._i32p),
                                                  lo.ctypes.data_as(N._i32p), hi.ctypes.data_as(N._i32p), N.DV_RVIEWS_EXACT if exact else 0,
                                                  N.f64ptr(fam), N.i64ptr(view), best.ctypes.data_as(N._i32p), flags.ctypes.data_as(N._u32p)),
                    "dv_rvwin_sense_step")
        return RouteViewResults(fam, view, best, flags)

    def _rviews_rows(self, routes):
        lens = np.diff(self.rviews_first)[routes]
        return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)

    def rviews_scene_u8(self, patches, route_of_member, chem_weights):
        """scene_familiarity of every member -> a list of float64[len(route of member i)]: per view the least value over the headings."""
        patches = self._rviews_patches(patches)
        n, A = patches.shape[:2]
        routes, w, _ = self._rviews_tables(n, route_of_member, chem_weights)
        row0 = self._rviews_rows(routes)
        out = np.empty(row0[-1], dtype=np.float64)
        self._check(self._lib.dv_rviews_scene_u8(self._ctx, N.u8ptr(patches), n, A, routes.ctypes.data_as(N._i32p), N.f64ptr(w), len(out),
                                                 N.f64ptr(out)), "dv_rviews_scene_u8")
        return [out[row0[i]:row0[i + 1]] for i in range(n)]

    def rviews_scene(self, x, y, angles, route_of_member, chem_weights, land_of_member=None, want_flags=False):
        """rviews_scene_u8 with the patches sensed as rviews_sense_step senses them; a member whose footprint leaves its landscape gets
        a row of +inf and DV_RES_SENSE_ERROR = 16 in its flag.  want_flags: returns (rows, flags uint32[n])."""
        x, y, angles = self._member_poses(x, y, angles)
        n, A = angles.shape
        routes, w, lands = self._rviews_tables(n, route_of_member, chem_weights, land_of_member)
        row0 = self._rviews_rows(routes)
        out = np.empty(row0[-1], dtype=np.float64)
        flags = np.zeros(n, dtype=np.uint32)
        self._check(self._lib.dv_rviews_scene(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angles), n, A, routes.ctypes.data_as(N._i32p),
                                              N.f64ptr(w), None if lands is None else lands.ctypes.data_as(N._i32p), len(out), N.f64ptr(out),
                                              flags.ctypes.data_as(N._u32p)), "dv_rviews_scene")
        rows = [out[row0[i]:row0[i + 1]] for i in range(n)]
        return (rows, flags) if want_flags else rows

    # -- SSD on the store: exact ssds of one channel on the int8 matrix cores (include/dejavu.h: dv_rvssd_*) ------------------------
    def _rvssd_tables(self, n, route_of_member, channel, land_of_member=None):
        """The tables of an SSD call as (int32[n], channel, int32[n] or None) -- checked before any library call."""
        if self.rviews_first is None:
            raise N.EngineError("no route views: rviews_set_u8 or rviews_set_from_poses first (DV_ERR_STATE)")
        if isinstance(channel, bool) or not isinstance(channel, (int, np.integer)) or not 0 <= channel <= 2:
            raise ValueError("channel must be 0, 1 or 2 (H, S or V), got %r" % (channel,))
        routes = self._index_table(route_of_member, "route_of_member", len(self.rviews_first) - 1, "n_banks", n, "bank")
        lands = None if land_of_member is None else self._land_table(land_of_member, n, "land_of_member")
        return routes, int(channel), lands

    def rvssd_step_u8(self, patches, route_of_member, channel=2):
        """patches: uint8[n, A, h, w, 3]; member i's channel `channel` is scored as the reference's ssds against the views of route
        route_of_member[i] -> RouteSsdResults: angle_ssd[n, A] (exact integers as float64), angle_view[n, A] (the least view of the
        route that attains it), best_idex[n] (the first least heading), flags[n], angle_familiarity = -angle_ssd."""
        patches = self._rviews_patches(patches)
        n, A = patches.shape[:2]
        routes, channel, _ = self._rvssd_tables(n, route_of_member, channel)
        ssd, best, flags = self._member_results(n, A)
        view = np.empty((n, A), dtype=np.int64)
        self._check(self._lib.dv_rvssd_step_u8(self._ctx, N.u8ptr(patches), n, A, routes.ctypes.data_as(N._i32p), channel, N.f64ptr(ssd),
                                               N.i64ptr(view), best.ctypes.data_as(N._i32p)), "dv_rvssd_step_u8")
        return RouteSsdResults(ssd, view, best, flags)

    def rvssd_sense_step(self, x, y, angles, route_of_member, channel=2, land_of_member=None):
        """rvssd_step_u8 with member i's patches sensed at (x[i], y[i]) along angles[i] (on landscape land_of_member[i] of the live
        set): one enqueue and one wait.  flags[i] carries DV_RES_SENSE_ERROR = 16 for a member whose footprint leaves its landscape."""
        x, y, angles = self._member_poses(x, y, angles)
        n, A = angles.shape
        routes, channel, lands = self._rvssd_tables(n, route_of_member, channel, land_of_member)
        ssd, best, flags = self._member_results(n, A)
        view = np.empty((n, A), dtype=np.int64)
        self._check(self._lib.dv_rvssd_sense_step(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angles), n, A, routes.ctypes.data_as(N._i32p),
                                                  None if lands is None else lands.ctypes.data_as(N._i32p), channel, N.f64ptr(ssd),
                                                  N.i64ptr(view), best.ctypes.data_as(N._i32p), flags.ctypes.data_as(N._u32p)),
                    "dv_rvssd_sense_step")
        return RouteSsdResults(ssd, view, best, flags)

    def rvssdw_step_u8(self, patches, route_of_member, win_lo, win_hi, channel=2, reloc_below=None):
        """rvssd_step_u8 with member i scored against views [win_lo[i], win_hi[i]) of its route only (at most RVWIN_MAX_VIEWS), in one
        scoring launch -> RouteSsdResults: what the unwindowed step gives on that slice of the route, angle_view counted from the
        route's first view.  reloc_below (float64[n], in the unit of angle_familiarity = -SSD; None: no loss test): member i whose
        largest windowed angle_familiarity is < reloc_below[i] is lost, and its row is rvssd_step_u8's on its whole route, in the same
        enqueue; results.relocalised says which."""
        patches = self._rviews_patches(patches)
        n, A = patches.shape[:2]
        routes, channel, _ = self._rvssd_tables(n, route_of_member, channel)
        lo, hi = self._rvwin_windows(routes, win_lo, win_hi)
        tau = self._rvwin_thresholds(reloc_below, n)
        ssd, best, flags = self._member_results(n, A)
        view = np.empty((n, A), dtype=np.int64)
        self._check(self._lib.dv_rvssdw_step_u8(self._ctx, N.u8ptr(patches), n, A, routes.ctypes.data_as(N._i32p), lo.ctypes.data_as(N._i32p),
                                                hi.ctypes.data_as(N._i32p), None if tau is None else N.f64ptr(tau), channel, N.f64ptr(ssd),
                                                N.i64ptr(view), best.ctypes.data_as(N._i32p), flags.ctypes.data_as(N._u32p)),
                    "dv_rvssdw_step_u8")
        return RouteSsdResults(ssd, view, best, flags)

    def rvssdw_sense_step(self, x, y, angles, route_of_member, win_lo, win_hi, channel=2, land_of_member=None, reloc_below=None):
        """rvssdw_step_u8 with the patches sensed as rvssd_sense_step senses them: one enqueue and one wait, with reloc_below too (a
        member flagged DV_RES_SENSE_ERROR is never lost)."""
        x, y, angles = self._member_poses(x, y, angles)
        n, A = angles.shape
        routes, channel, lands = self._rvssd_tables(n, route_of_member, channel, land_of_member)
        lo, hi = self._rvwin_windows(routes, win_lo, win_hi)
        tau = self._rvwin_thresholds(reloc_below, n)
        ssd, best, flags = self._member_results(n, A)
        view = np.empty((n, A), dtype=np.int64)
        self._check(self._lib.dv_rvssdw_sense_step(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angles), n, A, routes.ctypes.data_as(N._i32p),
                                                   None if lands is None else lands.ctypes.data_as(N._i32p), lo.ctypes.data_as(N._i32p),
                                                   hi.ctypes.data_as(N._i32p), None if tau is None else N.f64ptr(tau), channel, N.f64ptr(ssd),
                                                   N.i64ptr(view), best.ctypes.data_as(N._i32p), flags.ctypes.data_as(N._u32p)),
                    "dv_rvssdw_sense_step")
        return RouteSsdResults(ssd, view, best, flags)

    def rvssd_scene_u8(self, patches, route_of_member, channel=2):
        """Per member a float64[len(its route)]: per view the largest ssds over the headings (its negative is scene_familiarity)."""
        patches = self._rviews_patches(patches)
        n, A = patches.shape[:2]
        routes, channel, _ = self._rvssd_tables(n, route_of_member, channel)
        row0 = self._rviews_rows(routes)
        out = np.empty(row0[-1], dtype=np.float64)
        self._check(self._lib.dv_rvssd_scene_u8(self._ctx, N.u8ptr(patches), n, A, routes.ctypes.data_as(N._i32p), channel, len(out),
                                                N.f64ptr(out)), "dv_rvssd_scene_u8")
        return [out[row0[i]:row0[i + 1]] for i in range(n)]

    def rvssd_scene(self, x, y, angles, route_of_member, channel=2, land_of_member=None, want_flags=False):
        """rvssd_scene_u8 with the patches sensed as rvssd_sense_step senses them; a member whose footprint leaves its landscape gets
        a row of -inf and DV_RES_SENSE_ERROR = 16 in its flag.  want_flags: returns (rows, flags uint32[n])."""
        x, y, angles = self._member_poses(x, y, angles)
        n, A = angles.shape
        routes, channel, lands = self._rvssd_tables(n, route_of_member, channel, land_of_member)
        row0 = self._rviews_rows(routes)
        out = np.empty(row0[-1], dtype=np.float64)
        flags = np.zeros(n, dtype=np.uint32)
        self._check(self._lib.dv_rvssd_scene(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angles), n, A, routes.ctypes.data_as(N._i32p),
                                             None if lands is None else lands.ctypes.data_as(N._i32p), channel, len(out), N.f64ptr(out),
                                             flags.ctypes.data_as(N._u32p)), "dv_rvssd_scene")
        rows = [out[row0[i]:row0[i + 1]] for i in range(n)]
        return (rows, flags) if want_flags else rows

    # -- NCC on the store: the correlation coefficient of one channel, SSD's GEMM and a 64-bit epilogue (include/dejavu.h: dv_rvncc_*) --
    def rvncc_step_u8(self, patches, route_of_member, channel=2):
        """patches: uint8[n, A, h, w, 3]; member i's channel `channel` is scored by the correlation coefficient against the views of
        route route_of_member[i] -> RouteNccResults: angle_ncc[n, A] (in [-1, 1]; 0.0 where a plane is constant), angle_view[n, A] (the
        least view of the route that attains it), best_idex[n] (the first largest heading), flags[n]."""
        patches = self._rviews_patches(patches)
        n, A = patches.shape[:2]
        routes, channel, _ = self._rvssd_tables(n, route_of_member, channel)
        ncc, best, flags = self._member_results(n, A)
        view = np.empty((n, A), dtype=np.int64)
        self._check(self._lib.dv_rvncc_step_u8(self._ctx, N.u8ptr(patches), n, A, routes.ctypes.data_as(N._i32p), channel, N.f64ptr(ncc),
                                               N.i64ptr(view), best.ctypes.data_as(N._i32p)), "dv_rvncc_step_u8")
        return RouteNccResults(ncc, view, best, flags)

    def rvncc_sense_step(self, x, y, angles, route_of_member, channel=2, land_of_member=None):
        """rvncc_step_u8 with member i's patches sensed at (x[i], y[i]) along angles[i] (on landscape land_of_member[i] of the live
        set): one enqueue and one wait.  flags[i] carries DV_RES_SENSE_ERROR = 16 for a member whose footprint leaves its landscape."""
        x, y, angles = self._member_poses(x, y, angles)
        n, A = angles.shape
        routes, channel, lands = self._rvssd_tables(n, route_of_member, channel, land_of_member)
        ncc, best, flags = self._member_results(n, A)
        view = np.empty((n, A), dtype=np.int64)
        self._check(self._lib.dv_rvncc_sense_step(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angles), n, A, routes.ctypes.data_as(N._i32p),
                                                  None if lands is None else lands.ctypes.data_as(N._i32p), channel, N.f64ptr(ncc),
                                                  N.i64ptr(view), best.ctypes.data_as(N._i32p), flags.ctypes.data_as(N._u32p)),
                    "dv_rvncc_sense_step")
        return RouteNccResults(ncc, view, best, flags)

    def rvncc_scene_u8(self, patches, route_of_member, channel=2):
        """Per member a float64[len(its route)]: per view the least correlation coefficient over the headings (scene_familiarity)."""
        patches = self._rviews_patches(patches)
        n, A = patches.shape[:2]
        routes, channel, _ = self._rvssd_tables(n, route_of_member, channel)
        row0 = self._rviews_rows(routes)
        out = np.empty(row0[-1], dtype=np.float64)
        self._check(self._lib.dv_rvncc_scene_u8(self._ctx, N.u8ptr(patches), n, A, routes.ctypes.data_as(N._i32p), channel, len(out),
                                                N.f64ptr(out)), "dv_rvncc_scene_u8")
        return [out[row0[i]:row0[i + 1]] for i in range(n)]

    def rvncc_scene(self, x, y, angles, route_of_member, channel=2, land_of_member=None, want_flags=False):
        """rvncc_scene_u8 with the patches sensed as rvncc_sense_step senses them; a member whose footprint leaves its landscape gets
        a row of +inf and DV_RES_SENSE_ERROR = 16 in its flag.  want_flags: returns (rows, flags uint32[n])."""
        x, y, angles = self._member_poses(x, y, angles)
        n, A = angles.shape
        routes, channel, lands = self._rvssd_tables(n, route_of_member, channel, land_of_member)
        row0 = self._rviews_rows(routes)
        out = np.empty(row0[-1], dtype=np.float64)
        flags = np.zeros(n, dtype=np.uint32)
        self._check(self._lib.dv_rvncc_scene(self._ctx, N.f64ptr(x), N.f64ptr(y), N.f64ptr(angles), n, A, routes.ctypes.data_as(N._i32p),
                                             None if lands is None else lands.ctypes.data_as(N._i32p), channel, len(out), N.f64ptr(out),
                                             flags.ctypes.data_as(N._u32p)), "dv_rvncc_scene")
        rows = [out[row0[i]:row0[i + 1]] for i in range(n)]
        return (rows, flags) if want_flags else rows
