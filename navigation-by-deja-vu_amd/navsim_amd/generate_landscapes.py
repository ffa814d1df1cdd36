"""Landscape generators of the reference (navsim/generate_landscapes.py, navsim/util.pyx:189-235) with the heat equation on the GPU.

    from navsim_amd.generate_landscapes import *        # was: from navsim.generate_landscapes import *

`diffuse` runs on the device through libdejavu_hip.so (include/dejavu.h: dv_diffuse_*) and returns the reference's bits;
`diffuse_series` produces the snapshots of several diffusion times from ONE run instead of starting at step 0 for each
(what scripts/generate_landscapes.py does with its loop).  The small generators `random_squares`,
`random_matrix_bw_balance`, `checkerboard` and `image_from_prob_mat` are host NumPy under the reference's names and
signatures and draw from Python's and NumPy's global random state as the reference does.

Not here: `random_squares_rot`, which rotates its squares with scikit-image (skimage.transform.rotate); this package does
not depend on scikit-image.

There is no CPU fallback for `diffuse`: without the HIP library or a GPU it raises (only `nstep == 0`, which returns its
argument untouched, needs neither).
"""
import ctypes
import random

import numpy as np

from . import _native as N

_FORMS = {"auto": N.DV_DIFFUSE_AUTO, "plain": N.DV_DIFFUSE_PLAIN, "blocked": N.DV_DIFFUSE_BLOCKED}


class DiffuseRun:
    """One dv_ctx with a float64 field on it: begin at construction, advance / read on request, end + destroy at close.
    `window` (64 or 96) and `steps_per_launch` choose the blocked form's shape for an A/B (dv_diffuse_configure); None keeps
    the default.  What diffuse / diffuse_series are made of, and what tools/diffuse_time.py times."""

    def __init__(self, field, c=1.0, delta_t_factor=0.5, device=0, window=None, steps_per_launch=None):
        self._lib = N.load()
        self._ctx = ctypes.c_void_p()
        rc = self._lib.dv_create(ctypes.byref(self._ctx), int(device))
        if rc != 0:
            self._ctx = None
            raise N.EngineError("dv_create(device=%d) failed: %s (%s)" % (
                device, N.ERROR_NAMES.get(rc, rc), self._lib.dv_last_error(None).decode(errors="replace")))
        self._args = (float(c), float(delta_t_factor))
        try:
            if window is not None or steps_per_launch is not None:
                self._check(self._lib.dv_diffuse_configure(self._ctx, int(window or 0), int(steps_per_launch or 0)),
                            "dv_diffuse_configure")
            self.restart(field)
        except Exception:
            self.close()
            raise

    def restart(self, field):
        """Replace the field (a C-contiguous float64 square); the step count starts again at 0."""
        self.n = field.shape[0]
        self._check(self._lib.dv_diffuse_begin(self._ctx, N.f64ptr(field), self.n, *self._args), "dv_diffuse_begin")

    def timed_advance(self, nstep, form="auto"):
        """advance() between a hipEvent pair on the context's stream; returns the milliseconds (waits for the launches)."""
        ms = ctypes.c_float()
        self._check(self._lib.dv_timer_start(self._ctx), "dv_timer_start")
        self.advance(nstep, form)
        self._check(self._lib.dv_timer_stop(self._ctx, ctypes.byref(ms)), "dv_timer_stop")
        return ms.value

    def _check(self, rc, what):
        if rc != 0:
            raise N.EngineError("%s failed: %s (%s)" % (what, N.ERROR_NAMES.get(rc, rc),
                                                       self._lib.dv_last_error(self._ctx).decode(errors="replace")))

    def advance(self, nstep, form="auto"):
        self._check(self._lib.dv_diffuse_advance(self._ctx, int(nstep), _FORMS[form]), "dv_diffuse_advance")

    def read(self):
        out = np.empty((self.n, self.n), dtype=np.float64)
        self._check(self._lib.dv_diffuse_read(self._ctx, N.f64ptr(out)), "dv_diffuse_read")
        return out

    def info(self):
        tile, steps, done = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._check(self._lib.dv_diffuse_info(self._ctx, ctypes.byref(tile), ctypes.byref(steps), ctypes.byref(done)),
                    "dv_diffuse_info")
        return dict(tile=tile.value, steps_per_launch=steps.value, steps_done=done.value)

    def close(self):
        if self._ctx is not None:
            self._lib.dv_diffuse_end(self._ctx)
            self._lib.dv_destroy(self._ctx)
            self._ctx = None


def diffuse_info(device=0):
    """{tile, steps_per_launch, steps_done} of the blocked form on `device` (dv_diffuse_info)."""
    run = DiffuseRun(np.zeros((1, 1)), 1.0, 0.5, device)
    try:
        return run.info()
    finally:
        run.close()


def _prepare(initial_condition, c, form):
    """The float64 copy the device starts from; the reference's shape assertion (util.pyx:203) comes before any device call."""
    if form not in _FORMS:
        raise ValueError("form must be one of %s, got %r" % (sorted(_FORMS), form))
    shape = np.shape(initial_condition)
    assert len(shape) == 2 and shape[0] == shape[1]
    if float(c) == 0.0:
        raise ZeroDivisionError("float division")                      # util.pyx:207 divides by 2 * c
    return np.ascontiguousarray(initial_condition, dtype=np.float64)


def _sanity_check(result, initial_condition):
    """util.pyx:229-233, the same four NumPy expressions on the same two arrays (the ORIGINAL input, whatever its dtype)."""
    assert np.sum(result) - np.sum(initial_condition) < 0.0000001
    assert np.max(result) <= np.max(initial_condition)
    assert np.min(result) >= np.min(initial_condition)
    assert not np.any(np.isnan(result))


def diffuse(initial_condition, nstep, c=1.0, delta_t_factor=0.5, device=0, form="auto"):
    """`nstep` explicit five-point sweeps of the periodic heat equation on a square field, computed on the GPU.

    The reference's contract (navsim/util.pyx:189-235): `nstep == 0` returns the argument itself; otherwise a square 2-D
    input of any real dtype (contiguous or not) is taken as float64 and advanced `nstep` steps on the GPU, the result is
    checked against the input as the reference checks it (AssertionError when the sum grew, the range widened or a NaN
    appeared: an unstable `delta_t_factor`, or a float32 input whose own sum is not the float64 one) and returned as a new
    float64 array, bit-identical to the reference's.  `form` forces a kernel form ("plain", "blocked"); all give the same bits."""
    nstep = int(nstep)
    if nstep == 0:
        return initial_condition
    if nstep < 0:
        raise ValueError("nstep must not be negative")
    field = _prepare(initial_condition, c, form)
    run = DiffuseRun(field, c, delta_t_factor, device)
    try:
        run.advance(nstep, form)
        result = run.read()
    finally:
        run.close()
    _sanity_check(result, initial_condition)
    return result


def diffuse_series(initial_condition, times, c=1.0, delta_t_factor=0.5, device=0, form="auto", info=None):
    """[diffuse(initial_condition, t) for t in times], bit for bit, from ONE run that advances through the sorted times
    instead of starting at step 0 for each.  `times` may come in any order and repeat; an entry 0 yields the argument itself,
    as `diffuse` does; every snapshot gets the reference's four checks.  `info`, when a dict, receives the run's
    {tile, steps_per_launch, steps_done} at its end."""
    times = [int(t) for t in times]
    if any(t < 0 for t in times):
        raise ValueError("diffusion times must not be negative")
    later = sorted(set(t for t in times if t > 0))
    shots = {0: initial_condition}
    if later:
        field = _prepare(initial_condition, c, form)
        run = DiffuseRun(field, c, delta_t_factor, device)
        try:
            done = 0
            for t in later:
                run.advance(t - done, form)
                done = t
                shots[t] = run.read()
                _sanity_check(shots[t], initial_condition)
            if info is not None:
                info.update(run.info())
        finally:
            run.close()
    return [shots[t] for t in times]


def random_squares(shape, s, n, value=1):
    """Integer zeros of `shape` with `n` axis-aligned s x s blocks set to `value`.

    A block's centre is drawn with `random.randrange` (Python's global generator), first the row then the column, the
    draw order scripts seeded with `random.seed` rely on.  `s` must be even.  A block reaching past the last row or column
    is cut off there; one reaching before row or column 0 has a negative slice start, which NumPy counts from the far
    end -- that block usually comes out empty, as it does in the reference."""
    if s % 2:
        raise AssertionError("random_squares: the block side s must be even, got %r" % (s,))
    rows, cols = shape[0], shape[1]
    half = s // 2
    field = np.zeros(shape, dtype=int)
    for _ in range(n):
        r = random.randrange(0, rows)
        q = random.randrange(0, cols)
        field[r - half:r + half, q - half:q + half] = value
    return field


def random_matrix_bw_balance(shape, proportion=0.5, threshold=0.06, max_iter=100, func=random_squares, **kwargs):
    """Calls `func(shape, **kwargs)` until the mean of its result lies strictly within `threshold` of `proportion` and
    returns that result; RuntimeError after `max_iter` misses.  Both `proportion` and `threshold` lie strictly in (0, 1)."""
    if not (0 < threshold < 1 and 0 < proportion < 1):
        raise AssertionError("random_matrix_bw_balance: proportion and threshold must lie strictly between 0 and 1")
    cells = shape[0] * shape[1]
    low, high = proportion - threshold, proportion + threshold
    attempt = 0
    while attempt < max_iter:
        attempt += 1
        candidate = func(shape, **kwargs)
        if low < np.sum(candidate) / cells < high:
            return candidate
    raise RuntimeError("random_matrix_bw_balance: no matrix within %g of proportion %g in %d attempts" % (threshold, proportion, max_iter))


def checkerboard(shape, checkersize):
    """float64 board of side `shape` made of checkersize x checkersize fields: 1.0 where the field's row and column numbers
    have the same parity (so the top-left field is 1.0), else 0.0."""
    field_of = np.arange(shape) // checkersize
    same_parity = (field_of[:, None] + field_of[None, :]) % 2 == 0
    return same_parity.astype(np.float64)


def image_from_prob_mat(prob_mat):
    """One Bernoulli draw per cell: 1.0 with the cell's probability, else 0.0 (float64), from a single
    `np.random.random` call of the matrix's shape on NumPy's global generator."""
    prob_mat = np.asarray(prob_mat)
    return (np.random.random(prob_mat.shape) < prob_mat).astype(np.float64)
