"""GPU tests of the device heat equation (csrc/dejavu_diffuse.inl, navsim_amd/generate_landscapes.py): both kernel forms carry
the reference's bits -- against the reference's recorded outputs (tests/golden/t8_diffuse.*) and, for the shapes around the
blocked form's tile and steps per launch, against the NumPy restatement that tests/test_diffuse_host.py holds to the same
fixtures."""
import ctypes
import json
import os

import numpy as np
import pytest

from navsim_amd import _native as N
from navsim_amd import generate_landscapes as G
from tests import helpers_diffuse as H
from tests.helpers import kernel_case_inputs

pytestmark = pytest.mark.gpu

FORMS = ("auto", "plain", "blocked")
CASES = H.fixture_cases()


@pytest.fixture(scope="module")
def ctx():
    lib = N.load()
    c = N._ctx_p()
    assert lib.dv_create(ctypes.byref(c), 0) == 0
    yield lib, c
    lib.dv_destroy(c)


@pytest.fixture(scope="module")
def shape(ctx):
    lib, c = ctx
    tile, steps, done = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(-1)
    assert lib.dv_diffuse_info(c, ctypes.byref(tile), ctypes.byref(steps), ctypes.byref(done)) == 0
    assert tile.value >= 8 and steps.value >= 2 and done.value == 0
    return tile.value, steps.value


def one_shot(ctx, a, nstep, form, c=1.0, factor=0.5):
    lib, cx = ctx
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.full(a.shape, np.nan)
    rc = lib.dv_diffuse(cx, N.f64ptr(a), a.shape[0], nstep, c, factor, G._FORMS[form], N.f64ptr(out))
    assert rc == 0, lib.dv_last_error(cx)
    return out


@pytest.mark.parametrize("case,a,want", CASES, ids=[c["key"] for c, _, _ in CASES])
def test_fixture_cases_bit_equal_in_every_form(case, a, want):
    for form in FORMS:
        if want is None:
            with pytest.raises(AssertionError):
                G.diffuse(a, case["nstep"], case["c"], case["factor"], form=form)
            continue
        got = G.diffuse(a, case["nstep"], case["c"], case["factor"], form=form)
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.array_equal(H.bits(got), H.bits(want)), form


@pytest.mark.parametrize("which", range(9))
def test_sweep_around_tile_and_steps_per_launch(ctx, shape, which):
    B, T = shape
    n = (1, 2, 3, 5, B - 1, B, B + 1, 2 * B + 3, 257)[which]
    steps = sorted({1, 2, T - 1, T, T + 1, 3 * T + 2})
    for kind in ("f", "bool"):
        a = H.make_input(100 + n, n, kind)
        mult = H.multiplier(n)
        want, done = {}, 0
        field = np.array(a, dtype=np.float64)
        for s in steps:                                          # the reference once, advanced through the sorted step counts
            field = H.advance(field, s - done, mult)
            want[s], done = field, s
        for s in steps:
            for form in ("plain", "blocked"):
                got = one_shot(ctx, a, s, form)
                assert np.array_equal(H.bits(got), H.bits(want[s])), (n, s, kind, form)


def test_mid_size_all_forms(ctx):
    a = H.make_input(7, 512, "f")
    want = H.advance(a, 64, H.multiplier(512))
    for form in FORMS:
        assert np.array_equal(H.bits(G.diffuse(a, 64, form=form)), H.bits(want)), form
    sq = H.make_input(8, 512, "bool")
    assert np.array_equal(H.bits(one_shot(ctx, sq, 64, "blocked")), H.bits(H.advance(sq, 64, H.multiplier(512))))


def test_series_is_one_run():
    a = H.make_input(21, 70, "f")
    info = {}
    shots = G.diffuse_series(a, [40, 0, 7, 40, 123], info=info)
    assert len(shots) == 5 and shots[1] is a
    assert info["steps_done"] == 123
    for t, got in zip([40, 0, 7, 40, 123], shots):
        if t:
            assert np.array_equal(H.bits(got), H.bits(G.diffuse(a, t))), t
    assert np.array_equal(H.bits(shots[0]), H.bits(shots[3]))
    assert np.array_equal(H.bits(shots[4]), H.bits(H.advance(a, 123, H.multiplier(70))))
    with pytest.raises(AssertionError):                          # every snapshot gets the checks: unstable factor
        G.diffuse_series(H.make_input(3, 16, "f"), [2, 50], delta_t_factor=3.0)


def test_transposed_input_and_other_dtypes():
    base = H.make_input(5, 90, "f")
    view = base.T
    assert not view.flags["C_CONTIGUOUS"]
    assert np.array_equal(H.bits(G.diffuse(view, 19)), H.bits(G.diffuse(np.ascontiguousarray(view), 19)))
    ints = (H.make_input(6, 40, "sq") * 5).astype(np.int16)
    assert np.array_equal(H.bits(G.diffuse(ints[::-1], 11)), H.bits(H.advance(ints[::-1], 11, H.multiplier(40))))


def test_engine_on_the_same_context_is_untouched(ctx):
    lib, c = ctx
    with open(os.path.join(H.GOLDEN, "manifest.json")) as f:
        case = [k for k in json.load(f)["t1_kernel"] if (k["F"], k["h"], k["w"], k["kind"]) == (64, 8, 8, "levels")][0]
    views, scene = kernel_case_inputs(case)
    patches = np.ascontiguousarray(np.stack([scene, views[17], views[40], scene[::-1]]))
    assert lib.dv_set_library(c, N.u8ptr(views), 64, 8, 8, 3, 0.25, 0) == 0, lib.dv_last_error(c)
    before, after = N.StepResult(), N.StepResult()
    scene_before, scene_after = np.empty(64), np.empty(64)
    assert lib.dv_step(c, N.u8ptr(patches), 4, 0, ctypes.byref(before), N.f64ptr(scene_before)) == 0
    a = H.make_input(9, 100, "f")
    assert lib.dv_diffuse_begin(c, N.f64ptr(a), 100, 1.0, 0.5) == 0
    assert lib.dv_diffuse_advance(c, 13, N.DV_DIFFUSE_AUTO) == 0
    assert lib.dv_step(c, N.u8ptr(patches), 4, 0, ctypes.byref(after), N.f64ptr(scene_after)) == 0     # field still resident
    out = np.empty((100, 100))
    assert lib.dv_diffuse_read(c, N.f64ptr(out)) == 0 and lib.dv_diffuse_end(c) == 0
    assert np.array_equal(H.bits(out), H.bits(H.advance(a, 13, H.multiplier(100))))
    assert bytes(before) == bytes(after) and scene_before.tobytes() == scene_after.tobytes()
    assert before.best_view >= 0 and before.n_headings == 4
    assert lib.dv_clear_library(c) == 0


def test_bad_arguments_and_state(ctx):
    lib, c = ctx
    a = np.ones((4, 4))
    for args in ((N.f64ptr(a), 0, 1.0, 0.5), (N.f64ptr(a), 4, 0.0, 0.5), (None, 4, 1.0, 0.5)):
        lib.dv_synchronize(c)
        assert lib.dv_diffuse_begin(c, *args) == -1
        assert b"dv_diffuse_begin" in lib.dv_last_error(c)
    out = np.empty((4, 4))
    assert lib.dv_diffuse_advance(c, 3, N.DV_DIFFUSE_AUTO) == -3 and b"dv_diffuse_advance" in lib.dv_last_error(c)
    assert lib.dv_diffuse_read(c, N.f64ptr(out)) == -3
    assert lib.dv_diffuse_begin(c, N.f64ptr(a), 4, 1.0, 0.5) == 0
    assert lib.dv_diffuse_advance(c, 3, 7) == -1 and lib.dv_diffuse_advance(c, -1, 0) == -1
    done = ctypes.c_int()
    assert lib.dv_diffuse_advance(c, 0, 0) == 0 and lib.dv_diffuse_advance(c, 5, 0) == 0
    assert lib.dv_diffuse_info(c, None, None, ctypes.byref(done)) == 0 and done.value == 5
    assert lib.dv_diffuse_read(c, N.f64ptr(out)) == 0 and np.all(out == 1.0)
    assert lib.dv_diffuse_end(c) == 0 and lib.dv_diffuse_advance(c, 1, 0) == -3


def test_configured_window_and_steps_give_the_same_bits():
    a = H.make_input(31, 150, "f")
    want = H.advance(a, 37, H.multiplier(150))
    for window, steps, tile in ((96, 16, 64), (96, None, 80), (None, 3, 58), (64, 44, 8)):
        run = G.DiffuseRun(a, window=window, steps_per_launch=steps)
        try:
            run.advance(37, "blocked")
            assert run.info()["tile"] == tile and run.info()["steps_done"] == 37
            assert np.array_equal(H.bits(run.read()), H.bits(want)), (window, steps)
        finally:
            run.close()
    with pytest.raises(N.EngineError):
        G.DiffuseRun(a, window=80)
