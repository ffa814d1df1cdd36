"""CPU tests of the landscape generators (navsim_amd/generate_landscapes.py): the NumPy restatement of the reference's diffuse
against the reference's recorded outputs (tests/golden/t8_diffuse.*), the parts of diffuse's contract that need no GPU, the
host generators, and the C ABI's surface.  The device kernels are held to the same fixtures in tests/test_gpu_diffuse.py."""
import os
import random
import re

import numpy as np
import pytest

from navsim_amd import _native as N
from navsim_amd import generate_landscapes as G
import navsim_amd

from . import helpers_diffuse as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = H.fixture_cases()


def test_fixture_holds_the_cases_of_the_reference_check():
    have = {(c["n"], c["nstep"], c["c"], c["factor"], c["kind"]): c["raised"] for c, _, _ in CASES}
    for key in ((1, 3, 1.0, 0.5, "f"), (2, 5, 1.0, 0.5, "f"), (3, 7, 0.7, 0.5, "f"), (67, 33, 1.0, 0.5, "sq"),
                (130, 17, 0.7, 0.5, "f"), (96, 200, 1.0, 0.5, "sq")):
        assert have[key] is None, key
    for key in ((5, 40, 3.0, 0.9, "f"), (64, 1, 1.0, 0.5, "f32"), (16, 50, 1.0, 3.0, "f"), (16, 50, 1.0, 1.5, "sq")):
        assert have[key] == "AssertionError", key
    assert (33, 64, 1.0, 1.0, "f") in have


@pytest.mark.parametrize("case,a,want", CASES, ids=[c["key"] for c, _, _ in CASES])
def test_restatement_equals_the_reference(case, a, want):
    if want is None:
        with pytest.raises(AssertionError):
            H.diffuse_restated(a, case["nstep"], case["c"], case["factor"])
        return
    got = H.diffuse_restated(a, case["nstep"], case["c"], case["factor"])
    assert got.dtype == np.float64 and np.array_equal(H.bits(got), H.bits(want))


def test_zero_steps_return_the_argument_itself():
    a = np.ones((3, 3))
    assert G.diffuse(a, 0) is a
    ragged = np.ones((2, 5))
    assert G.diffuse(ragged, 0) is ragged                     # no checks at all (util.pyx:194)
    assert all(x is a for x in G.diffuse_series(a, [0, 0])) and len(G.diffuse_series(a, [0, 0])) == 2
    assert navsim_amd.diffuse is G.diffuse and navsim_amd.generate_landscapes is G


def test_non_square_input_raises_before_any_device_call(monkeypatch):
    def no_device(*args, **kwargs):
        raise RuntimeError("device call")
    monkeypatch.setattr(G, "DiffuseRun", no_device)
    for bad in (np.ones((4, 5)), np.ones(7), np.ones((3, 3, 3))):
        with pytest.raises(AssertionError):
            G.diffuse(bad, 3)
        with pytest.raises(AssertionError):
            G.diffuse_series(bad, [0, 2])
    with pytest.raises(ValueError):
        G.diffuse(np.ones((3, 3)), 2, form="fast")
    with pytest.raises(ValueError):
        G.diffuse(np.ones((3, 3)), -1)
    with pytest.raises(ZeroDivisionError):
        G.diffuse(np.ones((3, 3)), 2, c=0.0)


def test_checkerboard_literal():
    want = np.array([[1, 1, 0, 0, 1, 1, 0, 0],
                     [1, 1, 0, 0, 1, 1, 0, 0],
                     [0, 0, 1, 1, 0, 0, 1, 1],
                     [0, 0, 1, 1, 0, 0, 1, 1]] * 2, dtype=np.float64)
    got = G.checkerboard(8, 2)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    ragged = G.checkerboard(7, 3)                              # a side that is no multiple of the field
    assert ragged.shape == (7, 7) and np.array_equal(ragged[0], [1, 1, 1, 0, 0, 0, 1]) and np.array_equal(ragged[3], [0, 0, 0, 1, 1, 1, 0])


def test_random_squares_under_a_fixed_seed():
    random.seed(5)
    a = G.random_squares((40, 30), 6, 9, value=3)
    assert a.shape == (40, 30) and a.dtype == np.dtype(int) and set(np.unique(a)) == {0, 3}
    random.seed(5)
    centres = [(random.randrange(0, 40), random.randrange(0, 30)) for _ in range(9)]
    want = np.zeros((40, 30), dtype=int)
    for x, y in centres:
        want[x - 3:x + 3, y - 3:y + 3] = 3                    # negative starts slice as the reference's do
    assert np.array_equal(a, want)
    random.seed(5)
    assert np.array_equal(G.random_squares((40, 30), 6, 9, value=3), a)
    with pytest.raises(AssertionError):
        G.random_squares((8, 8), 3, 1)


def test_image_from_prob_mat_extremes():
    zeros, ones = G.image_from_prob_mat(np.zeros((5, 7))), G.image_from_prob_mat(np.ones((5, 7)))
    assert zeros.dtype == np.float64 and not zeros.any() and ones.shape == (5, 7) and np.all(ones == 1.0)
    np.random.seed(3)
    rand = np.random.random(size=(4, 4))
    np.random.seed(3)
    assert np.array_equal(G.image_from_prob_mat(np.full((4, 4), 0.5)), (rand < 0.5).astype(np.float64))


def test_random_matrix_bw_balance():
    calls = []

    def all_white(shape, **kwargs):
        calls.append(kwargs)
        return np.zeros(shape, dtype=int)
    with pytest.raises(RuntimeError):
        G.random_matrix_bw_balance((10, 10), max_iter=7, func=all_white, s=2)
    assert calls == [dict(s=2)] * 7
    half = np.zeros((10, 10), dtype=int)
    half[:5] = 1
    assert G.random_matrix_bw_balance((10, 10), func=lambda shape: half) is half
    random.seed(1)
    mat = G.random_matrix_bw_balance((60, 60), proportion=0.3, threshold=0.1, s=6, n=40)
    assert 0.2 < mat.sum() / 3600.0 < 0.4


def test_header_and_library_export_the_same_diffuse_names():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    declared = set(re.findall(r"\b(dv_diffuse[a-z0-9_]*)\s*\(", header))
    assert declared == {"dv_diffuse_begin", "dv_diffuse_advance", "dv_diffuse_read", "dv_diffuse_end", "dv_diffuse_info", "dv_diffuse",
                        "dv_diffuse_configure"}
    assert declared == {k for k in N.PROTOTYPES if k.startswith("dv_diffuse")}
    lib = N.load()
    for name in declared:
        assert hasattr(lib, name), name
    for name, value in (("DV_DIFFUSE_AUTO", 0), ("DV_DIFFUSE_PLAIN", 1), ("DV_DIFFUSE_BLOCKED", 2)):
        assert getattr(N, name) == value and re.search(r"#define %s\s+%du\b" % (name, value), header)
