"""NumPy restatement of the reference's diffuse (navsim/util.pyx:189-235) and the inputs of its fixtures (tests/golden/t8_diffuse.*).

The restatement performs the reference's operations in the reference's order, each a separate NumPy double operation (NumPy
never fuses a multiply into an add), with np.roll for the periodic neighbours; tests/test_diffuse_host.py holds it to the
reference's recorded outputs bit for bit, and the GPU tests then use it as the reference for shapes the fixtures do not cover."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def multiplier(n, c=1.0, delta_t_factor=0.5):
    delta_s = 1.0 / (n + 1)
    delta_t = delta_t_factor * (delta_s ** 2 / (2 * c))
    return c * (delta_t / (delta_s * delta_s))


def advance(mat, nstep, mult):
    """`nstep` sweeps on a float64 array; returns a new array."""
    mat = np.array(mat, dtype=np.float64)
    for _ in range(nstep):
        s = np.roll(mat, -1, axis=0) + np.roll(mat, 1, axis=0)      # m[i+1, j] + m[i-1, j]
        s = s - 4 * mat
        s = s + np.roll(mat, -1, axis=1)                            # m[i, j+1]
        s = s + np.roll(mat, 1, axis=1)                             # m[i, j-1]
        mat = mat + mult * s
    return mat


def diffuse_restated(initial_condition, nstep, c=1.0, delta_t_factor=0.5):
    if nstep == 0:
        return initial_condition
    assert initial_condition.shape[0] == initial_condition.shape[1]
    out = advance(initial_condition, nstep, multiplier(initial_condition.shape[0], c, delta_t_factor))
    assert np.sum(out) - np.sum(initial_condition) < 0.0000001
    assert np.max(out) <= np.max(initial_condition)
    assert np.min(out) >= np.min(initial_condition)
    assert not np.any(np.isnan(out))
    return out


def make_input(seed, n, kind):
    """Inputs of the fixture cases, regenerated from the seed.  "f": doubles in [0, 1); "f32": the same as float32; "sq": a few
    6 x 6 squares of ones on int64 zeros (clipped at the edges); "bool": those squares as bool."""
    rng = np.random.default_rng(seed)
    if kind in ("f", "f32"):
        a = rng.random((n, n))
        return a.astype(np.float32) if kind == "f32" else a
    a = np.zeros((n, n), dtype=np.int64)
    for _ in range(max(1, n * n // 150)):
        x, y = rng.integers(0, n, 2)
        a[max(0, x - 3):x + 3, max(0, y - 3):y + 3] = 1
    return a.astype(bool) if kind == "bool" else a


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def fixture_cases():
    """[(case dict, input array, the reference's output or None where it raised)]"""
    with open(os.path.join(GOLDEN, "t8_diffuse.json")) as f:
        meta = json.load(f)
    out = []
    with np.load(os.path.join(GOLDEN, "t8_diffuse.npz")) as z:
        for case in meta["cases"]:
            a = make_input(case["seed"], case["n"], case["kind"])
            assert sha(a) == case["input_sha"], case["key"]
            out.append((case, a, None if case["raised"] else z[case["key"]]))
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
