#!/usr/bin/env python3
"""Generate tests/golden/t8_diffuse.npz / t8_diffuse.json by RUNNING THE REFERENCE'S OWN diffuse (navsim/util.pyx:189-235).

Like make_golden.py (whose build_reference / import_reference it uses) this runs only where the reference, Cython and gcc
are; the reference is compiled in a scratch directory and nothing of it is written into the repository.  Committed are the
reference's OUTPUTS (npz) and, per case, seed / n / nstep / c / factor / kind, the SHA-256 of the input regenerated from the
seed (tests/helpers_diffuse.py:make_input) and whether the reference raised (json).  The npz is written with fixed zip
timestamps, so a second run gives the same bytes.

    python3 tests/golden/make_golden_diffuse.py --reference DIR [--out tests/golden] [--time]

--time prints the reference's seconds for 500 x 500 x 20 steps (the CPU figure beside the GPU table of DESIGN 4) and writes
nothing."""
import argparse
import io
import json
import os
import shutil
import sys
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import build_reference, import_reference  # noqa: E402
from helpers_diffuse import make_input, sha  # noqa: E402

# (n, nstep, c, factor, kind)
CASES = [
    (1, 3, 1.0, 0.5, "f"), (2, 5, 1.0, 0.5, "f"), (3, 7, 0.7, 0.5, "f"), (5, 40, 3.0, 0.9, "f"), (67, 33, 1.0, 0.5, "sq"),
    (130, 17, 0.7, 0.5, "f"), (96, 200, 1.0, 0.5, "sq"), (64, 1, 1.0, 0.5, "f32"), (33, 64, 1.0, 1.0, "f"),
    (16, 50, 1.0, 3.0, "f"), (16, 50, 1.0, 1.5, "sq"),
    # beyond the eleven: a side that is no multiple of any tile with a step count past several launches, and a stable c != 1 on squares
    (101, 45, 1.0, 0.5, "f"), (50, 29, 2.5, 0.4, "sq"),
]


def write_npz(path, arrays):
    """np.savez_compressed with every member's timestamp fixed (byte-identical regeneration)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    work = build_reference(args.reference)
    try:
        navsim = import_reference(work)
        ref_diffuse = navsim.util.diffuse
        if args.time:
            a = make_input(1, 500, "f")
            best = min(_timed(ref_diffuse, a, 20) for _ in range(5))
            print(json.dumps(dict(what="reference diffuse, 500x500, 20 steps", seconds=round(best, 4),
                                  ns_per_cell_step=round(best / (500 * 500 * 20) * 1e9, 2))))
            return
        arrays, cases = {}, []
        for k, (n, nstep, c, factor, kind) in enumerate(CASES):
            seed = 8000 + k
            a = make_input(seed, n, kind)
            key = "d%02d_n%d_s%d" % (k, n, nstep)
            raised = None
            try:
                out = ref_diffuse(a, nstep, c, factor)
                assert out.dtype == np.float64 and out.shape == (n, n)
                arrays[key] = out
            except AssertionError:
                raised = "AssertionError"
            cases.append(dict(key=key, seed=seed, n=n, nstep=nstep, c=c, factor=factor, kind=kind, input_sha=sha(a), raised=raised))
        write_npz(os.path.join(args.out, "t8_diffuse.npz"), arrays)
        with open(os.path.join(args.out, "t8_diffuse.json"), "w") as f:
            json.dump(dict(generator="tests/golden/make_golden_diffuse.py", numpy=np.__version__,
                           note="outputs of the reference's own diffuse on inputs regenerated from seeds", cases=cases),
                      f, indent=1, sort_keys=True)
            f.write("\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print("diffuse fixtures written to", args.out)


def _timed(fn, a, nstep):
    t0 = time.perf_counter()
    fn(a, nstep)
    return time.perf_counter() - t0


if __name__ == "__main__":
    main()
