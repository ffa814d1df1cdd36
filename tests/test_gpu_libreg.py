"""The fp4 body with the library rows in the consumers' registers (sad_lc_fp4_lreg) against the body that streams them through
the LDS ring (DEJAVU_LIBREG=0): the same integer sums, so the same scores to the last bit -- the fused steps' heading
familiarities and views, and (want_scene: the unfused pass, k_finish behind the kernel) every view's scene familiarity.
Ragged view counts (a partial last item of 8 view groups and a partial last view group), saturation / value boundaries
after one and after four stages, and a library whose value widths differ on bit positions 1..3 (the host then keeps the
LDS body) are covered; the oracle checks the winners.
"""

import numpy as np
import pytest

import navsim_amd
from navsim_amd import synth
from oracle import oracle
from tests.helpers import engine_with

pytestmark = pytest.mark.gpu


def _uneven_v(views):
    """The five value levels moved to 0 / 40 / 100 / 170 / 255: widths 40, 60, 70, 85 -- bit positions 1, 2, 3 disagree."""
    out = views.copy()
    remap = np.zeros(256, dtype=np.uint8)
    remap[np.asarray(synth.V_LEVELS, dtype=np.int64)] = np.array([0, 40, 100, 170, 255], dtype=np.uint8)
    out[..., 2] = remap[views[..., 2]]
    return out


CASES = [
    # (views, h, w, one K chunk forced, uneven value widths)
    (7000 + 19, 32, 32, True, False),       # 28 items, the last of 4 view groups, the last group of 11 views; boundary after stage 1
    (3000 + 5, 64, 64, True, False),        # saturation / value boundary after four stages of eight K-steps
    (41000 + 13, 32, 32, False, False),     # enough items for one chunk without forcing it
    (5000 + 21, 32, 32, True, True),        # the fallback: the LDS body on both sides
]


@pytest.mark.parametrize("F,h,w,force_chunk,uneven", CASES)
def test_register_body_gives_the_lds_bodys_sums(F, h, w, force_chunk, uneven):
    cw = 0.25
    lib0 = synth.synth_views(91 + F, F, h, w)
    lib = _uneven_v(lib0) if uneven else lib0
    base = {"DEJAVU_SHAPE": "6", "DEJAVU_BITS": "2"}
    if force_chunk:
        base["DEJAVU_MFMA_CHUNK"] = "1"
    e_new = engine_with(base)
    e_old = engine_with(dict(base, DEJAVU_LIBREG="0"))
    try:
        for e in (e_new, e_old):
            e.set_library(lib, cw)
            info = e.library_info()
            assert info["fp4_form"] and info["has_bit_planes"], info
        for A in (13, 32):
            pats = synth.synth_patches(300 + A, A, h, w)
            pats[A // 3] = synth.near_match_patch(lib0[(A * 977) % F], A, fraction=0.03)
            if uneven:
                pats = _uneven_v(pats)                      # (on the library's levels: the fp4 form)
            want = oracle.step(lib, pats, cw) if F < 10000 else None
            for want_scene in (False, True):
                got_new = e_new.step(pats, want_scene=want_scene)
                got_old = e_old.step(pats, want_scene=want_scene)
                assert (got_new["best_idex"], got_new["best_view"]) == (got_old["best_idex"], got_old["best_view"])
                assert np.array_equal(got_new["angle_familiarity"], got_old["angle_familiarity"]), (F, A, want_scene)
                assert np.array_equal(got_new["angle_view"], got_old["angle_view"]), (F, A, want_scene)
                if want_scene:
                    assert np.array_equal(got_new["scene_familiarity"], got_old["scene_familiarity"]), (F, A)
                if want is not None:
                    assert (got_new["best_idex"], got_new["best_view"]) == (want["best_idex"], want["best_view"]), (F, A)
                    np.testing.assert_allclose(got_new["angle_familiarity"], want["angle_familiarity"], rtol=1e-9)
    finally:
        e_new.close()
        e_old.close()
