"""The register-ring fp4 body on code rows with eight consumer waves (sad_lc_fp4_lreg8, Body::LcRegCode8, forced with
DEJAVU_LREG8=1) against the four-consumer body it derives from (DEJAVU_LREG8=0) and against the LDS-ring body
(DEJAVU_VCODE=0, DEJAVU_LIBREG=0).  The sums are integers, so every score agrees to the last bit: the steps' heading
familiarities and views, the decision, and (want_scene: the unfused form, which stores its sums) every view's scene familiarity.
Every wave counts its vector-memory waits by hand around the LDS-DMA it now issues itself, so the shapes are the smallest at
which each part of that schedule can go wrong: waves without view groups, a partial last group, one saturation stage that is
also the last, every peeled stage loop running more than once, no saturation segment, and more items than workgroups (the
library cursor and the DMA stage numbering cross an item boundary inside a workgroup, under the fused finishing).
"""

import numpy as np
import pytest

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
    # (views, h, w, cw, one K chunk forced, uneven value widths, the forced engine takes the new body)
    (89, 32, 32, 0.25, True, False, True),          # 3 view groups: waves 2-7 hold nothing, wave 1 one group; NK = 8 + 16: the one saturation stage is the last
    (300 + 5, 32, 32, 0.25, True, False, True),     # 10 groups: wave 4 is live, waves 5-7 are not, the last group is partial
    (7000 + 19, 32, 32, 0.25, True, False, True),   # several items of 15 or 16 groups on separate workgroups
    (3000 + 5, 64, 64, 0.25, True, False, True),    # NK = 32 + 64: every peeled loop runs more than once
    (7000 + 19, 32, 32, 0.0, True, False, True),    # no saturation segment: value follows value across items
    (140000 + 7, 32, 32, 0.25, False, False, True), # 274 items on 256 workgroups, one chunk unforced (the fused finishing)
    (300 + 5, 32, 32, 0.25, True, True, False),     # fallback: the value widths disagree
    (300 + 5, 32, 32, 1.0, True, False, False),     # fallback: no value plane, no code tiles
]

_BASE = {"DEJAVU_SHAPE": "6", "DEJAVU_BITS": "2", "DEJAVU_VCODE": None, "DEJAVU_LIBREG": None, "DEJAVU_MFMA_CHUNK": None,
         "DEJAVU_LREG8": None}


def _engines(force_chunk):
    base = dict(_BASE)
    if force_chunk:
        base["DEJAVU_MFMA_CHUNK"] = "1"
    return (engine_with(dict(base, DEJAVU_LREG8="1")), engine_with(dict(base, DEJAVU_LREG8="0")),
            engine_with(dict(base, DEJAVU_VCODE="0", DEJAVU_LIBREG="0")))


@pytest.mark.parametrize("F,h,w,cw,force_chunk,uneven,takes", CASES)
def test_eight_consumers_give_the_four_consumers_sums(F, h, w, cw, force_chunk, uneven, takes):
    lib0 = synth.synth_views(91 + F, F, h, w)
    lib = _uneven_v(lib0) if uneven else lib0
    engines = _engines(force_chunk)
    e_new, e_cur, e_lds = engines
    try:
        for e in engines:
            e.set_library(lib, cw)
            info = e.library_info()
            assert info["fp4_form"] and info["has_bit_planes"], info
        assert (e_new.library_info()["code_tile_bytes"] > 0) == takes
        assert (e_cur.library_info()["code_tile_bytes"] > 0) == takes and e_lds.library_info()["code_tile_bytes"] == 0
        for A in (13, 32):
            pats = synth.synth_patches(300 + A, A, h, w)
            pats[A // 3] = synth.near_match_patch(lib0[(A * 977) % F], A, fraction=0.03)
            if uneven:
                pats = _uneven_v(pats)                      # (on the library's levels: the fp4 form)
            want = oracle.step(lib, pats, cw) if F < 10000 else None
            for want_scene in (False, True):
                got = e_new.step(pats, want_scene=want_scene)
                form = e_new.scoring_form()
                assert form["matrix_cores"] and form["fp4"] and form["codes"] == takes and form["consumers8"] == takes, (form, F, A, want_scene)
                if not force_chunk:
                    assert form["fused_finish"] == (not want_scene), (form, F, A, want_scene)
                for other in (e_cur, e_lds):
                    ref = other.step(pats, want_scene=want_scene)
                    assert not other.scoring_form()["consumers8"]
                    assert (got["best_idex"], got["best_view"]) == (ref["best_idex"], ref["best_view"]), (F, A, want_scene)
                    assert np.array_equal(got["angle_familiarity"], ref["angle_familiarity"]), (F, A, want_scene)
                    assert np.array_equal(got["angle_view"], ref["angle_view"]), (F, A, want_scene)
                    if want_scene:
                        assert np.array_equal(got["scene_familiarity"], ref["scene_familiarity"]), (F, A)
                if want is not None:
                    assert (got["best_idex"], got["best_view"]) == (want["best_idex"], want["best_view"]), (F, A)
                    np.testing.assert_allclose(got["angle_familiarity"], want["angle_familiarity"], rtol=1e-9)
    finally:
        for e in engines:
            e.close()


def test_off_level_patches_take_the_int8_form_in_two_ranges_of_eight():
    """A patch byte strictly inside a gap has no fp4 coefficient: the new body's launch scores with the int8 ring body, which walks
    every item of 16 view groups as two ranges of 8 -- the four-consumer engine's results and the oracle's."""
    F, h, w, cw, A = 7000 + 19, 32, 32, 0.25, 13
    lib = synth.synth_views(91 + F, F, h, w)
    pats = synth.synth_patches(300 + A, A, h, w)
    pats[A // 3] = synth.near_match_patch(lib[(A * 977) % F], A, fraction=0.03)
    levels = sorted(int(v) for v in synth.V_LEVELS)
    pats[0, 1, 1, 2] = (levels[1] + levels[2]) // 2         # strictly between two value levels
    assert levels[1] < pats[0, 1, 1, 2] < levels[2]
    engines = _engines(True)
    e_new, e_cur, _ = engines
    try:
        for e in (e_new, e_cur):
            e.set_library(lib, cw)
        assert e_new.library_info()["code_tile_bytes"] > 0
        want = oracle.step(lib, pats, cw)
        for want_scene in (False, True):
            got = e_new.step(pats, want_scene=want_scene)
            form = e_new.scoring_form()
            assert form["matrix_cores"] and not form["fp4"] and not form["codes"] and not form["consumers8"], form
            ref = e_cur.step(pats, want_scene=want_scene)
            assert not e_cur.scoring_form()["fp4"]
            assert (got["best_idex"], got["best_view"]) == (ref["best_idex"], ref["best_view"]) == (want["best_idex"], want["best_view"])
            assert np.array_equal(got["angle_familiarity"], ref["angle_familiarity"])
            assert np.array_equal(got["angle_view"], ref["angle_view"])
            np.testing.assert_allclose(got["angle_familiarity"], want["angle_familiarity"], rtol=1e-9)
            if want_scene:
                assert np.array_equal(got["scene_familiarity"], ref["scene_familiarity"])
    finally:
        for e in engines:
            e.close()


def test_default_rule_keeps_four_consumers_for_a_small_library():
    """With the knob unset the new body needs two rounds of the grid in items of 16 view groups (512): 7000 views have 14."""
    F, h, w, cw, A = 7000, 32, 32, 0.25, 13
    lib = synth.synth_views(91 + F, F, h, w)
    pats = synth.synth_patches(300 + A, A, h, w)
    e = engine_with(dict(_BASE, DEJAVU_MFMA_CHUNK="1"))
    try:
        e.set_library(lib, cw)
        e.step(pats)
        form = e.scoring_form()
        assert form["matrix_cores"] and form["fp4"] and form["codes"] and not form["consumers8"], form
    finally:
        e.close()
