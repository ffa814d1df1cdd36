"""The register-ring fp4 body reading the value plane as 3-bit level codes (sad_lc_fp4_lreg<.., CODE>, Body::LcRegCode: the
default where the code tiles exist) against the same body on thermometer rows (DEJAVU_VCODE=0) and against the LDS-ring
body (DEJAVU_VCODE=0, DEJAVU_LIBREG=0).  The sums are integers, so every score agrees to the last bit: the steps' heading
familiarities and views, and (want_scene) every view's scene familiarity.  The shapes are the smallest that reach each of
the body's peeled stage loops (saturation -> saturation, last saturation -> value, value -> value, last value -> the next
item's first stage), a library without a saturation segment, more items than workgroups, and the two fallbacks (uneven
value widths, no value plane), where the default engine must not report codes.
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
    # (views, h, w, cw, one K chunk forced, uneven value widths, the default engine reads codes)
    (7000 + 19, 32, 32, 0.25, True, False, True),   # NK = 8 + 16: the one saturation stage is the last; last item of 4 groups, last group of 11 views
    (3000 + 5, 64, 64, 0.25, True, False, True),    # NK = 32 + 64: every peeled loop runs more than once
    (7000 + 19, 32, 32, 0.0, True, False, True),    # no saturation segment: value follows value across items
    (70000 + 7, 32, 32, 0.25, False, False, True),  # 274 items on 256 workgroups, one chunk unforced (fused finishing)
    (5000 + 21, 32, 32, 0.25, True, True, False),   # fallback: the value widths disagree
    (7000 + 19, 32, 32, 1.0, True, False, False),   # no value plane: no code tiles
]

_BASE = {"DEJAVU_SHAPE": "6", "DEJAVU_BITS": "2", "DEJAVU_VCODE": None, "DEJAVU_LIBREG": None, "DEJAVU_MFMA_CHUNK": None}


def _engines(force_chunk):
    base = dict(_BASE)
    if force_chunk:
        base["DEJAVU_MFMA_CHUNK"] = "1"
    return (engine_with(base), engine_with(dict(base, DEJAVU_VCODE="0")), engine_with(dict(base, DEJAVU_VCODE="0", DEJAVU_LIBREG="0")))


@pytest.mark.parametrize("F,h,w,cw,force_chunk,uneven,codes", CASES)
def test_code_rows_give_the_thermometer_rows_sums(F, h, w, cw, force_chunk, uneven, codes):
    lib0 = synth.synth_views(91 + F, F, h, w)
    lib = _uneven_v(lib0) if uneven else lib0
    engines = _engines(force_chunk)
    e_code, e_thermo, e_lds = engines
    try:
        for e in engines:
            e.set_library(lib, cw)
            info = e.library_info()
            assert info["fp4_form"] and info["has_bit_planes"], info
        assert (e_code.library_info()["code_tile_bytes"] > 0) == codes
        assert e_thermo.library_info()["code_tile_bytes"] == 0 and e_lds.library_info()["code_tile_bytes"] == 0
        for A in (13, 32):
            pats = synth.synth_patches(300 + A, A, h, w)
            pats[A // 3] = synth.near_match_patch(lib0[(A * 977) % F], A, fraction=0.03)
            if uneven:
                pats = _uneven_v(pats)                      # (on the library's levels: the fp4 form)
            want = oracle.step(lib, pats, cw) if F < 10000 else None
            for want_scene in (False, True):
                got = e_code.step(pats, want_scene=want_scene)
                form = e_code.scoring_form()
                assert form["matrix_cores"] and form["fp4"] and form["codes"] == codes, (form, F, A, want_scene)
                for other in (e_thermo, e_lds):
                    ref = other.step(pats, want_scene=want_scene)
                    assert not other.scoring_form()["codes"]
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


def test_off_level_patches_take_the_int8_form_and_the_bit_tiles():
    """A patch byte strictly inside a gap has no fp4 coefficient: the same launch scores with the int8 image, which reads the
    bit tiles -- no codes reported, and the decision is the DEJAVU_VCODE=0 engine's."""
    F, h, w, cw, A = 7000 + 19, 32, 32, 0.25, 13
    lib = synth.synth_views(91 + F, F, h, w)
    pats = synth.synth_patches(300 + A, A, h, w)
    pats[A // 3] = synth.near_match_patch(lib[(A * 977) % F], A, fraction=0.03)
    levels = sorted(int(v) for v in synth.V_LEVELS)
    pats[0, 1, 1, 2] = (levels[1] + levels[2]) // 2         # strictly between two value levels
    assert levels[1] < pats[0, 1, 1, 2] < levels[2]
    e_code, e_thermo, e_lds = _engines(True)
    try:
        for e in (e_code, e_thermo):
            e.set_library(lib, cw)
        assert e_code.library_info()["code_tile_bytes"] > 0
        want = oracle.step(lib, pats, cw)
        for want_scene in (False, True):
            got = e_code.step(pats, want_scene=want_scene)
            form = e_code.scoring_form()
            assert form["matrix_cores"] and not form["fp4"] and not form["codes"], form
            ref = e_thermo.step(pats, want_scene=want_scene)
            assert not e_thermo.scoring_form()["fp4"]
            assert (got["best_idex"], got["best_view"]) == (ref["best_idex"], ref["best_view"]) == (want["best_idex"], want["best_view"])
            assert np.array_equal(got["angle_familiarity"], ref["angle_familiarity"])
            assert np.array_equal(got["angle_view"], ref["angle_view"])
            if want_scene:
                assert np.array_equal(got["scene_familiarity"], ref["scene_familiarity"])
    finally:
        for e in (e_code, e_thermo, e_lds):
            e.close()
