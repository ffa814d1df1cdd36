"""Every fp4 scoring body on the coefficient image whose nibbles carry the bit positions' magnitudes (k_patch_prep: +-2 / 1 / 0.5 / 2
against library bits read in place as 0.5 / 1 / 2 and bit 3 brought down to 0.5), each forced with the engine's knobs and named by
scoring_form(), against the int8 form (DEJAVU_FP4=0: no fp4 image at all) bit for bit and against the oracle.

The sums are integers, so nothing is approximate: with want_scene the unfused form stores every sum and every view's
scene_familiarity must be the int8 engine's to the last bit; the step without it must give the same headings' familiarities, views
and decision.  The libraries are the smallest at which a convention slip can hide: three view groups (idle waves), a partial last
group, a sensor whose last K-step ends in zero padding (24x24 = 576 pixels), no saturation segment (chem_weight 0), no value plane
(chem_weight 1), value levels {0, 255} (a gap wider than 127: the first plane stands for the whole gap, its copies' coefficients
stay zero), and one library large enough for the bodies that only fused passes of >= 160 items take (Lc22) -- without a forced
chunk count, so its steps finish inside the scoring kernel.  A body that does not apply to a library falls back, and the test
says to which body.
"""
import functools

import numpy as np
import pytest

from navsim_amd import synth
from oracle import oracle
from tests.helpers import engine_with

pytestmark = pytest.mark.gpu

RTOL = 1e-9                                     # against the oracle's float64 scores (tests/test_gpu_lreg8.py)

# key: (views, h, w, chem_weight, value levels {0, 255}, one K chunk forced)
LIBS = {}
for _F in (89, 305):
    for _s in (32, 24):
        for _cw in (0.25, 0.0, 1.0):
            LIBS["%dv_%dpx_cw%g" % (_F, _s, _cw)] = (_F, _s, _s, _cw, False, True)
LIBS["305v_32px_cw0.25_split"] = (305, 32, 32, 0.25, True, True)
LIBS["41007v_32px_cw0.25_unforced"] = (41007, 32, 32, 0.25, False, False)

_KNOBS = ("DEJAVU_FP4", "DEJAVU_VCODE", "DEJAVU_LIBREG", "DEJAVU_LREG8", "DEJAVU_LC", "DEJAVU_LC22", "DEJAVU_HT", "DEJAVU_RING",
          "DEJAVU_MFMA_CHUNK", "DEJAVU_MFMA_TILES", "DEJAVU_FUSE", "DEJAVU_MIXED")
_BASE = dict(dict.fromkeys(_KNOBS), DEJAVU_SHAPE="6", DEJAVU_BITS="2")
# body: (knobs that force it where it fits, headings of its steps)
BODIES = {
    "Ring": ({"DEJAVU_LC": "0"}, (13, 32)),
    "Lc": ({"DEJAVU_VCODE": "0", "DEJAVU_LIBREG": "0"}, (13, 32)),
    "LcCode": ({"DEJAVU_VCODE": "1"}, (13, 32)),
    "LcReg": ({"DEJAVU_VCODE": "0"}, (13, 32)),
    "LcRegCode": ({"DEJAVU_LREG8": "0"}, (13, 32)),
    "LcRegCode8": ({"DEJAVU_LREG8": "1"}, (13, 32)),
    "Lc2Tiles": ({"DEJAVU_VCODE": "0", "DEJAVU_LC22": "0"}, (64,)),
    "Lc2TilesCode": ({"DEJAVU_VCODE": "1", "DEJAVU_LC22": "0"}, (64,)),
    "Lc22": ({}, (64,)),
}


def expected_body(body, key):
    """The body mfma_plan (csrc/dejavu_hip.hip) launches for a step without want_scene under `body`'s knobs: the body itself
    where its *_fits rule holds for the library, else what the rule falls back to."""
    F, h, w, cw, split, force_chunk = LIBS[key]
    has_v = cw < 1.0
    five_levels = has_v and not split                       # the 3-bit codes exist for a five-level value plane only
    # K-steps of 256 K-elements: hue and saturation are one plane each (2 per pixel, none at chem_weight 0), a five-level value
    # plane four, the {0, 255} plane three (a gap of 255 = three int8 planes); a segment's K-steps are padded to whole stages of four
    nk0 = -(-(-(-h * w * 2 // 256)) // 4) * 4 if cw > 0.0 else 0
    nk1 = -(-(-(-h * w * (3 if split else 4) // 256)) // 4) * 4 if has_v else 0
    g32 = (F + 63) // 64 * 2
    one_chunk = force_chunk or -(-g32 // 8) >= 160
    lreg_fits = nk0 % 8 == 0 and one_chunk                  # whole saturation stages; the register ring has no chunked form
    lreg_code_fits = lreg_fits and five_levels and nk1 % 8 == 0
    if body == "Lc2TilesCode":
        return "Lc2TilesCode" if five_levels else "Lc2Tiles"
    if body == "Lc22":                                      # fused passes of >= 160 items only; not with a forced chunk count
        return "Lc22" if (not force_chunk and -(-g32 // 8) >= 160) else "Lc2Tiles"
    if body == "LcCode":
        return "LcCode" if five_levels else ("LcReg" if lreg_fits else "Lc")
    if body == "LcReg":
        return "LcReg" if lreg_fits else "Lc"
    if body in ("LcRegCode", "LcRegCode8"):
        return body if lreg_code_fits else ("LcReg" if lreg_fits else "Lc")
    return body


def _split_value(x):
    """The five value levels folded onto {0, 255}."""
    out = x.copy()
    out[..., 2] = np.where(x[..., 2] >= 127, 255, 0).astype(np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def _case(key):
    """(library, {A: patches}, {(A, want_scene): the int8 engine's step}, {A: the oracle's step or None}), made once per library
    and read only."""
    F, h, w, cw, split, force_chunk = LIBS[key]
    lib0 = synth.synth_views(171 + F + h, F, h, w)
    lib = _split_value(lib0) if split else lib0
    pats = {}
    for A in (13, 32, 64):
        p = synth.synth_patches(400 + A + h, A, h, w)
        p[A // 3] = synth.near_match_patch(lib0[(A * 977) % F], A, fraction=0.03)
        p[A - 2] = lib0[F - 1]                             # the last view of a partial group, exactly
        pats[A] = _split_value(p) if split else p
        pats[A].setflags(write=False)
    lib.setflags(write=False)
    ref = {}
    e = engine_with(dict(_BASE, DEJAVU_FP4="0", DEJAVU_MFMA_CHUNK="1" if force_chunk else None))
    try:
        e.set_library(lib, cw)
        for A in pats:
            for want_scene in (True, False):
                r = e.step(pats[A], want_scene=want_scene)
                form = e.scoring_form()
                assert form["matrix_cores"] and not form["fp4"], (key, A, form)
                ref[A, want_scene] = {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in r.items()}
    finally:
        e.close()
    want = {A: oracle.step(lib, pats[A], cw) if F < 10000 else None for A in pats}
    return lib, pats, ref, want


@pytest.mark.parametrize("body", list(BODIES))
@pytest.mark.parametrize("key", list(LIBS))
def test_body_on_magnitude_image_equals_int8_form(key, body):
    F, h, w, cw, split, force_chunk = LIBS[key]
    lib, pats, ref, want = _case(key)
    knobs, headings = BODIES[body]
    eng = engine_with(dict(_BASE, **knobs, DEJAVU_MFMA_CHUNK="1" if force_chunk else None))
    names = []
    try:
        eng.set_library(lib, cw)
        info = eng.library_info()
        assert info["fp4_form"] and info["has_bit_planes"], (key, info)
        for A in headings:
            for want_scene in (True, False):
                got = eng.step(pats[A], want_scene=want_scene)
                form = eng.scoring_form()
                print(key, body, A, want_scene, form)
                assert form["matrix_cores"] and form["fp4"], (key, body, A, form)
                r = ref[A, want_scene]
                if want_scene:
                    assert np.array_equal(got["scene_familiarity"], r["scene_familiarity"]), (key, body, A)
                else:
                    names.append(form["body"])
                assert (got["best_idex"], got["best_view"]) == (r["best_idex"], r["best_view"]), (key, body, A, want_scene)
                assert np.array_equal(got["angle_familiarity"], r["angle_familiarity"]), (key, body, A, want_scene)
                assert np.array_equal(got["angle_view"], r["angle_view"]), (key, body, A, want_scene)
                if want[A] is not None:
                    assert (got["best_idex"], got["best_view"]) == (want[A]["best_idex"], want[A]["best_view"]), (key, body, A)
                    np.testing.assert_allclose(got["angle_familiarity"], want[A]["angle_familiarity"], rtol=RTOL)
                    if want_scene:
                        np.testing.assert_allclose(got["scene_familiarity"], want[A]["scene_familiarity"], rtol=RTOL)
        assert names == [expected_body(body, key)] * len(headings), (key, body, names)
    finally:
        eng.close()
