"""Shared pieces of the register-ring fp4 bodies' caller tests (tests/test_gpu_lreg_callers.py, tests/test_lreg_place_host.py):
where a view lands in a launch of those bodies, the engine sets the tests run under, a pair of views that score alike from
different integer sums, and the CPU oracle's score rows, computed once per (library, weight, patch) and shared.

place() restates launch_body (dejavu_hip.hip: item_groups, grid) and the bodies' cursor (dejavu_kernels.h: sad_lc_fp4_lreg,
sad_lc_fp4_lreg8: group g0 + wave * 2 + t of an item, both bodies; the four-consumer bodies have waves 0-3 and items of 8 view
groups, the eight-wave body waves 0-7 and items of 16) and fused_finish's register layout (a lane of half `lane >> 5` holds views
(r & 3) + 8 (r >> 2) + 4 half of a group).  The GPU tests use it to choose where to plant views and to assert that a planted view
is where a case says it is; expected results never come from it.
"""
import functools
import hashlib

import numpy as np

from navsim_amd import synth
from oracle import oracle

GROUPS_EIGHT_WAVES = 16      # view groups of 32 per work item: sad_lc_fp4_lreg8
GROUPS_FOUR_CONSUMERS = 8    # sad_lc_fp4_lreg


@functools.lru_cache(maxsize=None)
def item_bounds(F, groups_per_item):
    """(G32, GQ, [first group of item 0 .. GQ]) of a library of F views."""
    fpad = (F + 63) // 64 * 64
    g32 = fpad // 32
    gq = (g32 + groups_per_item - 1) // groups_per_item
    return g32, gq, tuple((i * g32) // gq for i in range(gq + 1))


def place(F, view, groups_per_item):
    """(item, n_items, groups_in_item, wave, t, half, workgroup) of view `view` of a library of F views."""
    if not 0 <= view < F:
        raise ValueError("view %d outside [0, %d)" % (view, F))
    g32, gq, first = item_bounds(F, groups_per_item)
    group = view // 32
    item = (group * gq) // g32
    while first[item + 1] <= group:
        item += 1
    while first[item] > group:
        item -= 1
    k = group - first[item]
    return item, gq, first[item + 1] - first[item], k // 2, k % 2, (view % 32) >> 2 & 1, item % 256


# ---- engine sets: the three bodies under test and the LDS-ring witness (the context reads the knobs when it is created)
_BASE = {"DEJAVU_SHAPE": "6", "DEJAVU_BITS": "2", "DEJAVU_VCODE": None, "DEJAVU_LIBREG": None, "DEJAVU_MFMA_CHUNK": None,
         "DEJAVU_LREG8": None, "DEJAVU_HT": None}
ENGINE_SETS = {
    "eight_waves": {"DEJAVU_LREG8": "1"},                           # Body::LcRegCode8
    "four_consumers_codes": {"DEJAVU_LREG8": "0"},                  # Body::LcRegCode
    "thermometer_ring": {"DEJAVU_VCODE": "0"},                      # Body::LcReg
    "lds_ring": {"DEJAVU_VCODE": "0", "DEJAVU_LIBREG": "0"},        # Body::Lc: the bit-for-bit witness
}
UNDER_TEST = ["eight_waves", "four_consumers_codes", "thermometer_ring"]
_FORM = {   # scoring_form() of a pass on the fp4 image
    "eight_waves": dict(codes=True, consumers8=True),
    "four_consumers_codes": dict(codes=True, consumers8=False),
    "thermometer_ring": dict(codes=False, consumers8=False),
    "lds_ring": dict(codes=False, consumers8=False),
}


def engine(kind, one_chunk=True, second_tile_as_pass=False):
    from tests.helpers import engine_with
    env = dict(_BASE, **ENGINE_SETS[kind])
    if one_chunk:
        env["DEJAVU_MFMA_CHUNK"] = "1"
    if second_tile_as_pass:
        env["DEJAVU_HT"] = "1"
    return engine_with(env)


def assert_form(eng, kind, fused, fp4=True):
    """The last pass ran the body the case is about.  fused: None = not looked at (a step that wanted the scene)."""
    form = eng.scoring_form()
    assert form["matrix_cores"], (kind, form)
    if not fp4:
        assert not form["fp4"] and not form["codes"] and not form["consumers8"], (kind, form)
    else:
        assert form["fp4"], (kind, form)
        assert form["codes"] == _FORM[kind]["codes"] and form["consumers8"] == _FORM[kind]["consumers8"], (kind, form)
    if fused is not None:
        assert form["fused_finish"] == fused, (kind, form)
    return form


# ---- equal scores from different sums
def tied_pair(x):
    """(Y, Z): Y = x with two saturation bytes flipped 0 <-> 127 (S_hs = 254, S_v = 0 against x), Z = x with one value byte moved
    0 -> 63 and one 63 -> 127 (S_hs = 0, S_v = 127).  0.25 * 254 = 0.5 * 127: the same score against x at chem_weight 0.5 and at no
    other weight.  The four pixels are distinct."""
    flat = x.reshape(-1, 3)
    y = flat.copy()
    for p in (5, 700):
        y[p, 1] = 127 - y[p, 1]
    assert set(np.unique(flat[:, 1])) <= {0, 127}
    z = flat.copy()
    p0 = int(np.flatnonzero(flat[:, 2] == 0)[3])
    p63 = int(np.flatnonzero(flat[:, 2] == 63)[-3])
    assert len({5, 700, p0, p63}) == 4
    z[p0, 2] = 63
    z[p63, 2] = 127
    return y.reshape(x.shape), z.reshape(x.shape)


# ---- the oracle's rows, once
_ROWS = {}


def oracle_rows(lib_name, lib, patches, cw):
    """float64[A, F]: oracle.sads_hsv of every patch against `lib` (named `lib_name`: the cache's key beside the weight and the
    patch's bytes).  Read-only rows."""
    out = np.empty((len(patches), len(lib)), dtype=np.float64)
    for a, p in enumerate(patches):
        key = (lib_name, float(cw), hashlib.sha256(np.ascontiguousarray(p).tobytes()).digest())
        row = _ROWS.get(key)
        if row is None:
            row = oracle.sads_hsv(lib, p, cw).copy()
            row.setflags(write=False)
            _ROWS[key] = row
        out[a] = row
    return out


def step_of_rows(rows):
    """oracle.step's decision from the rows (NavBySceneFamiliarity.py:313-316: first maximum over views, first over headings)."""
    fam = rows.max(axis=1)
    view = rows.argmax(axis=1)
    bi = int(fam.argmax())
    return dict(angle_familiarity=fam, angle_view=view, best_idex=bi, best_view=int(view[bi]), step_familiarity=float(fam[bi]),
                scene_familiarity=rows.min(axis=0))


def clear_headings(rows, tied=()):
    """Headings whose reported view the oracle settles: the best clears the second best by more than any rounding (1e-6 of ~1e3), or
    the case planted the tie (`tied`: exact copies or a checked pair -- the first view wins)."""
    if rows.shape[1] < 2:
        return np.ones(len(rows), dtype=bool)
    top2 = np.partition(rows, -2, axis=1)[:, -2:]
    clear = top2[:, 0] < top2[:, 1] - 1e-6
    clear[list(tied)] = True
    return clear


def fresh_view(i, h=32, w=32):
    """A view no library of the tests holds until a case plants it."""
    return synth.synth_views(5000 + i, 1, h, w)[0]
