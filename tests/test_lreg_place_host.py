"""tests/helpers_lreg.py on the CPU.  place: the cut of a library into work items of the register-ring fp4 bodies, as launch_body and
the bodies make it, held to the properties the GPU tests rely on when they choose where to plant a view.  tied_pair: two views
that score alike from different integer sums.  oracle_rows / step_of_rows: the oracle's rows give oracle.step's record."""
import numpy as np
import pytest

from navsim_amd import synth
from oracle import oracle
from tests.helpers_lreg import (GROUPS_EIGHT_WAVES, GROUPS_FOUR_CONSUMERS, clear_headings, fresh_view, item_bounds, oracle_rows, place,
                                step_of_rows, tied_pair)


def test_known_places_at_7019_views():
    F = 7019
    g32, gq, first = item_bounds(F, GROUPS_EIGHT_WAVES)
    assert (g32, gq) == (220, 14)
    assert sorted(set(np.diff(first))) == [15, 16]
    item, n_items, n_groups, wave, t, half, wg = place(F, 260, GROUPS_EIGHT_WAVES)
    assert (item, n_items, wave, half, wg) == (0, 14, 4, 1, 0) and n_groups == 15
    item, n_items, n_groups, wave, t, half, wg = place(F, 7018, GROUPS_EIGHT_WAVES)
    assert (item, wave, t, wg) == (13, 7, 1, 13) and n_groups == 16
    # the four-consumer bodies: items of 8 view groups, waves 0-3
    item, n_items, n_groups, wave, t, half, wg = place(F, 260, GROUPS_FOUR_CONSUMERS)
    assert n_items == 28 and (item, wave, t) == (1, 0, 1) and n_groups == 8


@pytest.mark.parametrize("gpi", [GROUPS_EIGHT_WAVES, GROUPS_FOUR_CONSUMERS])
@pytest.mark.parametrize("F", [89, 305, 7019, 41013, 140007])
def test_every_view_has_one_place(F, gpi):
    g32, gq, first = item_bounds(F, gpi)
    sizes = np.diff(first)
    assert first[0] == 0 and first[-1] == g32 and gq == -(-g32 // gpi)
    assert sizes.max() - sizes.min() <= 1 and sizes.max() <= gpi and sizes.min() >= 1
    seen = {}
    for group in range((F + 31) // 32):
        v0 = group * 32
        item, n_items, n_groups, wave, t, half, wg = place(F, v0, gpi)
        assert n_items == gq and n_groups == sizes[item] and wg == item % 256
        assert 0 <= wave < gpi // 2 and t in (0, 1) and first[item] + 2 * wave + t == group
        assert seen.setdefault((item, wave, t), group) == group          # one view group per (item, wave, t) ...
        for v in range(v0, min(F, v0 + 32)):                             # ... and every view of the group in it, in the half of bit 2
            assert place(F, v, gpi) == (item, n_items, n_groups, wave, t, (v % 32) // 4 % 2, wg)
    assert len(seen) == (F + 31) // 32
    with pytest.raises(ValueError):
        place(F, F, gpi)


def test_more_items_than_workgroups_wrap():
    F = 132500
    item, n_items, _, _, _, _, wg = place(F, F - 1, GROUPS_EIGHT_WAVES)
    assert n_items == 259 and item == 258 and wg == 2
    assert place(F, 131008, GROUPS_EIGHT_WAVES)[0] == 256 and place(F, 131008, GROUPS_EIGHT_WAVES)[6] == 0
    assert place(F, 131007, GROUPS_EIGHT_WAVES)[0] == 255


def test_tied_pair_sums():
    """Y and Z differ from X by integer sums (254, 0) and (0, 127): 0.25 * 254 == 0.5 * 127 at chem_weight 0.5 only."""
    x = fresh_view(9)
    y, z = tied_pair(x)
    s_hs, s_v = oracle.int_sums(np.stack([y, z]), x)
    assert (list(s_hs), list(s_v)) == ([254, 0], [0, 127])
    fam = oracle.sads_hsv(np.stack([y, z]), x, 0.5)
    assert fam[0] == fam[1] == 1023.7509803921569
    fam = oracle.sads_hsv(np.stack([y, z]), x, 0.25)
    assert abs(abs(fam[0] - fam[1]) - 0.249) < 1e-3


def test_rows_give_the_oracle_step():
    """The GPU tests take their expectations from oracle.sads_hsv rows (scored once per patch): the same record as oracle.step, first
    maxima included, and clear_headings names the headings whose best view is unique or a planted tie."""
    lib = synth.synth_views(5, 300, 8, 8)
    lib[40] = lib[210] = lib[7]                                  # copies: the first one is the view
    pats = synth.synth_patches(6, 5, 8, 8)
    pats[1] = pats[3] = lib[7]                                   # and the first heading the best
    for cw in (0.0, 0.25, 1.0):
        rows = oracle_rows("host", lib, pats, cw)
        want, got = oracle.step(lib, pats, cw), step_of_rows(rows)
        assert (got["best_idex"], got["best_view"], got["step_familiarity"]) == (want["best_idex"], want["best_view"], want["step_familiarity"])
        assert (got["best_idex"], got["best_view"]) == (1, 7)
        assert np.array_equal(got["angle_familiarity"], want["angle_familiarity"])
        assert np.array_equal(got["scene_familiarity"], want["scene_familiarity"])
        assert not clear_headings(rows)[[1, 3]].any() and clear_headings(rows, (1, 3))[[1, 3]].all()
