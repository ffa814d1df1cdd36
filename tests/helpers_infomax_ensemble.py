"""Inputs of the Infomax ensemble tests (tests/test_infomax_ensemble_host.py, tests/test_gpu_infomax_ensemble.py): the patch sets of
every case and member layout, and the NumPy restatement (tests/helpers_infomax.py) on them, computed once.

A patch set is uint8[n, A, h, w]: windows of a random 5-level strip that the case's model has not seen (novel), and in it
  - every member but the planted one carries ONE trained view, at heading (3 i + 1) % A of member i, so that its best heading is
    decided by the model and not by the order of the patches;
  - the planted member (the last one, in layouts of at least 8 headings) carries the SAME trained view -- the one the restatement finds
    most familiar -- at headings 2 and 7 and novel patches everywhere else: two equal maxima, of which np.argmax takes the first.
    The small models do not separate trained from novel views (under the 5x3 model half the novel windows score above every
    trained view), so this member's novel patches are the first windows of a strip of their own that the restatement scores at
    least 1e-3 (relative) below the planted view.
The seeds are chosen in the host test so that every member's best heading leads its second best by more than 1000 TOL."""
import functools

import numpy as np

from tests import helpers_infomax as H

# the last two: more than 64 row tiles, so k_im_decide's sum over a column's tiles takes a second trip (as k_im_dfinish's does)
KEYS = ("20x13", "40x1", "5x3_f2", "16x16_a16", "7x5_m1043", "32x32_m1040")
# (n_agents, A): a single member; one heading per member; 65 columns, member 4 straddles a column block; 180 columns, ragged last
# block; a member wider than a block
LAYOUTS = ((1, 16), (7, 1), (5, 13), (3, 60), (2, 65))
SEED = 5000                                                        # of the novel strips (tests/test_infomax_ensemble_host.py holds it)


def planted_member(n, A):
    return n - 1 if A >= 8 else None


@functools.lru_cache(maxsize=None)
def ensemble_data(key, n, A):
    """dict(planes uint8[n,A,h,w], fam float64[n,A] (the restatement's), planted (member or None), W)."""
    d = H.case_data(key)
    planes = H.route_views(SEED + d["seed"] * 100 + n * 7 + A, n * A, d["h"], d["w"]).reshape(n, A, d["h"], d["w"]).copy()
    planted = planted_member(n, A)
    for i in range(n):
        if i == planted:
            fam_views = H.familiarity(d["W"], d["views"])
            top = int(np.argmax(fam_views))
            pool = H.route_views(SEED + 1 + d["seed"] * 100 + n * 7 + A, 40 * A, d["h"], d["w"])
            # the first A such windows (familiarities are negative), the pool scored no further than they take
            below = np.empty((0, d["h"], d["w"]), dtype=np.uint8)
            for p0 in range(0, len(pool), A):
                part = pool[p0:p0 + A]
                below = np.concatenate([below, part[H.familiarity(d["W"], part) < fam_views[top] * (1 + 1e-3)]])[:A]
                if len(below) == A:
                    break
            assert len(below) == A
            planes[i] = below
            planes[i, 2] = planes[i, 7] = d["views"][top]
        else:
            planes[i, (3 * i + 1) % A] = d["views"][(5 * i + 1) % d["F"]]
    fam = H.familiarity(d["W"], planes.reshape(n * A, d["h"], d["w"])).reshape(n, A)
    planes.setflags(write=False)
    fam.setflags(write=False)
    return dict(planes=planes, fam=fam, planted=planted, W=d["W"], h=d["h"], w=d["w"], W0=d["W0"])
