"""The bank-set kernels (dejavu_mbset.inl) are mb_view with the set's read-out in pass 2: every instantiation keeps the k_mb* family's
budget -- no scratch (the S accumulators are unrolled under a uniform predicate, so no register array is indexed at run time), no
spills, at most 64 VGPRs (8 waves a SIMD, as k_mb*), and no static LDS beyond its twin's: the plane, the histograms, the hand-over
words and the wave totals are dynamic; the sensed forms keep the one barrier-reduction word block k_mb_pose has, and k_mbset_decide the
three arrays of k_mb_decide_batch.  Read from the built code object like tests/test_mbpop_resources.py."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# SRC bits (dejavu_mbset.inl): 1 pose, 2 landscape set, 4 sensor table, 8 noise rows
TWINS = {"k_mbset<0>": "k_mb_bank<1>", "k_mbset<1>": "k_mb_pose_bank", "k_mbset<3>": "k_mb_pose_bank_lands",
         "k_mbset<7>": "k_mb_pose_bank_lands_sensors", "k_mbset<11>": "k_mb_pose_bank_lands_noise",
         "k_mbset<15>": "k_mb_pose_bank_lands_sensors_noise", "k_mbset_decide": "k_mb_decide_batch"}


def test_the_set_kernels_keep_the_familys_budget():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = {r["name"]: r for r in kernel_resources.kernel_table()}
    assert sorted(n for n in rows if n.startswith("k_mbset")) == sorted(TWINS)            # every instantiation
    for name, twin in TWINS.items():
        row, old = rows[name], rows[twin]
        assert row["scratch"] == 0 and row.get("vgpr_spills", 0) == 0, row
        assert row["vgpr"] <= 64, row
        assert row["lds"] <= old["lds"], (row, old)
