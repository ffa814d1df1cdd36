"""The population-table kernels (dejavu_mbpop.inl) are mb_view on a descriptor's values: every instantiation keeps k_mb*'s budget -- no
scratch, no spills, no more registers than its twin without a table, and no static LDS beyond its twin's (the plane, the histograms and
the hand-over words are dynamic; the sensed forms keep the one barrier-reduction word block k_mb_pose has).  Read from the built code
object like tests/test_rvwin_resources.py."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWINS = {"k_mbpop_bank<0>": "k_mb_bank<0>", "k_mbpop_bank<1>": "k_mb_bank<1>", "k_mbpop_pose_bank": "k_mb_pose_bank",
         "k_mbpop_pose_bank_lands": "k_mb_pose_bank_lands", "k_mbpop_pose_bank_lands_sensors": "k_mb_pose_bank_lands_sensors",
         "k_mbpop_count": "k_mb_count"}


def test_the_population_kernels_keep_their_twins_budget():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = {r["name"]: r for r in kernel_resources.kernel_table()}
    assert sorted(n for n in rows if n.startswith("k_mbpop")) == sorted(TWINS)            # every instantiation
    for name, twin in TWINS.items():
        row, old = rows[name], rows[twin]
        assert row["scratch"] == 0 and row.get("vgpr_spills", 0) == 0, row
        assert row["lds"] <= old["lds"], (row, old)
        assert row["vgpr"] <= old["vgpr"] and row["vgpr"] <= 64, (row, old)               # (8 waves a SIMD, as k_mb*)
