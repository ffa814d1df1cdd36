"""The network-table kernels (dejavu_inet.inl) are the Infomax device functions on a descriptor's values: every one keeps its banked
twin's budget -- no scratch, no spills, no more vector registers than the twin and no more static LDS (k_inet_prep is held to k_im_prep,
whose body im_prep_view restates).  Read from the built code object like tests/test_mbpop_resources.py."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWINS = {"k_inet_prep": "k_im_prep", "k_inet_gemv": "k_im_gemv_banks", "k_inet_upart": "k_im_upart_banks", "k_inet_ureduce": "k_im_ureduce_banks",
         "k_inet_update": "k_im_update_banks", "k_inet_finite": "k_im_finite_banks", "k_inet_score_cols<false>": "k_im_score_cols_banks<false>",
         "k_inet_score_cols<true>": "k_im_score_cols_banks<true>", "k_inet_decide": "k_im_decide_banks"}


def test_the_network_kernels_keep_their_twins_budget():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = {r["name"]: r for r in kernel_resources.kernel_table()}
    assert sorted(n for n in rows if n.startswith("k_inet")) == sorted(TWINS)             # every kernel and instantiation
    assert sorted(TWINS) == sorted(r["name"] for r in kernel_resources.group_rows("inet") if r["name"].startswith("k_inet"))
    for name, twin in TWINS.items():
        row, old = rows[name], rows[twin]
        assert row["scratch"] == 0 and row.get("vgpr_spills", 0) == 0, row
        assert row["lds"] <= old["lds"], (row, old)
        assert row["vgpr"] <= old["vgpr"], (row, old)
