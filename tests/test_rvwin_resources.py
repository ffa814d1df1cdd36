"""The fused windowed kernel (dejavu_rvwin.inl) keeps its sums in registers: no scratch, no spills, at most 128 VGPRs in every
instantiation (read from the built code object like tests/test_rviews_resources.py); it has no static LDS: the patches' planes, the
fast scores and the partial sums are dynamic."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_rvwin_score<0>", "k_rvwin_score<1>")


def test_the_windowed_kernel_uses_no_scratch():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.kernel_table()
    assert sorted(r["name"] for r in rows if r["name"].startswith("k_rvwin")) == sorted(KERNELS)   # every instantiation
    for name in KERNELS:
        row = [r for r in rows if r["name"] == name][0]
        assert row["scratch"] == 0 and row.get("vgpr_spills", 0) == 0 and row["vgpr"] <= 128, row
        assert row["lds"] == 0, row
