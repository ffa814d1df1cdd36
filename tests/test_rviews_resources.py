"""The route-view kernels (dejavu_rviews.inl) keep their sums in registers: no scratch, no spills (read from the built code object like
tests/test_libreg_resources.py), and k_rv_pick's candidate list and reduction arrays are its only static LDS."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_rv_planes", "k_rv_prep", "k_rv_score", "k_rv_exact", "k_rv_pick<0>", "k_rv_pick<1>", "k_rv_best", "k_rv_scene")


def test_route_view_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.kernel_table()
    for name in KERNELS:
        row = [r for r in rows if r["name"] == name]
        assert row, name
        assert row[0]["scratch"] == 0 and row[0].get("vgpr_spills", 0) == 0 and row[0]["vgpr"] <= 128, row[0]
    assert [r for r in rows if r["name"] == "k_rv_score"][0]["lds"] == 0                  # (its patch tile is dynamic: 48 KiB at most)
