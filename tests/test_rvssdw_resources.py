"""The kernels of windowed SSD on the route view store (dejavu_rvssdw.inl) use no scratch, spill nothing and stay inside the LDS they
declare (read from the built library's code-object metadata by tools/kernel_resources.py, like tests/test_rvssd_resources.py: no
compile and no device).  The scoring kernel's LDS is the four waves' minima, [4][32] 64-bit keys; the planning kernel's its four wave
counts, as k_rvreloc_plan's; the whole-route scoring on the plan is k_rvssd_score<0>'s body and costs what that kernel costs."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_rvssdw_score", "k_rvssdw_plan", "k_rvssdw_whole", "k_rvssdw_unsort")


def test_the_windowed_ssd_kernels_use_no_scratch_and_the_lds_they_declare():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.kernel_table()
    assert sorted(r["name"] for r in rows if r["name"].startswith("k_rvssdw")) == sorted(KERNELS)
    by_name = {r["name"]: r for r in rows}
    for name in KERNELS:
        row = by_name[name]
        print("%-18s VGPR %3d SGPR %3d scratch %d spills %d LDS %d" % (name, row["vgpr"], row["sgpr"], row["scratch"], row.get("vgpr_spills", 0),
                                                                      row["lds"]))
        assert row["scratch"] == 0 and row.get("vgpr_spills", 0) == 0 and row.get("sgpr_spills", 0) == 0, row
    assert by_name["k_rvssdw_score"]["lds"] == 4 * 32 * 8 and by_name["k_rvssdw_plan"]["lds"] == by_name["k_rvreloc_plan"]["lds"] == 16
    assert by_name["k_rvssdw_whole"]["lds"] == 0 and by_name["k_rvssdw_unsort"]["lds"] == 0
    assert by_name["k_rvssdw_whole"]["vgpr"] <= by_name["k_rvssd_score<0>"]["vgpr"] + 8 <= 128
