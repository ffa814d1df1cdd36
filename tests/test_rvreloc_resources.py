"""The kernels of the re-localisation inside the windowed step (dejavu_rvreloc.inl) use no scratch and spill nothing, in every
instantiation (read from the built code object like tests/test_rvwin_resources.py).  The planning kernel's static LDS is its four wave
counts; the scoring kernel's patch tile is dynamic, as k_rv_score's; the picking kernels' static LDS is k_rv_pick's."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_rvreloc_plan", "k_rvreloc_score", "k_rvreloc_exact", "k_rvreloc_pick<0>", "k_rvreloc_pick<1>")


def test_the_relocalising_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.kernel_table()
    assert sorted(r["name"] for r in rows if r["name"].startswith("k_rvreloc")) == sorted(KERNELS)   # every instantiation
    by_name = {r["name"]: r for r in rows}
    for name in KERNELS:
        row = by_name[name]
        assert row["scratch"] == 0 and row.get("vgpr_spills", 0) == 0 and row["vgpr"] <= 128, row
    assert by_name["k_rvreloc_plan"]["lds"] == 16 and by_name["k_rvreloc_score"]["lds"] == 0
    for k in (0, 1):                                                                      # the shared bodies cost the same in both kernels
        assert by_name["k_rvreloc_pick<%d>" % k]["lds"] == by_name["k_rv_pick<%d>" % k]["lds"]
    assert by_name["k_rvreloc_score"]["vgpr"] <= by_name["k_rv_score"]["vgpr"] + 8
