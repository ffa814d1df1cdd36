"""The k_rvncc_* kernels of the built library, exactly, and their budget: no scratch, no spills, at most 128 VGPRs, at most 64 KB of LDS
(read from the code object by tools/kernel_resources.py; no compile and no device)."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

KERNELS = ("k_rvncc_stats", "k_rvncc_prep", "k_rvncc_score<0>", "k_rvncc_score<1>", "k_rvncc_pick", "k_rvncc_best", "k_rvncc_rows")


def test_every_rvncc_kernel_has_no_scratch_no_spills_and_at_most_128_vgprs():
    import kernel_resources
    rows = [r for r in kernel_resources.kernel_table() if r["name"].startswith("k_rvncc_")]
    assert sorted(r["name"] for r in rows) == sorted(KERNELS)
    for r in rows:
        print("%-20s VGPR %3d SGPR %3d scratch %d spills %d LDS %d" % (r["name"], r["vgpr"], r["sgpr"], r["scratch"], r.get("vgpr_spills", 0),
                                                                        r["lds"]))
        assert r["scratch"] == 0 and r.get("vgpr_spills", 0) == 0 and r["vgpr"] <= 128, r
        assert r["lds"] <= 64 * 1024, r
