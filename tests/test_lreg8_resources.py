"""The register-ring fp4 body with eight consumer waves (k_sad_mfma_dual with SKL = 88: sad_lc_fp4_lreg8) issues its library
loads and its LDS-DMA behind the compiler's back and counts its waits by hand, which is only right while the ring stays in
registers: no scratch, no spills, at most 256 VGPRs, fused and unfused (read from the built code object like
tests/test_libreg_code_resources.py)."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eight_consumer_body_uses_no_scratch():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.kernel_table()
    for name in ("k_sad_mfma_dual<4, 2, 2, 4, 1, true, 88, 3, true, 1>", "k_sad_mfma_dual<4, 2, 2, 4, 1, false, 88, 3, true, 1>"):
        row = [r for r in rows if r["name"] == name]
        assert row, name
        assert row[0]["scratch"] == 0 and row[0].get("vgpr_spills", 0) == 0 and row[0]["vgpr"] <= 256, row[0]
