"""The fp4 body with the library rows in registers (k_sad_mfma_dual with SKL = 8: sad_lc_fp4_lreg) keeps its register ring in
registers: no scratch, at most 256 VGPRs, in its fused and unfused forms (read from the built code object like
tests/test_host_logic.py:test_shipped_scoring_kernels_use_no_scratch)."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_register_body_uses_no_scratch():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.kernel_table()
    for name in ("k_sad_mfma_dual<4, 2, 2, 4, 1, true, 8, 3, false, 1>", "k_sad_mfma_dual<4, 2, 2, 4, 1, false, 8, 3, false, 1>"):
        row = [r for r in rows if r["name"] == name]
        assert row, name
        assert row[0]["scratch"] == 0 and row[0].get("vgpr_spills", 0) == 0 and row[0]["vgpr"] <= 256, row[0]
