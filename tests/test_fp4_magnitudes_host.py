"""The fp4 coefficient image's convention (csrc/dejavu_kernels.h, k_patch_prep and the fp4 scoring bodies), as arithmetic on the CPU:
the coefficient nibble of bit position b carries the inverse of the E2M1 value the library bit stands for where the bodies leave
it -- positions 0 / 1 / 2 in place (0.5 / 1 / 2), position 3 brought down to bit 0 (0.5) -- so every product is +-1 and the
accumulators hold signed counts, whichever positions share one."""
import numpy as np

E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0])
COEF_NIBBLE = {0: (0x4, 0xC), 1: (0x2, 0xA), 2: (0x1, 0x9), 3: (0x4, 0xC)}      # bit position -> (+, -): 2.0, 1.0, 0.5, 2.0
M = 0x11111111


def nibbles(x):
    """The eight nibbles of every dword as E2M1 values, [..., 8]."""
    x = np.asarray(x, dtype=np.uint32)
    return E2M1[(x[..., None] >> (4 * np.arange(8, dtype=np.uint32))) & 0xF]


def dot(lib_dwords, coef_dwords):
    """What the fp4 matrix instruction adds for these K-elements: the sum of the nibbles' products."""
    return float((nibbles(lib_dwords) * nibbles(coef_dwords)).sum())


def thermometer_operands(x):
    """The four operand dwords of a thermometer row's dword x, one per bit position."""
    x = np.asarray(x, dtype=np.uint32)
    return [x & np.uint32(M), x & np.uint32(M << 1), x & np.uint32(M << 2), (x >> np.uint32(3)) & np.uint32(M)]


def code_operands(x):
    """The four operand dwords of a code row's dword x (3-bit codes b2 b1 b0 in the nibbles): planes t1..t4."""
    x = np.asarray(x, dtype=np.uint32)
    xr = x >> np.uint32(1)
    return [(x | xr) & np.uint32(M), x & np.uint32(M << 1), x & np.uint32(M << 2), (x & xr) & np.uint32(M)]


def coef_rows(sign_bits):
    """The coefficient dwords of the four bit positions for [4][8] signs (True: minus), as k_patch_prep writes them."""
    rows = []
    for pos in range(4):
        d = 0
        for i in range(8):
            d |= COEF_NIBBLE[pos][1 if sign_bits[pos][i] else 0] << (4 * i)
        rows.append(np.uint32(d))
    return rows


def test_every_product_is_plus_or_minus_one():
    for pos in range(4):
        lib_nibble = 1 << pos
        (op,) = [o for s, o in enumerate(thermometer_operands(np.uint32(lib_nibble))) if s == pos]
        assert E2M1[int(op) & 0xF] == (0.5, 1.0, 2.0, 0.5)[pos]
        for sign, nib in zip((1.0, -1.0), COEF_NIBBLE[pos]):
            assert E2M1[int(op) & 0xF] * E2M1[nib] == sign
        # a position's operand holds nothing of the other positions' bits, in its own nibble or from the nibble above
        others = np.uint32((0xF ^ lib_nibble) * M)
        assert int(thermometer_operands(others)[pos]) == 0


def gap_planes(levels):
    """Planes of a byte plane with these levels: one per gap, a gap wider than 127 split for the int8 form into copies with the
    same library bit.  (lo, w) per plane for the int8 form; wfull: the whole gap on the first plane of a gap, 0 on its copies."""
    lo, w, wfull = [], [], []
    for a, b in zip(levels, levels[1:]):
        parts = -(-(b - a) // 127)
        edges = np.round(np.linspace(a, b, parts + 1)).astype(int)
        for k in range(parts):
            lo.append(int(edges[k])); w.append(int(edges[k + 1] - edges[k])); wfull.append(b - a if k == 0 else 0)
    return lo, w, wfull


def check_plane_set(levels, rng):
    lo, w, wfull = gap_planes(levels)
    T = len(lo)
    firsts = [t for t in range(T) if wfull[t]]
    gap_lo = {t: lo[t] for t in firsts}
    n_px = 64                                               # T * 64 K-elements: whole dwords, planes on every position they reach
    n_el = n_px * T
    assert n_el % 32 == 0
    # widths per bit position (planes on one position agree, or the position holds copies only), then per accumulator class
    wpos = [0, 0, 0, 0]
    for n in range(n_el):
        t = n % T
        if wfull[t]:
            assert wpos[n % 4] in (0, wfull[t])
            wpos[n % 4] = wfull[t]
    w_cls = [wpos[0], max(wpos[1:])]
    assert all(x in (0, w_cls[1]) for x in wpos[1:])
    lib_px = rng.choice(levels, n_px)
    on_levels = sorted(set(levels) | {0, 255})
    for a_fixed in on_levels + [None]:
        if a_fixed is not None and levels[0] < a_fixed < levels[-1] and a_fixed not in levels:
            continue
        pat_px = rng.choice(levels, n_px) if a_fixed is None else np.full(n_px, a_fixed)
        want = 0
        lib_dw = np.zeros(n_el // 32, dtype=np.uint32)
        signs = np.zeros((n_el // 32, 4, 8), dtype=bool)
        live = np.zeros((n_el // 32, 4, 8), dtype=bool)
        for n in range(n_el):
            p, t = n // T, n % T
            lib_bit = 1 if lib_px[p] >= lo[t] + w[t] else 0
            alpha = min(max(int(pat_px[p]) - lo[t], 0), w[t])
            want += lib_bit * (w[t] - 2 * alpha)            # the int8 form's term
            j, beta = n // 32, n % 32
            lib_dw[j] |= np.uint32(lib_bit << beta)        # the tiles are the int8 form's: copies keep their bits
            if wfull[t]:
                assert pat_px[p] <= gap_lo[t] or pat_px[p] >= gap_lo[t] + wfull[t]      # on a level: the coefficient is +-w
                signs[j, beta & 3, beta >> 2] = pat_px[p] - gap_lo[t] >= wfull[t]
                live[j, beta & 3, beta >> 2] = True
        acc = [0.0, 0.0]
        for j in range(n_el // 32):
            rows = coef_rows(signs[j])
            for pos in range(4):                            # copies of a split gap stay zero in the image
                keep = sum(0xF << (4 * i) for i in range(8) if live[j, pos, i])
                rows[pos] = rows[pos] & np.uint32(keep)
            ops = thermometer_operands(lib_dw[j])
            for pos in range(4):
                d = dot(ops[pos], rows[pos])
                assert d == int(d)
                acc[1 if pos else 0] += d
        got = w_cls[0] * int(acc[0]) + w_cls[1] * int(acc[1])
        assert got == want, (levels, a_fixed, got, want)


def test_sums_equal_the_int8_form():
    rng = np.random.default_rng(8)
    check_plane_set([0, 63, 127, 191, 255], rng)            # five-level value plane: widths 63 | 64, 64, 64
    check_plane_set([0, 127], rng)                          # two-level saturation plane
    check_plane_set([0, 255], rng)                          # a split gap: first plane full width, copies zero
    check_plane_set([0, 85, 170, 255], rng)                 # three planes per pixel: every plane visits every position
    check_plane_set([3, 200], rng)


def test_split_gap_first_plane_stands_for_the_gap():
    lo, w, wfull = gap_planes([0, 255])
    assert len(lo) == 3 and sum(w) == 255 and max(w) <= 127 and wfull == [255, 0, 0]


def test_body_names_agree_between_header_host_and_binding():
    """scoring_form()["body"] indexes the binding's list with the number the host makes from its enum: one order in all three."""
    import os
    import re
    from navsim_amd import _native as N
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "dejavu.h")).read()
    host = open(os.path.join(root, "navigation-by-deja-vu_amd", "csrc", "dejavu_hip.hip")).read()
    names = re.search(r'#define DV_FORM_BODY_NAMES "([^"]+)"', header).group(1).split()
    enum = [s.strip() for s in re.search(r"enum class Body \{([^}]+)\}", host).group(1).split(",")]
    assert enum[-1] == "Count" and enum[:-1] == names == N.DV_FORM_BODY_NAMES
    assert int(re.search(r"#define DV_FORM_BODY_SHIFT (\d+)", header).group(1)) == N.DV_FORM_BODY_SHIFT
    assert int(re.search(r"#define DV_FORM_BODY_BITS (\d+)", header).group(1)) == N.DV_FORM_BODY_BITS
    assert len(names) < (1 << N.DV_FORM_BODY_BITS)


def test_code_rows_decode_to_thermometer_planes():
    code = {0: 0b000, 1: 0b001, 2: 0b010, 3: 0b110, 4: 0b111}
    for level, cbits in code.items():
        b0, b1, b2 = cbits & 1, (cbits >> 1) & 1, (cbits >> 2) & 1
        assert [b0 | b1, b1, b2, b0 & b1] == [int(level >= t) for t in (1, 2, 3, 4)]
    # the same on packed dwords, with the coefficient rows: every product +-1, the sums those of the thermometer planes
    rng = np.random.default_rng(9)
    levels = rng.integers(0, 5, (16, 8))
    signs = rng.integers(0, 2, (16, 4, 8)).astype(bool)
    for j in range(16):
        x = np.uint32(sum(code[int(l)] << (4 * i) for i, l in enumerate(levels[j])))
        ops, rows = code_operands(x), coef_rows(signs[j])
        for s in range(4):
            want = sum((-1 if signs[j, s, i] else 1) * int(levels[j, i] >= s + 1) for i in range(8))
            assert dot(ops[s], rows[s]) == want
            vals = nibbles(ops[s])
            assert set(np.abs(vals).tolist()) <= {0.0, (0.5, 1.0, 2.0, 0.5)[s]}
