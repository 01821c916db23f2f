"""Host model of the probe kernels (``ops/csrc/gpu_probe.hip``), in numpy and plain Python.

Written from the formulas the kernel comments state, not by calling the library: the HBM
pattern (``mix32`` / ``pattern16``), the integer-valued probe operands and their product, the
device-side seed LCG of the graph path, and one iteration of ``busy_kernel`` through the
operand and C/D layouts of ``v_mfma_f32_32x32x16_bf16``.  Everything here is integer
arithmetic (or float64 on integers far below 2^53), so the GPU tests compare bit-exactly.
"""

import numpy as np

N_XCD = 8
PERIOD = 35  # lcm(5, 7): the probe operands repeat in k with this period


# ------------------------------------------------------------------ HBM pattern


def mix32(x):
    """The 32-bit finaliser of the pattern, elementwise on uint32 (wraps modulo 2^32)."""
    x = np.array(x, dtype=np.uint32, copy=True)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def pattern_words(n16, seed):
    """The ``4 * n16`` uint32 words of pattern elements 0 .. n16-1: element ``i`` is
    ``mix32(b), mix32(b + 1), mix32(b + 2), mix32(b + 3)`` with ``b = uint32(4 i) ^ seed``."""
    i = np.arange(n16, dtype=np.uint64)
    b = ((i * np.uint64(4)) & np.uint64(0xFFFFFFFF)).astype(np.uint32) ^ np.uint32(seed & 0xFFFFFFFF)
    words = np.empty((n16, 4), dtype=np.uint32)
    for lane in range(4):
        words[:, lane] = mix32(b + np.uint32(lane))  # uint32 addition wraps
    return words.reshape(-1)


def lcg(seed):
    """One step of the graph path's on-device seed."""
    return (seed * 1664525 + 1013904223) & 0xFFFFFFFF


# ------------------------------------------------------------------ probe GEMM


def probe_operands(m, n, k):
    """``A[i][k] = ((3i + 7k) mod 5) - 2`` and ``Bt[j][k] = ((11j + 5k) mod 7) - 3`` as int64."""
    kk = np.arange(k, dtype=np.int64)[None, :]
    a = (3 * np.arange(m, dtype=np.int64)[:, None] + 7 * kk) % 5 - 2
    bt = (11 * np.arange(n, dtype=np.int64)[:, None] + 5 * kk) % 7 - 3
    return a, bt


def probe_expected(m, n, k):
    """``A · Btᵀ`` of the probe operands as an exact int64 product."""
    a, bt = probe_operands(m, n, k)
    return a @ bt.T


def probe_class_table(k):
    """The closed form: the 5 × 7 table ``t`` with ``C[i][j] = t[i mod 5][j mod 7]``.

    Both operands have period 35 in k, so with ``K = 35 q + rem`` the first ``rem`` residues
    of k occur ``q + 1`` times and the others ``q`` times."""
    q, rem = divmod(k, PERIOD)
    t = np.zeros((5, 7), dtype=np.int64)
    for i in range(5):
        for j in range(7):
            t[i, j] = sum((q + (1 if r < rem else 0)) * ((3 * i + 7 * r) % 5 - 2) * ((11 * j + 5 * r) % 7 - 3)
                          for r in range(PERIOD))
    return t


def probe_expected_closed_form(m, n, k):
    t = probe_class_table(k)
    return t[np.arange(m)[:, None] % 5, np.arange(n)[None, :] % 7]


def zero_classes(k):
    """How many of the 35 ``(i mod 5, j mod 7)`` classes expect 0: the check cannot tell a
    correct product from an all-zero one there."""
    return int((probe_class_table(k) == 0).sum())


def fused_tile_id(tm, tn, tiles_m, tiles_n, gm=1):
    """The tile id (index into ``tile_xcd``) that computes output tile ``(tm, tn)`` in the 256²
    kernels: row-major, or with grouping ``gm`` (when it divides ``tiles_m``) consecutive ids
    walking ``gm`` tile-rows before the next column of the band."""
    if gm > 1 and tiles_m % gm == 0:
        return (tm // gm) * gm * tiles_n + tn * gm + tm % gm
    return tm * tiles_n + tn


def tile128_id(tm, tn, tiles_n):
    """The tile id of output tile ``(tm, tn)`` in the 128² store kernel and its check kernel: row-major."""
    return tm * tiles_n + tn


def line_errors(other, c, tile):
    """One operand element at k = ``c`` off by a non-zero amount makes its line of C (a row for an
    element of A, a column for one of Bt) wrong exactly where the other operand ``other[:, c]`` is not 0.
    Returns the count and the counts per ``tile`` elements along the line."""
    bad = other[:, c] != 0
    return int(bad.sum()), bad.reshape(-1, tile).sum(axis=1).tolist()


def errors_by_xcd(per_tile, xcds):
    """``per_tile[t]`` mismatches in a tile that ran on XCD ``xcds[t]``, summed per XCD."""
    out = [0] * N_XCD
    for count, xcd in zip(per_tile, xcds):
        out[int(xcd)] += int(count)
    return out


# ------------------------------------------------------------------ the resident probe's harness


GRAPH_SEED0 = 0x1E3779B9  # the device-side seed before the first replay
EAGER_SEED0 = 0x9E3779B9  # the host-side seed before the first eager run


def lcg_sequence(seed, n):
    """The seeds of runs 1 .. n from the start value ``seed``."""
    out = []
    for _ in range(n):
        seed = lcg(seed)
        out.append(seed)
    return out


def u64(h, i):
    """The u64 in the i32 slots ``i`` and ``i + 1`` of a counter block."""
    return (int(h[i]) & 0xFFFFFFFF) | ((int(h[i + 1]) & 0xFFFFFFFF) << 32)


def graph_span(h, slot):
    """``(begin, end)`` in ticks of a span of the graph layout: ``~begin`` in slots ``slot`` and
    ``slot + 1`` (so that a zeroed slot works with an atomic max), ``end`` in the next two."""
    return ~u64(h, slot) & 0xFFFFFFFFFFFFFFFF, u64(h, slot + 2)


def sweep_workgroups(n16):
    """Workgroups of the pattern sweep over ``n16`` elements: one per 1024, at most 4096."""
    return max(1, min(4096, -(-n16 // 1024)))


def link_flips(words, inside, seed, count=200):
    """Seeded places to corrupt in a buffer of ``words`` words of which a reader checks the first
    ``inside``: the first and the last word of the buffer, both words at the boundary, and ``count``
    random ones on either side of it.  Returns sorted positions and a non-zero int32 to XOR into each."""
    rng = np.random.default_rng(seed)
    pos = {0, words - 1, inside - 1}
    pos.update(rng.choice(inside, size=min(count, inside), replace=False).tolist())
    if inside < words:
        pos.add(inside)
        pos.update((inside + rng.choice(words - inside, size=min(count, words - inside), replace=False)).tolist())
    pos = np.array(sorted(pos), dtype=np.int64)
    return pos, rng.integers(1, 1 << 31, size=pos.size, dtype=np.int64).astype(np.int32)


# ------------------------------------------------------------------ f16: value against value


def f16_values():
    """256 half bit patterns (uint16) for the one-hot f16 case: the integers -8 .. 8, ±65504, the
    smallest normal, ±0, the all-ones mantissa of every normal exponent, and seeded random normal
    patterns in 0x0400 .. 0x7bff for the rest.  No subnormal, inf or NaN."""
    fixed = [np.arange(-8, 9).astype(np.float16).view(np.uint16), np.array([0x7BFF, 0xFBFF, 0x0400, 0x0000, 0x8000]),
             (np.arange(1, 31) << 10) | 0x03FF]
    fixed = np.concatenate([np.asarray(x, dtype=np.uint16) for x in fixed])
    rng = np.random.default_rng(160016)
    rest = rng.integers(0x0400, 0x7C00, size=256 - fixed.size, dtype=np.uint16)
    return np.concatenate([fixed, rest])


def f16_onehot_case():
    """Every value of ``f16_values`` against every value, 256 × 256 at one stage (K = 32):
    ``A[i][k]`` is value ``i`` at ``k = i % 32`` and +0 elsewhere, ``Bt[j][k]`` is value ``j`` at
    every k.  Each output is one product of two halves: 22 significant bits, exact in fp32 (and
    in the float64 computed here).  Returns ``a, bt`` (float16) and ``want`` (float64)."""
    v = f16_values()
    i = np.arange(256)
    a = np.zeros((256, 32), dtype=np.uint16)
    a[i, i % 32] = v
    bt = np.repeat(v[:, None], 32, axis=1)
    x = v.view(np.float16).astype(np.float64)
    return a.view(np.float16), bt.view(np.float16), x[:, None] * x[None, :]


# ------------------------------------------------------------------ busy kernel


def busy_expected():
    """Per-lane output (64 values) of one ``busy_kernel`` iteration.

    Each lane holds ``a[e] = (lane + e) & 3`` and ``b[e] = (3 lane + e) & 3``.  As the first or
    second MFMA operand a register vector is a 32 × 16 matrix: row (first operand) or column
    (second) ``lane & 31``, ``k = 8 (lane >> 5) + e``.  The four accumulators are ``a·b``,
    ``b·a``, ``a·a`` and ``b·b``; a lane's 16 result registers are column ``lane & 31``, rows
    ``(reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)``, and the kernel stores their sum."""
    va = np.zeros((32, 16), dtype=np.int64)  # [row or column][k]
    vb = np.zeros((32, 16), dtype=np.int64)
    for lane in range(64):
        for e in range(8):
            va[lane & 31, 8 * (lane >> 5) + e] = (lane + e) & 3
            vb[lane & 31, 8 * (lane >> 5) + e] = (lane * 3 + e) & 3
    # D[row][col] = sum_k first[row][k] * second[col][k]
    d = va @ vb.T + vb @ va.T + va @ va.T + vb @ vb.T
    out = np.zeros(64, dtype=np.int64)
    for lane in range(64):
        col = lane & 31
        for reg in range(16):
            out[lane] += d[(reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), col]
    return out
