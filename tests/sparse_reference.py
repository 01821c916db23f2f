"""Host model of the probe's 2:4 structured-sparsity kernels (``ops/csrc/gpu_probe_sparse.h``), in numpy.

Written from the formulas the kernel comments state, not by calling the library: the operand
family and its selector, compression and the metadata packing of the public layout, the FP8 / BF8
codes of the small integers, the 30 × 7 table of expected sums, the measured lane maps of the
``v_smfmac_*`` instructions, and the mismatches a changed value, nibble or B element must produce.
"""

import numpy as np

import probe_reference as ref

FORMATS = ["bf16", "f16", "i8", "fp8", "bf8"]
STAGE = {"bf16": 64, "f16": 64, "i8": 128, "fp8": 128, "bf8": 128}  # dense elements per stage: 128 bytes of a Bt row
ESIZE = {"bf16": 2, "f16": 2, "i8": 1, "fp8": 1, "bf8": 1}
MUL = {"bf16": (1, 1), "f16": (1, 1), "i8": (25, 41), "fp8": (1, 1), "bf8": (1, 1)}
# integers the accumulator holds exactly: fp32's 24 bits, int32's 31
EXACT_BELOW = {"bf16": 2 ** 24, "f16": 2 ** 24, "i8": 2 ** 31, "fp8": 2 ** 24, "bf8": 2 ** 24}
# the largest integer magnitude below which every integer is a value of the format
INT_RANGE = {"bf16": 256, "f16": 2048, "i8": 127, "fp8": 16, "bf8": 8}
CLASSES = (30, 7)

SEL = [(0, 3), (2, 3), (1, 3), (1, 2), (0, 1), (0, 2)]  # the pair group g of row i keeps: SEL[(i + g) % 6]
NIBBLES = [p0 | p1 << 2 for p0, p1 in SEL]
VALID_NIBBLES = sorted(NIBBLES)
assert VALID_NIBBLES == [4, 8, 9, 12, 13, 14]


# ------------------------------------------------------------------ family, selector, table


def nibbles(m, k):
    """The selector: the nibble of group ``g`` of row ``i``, ``[m, k / 4]``."""
    i = np.arange(m, dtype=np.int64)[:, None]
    g = np.arange(k // 4, dtype=np.int64)[None, :]
    return np.array(NIBBLES, dtype=np.int64)[(i + g) % 6]


def keep_mask(m, k):
    nib = np.repeat(nibbles(m, k), 4, axis=1)
    pos = np.arange(k, dtype=np.int64)[None, :] % 4
    return (pos == (nib & 3)) | (pos == (nib >> 2))


def pruned_operands(m, n, k):
    """The small integers: ``A`` of the bf16 probe pruned 2:4 by the selector (dense, zeros where
    pruned) and its ``Bt``, as int64."""
    a, bt = ref.probe_operands(m, n, k)
    return a * keep_mask(m, k), bt


def table(k):
    """Expected sums of the small integers by ``(i mod 30, j mod 7)``, from the definition."""
    a, bt = pruned_operands(30, 7, k)
    return a @ bt.T


def expected(fmt, m, n, k):
    """What the kernel's output must be: the table times the format's multipliers."""
    t = table(k) * (MUL[fmt][0] * MUL[fmt][1])
    return t[np.arange(m)[:, None] % 30, np.arange(n)[None, :] % 7]


def zero_classes(k):
    return int((table(k) == 0).sum())


# ------------------------------------------------------------------ compression and metadata


def pack_meta(nib):
    """``[m, groups]`` nibbles as the ``[m, groups / 2]`` bytes of the public layout."""
    nib = np.asarray(nib, dtype=np.int64)
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)


def unpack_meta(meta):
    meta = np.asarray(meta, dtype=np.uint8).astype(np.int64)
    out = np.empty((meta.shape[0], 2 * meta.shape[1]), dtype=np.int64)
    out[:, 0::2], out[:, 1::2] = meta & 15, meta >> 4
    return out


def compress_with(a, nib):
    """The kept elements of dense ``a`` under the given nibbles: ``[m, k / 2]``."""
    m, k = a.shape
    g = a.reshape(m, k // 4, 4)
    pos = np.stack((nib & 3, nib >> 2), axis=-1)
    return np.take_along_axis(g, pos, axis=-1).reshape(m, k // 2)


def decompress(ac, meta):
    """Dense ``[m, k]`` of compressed ``ac`` and metadata bytes (nibbles with ``p0 < p1``)."""
    nib = unpack_meta(meta)
    m, g = nib.shape
    out = np.zeros((m, g, 4), dtype=ac.dtype)
    pos = np.stack((nib & 3, nib >> 2), axis=-1)
    np.put_along_axis(out, pos, ac.reshape(m, g, 2), axis=-1)
    return out.reshape(m, 4 * g)


def compress(a, prune=False):
    """``sparse_compress`` of ``ops/gpu.py`` again: the two largest magnitudes of each group (non-zeros
    before zeros without ``prune``), ties to the lower position, kept in ascending position."""
    m, k = a.shape
    g = a.reshape(m, k // 4, 4)
    key = np.abs(g.astype(np.float64)) if prune else (g != 0).astype(np.int64)
    if not prune and (key.sum(-1) > 2).any():
        r, gg = np.argwhere(key.sum(-1) > 2)[0]
        raise ValueError(f"row {r}, group {gg}")
    order = np.argsort(-key, axis=-1, kind="stable")[..., :2]
    pos = np.sort(order, axis=-1)
    nib = pos[..., 0] | (pos[..., 1] << 2)
    return np.take_along_axis(g, pos, axis=-1).reshape(m, k // 2), pack_meta(nib)


def fill(fmt, m, n, k):
    """What ``sparse_fill_kernel`` writes, as integers: compressed A, metadata bytes, Bt (``i8``:
    times its multipliers)."""
    a, bt = ref.probe_operands(m, n, k)
    nib = nibbles(m, k)
    return compress_with(a, nib) * MUL[fmt][0], pack_meta(nib), bt * MUL[fmt][1]


# ------------------------------------------------------------------ encodings


def fp8_code(v):
    """OCP e4m3fn codes of integers in -3 … 3."""
    v = np.asarray(v, dtype=np.int64)
    return (np.array([0, 0x38, 0x40, 0x44], dtype=np.uint8)[np.abs(v)] | np.where(v < 0, 0x80, 0)).astype(np.uint8)


def bf8_code(v):
    """OCP e5m2 codes of integers in -3 … 3."""
    v = np.asarray(v, dtype=np.int64)
    return (np.array([0, 0x3C, 0x40, 0x42], dtype=np.uint8)[np.abs(v)] | np.where(v < 0, 0x80, 0)).astype(np.uint8)


def fp8_value(code):
    """The value of an e4m3fn code (no NaN codes expected: ``code_values`` has them)."""
    c = np.asarray(code, dtype=np.int64)
    e, mant = (c >> 3) & 15, c & 7
    mag = np.where(e == 0, mant / 8.0 * 2.0 ** -6, (1 + mant / 8.0) * 2.0 ** (e - 7))
    return np.where(c & 0x80, -mag, mag)


def bf8_value(code):
    """The value of an e5m2 code (no inf / NaN codes expected: ``code_values`` has them)."""
    c = np.asarray(code, dtype=np.int64)
    e, mant = (c >> 2) & 31, c & 3
    mag = np.where(e == 0, mant / 4.0 * 2.0 ** -14, (1 + mant / 4.0) * 2.0 ** (e - 15))
    return np.where(c & 0x80, -mag, mag)


def code_values(fmt):
    """All 256 codes of ``fp8`` (OCP e4m3fn: S.1111.111 is NaN, no infinity, largest ±448) or ``bf8`` (OCP
    e5m2: exponent 31 is ±inf with mantissa 0 and NaN otherwise, largest ±57344) as float64."""
    c = np.arange(256, dtype=np.int64)
    if fmt == "fp8":
        v = fp8_value(c)
        v[(c & 0x7F) == 0x7F] = np.nan
        return v
    assert fmt == "bf8"
    v = bf8_value(c)
    top = (c >> 2) & 31 == 31
    v[top & (c & 3 != 0)] = np.nan
    v[top & (c & 3 == 0)] = np.where(c[top & (c & 3 == 0)] & 0x80, -np.inf, np.inf)
    return v


# the elements as they are stored: bf16 as the int16 of its bits (numpy has no bfloat16), fp8 / bf8 as codes
NP_STORED = {"bf16": np.int16, "f16": np.float16, "i8": np.int8, "fp8": np.uint8, "bf8": np.uint8}


def encode(fmt, ints):
    """Small integers (the probe's: ``|v| <= 3``; bf16, f16 and i8: any the format holds) as stored elements."""
    v = np.asarray(ints, dtype=np.int64)
    if fmt == "bf16":
        bits = v.astype(np.float32).view(np.uint32)
        assert not (bits & 0xFFFF).any()  # 8 significant bits
        return (bits >> 16).astype(np.uint16).view(np.int16)
    if fmt in ("fp8", "bf8"):
        return (fp8_code if fmt == "fp8" else bf8_code)(v)
    out = v.astype(NP_STORED[fmt])
    assert np.array_equal(out.astype(np.int64), v)
    return out


def decode(fmt, stored):
    """Stored elements as float64, every bit pattern: subnormals, infinities and NaN included."""
    x = np.asarray(stored)
    assert x.dtype == NP_STORED[fmt], (fmt, x.dtype)
    if fmt == "bf16":
        return (x.view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    if fmt in ("fp8", "bf8"):
        return code_values(fmt)[x]
    return x.astype(np.float64)


# ------------------------------------------------------------------ the product and its mismatches


def product(ac, meta, bt):
    """``A · Btᵀ`` of integer operands in the public layout, exact int64."""
    return decompress(np.asarray(ac, dtype=np.int64), meta) @ np.asarray(bt, dtype=np.int64).T


def product_per_slot(ac, nib, bt):
    """The same product as the instruction forms it, each kept slot steered by its own 2-bit selector
    (measured: independently of its partner), so also for nibbles with ``p0 >= p1``: what a faulty
    decoder of the index would compute."""
    ac, bt, nib = np.asarray(ac, dtype=np.int64), np.asarray(bt, dtype=np.int64), np.asarray(nib, dtype=np.int64)
    m, g = nib.shape
    sel = np.stack((nib & 3, nib >> 2), axis=-1).reshape(m, 2 * g)
    kd = 4 * (np.arange(2 * g) // 2)[None, :] + sel
    return np.stack([(ac * bt[j][kd]).sum(axis=1) for j in range(bt.shape[0])], axis=1)


def product_per_slot_f64(ac, nib, bt):
    """``product_per_slot`` in float64, for operands with an infinity or a NaN.  Only the kept slots
    multiply: a row meets ``Bt[j][k]`` only if it keeps dense position k, and then also with a kept
    zero, and ``0 · inf`` and ``0 · NaN`` are NaN.  (``decompress(...) @ bt.T`` would multiply the pruned
    positions too and turn every row of the column into NaN.)"""
    ac, bt, nib = np.asarray(ac, dtype=np.float64), np.asarray(bt, dtype=np.float64), np.asarray(nib, dtype=np.int64)
    m, g = nib.shape
    sel = np.stack((nib & 3, nib >> 2), axis=-1).reshape(m, 2 * g)
    kd = 4 * (np.arange(2 * g) // 2)[None, :] + sel
    with np.errstate(invalid="ignore"):
        return np.stack([(ac * bt[j][kd]).sum(axis=1) for j in range(bt.shape[0])], axis=1)


def mismatches(fmt, ac, meta, bt, k):
    """Where the fused check must count: the product of the given (corrupted) operands against the table."""
    m, n = ac.shape[0], bt.shape[0]
    return product(ac, meta, bt) != expected(fmt, m, n, k)


def per_tile(wrong):
    """Mismatch counts by 256² output tile, ``[tiles_m, tiles_n]``."""
    m, n = wrong.shape
    return wrong.reshape(m // 256, 256, n // 256, 256).sum(axis=(1, 3))


# ------------------------------------------------------------------ measured lane maps
#
# One instruction, one wave, on an MI355X: lane l holds row l & 31 of A and column l & 31 of B,
# h = l >> 5.  In bytes the map is the same for all five instructions (an instruction covers 32
# bytes of a compressed A row and 64 bytes of a Bt row): lane half h holds bytes [16h, 16h + 16) of
# the A piece, and of the Bt piece the 16-byte chunks h (low half of the register) and h + 2 (high
# half).  Kept slot s of a lane is steered by bits [2s, 2s + 2) of the lane's own index register;
# the 16-bit formats use 16 bits of it (CBSZ = 0: ABID bit 0 picks the half; CBSZ = 1: the low
# half), the 8-bit formats all 32.


def lane_a_slot(fmt, lane, slot):
    """Kept element (of the instruction's 16 or 32) in kept slot ``slot`` of ``lane``."""
    per_lane = 16 // ESIZE[fmt]
    return (lane >> 5) * per_lane + slot


def lane_b_element(fmt, lane, e):
    """Dense k (of the instruction's 32 or 64) of element ``e`` of ``lane``'s B register."""
    per_chunk = 16 // ESIZE[fmt]
    chunk = (lane >> 5) + 2 * (e // per_chunk)
    return chunk * per_chunk + e % per_chunk


def lane_index_bits(fmt, lane, slot, cbsz=0, abid=0):
    """Bit position, in the lane's index register, of the 2-bit selector of kept slot ``slot``."""
    if ESIZE[fmt] == 2:
        return 2 * slot + (16 if cbsz == 0 and abid & 1 else 0)
    return 2 * slot


def instruction(fmt, a_regs, b_regs, idx):
    """One ``v_smfmac`` on integer register contents: ``a_regs`` ``[64, slots]``, ``b_regs`` ``[64, elems]``,
    ``idx`` ``[64]``; returns the 32 × 32 product (rows from A's lanes, columns from B's)."""
    slots, elems = a_regs.shape[1], b_regs.shape[1]
    kk = 2 * elems
    bd = np.zeros((32, kk), dtype=np.int64)  # B as [col][dense k]
    for lane in range(64):
        for e in range(elems):
            bd[lane & 31, lane_b_element(fmt, lane, e)] = b_regs[lane, e]
    out = np.zeros((32, 32), dtype=np.int64)
    for lane in range(64):
        for s in range(slots):
            sel = (int(idx[lane]) >> lane_index_bits(fmt, lane, s)) & 3
            kd = 4 * (lane_a_slot(fmt, lane, s) // 2) + sel
            out[lane & 31] += int(a_regs[lane, s]) * bd[:, kd]
    return out


def lanemap_case(fmt):
    """256 × 256 × one stage: row ``i`` has a single non-zero kept element, 1, in kept slot
    ``i mod (stage / 2)``, at position ``(i // (stage / 2)) mod 4`` of its group where that is valid for
    the slot (an even slot is p0 and cannot be 3, an odd one is p1 and cannot be 0: then 1 resp. 2);
    its partner in the group is p1 = 3 resp. p0 = 0, every other group has the pair (0,1).
    ``Bt[j][k]`` is value number ``(k + j) mod stage`` of ``stage`` distinct values of the format, so
    for every column it identifies k.  Returns ``ac`` (integers), ``meta`` (bytes), ``bt`` (integers, or
    uint8 codes for fp8 / bf8) and ``want`` (float64): ``C[i][j]`` is the one value ``Bt[j][k_i]``."""
    stage = STAGE[fmt]
    half = stage // 2
    i = np.arange(256)
    slot = i % half
    want_pos = (i // half) % 4
    odd = slot % 2 == 1
    pos = np.where(odd, np.where(want_pos == 0, 2, want_pos), np.where(want_pos == 3, 1, want_pos))
    ac = np.zeros((256, half), dtype=np.int64)
    ac[i, slot] = 1
    nib = np.full((256, stage // 4), 4, dtype=np.int64)  # (0,1)
    p0 = np.where(odd, 0, pos)
    p1 = np.where(odd, pos, 3)
    assert (p0 < p1).all()
    nib[i, slot // 2] = p0 | (p1 << 2)
    kd = 4 * (slot // 2) + pos  # the dense k the hot element stands at
    number = (np.arange(stage)[None, :] + np.arange(256)[:, None]) % stage
    if fmt in ("fp8", "bf8"):
        bt = np.where(number < 64, 8 + number, 0x88 + number - 64).astype(np.uint8)  # normal, finite, distinct
        values = (fp8_value if fmt == "fp8" else bf8_value)(bt)
    else:
        bt = (number + 1 + 128) % 256 - 128 if fmt == "i8" else number + 1  # i8: 1 … 127, -128
        values = bt.astype(np.float64)
    assert all(len(set(row.tolist())) == stage for row in values[:3])
    want = values[:, kd].T.copy()  # C[i][j] = Bt[j][kd_i]
    return ac, pack_meta(nib), bt, want


# ------------------------------------------------------------------ sweeps of the fused check


def other_value(v, mul=1):
    """Another small value of both families than ``v`` (multiples of ``mul``): 1, or 2 where it is 1."""
    v = np.asarray(v, dtype=np.int64)
    return np.where(v != mul, mul, 2 * mul)


def sweep_values(fmt, v, side):
    """The integers of the compressed A (``side`` 0) or of Bt (1) with element ``x mod width`` of every row x
    replaced by another value of the family, times the format's multiplier."""
    out = np.array(v, dtype=np.int64)
    idx = np.arange(out.shape[0])
    hot = idx % out.shape[1]
    out[idx, hot] = other_value(out[idx, hot], MUL[fmt][side])
    return out


def kept_slot_coordinates(fmt, slot):
    """Where kept slot ``slot`` of a compressed row lives in the kernel: ``(stage, instruction of the
    stage, lane half, group of the lane's eight or sixteen bytes, slot of the group)``.  A stage is 64
    bytes of a compressed row, an instruction 32 of them, a lane half 16."""
    byte = np.asarray(slot, dtype=np.int64) * ESIZE[fmt]
    per_half = 16 // ESIZE[fmt]  # kept elements of a lane
    return byte // 64, byte % 64 // 32, byte % 32 // 16, np.asarray(slot) % per_half // 2, np.asarray(slot) % 2


def nibble_sweep_plan(m, n, k):
    """One metadata nibble per row for a sweep of the fused check: ``(group [m], replacement [m], moved)``.

    The candidates of row i are the pairs (group, replacement) in cyclic order, six valid nibbles per
    group, from group ``i mod (K/4)`` and replacement number ``(i + i // (K/4) + 2) mod 6`` on (an offset at
    which few rows start on the nibble they already have); the plan takes
    the first under which row i of the product leaves the table in at least one column.  (The
    nibble the row has there changes nothing, and neither does moving the selector of a kept zero
    or between two positions at which ``Bt`` agrees in every column.)  ``moved`` counts the rows that did
    not take their first candidate.  The multipliers of i8 are not zero and change no mismatch, so
    the plan serves every format."""
    a, bt = ref.probe_operands(m, n, k)
    nib = nibbles(m, k)
    ac = compress_with(a, nib)
    groups = k // 4
    group, new, moved = np.empty(m, dtype=np.int64), np.empty(m, dtype=np.int64), 0
    for i in range(m):
        first = (i % groups) * 6 + (i + i // groups + 2) % 6
        for t in range(6 * groups):
            q = (first + t) % (6 * groups)
            g, cand = q // 6, VALID_NIBBLES[q % 6]
            old = int(nib[i, g])
            delta = np.zeros(n, dtype=np.int64)
            for s, (was, now) in enumerate(((old & 3, cand & 3), (old >> 2, cand >> 2))):
                delta += ac[i, 2 * g + s] * (bt[:, 4 * g + now] - bt[:, 4 * g + was])
            if delta.any():
                break
        else:
            raise AssertionError(f"row {i}: no nibble changes the product")
        group[i], new[i] = g, cand
        moved += t > 0
    return group, new, moved


def meta_with_nibbles(meta, group, new):
    """The metadata bytes with nibble ``group[i]`` of row i replaced by ``new[i]``."""
    nib = unpack_meta(meta)
    nib[np.arange(nib.shape[0]), group] = new
    return pack_meta(nib)


# ------------------------------------------------------------------ store kernel: value against value


def bf16_value_sets():
    """Two sets of 256 bf16 bit patterns (uint16) whose every product big · small is a normal fp32 or a
    zero, and exact (8 + 8 significant bits): no set holding both the largest finite value and the
    smallest normal can do that with itself, so they stand on opposite sides, and the case is
    run both ways round.
    ``big``: the integers -8 .. 8, ± the largest finite value, ±0, the all-ones mantissa of every exponent
    2^0 .. 2^126, and seeded normals of magnitude in [1, 2^128).
    ``small``: the smallest normal, ±0, the all-ones mantissa of every exponent 2^-126 .. 2^-2, and seeded
    normals of magnitude in [2^-126, 2^-1)."""
    rng = np.random.default_rng(161616)

    def normals(count, lo, hi):  # biased exponents lo .. hi
        e = rng.integers(lo, hi + 1, size=count)
        return (rng.integers(0, 2, size=count) << 15) | (e << 7) | rng.integers(0, 128, size=count)

    ints = (np.arange(-8, 9).astype(np.float32).view(np.uint32) >> 16).tolist()
    big = ints + [0x7F7F, 0xFF7F, 0x0000, 0x8000] + [(e << 7) | 0x7F for e in range(127, 254)]
    big += normals(256 - len(big), 127, 254).tolist()
    small = [0x0080, 0x0000, 0x8000] + [(e << 7) | 0x7F for e in range(1, 126)]
    small += normals(256 - len(small), 1, 125).tolist()
    return np.array(big, dtype=np.uint16), np.array(small, dtype=np.uint16)


def store_values(fmt, swap=False):
    """The 256 stored elements of the rows and of the columns of ``onehot_case``: every code of fp8 and
    bf8 and every value of i8 on both sides, the halves of ``probe_reference.f16_values`` on both, and
    for bf16 the two sets of ``bf16_value_sets`` (``swap``: the small one on the rows)."""
    if fmt in ("fp8", "bf8"):
        v = np.arange(256, dtype=np.uint8)
        return v, v
    if fmt == "i8":
        v = np.arange(256, dtype=np.uint8).view(np.int8)
        return v, v
    if fmt == "f16":
        v = ref.f16_values().view(np.float16)
        return v, v
    big, small = (x.view(np.int16) for x in bf16_value_sets())
    return (small, big) if swap else (big, small)


def onehot_case(fmt, swap=False):
    """256 × 256 at one stage, every output one product: compressed row i holds row value i in kept slot
    ``i mod (stage / 2)`` and +0 elsewhere (over the rows: every slot of the stage), the metadata is
    seeded random valid nibbles, and ``Bt[j]`` is column value j at every k, so whatever the nibbles
    select the expectation is the same.  Returns ``ac, meta, bt`` as stored and ``want`` in float64,
    the IEEE product ``row value i · column value j``: NaN for a NaN and for ``inf · 0``, the same-signed
    infinity for ``inf · x``.  The row's other kept slots are zeros and are multiplied too, so an
    infinite or NaN column value makes its whole column NaN (``0 · inf``), while a NaN or infinite
    row value meets only its own slot."""
    stage = STAGE[fmt]
    half = stage // 2
    rows, cols = store_values(fmt, swap)
    i = np.arange(256)
    ac = np.zeros((256, half), dtype=NP_STORED[fmt])  # all bits 0 is +0 in every format
    ac[i, i % half] = rows
    rng = np.random.default_rng(2400024 + FORMATS.index(fmt))
    meta = pack_meta(rng.choice(VALID_NIBBLES, size=(256, stage // 4)))
    bt = np.repeat(cols[:, None], stage, axis=1)
    va, vb = decode(fmt, rows), decode(fmt, cols)
    with np.errstate(invalid="ignore"):
        want = va[:, None] * vb[None, :]
    want = np.where(np.isfinite(vb)[None, :], want, np.nan)
    return ac, meta, bt, want
