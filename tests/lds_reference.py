"""Host model of the probe's LDS step (``ops/csrc/gpu_probe_lds.h``), in numpy only.

* the key table and the folds of a key to an element's width;
* the ``mem`` pattern of every pass and who reads what;
* the lane maps of the four transposing LDS reads as measured on an MI355X
  (``profiles/lds_probe/SUMMARY.txt``): :func:`tr_read` is one instruction on an image;
* the images, pitches and bases of the fused transposing-read checks;
* the selector -> source function of every lane exchange;
* pack, unpack and transpose of every format of the transposer, on the packing of ``mx_reference.py``;
* the banks the transposer's LDS accesses touch, by the bank rule;
* case counts, and the mismatches a wrong table byte gives.
"""

import numpy as np

import mx_reference as mx

MEM, TR16, TR8, TR4, TR6, XLANE = range(6)
NAMES = {"mem": MEM, "tr16": TR16, "tr8": TR8, "tr4": TR4, "tr6": TR6, "xlane": XLANE}
BLOCKS, TABLE, WAVES = 256, 1024, 4
M32 = 0xFFFFFFFF


def mix(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def key(check, i):
    return mix(0x9E3779B9 * (np.asarray(i, dtype=np.uint64) + 1) + 0x85EBCA6B * (check + 1))


def table(check):
    """The ``TABLE`` bytes ``odh_lds_fill`` writes."""
    return key(check, np.arange(256)).astype("<u4").view(np.uint8)


def fold(k, bits):
    k = np.asarray(k, dtype=np.uint64)
    if bits >= 32:
        return k
    k = k ^ (k >> 16)
    if bits == 16:
        return k & 0xFFFF
    k = k ^ (k >> 8)
    if bits == 8:
        return k & 0xFF
    return (k ^ (k >> 4)) & 0xF  # 4- and 6-bit elements: the XOR of the eight nibbles


# ------------------------------------------------------------------ mem

MEM_DWORDS, MEM_PASSES = 160 * 1024 // 4, 4


def mem_kidx(w, p):
    return (np.asarray(w) + 37 * (p & ~1)) & 255


def mem_values(p, keys=None):
    """What pass ``p`` stores in every dword (``keys``: the 256 key dwords; default: the table's)."""
    w = np.arange(MEM_DWORDS, dtype=np.uint64)
    keys = key(MEM, np.arange(256)) if keys is None else np.asarray(keys, dtype=np.uint64)
    v = mix(w * 0x9E3779B1 + (p & ~1) * 0x632BE5AB + 1) ^ keys[mem_kidx(w, p)]
    return (~v & M32) if p & 1 else v


def mem_writer_wave(w):
    """Both kinds of pass: of the 1024 dwords of an ``i``, wave v writes ``[256 v, 256 v + 256)``."""
    return (np.asarray(w) >> 8) & 3


def mem_reader_wave(w):
    w = np.asarray(w)
    src, i = (w >> 8) & 3, w >> 10
    return (src - 1 - i % 3) & 3  # the wave v with (v + 1 + i mod 3) mod 4 == src


# ------------------------------------------------------------------ the transposing reads

# bits of an element, rows of a block, alignment of an address, bytes a block row occupies, result bytes
TR = {TR16: (16, 4, 8, 32, 8), TR8: (8, 8, 8, 16, 8), TR4: (4, 16, 8, 8, 8), TR6: (6, 16, 16, 16, 12)}


def tr_lane_offset(check, i, pitch):
    """Byte offset, from a block's first byte, of the address lane ``i`` (0 .. 15) of a group supplies: a block
    row is 16 elements, and ``16 / rows`` lanes supply 8 bytes of it each (tr4, tr6: one lane, all of it)."""
    lpr = 16 // TR[check][1]
    return (i // lpr) * pitch + (i % lpr) * 8


def tr_read(check, image, addr):
    """One instruction: ``image`` uint8, ``addr`` the 64 lanes' byte addresses.  Lane ``i`` of a group of 16
    receives column ``i`` of the group's block, row ``q`` in bits ``[bits q, bits q + bits)`` of its result; row
    ``q``, piece ``p`` of the block is read at the address of lane ``(16 / rows) q + p`` of the group.  An
    address that is not aligned reads from the aligned address below it.  Returns uint8 ``[64, result bytes]``."""
    bits, rows, align, _, width = TR[check]
    lpr = 16 // rows
    per_piece = 16 // lpr  # elements of a row one lane's address supplies
    img = np.unpackbits(np.asarray(image, dtype=np.uint8), bitorder="little")
    out = np.zeros((64, width * 8), dtype=np.uint8)
    addr = [int(a) // align * align for a in addr]
    for lane in range(64):
        g, i = lane // 16, lane % 16
        for q in range(rows):
            src = addr[16 * g + lpr * q + i // per_piece] * 8 + (i % per_piece) * bits
            out[lane, bits * q:bits * q + bits] = img[src:src + bits]
    return np.packbits(out, axis=1, bitorder="little")


TR_COLS = 64


def tr_geometry(check):
    bits, rows, align, slot, _ = TR[check]
    positions = 256 // align
    return dict(bits=bits, rows=4 * rows, block_rows=rows, align=align, slot=slot, row_bytes=TR_COLS // 16 * slot,
                positions=positions, rounds=3 * positions)


def tr_pitch(check, rnd):
    g = tr_geometry(check)
    return (g["row_bytes"], g["row_bytes"] + g["align"], 2 * g["row_bytes"])[rnd // g["positions"]]


def tr_base(check, rnd):
    g = tr_geometry(check)
    return rnd % g["positions"] * g["align"]


def tr_kidx(r, c, rnd):
    return (64 * np.asarray(r) + np.asarray(c) + 17 * rnd) & 255


def tr_values(check, rnd, keys=None):
    """``[rows, 64]`` elements of the image of round ``rnd``."""
    g = tr_geometry(check)
    r, c = np.meshgrid(np.arange(g["rows"]), np.arange(TR_COLS), indexing="ij")
    keys = key(check, np.arange(256)) if keys is None else np.asarray(keys, dtype=np.uint64)
    h = mix(((rnd * 64 + r) * 64 + c).astype(np.uint64) * 0x9E3779B1 + check)
    return ((h >> 7) ^ fold(keys[tr_kidx(r, c, rnd)], g["bits"])) & ((1 << g["bits"]) - 1)


def tr_image(check, rnd, keys=None):
    """The bytes a wave's region holds in round ``rnd`` (from the region's first byte), and ``(base, pitch)``."""
    g = tr_geometry(check)
    v = tr_values(check, rnd, keys)
    base, pitch = tr_base(check, rnd), tr_pitch(check, rnd)
    img = np.zeros(base + g["rows"] * pitch + 16, dtype=np.uint8)
    for r in range(g["rows"]):
        for cb in range(TR_COLS // 16):
            e = v[r, 16 * cb:16 * cb + 16]
            b = np.zeros(16 * g["bits"], dtype=np.uint8)
            for k in range(16):
                b[g["bits"] * k:g["bits"] * (k + 1)] = (int(e[k]) >> np.arange(g["bits"])) & 1
            at = base + r * pitch + cb * g["slot"]
            img[at:at + 2 * g["bits"]] = np.packbits(b, bitorder="little")
    return img, base, pitch


def tr_block_of(group, read):
    """The block (row block, column block) group ``group`` reads in read ``read`` (0 .. 15) of a round."""
    b = (read + 5 * group) & 15
    return b >> 2, b & 3


def tr_unpack(check, out):
    """``[64, result bytes]`` -> ``[64, rows of a block]`` elements."""
    bits, rows = TR[check][:2]
    b = np.unpackbits(np.asarray(out, dtype=np.uint8), axis=1, bitorder="little")[:, :bits * rows]
    return (b.reshape(64, rows, bits).astype(np.int64) << np.arange(bits)).sum(axis=2)


# ------------------------------------------------------------------ lane exchange

OPS = {"bpermute": 0, "permute": 1, "swizzle": 2, "dpp": 3, "readlane": 4, "writelane": 5, "permlane16_swap": 6,
       "permlane32_swap": 7}
# swap 1, 2, 4, 8, 16; reverse 32, 4, 8; broadcast lane 0, 31, 3 of every 8; quad_perm [3,2,1,0]
SWIZZLE = [0x041F, 0x081F, 0x101F, 0x201F, 0x401F, 0x7C1F, 0x0C1F, 0x1C1F, 0x0000, 0x03E0, 0x0078, 0x801B]
# quad_perm six times, row_shl / row_shr / row_ror 1 .. 15, row_mirror, row_half_mirror, row_bcast:15, row_bcast:31
DPP = [0x1B, 0xB1, 0x4E, 0x00, 0xFF, 0x39] + [0x100 + n for n in range(1, 16)] + [0x110 + n for n in range(1, 16)] \
    + [0x120 + n for n in range(1, 16)] + [0x140, 0x141, 0x142, 0x143]
ARGS = {"bpermute": 65, "permute": 65, "swizzle": len(SWIZZLE), "dpp": len(DPP), "readlane": 64, "writelane": 64,
        "permlane16_swap": 4, "permlane32_swap": 4}
XL_REPEAT = 16


def bitrev6(l):
    return int(format(l, "06b")[::-1], 2)


def swizzle_src(pattern, l):
    if pattern & 0x8000:
        return (l & ~3) | (pattern >> (2 * (l & 3)) & 3)
    a, o, x = pattern & 31, pattern >> 5 & 31, pattern >> 10 & 31
    return (l & 32) | ((((l & 31) & a) | o) ^ x)


def dpp_src(ctrl, l):
    """bound_ctrl off, old = the lane's own value: a lane without a source keeps its own."""
    row, i, n = l & ~15, l & 15, ctrl & 15
    if ctrl < 0x100:
        return (l & ~3) | (ctrl >> (2 * (l & 3)) & 3)
    if ctrl < 0x110:
        return l + n if i + n < 16 else l
    if ctrl < 0x120:
        return l - n if i >= n else l
    if ctrl < 0x130:
        return row | ((i - n) & 15)
    if ctrl == 0x140:
        return row | (15 - i)
    if ctrl == 0x141:
        return (l & ~7) | (7 - (l & 7))
    if ctrl == 0x142:
        return row - 1 if l >= 16 else l
    return 31 if l >= 32 else l


def xl_src(op, arg, t):
    """The value index (0 .. 63; the swaps: 0 .. 127, 64 + l lane l's second register) that result index ``t``
    holds after the exchange."""
    op = OPS.get(op, op)
    l = t & 63
    if op == 0:
        return (l + arg) & 63 if arg < 64 else bitrev6(l)
    if op == 1:
        return (l - arg) & 63 if arg < 64 else bitrev6(l)
    if op == 2:
        return swizzle_src(SWIZZLE[arg], l)
    if op == 3:
        return dpp_src(DPP[arg], l)
    if op == 4:
        return arg
    if op == 5:
        return (arg + 1) & 63 if l == arg else l
    half = 16 if op == 6 else 32  # the first register's odd rows (upper half) change places with the second's even
    if t < 64:
        return 64 + l - half if l & half else l
    return 64 + l if l & half else l + half


def xl_sources(op, arg):
    n = 128 if OPS.get(op, op) >= 6 else 64
    return np.array([xl_src(op, arg, t) for t in range(n)])


def xl_exchanges():
    """(op, arg) of every exchange of one repeat of the fused check, in its order."""
    return [(op, arg) for op in range(8) for arg in range(list(ARGS.values())[op])]


# ------------------------------------------------------------------ counts


def _tr_hist(check):
    g = tr_geometry(check)
    h = np.zeros(256, dtype=np.int64)
    r, c = np.meshgrid(np.arange(g["rows"]), np.arange(TR_COLS), indexing="ij")
    for rnd in range(g["rounds"]):
        h += np.bincount(tr_kidx(r, c, rnd).ravel(), minlength=256)
    return h * 4 * WAVES  # each of the four groups of lanes of each wave is delivered every element once a round


def _xl_hist():
    h = np.zeros(256, dtype=np.int64)
    ex = xl_exchanges()
    srcs = [xl_sources(op, arg) for op, arg in ex]
    e = 0
    for _ in range(XL_REPEAT):
        for s in srcs:
            h += np.bincount((s + 67 * e) & 255, minlength=256)
            e += 1
    return h * WAVES


_HIST = {}


def key_histogram(check):
    """Compared elements of one workgroup by the key dword they use."""
    if check not in _HIST:
        if check == MEM:
            w = np.arange(MEM_DWORDS)
            _HIST[check] = sum(np.bincount(mem_kidx(w, p), minlength=256) for p in range(MEM_PASSES))
        elif check == XLANE:
            _HIST[check] = _xl_hist()
        else:
            _HIST[check] = _tr_hist(check)
    return _HIST[check]


def cases(check):
    return int(key_histogram(check).sum()) * BLOCKS


def fault_count(check, table_byte):
    return int(key_histogram(check)[table_byte // 4]) * BLOCKS


def fold_changes(check, delta):
    """Whether a table byte XOR ``delta`` changes the element a key folds to: always in the 32-, 16- and 8-bit
    checks, in ``tr4`` and ``tr6`` unless both nibbles of the byte change alike."""
    return delta != 0 and (check not in (TR4, TR6) or (delta ^ (delta >> 4)) & 15 != 0)


# ------------------------------------------------------------------ the transposer

FORMAT_BITS = {"bf16": 16, "f16": 16, "fp8": 8, "bf8": 8, "fp4": 4, "fp6": 6, "bf6": 6}


def unpack_codes(fmt, x):
    """``[R, row bytes]`` uint8 (16 bit: ``[R, C]`` uint16) -> ``[R, C]`` element codes."""
    bits = FORMAT_BITS[fmt]
    if bits == 16:
        return np.asarray(x).view(np.uint16).astype(np.int64)
    return np.asarray(mx.unpack({8: mx.FP8, 4: mx.FP4, 6: mx.FP6}[bits], x)).astype(np.int64)


def pack_codes(fmt, codes):
    bits = FORMAT_BITS[fmt]
    if bits == 16:
        return np.asarray(codes).astype(np.uint16)
    return mx.pack({8: mx.FP8, 4: mx.FP4, 6: mx.FP6}[bits], codes)


def transpose_codes(fmt, x):
    return pack_codes(fmt, np.ascontiguousarray(unpack_codes(fmt, x).T))


# format bits -> (transposing read, pitch of the LDS image, bytes of a tile row in the image)
TC = {16: (TR16, 288, 256), 8: (TR8, 144, 128), 4: (TR4, 80, 64), 6: (TR6, 144, 128)}


def tc_read_addresses(bits):
    """Per wave, step and read of the transposer: the 64 lanes' byte addresses into the LDS image."""
    check, pitch, _ = TC[bits]
    rows = TR[check][1]
    blocks = 128 // rows
    steps = 1 if bits == 6 else blocks // 4
    out = []
    for wave in range(4):
        for s in range(steps):
            step = wave * steps + s
            for n in range(4 if bits == 6 else 2):
                addr = []
                for lane in range(64):
                    g, i = lane // 16, lane % 16
                    h, sub = g >> 1, g & 1
                    if bits in (16, 8):
                        cb, first, down = 2 * (step & 3) + h, 4 * (step >> 2) + 2 * sub, sub
                    elif bits == 4:
                        cb, first, down = 2 * (step & 3) + sub, 4 * (step >> 2) + 2 * h, 0
                    else:
                        cb, first, down = 2 * step + h, 4 * sub, 0
                    rb = first + ((1 - n) if down else n)
                    col = 16 * cb if bits == 6 else cb * 2 * bits
                    addr.append(rb * rows * pitch + col + tr_lane_offset(check, i, pitch))
                out.append((wave, s, n, addr))
    return out


# lanes whose accesses share LDS cycles: halves of 32 for the 8-byte transposing reads; ds_read_b96's sets of 8
# (assumed for ds_read_b96_tr_b6)
HALVES = [list(range(32)), list(range(32, 64))]
B96_SETS = [[0, 1, 2, 3, 20, 21, 22, 23], [4, 5, 6, 7, 16, 17, 18, 19], [8, 9, 10, 11, 28, 29, 30, 31],
            [12, 13, 14, 15, 24, 25, 26, 27]]
B96_SETS = B96_SETS + [[l + 32 for l in s] for s in B96_SETS]


def bank_conflicts(addr, nbytes, groups, modulus):
    """Extra LDS cycles of one wave-instruction by the bank rule: per group of lanes, the most distinct
    addresses on one bank, minus one (equal addresses broadcast)."""
    extra = 0
    for grp in groups:
        banks = {}
        for lane in grp:
            for d in range(nbytes // 4):
                banks.setdefault((addr[lane] // 4 + d) % modulus, set()).add(addr[lane] // 4 + d)
        extra += max(len(v) for v in banks.values()) - 1
    return extra


def tc_read_conflicts(bits):
    if bits == 6:
        return sum(bank_conflicts(a, 12, B96_SETS, 32) for *_, a in tc_read_addresses(bits))
    return sum(bank_conflicts(a, 8, HALVES, 64) for *_, a in tc_read_addresses(bits))


def tc_write_conflicts(bits):
    """The staging stores: 16 bytes (6 bit: 12) per lane, 8 consecutive lanes share cycles, banks mod 32."""
    _, pitch, row = TC[bits]
    sets = [list(range(8 * k, 8 * k + 8)) for k in range(8)]
    extra = 0
    if bits == 6:
        for wave in range(4):
            for j in range(4):
                addr = [((64 * wave + l) >> 1) * pitch + 64 * (l & 1) + 16 * j for l in range(64)]
                extra += bank_conflicts(addr, 12, sets, 32)
        return extra
    ch = row // 16
    for u in range(128 * ch // 256):
        for wave in range(4):
            addr = []
            for l in range(64):
                k = 64 * wave + l + 256 * u
                r = k // ch
                if bits == 4:
                    r = (r & ~7) | (r & 1) << 2 | (r >> 1 & 3)
                addr.append(r * pitch + 16 * (k % ch))
            extra += bank_conflicts(addr, 16, sets, 32)
    return extra
