"""Sweeps of the 2:4 structured-sparsity and FP32 / FP64 probe kernels on a real MI355X:
``sparse_gemm256_kernel`` (``gpu_probe_sparse.h``, five formats) and ``fp_gemm_kernel`` (``gpu_probe_fp.h``),
held to the standard of ``test_gpu_lowprec_sweeps.py`` with the machinery of ``probe_gpu.py``.

* The fused checks: one compressed value per row, one B element per column, one metadata nibble per
  row (sparse), one element of A per row and of Bt per column (fp) is changed, launch by launch, at
  2 × 2 tiles of 256 rows (2 × 4 tiles for f64, whose tiles are 128 columns wide).  Every launch must
  count exactly the mismatches of the host model and attribute them to the XCDs its own
  ``tile_xcd`` map names.
* NaN and infinity, in A / Ac and in the sparse Bt, are counted where the model has them.
* The sparse store kernels: every fp8 code against every fp8 code, every bf8 code against every
  bf8 code, every i8 value against every i8 value, 256 halves and 2 × 256 bf16 values against each
  other, as one-hot products that are exact whatever the order of summation.

Everything is bit-exact.  The tests corrupt data only; every pointer handed to a kernel comes
from a torch allocation of exactly the size the shape implies (a launch's counter row and tile
map are rows of such an allocation).
"""

import functools
import itertools

import numpy as np
import pytest

import fp_reference as fp
import sparse_reference as sp
from probe_gpu import _assert_operands_are_the_models, _assert_store_exact, _gpu, _probe, _sweep
from probe_gpu import _own_timeout, dev  # noqa: F401  (fixtures)

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SPARSE = sp.FORMATS
# 2 × 2 tiles.  K = 640 is the smallest K of whole 8-bit stages at which no class expects 0: 5 stages of
# the 8-bit formats and 10 of the 16-bit ones, so the three-slot ring wraps
SPARSE_SHAPE = (512, 512, 640)
# 7 stages: more than the four ring slots, K no multiple of the operands' period 35, operands exact
FP_SHAPE = {"f32": (512, 512, 7 * fp.STAGE["f32"]), "f64": (512, 512, 7 * fp.STAGE["f64"])}


def _sparse(fmt):
    m, n, k = SPARSE_SHAPE
    assert sp.zero_classes(k) == 0 and k // sp.STAGE[fmt] in (5, 10)
    return _probe("sp:" + fmt, m, n, k)


def _fp(fmt):
    m, n, k = FP_SHAPE[fmt]
    assert k in (112, 56) and k % 35 != 0 and fp.k_exact(fmt, k) and k // fp.STAGE[fmt] > 4
    return _probe(fmt, m, n, k)


# ------------------------------------------------------------------ 1. sparse: every row, column and nibble


@pytest.mark.parametrize("fmt", SPARSE)
def test_sparse_check_sees_every_row_of_ac(dev, fmt):
    """512 launches: ``Ac[i][i % (K/2)]`` becomes another small value.  Row i is then wrong wherever ``Bt``
    is not 0 at the dense k the slot selects: 438 or 439 of 512 columns."""
    p = _sparse(fmt)
    idx = np.arange(p.m)
    slot = idx % (p.k // 2)
    # over the rows the slot is each slot of a group, in every group of a lane's bytes, in both lane
    # halves, both instructions of a stage and every stage
    stages = p.k // sp.STAGE[fmt]
    places = set(zip(*(np.asarray(c).tolist() for c in sp.kept_slot_coordinates(fmt, slot))))
    assert places == set(itertools.product(range(stages), range(2), range(2), range(8 // sp.ESIZE[fmt]), range(2)))
    want = _sweep(p, "ac", sp.encode(fmt, sp.sweep_values(fmt, p.values[0], 0)), True)
    assert want.min() >= 438 and want.max() <= 439


@pytest.mark.parametrize("fmt", SPARSE)
def test_sparse_check_sees_every_column_of_bt(dev, fmt):
    """512 launches: ``Bt[j][j % K]`` becomes another small value.  Column j is then wrong only in the rows
    that keep that k with a non-zero value: 204 to 206 of 512."""
    p = _sparse(fmt)
    idx = np.arange(p.n)
    hot = idx % p.k
    per_instruction = 64 // sp.ESIZE[fmt]  # dense k of one instruction: 64 bytes of a Bt row
    # every 16-byte chunk of an instruction (a lane half's low and high register half), both instructions
    chunks = set(zip((hot % sp.STAGE[fmt] // per_instruction).tolist(), (hot % per_instruction * sp.ESIZE[fmt] // 16).tolist()))
    assert chunks == set(itertools.product(range(2), range(4)))
    want = _sweep(p, "bt", sp.encode(fmt, sp.sweep_values(fmt, p.values[1], 1)), False)
    assert want.min() >= 204 and want.max() <= 206


@functools.lru_cache(maxsize=None)
def _nibble_plan():
    m, n, k = SPARSE_SHAPE
    group, new, moved = sp.nibble_sweep_plan(m, n, k)
    # every group of a row (so every nibble of a lane's index register in every instruction and
    # stage), every valid nibble as the replacement, both nibbles of a metadata byte
    assert set(group.tolist()) == set(range(k // 4)) and set(new.tolist()) == set(sp.VALID_NIBBLES)
    assert set((group % 2).tolist()) == {0, 1}
    print(f"nibble plan: {moved} of {m} rows moved on from their first candidate")
    return group, new


@pytest.mark.parametrize("fmt", SPARSE)
def test_sparse_check_reads_every_rows_metadata(dev, fmt):
    """512 launches: one nibble of row i, from group ``i % (K/4)`` on, becomes another valid nibble, chosen
    by the host model so that the row leaves the table somewhere (``sparse_reference.nibble_sweep_plan``)."""
    p = _sparse(fmt)
    group, new = _nibble_plan()
    wrong = sp.meta_with_nibbles(p.host["meta"], group, new)
    changed = np.argwhere(wrong != p.host["meta"])
    assert np.array_equal(changed, np.stack([np.arange(p.m), group // 2], axis=1))  # the one byte of every row
    want = _sweep(p, "meta", wrong, True)
    assert want.min() > 0 and want.max() <= p.n
    print(f"sp:{fmt} nibbles: {want.min()} .. {want.max()} mismatches a launch")


# ------------------------------------------------------------------ 2. fp: every row and column


@pytest.mark.parametrize("rows", [True, False], ids=["rows", "columns"])
@pytest.mark.parametrize("fmt", fp.FORMATS)
def test_fp_check_sees_every_row_and_column(dev, fmt, rows):
    """512 launches: ``A[i][i % K]`` plus ``MUL_A`` (``Bt[j][j % K]`` plus ``MUL_B``).  As in the dense probes a
    changed row is wrong in 438 or 439 of 512 columns and a changed column in 409 or 410 of 512 rows.
    For f64 a row's line crosses four tiles of 128 columns."""
    p = _fp(fmt)
    name = "a" if rows else "bt"
    v = fp.sweep_values(fmt, p.values[0 if rows else 1], 0 if rows else 1)
    assert set((np.arange(v.shape[0]) % p.k).tolist()) == set(range(p.k))  # every k of every stage
    # exact with every corrupted element in at once, so with each one alone
    other = np.abs(p.values[1 if rows else 0])
    assert (np.abs(v) @ other.T).max() < fp.EXACT_BELOW[fmt]
    wrong = v.astype(fp.NP_DTYPE[fmt])
    assert np.array_equal(wrong.astype(np.int64), v)
    want = _sweep(p, name, wrong, rows)
    assert set(want.tolist()) <= ({438, 439} if rows else {409, 410})


# ------------------------------------------------------------------ 3. NaN and infinity are counted

# Row 173 = 128 + 32 + 13.  In the 32 × 32 fragments (f32 and sparse: 2 wave rows of 128, fragments of 32,
# row of the fragment = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)) it is wave row 1, fragment 1, register 5
# of the upper lane half.  In the 16 × 16 fragments of f64 (4 wave rows of 64, fragments of 16, row of the
# fragment = (lane >> 4) + 4 reg) it is wave row 2, fragment 2, row 13: the last register, 3, of lane
# quarter 1 — wave, fragment, register and lane part are all non-zero in both maps.
NAN_ROW = 173
NAN_COLUMN = 300  # in the second tile column, wave column 0, second fragment

F32_NAN, F32_INF = 0x7FC00000, 0x7F800000
F64_NAN, F64_INF = 0x7FF8000000000000, 0x7FF0000000000000
FP_NONFINITE = [("f32", F32_NAN), ("f32", F32_INF), ("f64", F64_NAN), ("f64", F64_INF)]
SPARSE_NONFINITE = [("f16", 0x7E00), ("f16", 0x7C00), ("bf16", 0x7FC0), ("fp8", 0x7F), ("bf8", 0x7C), ("bf8", 0x7E)]


def _ids(cases):
    return [f"{fmt}-{bits:#x}" for fmt, bits in cases]


def _with_bits(host, i, kk, bits):
    """A copy of a host operand with the bit pattern ``bits`` at ``[i][kk]``."""
    out = host.copy()
    out.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[out.dtype.itemsize])[i, kk] = bits
    return out


def _one_launch_counts(p, name, i, kk, wrong_host, mismatch):
    """One launch with ``wrong_host[i][kk]`` in place of the element of ``name``: the total, the per-XCD counts
    against the launch's own tile map and the blocks per XCD are those of ``mismatch`` ``[m][n]``."""
    gpu = _gpu()
    tiles_n = p.n // p.tile_n
    tiles = (p.m // 256) * tiles_n
    target = p.t[name]
    counters = torch.zeros((gpu.ODH_NCOUNT,), dtype=torch.int32, device=p.device)
    tile_xcd = torch.full((tiles,), -1, dtype=torch.int32, device=p.device)
    clean = target[i, kk:kk + 1].clone()
    try:
        target[i, kk:kk + 1].copy_(torch.from_numpy(wrong_host[i, kk:kk + 1].copy()))
        p.launch(tile_xcd.data_ptr(), counters.data_ptr())
    finally:
        target[i, kk:kk + 1].copy_(clean)
    h = counters.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    tx = tile_xcd.cpu().numpy()
    _assert_operands_are_the_models(p)
    assert ((tx >= 0) & (tx < gpu.N_XCD)).all(), tx
    per_tile = mismatch.reshape(p.m // 256, 256, tiles_n, p.tile_n).sum(axis=(1, 3)).reshape(-1)
    want_xcd = np.zeros(gpu.N_XCD, dtype=np.int64)
    np.add.at(want_xcd, tx, per_tile)
    got_xcd = h[gpu.ODH_SLOT_ERR_XCD:gpu.ODH_SLOT_ERR_XCD + gpu.N_XCD]
    print(f"{p.fmt} {name}[{i}][{kk}]: {h[gpu.ODH_SLOT_GEMM_ERR]} counted, {int(mismatch.sum())} expected")
    assert h[gpu.ODH_SLOT_GEMM_ERR] == int(mismatch.sum()), (h[gpu.ODH_SLOT_GEMM_ERR], int(mismatch.sum()))
    assert np.array_equal(got_xcd, want_xcd), (got_xcd.tolist(), want_xcd.tolist())
    blocks = h[gpu.ODH_SLOT_XCD_BLOCKS:gpu.ODH_SLOT_XCD_BLOCKS + gpu.N_XCD]
    assert np.array_equal(blocks, np.bincount(tx, minlength=gpu.N_XCD))


@pytest.mark.parametrize("fmt,bits", FP_NONFINITE, ids=_ids(FP_NONFINITE))
def test_fp_check_counts_nan_and_inf(dev, fmt, bits):
    """One element of A becomes NaN or +inf: its row is wrong in all N columns — inf where ``Bt[j][k]`` is
    non-zero, NaN (inf · 0) where it is zero — and ``errors == N``, booked on the XCDs of the tiles of
    tile row 0."""
    p = _fp(fmt)
    i, kk = NAN_ROW, p.k - 3  # in the last stage
    if fmt == "f64":
        assert (i // 64, i % 64 // 16, i % 16 // 4, i % 4) == (2, 2, 3, 1)  # wave row, fragment, register, lane quarter
    else:
        row = i % 32
        assert (i // 128, i % 128 // 32) == (1, 1) and (row & 3) + 4 * (row >> 3) == 5 and (row >> 2) & 1 == 1
    host = _with_bits(p.host["a"], i, kk, bits)
    with np.errstate(invalid="ignore"):
        mismatch = (host.astype(np.float64) @ p.host["bt"].astype(np.float64).T) != p.expect
    assert mismatch[i].all() and int(mismatch.sum()) == p.n
    if np.isinf(host[i, kk]):
        assert (p.values[1][:, kk] == 0).any() and (p.values[1][:, kk] != 0).any()  # both inf and NaN occur
    _one_launch_counts(p, "a", i, kk, host, mismatch)


def _sparse_product_f64(p, fmt, host):
    return sp.product_per_slot_f64(sp.decode(fmt, host["ac"]), sp.unpack_meta(host["meta"]), sp.decode(fmt, host["bt"]))


@pytest.mark.parametrize("fmt,bits", SPARSE_NONFINITE, ids=_ids(SPARSE_NONFINITE))
def test_sparse_check_counts_nan_and_inf_in_ac(dev, fmt, bits):
    """One kept element becomes NaN or +inf: ``errors == N`` in its row, as in the dense checks."""
    p = _sparse(fmt)
    i, slot = NAN_ROW, p.k // 2 - 3  # in the last stage
    row = i % 32
    assert (i // 128, i % 128 // 32) == (1, 1) and (row & 3) + 4 * (row >> 3) == 5 and (row >> 2) & 1 == 1
    host = dict(p.host, ac=_with_bits(p.host["ac"], i, slot, bits))
    assert not np.isfinite(sp.decode(fmt, host["ac"])[i, slot])
    mismatch = _sparse_product_f64(p, fmt, host) != p.expect
    assert mismatch[i].all() and int(mismatch.sum()) == p.n
    _one_launch_counts(p, "ac", i, slot, host["ac"], mismatch)


@pytest.mark.parametrize("fmt,bits", SPARSE_NONFINITE, ids=_ids(SPARSE_NONFINITE))
def test_sparse_check_counts_nan_and_inf_in_bt(dev, fmt, bits):
    """One element of Bt becomes NaN or +inf.  Only the rows that keep that dense position multiply it,
    and a kept zero times NaN or inf is NaN too: the column is wrong in exactly the rows that keep k."""
    p = _sparse(fmt)
    j, kk = NAN_COLUMN, p.k - 6  # in the last stage
    host = dict(p.host, bt=_with_bits(p.host["bt"], j, kk, bits))
    assert not np.isfinite(sp.decode(fmt, host["bt"])[j, kk])
    mismatch = _sparse_product_f64(p, fmt, host) != p.expect
    keep = sp.keep_mask(p.m, p.k)[:, kk]
    assert np.array_equal(mismatch[:, j], keep) and int(mismatch.sum()) == int(keep.sum()) and 0 < keep.sum() < p.m
    assert (sp.decompress(p.values[0], p.host["meta"])[keep, kk] == 0).any()  # kept zeros meet it too
    _one_launch_counts(p, "bt", j, kk, host["bt"], mismatch)


# ------------------------------------------------------------------ 4. sparse store kernels: value against value

TORCH_DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16, "i8": torch.int8, "fp8": torch.float8_e4m3fn,
               "bf8": torch.float8_e5m2}
STORE_CASES = [("fp8", False), ("bf8", False), ("i8", False), ("f16", False), ("bf16", False), ("bf16", True)]
# a value no case expects: every product is at most 2^128 resp. 2^14 in magnitude
PREFILL = {torch.float32: 3e38, torch.int32: 2 ** 30}


@pytest.mark.parametrize("fmt,swap", STORE_CASES, ids=[f + ("-swapped" if s else "") for f, s in STORE_CASES])
def test_sparse_store_multiplies_every_value_by_every_value(dev, fmt, swap):
    """All 256 × 256 pairs of fp8 codes (subnormals, ±448 and both NaN codes included), of bf8 codes
    (subnormals, ±57344, both infinities and the six NaN codes) and of i8 values, the 256 halves of the
    dense f16 case, and two sets of 256 bf16 values, big against small and small against big:
    every output is one product (``sparse_reference.onehot_case``)."""
    ac, meta, bt, want = sp.onehot_case(fmt, swap)
    out = torch.int32 if fmt == "i8" else torch.float32
    assert not (want == PREFILL[out]).any()
    c = torch.full(want.shape, PREFILL[out], dtype=out, device=dev)
    as_fmt = lambda x: torch.from_numpy(x).view(TORCH_DTYPE[fmt]).to(dev)  # noqa: E731
    _gpu().sparse_gemm(fmt, as_fmt(ac), torch.from_numpy(meta).to(dev), as_fmt(bt), out=c)
    _assert_store_exact(f"sparse {fmt} value i × value j", c.cpu().numpy(), want)
