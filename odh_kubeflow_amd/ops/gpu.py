"""Python side of the MI355X node-agent kernels (``csrc/gpu_probe.hip``).

* :func:`gemm_bf16` — the MFMA bf16 GEMM (``C = A · Btᵀ``, fp32 out) on torch tensors.
* :class:`GpuProbe` — the torch-side harness of the probe kernels, for kernel tests and
  microbenchmarks: a resident bf16 GEMM whose integer-valued operands make every output
  element checkable bit-exactly on the GPU, plus an HBM3E pattern write/verify sweep.  Sized
  like the start-up probe (:data:`PROBE_SHAPE`, :data:`PROBE_HBM_BYTES`): 4096×4096 outputs
  are 256 tiles of 256², one workgroup per CU of the 256-CU chip, so every CU of every XCD
  runs MFMA work; K=1024 keeps the GEMM at ≈30 µs, and the 256 MiB sweep, interleaved over
  every HBM3E stack and channel, tests them all.  It runs the kernels three ways: eager on
  one stream, overlapped (sweep and GEMM on two streams), and as a hipGraph captured once
  (forked streams, counter reset, 128-byte read-back) and replayed with one launch per
  :meth:`GpuProbe.run`; in a graph the kernels time themselves (``wall_clock64`` spans),
  since events cannot split a graph launch.  Reports matrix-core TFLOP/s, HBM GB/s,
  mismatches (attributed to the XCD that computed them) and how many of the 8 XCDs ran
  workgroups.
* :func:`mx_fill`, :func:`mx_gemm`, :func:`mx_probe` — the block-scaled path of the matrix cores
  (``v_mfma_scale_f32_32x32x64_f8f6f4``) in its five operand formats (FP8, BF8, FP6, BF6, MXFP4)
  on uint8 code tensors: the same exact in-register check, against a 15 × 21 table
  (``odh-gpu-probe --mx``).
* :func:`dense_fill`, :func:`dense_gemm`, :func:`dense_probe` — the FP16 and INT8 paths
  (``v_mfma_f32_32x32x16_f16``, ``v_mfma_i32_32x32x32_i8``) on float16 / int8 tensors: the same
  check against the bf16 probe's 5 × 7 closed form (``odh-gpu-probe --dtypes``).
* :func:`fp_fill`, :func:`fp_gemm`, :func:`fp_probe` — the FP32 and FP64 paths
  (``v_mfma_f32_32x32x2_f32``, ``v_mfma_f64_16x16x4_f64``) on float32 / float64 tensors: the same
  check against that closed form times odd constants (``odh-gpu-probe --fp``).
* :func:`sparse_fill`, :func:`sparse_gemm`, :func:`sparse_probe` — the 2:4 structured-sparsity path
  (``v_smfmac_*`` on bf16, f16, int8, fp8 and bf8) on a compressed A, its metadata and a dense Bt: the
  same check against a 30 × 7 table (``odh-gpu-probe --sparse``); :func:`sparse_compress` and
  :func:`sparse_decompress` turn a dense tensor into that layout and back, in plain torch.
* :func:`lds_probe`, :func:`lds_tr_read`, :func:`lds_xlane`, :func:`transpose_codes`, :func:`mx_transpose` — the LDS
  itself, the transposing LDS reads (``ds_read_b64_tr_b16`` / ``_b8`` / ``_b4``, ``ds_read_b96_tr_b6``) and the lane
  exchanges (``odh-gpu-probe --lds``), and the transposer of packed codes built on those reads.
* :func:`mx_quantize`, :func:`cvt_encode`, :func:`cvt_probe` — the hardware converters that make those codes
  (``v_cvt_scalef32_pk_fp8_f32`` and its kin, ``v_cvt_pk_bf16_f32``): OCP MX quantisation of float32 rows into the
  layout :func:`mx_gemm` reads, the bare instruction, and the exact check of every rounding case on every SIMD
  (``odh-gpu-probe --cvt``); :func:`cvt_family` is that check's family of inputs and expected codes.
* :func:`probe_devices` / :func:`xgmi_ring_check` — the same harness over several GPUs; a link is
  :func:`link_check` of two probes, against :attr:`GpuProbe.pattern_seed` (the seed of the pattern the source's
  buffer holds, whichever path wrote it), and two probes on one GPU make a link too.
* The shipped start-up probe is none of these: it is the torch-free ``odh-gpu-probe`` init
  container (``csrc/probe_cli.cpp``, :mod:`.probe_main`), which launches the same kernels
  from plain hipMalloc'd buffers, serially on the null stream.
* :class:`LoadGenerator` — synthetic MFMA load at a given duty cycle (culler benchmarks).

The library's C ABI is declared in ``csrc/gpu_probe.h``; :data:`SIGNATURES` and the ``ODH_*``
counter slots below mirror it (``tests/test_probe_abi.py`` compares the two).  The library
is loaded with ctypes **after** ``import torch`` so it binds to the HIP runtime torch already
loaded.  If the ``.so`` is missing on a machine with a GPU the
calls raise :class:`NativeLibraryMissing` instead of silently falling back.
"""

from __future__ import annotations

import ctypes
import os
import threading
import time
from typing import Dict, List, Optional, Sequence

from .build import lib_path

PROBE_LIB = "libodh_gpu_probe.so"
BM = BN = 128
BK = 32
N_XCD = 8
PROBE_SHAPE = (4096, 4096, 1024)  # M, N, K of the start-up probe GEMM (256 tiles of 256²)
PROBE_HBM_BYTES = 256 << 20

# the counter block (csrc/gpu_probe.h): ODH_NCOUNT × i32; the CLI and graph layouts share
# slots 20-23 and are never used on the same block
ODH_NCOUNT = 32
ODH_N_XCD = N_XCD
ODH_SLOT_XCD_BLOCKS = 0  # [ODH_N_XCD] workgroups per XCD
ODH_SLOT_ERR_XCD = 8  # [ODH_N_XCD] GEMM mismatches per XCD
ODH_SLOT_GEMM_ERR = 16  # u32
ODH_SLOT_HBM_ERR = 18  # u64
ODH_SLOT_CLI_XGMI_ERR = 20  # u64 (odh-gpu-probe only)
ODH_SLOT_CLI_RCCL_ERR = 22  # u64 (odh-gpu-probe only)
ODH_SLOT_GRAPH_GEMM_SPAN = 20  # 2 × u64: ~begin, end (odh_probe_graph_create)
ODH_SLOT_GRAPH_SWEEP_SPAN = 24  # 2 × u64
# operand formats of the block-scaled (MX) kernels: the hardware's format codes
ODH_MX_FP8 = 0  # OCP e4m3fn, one byte per element
ODH_MX_FP4 = 4  # e2m1, two elements per byte (even k in the low nibble)
ODH_MX_BF8 = 1  # OCP e5m2, one byte per element
ODH_MX_FP6 = 2  # e2m3, packed: element k in bits [6k, 6k + 6) of the row, little endian
ODH_MX_BF6 = 3  # e3m2, packed as FP6
ODH_MX_CLASSES = 315  # floats in the table of expected values
MX_FORMATS = {"fp8": ODH_MX_FP8, "fp4": ODH_MX_FP4}  # what ``--mx`` of the "mx" notebooks checks
MX_EXTRA_FORMATS = {"bf8": ODH_MX_BF8, "fp6": ODH_MX_FP6, "bf6": ODH_MX_BF6}  # the instruction's other three
MX_ALL_FORMATS = {**MX_FORMATS, **MX_EXTRA_FORMATS}
MX_TABLE = (15, 21)  # expected values of the MX probe operands, by (i mod 15, j mod 21)
# operand formats of the dense FP16 / INT8 kernels (csrc/gpu_probe_dense.h)
ODH_DT_F16 = 1  # IEEE half, fp32 accumulation
ODH_DT_I8 = 2  # int8, int32 accumulation
ODH_DT_I8_MUL_A = 25  # the i8 probe operands are these odd multiples of the bf16 probe's A ...
ODH_DT_I8_MUL_B = 41  # ... and Bt: the expected product is 1025 × the bf16 probe's
DENSE_FORMATS = {"f16": ODH_DT_F16, "i8": ODH_DT_I8}
# operand formats of the FP32 / FP64 kernels (csrc/gpu_probe_fp.h): the codes are the element sizes
ODH_FP_F32 = 4  # float, fp32 accumulation
ODH_FP_F64 = 8  # double, fp64 accumulation
ODH_FP_F32_MUL_A = 25  # the f32 probe operands are the i8 probe's multiples of the bf16 probe's A ...
ODH_FP_F32_MUL_B = 41  # ... and Bt: 1025 × the bf16 probe's product
ODH_FP_F64_MUL_A = 1048573  # the f64 probe operands: odd 20-bit multiples ...
ODH_FP_F64_MUL_B = 1048575  # ... whose products toggle 41 mantissa bits
FP_FORMATS = {"f32": ODH_FP_F32, "f64": ODH_FP_F64}
# operand formats of the 2:4 structured-sparsity kernels (csrc/gpu_probe_sparse.h)
ODH_SP_BF16 = 0  # bfloat16, fp32 accumulation
ODH_SP_F16 = 1  # IEEE half, fp32 accumulation
ODH_SP_I8 = 2  # int8, int32 accumulation
ODH_SP_FP8 = 3  # OCP e4m3fn on both operands, fp32 accumulation
ODH_SP_BF8 = 4  # OCP e5m2 on both operands, fp32 accumulation
ODH_SP_CLASSES = 210  # ints in the table of expected values
SPARSE_FORMATS = {"bf16": ODH_SP_BF16, "f16": ODH_SP_F16, "i8": ODH_SP_I8, "fp8": ODH_SP_FP8, "bf8": ODH_SP_BF8}
SPARSE_TABLE = (30, 7)  # expected sums of the sparse probe operands, by (i mod 30, j mod 7)
# destination formats of the converter kernels (csrc/gpu_probe_cvt.h): the hardware's format codes, and bf16
ODH_CVT_FP8 = 0  # OCP e4m3fn
ODH_CVT_BF8 = 1  # OCP e5m2
ODH_CVT_FP6 = 2  # e2m3
ODH_CVT_BF6 = 3  # e3m2
ODH_CVT_FP4 = 4  # e2m1
ODH_CVT_BF16 = 5  # bfloat16: no scale
ODH_CVT_BLOCKS = 256  # workgroups of the fused check: one per CU
ODH_CVT_TABLE = 256  # bytes of its scale table
CVT_FORMATS = {"fp8": ODH_CVT_FP8, "bf8": ODH_CVT_BF8, "fp4": ODH_CVT_FP4, "fp6": ODH_CVT_FP6, "bf6": ODH_CVT_BF6,
               "bf16": ODH_CVT_BF16}  # what ``--cvt`` checks, in its order

# checks of the LDS step (csrc/gpu_probe_lds.h)
ODH_LDS_MEM = 0  # every dword of a CU's 160 KiB, written and read in different widths by different waves
ODH_LDS_TR16 = 1  # ds_read_b64_tr_b16
ODH_LDS_TR8 = 2  # ds_read_b64_tr_b8
ODH_LDS_TR4 = 3  # ds_read_b64_tr_b4
ODH_LDS_TR6 = 4  # ds_read_b96_tr_b6
ODH_LDS_XLANE = 5  # ds_bpermute / ds_permute / ds_swizzle, DPP, v_readlane / v_writelane, v_permlane16/32_swap
ODH_LDS_BLOCKS = 256  # workgroups of a fused check: one per CU
ODH_LDS_TABLE = 1024  # bytes of its key table
ODH_LDS_CU_WORDS = 64  # dwords of the bitmap of CUs behind a counter block
ODH_LDS_TR_RAW = 256  # added to odh_lds_tr_read's check: the alignment of the addresses is not checked (measuring)
# element formats of odh_transpose_codes
ODH_TC_B16 = 0  # 16-bit elements
ODH_TC_B8 = 1  # one byte per element
ODH_TC_B4 = 2  # two nibbles per byte, even index low
ODH_TC_B6 = 3  # element k in bits [6k, 6k + 6) of a row
LDS_CHECKS = {"mem": ODH_LDS_MEM, "tr16": ODH_LDS_TR16, "tr8": ODH_LDS_TR8, "tr4": ODH_LDS_TR4, "tr6": ODH_LDS_TR6,
              "xlane": ODH_LDS_XLANE}  # what ``--lds`` checks, in its order
LDS_XLANE_OPS = {"bpermute": 0, "permute": 1, "swizzle": 2, "dpp": 3, "readlane": 4, "writelane": 5,
                 "permlane16_swap": 6, "permlane32_swap": 7}  # ``op`` of :func:`lds_xlane`
LDS_XLANE_ARGS = {"bpermute": 65, "permute": 65, "swizzle": 12, "dpp": 55, "readlane": 64, "writelane": 64,
                  "permlane16_swap": 4, "permlane32_swap": 4}  # selectors of each
# format -> (element format of the transposer, bits of an element)
TRANSPOSE_FORMATS = {"bf16": (ODH_TC_B16, 16), "f16": (ODH_TC_B16, 16), "fp8": (ODH_TC_B8, 8), "bf8": (ODH_TC_B8, 8),
                     "fp4": (ODH_TC_B4, 4), "fp6": (ODH_TC_B6, 6), "bf6": (ODH_TC_B6, 6)}
# operand formats of the 16×16 matrix-core kernels (csrc/gpu_probe_m16.h)
ODH_M16_BF16 = 0  # bfloat16, 16x16x32, fp32 accumulation
ODH_M16_F16 = 1  # IEEE half, 16x16x32, fp32 accumulation
ODH_M16_I8 = 2  # int8, 16x16x64, int32 accumulation
ODH_M16_FP8 = 3  # OCP e4m3fn on both operands, block scaled, 16x16x128, fp32 accumulation
ODH_M16_FP4 = 4  # e2m1 on both operands, block scaled, 16x16x128, fp32 accumulation
M16_FORMATS = {"bf16": ODH_M16_BF16, "f16": ODH_M16_F16, "i8": ODH_M16_I8, "fp8": ODH_M16_FP8, "fp4": ODH_M16_FP4}

_vp, _i, _u32, _sz, _long = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_long
# name -> (restype, argtypes) of every function of csrc/gpu_probe.h that Python calls
SIGNATURES = {
    "odh_gemm_shape_ok": (_i, [_i, _i, _i]),
    "odh_gemm_tiles": (_i, [_i, _i, _i]),
    "odh_error_string": (ctypes.c_char_p, [_i]),
    "odh_wall_clock_khz": (_i, [_i]),
    "odh_probe_fill": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "odh_gemm_bf16": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "odh_gemm_bf16_128": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "odh_probe_verify": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "odh_probe_gemm_verify": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "odh_hbm_write": (_i, [_vp, _sz, _u32, _i, _vp]),
    "odh_hbm_check": (_i, [_vp, _sz, _u32, _vp, _vp]),
    "odh_const_check": (_i, [_vp, _sz, _u32, _vp, _vp]),
    "odh_peer_enable": (_i, [_i, _i]),
    "odh_busy": (_i, [_vp, _i, _i, _vp]),
    "odh_probe_graph_create": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp, _vp, _i, ctypes.POINTER(_vp)]),
    "odh_probe_graph_launch": (_i, [_vp, _vp]),
    "odh_probe_graph_destroy": (None, [_vp]),
    # A/B entry points (microbenchmarks, kernel numerics tests)
    "odh_gemm_bf16_256_variant": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "odh_probe_gemm_verify_2buf": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "odh_probe_gemm_verify_deep": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "odh_hbm_write_variant": (_i, [_vp, _sz, _u32, _i, _i, _vp]),
    "odh_hbm_check_variant": (_i, [_vp, _sz, _u32, _vp, _i, _i, _vp]),
    # block-scaled FP8 / MXFP4 (csrc/gpu_probe_mx.h)
    "odh_mx_zero_classes": (_i, [_i]),
    "odh_mx_fill": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "odh_mx_gemm": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "odh_mx_probe_gemm_verify": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    # dense FP16 / INT8 (csrc/gpu_probe_dense.h)
    "odh_dense_fill": (_i, [_i, _vp, _vp, _i, _i, _i, _vp]),
    "odh_dense_gemm": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "odh_dense_probe_gemm_verify": (_i, [_i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    # FP32 / FP64 (csrc/gpu_probe_fp.h)
    "odh_fp_tiles": (_i, [_i, _i, _i]),
    "odh_fp_fill": (_i, [_i, _vp, _vp, _i, _i, _i, _vp]),
    "odh_fp_gemm": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "odh_fp_probe_gemm_verify": (_i, [_i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    # 2:4 structured sparsity (csrc/gpu_probe_sparse.h)
    "odh_sparse_zero_classes": (_i, [_i]),
    "odh_sparse_fill": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "odh_sparse_gemm": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "odh_sparse_probe_gemm_verify": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    # converters (csrc/gpu_probe_cvt.h)
    "odh_cvt_family_size": (_u32, [_i]),
    "odh_cvt_family": (_i, [_i, _u32, _u32, _vp, _vp, _vp]),
    "odh_cvt_fill": (_i, [_i, _vp, _vp]),
    "odh_cvt_encode": (_i, [_i, _vp, _vp, _vp, _long, _long, _vp]),
    "odh_cvt_quantize": (_i, [_i, _vp, _vp, _vp, _long, _long, _vp]),
    "odh_cvt_probe_verify": (_i, [_i, _vp, _vp, _vp]),
    # the LDS step and the transposer of packed codes (csrc/gpu_probe_lds.h)
    "odh_lds_cases": (ctypes.c_ulonglong, [_i]),
    "odh_lds_fault_count": (ctypes.c_ulonglong, [_i, _i]),
    "odh_lds_fill": (_i, [_i, _vp, _vp]),
    "odh_lds_probe_verify": (_i, [_i, _vp, _vp, _vp]),
    "odh_lds_tr_read": (_i, [_i, _vp, ctypes.c_uint, _vp, _vp, _vp]),
    "odh_lds_xlane": (_i, [_i, _i, _vp, _vp, _vp]),
    "odh_transpose_codes": (_i, [_i, _vp, _vp, _long, _long, _vp]),
    # the 16×16 matrix-core shapes (csrc/gpu_probe_m16.h)
    "odh_m16_gemm": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "odh_m16_probe_gemm_verify": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "odh_m16_one": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    # the start-up probe program (ops/probe_main.py)
    "odh_probe_cli": (_i, [_i, ctypes.POINTER(ctypes.c_char_p)]),
}


def bind(lib, names=SIGNATURES):
    """Give the ctypes functions ``names`` of ``lib`` their :data:`SIGNATURES` (an export the
    library lacks raises ``AttributeError`` here, not at its first call)."""
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = SIGNATURES[name]
    return lib


class NativeLibraryMissing(RuntimeError):
    pass


class HipError(RuntimeError):
    pass


_lib = None
_lib_lock = threading.Lock()


def load_library(build_if_missing: bool = False):
    """Load (once) and return the ctypes handle of ``libodh_gpu_probe.so``."""
    global _lib
    if _lib is not None:
        return _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        import torch  # noqa: F401  -- must own libamdhip64.so.7 before we dlopen

        path = lib_path(PROBE_LIB)
        if not os.path.exists(path):
            if build_if_missing:
                from .build import build

                build(verbose=False)
            if not os.path.exists(path):
                raise NativeLibraryMissing(f"{path} not built; run `python -m odh_kubeflow_amd.ops.build`")
        lib = bind(ctypes.CDLL(path))
        _lib = lib
        return lib


def _check(rc: int) -> None:
    if rc != 0:
        msg = load_library().odh_error_string(rc)
        raise HipError(f"HIP error {rc}: {msg.decode() if msg else '?'}")


def _u64(h: Sequence[int], i: int) -> int:
    """The u64 counter in i32 slots ``i`` and ``i + 1``."""
    return (h[i] & 0xFFFFFFFF) | ((h[i + 1] & 0xFFFFFFFF) << 32)


def _stream_ptr(device) -> int:
    import torch

    return torch.cuda.current_stream(device).cuda_stream


def gemm_shape_ok(m: int, n: int, k: int) -> bool:
    return m > 0 and n > 0 and k > 0 and m % BM == 0 and n % BN == 0 and k % BK == 0


def gemm_tiles(m: int, n: int, k: int) -> int:
    """Workgroups the GEMM launches for this shape (256² tiles when they divide it, else 128²)."""
    return load_library().odh_gemm_tiles(m, n, k)


def fused_verify_ok(m: int, n: int, k: int) -> bool:
    return gemm_shape_ok(m, n, k) and m % 256 == 0 and n % 256 == 0 and k % 64 == 0


def probe_check_vacuous(k: int) -> bool:
    """The probe operands repeat in k with period 35 and sum to zero over one period in every
    ``(i mod 5, j mod 7)`` class, so at ``K % 35 == 0`` the expected product is 0 everywhere and
    matrix cores that return zeros would pass the check.  ``GpuProbe`` and ``odh-gpu-probe``
    refuse such shapes; the kernels themselves take them."""
    return k % 35 == 0


def gemm_bf16(a, bt, out=None, tile_xcd=None, xcd_blocks=None, tile: Optional[int] = None):
    """``C[M,N] = A[M,K] · Bt[N,K]ᵀ`` in fp32 on the matrix cores.

    Shapes must be multiples of the 128×128×32 tile (checked here, before launch); the
    256×256×64 LDS-DMA kernel runs when it divides the shape (``tile=128`` forces the
    smaller kernel, for A/B measurements).
    """
    import torch

    if a.dtype != torch.bfloat16 or bt.dtype != torch.bfloat16:
        raise TypeError("gemm_bf16 expects bfloat16 operands")
    if a.dim() != 2 or bt.dim() != 2 or a.shape[1] != bt.shape[1]:
        raise ValueError(f"shape mismatch: A{tuple(a.shape)} Bt{tuple(bt.shape)}")
    if not (a.is_cuda and bt.is_cuda) or a.device != bt.device:
        raise ValueError("operands must live on the same GPU")
    m, k = a.shape
    n = bt.shape[0]
    if not gemm_shape_ok(m, n, k):
        raise ValueError(f"M,N must be multiples of {BM}/{BN} and K of {BK}; got {m},{n},{k}")
    a = a.contiguous()
    bt = bt.contiguous()
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    elif out.shape != (m, n) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous fp32 [M,N] tensor")
    if tile_xcd is not None and tile_xcd.numel() < (m // BM) * (n // BN):
        raise ValueError("tile_xcd too small")
    if xcd_blocks is not None and xcd_blocks.numel() < N_XCD:
        raise ValueError("xcd_blocks too small")
    lib = load_library()
    fn = lib.odh_gemm_bf16_128 if tile == 128 else lib.odh_gemm_bf16
    _check(fn(a.data_ptr(), bt.data_ptr(), out.data_ptr(), m, n, k,
                             tile_xcd.data_ptr() if tile_xcd is not None else None,
                             xcd_blocks.data_ptr() if xcd_blocks is not None else None, _stream_ptr(a.device)))
    return out


def _mx_format(fmt) -> int:
    code = MX_ALL_FORMATS.get(fmt, fmt) if isinstance(fmt, str) else fmt
    if code not in MX_ALL_FORMATS.values():
        raise ValueError(f"MX format must be one of {sorted(MX_ALL_FORMATS)}; got {fmt!r}")
    return code


# The public layout of a row, by format code: elements per stage of the kernel, and row bytes as a
# fraction (numerator, denominator) of K.  One element per byte (FP8, BF8), two (FP4), or four in
# three bytes (FP6, BF6: element k in bits ``[6k, 6k + 6)`` of the row): a stage of a row is 64
# bytes, or 96 of the packed 6-bit formats.
_MX_LAYOUT = {
    ODH_MX_FP8: (64, 1, 1),
    ODH_MX_BF8: (64, 1, 1),
    ODH_MX_FP4: (128, 1, 2),
    ODH_MX_FP6: (128, 3, 4),
    ODH_MX_BF6: (128, 3, 4),
}


def _mx_stage(code: int) -> int:
    """Elements of a row per stage."""
    return _MX_LAYOUT[code][0]


def mx_row_bytes(fmt, k: int) -> int:
    """Bytes of a row of ``k`` elements in the public layout."""
    _, num, den = _MX_LAYOUT[_mx_format(fmt)]
    return k // den * num


def mx_shape_ok(fmt, m: int, n: int, k: int) -> bool:
    """256² output tiles, and K in whole stages: 64 FP8 or BF8 elements, 128 FP4, FP6 or BF6."""
    bk = _mx_stage(_mx_format(fmt))
    return m > 0 and n > 0 and k > 0 and m % 256 == 0 and n % 256 == 0 and k % bk == 0


def mx_zero_classes(k: int) -> int:
    """How many of the 315 ``(i mod 15, j mod 21)`` classes of the MX probe operands expect 0 at
    this K (-1: K is no positive multiple of 128).  Host arithmetic only."""
    return load_library().odh_mx_zero_classes(k)


def _same_gpu_2d(family: str, what: str, dtype, dtype_error: str, *ts) -> None:
    """What every MX, dense, fp and sparse entry point asks of its tensors before launch: ``dtype``, 2-D, one
    GPU, contiguous."""
    if any(t.dtype != dtype for t in ts):
        raise TypeError(dtype_error)
    if any(t.dim() != 2 for t in ts):
        raise ValueError(f"{family} {what} are 2-D")
    if not all(t.is_cuda and t.device == ts[0].device for t in ts):
        raise ValueError(f"{what} must live on the same GPU")
    if not all(t.is_contiguous() for t in ts):
        raise ValueError(f"{what} must be contiguous")


def _fused_check(dev, m: int, n: int, k: int, launch, tiles: Optional[int] = None) -> dict:
    """A fused check on a fresh counter block, and its report.  ``launch(tile_xcd, counters, stream)``
    is the one kernel launch; its time is taken with events around it.  ``tiles`` is the kernel's
    workgroup count (256² output tiles unless given)."""
    import torch

    if tiles is None:
        tiles = (m // 256) * (n // 256)
    with torch.cuda.device(dev):
        counters = torch.zeros((ODH_NCOUNT,), dtype=torch.int32, device=dev)
        tile_xcd = torch.full((tiles,), -1, dtype=torch.int32, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _check(launch(tile_xcd.data_ptr(), counters.data_ptr(), _stream_ptr(dev)))
        e1.record()
        e1.synchronize()
        h = counters.cpu().tolist()
    ms = e0.elapsed_time(e1)
    return {
        "errors": h[ODH_SLOT_GEMM_ERR] & 0xFFFFFFFF,
        "err_xcd": [x & 0xFFFFFFFF for x in h[ODH_SLOT_ERR_XCD:ODH_SLOT_ERR_XCD + ODH_N_XCD]],
        "xcd_blocks": h[ODH_SLOT_XCD_BLOCKS:ODH_SLOT_XCD_BLOCKS + ODH_N_XCD],
        "ms": ms, "tflops": 2.0 * m * n * k / (ms * 1e-3) / 1e12 if ms > 0 else 0.0,
    }


def _mx_operands(fmt, a, bt, sa, sbt):
    """Checks of the MX entry points, before launch: uint8, one GPU, contiguous, and the public
    layout (A ``[M, row bytes]``, Bt ``[N, row bytes]`` codes, scales ``[rows, K/32]``; row bytes are
    K, K/2 for FP4, or 3K/4 for FP6 / BF6).  Returns the format code, M, N, K."""
    import torch

    code = _mx_format(fmt)
    _same_gpu_2d("MX", "operands and scales", torch.uint8, "MX operands and scales are uint8 codes", a, bt, sa, sbt)
    stage, num, den = _MX_LAYOUT[code]
    row_bytes = a.shape[1]
    m, n, k = a.shape[0], bt.shape[0], row_bytes * den // num
    if num != 1 and row_bytes % (stage * num // den):  # packed 6-bit: a stage of a row is 96 bytes
        raise ValueError(f"rows of packed 6-bit codes are multiples of {stage * num // den} bytes; "
                         f"got A{tuple(a.shape)}")
    if bt.shape[1] != row_bytes or not mx_shape_ok(code, m, n, k):
        raise ValueError(f"M,N must be multiples of 256 and K of {stage}; "
                         f"got A{tuple(a.shape)} Bt{tuple(bt.shape)}")
    if tuple(sa.shape) != (m, k // 32) or tuple(sbt.shape) != (n, k // 32):
        raise ValueError(f"scales must be [{m},{k // 32}] and [{n},{k // 32}]; "
                         f"got {tuple(sa.shape)} {tuple(sbt.shape)}")
    return code, m, n, k


def mx_fill(fmt, a, bt, sa, sbt, table) -> None:
    """The probe operands encoded for ``fmt`` (a name of :data:`MX_ALL_FORMATS`), their E8M0 block scales and
    the 15 × 21 fp32 table of expected values, written into the given tensors."""
    import torch

    code, m, n, k = _mx_operands(fmt, a, bt, sa, sbt)
    if (table.dtype != torch.float32 or tuple(table.shape) != MX_TABLE or not table.is_contiguous()
            or table.device != a.device):
        raise ValueError("table must be a contiguous fp32 [15,21] tensor on the operands' GPU")
    _check(load_library().odh_mx_fill(code, a.data_ptr(), bt.data_ptr(), sa.data_ptr(), sbt.data_ptr(),
                                      table.data_ptr(), m, n, k, _stream_ptr(a.device)))


def mx_gemm(fmt, a, bt, sa, sbt, out=None):
    """``C[M,N] = (A ∘ sA) · (Bt ∘ sBt)ᵀ`` in fp32 on the block-scaled matrix cores
    (``v_mfma_scale_f32_32x32x64_f8f6f4``): uint8 codes, one E8M0 scale per 32 k of a row."""
    import torch

    code, m, n, k = _mx_operands(fmt, a, bt, sa, sbt)
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    elif tuple(out.shape) != (m, n) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != a.device:
        raise ValueError("out must be a contiguous fp32 [M,N] tensor on the operands' GPU")
    _check(load_library().odh_mx_gemm(code, a.data_ptr(), bt.data_ptr(), sa.data_ptr(), sbt.data_ptr(),
                                      out.data_ptr(), m, n, k, _stream_ptr(a.device)))
    return out


def mx_verify(fmt, a, bt, sa, sbt, table) -> dict:
    """The fused check of the given operands against ``table`` on a fresh counter block; the
    kernel's time is taken with events around its one launch."""
    code, m, n, k = _mx_operands(fmt, a, bt, sa, sbt)

    def launch(tile_xcd, counters, stream):
        return load_library().odh_mx_probe_gemm_verify(code, a.data_ptr(), bt.data_ptr(), sa.data_ptr(), sbt.data_ptr(),
                                                       table.data_ptr(), m, n, k, tile_xcd, counters, stream)

    return _fused_check(a.device, m, n, k, launch)


def mx_probe(device: int, fmt, m: int = PROBE_SHAPE[0], n: int = PROBE_SHAPE[1], k: int = PROBE_SHAPE[2]) -> dict:
    """One block-scaled probe of a GPU in any of the five formats: fill, then the GEMM with the check fused into its
    epilogue.  ``errors``, ``err_xcd``, ``xcd_blocks``, ``ms`` and ``tflops`` of the check kernel."""
    import torch

    code = _mx_format(fmt)
    if not mx_shape_ok(code, m, n, k):
        raise ValueError("MX probe shape must be tile aligned")
    dev = torch.device("cuda", device)
    rb = mx_row_bytes(code, k)
    with torch.cuda.device(dev):
        a = torch.empty((m, rb), dtype=torch.uint8, device=dev)
        bt = torch.empty((n, rb), dtype=torch.uint8, device=dev)
        sa = torch.empty((m, k // 32), dtype=torch.uint8, device=dev)
        sbt = torch.empty((n, k // 32), dtype=torch.uint8, device=dev)
        table = torch.empty(MX_TABLE, dtype=torch.float32, device=dev)
        mx_fill(code, a, bt, sa, sbt, table)
        return mx_verify(code, a, bt, sa, sbt, table)


def _dense_format(fmt) -> int:
    code = DENSE_FORMATS.get(fmt, fmt) if isinstance(fmt, str) else fmt
    if code not in DENSE_FORMATS.values():
        raise ValueError(f"dense format must be one of {sorted(DENSE_FORMATS)}; got {fmt!r}")
    return code


def dense_shape_ok(fmt, m: int, n: int, k: int) -> bool:
    """256² output tiles, and K in stages of 64 bytes per row: 32 halves or 64 int8."""
    bk = 64 if _dense_format(fmt) == ODH_DT_I8 else 32
    return m > 0 and n > 0 and k > 0 and m % 256 == 0 and n % 256 == 0 and k % bk == 0


def _dense_operands(fmt, a, bt):
    """Checks of the dense entry points, before launch: float16 (f16) or int8 (i8), one GPU,
    contiguous, A ``[M, K]`` and Bt ``[N, K]``.  Returns the format code and M, N, K."""
    import torch

    code = _dense_format(fmt)
    name, want = ("i8", torch.int8) if code == ODH_DT_I8 else ("f16", torch.float16)
    _same_gpu_2d("dense", "operands", want, f"{name} operands are {want}", a, bt)
    m, k = a.shape
    n = bt.shape[0]
    if bt.shape[1] != k or not dense_shape_ok(code, m, n, k):
        raise ValueError(f"M,N must be multiples of 256 and K of {64 if code == ODH_DT_I8 else 32}; "
                         f"got A{tuple(a.shape)} Bt{tuple(bt.shape)}")
    return code, m, n, k


def dense_fill(fmt, a, bt) -> None:
    """The probe operands for ``fmt`` written into the given tensors: exact halves (``"f16"``), or
    int8 times ``ODH_DT_I8_MUL_A`` / ``ODH_DT_I8_MUL_B`` (``"i8"``)."""
    code, m, n, k = _dense_operands(fmt, a, bt)
    _check(load_library().odh_dense_fill(code, a.data_ptr(), bt.data_ptr(), m, n, k, _stream_ptr(a.device)))


def dense_gemm(fmt, a, bt, out=None):
    """``C[M,N] = A[M,K] · Bt[N,K]ᵀ`` on the FP16 (``v_mfma_f32_32x32x16_f16``, fp32 out) or INT8
    (``v_mfma_i32_32x32x32_i8``, int32 out) matrix cores."""
    import torch

    code, m, n, k = _dense_operands(fmt, a, bt)
    want = torch.int32 if code == ODH_DT_I8 else torch.float32
    if out is None:
        out = torch.empty((m, n), dtype=want, device=a.device)
    elif tuple(out.shape) != (m, n) or out.dtype != want or not out.is_contiguous() or out.device != a.device:
        raise ValueError(f"out must be a contiguous {want} [M,N] tensor on the operands' GPU")
    _check(load_library().odh_dense_gemm(code, a.data_ptr(), bt.data_ptr(), out.data_ptr(), m, n, k,
                                         _stream_ptr(a.device)))
    return out


def dense_verify(fmt, a, bt) -> dict:
    """The fused check of the given operands against the closed form on a fresh counter block;
    the kernel's time is taken with events around its one launch.  The dict of :func:`mx_verify`
    (``tflops`` counts integer operations for ``"i8"``)."""
    code, m, n, k = _dense_operands(fmt, a, bt)

    def launch(tile_xcd, counters, stream):
        return load_library().odh_dense_probe_gemm_verify(code, a.data_ptr(), bt.data_ptr(), m, n, k, tile_xcd,
                                                          counters, stream)

    return _fused_check(a.device, m, n, k, launch)


def dense_probe(device: int, fmt, m: int = PROBE_SHAPE[0], n: int = PROBE_SHAPE[1], k: int = PROBE_SHAPE[2]) -> dict:
    """One FP16 / INT8 probe of a GPU: fill, then the GEMM with the check fused into its
    epilogue.  ``errors``, ``err_xcd``, ``xcd_blocks``, ``ms`` and ``tflops`` of the check kernel."""
    import torch

    code = _dense_format(fmt)
    if not dense_shape_ok(code, m, n, k):
        raise ValueError("dense probe shape must be tile aligned")
    dev = torch.device("cuda", device)
    dtype = torch.int8 if code == ODH_DT_I8 else torch.float16
    with torch.cuda.device(dev):
        a = torch.empty((m, k), dtype=dtype, device=dev)
        bt = torch.empty((n, k), dtype=dtype, device=dev)
        dense_fill(code, a, bt)
        return dense_verify(code, a, bt)


def _fp_format(fmt) -> int:
    code = FP_FORMATS.get(fmt, fmt) if isinstance(fmt, str) else fmt
    if code not in FP_FORMATS.values():
        raise ValueError(f"fp format must be one of {sorted(FP_FORMATS)}; got {fmt!r}")
    return code


def fp_shape_ok(fmt, m: int, n: int, k: int) -> bool:
    """256-row and 256-column multiples, and K in stages of 64 bytes per row: 16 floats or 8 doubles."""
    bk = 64 // _fp_format(fmt)
    return m > 0 and n > 0 and k > 0 and m % 256 == 0 and n % 256 == 0 and k % bk == 0


def fp_k_exact(fmt, k: int) -> bool:
    """Whether every partial sum of the fp probe operands, at most ``6 K MUL_A MUL_B``, is an exact
    integer of the accumulator type: below 2^24 (f32, K <= 2728) or 2^53 (f64, K <= 1365)."""
    if _fp_format(fmt) == ODH_FP_F64:
        return 6 * k * ODH_FP_F64_MUL_A * ODH_FP_F64_MUL_B < 2 ** 53
    return 6 * k * ODH_FP_F32_MUL_A * ODH_FP_F32_MUL_B < 2 ** 24


def fp_tiles(fmt, m: int, n: int) -> int:
    """Workgroups the fp kernels launch: 256×256 output tiles for f32, 256×128 for f64."""
    return load_library().odh_fp_tiles(_fp_format(fmt), m, n)


def _fp_operands(fmt, a, bt, probe: bool = False):
    """Checks of the fp entry points, before launch: float32 (f32) or float64 (f64), one GPU,
    contiguous, 16-byte aligned, A ``[M, K]`` and Bt ``[N, K]``; ``probe``: a K at which the probe
    operands are exact.
    Returns the format code and M, N, K."""
    import torch

    code = _fp_format(fmt)
    name, want = ("f64", torch.float64) if code == ODH_FP_F64 else ("f32", torch.float32)
    _same_gpu_2d("fp", "operands", want, f"{name} operands are {want}", a, bt)
    m, k = a.shape
    n = bt.shape[0]
    if bt.shape[1] != k or not fp_shape_ok(code, m, n, k):
        raise ValueError(f"M,N must be multiples of 256 and K of {64 // code}; "
                         f"got A{tuple(a.shape)} Bt{tuple(bt.shape)}")
    if a.data_ptr() % 16 or bt.data_ptr() % 16:
        raise ValueError("operands must be 16-byte aligned")
    if probe and not fp_k_exact(code, k):
        raise ValueError(f"the {name} probe operands are not exact at K = {k}")
    return code, m, n, k


def fp_fill(fmt, a, bt) -> None:
    """The probe operands for ``fmt`` written into the given tensors: the bf16 probe's families
    times ``ODH_FP_F32_MUL_A`` / ``_B`` as floats (``"f32"``) or ``ODH_FP_F64_MUL_A`` / ``_B`` as
    doubles (``"f64"``)."""
    code, m, n, k = _fp_operands(fmt, a, bt, probe=True)
    _check(load_library().odh_fp_fill(code, a.data_ptr(), bt.data_ptr(), m, n, k, _stream_ptr(a.device)))


def fp_gemm(fmt, a, bt, out=None):
    """``C[M,N] = A[M,K] · Bt[N,K]ᵀ`` on the FP32 (``v_mfma_f32_32x32x2_f32``) or FP64
    (``v_mfma_f64_16x16x4_f64``) matrix cores, out in the operands' type."""
    import torch

    code, m, n, k = _fp_operands(fmt, a, bt)
    want = a.dtype
    if out is None:
        out = torch.empty((m, n), dtype=want, device=a.device)
    elif tuple(out.shape) != (m, n) or out.dtype != want or not out.is_contiguous() or out.device != a.device:
        raise ValueError(f"out must be a contiguous {want} [M,N] tensor on the operands' GPU")
    _check(load_library().odh_fp_gemm(code, a.data_ptr(), bt.data_ptr(), out.data_ptr(), m, n, k,
                                      _stream_ptr(a.device)))
    return out


def fp_verify(fmt, a, bt) -> dict:
    """The fused check of the given operands against the closed form on a fresh counter block;
    the kernel's time is taken with events around its one launch.  The dict of :func:`mx_verify`."""
    code, m, n, k = _fp_operands(fmt, a, bt, probe=True)

    def launch(tile_xcd, counters, stream):
        return load_library().odh_fp_probe_gemm_verify(code, a.data_ptr(), bt.data_ptr(), m, n, k, tile_xcd,
                                                       counters, stream)

    return _fused_check(a.device, m, n, k, launch, tiles=fp_tiles(code, m, n))


def fp_probe(device: int, fmt, m: int = PROBE_SHAPE[0], n: int = PROBE_SHAPE[1], k: int = PROBE_SHAPE[2]) -> dict:
    """One FP32 / FP64 probe of a GPU: fill, then the GEMM with the check fused into its
    epilogue.  ``errors``, ``err_xcd``, ``xcd_blocks``, ``ms`` and ``tflops`` of the check kernel."""
    import torch

    code = _fp_format(fmt)
    if not fp_shape_ok(code, m, n, k) or not fp_k_exact(code, k):
        raise ValueError("fp probe shape must be tile aligned, with a K at which the operands are exact")
    dev = torch.device("cuda", device)
    dtype = torch.float64 if code == ODH_FP_F64 else torch.float32
    with torch.cuda.device(dev):
        a = torch.empty((m, k), dtype=dtype, device=dev)
        bt = torch.empty((n, k), dtype=dtype, device=dev)
        fp_fill(code, a, bt)
        return fp_verify(code, a, bt)


def _sparse_format(fmt) -> int:
    code = SPARSE_FORMATS.get(fmt, fmt) if isinstance(fmt, str) else fmt
    if code not in SPARSE_FORMATS.values():
        raise ValueError(f"sparse format must be one of {sorted(SPARSE_FORMATS)}; got {fmt!r}")
    return code


def _sparse_stage(code: int) -> int:
    """Dense elements of a row per stage: 128 bytes of a Bt row."""
    return 64 if code in (ODH_SP_BF16, ODH_SP_F16) else 128


def _sparse_dtype(code: int):
    import torch

    return {ODH_SP_BF16: torch.bfloat16, ODH_SP_F16: torch.float16, ODH_SP_I8: torch.int8,
            ODH_SP_FP8: torch.float8_e4m3fn, ODH_SP_BF8: torch.float8_e5m2}[code]


def sparse_shape_ok(fmt, m: int, n: int, k: int) -> bool:
    """256² output tiles, and K (the dense one) in whole stages: 64 bf16 or f16 elements, 128 i8, fp8 or bf8."""
    bk = _sparse_stage(_sparse_format(fmt))
    return m > 0 and n > 0 and k > 0 and m % 256 == 0 and n % 256 == 0 and k % bk == 0


def sparse_zero_classes(k: int) -> int:
    """How many of the 210 ``(i mod 30, j mod 7)`` classes of the sparse probe operands expect 0 at
    this K (-1: K is no positive multiple of 64).  Host arithmetic only."""
    return load_library().odh_sparse_zero_classes(k)


def _raw_view(t):
    """An integer view of a tensor's elements (gather and scatter take every integer dtype)."""
    import torch

    if not t.dtype.is_floating_point:
        return t
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def sparse_compress(a, prune: bool = False):
    """A dense ``[M, K]`` tensor (CPU or GPU, K a multiple of 8) with at most two non-zeros in every
    group of four consecutive elements of a row, as ``(ac, meta)`` in the layout of :func:`sparse_gemm`:
    ``ac`` is ``[M, K/2]`` in ``a``'s dtype, elements ``2g`` and ``2g + 1`` the kept ones of group ``g``;
    ``meta`` is ``[M, K/8]`` uint8, group ``g`` the nibble at bits ``[4g, 4g + 4)`` of the row,
    ``p0 | p1 << 2`` with ``p0 < p1`` the kept positions.  A group with more than two non-zeros raises
    ``ValueError`` (naming row and group) unless ``prune``, which keeps the two largest magnitudes
    of each group, ties to the lower position.  A group with fewer than two non-zeros keeps them
    and the lowest other positions, so every nibble is valid."""
    import torch

    if a.dim() != 2 or a.shape[1] % 8:
        raise ValueError(f"a must be [M, K] with K a multiple of 8; got {tuple(a.shape)}")
    m, k = a.shape
    val = a.double() if a.dtype.is_floating_point else a.long()
    groups = val.reshape(m, k // 4, 4)
    if prune:
        key = groups.abs()
    else:
        key = (groups != 0).to(torch.int64)
        over = (key.sum(-1) > 2).nonzero()
        if over.numel():
            r, g = over[0].tolist()
            raise ValueError(f"row {r}, group {g} (columns {4 * g} … {4 * g + 3}) has more than two non-zeros")
    # the two largest keys of a group, ties to the lower position, in ascending position
    order = torch.sort(key, dim=-1, descending=True, stable=True).indices[..., :2]
    pos = torch.sort(order, dim=-1).values
    ac = torch.gather(_raw_view(a.contiguous()).reshape(m, k // 4, 4), -1, pos).reshape(m, k // 2).view(a.dtype)
    nib = (pos[..., 0] | (pos[..., 1] << 2)).reshape(m, k // 8, 2)
    meta = (nib[..., 0] | (nib[..., 1] << 4)).to(torch.uint8)
    return ac.contiguous(), meta.contiguous()


def sparse_decompress(ac, meta):
    """The dense ``[M, K]`` tensor of a compressed ``ac`` ``[M, K/2]`` and its ``meta`` ``[M, K/8]``
    (nibbles with ``p0 < p1``): the inverse of :func:`sparse_compress`."""
    import torch

    if ac.dim() != 2 or meta.dim() != 2 or meta.dtype != torch.uint8 or ac.shape[0] != meta.shape[0] \
            or ac.shape[1] != 4 * meta.shape[1]:
        raise ValueError(f"ac must be [M, K/2] and meta [M, K/8] uint8; got {tuple(ac.shape)} {tuple(meta.shape)}")
    m, g = ac.shape[0], ac.shape[1] // 2
    nib = torch.stack((meta & 15, meta >> 4), dim=-1).reshape(m, g).long()
    pos = torch.stack((nib & 3, nib >> 2), dim=-1)
    raw = _raw_view(ac.contiguous())
    out = torch.zeros((m, g, 4), dtype=raw.dtype, device=ac.device)
    out.scatter_(-1, pos, raw.reshape(m, g, 2))
    return out.reshape(m, 4 * g).view(ac.dtype)


def _sparse_operands(fmt, ac, meta, bt, probe: bool = False):
    """Checks of the sparse entry points, before launch: ``ac`` ``[M, K/2]`` and ``bt`` ``[N, K]`` in the
    format's dtype (bfloat16, float16, int8, float8_e4m3fn, float8_e5m2), ``meta`` ``[M, K/8]`` uint8,
    one GPU, contiguous, aligned; ``probe``: a K at which no class of the probe operands expects 0.
    Returns the format code and M, N, K."""
    import torch

    code = _sparse_format(fmt)
    want = _sparse_dtype(code)
    name = next(n for n, c in SPARSE_FORMATS.items() if c == code)
    _same_gpu_2d("sparse", "operands", want, f"{name} operands are {want}", ac, bt)
    _same_gpu_2d("sparse", "operands and metadata", torch.uint8, "sparse metadata is uint8", meta)
    if meta.device != ac.device:
        raise ValueError("operands and metadata must live on the same GPU")
    m, n, k = ac.shape[0], bt.shape[0], bt.shape[1]
    if 2 * ac.shape[1] != k or tuple(meta.shape) != (m, k // 8) or not sparse_shape_ok(code, m, n, k):
        raise ValueError(f"M,N must be multiples of 256 and K of {_sparse_stage(code)}, Ac [M,K/2], meta [M,K/8]; "
                         f"got Ac{tuple(ac.shape)} meta{tuple(meta.shape)} Bt{tuple(bt.shape)}")
    if ac.data_ptr() % 16 or bt.data_ptr() % 16 or meta.data_ptr() % 4:
        raise ValueError("operands must be 16-byte aligned and metadata 4-byte aligned")
    if probe and sparse_zero_classes(k) != 0:
        raise ValueError(f"a class of the sparse probe operands expects 0 at K = {k}")
    return code, m, n, k


def _sparse_table(table, dev) -> None:
    import torch

    if (table.dtype != torch.int32 or tuple(table.shape) != SPARSE_TABLE or not table.is_contiguous()
            or table.device != dev):
        raise ValueError("table must be a contiguous int32 [30,7] tensor on the operands' GPU")


def sparse_fill(fmt, ac, meta, bt, table) -> None:
    """The sparse probe operands for ``fmt`` written into the given tensors: the bf16 probe's A pruned
    2:4 by a selector that uses all six position pairs, compressed, with its metadata; the dense Bt;
    and the 30 × 7 int32 table of expected sums (of the small integers: ``"i8"`` operands are
    those times ``ODH_DT_I8_MUL_A`` / ``ODH_DT_I8_MUL_B``, and the check scales the table)."""
    code, m, n, k = _sparse_operands(fmt, ac, meta, bt, probe=True)
    _sparse_table(table, ac.device)
    _check(load_library().odh_sparse_fill(code, ac.data_ptr(), meta.data_ptr(), bt.data_ptr(), table.data_ptr(),
                                          m, n, k, _stream_ptr(ac.device)))


def sparse_gemm(fmt, ac, meta, bt, out=None):
    """``C[M,N] = A[M,K] · Bt[N,K]ᵀ`` for a 2:4-sparse A given as :func:`sparse_compress` returns it, on
    the structured-sparsity matrix cores (``v_smfmac_*``): fp32 out, int32 for ``"i8"``."""
    import torch

    code, m, n, k = _sparse_operands(fmt, ac, meta, bt)
    want = torch.int32 if code == ODH_SP_I8 else torch.float32
    if out is None:
        out = torch.empty((m, n), dtype=want, device=ac.device)
    elif tuple(out.shape) != (m, n) or out.dtype != want or not out.is_contiguous() or out.device != ac.device:
        raise ValueError(f"out must be a contiguous {want} [M,N] tensor on the operands' GPU")
    _check(load_library().odh_sparse_gemm(code, ac.data_ptr(), meta.data_ptr(), bt.data_ptr(), out.data_ptr(),
                                          m, n, k, _stream_ptr(ac.device)))
    return out


def sparse_verify(fmt, ac, meta, bt, table) -> dict:
    """The fused check of the given operands against ``table`` on a fresh counter block; the kernel's
    time is taken with events around its one launch.  The dict of :func:`mx_verify` (``tflops`` counts
    the dense-equivalent ``2·M·N·K``)."""
    code, m, n, k = _sparse_operands(fmt, ac, meta, bt, probe=True)
    _sparse_table(table, ac.device)

    def launch(tile_xcd, counters, stream):
        return load_library().odh_sparse_probe_gemm_verify(code, ac.data_ptr(), meta.data_ptr(), bt.data_ptr(),
                                                           table.data_ptr(), m, n, k, tile_xcd, counters, stream)

    return _fused_check(ac.device, m, n, k, launch)


def sparse_probe(device: int, fmt, m: int = PROBE_SHAPE[0], n: int = PROBE_SHAPE[1], k: int = PROBE_SHAPE[2]) -> dict:
    """One structured-sparsity probe of a GPU: fill, then the GEMM with the check fused into its
    epilogue.  ``errors``, ``err_xcd``, ``xcd_blocks``, ``ms`` and ``tflops`` of the check kernel."""
    import torch

    code = _sparse_format(fmt)
    if not sparse_shape_ok(code, m, n, k) or sparse_zero_classes(k) != 0:
        raise ValueError("sparse probe shape must be tile aligned, with a K at which no class expects 0")
    dev = torch.device("cuda", device)
    dtype = _sparse_dtype(code)
    with torch.cuda.device(dev):
        ac = torch.empty((m, k // 2), dtype=dtype, device=dev)
        meta = torch.empty((m, k // 8), dtype=torch.uint8, device=dev)
        bt = torch.empty((n, k), dtype=dtype, device=dev)
        table = torch.empty(SPARSE_TABLE, dtype=torch.int32, device=dev)
        sparse_fill(code, ac, meta, bt, table)
        return sparse_verify(code, ac, meta, bt, table)


def _cvt_format(fmt) -> int:
    code = CVT_FORMATS.get(fmt, fmt) if isinstance(fmt, str) else fmt
    if code not in CVT_FORMATS.values():
        raise ValueError(f"converter format must be one of {sorted(CVT_FORMATS)}; got {fmt!r}")
    return code


def cvt_family_size(fmt) -> int:
    """Cases of the family the fused converter check walks.  Host arithmetic only."""
    return load_library().odh_cvt_family_size(_cvt_format(fmt))


def cvt_family(fmt, first: int = 0, n: Optional[int] = None) -> dict:
    """Cases ``[first, first + n)`` of the family of ``fmt`` (all of it by default), from the library's own
    generator, as CPU tensors: ``x`` float32 inputs, ``scale`` the E8M0 byte of each (127 for bf16), ``sel``
    the destination select, ``expect`` the code with its sign (int32; 16 bits for bf16).  32 consecutive
    cases from a multiple of 32 on share their scale.  Host arithmetic only."""
    import torch

    code = _cvt_format(fmt)
    size = cvt_family_size(code)
    if n is None:
        n = size - first
    if first < 0 or n < 0 or first + n > size:
        raise ValueError(f"cases [{first}, {first + n}) are not in the family of {size}")
    x, sc, ex = (torch.empty((n,), dtype=torch.int32) for _ in range(3))
    if load_library().odh_cvt_family(code, first, n, x.data_ptr(), sc.data_ptr(), ex.data_ptr()) != 0:
        raise ValueError("odh_cvt_family refused its arguments")
    return {"x": x.view(torch.float32), "scale": (sc & 255).to(torch.uint8), "sel": (sc >> 8).to(torch.uint8),
            "expect": ex}


def _cvt_rows(fmt, x, scales=None):
    """Checks of the converter entry points, before launch: ``x`` float32 ``[rows, K]`` on a GPU, contiguous,
    16-byte aligned, K a multiple of 32; ``scales`` (if given) uint8 ``[rows, K/32]`` on the same GPU.
    Returns the format code, rows, K."""
    import torch

    code = _cvt_format(fmt)
    if x.dtype != torch.float32 or (scales is not None and scales.dtype != torch.uint8):
        raise ValueError("the converters take float32 values and uint8 scales")
    if x.dim() != 2 or not x.is_cuda or not x.is_contiguous():
        raise ValueError("x must be a contiguous 2-D tensor on a GPU")
    rows, k = x.shape
    if rows < 1 or k < 32 or k % 32:
        raise ValueError(f"x must be [rows >= 1, K a positive multiple of 32]; got {tuple(x.shape)}")
    if x.data_ptr() % 16:
        raise ValueError("x must be 16-byte aligned")
    if scales is not None:
        if code == ODH_CVT_BF16:
            raise ValueError("bf16 takes no scales")
        if not scales.is_cuda or scales.device != x.device or not scales.is_contiguous() \
                or tuple(scales.shape) != (rows, k // 32):
            raise ValueError(f"scales must be a contiguous [{rows},{k // 32}] tensor on x's GPU")
    return code, rows, k


def _cvt_out(code: int, x, rows: int, k: int):
    import torch

    if code == ODH_CVT_BF16:
        return torch.empty((rows, k), dtype=torch.bfloat16, device=x.device)
    return torch.empty((rows, mx_row_bytes(code, k)), dtype=torch.uint8, device=x.device)


def cvt_encode(fmt, x, scales=None):
    """The hardware converter as it is: ``x`` ``[rows, K]`` float32 divided by the caller's E8M0 ``scales``
    ``[rows, K/32]`` and rounded to nearest even, to uint8 codes in the layout :func:`mx_gemm` reads
    (``[rows, mx_row_bytes]``); what lies beyond the largest finite value becomes what the instruction makes
    of it.  ``"bf16"`` takes no scales and returns a bfloat16 ``[rows, K]`` tensor."""
    code, rows, k = _cvt_rows(fmt, x, scales)
    if code != ODH_CVT_BF16 and scales is None:
        raise ValueError("the scaled formats need scales")
    out = _cvt_out(code, x, rows, k)
    _check(load_library().odh_cvt_encode(code, x.data_ptr(), scales.data_ptr() if scales is not None else None,
                                         out.data_ptr(), rows, k, _stream_ptr(x.device)))
    return out


def mx_quantize(fmt, x):
    """OCP MX quantisation on the GPU: ``x`` ``[rows, K]`` float32 to ``(codes, scales)`` as :func:`mx_gemm`
    takes them.  The scale of a block of 32 is ``2^(floor(log2(amax)) - emax)`` of the element format, clamped
    to E8M0 (2^0 for an all-zero block); the elements go through the hardware converter with that scale and
    saturate at the largest finite code.  ``"bf16"`` is the plain conversion: ``(bfloat16 tensor, None)``.

    Any float32 may come in.  For the scaled formats, per block of 32:

    * amax is the largest ``|x|`` over the elements that are not NaN; ±Inf counts as FLT_MAX.
    * If no such element exists, or all are zero, the scale byte is 127.
    * Otherwise the byte is ``clamp(floor(log2 amax) - emax + 127, 0, 254)``; with an Inf in the block that
      is ``254 - emax``.  Byte 255 (the E8M0 NaN) is never emitted.
    * Finite elements are clamped in float32 to ±(largest finite value · scale) and then converted.
    * ±Inf becomes the largest finite code with its sign, in every format, like finite overflow.
    * NaN becomes the format's NaN, fp8 0xFF and bf8 0xFE, whatever its sign.  fp4, fp6 and bf6 have no NaN:
      there a NaN becomes the largest code with the input's sign, so these three formats cannot carry a NaN.

    bf16: Inf stays Inf and NaN stays NaN, quieted."""
    import torch

    code, rows, k = _cvt_rows(fmt, x)
    out = _cvt_out(code, x, rows, k)
    scales = None if code == ODH_CVT_BF16 else torch.empty((rows, k // 32), dtype=torch.uint8, device=x.device)
    _check(load_library().odh_cvt_quantize(code, x.data_ptr(), out.data_ptr(),
                                           scales.data_ptr() if scales is not None else None, rows, k,
                                           _stream_ptr(x.device)))
    return out, scales


def cvt_fill(fmt, table) -> None:
    """The scale table of the fused converter check (``ODH_CVT_TABLE`` uint8) written into ``table``."""
    import torch

    code = _cvt_format(fmt)
    if table.dtype != torch.uint8 or tuple(table.shape) != (ODH_CVT_TABLE,) or not table.is_cuda \
            or not table.is_contiguous():
        raise ValueError(f"table must be a contiguous uint8 [{ODH_CVT_TABLE}] tensor on a GPU")
    _check(load_library().odh_cvt_fill(code, table.data_ptr(), _stream_ptr(table.device)))


def cvt_verify(fmt, table) -> dict:
    """The fused check against ``table`` on a fresh counter block: every wave of ``ODH_CVT_BLOCKS`` workgroups
    converts the whole family.  ``errors``, ``err_xcd``, ``xcd_blocks``, ``ms``, and ``gcvt_s``, family cases
    per nanosecond over all waves."""
    import torch

    code = _cvt_format(fmt)
    if table.dtype != torch.uint8 or tuple(table.shape) != (ODH_CVT_TABLE,) or not table.is_cuda \
            or not table.is_contiguous():
        raise ValueError(f"table must be a contiguous uint8 [{ODH_CVT_TABLE}] tensor on a GPU")
    dev = table.device
    with torch.cuda.device(dev):
        counters = torch.zeros((ODH_NCOUNT,), dtype=torch.int32, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _check(load_library().odh_cvt_probe_verify(code, table.data_ptr(), counters.data_ptr(), _stream_ptr(dev)))
        e1.record()
        e1.synchronize()
        h = counters.cpu().tolist()
    ms = e0.elapsed_time(e1)
    return {
        "errors": h[ODH_SLOT_GEMM_ERR] & 0xFFFFFFFF,
        "err_xcd": [x & 0xFFFFFFFF for x in h[ODH_SLOT_ERR_XCD:ODH_SLOT_ERR_XCD + ODH_N_XCD]],
        "xcd_blocks": h[ODH_SLOT_XCD_BLOCKS:ODH_SLOT_XCD_BLOCKS + ODH_N_XCD],
        "ms": ms, "gcvt_s": cvt_family_size(code) * ODH_CVT_BLOCKS * 4 / (ms * 1e6) if ms > 0 else 0.0,
    }


def cvt_probe(device: int, fmt) -> dict:
    """One converter probe of a GPU: the scale table, then the fused check.  The dict of :func:`cvt_verify`."""
    import torch

    code = _cvt_format(fmt)
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        table = torch.empty((ODH_CVT_TABLE,), dtype=torch.uint8, device=dev)
        cvt_fill(code, table)
        return cvt_verify(code, table)


def _lds_check(check) -> int:
    code = LDS_CHECKS.get(check, check) if isinstance(check, str) else check
    if isinstance(code, bool) or code not in LDS_CHECKS.values():
        raise ValueError(f"LDS check must be one of {sorted(LDS_CHECKS)}; got {check!r}")
    return code


def lds_cases(check) -> int:
    """Elements one launch of the fused check compares.  Host arithmetic only."""
    return load_library().odh_lds_cases(_lds_check(check))


def lds_fault_count(check, table_byte: int) -> int:
    """Mismatches the fused check counts when byte ``table_byte`` of its key table is wrong (for ``tr4`` and
    ``tr6``: wrong in another way in its low nibble than in its high one).  Host arithmetic only."""
    code = _lds_check(check)
    if not 0 <= table_byte < ODH_LDS_TABLE:
        raise ValueError(f"table_byte must be in [0, {ODH_LDS_TABLE}); got {table_byte}")
    return load_library().odh_lds_fault_count(code, table_byte)


def _lds_table(table) -> None:
    import torch

    if table.dtype != torch.uint8 or tuple(table.shape) != (ODH_LDS_TABLE,) or not table.is_cuda \
            or not table.is_contiguous() or table.data_ptr() % 4:
        raise ValueError(f"table must be a contiguous, 4-byte aligned uint8 [{ODH_LDS_TABLE}] tensor on a GPU")


def lds_fill(check, table) -> None:
    """The key table of a fused LDS check (``ODH_LDS_TABLE`` uint8) written into ``table``."""
    code = _lds_check(check)
    _lds_table(table)
    _check(load_library().odh_lds_fill(code, table.data_ptr(), _stream_ptr(table.device)))


def lds_verify(check, table) -> dict:
    """The fused check against ``table`` on a fresh counter block: ``ODH_LDS_BLOCKS`` workgroups, one wave per
    SIMD.  ``ok`` (no mismatch and every workgroup ran), ``errors``, ``blocks``, ``err_xcd``, ``xcd_blocks``,
    ``ms``, and ``cus``: the distinct CUs the workgroups reported, which is recorded and no part of ``ok``."""
    import torch

    code = _lds_check(check)
    _lds_table(table)
    dev = table.device
    with torch.cuda.device(dev):
        counters = torch.zeros((ODH_NCOUNT + ODH_LDS_CU_WORDS,), dtype=torch.int32, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _check(load_library().odh_lds_probe_verify(code, table.data_ptr(), counters.data_ptr(), _stream_ptr(dev)))
        e1.record()
        e1.synchronize()
        h = counters.cpu().tolist()
    errors = h[ODH_SLOT_GEMM_ERR] & 0xFFFFFFFF
    xcd_blocks = h[ODH_SLOT_XCD_BLOCKS:ODH_SLOT_XCD_BLOCKS + ODH_N_XCD]
    return {
        "ok": errors == 0 and sum(xcd_blocks) == ODH_LDS_BLOCKS, "errors": errors, "blocks": sum(xcd_blocks),
        "err_xcd": [x & 0xFFFFFFFF for x in h[ODH_SLOT_ERR_XCD:ODH_SLOT_ERR_XCD + ODH_N_XCD]],
        "xcd_blocks": xcd_blocks, "ms": e0.elapsed_time(e1),
        "cus": sum(bin(w & 0xFFFFFFFF).count("1") for w in h[ODH_NCOUNT:]),
    }


def lds_probe(device: int, check) -> dict:
    """One LDS probe of a GPU: the key table, then the fused check.  The dict of :func:`lds_verify`."""
    import torch

    code = _lds_check(check)
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        table = torch.empty((ODH_LDS_TABLE,), dtype=torch.uint8, device=dev)
        lds_fill(code, table)
        return lds_verify(code, table)


def lds_tr_read(check, image, lane_addr, raw: bool = False):
    """One wave, one transposing LDS read (``tr16``, ``tr8``, ``tr4``, ``tr6``): ``image`` (uint8 on a GPU, a
    multiple of 4 and at most 65536 bytes) is copied to LDS, lane ``l`` reads at byte address ``lane_addr[l]``
    (64 of them).  Returns uint8 ``[64, 8]`` (``tr6``: ``[64, 12]``), a lane's result bytes in register order.
    Addresses out of range or misaligned for the instruction raise ``ValueError`` before anything is launched;
    ``raw`` leaves the alignment unchecked (what the instruction then returns was measured with it)."""
    import torch

    code = _lds_check(check)
    if not ODH_LDS_TR16 <= code <= ODH_LDS_TR6:
        raise ValueError("lds_tr_read takes one of the transposing reads: tr16, tr8, tr4, tr6")
    if image.dtype != torch.uint8 or image.dim() != 1 or not image.is_cuda or not image.is_contiguous() \
            or not 0 < image.numel() <= 65536 or image.numel() % 4 or image.data_ptr() % 4:
        raise ValueError("image must be a contiguous, 4-byte aligned uint8 vector of at most 65536 bytes on a GPU")
    addr = [int(a) for a in lane_addr]
    width = 12 if code == ODH_LDS_TR6 else 8
    align = 16 if code == ODH_LDS_TR6 else 8
    if len(addr) != 64:
        raise ValueError("lane_addr holds one address per lane: 64")
    for a in addr:
        if a < 0 or a + width > image.numel() or (not raw and a % align):
            raise ValueError(f"lane address {a} is out of range or not {align}-byte aligned")
    out = torch.zeros((64, width), dtype=torch.uint8, device=image.device)
    host = (ctypes.c_uint32 * 64)(*addr)
    _check(load_library().odh_lds_tr_read(code + (ODH_LDS_TR_RAW if raw else 0), image.data_ptr(), image.numel(),
                                          ctypes.cast(host, ctypes.c_void_p), out.data_ptr(),
                                          _stream_ptr(image.device)))
    return out


def lds_xlane(op, arg: int, values):
    """One wave, one lane exchange of ``values`` (int32 or uint32-as-int32 ``[64]`` on a GPU; the two swaps:
    ``[128]``, lane ``l``'s second register at ``64 + l``).  ``op`` is a name of :data:`LDS_XLANE_OPS` or its
    number, ``arg`` its selector (``0 <= arg < LDS_XLANE_ARGS[op]``).  Returns the values after the exchange."""
    import torch

    name = op if isinstance(op, str) else {v: k for k, v in LDS_XLANE_OPS.items()}.get(op)
    if name not in LDS_XLANE_OPS:
        raise ValueError(f"op must be one of {sorted(LDS_XLANE_OPS)}; got {op!r}")
    if not 0 <= arg < LDS_XLANE_ARGS[name]:
        raise ValueError(f"{name} takes selectors 0 .. {LDS_XLANE_ARGS[name] - 1}; got {arg}")
    n = 128 if name.endswith("_swap") else 64
    if values.dtype != torch.int32 or tuple(values.shape) != (n,) or not values.is_cuda or not values.is_contiguous():
        raise ValueError(f"values must be a contiguous int32 [{n}] tensor on a GPU")
    out = torch.empty_like(values)
    _check(load_library().odh_lds_xlane(LDS_XLANE_OPS[name], arg, values.data_ptr(), out.data_ptr(),
                                        _stream_ptr(values.device)))
    return out


def transpose_codes(fmt, x):
    """The transpose of a tensor of packed codes, on the GPU with the transposing LDS reads
    (``ds_read_b64_tr_b16`` / ``_b8`` / ``_b4``, ``ds_read_b96_tr_b6``).  ``fmt``: ``bf16`` or ``f16`` (``x``
    ``[R, C]`` of that dtype), or ``fp8``, ``bf8``, ``fp4``, ``fp6``, ``bf6``: ``x`` uint8 ``[R, row bytes]`` in the
    layout :func:`mx_gemm` reads (a byte per element, two nibbles per byte with the even index low, or element
    ``k`` in bits ``[6k, 6k + 6)`` of the row), the logical column count following from the row bytes.  Returns
    the ``[C, R]`` codes in the same packing, bit for bit.  R and C are multiples of 128, ``x`` is contiguous and
    16-byte aligned; anything else raises ``ValueError`` before launch."""
    import torch

    if fmt not in TRANSPOSE_FORMATS:
        raise ValueError(f"format must be one of {sorted(TRANSPOSE_FORMATS)}; got {fmt!r}")
    code, bits = TRANSPOSE_FORMATS[fmt]
    want = {"bf16": torch.bfloat16, "f16": torch.float16}.get(fmt, torch.uint8)
    if x.dtype != want:
        raise ValueError(f"{fmt} codes are {want} tensors; got {x.dtype}")
    if x.dim() != 2 or not x.is_cuda or not x.is_contiguous():
        raise ValueError("x must be a contiguous 2-D tensor on a GPU")
    rows, row_bytes = x.shape[0], x.shape[1] * x.element_size()
    if row_bytes * 8 % bits:
        raise ValueError(f"a row of {row_bytes} bytes is no whole number of {bits}-bit elements")
    cols = row_bytes * 8 // bits
    if rows < 128 or cols < 128 or rows % 128 or cols % 128:
        raise ValueError(f"rows and columns must be positive multiples of 128; got {rows} x {cols}")
    if x.data_ptr() % 16:
        raise ValueError("x must be 16-byte aligned")
    out = torch.empty((cols, rows * bits // 8 // x.element_size()), dtype=x.dtype, device=x.device)
    _check(load_library().odh_transpose_codes(code, x.data_ptr(), out.data_ptr(), rows, cols, _stream_ptr(x.device)))
    return out


def mx_transpose(fmt, b, sb):
    """``(bt, sbt)`` as :func:`mx_gemm` takes them, from B held as ``[K, N]``: ``b`` the packed codes ``[K, row
    bytes of N elements]`` and ``sb`` its E8M0 scales ``[K/32, N]`` (one per 32 elements along K).  Both go
    through :func:`transpose_codes`, the scales as bytes; where K/32 is no multiple of 128 the scale rows are
    padded with zeros up to one and the padding is cut off the result."""
    import torch

    code = _mx_format(fmt)
    name = {v: k for k, v in MX_ALL_FORMATS.items()}[code]
    bt = transpose_codes(name, b)
    n, k = bt.shape[0], b.shape[0]
    if sb.dtype != torch.uint8 or sb.dim() != 2 or tuple(sb.shape) != (k // 32, n) or sb.device != b.device:
        raise ValueError(f"scales must be a uint8 [{k // 32},{n}] tensor on b's GPU")
    pad = -(k // 32) % 128
    if pad or not sb.is_contiguous() or sb.data_ptr() % 16:
        sb = torch.cat([sb, torch.zeros((pad, n), dtype=torch.uint8, device=sb.device)])
    sbt = transpose_codes("fp8", sb)
    return bt, sbt[:, :k // 32].contiguous() if pad else sbt


def _m16_format(fmt) -> int:
    code = M16_FORMATS.get(fmt, fmt) if isinstance(fmt, str) else fmt
    if code not in M16_FORMATS.values():
        raise ValueError(f"16x16 format must be one of {sorted(M16_FORMATS)}; got {fmt!r}")
    return code


# by format code: elements of one instruction (= of one stage), the operands' torch dtype by name, elements
# per operand byte or bytes per element as (numerator, denominator) of K for the row bytes, and the output dtype
_M16_LAYOUT = {
    ODH_M16_BF16: (32, "bfloat16", 1, 1, "float32"),
    ODH_M16_F16: (32, "float16", 1, 1, "float32"),
    ODH_M16_I8: (64, "int8", 1, 1, "int32"),
    ODH_M16_FP8: (128, "uint8", 1, 1, "float32"),
    ODH_M16_FP4: (128, "uint8", 1, 2, "float32"),
}


def m16_scaled(fmt) -> bool:
    """Whether the format takes E8M0 block scales (fp8, fp4)."""
    return _m16_format(fmt) in (ODH_M16_FP8, ODH_M16_FP4)


def m16_stage(fmt) -> int:
    """Elements of one instruction, which is one stage of the kernel: 32 (bf16, f16), 64 (i8), 128 (fp8, fp4)."""
    return _M16_LAYOUT[_m16_format(fmt)][0]


def m16_shape_ok(fmt, m: int, n: int, k: int) -> bool:
    """256² output tiles, and K in whole instructions of the format."""
    bk = m16_stage(fmt)
    return m > 0 and n > 0 and k > 0 and m % 256 == 0 and n % 256 == 0 and k % bk == 0


def _m16_operands(fmt, a, bt, sa, sbt):
    """Checks of the 16×16 entry points, before launch: the format's dtype, one GPU, contiguous, the public layout
    (A ``[M, row]``, Bt ``[N, row]``; fp8 and fp4 uint8 codes with uint8 scales ``[rows, K/32]``, the others no
    scales at all).  Returns the format code, M, N, K."""
    import torch

    code = _m16_format(fmt)
    stage, dtype, num, den, _ = _M16_LAYOUT[code]
    want = getattr(torch, dtype)
    name = next(k for k, v in M16_FORMATS.items() if v == code)
    if code in (ODH_M16_FP8, ODH_M16_FP4):
        if sa is None or sbt is None:
            raise ValueError(f"{name} operands come with their E8M0 scales")
        _same_gpu_2d("16x16", "operands and scales", want, f"{name} operands and scales are uint8 codes", a, bt, sa,
                     sbt)
    else:
        if sa is not None or sbt is not None:
            raise ValueError(f"{name} operands take no scales")
        _same_gpu_2d("16x16", "operands", want, f"{name} operands are {want}", a, bt)
    m, n, k = a.shape[0], bt.shape[0], a.shape[1] * den // num
    if bt.shape[1] != a.shape[1] or not m16_shape_ok(code, m, n, k):
        raise ValueError(f"M,N must be multiples of 256 and K of {stage}; got A{tuple(a.shape)} Bt{tuple(bt.shape)}")
    if sa is not None and (tuple(sa.shape) != (m, k // 32) or tuple(sbt.shape) != (n, k // 32)):
        raise ValueError(f"scales must be [{m},{k // 32}] and [{n},{k // 32}]; "
                         f"got {tuple(sa.shape)} {tuple(sbt.shape)}")
    return code, m, n, k


def _ptr(t):
    return t.data_ptr() if t is not None else None


def m16_gemm(fmt, a, bt, sa=None, sbt=None, out=None):
    """``C[M,N] = A · Btᵀ`` on the 16×16 shapes of the matrix-core instructions (``v_mfma_f32_16x16x32_bf16`` /
    ``_f16``, ``v_mfma_i32_16x16x64_i8``; fp8 and fp4: ``(A ∘ sA) · (Bt ∘ sBt)ᵀ`` on
    ``v_mfma_scale_f32_16x16x128_f8f6f4``): fp32 out, int32 for i8."""
    import torch

    code, m, n, k = _m16_operands(fmt, a, bt, sa, sbt)
    want = getattr(torch, _M16_LAYOUT[code][4])
    if out is None:
        out = torch.empty((m, n), dtype=want, device=a.device)
    elif tuple(out.shape) != (m, n) or out.dtype != want or not out.is_contiguous() or out.device != a.device:
        raise ValueError(f"out must be a contiguous {want} [M,N] tensor on the operands' GPU")
    _check(load_library().odh_m16_gemm(code, a.data_ptr(), bt.data_ptr(), _ptr(sa), _ptr(sbt), out.data_ptr(), m, n, k,
                                       _stream_ptr(a.device)))
    return out


def m16_verify(fmt, a, bt, sa=None, sbt=None, table=None) -> dict:
    """The fused check of the given operands (:func:`gemm_bf16`'s probe fill, :func:`dense_fill`'s or
    :func:`mx_fill`'s with its ``table``) on a fresh counter block; the dict of :func:`mx_verify`."""
    import torch

    code, m, n, k = _m16_operands(fmt, a, bt, sa, sbt)
    if (table is not None) != (sa is not None):
        raise ValueError("the table of expected values goes with the scaled formats, and only with them")
    if table is not None and (table.dtype != torch.float32 or tuple(table.shape) != MX_TABLE
                              or not table.is_contiguous() or table.device != a.device):
        raise ValueError("table must be a contiguous fp32 [15,21] tensor on the operands' GPU")

    def launch(tile_xcd, counters, stream):
        return load_library().odh_m16_probe_gemm_verify(code, a.data_ptr(), bt.data_ptr(), _ptr(sa), _ptr(sbt),
                                                        _ptr(table), m, n, k, tile_xcd, counters, stream)

    return _fused_check(a.device, m, n, k, launch)


def m16_fill(fmt, m: int, n: int, k: int, device):
    """Fresh tensors with the probe operands of a 16×16 format, by the fill of its layout: ``(a, bt, sa, sbt,
    table)``, the last three ``None`` for bf16, f16 and i8."""
    import torch

    code = _m16_format(fmt)
    if not m16_shape_ok(code, m, n, k):
        raise ValueError("16x16 probe shape must be tile aligned")
    dev = torch.device(device)
    _, dtype, num, den, _ = _M16_LAYOUT[code]
    with torch.cuda.device(dev):
        a = torch.empty((m, k * num // den), dtype=getattr(torch, dtype), device=dev)
        bt = torch.empty((n, k * num // den), dtype=getattr(torch, dtype), device=dev)
        if code in (ODH_M16_FP8, ODH_M16_FP4):
            sa = torch.empty((m, k // 32), dtype=torch.uint8, device=dev)
            sbt = torch.empty((n, k // 32), dtype=torch.uint8, device=dev)
            table = torch.empty(MX_TABLE, dtype=torch.float32, device=dev)
            mx_fill(ODH_MX_FP8 if code == ODH_M16_FP8 else ODH_MX_FP4, a, bt, sa, sbt, table)
            return a, bt, sa, sbt, table
        if code == ODH_M16_BF16:
            if not gemm_shape_ok(m, n, k):
                raise ValueError("bf16 probe shape must be tile aligned")
            _check(load_library().odh_probe_fill(a.data_ptr(), bt.data_ptr(), m, n, k, _stream_ptr(dev)))
        else:
            dense_fill(ODH_DT_F16 if code == ODH_M16_F16 else ODH_DT_I8, a, bt)
    return a, bt, None, None, None


def m16_probe(device: int, fmt, m: int = PROBE_SHAPE[0], n: int = PROBE_SHAPE[1], k: int = PROBE_SHAPE[2]) -> dict:
    """One 16×16 probe of a GPU: the fill of the format's layout, then the GEMM with the check fused into its
    epilogue.  ``errors``, ``err_xcd``, ``xcd_blocks``, ``ms`` and ``tflops`` of the check kernel."""
    import torch

    a, bt, sa, sbt, table = m16_fill(fmt, m, n, k, torch.device("cuda", device))
    return m16_verify(fmt, a, bt, sa, sbt, table)


def m16_one(fmt, a, b, sa=None, sb=None, opsel_a: int = 0, opsel_b: int = 0):
    """One wave, one 16×16 instruction on a zero accumulator.  ``a`` and ``b``: int32 ``[64, 8]``, lane l's
    registers in row l (a format uses the low 4 or 8); ``sa`` and ``sb``: int32 ``[64]`` scale VGPRs, for fp8 and
    fp4 only.  Returns int32 ``[64, 4]``: lane l's four result registers as bits."""
    import torch

    code = _m16_format(fmt)
    scaled = code in (ODH_M16_FP8, ODH_M16_FP4)
    ts = [a, b] + ([sa, sb] if scaled else [])
    if (sa is None or sb is None) if scaled else (sa is not None or sb is not None):
        raise ValueError("scale registers go with fp8 and fp4, and only with them")
    if any(t.dtype != torch.int32 for t in ts):
        raise TypeError("registers are int32 bit patterns")
    if tuple(a.shape) != (64, 8) or tuple(b.shape) != (64, 8) or (scaled and (tuple(sa.shape) != (64,)
                                                                            or tuple(sb.shape) != (64,))):
        raise ValueError("a and b are [64, 8], sa and sb [64]")
    if not all(t.is_cuda and t.device == a.device and t.is_contiguous() for t in ts):
        raise ValueError("registers must be contiguous tensors on one GPU")
    if opsel_a not in (0, 1, 2, 3) or opsel_b not in (0, 1, 2, 3):
        raise ValueError("opsel is 0, 1, 2 or 3")
    with torch.cuda.device(a.device):
        d = torch.empty((64, 4), dtype=torch.int32, device=a.device)
        _check(load_library().odh_m16_one(code, a.data_ptr(), b.data_ptr(), _ptr(sa), _ptr(sb), opsel_a, opsel_b,
                                          d.data_ptr(), _stream_ptr(a.device)))
    return d


class GpuProbe:
    """Resident start-up probe for one GPU (allocate + fill once, then ~1 ms per run)."""

    def __init__(self, device: int = 0, m: int = PROBE_SHAPE[0], n: int = PROBE_SHAPE[1], k: int = PROBE_SHAPE[2],
                 hbm_bytes: int = PROBE_HBM_BYTES,
                 hbm_nontemporal: bool = False, overlap: bool = True, graph=True):
        import torch

        if not gemm_shape_ok(m, n, k):
            raise ValueError("probe GEMM shape must be tile aligned")
        if probe_check_vacuous(k):
            raise ValueError("probe GEMM K must not be a multiple of 35: the expected product is all zero")
        if hbm_bytes < 16 or hbm_bytes % 16:
            raise ValueError("hbm_bytes must be a positive multiple of 16")
        self.device = torch.device("cuda", device)
        self.m, self.n, self.k = m, n, k
        self.hbm_bytes = hbm_bytes
        lib = load_library()
        with torch.cuda.device(self.device):
            self.a = torch.empty((m, k), dtype=torch.bfloat16, device=self.device)
            self.bt = torch.empty((n, k), dtype=torch.bfloat16, device=self.device)
            # the 256² kernel checks C in registers; other shapes store C and run the check kernel
            self.fused = fused_verify_ok(m, n, k)
            self.c = None if self.fused else torch.empty((m, n), dtype=torch.float32, device=self.device)
            self.tiles = lib.odh_gemm_tiles(m, n, k)
            self.tile_xcd = torch.full(((m // BM) * (n // BN),), -1, dtype=torch.int32, device=self.device)
            self.hbm = torch.empty((hbm_bytes // 4,), dtype=torch.int32, device=self.device)
            # the counter block (ODH_SLOT_*; the graph path adds its spans)
            self.counters = torch.zeros((ODH_NCOUNT,), dtype=torch.int32, device=self.device)
            self.host = torch.zeros((ODH_NCOUNT,), dtype=torch.int32).pin_memory()
            self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            self.streams = (torch.cuda.Stream(self.device), torch.cuda.Stream(self.device))
            _check(lib.odh_probe_fill(self.a.data_ptr(), self.bt.data_ptr(), m, n, k, _stream_ptr(self.device)))
            torch.cuda.current_stream(self.device).synchronize()
        self.hbm_nontemporal = hbm_nontemporal
        self.overlap = overlap
        # graph replay: fused + overlapped probes — one launch per run
        self.graph = graph
        self._graph = None
        self._graph_error: Optional[str] = None
        self.runs = 0
        self.seed = 0x9E3779B9
        # the pattern in ``hbm``: None (none yet, or a run that failed part-way), "graph" (the seed is in
        # ``seed_dev``: the replay advanced it on the device) or the seed itself (the eager launches)
        self._pattern = None
        # one probe in flight per GPU: runs share the counters, events and pinned host buffer
        # (two pods probing the same device — ranks sharing a GPU in a rehearsal — take turns)
        self._lock = threading.Lock()

    def run(self) -> dict:
        """One probe.  With ``overlap`` (default) the memory-bound HBM sweep and the
        MFMA-bound GEMM run concurrently on two streams of the probe: their waves co-reside
        on the CUs (the GEMM's 1 workgroup/CU leaves VGPRs and wave slots free), so the
        GEMM hides under the sweep instead of adding to it.  With ``graph`` (default) that
        whole sequence is one hipGraph launch."""
        with self._lock:
            if self.graph and self.fused and self.overlap:
                g = self._graph_handle()
                if g is not None:
                    return self._run_graph(g)
            return self._run()

    def _graph_handle(self):
        """Capture the probe graph once (``None`` if capture failed: the eager launches run
        instead and the error is kept in ``graph_error`` of every result)."""
        if self._graph is not None or self._graph_error is not None:
            return self._graph
        import torch

        lib = load_library()
        with torch.cuda.device(self.device):
            self.seed_dev = torch.full((1,), 0x1E3779B9, dtype=torch.int32, device=self.device)
            torch.cuda.current_stream(self.device).synchronize()
            h = ctypes.c_void_p()
            rc = lib.odh_probe_graph_create(self.a.data_ptr(), self.bt.data_ptr(), self.m, self.n, self.k,
                                            self.tile_xcd.data_ptr(), self.counters.data_ptr(), self.hbm.data_ptr(),
                                            self.hbm_bytes, self.seed_dev.data_ptr(), self.host.data_ptr(),
                                            int(self.graph == "serial"), ctypes.byref(h))
        if rc != 0:
            msg = lib.odh_error_string(rc)
            self._graph_error = f"HIP error {rc}: {msg.decode() if msg else '?'}"
            return None
        self._graph = h
        self._tick_khz = lib.odh_wall_clock_khz(self.device.index) or 100000
        return h

    def close(self) -> None:
        with self._lock:
            if self._graph is not None:
                self._pattern = self.pattern_seed  # the next capture starts a fresh ``seed_dev``
                load_library().odh_probe_graph_destroy(self._graph)
                self._graph = None

    @property
    def pattern_seed(self) -> Optional[int]:
        """The seed of the pattern ``hbm`` holds now, whichever path wrote it: the host-side ``seed`` of the
        eager launches, or the device-side one a graph replay advanced (read back here, not per run).
        ``None`` before the first run.  Not locked: a caller racing :meth:`run` holds ``_lock``."""
        if self._pattern == "graph":
            return int(self.seed_dev.item()) & 0xFFFFFFFF
        return self._pattern

    def _span_ms(self, h: List[int], i: int) -> float:
        begin = ~_u64(h, i) & 0xFFFFFFFFFFFFFFFF
        end = _u64(h, i + 2)
        return max(0.0, (end - begin) / self._tick_khz) if end and begin != 0xFFFFFFFFFFFFFFFF else 0.0

    def _launch_graph(self, graph) -> None:
        import torch

        with torch.cuda.device(self.device):
            sg = self.streams[0]
            sg.wait_stream(torch.cuda.current_stream(self.device))  # caller's writes to a / bt / hbm
            self.ev[0].record(sg)
            _check(load_library().odh_probe_graph_launch(graph, sg.cuda_stream))
            self.ev[4].record(sg)

    def _graph_result(self, t0: float) -> dict:
        h = self.host.tolist()
        return self._result(h, self._span_ms(h, ODH_SLOT_GRAPH_GEMM_SPAN), self._span_ms(h, ODH_SLOT_GRAPH_SWEEP_SPAN),
                            self.ev[0].elapsed_time(self.ev[4]), t0, graph=True)

    def _run_graph(self, graph) -> dict:
        t0 = time.perf_counter()
        self._pattern = None
        self._launch_graph(graph)
        self.ev[4].synchronize()
        self._pattern = "graph"
        return self._graph_result(t0)

    def _run(self) -> dict:
        import torch

        lib = load_library()
        t0 = time.perf_counter()
        with torch.cuda.device(self.device):
            sg, sh = self.streams
            cnt = self.counters
            xcd_blocks, err_xcd, gemm_err, hbm_err = (cnt.data_ptr() + 4 * slot for slot in (
                ODH_SLOT_XCD_BLOCKS, ODH_SLOT_ERR_XCD, ODH_SLOT_GEMM_ERR, ODH_SLOT_HBM_ERR))
            self.seed = (self.seed * 1664525 + 1013904223) & 0xFFFFFFFF
            self._pattern = None
            sg.wait_stream(torch.cuda.current_stream(self.device))  # caller's writes to a / bt / hbm
            with torch.cuda.stream(sg):
                cnt.zero_()
                self.ev[0].record(sg)
            g, h_ = sg.cuda_stream, (sh.cuda_stream if self.overlap else sg.cuda_stream)
            if self.overlap:
                sh.wait_event(self.ev[0])
            hs = sh if self.overlap else sg

            def sweep():
                self.ev[2].record(hs)
                _check(lib.odh_hbm_write(self.hbm.data_ptr(), self.hbm_bytes, self.seed, int(self.hbm_nontemporal),
                                         h_))
                _check(lib.odh_hbm_check(self.hbm.data_ptr(), self.hbm_bytes, self.seed, hbm_err, h_))
                self.ev[3].record(hs)

            if self.overlap:
                sweep()  # the longer, memory-bound part first: both are in flight together
            if self.fused:
                _check(lib.odh_probe_gemm_verify(self.a.data_ptr(), self.bt.data_ptr(), self.m, self.n, self.k,
                                                 self.tile_xcd.data_ptr(), xcd_blocks, gemm_err, err_xcd, g))
                self.ev[1].record(sg)
            else:
                _check(lib.odh_gemm_bf16(self.a.data_ptr(), self.bt.data_ptr(), self.c.data_ptr(), self.m, self.n,
                                         self.k, self.tile_xcd.data_ptr(), xcd_blocks, g))
                self.ev[1].record(sg)
                _check(lib.odh_probe_verify(self.c.data_ptr(), self.m, self.n, self.k, self.tile_xcd.data_ptr(),
                                            gemm_err, err_xcd, g))
            if not self.overlap:
                sweep()
            else:
                sg.wait_event(self.ev[3])
            with torch.cuda.stream(sg):
                self.host.copy_(cnt, non_blocking=True)
                self.ev[4].record(sg)
            self.ev[4].synchronize()
        self._pattern = self.seed
        h = self.host.tolist()
        return self._result(h, self.ev[0].elapsed_time(self.ev[1]), self.ev[2].elapsed_time(self.ev[3]),
                            self.ev[0].elapsed_time(self.ev[4]), t0, graph=False)

    def _result(self, h: List[int], gemm_ms: float, hbm_ms: float, probe_ms: float, t0: float, graph: bool) -> dict:
        xcd_blocks = h[ODH_SLOT_XCD_BLOCKS:ODH_SLOT_XCD_BLOCKS + ODH_N_XCD]
        err_xcd = h[ODH_SLOT_ERR_XCD:ODH_SLOT_ERR_XCD + ODH_N_XCD]
        gemm_err = h[ODH_SLOT_GEMM_ERR] & 0xFFFFFFFF
        hbm_err = _u64(h, ODH_SLOT_HBM_ERR)
        flops = 2.0 * self.m * self.n * self.k
        self.runs += 1
        ok = gemm_err == 0 and hbm_err == 0 and sum(xcd_blocks) == self.tiles
        return {
            "ok": bool(ok), "device": self.device.index, "gemm_ms": gemm_ms, "hbm_ms": hbm_ms,
            "gpu_ms": probe_ms, "fused_verify": self.fused, "overlap": self.overlap,
            "gemm_tflops": flops / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0,
            "hbm_gbps": 2.0 * self.hbm_bytes / (hbm_ms * 1e-3) / 1e9 if hbm_ms > 0 else 0.0,
            "gemm_errors": gemm_err, "hbm_errors": hbm_err, "xcd_blocks": xcd_blocks, "err_xcd": err_xcd,
            "xcds": sum(1 for x in xcd_blocks if x > 0), "wall_ms": (time.perf_counter() - t0) * 1e3,
            "graph": graph, "graph_error": self._graph_error,
        }


_probes: Dict[int, GpuProbe] = {}
_probe_lock = threading.Lock()


def get_probe(device: int, **kw) -> GpuProbe:
    with _probe_lock:
        p = _probes.get(device)
        if p is None:
            p = _probes[device] = GpuProbe(device, **kw)
        return p


XGMI_CHECK_BYTES = 64 << 20


def ring_pairs(devices: Sequence[int]) -> List[tuple]:
    """(reader, source) per xGMI link the multi-GPU probe checks: a ring over the pod's
    GPUs, so with k GPUs k links are read (MI355X: every GPU pair has a direct link)."""
    ds = list(dict.fromkeys(devices))
    if len(ds) < 2:
        return []
    if len(ds) == 2:
        return [(ds[1], ds[0]), (ds[0], ds[1])]
    return [(ds[(n + 1) % len(ds)], ds[n]) for n in range(len(ds))]


def link_check(pr: GpuProbe, ps: GpuProbe, nbytes: int = XGMI_CHECK_BYTES) -> dict:
    """One link: the GPU of probe ``pr`` reads the first ``nbytes`` of the HBM buffer of probe ``ps`` and
    verifies every word against the pattern ``ps`` wrote last (:attr:`GpuProbe.pattern_seed`).  Two probes
    on one device are a link like any other, without the peer mapping.  Whatever goes wrong, a source
    that has not run yet included, is the link's ``error``: no count, and not ok."""
    import torch

    reader, source = pr.device.index, ps.device.index
    r = {"reader": reader, "source": source, "ok": False}
    try:
        if pr is ps:
            raise ValueError("a link has two probes")
        n = min(nbytes, ps.hbm_bytes) & ~15
        first, second = sorted((pr, ps), key=lambda p: (p.device.index, id(p)))  # one order for every caller
        with first._lock, second._lock:
            seed = ps.pattern_seed
            if seed is None:
                raise RuntimeError(f"the probe of GPU {source} has written no pattern yet")
            _check(load_library().odh_peer_enable(reader, source))
            dev = pr.device
            with torch.cuda.device(dev):
                err = torch.zeros((2,), dtype=torch.int32, device=dev)
                s = pr.streams[0]
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.wait_stream(torch.cuda.current_stream(dev))
                torch.cuda.current_stream(ps.device).synchronize()  # source pattern is in HBM
                ev0.record(s)
                _check(load_library().odh_hbm_check(ps.hbm.data_ptr(), n, seed, err.data_ptr(), s.cuda_stream))
                ev1.record(s)
                ev1.synchronize()
                e = err.cpu().tolist()
            ms = ev0.elapsed_time(ev1)
        errors = _u64(e, 0)
        r.update(ok=errors == 0, errors=errors, bytes=n, ms=ms, gbps=n / (ms * 1e-3) / 1e9 if ms > 0 else 0.0)
    except Exception as ex:  # a link that cannot be checked fails the pod, not the agent
        r["error"] = repr(ex)
    return r


def xgmi_ring_check(devices: Sequence[int], nbytes: int = XGMI_CHECK_BYTES) -> List[dict]:
    """Peer-read check of a multi-GPU pod's xGMI links.

    Each GPU's probe has just written its seeded pattern into its HBM buffer; GPU
    ``reader`` now streams the first ``nbytes`` of GPU ``source``'s buffer over xGMI and
    verifies every word (:func:`link_check`: ``odh_hbm_check`` with a peer pointer).  One link failing
    fails the pod, like an XCD failing the GEMM check.  The reference has no equivalent: a
    multi-GPU notebook there starts on GPUs whose interconnect nobody has looked at.
    """
    out = []
    for reader, source in ring_pairs(devices):
        try:
            pr, ps = get_probe(reader), get_probe(source)
        except Exception as ex:  # a probe that cannot be built fails its links
            out.append({"reader": reader, "source": source, "ok": False, "error": repr(ex)})
            continue
        out.append(link_check(pr, ps, nbytes))
    return out


def probe_devices(devices: Sequence[int]) -> dict:
    results = []
    for d in devices:
        try:
            results.append(get_probe(d).run())
        except Exception as e:  # a failed probe fails the pod, it must not crash the agent
            results.append({"ok": False, "device": d, "error": repr(e)})
    links = xgmi_ring_check(devices) if all(r.get("ok") for r in results) else []
    error = next((r.get("error") or f"probe failed on GPU {r['device']}" for r in results if not r.get("ok")), None)
    if error is None:
        error = next((lk.get("error") or f"xGMI check failed reading GPU {lk['source']} from GPU {lk['reader']}"
                      for lk in links if not lk.get("ok")), None)
    out = {"ok": error is None, "devices": list(devices), "results": results, "error": error}
    if links:
        out["links"] = links
    return out


class LoadGenerator:
    """Keeps a GPU's matrix cores busy at ``duty`` (0..1) until :meth:`stop`."""

    def __init__(self, device: int = 0, duty: float = 1.0, chunk_ms: float = 5.0, blocks: int = 1024):
        self.device = device
        self.duty = max(0.0, min(1.0, duty))
        self.chunk_ms = chunk_ms
        self.blocks = blocks
        self._stop = threading.Event()
        self._thr: Optional[threading.Thread] = None
        self.launches = 0
        self.iters = 2048

    def _loop(self) -> None:
        import torch

        lib = load_library()
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            out = torch.empty((self.blocks * 256,), dtype=torch.float32, device=dev)
            s = _stream_ptr(dev)
            # calibrate iterations so one launch lasts ~chunk_ms
            t0 = time.perf_counter()
            _check(lib.odh_busy(out.data_ptr(), self.blocks, self.iters, s))
            torch.cuda.current_stream(dev).synchronize()
            dt = max(1e-4, time.perf_counter() - t0)
            self.iters = max(64, min(1 << 22, int(self.iters * (self.chunk_ms * 1e-3) / dt)))
            while not self._stop.is_set():
                t0 = time.perf_counter()
                _check(lib.odh_busy(out.data_ptr(), self.blocks, self.iters, s))
                torch.cuda.current_stream(dev).synchronize()
                self.launches += 1
                busy = time.perf_counter() - t0
                if self.duty < 1.0:
                    idle = busy * (1.0 - self.duty) / max(self.duty, 1e-3)
                    self._stop.wait(idle)

    def start(self) -> "LoadGenerator":
        self._thr = threading.Thread(target=self._loop, name=f"gpu-load-{self.device}", daemon=True)
        self._thr.start()
        return self

    def wait_running(self, timeout: float = 60.0) -> bool:
        """Block until the load is on the GPU (the first calibrated launch finished): the thread
        first initialises the HIP runtime, which takes from a few hundred ms to seconds."""
        deadline = time.monotonic() + timeout
        while self.launches < 1 and time.monotonic() < deadline:
            if self._thr is not None and not self._thr.is_alive():
                return False
            time.sleep(0.005)
        return self.launches >= 1

    def stop(self) -> None:
        self._stop.set()
        if self._thr is not None:
            self._thr.join(timeout=30)


def available() -> bool:
    """True when a GPU is visible (does not initialise HIP: device_count only)."""
    try:
        import torch

        return torch.cuda.device_count() > 0
    except Exception:
        return False


def loaded_libraries() -> List[str]:
    """Native libraries of this package mapped into the process (for smoke/bench logs)."""
    out = []
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "odh_kubeflow_amd" in line and line.rstrip().endswith(".so"):
                    p = line.split()[-1]
                    if p not in out:
                        out.append(p)
    except OSError:
        pass
    return out
