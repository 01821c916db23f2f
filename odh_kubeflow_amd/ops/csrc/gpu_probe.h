// C ABI of libodh_gpu_probe.so: every exported function and the layout of the counter block.
//
// gpu_probe.hip and probe_cli.cpp define these functions and include this header first, so
// a definition that disagrees with its declaration does not compile.  ops/gpu.py spells the
// same signatures for ctypes and mirrors the slot constants; tests/test_probe_abi.py reads
// this file as text and holds the two sides together (one declaration per statement, every
// constant as NAME = integer, keeps that parse trivial).
#pragma once

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

// The counter block: ODH_NCOUNT × i32 on the device, read back in one copy.  Slots 0-19 mean
// the same on every path.  From slot 20 on, the CLI (probe_cli.cpp) and the graph path
// (odh_probe_graph_create) each have a layout of their own: they share slots 20-23 and are
// never used on the same block.
enum {
  ODH_NCOUNT = 32,
  ODH_N_XCD = 8,
  ODH_SLOT_XCD_BLOCKS = 0,         // [ODH_N_XCD] workgroups that ran on each XCD
  ODH_SLOT_ERR_XCD = 8,            // [ODH_N_XCD] GEMM mismatches per XCD that computed them
  ODH_SLOT_GEMM_ERR = 16,          // u32: GEMM mismatches
  ODH_SLOT_HBM_ERR = 18,           // u64: HBM sweep mismatches
  ODH_SLOT_CLI_XGMI_ERR = 20,      // u64: mismatches on the xGMI link this device reads
  ODH_SLOT_CLI_RCCL_ERR = 22,      // u64: mismatches in this device's RCCL all-reduce result
  ODH_SLOT_GRAPH_GEMM_SPAN = 20,   // 2 × u64: ~(earliest begin), latest end (wall_clock64 ticks)
  ODH_SLOT_GRAPH_SWEEP_SPAN = 24,  // 2 × u64: the same for the HBM write + check
  // operand formats of the block-scaled (MX) kernels: the hardware's format codes
  ODH_MX_FP8 = 0,  // OCP e4m3fn, one byte per element
  ODH_MX_FP4 = 4,  // e2m1, two elements per byte (even k in the low nibble)
  ODH_MX_BF8 = 1,  // OCP e5m2, one byte per element
  ODH_MX_FP6 = 2,  // e2m3, packed: element k in bits [6k, 6k + 6) of the row, little endian
  ODH_MX_BF6 = 3,  // e3m2, packed as FP6
  ODH_MX_CLASSES = 315,  // floats in the table of expected values: (i mod 15, j mod 21)
  // operand formats of the dense FP16 / INT8 kernels (gpu_probe_dense.h)
  ODH_DT_F16 = 1,  // IEEE half, fp32 accumulation
  ODH_DT_I8 = 2,   // int8, int32 accumulation
  ODH_DT_I8_MUL_A = 25,  // the i8 probe operands: these odd multiples of the bf16 probe's A ...
  ODH_DT_I8_MUL_B = 41,  // ... and Bt, so the expected product is 1025 × the bf16 probe's
  // operand formats of the FP32 / FP64 kernels (gpu_probe_fp.h): the codes are the element sizes
  ODH_FP_F32 = 4,  // float, fp32 accumulation
  ODH_FP_F64 = 8,  // double, fp64 accumulation
  ODH_FP_F32_MUL_A = 25,  // the f32 probe operands: the i8 probe's multiples of the bf16 probe's A ...
  ODH_FP_F32_MUL_B = 41,  // ... and Bt: 1025 × the bf16 probe's product, exact in fp32 while 6150 K < 2^24
  ODH_FP_F64_MUL_A = 1048573,  // the f64 probe operands: odd 20-bit multiples ...
  ODH_FP_F64_MUL_B = 1048575,  // ... whose products toggle 41 mantissa bits; exact in fp64 at K <= 1365
  // operand formats of the 2:4 structured-sparsity kernels (gpu_probe_sparse.h)
  ODH_SP_BF16 = 0,  // bfloat16, 32x32x32, fp32 accumulation
  ODH_SP_F16 = 1,   // IEEE half, 32x32x32, fp32 accumulation
  ODH_SP_I8 = 2,    // int8, 32x32x64, int32 accumulation
  ODH_SP_FP8 = 3,   // OCP e4m3fn on both operands, 32x32x64, fp32 accumulation
  ODH_SP_BF8 = 4,   // OCP e5m2 on both operands, 32x32x64, fp32 accumulation
  ODH_SP_CLASSES = 210,  // ints in the table of expected values: (i mod 30, j mod 7)
  // destination formats of the converter kernels (gpu_probe_cvt.h): the hardware's format codes again, and bf16
  ODH_CVT_FP8 = 0,   // OCP e4m3fn
  ODH_CVT_BF8 = 1,   // OCP e5m2
  ODH_CVT_FP6 = 2,   // e2m3
  ODH_CVT_BF6 = 3,   // e3m2
  ODH_CVT_FP4 = 4,   // e2m1
  ODH_CVT_BF16 = 5,  // bfloat16: no scale
  ODH_CVT_BLOCKS = 256,  // workgroups of the fused check: one per CU
  ODH_CVT_TABLE = 256,   // bytes of its scale table
  // checks of the LDS step (gpu_probe_lds.h)
  ODH_LDS_MEM = 0,    // every dword of a CU's 160 KiB, written and read in different widths by different waves
  ODH_LDS_TR16 = 1,   // ds_read_b64_tr_b16
  ODH_LDS_TR8 = 2,    // ds_read_b64_tr_b8
  ODH_LDS_TR4 = 3,    // ds_read_b64_tr_b4
  ODH_LDS_TR6 = 4,    // ds_read_b96_tr_b6
  ODH_LDS_XLANE = 5,  // ds_bpermute / ds_permute / ds_swizzle, DPP, v_readlane / v_writelane, v_permlane16/32_swap
  ODH_LDS_BLOCKS = 256,   // workgroups of a fused check: one per CU
  ODH_LDS_TABLE = 1024,   // bytes of its key table
  ODH_LDS_CU_WORDS = 64,  // dwords of the bitmap of CUs behind a counter block: bit XCC_ID << 8 | SE_ID << 5 | SH_ID << 4 | CU_ID
  ODH_LDS_TR_RAW = 256,   // added to odh_lds_tr_read's check: the alignment of the addresses is not checked (measuring)
  // element formats of odh_transpose_codes
  ODH_TC_B16 = 0,  // 16-bit elements (bf16, f16)
  ODH_TC_B8 = 1,   // one byte per element (fp8, bf8, E8M0 scales)
  ODH_TC_B4 = 2,   // two nibbles per byte, even index low (fp4)
  ODH_TC_B6 = 3,   // element k in bits [6k, 6k + 6) of a row (fp6, bf6)
  // operand formats of the 16×16 matrix-core kernels (gpu_probe_m16.h)
  ODH_M16_BF16 = 0,  // bfloat16, 16x16x32, fp32 accumulation
  ODH_M16_F16 = 1,   // IEEE half, 16x16x32, fp32 accumulation
  ODH_M16_I8 = 2,    // int8, 16x16x64, int32 accumulation
  ODH_M16_FP8 = 3,   // OCP e4m3fn on both operands, block scaled, 16x16x128, fp32 accumulation
  ODH_M16_FP4 = 4,   // e2m1 on both operands, block scaled, 16x16x128, fp32 accumulation
};
static_assert(ODH_SLOT_XCD_BLOCKS + ODH_N_XCD <= ODH_SLOT_ERR_XCD, "per-XCD workgroups overlap the next slot");
static_assert(ODH_SLOT_ERR_XCD + ODH_N_XCD <= ODH_SLOT_GEMM_ERR, "per-XCD mismatches overlap the next slot");
static_assert(ODH_SLOT_GEMM_ERR + 1 <= ODH_SLOT_HBM_ERR && ODH_SLOT_HBM_ERR % 2 == 0, "HBM mismatches: aligned u64");
static_assert(ODH_SLOT_HBM_ERR + 2 <= ODH_SLOT_CLI_XGMI_ERR && ODH_SLOT_CLI_XGMI_ERR % 2 == 0, "CLI layout");
static_assert(ODH_SLOT_CLI_XGMI_ERR + 2 <= ODH_SLOT_CLI_RCCL_ERR && ODH_SLOT_CLI_RCCL_ERR + 2 <= ODH_NCOUNT,
              "CLI layout exceeds the block");
static_assert(ODH_SLOT_HBM_ERR + 2 <= ODH_SLOT_GRAPH_GEMM_SPAN && ODH_SLOT_GRAPH_GEMM_SPAN % 2 == 0, "graph layout");
static_assert(ODH_SLOT_GRAPH_GEMM_SPAN + 4 <= ODH_SLOT_GRAPH_SWEEP_SPAN &&
                  ODH_SLOT_GRAPH_SWEEP_SPAN + 4 <= ODH_NCOUNT,
              "graph layout exceeds the block");

extern "C" {

// every function returning int returns a hipError_t (0 = success) unless noted
int odh_gemm_shape_ok(int M, int N, int K);  // bool: multiples of the 128×128×32 tile
int odh_gemm_tiles(int M, int N, int K);     // workgroups the GEMM launches (0: bad shape)
const char* odh_error_string(int code);
int odh_wall_clock_khz(int device);  // wall_clock64() tick rate (0 on error)
int odh_probe_preload();
int odh_probe_fill(void* A, void* Bt, int M, int N, int K, hipStream_t stream);
int odh_gemm_bf16(const void* A, const void* Bt, float* C, int M, int N, int K, int* tile_xcd, int* xcd_blocks,
                  hipStream_t stream);
int odh_gemm_bf16_128(const void* A, const void* Bt, float* C, int M, int N, int K, int* tile_xcd, int* xcd_blocks,
                      hipStream_t stream);
int odh_gemm_bf16_256_variant(const void* A, const void* Bt, float* C, int M, int N, int K, int variant,
                              hipStream_t stream);
int odh_probe_verify(const float* C, int M, int N, int K, const int* tile_xcd, unsigned* err_total,
                     unsigned* err_xcd, hipStream_t stream);
int odh_probe_gemm_verify(const void* A, const void* Bt, int M, int N, int K, int* tile_xcd, int* xcd_blocks,
                          unsigned* err_total, unsigned* err_xcd, hipStream_t stream);
int odh_probe_gemm_verify_2buf(const void* A, const void* Bt, int M, int N, int K, int* tile_xcd, int* xcd_blocks,
                               unsigned* err_total, unsigned* err_xcd, hipStream_t stream);
int odh_probe_gemm_verify_deep(const void* A, const void* Bt, int M, int N, int K, int* tile_xcd, int* xcd_blocks,
                               unsigned* err_total, unsigned* err_xcd, int variant, hipStream_t stream);
int odh_hbm_write(void* buf, size_t bytes, uint32_t seed, int nontemporal, hipStream_t stream);
int odh_hbm_write_variant(void* buf, size_t bytes, uint32_t seed, int variant, int blocks, hipStream_t stream);
int odh_hbm_check(const void* buf, size_t bytes, uint32_t seed, unsigned long long* err, hipStream_t stream);
int odh_hbm_check_variant(const void* buf, size_t bytes, uint32_t seed, unsigned long long* err, int variant,
                          int blocks, hipStream_t stream);
int odh_const_check(const void* buf, size_t bytes, uint32_t expect, unsigned long long* err, hipStream_t stream);
int odh_peer_enable(int dev, int peer);
int odh_busy(float* out, int blocks, int iters, hipStream_t stream);
// Block-scaled FP8 / MXFP4 (fmt: ODH_MX_*): A [M][K] and Bt [N][K] codes, sA / sBt [rows][K/32] E8M0
// bytes (4-byte aligned), M and N multiples of 256, K of 64 (FP8) or 128 (FP4); table: ODH_MX_CLASSES floats
// BF8 as FP8; FP6 / BF6 rows are 3K/4 bytes (32 elements in 24 bytes), K a multiple of 128
int odh_mx_zero_classes(int K);  // host only: classes expecting 0 at this K (-1: K not a multiple of 128)
int odh_mx_fill(int fmt, void* A, void* Bt, void* sA, void* sBt, float* table, int M, int N, int K,
                hipStream_t stream);
int odh_mx_gemm(int fmt, const void* A, const void* Bt, const void* sA, const void* sBt, float* C, int M, int N, int K,
                hipStream_t stream);
int odh_mx_probe_gemm_verify(int fmt, const void* A, const void* Bt, const void* sA, const void* sBt,
                             const float* table, int M, int N, int K, int* tile_xcd, int* counters,
                             hipStream_t stream);
// Dense FP16 / INT8 (fmt: ODH_DT_*): A [M][K] and Bt [N][K] halves or int8 (16-byte aligned), C [M][N] fp32
// (f16) or int32 (i8); M and N multiples of 256, K of 32 (f16) or 64 (i8); counters: ODH_NCOUNT × i32 of
// this format's own on the device (slots ODH_SLOT_XCD_BLOCKS, ODH_SLOT_ERR_XCD, ODH_SLOT_GEMM_ERR)
int odh_dense_fill(int fmt, void* A, void* Bt, int M, int N, int K, hipStream_t stream);
int odh_dense_gemm(int fmt, const void* A, const void* Bt, void* C, int M, int N, int K, hipStream_t stream);
int odh_dense_probe_gemm_verify(int fmt, const void* A, const void* Bt, int M, int N, int K, int* tile_xcd,
                                int* counters, hipStream_t stream);
// FP32 / FP64 (fmt: ODH_FP_*): A [M][K] and Bt [N][K] floats or doubles (16-byte aligned), C [M][N] in the same
// type; M and N multiples of 256, K of 16 (f32) or 8 (f64); counters as for the dense kernels.  odh_fp_fill and
// odh_fp_probe_gemm_verify refuse a K at which the probe operands' sums are no longer exact integers
int odh_fp_tiles(int fmt, int M, int N);  // workgroups the kernels launch: 256×256 (f32) or 256×128 (f64) tiles (0: bad shape)
int odh_fp_fill(int fmt, void* A, void* Bt, int M, int N, int K, hipStream_t stream);
int odh_fp_gemm(int fmt, const void* A, const void* Bt, void* C, int M, int N, int K, hipStream_t stream);
int odh_fp_probe_gemm_verify(int fmt, const void* A, const void* Bt, int M, int N, int K, int* tile_xcd,
                             int* counters, hipStream_t stream);
// 2:4 structured sparsity (fmt: ODH_SP_*): C = A · Btᵀ with two of every four consecutive elements of an A row
// kept.  Ac [M][K/2]: the kept elements, 2g and 2g+1 those of group g (dense columns 4g … 4g+3); meta [M][K/8]
// bytes: group g of a row is the nibble at bits [4g, 4g+4) of the row, little endian, p0 | p1 << 2 = the dense
// positions of its two kept elements, p0 < p1 (a nibble with p0 >= p1 is unspecified); Bt [N][K] dense, in A's
// element type: bf16, half, int8 or one-byte e4m3fn / e5m2 codes; C [M][N] fp32, int32 for i8.  Ac and Bt are
// 16-byte aligned, meta 4-byte aligned; M and N multiples of 256, K of 64 (bf16, f16) or 128 (i8, fp8, bf8);
// table: ODH_SP_CLASSES ints, the expected sums of the probe operands; counters as for the dense kernels.
// odh_sparse_fill and odh_sparse_probe_gemm_verify refuse a K at which a class expects 0
int odh_sparse_zero_classes(int K);  // host only: classes expecting 0 at this K (-1: K not a positive multiple of 64)
int odh_sparse_fill(int fmt, void* Ac, void* meta, void* Bt, int* table, int M, int N, int K, hipStream_t stream);
int odh_sparse_gemm(int fmt, const void* Ac, const void* meta, const void* Bt, void* C, int M, int N, int K,
                    hipStream_t stream);
int odh_sparse_probe_gemm_verify(int fmt, const void* Ac, const void* meta, const void* Bt, const int* table, int M,
                                 int N, int K, int* tile_xcd, int* counters, hipStream_t stream);
// Converters (fmt: ODH_CVT_*): x [rows][K] f32, row-major, 16-byte aligned, K a multiple of 32; codes in the layout
// odh_mx_gemm reads (FP8 / BF8 a byte per element, FP4 two per byte, FP6 / BF6 32 in 24 bytes), 8-byte aligned, or
// [rows][K] bfloat16 for ODH_CVT_BF16, which takes no scales; scales [rows][K/32] E8M0 bytes.  The family of the
// fused check: odh_cvt_family_size cases, of which odh_cvt_family writes n from first on as x (f32 bits), the
// scale byte, the destination select in bits 8-9 of the same word, and the expected code, sign included
unsigned odh_cvt_family_size(int fmt);  // host only (0: no such format)
int odh_cvt_family(int fmt, unsigned first, unsigned n, uint32_t* x, uint32_t* scale, uint32_t* expect);  // host only; 0, or -1
int odh_cvt_fill(int fmt, void* scale_table, hipStream_t stream);  // ODH_CVT_TABLE bytes
int odh_cvt_encode(int fmt, const float* x, const void* scales, void* codes, long rows, long K, hipStream_t stream);
int odh_cvt_quantize(int fmt, const float* x, void* codes, void* scales_out, long rows, long K, hipStream_t stream);
int odh_cvt_probe_verify(int fmt, const void* scale_table, int* counters, hipStream_t stream);
// The LDS step (check: ODH_LDS_*; gpu_probe_lds.h).  table: ODH_LDS_TABLE bytes on the device, 4-byte aligned;
// counters: ODH_NCOUNT × i32 of this check's own (slots as for the converters) and ODH_LDS_CU_WORDS dwords behind
// them, the bitmap of the CUs the workgroups ran on.  odh_lds_tr_read: one wave, one transposing read; image
// (bytes of it, a multiple of 4, at most 65536) is copied to LDS, lane l reads at byte address lane_addr[l] (64
// of them, on the host) and stores its 8 or 12 result bytes at out + 8 l or out + 12 l; addresses out of range, or
// misaligned for the instruction unless ODH_LDS_TR_RAW is added to check, are refused.  odh_lds_xlane: one
// wave, one exchange of the 64 values in (the two swaps: of 128, lane l's second register at 64 + l) into out;
// op 0 … 7: ds_bpermute, ds_permute, ds_swizzle, DPP, v_readlane, v_writelane, v_permlane16_swap,
// v_permlane32_swap; arg: its selector (gpu_probe_lds.h).  odh_transpose_codes (fmt: ODH_TC_*): src [R][C]
// elements, row-major and packed, to dst [C][R]; R and C multiples of 128, both buffers 16-byte aligned
unsigned long long odh_lds_cases(int check);  // host only: elements compared per launch (0: no such check)
unsigned long long odh_lds_fault_count(int check, int table_byte);  // host only: mismatches when that byte is wrong
int odh_lds_fill(int check, void* table, hipStream_t stream);
int odh_lds_probe_verify(int check, const void* table, int* counters, hipStream_t stream);
int odh_lds_tr_read(int check, const void* image, unsigned bytes, const uint32_t* lane_addr, void* out,
                    hipStream_t stream);
int odh_lds_xlane(int op, int arg, const uint32_t* in, uint32_t* out, hipStream_t stream);
int odh_transpose_codes(int fmt, const void* src, void* dst, long R, long C, hipStream_t stream);
// The 16×16 matrix-core shapes (fmt: ODH_M16_*; gpu_probe_m16.h): operands in the public layouts of odh_gemm_bf16
// (bf16), odh_dense_gemm (f16, i8) and odh_mx_gemm (fp8, fp4, scales [rows][K/32]); C [M][N] fp32, int32 for i8; M
// and N multiples of 256, K of 32 (bf16, f16), 64 (i8) or 128 (fp8, fp4).  sA, sBt and table are NULL for bf16, f16
// and i8 (a non-NULL one is refused) and odh_mx_fill's for fp8 and fp4; the operands of the fused check are
// odh_probe_fill's, odh_dense_fill's or odh_mx_fill's; counters as for the dense kernels.  odh_m16_one: one wave, one
// instruction on a zero accumulator; a and b 64 lanes × 8 dwords (a format uses the low 4 or 8 of a lane), 16-byte
// aligned; sa and sb 64 scale dwords (NULL for bf16, f16 and i8); opsel_a and opsel_b 0 … 3; d 64 × 4 dwords
int odh_m16_gemm(int fmt, const void* A, const void* Bt, const void* sA, const void* sBt, void* C, int M, int N, int K,
                 hipStream_t stream);
int odh_m16_probe_gemm_verify(int fmt, const void* A, const void* Bt, const void* sA, const void* sBt,
                              const float* table, int M, int N, int K, int* tile_xcd, int* counters,
                              hipStream_t stream);
int odh_m16_one(int fmt, const uint32_t* a, const uint32_t* b, const uint32_t* sa, const uint32_t* sb, int opsel_a,
                int opsel_b, void* d, hipStream_t stream);
// counters: ODH_NCOUNT × i32 on the device (graph layout); host: the same, pinned; seed: one u32 on the device;
// *out: the handle, NULL after every failure
int odh_probe_graph_create(const void* A, const void* Bt, int M, int N, int K, int* tile_xcd, int* counters,
                           void* hbm, size_t hbm_bytes, uint32_t* seed, int* host, int serial, void** out);
int odh_probe_graph_launch(void* handle, hipStream_t stream);
void odh_probe_graph_destroy(void* handle);
// the start-up probe program (probe_cli.cpp); returns the process exit status
int odh_probe_cli(int argc, char** argv);

}  // extern "C"
