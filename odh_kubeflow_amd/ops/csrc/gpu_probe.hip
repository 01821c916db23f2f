// MI355X (gfx950) node-agent kernels: notebook start-up probe and synthetic GPU load.
//
// The reference control plane (harshad16/odh-kubeflow) never touches the accelerator:
// GPU support there is PodSpec passthrough (kf/controllers/notebook_controller.go:469).
// On an 8×MI355X node the node agent additionally proves that the GPU it is about to
// hand to a notebook is healthy before the pod is reported Ready, and drives synthetic
// load for the GPU-busy culler.  Everything here is written for CDNA4 directly:
//
//  * odh_gemm_bf16 — bf16 GEMM on the matrix cores (v_mfma_f32_32x32x16_bf16), fp32 out:
//    the 256×256×64 LDS-DMA kernel where it divides the shape, else odh_gemm_bf16_128:
//    128×128 tile per 256-thread workgroup (4 waves, 2×2 of 32×32 MFMA tiles each),
//    K staged through LDS in 32-deep double-buffered tiles with an XOR swizzle that
//    makes the 16-lane ds_read_b128 groups conflict-free, and an XCD-aware blockIdx
//    remap so the tiles of one XCD share A panels in that XCD's L2.  Every workgroup
//    records the XCD (HW_REG_XCC_ID) it ran on, so a verification failure is pinned to
//    the chiplet that produced it.
//  * odh_probe_gemm_verify — the start-up probe's GEMM: 256×256 tile, BK=32 stages in a
//    4-buffer LDS-DMA ring with three stages in flight across counted-vmcnt raw barriers,
//    result checked in registers (no C store); 1.1 PFLOP/s bf16 at 4096³ on MI355X.
//  * odh_probe_fill / odh_probe_verify — exact integer-valued operands whose product
//    has a closed form (period 35 in k), so the check needs no host reference and no
//    second GEMM: every element is compared bit-exactly on the GPU.
//  * odh_hbm_write / odh_hbm_check — 16 B/lane streaming pattern write + verify over a
//    resident HBM3E buffer (bandwidth and bit errors in one pass).
//  * odh_peer_enable — lets one GPU read another's HBM over xGMI; the multi-GPU probe
//    then runs odh_hbm_check on GPU j against GPU i's freshly written pattern buffer (a
//    ring over the pod's GPUs: every link verified, per-link GB/s).
//  * odh_const_check — every word of a buffer equal to one value (the RCCL result check).
//  * odh_probe_graph_create / _launch / _destroy — the probe captured as one hipGraph.
//  * odh_gemm_bf16_256_variant, odh_probe_gemm_verify_2buf / _deep, odh_hbm_write_variant,
//    odh_hbm_check_variant — A/B entry points (microbenchmarks, kernel numerics tests).
//  * odh_mx_fill / odh_mx_gemm / odh_mx_probe_gemm_verify — the same exact check on the
//    block-scaled path in each of its five operand formats, FP8, BF8, FP6, BF6 and MXFP4
//    (v_mfma_scale_f32_32x32x64_f8f6f4; gpu_probe_mx.h), and
//    odh_mx_zero_classes, the host-side guard against a K at which that check is blind.
//  * odh_dense_fill / odh_dense_gemm / odh_dense_probe_gemm_verify — the same exact check on the
//    FP16 and INT8 paths (v_mfma_f32_32x32x16_f16, v_mfma_i32_32x32x32_i8; gpu_probe_dense.h):
//    the deep-pipelined 256² tile again, with halves or int8 in its 64-byte stage rows.
//  * odh_fp_fill / odh_fp_gemm / odh_fp_probe_gemm_verify — the same exact check on the FP32 and
//    FP64 paths (v_mfma_f32_32x32x2_f32, v_mfma_f64_16x16x4_f64; gpu_probe_fp.h): the ring again, with
//    floats or doubles in its 64-byte stage rows and a 256×128 tile for f64 (odh_fp_tiles).
//  * odh_sparse_fill / odh_sparse_gemm / odh_sparse_probe_gemm_verify — the same exact check on the 2:4
//    structured-sparsity path (v_smfmac_*: bf16, f16, i8, fp8, bf8; gpu_probe_sparse.h): compressed A,
//    metadata and dense Bt on a three-slot ring, against a 30 × 7 table, and odh_sparse_zero_classes, the
//    host-side guard against a K at which that check is blind.
//  * odh_cvt_fill / odh_cvt_probe_verify — the converters that make low-precision codes at run time
//    (v_cvt_scalef32_pk_fp8_f32 / _bf8_f32 / _fp4_f32, v_cvt_scalef32_2xpk16_fp6_f32 / _bf6_f32,
//    v_cvt_pk_bf16_f32; gpu_probe_cvt.h): every rounding case of every code at every scale, on every SIMD,
//    against codes known by construction; odh_cvt_family, the host's view of that family; and
//    odh_cvt_quantize / odh_cvt_encode, f32 rows to OCP MX codes and scales in the layout odh_mx_gemm reads.
//  * odh_lds_fill / odh_lds_probe_verify — the LDS itself, the transposing LDS reads (ds_read_b64_tr_b16 / _b8 /
//    _b4, ds_read_b96_tr_b6) and the lane exchanges (ds_bpermute, ds_swizzle, DPP, v_readlane, v_permlane32_swap and
//    their kin; gpu_probe_lds.h), one workgroup per CU, against closed forms; odh_lds_cases and
//    odh_lds_fault_count, the host's view of what they compare; odh_lds_tr_read and odh_lds_xlane, one
//    instruction at a time, which the lane maps were measured with; and odh_transpose_codes, packed codes [R][C]
//    to [C][R] through those reads.
//  * odh_m16_gemm / odh_m16_probe_gemm_verify — the same exact checks on the 16×16 shapes of the matrix-core
//    instructions (v_mfma_f32_16x16x32_bf16 / _f16, v_mfma_i32_16x16x64_i8, v_mfma_scale_f32_16x16x128_f8f6f4 with FP8
//    or FP4 operands; gpu_probe_m16.h), whose operand, scale and C/D maps are not the 32×32 ones, on the operands and
//    tables of the fills above; and odh_m16_one, one instruction at a time, which the maps were measured with.
//  * odh_busy — MFMA issue loop with 4 independent accumulators (drives gfx activity
//    for the culler's amdgpu signal under synthetic load).
//
// C ABI only, declared in gpu_probe.h (loaded with ctypes after torch, sharing torch's
// libamdhip64.so.7; linked by odh-gpu-probe).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <utility>

#include "gpu_probe.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

namespace {

constexpr int BM = 128;
constexpr int BN = 128;
constexpr int BK = 32;           // bf16 elements per K tile = 4 × 16-byte chunks per row
constexpr int CH = BK / 8;       // 16-byte chunks per tile row
constexpr int THREADS = 256;

__device__ __forceinline__ unsigned xcc_id() {
  unsigned x;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
  return x & 7u;
}

// chunk c of tile row r lives at slot c ^ ((r >> 2) & 3): the 16 rows read by one
// ds_read_b128 lane group then hit 16 distinct 16-byte slots of the 256-byte bank row.
__device__ __forceinline__ int swz(int r, int c) { return r * CH + (c ^ ((r >> 2) & 3)); }

__global__ __launch_bounds__(THREADS, 2) void gemm_bf16_kernel(
    const uint4* __restrict__ A, const uint4* __restrict__ Bt, float* __restrict__ C,
    int /*M: the grid covers it*/, int N, int K, int* __restrict__ tile_xcd, int* __restrict__ xcd_blocks) {
  __shared__ uint4 sA[2][BM * CH];
  __shared__ uint4 sB[2][BN * CH];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int wm = w >> 1, wn = w & 1;
  const int tiles_n = N / BN;
  const int nwg = gridDim.x;
  int bid = blockIdx.x;
  if ((nwg & 7) == 0) bid = (bid & 7) * (nwg >> 3) + (bid >> 3);  // XCD-contiguous tiles
  const int tm = bid / tiles_n;
  const int tn = bid - tm * tiles_n;

  if (tid == 0) {
    const unsigned x = xcc_id();
    if (tile_xcd) tile_xcd[bid] = (int)x;
    if (xcd_blocks) atomicAdd(&xcd_blocks[x], 1);
  }

  const size_t kch = (size_t)(K / 8);  // 16-byte chunks per global row
  const uint4* Ag = A + (size_t)tm * BM * kch;
  const uint4* Bg = Bt + (size_t)tn * BN * kch;
  const int r0 = tid >> 2, c0 = tid & 3, r1 = r0 + 64;

  uint4 ra0, ra1, rb0, rb1;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nkt = K / BK;
  {
    ra0 = Ag[r0 * kch + c0];
    ra1 = Ag[r1 * kch + c0];
    rb0 = Bg[r0 * kch + c0];
    rb1 = Bg[r1 * kch + c0];
    sA[0][swz(r0, c0)] = ra0;
    sA[0][swz(r1, c0)] = ra1;
    sB[0][swz(r0, c0)] = rb0;
    sB[0][swz(r1, c0)] = rb1;
  }
  __syncthreads();

  const int lr = lane & 31, lh = lane >> 5;
  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nkt;
    if (more) {  // issue next tile's global loads before this tile's LDS reads + MFMAs
      const size_t kc = (size_t)(kt + 1) * CH + c0;
      ra0 = Ag[r0 * kch + kc];
      ra1 = Ag[r1 * kch + kc];
      rb0 = Bg[r0 * kch + kc];
      rb1 = Bg[r1 * kch + kc];
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int c = 2 * s + lh;  // lane half h holds k = 16s + 8h .. +7
      bf16x8 af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = wm * 64 + i * 32 + lr;
        af[i] = __builtin_bit_cast(bf16x8, sA[cur][swz(row, c)]);
        const int col = wn * 64 + i * 32 + lr;
        bf[i] = __builtin_bit_cast(bf16x8, sB[cur][swz(col, c)]);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    if (more) {
      const int nxt = cur ^ 1;
      sA[nxt][swz(r0, c0)] = ra0;
      sA[nxt][swz(r1, c0)] = ra1;
      sB[nxt][swz(r0, c0)] = rb0;
      sB[nxt][swz(r1, c0)] = rb1;
    }
    __syncthreads();
  }

  // C/D map of 32x32x16: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = tn * BN + wn * 64 + j * 32 + lr;
      const int rbase = tm * BM + wm * 64 + i * 32 + 4 * lh;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = rbase + (r & 3) + 8 * (r >> 2);
        C[(size_t)row * N + col] = acc[i][j][r];
      }
    }
}

// ---------------------------------------------------------------------------------------
// 256×256×64 tile, 512 threads (8 waves as 2(M)×4(N), 128×64 outputs per wave), one
// workgroup per CU (128 KiB of LDS: 2 buffers × (A+B) × 256 rows × 128 B).  Tiles are
// staged global→LDS by the LDS-DMA path (global_load_lds_dwordx4: no VGPR round trip, no
// ds_write pass); the image is lane-linear per wave instruction, so the bank swizzle is
// applied to the SOURCE address: LDS slot s of row r holds K-chunk s ^ ((r >> 1) & 7),
// which puts the 16 rows read by one ds_read_b128 lane group on 16 distinct 16-byte slots
// of the 256-byte bank row.  The next tile's DMA is in flight during this tile's MFMAs.
// VERIFY=true replaces the C store by an in-register check against the closed-form product
// of the probe operands (no C round trip through HBM, no second kernel).

constexpr int G_BM = 256;
constexpr int G_BN = 256;
constexpr int G_BK = 64;
constexpr int G_CH = G_BK / 8;  // 16-byte chunks per tile row
constexpr int G_THREADS = 512;
constexpr int G_TILE = G_BM * G_CH;  // uint4 per operand tile

__device__ __forceinline__ int gswz(int r, int c) { return r * G_CH + (c ^ ((r >> 1) & 7)); }

// expected C[i][j] of the probe operands depends only on (i mod 5, j mod 7)
__device__ int probe_expect(int ia5, int jb7, int K) {
  const int q = K / 35, rem = K - q * 35;
  const int ia = ia5 * 3 % 5, jb = jb7 * 11 % 7;
  int s = 0;
  for (int r = 0; r < 35; ++r) {
    int a = ia + (r * 7) % 5;
    a = (a >= 5 ? a - 5 : a) - 2;
    int b = jb + (r * 5) % 7;
    b = (b >= 7 ? b - 7 : b) - 3;
    s += (q + (r < rem ? 1 : 0)) * a * b;
  }
  return s;
}

// bijective XCD remap: the blocks dispatched to one XCD (orig % 8) take consecutive tiles
__device__ __forceinline__ int xcd_tile(int orig, int nwg) {
  const int xq = nwg >> 3, xr = nwg & 7, xs = orig & 7;
  return (xs < xr ? xs * (xq + 1) : xr * (xq + 1) + (xs - xr) * xq) + (orig >> 3);
}

template <bool VERIFY, bool PIPE = true>
__global__ __launch_bounds__(G_THREADS, 1) void gemm256_kernel(
    const uint4* __restrict__ A, const uint4* __restrict__ Bt, float* __restrict__ C, int /*M*/, int N, int K,
    int* __restrict__ tile_xcd, int* __restrict__ xcd_blocks, unsigned* __restrict__ err_total,
    unsigned* __restrict__ err_xcd) {
  __shared__ uint4 lds[2 * 2 * G_TILE];  // [buffer][A, B][row × chunk]
  __shared__ float expect[35];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int wm = w >> 2, wn = w & 3;
  const int tiles_n = N / G_BN;
  const int bid = xcd_tile(blockIdx.x, gridDim.x);
  const int tm = bid / tiles_n;
  const int tn = bid - tm * tiles_n;
  const unsigned xcc = xcc_id();
  if (tid == 0) {
    if (tile_xcd) tile_xcd[bid] = (int)xcc;
    if (xcd_blocks) atomicAdd(&xcd_blocks[xcc], 1);
  }
  if (VERIFY && tid < 35) expect[tid] = (float)probe_expect(tid / 7, tid % 7, K);

  const size_t kch = (size_t)(K / 8);
  const uint4* Ag = A + (size_t)tm * G_BM * kch;
  const uint4* Bg = Bt + (size_t)tn * G_BN * kch;

  // DMA of K-tile kt into buffer b: wave w fills rows [32w, 32w + 32) of A and of B,
  // 8 rows (1 KiB) per instruction; lane l lands at LDS chunk p = base + l.
  auto issue = [&](int kt, int b) {
    uint4* la = lds + (b * 2 + 0) * G_TILE;
    uint4* lb = lds + (b * 2 + 1) * G_TILE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int base = (w * 4 + i) * 64;
      const int p = base + lane;
      const int row = p >> 3;
      const int c = (p & 7) ^ ((row >> 1) & 7);
      const size_t g = (size_t)row * kch + (size_t)kt * G_CH + c;
      __builtin_amdgcn_global_load_lds(Ag + g, la + base, 16, 0, 0);
      __builtin_amdgcn_global_load_lds(Bg + g, lb + base, 16, 0, 0);
    }
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nkt = K / G_BK;
  issue(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int lr = lane & 31, lh = lane >> 5;
  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nkt) issue(kt + 1, cur ^ 1);  // buffer cur^1 was released by the last barrier
    const uint4* sa = lds + (cur * 2 + 0) * G_TILE;
    const uint4* sb = lds + (cur * 2 + 1) * G_TILE;
    // fragments of k-substep s (lane half h holds k = 16s + 8h .. +7); with PIPE the reads
    // of substep s+1 are issued before the MFMAs of substep s (two fragment sets in
    // registers), so LDS latency hides under matrix-core work instead of stalling on it
    bf16x8 af[2][4], bfr[2][2];
    auto load = [&](int s, int slot) {
      const int c = 2 * s + lh;
#pragma unroll
      for (int i = 0; i < 4; ++i) af[slot][i] = __builtin_bit_cast(bf16x8, sa[gswz(wm * 128 + i * 32 + lr, c)]);
#pragma unroll
      for (int j = 0; j < 2; ++j) bfr[slot][j] = __builtin_bit_cast(bf16x8, sb[gswz(wn * 64 + j * 32 + lr, c)]);
    };
    if (PIPE) load(0, 0);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int slot = PIPE ? (s & 1) : 0;
      if (PIPE) {
        if (s + 1 < 4) load(s + 1, (s + 1) & 1);
      } else {
        load(s, 0);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[slot][i], bfr[slot][j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // C/D map of 32x32x16: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  unsigned bad = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = tn * G_BN + wn * 64 + j * 32 + lr;
      const int rbase = tm * G_BM + wm * 128 + i * 32 + 4 * lh;
      if (VERIFY) {
        const int c7 = col % 7;
        const int r5 = rbase % 5;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int rr = r5 + (r & 3) + 8 * (r >> 2);
          rr %= 5;
          bad += acc[i][j][r] != expect[rr * 7 + c7];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) C[(size_t)(rbase + (r & 3) + 8 * (r >> 2)) * N + col] = acc[i][j][r];
      }
    }
  if (VERIFY) {
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
    if (lane == 0 && bad) {
      atomicAdd(err_total, bad);
      if (err_xcd) atomicAdd(&err_xcd[xcc], bad);
    }
  }
}

// host side: shapes the 256² kernels take (every one of them passes odh_gemm_shape_ok), their
// workgroup count, and the guard of the fused probe entry points
bool gemm256_ok(int M, int N, int K) {
  return M > 0 && N > 0 && K > 0 && M % G_BM == 0 && N % G_BN == 0 && K % G_BK == 0;
}
int gemm256_tiles(int M, int N) { return (M / G_BM) * (N / G_BN); }
bool fused_probe_ok(int M, int N, int K, const unsigned* err_total) { return gemm256_ok(M, N, K) && err_total; }

// ---------------------------------------------------------------------------------------
// Deep-pipelined 256×256 tile: BK = 32 stages in a 4-buffer LDS ring (4 × 32 KiB), with
// THREE stages in flight across every barrier.  At ~1 workgroup per CU the HBM/MALL
// latency of a stage (≈1-2 µs under load) is longer than one BK=64 tile of MFMA work
// (≈0.9 µs at peak), so the 2-buffer kernel above stalls on its per-tile vmcnt(0); here
// the wait is a COUNTED vmcnt (the two younger stages stay outstanding) followed by a raw
// s_barrier (a __syncthreads() fence would drain the LDS-DMA queue), and the stage issued
// after the barrier refills the buffer every wave finished reading one iteration ago.
// All LDS (ring + the verify table) is ONE __shared__ array, so hipcc does not fence the
// ds_reads of a stage behind the in-flight DMA of younger stages.
// LDS image per operand stage: 256 rows × 4 chunks of 16 B; slot s of row r holds K-chunk
// s ^ ((r >> 2) & 3) (conflict-free 16-lane ds_read_b128 groups), applied on the SOURCE
// address because the DMA image is lane-linear.

// In-kernel span timestamps for graph replays (events cannot split one graph launch):
// ts[0] holds ~(earliest start) so a zeroed slot works with atomicMax, ts[1] the latest
// end; both in wall_clock64() ticks (hipDeviceAttributeWallClockRate kHz).  Same-address
// atomics serialise in one L2 channel (measured: one per wave of the 16384-workgroup HBM
// sweep cost 0.16 ms), so the sweep stamps only from its first / last TS_EDGE workgroups
// (dispatched in order, ~16 KiB each: the span is exact to a few µs).
constexpr int TS_EDGE = 64;
__device__ __forceinline__ void ts_begin(unsigned long long* ts) { atomicMax(&ts[0], ~wall_clock64()); }
__device__ __forceinline__ void ts_end(unsigned long long* ts) { atomicMax(&ts[1], (unsigned long long)wall_clock64()); }

constexpr int D_BK = 32;
constexpr int D_CH = D_BK / 8;            // 16-byte chunks per row
constexpr int D_NBUF = 4;
constexpr int D_TILE = G_BM * D_CH;       // uint4 per operand stage (1024 = 16 KiB)
constexpr int D_RING = D_NBUF * 2 * D_TILE;

__device__ __forceinline__ int dswz(int r, int c) { return r * D_CH + (c ^ ((r >> 2) & 3)); }

template <bool VERIFY, bool XB = false, int GM = 1>
__global__ __launch_bounds__(G_THREADS, 1) void gemm256d_kernel(
    const uint4* __restrict__ A, const uint4* __restrict__ Bt, float* __restrict__ C, int M, int N, int K,
    int* __restrict__ tile_xcd, int* __restrict__ xcd_blocks, unsigned* __restrict__ err_total,
    unsigned* __restrict__ err_xcd, unsigned long long* __restrict__ ts = nullptr) {
  __shared__ uint4 lds[D_RING + 9];  // ring, then 35 floats of the probe's expected values
  float* expect = reinterpret_cast<float*>(lds + D_RING);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int wm = w >> 2, wn = w & 3;
  const int tiles_n = N / G_BN;
  const int bid = xcd_tile(blockIdx.x, gridDim.x);
  // GM > 1: consecutive tile ids walk GM tile-rows × (32/GM) columns, so the 32 tiles of
  // one XCD share GM A panels and 32/GM B panels in that XCD's L2 (GM = 1: row-major)
  int tm, tn;
  if (GM > 1 && (M / G_BM) % GM == 0) {
    const int band = bid / (GM * tiles_n), in_band = bid - band * GM * tiles_n;
    tm = band * GM + in_band % GM;
    tn = in_band / GM;
  } else {
    tm = bid / tiles_n;
    tn = bid - tm * tiles_n;
  }
  const unsigned xcc = xcc_id();
  if (tid == 0) {
    if (ts) ts_begin(ts);
    if (tile_xcd) tile_xcd[bid] = (int)xcc;
    if (xcd_blocks) atomicAdd(&xcd_blocks[xcc], 1);
  }
  if (VERIFY && tid < 35) expect[tid] = (float)probe_expect(tid / 7, tid % 7, K);

  const size_t kch = (size_t)(K / 8);
  const uint4* Ag = A + (size_t)tm * G_BM * kch;
  const uint4* Bg = Bt + (size_t)tn * G_BN * kch;

  // stage kt → ring slot b: wave w fills rows [32w, 32w + 32) of A and of B (16 rows per
  // instruction); 4 DMA instructions per thread per stage
  auto issue = [&](int kt, int b) {
    uint4* la = lds + (b * 2 + 0) * D_TILE;
    uint4* lb = lds + (b * 2 + 1) * D_TILE;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int base = (w * 2 + i) * 64;
      const int p = base + lane;
      const int row = p >> 2;
      const int c = (p & 3) ^ ((row >> 2) & 3);
      const size_t g = (size_t)row * kch + (size_t)kt * D_CH + c;
      __builtin_amdgcn_global_load_lds(Ag + g, la + base, 16, 0, 0);
      __builtin_amdgcn_global_load_lds(Bg + g, lb + base, 16, 0, 0);
    }
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nkt = K / D_BK;
  const int lr = lane & 31, lh = lane >> 5;
  // fragments of one stage: both k-substeps (lane half h holds k = 16s + 8h .. +7)
  auto read_stage = [&](int kt, bf16x8 (&af)[2][4], bf16x8 (&bfr)[2][2]) {
    const int cur = kt & 3;
    const uint4* sa = lds + (cur * 2 + 0) * D_TILE;
    const uint4* sb = lds + (cur * 2 + 1) * D_TILE;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int c = 2 * s + lh;
#pragma unroll
      for (int i = 0; i < 4; ++i) af[s][i] = __builtin_bit_cast(bf16x8, sa[dswz(wm * 128 + i * 32 + lr, c)]);
#pragma unroll
      for (int j = 0; j < 2; ++j) bfr[s][j] = __builtin_bit_cast(bf16x8, sb[dswz(wn * 64 + j * 32 + lr, c)]);
    }
  };
  auto mfma_stage = [&](const bf16x8 (&af)[2][4], const bf16x8 (&bfr)[2][2]) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s][i], bfr[s][j], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };

  if (!XB) {
    issue(0, 0);
    if (nkt > 1) issue(1, 1);
    if (nkt > 2) issue(2, 2);
    for (int kt = 0; kt < nkt; ++kt) {
      // retire THIS wave's DMA of stage kt (younger stages stay in flight), then the barrier
      // makes every wave's part visible and proves stage kt-1's slot is no longer read
      const int ahead = nkt - 1 - kt;
      if (ahead >= 2)
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else if (ahead == 1)
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (kt + 3 < nkt) issue(kt + 3, (kt + 3) & 3);
      bf16x8 af[2][4], bfr[2][2];
      read_stage(kt, af, bfr);
      mfma_stage(af, bfr);
    }
  } else {
    // XB: the barrier that publishes stage kt+1 comes BEFORE stage kt's MFMAs, so stage kt+1's
    // ds_reads run under stage kt's matrix work (two fragment sets in registers); the slot of
    // stage kt (already in registers: lgkmcnt(0) before the barrier) is refilled with kt+4,
    // so four stages are in flight.
    issue(0, 0);
    if (nkt > 1) issue(1, 1);
    if (nkt > 2) issue(2, 2);
    if (nkt > 3) issue(3, 3);
    {
      const int ahead = nkt - 1 < 3 ? nkt - 1 : 3;
      if (ahead == 3)
        asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
      else if (ahead == 2)
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else if (ahead == 1)
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    bf16x8 xa[2][4], xb[2][2], ya[2][4], yb[2][2];
    read_stage(0, xa, xb);
    for (int kt = 0; kt < nkt; kt += 2) {
      // stage kt in x; publish kt+1, read it into y, MFMA x
      if (kt + 1 < nkt) {
        const int ahead = nkt - 2 - kt;  // issued stages younger than kt+1 (at most kt+3)
        if (ahead >= 2)
          asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
        else if (ahead == 1)
          asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
        else
          asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (kt + 4 < nkt) issue(kt + 4, kt & 3);
        read_stage(kt + 1, ya, yb);
      }
      mfma_stage(xa, xb);
      if (kt + 1 >= nkt) break;
      // stage kt+1 in y; publish kt+2, read it into x, MFMA y
      if (kt + 2 < nkt) {
        const int ahead = nkt - 3 - kt;
        if (ahead >= 2)
          asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
        else if (ahead == 1)
          asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
        else
          asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (kt + 5 < nkt) issue(kt + 5, (kt + 1) & 3);
        read_stage(kt + 2, xa, xb);
      }
      mfma_stage(ya, yb);
    }
  }

  // the epilogue of gemm256_kernel, word for word: as a shared helper it compiles to other
  // instructions in the VERIFY kernels, so both keep their copy
  unsigned bad = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = tn * G_BN + wn * 64 + j * 32 + lr;
      const int rbase = tm * G_BM + wm * 128 + i * 32 + 4 * lh;
      if (VERIFY) {
        const int c7 = col % 7;
        const int r5 = rbase % 5;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int rr = r5 + (r & 3) + 8 * (r >> 2);
          rr %= 5;
          bad += acc[i][j][r] != expect[rr * 7 + c7];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) C[(size_t)(rbase + (r & 3) + 8 * (r >> 2)) * N + col] = acc[i][j][r];
      }
    }
  if (VERIFY) {
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
    if (lane == 0 && bad) {
      atomicAdd(err_total, bad);
      if (err_xcd) atomicAdd(&err_xcd[xcc], bad);
    }
  }
  if (ts && lane == 0) ts_end(ts);
}

#include "gpu_probe_mx.h"  // the block-scaled kernels (FP8, BF8, FP6, BF6, MXFP4), on the tile helpers above
#include "gpu_probe_dense.h"  // the FP16 / INT8 kernels, on the same helpers and the ring above
#include "gpu_probe_fp.h"  // the FP32 / FP64 kernels, on the same helpers and the ring's constants
#include "gpu_probe_sparse.h"  // the 2:4 structured-sparsity kernels, on the same helpers and a ring of their own

__device__ __forceinline__ uint16_t small_int_bf16(int v) {
  // exact for |v| < 256: take the high half of the f32 bit pattern
  return (uint16_t)(__float_as_uint((float)v) >> 16);
}

// A[i][k] = ((3i + 7k) mod 5) - 2 ; Bt[j][k] = ((11j + 5k) mod 7) - 3   (asymmetric in i/j)
__global__ void fill_kernel(uint16_t* __restrict__ A, uint16_t* __restrict__ Bt, int M, int N, int K) {
  const size_t na = (size_t)M * K, nb = (size_t)N * K;
  for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < na + nb;
       idx += (size_t)gridDim.x * blockDim.x) {
    if (idx < na) {
      const int i = (int)(idx / K), k = (int)(idx % K);
      A[idx] = small_int_bf16((int)(((long)i * 3 + (long)k * 7) % 5) - 2);
    } else {
      const size_t o = idx - na;
      const int j = (int)(o / K), k = (int)(o % K);
      Bt[o] = small_int_bf16((int)(((long)j * 11 + (long)k * 5) % 7) - 3);
    }
  }
}

__global__ void verify_kernel(const float* __restrict__ C, int M, int N, int K, const int* __restrict__ tile_xcd,
                              unsigned* __restrict__ err_total, unsigned* __restrict__ err_xcd) {
  const int q = K / 35, rem = K - q * 35;
  const size_t total = (size_t)M * N;
  const int tiles_n = N / BN;
  for (size_t base = blockIdx.x * (size_t)blockDim.x; base < total; base += (size_t)gridDim.x * blockDim.x) {
    const size_t idx = base + threadIdx.x;
    bool bad = false;
    if (idx < total) {
      const int i = (int)(idx / N), j = (int)(idx - (size_t)i * N);
      // probe_expect(i % 5, j % 7, K) with q and rem hoisted and the loop unrolled (a call
      // to it compiles to other instructions here)
      const int ia = (i % 5) * 3 % 5, jb = (j % 7) * 11 % 7;
      int s = 0;
#pragma unroll
      for (int r = 0; r < 35; ++r) {
        int a = ia + (r * 7) % 5;
        a = (a >= 5 ? a - 5 : a) - 2;
        int b = jb + (r * 5) % 7;
        b = (b >= 7 ? b - 7 : b) - 3;
        s += (q + (r < rem ? 1 : 0)) * a * b;
      }
      bad = C[idx] != (float)s;
      if (bad && err_xcd && tile_xcd) atomicAdd(&err_xcd[tile_xcd[(i / BM) * tiles_n + j / BN] & 7], 1u);
    }
    const unsigned long long m = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(err_total, (unsigned)__popcll(m));
  }
}

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}

// the 16 bytes of pattern element i
__device__ __forceinline__ u32x4 pattern16(size_t i, uint32_t seed) {
  const uint32_t b = (uint32_t)(i * 4) ^ seed;
  u32x4 v;
  v.x = mix32(b);
  v.y = mix32(b + 1);
  v.z = mix32(b + 2);
  v.w = mix32(b + 3);
  return v;
}

// this workgroup's slab [lo, hi) of n elements: equal slabs, a multiple of 1024 elements long
struct Slab {
  size_t lo, hi;
};
__device__ __forceinline__ Slab slab_of(size_t n) {
  const size_t per = ((n + gridDim.x - 1) / gridDim.x + 1023) & ~(size_t)1023;
  const size_t lo = blockIdx.x * per;
  return {lo, lo + per < n ? lo + per : n};
}

// Pattern sweeps: each workgroup owns one contiguous slab of the buffer (measured on
// MI355X, 1 GiB: 5.9 TB/s for slabs vs 4.1 TB/s for a grid-stride loop of the same
// stores; sequential DRAM pages per CU), 4 × 16 B per lane per iteration so every wave
// keeps 4 KiB of stores in flight.
template <bool NT>
__global__ __launch_bounds__(256) void hbm_write_kernel(u32x4* __restrict__ buf, size_t n, uint32_t seed,
                                                        const uint32_t* __restrict__ seedp = nullptr,
                                                        unsigned long long* __restrict__ ts = nullptr) {
  if (seedp) seed = *seedp;  // graph replays: the seed lives on the device
  if (ts && threadIdx.x == 0 && blockIdx.x < TS_EDGE) ts_begin(ts);
  const auto [lo, hi] = slab_of(n);
  for (size_t base = lo + threadIdx.x; base < hi; base += 4 * 256) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const size_t i = base + u * 256;
      if (i < hi) {
        const u32x4 v = pattern16(i, seed);
        if (NT)
          __builtin_nontemporal_store(v, &buf[i]);
        else
          buf[i] = v;
      }
    }
  }
}

// write-path variants for A/B measurement (odh_hbm_write_variant):
//   1: each wave stores 4 consecutive KiB per iteration (4 × 1 KiB instructions in flight)
//   2: each workgroup owns one contiguous slab (sequential DRAM pages per CU)
//   3: constant data (no pattern math: the store-path ceiling)
template <int V>
__global__ __launch_bounds__(256) void hbm_write_variant_kernel(u32x4* __restrict__ buf, size_t n, uint32_t seed) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (V == 1) {
    const size_t waves = (size_t)gridDim.x * 4;
    for (size_t w = (size_t)blockIdx.x * 4 + wave; w * 256 < n; w += waves) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const size_t i = w * 256 + u * 64 + lane;
        if (i < n) {
          const u32x4 v = pattern16(i, seed);
          buf[i] = v;
        }
      }
    }
  } else if (V == 2) {
    const size_t per = (n + gridDim.x - 1) / gridDim.x;
    const size_t lo = blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    for (size_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
      const u32x4 v = pattern16(i, seed);
      buf[i] = v;
    }
  } else {
    u32x4 v;
    v.x = v.y = v.z = v.w = seed;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
      buf[i] = v;
  }
}

__global__ __launch_bounds__(256) void hbm_check_kernel(const u32x4* __restrict__ buf, size_t n, uint32_t seed,
                                                        unsigned long long* __restrict__ err,
                                                        const uint32_t* __restrict__ seedp = nullptr,
                                                        unsigned long long* __restrict__ ts = nullptr) {
  if (seedp) seed = *seedp;
  const auto [lo, hi] = slab_of(n);
  unsigned local = 0;
  for (size_t base = lo + threadIdx.x; base < hi; base += 4 * 256) {
    u32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // all four loads in flight before the compares
      const size_t i = base + u * 256;
      if (i < hi) v[u] = __builtin_nontemporal_load(&buf[i]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const size_t i = base + u * 256;
      if (i < hi) {
        const uint32_t b = (uint32_t)(i * 4) ^ seed;
        local += (v[u].x != mix32(b)) + (v[u].y != mix32(b + 1)) + (v[u].z != mix32(b + 2)) +
                 (v[u].w != mix32(b + 3));
      }
    }
  }
  // wave reduction (64 lanes), one atomic per wave
  for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off, 64);
  if ((threadIdx.x & 63) == 0 && local) atomicAdd(err, (unsigned long long)local);
  if (ts && (threadIdx.x & 63) == 0 && blockIdx.x + TS_EDGE >= gridDim.x) ts_end(ts);
}

// read-path variants for A/B measurement (odh_hbm_check_variant): NT = nontemporal loads,
// U = 16-byte loads in flight per lane per iteration
template <bool NT, int U>
__global__ __launch_bounds__(256) void hbm_check_variant_kernel(const u32x4* __restrict__ buf, size_t n,
                                                                uint32_t seed, unsigned long long* __restrict__ err) {
  const auto [lo, hi] = slab_of(n);
  unsigned local = 0;
  for (size_t base = lo + threadIdx.x; base < hi; base += U * 256) {
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + u * 256;
      if (i < hi) v[u] = NT ? __builtin_nontemporal_load(&buf[i]) : buf[i];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + u * 256;
      if (i < hi) {
        const uint32_t b = (uint32_t)(i * 4) ^ seed;
        local += (v[u].x != mix32(b)) + (v[u].y != mix32(b + 1)) + (v[u].z != mix32(b + 2)) +
                 (v[u].w != mix32(b + 3));
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off, 64);
  if ((threadIdx.x & 63) == 0 && local) atomicAdd(err, (unsigned long long)local);
}

// every 32-bit word of buf equal to `expect` (the RCCL all-reduce result check)
__global__ __launch_bounds__(256) void const_check_kernel(const u32x4* __restrict__ buf, size_t n, uint32_t expect,
                                                          unsigned long long* __restrict__ err) {
  const auto [lo, hi] = slab_of(n);
  unsigned local = 0;
  for (size_t i = lo + threadIdx.x; i < hi; i += 256) {
    const u32x4 v = __builtin_nontemporal_load(&buf[i]);
    local += (v.x != expect) + (v.y != expect) + (v.z != expect) + (v.w != expect);
  }
  for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off, 64);
  if ((threadIdx.x & 63) == 0 && local) atomicAdd(err, (unsigned long long)local);
}

__global__ __launch_bounds__(256) void busy_kernel(float* __restrict__ out, int iters) {
  const int lane = threadIdx.x & 63;
  bf16x8 a, b;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    a[e] = (__bf16)(float)((lane + e) & 3);
    b[e] = (__bf16)(float)((lane * 3 + e) & 3);
  }
  f32x16 acc0 = {}, acc1 = {}, acc2 = {}, acc3 = {};
  for (int i = 0; i < iters; ++i) {
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b, a, acc1, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, a, acc2, 0, 0, 0);
    acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b, b, acc3, 0, 0, 0);
  }
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) s += acc0[r] + acc1[r] + acc2[r] + acc3[r];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

int grid_for(size_t n, int per_block) {
  size_t g = (n + per_block - 1) / per_block;
  if (g > 4096) g = 4096;  // 16 × 256 CUs of grid-stride work
  if (g < 1) g = 1;
  return (int)g;
}

#include "gpu_probe_cvt.h"  // the converter kernels (FP8, BF8, FP6, BF6, FP4, bf16), on xcc_id and the sweep's slabs
#include "gpu_probe_lds.h"  // the LDS, its transposing reads, the lane exchanges and the transposer of packed codes
#include "gpu_probe_m16.h"  // the 16×16 matrix-core shapes (bf16, f16, i8, FP8, MXFP4), on the tile helpers, ring and tables above

}  // namespace

extern "C" {

int odh_gemm_shape_ok(int M, int N, int K) {
  return M > 0 && N > 0 && K > 0 && M % BM == 0 && N % BN == 0 && K % BK == 0;
}

const char* odh_error_string(int code) { return hipGetErrorString((hipError_t)code); }

// Load this library's code object on the current device without launching anything: the
// runtime loads a module at its first kernel launch (or attribute query), tens of ms of host
// work that the start-up probe overlaps with its allocation (probe_cli.cpp).  The kernels
// the probe launches are queried; one query loads the whole code object.
int odh_probe_preload() {
  hipFuncAttributes a;
  for (const void* f : {(const void*)fill_kernel, (const void*)gemm256d_kernel<true>,
                        (const void*)hbm_write_kernel<false>, (const void*)hbm_check_kernel}) {
    const hipError_t e = hipFuncGetAttributes(&a, f);
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

int odh_probe_fill(void* A, void* Bt, int M, int N, int K, hipStream_t stream) {
  if (!odh_gemm_shape_ok(M, N, K)) return (int)hipErrorInvalidValue;
  const size_t n = (size_t)M * K + (size_t)N * K;
  fill_kernel<<<grid_for(n, 256), 256, 0, stream>>>((uint16_t*)A, (uint16_t*)Bt, M, N, K);
  return (int)hipGetLastError();
}

// the 128² two-buffer register-staged kernel, for shapes the 256² tile does not divide
// (exported on its own for A/B measurements and numerics tests of both kernels)
int odh_gemm_bf16_128(const void* A, const void* Bt, float* C, int M, int N, int K, int* tile_xcd, int* xcd_blocks,
                      hipStream_t stream) {
  if (!odh_gemm_shape_ok(M, N, K)) return (int)hipErrorInvalidValue;
  const int nwg = (M / BM) * (N / BN);
  gemm_bf16_kernel<<<nwg, THREADS, 0, stream>>>((const uint4*)A, (const uint4*)Bt, C, M, N, K, tile_xcd, xcd_blocks);
  return (int)hipGetLastError();
}

// A/B: the 256² kernel without fragment pipelining (variant 0), with it (variant 1), or the
// deep-pipelined BK=32 / 4-buffer ring (variant 2)
int odh_gemm_bf16_256_variant(const void* A, const void* Bt, float* C, int M, int N, int K, int variant,
                              hipStream_t stream) {
  if (!gemm256_ok(M, N, K)) return (int)hipErrorInvalidValue;
  const int nwg = gemm256_tiles(M, N);
  if (variant == 0)
    gemm256_kernel<false, false><<<nwg, G_THREADS, 0, stream>>>((const uint4*)A, (const uint4*)Bt, C, M, N, K,
                                                                 nullptr, nullptr, nullptr, nullptr);
  else if (variant == 2)
    gemm256d_kernel<false><<<nwg, G_THREADS, 0, stream>>>((const uint4*)A, (const uint4*)Bt, C, M, N, K,
                                                          nullptr, nullptr, nullptr, nullptr);
  else if (variant == 3)
    gemm256d_kernel<false, true><<<nwg, G_THREADS, 0, stream>>>((const uint4*)A, (const uint4*)Bt, C, M, N, K,
                                                                nullptr, nullptr, nullptr, nullptr);
  else
    gemm256_kernel<false, true><<<nwg, G_THREADS, 0, stream>>>((const uint4*)A, (const uint4*)Bt, C, M, N, K,
                                                                nullptr, nullptr, nullptr, nullptr);
  return (int)hipGetLastError();
}

// workgroups (= tiles) the GEMM launches for this shape: 256² tiles when they fit, else 128²
int odh_gemm_tiles(int M, int N, int K) {
  if (!odh_gemm_shape_ok(M, N, K)) return 0;
  return gemm256_ok(M, N, K) ? gemm256_tiles(M, N) : (M / BM) * (N / BN);
}

int odh_gemm_bf16(const void* A, const void* Bt, float* C, int M, int N, int K, int* tile_xcd, int* xcd_blocks,
                  hipStream_t stream) {
  if (!odh_gemm_shape_ok(M, N, K)) return (int)hipErrorInvalidValue;
  if (gemm256_ok(M, N, K)) {
    gemm256_kernel<false><<<gemm256_tiles(M, N), G_THREADS, 0, stream>>>(
        (const uint4*)A, (const uint4*)Bt, C, M, N, K, tile_xcd, xcd_blocks, nullptr, nullptr);
    return (int)hipGetLastError();
  }
  return odh_gemm_bf16_128(A, Bt, C, M, N, K, tile_xcd, xcd_blocks, stream);
}

int odh_probe_verify(const float* C, int M, int N, int K, const int* tile_xcd, unsigned* err_total,
                     unsigned* err_xcd, hipStream_t stream) {
  if (!odh_gemm_shape_ok(M, N, K)) return (int)hipErrorInvalidValue;
  verify_kernel<<<grid_for((size_t)M * N, 256), 256, 0, stream>>>(C, M, N, K, tile_xcd, err_total, err_xcd);
  return (int)hipGetLastError();
}

// probe GEMM with the check fused into the epilogue (operands from odh_probe_fill); the
// shape must take 256² tiles.  Mismatches go to err_total / err_xcd[XCC that computed them].
// Runs the deep-pipelined kernel (MI355X run 14, 4096³: 1104 TFLOP/s vs 996 for the
// 2-buffer BK=64 kernel, which stays exported as odh_probe_gemm_verify_2buf for A/B).
int odh_probe_gemm_verify(const void* A, const void* Bt, int M, int N, int K, int* tile_xcd, int* xcd_blocks,
                          unsigned* err_total, unsigned* err_xcd, hipStream_t stream) {
  if (!fused_probe_ok(M, N, K, err_total)) return (int)hipErrorInvalidValue;
  gemm256d_kernel<true><<<gemm256_tiles(M, N), G_THREADS, 0, stream>>>(
      (const uint4*)A, (const uint4*)Bt, nullptr, M, N, K, tile_xcd, xcd_blocks, err_total, err_xcd);
  return (int)hipGetLastError();
}

int odh_probe_gemm_verify_2buf(const void* A, const void* Bt, int M, int N, int K, int* tile_xcd, int* xcd_blocks,
                               unsigned* err_total, unsigned* err_xcd, hipStream_t stream) {
  if (!fused_probe_ok(M, N, K, err_total)) return (int)hipErrorInvalidValue;
  gemm256_kernel<true><<<gemm256_tiles(M, N), G_THREADS, 0, stream>>>(
      (const uint4*)A, (const uint4*)Bt, nullptr, M, N, K, tile_xcd, xcd_blocks, err_total, err_xcd);
  return (int)hipGetLastError();
}

// the same fused probe on the deep-pipelined kernel (A/B against odh_probe_gemm_verify)
// variant bit 0: cross-barrier fragment prefetch (XB); bits 1-2: tile grouping GM = 1, 2, 4, 8
int odh_probe_gemm_verify_deep(const void* A, const void* Bt, int M, int N, int K, int* tile_xcd, int* xcd_blocks,
                               unsigned* err_total, unsigned* err_xcd, int variant, hipStream_t stream) {
  if (!fused_probe_ok(M, N, K, err_total)) return (int)hipErrorInvalidValue;
  const int nwg = gemm256_tiles(M, N);
  const uint4 *a = (const uint4*)A, *b = (const uint4*)Bt;
#define ODH_DEEP(XB_, GM_)                                                                                  \
  gemm256d_kernel<true, XB_, GM_><<<nwg, G_THREADS, 0, stream>>>(a, b, nullptr, M, N, K, tile_xcd, xcd_blocks, \
                                                                 err_total, err_xcd)
  switch (variant) {
    case 0: ODH_DEEP(false, 1); break;
    case 1: ODH_DEEP(true, 1); break;
    case 2: ODH_DEEP(false, 2); break;
    case 3: ODH_DEEP(true, 2); break;
    case 4: ODH_DEEP(false, 4); break;
    case 5: ODH_DEEP(true, 4); break;
    case 6: ODH_DEEP(false, 8); break;
    case 7: ODH_DEEP(true, 8); break;
    default: return (int)hipErrorInvalidValue;
  }
#undef ODH_DEEP
  return (int)hipGetLastError();
}

int odh_hbm_write(void* buf, size_t bytes, uint32_t seed, int nontemporal, hipStream_t stream) {
  const size_t n = bytes / 16;
  if (n == 0) return (int)hipErrorInvalidValue;
  if (nontemporal)
    hbm_write_kernel<true><<<grid_for(n, 1024), 256, 0, stream>>>((u32x4*)buf, n, seed);
  else
    hbm_write_kernel<false><<<grid_for(n, 1024), 256, 0, stream>>>((u32x4*)buf, n, seed);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------ the probe as one hipGraph
//
// For the torch-side harness (ops/gpu.py::GpuProbe; the shipped odh-gpu-probe launches
// eagerly on the null stream).  A resident probe is launch-bound on the host side: a counter
// reset, the GEMM on one stream, the HBM write + check on a second, a fork/join and a 128-byte
// read-back — five launches and three stream operations per run.  odh_probe_graph_create captures
// them once (stream capture with an event fork/join, so the sweep and the GEMM still run
// concurrently) and odh_probe_graph_launch replays the whole probe with one launch.  A
// graph freezes kernel arguments, so the per-run HBM pattern seed lives on the device: the
// first node advances it (LCG) and the sweep kernels read it.

// first node: advance the seed and reset the counter block (one wave; no memset node)
__global__ void probe_seed_advance_kernel(uint32_t* seed, int* counters) {
  if (threadIdx.x < ODH_NCOUNT) counters[threadIdx.x] = 0;
  if (threadIdx.x == 0) *seed = *seed * 1664525u + 1013904223u;
}

struct ProbeGraph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  hipStream_t s0 = nullptr, s1 = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
};

static void probe_graph_free(ProbeGraph* g) {
  if (!g) return;
  // teardown: errors here have nothing left to undo
  if (g->exec) (void)hipGraphExecDestroy(g->exec);
  if (g->graph) (void)hipGraphDestroy(g->graph);
  if (g->fork) (void)hipEventDestroy(g->fork);
  if (g->join) (void)hipEventDestroy(g->join);
  if (g->s0) (void)hipStreamDestroy(g->s0);
  if (g->s1) (void)hipStreamDestroy(g->s1);
  delete g;
}

// counters: the counter block on the device in the graph layout of gpu_probe.h (the spans are
// ts_begin / ts_end pairs); host: the same size, pinned; seed: one u32 on the device
int odh_probe_graph_create(const void* A, const void* Bt, int M, int N, int K, int* tile_xcd, int* counters,
                           void* hbm, size_t hbm_bytes, uint32_t* seed, int* host, int serial, void** out) {
  if (out) *out = nullptr;  // whatever the outcome, the caller holds no stale handle
  if (!out || !gemm256_ok(M, N, K) || hbm_bytes < 16) return (int)hipErrorInvalidValue;
  ProbeGraph* g = new ProbeGraph();
  hipError_t e = hipStreamCreateWithFlags(&g->s0, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&g->s1, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&g->fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&g->join, hipEventDisableTiming);
  if (e == hipSuccess) e = hipStreamBeginCapture(g->s0, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) {
    probe_graph_free(g);
    return (int)e;
  }
  const size_t n = hbm_bytes / 16;
  unsigned* c = (unsigned*)counters;
  hipError_t cap = hipSuccess;  // first error while capturing (the capture is still ended)
  auto chk = [&](hipError_t r) {
    if (cap == hipSuccess && r != hipSuccess) cap = r;
  };
  // serial: one chain of kernels on s0 (graph branches may not run concurrently on every
  // runtime; measured both ways by tools/probe_microbench.py --startup)
  hipStream_t sw = serial ? g->s0 : g->s1;
  probe_seed_advance_kernel<<<1, 64, 0, g->s0>>>(seed, counters);
  chk(hipGetLastError());
  if (!serial) {
    chk(hipEventRecord(g->fork, g->s0));
    chk(hipStreamWaitEvent(g->s1, g->fork, 0));
  }
  // the memory-bound sweep on the second stream, issued first; the GEMM's one workgroup
  // per CU co-resides with its waves
  unsigned long long* gemm_span = (unsigned long long*)(counters + ODH_SLOT_GRAPH_GEMM_SPAN);
  unsigned long long* sweep_span = (unsigned long long*)(counters + ODH_SLOT_GRAPH_SWEEP_SPAN);
  hbm_write_kernel<false><<<grid_for(n, 1024), 256, 0, sw>>>((u32x4*)hbm, n, 0u, seed, sweep_span);
  chk(hipGetLastError());
  hbm_check_kernel<<<grid_for(n, 1024), 256, 0, sw>>>(
      (const u32x4*)hbm, n, 0u, (unsigned long long*)(counters + ODH_SLOT_HBM_ERR), seed, sweep_span);
  chk(hipGetLastError());
  gemm256d_kernel<true><<<gemm256_tiles(M, N), G_THREADS, 0, g->s0>>>(
      (const uint4*)A, (const uint4*)Bt, nullptr, M, N, K, tile_xcd, counters + ODH_SLOT_XCD_BLOCKS,
      c + ODH_SLOT_GEMM_ERR, c + ODH_SLOT_ERR_XCD, gemm_span);
  chk(hipGetLastError());
  if (!serial) {
    chk(hipEventRecord(g->join, g->s1));
    chk(hipStreamWaitEvent(g->s0, g->join, 0));
  }
  chk(hipMemcpyAsync(host, counters, ODH_NCOUNT * sizeof(int), hipMemcpyDeviceToHost, g->s0));
  e = hipStreamEndCapture(g->s0, &g->graph);
  if (e == hipSuccess && cap != hipSuccess) e = cap;
  if (e == hipSuccess) e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    probe_graph_free(g);
    return (int)e;
  }
  *out = g;
  return 0;
}

int odh_probe_graph_launch(void* handle, hipStream_t stream) {
  if (!handle) return (int)hipErrorInvalidValue;
  return (int)hipGraphLaunch(((ProbeGraph*)handle)->exec, stream);
}

void odh_probe_graph_destroy(void* handle) { probe_graph_free((ProbeGraph*)handle); }

// wall_clock64() tick rate of a device in kHz (0 on error)
int odh_wall_clock_khz(int device) {
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess) return 0;
  return khz;
}

int odh_hbm_write_variant(void* buf, size_t bytes, uint32_t seed, int variant, int blocks, hipStream_t stream) {
  const size_t n = bytes / 16;
  if (n == 0 || blocks <= 0) return (int)hipErrorInvalidValue;
  if (variant == 1)
    hbm_write_variant_kernel<1><<<blocks, 256, 0, stream>>>((u32x4*)buf, n, seed);
  else if (variant == 2)
    hbm_write_variant_kernel<2><<<blocks, 256, 0, stream>>>((u32x4*)buf, n, seed);
  else
    hbm_write_variant_kernel<3><<<blocks, 256, 0, stream>>>((u32x4*)buf, n, seed);
  return (int)hipGetLastError();
}

int odh_hbm_check(const void* buf, size_t bytes, uint32_t seed, unsigned long long* err, hipStream_t stream) {
  const size_t n = bytes / 16;
  if (n == 0) return (int)hipErrorInvalidValue;
  hbm_check_kernel<<<grid_for(n, 1024), 256, 0, stream>>>((const u32x4*)buf, n, seed, err);
  return (int)hipGetLastError();
}

int odh_hbm_check_variant(const void* buf, size_t bytes, uint32_t seed, unsigned long long* err, int variant,
                          int blocks, hipStream_t stream) {
  const size_t n = bytes / 16;
  if (n == 0 || blocks <= 0) return (int)hipErrorInvalidValue;
  const u32x4* b = (const u32x4*)buf;
  switch (variant) {
    case 0: hbm_check_variant_kernel<true, 4><<<blocks, 256, 0, stream>>>(b, n, seed, err); break;
    case 1: hbm_check_variant_kernel<false, 4><<<blocks, 256, 0, stream>>>(b, n, seed, err); break;
    case 2: hbm_check_variant_kernel<true, 8><<<blocks, 256, 0, stream>>>(b, n, seed, err); break;
    case 3: hbm_check_variant_kernel<false, 8><<<blocks, 256, 0, stream>>>(b, n, seed, err); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

// dev may read peer's memory afterwards (idempotent; restores the caller's current device)
int odh_peer_enable(int dev, int peer) {
  if (dev == peer) return 0;
  int can = 0;
  hipError_t e = hipDeviceCanAccessPeer(&can, dev, peer);
  if (e != hipSuccess) return (int)e;
  if (!can) return (int)hipErrorPeerAccessUnsupported;
  int cur = 0;
  e = hipGetDevice(&cur);
  if (e != hipSuccess) return (int)e;
  e = hipSetDevice(dev);
  if (e != hipSuccess) return (int)e;
  e = hipDeviceEnablePeerAccess(peer, 0);
  if (e == hipErrorPeerAccessAlreadyEnabled) {
    (void)hipGetLastError();  // clear the sticky "already enabled" status
    e = hipSuccess;
  }
  hipError_t r = hipSetDevice(cur);
  return (int)(e != hipSuccess ? e : r);
}

int odh_const_check(const void* buf, size_t bytes, uint32_t expect, unsigned long long* err, hipStream_t stream) {
  const size_t n = bytes / 16;
  if (n == 0 || bytes % 16) return (int)hipErrorInvalidValue;
  const_check_kernel<<<grid_for(n, 1024), 256, 0, stream>>>((const u32x4*)buf, n, expect, err);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------ block-scaled formats (gpu_probe_mx.h)

// host only (no HIP call): how many of the 315 (i mod 15, j mod 21) classes expect 0 at this K,
// where the check cannot tell a right product from an all-zero one; -1 for a K that is not a
// positive multiple of 128
int odh_mx_zero_classes(int K) {
  if (K <= 0 || K % 128) return -1;
  int zeros = 0;
  for (int t = 0; t < MX_CLASSES; ++t) zeros += mx_expect4(t / MX_COLS, t % MX_COLS, K) == 0;
  return zeros;
}

// the probe operands encoded for fmt, their scales, and the 15 × 21 table of expected values
int odh_mx_fill(int fmt, void* A, void* Bt, void* sA, void* sBt, float* table, int M, int N, int K,
                hipStream_t stream) {
  if (!mx_ok(fmt, M, N, K) || !A || !Bt || !sA || !sBt || !table) return (int)hipErrorInvalidValue;
  const size_t n = ((size_t)M + N) * mx_row_bytes(fmt, K) + ((size_t)M + N) * (size_t)(K / 32);
  mx_fill_kernel<<<grid_for(n, 256), 256, 0, stream>>>(fmt, (uint8_t*)A, (uint8_t*)Bt, (uint8_t*)sA, (uint8_t*)sBt, M,
                                                      N, K);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  mx_table_kernel<<<MX_CLASSES, 64, 0, stream>>>(table, K);
  return (int)hipGetLastError();
}

// C[M][N] = (A ∘ sA) · (Bt ∘ sBt)ᵀ in fp32 for any codes and scales
int odh_mx_gemm(int fmt, const void* A, const void* Bt, const void* sA, const void* sBt, float* C, int M, int N, int K,
                hipStream_t stream) {
  if (!mx_ok(fmt, M, N, K) || !mx_aligned(A, Bt, sA, sBt) || !C) return (int)hipErrorInvalidValue;
  mx_launch_gemm<false>(fmt, gemm256_tiles(M, N), stream, (const uint4*)A, (const uint4*)Bt, (const uint8_t*)sA,
                        (const uint8_t*)sBt, C, (const float*)nullptr, N, K, (int*)nullptr, (int*)nullptr,
                        (unsigned*)nullptr, (unsigned*)nullptr);
  return (int)hipGetLastError();
}

// the same tiles with the check against odh_mx_fill's table fused into the epilogue; counters is
// a counter block of this format's own (ODH_SLOT_XCD_BLOCKS, ODH_SLOT_ERR_XCD, ODH_SLOT_GEMM_ERR)
int odh_mx_probe_gemm_verify(int fmt, const void* A, const void* Bt, const void* sA, const void* sBt,
                             const float* table, int M, int N, int K, int* tile_xcd, int* counters,
                             hipStream_t stream) {
  if (!mx_ok(fmt, M, N, K) || !mx_aligned(A, Bt, sA, sBt) || !table || !counters) return (int)hipErrorInvalidValue;
  unsigned* c = (unsigned*)counters;
  mx_launch_gemm<true>(fmt, gemm256_tiles(M, N), stream, (const uint4*)A, (const uint4*)Bt, (const uint8_t*)sA,
                       (const uint8_t*)sBt, (float*)nullptr, table, N, K, tile_xcd, counters + ODH_SLOT_XCD_BLOCKS,
                       c + ODH_SLOT_GEMM_ERR, c + ODH_SLOT_ERR_XCD);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------ FP16 / INT8 (gpu_probe_dense.h)

// the probe operands as halves, or as int8 times ODH_DT_I8_MUL_A / _B
int odh_dense_fill(int fmt, void* A, void* Bt, int M, int N, int K, hipStream_t stream) {
  if (!dense_ok(fmt, M, N, K) || !dense_aligned(A, Bt)) return (int)hipErrorInvalidValue;
  const size_t n = ((size_t)M + N) * (size_t)K;
  dense_fill_kernel<<<grid_for(n, 256), 256, 0, stream>>>(fmt, A, Bt, M, N, K);
  return (int)hipGetLastError();
}

// C[M][N] = A · Btᵀ for any operands: fp32 out of halves, int32 out of int8
int odh_dense_gemm(int fmt, const void* A, const void* Bt, void* C, int M, int N, int K, hipStream_t stream) {
  if (!dense_ok(fmt, M, N, K) || !dense_aligned(A, Bt) || !C || ((uintptr_t)C & 3)) return (int)hipErrorInvalidValue;
  dense_launch_gemm<false>(fmt, gemm256_tiles(M, N), stream, (const uint4*)A, (const uint4*)Bt, C, N, K, (int*)nullptr,
                           (int*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr);
  return (int)hipGetLastError();
}

// the same tiles on odh_dense_fill's operands with the check against the closed form fused into
// the epilogue; counters is a counter block of this format's own
int odh_dense_probe_gemm_verify(int fmt, const void* A, const void* Bt, int M, int N, int K, int* tile_xcd,
                                int* counters, hipStream_t stream) {
  if (!dense_ok(fmt, M, N, K) || !dense_aligned(A, Bt) || !counters) return (int)hipErrorInvalidValue;
  unsigned* c = (unsigned*)counters;
  dense_launch_gemm<true>(fmt, gemm256_tiles(M, N), stream, (const uint4*)A, (const uint4*)Bt, (void*)nullptr, N, K,
                          tile_xcd, counters + ODH_SLOT_XCD_BLOCKS, c + ODH_SLOT_GEMM_ERR, c + ODH_SLOT_ERR_XCD);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------ FP32 / FP64 (gpu_probe_fp.h)

// workgroups (= tiles) the fp kernels launch: 256×256 tiles for f32, 256×128 for f64 (0: bad shape)
int odh_fp_tiles(int fmt, int M, int N) {
  return fp_fmt_ok(fmt) && M > 0 && N > 0 && M % G_BM == 0 && N % G_BN == 0 ? fp_tiles(fmt, M, N) : 0;
}

// the probe operands as floats or doubles, times ODH_FP_*_MUL_A / _B
int odh_fp_fill(int fmt, void* A, void* Bt, int M, int N, int K, hipStream_t stream) {
  if (!fp_ok(fmt, M, N, K) || !fp_k_exact(fmt, K) || !dense_aligned(A, Bt)) return (int)hipErrorInvalidValue;
  const size_t n = ((size_t)M + N) * (size_t)K;
  fp_fill_kernel<<<grid_for(n, 256), 256, 0, stream>>>(fmt, A, Bt, M, N, K);
  return (int)hipGetLastError();
}

// C[M][N] = A · Btᵀ for any operands, in the operands' type
int odh_fp_gemm(int fmt, const void* A, const void* Bt, void* C, int M, int N, int K, hipStream_t stream) {
  if (!fp_ok(fmt, M, N, K) || !dense_aligned(A, Bt) || !C || ((uintptr_t)C & (uintptr_t)(fmt - 1)))
    return (int)hipErrorInvalidValue;
  fp_launch_gemm<false>(fmt, fp_tiles(fmt, M, N), stream, (const uint4*)A, (const uint4*)Bt, C, N, K, (int*)nullptr,
                        (int*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr);
  return (int)hipGetLastError();
}

// the same tiles on odh_fp_fill's operands with the check against the closed form fused into the
// epilogue; counters is a counter block of this format's own
int odh_fp_probe_gemm_verify(int fmt, const void* A, const void* Bt, int M, int N, int K, int* tile_xcd,
                             int* counters, hipStream_t stream) {
  if (!fp_ok(fmt, M, N, K) || !fp_k_exact(fmt, K) || !dense_aligned(A, Bt) || !counters)
    return (int)hipErrorInvalidValue;
  unsigned* c = (unsigned*)counters;
  fp_launch_gemm<true>(fmt, fp_tiles(fmt, M, N), stream, (const uint4*)A, (const uint4*)Bt, (void*)nullptr, N, K,
                       tile_xcd, counters + ODH_SLOT_XCD_BLOCKS, c + ODH_SLOT_GEMM_ERR, c + ODH_SLOT_ERR_XCD);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------ 2:4 structured sparsity (gpu_probe_sparse.h)

// host only (no HIP call): how many of the 210 (i mod 30, j mod 7) classes expect 0 at this K, where
// the check cannot tell a right product from an all-zero one; -1 for a K that is not a positive
// multiple of 64
int odh_sparse_zero_classes(int K) { return K <= 0 || K % 64 ? -1 : sparse_zero_classes(K); }

// the probe operands pruned 2:4 and encoded for fmt, their metadata, and the 30 × 7 table of
// expected sums
int odh_sparse_fill(int fmt, void* Ac, void* meta, void* Bt, int* table, int M, int N, int K, hipStream_t stream) {
  if (!sparse_ok(fmt, M, N, K) || !sparse_aligned(Ac, meta, Bt) || !table || sparse_zero_classes(K) != 0)
    return (int)hipErrorInvalidValue;
  const size_t n = (size_t)M * (size_t)(K / 8) + (size_t)N * (size_t)K;
  sparse_fill_kernel<<<grid_for(n, 256), 256, 0, stream>>>(fmt, Ac, (uint8_t*)meta, Bt, M, N, K);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  sparse_table_kernel<<<ODH_SP_CLASSES, 64, 0, stream>>>(table, K);
  return (int)hipGetLastError();
}

// C[M][N] = A · Btᵀ for any compressed A with valid metadata and any Bt: fp32, or int32 out of int8
int odh_sparse_gemm(int fmt, const void* Ac, const void* meta, const void* Bt, void* C, int M, int N, int K,
                    hipStream_t stream) {
  if (!sparse_ok(fmt, M, N, K) || !sparse_aligned(Ac, meta, Bt) || !C || ((uintptr_t)C & 3))
    return (int)hipErrorInvalidValue;
  sparse_launch_gemm<false>(fmt, gemm256_tiles(M, N), stream, (const uint4*)Ac, (const uint32_t*)meta,
                            (const uint4*)Bt, C, (const int*)nullptr, N, K, (int*)nullptr, (int*)nullptr,
                            (unsigned*)nullptr, (unsigned*)nullptr);
  return (int)hipGetLastError();
}

// the same tiles on odh_sparse_fill's operands with the check against its table fused into the
// epilogue; counters is a counter block of this format's own
int odh_sparse_probe_gemm_verify(int fmt, const void* Ac, const void* meta, const void* Bt, const int* table, int M,
                                 int N, int K, int* tile_xcd, int* counters, hipStream_t stream) {
  if (!sparse_ok(fmt, M, N, K) || !sparse_aligned(Ac, meta, Bt) || !table || !counters ||
      sparse_zero_classes(K) != 0)
    return (int)hipErrorInvalidValue;
  unsigned* c = (unsigned*)counters;
  sparse_launch_gemm<true>(fmt, gemm256_tiles(M, N), stream, (const uint4*)Ac, (const uint32_t*)meta,
                           (const uint4*)Bt, (void*)nullptr, table, N, K, tile_xcd, counters + ODH_SLOT_XCD_BLOCKS,
                           c + ODH_SLOT_GEMM_ERR, c + ODH_SLOT_ERR_XCD);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------ converters (gpu_probe_cvt.h)

// host only (no HIP call): the cases of a format's family (0: no such format), and cases [first, first + n)
unsigned odh_cvt_family_size(int fmt) { return cvt_fmt_ok(fmt) ? cvt_family_size(fmt) : 0u; }

int odh_cvt_family(int fmt, unsigned first, unsigned n, uint32_t* x, uint32_t* scale, uint32_t* expect) {
  if (!cvt_fmt_ok(fmt) || !x || !scale || !expect || first > cvt_family_size(fmt) || n > cvt_family_size(fmt) - first)
    return -1;
  for (unsigned i = 0; i < n; ++i) {
    const CvtCase c = cvt_case(fmt, first + i);
    x[i] = c.x;
    scale[i] = c.scale | c.sel << 8;
    expect[i] = c.expect;
  }
  return 0;
}

// the table the fused check reads its scale bytes from (bf16: its exponent fields)
int odh_cvt_fill(int fmt, void* scale_table, hipStream_t stream) {
  if (!cvt_fmt_ok(fmt) || !scale_table) return (int)hipErrorInvalidValue;
  cvt_fill_kernel<<<1, ODH_CVT_TABLE, 0, stream>>>(fmt, (uint8_t*)scale_table);
  return (int)hipGetLastError();
}

// the bare instruction with the caller's scales (none for bf16)
int odh_cvt_encode(int fmt, const float* x, const void* scales, void* codes, long rows, long K, hipStream_t stream) {
  if (!cvt_rows_ok(fmt, x, codes, rows, K) || (cvt_scaled(fmt) && !scales)) return (int)hipErrorInvalidValue;
  const size_t n = cvt_pieces(fmt, rows, K);
  cvt_launch_rows<false>(fmt, grid_for(n, 1024), stream, (const cvt_f4*)x, n, (const uint8_t*)scales, codes,
                         (uint8_t*)nullptr);
  return (int)hipGetLastError();
}

// OCP MX: the scales by the rule, the codes saturating (bf16: the plain conversion, scales_out unused)
int odh_cvt_quantize(int fmt, const float* x, void* codes, void* scales_out, long rows, long K, hipStream_t stream) {
  if (!cvt_rows_ok(fmt, x, codes, rows, K) || (cvt_scaled(fmt) && !scales_out)) return (int)hipErrorInvalidValue;
  const size_t n = cvt_pieces(fmt, rows, K);
  cvt_launch_rows<true>(fmt, grid_for(n, 1024), stream, (const cvt_f4*)x, n, (const uint8_t*)nullptr, codes,
                        (uint8_t*)scales_out);
  return (int)hipGetLastError();
}

// every case of the family on every SIMD, against odh_cvt_fill's table; counters is a counter block of this
// format's own (ODH_SLOT_XCD_BLOCKS, ODH_SLOT_ERR_XCD, ODH_SLOT_GEMM_ERR)
int odh_cvt_probe_verify(int fmt, const void* scale_table, int* counters, hipStream_t stream) {
  if (!cvt_fmt_ok(fmt) || !scale_table || !counters) return (int)hipErrorInvalidValue;
  unsigned* c = (unsigned*)counters;
  cvt_launch_probe(fmt, stream, (const uint8_t*)scale_table, counters + ODH_SLOT_XCD_BLOCKS, c + ODH_SLOT_GEMM_ERR,
                   c + ODH_SLOT_ERR_XCD);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------ LDS step (gpu_probe_lds.h)

// host only (no HIP call): elements compared per launch, and of those the ones that use the key dword of a table byte
unsigned long long odh_lds_cases(int check) {
  return lds_check_ok(check) ? lds_block_cases(check, -1) * ODH_LDS_BLOCKS : 0ull;
}

unsigned long long odh_lds_fault_count(int check, int table_byte) {
  if (!lds_check_ok(check) || table_byte < 0 || table_byte >= ODH_LDS_TABLE) return 0ull;
  return lds_block_cases(check, table_byte / 4) * ODH_LDS_BLOCKS;
}

int odh_lds_fill(int check, void* table, hipStream_t stream) {
  if (!lds_check_ok(check) || !table || ((uintptr_t)table & 3)) return (int)hipErrorInvalidValue;
  lds_fill_kernel<<<1, ODH_LDS_TABLE / 4, 0, stream>>>(check, (uint32_t*)table);
  return (int)hipGetLastError();
}

// a fused check against odh_lds_fill's table; counters is a counter block of this check's own with the CU
// bitmap behind it (ODH_NCOUNT + ODH_LDS_CU_WORDS dwords)
int odh_lds_probe_verify(int check, const void* table, int* counters, hipStream_t stream) {
  if (!lds_check_ok(check) || !table || ((uintptr_t)table & 3) || !counters) return (int)hipErrorInvalidValue;
  unsigned* c = (unsigned*)counters;
  lds_launch_probe(check, stream, (const uint32_t*)table, counters + ODH_SLOT_XCD_BLOCKS, c + ODH_SLOT_GEMM_ERR,
                   c + ODH_SLOT_ERR_XCD, c + ODH_NCOUNT);
  return (int)hipGetLastError();
}

int odh_lds_tr_read(int check, const void* image, unsigned bytes, const uint32_t* lane_addr, void* out,
                    hipStream_t stream) {
  const bool raw = check >= ODH_LDS_TR_RAW;
  if (raw) check -= ODH_LDS_TR_RAW;
  if (!lds_is_tr(check) || !image || !lane_addr || !out || bytes == 0 || bytes > 65536 || bytes % 4 ||
      ((uintptr_t)image & 3) || ((uintptr_t)out & 3))
    return (int)hipErrorInvalidValue;
  const LdsTr s = lds_tr_spec(check);
  LdsLaneAddr a;
  for (int l = 0; l < 64; ++l) {
    a.a[l] = lane_addr[l];
    if (a.a[l] > bytes || 4u * s.words > bytes - a.a[l] || (!raw && a.a[l] % s.align)) return (int)hipErrorInvalidValue;
  }
  lds_launch_tr_read(check, (bytes + 15u) & ~15u, stream, (const uint32_t*)image, bytes, a, (uint32_t*)out);
  return (int)hipGetLastError();
}

int odh_lds_xlane(int op, int arg, const uint32_t* in, uint32_t* out, hipStream_t stream) {
  if (op < 0 || op >= LDS_XL_OPS || arg < 0 || arg >= lds_xl_args(op) || !in || !out) return (int)hipErrorInvalidValue;
  lds_xlane_one_kernel<<<1, 64, 0, stream>>>(op, arg, in, out);
  return (int)hipGetLastError();
}

// packed codes [R][C] to [C][R]; the format and the shape are checked before the pointers
int odh_transpose_codes(int fmt, const void* src, void* dst, long R, long C, hipStream_t stream) {
  if (!lds_tc_ok(fmt) || R <= 0 || C <= 0 || R % LDS_TC_TILE || C % LDS_TC_TILE || R > (1L << 40) / C ||
      (R / LDS_TC_TILE) * (C / LDS_TC_TILE) > 0x7FFFFFFFL || !src || !dst || ((uintptr_t)src & 15) ||
      ((uintptr_t)dst & 15) || src == dst)
    return (int)hipErrorInvalidValue;
  lds_launch_transpose(fmt, (unsigned)((R / LDS_TC_TILE) * (C / LDS_TC_TILE)), stream, (const unsigned char*)src,
                       (unsigned char*)dst, R, C);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------ 16×16 shapes (gpu_probe_m16.h)

// C[M][N] = A · Btᵀ for any operands (fp8, fp4: (A ∘ sA) · (Bt ∘ sBt)ᵀ for any codes and scales)
int odh_m16_gemm(int fmt, const void* A, const void* Bt, const void* sA, const void* sBt, void* C, int M, int N, int K,
                 hipStream_t stream) {
  if (!m16_ok(fmt, M, N, K) || !m16_aligned(fmt, A, Bt, sA, sBt) || !C || ((uintptr_t)C & 3))
    return (int)hipErrorInvalidValue;
  m16_launch_gemm<false>(fmt, gemm256_tiles(M, N), stream, (const uint4*)A, (const uint4*)Bt, (const uint8_t*)sA,
                         (const uint8_t*)sBt, C, (const float*)nullptr, N, K, (int*)nullptr, (int*)nullptr,
                         (unsigned*)nullptr, (unsigned*)nullptr);
  return (int)hipGetLastError();
}

// the same tiles on the operands of odh_probe_fill (bf16), odh_dense_fill (f16, i8) or odh_mx_fill (fp8, fp4, with
// its table) with the check fused into the epilogue; counters is a counter block of this format's own
int odh_m16_probe_gemm_verify(int fmt, const void* A, const void* Bt, const void* sA, const void* sBt,
                              const float* table, int M, int N, int K, int* tile_xcd, int* counters,
                              hipStream_t stream) {
  if (!m16_ok(fmt, M, N, K) || !m16_aligned(fmt, A, Bt, sA, sBt) || (table != nullptr) != m16_scaled(fmt) || !counters)
    return (int)hipErrorInvalidValue;
  unsigned* c = (unsigned*)counters;
  m16_launch_gemm<true>(fmt, gemm256_tiles(M, N), stream, (const uint4*)A, (const uint4*)Bt, (const uint8_t*)sA,
                        (const uint8_t*)sBt, (void*)nullptr, table, N, K, tile_xcd, counters + ODH_SLOT_XCD_BLOCKS,
                        c + ODH_SLOT_GEMM_ERR, c + ODH_SLOT_ERR_XCD);
  return (int)hipGetLastError();
}

// one wave, one instruction on a zero accumulator
int odh_m16_one(int fmt, const uint32_t* a, const uint32_t* b, const uint32_t* sa, const uint32_t* sb, int opsel_a,
                int opsel_b, void* d, hipStream_t stream) {
  if (!m16_fmt_ok(fmt) || !m16_aligned(fmt, a, b, sa, sb) || !d || ((uintptr_t)d & 3) || opsel_a < 0 || opsel_a > 3 ||
      opsel_b < 0 || opsel_b > 3)
    return (int)hipErrorInvalidValue;
  uint32_t* out = (uint32_t*)d;
  switch (fmt) {
    case ODH_M16_BF16: m16_one_kernel<ODH_M16_BF16><<<1, 64, 0, stream>>>(a, b, sa, sb, opsel_a, opsel_b, out); break;
    case ODH_M16_F16: m16_one_kernel<ODH_M16_F16><<<1, 64, 0, stream>>>(a, b, sa, sb, opsel_a, opsel_b, out); break;
    case ODH_M16_I8: m16_one_kernel<ODH_M16_I8><<<1, 64, 0, stream>>>(a, b, sa, sb, opsel_a, opsel_b, out); break;
    case ODH_M16_FP8: m16_one_kernel<ODH_M16_FP8><<<1, 64, 0, stream>>>(a, b, sa, sb, opsel_a, opsel_b, out); break;
    default: m16_one_kernel<ODH_M16_FP4><<<1, 64, 0, stream>>>(a, b, sa, sb, opsel_a, opsel_b, out); break;
  }
  return (int)hipGetLastError();
}

int odh_busy(float* out, int blocks, int iters, hipStream_t stream) {
  if (blocks <= 0 || iters < 0) return (int)hipErrorInvalidValue;
  busy_kernel<<<blocks, 256, 0, stream>>>(out, iters);
  return (int)hipGetLastError();
}

}  // extern "C"
