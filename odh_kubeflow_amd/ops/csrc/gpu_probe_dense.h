// The start-up probe's FP16 and INT8 kernels: the two dense matrix-core paths beside bf16 that
// PyTorch-ROCm notebooks run on every day and the bf16 probe never touches:
//   v_mfma_f32_32x32x16_f16 — torch.autocast("cuda")'s default dtype, most checkpoints;
//   v_mfma_i32_32x32x32_i8  — W8A8 / torch._int_mm: integer multipliers and i32 accumulation,
//                             which share nothing with the float pipes.
//
// Included by gpu_probe.hip inside its anonymous namespace, after the 256² bf16 kernels: it
// uses their tile constants (G_BM, G_BN, G_THREADS, D_CH, D_NBUF, D_TILE, D_RING), dswz,
// xcd_tile, xcc_id and probe_expect.  gemm256d_kernel itself is not shared (a template over
// the dtype would change its codegen): this is its loop again.
//
// Public memory layout (odh_dense_* of gpu_probe.h): A is [M][K] and Bt is [N][K] row-major,
// IEEE half or int8; C is [M][N] row-major, fp32 for f16 and int32 for i8.
//
// Both instructions take 16 bytes of A and 16 bytes of B per lane, as the bf16 one does: lane l
// holds row (A) or column (B) l & 31, and lane half h = l >> 5 one half of the instruction's k.
// A stage is 256 rows × 64 bytes per operand (D_BK bf16 elements: 32 halves or 64 int8), consumed
// by two instructions per 32×32 fragment; instruction s of a stage reads 16-byte chunk
// 2s + (lane >> 5) of its row.  Neither path has scale operands and the k order inside an
// instruction is the same for A and B, so it cannot change a dot product: no operand map has to
// be fitted (tests/test_gpu_dense_exact.py holds the kernels to a host product on random,
// asymmetric integer data all the same; tests/test_gpu_lowprec_sweeps.py multiplies 256 half
// values by each other and holds the fused check to the exact mismatch count and per-XCD
// attribution of a changed element in every row and every column, and of a NaN and an inf).
// C/D is the 32x32 map of the bf16 kernels.
//
// Tile and pipeline: those of gemm256d_kernel — 512 threads, 8 waves as 2×4, 128×64 outputs per
// wave, the 4-buffer LDS-DMA ring with three stages in flight across counted-vmcnt raw
// barriers.  The kernel issues no vector load but the DMA, so the counts are the ring's own.

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;

__host__ __device__ inline bool dense_fmt_ok(int fmt) { return fmt == ODH_DT_F16 || fmt == ODH_DT_I8; }
// bytes per element, and elements per stage of 64 bytes per row
__host__ __device__ inline int dense_esize(int fmt) { return fmt == ODH_DT_I8 ? 1 : 2; }
__host__ __device__ inline int dense_bk(int fmt) { return 64 / dense_esize(fmt); }

// The probe's operand families, A[i][k] = ((3i + 7k) mod 5) - 2 and Bt[j][k] = ((11j + 5k) mod 7) - 3:
// as exact halves for f16; for i8 times the odd multipliers ODH_DT_I8_MUL_A / _B (-50 … 50 and
// -123 … 123), so that operand bits 0-6 and the sign all toggle, not just the low three bits.
// One thread per element.
__global__ void dense_fill_kernel(int fmt, void* __restrict__ A, void* __restrict__ Bt, int M, int N, int K) {
  const size_t na = (size_t)M * K, nb = (size_t)N * K;
  for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < na + nb;
       idx += (size_t)gridDim.x * blockDim.x) {
    const bool isa = idx < na;
    const size_t o = isa ? idx : idx - na;
    const long r = (long)(o / K), k = (long)(o % K);
    const int v = isa ? (int)((r * 3 + k * 7) % 5) - 2 : (int)((r * 11 + k * 5) % 7) - 3;
    if (fmt == ODH_DT_I8)
      ((int8_t*)(isa ? A : Bt))[o] = (int8_t)(v * (isa ? ODH_DT_I8_MUL_A : ODH_DT_I8_MUL_B));
    else
      ((_Float16*)(isa ? A : Bt))[o] = (_Float16)(float)v;
  }
}

template <int FMT>
struct DenseTypes;
template <>
struct DenseTypes<ODH_DT_F16> {
  using Frag = f16x8;
  using Acc = f32x16;
  using Out = float;
  static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ Out expect(int ia5, int jb7, int K) { return (float)probe_expect(ia5, jb7, K); }
};
template <>
struct DenseTypes<ODH_DT_I8> {
  using Frag = i32x4;
  using Acc = i32x16;
  using Out = int;
  static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) {
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0);
  }
  // exact in i32: |.| <= 1025 · 6 · K
  static __device__ __forceinline__ Out expect(int ia5, int jb7, int K) {
    return ODH_DT_I8_MUL_A * ODH_DT_I8_MUL_B * probe_expect(ia5, jb7, K);
  }
};

template <int FMT, bool VERIFY>
__global__ __launch_bounds__(G_THREADS, 1) void dense_gemm256_kernel(
    const uint4* __restrict__ A, const uint4* __restrict__ Bt, void* __restrict__ Cv, int N, int K,
    int* __restrict__ tile_xcd, int* __restrict__ xcd_blocks, unsigned* __restrict__ err_total,
    unsigned* __restrict__ err_xcd) {
  using T = DenseTypes<FMT>;
  using Frag = typename T::Frag;
  using Acc = typename T::Acc;
  using Out = typename T::Out;
  constexpr int ESIZE = FMT == ODH_DT_I8 ? 1 : 2;
  constexpr int BKE = 64 / ESIZE;          // elements per stage
  __shared__ uint4 lds[D_RING + 9];        // one array: the ring, then the 35 expected values
  Out* expect = reinterpret_cast<Out*>(lds + D_RING);
  static_assert(sizeof(Out) == 4 && 35 * sizeof(Out) <= 9 * sizeof(uint4), "the table fits behind the ring");

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
  if (VERIFY && tid < 35) expect[tid] = T::expect(tid / 7, tid % 7, K);

  const size_t kch = (size_t)(K / BKE) * D_CH;  // 16-byte chunks per global row
  const uint4* Ag = A + (size_t)tm * G_BM * kch;
  const uint4* Bg = Bt + (size_t)tn * G_BN * kch;

  // stage kt → ring slot b: wave w fills rows [32w, 32w + 32) of A and of B (16 rows per
  // instruction); 4 DMA instructions per thread per stage.  Lane l lands at LDS chunk
  // p = base + l, which holds K-chunk (p & 3) ^ swizzle of row p >> 2
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

  Acc acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

  const int nkt = K / BKE;
  const int lr = lane & 31, lh = lane >> 5;
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
    const int cur = kt & 3;
    const uint4* sa = lds + (cur * 2 + 0) * D_TILE;
    const uint4* sb = lds + (cur * 2 + 1) * D_TILE;
    // both instructions of the stage: lane half h reads chunk 2s + h of its row
    Frag af[2][4], bfr[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int c = 2 * s + lh;
#pragma unroll
      for (int i = 0; i < 4; ++i) af[s][i] = __builtin_bit_cast(Frag, sa[dswz(wm * 128 + i * 32 + lr, c)]);
#pragma unroll
      for (int j = 0; j < 2; ++j) bfr[s][j] = __builtin_bit_cast(Frag, sb[dswz(wn * 64 + j * 32 + lr, c)]);
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = T::mfma(af[s][i], bfr[s][j], acc[i][j]);
    __builtin_amdgcn_s_setprio(0);
  }
  // every DMA is retired (the last stage waited vmcnt(0)): an ordinary barrier publishes the table
  if (VERIFY) __syncthreads();

  // C/D map of 32x32: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  Out* C = static_cast<Out*>(Cv);
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
          const int rr = (r5 + (r & 3) + 8 * (r >> 2)) % 5;
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

// both formats' kernel on one argument list
template <bool VERIFY, typename... Args>
void dense_launch_gemm(int fmt, int nwg, hipStream_t stream, Args... args) {
  if (fmt == ODH_DT_I8)
    dense_gemm256_kernel<ODH_DT_I8, VERIFY><<<nwg, G_THREADS, 0, stream>>>(args...);
  else
    dense_gemm256_kernel<ODH_DT_F16, VERIFY><<<nwg, G_THREADS, 0, stream>>>(args...);
}

// host side: what the dense entry points take
bool dense_ok(int fmt, int M, int N, int K) {
  return dense_fmt_ok(fmt) && M > 0 && N > 0 && K > 0 && M % G_BM == 0 && N % G_BN == 0 && K % dense_bk(fmt) == 0;
}
bool dense_aligned(const void* a, const void* b) { return a && b && (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }
