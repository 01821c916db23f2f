// The start-up probe's FP32 and FP64 kernels: the two dtypes a notebook gets without asking for
// anything, on matrix-core instructions no other kernel here issues:
//   v_mfma_f32_32x32x2_f32 — torch's default dtype (gfx950 has no xf32 / TF32: an fp32 matmul is this);
//   v_mfma_f64_16x16x4_f64 — NumPy's, CuPy's and SciPy's default: its own multiplier array, two-VGPR
//                            accumulators and a C/D lane map of its own.
//
// Included by gpu_probe.hip inside its anonymous namespace, after gpu_probe_dense.h: it uses the
// ring constants of the 256² bf16 kernels (G_BM, G_THREADS, D_CH, D_NBUF, D_TILE), dswz, xcd_tile,
// xcc_id and probe_expect.  The loop is dense_gemm256_kernel's again (a shared template would
// change that kernel's codegen).
//
// Public memory layout (odh_fp_* of gpu_probe.h): A is [M][K] and Bt is [N][K] row-major float or
// double, 16-byte aligned; C is [M][N] row-major in the same type.  M and N are multiples of 256,
// K of one stage: 64 bytes of a row, 16 floats or 8 doubles.
//
// Lane maps.  Both instructions take ONE element of A and one of B per lane.
//   32x32x2 f32:  lane l holds A[row l & 31][k = l >> 5] and B[k = l >> 5][col l & 31]; a 64-byte
//     stage row is 8 instructions per 32×32 fragment.  Lane half h = l >> 5 reads the 16-byte
//     chunks h and h + 2 of its row (two ds_read_b128) and uses element e of them in instruction e
//     resp. 4 + e, so instruction e sums k = {e, 4 + e} and instruction 4 + e k = {8 + e, 12 + e}.
//     C/D is the 32x32 map of the bf16 kernels: col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
//   16x16x4 f64:  lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; a stage row
//     of 8 doubles is 2 instructions per 16×16 fragment.  Lane quarter q = l >> 4 reads chunk q of
//     its row (one ds_read_b128) and uses double e of it in instruction e, which sums k = {e, 2 + e,
//     4 + e, 6 + e}.  C/D: col = l & 15, row = (l >> 4) + 4 reg, reg 0..3 of two VGPRs each — NOT the
//     f32 16x16 map (row = 4 (l >> 4) + reg), with which the kernel runs clean and places 3 of 4
//     results in the wrong row.
// In both, A and B see the same k permutation inside a stage, so no dot product changes
// (tests/test_gpu_fp_exact.py holds both kernels to a host product on random asymmetric data).
//
// Tiles.  f32: the bf16 tile, 256×256 per workgroup, 512 threads as 2(M)×4(N) waves of 128×64
// outputs, acc[4][2] of 16 registers.  f64: that wave tile is 128 doubles per lane = 256 VGPRs of
// accumulator, the whole budget at 2 waves per SIMD, so the workgroup tile is 256×128: 4(M)×2(N)
// waves of 64×64 outputs, acc[4][4] of 4 doubles = 128 registers.  Its B stage is 128 rows, so a
// stage takes 3 DMA instructions per thread (f32: 4) and the ring 4 × 24 KiB (f32: 4 × 32 KiB); the
// counted vmcnt of the ring follows.  odh_fp_tiles is the workgroup count: (M/256)·(N/256) or
// (M/256)·(N/128).
//
// The kernels are MFMA-bound: an f32 stage is 64 instructions × 64 cycles per wave for 16 k, so the
// ring's depth is not what sets their speed; it is kept rather than adding a second pipeline.
//
// hipcc -O3 --offload-arch=gfx950 (ROCm 7.2), -Rpass-analysis=kernel-resource-usage; the accumulators
// are VGPRs, and 2 waves per SIMD is the workgroup's own 8 waves:
//                                VGPRs  AGPRs  LDS bytes  scratch  waves/SIMD
//   fp_gemm_kernel<F32, false>     196      0    131216        0           2
//   fp_gemm_kernel<F32, true>      198      0    131216        0           2
//   fp_gemm_kernel<F64, false>     176      0     98592        0           2
//   fp_gemm_kernel<F64, true>      178      0     98592        0           2
// LDS: 4 × 32 KiB + 144 B of table (f32), 4 × 24 KiB + 288 B (f64): one workgroup per CU.

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) double f64x2;
typedef __attribute__((ext_vector_type(4))) double f64x4;

__host__ __device__ inline bool fp_fmt_ok(int fmt) { return fmt == ODH_FP_F32 || fmt == ODH_FP_F64; }
// the format codes are the element sizes; elements per stage of 64 bytes per row; columns of a workgroup tile
__host__ __device__ inline int fp_bk(int fmt) { return 64 / fmt; }
__host__ __device__ inline int fp_bn(int fmt) { return fmt == ODH_FP_F64 ? 128 : 256; }

// Every partial sum of the probe operands below is an integer of magnitude <= 6 K MUL_A MUL_B
// (|a| <= 2 MUL_A, |b| <= 3 MUL_B): exact in the accumulator type, in any summation order, while
// that stays below 2^24 (f32) resp. 2^53 (f64).
constexpr long long FP_F32_UNIT = 6LL * ODH_FP_F32_MUL_A * ODH_FP_F32_MUL_B;
constexpr long long FP_F64_UNIT = 6LL * ODH_FP_F64_MUL_A * ODH_FP_F64_MUL_B;
static_assert(1024 * FP_F32_UNIT < (1LL << 24), "the f32 probe is exact at K = 1024");
static_assert(1024 * FP_F64_UNIT < (1LL << 53), "the f64 probe is exact at K = 1024");
__host__ inline bool fp_k_exact(int fmt, int K) {
  return fmt == ODH_FP_F64 ? K <= ((1LL << 53) - 1) / FP_F64_UNIT : K <= ((1LL << 24) - 1) / FP_F32_UNIT;
}

// The bf16 probe's operand families, A[i][k] = ((3i + 7k) mod 5) - 2 and Bt[j][k] = ((11j + 5k) mod 7) - 3,
// times the odd multipliers ODH_FP_*_MUL_A / _B (the INT8 path's idea): more than the low three
// mantissa bits toggle — 7 bits of an f32 operand, 21 of an f64 one, 41 of an f64 product.
// One thread per element.
__global__ void fp_fill_kernel(int fmt, void* __restrict__ A, void* __restrict__ Bt, int M, int N, int K) {
  const size_t na = (size_t)M * K, nb = (size_t)N * K;
  for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < na + nb;
       idx += (size_t)gridDim.x * blockDim.x) {
    const bool isa = idx < na;
    const size_t o = isa ? idx : idx - na;
    const long r = (long)(o / K), k = (long)(o % K);
    const int v = isa ? (int)((r * 3 + k * 7) % 5) - 2 : (int)((r * 11 + k * 5) % 7) - 3;
    if (fmt == ODH_FP_F64)
      ((double*)(isa ? A : Bt))[o] = (double)(v * (isa ? ODH_FP_F64_MUL_A : ODH_FP_F64_MUL_B));
    else
      ((float*)(isa ? A : Bt))[o] = (float)(v * (isa ? ODH_FP_F32_MUL_A : ODH_FP_F32_MUL_B));
  }
}

template <int FMT>
struct FpTypes;
template <>
struct FpTypes<ODH_FP_F32> {
  using Elem = float;
  using Vec = f32x4;   // a 16-byte chunk of a row
  using Acc = f32x16;
  static constexpr int FR = 32;                // fragment rows and columns
  static constexpr int WAVES_N = 4, NI = 4, NJ = 2;  // 2×4 waves of 128×64 outputs
  static constexpr int NS = 2;                 // chunks a lane reads per row and stage
  static constexpr int NR = 16;                // results per lane and fragment
  static __device__ __forceinline__ int chunk(int lane, int s) { return (lane >> 5) + 2 * s; }
  static __device__ __forceinline__ Acc mfma(Elem a, Elem b, Acc c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
  }
  // row of result register r in its fragment: row_lane + row_reg
  static __device__ __forceinline__ int row_lane(int lane) { return 4 * (lane >> 5); }
  static __device__ __forceinline__ int row_reg(int r) { return (r & 3) + 8 * (r >> 2); }
  // exact in fp32: |.| <= 1025 · 6 · K < 2^24
  static __device__ __forceinline__ Elem expect(int ia5, int jb7, int K) {
    return (float)(ODH_FP_F32_MUL_A * ODH_FP_F32_MUL_B * probe_expect(ia5, jb7, K));
  }
};
template <>
struct FpTypes<ODH_FP_F64> {
  using Elem = double;
  using Vec = f64x2;
  using Acc = f64x4;
  static constexpr int FR = 16;
  static constexpr int WAVES_N = 2, NI = 4, NJ = 4;  // 4×2 waves of 64×64 outputs
  static constexpr int NS = 1;
  static constexpr int NR = 4;
  static __device__ __forceinline__ int chunk(int lane, int) { return lane >> 4; }
  static __device__ __forceinline__ Acc mfma(Elem a, Elem b, Acc c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row_lane(int lane) { return lane >> 4; }
  static __device__ __forceinline__ int row_reg(int r) { return 4 * r; }
  // exact in fp64: |.| <= MUL_A · MUL_B · 6 · K < 2^53
  static __device__ __forceinline__ Elem expect(int ia5, int jb7, int K) {
    return (double)((long long)ODH_FP_F64_MUL_A * ODH_FP_F64_MUL_B * probe_expect(ia5, jb7, K));
  }
};

template <int FMT, bool VERIFY>
__global__ __launch_bounds__(G_THREADS, 1) void fp_gemm_kernel(
    const uint4* __restrict__ A, const uint4* __restrict__ Bt, void* __restrict__ Cv, int N, int K,
    int* __restrict__ tile_xcd, int* __restrict__ xcd_blocks, unsigned* __restrict__ err_total,
    unsigned* __restrict__ err_xcd) {
  using T = FpTypes<FMT>;
  using Elem = typename T::Elem;
  using Vec = typename T::Vec;
  using Acc = typename T::Acc;
  constexpr int FR = T::FR, NI = T::NI, NJ = T::NJ, NS = T::NS, NR = T::NR;
  constexpr int NE = 16 / sizeof(Elem);            // elements per chunk = instructions per chunk read
  constexpr int BKE = 64 / sizeof(Elem);           // elements per stage
  constexpr int BN = FR * NJ * T::WAVES_N;         // 256 (f32) or 128 (f64) columns per workgroup
  constexpr int WM = FR * NI, WN = FR * NJ;        // outputs per wave
  constexpr int NB = BN / 128;                     // DMA instructions per thread and stage for B (A: 2)
  constexpr int B_TILE = BN * D_CH;                // uint4 per B stage
  constexpr int STAGE = D_TILE + B_TILE;           // a ring slot: the A stage, then the B stage
  constexpr int RING = D_NBUF * STAGE;
  constexpr int TABLE = (35 * sizeof(Elem) + 15) / 16;
  static_assert(G_BM == WM * (G_THREADS / 64 / T::WAVES_N) && BN == (FMT == ODH_FP_F64 ? 128 : 256), "wave grid");
  __shared__ uint4 lds[RING + TABLE];  // one array: the ring, then the 35 expected values
  Elem* expect = reinterpret_cast<Elem*>(lds + RING);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int wm = w / T::WAVES_N, wn = w % T::WAVES_N;
  const int tiles_n = N / BN;
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
  const uint4* Bg = Bt + (size_t)tn * BN * kch;

  // stage kt → ring slot b: 16 rows per instruction; wave w fills rows [32w, 32w + 32) of A and
  // [16 NB w, 16 NB (w + 1)) of B.  Lane l lands at LDS chunk p = base + l, which holds K-chunk
  // (p & 3) ^ swizzle of row p >> 2
  auto issue = [&](int kt, int b) {
    uint4* la = lds + b * STAGE;
    uint4* lb = la + D_TILE;
#pragma unroll
    for (int i = 0; i < 2 + NB; ++i) {
      const bool isa = i < 2;
      const int base = isa ? (w * 2 + i) * 64 : (w * NB + i - 2) * 64;
      const int p = base + lane;
      const int row = p >> 2;
      const int c = (p & 3) ^ ((row >> 2) & 3);
      const size_t g = (size_t)row * kch + (size_t)kt * D_CH + c;
      __builtin_amdgcn_global_load_lds((isa ? Ag : Bg) + g, (isa ? la : lb) + base, 16, 0, 0);
    }
  };

  Acc acc[NI][NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < NR; ++r) acc[i][j][r] = 0;

  const int nkt = K / BKE;
  const int lr = lane & (FR - 1);
  issue(0, 0);
  if (nkt > 1) issue(1, 1);
  if (nkt > 2) issue(2, 2);
  for (int kt = 0; kt < nkt; ++kt) {
    // retire THIS wave's DMA of stage kt (younger stages stay in flight: 2 + NB instructions
    // each), then the barrier makes every wave's part visible and proves stage kt-1's slot is no
    // longer read
    const int ahead = nkt - 1 - kt;
    if (NB == 2) {
      if (ahead >= 2)
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else if (ahead == 1)
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      if (ahead >= 2)
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      else if (ahead == 1)
        asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    if (kt + 3 < nkt) issue(kt + 3, (kt + 3) & 3);
    const uint4* sa = lds + (kt & 3) * STAGE;
    const uint4* sb = sa + D_TILE;
    // the stage's chunks of this lane: NS per row, NE instructions each
    Vec af[NS][NI], bfr[NS][NJ];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int c = T::chunk(lane, s);
#pragma unroll
      for (int i = 0; i < NI; ++i) af[s][i] = __builtin_bit_cast(Vec, sa[dswz(wm * WM + i * FR + lr, c)]);
#pragma unroll
      for (int j = 0; j < NJ; ++j) bfr[s][j] = __builtin_bit_cast(Vec, sb[dswz(wn * WN + j * FR + lr, c)]);
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int e = 0; e < NE; ++e)
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j) acc[i][j] = T::mfma(af[s][i][e], bfr[s][j][e], acc[i][j]);
    __builtin_amdgcn_s_setprio(0);
  }
  // every DMA is retired (the last stage waited vmcnt(0)): an ordinary barrier publishes the table
  if (VERIFY) __syncthreads();

  Elem* C = static_cast<Elem*>(Cv);
  unsigned bad = 0;
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = tn * BN + wn * WN + j * FR + lr;
      const int rbase = tm * G_BM + wm * WM + i * FR + T::row_lane(lane);
      if (VERIFY) {
        const int c7 = col % 7;
        const int r5 = rbase % 5;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int rr = (r5 + T::row_reg(r)) % 5;
          bad += acc[i][j][r] != expect[rr * 7 + c7];
        }
      } else {
#pragma unroll
        for (int r = 0; r < NR; ++r) C[(size_t)(rbase + T::row_reg(r)) * N + col] = acc[i][j][r];
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
void fp_launch_gemm(int fmt, int nwg, hipStream_t stream, Args... args) {
  if (fmt == ODH_FP_F64)
    fp_gemm_kernel<ODH_FP_F64, VERIFY><<<nwg, G_THREADS, 0, stream>>>(args...);
  else
    fp_gemm_kernel<ODH_FP_F32, VERIFY><<<nwg, G_THREADS, 0, stream>>>(args...);
}

// host side: what the fp entry points take, and their workgroup count
bool fp_ok(int fmt, int M, int N, int K) {
  return fp_fmt_ok(fmt) && M > 0 && N > 0 && K > 0 && M % G_BM == 0 && N % G_BN == 0 && K % fp_bk(fmt) == 0;
}
int fp_tiles(int fmt, int M, int N) { return (M / G_BM) * (N / fp_bn(fmt)); }
