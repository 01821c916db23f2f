// The start-up probe's 16×16 kernels: the other shape of the matrix-core instructions, which
// torch.compile's GEMM and convolution templates, Triton's attention kernels and CK's small-tile
// kernels issue and no 32×32 check touches:
//   v_mfma_f32_16x16x32_bf16, v_mfma_f32_16x16x32_f16, v_mfma_i32_16x16x64_i8, and
//   v_mfma_scale_f32_16x16x128_f8f6f4 with e4m3 (FP8) or e2m1 (FP4) on both sides.
// Out of scope here: bf8, fp6 and bf6 in the 16x16x128 instruction, v_mfma_f32_16x16x4_f32, the
// 16×16 v_smfmac_* and the unscaled *_fp8_fp8 forms.
//
// Included by gpu_probe.hip inside its anonymous namespace, after the other kernel headers: it uses
// the tile constants (G_BM, G_BN, G_THREADS, D_CH, D_NBUF, D_TILE, D_RING), dswz, xcd_tile, xcc_id,
// probe_expect, the vector types of gpu_probe_dense.h and the MX table of gpu_probe_mx.h.
//
// Public memory layout (odh_m16_* of gpu_probe.h): A is [M][K] and Bt is [N][K] row-major; bf16 as
// odh_gemm_bf16, f16 and i8 as odh_dense_gemm, fp8 and fp4 as odh_mx_gemm with E8M0 scales
// [rows][K/32].  C is [M][N] fp32, int32 for i8.
//
// Operand maps, as measured on the MI355X with odh_m16_one (one instruction on a zero accumulator:
// a single non-zero at every (lane, element) of A against random B and of B against random A, and
// random integer operands; held by tests/mfma16_reference.py and tests/test_gpu_mfma16_exact.py).
// Lane l holds row (A) or column (B) r = l & 15 and, with g = l >> 4, one quarter of the
// instruction's k, ascending from the low bits of VGPR 0:
//   bf16, f16 (4 VGPRs): k = 8g … 8g+7;
//   i8 (4 VGPRs): k = 16g … 16g+15;
//   fp4 (4 VGPRs, the low four of the eight the builtin takes): the lane holds its own block,
//     k = 32g … 32g+31, two per byte with the even k in the low nibble;
//   fp8 (8 VGPRs): VGPRs 0-3 hold k = 16g … 16g+15, sixteen elements of block g >> 1, and
//     VGPRs 4-7 hold k = 64+16g … 64+16g+15, sixteen of block 2 + (g >> 1): each lane carries a
//     quarter of two blocks, neither of them (but for g = 0) the block whose scale it carries.
// Scales (fp8, fp4): byte `opsel` of the scale VGPR of lane l is the scale of row r's block g
// (k = 32g … 32g+31) in both formats and on both sides.  For fp4 that is the block the lane holds.
// For fp8 the hardware scales a lane's VGPRs 0-3 by the scale in lane r + 16 (g >> 1) and its
// VGPRs 4-7 by the one in lane r + 16 (2 + (g >> 1)): the 32x32x64 FP8 map (gpu_probe_mx.h) with
// four lane groups for two, not a lane's eight VGPRs as one block.  Measured with a single 1.0 at
// every fourth element of every lane against all ones, a distinct scale byte in every lane and
// every byte position, `opsel` 0-3 on each side; only the block of an element can be observed (A
// and B share the order of k), the order inside a block is the natural one by convention.
// C/D: col = lane & 15, row = 4 (lane >> 4) + reg, for every format.
//
// Tile: that of the 32×32 kernels, 256×256 outputs, 512 threads, 8 waves as 2×4, 128×64 outputs per
// wave = 8 × 4 fragments of 16×16, 128 accumulator registers.  Stages are 256 rows × 64 bytes per
// operand, staged by the swizzled global_load_lds of 16 bytes; lane l reads 16-byte chunk l >> 4
// of row l & 15 of its fragment, so one instruction's K is one stage row for bf16 (32 elements),
// f16 (32), i8 (64) and fp4 (128).
//   Dense (bf16, f16, i8): the 4-buffer counted-vmcnt ring of dense_gemm256_kernel.
//   Scaled (fp8, fp4): the two-buffer loop of mx_gemm256_kernel, the scale dwords (one per row and
//     instruction: its four blocks) as ordinary global loads one stage ahead.  FP8 needs 128 bytes
//     of a row per instruction: its stage is two 64-byte half-tiles per operand (bytes 0-63 and
//     64-127 of the stage row, each in the layout above: 128-byte rows staged as two halves), 64 KiB
//     per buffer; a lane's VGPRs 0-3 are chunk g of the first half-tile and its VGPRs 4-7 chunk g of
//     the second, so public k = 16g … and 64+16g …, as the map asks.  The A fragments are loaded and consumed
//     two at a time against the four B fragments, so 8 A + 4 B fragments of 8 VGPRs never live at once.
// The stage layout and its swizzle are the 32×32 kernels', made for 32 lanes reading 32 rows at one chunk; the
// 16-row, four-chunk read of these kernels is 2-way bank conflicted on it (SQ_LDS_BANK_CONFLICT is half of their
// LDS cycles, 0 in the 32×32 kernels; profiles/mfma16_probe/SUMMARY.txt), which no check depends on.

typedef __attribute__((ext_vector_type(4))) float f32x4;

__host__ __device__ inline bool m16_fmt_ok(int fmt) { return fmt >= ODH_M16_BF16 && fmt <= ODH_M16_FP4; }
__host__ __device__ inline bool m16_scaled(int fmt) { return fmt == ODH_M16_FP8 || fmt == ODH_M16_FP4; }
// elements of one instruction = of one stage
__host__ __device__ inline int m16_bk(int fmt) {
  return fmt == ODH_M16_I8 ? 64 : m16_scaled(fmt) ? 128 : 32;
}

template <int FMT>
struct M16Types;
template <>
struct M16Types<ODH_M16_BF16> {
  using Acc = f32x4;
  using Out = float;
  static __device__ __forceinline__ Acc mfma(uint4 a, uint4 b, Acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0,
                                                   0, 0);
  }
  static __device__ __forceinline__ Out expect(int ia5, int jb7, int K) { return (float)probe_expect(ia5, jb7, K); }
};
template <>
struct M16Types<ODH_M16_F16> {
  using Acc = f32x4;
  using Out = float;
  static __device__ __forceinline__ Acc mfma(uint4 a, uint4 b, Acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0,
                                                  0);
  }
  static __device__ __forceinline__ Out expect(int ia5, int jb7, int K) { return (float)probe_expect(ia5, jb7, K); }
};
template <>
struct M16Types<ODH_M16_I8> {
  using Acc = i32x4;
  using Out = int;
  static __device__ __forceinline__ Acc mfma(uint4 a, uint4 b, Acc c) {
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, b), c, 0, 0,
                                                 0);
  }
  // odh_dense_fill's i8 operands; exact in i32: |.| <= 1025 · 6 · K
  static __device__ __forceinline__ Out expect(int ia5, int jb7, int K) {
    return ODH_DT_I8_MUL_A * ODH_DT_I8_MUL_B * probe_expect(ia5, jb7, K);
  }
};

// the scaled instruction: HW is the hardware's format code (0 e4m3, 4 e2m1), the opsels are immediates
template <int HW, int OA, int OB>
__device__ __forceinline__ f32x4 m16_scale_mfma(i32x8 a, i32x8 b, f32x4 acc, int sa, int sb) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, HW, HW, OA, sa, OB, sb);
}

// ---------------------------------------------------------------------------------------
// One wave, one instruction on a zero accumulator (odh_m16_one): lane l takes its registers from
// a[8l … 8l+7] and b[8l … 8l+7] (a format uses the low 4 or 8), its scale VGPRs from sa[l] and
// sb[l], and stores its four result registers at d[4l … 4l+3].
template <int FMT>
__global__ __launch_bounds__(64) void m16_one_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                     const uint32_t* __restrict__ sa, const uint32_t* __restrict__ sb,
                                                     int opsel_a, int opsel_b, uint32_t* __restrict__ d) {
  const int l = threadIdx.x;
  if constexpr (FMT == ODH_M16_FP8 || FMT == ODH_M16_FP4) {
    constexpr int HW = FMT == ODH_M16_FP4 ? 4 : 0;
    i32x8 fa, fb;
#pragma unroll
    for (int v = 0; v < 8; ++v) fa[v] = (int)a[8 * l + v], fb[v] = (int)b[8 * l + v];
    const int xa = (int)sa[l], xb = (int)sb[l];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#define ODH_M16_ONE(OA_, OB_) \
  case OA_ * 4 + OB_: acc = m16_scale_mfma<HW, OA_, OB_>(fa, fb, acc, xa, xb); break;
    switch (opsel_a * 4 + opsel_b) {
      ODH_M16_ONE(0, 0) ODH_M16_ONE(0, 1) ODH_M16_ONE(0, 2) ODH_M16_ONE(0, 3)
      ODH_M16_ONE(1, 0) ODH_M16_ONE(1, 1) ODH_M16_ONE(1, 2) ODH_M16_ONE(1, 3)
      ODH_M16_ONE(2, 0) ODH_M16_ONE(2, 1) ODH_M16_ONE(2, 2) ODH_M16_ONE(2, 3)
      ODH_M16_ONE(3, 0) ODH_M16_ONE(3, 1) ODH_M16_ONE(3, 2) ODH_M16_ONE(3, 3)
    }
#undef ODH_M16_ONE
#pragma unroll
    for (int r = 0; r < 4; ++r) d[4 * l + r] = __float_as_uint(acc[r]);
  } else {
    using T = M16Types<FMT>;
    const uint4 fa = reinterpret_cast<const uint4*>(a)[2 * l], fb = reinterpret_cast<const uint4*>(b)[2 * l];
    typename T::Acc acc = {0, 0, 0, 0};
    acc = T::mfma(fa, fb, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const typename T::Out v = acc[r];  // the element by value, then its bits
      d[4 * l + r] = __builtin_bit_cast(uint32_t, v);
    }
  }
}

// ---------------------------------------------------------------------------------------
// bf16, f16, i8: dense_gemm256_kernel's ring, one instruction per 16×16 fragment and stage
template <int FMT, bool VERIFY>
__global__ __launch_bounds__(G_THREADS, 1) void m16_gemm256_kernel(
    const uint4* __restrict__ A, const uint4* __restrict__ Bt, void* __restrict__ Cv, int N, int K,
    int* __restrict__ tile_xcd, int* __restrict__ xcd_blocks, unsigned* __restrict__ err_total,
    unsigned* __restrict__ err_xcd) {
  using T = M16Types<FMT>;
  using Acc = typename T::Acc;
  using Out = typename T::Out;
  constexpr int BKE = FMT == ODH_M16_I8 ? 64 : 32;  // elements per stage
  __shared__ uint4 lds[D_RING + 9];                 // one array: the ring, then the 35 expected values
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

  // stage kt → ring slot b, as dense_gemm256_kernel: wave w fills rows [32w, 32w + 32) of A and of B
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

  Acc acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][j][r] = 0;

  const int nkt = K / BKE;
  const int lr = lane & 15, lg = lane >> 4;
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
    // the stage's one instruction per fragment: lane group g reads chunk g of its row
    uint4 af[8], bfr[4];
#pragma unroll
    for (int i = 0; i < 8; ++i) af[i] = sa[dswz(wm * 128 + i * 16 + lr, lg)];
#pragma unroll
    for (int j = 0; j < 4; ++j) bfr[j] = sb[dswz(wn * 64 + j * 16 + lr, lg)];
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = T::mfma(af[i], bfr[j], acc[i][j]);
    __builtin_amdgcn_s_setprio(0);
  }
  // every DMA is retired (the last stage waited vmcnt(0)): an ordinary barrier publishes the table
  if (VERIFY) __syncthreads();

  // C/D map of 16x16: col = lane & 15, row = 4 * (lane >> 4) + reg
  Out* C = static_cast<Out*>(Cv);
  unsigned bad = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = tn * G_BN + wn * 64 + j * 16 + lr;
      const int rbase = tm * G_BM + wm * 128 + i * 16 + 4 * lg;
      if (VERIFY) {
        const int c7 = col % 7;
        const int r5 = rbase % 5;
#pragma unroll
        for (int r = 0; r < 4; ++r) bad += acc[i][j][r] != expect[((r5 + r) % 5) * 7 + c7];
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) C[(size_t)(rbase + r) * N + col] = acc[i][j][r];
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

// ---------------------------------------------------------------------------------------
// fp8, fp4: mx_gemm256_kernel's two-buffer loop, one instruction per 16×16 fragment and stage
template <int FMT, bool VERIFY>
__global__ __launch_bounds__(G_THREADS, 1) void m16_mx_gemm256_kernel(
    const uint4* __restrict__ A, const uint4* __restrict__ Bt, const uint8_t* __restrict__ sA,
    const uint8_t* __restrict__ sBt, float* __restrict__ C, const float* __restrict__ table, int N, int K,
    int* __restrict__ tile_xcd, int* __restrict__ xcd_blocks, unsigned* __restrict__ err_total,
    unsigned* __restrict__ err_xcd) {
  constexpr bool FP4 = FMT == ODH_M16_FP4;
  constexpr int HW = FP4 ? 4 : 0;           // the hardware's format code
  constexpr int HALVES = FP4 ? 1 : 2;       // 64-byte half-tiles per operand stage
  constexpr int TILE = HALVES * D_TILE;     // uint4 per operand stage
  constexpr int RING = 2 * 2 * TILE;        // [buffer][A, B][half][row × chunk]
  __shared__ uint4 lds[RING + MX_TABLE_U4];  // one array: the stages, then the table of expected values
  float* expect = reinterpret_cast<float*>(lds + RING);

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
  if (VERIFY && tid < MX_CLASSES) expect[tid] = table[tid];

  const size_t kch = (size_t)(K / 128) * (D_CH * HALVES);  // 16-byte chunks per global row
  const size_t nkb = (size_t)(K / 32);                     // scale bytes per row
  const uint4* Ag = A + (size_t)tm * G_BM * kch;
  const uint4* Bg = Bt + (size_t)tn * G_BN * kch;
  const int lr = lane & 15, lg = lane >> 4;
  const uint8_t* sAg = sA + (size_t)(tm * G_BM + wm * 128 + lr) * nkb;
  const uint8_t* sBg = sBt + (size_t)(tn * G_BN + wn * 64 + lr) * nkb;

  // stage kt → buffer b: wave w fills rows [32w, 32w + 32) of A and of B, 16 rows per instruction
  // and half-tile; lane l lands at LDS chunk p = base + l, which holds K-chunk (p & 3) ^ swizzle of
  // its half of the stage row
  auto issue = [&](int kt, int b) {
    uint4* la = lds + (b * 2 + 0) * TILE;
    uint4* lb = lds + (b * 2 + 1) * TILE;
#pragma unroll
    for (int hf = 0; hf < HALVES; ++hf)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int base = (w * 2 + i) * 64;
        const int p = base + lane;
        const int row = p >> 2;
        const int c = (p & 3) ^ ((row >> 2) & 3);
        const size_t g = (size_t)row * kch + (size_t)(kt * HALVES + hf) * D_CH + c;
        __builtin_amdgcn_global_load_lds(Ag + g, la + hf * D_TILE + base, 16, 0, 0);
        __builtin_amdgcn_global_load_lds(Bg + g, lb + hf * D_TILE + base, 16, 0, 0);
      }
  };
  // the stage's scale dword of each of this lane's rows, its own block's byte moved to byte 0
  // (the bytes above are other blocks' scales, which opsel 0 ignores)
  auto scales = [&](int kt, int (&sa)[8], int (&sb)[4]) {
    const size_t o = (size_t)kt * 4;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      sa[i] = (int)(*reinterpret_cast<const uint32_t*>(sAg + (size_t)i * 16 * nkb + o) >> (8 * lg));
#pragma unroll
    for (int j = 0; j < 4; ++j)
      sb[j] = (int)(*reinterpret_cast<const uint32_t*>(sBg + (size_t)j * 16 * nkb + o) >> (8 * lg));
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

  const int nkt = K / 128;
  int sa[8], sb[4], na[8], nb[4];
  issue(0, 0);
  scales(0, sa, sb);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nkt) {  // buffer cur^1 was released by the last barrier
      issue(kt + 1, cur ^ 1);
      scales(kt + 1, na, nb);
    }
    const uint4* la = lds + (cur * 2 + 0) * TILE;
    const uint4* lb = lds + (cur * 2 + 1) * TILE;
    // a lane's elements of its row: chunk g of the stage row's 64 bytes (FP4), or of each of its two halves (FP8)
    auto frag = [&](const uint4* t, int row) {
      i32x8 f = {};
      if constexpr (FP4) {
        const uint4 lo = t[dswz(row, lg)];
        f[0] = (int)lo.x, f[1] = (int)lo.y, f[2] = (int)lo.z, f[3] = (int)lo.w;
      } else {
        const uint4 lo = t[dswz(row, lg)], hi = t[D_TILE + dswz(row, lg)];
        f[0] = (int)lo.x, f[1] = (int)lo.y, f[2] = (int)lo.z, f[3] = (int)lo.w;
        f[4] = (int)hi.x, f[5] = (int)hi.y, f[6] = (int)hi.z, f[7] = (int)hi.w;
      }
      return f;
    };
    i32x8 bf[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bf[j] = frag(lb, wn * 64 + j * 16 + lr);
#pragma unroll
    for (int ig = 0; ig < 4; ++ig) {  // the A fragments two at a time
      i32x8 af[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) af[u] = frag(la, wm * 128 + (2 * ig + u) * 16 + lr);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[2 * ig + u][j] = m16_scale_mfma<HW, 0, 0>(af[u], bf[j], acc[2 * ig + u][j], sa[2 * ig + u], sb[j]);
      __builtin_amdgcn_s_setprio(0);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) sa[i] = na[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) sb[j] = nb[j];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // C/D map of 16x16: col = lane & 15, row = 4 * (lane >> 4) + reg
  unsigned bad = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = tn * G_BN + wn * 64 + j * 16 + lr;
      const int rbase = tm * G_BM + wm * 128 + i * 16 + 4 * lg;
      if (VERIFY) {
        const int c21 = col % MX_COLS;
        const int r15 = rbase % MX_ROWS;
#pragma unroll
        for (int r = 0; r < 4; ++r) bad += acc[i][j][r] != expect[((r15 + r) % MX_ROWS) * MX_COLS + c21];
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) C[(size_t)(rbase + r) * N + col] = acc[i][j][r];
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

// every format's kernel on one argument list: the dense ones ignore the scales and the table
template <bool VERIFY>
void m16_launch_gemm(int fmt, int nwg, hipStream_t stream, const uint4* A, const uint4* Bt, const uint8_t* sA,
                     const uint8_t* sBt, void* C, const float* table, int N, int K, int* tile_xcd, int* xcd_blocks,
                     unsigned* err_total, unsigned* err_xcd) {
  if (fmt == ODH_M16_FP8)
    m16_mx_gemm256_kernel<ODH_M16_FP8, VERIFY><<<nwg, G_THREADS, 0, stream>>>(
        A, Bt, sA, sBt, (float*)C, table, N, K, tile_xcd, xcd_blocks, err_total, err_xcd);
  else if (fmt == ODH_M16_FP4)
    m16_mx_gemm256_kernel<ODH_M16_FP4, VERIFY><<<nwg, G_THREADS, 0, stream>>>(
        A, Bt, sA, sBt, (float*)C, table, N, K, tile_xcd, xcd_blocks, err_total, err_xcd);
  else if (fmt == ODH_M16_I8)
    m16_gemm256_kernel<ODH_M16_I8, VERIFY><<<nwg, G_THREADS, 0, stream>>>(A, Bt, C, N, K, tile_xcd, xcd_blocks,
                                                                          err_total, err_xcd);
  else if (fmt == ODH_M16_F16)
    m16_gemm256_kernel<ODH_M16_F16, VERIFY><<<nwg, G_THREADS, 0, stream>>>(A, Bt, C, N, K, tile_xcd, xcd_blocks,
                                                                           err_total, err_xcd);
  else
    m16_gemm256_kernel<ODH_M16_BF16, VERIFY><<<nwg, G_THREADS, 0, stream>>>(A, Bt, C, N, K, tile_xcd, xcd_blocks,
                                                                            err_total, err_xcd);
}

// host side: what the 16×16 entry points take.  The dense formats take no scales and no table (a
// non-null one is refused); the scaled ones take all of them, the scale rows read 4 bytes at a time
bool m16_ok(int fmt, int M, int N, int K) {
  return m16_fmt_ok(fmt) && M > 0 && N > 0 && K > 0 && M % G_BM == 0 && N % G_BN == 0 && K % m16_bk(fmt) == 0;
}
bool m16_aligned(int fmt, const void* a, const void* b, const void* sa, const void* sb) {
  if (!a || !b || (((uintptr_t)a | (uintptr_t)b) & 15)) return false;
  if (!m16_scaled(fmt)) return !sa && !sb;
  return sa && sb && (((uintptr_t)sa | (uintptr_t)sb) & 3) == 0;
}
