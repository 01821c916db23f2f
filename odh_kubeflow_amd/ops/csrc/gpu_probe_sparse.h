// The start-up probe's 2:4 structured-sparsity kernels: the v_smfmac_* instructions, which
// torch.sparse.to_sparse_semi_structured and hipSPARSELt run on and no other kernel here issues:
//   v_smfmac_f32_32x32x32_bf16 / _f16      — 16 kept of 32 k per instruction, fp32 accumulation;
//   v_smfmac_i32_32x32x64_i8               — 32 kept of 64 k, i32 accumulation;
//   v_smfmac_f32_32x32x64_fp8_fp8 / _bf8_bf8 — the same shape on OCP e4m3fn / e5m2, fp32 accumulation.
// What they exercise beyond the dense instructions: the index operand (a VGPR of 2-bit selectors),
// the per-lane multiplexers that pick two of four B elements for each kept A element, and the
// compressed-A operand feed.
//
// Included by gpu_probe.hip inside its anonymous namespace, after gpu_probe_fp.h: it uses the tile
// constants of the 256² bf16 kernels (G_BM, G_BN, G_THREADS, D_CH, D_TILE), dswz, xcd_tile and
// xcc_id.  The loop is dense_gemm256_kernel's on a ring of its own.
//
// Public memory layout (odh_sparse_* of gpu_probe.h).  Ac is [M][K/2] row-major, the kept elements
// of A: kept elements 2g and 2g+1 belong to group g, the dense columns 4g … 4g+3.  meta is
// [M][K/8] bytes: group g of a row is the nibble at bits [4g, 4g+4) of the row, little endian, a
// nibble being p0 | p1 << 2, the dense positions of the two kept elements, p0 < p1 (a nibble with
// p0 >= p1 is unspecified).  Bt is [N][K] row-major, dense, in A's element type; C is [M][N], fp32
// or int32.  Ac and Bt are 16-byte aligned, meta 4-byte aligned.  M and N are multiples of 256, K
// of one stage: 64 for bf16 and f16, 128 for i8, fp8 and bf8 (128 bytes of a Bt row either way).
//
// Lane maps, measured on an MI355X with one instruction per wave: one-hot compressed A in one slot
// of one lane half against a B whose 64 (lane half, element) values are all distinct, for every
// slot, every 2-bit field of the index register set to 1, 2 and 3 in turn, and CBSZ/ABID 0/0, 0/1,
// 0/2, 0/3, 1/0 and 1/1; then 48 cases per format of random operands and random valid nibbles (CBSZ/ABID
// 0/0, 0/1 and 1/1) against the map read off: no mismatch in any of the 5 × 3 × 49152 outputs
// (profiles/sparse_probe/SUMMARY.txt).  i8, fp8 and bf8 were measured separately and agree.
//   * Lane l holds row l & 31 of A and column l & 31 of B; h = l >> 5 is its half.  In BYTES the map
//     is the same for all five instructions: an instruction reads 32 bytes of a compressed A row
//     and 64 bytes of a Bt row; lane half h holds bytes [16h, 16h + 16) of the A piece (kept
//     elements 8h … 8h+7 of 16, or 16h … 16h+15 of 32: the groups 4h … 4h+3 resp. 8h … 8h+7), and
//     of the Bt piece the two 16-byte chunks h and h + 2 (chunk h in the low half of the operand
//     register, chunk h + 2 in the high half) — not the contiguous chunks 2h and 2h + 1.  Kept
//     slot s of a lane pairs with B elements 4 (s >> 1) … 4 (s >> 1) + 3 of that order.
//   * Kept slot s of a lane is steered by the 2-bit field s of the lane's OWN index register,
//     bits [2s, 2s + 2): the value is the position in the group, independently for the two slots of
//     a group.  So the lane's index is its groups' nibbles in order, the public layout as it is.
//   * 16-bit formats use 16 bits of the register: with CBSZ = 0, ABID bit 0 picks the low or the
//     high half (ABID bit 1 is ignored); with CBSZ = 1 the low half whatever ABID.  The 8-bit
//     formats use all 32 bits and ignore both.  The kernel passes CBSZ = ABID = 0 and shifts the
//     32 bits of an instruction's metadata right by 16 h for the 16-bit formats.
//   * C/D is the 32x32 map of the bf16 kernels.
//
// Tile and pipeline: 256×256 per workgroup, 512 threads as 2(M)×4(N) waves of 128×64 outputs, two
// instructions per 32×32 fragment and stage, as dense_gemm256_kernel.  A stage is 64 bytes of each
// compressed-A row (16 KiB), 128 bytes of each Bt row (32 KiB, as two 64-byte tiles of the bf16
// layout and swizzle) and the rows' metadata (8 or 16 bytes a row: 2 or 4 KiB, [row][dword]): 50 or
// 52 KiB, so the ring has three slots, two stages in flight: 3 × 52 KiB + the table < 160 KiB with
// one workgroup per CU.  Everything is staged by LDS-DMA, the metadata in 4-byte pieces (one or two
// instructions per thread), so a stage is 2 (A) + 4 (Bt) + 1 or 2 (metadata) = 7 or 8 DMA
// instructions per thread.  The loop issues no other vector load (the VERIFY instances load their
// table entry once, before the first DMA: it is older than every DMA, so the counts hold): at stage
// kt each wave waits for vmcnt(7 resp. 8), the one younger stage, or vmcnt(0) at the last, then the
// raw barrier publishes the stage and proves the slot of stage kt - 1 free for stage kt + 2.
// Fragments and metadata are read from LDS as native vectors (__builtin_bit_cast of a uint4
// lvalue, as the dense kernels do).  Copying a uint4 or a struct of two instead turns into untyped
// 8-byte loads, and before such a load the compiler puts an s_waitcnt vmcnt(0) of its own, which
// drains the ring at every stage: the loop in the assembly must hold the counted wait alone.
//
// hipcc -O3 --offload-arch=gfx950 (ROCm 7.2), -Rpass-analysis=kernel-resource-usage; 2 waves per
// SIMD is the workgroup's own 8 waves:
//                                        VGPRs  AGPRs  LDS bytes  scratch  waves/SIMD
//   sparse_gemm256_kernel<BF16 | F16, false>      232      0     154448        0           2
//   sparse_gemm256_kernel<BF16 | F16, true>       233      0     154448        0           2
//   sparse_gemm256_kernel<I8 | FP8 | BF8, false>  233      0     160592        0           2
//   sparse_gemm256_kernel<I8 | FP8 | BF8, true>   234      0     160592        0           2
// LDS: 3 × (48 KiB + 2 resp. 4 KiB of metadata) + 848 B of table: one workgroup per CU.

typedef __attribute__((ext_vector_type(16))) __bf16 bf16x16;
typedef __attribute__((ext_vector_type(16))) _Float16 f16x16;
typedef __attribute__((ext_vector_type(8))) int i32x8;

__host__ __device__ inline bool sp_fmt_ok(int fmt) { return fmt >= ODH_SP_BF16 && fmt <= ODH_SP_BF8; }
// bytes per element, and dense elements per stage (128 bytes of a Bt row)
__host__ __device__ inline int sp_esize(int fmt) { return fmt == ODH_SP_BF16 || fmt == ODH_SP_F16 ? 2 : 1; }
__host__ __device__ inline int sp_bk(int fmt) { return 128 / sp_esize(fmt); }

constexpr int SP_ROWS = 30, SP_COLS = 7;  // classes: (i mod 30, j mod 7)
static_assert(SP_ROWS * SP_COLS == ODH_SP_CLASSES, "the table of expected values is ODH_SP_CLASSES ints");
constexpr int SP_TABLE_U4 = (ODH_SP_CLASSES + 3) / 4;  // the table in uint4 units of LDS

// The probe operands.  Bt[j][k] = ((11j + 5k) mod 7) - 3; A[i][k] = ((3i + 7k) mod 5) - 2 pruned to
// 2:4: group g = k / 4 of row i keeps the pair SEL[(i + g) mod 6], SEL = {(0,3), (2,3), (1,3), (1,2),
// (0,1), (0,2)}: the nibbles 12, 14, 13, 9, 4, 8.
__host__ __device__ inline int sp_a(long i, long k) { return (int)((i * 3 + k * 7) % 5) - 2; }
__host__ __device__ inline int sp_b(long j, long k) { return (int)((j * 11 + k * 5) % 7) - 3; }
__host__ __device__ inline unsigned sp_nibble(long i, long g) { return (0x849DECu >> (4 * (int)((i + g) % 6))) & 15u; }
// one term of the expected value, from the definition: A as pruned, times Bt
__host__ __device__ inline int sp_term(int i, int j, int k) {
  const unsigned nib = sp_nibble(i, k >> 2), pos = (unsigned)k & 3u;
  return pos == (nib & 3u) || pos == (nib >> 2) ? sp_a(i, k) * sp_b(j, k) : 0;
}
__host__ inline int sp_expect(int i30, int j7, int K) {
  int s = 0;
  for (int k = 0; k < K; ++k) s += sp_term(i30, j7, k);
  return s;
}

// a small integer (|v| <= 3) in the format's own code: the value times the dense i8 step's odd
// multipliers for i8, the exact value otherwise
__device__ inline unsigned sp_code(int fmt, int v, bool isa) {
  const unsigned m = (unsigned)(v < 0 ? -v : v);
  switch (fmt) {
    case ODH_SP_BF16: return __builtin_bit_cast(unsigned, (float)v) >> 16;
    case ODH_SP_F16: return __builtin_bit_cast(unsigned short, (_Float16)(float)v);
    case ODH_SP_I8: return (unsigned)(v * (isa ? ODH_DT_I8_MUL_A : ODH_DT_I8_MUL_B)) & 0xFFu;
    case ODH_SP_FP8: return (m == 0 ? 0u : m == 1 ? 0x38u : m == 2 ? 0x40u : 0x44u) | (v < 0 ? 0x80u : 0u);
    default: return (m == 0 ? 0u : m == 1 ? 0x3Cu : m == 2 ? 0x40u : 0x42u) | (v < 0 ? 0x80u : 0u);
  }
}

// one thread per 8 dense k of an A row (two groups: four kept elements and one metadata byte), then
// one per Bt element
__global__ void sparse_fill_kernel(int fmt, void* __restrict__ Ac, uint8_t* __restrict__ meta, void* __restrict__ Bt,
                                   int M, int N, int K) {
  const size_t na = (size_t)M * (K / 8), nb = (size_t)N * K;
  const bool wide = sp_esize(fmt) == 2;
  for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < na + nb;
       idx += (size_t)gridDim.x * blockDim.x) {
    if (idx < na) {
      const long r = (long)(idx / (K / 8)), u = (long)(idx % (K / 8));
      unsigned byte = 0;
      for (int t = 0; t < 2; ++t) {
        const long g = 2 * u + t;
        const unsigned nib = sp_nibble(r, g);
        byte |= nib << (4 * t);
        for (int e = 0; e < 2; ++e) {
          const unsigned c = sp_code(fmt, sp_a(r, 4 * g + (e ? nib >> 2 : nib & 3u)), true);
          const size_t o = (size_t)r * (K / 2) + 2 * g + e;
          if (wide)
            ((uint16_t*)Ac)[o] = (uint16_t)c;
          else
            ((uint8_t*)Ac)[o] = (uint8_t)c;
        }
      }
      meta[idx] = (uint8_t)byte;
    } else {
      const size_t o = idx - na;
      const unsigned c = sp_code(fmt, sp_b((long)(o / K), (long)(o % K)), false);
      if (wide)
        ((uint16_t*)Bt)[o] = (uint16_t)c;
      else
        ((uint8_t*)Bt)[o] = (uint8_t)c;
    }
  }
}

// the 30 × 7 table of expected sums of the small integers, from the definition (family and
// selector), not from the compressed arrays; one wave per class, its lanes striding k
__global__ __launch_bounds__(64) void sparse_table_kernel(int* __restrict__ table, int K) {
  const int t = blockIdx.x;
  int s = 0;
  for (int k = threadIdx.x; k < K; k += 64) s += sp_term(t / SP_COLS, t % SP_COLS, k);
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (threadIdx.x == 0) table[t] = s;
}

// the two 16-byte chunks of a lane's B operand as one 32-byte register
__device__ __forceinline__ i32x8 sp_b32(i32x4 lo, i32x4 hi) { return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7); }

template <int FMT>
struct SpTypes;
template <>
struct SpTypes<ODH_SP_BF16> {
  using Acc = f32x16;
  using Out = float;
  static constexpr int ESIZE = 2, SCALE = 1;
  static __device__ __forceinline__ Acc mfma(i32x4 a, i32x8 b, Acc c, int idx) {
    return __builtin_amdgcn_smfmac_f32_32x32x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x16, b), c,
                                                     idx, 0, 0);
  }
};
template <>
struct SpTypes<ODH_SP_F16> {
  using Acc = f32x16;
  using Out = float;
  static constexpr int ESIZE = 2, SCALE = 1;
  static __device__ __forceinline__ Acc mfma(i32x4 a, i32x8 b, Acc c, int idx) {
    return __builtin_amdgcn_smfmac_f32_32x32x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x16, b), c,
                                                    idx, 0, 0);
  }
};
template <>
struct SpTypes<ODH_SP_I8> {
  using Acc = i32x16;
  using Out = int;
  static constexpr int ESIZE = 1, SCALE = ODH_DT_I8_MUL_A * ODH_DT_I8_MUL_B;  // exact in i32: |.| <= 1025 · 6 · K / 2
  static __device__ __forceinline__ Acc mfma(i32x4 a, i32x8 b, Acc c, int idx) {
    return __builtin_amdgcn_smfmac_i32_32x32x64_i8(a, b, c, idx,
                                                   0, 0);
  }
};
template <>
struct SpTypes<ODH_SP_FP8> {
  using Acc = f32x16;
  using Out = float;
  static constexpr int ESIZE = 1, SCALE = 1;
  static __device__ __forceinline__ Acc mfma(i32x4 a, i32x8 b, Acc c, int idx) {
    return __builtin_amdgcn_smfmac_f32_32x32x64_fp8_fp8(a, b, c,
                                                        idx, 0, 0);
  }
};
template <>
struct SpTypes<ODH_SP_BF8> {
  using Acc = f32x16;
  using Out = float;
  static constexpr int ESIZE = 1, SCALE = 1;
  static __device__ __forceinline__ Acc mfma(i32x4 a, i32x8 b, Acc c, int idx) {
    return __builtin_amdgcn_smfmac_f32_32x32x64_bf8_bf8(a, b, c,
                                                        idx, 0, 0);
  }
};

template <int FMT, bool VERIFY>
__global__ __launch_bounds__(G_THREADS, 1) void sparse_gemm256_kernel(
    const uint4* __restrict__ Ac, const uint32_t* __restrict__ meta, const uint4* __restrict__ Bt,
    void* __restrict__ Cv, const int* __restrict__ table, int N, int K, int* __restrict__ tile_xcd,
    int* __restrict__ xcd_blocks, unsigned* __restrict__ err_total, unsigned* __restrict__ err_xcd) {
  using T = SpTypes<FMT>;
  using Acc = typename T::Acc;
  using Out = typename T::Out;
  constexpr int BKE = 128 / T::ESIZE;      // dense elements per stage
  constexpr int DW = BKE / 32;             // metadata dwords per row and stage: 2 or 4
  constexpr int NM = DW / 2;               // metadata DMA instructions per thread and stage
  constexpr int META_U4 = G_BM * DW / 4;   // uint4 of metadata per stage
  constexpr int SLOT = 3 * D_TILE + META_U4;  // a ring slot: A, Bt bytes [0, 64), Bt bytes [64, 128), metadata
  constexpr int NSLOT = 3;
  constexpr int RING = NSLOT * SLOT;
  static_assert((RING + SP_TABLE_U4) * 16 <= 160 * 1024, "the ring and the table fit in the CU's LDS");
  __shared__ uint4 lds[RING + SP_TABLE_U4];  // one array: the ring, then the 210 expected values
  Out* expect = reinterpret_cast<Out*>(lds + RING);

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
  if (VERIFY && tid < ODH_SP_CLASSES) expect[tid] = (Out)(table[tid] * T::SCALE);

  const int nkt = K / BKE;
  const size_t kcha = (size_t)nkt * D_CH;      // 16-byte chunks per compressed-A row
  const size_t kchb = (size_t)nkt * 2 * D_CH;  // per Bt row
  const size_t kdw = (size_t)nkt * DW;         // metadata dwords per row
  const uint4* Ag = Ac + (size_t)tm * G_BM * kcha;
  const uint4* Bg = Bt + (size_t)tn * G_BN * kchb;
  const uint32_t* Mg = meta + (size_t)tm * G_BM * kdw;

  // stage kt → ring slot b.  A and each 64-byte half of Bt as in dense_gemm256_kernel: wave w fills
  // rows [32w, 32w + 32), lane l lands at LDS chunk p = base + l, which holds K-chunk (p & 3) ^
  // swizzle of row p >> 2.  Metadata: dword p = 512 i + 64 w + l of the stage's [row][DW] block.
  auto issue = [&](int kt, int b) {
    uint4* la = lds + b * SLOT;
    uint32_t* lm = reinterpret_cast<uint32_t*>(la + 3 * D_TILE);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int base = (w * 2 + i) * 64;
      const int p = base + lane;
      const int row = p >> 2;
      const int c = (p & 3) ^ ((row >> 2) & 3);
      __builtin_amdgcn_global_load_lds(Ag + ((size_t)row * kcha + (size_t)kt * D_CH + c), la + base, 16, 0, 0);
      const size_t g = (size_t)row * kchb + (size_t)kt * 2 * D_CH + c;
      __builtin_amdgcn_global_load_lds(Bg + g, la + D_TILE + base, 16, 0, 0);
      __builtin_amdgcn_global_load_lds(Bg + g + D_CH, la + 2 * D_TILE + base, 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < NM; ++i) {
      const int base = i * G_THREADS + w * 64;
      const int p = base + lane;
      __builtin_amdgcn_global_load_lds(Mg + ((size_t)(p / DW) * kdw + (size_t)kt * DW + p % DW), lm + base, 4, 0, 0);
    }
  };

  Acc acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

  const int lr = lane & 31, lh = lane >> 5;
  issue(0, 0);
  if (nkt > 1) issue(1, 1);
  int cur = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    // retire THIS wave's DMA of stage kt (the one younger stage stays in flight), then the barrier
    // makes every wave's part visible and proves stage kt-1's slot is no longer read
    if (kt + 1 < nkt) {
      if (NM == 1)
        asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    const int nxt = cur == 0 ? NSLOT - 1 : cur - 1;  // the slot of stage kt - 1 = of stage kt + 2
    if (kt + 2 < nkt) issue(kt + 2, nxt);
    const uint4* sa = lds + cur * SLOT;
    const uint4* sb = sa + D_TILE;
    const uint4* sm = sa + 3 * D_TILE;
    // both instructions of the stage: lane half h reads chunk 2s + h of its compressed-A row, chunks
    // h and h + 2 of the s-th 64 bytes of its Bt row, and its row's metadata
    i32x4 af[2][4];
    i32x8 bfr[2][2];
    int ix[2][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = wm * 128 + i * 32 + lr;
      if (DW == 2) {
        const i32x4 m4 = __builtin_bit_cast(i32x4, sm[row >> 1]);  // two rows' metadata
        ix[0][i] = (int)((unsigned)(row & 1 ? m4[2] : m4[0]) >> (16 * lh));
        ix[1][i] = (int)((unsigned)(row & 1 ? m4[3] : m4[1]) >> (16 * lh));
      } else {
        const i32x4 m4 = __builtin_bit_cast(i32x4, sm[row]);
        ix[0][i] = lh ? m4[1] : m4[0];
        ix[1][i] = lh ? m4[3] : m4[2];
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) af[s][i] = __builtin_bit_cast(i32x4, sa[dswz(row, 2 * s + lh)]);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = wn * 64 + j * 32 + lr;
        bfr[s][j] = sp_b32(__builtin_bit_cast(i32x4, sb[s * D_TILE + dswz(col, lh)]),
                           __builtin_bit_cast(i32x4, sb[s * D_TILE + dswz(col, lh + 2)]));
      }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = T::mfma(af[s][i], bfr[s][j], acc[i][j], ix[s][i]);
    __builtin_amdgcn_s_setprio(0);
    cur = cur == NSLOT - 1 ? 0 : cur + 1;
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
        const int c7 = col % SP_COLS;
        const int r30 = rbase % SP_ROWS;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rr = (r30 + (r & 3) + 8 * (r >> 2)) % SP_ROWS;
          bad += acc[i][j][r] != expect[rr * SP_COLS + c7];
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

// every format's kernel on one argument list
template <bool VERIFY, typename... Args>
void sparse_launch_gemm(int fmt, int nwg, hipStream_t stream, Args... args) {
  switch (fmt) {
    case ODH_SP_BF16: sparse_gemm256_kernel<ODH_SP_BF16, VERIFY><<<nwg, G_THREADS, 0, stream>>>(args...); break;
    case ODH_SP_F16: sparse_gemm256_kernel<ODH_SP_F16, VERIFY><<<nwg, G_THREADS, 0, stream>>>(args...); break;
    case ODH_SP_I8: sparse_gemm256_kernel<ODH_SP_I8, VERIFY><<<nwg, G_THREADS, 0, stream>>>(args...); break;
    case ODH_SP_FP8: sparse_gemm256_kernel<ODH_SP_FP8, VERIFY><<<nwg, G_THREADS, 0, stream>>>(args...); break;
    default: sparse_gemm256_kernel<ODH_SP_BF8, VERIFY><<<nwg, G_THREADS, 0, stream>>>(args...); break;
  }
}

// host side: what the sparse entry points take
bool sparse_ok(int fmt, int M, int N, int K) {
  return sp_fmt_ok(fmt) && M > 0 && N > 0 && K > 0 && M % G_BM == 0 && N % G_BN == 0 && K % sp_bk(fmt) == 0;
}
bool sparse_aligned(const void* ac, const void* meta, const void* bt) {
  return ac && meta && bt && (((uintptr_t)ac | (uintptr_t)bt) & 15) == 0 && ((uintptr_t)meta & 3) == 0;
}
// classes expecting 0 at this K (K > 0).  210 sums of K terms on the host: 0.3 ms at K = 1024, which a
// fused check would otherwise spend between its caller's two events on every launch, so the answer
// for the last K asked about is kept (K << 32 | zeros)
int sparse_zero_classes(int K) {
  static std::atomic<unsigned long long> last{0};
  const unsigned long long seen = last.load(std::memory_order_relaxed);
  if (seen >> 32 == (unsigned long long)K) return (int)(seen & 0xFFFFFFFFu);
  int zeros = 0;
  for (int t = 0; t < ODH_SP_CLASSES; ++t) zeros += sp_expect(t / SP_COLS, t % SP_COLS, K) == 0;
  last.store((unsigned long long)K << 32 | (unsigned)zeros, std::memory_order_relaxed);
  return zeros;
}
