// The start-up probe's block-scaled kernels, one per operand format of the instruction (FP8,
// BF8, FP6, BF6, FP4): the block-scaled matrix-core path of gfx950
// (v_mfma_scale_f32_32x32x64_f8f6f4), which the bf16 probe never touches: the operand decode,
// the per-32-element E8M0 block scale and the scale multiply.
//
// Included by gpu_probe.hip inside its anonymous namespace, after the 256² bf16 kernels: it
// uses their tile constants (G_BM, G_BN, G_THREADS, D_CH, D_TILE), dswz, xcd_tile and xcc_id.
//
// Public memory layout (odh_mx_* of gpu_probe.h): A is [M][K] and Bt is [N][K] row-major
// codes, FP8 (OCP e4m3fn) one byte per element, FP4 (e2m1) two per byte with the even k in
// the low nibble; scales are [rows][K/32] E8M0 bytes, one per 32 consecutive k of a row.  BF8
// (OCP e5m2) is laid out as FP8.  FP6 (e2m3) and BF6 (e3m2) are packed: element k of a row is
// bits [6k, 6k + 6) of the row read as a little-endian bit string, so a block of 32 elements is
// 24 consecutive bytes and a row 3K/4 bytes.
//
// Operand map of the 32x32x64 instruction, as measured on the MI355X (one instruction on random
// codes and scales, fitted on the host).  Lane l holds row (A) or column (B) l & 31; with
// h = l >> 5, byte `opsel` of the scale VGPR of lane l is the scale of that row's k-block h
// (k = 32h … 32h+31) in every format.  The elements differ:
//   FP4 (4 VGPRs): the lane holds its own block, k = 32h … 32h+31, ascending from the low
//     nibble of VGPR 0;
//   FP8 (8 VGPRs): VGPRs 0-3 hold k = 16h … 16h+15 of block 0 and VGPRs 4-7 hold
//     k = 32+16h … 32+16h+15 of block 1, ascending from the low byte: each lane carries half of
//     either block, and the hardware scales its upper four VGPRs by the scale in lane (l & 31) + 32;
//   BF8 (8 VGPRs): as FP8, scales included.  The two infinity codes 0x7C / 0xFC and the six NaN
//     codes behave as IEEE says: inf · 0 = NaN, inf · x = ±inf;
//   FP6, BF6 (6 VGPRs, the low six of the eight the builtin takes; the other two are ignored):
//     as FP4, the lane holds its own block, k = 32h … 32h+31, element e in bits [6e, 6e + 6) of
//     its 192 bits, ascending from bit 0 of VGPR 0, with the block's scale in byte `opsel` of
//     the lane's scale VGPR (measured with `opsel` 0-3 on the A side and 0, 2, 3 on the B side;
//     FP6 bit for bit on all 64 codes; BF6 on all 64 codes to 7e-5 of sum |a||b|, where an fp32
//     chain of 64 terms rounds to 4e-6 at most: products up to 2^18 apart in one instruction lose
//     low bits.  With products at most 2^16 apart, as in the tests, BF6 is bit for bit too).
// C/D is the 32x32 map of the bf16 kernels.
//
// Tests, all five formats against the one host model tests/mx_reference.py, each written once:
// tests/test_gpu_mx_exact.py and tests/test_gpu_lowprec_sweeps.py (with tests/probe_gpu.py) run on
// FP8 and FP4, and tests/test_gpu_mx_formats_exact.py calls the same functions on BF8, FP6, BF6.
// Random codes and scales; every code of a format against every code of it (the subnormals, the
// NaN codes and BF8's infinities decode as the OCP definitions say); every E8M0 byte 1 … 254
// through the 8-bit and the 6-bit arms; and the fused check's exact mismatch count and per-XCD
// attribution for a changed element and a changed scale byte in every row and every column.
//
// Tile: the 256×256 tile of gemm256_kernel (512 threads, 8 waves as 2×4, 128×64 outputs per
// wave), 16 KiB per operand stage = 256 rows × 64 bytes (BK = 64 FP8 or 128 FP4 elements),
// staged by global_load_lds of 16 B with the XOR swizzle of the deep bf16 kernel on the source
// address, two buffers, vmcnt(0) + __syncthreads() per stage.  The scale bytes are ordinary
// global loads into registers (one 2- or 4-byte load per 32-row fragment per stage, issued one
// stage ahead); a counted-vmcnt ring would have to count them too, so this kernel has none.
// FP6 / BF6 rows are 96 bytes per stage: the same kernel takes them in `if constexpr (P6)` arms
// of its staging, scale loads and fragment reads (see S_CH below).  The arms are the bodies of
// what were two kernels, kept word for word: so written, every instantiation compiles to the
// instructions it had as a kernel of its own, while an earlier merge that shared more of the two
// bodies changed the 6-bit kernels' code.  Share more between the arms only if they still do.

typedef __attribute__((ext_vector_type(8))) int i32x8;

constexpr int MX_ROWS = 15;  // A[i][k] has period 5 in i, its scale period 3
constexpr int MX_COLS = 21;  // Bt[j][k] has period 7 in j, its scale period 3
constexpr int MX_CLASSES = MX_ROWS * MX_COLS;
static_assert(MX_CLASSES == ODH_MX_CLASSES, "the table of expected values is ODH_MX_CLASSES floats");
constexpr int MX_TABLE_U4 = (MX_CLASSES + 3) / 4;  // the table in uint4 units of LDS

__host__ __device__ inline bool mx_fmt_ok(int fmt) { return fmt >= ODH_MX_FP8 && fmt <= ODH_MX_FP4; }
__host__ __device__ inline bool mx_packed6(int fmt) { return fmt == ODH_MX_FP6 || fmt == ODH_MX_BF6; }
// elements per stage: 64 bytes per row of FP8, BF8 or FP4, 96 bytes of FP6 or BF6
__host__ __device__ inline int mx_bk(int fmt) { return fmt == ODH_MX_FP8 || fmt == ODH_MX_BF8 ? 64 : 128; }
// bytes of a row of K elements
__host__ __device__ inline size_t mx_row_bytes(int fmt, int K) {
  return mx_packed6(fmt) ? (size_t)(K / 4) * 3 : (size_t)(K / (fmt == ODH_MX_FP4 ? 2 : 1));
}

// the bf16 probe's operand families and the scale exponents (E8M0 byte 126 + e: 2^-1, 1, 2)
__host__ __device__ inline int mx_a(int i, int k) { return (int)((3L * i + 7L * k) % 5) - 2; }
__host__ __device__ inline int mx_b(int j, int k) { return (int)((11L * j + 5L * k) % 7) - 3; }
__host__ __device__ inline int mx_e(int r, int kb) { return (r + kb) % 3; }

// 4 × the term of k in the expected C[i][j], an integer: it depends only on (i mod 15, j mod 21)
__host__ __device__ inline int mx_term4(int i15, int j21, int k) {
  const int kb = k >> 5;
  return mx_a(i15, k) * mx_b(j21, k) * (1 << (mx_e(i15, kb) + mx_e(j21, kb)));
}
inline int mx_expect4(int i15, int j21, int K) {
  int s = 0;
  for (int k = 0; k < K; ++k) s += mx_term4(i15, j21, k);
  return s;
}

// the code of the integer v, |v| <= 3: e4m3fn 1 = 0x38, 2 = 0x40, 3 = 0x44; e2m1 1 = 2, 2 = 4, 3 = 5;
// e5m2 0x3C, 0x40, 0x42; e2m3 0x08, 0x10, 0x14; e3m2 0x0C, 0x10, 0x12 (the 6-bit sign is 0x20)
__device__ __forceinline__ unsigned mx_code(int fmt, int v) {
  const int m = v < 0 ? -v : v;
  if (fmt == ODH_MX_FP4) return (m == 0 ? 0u : m == 1 ? 2u : m == 2 ? 4u : 5u) | (v < 0 ? 8u : 0u);
  if (fmt == ODH_MX_BF8) return (m == 0 ? 0u : m == 1 ? 0x3Cu : m == 2 ? 0x40u : 0x42u) | (v < 0 ? 0x80u : 0u);
  if (fmt == ODH_MX_FP6) return (m == 0 ? 0u : m == 1 ? 0x08u : m == 2 ? 0x10u : 0x14u) | (v < 0 ? 0x20u : 0u);
  if (fmt == ODH_MX_BF6) return (m == 0 ? 0u : m == 1 ? 0x0Cu : m == 2 ? 0x10u : 0x12u) | (v < 0 ? 0x20u : 0u);
  return (m == 0 ? 0u : m == 1 ? 0x38u : m == 2 ? 0x40u : 0x44u) | (v < 0 ? 0x80u : 0u);
}

// one thread per operand byte, then per scale byte
__global__ void mx_fill_kernel(int fmt, uint8_t* __restrict__ A, uint8_t* __restrict__ Bt, uint8_t* __restrict__ sA,
                               uint8_t* __restrict__ sBt, int M, int N, int K) {
  const int epb = fmt == ODH_MX_FP4 ? 2 : 1;
  const bool p6 = mx_packed6(fmt);
  const size_t rb = mx_row_bytes(fmt, K), nkb = (size_t)(K / 32);
  const size_t na = (size_t)M * rb, nb = (size_t)N * rb, nsa = (size_t)M * nkb, nsb = (size_t)N * nkb;
  for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < na + nb + nsa + nsb;
       idx += (size_t)gridDim.x * blockDim.x) {
    if (idx < na + nb) {
      const bool isa = idx < na;
      const size_t o = isa ? idx : idx - na;
      const int r = (int)(o / rb);
      unsigned c;
      if (p6) {  // byte y of the 3 that hold the elements 4g … 4g+3, 6 bits each from bit 0 up
        const int g = (int)(o % rb) / 3, y = (int)(o % rb) % 3;
        unsigned w = 0;
        for (int e = 0; e < 4; ++e) w |= mx_code(fmt, isa ? mx_a(r, 4 * g + e) : mx_b(r, 4 * g + e)) << (6 * e);
        c = w >> (8 * y);
      } else {
        const int k = (int)(o % rb) * epb;
        c = mx_code(fmt, isa ? mx_a(r, k) : mx_b(r, k));
        if (epb == 2) c |= mx_code(fmt, isa ? mx_a(r, k + 1) : mx_b(r, k + 1)) << 4;
      }
      (isa ? A : Bt)[o] = (uint8_t)c;
    } else {
      const size_t s = idx - na - nb;
      const bool isa = s < nsa;
      const size_t o = isa ? s : s - nsa;
      (isa ? sA : sBt)[o] = (uint8_t)(126 + mx_e((int)(o / nkb), (int)(o % nkb)));
    }
  }
}

// one wave per class, its lanes striding k: an integer sum, so the order does not matter (one
// thread per class took 110 µs at K = 1024, twice the GEMM it serves)
__global__ __launch_bounds__(64) void mx_table_kernel(float* __restrict__ table, int K) {
  const int t = blockIdx.x;
  int s = 0;
  for (int k = threadIdx.x; k < K; k += 64) s += mx_term4(t / MX_COLS, t % MX_COLS, k);
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (threadIdx.x == 0) table[t] = (float)s * 0.25f;
}

template <int FMT, int OPSEL>
__device__ __forceinline__ f32x16 mx_mfma(i32x8 a, i32x8 b, f32x16 acc, int sa, int sb) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, FMT, FMT, OPSEL, sa, OPSEL, sb);
}

// FP6 / BF6, the P6 arms of mx_gemm256_kernel: the same tile, waves and epilogue on 96-byte stage
// rows.  A stage of 128 elements
// is 256 rows × 6 chunks of 16 B = 24 KiB per operand, two buffers = 96 KiB.  Wave w stages rows
// [32w, 32w + 32) of A and of B with three global_load_lds of 16 B each: lane l of instruction i
// lands at LDS chunk p = 192w + 64i + l, row p / 6, slot p % 6, and fetches K-chunk
// slot ^ ((row >> 3) & 1) of that row.  A lane's fragment of k-step s is block 2s + h of its row,
// bytes [24 (2s + h), + 24): 8-byte aligned only, so it is read as three ds_read_b64.  A 32-lane
// group of such a read covers 32 rows 24 dwords apart, which fall on 8 distinct bank offsets; the
// XOR moves every second group of 8 rows by 4 dwords, which leaves a 2-way conflict (a 16-byte
// chunk cannot be moved by the 2 dwords that would remove it).  Scales as in the FP4 path: one
// u32 per row and stage, `opsel` 0 and 2.
constexpr int S_CH = 6;               // 16-byte chunks per stage row
constexpr int S_TILE = G_BM * S_CH;   // uint4 per operand stage (1536 = 24 KiB)

// LDS index, in 8-byte units, of piece q (0 … 11) of a stage row
__device__ __forceinline__ int sswz(int r, int q) { return (r * S_CH + ((q >> 1) ^ ((r >> 3) & 1))) * 2 + (q & 1); }

template <int FMT, bool VERIFY>
__global__ __launch_bounds__(G_THREADS, 1) void mx_gemm256_kernel(
    const uint4* __restrict__ A, const uint4* __restrict__ Bt, const uint8_t* __restrict__ sA,
    const uint8_t* __restrict__ sBt, float* __restrict__ C, const float* __restrict__ table, int N, int K,
    int* __restrict__ tile_xcd, int* __restrict__ xcd_blocks, unsigned* __restrict__ err_total,
    unsigned* __restrict__ err_xcd) {
  constexpr bool FP4 = FMT == ODH_MX_FP4;
  constexpr bool P6 = FMT == ODH_MX_FP6 || FMT == ODH_MX_BF6;  // packed 6-bit: 96-byte stage rows
  constexpr int EPB = FP4 ? 2 : 1;            // elements per byte (P6: four in three bytes, not used)
  constexpr int BKE = P6 ? 128 : 64 * EPB;    // elements per stage
  constexpr int KB_STAGE = BKE / 32;          // scale blocks per row per stage: 2 (one u16) or 4 (one u32)
  constexpr int TILE = P6 ? S_TILE : D_TILE;  // uint4 per operand stage
  constexpr int RING = 2 * 2 * TILE;          // [buffer][A, B][row × chunk]
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

  const size_t kch = P6 ? (size_t)(K / BKE) * S_CH : (size_t)(K / EPB / 16);  // 16-byte chunks per global row
  const size_t nkb = (size_t)(K / 32);        // scale bytes per row
  const uint4* Ag = A + (size_t)tm * G_BM * kch;
  const uint4* Bg = Bt + (size_t)tn * G_BN * kch;
  const int lr = lane & 31, lh = lane >> 5;
  const uint8_t* sAg = sA + (size_t)(tm * G_BM + wm * 128 + lr) * nkb;
  const uint8_t* sBg = sBt + (size_t)(tn * G_BN + wn * 64 + lr) * nkb;

  // stage kt → buffer b: wave w fills rows [32w, 32w + 32) of A and of B, 16 rows per
  // instruction; lane l lands at LDS chunk p = base + l, which holds K-chunk (p & 3) ^ swizzle
  // (P6: three instructions of 64 chunks, six chunks per row)
  auto issue = [&](int kt, int b) {
    uint4* la = lds + (b * 2 + 0) * TILE;
    uint4* lb = lds + (b * 2 + 1) * TILE;
    if constexpr (P6) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int base = (w * 3 + i) * 64;
        const int p = base + lane;
        const int row = p / S_CH;
        const int c = (p - row * S_CH) ^ ((row >> 3) & 1);
        const size_t g = (size_t)row * kch + (size_t)kt * S_CH + c;
        __builtin_amdgcn_global_load_lds(Ag + g, la + base, 16, 0, 0);
        __builtin_amdgcn_global_load_lds(Bg + g, lb + base, 16, 0, 0);
      }
    } else {
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
    }
  };
  // the stage's scale bytes of this lane's rows, its own k-half in byte 0 (FP4: and its
  // second k-step's in byte 2; P6 the same four bytes); the bytes above are other blocks' scales,
  // which opsel ignores
  auto scales = [&](int kt, int (&sa)[4], int (&sb)[2]) {
    const size_t o = (size_t)kt * KB_STAGE;
    if constexpr (P6) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        sa[i] = (int)(*reinterpret_cast<const uint32_t*>(sAg + (size_t)i * 32 * nkb + o) >> (8 * lh));
#pragma unroll
      for (int j = 0; j < 2; ++j)
        sb[j] = (int)(*reinterpret_cast<const uint32_t*>(sBg + (size_t)j * 32 * nkb + o) >> (8 * lh));
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint8_t* p = sAg + (size_t)i * 32 * nkb + o;
        sa[i] = (int)((FP4 ? *reinterpret_cast<const uint32_t*>(p) : *reinterpret_cast<const uint16_t*>(p)) >>
                    (8 * lh));
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const uint8_t* p = sBg + (size_t)j * 32 * nkb + o;
        sb[j] = (int)((FP4 ? *reinterpret_cast<const uint32_t*>(p) : *reinterpret_cast<const uint16_t*>(p)) >>
                    (8 * lh));
      }
    }
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nkt = K / BKE;
  int sa[4], sb[2], na[4], nb[2];
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
    if constexpr (P6) {
      const uint2* la = reinterpret_cast<const uint2*>(lds + (cur * 2 + 0) * S_TILE);
      const uint2* lb = reinterpret_cast<const uint2*>(lds + (cur * 2 + 1) * S_TILE);
      // a lane's 32 elements: the 24 bytes of block blk of its row, in the low six VGPRs
      auto frag = [&](const uint2* t, int row, int blk) {
        i32x8 f = {};
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const uint2 v = t[sswz(row, 3 * blk + q)];
          f[2 * q] = (int)v.x, f[2 * q + 1] = (int)v.y;
        }
        return f;
      };
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int blk = 2 * s + lh;
        i32x8 af[4], bf[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = frag(la, wm * 128 + i * 32 + lr, blk);
#pragma unroll
        for (int j = 0; j < 2; ++j) bf[j] = frag(lb, wn * 64 + j * 32 + lr, blk);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = s == 0 ? mx_mfma<FMT, 0>(af[i], bf[j], acc[i][j], sa[i], sb[j])
                               : mx_mfma<FMT, 2>(af[i], bf[j], acc[i][j], sa[i], sb[j]);
        __builtin_amdgcn_s_setprio(0);
      }
    } else {
      const uint4* la = lds + (cur * 2 + 0) * D_TILE;
      const uint4* lb = lds + (cur * 2 + 1) * D_TILE;
      // a lane's 32 elements: FP8 the chunks h (block 0) and 2 + h (block 1) of its row, FP4 chunk
      // 2s + h of k-step s
      auto frag = [&](const uint4* t, int row, int c) {
        i32x8 f = {};
        const uint4 lo = t[dswz(row, c)];
        f[0] = (int)lo.x, f[1] = (int)lo.y, f[2] = (int)lo.z, f[3] = (int)lo.w;
        if (!FP4) {
          const uint4 hi = t[dswz(row, c + 2)];
          f[4] = (int)hi.x, f[5] = (int)hi.y, f[6] = (int)hi.z, f[7] = (int)hi.w;
        }
        return f;
      };
#pragma unroll
      for (int s = 0; s < EPB; ++s) {
        const int c = FP4 ? 2 * s + lh : lh;
        i32x8 af[4], bf[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = frag(la, wm * 128 + i * 32 + lr, c);
#pragma unroll
        for (int j = 0; j < 2; ++j) bf[j] = frag(lb, wn * 64 + j * 32 + lr, c);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = s == 0 ? mx_mfma<FMT, 0>(af[i], bf[j], acc[i][j], sa[i], sb[j])
                               : mx_mfma<FMT, 2>(af[i], bf[j], acc[i][j], sa[i], sb[j]);
        __builtin_amdgcn_s_setprio(0);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) sa[i] = na[i];
#pragma unroll
    for (int j = 0; j < 2; ++j) sb[j] = nb[j];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // C/D map of 32x32: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  unsigned bad = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = tn * G_BN + wn * 64 + j * 32 + lr;
      const int rbase = tm * G_BM + wm * 128 + i * 32 + 4 * lh;
      if (VERIFY) {
        const int c21 = col % MX_COLS;
        const int r15 = rbase % MX_ROWS;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rr = (r15 + (r & 3) + 8 * (r >> 2)) % MX_ROWS;
          bad += acc[i][j][r] != expect[rr * MX_COLS + c21];
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
void mx_launch_gemm(int fmt, int nwg, hipStream_t stream, Args... args) {
  if (fmt == ODH_MX_FP4)
    mx_gemm256_kernel<ODH_MX_FP4, VERIFY><<<nwg, G_THREADS, 0, stream>>>(args...);
  else if (fmt == ODH_MX_BF8)
    mx_gemm256_kernel<ODH_MX_BF8, VERIFY><<<nwg, G_THREADS, 0, stream>>>(args...);
  else if (fmt == ODH_MX_FP6)
    mx_gemm256_kernel<ODH_MX_FP6, VERIFY><<<nwg, G_THREADS, 0, stream>>>(args...);
  else if (fmt == ODH_MX_BF6)
    mx_gemm256_kernel<ODH_MX_BF6, VERIFY><<<nwg, G_THREADS, 0, stream>>>(args...);
  else
    mx_gemm256_kernel<ODH_MX_FP8, VERIFY><<<nwg, G_THREADS, 0, stream>>>(args...);
}

// host side: what the MX entry points take.  The scale rows are read 2 (FP8, BF8) or 4 bytes
// at a time, so the scale pointers are 4-byte aligned and K/32 is even (FP8, BF8) or a multiple of 4.
bool mx_ok(int fmt, int M, int N, int K) {
  return mx_fmt_ok(fmt) && M > 0 && N > 0 && K > 0 && M % G_BM == 0 && N % G_BN == 0 && K % mx_bk(fmt) == 0;
}
bool mx_aligned(const void* a, const void* b, const void* sa, const void* sb) {
  return a && b && sa && sb && (((uintptr_t)a | (uintptr_t)b) & 15) == 0 && (((uintptr_t)sa | (uintptr_t)sb) & 3) == 0;
}
