// The start-up probe's LDS step: the 160 KiB of on-chip SRAM of every CU, the transposing LDS reads that
// CDNA4 added, and the paths that move a value from one lane of a wave to another:
//   mem    every dword of the CU's 163,840 bytes, four passes, written 16 bytes wide and read 4 bytes wide by
//          another wave, and the reverse (ds_write_b128 / ds_read_b32, ds_write_b32 / ds_read_b128);
//   tr16   ds_read_b64_tr_b16      tr8   ds_read_b64_tr_b8      tr4   ds_read_b64_tr_b4      tr6   ds_read_b96_tr_b6
//   xlane  ds_bpermute_b32, ds_permute_b32, ds_swizzle_b32, the DPP row operations, v_readlane_b32,
//          v_writelane_b32, v_permlane16_swap_b32, v_permlane32_swap_b32.
// A fault in any of them gives wrong operands with no error.
//
// Included by gpu_probe.hip inside its anonymous namespace, after gpu_probe_cvt.h: it uses xcc_id.
//
// Rules every kernel here keeps: all LDS is the one extern __shared__ region below, 16-byte aligned, no static
// __shared__; a transposing read is never inside a divergent branch and the workgroups are whole waves (the
// gather crosses lanes, so EXEC must be all ones: every lane gets an address inside the image and what is not
// needed is discarded); every transposing-read address has the instruction's alignment (LdsTr::align); no
// workgroup waits for another.  A fused check launches ODH_LDS_BLOCKS workgroups of 256 threads that each
// claim more than half of a CU's LDS (mem: all of it), so a CU takes one workgroup and each SIMD one wave.
//
// The data-only fault.  odh_lds_fill writes a table of 256 key dwords, lds_key(check, i).  What a kernel
// stores to LDS or holds in a lane is a closed form of its position XOR a fold of key[index mod 256] READ FROM
// THE TABLE (ordinary global loads); what it compares with uses lds_key computed in registers.  A healthy run
// counts 0; with one table byte changed every compared element that uses that key dword is a mismatch:
// odh_lds_fault_count.  The fold to an element's width is the XOR of the key's pieces of that width, so in the
// 32-, 16- and 8-bit checks any change of a byte counts; a 4- or 6-bit element takes the XOR of the key's eight
// nibbles, which a change misses when it is the same in both nibbles of the byte: the fault hooks flip bit 0.
//
// The lane maps of the transposing reads, per group of 16 consecutive lanes (lane i = 0 … 15 of the group):
// see LdsTr and lds_tr_spec below; profiles/lds_probe/SUMMARY.txt has the measurement.
//
// DPP controls: the compiler accepts every one asked for on gfx950 (quad_perm, row_shl / row_shr / row_ror
// 1 … 15, row_mirror, row_half_mirror, row_bcast:15, row_bcast:31); none is refused.  There is no builtin for
// v_writelane_b32: it is inline assembly behind an s_nop 4 (its lane select and data come from scalar
// registers that a VALU instruction may just have written).

#define ODH_LDS_AS __attribute__((address_space(3)))
extern __shared__ __attribute__((aligned(16))) unsigned char lds_smem[];

typedef __attribute__((ext_vector_type(4))) short lds_s16x4;
typedef __attribute__((ext_vector_type(2))) int lds_i32x2;
typedef __attribute__((ext_vector_type(3))) int lds_i32x3;

constexpr int LDS_CU_BYTES = 160 * 1024;  // the whole LDS of a CU: the mem check's claim
constexpr int LDS_TR_BYTES = 96 * 1024;   // the other checks': more than half, so a CU takes one workgroup
constexpr int LDS_WAVES = 4;

__host__ __device__ constexpr bool lds_check_ok(int check) { return check >= ODH_LDS_MEM && check <= ODH_LDS_XLANE; }
__host__ __device__ constexpr bool lds_is_tr(int check) { return check >= ODH_LDS_TR16 && check <= ODH_LDS_TR6; }

__host__ __device__ constexpr uint32_t lds_mix(uint32_t x) {
  x ^= x >> 16, x *= 0x7FEB352Du, x ^= x >> 15, x *= 0x846CA68Bu, x ^= x >> 16;
  return x;
}
// key dword i of a check's table
__host__ __device__ constexpr uint32_t lds_key(int check, uint32_t i) {
  return lds_mix(0x9E3779B9u * (i + 1) + 0x85EBCA6Bu * (uint32_t)(check + 1));
}
// a key folded to an element of `bits` bits: the XOR of its pieces (4 and 6 bits: of its eight nibbles)
__host__ __device__ constexpr uint32_t lds_fold(uint32_t k, int bits) {
  if (bits >= 32) return k;
  k ^= k >> 16;
  if (bits == 16) return k & 0xFFFFu;
  k ^= k >> 8;
  if (bits == 8) return k & 0xFFu;
  return (k ^ k >> 4) & 0xFu;
}

__global__ void lds_fill_kernel(int check, uint32_t* __restrict__ table) { table[threadIdx.x] = lds_key(check, threadIdx.x); }

// workgroups per XCD, and the CU the workgroup runs on into the bitmap: bit (XCC_ID, SE_ID, SH_ID, CU_ID) of
// ODH_LDS_CU_WORDS dwords, with a vector atomic
__device__ __forceinline__ unsigned lds_book_block(int* xcd_blocks, unsigned* cu_bitmap) {
  const unsigned xcc = xcc_id();
  if (threadIdx.x == 0) {
    unsigned hw;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    // HW_ID: CU_ID in bits 8-11, SH_ID in bit 12, SE_ID in bits 13-15
    const unsigned cu = xcc << 8 | (hw >> 8 & 0xFFu);
    atomicAdd(&xcd_blocks[xcc], 1);
    atomicOr(&cu_bitmap[cu >> 5], 1u << (cu & 31));
  }
  return xcc;
}
__device__ __forceinline__ void lds_book_errors(unsigned bad, unsigned xcc, unsigned* err_total, unsigned* err_xcd) {
  for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
  if ((threadIdx.x & 63) == 0 && bad) {
    atomicAdd(err_total, bad);
    atomicAdd(&err_xcd[xcc], bad);
  }
}

// ------------------------------------------------------------------ mem
//
// Dword w of the 40,960, pass p: even p stores lds_mix(w, p) ^ key[(w + 37 p) mod 256], odd p the complement of
// pass p - 1 (with its key), so every bit of every word is written as 0 and as 1.  Even passes write ds_write_b128 (thread t
// of the workgroup the uint4 256 i + t, i = 0 … 39) and read ds_read_b32; odd passes write ds_write_b32 and
// read ds_read_b128.  Of the 1,024 dwords of an i, wave v wrote (or writes) [256 v, 256 v + 256) and reads
// those of wave (v + 1 + i mod 3) mod 4: a rotation by 1, 2 or 3, so every dword is read once, by another
// wave than wrote it, behind the barrier.  The four kinds of access are inline assembly, so that each is the
// instruction it says (the compiler would pair the 4-byte ones into ds_read2st64_b32).
constexpr int LDS_MEM_DWORDS = LDS_CU_BYTES / 4;
constexpr int LDS_MEM_ITERS = LDS_MEM_DWORDS / 1024;
constexpr int LDS_MEM_PASSES = 4;
__host__ __device__ constexpr uint32_t lds_mem_kidx(uint32_t w, int pass) { return (w + 37u * (uint32_t)(pass & ~1)) & 255u; }
__host__ __device__ constexpr uint32_t lds_mem_value(uint32_t w, int pass, uint32_t key) {
  const uint32_t v = lds_mix(w * 0x9E3779B1u + (uint32_t)(pass & ~1) * 0x632BE5ABu + 1u) ^ key;
  return pass & 1 ? ~v : v;
}
__host__ __device__ constexpr int lds_mem_reads_wave(int wave, int i) { return (wave + 1 + i % 3) & 3; }

__global__ __launch_bounds__(256, 1) void lds_mem_kernel(const uint32_t* __restrict__ table, int* __restrict__ xcd_blocks,
                                                         unsigned* __restrict__ err_total,
                                                         unsigned* __restrict__ err_xcd,
                                                         unsigned* __restrict__ cu_bitmap) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned xcc = lds_book_block(xcd_blocks, cu_bitmap);
  const uint32_t base = (uint32_t)(uintptr_t)(ODH_LDS_AS unsigned char*)lds_smem;
  unsigned bad = 0;
  for (int pass = 0; pass < LDS_MEM_PASSES; ++pass) {
    // the four keys of a lane's 4-byte accesses (dwords 64 c + lane of a wave's 256) and of its 16-byte ones
    // (dwords 4 lane + e): neither depends on i or on the wave, 256 divides both strides
    uint32_t k4[4], k16[4], want4[4], want16[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      k4[c] = table[lds_mem_kidx(64 * c + lane, pass)], want4[c] = lds_key(ODH_LDS_MEM, lds_mem_kidx(64 * c + lane, pass));
      k16[c] = table[lds_mem_kidx(4 * lane + c, pass)], want16[c] = lds_key(ODH_LDS_MEM, lds_mem_kidx(4 * lane + c, pass));
    }
    if ((pass & 1) == 0) {
      for (int i = 0; i < LDS_MEM_ITERS; ++i) {
        const uint32_t w = 1024u * i + 256u * wave + 4u * lane;
        const u32x4 v = {lds_mem_value(w, pass, k16[0]), lds_mem_value(w + 1, pass, k16[1]),
                         lds_mem_value(w + 2, pass, k16[2]), lds_mem_value(w + 3, pass, k16[3])};
        asm volatile("ds_write_b128 %0, %1" : : "v"(base + 4 * w), "v"(v) : "memory");
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __syncthreads();
      for (int i = 0; i < LDS_MEM_ITERS; ++i) {
        const uint32_t w = 1024u * i + 256u * lds_mem_reads_wave(wave, i) + lane;
        uint32_t r0, r1, r2, r3;
        asm volatile(
            "ds_read_b32 %0, %4\n\tds_read_b32 %1, %4 offset:256\n\tds_read_b32 %2, %4 offset:512\n\t"
            "ds_read_b32 %3, %4 offset:768\n\ts_waitcnt lgkmcnt(0)"
            : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3)
            : "v"(base + 4 * w)
            : "memory");
        bad += r0 != lds_mem_value(w, pass, want4[0]);
        bad += r1 != lds_mem_value(w + 64, pass, want4[1]);
        bad += r2 != lds_mem_value(w + 128, pass, want4[2]);
        bad += r3 != lds_mem_value(w + 192, pass, want4[3]);
      }
    } else {
      for (int i = 0; i < LDS_MEM_ITERS; ++i) {
        const uint32_t w = 1024u * i + 256u * wave + lane;
        asm volatile(
            "ds_write_b32 %0, %1\n\tds_write_b32 %0, %2 offset:256\n\tds_write_b32 %0, %3 offset:512\n\t"
            "ds_write_b32 %0, %4 offset:768"
            :
            : "v"(base + 4 * w), "v"(lds_mem_value(w, pass, k4[0])), "v"(lds_mem_value(w + 64, pass, k4[1])),
              "v"(lds_mem_value(w + 128, pass, k4[2])), "v"(lds_mem_value(w + 192, pass, k4[3]))
            : "memory");
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __syncthreads();
      for (int i = 0; i < LDS_MEM_ITERS; ++i) {
        const uint32_t w = 1024u * i + 256u * lds_mem_reads_wave(wave, i) + 4u * lane;
        u32x4 r;
        asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(r) : "v"(base + 4 * w) : "memory");
#pragma unroll
        for (int e = 0; e < 4; ++e) bad += r[e] != lds_mem_value(w + e, pass, want16[e]);
      }
    }
    __syncthreads();  // the next pass overwrites what other waves have just read
  }
  lds_book_errors(bad, xcc, err_total, err_xcd);
}

// ------------------------------------------------------------------ the transposing reads
//
// One instruction moves, per group of 16 lanes, a block of `rows` rows × 16 columns of `bits`-bit elements:
// 64 bits per lane (tr_b6: 96).  A block row is 16 elements, 2 `bits` bytes, and `16 / rows` lanes supply
// its address, 8 bytes each (tr_b4: one lane, its 8 bytes; tr_b6: one lane, its 12 bytes).  Lane
// (16 / rows) q + p of the group supplies the address of row q, piece p; lane i receives column i, row q in
// bits [bits q, bits q + bits) of its result.
// tr_b6 rows: the 12 bytes of a block row live in a slot of 16, so that every address is 16-byte aligned:
// the staging store re-pitches packed rows (12-byte pieces to 16-byte slots); `slot` is that size.
struct LdsTr {
  int bits;   // of an element
  int rows;   // of a block
  int align;  // of every lane's address, bytes
  int slot;   // bytes a block row occupies in the image
  int words;  // result dwords per lane
};
__host__ __device__ constexpr LdsTr lds_tr_spec(int check) {
  switch (check) {
    case ODH_LDS_TR16: return {16, 4, 8, 32, 2};
    case ODH_LDS_TR8: return {8, 8, 8, 16, 2};
    case ODH_LDS_TR4: return {4, 16, 8, 8, 2};
    default: return {6, 16, 16, 16, 3};  // ODH_LDS_TR6
  }
}
// byte offset of the address lane i of a group supplies, from the block's first byte, at this row pitch
__host__ __device__ constexpr uint32_t lds_tr_lane_offset(LdsTr s, int i, uint32_t pitch) {
  const int lpr = 16 / s.rows;
  return (uint32_t)(i / lpr) * pitch + (uint32_t)(i % lpr) * 8u;
}

struct LdsTrOut {
  uint32_t w[3];
};
template <int CHECK>
__device__ __forceinline__ LdsTrOut lds_tr_read(uint32_t byte_offset) {
  unsigned char* p = lds_smem + byte_offset;
  LdsTrOut o = {{0, 0, 0}};
  if constexpr (CHECK == ODH_LDS_TR16) {
    const lds_i32x2 v = __builtin_bit_cast(lds_i32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((ODH_LDS_AS lds_s16x4*)p));
    o.w[0] = v[0], o.w[1] = v[1];
  } else if constexpr (CHECK == ODH_LDS_TR8) {
    const lds_i32x2 v = __builtin_amdgcn_ds_read_tr8_b64_v2i32((ODH_LDS_AS lds_i32x2*)p);
    o.w[0] = v[0], o.w[1] = v[1];
  } else if constexpr (CHECK == ODH_LDS_TR4) {
    const lds_i32x2 v = __builtin_amdgcn_ds_read_tr4_b64_v2i32((ODH_LDS_AS lds_i32x2*)p);
    o.w[0] = v[0], o.w[1] = v[1];
  } else {
    const lds_i32x3 v = __builtin_amdgcn_ds_read_tr6_b96_v3i32((ODH_LDS_AS lds_i32x3*)p);
    o.w[0] = v[0], o.w[1] = v[1], o.w[2] = v[2];
  }
  return o;
}
// element q of a lane's result
__device__ __forceinline__ uint32_t lds_tr_element(const LdsTrOut& o, int bits, int q) {
  const int at = bits * q;
  const uint64_t two = (uint64_t)o.w[at >> 5] | (uint64_t)o.w[(at >> 5) + ((at >> 5) < 2)] << 32;
  return (uint32_t)(two >> (at & 31)) & ((1u << bits) - 1u);
}

struct LdsLaneAddr {
  uint32_t a[64];
};
// the measuring tool: one wave, one instruction; lane l reads at a[l] and stores its result dwords at out
template <int CHECK>
__global__ __launch_bounds__(64) void lds_tr_read_kernel(const uint32_t* __restrict__ image, unsigned bytes, LdsLaneAddr addr,
                                                        uint32_t* __restrict__ out) {
  const int lane = threadIdx.x;
  for (unsigned i = lane; i < bytes / 4; i += 64) reinterpret_cast<uint32_t*>(lds_smem)[i] = image[i];
  __syncthreads();
  const LdsTrOut o = lds_tr_read<CHECK>(addr.a[lane]);
  constexpr int W = lds_tr_spec(CHECK).words;
#pragma unroll
  for (int w = 0; w < W; ++w) out[W * lane + w] = o.w[w];
}

// The fused check.  Each wave owns a quarter of the workgroup's LDS and keeps an image there of 64 columns
// and 4 blocks of rows (16 blocks), a row of a block in its slot: element (r, c) of round n holds
//   (lds_mix(n, r, c) >> 7 ^ fold(key[(64 r + c + 17 n) mod 256])) mod 2^bits.
// A round is a row pitch (the image row's bytes, that plus the alignment, which is no power of two, and
// twice that) and a base (every aligned position of a 256-byte bank row); per round the wave reads all 16
// blocks, each group of lanes another block in every read (group g, read j: block (j + 5 g) mod 16), and
// compares every element it gets with the closed form of the (row, column) the lane map gives it: over the 16
// reads of a round every group reads every block.
constexpr int LDS_TR_COLS = 64;
__host__ __device__ constexpr int lds_tr_image_rows(LdsTr s) { return 4 * s.rows; }
__host__ __device__ constexpr int lds_tr_row_bytes(LdsTr s) { return LDS_TR_COLS / 16 * s.slot; }
__host__ __device__ constexpr int lds_tr_positions(LdsTr s) { return 256 / s.align; }
__host__ __device__ constexpr int lds_tr_rounds(LdsTr s) { return 3 * lds_tr_positions(s); }
__host__ __device__ constexpr uint32_t lds_tr_pitch(LdsTr s, int round) {
  const int rb = lds_tr_row_bytes(s), pi = round / lds_tr_positions(s);
  return (uint32_t)(pi == 0 ? rb : pi == 1 ? rb + s.align : 2 * rb);
}
__host__ __device__ constexpr uint32_t lds_tr_base(LdsTr s, int round) {
  return (uint32_t)(round % lds_tr_positions(s) * s.align);
}
__host__ __device__ constexpr uint32_t lds_tr_kidx(int r, int c, int round) {
  return (uint32_t)(64 * r + c + 17 * round) & 255u;
}
__host__ __device__ constexpr uint32_t lds_tr_value(int check, int r, int c, int round, uint32_t key) {
  const int bits = lds_tr_spec(check).bits;
  const uint32_t h = lds_mix((uint32_t)((round * 64 + r) * 64 + c) * 0x9E3779B1u + (uint32_t)check);
  return (h >> 7 ^ lds_fold(key, bits)) & ((1u << bits) - 1u);
}

template <int CHECK>
__global__ __launch_bounds__(256, 1) void lds_tr_kernel(const uint32_t* __restrict__ table, int* __restrict__ xcd_blocks,
                                                        unsigned* __restrict__ err_total,
                                                        unsigned* __restrict__ err_xcd,
                                                        unsigned* __restrict__ cu_bitmap) {
  constexpr LdsTr S = lds_tr_spec(CHECK);
  constexpr int ROWS = lds_tr_image_rows(S), PER_SLOT = 16, SLOT_WORDS = S.slot / 4, DATA_WORDS = 2 * S.bits / 4;
  constexpr int SLOTS = ROWS * (LDS_TR_COLS / 16);  // 64, 128 or 256: whole waves
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned xcc = lds_book_block(xcd_blocks, cu_bitmap);
  const uint32_t region = (uint32_t)wave * (LDS_TR_BYTES / LDS_WAVES);
  unsigned bad = 0;
  for (int round = 0; round < lds_tr_rounds(S); ++round) {
    const uint32_t pitch = lds_tr_pitch(S, round), image = region + lds_tr_base(S, round);
    // the image: a lane builds whole slots, 16 elements each, from the table's keys
    for (int slot = lane; slot < SLOTS; slot += 64) {
      const int r = slot / (LDS_TR_COLS / 16), cb = slot % (LDS_TR_COLS / 16);
      uint32_t w[8] = {};
#pragma unroll
      for (int e = 0; e < PER_SLOT; ++e) {
        const int c = 16 * cb + e, at = S.bits * e;
        const uint32_t v = lds_tr_value(CHECK, r, c, round, table[lds_tr_kidx(r, c, round)]);
        w[at >> 5] |= v << (at & 31);
        if ((at & 31) + S.bits > 32) w[(at >> 5) + 1] |= v >> (32 - (at & 31));
      }
      uint32_t* dst = reinterpret_cast<uint32_t*>(lds_smem + image + (uint32_t)r * pitch + (uint32_t)cb * S.slot);
#pragma unroll
      for (int k = 0; k < SLOT_WORDS; ++k) dst[k] = k < DATA_WORDS ? w[k] : 0u;
    }
    __syncthreads();
    const int g = lane >> 4, i = lane & 15;
    for (int j = 0; j < 16; ++j) {
      const int b = (j + 5 * g) & 15, r0 = (b >> 2) * S.rows, cb = b & 3;
      const LdsTrOut o = lds_tr_read<CHECK>(image + (uint32_t)r0 * pitch + (uint32_t)cb * S.slot + lds_tr_lane_offset(S, i, pitch));
#pragma unroll
      for (int q = 0; q < S.rows; ++q) {
        const int r = r0 + q, c = 16 * cb + i;
        bad += lds_tr_element(o, S.bits, q) != lds_tr_value(CHECK, r, c, round, lds_key(CHECK, lds_tr_kidx(r, c, round)));
      }
    }
    __syncthreads();  // uniform: every wave runs every round
  }
  lds_book_errors(bad, xcc, err_total, err_xcd);
}

// ------------------------------------------------------------------ lane exchange
//
// op (LDS_XL_*) and arg select one exchange of the 64 values x (the swaps: of the 128 values x, y: value
// 64 + l is lane l's y).  lds_xl_src is the value index that lane l ends up with (the swaps: result index
// 0 … 127 as well), one function for the host and the kernels:
//   BPERMUTE / PERMUTE   arg 0 … 63: lane l reads from (sends to) lane (l + arg) mod 64; arg 64: the bit
//                        reversal of l
//   SWIZZLE              arg indexes lds_swizzle_pattern: swaps, reversals, broadcasts, quad permutations
//   DPP                  arg indexes lds_dpp_ctrl; row_mask and bank_mask 0xF, bound_ctrl off, old = x: a
//                        lane without a source keeps its own value
//   READLANE             arg = the lane every lane reads
//   WRITELANE            lane arg gets lane (arg + 1) mod 64's value, the others keep theirs
//   PERMLANE16_SWAP / PERMLANE32_SWAP   arg = fi | bound_ctrl << 1
enum {
  LDS_XL_BPERMUTE = 0,
  LDS_XL_PERMUTE = 1,
  LDS_XL_SWIZZLE = 2,
  LDS_XL_DPP = 3,
  LDS_XL_READLANE = 4,
  LDS_XL_WRITELANE = 5,
  LDS_XL_PERMLANE16_SWAP = 6,
  LDS_XL_PERMLANE32_SWAP = 7,
  LDS_XL_OPS = 8,
  LDS_XL_NSWIZZLE = 12,
  LDS_XL_NDPP = 55,
};
// bit-mask mode: and_mask in bits 0-4, or_mask in 5-9, xor_mask in 10-14, inside each half of 32 lanes; bit
// 15: quad-permutation mode, two bits per lane of a quad
__host__ __device__ constexpr int lds_swizzle_pattern(int i) {
  constexpr int P[LDS_XL_NSWIZZLE] = {0x041F, 0x081F, 0x101F, 0x201F, 0x401F,  // swap 1, 2, 4, 8, 16
                                      0x7C1F, 0x0C1F, 0x1C1F,                  // reverse 32, 4, 8
                                      0x0000, 0x03E0, 0x0078,                  // broadcast lane 0, 31, 3 of every 8
                                      0x801B};                                 // quad_perm [3,2,1,0]
  return P[i];
}
// quad_perm six times, row_shl / row_shr / row_ror 1 … 15, row_mirror, row_half_mirror, row_bcast:15, row_bcast:31
__host__ __device__ constexpr int lds_dpp_ctrl(int i) {
  constexpr int Q[6] = {0x1B, 0xB1, 0x4E, 0x00, 0xFF, 0x39};
  return i < 6 ? Q[i] : i < 21 ? 0x101 + (i - 6) : i < 36 ? 0x111 + (i - 21) : i < 51 ? 0x121 + (i - 36) : 0x140 + (i - 51);
}
__host__ __device__ constexpr int lds_xl_args(int op) {
  switch (op) {
    case LDS_XL_BPERMUTE:
    case LDS_XL_PERMUTE: return 65;
    case LDS_XL_SWIZZLE: return LDS_XL_NSWIZZLE;
    case LDS_XL_DPP: return LDS_XL_NDPP;
    case LDS_XL_READLANE:
    case LDS_XL_WRITELANE: return 64;
    case LDS_XL_PERMLANE16_SWAP:
    case LDS_XL_PERMLANE32_SWAP: return 4;
    default: return 0;
  }
}
__host__ __device__ constexpr bool lds_xl_pair(int op) { return op == LDS_XL_PERMLANE16_SWAP || op == LDS_XL_PERMLANE32_SWAP; }
__host__ __device__ constexpr int lds_bitrev6(int l) {
  return (l & 1) << 5 | (l & 2) << 3 | (l & 4) << 1 | (l & 8) >> 1 | (l & 16) >> 3 | (l & 32) >> 5;
}
__host__ __device__ constexpr int lds_xl_select(int arg, int l) { return arg < 64 ? (l + arg) & 63 : lds_bitrev6(l); }
__host__ __device__ constexpr int lds_swizzle_src(int pattern, int l) {
  if (pattern & 0x8000) return (l & ~3) | (pattern >> (2 * (l & 3)) & 3);
  const int a = pattern & 31, o = pattern >> 5 & 31, x = pattern >> 10 & 31;
  return (l & 32) | ((((l & 31) & a) | o) ^ x);
}
__host__ __device__ constexpr int lds_dpp_src(int ctrl, int l) {
  const int row = l & ~15, i = l & 15, n = ctrl & 15;
  if (ctrl < 0x100) return (l & ~3) | (ctrl >> (2 * (l & 3)) & 3);
  if (ctrl < 0x110) return i + n < 16 ? l + n : l;             // row_shl: from the lane n above
  if (ctrl < 0x120) return i >= n ? l - n : l;                 // row_shr: from the lane n below
  if (ctrl < 0x130) return row | ((i - n) & 15);               // row_ror
  if (ctrl == 0x140) return row | (15 - i);                    // row_mirror
  if (ctrl == 0x141) return (l & ~7) | (7 - (l & 7));          // row_half_mirror
  if (ctrl == 0x142) return l >= 16 ? row - 1 : l;             // row_bcast:15: lane 15 of the row below
  return l >= 32 ? 31 : l;                                     // row_bcast:31: lane 31, to rows 2 and 3
}
// result index t (0 … 63: x after; 64 … 127: y after, the swaps only) holds value index lds_xl_src
__host__ __device__ constexpr int lds_xl_src(int op, int arg, int t) {
  const int l = t & 63;
  switch (op) {
    case LDS_XL_BPERMUTE: return lds_xl_select(arg, l);
    case LDS_XL_PERMUTE: return arg < 64 ? (l - arg) & 63 : lds_bitrev6(l);
    case LDS_XL_SWIZZLE: return lds_swizzle_src(lds_swizzle_pattern(arg), l);
    case LDS_XL_DPP: return lds_dpp_src(lds_dpp_ctrl(arg), l);
    case LDS_XL_READLANE: return arg;
    case LDS_XL_WRITELANE: return l == arg ? (arg + 1) & 63 : l;
    case LDS_XL_PERMLANE16_SWAP:  // x's odd rows of 16 change places with y's even rows
      return t < 64 ? (l & 16 ? 64 + l - 16 : l) : (l & 16 ? 64 + l : l + 16);
    default:  // PERMLANE32_SWAP: x's upper half changes places with y's lower half
      return t < 64 ? (l & 32 ? 64 + l - 32 : l) : (l & 32 ? 64 + l : l + 32);
  }
}

template <int... I>
__device__ __forceinline__ uint32_t lds_swizzle_sel(int arg, uint32_t x, std::integer_sequence<int, I...>) {
  uint32_t r = x;
  ((arg == I ? (void)(r = (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, lds_swizzle_pattern(I))) : (void)0), ...);
  return r;
}
template <int... I>
__device__ __forceinline__ uint32_t lds_dpp_sel(int arg, uint32_t x, std::integer_sequence<int, I...>) {
  uint32_t r = x;
  ((arg == I ? (void)(r = (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, lds_dpp_ctrl(I), 0xF, 0xF, false)) : (void)0), ...);
  return r;
}
struct LdsPair {
  uint32_t x, y;
};
template <bool FI, bool BC>
__device__ __forceinline__ LdsPair lds_swap16(uint32_t x, uint32_t y) {
  const auto r = __builtin_amdgcn_permlane16_swap(x, y, FI, BC);
  return {r[0], r[1]};
}
template <bool FI, bool BC>
__device__ __forceinline__ LdsPair lds_swap32(uint32_t x, uint32_t y) {
  const auto r = __builtin_amdgcn_permlane32_swap(x, y, FI, BC);
  return {r[0], r[1]};
}
// one exchange; op and arg are uniform over the wave
__device__ __forceinline__ LdsPair lds_xl_exchange(int op, int arg, int lane, uint32_t x, uint32_t y) {
  switch (op) {
    case LDS_XL_BPERMUTE: return {(uint32_t)__builtin_amdgcn_ds_bpermute(4 * lds_xl_select(arg, lane), (int)x), y};
    case LDS_XL_PERMUTE: return {(uint32_t)__builtin_amdgcn_ds_permute(4 * lds_xl_select(arg, lane), (int)x), y};
    case LDS_XL_SWIZZLE: return {lds_swizzle_sel(arg, x, std::make_integer_sequence<int, LDS_XL_NSWIZZLE>{}), y};
    case LDS_XL_DPP: return {lds_dpp_sel(arg, x, std::make_integer_sequence<int, LDS_XL_NDPP>{}), y};
    case LDS_XL_READLANE: return {(uint32_t)__builtin_amdgcn_readlane((int)x, arg), y};
    case LDS_XL_WRITELANE: {
      const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)x, (arg + 1) & 63);
      // two scalar registers do not fit one instruction's constant bus: the lane select goes through M0
      unsigned keep;
      asm volatile("s_mov_b32 %1, m0\n\ts_mov_b32 m0, %3\n\ts_nop 4\n\tv_writelane_b32 %0, %2, m0\n\ts_mov_b32 m0, %1"
                   : "+v"(x), "=&s"(keep)
                   : "s"(v), "s"(arg));
      return {x, y};
    }
    case LDS_XL_PERMLANE16_SWAP:
      return arg == 0 ? lds_swap16<false, false>(x, y) : arg == 1 ? lds_swap16<true, false>(x, y)
             : arg == 2 ? lds_swap16<false, true>(x, y) : lds_swap16<true, true>(x, y);
    default:
      return arg == 0 ? lds_swap32<false, false>(x, y) : arg == 1 ? lds_swap32<true, false>(x, y)
             : arg == 2 ? lds_swap32<false, true>(x, y) : lds_swap32<true, true>(x, y);
  }
}

__global__ __launch_bounds__(64) void lds_xlane_one_kernel(int op, int arg, const uint32_t* __restrict__ in,
                                                           uint32_t* __restrict__ out) {
  const int lane = threadIdx.x;
  const bool pair = lds_xl_pair(op);
  const LdsPair r = lds_xl_exchange(op, arg, lane, in[lane], pair ? in[64 + lane] : 0u);
  out[lane] = r.x;
  if (pair) out[64 + lane] = r.y;
}

// The fused check: every wave runs every exchange, LDS_XL_REPEAT times with other values (the launch claims
// LDS_TR_BYTES so that a CU takes one workgroup; the kernel itself stores nothing there).  Value index s
// (0 … 127) of exchange number e holds lds_mix(e, s) ^ key[(s + 67 e) mod 256]; after the exchange result
// index t is compared with the closed form of lds_xl_src(t).
constexpr int LDS_XL_REPEAT = 16;
__host__ __device__ constexpr uint32_t lds_xl_kidx(int s, int e) { return (uint32_t)(s + 67 * e) & 255u; }
__host__ __device__ constexpr uint32_t lds_xl_value(int s, int e, uint32_t key) {
  return lds_mix((uint32_t)(e * 128 + s) * 0x9E3779B1u + 0x51u) ^ key;
}

__global__ __launch_bounds__(256, 1) void lds_xlane_kernel(const uint32_t* __restrict__ table, int* __restrict__ xcd_blocks,
                                                           unsigned* __restrict__ err_total,
                                                           unsigned* __restrict__ err_xcd,
                                                           unsigned* __restrict__ cu_bitmap) {
  const int lane = threadIdx.x & 63;
  const unsigned xcc = lds_book_block(xcd_blocks, cu_bitmap);
  unsigned bad = 0;
  int e = 0;
  for (int rep = 0; rep < LDS_XL_REPEAT; ++rep)
    for (int op = 0; op < LDS_XL_OPS; ++op)
      for (int arg = 0; arg < lds_xl_args(op); ++arg, ++e) {
        const uint32_t x = lds_xl_value(lane, e, table[lds_xl_kidx(lane, e)]);
        const uint32_t y = lds_xl_value(64 + lane, e, table[lds_xl_kidx(64 + lane, e)]);
        const LdsPair r = lds_xl_exchange(op, arg, lane, x, y);
        const int sx = lds_xl_src(op, arg, lane);
        bad += r.x != lds_xl_value(sx, e, lds_key(ODH_LDS_XLANE, lds_xl_kidx(sx, e)));
        if (lds_xl_pair(op)) {
          const int sy = lds_xl_src(op, arg, 64 + lane);
          bad += r.y != lds_xl_value(sy, e, lds_key(ODH_LDS_XLANE, lds_xl_kidx(sy, e)));
        }
      }
  lds_book_errors(bad, xcc, err_total, err_xcd);
}

// ------------------------------------------------------------------ host side

// compared elements of one workgroup that use key dword k (k < 0: all of them)
unsigned long long lds_block_cases(int check, int k) {
  unsigned long long n = 0;
  if (check == ODH_LDS_MEM) {
    for (int pass = 0; pass < LDS_MEM_PASSES; ++pass)
      for (uint32_t w = 0; w < (uint32_t)LDS_MEM_DWORDS; ++w) n += k < 0 || (int)lds_mem_kidx(w, pass) == k;
  } else if (lds_is_tr(check)) {
    // every element of the image is delivered to each of the four groups of lanes once per round and wave
    const LdsTr s = lds_tr_spec(check);
    for (int round = 0; round < lds_tr_rounds(s); ++round)
      for (int r = 0; r < lds_tr_image_rows(s); ++r)
        for (int c = 0; c < LDS_TR_COLS; ++c) n += k < 0 || (int)lds_tr_kidx(r, c, round) == k;
    n *= 4 * LDS_WAVES;
  } else if (check == ODH_LDS_XLANE) {
    int e = 0;
    for (int rep = 0; rep < LDS_XL_REPEAT; ++rep)
      for (int op = 0; op < LDS_XL_OPS; ++op)
        for (int arg = 0; arg < lds_xl_args(op); ++arg, ++e)
          for (int t = 0; t < (lds_xl_pair(op) ? 128 : 64); ++t)
            n += k < 0 || (int)lds_xl_kidx(lds_xl_src(op, arg, t), e) == k;
    n *= LDS_WAVES;
  }
  return n;
}

template <typename... Args>
void lds_launch_probe(int check, hipStream_t stream, Args... args) {
  switch (check) {
    case ODH_LDS_MEM: lds_mem_kernel<<<ODH_LDS_BLOCKS, 256, LDS_CU_BYTES, stream>>>(args...); break;
    case ODH_LDS_TR16: lds_tr_kernel<ODH_LDS_TR16><<<ODH_LDS_BLOCKS, 256, LDS_TR_BYTES, stream>>>(args...); break;
    case ODH_LDS_TR8: lds_tr_kernel<ODH_LDS_TR8><<<ODH_LDS_BLOCKS, 256, LDS_TR_BYTES, stream>>>(args...); break;
    case ODH_LDS_TR4: lds_tr_kernel<ODH_LDS_TR4><<<ODH_LDS_BLOCKS, 256, LDS_TR_BYTES, stream>>>(args...); break;
    case ODH_LDS_TR6: lds_tr_kernel<ODH_LDS_TR6><<<ODH_LDS_BLOCKS, 256, LDS_TR_BYTES, stream>>>(args...); break;
    default: lds_xlane_kernel<<<ODH_LDS_BLOCKS, 256, LDS_TR_BYTES, stream>>>(args...); break;
  }
}
template <typename... Args>
void lds_launch_tr_read(int check, unsigned lds_bytes, hipStream_t stream, Args... args) {
  switch (check) {
    case ODH_LDS_TR16: lds_tr_read_kernel<ODH_LDS_TR16><<<1, 64, lds_bytes, stream>>>(args...); break;
    case ODH_LDS_TR8: lds_tr_read_kernel<ODH_LDS_TR8><<<1, 64, lds_bytes, stream>>>(args...); break;
    case ODH_LDS_TR4: lds_tr_read_kernel<ODH_LDS_TR4><<<1, 64, lds_bytes, stream>>>(args...); break;
    default: lds_tr_read_kernel<ODH_LDS_TR6><<<1, 64, lds_bytes, stream>>>(args...); break;
  }
}

// ------------------------------------------------------------------ the transposer of packed codes
//
// src [R][C] elements, row-major and packed, to dst [C][R] in the same packing; R and C multiples of 128.  A
// workgroup of four waves takes a tile of 128 × 128 elements: 16-byte global loads, coalesced along the source
// rows, staged through registers into an LDS image of the tile, read back with the format's transposing
// instruction, and 16-byte pieces of destination rows stored: a lane's 8 result bytes are 64 / bits elements
// of ONE destination row, so two reads of row blocks one above the other (tr_b6: four reads, 48 bytes) make
// whole 16-byte pieces.  Bit-exact by construction: no element is decoded.
//
// The image is the tile's rows at a padded pitch (LdsTc::pitch), computed with the bank rule (bank of byte a:
// (a / 4) mod 64 for the 8-byte transposing reads, whose lanes conflict inside a half of 32; mod 32 for the
// 16- and 12-byte stores, inside 8 consecutive lanes, and, it is assumed, for ds_read_b96_tr_b6 in
// ds_read_b96's sets of 8 lanes):
//   16 bit  rows of 256 B at pitch 288: a row starts 8 banks after the one above.  A group reads 4 rows × 32 B,
//           32 banks; the half's other group reads 4 or 12 rows further down in the same columns, the other 32.
//   8 bit   rows of 128 B at pitch 144, 36 banks: 16 rows × 16 B start at 36 q mod 64, the 16 multiples of 4.
//           The half's groups read blocks an odd number of blocks (8 rows) apart in the same columns.
//   4 bit   rows of 64 B at pitch 80, 20 banks: 16 rows × 8 B start at 20 q mod 64 = 4 (5 q mod 16), banks
//           4 m and 4 m + 1; the half's other group reads the next 16 columns, 8 B on: banks 4 m + 2, 4 m + 3.
//   6 bit   a row's eight 12-byte pieces in 16-byte slots, 128 B at pitch 144, 4 banks mod 32 per row: the
//           two groups that share sets of 8 lanes read the same columns 64 rows apart (64 · 36 = 0 mod 32),
//           rows 0-3 of one with rows 4-7 of the other: starts 0, 4, 8, 12 and 16, 20, 24, 28, 3 banks each.
// The staging stores: 8 consecutive lanes write 128 contiguous bytes of a row (16 bit, 8 bit), the 64 B of
// rows r and r + 4 (4 bit: banks 20 r … + 15 and 20 r + 80 … + 95 = 20 r + 16 … mod 32), or four rows' slots
// j and j + 4 (6 bit: starts 4 r + 16 half + 4 j mod 32): conflict-free each.  A padded pitch is no
// lane-linear image, so the LDS-DMA loads (global_load_lds_dwordx4) do not fit; the loads go through registers.
// tests/lds_reference.py recomputes every one of these sets of banks.
struct LdsTc {
  int check;  // the transposing read
  int pitch;  // bytes between rows of the LDS image
  int row;    // bytes of a tile row in global memory
};
__host__ __device__ constexpr LdsTc lds_tc_spec(int fmt) {
  switch (fmt) {
    case ODH_TC_B16: return {ODH_LDS_TR16, 288, 256};
    case ODH_TC_B8: return {ODH_LDS_TR8, 144, 128};
    case ODH_TC_B4: return {ODH_LDS_TR4, 80, 64};
    default: return {ODH_LDS_TR6, 144, 96};  // ODH_TC_B6
  }
}
__host__ __device__ constexpr bool lds_tc_ok(int fmt) { return fmt >= ODH_TC_B16 && fmt <= ODH_TC_B6; }
constexpr int LDS_TC_TILE = 128;

template <int FMT>
__global__ __launch_bounds__(256) void transpose_codes_kernel(const unsigned char* __restrict__ src,
                                                              unsigned char* __restrict__ dst, long R, long C) {
  constexpr LdsTc T = lds_tc_spec(FMT);
  constexpr LdsTr S = lds_tr_spec(T.check);
  constexpr int P = T.pitch;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, i = lane & 15;
  const long tiles_r = R / LDS_TC_TILE;
  const long tr = (long)blockIdx.x % tiles_r, tc = (long)blockIdx.x / tiles_r;
  const size_t src_pitch = (size_t)C * S.bits / 8, dst_pitch = (size_t)R * S.bits / 8;
  const unsigned char* tile = src + (size_t)tr * LDS_TC_TILE * src_pitch + (size_t)tc * T.row;

  if constexpr (FMT == ODH_TC_B6) {
    // thread: half a row, 48 packed bytes = four 12-byte pieces into four 16-byte slots
    const int r = tid >> 1, half = tid & 1;
    const uint4* s = reinterpret_cast<const uint4*>(tile + (size_t)r * src_pitch + 48 * half);
    const uint4 a = s[0], b = s[1], c = s[2];
    const uint32_t d[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
    uint32_t* slot = reinterpret_cast<uint32_t*>(lds_smem + r * P + 64 * half);
#pragma unroll
    for (int j = 0; j < 4; ++j) slot[4 * j] = d[3 * j], slot[4 * j + 1] = d[3 * j + 1], slot[4 * j + 2] = d[3 * j + 2];
  } else {
    constexpr int CH = T.row / 16;  // 16-byte chunks of a tile row
#pragma unroll
    for (int u = 0; u < LDS_TC_TILE * CH / 256; ++u) {
      const int k = tid + 256 * u, ch = k % CH;
      int r = k / CH;
      // 4 bit: 8 lanes are two rows; rows r and r + 4 keep their 64 B apart by 16 banks mod 32
      if constexpr (FMT == ODH_TC_B4) r = (r & ~7) | (r & 1) << 2 | (r >> 1 & 3);
      *reinterpret_cast<uint4*>(lds_smem + r * P + 16 * ch) =
          *reinterpret_cast<const uint4*>(tile + (size_t)r * src_pitch + 16 * ch);
    }
  }
  __syncthreads();

  // a step: every lane makes the 16-byte pieces (6 bit: three of them) of one destination row.  cb: the block
  // of 16 columns, first: the first of the lane's row blocks, and the order it reads its two in
  constexpr int BLOCKS = LDS_TC_TILE / S.rows;  // row blocks of the tile: 32, 16, 8, 8
  constexpr int STEPS = FMT == ODH_TC_B6 ? 1 : BLOCKS / 4;  // per wave
  const int h = g >> 1, sub = g & 1;
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    const int step = wave * STEPS + s;
    int cb, first;
    bool down = false;
    if constexpr (FMT == ODH_TC_B16 || FMT == ODH_TC_B8) {
      // the half's groups: row blocks 4 dp, 4 dp + 1 and 4 dp + 3, 4 dp + 2, in that order; the halves: two column blocks
      cb = 2 * (step & 3) + h, first = 4 * (step >> 2) + 2 * sub, down = sub;
    } else if constexpr (FMT == ODH_TC_B4) {
      // the half's groups: two column blocks; the halves: row blocks 4 mp, 4 mp + 1 and 4 mp + 2, 4 mp + 3
      cb = 2 * (step & 3) + sub, first = 4 * (step >> 2) + 2 * h;
    } else {
      // the groups that share sets of lanes: row blocks 0 … 3 and 4 … 7; the halves: two column blocks
      cb = 2 * step + h, first = 4 * sub;
    }
    const uint32_t col = FMT == ODH_TC_B6 ? 16u * cb : (uint32_t)cb * 2 * S.bits;  // bytes into an image row
    constexpr int NREAD = FMT == ODH_TC_B6 ? 4 : 2;
    LdsTrOut o[NREAD];
#pragma unroll
    for (int n = 0; n < NREAD; ++n) {
      const int rb = first + (down ? 1 - n : n);
      o[n] = lds_tr_read<T.check>((uint32_t)(rb * S.rows) * P + col + lds_tr_lane_offset(S, i, P));
    }
    unsigned char* out = dst + ((size_t)tc * LDS_TC_TILE + 16 * cb + i) * dst_pitch +
                         ((size_t)tr * LDS_TC_TILE + (size_t)first * S.rows) * S.bits / 8;
    if constexpr (FMT == ODH_TC_B6) {
      uint4* q = reinterpret_cast<uint4*>(out);
      q[0] = make_uint4(o[0].w[0], o[0].w[1], o[0].w[2], o[1].w[0]);
      q[1] = make_uint4(o[1].w[1], o[1].w[2], o[2].w[0], o[2].w[1]);
      q[2] = make_uint4(o[2].w[2], o[3].w[0], o[3].w[1], o[3].w[2]);
    } else {
      const LdsTrOut& lo = down ? o[1] : o[0];
      const LdsTrOut& hi = down ? o[0] : o[1];
      *reinterpret_cast<uint4*>(out) = make_uint4(lo.w[0], lo.w[1], hi.w[0], hi.w[1]);
    }
  }
}

template <typename... Args>
void lds_launch_transpose(int fmt, unsigned grid, hipStream_t stream, Args... args) {
  constexpr int L = LDS_TC_TILE;
  switch (fmt) {
    case ODH_TC_B16: transpose_codes_kernel<ODH_TC_B16><<<grid, 256, L * lds_tc_spec(ODH_TC_B16).pitch, stream>>>(args...); break;
    case ODH_TC_B8: transpose_codes_kernel<ODH_TC_B8><<<grid, 256, L * lds_tc_spec(ODH_TC_B8).pitch, stream>>>(args...); break;
    case ODH_TC_B4: transpose_codes_kernel<ODH_TC_B4><<<grid, 256, L * lds_tc_spec(ODH_TC_B4).pitch, stream>>>(args...); break;
    default: transpose_codes_kernel<ODH_TC_B6><<<grid, 256, L * lds_tc_spec(ODH_TC_B6).pitch, stream>>>(args...); break;
  }
}
