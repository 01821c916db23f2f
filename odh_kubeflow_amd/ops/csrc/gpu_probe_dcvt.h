// The start-up probe's decoding converters: the VALU instructions that turn low-precision codes BACK into
// f32, f16 or bf16, multiplied by the power of two in the exponent field of their f32 scale operand (an E8M0
// byte shifted left by 23).  gpu_probe_cvt.h makes such codes, the matrix-core steps decode them inside the
// MFMA; this is the third datapath, the one of every weight-only-quantised GEMM prologue and FP8 / FP4
// KV-cache read:
//   v_cvt_scalef32_pk_{f32,f16,bf16}_{fp8,bf8}   — the two bytes of the low or high half of the source
//                                                  register (word select) to two values;
//   v_cvt_scalef32_f32_{fp8,bf8}                 — one byte of the four (byte select) to one f32;
//   v_cvt_scalef32_pk_{f32,f16,bf16}_fp4         — the two nibbles of one byte of the four (byte select);
//   v_cvt_scalef32_pk32_{f32,f16,bf16}_{fp6,bf6} — 24 bytes to 32 values.
// What they exercise that nothing else here does: the source-select multiplexers, the 6-bit unpacker, the
// exponent adder and the three destination formats.
//
// Included by gpu_probe.hip inside its anonymous namespace, after gpu_probe_cvt.h: it uses CvtSpec, cvt_m,
// cvt_e, cvt_ilog2, cvt_scale_operand, xcc_id, slab_of and grid_for.
//
// The exact window.  For a source format and a destination, with e = scale byte - 127, the window is the
// range of e in which every finite code times 2^e is a normal finite number of the destination:
//   e >= emin_dst - (1 - bias - mbits)   and   v(cmax) · 2^e <= the destination's largest finite value
// (fp8 -> f32: bytes 10 … 246; fp8 -> f16: 122 … 134; bf16's windows are f32's; bf8 -> f16 has none: e5m2 has
// f16's own exponent range, so its smallest code is an f16 subnormal where its largest still fits).  The
// sources have at most 4 significant bits, so inside the window every product is exact in all three
// destinations and its bit pattern follows by integer construction (dcvt_expect): no decoder runs anywhere.
//
// The fused check (dcvt_probe_kernel) walks, per destination and per scale byte of its window, these items:
//   fp8, bf8   item i < 256: a source register whose byte j holds code (i + 85 j) & 255, so every code passes
//              through every byte and the four bytes always differ; both word selects of the packed form, both
//              results of each, and for f32 the four byte selects of the one-value form.  The NaN codes (fp8 0x7F /
//              0xFF, bf8 0x7D … 0x7F / 0xFD … 0xFF) are compared through "is a NaN", bf8's infinities through "is that
//              infinity" (dcvt_wrong), as the instructions were measured to deliver them
//   fp4        item i < 256: byte j holds (i + 85 j) & 255; the four byte selects, both nibbles
//   fp6, bf6   item r < 64: position k of the 32 holds code (r + k) & 63; all 32 results
// Scale bytes come from a table in memory (dcvt_fill_kernel: entry i = the first byte of the f32 window + i;
// the f16 window indexes into the same entries), staged in LDS.  A wrong table byte (other than 255)
// gives every finite non-zero code of its items another exponent: dcvt_fault_count mismatches.  What the
// instructions do at scales outside the window is in profiles/dcvt_probe/SUMMARY.txt.
//
// The public operation (dcvt_rows_kernel): codes in the layout odh_mx_gemm reads and E8M0 scales
// [rows][K/32] to [rows][K] f32 / f16 / bf16, the inverse of cvt_rows_kernel.  Contract, for every code and
// every scale byte: bytes 0 … 254 give value(code) · 2^(byte - 127) rounded to nearest even into the
// destination (exact wherever representable, subnormals kept, overflow to the infinity of that sign, -0 stays
// -0); fp8 and bf8 NaN codes give a NaN, bf8 infinities stay infinities; byte 255 makes the whole block NaN.
// It writes 4 to 8 times what it reads, so the work is laid out by the stores: every lane issues 16-byte
// non-temporal stores that the wave coalesces (a lane owns 4 elements to f32, 8 to f16 / bf16, so 8 or 4 lanes
// to a block of 32, whose scale byte the first of them loads and the others take by a lane exchange); the 2-
// to 8-byte loads behind them are coalesced too, four in flight per lane before the first conversion.  A lane
// of the 6-bit formats owns a whole block: three 8-byte loads, one instruction, one full 128-byte line (f32)
// or 64 bytes out.
// Every block takes the destination's own instruction, with no fallback: measured on an MI355X with dcvt_one_kernel
// (profiles/dcvt_probe/SUMMARY.txt), every code in every source position through every select at ALL 256 scale
// bytes, each of the fifteen instructions gives exactly what the contract asks: subnormal results kept, rounding to
// nearest even into f16 / bf16, overflow to infinity, NaN codes to NaN, bf8 infinities kept, byte 0 as 2^-127 and
// byte 255 as NaN; mantissa and sign of the scale operand are ignored.  The operation is a function of one code and
// one scale byte, so that measurement covers all of its inputs; tests/test_gpu_dcvt_edges.py repeats it with every
// suite: every code at every scale byte in every position of a lane's load, against the reference.

typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(32))) float f32x32;
typedef __attribute__((ext_vector_type(16))) unsigned u32x16;
typedef __attribute__((ext_vector_type(2))) unsigned dcvt_u2;

__host__ __device__ constexpr bool dcvt_fmt_ok(int fmt) { return cvt_scaled(fmt); }
__host__ __device__ constexpr bool dcvt_dst_ok(int dst) { return dst >= ODH_DCVT_F32 && dst <= ODH_DCVT_BF16; }

// a destination: exponent bias, mantissa bits, the smallest normal exponent
__host__ __device__ constexpr int dcvt_dbias(int dst) { return dst == ODH_DCVT_F16 ? 15 : 127; }
__host__ __device__ constexpr int dcvt_dmbits(int dst) { return dst == ODH_DCVT_F32 ? 23 : dst == ODH_DCVT_F16 ? 10 : 7; }
// the window's scale bytes [lo, hi]; empty when lo > hi
__host__ __device__ constexpr int dcvt_lo(CvtSpec s, int dst) { return 127 + (1 - dcvt_dbias(dst)) - (1 - s.bias - s.mbits); }
__host__ __device__ constexpr int dcvt_hi(CvtSpec s, int dst) {
  // v(cmax) = m · 2^k with p = floor(log2 m); every such m has at most 4 bits, fewer than any destination keeps,
  // so it is finite exactly when its exponent p + k + e is at most the bias (f16: 15, the others 127)
  return 127 + dcvt_dbias(dst) - (cvt_ilog2((unsigned)cvt_m(s, s.cmax)) + cvt_e(s, s.cmax));
}
__host__ __device__ constexpr int dcvt_nscale(CvtSpec s, int dst) {
  return dcvt_hi(s, dst) >= dcvt_lo(s, dst) ? dcvt_hi(s, dst) - dcvt_lo(s, dst) + 1 : 0;
}
static_assert(dcvt_lo(cvt_spec(ODH_CVT_FP8), ODH_DCVT_F32) == 10 && dcvt_hi(cvt_spec(ODH_CVT_FP8), ODH_DCVT_F32) == 246 &&
                  dcvt_lo(cvt_spec(ODH_CVT_FP8), ODH_DCVT_F16) == 122 && dcvt_hi(cvt_spec(ODH_CVT_FP8), ODH_DCVT_F16) == 134 &&
                  dcvt_nscale(cvt_spec(ODH_CVT_BF8), ODH_DCVT_F16) == 0,
              "the exact windows");

// items of one scale byte, values an item compares per destination (f32 of fp8 / bf8: the one-value form too)
__host__ __device__ constexpr int dcvt_nitems(int fmt) {
  return cvt_packed6(fmt) ? 64 : 256;
}
__host__ __device__ constexpr int dcvt_item_values(int fmt, int dst) {
  return cvt_packed6(fmt) ? 32 : fmt == ODH_CVT_FP4 ? 8 : dst == ODH_DCVT_F32 ? 8 : 4;
}
// of those, the ones a wrong scale changes, summed over the items of one scale byte: the codes that are neither a
// zero nor, in fp8 and bf8, a NaN or an infinity
__host__ __device__ constexpr int dcvt_scale_nonzero(int fmt, int dst) {
  // 6-bit: 32 consecutive codes mod 64 hold exactly one of 0 and 32; fp4: 32 of 256 bytes have a zero low nibble,
  // 32 a zero high one; fp8, bf8: every byte position sees the 2 cmax finite non-zero codes once
  return cvt_packed6(fmt)     ? 64 * 31
         : fmt == ODH_CVT_FP4 ? 4 * (2 * 256 - 64)
                              : 2 * cvt_spec(fmt).cmax * dcvt_item_values(fmt, dst);
}
// scale slots of the walk: f32's window, then f16's, then bf16's
__host__ __device__ constexpr int dcvt_slots(int fmt) {
  const CvtSpec s = cvt_spec(fmt);
  return dcvt_nscale(s, ODH_DCVT_F32) + dcvt_nscale(s, ODH_DCVT_F16) + dcvt_nscale(s, ODH_DCVT_BF16);
}
// values one wave compares
__host__ __device__ constexpr unsigned dcvt_family_size(int fmt) {
  const CvtSpec s = cvt_spec(fmt);
  unsigned n = 0;
  for (int dst = ODH_DCVT_F32; dst <= ODH_DCVT_BF16; ++dst)
    n += (unsigned)dcvt_nscale(s, dst) * dcvt_nitems(fmt) * dcvt_item_values(fmt, dst);
  return n;
}
// mismatches one wave counts when entry t of the table is wrong
__host__ __device__ constexpr unsigned dcvt_fault_values(int fmt, int t) {
  const CvtSpec s = cvt_spec(fmt);
  unsigned n = 0;
  for (int dst = ODH_DCVT_F32; dst <= ODH_DCVT_BF16; ++dst) {
    const int byte = dcvt_lo(s, ODH_DCVT_F32) + t;
    if (t >= 0 && byte >= dcvt_lo(s, dst) && byte <= dcvt_hi(s, dst)) n += dcvt_scale_nonzero(fmt, dst);
  }
  return n;
}

struct DcvtSlot {
  int dst, si;  // destination and index into the scale table
};
// scale slot q of the walk
__host__ __device__ constexpr DcvtSlot dcvt_slot(int fmt, int q) {
  const CvtSpec s = cvt_spec(fmt);
  const int n32 = dcvt_nscale(s, ODH_DCVT_F32), n16 = dcvt_nscale(s, ODH_DCVT_F16);
  if (q < n32) return {ODH_DCVT_F32, q};
  if (q < n32 + n16) return {ODH_DCVT_F16, q - n32 + dcvt_lo(s, ODH_DCVT_F16) - dcvt_lo(s, ODH_DCVT_F32)};
  return {ODH_DCVT_BF16, q - n32 - n16};  // bf16's window is f32's
}
// the code, sign included, at position pos of item i: byte pos of the source register (fp8, bf8: a code; fp4: a
// byte, two codes) or element pos of the 32 (fp6, bf6)
__host__ __device__ constexpr unsigned dcvt_code(int fmt, unsigned i, unsigned pos) {
  return cvt_packed6(fmt) ? (i + pos) & 63u : (i + 85u * pos) & 255u;
}
// what a code is: 0 a finite number, 1 a NaN (fp8 0x7F / 0xFF, bf8 0x7D … 0x7F / 0xFD … 0xFF), 2 an infinity (bf8
// 0x7C / 0xFC)
__host__ __device__ constexpr int dcvt_class(int fmt, unsigned code) {
  const unsigned mag = code & 0x7Fu;
  if (fmt == ODH_CVT_FP8) return mag == 0x7Fu ? 1 : 0;
  if (fmt == ODH_CVT_BF8) return mag > 0x7Cu ? 1 : mag == 0x7Cu ? 2 : 0;
  return 0;
}
// The expected value of a case, shared by host and device: the destination's bits of v(code) · 2^(byte - 127)
// for a finite code, sign included, and a scale byte of the window, by integer construction
__host__ __device__ constexpr uint32_t dcvt_expect(int fmt, int dst, unsigned code, int byte) {
  const CvtSpec s = cvt_spec(fmt);
  const unsigned sign = code >> (s.ebits + s.mbits) & 1u, mag = code & ((1u << (s.ebits + s.mbits)) - 1u);
  const unsigned m = (unsigned)cvt_m(s, (int)mag);
  const int mb = dcvt_dmbits(dst), sb = dst == ODH_DCVT_F32 ? 31 : 15;
  if (m == 0) return sign << sb;
  const int p = cvt_ilog2(m);
  return sign << sb | (uint32_t)(dcvt_dbias(dst) + p + cvt_e(s, (int)mag) + byte - 127) << mb |
         ((m << (mb - p)) & ((1u << mb) - 1u));
}
// whether the result `got` of a case is wrong: a finite code against dcvt_expect, a NaN code through "is a NaN",
// an infinity through "is that infinity"
__host__ __device__ constexpr bool dcvt_wrong(int fmt, int dst, uint32_t got, unsigned code, int byte) {
  const int mb = dcvt_dmbits(dst), sb = dst == ODH_DCVT_F32 ? 31 : 15;
  const uint32_t inf = ((1u << (sb - mb)) - 1u) << mb, cls = (uint32_t)dcvt_class(fmt, code);
  if (cls == 1) return (got & ((1u << sb) - 1u)) <= inf;
  if (cls == 2) return got != ((code >> 7) << sb | inf);
  return got != dcvt_expect(fmt, dst, code, byte);
}

// the table the probe kernel reads its scales from: the bytes of f32's window; ODH_CVT_TABLE bytes, the rest zero
__global__ void dcvt_fill_kernel(int fmt, uint8_t* __restrict__ table) {
  const int i = threadIdx.x;
  const CvtSpec s = cvt_spec(fmt);
  table[i] = (uint8_t)(i < dcvt_nscale(s, ODH_DCVT_F32) ? dcvt_lo(s, ODH_DCVT_F32) + i : 0);
}

// the packed instruction of (FMT, DST) on source dword v with select SEL (word select of fp8 / bf8, byte
// select of fp4): two values, as bits (f16 / bf16: the first in the low half of .x)
template <int FMT, int DST, int SEL>
__device__ __forceinline__ uint2 dcvt_pk(uint32_t v, float s) {
  static_assert(!cvt_packed6(FMT) && SEL >= 0 && SEL < (FMT == ODH_CVT_FP4 ? 4 : 2), "no such select");
  if constexpr (DST == ODH_DCVT_F32) {
    f32x2 r;
    if constexpr (FMT == ODH_CVT_FP8) r = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(v, s, SEL != 0);
    else if constexpr (FMT == ODH_CVT_BF8) r = __builtin_amdgcn_cvt_scalef32_pk_f32_bf8(v, s, SEL != 0);
    else r = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v, s, SEL);
    return make_uint2(__float_as_uint(r[0]), __float_as_uint(r[1]));
  } else if constexpr (DST == ODH_DCVT_F16) {
    f16x2 r;
    if constexpr (FMT == ODH_CVT_FP8) r = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(v, s, SEL != 0);
    else if constexpr (FMT == ODH_CVT_BF8) r = __builtin_amdgcn_cvt_scalef32_pk_f16_bf8(v, s, SEL != 0);
    else r = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(v, s, SEL);
    return make_uint2(__builtin_bit_cast(uint32_t, r), 0u);
  } else {
    bf16x2 r;
    if constexpr (FMT == ODH_CVT_FP8) r = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, s, SEL != 0);
    else if constexpr (FMT == ODH_CVT_BF8) r = __builtin_amdgcn_cvt_scalef32_pk_bf16_bf8(v, s, SEL != 0);
    else r = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, s, SEL);
    return make_uint2(__builtin_bit_cast(uint32_t, r), 0u);
  }
}
// the one-value form: byte SEL of v to one f32
template <int FMT, int SEL>
__device__ __forceinline__ uint32_t dcvt_single(uint32_t v, float s) {
  if constexpr (FMT == ODH_CVT_FP8) return __float_as_uint(__builtin_amdgcn_cvt_scalef32_f32_fp8((int)v, s, SEL));
  else return __float_as_uint(__builtin_amdgcn_cvt_scalef32_f32_bf8((int)v, s, SEL));
}
// 24 bytes to 32 f32
template <int FMT>
__device__ __forceinline__ f32x32 dcvt_pk32_f32(u32x6 v, float s) {
  if constexpr (FMT == ODH_CVT_FP6) return __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(v, s);
  else return __builtin_amdgcn_cvt_scalef32_pk32_f32_bf6(v, s);
}
// 24 bytes to 32 f16 or bf16, as 16 dwords: element 2w in the low half of dword w
template <int FMT, int DST>
__device__ __forceinline__ u32x16 dcvt_pk32_h(u32x6 v, float s) {
  if constexpr (DST == ODH_DCVT_F16) {
    if constexpr (FMT == ODH_CVT_FP6) return __builtin_bit_cast(u32x16, __builtin_amdgcn_cvt_scalef32_pk32_f16_fp6(v, s));
    else return __builtin_bit_cast(u32x16, __builtin_amdgcn_cvt_scalef32_pk32_f16_bf6(v, s));
  } else {
    if constexpr (FMT == ODH_CVT_FP6) return __builtin_bit_cast(u32x16, __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(v, s));
    else return __builtin_bit_cast(u32x16, __builtin_amdgcn_cvt_scalef32_pk32_bf16_bf6(v, s));
  }
}

// mismatches of item i of (FMT, DST): converted with the scale byte the table holds, compared with what the scale
// byte `byte` of the closed form gives
template <int FMT, int DST>
__device__ __forceinline__ unsigned dcvt_check_item(unsigned i, unsigned table_byte, int byte) {
  const float s = cvt_scale_operand(table_byte);
  unsigned bad = 0;
  if constexpr (cvt_packed6(FMT)) {
    u32x6 v = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      const unsigned c = dcvt_code(FMT, i, k);
      v[6 * k / 32] |= c << (6 * k % 32);
      if (6 * k % 32 > 26) v[6 * k / 32 + 1] |= c >> (32 - 6 * k % 32);
    }
    if constexpr (DST == ODH_DCVT_F32) {
      const f32x32 r = dcvt_pk32_f32<FMT>(v, s);
#pragma unroll
      for (int k = 0; k < 32; ++k) bad += dcvt_wrong(FMT, DST, __float_as_uint(r[k]), dcvt_code(FMT, i, k), byte);
    } else {
      const u32x16 r = dcvt_pk32_h<FMT, DST>(v, s);
#pragma unroll
      for (int k = 0; k < 32; ++k)
        bad += dcvt_wrong(FMT, DST, r[k / 2] >> (16 * (k & 1)) & 0xFFFFu, dcvt_code(FMT, i, k), byte);
    }
  } else {
    unsigned code[4];
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) code[j] = dcvt_code(FMT, i, j), v |= code[j] << (8 * j);
    // the values of byte j: fp4 its two nibbles, low first; fp8, bf8 the byte
    auto pair = [&](uint2 r, unsigned c0, unsigned c1) {
      if constexpr (DST == ODH_DCVT_F32)
        return (unsigned)dcvt_wrong(FMT, DST, r.x, c0, byte) + (unsigned)dcvt_wrong(FMT, DST, r.y, c1, byte);
      else
        return (unsigned)dcvt_wrong(FMT, DST, r.x & 0xFFFFu, c0, byte) + (unsigned)dcvt_wrong(FMT, DST, r.x >> 16, c1, byte);
    };
    if constexpr (FMT == ODH_CVT_FP4) {
      bad += pair(dcvt_pk<FMT, DST, 0>(v, s), code[0] & 15u, code[0] >> 4);
      bad += pair(dcvt_pk<FMT, DST, 1>(v, s), code[1] & 15u, code[1] >> 4);
      bad += pair(dcvt_pk<FMT, DST, 2>(v, s), code[2] & 15u, code[2] >> 4);
      bad += pair(dcvt_pk<FMT, DST, 3>(v, s), code[3] & 15u, code[3] >> 4);
    } else {
      bad += pair(dcvt_pk<FMT, DST, 0>(v, s), code[0], code[1]);
      bad += pair(dcvt_pk<FMT, DST, 1>(v, s), code[2], code[3]);
      if constexpr (DST == ODH_DCVT_F32) {
        bad += dcvt_wrong(FMT, DST, dcvt_single<FMT, 0>(v, s), code[0], byte);
        bad += dcvt_wrong(FMT, DST, dcvt_single<FMT, 1>(v, s), code[1], byte);
        bad += dcvt_wrong(FMT, DST, dcvt_single<FMT, 2>(v, s), code[2], byte);
        bad += dcvt_wrong(FMT, DST, dcvt_single<FMT, 3>(v, s), code[3], byte);
      }
    }
  }
  return bad;
}

// The fused check: 256 workgroups of 256 threads, one per CU, a wave per SIMD, and every wave walks the whole
// family: a lane takes item after item of a scale slot, its scale byte from the table in LDS, and compares
// in registers
template <int FMT>
__global__ __launch_bounds__(256, 1) void dcvt_probe_kernel(const uint8_t* __restrict__ table,
                                                            int* __restrict__ xcd_blocks,
                                                            unsigned* __restrict__ err_total,
                                                            unsigned* __restrict__ err_xcd) {
  __shared__ uint4 lds[CVT_LDS_U4];
  uint8_t* scales = reinterpret_cast<uint8_t*>(lds);
  const int tid = threadIdx.x, lane = tid & 63;
  const unsigned xcc = xcc_id();
  if (tid == 0) atomicAdd(&xcd_blocks[xcc], 1);
  scales[tid] = table[tid];  // ODH_CVT_TABLE = 256 bytes
  __syncthreads();

  constexpr unsigned NI = dcvt_nitems(FMT), ITEMS = (unsigned)dcvt_slots(FMT) * NI;
  unsigned bad = 0;
  for (unsigned idx = lane; idx < ITEMS; idx += 64) {
    const DcvtSlot q = dcvt_slot(FMT, (int)(idx / NI));
    const unsigned i = idx % NI, table_byte = scales[q.si];
    const int byte = dcvt_lo(cvt_spec(FMT), ODH_DCVT_F32) + q.si;  // what the fill put there
    if (q.dst == ODH_DCVT_F32) bad += dcvt_check_item<FMT, ODH_DCVT_F32>(i, table_byte, byte);
    else if (q.dst == ODH_DCVT_F16) bad += dcvt_check_item<FMT, ODH_DCVT_F16>(i, table_byte, byte);
    else bad += dcvt_check_item<FMT, ODH_DCVT_BF16>(i, table_byte, byte);
  }
  for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
  if (lane == 0 && bad) {
    atomicAdd(err_total, bad);
    atomicAdd(&err_xcd[xcc], bad);
  }
}

// words a lane of dcvt_one_kernel writes: the raw result registers of one instruction
__host__ __device__ constexpr int dcvt_one_words(int fmt, int dst, int form) {
  return cvt_packed6(fmt) ? (dst == ODH_DCVT_F32 ? 32 : 16) : form == 1 ? 1 : dst == ODH_DCVT_F32 ? 2 : 1;
}
// form 0: the packed instruction; form 1: the one-value form, fp8 / bf8 to f32 only.  sel: the word select
// (0 … 1) of packed fp8 / bf8, the byte select (0 … 3) of fp4 and of the one-value form, 0 for the 6-bit formats
__host__ __device__ constexpr bool dcvt_one_ok(int fmt, int dst, int form, int sel) {
  if (!dcvt_fmt_ok(fmt) || !dcvt_dst_ok(dst) || form < 0 || form > 1 || sel < 0) return false;
  if (form == 1) return (fmt == ODH_CVT_FP8 || fmt == ODH_CVT_BF8) && dst == ODH_DCVT_F32 && sel < 4;
  return sel < (cvt_packed6(fmt) ? 1 : fmt == ODH_CVT_FP4 ? 4 : 2);
}

template <int FMT, int DST>
__device__ __forceinline__ void dcvt_one_lane(int form, int sel, const uint32_t* __restrict__ src, float s,
                                              uint32_t* __restrict__ out) {
  if constexpr (cvt_packed6(FMT)) {
    u32x6 v;
#pragma unroll
    for (int w = 0; w < 6; ++w) v[w] = src[w];
    if constexpr (DST == ODH_DCVT_F32) {
      const f32x32 r = dcvt_pk32_f32<FMT>(v, s);
#pragma unroll
      for (int k = 0; k < 32; ++k) out[k] = __float_as_uint(r[k]);
    } else {
      const u32x16 r = dcvt_pk32_h<FMT, DST>(v, s);
#pragma unroll
      for (int k = 0; k < 16; ++k) out[k] = r[k];
    }
  } else {
    const uint32_t v = src[0];
    if constexpr (FMT != ODH_CVT_FP4 && DST == ODH_DCVT_F32) {
      if (form == 1) {
        out[0] = sel == 0 ? dcvt_single<FMT, 0>(v, s) : sel == 1 ? dcvt_single<FMT, 1>(v, s)
                 : sel == 2 ? dcvt_single<FMT, 2>(v, s) : dcvt_single<FMT, 3>(v, s);
        return;
      }
    }
    uint2 r;
    if constexpr (FMT == ODH_CVT_FP4)
      r = sel == 0 ? dcvt_pk<FMT, DST, 0>(v, s) : sel == 1 ? dcvt_pk<FMT, DST, 1>(v, s)
          : sel == 2 ? dcvt_pk<FMT, DST, 2>(v, s) : dcvt_pk<FMT, DST, 3>(v, s);
    else
      r = sel == 0 ? dcvt_pk<FMT, DST, 0>(v, s) : dcvt_pk<FMT, DST, 1>(v, s);
    out[0] = r.x;
    if constexpr (DST == ODH_DCVT_F32) out[1] = r.y;
  }
}

// One instruction, one wave: lane l converts its source register src[l] (6-bit formats: src[6 l … 6 l + 5])
// with the raw scale operand scale[l] and writes its dcvt_one_words result dwords
template <int FMT>
__global__ __launch_bounds__(64) void dcvt_one_kernel(int dst, int form, int sel, const uint32_t* __restrict__ src,
                                                      const uint32_t* __restrict__ scale, uint32_t* __restrict__ out) {
  const int l = threadIdx.x;
  const float s = __uint_as_float(scale[l]);
  const uint32_t* in = src + l * (cvt_packed6(FMT) ? 6 : 1);
  uint32_t* o = out + l * dcvt_one_words(FMT, dst, form);
  if (dst == ODH_DCVT_F32) dcvt_one_lane<FMT, ODH_DCVT_F32>(form, sel, in, s, o);
  else if (dst == ODH_DCVT_F16) dcvt_one_lane<FMT, ODH_DCVT_F16>(form, sel, in, s, o);
  else dcvt_one_lane<FMT, ODH_DCVT_BF16>(form, sel, in, s, o);
}

// codes and scales to out; n counts 16-byte pieces of out (6-bit formats: blocks).  Every block goes through the
// destination's own instruction, whatever its scale byte and codes: see the measurement in the header comment
template <int FMT, int DST>
__global__ __launch_bounds__(256) void dcvt_rows_kernel(const void* __restrict__ codes, size_t n,
                                                        const uint8_t* __restrict__ scales, u32x4* __restrict__ out) {
  const auto [lo, hi] = slab_of(n);
  if constexpr (cvt_packed6(FMT)) {
    const dcvt_u2* in = static_cast<const dcvt_u2*>(codes);
    constexpr int PIECES = DST == ODH_DCVT_F32 ? 8 : 4;  // 16-byte stores of a block
    for (size_t blk = lo + threadIdx.x; blk < hi; blk += 256) {
      const dcvt_u2 a = __builtin_nontemporal_load(&in[blk * 3]), b = __builtin_nontemporal_load(&in[blk * 3 + 1]),
                    c = __builtin_nontemporal_load(&in[blk * 3 + 2]);
      const float s = cvt_scale_operand(scales[blk]);
      const u32x6 v = {a.x, a.y, b.x, b.y, c.x, c.y};
      uint32_t r[4 * PIECES];
      if constexpr (DST == ODH_DCVT_F32) {
        const f32x32 t = dcvt_pk32_f32<FMT>(v, s);
#pragma unroll
        for (int k = 0; k < 32; ++k) r[k] = __float_as_uint(t[k]);
      } else {
        const u32x16 h = dcvt_pk32_h<FMT, DST>(v, s);
#pragma unroll
        for (int k = 0; k < 16; ++k) r[k] = h[k];
      }
#pragma unroll
      for (int u = 0; u < PIECES; ++u) {
        u32x4 q;
        q.x = r[4 * u], q.y = r[4 * u + 1], q.z = r[4 * u + 2], q.w = r[4 * u + 3];
        __builtin_nontemporal_store(q, &out[blk * PIECES + u]);
      }
    }
  } else {
    constexpr bool WIDE = DST == ODH_DCVT_F32;  // 4 elements to a piece, else 8
    constexpr int LPB = WIDE ? 8 : 4;           // lanes to a block of 32
    // a piece's codes: 2 bytes (fp4 -> f32), 4 (fp4 -> 16 bits, 8 bits -> f32) or 8 (8 bits -> 16 bits)
    using Load = std::conditional_t<FMT == ODH_CVT_FP4, std::conditional_t<WIDE, uint16_t, uint32_t>,
                                    std::conditional_t<WIDE, uint32_t, dcvt_u2>>;
    const Load* in = static_cast<const Load*>(codes);
    const int lane = threadIdx.x & 63;
    for (size_t base = lo + threadIdx.x; base < hi; base += 4 * 256) {
      Load v[4];
      unsigned sc[4] = {0, 0, 0, 0};
#pragma unroll
      for (int u = 0; u < 4; ++u) {  // all four loads, and the scale bytes of the lanes that lead a block, in flight
        const size_t i = base + u * 256;
        if (i < hi) {
          v[u] = __builtin_nontemporal_load(&in[i]);
          if ((i & (LPB - 1)) == 0) sc[u] = scales[i / LPB];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const size_t i = base + u * 256;
        if (i >= hi) continue;  // uniform over the lanes of a block: slabs and n are multiples of LPB
        // pieces of a block are consecutive lanes from a multiple of LPB on: slabs start at multiples of 1024
        const float s = cvt_scale_operand(__shfl(sc[u], lane & ~(LPB - 1), 64));
        u32x4 q;
        if constexpr (WIDE) {  // two bytes, or two nibble pairs, per instruction
          const uint2 a = dcvt_pk<FMT, DST, 0>(v[u], s), b = dcvt_pk<FMT, DST, 1>(v[u], s);
          q.x = a.x, q.y = a.y, q.z = b.x, q.w = b.y;
        } else if constexpr (FMT == ODH_CVT_FP4) {
          q.x = dcvt_pk<FMT, DST, 0>(v[u], s).x, q.y = dcvt_pk<FMT, DST, 1>(v[u], s).x;
          q.z = dcvt_pk<FMT, DST, 2>(v[u], s).x, q.w = dcvt_pk<FMT, DST, 3>(v[u], s).x;
        } else {
          q.x = dcvt_pk<FMT, DST, 0>(v[u].x, s).x, q.y = dcvt_pk<FMT, DST, 1>(v[u].x, s).x;
          q.z = dcvt_pk<FMT, DST, 0>(v[u].y, s).x, q.w = dcvt_pk<FMT, DST, 1>(v[u].y, s).x;
        }
        __builtin_nontemporal_store(q, &out[i]);
      }
    }
  }
}

// every format's kernels on one argument list
template <typename... Args>
void dcvt_launch_probe(int fmt, hipStream_t stream, Args... args) {
  switch (fmt) {
    case ODH_CVT_FP8: dcvt_probe_kernel<ODH_CVT_FP8><<<ODH_CVT_BLOCKS, 256, 0, stream>>>(args...); break;
    case ODH_CVT_BF8: dcvt_probe_kernel<ODH_CVT_BF8><<<ODH_CVT_BLOCKS, 256, 0, stream>>>(args...); break;
    case ODH_CVT_FP6: dcvt_probe_kernel<ODH_CVT_FP6><<<ODH_CVT_BLOCKS, 256, 0, stream>>>(args...); break;
    case ODH_CVT_BF6: dcvt_probe_kernel<ODH_CVT_BF6><<<ODH_CVT_BLOCKS, 256, 0, stream>>>(args...); break;
    default: dcvt_probe_kernel<ODH_CVT_FP4><<<ODH_CVT_BLOCKS, 256, 0, stream>>>(args...); break;
  }
}
template <typename... Args>
void dcvt_launch_one(int fmt, hipStream_t stream, Args... args) {
  switch (fmt) {
    case ODH_CVT_FP8: dcvt_one_kernel<ODH_CVT_FP8><<<1, 64, 0, stream>>>(args...); break;
    case ODH_CVT_BF8: dcvt_one_kernel<ODH_CVT_BF8><<<1, 64, 0, stream>>>(args...); break;
    case ODH_CVT_FP6: dcvt_one_kernel<ODH_CVT_FP6><<<1, 64, 0, stream>>>(args...); break;
    case ODH_CVT_BF6: dcvt_one_kernel<ODH_CVT_BF6><<<1, 64, 0, stream>>>(args...); break;
    default: dcvt_one_kernel<ODH_CVT_FP4><<<1, 64, 0, stream>>>(args...); break;
  }
}
template <int DST, typename... Args>
void dcvt_launch_rows_to(int fmt, int grid, hipStream_t stream, Args... args) {
  switch (fmt) {
    case ODH_CVT_FP8: dcvt_rows_kernel<ODH_CVT_FP8, DST><<<grid, 256, 0, stream>>>(args...); break;
    case ODH_CVT_BF8: dcvt_rows_kernel<ODH_CVT_BF8, DST><<<grid, 256, 0, stream>>>(args...); break;
    case ODH_CVT_FP6: dcvt_rows_kernel<ODH_CVT_FP6, DST><<<grid, 256, 0, stream>>>(args...); break;
    case ODH_CVT_BF6: dcvt_rows_kernel<ODH_CVT_BF6, DST><<<grid, 256, 0, stream>>>(args...); break;
    default: dcvt_rows_kernel<ODH_CVT_FP4, DST><<<grid, 256, 0, stream>>>(args...); break;
  }
}
template <typename... Args>
void dcvt_launch_rows(int fmt, int dst, int grid, hipStream_t stream, Args... args) {
  if (dst == ODH_DCVT_F32) dcvt_launch_rows_to<ODH_DCVT_F32>(fmt, grid, stream, args...);
  else if (dst == ODH_DCVT_F16) dcvt_launch_rows_to<ODH_DCVT_F16>(fmt, grid, stream, args...);
  else dcvt_launch_rows_to<ODH_DCVT_BF16>(fmt, grid, stream, args...);
}

// host side: what odh_mx_dequantize takes.  codes 8-byte aligned, out 16-byte aligned; rows · K below 2^40
bool dcvt_rows_ok(int fmt, int dst, const void* codes, const void* scales, const void* out, long rows, long K) {
  return dcvt_fmt_ok(fmt) && dcvt_dst_ok(dst) && rows > 0 && K > 0 && K % 32 == 0 && rows <= ((1L << 40) - 1) / K && codes &&
         scales && out && ((uintptr_t)codes & 7) == 0 && ((uintptr_t)out & 15) == 0;
}
// pieces the row kernel strides over: blocks for the 6-bit formats, 16 bytes of out otherwise
size_t dcvt_pieces(int fmt, int dst, long rows, long K) {
  return (size_t)rows * (size_t)K / (cvt_packed6(fmt) ? 32 : dst == ODH_DCVT_F32 ? 4 : 8);
}
