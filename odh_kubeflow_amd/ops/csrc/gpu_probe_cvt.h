// The start-up probe's converter kernels: the VALU instructions that PRODUCE low-precision codes at run
// time, which the matrix-core steps (gpu_probe_mx.h and the others) only ever decode:
//   v_cvt_scalef32_pk_fp8_f32 / _pk_bf8_f32    — two f32 to two OCP e4m3fn / e5m2 bytes, into the low or the
//                                                high half of the destination (word select);
//   v_cvt_scalef32_pk_fp4_f32                  — two f32 to two e2m1 nibbles, into one of the four bytes of the
//                                                destination (byte select);
//   v_cvt_scalef32_2xpk16_fp6_f32 / _bf6_f32   — two registers of 16 f32 to 32 packed e2m3 / e3m2 codes (24 bytes);
//   v_cvt_pk_bf16_f32                          — two f32 to two bfloat16 (a plain cast; there is no builtin).
// The scaled ones divide by the power of two in the exponent field of their f32 scale operand (an E8M0 byte
// shifted left by 23) and round to nearest even.  What they exercise that nothing else here does: the
// rounding increment, the sticky-bit collection over the 20-odd discarded mantissa bits, the subnormal
// shifter, the E8M0 exponent subtractor and the destination selects, one datapath per SIMD.
//
// Included by gpu_probe.hip inside its anonymous namespace, after the HBM sweep kernels: it uses xcc_id,
// slab_of and grid_for.
//
// The probe's input family (cvt_case) has its expected codes by construction; no encoder runs anywhere.
// For a format with finite magnitude codes 0 … cmax, value v(c):
//   exact   v(c)                                             -> c
//   tie     the midpoint of v(c) and v(c + 1), c < cmax      -> whichever of c, c + 1 is even
//   below   the f32 just below that midpoint                 -> c
//   above   the f32 just above it                            -> c + 1
// and the overflow class at c = cmax, whose midpoint is half a step above the largest finite value:
//   just below it -> cmax; at it -> CvtSpec::ovf_tie; just above it, and four times it -> CvtSpec::ovf.
// v(c) is M · 2^E with M < 2^(mbits + 1), so a midpoint is (2M + 1) · 2^(E - 1): an f32 with at most five
// mantissa bits set, and its two neighbours differ from it in bit 0 of the mantissa (a converter that loses
// low sticky bits turns them into ties).  Each case is multiplied by 2^e (added to the exponent field, so
// exactly) and converted with the scale 2^e, for every e at which all cases of the format are normal finite
// f32 (cvt_emin … cvt_emax; e4m3fn: -115 … 117), in both signs and through every destination select.  No
// case is NaN, infinite or f32-subnormal.  A scale's block of cases is padded with exact cases to a multiple
// of 32, so that 32 consecutive cases (one 6-bit instruction) and two (one packed one) share their scale.
//   index = ((scale index · selects + select) · 2 + sign) · NVP + variant index
// bf16 has no scale: every exponent field 1 … 254 × 128 mantissas × the four variants × both signs; the last
// one rounds the largest finite bf16 up to infinity.
//
// What the hardware answers beyond the largest finite value (CvtSpec::ovf_tie and ::ovf) is in cvt_spec
// below, per format, as measured on an MI355X; profiles/cvt_probe/SUMMARY.txt has the run.
//
// The public operation (cvt_rows_kernel): x [rows][K] f32, K a multiple of 32, to codes in the layout
// odh_mx_gemm reads (mx_row_bytes) and E8M0 scales [rows][K/32].  QUANT: the OCP MX rule, the block's
// shared exponent floor(log2(amax)) - emax of the element format clamped to the E8M0 range, 2^0 for an
// all-zero block, and OCP saturation (clamped in f32 before the conversion, so the contract does not
// depend on what the instruction does beyond the largest finite value).  Not QUANT: the caller's scales
// and the bare instruction.  QUANT's contract for every f32, per block of 32 (tests/cvt_reference.py is its
// model, tests/test_gpu_cvt_edges.py holds the kernel to it):
//   - amax is the largest |x| over the elements that are not NaN; +-Inf counts as FLT_MAX;
//   - if no such element exists, or all are zero, the byte is 127;
//   - otherwise byte = clamp(floor(log2 amax) - emax + 127, 0, 254); with an Inf in the block that is
//     254 - emax.  Byte 255 (the E8M0 NaN) is never emitted;
//   - finite elements are clamped in f32 to +-(largest finite value · scale) and then converted;
//   - +-Inf becomes the largest finite code with its sign, in every format: the saturation of finite overflow;
//   - NaN goes to the instruction unclamped: fp8 0xFF and bf8 0xFE whatever the sign; fp4, fp6 and bf6 have no
//     NaN and give their largest code with the input's sign, so these three formats cannot carry a NaN.
// bf16 is the plain conversion: Inf stays Inf, NaN stays NaN, quieted.
// A streaming kernel on the slabs of the HBM sweep: 16-byte loads, four in flight per lane, eight lanes to
// a block of 32 with amax by three cross-lane steps; the 6-bit formats take a block per lane, because
// their one instruction wants all 32 values in one lane.

typedef __attribute__((ext_vector_type(2))) short i16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) float cvt_f4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(6))) unsigned u32x6;

struct CvtSpec {
  int ebits, mbits, bias;
  int cmax;     // the largest finite magnitude code
  int nsel;     // destination selects of the instruction
  int emax;     // exponent of the largest finite value: floor(log2(v(cmax)))
  int ovf_tie;  // magnitude code of an input exactly half a step above v(cmax)
  int ovf;      // magnitude code of an input beyond that
};

// Overflow, as measured (the sign is kept in every case):
//   e4m3fn: half a step above 448 (464) is a tie and rounds to the even code, 0x7E = 448 itself; everything
//           beyond it -> 0x7F, NaN: the format has no infinity
//   e5m2:   half a step above 57344 (61440) is a tie too and rounds to the even code, 0x7C, infinity, as does
//           everything beyond it
//   e2m1, e2m3, e3m2: no NaN and no infinity to give: everything beyond the largest value saturates to it
__host__ __device__ constexpr CvtSpec cvt_spec(int fmt) {
  switch (fmt) {
    case ODH_CVT_FP8: return {4, 3, 7, 126, 2, 8, 126, 0x7F};
    case ODH_CVT_BF8: return {5, 2, 15, 123, 2, 15, 0x7C, 0x7C};
    case ODH_CVT_FP6: return {2, 3, 1, 31, 1, 2, 31, 31};
    case ODH_CVT_BF6: return {3, 2, 3, 31, 1, 4, 31, 31};
    default: return {2, 1, 1, 7, 4, 2, 7, 7};  // ODH_CVT_FP4
  }
}
__host__ __device__ constexpr bool cvt_scaled(int fmt) { return fmt >= ODH_CVT_FP8 && fmt <= ODH_CVT_FP4; }
__host__ __device__ constexpr bool cvt_fmt_ok(int fmt) { return cvt_scaled(fmt) || fmt == ODH_CVT_BF16; }
__host__ __device__ constexpr bool cvt_packed6(int fmt) { return fmt == ODH_CVT_FP6 || fmt == ODH_CVT_BF6; }

// v(c) = cvt_m(c) · 2^cvt_e(c)
__host__ __device__ constexpr int cvt_m(CvtSpec s, int c) {
  return (c >> s.mbits) ? (1 << s.mbits) | (c & ((1 << s.mbits) - 1)) : c;
}
__host__ __device__ constexpr int cvt_e(CvtSpec s, int c) {
  return ((c >> s.mbits) ? (c >> s.mbits) : 1) - s.bias - s.mbits;
}
__host__ __device__ constexpr int cvt_ilog2(unsigned n) { return 31 - __builtin_clz(n); }
// variants of one sign and scale, and that padded to a multiple of 16
__host__ __device__ constexpr int cvt_nv(CvtSpec s) { return (s.cmax + 1) + 3 * s.cmax + 4; }
__host__ __device__ constexpr int cvt_nvp(CvtSpec s) { return (cvt_nv(s) + 15) & ~15; }
// the scale exponents: the smallest input, just below the midpoint 2^(-bias - mbits) of 0 and v(1), stays
// normal; the largest, four times the overflow midpoint, finite
__host__ __device__ constexpr int cvt_emin(CvtSpec s) { return -126 + s.bias + s.mbits + 1; }
__host__ __device__ constexpr int cvt_emax(CvtSpec s) {
  return 127 - (cvt_ilog2(2 * cvt_m(s, s.cmax) + 1) + cvt_e(s, s.cmax) + 1);
}
__host__ __device__ constexpr int cvt_nscale(CvtSpec s) { return cvt_emax(s) - cvt_emin(s) + 1; }

constexpr int CVT_BF16_EXPS = 254;  // exponent fields 1 … 254
__host__ __device__ constexpr unsigned cvt_family_size(int fmt) {
  return cvt_scaled(fmt) ? (unsigned)cvt_nscale(cvt_spec(fmt)) * cvt_spec(fmt).nsel * 2u * cvt_nvp(cvt_spec(fmt))
                         : 2u * CVT_BF16_EXPS * 128u * 4u;
}

// the f32 bits of the integer n >= 1 times 2^sh, by construction (n < 2^24)
__host__ __device__ constexpr uint32_t cvt_fbits(unsigned n, int sh) {
  const int p = cvt_ilog2(n);
  return (uint32_t)(((127 + p + sh) << 23) | (int)((n << (23 - p)) & 0x7FFFFFu));
}

struct CvtCase {
  uint32_t x;       // the f32 input, as bits
  uint32_t si;      // index into the scale table (bf16: into the table of exponent fields)
  uint32_t scale;   // E8M0 byte of the scale operand (bf16: 127)
  uint32_t sel;     // destination select
  uint32_t expect;  // the code, sign included (bf16: 16 bits)
};

// Case idx of the family of fmt.  One function for the host (odh_cvt_family) and the kernels.
__host__ __device__ constexpr CvtCase cvt_case(int fmt, uint32_t idx) {
  if (!cvt_scaled(fmt)) {
    // idx = ((sign · 254 + exponent index) · 128 + mantissa) · 4 + variant
    const uint32_t var = idx & 3, m = (idx >> 2) & 127, ei = (idx >> 9) % CVT_BF16_EXPS, sign = (idx >> 9) / CVT_BF16_EXPS;
    const uint32_t c = ((ei + 1) << 7) | m;
    const uint32_t low = var == 0 ? 0u : var == 1 ? 0x8000u : var == 2 ? 0x7FFFu : 0x8001u;
    const uint32_t e = var == 0 ? c : var == 1 ? c + (c & 1) : var == 2 ? c : c + 1;
    return {sign << 31 | c << 16 | low, ei, 127, 0, sign << 15 | e};
  }
  const CvtSpec s = cvt_spec(fmt);
  const int nv = cvt_nv(s), nvp = cvt_nvp(s);
  const uint32_t b = idx / (2u * nvp), r = idx % (2u * nvp);
  const uint32_t si = b / s.nsel, sel = b % s.nsel, sign = r / nvp;
  const int v = (int)(r % nvp), e = cvt_emin(s) + (int)si;
  int c = 0, n = 0, sh = 0, delta = 0, expect = 0;
  if (v <= s.cmax || v >= nv) {  // exact, the padding included
    c = v <= s.cmax ? v : (v - nv) % (s.cmax + 1);
    n = cvt_m(s, c), sh = cvt_e(s, c), expect = c;
  } else if (v - (s.cmax + 1) < 3 * s.cmax) {  // the midpoint of c and c + 1 and its neighbours
    const int t = v - (s.cmax + 1), var = t % 3;
    c = t / 3;
    n = 2 * cvt_m(s, c) + 1, sh = cvt_e(s, c) - 1;
    delta = var == 0 ? 0 : var == 1 ? -1 : 1;
    expect = var == 0 ? c + (c & 1) : var == 1 ? c : c + 1;
  } else {  // the overflow class
    const int o = v - (s.cmax + 1) - 3 * s.cmax;
    c = s.cmax;
    n = 2 * cvt_m(s, c) + 1, sh = cvt_e(s, c) + (o == 3 ? 1 : -1);
    delta = o == 0 ? -1 : o == 2 ? 1 : 0;
    expect = o == 0 ? c : o == 1 ? s.ovf_tie : s.ovf;
  }
  const uint32_t x = n ? (uint32_t)((int)cvt_fbits((unsigned)n, sh + e) + delta) : 0u;
  return {sign << 31 | x, si, (uint32_t)(e + 127), sel, sign << (s.ebits + s.mbits) | (uint32_t)expect};
}

// the table the probe kernel reads its scales from: the E8M0 byte of every scale index (bf16: the exponent
// field of every exponent index); ODH_CVT_TABLE bytes, the rest zero
__global__ void cvt_fill_kernel(int fmt, uint8_t* __restrict__ table) {
  const int i = threadIdx.x;
  const int n = cvt_scaled(fmt) ? cvt_nscale(cvt_spec(fmt)) : CVT_BF16_EXPS;
  const int first = cvt_scaled(fmt) ? cvt_emin(cvt_spec(fmt)) + 127 : 1;
  table[i] = (uint8_t)(i < n ? first + i : 0);
}

__device__ __forceinline__ float cvt_scale_operand(unsigned byte) { return __uint_as_float(byte << 23); }

// Element k of the 32 that one 6-bit instruction packs comes from operand k & 1, element k >> 1: the two
// 16-float operands interleave (measured: x[k] = v(k) gives the codes 0 … 31 in order).
template <int FMT>
__device__ __forceinline__ u32x6 cvt_pk32(const float (&x)[32], float scale) {
  f32x16 a, b;
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = x[2 * i], b[i] = x[2 * i + 1];
  if constexpr (FMT == ODH_CVT_FP6)
    return __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(a, b, scale);
  else
    return __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(a, b, scale);
}

// two f32 to two bytes in the low (SEL = 0) or high half of old
template <int FMT, bool SEL>
__device__ __forceinline__ uint32_t cvt_pk8(uint32_t old, float a, float b, float scale) {
  const i16x2 o = __builtin_bit_cast(i16x2, old);
  if constexpr (FMT == ODH_CVT_FP8)
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(o, a, b, scale, SEL));
  else
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf8_f32(o, a, b, scale, SEL));
}

__device__ __forceinline__ uint32_t cvt_pk_bf16(float a, float b) {
  f32x2 v;
  v[0] = a, v[1] = b;
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

constexpr int CVT_LDS_U4 = 96 * 1024 / 16;  // 96 of the CU's 160 KiB: two workgroups cannot share a CU

// The fused check: 256 workgroups of 256 threads, one per CU, a wave per SIMD, and every wave walks the
// whole family.  Inputs from cvt_case and the scale table, results compared in registers.  A packed
// instruction converts a lane's own case in its first operand and its neighbour's (lane ^ 1: the same scale
// and select) in the second, so every case passes through both; every select of the destination is
// issued, the case's own one checked against the codes and the rest of the register against what was there.
template <int FMT>
__global__ __launch_bounds__(256, 1) void cvt_probe_kernel(const uint8_t* __restrict__ table,
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

  constexpr unsigned SIZE = cvt_family_size(FMT);
  constexpr uint32_t OLD = 0xA5C35A3Cu;
  unsigned bad = 0;
  if constexpr (FMT == ODH_CVT_BF16) {
    for (unsigned idx = lane; idx < SIZE; idx += 64) {
      const CvtCase c = cvt_case(FMT, idx);
      // the exponent field from the table, the rest from the closed form
      const uint32_t xb = (c.x & 0x807FFFFFu) | (uint32_t)scales[c.si] << 23;
      const uint32_t yb = __shfl_xor(xb, 1, 64), ye = __shfl_xor(c.expect, 1, 64);
      bad += cvt_pk_bf16(__uint_as_float(xb), __uint_as_float(yb)) != (c.expect | ye << 16);
    }
  } else if constexpr (cvt_packed6(FMT)) {
    for (unsigned t = lane; t < SIZE / 32; t += 64) {
      float x[32];
      u32x6 want = {0, 0, 0, 0, 0, 0};
      unsigned si = 0;
#pragma unroll
      for (int k = 0; k < 32; ++k) {
        const CvtCase c = cvt_case(FMT, t * 32 + k);
        x[k] = __uint_as_float(c.x);
        si = c.si;
        // element k in bits [6k, 6k + 6) of the 24 bytes
        want[6 * k / 32] |= c.expect << (6 * k % 32);
        if (6 * k % 32 > 26) want[6 * k / 32 + 1] |= c.expect >> (32 - 6 * k % 32);
      }
      const u32x6 got = cvt_pk32<FMT>(x, cvt_scale_operand(scales[si]));
#pragma unroll
      for (int w = 0; w < 6; ++w) bad += got[w] != want[w];
    }
  } else {
    for (unsigned idx = lane; idx < SIZE; idx += 64) {
      const CvtCase c = cvt_case(FMT, idx);
      const float s = cvt_scale_operand(scales[c.si]);
      const float x = __uint_as_float(c.x), y = __uint_as_float(__shfl_xor(c.x, 1, 64));
      const uint32_t ye = __shfl_xor(c.expect, 1, 64);
      if constexpr (FMT == ODH_CVT_FP4) {
        const uint32_t r[4] = {__builtin_amdgcn_cvt_scalef32_pk_fp4_f32(OLD, x, y, s, 0),
                               __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(OLD, x, y, s, 1),
                               __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(OLD, x, y, s, 2),
                               __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(OLD, x, y, s, 3)};
        const uint32_t got = c.sel == 0 ? r[0] : c.sel == 1 ? r[1] : c.sel == 2 ? r[2] : r[3];
        const uint32_t mask = 0xFFu << (8 * c.sel);
        bad += got != ((OLD & ~mask) | (c.expect | ye << 4) << (8 * c.sel));
      } else {
        const uint32_t lo = cvt_pk8<FMT, false>(OLD, x, y, s), hi = cvt_pk8<FMT, true>(OLD, x, y, s);
        const uint32_t codes = c.expect | ye << 8;
        bad += c.sel ? hi != ((OLD & 0xFFFFu) | codes << 16) : lo != ((OLD & 0xFFFF0000u) | codes);
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
  if (lane == 0 && bad) {
    atomicAdd(err_total, bad);
    atomicAdd(&err_xcd[xcc], bad);
  }
}

// The running amax of a block, on the bits: among f32 that are not NaN the magnitude's bits order as the
// values do.  A NaN counts as 0, whatever it is: fmaxf would drop a quiet one but returns a NaN for a
// signalling one, and with it loses what it had seen before
__device__ __forceinline__ uint32_t cvt_amax(uint32_t amax, float x) {
  const uint32_t m = __float_as_uint(x) & 0x7FFFFFFFu;
  return max(amax, m > 0x7F800000u ? 0u : m);
}
// the OCP MX scale of a block from amax's bits: floor(log2(amax)) - emax as an E8M0 byte, clamped; 2^0 for
// amax = 0.  An infinite amax counts as FLT_MAX, so the byte is at most 254 - emax.  The exponent field of a
// subnormal amax is 0, which clamps to byte 0 as its true exponent would
__device__ __forceinline__ unsigned cvt_mx_scale(uint32_t amax, int emax) {
  if (amax == 0u) return 127u;
  const int b = (int)(min(amax, 0x7F7FFFFFu) >> 23) - emax;
  return (unsigned)(b < 0 ? 0 : b > 254 ? 254 : b);
}
// the largest finite value of the format times the scale, as an f32 no larger than FLT_MAX
__device__ __forceinline__ float cvt_limit(CvtSpec s, unsigned byte) {
  const int sh = cvt_e(s, s.cmax) + (int)byte - 127;
  const unsigned m = (unsigned)cvt_m(s, s.cmax);
  return 127 + cvt_ilog2(m) + sh > 254 ? 3.402823466e38f : __uint_as_float(cvt_fbits(m, sh));
}
// a NaN passes: the instruction turns it into the format's NaN, or the largest code where there is none
__device__ __forceinline__ float cvt_clamp(float x, float lim) { return x != x ? x : fminf(fmaxf(x, -lim), lim); }

// x [n / 8 blocks of 32] to codes and scales; n counts 16-byte pieces of x (6-bit formats: blocks)
template <int FMT, bool QUANT>
__global__ __launch_bounds__(256) void cvt_rows_kernel(const cvt_f4* __restrict__ x, size_t n,
                                                       const uint8_t* __restrict__ scales_in,
                                                       void* __restrict__ codes, uint8_t* __restrict__ scales_out) {
  const auto [lo, hi] = slab_of(n);
  constexpr CvtSpec S = cvt_spec(FMT);
  if constexpr (cvt_packed6(FMT)) {
    uint2* out = static_cast<uint2*>(codes);
    for (size_t blk = lo + threadIdx.x; blk < hi; blk += 256) {
      cvt_f4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load(&x[blk * 8 + u]);
      float e[32];
#pragma unroll
      for (int u = 0; u < 8; ++u) e[4 * u] = v[u].x, e[4 * u + 1] = v[u].y, e[4 * u + 2] = v[u].z, e[4 * u + 3] = v[u].w;
      unsigned byte;
      if (QUANT) {
        uint32_t amax = 0u;
#pragma unroll
        for (int k = 0; k < 32; ++k) amax = cvt_amax(amax, e[k]);
        byte = cvt_mx_scale(amax, S.emax);
        scales_out[blk] = (uint8_t)byte;
        const float lim = cvt_limit(S, byte);
#pragma unroll
        for (int k = 0; k < 32; ++k) e[k] = cvt_clamp(e[k], lim);
      } else {
        byte = scales_in[blk];
      }
      const u32x6 r = cvt_pk32<FMT>(e, cvt_scale_operand(byte));
      out[blk * 3] = make_uint2(r[0], r[1]);
      out[blk * 3 + 1] = make_uint2(r[2], r[3]);
      out[blk * 3 + 2] = make_uint2(r[4], r[5]);
    }
  } else {
    for (size_t base = lo + threadIdx.x; base < hi; base += 4 * 256) {
      cvt_f4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {  // all four loads in flight before the conversions
        const size_t i = base + u * 256;
        if (i < hi) v[u] = __builtin_nontemporal_load(&x[i]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const size_t i = base + u * 256;
        if (i >= hi) continue;  // uniform over the eight lanes of a block: slabs and n are multiples of 8
        cvt_f4 w = v[u];
        if constexpr (FMT == ODH_CVT_BF16) {
          static_cast<uint2*>(codes)[i] = make_uint2(cvt_pk_bf16(w.x, w.y), cvt_pk_bf16(w.z, w.w));
        } else {
          const size_t blk = i >> 3;
          unsigned byte;
          if (QUANT) {
            uint32_t amax = cvt_amax(cvt_amax(cvt_amax(cvt_amax(0u, w.x), w.y), w.z), w.w);
#pragma unroll
            for (int off = 1; off < 8; off <<= 1) amax = max(amax, __shfl_xor(amax, off, 64));
            byte = cvt_mx_scale(amax, S.emax);
            if ((i & 7) == 0) scales_out[blk] = (uint8_t)byte;
            const float lim = cvt_limit(S, byte);
            w.x = cvt_clamp(w.x, lim), w.y = cvt_clamp(w.y, lim), w.z = cvt_clamp(w.z, lim), w.w = cvt_clamp(w.w, lim);
          } else {
            byte = scales_in[blk];
          }
          const float s = cvt_scale_operand(byte);
          if constexpr (FMT == ODH_CVT_FP4) {
            uint32_t r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(0u, w.x, w.y, s, 0);
            r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, w.z, w.w, s, 1);
            static_cast<uint16_t*>(codes)[i] = (uint16_t)r;
          } else {
            uint32_t r = cvt_pk8<FMT, false>(0u, w.x, w.y, s);
            r = cvt_pk8<FMT, true>(r, w.z, w.w, s);
            static_cast<uint32_t*>(codes)[i] = r;
          }
        }
      }
    }
  }
}

// every format's kernels on one argument list
template <typename... Args>
void cvt_launch_probe(int fmt, hipStream_t stream, Args... args) {
  switch (fmt) {
    case ODH_CVT_FP8: cvt_probe_kernel<ODH_CVT_FP8><<<ODH_CVT_BLOCKS, 256, 0, stream>>>(args...); break;
    case ODH_CVT_BF8: cvt_probe_kernel<ODH_CVT_BF8><<<ODH_CVT_BLOCKS, 256, 0, stream>>>(args...); break;
    case ODH_CVT_FP6: cvt_probe_kernel<ODH_CVT_FP6><<<ODH_CVT_BLOCKS, 256, 0, stream>>>(args...); break;
    case ODH_CVT_BF6: cvt_probe_kernel<ODH_CVT_BF6><<<ODH_CVT_BLOCKS, 256, 0, stream>>>(args...); break;
    case ODH_CVT_FP4: cvt_probe_kernel<ODH_CVT_FP4><<<ODH_CVT_BLOCKS, 256, 0, stream>>>(args...); break;
    default: cvt_probe_kernel<ODH_CVT_BF16><<<ODH_CVT_BLOCKS, 256, 0, stream>>>(args...); break;
  }
}
template <bool QUANT, typename... Args>
void cvt_launch_rows(int fmt, int grid, hipStream_t stream, Args... args) {
  switch (fmt) {
    case ODH_CVT_FP8: cvt_rows_kernel<ODH_CVT_FP8, QUANT><<<grid, 256, 0, stream>>>(args...); break;
    case ODH_CVT_BF8: cvt_rows_kernel<ODH_CVT_BF8, QUANT><<<grid, 256, 0, stream>>>(args...); break;
    case ODH_CVT_FP6: cvt_rows_kernel<ODH_CVT_FP6, QUANT><<<grid, 256, 0, stream>>>(args...); break;
    case ODH_CVT_BF6: cvt_rows_kernel<ODH_CVT_BF6, QUANT><<<grid, 256, 0, stream>>>(args...); break;
    case ODH_CVT_FP4: cvt_rows_kernel<ODH_CVT_FP4, QUANT><<<grid, 256, 0, stream>>>(args...); break;
    default: cvt_rows_kernel<ODH_CVT_BF16, false><<<grid, 256, 0, stream>>>(args...); break;
  }
}

// host side: what the row entry points take.  x 16-byte aligned, codes 8-byte aligned; rows · K below 2^40
bool cvt_rows_ok(int fmt, const void* x, const void* codes, long rows, long K) {
  return cvt_fmt_ok(fmt) && rows > 0 && K > 0 && K % 32 == 0 && rows <= (1L << 40) / K && x && codes &&
         ((uintptr_t)x & 15) == 0 && ((uintptr_t)codes & 7) == 0;
}
// pieces the row kernel strides over: blocks for the 6-bit formats, 16 bytes of x otherwise
size_t cvt_pieces(int fmt, long rows, long K) { return (size_t)rows * (size_t)K / (cvt_packed6(fmt) ? 32 : 4); }
