// The quantiser for 16-bit rows: bfloat16 or float16 x [rows][K] to the codes and E8M0 scales cvt_rows_kernel
// makes of f32 rows, on the converters that read 16-bit sources:
//   v_cvt_scalef32_pk_fp8_bf16 / _f16, v_cvt_scalef32_pk_bf8_bf16 / _f16  — two values of one register to two bytes
//                                                                           in the low or high half (word select);
//   v_cvt_scalef32_pk_fp4_bf16 / _f16                                     — two values to two nibbles in one of the
//                                                                           four bytes (byte select);
//   v_cvt_scalef32_pk32_fp6_bf16 / _f16, v_cvt_scalef32_pk32_bf6_bf16 / _f16 — 16 registers of 32 values to 24 bytes.
// Nothing is widened to f32: a model's activations and weights are quantised from the two bytes an element they
// take in memory, without the f32 copy that cvt_rows_kernel needs.
//
// Included by gpu_probe.hip inside its anonymous namespace, after gpu_probe_cvt.h and gpu_probe_dcvt.h: it uses
// CvtSpec, cvt_m, cvt_mx_scale, cvt_limit, cvt_scale_operand, the vector types of both, slab_of and grid_for.
//
// Contract (QUANT): the codes and scales are, byte for byte, what cvt_rows_kernel<FMT, true> gives for the exactly
// widened values; gpu_probe_cvt.h states that rule.  Not QUANT: the caller's scales and the bare instruction.
//
// Everything before the conversion works on the 16-bit patterns, two elements to a register:
//   amax   among values that are not NaN the magnitude's bits order as the values do, in both types.  The
//          magnitude plus (0x7FFF - the bits of infinity) is at most 0x7FFF for a number and has bit 15 set for a
//          NaN: as SIGNED 16-bit integers every NaN lies below every number, so a packed signed maximum that starts
//          at the biased zero never sees one (a NaN counts as 0), and a packed signed minimum against the biased
//          limit clamps the numbers and lets a NaN pass.  One v_pk_add_u16, one v_pk_max_i16 and one v_pk_min_i16
//          per two elements;
//   scale  bfloat16 has f32's exponent field, so the byte is cvt_mx_scale of the bits shifted up.  float16:
//          floor(log2 amax) is its 5-bit field minus 15, and for a subnormal amax (2^-24 … 2^-15, field 0) the
//          position of its leading one minus 24: those are normal f32, so "field 0 clamps to byte 0" would be wrong;
//   limit  v(cmax) · 2^(byte - 127) has at most four significant bits and the exponent of amax, so it is a number of
//          the source type, except under a float16-subnormal amax, where its low bits can fall below 2^-24.  There
//          it is rounded down: every element is an integer number of 2^-24 below the next power of two, and the
//          limit rounded down is still the largest such integer or more, so no element exceeds it;
//   Inf    in bfloat16 an infinity is clamped like any number: the limit at byte 254 - emax is a bfloat16.  In
//          float16 it is not (2^127), and the scale 2^(127 - emax) sends every finite float16 to zero.  Such a
//          block takes a path of its own: ±Inf becomes ±v(cmax) and every finite element ±0, converted at 2^0,
//          while the byte written is 254 - emax; a NaN stays.
//
// fp8, bf8, fp4 (cvt16_rows_kernel): a lane takes 16 bytes = 8 elements, four lanes a block of 32: amax by two
// quad permutes (DPP, no LDS traffic), the first lane of a block writes the scale, every lane 8 (fp8, bf8) or 4
// (fp4) bytes of codes.  On the sweep's slabs, four non-temporal loads in flight per lane.
//
// fp6, bf6 (cvt16_rows6_kernel): the one instruction wants a block's 64 bytes in one lane.  A workgroup regroups a
// tile of 256 blocks (16 KiB) through LDS instead of letting every lane fetch its own 64 bytes from four cache
// lines: consecutive lanes load consecutive 16-byte pieces (the next tile's are in flight while this one is
// converted) and write them to LDS, a block every 80 bytes: 20 dwords, so the sixteen lanes that a 16-byte LDS read
// serves at a time start in sixteen different groups of four banks.  Each lane reads its block back, takes amax,
// scale and clamp alone and converts; the 24 bytes of codes go to LDS and leave as 16-byte stores by consecutive
// lanes (a last 8 bytes where a short tile has an odd number of blocks); the scale bytes leave as 64 consecutive
// bytes a wave.

typedef __attribute__((ext_vector_type(2))) unsigned short u16x2;
typedef __attribute__((ext_vector_type(32))) __bf16 bf16x32;
typedef __attribute__((ext_vector_type(32))) _Float16 f16x32;

__host__ __device__ constexpr bool cvt16_src_ok(int src) { return src == ODH_DCVT_F16 || src == ODH_DCVT_BF16; }
// the bits of infinity, and what lifts every NaN's magnitude into the sign bit
__host__ __device__ constexpr uint32_t cvt16_inf(int src) { return src == ODH_DCVT_F16 ? 0x7C00u : 0x7F80u; }
__host__ __device__ constexpr uint32_t cvt16_bias(int src) { return 0x7FFFu - cvt16_inf(src); }

__device__ __forceinline__ i16x2 cvt16_splat(uint32_t h) { return __builtin_bit_cast(i16x2, h * 0x10001u); }
// the biased magnitudes of the two elements of w
template <int SRC>
__device__ __forceinline__ i16x2 cvt16_biased(uint32_t w) {
  return __builtin_bit_cast(i16x2, __builtin_bit_cast(u16x2, w & 0x7FFF7FFFu) +
                                       __builtin_bit_cast(u16x2, cvt16_bias(SRC) * 0x10001u));
}
// the larger of the two halves of a running maximum, as the magnitude's bits
template <int SRC>
__device__ __forceinline__ int cvt16_halves(i16x2 a) { return (a.x > a.y ? a.x : a.y) - (int)cvt16_bias(SRC); }
// the two elements of w clamped to the biased limit; t is cvt16_biased(w).  A NaN passes, the signs stay
template <int SRC>
__device__ __forceinline__ uint32_t cvt16_clamp(uint32_t w, i16x2 t, i16x2 limb) {
  const u16x2 m = __builtin_bit_cast(u16x2, __builtin_elementwise_min(t, limb)) -
                  __builtin_bit_cast(u16x2, cvt16_bias(SRC) * 0x10001u);
  return __builtin_bit_cast(uint32_t, m) | (w & 0x80008000u);
}
// float16, a block with an infinity: ±Inf to ±vmax, finite to ±0, a NaN as it is (converted at 2^0)
__device__ __forceinline__ uint32_t cvt16_inf_block(uint32_t w, uint32_t vmax) {
  const uint32_t lo = w & 0x7FFFu, hi = (w >> 16) & 0x7FFFu;
  return (w & 0x80008000u) | (lo > 0x7C00u ? lo : lo == 0x7C00u ? vmax : 0u) |
         (hi > 0x7C00u ? hi : hi == 0x7C00u ? vmax : 0u) << 16;
}

// the OCP MX scale byte of a block from the bits of its amax (no NaN: at most the bits of infinity)
template <int SRC>
__device__ __forceinline__ unsigned cvt16_mx_scale(uint32_t amax, int emax) {
  if constexpr (SRC == ODH_DCVT_BF16) return cvt_mx_scale(amax << 16, emax);
  if (amax == 0u) return 127u;
  if (amax >= 0x7C00u) return (unsigned)(254 - emax);  // an infinity counts as FLT_MAX
  const int field = (int)(amax >> 10);
  // floor(log2): field - 15, or for a subnormal (an integer number of 2^-24) the place of its leading one - 24
  return (unsigned)((field ? field - 15 : 7 - __clz((int)amax)) + 127 - emax);
}
// the bits, in the source type, of v(cmax) · 2^(byte - 127); rounded down where float16 cannot hold it
template <int SRC>
__device__ __forceinline__ uint32_t cvt16_limit(CvtSpec s, unsigned byte) {
  if constexpr (SRC == ODH_DCVT_BF16) return __float_as_uint(cvt_limit(s, byte)) >> 16;
  const int m = cvt_m(s, s.cmax);             // mbits + 1 significant bits
  const int e = (int)byte - 127 + s.emax;     // the exponent of amax and of the limit: -24 … 15
  const int sh = e + 24 - s.mbits;            // subnormal: m · 2^sh times 2^-24
  return e >= -14 ? (uint32_t)((e + 15) << 10 | ((m << (10 - s.mbits)) & 0x3FF))
                  : (uint32_t)(sh >= 0 ? m << sh : m >> -sh);
}
// v(cmax) itself as float16 bits
__device__ __forceinline__ uint32_t cvt16_vmax_f16(CvtSpec s) {
  return (uint32_t)((s.emax + 15) << 10 | ((cvt_m(s, s.cmax) << (10 - s.mbits)) & 0x3FF));
}

// the two elements of w to two bytes (fp8, bf8: SEL 0 / 1 the low / high half of old) or two nibbles (fp4: byte
// SEL of old)
template <int FMT, int SRC, int SEL>
__device__ __forceinline__ uint32_t cvt16_pk(uint32_t old, uint32_t w, float scale) {
  const i16x2 o = __builtin_bit_cast(i16x2, old);
  if constexpr (SRC == ODH_DCVT_BF16) {
    const bf16x2 v = __builtin_bit_cast(bf16x2, w);
    if constexpr (FMT == ODH_CVT_FP8)
      return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(o, v, scale, SEL != 0));
    else if constexpr (FMT == ODH_CVT_BF8)
      return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf8_bf16(o, v, scale, SEL != 0));
    else
      return __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(old, v, scale, SEL);
  } else {
    const f16x2 v = __builtin_bit_cast(f16x2, w);
    if constexpr (FMT == ODH_CVT_FP8)
      return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(o, v, scale, SEL != 0));
    else if constexpr (FMT == ODH_CVT_BF8)
      return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf8_f16(o, v, scale, SEL != 0));
    else
      return __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(old, v, scale, SEL);
  }
}
// a block of 32 in 16 registers to its 24 bytes: element k in bits [6k, 6k + 6)
template <int FMT, int SRC>
__device__ __forceinline__ u32x6 cvt16_pk32(const uint32_t (&w)[16], float scale) {
  u32x16 v;
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = w[i];
  if constexpr (SRC == ODH_DCVT_BF16) {
    if constexpr (FMT == ODH_CVT_FP6)
      return __builtin_amdgcn_cvt_scalef32_pk32_fp6_bf16(__builtin_bit_cast(bf16x32, v), scale);
    else
      return __builtin_amdgcn_cvt_scalef32_pk32_bf6_bf16(__builtin_bit_cast(bf16x32, v), scale);
  } else {
    if constexpr (FMT == ODH_CVT_FP6)
      return __builtin_amdgcn_cvt_scalef32_pk32_fp6_f16(__builtin_bit_cast(f16x32, v), scale);
    else
      return __builtin_amdgcn_cvt_scalef32_pk32_bf6_f16(__builtin_bit_cast(f16x32, v), scale);
  }
}

// QUANT, what a lane holds of a block in w[N] with the block's amax known: clamps w and returns the scale
// operand's byte (the byte written is cvt16_mx_scale's, which differs only in float16's block with an infinity)
template <int FMT, int SRC, int N>
__device__ __forceinline__ unsigned cvt16_saturate(uint32_t (&w)[N], const i16x2 (&t)[N], uint32_t amax, unsigned byte) {
  constexpr CvtSpec S = cvt_spec(FMT);
  if (SRC == ODH_DCVT_F16 && amax == 0x7C00u) {
    const uint32_t vmax = cvt16_vmax_f16(S);
#pragma unroll
    for (int r = 0; r < N; ++r) w[r] = cvt16_inf_block(w[r], vmax);
    return 127u;
  }
  const i16x2 limb = cvt16_splat(cvt16_limit<SRC>(S, byte) + cvt16_bias(SRC));
#pragma unroll
  for (int r = 0; r < N; ++r) w[r] = cvt16_clamp<SRC>(w[r], t[r], limb);
  return byte;
}

// lane ^ 1 and lane ^ 2 by quad permutes
__device__ __forceinline__ int cvt16_quad_max(int v) {
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));  // quad_perm [1, 0, 3, 2]
  return max(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));  // quad_perm [2, 3, 0, 1]
}

// fp8, bf8, fp4: x [n / 4 blocks of 32] to codes and scales; n counts 16-byte pieces of x
template <int FMT, int SRC, bool QUANT>
__global__ __launch_bounds__(256) void cvt16_rows_kernel(const u32x4* __restrict__ x, size_t n,
                                                         const uint8_t* __restrict__ scales_in,
                                                         void* __restrict__ codes, uint8_t* __restrict__ scales_out) {
  const auto [lo, hi] = slab_of(n);
  constexpr CvtSpec S = cvt_spec(FMT);
  for (size_t base = lo + threadIdx.x; base < hi; base += 4 * 256) {
    u32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // all four loads in flight before the conversions
      const size_t i = base + u * 256;
      if (i < hi) v[u] = __builtin_nontemporal_load(&x[i]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const size_t i = base + u * 256;
      if (i >= hi) continue;  // uniform over the four lanes of a block: slabs and n are multiples of 4
      uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
      const size_t blk = i >> 2;
      unsigned op;
      if (QUANT) {
        const i16x2 t[4] = {cvt16_biased<SRC>(w[0]), cvt16_biased<SRC>(w[1]), cvt16_biased<SRC>(w[2]),
                            cvt16_biased<SRC>(w[3])};
        const i16x2 a = __builtin_elementwise_max(__builtin_elementwise_max(t[0], t[1]),
                                                  __builtin_elementwise_max(t[2], t[3]));
        // eight NaN leave a negative maximum: they count as 0
        const uint32_t amax = (uint32_t)cvt16_quad_max(max(cvt16_halves<SRC>(a), 0));
        const unsigned byte = cvt16_mx_scale<SRC>(amax, S.emax);
        if ((i & 3) == 0) scales_out[blk] = (uint8_t)byte;
        op = cvt16_saturate<FMT, SRC>(w, t, amax, byte);
      } else {
        op = scales_in[blk];
      }
      const float s = cvt_scale_operand(op);
      if constexpr (FMT == ODH_CVT_FP4) {
        uint32_t r = cvt16_pk<FMT, SRC, 0>(0u, w[0], s);
        r = cvt16_pk<FMT, SRC, 1>(r, w[1], s);
        r = cvt16_pk<FMT, SRC, 2>(r, w[2], s);
        r = cvt16_pk<FMT, SRC, 3>(r, w[3], s);
        static_cast<uint32_t*>(codes)[i] = r;
      } else {
        const uint32_t r0 = cvt16_pk<FMT, SRC, 1>(cvt16_pk<FMT, SRC, 0>(0u, w[0], s), w[1], s);
        const uint32_t r1 = cvt16_pk<FMT, SRC, 1>(cvt16_pk<FMT, SRC, 0>(0u, w[2], s), w[3], s);
        static_cast<uint2*>(codes)[i] = make_uint2(r0, r1);
      }
    }
  }
}

constexpr int CVT16_TILE = 256;  // blocks a workgroup regroups at a time: one a lane, 1024 pieces, a slab's unit
constexpr int CVT16_PITCH = 5;   // 16-byte pieces from block to block in LDS: four of data, one of padding

// fp6, bf6: the same, a tile of 256 blocks at a time through LDS
template <int FMT, int SRC, bool QUANT>
__global__ __launch_bounds__(256) void cvt16_rows6_kernel(const u32x4* __restrict__ x, size_t n,
                                                          const uint8_t* __restrict__ scales_in,
                                                          void* __restrict__ codes, uint8_t* __restrict__ scales_out) {
  __shared__ u32x4 in[CVT16_TILE * CVT16_PITCH];  // 20 KiB
  __shared__ u32x4 out[CVT16_TILE * 24 / 16];     // 6 KiB
  constexpr CvtSpec S = cvt_spec(FMT);
  const auto [lo, hi] = slab_of(n);
  const int tid = threadIdx.x;
  u32x4 v[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const size_t i = lo + u * 256 + tid;
    if (i < hi) v[u] = __builtin_nontemporal_load(&x[i]);
  }
  for (size_t tile = lo; tile < hi; tile += 4 * CVT16_TILE) {
    const int np = (int)(hi - tile < 4 * CVT16_TILE ? hi - tile : 4 * CVT16_TILE);  // pieces of this tile
    const int nb = np >> 2;                                                         // its blocks
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int p = u * 256 + tid;
      if (p < np) in[(p >> 2) * CVT16_PITCH + (p & 3)] = v[u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // the next tile's loads fly while this one is converted
      const size_t i = tile + 4 * CVT16_TILE + u * 256 + tid;
      if (i < hi) v[u] = __builtin_nontemporal_load(&x[i]);
    }
    __syncthreads();
    if (tid < nb) {
      const size_t blk = (tile >> 2) + tid;
      uint32_t w[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const u32x4 r = in[tid * CVT16_PITCH + q];
        w[4 * q] = r.x, w[4 * q + 1] = r.y, w[4 * q + 2] = r.z, w[4 * q + 3] = r.w;
      }
      unsigned op;
      if (QUANT) {
        i16x2 t[16];
        i16x2 a = cvt16_splat(cvt16_bias(SRC));
#pragma unroll
        for (int r = 0; r < 16; ++r) t[r] = cvt16_biased<SRC>(w[r]), a = __builtin_elementwise_max(a, t[r]);
        const uint32_t amax = (uint32_t)cvt16_halves<SRC>(a);
        const unsigned byte = cvt16_mx_scale<SRC>(amax, S.emax);
        scales_out[blk] = (uint8_t)byte;
        op = cvt16_saturate<FMT, SRC>(w, t, amax, byte);
      } else {
        op = scales_in[blk];
      }
      const u32x6 r = cvt16_pk32<FMT, SRC>(w, cvt_scale_operand(op));
      uint2* o = reinterpret_cast<uint2*>(out) + tid * 3;
      o[0] = make_uint2(r[0], r[1]);
      o[1] = make_uint2(r[2], r[3]);
      o[2] = make_uint2(r[4], r[5]);
    }
    __syncthreads();
    // 24 · nb bytes from byte 24 · (tile / 4) of the codes on: a tile starts at a multiple of 256 blocks
    u32x4* dst = static_cast<u32x4*>(codes) + (tile >> 2) / 2 * 3;
    const int n16 = nb * 3 / 2;
    for (int j = tid; j < n16; j += 256) dst[j] = out[j];
    if ((nb & 1) && tid == 0) *reinterpret_cast<uint2*>(dst + n16) = reinterpret_cast<const uint2*>(out)[nb * 3 - 1];
  }
}

// every format's and source type's kernel on one argument list
template <int SRC, bool QUANT, typename... Args>
void cvt16_launch_src(int fmt, int grid, hipStream_t stream, Args... args) {
  switch (fmt) {
    case ODH_CVT_FP8: cvt16_rows_kernel<ODH_CVT_FP8, SRC, QUANT><<<grid, 256, 0, stream>>>(args...); break;
    case ODH_CVT_BF8: cvt16_rows_kernel<ODH_CVT_BF8, SRC, QUANT><<<grid, 256, 0, stream>>>(args...); break;
    case ODH_CVT_FP6: cvt16_rows6_kernel<ODH_CVT_FP6, SRC, QUANT><<<grid, 256, 0, stream>>>(args...); break;
    case ODH_CVT_BF6: cvt16_rows6_kernel<ODH_CVT_BF6, SRC, QUANT><<<grid, 256, 0, stream>>>(args...); break;
    default: cvt16_rows_kernel<ODH_CVT_FP4, SRC, QUANT><<<grid, 256, 0, stream>>>(args...); break;
  }
}
template <bool QUANT, typename... Args>
void cvt16_launch_rows(int fmt, int src, int grid, hipStream_t stream, Args... args) {
  if (src == ODH_DCVT_F16)
    cvt16_launch_src<ODH_DCVT_F16, QUANT>(fmt, grid, stream, args...);
  else
    cvt16_launch_src<ODH_DCVT_BF16, QUANT>(fmt, grid, stream, args...);
}

// host side: what the 16-bit row entry points take.  x 16-byte aligned; codes 16-byte aligned for the 6-bit
// formats, which leave in 16-byte stores, 8-byte otherwise; rows · K below 2^40
bool cvt16_rows_ok(int fmt, int src, const void* x, const void* codes, const void* scales, long rows, long K) {
  return cvt_scaled(fmt) && cvt16_src_ok(src) && rows > 0 && K > 0 && K % 32 == 0 && rows <= ((1L << 40) - 1) / K &&
         x && codes && scales && ((uintptr_t)x & 15) == 0 && ((uintptr_t)codes & (cvt_packed6(fmt) ? 15 : 7)) == 0;
}
