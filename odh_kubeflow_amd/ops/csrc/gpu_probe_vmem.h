// The start-up probe's vector-memory step: the path between a CU's registers and HBM that the 256 MiB sweep
// (16-byte, aligned, non-temporal, written and read once) leaves untouched:
//   cache  a slab written and re-read through the vector L1 and the XCD's L2: 16-byte stores and 4-byte loads by
//          another wave, three times (L1 fill, L1 hit, L1 bypass = L2 hit), and the reverse widths;
//   sub    byte enables and odd widths: dwords assembled from byte and 16-bit stores (plain and d16_hi forms) by
//          three waves, the extending and half-register loads (ubyte, sbyte, ushort, sshort, short_d16,
//          short_d16_hi), and 8-, 12- and 16-byte accesses at 4-byte alignment across 64- and 128-byte lines;
//   buf    buffer-descriptor addressing (__builtin_amdgcn_make_buffer_rsrc, buffer_load / buffer_store of 1, 2, 4,
//          8, 12 and 16 bytes) and its range check: lanes past num_records read 0 and write nothing;
//   dma    the global -> LDS direct loads (global_load_lds_dword / _dwordx3 / _dwordx4, buffer_load_dwordx4 ... lds).
// A fault in any of them gives wrong operands with no error.
//
// Included by gpu_probe.hip inside its anonymous namespace, after gpu_probe_lds.h: it uses lds_smem, lds_mix,
// lds_fold, lds_book_block, lds_book_errors and LdsLaneAddr.
//
// Rules every kernel here keeps.  A fused check launches ODH_VM_BLOCKS workgroups of 256 threads that claim
// VM_LDS_BYTES of LDS, more than half of a CU's, so a CU takes one workgroup.  Workgroup b owns bytes
// [b ODH_VM_SLAB, (b + 1) ODH_VM_SLAB) of the arena and no workgroup reads, writes or waits for another's slab: the
// only synchronisation is __syncthreads() behind s_waitcnt vmcnt(0).  Every address a lane can form lies inside its
// workgroup's slab, whatever the table holds and whether or not a buffer's range check clamps: the largest buffer
// offset a lane forms, VM_BUF_SOFF + VM_BUF_IMM + 64 * 16, is inside the wave's quarter of the slab.  Every access
// under test is inline assembly (global_*, buffer_*) or the exact builtin (the LDS-DMA loads), so that it is the
// instruction its name says: the compiler narrows a buffer load whose components are not all used and folds a
// constant into the immediate only sometimes.
//
// The data-only fault, as in gpu_probe_lds.h.  odh_vmem_fill writes 256 key dwords, vm_key(check, i).  A stored
// dword is a closed form of its dword index w in the slab and the pass, XOR vm_spread(key[(w + 37 pass) mod 256])
// READ FROM THE TABLE; what it is compared with uses vm_key computed in registers.  vm_spread is the XOR of the
// key's four bytes in every byte of a dword, so any change of one table byte changes every byte of every element
// that uses that key dword, whatever the width of the access: odh_vmem_fault_count is exact.  Even passes store
// the value and odd passes its complement, so every bit is moved as 0 and as 1.
//
// Measured one access at a time with odh_vmem_access on an MI355X (profiles/vmem_probe/SUMMARY.txt):
//   * the scalar offset of a buffer access is part of the range check: a lane is in range when scalar offset + vector
//     offset + immediate + width <= num_records (VM_SOFF_CHECKED);
//   * partial buffer accesses: the range is checked per dword.  Of a 8-, 12- or 16-byte load whose range ends inside
//     it the dwords in range arrive and the others are 0; of such a store the dwords in range land and the others
//     are dropped.  A 16-bit access that the range cuts is dropped whole.  The fused check ends every range on a
//     multiple of the access size, so it does not depend on this;
//   * global_load_short_d16 / _d16_hi write 0 to the other half of the destination: the MI355X runs with SRAM ECC,
//     under which the d16 loads do not preserve it (VM_D16_KEEPS).  The check expects that 0 in a register that
//     held something else;
//   * the immediate of an LDS-DMA load is added to the global (or buffer) address and to the LDS address.  Lane l's
//     data lands at M0 base + immediate + l * size for 4 and 16 bytes, and at M0 base + immediate + 16 l for 12
//     bytes: a 12-byte lane has a 16-byte slot whose last dword is left as it was (vm_dma_stride).  A buffer lane
//     past the end lands zeros, per dword as above.

typedef __attribute__((ext_vector_type(2))) unsigned vm_u32x2;
typedef __attribute__((ext_vector_type(3))) unsigned vm_u32x3;
#define ODH_VM_GLOBAL __attribute__((address_space(1)))

constexpr int VM_LDS_BYTES = 96 * 1024;  // the launch's claim: more than half of a CU's LDS
constexpr int VM_WAVE_DWORDS = ODH_VM_SLAB / 16;  // a wave's quarter of the slab, in dwords
constexpr bool VM_SOFF_CHECKED = true;  // whether the range check of a buffer access counts the scalar offset
constexpr bool VM_D16_KEEPS = false;    // whether a d16 load keeps the other half of its destination (else: writes 0)

__host__ __device__ constexpr bool vm_check_ok(int check) { return check >= ODH_VM_CACHE && check <= ODH_VM_DMA; }
__host__ __device__ constexpr uint32_t vm_key(int check, uint32_t i) {
  return lds_mix(0xC2B2AE35u * (i + 1) + 0x27D4EB2Fu * (uint32_t)(check + 1));
}
__host__ __device__ constexpr uint32_t vm_spread(uint32_t key) { return lds_fold(key, 8) * 0x01010101u; }
__host__ __device__ constexpr uint32_t vm_kidx(uint32_t w, int pass) { return (w + 37u * (uint32_t)(pass & ~1)) & 255u; }
// dword w of the slab in pass `pass`: passes 2 q and 2 q + 1 are a value and its complement
__host__ __device__ constexpr uint32_t vm_value(int check, uint32_t w, int pass, uint32_t key) {
  const uint32_t v = lds_mix(w * 0x9E3779B1u + (uint32_t)(pass & ~1) * 0x632BE5ABu + (uint32_t)check + 1u) ^ vm_spread(key);
  return pass & 1 ? ~v : v;
}
__host__ __device__ constexpr int vm_reads_wave(int wave, int i) { return (wave + 1 + i % 3) & 3; }

__global__ void vm_fill_kernel(int check, uint32_t* __restrict__ table) { table[threadIdx.x] = vm_key(check, threadIdx.x); }

// what a kernel stores (key from the table) and what it expects (key in registers)
template <int CHECK>
__device__ __forceinline__ uint32_t vm_stored(const uint32_t* table, uint32_t w, int pass) {
  return vm_value(CHECK, w, pass, table[vm_kidx(w, pass)]);
}
template <int CHECK>
__device__ __forceinline__ uint32_t vm_want(uint32_t w, int pass) {
  return vm_value(CHECK, w, pass, vm_key(CHECK, vm_kidx(w, pass)));
}

// ------------------------------------------------------------------ the accesses
//
// A load waits for its own data (the compiler does not count what inline assembly issues); a kernel waits for its
// stores with vm_wait() before the barrier that hands them to another wave.
#define VM_DEF_LOAD(fn, T, text)                                                          \
  __device__ __forceinline__ T fn(const void* p) {                                        \
    T r;                                                                                  \
    asm volatile(text "\n\ts_waitcnt vmcnt(0)" : "=&v"(r) : "v"(p) : "memory");           \
    return r;                                                                             \
  }
#define VM_DEF_LOAD_D16(fn, text)                                                         \
  __device__ __forceinline__ uint32_t fn(const void* p, uint32_t keep) {                  \
    asm volatile(text "\n\ts_waitcnt vmcnt(0)" : "+v"(keep) : "v"(p) : "memory");         \
    return keep;                                                                          \
  }
#define VM_DEF_STORE(fn, T, text)                                                         \
  __device__ __forceinline__ void fn(void* p, T v) { asm volatile(text : : "v"(p), "v"(v) : "memory"); }
VM_DEF_LOAD(vm_ld_u8, uint32_t, "global_load_ubyte %0, %1, off")
VM_DEF_LOAD(vm_ld_i8, uint32_t, "global_load_sbyte %0, %1, off")
VM_DEF_LOAD(vm_ld_u16, uint32_t, "global_load_ushort %0, %1, off")
VM_DEF_LOAD(vm_ld_i16, uint32_t, "global_load_sshort %0, %1, off")
VM_DEF_LOAD_D16(vm_ld_d16, "global_load_short_d16 %0, %1, off")
VM_DEF_LOAD_D16(vm_ld_d16_hi, "global_load_short_d16_hi %0, %1, off")
VM_DEF_LOAD(vm_ld_b32, uint32_t, "global_load_dword %0, %1, off")
VM_DEF_LOAD(vm_ld_b32_l2, uint32_t, "global_load_dword %0, %1, off sc1")  // agent scope: the L1 is bypassed
VM_DEF_LOAD(vm_ld_b64, vm_u32x2, "global_load_dwordx2 %0, %1, off")
VM_DEF_LOAD(vm_ld_b96, vm_u32x3, "global_load_dwordx3 %0, %1, off")
VM_DEF_LOAD(vm_ld_b128, u32x4, "global_load_dwordx4 %0, %1, off")
VM_DEF_LOAD(vm_ld_b128_l2, u32x4, "global_load_dwordx4 %0, %1, off sc1")
VM_DEF_STORE(vm_st_b8, uint32_t, "global_store_byte %0, %1, off")
VM_DEF_STORE(vm_st_b16, uint32_t, "global_store_short %0, %1, off")
VM_DEF_STORE(vm_st_b8_hi, uint32_t, "global_store_byte_d16_hi %0, %1, off")    // bits 16-23 of the register
VM_DEF_STORE(vm_st_b16_hi, uint32_t, "global_store_short_d16_hi %0, %1, off")  // bits 16-31
VM_DEF_STORE(vm_st_b32, uint32_t, "global_store_dword %0, %1, off")
VM_DEF_STORE(vm_st_b64, vm_u32x2, "global_store_dwordx2 %0, %1, off")
VM_DEF_STORE(vm_st_b96, vm_u32x3, "global_store_dwordx3 %0, %1, off")
VM_DEF_STORE(vm_st_b128, u32x4, "global_store_dwordx4 %0, %1, off")
__device__ __forceinline__ void vm_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// a raw buffer (stride 0, no swizzle) of num_records bytes at p: DATA_FORMAT 32 in the fourth dword
// (p and num_records are uniform over the wave; the compiler is told so, since a descriptor lives in scalar registers)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t vm_rsrc(void* p, unsigned num_records) {
  const uint64_t a = (uint64_t)(uintptr_t)p;
  const uint64_t u = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a) |
                     ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32)) << 32);
  return __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)u, 0, __builtin_amdgcn_readfirstlane((int)num_records), 0x00020000);
}
#define VM_DEF_BUF_LOAD(fn, T, insn)                                                                       \
  template <int IMM>                                                                                       \
  __device__ __forceinline__ T fn(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {               \
    T r;                                                                                                   \
    asm volatile(insn " %0, %1, %2, %3 offen offset:%4\n\ts_waitcnt vmcnt(0)"                              \
                 : "=&v"(r)                                                                                \
                 : "v"(voff), "s"(rs), "s"(soff), "n"(IMM)                                                 \
                 : "memory");                                                                              \
    return r;                                                                                              \
  }
#define VM_DEF_BUF_STORE(fn, T, insn)                                                                      \
  template <int IMM>                                                                                       \
  __device__ __forceinline__ void fn(T v, __amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {       \
    asm volatile(insn " %0, %1, %2, %3 offen offset:%4" : : "v"(v), "v"(voff), "s"(rs), "s"(soff), "n"(IMM) : "memory"); \
  }
VM_DEF_BUF_LOAD(vm_buf_ld_b8, uint32_t, "buffer_load_ubyte")
VM_DEF_BUF_LOAD(vm_buf_ld_b16, uint32_t, "buffer_load_ushort")
VM_DEF_BUF_LOAD(vm_buf_ld_b32, uint32_t, "buffer_load_dword")
VM_DEF_BUF_LOAD(vm_buf_ld_b64, vm_u32x2, "buffer_load_dwordx2")
VM_DEF_BUF_LOAD(vm_buf_ld_b96, vm_u32x3, "buffer_load_dwordx3")
VM_DEF_BUF_LOAD(vm_buf_ld_b128, u32x4, "buffer_load_dwordx4")
VM_DEF_BUF_STORE(vm_buf_st_b8, uint32_t, "buffer_store_byte")
VM_DEF_BUF_STORE(vm_buf_st_b16, uint32_t, "buffer_store_short")
VM_DEF_BUF_STORE(vm_buf_st_b32, uint32_t, "buffer_store_dword")
VM_DEF_BUF_STORE(vm_buf_st_b64, vm_u32x2, "buffer_store_dwordx2")
VM_DEF_BUF_STORE(vm_buf_st_b96, vm_u32x3, "buffer_store_dwordx3")
VM_DEF_BUF_STORE(vm_buf_st_b128, u32x4, "buffer_store_dwordx4")

// a buffer access of W bytes as up to four dwords (a byte or a short in the low bits of the first)
template <int W, int IMM>
__device__ __forceinline__ u32x4 vm_buf_load(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
  u32x4 o = {0, 0, 0, 0};
  if constexpr (W == 1) o[0] = vm_buf_ld_b8<IMM>(rs, voff, soff);
  else if constexpr (W == 2) o[0] = vm_buf_ld_b16<IMM>(rs, voff, soff);
  else if constexpr (W == 4) o[0] = vm_buf_ld_b32<IMM>(rs, voff, soff);
  else if constexpr (W == 8) { const vm_u32x2 r = vm_buf_ld_b64<IMM>(rs, voff, soff); o[0] = r[0], o[1] = r[1]; }
  else if constexpr (W == 12) { const vm_u32x3 r = vm_buf_ld_b96<IMM>(rs, voff, soff); o[0] = r[0], o[1] = r[1], o[2] = r[2]; }
  else o = vm_buf_ld_b128<IMM>(rs, voff, soff);
  return o;
}
template <int W, int IMM>
__device__ __forceinline__ void vm_buf_store(u32x4 v, __amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
  if constexpr (W == 1) vm_buf_st_b8<IMM>(v[0], rs, voff, soff);
  else if constexpr (W == 2) vm_buf_st_b16<IMM>(v[0], rs, voff, soff);
  else if constexpr (W == 4) vm_buf_st_b32<IMM>(v[0], rs, voff, soff);
  else if constexpr (W == 8) vm_buf_st_b64<IMM>(vm_u32x2{v[0], v[1]}, rs, voff, soff);
  else if constexpr (W == 12) vm_buf_st_b96<IMM>(vm_u32x3{v[0], v[1], v[2]}, rs, voff, soff);
  else vm_buf_st_b128<IMM>(v, rs, voff, soff);
}
// whether the range check lets a lane's access through
__host__ __device__ constexpr bool vm_buf_in_range(unsigned voff_imm, unsigned soff, unsigned w, unsigned num_records) {
  return (unsigned long long)voff_imm + (VM_SOFF_CHECKED ? soff : 0u) + w <= num_records;
}

// an LDS-DMA load of SIZE bytes per lane to LDS byte lds_base (uniform over the wave: it goes to M0).  The builtins
// take the size and the immediate as literals only, so every pair in use is spelled out
#define VM_DMA_PICK_IMM(CALL)                                  \
  if constexpr (IMM == 0) { CALL(0); }                         \
  else if constexpr (IMM == ODH_VM_ACCESS_IMM) { CALL(64); }   \
  else { static_assert(IMM == 2064, "add the literal"); CALL(2064); }
template <int SIZE, int IMM>
__device__ __forceinline__ void vm_dma_global(const void* p, uint32_t lds_base) {
  ODH_VM_GLOBAL void* g = (ODH_VM_GLOBAL void*)p;
  ODH_LDS_AS void* l = (ODH_LDS_AS void*)(lds_smem + lds_base);
#define VM_DMA_G4(I) __builtin_amdgcn_global_load_lds(g, l, 4, I, 0)
#define VM_DMA_G12(I) __builtin_amdgcn_global_load_lds(g, l, 12, I, 0)
#define VM_DMA_G16(I) __builtin_amdgcn_global_load_lds(g, l, 16, I, 0)
  if constexpr (SIZE == 4) { VM_DMA_PICK_IMM(VM_DMA_G4) }
  else if constexpr (SIZE == 12) { VM_DMA_PICK_IMM(VM_DMA_G12) }
  else { static_assert(SIZE == 16, "4, 12 or 16 bytes"); VM_DMA_PICK_IMM(VM_DMA_G16) }
}
template <int IMM>
__device__ __forceinline__ void vm_dma_buffer(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff, uint32_t lds_base) {
  ODH_LDS_AS void* l = (ODH_LDS_AS void*)(lds_smem + lds_base);
#define VM_DMA_B16(I) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, l, 16, (int)voff, (int)soff, I, 0)
  VM_DMA_PICK_IMM(VM_DMA_B16)
}

// ------------------------------------------------------------------ cache
//
// The slab's 16,384 dwords as 16 iterations of 1,024, gpu_probe_lds.h's mem check in global memory.  Even passes:
// wave v writes dwords [256 v, 256 v + 256) of every iteration 16 bytes wide; behind the barrier wave
// vm_reads_wave(v, i) reads them 4 bytes wide, per iteration three times: ordinary loads (the L1 fills), ordinary
// loads again (the L1 holds the 4 KiB), loads at agent scope, which the L1 does not serve (the L2 does).  Odd passes
// write the complement 4 bytes wide and read 16 bytes wide.  All twelve reads of every dword are compared.
constexpr int VM_CACHE_ITERS = ODH_VM_SLAB / 4096;
constexpr int VM_CACHE_PASSES = 4;
constexpr int VM_CACHE_READS = 3;

__global__ __launch_bounds__(256, 1) void vm_cache_kernel(const uint32_t* __restrict__ table, unsigned char* arena,
                                                          int* __restrict__ xcd_blocks, unsigned* __restrict__ err_total,
                                                          unsigned* __restrict__ err_xcd, unsigned* __restrict__ cu_bitmap) {
  constexpr int C = ODH_VM_CACHE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned xcc = lds_book_block(xcd_blocks, cu_bitmap);
  uint32_t* slab = reinterpret_cast<uint32_t*>(arena + (size_t)blockIdx.x * ODH_VM_SLAB);
  unsigned bad = 0;
  for (int pass = 0; pass < VM_CACHE_PASSES; ++pass) {
    if ((pass & 1) == 0) {
      for (int i = 0; i < VM_CACHE_ITERS; ++i) {
        const uint32_t w = 1024u * i + 256u * wave + 4u * lane;
        const u32x4 v = {vm_stored<C>(table, w, pass), vm_stored<C>(table, w + 1, pass), vm_stored<C>(table, w + 2, pass),
                         vm_stored<C>(table, w + 3, pass)};
        vm_st_b128(slab + w, v);
      }
      vm_wait();
      __syncthreads();
      for (int i = 0; i < VM_CACHE_ITERS; ++i) {
        const uint32_t w = 1024u * i + 256u * vm_reads_wave(wave, i) + lane;
        for (int rep = 0; rep < VM_CACHE_READS; ++rep) {
          uint32_t r0, r1, r2, r3;
          if (rep < 2)
            asm volatile(
                "global_load_dword %0, %4, off\n\tglobal_load_dword %1, %4, off offset:256\n\t"
                "global_load_dword %2, %4, off offset:512\n\tglobal_load_dword %3, %4, off offset:768\n\t"
                "s_waitcnt vmcnt(0)"
                : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3)
                : "v"(slab + w)
                : "memory");
          else
            asm volatile(
                "global_load_dword %0, %4, off sc1\n\tglobal_load_dword %1, %4, off offset:256 sc1\n\t"
                "global_load_dword %2, %4, off offset:512 sc1\n\tglobal_load_dword %3, %4, off offset:768 sc1\n\t"
                "s_waitcnt vmcnt(0)"
                : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3)
                : "v"(slab + w)
                : "memory");
          bad += r0 != vm_want<C>(w, pass);
          bad += r1 != vm_want<C>(w + 64, pass);
          bad += r2 != vm_want<C>(w + 128, pass);
          bad += r3 != vm_want<C>(w + 192, pass);
        }
      }
    } else {
      for (int i = 0; i < VM_CACHE_ITERS; ++i) {
        const uint32_t w = 1024u * i + 256u * wave + lane;
#pragma unroll
        for (int c = 0; c < 4; ++c) vm_st_b32(slab + w + 64 * c, vm_stored<C>(table, w + 64 * c, pass));
      }
      vm_wait();
      __syncthreads();
      for (int i = 0; i < VM_CACHE_ITERS; ++i) {
        const uint32_t w = 1024u * i + 256u * vm_reads_wave(wave, i) + 4u * lane;
        for (int rep = 0; rep < VM_CACHE_READS; ++rep) {
          const u32x4 r = rep < 2 ? vm_ld_b128(slab + w) : vm_ld_b128_l2(slab + w);
#pragma unroll
          for (int e = 0; e < 4; ++e) bad += r[e] != vm_want<C>(w + e, pass);
        }
      }
    }
    __syncthreads();  // the next pass overwrites what other waves have just read
  }
  lds_book_errors(bad, xcc, err_total, err_xcd);
}

// ------------------------------------------------------------------ sub
//
// The first 16 KiB of the slab, in three parts (dwords of the slab):
//   (a) [0, 512)      eight passes.  In pass p wave v has role (v + (p >> 1)) mod 4: role 0 stores byte 0 of every
//                     dword, role 1 byte 1, role 2 the upper half as one 16-bit store, and role 3 reads the dwords 16
//                     bytes wide behind the barrier.  Odd passes store the complement with the d16_hi forms, which
//                     take bits 16-23 or 16-31 of a register whose other bits hold the wrong value.
//   (b) [512, 1536)   four passes.  Wave v writes dwords [256 v, 256 v + 256) of the part 16 bytes wide; another wave
//                     reads every dword back 16 times: each byte unsigned and signed, each half unsigned and signed,
//                     and each half into the low (short_d16) and the high (short_d16_hi) half of a register whose
//                     other half held something else and must read 0 afterwards (VM_D16_KEEPS).  A value and its complement: every access sees both sign-bit states.
//   (c) [1536, 4096)  four passes, 640 dwords per wave.  Records of 8, 12 and 16 bytes, one per lane, at dwords 1,
//                     129 and 321 of the wave's 2,560-byte region: 4-byte aligned and not 8- or 16-byte aligned, so
//                     that lanes 7 and 15 (8 bytes), 10 and 15 (12) and 3 and 7 (16) straddle a 64- or a 128-byte
//                     line.  Written with global_store_dwordx2 / x3 / x4 and read by another wave with the loads of
//                     the same widths.
constexpr int VM_SUB_A = 0, VM_SUB_A_DWORDS = 512, VM_SUB_A_PASSES = 8;
constexpr int VM_SUB_B = 512, VM_SUB_B_DWORDS = 1024, VM_SUB_B_LOADS = 16;
constexpr int VM_SUB_C = 1536, VM_SUB_C_WAVE = 640, VM_SUB_C_W2 = 1, VM_SUB_C_W3 = 129, VM_SUB_C_W4 = 321;
constexpr int VM_SUB_PASSES = 4;  // of (b) and (c)
__host__ __device__ constexpr uint32_t vm_sext(uint32_t x, int bits) { return (uint32_t)((int32_t)(x << (32 - bits)) >> (32 - bits)); }

__global__ __launch_bounds__(256, 1) void vm_sub_kernel(const uint32_t* __restrict__ table, unsigned char* arena,
                                                        int* __restrict__ xcd_blocks, unsigned* __restrict__ err_total,
                                                        unsigned* __restrict__ err_xcd, unsigned* __restrict__ cu_bitmap) {
  constexpr int C = ODH_VM_SUB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned xcc = lds_book_block(xcd_blocks, cu_bitmap);
  uint32_t* slab = reinterpret_cast<uint32_t*>(arena + (size_t)blockIdx.x * ODH_VM_SLAB);
  unsigned bad = 0;
  // (a)
  for (int pass = 0; pass < VM_SUB_A_PASSES; ++pass) {
    const int role = (wave + (pass >> 1)) & 3;
    const bool hi = pass & 1;
    if (role < 3) {
      for (int c = 0; c < VM_SUB_A_DWORDS / 64; ++c) {
        const uint32_t w = VM_SUB_A + 64u * c + lane, v = vm_stored<C>(table, w, pass);
        unsigned char* p = reinterpret_cast<unsigned char*>(slab + w);
        const int width = role == 2 ? 16 : 8;
        const uint32_t piece = (role == 0 ? v : role == 1 ? v >> 8 : v >> 16) & ((1u << width) - 1u), junk = ~piece;
        // every bit of the register that the store must not take holds the wrong value
        const uint32_t reg = hi ? piece << 16 | (junk & 0xFFFFu) | (width == 8 ? junk << 24 : 0u) : piece | junk << width;
        if (role == 2) {
          if (hi) vm_st_b16_hi(p + 2, reg); else vm_st_b16(p + 2, reg);
        } else {
          if (hi) vm_st_b8_hi(p + role, reg); else vm_st_b8(p + role, reg);
        }
      }
    }
    vm_wait();
    __syncthreads();
    if (role == 3) {
      for (int c = 0; c < VM_SUB_A_DWORDS / 256; ++c) {
        const uint32_t w = VM_SUB_A + 256u * c + 4u * lane;
        const u32x4 r = vm_ld_b128(slab + w);
#pragma unroll
        for (int e = 0; e < 4; ++e) bad += r[e] != vm_want<C>(w + e, pass);
      }
    }
    __syncthreads();
  }
  // (b) and (c)
  for (int pass = 0; pass < VM_SUB_PASSES; ++pass) {
    {
      const uint32_t w = VM_SUB_B + 256u * wave + 4u * lane;
      const u32x4 v = {vm_stored<C>(table, w, pass), vm_stored<C>(table, w + 1, pass), vm_stored<C>(table, w + 2, pass),
                       vm_stored<C>(table, w + 3, pass)};
      vm_st_b128(slab + w, v);
      const uint32_t base = VM_SUB_C + (uint32_t)VM_SUB_C_WAVE * wave;
      const uint32_t w2 = base + VM_SUB_C_W2 + 2u * lane, w3 = base + VM_SUB_C_W3 + 3u * lane, w4 = base + VM_SUB_C_W4 + 4u * lane;
      vm_st_b64(slab + w2, vm_u32x2{vm_stored<C>(table, w2, pass), vm_stored<C>(table, w2 + 1, pass)});
      vm_st_b96(slab + w3, vm_u32x3{vm_stored<C>(table, w3, pass), vm_stored<C>(table, w3 + 1, pass), vm_stored<C>(table, w3 + 2, pass)});
      vm_st_b128(slab + w4, u32x4{vm_stored<C>(table, w4, pass), vm_stored<C>(table, w4 + 1, pass),
                                  vm_stored<C>(table, w4 + 2, pass), vm_stored<C>(table, w4 + 3, pass)});
    }
    vm_wait();
    __syncthreads();
    const int from = vm_reads_wave(wave, pass);
    for (int c = 0; c < 4; ++c) {
      const uint32_t w = VM_SUB_B + 256u * from + 64u * c + lane, x = vm_want<C>(w, pass);
      const uint32_t keep = lds_mix(w + 0x5A5Au);  // the register before a half-register load
      const unsigned char* p = reinterpret_cast<const unsigned char*>(slab + w);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        bad += vm_ld_u8(p + b) != (x >> 8 * b & 0xFFu);
        bad += vm_ld_i8(p + b) != vm_sext(x >> 8 * b & 0xFFu, 8);
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint32_t half = x >> 16 * h & 0xFFFFu;
        bad += vm_ld_u16(p + 2 * h) != half;
        bad += vm_ld_i16(p + 2 * h) != vm_sext(half, 16);
        bad += vm_ld_d16(p + 2 * h, keep) != ((VM_D16_KEEPS ? keep & 0xFFFF0000u : 0u) | half);
        bad += vm_ld_d16_hi(p + 2 * h, keep) != (half << 16 | (VM_D16_KEEPS ? keep & 0xFFFFu : 0u));
      }
    }
    {
      const uint32_t base = VM_SUB_C + (uint32_t)VM_SUB_C_WAVE * from;
      const uint32_t w2 = base + VM_SUB_C_W2 + 2u * lane, w3 = base + VM_SUB_C_W3 + 3u * lane, w4 = base + VM_SUB_C_W4 + 4u * lane;
      const vm_u32x2 r2 = vm_ld_b64(slab + w2);
      const vm_u32x3 r3 = vm_ld_b96(slab + w3);
      const u32x4 r4 = vm_ld_b128(slab + w4);
#pragma unroll
      for (int e = 0; e < 2; ++e) bad += r2[e] != vm_want<C>(w2 + e, pass);
#pragma unroll
      for (int e = 0; e < 3; ++e) bad += r3[e] != vm_want<C>(w3 + e, pass);
#pragma unroll
      for (int e = 0; e < 4; ++e) bad += r4[e] != vm_want<C>(w4 + e, pass);
    }
    __syncthreads();
  }
  lds_book_errors(bad, xcc, err_total, err_xcd);
}

// ------------------------------------------------------------------ buf
//
// Every wave works alone on its quarter of the slab through a descriptor of its own whose base is the quarter's
// first byte.  A round is a width W (1, 2, 4, 8, 12, 16) and a number n of lanes in range (0, 1, 23, 40, 63, 64):
// lane l accesses W bytes at base + VM_BUF_SOFF (scalar offset) + l W (vector offset) + VM_BUF_IMM (immediate), and
// num_records ends the range behind lane n - 1, on a multiple of W.  The round
//   1. writes the window, 320 dwords from VM_BUF_SOFF on, with the round's values, plain 4-byte stores;
//   2. buffer-stores the complement: it must land for lanes below n and nowhere else;
//   3. reads the window back with plain 4-byte loads: complement in [first, first + n W), the value everywhere
//      else, byte for byte.  The bytes behind the range, up to the window's end, are the guard zone;
//   4. buffer-loads with the same descriptor: lanes below n get the complement, the others 0.
constexpr int VM_BUF_SOFF = 768, VM_BUF_IMM = 48, VM_BUF_WINDOW = 320, VM_BUF_SIZES = 6, VM_BUF_RANGES = 6;
constexpr int VM_BUF_ROUNDS = VM_BUF_SIZES * VM_BUF_RANGES;
__host__ __device__ constexpr int vm_buf_size(int i) { constexpr int W[VM_BUF_SIZES] = {1, 2, 4, 8, 12, 16}; return W[i]; }
__host__ __device__ constexpr int vm_buf_lanes(int j) { constexpr int N[VM_BUF_RANGES] = {0, 1, 23, 40, 63, 64}; return N[j]; }
__host__ __device__ constexpr unsigned vm_buf_records(int w, int n) {
  return (unsigned)((VM_SOFF_CHECKED ? VM_BUF_SOFF : 0) + VM_BUF_IMM + w * n);
}
static_assert(VM_BUF_SOFF + VM_BUF_IMM + 64 * 16 <= VM_BUF_SOFF + 4 * VM_BUF_WINDOW && VM_BUF_SOFF + 4 * VM_BUF_WINDOW <= 4 * VM_WAVE_DWORDS,
              "every buffer address, clamped or not, is inside the window and the window inside the wave's quarter");

template <int SI>
__device__ __forceinline__ unsigned vm_buf_rounds(const uint32_t* table, uint32_t* slab, int wave, int lane) {
  constexpr int C = ODH_VM_BUF, W = vm_buf_size(SI), RW = W < 4 ? 1 : W / 4;
  const uint32_t region = (uint32_t)VM_WAVE_DWORDS * wave, win = region + VM_BUF_SOFF / 4;
  const uint32_t first = VM_BUF_SOFF + VM_BUF_IMM;  // byte of the region lane 0 accesses
  unsigned bad = 0;
  for (int j = 0; j < VM_BUF_RANGES; ++j) {
    const int n = vm_buf_lanes(j), pass = 2 * (VM_BUF_RANGES * SI + j);
    const __amdgpu_buffer_rsrc_t rs = vm_rsrc(slab + region, vm_buf_records(W, n));
    for (int c = 0; c < VM_BUF_WINDOW / 64; ++c) vm_st_b32(slab + win + 64 * c + lane, vm_stored<C>(table, win + 64 * c + lane, pass));
    vm_wait();
    // the lane's W bytes of the complement
    const uint32_t q = first + (uint32_t)lane * W, dq = region + q / 4;
    u32x4 v = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < RW; ++e) v[e] = vm_stored<C>(table, dq + e, pass + 1);
    if (W < 4) v[0] = v[0] >> 8 * (q & 3) & (W == 1 ? 0xFFu : 0xFFFFu);
    vm_buf_store<W, VM_BUF_IMM>(v, rs, (unsigned)lane * W, VM_BUF_SOFF);
    vm_wait();
    for (int c = 0; c < VM_BUF_WINDOW / 64; ++c) {
      const uint32_t d = VM_BUF_SOFF / 4 + 64 * c + lane;  // dword of the region
      uint32_t landed = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) landed |= (4 * d + b >= first && 4 * d + b < first + (uint32_t)n * W) ? 0xFFu << 8 * b : 0u;
      bad += vm_ld_b32(slab + region + d) != (vm_want<C>(region + d, pass) ^ landed);
    }
    const u32x4 r = vm_buf_load<W, VM_BUF_IMM>(rs, (unsigned)lane * W, VM_BUF_SOFF);
#pragma unroll
    for (int e = 0; e < RW; ++e) {
      uint32_t want = vm_want<C>(dq + e, pass + 1);
      if (W < 4) want = want >> 8 * (q & 3) & (W == 1 ? 0xFFu : 0xFFFFu);
      bad += r[e] != (lane < n ? want : 0u);
    }
  }
  return bad;
}

__global__ __launch_bounds__(256, 1) void vm_buf_kernel(const uint32_t* __restrict__ table, unsigned char* arena,
                                                        int* __restrict__ xcd_blocks, unsigned* __restrict__ err_total,
                                                        unsigned* __restrict__ err_xcd, unsigned* __restrict__ cu_bitmap) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned xcc = lds_book_block(xcd_blocks, cu_bitmap);
  uint32_t* slab = reinterpret_cast<uint32_t*>(arena + (size_t)blockIdx.x * ODH_VM_SLAB);
  unsigned bad = vm_buf_rounds<0>(table, slab, wave, lane);
  bad += vm_buf_rounds<1>(table, slab, wave, lane);
  bad += vm_buf_rounds<2>(table, slab, wave, lane);
  bad += vm_buf_rounds<3>(table, slab, wave, lane);
  bad += vm_buf_rounds<4>(table, slab, wave, lane);
  bad += vm_buf_rounds<5>(table, slab, wave, lane);
  lds_book_errors(bad, xcc, err_total, err_xcd);
}

// ------------------------------------------------------------------ dma
//
// Two passes (a value, its complement) of eight rounds.  Wave v keeps the source in its quarter of the slab (1,024
// dwords, written 16 bytes wide once per pass) and the image in its 16 KiB of LDS, of which the first 8 KiB are
// compared.  A round is a kind (global_load_lds of 4, 12 or 16 bytes; buffer_load_dwordx4 ... lds) and an M0 base (0
// or VM_DMA_M0 into the wave's LDS).  The wave poisons its LDS, issues the load twice, with immediates 0 and
// VM_DMA_IMM, lane l reading at source byte 128 round + immediate + l size, and waits; behind the barrier another
// wave reads all 2,048 dwords with ds_read_b32: source data at M0 base + immediate + l vm_dma_stride(size) +
// [0, size), the poison everywhere else.  The buffer kind ends its range behind lane VM_DMA_LANES - 1: zeros land for the rest.
constexpr int VM_DMA_PASSES = 2, VM_DMA_KINDS = 4, VM_DMA_ROUNDS = 2 * VM_DMA_KINDS;
constexpr int VM_DMA_M0 = 4112, VM_DMA_IMM = 2064, VM_DMA_LANES = 41;  // VM_DMA_IMM: a literal of VM_DMA_PICK_IMM
constexpr int VM_DMA_SRC_DWORDS = 1024, VM_DMA_LDS_WAVE = 16384, VM_DMA_IMAGE_DWORDS = 2048;
__host__ __device__ constexpr int vm_dma_size(int kind) { return kind == 0 ? 4 : kind == 1 ? 12 : 16; }
__host__ __device__ constexpr int vm_dma_stride(int size) { return size == 12 ? 16 : size; }  // bytes of LDS between lanes
__host__ __device__ constexpr uint32_t vm_dma_poison(uint32_t d) { return 0xDEAD0000u | d; }
static_assert(128 * (VM_DMA_ROUNDS - 1) + VM_DMA_IMM + 64 * 16 <= 4 * VM_DMA_SRC_DWORDS, "the source covers every lane's read");
static_assert(VM_DMA_M0 + VM_DMA_IMM + 64 * 16 <= 4 * VM_DMA_IMAGE_DWORDS, "every lane's data lands in the compared image");
// which source byte of the wave's quarter lands at byte a of its LDS image in this round: -1 poison, -2 zeros
__host__ __device__ constexpr int vm_dma_source(int round, uint32_t a) {
  const int kind = round >> 1, size = vm_dma_size(kind), m0 = round & 1 ? VM_DMA_M0 : 0;
  for (int imm = 0; imm <= VM_DMA_IMM; imm += VM_DMA_IMM) {
    const int at = (int)a - m0 - imm, stride = vm_dma_stride(size);
    if (at < 0 || at >= 64 * stride || at % stride >= size) continue;
    if (kind == 3 && at / stride >= VM_DMA_LANES) return -2;
    return 128 * round + imm + at / stride * size + at % stride;
  }
  return -1;
}

template <int KIND>
__device__ __forceinline__ void vm_dma_issue(uint32_t* src, int round, int lane, uint32_t lds_base) {
  constexpr int S = vm_dma_size(KIND);
  const unsigned voff = 128u * round + (unsigned)lane * S;
  if constexpr (KIND < 3) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(src) + voff;
    vm_dma_global<S, 0>(p, lds_base);
    vm_dma_global<S, VM_DMA_IMM>(p, lds_base);
  } else {
    // each load's range ends behind its lane VM_DMA_LANES - 1
    vm_dma_buffer<0>(vm_rsrc(src, 128u * round + 16u * VM_DMA_LANES), voff, 0, lds_base);
    vm_dma_buffer<VM_DMA_IMM>(vm_rsrc(src, 128u * round + VM_DMA_IMM + 16u * VM_DMA_LANES), voff, 0, lds_base);
  }
}

__global__ __launch_bounds__(256, 1) void vm_dma_kernel(const uint32_t* __restrict__ table, unsigned char* arena,
                                                        int* __restrict__ xcd_blocks, unsigned* __restrict__ err_total,
                                                        unsigned* __restrict__ err_xcd, unsigned* __restrict__ cu_bitmap) {
  constexpr int C = ODH_VM_DMA;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned xcc = lds_book_block(xcd_blocks, cu_bitmap);
  uint32_t* slab = reinterpret_cast<uint32_t*>(arena + (size_t)blockIdx.x * ODH_VM_SLAB);
  const uint32_t region = (uint32_t)VM_WAVE_DWORDS * wave;
  ODH_LDS_AS volatile uint32_t* image = (ODH_LDS_AS volatile uint32_t*)lds_smem;  // ds_write_b32, ds_read_b32
  unsigned bad = 0;
  for (int pass = 0; pass < VM_DMA_PASSES; ++pass) {
    for (int c = 0; c < VM_DMA_SRC_DWORDS / 256; ++c) {
      const uint32_t w = region + 256u * c + 4u * lane;
      vm_st_b128(slab + w, u32x4{vm_stored<C>(table, w, pass), vm_stored<C>(table, w + 1, pass),
                                 vm_stored<C>(table, w + 2, pass), vm_stored<C>(table, w + 3, pass)});
    }
    vm_wait();
    for (int round = 0; round < VM_DMA_ROUNDS; ++round) {
      const uint32_t mine = (uint32_t)VM_DMA_LDS_WAVE * wave;
      for (int d = lane; d < VM_DMA_IMAGE_DWORDS; d += 64) image[mine / 4 + d] = vm_dma_poison(d);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const uint32_t base = mine + (round & 1 ? VM_DMA_M0 : 0);
      switch (round >> 1) {
        case 0: vm_dma_issue<0>(slab + region, round, lane, base); break;
        case 1: vm_dma_issue<1>(slab + region, round, lane, base); break;
        case 2: vm_dma_issue<2>(slab + region, round, lane, base); break;
        default: vm_dma_issue<3>(slab + region, round, lane, base); break;
      }
      vm_wait();
      __syncthreads();
      const int from = vm_reads_wave(wave, round);
      for (int d = lane; d < VM_DMA_IMAGE_DWORDS; d += 64) {
        const int s = vm_dma_source(round, 4u * d);
        const uint32_t want = s == -1 ? vm_dma_poison(d) : s == -2 ? 0u : vm_want<C>((uint32_t)VM_WAVE_DWORDS * from + s / 4, pass);
        bad += image[VM_DMA_LDS_WAVE / 4 * from + d] != want;
      }
      __syncthreads();  // the next round's poison overwrites what another wave has just read
    }
  }
  lds_book_errors(bad, xcc, err_total, err_xcd);
}

// ------------------------------------------------------------------ one access
//
// op: ODH_VM_OP_*.  kind 0 / 1: a global load / store, 2 / 3: a buffer load / store, 4 / 5: an LDS-DMA load through a
// global address / a buffer; width in bytes; align: what the instruction asks of the address
struct VmOp {
  int kind, width, align;
};
__host__ __device__ constexpr VmOp vm_op_spec(int op) {
  switch (op) {
    case ODH_VM_OP_LD_U8: case ODH_VM_OP_LD_I8: return {0, 1, 1};
    case ODH_VM_OP_LD_U16: case ODH_VM_OP_LD_I16: case ODH_VM_OP_LD_D16: case ODH_VM_OP_LD_D16_HI: return {0, 2, 2};
    case ODH_VM_OP_LD_B32: case ODH_VM_OP_LD_B32_L2: return {0, 4, 4};
    case ODH_VM_OP_LD_B64: return {0, 8, 4};
    case ODH_VM_OP_LD_B96: return {0, 12, 4};
    case ODH_VM_OP_LD_B128: return {0, 16, 4};
    case ODH_VM_OP_ST_B8: case ODH_VM_OP_ST_B8_D16_HI: return {1, 1, 1};
    case ODH_VM_OP_ST_B16: case ODH_VM_OP_ST_B16_D16_HI: return {1, 2, 2};
    case ODH_VM_OP_ST_B32: return {1, 4, 4};
    case ODH_VM_OP_ST_B64: return {1, 8, 4};
    case ODH_VM_OP_ST_B96: return {1, 12, 4};
    case ODH_VM_OP_ST_B128: return {1, 16, 4};
    case ODH_VM_OP_BUF_LD_B8: return {2, 1, 1};
    case ODH_VM_OP_BUF_LD_B16: return {2, 2, 2};
    case ODH_VM_OP_BUF_LD_B32: return {2, 4, 4};
    case ODH_VM_OP_BUF_LD_B64: return {2, 8, 4};
    case ODH_VM_OP_BUF_LD_B96: return {2, 12, 4};
    case ODH_VM_OP_BUF_LD_B128: return {2, 16, 4};
    case ODH_VM_OP_BUF_ST_B8: return {3, 1, 1};
    case ODH_VM_OP_BUF_ST_B16: return {3, 2, 2};
    case ODH_VM_OP_BUF_ST_B32: return {3, 4, 4};
    case ODH_VM_OP_BUF_ST_B64: return {3, 8, 4};
    case ODH_VM_OP_BUF_ST_B96: return {3, 12, 4};
    case ODH_VM_OP_BUF_ST_B128: return {3, 16, 4};
    case ODH_VM_OP_DMA_B32: return {4, 4, 4};
    case ODH_VM_OP_DMA_B96: return {4, 12, 4};
    case ODH_VM_OP_DMA_B128: return {4, 16, 4};
    case ODH_VM_OP_DMA_BUF_B128: return {5, 16, 4};
    default: return {-1, 0, 0};
  }
}

template <int IMM>
__device__ __forceinline__ u32x4 vm_access_imm(int op, unsigned char* image, unsigned off, u32x4 v, __amdgpu_buffer_rsrc_t rs,
                                               unsigned soff, uint32_t lds_base) {
  switch (op) {
    case ODH_VM_OP_BUF_LD_B8: return vm_buf_load<1, IMM>(rs, off, soff);
    case ODH_VM_OP_BUF_LD_B16: return vm_buf_load<2, IMM>(rs, off, soff);
    case ODH_VM_OP_BUF_LD_B32: return vm_buf_load<4, IMM>(rs, off, soff);
    case ODH_VM_OP_BUF_LD_B64: return vm_buf_load<8, IMM>(rs, off, soff);
    case ODH_VM_OP_BUF_LD_B96: return vm_buf_load<12, IMM>(rs, off, soff);
    case ODH_VM_OP_BUF_LD_B128: return vm_buf_load<16, IMM>(rs, off, soff);
    case ODH_VM_OP_BUF_ST_B8: vm_buf_store<1, IMM>(v, rs, off, soff); break;
    case ODH_VM_OP_BUF_ST_B16: vm_buf_store<2, IMM>(v, rs, off, soff); break;
    case ODH_VM_OP_BUF_ST_B32: vm_buf_store<4, IMM>(v, rs, off, soff); break;
    case ODH_VM_OP_BUF_ST_B64: vm_buf_store<8, IMM>(v, rs, off, soff); break;
    case ODH_VM_OP_BUF_ST_B96: vm_buf_store<12, IMM>(v, rs, off, soff); break;
    case ODH_VM_OP_BUF_ST_B128: vm_buf_store<16, IMM>(v, rs, off, soff); break;
    case ODH_VM_OP_DMA_B32: vm_dma_global<4, IMM>(image + off, lds_base); break;
    case ODH_VM_OP_DMA_B96: vm_dma_global<12, IMM>(image + off, lds_base); break;
    case ODH_VM_OP_DMA_B128: vm_dma_global<16, IMM>(image + off, lds_base); break;
    default: vm_dma_buffer<IMM>(rs, off, soff, lds_base); break;  // ODH_VM_OP_DMA_BUF_B128
  }
  return u32x4{0, 0, 0, 0};
}

// one wave, one access per lane: lane l at image + off.a[l] (buffer kinds: vector offset off.a[l] of a descriptor
// whose base is image).  Loads give out[l] (a half-register load starts from data[l][0]); stores take data[l]; an
// LDS-DMA load runs over LDS poisoned with 0xEE bytes and out[l] is the 16 bytes at lds_base + imm + l * vm_dma_stride(width)
__global__ __launch_bounds__(64) void vm_access_kernel(int op, unsigned char* image, LdsLaneAddr off, const u32x4* __restrict__ data,
                                                       unsigned num_records, unsigned soff, int imm, uint32_t lds_base,
                                                       u32x4* __restrict__ out) {
  const int lane = threadIdx.x;
  const VmOp s = vm_op_spec(op);
  const u32x4 v = data[lane];
  unsigned char* p = image + off.a[lane];
  u32x4 o = {0, 0, 0, 0};
  if (s.kind >= 4) {
    for (int d = lane; d < 65536 / 4; d += 64) ((ODH_LDS_AS volatile uint32_t*)lds_smem)[d] = 0xEEEEEEEEu;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  switch (op) {
    case ODH_VM_OP_LD_U8: o[0] = vm_ld_u8(p); break;
    case ODH_VM_OP_LD_I8: o[0] = vm_ld_i8(p); break;
    case ODH_VM_OP_LD_U16: o[0] = vm_ld_u16(p); break;
    case ODH_VM_OP_LD_I16: o[0] = vm_ld_i16(p); break;
    case ODH_VM_OP_LD_D16: o[0] = vm_ld_d16(p, v[0]); break;
    case ODH_VM_OP_LD_D16_HI: o[0] = vm_ld_d16_hi(p, v[0]); break;
    case ODH_VM_OP_LD_B32: o[0] = vm_ld_b32(p); break;
    case ODH_VM_OP_LD_B32_L2: o[0] = vm_ld_b32_l2(p); break;
    case ODH_VM_OP_LD_B64: { const vm_u32x2 r = vm_ld_b64(p); o[0] = r[0], o[1] = r[1]; break; }
    case ODH_VM_OP_LD_B96: { const vm_u32x3 r = vm_ld_b96(p); o[0] = r[0], o[1] = r[1], o[2] = r[2]; break; }
    case ODH_VM_OP_LD_B128: o = vm_ld_b128(p); break;
    case ODH_VM_OP_ST_B8: vm_st_b8(p, v[0]); break;
    case ODH_VM_OP_ST_B16: vm_st_b16(p, v[0]); break;
    case ODH_VM_OP_ST_B8_D16_HI: vm_st_b8_hi(p, v[0]); break;
    case ODH_VM_OP_ST_B16_D16_HI: vm_st_b16_hi(p, v[0]); break;
    case ODH_VM_OP_ST_B32: vm_st_b32(p, v[0]); break;
    case ODH_VM_OP_ST_B64: vm_st_b64(p, vm_u32x2{v[0], v[1]}); break;
    case ODH_VM_OP_ST_B96: vm_st_b96(p, vm_u32x3{v[0], v[1], v[2]}); break;
    case ODH_VM_OP_ST_B128: vm_st_b128(p, v); break;
    default: {
      const __amdgpu_buffer_rsrc_t rs = vm_rsrc(image, num_records);
      o = imm ? vm_access_imm<ODH_VM_ACCESS_IMM>(op, image, off.a[lane], v, rs, soff, lds_base)
              : vm_access_imm<0>(op, image, off.a[lane], v, rs, soff, lds_base);
    }
  }
  vm_wait();
  if (s.kind >= 4) {
    __syncthreads();
    ODH_LDS_AS const volatile uint32_t* at = (ODH_LDS_AS const volatile uint32_t*)(lds_smem + lds_base + imm + lane * vm_dma_stride(s.width));
    for (int e = 0; e < 4; ++e) o[e] = at[e];
  }
  out[lane] = o;
}

// ------------------------------------------------------------------ host side

// compared elements of one workgroup that use key dword k (k < 0: all that use a key)
unsigned long long vm_block_cases(int check, int k) {
  unsigned long long n = 0;
  auto hit = [&](uint32_t w, int pass) { return (unsigned long long)(k < 0 || (int)vm_kidx(w, pass) == k); };
  if (check == ODH_VM_CACHE) {
    for (int pass = 0; pass < VM_CACHE_PASSES; ++pass)
      for (uint32_t w = 0; w < ODH_VM_SLAB / 4; ++w) n += VM_CACHE_READS * hit(w, pass);
  } else if (check == ODH_VM_SUB) {
    for (int pass = 0; pass < VM_SUB_A_PASSES; ++pass)
      for (uint32_t w = 0; w < VM_SUB_A_DWORDS; ++w) n += hit(VM_SUB_A + w, pass);
    for (int pass = 0; pass < VM_SUB_PASSES; ++pass) {
      for (uint32_t w = 0; w < VM_SUB_B_DWORDS; ++w) n += VM_SUB_B_LOADS * hit(VM_SUB_B + w, pass);
      for (int wave = 0; wave < 4; ++wave)
        for (uint32_t w = VM_SUB_C_W2; w < VM_SUB_C_W4 + 4 * 64; ++w) n += hit(VM_SUB_C + VM_SUB_C_WAVE * wave + w, pass);
    }
  } else if (check == ODH_VM_BUF) {
    for (int wave = 0; wave < 4; ++wave)
      for (int si = 0; si < VM_BUF_SIZES; ++si)
        for (int j = 0; j < VM_BUF_RANGES; ++j) {
          const int pass = 2 * (VM_BUF_RANGES * si + j), w = vm_buf_size(si), rw = w < 4 ? 1 : w / 4;
          const uint32_t region = (uint32_t)VM_WAVE_DWORDS * wave;
          for (uint32_t d = 0; d < VM_BUF_WINDOW; ++d) n += hit(region + VM_BUF_SOFF / 4 + d, pass);
          for (int lane = 0; lane < vm_buf_lanes(j); ++lane)
            for (int e = 0; e < rw; ++e) n += hit(region + (VM_BUF_SOFF + VM_BUF_IMM + lane * w) / 4 + e, pass);
        }
  } else if (check == ODH_VM_DMA) {
    for (int pass = 0; pass < VM_DMA_PASSES; ++pass)
      for (int wave = 0; wave < 4; ++wave)
        for (int round = 0; round < VM_DMA_ROUNDS; ++round)
          for (uint32_t d = 0; d < VM_DMA_IMAGE_DWORDS; ++d) {
            const int s = vm_dma_source(round, 4 * d);
            if (s >= 0) n += hit((uint32_t)VM_WAVE_DWORDS * wave + s / 4, pass);
          }
  }
  return n;
}

template <typename... Args>
void vm_launch_probe(int check, hipStream_t stream, Args... args) {
  switch (check) {
    case ODH_VM_CACHE: vm_cache_kernel<<<ODH_VM_BLOCKS, 256, VM_LDS_BYTES, stream>>>(args...); break;
    case ODH_VM_SUB: vm_sub_kernel<<<ODH_VM_BLOCKS, 256, VM_LDS_BYTES, stream>>>(args...); break;
    case ODH_VM_BUF: vm_buf_kernel<<<ODH_VM_BLOCKS, 256, VM_LDS_BYTES, stream>>>(args...); break;
    default: vm_dma_kernel<<<ODH_VM_BLOCKS, 256, VM_LDS_BYTES, stream>>>(args...); break;
  }
}
