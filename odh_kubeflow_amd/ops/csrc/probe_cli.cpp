// MI355X start-up probe as a stand-alone program: the notebook pod's init container.
//
// `odh-gpu-probe` (probe_main.cpp) and `python -m odh_kubeflow_amd.ops.probe_main` both call
// odh_probe_cli().  It needs only the HIP runtime — no Python, no torch — so the init
// container costs process start + HIP init + ~0.2 ms of GPU work, not the ~1.6 s of an
// `import torch`.  For every GPU the device plugin made visible to the pod it:
//
//   1. allocates the probe operands and a 256 MiB HBM3E buffer with hipMalloc and fills the
//      integer-valued bf16 operands on the GPU (odh_probe_fill);
//   2. runs the MFMA bf16 GEMM with the check fused into its epilogue
//      (odh_probe_gemm_verify: every output element compared in registers against a closed
//      form, mismatches attributed to the XCD that computed them), then the HBM pattern
//      write + verify sweep, both on the device's null stream (--streams 0, the default;
//      --streams 2 overlaps the sweep with the GEMM on a second stream);
//   3. with 2+ GPUs, reads every link of a ring over them through xGMI (peer access) and
//      verifies the neighbour's pattern word for word;
//   4. with --rccl-mib N (the `amd.com/gpu-probe: "rccl"` notebooks), an RCCL all-reduce over
//      all of them in this one process (ncclCommInitAll; librccl is dlopen'ed only then — it
//      is 570 MB), every element of every device's result checked on its GPU: the
//      collective library and its xGMI transport ready for the notebook's torch.distributed;
//   5. with --mx fp8,fp4 (the `amd.com/gpu-probe: "mx"` notebooks), after the HBM sweep and on
//      its stream, per format: the probe operands re-encoded as FP8 / MXFP4 codes with E8M0
//      block scales into the bf16 operands' buffers (odh_mx_fill), then the block-scaled GEMM
//      (v_mfma_scale_f32_32x32x64_f8f6f4) checked in registers against a 15 × 21 table
//      (odh_mx_probe_gemm_verify): the data path a quantised model runs on.  The list may name
//      any of the instruction's five operand formats, fp8,fp4,bf8,fp6,bf6 (the "mxall" notebooks):
//      BF8 is the gradient format of FP8 training, FP6 and BF6 the MXFP6 formats, whose 6-bit
//      decode and 96-byte stage rows no other check touches;
//   6. with --dtypes f16,i8 (the `amd.com/gpu-probe: "dtypes"` notebooks), after the HBM sweep, on
//      its stream and before step 5, per format: the probe operands re-encoded as halves or as
//      int8 (odh_dense_fill) into the bf16 operands' buffers, then the FP16
//      (v_mfma_f32_32x32x16_f16) or INT8 (v_mfma_i32_32x32x32_i8) GEMM checked in registers against
//      the closed form (odh_dense_probe_gemm_verify): autocast's default dtype and the W8A8 path;
//   7. with --fp f32,f64 (the `amd.com/gpu-probe: "fp"` notebooks), after step 6 and before step 5,
//      per format: the probe operands times odd constants as floats or doubles (odh_fp_fill) into
//      the operands' buffers, which are then sized for them, and the FP32 (v_mfma_f32_32x32x2_f32)
//      or FP64 (v_mfma_f64_16x16x4_f64) GEMM checked in registers against the closed form
//      (odh_fp_probe_gemm_verify): torch's default dtype and NumPy's;
//   8. with --sparse bf16,f16,i8,fp8,bf8 (the `amd.com/gpu-probe: "sparse"` notebooks), after step 7 and
//      before step 5, per format: the probe's A pruned 2:4 and compressed, its metadata and the dense Bt
//      (odh_sparse_fill) into the operands' buffers, and the structured-sparsity GEMM (v_smfmac_*) checked
//      in registers against a 30 × 7 table (odh_sparse_probe_gemm_verify): the index operand and the
//      selection multiplexers a pruned model runs on, which no dense instruction touches;
//   9. with --cvt fp8,bf8,fp4,fp6,bf6,bf16 (the `amd.com/gpu-probe: "cvt"` notebooks), after step 5, per format: the
//      hardware converters that make those codes at run time (v_cvt_scalef32_pk_fp8_f32 and its kin,
//      v_cvt_pk_bf16_f32), every rounding case of every code at every scale on every SIMD, compared in
//      registers with codes known by construction (odh_cvt_probe_verify): no operand buffer, a 256-byte scale
//      table (odh_cvt_fill) and a counter block per format;
//  10. with --lds mem,tr16,tr8,tr4,tr6,xlane (the `amd.com/gpu-probe: "lds"` notebooks), after step 9, per check: every
//      dword of every CU's 160 KiB of LDS, the transposing LDS reads (ds_read_b64_tr_b16 / _b8 / _b4,
//      ds_read_b96_tr_b6) and the lane exchanges (ds_bpermute, ds_swizzle, DPP, v_readlane, v_permlane32_swap and
//      their kin), one workgroup per CU and one wave per SIMD, compared in registers with closed forms
//      (odh_lds_probe_verify): no operand buffer, a 1 KiB key table (odh_lds_fill) and a counter block per check.
//      Its verdict is one entry for the whole step: "lds":{"ok","errors","ms","bad"}.
//  11. with --mfma16 bf16,f16,i8,fp8,fp4 (the `amd.com/gpu-probe: "mfma16"` notebooks), after step 10, per format: the
//      probe operands in that format's layout (odh_probe_fill, odh_dense_fill or odh_mx_fill, into the bf16 operands'
//      buffers) and the GEMM again on the 16×16 shape of its matrix-core instruction (v_mfma_f32_16x16x32_bf16 / _f16,
//      v_mfma_i32_16x16x64_i8, v_mfma_scale_f32_16x16x128_f8f6f4), checked in registers against the same closed form
//      or table (odh_m16_probe_gemm_verify): the shape torch.compile's templates, Triton and CK's small tiles issue,
//      whose operand, scale and C/D maps are not the 32×32 ones.  One entry for the whole step, as --lds:
//      "mfma16":{"ok","errors","ms","bad"}.
//
// All devices are launched before any is waited on.  The result is one compact JSON object
// (<4 KiB: the kubelet's termination-message limit) written to --json (default
// /dev/termination-log when it exists) and printed on stdout.  Exit status: 0 healthy,
// 1 a check failed, 2 no GPU or a HIP error, 3 the --timeout-ms watchdog fired, 64 usage.
//
// Reference parallel: the upstream pod has no GPU gate at all — kf generateStatefulSet
// (kf/controllers/notebook_controller.go:433-523) copies resources.limits verbatim and the
// pod is Ready when Jupyter answers; this program is what `amd.com/gpu-probe: "true"` adds
// in front of the notebook container (controllers/notebook.py::_gpu_probe_init_container).

#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: the library is dlopen'ed (rccl_allreduce)

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <memory>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

#include "gpu_probe.h"

namespace {

using Clock = std::chrono::steady_clock;

double ms_since(Clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

struct Dev;
struct Options;

// what one asked-for format of an optional GEMM step keeps on one device
struct Slot {
  int* counters = nullptr;  // its counter block on the device
  int host[ODH_NCOUNT] = {};
  hipEvent_t e0 = nullptr, e1 = nullptr;
  float ms = 0;
};

// An optional step (--mx, --dtypes, --fp, --sparse: per asked-for format, the probe operands re-encoded into
// the bf16 operands' buffers and a fused check of that format's matrix-core instruction; --cvt: per format, the
// fused check of its converter).
struct Step {
  const char* word;  // the option (--word), the --inject-fault word and the verdict key
  const char* what;  // in the error string: "<N> <what> mismatches"
  std::vector<std::pair<const char*, int>> formats;  // name <-> code
  // one format on one device, on the sweep's stream: fill, the fault if asked for, event, fused
  // verify, event, the counters copied back
  bool (*run)(Dev&, const Options&, int fmt, Slot&);
  int (*tiles)(int fmt, int M, int N) = nullptr;  // workgroups of a format's kernel; null: the bf16 GEMM's
  double (*work)(int fmt) = nullptr;  // operations of a format's kernel; null: the GEMM's 2 M N K, reported as tflops
  const char* rate = "tflops";        // the verdict key of the rate: with work, operations per nanosecond
  bool host_ms = true;                // whether a format's entry ends with its host time
  bool flat = false;                  // one entry for the whole step instead of one per format (--lds)
  std::vector<int> asked = {};  // the formats to check, in the order given

  const char* name(int fmt) const {
    for (const auto& nf : formats)
      if (nf.second == fmt) return nf.first;
    return "?";
  }
  // a comma list of formats, each at most once
  bool ask(const std::string& v) {
    for (size_t at = 0; at <= v.size();) {
      const size_t comma = std::min(v.find(',', at), v.size());
      const std::string name = v.substr(at, comma - at);
      int fmt = -1;
      for (const auto& nf : formats)
        if (name == nf.first) fmt = nf.second;
      if (fmt < 0 || std::find(asked.begin(), asked.end(), fmt) != asked.end()) return false;
      asked.push_back(fmt);
      at = comma + 1;
    }
    return true;
  }
};

bool mx_run(Dev& d, const Options& o, int fmt, Slot& s);
bool dt_run(Dev& d, const Options& o, int fmt, Slot& s);
bool fp_run(Dev& d, const Options& o, int fmt, Slot& s);
bool sp_run(Dev& d, const Options& o, int fmt, Slot& s);
bool cvt_run(Dev& d, const Options& o, int fmt, Slot& s);
bool lds_run(Dev& d, const Options& o, int check, Slot& s);
bool m16_run(Dev& d, const Options& o, int fmt, Slot& s);
int lds_blocks(int, int, int) { return ODH_LDS_BLOCKS; }
int cvt_blocks(int, int, int) { return ODH_CVT_BLOCKS; }
// conversions of the fused check: four waves in each of its workgroups convert the whole family
double cvt_work(int fmt) { return (double)odh_cvt_family_size(fmt) * ODH_CVT_BLOCKS * 4; }

// the steps in the verdict's order, which is also the order of their counter blocks and events;
// they run --dtypes, --fp, --sparse, --mx, --cvt, --lds, --mfma16
enum { STEP_MX, STEP_DTYPES, STEP_FP, STEP_SPARSE, STEP_CVT, STEP_LDS, STEP_MFMA16, N_STEPS };

struct Options {
  int M = 4096, N = 4096, K = 1024;
  size_t hbm_bytes = 256ull << 20;
  size_t xgmi_bytes = 64ull << 20;
  size_t rccl_bytes = 0;  // 0: no RCCL step
  long timeout_ms = 30000;
  std::string json_path;  // "" = default; "-" = stdout only
  std::string fault;      // test hook: gemm | hbm | xgmi | rccl | a step's word
  Step steps[N_STEPS] = {
      {"mx", "MX GEMM",
       {{"fp8", ODH_MX_FP8}, {"fp4", ODH_MX_FP4}, {"bf8", ODH_MX_BF8}, {"fp6", ODH_MX_FP6}, {"bf6", ODH_MX_BF6}},
       mx_run},
      {"dtypes", "GEMM", {{"f16", ODH_DT_F16}, {"i8", ODH_DT_I8}}, dt_run},  // tflops counts integer operations for i8
      {"fp", "GEMM", {{"f32", ODH_FP_F32}, {"f64", ODH_FP_F64}}, fp_run, odh_fp_tiles},
      {"sparse", "sparse GEMM",  // tflops counts the dense-equivalent 2 M N K
       {{"bf16", ODH_SP_BF16}, {"f16", ODH_SP_F16}, {"i8", ODH_SP_I8}, {"fp8", ODH_SP_FP8}, {"bf8", ODH_SP_BF8}},
       sp_run},
      {"cvt", "conversion",  // gcvt_s: family cases per nanosecond over all waves
       {{"fp8", ODH_CVT_FP8}, {"bf8", ODH_CVT_BF8}, {"fp4", ODH_CVT_FP4}, {"fp6", ODH_CVT_FP6}, {"bf6", ODH_CVT_BF6},
        {"bf16", ODH_CVT_BF16}},
       // no host_ms: with it the verdict of 8 healthy GPUs and every step is 3914 bytes at the widest, which one
       // failing check's error string takes to the kubelet's 4096; its entries are 17 bytes shorter each
       cvt_run, cvt_blocks, cvt_work, "gcvt_s", false},
      {"lds", "LDS",
       {{"mem", ODH_LDS_MEM}, {"tr16", ODH_LDS_TR16}, {"tr8", ODH_LDS_TR8}, {"tr4", ODH_LDS_TR4}, {"tr6", ODH_LDS_TR6},
        {"xlane", ODH_LDS_XLANE}},
       // flat: six more entries would not fit the kubelet's 4096 bytes next to every other step on 8 GPUs
       lds_run, lds_blocks, nullptr, "", false, true},
      {"mfma16", "16x16 GEMM",
       {{"bf16", ODH_M16_BF16}, {"f16", ODH_M16_F16}, {"i8", ODH_M16_I8}, {"fp8", ODH_M16_FP8}, {"fp4", ODH_M16_FP4}},
       // flat, as --lds: the verdict of 8 healthy GPUs with every step was 3875 bytes at its widest; the entry
       // ,"mfma16":{"ok":true,"errors":0,"ms":99.999,"bad":""} is 53 and "mfma16":99.999, in timings_ms 16, so 3944,
       // below 4096 - 120 = 3976.  A failing step adds "false" for "true" (1), a count of up to 10 digits (9) and a
       // bad list of at most 19 bytes, and the verdict one error string of up to 120: 4093, which still fits
       m16_run, nullptr, nullptr, "", false, true},
  };
  bool quiet = false;
  // streams created per device: 0 = the device's null stream (nothing created; the default),
  // 1 = one stream, 2 = the HBM sweep overlapping the GEMM on a second stream.  Each stream is
  // a hardware queue: on the MI355X one costs 10-15 ms to create (2 streams: 27-31 ms of
  // set-up, 1: 22 ms; the null stream's queue, made at its first launch, 17.5 ms), while
  // overlapping the sweep saves 0.005 ms of GPU time and halves both measured rates (pass r6_g9)
  int streams = 0;
};

// device counters: the counter block of gpu_probe.h in its CLI layout
struct Dev {
  int index = 0;
  void* block = nullptr;  // the one allocation every buffer below is carved from
  void *a = nullptr, *bt = nullptr, *hbm = nullptr;
  int* tile_xcd = nullptr;
  int* counters = nullptr;
  int host[ODH_NCOUNT] = {};
  hipStream_t sg = nullptr, sh = nullptr;
  hipEvent_t e0 = nullptr, e_gemm = nullptr, e_h0 = nullptr, e_h1 = nullptr, e_link0 = nullptr, e_link1 = nullptr;
  hipEvent_t e_r0 = nullptr, e_r1 = nullptr;
  uint32_t seed = 0;
  float gemm_ms = 0, hbm_ms = 0, link_ms = 0, rccl_ms = 0;
  double malloc_ms = 0, streams_ms = 0, events_ms = 0, first_op_ms = 0;  // host-side set-up, step by step
  int link_source = -1;
  // --mx, and fp8 or fp4 of --mfma16: scales and table behind the counters
  void *mx_sa = nullptr, *mx_sbt = nullptr;
  float* mx_table = nullptr;
  // --sparse: metadata and table behind those
  void* sp_meta = nullptr;
  int* sp_table = nullptr;
  // --cvt: the scale table behind those
  void* cvt_table = nullptr;
  // --lds: its key table behind that, and its counter blocks (each with the CU bitmap) behind the table
  void* lds_table = nullptr;
  std::vector<Slot> slots[N_STEPS];  // per step, one per asked-for format: counter blocks behind the first
  std::string error;
};

int usage(const char* argv0) {
  std::fprintf(stderr,
               "usage: %s [--json PATH|-] [--shape M,N,K] [--hbm-mib N] [--xgmi-mib N] [--rccl-mib N] "
               "[--mx fp8,fp4[,bf8,fp6,bf6]] [--dtypes f16,i8] [--fp f32,f64] [--sparse bf16,f16,i8,fp8,bf8] "
               "[--cvt fp8,bf8,fp4,fp6,bf6,bf16] [--lds mem,tr16,tr8,tr4,tr6,xlane] "
               "[--timeout-ms N] [--streams 0|1|2] [--inject-fault gemm|hbm|xgmi|rccl|mx|dtypes|fp] "
               "[--inject-fault sparse] [--inject-fault cvt] [--inject-fault lds] [--quiet] "
               "[--mfma16 bf16,f16,i8,fp8,fp4] [--inject-fault mfma16]\n",
               argv0);
  return 64;
}

// the largest K at which every partial sum of the --fp operands, at most 6 K MUL_A MUL_B, is an
// exact integer of the accumulator type: below 2^24 (f32) or 2^53 (f64)
long long fp_max_k(int fmt) {
  return fmt == ODH_FP_F64 ? ((1LL << 53) - 1) / (6LL * ODH_FP_F64_MUL_A * ODH_FP_F64_MUL_B)
                           : ((1LL << 24) - 1) / (6LL * ODH_FP_F32_MUL_A * ODH_FP_F32_MUL_B);
}

bool parse(int argc, char** argv, Options& o) {
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    std::string v;
    const size_t eq = a.find('=');
    if (eq != std::string::npos) {
      v = a.substr(eq + 1);
      a = a.substr(0, eq);
    } else if (a != "--quiet") {
      if (i + 1 >= argc) return false;
      v = argv[++i];
    }
    if (a == "--json") {
      o.json_path = v;
    } else if (a == "--shape") {
      if (std::sscanf(v.c_str(), "%d,%d,%d", &o.M, &o.N, &o.K) != 3) return false;
    } else if (a == "--hbm-mib") {
      o.hbm_bytes = (size_t)std::strtoull(v.c_str(), nullptr, 10) << 20;
    } else if (a == "--xgmi-mib") {
      o.xgmi_bytes = (size_t)std::strtoull(v.c_str(), nullptr, 10) << 20;
    } else if (a == "--rccl-mib") {
      o.rccl_bytes = (size_t)std::strtoull(v.c_str(), nullptr, 10) << 20;
    } else if (a == "--timeout-ms") {
      o.timeout_ms = std::strtol(v.c_str(), nullptr, 10);
    } else if (a == "--streams") {
      o.streams = (int)std::strtol(v.c_str(), nullptr, 10);
      if (o.streams < 0 || o.streams > 2) return false;
    } else if (a == "--inject-fault") {
      o.fault = v;
      bool known = v == "gemm" || v == "hbm" || v == "xgmi" || v == "rccl";
      for (const Step& s : o.steps) known = known || v == s.word;
      if (!known) return false;
    } else if (a == "--quiet") {
      o.quiet = true;
    } else {
      Step* step = nullptr;
      for (Step& s : o.steps)
        if (a == std::string("--") + s.word) step = &s;
      if (!step || !step->ask(v)) return false;
    }
  }
  // the fused check needs 256² output tiles and K in 64-element steps
  // the probe operands sum to zero over their period of 35 in k: at K % 35 == 0 the expected
  // product is 0 everywhere and matrix cores that return zeros would pass, so K is refused
  // the all-reduce's send and receive buffers are the two halves of the HBM buffer
  // --mx: one K for every format (128 = one FP4, FP6 or BF6 stage), and none of the 315 classes of the MX
  // operands may expect 0 at it (odh_mx_zero_classes: host arithmetic, before any HIP call)
  if (!o.steps[STEP_MX].asked.empty() && (o.K % 128 != 0 || odh_mx_zero_classes(o.K) != 0)) return false;
  // --dtypes: the operands are the bf16 probe's (times constants for i8), so the K rules below
  // cover it: K % 64 == 0 is a whole number of f16 and of i8 stages, K % 35 != 0 a non-zero product
  // --fp: the same operands times constants, floats or doubles: K % 64 == 0 is a whole number of their
  // stages too, and every partial sum must stay an exact integer of the accumulator type
  for (int fmt : o.steps[STEP_FP].asked)
    if (o.K > fp_max_k(fmt)) return false;
  // --sparse: 64 is a stage of its 16-bit formats, 128 of its 8-bit ones, and none of the 210 classes of the
  // pruned operands may expect 0 (odh_sparse_zero_classes: host arithmetic, before any HIP call)
  if (!o.steps[STEP_SPARSE].asked.empty() && odh_sparse_zero_classes(o.K) != 0) return false;
  for (int fmt : o.steps[STEP_SPARSE].asked)
    if (fmt != ODH_SP_BF16 && fmt != ODH_SP_F16 && o.K % 128 != 0) return false;
  // --mfma16: K % 64 == 0 below is a whole number of bf16, f16 and i8 instructions; fp8 and fp4 take 128 elements
  // per instruction and check against the MX table, in which no class may expect 0
  for (int fmt : o.steps[STEP_MFMA16].asked)
    if ((fmt == ODH_M16_FP8 || fmt == ODH_M16_FP4) && (o.K % 128 != 0 || odh_mx_zero_classes(o.K) != 0)) return false;
  // a step's fault needs the step
  for (const Step& s : o.steps)
    if (o.fault == s.word && s.asked.empty()) return false;
  return o.M > 0 && o.N > 0 && o.K > 0 && o.M % 256 == 0 && o.N % 256 == 0 && o.K % 64 == 0 && o.K % 35 != 0 &&
         o.hbm_bytes >= (1u << 20) && o.timeout_ms > 0 && 2 * o.rccl_bytes <= o.hbm_bytes &&
         (o.fault != "rccl" || o.rccl_bytes > 0);
}

// bytes of an element of the A and Bt carve-outs: bf16's 2, or the widest --fp format's (its codes
// are the element sizes)
size_t operand_esize(const Options& o) {
  size_t e = 2;
  for (int fmt : o.steps[STEP_FP].asked) e = std::max(e, (size_t)fmt);
  return e;
}

void emit(const Options& o, const std::string& json) {
  std::string path = o.json_path;
  if (path.empty()) path = access("/dev/termination-log", W_OK) == 0 ? "/dev/termination-log" : "-";
  if (path != "-") {
    if (FILE* f = std::fopen(path.c_str(), "w")) {
      std::fwrite(json.data(), 1, json.size(), f);
      std::fclose(f);
    }
  }
  if (!o.quiet || path == "-") {
    std::fwrite(json.data(), 1, json.size(), stdout);
    std::fputc('\n', stdout);
    std::fflush(stdout);
  }
}

std::string esc(const std::string& s) {
  std::string out;
  for (char c : s) {
    if (c == '"' || c == '\\') {
      out += '\\';
      out += c;
    } else if ((unsigned char)c < 0x20) {
      out += ' ';
    } else {
      out += c;
    }
  }
  return out;
}

std::string fail_json(const char* what, const std::string& msg, double total_ms) {
  char buf[512];
  std::snprintf(buf, sizeof buf, "{\"ok\":false,\"error\":\"%s: %s\",\"timings_ms\":{\"total\":%.3f}}", what,
                esc(msg).c_str(), total_ms);
  return buf;
}

#define HIP_TRY(expr)                                   \
  do {                                                  \
    const int rc_ = (int)(expr);                        \
    if (rc_ != 0) {                                     \
      d.error = std::string(#expr) + ": " + hipGetErrorString((hipError_t)rc_); \
      return false;                                     \
    }                                                   \
  } while (0)

size_t align_up(size_t x) { return (x + 4095) & ~(size_t)4095; }

// One hipMalloc per device for the operands, the HBM sweep buffer, the tile map and the
// counters (each 4 KiB aligned): a single mapping of the device's memory instead of five,
// then the streams and events.  Host-side set-up time is what the notebook pod waits for.
bool setup_alloc(Dev& d, const Options& o) {
  HIP_TRY(hipSetDevice(d.index));
  const size_t esz = operand_esize(o);
  const size_t na = align_up((size_t)o.M * o.K * esz), nb = align_up((size_t)o.N * o.K * esz);
  const size_t nh = align_up(o.hbm_bytes), nt = align_up(sizeof(int) * (size_t)(o.M / 128) * (o.N / 128));
  auto t0 = Clock::now();
  // every optional step adds a counter block per format behind the first; --mx also the scales of both
  // operands and the table, --dtypes nothing else: its operands are no larger; --fp widens the operands;
  // --sparse adds the metadata and its table (compressed A and Bt are no larger than the bf16 operands);
  // --cvt adds its scale table; --lds its key table and counter blocks of its own size, with the CU bitmap;
  // --mfma16 a counter block per format like the GEMM steps and, for fp8 or fp4, the scales and table of --mx
  size_t nslots = 0;
  for (int s = 0; s < N_STEPS; ++s)
    if (s != STEP_LDS) nslots += o.steps[s].asked.size();
  const size_t nlds_asked = o.steps[STEP_LDS].asked.size();
  const size_t lds_block = sizeof(int) * (ODH_NCOUNT + ODH_LDS_CU_WORDS);
  const size_t nldstab = nlds_asked ? align_up(ODH_LDS_TABLE) : 0, nldsc = nlds_asked ? align_up(lds_block * nlds_asked) : 0;
  size_t nmx = o.steps[STEP_MX].asked.size();  // then: whether any step needs the MX scales and table
  for (int fmt : o.steps[STEP_MFMA16].asked) nmx += fmt == ODH_M16_FP8 || fmt == ODH_M16_FP4;
  const size_t nc = align_up(sizeof(int) * ODH_NCOUNT * (1 + nslots));
  const size_t nsa = nmx ? align_up((size_t)o.M * (o.K / 32)) : 0, nsb = nmx ? align_up((size_t)o.N * (o.K / 32)) : 0;
  const size_t ntab = nmx ? align_up(sizeof(float) * ODH_MX_CLASSES) : 0;
  const bool sparse = !o.steps[STEP_SPARSE].asked.empty();
  const size_t nmeta = sparse ? align_up((size_t)o.M * (o.K / 8)) : 0;
  const size_t nsptab = sparse ? align_up(sizeof(int) * ODH_SP_CLASSES) : 0;
  const size_t ncvt = o.steps[STEP_CVT].asked.empty() ? 0 : align_up(ODH_CVT_TABLE);
  HIP_TRY(hipMalloc(&d.block, na + nb + nh + nt + nc + nsa + nsb + ntab + nmeta + nsptab + ncvt + nldstab + nldsc));
  d.malloc_ms = ms_since(t0);
  char* p = (char*)d.block;
  d.a = p;
  d.bt = p + na;
  d.hbm = p + na + nb;
  d.tile_xcd = (int*)(p + na + nb + nh);
  d.counters = (int*)(p + na + nb + nh + nt);
  if (nmx) {
    d.mx_sa = p + na + nb + nh + nt + nc;
    d.mx_sbt = p + na + nb + nh + nt + nc + nsa;
    d.mx_table = (float*)(p + na + nb + nh + nt + nc + nsa + nsb);
  }
  if (sparse) {
    d.sp_meta = p + na + nb + nh + nt + nc + nsa + nsb + ntab;
    d.sp_table = (int*)(p + na + nb + nh + nt + nc + nsa + nsb + ntab + nmeta);
  }
  if (ncvt) d.cvt_table = p + na + nb + nh + nt + nc + nsa + nsb + ntab + nmeta + nsptab;
  if (nlds_asked) d.lds_table = p + na + nb + nh + nt + nc + nsa + nsb + ntab + nmeta + nsptab + ncvt;
  int* block = d.counters;
  for (int s = 0; s < N_STEPS; ++s) {
    d.slots[s].resize(o.steps[s].asked.size());
    if (s == STEP_LDS) continue;
    for (Slot& slot : d.slots[s]) slot.counters = block += ODH_NCOUNT;
  }
  for (size_t f = 0; f < nlds_asked; ++f)
    d.slots[STEP_LDS][f].counters = (int*)((char*)d.lds_table + nldstab + lds_block * f);
  t0 = Clock::now();
  if (o.streams >= 1) HIP_TRY(hipStreamCreateWithFlags(&d.sg, hipStreamNonBlocking));
  if (o.streams == 2) HIP_TRY(hipStreamCreateWithFlags(&d.sh, hipStreamNonBlocking));
  else d.sh = d.sg;
  d.streams_ms = ms_since(t0);
  t0 = Clock::now();
  for (hipEvent_t* e : {&d.e0, &d.e_gemm, &d.e_h0, &d.e_h1, &d.e_link0, &d.e_link1, &d.e_r0, &d.e_r1})
    HIP_TRY(hipEventCreate(e));
  for (auto& slots : d.slots)
    for (Slot& slot : slots) {
      HIP_TRY(hipEventCreate(&slot.e0));
      HIP_TRY(hipEventCreate(&slot.e1));
    }
  d.events_ms = ms_since(t0);
  // the first operation on the stream: on the null stream it creates the hardware queue, here
  // while the other thread is still loading the code object
  t0 = Clock::now();
  HIP_TRY(hipMemsetAsync(d.counters, 0, sizeof(int) * ODH_NCOUNT * (1 + nslots), d.sg));
  d.first_op_ms = ms_since(t0);
  return true;
}

bool setup_fill(Dev& d, const Options& o) {
  HIP_TRY(hipSetDevice(d.index));
  HIP_TRY(odh_probe_fill(d.a, d.bt, o.M, o.N, o.K, d.sg));
  if (o.fault == "gemm") {
    // one corrupted operand element: row 0 of C is wrong in every column
    HIP_TRY(hipMemsetAsync(d.a, 0x44, 2, d.sg));
  }
  d.seed = 0x9E3779B9u ^ (uint32_t)(d.index * 0x85EBCA6Bu) ^ (uint32_t)getpid();
  return true;
}

bool launch(Dev& d, const Options& o) {
  HIP_TRY(hipSetDevice(d.index));
  unsigned* c = (unsigned*)d.counters;
  auto sweep = [&]() -> bool {
    HIP_TRY(hipEventRecord(d.e_h0, d.sh));
    HIP_TRY(odh_hbm_write(d.hbm, o.hbm_bytes, d.seed, 0, d.sh));
    HIP_TRY(odh_hbm_check(d.hbm, o.hbm_bytes, o.fault == "hbm" ? d.seed + 1 : d.seed,
                          (unsigned long long*)(d.counters + ODH_SLOT_HBM_ERR), d.sh));
    HIP_TRY(hipEventRecord(d.e_h1, d.sh));
    return true;
  };
  HIP_TRY(hipEventRecord(d.e0, d.sg));
  if (d.sh != d.sg) {
    // the memory-bound sweep first, on the second stream: the GEMM's one workgroup per CU
    // co-resides with its waves
    HIP_TRY(hipStreamWaitEvent(d.sh, d.e0, 0));
    if (!sweep()) return false;
  }
  HIP_TRY(odh_probe_gemm_verify(d.a, d.bt, o.M, o.N, o.K, d.tile_xcd, d.counters + ODH_SLOT_XCD_BLOCKS,
                                c + ODH_SLOT_GEMM_ERR, c + ODH_SLOT_ERR_XCD, d.sg));
  HIP_TRY(hipEventRecord(d.e_gemm, d.sg));
  // one stream: the sweep after the GEMM, so e0..e_gemm still times the GEMM alone
  if (d.sh == d.sg && !sweep()) return false;
  return true;
}

bool drain(Dev& d) {
  HIP_TRY(hipSetDevice(d.index));
  if (d.sh != d.sg) HIP_TRY(hipStreamSynchronize(d.sh));
  HIP_TRY(hipStreamSynchronize(d.sg));
  return true;
}

bool finish(Dev& d) {
  if (!drain(d)) return false;
  HIP_TRY(hipEventElapsedTime(&d.gemm_ms, d.e0, d.e_gemm));
  HIP_TRY(hipEventElapsedTime(&d.hbm_ms, d.e_h0, d.e_h1));
  return true;
}

// a format of --mx, after the sweep: the operands re-encoded into the bf16 operands' buffers (that
// GEMM is done, and the codes are no larger) with their scales and the table, then the fused check
bool mx_run(Dev& d, const Options& o, int fmt, Slot& s) {
  HIP_TRY(hipSetDevice(d.index));
  HIP_TRY(odh_mx_fill(fmt, d.a, d.bt, d.mx_sa, d.mx_sbt, d.mx_table, o.M, o.N, o.K, d.sh));
  if (o.fault == "mx") {
    // A[0][0] becomes +3 (A[0][1] is 0, so byte 0 holds nothing else that is set in FP4's high nibble
    // or the packed formats' upper two bits): row 0 of C is wrong wherever Bt[j][0] != 0
    const int three = fmt == ODH_MX_FP4   ? 0x05
                      : fmt == ODH_MX_BF8 ? 0x42
                      : fmt == ODH_MX_FP6 ? 0x14
                      : fmt == ODH_MX_BF6 ? 0x12
                                          : 0x44;
    HIP_TRY(hipMemsetAsync(d.a, three, 1, d.sh));
  }
  HIP_TRY(hipEventRecord(s.e0, d.sh));
  HIP_TRY(odh_mx_probe_gemm_verify(fmt, d.a, d.bt, d.mx_sa, d.mx_sbt, d.mx_table, o.M, o.N, o.K, nullptr, s.counters,
                                   d.sh));
  HIP_TRY(hipEventRecord(s.e1, d.sh));
  HIP_TRY(hipMemcpyAsync(s.host, s.counters, sizeof s.host, hipMemcpyDeviceToHost, d.sh));
  return true;
}

// a format of --dtypes, after the sweep and before --mx: the operands re-encoded into the bf16
// operands' buffers (halves are as large, int8 half as large), then the fused check
bool dt_run(Dev& d, const Options& o, int fmt, Slot& s) {
  HIP_TRY(hipSetDevice(d.index));
  HIP_TRY(odh_dense_fill(fmt, d.a, d.bt, o.M, o.N, o.K, d.sh));
  if (o.fault == "dtypes") {
    // A[0][0] becomes +1 (the half 0x3C00, or the int8 25 = 1 × ODH_DT_I8_MUL_A): row 0 of C is
    // wrong wherever Bt[j][0] != 0
    if (fmt == ODH_DT_I8) {
      HIP_TRY(hipMemsetAsync(d.a, ODH_DT_I8_MUL_A, 1, d.sh));
    } else {
      HIP_TRY(hipMemsetAsync(d.a, 0x00, 1, d.sh));
      HIP_TRY(hipMemsetAsync((char*)d.a + 1, 0x3C, 1, d.sh));
    }
  }
  HIP_TRY(hipEventRecord(s.e0, d.sh));
  HIP_TRY(odh_dense_probe_gemm_verify(fmt, d.a, d.bt, o.M, o.N, o.K, nullptr, s.counters, d.sh));
  HIP_TRY(hipEventRecord(s.e1, d.sh));
  HIP_TRY(hipMemcpyAsync(s.host, s.counters, sizeof s.host, hipMemcpyDeviceToHost, d.sh));
  return true;
}

// a format of --fp, after --dtypes and before --mx: the operands times odd constants as floats or
// doubles into the operands' buffers (sized for the widest asked-for format), then the fused check
bool fp_run(Dev& d, const Options& o, int fmt, Slot& s) {
  HIP_TRY(hipSetDevice(d.index));
  HIP_TRY(odh_fp_fill(fmt, d.a, d.bt, o.M, o.N, o.K, d.sh));
  if (o.fault == "fp") {
    // A[0][0] becomes +MUL_A (the fill has -2 MUL_A): row 0 of C is wrong wherever Bt[j][0] != 0
    static const float one32 = ODH_FP_F32_MUL_A;
    static const double one64 = ODH_FP_F64_MUL_A;
    if (fmt == ODH_FP_F64)
      HIP_TRY(hipMemcpyAsync(d.a, &one64, sizeof one64, hipMemcpyHostToDevice, d.sh));
    else
      HIP_TRY(hipMemcpyAsync(d.a, &one32, sizeof one32, hipMemcpyHostToDevice, d.sh));
  }
  HIP_TRY(hipEventRecord(s.e0, d.sh));
  HIP_TRY(odh_fp_probe_gemm_verify(fmt, d.a, d.bt, o.M, o.N, o.K, nullptr, s.counters, d.sh));
  HIP_TRY(hipEventRecord(s.e1, d.sh));
  HIP_TRY(hipMemcpyAsync(s.host, s.counters, sizeof s.host, hipMemcpyDeviceToHost, d.sh));
  return true;
}

// a format of --sparse, after --fp and before --mx: the pruned A compressed, its metadata and the dense Bt
// (no larger than the bf16 operands) with the table, then the fused check
bool sp_run(Dev& d, const Options& o, int fmt, Slot& s) {
  HIP_TRY(hipSetDevice(d.index));
  HIP_TRY(odh_sparse_fill(fmt, d.a, d.sp_meta, d.bt, d.sp_table, o.M, o.N, o.K, d.sh));
  if (o.fault == "sparse") {
    // the nibble of row 0, group 0 becomes the pair (0,1) (the fill has (0,3); byte 0 is 0xEC, group 1
    // in its high nibble): the kept A[0][3] = -1 meets Bt[j][1] instead of Bt[j][3], which differ for
    // every j, so row 0 of C is wrong in every column
    HIP_TRY(hipMemsetAsync(d.sp_meta, 0xE4, 1, d.sh));
  }
  HIP_TRY(hipEventRecord(s.e0, d.sh));
  HIP_TRY(odh_sparse_probe_gemm_verify(fmt, d.a, d.sp_meta, d.bt, d.sp_table, o.M, o.N, o.K, nullptr, s.counters,
                                       d.sh));
  HIP_TRY(hipEventRecord(s.e1, d.sh));
  HIP_TRY(hipMemcpyAsync(s.host, s.counters, sizeof s.host, hipMemcpyDeviceToHost, d.sh));
  return true;
}

// a format of --cvt, after --mx: its scale table, then the fused check of its converter
bool cvt_run(Dev& d, const Options& o, int fmt, Slot& s) {
  HIP_TRY(hipSetDevice(d.index));
  HIP_TRY(odh_cvt_fill(fmt, d.cvt_table, d.sh));
  if (o.fault == "cvt") {
    // entry 3 of the table becomes 0 (the fill has at least 4 there): every case of that scale is divided by
    // another power of two than the one it was multiplied by (bf16: gets another exponent than it expects)
    HIP_TRY(hipMemsetAsync((char*)d.cvt_table + 3, 0, 1, d.sh));
  }
  HIP_TRY(hipEventRecord(s.e0, d.sh));
  HIP_TRY(odh_cvt_probe_verify(fmt, d.cvt_table, s.counters, d.sh));
  HIP_TRY(hipEventRecord(s.e1, d.sh));
  HIP_TRY(hipMemcpyAsync(s.host, s.counters, sizeof s.host, hipMemcpyDeviceToHost, d.sh));
  return true;
}

// a check of --lds, after --cvt: its key table, then the fused check; the counter block is cleared here
bool lds_run(Dev& d, const Options& o, int check, Slot& s) {
  HIP_TRY(hipSetDevice(d.index));
  HIP_TRY(hipMemsetAsync(s.counters, 0, sizeof(int) * (ODH_NCOUNT + ODH_LDS_CU_WORDS), d.sh));
  HIP_TRY(odh_lds_fill(check, d.lds_table, d.sh));
  if (o.fault == "lds") {
    // bit 0 of byte 5 of the table flips (a change a 4- or 6-bit element cannot miss): everything stored with
    // key dword 1 differs from what the kernel expects of it
    unsigned char byte = 0;
    HIP_TRY(hipMemcpyAsync(&byte, (char*)d.lds_table + 5, 1, hipMemcpyDeviceToHost, d.sh));
    HIP_TRY(hipStreamSynchronize(d.sh));
    HIP_TRY(hipMemsetAsync((char*)d.lds_table + 5, byte ^ 1, 1, d.sh));
  }
  HIP_TRY(hipEventRecord(s.e0, d.sh));
  HIP_TRY(odh_lds_probe_verify(check, d.lds_table, s.counters, d.sh));
  HIP_TRY(hipEventRecord(s.e1, d.sh));
  HIP_TRY(hipMemcpyAsync(s.host, s.counters, sizeof s.host, hipMemcpyDeviceToHost, d.sh));
  return true;
}

// a format of --mfma16, after --lds: the operands in the format's layout by the fill of that layout, into the bf16
// operands' buffers (none is larger), then the fused check on the 16×16 instruction
bool m16_run(Dev& d, const Options& o, int fmt, Slot& s) {
  HIP_TRY(hipSetDevice(d.index));
  const bool scaled = fmt == ODH_M16_FP8 || fmt == ODH_M16_FP4;
  if (scaled)
    HIP_TRY(odh_mx_fill(fmt == ODH_M16_FP8 ? ODH_MX_FP8 : ODH_MX_FP4, d.a, d.bt, d.mx_sa, d.mx_sbt, d.mx_table, o.M,
                        o.N, o.K, d.sh));
  else if (fmt == ODH_M16_BF16)
    HIP_TRY(odh_probe_fill(d.a, d.bt, o.M, o.N, o.K, d.sh));
  else
    HIP_TRY(odh_dense_fill(fmt == ODH_M16_F16 ? ODH_DT_F16 : ODH_DT_I8, d.a, d.bt, o.M, o.N, o.K, d.sh));
  if (o.fault == "mfma16") {
    // A[0][0], -2 in every fill, becomes wrong, as in the steps these layouts come from: +3 as FP8 0x44 or FP4 0x05
    // (A[0][1] is 0), +1 × ODH_DT_I8_MUL_A as int8, +1 as the half 0x3C00 or the bf16 0x3F80: row 0 of C is wrong
    // wherever Bt[j][0] != 0
    if (fmt == ODH_M16_FP8 || fmt == ODH_M16_FP4 || fmt == ODH_M16_I8) {
      HIP_TRY(hipMemsetAsync(d.a, fmt == ODH_M16_FP8 ? 0x44 : fmt == ODH_M16_FP4 ? 0x05 : ODH_DT_I8_MUL_A, 1, d.sh));
    } else {
      HIP_TRY(hipMemsetAsync(d.a, fmt == ODH_M16_F16 ? 0x00 : 0x80, 1, d.sh));
      HIP_TRY(hipMemsetAsync((char*)d.a + 1, fmt == ODH_M16_F16 ? 0x3C : 0x3F, 1, d.sh));
    }
  }
  HIP_TRY(hipEventRecord(s.e0, d.sh));
  HIP_TRY(odh_m16_probe_gemm_verify(fmt, d.a, d.bt, scaled ? d.mx_sa : nullptr, scaled ? d.mx_sbt : nullptr,
                                    scaled ? d.mx_table : nullptr, o.M, o.N, o.K, nullptr, s.counters, d.sh));
  HIP_TRY(hipEventRecord(s.e1, d.sh));
  HIP_TRY(hipMemcpyAsync(s.host, s.counters, sizeof s.host, hipMemcpyDeviceToHost, d.sh));
  return true;
}

bool step_finish(Dev& d, Slot& s) {
  HIP_TRY(hipSetDevice(d.index));
  HIP_TRY(hipStreamSynchronize(d.sh));
  HIP_TRY(hipEventElapsedTime(&s.ms, s.e0, s.e1));
  return true;
}

// reader d checks source s's freshly written pattern over xGMI
bool link_check(Dev& d, const Dev& s, const Options& o) {
  HIP_TRY(odh_peer_enable(d.index, s.index));
  HIP_TRY(hipSetDevice(d.index));
  const size_t n = (o.xgmi_bytes < o.hbm_bytes ? o.xgmi_bytes : o.hbm_bytes) & ~(size_t)15;
  HIP_TRY(hipEventRecord(d.e_link0, d.sg));
  HIP_TRY(odh_hbm_check(s.hbm, n, o.fault == "xgmi" ? s.seed ^ 1u : s.seed,
                        (unsigned long long*)(d.counters + ODH_SLOT_CLI_XGMI_ERR), d.sg));
  HIP_TRY(hipEventRecord(d.e_link1, d.sg));
  d.link_source = s.index;
  return true;
}

bool link_finish(Dev& d) {
  HIP_TRY(hipSetDevice(d.index));
  HIP_TRY(hipMemcpyAsync(d.host, d.counters, sizeof d.host, hipMemcpyDeviceToHost, d.sg));
  HIP_TRY(hipStreamSynchronize(d.sg));
  if (d.link_source >= 0) HIP_TRY(hipEventElapsedTime(&d.link_ms, d.e_link0, d.e_link1));
  return true;
}

void release(Dev& d) {
  // teardown: nothing is left to undo if a free fails
  (void)hipSetDevice(d.index);
  if (d.block) (void)hipFree(d.block);
  for (hipEvent_t e : {d.e0, d.e_gemm, d.e_h0, d.e_h1, d.e_link0, d.e_link1, d.e_r0, d.e_r1})
    if (e) (void)hipEventDestroy(e);
  for (auto& slots : d.slots)
    for (Slot& slot : slots)
      for (hipEvent_t e : {slot.e0, slot.e1})
        if (e) (void)hipEventDestroy(e);
  if (d.sh && d.sh != d.sg) (void)hipStreamDestroy(d.sh);
  if (d.sg) (void)hipStreamDestroy(d.sg);
}

uint64_t u64(const int* h, int i) { return (uint64_t)(uint32_t)h[i] | ((uint64_t)(uint32_t)h[i + 1] << 32); }

// RCCL, resolved at run time: only --rccl-mib pays for loading the library
struct Rccl {
  decltype(&ncclCommInitAll) init_all = nullptr;
  decltype(&ncclAllReduce) all_reduce = nullptr;
  decltype(&ncclGroupStart) group_start = nullptr;
  decltype(&ncclGroupEnd) group_end = nullptr;
  decltype(&ncclCommDestroy) destroy = nullptr;
  decltype(&ncclGetErrorString) error_string = nullptr;

  bool load(std::string& err) {
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) {
      const char* e = dlerror();
      err = std::string("cannot load librccl: ") + (e ? e : "?");
      return false;
    }
    init_all = (decltype(init_all))dlsym(h, "ncclCommInitAll");
    all_reduce = (decltype(all_reduce))dlsym(h, "ncclAllReduce");
    group_start = (decltype(group_start))dlsym(h, "ncclGroupStart");
    group_end = (decltype(group_end))dlsym(h, "ncclGroupEnd");
    destroy = (decltype(destroy))dlsym(h, "ncclCommDestroy");
    error_string = (decltype(error_string))dlsym(h, "ncclGetErrorString");
    if (!init_all || !all_reduce || !group_start || !group_end || !destroy || !error_string) {
      err = "librccl lacks the NCCL API";
      return false;
    }
    return true;  // never unloaded: the process leaves through _Exit
  }
};

struct RcclRun {
  double load_ms = 0, init_ms = 0, wall_ms = 0;  // dlopen (the library is 570 MB), ncclCommInitAll, the collective
  size_t bytes = 0;
};

#define RCCL_TRY(expr)                                                                   \
  do {                                                                                   \
    const ncclResult_t r_ = (expr);                                                      \
    if (r_ != ncclSuccess) {                                                             \
      err = std::string(#expr) + ": " + rc.error_string(r_);                             \
      for (ncclComm_t c : comms)                                                         \
        if (c) (void)rc.destroy(c);                                                      \
      return false;                                                                      \
    }                                                                                    \
  } while (0)

// Sum-all-reduce of float32 over every device: device i contributes i+1, so every element
// of every result must be n(n+1)/2 (exact in float).  Send / receive buffers are the two
// halves of each device's (already checked) HBM buffer.  On return each device's mismatch
// count sits in slot ODH_SLOT_CLI_RCCL_ERR of its counters and of its host copy.
bool rccl_allreduce(std::vector<Dev>& devs, const Options& o, RcclRun& run, std::string& err) {
  Rccl rc;
  const auto t_load = Clock::now();
  if (!rc.load(err)) return false;
  run.load_ms = ms_since(t_load);
  const int n = (int)devs.size();
  run.bytes = o.rccl_bytes & ~(size_t)15;
  const size_t count = run.bytes / 4;
  std::vector<int> ids(n);
  for (int i = 0; i < n; ++i) ids[i] = devs[i].index;
  std::vector<ncclComm_t> comms(n, nullptr);
  auto t0 = Clock::now();
  const ncclResult_t ri = rc.init_all(comms.data(), n, ids.data());
  if (ri != ncclSuccess) {  // no communicator to destroy: a failed init leaves none usable
    err = std::string("ncclCommInitAll: ") + rc.error_string(ri);
    return false;
  }
  run.init_ms = ms_since(t0);
  auto hip_fail = [&](Dev& d, const char* what, hipError_t e) {
    err = "GPU " + std::to_string(d.index) + ": " + what + ": " + hipGetErrorString(e);
    for (ncclComm_t c : comms) (void)rc.destroy(c);
    return false;
  };
  for (int i = 0; i < n; ++i) {
    Dev& d = devs[i];
    float v = (float)(i + 1) + (o.fault == "rccl" && i == 0 ? 0.5f : 0.0f);
    uint32_t bits;
    std::memcpy(&bits, &v, 4);
    hipError_t e = hipSetDevice(d.index);
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)d.hbm, (int)bits, count, d.sg);
    if (e == hipSuccess) e = hipMemsetAsync((char*)d.hbm + run.bytes, 0, run.bytes, d.sg);
    if (e == hipSuccess) e = hipMemsetAsync(d.counters + ODH_SLOT_CLI_RCCL_ERR, 0, 8, d.sg);
    if (e == hipSuccess) e = hipEventRecord(d.e_r0, d.sg);
    if (e != hipSuccess) return hip_fail(d, "fill", e);
  }
  t0 = Clock::now();
  RCCL_TRY(rc.group_start());
  for (int i = 0; i < n; ++i) {
    Dev& d = devs[i];
    const ncclResult_t r = rc.all_reduce(d.hbm, (char*)d.hbm + run.bytes, count, ncclFloat32, ncclSum, comms[i], d.sg);
    if (r != ncclSuccess) {
      (void)rc.group_end();
      err = std::string("ncclAllReduce: ") + rc.error_string(r);
      for (ncclComm_t c : comms) (void)rc.destroy(c);
      return false;
    }
  }
  RCCL_TRY(rc.group_end());
  const float want = (float)n * (float)(n + 1) / 2.0f;
  uint32_t want_bits;
  std::memcpy(&want_bits, &want, 4);
  for (Dev& d : devs) {
    hipError_t e = hipSetDevice(d.index);
    if (e == hipSuccess) e = hipEventRecord(d.e_r1, d.sg);
    if (e == hipSuccess)
      e = (hipError_t)odh_const_check((char*)d.hbm + run.bytes, run.bytes, want_bits,
                                      (unsigned long long*)(d.counters + ODH_SLOT_CLI_RCCL_ERR), d.sg);
    if (e == hipSuccess)
      e = hipMemcpyAsync(d.host + ODH_SLOT_CLI_RCCL_ERR, d.counters + ODH_SLOT_CLI_RCCL_ERR, 8, hipMemcpyDeviceToHost,
                         d.sg);
    if (e != hipSuccess) return hip_fail(d, "check", e);
  }
  for (Dev& d : devs) {
    hipError_t e = hipSetDevice(d.index);
    if (e == hipSuccess) e = hipStreamSynchronize(d.sg);
    if (e == hipSuccess) e = hipEventElapsedTime(&d.rccl_ms, d.e_r0, d.e_r1);
    if (e != hipSuccess) return hip_fail(d, "sync", e);
  }
  run.wall_ms = ms_since(t0);
  for (ncclComm_t c : comms) (void)rc.destroy(c);
  return true;
}

}  // namespace

// ms from the spawner's CLOCK_REALTIME stamp (ODH_PROBE_T0_NS, ns) to now: process start,
// dynamic linking of the HIP runtime; -1 when the spawner did not stamp
double exec_ms() {
  const char* t0 = std::getenv("ODH_PROBE_T0_NS");
  if (!t0 || !*t0) return -1.0;
  timespec ts;
  clock_gettime(CLOCK_REALTIME, &ts);
  return (ts.tv_sec * 1e9 + ts.tv_nsec - std::strtod(t0, nullptr)) / 1e6;
}

extern "C" int odh_probe_cli(int argc, char** argv) {
  const double t_exec = exec_ms();
  const auto t_start = Clock::now();
  Options o;
  if (!parse(argc, argv, o)) return usage(argc > 0 ? argv[0] : "odh-gpu-probe");

  // watchdog: a wedged GPU must not hold the pod in Init forever; each call has its own flag,
  // so a later call in the same process is never cut short by an earlier call's watchdog
  auto finished = std::make_shared<std::atomic<bool>>(false);
  std::thread([o, t_start, finished] {
    const auto deadline = t_start + std::chrono::milliseconds(o.timeout_ms);
    while (!finished->load() && Clock::now() < deadline) std::this_thread::sleep_for(std::chrono::milliseconds(5));
    if (!finished->exchange(true)) {
      emit(o, fail_json("timeout", "probe did not finish within " + std::to_string(o.timeout_ms) + " ms",
                        ms_since(t_start)));
      std::_Exit(3);
    }
  }).detach();
  auto done = [&](int rc, const std::string& json) {
    if (finished->exchange(true)) {  // the watchdog reported already and is exiting
      for (;;) std::this_thread::sleep_for(std::chrono::seconds(1));
    }
    emit(o, json);
    return rc;
  };

  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return done(2, fail_json("no GPU", e != hipSuccess ? hipGetErrorString(e) : "no visible device", ms_since(t_start)));
  std::vector<Dev> devs(ndev);
  for (int i = 0; i < ndev; ++i) devs[i].index = i;
  e = hipSetDevice(0);
  if (e == hipSuccess) e = hipFree(nullptr);  // context creation: the HIP-init share of the run
  if (e != hipSuccess) return done(2, fail_json("hip init", hipGetErrorString(e), ms_since(t_start)));
  const double t_init = ms_since(t_start);

  std::string err;
  auto fail_all = [&](Dev& d) {
    err = "GPU " + std::to_string(d.index) + ": " + d.error;
    for (Dev& x : devs) release(x);
    return done(2, fail_json("hip", err, ms_since(t_start)));
  };
  // the code object loads on a second thread while this one allocates and makes the stream's
  // hardware queue (both host-side work the pod waits for)
  std::vector<int> preload_rc(ndev, 0);
  double t_preload = 0;
  std::thread preload([&] {
    for (int i = 0; i < ndev; ++i) {
      hipError_t se = hipSetDevice(i);
      preload_rc[i] = se != hipSuccess ? (int)se : odh_probe_preload();
    }
    t_preload = ms_since(t_start);
  });
  bool alloc_ok = true;
  Dev* bad = nullptr;
  for (Dev& d : devs)
    if (!setup_alloc(d, o)) {
      alloc_ok = false;
      bad = &d;
      break;
    }
  const double t_alloc_only = ms_since(t_start);
  preload.join();
  if (!alloc_ok) return fail_all(*bad);
  for (int i = 0; i < ndev; ++i)
    if (preload_rc[i] != 0) {
      devs[i].error = std::string("odh_probe_preload: ") + hipGetErrorString((hipError_t)preload_rc[i]);
      return fail_all(devs[i]);
    }
  const double t_malloc = ms_since(t_start);
  for (Dev& d : devs)
    if (!setup_fill(d, o)) return fail_all(d);
  for (Dev& d : devs)
    if (!drain(d)) return fail_all(d);  // operands filled on every device
  const double t_alloc = ms_since(t_start);
  const auto t_probe0 = Clock::now();
  for (Dev& d : devs)
    if (!launch(d, o)) return fail_all(d);
  for (Dev& d : devs)
    if (!finish(d)) return fail_all(d);
  const double probe_ms = ms_since(t_probe0);
  // --dtypes, --fp, --sparse, --mx, --cvt, --lds, then --mfma16: one format at a time over every device, so each format has a host time
  // of its own
  std::vector<double> step_host_ms[N_STEPS];  // per asked-for format: launch on every device to the last one done
  double step_total_ms[N_STEPS] = {};
  for (int si : {STEP_DTYPES, STEP_FP, STEP_SPARSE, STEP_MX, STEP_CVT, STEP_LDS, STEP_MFMA16}) {
    const Step& s = o.steps[si];
    step_host_ms[si].resize(s.asked.size());  // sized before the clock starts
    const auto t_step0 = Clock::now();
    for (size_t f = 0; f < s.asked.size(); ++f) {
      const auto t0 = Clock::now();
      for (Dev& d : devs)
        if (!s.run(d, o, s.asked[f], d.slots[si][f])) return fail_all(d);
      for (Dev& d : devs)
        if (!step_finish(d, d.slots[si][f])) return fail_all(d);
      step_host_ms[si][f] = ms_since(t0);
    }
    step_total_ms[si] = ms_since(t_step0);
  }
  // xGMI ring: device r reads the pattern device r-1 wrote (2 GPUs: each reads the other)
  const auto t_link0 = Clock::now();
  if (ndev >= 2) {
    for (int r = 0; r < ndev; ++r)
      if (!link_check(devs[r], devs[(r + ndev - 1) % ndev], o)) return fail_all(devs[r]);
  }
  for (Dev& d : devs)
    if (!link_finish(d)) return fail_all(d);
  const double link_ms = ndev >= 2 ? ms_since(t_link0) : 0.0;
  RcclRun rr;
  if (o.rccl_bytes) {
    std::string rerr;
    if (!rccl_allreduce(devs, o, rr, rerr)) {
      for (Dev& x : devs) release(x);
      return done(2, fail_json("rccl", rerr, ms_since(t_start)));
    }
  }

  const int tiles = odh_gemm_tiles(o.M, o.N, o.K);
  const double flops = 2.0 * o.M * o.N * o.K;
  bool ok = true;
  std::string first_err;
  std::string res = "[";
  for (Dev& d : devs) {
    const int* h = d.host;
    long blocks = 0;
    int xcds = 0;
    for (int x = 0; x < ODH_N_XCD; ++x) {
      blocks += h[ODH_SLOT_XCD_BLOCKS + x];
      xcds += h[ODH_SLOT_XCD_BLOCKS + x] > 0;
    }
    const uint64_t gemm_err = (uint32_t)h[ODH_SLOT_GEMM_ERR], hbm_err = u64(h, ODH_SLOT_HBM_ERR);
    const bool dok = gemm_err == 0 && hbm_err == 0 && blocks == tiles;
    if (!dok && first_err.empty()) {
      char b[160];
      std::snprintf(b, sizeof b, "GPU %d: %llu GEMM mismatches, %llu HBM mismatches, %ld/%d tiles", d.index,
                    (unsigned long long)gemm_err, (unsigned long long)hbm_err, blocks, tiles);
      first_err = b;
    }
    ok = ok && dok;
    std::string ex = "[";
    for (int x = 0; x < ODH_N_XCD; ++x)
      ex += std::to_string((unsigned)h[ODH_SLOT_ERR_XCD + x]) + (x < ODH_N_XCD - 1 ? "," : "]");
    char b[512];
    std::snprintf(b, sizeof b,
                  "%s{\"device\":%d,\"ok\":%s,\"gemm_tflops\":%.1f,\"hbm_gbps\":%.1f,\"gemm_ms\":%.4f,\"hbm_ms\":%.4f,"
                  "\"gemm_errors\":%llu,\"hbm_errors\":%llu,\"xcds\":%d,\"err_xcd\":%s}",
                  d.index ? "," : "", d.index, dok ? "true" : "false",
                  d.gemm_ms > 0 ? flops / (d.gemm_ms * 1e-3) / 1e12 : 0.0,
                  d.hbm_ms > 0 ? 2.0 * o.hbm_bytes / (d.hbm_ms * 1e-3) / 1e9 : 0.0, d.gemm_ms, d.hbm_ms,
                  (unsigned long long)gemm_err, (unsigned long long)hbm_err, xcds, ex.c_str());
    res += b;
  }
  res += "]";
  std::string links = "[";
  if (ndev >= 2) {
    const size_t n = (o.xgmi_bytes < o.hbm_bytes ? o.xgmi_bytes : o.hbm_bytes) & ~(size_t)15;
    for (Dev& d : devs) {
      const uint64_t lerr = u64(d.host, ODH_SLOT_CLI_XGMI_ERR);
      const bool lok = lerr == 0;
      if (!lok && first_err.empty())
        first_err = "xGMI link GPU " + std::to_string(d.link_source) + " -> GPU " + std::to_string(d.index) + ": " +
                    std::to_string((unsigned long long)lerr) + " mismatches";
      ok = ok && lok;
      char b[200];
      std::snprintf(b, sizeof b, "%s{\"reader\":%d,\"source\":%d,\"ok\":%s,\"errors\":%llu,\"gbps\":%.1f}",
                    d.index ? "," : "", d.index, d.link_source, lok ? "true" : "false", (unsigned long long)lerr,
                    d.link_ms > 0 ? n / (d.link_ms * 1e-3) / 1e9 : 0.0);
      links += b;
    }
  }
  links += "]";
  std::string rccl;
  if (o.rccl_bytes) {
    uint64_t rerr = 0;
    float slowest = 0;
    for (Dev& d : devs) {
      rerr += u64(d.host, ODH_SLOT_CLI_RCCL_ERR);
      slowest = d.rccl_ms > slowest ? d.rccl_ms : slowest;
    }
    const bool rok = rerr == 0;
    if (!rok && first_err.empty())
      first_err = "RCCL all-reduce over " + std::to_string(ndev) + " GPUs: " +
                  std::to_string((unsigned long long)rerr) + " mismatches";
    ok = ok && rok;
    // bus bandwidth as nccl-tests define it: algbw x 2(n-1)/n
    const double algbw = slowest > 0 ? rr.bytes / (slowest * 1e-3) / 1e9 : 0.0;
    char b[256];
    std::snprintf(b, sizeof b,
                  ",\"rccl\":{\"ranks\":%d,\"ok\":%s,\"errors\":%llu,\"mib\":%zu,\"load_ms\":%.2f,\"init_ms\":%.2f,"
                  "\"allreduce_ms\":%.4f,\"busbw_gbps\":%.1f}",
                  ndev, rok ? "true" : "false", (unsigned long long)rerr, rr.bytes >> 20, rr.load_ms, rr.init_ms, slowest,
                  ndev > 1 ? algbw * 2.0 * (ndev - 1) / ndev : algbw);
    rccl = b;
  }
  // the objects of the optional GEMM steps, "" without them: per format, whatever the device count,
  // total mismatches and the slowest device's kernel time
  std::string steps;
  char step_timing[336] = "";  // N_STEPS entries of "word":ms,
  for (int si = 0; si < N_STEPS; ++si) {
    const Step& s = o.steps[si];
    // a flat step: total mismatches, the slowest device's kernel time summed over the checks, and the checks
    // that counted mismatches or missed workgroups
    uint64_t flat_errs = 0;
    std::string flat_bad;
    std::vector<float> flat_ms(devs.size(), 0.f);
    for (size_t f = 0; f < s.asked.size(); ++f) {
      const int ftiles = s.tiles ? s.tiles(s.asked[f], o.M, o.N) : tiles;
      uint64_t errs = 0;
      float slowest = 0;
      bool fok = true;
      for (Dev& d : devs) {
        const Slot& slot = d.slots[si][f];
        const int* h = slot.host;
        long blocks = 0;
        std::string where;
        for (int x = 0; x < ODH_N_XCD; ++x) {
          blocks += h[ODH_SLOT_XCD_BLOCKS + x];
          if (h[ODH_SLOT_ERR_XCD + x]) where += (where.empty() ? "" : ",") + std::to_string(x);
        }
        const uint32_t e = (uint32_t)h[ODH_SLOT_GEMM_ERR];
        errs += e;
        slowest = slot.ms > slowest ? slot.ms : slowest;
        if (e == 0 && blocks == ftiles) continue;
        fok = false;
        if (first_err.empty()) {
          char b[200];
          std::snprintf(b, sizeof b, "GPU %d: %s%s%s: %u %s mismatches on XCD %s, %ld/%d tiles", d.index,
                        s.flat ? s.word : "", s.flat ? " " : "", s.name(s.asked[f]), e, s.what,
                        where.empty() ? "-" : where.c_str(), blocks, ftiles);
          first_err = b;
        }
      }
      ok = ok && fok;
      if (s.flat) {
        flat_errs += errs;
        if (!fok) flat_bad += (flat_bad.empty() ? "" : ",") + std::string(s.name(s.asked[f]));
        for (size_t di = 0; di < devs.size(); ++di) flat_ms[di] += devs[di].slots[si][f].ms;
        continue;
      }
      const double rate = slowest <= 0 ? 0.0
                          : s.work     ? s.work(s.asked[f]) / (slowest * 1e6)
                                       : flops / (slowest * 1e-3) / 1e12;
      char b[160];
      const int at = std::snprintf(b, sizeof b, "%s\"%s\":{\"ok\":%s,\"errors\":%llu,\"ms\":%.4f,\"%s\":%.1f",
                                   f ? "," : (std::string(",\"") + s.word + "\":{").c_str(), s.name(s.asked[f]),
                                   fok ? "true" : "false", (unsigned long long)errs, slowest, s.rate, rate);
      if (s.host_ms)
        std::snprintf(b + at, sizeof b - at, ",\"host_ms\":%.3f}", step_host_ms[si][f]);
      else
        std::snprintf(b + at, sizeof b - at, "}");
      steps += b;
    }
    if (s.asked.empty()) continue;
    if (s.flat) {
      char b[200];
      std::snprintf(b, sizeof b, ",\"%s\":{\"ok\":%s,\"errors\":%llu,\"ms\":%.3f,\"bad\":\"%s\"", s.word,
                    flat_bad.empty() ? "true" : "false", (unsigned long long)flat_errs,
                    *std::max_element(flat_ms.begin(), flat_ms.end()), flat_bad.c_str());
      steps += b;
    }
    steps += "}";
    const size_t at = std::strlen(step_timing);
    std::snprintf(step_timing + at, sizeof step_timing - at, "\"%s\":%.3f,", s.word, step_total_ms[si]);
  }
  for (Dev& d : devs) release(d);
  char tail[640];
  std::snprintf(tail, sizeof tail,
                ",\"timings_ms\":{\"exec\":%.3f,\"hip_init\":%.3f,\"alloc_fill\":%.3f,\"alloc\":%.3f,"
                "\"code_load\":%.3f,\"fill\":%.3f,\"probe\":%.3f,\"xgmi\":%.3f,\"rccl\":%.3f,%s\"total\":%.3f}}",
                t_exec, t_init, t_alloc - t_init, t_alloc_only - t_init, t_preload - t_init, t_alloc - t_malloc, probe_ms,
                link_ms, rr.load_ms + rr.init_ms + rr.wall_ms, step_timing, ms_since(t_start));
  char setup[192];
  std::snprintf(setup, sizeof setup,
                ",\"setup_ms\":{\"malloc\":%.3f,\"streams\":%.3f,\"events\":%.3f,\"first_op\":%.3f,\"n_streams\":%d}",
                devs[0].malloc_ms, devs[0].streams_ms, devs[0].events_ms, devs[0].first_op_ms, o.streams);
  std::string json = std::string("{\"ok\":") + (ok ? "true" : "false") + ",\"devices\":" + std::to_string(ndev) +
                     ",\"shape\":[" + std::to_string(o.M) + "," + std::to_string(o.N) + "," + std::to_string(o.K) +
                     "],\"hbm_mib\":" + std::to_string(o.hbm_bytes >> 20) +
                     (first_err.empty() ? "" : ",\"error\":\"" + esc(first_err) + "\"") + ",\"results\":" + res +
                     ",\"links\":" + links + rccl + steps + setup + tail;
  return done(ok ? 0 : 1, json);
}
