// Host-side plumbing shared by the translation units of libaxvs.so: error string, launch status, the bump allocator over
// caller-owned buffers and its workspace checks (unsigned and signed sizes), per-device kernel attributes, the
// packed-weight / workspace views of one trajectory attention, and the launcher of the fused trajectory kernels (whose
// instantiations are compiled one (operand type, frame count) pair per translation unit: axvs_temporal_inst.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "../../include/axvs.h"
#include "axvs_common.h"

namespace axvs {

inline thread_local char g_err[512] = "";
// axvs_set_option("train_valu", 1): keep the spatial attention of the training tier on the fp32 VALU kernels (the head_dim 8 / 16
// path) instead of the fp32 MFMA ones -- A/B comparisons and tests of both.  Process-wide, not per thread: autograd runs the
// backward call on its own thread and forward / backward must agree on the kernel family (the statistics travel between them).
inline int g_train_valu = 0;
// The FORWARD GEMMs of the training tier split their operands into three bf16 pieces (fp32 accuracy, 6 MFMAs per product: the
// forward decides the ReLU masks); axvs_set_option("train_exact", 0) makes them two-piece (1.5e-5 per product, 3 MFMAs) like the
// backward ones, 2: three pieces for the input-gradient GEMMs as well -- see axvs_train_gemm.h.  Process-wide like train_valu.
inline int g_train_exact = 1;
// axvs_set_option("train_amp", 1 | 2): the GEMMs of the training tier (forward, input gradients, weight gradients) take ONE 16-bit piece per
// operand (1: bf16, 2: fp16) -- the products torch.autocast gives the reference's nn.Linear layers; 0 (default): split precision
inline int g_train_amp = 0;
// workgroups the spatial-attention kernels of the training tier are spread over (a constant: round 6 dropped the option key
// "train_spatial_wgs" with the other thresholds)
inline int g_spatial_wgs = 512;
// 0 (a constant as well: no option key sets it): the training tier's attention forward on the fp32 MFMA kernel (any axis length) instead of
// the split-precision 16-bit MFMA one (three bf16 pieces per operand, a frame's score tiles in registers; axis length <= 128)
inline int g_train_attn_split = 1;

// axvs_set_option("cc_aspp_affine", 1): the ASPP projection's norm is a per-channel affine (norm_fn 'syncbn' in eval mode, folded by the caller into
// aspp_norm_w / aspp_norm_b = scale / shift; 'none' = ones / zeros) instead of the channels-first LayerNorm of the shipped configs
inline thread_local int g_cc_aspp_affine = 0;
// axvs_set_option("cc_last_heads_only", 1): axvs_cc_module_fwd computes the predictor heads (class logits, mask einsum) of the LAST layer
// only; pred_logits / pred_masks then hold ONE layer.  The reference computes every layer's predictions in eval too (CC/...:283-318) and
// its inference path drops all but the last (maxtron_cc_model.py:301-: aux_outputs are read under self.training only): an inference
// pipeline that does not want them saves 3/4 of the mask einsum's HBM writes
inline thread_local int g_cc_last_only = 0;

// optional per-stage event recording (bench.py / tuning): events[i] is recorded on the stream after stage i; the entry point that
// records stages sets g_prof_next = 0 first (the axvs_profile_* entry points of the axial unit, axvs_api.hip, read the state)
inline thread_local hipEvent_t* g_prof_events = nullptr;
inline thread_local int g_prof_cap = 0;
inline thread_local int g_prof_next = 0;
inline thread_local int g_reg_passes = 0;      // bit 0 / 1: the last height (or only) / width trajectory pass ran the regular-tile instantiation (axvs_plan_regular_tiles)
constexpr int kMaxStages = 32;
inline thread_local const char* g_stage_names[kMaxStages] = {};
inline void mark(hipStream_t st, const char* name) {
  if (g_prof_next < kMaxStages) g_stage_names[g_prof_next] = name;
  if (g_prof_events && g_prof_next < g_prof_cap) (void)hipEventRecord(g_prof_events[g_prof_next], st);
  ++g_prof_next;
}

inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

inline int last_launch_status() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(AXVS_ERR_LAUNCH, "HIP launch failed: %s", hipGetErrorString(e));
  return AXVS_OK;
}

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

struct Carver {  // bump allocator over a caller-owned buffer (nullptr: size only)
  char* base;
  size_t off = 0;
  explicit Carver(void* p) : base(static_cast<char*>(p)) {}
  template <class T>
  T* take(size_t n) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off = align_up(off + n * sizeof(T));
    return p;
  }
  float* f(size_t n) { return take<float>(n); }
};

// bytes a carve step takes: the size query of a layout that its carver states -- carved([&](Carver& c) { carve_x(c, ...); })
template <class F>
size_t carved(F&& step) {
  Carver c(nullptr);
  step(c);
  return c.off;
}

inline int check_ws(size_t have, size_t need) {
  if (have < need) return fail(AXVS_ERR_WORKSPACE, "workspace too small: %zu < %zu", have, need);
  return AXVS_OK;
}
// the entries whose ABI takes a signed size: a negative one is too small as well
inline int check_ws(long long have, size_t need) {
  if (have < 0 || (size_t)have < need) return fail(AXVS_ERR_WORKSPACE, "workspace too small: %lld < %zu", have, need);
  return AXVS_OK;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: remember (device, kernel) pairs that have
// been raised so a second device in the same process is configured too.  The attribute is always raised to the full 160 KiB,
// never to the size of the launch at hand: the cache below remembers only THAT a kernel was configured, so a shape-dependent
// size would pin the first (possibly smaller) request and fail a later, larger launch.
inline int ensure_max_lds(const void* fn) {
  constexpr int kCap = 256;
  struct Entry { int dev; const void* fn; };
  static thread_local Entry seen[kCap];
  static thread_local int nseen = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fail(AXVS_ERR_LAUNCH, "hipGetDevice failed");
  for (int i = 0; i < nseen; ++i)
    if (seen[i].fn == fn && seen[i].dev == dev) return AXVS_OK;
  // the dynamic part may use what the kernel's static __shared__ objects leave of the CU's 160 KiB
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, fn) != hipSuccess) return fail(AXVS_ERR_LAUNCH, "hipFuncGetAttributes failed");
  const int bytes = 160 * 1024 - (int)((fa.sharedSizeBytes + 255) / 256 * 256);
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
    return fail(AXVS_ERR_LAUNCH, "hipFuncSetAttribute failed");
  if (nseen < kCap) seen[nseen++] = Entry{dev, fn};
  return AXVS_OK;
}

struct TrajPacked {  // pointers into the packed blob
  u16 *wq, *wk, *wv, *wpq, *wpkv, *wp, *wk2t;     // wk2t: transposed k half of proj_kv (fused temporal kernel, C = 256)
  u16 *wk2n, *wv2h;                               // per-head copies for the reassociated generic temporal half (axvs_misc.h)
  float *bq, *bk, *bv, *bpq, *bpkv, *bp;
  const float *post_ln_g = nullptr, *post_ln_b = nullptr;   // optional LayerNorm on (residual + attention) in the kernel epilogue (not in the blob)
};

struct TrajWs {
  u16 *q16, *k16, *v16, *x16, *o16, *vt16;
  float *q2, *kv2;
};

struct FfnArgs;   // axvs_fused.h
struct OwnQkv;    // axvs_fused.h

// nks = 0: x staged from global (after spatial_attn_kernel); nks > 0: spatial half inside the kernel.  `fa` non-null: the
// layer's FFN rides along (needs nks > 0 and 64-row tiles).
template <bool BF, int T, int MT>
int launch_temporal_n(int nks, const TrajWs& w, const TrajPacked& p, const float* res, float* out, RowMap rm, long long Mp, int N,
                      int L, float scale, hipStream_t st, const FfnArgs* fa, int flags /* bit 0: write-through output rows, bits 1-2: stop after the spatial half / the q,k,v part, bit 3: the regular-tile instantiation (kTrajReg; merged launches on 64-key frames), bits 4-5: 16-bit output map of the FFN-carrying kernel (kOutF16 / kOutBf16) */,
                      const OwnQkv* oq /* non-null: the kernel computes q, k, v of its own rows first (merged launch) */);

}  // namespace axvs
