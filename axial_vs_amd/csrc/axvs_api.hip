// C-ABI entry points of the axial family (see include/axvs.h: options, status, sync and profile state, the trajectory attention, the
// axial and full-trajectory layers, the FFN, pos3d) and the launch sequences behind them.  What the sibling units of the cross-clip
// modules and the pixel decoder use of this one is declared in axvs_infer.h and defined at the end of the namespace below.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "axvs_infer.h"
#include "axvs_attn.h"
#include "axvs_fused.h"
#include "axvs_ffn_split.h"
#include "axvs_ffn_wide.h"
#include "axvs_misc.h"

namespace axvs {
namespace {

constexpr int kMergeSmall = 128;         // 16-row-tile passes (T <= 4) of at most this many tiles run merged too: -3 % per layer at 128 tiles in a stack with cold weights, +3 % at 256 (profiles/r5_merged_16row_tiles.txt)
// ---- options (axvs_set_option; the comment above it is the list of the 15 keys) ----
thread_local int g_generic_only = 0;     // option "generic_only": 1 = always use the shape-generic v1 kernels
thread_local int* g_status = nullptr;     // axvs_set_status_buffer: word that kernels OR condition bits into (device memory, or pinned host memory)
thread_local volatile int* g_status_host = nullptr;   // the same word when the HOST can read it (pinned host memory): the entry points of the
                                          // axial layer then refuse to run on top of a reported hand-off timeout (status_gate)
thread_local unsigned g_sync_spin_limit = axvs::kSyncSpinLimit;   // option "sync_spin_limit": polls before a hand-off wait gives up (tests shorten it)
thread_local long long g_row_span = 0;   // rows spanned by the layer's row-addressed tensors when their frames are strided (0: natural)
thread_local int g_ffn_wide = 0;         // option "plan_force" bits 2 / 4: 0 = 128-row FFN tiles when they save a round of the chip (ffn_wide_pays), 1 = always, 2 = never
thread_local int g_no_small_tiles = 0;   // option "plan_force" bit 1: never use the 16-row trajectory tiles
thread_local int g_ffn_split_pairs = 1;  // option "plan_force" bit 8 clears it: 65 .. 88 tiles run the chunk-per-workgroup FFN with two chunks per workgroup (0: the one-workgroup-per-tile kernel)
thread_local int g_spatial_only = 0;     // option "spatial_only": 1 = the fused trajectory kernels return after QK^T / softmax / AV (timing only; outputs unwritten);
                                         // 2 = the merged q/k/v + trajectory kernels return after their q/k/v part (the two-launch kernels treat it as 1)
thread_local int g_no_ffn_fusion = 0;    // option "no_ffn_fusion": keep the FFN in its own kernel
thread_local int g_no_reg_tiles = 0;     // option "plan_force" bit 128: never the regular-tile instantiation of the merged trajectory kernels (TrajPlan::reg)
thread_local int g_no_reassoc = 0;       // option "plan_force" bit 64: generic tier computes k2, v2 = proj_kv(x) for every frame slot (the reference's form)
thread_local int g_ffn_gelu = 0;         // option "ffn_gelu": the layer's FFN activation is exact GELU (F.gelu) instead of ReLU -- set by the
                                         // host module around its calls for activation="gelu" (WC/temporal_attention.py:9-17): the FFN then runs on the
                                         // stand-alone fused kernels' GELU instantiation instead of riding in the width-pass kernel
// Merged q/k/v + trajectory launches (temporal_fused_kernel<..., MQ>): one launch per axial pass.  The sibling row tiles of a
// sequence hand K / V^T over inside the launch through arrival counters the CALLER provides (axvs_set_sync_buffer: device words
// that are zero when registered; every launch leaves them zero) -- without a registered buffer the passes run as two launches.
thread_local unsigned* g_sync = nullptr;
thread_local size_t g_sync_words = 0;
thread_local int g_merge_qkv_any = 0;    // option "merge_qkv_any": merged launches at every grid size (A/B; see plan_traj)
thread_local int g_merge_small = kMergeSmall;   // option "plan_force" bits 16 / 32: 0 never, 1 at any size, n > 1: passes of at most n tiles of 16 rows (kMergeSmall)
thread_local int g_out_dtype = 0;        // option "layer_out_dtype": 0 = the layer's output rows are fp32 (the reference's type); 1 / 2 = the kernel that ends the layer
                                         // (norm2 epilogue of the FFN) writes them as f16 / bf16 -- the map a batch-sharded caller gathers over the links
                                         // (BASELINE config 5 is worded "bf16"), written once instead of cast by a second pass
                                         // (options "cc_aspp_affine" and "cc_last_heads_only" are read by the cross-clip unit: axvs_host.h)
thread_local int g_no_merge_qkv = 0;     // option "no_merge_qkv": keep qkv_fused_kernel + trajectory kernel as two launches (A/B, tests)
thread_local int g_no_attn_fusion = 0;   // option "no_attn_fusion": keep spatial_attn_kernel + temporal kernel separate

// ---- planner constants (measured; settable in rounds 2 - 5, fixed since round 6) ----
constexpr int kSmallBelow = 65;          // problems with fewer 64-row tiles than this run the few-rows forms (16-row trajectory tiles, 3-way split q/k/v
                                         // projection, chunk-per-workgroup FFN): their 4x workgroups fit one round of the 256 CUs up to 64 tiles, and from 65 on
                                         // the 64-row forms (merged launch per pass, FFN riding in the width pass) are faster at every T -- round 5 sweep,
                                         // profiles/r5_planner_threshold.txt (128 until then: [1,2,256,48,80] 93.4 -> 79.5 us, [1,5,256,24,40] 94.6 -> 82.8)
constexpr int kMergeMid = 1;             // merged q/k/v + trajectory launch on 32-row tiles (T = 5 .. 8): 1 = while the pass fits one round of the chip, 0 never,
                                         // 2 always: -4 .. -9 % per layer up to 256 tiles, +4 .. +15 % beyond (profiles/r5_merged_32row_tiles.txt)
constexpr int kQkvSplitUpto = 64;        // the stand-alone q/k/v kernel runs one workgroup per (tile, q | k | v) up to this many tiles of 64 rows
// CUs of the current device (the persistent merged launches run one workgroup per CU: their LDS footprint admits no second one)
int cu_count() {
  static thread_local int dev_seen = -1, cus = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (dev != dev_seen) {
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, dev) != hipSuccess) return 0;
    cus = pr.multiProcessorCount;
    dev_seen = dev;
  }
  return cus;
}

// Fail loudly (round 5): a hand-off wait of a merged launch that ran out has set AXVS_STATUS_SYNC_TIMEOUT; that launch's outputs are
// garbage and its arrival counters are left non-zero.  When the status word is host-readable the NEXT call of an axial-layer entry
// point on this thread returns AXVS_ERR_STATE instead of computing on top of it (no synchronisation: the word is read as it is).
int status_gate() {
  if (g_status_host != nullptr && (*g_status_host & AXVS_STATUS_SYNC_TIMEOUT))
    return fail(AXVS_ERR_STATE, "an earlier merged q/k/v + trajectory launch gave up waiting for its sibling row tiles (status bit 2, "
                                "AXVS_STATUS_SYNC_TIMEOUT): its outputs are invalid and its sync words are not zero.  Synchronise, zero the sync words "
                                "(axvs_set_sync_buffer contract), clear the status word, then call again -- or run two launches per pass "
                                "(axvs_set_sync_buffer(NULL, 0) / option no_merge_qkv)");
  return AXVS_OK;
}

// ---------------- packed weights ----------------
template <bool BF>
void pack_w(const float* W, u16* out, PackDim nd, PackDim kd, hipStream_t st, int n_off = 0, int n_total = 0) {
  long long total = (long long)nd.padded * kd.padded;
  hipLaunchKernelGGL((pack_weight_kernel<BF>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, W, out, nd, kd, n_off,
                     n_total ? n_total : nd.padded);
}
template <bool BF>
void pack_w3(const float* W, u16* out, PackDim nd, PackDim kd, hipStream_t st, int n_off = 0, int n_total = 0) {   // split precision
  long long total = (long long)nd.padded * kd.padded;
  hipLaunchKernelGGL((pack_weight_split3_kernel<BF>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, W, out, nd, kd, n_off,
                     n_total ? n_total : nd.padded);
}

template <bool BF>
void pack_ffn(const float* n1w, const float* n1b, const float* l1w, const float* l1b, const float* l2w, const float* l2b,
              const float* n2w, const float* n2b, const LayerPacked& l, int C, int F, hipStream_t st) {
  PackDim plainC{C, C, 0, 0, 0}, plainF{F, F, 0, 0, 0};
  pack_w<BF>(l1w, l.w1, plainF, plainC, st);
  pack_w<BF>(l2w, l.w2, plainC, plainF, st);
  pack_b(l1b, l.b1, plainF, st);
  pack_b(l2b, l.b2, plainC, st);
  pack_b(n1w, l.g1, plainC, st);
  pack_b(n1b, l.be1, plainC, st);
  pack_b(n2w, l.g2, plainC, st);
  pack_b(n2b, l.be2, plainC, st);
}

template <bool BF>
void pack_traj(const AxvsTrajParams& p, const TrajPacked& t, int C, int heads, hipStream_t st) {
  const int d = C / heads, Cp = heads * 32;
  // The kernels store q, k and x (the spatial-attention output) with the 32 channels of a head block in perm32 order
  // (16-byte stores per lane).  q.k is invariant to a common permutation of d; proj_q / proj_kv consume x, so their K
  // columns are packed in the same order.
  PackDim plainC{C, C, 0, 0, 0}, headC{C, Cp, heads, d, 0}, head2C{2 * C, 2 * Cp, heads, d, 0}, headCp{C, Cp, heads, d, 1};
  pack_w<BF>(p.q_w, t.wq, headC, plainC, st);
  pack_w<BF>(p.k_w, t.wk, headC, plainC, st);
  pack_w<BF>(p.v_w, t.wv, headC, plainC, st);
  pack_w<BF>(p.proj_q_w, t.wpq, headC, headCp, st);
  pack_w<BF>(p.proj_kv_w, t.wpkv, head2C, headCp, st);
  if (d == 32) {
    const dim3 pg((unsigned)(((long long)heads * C * 32 + 255) / 256));
    hipLaunchKernelGGL((pack_wk2t_kernel<BF>), pg, dim3(256), 0, st, p.proj_kv_w, t.wk2t, C, heads);
    hipLaunchKernelGGL((pack_wk2n_kernel<BF>), pg, dim3(256), 0, st, p.proj_kv_w, t.wk2n, C, heads);
    hipLaunchKernelGGL((pack_wv2h_kernel<BF>), pg, dim3(256), 0, st, p.proj_kv_w, t.wv2h, C, heads);
  }
  pack_w<BF>(p.proj_w, t.wp, plainC, headC, st);
  pack_b(p.q_b, t.bq, headC, st);
  pack_b(p.k_b, t.bk, headC, st);
  pack_b(p.v_b, t.bv, headC, st);
  pack_b(p.proj_q_b, t.bpq, headC, st);
  pack_b(p.proj_kv_b, t.bpkv, head2C, st);
  pack_b(p.proj_b, t.bp, plainC, st);
}

struct TrajAttnWs {
  TrajWs tw;
  float* zeros;      // [S T L][C]: the residual the fused kernels always add
};
TrajAttnWs carve_traj_attn_ws(Carver& c, int S, int T, int L, int C, int heads) {
  const long long M = (long long)S * T * L;
  TrajAttnWs w{};
  w.tw = carve_traj_ws(c, M, T, heads, false, padded_rows(M, L));
  w.zeros = c.take<float>((size_t)M * C);
  return w;
}
struct TrajLayerWs {
  TrajWs tw;
  FfnWs f;
};
TrajLayerWs carve_traj_layer_ws(Carver& c, int B, int T, int HW, int C, int heads, int F) {
  const long long M = (long long)B * T * HW;
  TrajLayerWs w{};
  w.tw = carve_traj_ws(c, M, T, heads, false, padded_rows(M, HW));
  w.f = carve_ffn_ws(c, M, C, F);
  return w;
}

// ---------------- the inference planner ----------------
// Which kernel form a trajectory pass and an FFN take is decided HERE, once per call: plan_traj / plan_ffn read the shape, the
// thread's options and the sync buffer, and everything else -- the workspace carve, the size queries, the launch sequences -- reads
// the plan.  ("The inference planner", has the measurements behind the thresholds.)
// Frame counts the fused trajectory kernels exist for: T <= 8 (64- / 32-row tiles), and 9 .. 12 on 16-row tiles (x tile T * 8 KiB)
// -- whole-video cross-clip inference with up to 12 clips.  T alone decides, never the number of rows: the fused and the generic
// tier differ at the 16-bit level, and a clip's result must not depend on how many other clips share its batch.
// kFused also needs q, k and v from ONE source, no attention-map output and 8 .. 128 keys per frame (V^T is padded to 32-key steps:
// below 8 keys the padding would more than double the work).  Any axis length: row tiles are cut per sequence, partial key tiles masked.
// F: the FFN that could ride in this pass (0: none).
}  // namespace
TrajPlan plan_traj(int S, int T, int L, int C, int heads, bool want_attn, bool same_src, int F, bool may_merge) {
  TrajPlan p{};
  p.may_merge = may_merge;
  const bool kernels = !g_generic_only && C == 256 && heads == 8;
  const bool few_rows_forms = !g_no_small_tiles;
  p.tier = !(kernels && (T <= 8 || (T <= 12 && few_rows_forms))) ? TrajPlan::kGeneric
           : same_src && !g_no_attn_fusion && !want_attn && L >= 8 && L <= 128 ? TrajPlan::kFused : TrajPlan::kTemporalFused;
  p.L = p.tier == TrajPlan::kFused ? pad16(L) : L;
  p.nks = (p.L + 31) / 32;
  p.reassoc = p.tier == TrajPlan::kGeneric && kernels && !g_no_reassoc && T >= 12;   // (below ~12 frames the per-head GEMMs cost more than they save)
  const int N = T * p.L;
  const long long Mreal = (long long)S * T * L, Mp = (long long)S * N;
  p.qkv = !(kernels && same_src) ? TrajPlan::kQkvGemms : ((Mp + 63) / 64 <= kQkvSplitUpto && few_rows_forms) ? TrajPlan::kQkvKernel3 : TrajPlan::kQkvKernel;
  if (p.tier == TrajPlan::kGeneric) return p;
  // The FFN rides only in a kernel of at least kSmallBelow tiles (counted in REAL rows): with fewer every workgroup's private 1 MB FFN
  // weight stream is pure latency, and a 16-row trajectory kernel + the stand-alone FFN kernel is faster.  (GELU: only the stand-alone
  // FFN kernels carry it.)
  p.with_ffn = p.tier == TrajPlan::kFused && F > 0 && !g_no_ffn_fusion && !g_ffn_gelu && T <= 4 && F % 256 == 0 && F <= 4096 &&
               (Mreal >= (long long)kSmallBelow * 64 || !few_rows_forms);
  // 16-row tiles (4x the workgroups) below kSmallBelow tiles of 64 PADDED rows unless the FFN rides, and for T > 8; else 64 rows for T <= 4, 32 above
  const long long tiles64 = p.tier == TrajPlan::kFused ? (long long)S * ((N + 63) / 64) : (Mp + 63) / 64;
  p.rows = !p.with_ffn && (tiles64 < kSmallBelow || T > 8) && few_rows_forms ? 16 : T <= 4 ? 64 : 32;
  // One launch per pass (the kernel computes q, k, v of its own rows, bit-identical to two launches): the fully fused tier on up to 3 key
  // steps (register budget; 4 on 16-row tiles), T <= 4 or 32-row tiles, K / V^T byte offsets below 4 GiB, one registered arrival counter
  // per sequence -- and a grid small enough that the sibling tiles of a hand-off start together:
  //   64 rows: frames of 64 keys (mq = 2) at every size; other frames up to 640 tiles (option merge_qkv_any: any size)
  //   32 rows: while the pass fits one round of the chip (kMergeMid)
  //   16 rows: up to kMergeSmall tiles (plan_force 16 / 32: never / at any size)
  const bool own_frame = p.rows == 64 && p.L == 64 && T >= 2;
  const auto fits = [&] {
    return p.rows == 64   ? own_frame || tiles64 <= 640 || g_merge_qkv_any
           : p.rows == 32 ? kMergeMid && (kMergeMid == 2 || (long long)S * ((N + 31) / 32) <= cu_count())
                          : g_merge_small && (g_merge_small == 1 || (long long)S * ((N + 15) / 16) <= g_merge_small);
  };
  const bool merge = p.tier == TrajPlan::kFused && may_merge && !g_no_merge_qkv && g_sync != nullptr && (size_t)S <= g_sync_words &&
                     (T <= 4 || p.rows == 32) && p.nks <= (p.rows == 16 ? 4 : 3) && 2 * (long long)heads * 32 * Mp * 2 < (1ll << 32) && fits();
  p.mq = !merge ? 0 : own_frame ? 2 : 1;
  // Regular tiles: the frames are not padded (L is a multiple of 16, so the RowMap's Lv stays 0), every sequence is T whole 64-row tiles (mq = 2),
  // the row-addressed tensors stay below 4 GiB (the write-through rows' 32-bit byte offsets) and the rows leave as fp32.
  p.reg = p.mq == 2 && p.L == L && !g_no_reg_tiles && (g_row_span ? g_row_span : Mp) * 256 * 4 < (1ll << 32) && !(p.with_ffn && g_out_dtype);
  return p;
}
namespace {

// A 128-row FFN tile takes 33 us where a 64-row tile takes 18 (one workgroup per CU; measured stand-alone, tools/ffn_wide_check.py):
// the wide kernel pays when its rounds of the 256-CU chip are so much fewer (21504 rows: 1 x 33 against 2 x 18).
bool ffn_wide_pays(long long M) {
  const long long r64 = ((M + kRows - 1) / kRows + 255) / 256, r128 = ((M + kWideRows - 1) / kWideRows + 255) / 256;
  return r64 > 1 && r128 * 11 < r64 * 6;
}

struct FfnPlan {
  // kSplit1 / kSplit2: one workgroup per (64-row tile, one / two 256-unit chunks of the hidden layer) + a row-wise finishing kernel
  // (axvs_ffn_split.h); kWide: 128-row tiles (axvs_ffn_wide.h); kFused: one workgroup per 64-row tile; kGeneric: LayerNorm / GEMM /
  // GEMM / LayerNorm.  The first four are bit-identical, so the row count may decide between them.
  enum Kind { kSplit2, kSplit1, kWide, kFused, kGeneric } kind;
  int split;        // chunks per workgroup of the split form the SHAPE admits (0: none): what a layer's workspace holds partial outputs for,
                    // also where a 16-bit output map keeps the call itself off that form
  bool gelu;        // exact GELU instead of ReLU
  int oflags;       // kOutF16 / kOutBf16: the norm2 epilogue writes 16-bit rows (0: fp32)
  const char* refuse;   // non-null: no kernel form serves this call
};
// has_part: the caller provides [F/256][M][256] fp32 partial outputs; strided: X and out rows are frames a stride apart (RowStride)
FfnPlan plan_ffn(int C, int heads, int F, long long M, bool has_part, bool strided) {
  FfnPlan p{};
  p.gelu = g_ffn_gelu != 0;
  p.oflags = g_out_dtype ? (g_out_dtype == 1 ? kOutF16 : kOutBf16) : 0;
  const bool kernels = !g_generic_only && C == 256 && heads == 8 && F % 256 == 0 && F <= 4096;
  // few rows (below kSmallBelow tiles): one chunk per workgroup.  Up to 88 tiles: two consecutive chunks -- tiles x F/512 workgroups, still one
  // round of the chip, where one workgroup per tile leaves half the CUs idle behind a private 1 MB stream (-2.4 us at 75 tiles, -0.5 .. -0.9 at
  // 80 .. 84, +0.9 at 96, +4.5 at 128; only reached when the FFN does not ride in the width pass: T >= 5, GELU)
  if (kernels && !g_no_small_tiles && F >= 512)
    p.split = M < (long long)kSmallBelow * 64 ? 1 : (g_ffn_split_pairs && F % 512 == 0 && M <= 88 * 64) ? 2 : 0;
  static_assert(kFfnTiles + (4096 + 5 * 256) * sizeof(float) <= 160 * 1024, "ffn_lds_bytes: every d_ffn the fused FFN kernels take fits the LDS");
  if (!kernels) {
    p.kind = FfnPlan::kGeneric;
    p.refuse = p.oflags ? "layer_out_dtype: a 16-bit output map needs the fused FFN tier (C = 256, 8 heads, d_ffn a multiple of 256 up to 4096)"
               : strided ? "internal: strided frames need the fused FFN kernels" : nullptr;
  } else if (!p.oflags && has_part && p.split) {
    p.kind = p.split == 2 ? FfnPlan::kSplit2 : FfnPlan::kSplit1;
  } else if (!p.oflags && F <= 2048 && (g_ffn_wide == 1 || (g_ffn_wide == 0 && ffn_wide_pays(M)))) {
    p.kind = FfnPlan::kWide;      // more 64-row tiles than CUs: 128-row tiles when that saves a round of the chip
  } else {
    p.kind = FfnPlan::kFused;
  }
  return p;
}

// One axial layer: the height pass, the width pass (the FFN may ride in it) and the FFN.  What the launch sequence touches in the
// workspace is read off the same plans it dispatches on.
struct LayerPlan {
  TrajPlan h, w;
  FfnPlan ffn;
  bool pos_in_kernel;   // positions given as a sine specification are evaluated by the q/k/v kernels (else materialised first)
  bool lean_traj() const { return h.tier == TrajPlan::kFused && w.tier == TrajPlan::kFused; }   // only q, k and V^T round-trip
  bool need_buf2() const { return !w.with_ffn; }                                               // the width pass writes rows for a separate FFN launch
  bool need_ffn_tmp() const { return need_buf2() && ffn.kind == FfnPlan::kGeneric; }           // fp32 scratch + 16-bit y and h
  bool need_ffn_part() const { return need_buf2() && ffn.split != 0; }                          // [F/256][M][256] fp32 partial outputs
};
LayerPlan plan_layer(int B, int T, int H, int W, int C, int heads, int F, bool want_h_attn, bool want_w_attn, bool strided = false) {
  LayerPlan p{};
  p.h = plan_traj(B * W, T, H, C, heads, want_h_attn, true, 0, true);
  p.w = plan_traj(B * H, T, W, C, heads, want_w_attn, true, F, true);
  p.ffn = plan_ffn(C, heads, F, (long long)B * T * H * W, true, strided);
  p.pos_in_kernel = p.h.qkv != TrajPlan::kQkvGemms && p.w.qkv != TrajPlan::kQkvGemms;
  return p;
}

// members the plan does not need are null
struct AxialWs {
  TrajWs tw;
  float *buf1, *buf2;   // height pass -> width pass -> FFN rows; buf1 doubles as the fp32 scratch of the generic FFN path
  u16 *y16, *h16;
  float* ffn_part;
  float* pos;           // materialised sine positions (tiers without in-kernel evaluation)
};
// span: rows spanned by a row-addressed temporary (= M unless the frames are strided)
AxialWs carve_axial_ws(Carver& c, const LayerPlan& plan, bool sine, long long span, int B, int T, int H, int W, int C, int heads, int F) {
  const long long M = (long long)B * T * H * W;
  AxialWs w{};
  w.tw = carve_traj_ws(c, M, T, heads, plan.lean_traj(), std::max(padded_rows(M, H), padded_rows(M, W)));      // q/k/v row space: frames padded to multiples of 16 rows
  w.buf1 = c.take<float>((size_t)span * C);
  if (plan.need_buf2()) w.buf2 = c.take<float>((size_t)span * C);
  if (plan.need_ffn_tmp()) {
    w.y16 = c.take<u16>((size_t)M * C);
    w.h16 = c.take<u16>((size_t)M * F);
  }
  if (plan.need_ffn_part()) w.ffn_part = c.take<float>((size_t)(F / 256) * M * C);
  if (sine && !plan.pos_in_kernel) w.pos = c.take<float>((size_t)M * C);
  return w;
}

template <bool BF, int NKS>
int launch_attn(const TrajWs& w, float* attn, int S, int N, int T, int L, int heads, long long Mp, hipStream_t st) {
  // K and V of a (sequence, head) are staged in LDS, as many frames at a time as fit (whole-video cross-clip inference: T = clips)
  const size_t per_frame = (size_t)NKS * 32 * 32 * 2 * sizeof(u16);
  const int tch = (int)((150 * 1024) / per_frame) < T ? (int)((150 * 1024) / per_frame) : T;
  const size_t lds = per_frame * tch;
  if (int rc = ensure_max_lds(reinterpret_cast<const void*>(&spatial_attn_kernel<BF, NKS>))) return rc;
  const int nwaves = (N + 31) / 32 >= 8 ? 8 : (N + 31) / 32;  // 32 queries per wave, at most 8 waves
  dim3 grid((N + 32 * nwaves - 1) / (32 * nwaves), heads, S);
  hipLaunchKernelGGL((spatial_attn_kernel<BF, NKS>), grid, dim3(64 * nwaves), lds, st, w.q16, w.k16, w.v16, w.x16, attn, N, T, L,
                     heads, Mp, tch);
  return AXVS_OK;
}

// f(std::integral_constant<int, i>{}) for a runtime i in 1 .. N: the template argument of a kernel family
template <int N, class F>
int by_int(int i, F&& f) {
  if constexpr (N == 0) return fail(AXVS_ERR_ARG, "internal: no kernel is instantiated for %d", i);
  else return i == N ? f(std::integral_constant<int, N>{}) : by_int<N - 1>(i, f);
}

// nks = 0: x staged from global (after spatial_attn_kernel); nks > 0: spatial half inside the kernel.  Tile rows: the plan's
// (instantiated: 64 rows for T = 1 .. 4, 32 for 5 .. 8, 16 for 1 .. 12; the x tile takes T * 16 KiB of LDS per 32 rows).
template <bool BF>
int launch_temporal(const TrajPlan& pl, int nks, const TrajWs& w, const TrajPacked& p, const float* res, float* out, RowMap rm, long long Mp, int N,
                    int T, float scale, hipStream_t st, const FfnArgs* fa = nullptr, const OwnQkv* oq = nullptr) {
  // output rows are addressed through the RowMap: the largest byte offset is that of the natural [rows, 256] fp32 tensor
  const int wt = ((g_row_span ? g_row_span : Mp) * 256 * 4 < (1ll << 32) ? 1 : 0) | (g_spatial_only && nks > 0 ? (oq ? g_spatial_only : 1) << 1 : 0) |
                 (fa != nullptr && g_out_dtype ? (g_out_dtype == 1 ? kOutF16 : kOutBf16) : 0) | (pl.reg && oq ? kTrajReg : 0);
  if (oq && !(nks > 0 && T <= 8)) return fail(AXVS_ERR_ARG, "internal: own q,k,v need the in-kernel spatial half and T <= 8");
  return by_int<12>(T, [&](auto t) {
    constexpr int kT = decltype(t)::value;
    if (pl.rows == 16) return launch_temporal_n<BF, kT, 1>(nks, w, p, res, out, rm, Mp, N, pl.L, scale, st, fa, wt, oq);
    if constexpr (kT <= 4) return launch_temporal_n<BF, kT, 4>(nks, w, p, res, out, rm, Mp, N, pl.L, scale, st, fa, wt, oq);
    else if constexpr (kT <= 8) return launch_temporal_n<BF, kT, 2>(nks, w, p, res, out, rm, Mp, N, pl.L, scale, st, fa, wt, oq);
    else return fail(AXVS_ERR_ARG, "fused temporal kernel supports T <= 8");
  });
}

// One trajectory attention over sequence-ordered rows, by the plan `pl` of plan_traj(S, T, L, ...) for these arguments.
// q/k/v inputs are fp32 token rows addressed through `rm`; `qk_add` (nullable) is added to the q and k inputs.
// Result (+ bias, + optional residual `res`) goes to fp32 rows of `out` through `rm`; where the plan lets the layer's FFN ride
// (pl.with_ffn), norm2(FFN(norm1(...))) goes to `ffn_out` instead.
template <bool BF>
int run_traj(const TrajPlan& pl, const float* qsrc, const float* ksrc, const float* vsrc, const float* qk_add, const float* res, float* out,
             float* attn, const TrajPacked& p, const TrajWs& w, RowMap rm, int S, int T, int L, int C, int heads,
             hipStream_t st, int pass = 0, const FfnArgs* ffn = nullptr, float* ffn_out = nullptr, const PosGen* posgen = nullptr) {
  static const char* const kNames[3][9] = {
      {"qkv_proj", "spatial_attn", "proj_q", "proj_kv", "temporal_attn", "proj", "temporal_fused", "traj_fused", "qkv+traj"},
      {"h.qkv_proj", "h.spatial_attn", "h.proj_q", "h.proj_kv", "h.temporal_attn", "h.proj", "h.temporal_fused", "h.traj_fused", "h.qkv+traj"},
      {"w.qkv_proj", "w.spatial_attn", "w.proj_q", "w.proj_kv", "w.temporal_attn", "w.proj", "w.temporal_fused", "w.traj_fused", "w.qkv+traj"}};
  const char* const* nm = kNames[pass];
  if (pl.may_merge)      // never compute on top of a reported hand-off timeout (host-readable status word; no synchronisation)
    if (int rc = status_gate()) return rc;
  const int Cp = heads * 32, d = C / heads;
  if ((long long)S * T * L * T > 2147483647LL / 4) return fail(AXVS_ERR_ARG, "too many tokens for 32-bit row indices");
  const float scale = 1.0f / sqrtf((float)d);
  const float qscale = scale * 1.4426950408889634f;      // q is pre-multiplied by scale * log2(e) for the exp2 softmax
  // The fused tier runs in the PADDED row space (RowMap): frames of roundup16(L) rows, the last ones of each frame clamped copies
  // that are computed and never stored -- every 16-row MFMA tile then lies inside one frame, K / V^T are stored 16 / 8 bytes per lane
  // and the merged launch applies for any frame length (the shipped VIPSeg maps: 49 x 85, 25 x 43).  Every other tier is dense.
  if (pl.L != L) {
    rm.Lv = L;
    rm.L = pl.L;
    rm.N = T * pl.L;
  }
  const int N = T * pl.L;
  const long long Mp = (long long)S * N;
  const int M = (int)Mp;
  const FfnArgs* const fa = pl.with_ffn ? ffn : nullptr;
  float* const dst = pl.with_ffn ? ffn_out : out;
  const PosGen pg = posgen ? *posgen : PosGen{};
  // (a height pass or a stand-alone trajectory attention starts the record afresh; a width pass adds its bit)
  g_reg_passes = pass == 2 ? (g_reg_passes & 1) | (pl.mq && pl.reg ? 2 : 0) : (pl.mq && pl.reg ? 1 : 0);
  if (pl.mq) {      // one launch per pass: the trajectory kernel computes q, k, v of its own rows
    const OwnQkv oq{qsrc, qk_add, pg, p.wq, p.wk, p.wv, p.bq, p.bk, p.bv, qscale, g_sync, g_status, g_sync_spin_limit};
    if (int rc = launch_temporal<BF>(pl, pl.nks, w, p, res, dst, rm, Mp, N, T, scale, st, fa, &oq)) return rc;
    mark(st, pl.with_ffn ? "w.qkv+traj+ffn" : nm[8]);
    return AXVS_OK;
  }
  // q, k, v projections -> blocked 16-bit
  if (pl.qkv == TrajPlan::kQkvGemms) {
    if (posgen) return fail(AXVS_ERR_ARG, "internal: generated positions need the fused QKV kernel");
    ALoadRowsF32<BF> aq{qsrc, qk_add, rm, M, C}, ak{ksrc, qk_add, rm, M, C}, av{vsrc, nullptr, rm, M, C};
    launch_gemm<BF>(aq, p.wq, EpiBlocked16<BF>{w.q16, Mp, p.bq, qscale, Cp, 0}, M, Cp, C, st);
    launch_gemm<BF>(ak, p.wk, EpiBlocked16<BF>{w.k16, Mp, p.bk, 1.f, 0, 0}, M, Cp, C, st);
    launch_gemm<BF>(av, p.wv, EpiBlocked16<BF>{w.v16, Mp, p.bv, 1.f, 0, 0}, M, Cp, C, st);
  } else {
    // the fused kernel reads the value rows from the same tensor as the q/k rows (+ optional additive term); few tiles: one workgroup
    // per (tile, q | k | v) -- a third of the weight stream each.  (It clears the V^T padding keys of frames that are no multiple of 32 keys itself.)
    if (int rc = ensure_max_lds(reinterpret_cast<const void*>(&qkv_fused_kernel<BF>))) return rc;
    hipLaunchKernelGGL((qkv_fused_kernel<BF>), dim3((unsigned)((Mp + 63) / 64), pl.qkv == TrajPlan::kQkvKernel3 ? 3 : 1), dim3(512), kQkvLdsBytes, st, qsrc, qk_add, rm,
                       p.wq, p.wk, p.wv, p.bq, p.bk, p.bv, w.q16, w.k16, w.v16, Mp, qscale,
                       pl.tier == TrajPlan::kFused ? w.vt16 : (u16*)nullptr, N, pl.L, T, pl.nks, pg,
                       2 * (long long)Cp * Mp * 2 < (1ll << 32) ? 1 : 0 /* write-through stores */, g_status);
  }
  mark(st, nm[0]);
  if (pl.tier == TrajPlan::kFused) {
    if (int rc = launch_temporal<BF>(pl, pl.nks, w, p, res, dst, rm, Mp, N, T, scale, st, fa)) return rc;
    mark(st, pl.with_ffn ? "w.traj_fused+ffn" : nm[7]);
    return AXVS_OK;
  }

  // spatial half
  if (pl.nks <= 8) {
    if (int rc = by_int<8>(pl.nks, [&](auto nks) { return launch_attn<BF, decltype(nks)::value>(w, attn, S, N, T, L, heads, Mp, st); })) return rc;
  } else {   // more than 256 keys per frame (full T*H*W trajectory attention): chunked keys, online softmax
    if (attn != nullptr) return fail(AXVS_ERR_ARG, "attention maps are not available for frames of more than 256 keys (L=%d)", L);
    if (int rc = ensure_max_lds(reinterpret_cast<const void*>(&spatial_attn_long_kernel<BF>))) return rc;
    const int nwaves = (N + 31) / 32 >= 8 ? 8 : (N + 31) / 32;
    dim3 grid((N + 32 * nwaves - 1) / (32 * nwaves), heads, S);
    hipLaunchKernelGGL((spatial_attn_long_kernel<BF>), grid, dim3(64 * nwaves), (size_t)2 * 256 * 32 * sizeof(u16), st, w.q16, w.k16, w.v16,
                       w.x16, N, T, L, heads, Mp);
  }
  mark(st, nm[1]);

  // temporal half + output projection + residual
  if (pl.tier == TrajPlan::kTemporalFused) {
    if (int rc = launch_temporal<BF>(pl, 0, w, p, res, out, rm, Mp, N, T, scale, st)) return rc;
    mark(st, nm[6]);
    return AXVS_OK;
  }
  ALoadBlocked<BF> adiag{w.x16, Mp * T, M, T, N, L};
  launch_gemm<BF>(adiag, p.wpq, EpiRowsF32{w.q2, nullptr, p.bpq, identity_map(Mp), Cp, scale}, M, Cp, Cp, st);
  mark(st, nm[2]);
  if (pl.reassoc) {
    // Reassociated (see temporal_fused_kernel): proj_kv is applied to u_h = Wk2_h^T q2_h and z_h = sum_f a_f x_f instead of to
    // every frame slot of x -- 2 C^2 instead of 2 T C^2 MACs per token, and no [T*M, 2C] tensor.  Whole-video cross-clip
    // inference runs T = number of clips (tens): this is what keeps the temporal half linear in T.
    float* U = w.kv2;
    float* Z = w.kv2 + (size_t)Mp * heads * Cp;
    {
      GemmBatch<ALoadRowsLd<BF>, EpiRowsF32, 8> gb;
      for (int h = 0; h < 8; ++h) {
        gb.al[h] = ALoadRowsLd<BF>{w.q2, Cp, h * 32, M};
        gb.W[h] = p.wk2n + (size_t)h * Cp * 32;
        gb.epi[h] = EpiRowsF32{U + h * Cp, nullptr, nullptr, identity_map(Mp), heads * Cp, 1.f};
      }
      launch_gemm_batched<BF>(gb, M, Cp, 32, st);
    }
    hipLaunchKernelGGL((temporal_stream_kernel<BF>), dim3((unsigned)((Mp + 3) / 4)), dim3(256), 0, st, (const float*)U, (const u16*)w.x16, Z,
                       (long long)M, Mp, T);
    mark(st, nm[3]);
    {
      GemmBatch<ALoadRowsLd<BF>, EpiBlocked16<BF>, 8> gb;
      for (int h = 0; h < 8; ++h) {
        gb.al[h] = ALoadRowsLd<BF>{Z, heads * Cp, h * Cp, M};
        gb.W[h] = p.wv2h + (size_t)h * Cp * 32;
        gb.epi[h] = EpiBlocked16<BF>{w.o16, Mp, p.bpkv + Cp + h * 32, 1.f, 0, 0};
        gb.epi[h].n_off = h * 32;
      }
      launch_gemm_batched<BF>(gb, M, 32, Cp, st);
    }
    mark(st, nm[4]);
  } else {
    ALoadBlocked<BF> aall{w.x16, Mp * T, M * T, 0, 1, 1};
    launch_gemm<BF>(aall, p.wpkv, EpiRowsF32{w.kv2, nullptr, p.bpkv, identity_map(Mp * T), 2 * Cp, 1.f}, M * T, 2 * Cp, Cp, st);
    mark(st, nm[3]);
    const long long threads = Mp * heads * 8;
    hipLaunchKernelGGL((temporal_attn_kernel<BF>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, w.q2, w.kv2,
                       w.o16, Mp, T, heads);
    mark(st, nm[4]);
  }
  ALoadBlocked<BF> ao{w.o16, Mp, M, 0, 1, 1};
  launch_gemm<BF>(ao, p.wp, EpiRowsF32{out, res, p.bp, rm, C, 1.f}, M, C, Cp, st);
  mark(st, nm[5]);
  return AXVS_OK;
}

// f(std::bool_constant<GELU>) for the FFN activation (exact GELU or ReLU)
template <class F>
auto by_gelu(bool gelu, F&& f) {
  return gelu ? f(std::true_type{}) : f(std::false_type{});
}

// norm1 -> linear1 -> ReLU / GELU -> linear2 -> +residual -> norm2 on fp32 rows X[M][C] (X is clobbered by the generic path), by the
// plan `pl` of plan_ffn(C, heads, F, M, part != nullptr, rs.hw != 0)
template <bool BF>
int run_ffn(const FfnPlan& pl, float* X, float* out, const LayerPacked& p, long long M, int C, int F, float* tmp, u16* y16, u16* h16,
            hipStream_t st, float* part = nullptr /* [F/256][M][256] fp32 partial outputs of the split forms */,
            RowStride rs = RowStride{0, 0} /* X and out rows: frames of rs.hw rows, rs.hw + rs.extra rows apart (fused kernels only) */) {
  if (pl.refuse) return fail(AXVS_ERR_ARG, "%s", pl.refuse);
  const unsigned tiles = (unsigned)((M + kRows - 1) / kRows);
  switch (pl.kind) {
    case FfnPlan::kSplit2:
    case FfnPlan::kSplit1: {
      const int rc = by_gelu(pl.gelu, [&](auto g) {
        const auto launch = [&](auto cpw) {
          const auto kern = &ffn_split_kernel<BF, decltype(g)::value, decltype(cpw)::value>;
          if (int rc = ensure_max_lds(reinterpret_cast<const void*>(kern))) return rc;
          hipLaunchKernelGGL(kern, dim3(tiles, F / (256 * decltype(cpw)::value)), dim3(512), kFfnSplitLds, st, (const float*)X, p.w1, p.b1, p.w2, p.g1, p.be1, part, M, F, rs);
          return (int)AXVS_OK;
        };
        return pl.kind == FfnPlan::kSplit2 ? launch(std::integral_constant<int, 2>{}) : launch(std::integral_constant<int, 1>{});
      });
      if (rc != AXVS_OK) return rc;
      hipLaunchKernelGGL(ffn_finish_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, (const float*)X, (const float*)part, p.b2, p.g1, p.be1,
                         p.g2, p.be2, out, M, F / 256, rs);
      break;
    }
    case FfnPlan::kWide: {
      const int rc = by_gelu(pl.gelu, [&](auto g) {
        const auto kern = &ffn_wide_kernel<BF, decltype(g)::value>;
        if (int rc = ensure_max_lds(reinterpret_cast<const void*>(kern))) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)((M + kWideRows - 1) / kWideRows)), dim3(512), ffn_wide_lds_bytes(F), st, (const float*)X, p.w1, p.b1, p.w2, p.b2,
                           p.g1, p.be1, p.g2, p.be2, out, M, F, rs);
        return (int)AXVS_OK;
      });
      if (rc != AXVS_OK) return rc;
      break;
    }
    case FfnPlan::kFused: {
      const int rc = by_gelu(pl.gelu, [&](auto g) {
        const auto launch = [&](auto of) {      // the output form is a template argument: the plan's, nothing decided here
          const auto kern = &ffn_fused_kernel<BF, decltype(g)::value, decltype(of)::value>;
          if (int rc = ensure_max_lds(reinterpret_cast<const void*>(kern))) return rc;
          hipLaunchKernelGGL(kern, dim3(tiles), dim3(512), ffn_lds_bytes(F), st, X, p.w1, p.b1, p.w2, p.b2, p.g1, p.be1, p.g2, p.be2, out, M, F, rs);
          return (int)AXVS_OK;
        };
        return pl.oflags == kOutF16 ? launch(std::integral_constant<int, kOutF16>{})
               : pl.oflags == kOutBf16 ? launch(std::integral_constant<int, kOutBf16>{}) : launch(std::integral_constant<int, 0>{});
      });
      if (rc != AXVS_OK) return rc;
      break;
    }
    case FfnPlan::kGeneric: {
      const unsigned lnblocks = (unsigned)((M + 3) / 4);
      hipLaunchKernelGGL((layernorm_kernel<BF>), dim3(lnblocks), dim3(256), 0, st, X, p.g1, p.be1, tmp, y16, M, C, 1e-5f);
      mark(st, "norm1");
      ALoadBlocked<BF> ay{y16, M, (int)M, 0, 1, 1};
      launch_gemm<BF>(ay, p.w1, EpiBlocked16<BF>{h16, M, p.b1, 1.f, 0, pl.gelu ? 2 : 1}, (int)M, F, C, st);
      mark(st, "ffn.linear1");
      ALoadBlocked<BF> ah{h16, M, (int)M, 0, 1, 1};
      launch_gemm<BF>(ah, p.w2, EpiRowsF32{X, tmp, p.b2, identity_map(M), C, 1.f}, (int)M, C, F, st);
      mark(st, "ffn.linear2");
      hipLaunchKernelGGL((layernorm_kernel<BF>), dim3(lnblocks), dim3(256), 0, st, X, p.g2, p.be2, out, (u16*)nullptr, M, C, 1e-5f);
      mark(st, "norm2");
      return AXVS_OK;
    }
  }
  mark(st, "norm1+ffn+norm2");
  return AXVS_OK;
}

template <bool BF>
int traj_attn_fwd_t(const float* query, const float* key, const float* value, float* out, float* attn, const void* packed,
                    int S, int T, int L, int C, int heads, void* ws, hipStream_t st) {
  Carver pc(const_cast<void*>(packed));
  TrajPacked p = carve_traj(pc, C, heads);
  Carver wc(ws);
  const TrajAttnWs w = carve_traj_attn_ws(wc, S, T, L, C, heads);
  // the fused kernels always add a residual: feed zeros here (TrajectoryAttention.forward itself has none)
  if (hipMemsetAsync(w.zeros, 0, (size_t)S * T * L * C * sizeof(float), st) != hipSuccess) return fail(AXVS_ERR_LAUNCH, "memset failed");
  RowMap rm{T * L, L, 1, (long long)T * L, L, 1, 0};
  const TrajPlan plan = plan_traj(S, T, L, C, heads, attn != nullptr, query == key && value == query, 0, false);
  int rc = run_traj<BF>(plan, query, key, value, nullptr, w.zeros, out, attn, p, w.tw, rm, S, T, L, C, heads, st);
  return rc != AXVS_OK ? rc : last_launch_status();
}

PosGen make_posgen(const AxvsSinePos3D& sp, int T, int H, int W, int C, int l_is_h) {
  PosGen pg{};
  pg.mode = 1;
  pg.l_is_h = l_is_h;
  const float eps = 1e-6f;
  pg.zs = sp.normalize ? sp.scale / ((float)T + eps) : 1.f;
  pg.ys = sp.normalize ? sp.scale / ((float)H + eps) : 1.f;
  pg.xs = sp.normalize ? sp.scale / ((float)W + eps) : 1.f;
  pg.n = C / 2;
  pg.ke_yx = -log2f(sp.temperature) * 2.f / (float)pg.n;
  pg.ke_z = -log2f(sp.temperature) * 2.f / (float)C;
  pg.level = sp.level_embed;
  return pg;
}

template <bool BF>
int axial_layer_fwd_t(const float* src, const float* pos, float* out, const void* packed, int B, int T, int H, int W, int C,
                      int heads, int F, void* ws, float* h_attn, float* w_attn, hipStream_t st, const AxvsSinePos3D* sine = nullptr,
                      int which = 0 /* 0: whole layer; 1: height pass only (out = src + height_attn); 2: width pass + norm1 + FFN + norm2 on src */,
                      long long fs = 0 /* > 0: frames of src / out (and of the row-addressed temporaries) are fs rows apart; out may be src */) {
  Carver pc(const_cast<void*>(packed));
  LayerPacked p = carve_layer(pc, C, heads, F);
  const long long M = (long long)B * T * H * W;
  const long long span = fs ? ((long long)B * T - 1) * fs + (long long)H * W : M;      // rows spanned by a row-addressed tensor
  struct SpanGuard { SpanGuard(long long v) { g_row_span = v; } ~SpanGuard() { g_row_span = 0; } } span_guard(fs ? span : 0);
  if (g_out_dtype && (fs != 0 || which == 1))
    return fail(AXVS_ERR_ARG, "layer_out_dtype: a 16-bit output map exists for the whole layer / its width pass on contiguous frames only");
  Carver wc(ws);
  const LayerPlan plan = plan_layer(B, T, H, W, C, heads, F, h_attn != nullptr, w_attn != nullptr, fs != 0);
  const AxialWs w = carve_axial_ws(wc, plan, sine != nullptr, span, B, T, H, W, C, heads, F);
  float* buf1 = w.buf1;
  float* const scratch1 = buf1;                // fp32 scratch of the generic FFN path (free once the width pass has read the rows)
  const long long sB = fs ? (long long)T * fs : (long long)T * H * W, sT = fs ? fs : (long long)H * W;

  g_prof_next = 0;
  mark(st, "begin");
  // positions given as a PositionEmbeddingSine3D specification: the fused QKV kernel evaluates them (no HBM read); the other
  // tiers get them materialised into the workspace first
  PosGen pgh{}, pgw{};
  const PosGen *ph = nullptr, *pw = nullptr;
  if (sine) {
    if (plan.pos_in_kernel) {
      pgh = make_posgen(*sine, T, H, W, C, 1);
      pgw = make_posgen(*sine, T, H, W, C, 0);
      ph = &pgh;
      pw = &pgw;
    } else {
      float* pbuf = w.pos;
      const long long total = (long long)T * H * W * C;
      hipLaunchKernelGGL(pos3d_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, pbuf, B, T, H, W, C, sine->temperature,
                         sine->normalize, sine->scale);
      if (sine->level_embed)
        hipLaunchKernelGGL(add_channel_vector_kernel, dim3((unsigned)(((size_t)M * C + 255) / 256)), dim3(256), 0, st, pbuf, sine->level_embed,
                           (size_t)M * C, C);
      pos = pbuf;
      mark(st, "pos3d");
    }
  }
  // height pass: sequences (b, w), tokens (t, h)        WC/temporal_attention.py:197-204
  RowMap rmh{T * H, H, W, sB, sT, W, 1};
  int rc = AXVS_OK;
  if (which != 2) {
    rc = run_traj<BF>(plan.h, src, src, src, pos, src, which == 1 ? out : buf1, h_attn, p.th, w.tw, rmh, B * W, T, H, C, heads, st, 1, nullptr, nullptr, ph);
    if (rc != AXVS_OK) return rc;
    if (which == 1) return last_launch_status();
  } else {
    buf1 = const_cast<float*>(src);            // the caller's tensor IS the height pass's output (read only below)
  }
  // width pass: sequences (b, h), tokens (t, w)         :206-213
  RowMap rmw{T * W, W, H, sB, sT, 1, W};
  const FfnArgs fa{p.w1, p.w2, p.b1, p.b2, p.g1, p.be1, p.g2, p.be2, F};
  rc = run_traj<BF>(plan.w, buf1, buf1, buf1, pos, buf1, w.buf2, w_attn, p.tw, w.tw, rmw, B * H, T, W, C, heads, st, 2, &fa, out, pw);
  if (rc != AXVS_OK) return rc;
  if (plan.w.with_ffn) return last_launch_status();   // the width-pass kernel ran norm1 -> FFN -> norm2 too and wrote `out`

  // norm1 -> FFN -> norm2                               :181-185, :217-218
  int rc2 = run_ffn<BF>(plan.ffn, w.buf2, out, p, M, C, F, scratch1, w.y16, w.h16, st, w.ffn_part, fs ? RowStride{H * W, fs - (long long)H * W} : RowStride{0, 0});
  if (rc2 != AXVS_OK) return rc2;
  return last_launch_status();
}

// TemporalTrajectoryAttentionLayer (WC/temporal_attention.py:103-155): ONE trajectory attention over all T*H*W tokens of a clip
// (frames of H*W keys), then norm1 -> FFN -> norm2.  Packed blob: TrajPacked | FFN part of LayerPacked.
template <bool BF>
int traj_layer_fwd_t(const float* src, const float* pos, float* out, const void* packed, int B, int T, int HW, int C, int heads, int F,
                     void* ws, hipStream_t st) {
  Carver pc(const_cast<void*>(packed));
  TrajPacked pt = carve_traj(pc, C, heads);
  LayerPacked pf = carve_ffn(pc, C, F);
  const long long M = (long long)B * T * HW;
  Carver wc(ws);
  const TrajLayerWs w = carve_traj_layer_ws(wc, B, T, HW, C, heads, F);
  g_prof_next = 0;
  mark(st, "begin");
  // src [(B T), HW, C] is already the sequence order 'B (T HW) C': identity row map, T frames of HW keys
  RowMap rm{T * HW, HW, 1, (long long)T * HW, HW, 1, 0};
  int rc = run_traj<BF>(plan_traj(B, T, HW, C, heads, false, true, 0, false), src, src, src, pos, src, w.f.x, nullptr, pt, w.tw, rm, B, T, HW, C, heads, st, 0);
  if (rc != AXVS_OK) return rc;
  rc = run_ffn<BF>(plan_ffn(C, heads, F, M, false, false), w.f.x, out, pf, M, C, F, w.f.tmp, w.f.y16, w.f.h16, st);
  return rc != AXVS_OK ? rc : last_launch_status();
}

}  // namespace

// ---------------- axvs_infer.h: this unit's templates over the operand type, as plain functions for the sibling units ----------------
void pack_w(int dtype, const float* W, u16* out, PackDim nd, PackDim kd, hipStream_t st, int n_off, int n_total) {
  by_dtype(dtype, [&](auto bf) { pack_w<bf()>(W, out, nd, kd, st, n_off, n_total); });
}
void pack_w3(int dtype, const float* W, u16* out, PackDim nd, PackDim kd, hipStream_t st, int n_off, int n_total) {
  by_dtype(dtype, [&](auto bf) { pack_w3<bf()>(W, out, nd, kd, st, n_off, n_total); });
}
void pack_b(const float* b, float* out, PackDim nd, hipStream_t st) {
  hipLaunchKernelGGL(pack_bias_kernel, dim3((nd.padded + 255) / 256), dim3(256), 0, st, b, out, nd);
}
void copy_f32(const float* src, float* dst, int n, hipStream_t st) {
  PackDim d{n, n, 0, 0, 0};
  pack_b(src, dst, d, st);
}
void pack_traj(int dtype, const AxvsTrajParams& p, const TrajPacked& t, int C, int heads, hipStream_t st) {
  by_dtype(dtype, [&](auto bf) { pack_traj<bf()>(p, t, C, heads, st); });
}
void pack_ffn(int dtype, const float* n1w, const float* n1b, const float* l1w, const float* l1b, const float* l2w, const float* l2b,
              const float* n2w, const float* n2b, const LayerPacked& l, int C, int F, hipStream_t st) {
  by_dtype(dtype, [&](auto bf) { pack_ffn<bf()>(n1w, n1b, l1w, l1b, l2w, l2b, n2w, n2b, l, C, F, st); });
}
int run_traj(int dtype, const TrajPlan& pl, const float* qsrc, const float* ksrc, const float* vsrc, const float* qk_add, const float* res,
             float* out, float* attn, const TrajPacked& p, const TrajWs& w, RowMap rm, int S, int T, int L, int C, int heads, hipStream_t st) {
  return by_dtype(dtype, [&](auto bf) { return run_traj<bf()>(pl, qsrc, ksrc, vsrc, qk_add, res, out, attn, p, w, rm, S, T, L, C, heads, st); });
}
int ffn_rows(int dtype, const FfnWs& w, float* out, const LayerPacked& p, long long M, int C, int heads, int d_ffn, hipStream_t st) {
  int rc = by_dtype(dtype, [&](auto bf) { return run_ffn<bf()>(plan_ffn(C, heads, d_ffn, M, false, false), w.x, out, p, M, C, d_ffn, w.tmp, w.y16, w.h16, st); });
  return rc != AXVS_OK ? rc : last_launch_status();
}
int ffn_rows(int dtype, const float* x, float* out, const LayerPacked& p, long long M, int C, int heads, int d_ffn, void* workspace, hipStream_t st) {
  Carver wc(workspace);
  const FfnWs w = carve_ffn_ws(wc, M, C, d_ffn);
  if (hipMemcpyAsync(w.x, x, (size_t)M * C * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
    return fail(AXVS_ERR_LAUNCH, "copy failed");
  g_prof_next = 0;
  return ffn_rows(dtype, w, out, p, M, C, heads, d_ffn, st);
}
void layernorm_rows(int dtype, const float* X, const float* gamma, const float* beta, float* Y, u16* Y16, long long M, int C, hipStream_t st) {
  by_dtype(dtype, [&](auto bf) { hipLaunchKernelGGL((layernorm_kernel<bf()>), dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, X, gamma, beta, Y, Y16, M, C, 1e-5f); });
}
template void launch_gemm<false, ALoadBlocked<false>, EpiBlocked16<false>>(const ALoadBlocked<false>&, const u16*, const EpiBlocked16<false>&, int, int, int, hipStream_t, int);
#ifdef AXVS_WITH_BF16
template void launch_gemm<true, ALoadBlocked<true>, EpiBlocked16<true>>(const ALoadBlocked<true>&, const u16*, const EpiBlocked16<true>&, int, int, int, hipStream_t, int);
#endif

}  // namespace axvs

using namespace axvs;

// =====================================================================================
extern "C" {

int axvs_version(void) { return 1; }
int axvs_has_bf16(void) { return kBF ? 1 : 0; }

int axvs_profile_stages(void** events, int capacity) {
  g_prof_events = reinterpret_cast<hipEvent_t*>(events);
  g_prof_cap = events ? capacity : 0;
  return kMaxStages;
}
int axvs_plan_regular_tiles(void) { return g_reg_passes; }
int axvs_profile_stage_count(void) { return g_prof_next < kMaxStages ? g_prof_next : kMaxStages; }
const char* axvs_profile_stage_name(int i) { return (i >= 0 && i < kMaxStages && g_stage_names[i]) ? g_stage_names[i] : ""; }

#if defined(AXVS_STAMPS) && defined(AXVS_STAMPS_QKV)   // the QKV kernel lives in this unit; the trajectory kernels: axvs_temporal_inst.hip
int axvs_debug_read_stamps(unsigned long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(axvs::g_stamps), sizeof(unsigned long long) * n);
}
#endif

// 15 keys.  Functional switches the host modules set around their calls: ffn_gelu, layer_out_dtype, cc_aspp_affine, cc_last_heads_only, train_amp, no_merge_qkv
// (the 'verify' hand-off policy's re-run).  Tier selection for parity tests and the bench's QK^T/AV probe: generic_only, no_attn_fusion, no_ffn_fusion,
// merge_qkv_any, spatial_only, train_valu, train_exact.  Test hooks: sync_spin_limit, and plan_force -- ONE diagnostic bit mask that forces the planner's
// size-dependent choices for the bit-identity tests (forms that are bit-identical by construction, so the row count may decide):
//   1 never the 16-row trajectory tiles | 2 / 4 the 128-row FFN tiles always / never | 8 no two-chunk FFN workgroups | 16 / 32 merged launch on 16-row tiles
//   never / at any size | 64 generic tier without the reassociated temporal half | 128 never the regular-tile instantiation of the merged kernels.
// (Rounds 2 - 5 exposed 37 keys, most of them thresholds and forms measured slower; those are constants / gone since round 6: DESIGN.md.)
int axvs_set_option(const char* key, int value) {
  if (!key) return fail(AXVS_ERR_ARG, "null option key");
  if (!strcmp(key, "generic_only")) { g_generic_only = value; return AXVS_OK; }
  if (!strcmp(key, "no_attn_fusion")) { g_no_attn_fusion = value; return AXVS_OK; }
  if (!strcmp(key, "no_ffn_fusion")) { g_no_ffn_fusion = value; return AXVS_OK; }
  if (!strcmp(key, "ffn_gelu")) { g_ffn_gelu = value; return AXVS_OK; }
  if (!strcmp(key, "train_valu")) { g_train_valu = value; return AXVS_OK; }
  if (!strcmp(key, "train_exact")) { g_train_exact = value; return AXVS_OK; }
  if (!strcmp(key, "train_amp")) {
    if (value < 0 || value > 2) return fail(AXVS_ERR_ARG, "train_amp: 0 (off), 1 (bf16 products) or 2 (fp16 products)");
    g_train_amp = value;
    return AXVS_OK;
  }
  if (!strcmp(key, "spatial_only")) { g_spatial_only = value; return AXVS_OK; }
  if (!strcmp(key, "cc_aspp_affine")) { g_cc_aspp_affine = value ? 1 : 0; return AXVS_OK; }
  if (!strcmp(key, "cc_last_heads_only")) { g_cc_last_only = value; return AXVS_OK; }
  if (!strcmp(key, "no_merge_qkv")) { g_no_merge_qkv = value; return AXVS_OK; }
  if (!strcmp(key, "merge_qkv_any")) { g_merge_qkv_any = value; return AXVS_OK; }
  if (!strcmp(key, "layer_out_dtype")) {
    if (value < 0 || value > 2) return fail(AXVS_ERR_ARG, "layer_out_dtype: 0 (fp32), 1 (f16) or 2 (bf16)");
    g_out_dtype = value;
    return AXVS_OK;
  }
  if (!strcmp(key, "sync_spin_limit")) { g_sync_spin_limit = value > 0 ? (unsigned)value : axvs::kSyncSpinLimit; return AXVS_OK; }
  if (!strcmp(key, "plan_force")) {
    g_no_small_tiles = (value & 1) ? 1 : 0;
    g_ffn_wide = (value & 2) ? 1 : (value & 4) ? 2 : 0;
    g_ffn_split_pairs = (value & 8) ? 0 : 1;
    g_merge_small = (value & 16) ? 0 : (value & 32) ? 1 : kMergeSmall;
    g_no_reassoc = (value & 64) ? 1 : 0;
    g_no_reg_tiles = (value & 128) ? 1 : 0;
    return AXVS_OK;
  }
  return fail(AXVS_ERR_ARG, "unknown option");
}
const char* axvs_last_error(void) { return g_err; }

int axvs_set_status_buffer(int* device_word) {
  g_status = device_word;
  g_status_host = nullptr;
  if (device_word != nullptr) {
    // a word in pinned host memory (hipHostMalloc: device-visible at the same address) can be read by the host without a copy
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, device_word) == hipSuccess && at.type == hipMemoryTypeHost && at.hostPointer != nullptr)
      g_status_host = static_cast<volatile int*>(at.hostPointer);
    else
      (void)hipGetLastError();      // (an unregistered pointer leaves an error behind: not ours to report)
  }
  return AXVS_OK;
}

int axvs_check_status(void) { return status_gate(); }

int axvs_set_sync_buffer(unsigned* device_words, size_t n_words) {
  if (device_words != nullptr && n_words == 0) return fail(AXVS_ERR_ARG, "empty sync buffer");
  g_sync = device_words;
  g_sync_words = device_words ? n_words : 0;
  return AXVS_OK;
}

size_t axvs_traj_packed_bytes(int C, int heads) { return carved([&](Carver& c) { carve_traj(c, C, heads); }); }

int axvs_traj_pack(const AxvsTrajParams* p, void* packed, int C, int heads, int dtype, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!p || !packed) return fail(AXVS_ERR_ARG, "null pointer");
  if (int rc = check_cfg(C, heads)) return rc;
  Carver c(packed);
  TrajPacked t = carve_traj(c, C, heads);
  hipStream_t st = static_cast<hipStream_t>(stream);
  pack_traj(dtype, *p, t, C, heads, st);
  return last_launch_status();
}

size_t axvs_axial_layer_packed_bytes(int C, int heads, int d_ffn) { return carved([&](Carver& c) { carve_layer(c, C, heads, d_ffn); }); }

int axvs_axial_layer_pack(const AxvsAxialLayerParams* p, void* packed, int C, int heads, int d_ffn, int dtype, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!p || !packed) return fail(AXVS_ERR_ARG, "null pointer");
  if (int rc = check_cfg(C, heads)) return rc;
  if (int rc = check_ffn(d_ffn)) return rc;
  Carver c(packed);
  LayerPacked l = carve_layer(c, C, heads, d_ffn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  pack_traj(dtype, p->height_attn, l.th, C, heads, st);
  pack_traj(dtype, p->width_attn, l.tw, C, heads, st);
  pack_ffn(dtype, *p, l, C, d_ffn, st);
  return last_launch_status();
}

size_t axvs_traj_attn_workspace_bytes(int S, int T, int L, int C, int heads) { return carved([&](Carver& c) { carve_traj_attn_ws(c, S, T, L, C, heads); }); }

int axvs_traj_attn_fwd(const float* query, const float* key, const float* value, float* out, float* space_attn,
                       const void* packed, int S, int T, int L, int C, int heads, int dtype, void* workspace,
                       size_t workspace_bytes, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!query || !key || !value || !out || !packed || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (S <= 0 || T <= 0 || L <= 0) return fail(AXVS_ERR_ARG, "empty shape S=%d T=%d L=%d", S, T, L);
  if (int rc = check_cfg(C, heads)) return rc;
  if (int rc = check_ws(workspace_bytes, axvs_traj_attn_workspace_bytes(S, T, L, C, heads))) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return by_dtype(dtype, [&](auto bf) { return traj_attn_fwd_t<bf()>(query, key, value, out, space_attn, packed, S, T, L, C, heads, workspace, st); });
}

static size_t layer_ws_bytes(int B, int T, int H, int W, int C, int heads, int d_ffn, int want_attn_maps, int sine_pos, long long span) {
  return carved([&](Carver& c) { carve_axial_ws(c, plan_layer(B, T, H, W, C, heads, d_ffn, want_attn_maps != 0, want_attn_maps != 0), sine_pos != 0, span, B, T, H, W, C, heads, d_ffn); });
}
size_t axvs_axial_layer_workspace_bytes_ex(int B, int T, int H, int W, int C, int heads, int d_ffn, int want_attn_maps, int sine_pos) {
  return layer_ws_bytes(B, T, H, W, C, heads, d_ffn, want_attn_maps, sine_pos, (long long)B * T * H * W);
}

// frames of src / out `frame_stride_rows` rows apart (a level of the pixel decoder's concatenated token buffer, used in place): the
// row-addressed temporaries take the same stride, i.e. span ((B T - 1) stride + H W) rows each
size_t axvs_axial_layer_workspace_bytes_strided(int B, int T, int H, int W, int C, int heads, int d_ffn, long long frame_stride_rows) {
  return layer_ws_bytes(B, T, H, W, C, heads, d_ffn, 0, 1, ((long long)B * T - 1) * frame_stride_rows + (long long)H * W);
}

int axvs_axial_layer_strided_ok(int C, int heads, int d_ffn) {
  const LayerPlan plan = plan_layer(1, 1, 16, 16, C, heads, d_ffn, false, false, true);      // (neither answer depends on the shape)
  return plan.pos_in_kernel && !plan.ffn.refuse ? 1 : 0;
}

int axvs_axial_layer_fwd_sine3d_strided(const float* src, const AxvsSinePos3D* pos, float* out, const void* packed, int B, int T, int H, int W,
                                        int C, int heads, int d_ffn, int dtype, long long frame_stride_rows, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!src || !pos || !out || !packed || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0) return fail(AXVS_ERR_ARG, "empty shape B=%d T=%d H=%d W=%d", B, T, H, W);
  if (int rc = check_cfg(C, heads)) return rc;
  if (int rc = check_ffn(d_ffn)) return rc;
  if (!axvs_axial_layer_strided_ok(C, heads, d_ffn)) return fail(AXVS_ERR_ARG, "strided frames need the fused tier (C = 256, 8 heads, d_ffn a multiple of 256)");
  if (frame_stride_rows < (long long)H * W) return fail(AXVS_ERR_ARG, "frame stride %lld < H W = %d rows", frame_stride_rows, H * W);
  if (T > 255 || H > 4095 || W > 4095) return fail(AXVS_ERR_ARG, "grid too large for generated positions");
  const long long span = ((long long)B * T - 1) * frame_stride_rows + (long long)H * W;
  if (span > 2147483647LL / 64) return fail(AXVS_ERR_ARG, "too many rows for 32-bit row indices");
  if (int rc = check_ws(workspace_bytes, axvs_axial_layer_workspace_bytes_strided(B, T, H, W, C, heads, d_ffn, frame_stride_rows))) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return by_dtype(dtype, [&](auto bf) { return axial_layer_fwd_t<bf()>(src, nullptr, out, packed, B, T, H, W, C, heads, d_ffn, workspace, nullptr, nullptr, st, pos, 0, frame_stride_rows); });
}

size_t axvs_axial_layer_workspace_bytes(int B, int T, int H, int W, int C, int heads, int d_ffn) {
  return axvs_axial_layer_workspace_bytes_ex(B, T, H, W, C, heads, d_ffn, 1 /* upper bound: with attention maps */, 0);
}

static int axial_layer_entry(const float* src, const float* pos, const AxvsSinePos3D* sine, float* out, const void* packed, int B, int T,
                             int H, int W, int C, int heads, int d_ffn, int dtype, void* workspace, size_t workspace_bytes, float* h_attn,
                             float* w_attn, void* stream) {
  if (!src || (!pos && !sine) || !out || !packed || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0) return fail(AXVS_ERR_ARG, "empty shape B=%d T=%d H=%d W=%d", B, T, H, W);
  if (src == out) return fail(AXVS_ERR_ARG, "out may not alias src");
  if (int rc = check_cfg(C, heads)) return rc;
  if (int rc = check_ffn(d_ffn)) return rc;
  if (sine && (T > 255 || H > 4095 || W > 4095)) return fail(AXVS_ERR_ARG, "grid too large for generated positions");
  if (int rc = check_ws(workspace_bytes, axvs_axial_layer_workspace_bytes_ex(B, T, H, W, C, heads, d_ffn, h_attn != nullptr || w_attn != nullptr, sine != nullptr))) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return by_dtype(dtype, [&](auto bf) { return axial_layer_fwd_t<bf()>(src, pos, out, packed, B, T, H, W, C, heads, d_ffn, workspace, h_attn, w_attn, st, sine); });
}

int axvs_axial_layer_fwd(const float* src, const float* pos, float* out, const void* packed, int B, int T, int H, int W,
                         int C, int heads, int d_ffn, int dtype, void* workspace, size_t workspace_bytes, float* h_attn,
                         float* w_attn, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!pos) return fail(AXVS_ERR_ARG, "null pointer");
  return axial_layer_entry(src, pos, nullptr, out, packed, B, T, H, W, C, heads, d_ffn, dtype, workspace, workspace_bytes, h_attn, w_attn, stream);
}

int axvs_axial_pass_fwd(const float* src, const float* pos, float* out, const void* packed, int pass, int B, int T, int H, int W, int C,
                        int heads, int d_ffn, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!src || !pos || !out || !packed || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (pass != 0 && pass != 1) return fail(AXVS_ERR_ARG, "pass must be 0 (height) or 1 (width + FFN)");
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0) return fail(AXVS_ERR_ARG, "empty shape B=%d T=%d H=%d W=%d", B, T, H, W);
  if (src == out) return fail(AXVS_ERR_ARG, "out may not alias src");
  if (int rc = check_cfg(C, heads)) return rc;
  if (int rc = check_ffn(d_ffn)) return rc;
  if (int rc = check_ws(workspace_bytes, axvs_axial_layer_workspace_bytes_ex(B, T, H, W, C, heads, d_ffn, 0, 0))) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return by_dtype(dtype, [&](auto bf) { return axial_layer_fwd_t<bf()>(src, pos, out, packed, B, T, H, W, C, heads, d_ffn, workspace, nullptr, nullptr, st, nullptr, pass + 1); });
}

size_t axvs_axial_layer_sine3d_workspace_bytes(int B, int T, int H, int W, int C, int heads, int d_ffn) {
  return axvs_axial_layer_workspace_bytes_ex(B, T, H, W, C, heads, d_ffn, 1, 1);
}

int axvs_axial_layer_fwd_sine3d(const float* src, const AxvsSinePos3D* pos, float* out, const void* packed, int B, int T, int H, int W,
                                int C, int heads, int d_ffn, int dtype, void* workspace, size_t workspace_bytes, float* h_attn,
                                float* w_attn, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!pos) return fail(AXVS_ERR_ARG, "null pointer");
  if (!(pos->temperature > 0.f)) return fail(AXVS_ERR_ARG, "temperature must be positive");
  return axial_layer_entry(src, nullptr, pos, out, packed, B, T, H, W, C, heads, d_ffn, dtype, workspace, workspace_bytes, h_attn, w_attn, stream);
}

size_t axvs_traj_layer_packed_bytes(int C, int heads, int d_ffn) { return carved([&](Carver& c) { carve_traj(c, C, heads); carve_ffn(c, C, d_ffn); }); }

int axvs_traj_layer_pack(const AxvsTrajLayerParams* p, void* packed, int C, int heads, int d_ffn, int dtype, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!p || !packed) return fail(AXVS_ERR_ARG, "null pointer");
  if (int rc = check_cfg(C, heads)) return rc;
  if (int rc = check_ffn(d_ffn)) return rc;
  Carver c(packed);
  TrajPacked t = carve_traj(c, C, heads);
  LayerPacked l = carve_ffn(c, C, d_ffn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  pack_traj(dtype, p->temporal_attn, t, C, heads, st);
  pack_ffn(dtype, *p, l, C, d_ffn, st);
  return last_launch_status();
}

size_t axvs_traj_layer_workspace_bytes(int B, int T, int HW, int C, int heads, int d_ffn) { return carved([&](Carver& c) { carve_traj_layer_ws(c, B, T, HW, C, heads, d_ffn); }); }

int axvs_traj_layer_fwd(const float* src, const float* pos, float* out, const void* packed, int B, int T, int HW, int C, int heads, int d_ffn,
                        int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!src || !pos || !out || !packed || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (B <= 0 || T <= 0 || HW <= 0) return fail(AXVS_ERR_ARG, "empty shape B=%d T=%d HW=%d", B, T, HW);
  if (src == out) return fail(AXVS_ERR_ARG, "out may not alias src");
  if (int rc = check_cfg(C, heads)) return rc;
  if (int rc = check_ffn(d_ffn)) return rc;
  if (int rc = check_ws(workspace_bytes, axvs_traj_layer_workspace_bytes(B, T, HW, C, heads, d_ffn))) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return by_dtype(dtype, [&](auto bf) { return traj_layer_fwd_t<bf()>(src, pos, out, packed, B, T, HW, C, heads, d_ffn, workspace, st); });
}

size_t axvs_ffn_workspace_bytes(long long M, int C, int d_ffn) { return carved([&](Carver& c) { carve_ffn_ws(c, M, C, d_ffn); }); }

int axvs_ffn_fwd(const float* x, float* out, const void* packed_layer, long long M, int C, int heads, int d_ffn, int dtype,
                 void* workspace, size_t workspace_bytes, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!x || !out || !packed_layer || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (M <= 0) return fail(AXVS_ERR_ARG, "empty input");
  if (int rc = check_cfg(C, heads)) return rc;
  if (int rc = check_ws(workspace_bytes, axvs_ffn_workspace_bytes(M, C, d_ffn))) return rc;
  Carver pc(const_cast<void*>(packed_layer));
  return ffn_rows(dtype, x, out, carve_layer(pc, C, heads, d_ffn), M, C, heads, d_ffn, workspace, static_cast<hipStream_t>(stream));
}

// (beside pos3d: the layer adds a level embedding to materialised positions with the same kernel)
int axvs_add_channel_vector(float* x, const float* v, size_t n, int C, void* stream) {
  if (!x || !v || C <= 0) return fail(AXVS_ERR_ARG, "bad argument");
  hipLaunchKernelGGL(add_channel_vector_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, v, n, C);
  return last_launch_status();
}

int axvs_pos3d(float* pos, int B, int T, int H, int W, int C, float temperature, int normalize, float scale, void* stream) {
  if (!pos) return fail(AXVS_ERR_ARG, "null pointer");
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 2) return fail(AXVS_ERR_ARG, "bad shape");
  long long total = (long long)T * H * W * C;
  hipLaunchKernelGGL(pos3d_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pos,
                     B, T, H, W, C, temperature, normalize, scale);
  return last_launch_status();
}

int axvs_pos3d_masked(float* pos, const unsigned char* mask, int B, int T, int H, int W, int C, float temperature, int normalize,
                      float scale, void* stream) {
  if (!pos || !mask) return fail(AXVS_ERR_ARG, "null pointer");
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 2) return fail(AXVS_ERR_ARG, "bad shape");
  long long total = (long long)B * T * H * W * C;
  hipLaunchKernelGGL(pos3d_masked_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pos, mask,
                     B, T, H, W, C, temperature, normalize, scale);
  return last_launch_status();
}

}  // extern "C"
