// What the axial unit (axvs_api.hip) offers its sibling units of the inference C ABI -- the cross-clip modules (axvs_cross_clip.hip)
// and the pixel decoder (axvs_pixdec.hip): the argument checks and the dtype dispatch, the packed-weight / workspace layouts of a
// trajectory attention and an FFN, and plain functions for what stays a template over the operand type inside the axial unit (the
// packers, one planned trajectory attention, the stand-alone FFN, the row LayerNorm).  The planner's FFN and layer plans, the
// options and the status / sync state do not leave axvs_api.hip.
#pragma once
#include <type_traits>

#include "axvs_host.h"
#include "axvs_gemm.h"

namespace axvs {

// The bf16 operand tier sits OUTSIDE the 1e-3 parity bar (2.6e-3 .. 7e-3 against the reference; a bf16 significand has 8 bits) and is not part of the
// default library since round 6: build with -DAXVS_WITH_BF16 to get it (every kernel is a template over the operand type; `kBF` below is the bf16
// arm's template argument, which collapses onto the f16 code -- never reached -- when the tier is not built).
#ifdef AXVS_WITH_BF16
constexpr bool kBF = true;
#else
constexpr bool kBF = false;
#endif
inline int check_dtype(int dtype) {
  if (dtype == AXVS_F16) return AXVS_OK;
  if (dtype == AXVS_BF16) {
    if (kBF) return AXVS_OK;
    return fail(AXVS_ERR_ARG, "the bf16 operand tier is not built into this library (it does not hold the 1e-3 parity bar; fp16 operands run at the same rate and do): rebuild with AXVS_WITH_BF16=1");
  }
  return fail(AXVS_ERR_ARG, "unknown dtype %d", dtype);
}
// f(std::bool_constant<BF>) for the operand type of a dtype that check_dtype has accepted
template <class F>
auto by_dtype(int dtype, F&& f) {
  return dtype == AXVS_BF16 ? f(std::bool_constant<kBF>{}) : f(std::false_type{});
}
// ... and back: the dtype code a template over the operand type hands to the plain functions below
template <bool BF>
constexpr int kDtypeOf = BF ? AXVS_BF16 : AXVS_F16;

inline int check_ffn(int d_ffn) {
  if (d_ffn <= 0 || d_ffn % 32 != 0) return fail(AXVS_ERR_ARG, "d_ffn=%d must be a positive multiple of 32", d_ffn);
  return AXVS_OK;
}

inline int check_cfg(int C, int heads) {
  if (C <= 0 || heads <= 0 || C % heads != 0) return fail(AXVS_ERR_ARG, "C=%d must be a positive multiple of heads=%d", C, heads);
  if (C % 32 != 0) return fail(AXVS_ERR_ARG, "C=%d must be a multiple of 32", C);
  if (C / heads > 32) return fail(AXVS_ERR_ARG, "head_dim=%d > 32 is not supported yet", C / heads);
  return AXVS_OK;
}

inline RowMap identity_map(long long rows) {
  int n = (int)(rows > 0 ? rows : 1);
  return RowMap{n, n, 1, 0, 0, 1, 0};
}

// ---------------- packed weights ----------------
inline TrajPacked carve_traj(Carver& c, int C, int heads) {
  const size_t Cp = (size_t)heads * 32;
  TrajPacked t{};
  t.wq = c.take<u16>(Cp * C);
  t.wk = c.take<u16>(Cp * C);
  t.wv = c.take<u16>(Cp * C);
  t.wpq = c.take<u16>(Cp * Cp);
  t.wpkv = c.take<u16>(2 * Cp * Cp);
  t.wk2t = c.take<u16>(Cp * Cp);
  t.wk2n = c.take<u16>(Cp * Cp);
  t.wv2h = c.take<u16>(Cp * Cp);
  t.wp = c.take<u16>((size_t)C * Cp);
  t.bq = c.take<float>(Cp);
  t.bk = c.take<float>(Cp);
  t.bv = c.take<float>(Cp);
  t.bpq = c.take<float>(Cp);
  t.bpkv = c.take<float>(2 * Cp);
  t.bp = c.take<float>(C);
  return t;
}

struct LayerPacked {
  TrajPacked th, tw;
  u16 *w1, *w2;
  float *b1, *b2, *g1, *be1, *g2, *be2;
};

inline LayerPacked carve_ffn(Carver& c, int C, int F) {   // norm1 / linear1 / linear2 / norm2 only (th, tw unused)
  LayerPacked l{};
  l.w1 = c.take<u16>((size_t)F * C);
  l.w2 = c.take<u16>((size_t)F * C);
  l.b1 = c.take<float>(F);
  l.b2 = c.take<float>(C);
  l.g1 = c.take<float>(C);
  l.be1 = c.take<float>(C);
  l.g2 = c.take<float>(C);
  l.be2 = c.take<float>(C);
  return l;
}

inline LayerPacked carve_layer(Carver& c, int C, int heads, int F) {
  const TrajPacked th = carve_traj(c, C, heads), tw = carve_traj(c, C, heads);
  LayerPacked l = carve_ffn(c, C, F);
  l.th = th;
  l.tw = tw;
  return l;
}

// W [n][k] fp32 -> the 16-bit blocked layout the GEMM kernels read (pack_w3: split precision, hi | lo | hi along K); b -> padded fp32
void pack_w(int dtype, const float* W, u16* out, PackDim nd, PackDim kd, hipStream_t st, int n_off = 0, int n_total = 0);
void pack_w3(int dtype, const float* W, u16* out, PackDim nd, PackDim kd, hipStream_t st, int n_off = 0, int n_total = 0);
void pack_b(const float* b, float* out, PackDim nd, hipStream_t st);
void copy_f32(const float* src, float* dst, int n, hipStream_t st);
void pack_traj(int dtype, const AxvsTrajParams& p, const TrajPacked& t, int C, int heads, hipStream_t st);
void pack_ffn(int dtype, const float* n1w, const float* n1b, const float* l1w, const float* l1b, const float* l2w, const float* l2b,
              const float* n2w, const float* n2b, const LayerPacked& l, int C, int F, hipStream_t st);
// ... from any parameter struct that carries the eight tensors of norm1 / linear1 / linear2 / norm2
template <class P>
void pack_ffn(int dtype, const P& p, const LayerPacked& l, int C, int F, hipStream_t st) {
  pack_ffn(dtype, p.norm1_w, p.norm1_b, p.linear1_w, p.linear1_b, p.linear2_w, p.linear2_b, p.norm2_w, p.norm2_b, l, C, F, st);
}

// ---------------- one trajectory attention over sequence-ordered rows ----------------
// lean: the fully fused tier only round-trips q, k and V^T (x, the T-expanded attention output, stays in LDS)
// rows of the q/k/v row space of `M` token rows in frames of L rows: the fused trajectory tier pads every frame to a multiple of 16
// rows (RowMap, "padded frames"), so that 16-row MFMA tiles never straddle frames
inline int pad16(int L) { return (L + 15) & ~15; }
inline long long padded_rows(long long M, int L) { return L > 0 && L % 16 ? M / L * pad16(L) : M; }

// Mq: capacity of q16 / k16 / vt16 in rows (>= Mp: padded_rows of the longest frame the caller will run)
inline TrajWs carve_traj_ws(Carver& c, long long Mp, int T, int heads, bool lean = false, long long Mq = 0) {
  const size_t Cp = (size_t)heads * 32;
  if (Mq < Mp) Mq = Mp;
  TrajWs w{};
  w.q16 = c.take<u16>(Cp * Mq);
  w.k16 = c.take<u16>(Cp * Mq);
  w.vt16 = c.take<u16>(2 * Cp * Mq);      // block-transposed V (frames padded to a multiple of 32 keys: at most 2x)
  if (lean) return w;
  w.v16 = c.take<u16>(Cp * Mp);
  w.x16 = c.take<u16>(Cp * Mp * T);
  w.o16 = c.take<u16>(Cp * Mp);
  w.q2 = c.take<float>(Cp * Mp);
  // (k2 | v2) of every frame slot, or -- reassociated temporal half, T > 5 -- u and z: [Mp][heads * Cp] fp32 each
  w.kv2 = c.take<float>(((size_t)2 * Cp * T > (size_t)2 * heads * Cp ? (size_t)2 * Cp * T : (size_t)2 * heads * Cp) * Mp);
  return w;
}

// rows the stand-alone FFN works on (x: its input, clobbered by the generic path) + the generic path's scratch
struct FfnWs {
  float *x, *tmp;
  u16 *y16, *h16;
};
inline FfnWs carve_ffn_ws(Carver& c, long long M, int C, int F) {
  FfnWs w{};
  w.x = c.take<float>((size_t)M * C);
  w.tmp = c.take<float>((size_t)M * C);
  w.y16 = c.take<u16>((size_t)M * C);
  w.h16 = c.take<u16>((size_t)M * F);
  return w;
}

// Which kernel form a trajectory pass takes, decided once per call by plan_traj from the shape, the thread's options and the sync
// buffer (axvs_api.hip, "the inference planner")
struct TrajPlan {
  // kFused: spatial half inside the trajectory kernel, x never leaves LDS.  kTemporalFused: spatial_attn_kernel, then the trajectory
  // kernel stages x from global.  kGeneric: GEMMs + row-wise kernels.
  enum Tier { kFused, kTemporalFused, kGeneric } tier;
  enum Qkv { kQkvKernel, kQkvKernel3, kQkvGemms } qkv;   // without a merged launch: qkv_fused_kernel, its (tile, q | k | v) grid, or three GEMMs
  int L;            // frame length in the q/k/v row space: the fused tier pads frames to a multiple of 16 rows (RowMap), the others are dense
  int nks;          // 32-key steps per frame
  int rows;         // rows per tile of the trajectory kernel: 64, 32 or 16 (0: kGeneric)
  int mq;           // merged q/k/v + trajectory launch: 0 = two launches, 1 = merged, 2 = merged and a row tile IS a frame (own K / V^T from registers)
  bool with_ffn;    // the layer's FFN rides in this pass's kernel
  bool reg;         // mq == 2 on regular tiles: whole unpadded 64-key frames, row offsets that fit 32 bits, fp32 output rows -- the kernel's REG
                    // instantiation (clamps, row masks and per-row RowMap divisions compiled out; bit-identical to the generic one)
  bool reassoc;     // kGeneric: the reassociated temporal half
  bool may_merge;   // (input) the caller's sequences may use the registered sync words: one trajectory call at a time per buffer
};
TrajPlan plan_traj(int S, int T, int L, int C, int heads, bool want_attn, bool same_src, int F, bool may_merge);

// One trajectory attention over sequence-ordered rows, by the plan `pl` of plan_traj(S, T, L, ...) for these arguments (no FFN riding).
// q/k/v inputs are fp32 token rows addressed through `rm`; `qk_add` (nullable) is added to the q and k inputs.
// Result (+ bias, + optional residual `res`) goes to fp32 rows of `out` through `rm`.
int run_traj(int dtype, const TrajPlan& pl, const float* qsrc, const float* ksrc, const float* vsrc, const float* qk_add, const float* res,
             float* out, float* attn, const TrajPacked& p, const TrajWs& w, RowMap rm, int S, int T, int L, int C, int heads, hipStream_t st);

// norm1 -> linear1 -> ReLU / GELU -> linear2 -> +residual -> norm2 on the fp32 rows w.x[M][C] (clobbered by the generic path), in the
// form the planner picks for a stand-alone FFN; returns the launch status
int ffn_rows(int dtype, const FfnWs& w, float* out, const LayerPacked& p, long long M, int C, int heads, int d_ffn, hipStream_t st);
// the same as a call of its own on a copy of x (workspace: carve_ffn_ws); p: the FFN part of a packed layer / a packed FFN
int ffn_rows(int dtype, const float* x, float* out, const LayerPacked& p, long long M, int C, int heads, int d_ffn, void* workspace, hipStream_t st);

// Y = LayerNorm(X) over rows of C channels, eps 1e-5: fp32 rows and, when Y16 is non-null, a blocked 16-bit copy
void layernorm_rows(int dtype, const float* X, const float* gamma, const float* beta, float* Y, u16* Y16, long long M, int C, hipStream_t st);

// The one launch_gemm (A loader, epilogue) pair two units share -- the generic FFN's linear1 and Tube-Link's mask_embed: its five
// kernels are instantiated in axvs_api.hip only
extern template void launch_gemm<false, ALoadBlocked<false>, EpiBlocked16<false>>(const ALoadBlocked<false>&, const u16*, const EpiBlocked16<false>&, int, int, int, hipStream_t, int);
#ifdef AXVS_WITH_BF16
extern template void launch_gemm<true, ALoadBlocked<true>, EpiBlocked16<true>>(const ALoadBlocked<true>&, const u16*, const EpiBlocked16<true>&, int, int, int, hipStream_t, int);
#endif

}  // namespace axvs
