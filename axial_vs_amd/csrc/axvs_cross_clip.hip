// C-ABI entry points of the cross-clip family (include/axvs.h: axvs_cc_*, axvs_tl_cc_module_*, axvs_tl_heads_*) and the launch
// sequences behind them.  The trajectory attention inside a cross-clip layer is the axial unit's (axvs_infer.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "axvs_infer.h"
#include "axvs_cc.h"

using namespace axvs;

namespace {

// ---------------- cross-clip module ----------------
struct CCLayerPacked {
  TrajPacked t;
  u16* aspp_taps;                      // the folded temporal ASPP (axvs_cc.h, pack_aspp_taps_kernel): blocked weights [K = 7 * 256][256]
  float *aspp_bias, *norm_w, *norm_b, *an_w, *an_b, *cn_w, *cn_b;
};
CCLayerPacked carve_cc_layer(Carver& c) {
  CCLayerPacked l;
  l.t = carve_traj(c, 256, 8);
  l.aspp_taps = c.take<u16>(7 * 256 * 256);
  l.aspp_bias = c.take<float>(256);
  l.norm_w = c.take<float>(256); l.norm_b = c.take<float>(256);
  l.an_w = c.take<float>(256); l.an_b = c.take<float>(256);
  l.cn_w = c.take<float>(256); l.cn_b = c.take<float>(256);
  return l;
}
struct CCHeadsPacked {
  u16 *wemb, *wmh;                       // [512,256] (class | mask projection), [128,256]
  float *emb_mul, *emb_add, *mh_mul, *mh_add, *wc, *bc, *wa, *ba, *pix;   // folded BN; class / activation heads fp32; pixel BN (mul, add)
};
CCHeadsPacked carve_cc_heads(Carver& c, int K1) {
  CCHeadsPacked h;
  h.wemb = c.take<u16>(512 * 256);
  h.wmh = c.take<u16>(128 * 256);
  h.emb_mul = c.take<float>(512); h.emb_add = c.take<float>(512);
  h.mh_mul = c.take<float>(128); h.mh_add = c.take<float>(128);
  h.wc = c.take<float>((size_t)K1 * 256); h.bc = c.take<float>(K1);
  h.wa = c.take<float>(256); h.ba = c.take<float>(4);
  h.pix = c.take<float>(4);
  return h;
}
struct CCHeadsWs {
  float* emb;        // [R][512] class | mask embeddings
  u16* kern16;       // blocked [4][R][32] mask kernels
};
CCHeadsWs carve_cc_heads_ws(Carver& c, long long R) {
  CCHeadsWs w;
  w.emb = c.take<float>((size_t)R * 512);
  w.kern16 = c.take<u16>((size_t)R * 128);
  return w;
}
struct CCLayerWs {
  TrajWs tw;
  float *t1, *t2, *y;
};
CCLayerWs carve_cc_layer_ws(Carver& c, long long R, int Tc, int Q) {
  CCLayerWs w;
  w.tw = carve_traj_ws(c, R, Tc, 8, false, padded_rows(R, Q));      // (Tube-Link: 100 queries per clip -> frames of 112 rows)
  w.t1 = c.take<float>((size_t)R * 256);
  w.t2 = c.take<float>((size_t)R * 256);
  w.y = c.take<float>((size_t)R * 256);
  return w;
}

void fold_bn(const AxvsBN& bn, float* mul, float* add, int n, hipStream_t st) {
  hipLaunchKernelGGL(bn_fold_kernel, dim3((n + 255) / 256), dim3(256), 0, st, bn.w, bn.b, bn.mean, bn.var, 1e-3f, mul, add, n);
}

template <bool BF>
int cc_layer_fwd_t(const float* x, float* out, const void* packed, int B, int Q, int Tc, const int* rates, void* ws, hipStream_t st,
                   float* out2 = nullptr /* optional second copy of the output rows */) {
  Carver pc(const_cast<void*>(packed));
  CCLayerPacked p = carve_cc_layer(pc);
  const long long R = (long long)B * Q * Tc;
  Carver wc(ws);
  CCLayerWs w = carve_cc_layer_ws(wc, R, Tc, Q);
  g_prof_next = 0;
  mark(st, "begin");
  // trajectory attention over (t q) tokens of each video, read in place from [B,Q,Tc,C]:  row (b; t,q) -> b*Q*Tc + q*Tc + t
  RowMap rm{Tc * Q, Q, 1, (long long)Q * Tc, 1, Tc, 0};
  const unsigned lnblocks = (unsigned)((R + 3) / 4);
  // the post-norm LayerNorm(x + attn(x)) rides in the trajectory kernel's row-wise epilogue when a fused kernel runs
  const TrajPlan plan = plan_traj(B, Tc, Q, 256, 8, false, true, 0, true);
  const bool ln_in_kernel = plan.tier != TrajPlan::kGeneric;
  if (ln_in_kernel) {
    p.t.post_ln_g = p.norm_w;
    p.t.post_ln_b = p.norm_b;
  }
  int rc = run_traj(kDtypeOf<BF>, plan, x, x, x, nullptr, x, ln_in_kernel ? w.t2 : w.t1, nullptr, p.t, w.tw, rm, B, Tc, Q, 256, 8, st);
  if (rc != AXVS_OK) return rc;
  if (!ln_in_kernel) {
    layernorm_rows(kDtypeOf<BF>, w.t1, p.norm_w, p.norm_b, w.t2, nullptr, R, 256, st);
    mark(st, "cc.norm");
  }
  // temporal ASPP, folded at pack time into ONE linear map of the clip axis (three dilated 3-tap branches + concat + 1x1 projection:
  // CC/maxtron_cross_clip_tracking_module.py:176-201): y[t] = sum_j M_j x[clamp(t + off_j)] + b', 7 taps, K = 1792
  {
    ALoadTaps7<BF> at{w.t2, Tc, (int)R, {0, -rates[0], rates[0], -rates[1], rates[1], -rates[2], rates[2]}};
    launch_gemm<BF>(at, p.aspp_taps, EpiRowsF32{w.y, nullptr, p.aspp_bias, identity_map(R), 256, 1.f}, (int)R, 256, 7 * 256, st, 7);
  }
  mark(st, "cc.aspp");
  hipLaunchKernelGGL(cc_aspp_post_kernel, dim3(lnblocks), dim3(256), 0, st, w.y, w.t2, p.an_w, p.an_b, p.cn_w, p.cn_b, out, R, out2, g_cc_aspp_affine);
  mark(st, "cc.aspp_post");
  return last_launch_status();
}

// embeddings + mask-head kernels (-> kern16, blocked [4][R][32]) + class head; the mask einsum follows separately so that the
// module loop can run it once for all layers
// x: the clip queries of `nl` layers back to back ([nl][R][256]); the projections share their weights across layers, so all layers
// go through ONE launch per GEMM (kern16: blocked [4][nl*R][32], logits [nl][Q][K1])
template <bool BF>
int cc_heads_small_t(const float* x, float* logits, u16* kern16, const void* packed, int B, int Q, int Tc, int K1, float* emb, hipStream_t st,
                     int nl = 1) {
  Carver pc(const_cast<void*>(packed));
  CCHeadsPacked p = carve_cc_heads(pc, K1);
  const long long R = (long long)nl * B * Q * Tc;
  ALoadRowsLd<BF> ax{x, 256, 0, (int)R};
  EpiRowsF32 ee{emb, nullptr, p.emb_add, identity_map(R), 512, 1.f};
  ee.mul = p.emb_mul;
  ee.gelu = 1;
  launch_gemm<BF>(ax, p.wemb, ee, (int)R, 512, 256, st);
  ALoadRowsLd<BF> am{emb, 512, 256, (int)R};
  EpiBlocked16<BF> ek{kern16, R, p.mh_add, 1.f, 0, 0};
  ek.mul = p.mh_mul;
  launch_gemm<BF>(am, p.wmh, ek, (int)R, 128, 256, st);
  mark(st, "cc.embeddings");
  const float void_bias = logf((float)(K1 - 1) * 0.9f / (1.f - 0.9f));
  hipLaunchKernelGGL(cc_class_head_kernel, dim3(Q, nl), dim3(256), 0, st, emb, 512, p.wa, p.ba, p.wc, p.bc, logits, B, Q, Tc, K1, void_bias);
  mark(st, "cc.class_head");
  return AXVS_OK;
}

// The mask einsum of both modules: masks of `nl` layers (kernels kstride apart, outputs ostride apart) from one pass over `frames`
// feature maps of P pixels, CK mask-kernel channels.  Every stride of the map is a multiple of P: the pixel rows are as aligned as P
// (and the two base pointers) allow, and rows that are not 16-byte aligned take the kernel's generic form.
template <bool BF, int CK>
int mask_einsum(int frames, const float* feat, const u16* kern16, float* masks, int Q, int Tc, long long P, long long R, const EinsumMap& mp,
                const float* pix, int nl, long long kstride, long long ostride, hipStream_t st) {
  const dim3 grid((unsigned)((P + kEinsumPx - 1) / kEinsumPx), frames);
  const int al = std::min(row_align(feat, P, P), row_align(masks, P, P));
  const auto launch = [&](auto gen) {
    const auto kern = &mask_einsum_kernel<BF, CK, decltype(gen)::value>;
    if (int rc = ensure_max_lds(reinterpret_cast<const void*>(kern))) return rc;
    hipLaunchKernelGGL(kern, grid, dim3(256), einsum_lds_bytes<CK>(), st, feat, kern16, masks, Q, Tc, P, R, mp, pix, nl, kstride, ostride, al);
    return (int)AXVS_OK;
  };
  return al == 4 && P % 4 == 0 ? launch(std::false_type{}) : launch(std::true_type{});
}

template <bool BF>
int cc_masks_t(const float* pf, const u16* kern16, float* masks, const void* packed, int B, int Q, int Tc, int V, int H, int W, int K1, int nl,
               long long kstride, long long ostride, hipStream_t st) {
  Carver pc(const_cast<void*>(packed));
  CCHeadsPacked p = carve_cc_heads(pc, K1);
  const long long R = (long long)nl * B * Q * Tc, P = (long long)V * H * W;      // rows of the blocked kernel matrix: all layers
  const long long TP = (long long)Tc * P;
  const EinsumMap mp{128 * TP, P, TP, (long long)Q * TP, P, TP, Tc, 1};
  if (int rc = mask_einsum<BF, 128>(B * Tc, pf, kern16, masks, Q, Tc, P, R, mp, p.pix, nl, kstride, ostride, st)) return rc;
  mark(st, "cc.mask_einsum");
  return AXVS_OK;
}

template <bool BF>
int cc_heads_fwd_t(const float* x, const float* pf, float* logits, float* masks, const void* packed, int B, int Q, int Tc, int V, int H,
                   int W, int K1, void* ws, hipStream_t st) {
  const long long R = (long long)B * Q * Tc;
  Carver wc(ws);
  const CCHeadsWs w = carve_cc_heads_ws(wc, R);
  g_prof_next = 0;
  mark(st, "begin");
  cc_heads_small_t<BF>(x, logits, w.kern16, packed, B, Q, Tc, K1, w.emb, st);
  cc_masks_t<BF>(pf, w.kern16, masks, packed, B, Q, Tc, V, H, W, K1, 1, 0, 0, st);
  return last_launch_status();
}

// ---------------- Tube-Link cross-clip heads ----------------
struct TLHeadsPacked {
  u16 *w0, *w1, *w2;                                     // mask_embed MLP [256,256], [256,256], [Cm,256]
  float *b0, *b1, *b2, *pn_w, *pn_b, *wa, *ba, *wc, *bc;  // biases, post_norm, activation_proj, cls_embed (fp32)
};
TLHeadsPacked carve_tl_heads(Carver& c, int K1, int Cm) {
  TLHeadsPacked h;
  h.w0 = c.take<u16>(256 * 256); h.w1 = c.take<u16>(256 * 256); h.w2 = c.take<u16>((size_t)Cm * 256);
  h.b0 = c.take<float>(256); h.b1 = c.take<float>(256); h.b2 = c.take<float>(Cm);
  h.pn_w = c.take<float>(256); h.pn_b = c.take<float>(256);
  h.wa = c.take<float>(256); h.ba = c.take<float>(1);
  h.wc = c.take<float>((size_t)K1 * 256); h.bc = c.take<float>(K1);
  return h;
}

struct TLHeadsWs {
  float* xn;
  u16 *xn16, *h1, *h2;
};
TLHeadsWs carve_tl_heads_ws(Carver& c, long long R) {
  TLHeadsWs w;
  w.xn = c.take<float>((size_t)R * 256);
  w.xn16 = c.take<u16>((size_t)R * 256);
  w.h1 = c.take<u16>((size_t)R * 256);
  w.h2 = c.take<u16>((size_t)R * 256);
  return w;
}
struct TLHeadsFwdWs {      // the stand-alone heads call: + the mask kernels (the modules keep theirs in ModuleWs::kern)
  TLHeadsWs hw;
  u16* kern16;
};
TLHeadsFwdWs carve_tl_heads_fwd_ws(Carver& c, long long R, int Cm) {
  TLHeadsFwdWs w;
  w.hw = carve_tl_heads_ws(c, R);
  w.kern16 = c.take<u16>((size_t)R * Cm);
  return w;
}

template <bool BF>
int tl_heads_small_t(const float* x, float* logits, u16* kern16, const void* packed, int B, int Q, int Tc, int K1, int Cm, const TLHeadsWs& w,
                     hipStream_t st, int nl = 1) {
  Carver pc(const_cast<void*>(packed));
  TLHeadsPacked p = carve_tl_heads(pc, K1, Cm);
  const long long R = (long long)nl * B * Q * Tc;
  layernorm_rows(kDtypeOf<BF>, x, p.pn_w, p.pn_b, w.xn, w.xn16, R, 256, st);
  mark(st, "tl.post_norm");
  hipLaunchKernelGGL(tl_class_head_kernel, dim3((unsigned)(B * Q), nl), dim3(256), 0, st, w.xn, p.wa, p.ba, p.wc, p.bc, logits, Tc, K1);
  mark(st, "tl.class_head");
  launch_gemm<BF>(ALoadBlocked<BF>{w.xn16, R, (int)R, 0, 1, 1}, p.w0, EpiBlocked16<BF>{w.h1, R, p.b0, 1.f, 0, 1}, (int)R, 256, 256, st);
  launch_gemm<BF>(ALoadBlocked<BF>{w.h1, R, (int)R, 0, 1, 1}, p.w1, EpiBlocked16<BF>{w.h2, R, p.b1, 1.f, 0, 1}, (int)R, 256, 256, st);
  launch_gemm<BF>(ALoadBlocked<BF>{w.h2, R, (int)R, 0, 1, 1}, p.w2, EpiBlocked16<BF>{kern16, R, p.b2, 1.f, 0, 0}, (int)R, Cm, 256, st);
  mark(st, "tl.mask_embed");
  return AXVS_OK;
}

template <bool BF>
int tl_masks_t(const float* mf, const u16* kern16, float* masks, int B, int Q, int Tc, int fpc, int h, int w, int Cm, int nl, long long kstride,
               long long ostride, hipStream_t st) {
  const long long R = (long long)nl * B * Q * Tc, P = (long long)h * w;
  const int T = Tc * fpc;
  const EinsumMap mp{(long long)T * Cm * P, (long long)Cm * P, P, (long long)T * Q * P, (long long)Q * P, P, T, fpc};
  if (int rc = Cm == 128 ? mask_einsum<BF, 128>(B * T, mf, kern16, masks, Q, Tc, P, R, mp, nullptr, nl, kstride, ostride, st)
                         : mask_einsum<BF, 256>(B * T, mf, kern16, masks, Q, Tc, P, R, mp, nullptr, nl, kstride, ostride, st))
    return rc;
  mark(st, "tl.mask_einsum");
  return AXVS_OK;
}

template <bool BF>
int tl_heads_fwd_t(const float* x, const float* mf, float* logits, float* masks, const void* packed, int B, int Q, int Tc, int fpc,
                   int h, int w, int K1, int Cm, void* ws, hipStream_t st) {
  const long long R = (long long)B * Q * Tc;
  Carver wc(ws);
  const TLHeadsFwdWs s = carve_tl_heads_fwd_ws(wc, R, Cm);
  g_prof_next = 0;
  mark(st, "begin");
  tl_heads_small_t<BF>(x, logits, s.kern16, packed, B, Q, Tc, K1, Cm, s.hw, st);
  tl_masks_t<BF>(mf, s.kern16, masks, B, Q, Tc, fpc, h, w, Cm, 1, 0, 0, st);
  return last_launch_status();
}

struct ModuleWs {
  void *chain, *heads;
  float* q;            // [layers][R][256] clip queries after every layer: the predictor heads run on all of them at once
  u16* kern;           // blocked [Cm/32][layers*R][32] mask kernels of every layer
};
ModuleWs carve_module_ws(Carver& c, size_t chain_bytes, size_t heads_bytes, long long R, int layers, int Cm) {
  ModuleWs m;
  m.chain = c.take<char>(chain_bytes);
  m.heads = c.take<char>(heads_bytes);
  m.q = c.take<float>((size_t)layers * R * 256);
  m.kern = c.take<u16>((size_t)layers * R * Cm);
  return m;
}

// The layer chain (trajectory attention -> ASPP -> norms) of layer i+1 only needs layer i's clip queries, not its predictions, and
// the predictor heads share their weights across layers: the chain runs first, then heads(stream) computes the class logits and
// mask kernels of ALL layers (one launch per GEMM over layers*R rows) and the mask einsum of all layers in one pass over the pixel
// features (read once instead of once per layer).
template <class Heads>
int run_cc_module(const float* clip_query, const void* const* packed_layers, int layers, float* last_query, int B, int Q, int Tc, const int* rates,
                  int dtype, const ModuleWs& w, hipStream_t st, Heads heads) {
  const long long R = (long long)B * Q * Tc;
  if (layers <= 0 || layers > 64) return fail(AXVS_ERR_ARG, "num_layers=%d must be in 1..64", layers);
  const float* cur = clip_query;
  for (int i = 0; i < layers; ++i) {
    float* nxt = w.q + (size_t)i * R * 256;
    float* also = i == layers - 1 ? last_query : nullptr;      // the caller's copy of the last layer's queries
    int rc = by_dtype(dtype, [&](auto bf) { return cc_layer_fwd_t<bf()>(cur, nxt, packed_layers[i], B, Q, Tc, rates, w.chain, st, also); });
    if (rc != AXVS_OK) return rc;
    cur = nxt;
  }
  if (int rc = heads(st)) return rc;
  return last_launch_status();
}
}  // namespace

extern "C" {

size_t axvs_cc_layer_packed_bytes(void) { return carved([&](Carver& c) { carve_cc_layer(c); }); }

int axvs_cc_layer_pack(const AxvsCCLayerParams* p, void* packed, int dtype, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!p || !packed) return fail(AXVS_ERR_ARG, "null pointer");
  Carver c(packed);
  CCLayerPacked l = carve_cc_layer(c);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned cb = (7 * 256 * 256 + 255) / 256;
  pack_traj(dtype, p->attn, l.t, 256, 8, st);
  by_dtype(dtype, [&](auto bf) {
    hipLaunchKernelGGL((pack_aspp_taps_kernel<bf()>), dim3(cb), dim3(256), 0, st, p->aspp_w[0], p->aspp_w[1], p->aspp_w[2], p->aspp_proj_w, l.aspp_taps);
  });
  hipLaunchKernelGGL(pack_aspp_bias_kernel, dim3(1), dim3(256), 0, st, p->aspp_b[0], p->aspp_b[1], p->aspp_b[2], p->aspp_proj_w, l.aspp_bias);
  copy_f32(p->norm_w, l.norm_w, 256, st); copy_f32(p->norm_b, l.norm_b, 256, st);
  copy_f32(p->aspp_norm_w, l.an_w, 256, st); copy_f32(p->aspp_norm_b, l.an_b, 256, st);
  copy_f32(p->conv_norm_w, l.cn_w, 256, st); copy_f32(p->conv_norm_b, l.cn_b, 256, st);
  return last_launch_status();
}

size_t axvs_cc_layer_workspace_bytes(int B, int Q, int Tc) { return carved([&](Carver& c) { carve_cc_layer_ws(c, (long long)B * Q * Tc, Tc, Q); }); }

int axvs_cc_layer_fwd(const float* clip_query, float* out, const void* packed, int B, int Q, int Tc, const int* rates, int dtype,
                      void* workspace, size_t workspace_bytes, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!clip_query || !out || !packed || !rates || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (B <= 0 || Q <= 0 || Tc <= 0) return fail(AXVS_ERR_ARG, "empty shape");
  if (clip_query == out) return fail(AXVS_ERR_ARG, "out may not alias clip_query");
  if (int rc = check_ws(workspace_bytes, axvs_cc_layer_workspace_bytes(B, Q, Tc))) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return by_dtype(dtype, [&](auto bf) { return cc_layer_fwd_t<bf()>(clip_query, out, packed, B, Q, Tc, rates, workspace, st); });
}

size_t axvs_cc_heads_packed_bytes(int K1) { return carved([&](Carver& c) { carve_cc_heads(c, K1); }); }

int axvs_cc_heads_pack(const AxvsCCHeadParams* p, void* packed, int K1, int dtype, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!p || !packed || K1 <= 0) return fail(AXVS_ERR_ARG, "bad argument");
  Carver c(packed);
  CCHeadsPacked h = carve_cc_heads(c, K1);
  hipStream_t st = static_cast<hipStream_t>(stream);
  PackDim n256{256, 256, 0, 0, 0}, n128{128, 128, 0, 0, 0};
  pack_w(dtype, p->class_proj_w, h.wemb, n256, n256, st, 0, 512);
  pack_w(dtype, p->mask_proj_w, h.wemb, n256, n256, st, 256, 512);
  pack_w(dtype, p->mask_head_w, h.wmh, n128, n256, st);
  fold_bn(p->class_proj_bn, h.emb_mul, h.emb_add, 256, st);
  fold_bn(p->mask_proj_bn, h.emb_mul + 256, h.emb_add + 256, 256, st);
  fold_bn(p->mask_head_bn, h.mh_mul, h.mh_add, 128, st);
  fold_bn(p->pixel_bn, h.pix, h.pix + 1, 1, st);
  hipLaunchKernelGGL(transpose_k1x256_kernel, dim3((unsigned)((K1 * 256 + 255) / 256)), dim3(256), 0, st, p->class_head_w, h.wc, K1);      // [256][K1]: class index on the lanes
  copy_f32(p->class_head_b, h.bc, K1, st);
  copy_f32(p->act_head_w, h.wa, 256, st);
  copy_f32(p->act_head_b, h.ba, 1, st);
  return last_launch_status();
}

size_t axvs_cc_heads_workspace_bytes(int B, int Q, int Tc) { return carved([&](Carver& c) { carve_cc_heads_ws(c, (long long)B * Q * Tc); }); }

int axvs_cc_heads_fwd(const float* clip_query, const float* panoptic_features, float* pred_logits, float* pred_masks,
                      const void* packed, int B, int Q, int Tc, int V, int H, int W, int K1, int dtype, void* workspace,
                      size_t workspace_bytes, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!clip_query || !panoptic_features || !pred_logits || !pred_masks || !packed || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (B <= 0 || Q <= 0 || Tc <= 0 || V <= 0 || H <= 0 || W <= 0 || K1 <= 0) return fail(AXVS_ERR_ARG, "empty shape");
  if (B * Tc > 1024) return fail(AXVS_ERR_ARG, "B*Tc > 1024 is not supported by the class head");
  if (int rc = check_ws(workspace_bytes, axvs_cc_heads_workspace_bytes(B, Q, Tc))) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return by_dtype(dtype, [&](auto bf) { return cc_heads_fwd_t<bf()>(clip_query, panoptic_features, pred_logits, pred_masks, packed, B, Q, Tc, V, H, W, K1, workspace, st); });
}

// ---- the whole layer loop of the cross-clip modules in ONE call (CC/...:283-318, TLCC:925-950): the Python host of round 1 made
//      2 library calls + 3 allocations per layer and became the bottleneck once the kernels were fused (494 us of host time per
//      forward against ~430 us of GPU time at BASELINE config 4).  The layer chain (trajectory attention -> ASPP -> norms) of layer
//      i+1 only needs layer i's clip queries, not its predictions: with an auxiliary stream the predictor heads of layer i run
//      beside the chain of layer i+1 (fork / join with events, capturable into a HIP graph).
size_t axvs_cc_module_workspace_bytes(int B, int Q, int Tc, int num_layers) {
  return carved([&](Carver& c) { carve_module_ws(c, axvs_cc_layer_workspace_bytes(B, Q, Tc), (size_t)num_layers * B * Q * Tc * 512 * sizeof(float), (long long)B * Q * Tc, num_layers, 128); });
}

int axvs_cc_module_fwd(const float* clip_query, const float* panoptic_features, float* pred_logits, float* pred_masks, float* last_query,
                       const void* const* packed_layers, const void* packed_heads, int num_layers, int B, int Q, int Tc, int V, int H, int W,
                       int K1, const int* rates, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!clip_query || !panoptic_features || !pred_logits || !pred_masks || !last_query || !packed_layers || !packed_heads || !rates || !workspace)
    return fail(AXVS_ERR_ARG, "null pointer");
  if (B <= 0 || Q <= 0 || Tc <= 0 || V <= 0 || H <= 0 || W <= 0 || K1 <= 0 || num_layers <= 0) return fail(AXVS_ERR_ARG, "empty shape");
  if (B * Tc > 1024) return fail(AXVS_ERR_ARG, "B*Tc > 1024 is not supported by the class head");
  if (int rc = check_ws(workspace_bytes, axvs_cc_module_workspace_bytes(B, Q, Tc, num_layers))) return rc;
  const long long R = (long long)B * Q * Tc;
  Carver wc(workspace);
  const ModuleWs w = carve_module_ws(wc, axvs_cc_layer_workspace_bytes(B, Q, Tc), (size_t)num_layers * R * 512 * sizeof(float), R, num_layers, 128);
  const long long mstride = (long long)B * Q * Tc * V * H * W;
  g_prof_next = 0;
  // heads of all layers (the reference's return value), or of the last one only (option "cc_last_heads_only": outputs hold one layer)
  const int hl = g_cc_last_only ? 1 : num_layers;
  const float* hq = w.q + (size_t)(num_layers - hl) * R * 256;
  auto heads = [&](hipStream_t hs) {
    float* emb = static_cast<float*>(w.heads);
    return by_dtype(dtype, [&](auto bf) {
      cc_heads_small_t<bf()>(hq, pred_logits, w.kern, packed_heads, B, Q, Tc, K1, emb, hs, hl);
      return cc_masks_t<bf()>(panoptic_features, w.kern, pred_masks, packed_heads, B, Q, Tc, V, H, W, K1, hl, R * 32, mstride, hs);
    });
  };
  return run_cc_module(clip_query, packed_layers, num_layers, last_query, B, Q, Tc, rates, dtype, w, static_cast<hipStream_t>(stream), heads);
}

size_t axvs_tl_cc_module_workspace_bytes(int B, int Q, int Tc, int Cm, int num_layers) {
  const size_t heads = carved([&](Carver& c) { carve_tl_heads_ws(c, (long long)num_layers * B * Q * Tc); });
  return carved([&](Carver& c) { carve_module_ws(c, axvs_cc_layer_workspace_bytes(B, Q, Tc), heads, (long long)B * Q * Tc, num_layers, Cm); });
}

int axvs_tl_cc_module_fwd(const float* clip_query, const float* mask_feature, float* cls_logits, float* mask_logits, float* last_query,
                          const void* const* packed_layers, const void* packed_heads, int num_layers, int B, int Q, int Tc, int frames_per_clip,
                          int h, int w_, int K1, int Cm, const int* rates, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!clip_query || !mask_feature || !cls_logits || !mask_logits || !last_query || !packed_layers || !packed_heads || !rates || !workspace)
    return fail(AXVS_ERR_ARG, "null pointer");
  if (B <= 0 || Q <= 0 || Tc <= 0 || frames_per_clip <= 0 || h <= 0 || w_ <= 0 || K1 <= 0 || num_layers <= 0) return fail(AXVS_ERR_ARG, "empty shape");
  if (Cm != 128 && Cm != 256) return fail(AXVS_ERR_ARG, "mask feature channels must be 128 or 256 (got %d)", Cm);
  if (Tc > 1024) return fail(AXVS_ERR_ARG, "more than 1024 clips are not supported by the class head");
  if (int rc = check_ws(workspace_bytes, axvs_tl_cc_module_workspace_bytes(B, Q, Tc, Cm, num_layers))) return rc;
  const long long R = (long long)B * Q * Tc;
  const size_t heads_bytes = carved([&](Carver& c) { carve_tl_heads_ws(c, (long long)num_layers * R); });
  Carver wc(workspace);
  const ModuleWs w = carve_module_ws(wc, axvs_cc_layer_workspace_bytes(B, Q, Tc), heads_bytes, R, num_layers, Cm);
  const long long mstride = (long long)B * Tc * frames_per_clip * Q * h * w_;
  g_prof_next = 0;
  auto heads = [&](hipStream_t hs) {
    Carver hc(w.heads);
    const TLHeadsWs hw = carve_tl_heads_ws(hc, (long long)num_layers * R);
    return by_dtype(dtype, [&](auto bf) {
      tl_heads_small_t<bf()>(w.q, cls_logits, w.kern, packed_heads, B, Q, Tc, K1, Cm, hw, hs, num_layers);
      return tl_masks_t<bf()>(mask_feature, w.kern, mask_logits, B, Q, Tc, frames_per_clip, h, w_, Cm, num_layers, R * 32, mstride, hs);
    });
  };
  return run_cc_module(clip_query, packed_layers, num_layers, last_query, B, Q, Tc, rates, dtype, w, static_cast<hipStream_t>(stream), heads);
}

size_t axvs_tl_heads_packed_bytes(int K1, int Cm) { return carved([&](Carver& c) { carve_tl_heads(c, K1, Cm); }); }

int axvs_tl_heads_pack(const AxvsTLHeadParams* p, void* packed, int K1, int Cm, int dtype, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!p || !packed) return fail(AXVS_ERR_ARG, "null pointer");
  if (K1 <= 0 || (Cm != 128 && Cm != 256)) return fail(AXVS_ERR_ARG, "mask feature channels must be 128 or 256 (got %d)", Cm);
  Carver c(packed);
  TLHeadsPacked h = carve_tl_heads(c, K1, Cm);
  hipStream_t st = static_cast<hipStream_t>(stream);
  PackDim n256{256, 256, 0, 0, 0}, ncm{Cm, Cm, 0, 0, 0};
  pack_w(dtype, p->mask_embed_w[0], h.w0, n256, n256, st);
  pack_w(dtype, p->mask_embed_w[1], h.w1, n256, n256, st);
  pack_w(dtype, p->mask_embed_w[2], h.w2, ncm, n256, st);
  copy_f32(p->mask_embed_b[0], h.b0, 256, st);
  copy_f32(p->mask_embed_b[1], h.b1, 256, st);
  copy_f32(p->mask_embed_b[2], h.b2, Cm, st);
  copy_f32(p->post_norm_w, h.pn_w, 256, st);
  copy_f32(p->post_norm_b, h.pn_b, 256, st);
  copy_f32(p->activation_proj_w, h.wa, 256, st);
  copy_f32(p->activation_proj_b, h.ba, 1, st);
  hipLaunchKernelGGL(transpose_k1x256_kernel, dim3((unsigned)((K1 * 256 + 255) / 256)), dim3(256), 0, st, p->cls_embed_w, h.wc, K1);
  copy_f32(p->cls_embed_b, h.bc, K1, st);
  return last_launch_status();
}

size_t axvs_tl_heads_workspace_bytes(int B, int Q, int Tc, int Cm) { return carved([&](Carver& c) { carve_tl_heads_fwd_ws(c, (long long)B * Q * Tc, Cm); }); }

int axvs_tl_heads_fwd(const float* clip_query, const float* mask_feature, float* cls_logits, float* mask_logits,
                      const void* packed, int B, int Q, int Tc, int frames_per_clip, int h, int w, int K1, int Cm, int dtype,
                      void* workspace, size_t workspace_bytes, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!clip_query || !mask_feature || !cls_logits || !mask_logits || !packed || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (B <= 0 || Q <= 0 || Tc <= 0 || frames_per_clip <= 0 || h <= 0 || w <= 0 || K1 <= 0) return fail(AXVS_ERR_ARG, "empty shape");
  if (Cm != 128 && Cm != 256) return fail(AXVS_ERR_ARG, "mask feature channels must be 128 or 256 (got %d)", Cm);
  if (Tc > 1024) return fail(AXVS_ERR_ARG, "more than 1024 clips are not supported by the class head");
  if (int rc = check_ws(workspace_bytes, axvs_tl_heads_workspace_bytes(B, Q, Tc, Cm))) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return by_dtype(dtype, [&](auto bf) { return tl_heads_fwd_t<bf()>(clip_query, mask_feature, cls_logits, mask_logits, packed, B, Q, Tc, frames_per_clip, h, w, K1, Cm, workspace, st); });
}

}  // extern "C"
