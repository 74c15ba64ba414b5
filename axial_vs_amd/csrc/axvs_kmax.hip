// C-ABI entry points of Video-kMaX's k-means query decoder (include/axvs.h: axvs_kmax_*) and the launch sequence behind them.
// 1x1 convolutions with their folded BatchNorms: linear() of axvs_eval_host.h (with the slot-list helpers of the pack), the three-piece
// split-precision GEMM always in its form with the gelu epilogues; everything else: axvs_kmax.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "axvs_eval_host.h"
#include "axvs_kmax.h"

using namespace axvs;

namespace {

constexpr int C = kKmaxC, D = kKmaxD, kFfn = 2048;

// the slots of AxvsKmaxLayerParams / AxvsKmaxHeadParams, in declaration order (axial_vs_amd/_params.py states the same order)
enum { PR_DW_W, PR_DW_B, PR_PH1_W, PR_PH1_B, PR_PH2_W, PR_PH2_B, PR_MH_W, PR_MH_B, PR_CLS_W, PR_CLS_B, PR_MASK_AB, PR_N };
enum { LY_PIX1_W, LY_PIX1_B, LY_Q1_W, LY_Q1_B, LY_PRED, LY_KV_W = LY_PRED + PR_N, LY_KV_B, LY_K3_W, LY_K3_B, LY_QKV_W, LY_QKV_B, LY_SIM_AB, LY_RV_AB,
       LY_A3_W, LY_A3_B, LY_F1_W, LY_F1_B, LY_F2_W, LY_F2_B, LY_N };
enum { HD_CENTERS, HD_CEP_W, HD_CEP_B, HD_MEP_W, HD_MEP_B, HD_PRED, HD_N = HD_PRED + PR_N };
static_assert(sizeof(AxvsKmaxLayerParams) == LY_N * sizeof(void*) && sizeof(AxvsKmaxHeadParams) == HD_N * sizeof(void*), "slot lists out of step");

int kmax_check(const AxvsKmaxCfg* c) {
  if (!c) return fail(AXVS_ERR_ARG, "null pointer (cfg)");
  if (c->heads != 8 || c->base_filters != 128 || c->pan_channels != 256)
    return fail(AXVS_ERR_ARG, "heads %d, base_filters %d, panoptic channels %d: the decoder kernels are built for 8 / 128 / 256", c->heads, c->base_filters,
                c->pan_channels);
  if (c->num_layers < 1 || c->num_layers > 16) return fail(AXVS_ERR_ARG, "num_layers=%d must be in 1..16", c->num_layers);
  if (c->L < 1 || c->L > 256) return fail(AXVS_ERR_ARG, "L=%d queries must be in 1..256", c->L);
  if (c->K1 < 1 || c->K1 > 256) return fail(AXVS_ERR_ARG, "K + 1 = %d class logits must be in 1..256", c->K1);
  if (c->T < 1 || c->T > 16) return fail(AXVS_ERR_ARG, "T=%d frames per clip must be in 1..16", c->T);
  if (c->B < 1 || c->B > 4095) return fail(AXVS_ERR_ARG, "B=%d clips must be in 1..4095", c->B);
  for (int i = 0; i < c->num_layers; ++i)
    if (c->layer_level[i] < 0 || c->layer_level[i] > 2) return fail(AXVS_ERR_ARG, "layer %d: level %d must be in 0..2", i, c->layer_level[i]);
  for (int l = 0; l < 3; ++l) {
    if (c->in_channels[l] < 16 || c->in_channels[l] > 2048 || c->in_channels[l] % 16)
      return fail(AXVS_ERR_ARG, "level %d: %d input channels must be a multiple of 16 in 16..2048", l, c->in_channels[l]);
    if (c->h[l] < 1 || c->w[l] < 1 || c->h[l] > 16383 || (long long)c->T * c->h[l] * c->w[l] >= (1ll << 24))
      return fail(AXVS_ERR_ARG, "level %d: T*h*w = %d*%d*%d pixels must be in 1..2^24-1, h <= 16383", l, c->T, c->h[l], c->w[l]);
  }
  if (c->H < 1 || c->W < 1 || c->H > 16383 || (long long)c->T * c->H * c->W >= (1ll << 24))
    return fail(AXVS_ERR_ARG, "panoptic features: T*H*W = %d*%d*%d pixels must be in 1..2^24-1, H <= 16383", c->T, c->H, c->W);
  return AXVS_OK;
}

inline size_t pixels_of(const AxvsKmaxCfg* c, int l) { return (size_t)c->T * c->h[l] * c->w[l]; }       // of one clip
inline size_t pan_pixels(const AxvsKmaxCfg* c) { return (size_t)c->T * c->H * c->W; }
// cluster-sum chunks: a function of the clip's own pixel count alone
inline int sum_chunk(size_t S) {
  const size_t n = std::min((S + kKmaxSumMinChunk - 1) / kKmaxSumMinChunk, (size_t)kKmaxSumMaxChunks);
  return (int)(((S + n - 1) / n + 63) / 64 * 64);
}
inline int sum_chunks(size_t S) { return (int)((S + sum_chunk(S) - 1) / sum_chunk(S)); }

// ---- the packed weights: fp32, BatchNorms folded (by the caller, in float64), one slot after the other -------------------------------------
void pred_sizes(const AxvsKmaxCfg* c, size_t* n) {
  n[PR_DW_W] = 25 * C, n[PR_DW_B] = C, n[PR_PH1_W] = (size_t)C * C, n[PR_PH1_B] = C, n[PR_PH2_W] = (size_t)D * C, n[PR_PH2_B] = D;
  n[PR_MH_W] = (size_t)D * C, n[PR_MH_B] = D, n[PR_CLS_W] = (size_t)c->K1 * C, n[PR_CLS_B] = c->K1, n[PR_MASK_AB] = 4;
}
void layer_sizes(const AxvsKmaxCfg* c, int i, size_t* n) {
  const size_t cin = c->in_channels[c->layer_level[i]];
  n[LY_PIX1_W] = C * cin, n[LY_PIX1_B] = C, n[LY_Q1_W] = (size_t)C * C, n[LY_Q1_B] = C;
  pred_sizes(c, n + LY_PRED);
  n[LY_KV_W] = (size_t)C * kKmaxAug, n[LY_KV_B] = C, n[LY_K3_W] = (size_t)C * C, n[LY_K3_B] = C, n[LY_QKV_W] = (size_t)2 * C * C, n[LY_QKV_B] = 2 * C;
  n[LY_SIM_AB] = 16, n[LY_RV_AB] = 2 * C, n[LY_A3_W] = (size_t)C * C, n[LY_A3_B] = C;
  n[LY_F1_W] = (size_t)kFfn * C, n[LY_F1_B] = kFfn, n[LY_F2_W] = (size_t)C * kFfn, n[LY_F2_B] = C;
}
void head_sizes(const AxvsKmaxCfg* c, size_t* n) {
  n[HD_CENTERS] = (size_t)c->L * C, n[HD_CEP_W] = (size_t)C * C, n[HD_CEP_B] = C, n[HD_MEP_W] = (size_t)C * C, n[HD_MEP_B] = C;
  pred_sizes(c, n + HD_PRED);
}

struct KmaxW {
  float* head[HD_N];
  float* layer[16][LY_N];
  size_t bytes;
};

KmaxW kmax_weights(void* blob, const AxvsKmaxCfg* c) {
  Carver cv(blob);
  KmaxW w;
  size_t n[LY_N > HD_N ? LY_N : HD_N];
  head_sizes(c, n);
  carve_slots(cv, n, HD_N, w.head);
  for (int i = 0; i < c->num_layers; ++i) {
    layer_sizes(c, i, n);
    carve_slots(cv, n, LY_N, w.layer[i]);
  }
  w.bytes = cv.off;
  return w;
}

// ---- the workspace --------------------------------------------------------------------------------------------------------------------------
struct KmaxWs {
  float* gx[3];                      // per level: gelu(feature), channels-last [B*S][Cin]
  float *pa, *pb, *pc, *pf;          // pixel rows [.][256] x 3, [.][128]
  int *idx, *pcnt;
  float *part, *saug;
  float *x, *qs, *mk, *u, *x1, *qkv, *att, *x2, *hid, *ce, *me;
  size_t bytes;
};

// what: 0 the whole decoder, 1 / 2 the assignment / the update of layer `arg`
KmaxWs kmax_carve(void* ws, const AxvsKmaxCfg* c, int what, int arg) {
  Carver cv(ws);
  KmaxWs w = {};
  const size_t B = c->B, R = B * c->L;
  size_t smax = 0;
  for (int l = 0; l < 3; ++l) {
    bool used = what != 0 && l == c->layer_level[arg];
    if (what == 0)
      for (int i = 0; i < c->num_layers; ++i) used |= c->layer_level[i] == l;
    if (!used) continue;
    smax = std::max(smax, pixels_of(c, l));
    w.gx[l] = cv.f(B * pixels_of(c, l) * c->in_channels[l]);
  }
  const bool pan = what == 0 && (c->want_masks || c->want_pixel_feature);
  const size_t sall = std::max(smax, pan ? pan_pixels(c) : 0);
  w.pa = cv.f(B * sall * C), w.pb = cv.f(B * sall * C), w.pc = cv.f(B * smax * C), w.pf = cv.f(B * sall * D);
  w.idx = cv.take<int>(B * smax);
  w.pcnt = cv.take<int>(B * kKmaxSumMaxChunks * c->L);
  w.part = cv.f(B * kKmaxSumMaxChunks * c->L * C), w.saug = cv.f(R * kKmaxAug);
  w.x = cv.f(R * C), w.qs = cv.f(R * C), w.mk = cv.f(R * D), w.u = cv.f(R * C), w.x1 = cv.f(R * C), w.qkv = cv.f(R * 2 * C), w.att = cv.f(R * C);
  w.x2 = cv.f(R * C), w.hid = cv.f(R * kFfn), w.ce = cv.f(R * C), w.me = cv.f(R * C);
  w.bytes = cv.off;
  return w;
}

// ---- launches -------------------------------------------------------------------------------------------------------------------------------
template <bool GELU>
void to_cl(const float* src, float* out, int BT, int Cin, int h, int w, hipStream_t st) {
  nchw_to_rows<GELU>(src, out, BT, Cin, h * w, st);
}

// the predictor's pixel branch on rows `in` [B*TH*w][256] (which it does not change): dw 5x5 -> pb, 1x1 -> `mid`, 1x1 + bias -> pf [.][128]
int predictor_pixels(const AxvsKmaxCfg* c, float* const* pr, const KmaxWs& w, const float* in, float* mid, int TH, int wd, hipStream_t st) {
  const long long P = (long long)c->B * TH * wd;
  hipLaunchKernelGGL(kmax_dw5_kernel, dim3((unsigned)((wd + 7) / 8 * 4), (unsigned)((TH + 3) / 4), (unsigned)c->B), dim3(256), 0, st, in,
                     (const float*)pr[PR_DW_W], (const float*)pr[PR_DW_B], w.pb, TH, wd);
  if (int rc = linear(w.pb, C, pr[PR_PH1_W], pr[PR_PH1_B], mid, P, C, C, C, kActGelu, nullptr, kForm3Gelu, st)) return rc;
  return linear(mid, C, pr[PR_PH2_W], pr[PR_PH2_B], w.pf, P, D, C, D, kActNone, nullptr, kForm3Gelu, st);
}

// The assignment of layer i: x [B*L][256], gx = gelu(level feature) rows -> w.qs (query space), w.pa (pixel space), idx [B*S]
int assign(const AxvsKmaxCfg* c, int i, const KmaxW& p, const KmaxWs& w, const float* x, const float* gx, int* idx, hipStream_t st) {
  float* const* y = p.layer[i];
  const int l = c->layer_level[i], S = (int)pixels_of(c, l);
  const long long R = (long long)c->B * c->L, P = (long long)c->B * S;
  if (int rc = linear(gx, c->in_channels[l], y[LY_PIX1_W], y[LY_PIX1_B], w.pa, P, C, c->in_channels[l], C, kActGelu, nullptr, kForm3Gelu, st)) return rc;
  if (int rc = linear(x, C, y[LY_Q1_W], y[LY_Q1_B], w.qs, R, C, C, C, kActGelu, nullptr, kForm3Gelu, st)) return rc;
  if (int rc = predictor_pixels(c, y + LY_PRED, w, w.pa, w.pc, c->T * c->h[l], c->w[l], st)) return rc;
  if (int rc = linear(w.qs, C, y[LY_PRED + PR_MH_W], y[LY_PRED + PR_MH_B], w.mk, R, D, C, D, kActNone, nullptr, kForm3Gelu, st)) return rc;
  hipLaunchKernelGGL((kmax_assign_kernel<false>), dim3((unsigned)((S + 127) / 128), (unsigned)c->B), dim3(256), 0, st, (const float*)w.pf, (const float*)w.mk,
                     (const float*)y[LY_PRED + PR_MASK_AB], c->L, S, idx, (float*)nullptr, (float*)nullptr);
  return AXVS_OK;
}

// The update of layer i given idx, from w.qs and w.pa as assign() left them: k-means update, self-attention, FFN -> x_out (may be x)
int update(const AxvsKmaxCfg* c, int i, const KmaxW& p, const KmaxWs& w, const float* x, const int* idx, float* x_out, hipStream_t st) {
  float* const* y = p.layer[i];
  const int l = c->layer_level[i], S = (int)pixels_of(c, l), L = c->L;
  const long long R = (long long)c->B * L;
  const int chunk = sum_chunk(S), nchunk = sum_chunks(S);
  // sum of the pixel-space rows per cluster; the value projection and both BatchNorms act on the sums (linearity), the value bias times
  // the pixel count, which rides in column 256 of the sums
  hipLaunchKernelGGL(kmax_sum_kernel, dim3((unsigned)nchunk, (unsigned)((L + kKmaxLChunk - 1) / kKmaxLChunk), (unsigned)c->B), dim3(256), 0, st,
                     (const float*)w.pa, idx, L, S, chunk, nchunk, w.part, w.pcnt);
  hipLaunchKernelGGL(kmax_sum_reduce_kernel, dim3((unsigned)R), dim3(256), 0, st, (const float*)w.part, (const int*)w.pcnt, w.saug, L, nchunk);
  if (int rc = linear(w.saug, kKmaxAug, y[LY_KV_W], y[LY_KV_B], w.u, R, C, kKmaxAug, C, kActNone, nullptr, kForm3Gelu, st)) return rc;
  if (int rc = linear(w.u, C, y[LY_K3_W], y[LY_K3_B], w.x1, R, C, C, C, kActNone, x, kForm3Gelu, st)) return rc;
  // self-attention, from the query space of the incoming queries
  if (int rc = linear(w.qs, C, y[LY_QKV_W], y[LY_QKV_B], w.qkv, R, 2 * C, C, 2 * C, kActNone, nullptr, kForm3Gelu, st)) return rc;
  hipLaunchKernelGGL(kmax_attn_kernel, dim3(kKmaxHeads, (unsigned)c->B), dim3(256), 0, st, (const float*)w.qkv, (const float*)y[LY_SIM_AB],
                     (const float*)y[LY_RV_AB], w.att, L);
  if (int rc = linear(w.att, C, y[LY_A3_W], y[LY_A3_B], w.x2, R, C, C, C, kActGeluAfterRes, w.x1, kForm3Gelu, st)) return rc;
  // FFN
  if (int rc = linear(w.x2, C, y[LY_F1_W], y[LY_F1_B], w.hid, R, kFfn, C, kFfn, kActGelu, nullptr, kForm3Gelu, st)) return rc;
  return linear(w.hid, kFfn, y[LY_F2_W], y[LY_F2_B], x_out, R, C, kFfn, C, kActGeluAfterRes, w.x2, kForm3Gelu, st);
}

void class_logits(const AxvsKmaxCfg* c, float* const* pr, const float* emb, float* out, hipStream_t st) {
  class_logits_rows(emb, pr[PR_CLS_W], pr[PR_CLS_B], out, c->B * c->L, c->K1, st);
}

}  // namespace

size_t axvs_kmax_decoder_packed_bytes(const AxvsKmaxCfg* cfg) {
  if (kmax_check(cfg)) return 0;
  return kmax_weights(nullptr, cfg).bytes;
}

int axvs_kmax_decoder_pack(const AxvsKmaxLayerParams* layers, const AxvsKmaxHeadParams* head, const AxvsKmaxCfg* cfg, void* packed, void* stream) {
  if (int rc = kmax_check(cfg)) return rc;
  if (!layers || !head || !packed) return fail(AXVS_ERR_ARG, "null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const KmaxW w = kmax_weights(packed, cfg);
  size_t n[LY_N > HD_N ? LY_N : HD_N];
  head_sizes(cfg, n);
  if (int rc = copy_slots(w.head, head, n, HD_N, "head", 0, st)) return rc;
  for (int i = 0; i < cfg->num_layers; ++i) {
    layer_sizes(cfg, i, n);
    if (int rc = copy_slots(w.layer[i], layers + i, n, LY_N, "layer", i, st)) return rc;
  }
  return AXVS_OK;
}

size_t axvs_kmax_decoder_workspace_bytes(const AxvsKmaxCfg* cfg) {
  if (kmax_check(cfg)) return 0;
  return kmax_carve(nullptr, cfg, 0, 0).bytes;
}

int axvs_kmax_decoder_fwd(const AxvsKmaxCfg* cfg, const void* packed, const float* const* features, const float* panoptic, float* pred_logits,
                          float* pred_masks, float* pred_mask_embeddings, float* pixel_feature, float* cluster_centers, int* debug_idx, void* workspace,
                          long long workspace_bytes, void* stream) {
  if (int rc = kmax_check(cfg)) return rc;
  if (!packed || !features || !pred_logits || !pred_mask_embeddings || !cluster_centers || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if ((cfg->want_masks && !pred_masks) || (cfg->want_pixel_feature && !pixel_feature) || ((cfg->want_masks || cfg->want_pixel_feature) && !panoptic))
    return fail(AXVS_ERR_ARG, "null pointer (an output flag without its buffer, or without the panoptic features)");
  const KmaxWs w = kmax_carve(workspace, cfg, 0, 0);
  if (int rc = check_ws(workspace_bytes, w.bytes)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const KmaxW p = kmax_weights(const_cast<void*>(packed), cfg);
  const int R = cfg->B * cfg->L, nl = cfg->num_layers, BT = cfg->B * cfg->T;
  for (int l = 0; l < 3; ++l)
    if (w.gx[l]) {
      if (!features[l]) return fail(AXVS_ERR_ARG, "null pointer (level %d features)", l);
      to_cl<true>(features[l], w.gx[l], BT, cfg->in_channels[l], cfg->h[l], cfg->w[l], st);      // the input gelu, once per level
    }
  broadcast_rows(p.head[HD_CENTERS], w.x, cfg->L, R, st);
  int* dbg = debug_idx;
  for (int i = 0; i < nl; ++i) {
    const int l = cfg->layer_level[i];
    int* const idx = dbg ? dbg : w.idx;
    if (int rc = assign(cfg, i, p, w, w.x, w.gx[l], idx, st)) return rc;
    if (int rc = update(cfg, i, p, w, w.x, idx, i == nl - 1 ? cluster_centers : w.x, st)) return rc;
    if (dbg) dbg += (size_t)cfg->B * pixels_of(cfg, l);
  }
  // the final predictor
  const long long Rl = R;
  float* const* pr = p.head + HD_PRED;
  if (int rc = linear(cluster_centers, C, p.head[HD_CEP_W], p.head[HD_CEP_B], w.ce, Rl, C, C, C, kActGelu, nullptr, kForm3Gelu, st)) return rc;
  if (int rc = linear(cluster_centers, C, p.head[HD_MEP_W], p.head[HD_MEP_B], w.me, Rl, C, C, C, kActGelu, nullptr, kForm3Gelu, st)) return rc;
  class_logits(cfg, pr, w.ce, pred_logits, st);
  if (int rc = linear(w.me, C, pr[PR_MH_W], pr[PR_MH_B], pred_mask_embeddings, Rl, D, C, D, kActNone, nullptr, kForm3Gelu, st)) return rc;
  if (cfg->want_masks || cfg->want_pixel_feature) {
    const int S = (int)pan_pixels(cfg);
    to_cl<false>(panoptic, w.pa, BT, C, cfg->H, cfg->W, st);
    if (int rc = predictor_pixels(cfg, pr, w, w.pa, w.pa, cfg->T * cfg->H, cfg->W, st)) return rc;      // (w.pa is dead once the dw conv has read it)
    hipLaunchKernelGGL((kmax_assign_kernel<true>), dim3((unsigned)((S + 127) / 128), (unsigned)cfg->B), dim3(256), 0, st, (const float*)w.pf,
                       (const float*)pred_mask_embeddings, (const float*)pr[PR_MASK_AB], cfg->L, S, (int*)nullptr, cfg->want_masks ? pred_masks : nullptr,
                       cfg->want_pixel_feature ? pixel_feature : nullptr);
  }
  return last_launch_status();
}

size_t axvs_kmax_stage_workspace_bytes(const AxvsKmaxCfg* cfg, int layer, int update_stage) {
  if (kmax_check(cfg) || layer < 0 || layer >= cfg->num_layers) return 0;
  return kmax_carve(nullptr, cfg, update_stage ? 2 : 1, layer).bytes;
}

int axvs_kmax_assign_fwd(const AxvsKmaxCfg* cfg, const void* packed, int layer, const float* query, const float* feature, int* idx, float* class_logits_out,
                         void* workspace, long long workspace_bytes, void* stream) {
  if (int rc = kmax_check(cfg)) return rc;
  if (layer < 0 || layer >= cfg->num_layers) return fail(AXVS_ERR_ARG, "layer=%d must be in 0..%d", layer, cfg->num_layers - 1);
  if (!packed || !query || !feature || !idx || !class_logits_out || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  const KmaxWs w = kmax_carve(workspace, cfg, 1, layer);
  if (int rc = check_ws(workspace_bytes, w.bytes)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const KmaxW p = kmax_weights(const_cast<void*>(packed), cfg);
  const int l = cfg->layer_level[layer];
  to_cl<true>(feature, w.gx[l], cfg->B * cfg->T, cfg->in_channels[l], cfg->h[l], cfg->w[l], st);
  if (int rc = assign(cfg, layer, p, w, query, w.gx[l], idx, st)) return rc;
  class_logits(cfg, p.layer[layer] + LY_PRED, w.qs, class_logits_out, st);
  return last_launch_status();
}

int axvs_kmax_layer_fwd(const AxvsKmaxCfg* cfg, const void* packed, int layer, const float* query, const float* feature, const int* idx, float* out,
                        void* workspace, long long workspace_bytes, void* stream) {
  if (int rc = kmax_check(cfg)) return rc;
  if (layer < 0 || layer >= cfg->num_layers) return fail(AXVS_ERR_ARG, "layer=%d must be in 0..%d", layer, cfg->num_layers - 1);
  if (!packed || !query || !feature || !idx || !out || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  const KmaxWs w = kmax_carve(workspace, cfg, 2, layer);
  if (int rc = check_ws(workspace_bytes, w.bytes)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const KmaxW p = kmax_weights(const_cast<void*>(packed), cfg);
  float* const* y = p.layer[layer];
  const int l = cfg->layer_level[layer];
  const long long R = (long long)cfg->B * cfg->L, P = (long long)cfg->B * pixels_of(cfg, l);
  to_cl<true>(feature, w.gx[l], cfg->B * cfg->T, cfg->in_channels[l], cfg->h[l], cfg->w[l], st);
  if (int rc = linear(w.gx[l], cfg->in_channels[l], y[LY_PIX1_W], y[LY_PIX1_B], w.pa, P, C, cfg->in_channels[l], C, kActGelu, nullptr, kForm3Gelu, st)) return rc;
  if (int rc = linear(query, C, y[LY_Q1_W], y[LY_Q1_B], w.qs, R, C, C, C, kActGelu, nullptr, kForm3Gelu, st)) return rc;
  if (int rc = update(cfg, layer, p, w, query, idx, out, st)) return rc;
  return last_launch_status();
}
