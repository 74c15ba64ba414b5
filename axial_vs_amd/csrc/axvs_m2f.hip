// C-ABI entry points of Tube-Link's per-clip masked-attention query decoder (include/axvs.h: axvs_m2f_*) and the launch sequence behind
// them.  Linear layers: linear() of axvs_eval_host.h on the three-piece split-precision GEMM in its ReLU form (kForm3), x + query_pos as
// the addend X2, and linear_split() below; everything else: axvs_m2f.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "axvs_eval_host.h"
#include "axvs_m2f.h"

using namespace axvs;

namespace {

constexpr int C = kM2fC;
constexpr int kMaxSplits = 16;      // split-K partials of the GEMMs in front of a LayerNorm

int m2f_check(const AxvsM2fCfg* c) {
  if (!c) return fail(AXVS_ERR_ARG, "null pointer (cfg)");
  if (c->C != 256 || c->heads != 8 || c->ffn != 2048 || c->num_levels != 3)
    return fail(AXVS_ERR_ARG, "embed dims %d, heads %d, FFN %d, levels %d: the decoder kernels are built for 256 / 8 / 2048 / 3", c->C, c->heads, c->ffn,
                c->num_levels);
  if (c->num_layers < 1 || c->num_layers > 16) return fail(AXVS_ERR_ARG, "num_layers=%d must be in 1..16", c->num_layers);
  if (c->Q < 1 || c->Q > 256) return fail(AXVS_ERR_ARG, "Q=%d queries must be in 1..256", c->Q);
  if (c->T < 1 || c->T > 16) return fail(AXVS_ERR_ARG, "T=%d frames per clip must be in 1..16", c->T);
  if (c->N < 1 || c->N > 4095) return fail(AXVS_ERR_ARG, "N=%d clips must be in 1..4095", c->N);
  if (c->K1 < 1 || c->K1 > 4096) return fail(AXVS_ERR_ARG, "K + 1 = %d class logits must be in 1..4096", c->K1);
  if (c->h < 1 || c->w < 1 || (long long)c->h * c->w >= (1ll << 24) || c->h > 65535)
    return fail(AXVS_ERR_ARG, "mask features %d x %d: h*w must be in 1..2^24-1", c->h, c->w);
  for (int l = 0; l < 3; ++l)
    if (c->lh[l] < 1 || c->lw[l] < 1 || c->lh[l] > 65535 || (long long)c->T * c->lh[l] * c->lw[l] >= (1ll << 24))
      return fail(AXVS_ERR_ARG, "level %d: T*h*w = %d*%d*%d keys must be in 1..2^24-1", l, c->T, c->lh[l], c->lw[l]);
  return AXVS_OK;
}

inline int keys_of(const AxvsM2fCfg* c, int l) { return c->T * c->lh[l] * c->lw[l]; }
inline int layers_of(const AxvsM2fCfg* c, int l) { return l < c->num_layers ? (c->num_layers - l + 2) / 3 : 0; }
inline int words_of(int S) { return (S + 31) / 32; }
inline int chunks_of(int S) { return std::min((S + kM2fKeyChunk - 1) / kM2fKeyChunk, kM2fMaxChunks); }
inline int chunk_of(int S) { return ((S + chunks_of(S) - 1) / chunks_of(S) + 31) / 32 * 32; }

// ---- the packed weights: fp32, the k / v rows of the cross-attention in_proj of every layer of a level stacked into one matrix ------------
struct M2fLayerW {
  float *wq, *bq, *cross_out_w, *cross_out_b, *norm0_w, *norm0_b, *self_in_w, *self_in_b, *self_out_w, *self_out_b, *norm1_w, *norm1_b, *ffn1_w, *ffn1_b,
      *ffn2_w, *ffn2_b, *norm2_w, *norm2_b;
};
struct M2fW {
  float *post_norm_w, *post_norm_b, *query_embed, *query_feat, *level_embed, *me_w[3], *me_b[3], *cls_w, *cls_b;
  float *wk[3], *bk[3], *wv[3], *bv[3];      // per level: [layers of the level * C][C], [layers of the level * C]
  M2fLayerW layer[16];
  size_t bytes;
};

M2fW m2f_weights(void* blob, const AxvsM2fCfg* c) {
  Carver cv(blob);
  M2fW w;
  w.post_norm_w = cv.f(C), w.post_norm_b = cv.f(C);
  w.query_embed = cv.f((size_t)c->Q * C), w.query_feat = cv.f((size_t)c->Q * C), w.level_embed = cv.f(3 * C);
  for (int i = 0; i < 3; ++i) w.me_w[i] = cv.f((size_t)C * C), w.me_b[i] = cv.f(C);
  w.cls_w = cv.f((size_t)c->K1 * C), w.cls_b = cv.f(c->K1);
  for (int l = 0; l < 3; ++l) {
    const size_t n = (size_t)std::max(layers_of(c, l), 1) * C;
    w.wk[l] = cv.f(n * C), w.bk[l] = cv.f(n), w.wv[l] = cv.f(n * C), w.bv[l] = cv.f(n);
  }
  for (int i = 0; i < c->num_layers; ++i) {
    M2fLayerW& y = w.layer[i];
    y.wq = cv.f((size_t)C * C), y.bq = cv.f(C), y.cross_out_w = cv.f((size_t)C * C), y.cross_out_b = cv.f(C), y.norm0_w = cv.f(C), y.norm0_b = cv.f(C);
    y.self_in_w = cv.f((size_t)3 * C * C), y.self_in_b = cv.f(3 * C), y.self_out_w = cv.f((size_t)C * C), y.self_out_b = cv.f(C);
    y.norm1_w = cv.f(C), y.norm1_b = cv.f(C);
    y.ffn1_w = cv.f((size_t)c->ffn * C), y.ffn1_b = cv.f(c->ffn), y.ffn2_w = cv.f((size_t)C * c->ffn), y.ffn2_b = cv.f(C);
    y.norm2_w = cv.f(C), y.norm2_b = cv.f(C);
  }
  w.bytes = cv.off;
  return w;
}

// ---- the workspace --------------------------------------------------------------------------------------------------------------------------
struct M2fWs {
  float *mf[3], *K[3], *V[3];        // per level: resized mask features [N][S][C]; keys / values of the level's layers [N*S][layers * C]
  float *key_in, *val_in;            // [N*S_max][C]: the projections' inputs of the level at hand
  float *x, *y, *qpos, *h1, *h2, *me, *qp, *att, *t, *x1, *x2, *qk, *v, *hid, *po, *pml;      // t: [kMaxSplits][N*Q][C] split-K partials
  unsigned* bits;
  int* flags;
  size_t bytes;
};

// what: 0 the whole decoder, 1 one mask head (level `arg`), 2 one layer (`arg`)
M2fWs m2f_carve(void* ws, const AxvsM2fCfg* c, int what, int arg) {
  Carver cv(ws);
  M2fWs w = {};
  const size_t N = c->N, R = N * c->Q;
  size_t smax = 0, wmax = 0, chmax = 1;
  for (int l = 0; l < 3; ++l) {
    const bool level_used = what == 0 || (what == 1 && l == arg) || (what == 2 && l == arg % 3);
    if (!level_used) continue;
    const size_t S = keys_of(c, l);
    smax = std::max(smax, S), wmax = std::max(wmax, (size_t)words_of((int)S)), chmax = std::max(chmax, (size_t)chunks_of((int)S));
    if (what != 2) w.mf[l] = cv.f(N * S * C);
    if (what != 1) {
      const size_t nl = what == 0 ? layers_of(c, l) : 1;
      w.K[l] = cv.f(N * S * nl * C), w.V[l] = cv.f(N * S * nl * C);
    }
  }
  if (what != 1) w.key_in = cv.f(N * smax * C), w.val_in = cv.f(N * smax * C);
  w.x = cv.f(R * C), w.y = cv.f(R * C), w.qpos = cv.f(R * C), w.h1 = cv.f(R * C), w.h2 = cv.f(R * C), w.me = cv.f(R * C);
  w.qp = cv.f(R * C), w.att = cv.f(R * C), w.t = cv.f(R * C * kMaxSplits), w.x1 = cv.f(R * C), w.x2 = cv.f(R * C);
  w.qk = cv.f(R * 2 * C), w.v = cv.f(R * C), w.hid = cv.f(R * c->ffn);
  w.po = cv.f(N * kM2fHeads * chmax * c->Q * 32), w.pml = cv.f(N * kM2fHeads * chmax * c->Q * 2);
  w.bits = cv.take<unsigned>(R * wmax);
  w.flags = cv.take<int>(R);
  w.bytes = cv.off;
  return w;
}

// ---- launches -------------------------------------------------------------------------------------------------------------------------------
// The GEMMs in front of a LayerNorm: M = N*Q rows alone are one or two row tiles, so the contraction is split over workgroups (ksteps
// 32-wide steps each); the partials P[z][M][C] are added, with bias and residual, by m2f_ln_kernel.  Returns the number of partials.
int linear_split(const float* X, const float* W, float* P, long long M, int K, int ksteps, hipStream_t st, int* nparts) {
  const int nk = (K + tr::kGK - 1) / tr::kGK, z = (nk + ksteps - 1) / ksteps;
  if (z > kMaxSplits) return fail(AXVS_ERR_ARG, "split-K: %d partials, at most %d", z, kMaxSplits);
  tr::GemmLd ld{K, K, C, ksteps, nullptr};
  const tr::GemmEpi e{nullptr, 1.f, 0, tr::Drop{0u, 0u, 0u, 1.f}, 0.f};
  *nparts = z;
  return tr::gemm_nt(X, W, P, M, C, K, ld, e, tr::GemmNtForm{3}, z, st);
}

M2fMap level_map(const AxvsM2fCfg* c, int l, bool mem) { return M2fMap{c->T, mem ? c->lh[l] : c->h, mem ? c->lw[l] : c->w, c->lh[l], c->lw[l]}; }

void resize_level(const AxvsM2fCfg* c, int l, const float* mask_features, float* mf, hipStream_t st) {
  const dim3 grid((unsigned)((c->lw[l] + 31) / 32 * (C / 64)), (unsigned)c->lh[l], (unsigned)(c->N * c->T));
  hipLaunchKernelGGL((m2f_to_cl_kernel<false>), grid, dim3(256), 0, st, mask_features, mf, (float*)nullptr, (const float*)nullptr, level_map(c, l, false),
                     0.f, 0, 0.f);
}

// keys and values of `nl` layers of level l: memory -> (values, keys) inputs -> two GEMMs against the stacked weights wk / wv [nl*C][C]
int project_level(const AxvsM2fCfg* c, int l, const float* memory, const M2fW& p, const M2fWs& w, const float* wk, const float* bk, const float* wv,
                  const float* bv, int nl, hipStream_t st) {
  const dim3 grid((unsigned)((c->lw[l] + 31) / 32 * (C / 64)), (unsigned)c->lh[l], (unsigned)(c->N * c->T));
  hipLaunchKernelGGL((m2f_to_cl_kernel<true>), grid, dim3(256), 0, st, memory, w.val_in, w.key_in, (const float*)(p.level_embed + l * C), level_map(c, l, true),
                     c->pos_temperature, c->pos_normalize, c->pos_scale);
  const long long rows = (long long)c->N * keys_of(c, l);
  if (int rc = linear(w.key_in, C, wk, bk, w.K[l], rows, nl * C, C, (long long)nl * C, kActNone, nullptr, kForm3, st)) return rc;
  return linear(w.val_in, C, wv, bv, w.V[l], rows, nl * C, C, (long long)nl * C, kActNone, nullptr, kForm3, st);
}

void logits_grid(int Q, int S, int Z, dim3* grid, int* per_y) {
  const int nqt = (Q + 15) / 16, waves = (S + 31) / 32 * Z;
  const int ysplit = std::max(1, std::min(nqt, (1024 + waves - 1) / waves));      // about a thousand waves, when the queries allow it
  *per_y = (nqt + ysplit - 1) / ysplit;
  *grid = dim3((unsigned)((S + 127) / 128), (unsigned)((nqt + *per_y - 1) / *per_y), (unsigned)Z);
}

// y (post-normed queries) -> mask_embed MLP -> w.me
int mask_embed(const AxvsM2fCfg* c, const M2fW& p, const M2fWs& w, const float* y, hipStream_t st) {
  const long long R = (long long)c->N * c->Q;
  if (int rc = linear(y, C, p.me_w[0], p.me_b[0], w.h1, R, C, C, C, kActRelu, nullptr, kForm3, st)) return rc;
  if (int rc = linear(w.h1, C, p.me_w[1], p.me_b[1], w.h2, R, C, C, C, kActRelu, nullptr, kForm3, st)) return rc;
  return linear(w.h2, C, p.me_w[2], p.me_b[2], w.me, R, C, C, C, kActNone, nullptr, kForm3, st);
}

// the mask head in front of a layer of level l, from the post-normed queries y: bits [N*Q][ceil(S/32)], flags [N*Q] (cleared by the caller)
int mask_head(const AxvsM2fCfg* c, int l, const M2fW& p, const M2fWs& w, const float* y, unsigned* bits, int* flags, hipStream_t st) {
  if (int rc = mask_embed(c, p, w, y, st)) return rc;
  const int S = keys_of(c, l);
  dim3 grid;
  int per_y;
  logits_grid(c->Q, S, c->N, &grid, &per_y);
  hipLaunchKernelGGL((m2f_logits_kernel<true, true>), grid, dim3(256), 0, st, (const float*)w.me, (const float*)w.mf[l], c->Q, S, 1, bits, flags,
                     (float*)nullptr, words_of(S), per_y);
  return AXVS_OK;
}

void attention(const AxvsM2fCfg* c, const M2fWs& w, const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv, int S,
               const unsigned* bits, const int* flags, hipStream_t st) {
  M2fAttn a;
  a.q = q, a.k = k, a.v = v, a.ldq = ldq, a.ldk = ldk, a.ldv = ldv;
  a.Q = c->Q, a.S = S, a.chunk = chunk_of(S), a.nchunk = (S + a.chunk - 1) / a.chunk;
  a.scale = 0.17677669529663687f;      // 1 / sqrt(32)
  a.bits = bits, a.flags = flags, a.W = words_of(S), a.po = w.po, a.pml = w.pml;
  hipLaunchKernelGGL(m2f_attn_kernel, dim3((unsigned)((c->Q + 15) / 16), (unsigned)a.nchunk, (unsigned)(c->N * kM2fHeads)), dim3(64), 0, st, a);
  hipLaunchKernelGGL(m2f_attn_combine_kernel, dim3((unsigned)(c->N * c->Q)), dim3(256), 0, st, (const float*)w.po, (const float*)w.pml, w.att, c->Q, a.nchunk);
}

void layer_norm(const float* in, int nparts, size_t part_stride, const float* bias, const float* res, const float* g1, const float* b1, float* out1,
                const float* g2, const float* b2, float* out2, int* flags, int rows, hipStream_t st) {
  hipLaunchKernelGGL(m2f_ln_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, in, nparts, part_stride, bias, res, g1, b1, out1, g2, b2, out2, flags,
                     rows);
}

// One layer: cross_attn, norm, self_attn, norm, ffn, norm.  K / V: the layer's keys / values (row stride ldkv).  x_out may be x_in.
// y_out (nullable): post_norm(x_out), the input of the next mask head; flags_next (nullable): cleared along with it.
int layer(const AxvsM2fCfg* c, int i, const M2fW& p, const M2fWs& w, const float* x_in, const float* K, const float* V, long long ldkv,
          const unsigned* bits, const int* flags, float* x_out, float* y_out, int* flags_next, hipStream_t st) {
  const M2fLayerW& y = p.layer[i];
  const long long R = (long long)c->N * c->Q;
  const int rows = (int)R, S = keys_of(c, i % 3);
  const size_t ps = (size_t)R * C;
  int np = 1;
  // cross-attention: q = (x + query_pos) Wq^T + bq
  if (int rc = linear(x_in, C, y.wq, y.bq, w.qp, R, C, C, C, kActNone, nullptr, kForm3, st, w.qpos)) return rc;
  attention(c, w, w.qp, C, K, ldkv, V, ldkv, S, bits, flags, st);
  if (int rc = linear_split(w.att, y.cross_out_w, w.t, R, C, 2, st, &np)) return rc;
  layer_norm(w.t, np, ps, y.cross_out_b, x_in, y.norm0_w, y.norm0_b, w.x1, nullptr, nullptr, nullptr, nullptr, rows, st);
  // self-attention: q = k = x + query_pos, v = x
  if (int rc = linear(w.x1, C, y.self_in_w, y.self_in_b, w.qk, R, 2 * C, C, 2 * C, kActNone, nullptr, kForm3, st, w.qpos)) return rc;
  if (int rc = linear(w.x1, C, y.self_in_w + (size_t)2 * C * C, y.self_in_b + 2 * C, w.v, R, C, C, C, kActNone, nullptr, kForm3, st)) return rc;
  attention(c, w, w.qk, 2 * C, w.qk + C, 2 * C, w.v, C, c->Q, nullptr, nullptr, st);
  if (int rc = linear_split(w.att, y.self_out_w, w.t, R, C, 2, st, &np)) return rc;
  layer_norm(w.t, np, ps, y.self_out_b, w.x1, y.norm1_w, y.norm1_b, w.x2, nullptr, nullptr, nullptr, nullptr, rows, st);
  // FFN: the second GEMM contracts 2048 channels -- 16 partials of 4 steps
  if (int rc = linear(w.x2, C, y.ffn1_w, y.ffn1_b, w.hid, R, c->ffn, C, c->ffn, kActRelu, nullptr, kForm3, st)) return rc;
  if (int rc = linear_split(w.hid, y.ffn2_w, w.t, R, c->ffn, 4, st, &np)) return rc;
  layer_norm(w.t, np, ps, y.ffn2_b, w.x2, y.norm2_w, y.norm2_b, x_out, y_out ? p.post_norm_w : nullptr, p.post_norm_b, y_out, flags_next, rows, st);
  return AXVS_OK;
}

}  // namespace

size_t axvs_m2f_decoder_packed_bytes(const AxvsM2fCfg* cfg) {
  if (m2f_check(cfg)) return 0;
  return m2f_weights(nullptr, cfg).bytes;
}

int axvs_m2f_decoder_pack(const AxvsM2fLayerParams* layers, const AxvsM2fHeadParams* head, const AxvsM2fCfg* cfg, void* packed, void* stream) {
  if (int rc = m2f_check(cfg)) return rc;
  if (!layers || !head || !packed) return fail(AXVS_ERR_ARG, "null pointer");
  const void* const* hp = reinterpret_cast<const void* const*>(head);
  for (size_t i = 0; i < sizeof(AxvsM2fHeadParams) / sizeof(void*); ++i)
    if (!hp[i]) return fail(AXVS_ERR_ARG, "null pointer (head parameter %zu)", i);
  for (int l = 0; l < cfg->num_layers; ++l) {
    const void* const* lp = reinterpret_cast<const void* const*>(layers + l);
    for (size_t i = 0; i < sizeof(AxvsM2fLayerParams) / sizeof(void*); ++i)
      if (!lp[i]) return fail(AXVS_ERR_ARG, "null pointer (layer %d, parameter %zu)", l, i);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const M2fW w = m2f_weights(packed, cfg);
  const size_t CC = (size_t)C * C, Q = cfg->Q, F = cfg->ffn;
  struct Cp { float* d; const float* s; size_t n; };
  Cp hc[] = {{w.post_norm_w, head->post_norm_w, (size_t)C}, {w.post_norm_b, head->post_norm_b, (size_t)C}, {w.query_embed, head->query_embed, Q * C},
             {w.query_feat, head->query_feat, Q * C}, {w.level_embed, head->level_embed, (size_t)3 * C},
             {w.me_w[0], head->mask_embed_w[0], CC}, {w.me_w[1], head->mask_embed_w[1], CC}, {w.me_w[2], head->mask_embed_w[2], CC},
             {w.me_b[0], head->mask_embed_b[0], (size_t)C}, {w.me_b[1], head->mask_embed_b[1], (size_t)C}, {w.me_b[2], head->mask_embed_b[2], (size_t)C},
             {w.cls_w, head->cls_embed_w, (size_t)cfg->K1 * C}, {w.cls_b, head->cls_embed_b, (size_t)cfg->K1}};
  for (const Cp& c : hc)
    if (int rc = copy_f(c.d, c.s, c.n, st)) return rc;
  for (int i = 0; i < cfg->num_layers; ++i) {
    const AxvsM2fLayerParams& s = layers[i];
    const M2fLayerW& y = w.layer[i];
    const int l = i % 3, j = i / 3;
    Cp lc[] = {{y.wq, s.cross_in_w, CC}, {y.bq, s.cross_in_b, (size_t)C},
               {w.wk[l] + j * CC, s.cross_in_w + CC, CC}, {w.bk[l] + j * C, s.cross_in_b + C, (size_t)C},
               {w.wv[l] + j * CC, s.cross_in_w + 2 * CC, CC}, {w.bv[l] + j * C, s.cross_in_b + 2 * C, (size_t)C},
               {y.cross_out_w, s.cross_out_w, CC}, {y.cross_out_b, s.cross_out_b, (size_t)C}, {y.norm0_w, s.norm0_w, (size_t)C}, {y.norm0_b, s.norm0_b, (size_t)C},
               {y.self_in_w, s.self_in_w, 3 * CC}, {y.self_in_b, s.self_in_b, (size_t)3 * C}, {y.self_out_w, s.self_out_w, CC},
               {y.self_out_b, s.self_out_b, (size_t)C}, {y.norm1_w, s.norm1_w, (size_t)C}, {y.norm1_b, s.norm1_b, (size_t)C},
               {y.ffn1_w, s.ffn1_w, F * C}, {y.ffn1_b, s.ffn1_b, F}, {y.ffn2_w, s.ffn2_w, F * C}, {y.ffn2_b, s.ffn2_b, (size_t)C},
               {y.norm2_w, s.norm2_w, (size_t)C}, {y.norm2_b, s.norm2_b, (size_t)C}};
    for (const Cp& c : lc)
      if (int rc = copy_f(c.d, c.s, c.n, st)) return rc;
  }
  return AXVS_OK;
}

size_t axvs_m2f_decoder_workspace_bytes(const AxvsM2fCfg* cfg) {
  if (m2f_check(cfg)) return 0;
  return m2f_carve(nullptr, cfg, 0, 0).bytes;
}

int axvs_m2f_decoder_fwd(const AxvsM2fCfg* cfg, const void* packed, const float* mask_features, const float* const* memories, float* query_out,
                         float* cls_pred, float* mask_pred, unsigned* debug_bits, int* debug_flags, void* workspace, long long workspace_bytes,
                         void* stream) {
  if (int rc = m2f_check(cfg)) return rc;
  if (!packed || !mask_features || !memories || !memories[0] || !memories[1] || !memories[2] || !query_out || !workspace)
    return fail(AXVS_ERR_ARG, "null pointer");
  if (cfg->return_predictions && (!cls_pred || !mask_pred)) return fail(AXVS_ERR_ARG, "null pointer (return_predictions without cls_pred / mask_pred)");
  if ((debug_bits == nullptr) != (debug_flags == nullptr)) return fail(AXVS_ERR_ARG, "debug_bits and debug_flags come together");
  const M2fWs w = m2f_carve(workspace, cfg, 0, 0);
  if (int rc = check_ws(workspace_bytes, w.bytes)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const M2fW p = m2f_weights(const_cast<void*>(packed), cfg);
  const int R = cfg->N * cfg->Q, nl = cfg->num_layers;
  // keys and values of every layer, and the mask features at every level's size: none of it depends on the queries
  for (int l = 0; l < 3; ++l) {
    resize_level(cfg, l, mask_features, w.mf[l], st);
    if (layers_of(cfg, l) > 0)
      if (int rc = project_level(cfg, l, memories[l], p, w, p.wk[l], p.bk[l], p.wv[l], p.bv[l], layers_of(cfg, l), st)) return rc;
  }
  // the sequential chain
  unsigned* bits = debug_bits ? debug_bits : w.bits;
  int* flags = debug_flags ? debug_flags : w.flags;
  broadcast_rows(p.query_feat, w.x, cfg->Q, R, st, p.query_embed, w.qpos);
  layer_norm(w.x, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, p.post_norm_w, p.post_norm_b, w.y, flags, R, st);
  for (int i = 0; i < nl; ++i) {
    const int l = i % 3, j = i / 3;
    if (int rc = mask_head(cfg, l, p, w, w.y, bits, flags, st)) return rc;
    unsigned* nbits = bits;
    int* nflags = flags;
    if (debug_bits) nbits = bits + (size_t)R * words_of(keys_of(cfg, l)), nflags = flags + R;
    const long long ldkv = (long long)layers_of(cfg, l) * C;
    const bool last = i == nl - 1;
    if (int rc = layer(cfg, i, p, w, w.x, w.K[l] + (size_t)j * C, w.V[l] + (size_t)j * C, ldkv, bits, flags, last ? query_out : w.x,
                       last && !cfg->return_predictions ? nullptr : w.y, last ? nullptr : nflags, st))
      return rc;
    bits = nbits, flags = nflags;
  }
  if (cfg->return_predictions) {      // the one full-resolution mask einsum
    class_logits_rows(w.y, p.cls_w, p.cls_b, cls_pred, R, cfg->K1, st);
    if (int rc = mask_embed(cfg, p, w, w.y, st)) return rc;
    dim3 grid;
    int per_y;
    logits_grid(cfg->Q, cfg->h * cfg->w, cfg->N * cfg->T, &grid, &per_y);
    hipLaunchKernelGGL((m2f_logits_kernel<false, false>), grid, dim3(256), 0, st, (const float*)w.me, mask_features, cfg->Q, cfg->h * cfg->w, cfg->T,
                       (unsigned*)nullptr, (int*)nullptr, mask_pred, 0, per_y);
  }
  return last_launch_status();
}

size_t axvs_m2f_attn_mask_workspace_bytes(const AxvsM2fCfg* cfg, int level) {
  if (m2f_check(cfg) || level < 0 || level > 2) return 0;
  return m2f_carve(nullptr, cfg, 1, level).bytes;
}

int axvs_m2f_attn_mask_fwd(const AxvsM2fCfg* cfg, const void* packed, const float* x, const float* mask_features, int level, unsigned* bits, int* flags,
                           void* workspace, long long workspace_bytes, void* stream) {
  if (int rc = m2f_check(cfg)) return rc;
  if (level < 0 || level > 2) return fail(AXVS_ERR_ARG, "level=%d must be in 0..2", level);
  if (!packed || !x || !mask_features || !bits || !flags || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  const M2fWs w = m2f_carve(workspace, cfg, 1, level);
  if (int rc = check_ws(workspace_bytes, w.bytes)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const M2fW p = m2f_weights(const_cast<void*>(packed), cfg);
  const int R = cfg->N * cfg->Q;
  resize_level(cfg, level, mask_features, w.mf[level], st);
  layer_norm(x, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, p.post_norm_w, p.post_norm_b, w.y, flags, R, st);
  if (int rc = mask_head(cfg, level, p, w, w.y, bits, flags, st)) return rc;
  return last_launch_status();
}

size_t axvs_m2f_layer_workspace_bytes(const AxvsM2fCfg* cfg, int layer_index) {
  if (m2f_check(cfg) || layer_index < 0 || layer_index >= cfg->num_layers) return 0;
  return m2f_carve(nullptr, cfg, 2, layer_index).bytes;
}

int axvs_m2f_layer_fwd(const AxvsM2fCfg* cfg, const void* packed, int layer_index, const float* x, const float* memory, const unsigned* bits,
                       const int* flags, float* out, void* workspace, long long workspace_bytes, void* stream) {
  if (int rc = m2f_check(cfg)) return rc;
  if (layer_index < 0 || layer_index >= cfg->num_layers) return fail(AXVS_ERR_ARG, "layer=%d must be in 0..%d", layer_index, cfg->num_layers - 1);
  if (!packed || !x || !memory || !bits || !flags || !out || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  const M2fWs w = m2f_carve(workspace, cfg, 2, layer_index);
  if (int rc = check_ws(workspace_bytes, w.bytes)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const M2fW p = m2f_weights(const_cast<void*>(packed), cfg);
  const int R = cfg->N * cfg->Q, l = layer_index % 3, j = layer_index / 3;
  broadcast_rows(p.query_feat, w.x, cfg->Q, R, st, p.query_embed, w.qpos);      // (w.x: scratch here; the layer's input is the caller's x)
  if (int rc = project_level(cfg, l, memory, p, w, p.wk[l] + (size_t)j * C * C, p.bk[l] + j * C, p.wv[l] + (size_t)j * C * C, p.bv[l] + j * C, 1, st)) return rc;
  if (int rc = layer(cfg, layer_index, p, w, x, w.K[l], w.V[l], C, bits, flags, out, nullptr, nullptr, st)) return rc;
  return last_launch_status();
}
