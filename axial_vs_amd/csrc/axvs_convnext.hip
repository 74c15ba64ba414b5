// C-ABI entry points of the ConvNeXt / ConvNeXtV2 backbone (include/axvs.h: axvs_cnx_*) and the launch sequence behind them.
// Every Linear layer -- the two kinds of patchify convolution over gathered patches, pwconv1 with its gelu, pwconv2 with the residual --
// is one linear() of axvs_eval_host.h (with the slot-list helpers of the pack and locate()): the three-piece split-precision GEMM in its
// form with the gelu epilogues; everything else: axvs_convnext.h.
// V2's GRN reaches pwconv2 as a per-frame scaled copy of its weight, W2 diag(s_n): one GEMM per frame, the hidden rows are read once
// more for their sums of squares and never rewritten.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "axvs_convnext.h"
#include "axvs_eval_host.h"
#include "axvs_layout.h"

using namespace axvs;

namespace {

constexpr int kStages = 4, kMaxDepth = 64;

// the slots of AxvsCnxDownParams / AxvsCnxBlockParams, in declaration order (axial_vs_amd/_params.py states the same order)
enum { DN_LN_W, DN_LN_B, DN_W, DN_B, DN_N };
enum { BK_DW_W, BK_DW_B, BK_LN_W, BK_LN_B, BK_W1, BK_B1, BK_W2, BK_B2, BK_GRN, BK_N };
static_assert(sizeof(AxvsCnxDownParams) == DN_N * sizeof(void*) && sizeof(AxvsCnxBlockParams) == BK_N * sizeof(void*), "slot lists out of step");

inline size_t pixels_of(const AxvsCnxCfg* c, int i) { return (size_t)c->N * c->h[i] * c->w[i]; }
inline int grn_chunks(const AxvsCnxCfg* c, int i) { return (c->h[i] * c->w[i] + kCnxGrnChunk - 1) / kCnxGrnChunk; }

int cnx_check(const AxvsCnxCfg* c) {
  if (!c) return fail(AXVS_ERR_ARG, "null pointer (cfg)");
  if (c->N < 1 || c->N > 4096) return fail(AXVS_ERR_ARG, "N=%d frames must be in 1..4096", c->N);
  for (int i = 0; i < kStages; ++i) {
    if (c->dims[i] < 16 || c->dims[i] > kCnxMaxC || c->dims[i] % 16)
      return fail(AXVS_ERR_ARG, "stage %d: %d channels must be a multiple of 16 in 16..%d", i, c->dims[i], kCnxMaxC);
    if (c->depths[i] < 1 || c->depths[i] > kMaxDepth) return fail(AXVS_ERR_ARG, "stage %d: %d blocks must be in 1..%d", i, c->depths[i], kMaxDepth);
    if (c->h[i] < 1 || c->w[i] < 1 || c->h[i] > 16383 || c->w[i] > 16383 || (long long)c->N * c->h[i] * c->w[i] >= (1ll << 24))
      return fail(AXVS_ERR_ARG, "stage %d: N*h*w = %d*%d*%d pixels must be in 1..2^24-1, h and w <= 16383", i, c->N, c->h[i], c->w[i]);
  }
  return AXVS_OK;
}

// the whole network: the image's size decides every map's
int cnx_check_sizes(const AxvsCnxCfg* c) {
  if (c->H < 1 || c->W < 1 || c->H > 65535 || c->W > 65535) return fail(AXVS_ERR_ARG, "image %d x %d: H and W must be in 1..65535", c->H, c->W);
  int h = (c->H + 3) / 4, w = (c->W + 3) / 4;
  for (int i = 0; i < kStages; ++i) {
    if (c->h[i] != h || c->w[i] != w)
      return fail(AXVS_ERR_ARG, "stage %d: map %d x %d, but an image of %d x %d gives %d x %d", i, c->h[i], c->w[i], c->H, c->W, h, w);
    h = (h + 1) / 2, w = (w + 1) / 2;
  }
  return AXVS_OK;
}

// ---- the packed weights: fp32, one slot after the other ----------------------------------------------------------------------------------------
void down_sizes(const AxvsCnxCfg* c, int i, size_t* n) {
  const size_t cout = c->dims[i], k = i == 0 ? 48 : 4 * (size_t)c->dims[i - 1], ln = i == 0 ? cout : c->dims[i - 1];
  n[DN_LN_W] = ln, n[DN_LN_B] = ln, n[DN_W] = cout * k, n[DN_B] = cout;
}
void block_sizes(const AxvsCnxCfg* c, int i, size_t* n) {
  const size_t C = c->dims[i];
  n[BK_DW_W] = 49 * C, n[BK_DW_B] = C, n[BK_LN_W] = C, n[BK_LN_B] = C, n[BK_W1] = 4 * C * C, n[BK_B1] = 4 * C, n[BK_W2] = 4 * C * C, n[BK_B2] = C;
  n[BK_GRN] = c->v2 ? 4 * C : 0;
}

struct CnxW {
  float* down[kStages][DN_N];
  float* block[kStages][kMaxDepth][BK_N];
  size_t bytes;
};

CnxW cnx_weights(void* blob, const AxvsCnxCfg* c) {
  Carver cv(blob);
  CnxW w = {};
  size_t n[BK_N];
  for (int i = 0; i < kStages; ++i) {
    down_sizes(c, i, n);
    carve_slots(cv, n, DN_N, w.down[i]);
    block_sizes(c, i, n);
    for (int j = 0; j < c->depths[i]; ++j) carve_slots(cv, n, BK_N, w.block[i][j]);
  }
  w.bytes = cv.off;
  return w;
}

// ---- the workspace: sized for the largest stage, carved once -----------------------------------------------------------------------------------
struct CnxWs {
  float *x, *y;          // a block's input and output rows, swapped from block to block
  float *t;              // the normalised rows of a block; the patches of the stem and of a downsample layer
  float *hid;            // the hidden rows [P][4 C]
  float *part, *s, *w2s; // v2: the chunk sums [N][chunks][4 C], the scales [N][4 C], one frame's W2 diag(s)
  size_t bytes;
};

CnxWs cnx_carve(void* ws, const AxvsCnxCfg* c) {
  size_t xy = 0, t = 0, hid = 0, part = 0, s = 0, w2s = 0;
  for (int i = 0; i < kStages; ++i) {
    const size_t P = pixels_of(c, i), C = c->dims[i];
    xy = std::max(xy, P * C), hid = std::max(hid, P * 4 * C);
    t = std::max(t, P * std::max(C, i == 0 ? (size_t)48 : 4 * (size_t)c->dims[i - 1]));
    if (c->v2) part = std::max(part, (size_t)c->N * grn_chunks(c, i) * 4 * C), s = std::max(s, (size_t)c->N * 4 * C), w2s = std::max(w2s, 4 * C * C);
  }
  Carver cv(ws);
  CnxWs w = {};
  w.x = cv.f(xy), w.y = cv.f(xy), w.t = cv.f(t), w.hid = cv.f(hid), w.part = cv.f(part), w.s = cv.f(s), w.w2s = cv.f(w2s);
  w.bytes = cv.off;
  return w;
}

// ---- launches -------------------------------------------------------------------------------------------------------------------------------
void row_ln(const float* src, const float* g, const float* b, float* dst, int C, size_t P, hipStream_t st) {
  hipLaunchKernelGGL(cnx_row_ln_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, st, src, g, b, dst, C, P);
}

// image -> out rows [P0][dims[0]]
int stem(const AxvsCnxCfg* c, float* const* p, const CnxWs& w, const float* image, float* out, hipStream_t st) {
  const size_t P = pixels_of(c, 0), total = P * 12;
  hipLaunchKernelGGL(cnx_stem_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, image, w.t, c->H, c->W, c->h[0], c->w[0], total);
  if (int rc = linear(w.t, 48, p[DN_W], p[DN_B], out, (long long)P, c->dims[0], 48, c->dims[0], kActNone, nullptr, kForm3Gelu, st)) return rc;
  row_ln(out, p[DN_LN_W], p[DN_LN_B], out, c->dims[0], P, st);
  return AXVS_OK;
}

// downsample layer i (1..3): x rows [P_{i-1}][dims[i-1]] -> out rows [P_i][dims[i]]
int down(const AxvsCnxCfg* c, int i, float* const* p, const CnxWs& w, const float* x, float* out, hipStream_t st) {
  const int C = c->dims[i - 1];
  const size_t P = pixels_of(c, i), total = P * 4;
  hipLaunchKernelGGL(cnx_down_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, st, x, (const float*)p[DN_LN_W], (const float*)p[DN_LN_B], w.t, C,
                     c->h[i - 1], c->w[i - 1], c->h[i], c->w[i], total);
  return linear(w.t, 4 * C, p[DN_W], p[DN_B], out, (long long)P, c->dims[i], 4 * C, c->dims[i], kActNone, nullptr, kForm3Gelu, st);
}

template <int TH>
int dwln_launch(const AxvsCnxCfg* c, int i, float* const* p, const float* x, float* out, hipStream_t st) {
  auto* fn = cnx_dwln_kernel<TH>;
  if (int rc = ensure_max_lds(reinterpret_cast<const void*>(fn))) return rc;
  const dim3 grid((unsigned)((c->w[i] + kCnxTW - 1) / kCnxTW), (unsigned)((c->h[i] + TH - 1) / TH), (unsigned)c->N);
  hipLaunchKernelGGL(fn, grid, dim3(256), (size_t)cnx_dw_lds(TH), st, x, (const float*)p[BK_DW_W], (const float*)p[BK_DW_B], (const float*)p[BK_LN_W],
                     (const float*)p[BK_LN_B], out, c->dims[i], c->h[i], c->w[i]);
  return AXVS_OK;
}

// the tallest tile (8, 4, 2 rows of 16 pixels) that gives kCnxDwWgs workgroups, else the shortest
int dwln(const AxvsCnxCfg* c, int i, float* const* p, const float* x, float* out, hipStream_t st) {
  const long long cols = (long long)c->N * ((c->w[i] + kCnxTW - 1) / kCnxTW);
  if (cols * ((c->h[i] + 7) / 8) >= kCnxDwWgs) return dwln_launch<8>(c, i, p, x, out, st);
  if (cols * ((c->h[i] + 3) / 4) >= kCnxDwWgs) return dwln_launch<4>(c, i, p, x, out, st);
  return dwln_launch<2>(c, i, p, x, out, st);
}

// one block of stage i: x rows [P][C] -> y rows [P][C]
int block(const AxvsCnxCfg* c, int i, float* const* p, const CnxWs& w, const float* x, float* y, hipStream_t st) {
  const int C = c->dims[i], K = 4 * C, hw = c->h[i] * c->w[i];
  const long long P = (long long)pixels_of(c, i);
  if (int rc = dwln(c, i, p, x, w.t, st)) return rc;
  if (int rc = linear(w.t, C, p[BK_W1], p[BK_B1], w.hid, P, K, C, K, kActGelu, nullptr, kForm3Gelu, st)) return rc;
  if (!c->v2) return linear(w.hid, K, p[BK_W2], p[BK_B2], y, P, C, K, C, kActNone, x, kForm3Gelu, st);
  const int nch = grn_chunks(c, i);
  hipLaunchKernelGGL(cnx_sumsq_kernel, dim3((unsigned)((K + 255) / 256), (unsigned)nch, (unsigned)c->N), dim3(256), 0, st, (const float*)w.hid, w.part, K, hw);
  hipLaunchKernelGGL(cnx_grn_gx_kernel, dim3((unsigned)((K + 255) / 256), (unsigned)c->N), dim3(256), 0, st, (const float*)w.part, w.s, K, nch);
  hipLaunchKernelGGL(cnx_grn_scale_kernel, dim3((unsigned)c->N), dim3(256), 0, st, (const float*)p[BK_GRN], w.s, K);
  const size_t n4 = (size_t)C * K / 4;
  for (int n = 0; n < c->N; ++n) {          // (one buffer for W2 diag(s_n): the stream orders frame n's GEMM in front of frame n + 1's copy)
    hipLaunchKernelGGL(cnx_scale_w_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, (const float*)p[BK_W2], (const float*)(w.s + (size_t)n * K), w.w2s, K,
                       n4);
    const size_t r0 = (size_t)n * hw;
    if (int rc = linear(w.hid + r0 * K, K, w.w2s, p[BK_B2], y + r0 * C, hw, C, K, C, kActNone, x + r0 * C, kForm3Gelu, st)) return rc;
  }
  return AXVS_OK;
}

}  // namespace

size_t axvs_cnx_packed_bytes(const AxvsCnxCfg* cfg) {
  if (cnx_check(cfg)) return 0;
  return cnx_weights(nullptr, cfg).bytes;
}

int axvs_cnx_pack(const AxvsCnxDownParams* downs, const AxvsCnxBlockParams* blocks, const AxvsCnxCfg* cfg, void* packed, void* stream) {
  if (int rc = cnx_check(cfg)) return rc;
  if (!downs || !blocks || !packed) return fail(AXVS_ERR_ARG, "null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const CnxW w = cnx_weights(packed, cfg);
  size_t n[BK_N];
  int index = 0;
  for (int i = 0; i < kStages; ++i) {
    down_sizes(cfg, i, n);
    if (int rc = copy_slots(w.down[i], downs + i, n, DN_N, "downsample layer", i, st)) return rc;
    block_sizes(cfg, i, n);
    for (int j = 0; j < cfg->depths[i]; ++j, ++index)
      if (int rc = copy_slots(w.block[i][j], blocks + index, n, BK_N, "block", index, st)) return rc;
  }
  return AXVS_OK;
}

size_t axvs_cnx_workspace_bytes(const AxvsCnxCfg* cfg) {
  if (cnx_check(cfg)) return 0;
  return cnx_carve(nullptr, cfg).bytes;
}

int axvs_cnx_fwd(const AxvsCnxCfg* cfg, const void* packed, const float* image, float* const* outputs, void* workspace, long long workspace_bytes,
                 void* stream) {
  if (int rc = cnx_check(cfg)) return rc;
  if (int rc = cnx_check_sizes(cfg)) return rc;
  if (!packed || !image || !outputs || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  const CnxWs w = cnx_carve(workspace, cfg);
  if (int rc = check_ws(workspace_bytes, w.bytes)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const CnxW p = cnx_weights(const_cast<void*>(packed), cfg);
  float *cur = w.x, *nxt = w.y;
  for (int i = 0; i < kStages; ++i) {
    if (i == 0) {
      if (int rc = stem(cfg, p.down[0], w, image, cur, st)) return rc;
      if (outputs[0]) rows_to_nchw(cur, outputs[0], cfg->N, cfg->dims[0], cfg->h[0] * cfg->w[0], st);
    } else {
      if (int rc = down(cfg, i, p.down[i], w, cur, nxt, st)) return rc;
      std::swap(cur, nxt);
    }
    for (int j = 0; j < cfg->depths[i]; ++j) {
      if (int rc = block(cfg, i, p.block[i][j], w, cur, nxt, st)) return rc;
      std::swap(cur, nxt);
    }
    if (outputs[i + 1]) rows_to_nchw(cur, outputs[i + 1], cfg->N, cfg->dims[i], cfg->h[i] * cfg->w[i], st);
  }
  return last_launch_status();
}

int axvs_cnx_stem_fwd(const AxvsCnxCfg* cfg, const void* packed, const float* image, float* out, void* workspace, long long workspace_bytes, void* stream) {
  if (int rc = cnx_check(cfg)) return rc;
  if (cfg->H < 1 || cfg->W < 1 || cfg->H > 65535 || cfg->W > 65535 || cfg->h[0] != (cfg->H + 3) / 4 || cfg->w[0] != (cfg->W + 3) / 4)
    return fail(AXVS_ERR_ARG, "image %d x %d (in 1..65535) must give the stem's map %d x %d", cfg->H, cfg->W, cfg->h[0], cfg->w[0]);
  if (!packed || !image || !out || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  const CnxWs w = cnx_carve(workspace, cfg);
  if (int rc = check_ws(workspace_bytes, w.bytes)) return rc;
  const CnxW p = cnx_weights(const_cast<void*>(packed), cfg);
  if (int rc = stem(cfg, p.down[0], w, image, out, static_cast<hipStream_t>(stream))) return rc;
  return last_launch_status();
}

int axvs_cnx_down_fwd(const AxvsCnxCfg* cfg, const void* packed, int index, const float* x, float* out, void* workspace, long long workspace_bytes,
                      void* stream) {
  if (int rc = cnx_check(cfg)) return rc;
  if (index < 1 || index > 3) return fail(AXVS_ERR_ARG, "index=%d must be in 1..3", index);
  if (cfg->h[index] != (cfg->h[index - 1] + 1) / 2 || cfg->w[index] != (cfg->w[index - 1] + 1) / 2)
    return fail(AXVS_ERR_ARG, "downsample layer %d: map %d x %d does not give %d x %d", index, cfg->h[index - 1], cfg->w[index - 1], cfg->h[index], cfg->w[index]);
  if (!packed || !x || !out || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  const CnxWs w = cnx_carve(workspace, cfg);
  if (int rc = check_ws(workspace_bytes, w.bytes)) return rc;
  const CnxW p = cnx_weights(const_cast<void*>(packed), cfg);
  if (int rc = down(cfg, index, p.down[index], w, x, out, static_cast<hipStream_t>(stream))) return rc;
  return last_launch_status();
}

int axvs_cnx_dwln_fwd(const AxvsCnxCfg* cfg, const void* packed, int block_index, const float* x, float* out, void* stream) {
  if (int rc = cnx_check(cfg)) return rc;
  int i, j;
  if (int rc = locate(cfg->depths, block_index, "network's", &i, &j)) return rc;
  if (!packed || !x || !out || x == out) return fail(AXVS_ERR_ARG, "null pointer, or out == x");
  const CnxW p = cnx_weights(const_cast<void*>(packed), cfg);
  if (int rc = dwln(cfg, i, p.block[i][j], x, out, static_cast<hipStream_t>(stream))) return rc;
  return last_launch_status();
}

int axvs_cnx_block_fwd(const AxvsCnxCfg* cfg, const void* packed, int block_index, const float* x, float* out, void* workspace, long long workspace_bytes,
                       void* stream) {
  if (int rc = cnx_check(cfg)) return rc;
  int i, j;
  if (int rc = locate(cfg->depths, block_index, "network's", &i, &j)) return rc;
  if (!packed || !x || !out || !workspace || x == out) return fail(AXVS_ERR_ARG, "null pointer, or out == x");
  const CnxWs w = cnx_carve(workspace, cfg);
  if (int rc = check_ws(workspace_bytes, w.bytes)) return rc;
  const CnxW p = cnx_weights(const_cast<void*>(packed), cfg);
  if (int rc = block(cfg, i, p.block[i][j], w, x, out, static_cast<hipStream_t>(stream))) return rc;
  return last_launch_status();
}
