// C-ABI entry points of the ResNet bottleneck backbone (include/axvs.h: axvs_rn_*) and the launch sequence behind them.  Every 1x1
// convolution is one linear() of axvs_eval_host.h (the three-piece split-precision GEMM in its form with the after-the-residual epilogues:
// the folded BatchNorm is its bias, the block's last one ends in relu(... + shortcut)); a stride-2 1x1 convolution reads the rows
// rn_gather2_kernel picked.  The stem, the gather and the 3x3 convolution: axvs_resnet.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "axvs_eval_host.h"
#include "axvs_layout.h"
#include "axvs_resnet.h"

using namespace axvs;

namespace {

constexpr int kStages = 4, kMaxBlocks = 64, kMaxWidth = 512, kMaxStem = 128, kMaxC = 2048;
constexpr int kRnConv3Wgs = 256;         // the wide output-channel tile is taken where it still gives this many workgroups (one per compute unit)
constexpr int kActReluAfterRes = 4;      // GemmEpi::relu under GemmNtForm::gelu (axvs_gemm_nt.h)

// the slots of AxvsRnStemParams / AxvsRnBlockParams, in declaration order (axial_vs_amd/_params.py states the same order)
enum { ST_W, ST_B, ST_N };
enum { BK_W1, BK_B1, BK_W2, BK_B2, BK_W3, BK_B3, BK_WS, BK_BS, BK_N };
static_assert(sizeof(AxvsRnStemParams) == ST_N * sizeof(void*) && sizeof(AxvsRnBlockParams) == BK_N * sizeof(void*), "slot lists out of step");

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int in_channels(const AxvsRnCfg* c, int i) { return i == 0 ? c->stem_channels : c->out_channels[i - 1]; }
inline bool has_shortcut(const AxvsRnCfg* c, int i, int j) { return j == 0 && in_channels(c, i) != c->out_channels[i]; }
inline int block_stride(const AxvsRnCfg* c, int i, int j) { return j == 0 ? c->stride[i] : 1; }
// the stage's output map (its input map: cfg->h[i] x cfg->w[i])
inline int out_h(const AxvsRnCfg* c, int i) { return cdiv(c->h[i], c->stride[i]); }
inline int out_w(const AxvsRnCfg* c, int i) { return cdiv(c->w[i], c->stride[i]); }
inline int stem_conv(int x) { return (x + 1) / 2; }             // 7x7 / stride 2 / padding 3, and the 3x3 / stride 2 / padding 1 pool alike

// what depends on the channel configuration alone (the packed blob does)
int rn_check_channels(const AxvsRnCfg* c) {
  if (!c) return fail(AXVS_ERR_ARG, "null pointer (cfg)");
  if (c->in_channels != 3) return fail(AXVS_ERR_ARG, "in_channels=%d: the stem kernel takes 3-channel images", c->in_channels);
  if (c->stem_channels < 16 || c->stem_channels > kMaxStem || c->stem_channels % 16)
    return fail(AXVS_ERR_ARG, "stem: %d channels must be a multiple of 16 in 16..%d", c->stem_channels, kMaxStem);
  for (int i = 0; i < kStages; ++i) {
    if (c->blocks[i] < 1 || c->blocks[i] > kMaxBlocks) return fail(AXVS_ERR_ARG, "stage %d: %d blocks must be in 1..%d", i, c->blocks[i], kMaxBlocks);
    if (c->width[i] < 32 || c->width[i] > kMaxWidth || c->width[i] % 32)
      return fail(AXVS_ERR_ARG, "stage %d: bottleneck width %d must be a multiple of 32 in 32..%d", i, c->width[i], kMaxWidth);
    if (c->out_channels[i] < 16 || c->out_channels[i] > kMaxC || c->out_channels[i] % 16)
      return fail(AXVS_ERR_ARG, "stage %d: %d output channels must be a multiple of 16 in 16..%d", i, c->out_channels[i], kMaxC);
    if (c->stride[i] < 1 || c->stride[i] > 2) return fail(AXVS_ERR_ARG, "stage %d: stride %d must be 1 or 2", i, c->stride[i]);
    if (c->dilation[i] < 1 || c->dilation[i] > 2) return fail(AXVS_ERR_ARG, "stage %d: dilation %d must be 1 or 2", i, c->dilation[i]);
    if (c->stride[i] == 2 && c->dilation[i] == 2)
      return fail(AXVS_ERR_ARG, "stage %d: stride 2 together with dilation 2 is not built (the reference dilates res5 in place of its stride)", i);
    if (c->stride[i] == 2 && in_channels(c, i) == c->out_channels[i])
      return fail(AXVS_ERR_ARG, "stage %d: stride 2 needs a projection shortcut, but the stage keeps its %d channels", i, c->out_channels[i]);
  }
  return AXVS_OK;
}

int rn_check(const AxvsRnCfg* c) {
  if (int rc = rn_check_channels(c)) return rc;
  if (c->N < 1 || c->N > 4096) return fail(AXVS_ERR_ARG, "N=%d frames must be in 1..4096", c->N);
  for (int i = 0; i < kStages; ++i)
    if (c->h[i] < 1 || c->w[i] < 1 || c->h[i] > 16383 || c->w[i] > 16383 || (long long)c->N * c->h[i] * c->w[i] >= (1ll << 24))
      return fail(AXVS_ERR_ARG, "stage %d: N*h*w = %d*%d*%d pixels must be in 1..2^24-1, h and w <= 16383", i, c->N, c->h[i], c->w[i]);
  return AXVS_OK;
}

int rn_check_image(const AxvsRnCfg* c) {
  if (c->H < 1 || c->W < 1 || c->H > 32767 || c->W > 32767) return fail(AXVS_ERR_ARG, "image %d x %d: H and W must be in 1..32767", c->H, c->W);
  const int hp = stem_conv(stem_conv(c->H)), wp = stem_conv(stem_conv(c->W));
  if (c->h[0] != hp || c->w[0] != wp)
    return fail(AXVS_ERR_ARG, "stage 0: map %d x %d, but an image of %d x %d gives %d x %d", c->h[0], c->w[0], c->H, c->W, hp, wp);
  return AXVS_OK;
}

// the whole network: the image's size decides every map's
int rn_check_sizes(const AxvsRnCfg* c) {
  if (int rc = rn_check_image(c)) return rc;
  for (int i = 1; i < kStages; ++i)
    if (c->h[i] != out_h(c, i - 1) || c->w[i] != out_w(c, i - 1))
      return fail(AXVS_ERR_ARG, "stage %d: map %d x %d, but stage %d leaves %d x %d", i, c->h[i], c->w[i], i - 1, out_h(c, i - 1), out_w(c, i - 1));
  return AXVS_OK;
}

// ---- the packed weights: fp32 slots one after the other; the 3x3 weight's slot holds its split pieces (rn_w3_elems 16-bit values) --------
void block_sizes(const AxvsRnCfg* c, int i, int j, size_t* n) {
  const size_t cin = j == 0 ? in_channels(c, i) : c->out_channels[i], bw = c->width[i], co = c->out_channels[i];
  n[BK_W1] = bw * cin, n[BK_B1] = bw, n[BK_W2] = rn_w3_elems((int)bw) / 2, n[BK_B2] = bw, n[BK_W3] = co * bw, n[BK_B3] = co;
  n[BK_WS] = has_shortcut(c, i, j) ? co * cin : 0, n[BK_BS] = has_shortcut(c, i, j) ? co : 0;
}

struct RnW {
  float* stem[ST_N];
  float* block[kStages][kMaxBlocks][BK_N];
  size_t bytes;
};

RnW rn_weights(void* blob, const AxvsRnCfg* c) {
  Carver cv(blob);
  RnW w = {};
  const size_t ns[ST_N] = {rn_stem_w_elems(c->stem_channels) / 2, (size_t)c->stem_channels};      // (the weight's slot holds its split pieces)
  carve_slots(cv, ns, ST_N, w.stem);
  size_t n[BK_N];
  for (int i = 0; i < kStages; ++i)
    for (int j = 0; j < c->blocks[i]; ++j) {
      block_sizes(c, i, j, n);
      carve_slots(cv, n, BK_N, w.block[i][j]);
    }
  w.bytes = cv.off;
  return w;
}

// ---- the workspace: sized for the largest stage, carved once -----------------------------------------------------------------------------------
struct RnWs {
  float *x, *y;      // a block's input and output rows, swapped from block to block
  float *g;          // the gathered rows of a stride-2 1x1 convolution
  float *t1, *t2;    // conv1's and conv2's rows
  float *sc;         // the projected shortcut
  size_t bytes;
};

RnWs rn_carve(void* ws, const AxvsRnCfg* c) {
  size_t xy = 0, g = 0, t = 0, sc = 0;
  for (int i = 0; i < kStages; ++i) {
    const size_t Pi = (size_t)c->N * c->h[i] * c->w[i], Po = (size_t)c->N * out_h(c, i) * out_w(c, i);
    xy = std::max(xy, std::max(Pi * in_channels(c, i), Po * c->out_channels[i]));
    t = std::max(t, Pi * c->width[i]);
    if (c->stride[i] == 2) g = std::max(g, Po * in_channels(c, i));
    sc = std::max(sc, Po * c->out_channels[i]);
  }
  Carver cv(ws);
  RnWs w = {};
  w.x = cv.f(xy), w.y = cv.f(xy), w.g = cv.f(g), w.t1 = cv.f(t), w.t2 = cv.f(t), w.sc = cv.f(sc);
  w.bytes = cv.off;
  return w;
}

// ---- launches -------------------------------------------------------------------------------------------------------------------------------
// image -> out rows [N][h[0]][w[0]][stem_channels]
int stem(const AxvsRnCfg* c, float* const* p, const float* image, float* out, hipStream_t st) {
  if (int rc = ensure_max_lds(reinterpret_cast<const void*>(rn_stem_kernel))) return rc;
  const dim3 grid((unsigned)cdiv(c->w[0], kRnStemPW), (unsigned)cdiv(c->h[0], kRnStemPH), (unsigned)c->N);
  hipLaunchKernelGGL(rn_stem_kernel, grid, dim3(256), (size_t)kRnStemLds, st, image, reinterpret_cast<const u16*>(p[ST_W]), (const float*)p[ST_B], out, c->stem_channels, c->H, c->W,
                     stem_conv(c->H), stem_conv(c->W), c->h[0], c->w[0]);
  return AXVS_OK;
}

void gather2(const float* x, float* y, int N, int C, int h, int w, hipStream_t st) {
  const int h2 = cdiv(h, 2), w2 = cdiv(w, 2);
  const size_t total = (size_t)N * h2 * w2 * (C / 4);
  hipLaunchKernelGGL(rn_gather2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, y, C / 4, h, w, h2, w2, total);
}

template <int S, int BN>
int conv3_launch(const float* x, const u16* wp, const float* bias, float* y, int N, int C, int h, int w, int d, hipStream_t st) {
  using K = RnConv3<S, BN>;
  auto* fn = rn_conv3_kernel<S, BN>;
  if (int rc = ensure_max_lds(reinterpret_cast<const void*>(fn))) return rc;
  const int ho = cdiv(h, S), wo = cdiv(w, S);
  const dim3 grid((unsigned)cdiv(wo, K::TW), (unsigned)cdiv(ho, K::TH), (unsigned)(N * cdiv(C, BN)));
  hipLaunchKernelGGL(fn, grid, dim3(256), (size_t)K::lds(d), st, x, wp, bias, y, C, h, w, ho, wo, d);
  return AXVS_OK;
}

// x rows [N][h][w][C] -> y rows [N][ceil(h / s)][ceil(w / s)][C]
int conv3(const float* x, const float* wp, const float* bias, float* y, int N, int C, int h, int w, int s, int d, hipStream_t st) {
  const u16* p = reinterpret_cast<const u16*>(wp);
  // 64 output channels per workgroup where 128 would leave compute units without one (an element's sum has the same order either way)
  const long long wgs128 = (long long)N * cdiv(C, 128) * cdiv(cdiv(w, s), 16) * cdiv(cdiv(h, s), s == 1 ? 8 : 4);
  const bool narrow = C <= 64 || wgs128 < kRnConv3Wgs;
  if (s == 1) return narrow ? conv3_launch<1, 64>(x, p, bias, y, N, C, h, w, d, st) : conv3_launch<1, 128>(x, p, bias, y, N, C, h, w, d, st);
  return narrow ? conv3_launch<2, 64>(x, p, bias, y, N, C, h, w, d, st) : conv3_launch<2, 128>(x, p, bias, y, N, C, h, w, d, st);
}

// where block j of stage i puts its stride: (conv1's, conv2's); the map conv2 reads
struct BlockGeom {
  int s1, s2, hin, win, hm, wm, ho, wo;
};
BlockGeom geom(const AxvsRnCfg* c, int i, int j) {
  BlockGeom g;
  const int s = block_stride(c, i, j);
  g.s1 = c->stride_in_1x1 ? s : 1, g.s2 = c->stride_in_1x1 ? 1 : s;
  g.hin = j == 0 ? c->h[i] : out_h(c, i), g.win = j == 0 ? c->w[i] : out_w(c, i);
  g.hm = cdiv(g.hin, g.s1), g.wm = cdiv(g.win, g.s1);
  g.ho = cdiv(g.hm, g.s2), g.wo = cdiv(g.wm, g.s2);
  return g;
}

// block j of stage i: x rows [N][hin][win][cin] -> y rows [N][ho][wo][out_channels[i]]
int block(const AxvsRnCfg* c, int i, int j, float* const* p, const RnWs& w, const float* x, float* y, hipStream_t st) {
  const BlockGeom g = geom(c, i, j);
  const int cin = j == 0 ? in_channels(c, i) : c->out_channels[i], bw = c->width[i], co = c->out_channels[i], s = block_stride(c, i, j);
  const long long Pm = (long long)c->N * g.hm * g.wm, Po = (long long)c->N * g.ho * g.wo;
  const float* xs = x;                     // x at the block's output positions: what a stride-2 1x1 convolution reads
  if (s == 2 && (c->stride_in_1x1 || p[BK_WS])) {
    gather2(x, w.g, c->N, cin, g.hin, g.win, st);
    xs = w.g;
  }
  if (int rc = linear(g.s1 == 2 ? xs : x, cin, p[BK_W1], p[BK_B1], w.t1, Pm, bw, cin, bw, kActRelu, nullptr, kForm3Gelu, st)) return rc;
  if (int rc = conv3(w.t1, p[BK_W2], p[BK_B2], w.t2, c->N, bw, g.hm, g.wm, g.s2, c->dilation[i], st)) return rc;
  const float* res = x;                    // the identity shortcut: a block without projection has stride 1
  if (p[BK_WS]) {
    if (int rc = linear(xs, cin, p[BK_WS], p[BK_BS], w.sc, Po, co, cin, co, kActNone, nullptr, kForm3Gelu, st)) return rc;
    res = w.sc;
  }
  return linear(w.t2, bw, p[BK_W3], p[BK_B3], y, Po, co, bw, co, kActReluAfterRes, res, kForm3Gelu, st);
}

int locate_block(const AxvsRnCfg* c, int block_index, int* i, int* j) { return locate(c->blocks, block_index, "network's", i, j); }

}  // namespace

size_t axvs_rn_packed_bytes(const AxvsRnCfg* cfg) {
  if (rn_check_channels(cfg)) return 0;
  return rn_weights(nullptr, cfg).bytes;
}

int axvs_rn_pack(const AxvsRnStemParams* stem_params, const AxvsRnBlockParams* blocks, const AxvsRnCfg* cfg, void* packed, void* stream) {
  if (int rc = rn_check_channels(cfg)) return rc;
  if (!stem_params || !blocks || !packed) return fail(AXVS_ERR_ARG, "null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const RnW w = rn_weights(packed, cfg);
  const size_t ns[ST_N] = {0, (size_t)cfg->stem_channels};      // (the weight is not a copy: split below)
  if (int rc = copy_slots(w.stem, stem_params, ns, ST_N, "stem", 0, st)) return rc;
  if (!stem_params->w) return fail(AXVS_ERR_ARG, "null pointer (stem, parameter %d)", (int)ST_W);
  {
    const size_t total = (size_t)(cfg->stem_channels / 16) * kRnStemSteps * 64;      // one thread per (fragment triple, lane)
    hipLaunchKernelGGL(rn_pack_stem_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, stem_params->w, reinterpret_cast<u16*>(w.stem[ST_W]),
                       cfg->stem_channels, total);
  }
  size_t n[BK_N];
  int index = 0;
  for (int i = 0; i < kStages; ++i)
    for (int j = 0; j < cfg->blocks[i]; ++j, ++index) {
      block_sizes(cfg, i, j, n);
      n[BK_W2] = 0;                          // (not a copy: split below)
      if (int rc = copy_slots(w.block[i][j], blocks + index, n, BK_N, "block", index, st)) return rc;
      if (!blocks[index].w2) return fail(AXVS_ERR_ARG, "null pointer (block %d, parameter %d)", index, (int)BK_W2);
      const int bw = cfg->width[i];
      const size_t total = rn_w3_elems(bw) / 24;      // one thread per (fragment triple, lane): 3 pieces x 8 values
      hipLaunchKernelGGL(rn_pack_w3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, blocks[index].w2, reinterpret_cast<u16*>(w.block[i][j][BK_W2]),
                         bw, total);
    }
  return last_launch_status();
}

size_t axvs_rn_workspace_bytes(const AxvsRnCfg* cfg) {
  if (rn_check(cfg)) return 0;
  return rn_carve(nullptr, cfg).bytes;
}

int axvs_rn_fwd(const AxvsRnCfg* cfg, const void* packed, const float* image, float* const* outputs, void* stream, void* workspace, long long workspace_bytes) {
  if (int rc = rn_check(cfg)) return rc;
  if (int rc = rn_check_sizes(cfg)) return rc;
  if (!packed || !image || !outputs || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  const RnWs w = rn_carve(workspace, cfg);
  if (int rc = check_ws(workspace_bytes, w.bytes)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const RnW p = rn_weights(const_cast<void*>(packed), cfg);
  float *cur = w.x, *nxt = w.y;
  if (int rc = stem(cfg, p.stem, image, cur, st)) return rc;
  if (outputs[0]) rows_to_nchw(cur, outputs[0], cfg->N, cfg->stem_channels, cfg->h[0] * cfg->w[0], st);
  for (int i = 0; i < kStages; ++i) {
    for (int j = 0; j < cfg->blocks[i]; ++j) {
      if (int rc = block(cfg, i, j, p.block[i][j], w, cur, nxt, st)) return rc;
      std::swap(cur, nxt);
    }
    if (outputs[i + 1]) rows_to_nchw(cur, outputs[i + 1], cfg->N, cfg->out_channels[i], out_h(cfg, i) * out_w(cfg, i), st);
  }
  return last_launch_status();
}

int axvs_rn_stem_fwd(const AxvsRnCfg* cfg, const void* packed, const float* image, float* out, void* stream) {
  if (int rc = rn_check(cfg)) return rc;
  if (int rc = rn_check_image(cfg)) return rc;
  if (!packed || !image || !out) return fail(AXVS_ERR_ARG, "null pointer");
  const RnW p = rn_weights(const_cast<void*>(packed), cfg);
  if (int rc = stem(cfg, p.stem, image, out, static_cast<hipStream_t>(stream))) return rc;
  return last_launch_status();
}

int axvs_rn_conv3_fwd(const AxvsRnCfg* cfg, const void* packed, int block_index, const float* x, float* out, void* stream) {
  if (int rc = rn_check(cfg)) return rc;
  int i, j;
  if (int rc = locate_block(cfg, block_index, &i, &j)) return rc;
  if (!packed || !x || !out || x == out) return fail(AXVS_ERR_ARG, "null pointer, or out == x");
  const RnW p = rn_weights(const_cast<void*>(packed), cfg);
  const BlockGeom g = geom(cfg, i, j);
  if (int rc = conv3(x, p.block[i][j][BK_W2], p.block[i][j][BK_B2], out, cfg->N, cfg->width[i], g.hm, g.wm, g.s2, cfg->dilation[i], static_cast<hipStream_t>(stream)))
    return rc;
  return last_launch_status();
}

int axvs_rn_block_fwd(const AxvsRnCfg* cfg, const void* packed, int block_index, const float* x, float* out, void* stream, void* workspace,
                      long long workspace_bytes) {
  if (int rc = rn_check(cfg)) return rc;
  int i, j;
  if (int rc = locate_block(cfg, block_index, &i, &j)) return rc;
  if (!packed || !x || !out || !workspace || x == out) return fail(AXVS_ERR_ARG, "null pointer, or out == x");
  const RnWs w = rn_carve(workspace, cfg);
  if (int rc = check_ws(workspace_bytes, w.bytes)) return rc;
  const RnW p = rn_weights(const_cast<void*>(packed), cfg);
  if (int rc = block(cfg, i, j, p.block[i][j], w, x, out, static_cast<hipStream_t>(stream))) return rc;
  return last_launch_status();
}
