// C-ABI entry points of Video-kMaX's pixel decoder (include/axvs.h: axvs_kmax_pix_*) and the launch sequence behind them.
// 1x1 convolutions with their folded BatchNorms: linear() of axvs_eval_host.h (with the slot-list helpers of the pack and locate()), the
// three-piece split-precision GEMM in its form with the gelu epilogues, the block's residual as `res`; everything else: axvs_kmax_pix.h.
// The gelu in front of a block or a fuse convolution is a pass of its own (the raw stage outputs are results); the gelu behind the
// width-axis attention rides in that kernel.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "axvs_eval_host.h"
#include "axvs_kmax_pix.h"

using namespace axvs;

namespace {

constexpr int kStages = 4, kMaxBlocks = 16;

// the slots of AxvsKpixBlockParams / AxvsKpixFuseParams, in declaration order (axial_vs_amd/_params.py states the same order)
enum { AX_QKV_W, AX_QKV_B, AX_EQ, AX_EK, AX_EV, AX_SIM, AX_OUT, AX_N };
enum { BK_SC_W, BK_SC_B, BK_C1_W, BK_C1_B, BK_C2_W, BK_C2_B, BK_HEIGHT, BK_WIDTH = BK_HEIGHT + AX_N, BK_C3_W = BK_WIDTH + AX_N, BK_C3_B, BK_N };
enum { FU_LN_W, FU_LN_B, FU_LOW_W, FU_LOW_B, FU_HIGH_W, FU_HIGH_B, FU_N };
static_assert(sizeof(AxvsKpixBlockParams) == BK_N * sizeof(void*) && sizeof(AxvsKpixFuseParams) == FU_N * sizeof(void*), "slot lists out of step");

inline int block_cin(const AxvsKpixCfg* c, int i, int j) { return j > 0 ? 4 * c->base[i] : i == 0 ? c->in_channels[0] : c->base[i]; }
inline int mid_channels(const AxvsKpixCfg* c, int i) { return c->axial[i] ? 2 * c->base[i] : c->base[i]; }
inline size_t pixels_of(const AxvsKpixCfg* c, int i) { return (size_t)c->N * c->h[i] * c->w[i]; }

int attn_lds_floats(int L, int b) { return kpix_attn_lds(L, b / 8, 2 * b / 8).total; }

int kpix_check(const AxvsKpixCfg* c) {
  if (!c) return fail(AXVS_ERR_ARG, "null pointer (cfg)");
  if (c->heads != kKpixHeads) return fail(AXVS_ERR_ARG, "heads=%d: the axial attention kernel is built for 8", c->heads);
  if (c->N < 1 || c->N > 4096) return fail(AXVS_ERR_ARG, "N=%d frames must be in 1..4096", c->N);
  for (int i = 0; i < kStages; ++i) {
    const int b = c->base[i];
    if (c->blocks[i] < 1 || c->blocks[i] > kMaxBlocks) return fail(AXVS_ERR_ARG, "stage %d: %d blocks must be in 1..%d", i, c->blocks[i], kMaxBlocks);
    if (c->in_channels[i] < 16 || c->in_channels[i] > 2048 || c->in_channels[i] % 16)
      return fail(AXVS_ERR_ARG, "stage %d: %d input channels must be a multiple of 16 in 16..2048", i, c->in_channels[i]);
    if (c->h[i] < 1 || c->w[i] < 1 || c->h[i] > 16383 || c->w[i] > 16383 || (long long)c->N * c->h[i] * c->w[i] >= (1ll << 24))
      return fail(AXVS_ERR_ARG, "stage %d: N*h*w = %d*%d*%d pixels must be in 1..2^24-1, h and w <= 16383", i, c->N, c->h[i], c->w[i]);
    if (c->axial[i]) {
      if (b != 512 && b != 256 && b != 128) return fail(AXVS_ERR_ARG, "stage %d: an axial stage's base filter %d must be 512, 256 or 128", i, b);
      const int L = std::max(c->h[i], c->w[i]);
      if (L > 128 || attn_lds_floats(L, b) * 4 > kKpixMaxLds)
        return fail(AXVS_ERR_ARG, "stage %d: axis length %d at base filter %d is past what the attention kernel holds in LDS (128; 80 at base filter 512)", i, L, b);
      if ((long long)c->N * L > 65535) return fail(AXVS_ERR_ARG, "stage %d: N * axis length = %d * %d sequences must be at most 65535", i, c->N, L);
    } else if (b < 32 || b > 256 || b % 32) {
      return fail(AXVS_ERR_ARG, "stage %d: a bottleneck stage's base filter %d must be a multiple of 32 in 32..256", i, b);
    }
  }
  return AXVS_OK;
}

// ---- the packed weights: fp32, BatchNorms folded (by the caller, in float64), one slot after the other -------------------------------------
void axis_sizes(int b, bool on, size_t* n) {
  const size_t dk = b / 8, dv = 2 * b / 8;
  n[AX_QKV_W] = on ? (size_t)4 * b * 2 * b : 0, n[AX_QKV_B] = on ? 4 * b : 0, n[AX_EQ] = on ? kKpixTable * dk : 0, n[AX_EK] = n[AX_EQ];
  n[AX_EV] = on ? kKpixTable * dv : 0, n[AX_SIM] = on ? 24 : 0, n[AX_OUT] = on ? 6 * b : 0;
}
void block_sizes(const AxvsKpixCfg* c, int i, int j, size_t* n) {
  const size_t b = c->base[i], cin = block_cin(c, i, j), mid = mid_channels(c, i);
  const bool sc = cin != 4 * b, ax = c->axial[i] != 0;
  n[BK_SC_W] = sc ? 4 * b * cin : 0, n[BK_SC_B] = sc ? 4 * b : 0, n[BK_C1_W] = mid * cin, n[BK_C1_B] = mid;
  n[BK_C2_W] = ax ? 0 : 9 * b * b, n[BK_C2_B] = ax ? 0 : b;
  axis_sizes((int)b, ax, n + BK_HEIGHT);
  axis_sizes((int)b, ax, n + BK_WIDTH);
  n[BK_C3_W] = 4 * b * mid, n[BK_C3_B] = 4 * b;
}
void fuse_sizes(const AxvsKpixCfg* c, int i, size_t* n) {       // the fuse in front of stage i (1..3)
  const size_t lowc = 4 * (size_t)c->base[i - 1], highc = c->in_channels[i], b = c->base[i];
  n[FU_LN_W] = highc, n[FU_LN_B] = highc;
  n[FU_LOW_W] = lowc != b ? b * lowc : 0, n[FU_LOW_B] = lowc != b ? b : 0;
  n[FU_HIGH_W] = highc != b ? b * highc : 0, n[FU_HIGH_B] = highc != b ? b : 0;
}

struct KpixW {
  float *ln0_w, *ln0_b;
  float* fuse[kStages][FU_N];                 // [0] unused
  float* block[kStages][kMaxBlocks][BK_N];
  size_t bytes;
};

KpixW kpix_weights(void* blob, const AxvsKpixCfg* c) {
  Carver cv(blob);
  KpixW w = {};
  size_t n[BK_N];
  w.ln0_w = cv.f(c->in_channels[0]), w.ln0_b = cv.f(c->in_channels[0]);
  for (int i = 0; i < kStages; ++i) {
    if (i > 0) {
      fuse_sizes(c, i, n);
      carve_slots(cv, n, FU_N, w.fuse[i]);
    }
    for (int j = 0; j < c->blocks[i]; ++j) {
      block_sizes(c, i, j, n);
      carve_slots(cv, n, BK_N, w.block[i][j]);
    }
  }
  w.bytes = cv.off;
  return w;
}

// ---- the workspace --------------------------------------------------------------------------------------------------------------------------
struct KpixWs {
  float *x, *y;          // a block's input and output rows (raw), swapped from block to block
  float *g;              // gelu(block input); a fuse's gelu(low) and its normalised high-resolution rows
  float *sc, *h1, *qkv, *a1, *a2, *lo;
  size_t bytes;
};

KpixWs kpix_carve(void* ws, const AxvsKpixCfg* c) {
  size_t xy = 0, g = 0, sc = 0, h1 = 0, qkv = 0, a = 0, lo = 0;
  for (int i = 0; i < kStages; ++i) {
    const size_t P = pixels_of(c, i), b = c->base[i];
    xy = std::max(xy, P * std::max((size_t)block_cin(c, i, 0), 4 * b));
    g = std::max(g, P * std::max((size_t)block_cin(c, i, 0), 4 * b));
    sc = std::max(sc, P * 4 * b), h1 = std::max(h1, P * mid_channels(c, i));
    a = std::max(a, P * mid_channels(c, i));
    if (c->axial[i]) qkv = std::max(qkv, P * 4 * b);
    if (i > 0) {
      g = std::max(g, P * c->in_channels[i]);
      lo = std::max(lo, pixels_of(c, i - 1) * b);
    }
  }
  Carver cv(ws);
  KpixWs w = {};
  w.x = cv.f(xy), w.y = cv.f(xy), w.g = cv.f(g), w.sc = cv.f(sc), w.h1 = cv.f(h1), w.qkv = cv.f(qkv), w.a1 = cv.f(a), w.a2 = cv.f(a), w.lo = cv.f(lo);
  w.bytes = cv.off;
  return w;
}

// ---- launches -------------------------------------------------------------------------------------------------------------------------------
void gelu(const float* x, float* y, size_t n, hipStream_t st) {
  hipLaunchKernelGGL(kpix_gelu_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, x, y, n / 4);
}

void innorm(const float* src, const float* g, const float* b, float* out, int N, int C, int hw, bool act, hipStream_t st) {
  const dim3 grid((unsigned)((hw + 31) / 32), (unsigned)N);
  if (act) hipLaunchKernelGGL((kpix_innorm_kernel<true>), grid, dim3(256), 0, st, src, g, b, out, C, hw);
  else hipLaunchKernelGGL((kpix_innorm_kernel<false>), grid, dim3(256), 0, st, src, g, b, out, C, hw);
}

void to_rows(const float* src, float* out, int N, int C, int h, int w, hipStream_t st) { nchw_to_rows(src, out, N, C, h * w, st); }

template <int DK, int DV>
int attn_launch(const float* qkv, KpixSeq sq, int L, long long nseq, float* const* ax, float* out, int act, hipStream_t st) {
  const KpixAttnLds P = kpix_attn_lds(L, DK, DV);
  auto* fn = kpix_axial_attn_kernel<DK, DV>;
  if (int rc = ensure_max_lds(reinterpret_cast<const void*>(fn))) return rc;
  hipLaunchKernelGGL(fn, dim3((unsigned)(P.L16 / P.qb + (P.L16 % P.qb ? 1 : 0)), kKpixHeads, (unsigned)nseq), dim3(256), (size_t)P.total * sizeof(float), st, qkv,
                     sq, L, (const float*)ax[AX_EQ], (const float*)ax[AX_EK], (const float*)ax[AX_EV], (const float*)ax[AX_SIM], (const float*)ax[AX_OUT], out,
                     act);
  return AXVS_OK;
}

// one axis pass over rows [N][h][w][4 b] -> [N][h][w][2 b]; axis 0: the columns of a frame (length h), 1: its rows
int attn(const AxvsKpixCfg* c, int i, int axis, float* const* ax, const float* qkv, float* out, int act, hipStream_t st) {
  const int h = c->h[i], w = c->w[i], b = c->base[i], L = axis ? w : h;
  const long long nseq = (long long)c->N * (axis ? h : w);
  if (L > 128 || attn_lds_floats(L, b) * 4 > kKpixMaxLds || nseq > 65535) return fail(AXVS_ERR_ARG, "axis length %d at base filter %d: outside the attention kernel", L, b);
  const KpixSeq sq = axis ? KpixSeq{1, w, 0, 1} : KpixSeq{w, (long long)h * w, 1, w};
  switch (b) {
    case 512: return attn_launch<64, 128>(qkv, sq, L, nseq, ax, out, act, st);
    case 256: return attn_launch<32, 64>(qkv, sq, L, nseq, ax, out, act, st);
    case 128: return attn_launch<16, 32>(qkv, sq, L, nseq, ax, out, act, st);
  }
  return fail(AXVS_ERR_ARG, "base filter %d: the attention kernel is built for 512, 256 and 128", b);
}

int conv3(const float* in, const float* wt, const float* bias, float* out, int N, int C, int h, int w, hipStream_t st) {
  if (int rc = ensure_max_lds(reinterpret_cast<const void*>(kpix_conv3_kernel))) return rc;
  hipLaunchKernelGGL(kpix_conv3_kernel, dim3((unsigned)((w + 15) / 16), (unsigned)((h + 3) / 4), (unsigned)N), dim3(256), (size_t)108 * (C + 4) * sizeof(float), st,
                     in, wt, bias, out, C, h, w);
  return AXVS_OK;
}

// SingleBlock j of stage i: x rows [P][cin] (raw) -> y rows [P][4 b] (raw)
int block(const AxvsKpixCfg* c, int i, int j, float* const* p, const KpixWs& w, const float* x, float* y, hipStream_t st) {
  const int b = c->base[i], cin = block_cin(c, i, j), mid = mid_channels(c, i), cout = 4 * b;
  const long long P = (long long)pixels_of(c, i);
  gelu(x, w.g, (size_t)P * cin, st);
  const float* res = w.g;
  if (p[BK_SC_W]) {
    if (int rc = linear(w.g, cin, p[BK_SC_W], p[BK_SC_B], w.sc, P, cout, cin, cout, kActNone, nullptr, kForm3Gelu, st)) return rc;
    res = w.sc;
  }
  if (int rc = linear(w.g, cin, p[BK_C1_W], p[BK_C1_B], w.h1, P, mid, cin, mid, kActGelu, nullptr, kForm3Gelu, st)) return rc;
  if (c->axial[i]) {
    float* const* hp = p + BK_HEIGHT;
    float* const* wp = p + BK_WIDTH;
    if (int rc = linear(w.h1, mid, hp[AX_QKV_W], hp[AX_QKV_B], w.qkv, P, 4 * b, mid, 4 * b, kActNone, nullptr, kForm3Gelu, st)) return rc;
    if (int rc = attn(c, i, 0, hp, w.qkv, w.a1, 0, st)) return rc;
    if (int rc = linear(w.a1, mid, wp[AX_QKV_W], wp[AX_QKV_B], w.qkv, P, 4 * b, mid, 4 * b, kActNone, nullptr, kForm3Gelu, st)) return rc;
    if (int rc = attn(c, i, 1, wp, w.qkv, w.a2, 1, st)) return rc;
    return linear(w.a2, mid, p[BK_C3_W], p[BK_C3_B], y, P, cout, mid, cout, kActNone, res, kForm3Gelu, st);
  }
  if (int rc = conv3(w.h1, p[BK_C2_W], p[BK_C2_B], w.a1, c->N, b, c->h[i], c->w[i], st)) return rc;
  return linear(w.a1, mid, p[BK_C3_W], p[BK_C3_B], y, P, cout, mid, cout, kActNone, res, kForm3Gelu, st);
}

PanAxis axis_of(int in, int out, int ac) {
  // area_pixel_compute_scale<float>: (in - 1) / (out - 1) with align_corners (0 for one output), else in / out
  const float s = ac ? (out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f) : (float)in / (float)out;
  return PanAxis{in, out, s};
}

// ResizedFuse in front of stage i: low rows [P_{i-1}][4 b_{i-1}] (raw), high NCHW feature -> out rows [P_i][b_i]
int fuse(const AxvsKpixCfg* c, int i, float* const* p, const KpixWs& w, const float* low, const float* high, float* out, hipStream_t st) {
  const int lowc = 4 * c->base[i - 1], highc = c->in_channels[i], b = c->base[i];
  const long long Pl = (long long)pixels_of(c, i - 1), Ph = (long long)pixels_of(c, i);
  const float* lo = low;
  if (p[FU_LOW_W]) {
    gelu(low, w.g, (size_t)Pl * lowc, st);
    if (int rc = linear(w.g, lowc, p[FU_LOW_W], p[FU_LOW_B], w.lo, Pl, b, lowc, b, kActNone, nullptr, kForm3Gelu, st)) return rc;
    lo = w.lo;
  }
  if (p[FU_HIGH_W]) {
    innorm(high, p[FU_LN_W], p[FU_LN_B], w.g, c->N, highc, c->h[i] * c->w[i], true, st);
    if (int rc = linear(w.g, highc, p[FU_HIGH_W], p[FU_HIGH_B], out, Ph, b, highc, b, kActNone, nullptr, kForm3Gelu, st)) return rc;
  } else {
    innorm(high, p[FU_LN_W], p[FU_LN_B], out, c->N, highc, c->h[i] * c->w[i], false, st);
  }
  const int ac = c->w[i - 1] % 2;
  hipLaunchKernelGGL(kpix_resize_add_kernel, dim3((unsigned)(((size_t)Ph * b / 4 + 255) / 256)), dim3(256), 0, st, lo, (const float*)out, out, c->N, b,
                     axis_of(c->h[i - 1], c->h[i], ac), axis_of(c->w[i - 1], c->w[i], ac), ac);
  return AXVS_OK;
}

}  // namespace

size_t axvs_kmax_pix_packed_bytes(const AxvsKpixCfg* cfg) {
  if (kpix_check(cfg)) return 0;
  return kpix_weights(nullptr, cfg).bytes;
}

int axvs_kmax_pix_pack(const AxvsKpixBlockParams* blocks, const AxvsKpixFuseParams* fuses, const float* ln0_w, const float* ln0_b, const AxvsKpixCfg* cfg,
                       void* packed, void* stream) {
  if (int rc = kpix_check(cfg)) return rc;
  if (!blocks || !fuses || !ln0_w || !ln0_b || !packed) return fail(AXVS_ERR_ARG, "null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const KpixW w = kpix_weights(packed, cfg);
  size_t n[BK_N];
  if (int rc = copy_f(w.ln0_w, ln0_w, cfg->in_channels[0], st)) return rc;
  if (int rc = copy_f(w.ln0_b, ln0_b, cfg->in_channels[0], st)) return rc;
  int index = 0;
  for (int i = 0; i < kStages; ++i) {
    if (i > 0) {
      fuse_sizes(cfg, i, n);
      if (int rc = copy_slots(w.fuse[i], fuses + (i - 1), n, FU_N, "fuse", i - 1, st)) return rc;
    }
    for (int j = 0; j < cfg->blocks[i]; ++j, ++index) {
      block_sizes(cfg, i, j, n);
      if (int rc = copy_slots(w.block[i][j], blocks + index, n, BK_N, "block", index, st)) return rc;
    }
  }
  return AXVS_OK;
}

size_t axvs_kmax_pix_workspace_bytes(const AxvsKpixCfg* cfg) {
  if (kpix_check(cfg)) return 0;
  return kpix_carve(nullptr, cfg).bytes;
}

int axvs_kmax_pix_decoder_fwd(const AxvsKpixCfg* cfg, const void* packed, const float* const* features, float* const* outputs, void* workspace,
                              long long workspace_bytes, void* stream) {
  if (int rc = kpix_check(cfg)) return rc;
  if (!packed || !features || !outputs || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  for (int i = 0; i < kStages; ++i)
    if (!features[i] || !outputs[i]) return fail(AXVS_ERR_ARG, "null pointer (stage %d features or output)", i);
  const KpixWs w = kpix_carve(workspace, cfg);
  if (int rc = check_ws(workspace_bytes, w.bytes)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const KpixW p = kpix_weights(const_cast<void*>(packed), cfg);
  float *cur = w.x, *nxt = w.y;
  innorm(features[0], p.ln0_w, p.ln0_b, cur, cfg->N, cfg->in_channels[0], cfg->h[0] * cfg->w[0], false, st);
  for (int i = 0; i < kStages; ++i) {
    if (i > 0) {
      if (int rc = fuse(cfg, i, p.fuse[i], w, cur, features[i], nxt, st)) return rc;
      std::swap(cur, nxt);
    }
    for (int j = 0; j < cfg->blocks[i]; ++j) {
      if (int rc = block(cfg, i, j, p.block[i][j], w, cur, nxt, st)) return rc;
      std::swap(cur, nxt);
    }
    rows_to_nchw(cur, outputs[i], cfg->N, 4 * cfg->base[i], cfg->h[i] * cfg->w[i], st);
  }
  return last_launch_status();
}

int axvs_kmax_pix_axial_attn_fwd(const AxvsKpixCfg* cfg, const void* packed, int block_index, int axis, const float* qkv, float* out, void* stream) {
  if (int rc = kpix_check(cfg)) return rc;
  int i, j;
  if (int rc = locate(cfg->blocks, block_index, "decoder's", &i, &j)) return rc;
  if (!cfg->axial[i] || axis < 0 || axis > 1) return fail(AXVS_ERR_ARG, "block %d is not an axial block, or axis=%d is not 0 / 1", block_index, axis);
  if (!packed || !qkv || !out) return fail(AXVS_ERR_ARG, "null pointer");
  const KpixW p = kpix_weights(const_cast<void*>(packed), cfg);
  if (int rc = attn(cfg, i, axis, p.block[i][j] + (axis ? BK_WIDTH : BK_HEIGHT), qkv, out, 0, static_cast<hipStream_t>(stream))) return rc;
  return last_launch_status();
}

int axvs_kmax_pix_block_fwd(const AxvsKpixCfg* cfg, const void* packed, int block_index, const float* x, float* out, void* workspace,
                            long long workspace_bytes, void* stream) {
  if (int rc = kpix_check(cfg)) return rc;
  int i, j;
  if (int rc = locate(cfg->blocks, block_index, "decoder's", &i, &j)) return rc;
  if (!packed || !x || !out || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  const KpixWs w = kpix_carve(workspace, cfg);
  if (int rc = check_ws(workspace_bytes, w.bytes)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const KpixW p = kpix_weights(const_cast<void*>(packed), cfg);
  to_rows(x, w.x, cfg->N, block_cin(cfg, i, j), cfg->h[i], cfg->w[i], st);
  if (int rc = block(cfg, i, j, p.block[i][j], w, w.x, w.y, st)) return rc;
  rows_to_nchw(w.y, out, cfg->N, 4 * cfg->base[i], cfg->h[i] * cfg->w[i], st);
  return last_launch_status();
}

int axvs_kmax_pix_fuse_fwd(const AxvsKpixCfg* cfg, const void* packed, int fuse_index, const float* low, const float* high, float* out, void* workspace,
                           long long workspace_bytes, void* stream) {
  if (int rc = kpix_check(cfg)) return rc;
  if (fuse_index < 0 || fuse_index > 2) return fail(AXVS_ERR_ARG, "fuse_index=%d must be in 0..2", fuse_index);
  if (!packed || !low || !high || !out || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  const KpixWs w = kpix_carve(workspace, cfg);
  if (int rc = check_ws(workspace_bytes, w.bytes)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const KpixW p = kpix_weights(const_cast<void*>(packed), cfg);
  const int i = fuse_index + 1;
  to_rows(low, w.y, cfg->N, 4 * cfg->base[i - 1], cfg->h[i - 1], cfg->w[i - 1], st);
  if (int rc = fuse(cfg, i, p.fuse[i], w, w.y, high, w.x, st)) return rc;
  rows_to_nchw(w.x, out, cfg->N, cfg->base[i], cfg->h[i] * cfg->w[i], st);
  return last_launch_status();
}
