// C-ABI entry points of the video instance post-processing (include/axvs.h: axvs_video_instance_*) and the launch sequence behind them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "axvs_host.h"
#include "axvs_vis.h"

using namespace axvs;

namespace {

int vis_check(const AxvsVisCfg* c) {
  if (!c) return fail(AXVS_ERR_ARG, "null pointer (cfg)");
  if (c->Q <= 0 || c->Q > kVisMaxQ) return fail(AXVS_ERR_ARG, "Q=%d queries must be in 1..%d", c->Q, kVisMaxQ);
  if (c->K1 < 2) return fail(AXVS_ERR_ARG, "need C + 1 = %d >= 2 class logits", c->K1);
  const long long keys = (long long)c->Q * (c->K1 - 1);
  if (keys > kVisMaxKeys) return fail(AXVS_ERR_ARG, "Q*C = %lld class scores must be at most 2^17 = %d", keys, kVisMaxKeys);
  if (c->k_cand <= 0 || c->k_cand > kVisMaxCand || c->k_cand > keys)
    return fail(AXVS_ERR_ARG, "max_per_image=%d candidates must be in 1..min(Q*C = %lld, %d)", c->k_cand, keys, kVisMaxCand);
  if (c->k_out <= 0 || c->k_out > c->k_cand) return fail(AXVS_ERR_ARG, "keep_per_frame=%d must be in 1..max_per_image = %d", c->k_out, c->k_cand);
  if (c->num_things < 0) return fail(AXVS_ERR_ARG, "num_things_classes=%d must not be negative", c->num_things);
  if (c->T <= 0 || c->num_frames <= 0 || c->num_frames > c->T || c->num_frames > 65535)
    return fail(AXVS_ERR_ARG, "num_frames=%d must be in 1..min(T = %d, 65535)", c->num_frames, c->T);
  if (c->h <= 0 || c->w <= 0 || c->image_h <= 0 || c->image_w <= 0 || c->H <= 0 || c->W <= 0)
    return fail(AXVS_ERR_ARG, "h=%d, w=%d, batch input %d x %d and original %d x %d must be positive", c->h, c->w, c->image_h, c->image_w, c->H, c->W);
  if (c->crop_h <= 0 || c->crop_h > c->image_h || c->crop_w <= 0 || c->crop_w > c->image_w)
    return fail(AXVS_ERR_ARG, "img_shape %d x %d must lie inside the batch input %d x %d", c->crop_h, c->crop_w, c->image_h, c->image_w);
  if ((long long)c->H * c->W >= (1ll << 31) || (long long)c->h * c->w * c->Q >= (1ll << 31))
    return fail(AXVS_ERR_ARG, "H*W = %lld output pixels and Q*h*w = %lld logits per frame must be below 2^31", (long long)c->H * c->W,
                (long long)c->h * c->w * c->Q);
  return AXVS_OK;
}

struct VisWs {
  unsigned long long* keys;
  int* ref_list;
  VisAcc acc;
  char* zero_from;
  size_t zero_bytes, bytes;
};

VisWs vis_carve(void* ws, const AxvsVisCfg* c) {
  const size_t FQ = (size_t)c->num_frames * c->Q;
  Carver cv(ws);
  VisWs w;
  w.keys = cv.take<unsigned long long>((size_t)c->Q * (c->K1 - 1));
  w.ref_list = cv.take<int>(c->Q);
  // the accumulators the statistics pass adds into: one block, zeroed by one memset
  const size_t z0 = cv.off;
  w.acc.sum = cv.take<unsigned long long>(FQ);
  w.acc.area = cv.take<unsigned>(FQ);
  w.acc.box = cv.take<unsigned>(FQ * 4);
  w.zero_from = ws ? static_cast<char*>(ws) + z0 : nullptr;
  w.zero_bytes = cv.off - z0;
  w.bytes = cv.off;
  return w;
}

PanAxis axis(int in, int out) { return PanAxis{in, out, (float)in / (float)out}; }      // area_pixel_compute_scale<float>, align_corners=False

template <int DT>
void vis_launch_tiles(const void* logits, const PanGeom& g, const AxvsVisCfg* c, const VisWs& w, const VisTabs& tb, void* masks, bool emit, hipStream_t st) {
  const int F = c->num_frames;
  const int ntile = ((g.H + kVisTileH - 1) / kVisTileH) * ((g.W + kVisTileW - 1) / kVisTileW);
  // about 2048 workgroups in all: each accumulates (or emits) over a run of tiles of one frame
  const int want = std::min(ntile, std::max(1, (2048 + F - 1) / F));
  const int per = (ntile + want - 1) / want, wgs = (ntile + per - 1) / per;
  const dim3 grid(wgs, F), block(kVisThreads);
  if (!emit)
    hipLaunchKernelGGL((vis_tile_kernel<DT, kVisStats>), grid, block, 0, st, logits, g, (const int*)w.ref_list, 0, (const int*)(tb.head + 1), 0, per, c->k_out,
                       w.acc, masks);
  else if (c->mask_bits)
    hipLaunchKernelGGL((vis_tile_kernel<DT, kVisEmitBits>), grid, block, 0, st, logits, g, (const int*)tb.query, c->k_out, (const int*)tb.count, 1, per,
                       c->k_out, w.acc, masks);
  else
    hipLaunchKernelGGL((vis_tile_kernel<DT, kVisEmitU8>), grid, block, 0, st, logits, g, (const int*)tb.query, c->k_out, (const int*)tb.count, 1, per,
                       c->k_out, w.acc, masks);
}

}  // namespace

size_t axvs_video_instance_workspace_bytes(const AxvsVisCfg* cfg) {
  if (vis_check(cfg)) return 0;
  return vis_carve(nullptr, cfg).bytes;
}

int axvs_video_instance_fwd(const AxvsVisCfg* cfg, const float* mask_cls, const void* mask_pred, int mask_dtype, void* out_masks, int* table_ints,
                            float* table_floats, void* workspace, long long workspace_bytes, void* stream) {
  if (int rc = vis_check(cfg)) return rc;
  if (mask_dtype != AXVS_F32 && mask_dtype != AXVS_F16 && mask_dtype != AXVS_BF16)
    return fail(AXVS_ERR_ARG, "mask dtype %d is not AXVS_F16 / AXVS_BF16 / AXVS_F32", mask_dtype);
  if (!mask_cls || !mask_pred || !out_masks || !table_ints || !table_floats || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  const VisWs w = vis_carve(workspace, cfg);
  if (int rc = check_ws(workspace_bytes, w.bytes)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int F = cfg->num_frames, K = cfg->k_cand, Ko = cfg->k_out;
  const VisTabs tb = vis_tabs(table_ints, table_floats, F, K, Ko);
  PanGeom g;
  g.N = cfg->Q, g.T = cfg->T, g.h = cfg->h, g.w = cfg->w, g.H = cfg->H, g.W = cfg->W, g.two = 1, g.ac = 0, g.thr = 0.f;
  g.y1 = axis(cfg->h, cfg->image_h), g.x1 = axis(cfg->w, cfg->image_w);
  g.y2 = axis(cfg->crop_h, cfg->H), g.x2 = axis(cfg->crop_w, cfg->W);
  if (hipMemsetAsync(w.zero_from, 0, w.zero_bytes, st) != hipSuccess) return fail(AXVS_ERR_LAUNCH, "hipMemsetAsync failed");
  hipLaunchKernelGGL(vis_candidate_kernel, dim3(1), dim3(kVisCandThreads), 0, st, mask_cls, cfg->Q, cfg->K1 - 1, K, cfg->num_things, w.keys, tb, w.ref_list);
  auto tiles = [&](bool emit) {
    if (mask_dtype == AXVS_F32) vis_launch_tiles<kPanF32>(mask_pred, g, cfg, w, tb, out_masks, emit, st);
    else if (mask_dtype == AXVS_F16) vis_launch_tiles<kPanF16>(mask_pred, g, cfg, w, tb, out_masks, emit, st);
    else vis_launch_tiles<kPanBf16>(mask_pred, g, cfg, w, tb, out_masks, emit, st);
  };
  tiles(false);
  hipLaunchKernelGGL(vis_select_kernel, dim3(F), dim3(kVisMaxCand), 0, st, tb, w.acc, cfg->Q, K, Ko, cfg->H, cfg->W);
  tiles(true);
  return last_launch_status();
}
