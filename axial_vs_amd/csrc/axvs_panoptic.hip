// C-ABI entry points of the video panoptic post-processing (include/axvs.h: axvs_video_panoptic_*) and the launch sequence behind them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "axvs_host.h"
#include "axvs_panoptic.h"

using namespace axvs;

namespace {

int pan_check(const AxvsPanopticCfg* c) {
  if (!c) return fail(AXVS_ERR_ARG, "null pointer (cfg)");
  if (c->N <= 0 || c->N > kPanMaxN) return fail(AXVS_ERR_ARG, "N=%d mask slots must be in 1..%d", c->N, kPanMaxN);
  if (c->K1 < 2) return fail(AXVS_ERR_ARG, "need K + 1 = %d >= 2 class logits", c->K1);
  if (c->T <= 0 || c->h <= 0 || c->w <= 0 || c->H <= 0 || c->W <= 0 || c->image_h <= 0 || c->image_w <= 0)
    return fail(AXVS_ERR_ARG, "T=%d, h=%d, w=%d, image %d x %d and H=%d, W=%d must be positive", c->T, c->h, c->w, c->image_h, c->image_w, c->H, c->W);
  if (c->two_stage) {
    if (c->crop_h <= 0 || c->crop_h > c->image_h || c->crop_w <= 0 || c->crop_w > c->image_w)
      return fail(AXVS_ERR_ARG, "crop %d x %d must lie inside the resized image %d x %d", c->crop_h, c->crop_w, c->image_h, c->image_w);
  } else if (c->H > c->image_h || c->W > c->image_w) {
    return fail(AXVS_ERR_ARG, "H=%d, W=%d is a crop of the resized image %d x %d and must lie inside it", c->H, c->W, c->image_h, c->image_w);
  }
  if ((long long)c->T * c->H * c->W >= (1ll << 31)) return fail(AXVS_ERR_ARG, "T*H*W = %lld output pixels must be below 2^31", (long long)c->T * c->H * c->W);
  if (!(c->pixel_confidence_threshold > 0.25 && c->pixel_confidence_threshold < 1.0))
    return fail(AXVS_ERR_ARG, "pixel_confidence_threshold=%g must be in (0.25, 1): at most three slots pass per pixel", c->pixel_confidence_threshold);
  if (c->label_divisor < 0) return fail(AXVS_ERR_ARG, "label_divisor=%d must not be negative", c->label_divisor);
  if (!std::isfinite(c->overlap_threshold) || !std::isfinite(c->class_threshold_thing) || !std::isfinite(c->class_threshold_stuff) ||
      !std::isfinite(c->reorder_class_weight) || !std::isfinite(c->reorder_mask_weight))
    return fail(AXVS_ERR_ARG, "thresholds and reorder weights must be finite");
  return AXVS_OK;
}

struct PanWs {
  unsigned *words, *contested, *area, *n_contested;
  unsigned long long* sums;
  char* zero_from;
  size_t zero_bytes, bytes;
};

PanWs pan_carve(void* ws, const AxvsPanopticCfg* c) {
  const size_t P = (size_t)c->T * c->H * c->W;
  Carver cv(ws);
  PanWs w;
  w.words = cv.take<unsigned>(P);
  w.contested = cv.take<unsigned>(P);
  // the accumulators the pixel pass adds into: one block, zeroed by one memset
  const size_t z0 = cv.off;
  w.sums = cv.take<unsigned long long>(c->N);
  w.area = cv.take<unsigned>(c->N);
  w.n_contested = cv.take<unsigned>(4);
  w.zero_from = ws ? static_cast<char*>(ws) + z0 : nullptr;
  w.zero_bytes = cv.off - z0;
  w.bytes = cv.off;
  return w;
}

PanAxis axis(int in, int out, int ac) {
  // area_pixel_compute_scale<float>: (in - 1) / (out - 1) with align_corners (0 for one output), else in / out
  const float s = ac ? (out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f) : (float)in / (float)out;
  return PanAxis{in, out, s};
}

// upper bound of the low-resolution extent a 16-pixel output span reads along one axis
long long box_extent(const PanAxis& a1, const PanAxis& a2, int two) {
  double span = kPanTile;
  if (two) span = span * a2.in / a2.out + 3.0;
  return (long long)std::ceil(span * a1.in / a1.out) + 3;
}

template <int DT>
int pan_launch_pixel(const void* logits, const PanGeom& g, const PanWs& w, hipStream_t st) {
  const long long est = (long long)g.N * std::min<long long>(box_extent(g.y1, g.y2, g.two), g.h) * std::min<long long>(box_extent(g.x1, g.x2, g.two), g.w);
  const int lds_floats = est * 4 <= kPanMaxLdsBytes ? (int)est : 0;        // 0: every tile reads its taps from global memory
  const long long ntiles = (long long)g.T * ((g.H + kPanTile - 1) / kPanTile) * ((g.W + kPanTile - 1) / kPanTile);
  const int grid = (int)std::min<long long>(ntiles, 1024);
  auto go = [&](auto kernel) -> int {
    if (lds_floats * 4 > 48 * 1024)
      if (int rc = ensure_max_lds(reinterpret_cast<const void*>(kernel))) return rc;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kPanThreads), (size_t)lds_floats * 4, st, logits, g, lds_floats, w.words, w.contested, w.n_contested,
                       w.area, w.sums);
    return AXVS_OK;
  };
  return g.two ? go(panoptic_pixel_kernel<DT, 2>) : go(panoptic_pixel_kernel<DT, 1>);
}

}  // namespace

size_t axvs_video_panoptic_workspace_bytes(const AxvsPanopticCfg* cfg) {
  if (pan_check(cfg)) return 0;
  return pan_carve(nullptr, cfg).bytes;
}

size_t axvs_video_panoptic_table_ints(int N) {
  if (N <= 0 || N > kPanMaxN) {
    fail(AXVS_ERR_ARG, "N=%d mask slots must be in 1..%d", N, kPanMaxN);
    return 0;
  }
  return (size_t)kPanHdr + (size_t)kPanIntArrays * N;
}

int axvs_video_panoptic_fwd(const AxvsPanopticCfg* cfg, const float* mask_cls, const void* mask_pred, int mask_dtype, const int* is_thing,
                            const int* cat_id, int* out_map, int* slot_ints, float* slot_floats, void* workspace, long long workspace_bytes,
                            void* stream) {
  if (int rc = pan_check(cfg)) return rc;
  if (mask_dtype != AXVS_F32 && mask_dtype != AXVS_F16 && mask_dtype != AXVS_BF16)
    return fail(AXVS_ERR_ARG, "mask dtype %d is not AXVS_F16 / AXVS_BF16 / AXVS_F32", mask_dtype);
  if (!mask_cls || !mask_pred || !is_thing || !cat_id || !out_map || !slot_ints || !slot_floats || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  const PanWs w = pan_carve(workspace, cfg);
  if (int rc = check_ws(workspace_bytes, w.bytes)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int ac = cfg->align_corners != 0, two = cfg->two_stage != 0;
  PanGeom g;
  g.N = cfg->N, g.T = cfg->T, g.h = cfg->h, g.w = cfg->w, g.H = cfg->H, g.W = cfg->W, g.two = two, g.ac = ac;
  g.y1 = axis(cfg->h, cfg->image_h, ac), g.x1 = axis(cfg->w, cfg->image_w, ac);
  g.y2 = two ? axis(cfg->crop_h, cfg->H, ac) : PanAxis{1, 1, 0.f};
  g.x2 = two ? axis(cfg->crop_w, cfg->W, ac) : PanAxis{1, 1, 0.f};
  g.thr = (float)cfg->pixel_confidence_threshold;
  if (hipMemsetAsync(w.zero_from, 0, w.zero_bytes, st) != hipSuccess) return fail(AXVS_ERR_LAUNCH, "hipMemsetAsync failed");
  int rc = mask_dtype == AXVS_F32   ? pan_launch_pixel<kPanF32>(mask_pred, g, w, st)
           : mask_dtype == AXVS_F16 ? pan_launch_pixel<kPanF16>(mask_pred, g, w, st)
                                    : pan_launch_pixel<kPanBf16>(mask_pred, g, w, st);
  if (rc) return rc;
  const PanMerge m{cfg->N, cfg->K1, cfg->label_divisor, cfg->class_threshold_thing, cfg->class_threshold_stuff, cfg->overlap_threshold,
                   cfg->reorder_class_weight, cfg->reorder_mask_weight};
  hipLaunchKernelGGL(panoptic_slot_kernel, dim3(1), dim3(kPanSlotThreads), 0, st, mask_cls, is_thing, cat_id, m,
                     (const unsigned*)w.contested, (const unsigned*)w.n_contested, (const unsigned*)w.area, (const unsigned long long*)w.sums, slot_ints,
                     slot_floats);
  const long long P = (long long)cfg->T * cfg->H * cfg->W;
  hipLaunchKernelGGL(panoptic_paint_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, (const unsigned*)w.words, (const int*)slot_ints, cfg->N, P,
                     out_map);
  return last_launch_status();
}
