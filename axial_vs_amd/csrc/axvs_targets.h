// Scaffold shared by the training-target units (axvs_matching.hip, axvs_criterion.hip, axvs_pixel_loss.hip, axvs_tl_loss.hip).  Each of them
// takes L layers x B videos, per-layer prediction pointers, the videos' ground-truth masks concatenated along the objects with
// m_per_video, and u8 or fp32 targets: the limits, the typed element loader of their kernels, the host-side checks and fills, the split of
// a problem's tiles over workgroups and the dispatch on the target type are stated here once.
#pragma once
#include <algorithm>
#include <type_traits>

#include "axvs_host.h"

namespace axvs {

constexpr int kMaxLayers = 16, kMaxVideos = 64;
constexpr int kMaxQueries = kLsapMax, kMaxObjects = kLsapMax;      // every (layer, video) problem goes through the assignment kernel

// element i of a tensor of dtype DT (AXVS_F16 / AXVS_BF16 / AXVS_F32 / AXVS_U8) as a float
template <int DT>
__device__ __forceinline__ float load_f32(const void* p, long long i) {
  if constexpr (DT == AXVS_F32) return static_cast<const float*>(p)[i];
  else if constexpr (DT == AXVS_U8) return (float)static_cast<const unsigned char*>(p)[i];
  else return H16<DT == AXVS_BF16>::to_f32(static_cast<const u16*>(p)[i]);
}

// lname = L layers in 1..kMaxLayers, B videos in 1..kMaxVideos, qname = `queries` in 1..kMaxQueries, K1 = K + 1 >= 2 logits, 1 <= P <= 2^40
// pixels (a unit without logits or with pixel extents of its own leaves the defaults)
inline int check_shape(const char* lname, int L, int B, const char* qname, int queries, int K1 = 2, long long P = 1) {
  if (L <= 0 || L > kMaxLayers || B <= 0 || B > kMaxVideos)
    return fail(AXVS_ERR_ARG, "%s=%d must be in 1..%d and B=%d in 1..%d", lname, L, kMaxLayers, B, kMaxVideos);
  if (queries <= 0 || queries > kMaxQueries)
    return fail(AXVS_ERR_ARG, "%s=%d queries must be in 1..%d (the assignment kernel's bound)", qname, queries, kMaxQueries);
  if (K1 < 2 || P <= 0 || P > (1ll << 40)) return fail(AXVS_ERR_ARG, "need K + 1 = %d >= 2 logits and P = %lld >= 1 pixels", K1, P);
  return AXVS_OK;
}

// m[b] = m_per_video[b] in 0..bound (`bound_name`: what the refusal calls the bound), off[b] = first row of video b in the concatenated
// targets.  The caller has zeroed the struct m and off belong to.
struct VideoFill { int total, max; };
inline int fill_videos(const int* m_per_video, int B, int bound, const char* bound_name, int (&m)[kMaxVideos], int (&off)[kMaxVideos], VideoFill* out) {
  if (!m_per_video) return fail(AXVS_ERR_ARG, "null pointer");
  *out = VideoFill{0, 0};
  for (int b = 0; b < B; ++b) {
    if (m_per_video[b] < 0 || m_per_video[b] > bound) return fail(AXVS_ERR_ARG, "m_per_video[%d]=%d is outside 0..%s%d", b, m_per_video[b], bound_name, bound);
    m[b] = m_per_video[b];
    off[b] = out->total;
    out->total += m_per_video[b];
    out->max = std::max(out->max, m_per_video[b]);
  }
  return AXVS_OK;
}

// a host array of L device pointers -> the kernel-argument table
template <class T>
inline int fill_layers(const T* const* src, int L, const T* (&dst)[kMaxLayers]) {
  if (!src) return fail(AXVS_ERR_ARG, "null pointer");
  for (int l = 0; l < L; ++l) {
    if (!src[l]) return fail(AXVS_ERR_ARG, "null pointer (layer %d)", l);
    dst[l] = src[l];
  }
  return AXVS_OK;
}

// `ntiles` tiles of a problem over npb workgroups of tiles_per_wg tiles each: about `target_workgroups` over all `problems`, at least 4
// tiles per workgroup (a workgroup ends with a reduction or a set of partial sums worth about a tile), at most max_tiles_per_wg (0: no cap)
struct TileSplit { int npb, tiles_per_wg; };
inline TileSplit split_tiles(long long ntiles, long long problems, int target_workgroups, long long max_tiles_per_wg = 0) {
  long long npb = std::min((target_workgroups + problems - 1) / problems, (ntiles + 3) / 4);
  if (max_tiles_per_wg) npb = std::max(npb, (ntiles + max_tiles_per_wg - 1) / max_tiles_per_wg);
  npb = std::max<long long>(npb, 1);
  const long long per = (ntiles + npb - 1) / npb;
  return {(int)((ntiles + per - 1) / per), (int)per};
}

inline int check_target_dtype(int dtype) {
  if (dtype != AXVS_F32 && dtype != AXVS_U8) return fail(AXVS_ERR_ARG, "target dtype %d is not AXVS_F32 / AXVS_U8", dtype);
  return AXVS_OK;
}
// f(td), td() = AXVS_U8 or AXVS_F32 as a constant: the target type of a kernel template (check_target_dtype first)
template <class F>
auto by_target_dtype(int dtype, F&& f) {
  if (dtype == AXVS_U8) return f(std::integral_constant<int, AXVS_U8>{});
  return f(std::integral_constant<int, AXVS_F32>{});
}
// the same over the matcher's prediction masks: AXVS_F16, AXVS_BF16 or AXVS_F32
template <class F>
auto by_mask_dtype(int dtype, F&& f) {
  if (dtype == AXVS_F32) return f(std::integral_constant<int, AXVS_F32>{});
  if (dtype == AXVS_BF16) return f(std::integral_constant<int, AXVS_BF16>{});
  return f(std::integral_constant<int, AXVS_F16>{});
}

}  // namespace axvs
