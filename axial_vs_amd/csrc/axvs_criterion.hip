// C-ABI entry points of the set criterion (include/axvs.h: axvs_set_criterion_*) and the launch sequences behind them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "axvs_criterion.h"

using namespace axvs;

namespace {

// workgroups per problem of the pixel kernels: two per CU over all problems, at least 4 pixel tiles each (a workgroup ends with one
// cross-lane reduction per query, about a tile's worth of work), and at most 2^22 pixels each (the nonzero count of a workgroup is
// kept in fp32)
TileSplit crit_plan(int nprob, long long P) { return split_tiles((P + kCritTP - 1) / kCritTP, nprob, 512, 65536); }

int fill_args(CritArgs& a, const float* const* pred_masks, const float* const* pred_logits, const int* m_per_video, int L, int B, int* total) {
  memset(&a, 0, sizeof(a));
  if (!pred_masks || !pred_logits || !m_per_video) return fail(AXVS_ERR_ARG, "null pointer");
  VideoFill v;
  if (int rc = fill_videos(m_per_video, B, kMaxObjects, "", a.m, a.off, &v)) return rc;
  if (int rc = fill_layers(pred_masks, L, a.masks)) return rc;
  *total = v.total;
  return fill_layers(pred_logits, L, a.logits);
}

}  // namespace

size_t axvs_set_criterion_saved_bytes(int L, int B, int N) {
  if (check_shape("L", L, B, "N", N)) return 0;
  return align_up((size_t)crit_saved_words(L, B, N) * 4);
}

size_t axvs_set_criterion_workspace_bytes(int L, int B, int N, int K1, long long P) {
  if (check_shape("L", L, B, "N", N, K1, P)) return 0;
  const TileSplit pl = crit_plan(L * B, P);
  return align_up((size_t)L * B * pl.npb * crit_part_stride(N) * sizeof(float));
}

int axvs_set_criterion_fwd(const float* const* pred_masks, const float* const* pred_logits, const void* targets, int target_dtype,
                           const long long* labels, const int* m_per_video, const long long* rows, const long long* cols,
                           const float* matched_dice, const float* matched_cls, int kmax, int L, int B, int N, int K1, long long P,
                           int masking_void_pixel, int share_final_matching, float* losses, void* saved, void* workspace,
                           long long workspace_bytes, void* stream) {
  if (int rc = check_shape("L", L, B, "N", N, K1, P)) return rc;
  if (int rc = check_target_dtype(target_dtype)) return rc;
  CritArgs a;
  int total = 0;
  if (int rc = fill_args(a, pred_masks, pred_logits, m_per_video, L, B, &total)) return rc;
  if (kmax < 0 || kmax > N) return fail(AXVS_ERR_ARG, "kmax=%d pairs per problem must be in 0..N=%d", kmax, N);
  if (!losses || !saved || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (kmax > 0 && (!targets || !labels || !rows || !cols || !matched_dice || !matched_cls)) return fail(AXVS_ERR_ARG, "null pointer");
  const size_t need = axvs_set_criterion_workspace_bytes(L, B, N, K1, P);
  if (int rc = check_ws(workspace_bytes, need)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nprob = L * B, share = share_final_matching != 0, masking = masking_void_pixel != 0;
  const TileSplit pl = crit_plan(nprob, P);
  const CritSaved s = crit_saved_views(saved, L, B, N);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(criterion_index_kernel, dim3((share ? 1 : L) * B), dim3(256), 0, st, a, rows, cols, matched_dice, matched_cls, labels, B, N, K1, kmax, s);
  const dim3 grid(pl.npb, nprob);
  by_target_dtype(target_dtype, [&](auto td) {
    hipLaunchKernelGGL(N <= 4 * kCritNPW ? criterion_fwd_kernel<td()> : criterion_fwd_any_kernel<td()>, grid, dim3(256), 0, st, a, targets, (const int*)s.inv,
                       B, N, P, pl.tiles_per_wg, masking, share, part);
  });
  hipLaunchKernelGGL(criterion_finish_kernel, dim3(L), dim3(256), 0, st, a, (const float*)part, pl.npb, B, N, K1, masking, share, s, losses);
  return last_launch_status();
}

int axvs_set_criterion_bwd(const float* grad_losses, const float* const* pred_masks, const float* const* pred_logits, const void* targets,
                           int target_dtype, const int* m_per_video, int L, int B, int N, int K1, long long P, int masking_void_pixel,
                           int share_final_matching, const void* saved, float* const* d_pred_masks, float* const* d_pred_logits, void* stream) {
  if (int rc = check_shape("L", L, B, "N", N, K1, P)) return rc;
  if (int rc = check_target_dtype(target_dtype)) return rc;
  CritArgs a;
  int total = 0;
  if (int rc = fill_args(a, pred_masks, pred_logits, m_per_video, L, B, &total)) return rc;
  if (!grad_losses || !saved || !d_pred_masks || !d_pred_logits) return fail(AXVS_ERR_ARG, "null pointer");
  if (total > 0 && !targets) return fail(AXVS_ERR_ARG, "null pointer");
  bool any_masks = false, any_logits = false;
  for (int l = 0; l < L; ++l) {
    a.dmasks[l] = d_pred_masks[l];
    a.dlogits[l] = d_pred_logits[l];
    any_masks |= d_pred_masks[l] != nullptr;
    any_logits |= d_pred_logits[l] != nullptr;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nprob = L * B, share = share_final_matching != 0, masking = masking_void_pixel != 0;
  const TileSplit pl = crit_plan(nprob, P);
  const CritSaved s = crit_saved_views(const_cast<void*>(saved), L, B, N);
  const dim3 grid(pl.npb, nprob);
  if (any_masks)
    by_target_dtype(target_dtype, [&](auto td) {
      hipLaunchKernelGGL(N <= 4 * kCritNPW ? criterion_bwd_kernel<td()> : criterion_bwd_any_kernel<td()>, grid, dim3(256), 0, st, a, targets, grad_losses, B,
                         N, P, pl.tiles_per_wg, masking, share, s);
    });
  const int nrows = nprob * N;
  if (any_logits) hipLaunchKernelGGL(criterion_logits_bwd_kernel, dim3((nrows + 3) / 4), dim3(256), 0, st, a, grad_losses, B, N, K1, s, nrows);
  return last_launch_status();
}
