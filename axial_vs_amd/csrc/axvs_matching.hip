// C-ABI entry points of the matching family (include/axvs.h: axvs_linear_sum_assignment*, axvs_match_embds, axvs_match_clips,
// axvs_video_matcher) and the launch sequences behind them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "axvs_matcher.h"

using namespace axvs;

namespace {

// f(cpl, in_lds) with the assignment kernels' template arguments as constants: cpl() columns per lane for problems of up to `big` rows /
// columns, in_lds() = the cost matrix fits the kernel's dynamic LDS
template <class F>
int by_lsap_form(int big, bool lds, F&& f) {
  auto pick = [&](auto cpl) { return lds ? f(cpl, std::true_type{}) : f(cpl, std::false_type{}); };
  if (big <= 64) return pick(std::integral_constant<int, 1>{});
  if (big <= 128) return pick(std::integral_constant<int, 2>{});
  if (big <= 256) return pick(std::integral_constant<int, 4>{});
  return pick(std::integral_constant<int, 8>{});
}

}  // namespace

// ---- clip-to-clip query alignment ----
static int launch_lsap(const float* cost, long long* col4row, int batch, int n, hipStream_t st, int chain = 1) {
  const size_t bytes = (size_t)n * n * sizeof(float);
  const bool lds = bytes <= 128 * 1024;
  if (int rc = by_lsap_form(n, lds, [&](auto cpl, auto in_lds) {
        if (in_lds())
          if (int rc = ensure_max_lds(reinterpret_cast<const void*>(&lsap_kernel<cpl(), in_lds()>))) return rc;
        hipLaunchKernelGGL((lsap_kernel<cpl(), in_lds()>), dim3(batch), dim3(64), in_lds() ? bytes : 0, st, cost, col4row, n, chain);
        return (int)AXVS_OK;
      }))
    return rc;
  return last_launch_status();
}

int axvs_linear_sum_assignment(const float* cost, long long* col4row, int batch, int n, void* stream) {
  if (!cost || !col4row) return fail(AXVS_ERR_ARG, "null pointer");
  if (batch <= 0 || n <= 0 || n > kLsapMax) return fail(AXVS_ERR_ARG, "n=%d must be in 1..%d", n, kLsapMax);
  return launch_lsap(cost, col4row, batch, n, static_cast<hipStream_t>(stream));
}

static int cost_tile_lds(int C) {     // two 16-row panels of C + 1 floats
  const size_t bytes = (size_t)2 * 16 * (C + 1) * sizeof(float);
  if (bytes > 160 * 1024) return fail(AXVS_ERR_ARG, "embedding width C=%d too large for the cost kernel's LDS panels", C);
  return bytes > 64 * 1024 ? ensure_max_lds(reinterpret_cast<const void*>(&cost_tile_kernel)) : AXVS_OK;
}

size_t axvs_match_embds_workspace_bytes(int Q, int C) { return ((size_t)Q * Q + 2 * (size_t)Q * C) * sizeof(float); }

int axvs_match_embds(const float* tgt_embds, const float* cur_embds, long long* indices, int Q, int C, void* workspace,
                     size_t workspace_bytes, void* stream) {
  if (!tgt_embds || !cur_embds || !indices || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (Q <= 0 || Q > kLsapMax || C <= 0) return fail(AXVS_ERR_ARG, "Q=%d must be in 1..%d", Q, kLsapMax);
  if (int rc = check_ws(workspace_bytes, axvs_match_embds_workspace_bytes(Q, C))) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* cost = static_cast<float*>(workspace);
  float* nrm = cost + (size_t)Q * Q;
  if (int rc = cost_tile_lds(C)) return rc;
  hipLaunchKernelGGL(normalize_rows_kernel, dim3((unsigned)((2 * Q + 3) / 4)), dim3(256), 0, st, tgt_embds, cur_embds, nrm, Q, C);
  hipLaunchKernelGGL(cost_tile_kernel, dim3((Q + 15) / 16, (Q + 15) / 16, 1), dim3(256), (size_t)2 * 16 * (C + 1) * sizeof(float), st, (const float*)nrm,
                     cost, 0, Q, C);
  return launch_lsap(cost, indices, 1, Q, st);
}

// the whole clip-alignment loop of a batch of videos (maxtron_cc_model.py:280-301) in three launches
size_t axvs_match_clips_workspace_bytes(int V, int Tc, int Q, int C) {
  return ((size_t)V * Tc * Q * C + (size_t)V * (Tc > 1 ? Tc - 1 : 1) * Q * Q) * sizeof(float);
}

int axvs_match_clips(const float* mask_embeddings, long long* indices, int V, int Tc, int Q, int C, void* workspace,
                     size_t workspace_bytes, void* stream) {
  if (!mask_embeddings || !indices || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (V <= 0 || Tc <= 1 || C <= 0 || Q <= 0 || Q > kLsapMax) return fail(AXVS_ERR_ARG, "need V >= 1, Tc >= 2, Q in 1..%d", kLsapMax);
  if (int rc = check_ws(workspace_bytes, axvs_match_clips_workspace_bytes(V, Tc, Q, C))) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* nrm = static_cast<float*>(workspace);
  float* cost = nrm + (size_t)V * Tc * Q * C;
  const long long R = (long long)V * Tc * Q;
  if (int rc = cost_tile_lds(C)) return rc;
  hipLaunchKernelGGL(normalize_rows1_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, mask_embeddings, nrm, R, C);
  hipLaunchKernelGGL(cost_tile_kernel, dim3((Q + 15) / 16, (Q + 15) / 16, (unsigned)(V * (Tc - 1))), dim3(256), (size_t)2 * 16 * (C + 1) * sizeof(float), st,
                     (const float*)nrm, cost, Tc, Q, C);
  return launch_lsap(cost, indices, V, Q, st, Tc - 1);
}

// ---- prediction-to-ground-truth matching: rectangular assignment + the fused similarity / cost kernels (axvs_matcher.h) ----
static int launch_lsap_rect(const float* cost, long long ld, int nr, int nc_max, const int* nc_per_problem, long long* rows, long long* cols,
                            int batch, hipStream_t st) {
  const int kmax = nr < nc_max ? nr : nc_max, big = nr > nc_max ? nr : nc_max;
  const size_t bytes = (size_t)nr * nc_max * sizeof(float);
  const bool lds = bytes <= 128 * 1024;
  for (int z0 = 0; z0 < batch; z0 += kLsapCountsPerLaunch) {
    const int nb = batch - z0 < kLsapCountsPerLaunch ? batch - z0 : kLsapCountsPerLaunch;
    LsapCounts cnt;
    if (nc_per_problem)
      for (int i = 0; i < nb; ++i) cnt.nc[i] = (unsigned short)nc_per_problem[z0 + i];
    const float* c = cost + (long long)z0 * nr * ld;
    long long* ro = rows + (long long)z0 * kmax;
    long long* co = cols + (long long)z0 * kmax;
    if (int rc = by_lsap_form(big, lds, [&](auto cpl, auto in_lds) {
          if (in_lds())
            if (int rc = ensure_max_lds(reinterpret_cast<const void*>(&lsap_rect_kernel<cpl(), in_lds()>))) return rc;
          hipLaunchKernelGGL((lsap_rect_kernel<cpl(), in_lds()>), dim3(nb), dim3(64), in_lds() ? bytes : 0, st, c, ld, nr, nc_max, cnt, nc_per_problem != nullptr, ro,
                             co, kmax);
          return (int)AXVS_OK;
        }))
      return rc;
  }
  return last_launch_status();
}

int axvs_linear_sum_assignment_rect(const float* cost, long long ld, int nr, int nc_max, const int* nc_per_problem, long long* rows_out,
                                    long long* cols_out, int batch, void* stream) {
  if (batch <= 0 || nr <= 0 || nr > kLsapMax || nc_max < 0 || nc_max > kLsapMax)
    return fail(AXVS_ERR_ARG, "nr=%d must be in 1..%d and nc_max=%d in 0..%d (batch=%d >= 1)", nr, kLsapMax, nc_max, kLsapMax, batch);
  if (ld < nc_max) return fail(AXVS_ERR_ARG, "ld=%lld is smaller than nc_max=%d", ld, nc_max);
  if (nc_per_problem)
    for (int i = 0; i < batch; ++i)
      if (nc_per_problem[i] < 0 || nc_per_problem[i] > nc_max) return fail(AXVS_ERR_ARG, "nc_per_problem[%d]=%d is outside 0..nc_max=%d", i, nc_per_problem[i], nc_max);
  if (nc_max == 0) return AXVS_OK;          // min(nr, 0) pairs per problem: nothing to write
  if (!cost || !rows_out || !cols_out) return fail(AXVS_ERR_ARG, "null pointer");
  return launch_lsap_rect(cost, ld, nr, nc_max, nc_per_problem, rows_out, cols_out, batch, static_cast<hipStream_t>(stream));
}

namespace {
// workgroups per problem of the similarity kernel: enough to fill the device over all problems, at least 4 pixel tiles each (the
// partial sums a workgroup writes are Q * M floats: fewer tiles per workgroup would make them a visible share of the traffic)
TileSplit matcher_plan(int nprob, long long P) { return split_tiles((P + kMatcherTP - 1) / kMatcherTP, nprob, 512); }
int matcher_check_shape(int L, int B, int Q, int K1, long long P, int M_max) {
  if (int rc = check_shape("L", L, B, "Q", Q, K1, P)) return rc;
  if (M_max < 0 || M_max > kMaxObjects) return fail(AXVS_ERR_ARG, "M_max=%d must be in 0..%d", M_max, kMaxObjects);
  if (((Q + 31) / 32 + (M_max + 31) / 32) * 32 > kMatcherMaxRows)
    return fail(AXVS_ERR_ARG, "Q=%d and M_max=%d, each rounded up to 32, must add up to at most 576 (the similarity kernel's LDS tiles)", Q, M_max);
  return AXVS_OK;
}
template <int DT, int TDT>
int launch_matcher_sim(const MatcherArgs& a, const void* targets, int nprob, int B, int Q, long long P, int M_max, int masking, float* part,
                       TileSplit pl, hipStream_t st) {
  const size_t lds = (size_t)(((Q + 31) / 32 + (M_max + 31) / 32) * 32) * kMatcherLDP * sizeof(float);
  if (lds > 48 * 1024)
    if (int rc = ensure_max_lds(reinterpret_cast<const void*>(&matcher_sim_kernel<DT, TDT>))) return rc;
  // more than 16 output blocks: block chunks over grid.y, each of which reads the logits and redoes the softmax (include/axvs.h)
  const int nblk = ((Q + 31) / 32) * ((M_max + 31) / 32), chunks = (nblk + kMatcherBlocksPerChunk - 1) / kMatcherBlocksPerChunk;
  hipLaunchKernelGGL((matcher_sim_kernel<DT, TDT>), dim3(pl.npb, chunks, nprob), dim3(256), lds, st, a, targets, B, Q, P, M_max, pl.tiles_per_wg, masking, part);
  return AXVS_OK;
}
}  // namespace

size_t axvs_video_matcher_workspace_bytes(int L, int B, int Q, int M_max, long long P) {
  if (L <= 0 || B <= 0 || Q <= 0 || M_max <= 0 || P <= 0) return 0;
  const int nprob = L * B;
  const TileSplit pl = matcher_plan(nprob, P);
  return align_up((size_t)nprob * pl.npb * matcher_part_stride(Q, M_max) * sizeof(float)) + align_up((size_t)2 * nprob * Q * sizeof(float));
}

int axvs_video_matcher(const void* const* pred_masks, int mask_dtype, const float* const* pred_logits, const void* targets, int target_dtype,
                       const long long* labels, const int* m_per_video, int L, int B, int Q, int K1, long long P, int M_max, int masking_void_pixel,
                       float* sims, long long* rows_out, long long* cols_out, float* matched_dice, float* matched_cls, void* workspace,
                       size_t workspace_bytes, void* stream) {
  if (int rc = matcher_check_shape(L, B, Q, K1, P, M_max)) return rc;
  if (!pred_masks || !pred_logits) return fail(AXVS_ERR_ARG, "null pointer");
  if (mask_dtype != AXVS_F16 && mask_dtype != AXVS_BF16 && mask_dtype != AXVS_F32) return fail(AXVS_ERR_ARG, "pred_masks dtype %d is not AXVS_F16 / AXVS_BF16 / AXVS_F32", mask_dtype);
  if (int rc = check_target_dtype(target_dtype)) return rc;
  MatcherArgs a;
  memset(&a, 0, sizeof(a));
  VideoFill v;
  if (int rc = fill_videos(m_per_video, B, M_max, "M_max=", a.m, a.off, &v)) return rc;
  if (v.max != M_max) return fail(AXVS_ERR_ARG, "M_max=%d is not the largest entry of m_per_video (%d)", M_max, v.max);
  if (M_max == 0) return AXVS_OK;           // no ground-truth object in any video: every result is empty
  if (int rc = fill_layers(pred_masks, L, a.masks)) return rc;
  if (int rc = fill_layers(pred_logits, L, a.logits)) return rc;
  if (!targets || !labels || !sims || !rows_out || !cols_out || !matched_dice || !matched_cls || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (int rc = check_ws(workspace_bytes, axvs_video_matcher_workspace_bytes(L, B, Q, M_max, P))) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nprob = L * B, kmax = std::min(Q, M_max);
  const TileSplit pl = matcher_plan(nprob, P);
  Carver cw(workspace);
  float* part = cw.take<float>((size_t)nprob * pl.npb * matcher_part_stride(Q, M_max));
  float* stats = cw.take<float>((size_t)2 * nprob * Q);
  const size_t plane = (size_t)nprob * Q * M_max;
  float *mask_sim = sims, *class_sim = sims + plane, *cost = sims + 2 * plane;
  const int masking = masking_void_pixel != 0;
  g_prof_next = 0;
  mark(st, "begin");
  const int rc = by_mask_dtype(mask_dtype, [&](auto md) {
    return by_target_dtype(target_dtype, [&](auto td) { return launch_matcher_sim<md(), td()>(a, targets, nprob, B, Q, P, M_max, masking, part, pl, st); });
  });
  if (rc) return rc;
  mark(st, "matcher.similarity");
  const int nrows = nprob * Q;
  hipLaunchKernelGGL(matcher_class_stats_kernel, dim3((nrows + 3) / 4), dim3(256), 0, st, a, B, Q, K1, stats, nrows);
  hipLaunchKernelGGL(matcher_finish_kernel, dim3((Q * M_max + 255) / 256, nprob), dim3(256), 0, st, a, (const float*)part, pl.npb, (const float*)stats, labels,
                     B, Q, K1, M_max, mask_sim, class_sim, cost);
  mark(st, "matcher.cost");
  int nc[kMaxLayers * kMaxVideos];
  for (int z = 0; z < nprob; ++z) nc[z] = m_per_video[z % B];
  if (int rc2 = launch_lsap_rect(cost, M_max, Q, M_max, nc, rows_out, cols_out, nprob, st)) return rc2;
  mark(st, "matcher.assignment");
  const long long total = (long long)nprob * kmax;
  hipLaunchKernelGGL(matcher_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const long long*)rows_out, (const long long*)cols_out,
                     (const float*)mask_sim, (const float*)class_sim, Q, M_max, kmax, total, matched_dice, matched_cls);
  mark(st, "matcher.gather");
  return last_launch_status();
}

