// C-ABI entry points of Tube-Link's point-sampled training loss (include/axvs.h: axvs_tl_loss_*) and the launch sequences behind them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "axvs_tl_loss.h"

using namespace axvs;

namespace {

// workgroups per (problem, query block) of the cost kernel: about four per CU over everything, at least 4 point tiles each
TileSplit tl_plan(int nprob, int nqb, int P) { return split_tiles((P + kTLTP - 1) / kTLTP, nprob * nqb, 1024); }

struct TLHost {
  TLArgs a;
  TLShape s;
  int total;      // rows of the concatenated targets
};

int tl_setup(TLHost& h, const AxvsTLLossCfg* c, const int* m_per_video) {
  memset(&h, 0, sizeof(h));
  if (!c || !m_per_video) return fail(AXVS_ERR_ARG, "null pointer");
  if (int rc = check_shape("L", c->L, c->B, "Q", c->Q, c->K1)) return rc;
  if (c->T <= 0 || c->h <= 0 || c->w <= 0 || c->Hg <= 0 || c->Wg <= 0) return fail(AXVS_ERR_ARG, "T, h, w, Hg, Wg must be positive");
  if ((long long)c->T * c->h > kTLMaxRows || (long long)c->T * c->Hg > (1 << 24) || c->w > (1 << 20) || c->Wg > (1 << 20))
    return fail(AXVS_ERR_ARG, "T*h=%lld rows of the long image must be at most %d (T*Hg at most 2^24, w and Wg at most 2^20)", (long long)c->T * c->h, kTLMaxRows);
  if ((long long)c->B * c->T * c->Q * c->h * c->w >= (1ll << 40)) return fail(AXVS_ERR_ARG, "B*T*Q*h*w must be below 2^40");
  if (c->num_points <= 0 || c->num_points > kTLMaxPoints) return fail(AXVS_ERR_ARG, "num_points=%d must be in 1..%d", c->num_points, kTLMaxPoints);
  if (c->num_cand < 0 || c->num_cand > kTLMaxCand) return fail(AXVS_ERR_ARG, "S=%d candidate points must be in 0..%d", c->num_cand, kTLMaxCand);
  if (c->num_kept < 0 || c->num_kept > c->num_points || c->num_kept > c->num_cand)
    return fail(AXVS_ERR_ARG, "k=%d kept points must be in 0..min(num_points=%d, S=%d)", c->num_kept, c->num_points, c->num_cand);
  if (int rc = check_target_dtype(c->target_dtype)) return rc;
  TLShape& s = h.s;
  s.L = c->L; s.B = c->B; s.Q = c->Q; s.K1 = c->K1; s.T = c->T; s.h = c->h; s.w = c->w; s.Hg = c->Hg; s.Wg = c->Wg;
  s.P = c->num_points; s.S = c->num_cand; s.k = c->num_kept;
  s.cost_cls = c->cost_cls; s.cost_mask = c->cost_mask; s.cost_dice = c->cost_dice;
  s.loss_cls = c->loss_cls; s.loss_mask = c->loss_mask; s.loss_dice = c->loss_dice; s.eps = c->dice_eps;
  VideoFill v;
  if (int rc = fill_videos(m_per_video, c->B, kMaxObjects, "", h.a.m, h.a.off, &v)) return rc;
  for (int b = 0; b < c->B; ++b) h.a.goff[b + 1] = h.a.goff[b] + std::min(c->Q, h.a.m[b]);
  s.G = h.a.goff[c->B];
  s.Mmax = v.max;
  s.kmax = std::min(c->Q, v.max);
  h.total = v.total;
  return AXVS_OK;
}

TLSaved tl_saved_views(void* saved, const TLShape& s, size_t* bytes) {
  Carver cv(saved);
  TLSaved v;
  v.pairs = cv.take<int>((size_t)s.L * s.G * 2);
  v.pairsum = cv.f((size_t)s.L * s.G * 4);
  v.chosen = cv.f((size_t)s.L * s.G * s.P * 2);
  v.labels = cv.take<int>((size_t)s.L * s.B * s.Q);
  v.avg = cv.f(s.L);
  if (bytes) *bytes = cv.off;
  return v;
}

struct TLWork { float* part; float* cost; };
TLWork tl_work_views(void* ws, const TLShape& s, size_t* bytes) {
  Carver cv(ws);
  TLWork v{nullptr, nullptr};
  if (s.G > 0) {
    const int Qp = (s.Q + 31) & ~31, Mpm = (s.Mmax + 31) & ~31, nprob = s.L * s.B;
    const TileSplit pl = tl_plan(nprob, Qp >> 5, s.P);
    v.part = cv.f((size_t)nprob * pl.npb * tl_part_stride(Qp, Mpm));
    v.cost = cv.f((size_t)nprob * s.Q * s.Mmax);
  }
  if (bytes) *bytes = std::max<size_t>(cv.off, 256);
  return v;
}

}  // namespace

size_t axvs_tl_loss_saved_bytes(const AxvsTLLossCfg* cfg, const int* m_per_video) {
  TLHost h;
  if (tl_setup(h, cfg, m_per_video)) return 0;
  size_t n = 0;
  tl_saved_views(nullptr, h.s, &n);
  return n;
}

size_t axvs_tl_loss_workspace_bytes(const AxvsTLLossCfg* cfg, const int* m_per_video) {
  TLHost h;
  if (tl_setup(h, cfg, m_per_video)) return 0;
  size_t n = 0;
  tl_work_views(nullptr, h.s, &n);
  return n;
}

int axvs_tl_loss_fwd(const AxvsTLLossCfg* cfg, const float* const* cls_scores, const float* const* mask_preds, const void* targets,
                     const long long* labels, const int* m_per_video, const float* class_weight, const float* match_coords,
                     const float* cand_coords, const float* rand_coords, const float* num_total_masks, float* losses, long long* rows,
                     long long* cols, float* cost, int* sel_idx, void* saved, void* workspace, long long workspace_bytes, void* stream) {
  TLHost h;
  if (int rc = tl_setup(h, cfg, m_per_video)) return rc;
  const TLShape& s = h.s;
  if (!cls_scores || !mask_preds || !class_weight || !num_total_masks || !losses || !saved || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (int rc = fill_layers(cls_scores, s.L, h.a.cls)) return rc;
  if (int rc = fill_layers(mask_preds, s.L, h.a.masks)) return rc;
  if (s.G > 0 && (!targets || !labels || !match_coords || !rows || !cols)) return fail(AXVS_ERR_ARG, "null pointer");
  if (s.G > 0 && s.k > 0 && !cand_coords) return fail(AXVS_ERR_ARG, "null pointer (cand_coords)");
  if (s.G > 0 && s.P - s.k > 0 && !rand_coords) return fail(AXVS_ERR_ARG, "null pointer (rand_coords)");
  size_t need = 0;
  const TLWork wk = tl_work_views(workspace, s, &need);
  if (int rc = check_ws(workspace_bytes, need)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const TLSaved sv = tl_saved_views(saved, s, nullptr);
  const int nprob = s.L * s.B;
  if (s.G > 0) {
    const int Qp = (s.Q + 31) & ~31, Mpm = (s.Mmax + 31) & ~31;
    const TileSplit pl = tl_plan(nprob, Qp >> 5, s.P);
    const size_t lds = (size_t)(96 + Mpm) * kTLLDP * sizeof(float);
    float* cst = cost ? cost : wk.cost;
    const dim3 grid(pl.npb, Qp >> 5, nprob);
    const int rc = by_target_dtype(cfg->target_dtype, [&](auto td) {
      if (int rc = ensure_max_lds(reinterpret_cast<const void*>(&tl_cost_kernel<td()>))) return rc;
      hipLaunchKernelGGL(tl_cost_kernel<td()>, grid, dim3(256), lds, st, h.a, targets, match_coords, s, pl.tiles_per_wg, wk.part);
      return (int)AXVS_OK;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(tl_cost_finish_kernel, dim3((s.Q * s.Mmax + 255) / 256, nprob), dim3(256), 0, st, h.a, (const float*)wk.part, pl.npb, labels, s, cst);
    if (int rc = last_launch_status()) return rc;
    int nc[kMaxLayers * kMaxVideos];
    for (int z = 0; z < nprob; ++z) nc[z] = h.a.m[z % s.B];
    if (int rc = axvs_linear_sum_assignment_rect(cst, s.Mmax, s.Q, s.Mmax, nc, rows, cols, nprob, stream)) return rc;
    const dim3 pgrid(s.G, s.L);
    by_target_dtype(cfg->target_dtype, [&](auto td) {
      hipLaunchKernelGGL(tl_select_loss_kernel<td()>, pgrid, dim3(kTLThreads), 0, st, h.a, targets, (const long long*)rows, (const long long*)cols, cand_coords,
                         rand_coords, s, sv, sel_idx);
    });
  }
  hipLaunchKernelGGL(tl_finish_kernel, dim3(s.L), dim3(256), 0, st, h.a, labels, class_weight, num_total_masks, s, sv, losses);
  return last_launch_status();
}

int axvs_tl_loss_bwd(const AxvsTLLossCfg* cfg, const float* grad_losses, const float* const* cls_scores, const float* const* mask_preds,
                     const void* targets, const int* m_per_video, const float* class_weight, const float* num_total_masks, const void* saved,
                     float* const* d_cls_scores, float* const* d_mask_preds, void* stream) {
  TLHost h;
  if (int rc = tl_setup(h, cfg, m_per_video)) return rc;
  const TLShape& s = h.s;
  if (!grad_losses || !cls_scores || !mask_preds || !class_weight || !num_total_masks || !saved || !d_cls_scores || !d_mask_preds)
    return fail(AXVS_ERR_ARG, "null pointer");
  if (s.G > 0 && !targets) return fail(AXVS_ERR_ARG, "null pointer");
  if (int rc = fill_layers(cls_scores, s.L, h.a.cls)) return rc;
  if (int rc = fill_layers(mask_preds, s.L, h.a.masks)) return rc;
  bool any_masks = false, any_cls = false;
  for (int l = 0; l < s.L; ++l) {
    h.a.dcls[l] = d_cls_scores[l];
    h.a.dmasks[l] = d_mask_preds[l];
    any_masks |= d_mask_preds[l] != nullptr;
    any_cls |= d_cls_scores[l] != nullptr;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const TLSaved sv = tl_saved_views(const_cast<void*>(saved), s, nullptr);
  if (any_masks) {
    const long long n = (long long)s.B * s.T * s.Q * s.h * s.w;
    const int chunks = (int)std::min<long long>((n / 4 + 255) / 256 + 1, 2048);
    hipLaunchKernelGGL(tl_fill_zero_kernel, dim3(chunks, s.L), dim3(256), 0, st, h.a, n);
    if (s.G > 0) {
      const size_t lds = (size_t)(2 * (s.T * s.h + 1) + 1) * sizeof(int) + (size_t)2 * s.P * sizeof(unsigned short);
      const dim3 pgrid(s.G, s.L);
      const int rc = by_target_dtype(cfg->target_dtype, [&](auto td) {
        if (int rc = ensure_max_lds(reinterpret_cast<const void*>(&tl_scatter_kernel<td()>))) return rc;
        hipLaunchKernelGGL(tl_scatter_kernel<td()>, pgrid, dim3(kTLThreads), lds, st, h.a, targets, grad_losses, num_total_masks, s, sv);
        return (int)AXVS_OK;
      });
      if (rc) return rc;
    }
  }
  const long long nrows = (long long)s.L * s.B * s.Q;
  if (any_cls) hipLaunchKernelGGL(tl_cls_bwd_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, st, h.a, grad_losses, class_weight, s, sv, nrows);
  return last_launch_status();
}
