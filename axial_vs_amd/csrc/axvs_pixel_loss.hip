// C-ABI entry points of the sampled pixel losses (include/axvs.h: axvs_pixel_*) and the launch sequences behind them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "axvs_pixel_loss.h"

using namespace axvs;

namespace {

int ceil16(int x) { return (x + 15) / 16 * 16; }

int px_fill_videos(PxVideos& v, const int* m_per_video, int B, int* total) {
  memset(&v, 0, sizeof(v));
  VideoFill f;
  if (int rc = fill_videos(m_per_video, B, kMaxObjects, "", v.m, v.off, &f)) return rc;
  *total = f.total;
  return AXVS_OK;
}

int px_check_samples(int k, int kstride, long long P) {
  if (P <= 0 || P > kPxMaxP) return fail(AXVS_ERR_ARG, "P=%lld pixels must be in 1..%lld", P, kPxMaxP);
  if (k < 0 || k > kPxMaxK) return fail(AXVS_ERR_ARG, "k=%d samples must be in 0..%d", k, kPxMaxK);
  if (k > P) return fail(AXVS_ERR_ARG, "k=%d samples out of P=%lld pixels: selected index k out of range", k, P);
  if (kstride < k) return fail(AXVS_ERR_ARG, "kstride=%d is less than k=%d", kstride, k);
  return AXVS_OK;
}

int px_check_insdis(int L, int B, int C, int kmax, int N) {
  if (int rc = check_shape("L", L, B, "N", N)) return rc;
  if (C <= 0 || C > kPxMaxC || C % 4) return fail(AXVS_ERR_ARG, "C=%d feature channels must be a multiple of 4 in 4..%d", C, kPxMaxC);
  if (kmax < 0 || kmax > N || kmax > kMaxObjects) return fail(AXVS_ERR_ARG, "kmax=%d pairs per problem must be in 0..min(N, %d)", kmax, kMaxObjects);
  return AXVS_OK;
}

struct InsdisWs {
  float *F, *G;
  size_t bytes;
};
InsdisWs insdis_ws(void* ws, int L, int B, int C, int kmax, int k) {
  Carver cv(ws);
  InsdisWs w;
  const size_t Kp = ceil16(k);
  w.F = cv.f((size_t)L * B * Kp * ceil16(C));
  w.G = cv.f((size_t)L * B * Kp * ceil16(kmax));
  w.bytes = cv.off;
  return w;
}

PxSaved insdis_saved(void* saved, int L, int B, int k, size_t* bytes) {
  Carver cv(saved);
  PxSaved s;
  const size_t n = (size_t)L * B * ceil16(k);
  s.lse = cv.f(n);
  s.c = cv.f(n);
  s.lossj = cv.f(n);
  s.nnz = cv.f((size_t)L * B);
  if (bytes) *bytes = cv.off;
  return s;
}

struct InsdisCall {
  PxVideos v;
  PxLayers ly;
  int Kp, Cp, Mp;
};

int insdis_gather(const InsdisCall& c, const void* targets, int target_dtype, const long long* cols, const int* idx, int kmax, int share, int L,
                  int B, int N, int C, int P, int k, int kstride, const InsdisWs& w, hipStream_t st) {
  const dim3 grid((c.Kp + 63) / 64, L * B);
  hipLaunchKernelGGL(px_gather_feat_kernel, grid, dim3(256), 0, st, c.ly, idx, B, C, P, k, kstride, c.Kp, c.Cp, w.F);
  if (c.Mp > 0)
    by_target_dtype(target_dtype, [&](auto td) {
      hipLaunchKernelGGL(px_gather_tgt_kernel<td()>, grid, dim3(256), 0, st, c.v, targets, cols, idx, kmax, share, B, N, P, k, kstride, c.Kp, c.Mp, w.G);
    });
  return AXVS_OK;
}

}  // namespace

int axvs_pixel_sample(const void* targets, int target_dtype, const int* m_per_video, const long long* cols, int kmax, int LM, int B, int N,
                      long long P, const float* const* noise, const int* row_matching, const float* row_temperature, const int* row_k, int R,
                      float* area, float* keys, int* idx, int kstride, void* stream) {
  PxVideos v;
  int total = 0;
  if (int rc = check_shape("LM", LM, B, "N", N)) return rc;
  if (int rc = px_fill_videos(v, m_per_video, B, &total)) return rc;
  if (int rc = check_target_dtype(target_dtype)) return rc;
  if (R <= 0 || R > kPxMaxRows) return fail(AXVS_ERR_ARG, "R=%d noise rows must be in 1..%d", R, kPxMaxRows);
  if (kmax < 0 || kmax > N) return fail(AXVS_ERR_ARG, "kmax=%d pairs per problem must be in 0..N=%d", kmax, N);
  if (!noise || !row_matching || !row_temperature || !row_k || !keys || !idx) return fail(AXVS_ERR_ARG, "null pointer");
  if (kmax > 0 && (!targets || !cols || !area)) return fail(AXVS_ERR_ARG, "null pointer");
  if (kmax == 0 && total > 0) return fail(AXVS_ERR_ARG, "kmax=0 with %d objects", total);
  PxRows rw;
  memset(&rw, 0, sizeof(rw));
  rw.R = R;
  for (int r = 0; r < R; ++r) {
    if (int rc = px_check_samples(row_k[r], kstride, P)) return rc;
    if (!noise[r]) return fail(AXVS_ERR_ARG, "null pointer (noise row %d)", r);
    if (row_matching[r] < 0 || row_matching[r] >= LM) return fail(AXVS_ERR_ARG, "row_matching[%d]=%d is outside 0..%d", r, row_matching[r], LM - 1);
    rw.u[r] = noise[r];
    rw.matching[r] = row_matching[r];
    rw.temperature[r] = row_temperature[r];
    rw.k[r] = row_k[r];
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int Pi = (int)P;
  const dim3 kgrid((Pi + 255) / 256, LM * B);
  by_target_dtype(target_dtype, [&](auto td) {
    if (kmax > 0) hipLaunchKernelGGL(px_area_kernel<td()>, dim3(kmax, LM * B), dim3(256), 0, st, v, targets, cols, kmax, B, N, Pi, area);
    hipLaunchKernelGGL(px_key_kernel<td()>, kgrid, dim3(256), 0, st, v, rw, targets, cols, (const float*)area, kmax, B, N, Pi, keys);
  });
  hipLaunchKernelGGL(px_select_kernel, dim3(R * B), dim3(kPxSelThreads), 0, st, rw, (const float*)keys, B, Pi, kstride, idx);
  return last_launch_status();
}

size_t axvs_pixel_insdis_saved_bytes(int L, int B, int k) {
  if (L <= 0 || L > kMaxLayers || B <= 0 || B > kMaxVideos || k < 0 || k > kPxMaxK) {
    fail(AXVS_ERR_ARG, "L=%d must be in 1..%d, B=%d in 1..%d and k=%d in 0..%d", L, kMaxLayers, B, kMaxVideos, k, kPxMaxK);
    return 0;
  }
  size_t bytes = 0;
  insdis_saved(nullptr, L, B, k, &bytes);
  return bytes;
}

size_t axvs_pixel_insdis_workspace_bytes(int L, int B, int C, int kmax, int k) {
  if (px_check_insdis(L, B, C, kmax, kMaxQueries)) return 0;
  if (k < 0 || k > kPxMaxK) {
    fail(AXVS_ERR_ARG, "k=%d samples must be in 0..%d", k, kPxMaxK);
    return 0;
  }
  return std::max<size_t>(insdis_ws(nullptr, L, B, C, kmax, k).bytes, 256);
}

int axvs_pixel_insdis_fwd(const float* const* pixel_feature, const void* targets, int target_dtype, const int* m_per_video, const long long* cols,
                          int kmax, int share_final_matching, int L, int B, int N, int C, long long P, const int* idx, int k, int kstride,
                          float* losses, void* saved, void* workspace, long long workspace_bytes, void* stream) {
  InsdisCall c;
  int total = 0;
  if (int rc = px_check_insdis(L, B, C, kmax, N)) return rc;
  if (int rc = px_fill_videos(c.v, m_per_video, B, &total)) return rc;
  if (int rc = check_target_dtype(target_dtype)) return rc;
  if (int rc = px_check_samples(k, kstride, P)) return rc;
  if (!pixel_feature || !losses || !saved || !workspace || (k > 0 && !idx)) return fail(AXVS_ERR_ARG, "null pointer");
  if (kmax > 0 && (!targets || !cols)) return fail(AXVS_ERR_ARG, "null pointer");
  memset(&c.ly, 0, sizeof(c.ly));
  if (int rc = fill_layers(pixel_feature, L, c.ly.feat)) return rc;
  const size_t need = axvs_pixel_insdis_workspace_bytes(L, B, C, kmax, k);
  if (int rc = check_ws(workspace_bytes, need)) return rc;
  c.Kp = ceil16(k), c.Cp = ceil16(C), c.Mp = ceil16(kmax);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const InsdisWs w = insdis_ws(workspace, L, B, C, kmax, k);
  const PxSaved s = insdis_saved(saved, L, B, k, nullptr);
  if (k > 0) {
    insdis_gather(c, targets, target_dtype, cols, idx, kmax, share_final_matching != 0, L, B, N, C, (int)P, k, kstride, w, st);
    hipLaunchKernelGGL(px_insdis_fwd_kernel, dim3((c.Kp + kPxTJ - 1) / kPxTJ, L * B), dim3(256), 0, st, (const float*)w.F, (const float*)w.G, k, c.Kp,
                       c.Cp, c.Mp, s);
  }
  hipLaunchKernelGGL(px_finish_kernel, dim3(L), dim3(256), 0, st, (const float*)s.lossj, B, k, c.Kp, s.nnz, losses);
  return last_launch_status();
}

int axvs_pixel_insdis_bwd(const float* grad_losses, const float* const* pixel_feature, const void* targets, int target_dtype,
                          const int* m_per_video, const long long* cols, int kmax, int share_final_matching, int L, int B, int N, int C,
                          long long P, const int* idx, int k, int kstride, const void* saved, float* const* d_pixel_feature, void* workspace,
                          long long workspace_bytes, void* stream) {
  InsdisCall c;
  int total = 0;
  if (int rc = px_check_insdis(L, B, C, kmax, N)) return rc;
  if (int rc = px_fill_videos(c.v, m_per_video, B, &total)) return rc;
  if (int rc = check_target_dtype(target_dtype)) return rc;
  if (int rc = px_check_samples(k, kstride, P)) return rc;
  if (!grad_losses || !pixel_feature || !d_pixel_feature || !saved || !workspace || (k > 0 && !idx)) return fail(AXVS_ERR_ARG, "null pointer");
  if (kmax > 0 && (!targets || !cols)) return fail(AXVS_ERR_ARG, "null pointer");
  memset(&c.ly, 0, sizeof(c.ly));
  if (int rc = fill_layers(pixel_feature, L, c.ly.feat)) return rc;
  for (int l = 0; l < L; ++l) c.ly.dfeat[l] = d_pixel_feature[l];      // NULL: that layer's gradient is skipped
  const size_t need = axvs_pixel_insdis_workspace_bytes(L, B, C, kmax, k);
  if (int rc = check_ws(workspace_bytes, need)) return rc;
  if (k == 0) return AXVS_OK;
  c.Kp = ceil16(k), c.Cp = ceil16(C), c.Mp = ceil16(kmax);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const InsdisWs w = insdis_ws(workspace, L, B, C, kmax, k);
  const PxSaved s = insdis_saved(const_cast<void*>(saved), L, B, k, nullptr);
  insdis_gather(c, targets, target_dtype, cols, idx, kmax, share_final_matching != 0, L, B, N, C, (int)P, k, kstride, w, st);
  const dim3 grid((c.Kp + kPxTJ - 1) / kPxTJ, L * B);
  const size_t lds = (size_t)3 * (c.Cp / 16) * 4 * 64 * sizeof(float);      // at most 48 KB
  if (c.Cp <= 128)
    hipLaunchKernelGGL(px_insdis_bwd_kernel<8>, grid, dim3(256), lds, st, c.ly, grad_losses, (const float*)w.F, (const float*)w.G, idx, B, C, (int)P,
                       k, kstride, c.Kp, c.Cp, c.Mp, s);
  else
    hipLaunchKernelGGL(px_insdis_bwd_kernel<16>, grid, dim3(256), lds, st, c.ly, grad_losses, (const float*)w.F, (const float*)w.G, idx, B, C, (int)P,
                       k, kstride, c.Kp, c.Cp, c.Mp, s);
  return last_launch_status();
}

size_t axvs_pixel_semantic_saved_bytes(int B, int k) {
  if (B <= 0 || B > kMaxVideos || k < 0 || k > kPxMaxK) {
    fail(AXVS_ERR_ARG, "B=%d must be in 1..%d and k=%d in 0..%d", B, kMaxVideos, k, kPxMaxK);
    return 0;
  }
  return align_up((size_t)B * k * 4) * 2 + align_up((size_t)B * 4);
}

namespace {
struct SemSaved { float *lse, *lossj, *nnz; };
SemSaved sem_saved(void* p, int B, int k) {
  Carver cv(p);
  SemSaved s;
  s.lse = cv.f((size_t)B * k);
  s.lossj = cv.f((size_t)B * k);
  s.nnz = cv.f(B);
  return s;
}
int sem_check(int B, int Cs, long long P, int k, int kstride, int num_classes) {
  if (B <= 0 || B > kMaxVideos) return fail(AXVS_ERR_ARG, "B=%d videos must be in 1..%d", B, kMaxVideos);
  if (Cs <= 0 || Cs > kPxMaxC) return fail(AXVS_ERR_ARG, "%d class channels must be in 1..%d", Cs, kPxMaxC);
  if (num_classes < 0) return fail(AXVS_ERR_ARG, "num_classes=%d is negative", num_classes);
  return px_check_samples(k, kstride, P);
}
}  // namespace

int axvs_pixel_semantic_fwd(const float* pred, const long long* sem, const int* idx, int k, int kstride, int B, int Cs, long long P,
                            int num_classes, float* loss, void* saved, void* stream) {
  if (int rc = sem_check(B, Cs, P, k, kstride, num_classes)) return rc;
  if (!pred || !sem || !loss || !saved || (k > 0 && !idx)) return fail(AXVS_ERR_ARG, "null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const SemSaved s = sem_saved(saved, B, k);
  if (k > 0)
    hipLaunchKernelGGL(px_semantic_fwd_kernel, dim3((k + 255) / 256, B), dim3(256), 0, st, pred, sem, idx, k, kstride, Cs, (int)P, num_classes, s.lse,
                       s.lossj);
  hipLaunchKernelGGL(px_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)s.lossj, B, k, k, s.nnz, loss);
  return last_launch_status();
}

int axvs_pixel_semantic_bwd(const float* grad_loss, const float* pred, const long long* sem, const int* idx, int k, int kstride, int B, int Cs,
                            long long P, int num_classes, const void* saved, float* d_pred, void* stream) {
  if (int rc = sem_check(B, Cs, P, k, kstride, num_classes)) return rc;
  if (!grad_loss || !pred || !sem || !saved || !d_pred || (k > 0 && !idx)) return fail(AXVS_ERR_ARG, "null pointer");
  if (k == 0) return AXVS_OK;
  const SemSaved s = sem_saved(const_cast<void*>(saved), B, k);
  hipLaunchKernelGGL(px_semantic_bwd_kernel, dim3((k + 255) / 256, B), dim3(256), 0, static_cast<hipStream_t>(stream), grad_loss, pred, sem, idx, B, k,
                     kstride, Cs, (int)P, num_classes, (const float*)s.lse, (const float*)s.nnz, d_pred);
  return last_launch_status();
}
