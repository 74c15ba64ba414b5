// Training tier of the pixel decoder's glue (round 6; SURVEY 8f-4 / VERDICT r5 "missing" 4): the 1x1 convolution + GroupNorm projections
// (WC/msdeformattn.py:349-375, used at :412 and :434) forward AND backward, so that the within-clip module's train() mode runs no torch kernel between the
// backbone maps and its output maps.  fp32 tensors, the GEMMs on the training tier's split-precision kernels (axvs_train_gemm.h: three bf16 pieces
// forward -- fp32 accuracy --, two backward), GroupNorm statistics and their gradients in fp32 with fixed summation orders (no atomics).
//   forward   y = x W^T + b            [M = N HW rows, Cout]                   (token rows; an NCHW input is transposed once: axvs_layout.h)
//             mean, rstd per (sample n, group g) over HW x Cout/G values, centred at every level (block, channel, group): no E[y^2] - mean^2
//             out = (y - mean) rstd gamma + beta
//   backward  xhat = (y - mean) rstd;   A[n,c] = sum_p d_out,  B[n,c] = sum_p d_out xhat
//             d_beta = sum_n A,  d_gamma = sum_n B,  S1[n,g] = sum_{c in g} gamma_c A[n,c],  S2[n,g] = sum_{c in g} gamma_c B[n,c]
//             d_y = rstd (gamma d_out - (S1 + xhat S2) / cnt)
//             d_W = d_y^T x,  d_b = column sums of d_y,  d_x = d_y W
// Part of axvs_train.hip's translation unit only: the kernels have internal linkage.
#pragma once
#include "axvs_common.h"
#include "axvs_layout.h"

namespace axvs {
namespace {

// token rows that are a slice of a wider buffer -> contiguous [N][HW][C]
__global__ __launch_bounds__(256) void gt_gather_tokens_kernel(const float* __restrict__ src, float* __restrict__ dst, int HW, int C, long long batch_stride, long long ld,
                                                               long long total4) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int c4 = (int)(i % (C / 4));
  const long long r = i / (C / 4);
  const long long n = r / HW, p = r - n * HW;
  *reinterpret_cast<float4*>(dst + r * C + c4 * 4) = *reinterpret_cast<const float4*>(src + n * batch_stride + p * ld + c4 * 4);
}

// Per-(sample, 64-row block, channel) column sums, part [N][nblk][C][2], fixed order inside the block.
// MODE 0 (forward statistics): (mean of y, M2 = sum of squares of y about it) of the block's rows of the channel.  Never sum y^2, nor y itself: a group whose
//         mean is tens of standard deviations loses (mean / std)^2 ulps in E[y^2] - mean^2, and a long fp32 sum of such values rounds at the sum's size at
//         every step.  One sweep with the block's first row y0 as the reference: a = sum (y - y0), q = sum (y - y0)^2, mean = y0 + a / rows,
//         M2 = q - a^2 / rows.  Merged upwards as in axvs_glue.h's gn_stats_kernel (gt_merge_blocks_kernel, gt_group_stats_kernel).
// MODE 1 (backward): (sum d, sum d xhat), xhat = (y - mean[n,g]) rstd[n,g].
template <int MODE>
__global__ __launch_bounds__(256) void gt_block_colsums_kernel(const float* __restrict__ v, const float* __restrict__ y, const float* __restrict__ stats /* [N][G][2] */,
                                                               float* __restrict__ part, int HW, int C, int G) {
  const int n = blockIdx.y, r0 = blockIdx.x * 64, rows = min(64, HW - r0);
  const int cg = C / G;
  for (int c4 = threadIdx.x; c4 < C / 4; c4 += 256) {
    float4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    float mu[4] = {0.f, 0.f, 0.f, 0.f}, rs[4] = {1.f, 1.f, 1.f, 1.f};
    if (MODE == 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int g = (c4 * 4 + k) / cg;
        mu[k] = stats[((long long)n * G + g) * 2];
        rs[k] = stats[((long long)n * G + g) * 2 + 1];
      }
    }
    float4 sh = {0.f, 0.f, 0.f, 0.f}, e = {0.f, 0.f, 0.f, 0.f};      // MODE 0: the reference (first row), sums of (y - reference)
    if (MODE == 0) sh = *reinterpret_cast<const float4*>(v + ((long long)n * HW + r0) * C + c4 * 4);
    for (int r = 0; r < rows; ++r) {
      const long long o = ((long long)n * HW + r0 + r) * C + c4 * 4;
      const float4 d = *reinterpret_cast<const float4*>(v + o);
      if (MODE == 0) {
        const float4 t = {d.x - sh.x, d.y - sh.y, d.z - sh.z, d.w - sh.w};
        e.x += t.x; e.y += t.y; e.z += t.z; e.w += t.w;
        b.x += t.x * t.x; b.y += t.y * t.y; b.z += t.z * t.z; b.w += t.w * t.w;
      } else {
        a.x += d.x; a.y += d.y; a.z += d.z; a.w += d.w;
        const float4 yy = *reinterpret_cast<const float4*>(y + o);
        b.x += d.x * ((yy.x - mu[0]) * rs[0]); b.y += d.y * ((yy.y - mu[1]) * rs[1]);
        b.z += d.z * ((yy.z - mu[2]) * rs[2]); b.w += d.w * ((yy.w - mu[3]) * rs[3]);
      }
    }
    if (MODE == 0) {
      const float inv = 1.f / (float)rows;
      a = float4{sh.x + e.x * inv, sh.y + e.y * inv, sh.z + e.z * inv, sh.w + e.w * inv};
      b = float4{fmaxf(b.x - e.x * e.x * inv, 0.f), fmaxf(b.y - e.y * e.y * inv, 0.f), fmaxf(b.z - e.z * e.z * inv, 0.f), fmaxf(b.w - e.w * e.w * inv, 0.f)};
    }
    float* o = part + (((long long)n * gridDim.x + blockIdx.x) * C + c4 * 4) * 2;
    o[0] = a.x; o[1] = b.x; o[2] = a.y; o[3] = b.y; o[4] = a.z; o[5] = b.z; o[6] = a.w; o[7] = b.w;
  }
}

// ab [N][C][2] = sum over the blocks (block order): the backward's (sum d, sum d xhat)
__global__ __launch_bounds__(256) void gt_sum_blocks_kernel(const float* __restrict__ part, float* __restrict__ ab, int nblk, int C, long long total /* N * C */) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long n = i / C;
  const int c = (int)(i - n * C);
  float a = 0.f, b = 0.f;
  for (int k = 0; k < nblk; ++k) {
    const float* p = part + (((long long)n * nblk + k) * C + c) * 2;
    a += p[0]; b += p[1];
  }
  ab[i * 2] = a; ab[i * 2 + 1] = b;
}

// forward statistics, blocks -> channel: ab [N][C][2] = (mean, M2 about it) of the channel from the blocks' (mean, M2) in block order, about block 0's mean
__global__ __launch_bounds__(256) void gt_merge_blocks_kernel(const float* __restrict__ part, float* __restrict__ ab, int nblk, int C, int HW, long long total /* N * C */) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long n = i / C;
  const int c = (int)(i - n * C);
  const float* p = part + ((long long)n * nblk * C + c) * 2;
  const float ref = p[0];
  float s = 0.f;
  for (int k = 0; k < nblk; ++k) s += (float)min(64, HW - 64 * k) * (p[(long long)k * C * 2] - ref);
  const float mu = ref + s / (float)HW;
  float m2 = 0.f;
  for (int k = 0; k < nblk; ++k) {
    const float d = p[(long long)k * C * 2] - mu;
    m2 += p[(long long)k * C * 2 + 1] + (float)min(64, HW - 64 * k) * d * d;
  }
  ab[i * 2] = mu; ab[i * 2 + 1] = m2;
}

// forward statistics, channels -> group: stats [N][G] = (mean, rstd) from ab = (mean, M2) per (n, c) over HW values each, channels of a group in order, in double
__global__ __launch_bounds__(256) void gt_group_stats_kernel(const float* __restrict__ ab, float* __restrict__ stats, int C, int G, int HW, float eps, int total /* N * G */) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int n = i / G, g = i - n * G, cg = C / G;
  const float* a = ab + ((long long)n * C + (long long)g * cg) * 2;
  double s = 0.0, m2 = 0.0;
  for (int c = 0; c < cg; ++c) s += a[c * 2];
  const double mu = s / cg;
  for (int c = 0; c < cg; ++c) {
    const double d = (double)a[c * 2] - mu;
    m2 += (double)a[c * 2 + 1] + HW * d * d;
  }
  stats[i * 2] = (float)mu;
  stats[i * 2 + 1] = (float)(1.0 / sqrt(m2 / ((double)HW * cg) + (double)eps));
}

// out = (y - mean) rstd gamma + beta on token rows (contiguous y; out rows at n * out_batch_stride + p * out_ld)
__global__ __launch_bounds__(256) void gt_gn_apply_kernel(const float* __restrict__ y, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float* __restrict__ out, int HW, int C, int G, long long out_batch_stride,
                                                          long long out_ld, long long total4) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int c = (int)(i % (C / 4)) * 4;
  const long long r = i / (C / 4);
  const long long n = r / HW, p = r - n * HW;
  const float4 v = *reinterpret_cast<const float4*>(y + r * C + c);
  const float4 ga = *reinterpret_cast<const float4*>(gamma + c), be = *reinterpret_cast<const float4*>(beta + c);
  const int cg = C / G;
  float o[4] = {v.x, v.y, v.z, v.w};
  const float gg[4] = {ga.x, ga.y, ga.z, ga.w}, bb[4] = {be.x, be.y, be.z, be.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float* st = stats + (n * G + (c + k) / cg) * 2;
    o[k] = (o[k] - st[0]) * st[1] * gg[k] + bb[k];
  }
  *reinterpret_cast<float4*>(out + n * out_batch_stride + p * out_ld + c) = float4{o[0], o[1], o[2], o[3]};
}

// backward finalisation: d_beta[c] = sum_n A, d_gamma[c] = sum_n B (sample order); S [N][G][2] = sum_{c in g} gamma_c (A, B)
__global__ __launch_bounds__(256) void gt_gn_bwd_params_kernel(const float* __restrict__ ab, float* __restrict__ d_gamma, float* __restrict__ d_beta, int N, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float a = 0.f, b = 0.f;
  for (int n = 0; n < N; ++n) { a += ab[((long long)n * C + c) * 2]; b += ab[((long long)n * C + c) * 2 + 1]; }
  d_beta[c] = a;
  d_gamma[c] = b;
}
__global__ __launch_bounds__(256) void gt_gn_bwd_groups_kernel(const float* __restrict__ ab, const float* __restrict__ gamma, float* __restrict__ S, int C, int G, int total) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int n = i / G, g = i - n * G, cg = C / G;
  float s1 = 0.f, s2 = 0.f;
  for (int c = g * cg; c < (g + 1) * cg; ++c) {
    s1 += gamma[c] * ab[((long long)n * C + c) * 2];
    s2 += gamma[c] * ab[((long long)n * C + c) * 2 + 1];
  }
  S[i * 2] = s1; S[i * 2 + 1] = s2;
}
// d_y = rstd (gamma d - (S1 + xhat S2) / cnt), written over d (contiguous token rows)
__global__ __launch_bounds__(256) void gt_gn_bwd_apply_kernel(float* __restrict__ d, const float* __restrict__ y, const float* __restrict__ stats, const float* __restrict__ S,
                                                              const float* __restrict__ gamma, int HW, int C, int G, float inv_cnt, long long total4) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int c = (int)(i % (C / 4)) * 4;
  const long long r = i / (C / 4);
  const long long n = r / HW;
  const float4 dv = *reinterpret_cast<const float4*>(d + r * C + c), yv = *reinterpret_cast<const float4*>(y + r * C + c);
  const float4 ga = *reinterpret_cast<const float4*>(gamma + c);
  const int cg = C / G;
  float dd[4] = {dv.x, dv.y, dv.z, dv.w};
  const float yy[4] = {yv.x, yv.y, yv.z, yv.w}, gg[4] = {ga.x, ga.y, ga.z, ga.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long sg = (n * G + (c + k) / cg) * 2;
    const float mu = stats[sg], rs = stats[sg + 1];
    const float xh = (yy[k] - mu) * rs;
    dd[k] = rs * (gg[k] * dd[k] - (S[sg] + xh * S[sg + 1]) * inv_cnt);
  }
  *reinterpret_cast<float4*>(d + r * C + c) = float4{dd[0], dd[1], dd[2], dd[3]};
}

}  // namespace
}  // namespace axvs
