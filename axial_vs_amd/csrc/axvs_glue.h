// Pixel-decoder glue around the within-clip stages: 1x1 conv + GroupNorm projections between backbone NCHW maps and
// token rows, 2-D sine position embedding.  Reference: WC/msdeformattn.py:349-375 (input_proj / output_proj), :404-435
// (forward_features), WC/pos_embeddings.py:12-53 (PositionEmbeddingSine).
#pragma once
#include "axvs_common.h"
#include "axvs_layout.h"

namespace axvs {

// A-operand loader for a 1x1 convolution that reads the backbone map where it lies: x [N][Cin][HW] fp32 (NCHW), row m = n*HW + p,
// k = input channel.  Lanes of a wave hold consecutive m, so each of the 8 strided loads is coalesced across the wave.
// Split precision (hi | hi | lo along a 3x longer K, see ALoadRowsF32Split3): the projection output feeds a GroupNorm directly.
template <bool BF>
struct ALoadNCHWSplit3 {
  static constexpr int kPrefetch = 1;
  const float* x;
  int M, K, HW;          // M = N*HW rows, K = Cin
  __device__ __forceinline__ u16x8 load(int m, int k) const {
    m = min(m, M - 1);
    const int part = k / K, kk = k - part * K;
    const int n = m / HW, p = m - n * HW;
    const float* s = x + ((long long)n * K + kk) * HW + p;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = s[(long long)i * HW];
    u16x8 hi = cvt8<BF>(v);
    if (part < 2) return hi;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] -= H16<BF>::to_f32(hi[i]);
    return cvt8<BF>(v);
  }
};

// The transposing stage in front of the 128 x 128 three-piece GEMM for the input projections of the large pyramid levels is nchw_to_rows()
// (axvs_layout.h; round 5: ALoadNCHWSplit3 above reads every element three times, 64 bytes at a time -- 63 TFLOP/s at [32786 x 256 x 512]).

// y[i] = bias[col(i)] + p_0[i] + p_1[i] + ... (z order): the split-K partials of the 128 x 128 GEMM
__global__ __launch_bounds__(256) void splitk_sum_bias_kernel(const float* __restrict__ part, float* __restrict__ y, int Z, long long stride, const float* __restrict__ bias,
                                                              int N, long long tot4) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= tot4) return;
  float4 a = *reinterpret_cast<const float4*>(part + 4 * i);
  for (int z = 1; z < Z; ++z) {
    const float4 p = *reinterpret_cast<const float4*>(part + z * stride + 4 * i);
    a.x += p.x; a.y += p.y; a.z += p.z; a.w += p.w;
  }
  const float4 b = *reinterpret_cast<const float4*>(bias + (int)((4 * i) % N));
  *reinterpret_cast<float4*>(y + 4 * i) = float4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
}

// token rows that may be a slice of a wider buffer: row (n, p) at x + n*batch_stride + p*ld  (split precision as above)
template <bool BF>
struct ALoadTokensSplit3 {
  static constexpr int kPrefetch = 1;
  const float* x;
  int M, K, HW;
  long long batch_stride, ld;
  __device__ __forceinline__ u16x8 load(int m, int k) const {
    m = min(m, M - 1);
    const int part = k / K, kk = k - part * K;
    const int n = m / HW, p = m - n * HW;
    const float4* s = reinterpret_cast<const float4*>(x + n * batch_stride + p * ld + kk);
    const float4 a = s[0], b = s[1];
    float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    u16x8 hi = cvt8<BF>(v);
    if (part < 2) return hi;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] -= H16<BF>::to_f32(hi[i]);
    return cvt8<BF>(v);
  }
};

// GroupNorm statistics over token rows y [N*HW][C], deterministic (no atomics: a 1-ulp change of a statistic flips 16-bit
// roundings downstream and shows up as run-to-run differences of whole f16 ulps), and CENTRED: the variance is never formed as
// E[y^2] - mean^2 (a projection of post-ReLU backbone maps has groups whose mean is tens of standard deviations; the raw second
// moment loses (mean / std)^2 ulps there, torch's group_norm only mean / std).  Every level carries (count, mean, M2 = sum of
// squares about its own mean); the counts follow from the indices and are not stored.  A parent of children i is, in a fixed order,
//     mean = ref + sum_i n_i (mean_i - ref) / n      (ref = the first child's mean: the sum is of std-sized terms, so the mean is
//     M2   = sum_i M2_i + n_i (mean_i - mean)^2       rounded at ITS size once per level, not once per addend)
// Stage 1: one workgroup = 64 rows of one sample, thread = 4 consecutive channels of every RG-th row, one sweep with the thread's
// first row y0 as the reference: a = sum (y - y0), q = sum (y - y0)^2 -> mean = y0 + a / n, M2 = q - a^2 / n per (row group,
// channel) in LDS -> per (block, group), row groups then channels: partial [N][nblk][G][2] = (mean, M2) of the block's rows x cg values.
// Stage 2: the blocks' partials merged in block order by whoever needs them (gn_apply_kernel's prologue, fpn_gn_finalize_kernel).
__device__ __forceinline__ int gn_block_rows(int b, int HW) { return min(64, HW - 64 * b); }      // rows of 64-row block b

__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ y, float* __restrict__ partial, int HW, int C, int G) {
  extern __shared__ float chs[];                        // [RG][C] means | [RG][C] M2 about them (RG row groups)
  const int n = blockIdx.y, r0 = blockIdx.x * 64, tid = threadIdx.x;
  const int rows = min(64, HW - r0);
  // threads = `lanes` float4 columns x RG row groups (C = 256: 64 x 4, 16 rows each, loads independent of one another): the
  // serial 64-row loop of round 1 made this kernel a 18 us latency chain whatever the problem size
  const int n4 = C / 4, lanes = n4 < 256 ? n4 : 256, RG = 256 / lanes;
  const int col = tid % lanes, g = tid / lanes;
  float* chq = chs + RG * C;
  for (int c0 = 0; c0 < n4; c0 += lanes) {
    const int c4 = c0 + col;
    if (g < RG && c4 < n4) {
      const float* yc = y + ((long long)n * HW + r0) * C + c4 * 4;
      float4 a = {0.f, 0.f, 0.f, 0.f}, q = {0.f, 0.f, 0.f, 0.f}, v0 = {0.f, 0.f, 0.f, 0.f};
      if (g < rows) v0 = *reinterpret_cast<const float4*>(yc + (long long)g * C);
#pragma unroll 4
      for (int r = g; r < rows; r += RG) {
        const float4 v = *reinterpret_cast<const float4*>(yc + (long long)r * C);
        const float4 d = {v.x - v0.x, v.y - v0.y, v.z - v0.z, v.w - v0.w};
        a.x += d.x; a.y += d.y; a.z += d.z; a.w += d.w;
        q.x += d.x * d.x; q.y += d.y * d.y; q.z += d.z * d.z; q.w += d.w * d.w;
      }
      const float inv = 1.f / (float)max(1, (rows - g + RG - 1) / RG);      // my rows: g, g + RG, ...  (none: the entry is not read)
      *reinterpret_cast<float4*>(chs + g * C + c4 * 4) = float4{v0.x + a.x * inv, v0.y + a.y * inv, v0.z + a.z * inv, v0.w + a.w * inv};
      *reinterpret_cast<float4*>(chq + g * C + c4 * 4) =
          float4{fmaxf(q.x - a.x * a.x * inv, 0.f), fmaxf(q.y - a.y * a.y * inv, 0.f), fmaxf(q.z - a.z * a.z * inv, 0.f), fmaxf(q.w - a.w * a.w * inv, 0.f)};
    }
  }
  __syncthreads();
  const int cg = C / G, jn = min(RG, rows);
  for (int gg = tid; gg < G; gg += 256) {
    const float ref = chs[gg * cg];
    float s = 0.f;
    for (int j = 0; j < jn; ++j) {                        // fixed order: row groups, then channels
      const float nj = (float)((rows - j + RG - 1) / RG);
      for (int c = gg * cg; c < (gg + 1) * cg; ++c) s += nj * (chs[j * C + c] - ref);
    }
    const float mu = ref + s / (float)(rows * cg);
    float m2 = 0.f;
    for (int j = 0; j < jn; ++j) {
      const float nj = (float)((rows - j + RG - 1) / RG);
      for (int c = gg * cg; c < (gg + 1) * cg; ++c) {
        const float d = chs[j * C + c] - mu;
        m2 += chq[j * C + c] + nj * d * d;
      }
    }
    float* o = partial + (((long long)n * gridDim.x + blockIdx.x) * G + gg) * 2;
    o[0] = mu; o[1] = m2;
  }
}

// (Round 4: the second stage -- per (n, g): lanes stride over the blocks' partials, then a fixed-order butterfly -- is the first thing
//  gn_apply_kernel does for the groups its 64 channels touch, instead of a launch of its own: 3 launches per GroupNorm -> 2.)
// GroupNorm apply: out = (y - mean_g) * rstd_g * gamma_c + beta_c; token rows in, token rows (in place allowed) or NCHW out.
// Workgroup = 64 pixels x 64 channels of one sample, transposed through LDS for the NCHW store.
template <bool OUT_NCHW>
__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ y, const float* __restrict__ partial, int nblk,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float* __restrict__ out, int HW, int C, int G, float eps, long long out_ld,
                                                       long long out_batch_stride) {
  __shared__ float tile[64][65];
  __shared__ float gmu[64], grs[64];                   // mean / rstd of the (at most 33: channels per group >= 2) groups of my 64 channels
  const int n = blockIdx.z, p0 = blockIdx.x * 64, c0 = blockIdx.y * 64, tid = threadIdx.x;
  const int cg = C / G;
  const float cnt = (float)HW * cg;
  {
    // statistics of my groups from the blocks' (mean, M2), in a fixed order (every workgroup that needs a group computes the same
    // bits): one wave per group, lanes stride over the blocks, xor butterfly; first the mean (about block 0's), then M2 about it
    const int g_first = c0 / cg, g_last = min(c0 + 63, C - 1) / cg, lane = tid & 63;
    for (int g = g_first + (tid >> 6); g <= g_last; g += 4) {
      const float* pg = partial + ((long long)n * nblk * G + g) * 2;
      // eight partials per lane in flight at a time, added in block order as before (round 6: one dependent load per 64 blocks made this prologue a
      // chain of L2 round trips in front of EVERY workgroup's 16 KB of work on the large maps: 257 blocks at the shipped VIPSeg res3 size);
      // the first eight stay in registers for the second sweep, blocks past 512 are read again
      float2 pv[8];
      float nb[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int b = lane + 64 * u;
        pv[u] = b < nblk ? *reinterpret_cast<const float2*>(pg + (long long)b * G * 2) : float2{0.f, 0.f};
        nb[u] = b < nblk ? (float)(gn_block_rows(b, HW) * cg) : 0.f;
      }
      const float ref = pg[0];                // block 0's mean: the reference of this level (the same bits in every lane and workgroup)
      float s = 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u) s += nb[u] * (pv[u].x - ref);
      for (int b = lane + 512; b < nblk; b += 64) s += (float)(gn_block_rows(b, HW) * cg) * (pg[(long long)b * G * 2] - ref);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      const float mu = ref + s / cnt;
      float q = 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float d = pv[u].x - mu;
        q += pv[u].y + nb[u] * d * d;
      }
      for (int b = lane + 512; b < nblk; b += 64) {
        const float2 p = *reinterpret_cast<const float2*>(pg + (long long)b * G * 2);
        const float d = p.x - mu;
        q += p.y + (float)(gn_block_rows(b, HW) * cg) * d * d;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
      if (lane == 0) {
        gmu[g - g_first] = mu;
        grs[g - g_first] = 1.f / sqrtf(q / cnt + eps);      // correctly rounded steps (rsqrtf is an approximation of a few ulps; one lane per group pays)
      }
    }
    __syncthreads();
  }
  const int g_first = c0 / cg;
  // read: thread -> (pixel row, 16 channels) as float4 x 4: 64 rows x 16 float4
  for (int i = tid; i < 64 * 16; i += 256) {
    const int r = i >> 4, c4 = (i & 15) * 4;
    const int p = p0 + r, c = c0 + c4;
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (p < HW && c < C) {
      v = *reinterpret_cast<const float4*>(y + ((long long)n * HW + p) * C + c);
      float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int g = (c + k) / cg - g_first;
        o[k] = (o[k] - gmu[g]) * grs[g] * gamma[c + k] + beta[c + k];
      }
      v = float4{o[0], o[1], o[2], o[3]};
      if (!OUT_NCHW) *reinterpret_cast<float4*>(out + (long long)n * out_batch_stride + (long long)p * out_ld + c) = v;
    }
    if (OUT_NCHW) {
      tile[r][c4] = v.x; tile[r][c4 + 1] = v.y; tile[r][c4 + 2] = v.z; tile[r][c4 + 3] = v.w;
    }
  }
  if (OUT_NCHW) {
    __syncthreads();
    for (int i = tid; i < 64 * 64; i += 256) {
      const int cc = i >> 6, r = i & 63;
      if (p0 + r < HW && c0 + cc < C) out[(long long)n * out_batch_stride + (long long)(c0 + cc) * HW + p0 + r] = tile[r][cc];
    }
  }
}

// PositionEmbeddingSine(num_pos_feats = C/2, normalize, mask = None) in token form, plus an optional per-channel vector (the
// level embedding, WC/msdeformattn.py:113-114): pos[n][row0 + y*W + x][c], rows of a level inside a [N][S][C] buffer.
__global__ void pos2d_kernel(float* __restrict__ pos, const float* __restrict__ add, int N, int H, int W, int C, long long S, long long row0,
                             float temperature, int normalize, float scale) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)H * W * C;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  const long long r = idx / C;
  const int x = (int)(r % W), y = (int)(r / W);
  const int n = C / 2;
  float ye = (float)(y + 1), xe = (float)(x + 1);
  if (normalize) {
    const float eps = 1e-6f;
    ye = ye / ((float)H + eps) * scale;
    xe = xe / ((float)W + eps) * scale;
  }
  const int cc = c < n ? c : c - n;                       // first half: y, second half: x (pos_embeddings.py:52)
  const float dim_t = powf(temperature, 2.f * (float)(cc / 2) / (float)n);
  const float a = (c < n ? ye : xe) / dim_t;
  float v = (cc & 1) ? cosf(a) : sinf(a);
  if (add) v += add[c];
  for (int b = 0; b < N; ++b) pos[((long long)b * S + row0 + r) * C + c] = v;
}

__global__ void scaled_residual_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                       const float* __restrict__ gamma, float* __restrict__ out, size_t n, int C) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a[i] + gamma[i % C] * b[i];
}

}  // namespace axvs
