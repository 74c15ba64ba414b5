// FPN tail of Tube-Link's MSDeformAttnPixelDecoder (TL = MaXTron_Tube-Link/mmdet/models/plugins/msdeformattn_pixel_decoder.py:311-325)
// for a level the encoder does not see:
//   y = GN(lateral_conv1x1(x)) + bilinear(up, size = y.shape, align_corners = False)        TL:313-318
//   c = ReLU(GN(conv3x3(y)))                                                                 TL:319 (ConvModule: conv -> gn -> act)
//   mask_feature = conv1x1(c) + bias                                                         TL:324
// The lateral GEMM is the 1x1 conv + GroupNorm machinery of axvs_glue.h; the kernels below are the merge (GroupNorm apply fused with the
// bilinear upsample-add, f16 channels-last rows out), the 3x3 implicit GEMM with per-tile GroupNorm partial sums, the fixed-order
// statistics reduction, and the mask_feature GEMM's loader / epilogue (GroupNorm apply + ReLU on the A operand, NCHW fp32 out).
#pragma once
#include "axvs_common.h"

namespace axvs {

constexpr int kFpnTH = 8, kFpnTW = 16, kFpnPS = 40;      // tile rows / columns; LDS pixel stride in 16-bit elements (80 B: spreads the banks)

// GroupNorm statistics from per-block partials, in a fixed order (bit-identical from run to run): part [N][nblk][P][2] holds
// (mean, M2 = sum of squares about that mean) per block and entry, the centred form of gn_stats_kernel (axvs_glue.h: no variance by
// E[y^2] - mean^2); group g owns entries [g*cpp, (g+1)*cpp) (cpp = 1: per-group partials of gn_stats_kernel, cpp = channels per
// group: per-channel partials of fpn_conv3x3_kernel).  An entry's count follows from its block: ntx = 0: 64-row blocks of HW = H*W
// rows x `per_row` values (gn_stats_kernel), ntx > 0: the valid pixels of a kFpnTH x kFpnTW tile of an H x W map (fpn_conv3x3_kernel).
// First the mean, then M2 about it.  stats [N][G][2] = (mean, rstd).  Grid (G, N), 256 threads.
__device__ __forceinline__ double fpn_gn_block_count(long long b, int H, int W, int ntx, int per_row) {
  if (ntx == 0) return (double)(gn_block_rows((int)b, H * W) * per_row);
  const int ty = (int)(b / ntx), tx = (int)(b - (long long)ty * ntx);
  return (double)(min(kFpnTH, H - kFpnTH * ty) * min(kFpnTW, W - kFpnTW * tx));
}

__global__ __launch_bounds__(256) void fpn_gn_finalize_kernel(const float* __restrict__ part, int nblk, int P, int cpp, int G, int H, int W, int ntx, int per_row,
                                                              double cnt, float eps, float* __restrict__ stats) {
  __shared__ double sh[256];
  const int g = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const long long items = (long long)nblk * cpp;
  const float* pg = part + ((long long)n * nblk * P + (long long)g * cpp) * 2;
  auto total = [&](double v) {            // fixed tree over the 256 threads; every thread returns the same bits
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) sh[tid] += sh[tid + o];
      __syncthreads();
    }
    return sh[0];
  };
  double s = 0.0;
  for (long long i = tid; i < items; i += 256) {
    const long long b = i / cpp;
    s += fpn_gn_block_count(b, H, W, ntx, per_row) * (double)pg[(b * P + (i - b * cpp)) * 2];
  }
  const double mu = total(s) / cnt;
  double q = 0.0;
  for (long long i = tid; i < items; i += 256) {
    const long long b = i / cpp;
    const float2 v = *reinterpret_cast<const float2*>(pg + (b * P + (i - b * cpp)) * 2);
    const double d = (double)v.x - mu;
    q += (double)v.y + fpn_gn_block_count(b, H, W, ntx, per_row) * d * d;
  }
  const double m2 = total(q);
  if (tid == 0) {
    stats[((long long)n * G + g) * 2] = (float)mu;
    stats[((long long)n * G + g) * 2 + 1] = (float)(1.0 / sqrt(m2 / cnt + (double)eps));
  }
}

// PyTorch's bilinear source index, align_corners = False with the size given (scale = in / out, upsample_bilinear2d's area_pixel_compute_scale):
// src = max((dst + 0.5) * scale - 0.5, 0), i1 = i0 + 1 clamped to the last row / column.
__device__ __forceinline__ void bilin_src(int dst, int in, float scale, int& i0, int& i1, float& l1) {
  float s = ((float)dst + 0.5f) * scale - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = min((int)s, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = s - (float)i0;
}

// merged[n][p][c] = f16((lat[n][p][c] - mean) * rstd * gamma[c] + beta[c] + bilinear(up)[n][p][c]): one thread per 4 channels of a pixel.
// lat: raw lateral conv output, rows [N*HW][C]; up: token rows of the coarser level, row (n, y*Wu + x) at up + n*ub + (y*Wu + x)*uld.
template <bool BF>
__global__ __launch_bounds__(256) void fpn_merge_kernel(const float* __restrict__ lat, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ up, long long ub, long long uld, int Hu,
                                                        int Wu, u16* __restrict__ merged, int N, int H, int W, int C, int G) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int c4 = C / 4;
  const long long total = (long long)N * H * W * c4;
  if (i >= total) return;
  const int c = (int)(i % c4) * 4;
  const long long row = i / c4;
  const int HW = H * W;
  const int n = (int)(row / HW), p = (int)(row - (long long)n * HW);
  const int y = p / W, x = p - y * W;
  const int cg = C / G;
  const float4 v = *reinterpret_cast<const float4*>(lat + row * C + c);
  int y0, y1, x0, x1;
  float ly, lx;
  bilin_src(y, Hu, (float)Hu / (float)H, y0, y1, ly);
  bilin_src(x, Wu, (float)Wu / (float)W, x0, x1, lx);
  const float* ubase = up + n * ub + c;
  const float4 a = *reinterpret_cast<const float4*>(ubase + ((long long)y0 * Wu + x0) * uld);
  const float4 b = *reinterpret_cast<const float4*>(ubase + ((long long)y0 * Wu + x1) * uld);
  const float4 d = *reinterpret_cast<const float4*>(ubase + ((long long)y1 * Wu + x0) * uld);
  const float4 e = *reinterpret_cast<const float4*>(ubase + ((long long)y1 * Wu + x1) * uld);
  const float h0 = 1.f - ly, w0 = 1.f - lx;
  const float va[4] = {v.x, v.y, v.z, v.w}, aa[4] = {a.x, a.y, a.z, a.w}, ba[4] = {b.x, b.y, b.z, b.w}, da[4] = {d.x, d.y, d.z, d.w},
              ea[4] = {e.x, e.y, e.z, e.w};
  u16x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int g = (c + k) / cg;
    const float mu = stats[((long long)n * G + g) * 2], rs = stats[((long long)n * G + g) * 2 + 1];
    const float u = h0 * (w0 * aa[k] + lx * ba[k]) + ly * (w0 * da[k] + lx * ea[k]);   // upsample_bilinear2d's order of terms
    o[k] = H16<BF>::from_f32((va[k] - mu) * rs * gamma[c + k] + beta[c + k] + u);
  }
  *reinterpret_cast<u16x4*>(merged + row * C + c) = o;
}

// 3x3 weights [Cout][Cin][3][3] fp32 -> fragment-order 16-bit blocks: k index kk = (kc*9 + tap)*32 + j (input channel kc*32 + j, tap = 3*ky + kx),
// addressed through wblk_off like every other packed weight.
template <bool BF>
__global__ void fpn_pack3x3_kernel(const float* __restrict__ w, u16* __restrict__ out, int Cin, int Cout) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long K = 9LL * Cin;
  if (idx >= (long long)Cout * K) return;
  const int n = (int)(idx / K);
  const int kk = (int)(idx - (long long)n * K);
  const int blk = kk >> 5, j = kk & 31, kc = blk / 9, tap = blk - kc * 9;
  out[wblk_off(Cout, n, kk)] = H16<BF>::from_f32(w[((long long)n * Cin + kc * 32 + j) * 9 + tap]);
}

// 3x3 convolution, stride 1, zero padding 1, no bias, as an implicit GEMM: M = N*H*W pixels, Nout = Cout, K = 9*Cin.
// Workgroup = an 8 x 16 pixel tile of one frame x 256 output channels; wave w owns channels [64 w, 64 w + 64) of the block: 8 tile rows
// (M fragments) x 4 N fragments of 16x16x32 MFMAs.  Per 32-channel input chunk the (8+2) x (16+2) halo tile is staged in LDS once (zeros
// outside the map: the padding) and read by all nine taps; the next chunk's global loads are in flight during the current chunk's MFMAs
// (two LDS buffers, one barrier per chunk).  Weights come from L2 in fragment order.
// Epilogue: raw fp32 rows y [N*H*W][Cout] and, per (frame, tile, channel), (mean, sum of squares about it) over the tile's pixels ->
// part [N][tiles][Cout][2] (lanes of a channel combined by a fixed xor butterfly).
constexpr int kFpnHalo = (kFpnTH + 2) * (kFpnTW + 2);

template <bool BF>
__global__ __launch_bounds__(256) void fpn_conv3x3_kernel(const u16* __restrict__ xin, const u16* __restrict__ wp, float* __restrict__ y,
                                                          float* __restrict__ part, int H, int W, int Cin, int Cout, int ntx) {
  __shared__ __attribute__((aligned(16))) u16 sx[2][kFpnHalo * kFpnPS];
  const int tile = blockIdx.x, n = blockIdx.z;
  const int ty0 = (tile / ntx) * kFpnTH, tx0 = (tile - (tile / ntx) * ntx) * kFpnTW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fi = lane & 15, fg = lane >> 4;
  const int n0 = blockIdx.y * 256 + wave * 64;
  const int nfr = max(0, min(4, (Cout - n0) / 16));        // valid N fragments of this wave (Cout is a multiple of 32)
  const int nkc = Cin / 32;
  const u16* xbase = xin + (long long)n * H * W * Cin;
  constexpr int kChunks = kFpnHalo * 4;                    // 16-byte chunks of one staged tile
  constexpr int kPer = (kChunks + 255) / 256;
  u16x8 rx[kPer];
  auto fetch = [&](int kc) {
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int ch = tid + 256 * u;
      u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (ch < kChunks) {
        const int pix = ch >> 2, q = ch & 3;
        const int hy = pix / (kFpnTW + 2), hx = pix - hy * (kFpnTW + 2);
        const int gy = ty0 - 1 + hy, gx = tx0 - 1 + hx;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W)
          v = *reinterpret_cast<const u16x8*>(xbase + ((long long)gy * W + gx) * Cin + kc * 32 + q * 8);
      }
      rx[u] = v;
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int ch = tid + 256 * u;
      if (ch < kChunks) *reinterpret_cast<u16x8*>(&sx[buf][(ch >> 2) * kFpnPS + (ch & 3) * 8]) = rx[u];
    }
  };
  f32x4 acc[kFpnTH][4];
#pragma unroll
  for (int a = 0; a < kFpnTH; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  fetch(0);
  stage(0);
  __syncthreads();
  for (int kc = 0; kc < nkc; ++kc) {
    const int buf = kc & 1;
    if (kc + 1 < nkc) fetch(kc + 1);
    if (nfr > 0) {
      const u16* sb = sx[buf];
#pragma unroll 1
      for (int tap = 0; tap < 9; ++tap) {
        const int dy = tap / 3, dx = tap - dy * 3;
        u16x8 b[4];
        const u16* wt = wp + ((long long)(kc * 9 + tap) * Cout + n0) * 32 + lane * 8;     // = wblk_off(Cout, n0 + 16 f + fi, kk + 8 fg)
#pragma unroll
        for (int f = 0; f < 4; ++f) b[f] = f < nfr ? *reinterpret_cast<const u16x8*>(wt + f * 512) : u16x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int mi = 0; mi < kFpnTH; ++mi) {
          const u16x8 a = *reinterpret_cast<const u16x8*>(sb + ((mi + dy) * (kFpnTW + 2) + fi + dx) * kFpnPS + fg * 8);
#pragma unroll
          for (int f = 0; f < 4; ++f) acc[mi][f] = H16<BF>::mfma(a, b[f], acc[mi][f]);
        }
      }
    }
    if (kc + 1 < nkc) stage(buf ^ 1);
    __syncthreads();
  }
  if (nfr == 0) return;
  // D[pixel 4 fg + r][channel fi] of fragment (mi, f): pixel (ty0 + mi, tx0 + 4 fg + r), channel n0 + 16 f + fi
  const int ntiles = gridDim.x;
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    if (f >= nfr) break;
    const int ch = n0 + 16 * f + fi;
    float s = 0.f;
#pragma unroll
    for (int mi = 0; mi < kFpnTH; ++mi) {
      const int gy = ty0 + mi;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gx = tx0 + 4 * fg + r;
        if (gy < H && gx < W) {
          const float v = acc[mi][f][r];
          y[(((long long)n * H + gy) * W + gx) * Cout + ch] = v;
          s += v;
        }
      }
    }
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    // the tile's mean (the same bits on the four lanes of a channel), then the squares about it: the accumulators are still in registers
    const float mu = s / (float)(min(kFpnTH, H - ty0) * min(kFpnTW, W - tx0));
    float q = 0.f;
#pragma unroll
    for (int mi = 0; mi < kFpnTH; ++mi) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (ty0 + mi < H && tx0 + 4 * fg + r < W) {
          const float d = acc[mi][f][r] - mu;
          q += d * d;
        }
      }
    }
    q += __shfl_xor(q, 16, 64);
    q += __shfl_xor(q, 32, 64);
    if (fg == 0) *reinterpret_cast<float2*>(part + (((long long)n * ntiles + tile) * Cout + ch) * 2) = float2{mu, q};
  }
}

// c [N*HW][C] -> ReLU(GroupNorm(c)) as fp32 rows (the level's output when it is returned or feeds a further level)
__global__ __launch_bounds__(256) void fpn_gn_relu_rows_kernel(const float* __restrict__ c, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float* __restrict__ out, long long M, int HW, int C, int G) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int c4 = C / 4;
  if (i >= M * c4) return;
  const int ch = (int)(i % c4) * 4;
  const long long row = i / c4;
  const int n = (int)(row / HW), cg = C / G;
  float4 v = *reinterpret_cast<const float4*>(c + row * C + ch);
  float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int g = (ch + k) / cg;
    o[k] = fmaxf((o[k] - stats[((long long)n * G + g) * 2]) * stats[((long long)n * G + g) * 2 + 1] * gamma[ch + k] + beta[ch + k], 0.f);
  }
  *reinterpret_cast<float4*>(out + row * C + ch) = float4{o[0], o[1], o[2], o[3]};
}

// A operand of the mask_feature GEMM: 8 channels of row m of ReLU(GroupNorm(c)), normalised in the loader (the map is never written)
template <bool BF>
struct ALoadGnRelu {
  static constexpr int kPrefetch = 1;
  const float* c;          // [M][K] raw conv output
  const float* stats;      // [N][G][2] (mean, rstd)
  const float *gamma, *beta;
  int M, K, HW, G;
  __device__ __forceinline__ u16x8 load(int m, int k) const {
    m = min(m, M - 1);
    const int n = m / HW, cg = K / G;
    const float4* s = reinterpret_cast<const float4*>(c + (long long)m * K + k);
    const float4 a = s[0], b = s[1];
    float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int g = (k + e) / cg;
      const float* st = stats + ((long long)n * G + g) * 2;
      v[e] = fmaxf((v[e] - st[0]) * st[1] * gamma[k + e] + beta[k + e], 0.f);
    }
    return cvt8<BF>(v);
  }
};

// epilogue: 4 consecutive output channels n..n+3 of pixel m (+ bias) into an NCHW fp32 map [N][Nout][HW]
struct EpiNCHWBias {
  float* Y;
  const float* bias;
  int HW, Nout;
  __device__ __forceinline__ void store(int m, int n, f32x4 v) const {
    const int f = m / HW, p = m - f * HW;
    float* o = Y + ((long long)f * Nout + n) * HW + p;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[(long long)i * HW] = v[i] + bias[n + i];
  }
};

}  // namespace axvs
