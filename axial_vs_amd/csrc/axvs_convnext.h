// Kernels of the ConvNeXt / ConvNeXtV2 backbone (eval forward): everything that is not a pointwise Linear layer.  The Linear layers (the
// patchify convolutions as GEMMs over gathered patches, pwconv1 + gelu, pwconv2 + residual) run on the three-piece split-precision GEMM
// (axvs_gemm_nt.h).  Maps travel channels-last from the stem to the last block: rows [N][h][w][C] fp32.
//
//   cnx_stem_gather_kernel  image [N, 3, H, W] -> rows [N*h0*w0][48] of the 4 x 4 / stride-4 patches through the reference's
//                           F.pad(x, (1, 2, 1, 2)): the zeros come from the index test
//   cnx_row_ln_kernel       rows [P][C] -> LayerNorm (eps 1e-6) of each row: one wave per row, the row in registers
//   cnx_down_kernel         rows [N][h][w][C] -> rows [N][h2][w2][4 C] of the 2 x 2 / stride-2 patches of LayerNorm(F.pad(x, (0, 1, 0, 1))):
//                           a position past the map is a zero vector IN FRONT of the LayerNorm, so it comes out as the LayerNorm's bias
//   cnx_dwln_kernel         depthwise 7 x 7 (padding 3, bias) + channels-last LayerNorm in one launch: a workgroup owns TH x 16 pixels
//                           (TH 8, 4 or 2 by the map's size); per chunk of 64 channels the (TH + 6) x 22 halo tile goes through LDS and
//                           the raw sums go to the output rows; then each pixel's row is read back (by the workgroup that wrote it),
//                           normalised in registers and rewritten
//   cnx_sumsq_kernel        GRN: per (frame, chunk of 256 pixels, channel) sums of squares of the hidden rows
//   cnx_grn_gx_kernel       GRN: chunk sums in chunk order -> Gx
//   cnx_grn_scale_kernel    GRN: Gx -> s = 1 + gamma Gx / (mean_c Gx + 1e-6) per frame
//   cnx_scale_w_kernel      W2 diag(s_n): pwconv2's weight of one frame
// and rows [N*h*w][C] -> [N, C, h, w] for the outputs: rows_to_nchw() (axvs_layout.h).
// No kernel waits for another workgroup and none adds floating-point numbers atomically: equal inputs give equal bits, and a frame's
// bits do not depend on the frames stacked beside it.
#pragma once
#include <hip/hip_runtime.h>

#include "axvs_common.h"

namespace axvs {

constexpr int kCnxTW = 16, kCnxHaloW = kCnxTW + 6;            // a workgroup of the depthwise kernel owns TH (8, 4 or 2) x 16 output pixels
constexpr int kCnxCC = 64;                                    // channels per LDS pass
constexpr int cnx_dw_lds(int th) { return (th + 6) * kCnxHaloW * kCnxCC * (int)sizeof(float); }
constexpr int kCnxDwWgs = 512;                                // the tallest tile that still gives this many workgroups is taken
constexpr int kCnxGrnChunk = 256;                             // pixels per partial sum of the GRN statistics
constexpr int kCnxMaxC = 2048;                                // a row in registers: eight float4 per lane

// ---- a row of C <= 2048 channels in the registers of one wave: lane l holds channels 4 (l + 64 j) .. + 3 ------------------------------
__device__ __forceinline__ void cnx_row_load(const float* src, int C, int lane, float4 (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = 4 * (lane + 64 * j);
    v[j] = c < C ? *reinterpret_cast<const float4*>(src + c) : float4{0.f, 0.f, 0.f, 0.f};
  }
}

// LayerNorm over the row (two passes: the mean, then the centred squares), dst = g (x - mean) / sqrt(var + 1e-6) + b
__device__ __forceinline__ void cnx_row_norm_store(const float4 (&v)[8], const float* __restrict__ g, const float* __restrict__ b, float* dst, int C, int lane) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);      // (zeros past C)
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) s = wave_xor_sum(s, o);
  const float mean = s / (float)C;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (4 * (lane + 64 * j) < C) {
      const float d0 = v[j].x - mean, d1 = v[j].y - mean, d2 = v[j].z - mean, d3 = v[j].w - mean;
      q = fmaf(d0, d0, q), q = fmaf(d1, d1, q), q = fmaf(d2, d2, q), q = fmaf(d3, d3, q);
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) q = wave_xor_sum(q, o);
  const float den = sqrtf(q / (float)C + 1e-6f);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = 4 * (lane + 64 * j);
    if (c < C) {
      const float4 gg = *reinterpret_cast<const float4*>(g + c), bb = *reinterpret_cast<const float4*>(b + c);
      *reinterpret_cast<float4*>(dst + c) = float4{gg.x * ((v[j].x - mean) / den) + bb.x, gg.y * ((v[j].y - mean) / den) + bb.y,
                                                   gg.z * ((v[j].z - mean) / den) + bb.z, gg.w * ((v[j].w - mean) / den) + bb.w};
    }
  }
}

// ---- the stem's patches --------------------------------------------------------------------------------------------------------------------
// out row p = (n, oy, ox), element c*16 + ky*4 + kx (the convolution weight's own order) = image[n][c][4 oy + ky - 1][4 ox + kx - 1], zero
// outside the image.  One thread per (p, c, ky): four kx.  grid ceil(total / 256), total = N*h0*w0*12.
__global__ __launch_bounds__(256) void cnx_stem_gather_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W, int h0, int w0, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int q = (int)(i % 12), c = q >> 2, ky = q & 3;
  const size_t p = i / 12;
  const int ox = (int)(p % w0), oy = (int)(p / w0 % h0);
  const size_t n = p / w0 / h0;
  const int y = 4 * oy + ky - 1, x0 = 4 * ox - 1;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (y >= 0 && y < H) {
    const float* const src = x + ((n * 3 + c) * H + y) * (size_t)W;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (x0 + e >= 0 && x0 + e < W) v[e] = src[x0 + e];
  }
  reinterpret_cast<float4*>(out)[i] = float4{v[0], v[1], v[2], v[3]};
}

// ---- LayerNorm of rows [P][C], in place or not.  grid ceil(P / 4), 256 threads: a wave per row ----------------------------------------
__global__ __launch_bounds__(256) void cnx_row_ln_kernel(const float* src, const float* __restrict__ g, const float* __restrict__ b, float* dst, int C, size_t P) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= P) return;
  float4 v[8];
  cnx_row_load(src + row * C, C, lane, v);
  cnx_row_norm_store(v, g, b, dst + row * C, C, lane);
}

// ---- the downsample layers' patches ------------------------------------------------------------------------------------------------------------
// out row (n, oy, ox), elements (2 ky + kx) C + c = LayerNorm(x[n][2 oy + ky][2 ox + kx])[c]; past the map: b[c].
// grid ceil(N*h2*w2*4 / 4), 256 threads: a wave per (output pixel, slot).
__global__ __launch_bounds__(256) void cnx_down_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b, float* __restrict__ out,
                                                       int C, int h, int w, int h2, int w2, size_t total) {
  const int lane = threadIdx.x & 63;
  const size_t id = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (id >= total) return;
  const int slot = (int)(id & 3);
  const size_t op = id >> 2;
  const int ox = (int)(op % w2), oy = (int)(op / w2 % h2);
  const size_t n = op / w2 / h2;
  const int y = 2 * oy + (slot >> 1), xx = 2 * ox + (slot & 1);
  float* const dst = out + (op * 4 + slot) * C;
  if (y < h && xx < w) {
    float4 v[8];
    cnx_row_load(x + ((n * h + y) * w + xx) * C, C, lane, v);
    cnx_row_norm_store(v, g, b, dst, C, lane);
  } else {
    for (int c = 4 * lane; c < C; c += 256) *reinterpret_cast<float4*>(dst + c) = *reinterpret_cast<const float4*>(b + c);
  }
}

// ---- depthwise 7 x 7 + LayerNorm ------------------------------------------------------------------------------------------------------------
// x rows [N][h][w][C], taps [49][C] (tap ky*7 + kx, the channel fastest), bias / g / b [C], out rows [N][h][w][C].
// A workgroup owns TH x 16 output pixels.  Thread (channel pair tid & 31, tile columns tid >> 5 and + 8) owns the TH output rows of a
// column: its 49 taps stay in registers, the TH + 6 halo rows pass once through them, each feeding the outputs it reaches (taps in
// (ky, kx) order per output, after the bias: the same sums whatever TH).  A workgroup's raw rows go to `out` chunk after chunk; behind
// the barrier its waves read them back four pixels at a time (L1 / L2: the workgroup wrote them itself), normalise in registers and
// write the rows again -- no second full-size buffer, no statistics by E[x^2] - mean^2.
// A workgroup walks its channel chunks one after the other, so a small map of many channels (49 x 85 x 768, 27 blocks of ConvNeXt-L)
// wants short tiles: more workgroups, each with less to walk, for more halo traffic out of L2.
// grid (ceil(w/16), ceil(h/TH), N), 256 threads, dynamic LDS cnx_dw_lds(TH).
template <int TH>
__global__ __launch_bounds__(256) void cnx_dwln_kernel(const float* __restrict__ x, const float* __restrict__ taps, const float* __restrict__ bias,
                                                       const float* __restrict__ g, const float* __restrict__ b, float* out, int C, int h, int w) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, cp = tid & 31, pg = tid >> 5;
  const int x0 = (int)blockIdx.x * kCnxTW, y0 = (int)blockIdx.y * TH;
  const size_t base = (size_t)blockIdx.z * h * w;
  for (int c0 = 0; c0 < C; c0 += kCnxCC) {
    __syncthreads();            // the previous chunk's tile has been read
    for (int i = tid; i < (TH + 6) * kCnxHaloW * (kCnxCC / 4); i += 256) {
      const int q = i & 15, pi = i >> 4, ty = pi / kCnxHaloW, tx = pi % kCnxHaloW;
      const int y = y0 + ty - 3, xx = x0 + tx - 3, c = c0 + 4 * q;
      float4 v = {0.f, 0.f, 0.f, 0.f};
      if (c < C && y >= 0 && y < h && xx >= 0 && xx < w) v = *reinterpret_cast<const float4*>(x + (base + (size_t)y * w + xx) * C + c);
      *reinterpret_cast<float4*>(smem + pi * kCnxCC + 4 * q) = v;
    }
    __syncthreads();
    const int c = c0 + 2 * cp;
    if (c < C) {
      float2 tp[49];
#pragma unroll
      for (int t = 0; t < 49; ++t) tp[t] = *reinterpret_cast<const float2*>(taps + (size_t)t * C + c);
      const float2 b2 = *reinterpret_cast<const float2*>(bias + c);
      for (int px = pg; px < kCnxTW && x0 + px < w; px += 8) {
        float2 acc[TH];
#pragma unroll
        for (int y = 0; y < TH; ++y) acc[y] = b2;
#pragma unroll
        for (int r = 0; r < (TH + 6); ++r) {
          float2 in[7];
#pragma unroll
          for (int kx = 0; kx < 7; ++kx) in[kx] = *reinterpret_cast<const float2*>(smem + (r * kCnxHaloW + px + kx) * kCnxCC + 2 * cp);
#pragma unroll
          for (int y = TH - 1; y >= 0; --y) {
            const int ky = r - y;
            if (ky < 0 || ky > 6) continue;
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
              const float2 t = tp[ky * 7 + kx];
              acc[y].x = fmaf(in[kx].x, t.x, acc[y].x), acc[y].y = fmaf(in[kx].y, t.y, acc[y].y);
            }
          }
        }
#pragma unroll
        for (int y = 0; y < TH; ++y)
          if (y0 + y < h) *reinterpret_cast<float2*>(out + (base + (size_t)(y0 + y) * w + x0 + px) * C + c) = acc[y];
      }
    }
  }
  __syncthreads();              // the tile's raw rows are written, and visible to the workgroup
  const int lane = tid & 63;
  // a wave's 32 pixels, four at a time: the four rows are requested before the first is reduced (one row at a time the wave stood
  // through a load's latency per pixel, and that was most of the kernel's time)
  for (int i0 = tid >> 6; i0 < TH * kCnxTW; i0 += 16) {
    float* row[4];
    float4 v[4][8];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + 4 * u, y = y0 + i / kCnxTW, xx = x0 + i % kCnxTW;
      row[u] = y < h && xx < w ? out + (base + (size_t)y * w + xx) * C : nullptr;
      if (row[u]) cnx_row_load(row[u], C, lane, v[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (row[u]) cnx_row_norm_store(v[u], g, b, row[u], C, lane);
  }
}

// ---- Global Response Normalization ------------------------------------------------------------------------------------------------------------
// hid rows [N][hw][K]; part[(n nchunks + chunk) K + k] = sum of hid^2 over the chunk's pixels: four running sums (pixel mod 4), joined as
// (a0 + a1) + (a2 + a3).  grid (ceil(K/256), nchunks = ceil(hw/256), N), 256 threads.
__global__ __launch_bounds__(256) void cnx_sumsq_kernel(const float* __restrict__ hid, float* __restrict__ part, int K, int hw) {
  const int k = (int)blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  const int p0 = (int)blockIdx.y * kCnxGrnChunk, p1 = p0 + kCnxGrnChunk < hw ? p0 + kCnxGrnChunk : hw;
  const float* src = hid + ((size_t)blockIdx.z * hw + p0) * K + k;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  int p = p0;
  for (; p + 4 <= p1; p += 4, src += (size_t)4 * K) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float v = src[(size_t)e * K];
      a[e] = fmaf(v, v, a[e]);
    }
  }
  for (int e = 0; p < p1; ++p, ++e, src += K) a[e] = fmaf(src[0], src[0], a[e]);
  part[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * K + k] = (a[0] + a[1]) + (a[2] + a[3]);
}

// s[n][k] = Gx = sqrt(the chunk sums in chunk order).  grid (ceil(K/256), N), 256 threads.
__global__ __launch_bounds__(256) void cnx_grn_gx_kernel(const float* __restrict__ part, float* __restrict__ s, int K, int nchunks) {
  const int k = (int)blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  const size_t n = blockIdx.y;
  float t = 0.f;
#pragma unroll 8
  for (int ch = 0; ch < nchunks; ++ch) t += part[(n * nchunks + ch) * K + k];
  s[n * K + k] = sqrtf(t);
}

// s[n][k] = 1 + gamma[k] Gx / (mean_k Gx + 1e-6), in place.  grid N, 256 threads.
__global__ __launch_bounds__(256) void cnx_grn_scale_kernel(const float* __restrict__ gamma, float* s, int K) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
  const size_t n = blockIdx.x;
  float loc = 0.f;
  for (int k = tid; k < K; k += 256) loc += s[n * K + k];
  red[tid] = loc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  const float den = red[0] / (float)K + 1e-6f;
  for (int k = tid; k < K; k += 256) s[n * K + k] = 1.f + gamma[k] * (s[n * K + k] / den);      // (the thread's own Gx)
}

// out[o][k] = w[o][k] s[k], four k per thread.  grid ceil(n4 / 256), n4 = C K / 4
__global__ __launch_bounds__(256) void cnx_scale_w_kernel(const float* __restrict__ w, const float* __restrict__ s, float* __restrict__ out, int K, size_t n4) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 a = reinterpret_cast<const float4*>(w)[i], f = *reinterpret_cast<const float4*>(s + (i * 4) % K);
  reinterpret_cast<float4*>(out)[i] = float4{a.x * f.x, a.y * f.y, a.z * f.z, a.w * f.w};
}

}  // namespace axvs
