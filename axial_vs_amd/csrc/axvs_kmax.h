// Kernels of Video-kMaX's k-means query decoder (MaXTronTransformerDecoder in eval mode: six kMaXTransformerLayers and the final
// kMaXPredictor): everything that is not a 1x1 convolution.  The 1x1 convolutions, with their BatchNorms folded in at pack time, run on the
// three-piece split-precision GEMM (axvs_gemm_nt.h); the contractions here are f32-input MFMAs (v_mfma_f32_16x16x4_f32) or plain fp32
// FMAs: the cluster assignment is a hard decision.  Pixels travel channels-last, rows in the order (clip, frame, y, x): the reference's
// stacked `b c (t h) w` map.
//
//   (axvs_layout.h)         [(B T), C, h, w] -> rows [B*T*h*w][C], optionally through gelu (a layer's input activation, once per level):
//                           nchw_to_rows<GELU>(); the cluster centres' broadcast over the clips and the class logits: broadcast_rows(),
//                           class_logits_rows()
//   kmax_dw5_kernel         depthwise 5 x 5 (+ folded BN + gelu) over the stacked T*h x w map through an LDS halo tile: the window crosses
//                           frame boundaries, as the reference's does
//   kmax_assign_kernel      a tile of pixels: L2-normalise the 128-channel rows, contract with the [L,128] mask kernels (held in LDS in
//                           chunks of 64 clusters), apply the one-channel BatchNorm (a z + b), and keep a running (max, index) per pixel
//                           -> one int32 per pixel; the [B, L, T*h*w] logits never exist.  OUT = true (the final predictor): the logits and
//                           the normalised rows go out instead, channels-first
//   kmax_sum_kernel         cluster sums as a one-hot contraction over a fixed chunk of a clip's pixels (exact one-hot f32 MFMA operand),
//                           plus integer pixel counts per cluster; kmax_sum_reduce_kernel adds the chunk slabs in chunk order
//   kmax_attn_kernel        the query self-attention of one (clip, head): similarity without 1/sqrt(d), per-head affine, softmax, retrieved
//                           values through their BatchNorm and gelu
// No kernel waits for another workgroup and none adds floating-point numbers atomically: equal inputs give equal bits, and a clip's bits
// do not depend on the clips stacked beside it.
#pragma once
#include <hip/hip_runtime.h>

#include "axvs_common.h"
#include "axvs_layout.h"

namespace axvs {

constexpr int kKmaxC = 256;           // query channels, bottleneck channels, value depth
constexpr int kKmaxD = 128;           // mask-kernel channels (base_filters)
constexpr int kKmaxHeads = 8;         // key depth 16, value depth 32 per head
constexpr int kKmaxLChunk = 64;       // clusters per LDS chunk of the mask kernels / per workgroup of the cluster sums
constexpr int kKmaxLLd = kKmaxD + 4;  // LDS row stride of a mask kernel
constexpr int kKmaxSumMinChunk = 256; // pixels per cluster-sum chunk, at least
constexpr int kKmaxSumMaxChunks = 64; // chunks per clip, at most: the slabs do not grow with the map
constexpr int kKmaxAug = kKmaxC + 4;  // a cluster-sum row: 256 sums, the pixel count, three zeros

// ---- depthwise 5 x 5, padding 2, over the stacked map [B][TH][w][256]: out = gelu(sum_k wt[k][c] in[y + ky - 2][x + kx - 2][c] + bias[c]) -----
// A workgroup: 4 rows x 8 columns of outputs x 64 channels; the 8 x 12 halo tile in LDS (zeros outside the stacked map -- and only
// there: rows of the neighbouring frame are inside it).  grid (ceil(w/8) * 4, ceil(TH/4), B), 256 threads.
__global__ __launch_bounds__(256) void kmax_dw5_kernel(const float* __restrict__ in, const float* __restrict__ wt, const float* __restrict__ bias,
                                                       float* __restrict__ out, int TH, int w) {
  __shared__ float tile[8][12][64];
  const int tid = threadIdx.x, c = tid & 63, g = tid >> 6;
  const int x0 = (int)(blockIdx.x >> 2) * 8, c0 = (int)(blockIdx.x & 3) * 64, y0 = (int)blockIdx.y * 4;
  const size_t base = (size_t)blockIdx.z * TH * w;
#pragma unroll
  for (int j = 0; j < 24; ++j) {
    const int pi = g + 4 * j, ty = pi / 12, tx = pi % 12;
    const int y = y0 + ty - 2, x = x0 + tx - 2;
    float v = 0.f;
    if (y >= 0 && y < TH && x >= 0 && x < w) v = in[(base + (size_t)y * w + x) * kKmaxC + c0 + c];
    tile[ty][tx][c] = v;
  }
  float wk[25];
#pragma unroll
  for (int k = 0; k < 25; ++k) wk[k] = wt[k * kKmaxC + c0 + c];
  __syncthreads();
  const int y = y0 + g;
  if (y >= TH) return;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ky = 0; ky < 5; ++ky) {
#pragma unroll
    for (int xx = 0; xx < 12; ++xx) {
      const float v = tile[g + ky][xx][c];
#pragma unroll
      for (int kx = 0; kx < 5; ++kx) {
        const int o = xx - kx;
        if (o >= 0 && o < 8) acc[o] = fmaf(wk[ky * 5 + kx], v, acc[o]);
      }
    }
  }
  const float bb = bias[c0 + c];
#pragma unroll
  for (int o = 0; o < 8; ++o)
    if (x0 + o < w) out[(base + (size_t)y * w + x0 + o) * kKmaxC + c0 + c] = gelu_exact(acc[o] + bb);
}

// ---- normalise, contract with the mask kernels, affine, argmax ----------------------------------------------------------------------------
// One wave: 32 pixels (two 16-pixel MFMA tiles, their 128 channels in registers) against every cluster, 16 at a time:
//   D[cluster 4 g + r][pixel i] = sum_c mk[cluster][c] f[pixel][c]; lane group g holds channels 16 c4 + 4 g + e of both operands.
// pf [B][S][128] (not yet normalised), mk [B][L][128], ab = (a, b) of the one-channel BatchNorm.
// OUT = false: idx[b*S + p] = argmax_l (a z + b), equal maxima to the lower index (a may be negative or zero: the affine comes first).
// OUT = true:  masks[(b*L + l)*S + p] = a z + b and feat[(b*128 + c)*S + p] = the normalised row (either may be null).
// grid (ceil(S/128), B), 256 threads.
template <bool OUT>
__global__ __launch_bounds__(256) void kmax_assign_kernel(const float* __restrict__ pf, const float* __restrict__ mk, const float* __restrict__ ab, int L,
                                                          int S, int* __restrict__ idx, float* __restrict__ masks, float* __restrict__ feat) {
  __shared__ __attribute__((aligned(16))) float smk[kKmaxLChunk * kKmaxLLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fi = lane & 15, fg = lane >> 4;
  const int b = blockIdx.y;
  const int key0 = ((int)blockIdx.x * 4 + wave) * 32;
  const float* const F = pf + (size_t)b * S * kKmaxD;
  const float* const A = mk + (size_t)b * L * kKmaxD;
  const float ga = ab[0], gb = ab[1];
  float f[2][8][4];
  bool valid[2];
#pragma unroll
  for (int tl = 0; tl < 2; ++tl) {
    const int key = key0 + 16 * tl + fi;
    valid[tl] = key < S;
    const int kc = valid[tl] ? key : S - 1;
    float ss = 0.f;
#pragma unroll
    for (int c4 = 0; c4 < 8; ++c4) {
      const float4 v = *reinterpret_cast<const float4*>(F + (size_t)kc * kKmaxD + 16 * c4 + 4 * fg);
      f[tl][c4][0] = v.x, f[tl][c4][1] = v.y, f[tl][c4][2] = v.z, f[tl][c4][3] = v.w;
      ss = fmaf(v.x, v.x, ss), ss = fmaf(v.y, v.y, ss), ss = fmaf(v.z, v.z, ss), ss = fmaf(v.w, v.w, ss);
    }
    ss = wave_xor_sum(ss, 16);
    ss = wave_xor_sum(ss, 32);
    const float den = fmaxf(sqrtf(ss), 1e-12f);        // F.normalize: x / max(|x|, eps)
#pragma unroll
    for (int c4 = 0; c4 < 8; ++c4)
#pragma unroll
      for (int e = 0; e < 4; ++e) f[tl][c4][e] = f[tl][c4][e] / den;
    if constexpr (OUT) {
      if (feat && valid[tl]) {
#pragma unroll
        for (int c4 = 0; c4 < 8; ++c4)
#pragma unroll
          for (int e = 0; e < 4; ++e) feat[((size_t)b * kKmaxD + 16 * c4 + 4 * fg + e) * S + key] = f[tl][c4][e];
      }
    }
  }
  if constexpr (OUT) {
    if (!masks) return;         // (uniform: before the first barrier)
  }
  float bv[2] = {-INFINITY, -INFINITY};
  int bi[2] = {0, 0};
  for (int l0 = 0; l0 < L; l0 += kKmaxLChunk) {
    __syncthreads();            // the previous chunk has been read
#pragma unroll
    for (int j = 0; j < kKmaxLChunk * (kKmaxD / 4) / 256; ++j) {
      const int q = tid + 256 * j, row = q >> 5, c4 = q & 31;
      const int l = min(l0 + row, L - 1);
      *reinterpret_cast<float4*>(smk + row * kKmaxLLd + 4 * c4) = *reinterpret_cast<const float4*>(A + (size_t)l * kKmaxD + 4 * c4);
    }
    __syncthreads();
    const int ntile = min(kKmaxLChunk / 16, (L - l0 + 15) / 16);
    for (int qt = 0; qt < ntile; ++qt) {
      f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int c4 = 0; c4 < 8; ++c4) {
        const float4 a4 = *reinterpret_cast<const float4*>(smk + (qt * 16 + fi) * kKmaxLLd + 16 * c4 + 4 * fg);
        const float a[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], f[0][c4][e], acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], f[1][c4][e], acc[1], 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int l = l0 + qt * 16 + 4 * fg + r;
        if (l >= L) continue;
#pragma unroll
        for (int tl = 0; tl < 2; ++tl) {
          const float z = fmaf(ga, acc[tl][r], gb);
          if constexpr (OUT) {
            if (valid[tl]) masks[((size_t)b * L + l) * S + key0 + 16 * tl + fi] = z;
          } else {
            if (z > bv[tl]) bv[tl] = z, bi[tl] = l;     // a lane meets its clusters in rising order: strict > keeps the lowest
          }
        }
      }
    }
  }
  if constexpr (!OUT) {
#pragma unroll
    for (int tl = 0; tl < 2; ++tl) {
#pragma unroll
      for (int o = 16; o <= 32; o <<= 1) {
        const float ov = __shfl_xor(bv[tl], o, kWave);
        const int oi = __shfl_xor(bi[tl], o, kWave);
        if (ov > bv[tl] || (ov == bv[tl] && oi < bi[tl])) bv[tl] = ov, bi[tl] = oi;
      }
      if (fg == 0 && valid[tl]) idx[(size_t)b * S + key0 + 16 * tl + fi] = bi[tl];
    }
  }
}

// ---- cluster sums ---------------------------------------------------------------------------------------------------------------------------
// part[((b*nchunk + ch)*L + l)*256 + c] = sum over the pixels p of chunk ch of clip b with idx[p] == l of ps[p][c], as the contraction of the
// exact one-hot matrix with the value rows: D[l][c] += onehot[l][p] ps[p][c], four pixels per MFMA.  pcnt[(b*nchunk + ch)*L + l]: how many.
// A workgroup: 64 clusters x 256 channels (wave w: channels 64 w ..), the chunk's pixels in order.  An index outside 0..L-1 matches no
// cluster.  grid (nchunk, ceil(L/64), B), 256 threads.
__global__ __launch_bounds__(256) void kmax_sum_kernel(const float* __restrict__ ps, const int* __restrict__ idx, int L, int S, int chunk, int nchunk,
                                                       float* __restrict__ part, int* __restrict__ pcnt) {
  __shared__ int cnt[kKmaxLChunk];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fi = lane & 15, fg = lane >> 4;
  const int ch = blockIdx.x, l0 = (int)blockIdx.y * kKmaxLChunk, b = blockIdx.z;
  const int p0 = ch * chunk, p1 = min(S, p0 + chunk);
  const int* const I = idx + (size_t)b * S;
  const float* const P = ps + (size_t)b * S * kKmaxC + 64 * wave + fi;
  if (tid < kKmaxLChunk) cnt[tid] = 0;
  __syncthreads();
  for (int p = p0 + tid; p < p1; p += 256) {
    const int i = I[p] - l0;
    if (i >= 0 && i < kKmaxLChunk) atomicAdd(&cnt[i], 1);       // integers: any order gives the same count
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int lt = 0; lt < 4; ++lt)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[lt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int p = p0; p < p1; p += 4) {
    const bool in = p + fg < p1;
    const int pc = in ? p + fg : p1 - 1;
    const int li = in ? I[pc] - l0 : -1;
    float v[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const float t = P[(size_t)pc * kKmaxC + 16 * ct];
      v[ct] = in ? t : 0.f;
    }
#pragma unroll
    for (int lt = 0; lt < 4; ++lt) {
      const float oh = li == 16 * lt + fi ? 1.f : 0.f;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[lt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(oh, v[ct], acc[lt][ct], 0, 0, 0);
    }
  }
  float* const O = part + ((size_t)b * nchunk + ch) * L * kKmaxC + 64 * wave + fi;
#pragma unroll
  for (int lt = 0; lt < 4; ++lt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int l = l0 + 16 * lt + 4 * fg + r;
      if (l >= L) continue;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) O[(size_t)l * kKmaxC + 16 * ct] = acc[lt][ct][r];
    }
  __syncthreads();
  if (tid < kKmaxLChunk && l0 + tid < L) pcnt[((size_t)b * nchunk + ch) * L + l0 + tid] = cnt[tid];
}

// saug[(b*L + l)][c] = sum_ch part, the chunks in order; column 256 = the pixel count (an exact integer below 2^24), 257..259 = 0.
// grid B*L, 256 threads.
__global__ __launch_bounds__(256) void kmax_sum_reduce_kernel(const float* __restrict__ part, const int* __restrict__ pcnt, float* __restrict__ saug, int L,
                                                              int nchunk) {
  const int row = blockIdx.x, b = row / L, l = row % L, c = threadIdx.x;
  float s = 0.f;
  for (int ch = 0; ch < nchunk; ++ch) s += part[(((size_t)b * nchunk + ch) * L + l) * kKmaxC + c];
  saug[(size_t)row * kKmaxAug + c] = s;
  if (c < 4) {
    int n = 0;
    if (c == 0)
      for (int ch = 0; ch < nchunk; ++ch) n += pcnt[((size_t)b * nchunk + ch) * L + l];
    saug[(size_t)row * kKmaxAug + kKmaxC + c] = (float)n;
  }
}

// ---- query self-attention -------------------------------------------------------------------------------------------------------------------
// qkv rows [B*L][512]: q at 16 h, k at 128 + 16 h, v at 256 + 32 h.  Thread = query l of (head, clip): s[m] = sim_a[h] (q . k_m) + sim_b[h]
// (no 1/sqrt(d)), softmax over m, out = sum_m p[m] v_m, att[(b*L + l)*256 + 32 h + d] = gelu(rv_a out + rv_b).
// sim_ab: a[8] then b[8]; rv_ab: a[256] then b[256].  grid (8, B), 256 threads, L <= 256.
__global__ __launch_bounds__(256) void kmax_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ sim_ab, const float* __restrict__ rv_ab,
                                                        float* __restrict__ att, int L) {
  __shared__ float sk[256][16];
  __shared__ float sv[256][32];
  const int h = blockIdx.x, b = blockIdx.y, l = threadIdx.x;
  const float* const row = qkv + ((size_t)b * L + min(l, L - 1)) * 512;
  float q[16];
#pragma unroll
  for (int d = 0; d < 16; d += 4) {
    const float4 u = *reinterpret_cast<const float4*>(row + 16 * h + d);
    q[d] = u.x, q[d + 1] = u.y, q[d + 2] = u.z, q[d + 3] = u.w;
    if (l < L) *reinterpret_cast<float4*>(&sk[l][d]) = *reinterpret_cast<const float4*>(row + 128 + 16 * h + d);
  }
  if (l < L) {
#pragma unroll
    for (int d = 0; d < 32; d += 4) *reinterpret_cast<float4*>(&sv[l][d]) = *reinterpret_cast<const float4*>(row + 256 + 32 * h + d);
  }
  __syncthreads();
  if (l >= L) return;
  const float sa = sim_ab[h], sb = sim_ab[8 + h];
  auto score = [&](int m) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < 16; ++d) s = fmaf(q[d], sk[m][d], s);
    return fmaf(sa, s, sb);
  };
  float mx = -INFINITY;
  for (int m = 0; m < L; ++m) mx = fmaxf(mx, score(m));
  float o[32], den = 0.f;
#pragma unroll
  for (int d = 0; d < 32; ++d) o[d] = 0.f;
  for (int m = 0; m < L; ++m) {
    const float p = expf(score(m) - mx);
    den += p;
#pragma unroll
    for (int d = 0; d < 32; ++d) o[d] = fmaf(p, sv[m][d], o[d]);
  }
  float* const out = att + ((size_t)b * L + l) * kKmaxC + 32 * h;
#pragma unroll
  for (int d = 0; d < 32; ++d) out[d] = gelu_exact(fmaf(rv_ab[32 * h + d], o[d] / den, rv_ab[kKmaxC + 32 * h + d]));
}

}  // namespace axvs
