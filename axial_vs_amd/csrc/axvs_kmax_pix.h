// Kernels of Video-kMaX's pixel decoder (kMaXPixelDecoder in eval mode: axial-attention and bottleneck blocks from stride 32 down to
// stride 4, joined by resized fuses): everything that is not a 1x1 convolution.  The 1x1 convolutions, with their BatchNorms folded in at
// pack time, run on the three-piece split-precision GEMM (axvs_gemm_nt.h); every contraction here is an f32-input MFMA
// (v_mfma_f32_16x16x4_f32) with fp32 accumulation.  Maps travel channels-last, rows in the order (frame, y, x).
//
//   kpix_innorm_kernel      [N, C, h, w] -> rows [N*h*w][C] through the channels-first LayerNorm (two passes over a pixel's channels, eps
//                           1e-6), optionally through gelu
//   kpix_gelu_kernel        y = gelu(x), four floats per thread
//   kpix_axial_attn_kernel  one axis pass of AxialAttention: a workgroup owns up to 64 queries of one (sequence, head); content, query-
//                           position and key-position similarities as MFMA tiles, the position terms read back along the skew
//                           (they are Toeplitz in (l, m)); softmax in LDS; retrieved content and retrieved positions as MFMA tiles, the
//                           latter with the skewed weights as the A operand.  The [N, 24, L, L] similarities and the [L, L, d] tables
//                           never exist
//   kpix_conv3_kernel       3 x 3, stride 1, zero padding 1, folded BN, gelu: implicit GEMM over a halo tile in LDS
//   kpix_resize_add_kernel  out = high + bilinear(low), either align_corners value (axvs_resize.h's coordinate rule)
// [N, C, h, w] <-> rows [N*h*w][C] without a norm: nchw_to_rows() / rows_to_nchw() (axvs_layout.h).
// No kernel waits for another workgroup and none adds floating-point numbers atomically: equal inputs give equal bits, and a frame's
// bits do not depend on the frames stacked beside it.
#pragma once
#include <hip/hip_runtime.h>

#include "axvs_common.h"
#include "axvs_layout.h"
#include "axvs_resize.h"

namespace axvs {

constexpr int kKpixHeads = 8;
constexpr int kKpixSpan = 255;                   // MAX_SPAN: the position tables have 2 * 255 - 1 rows, row r + 254 for the offset r = m - l
constexpr int kKpixTable = 2 * kKpixSpan - 1;
constexpr int kKpixQB = 64;                      // queries per workgroup of the attention kernel, at most (four waves x 16)
constexpr int kKpixSkew = 33;                    // row stride of a wave's 16 x 32 position-term tile
constexpr int kKpixMaxLds = 160 * 1024;

// ---- the channels-first LayerNorm: 32 pixels of one frame per workgroup ------------------------------------------------------------------------
// grid (ceil(h*w/32), N), 256 threads: thread (pixel tid & 31, channel group tid >> 5).
template <bool GELU>
__global__ __launch_bounds__(256) void kpix_innorm_kernel(const float* __restrict__ src, const float* __restrict__ g, const float* __restrict__ b,
                                                          float* __restrict__ out, int C, int hw) {
  __shared__ float red[8][33];
  __shared__ float tile[32][65];
  const int tid = threadIdx.x, tx = tid & 31, cy = tid >> 5;
  const int p0 = (int)blockIdx.x * 32, p = p0 + tx;
  const size_t n = blockIdx.y;
  const bool in = p < hw;
  const float* const S = src + n * C * (size_t)hw + (in ? p : hw - 1);
  float s = 0.f;
  for (int c = cy; c < C; c += 8) s += S[(size_t)c * hw];
  red[cy][tx] = s;
  __syncthreads();
  float mean = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) mean += red[j][tx];
  mean /= (float)C;
  __syncthreads();
  s = 0.f;
  for (int c = cy; c < C; c += 8) {
    const float d = S[(size_t)c * hw] - mean;
    s = fmaf(d, d, s);
  }
  red[cy][tx] = s;
  __syncthreads();
  float var = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) var += red[j][tx];
  const float den = sqrtf(var / (float)C + 1e-6f);
  const int oc = tid & 63, orow = tid >> 6;
  for (int c0 = 0; c0 < C; c0 += 64) {
    __syncthreads();            // the previous chunk has been written out
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + cy + 8 * j;
      if (c < C) {
        const float v = g[c] * ((S[(size_t)c * hw] - mean) / den) + b[c];
        tile[tx][cy + 8 * j] = GELU ? gelu_exact(v) : v;
      }
    }
    __syncthreads();
    if (c0 + oc < C) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int q = p0 + orow + 4 * j;
        if (q < hw) out[(n * hw + q) * C + c0 + oc] = tile[orow + 4 * j][oc];
      }
    }
  }
}

__global__ __launch_bounds__(256) void kpix_gelu_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n4) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 v = reinterpret_cast<const float4*>(x)[i];
  reinterpret_cast<float4*>(y)[i] = float4{gelu_exact(v.x), gelu_exact(v.y), gelu_exact(v.z), gelu_exact(v.w)};
}

// ---- one axis pass of the axial attention ---------------------------------------------------------------------------------------------------
// Sequences are addressed by strides (in rows): sequence s starts at row (s / seq_inner) * seq_outer + (s % seq_inner) * seq_step, its
// element l is lstride rows further.  Columns of a frame: seq_inner = w, seq_outer = h*w, seq_step = 1, lstride = w; rows of a frame:
// seq_inner = 1, seq_outer = w, lstride = 1.
struct KpixSeq {
  long long seq_inner, seq_outer, seq_step, lstride;
};

struct KpixAttnLds {       // in floats
  int L16, qb, nw, lds_s, s, skew, u, q, k, eq, ek, v, ev, total;
};

// The LDS plan of one (L, dk, dv): the scores S [qb][L16 + 4], the waves' skew tiles, and one region that holds q, k and the two
// similarity windows while the scores are formed, then v and the value window.  A window has L16 + qb rows: offsets r = m - l of the
// workgroup's queries l in [Q0, Q0 + qb) against keys m in [0, L16), row j <-> r = j - Q0 - qb + 1.
__host__ __device__ inline KpixAttnLds kpix_attn_lds(int L, int dk, int dv) {
  KpixAttnLds p;
  p.L16 = (L + 15) / 16 * 16;
  p.qb = p.L16 < kKpixQB ? p.L16 : kKpixQB;
  p.nw = p.L16 + p.qb;
  p.lds_s = p.L16 + 4;
  p.s = 0;
  p.skew = p.s + p.qb * p.lds_s;
  p.u = p.skew + 4 * 2 * 16 * kKpixSkew;
  const int ldk = dk + 4, ldv = dv + 4;
  p.q = p.u, p.k = p.q + p.qb * ldk, p.eq = p.k + p.L16 * ldk, p.ek = p.eq + p.nw * ldk;
  const int enda = p.ek + p.nw * ldk;
  p.v = p.u, p.ev = p.v + p.L16 * ldv;
  const int endb = p.ev + p.nw * ldv;
  p.total = enda > endb ? enda : endb;
  return p;
}

// qkv rows [.][cq]: q at h*DK, k at 8*DK + h*DK, v at 16*DK + h*DV (the reference's split of the channels, heads outermost).
// eq, ek [509][DK], ev [509][DV]; sim_a [24]: the gains of the similarity BatchNorm, channel part*8 + h (its offsets are constant in m:
// they cancel in the softmax); out_ab [3][8*DV]: the gains of the retrieved content and the retrieved positions, and the sum of
// their offsets.  out rows [.][8*DV], optionally through gelu.
// grid (ceil(L16 / qb), 8, sequences), 256 threads, dynamic LDS kpix_attn_lds(L, DK, DV).total floats.
template <int DK, int DV>
__global__ __launch_bounds__(256) void kpix_axial_attn_kernel(const float* __restrict__ qkv, KpixSeq sq, int L, const float* __restrict__ eq_t,
                                                              const float* __restrict__ ek_t, const float* __restrict__ ev_t,
                                                              const float* __restrict__ sim_a, const float* __restrict__ out_ab, float* __restrict__ out,
                                                              int gelu) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int LDK = DK + 4, LDV = DV + 4, CQ = kKpixHeads * (2 * DK + DV), CO = kKpixHeads * DV, ND = DV / 16;
  const KpixAttnLds P = kpix_attn_lds(L, DK, DV);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fi = lane & 15, fg = lane >> 4;
  const int Q0 = (int)blockIdx.x * P.qb, h = blockIdx.y;
  const long long s = blockIdx.z;
  const long long row0 = (s / sq.seq_inner) * sq.seq_outer + (s % sq.seq_inner) * sq.seq_step;
  const int rmin = -Q0 - P.qb + 1;                 // the offset of window row 0
  const bool active = 16 * wave < P.qb && Q0 + 16 * wave < L;
  float* const S = smem + P.s;
  float* const sk = smem + P.skew + wave * (2 * 16 * kKpixSkew);
  const float4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // ---- q, k and the two similarity windows -> LDS (rows past L: zeros)
  {
    float* const qs = smem + P.q;
    float* const ks = smem + P.k;
    float* const eqs = smem + P.eq;
    float* const eks = smem + P.ek;
    constexpr int D4 = DK / 4;
    for (int i = tid; i < P.qb * D4; i += 256) {
      const int r = i / D4, c4 = i % D4, l = Q0 + r;
      float4 v = zero4;
      if (l < L) v = *reinterpret_cast<const float4*>(qkv + (row0 + l * sq.lstride) * CQ + h * DK + 4 * c4);
      *reinterpret_cast<float4*>(qs + r * LDK + 4 * c4) = v;
    }
    for (int i = tid; i < P.L16 * D4; i += 256) {
      const int r = i / D4, c4 = i % D4;
      float4 v = zero4;
      if (r < L) v = *reinterpret_cast<const float4*>(qkv + (row0 + r * sq.lstride) * CQ + kKpixHeads * DK + h * DK + 4 * c4);
      *reinterpret_cast<float4*>(ks + r * LDK + 4 * c4) = v;
    }
    for (int i = tid; i < P.nw * D4; i += 256) {
      const int r = i / D4, c4 = i % D4, t = r + rmin + kKpixSpan - 1;
      float4 a = zero4, b = zero4;
      if (t >= 0 && t < kKpixTable) {
        a = *reinterpret_cast<const float4*>(eq_t + t * DK + 4 * c4);
        b = *reinterpret_cast<const float4*>(ek_t + t * DK + 4 * c4);
      }
      *reinterpret_cast<float4*>(eqs + r * LDK + 4 * c4) = a;
      *reinterpret_cast<float4*>(eks + r * LDK + 4 * c4) = b;
    }
  }
  __syncthreads();

  // ---- the scores, one 16 x 16 tile of (queries of this wave, keys m0..) at a time
  {
    const float* const qs = smem + P.q + (16 * wave + fi) * LDK + 4 * fg;
    const float* const ks = smem + P.k + fi * LDK + 4 * fg;
    const float* const eqs = smem + P.eq + fi * LDK + 4 * fg;
    const float* const eks = smem + P.ek + fi * LDK + 4 * fg;
    const float a0 = sim_a[h], a1 = sim_a[8 + h], a2 = sim_a[16 + h];
    for (int m0 = 0; m0 < P.L16; m0 += 16) {
      f32x4 cc = {0.f, 0.f, 0.f, 0.f}, pq0 = cc, pq1 = cc, pk0 = cc, pk1 = cc;
      if (active) {
        const int jb = m0 - 16 * wave + P.qb - 16;       // window row of the tile's lowest offset (l = its last query, m = m0)
#pragma unroll
        for (int c4 = 0; c4 < DK / 16; ++c4) {
          const float4 q4 = *reinterpret_cast<const float4*>(qs + 16 * c4);
          const float4 k4 = *reinterpret_cast<const float4*>(ks + m0 * LDK + 16 * c4);
          const float4 e0 = *reinterpret_cast<const float4*>(eqs + jb * LDK + 16 * c4);
          const float4 e1 = *reinterpret_cast<const float4*>(eqs + (jb + 16) * LDK + 16 * c4);
          const float4 g0 = *reinterpret_cast<const float4*>(eks + jb * LDK + 16 * c4);
          const float4 g1 = *reinterpret_cast<const float4*>(eks + (jb + 16) * LDK + 16 * c4);
          const float qa[4] = {q4.x, q4.y, q4.z, q4.w}, ka[4] = {k4.x, k4.y, k4.z, k4.w};
          const float e0a[4] = {e0.x, e0.y, e0.z, e0.w}, e1a[4] = {e1.x, e1.y, e1.z, e1.w};
          const float g0a[4] = {g0.x, g0.y, g0.z, g0.w}, g1a[4] = {g1.x, g1.y, g1.z, g1.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            cc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[e], ka[e], cc, 0, 0, 0);         // [query][key]
            pq0 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[e], e0a[e], pq0, 0, 0, 0);      // [query][offset jb + 0..15]
            pq1 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[e], e1a[e], pq1, 0, 0, 0);      // [query][offset jb + 16..31]
            pk0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[e], g0a[e], pk0, 0, 0, 0);      // [key][offset]
            pk1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[e], g1a[e], pk1, 0, 0, 0);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          sk[(4 * fg + r) * kKpixSkew + fi] = pq0[r];
          sk[(4 * fg + r) * kKpixSkew + 16 + fi] = pq1[r];
          sk[(16 + 4 * fg + r) * kKpixSkew + fi] = pk0[r];
          sk[(16 + 4 * fg + r) * kKpixSkew + 16 + fi] = pk1[r];
        }
      }
      __syncthreads();
      if (active) {
        // query i = 4 fg + r, key c = fi: the offset m - l sits at column c - i + 15 of both tiles
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 4 * fg + r, col = fi - i + 15;
          const float v = a0 * cc[r] + a1 * sk[i * kKpixSkew + col] + a2 * sk[(16 + fi) * kKpixSkew + col];
          S[(16 * wave + i) * P.lds_s + m0 + fi] = v;
        }
      }
      __syncthreads();
    }
  }

  // ---- softmax over the keys m < L of the wave's own rows; the pad columns become zero weights
  if (active) {
    for (int r = 0; r < 16; ++r) {
      float* const row = S + (16 * wave + r) * P.lds_s;
      const float x0 = lane < L ? row[lane] : -INFINITY, x1 = lane + 64 < L ? row[lane + 64] : -INFINITY;
      float mx = fmaxf(x0, x1);
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, kWave));
      const float e0 = lane < L ? expf(x0 - mx) : 0.f, e1 = lane + 64 < L ? expf(x1 - mx) : 0.f;
      float sum = e0 + e1;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) sum += __shfl_xor(sum, o, kWave);
      if (lane < P.L16) row[lane] = e0 / sum;
      if (lane + 64 < P.L16) row[lane + 64] = e1 / sum;
    }
  }
  __syncthreads();

  // ---- v and the value window -> LDS, over q / k / the similarity windows
  {
    float* const vs = smem + P.v;
    float* const evs = smem + P.ev;
    constexpr int D4 = DV / 4;
    for (int i = tid; i < P.L16 * D4; i += 256) {
      const int r = i / D4, c4 = i % D4;
      float4 v = zero4;
      if (r < L) v = *reinterpret_cast<const float4*>(qkv + (row0 + r * sq.lstride) * CQ + 2 * kKpixHeads * DK + h * DV + 4 * c4);
      *reinterpret_cast<float4*>(vs + r * LDV + 4 * c4) = v;
    }
    for (int i = tid; i < P.nw * D4; i += 256) {
      const int r = i / D4, c4 = i % D4, t = r + rmin + kKpixSpan - 1;
      float4 a = zero4;
      if (t >= 0 && t < kKpixTable) a = *reinterpret_cast<const float4*>(ev_t + t * DV + 4 * c4);
      *reinterpret_cast<float4*>(evs + r * LDV + 4 * c4) = a;
    }
  }
  __syncthreads();
  if (!active) return;

  // ---- retrieved content W v and retrieved positions: sum_m W[l][m] Ev[m - l] = (W read along the skew) x (the window)
  f32x4 oc[ND], orp[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) oc[d] = f32x4{0.f, 0.f, 0.f, 0.f}, orp[d] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* const wrow = S + (16 * wave + fi) * P.lds_s;
  {
    const float* const vs = smem + P.v + fi;
    for (int m0 = 0; m0 < P.L16; m0 += 16) {
      const float4 w4 = *reinterpret_cast<const float4*>(wrow + m0 + 4 * fg);
      const float wa[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float* const vr = vs + (m0 + 4 * fg + e) * LDV;
#pragma unroll
        for (int d = 0; d < ND; ++d) oc[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[e], vr[16 * d], oc[d], 0, 0, 0);
      }
    }
  }
  {
    // window rows jlo + jj, jj in [0, L16 + 16): query i reads key m = jj - 15 + i there
    const int jlo = P.qb - 16 - 16 * wave;
    const float* const evs = smem + P.ev + jlo * LDV + fi;
    for (int j0 = 0; j0 < P.L16 + 16; j0 += 16) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int jj = j0 + 4 * fg + e, m = jj - 15 + fi;
        const float wv = (m >= 0 && m < P.L16) ? wrow[m] : 0.f;
        const float* const er = evs + jj * LDV;
#pragma unroll
        for (int d = 0; d < ND; ++d) orp[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv, er[16 * d], orp[d], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int l = Q0 + 16 * wave + 4 * fg + r;
    if (l >= L) continue;
    float* const o = out + (row0 + l * sq.lstride) * CO + h * DV + fi;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      const int ch = h * DV + 16 * d + fi;
      const float v = out_ab[ch] * oc[d][r] + out_ab[CO + ch] * orp[d][r] + out_ab[2 * CO + ch];
      o[16 * d] = gelu ? gelu_exact(v) : v;
    }
  }
}

// ---- 3 x 3 convolution, stride 1, zero padding 1, folded BN, gelu -----------------------------------------------------------------------------
// in rows [N][h][w][C], wt [9][C (out)][C (in)] (tap-major), out rows [N][h][w][C].  A workgroup: 4 rows x 16 columns of outputs, the
// 6 x 18 halo tile with all C channels in LDS (row stride C + 4); wave = one output row; 32 output channels at a time, the weights
// straight from global memory (L2-resident: 9 C^2 floats).  C a multiple of 32, at most 256.
// grid (ceil(w/16), ceil(h/4), N), 256 threads, dynamic LDS 108 * (C + 4) floats.
__global__ __launch_bounds__(256) void kpix_conv3_kernel(const float* __restrict__ in, const float* __restrict__ wt, const float* __restrict__ bias,
                                                         float* __restrict__ out, int C, int h, int w) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int LD = C + 4, C4 = C / 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fi = lane & 15, fg = lane >> 4;
  const int x0 = (int)blockIdx.x * 16, y0 = (int)blockIdx.y * 4;
  const size_t base = (size_t)blockIdx.z * h * w;
  for (int i = tid; i < 108 * C4; i += 256) {
    const int pi = i / C4, c4 = i % C4, ty = pi / 18, tx = pi % 18;
    const int y = y0 + ty - 1, x = x0 + tx - 1;
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (y >= 0 && y < h && x >= 0 && x < w) v = *reinterpret_cast<const float4*>(in + (base + (size_t)y * w + x) * C + 4 * c4);
    *reinterpret_cast<float4*>(smem + pi * LD + 4 * c4) = v;
  }
  __syncthreads();
  const int y = y0 + wave;
  if (y >= h) return;
  for (int n0 = 0; n0 < C; n0 += 32) {
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int tap = 0; tap < 9; ++tap) {
      const float* const a = smem + ((wave + tap / 3) * 18 + fi + tap % 3) * LD + 4 * fg;
      const float* const b = wt + ((size_t)tap * C + n0 + fi) * C + 4 * fg;
      for (int c = 0; c < C; c += 16) {
        const float4 a4 = *reinterpret_cast<const float4*>(a + c);
        const float4 b0 = *reinterpret_cast<const float4*>(b + c);
        const float4 b1 = *reinterpret_cast<const float4*>(b + (size_t)16 * C + c);
        const float aa[4] = {a4.x, a4.y, a4.z, a4.w}, b0a[4] = {b0.x, b0.y, b0.z, b0.w}, b1a[4] = {b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(aa[e], b0a[e], acc[0], 0, 0, 0);       // [pixel][output channel]
          acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(aa[e], b1a[e], acc[1], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int x = x0 + 4 * fg + r;
      if (x >= w) continue;
      float* const o = out + (base + (size_t)y * w + x) * C + n0 + fi;
      o[0] = gelu_exact(acc[0][r] + bias[n0 + fi]);
      o[16] = gelu_exact(acc[1][r] + bias[n0 + 16 + fi]);
    }
  }
}

// ---- out = high + bilinear(low): rows [N][H][W][C] and [N][h][w][C], four channels per thread ------------------------------------------------------
// upsample_bilinear2d's expression: h0 (w0 a + w1 b) + h1 (w0 c + w1 d).  out may be high.  grid ceil(N*H*W*C/4 / 256).
__global__ __launch_bounds__(256) void kpix_resize_add_kernel(const float* __restrict__ low, const float* high, float* out, int N, int C, PanAxis ay,
                                                              PanAxis ax, int ac) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int C4 = C / 4;
  if (i >= (size_t)N * ay.out * ax.out * C4) return;
  const int c4 = (int)(i % C4);
  const size_t p = i / C4;
  const int x = (int)(p % ax.out), y = (int)(p / ax.out % ay.out);
  const size_t n = p / ax.out / ay.out;
  const PanTap ty = pan_tap(y, ay, ac), tx = pan_tap(x, ax, ac);
  const float* const L0 = low + (n * ay.in * ax.in) * C + 4 * c4;
  const float4 a = *reinterpret_cast<const float4*>(L0 + ((size_t)ty.i0 * ax.in + tx.i0) * C);
  const float4 b = *reinterpret_cast<const float4*>(L0 + ((size_t)ty.i0 * ax.in + tx.i1) * C);
  const float4 c = *reinterpret_cast<const float4*>(L0 + ((size_t)ty.i1 * ax.in + tx.i0) * C);
  const float4 d = *reinterpret_cast<const float4*>(L0 + ((size_t)ty.i1 * ax.in + tx.i1) * C);
  const float4 hv = reinterpret_cast<const float4*>(high)[i];
  auto f = [&](float a_, float b_, float c_, float d_, float h_) {
    return (ty.l0 * (tx.l0 * a_ + tx.l1 * b_) + ty.l1 * (tx.l0 * c_ + tx.l1 * d_)) + h_;
  };
  reinterpret_cast<float4*>(out)[i] = float4{f(a.x, b.x, c.x, d.x, hv.x), f(a.y, b.y, c.y, d.y, hv.y), f(a.z, b.z, c.z, d.z, hv.z),
                                             f(a.w, b.w, c.w, d.w, hv.w)};
}

}  // namespace axvs
