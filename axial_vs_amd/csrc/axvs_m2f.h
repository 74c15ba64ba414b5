// Kernels of Tube-Link's per-clip masked-attention query decoder (Mask2FormerVideoCCHeadTube.forward, the loop over the nine
// DetrTransformerDecoderLayers with forward_head_video in front of each): everything that is not a Linear layer.  The Linear layers run
// on the three-piece split-precision GEMM (axvs_gemm_nt.h); the contractions here are f32-input MFMAs (v_mfma_f32_16x16x4_f32), so
// every product of the decoder is fp32-accurate: the attention masks are decisions, and so is the matching that consumes the output.
//
//   m2f_to_cl_kernel<false> mask features [N,T,C,h,w] -> level resolution, channels-last [N][T*hl*wl][C] (bilinear, align_corners=False):
//                           the resize commutes with the mask einsum, so the mask logits at level resolution are
//                           mask_embed . resize(mask_feature) and the [N,T,Q,h,w] tensor of the reference never exists
//   m2f_to_cl_kernel<true>  memory [N,T,C,hl,wl] -> values (memory + level_embed) and keys (values + 3-D sine embedding), rows (t,y,x)
//   m2f_ln_kernel           sum of a GEMM's split-K partials + bias + residual, LayerNorm, optionally post_norm of the result (the next mask
//                           head's input)
//   m2f_logits_kernel       mask_embed . features: as a bit-packed attention mask + "any key open" flags, or as fp32 logits
//   m2f_attn_kernel         masked attention of one (clip, head, 16 queries, key chunk): online softmax, partial result
//   m2f_attn_combine_kernel the chunks' partial results -> [N*Q][C]
// No kernel waits for another workgroup and none adds floating-point numbers atomically: equal inputs give equal bits.
#pragma once
#include <hip/hip_runtime.h>

#include "axvs_common.h"
#include "axvs_layout.h"
#include "axvs_resize.h"

namespace axvs {

constexpr int kM2fC = 256;            // embed dims
constexpr int kM2fHeads = 8;          // heads of 32
constexpr int kM2fKeyChunk = 256;     // keys per attention workgroup, at least
constexpr int kM2fMaxChunks = 64;     // key chunks per (clip, head, query tile), at most

// ---- [N,T,C,h,w] -> channels-last rows at (hl, wl): a 32 (x) x 64 (channels) tile through LDS, reads along x, writes along c -------------
struct M2fMap { int T, h, w, hl, wl; };

__device__ __forceinline__ float m2f_sine3d(int t, int y, int x, int c, const M2fMap& g, float temperature, int normalize, float scale) {
  // SinePositionalEncoding3D (all positions valid): the arithmetic of pos3d_kernel (axvs_misc.h), C = 256 channels, num_feats = 128
  const int n = kM2fC / 2;
  float z = (float)(t + 1), yy = (float)(y + 1), xx = (float)(x + 1);
  if (normalize) {
    const float eps = 1e-6f;
    z = z / ((float)g.T + eps) * scale;
    yy = yy / ((float)g.hl + eps) * scale;
    xx = xx / ((float)g.wl + eps) * scale;
  }
  const int cc = c < n ? c : c - n;
  const float dim_t = powf(temperature, 2.f * (float)(cc / 2) / (float)n);
  const float a = (c < n ? yy : xx) / dim_t;
  float v = (cc & 1) ? cosf(a) : sinf(a);
  const float dim_z = powf(temperature, 2.f * (float)(c / 2) / (float)kM2fC);
  const float az = z / dim_z;
  v += (c & 1) ? cosf(az) : sinf(az);
  return v;
}

// MEM = false: out = bilinear resize of src (h, w) -> (hl, wl).  MEM = true (h = hl, w = wl): out = src + level_embed (the values),
// out2 = out + sine embedding (the keys).  grid (ceil(wl/32) * C/64, hl, N*T), 256 threads.
template <bool MEM>
__global__ __launch_bounds__(256) void m2f_to_cl_kernel(const float* __restrict__ src, float* __restrict__ out, float* __restrict__ out2,
                                                        const float* __restrict__ level_embed, M2fMap g, float temperature, int normalize,
                                                        float scale) {
  __shared__ float tile[32][65];
  const int tid = threadIdx.x;
  const int cchunks = kM2fC / 64;
  const int x0 = (int)(blockIdx.x / cchunks) * 32, c0 = (int)(blockIdx.x % cchunks) * 64, y = blockIdx.y;
  const int nt = blockIdx.z, t = nt % g.T, n = nt / g.T;
  {
    const int tx = tid & 31, cy = tid >> 5, x = x0 + tx;
    if (x < g.wl) {
      const float* const base = src + ((size_t)nt * kM2fC + c0) * g.h * g.w;
      if constexpr (MEM) {
#pragma unroll
        for (int j = 0; j < 8; ++j) tile[tx][cy + 8 * j] = base[(size_t)(cy + 8 * j) * g.h * g.w + (size_t)y * g.w + x];
      } else {
        const PanTap ty = pan_tap(y, PanAxis{g.h, g.hl, (float)g.h / (float)g.hl}, 0);
        const PanTap tx_ = pan_tap(x, PanAxis{g.w, g.wl, (float)g.w / (float)g.wl}, 0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float* const p = base + (size_t)(cy + 8 * j) * g.h * g.w;
          const float a = p[ty.i0 * g.w + tx_.i0], b = p[ty.i0 * g.w + tx_.i1], c = p[ty.i1 * g.w + tx_.i0], d = p[ty.i1 * g.w + tx_.i1];
          tile[tx][cy + 8 * j] = ty.l0 * (tx_.l0 * a + tx_.l1 * b) + ty.l1 * (tx_.l0 * c + tx_.l1 * d);      // upsample_bilinear2d's expression
        }
      }
    }
  }
  __syncthreads();
  const int c = tid & 63, xr = tid >> 6;
  const size_t S = (size_t)g.T * g.hl * g.wl;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int x = x0 + xr + 4 * j;
    if (x >= g.wl) continue;
    const size_t row = (size_t)n * S + ((size_t)t * g.hl + y) * g.wl + x;
    float v = tile[xr + 4 * j][c];
    if constexpr (MEM) {
      v += level_embed[c0 + c];
      out2[row * kM2fC + c0 + c] = v + m2f_sine3d(t, y, x, c0 + c, g, temperature, normalize, scale);
    }
    out[row * kM2fC + c0 + c] = v;
  }
}

// ---- rows ---------------------------------------------------------------------------------------------------------------------------------
// (x[n*Q + q] = query_feat[q], qpos[n*Q + q] = query_embed[q]: one broadcast_rows() launch with two pairs; the class logits:
//  class_logits_rows(), both axvs_layout.h)
__device__ __forceinline__ float4 m2f_ln_row(float4 v, const float* __restrict__ g, const float* __restrict__ b, int lane) {
  float s = v.x + v.y + v.z + v.w;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s = wave_xor_sum(s, o);
  const float mean = s * (1.f / kM2fC);
  const float dx = v.x - mean, dy = v.y - mean, dz = v.z - mean, dw = v.w - mean;
  float q = dx * dx + dy * dy + dz * dz + dw * dw;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q = wave_xor_sum(q, o);
  const float inv = 1.f / sqrtf(q * (1.f / kM2fC) + 1e-5f);
  const float4 gg = *reinterpret_cast<const float4*>(g + 4 * lane), bb = *reinterpret_cast<const float4*>(b + 4 * lane);
  return make_float4(dx * inv * gg.x + bb.x, dy * inv * gg.y + bb.y, dz * inv * gg.z + bb.z, dw * inv * gg.w + bb.w);
}

// One wave per row of 256: v = in (+ the further split-K partials in + z*part_stride, z < nparts, in order, + bias + res: the epilogue of a
// GEMM whose contraction was split over workgroups); out1 = LN(v; g1, b1) (g1 null: out1 is not written and stands for v),
// out2 = LN(out1; g2, b2) (g2 null: none); flags (nullable): the row's "any key open" flag is cleared for the mask head that follows.
__global__ __launch_bounds__(256) void m2f_ln_kernel(const float* __restrict__ in, int nparts, size_t part_stride, const float* __restrict__ bias,
                                                     const float* __restrict__ res, const float* __restrict__ g1, const float* __restrict__ b1,
                                                     float* __restrict__ out1, const float* __restrict__ g2, const float* __restrict__ b2,
                                                     float* __restrict__ out2, int* __restrict__ flags, int rows) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const size_t off = (size_t)row * kM2fC + 4 * lane;
  float4 v = *reinterpret_cast<const float4*>(in + off);
  for (int z = 1; z < nparts; ++z) {
    const float4 p = *reinterpret_cast<const float4*>(in + z * part_stride + off);
    v.x += p.x, v.y += p.y, v.z += p.z, v.w += p.w;
  }
  if (bias) {
    const float4 p = *reinterpret_cast<const float4*>(bias + 4 * lane);
    v.x += p.x, v.y += p.y, v.z += p.z, v.w += p.w;
  }
  if (res) {
    const float4 p = *reinterpret_cast<const float4*>(res + off);
    v.x += p.x, v.y += p.y, v.z += p.z, v.w += p.w;
  }
  if (g1) {
    v = m2f_ln_row(v, g1, b1, lane);
    *reinterpret_cast<float4*>(out1 + off) = v;
  }
  if (g2) *reinterpret_cast<float4*>(out2 + off) = m2f_ln_row(v, g2, b2, lane);
  if (flags && lane == 0) flags[row] = 0;
}

// ---- mask_embed . features ------------------------------------------------------------------------------------------------------------------
// One wave: 32 keys (two 16-key MFMA tiles, their 256 channels held in registers) against a run of 16-query tiles.
//   D[query 4 g + r][key i] = sum_c me[query][c] f[key][c]:  A = query rows, B = key rows, the contraction in the order the float4 loads give
//   (lane group g holds channels 16 c4 + 4 g + e: step (c4, e) contracts channels {16 c4 + 4 g' + e}, the same for both operands).
// CL:   features channels-last [Z][S][C]; else channels-first [Z][C][S] (the mask features themselves: Z = (clip, frame), S = h*w)
// BITS: bit (key & 31) of bits[(z*Q + q)*W + key / 32] = logit < 0 (sigmoid < 0.5: the key is masked), bits past S are 0, and
//       flags[z*Q + q] = 1 when a key of the row is open (all writers store the same value); else: out[(z*Q + q)*S + key] = logit.
// me rows of batch z / zdiv.  grid (ceil(S/128), query splits, Z), 256 threads; no barrier: a wave past the keys returns.
template <bool CL, bool BITS>
__global__ __launch_bounds__(256) void m2f_logits_kernel(const float* __restrict__ me, const float* __restrict__ feat, int Q, int S, int zdiv,
                                                         unsigned* __restrict__ bits, int* __restrict__ flags, float* __restrict__ out, int W,
                                                         int qtiles_per_y) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fi = lane & 15, fg = lane >> 4;
  const int z = blockIdx.z;
  const int key0 = ((int)blockIdx.x * 4 + wave) * 32;
  if (key0 >= S) return;
  const float* const A = me + (size_t)(z / zdiv) * Q * kM2fC;
  const float* const F = feat + (size_t)z * S * kM2fC;
  float b[2][16][4];
  bool valid[2];
#pragma unroll
  for (int tl = 0; tl < 2; ++tl) {
    const int key = key0 + 16 * tl + fi;
    valid[tl] = key < S;
    const int kc = valid[tl] ? key : S - 1;
#pragma unroll
    for (int c4 = 0; c4 < 16; ++c4) {
      if constexpr (CL) {
        const float4 v = *reinterpret_cast<const float4*>(F + (size_t)kc * kM2fC + 16 * c4 + 4 * fg);
        b[tl][c4][0] = v.x, b[tl][c4][1] = v.y, b[tl][c4][2] = v.z, b[tl][c4][3] = v.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) b[tl][c4][e] = F[(size_t)(16 * c4 + 4 * fg + e) * S + kc];
      }
    }
  }
  const int nqt = (Q + 15) / 16;
  const int qt0 = (int)blockIdx.y * qtiles_per_y, qt1 = min(nqt, qt0 + qtiles_per_y);
  for (int qt = qt0; qt < qt1; ++qt) {
    const int qc = min(qt * 16 + fi, Q - 1);
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int c4 = 0; c4 < 16; ++c4) {
      const float4 a4 = *reinterpret_cast<const float4*>(A + (size_t)qc * kM2fC + 16 * c4 + 4 * fg);
      const float a[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[0][c4][e], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[1][c4][e], acc[1], 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = qt * 16 + 4 * fg + r;                 // this lane's query of accumulator element r; its keys: key0 + 16 tl + fi
      if constexpr (BITS) {
        // a ballot holds 16 keys of four queries: bits 16 g' .. 16 g' + 15 belong to query 4 g' + r
        const unsigned long long m0 = __ballot(valid[0] && acc[0][r] < 0.f), m1 = __ballot(valid[1] && acc[1][r] < 0.f);
        const unsigned long long o0 = __ballot(valid[0] && !(acc[0][r] < 0.f)), o1 = __ballot(valid[1] && !(acc[1][r] < 0.f));
        if (fi == 0 && q < Q) {
          const unsigned word = (unsigned)((m0 >> (16 * fg)) & 0xffffull) | ((unsigned)((m1 >> (16 * fg)) & 0xffffull) << 16);
          bits[((size_t)z * Q + q) * W + (key0 >> 5)] = word;
          if ((((o0 | o1) >> (16 * fg)) & 0xffffull) != 0) flags[(size_t)z * Q + q] = 1;
        }
      } else if (q < Q) {
        float* const o = out + ((size_t)z * Q + q) * S + key0 + fi;
        if (valid[0]) o[0] = acc[0][r];
        if (valid[1]) o[16] = acc[1][r];
      }
    }
  }
}

// ---- attention ----------------------------------------------------------------------------------------------------------------------------------
struct M2fAttn {
  const float *q, *k, *v;            // rows (n*Q + query) / (n*S + key), head h at columns 32 h ..; row strides ldq / ldk / ldv
  long long ldq, ldk, ldv;
  int Q, S, chunk, nchunk;           // chunk: keys per workgroup, a multiple of 32
  float scale;
  const unsigned* bits;              // nullable [N*Q][W]: bit set = key masked
  const int* flags;                  // [N*Q]: 0 = every key of the row is masked -> the row attends to all keys
  int W;
  float *po, *pml;                   // partial results [N*8][nchunk][Q][32] and (running maximum, sum) [N*8][nchunk][Q][2]
};

// One wave: 16 queries x one key chunk of one (clip, head).  Scores transposed, D[key 4 g + r][query i] (A = key rows, B = query rows), so
// the probabilities of a lane are the B operand of the value product as they stand: D[channel][query] += V^T[channel][key] P[key][query].
// grid (query tiles, chunks, N*8), 64 threads.
__global__ __launch_bounds__(64) void m2f_attn_kernel(M2fAttn a) {
  const int lane = threadIdx.x, fi = lane & 15, fg = lane >> 4;
  const int qt = blockIdx.x, ch = blockIdx.y, z = blockIdx.z, n = z >> 3, h = z & 7;
  const int qrow = qt * 16 + fi, qc = min(qrow, a.Q - 1);
  float qr[8];
  {
    const float* const p = a.q + ((size_t)n * a.Q + qc) * a.ldq + 32 * h + 8 * fg;
    const float4 u = *reinterpret_cast<const float4*>(p), w = *reinterpret_cast<const float4*>(p + 4);
    qr[0] = u.x * a.scale, qr[1] = u.y * a.scale, qr[2] = u.z * a.scale, qr[3] = u.w * a.scale;
    qr[4] = w.x * a.scale, qr[5] = w.y * a.scale, qr[6] = w.z * a.scale, qr[7] = w.w * a.scale;
  }
  const bool use_mask = a.bits != nullptr && a.flags[(size_t)n * a.Q + qc] != 0;
  const unsigned* const brow = a.bits ? a.bits + ((size_t)n * a.Q + qc) * a.W : nullptr;
  const int s0 = ch * a.chunk, s1 = min(a.S, s0 + a.chunk);
  float m = -INFINITY, sum = 0.f;
  f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int key0 = s0; key0 < s1; key0 += 16) {
    float kr[8];
    {
      const int kc = min(key0 + fi, a.S - 1);
      const float* const p = a.k + ((size_t)n * a.S + kc) * a.ldk + 32 * h + 8 * fg;
      const float4 u = *reinterpret_cast<const float4*>(p), w = *reinterpret_cast<const float4*>(p + 4);
      kr[0] = u.x, kr[1] = u.y, kr[2] = u.z, kr[3] = u.w, kr[4] = w.x, kr[5] = w.y, kr[6] = w.z, kr[7] = w.w;
    }
    float va[4][2];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int kc = min(key0 + 4 * fg + r, a.S - 1);
      const float* const p = a.v + ((size_t)n * a.S + kc) * a.ldv + 32 * h + fi;
      va[r][0] = p[0];
      va[r][1] = p[16];
    }
    f32x4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 8; ++t) sc = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[t], qr[t], sc, 0, 0, 0);
    const unsigned word = use_mask ? brow[key0 >> 5] >> ((key0 & 31) + 4 * fg) : 0u;
    float sv[4], tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool open = key0 + 4 * fg + r < s1 && !((word >> r) & 1u);
      sv[r] = open ? sc[r] : -INFINITY;
      tmax = fmaxf(tmax, sv[r]);
    }
    tmax = wave_xor_max(tmax, 16);
    tmax = wave_xor_max(tmax, 32);
    const float mn = fmaxf(m, tmax), ms = mn == -INFINITY ? 0.f : mn;
    const float alpha = expf(m - ms);
    float p[4], ps = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[r] = expf(sv[r] - ms);
      ps += p[r];
    }
    sum = sum * alpha + ps;         // this lane's keys only: the four lane groups are added once, at the end
    m = mn;
    acc[0] *= alpha;
    acc[1] *= alpha;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[r][0], p[r], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[r][1], p[r], acc[1], 0, 0, 0);
    }
  }
  sum = wave_xor_sum(sum, 16);
  sum = wave_xor_sum(sum, 32);
  if (qrow < a.Q) {
    const size_t row = ((size_t)z * a.nchunk + ch) * a.Q + qrow;
    *reinterpret_cast<float4*>(a.po + row * 32 + 4 * fg) = make_float4(acc[0][0], acc[0][1], acc[0][2], acc[0][3]);
    *reinterpret_cast<float4*>(a.po + row * 32 + 16 + 4 * fg) = make_float4(acc[1][0], acc[1][1], acc[1][2], acc[1][3]);
    if (fg == 0) {
      a.pml[row * 2] = m;
      a.pml[row * 2 + 1] = sum;
    }
  }
}

// out[(n*Q + q)][32 h + d] = sum_c e^(m_c - M) po_c / sum_c e^(m_c - M) sum_c, the chunks in order.  grid N*Q, 256 threads.
__global__ __launch_bounds__(256) void m2f_attn_combine_kernel(const float* __restrict__ po, const float* __restrict__ pml, float* __restrict__ out,
                                                               int Q, int nchunk) {
  const int row = blockIdx.x, n = row / Q, q = row % Q, h = threadIdx.x >> 5, d = threadIdx.x & 31;
  const size_t base = (size_t)(n * kM2fHeads + h) * nchunk;
  float M = -INFINITY;
  for (int c = 0; c < nchunk; ++c) M = fmaxf(M, pml[((base + c) * Q + q) * 2]);
  if (M == -INFINITY) M = 0.f;
  float num = 0.f, den = 0.f;
  for (int c = 0; c < nchunk; ++c) {
    const size_t r = (base + c) * Q + q;
    const float w = expf(pml[r * 2] - M);
    num += w * po[r * 32 + d];
    den += w * pml[r * 2 + 1];
  }
  out[(size_t)row * kM2fC + threadIdx.x] = num / den;
}

}  // namespace axvs
