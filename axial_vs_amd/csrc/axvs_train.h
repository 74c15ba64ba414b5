// Training tier of the axial-trajectory attention layer: fp32 activations in natural [B,T,H,W] row order, the
// attention / softmax / dropout / LayerNorm kernels here, the Linear layers' GEMMs (forward, dgrad, wgrad) in axvs_gemm_nt.h /
// axvs_train_gemm.h (split-precision bf16 MFMA; host side: axvs_train.hip).  Nothing here is on the inference path; that stays on the fused 16-bit MFMA kernels (axvs_fused.h).
//
// Reference semantics (WC/temporal_attention.py): TrajectoryAttention.forward :35-76 (dropout on the spatial attention map :55),
// TemporalAxialTrajectoryAttentionLayer.forward :187-220 (dropout1 on each pass output :204, :213; dropout2 / dropout3 in the
// FFN :182-183).  Dropout masks come from a counter-based hash of (seed, site, element index) so that the backward pass (and the
// recomputed forward, and the CPU oracle in the tests) regenerate them instead of storing them.
#pragma once
#include "axvs_common.h"
#include "axvs_gemm_nt.h"

namespace axvs {
namespace tr {

template <int D>
__device__ __forceinline__ void load_row(float (&r)[D], const float* p) {
#pragma unroll
  for (int i = 0; i < D; i += 4) {
    const float4 v = *reinterpret_cast<const float4*>(p + i);
    r[i] = v.x; r[i + 1] = v.y; r[i + 2] = v.z; r[i + 3] = v.w;
  }
}
template <int D>
__device__ __forceinline__ void store_row(float* p, const float (&r)[D]) {
#pragma unroll
  for (int i = 0; i < D; i += 4) *reinterpret_cast<float4*>(p + i) = make_float4(r[i], r[i + 1], r[i + 2], r[i + 3]);
}
template <int D>
__device__ __forceinline__ float dot_lds(const float (&a)[D], const float* s) {   // s: LDS row (all lanes the same row: broadcast)
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < D; i += 4) {
    const float4 v = *reinterpret_cast<const float4*>(s + i);
    acc += a[i] * v.x + a[i + 1] * v.y + a[i + 2] * v.z + a[i + 3] * v.w;
  }
  return acc;
}
template <int D>
__device__ __forceinline__ void axpy_lds(float (&acc)[D], float a, const float* s) {
#pragma unroll
  for (int i = 0; i < D; i += 4) {
    const float4 v = *reinterpret_cast<const float4*>(s + i);
    acc[i] += a * v.x; acc[i + 1] += a * v.y; acc[i + 2] += a * v.z; acc[i + 3] += a * v.w;
  }
}

// the rows of frame f of sequence s, head h: global [.., C] -> LDS [L][D]
template <int D>
__device__ __forceinline__ void stage_frame(float* dst, const float* src, const RowMap& rm, int s, int f, int h, int C, int tid) {
  constexpr int V = D / 4;
  for (int i = tid; i < rm.L * V; i += 256) {
    const int n = i / V, c4 = i - n * V;
    const long long row = nat_row(rm, s * rm.N + f * rm.L + n);
    *reinterpret_cast<float4*>(dst + n * D + c4 * 4) = *reinterpret_cast<const float4*>(src + row * C + h * D + c4 * 4);
  }
}

// ---- spatial half, forward (WC/temporal_attention.py:47-58): x[q, f, :] = sum_n drop(softmax_n(scale q.k_{f,n})) v_{f,n}
//      one workgroup per (sequence, head), one thread per query, K_f / V_f of the frame in LDS.  x: [M, T, C] by natural row.
//      dropout index of P[(s h), q, f, n] is its offset in the reference's tensor: (((s heads + h) N + q) T + f) L + n.
template <int D>
__global__ __launch_bounds__(256) void tr_spatial_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                              const float* __restrict__ v, float* __restrict__ x, RowMap rm, int T, int C,
                                                              int heads, float scale, Drop dr) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x, s = blockIdx.x / heads, h = blockIdx.x - s * heads, N = rm.N, L = rm.L;
  float* ks = smem;
  float* vs = smem + L * D;
  for (int q0 = 0; q0 < N; q0 += 256) {
    const int qn = q0 + tid;
    const bool act = qn < N;
    const long long mq = nat_row(rm, s * N + (act ? qn : 0));
    float qr[D];
    load_row<D>(qr, q + mq * C + h * D);
#pragma unroll
    for (int i = 0; i < D; ++i) qr[i] *= scale;
    for (int f = 0; f < T; ++f) {
      __syncthreads();
      stage_frame<D>(ks, k, rm, s, f, h, C, tid);
      stage_frame<D>(vs, v, rm, s, f, h, C, tid);
      __syncthreads();
      if (!act) continue;
      float mx = -INFINITY;
      for (int n = 0; n < L; ++n) mx = fmaxf(mx, dot_lds<D>(qr, ks + n * D));
      float sum = 0.f, acc[D];
#pragma unroll
      for (int i = 0; i < D; ++i) acc[i] = 0.f;
      const unsigned long long base = ((((unsigned long long)s * heads + h) * N + qn) * T + f) * L;
      for (int n = 0; n < L; ++n) {
        const float p = __expf(dot_lds<D>(qr, ks + n * D) - mx);
        sum += p;
        const float kp = drop_keep(dr, base + n);
        if (kp != 0.f) axpy_lds<D>(acc, p * kp, vs + n * D);
      }
      const float inv = 1.f / sum;
#pragma unroll
      for (int i = 0; i < D; ++i) acc[i] *= inv;
      store_row<D>(x + (mq * T + f) * C + h * D, acc);
    }
  }
}

// ---- the same forward on the matrix cores, head_dim 32: v_mfma_f32_16x16x4_f32 (fp32 operands: the tier stays fp32) ----
// One workgroup per (sequence, head), K_f / V_f of the frame in LDS (row stride 36 floats), 4 waves that each take 16-query tiles.
// Per (query tile, 16-key tile): S^T = K Q^T as 8 MFMAs (lane (j, g) supplies d = 8 g + t at step t for key / query j: the
// contraction order over d is free), flash-style running max / sum per query (the 4 lane groups of a query reduce with two
// xor-shuffles), then X^T += V^T P^T as 4 x 2 MFMAs where step r contracts keys {4 g + r}: exactly the keys lane group g holds in
// register r of the score tile, so probabilities feed the B operand without leaving their registers.
constexpr int kTrLd = 36;   // LDS row stride (floats) of the staged K / V rows

__device__ __forceinline__ float xor_max16_32(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float xor_sum16_32(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// rows of frame f of (sequence s, head h) -> LDS [ceil16(L)][kTrLd], rows past L zero
__device__ __forceinline__ void stage_frame36(float* dst, const float* src, const RowMap& rm, int s, int f, int h, int C, int tid) {
  const int Lp = (rm.L + 15) & ~15;
  for (int i = tid; i < Lp * 8; i += 256) {
    const int n = i >> 3, c4 = i & 7;
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (n < rm.L) v = *reinterpret_cast<const float4*>(src + nat_row(rm, s * rm.N + f * rm.L + n) * C + h * 32 + c4 * 4);
    *reinterpret_cast<float4*>(dst + n * kTrLd + c4 * 4) = v;
  }
}

__global__ __launch_bounds__(256) void tr_spatial_fwd_mfma_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                   const float* __restrict__ v, float* __restrict__ x,
                                                                   float* __restrict__ stats /* [(s heads + h), N, T, 3]: max, 1 / sum, - */,
                                                                   RowMap rm, int T, int C, int heads, float scale, Drop dr) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int s = blockIdx.x / heads, h = blockIdx.x - s * heads, N = rm.N, L = rm.L;
  const int Lp = (L + 15) & ~15, nkt = Lp >> 4, nqt = (N + 15) >> 4;
  float* ks = smem;
  float* vs = smem + Lp * kTrLd;
  // few sequences (the cross-clip module: B x heads workgroups): gridDim.y splits the query tiles, gridDim.z the frames -- every
  // (query tile, frame) is computed by exactly one wave whatever the split, with the same instructions
  const int fper = (T + (int)gridDim.z - 1) / (int)gridDim.z, f0 = (int)blockIdx.z * fper, f1 = min(T, f0 + fper);
  for (int f = f0; f < f1; ++f) {
    __syncthreads();
    stage_frame36(ks, k, rm, s, f, h, C, tid);
    stage_frame36(vs, v, rm, s, f, h, C, tid);
    __syncthreads();
    for (int qt = (int)blockIdx.y * 4 + wave; qt < nqt; qt += 4 * (int)gridDim.y) {
      const int qn = qt * 16 + j;
      const long long mq = nat_row(rm, s * N + min(qn, N - 1));
      float qr[8];
      {
        const float4 a = *reinterpret_cast<const float4*>(q + mq * C + h * 32 + 8 * g), b = *reinterpret_cast<const float4*>(q + mq * C + h * 32 + 8 * g + 4);
        qr[0] = a.x * scale; qr[1] = a.y * scale; qr[2] = a.z * scale; qr[3] = a.w * scale;
        qr[4] = b.x * scale; qr[5] = b.y * scale; qr[6] = b.z * scale; qr[7] = b.w * scale;
      }
      float m = -INFINITY, sum = 0.f;
      f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      const unsigned long long base = ((((unsigned long long)s * heads + h) * N + min(qn, N - 1)) * T + f) * L;
      for (int kt = 0; kt < nkt; ++kt) {
        const float* kp = ks + (kt * 16 + j) * kTrLd + 8 * g;
        const float4 ka = *reinterpret_cast<const float4*>(kp), kb = *reinterpret_cast<const float4*>(kp + 4);
        const float kr[8] = {ka.x, ka.y, ka.z, ka.w, kb.x, kb.y, kb.z, kb.w};
        f32x4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 8; ++t) sc = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[t], qr[t], sc, 0, 0, 0);
        const int n0 = kt * 16 + 4 * g;             // my 4 keys: n0 .. n0 + 3
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (n0 + r >= L) sc[r] = -INFINITY;
          tmax = fmaxf(tmax, sc[r]);
        }
        const float mn = fmaxf(m, xor_max16_32(tmax));
        const float alpha = __expf(m - mn);
        float p[4], ps = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p[r] = __expf(sc[r] - mn);
          ps += p[r];
          if (n0 + r < L) p[r] *= drop_keep(dr, base + n0 + r);
        }
        sum = sum * alpha + xor_sum16_32(ps);
        m = mn;
        acc[0] *= alpha;
        acc[1] *= alpha;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float* vp = vs + (n0 + r) * kTrLd + j;
          acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[0], p[r], acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[16], p[r], acc[1], 0, 0, 0);
        }
      }
      if (qn < N) {
        const float inv = 1.f / sum;
        float* xo = x + (mq * T + f) * C + h * 32 + 4 * g;        // lane (query j, group g): channels dt * 16 + 4 g + r
        *reinterpret_cast<float4*>(xo) = float4{acc[0][0] * inv, acc[0][1] * inv, acc[0][2] * inv, acc[0][3] * inv};
        *reinterpret_cast<float4*>(xo + 16) = float4{acc[1][0] * inv, acc[1][1] * inv, acc[1][2] * inv, acc[1][3] * inv};
        if (g == 0) {                                 // softmax statistics of (query, frame): the backward kernels rebuild P from them
          float* st = stats + ((((size_t)s * heads + h) * N + qn) * T + f) * 3;
          st[0] = m;
          st[1] = inv;
        }
      }
    }
  }
}

// ---- the same forward for frames of at most 128 keys (every shipped axis length): 16-bit matrix cores in split precision, and the
//      score tiles of a WHOLE frame in registers.  (a) Every fp32 operand is cut into THREE bf16 pieces (24 mantissa bits = all of
//      fp32) and a product is six 16-bit MFMAs (hh, hm, mh, mm, hl, lh; what is dropped is 2^-24 of the product), as in the forward
//      GEMMs (axvs_gemm_nt.h): 96 + 96 instead of 256 + 256 matrix-pipe cycles per 16-key tile (v_mfma_f32_16x16x4_f32 runs at 1/16
//      of the 16-bit rate); K and V of the frame are split ONCE while they are staged (K: [piece][key][32], V transposed:
//      [piece][channel][key] so that a lane reads its four keys of a channel as 8 bytes), q once per query tile (its rows requested a
//      tile ahead).  (b) All score tiles of the frame are computed first (<= 8 tiles = 32 registers), so the softmax takes one
//      maximum and one sum per (query, frame): two cross-lane exchanges per frame instead of four per tile, no rescaling of the
//      accumulators, no running statistics.  Operand layouts: S^T = K Q^T is a 16x16x32 product (lane (j, g) holds channels
//      8 g .. 8 g + 7 of key / query j, as in the fp32 kernel), X^T += V^T P^T a 16x16x16 one (lane (j, g) holds keys 4 g .. 4 g + 3:
//      the probabilities stay where the score tile left them).  Statistics (max, 1 / sum), dropout indices and the output layout
//      are those of tr_spatial_fwd_mfma_kernel, so the backward kernels do not care which one ran (saved activations of the two
//      agree to 1e-6).  Measured at [1,4,256,64,64]: 107 -> 97 us per launch -- and the counters say why not more
//      (profiles/r3_train_attention_pmc.json): the kernel is bound by VALU issue, 290 VALU instructions per 16-key tile and wave
//      (dropout hash of four scores ~100, the three-piece split of four probabilities ~50, mask / max / exp / sum ~30, 64-bit
//      element indices, LDS addresses) against 18 MFMAs; the matrix pipe is busy 15 % of the time.
typedef short s16x4 __attribute__((ext_vector_type(4)));
constexpr int kSpMaxTiles = 8;      // key tiles of a frame held in registers: L <= 128

__device__ __forceinline__ void split3(float x, u16& h, u16& m, u16& l) {
  const __bf16 a = (__bf16)x;
  const float r1 = x - (float)a;
  const __bf16 b = (__bf16)r1;
  const __bf16 c = (__bf16)(r1 - (float)b);
  h = __builtin_bit_cast(u16, a);
  m = __builtin_bit_cast(u16, b);
  l = __builtin_bit_cast(u16, c);
}
__device__ __forceinline__ f32x4 mfma6_32(const u16x8 (&a)[3], const u16x8 (&b)[3], f32x4 c) {     // 16x16x32, three-piece operands
  c = H16<true>::mfma(a[0], b[0], c);
  c = H16<true>::mfma(a[0], b[1], c);
  c = H16<true>::mfma(a[1], b[0], c);
  c = H16<true>::mfma(a[1], b[1], c);
  c = H16<true>::mfma(a[0], b[2], c);
  return H16<true>::mfma(a[2], b[0], c);
}
__device__ __forceinline__ f32x4 mfma6_16(const s16x4 (&a)[3], const s16x4 (&b)[3], f32x4 c) {     // 16x16x16
  c = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a[0], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a[0], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a[1], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a[1], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a[0], b[2], c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a[2], b[0], c, 0, 0, 0);
}
// LDS bytes: K pieces [3][Lp][32] + V^T pieces [3][32][Lp + 4] (16-bit)
__host__ __device__ inline size_t spatial_split_lds(int L) {
  const int Lp = (L + 15) & ~15;
  return (size_t)3 * ((size_t)Lp * 32 + (size_t)32 * (Lp + 4)) * sizeof(u16);
}

__global__ __launch_bounds__(256) void tr_spatial_fwd_split_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                    const float* __restrict__ v, float* __restrict__ x,
                                                                    float* __restrict__ stats, RowMap rm, int T, int C, int heads, float scale,
                                                                    Drop dr) {
  extern __shared__ float smem[];
  u16* const kp = reinterpret_cast<u16*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int s = blockIdx.x / heads, h = blockIdx.x - s * heads, N = rm.N, L = rm.L;
  const int Lp = (L + 15) & ~15, nkt = Lp >> 4, nqt = (N + 15) >> 4, LV = Lp + 4;
  u16* const vt = kp + 3 * Lp * 32;
  const int fper = (T + (int)gridDim.z - 1) / (int)gridDim.z, f0 = (int)blockIdx.z * fper, f1 = min(T, f0 + fper);
  const int qstep = 4 * (int)gridDim.y;
  for (int f = f0; f < f1; ++f) {
    __syncthreads();
    for (int i = tid; i < Lp * 4; i += 256) {          // (key n, 8-channel chunk c8): K into its [piece][n][32] tiles, V into [piece][c][n]
      const int n = i >> 2, c8 = i & 3;
      float kv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, vv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (n < L) {
        const long long row = nat_row(rm, s * N + f * L + n) * C + h * 32 + c8 * 8;
        const float4 a = *reinterpret_cast<const float4*>(k + row), b = *reinterpret_cast<const float4*>(k + row + 4);
        const float4 c = *reinterpret_cast<const float4*>(v + row), d = *reinterpret_cast<const float4*>(v + row + 4);
        kv[0] = a.x; kv[1] = a.y; kv[2] = a.z; kv[3] = a.w; kv[4] = b.x; kv[5] = b.y; kv[6] = b.z; kv[7] = b.w;
        vv[0] = c.x; vv[1] = c.y; vv[2] = c.z; vv[3] = c.w; vv[4] = d.x; vv[5] = d.y; vv[6] = d.z; vv[7] = d.w;
      }
      u16x8 ph, pm, pl;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        u16 a, b, c;
        split3(kv[e], a, b, c);
        ph[e] = a; pm[e] = b; pl[e] = c;
        split3(vv[e], a, b, c);
        vt[(0 * 32 + c8 * 8 + e) * LV + n] = a;
        vt[(1 * 32 + c8 * 8 + e) * LV + n] = b;
        vt[(2 * 32 + c8 * 8 + e) * LV + n] = c;
      }
      *reinterpret_cast<u16x8*>(kp + (0 * Lp + n) * 32 + c8 * 8) = ph;
      *reinterpret_cast<u16x8*>(kp + (1 * Lp + n) * 32 + c8 * 8) = pm;
      *reinterpret_cast<u16x8*>(kp + (2 * Lp + n) * 32 + c8 * 8) = pl;
    }
    __syncthreads();
    const int qt0 = (int)blockIdx.y * 4 + wave;
    float4 qa = {0.f, 0.f, 0.f, 0.f}, qb = qa;            // the next tile's q rows are requested while this tile computes
    if (qt0 < nqt) {
      const float* qp0 = q + nat_row(rm, s * N + min(qt0 * 16 + j, N - 1)) * C + h * 32 + 8 * g;
      qa = *reinterpret_cast<const float4*>(qp0);
      qb = *reinterpret_cast<const float4*>(qp0 + 4);
    }
    for (int qt = qt0; qt < nqt; qt += qstep) {
      const int qn = qt * 16 + j;
      const long long mq = nat_row(rm, s * N + min(qn, N - 1));
      u16x8 qp[3];
      {
        const float qr[8] = {qa.x * scale, qa.y * scale, qa.z * scale, qa.w * scale, qb.x * scale, qb.y * scale, qb.z * scale, qb.w * scale};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          u16 a_, b_, c_;
          split3(qr[e], a_, b_, c_);
          qp[0][e] = a_; qp[1][e] = b_; qp[2][e] = c_;
        }
      }
      if (qt + qstep < nqt) {
        const float* qpn = q + nat_row(rm, s * N + min((qt + qstep) * 16 + j, N - 1)) * C + h * 32 + 8 * g;
        qa = *reinterpret_cast<const float4*>(qpn);
        qb = *reinterpret_cast<const float4*>(qpn + 4);
      }
      // scores of the whole frame: sc[kt][r] = S^T[key 16 kt + 4 g + r][query j]
      f32x4 sc[kSpMaxTiles];
      float m = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < kSpMaxTiles; ++kt) {
        if (kt < nkt) {
          u16x8 ka[3];
#pragma unroll
          for (int p = 0; p < 3; ++p) ka[p] = *reinterpret_cast<const u16x8*>(kp + (p * Lp + kt * 16 + j) * 32 + 8 * g);
          sc[kt] = mfma6_32(ka, qp, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (kt * 16 + 4 * g + r >= L) sc[kt][r] = -INFINITY;
            m = fmaxf(m, sc[kt][r]);
          }
        }
      }
      m = xor_max16_32(m);
      const unsigned long long base = ((((unsigned long long)s * heads + h) * N + min(qn, N - 1)) * T + f) * L;
      float sum = 0.f;
      f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int kt = 0; kt < kSpMaxTiles; ++kt) {
        if (kt < nkt) {
          const int n0 = kt * 16 + 4 * g;
          s16x4 pp[3];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float p = __expf(sc[kt][r] - m);
            sum += p;
            if (n0 + r < L) p *= drop_keep(dr, base + n0 + r);
            u16 a_, b_, c_;
            split3(p, a_, b_, c_);
            pp[0][r] = (short)a_; pp[1][r] = (short)b_; pp[2][r] = (short)c_;
          }
#pragma unroll
          for (int ct = 0; ct < 2; ++ct) {
            s16x4 va[3];
#pragma unroll
            for (int p3 = 0; p3 < 3; ++p3) va[p3] = *reinterpret_cast<const s16x4*>(vt + (p3 * 32 + ct * 16 + j) * LV + n0);
            acc[ct] = mfma6_16(va, pp, acc[ct]);        // X^T[channel 16 ct + 4 g + r][query j]
          }
        }
      }
      sum = xor_sum16_32(sum);
      if (qn < N) {
        const float inv = 1.f / sum;
        float* xo = x + (mq * T + f) * C + h * 32 + 4 * g;
        *reinterpret_cast<float4*>(xo) = float4{acc[0][0] * inv, acc[0][1] * inv, acc[0][2] * inv, acc[0][3] * inv};
        *reinterpret_cast<float4*>(xo + 16) = float4{acc[1][0] * inv, acc[1][1] * inv, acc[1][2] * inv, acc[1][3] * inv};
        if (g == 0) {
          float* st = stats + ((((size_t)s * heads + h) * N + qn) * T + f) * 3;
          st[0] = m;
          st[1] = inv;
        }
      }
    }
  }
}

// ---- backward on the matrix cores, part 1 (queries): D = dx . x (= sum_n P keep dP, the flash-attention identity), then per
//      16-key tile  S^T = K Q^T,  dP^T = V dX^T  (8 + 8 MFMAs),  dS = P (keep dP - D) with P rebuilt from the forward's (max, 1/sum),
//      dq^T += K^T dS^T (4 x 2 MFMAs, keys {4 g + r} per step as in the forward).  dq accumulates over the frames in global memory
//      (first frame writes).  Writes D into stats[.., 2] for part 2.
__global__ __launch_bounds__(256) void tr_spatial_bwd_q_mfma_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                     const float* __restrict__ v, const float* __restrict__ x,
                                                                     const float* __restrict__ dx, float* __restrict__ dq,
                                                                     float* __restrict__ stats, RowMap rm, int T, int C, int heads, float scale,
                                                                     Drop dr) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int s = blockIdx.x / heads, h = blockIdx.x - s * heads, N = rm.N, L = rm.L;
  const int Lp = (L + 15) & ~15, nkt = Lp >> 4, nqt = (N + 15) >> 4;
  float* ks = smem;
  float* vs = smem + Lp * kTrLd;
  for (int f = 0; f < T; ++f) {            // (dq accumulates over the frames: they stay in one workgroup; gridDim.y splits the query tiles)
    __syncthreads();
    stage_frame36(ks, k, rm, s, f, h, C, tid);
    stage_frame36(vs, v, rm, s, f, h, C, tid);
    __syncthreads();
    for (int qt = (int)blockIdx.y * 4 + wave; qt < nqt; qt += 4 * (int)gridDim.y) {
      const int qn = qt * 16 + j, qc = min(qn, N - 1);
      const long long mq = nat_row(rm, s * N + qc);
      float qr[8], dxr[8];
      float dsum;
      {
        const float* qp = q + mq * C + h * 32 + 8 * g;
        const float* gp = dx + (mq * T + f) * C + h * 32 + 8 * g;
        const float* xp = x + (mq * T + f) * C + h * 32 + 8 * g;
        const float4 a = *reinterpret_cast<const float4*>(qp), b = *reinterpret_cast<const float4*>(qp + 4);
        const float4 c = *reinterpret_cast<const float4*>(gp), d = *reinterpret_cast<const float4*>(gp + 4);
        const float4 e = *reinterpret_cast<const float4*>(xp), e2 = *reinterpret_cast<const float4*>(xp + 4);
        qr[0] = a.x * scale; qr[1] = a.y * scale; qr[2] = a.z * scale; qr[3] = a.w * scale;
        qr[4] = b.x * scale; qr[5] = b.y * scale; qr[6] = b.z * scale; qr[7] = b.w * scale;
        dxr[0] = c.x; dxr[1] = c.y; dxr[2] = c.z; dxr[3] = c.w; dxr[4] = d.x; dxr[5] = d.y; dxr[6] = d.z; dxr[7] = d.w;
        dsum = xor_sum16_32(c.x * e.x + c.y * e.y + c.z * e.z + c.w * e.w + d.x * e2.x + d.y * e2.y + d.z * e2.z + d.w * e2.w);
      }
      float* st = stats + ((((size_t)s * heads + h) * N + qc) * T + f) * 3;
      const float m = st[0], inv = st[1];
      f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      const unsigned long long base = ((((unsigned long long)s * heads + h) * N + qc) * T + f) * L;
      for (int kt = 0; kt < nkt; ++kt) {
        const float* kp = ks + (kt * 16 + j) * kTrLd + 8 * g;
        const float* vp = vs + (kt * 16 + j) * kTrLd + 8 * g;
        const float4 ka = *reinterpret_cast<const float4*>(kp), kb = *reinterpret_cast<const float4*>(kp + 4);
        const float4 va = *reinterpret_cast<const float4*>(vp), vb = *reinterpret_cast<const float4*>(vp + 4);
        const float kr[8] = {ka.x, ka.y, ka.z, ka.w, kb.x, kb.y, kb.z, kb.w};
        const float vr[8] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w};
        f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          sc = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[t], qr[t], sc, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[t], dxr[t], dp, 0, 0, 0);
        }
        const int n0 = kt * 16 + 4 * g;
        float ds[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool valid = n0 + r < L;
          const float P = valid ? __expf(sc[r] - m) * inv : 0.f;
          const float kp_ = valid ? drop_keep(dr, base + n0 + r) : 0.f;
          ds[r] = P * (kp_ * dp[r] - dsum);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float* kt_ = ks + (n0 + r) * kTrLd + j;
          acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(kt_[0], ds[r], acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(kt_[16], ds[r], acc[1], 0, 0, 0);
        }
      }
      if (qn < N) {
        float* o = dq + mq * C + h * 32 + 4 * g;
        float4 o0 = float4{acc[0][0] * scale, acc[0][1] * scale, acc[0][2] * scale, acc[0][3] * scale};
        float4 o1 = float4{acc[1][0] * scale, acc[1][1] * scale, acc[1][2] * scale, acc[1][3] * scale};
        if (f > 0) {
          const float4 p0 = *reinterpret_cast<const float4*>(o), p1 = *reinterpret_cast<const float4*>(o + 16);
          o0.x += p0.x; o0.y += p0.y; o0.z += p0.z; o0.w += p0.w;
          o1.x += p1.x; o1.y += p1.y; o1.z += p1.z; o1.w += p1.w;
        }
        *reinterpret_cast<float4*>(o) = o0;
        *reinterpret_cast<float4*>(o + 16) = o1;
        if (g == 0) st[2] = dsum;
      }
    }
  }
}

// ---- backward on the matrix cores, part 2 (keys): per frame the queries' scaled q, dx and statistics sit in LDS; a wave owns a
//      16-key tile and walks all query tiles:  S = Q K^T, dP = dX V^T (queries on the D rows: lane (key j, group g) holds queries
//      4 g + r),  dv^T += dX^T (P keep),  dk^T += (scale Q)^T dS  (4 x 2 MFMAs each, queries {4 g + r} per step).
__global__ __launch_bounds__(256) void tr_spatial_bwd_kv_mfma_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                      const float* __restrict__ v, const float* __restrict__ dx,
                                                                      const float* __restrict__ stats, float* __restrict__ dk,
                                                                      float* __restrict__ dv, RowMap rm, int T, int C, int heads, float scale,
                                                                      Drop dr, int Nc /* queries staged at a time: a multiple of 16 */) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int s = blockIdx.x / heads, h = blockIdx.x - s * heads, N = rm.N, L = rm.L;
  const int Np = (N + 15) & ~15, nkt = (L + 15) >> 4;
  const int nchunks = (Np + Nc - 1) / Nc;          // 1: the whole sequence's queries fit (the within-clip layer); more: 12+ clips of 128 queries
  float* qs = smem;                      // [Nc][kTrLd] scale * q
  float* gs = qs + Nc * kTrLd;           // [Nc][kTrLd] dx of the frame
  float* ss = gs + Nc * kTrLd;           // [Nc][4]     max, 1/sum, D of (query, frame)
  auto stage_q = [&](int c0) {           // scaled q rows c0 .. c0 + Nc
    for (int i = tid; i < Nc * 8; i += 256) {
      const int n = i >> 3, c4 = i & 7;
      float4 t = {0.f, 0.f, 0.f, 0.f};
      if (c0 + n < N) {
        t = *reinterpret_cast<const float4*>(q + nat_row(rm, s * N + c0 + n) * C + h * 32 + c4 * 4);
        t.x *= scale; t.y *= scale; t.z *= scale; t.w *= scale;
      }
      *reinterpret_cast<float4*>(qs + n * kTrLd + c4 * 4) = t;
    }
  };
  auto stage_frame = [&](int c0, int f) { // dx and the statistics of frame f for the same rows
    for (int i = tid; i < Nc * 8; i += 256) {
      const int n = i >> 3, c4 = i & 7;
      float4 t = {0.f, 0.f, 0.f, 0.f};
      if (c0 + n < N) t = *reinterpret_cast<const float4*>(dx + (nat_row(rm, s * N + c0 + n) * T + f) * C + h * 32 + c4 * 4);
      *reinterpret_cast<float4*>(gs + n * kTrLd + c4 * 4) = t;
    }
    for (int n = tid; n < Nc; n += 256) {
      const float* st = stats + ((((size_t)s * heads + h) * N + min(c0 + n, N - 1)) * T + f) * 3;
      // padding queries: 1/sum = 0 makes their probabilities vanish
      *reinterpret_cast<float4*>(ss + n * 4) = float4{st[0], c0 + n < N ? st[1] : 0.f, st[2], 0.f};
    }
  };
  if (nchunks == 1) stage_q(0);
  const int fper = (T + (int)gridDim.z - 1) / (int)gridDim.z, f0 = (int)blockIdx.z * fper, f1 = min(T, f0 + fper);   // as in the forward kernel
  const int iters = (nkt + 4 * (int)gridDim.y - 1) / (4 * (int)gridDim.y);   // key tiles per wave (uniform: every wave meets every barrier)
  for (int f = f0; f < f1; ++f) {
    if (nchunks == 1) {
      __syncthreads();
      stage_frame(0, f);
      __syncthreads();
    }
    for (int it = 0; it < iters; ++it) {
      const int kt = (it * (int)gridDim.y + (int)blockIdx.y) * 4 + wave;
      const bool have = kt < nkt;
      const int kn = kt * 16 + j, kc = min(kn, L - 1);                  // key index within the frame
      const long long mk = nat_row(rm, s * N + f * L + (have ? kc : 0));
      float kr[8], vr[8];
      {
        const float* kp = k + mk * C + h * 32 + 8 * g;
        const float* vp = v + mk * C + h * 32 + 8 * g;
        const float4 a = *reinterpret_cast<const float4*>(kp), b = *reinterpret_cast<const float4*>(kp + 4);
        const float4 c = *reinterpret_cast<const float4*>(vp), d = *reinterpret_cast<const float4*>(vp + 4);
        kr[0] = a.x; kr[1] = a.y; kr[2] = a.z; kr[3] = a.w; kr[4] = b.x; kr[5] = b.y; kr[6] = b.z; kr[7] = b.w;
        vr[0] = c.x; vr[1] = c.y; vr[2] = c.z; vr[3] = c.w; vr[4] = d.x; vr[5] = d.y; vr[6] = d.z; vr[7] = d.w;
      }
      f32x4 dka[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}}, dva[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      for (int ch = 0; ch < nchunks; ++ch) {
        const int c0 = ch * Nc;
        if (nchunks > 1) {                 // (the chunk order is the order of additions into dk / dv: fixed)
          __syncthreads();
          stage_q(c0);
          stage_frame(c0, f);
          __syncthreads();
        }
        const int nq_here = min(Nc, Np - c0) >> 4;
        if (have)
          for (int qt = 0; qt < nq_here; ++qt) {
            const float* qp = qs + (qt * 16 + j) * kTrLd + 8 * g;
            const float* gp = gs + (qt * 16 + j) * kTrLd + 8 * g;
            const float4 qa = *reinterpret_cast<const float4*>(qp), qb = *reinterpret_cast<const float4*>(qp + 4);
            const float4 ga = *reinterpret_cast<const float4*>(gp), gb = *reinterpret_cast<const float4*>(gp + 4);
            const float qr[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
            const float gr[8] = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y, gb.z, gb.w};
            f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 8; ++t) {                 // D[i = query 4 g' + r][j = key]: A = query rows, B = key rows
              sc = __builtin_amdgcn_mfma_f32_16x16x4f32(qr[t], kr[t], sc, 0, 0, 0);
              dp = __builtin_amdgcn_mfma_f32_16x16x4f32(gr[t], vr[t], dp, 0, 0, 0);
            }
            const int ql = qt * 16 + 4 * g;               // my 4 queries within the chunk: ql .. ql + 3 (global: c0 + ql ..)
            float pk[4], ds[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float4 st = *reinterpret_cast<const float4*>(ss + (ql + r) * 4);
              const float P = __expf(sc[r] - st.x) * st.y;
              const float kp_ = (c0 + ql + r < N && kn < L)
                                    ? drop_keep(dr, ((((unsigned long long)s * heads + h) * N + c0 + ql + r) * T + f) * L + kn) : 0.f;
              pk[r] = P * kp_;
              ds[r] = P * (kp_ * dp[r] - st.z);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float* gq = gs + (ql + r) * kTrLd + j;      // A: dx^T (resp. q^T) of query ql + r, channels j and 16 + j
              const float* qq = qs + (ql + r) * kTrLd + j;
              dva[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(gq[0], pk[r], dva[0], 0, 0, 0);
              dva[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(gq[16], pk[r], dva[1], 0, 0, 0);
              dka[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(qq[0], ds[r], dka[0], 0, 0, 0);
              dka[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(qq[16], ds[r], dka[1], 0, 0, 0);
            }
          }
      }
      if (have && kn < L) {                            // lane (key j, group g): channels dt * 16 + 4 g + r
        float* ok = dk + mk * C + h * 32 + 4 * g;
        float* ov = dv + mk * C + h * 32 + 4 * g;
        *reinterpret_cast<float4*>(ok) = float4{dka[0][0], dka[0][1], dka[0][2], dka[0][3]};
        *reinterpret_cast<float4*>(ok + 16) = float4{dka[1][0], dka[1][1], dka[1][2], dka[1][3]};
        *reinterpret_cast<float4*>(ov) = float4{dva[0][0], dva[0][1], dva[0][2], dva[0][3]};
        *reinterpret_cast<float4*>(ov + 16) = float4{dva[1][0], dva[1][1], dva[1][2], dva[1][3]};
      }
    }
  }
}

// ---- long frames (the full T*H*W layer: a frame is all H*W keys -- 4096 at 64 x 64): the same two query-side kernels with a
//      frame's keys staged kSpChunk at a time.  The forward's running max / sum per 16-key tile is the one of
//      tr_spatial_fwd_mfma_kernel (same tile order: the same statistics (max, 1 / sum) into `stats`, the same x layout), so the
//      key-side backward (tr_spatial_bwd_kv_mfma_kernel, which stages QUERIES in chunks and never holds a whole frame) serves
//      both.  A wave owns kSpQT query tiles at a time, so each K / V fragment read from LDS feeds kSpQT tiles.  LDS: K and V
//      chunks [kSpChunk][kTrLd] = 72 KiB (two workgroups per CU).  Dropout element indices are 64-bit (2.1e9 at 64 x 64 x 4).
constexpr int kSpChunk = 256;   // keys of a frame per LDS stage (a multiple of 16)
constexpr int kSpQT = 2;        // 16-query tiles per wave
__host__ __device__ inline size_t spatial_chunk_lds() { return (size_t)2 * kSpChunk * kTrLd * sizeof(float); }

// keys c0 .. c0 + ceil16(Lc) of frame f of (sequence s, head h) -> LDS [.][kTrLd], rows past the frame zero
__device__ __forceinline__ void stage_chunk36(float* dst, const float* src, const RowMap& rm, int s, int f, int c0, int h, int C, int tid) {
  const int Lc = min(kSpChunk, rm.L - c0), Lp = (Lc + 15) & ~15;
  for (int i = tid; i < Lp * 8; i += 256) {
    const int n = i >> 3, c4 = i & 7;
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (n < Lc) v = *reinterpret_cast<const float4*>(src + nat_row(rm, s * rm.N + f * rm.L + c0 + n) * C + h * 32 + c4 * 4);
    *reinterpret_cast<float4*>(dst + n * kTrLd + c4 * 4) = v;
  }
}

// grid: x = (sequence, head), y = blocks of 4 * kSpQT query tiles, z = frames (as tr_spatial_fwd_mfma_kernel)
__global__ __launch_bounds__(256) void tr_spatial_fwd_chunk_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                    const float* __restrict__ v, float* __restrict__ x,
                                                                    float* __restrict__ stats, RowMap rm, int T, int C, int heads, float scale,
                                                                    Drop dr) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int s = blockIdx.x / heads, h = blockIdx.x - s * heads, N = rm.N, L = rm.L;
  const int nqt = (N + 15) >> 4, nqb = (nqt + 4 * kSpQT - 1) / (4 * kSpQT);
  float* ks = smem;
  float* vs = smem + kSpChunk * kTrLd;
  const int fper = (T + (int)gridDim.z - 1) / (int)gridDim.z, f0 = (int)blockIdx.z * fper, f1 = min(T, f0 + fper);
  for (int f = f0; f < f1; ++f)
    for (int qb = (int)blockIdx.y; qb < nqb; qb += (int)gridDim.y) {
      float qr[kSpQT][8], m[kSpQT], sum[kSpQT];
      f32x4 acc[kSpQT][2];
      unsigned long long base[kSpQT];
#pragma unroll
      for (int u = 0; u < kSpQT; ++u) {
        const int qc = min((qb * 4 * kSpQT + u * 4 + wave) * 16 + j, N - 1);
        const float* qp = q + nat_row(rm, s * N + qc) * C + h * 32 + 8 * g;
        const float4 a = *reinterpret_cast<const float4*>(qp), b = *reinterpret_cast<const float4*>(qp + 4);
        qr[u][0] = a.x * scale; qr[u][1] = a.y * scale; qr[u][2] = a.z * scale; qr[u][3] = a.w * scale;
        qr[u][4] = b.x * scale; qr[u][5] = b.y * scale; qr[u][6] = b.z * scale; qr[u][7] = b.w * scale;
        m[u] = -INFINITY;
        sum[u] = 0.f;
        acc[u][0] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc[u][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        base[u] = ((((unsigned long long)s * heads + h) * N + qc) * T + f) * L;
      }
      for (int c0 = 0; c0 < L; c0 += kSpChunk) {
        __syncthreads();
        stage_chunk36(ks, k, rm, s, f, c0, h, C, tid);
        stage_chunk36(vs, v, rm, s, f, c0, h, C, tid);
        __syncthreads();
        const int nkt = (min(kSpChunk, L - c0) + 15) >> 4;
        for (int kt = 0; kt < nkt; ++kt) {
          const float* kp = ks + (kt * 16 + j) * kTrLd + 8 * g;
          const float4 ka = *reinterpret_cast<const float4*>(kp), kb = *reinterpret_cast<const float4*>(kp + 4);
          const float kr[8] = {ka.x, ka.y, ka.z, ka.w, kb.x, kb.y, kb.z, kb.w};
          const int nl = kt * 16 + 4 * g, n0 = c0 + nl;          // my 4 keys: n0 .. n0 + 3 of the frame (nl .. within the chunk)
          float vr[4][2];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            vr[r][0] = vs[(nl + r) * kTrLd + j];
            vr[r][1] = vs[(nl + r) * kTrLd + j + 16];
          }
#pragma unroll
          for (int u = 0; u < kSpQT; ++u) {
            if ((qb * 4 * kSpQT + u * 4 + wave) >= nqt) continue;      // (uniform per wave)
            f32x4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 8; ++t) sc = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[t], qr[u][t], sc, 0, 0, 0);
            float tmax = -INFINITY;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              if (n0 + r >= L) sc[r] = -INFINITY;
              tmax = fmaxf(tmax, sc[r]);
            }
            const float mn = fmaxf(m[u], xor_max16_32(tmax));
            const float alpha = __expf(m[u] - mn);
            float p[4], ps = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              p[r] = __expf(sc[r] - mn);
              ps += p[r];
              if (n0 + r < L) p[r] *= drop_keep(dr, base[u] + n0 + r);
            }
            sum[u] = sum[u] * alpha + xor_sum16_32(ps);
            m[u] = mn;
            acc[u][0] *= alpha;
            acc[u][1] *= alpha;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              acc[u][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[r][0], p[r], acc[u][0], 0, 0, 0);
              acc[u][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[r][1], p[r], acc[u][1], 0, 0, 0);
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kSpQT; ++u) {
        const int qn = (qb * 4 * kSpQT + u * 4 + wave) * 16 + j;
        if (qn < N) {
          const long long mq = nat_row(rm, s * N + qn);
          const float inv = 1.f / sum[u];
          float* xo = x + (mq * T + f) * C + h * 32 + 4 * g;
          *reinterpret_cast<float4*>(xo) = float4{acc[u][0][0] * inv, acc[u][0][1] * inv, acc[u][0][2] * inv, acc[u][0][3] * inv};
          *reinterpret_cast<float4*>(xo + 16) = float4{acc[u][1][0] * inv, acc[u][1][1] * inv, acc[u][1][2] * inv, acc[u][1][3] * inv};
          if (g == 0) {
            float* st = stats + ((((size_t)s * heads + h) * N + qn) * T + f) * 3;
            st[0] = m[u];
            st[1] = inv;
          }
        }
      }
    }
}

// backward, query side (tr_spatial_bwd_q_mfma_kernel with chunked keys): per (query, frame) D = dx . x, then per 16-key tile
// S^T = K Q^T, dP^T = V dX^T, dS = P (keep dP - D) with P from the forward's (max, 1 / sum), dq^T += K^T dS^T.  dq stays in
// registers over all frames and chunks (one store); D goes to stats[.., 2] for the key side.  grid: x = (sequence, head),
// y = blocks of 4 * kSpQT query tiles.
__global__ __launch_bounds__(256) void tr_spatial_bwd_q_chunk_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                      const float* __restrict__ v, const float* __restrict__ x,
                                                                      const float* __restrict__ dx, float* __restrict__ dq,
                                                                      float* __restrict__ stats, RowMap rm, int T, int C, int heads, float scale,
                                                                      Drop dr) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int s = blockIdx.x / heads, h = blockIdx.x - s * heads, N = rm.N, L = rm.L;
  const int nqt = (N + 15) >> 4, nqb = (nqt + 4 * kSpQT - 1) / (4 * kSpQT);
  float* ks = smem;
  float* vs = smem + kSpChunk * kTrLd;
  for (int qb = (int)blockIdx.y; qb < nqb; qb += (int)gridDim.y) {
    float qr[kSpQT][8];
    long long mq[kSpQT];
    int qc[kSpQT];
    f32x4 acc[kSpQT][2];
#pragma unroll
    for (int u = 0; u < kSpQT; ++u) {
      qc[u] = min((qb * 4 * kSpQT + u * 4 + wave) * 16 + j, N - 1);
      mq[u] = nat_row(rm, s * N + qc[u]);
      const float* qp = q + mq[u] * C + h * 32 + 8 * g;
      const float4 a = *reinterpret_cast<const float4*>(qp), b = *reinterpret_cast<const float4*>(qp + 4);
      qr[u][0] = a.x * scale; qr[u][1] = a.y * scale; qr[u][2] = a.z * scale; qr[u][3] = a.w * scale;
      qr[u][4] = b.x * scale; qr[u][5] = b.y * scale; qr[u][6] = b.z * scale; qr[u][7] = b.w * scale;
      acc[u][0] = f32x4{0.f, 0.f, 0.f, 0.f};
      acc[u][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int f = 0; f < T; ++f) {
      float dxr[kSpQT][8], dsum[kSpQT], m[kSpQT], inv[kSpQT];
      unsigned long long base[kSpQT];
#pragma unroll
      for (int u = 0; u < kSpQT; ++u) {
        const float* gp = dx + (mq[u] * T + f) * C + h * 32 + 8 * g;
        const float* xp = x + (mq[u] * T + f) * C + h * 32 + 8 * g;
        const float4 c = *reinterpret_cast<const float4*>(gp), d = *reinterpret_cast<const float4*>(gp + 4);
        const float4 e = *reinterpret_cast<const float4*>(xp), e2 = *reinterpret_cast<const float4*>(xp + 4);
        dxr[u][0] = c.x; dxr[u][1] = c.y; dxr[u][2] = c.z; dxr[u][3] = c.w; dxr[u][4] = d.x; dxr[u][5] = d.y; dxr[u][6] = d.z; dxr[u][7] = d.w;
        dsum[u] = xor_sum16_32(c.x * e.x + c.y * e.y + c.z * e.z + c.w * e.w + d.x * e2.x + d.y * e2.y + d.z * e2.z + d.w * e2.w);
        const float* st = stats + ((((size_t)s * heads + h) * N + qc[u]) * T + f) * 3;
        m[u] = st[0];
        inv[u] = st[1];
        base[u] = ((((unsigned long long)s * heads + h) * N + qc[u]) * T + f) * L;
      }
      for (int c0 = 0; c0 < L; c0 += kSpChunk) {
        __syncthreads();
        stage_chunk36(ks, k, rm, s, f, c0, h, C, tid);
        stage_chunk36(vs, v, rm, s, f, c0, h, C, tid);
        __syncthreads();
        const int nkt = (min(kSpChunk, L - c0) + 15) >> 4;
        for (int kt = 0; kt < nkt; ++kt) {
          const float* kp = ks + (kt * 16 + j) * kTrLd + 8 * g;
          const float* vp = vs + (kt * 16 + j) * kTrLd + 8 * g;
          const float4 ka = *reinterpret_cast<const float4*>(kp), kb = *reinterpret_cast<const float4*>(kp + 4);
          const float4 va = *reinterpret_cast<const float4*>(vp), vb = *reinterpret_cast<const float4*>(vp + 4);
          const float kr[8] = {ka.x, ka.y, ka.z, ka.w, kb.x, kb.y, kb.z, kb.w};
          const float vr[8] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w};
          const int nl = kt * 16 + 4 * g, n0 = c0 + nl;
          float kt_[4][2];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            kt_[r][0] = ks[(nl + r) * kTrLd + j];
            kt_[r][1] = ks[(nl + r) * kTrLd + j + 16];
          }
#pragma unroll
          for (int u = 0; u < kSpQT; ++u) {
            if ((qb * 4 * kSpQT + u * 4 + wave) >= nqt) continue;      // (uniform per wave)
            f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 8; ++t) {
              sc = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[t], qr[u][t], sc, 0, 0, 0);
              dp = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[t], dxr[u][t], dp, 0, 0, 0);
            }
            float ds[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const bool valid = n0 + r < L;
              const float P = valid ? __expf(sc[r] - m[u]) * inv[u] : 0.f;
              const float kp_ = valid ? drop_keep(dr, base[u] + n0 + r) : 0.f;
              ds[r] = P * (kp_ * dp[r] - dsum[u]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              acc[u][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(kt_[r][0], ds[r], acc[u][0], 0, 0, 0);
              acc[u][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(kt_[r][1], ds[r], acc[u][1], 0, 0, 0);
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kSpQT; ++u)
        if (g == 0 && (qb * 4 * kSpQT + u * 4 + wave) * 16 + j < N) stats[((((size_t)s * heads + h) * N + qc[u]) * T + f) * 3 + 2] = dsum[u];
    }
#pragma unroll
    for (int u = 0; u < kSpQT; ++u) {
      if ((qb * 4 * kSpQT + u * 4 + wave) * 16 + j >= N) continue;
      float* o = dq + mq[u] * C + h * 32 + 4 * g;
      *reinterpret_cast<float4*>(o) = float4{acc[u][0][0] * scale, acc[u][0][1] * scale, acc[u][0][2] * scale, acc[u][0][3] * scale};
      *reinterpret_cast<float4*>(o + 16) = float4{acc[u][1][0] * scale, acc[u][1][1] * scale, acc[u][1][2] * scale, acc[u][1][3] * scale};
    }
  }
}

// ---- spatial half, backward, part 1 (one thread per query): the softmax statistics (max, 1/sum, D = sum_n P dP) of every
//      (query, frame) and dq.  dP_n = keep_n (dx_f . v_n),  dS_n = P_n (dP_n - D),  dq = scale sum_{f,n} dS_n k_n.
//      stats: [(s heads + h), N, T, 3].
template <int D>
__global__ __launch_bounds__(256) void tr_spatial_bwd_q_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                const float* __restrict__ v, const float* __restrict__ dx,
                                                                float* __restrict__ dq, float* __restrict__ stats, RowMap rm, int T, int C,
                                                                int heads, float scale, Drop dr) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x, s = blockIdx.x / heads, h = blockIdx.x - s * heads, N = rm.N, L = rm.L;
  float* ks = smem;
  float* vs = smem + L * D;
  for (int q0 = 0; q0 < N; q0 += 256) {
    const int qn = q0 + tid;
    const bool act = qn < N;
    const long long mq = nat_row(rm, s * N + (act ? qn : 0));
    float qr[D], dqr[D];
    load_row<D>(qr, q + mq * C + h * D);
#pragma unroll
    for (int i = 0; i < D; ++i) {
      qr[i] *= scale;
      dqr[i] = 0.f;
    }
    for (int f = 0; f < T; ++f) {
      __syncthreads();
      stage_frame<D>(ks, k, rm, s, f, h, C, tid);
      stage_frame<D>(vs, v, rm, s, f, h, C, tid);
      __syncthreads();
      if (!act) continue;
      float dxr[D];
      load_row<D>(dxr, dx + (mq * T + f) * C + h * D);
      float mx = -INFINITY;
      for (int n = 0; n < L; ++n) mx = fmaxf(mx, dot_lds<D>(qr, ks + n * D));
      const unsigned long long base = ((((unsigned long long)s * heads + h) * N + qn) * T + f) * L;
      float sum = 0.f, pd = 0.f;
      for (int n = 0; n < L; ++n) {
        const float p = __expf(dot_lds<D>(qr, ks + n * D) - mx);
        sum += p;
        const float kp = drop_keep(dr, base + n);
        if (kp != 0.f) pd += p * kp * dot_lds<D>(dxr, vs + n * D);
      }
      const float inv = 1.f / sum, Dsum = pd * inv;
      for (int n = 0; n < L; ++n) {
        const float P = __expf(dot_lds<D>(qr, ks + n * D) - mx) * inv;
        const float kp = drop_keep(dr, base + n);
        const float dP = kp != 0.f ? kp * dot_lds<D>(dxr, vs + n * D) : 0.f;
        axpy_lds<D>(dqr, P * (dP - Dsum), ks + n * D);
      }
      float* st = stats + ((((size_t)s * heads + h) * N + qn) * T + f) * 3;
      st[0] = mx;
      st[1] = inv;
      st[2] = Dsum;
    }
    if (act) {
#pragma unroll
      for (int i = 0; i < D; ++i) dqr[i] *= scale;
      store_row<D>(dq + mq * C + h * D, dqr);
    }
  }
}

// ---- spatial half, backward, part 2 (one thread per key): dk = scale sum_q dS q,  dv = sum_q keep P dx_f, with P rebuilt from
//      the statistics of part 1.  Queries are staged QC at a time (scaled q, dx of all T frames, statistics).
template <int D>
__global__ __launch_bounds__(256) void tr_spatial_bwd_kv_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                 const float* __restrict__ v, const float* __restrict__ dx,
                                                                 const float* __restrict__ stats, float* __restrict__ dk,
                                                                 float* __restrict__ dv, RowMap rm, int T, int C, int heads, float scale,
                                                                 Drop dr, int QC) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x, s = blockIdx.x / heads, h = blockIdx.x - s * heads, N = rm.N, L = rm.L;
  float* qs = smem;                  // [QC][D]
  float* dxs = qs + QC * D;          // [QC][T][D]
  float* sts = dxs + QC * T * D;     // [QC][T][3]
  constexpr int V = D / 4;
  for (int k0 = 0; k0 < N; k0 += 256) {
    const int kn = k0 + tid;
    const bool act = kn < N;
    const int f = act ? kn / L : 0, n = act ? kn - f * L : 0;
    const long long mk = nat_row(rm, s * N + (act ? kn : 0));
    float kr[D], vr[D], dkr[D], dvr[D];
    load_row<D>(kr, k + mk * C + h * D);
    load_row<D>(vr, v + mk * C + h * D);
#pragma unroll
    for (int i = 0; i < D; ++i) dkr[i] = dvr[i] = 0.f;
    for (int q0 = 0; q0 < N; q0 += QC) {
      const int nq = min(QC, N - q0);
      __syncthreads();
      for (int i = tid; i < nq * V; i += 256) {
        const int qi = i / V, c4 = i - qi * V;
        const long long mq = nat_row(rm, s * N + q0 + qi);
        float4 t = *reinterpret_cast<const float4*>(q + mq * C + h * D + c4 * 4);
        t.x *= scale; t.y *= scale; t.z *= scale; t.w *= scale;
        *reinterpret_cast<float4*>(qs + qi * D + c4 * 4) = t;
      }
      for (int i = tid; i < nq * T * V; i += 256) {
        const int qi = i / (T * V), r = i - qi * (T * V), ff = r / V, c4 = r - ff * V;
        const long long mq = nat_row(rm, s * N + q0 + qi);
        *reinterpret_cast<float4*>(dxs + (qi * T + ff) * D + c4 * 4) = *reinterpret_cast<const float4*>(dx + (mq * T + ff) * C + h * D + c4 * 4);
      }
      for (int i = tid; i < nq * T * 3; i += 256) sts[i] = stats[((((size_t)s * heads + h) * N + q0) * T) * 3 + i];
      __syncthreads();
      if (!act) continue;
      for (int qi = 0; qi < nq; ++qi) {
        const float* st = sts + (qi * T + f) * 3;
        const float P = __expf(dot_lds<D>(kr, qs + qi * D) - st[0]) * st[1];
        const float kp = drop_keep(dr, ((((unsigned long long)s * heads + h) * N + q0 + qi) * T + f) * L + n);
        const float* dxr = dxs + (qi * T + f) * D;
        const float dP = kp != 0.f ? kp * dot_lds<D>(vr, dxr) : 0.f;
        axpy_lds<D>(dkr, P * (dP - st[2]), qs + qi * D);      // qs is scale * q: the factor `scale` of dk rides along
        if (kp != 0.f) axpy_lds<D>(dvr, P * kp, dxr);
      }
    }
    if (act) {
      store_row<D>(dk + mk * C + h * D, dkr);
      store_row<D>(dv + mk * C + h * D, dvr);
    }
  }
}

// ---- temporal half (WC/temporal_attention.py:69-73), one thread per (token, head):
//      logits_f = q2 . k2_f, a = softmax_f, o = sum_f a_f v2_f.   q2 [M,C] (already scaled), kv2 [M*T, 2C] = (k2 | v2), T <= TMAX (8: the clips of the within-clip layer; 16: the cross-clip module walks up to 16 clips).
template <int D, int TMAX>
__global__ __launch_bounds__(256) void tr_temporal_fwd_kernel(const float* __restrict__ q2, const float* __restrict__ kv2,
                                                               float* __restrict__ o, long long M, int T, int C, int heads) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * heads) return;
  const long long m = i / heads;
  const int h = (int)(i - m * heads);
  float qr[D], acc[D], lg[TMAX];
  load_row<D>(qr, q2 + m * C + h * D);
  float mx = -INFINITY;
#pragma unroll
  for (int f = 0; f < TMAX; ++f)
    if (f < T) {
      float kr[D];
      load_row<D>(kr, kv2 + (m * T + f) * 2 * C + h * D);
      float a = 0.f;
#pragma unroll
      for (int c = 0; c < D; ++c) a += qr[c] * kr[c];
      lg[f] = a;
      mx = fmaxf(mx, a);
    }
  float sum = 0.f;
#pragma unroll
  for (int f = 0; f < TMAX; ++f)
    if (f < T) {
      lg[f] = __expf(lg[f] - mx);
      sum += lg[f];
    }
  const float inv = 1.f / sum;
#pragma unroll
  for (int c = 0; c < D; ++c) acc[c] = 0.f;
#pragma unroll
  for (int f = 0; f < TMAX; ++f)
    if (f < T) {
      float vr[D];
      load_row<D>(vr, kv2 + (m * T + f) * 2 * C + C + h * D);
      const float a = lg[f] * inv;
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] += a * vr[c];
    }
  store_row<D>(o + m * C + h * D, acc);
}

// backward: d_o -> dq2 [M,C], dkv2 [M*T, 2C]
template <int D, int TMAX>
__global__ __launch_bounds__(256) void tr_temporal_bwd_kernel(const float* __restrict__ q2, const float* __restrict__ kv2,
                                                               const float* __restrict__ d_o, float* __restrict__ dq2,
                                                               float* __restrict__ dkv2, long long M, int T, int C, int heads) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * heads) return;
  const long long m = i / heads;
  const int h = (int)(i - m * heads);
  float qr[D], gr[D], lg[TMAX], da[TMAX];
  load_row<D>(qr, q2 + m * C + h * D);
  load_row<D>(gr, d_o + m * C + h * D);
  float mx = -INFINITY;
#pragma unroll
  for (int f = 0; f < TMAX; ++f)
    if (f < T) {
      float kr[D], vr[D];
      load_row<D>(kr, kv2 + (m * T + f) * 2 * C + h * D);
      load_row<D>(vr, kv2 + (m * T + f) * 2 * C + C + h * D);
      float a = 0.f, b = 0.f;
#pragma unroll
      for (int c = 0; c < D; ++c) {
        a += qr[c] * kr[c];
        b += gr[c] * vr[c];
      }
      lg[f] = a;
      da[f] = b;
      mx = fmaxf(mx, a);
    }
  float sum = 0.f;
#pragma unroll
  for (int f = 0; f < TMAX; ++f)
    if (f < T) {
      lg[f] = __expf(lg[f] - mx);
      sum += lg[f];
    }
  const float inv = 1.f / sum;
  float dot = 0.f;
#pragma unroll
  for (int f = 0; f < TMAX; ++f)
    if (f < T) {
      lg[f] *= inv;
      dot += lg[f] * da[f];
    }
  float dqr[D];
#pragma unroll
  for (int c = 0; c < D; ++c) dqr[c] = 0.f;
#pragma unroll
  for (int f = 0; f < TMAX; ++f)
    if (f < T) {
      const float dl = lg[f] * (da[f] - dot);
      float kr[D], t0[D], t1[D];
      load_row<D>(kr, kv2 + (m * T + f) * 2 * C + h * D);
#pragma unroll
      for (int c = 0; c < D; ++c) {
        dqr[c] += dl * kr[c];
        t0[c] = dl * qr[c];
        t1[c] = lg[f] * gr[c];
      }
      store_row<D>(dkv2 + (m * T + f) * 2 * C + h * D, t0);
      store_row<D>(dkv2 + (m * T + f) * 2 * C + C + h * D, t1);
    }
  store_row<D>(dq2 + m * C + h * D, dqr);
}

// ---- LayerNorm over the channel dimension, one wave per row; eps 1e-5 for nn.LayerNorm (WC/temporal_attention.py:167,175),
//      1e-6 for the channels-first LayerNorm of the cross-clip ASPP
__device__ __forceinline__ float wave_total(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void tr_ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b,
                                                         float* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd,
                                                         long long M, int C, float eps) {
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= M) return;
  const float* xr = x + r * C;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += xr[c];
  const float mu = wave_total(s) / C;
  float vs = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float d = xr[c] - mu;
    vs += d * d;
  }
  const float rs = rsqrtf(wave_total(vs) / C + eps);
  for (int c = lane; c < C; c += 64) y[r * C + c] = (xr[c] - mu) * rs * g[c] + b[c];
  if (lane == 0) {
    mean[r] = mu;
    rstd[r] = rs;
  }
}

// dx = rstd (g dy - mean_c(g dy) - xhat mean_c(g dy xhat))
__global__ __launch_bounds__(256) void tr_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ g,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         float* __restrict__ dx, long long M, int C) {
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= M) return;
  const float mu = mean[r], rs = rstd[r];
  float a = 0.f, b = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float w = dy[r * C + c] * g[c], xh = (x[r * C + c] - mu) * rs;
    a += w;
    b += w * xh;
  }
  a = wave_total(a) / C;
  b = wave_total(b) / C;
  for (int c = lane; c < C; c += 64) {
    const float w = dy[r * C + c] * g[c], xh = (x[r * C + c] - mu) * rs;
    dx[r * C + c] = rs * (w - a - xh * b);
  }
}

// ---- column sums over rows (bias / LayerNorm parameter gradients), two deterministic stages.
//      stage 1: a block sums `rows_per_blk` rows; its 256 threads are `lanes` float4 columns x 256 / lanes row groups, reduced
//      through LDS:  part_a[blk][c] = sum_r dy[r][c];  with x: part_b[blk][c] = sum_r dy[r][c] * xhat[r][c]
__global__ __launch_bounds__(256) void tr_colsum_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, float* __restrict__ part_a,
                                                         float* __restrict__ part_b, long long M, int C, int rows_per_blk) {
  __shared__ float4 red[2][256];
  const int n4 = C / 4, lanes = n4 < 256 ? n4 : 256, rg = 256 / lanes;
  const int col = threadIdx.x % lanes, g = threadIdx.x / lanes;
  const long long r0 = (long long)blockIdx.x * rows_per_blk;
  const long long r1 = r0 + rows_per_blk < M ? r0 + rows_per_blk : M;
  for (int c0 = 0; c0 < n4; c0 += lanes) {        // (more than one trip only when C > 1024; uniform trip count: barriers inside)
    const int c4 = c0 + col;
    const bool valid = c4 < n4;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (g < rg && valid) {
      for (long long r = r0 + g; r < r1; r += rg) {
        const float4 d = *reinterpret_cast<const float4*>(dy + r * C + c4 * 4);
        a.x += d.x; a.y += d.y; a.z += d.z; a.w += d.w;
        if (x) {
          const float4 xv = *reinterpret_cast<const float4*>(x + r * C + c4 * 4);
          const float mu = mean[r], rs = rstd[r];
          b.x += d.x * (xv.x - mu) * rs; b.y += d.y * (xv.y - mu) * rs; b.z += d.z * (xv.z - mu) * rs; b.w += d.w * (xv.w - mu) * rs;
        }
      }
    }
    __syncthreads();
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    if (g == 0 && valid) {
      for (int j = 1; j < rg; ++j) {
        const float4 u = red[0][j * lanes + col], w = red[1][j * lanes + col];
        a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w;
        b.x += w.x; b.y += w.y; b.z += w.z; b.w += w.w;
      }
      *reinterpret_cast<float4*>(part_a + (size_t)blockIdx.x * C + c4 * 4) = a;
      if (x) *reinterpret_cast<float4*>(part_b + (size_t)blockIdx.x * C + c4 * 4) = b;
    }
  }
}

// stage 2 (also the reduction of split-K weight-gradient partials): out[c] = sum_i part[i][c].  A block = 64 float4 columns x 4
// partial groups (1 KiB contiguous per wave and partial row), joined through LDS in a fixed order; C % 4 == 0.
__global__ __launch_bounds__(256) void tr_colsum_final_kernel(const float* __restrict__ part, int nblk, size_t C, float* __restrict__ out,
                                                               float mul = 1.f) {
  __shared__ float4 red[256];
  const size_t c4 = (size_t)blockIdx.x * 64 + (threadIdx.x & 63), n4 = C / 4;
  const int g = threadIdx.x >> 6;
  float4 a = {0.f, 0.f, 0.f, 0.f};
  if (c4 < n4) {
#pragma unroll 4
    for (int i = g; i < nblk; i += 4) {
      const float4 v = *reinterpret_cast<const float4*>(part + (size_t)i * C + c4 * 4);
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
  }
  red[threadIdx.x] = a;
  __syncthreads();
  if (g == 0 && c4 < n4) {
    const float4 b = red[threadIdx.x + 64], c = red[threadIdx.x + 128], d = red[threadIdx.x + 192];
    *reinterpret_cast<float4*>(out + c4 * 4) =
        float4{(a.x + b.x + c.x + d.x) * mul, (a.y + b.y + c.y + d.y) * mul, (a.z + b.z + c.z + d.z) * mul, (a.w + b.w + c.w + d.w) * mul};
  }
}

// the same for TWO partial sets in one launch (a weight gradient and its bias gradient): blocks [0, blocks_a) reduce set a, the rest set b
__global__ __launch_bounds__(256) void tr_colsum_final_pair_kernel(const float* __restrict__ part_a, size_t Ca, float* __restrict__ out_a,
                                                                    const float* __restrict__ part_b, size_t Cb, float* __restrict__ out_b,
                                                                    int nblk, int blocks_a, float mul = 1.f) {
  __shared__ float4 red[256];
  const bool second = (int)blockIdx.x >= blocks_a;
  const float* part = second ? part_b : part_a;
  const size_t C = second ? Cb : Ca;
  float* out = second ? out_b : out_a;
  const size_t c4 = (size_t)(second ? blockIdx.x - blocks_a : blockIdx.x) * 64 + (threadIdx.x & 63), n4 = C / 4;
  const int g = threadIdx.x >> 6;
  float4 a = {0.f, 0.f, 0.f, 0.f};
  if (c4 < n4) {
#pragma unroll 4
    for (int i = g; i < nblk; i += 4) {
      const float4 v = *reinterpret_cast<const float4*>(part + (size_t)i * C + c4 * 4);
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
  }
  red[threadIdx.x] = a;
  __syncthreads();
  if (g == 0 && c4 < n4) {
    const float4 b = red[threadIdx.x + 64], c = red[threadIdx.x + 128], d = red[threadIdx.x + 192];
    *reinterpret_cast<float4*>(out + c4 * 4) =
        float4{(a.x + b.x + c.x + d.x) * mul, (a.y + b.y + c.y + d.y) * mul, (a.z + b.z + c.z + d.z) * mul, (a.w + b.w + c.w + d.w) * mul};
  }
}

// Wt[K][N] = W[N][K]^T (32 x 32 tiles through LDS): the input-gradient GEMMs then run in the same (fast) form as the forward ones
__global__ __launch_bounds__(256) void tr_transpose_kernel(const float* __restrict__ w, float* __restrict__ wt, int N, int K) {
  __shared__ float tile[32][33];
  const int k0 = blockIdx.x * 32, n0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int j = ty; j < 32; j += 8)
    if (n0 + j < N && k0 + tx < K) tile[j][tx] = w[(size_t)(n0 + j) * K + k0 + tx];
  __syncthreads();
  for (int j = ty; j < 32; j += 8)
    if (k0 + j < K && n0 + tx < N) wt[(size_t)(k0 + j) * N + n0 + tx] = tile[tx][j];
}

// ---- elementwise pieces -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tr_add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y, size_t n4) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 u = reinterpret_cast<const float4*>(a)[i], w = reinterpret_cast<const float4*>(b)[i];
  reinterpret_cast<float4*>(y)[i] = make_float4(u.x + w.x, u.y + w.y, u.z + w.z, u.w + w.w);
}

// y = relu?((y + bias) * mul), then dropout by element index r * N + c (site: dropout2 of the FFN)
__global__ __launch_bounds__(256) void tr_bias_act_kernel(float* __restrict__ y, const float* __restrict__ bias, long long M, int N, float mul,
                                                           int relu, Drop dr) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;   // float4 index
  const int n4 = N / 4;
  if (i >= (size_t)M * n4) return;
  const int c = (int)(i % n4) * 4;
  float4 v = reinterpret_cast<float4*>(y)[i];
  const float4 b = *reinterpret_cast<const float4*>(bias + c);
  float t[4] = {(v.x + b.x) * mul, (v.y + b.y) * mul, (v.z + b.z) * mul, (v.w + b.w) * mul};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (relu) t[e] = fmaxf(t[e], 0.f);
    t[e] *= drop_keep(dr, (unsigned long long)i * 4 + e);
  }
  reinterpret_cast<float4*>(y)[i] = make_float4(t[0], t[1], t[2], t[3]);
}

// out[row] = res[row] + drop(y[row] + bias), rows visited in SEQUENCE order mp (row = nat_row(rm, mp)): the dropout index of the
// reference's [(B Loff), (T L), C] tensor is mp * C + c.  With rm = identity this is the FFN's dropout3 + residual.
__global__ __launch_bounds__(256) void tr_bias_drop_res_kernel(const float* __restrict__ y, const float* __restrict__ bias,
                                                                const float* __restrict__ res, float* __restrict__ out, RowMap rm, long long M,
                                                                int C, Drop dr) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int n4 = C / 4;
  if (i >= (size_t)M * n4) return;
  const long long mp = (long long)(i / n4);
  const int c = (int)(i - (size_t)mp * n4) * 4;
  const long long row = nat_row(rm, (int)mp);
  const float4 v = *reinterpret_cast<const float4*>(y + row * C + c), b = *reinterpret_cast<const float4*>(bias + c);
  const float4 r = *reinterpret_cast<const float4*>(res + row * C + c);
  const unsigned long long e = (unsigned long long)mp * C + c;
  *reinterpret_cast<float4*>(out + row * C + c) =
      make_float4(r.x + (v.x + b.x) * drop_keep(dr, e), r.y + (v.y + b.y) * drop_keep(dr, e + 1), r.z + (v.z + b.z) * drop_keep(dr, e + 2),
                  r.w + (v.w + b.w) * drop_keep(dr, e + 3));
}

// dy[row] = keep * dout[row]  (same indexing as tr_bias_drop_res_kernel)
__global__ __launch_bounds__(256) void tr_drop_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dy, RowMap rm, long long M, int C,
                                                           Drop dr) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int n4 = C / 4;
  if (i >= (size_t)M * n4) return;
  const long long mp = (long long)(i / n4);
  const int c = (int)(i - (size_t)mp * n4) * 4;
  const long long row = nat_row(rm, (int)mp);
  const float4 v = *reinterpret_cast<const float4*>(dout + row * C + c);
  const unsigned long long e = (unsigned long long)mp * C + c;
  *reinterpret_cast<float4*>(dy + row * C + c) =
      make_float4(v.x * drop_keep(dr, e), v.y * drop_keep(dr, e + 1), v.z * drop_keep(dr, e + 2), v.w * drop_keep(dr, e + 3));
}

// r = dropout2(relu(h)) was stored: d_h = (r > 0) ? scale * d_r : 0   (a dropped or clipped element has r == 0 and no gradient)
__global__ __launch_bounds__(256) void tr_relu_drop_bwd_kernel(float* __restrict__ dr_, const float* __restrict__ r, size_t n4, float scale) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  float4 d = reinterpret_cast<float4*>(dr_)[i];
  const float4 a = reinterpret_cast<const float4*>(r)[i];
  d.x = a.x > 0.f ? d.x * scale : 0.f;
  d.y = a.y > 0.f ? d.y * scale : 0.f;
  d.z = a.z > 0.f ? d.z * scale : 0.f;
  d.w = a.w > 0.f ? d.w * scale : 0.f;
  reinterpret_cast<float4*>(dr_)[i] = d;
}

// xd[m] = x[m, t(m)], t(m) = (m / HW) % T: the own-frame slot of every token (torch.diagonal, WC/temporal_attention.py:62-64)
__global__ __launch_bounds__(256) void tr_diag_gather_kernel(const float* __restrict__ x, float* __restrict__ xd, long long M, int T, long long HW,
                                                              int C) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int n4 = C / 4;
  if (i >= (size_t)M * n4) return;
  const long long m = (long long)(i / n4);
  const int c4 = (int)(i - (size_t)m * n4);
  const int t = (int)((m / HW) % T);
  reinterpret_cast<float4*>(xd)[i] = reinterpret_cast<const float4*>(x)[((size_t)m * T + t) * n4 + c4];
}

// dx[m, t(m)] += mul * dxd[m]
__global__ __launch_bounds__(256) void tr_diag_scatter_add_kernel(float* __restrict__ dx, const float* __restrict__ dxd, long long M, int T,
                                                                   long long HW, int C) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int n4 = C / 4;
  if (i >= (size_t)M * n4) return;
  const long long m = (long long)(i / n4);
  const int c4 = (int)(i - (size_t)m * n4);
  const int t = (int)((m / HW) % T);
  float4* p = reinterpret_cast<float4*>(dx) + ((size_t)m * T + t) * n4 + c4;
  const float4 a = *p, b = reinterpret_cast<const float4*>(dxd)[i];
  *p = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

__global__ __launch_bounds__(256) void tr_scale_kernel(float* __restrict__ y, size_t n4, float mul) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  float4 v = reinterpret_cast<float4*>(y)[i];
  v.x *= mul; v.y *= mul; v.z *= mul; v.w *= mul;
  reinterpret_cast<float4*>(y)[i] = v;
}

// ---- the deformable encoder layer (MSDeformAttnTransformerEncoderLayer, WC/msdeformattn.py:177-216): the sampling head of its
//      attention (OPS/modules/ms_deform_attn.py:98-117) around the fp32 core op of the inference library ------------------------------
constexpr int kMdMaxLevels = 8;   // = the core op's level bound
constexpr int kMdMaxLP = 32;      // n_levels * n_points: one thread holds a (row, head)'s logits in registers

struct MdLevels {
  float w[kMdMaxLevels], h[kMdMaxLevels];   // W_l, H_l (the offsets of 2-dim reference points are in pixels of their level)
  int L, P;
};

// rows flagged in `mask` (one byte per row, non-zero = padded key) are zeroed: value_proj(src).masked_fill (:99-100) and its gradient
__global__ __launch_bounds__(256) void md_zero_rows_kernel(float* __restrict__ x, const unsigned char* __restrict__ mask, long long M, int C) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int n4 = C / 4;
  if (i >= (size_t)M * n4) return;
  if (mask[i / n4]) reinterpret_cast<float4*>(x)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// sampling head, forward: one thread per (query row r, head m).  offlog [rows][heads L P 2 | heads L P]: the fused GEMM of the
// sampling_offsets and attention_weights Linears.  aw [rows][heads][L P] = softmax of the row's L P logits (:103-104);
// loc [rows][heads][L][P][2] = ref + off / (W_l, H_l) (2-dim points, :107-109) or ref[:2] + off / P * ref[2:] * 0.5 (boxes, :110-113)
__global__ __launch_bounds__(256) void md_head_fwd_kernel(const float* __restrict__ offlog, const float* __restrict__ ref, int ref_dim,
                                                         float* __restrict__ loc, float* __restrict__ aw, long long rows, int heads, MdLevels lv) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * heads) return;
  const long long r = i / heads;
  const int m = (int)(i - r * heads);
  const int L = lv.L, P = lv.P, LP = L * P;
  const long long NO = (long long)heads * LP * 3;
  const float* const lg = offlog + r * NO + (long long)heads * LP * 2 + (long long)m * LP;
  float e[kMdMaxLP];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < kMdMaxLP; ++j)
    if (j < LP) {
      e[j] = lg[j];
      mx = fmaxf(mx, e[j]);
    }
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < kMdMaxLP; ++j)
    if (j < LP) {
      e[j] = expf(e[j] - mx);
      sum += e[j];
    }
  const float inv = 1.f / sum;
  float* const a = aw + i * LP;
#pragma unroll
  for (int j = 0; j < kMdMaxLP; ++j)
    if (j < LP) a[j] = e[j] * inv;
  const float* const of = offlog + r * NO + (long long)m * LP * 2;
  const float* const rp = ref + r * L * ref_dim;
  float* const lo = loc + i * LP * 2;
  for (int l = 0; l < L; ++l) {
    const float rx = rp[l * ref_dim], ry = rp[l * ref_dim + 1];
    for (int p = 0; p < P; ++p) {
      const int j = l * P + p;
      const float ox = of[2 * j], oy = of[2 * j + 1];
      if (ref_dim == 2) {
        lo[2 * j] = rx + ox / lv.w[l];
        lo[2 * j + 1] = ry + oy / lv.h[l];
      } else {
        lo[2 * j] = rx + ox / (float)P * rp[l * 4 + 2] * 0.5f;
        lo[2 * j + 1] = ry + oy / (float)P * rp[l * 4 + 3] * 0.5f;
      }
    }
  }
}

// sampling head, backward: from the core op's gradients of the locations and weights to d_offlog (offlog's layout).
// d_logits = w (g - sum w g) over the row's L P weights; d_off = grad_loc times the factor each offset entered its location with.
// The reference points are constants (every caller builds them from the shapes): no gradient.
__global__ __launch_bounds__(256) void md_head_bwd_kernel(const float* __restrict__ gloc, const float* __restrict__ gaw, const float* __restrict__ aw,
                                                         const float* __restrict__ ref, int ref_dim, float* __restrict__ d_offlog, long long rows,
                                                         int heads, MdLevels lv) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * heads) return;
  const long long r = i / heads;
  const int m = (int)(i - r * heads);
  const int L = lv.L, P = lv.P, LP = L * P;
  const long long NO = (long long)heads * LP * 3;
  const float* const a = aw + i * LP;
  const float* const g = gaw + i * LP;
  float dot = 0.f;
  for (int j = 0; j < LP; ++j) dot += a[j] * g[j];
  float* const dl = d_offlog + r * NO + (long long)heads * LP * 2 + (long long)m * LP;
  for (int j = 0; j < LP; ++j) dl[j] = a[j] * (g[j] - dot);
  const float* const gl = gloc + i * LP * 2;
  const float* const rp = ref + r * L * ref_dim;
  float* const dof = d_offlog + r * NO + (long long)m * LP * 2;
  for (int l = 0; l < L; ++l)
    for (int p = 0; p < P; ++p) {
      const int j = l * P + p;
      if (ref_dim == 2) {
        dof[2 * j] = gl[2 * j] / lv.w[l];
        dof[2 * j + 1] = gl[2 * j + 1] / lv.h[l];
      } else {
        dof[2 * j] = gl[2 * j] / (float)P * rp[l * 4 + 2] * 0.5f;
        dof[2 * j + 1] = gl[2 * j + 1] / (float)P * rp[l * 4 + 3] * 0.5f;
      }
    }
}

}  // namespace tr
}  // namespace axvs
