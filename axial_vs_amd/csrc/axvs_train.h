// Training tier of the axial-trajectory attention layer: fp32 activations in natural [B,T,H,W] row order, the
// attention / softmax / dropout / LayerNorm kernels here, the Linear layers' GEMMs (forward, dgrad, wgrad) in axvs_gemm_nt.hip /
// axvs_train_gemm.h (split-precision bf16 MFMA).  Host side: axvs_train_host.h (shapes, buffers, the tier choice and the launches of a
// trajectory pass), entry points in axvs_train.hip.  Nothing here is on the inference path; that stays on the fused 16-bit MFMA kernels (axvs_fused.h).
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
__device__ __forceinline__ void load_row(float (&r)[D], const float* p, float scale) {
  load_row<D>(r, p);
#pragma unroll
  for (int i = 0; i < D; ++i) r[i] *= scale;
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

// The two layouts every spatial kernel shares (the backward rebuilds P and the dropout masks from exactly these):
// statistics (max, 1 / sum, D) of (sequence s, head h, query qn, frame f): stats is [(s heads + h), N, T, 3]
template <class F>
__device__ __forceinline__ F* stat_ptr(F* stats, int s, int h, int qn, int f, int heads, int N, int T) {
  return stats + ((((size_t)s * heads + h) * N + qn) * T + f) * 3;
}
// dropout element index of P[(s h), qn, f, n = 0]: its offset in the reference's tensor; key n of the frame is + n
// (qn is 64-bit so that a caller's sum of chunk, tile and lane offsets joins the 64-bit sum term by term)
__device__ __forceinline__ unsigned long long drop_base(int s, int h, unsigned long long qn, int f, int heads, int N, int T, int L) {
  return ((((unsigned long long)s * heads + h) * N + qn) * T + f) * L;
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
//      dropout index of P[(s h), q, f, n]: drop_base(..) + n.
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
      const unsigned long long base = drop_base(s, h, qn, f, heads, N, T, L);
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

__host__ __device__ inline int ceil16(int n) { return (n + 15) & ~15; }

// `count` rows of (sequence s, head h) from sequence row `first` on -> LDS [ceil16(count)][kTrLd], rows past `count` zero.
// A frame's keys: first = f L, count = L; a chunk of them: first = f L + c0.
__device__ __forceinline__ void stage_rows36(float* dst, const float* src, const RowMap& rm, int s, int first, int count, int h, int C, int tid) {
  const int np = ceil16(count);
  for (int i = tid; i < np * 8; i += 256) {
    const int n = i >> 3, c4 = i & 7;
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (n < count) v = *reinterpret_cast<const float4*>(src + nat_row(rm, s * rm.N + first + n) * C + h * 32 + c4 * 4);
    *reinterpret_cast<float4*>(dst + n * kTrLd + c4 * 4) = v;
  }
}
// A operands of the 4 x 2 MFMAs that contract keys nl .. nl + 3: channels j and 16 + j of those rows of a staged tile
__device__ __forceinline__ void load_cols(float (&a)[4][2], const float* tile, int nl, int j) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    a[r][0] = tile[(nl + r) * kTrLd + j];
    a[r][1] = tile[(nl + r) * kTrLd + j + 16];
  }
}

// The same operands less channels j and 16 + j of a reference key (c0, c1), for dq = sum_n dS_n k_n.  sum_n dS_n is 0 in exact
// arithmetic, so any reference gives the same dq; what fp32 leaves of that sum (P is rebuilt from the forward's statistics on scores
// accumulated in another order, so sum_n P_n is 1 only to ~|s| 2^-23) then multiplies the keys' spread and not their common part.  With
// a k.bias 800 times the usual the common part cost dq 2e-4 (profiles/traj_train_regimes_parity.txt).  Padding rows carry dS = 0.
__device__ __forceinline__ void load_cols_less(float (&a)[4][2], const float* tile, int nl, int j, float c0, float c1) {
  load_cols(a, tile, nl, j);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    a[r][0] -= c0;
    a[r][1] -= c1;
  }
}

// dynamic LDS of the LDS-resident query-side kernels: K | V of a frame, [ceil16(L)][kTrLd] each (two equal halves)
__host__ __device__ inline size_t spatial_frame_lds(int L) { return (size_t)2 * ceil16(L) * kTrLd * sizeof(float); }

// One (16-query, 16-key) tile of the forward: kr / qr are this lane's 8 channels of key / scaled query j, va the V^T operands of
// keys n0 .. n0 + 3 (this lane's 4 keys of the frame), base the query's dropout base; m / sum / acc are the query's running state.
__device__ __forceinline__ void fwd_tile(const float (&kr)[8], const float (&qr)[8], const float (&va)[4][2], int n0, int L, const Drop& dr,
                                         unsigned long long base, float& m, float& sum, f32x4 (&acc)[2]) {
  f32x4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 8; ++t) sc = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[t], qr[t], sc, 0, 0, 0);
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
    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[r][0], p[r], acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[r][1], p[r], acc[1], 0, 0, 0);
  }
}
// x of (query, frame) = acc / sum and the softmax statistics the backward kernels rebuild P from.  xo: the lane's channels 4 g .. of
// the x row (lane (query j, group g) holds channels dt * 16 + 4 g + r); st: the statistics triple, written by group 0.
__device__ __forceinline__ void fwd_store(float* xo, float* st, const f32x4 (&acc)[2], float m, float sum, int g) {
  const float inv = 1.f / sum;
  *reinterpret_cast<float4*>(xo) = float4{acc[0][0] * inv, acc[0][1] * inv, acc[0][2] * inv, acc[0][3] * inv};
  *reinterpret_cast<float4*>(xo + 16) = float4{acc[1][0] * inv, acc[1][1] * inv, acc[1][2] * inv, acc[1][3] * inv};
  if (g == 0) {
    st[0] = m;
    st[1] = inv;
  }
}

__global__ __launch_bounds__(256) void tr_spatial_fwd_mfma_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                   const float* __restrict__ v, float* __restrict__ x,
                                                                   float* __restrict__ stats /* [(s heads + h), N, T, 3]: max, 1 / sum, - */,
                                                                   RowMap rm, int T, int C, int heads, float scale, Drop dr) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int s = blockIdx.x / heads, h = blockIdx.x - s * heads, N = rm.N, L = rm.L;
  const int nkt = ceil16(L) >> 4, nqt = (N + 15) >> 4;
  float* ks = smem;
  float* vs = smem + spatial_frame_lds(L) / sizeof(float) / 2;
  // few sequences (the cross-clip module: B x heads workgroups): gridDim.y splits the query tiles, gridDim.z the frames -- every
  // (query tile, frame) is computed by exactly one wave whatever the split, with the same instructions
  const int fper = (T + (int)gridDim.z - 1) / (int)gridDim.z, f0 = (int)blockIdx.z * fper, f1 = min(T, f0 + fper);
  for (int f = f0; f < f1; ++f) {
    __syncthreads();
    stage_rows36(ks, k, rm, s, f * L, L, h, C, tid);
    stage_rows36(vs, v, rm, s, f * L, L, h, C, tid);
    __syncthreads();
    for (int qt = (int)blockIdx.y * 4 + wave; qt < nqt; qt += 4 * (int)gridDim.y) {
      const int qn = qt * 16 + j, qc = min(qn, N - 1);
      const long long mq = nat_row(rm, s * N + qc);
      float qr[8];
      load_row(qr, q + mq * C + h * 32 + 8 * g, scale);
      float m = -INFINITY, sum = 0.f;
      f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      const unsigned long long base = drop_base(s, h, qc, f, heads, N, T, L);
      for (int kt = 0; kt < nkt; ++kt) {
        float kr[8], va[4][2];
        load_row(kr, ks + (kt * 16 + j) * kTrLd + 8 * g);
        const int n0 = kt * 16 + 4 * g;             // my 4 keys: n0 .. n0 + 3
        load_cols(va, vs, n0, j);
        fwd_tile(kr, qr, va, n0, L, dr, base, m, sum, acc);
      }
      if (qn < N) fwd_store(x + (mq * T + f) * C + h * 32 + 4 * g, stat_ptr(stats, s, h, qn, f, heads, N, T), acc, m, sum, g);
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
//      are those of tr_spatial_fwd_mfma_kernel (stat_ptr, drop_base, fwd_store), so the backward kernels do not care which one ran (saved activations of the two
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
  const int Lp = ceil16(L);
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
  const int Lp = ceil16(L), nkt = Lp >> 4, nqt = (N + 15) >> 4, LV = Lp + 4;
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
        load_row(kv, k + row);
        load_row(vv, v + row);
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
      const unsigned long long base = drop_base(s, h, min(qn, N - 1), f, heads, N, T, L);
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
      if (qn < N) fwd_store(x + (mq * T + f) * C + h * 32 + 4 * g, stat_ptr(stats, s, h, qn, f, heads, N, T), acc, m, sum, g);
    }
  }
}

// ---- backward on the matrix cores, part 1 (queries): D = dx . x (= sum_n P keep dP, the flash-attention identity), then per
//      16-key tile  S^T = K Q^T,  dP^T = V dX^T  (8 + 8 MFMAs),  dS = P (keep dP - D) with P rebuilt from the forward's (max, 1/sum),
//      dq^T += K^T dS^T (4 x 2 MFMAs, keys {4 g + r} per step as in the forward).  dq accumulates over the frames in global memory
//      (first frame writes).  Writes D into stats[.., 2] for part 2.
// dx of (query, frame) for the lane's 8 channels and D = dx . x summed over the query's 4 lane groups
__device__ __forceinline__ float load_dx_D(float (&dxr)[8], const float* dxp, const float* xp) {
  float xr[8];
  load_row(dxr, dxp);
  load_row(xr, xp);
  return xor_sum16_32(dxr[0] * xr[0] + dxr[1] * xr[1] + dxr[2] * xr[2] + dxr[3] * xr[3] + dxr[4] * xr[4] + dxr[5] * xr[5] + dxr[6] * xr[6] +
                      dxr[7] * xr[7]);
}
// One (16-query, 16-key) tile of the query-side backward: kr / vr are this lane's 8 channels of key j, qr / dxr those of query j,
// ka the K^T operands of keys n0 .. n0 + 3; (m, inv) the forward's statistics, D = dx . x; acc is dq^T before the scale.
__device__ __forceinline__ void bwd_q_tile(const float (&kr)[8], const float (&vr)[8], const float (&qr)[8], const float (&dxr)[8],
                                           const float (&ka)[4][2], float m, float inv, float D, int n0, int L, const Drop& dr,
                                           unsigned long long base, f32x4 (&acc)[2]) {
  f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    sc = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[t], qr[t], sc, 0, 0, 0);
    dp = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[t], dxr[t], dp, 0, 0, 0);
  }
  float ds[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool valid = n0 + r < L;
    const float P = valid ? __expf(sc[r] - m) * inv : 0.f;
    const float keep = drop_keep(dr, base + n0 + r);      // (hashed for padding keys too: no branch; P = 0 there)
    ds[r] = P * ((valid ? keep : 0.f) * dp[r] - D);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[r][0], ds[r], acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[r][1], ds[r], acc[1], 0, 0, 0);
  }
}

__global__ __launch_bounds__(256) void tr_spatial_bwd_q_mfma_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                     const float* __restrict__ v, const float* __restrict__ x,
                                                                     const float* __restrict__ dx, float* __restrict__ dq,
                                                                     float* __restrict__ stats, RowMap rm, int T, int C, int heads, float scale,
                                                                     Drop dr) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int s = blockIdx.x / heads, h = blockIdx.x - s * heads, N = rm.N, L = rm.L;
  const int nkt = ceil16(L) >> 4, nqt = (N + 15) >> 4;
  float* ks = smem;
  float* vs = smem + spatial_frame_lds(L) / sizeof(float) / 2;
  for (int f = 0; f < T; ++f) {            // (dq accumulates over the frames: they stay in one workgroup; gridDim.y splits the query tiles)
    __syncthreads();
    stage_rows36(ks, k, rm, s, f * L, L, h, C, tid);
    stage_rows36(vs, v, rm, s, f * L, L, h, C, tid);
    __syncthreads();
    const float k0a = ks[j], k0b = ks[j + 16];      // key 0 of the frame, channels j and 16 + j: the reference of load_cols_less
    for (int qt = (int)blockIdx.y * 4 + wave; qt < nqt; qt += 4 * (int)gridDim.y) {
      const int qn = qt * 16 + j, qc = min(qn, N - 1);
      const long long mq = nat_row(rm, s * N + qc);
      float qr[8], dxr[8];
      load_row(qr, q + mq * C + h * 32 + 8 * g, scale);
      const float dsum = load_dx_D(dxr, dx + (mq * T + f) * C + h * 32 + 8 * g, x + (mq * T + f) * C + h * 32 + 8 * g);
      float* st = stat_ptr(stats, s, h, qc, f, heads, N, T);
      const float m = st[0], inv = st[1];
      f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      const unsigned long long base = drop_base(s, h, qc, f, heads, N, T, L);
      for (int kt = 0; kt < nkt; ++kt) {
        float kr[8], vr[8], ka[4][2];
        load_row(kr, ks + (kt * 16 + j) * kTrLd + 8 * g);
        load_row(vr, vs + (kt * 16 + j) * kTrLd + 8 * g);
        const int n0 = kt * 16 + 4 * g;
        load_cols_less(ka, ks, n0, j, k0a, k0b);
        bwd_q_tile(kr, vr, qr, dxr, ka, m, inv, dsum, n0, L, dr, base, acc);
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
// dynamic LDS for Nc staged queries: scale * q [Nc][kTrLd] | dx of the frame [Nc][kTrLd] | (max, 1 / sum, D, -) [Nc][4]
__host__ __device__ inline size_t spatial_kv_lds(int Nc) { return (size_t)Nc * (2 * kTrLd + 4) * sizeof(float); }

__global__ __launch_bounds__(256) void tr_spatial_bwd_kv_mfma_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                      const float* __restrict__ v, const float* __restrict__ dx,
                                                                      const float* __restrict__ stats, float* __restrict__ dk,
                                                                      float* __restrict__ dv, RowMap rm, int T, int C, int heads, float scale,
                                                                      Drop dr, int Nc /* queries staged at a time: a multiple of 16 */) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int s = blockIdx.x / heads, h = blockIdx.x - s * heads, N = rm.N, L = rm.L;
  const int Np = ceil16(N), nkt = (L + 15) >> 4;
  const int nchunks = (Np + Nc - 1) / Nc;          // 1: the whole sequence's queries fit (the within-clip layer); more: 12+ clips of 128 queries
  float* qs = smem;                      // the three parts of spatial_kv_lds(Nc)
  float* gs = qs + Nc * kTrLd;
  float* ss = gs + Nc * kTrLd;
  // (the two staging loops are stage_rows36 with a scale, a T-strided source and all Nc rows filled.  They stay written out, and the
  //  dropout index below sums its query offsets in 64 bits: with stage_rows36 here and an int query index the kernel's code changed
  //  throughout and measured 4 - 6 % slower; as written its assembly is the parent's but for the order of two loads --
  //  profiles/train_attn_refactor.md)
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
      const float* st = stat_ptr(stats, s, h, min(c0 + n, N - 1), f, heads, N, T);
      // padding queries: 1/sum = 0 makes their probabilities vanish.  Their staged q is zero, so their scores are 0: the maximum is
      // 0 too, not the last live query's -- under that one __expf(0 - max) is inf once a live maximum lies below -88.7, and inf * 0 = NaN
      const bool live = c0 + n < N;
      *reinterpret_cast<float4*>(ss + n * 4) = float4{live ? st[0] : 0.f, live ? st[1] : 0.f, st[2], 0.f};
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
      load_row(kr, k + mk * C + h * 32 + 8 * g);
      load_row(vr, v + mk * C + h * 32 + 8 * g);
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
            float qr[8], gr[8];
            load_row(qr, qs + (qt * 16 + j) * kTrLd + 8 * g);
            load_row(gr, gs + (qt * 16 + j) * kTrLd + 8 * g);
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
              const float kp_ = (c0 + ql + r < N && kn < L) ? drop_keep(dr, drop_base(s, h, (unsigned long long)c0 + ql + r, f, heads, N, T, L) + kn) : 0.f;
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
//      frame's keys staged kSpChunk at a time.  The forward's running max / sum per 16-key tile is fwd_tile, the step
//      tr_spatial_fwd_mfma_kernel takes (same tile order: the same statistics (max, 1 / sum) into `stats`, the same x layout), so the
//      key-side backward (tr_spatial_bwd_kv_mfma_kernel, which stages QUERIES in chunks and never holds a whole frame) serves
//      both.  A wave owns kSpQT query tiles at a time, so each K / V fragment read from LDS feeds kSpQT tiles.  LDS: K and V
//      chunks [kSpChunk][kTrLd] = 72 KiB (two workgroups per CU).  Dropout element indices are 64-bit (2.1e9 at 64 x 64 x 4).
constexpr int kSpChunk = 256;   // keys of a frame per LDS stage (a multiple of 16)
constexpr int kSpQT = 2;        // 16-query tiles per wave
__host__ __device__ inline size_t spatial_chunk_lds() { return (size_t)2 * kSpChunk * kTrLd * sizeof(float); }   // K | V chunk, equal halves

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
  float* vs = smem + spatial_chunk_lds() / sizeof(float) / 2;
  const int fper = (T + (int)gridDim.z - 1) / (int)gridDim.z, f0 = (int)blockIdx.z * fper, f1 = min(T, f0 + fper);
  for (int f = f0; f < f1; ++f)
    for (int qb = (int)blockIdx.y; qb < nqb; qb += (int)gridDim.y) {
      float qr[kSpQT][8], m[kSpQT], sum[kSpQT];
      f32x4 acc[kSpQT][2];
      unsigned long long base[kSpQT];
#pragma unroll
      for (int u = 0; u < kSpQT; ++u) {
        const int qc = min((qb * 4 * kSpQT + u * 4 + wave) * 16 + j, N - 1);
        load_row(qr[u], q + nat_row(rm, s * N + qc) * C + h * 32 + 8 * g, scale);
        m[u] = -INFINITY;
        sum[u] = 0.f;
        acc[u][0] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc[u][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        base[u] = drop_base(s, h, qc, f, heads, N, T, L);
      }
      for (int c0 = 0; c0 < L; c0 += kSpChunk) {
        const int Lc = min(kSpChunk, L - c0);            // keys of this chunk
        __syncthreads();
        stage_rows36(ks, k, rm, s, f * L + c0, Lc, h, C, tid);
        stage_rows36(vs, v, rm, s, f * L + c0, Lc, h, C, tid);
        __syncthreads();
        const int nkt = (Lc + 15) >> 4;
        for (int kt = 0; kt < nkt; ++kt) {
          float kr[8], va[4][2];
          load_row(kr, ks + (kt * 16 + j) * kTrLd + 8 * g);
          const int nl = kt * 16 + 4 * g, n0 = c0 + nl;          // my 4 keys: n0 .. n0 + 3 of the frame (nl .. within the chunk)
          load_cols(va, vs, nl, j);
#pragma unroll
          for (int u = 0; u < kSpQT; ++u) {
            if ((qb * 4 * kSpQT + u * 4 + wave) >= nqt) continue;      // (uniform per wave)
            fwd_tile(kr, qr[u], va, n0, L, dr, base[u], m[u], sum[u], acc[u]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kSpQT; ++u) {
        const int qn = (qb * 4 * kSpQT + u * 4 + wave) * 16 + j;
        if (qn < N)
          fwd_store(x + (nat_row(rm, s * N + qn) * T + f) * C + h * 32 + 4 * g, stat_ptr(stats, s, h, qn, f, heads, N, T), acc[u], m[u], sum[u], g);
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
  float* vs = smem + spatial_chunk_lds() / sizeof(float) / 2;
  for (int qb = (int)blockIdx.y; qb < nqb; qb += (int)gridDim.y) {
    float qr[kSpQT][8];
    long long mq[kSpQT];
    int qc[kSpQT];
    f32x4 acc[kSpQT][2];
#pragma unroll
    for (int u = 0; u < kSpQT; ++u) {
      qc[u] = min((qb * 4 * kSpQT + u * 4 + wave) * 16 + j, N - 1);
      mq[u] = nat_row(rm, s * N + qc[u]);
      load_row(qr[u], q + mq[u] * C + h * 32 + 8 * g, scale);
      acc[u][0] = f32x4{0.f, 0.f, 0.f, 0.f};
      acc[u][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int f = 0; f < T; ++f) {
      float dxr[kSpQT][8], dsum[kSpQT], m[kSpQT], inv[kSpQT];
      unsigned long long base[kSpQT];
#pragma unroll
      for (int u = 0; u < kSpQT; ++u) {
        dsum[u] = load_dx_D(dxr[u], dx + (mq[u] * T + f) * C + h * 32 + 8 * g, x + (mq[u] * T + f) * C + h * 32 + 8 * g);
        const float* st = stat_ptr(stats, s, h, qc[u], f, heads, N, T);
        m[u] = st[0];
        inv[u] = st[1];
        base[u] = drop_base(s, h, qc[u], f, heads, N, T, L);
      }
      float k0a = 0.f, k0b = 0.f;                  // key 0 of the frame, channels j and 16 + j: the reference of load_cols_less
      for (int c0 = 0; c0 < L; c0 += kSpChunk) {
        __syncthreads();
        stage_rows36(ks, k, rm, s, f * L + c0, min(kSpChunk, L - c0), h, C, tid);
        stage_rows36(vs, v, rm, s, f * L + c0, min(kSpChunk, L - c0), h, C, tid);
        __syncthreads();
        if (c0 == 0) {
          k0a = ks[j];
          k0b = ks[j + 16];
        }
        const int nkt = (min(kSpChunk, L - c0) + 15) >> 4;
        for (int kt = 0; kt < nkt; ++kt) {
          float kr[8], vr[8], ka[4][2];
          load_row(kr, ks + (kt * 16 + j) * kTrLd + 8 * g);
          load_row(vr, vs + (kt * 16 + j) * kTrLd + 8 * g);
          const int nl = kt * 16 + 4 * g, n0 = c0 + nl;
          load_cols_less(ka, ks, nl, j, k0a, k0b);
#pragma unroll
          for (int u = 0; u < kSpQT; ++u) {
            if ((qb * 4 * kSpQT + u * 4 + wave) >= nqt) continue;      // (uniform per wave)
            bwd_q_tile(kr, vr, qr[u], dxr[u], ka, m[u], inv[u], dsum[u], n0, L, dr, base[u], acc[u]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kSpQT; ++u)
        if (g == 0 && (qb * 4 * kSpQT + u * 4 + wave) * 16 + j < N) stat_ptr(stats, s, h, qc[u], f, heads, N, T)[2] = dsum[u];
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
      const unsigned long long base = drop_base(s, h, qn, f, heads, N, T, L);
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
        const float dS = P * (dP - Dsum);
#pragma unroll
        for (int i = 0; i < D; ++i) dqr[i] += dS * (ks[n * D + i] - ks[i]);      // less key 0 of the frame: see load_cols_less
      }
      float* st = stat_ptr(stats, s, h, qn, f, heads, N, T);
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
      for (int i = tid; i < nq * T * 3; i += 256) sts[i] = stat_ptr(stats, s, h, q0, 0, heads, N, T)[i];
      __syncthreads();
      if (!act) continue;
      for (int qi = 0; qi < nq; ++qi) {
        const float* st = sts + (qi * T + f) * 3;
        const float P = __expf(dot_lds<D>(kr, qs + qi * D) - st[0]) * st[1];
        const float kp = drop_keep(dr, drop_base(s, h, q0 + qi, f, heads, N, T, L) + n);
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
