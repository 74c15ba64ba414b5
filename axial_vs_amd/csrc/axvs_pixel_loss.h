// The sampled pixel losses of the within-clip criterion (maxtron_deeplab/modeling/wc_criterion.py:62-142, :341-415): Gumbel top-k
// pixel sampling, the pixel-wise instance-discrimination loss and the auxiliary semantic loss, with their gradients.
//
//   sampling (3 launches for all noise rows of a step)
//     1 px_area_kernel       one workgroup per matched pair: area[i] = sum_p t[i, p]
//     2 px_key_kernel        per matching and video, one thread per pixel: pix_area, void and log(P / max(pix_area, 1)) from ONE read of
//                            the matched targets, then key[p] of every noise row that uses this matching, in the reference's fp32
//                            operation order (no contraction of the multiply and the adds)
//     3 px_select_kernel     one workgroup per (noise row, video): radix select of the k largest keys over the order-preserving integer
//                            image of a float (four 8-bit passes over the row in global memory), equal keys to the lower pixel, the
//                            indices written in increasing pixel order
//   instance discrimination, forward (4): gather F [k][C] and G [k][pairs] (zero padded to multiples of 16), the streamed kernel, finish
//     px_insdis_fwd_kernel   a workgroup owns 16 columns j; its four waves walk the 16-row tiles of k in turn: S = F^T F / 0.3 and
//                            g = G^T G on the f32-input MFMA (0 / 1 targets give exact g), running max / sum of exponentials, c_j and
//                            sum_k g S per column, combined over the waves in wave order.  No K x K tensor exists.
//   instance discrimination, backward (3): the two gathers, then px_insdis_bwd_kernel: the same walk recomputes each S tile once,
//                            forms dS[k, j] + dS[j, k] from the saved statistics of both tiles and contracts it with F on the MFMA;
//                            the waves' partial tiles are added in wave order and one wave writes the 16 samples' gradient columns
//                            (distinct pixels: plain stores)
//   auxiliary semantic loss: one thread per sample, forward and backward
//
// Every sum has a fixed order (no floating-point atomics), so two runs give the same bits.
#pragma once
#include "axvs_targets.h"

namespace axvs {

constexpr int kPxMaxRows = kMaxLayers + 1;      // noise rows of a step: one per layer ('pixels') and one for 'aux_semantic'
constexpr int kPxMaxK = 8192, kPxMaxC = 256;
constexpr long long kPxMaxP = 1ll << 20;
constexpr int kPxSelThreads = 1024;
constexpr int kPxTJ = 16;                         // columns of a workgroup of the streamed kernels; its 4 waves share the rows of k
constexpr float kPxInvTau = 1.0f / 0.3f;          // instance_discrimination_temperature (wc_criterion.py:282)
constexpr float kPxVoidLogit = -99999.0f;         // _SOFTMAX_MASKING_CONSTANT

typedef float px_f32x4 __attribute__((ext_vector_type(4)));

struct PxVideos {
  int m[kMaxVideos];                            // objects of video b
  int off[kMaxVideos];                          // first row of video b in the concatenated targets
};

struct PxRows {
  int R;
  const float* u[kPxMaxRows];                     // [B][P] uniform noise of row r
  int matching[kPxMaxRows];                       // the matching whose targets row r samples from
  float temperature[kPxMaxRows];
  int k[kPxMaxRows];
};

struct PxLayers {
  const float* feat[kMaxLayers];                // per layer: pixel_feature [B][C][P]
  float* dfeat[kMaxLayers];
};

// a product / sum rounded once, whatever the compiler's contraction mode: the result never fuses into a neighbouring operation
__device__ __forceinline__ float px_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float px_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// pairs of matching problem z = lm * B + b: min(N, M_b); a column outside 0 .. M_b - 1 (never written by the matcher) reads target 0
__device__ __forceinline__ int px_pairs(const PxVideos& v, int b, int N) { return min(N, v.m[b]); }
__device__ __forceinline__ int px_col(const long long* cols, long long at, int mb) {
  const long long c = cols[at];
  return (c < 0 || c >= mb) ? 0 : (int)c;
}

// deterministic sum over a 256-thread workgroup (every thread gets it)
__device__ __forceinline__ float px_block_sum256(float v, float* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// ---- sampling ---------------------------------------------------------------------------------------------------------------------
template <int TD>
__global__ __launch_bounds__(256) void px_area_kernel(PxVideos v, const void* __restrict__ targets, const long long* __restrict__ cols,
                                                      int kmax, int B, int N, int P, float* __restrict__ area) {
  __shared__ float red[256];
  const int i = blockIdx.x, z = blockIdx.y, b = z % B;
  float acc = 0.f;
  if (i < px_pairs(v, b, N)) {                    // uniform over the workgroup
    const long long base = (long long)(v.off[b] + px_col(cols, (long long)z * kmax + i, v.m[b])) * P;
    for (int p = threadIdx.x; p < P; p += 256) acc += load_f32<TD>(targets, base + p);
  }
  const float s = px_block_sum256(acc, red);
  if (threadIdx.x == 0) area[(long long)z * kmax + i] = s;
}

template <int TD>
__global__ __launch_bounds__(256) void px_key_kernel(PxVideos v, PxRows rw, const void* __restrict__ targets, const long long* __restrict__ cols,
                                                     const float* __restrict__ area, int kmax, int B, int N, int P, float* __restrict__ keys) {
  __shared__ float s_area[kMaxObjects];
  __shared__ int s_row[kMaxObjects];
  const int z = blockIdx.y, b = z % B, lm = z / B, kb = px_pairs(v, b, N);
  for (int i = threadIdx.x; i < kb; i += 256) {
    s_area[i] = area[(long long)z * kmax + i];
    s_row[i] = v.off[b] + px_col(cols, (long long)z * kmax + i, v.m[b]);
  }
  __syncthreads();
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  float st = 0.f, pa = 0.f;
  for (int i = 0; i < kb; ++i) {
    const float t = load_f32<TD>(targets, (long long)s_row[i] * P + p);
    st += t;
    pa += t * s_area[i];
  }
  const bool is_void = st < 1.0f;
  // P / clamp(pix_area, 1) with a Python int on the left is reciprocal() * P in torch
  const float inv = px_mul(1.0f / fmaxf(pa, 1.0f), (float)P);
  const float lg = logf(inv);
  for (int r = 0; r < rw.R; ++r) {
    if (rw.matching[r] != lm) continue;
    float a = px_mul(lg, rw.temperature[r]);
    if (is_void) a = px_add(a, kPxVoidLogit);
    const float g = -logf(-logf(rw.u[r][(long long)b * P + p]));
    keys[((long long)r * B + b) * P + p] = px_add(a, g);
  }
}

// order-preserving integer image of a float: a > b  <=>  image(a) > image(b)  (-0 sorts under +0: the one pair torch calls equal)
__device__ __forceinline__ unsigned px_image(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(kPxSelThreads) void px_select_kernel(PxRows rw, const float* __restrict__ keys, int B, int P, int kstride,
                                                                   int* __restrict__ idx) {
  __shared__ unsigned hist[256];
  __shared__ unsigned sh_prefix, sh_need;
  __shared__ unsigned w_gt[kPxSelThreads / 64], w_eq[kPxSelThreads / 64];
  const int row = blockIdx.x, r = row / B, k = rw.k[r];
  if (k <= 0) return;                               // uniform
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* key = keys + (long long)row * P;
  int* out = idx + (long long)row * kstride;
  // the k-th largest image, 8 bits a pass from the top
  unsigned prefix = 0, need = (unsigned)k;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int p = tid; p < P; p += kPxSelThreads) {
      const unsigned im = px_image(key[p]);
      if (pass == 0 || (im >> (shift + 8)) == prefix) atomicAdd(&hist[(im >> shift) & 255], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned cum = 0;
      int d = 255;
      for (; d > 0; --d) {
        if (cum + hist[d] >= need) break;
        cum += hist[d];
      }
      sh_prefix = (prefix << 8) | (unsigned)d;
      sh_need = need - cum;
    }
    __syncthreads();
    prefix = sh_prefix;
    need = sh_need;
  }
  // keep every key above the threshold and the first `need` pixels at it.  Wave w owns one contiguous range of pixels: count, then write.
  const unsigned thr = prefix;
  const int seg = ((P + kPxSelThreads / 64 - 1) / (kPxSelThreads / 64) + 63) / 64 * 64;
  const int p0 = min(P, wv * seg), p1 = min(P, p0 + seg);
  unsigned n_gt = 0, n_eq = 0;
  for (int c = p0; c < p1; c += 64) {
    const int p = c + lane;
    const unsigned im = p < p1 ? px_image(key[p]) : 0u;
    n_gt += __popcll(__builtin_amdgcn_ballot_w64(p < p1 && im > thr));
    n_eq += __popcll(__builtin_amdgcn_ballot_w64(p < p1 && im == thr));
  }
  if (lane == 0) { w_gt[wv] = n_gt; w_eq[wv] = n_eq; }
  __syncthreads();
  unsigned gt_before = 0, eq_before = 0;
  for (int w = 0; w < wv; ++w) { gt_before += w_gt[w]; eq_before += w_eq[w]; }
  unsigned written = gt_before + min(eq_before, need);
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int c = p0; c < p1; c += 64) {
    const int p = c + lane;
    const unsigned im = p < p1 ? px_image(key[p]) : 0u;
    const bool eq = p < p1 && im == thr;
    const unsigned long long eqb = __builtin_amdgcn_ballot_w64(eq);
    const bool sel = (p < p1 && im > thr) || (eq && eq_before + (unsigned)__popcll(eqb & lt) < need);
    const unsigned long long selb = __builtin_amdgcn_ballot_w64(sel);
    const unsigned pos = written + (unsigned)__popcll(selb & lt);
    if (sel && pos < (unsigned)k) out[pos] = p;
    written += (unsigned)__popcll(selb);
    eq_before += (unsigned)__popcll(eqb);
  }
}

// ---- gathers: the samples' features F [lb][Kp][Cp] and matched targets G [lb][Kp][Mp], zero beyond k / C / the pairs ----------------
__global__ __launch_bounds__(256) void px_gather_feat_kernel(PxLayers ly, const int* __restrict__ idx, int B, int C, int P, int k, int kstride,
                                                             int Kp, int Cp, float* __restrict__ F) {
  const int lb = blockIdx.y, l = lb / B, b = lb % B;
  const int j = blockIdx.x * 64 + (threadIdx.x & 63);
  if (j >= Kp) return;
  const int p = j < k ? idx[(long long)lb * kstride + j] : -1;
  const float* src = ly.feat[l] + (long long)b * C * P;
  float* dst = F + ((long long)lb * Kp + j) * Cp;
  for (int c = threadIdx.x >> 6; c < Cp; c += 4) dst[c] = (p >= 0 && c < C) ? src[(long long)c * P + p] : 0.f;
}

template <int TD>
__global__ __launch_bounds__(256) void px_gather_tgt_kernel(PxVideos v, const void* __restrict__ targets, const long long* __restrict__ cols,
                                                            const int* __restrict__ idx, int kmax, int share, int B, int N, int P, int k,
                                                            int kstride, int Kp, int Mp, float* __restrict__ G) {
  const int lb = blockIdx.y, l = lb / B, b = lb % B, z = (share ? 0 : l) * B + b, kb = px_pairs(v, b, N);
  const int j = blockIdx.x * 64 + (threadIdx.x & 63);
  if (j >= Kp) return;
  const int p = j < k ? idx[(long long)lb * kstride + j] : -1;
  float* dst = G + ((long long)lb * Kp + j) * Mp;
  for (int i = threadIdx.x >> 6; i < Mp; i += 4) {
    float t = 0.f;
    if (p >= 0 && i < kb) t = load_f32<TD>(targets, (long long)(v.off[b] + px_col(cols, (long long)z * kmax + i, v.m[b])) * P + p);
    dst[i] = t;
  }
}

// ---- the 16 x 16 tile of X^T X for sample rows r0 .. r0 + 15 and columns c0 .. c0 + 15, X [Kp][D] with D a multiple of 16 ------------
// Lane (i = lane & 15, q = lane >> 4) loads 4 consecutive values of its sample: the MFMA's contraction index runs over the same
// permutation of D on both operands.  Two accumulators keep two MFMA chains in flight.
__device__ __forceinline__ px_f32x4 px_gram_tile(const float* __restrict__ X, int D, int r0, int c0, int lane) {
  const float* pa = X + (long long)(r0 + (lane & 15)) * D + 4 * (lane >> 4);
  const float* pb = X + (long long)(c0 + (lane & 15)) * D + 4 * (lane >> 4);
  px_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  for (int d = 0; d < D; d += 16) {
    const float4 a = *reinterpret_cast<const float4*>(pa + d);
    const float4 b = *reinterpret_cast<const float4*>(pb + d);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc1, 0, 0, 0);
  }
  return acc0 + acc1;
}

// what the forward keeps per (layer, video): [Kp] each, and the nonzero count per (layer, video)
struct PxSaved {
  float *lse, *c, *lossj, *nnz;
};

// A workgroup of the streamed kernels owns 16 columns; its four waves walk the 16-row tiles of k in turn (wave w: tiles w, w + 4, ...)
// and their partial results are combined through LDS in wave order.  Result element r of a lane is row 4 (lane >> 4) + r, column
// lane & 15 of the tile.
__global__ __launch_bounds__(256) void px_insdis_fwd_kernel(const float* __restrict__ F, const float* __restrict__ G, int k, int Kp, int Cp, int Mp,
                                                            PxSaved sv) {
  __shared__ float part[4][4][16];                // [wave][max, sum of exponentials, c, sum g S][column]
  const int lb = blockIdx.y, lane = threadIdx.x & 63, q = lane >> 4, wv = threadIdx.x >> 6;
  const int j0 = blockIdx.x * kPxTJ;
  const float* Fl = F + (long long)lb * Kp * Cp;
  const float* Gl = G + (long long)lb * Kp * Mp;
  float m = -INFINITY, se = 0.f, c = 0.f, gs = 0.f;
  for (int r0 = 16 * wv; r0 < Kp; r0 += 64) {
    const px_f32x4 s4 = px_gram_tile(Fl, Cp, r0, j0, lane);
    px_f32x4 g4 = {0.f, 0.f, 0.f, 0.f};
    if (Mp > 0) g4 = px_gram_tile(Gl, Mp, r0, j0, lane);
    float s[4], tmax = -INFINITY;
    for (int r = 0; r < 4; ++r) {
      s[r] = px_mul(s4[r], kPxInvTau);      // rounded once, here and in the backward: a contraction into the subtractions below would not be
      if (r0 + 4 * q + r < k) tmax = fmaxf(tmax, s[r]);
      c += g4[r];                                 // rows beyond k are zero rows of G and of F
      gs += g4[r] * s[r];
    }
    if (tmax > -INFINITY) {
      const float mn = fmaxf(m, tmax);
      float add = 0.f;
      for (int r = 0; r < 4; ++r)
        if (r0 + 4 * q + r < k) add += expf(s[r] - mn);
      se = se * expf(m - mn) + add;
      m = mn;
    }
  }
  // the four row groups of a column, combined in a fixed order; a group (or a wave) without a valid row has max -inf and sum 0
  float M = -INFINITY;
  for (int qq = 0; qq < 4; ++qq) M = fmaxf(M, __shfl(m, (lane & 15) + 16 * qq));
  float se_t = 0.f, c_t = 0.f, gs_t = 0.f;
  for (int qq = 0; qq < 4; ++qq) {
    const int from = (lane & 15) + 16 * qq;
    const float mq = __shfl(m, from), sq = __shfl(se, from);
    se_t += mq > -INFINITY ? sq * expf(mq - M) : 0.f;
    c_t += __shfl(c, from);
    gs_t += __shfl(gs, from);
  }
  if (q == 0) {
    part[wv][0][lane] = M;
    part[wv][1][lane] = se_t;
    part[wv][2][lane] = c_t;
    part[wv][3][lane] = gs_t;
  }
  __syncthreads();
  const int j = j0 + lane;
  if (threadIdx.x < 16 && j < k) {
    float Mw = -INFINITY, sew = 0.f, cw = 0.f, gsw = 0.f;
    for (int w = 0; w < 4; ++w) Mw = fmaxf(Mw, part[w][0][lane]);
    for (int w = 0; w < 4; ++w) {
      sew += part[w][0][lane] > -INFINITY ? part[w][1][lane] * expf(part[w][0][lane] - Mw) : 0.f;
      cw += part[w][2][lane];
      gsw += part[w][3][lane];
    }
    const float lse = Mw + logf(sew);
    const long long at = (long long)lb * Kp + j;
    sv.lse[at] = lse;
    sv.c[at] = cw;
    sv.lossj[at] = (lse * cw - gsw) / fmaxf(cw, 1.0f);
  }
}

// One workgroup per layer (grid = rows): per video, sum_j loss_j / max(#{loss_j != 0}, 1); the mean over the videos.
__global__ __launch_bounds__(256) void px_finish_kernel(const float* __restrict__ lossj, int B, int k, int stride, float* __restrict__ nnz,
                                                        float* __restrict__ losses) {
  __shared__ float red[256];
  const int l = blockIdx.x;
  float total = 0.f;
  for (int b = 0; b < B; ++b) {
    const float* v = lossj + (long long)(l * B + b) * stride;
    float s = 0.f, n = 0.f;
    for (int j = threadIdx.x; j < k; j += 256) {
      s += v[j];
      n += v[j] != 0.f ? 1.f : 0.f;
    }
    s = px_block_sum256(s, red);
    n = px_block_sum256(n, red);
    if (threadIdx.x == 0) nnz[l * B + b] = n;
    total += s / fmaxf(n, 1.0f);
  }
  if (threadIdx.x == 0) losses[l] = total / (float)B;
}

// NCB: 16-channel blocks the accumulators are sized for (Cp <= 16 NCB)
template <int NCB>
__global__ __launch_bounds__(256) void px_insdis_bwd_kernel(PxLayers ly, const float* __restrict__ grad, const float* __restrict__ F,
                                                            const float* __restrict__ G, const int* __restrict__ idx, int B, int C, int P, int k,
                                                            int kstride, int Kp, int Cp, int Mp, PxSaved sv) {
  extern __shared__ float px_part[];              // [3 waves][Cp / 16][4][64]: the partial gradient tiles of waves 1 .. 3
  const int lb = blockIdx.y, l = lb / B, b = lb % B, lane = threadIdx.x & 63, q = lane >> 4, wv = threadIdx.x >> 6;
  const int j0 = blockIdx.x * kPxTJ;
  if (ly.dfeat[l] == nullptr) return;             // uniform over the workgroup
  const float* Fl = F + (long long)lb * Kp * Cp;
  const float* Gl = G + (long long)lb * Kp * Mp;
  const float* lse = sv.lse + (long long)lb * Kp;
  const float* cs = sv.c + (long long)lb * Kp;
  const float w = grad[l] / ((float)B * fmaxf(sv.nnz[lb], 1.0f));
  const int j = j0 + (lane & 15);
  const float lse_j = j < k ? lse[j] : 0.f, c_j = j < k ? cs[j] : 0.f, rj = 1.0f / fmaxf(c_j, 1.0f);
  px_f32x4 acc[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) acc[cb] = px_f32x4{0.f, 0.f, 0.f, 0.f};
  const int ncb = Cp / 16;
  for (int r0 = 16 * wv; r0 < Kp; r0 += 64) {
    const px_f32x4 s4 = px_gram_tile(Fl, Cp, r0, j0, lane);
    px_f32x4 g4 = {0.f, 0.f, 0.f, 0.f};
    if (Mp > 0) g4 = px_gram_tile(Gl, Mp, r0, j0, lane);
    float e[4];
    for (int r = 0; r < 4; ++r) {
      const int kr = r0 + 4 * q + r;
      e[r] = 0.f;
      if (kr < k && j < k) {
        const float s = px_mul(s4[r], kPxInvTau), c_k = cs[kr], rk = 1.0f / fmaxf(c_k, 1.0f);      // the forward's value, bit for bit
        // dS[kr, j] + dS[j, kr]
        e[r] = w * ((expf(s - lse_j) * c_j - g4[r]) * rj + (expf(s - lse[kr]) * c_k - g4[r]) * rk);
      }
    }
    // d F[j, :] += sum_k e[k, j] F[k, :]: the tile's element r of a lane is row 4 q + r, which is the A operand of contraction step r
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      if (cb < ncb) {
        for (int r = 0; r < 4; ++r) {
          const float f = Fl[(long long)(r0 + 4 * q + r) * Cp + cb * 16 + (lane & 15)];
          acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(e[r], f, acc[cb], 0, 0, 0);
        }
      }
    }
  }
  // waves 1 .. 3 hand their tiles to wave 0, which adds them in wave order and is the only writer of the 16 samples' gradient columns
  if (wv > 0) {
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
      if (cb < ncb)
        for (int r = 0; r < 4; ++r) px_part[(((wv - 1) * ncb + cb) * 4 + r) * 64 + lane] = acc[cb][r];
  }
  __syncthreads();
  if (wv > 0) return;
  float* dst = ly.dfeat[l] + (long long)b * C * P;
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    if (cb < ncb) {
      const int ch = cb * 16 + (lane & 15);
      for (int r = 0; r < 4; ++r) {
        float v = acc[cb][r];
        for (int ww = 0; ww < 3; ++ww) v += px_part[((ww * ncb + cb) * 4 + r) * 64 + lane];
        const int jj = j0 + 4 * q + r;
        if (jj < k && ch < C) dst[(long long)ch * P + idx[(long long)lb * kstride + jj]] = v * kPxInvTau;
      }
    }
  }
}

// ---- auxiliary semantic loss: cross-entropy of pred [B][Cs][P] against sem [B][P] at the samples; -1 and every class outside 0 .. Cs - 1
// (num_classes among them) are ignored ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool px_sem_kept(long long t, int Cs, int num_classes) { return t >= 0 && t < Cs && t != num_classes; }

__global__ __launch_bounds__(256) void px_semantic_fwd_kernel(const float* __restrict__ pred, const long long* __restrict__ sem,
                                                              const int* __restrict__ idx, int k, int kstride, int Cs, int P, int num_classes,
                                                              float* __restrict__ lse_out, float* __restrict__ lossj) {
  const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= k) return;
  const int p = idx[(long long)b * kstride + j];
  const float* x = pred + (long long)b * Cs * P + p;
  float m = -INFINITY;
  for (int c = 0; c < Cs; ++c) m = fmaxf(m, x[(long long)c * P]);
  float se = 0.f;
  for (int c = 0; c < Cs; ++c) se += expf(x[(long long)c * P] - m);
  const float lse = m + logf(se);
  const long long t = sem[(long long)b * P + p];
  lse_out[(long long)b * k + j] = lse;
  lossj[(long long)b * k + j] = px_sem_kept(t, Cs, num_classes) ? lse - x[t * P] : 0.f;
}

__global__ __launch_bounds__(256) void px_semantic_bwd_kernel(const float* __restrict__ grad, const float* __restrict__ pred,
                                                              const long long* __restrict__ sem, const int* __restrict__ idx, int B, int k,
                                                              int kstride, int Cs, int P, int num_classes, const float* __restrict__ lse_in,
                                                              const float* __restrict__ nnz, float* __restrict__ dpred) {
  const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= k) return;
  const int p = idx[(long long)b * kstride + j];
  const long long t = sem[(long long)b * P + p];
  if (!px_sem_kept(t, Cs, num_classes)) return;   // the gradient map is zero-filled
  const float w = grad[0] / ((float)B * fmaxf(nnz[b], 1.0f)), lse = lse_in[(long long)b * k + j];
  const float* x = pred + (long long)b * Cs * P + p;
  float* d = dpred + (long long)b * Cs * P + p;
  for (int c = 0; c < Cs; ++c) d[(long long)c * P] = w * (expf(x[(long long)c * P] - lse) - (c == t ? 1.f : 0.f));
}

}  // namespace axvs
