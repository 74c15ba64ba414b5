// Tube-Link's point-sampled training loss on the device: Mask2FormerVideoCCHeadTube.loss / loss_single / _get_target_single
// (MaXTron_Tube-Link/models/video/tube_link_vis/mask2former_video_cc_head.py:519-694) with mmdet's ClassificationCost,
// CrossEntropyLossCost, DiceCost (core/bbox/match_costs/match_cost.py:153-359), MaskHungarianAssigner, the uncertain-point selection
// (models/utils/point_sample.py:32-87), CrossEntropyLoss and the naive DiceLoss.
//
// All (layer, video) problems of a step go through a fixed number of launches on one stream, no host synchronisation and no copy:
//   forward  (5; the assignment is one launch per 256 problems, so 5 + ceil(L*B / 256) - 1 at most 8)
//     1 tl_cost_kernel         samples the Q predictions and M targets of a problem at its P shared points, 32 points a tile, and
//                              contracts x . g and sigmoid(x) . g over the points on the f32-input MFMA (32 x 32 output blocks, like
//                              axvs_matcher.h); row sums of softplus(x), sigmoid(x) and g.  A workgroup owns a point range and writes
//                              ONE set of partial sums.
//     2 tl_cost_finish_kernel  adds the partials in workgroup order (double), class term, cost [L*B][Q][M_max]
//     3 lsap_rect_kernel       the device assignment (axvs_lsap.h) through axvs_linear_sum_assignment_rect
//     4 tl_select_loss_kernel  one workgroup per matched pair: radix select of the k smallest |logit| among the S candidates (four 8-bit
//                              passes over the non-negative fp32 keys, nothing sorted, nothing stored: a candidate is sampled again in
//                              every pass), the kept points written in candidate order, then the pair's BCE and dice sums at its P points
//     5 tl_finish_kernel       one workgroup per layer: labels of the B*Q queries, weighted class cross-entropy, the three losses
//   backward (3)
//     1 tl_fill_zero_kernel    d_mask_preds = 0 (unmatched queries keep exactly that)
//     2 tl_scatter_kernel      one workgroup per matched pair: the transpose of the bilinear sampling without floating-point atomics
//     3 tl_cls_bwd_kernel      one wave per (layer, video, query) row of class logits
//
// Selection rule: the k candidates with the smallest |logit|; among candidates with EQUAL |logit| the lower candidate index is kept
// (the reference's topk leaves that order open).  The kept points are stored in increasing candidate order, which fixes the order of
// every later sum.
//
// Scatter order (tl_scatter_kernel): a pair's workgroup is the only writer of its query's gradient map.  It buckets the pair's P
// points by the long-image row of their upper taps (integer LDS counters), orders every bucket by point index (a rank count inside
// the bucket), and then adds the upper-row taps and, after a barrier, the lower-row taps: in either pass ONE thread owns a
// long-image row and walks that row's points in increasing point index, so every pixel is written by one thread at a time in a
// fixed order and two runs give the same bits.
#pragma once
#include "axvs_targets.h"

namespace axvs {

constexpr int kTLMaxPoints = 16384, kTLMaxCand = 65536;
constexpr int kTLMaxRows = 8192;          // T * h rows of the long image: the scatter kernel keeps two counters per row in LDS
constexpr int kTLTP = 32;                 // points per tile of the cost kernel
constexpr int kTLLDP = kTLTP + 1;         // LDS row stride (odd: the MFMA operand reads walk 32 rows at one point)
constexpr int kTLThreads = 1024;          // workgroup of the per-pair kernels

typedef float tl_f32x16 __attribute__((ext_vector_type(16)));

struct TLArgs {
  const float* cls[kMaxLayers];         // per layer: cls_scores [B][Q][K1]
  const float* masks[kMaxLayers];       // per layer: mask_preds [B][T][Q][h][w]
  float* dcls[kMaxLayers];
  float* dmasks[kMaxLayers];
  int m[kMaxVideos];                    // objects of video b
  int off[kMaxVideos];                  // first row of video b in the concatenated targets / labels
  int goff[kMaxVideos + 1];             // first matched pair of video b in a layer's pair list: sum of min(Q, M_b') over b' < b
};

struct TLShape {
  int L, B, Q, K1, T, h, w, Hg, Wg, P, S, k, G, Mmax, kmax;
  float cost_cls, cost_mask, cost_dice, loss_cls, loss_mask, loss_dice, eps;
};

// what the forward keeps for the backward: O(L * G * P)
struct TLSaved {
  int* pairs;          // [L][G][2]: b * Q + q, row of the concatenated targets
  float* pairsum;      // [L][G][4]: BCE sum, sum s*g, sum s + sum g, unused
  float* chosen;       // [L][G][P][2]: the k kept candidates in candidate order, then the P - k random points
  int* labels;         // [L][B][Q]
  float* avg;          // [L]: sum of class_weight[labels]
};

// ---- point sampling: mmcv.ops.point_sample = F.grid_sample(input, 2 p - 1, 'bilinear', 'zeros', align_corners=False) --------------------
// taps of a point on a W x R image; a tap outside the image has weight zero.  x0 is in [-1, W-1] and y0 in [-1, R-1] always.
struct Bilin {
  int x0, y0;
  float wx0, wx1, wy0, wy1;
};
__device__ __forceinline__ void tl_axis(float p, int n, int& i0, float& w0, float& w1) {
  const float g = 2.f * p - 1.f;
  const float x = ((g + 1.f) * (float)n - 1.f) * 0.5f;        // grid_sampler_unnormalize, align_corners = False
  float f = floorf(x);
  w1 = x - f;
  w0 = 1.f - w1;
  if (!(f >= -1.f && f <= (float)(n - 1))) { f = -1.f; w0 = 0.f; w1 = 0.f; }      // (NaN lands here as well)
  i0 = (int)f;
  if (i0 < 0) w0 = 0.f;
  if (i0 + 1 >= n) w1 = 0.f;
}
__device__ __forceinline__ Bilin tl_taps(float px, float py, int W, int R) {
  Bilin t;
  tl_axis(px, W, t.x0, t.wx0, t.wx1);
  tl_axis(py, R, t.y0, t.wy0, t.wy1);
  return t;
}
// prediction of one query: row r of its long image is line r % h of frame r / h; frames are `fs` = Q * h * w floats apart
__device__ __forceinline__ float tl_sample_pred(const float* __restrict__ base, const Bilin& t, int h, int w, int R, long long fs) {
  float v = 0.f;
  const bool xa = t.x0 >= 0, xb = t.x0 + 1 < w;
  if (t.y0 >= 0) {
    const float* row = base + (long long)(t.y0 / h) * fs + (t.y0 % h) * w;
    if (xa) v += row[t.x0] * (t.wx0 * t.wy0);
    if (xb) v += row[t.x0 + 1] * (t.wx1 * t.wy0);
  }
  if (t.y0 + 1 < R) {
    const int y1 = t.y0 + 1;
    const float* row = base + (long long)(y1 / h) * fs + (y1 % h) * w;
    if (xa) v += row[t.x0] * (t.wx0 * t.wy1);
    if (xb) v += row[t.x0 + 1] * (t.wx1 * t.wy1);
  }
  return v;
}
// target mask: contiguous [T * Hg][Wg] from element `base`
template <int TDT>
__device__ __forceinline__ float tl_sample_target(const void* __restrict__ tg, long long base, const Bilin& t, int W, int R) {
  float v = 0.f;
  const bool xa = t.x0 >= 0, xb = t.x0 + 1 < W;
  if (t.y0 >= 0) {
    const long long row = base + (long long)t.y0 * W;
    if (xa) v += load_f32<TDT>(tg, row + t.x0) * (t.wx0 * t.wy0);
    if (xb) v += load_f32<TDT>(tg, row + t.x0 + 1) * (t.wx1 * t.wy0);
  }
  if (t.y0 + 1 < R) {
    const long long row = base + (long long)(t.y0 + 1) * W;
    if (xa) v += load_f32<TDT>(tg, row + t.x0) * (t.wx0 * t.wy1);
    if (xb) v += load_f32<TDT>(tg, row + t.x0 + 1) * (t.wx1 * t.wy1);
  }
  return v;
}

__device__ __forceinline__ float tl_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float tl_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// floats of one workgroup's partial sums: x.g [Qp][Mp], s.g [Qp][Mp], sum s [Qp], sum softplus [Qp], sum g [Mp] (Qp, Mp: Q, M_max rounded up to 32)
__host__ __device__ inline long long tl_part_stride(int Qp, int Mp) { return 2ll * Qp * Mp + 2ll * Qp + Mp; }

// grid (npb, Qp / 32, L * B), 256 threads.  Dynamic LDS: rows x (32), sigmoid (32), softplus (32), targets (M rounded up to 32) of a tile.
template <int TDT>
__global__ __launch_bounds__(256) void tl_cost_kernel(TLArgs a, const void* __restrict__ targets, const float* __restrict__ match_coords,
                                                      TLShape s, int tiles_per_wg, float* __restrict__ part) {
  extern __shared__ float tsm[];
  __shared__ float sacc[64 + kMaxObjects];      // running sums of the sigmoid, softplus and target rows, in LDS row order
  const int z = blockIdx.z, l = z / s.B, b = z - l * s.B;
  const int M = a.m[b];
  if (M <= 0) return;
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6, qb = blockIdx.y;
  const int Qp = (s.Q + 31) & ~31, Mpm = (s.Mmax + 31) & ~31, Mp = (M + 31) & ~31, nmb = Mp >> 5;
  float* xs = tsm;
  float* sg = xs + 32 * kTLLDP;
  float* gs = sg + 64 * kTLLDP;
  const int R = s.T * s.h, Rg = s.T * s.Hg;
  const long long fs = (long long)s.Q * s.h * s.w, tsz = (long long)Rg * s.Wg;
  const float* pbase = a.masks[l] + (long long)b * s.T * fs;
  const float* coords = match_coords + (long long)z * s.P * 2;
  for (int i = tid; i < 64 + kMaxObjects; i += 256) sacc[i] = 0.f;
  tl_f32x16 acc1[4], acc2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    for (int r = 0; r < 16; ++r) { acc1[k][r] = 0.f; acc2[k][r] = 0.f; }
  __syncthreads();

  const int ntiles = (s.P + kTLTP - 1) / kTLTP;
  const int t0 = blockIdx.x * tiles_per_wg, t1 = t0 + tiles_per_wg < ntiles ? t0 + tiles_per_wg : ntiles;
  const int pl = tid & 31, rr = tid >> 5;
  for (int tile = t0; tile < t1; ++tile) {
    const int p = tile * kTLTP + pl;
    const bool ok = p < s.P;
    Bilin tp, tg;
    if (ok) {
      const float px = coords[2 * p], py = coords[2 * p + 1];
      tp = tl_taps(px, py, s.w, R);
      tg = tl_taps(px, py, s.Wg, Rg);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int qr = rr + 8 * i, q = qb * 32 + qr;
      const bool v = ok && q < s.Q;
      const float x = v ? tl_sample_pred(pbase + (long long)q * s.h * s.w, tp, s.h, s.w, R, fs) : 0.f;
      xs[qr * kTLLDP + pl] = x;
      sg[qr * kTLLDP + pl] = v ? tl_sigmoid(x) : 0.f;
      sg[(32 + qr) * kTLLDP + pl] = v ? tl_softplus(x) : 0.f;
    }
    for (int m = rr; m < Mp; m += 8)
      gs[m * kTLLDP + pl] = (ok && m < M) ? tl_sample_target<TDT>(targets, (a.off[b] + m) * tsz, tg, s.Wg, Rg) : 0.f;
    __syncthreads();
    for (int r = tid; r < 64 + Mp; r += 256) {
      const float* row = sg + r * kTLLDP;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
      for (int c = 0; c < kTLTP; c += 4) { s0 += row[c]; s1 += row[c + 1]; s2 += row[c + 2]; s3 += row[c + 3]; }
      sacc[r] += (s0 + s1) + (s2 + s3);
    }
    // A[i = q][k = point], B[k = point][j = m], two points per MFMA; the x and the sigmoid contraction share the target operand
    const float* ap = xs + (lane & 31) * kTLLDP + (lane >> 5);
    const float* sp = sg + (lane & 31) * kTLLDP + (lane >> 5);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int mb = g + 4 * k;
      if (mb < nmb) {
        const float* bp = gs + (mb * 32 + (lane & 31)) * kTLLDP + (lane >> 5);
#pragma unroll 8
        for (int c = 0; c < kTLTP; c += 2) {
          const float bv = bp[c];
          acc1[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[c], bv, acc1[k], 0, 0, 0);
          acc2[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(sp[c], bv, acc2[k], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  float* pw = part + ((long long)z * gridDim.x + blockIdx.x) * tl_part_stride(Qp, Mpm);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int mb = g + 4 * k;
    if (mb < nmb) {
      const int m = mb * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int q = qb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (q < s.Q && m < M) {
          pw[(long long)q * Mpm + m] = acc1[k][r];
          pw[(long long)Qp * Mpm + (long long)q * Mpm + m] = acc2[k][r];
        }
      }
    }
  }
  float* pr = pw + 2ll * Qp * Mpm;
  for (int q = tid; q < 32; q += 256) {
    if (qb * 32 + q < s.Q) {
      pr[qb * 32 + q] = sacc[q];
      pr[Qp + qb * 32 + q] = sacc[32 + q];
    }
  }
  if (qb == 0)
    for (int m = tid; m < M; m += 256) pr[2 * Qp + m] = sacc[64 + m];
}

// partials -> cost fp32 [L * B][Q][Mmax] (columns m >= M of a problem are zero).  grid (ceil(Q * Mmax / 256), L * B)
__global__ __launch_bounds__(256) void tl_cost_finish_kernel(TLArgs a, const float* __restrict__ part, int npb, const long long* __restrict__ labels,
                                                             TLShape s, float* __restrict__ cost) {
  const int idx = blockIdx.x * 256 + threadIdx.x, z = blockIdx.y;
  if (idx >= s.Q * s.Mmax) return;
  const int q = idx / s.Mmax, m = idx - q * s.Mmax, l = z / s.B, b = z - l * s.B;
  const long long o = (long long)z * s.Q * s.Mmax + idx;
  if (m >= a.m[b]) { cost[o] = 0.f; return; }
  const int Qp = (s.Q + 31) & ~31, Mpm = (s.Mmax + 31) & ~31;
  const long long stride = tl_part_stride(Qp, Mpm);
  const float* pw = part + (long long)z * npb * stride;
  double xg = 0.0, sgm = 0.0, ss = 0.0, sp = 0.0, gg = 0.0;
  for (int w = 0; w < npb; ++w, pw += stride) {
    xg += (double)pw[(long long)q * Mpm + m];
    sgm += (double)pw[(long long)Qp * Mpm + (long long)q * Mpm + m];
    ss += (double)pw[2ll * Qp * Mpm + q];
    sp += (double)pw[2ll * Qp * Mpm + Qp + q];
    gg += (double)pw[2ll * Qp * Mpm + 2 * Qp + m];
  }
  // softplus(x) - softplus(-x) = x: sum_p softplus(-x) g + softplus(x) (1 - g) = sum_p softplus(x) - sum_p x g
  const float bce = ((float)sp - (float)xg) / (float)s.P;
  const float dice = 1.f - (2.f * (float)sgm + s.eps) / ((float)ss + (float)gg + s.eps);
  long long lab = labels[a.off[b] + m];
  lab = lab < 0 ? 0 : (lab > s.K1 - 2 ? s.K1 - 2 : lab);          // (the reference raises on a label outside 0 .. K-1; here it is clamped)
  const float* x = a.cls[l] + ((long long)b * s.Q + q) * s.K1;
  float mx = x[0];
  for (int c = 1; c < s.K1; ++c) mx = fmaxf(mx, x[c]);
  float se = 0.f;
  for (int c = 0; c < s.K1; ++c) se += expf(x[c] - mx);
  const float prob = expf(x[lab] - mx) / se;
  cost[o] = -prob * s.cost_cls + bce * s.cost_mask + dice * s.cost_dice;
}

// the matched pair `g` of layer `l`: video, query, target row (q < 0: the assignment left the slot empty, which it never does)
struct TLPair { int b, q, tm; };
__device__ __forceinline__ TLPair tl_pair_of(const TLArgs& a, const TLShape& s, const long long* __restrict__ rows, const long long* __restrict__ cols, int l, int g) {
  int b = 0;
  while (b + 1 < s.B && g >= a.goff[b + 1]) ++b;
  const long long i = (long long)(l * s.B + b) * s.kmax + (g - a.goff[b]);
  const long long r = rows[i], c = cols[i];
  return TLPair{b, (r >= 0 && c >= 0) ? (int)r : -1, a.off[b] + (int)(c >= 0 ? c : 0)};
}

// sum of v over the workgroup in a fixed order (wave reduction, then the waves in order); every thread gets the result.  `red`: one float per wave
__device__ __forceinline__ float tl_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
  return t;
}

// grid (G, L), kTLThreads threads: selection of the pair's points, then its loss sums
template <int TDT>
__global__ __launch_bounds__(kTLThreads) void tl_select_loss_kernel(TLArgs a, const void* __restrict__ targets, const long long* __restrict__ rows,
                                                                    const long long* __restrict__ cols, const float* __restrict__ cand_coords,
                                                                    const float* __restrict__ rand_coords, TLShape s, TLSaved sv, int* __restrict__ sel_idx) {
  __shared__ int hist[256];
  __shared__ unsigned sh_prefix;
  __shared__ int sh_need;
  __shared__ int wtot[2][kTLThreads / 64][2];
  __shared__ float red[kTLThreads / 64];
  const int g = blockIdx.x, l = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long pi = (long long)l * s.G + g;
  const TLPair pr = tl_pair_of(a, s, rows, cols, l, g);
  float* chosen = sv.chosen + pi * s.P * 2;
  if (pr.q < 0) {                                    // uniform over the workgroup
    for (int i = tid; i < 2 * s.P; i += kTLThreads) chosen[i] = 0.f;
    if (tid == 0) { sv.pairs[2 * pi] = -1; sv.pairs[2 * pi + 1] = 0; }
    if (tid < 4) sv.pairsum[4 * pi + tid] = 0.f;
    return;
  }
  const int R = s.T * s.h, Rg = s.T * s.Hg;
  const long long fs = (long long)s.Q * s.h * s.w;
  const float* pm = a.masks[l] + ((long long)pr.b * s.T * s.Q + pr.q) * s.h * s.w;
  const float* cand = cand_coords + pi * s.S * 2;
  auto key_of = [&](int i) -> unsigned {
    const Bilin t = tl_taps(cand[2 * i], cand[2 * i + 1], s.w, R);
    return __float_as_uint(fabsf(tl_sample_pred(pm, t, s.h, s.w, R, fs)));
  };

  if (s.k > 0) {
    // the k-th smallest key, 8 bits a pass from the top: `prefix` holds the bits decided so far, `need` the rank among the keys under it
    unsigned prefix = 0;
    int need = s.k;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for (int i = tid; i < s.S; i += kTLThreads) {
        const unsigned key = key_of(i);
        if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1);
      }
      __syncthreads();
      if (tid == 0) {
        int cum = 0, d = 0;
        for (; d < 255; ++d) {
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
    // keep: every key below the threshold, and the first `need` candidates (by index) at it; written in candidate order
    const unsigned thr = prefix;
    int base_lt = 0, base_eq = 0;
    for (int i0 = 0, it = 0; i0 < s.S; i0 += kTLThreads, ++it) {
      const int i = i0 + tid;
      const bool in = i < s.S;
      const unsigned key = in ? key_of(i) : 0xffffffffu;
      const bool lt = in && key < thr, eq = in && key == thr;
      const unsigned long long mlt = __ballot(lt), meq = __ballot(eq);
      const unsigned long long below = (1ull << lane) - 1ull;
      if (lane == 0) { wtot[it & 1][wv][0] = __popcll(mlt); wtot[it & 1][wv][1] = __popcll(meq); }
      __syncthreads();
      int lt_before = __popcll(mlt & below), eq_before = __popcll(meq & below), tot_lt = 0, tot_eq = 0;
      for (int w = 0; w < kTLThreads / 64; ++w) {
        const int c0 = wtot[it & 1][w][0], c1 = wtot[it & 1][w][1];
        if (w < wv) { lt_before += c0; eq_before += c1; }
        tot_lt += c0;
        tot_eq += c1;
      }
      const int eqr = base_eq + eq_before;
      if (lt || (eq && eqr < need)) {
        const int pos = base_lt + lt_before + (eqr < need ? eqr : need);
        if (pos < s.k) {
          chosen[2 * pos] = cand[2 * i];
          chosen[2 * pos + 1] = cand[2 * i + 1];
          if (sel_idx) sel_idx[pi * s.k + pos] = i;
        }
      }
      base_lt += tot_lt;
      base_eq += tot_eq;
    }
  }
  const float* rnd = rand_coords + pi * (s.P - s.k) * 2;
  for (int i = tid; i < 2 * (s.P - s.k); i += kTLThreads) chosen[2 * s.k + i] = rnd[i];
  __syncthreads();                                   // the workgroup reads back the points it has just written

  const long long tbase = (long long)pr.tm * Rg * s.Wg;
  float bce = 0.f, sa = 0.f, sb = 0.f, sc = 0.f;
  for (int p = tid; p < s.P; p += kTLThreads) {
    const float px = chosen[2 * p], py = chosen[2 * p + 1];
    const float x = tl_sample_pred(pm, tl_taps(px, py, s.w, R), s.h, s.w, R, fs);
    const float t = tl_sample_target<TDT>(targets, tbase, tl_taps(px, py, s.Wg, Rg), s.Wg, Rg);
    const float sgm = tl_sigmoid(x);
    bce += tl_softplus(x) - x * t;
    sa += sgm * t;
    sb += sgm;
    sc += t;
  }
  bce = tl_block_sum(bce, red);
  sa = tl_block_sum(sa, red);
  sb = tl_block_sum(sb, red);
  sc = tl_block_sum(sc, red);
  if (tid == 0) {
    sv.pairs[2 * pi] = pr.b * s.Q + pr.q;
    sv.pairs[2 * pi + 1] = pr.tm;
    sv.pairsum[4 * pi] = bce;
    sv.pairsum[4 * pi + 1] = sa;
    sv.pairsum[4 * pi + 2] = sb + sc;
    sv.pairsum[4 * pi + 3] = 0.f;
  }
}

// grid (L), 256 threads: the labels of the layer's B * Q queries, then losses[l] = (loss_cls, loss_mask, loss_dice)
__global__ __launch_bounds__(256) void tl_finish_kernel(TLArgs a, const long long* __restrict__ labels, const float* __restrict__ class_weight,
                                                        const float* __restrict__ num_total_masks, TLShape s, TLSaved sv, float* __restrict__ losses) {
  __shared__ float red[4];
  const int l = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nrows = s.B * s.Q;
  int* lab = sv.labels + (long long)l * nrows;
  for (int i = tid; i < nrows; i += 256) lab[i] = s.K1 - 1;            // unmatched: the background class
  __syncthreads();
  for (int g = tid; g < s.G; g += 256) {
    const long long pi = (long long)l * s.G + g;
    const int row = sv.pairs[2 * pi];
    if (row < 0) continue;
    long long y = labels[sv.pairs[2 * pi + 1]];
    y = y < 0 ? 0 : (y > s.K1 - 2 ? s.K1 - 2 : y);
    lab[row] = (int)y;
  }
  __syncthreads();
  // mmdet's CrossEntropyLoss with class_weight: sum_i w[y_i] * -log softmax(x_i)[y_i] / (sum_i w[y_i] + eps32)
  float num = 0.f, den = 0.f;
  for (int row = wv; row < nrows; row += 4) {
    const float* x = a.cls[l] + (long long)row * s.K1;
    float mx = -__builtin_huge_valf();
    for (int c = lane; c < s.K1; c += 64) mx = fmaxf(mx, x[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float se = 0.f;
    for (int c = lane; c < s.K1; c += 64) se += expf(x[c] - mx);
    se = wave_sum(se);
    const int y = lab[row];
    const float w = class_weight[y];
    num += w * (mx + logf(se) - x[y]);
    den += w;
  }
  if (lane != 0) { num = 0.f; den = 0.f; }
  num = tl_block_sum(num, red);
  den = tl_block_sum(den, red);
  float sb = 0.f, sd = 0.f;
  for (int g = tid; g < s.G; g += 256) {
    const float* ps = sv.pairsum + 4 * ((long long)l * s.G + g);
    if (sv.pairs[2 * ((long long)l * s.G + g)] < 0) continue;
    sb += ps[0];
    sd += 1.f - (2.f * ps[1] + s.eps) / (ps[2] + s.eps);
  }
  sb = tl_block_sum(sb, red);
  sd = tl_block_sum(sd, red);
  if (tid == 0) {
    const float ntm = num_total_masks[0];
    sv.avg[l] = den;
    losses[3 * l] = s.loss_cls * (num / (den + 1.1920928955078125e-07f));
    losses[3 * l + 1] = s.G > 0 ? s.loss_mask * (sb / (ntm * (float)s.P + 1.1920928955078125e-07f)) : 0.f;
    losses[3 * l + 2] = s.G > 0 ? s.loss_dice * (sd / (ntm + 1.1920928955078125e-07f)) : 0.f;
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------
// grid (chunks, L): d_mask_preds[l] = 0
__global__ __launch_bounds__(256) void tl_fill_zero_kernel(TLArgs a, long long n) {
  float* d = a.dmasks[blockIdx.y];
  if (!d) return;
  const long long n4 = n >> 2, step = (long long)gridDim.x * 256;
  float4* d4 = reinterpret_cast<float4*>(d);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += step) d4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (long long i = (n4 << 2) + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) d[i] = 0.f;
}

// one wave per (layer, video, query) row: d_cls = g_cls * loss_weight * w[y] / avg * (softmax - onehot)
__global__ __launch_bounds__(256) void tl_cls_bwd_kernel(TLArgs a, const float* __restrict__ grad_losses, const float* __restrict__ class_weight,
                                                         TLShape s, TLSaved sv, long long total) {
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= total) return;
  const int nrows = s.B * s.Q, l = (int)(r / nrows), row = (int)(r - (long long)l * nrows);
  float* d = a.dcls[l];
  if (!d) return;
  const float* x = a.cls[l] + (long long)row * s.K1;
  d += (long long)row * s.K1;
  float mx = -__builtin_huge_valf();
  for (int c = lane; c < s.K1; c += 64) mx = fmaxf(mx, x[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float se = 0.f;
  for (int c = lane; c < s.K1; c += 64) se += expf(x[c] - mx);
  se = wave_sum(se);
  const int y = sv.labels[(long long)l * nrows + row];
  const float coef = grad_losses[3 * l] * s.loss_cls * class_weight[y] / (sv.avg[l] + 1.1920928955078125e-07f);
  for (int c = lane; c < s.K1; c += 64) d[c] = coef * (expf(x[c] - mx) / se - (c == y ? 1.f : 0.f));
}

// grid (G, L), kTLThreads threads.  Dynamic LDS: int cnt[R + 1], int start[R + 2], u16 list[P], u16 sorted[P]
template <int TDT>
__global__ __launch_bounds__(kTLThreads) void tl_scatter_kernel(TLArgs a, const void* __restrict__ targets, const float* __restrict__ grad_losses,
                                                                const float* __restrict__ num_total_masks, TLShape s, TLSaved sv) {
  extern __shared__ int ssm[];
  __shared__ int wsum[kTLThreads / 64];
  const int g = blockIdx.x, l = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float* dm = a.dmasks[l];
  if (!dm) return;
  const long long pi = (long long)l * s.G + g;
  const int prow = sv.pairs[2 * pi];
  if (prow < 0) return;
  const int b = prow / s.Q, q = prow - b * s.Q;
  const int R = s.T * s.h, Rg = s.T * s.Hg, nbk = R + 1;
  int* cnt = ssm;
  int* start = cnt + nbk;
  unsigned short* list = reinterpret_cast<unsigned short*>(start + nbk + 1);
  unsigned short* sorted = list + s.P;
  const long long fs = (long long)s.Q * s.h * s.w;
  const long long qoff = ((long long)b * s.T * s.Q + q) * s.h * s.w;
  const float* pm = a.masks[l] + qoff;
  dm += qoff;
  const long long tbase = (long long)sv.pairs[2 * pi + 1] * Rg * s.Wg;
  const float* coords = sv.chosen + pi * s.P * 2;
  const float ntm = num_total_masks[0];
  const float gm = grad_losses[3 * l + 1] * s.loss_mask / (ntm * (float)s.P + 1.1920928955078125e-07f);
  const float gd = grad_losses[3 * l + 2] * s.loss_dice / (ntm + 1.1920928955078125e-07f);
  const float den = sv.pairsum[4 * pi + 2] + s.eps, numr = 2.f * sv.pairsum[4 * pi + 1] + s.eps;
  auto bucket_of = [&](int p) -> int {
    int y0;
    float w0, w1;
    tl_axis(coords[2 * p + 1], R, y0, w0, w1);
    return y0 + 1;                                   // 0 .. R
  };

  for (int i = tid; i < nbk; i += kTLThreads) cnt[i] = 0;
  __syncthreads();
  for (int p = tid; p < s.P; p += kTLThreads) atomicAdd(&cnt[bucket_of(p)], 1);
  __syncthreads();
  // exclusive scan of the bucket sizes: a contiguous run of buckets per thread, a wave scan of the run totals, the waves in order
  const int per = (nbk + kTLThreads - 1) / kTLThreads, r0 = tid * per, r1 = r0 + per < nbk ? r0 + per : nbk;
  int mine = 0;
  for (int r = r0; r < r1; ++r) mine += cnt[r];
  int inc = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  int run = inc - mine;
  for (int w = 0; w < wv; ++w) run += wsum[w];
  for (int r = r0; r < r1; ++r) {
    start[r] = run;
    run += cnt[r];
  }
  if (tid == kTLThreads - 1) start[nbk] = run;
  __syncthreads();
  for (int i = tid; i < nbk; i += kTLThreads) cnt[i] = 0;
  __syncthreads();
  for (int p = tid; p < s.P; p += kTLThreads) {
    const int r = bucket_of(p);
    list[start[r] + atomicAdd(&cnt[r], 1)] = (unsigned short)p;
  }
  __syncthreads();
  // the order inside a bucket came from the hardware: put every point at its rank by point index
  for (int i = tid; i < s.P; i += kTLThreads) {
    const int p = list[i], r = bucket_of(p);
    int rank = 0;
    for (int j = start[r]; j < start[r + 1]; ++j) rank += list[j] < p;
    sorted[start[r] + rank] = (unsigned short)p;
  }
  __syncthreads();

  for (int pass = 0; pass < 2; ++pass) {             // 0: the upper taps (row y0), 1: the lower taps (row y0 + 1)
    for (int r = tid; r < nbk; r += kTLThreads) {
      const int rowi = r - 1 + pass;
      if (rowi < 0 || rowi >= R) continue;
      float* rowp = dm + (long long)(rowi / s.h) * fs + (rowi % s.h) * s.w;
      for (int j = start[r]; j < start[r + 1]; ++j) {
        const int p = sorted[j];
        const float px = coords[2 * p], py = coords[2 * p + 1];
        const Bilin tp = tl_taps(px, py, s.w, R);
        const float x = tl_sample_pred(pm, tp, s.h, s.w, R, fs);
        const float t = tl_sample_target<TDT>(targets, tbase, tl_taps(px, py, s.Wg, Rg), s.Wg, Rg);
        const float sgm = tl_sigmoid(x);
        // d/dx of BCE-with-logits and of 1 - (2 sum s g + eps) / (sum s + sum g + eps)
        const float coef = gm * (sgm - t) + gd * (numr / (den * den) - 2.f * t / den) * sgm * (1.f - sgm);
        const float wy = pass ? tp.wy1 : tp.wy0;
        if (tp.x0 >= 0) rowp[tp.x0] += coef * (tp.wx0 * wy);
        if (tp.x0 + 1 < s.w) rowp[tp.x0 + 1] += coef * (tp.wx1 * wy);
      }
    }
    __syncthreads();
  }
}

}  // namespace axvs
