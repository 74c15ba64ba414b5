// The set criterion of the Video-kMaX models on the device: the `labels` and `masks` losses of MaXTronCCSetCriterion /
// MaXTronWCSetCriterion (MaXTron_Video-kMaX/maxtron_deeplab/modeling/cc_criterion.py:144-200, :237-266, :338-412) and their
// gradients, on top of the matcher's device indices (axvs_matcher.h).
//
// Per (layer l, video b) problem z = l * B + b, x = pred_masks [N][P], P = T*H*W, and the matching zm = share ? b : z:
//   t[n][:]   = targets[inv[zm][n]] for a matched query, 0 otherwise           (the padded target tensor is never materialised)
//   void[p]   = sum_n t[n][p] < 1,   keep[p] = !(masking && void[p]),   prob = softmax_n(x)
//   ce[p]     = keep[p] * -sum_n t[n][p] log_softmax_n(x)[n][p];   loss_mask = mean_b sum_p ce / max(#{ce != 0}, 1)
//   loss_dice = mean_b sum_n (1 - (2 I_n + 1) / (Q_n + T_n + 1)) w_mask[n] * 0.75 / N,   I = sum_p keep prob t,  Q = sum_p keep prob,  T = sum_p t
//   w_cls[n]  = matched dice, or the void IoU sum_p prob void / (sum_p prob + 1e-5) of an unmatched query, clamped at 1e-5
//   loss_ce   = mean_b sum_n alpha_n w_cls[n] CE(pred_logits[n], label[n]) / max(#nonzero, 1),   alpha = 0.75 (0.25 for the void class)
//
// criterion_index_kernel   matcher pairs -> inverse map [LM*B][N] (target row or -1), w_mask, the matched part of w_cls and label
// criterion_fwd_kernel     ONE launch for all problems; reads pred_masks once and the mapped targets once per layer.  A workgroup owns a
//                          contiguous pixel range: lane = pixel of a 64-pixel tile, wave g holds queries g, g + 4, ...  The wave keeps its
//                          part of a pixel's query column in registers from the load to the accumulation (one exp per element), the four
//                          waves exchange (max, sum of exp, sum t, sum t x) through LDS with ONE barrier per tile (two exchange buffers),
//                          and the per-query pixel sums are per-lane running sums reduced across lanes once per workgroup.  N > 128 does
//                          not fit the register column: criterion_fwd_any_kernel re-reads the tile (from L2) and reduces per tile.
// criterion_finish_kernel  adds the workgroups' partial sums in workgroup order in double (no atomics anywhere: results are run-to-run
//                          identical), computes w_cls, the class loss and the three scalars of a layer, saves O(L*B*N) values.
// criterion_bwd_kernel     recomputes the softmax per pixel and writes d pred_masks once:
//                          d x[n][p] = keep[p] (gm (prob ts - t) + prob (u[n][p] - sum_n' prob[n'] u[n'][p])),  u = ca[n] + cb[n] t[n][p],
//                          gm = g_mask / (B count_b), ca / cb the dice coefficients of the saved sums times g_dice 0.75 / (N B)
//                          (zero for an unmatched query).  The upstream gradients of the 3 L scalars are read from device memory.
// criterion_logits_bwd_kernel   d pred_logits, one wave per query row.
#pragma once
#include "axvs_targets.h"

namespace axvs {

constexpr int kCritNPW = 32;          // queries per wave of the register-column kernels: N <= 4 * 32
constexpr int kCritTP = 64;           // pixels per tile, one per lane

struct CritArgs {
  const float* masks[kMaxLayers];     // per layer: pred_masks fp32 [B][N][P]
  const float* logits[kMaxLayers];    // per layer: pred_logits fp32 [B][N][K1]
  float* dmasks[kMaxLayers];          // backward: d pred_masks (NULL: skipped)
  float* dlogits[kMaxLayers];         // backward: d pred_logits (NULL: skipped)
  int m[kMaxVideos];
  int off[kMaxVideos];
};

// what the forward saves for the backward, all O(L * B * N): views into one caller-owned buffer of crit_saved_words() 4-byte words
struct CritSaved {
  int* inv;        // [L*B][N]  target row (in the concatenated targets) of query n under matching zm, or -1
  float* wmask;    // [L*B][N]  by zm
  float* mdice;    // [L*B][N]  by zm: matched dice (0 unmatched)
  int* mlabel;     // [L*B][N]  by zm: matched label (K1 - 1 unmatched)
  float* sums;     // [L*B][3][N]  I, Q (masked), T
  float* wcls;     // [L*B][N]
  int* label;      // [L*B][N]
  float* cnt;      // [L*B][2]  nonzero counts of the mask loss and the class loss, each at least 1
};
__host__ __device__ inline long long crit_saved_words(int L, int B, int N) { return (long long)L * B * (9ll * N + 2); }
__host__ __device__ inline CritSaved crit_saved_views(void* base, int L, int B, int N) {
  const long long n = (long long)L * B * N;
  float* f = static_cast<float*>(base);
  CritSaved s;
  s.inv = reinterpret_cast<int*>(f);
  s.wmask = f + n;
  s.mdice = f + 2 * n;
  s.mlabel = reinterpret_cast<int*>(f + 3 * n);
  s.sums = f + 4 * n;
  s.wcls = f + 7 * n;
  s.label = reinterpret_cast<int*>(f + 8 * n);
  s.cnt = f + 9 * n;
  return s;
}
// floats of one workgroup's partial sums: A = sum prob void, Bq = sum prob (1 - void), I, T per query, then (sum ce, #{ce != 0})
__host__ __device__ inline long long crit_part_stride(int N) { return 4ll * N + 2; }

// grid LM * B, 256 threads
__global__ __launch_bounds__(256) void criterion_index_kernel(CritArgs a, const long long* __restrict__ rows, const long long* __restrict__ cols,
                                                              const float* __restrict__ dice, const float* __restrict__ cls,
                                                              const long long* __restrict__ labels, int B, int N, int K1, int kmax, CritSaved s) {
  const int zm = blockIdx.x, b = zm % B;
  const long long o = (long long)zm * N;
  for (int n = threadIdx.x; n < N; n += 256) {
    s.inv[o + n] = -1;
    s.wmask[o + n] = 0.f;
    s.mdice[o + n] = 0.f;
    s.mlabel[o + n] = K1 - 1;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kmax; i += 256) {
    const long long r = rows[(long long)zm * kmax + i], c = cols[(long long)zm * kmax + i];
    if (r < 0 || c < 0 || r >= N || c >= a.m[b]) continue;
    long long lab = labels[a.off[b] + c];
    lab = lab < 0 ? 0 : (lab > K1 - 2 ? K1 - 2 : lab);        // (the reference raises on a label outside 0 .. K-1; clamped as the matcher does)
    s.inv[o + r] = a.off[b] + (int)c;
    s.wmask[o + r] = fmaxf(cls[(long long)zm * kmax + i], 1e-5f);
    s.mdice[o + r] = dice[(long long)zm * kmax + i];
    s.mlabel[o + r] = (int)lab;
  }
}

// the four waves' (max, sum of exp relative to that max, two more sums) of a pixel -> the pixel's values; ONE barrier, the buffer
// alternates by tile so that a wave writing tile i + 1 does not meet a wave still reading tile i
struct CritPixel { float mx, se, s2, s3, f; };   // f: what this wave's exp(x - its max) is multiplied by to give the probability
__device__ __forceinline__ CritPixel crit_exchange(float (*sx)[4][kCritTP], int g, int lane, float mx, float se, float s2, float s3, bool scale3) {
  sx[g][0][lane] = mx;
  sx[g][1][lane] = se;
  sx[g][2][lane] = s2;
  sx[g][3][lane] = s3;
  __syncthreads();
  CritPixel r;
  r.mx = fmaxf(fmaxf(sx[0][0][lane], sx[1][0][lane]), fmaxf(sx[2][0][lane], sx[3][0][lane]));
  r.se = 0.f;
  r.s2 = 0.f;
  r.s3 = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const float k = expf(sx[w][0][lane] - r.mx);
    r.se += sx[w][1][lane] * k;
    r.s2 += sx[w][2][lane];
    r.s3 += scale3 ? sx[w][3][lane] * k : sx[w][3][lane];
  }
  r.f = expf(mx - r.mx) / r.se;
  return r;
}

__device__ __forceinline__ void crit_tile_range(long long P, int tiles_per_wg, long long& t0, long long& t1) {
  const long long ntiles = (P + kCritTP - 1) / kCritTP;
  t0 = (long long)blockIdx.x * tiles_per_wg;
  t1 = t0 + tiles_per_wg < ntiles ? t0 + tiles_per_wg : ntiles;
}

// grid (npb, L * B), 256 threads, N <= 128
template <int TDT>
__global__ __launch_bounds__(256, 2) void criterion_fwd_kernel(CritArgs a, const void* __restrict__ targets, const int* __restrict__ inv, int B, int N,
                                                            long long P, int tiles_per_wg, int masking, int share, float* __restrict__ part) {
  __shared__ float sx[2][4][4][kCritTP];
  __shared__ int sinv[4 * kCritNPW];
  const int z = blockIdx.y, l = z / B, b = z - l * B, zm = share ? b : z;
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  for (int n = tid; n < 4 * kCritNPW; n += 256) sinv[n] = n < N ? inv[(long long)zm * N + n] : -1;
  __syncthreads();
  const float* x0 = a.masks[l] + (long long)b * N * P;
  float x[kCritNPW], sA[kCritNPW], sB[kCritNPW], sI[kCritNPW], sT[kCritNPW];
#pragma unroll
  for (int j = 0; j < kCritNPW; ++j) { sA[j] = 0.f; sB[j] = 0.f; sI[j] = 0.f; sT[j] = 0.f; }
  float sce = 0.f, scnt = 0.f;
  long long t0, t1;
  crit_tile_range(P, tiles_per_wg, t0, t1);
  for (long long tile = t0; tile < t1; ++tile) {
    const long long pix = tile * kCritTP + lane;
    const bool ok = pix < P;
    float mx = -__builtin_huge_valf(), ts = 0.f, tx = 0.f;
#pragma unroll
    for (int j = 0; j < kCritNPW; ++j) {
      const int q = g + 4 * j;
      if (q < N) {
        x[j] = ok ? x0[(long long)q * P + pix] : 0.f;
        mx = fmaxf(mx, x[j]);
        const int r = sinv[q];
        if (r >= 0) {
          const float t = ok ? load_f32<TDT>(targets, (long long)r * P + pix) : 0.f;
          ts += t;
          tx += t * x[j];
        }
      }
    }
    float se = 0.f;
#pragma unroll
    for (int j = 0; j < kCritNPW; ++j) {
      if (g + 4 * j < N) {
        x[j] = expf(x[j] - mx);
        se += x[j];
      }
    }
    if (g >= N) { mx = -1e30f; se = 0.f; }       // a wave without a query (N < 4)
    const CritPixel px = crit_exchange(sx[tile & 1], g, lane, mx, se, ts, tx, false);
    const bool vd = px.s2 < 1.f, keep = ok && !(masking && vd);
#pragma unroll
    for (int j = 0; j < kCritNPW; ++j) {
      const int q = g + 4 * j;
      if (q < N) {
        const float pr = ok ? x[j] * px.f : 0.f;
        sA[j] += vd ? pr : 0.f;
        sB[j] += vd ? 0.f : pr;
        const int r = sinv[q];
        if (r >= 0) {
          const float t = ok ? load_f32<TDT>(targets, (long long)r * P + pix) : 0.f;
          sT[j] += t;
          sI[j] += keep ? pr * t : 0.f;
        }
      }
    }
    if (g == 0) {
      const float ce = keep ? px.s2 * (px.mx + logf(px.se)) - px.s3 : 0.f;
      sce += ce;
      scnt += ce != 0.f ? 1.f : 0.f;
    }
  }
  float* pw = part + ((long long)z * gridDim.x + blockIdx.x) * crit_part_stride(N);
#pragma unroll
  for (int j = 0; j < kCritNPW; ++j) {
    const int q = g + 4 * j;
    if (q < N) {
      const float vA = wave_sum(sA[j]), vB = wave_sum(sB[j]), vI = wave_sum(sI[j]), vT = wave_sum(sT[j]);
      if (lane == 0) { pw[q] = vA; pw[N + q] = vB; pw[2 * N + q] = vI; pw[3 * N + q] = vT; }
    }
  }
  if (g == 0) {
    sce = wave_sum(sce);
    scnt = wave_sum(scnt);
    if (lane == 0) { pw[4 * N] = sce; pw[4 * N + 1] = scnt; }
  }
}

// the same for any N <= 512: the tile is read three times (the second and third time from L2) and the pixel sums of a query are
// reduced across lanes per tile into LDS accumulators
template <int TDT>
__global__ __launch_bounds__(256) void criterion_fwd_any_kernel(CritArgs a, const void* __restrict__ targets, const int* __restrict__ inv, int B, int N,
                                                                long long P, int tiles_per_wg, int masking, int share, float* __restrict__ part) {
  __shared__ float sx[2][4][4][kCritTP];
  __shared__ int sinv[kMaxQueries];
  __shared__ float sacc[4][kMaxQueries];
  const int z = blockIdx.y, l = z / B, b = z - l * B, zm = share ? b : z;
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  for (int n = tid; n < kMaxQueries; n += 256) {
    sinv[n] = n < N ? inv[(long long)zm * N + n] : -1;
    sacc[0][n] = 0.f; sacc[1][n] = 0.f; sacc[2][n] = 0.f; sacc[3][n] = 0.f;
  }
  __syncthreads();
  const float* x0 = a.masks[l] + (long long)b * N * P;
  float sce = 0.f, scnt = 0.f;
  long long t0, t1;
  crit_tile_range(P, tiles_per_wg, t0, t1);
  for (long long tile = t0; tile < t1; ++tile) {
    const long long pix = tile * kCritTP + lane;
    const bool ok = pix < P;
    float mx = -__builtin_huge_valf(), ts = 0.f, tx = 0.f;
    for (int q = g; q < N; q += 4) {
      const float xv = ok ? x0[(long long)q * P + pix] : 0.f;
      mx = fmaxf(mx, xv);
      const int r = sinv[q];
      if (r >= 0) {
        const float t = ok ? load_f32<TDT>(targets, (long long)r * P + pix) : 0.f;
        ts += t;
        tx += t * xv;
      }
    }
    float se = 0.f;
    for (int q = g; q < N; q += 4) se += expf((ok ? x0[(long long)q * P + pix] : 0.f) - mx);
    if (g >= N) { mx = -1e30f; se = 0.f; }
    const CritPixel px = crit_exchange(sx[tile & 1], g, lane, mx, se, ts, tx, false);
    const bool vd = px.s2 < 1.f, keep = ok && !(masking && vd);
    for (int q = g; q < N; q += 4) {
      const float pr = ok ? expf(x0[(long long)q * P + pix] - mx) * px.f : 0.f;
      const float vA = wave_sum(vd ? pr : 0.f), vB = wave_sum(vd ? 0.f : pr);
      float vI = 0.f, vT = 0.f;
      const int r = sinv[q];
      if (r >= 0) {
        const float t = ok ? load_f32<TDT>(targets, (long long)r * P + pix) : 0.f;
        vT = wave_sum(t);
        vI = wave_sum(keep ? pr * t : 0.f);
      }
      if (lane == 0) { sacc[0][q] += vA; sacc[1][q] += vB; sacc[2][q] += vI; sacc[3][q] += vT; }
    }
    if (g == 0) {
      const float ce = keep ? px.s2 * (px.mx + logf(px.se)) - px.s3 : 0.f;
      sce += ce;
      scnt += ce != 0.f ? 1.f : 0.f;
    }
  }
  __syncthreads();
  float* pw = part + ((long long)z * gridDim.x + blockIdx.x) * crit_part_stride(N);
  for (int i = tid; i < 4 * N; i += 256) pw[i] = sacc[i / N][i % N];
  if (g == 0) {
    sce = wave_sum(sce);
    scnt = wave_sum(scnt);
    if (lane == 0) { pw[4 * N] = sce; pw[4 * N + 1] = scnt; }
  }
}

// grid L, 256 threads: the videos of a layer one after the other
__global__ __launch_bounds__(256) void criterion_finish_kernel(CritArgs a, const float* __restrict__ part, int npb, int B, int N, int K1, int masking,
                                                               int share, CritSaved s, float* __restrict__ losses) {
  __shared__ float sf[kMaxQueries], sd[kMaxQueries];
  const int l = blockIdx.x, tid = threadIdx.x;
  const long long stride = crit_part_stride(N);
  float lce = 0.f, lmask = 0.f, ldice = 0.f;        // thread 0 only
  for (int b = 0; b < B; ++b) {
    const int z = l * B + b, zm = share ? b : z, zv = share ? b : z;     // zv: the problem whose masks give the void IoU (the final prediction's when shared)
    for (int n = tid; n < N; n += 256) {
      const float* pw = part + (long long)z * npb * stride;
      double A = 0.0, Bq = 0.0, I = 0.0, T = 0.0;
#pragma unroll 8
      for (int w = 0; w < npb; ++w) {         // (unrolled: 32 independent loads in flight; the additions stay in workgroup order)
        const float* pp = pw + (long long)w * stride;
        A += (double)pp[n]; Bq += (double)pp[N + n]; I += (double)pp[2 * N + n]; T += (double)pp[3 * N + n];
      }
      double Av = A, Bv = Bq;
      if (zv != z) {
        Av = 0.0; Bv = 0.0;
        const float* pv = part + (long long)zv * npb * stride;
#pragma unroll 8
        for (int w = 0; w < npb; ++w) { Av += (double)pv[(long long)w * stride + n]; Bv += (double)pv[(long long)w * stride + N + n]; }
      }
      const float fI = (float)I, fQ = (float)(masking ? Bq : A + Bq), fT = (float)T;
      const long long o = (long long)z * N + n, om = (long long)zm * N + n;
      s.sums[(long long)z * 3 * N + n] = fI;
      s.sums[(long long)z * 3 * N + N + n] = fQ;
      s.sums[(long long)z * 3 * N + 2 * N + n] = fT;
      sd[n] = (1.f - (2.f * fI + 1.f) / (fQ + fT + 1.f)) * s.wmask[om];
      const bool matched = s.inv[om] >= 0;
      const float wc = fmaxf(matched ? s.mdice[om] : (float)Av / ((float)(Av + Bv) + 1e-5f), 1e-5f);
      const int lab = s.mlabel[om];
      s.wcls[o] = wc;
      s.label[o] = lab;
      const float* x = a.logits[l] + ((long long)b * N + n) * K1;
      // CE = log(1 + sum of exp(x[c] - max) over the other classes) - (x[lab] - max): (max + log(sum)) - x[lab] cancels when the label's logit
      // dominates (the whole loss of a one-query problem), and log(1 + s) of a rounded 1 + s loses s's low bits
      float mx = x[0];
      int am = 0;
#pragma unroll 8
      for (int c = 1; c < K1; ++c)
        if (x[c] > mx) { mx = x[c]; am = c; }
      float se = 0.f;
#pragma unroll 8
      for (int c = 0; c < K1; ++c) se += c == am ? 0.f : expf(x[c] - mx);
      const float ce = log1pf(se) - (x[lab] - mx);
      sf[n] = (lab == K1 - 1 ? 0.25f : 0.75f) * ce * wc;
    }
    __syncthreads();
    if (tid == 0) {
      double f = 0.0, d = 0.0, ce = 0.0, cm = 0.0;
      float cf = 0.f;
      for (int n = 0; n < N; ++n) { f += (double)sf[n]; d += (double)sd[n]; cf += sf[n] != 0.f ? 1.f : 0.f; }
      const float* pw = part + (long long)z * npb * stride + 4 * N;
      for (int w = 0; w < npb; ++w, pw += stride) { ce += (double)pw[0]; cm += (double)pw[1]; }
      const float cntm = fmaxf((float)cm, 1.f), cntf = fmaxf(cf, 1.f);
      s.cnt[2 * z] = cntm;
      s.cnt[2 * z + 1] = cntf;
      lce += (float)f / cntf;
      lmask += (float)ce / cntm;
      ldice += (float)d * 0.75f / (float)N;
    }
    __syncthreads();
  }
  if (tid == 0) {
    losses[3 * l] = lce / (float)B;
    losses[3 * l + 1] = lmask / (float)B;
    losses[3 * l + 2] = ldice / (float)B;
  }
}

// the dice coefficients of a problem's queries into LDS: u[n][p] = ca[n] + cb[n] t[n][p]
__device__ __forceinline__ void crit_dice_coefs(const CritSaved& s, int z, int zm, int N, int B, float gdice, float* ca, float* cb, int nmax) {
  const float gd = gdice * 0.75f / ((float)N * (float)B);
  for (int n = threadIdx.x; n < nmax; n += 256) {
    float va = 0.f, vb = 0.f;
    if (n < N) {
      const float I = s.sums[(long long)z * 3 * N + n], Q = s.sums[(long long)z * 3 * N + N + n], T = s.sums[(long long)z * 3 * N + 2 * N + n];
      const float w = s.wmask[(long long)zm * N + n], D = Q + T + 1.f;
      va = gd * w * (2.f * I + 1.f) / (D * D);
      vb = -2.f * gd * w / D;
    }
    ca[n] = va;
    cb[n] = vb;
  }
}

// grid (npb, L * B), 256 threads, N <= 128.  gout: the upstream gradients of the [L][3] losses, in device memory
template <int TDT>
__global__ __launch_bounds__(256, 2) void criterion_bwd_kernel(CritArgs a, const void* __restrict__ targets, const float* __restrict__ gout, int B, int N,
                                                            long long P, int tiles_per_wg, int masking, int share, CritSaved s) {
  __shared__ float sx[2][4][4][kCritTP];
  __shared__ int sinv[4 * kCritNPW];
  __shared__ float ca[4 * kCritNPW], cb[4 * kCritNPW];
  const int z = blockIdx.y, l = z / B, b = z - l * B, zm = share ? b : z;
  float* dx0 = a.dmasks[l];
  if (!dx0) return;
  dx0 += (long long)b * N * P;
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  for (int n = tid; n < 4 * kCritNPW; n += 256) sinv[n] = n < N ? s.inv[(long long)zm * N + n] : -1;
  crit_dice_coefs(s, z, zm, N, B, gout[3 * l + 2], ca, cb, 4 * kCritNPW);
  __syncthreads();
  const float gm = gout[3 * l + 1] / ((float)B * s.cnt[2 * z]);
  const float* x0 = a.masks[l] + (long long)b * N * P;
  float x[kCritNPW], t[kCritNPW];
  long long t0, t1;
  crit_tile_range(P, tiles_per_wg, t0, t1);
  for (long long tile = t0; tile < t1; ++tile) {
    const long long pix = tile * kCritTP + lane;
    const bool ok = pix < P;
    float mx = -__builtin_huge_valf(), ts = 0.f;
#pragma unroll
    for (int j = 0; j < kCritNPW; ++j) {
      const int q = g + 4 * j;
      t[j] = 0.f;
      if (q < N) {
        x[j] = ok ? x0[(long long)q * P + pix] : 0.f;
        mx = fmaxf(mx, x[j]);
        const int r = sinv[q];
        if (r >= 0) {
          t[j] = ok ? load_f32<TDT>(targets, (long long)r * P + pix) : 0.f;
          ts += t[j];
        }
      }
    }
    float se = 0.f, sd = 0.f;
#pragma unroll
    for (int j = 0; j < kCritNPW; ++j) {
      const int q = g + 4 * j;
      if (q < N) {
        x[j] = expf(x[j] - mx);
        se += x[j];
        sd += x[j] * (ca[q] + cb[q] * t[j]);
      }
    }
    if (g >= N) { mx = -1e30f; se = 0.f; }
    const CritPixel px = crit_exchange(sx[tile & 1], g, lane, mx, se, ts, sd, true);
    const float sdot = px.s3 / px.se;
    const bool keep = ok && !(masking && px.s2 < 1.f);
    if (ok) {
#pragma unroll
      for (int j = 0; j < kCritNPW; ++j) {
        const int q = g + 4 * j;
        if (q < N) {
          const float pr = x[j] * px.f;
          dx0[(long long)q * P + pix] = keep ? gm * (pr * px.s2 - t[j]) + pr * (ca[q] + cb[q] * t[j] - sdot) : 0.f;
        }
      }
    }
  }
}

template <int TDT>
__global__ __launch_bounds__(256) void criterion_bwd_any_kernel(CritArgs a, const void* __restrict__ targets, const float* __restrict__ gout, int B, int N,
                                                                long long P, int tiles_per_wg, int masking, int share, CritSaved s) {
  __shared__ float sx[2][4][4][kCritTP];
  __shared__ int sinv[kMaxQueries];
  __shared__ float ca[kMaxQueries], cb[kMaxQueries];
  const int z = blockIdx.y, l = z / B, b = z - l * B, zm = share ? b : z;
  float* dx0 = a.dmasks[l];
  if (!dx0) return;
  dx0 += (long long)b * N * P;
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  for (int n = tid; n < kMaxQueries; n += 256) sinv[n] = n < N ? s.inv[(long long)zm * N + n] : -1;
  crit_dice_coefs(s, z, zm, N, B, gout[3 * l + 2], ca, cb, kMaxQueries);
  __syncthreads();
  const float gm = gout[3 * l + 1] / ((float)B * s.cnt[2 * z]);
  const float* x0 = a.masks[l] + (long long)b * N * P;
  long long t0, t1;
  crit_tile_range(P, tiles_per_wg, t0, t1);
  for (long long tile = t0; tile < t1; ++tile) {
    const long long pix = tile * kCritTP + lane;
    const bool ok = pix < P;
    float mx = -__builtin_huge_valf(), ts = 0.f;
    for (int q = g; q < N; q += 4) {
      mx = fmaxf(mx, ok ? x0[(long long)q * P + pix] : 0.f);
      const int r = sinv[q];
      if (r >= 0) ts += ok ? load_f32<TDT>(targets, (long long)r * P + pix) : 0.f;
    }
    float se = 0.f, sd = 0.f;
    for (int q = g; q < N; q += 4) {
      const float e = expf((ok ? x0[(long long)q * P + pix] : 0.f) - mx);
      const int r = sinv[q];
      const float t = (r >= 0 && ok) ? load_f32<TDT>(targets, (long long)r * P + pix) : 0.f;
      se += e;
      sd += e * (ca[q] + cb[q] * t);
    }
    if (g >= N) { mx = -1e30f; se = 0.f; }
    const CritPixel px = crit_exchange(sx[tile & 1], g, lane, mx, se, ts, sd, true);
    const float sdot = px.s3 / px.se;
    const bool keep = ok && !(masking && px.s2 < 1.f);
    if (ok) {
      for (int q = g; q < N; q += 4) {
        const float pr = expf(x0[(long long)q * P + pix] - mx) * px.f;
        const int r = sinv[q];
        const float t = r >= 0 ? load_f32<TDT>(targets, (long long)r * P + pix) : 0.f;
        dx0[(long long)q * P + pix] = keep ? gm * (pr * px.s2 - t) + pr * (ca[q] + cb[q] * t - sdot) : 0.f;
      }
    }
  }
}

// one wave per (problem, query) row of K1 logits
__global__ __launch_bounds__(256) void criterion_logits_bwd_kernel(CritArgs a, const float* __restrict__ gout, int B, int N, int K1, CritSaved s, int nrows) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= nrows) return;
  const int z = row / N, n = row - z * N, l = z / B, b = z - l * B;
  float* d = a.dlogits[l];
  if (!d) return;
  d += ((long long)b * N + n) * K1;
  const float* x = a.logits[l] + ((long long)b * N + n) * K1;
  float mx = -__builtin_huge_valf();
  for (int c = lane; c < K1; c += 64) mx = fmaxf(mx, x[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float se = 0.f;
  for (int c = lane; c < K1; c += 64) se += expf(x[c] - mx);
  se = wave_sum(se);
  const int lab = s.label[row];
  const float k = gout[3 * l] / ((float)B * s.cnt[2 * z + 1]) * (lab == K1 - 1 ? 0.25f : 0.75f) * s.wcls[row];
  for (int c = lane; c < K1; c += 64) d[c] = k * (expf(x[c] - mx) / se - (c == lab ? 1.f : 0.f));
}

}  // namespace axvs
