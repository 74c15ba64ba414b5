// Prediction-to-ground-truth matching on the device: the similarity / cost half of VideoHungarianMatcher
// (MaXTron_Video-kMaX/maxtron_deeplab/modeling/matcher.py:18-45, :76-92); the assignment half is lsap_rect_kernel (axvs_lsap.h).
//
//   mask similarity (matcher.py:18-38)   softmax over the Q queries of pred_masks [Q, P] (P = T*H*W), times the non-void flag of the
//                                        pixel (sum_m t > 0) when masking_void_pixel, inter = prob @ t^T, dice-like ratio
//                                        inter / ((sum_p prob + sum_p t) / 2 + 1e-5)
//   class similarity (matcher.py:42-45)  softmax over the K + 1 logits, void column dropped, the M labels gathered
//   cost (matcher.py:86)                 C = -mask_sim * class_sim, fp32 [Q, M]: the assignment kernel's input
//
// One launch of matcher_sim_kernel covers every (layer, video) problem of a training step: the targets belong to the video and
// are shared by the layers, M is ragged over the videos (object counts and row offsets travel as kernel arguments: the caller
// knows them on the host).  pred_masks is read once and the targets once per layer; nothing is accumulated with atomics:
// workgroup w of a problem owns a contiguous pixel range, writes ONE set of partial sums, and matcher_finish_kernel adds the
// partials in workgroup order (in double), so results are run-to-run identical.
//
// The [Q x P] . [P x M] contraction runs on the f32-input MFMA (v_mfma_f32_32x32x2_f32: exact fp32 products, a k-ordered fmaf chain):
// it needs no split of the probability or of a non-binary target into 16-bit pieces.  Measured at Q = 128, P = 65536, 4 layers
// (profiles/matcher_time.md): the kernel takes 158 us at M = 8 and 230 us at M = 96, 0.9 TB/s of needed traffic -- 11 % of HBM.  The
// contraction accounts for the ~70 us between the two; the rest is the softmax half (three passes over the LDS tile, four barriers
// per tile, one tile in flight per workgroup, and the MFMA phase does not overlap it).  A 16-bit MFMA form could save at most those
// 70 us; the softmax half is what limits the kernel.
#pragma once
#include "axvs_targets.h"
#include "axvs_lsap.h"

namespace axvs {

constexpr int kMatcherTP = 64;                 // pixels per tile: one per lane, so a query's row of a tile is one coalesced wave read
constexpr int kMatcherLDP = kMatcherTP + 1;    // LDS row stride (odd: the MFMA operand reads walk 32 rows at one pixel)
constexpr int kMatcherMaxRows = 576;            // ceil32(Q) + ceil32(M_max) rows of LDS tiles (150 KB of the 160)
constexpr int kMatcherBlocksPerChunk = 16;     // 32 x 32 output blocks per workgroup: 4 waves x 4 accumulator tiles

struct MatcherArgs {
  const void* masks[kMaxLayers];      // per layer: pred_masks [B][Q][P]
  const float* logits[kMaxLayers];    // per layer: pred_logits fp32 [B][Q][K1]
  int m[kMaxVideos];                  // objects of video b
  int off[kMaxVideos];                // first row of video b in the concatenated targets / labels
};

typedef float f32x16 __attribute__((ext_vector_type(16)));

// floats of one workgroup's partial sums: inter [Q][Mmax], in_sum [Q], t_sum [Mmax]
__host__ __device__ inline long long matcher_part_stride(int Q, int Mmax) { return (long long)Q * Mmax + Q + Mmax; }

// grid (npb, chunks, L * B), 256 threads.  Dynamic LDS: sp [Qp][LDP] (logits -> exp -> masked probabilities) and st [Mp][LDP] (targets),
// Qp / Mp = Q / Mmax rounded up to 32.
template <int DT, int TDT>
__global__ __launch_bounds__(256) void matcher_sim_kernel(MatcherArgs a, const void* __restrict__ targets, int B, int Q, long long P, int Mmax,
                                                          int tiles_per_wg, int masking, float* __restrict__ part) {
  extern __shared__ float msm[];
  __shared__ float sred[3][4][kMatcherTP];
  __shared__ float sacc[kMatcherMaxRows];      // running pixel sums of the rows of sp (queries) and st (targets), in LDS row order
  const int z = blockIdx.z, l = z / B, b = z - l * B;
  const int M = a.m[b];
  if (M <= 0) return;
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  const int Qp = (Q + 31) & ~31, nqb = Qp >> 5, nmb = (M + 31) >> 5, Mp = nmb << 5;
  float* sp = msm;
  float* st = msm + (size_t)Qp * kMatcherLDP;
  const int blk0 = blockIdx.y * kMatcherBlocksPerChunk, nblk = nqb * nmb;
  if (blk0 >= nblk) return;
  const void* mask = a.masks[l];
  const long long mbase = (long long)b * Q * P, tbase = (long long)a.off[b] * P;

  for (int i = tid; i < (Qp - Q) * kMatcherLDP; i += 256) sp[(size_t)Q * kMatcherLDP + i] = 0.f;
  for (int i = tid; i < kMatcherMaxRows; i += 256) sacc[i] = 0.f;
  f32x16 acc[4];
  int aoff[4], boff[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;
    const int t = blk0 + g + 4 * k, qb = t % nqb, mb = t / nqb;
    aoff[k] = (qb * 32 + (lane & 31)) * kMatcherLDP + (lane >> 5);
    boff[k] = (mb * 32 + (lane & 31)) * kMatcherLDP + (lane >> 5);
  }
  __syncthreads();

  const long long ntiles = (P + kMatcherTP - 1) / kMatcherTP;
  const long long t0 = (long long)blockIdx.x * tiles_per_wg;
  const long long t1 = t0 + tiles_per_wg < ntiles ? t0 + tiles_per_wg : ntiles;
  for (long long tile = t0; tile < t1; ++tile) {
    const long long pix = tile * kMatcherTP + lane;
    const bool ok = pix < P;
    // targets of the tile; column sums for the non-void flag, row sums for the denominator
    float cs = 0.f;
    for (int m = g; m < Mp; m += 4) {
      const float t = (m < M && ok) ? load_f32<TDT>(targets, tbase + (long long)m * P + pix) : 0.f;
      st[m * kMatcherLDP + lane] = t;
      cs += t;
    }
    // softmax over the queries of every pixel: wave g holds queries g, g + 4, ...
    float mx = -__builtin_huge_valf();
    for (int q = g; q < Q; q += 4) {
      const float x = ok ? load_f32<DT>(mask, mbase + (long long)q * P + pix) : 0.f;
      sp[q * kMatcherLDP + lane] = x;
      mx = fmaxf(mx, x);
    }
    sred[0][g][lane] = mx;
    sred[1][g][lane] = cs;
    __syncthreads();
    mx = fmaxf(fmaxf(sred[0][0][lane], sred[0][1][lane]), fmaxf(sred[0][2][lane], sred[0][3][lane]));
    cs = sred[1][0][lane] + sred[1][1][lane] + sred[1][2][lane] + sred[1][3][lane];
    float se = 0.f;
    for (int q = g; q < Q; q += 4) {
      const float e = expf(sp[q * kMatcherLDP + lane] - mx);
      sp[q * kMatcherLDP + lane] = e;
      se += e;
    }
    sred[2][g][lane] = se;
    __syncthreads();
    se = sred[2][0][lane] + sred[2][1][lane] + sred[2][2][lane] + sred[2][3][lane];
    const bool keep = ok && (!masking || cs > 0.f);
    for (int q = g; q < Q; q += 4) {
      const float pr = keep ? sp[q * kMatcherLDP + lane] / se : 0.f;
      sp[q * kMatcherLDP + lane] = pr;
    }
    __syncthreads();
    // row sums of the tile (in_sum of the queries, t_sum of the targets): one thread per LDS row, four interleaved chains over the
    // 64 pixels; the odd row stride keeps the 64 lanes of a wave on 64 banks
    for (int r = tid; r < Qp + Mp; r += 256) {
      const float* row = msm + r * kMatcherLDP;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 4
      for (int p = 0; p < kMatcherTP; p += 4) { s0 += row[p]; s1 += row[p + 1]; s2 += row[p + 2]; s3 += row[p + 3]; }
      sacc[r] += (s0 + s1) + (s2 + s3);
    }
    // inter[q][m] += sum_p prob[q][p] * t[m][p]: A[i = q][k = p], B[k = p][j = m], two pixels per MFMA
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (blk0 + g + 4 * k < nblk) {
        const float* ap = sp + aoff[k];
        const float* bp = st + boff[k];
#pragma unroll 8
        for (int p = 0; p < kMatcherTP; p += 2) acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[p], bp[p], acc[k], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  float* pw = part + ((long long)z * gridDim.x + blockIdx.x) * matcher_part_stride(Q, Mmax);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int t = blk0 + g + 4 * k;
    if (t < nblk) {
      const int qb = t % nqb, mb = t / nqb, m = mb * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int q = qb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (q < Q && m < M) pw[(long long)q * Mmax + m] = acc[k][r];
      }
    }
  }
  if (blockIdx.y == 0) {
    for (int q = tid; q < Q; q += 256) pw[(long long)Q * Mmax + q] = sacc[q];
    for (int m = tid; m < M; m += 256) pw[(long long)Q * Mmax + Q + m] = sacc[Qp + m];
  }
}

// softmax statistics of the class logits: one wave per (problem, query) row of K1 logits -> (max, sum of exp)
__global__ __launch_bounds__(256) void matcher_class_stats_kernel(MatcherArgs a, int B, int Q, int K1, float* __restrict__ stats, int nrows) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= nrows) return;
  const int z = row / Q, q = row - z * Q, l = z / B, b = z - l * B;
  const float* x = a.logits[l] + ((long long)b * Q + q) * K1;
  float mx = -__builtin_huge_valf();
  for (int c = lane; c < K1; c += 64) mx = fmaxf(mx, x[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float s = 0.f;
  for (int c = lane; c < K1; c += 64) s += expf(x[c] - mx);
  s = wave_sum(s);
  if (lane == 0) { stats[2 * (long long)row] = mx; stats[2 * (long long)row + 1] = s; }
}

// partials -> mask_sim, class_sim, cost (each fp32 [L * B][Q][Mmax]; columns m >= M of a problem are zero).  grid (ceil(Q * Mmax / 256), L * B)
__global__ __launch_bounds__(256) void matcher_finish_kernel(MatcherArgs a, const float* __restrict__ part, int npb, const float* __restrict__ stats,
                                                             const long long* __restrict__ labels, int B, int Q, int K1, int Mmax,
                                                             float* __restrict__ mask_sim, float* __restrict__ class_sim, float* __restrict__ cost) {
  const int idx = blockIdx.x * 256 + threadIdx.x, z = blockIdx.y;
  if (idx >= Q * Mmax) return;
  const int q = idx / Mmax, m = idx - q * Mmax, l = z / B, b = z - l * B;
  const long long o = (long long)z * Q * Mmax + idx;
  if (m >= a.m[b]) { mask_sim[o] = 0.f; class_sim[o] = 0.f; cost[o] = 0.f; return; }
  const long long stride = matcher_part_stride(Q, Mmax);
  const float* pw = part + (long long)z * npb * stride;
  double si = 0.0, sq = 0.0, sm = 0.0;
  for (int w = 0; w < npb; ++w, pw += stride) {
    si += (double)pw[idx];
    sq += (double)pw[(long long)Q * Mmax + q];
    sm += (double)pw[(long long)Q * Mmax + Q + m];
  }
  const float den = ((float)sq + (float)sm) / 2.0f;
  const float ms = (float)si / (den + 1e-5f);
  long long lab = labels[a.off[b] + m];
  lab = lab < 0 ? 0 : (lab > K1 - 2 ? K1 - 2 : lab);        // (the reference raises on a label outside 0 .. K-1; here it is clamped)
  const long long row = (long long)z * Q + q;
  const float cp = expf(a.logits[l][((long long)b * Q + q) * K1 + lab] - stats[2 * row]) / stats[2 * row + 1];
  mask_sim[o] = ms;
  class_sim[o] = cp;
  cost[o] = -ms * cp;
}

// matched values: mask_sim / class_sim at the assigned (row, col) pairs; unused slots (-1) give 0
__global__ __launch_bounds__(256) void matcher_gather_kernel(const long long* __restrict__ rows, const long long* __restrict__ cols,
                                                             const float* __restrict__ mask_sim, const float* __restrict__ class_sim, int Q, int Mmax,
                                                             int kmax, long long total, float* __restrict__ dice, float* __restrict__ cls) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long z = i / kmax, r = rows[i], c = cols[i];
  const bool ok = r >= 0 && c >= 0;
  const long long o = (z * Q + (ok ? r : 0)) * Mmax + (ok ? c : 0);
  dice[i] = ok ? mask_sim[o] : 0.f;
  cls[i] = ok ? class_sim[o] : 0.f;
}

}  // namespace axvs
