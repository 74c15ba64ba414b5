// Video panoptic post-processing on the device (maxtron_cc_model.py:442-571 / maxtron_wc_model.py:440-551): the bilinear resize(s) of
// the [N,T,h,w] mask logits, the softmax over the N slots, the pixel threshold, the slots' areas and mean scores, the reorder, the
// sequential merge and the relabelled map -- without ever holding the [N,T,H,W] tensor.
//
//   pixel pass   per output pixel: the N resized logits from a low-resolution LDS tile, the softmax over them, the (at most three)
//                slots above the pixel threshold as one packed word; per slot the exact area (integer) and the EXACT sum of the scores
//                over it: a score in (0.25, 1] is a multiple of 2^-26 in fp32, so it is added as a 2^-32 fixed-point integer and the
//                sum is the same whatever order the workgroups arrive in (integer atomics only).  The words of pixels with two or
//                three candidates are also appended to the contested list (its order varies from run to run; only counts are taken).
//   slot pass    one workgroup: class softmax, reorder score, rank (descending, ties to the lower slot), then the reference's merge loop
//                in that order; the pixels a slot loses to earlier painted slots are counted over the contested list.
//   paint pass   per pixel the final id of its first painted candidate in merge order, else -1.
#pragma once
#include <hip/hip_runtime.h>

#include "axvs_common.h"
#include "axvs_resize.h"

namespace axvs {

constexpr int kPanMaxN = 512;       // slots: 10 bits per candidate in the packed word (slot + 1; 0: none)
constexpr int kPanTile = 16;        // output tile 16 x 16 pixels, one per thread
constexpr int kPanThreads = kPanTile * kPanTile;
constexpr int kPanSlotThreads = 1024;
constexpr int kPanMaxLdsBytes = 128 * 1024;
constexpr double kPanFix = 4294967296.0;      // 2^32: scores travel as 2^-32 fixed point

__device__ __forceinline__ int pan_cand(unsigned word, int k) { return (int)((word >> (10 * k)) & 1023u) - 1; }

// softmax over the slots of one pixel -> packed candidates; areas and fixed-point score sums into the workgroup's LDS accumulators
template <int NS, class Src>
__device__ __forceinline__ unsigned pan_pixel(int y, int x, const PanGeom& g, const Src& s, unsigned* s_area, unsigned long long* s_sum) {
  PanPixel<NS> px;
  px.setup(y, x, g, s);
  // one sweep over the slots: the three largest logits (a score above 1/4 belongs to one of them; ties keep the lower slot first) and
  // the softmax denominator relative to the running maximum, rescaled the few times the maximum moves
  float v0 = -INFINITY, v1 = -INFINITY, v2 = -INFINITY, sum = 0.f;
  int i0 = -1, i1 = -1, i2 = -1;
  for (int n = 0; n < g.N; ++n) {
    const float v = px.eval(n, s);
    if (v > v0) {
      sum = sum * expf(v0 - v) + 1.f;
      v2 = v1, i2 = i1, v1 = v0, i1 = i0, v0 = v, i0 = n;
    } else {
      sum += expf(v - v0);
      if (v > v1) v2 = v1, i2 = i1, v1 = v, i1 = n;
      else if (v > v2) v2 = v, i2 = n;
    }
  }
  unsigned word = 0;
  int k = 0;
  const float vs[3] = {v0, v1, v2};
  const int is[3] = {i0, i1, i2};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (is[j] < 0) continue;
    const float sc = expf(vs[j] - v0) / sum;
    if (sc > g.thr) {
      word |= (unsigned)(is[j] + 1) << (10 * k++);
      atomicAdd(&s_area[is[j]], 1u);
      atomicAdd(&s_sum[is[j]], (unsigned long long)((double)sc * kPanFix));
    }
  }
  return word;
}

// grid: workgroups striding over the T * ceil(H/16) * ceil(W/16) output tiles; dynamic LDS: lds_floats floats for the tile
template <int DT, int NS>
__global__ __launch_bounds__(kPanThreads) void panoptic_pixel_kernel(const void* __restrict__ logits, PanGeom g, int lds_floats, unsigned* __restrict__ words,
                                                                     unsigned* __restrict__ contested, unsigned* __restrict__ n_contested,
                                                                     unsigned* __restrict__ area, unsigned long long* __restrict__ sums) {
  extern __shared__ float s_tile[];
  __shared__ unsigned s_area[kPanMaxN];
  __shared__ unsigned long long s_sum[kPanMaxN];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  for (int n = tid; n < g.N; n += kPanThreads) s_area[n] = 0, s_sum[n] = 0;
  const int tx_n = (g.W + kPanTile - 1) / kPanTile, ty_n = (g.H + kPanTile - 1) / kPanTile;
  const long long ntiles = (long long)g.T * ty_n * tx_n;
  const long long frame = (long long)g.h * g.w;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int t = (int)(tile / (ty_n * tx_n)), rem = (int)(tile % (ty_n * tx_n));
    const int y0 = rem / tx_n * kPanTile, x0 = rem % tx_n * kPanTile;
    int rlo, rhi, clo, chi;
    pan_range(y0, min(y0 + kPanTile, g.H) - 1, g, g.y1, g.y2, &rlo, &rhi);
    pan_range(x0, min(x0 + kPanTile, g.W) - 1, g, g.x1, g.x2, &clo, &chi);
    const int bh = rhi - rlo + 1, bw = chi - clo + 1;
    const bool fits = (long long)g.N * bh * bw <= lds_floats;
    __syncthreads();          // the previous tile's readers are done (and the accumulators are zero before the first)
    if (fits) {
      const int box = bh * bw, total = g.N * box;
      if (box <= kPanThreads) {        // a thread keeps its place in the box and steps over the slots: no division per element
        const int per = kPanThreads / box, n0 = tid / box, q = tid - n0 * box, r = q / bw, c = q - r * bw;
        const long long at = (long long)t * frame + (long long)(rlo + r) * g.w + (clo + c);
        if (n0 < per)
          for (int n = n0; n < g.N; n += per) s_tile[n * box + q] = pan_load<DT>(logits, (long long)n * g.T * frame + at);
      } else {
        for (int e = tid; e < total; e += kPanThreads) {
          const int n = e / box, q = e - n * box, r = q / bw, c = q - r * bw;
          s_tile[e] = pan_load<DT>(logits, ((long long)n * g.T + t) * frame + (long long)(rlo + r) * g.w + (clo + c));
        }
      }
    }
    __syncthreads();
    const int y = y0 + tid / kPanTile, x = x0 + tid % kPanTile;
    const bool live = y < g.H && x < g.W;
    unsigned word = 0;
    if (live) {
      if (fits) word = pan_pixel<NS>(y, x, g, PanLdsSrc{s_tile, bh * bw, bw, rlo, clo}, s_area, s_sum);
      else word = pan_pixel<NS>(y, x, g, PanGlobalSrc<DT>{logits, (long long)t * frame, (long long)g.T * frame, g.w}, s_area, s_sum);
    }
    const unsigned pix = live ? (unsigned)(((long long)t * g.H + y) * g.W + x) : 0u;
    if (live) words[pix] = word;
    // contested pixels (two or three candidates): one counter bump per wave
    const bool con = live && (word >> 10) != 0;
    const unsigned long long m = __ballot(con);
    if (m) {
      const int leader = __ffsll((long long)m) - 1;
      unsigned base = 0;
      if (lane == leader) base = atomicAdd(n_contested, (unsigned)__popcll(m));
      base = __shfl(base, leader, kWave);
      if (con) contested[base + __popcll(m & ((1ull << lane) - 1ull))] = word;
    }
  }
  __syncthreads();
  for (int n = tid; n < g.N; n += kPanThreads)
    if (s_area[n]) {
      atomicAdd(&area[n], s_area[n]);
      atomicAdd(&sums[n], s_sum[n]);
    }
}

struct PanMerge {
  int N, K1, label_divisor;
  double thr_thing, thr_stuff, overlap, w_class, w_mask;
};

// int32 slot table: 4 header words, then 7 arrays of N (include/axvs.h)
enum { kPanHdr = 4, kPanFinal = 0, kPanRank = 1, kPanLabel = 2, kPanArea = 3, kPanThingSlot = 4, kPanThingCat = 5, kPanThingIi = 6, kPanIntArrays = 7 };

// one workgroup.  mask_cls fp32 [N][K1]; is_thing / cat_id int32 [K1 - 1].
__global__ __launch_bounds__(kPanSlotThreads) void panoptic_slot_kernel(const float* __restrict__ mask_cls, const int* __restrict__ is_thing,
                                                                        const int* __restrict__ cat_id, PanMerge m,
                                                                        const unsigned* __restrict__ contested, const unsigned* __restrict__ n_contested,
                                                                        const unsigned* __restrict__ area, const unsigned long long* __restrict__ sums,
                                                                        int* __restrict__ itab, float* __restrict__ ftab) {
  __shared__ double s_score[kPanMaxN];
  __shared__ float s_cls[kPanMaxN];
  __shared__ int s_label[kPanMaxN], s_order[kPanMaxN], s_red[kPanSlotThreads / kWave];
  __shared__ unsigned char s_painted[kPanMaxN];
  const int tid = threadIdx.x, N = m.N, K = m.K1 - 1;
  if (tid < N) {
    // F.softmax(mask_cls, -1)[..., :-1].max(-1): fp32, the first maximum
    const float* row = mask_cls + (long long)tid * m.K1;
    float mx = row[0];
    for (int k = 1; k < m.K1; ++k) mx = fmaxf(mx, row[k]);
    float sum = 0.f, best = -INFINITY;
    int lab = 0;
    for (int k = 0; k < m.K1; ++k) {
      sum += expf(row[k] - mx);
      if (k < K && row[k] > best) best = row[k], lab = k;
    }
    const float cls = expf(best - mx) / sum;
    const unsigned a = area[tid];
    const double mean = (double)sums[tid] / kPanFix / (double)(a > 0 ? a : 1u);
    double score = pow((double)cls, m.w_class) * pow(mean, m.w_mask);
    if (!(score == score)) score = -1.0;        // NaN (non-finite logits, 0 * inf with a negative weight) must still rank: last
    s_cls[tid] = cls, s_label[tid] = lab, s_score[tid] = score, s_painted[tid] = 0;
    ftab[tid] = cls, ftab[N + tid] = (float)mean, ftab[2 * N + tid] = (float)score;
    itab[kPanHdr + kPanLabel * N + tid] = lab;
    itab[kPanHdr + kPanArea * N + tid] = (int)a;
    itab[kPanHdr + kPanFinal * N + tid] = -1;
    itab[kPanHdr + kPanThingSlot * N + tid] = -1;
    itab[kPanHdr + kPanThingCat * N + tid] = -1;
    itab[kPanHdr + kPanThingIi * N + tid] = -1;
  }
  __syncthreads();
  if (tid < N) {       // descending; equal scores: the lower slot first
    const double s = s_score[tid];
    int rank = 0;
    for (int j = 0; j < N; ++j) {
      const double o = s_score[j];
      rank += (o > s || (o == s && j < tid)) ? 1 : 0;
    }
    s_order[rank] = tid;
    itab[kPanHdr + kPanRank * N + tid] = rank;
  }
  __syncthreads();
  const unsigned ncon = *n_contested;
  int segments = 0, things = 0;      // uniform over the workgroup
  for (int r = 0; r < N; ++r) {
    const int i = s_order[r], lab = s_label[i];
    const bool thing = is_thing[lab] != 0;
    const unsigned orig = area[i];
    if (!((double)s_cls[i] > (thing ? m.thr_thing : m.thr_stuff)) || orig == 0) continue;
    // pixels of slot i that an earlier painted slot holds already
    int lost = 0;
    for (unsigned e = tid; e < ncon; e += kPanSlotThreads) {
      const unsigned wd = contested[e];
      const int a = pan_cand(wd, 0), b = pan_cand(wd, 1), c = pan_cand(wd, 2);
      const bool mine = a == i || b == i || c == i;
      const bool taken = s_painted[a] || s_painted[b] || (c >= 0 && s_painted[c]);
      lost += (mine && taken) ? 1 : 0;
    }
    lost = pan_block_sum(lost, s_red, kPanSlotThreads);
    const unsigned fresh = orig - (unsigned)lost;
    if (!((double)fresh > (double)orig * m.overlap)) continue;
    // painted slots of the same class so far: a thing's `ii`, or whether a stuff class has its segment already
    const int same = pan_block_sum((tid < N && s_painted[tid] && s_label[tid] == lab) ? 1 : 0, s_red, kPanSlotThreads);
    const int cat = cat_id[lab];
    if (thing) {
      if (tid == 0) {
        itab[kPanHdr + kPanFinal * N + i] = cat * m.label_divisor + same;
        itab[kPanHdr + kPanThingSlot * N + things] = i;
        itab[kPanHdr + kPanThingCat * N + things] = cat;
        itab[kPanHdr + kPanThingIi * N + things] = same;
      }
      ++things, ++segments;
    } else {
      if (same == 0) ++segments;      // a repeated stuff class paints with the remembered segment and takes no new id
      if (tid == 0) itab[kPanHdr + kPanFinal * N + i] = cat;
    }
    __syncthreads();             // every thread has read s_painted for this slot
    if (tid == 0) s_painted[i] = 1;
    __syncthreads();
  }
  if (tid == 0) itab[0] = things, itab[1] = segments, itab[2] = (int)ncon, itab[3] = 0;
}

__global__ __launch_bounds__(256) void panoptic_paint_kernel(const unsigned* __restrict__ words, const int* __restrict__ itab, int N, long long P,
                                                             int* __restrict__ out) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const unsigned wd = words[p];
  int id = -1, best = N;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int c = pan_cand(wd, k);
    if (c < 0) continue;
    const int f = itab[kPanHdr + kPanFinal * N + c], r = itab[kPanHdr + kPanRank * N + c];
    if (f != -1 && r < best) best = r, id = f;
  }
  out[p] = id;
}

}  // namespace axvs
