// Video instance post-processing on the device for Tube-Link VIS (mask2former_video_cc_head.py:1026-1034: the whole-video resize;
// maskformer_fusion_head.py:405-462: `instance_postprocess` per frame; mask/utils.py:68-89: `mask2bbox`; mask2former_vis_video.py:184-193:
// the per-frame top 30) -- without ever holding a resized [T,Q,H,W] tensor.
//
//   candidate pass  one workgroup: class softmax, the k_cand largest of the Q*C scores in descending order (equal scores: the lower flat
//                   index first) by a bitwise search for the k-th largest 47-bit key (score bits, inverted index), the thing filter with
//                   order-preserving compaction, the ascending list of the queries a candidate refers to.
//   statistics pass per output tile of 4 rows x 64 pixels (one wave per row): the referenced queries' low-resolution boxes in LDS, the two
//                   bilinear stages per pixel (skipped for a query whose box holds no positive value), and per (frame, query) the exact area (integer), the EXACT sum of the sigmoids over the mask
//                   -- a sigmoid of a positive logit is a fp32 in [0.5, 1], a multiple of 2^-24, so it is added as a 2^-24 fixed-point
//                   integer: a wave's 64 fit in 32 bits, the total in 64, and the sum is the same in whatever order the workgroups arrive
//                   -- and the box by integer max.  A wave reduces (the box comes from its ballot alone), the workgroup accumulates in LDS
//                   over its run of tiles, and only then do global atomics follow.  Nothing full-resolution is written.
//   select pass     one workgroup per frame: mask score, detection score and box per candidate, rank (descending, equal scores to the
//                   lower candidate position), the top k_out rows.
//   emit pass       the statistics pass's tile loop over the k_out selected queries of the frame: the resized logit again, then `> 0` as a
//                   uint8 map or as one ballot word per 64 pixels of a row.
#pragma once
#include <hip/hip_runtime.h>

#include "axvs_common.h"
#include "axvs_resize.h"

namespace axvs {

constexpr int kVisMaxQ = 512;
constexpr int kVisMaxCand = 256;
constexpr int kVisMaxKeys = 1 << 17;         // Q * C: the flat index takes 17 bits of the key
constexpr int kVisKeysLds = 4096;            // up to this many keys stay in LDS during the search (the shipped 100 x 40 do)
constexpr int kVisCandThreads = 1024;
constexpr int kVisTileW = 64, kVisTileH = 4; // output tile: one wave per row, one ballot word per wave
constexpr int kVisThreads = kVisTileW * kVisTileH;
constexpr int kVisLdsFloats = 8192;          // 32 KiB tile: blocks of kVisLdsFloats / box queries are staged at a time
constexpr int kVisBox = 256;                 // a tile whose low-resolution box has more positions per query (a resize that shrinks about
                                             // threefold or more) reads its taps from global memory: at least 32 queries fit in a block
constexpr float kVisFix = 16777216.f;        // 2^24: sigmoids travel as 2^-24 fixed point

enum { kVisStats = 0, kVisEmitU8 = 1, kVisEmitBits = 2 };

// Tables (include/axvs.h): int32 {ncand, nref}, cand query [K], cand label [K], area [F][K], count [F], track id / label / query [F][Ko];
// fp32 class score [K], mask score [F][K], detection score [F][K], cand box [F][K][4], box [F][Ko][4], score [F][Ko]
struct VisTabs {
  int *head, *cand_query, *cand_label, *area, *count, *track, *label, *query;
  float *cls, *mask_score, *det, *cand_box, *box, *score;
};

__host__ __device__ inline VisTabs vis_tabs(int* ti, float* tf, int F, int K, int Ko) {
  VisTabs t;
  t.head = ti, t.cand_query = ti + 2, t.cand_label = t.cand_query + K, t.area = t.cand_label + K, t.count = t.area + (long long)F * K;
  t.track = t.count + F, t.label = t.track + (long long)F * Ko, t.query = t.label + (long long)F * Ko;
  t.cls = tf, t.mask_score = tf + K, t.det = t.mask_score + (long long)F * K, t.cand_box = t.det + (long long)F * K;
  t.box = t.cand_box + (long long)F * K * 4, t.score = t.box + (long long)F * Ko * 4;
  return t;
}

// per (frame, query), zeroed before the statistics pass; box = {W - xmin, H - ymin, xmax + 1, ymax + 1}, all by max (0: empty mask)
struct VisAcc {
  unsigned long long* sum;
  unsigned* area;
  unsigned* box;
};

// one workgroup.  mask_cls fp32 [Q][C + 1]; g_keys: Q * C words of workspace (used when they do not fit in LDS)
__global__ __launch_bounds__(kVisCandThreads) void vis_candidate_kernel(const float* __restrict__ mask_cls, int Q, int C, int K, int num_things,
                                                                        unsigned long long* g_keys, VisTabs tb, int* __restrict__ ref_list) {
  __shared__ unsigned long long s_keys[kVisKeysLds], s_sel[kVisMaxCand], s_sorted[kVisMaxCand];
  __shared__ int s_red[kVisCandThreads / kWave], s_keep[kVisMaxCand], s_n;
  __shared__ unsigned char s_ref[kVisMaxQ];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), n = Q * C, K1 = C + 1;
  unsigned long long* keys = n <= kVisKeysLds ? s_keys : g_keys;
  // F.softmax(mask_cls, -1)[:, :-1] in fp32, a wave per row; key = score bits (a score is in [0, 1]: below 2^30) and the inverted index
  for (int q = tid / kWave; q < Q; q += kVisCandThreads / kWave) {
    const float* row = mask_cls + (long long)q * K1;
    float mx = -INFINITY, sum = 0.f;
    for (int k = lane; k < K1; k += kWave) mx = fmaxf(mx, row[k]);
    for (int o = kWave / 2; o > 0; o >>= 1) mx = wave_xor_max(mx, o);
    for (int k = lane; k < K1; k += kWave) sum += expf(row[k] - mx);
    for (int o = kWave / 2; o > 0; o >>= 1) sum = wave_xor_sum(sum, o);
    for (int k = lane; k < C; k += kWave) {
      float sc = expf(row[k] - mx) / sum;
      sc = sc >= 0.f ? fminf(sc, 1.f) : 0.f;           // (a NaN from non-finite logits must still be a key: it ranks last)
      const int idx = q * C + k;
      keys[idx] = ((unsigned long long)__float_as_uint(sc) << 17) | (unsigned long long)(kVisMaxKeys - 1 - idx);
    }
  }
  if (tid == 0) s_n = 0;
  if (tid < kVisMaxQ) s_ref[tid] = 0;
  __syncthreads();
  // the K-th largest key (keys are distinct): the largest value that at least K keys reach, bit by bit
  unsigned long long kth = 0;
  for (int b = 46; b >= 0; --b) {
    const unsigned long long probe = kth | (1ull << b);
    int cnt = 0;
    for (int i = tid; i < n; i += kVisCandThreads) cnt += keys[i] >= probe ? 1 : 0;
    if (pan_block_sum(cnt, s_red, kVisCandThreads) >= K) kth = probe;
  }
  for (int i = tid; i < n; i += kVisCandThreads) {
    const unsigned long long k = keys[i];
    if (k >= kth) s_sel[atomicAdd(&s_n, 1) & (kVisMaxCand - 1)] = k;        // exactly K of them (the keys are distinct), in any order
  }
  __syncthreads();
  if (tid < K) {
    const unsigned long long mine = s_sel[tid];
    int rank = 0;
    for (int j = 0; j < K; ++j) rank += s_sel[j] > mine ? 1 : 0;
    s_sorted[rank] = mine;
  }
  __syncthreads();
  int q = -1, label = -1, keep = 0;
  float sc = 0.f;
  if (tid < K) {
    const unsigned long long k = s_sorted[tid];
    const int idx = kVisMaxKeys - 1 - (int)(k & (unsigned long long)(kVisMaxKeys - 1));
    sc = __uint_as_float((unsigned)(k >> 17));
    q = idx / C, label = idx - q * C;
    keep = label < num_things ? 1 : 0;                 // `is_thing`: order-preserving compaction below
    s_keep[tid] = keep;
  }
  __syncthreads();
  const int ncand = pan_block_sum(keep, s_red, kVisCandThreads);
  if (keep) {
    int pos = 0;
    for (int j = 0; j < tid; ++j) pos += s_keep[j];
    tb.cand_query[pos] = q, tb.cand_label[pos] = label, tb.cls[pos] = sc;
    s_ref[q] = 1;
  }
  if (tid >= ncand && tid < K) tb.cand_query[tid] = -1, tb.cand_label[tid] = -1, tb.cls[tid] = -1.f;
  __syncthreads();
  const int isref = (tid < Q && s_ref[tid]) ? 1 : 0;
  const int nref = pan_block_sum(isref, s_red, kVisCandThreads);
  if (isref) {
    int pos = 0;
    for (int j = 0; j < tid; ++j) pos += s_ref[j];
    ref_list[pos] = tid;
  }
  if (tid == 0) tb.head[0] = ncand, tb.head[1] = nref;
}

// exact integer sum over the wave on the VALU (the DPP / permlane steps of axvs_common.h's wave_sum): no trip through the LDS crossbar
template <int CTRL>
__device__ __forceinline__ unsigned vis_dpp(unsigned v) { return __builtin_amdgcn_update_dpp(0u, v, CTRL, 0xF, 0xF, true); }
__device__ __forceinline__ unsigned vis_wave_sum(unsigned v) {
  v += vis_dpp<0xB1>(v);       // quad_perm [1,0,3,2]
  v += vis_dpp<0x4E>(v);       // quad_perm [2,3,0,1]
  v += vis_dpp<0x141>(v);      // row_half_mirror
  v += vis_dpp<0x140>(v);      // row_mirror: every lane holds its 16-lane row's sum
  auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  v = r[0] + r[1];
  r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return r[0] + r[1];
}

// What a tile does with the resized logit `v` of list entry `r` at the thread's pixel (every thread of the wave calls it).
struct VisStatsOut {
  unsigned* s_area;
  unsigned long long* s_sum;
  unsigned* s_box;                  // [4][kVisMaxQ]
  int H, W;
  __device__ __forceinline__ void operator()(int r, float v, bool live, int y, int x0) const {
    const bool pos = live && v > 0.f;
    const unsigned long long m = __ballot(pos);
    if (m == 0) return;
    unsigned s = pos ? (unsigned)((1.f / (1.f + expf(-v))) * kVisFix) : 0u;      // exact: a multiple of 2^-24 in [0.5, 1]
    s = vis_wave_sum(s);
    if ((threadIdx.x & (kWave - 1)) == 0) {          // the wave is one row: lane = column - x0
      atomicAdd(&s_area[r], (unsigned)__popcll(m));
      atomicAdd(&s_sum[r], (unsigned long long)s);
      atomicMax(&s_box[r], (unsigned)(W - (x0 + __ffsll((long long)m) - 1)));
      atomicMax(&s_box[kVisMaxQ + r], (unsigned)(H - y));
      atomicMax(&s_box[2 * kVisMaxQ + r], (unsigned)(x0 + 64 - __clzll((long long)m)));
      atomicMax(&s_box[3 * kVisMaxQ + r], (unsigned)(y + 1));
    }
  }
};

template <int MODE>
struct VisEmitOut {
  void* out;                        // this frame's [Ko][H][W] bytes or [Ko][H][ceil(W/64)] words
  int H, W;
  __device__ __forceinline__ void operator()(int r, float v, bool live, int y, int x0) const {
    const bool pos = live && v > 0.f;
    if constexpr (MODE == kVisEmitU8) {
      if (live) static_cast<unsigned char*>(out)[((long long)r * H + y) * W + x0 + (threadIdx.x & (kWave - 1))] = pos ? 1 : 0;
    } else {
      const unsigned long long m = __ballot(pos);      // bit i = pixel x0 + i; pixels past the row's end are not live: tail bits zero
      if ((threadIdx.x & (kWave - 1)) == 0 && y < H) static_cast<unsigned long long*>(out)[((long long)r * H + y) * ((W + 63) / 64) + x0 / 64] = m;
    }
  }
};

// grid (workgroups per frame, frames): a workgroup takes `tiles_per_wg` consecutive tiles of its frame.  g.N = Q; logits [T][Q][h][w].
// The list of frame t: list + t * list_stride, *(count + t * count_stride) entries (the referenced queries, or the selected ones).
template <int DT, int MODE>
__global__ __launch_bounds__(kVisThreads) void vis_tile_kernel(const void* __restrict__ logits, PanGeom g, const int* __restrict__ list, int list_stride,
                                                               const int* __restrict__ count, int count_stride, int tiles_per_wg, int Ko, VisAcc acc,
                                                               void* __restrict__ masks) {
  __shared__ float s_tile[kVisLdsFloats];
  __shared__ int s_list[kVisMaxQ];
  __shared__ unsigned char s_some[kVisMaxQ];
  const int tid = threadIdx.x, t = blockIdx.y;
  const int nl = min(count[(long long)t * count_stride], kVisMaxQ);
  for (int i = tid; i < nl; i += kVisThreads) s_list[i] = list[(long long)t * list_stride + i];
  const int tx_n = (g.W + kVisTileW - 1) / kVisTileW, ty_n = (g.H + kVisTileH - 1) / kVisTileH, ntile = tx_n * ty_n;
  const long long frame = (long long)g.h * g.w;
  const PanGlobalSrc<DT> gsrc{logits, (long long)t * g.N * frame, frame, g.w};

  auto tiles = [&](auto sink) {
    const int first = blockIdx.x * tiles_per_wg, last = min(first + tiles_per_wg, ntile);
    for (int tile = first; tile < last; ++tile) {
      const int y0 = tile / tx_n * kVisTileH, x0 = tile % tx_n * kVisTileW;
      int rlo, rhi, clo, chi;
      pan_range(y0, min(y0 + kVisTileH, g.H) - 1, g, g.y1, g.y2, &rlo, &rhi);
      pan_range(x0, min(x0 + kVisTileW, g.W) - 1, g, g.x1, g.x2, &clo, &chi);
      const int bh = rhi - rlo + 1, bw = chi - clo + 1, box = bh * bw;
      const int y = y0 + tid / kVisTileW, x = x0 + tid % kVisTileW;
      const bool live = y < g.H && x < g.W;
      const int yc = min(y, g.H - 1), xc = min(x, g.W - 1);         // threads past the edge evaluate an edge pixel and discard it
      PanPixel<2> px;
      if (box <= kVisBox) {
        const PanLdsSrc lsrc{s_tile, box, bw, rlo, clo};
        px.setup(yc, xc, g, lsrc);
        const int per = kVisLdsFloats / box;
        for (int r0 = 0; r0 < nl; r0 += per) {
          const int nb = min(per, nl - r0);
          __syncthreads();                      // the previous block's readers are done (and s_list is written before the first)
          for (int e = tid; e < nb * box; e += kVisThreads) {
            const int n = e / box, q = e - n * box, r = q / bw, c = q - r * bw;
            s_tile[e] = gsrc(s_list[r0 + n], (rlo + r) * g.w + (clo + c));
          }
          __syncthreads();
          // A resized logit is a convex combination of the box's values: a query whose box has no positive value has no pixel in
          // this tile (exactly so in fp32: non-negative weights times non-positive values).  Most tiles of most queries are such.
          for (int n = tid; n < nb; n += kVisThreads) {
            float mx = s_tile[n * box];
            for (int j = 1; j < box; ++j) mx = fmaxf(mx, s_tile[n * box + j]);
            s_some[n] = mx > 0.f ? 1 : 0;
          }
          __syncthreads();
          for (int n = 0; n < nb; ++n) {
            if (s_some[n]) sink(r0 + n, px.eval<true>(n, lsrc), live, y, x0);
            else if constexpr (MODE != kVisStats) sink(r0 + n, -1.f, live, y, x0);
          }
        }
      } else {
        __syncthreads();                        // (s_list before the first tile)
        px.setup(yc, xc, g, gsrc);
        for (int r = 0; r < nl; ++r) sink(r, px.eval(s_list[r], gsrc), live, y, x0);
      }
    }
  };

  if constexpr (MODE == kVisStats) {
    __shared__ unsigned s_area[kVisMaxQ], s_box[4 * kVisMaxQ];
    __shared__ unsigned long long s_sum[kVisMaxQ];
    for (int i = tid; i < nl; i += kVisThreads) s_area[i] = 0, s_sum[i] = 0, s_box[i] = s_box[kVisMaxQ + i] = s_box[2 * kVisMaxQ + i] = s_box[3 * kVisMaxQ + i] = 0;
    tiles(VisStatsOut{s_area, s_sum, s_box, g.H, g.W});        // (its first barrier comes before any accumulation)
    __syncthreads();
    for (int i = tid; i < nl; i += kVisThreads)
      if (s_area[i]) {
        const long long at = (long long)t * g.N + s_list[i];
        atomicAdd(&acc.area[at], s_area[i]);
        atomicAdd(&acc.sum[at], s_sum[i]);
#pragma unroll
        for (int k = 0; k < 4; ++k) atomicMax(&acc.box[at * 4 + k], s_box[k * kVisMaxQ + i]);
      }
  } else {
    const long long per_mask = MODE == kVisEmitU8 ? (long long)g.H * g.W : (long long)g.H * ((g.W + 63) / 64) * 8;
    char* out = static_cast<char*>(masks) + (long long)t * Ko * per_mask;
    tiles(VisEmitOut<MODE>{out, g.H, g.W});
    // rows past the frame's count (fewer candidates than k_out): empty masks
    const int first = blockIdx.x * tiles_per_wg, last = min(first + tiles_per_wg, ntile);
    for (int r = nl; r < Ko; ++r)
      for (int tile = first; tile < last; ++tile) {
        const int y = tile / tx_n * kVisTileH + tid / kVisTileW, x0 = tile % tx_n * kVisTileW;
        VisEmitOut<MODE>{out, g.H, g.W}(r, -1.f, y < g.H && x0 + tid % kVisTileW < g.W, y, x0);
      }
  }
}

// grid: one workgroup per frame.  Finishes the candidates' scores and boxes and writes the frame's top Ko rows.
__global__ __launch_bounds__(kVisMaxCand) void vis_select_kernel(VisTabs tb, VisAcc acc, int Q, int K, int Ko, int H, int W) {
  __shared__ double s_det[kVisMaxCand];
  const int c = threadIdx.x, t = blockIdx.x, ncand = tb.head[0];
  const long long row = (long long)t * K + c;
  double det = -1.0;
  float bx[4] = {0.f, 0.f, 0.f, 0.f};
  int q = -1;
  if (c < ncand) {
    q = tb.cand_query[c];
    const long long at = (long long)t * Q + q;
    const unsigned a = acc.area[at];
    // sum(sigmoid * binary) / (area + 1e-6), then * the class score
    const double ms = (double)acc.sum[at] / (double)kVisFix / ((double)a + 1e-6);
    det = (double)tb.cls[c] * ms;
    if (a) bx[0] = (float)(W - (int)acc.box[at * 4]), bx[1] = (float)(H - (int)acc.box[at * 4 + 1]), bx[2] = (float)acc.box[at * 4 + 2], bx[3] = (float)acc.box[at * 4 + 3];
    tb.area[row] = (int)a, tb.mask_score[row] = (float)ms, tb.det[row] = (float)det;
#pragma unroll
    for (int k = 0; k < 4; ++k) tb.cand_box[row * 4 + k] = bx[k];
  } else if (c < K) {
    tb.area[row] = -1, tb.mask_score[row] = -1.f, tb.det[row] = -1.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) tb.cand_box[row * 4 + k] = -1.f;
  }
  s_det[c] = det;
  __syncthreads();
  const int n = min(ncand, Ko);
  if (c < ncand) {         // descending; equal scores (the empty masks: 0): the lower candidate position first
    int rank = 0;
    for (int j = 0; j < ncand; ++j) rank += (s_det[j] > det || (s_det[j] == det && j < c)) ? 1 : 0;
    if (rank < Ko) {
      const long long o = (long long)t * Ko + rank;
      tb.track[o] = c + 1, tb.label[o] = tb.cand_label[c], tb.query[o] = q, tb.score[o] = (float)det;
#pragma unroll
      for (int k = 0; k < 4; ++k) tb.box[o * 4 + k] = bx[k];
    }
  }
  if (c >= n && c < Ko) {
    const long long o = (long long)t * Ko + c;
    tb.track[o] = tb.label[o] = tb.query[o] = -1, tb.score[o] = -1.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) tb.box[o * 4 + k] = -1.f;
  }
  if (c == 0) tb.count[t] = n;
}

}  // namespace axvs
