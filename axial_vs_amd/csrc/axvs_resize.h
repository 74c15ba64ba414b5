// The bilinear resize shared by the post-processing units (axvs_panoptic.h, axvs_vis.h): torch's index arithmetic for one axis, the
// low-resolution box an output tile reads, tap sources (LDS tile / global memory), the one- or two-stage evaluation of one output
// pixel, and the workgroup integer sum both units' table passes use.
#pragma once
#include <hip/hip_runtime.h>

#include "axvs_common.h"

namespace axvs {

enum { kPanF16 = 0, kPanBf16 = 1, kPanF32 = 2 };

// one bilinear stage along one axis: torch's area_pixel_compute_scale / area_pixel_compute_source_index (upsample_bilinear2d)
struct PanAxis { int in, out; float scale; };
struct PanGeom {
  int N, T, h, w, H, W;             // logits [N,T,h,w] -> map [T,H,W]
  int two, ac;                      // two stages (crop between them); align_corners
  PanAxis y1, x1, y2, x2;           // stage 1: (h, w) -> padded image; stage 2: the crop -> (H, W)
  float thr;
};

struct PanTap { int i0, i1; float l0, l1; };

__device__ __forceinline__ PanTap pan_tap(int dst, const PanAxis& a, int ac) {
  float src = ac ? a.scale * (float)dst : fmaxf(a.scale * ((float)dst + 0.5f) - 0.5f, 0.f);
  int i0 = min((int)src, a.in - 1);
  PanTap t;
  t.i0 = i0;
  t.i1 = i0 + (i0 < a.in - 1 ? 1 : 0);
  t.l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
  t.l0 = 1.f - t.l1;
  return t;
}

template <int DT>
__device__ __forceinline__ float pan_load(const void* p, long long i) {
  if constexpr (DT == kPanF32) return static_cast<const float*>(p)[i];
  else if constexpr (DT == kPanF16) return (float)static_cast<const _Float16*>(p)[i];
  else return __uint_as_float((unsigned)static_cast<const u16*>(p)[i] << 16);
}

// low-resolution rows (columns) the output rows [d0, d1] read
__device__ __forceinline__ void pan_range(int d0, int d1, const PanGeom& g, const PanAxis& a1, const PanAxis& a2, int* lo, int* hi) {
  if (g.two) {
    d0 = pan_tap(d0, a2, g.ac).i0;
    d1 = pan_tap(d1, a2, g.ac).i1;
  }
  *lo = pan_tap(d0, a1, g.ac).i0;
  *hi = pan_tap(d1, a1, g.ac).i1;
}

template <int DT>
struct PanGlobalSrc {             // taps straight from the logits of frame t (a tile whose low-resolution box does not fit in LDS)
  const void* p;
  long long base, sn;
  int w;
  __device__ __forceinline__ float operator()(int n, int off) const { return pan_load<DT>(p, base + n * sn + off); }
  __device__ __forceinline__ int off(int r, int c) const { return r * w + c; }
};
struct PanLdsSrc {
  const float* s;
  int sn, bw, rlo, clo;
  __device__ __forceinline__ float operator()(int n, int off) const { return s[n * sn + off]; }
  __device__ __forceinline__ int off(int r, int c) const { return (r - rlo) * bw + (c - clo); }
};

// The taps of one output pixel: NS = 1 (one stage) or 2 stage-1 points per axis, each with two low-resolution taps.
template <int NS>
struct PanPixel {
  int off[NS][NS][4];
  float wy[NS][2], wx[NS][2], ly[2], lx[2];
  template <class Src>
  __device__ __forceinline__ void setup(int y, int x, const PanGeom& g, const Src& s) {
    int ys[2] = {y, y}, xs[2] = {x, x};
    if constexpr (NS == 2) {
      PanTap ty = pan_tap(y, g.y2, g.ac), tx = pan_tap(x, g.x2, g.ac);
      ys[0] = ty.i0, ys[1] = ty.i1, xs[0] = tx.i0, xs[1] = tx.i1;
      ly[0] = ty.l0, ly[1] = ty.l1, lx[0] = tx.l0, lx[1] = tx.l1;
    }
    PanTap ry[NS], rx[NS];
#pragma unroll
    for (int a = 0; a < NS; ++a) {
      ry[a] = pan_tap(ys[a], g.y1, g.ac);
      rx[a] = pan_tap(xs[a], g.x1, g.ac);
      wy[a][0] = ry[a].l0, wy[a][1] = ry[a].l1, wx[a][0] = rx[a].l0, wx[a][1] = rx[a].l1;
    }
#pragma unroll
    for (int a = 0; a < NS; ++a)
#pragma unroll
      for (int b = 0; b < NS; ++b) {
        off[a][b][0] = s.off(ry[a].i0, rx[b].i0);
        off[a][b][1] = s.off(ry[a].i0, rx[b].i1);
        off[a][b][2] = s.off(ry[a].i1, rx[b].i0);
        off[a][b][3] = s.off(ry[a].i1, rx[b].i1);
      }
  }
  // upsample_bilinear2d's expression, stage by stage: h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d).  FENCE (for an LDS source with
  // two stages): the sixteen reads go out in two batches of eight -- lgkmcnt counts to 15, and a wave with sixteen reads in flight can
  // pass its wait early (axvs_common.h: lds_fence; tools/check_lgkm.py scans for it)
  template <bool FENCE = false, class Src>
  __device__ __forceinline__ float eval(int n, const Src& s) const {
    float u[NS][NS];
#pragma unroll
    for (int a = 0; a < NS; ++a) {
#pragma unroll
      for (int b = 0; b < NS; ++b)
        u[a][b] = wy[a][0] * (wx[b][0] * s(n, off[a][b][0]) + wx[b][1] * s(n, off[a][b][1])) +
                  wy[a][1] * (wx[b][0] * s(n, off[a][b][2]) + wx[b][1] * s(n, off[a][b][3]));
      if constexpr (FENCE && NS == 2)
        if (a == 0) lds_fence();
    }
    if constexpr (NS == 1) return u[0][0];
    else return ly[0] * (lx[0] * u[0][0] + lx[1] * u[0][1]) + ly[1] * (lx[0] * u[1][0] + lx[1] * u[1][1]);
  }
};

__device__ __forceinline__ int pan_block_sum(int v, int* s_red, int nthreads) {
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  __syncthreads();                              // s_red of the previous call has been read
  if ((threadIdx.x & (kWave - 1)) == 0) s_red[threadIdx.x / kWave] = v;
  __syncthreads();
  int tot = 0;
  for (int i = 0; i < nthreads / kWave; ++i) tot += s_red[i];
  return tot;
}

}  // namespace axvs
