// Device pieces that several units need and that exist once: the NCHW <-> rows kernel pair and two row kernels of the
// query decoders.
//   nchw_to_rows<GELU>()        [N, C, HW] -> rows [N*HW][C]                                      } either way optionally through gelu
//   rows_to_nchw<GELU>()        rows (n, p) at t + n*batch_stride + p*ld -> [N, C, HW]            }
//   class_logits_rows<RC>()     cls[row][k] = y[row] . w[k] + b[k], rows of RC = 256
//   broadcast_rows<RC>()        x[n*Q + q] = src[q], rows of RC = 256, one or two (source, destination) pairs per launch
// Kernels and launchers are static templates: a unit that calls a launcher carries its own copy of the kernel in its code object, the
// others none (a static kernel that no template stands in front of is emitted into every unit that includes its header, and so is a
// kernel template that such a launcher names), and no symbol stands in two code objects' export lists.
// A layout copy is exact, so the tile form is free: both directions use the 64 (pixels) x 64 (channels) tile with float4 accesses on
// the row side that the pixel decoder's input projections were tuned on.
#pragma once
#include "axvs_common.h"

namespace axvs {

// ---- [N, C, HW] -> rows [N*HW][C] --------------------------------------------------------------------------------------------------------
// 64 channels x 64 pixels per workgroup through LDS; any C and HW (pixel rows start at 4-byte boundaries).  VEC: the rows take float4
// stores (C a multiple of 4, t 16-byte aligned: the launcher decides).  grid (ceil(HW/64), ceil(C/64), N), 256 threads.
template <bool GELU, bool VEC>
static __global__ __launch_bounds__(256) void nchw_to_rows_kernel(const float* __restrict__ x, float* __restrict__ t, int C, int HW) {
  __shared__ float tile[64][65];
  const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64, n = blockIdx.z;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;      // read: tx = pixel, 4 channel rows at a time
  const float* src = x + ((long long)n * C + c0) * HW + p0;
  float v[16];                 // all 16 loads of a thread in flight before the first LDS store (four at a time left the kernel at 1.7 TB/s)
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = ty + 4 * i;
    v[i] = (c0 + c < C && p0 + tx < HW) ? src[(long long)c * HW + tx] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) tile[ty + 4 * i][tx] = GELU ? gelu_exact(v[i]) : v[i];
  __syncthreads();
  float* dst = t + ((long long)n * HW + p0) * C + c0;
  if constexpr (VEC) {
    // write: 16 threads x float4 cover the 64 channels of a pixel row (256 contiguous bytes), 16 pixels per round
    const int wc = (threadIdx.x & 15) * 4, wp = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = wp + 16 * i;
      if (p0 + p < HW && c0 + wc < C)
        *reinterpret_cast<float4*>(dst + (long long)p * C + wc) = float4{tile[wc][p], tile[wc + 1][p], tile[wc + 2][p], tile[wc + 3][p]};
    }
  } else {
    // a wave = the 64 channels of a pixel row, 4 pixels per round
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int p = ty + 4 * i;
      if (p0 + p < HW && c0 + tx < C) dst[(long long)p * C + tx] = tile[tx][p];
    }
  }
}

template <bool GELU = false>
static inline void nchw_to_rows(const float* x, float* t, int N, int C, int HW, hipStream_t st) {
  const bool vec = C % 4 == 0 && reinterpret_cast<uintptr_t>(t) % 16 == 0;
  hipLaunchKernelGGL((vec ? nchw_to_rows_kernel<GELU, true> : nchw_to_rows_kernel<GELU, false>), dim3((unsigned)((HW + 63) / 64), (unsigned)((C + 63) / 64), (unsigned)N),
                     dim3(256), 0, st, x, t, C, HW);
}

// ---- rows -> [N, C, HW] ------------------------------------------------------------------------------------------------------------------
// The same tile the other way; the rows may be a slice of a wider buffer (row (n, p) at t + n*t_batch_stride + p*t_ld).  VEC: the rows
// take float4 loads.  grid (ceil(HW/64), ceil(C/64), N), 256 threads.
template <bool GELU, bool VEC>
static __global__ __launch_bounds__(256) void rows_to_nchw_kernel(const float* __restrict__ t, float* __restrict__ x, int C, int HW, long long t_batch_stride,
                                                                  long long t_ld) {
  __shared__ float tile[64][65];
  const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64, n = blockIdx.z;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const float* src = t + (long long)n * t_batch_stride + (long long)p0 * t_ld + c0;
  if constexpr (VEC) {
    const int rc = (threadIdx.x & 15) * 4, rp = threadIdx.x >> 4;      // read: 16 threads x float4 cover 64 channels of a pixel row
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = rp + 16 * i;
      float4 v = {0.f, 0.f, 0.f, 0.f};
      if (p0 + p < HW && c0 + rc < C) v = *reinterpret_cast<const float4*>(src + (long long)p * t_ld + rc);
      tile[p][rc] = v.x; tile[p][rc + 1] = v.y; tile[p][rc + 2] = v.z; tile[p][rc + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int p = ty + 4 * i;
      tile[p][tx] = (p0 + p < HW && c0 + tx < C) ? src[(long long)p * t_ld + tx] : 0.f;
    }
  }
  __syncthreads();
  float* dst = x + ((long long)n * C + c0) * HW + p0;      // write: tx = pixel, 4 channel rows at a time
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const int c = ty + 4 * i;
    if (c0 + c < C && p0 + tx < HW) dst[(long long)c * HW + tx] = GELU ? gelu_exact(tile[tx][c]) : tile[tx][c];
  }
}

// t_ld = 0: contiguous rows [N*HW][C]
template <bool GELU = false>
static inline void rows_to_nchw(const float* t, float* x, int N, int C, int HW, hipStream_t st, long long t_batch_stride = 0, long long t_ld = 0) {
  if (!t_ld) t_ld = C, t_batch_stride = (long long)HW * C;
  const bool vec = C % 4 == 0 && t_ld % 4 == 0 && t_batch_stride % 4 == 0 && reinterpret_cast<uintptr_t>(t) % 16 == 0;
  hipLaunchKernelGGL((vec ? rows_to_nchw_kernel<GELU, true> : rows_to_nchw_kernel<GELU, false>), dim3((unsigned)((HW + 63) / 64), (unsigned)((C + 63) / 64), (unsigned)N), dim3(256), 0, st,
                     t, x, C, HW, t_batch_stride, t_ld);
}

// ---- rows of RC floats (256: the embed dims of both query decoders) --------------------------------------------------------------------------
// cls[row][k] = y[row] . w[k] + b[k]   (K + 1 classes: any count, so not a tile of the GEMM; b may hold the bias towards void)
template <int RC>
static __global__ __launch_bounds__(256) void class_logits_rows_kernel(const float* __restrict__ y, const float* __restrict__ w, const float* __restrict__ b,
                                                                       float* __restrict__ cls, int rows, int K1) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)rows * K1) return;
  const float* const yr = y + (i / K1) * RC;
  const float* const wr = w + (i % K1) * RC;
  float acc = 0.f;
  for (int c = 0; c < RC; ++c) acc = fmaf(yr[c], wr[c], acc);
  cls[i] = acc + b[i % K1];
}

template <int RC = 256>
static inline void class_logits_rows(const float* y, const float* w, const float* b, float* cls, int rows, int K1, hipStream_t st) {
  hipLaunchKernelGGL(class_logits_rows_kernel<RC>, dim3((unsigned)(((size_t)rows * K1 + 255) / 256)), dim3(256), 0, st, y, w, b, cls, rows, K1);
}

// x0[n*Q + q] = s0[q] (blockIdx.y = 0) and x1[n*Q + q] = s1[q] (blockIdx.y = 1: only where the launch has a second pair)
template <int RC>
static __global__ __launch_bounds__(256) void broadcast_rows_kernel(const float* __restrict__ s0, float* __restrict__ x0, const float* __restrict__ s1,
                                                                    float* __restrict__ x1, int Q, int rows) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)rows * RC) return;
  const size_t src = (i / RC % Q) * RC + i % RC;
  if (blockIdx.y == 0) x0[i] = s0[src];
  else x1[i] = s1[src];
}

template <int RC = 256>
static inline void broadcast_rows(const float* s0, float* x0, int Q, int rows, hipStream_t st, const float* s1 = nullptr, float* x1 = nullptr) {
  hipLaunchKernelGGL(broadcast_rows_kernel<RC>, dim3((unsigned)(((size_t)rows * RC + 255) / 256), s1 ? 2u : 1u), dim3(256), 0, st, s0, x0, s1, x1, Q, rows);
}

}  // namespace axvs
