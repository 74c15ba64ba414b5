// Host scaffold shared by the eval-forward units (axvs_m2f.hip, axvs_kmax.hip, axvs_kmax_pix.hip, axvs_convnext.hip): the Linear layer
// on the split-precision GEMM, the slot lists of a packed blob (a parameter struct read as an array of pointers, axial_vs_amd/_params.py
// states the same order), a flat block index -> (stage, block of the stage), and the one layout kernel two of them share.
//   rows_to_nchw_kernel     rows [N*h*w][C] -> [N, C, h, w]
#pragma once
#include "axvs_gemm_nt.h"
#include "axvs_host.h"

namespace axvs {

constexpr int kActNone = 0, kActRelu = 1, kActGelu = 2, kActGeluAfterRes = 3;      // GemmEpi::relu; 2 and 3 under GemmNtForm::gelu alone
constexpr tr::GemmNtForm kForm3{3}, kForm3Gelu{3, false, true};                    // three bf16 pieces per operand: two instantiations

// Y[M][N] (row stride ldc) = act((X (+ X2))[M][K] (row stride lda) W[N][K]^T + bias) (+ res[M][ldc]); kActGeluAfterRes: the gelu comes
// behind the residual
inline int linear(const float* X, long long lda, const float* W, const float* bias, float* Y, long long M, int N, int K, long long ldc, int act, const float* res,
                  tr::GemmNtForm form, hipStream_t st, const float* X2 = nullptr) {
  tr::GemmLd ld{lda, K, ldc, 0, X2};
  tr::GemmEpi e{bias, 1.f, act, tr::Drop{0u, 0u, 0u, 1.f}, 0.f};
  e.res = res;
  return tr::gemm_nt(X, W, Y, M, N, K, ld, e, form, 1, st);
}

// ---- slot lists: n[s] floats per slot, a zero-sized slot has no view and no source -------------------------------------------------------------
inline void carve_slots(Carver& cv, const size_t* n, int slots, float** dst) {
  for (int s = 0; s < slots; ++s) dst[s] = n[s] ? cv.f(n[s]) : nullptr;
}

inline int copy_f(float* dst, const float* src, size_t n, hipStream_t st) {
  if (hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(AXVS_ERR_LAUNCH, "hipMemcpyAsync failed");
  return AXVS_OK;
}

// the caller's parameter struct `src_struct` -> the views carve_slots() gave; what / index: the struct's name in the refusal
inline int copy_slots(float* const* dst, const void* src_struct, const size_t* n, int slots, const char* what, int index, hipStream_t st) {
  const float* const* src = reinterpret_cast<const float* const*>(src_struct);
  for (int s = 0; s < slots; ++s) {
    if (!n[s]) continue;
    if (!src[s]) return fail(AXVS_ERR_ARG, "null pointer (%s %d, parameter %d)", what, index, s);
    if (int rc = copy_f(dst[s], src[s], n[s], st)) return rc;
  }
  return AXVS_OK;
}

// block `index` of the whole decoder / network (`whose`) -> (stage, block of the stage), counts[i] blocks in stage i
inline int locate(const int (&counts)[4], int index, const char* whose, int* stage, int* j) {
  for (int i = 0; i < 4; ++i) {
    if (index >= 0 && index < counts[i]) {
      *stage = i, *j = index;
      return AXVS_OK;
    }
    index -= counts[i];
  }
  return fail(AXVS_ERR_ARG, "block index outside the %s blocks", whose);
}

// ---- rows [N*hw][C] -> [N, C, hw]: a 32 (pixels) x 64 (channels) tile through LDS.  grid (ceil(hw/32) * ceil(C/64), N), 256 threads ----
// (static: each unit that launches it carries its own copy in its code object, the others none)
static __global__ __launch_bounds__(256) void rows_to_nchw_kernel(const float* __restrict__ rows, float* __restrict__ out, int C, int hw) {
  __shared__ float tile[32][65];
  const int tid = threadIdx.x;
  const int cchunks = (C + 63) / 64;
  const int p0 = (int)(blockIdx.x / cchunks) * 32, c0 = (int)(blockIdx.x % cchunks) * 64;
  const size_t n = blockIdx.y;
  {
    const int c = tid & 63, pr = tid >> 6;
    if (c0 + c < C) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int p = p0 + pr + 4 * j;
        if (p < hw) tile[pr + 4 * j][c] = rows[(n * hw + p) * C + c0 + c];
      }
    }
  }
  __syncthreads();
  const int tx = tid & 31, cy = tid >> 5, p = p0 + tx;
  if (p >= hw) return;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = c0 + cy + 8 * j;
    if (c < C) out[(n * C + c) * (size_t)hw + p] = tile[tx][cy + 8 * j];
  }
}

static inline void rows_to_nchw(const float* rows, float* out, int N, int C, int hw, hipStream_t st) {
  hipLaunchKernelGGL(rows_to_nchw_kernel, dim3((unsigned)((hw + 31) / 32 * ((C + 63) / 64)), (unsigned)N), dim3(256), 0, st, rows, out, C, hw);
}

}  // namespace axvs
