// Host scaffold shared by the eval-forward units (axvs_m2f.hip, axvs_kmax.hip, axvs_kmax_pix.hip, axvs_convnext.hip): the Linear layer
// on the split-precision GEMM, the slot lists of a packed blob (a parameter struct read as an array of pointers, axial_vs_amd/_params.py
// states the same order), and a flat block index -> (stage, block of the stage).  The device pieces they share: axvs_layout.h.
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

}  // namespace axvs
