// C[M,N] = epilogue(A[M,K] B[N,K]^T) on fp32 operands in split precision ("bf16x3" / three-piece): the GEMM of the training tier's
// Linear layers (axvs_train_gemm.h has the story), which the inference path uses too for projections whose fp32 inputs and outputs
// make a 128 x 128 tile pay (the deformable attention's projections and the 1x1 convolutions of axvs_pixdec.hip, the query decoders of
// axvs_m2f.hip and axvs_kmax.hip).  This header is what its callers see: the argument structs and gemm_nt(), the one launcher.  The
// kernel itself, tr_gemm_nt_kernel, is instantiated and launched in axvs_gemm_nt.hip alone: one code object carries each
// instantiation, and every caller gets the same argument checks.
#pragma once
#include "axvs_common.h"

namespace axvs {
namespace tr {

__host__ __device__ __forceinline__ unsigned fmix32(unsigned h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// keep element `idx` of dropout site `site` iff (hash >> 8) >= thr, thr = floor(p * 2^24)
struct Drop {
  unsigned seed, site, thr;
  float scale;   // 1 / (1 - p)
};

__host__ __device__ __forceinline__ unsigned drop_hash(unsigned seed, unsigned site, unsigned long long idx) {
  unsigned h = seed ^ (site * 0x9E3779B9u);
  h = fmix32(h ^ (unsigned)idx);
  h = fmix32(h ^ (unsigned)(idx >> 32));
  return h;
}

__device__ __forceinline__ float drop_keep(const Drop& d, unsigned long long idx) {   // 0 or 1/(1-p)
  if (d.thr == 0) return 1.f;
  return (drop_hash(d.seed, d.site, idx) >> 8) >= d.thr ? d.scale : 0.f;
}

constexpr int kGT = 128;                 // block tile (both output dimensions)
constexpr int kGK = 32;                  // contraction step
constexpr int kGTileElems = kGT * kGK;   // one 16-bit operand tile
constexpr int kGLd = kGT + 4;            // fp32 row stride of the epilogue staging tile
constexpr size_t kGemmLds = (size_t)kGT * kGLd * sizeof(float);   // 67.6 KB >= 2 stages x 4 tiles x 8 KB

struct GemmLd {     // row strides (floats, multiples of 4) of A, B, C; ksteps > 0: split-K, that many 32-wide k-steps per blockIdx.z
  long long a, b, c;
  int ksteps;
  const float* a2 = nullptr;   // optional second A operand with A's shape and stride, added element-wise on load (x + pos)
  // alignment (in floats: 4, 2 or 1) every row start of A, B, C is known to have.  4: 16-byte vector accesses (the rule: row
  // strides and extents multiples of 4); smaller: rows of pixels whose count is whatever the image size gives (the mask einsum
  // over 193 x 337 maps) -- narrower accesses, and an extent that is not a multiple of 4 ends inside a group of four
  int al_a = 4, al_b = 4, al_c = 4;
  // tr_gemm_tn_kernel<.., STATS>: the output tile's sum (x - *stat_shift) and sum (x - *stat_shift)^2 go to
  // stat_part[(g stat_nblk + stat_blk0 + tile)][2], g = first row of the tile / stat_rows (a tile lies inside one group of rows) --
  // the one-channel BatchNorm statistics of the mask logits without a pass of their own over them
  // tr_gemm_nt_kernel<.., AFF>: the A operand is an affine function of A and a2, per group of aff_rows rows:
  // A_eff = aff[3 g] A + aff[3 g + 1] a2 + aff[3 g + 2], g = row / aff_rows (the input gradient of a one-channel BatchNorm formed in the
  // loader of the GEMM that consumes it, instead of a pass that writes it out)
  const float* aff = nullptr;
  int aff_rows = 1;
  float* stat_part = nullptr;
  const float* stat_shift = nullptr;
  int stat_nblk = 0, stat_blk0 = 0, stat_rows = 0;
  // tr_gemm_tn_kernel<.., GRP>: output row n starts at (n / c_grp_rows) c_grp_ld + (n % c_grp_rows) c -- rows (layer, query)
  // of the Tube-Link mask einsum written straight into [layer][B][T][Q][pixels]
  int c_grp_rows = 0;
  long long c_grp_ld = 0;
};

inline bool gemm_nt_general(const GemmLd& ld, int K) { return !(ld.al_a == 4 && ld.al_b == 4 && (K & 3) == 0); }

struct GemmEpi {
  const float* bias;   // nullable [N]: added first
  float mul;           // then multiplied
  int relu;            // then max(., 0); with GemmNtForm::gelu also 2 / 3 / 4, see there
  Drop dr;             // then dropout, element index row * N + col (thr = 0: none)
  float beta;          // 0: overwrite C, 1: add to it
  const float* res = nullptr;   // optional residual [M][ldc], added last (out = ... + res)
  const float* res2 = nullptr;  // a second one (d_in = dv Wv + d_out + da in one epilogue)
  // out16 != nullptr: the result goes out as ONE 16-bit piece in the blocked activation layout [N/32][M][32] (kind16: 1 f16, 2 bf16)
  // instead of fp32 rows; rows flagged in zero_rows (nullable, one byte per row) are written as zeros
  u16* out16 = nullptr;
  int kind16 = 0;
  const unsigned char* zero_rows = nullptr;
};

// NS pieces of eight floats: bf16 pieces that sum to the value (each the rounding of what the ones before it left), or with F16 the
// one fp16 rounding -- the operand split of tr_gemm_nt_kernel (axvs_gemm_nt.hip) and tr_gemm_tn_kernel (axvs_train_gemm.h)
template <int NS, bool F16 = false>
__device__ __forceinline__ void split_n(const float4& a, const float4& b, u16x8 (&p)[NS]) {
  const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float r = x[i];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if constexpr (F16) {
        p[s][i] = __builtin_bit_cast(u16, (_Float16)r);
      } else {
        const __bf16 h = (__bf16)r;
        p[s][i] = __builtin_bit_cast(u16, h);
        r -= (float)h;                       // exact in fp32
      }
    }
  }
}

// What the caller alone decides about a launch; the loader (general, addend, affine) follows from GemmLd.
struct GemmNtForm {
  int pieces;          // 16-bit pieces per operand: 3 (fp32 accuracy, six MFMAs per product), 2 (1.5e-5, three), 1 (autocast's products)
  bool f16 = false;    // pieces == 1: an fp16 piece instead of a bf16 one
  bool gelu = false;   // GemmEpi::relu also takes 2 (exact GELU in the ReLU's place), 3 (exact GELU after the residuals: out =
                       // gelu(... + res)) and 4 (ReLU after the residuals: out = relu(... + res)): an instantiation of its own, three
                       // pieces on the 16-byte loader without addend
};

// The refusals of gemm_nt() alone, no device work (AXVS_ERR_ARG with a message): N and the row strides against the stated alignment,
// the affine loader without its second operand, relu > 1 without `gelu`, a form outside the instantiations that exist.
// variant (nullable, out): the instantiation the call takes, in the encoding of AxvsTestGemm::variant (include/axvs.h)
int gemm_nt_check(int N, int K, const GemmLd& ld, const GemmEpi& ep, GemmNtForm f, int* variant = nullptr);

// C[M,N] = epilogue(A[M,K] B[N,K]^T): the checks, the instantiation's dynamic LDS limit (raised once per device), the launch of grid
// (ceil(M / 128), ceil(N / 128), zsplits) on `st`.  M <= 0: nothing to do.  variant: set when a kernel was launched.
// dev: the current device where the caller knows it (the training tier fetches it once per entry point), -1: ask the runtime
int gemm_nt(const float* A, const float* B, float* C, long long M, int N, int K, const GemmLd& ld, const GemmEpi& ep, GemmNtForm f, int zsplits,
            hipStream_t st, int dev = -1, int* variant = nullptr);

}  // namespace tr
}  // namespace axvs
