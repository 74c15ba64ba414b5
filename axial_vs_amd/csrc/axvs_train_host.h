// Host side the families of the training tier share (axvs_train.hip is their one translation unit): the GEMM launcher, shapes and
// buffers of a trajectory pass, the launch context with its weight- / input-gradient wrappers, one trajectory pass forward and backward,
// and the checks and setup every training entry point makes.  Everything has internal linkage, like the kernels of axvs_glue_train.h.
#pragma once
#include "axvs_host.h"
#include "axvs_train.h"
#include "axvs_train_gemm.h"

namespace axvs {
namespace {

using namespace tr;

// ---- the Linear layers' GEMMs: split-precision bf16 MFMA kernels (axvs_train_gemm.h) ------------------------------------------------
// The instantiation the last Gemm launch of this thread ran (include/axvs.h, AxvsTestGemm::variant, has the encoding): set by
// gemm_nt (through nt) and launch_tn, the only places that launch the GEMM kernels, and reported by axvs_test_train_gemm.
inline thread_local int t_gemm_variant = 0;

struct Gemm {
  hipStream_t st = nullptr;
  static constexpr int kNoDevice = -2;      // (never equal to `dev`, not even before init())
  int dev = -1;          // the current device, fetched once per entry-point call (init)
  int init(hipStream_t s) {
    st = s;
    if (hipGetDevice(&dev) != hipSuccess) return fail(AXVS_ERR_LAUNCH, "hipGetDevice failed");
    return AXVS_OK;
  }
  // The dY^T X kernels take more dynamic LDS than the default limit: launch_tn raises the limit of the instantiation it is about to
  // launch (gemm_nt does the same).  `seen_dev` is that instantiation's own thread_local: the device it was last raised on, so a repeat launch
  // costs a compare (a thread that alternates between devices falls through to ensure_max_lds, which remembers every (device, kernel) pair).
  int raise_lds(const void* fn, int& seen_dev) const {
    if (seen_dev == dev) return AXVS_OK;
    if (int rc = ensure_max_lds(fn)) return rc;
    seen_dev = dev;
    return AXVS_OK;
  }
  // The policy of nt(): affine A operand (an input-gradient GEMM): two pieces; torch.autocast: one 16-bit piece per operand (1: bf16,
  // 2: fp16), whatever the caller's `exact`
  static GemmNtForm nt_form(const GemmLd& ld, bool exact, bool gelu = false) {
    if (ld.aff) return GemmNtForm{2, false, gelu};
    return g_train_amp ? GemmNtForm{1, g_train_amp == 2, gelu} : GemmNtForm{exact ? 3 : 2, false, gelu};
  }
  // The argument checks of nt(), wgrad_partials() and tn_direct(): they run before anything touches the device (axvs_test_train_gemm
  // calls them ahead of init(), so a refused call needs no GPU).
  static int check_nt(int N, int K, const GemmLd& ld, const GemmEpi& e, bool exact, bool gelu = false) {
    return gemm_nt_check(N, K, ld, e, nt_form(ld, exact, gelu));
  }
  // (the weight-gradient kernel always runs its 16-byte loader: both row strides must keep every row 16-byte aligned)
  static int check_wgrad(int N, int K, long long ldy, long long ldx) {
    if (N % 8 || K % 8 || ldy % 4 || ldx % 4)
      return fail(AXVS_ERR_ARG, "training GEMM: N=%d and K=%d must be multiples of 8, the row strides ldy=%lld and ldx=%lld multiples of 4", N, K,
                  ldy, ldx);
    return AXVS_OK;
  }
  static int check_tn(int N, long long lda, bool stat, int grp_rows) {
    if (N % 4 || lda % 4) return fail(AXVS_ERR_ARG, "einsum GEMM: N=%d must be a multiple of 4", N);
    if (grp_rows > 0 && stat) return fail(AXVS_ERR_ARG, "einsum GEMM: grouped output rows take no statistics");
    return AXVS_OK;
  }
  template <bool GEN, int AMP = 0, bool STATS = false, bool GRP = false>
  int launch_tn(dim3 grid, const float* dY, const float* X, float* part, long long M, int N, int K, long long chunk, float* part_b,
                const GemmLd& ld) const {
    static thread_local int lds_dev = kNoDevice;
    if (int rc = raise_lds(reinterpret_cast<const void*>(tr_gemm_tn_kernel<GEN, AMP, STATS, GRP>), lds_dev)) return rc;
    t_gemm_variant = 0x200 | GEN | AMP << 1 | STATS << 3 | GRP << 4;
    hipLaunchKernelGGL((tr_gemm_tn_kernel<GEN, AMP, STATS, GRP>), grid, dim3(512), kGemmLds, st, dY, X, part, M, N, K, chunk, part_b, ld);
    return AXVS_OK;
  }
  // row-major:  Y[M,N] = beta Y + epilogue(X[M,K] W[N,K]^T); epilogue (optional): + bias, * mul, ReLU, dropout by element index
  // exact: three bf16 pieces per operand (fp32 accuracy) -- for the GEMM in front of the ReLU (see tr_gemm_nt_kernel)
  // ld (optional): row strides of X, W, Y (sub-matrices of wider buffers); ld.ksteps > 0 with zsplits: split-K partials [z][M][ld.c]
  // gelu: the instantiation whose epilogue takes e.relu = 2 / 3 (GemmNtForm)
  int nt(const float* X, const float* W, float* Y, long long M, int N, int K, GemmLd ld, const GemmEpi& e, bool exact, int zsplits = 1,
         bool gelu = false) const {
    return gemm_nt(X, W, Y, M, N, K, ld, e, nt_form(ld, exact, gelu), zsplits, st, dev, &t_gemm_variant);
  }
  // X2 (nullable): added to X element-wise in the loader (q = k = Linear(x + pos) without an x + pos buffer)
  int fwd(const float* X, const float* W, float* Y, long long M, int N, int K, float beta = 0.f, const GemmEpi* ep = nullptr,
          bool exact = false, const float* X2 = nullptr, bool gelu = false) const {
    GemmEpi e = ep ? *ep : GemmEpi{nullptr, 1.f, 0, Drop{0u, 0u, 0u, 1.f}, 0.f};
    e.beta = beta;
    return nt(X, W, Y, M, N, K, GemmLd{K, K, N, 0, X2}, e, exact, 1, gelu);
  }
  // dW[N,K] = dY[M,N]^T X[M,K]: the reduction runs over the M rows and the output is small, so the rows are split kSplit ways
  // into `part` ([kSplit + 1][N*K]); the caller sums the partials (deterministic).  ldy / ldx: row strides of dY / X (0: N / K).
  static constexpr int kSplit = 64;
  int wgrad_partials(const float* dY, const float* X, float* part, long long M, int N, int K, int* nparts, float* part_b = nullptr,
                     long long ldy = 0, long long ldx = 0) const {
    const GemmLd ld{ldy ? ldy : N, ldx ? ldx : K, K, 0};
    if (int rc = check_wgrad(N, K, ld.a, ld.b)) return rc;
    long long chunk = (M + kSplit - 1) / kSplit;
    chunk = (chunk + kGK - 1) / kGK * kGK;                 // whole k-steps per split
    const int np = (int)((M + chunk - 1) / chunk);
    const dim3 grid((unsigned)(((N + kGT - 1) / kGT) * ((K + kGT - 1) / kGT)), (unsigned)np);
    *nparts = np;
    if (g_train_amp == 1) return launch_tn<false, 1>(grid, dY, X, part, M, N, K, chunk, part_b, ld);
    if (g_train_amp == 2) return launch_tn<false, 2>(grid, dY, X, part, M, N, K, chunk, part_b, ld);
    return launch_tn<false>(grid, dY, X, part, M, N, K, chunk, part_b, ld);
  }
  // P[N][K] (row stride ldo) = A[Mc][N]^T X[Mc][K]: the contraction over a FEW rows Mc (the 128 channels of the mask einsum,
  // CC:55) in one split, straight into the caller's tensor
  // al_x / al_o: alignment (floats) of the rows of X and P -- K is a pixel count and need not be a multiple of anything
  // stat (nullable): GemmLd with the stat_* fields set -- the tile sums of P for the BatchNorm behind the einsum (STATS instantiation)
  // grp_rows > 0: output row n at P + (n / grp_rows) grp_ld + (n % grp_rows) ldo (GemmLd::c_grp_rows)
  int tn_direct(const float* A, const float* X, float* P, int Mc, int N, int K, long long lda, long long ldx, long long ldo, int al_x, int al_o,
                const GemmLd* stat = nullptr, int grp_rows = 0, long long grp_ld = 0) const {
    if (int rc = check_tn(N, lda, stat != nullptr, grp_rows)) return rc;
    const dim3 grid((unsigned)(((N + kGT - 1) / kGT) * ((K + kGT - 1) / kGT)), 1u);
    const long long chunk = (Mc + kGK - 1) / kGK * kGK;
    GemmLd ld{lda, ldx, ldo, 0};
    ld.al_b = al_x;
    ld.al_c = al_o;
    ld.c_grp_rows = grp_rows;
    ld.c_grp_ld = grp_ld;
    const bool gen = !(al_x == 4 && al_o == 4 && K % 4 == 0);
    if (grp_rows > 0)
      return gen ? launch_tn<true, 0, false, true>(grid, A, X, P, Mc, N, K, chunk, nullptr, ld) : launch_tn<false, 0, false, true>(grid, A, X, P, Mc, N, K, chunk, nullptr, ld);
    if (stat) {
      ld.stat_part = stat->stat_part; ld.stat_shift = stat->stat_shift; ld.stat_nblk = stat->stat_nblk; ld.stat_blk0 = stat->stat_blk0;
      ld.stat_rows = stat->stat_rows;
      return gen ? launch_tn<true, 0, true>(grid, A, X, P, Mc, N, K, chunk, nullptr, ld) : launch_tn<false, 0, true>(grid, A, X, P, Mc, N, K, chunk, nullptr, ld);
    }
    return gen ? launch_tn<true>(grid, A, X, P, Mc, N, K, chunk, nullptr, ld) : launch_tn<false>(grid, A, X, P, Mc, N, K, chunk, nullptr, ld);
  }
};

// ---- shapes and buffers ----------------------------------------------------------------------------------------------------
struct Dims {
  int B, T, H, W, C, heads, F, D;
  long long M, HW;
};

int make_dims_any(Dims& d, int B, int T, int H, int W, int C, int heads, int F) {
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || C <= 0 || heads <= 0 || F <= 0) return fail(AXVS_ERR_ARG, "non-positive dimension");
  if (C % heads) return fail(AXVS_ERR_ARG, "C=%d must be a multiple of heads=%d", C, heads);
  const int D = C / heads;
  if (D != 8 && D != 16 && D != 32 && D != 64) return fail(AXVS_ERR_ARG, "training tier: head_dim=%d not built (8, 16, 32, 64)", D);
  if (F % 8) return fail(AXVS_ERR_ARG, "training tier: d_ffn=%d must be a multiple of 8", F);
  if (T > 16) return fail(AXVS_ERR_ARG, "training tier: T=%d > 16 frames per clip not built", T);
  const long long M = (long long)B * T * H * W;
  if (M * (long long)(T > 1 ? T : 1) > INT32_MAX) return fail(AXVS_ERR_ARG, "training tier: B*T*H*W*T exceeds 2^31 rows");
  d = Dims{B, T, H, W, C, heads, F, D, M, (long long)H * W};
  return AXVS_OK;
}

// the axial layer: frames are axis lengths (H or W keys)
int make_dims(Dims& d, int B, int T, int H, int W, int C, int heads, int F) {
  if (int rc = make_dims_any(d, B, T, H, W, C, heads, F)) return rc;
  if ((size_t)2 * (H > W ? H : W) * d.D * sizeof(float) > 160 * 1024) return fail(AXVS_ERR_ARG, "training tier: axis length too long for LDS");
  return AXVS_OK;
}

// The kernel family of the spatial half, decided here and nowhere else (the backward reads the statistics the forward leaves, so
// both ask this function).  head_dim 32: the MFMA kernels -- a frame's K and V resident in LDS (Split: the 16-bit split-precision
// forward for frames of at most 128 keys, unless g_train_attn_split is 0; Mfma: fp32 operands; the two share the backward), or, beyond the
// ~550 keys LDS holds, Chunk: keys staged kSpChunk at a time.  Any other head_dim, or option train_valu: the VALU kernels.
enum class SpatialTier { Valu, Split, Mfma, Chunk };
constexpr size_t kMaxLds = 160 * 1024;

SpatialTier spatial_tier(const Dims& d, const RowMap& rm) {
  if (d.D != 32 || g_train_valu) return SpatialTier::Valu;
  if (spatial_frame_lds(rm.L) > kMaxLds) return SpatialTier::Chunk;
  return g_train_attn_split && rm.L <= 16 * kSpMaxTiles ? SpatialTier::Split : SpatialTier::Mfma;
}
// dynamic LDS of the VALU query-side kernels: K | V of a frame, [L][D] each
inline size_t spatial_valu_lds(const Dims& d, const RowMap& rm) { return (size_t)2 * rm.L * d.D * sizeof(float); }

// Frame length the spatial half's kernels take: the MFMA kernels any, the VALU kernels what LDS holds.
int check_frame(const Dims& d, const RowMap& rm) {
  if (spatial_tier(d, rm) != SpatialTier::Valu || spatial_valu_lds(d, rm) <= kMaxLds) return AXVS_OK;
  return fail(AXVS_ERR_ARG, "training tier: head_dim=%d with frames of %d keys: the VALU attention kernel holds a frame in LDS, at most %lld keys "
              "(frames of any length need head_dim 32)", d.D, rm.L, (long long)(kMaxLds / (2 * d.D * sizeof(float))));
}

// the full T*H*W layer: one frame is all HW tokens of an image
inline RowMap traj_rowmap(const Dims& d) { return RowMap{d.T * (int)d.HW, (int)d.HW, 1, (long long)d.T * d.HW, d.HW, 1, 0}; }
int make_traj_dims(Dims& d, int B, int T, int HW, int C, int heads, int F) {
  if (int rc = make_dims_any(d, B, T, 1, HW, C, heads, F)) return rc;
  return check_frame(d, traj_rowmap(d));
}

struct PassSaved {
  float *q, *k, *v, *x, *xd, *q2, *kv2, *o;
  float* st;   // softmax statistics of the spatial half [(s heads + h), N, T, 3]: max, 1 / sum (forward), D (backward part 1)
};
struct Saved {
  PassSaved p[2];
  float *buf1, *buf2, *mean1, *rstd1, *z, *r, *u, *mean2, *rstd2;
};

PassSaved carve_pass(Carver& b, const Dims& d) {
  PassSaved p{};
  const size_t MC = (size_t)d.M * d.C;
  p.q = b.f(MC);
  p.k = b.f(MC);
  p.v = b.f(MC);
  p.x = b.f(MC * d.T);
  p.xd = b.f(MC);
  p.q2 = b.f(MC);
  p.kv2 = b.f(MC * d.T * 2);
  p.o = b.f(MC);
  p.st = b.f((size_t)d.M * d.heads * d.T * 3);
  return p;
}

// npass: 2 (axial layer: height and width pass, buf1 between them) or 1 (full layer: its pass writes buf2)
Saved carve_saved(Carver& b, const Dims& d, int npass = 2) {
  Saved s{};
  const size_t MC = (size_t)d.M * d.C;
  for (int i = 0; i < npass; ++i) s.p[i] = carve_pass(b, d);
  if (npass == 2) s.buf1 = b.f(MC);
  s.buf2 = b.f(MC);
  s.mean1 = b.f(d.M);
  s.rstd1 = b.f(d.M);
  s.z = b.f(MC);
  s.r = b.f((size_t)d.M * d.F);
  s.u = b.f(MC);
  s.mean2 = b.f(d.M);
  s.rstd2 = b.f(d.M);
  return s;
}

constexpr int kColsumBlocks = 512;

struct Scratch {
  float *a, *t0, *d_o, *dq2, *dkv2, *dx, *dxd, *dq, *dk, *dv, *da, *g0, *g1, *dr, *part_a, *part_b, *wpart, *wt;
};

Scratch carve_scratch(Carver& b, const Dims& d, bool backward) {
  Scratch s{};
  const size_t MC = (size_t)d.M * d.C;
  s.a = b.f(MC);
  s.t0 = b.f(MC);
  if (!backward) return s;
  s.d_o = b.f(MC);
  s.dq2 = b.f(MC);
  s.dkv2 = b.f(MC * d.T * 2);
  s.dx = b.f(MC * d.T);
  s.dxd = b.f(MC);
  s.dq = b.f(MC);
  s.dk = b.f(MC);
  s.dv = b.f(MC);
  s.da = b.f(MC);
  s.g0 = b.f(MC);
  s.g1 = b.f(MC);
  s.dr = b.f((size_t)d.M * d.F);
  const size_t wide = (size_t)(2 * d.C > d.F ? 2 * d.C : d.F);
  s.part_a = b.f(kColsumBlocks * wide);
  s.part_b = b.f(kColsumBlocks * wide);
  const size_t wmax = (size_t)d.C * (2 * d.C > d.F ? 2 * d.C : d.F);     // largest weight: proj_kv [2C, C] or linear1/2 [F, C]
  s.wpart = b.f((Gemm::kSplit + 1) * wmax);
  s.wt = b.f(wmax);
  return s;
}

Drop make_drop(float p, unsigned seed, unsigned site) {
  Drop d{seed, site, 0u, 1.f};
  if (p > 0.f) {
    d.thr = (unsigned)((double)p * 16777216.0);
    d.scale = 1.f / (1.f - p);
  }
  return d;
}

inline unsigned blocks(size_t n, unsigned per = 256) { return (unsigned)((n + per - 1) / per); }

#define AXVS_D_SWITCH(D_, ...)                       \
  switch (D_) {                                      \
    case 8: { constexpr int kD = 8; __VA_ARGS__; } break;   \
    case 16: { constexpr int kD = 16; __VA_ARGS__; } break; \
    case 64: { constexpr int kD = 64; __VA_ARGS__; } break; \
    default: { constexpr int kD = 32; __VA_ARGS__; } break; \
  }

struct Ctx {
  Dims d;
  Gemm g;
  hipStream_t st;
  float scale;
  Scratch sc;

  void add(const float* a, const float* b, float* y, size_t n) const {
    hipLaunchKernelGGL(tr_add_kernel, dim3(blocks(n / 4)), dim3(256), 0, st, a, b, y, n / 4);
  }
  void bias_act(float* y, const float* bias, long long rows, int N, float mul, int relu, Drop dr) const {
    hipLaunchKernelGGL(tr_bias_act_kernel, dim3(blocks((size_t)rows * N / 4)), dim3(256), 0, st, y, bias, rows, N, mul, relu, dr);
  }
  // bias / LayerNorm parameter gradients: out_a[c] = sum_r dy[r][c]; with x: out_b[c] = sum_r dy[r][c] xhat[r][c]
  void colsum(const float* dy, long long rows, int N, float* out_a, const float* x = nullptr, const float* mean = nullptr,
              const float* rstd = nullptr, float* out_b = nullptr) const {
    long long rpb = (rows + kColsumBlocks - 1) / kColsumBlocks;
    if (rpb < 64) rpb = 64;
    const int nblk = (int)((rows + rpb - 1) / rpb);
    hipLaunchKernelGGL(tr_colsum_kernel, dim3(nblk), dim3(256), 0, st, dy, x, mean, rstd, sc.part_a, sc.part_b, rows, N, (int)rpb);
    hipLaunchKernelGGL(tr_colsum_final_kernel, dim3(blocks(N, 256)), dim3(256), 0, st, (const float*)sc.part_a, nblk, (size_t)N, out_a);
    if (x) hipLaunchKernelGGL(tr_colsum_final_kernel, dim3(blocks(N, 256)), dim3(256), 0, st, (const float*)sc.part_b, nblk, (size_t)N, out_b);
  }
  // dW[N,K] = dY[M,N]^T X[M,K]; db (nullable) [N] = column sums of dY -- the bias gradient rides in the same GEMM launch
  // mul: the gradients are those of mul * dY (a scale that sits between the Linear layer and the tensor dY belongs to)
  int wgrad(const float* dY, const float* X, float* dW, long long M, int N, int K, float* db = nullptr, long long ldy = 0,
            long long ldx = 0, float mul = 1.f) const {
    int np = 0;
    int rc = g.wgrad_partials(dY, X, sc.wpart, M, N, K, &np, db ? sc.part_a : nullptr, ldy, ldx);
    if (rc != AXVS_OK) return rc;
    const size_t n = (size_t)N * K;
    if (db) {      // one launch adds the partials of the weight and of the bias gradient (same order of additions as the single kernel)
      const unsigned ba = blocks(n, 256), bb = blocks(N, 256);
      hipLaunchKernelGGL(tr_colsum_final_pair_kernel, dim3(ba + bb), dim3(256), 0, st, (const float*)sc.wpart, n, dW, (const float*)sc.part_a, (size_t)N, db,
                         np, (int)ba, mul);
    } else {
      hipLaunchKernelGGL(tr_colsum_final_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, (const float*)sc.wpart, np, n, dW, mul);
    }
    return AXVS_OK;
  }
  // dX[M,K] = beta dX + dY[M,N] W[N,K]      (through W^T, in the forward GEMM's form)
  // exact: three-piece operands (see axvs_train_gemm.h) -- where the result feeds a sum that cancels analytically
  // mul: dX = mul * dY W; res / res2 (nullable, [M][K]): added in the epilogue
  int dgrad(const float* dY, const float* W, float* dX, long long M, int N, int K, float beta, long long ldy = 0, bool exact = false,
            float mul = 1.f, const float* res = nullptr, const float* res2 = nullptr) const {
    const GemmLd ld{ldy ? ldy : N, N, K, 0};
    GemmEpi e{nullptr, mul, 0, Drop{0u, 0u, 0u, 1.f}, beta};
    e.res = res;
    e.res2 = res2;
    exact = exact || g_train_exact >= 2;
    if (int rc = Gemm::check_nt(K, N, ld, e, exact)) return rc;      // (before the transpose: a refused call launches nothing)
    hipLaunchKernelGGL(tr_transpose_kernel, dim3((K + 31) / 32, (N + 31) / 32), dim3(256), 0, st, W, sc.wt, N, K);
    return g.nt(dY, sc.wt, dX, M, K, N, ld, e, exact);
  }
  // launch 256-thread workgroups with `lds` bytes of dynamic LDS, raising the kernel's limit first where that is above the 64 KiB default
  template <class... P, class... A>
  int launch_lds(void (*kern)(P...), dim3 grid, size_t lds, A... args) const {
    if (lds > 64 * 1024)
      if (int rc = ensure_max_lds(reinterpret_cast<const void*>(kern))) return rc;
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, args...);
    return AXVS_OK;
  }
};

// queries the key-side backward kernel stages at a time: all of a sequence when they fit in LDS (the within-clip layer: <= 512),
// else chunks of 512 (the cross-clip module over 12 clips of 128 queries)
int spatial_kv_chunk(const RowMap& rm) {
  const int Np = (rm.N + 15) / 16 * 16;
  return Np <= 512 ? Np : 512;
}
// grid of the chunked kernels: y counts blocks of 4 * kSpQT query tiles
inline int chunk_tiles(const RowMap& rm) { return (((rm.N + 15) / 16 + 4 * kSpQT - 1) / (4 * kSpQT)) * 4; }

// Launch grid of the fp32 MFMA spatial-attention kernels: x = (sequence, head); the 16-row tiles each wave walks (y) and the frames (z)
// are spread over more workgroups until there are about g_spatial_wgs of them -- every (tile, frame) is computed by exactly one
// wave with the same instructions whatever the split.
dim3 spatial_grid(int sh, int tiles, int frames) {
  const int target = g_spatial_wgs;                  // workgroups wanted
  if (sh >= target) return dim3(sh, 1, 1);
  const int z = frames;
  int y = (target + sh * z - 1) / (sh * z);
  const int ymax = (tiles + 3) / 4;
  y = y > ymax ? ymax : (y < 1 ? 1 : y);
  return dim3(sh, y, z);
}

// the spatial half, forward (WC/temporal_attention.py:47-58): s.q, s.k, s.v -> s.x, and on the MFMA tiers (max, 1 / sum) -> s.st
int spatial_fwd(const Ctx& c, const PassSaved& s, const RowMap& rm, int S, Drop attn_drop) {
  const Dims& d = c.d;
  const int sh = S * d.heads, nqt = (rm.N + 15) / 16;
  switch (spatial_tier(d, rm)) {
    case SpatialTier::Split:      // 16-bit matrix cores, three-piece operands, a frame's scores in registers
      return c.launch_lds(tr_spatial_fwd_split_kernel, spatial_grid(sh, nqt, d.T), spatial_split_lds(rm.L), s.q, s.k, s.v, s.x, s.st, rm, d.T, d.C,
                          d.heads, c.scale, attn_drop);
    case SpatialTier::Mfma:       // fp32 MFMA, the frame in LDS
      return c.launch_lds(tr_spatial_fwd_mfma_kernel, spatial_grid(sh, nqt, d.T), spatial_frame_lds(rm.L), s.q, s.k, s.v, s.x, s.st, rm, d.T, d.C,
                          d.heads, c.scale, attn_drop);
    case SpatialTier::Chunk:      // long frames: keys chunked through LDS
      return c.launch_lds(tr_spatial_fwd_chunk_kernel, spatial_grid(sh, chunk_tiles(rm), d.T), spatial_chunk_lds(), s.q, s.k, s.v, s.x, s.st, rm, d.T,
                          d.C, d.heads, c.scale, attn_drop);
    case SpatialTier::Valu:
      break;
  }
  if (int rc = check_frame(d, rm)) return rc;
  AXVS_D_SWITCH(d.D, return c.launch_lds(tr_spatial_fwd_kernel<kD>, dim3(sh), spatial_valu_lds(d, rm), s.q, s.k, s.v, s.x, rm, d.T, d.C, d.heads,
                                         c.scale, attn_drop))
  return AXVS_OK;
}

// the spatial half, backward: c.sc.dx (gradient of s.x) -> c.sc.dq, dk, dv; D -> s.st[.., 2].  Split and Mfma share their backward.
int spatial_bwd(const Ctx& c, const PassSaved& s, const RowMap& rm, int S, Drop attn_drop) {
  const Dims& d = c.d;
  const Scratch& sc = c.sc;
  const int sh = S * d.heads, nqt = (rm.N + 15) / 16, T = d.T;
  int rc;
  switch (spatial_tier(d, rm)) {
    case SpatialTier::Valu: {
      if ((rc = check_frame(d, rm)) != AXVS_OK) return rc;
      constexpr int QC = 32;      // queries the key-side kernel stages at a time: scaled q, dx of all T frames, statistics
      const size_t lds_kv = (size_t)(QC * d.D + QC * T * d.D + QC * T * 3) * sizeof(float);
      AXVS_D_SWITCH(d.D, {
        if ((rc = c.launch_lds(tr_spatial_bwd_q_kernel<kD>, dim3(sh), spatial_valu_lds(d, rm), s.q, s.k, s.v, sc.dx, sc.dq, s.st, rm, T, d.C, d.heads,
                               c.scale, attn_drop)) != AXVS_OK)
          return rc;
        return c.launch_lds(tr_spatial_bwd_kv_kernel<kD>, dim3(sh), lds_kv, s.q, s.k, s.v, sc.dx, s.st, sc.dk, sc.dv, rm, T, d.C, d.heads, c.scale,
                            attn_drop, QC);
      })
      return AXVS_OK;
    }
    case SpatialTier::Chunk:
      rc = c.launch_lds(tr_spatial_bwd_q_chunk_kernel, spatial_grid(sh, chunk_tiles(rm), 1), spatial_chunk_lds(), s.q, s.k, s.v, s.x, sc.dx, sc.dq, s.st,
                        rm, T, d.C, d.heads, c.scale, attn_drop);
      break;
    case SpatialTier::Split:
    case SpatialTier::Mfma:
      rc = c.launch_lds(tr_spatial_bwd_q_mfma_kernel, spatial_grid(sh, nqt, 1), spatial_frame_lds(rm.L), s.q, s.k, s.v, s.x, sc.dx, sc.dq, s.st, rm, T,
                        d.C, d.heads, c.scale, attn_drop);
      break;
  }
  if (rc != AXVS_OK) return rc;
  const int Nc = spatial_kv_chunk(rm);      // the key side never holds a whole frame: one kernel behind both query-side kernels
  return c.launch_lds(tr_spatial_bwd_kv_mfma_kernel, spatial_grid(sh, (rm.L + 15) / 16, T), spatial_kv_lds(Nc), s.q, s.k, s.v, sc.dx, s.st, sc.dk, sc.dv,
                      rm, T, d.C, d.heads, c.scale, attn_drop, Nc);
}

// one axial pass, forward: xout = xin + dropout1(TrajectoryAttention(q = k = xin + pos, v = xin))   WC/temporal_attention.py:35-76
int pass_fwd(const Ctx& c, const float* xin, const float* pos, float* xout, const AxvsTrajParams& w, const PassSaved& s, RowMap rm, int S,
             Drop attn_drop, Drop drop1) {
  const Dims& d = c.d;
  const long long M = d.M;
  const int C = d.C;
  const Drop none = make_drop(0.f, 0, 0);
  int rc;
  // q = k = Linear(x + pos): the sum is formed in the GEMM's A loader (the cross-clip layer has no positional term, CC:96)
  // (the biases ride in the GEMM epilogues; `ex`: option train_exact -- forward products with fp32 accuracy)
  const bool ex = g_train_exact != 0;
  const GemmEpi eq{w.q_b, 1.f, 0, none, 0.f}, ek{w.k_b, 1.f, 0, none, 0.f}, ev{w.v_b, 1.f, 0, none, 0.f};
  if ((rc = c.g.fwd(xin, w.q_w, s.q, M, C, C, 0.f, &eq, ex, pos)) != AXVS_OK) return rc;
  if ((rc = c.g.fwd(xin, w.k_w, s.k, M, C, C, 0.f, &ek, ex, pos)) != AXVS_OK) return rc;
  if ((rc = c.g.fwd(xin, w.v_w, s.v, M, C, C, 0.f, &ev, ex)) != AXVS_OK) return rc;
  if ((rc = spatial_fwd(c, s, rm, S, attn_drop)) != AXVS_OK) return rc;
  hipLaunchKernelGGL(tr_diag_gather_kernel, dim3(blocks((size_t)M * C / 4)), dim3(256), 0, c.st, (const float*)s.x, s.xd, M, d.T, d.HW, C);
  const GemmEpi epq{w.proj_q_b, c.scale, 0, none, 0.f}, epkv{w.proj_kv_b, 1.f, 0, none, 0.f};
  if ((rc = c.g.fwd(s.xd, w.proj_q_w, s.q2, M, C, C, 0.f, &epq, ex)) != AXVS_OK) return rc;
  if ((rc = c.g.fwd(s.x, w.proj_kv_w, s.kv2, M * d.T, 2 * C, C, 0.f, &epkv, ex)) != AXVS_OK) return rc;
  AXVS_D_SWITCH(d.D, {
    if (d.T <= 8) hipLaunchKernelGGL((tr_temporal_fwd_kernel<kD, 8>), dim3(blocks((size_t)M * d.heads)), dim3(256), 0, c.st, (const float*)s.q2,
                                     (const float*)s.kv2, s.o, M, d.T, C, d.heads);
    else hipLaunchKernelGGL((tr_temporal_fwd_kernel<kD, 16>), dim3(blocks((size_t)M * d.heads)), dim3(256), 0, c.st, (const float*)s.q2,
                            (const float*)s.kv2, s.o, M, d.T, C, d.heads);
  })
  if ((rc = c.g.fwd(s.o, w.proj_w, c.sc.t0, M, C, C, 0.f, nullptr, ex)) != AXVS_OK) return rc;
  hipLaunchKernelGGL(tr_bias_drop_res_kernel, dim3(blocks((size_t)M * C / 4)), dim3(256), 0, c.st, (const float*)c.sc.t0, w.proj_b, xin, xout, rm,
                     M, C, drop1);
  return AXVS_OK;
}

// backward of one axial pass.  d_out: gradient of the pass output; d_in: gradient of the pass input (written); d_pos: nullable,
// written when `pos_first`, accumulated otherwise.
int pass_bwd(const Ctx& c, const float* d_out, const float* xin, const float* pos, const AxvsTrajParams& w, const AxvsTrajGrads& gw,
             const PassSaved& s, RowMap rm, int S, Drop attn_drop, Drop drop1, float* d_in, float* d_pos, bool pos_first) {
  const Dims& d = c.d;
  const long long M = d.M;
  const int C = d.C, T = d.T;
  const Scratch& sc = c.sc;
  const size_t MC = (size_t)M * C;
  int rc;
  // proj and dropout1
  hipLaunchKernelGGL(tr_drop_bwd_kernel, dim3(blocks(MC / 4)), dim3(256), 0, c.st, d_out, sc.t0, rm, M, C, drop1);
  if ((rc = c.wgrad(sc.t0, s.o, gw.proj_w, M, C, C, gw.proj_b)) != AXVS_OK) return rc;
  if ((rc = c.dgrad(sc.t0, w.proj_w, sc.d_o, M, C, C, 0.f)) != AXVS_OK) return rc;
  // temporal half
  AXVS_D_SWITCH(d.D, {
    if (T <= 8) hipLaunchKernelGGL((tr_temporal_bwd_kernel<kD, 8>), dim3(blocks((size_t)M * d.heads)), dim3(256), 0, c.st, (const float*)s.q2,
                                   (const float*)s.kv2, (const float*)sc.d_o, sc.dq2, sc.dkv2, M, T, C, d.heads);
    else hipLaunchKernelGGL((tr_temporal_bwd_kernel<kD, 16>), dim3(blocks((size_t)M * d.heads)), dim3(256), 0, c.st, (const float*)s.q2,
                            (const float*)s.kv2, (const float*)sc.d_o, sc.dq2, sc.dkv2, M, T, C, d.heads);
  })
  if ((rc = c.wgrad(sc.dkv2, s.x, gw.proj_kv_w, M * T, 2 * C, C, gw.proj_kv_b)) != AXVS_OK) return rc;
  if ((rc = c.dgrad(sc.dkv2, w.proj_kv_w, sc.dx, M * T, 2 * C, C, 0.f)) != AXVS_OK) return rc;
  // q2 = scale (proj_q(xd)): the scale rides in the two GEMMs' epilogues
  if ((rc = c.wgrad(sc.dq2, s.xd, gw.proj_q_w, M, C, C, gw.proj_q_b, 0, 0, c.scale)) != AXVS_OK) return rc;
  if ((rc = c.dgrad(sc.dq2, w.proj_q_w, sc.dxd, M, C, C, 0.f, 0, false, c.scale)) != AXVS_OK) return rc;
  hipLaunchKernelGGL(tr_diag_scatter_add_kernel, dim3(blocks(MC / 4)), dim3(256), 0, c.st, sc.dx, (const float*)sc.dxd, M, T, d.HW, C);
  if ((rc = spatial_bwd(c, s, rm, S, attn_drop)) != AXVS_OK) return rc;
  // q / k / v projections
  const float* const xa = pos ? sc.a : xin;
  if (pos) c.add(xin, pos, sc.a, MC);
  if ((rc = c.wgrad(sc.dq, xa, gw.q_w, M, C, C, gw.q_b)) != AXVS_OK) return rc;
  if ((rc = c.wgrad(sc.dk, xa, gw.k_w, M, C, C, gw.k_b)) != AXVS_OK) return rc;
  if ((rc = c.wgrad(sc.dv, xin, gw.v_w, M, C, C, gw.v_b)) != AXVS_OK) return rc;
  if ((rc = c.dgrad(sc.dq, w.q_w, sc.da, M, C, C, 0.f)) != AXVS_OK) return rc;
  if ((rc = c.dgrad(sc.dk, w.k_w, sc.da, M, C, C, 1.f)) != AXVS_OK) return rc;
  // d_in = d_out (residual) + dv Wv + da;   d_pos (+)= da
  if ((rc = c.dgrad(sc.dv, w.v_w, d_in, M, C, C, 0.f, 0, false, 1.f, d_out, sc.da)) != AXVS_OK) return rc;
  if (d_pos) {
    if (pos_first) {
      if (hipMemcpyAsync(d_pos, sc.da, MC * sizeof(float), hipMemcpyDeviceToDevice, c.st) != hipSuccess) return fail(AXVS_ERR_LAUNCH, "hipMemcpyAsync failed");
    } else {
      c.add(d_pos, sc.da, d_pos, MC);
    }
  }
  return AXVS_OK;
}

// every field of a parameter / gradient struct (pointers only) is non-null
template <class P>
int check_ptrs(const P* p, const char* what) {
  const void* const* f = reinterpret_cast<const void* const*>(p);
  for (size_t i = 0; i < sizeof(P) / sizeof(void*); ++i)
    if (!f[i]) return fail(AXVS_ERR_ARG, "null pointer (field %zu of %s)", i, what);
  return AXVS_OK;
}

inline int check_drop(float p_dropout, float p_attn_drop) {
  if (!(p_dropout >= 0.f && p_dropout < 1.f) || !(p_attn_drop >= 0.f && p_attn_drop < 1.f)) return fail(AXVS_ERR_ARG, "dropout probability outside [0, 1)");
  return AXVS_OK;
}

// The end of every training entry point's setup, once its buffers are carved: what was carved against what the caller brought (before
// anything touches the device), the stream, the GEMM launcher.
inline int train_begin(Ctx& c, const Carver& saved, size_t saved_bytes, const Carver& scratch, size_t scratch_bytes, void* stream) {
  if (saved.off > saved_bytes || scratch.off > scratch_bytes)
    return fail(AXVS_ERR_WORKSPACE, "training buffers too small: saved %zu < %zu or scratch %zu < %zu", saved_bytes, saved.off, scratch_bytes, scratch.off);
  c.st = static_cast<hipStream_t>(stream);
  return c.g.init(c.st);
}

}  // namespace
}  // namespace axvs
