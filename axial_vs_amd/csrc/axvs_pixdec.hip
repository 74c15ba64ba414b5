// C-ABI entry points of the pixel-decoder family (include/axvs.h: axvs_msda_*, axvs_conv1x1_gn_*, axvs_fpn_level_*, axvs_pos2d,
// axvs_scaled_residual, axvs_ffn_pack / axvs_ffn_packed_fwd) and the launch sequences behind them.  The FFN of a deformable encoder
// layer is the axial unit's (axvs_infer.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "axvs_infer.h"
#include "axvs_msda.h"
#include "axvs_glue.h"
#include "axvs_fpn.h"
#include "axvs_gemm_nt.h"

using namespace axvs;

namespace {

// Pieces of the 128 x 128 split-precision GEMM of axvs_gemm_nt.h, which runs the deformable attention's three projections when the
// level set has >= 2048 rows.  4 (rounds 3 - 4): two bf16 pieces for value_proj (its output is rounded to 16 bits anyway) and for the
// offset | weight projection, three pieces (fp32 accuracy) for output_proj, whose result enters the residual stream without a norm;
// 2 (since the end of round 5) / 3: two / three pieces everywhere; 0: the 64 x 64 kernels of axvs_gemm.h.
// (Two pieces put 5e-6 on a projection; the free-running 16-bit stack's max-norm at BASELINE config 3 is chaotic in its 16-bit roundings either way -- 1.29e-3 with 2,
//  1.38 - 1.48e-3 with 4, relative L2 5.7e-4 for both -- and 2 saves 2.5 % of the module: profiles/r5_planner_threshold.txt.)
constexpr int kMsdaGemm = 2;
constexpr int kConvNt128 = 192;          // token-row 1x1 projections run the 128 x 128 GEMM from this many tiles per launch on (0: never)
constexpr int kConvNt128Nchw = 128;      // the same for NCHW inputs (transposed to token rows first), tiles of the ONE launch over all frames
constexpr int kConvNt128Exact = 1;       // 0 = two bf16 pieces per operand (5e-6 of the float64 projection + GroupNorm on zero-mean operands, 114 against 147 us at
                                         // [32786 x 256 x 512]), 1 = three (9e-7).  Two pieces drop lo x lo, 2^-18 of EVERY product with the same sign where the operands have a DC
                                         // part: 1.4e-6 of a group's mean, i.e. 1.5e-4 of the normalised output at |mean| / std = 100 (tests/test_hip_groupnorm.py, drawn family)
constexpr int kConvNt128SplitK = 1024;   // split-K for the NCHW projections with few row tiles and Cin >= this (0: never)
constexpr bool kConvOnNt128 = kMsdaGemm != 0 && kConvNt128 != 0;      // the 1x1 projections may take the 128 x 128 kernel at all

// ---------------- multi-scale deformable attention ----------------
struct MsdaPacked {
  u16 *wv, *wq, *wo;            // value_proj [Cp,C] (head blocks), sampling_offsets|attention_weights [3MLP,C], output_proj [C,Cp]
  float *bv, *bq, *bo;
  float* wq32;                  // sampling_offsets | attention_weights as fp32 rows [3MLP][C]: operand of the 128 x 128 split-precision GEMM
  float *wv32, *wo32;           // value_proj / output_proj as fp32 rows [C][C] (head_dim 32: the head-block order is the natural one)
};
MsdaPacked carve_msda(Carver& c, int C, int heads, int L, int P) {
  const size_t Cp = (size_t)heads * 32, nq = (size_t)3 * heads * L * P;
  MsdaPacked m;
  m.wv = c.take<u16>(3 * Cp * C);          // split precision: (hi | lo | hi) along K
  m.wq = c.take<u16>(3 * ((nq + 15) & ~(size_t)15) * C);      // (weight rows are stored in groups of 16: wblk_off)
  m.wo = c.take<u16>(3 * (size_t)C * Cp);
  m.bv = c.take<float>(Cp);
  m.bq = c.take<float>(nq);
  m.bo = c.take<float>(C);
  m.wq32 = c.take<float>(nq * C);
  m.wv32 = c.take<float>((size_t)C * C);
  m.wo32 = c.take<float>((size_t)C * C);
  return m;
}

void pack_msda(int dtype, const AxvsMsdaParams& p, const MsdaPacked& m, int C, int heads, int L, int P, hipStream_t st) {
  const int d = C / heads, Cp = heads * 32, mlp = heads * L * P;
  PackDim plainC{C, C, 0, 0, 0}, headC{C, Cp, heads, d, 0}, off{2 * mlp, 2 * mlp, 0, 0, 0}, lg{mlp, mlp, 0, 0, 0};
  pack_w3(dtype, p.value_proj_w, m.wv, headC, plainC, st);
  pack_w3(dtype, p.sampling_offsets_w, m.wq, off, plainC, st, 0, 3 * mlp);
  pack_w3(dtype, p.attention_weights_w, m.wq, lg, plainC, st, 2 * mlp, 3 * mlp);
  pack_w3(dtype, p.output_proj_w, m.wo, plainC, headC, st);
  pack_b(p.value_proj_b, m.bv, headC, st);
  copy_f32(p.sampling_offsets_b, m.bq, 2 * mlp, st);
  copy_f32(p.attention_weights_b, m.bq + 2 * mlp, mlp, st);
  copy_f32(p.output_proj_b, m.bo, C, st);
  copy_f32(p.sampling_offsets_w, m.wq32, (size_t)2 * mlp * C, st);
  copy_f32(p.attention_weights_w, m.wq32 + (size_t)2 * mlp * C, (size_t)mlp * C, st);
  copy_f32(p.value_proj_w, m.wv32, (size_t)C * C, st);
  copy_f32(p.output_proj_w, m.wo32, (size_t)C * C, st);
}
int check_msda_pack(int L, int P) {
  if (L <= 0 || L > kMsdaMaxLevels || P <= 0 || L * P > 64) return fail(AXVS_ERR_ARG, "unsupported n_levels=%d / n_points=%d", L, P);
  return AXVS_OK;
}

struct MsdaWs {
  u16* value16;      // value_proj output, blocked 16-bit [N S][Cp]
  float* qproj;      // sampling offsets | attention logits [N Lq][msda_qld(heads, L, P)]
  u16* o16;          // sampled rows: two 16-bit pieces / the same bytes as fp32 rows
};
// row stride of qproj: 3 heads L P rounded up to the float4 groups the GEMM epilogue stores (a group that crossed the end of a row
// overwrote the first offsets of the next one when 3 heads L P was no multiple of 4)
inline int msda_qld(int heads, int L, int P) { return (3 * heads * L * P + 3) & ~3; }
MsdaWs carve_msda_ws(Carver& c, int N, int Lq, int S, int heads, int L, int P) {
  const size_t Cp = (size_t)heads * 32;
  MsdaWs w;
  w.value16 = c.take<u16>((size_t)N * S * Cp);
  w.qproj = c.take<float>((size_t)N * Lq * msda_qld(heads, L, P));
  w.o16 = c.take<u16>(2 * (size_t)N * Lq * Cp);
  return w;
}
struct MsdaLayerWs {
  void* mws;         // the self-attention's MsdaWs (msda_fwd_t carves it)
  FfnWs f;           // f.x = src + attention
};
MsdaLayerWs carve_msda_layer_ws(Carver& c, int N, int S, int C, int heads, int L, int P, int F) {
  MsdaLayerWs w;
  w.mws = c.take<char>(carved([&](Carver& m) { carve_msda_ws(m, N, S, S, heads, L, P); }));
  w.f = carve_ffn_ws(c, (long long)N * S, C, F);
  return w;
}

int msda_levels(const int* shapes, int L, int S, MsdaLevels* lv) {
  if (L <= 0 || L > kMsdaMaxLevels) return fail(AXVS_ERR_ARG, "n_levels=%d must be in 1..%d", L, kMsdaMaxLevels);
  long long start = 0;
  lv->L = L;
  for (int l = 0; l < L; ++l) {
    if (shapes[2 * l] <= 0 || shapes[2 * l + 1] <= 0) return fail(AXVS_ERR_ARG, "empty level %d", l);
    lv->H[l] = shapes[2 * l];
    lv->W[l] = shapes[2 * l + 1];
    lv->start[l] = (int)start;
    start += (long long)shapes[2 * l] * shapes[2 * l + 1];
  }
  if (start != S) return fail(AXVS_ERR_ARG, "spatial shapes cover %lld tokens, input has %d", start, S);   // modules/ms_deform_attn.py:96
  return AXVS_OK;
}
// the deformable attention's argument checks, in two halves (axvs_msda_layer_fwd has a check of its own between them)
int check_msda_points(int ref_dim, int L, int P) {
  if (ref_dim != 2 && ref_dim != 4) return fail(AXVS_ERR_ARG, "Last dim of reference_points must be 2 or 4, but get %d instead.", ref_dim);
  if (L * P > 64) return fail(AXVS_ERR_ARG, "n_levels * n_points > 64 is not supported");
  return AXVS_OK;
}
int check_msda_shapes(int N, int Lq, int S, const int* spatial_shapes, int L, MsdaLevels* lv) {
  if ((long long)N * S > 2147483647LL / 64 || (long long)N * Lq > 2147483647LL / 64) return fail(AXVS_ERR_ARG, "too many tokens for 32-bit row indices");
  return msda_levels(spatial_shapes, L, S, lv);
}

// Y[M][N] = epilogue(X[M][K] (+ X2) . W[N][K]^T) on the 128 x 128 split-precision kernel (axvs_gemm_nt.h), option msda_gemm = pieces
enum Nt128Use { kNt128Plain = 0, kNt128FeedsResidual = 1 /* three pieces under kMsdaGemm = 4 */, kNt128Fp32Grade = 2 /* three pieces whatever kMsdaGemm says */ };
int launch_nt128(const float* X, const float* X2, const float* W, float* Y, long long M, int N, int K, const tr::GemmEpi& e, hipStream_t st,
                 int use = kNt128Plain, long long lda = 0 /* row stride of X in floats (0: K) */,
                 int zsplit = 1 /* > 1: split-K -- workgroup z writes the partial product of its k-steps to Y + z M N (no epilogue terms) */) {
  tr::GemmLd ld{lda ? lda : K, K, N, 0, X2};
  if (zsplit > 1) ld.ksteps = ((K + tr::kGK - 1) / tr::kGK + zsplit - 1) / zsplit;
  const bool exact = kMsdaGemm == 3 || (kMsdaGemm == 4 && use == kNt128FeedsResidual) || use == kNt128Fp32Grade;
  return tr::gemm_nt(X, W, Y, M, N, K, ld, e, tr::GemmNtForm{exact ? 3 : 2}, zsplit > 1 ? zsplit : 1, st);
}
// NCHW x [N][K][HW] -> token rows `tok` (64 x 64 tiles through LDS), then Y = epilogue(tok . W^T) on the same kernel in ONE launch over all frames
int nchw_nt128(const float* x, float* tok, const float* W, float* Y, int N, int HW, int K, int Nout, const tr::GemmEpi& e, hipStream_t st,
               int use = kNt128Plain, int zsplit = 1) {
  nchw_to_rows(x, tok, N, K, HW, st);
  return launch_nt128(tok, nullptr, W, Y, (long long)N * HW, Nout, K, e, st, use, 0, zsplit);
}
// per-(frame, 64-row block) partial GroupNorm sums of fp32 rows y [N HW][C]: a thread owns 4 channels, 256 / (C / 4) row groups share a block
void launch_gn_stats(const float* y, float* partial, int N, int HW, int C, int groups, hipStream_t st) {
  const int n4 = C / 4, lanes = n4 < 256 ? n4 : 256, rg = 256 / lanes;
  hipLaunchKernelGGL(gn_stats_kernel, dim3((unsigned)((HW + 63) / 64), N), dim3(256), 2 * (size_t)rg * C * sizeof(float), st, y, partial, HW, C, groups);
}
// rows from which the 128 x 128 kernel beats the 64 x 64 one (fewer rows: too few workgroups)
inline bool use_nt128(long long rows, int C, int heads) { return kMsdaGemm && rows >= 2048 && C % 4 == 0 && C / heads == 32; }

// what: 0 = whole module (value_proj, offsets | logits, gather, output_proj), 1 = up to the gather with fp32 rows out
// (`out` = sampled [N*Lq][C], no output_proj)
template <bool BF>
int msda_fwd_t(const float* query, const float* refp, int ref_dim, const float* input, const unsigned char* mask, const MsdaLevels& lv,
               float* out, const MsdaPacked& p, int N, int Lq, int S, int C, int heads, int P, void* ws, hipStream_t st,
               const float* qadd = nullptr, const float* residual = nullptr, int what = 0) {
  const int L = lv.L, Cp = heads * 32, nq = 3 * heads * L * P, qld = msda_qld(heads, L, P);
  const long long Rv = (long long)N * S, Rq = (long long)N * Lq;
  Carver wc(ws);
  const MsdaWs w = carve_msda_ws(wc, N, Lq, S, heads, L, P);
  g_prof_next = 0;
  mark(st, "begin");
  // value_proj and output_proj feed the module output directly (no residual / norm inside the module): split precision
  const tr::Drop nodrop{0u, 0u, 0u, 1.f};
  if (use_nt128(Rv, C, heads)) {          // fp32 rows in, one 16-bit piece out in the blocked layout the gather reads
    tr::GemmEpi e{p.bv, 1.f, 0, nodrop, 0.f};
    e.out16 = w.value16;
    e.kind16 = BF ? 2 : 1;
    e.zero_rows = mask;
    if (int rc = launch_nt128(input, nullptr, p.wv32, nullptr, Rv, Cp, C, e, st)) return rc;
  } else {
    EpiBlocked16<BF> ev{w.value16, Rv, p.bv, 1.f, 0, 0};
    ev.zero_rows = mask;
    launch_gemm<BF>(ALoadRowsF32Split3<BF>{input, (int)Rv, C}, p.wv, ev, (int)Rv, Cp, 3 * C, st);
  }
  mark(st, "msda.value_proj");
  // sampling offsets | attention logits: fp32 rows in, fp32 rows out, [N Lq] x [3 heads L P] x C -- at a few thousand rows and more
  // the 128 x 128 split-precision kernel of the training tier (axvs_gemm_nt.h: fp32 operands split into bf16 pieces in its
  // loader) beats the 64 x 64 one (config 3, 21504 rows: the three projections of a deformable layer 27 + 59 + 30 us -> ~65 us)
  if (kMsdaGemm && Rq >= 2048 && C % 4 == 0 && nq % 4 == 0) {
    const tr::GemmEpi e{p.bq, 1.f, 0, nodrop, 0.f};
    if (int rc = launch_nt128(query, qadd, p.wq32, w.qproj, Rq, nq, C, e, st)) return rc;
  } else {
    launch_gemm<BF>(ALoadRowsF32Split3<BF>{query, (int)Rq, C, qadd}, p.wq, EpiRowsF32{w.qproj, nullptr, p.bq, identity_map(Rq), qld, 1.f}, (int)Rq,
                    nq, 3 * C, st);
  }
  mark(st, "msda.offsets+weights");
  const long long groups = Rq * heads;
  const dim3 ggrid((unsigned)((groups + 63) / 64));
  // the output projection on the 128 x 128 kernel reads the sampled rows as fp32 [N Lq][C] (same bytes as the two 16-bit pieces)
  const bool out128 = what != 1 && use_nt128(Rq, C, heads);
  float* of32 = what == 1 ? out : (out128 ? reinterpret_cast<float*>(w.o16) : nullptr);
  if (P == 4) hipLaunchKernelGGL((msda_gather_kernel<BF, 4>), ggrid, dim3(256), 0, st, w.value16, w.qproj, refp, ref_dim, lv, w.o16, N, S, Lq, heads, P, qld, of32, C / heads);
  else hipLaunchKernelGGL((msda_gather_kernel<BF, 0>), ggrid, dim3(256), 0, st, w.value16, w.qproj, refp, ref_dim, lv, w.o16, N, S, Lq, heads, P, qld, of32, C / heads);
  mark(st, "msda.gather");
  if (what == 1) return last_launch_status();
  if (out128) {
    tr::GemmEpi e{p.bo, 1.f, 0, nodrop, 0.f};
    e.res = residual;
    if (int rc = launch_nt128(of32, nullptr, p.wo32, out, Rq, C, C, e, st, kNt128FeedsResidual)) return rc;
  } else {
    launch_gemm<BF>(ALoadBlockedSplit3<BF>{w.o16, Rq, (int)Rq, Cp}, p.wo, EpiRowsF32{out, residual, p.bo, identity_map(Rq), C, 1.f}, (int)Rq,
                    C, 3 * Cp, st);
  }
  mark(st, "msda.output_proj");
  return last_launch_status();
}

}  // namespace

extern "C" {

size_t axvs_msda_packed_bytes(int C, int heads, int L, int P) { return carved([&](Carver& c) { carve_msda(c, C, heads, L, P); }); }

int axvs_msda_pack(const AxvsMsdaParams* p, void* packed, int C, int heads, int L, int P, int dtype, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!p || !packed) return fail(AXVS_ERR_ARG, "null pointer");
  if (int rc = check_cfg(C, heads)) return rc;
  if (int rc = check_msda_pack(L, P)) return rc;
  Carver c(packed);
  const MsdaPacked m = carve_msda(c, C, heads, L, P);
  pack_msda(dtype, *p, m, C, heads, L, P, static_cast<hipStream_t>(stream));
  return last_launch_status();
}

size_t axvs_msda_workspace_bytes(int N, int Lq, int S, int C, int heads, int L, int P) {
  (void)C;
  return carved([&](Carver& c) { carve_msda_ws(c, N, Lq, S, heads, L, P); });
}

int axvs_msda_fwd(const float* query, const float* reference_points, int ref_dim, const float* input_flatten,
                  const unsigned char* padding_mask, const int* spatial_shapes, float* out, const void* packed, int N, int Lq, int S,
                  int C, int heads, int L, int P, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!query || !reference_points || !input_flatten || !spatial_shapes || !out || !packed || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (N <= 0 || Lq <= 0 || S <= 0 || P <= 0) return fail(AXVS_ERR_ARG, "empty shape");
  if (int rc = check_cfg(C, heads)) return rc;
  if (int rc = check_msda_points(ref_dim, L, P)) return rc;
  MsdaLevels lv;
  if (int rc = check_msda_shapes(N, Lq, S, spatial_shapes, L, &lv)) return rc;
  if (int rc = check_ws(workspace_bytes, axvs_msda_workspace_bytes(N, Lq, S, C, heads, L, P))) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Carver pc(const_cast<void*>(packed));
  const MsdaPacked mp = carve_msda(pc, C, heads, L, P);
  return by_dtype(dtype, [&](auto bf) { return msda_fwd_t<bf()>(query, reference_points, ref_dim, input_flatten, padding_mask, lv, out, mp, N, Lq, S, C, heads, P, workspace, st); });
}

// ---- the two halves of the module for callers that work on the sampled rows before output_proj (Tube-Link plugin) ----
int axvs_msda_sample_fwd(const float* query, const float* query_pos, const float* reference_points, int ref_dim, const float* value,
                         const unsigned char* padding_mask, const int* spatial_shapes, float* sampled, const void* packed, int N, int Lq,
                         int S, int C, int heads, int L, int P, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!query || !reference_points || !value || !spatial_shapes || !sampled || !packed || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (N <= 0 || Lq <= 0 || S <= 0 || P <= 0) return fail(AXVS_ERR_ARG, "empty shape");
  if (int rc = check_cfg(C, heads)) return rc;
  if ((C / heads) % 8) return fail(AXVS_ERR_ARG, "head_dim=%d must be a multiple of 8", C / heads);
  if (int rc = check_msda_points(ref_dim, L, P)) return rc;
  MsdaLevels lv;
  if (int rc = check_msda_shapes(N, Lq, S, spatial_shapes, L, &lv)) return rc;
  if (int rc = check_ws(workspace_bytes, axvs_msda_workspace_bytes(N, Lq, S, C, heads, L, P))) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Carver pc(const_cast<void*>(packed));
  const MsdaPacked mp = carve_msda(pc, C, heads, L, P);
  return by_dtype(dtype, [&](auto bf) {
    return msda_fwd_t<bf()>(query, reference_points, ref_dim, value, padding_mask, lv, sampled, mp, N, Lq, S, C, heads, P, workspace, st, query_pos, nullptr, 1);
  });
}

int axvs_msda_output_proj_fwd(const float* x, const float* identity, float* out, const void* packed, long long rows, int C, int heads,
                              int L, int P, int dtype, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!x || !out || !packed) return fail(AXVS_ERR_ARG, "null pointer");
  if (rows <= 0 || rows > 2147483647LL / 64) return fail(AXVS_ERR_ARG, "bad row count");
  if (int rc = check_cfg(C, heads)) return rc;
  if (C / heads != 32) return fail(AXVS_ERR_ARG, "axvs_msda_output_proj_fwd needs head_dim 32 (got %d)", C / heads);
  hipStream_t st = static_cast<hipStream_t>(stream);
  Carver pc(const_cast<void*>(packed));
  const MsdaPacked mp = carve_msda(pc, C, heads, L, P);
  const EpiRowsF32 e{out, identity, mp.bo, identity_map(rows), C, 1.f};
  // split-precision operands as in the module path (the projection output has no norm behind it)
  if (use_nt128(rows, C, heads)) {
    tr::GemmEpi e128{mp.bo, 1.f, 0, tr::Drop{0u, 0u, 0u, 1.f}, 0.f};
    e128.res = identity;
    if (int rc = launch_nt128(x, nullptr, mp.wo32, out, rows, C, C, e128, st, kNt128FeedsResidual)) return rc;
    return last_launch_status();
  }
  by_dtype(dtype, [&](auto bf) { launch_gemm<bf()>(ALoadRowsF32Split3<bf()>{x, (int)rows, C}, mp.wo, e, (int)rows, C, 3 * C, st); });
  return last_launch_status();
}

// ---- MSDeformAttnTransformerEncoderLayer (WC/msdeformattn.py:177-216): self-attention + residual, norm1, FFN, norm2 ----
size_t axvs_msda_layer_packed_bytes(int C, int heads, int L, int P, int d_ffn) { return carved([&](Carver& c) { carve_msda(c, C, heads, L, P); carve_ffn(c, C, d_ffn); }); }

int axvs_msda_layer_pack(const AxvsMsdaLayerParams* p, void* packed, int C, int heads, int L, int P, int d_ffn, int dtype, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!p || !packed) return fail(AXVS_ERR_ARG, "null pointer");
  if (int rc = check_ffn(d_ffn)) return rc;
  if (int rc = check_cfg(C, heads)) return rc;
  if (int rc = check_msda_pack(L, P)) return rc;
  Carver c(packed);
  const MsdaPacked m = carve_msda(c, C, heads, L, P);
  const LayerPacked l = carve_ffn(c, C, d_ffn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  pack_msda(dtype, p->self_attn, m, C, heads, L, P, st);
  pack_ffn(dtype, *p, l, C, d_ffn, st);
  return last_launch_status();
}

size_t axvs_msda_layer_workspace_bytes(int N, int S, int C, int heads, int L, int P, int d_ffn) { return carved([&](Carver& c) { carve_msda_layer_ws(c, N, S, C, heads, L, P, d_ffn); }); }

int axvs_msda_layer_fwd(const float* src, const float* pos, const float* reference_points, int ref_dim, const unsigned char* padding_mask,
                        const int* spatial_shapes, float* out, const void* packed, int N, int S, int C, int heads, int L, int P,
                        int d_ffn, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!src || !reference_points || !spatial_shapes || !out || !packed || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (N <= 0 || S <= 0 || P <= 0) return fail(AXVS_ERR_ARG, "empty shape");
  if (int rc = check_cfg(C, heads)) return rc;
  if (int rc = check_msda_points(ref_dim, L, P)) return rc;
  if (out == src) return fail(AXVS_ERR_ARG, "out must not alias src");
  MsdaLevels lv;
  if (int rc = check_msda_shapes(N, S, S, spatial_shapes, L, &lv)) return rc;
  if (int rc = check_ws(workspace_bytes, axvs_msda_layer_workspace_bytes(N, S, C, heads, L, P, d_ffn))) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Carver pc(const_cast<void*>(packed));
  const MsdaPacked mp = carve_msda(pc, C, heads, L, P);
  const LayerPacked lp = carve_ffn(pc, C, d_ffn);
  Carver wc(workspace);
  const MsdaLayerWs w = carve_msda_layer_ws(wc, N, S, C, heads, L, P, d_ffn);
  const long long M = (long long)N * S;
  if (int rc = by_dtype(dtype, [&](auto bf) { return msda_fwd_t<bf()>(src, reference_points, ref_dim, src, padding_mask, lv, w.f.x, mp, N, S, S, C, heads, P, w.mws, st, pos, src); })) return rc;
  return ffn_rows(dtype, w.f, out, lp, M, C, heads, d_ffn, st);
}

int axvs_msda_core_fwd(const float* value, const int* spatial_shapes, const float* sampling_loc, const float* attn_weight, float* out,
                       int N, int S, int M, int D, int Lq, int L, int P, void* stream) {
  if (!value || !spatial_shapes || !sampling_loc || !attn_weight || !out) return fail(AXVS_ERR_ARG, "null pointer");
  if (N <= 0 || S <= 0 || M <= 0 || D <= 0 || Lq <= 0 || P <= 0) return fail(AXVS_ERR_ARG, "empty shape");
  MsdaLevels lv;
  if (int rc = msda_levels(spatial_shapes, L, S, &lv)) return rc;
  const long long total = (long long)N * Lq * M * D;
  hipLaunchKernelGGL(msda_core_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), value, lv,
                     sampling_loc, attn_weight, out, N, S, M, D, Lq, P);
  return last_launch_status();
}

int axvs_msda_core_bwd(const float* value, const int* spatial_shapes, const float* sampling_loc, const float* attn_weight, const float* grad_output,
                       float* grad_value, float* grad_sampling_loc, float* grad_attn_weight, int N, int S, int M, int D, int Lq, int L, int P,
                       void* stream) {
  if (!value || !spatial_shapes || !sampling_loc || !attn_weight || !grad_output || !grad_value || !grad_sampling_loc || !grad_attn_weight)
    return fail(AXVS_ERR_ARG, "null pointer");
  if (N <= 0 || S <= 0 || M <= 0 || D <= 0 || Lq <= 0 || P <= 0) return fail(AXVS_ERR_ARG, "empty shape");
  MsdaLevels lv;
  if (int rc = msda_levels(spatial_shapes, L, S, &lv)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long total = (long long)N * Lq * M * D, samples = (long long)N * Lq * M * L * P;
  if (hipMemsetAsync(grad_value, 0, (size_t)N * S * M * D * sizeof(float), st) != hipSuccess) return fail(AXVS_ERR_LAUNCH, "hipMemsetAsync failed");
  const bool shfl = D <= 64 && (D & (D - 1)) == 0;        // a (n, q, m) group = D aligned lanes of one wave
  const dim3 grid((unsigned)((total + 255) / 256));
  if (shfl) {
    hipLaunchKernelGGL(msda_core_bwd_kernel<true>, grid, dim3(256), 0, st, value, lv, sampling_loc, attn_weight, grad_output, grad_value,
                       grad_sampling_loc, grad_attn_weight, N, S, M, D, Lq, P);
  } else {
    if (hipMemsetAsync(grad_sampling_loc, 0, (size_t)samples * 2 * sizeof(float), st) != hipSuccess ||
        hipMemsetAsync(grad_attn_weight, 0, (size_t)samples * sizeof(float), st) != hipSuccess)
      return fail(AXVS_ERR_LAUNCH, "hipMemsetAsync failed");
    hipLaunchKernelGGL(msda_core_bwd_kernel<false>, grid, dim3(256), 0, st, value, lv, sampling_loc, attn_weight, grad_output, grad_value,
                       grad_sampling_loc, grad_attn_weight, N, S, M, D, Lq, P);
  }
  return last_launch_status();
}

// ---- pixel-decoder glue ----
namespace {
struct ConvGnPacked {
  u16* w;                // split precision (hi | lo | hi) along K, rows in groups of 16
  float *b, *g, *be;     // conv bias, GroupNorm weight / bias
  float* wf;             // the fp32 weight as it is: the 128 x 128 split-precision GEMM splits its operands itself (token rows in, many rows)
};
ConvGnPacked carve_conv_gn(Carver& c, int Cin, int Cout) {
  ConvGnPacked p;
  p.w = c.take<u16>(3 * (size_t)Cin * ((Cout + 15) & ~15));
  p.b = c.take<float>(Cout);
  p.g = c.take<float>(Cout);
  p.be = c.take<float>(Cout);
  p.wf = c.take<float>((size_t)Cout * Cin);
  return p;
}
struct ConvGnWs {
  float *y, *stats, *partial, *tok;
};
// Callers size this workspace with max(Cin, Cout) in the Cout slot; the forward carves it with the real Cout.  The size is that of
// y | tok | stats | partial with an [M][Cout] block each for y and tok, so that the token-row copy of an NCHW input ([M][Cin]) fits a
// workspace sized that way (without the room the NCHW loader runs).  tok is the LAST block and ends where the workspace ends: it
// starts M Cout floats before the end, NOT on a 256-byte boundary.  Whatever the caller's buffer holds behind tok's [M][Cin] rows
// takes the split-K partials (axvs_conv1x1_gn_fwd).  stats is unused (the apply kernel sums the partials itself) and kept for the size.
ConvGnWs carve_conv_gn_ws(Carver& c, int N, int HW, int Cout, int groups) {
  const size_t ybytes = (size_t)N * HW * Cout * sizeof(float);
  ConvGnWs w;
  w.y = c.take<float>((size_t)N * HW * Cout);
  w.stats = c.take<float>((size_t)N * groups * 2);
  w.partial = c.take<float>((size_t)N * ((HW + 63) / 64) * groups * 2);
  c.off += align_up(ybytes) - ybytes;
  w.tok = c.take<float>((size_t)N * HW * Cout);
  return w;
}
}  // namespace

size_t axvs_conv1x1_gn_packed_bytes(int Cin, int Cout) { return carved([&](Carver& c) { carve_conv_gn(c, Cin, Cout); }); }

int axvs_conv1x1_gn_pack(const AxvsConvGnParams* p, void* packed, int Cin, int Cout, int dtype, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!p || !packed) return fail(AXVS_ERR_ARG, "null pointer");
  if (Cin <= 0 || Cin % 32 || Cout <= 0 || Cout % 4) return fail(AXVS_ERR_ARG, "Cin=%d must be a multiple of 32, Cout=%d of 4", Cin, Cout);
  Carver c(packed);
  const ConvGnPacked k = carve_conv_gn(c, Cin, Cout);
  hipStream_t st = static_cast<hipStream_t>(stream);
  PackDim nd{Cout, Cout, 0, 0, 0}, kd{Cin, Cin, 0, 0, 0};
  pack_w3(dtype, p->conv_w, k.w, nd, kd, st);
  copy_f32(p->conv_b, k.b, Cout, st);
  copy_f32(p->gn_w, k.g, Cout, st);
  copy_f32(p->gn_b, k.be, Cout, st);
  if (hipMemcpyAsync(k.wf, p->conv_w, (size_t)Cout * Cin * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(AXVS_ERR_LAUNCH, "copy failed");
  return last_launch_status();
}

size_t axvs_conv1x1_gn_workspace_bytes(int N, int HW, int Cout, int groups) { return carved([&](Carver& c) { carve_conv_gn_ws(c, N, HW, Cout, groups); }); }

int axvs_conv1x1_gn_fwd(const float* x, int in_layout, long long in_batch_stride, long long in_ld, float* out, int out_layout,
                        long long out_batch_stride, long long out_ld, const void* packed, int N, int HW, int Cin, int Cout, int groups,
                        float eps, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!x || !out || !packed || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (N <= 0 || HW <= 0) return fail(AXVS_ERR_ARG, "empty shape");
  if (Cin % 32 || Cout % 4 || groups <= 0 || Cout % groups || groups > 256) return fail(AXVS_ERR_ARG, "unsupported channels/groups %d/%d/%d", Cin, Cout, groups);
  if ((in_layout != 0 && in_layout != 1) || (out_layout != 0 && out_layout != 1)) return fail(AXVS_ERR_ARG, "layout must be 0 (NCHW) or 1 (token rows)");
  if ((long long)N * HW > 2147483647LL / 64) return fail(AXVS_ERR_ARG, "too many tokens for 32-bit row indices");
  if (int rc = check_ws(workspace_bytes, axvs_conv1x1_gn_workspace_bytes(N, HW, Cout, groups))) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Carver pc(const_cast<void*>(packed));
  const ConvGnPacked k = carve_conv_gn(pc, Cin, Cout);
  Carver wc(workspace);
  const long long M = (long long)N * HW;
  const ConvGnWs cw = carve_conv_gn_ws(wc, N, HW, Cout, groups);
  float *const y = cw.y, *const tok = cw.tok;
  // bytes the token-row copy of an NCHW input needs from the start of the workspace (its [M][Cin] rows may reach past the size query's end)
  const size_t tok_end = (size_t)(reinterpret_cast<char*>(tok) - static_cast<char*>(workspace)) + (size_t)M * Cin * sizeof(float);
  const int nblk = (HW + 63) / 64;
  if (Cout > 8192) return fail(AXVS_ERR_ARG, "Cout=%d too large for the GroupNorm statistics kernel", Cout);
  g_prof_next = 0;
  mark(st, "begin");
  const EpiRowsF32 ey{y, nullptr, k.b, identity_map(M), Cout, 1.f};
  // token rows in, many of them (the output projections of the large pyramid levels: [32786 x 512 x 256] at the shipped VIPSeg setting): the 128 x 128
  // three-piece kernel of the deformable attention's projections (fp32-grade like the split3 GEMM below; 143 against 60 - 115 TFLOP/s), one launch per
  // frame when the frames are rows of a larger buffer
  // (every launch has to fill the chip on its own: >= 192 tiles of 128 x 128 -- BASELINE config 3's 64 x 64 level, 64 tiles per frame, stays on the kernels below)
  const bool one = in_batch_stride == (long long)HW * in_ld;
  // split-K factor of the NCHW path: few 128 x 128 tiles and a long reduction -> enough workgroups for one round of the chip (at most 8, at least 4 k-steps each)
  int zs = 1;
  if (in_layout == 0 && kConvNt128SplitK && Cin >= kConvNt128SplitK) {
    const long long tiles = ((M + 127) / 128) * ((Cout + 127) / 128);
    if (tiles < kConvNt128Nchw && tiles >= 8) {
      zs = (int)std::min<long long>(8, std::max<long long>(1, 256 / tiles));
      zs = std::min(zs, Cin / 32 / 4);
      // the partials live behind the token-row copy: as many as the caller's workspace has room for
      const long long room = workspace_bytes > tok_end ? (long long)((workspace_bytes - tok_end) / ((size_t)M * Cout * sizeof(float))) : 0;
      zs = (int)std::min<long long>(zs, room);
      if (zs < 2) zs = 1;
    }
  }
  if (in_layout == 1 && kConvOnNt128 && Cin % 4 == 0 && Cout % 4 == 0 && in_ld % 4 == 0 && in_batch_stride % 4 == 0 &&
      (((one ? M : (long long)HW) + 127) / 128) * ((Cout + 127) / 128) >= kConvNt128 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
    const tr::GemmEpi e{k.b, 1.f, 0, tr::Drop{0, 0, 0, 1.f}, 0.f};
    for (int n = 0; n < (one ? 1 : N); ++n)
      if (int rc = launch_nt128(x + (size_t)n * in_batch_stride, nullptr, k.wf, y + (size_t)n * HW * Cout, one ? M : HW, Cout, Cin, e, st, kConvNt128Exact ? kNt128Fp32Grade : kNt128Plain, in_ld)) return rc;
  } else if (in_layout == 0 && kConvOnNt128 && Cin % 4 == 0 && Cout % 4 == 0 &&
             (((M + 127) / 128) * ((Cout + 127) / 128) >= kConvNt128Nchw || zs > 1) && (reinterpret_cast<uintptr_t>(y) & 15) == 0 &&
             workspace_bytes >= tok_end) {
    // NCHW in, many rows: transposed to token rows once, then the same 128 x 128 kernel.  Few row tiles and a long reduction (zs > 1; the
    // coarsest level: [2150 x 256 x 2048]): split-K partials behind the token rows, added in z order + bias
    float* part = tok + (size_t)M * Cin;
    const tr::GemmEpi e{zs > 1 ? nullptr : k.b, 1.f, 0, tr::Drop{0, 0, 0, 1.f}, 0.f};
    if (int rc = nchw_nt128(x, tok, k.wf, zs > 1 ? part : y, N, HW, Cin, Cout, e, st, kConvNt128Exact ? kNt128Fp32Grade : kNt128Plain, zs)) return rc;
    if (zs > 1) {
      const long long tot4 = M * Cout / 4;
      hipLaunchKernelGGL(splitk_sum_bias_kernel, dim3((unsigned)((tot4 + 255) / 256)), dim3(256), 0, st, (const float*)part, y, zs, M * Cout, k.b, Cout, tot4);
    }
  } else {
    by_dtype(dtype, [&](auto bf) {
      if (in_layout == 0) launch_gemm<bf()>(ALoadNCHWSplit3<bf()>{x, (int)M, Cin, HW}, k.w, ey, (int)M, Cout, 3 * Cin, st);
      else launch_gemm<bf()>(ALoadTokensSplit3<bf()>{x, (int)M, Cin, HW, in_batch_stride, in_ld}, k.w, ey, (int)M, Cout, 3 * Cin, st);
    });
  }
  mark(st, "glue.conv1x1");
  launch_gn_stats(y, cw.partial, N, HW, Cout, groups, st);
  // (the per-group sums of the blocks' partials are formed by the apply kernel itself: no launch of their own)
  const dim3 ag((unsigned)((HW + 63) / 64), (unsigned)((Cout + 63) / 64), N);
  if (out_layout == 0) hipLaunchKernelGGL((gn_apply_kernel<true>), ag, dim3(256), 0, st, y, (const float*)cw.partial, nblk, k.g, k.be, out, HW, Cout, groups, eps, (long long)0, (long long)Cout * HW);
  else hipLaunchKernelGGL((gn_apply_kernel<false>), ag, dim3(256), 0, st, y, (const float*)cw.partial, nblk, k.g, k.be, out, HW, Cout, groups, eps, out_ld, out_batch_stride);
  mark(st, "glue.group_norm");
  return last_launch_status();
}

int axvs_pos2d(float* pos, const float* add, int N, int H, int W, int C, long long S, long long row0, float temperature, int normalize,
               float scale, void* stream) {
  if (!pos) return fail(AXVS_ERR_ARG, "null pointer");
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 2 || row0 < 0 || row0 + (long long)H * W > S) return fail(AXVS_ERR_ARG, "bad shape");
  const long long total = (long long)H * W * C;
  hipLaunchKernelGGL(pos2d_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pos, add, N, H, W,
                     C, S, row0, temperature, normalize, scale);
  return last_launch_status();
}

int axvs_scaled_residual(const float* a, const float* b, const float* gamma, float* out, size_t n, int C, void* stream) {
  if (!a || !b || !gamma || !out || C <= 0) return fail(AXVS_ERR_ARG, "bad argument");
  hipLaunchKernelGGL(scaled_residual_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     a, b, gamma, out, n, C);
  return last_launch_status();
}

// ---- Tube-Link MSDeformAttnPixelDecoder (TL/mmdet/models/plugins/msdeformattn_pixel_decoder.py): encoder-layer FFN tail and FPN tail ----
size_t axvs_ffn_packed_bytes(int C, int d_ffn) { return carved([&](Carver& c) { carve_ffn(c, C, d_ffn); }); }

int axvs_ffn_pack(const AxvsFfnParams* p, void* packed, int C, int d_ffn, int dtype, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!p || !packed) return fail(AXVS_ERR_ARG, "null pointer");
  if (int rc = check_cfg(C, C / 32 > 0 ? C / 32 : 1)) return rc;
  if (int rc = check_ffn(d_ffn)) return rc;
  Carver c(packed);
  LayerPacked l = carve_ffn(c, C, d_ffn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  pack_ffn(dtype, *p, l, C, d_ffn, st);
  return last_launch_status();
}

int axvs_ffn_packed_fwd(const float* x, float* out, const void* packed_ffn, long long M, int C, int d_ffn, int dtype, void* workspace,
                        size_t workspace_bytes, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!x || !out || !packed_ffn || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (M <= 0) return fail(AXVS_ERR_ARG, "empty input");
  const int heads = C / 32 > 0 ? C / 32 : 1;      // head_dim 32: the fused FFN tier's configuration at C = 256 (heads only select the tier here)
  if (int rc = check_cfg(C, heads)) return rc;
  if (int rc = check_ffn(d_ffn)) return rc;
  if (int rc = check_ws(workspace_bytes, axvs_ffn_workspace_bytes(M, C, d_ffn))) return rc;
  Carver pc(const_cast<void*>(packed_ffn));
  return ffn_rows(dtype, x, out, carve_ffn(pc, C, d_ffn), M, C, heads, d_ffn, workspace, static_cast<hipStream_t>(stream));
}

namespace {
struct FpnPacked {
  u16 *lat_w3, *out_w, *mask_w;
  float *lat_wf, *lat_g, *lat_b, *out_g, *out_b, *mask_b;
};
FpnPacked carve_fpn(Carver& c, int Cin, int C, int Cm) {
  FpnPacked f{};
  f.lat_w3 = c.take<u16>(3 * (size_t)Cin * ((C + 15) & ~15));
  f.lat_wf = c.take<float>((size_t)C * Cin);
  f.lat_g = c.take<float>(C);
  f.lat_b = c.take<float>(C);
  f.out_w = c.take<u16>(9 * (size_t)C * C);
  f.out_g = c.take<float>(C);
  f.out_b = c.take<float>(C);
  if (Cm > 0) {
    f.mask_w = c.take<u16>((size_t)C * Cm);
    f.mask_b = c.take<float>(Cm);
  }
  return f;
}
struct FpnWs {
  float *tok, *lat, *gpart, *stats1, *cpart, *stats2;
  u16* m16;
};
FpnWs carve_fpn_ws(Carver& c, int N, int H, int W, int Cin, int C, int groups) {
  const size_t M = (size_t)N * H * W;
  const size_t nblk = (size_t)(H * W + 63) / 64, tiles = (size_t)((W + kFpnTW - 1) / kFpnTW) * ((H + kFpnTH - 1) / kFpnTH);
  FpnWs w{};
  w.tok = c.take<float>(M * Cin);            // token-row copy of the NCHW lateral input (128 x 128 GEMM path)
  w.lat = c.take<float>(M * C);              // raw lateral conv output, then the raw 3x3 conv output
  w.m16 = c.take<u16>(M * C);                // merged map, f16 channels-last rows
  w.gpart = c.take<float>((size_t)N * nblk * groups * 2);
  w.cpart = c.take<float>((size_t)N * tiles * C * 2);
  w.stats1 = c.take<float>((size_t)N * groups * 2);
  w.stats2 = c.take<float>((size_t)N * groups * 2);
  return w;
}
int fpn_check(int Cin, int C, int Cm) {
  if (Cin <= 0 || Cin % 32 || C <= 0 || C % 32 || C > 4096 || Cm < 0 || Cm % 32)
    return fail(AXVS_ERR_ARG, "Cin=%d and C=%d must be positive multiples of 32 (C <= 4096), Cm=%d a multiple of 32 (0: no mask_feature)", Cin, C, Cm);
  return AXVS_OK;
}
}  // namespace

size_t axvs_fpn_level_packed_bytes(int Cin, int C, int Cm) { return carved([&](Carver& c) { carve_fpn(c, Cin, C, Cm); }); }

int axvs_fpn_level_pack(const AxvsFpnLevelParams* p, void* packed, int Cin, int C, int Cm, int dtype, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!p || !packed || !p->lateral_w || !p->lateral_gn_w || !p->lateral_gn_b || !p->output_w || !p->output_gn_w || !p->output_gn_b)
    return fail(AXVS_ERR_ARG, "null pointer");
  if (int rc = fpn_check(Cin, C, Cm)) return rc;
  if (Cm > 0 && (!p->mask_w || !p->mask_b)) return fail(AXVS_ERR_ARG, "null pointer (mask_feature weights with Cm=%d)", Cm);
  Carver c(packed);
  const FpnPacked f = carve_fpn(c, Cin, C, Cm);
  hipStream_t st = static_cast<hipStream_t>(stream);
  PackDim nd{C, C, 0, 0, 0}, kd{Cin, Cin, 0, 0, 0}, md{Cm, Cm, 0, 0, 0}, cd{C, C, 0, 0, 0};
  const long long w3 = 9LL * C * C;
  pack_w3(dtype, p->lateral_w, f.lat_w3, nd, kd, st);
  by_dtype(dtype, [&](auto bf) { hipLaunchKernelGGL((fpn_pack3x3_kernel<bf()>), dim3((unsigned)((w3 + 255) / 256)), dim3(256), 0, st, p->output_w, f.out_w, C, C); });
  if (Cm > 0) pack_w(dtype, p->mask_w, f.mask_w, md, cd, st);
  if (hipMemcpyAsync(f.lat_wf, p->lateral_w, (size_t)C * Cin * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
    return fail(AXVS_ERR_LAUNCH, "copy failed");
  copy_f32(p->lateral_gn_w, f.lat_g, C, st);
  copy_f32(p->lateral_gn_b, f.lat_b, C, st);
  copy_f32(p->output_gn_w, f.out_g, C, st);
  copy_f32(p->output_gn_b, f.out_b, C, st);
  if (Cm > 0) copy_f32(p->mask_b, f.mask_b, Cm, st);
  return last_launch_status();
}

size_t axvs_fpn_level_workspace_bytes(int N, int H, int W, int Cin, int C, int groups) { return carved([&](Carver& c) { carve_fpn_ws(c, N, H, W, Cin, C, groups); }); }

int axvs_fpn_level_fwd(const float* x, const float* up, long long up_batch_stride, long long up_ld, int Hu, int Wu, float* y,
                       float* mask_feature, const void* packed, int N, int H, int W, int Cin, int C, int Cm, int groups, float eps, int dtype,
                       void* workspace, size_t workspace_bytes, void* stream) {
  if (int rcd = check_dtype(dtype)) return rcd;
  if (!x || !up || !packed || !workspace) return fail(AXVS_ERR_ARG, "null pointer");
  if (!y && !mask_feature) return fail(AXVS_ERR_ARG, "null pointer: neither y nor mask_feature requested");
  if (mask_feature && Cm <= 0) return fail(AXVS_ERR_ARG, "mask_feature requested from a pack without mask_feature weights (Cm=%d)", Cm);
  if (int rc = fpn_check(Cin, C, Cm)) return rc;
  if (N <= 0 || H <= 0 || W <= 0 || Hu <= 0 || Wu <= 0) return fail(AXVS_ERR_ARG, "empty shape");
  if (N > 65535) return fail(AXVS_ERR_ARG, "N=%d frames: at most 65535 (grid dimension)", N);
  if (groups <= 0 || C % groups) return fail(AXVS_ERR_ARG, "groups=%d must divide C=%d", groups, C);
  if ((long long)N * H * W > 2147483647LL / 64) return fail(AXVS_ERR_ARG, "N*H*W=%lld too large for 32-bit row indices", (long long)N * H * W);
  if (up_ld < C || up_ld % 4 || up_batch_stride % 4 || up_batch_stride < (long long)Hu * Wu * up_ld - (up_ld - C) ||
      (reinterpret_cast<uintptr_t>(up) & 15))
    return fail(AXVS_ERR_ARG, "up: row stride %lld / batch stride %lld must be multiples of 4 floats covering [Hu*Wu, C] rows, pointer 16-byte aligned",
                up_ld, up_batch_stride);
  if (int rc = check_ws(workspace_bytes, axvs_fpn_level_workspace_bytes(N, H, W, Cin, C, groups))) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Carver pc(const_cast<void*>(packed));
  const FpnPacked f = carve_fpn(pc, Cin, C, Cm);
  Carver wc(workspace);
  const FpnWs w = carve_fpn_ws(wc, N, H, W, Cin, C, groups);
  const int HW = H * W;
  const long long M = (long long)N * HW;
  const int nblk = (HW + 63) / 64, ntx = (W + kFpnTW - 1) / kFpnTW, tiles = ntx * ((H + kFpnTH - 1) / kFpnTH);
  g_prof_next = 0;
  mark(st, "begin");
  // 1. lateral 1x1 conv (no bias: use_bias = norm_cfg is None, TL:136) -> raw fp32 rows; the GEMMs of axvs_conv1x1_gn_fwd
  if (kConvOnNt128 && ((M + 127) / 128) * ((C + 127) / 128) >= kConvNt128Nchw) {
    const tr::GemmEpi e{nullptr, 1.f, 0, tr::Drop{0, 0, 0, 1.f}, 0.f};
    // (two pieces, as before: the lateral's GroupNorm output is merged into f16 rows, whose rounding is far above what the third piece buys)
    if (int rc = nchw_nt128(x, w.tok, f.lat_wf, w.lat, N, HW, Cin, C, e, st)) return rc;
  } else {
    const EpiRowsF32 ey{w.lat, nullptr, nullptr, identity_map(M), C, 1.f};
    by_dtype(dtype, [&](auto bf) { launch_gemm<bf()>(ALoadNCHWSplit3<bf()>{x, (int)M, Cin, HW}, f.lat_w3, ey, (int)M, C, 3 * Cin, st); });
  }
  mark(st, "fpn.lateral");
  launch_gn_stats(w.lat, w.gpart, N, HW, C, groups, st);
  hipLaunchKernelGGL(fpn_gn_finalize_kernel, dim3(groups, N), dim3(256), 0, st, (const float*)w.gpart, nblk, groups, 1, groups, H, W, 0, C / groups,
                     (double)HW * (C / groups), eps, w.stats1);
  // 2. GroupNorm apply + bilinear(up) -> merged f16 rows (TL:314-318)
  {
    const long long tot = M * (C / 4);
    by_dtype(dtype, [&](auto bf) {
      hipLaunchKernelGGL((fpn_merge_kernel<bf()>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (const float*)w.lat, (const float*)w.stats1, (const float*)f.lat_g,
                         (const float*)f.lat_b, up, up_batch_stride, up_ld, Hu, Wu, w.m16, N, H, W, C, groups);
    });
  }
  mark(st, "fpn.merge");
  // 3. 3x3 conv (implicit GEMM) + per-tile partial sums -> GroupNorm statistics (TL:319)
  {
    const dim3 grid((unsigned)tiles, (unsigned)((C + 255) / 256), (unsigned)N);
    by_dtype(dtype, [&](auto bf) { hipLaunchKernelGGL((fpn_conv3x3_kernel<bf()>), grid, dim3(256), 0, st, (const u16*)w.m16, (const u16*)f.out_w, w.lat, w.cpart, H, W, C, C, ntx); });
    mark(st, "fpn.conv3x3");
    hipLaunchKernelGGL(fpn_gn_finalize_kernel, dim3(groups, N), dim3(256), 0, st, (const float*)w.cpart, tiles, C, C / groups, groups, H, W, ntx, 0,
                       (double)HW * (C / groups), eps, w.stats2);
  }
  // 4. the level's output ReLU(GN(c)) as fp32 rows, when asked for
  if (y) {
    const long long tot = M * (C / 4);
    hipLaunchKernelGGL(fpn_gn_relu_rows_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (const float*)w.lat, (const float*)w.stats2,
                       (const float*)f.out_g, (const float*)f.out_b, y, M, HW, C, groups);
    mark(st, "fpn.gn_relu");
  }
  // 5. mask_feature = conv1x1(ReLU(GN(c))) + bias (TL:324), GroupNorm + ReLU in the A loader, NCHW fp32 out
  if (mask_feature) {
    const EpiNCHWBias em{mask_feature, f.mask_b, HW, Cm};
    by_dtype(dtype, [&](auto bf) { launch_gemm<bf()>(ALoadGnRelu<bf()>{w.lat, w.stats2, f.out_g, f.out_b, (int)M, C, HW, groups}, f.mask_w, em, (int)M, Cm, C, st); });
    mark(st, "fpn.mask_feature");
  }
  return last_launch_status();
}

}  // extern "C"
