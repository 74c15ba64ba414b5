// Training tier of TemporalAxialTrajectoryAttentionLayer behind the C ABI: forward that keeps the activations,
// and the backward pass.  Kernels: axvs_train.h; the Linear layers (forward, input gradient, weight gradient) run on the
// split-precision bf16 MFMA GEMM kernels of axvs_train_gemm.h (round 3: no vendor BLAS on this path any more).
#include "axvs_train_host.h"
#include "axvs_cc_train_host.h"
#include "axvs_glue_train.h"

namespace axvs {
namespace {

// norm1 -> FFN -> norm2 behind the attention (WC/temporal_attention.py:181-185): the same in both layers, whose parameter / gradient
// structs end in these eight fields
struct TailParams {
  const float *norm1_w, *norm1_b, *linear1_w, *linear1_b, *linear2_w, *linear2_b, *norm2_w, *norm2_b;
};
struct TailGrads {
  float *norm1_w, *norm1_b, *linear1_w, *linear1_b, *linear2_w, *linear2_b, *norm2_w, *norm2_b;
};
template <class P>
TailParams tail_params(const P& p) { return TailParams{p.norm1_w, p.norm1_b, p.linear1_w, p.linear1_b, p.linear2_w, p.linear2_b, p.norm2_w, p.norm2_b}; }
template <class G>
TailGrads tail_grads(const G& g) { return TailGrads{g.norm1_w, g.norm1_b, g.linear1_w, g.linear1_b, g.linear2_w, g.linear2_b, g.norm2_w, g.norm2_b}; }

// site_h / site_o: dropout sites of the FFN hidden and output (5, 6 in the trajectory layers)
int tail_fwd(const Ctx& c, const TailParams& p, const Saved& s, float* out, float p_drop, unsigned seed, unsigned site_h = 5, unsigned site_o = 6);

int forward(const Ctx& c, const float* src, const float* pos, float* out, const AxvsAxialLayerParams& p, const Saved& s, float p_drop,
            float p_attn, unsigned seed) {
  const Dims& d = c.d;
  const long long M = d.M, sB = (long long)d.T * d.H * d.W, sT = (long long)d.H * d.W;
  const int C = d.C;
  int rc;
  // height pass: sequences (b, w), tokens (t, h)        WC/temporal_attention.py:197-204
  const RowMap rmh{d.T * d.H, d.H, d.W, sB, sT, d.W, 1};
  if ((rc = pass_fwd(c, src, pos, s.buf1, p.height_attn, s.p[0], rmh, d.B * d.W, make_drop(p_drop, seed, 1), make_drop(p_attn, seed, 2))) != AXVS_OK)
    return rc;
  // width pass: sequences (b, h), tokens (t, w)         :206-213
  const RowMap rmw{d.T * d.W, d.W, d.H, sB, sT, 1, d.W};
  if ((rc = pass_fwd(c, s.buf1, pos, s.buf2, p.width_attn, s.p[1], rmw, d.B * d.H, make_drop(p_drop, seed, 3), make_drop(p_attn, seed, 4))) != AXVS_OK)
    return rc;
  return tail_fwd(c, tail_params(p), s, out, p_drop, seed);
}

// norm1 -> FFN -> norm2 on s.buf2 (dropout sites site_h, site_o)    WC/temporal_attention.py:181-185, :217-218 (:150-155 in the full layer)
int tail_fwd(const Ctx& c, const TailParams& p, const Saved& s, float* out, float p_drop, unsigned seed, unsigned site_h, unsigned site_o) {
  const Dims& d = c.d;
  const long long M = d.M;
  const int C = d.C;
  int rc;
  hipLaunchKernelGGL(tr_ln_fwd_kernel, dim3(blocks(M, 4)), dim3(256), 0, c.st, (const float*)s.buf2, p.norm1_w, p.norm1_b, s.z, s.mean1, s.rstd1, M, C, 1e-5f);
  {   // linear1 + bias + ReLU + dropout2 in one launch
    const GemmEpi e1{p.linear1_b, 1.f, 1, make_drop(p_drop, seed, site_h), 0.f};
    if ((rc = c.g.fwd(s.z, p.linear1_w, s.r, M, d.F, C, 0.f, &e1, g_train_exact != 0)) != AXVS_OK) return rc;
  }
  if ((rc = c.g.fwd(s.r, p.linear2_w, c.sc.t0, M, C, d.F, 0.f, nullptr, g_train_exact != 0)) != AXVS_OK) return rc;
  const RowMap id{(int)(M > INT32_MAX ? INT32_MAX : M), (int)(M > INT32_MAX ? INT32_MAX : M), 1, M, M, 1, 0};
  hipLaunchKernelGGL(tr_bias_drop_res_kernel, dim3(blocks((size_t)M * C / 4)), dim3(256), 0, c.st, (const float*)c.sc.t0, p.linear2_b, (const float*)s.z,
                     s.u, id, M, C, make_drop(p_drop, seed, site_o));
  hipLaunchKernelGGL(tr_ln_fwd_kernel, dim3(blocks(M, 4)), dim3(256), 0, c.st, (const float*)s.u, p.norm2_w, p.norm2_b, out, s.mean2, s.rstd2, M, C, 1e-5f);
  return last_launch_status();
}

// the full layer (WC/temporal_attention.py:133-155): one pass over all T*HW tokens of a clip (one sequence per clip, frames of HW keys;
// natural row order [(B T), HW] is the sequence order), dropout sites 1 (attention map) and 2 (pass output), then the same tail
// (traj_rowmap: axvs_train_host.h)
int traj_forward(const Ctx& c, const float* src, const float* pos, float* out, const AxvsTrajLayerParams& p, const Saved& s, float p_drop,
                 float p_attn, unsigned seed) {
  int rc;
  if ((rc = pass_fwd(c, src, pos, s.buf2, p.temporal_attn, s.p[0], traj_rowmap(c.d), c.d.B, make_drop(p_drop, seed, 1), make_drop(p_attn, seed, 2))) != AXVS_OK)
    return rc;
  return tail_fwd(c, tail_params(p), s, out, p_drop, seed);
}

// backward of the tail: d_out -> sc.g1 = gradient of s.buf2 (sc.g0 is overwritten)
int tail_bwd(const Ctx& c, const float* d_out, const TailParams& p, const TailGrads& g, const Saved& s, float p_dropout, unsigned seed,
             unsigned site_h = 5, unsigned site_o = 6) {
  const Dims& d = c.d;
  const Scratch& sc = c.sc;
  const long long M = d.M;
  const int C = d.C;
  const size_t MC = (size_t)M * C, MF = (size_t)M * d.F;
  int rc;
  // norm2                                                                       WC/temporal_attention.py:184
  c.colsum(d_out, M, C, g.norm2_b, s.u, s.mean2, s.rstd2, g.norm2_w);
  hipLaunchKernelGGL(tr_ln_bwd_kernel, dim3(blocks(M, 4)), dim3(256), 0, c.st, d_out, (const float*)s.u, p.norm2_w, (const float*)s.mean2,
                     (const float*)s.rstd2, sc.g0, M, C);                                 // g0 = d u
  // FFN: u = z + dropout3(linear2(r)), r = dropout2(relu(linear1(z)))             :181-183
  const RowMap id{(int)M, (int)M, 1, M, M, 1, 0};
  hipLaunchKernelGGL(tr_drop_bwd_kernel, dim3(blocks(MC / 4)), dim3(256), 0, c.st, (const float*)sc.g0, sc.t0, id, M, C, make_drop(p_dropout, seed, site_o));
  if ((rc = c.wgrad(sc.t0, s.r, g.linear2_w, M, C, d.F, g.linear2_b)) != AXVS_OK) return rc;
  if ((rc = c.dgrad(sc.t0, p.linear2_w, sc.dr, M, C, d.F, 0.f)) != AXVS_OK) return rc;
  hipLaunchKernelGGL(tr_relu_drop_bwd_kernel, dim3(blocks(MF / 4)), dim3(256), 0, c.st, sc.dr, (const float*)s.r, MF / 4, make_drop(p_dropout, seed, site_h).scale);
  if ((rc = c.wgrad(sc.dr, s.z, g.linear1_w, M, d.F, C, g.linear1_b)) != AXVS_OK) return rc;
  if ((rc = c.dgrad(sc.dr, p.linear1_w, sc.g0, M, d.F, C, 1.f)) != AXVS_OK) return rc;   // g0 = d z = d u + d r W1
  // norm1                                                                       :217
  c.colsum(sc.g0, M, C, g.norm1_b, s.buf2, s.mean1, s.rstd1, g.norm1_w);
  hipLaunchKernelGGL(tr_ln_bwd_kernel, dim3(blocks(M, 4)), dim3(256), 0, c.st, (const float*)sc.g0, (const float*)s.buf2, p.norm1_w,
                     (const float*)s.mean1, (const float*)s.rstd1, sc.g1, M, C);          // g1 = d buf2
  return AXVS_OK;
}

// the shared prologue of the four entry points of each trajectory layer: buffers, checks, stream
int train_setup(Ctx& c, Saved& s, int npass, bool backward, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream) {
  Carver sb(saved), cb(scratch);
  s = carve_saved(sb, c.d, npass);
  c.sc = carve_scratch(cb, c.d, backward);
  c.scale = 1.f / sqrtf((float)c.d.D);
  return train_begin(c, sb, saved_bytes, cb, scratch_bytes, stream);
}

// ---- 1x1 convolution + GroupNorm in train() mode (axvs_glue_train.h) ----
struct ConvGnBufs {
  float *y, *stats;                // saved: conv output [M][Cout] (token rows), (mean, rstd) [N][G][2]
  float* xt;                       // saved: the input as contiguous token rows [M][Cin] (null when the caller's x already is)
  float *part, *ab, *S, *dy, *dxt, *otok;      // scratch
  float *wpart, *part_a, *wt;      // scratch of the weight-gradient / input-gradient GEMMs
};
ConvGnBufs carve_convgn(Carver& sv, Carver& sc, long long N, long long HW, int Cin, int Cout, int G, bool copy_x, bool backward, bool out_nchw) {
  ConvGnBufs b{};
  const size_t M = (size_t)(N * HW);
  const int nblk = (int)((HW + 63) / 64);
  b.y = sv.f(M * Cout);
  b.stats = sv.f((size_t)N * G * 2);
  b.xt = copy_x ? sv.f(M * Cin) : nullptr;
  b.part = sc.f((size_t)N * nblk * Cout * 2);
  b.ab = sc.f((size_t)N * Cout * 2);
  b.otok = out_nchw ? sc.f(M * Cout) : nullptr;
  if (backward) {
    b.S = sc.f((size_t)N * G * 2);
    b.dy = sc.f(M * Cout);
    b.dxt = sc.f(M * Cin);
    b.wpart = sc.f((size_t)(Gemm::kSplit + 1) * Cout * Cin);
    b.part_a = sc.f((size_t)kColsumBlocks * (Cout > Cin ? Cout : Cin));
    b.wt = sc.f((size_t)Cout * Cin);
  }
  return b;
}
int convgn_check(int N, int HW, int Cin, int Cout, int G, int in_layout, int out_layout, long long in_bs, long long in_ld, long long out_bs, long long out_ld) {
  if (N <= 0 || HW <= 0) return fail(AXVS_ERR_ARG, "empty shape");
  if (Cin % 8 || Cout % 8 || G <= 0 || Cout % G) return fail(AXVS_ERR_ARG, "conv1x1 + GroupNorm training tier: Cin=%d and Cout=%d must be multiples of 8, Cout of groups=%d", Cin, Cout, G);
  if ((in_layout != 0 && in_layout != 1) || (out_layout != 0 && out_layout != 1)) return fail(AXVS_ERR_ARG, "layout must be 0 (NCHW) or 1 (token rows)");
  if (in_layout == 1 && (in_ld % 4 || in_bs % 4 || in_ld < Cin)) return fail(AXVS_ERR_ARG, "token rows: strides must be multiples of 4 floats");
  if (out_layout == 1 && (out_ld % 4 || out_bs % 4 || out_ld < Cout)) return fail(AXVS_ERR_ARG, "token rows: strides must be multiples of 4 floats");
  return AXVS_OK;
}

// ---- MSDeformAttnTransformerEncoderLayer in train() mode (WC/msdeformattn.py:177-216 under autograd) ----------------------------------
// value_proj (padded keys zeroed), the sampling_offsets | attention_weights GEMM on src + pos, the sampling head (md_head_*_kernel),
// the fp32 core op of the library (axvs_msda_core_fwd / _bwd), output_proj, dropout1 + residual, then the trajectory layers' tail.
// Dropout sites 7 (dropout1, [N, S, C]), 8 (dropout2, [N, S, d_ffn]), 9 (dropout3, [N, S, C]).
constexpr unsigned kMdSite1 = 7, kMdSite2 = 8, kMdSite3 = 9;

struct MdShape {
  Dims d;                          // B = N, T = 1, H = 1, W = S: M = N S token rows
  int N, S, L, P, LP, NO;          // NO = heads L P 3: width of the offsets | logits rows
  int ref_dim;
  int shapes[2 * kMdMaxLevels];    // (H_l, W_l)
  MdLevels lv;
};

int make_md_shape(MdShape& m, int N, int S, int C, int heads, int L, int P, int F) {
  if (N <= 0 || S <= 0 || L <= 0 || P <= 0) return fail(AXVS_ERR_ARG, "non-positive dimension");
  if (L > kMdMaxLevels) return fail(AXVS_ERR_ARG, "deformable layer training tier: n_levels=%d > %d", L, kMdMaxLevels);
  if (L * P > kMdMaxLP) return fail(AXVS_ERR_ARG, "deformable layer training tier: n_levels * n_points = %d > %d", L * P, kMdMaxLP);
  if ((long long)heads * L * P % 8) return fail(AXVS_ERR_ARG, "deformable layer training tier: n_heads * n_levels * n_points = %d must be a multiple of 8", heads * L * P);
  if (int rc = make_dims_any(m.d, N, 1, 1, S, C, heads, F)) return rc;
  m.N = N; m.S = S; m.L = L; m.P = P; m.LP = L * P; m.NO = heads * L * P * 3;
  m.lv.L = L;
  m.lv.P = P;
  return AXVS_OK;
}

// the run-time arguments the size functions do not see: reference-point form and spatial shapes (HOST ints)
int md_levels(MdShape& m, int ref_dim, const int* spatial_shapes) {
  if (ref_dim != 2 && ref_dim != 4) return fail(AXVS_ERR_ARG, "Last dim of reference_points must be 2 or 4, got %d", ref_dim);
  m.ref_dim = ref_dim;
  long long total = 0;
  for (int l = 0; l < m.L; ++l) {
    const int H = spatial_shapes[2 * l], W = spatial_shapes[2 * l + 1];
    if (H <= 0 || W <= 0) return fail(AXVS_ERR_ARG, "empty level %d", l);
    m.shapes[2 * l] = H;
    m.shapes[2 * l + 1] = W;
    m.lv.h[l] = (float)H;
    m.lv.w[l] = (float)W;
    total += (long long)H * W;
  }
  if (total != m.S) return fail(AXVS_ERR_ARG, "spatial shapes cover %lld tokens, src has %d", total, m.S);
  return AXVS_OK;
}

struct MdSaved {
  Saved t;                         // buf2 = src + dropout1(attention), then the tail's activations
  float *value, *loc, *aw, *samp;  // value_proj(src) masked [M][C], locations, softmaxed weights, sampled rows [M][C]
};
struct MdScratch {
  float *wcat, *bcat, *offlog;                  // [sampling_offsets; attention_weights] weight / bias, offsets | logits [M][NO]
  float *dval, *dsamp, *gloc, *gaw, *doff;      // backward
};

MdSaved carve_md_saved(Carver& b, const MdShape& m) {
  MdSaved s{};
  const size_t MC = (size_t)m.d.M * m.d.C, MH = (size_t)m.d.M * m.d.heads * m.LP;
  s.t = carve_saved(b, m.d, 0);
  s.value = b.f(MC);
  s.loc = b.f(MH * 2);
  s.aw = b.f(MH);
  s.samp = b.f(MC);
  return s;
}

// the Scratch fields the shared code uses here: a, t0 (forward); g0, g1, dr, part_a / part_b, wpart, wt (backward)
void carve_md_scratch(Carver& b, const MdShape& m, bool backward, Scratch& sc, MdScratch& x) {
  const Dims& d = m.d;
  const size_t MC = (size_t)d.M * d.C, MH = (size_t)d.M * d.heads * m.LP;
  sc = Scratch{};
  x = MdScratch{};
  sc.a = b.f(MC);
  sc.t0 = b.f(MC);
  x.wcat = b.f((size_t)m.NO * d.C);
  x.bcat = b.f(m.NO);
  x.offlog = b.f((size_t)d.M * m.NO);
  if (!backward) return;
  sc.g0 = b.f(MC);
  sc.g1 = b.f(MC);
  sc.dr = b.f((size_t)d.M * d.F);
  size_t wide = (size_t)(d.F > m.NO ? d.F : m.NO);
  if (wide < (size_t)d.C) wide = d.C;
  sc.part_a = b.f(kColsumBlocks * wide);
  sc.part_b = b.f(kColsumBlocks * wide);
  const size_t wmax = (size_t)d.C * wide;       // largest weight: linear1 / linear2 [F, C] or the fused [NO, C]
  sc.wpart = b.f((Gemm::kSplit + 1) * wmax);
  sc.wt = b.f(wmax);
  x.dval = b.f(MC);
  x.dsamp = b.f(MC);
  x.gloc = b.f(MH * 2);
  x.gaw = b.f(MH);
  x.doff = b.f((size_t)d.M * m.NO);
}

int md_setup(Ctx& c, const MdShape& m, MdSaved& s, MdScratch& x, bool backward, void* saved, size_t saved_bytes, void* scratch,
             size_t scratch_bytes, void* stream) {
  Carver sb(saved), cb(scratch);
  c.d = m.d;
  s = carve_md_saved(sb, m);
  carve_md_scratch(cb, m, backward, c.sc, x);
  c.scale = 1.f;
  return train_begin(c, sb, saved_bytes, cb, scratch_bytes, stream);
}

// [sampling_offsets; attention_weights] weight and bias, so that the query path is one GEMM (and one input-gradient GEMM)
int md_concat_weights(const Ctx& c, const MdShape& m, const AxvsMsdaParams& a, const MdScratch& x) {
  const size_t no = (size_t)m.d.heads * m.LP * 2, nl = (size_t)m.d.heads * m.LP, C = m.d.C;
  if (hipMemcpyAsync(x.wcat, a.sampling_offsets_w, no * C * sizeof(float), hipMemcpyDeviceToDevice, c.st) != hipSuccess ||
      hipMemcpyAsync(x.wcat + no * C, a.attention_weights_w, nl * C * sizeof(float), hipMemcpyDeviceToDevice, c.st) != hipSuccess ||
      hipMemcpyAsync(x.bcat, a.sampling_offsets_b, no * sizeof(float), hipMemcpyDeviceToDevice, c.st) != hipSuccess ||
      hipMemcpyAsync(x.bcat + no, a.attention_weights_b, nl * sizeof(float), hipMemcpyDeviceToDevice, c.st) != hipSuccess)
    return fail(AXVS_ERR_LAUNCH, "hipMemcpyAsync failed");
  return AXVS_OK;
}

inline RowMap md_rowmap(long long M) { return RowMap{(int)M, (int)M, 1, M, M, 1, 0}; }

int md_forward(const Ctx& c, const MdShape& m, const MdScratch& x, const float* src, const float* pos, const float* ref,
               const unsigned char* mask, float* out, const AxvsMsdaLayerParams& p, const MdSaved& s, float p_drop, float p_attn, unsigned seed) {
  const Dims& d = c.d;
  const long long M = d.M;
  const int C = d.C;
  const AxvsMsdaParams& a = p.self_attn;
  const bool ex = g_train_exact != 0;
  const Drop none = make_drop(0.f, 0, 0);
  int rc;
  // value = value_proj(src), rows of padded keys zeroed                       OPS/modules/ms_deform_attn.py:98-100
  const GemmEpi ev{a.value_proj_b, 1.f, 0, none, 0.f};
  if ((rc = c.g.fwd(src, a.value_proj_w, s.value, M, C, C, 0.f, &ev, ex)) != AXVS_OK) return rc;
  if (mask) hipLaunchKernelGGL(md_zero_rows_kernel, dim3(blocks((size_t)M * C / 4)), dim3(256), 0, c.st, s.value, mask, M, C);
  // offsets | logits = [sampling_offsets; attention_weights](src + pos): the sum is formed in the GEMM's loader    :101-104
  if ((rc = md_concat_weights(c, m, a, x)) != AXVS_OK) return rc;
  const GemmEpi eo{x.bcat, 1.f, 0, none, 0.f};
  if ((rc = c.g.fwd(src, x.wcat, x.offlog, M, m.NO, C, 0.f, &eo, ex, pos)) != AXVS_OK) return rc;
  hipLaunchKernelGGL(md_head_fwd_kernel, dim3(blocks((size_t)M * d.heads)), dim3(256), 0, c.st, (const float*)x.offlog, ref, m.ref_dim, s.loc, s.aw,
                     M, d.heads, m.lv);
  if ((rc = axvs_msda_core_fwd(s.value, m.shapes, s.loc, s.aw, s.samp, m.N, m.S, d.heads, d.D, m.S, m.L, m.P, c.st)) != AXVS_OK) return rc;
  // buf2 = src + dropout1(output_proj(sampled))                                 WC/msdeformattn.py:210-211
  if ((rc = c.g.fwd(s.samp, a.output_proj_w, c.sc.t0, M, C, C, 0.f, nullptr, ex)) != AXVS_OK) return rc;
  hipLaunchKernelGGL(tr_bias_drop_res_kernel, dim3(blocks((size_t)M * C / 4)), dim3(256), 0, c.st, (const float*)c.sc.t0, a.output_proj_b, src, s.t.buf2,
                     md_rowmap(M), M, C, make_drop(p_attn, seed, kMdSite1));
  return tail_fwd(c, tail_params(p), s.t, out, p_drop, seed, kMdSite2, kMdSite3);                          // :211-215
}

int md_backward(const Ctx& c, const MdShape& m, const MdScratch& x, const float* d_out, const float* src, const float* pos, const float* ref,
                const unsigned char* mask, const AxvsMsdaLayerParams& p, const AxvsMsdaLayerGrads& g, float* d_src, float* d_pos, const MdSaved& s,
                float p_drop, float p_attn, unsigned seed) {
  const Dims& d = c.d;
  const Scratch& sc = c.sc;
  const long long M = d.M;
  const int C = d.C, HLP = d.heads * m.LP;
  const size_t MC = (size_t)M * C;
  const AxvsMsdaParams& a = p.self_attn;
  int rc;
  if ((rc = tail_bwd(c, d_out, tail_params(p), tail_grads(g), s.t, p_drop, seed, kMdSite2, kMdSite3)) != AXVS_OK) return rc;   // sc.g1 = d buf2
  // output_proj and dropout1
  hipLaunchKernelGGL(tr_drop_bwd_kernel, dim3(blocks(MC / 4)), dim3(256), 0, c.st, (const float*)sc.g1, sc.t0, md_rowmap(M), M, C, make_drop(p_attn, seed, kMdSite1));
  if ((rc = c.wgrad(sc.t0, s.samp, g.self_attn.output_proj_w, M, C, C, g.self_attn.output_proj_b)) != AXVS_OK) return rc;
  if ((rc = c.dgrad(sc.t0, a.output_proj_w, x.dsamp, M, C, C, 0.f)) != AXVS_OK) return rc;
  // the core op: gradients of the value, the locations and the weights; padded keys get none
  if ((rc = axvs_msda_core_bwd(s.value, m.shapes, s.loc, s.aw, x.dsamp, x.dval, x.gloc, x.gaw, m.N, m.S, d.heads, d.D, m.S, m.L, m.P, c.st)) != AXVS_OK)
    return rc;
  if (mask) hipLaunchKernelGGL(md_zero_rows_kernel, dim3(blocks(MC / 4)), dim3(256), 0, c.st, x.dval, mask, M, C);
  hipLaunchKernelGGL(md_head_bwd_kernel, dim3(blocks((size_t)M * d.heads)), dim3(256), 0, c.st, (const float*)x.gloc, (const float*)x.gaw, (const float*)s.aw,
                     ref, m.ref_dim, x.doff, M, d.heads, m.lv);
  // weight gradients of the three input Linears
  const float* const xa = pos ? sc.a : src;
  if (pos) c.add(src, pos, sc.a, MC);
  if ((rc = c.wgrad(x.doff, xa, g.self_attn.sampling_offsets_w, M, 2 * HLP, C, g.self_attn.sampling_offsets_b, m.NO)) != AXVS_OK) return rc;
  if ((rc = c.wgrad(x.doff + 2 * HLP, xa, g.self_attn.attention_weights_w, M, HLP, C, g.self_attn.attention_weights_b, m.NO)) != AXVS_OK) return rc;
  if ((rc = c.wgrad(x.dval, src, g.self_attn.value_proj_w, M, C, C, g.self_attn.value_proj_b)) != AXVS_OK) return rc;
  // t0 = d(src + pos) through the query path; d_src = d buf2 (residual) + dval Wv + t0;  d_pos = t0
  if ((rc = md_concat_weights(c, m, a, x)) != AXVS_OK) return rc;
  if ((rc = c.dgrad(x.doff, x.wcat, sc.t0, M, m.NO, C, 0.f)) != AXVS_OK) return rc;
  if ((rc = c.dgrad(x.dval, a.value_proj_w, d_src, M, C, C, 0.f, 0, false, 1.f, sc.g1, sc.t0)) != AXVS_OK) return rc;
  if (d_pos && hipMemcpyAsync(d_pos, sc.t0, MC * sizeof(float), hipMemcpyDeviceToDevice, c.st) != hipSuccess)
    return fail(AXVS_ERR_LAUNCH, "hipMemcpyAsync failed");
  return last_launch_status();
}

}  // namespace
}  // namespace axvs

using namespace axvs;

extern "C" {

size_t axvs_axial_layer_train_saved_bytes(int B, int T, int H, int W, int C, int heads, int d_ffn) {
  Dims d;
  if (make_dims(d, B, T, H, W, C, heads, d_ffn) != AXVS_OK) return 0;
  Carver b(nullptr);
  carve_saved(b, d);
  return b.off;
}

size_t axvs_axial_layer_train_scratch_bytes(int B, int T, int H, int W, int C, int heads, int d_ffn, int backward) {
  Dims d;
  if (make_dims(d, B, T, H, W, C, heads, d_ffn) != AXVS_OK) return 0;
  Carver b(nullptr);
  carve_scratch(b, d, backward != 0);
  return b.off;
}

int axvs_axial_layer_train_fwd(const float* src, const float* pos, float* out, const AxvsAxialLayerParams* params, int B, int T, int H,
                               int W, int C, int heads, int d_ffn, float p_dropout, float p_attn_drop, unsigned seed, void* saved,
                               size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream) {
  if (!src || !pos || !out || !params || !saved || !scratch) return fail(AXVS_ERR_ARG, "null pointer");
  if (int rc = check_drop(p_dropout, p_attn_drop)) return rc;
  Ctx c{};
  Saved s;
  int rc;
  if ((rc = make_dims(c.d, B, T, H, W, C, heads, d_ffn)) != AXVS_OK || (rc = check_ptrs(params, "AxvsAxialLayerParams")) != AXVS_OK) return rc;
  if ((rc = train_setup(c, s, 2, false, saved, saved_bytes, scratch, scratch_bytes, stream)) != AXVS_OK) return rc;
  return forward(c, src, pos, out, *params, s, p_dropout, p_attn_drop, seed);
}

int axvs_axial_layer_train_bwd(const float* d_out, const float* src, const float* pos, const AxvsAxialLayerParams* params,
                               const AxvsAxialLayerGrads* grads, float* d_src, float* d_pos, int B, int T, int H, int W, int C, int heads,
                               int d_ffn, float p_dropout, float p_attn_drop, unsigned seed, int recompute, void* saved, size_t saved_bytes,
                               void* scratch, size_t scratch_bytes, void* stream) {
  if (!d_out || !src || !pos || !params || !grads || !d_src || !saved || !scratch) return fail(AXVS_ERR_ARG, "null pointer");
  if (int rc = check_drop(p_dropout, p_attn_drop)) return rc;
  Ctx c{};
  Saved s;
  int rc;
  if ((rc = make_dims(c.d, B, T, H, W, C, heads, d_ffn)) != AXVS_OK || (rc = check_ptrs(params, "AxvsAxialLayerParams")) != AXVS_OK ||
      (rc = check_ptrs(grads, "AxvsAxialLayerGrads")) != AXVS_OK)
    return rc;
  if ((rc = train_setup(c, s, 2, true, saved, saved_bytes, scratch, scratch_bytes, stream)) != AXVS_OK) return rc;
  const Dims& d = c.d;
  const AxvsAxialLayerParams& p = *params;
  const AxvsAxialLayerGrads& g = *grads;
  const Scratch& sc = c.sc;
  const long long sB = (long long)d.T * d.H * d.W, sT = (long long)d.H * d.W;
  if (recompute) {   // rebuild the activations from (src, pos, seed) instead of having kept them since the forward pass
    if ((rc = forward(c, src, pos, sc.g0, p, s, p_dropout, p_attn_drop, seed)) != AXVS_OK) return rc;
  }
  if ((rc = tail_bwd(c, d_out, tail_params(p), tail_grads(g), s, p_dropout, seed)) != AXVS_OK) return rc;     // sc.g1 = d buf2
  // width pass, then height pass
  const RowMap rmw{d.T * d.W, d.W, d.H, sB, sT, 1, d.W};
  if ((rc = pass_bwd(c, sc.g1, s.buf1, pos, p.width_attn, g.width_attn, s.p[1], rmw, d.B * d.H, make_drop(p_dropout, seed, 3),
                     make_drop(p_attn_drop, seed, 4), sc.g0, d_pos, true)) != AXVS_OK)
    return rc;
  const RowMap rmh{d.T * d.H, d.H, d.W, sB, sT, d.W, 1};
  if ((rc = pass_bwd(c, sc.g0, src, pos, p.height_attn, g.height_attn, s.p[0], rmh, d.B * d.W, make_drop(p_dropout, seed, 1),
                     make_drop(p_attn_drop, seed, 2), d_src, d_pos, false)) != AXVS_OK)
    return rc;
  return last_launch_status();
}

// ---- the full T*H*W layer (TemporalTrajectoryAttentionLayer), training tier: the axial layer's pass and tail code -----------------------
size_t axvs_traj_layer_train_saved_bytes(int B, int T, int HW, int C, int heads, int d_ffn) {
  Dims d;
  if (make_traj_dims(d, B, T, HW, C, heads, d_ffn) != AXVS_OK) return 0;
  Carver b(nullptr);
  carve_saved(b, d, 1);
  return b.off;
}

size_t axvs_traj_layer_train_scratch_bytes(int B, int T, int HW, int C, int heads, int d_ffn, int backward) {
  Dims d;
  if (make_traj_dims(d, B, T, HW, C, heads, d_ffn) != AXVS_OK) return 0;
  Carver b(nullptr);
  carve_scratch(b, d, backward != 0);
  return b.off;
}

int axvs_traj_layer_train_fwd(const float* src, const float* pos, float* out, const AxvsTrajLayerParams* params, int B, int T, int HW, int C,
                              int heads, int d_ffn, float p_dropout, float p_attn_drop, unsigned seed, void* saved, size_t saved_bytes, void* scratch,
                              size_t scratch_bytes, void* stream) {
  if (!src || !pos || !out || !params || !saved || !scratch) return fail(AXVS_ERR_ARG, "null pointer");
  if (int rc = check_drop(p_dropout, p_attn_drop)) return rc;
  Ctx c{};
  Saved s;
  int rc;
  if ((rc = make_traj_dims(c.d, B, T, HW, C, heads, d_ffn)) != AXVS_OK || (rc = check_ptrs(params, "AxvsTrajLayerParams")) != AXVS_OK) return rc;
  if ((rc = train_setup(c, s, 1, false, saved, saved_bytes, scratch, scratch_bytes, stream)) != AXVS_OK) return rc;
  return traj_forward(c, src, pos, out, *params, s, p_dropout, p_attn_drop, seed);
}

int axvs_traj_layer_train_bwd(const float* d_out, const float* src, const float* pos, const AxvsTrajLayerParams* params, const AxvsTrajLayerGrads* grads,
                              float* d_src, float* d_pos, int B, int T, int HW, int C, int heads, int d_ffn, float p_dropout, float p_attn_drop,
                              unsigned seed, int recompute, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream) {
  if (!d_out || !src || !pos || !params || !grads || !d_src || !saved || !scratch) return fail(AXVS_ERR_ARG, "null pointer");
  if (int rc = check_drop(p_dropout, p_attn_drop)) return rc;
  Ctx c{};
  Saved s;
  int rc;
  if ((rc = make_traj_dims(c.d, B, T, HW, C, heads, d_ffn)) != AXVS_OK || (rc = check_ptrs(params, "AxvsTrajLayerParams")) != AXVS_OK ||
      (rc = check_ptrs(grads, "AxvsTrajLayerGrads")) != AXVS_OK)
    return rc;
  if ((rc = train_setup(c, s, 1, true, saved, saved_bytes, scratch, scratch_bytes, stream)) != AXVS_OK) return rc;
  if (recompute) {
    if ((rc = traj_forward(c, src, pos, c.sc.g0, *params, s, p_dropout, p_attn_drop, seed)) != AXVS_OK) return rc;
  }
  if ((rc = tail_bwd(c, d_out, tail_params(*params), tail_grads(*grads), s, p_dropout, seed)) != AXVS_OK) return rc;     // sc.g1 = d buf2
  if ((rc = pass_bwd(c, c.sc.g1, src, pos, params->temporal_attn, grads->temporal_attn, s.p[0], traj_rowmap(c.d), B, make_drop(p_dropout, seed, 1),
                     make_drop(p_attn_drop, seed, 2), d_src, d_pos, true)) != AXVS_OK)
    return rc;
  return last_launch_status();
}

// ---- MSDeformAttnTransformerEncoderLayer, training tier ------------------------------------------------------------------------
size_t axvs_msda_layer_train_saved_bytes(int N, int S, int C, int heads, int L, int P, int d_ffn) {
  MdShape m;
  if (make_md_shape(m, N, S, C, heads, L, P, d_ffn) != AXVS_OK) return 0;
  Carver b(nullptr);
  carve_md_saved(b, m);
  return b.off;
}
size_t axvs_msda_layer_train_scratch_bytes(int N, int S, int C, int heads, int L, int P, int d_ffn, int backward) {
  MdShape m;
  if (make_md_shape(m, N, S, C, heads, L, P, d_ffn) != AXVS_OK) return 0;
  Carver b(nullptr);
  Scratch sc;
  MdScratch x;
  carve_md_scratch(b, m, backward != 0, sc, x);
  return b.off;
}
int axvs_msda_layer_train_fwd(const float* src, const float* pos, const float* reference_points, int ref_dim, const unsigned char* padding_mask,
                              const int* spatial_shapes, float* out, const AxvsMsdaLayerParams* params, int N, int S, int C, int heads, int L, int P,
                              int d_ffn, float p_dropout, float p_attn_drop, unsigned seed, void* saved, size_t saved_bytes, void* scratch,
                              size_t scratch_bytes, void* stream) {
  if (!src || !reference_points || !spatial_shapes || !out || !params || !saved || !scratch) return fail(AXVS_ERR_ARG, "null pointer");
  if (int rc = check_drop(p_dropout, p_attn_drop)) return rc;
  MdShape m;
  Ctx c{};
  MdSaved s;
  MdScratch x;
  int rc;
  if ((rc = make_md_shape(m, N, S, C, heads, L, P, d_ffn)) != AXVS_OK || (rc = md_levels(m, ref_dim, spatial_shapes)) != AXVS_OK ||
      (rc = check_ptrs(params, "AxvsMsdaLayerParams")) != AXVS_OK)
    return rc;
  if ((rc = md_setup(c, m, s, x, false, saved, saved_bytes, scratch, scratch_bytes, stream)) != AXVS_OK) return rc;
  return md_forward(c, m, x, src, pos, reference_points, padding_mask, out, *params, s, p_dropout, p_attn_drop, seed);
}
int axvs_msda_layer_train_bwd(const float* d_out, const float* src, const float* pos, const float* reference_points, int ref_dim,
                              const unsigned char* padding_mask, const int* spatial_shapes, const AxvsMsdaLayerParams* params,
                              const AxvsMsdaLayerGrads* grads, float* d_src, float* d_pos, int N, int S, int C, int heads, int L, int P, int d_ffn,
                              float p_dropout, float p_attn_drop, unsigned seed, int recompute, void* saved, size_t saved_bytes, void* scratch,
                              size_t scratch_bytes, void* stream) {
  if (!d_out || !src || !reference_points || !spatial_shapes || !params || !grads || !d_src || !saved || !scratch) return fail(AXVS_ERR_ARG, "null pointer");
  if (d_pos && !pos) return fail(AXVS_ERR_ARG, "d_pos wanted without pos");
  if (int rc = check_drop(p_dropout, p_attn_drop)) return rc;
  MdShape m;
  Ctx c{};
  MdSaved s;
  MdScratch x;
  int rc;
  if ((rc = make_md_shape(m, N, S, C, heads, L, P, d_ffn)) != AXVS_OK || (rc = md_levels(m, ref_dim, spatial_shapes)) != AXVS_OK ||
      (rc = check_ptrs(params, "AxvsMsdaLayerParams")) != AXVS_OK || (rc = check_ptrs(grads, "AxvsMsdaLayerGrads")) != AXVS_OK)
    return rc;
  if ((rc = md_setup(c, m, s, x, true, saved, saved_bytes, scratch, scratch_bytes, stream)) != AXVS_OK) return rc;
  if (recompute) {   // rebuild the activations from (src, pos, seed)
    if ((rc = md_forward(c, m, x, src, pos, reference_points, padding_mask, c.sc.g0, *params, s, p_dropout, p_attn_drop, seed)) != AXVS_OK) return rc;
  }
  return md_backward(c, m, x, d_out, src, pos, reference_points, padding_mask, *params, *grads, d_src, d_pos, s, p_dropout, p_attn_drop, seed);
}
// ---- cross-clip tracking module, training tier (axvs_cc_train_host.h) ---------------------------------------------------------------
size_t axvs_cc_module_train_saved_bytes(const AxvsCCTrainCfg* cfg) {
  CCShape s;
  if (make_cc_shape(s, cfg) != AXVS_OK) return 0;
  Carver b(nullptr);
  carve_cc_saved(b, s);
  return b.off;
}

size_t axvs_cc_module_train_scratch_bytes(const AxvsCCTrainCfg* cfg, int backward) {
  CCShape s;
  if (make_cc_shape(s, cfg) != AXVS_OK) return 0;
  Carver b(nullptr);
  carve_scratch(b, s.d, backward != 0);
  carve_cc_scratch(b, s, backward != 0);
  return b.off;
}

size_t axvs_cc_module_train_bn_stats_floats(const AxvsCCTrainCfg* cfg) {
  CCShape s;
  if (make_cc_shape(s, cfg) != AXVS_OK) return 0;
  return (size_t)s.nl * (4 * kCcC + 2 * kCcCm + 2);
}

int axvs_cc_module_train_fwd(const float* clip_query, const float* panoptic_features, float* pred_logits, float* pred_masks, float* bn_stats,
                             const AxvsCCLayerParams* layers, const AxvsCCHeadParams* heads, const AxvsCCTrainCfg* cfg, void* saved,
                             size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream) {
  if (!clip_query || !panoptic_features || !pred_logits || !pred_masks || !bn_stats || !layers || !heads || !cfg || !saved || !scratch)
    return fail(AXVS_ERR_ARG, "null pointer");
  CCCtx k{};
  CCSaved sv;
  int rc;
  if ((rc = cc_setup(k, cfg, scratch, scratch_bytes, saved, saved_bytes, sv, false, stream)) != AXVS_OK) return rc;
  for (int l = 0; l < k.s.nl; ++l)
    if ((rc = check_ptrs(&layers[l], "AxvsCCLayerParams")) != AXVS_OK) return rc;
  if ((rc = check_ptrs(heads, "AxvsCCHeadParams")) != AXVS_OK) return rc;
  return cc_forward(k, clip_query, panoptic_features, pred_logits, pred_masks, bn_stats, layers, *heads, sv);
}

int axvs_cc_module_train_bwd(const float* d_logits, const float* d_masks, const float* clip_query, const float* panoptic_features,
                             const AxvsCCLayerParams* layers, const AxvsCCHeadParams* heads, const AxvsCCLayerGrads* layer_grads,
                             const AxvsCCHeadGrads* head_grads, float* d_clip_query, const AxvsCCTrainCfg* cfg, void* saved, size_t saved_bytes,
                             void* scratch, size_t scratch_bytes, void* stream) {
  if (!d_logits || !d_masks || !clip_query || !panoptic_features || !layers || !heads || !layer_grads || !head_grads || !d_clip_query || !cfg ||
      !saved || !scratch)
    return fail(AXVS_ERR_ARG, "null pointer");
  CCCtx k{};
  CCSaved sv;
  int rc;
  if ((rc = cc_setup(k, cfg, scratch, scratch_bytes, saved, saved_bytes, sv, true, stream)) != AXVS_OK) return rc;
  for (int l = 0; l < k.s.nl; ++l) {
    if ((rc = check_ptrs(&layers[l], "AxvsCCLayerParams")) != AXVS_OK) return rc;
    if ((rc = check_ptrs(&layer_grads[l], "AxvsCCLayerGrads")) != AXVS_OK) return rc;
  }
  if ((rc = check_ptrs(heads, "AxvsCCHeadParams")) != AXVS_OK) return rc;
  if ((rc = check_ptrs(head_grads, "AxvsCCHeadGrads")) != AXVS_OK) return rc;
  return cc_backward(k, d_logits, d_masks, clip_query, panoptic_features, layers, *heads, layer_grads, *head_grads, d_clip_query, sv);
}

// ---- the layer chain of the cross-clip modules alone (the Tube-Link head trains its own prediction heads around it) -----------------
int axvs_cc_layers_train_fwd(const float* clip_query, float* out_queries, const AxvsCCLayerParams* layers, const AxvsCCTrainCfg* cfg, void* saved,
                             size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream) {
  if (!clip_query || !out_queries || !layers || !cfg || !saved || !scratch) return fail(AXVS_ERR_ARG, "null pointer");
  CCCtx k{};
  CCSaved sv;
  int rc;
  if ((rc = cc_setup(k, cfg, scratch, scratch_bytes, saved, saved_bytes, sv, false, stream)) != AXVS_OK) return rc;
  for (int l = 0; l < k.s.nl; ++l)
    if ((rc = check_ptrs(&layers[l], "AxvsCCLayerParams")) != AXVS_OK) return rc;
  if ((rc = cc_chain_forward(k, clip_query, layers, sv)) != AXVS_OK) return rc;
  const size_t n = (size_t)k.s.nl * k.s.M * kCcC;
  if (hipMemcpyAsync(out_queries, sv.x2, n * sizeof(float), hipMemcpyDeviceToDevice, k.st) != hipSuccess) return fail(AXVS_ERR_LAUNCH, "hipMemcpyAsync failed");
  return last_launch_status();
}

int axvs_cc_layers_train_bwd(const float* d_queries, const float* clip_query, const AxvsCCLayerParams* layers, const AxvsCCLayerGrads* layer_grads,
                             float* d_clip_query, const AxvsCCTrainCfg* cfg, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes,
                             void* stream) {
  if (!d_queries || !clip_query || !layers || !layer_grads || !d_clip_query || !cfg || !saved || !scratch) return fail(AXVS_ERR_ARG, "null pointer");
  CCCtx k{};
  CCSaved sv;
  int rc;
  if ((rc = cc_setup(k, cfg, scratch, scratch_bytes, saved, saved_bytes, sv, true, stream)) != AXVS_OK) return rc;
  for (int l = 0; l < k.s.nl; ++l) {
    if ((rc = check_ptrs(&layers[l], "AxvsCCLayerParams")) != AXVS_OK) return rc;
    if ((rc = check_ptrs(&layer_grads[l], "AxvsCCLayerGrads")) != AXVS_OK) return rc;
  }
  const size_t n = (size_t)k.s.nl * k.s.M * kCcC;            // the chain adds the next layer's input gradient into this buffer
  if (hipMemcpyAsync(k.x.dx2h, d_queries, n * sizeof(float), hipMemcpyDeviceToDevice, k.st) != hipSuccess) return fail(AXVS_ERR_LAUNCH, "hipMemcpyAsync failed");
  return cc_chain_backward(k, clip_query, layers, layer_grads, d_clip_query, sv);
}

// ---- the Tube-Link cross-clip head's prediction heads (axvs_cc_train_host.h) -----------------------------------------------------------
size_t axvs_tl_heads_train_saved_bytes(const AxvsTLHeadTrainCfg* cfg) {
  TLHShape s;
  if (make_tlh_shape(s, cfg) != AXVS_OK) return 0;
  Carver b(nullptr);
  carve_tlh_saved(b, s);
  return b.off;
}

size_t axvs_tl_heads_train_scratch_bytes(const AxvsTLHeadTrainCfg* cfg, int backward) {
  TLHShape s;
  if (make_tlh_shape(s, cfg) != AXVS_OK) return 0;
  Carver b(nullptr);
  Scratch sc{};
  carve_tlh_scratch(b, s, backward != 0, &sc);
  return b.off;
}

int axvs_tl_heads_train_fwd(const float* queries, const float* mask_feature, float* cls_logits, float* mask_logits, const AxvsTLHeadParams* params,
                            const AxvsTLHeadTrainCfg* cfg, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream) {
  if (!queries || !mask_feature || !cls_logits || !mask_logits || !params || !cfg || !saved || !scratch) return fail(AXVS_ERR_ARG, "null pointer");
  Ctx c{};
  TLHShape s;
  TLHSaved sv;
  TLHScratch x;
  int rc;
  if ((rc = check_ptrs(params, "AxvsTLHeadParams")) != AXVS_OK) return rc;
  if ((rc = tlh_setup(c, s, sv, x, cfg, saved, saved_bytes, scratch, scratch_bytes, false, stream)) != AXVS_OK) return rc;
  return tlh_forward(c, s, queries, mask_feature, cls_logits, mask_logits, *params, sv, x);
}

int axvs_tl_heads_train_bwd(const float* d_cls, const float* d_masks, const float* queries, const float* mask_feature, const AxvsTLHeadParams* params,
                            const AxvsTLHeadGrads* grads, float* d_queries, float* d_mask_feature, const AxvsTLHeadTrainCfg* cfg, void* saved,
                            size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream) {
  if (!d_cls || !d_masks || !queries || !mask_feature || !params || !grads || !d_queries || !cfg || !saved || !scratch)
    return fail(AXVS_ERR_ARG, "null pointer");
  Ctx c{};
  TLHShape s;
  TLHSaved sv;
  TLHScratch x;
  int rc;
  if ((rc = check_ptrs(params, "AxvsTLHeadParams")) != AXVS_OK) return rc;
  if ((rc = check_ptrs(grads, "AxvsTLHeadGrads")) != AXVS_OK) return rc;
  if ((rc = tlh_setup(c, s, sv, x, cfg, saved, saved_bytes, scratch, scratch_bytes, true, stream)) != AXVS_OK) return rc;
  return tlh_backward(c, s, d_cls, d_masks, queries, mask_feature, *params, *grads, d_queries, d_mask_feature, sv, x);
}

// ---- 1x1 convolution + GroupNorm, train() mode (WC/msdeformattn.py:349-375 under autograd) ----
size_t axvs_conv1x1_gn_train_saved_bytes(int N, int HW, int Cin, int Cout, int groups, int in_layout, long long in_batch_stride, long long in_ld) {
  Carver sv(nullptr), sc(nullptr);
  const bool copy_x = in_layout == 0 || !(in_ld == Cin && in_batch_stride == (long long)HW * Cin);
  carve_convgn(sv, sc, N, HW, Cin, Cout, groups, copy_x, false, false);
  return sv.off;
}
size_t axvs_conv1x1_gn_train_scratch_bytes(int N, int HW, int Cin, int Cout, int groups, int backward) {
  Carver sv(nullptr), sc(nullptr);
  carve_convgn(sv, sc, N, HW, Cin, Cout, groups, true, backward != 0, true);
  return sc.off;
}

int axvs_conv1x1_gn_train_fwd(const float* x, int in_layout, long long in_batch_stride, long long in_ld, float* out, int out_layout,
                              long long out_batch_stride, long long out_ld, const AxvsConvGnParams* p, int N, int HW, int Cin, int Cout, int groups,
                              float eps, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream) {
  if (!x || !out || !p || !p->conv_w || !p->conv_b || !p->gn_w || !p->gn_b || !saved || !scratch) return fail(AXVS_ERR_ARG, "null pointer");
  if (int rc = convgn_check(N, HW, Cin, Cout, groups, in_layout, out_layout, in_batch_stride, in_ld, out_batch_stride, out_ld)) return rc;
  const bool copy_x = in_layout == 0 || !(in_ld == Cin && in_batch_stride == (long long)HW * Cin);
  Carver sv(saved), sc(scratch);
  const ConvGnBufs b = carve_convgn(sv, sc, N, HW, Cin, Cout, groups, copy_x, false, out_layout == 0);
  Ctx c{};
  if (int rc = train_begin(c, sv, saved_bytes, sc, scratch_bytes, stream)) return rc;
  hipStream_t st = c.st;
  const long long M = (long long)N * HW;
  const int nblk = (HW + 63) / 64;
  const float* xt = x;
  if (in_layout == 0) {
    nchw_to_rows(x, b.xt, N, Cin, HW, st);
    xt = b.xt;
  } else if (copy_x) {
    const long long t4 = M * Cin / 4;
    hipLaunchKernelGGL(gt_gather_tokens_kernel, dim3(blocks((size_t)t4)), dim3(256), 0, st, x, b.xt, HW, Cin, in_batch_stride, in_ld, t4);
    xt = b.xt;
  }
  // y = x W^T + b: three bf16 pieces per operand (fp32 accuracy: the GroupNorm statistics are formed on it)
  GemmEpi e{p->conv_b, 1.f, 0, Drop{0u, 0u, 0u, 1.f}, 0.f};
  if (int rc = c.g.fwd(xt, p->conv_w, b.y, M, Cout, Cin, 0.f, &e, true)) return rc;
  hipLaunchKernelGGL((gt_block_colsums_kernel<0>), dim3((unsigned)nblk, (unsigned)N), dim3(256), 0, st, (const float*)b.y, (const float*)nullptr, (const float*)nullptr, b.part,
                     HW, Cout, groups);
  hipLaunchKernelGGL(gt_merge_blocks_kernel, dim3(blocks((size_t)N * Cout)), dim3(256), 0, st, (const float*)b.part, b.ab, nblk, Cout, HW, (long long)N * Cout);
  hipLaunchKernelGGL(gt_group_stats_kernel, dim3(blocks((size_t)N * groups)), dim3(256), 0, st, (const float*)b.ab, b.stats, Cout, groups, HW, eps, N * groups);
  const long long t4 = M * Cout / 4;
  if (out_layout == 1) {
    hipLaunchKernelGGL(gt_gn_apply_kernel, dim3(blocks((size_t)t4)), dim3(256), 0, st, (const float*)b.y, (const float*)b.stats, p->gn_w, p->gn_b, out, HW, Cout, groups,
                       out_batch_stride, out_ld, t4);
  } else {
    hipLaunchKernelGGL(gt_gn_apply_kernel, dim3(blocks((size_t)t4)), dim3(256), 0, st, (const float*)b.y, (const float*)b.stats, p->gn_w, p->gn_b, b.otok, HW, Cout, groups,
                       (long long)HW * Cout, (long long)Cout, t4);
    rows_to_nchw(b.otok, out, N, Cout, HW, st);
  }
  return last_launch_status();
}

/* d_out in the forward's out layout; x as in the forward (read only when it was contiguous token rows: otherwise the saved copy is used); grads: every
 * buffer is written; d_x (nullable) in the forward's in layout. */
int axvs_conv1x1_gn_train_bwd(const float* d_out, int out_layout, long long out_batch_stride, long long out_ld, const float* x, int in_layout,
                              long long in_batch_stride, long long in_ld, const AxvsConvGnParams* p, const AxvsConvGnGrads* grads, float* d_x, int N, int HW,
                              int Cin, int Cout, int groups, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream) {
  if (!d_out || !x || !p || !p->conv_w || !p->gn_w || !grads || !grads->conv_w || !grads->conv_b || !grads->gn_w || !grads->gn_b || !saved || !scratch)
    return fail(AXVS_ERR_ARG, "null pointer");
  if (int rc = convgn_check(N, HW, Cin, Cout, groups, in_layout, out_layout, in_batch_stride, in_ld, out_batch_stride, out_ld)) return rc;
  const bool copy_x = in_layout == 0 || !(in_ld == Cin && in_batch_stride == (long long)HW * Cin);
  Carver sv(saved), sc(scratch);
  const ConvGnBufs b = carve_convgn(sv, sc, N, HW, Cin, Cout, groups, copy_x, true, out_layout == 0);
  Ctx c{};
  if (int rc = train_begin(c, sv, saved_bytes, sc, scratch_bytes, stream)) return rc;
  c.sc.wpart = b.wpart; c.sc.part_a = b.part_a; c.sc.wt = b.wt;
  hipStream_t st = c.st;
  const long long M = (long long)N * HW;
  const int nblk = (HW + 63) / 64;
  const float* xt = copy_x ? b.xt : x;
  // d_out -> contiguous token rows (they are overwritten with d_y below)
  if (out_layout == 0) {
    nchw_to_rows(d_out, b.dy, N, Cout, HW, st);
  } else {
    const long long t4 = M * Cout / 4;
    hipLaunchKernelGGL(gt_gather_tokens_kernel, dim3(blocks((size_t)t4)), dim3(256), 0, st, d_out, b.dy, HW, Cout, out_batch_stride, out_ld, t4);
  }
  hipLaunchKernelGGL((gt_block_colsums_kernel<1>), dim3((unsigned)nblk, (unsigned)N), dim3(256), 0, st, (const float*)b.dy, (const float*)b.y, (const float*)b.stats, b.part,
                     HW, Cout, groups);
  hipLaunchKernelGGL(gt_sum_blocks_kernel, dim3(blocks((size_t)N * Cout)), dim3(256), 0, st, (const float*)b.part, b.ab, nblk, Cout, (long long)N * Cout);
  hipLaunchKernelGGL(gt_gn_bwd_params_kernel, dim3(blocks((size_t)Cout)), dim3(256), 0, st, (const float*)b.ab, grads->gn_w, grads->gn_b, N, Cout);
  hipLaunchKernelGGL(gt_gn_bwd_groups_kernel, dim3(blocks((size_t)N * groups)), dim3(256), 0, st, (const float*)b.ab, p->gn_w, b.S, Cout, groups, N * groups);
  const long long t4 = M * Cout / 4;
  hipLaunchKernelGGL(gt_gn_bwd_apply_kernel, dim3(blocks((size_t)t4)), dim3(256), 0, st, b.dy, (const float*)b.y, (const float*)b.stats, (const float*)b.S, p->gn_w, HW, Cout,
                     groups, (float)(1.0 / ((double)HW * (Cout / groups))), t4);
  // d_W = d_y^T x, d_b = column sums of d_y (same launch), d_x = d_y W
  if (int rc = c.wgrad(b.dy, xt, grads->conv_w, M, Cout, Cin, grads->conv_b)) return rc;
  if (d_x != nullptr) {
    float* dxt = (in_layout == 1 && !copy_x) ? d_x : b.dxt;
    // three-piece operands: where a level passes through no layer between two projections (the temporal-only decoder's res3) this gradient feeds the GroupNorm
    // backward of the projection in front of it, whose bias gradient is a sum that cancels analytically (the second GroupNorm removes a constant shift)
    if (int rc = c.dgrad(b.dy, p->conv_w, dxt, M, Cout, Cin, 0.f, 0, true)) return rc;
    if (in_layout == 0) {
      rows_to_nchw(dxt, d_x, N, Cin, HW, st);
    } else if (copy_x) {      // strided token rows: scatter back through the apply kernel's addressing (identity statistics)
      return fail(AXVS_ERR_ARG, "conv1x1 + GroupNorm backward: an input gradient in strided token rows is not built (pass contiguous rows or NCHW)");
    }
  }
  return last_launch_status();
}

// the Ctx scratch one test call uses: wpart and the bias partials part_a (weight gradient), wt (input gradient)
static void carve_test_gemm(Carver& b, const AxvsTestGemm& t, Scratch& sc) {
  if (t.op == AXVS_TEST_GEMM_WGRAD) {
    sc.wpart = b.f((size_t)(Gemm::kSplit + 1) * t.N * t.K);
    sc.part_a = b.f((size_t)Gemm::kSplit * t.N);
  } else if (t.op == AXVS_TEST_GEMM_DGRAD) {
    sc.wt = b.f((size_t)t.N * t.K);
  }
}

// ---- test hooks: one call of the GEMM dispatch (axvs_train_host.h, include/axvs.h) --------------------------------------------------------------
size_t axvs_test_train_gemm_scratch_bytes(const AxvsTestGemm* t) {
  if (!t) return 0;
  Carver b(nullptr);
  Scratch sc{};
  carve_test_gemm(b, *t, sc);
  return b.off;
}

int axvs_test_train_gemm(AxvsTestGemm* t, void* scratch, void* stream) {
  if (!t || !t->a || !t->b || !t->c) return fail(AXVS_ERR_ARG, "null pointer");
  t->variant = 0;
  if (t->M <= 0 || t->N <= 0 || t->K <= 0) return fail(AXVS_ERR_ARG, "non-positive dimension");
  GemmLd ld{t->lda, t->ldb, t->ldc, t->ksteps, t->a2};
  ld.al_a = t->al_a; ld.al_b = t->al_b; ld.al_c = t->al_c;
  ld.aff = t->aff; ld.aff_rows = t->aff_rows;
  GemmEpi e{t->bias, t->mul, t->relu, Drop{t->drop_seed, t->drop_site, t->drop_thr, t->drop_scale}, t->beta};
  e.res = t->res; e.res2 = t->res2;
  e.out16 = t->out16; e.kind16 = t->kind16; e.zero_rows = t->zero_rows;
  GemmLd stat{0, 0, 0, 0};
  stat.stat_part = t->stat_part; stat.stat_shift = t->stat_shift; stat.stat_nblk = t->stat_nblk; stat.stat_blk0 = t->stat_blk0;
  stat.stat_rows = t->stat_rows;
  const bool gelu = t->relu > 1;      // (NT, FWD) the GELU epilogues: their own instantiation, which exists for three pieces (exact) only
  // the host-side refusals first: they need no device
  int rc;
  switch (t->op) {
    case AXVS_TEST_GEMM_NT: rc = Gemm::check_nt(t->N, t->K, ld, e, t->exact != 0, gelu); break;
    case AXVS_TEST_GEMM_FWD: rc = Gemm::check_nt(t->N, t->K, GemmLd{t->K, t->K, t->N, 0, t->a2}, e, t->exact != 0, gelu); break;
    case AXVS_TEST_GEMM_WGRAD: rc = Gemm::check_wgrad(t->N, t->K, t->lda ? t->lda : t->N, t->ldb ? t->ldb : t->K); break;
    case AXVS_TEST_GEMM_DGRAD: rc = Gemm::check_nt(t->K, t->N, GemmLd{t->lda ? t->lda : t->N, t->N, t->K, 0}, GemmEpi{}, t->exact != 0 || g_train_exact >= 2); break;
    case AXVS_TEST_GEMM_TN_DIRECT:
      if (t->M > INT32_MAX) return fail(AXVS_ERR_ARG, "einsum GEMM: Mc=%lld rows > 2^31 - 1", t->M);
      rc = Gemm::check_tn(t->N, t->lda, t->stat_part != nullptr, t->grp_rows);
      break;
    default: return fail(AXVS_ERR_ARG, "test GEMM: unknown op %d", t->op);
  }
  if (rc) return rc;
  if ((t->op == AXVS_TEST_GEMM_WGRAD || t->op == AXVS_TEST_GEMM_DGRAD) && !scratch) return fail(AXVS_ERR_ARG, "null scratch");
  Ctx c{};
  c.st = static_cast<hipStream_t>(stream);
  if ((rc = c.g.init(c.st))) return rc;
  Carver b(scratch);
  carve_test_gemm(b, *t, c.sc);
  t_gemm_variant = 0;
  switch (t->op) {
    case AXVS_TEST_GEMM_NT: rc = c.g.nt(t->a, t->b, t->c, t->M, t->N, t->K, ld, e, t->exact != 0, t->zsplits > 0 ? t->zsplits : 1, gelu); break;
    case AXVS_TEST_GEMM_FWD: rc = c.g.fwd(t->a, t->b, t->c, t->M, t->N, t->K, t->beta, &e, t->exact != 0, t->a2, gelu); break;
    case AXVS_TEST_GEMM_WGRAD: rc = c.wgrad(t->a, t->b, t->c, t->M, t->N, t->K, t->db, t->lda, t->ldb, t->mul); break;
    case AXVS_TEST_GEMM_DGRAD:
      rc = c.dgrad(t->a, t->b, t->c, t->M, t->N, t->K, t->beta, t->lda, t->exact != 0, t->mul, t->res, t->res2);
      break;
    default:
      rc = c.g.tn_direct(t->a, t->b, t->c, (int)t->M, t->N, t->K, t->lda, t->ldb, t->ldc, t->al_b, t->al_c, t->stat_part ? &stat : nullptr,
                         t->grp_rows, t->grp_ld);
      break;
  }
  t->variant = t_gemm_variant;
  if (rc) return rc;
  return last_launch_status();
}

}  // extern "C"
