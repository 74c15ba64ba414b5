/* axvs.h -- C-ABI of libaxvs.so: MI355X (gfx950) kernels for the Axial-VS / MaXTron
 * axial-trajectory-attention hot path.
 *
 * Plain pointers and sizes only; no torch types.  Every function is asynchronous on the
 * hipStream_t it is given (passed as void*), never allocates or frees device memory and
 * never synchronises: the caller owns every buffer (inputs, outputs, packed weights,
 * workspace).  Return value 0 = success, negative = error (message: axvs_last_error()).
 *
 * Reference interfaces replaced (paths relative to /root/reference):
 *   WC = MaXTron_Video-kMaX/maxtron_deeplab/modeling/within_clip_tracking_module
 *   CC = MaXTron_Video-kMaX/maxtron_deeplab/modeling/cross_clip_tracking_module
 *   TL = MaXTron_Tube-Link
 *
 * Row-major fp32 tensors use nn.Linear's [out, in] weight layout.  "dtype" selects the
 * 16-bit MFMA operand type (accumulation, softmax, LayerNorm and the residual stream are
 * always fp32): AXVS_F16 meets the 1e-3 parity bar; AXVS_BF16 trades accuracy (about 3e-3)
 * for fp32-like range.
 */
#ifndef AXVS_H
#define AXVS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AXVS_F16 0
#define AXVS_BF16 1
#define AXVS_F32 2  /* fp32 / uint8 (bool) inputs: only where an entry point says so (axvs_video_matcher) */
#define AXVS_U8 3

#define AXVS_OK 0
#define AXVS_ERR_ARG (-1)       /* bad shape / null pointer / unsupported configuration */
#define AXVS_ERR_WORKSPACE (-2) /* workspace too small */
#define AXVS_ERR_LAUNCH (-3)    /* HIP launch failure */
#define AXVS_ERR_STATE (-4)     /* an EARLIER call on this thread's status word reported AXVS_STATUS_SYNC_TIMEOUT (see below) */

/* fp32 parameters of one TrajectoryAttention (WC/temporal_attention.py:21-33,
 * TL/mmdet/models/plugins/msdeformattn_pixel_decoder.py:653-665).  Device pointers.
 * CC flavour (CC/maxtron_cross_clip_tracking_module.py:79-89): the fused qkv Linear is
 * passed as three row slices of qkv.weight / qkv.bias. */
typedef struct AxvsTrajParams {
  const float *q_w, *q_b;         /* [C,C], [C]   */
  const float *k_w, *k_b;         /* [C,C], [C]   */
  const float *v_w, *v_b;         /* [C,C], [C]   */
  const float *proj_q_w, *proj_q_b;   /* [C,C], [C]   */
  const float *proj_kv_w, *proj_kv_b; /* [2C,C], [2C] */
  const float *proj_w, *proj_b;   /* [C,C], [C]   */
} AxvsTrajParams;

/* fp32 parameters of one TemporalAxialTrajectoryAttentionLayer
 * (WC/temporal_attention.py:158-178; TL/...pixel_decoder.py:730-756). */
typedef struct AxvsAxialLayerParams {
  AxvsTrajParams height_attn, width_attn;
  const float *norm1_w, *norm1_b;       /* [C] */
  const float *linear1_w, *linear1_b;   /* [F,C], [F] */
  const float *linear2_w, *linear2_b;   /* [C,F], [C] */
  const float *norm2_w, *norm2_b;       /* [C] */
} AxvsAxialLayerParams;

int axvs_version(void);
/* 1 if the library was built with the bf16 operand tier (-DAXVS_WITH_BF16; not part of the default build since round 6: the tier does not hold the
 * 1e-3 parity bar -- every entry point refuses dtype = AXVS_BF16 with AXVS_ERR_ARG otherwise), else 0 */
int axvs_has_bf16(void);
const char* axvs_last_error(void);

/* Asynchronous condition bits.  The entry points never synchronise, so conditions only a kernel can see are OR-ed into a word
 * the caller registers (per calling thread; NULL disables) and reads back when it likes.  The word may live in device memory
 * or in PINNED HOST memory (hipHostMalloc: device-visible at the same address; the kernels touch it only when a condition
 * fires, so it costs nothing on the normal path -- profiles/r5_pinned_status_probe.txt).  With a host-readable word the
 * library FAILS LOUDLY: every later call of an axial-layer entry point on this thread returns AXVS_ERR_STATE while bit 2 is set
 * (axvs_check_status() reports the same without launching anything).  The Python modules always register a pinned word.
 *   bit 0  AXVS_STATUS_FP16_RANGE: a q/k/v operand of the C = 256 fused kernels (src or src + pos) exceeded the fp16 range
 *          (|x| > 65504) or was NaN -- with f16 MFMA operands the result would silently contain inf / NaN; use AXVS_BF16. */
#define AXVS_STATUS_FP16_RANGE 1
/*   bit 2  AXVS_STATUS_SYNC_TIMEOUT: a workgroup of a merged q/k/v + trajectory launch (axvs_set_sync_buffer) gave up waiting for
 *          its sibling row tiles (~1 s; option "sync_spin_limit" = number of polls): the sync words were not zero at launch, or the
 *          sibling tiles were not scheduled (the hand-off relies on the tiles of a sequence being dispatched in order onto a GPU
 *          that can hold them: true on a whole MI355X, not under CU masking).  The outputs of that call are INVALID and its sync
 *          words are left non-zero: synchronise, zero the words (hipMemset), clear the status word, then call again. */
#define AXVS_STATUS_SYNC_TIMEOUT 4
int axvs_set_status_buffer(int* device_word);
/* 0, or AXVS_ERR_STATE when the registered status word is host-readable and has AXVS_STATUS_SYNC_TIMEOUT set (reads the word as it
 * is: synchronise first to see launches still in flight).  A word in device memory cannot be inspected: returns 0. */
int axvs_check_status(void);

/* Synchronisation words of the ONE-LAUNCH-PER-PASS form of the axial layer (axvs_axial_layer_fwd[_sine3d], axvs_axial_pass_fwd;
 * C = 256, 8 heads, T <= 4, axis lengths up to 96 -- any length since round 5: frames are padded to a multiple of 16 rows in the
 * library's own q/k/v row space, the boundary tensors stay dense).  Reference: WC/temporal_attention.py:197-213 -- the
 * q/k/v Linear layers and the trajectory attention of a pass.  With a buffer registered, the trajectory kernel of a pass computes
 * q, k, v of its own 64 rows itself and the row tiles of one sequence hand K / V^T to each other INSIDE the launch, through one
 * arrival counter per sequence (B*W for the height pass, B*H for the width pass) taken from `device_words`; without one (the
 * default) every pass is a q/k/v launch followed by a trajectory launch.  Both forms give bit-identical results.
 * Contract: `device_words` are n_words 32-bit words of device memory that are ZERO when registered (hipMemset once); every launch
 * leaves them zero again.  One buffer serves one stream at a time: calls that may run concurrently (different streams) need
 * different buffers.  Registration is per calling thread, like the status word; (NULL, 0) unregisters.  A call with more
 * sequences than n_words runs the two-launch form. */
int axvs_set_sync_buffer(unsigned* device_words, size_t n_words);

/* ---- optional per-stage timing of axvs_axial_layer_fwd (used by bench.py; thread-local).
 *      events: array of `capacity` hipEvent_t created by the caller, or NULL to switch off.  While set, the layer
 *      records events[i] on its stream after stage i (events[0] at entry).  Returns the maximum stage count;
 *      after a forward, axvs_profile_stage_count() / _name(i) describe the stages that forward actually ran. */
int axvs_profile_stages(void** events, int capacity);
int axvs_profile_stage_count(void);
const char* axvs_profile_stage_name(int i);

/* ---- options: 15 keys (round 6; rounds 2 - 5 exposed 37, most of them planner thresholds and forms measured slower: those are constants / gone).
 *      Thread-local unless noted.  Unknown keys return AXVS_ERR_ARG.
 *      Set by the host modules around their calls:
 *        "ffn_gelu"            the layer's FFN activation is exact GELU instead of ReLU (activation = "gelu", WC/temporal_attention.py:9-17)
 *        "layer_out_dtype"     0 (default): axvs_axial_layer_fwd* / axvs_axial_pass_fwd(pass = 1) / axvs_traj_layer_fwd / axvs_ffn_fwd write fp32 rows, the reference's
 *                              type; 1 / 2: `out` is a [rows, C] f16 / bf16 map written by the epilogue of the kernel that ends the layer -- the map a batch-sharded
 *                              caller sends over xGMI (BASELINE config 5), without a cast pass; fused FFN tier, contiguous frames only
 *        "cc_aspp_affine"      the ASPP projection of a cross-clip layer is followed by a per-channel scale / shift packed into aspp_norm_w / aspp_norm_b
 *                              (eval-mode SyncBatchNorm, norm_fn = 'syncbn') instead of the channels-first LayerNorm of the shipped configs
 *        "cc_last_heads_only"  axvs_cc_module_fwd computes the predictor heads of the LAST layer only (pred_logits / pred_masks then hold one layer)
 *        "train_amp"           process-wide; 1 / 2: the X W^T GEMMs of the training tier multiply ONE bf16 / fp16 piece per operand (what torch.autocast gives nn.Linear)
 *        "no_merge_qkv"        two launches per axial pass (q/k/v kernel + trajectory kernel) instead of the merged launch with its in-launch hand-off: bit-identical;
 *                              the 'verify' hand-off policy's re-run
 *      Tier selection for parity tests and measurements:
 *        "generic_only", "no_attn_fusion", "no_ffn_fusion"   the shape-generic kernels / separate attention and temporal kernels / the FFN in its own kernel
 *        "merge_qkv_any"       merged launches at every grid size (default: up to ~2 rounds of the chip, or frames of 64 keys)
 *        "spatial_only"        timing: 1 = the fused trajectory kernels return after QK^T / softmax / AV, 2 = the merged kernels after their q/k/v part (outputs unwritten)
 *        "train_valu", "train_exact"   process-wide: VALU instead of fp32-MFMA attention in the training tier; 1 (default) / 0 / 2: three- / two-piece forward GEMMs / three-piece
 *                              input-gradient GEMMs as well
 *      Test hooks:
 *        "sync_spin_limit"     polls before a hand-off wait gives up and sets AXVS_STATUS_SYNC_TIMEOUT (default 2^22, about one second; 0 restores it)
 *        "plan_force"          ONE bit mask that forces the planner's size-dependent choices between forms that are bit-identical by construction (the bit-identity tests):
 *                              1 never the 16-row trajectory tiles | 2 / 4 the 128-row FFN tiles always / never | 8 no two-chunk FFN workgroups |
 *                              16 / 32 merged launch on 16-row tiles never / at any size | 64 generic tier without the reassociated temporal half |
 *                              128 never the regular-tile instantiation of the merged trajectory kernels (the shape-generic one serves every shape); 0 = the planner's own choice */
int axvs_set_option(const char* key, int value);

/* ---- which instantiation the last trajectory passes of this thread ran: bit 0 = the height pass of a layer (or a stand-alone trajectory attention),
 *      bit 1 = the width pass, set when the pass ran the regular-tile instantiation of the merged kernel (whole unpadded 64-key frames; bit-identical
 *      to the shape-generic one, which "plan_force" 128 forces) */
int axvs_plan_regular_tiles(void);

/* ---- weight packing (once per load_state_dict; result is opaque, device-resident: 16-bit operands in MFMA-fragment order,
 *      16 rows x 32 k-values per KiB, so that a wave's fragment load reads consecutive addresses in lane order) ---- */
size_t axvs_traj_packed_bytes(int C, int heads);
int axvs_traj_pack(const AxvsTrajParams* p, void* packed, int C, int heads, int dtype, void* stream);
size_t axvs_axial_layer_packed_bytes(int C, int heads, int d_ffn);
int axvs_axial_layer_pack(const AxvsAxialLayerParams* p, void* packed, int C, int heads, int d_ffn, int dtype,
                          void* stream);

/* ---- TrajectoryAttention.forward(query, key, value, num_frames)
 *      WC/temporal_attention.py:35-76.  query/key/value/out: fp32 [S, T*L, C].
 *      space_attn: NULL or fp32 [(S*heads), T*L, T, L] (the reference's second return value). */
size_t axvs_traj_attn_workspace_bytes(int S, int T, int L, int C, int heads);
int axvs_traj_attn_fwd(const float* query, const float* key, const float* value, float* out, float* space_attn,
                       const void* packed, int S, int T, int L, int C, int heads, int dtype, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- TemporalAxialTrajectoryAttentionLayer.forward(src, pos)
 *      WC/temporal_attention.py:187-220 (TL/...pixel_decoder.py:758-791).
 *      src/out: fp32 [(B*T), (H*W), C]; pos: fp32 [B,T,H,W,C]; out may not alias src.
 *      h_attn: NULL or fp32 [(B*W*heads), T*H, T, H]; w_attn: NULL or fp32 [(B*H*heads), T*W, T, W].
 *      (Tube-Link's `f + gamma * encoder(f)`, TL/...pixel_decoder.py:623-627: axvs_scaled_residual below.) */
size_t axvs_axial_layer_workspace_bytes(int B, int T, int H, int W, int C, int heads, int d_ffn);
int axvs_axial_layer_fwd(const float* src, const float* pos, float* out, const void* packed, int B, int T, int H,
                         int W, int C, int heads, int d_ffn, int dtype, void* workspace, size_t workspace_bytes,
                         float* h_attn, float* w_attn, void* stream);

/* ---- TemporalTrajectoryAttentionLayer.forward(src, pos)  (temporal_attn_type = "trajectory")
 *      WC/temporal_attention.py:103-155: ONE TrajectoryAttention over all T*H*W tokens of a clip (q = k = src + pos, v = src,
 *      frames of H*W keys each), residual, norm1, FFN, norm2.  src/out fp32 [(B*T), HW, C]; pos fp32 [B,T,H,W,C] (= [B, T*HW, C]).
 *      Frames of more than 256 keys take a chunked-key attention kernel with an online softmax (the reference's N x N logits
 *      would be 8.6 GB at 64 x 64).  No attention-map output (the reference returns None, None). */
typedef struct AxvsTrajLayerParams {
  AxvsTrajParams temporal_attn;
  const float *norm1_w, *norm1_b, *linear1_w, *linear1_b, *linear2_w, *linear2_b, *norm2_w, *norm2_b;
} AxvsTrajLayerParams;
size_t axvs_traj_layer_packed_bytes(int C, int heads, int d_ffn);
int axvs_traj_layer_pack(const AxvsTrajLayerParams* p, void* packed, int C, int heads, int d_ffn, int dtype, void* stream);
size_t axvs_traj_layer_workspace_bytes(int B, int T, int HW, int C, int heads, int d_ffn);
int axvs_traj_layer_fwd(const float* src, const float* pos, float* out, const void* packed, int B, int T, int HW, int C, int heads,
                        int d_ffn, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* One axial pass of the layer on a LOCAL block of the token grid -- the building block of off-axis sharding of a single clip over
 * GPUs (SURVEY 8e option ii: the height pass mixes tokens along H only, so it runs on any block of columns; the width pass, norm1,
 * FFN and norm2 run on any block of rows; between the two the blocks are exchanged with one all-to-all):
 *   pass 0: out = src + height_attn(q = k = src + pos, v = src)                     (WC/temporal_attention.py:197-204)
 *   pass 1: out = norm2(FFN(norm1(src + width_attn(q = k = src + pos, v = src))))   (:206-218)
 * src / pos / out: fp32 [B,T,H,W,C] contiguous blocks (pos: the matching block of the full embedding).  Workspace:
 * axvs_axial_layer_workspace_bytes_ex(B,T,H,W,C,heads,d_ffn,0,0). */
int axvs_axial_pass_fwd(const float* src, const float* pos, float* out, const void* packed, int pass, int B, int T, int H, int W,
                        int C, int heads, int d_ffn, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* The same layer with `pos` given as a SPECIFICATION instead of a tensor: pos = PositionEmbeddingSine3D(num_pos_feats = C/2,
 * temperature, normalize, scale)(x, fmt) in channels-last form (WC/pos_embeddings.py:86-130, mask = None) plus an optional
 * per-channel vector (the decoder's level_embed_3d[lvl], WC/msdeformattn.py:112-115).  This is what every caller of the layer
 * in the reference passes; the C = 256 / 8-head kernels then evaluate the embedding inside the q/k loaders instead of reading
 * B*T*H*W*C floats per pass from HBM (other shapes: materialised into the workspace first, same results as axvs_pos3d). */
typedef struct AxvsSinePos3D {
  float temperature;
  int normalize;
  float scale;
  const float* level_embed;   /* NULL or device fp32 [C] */
} AxvsSinePos3D;
/* Exact workspace of one call, by the kernel tier it will take (the fully fused C = 256 tier only round-trips q, k and V^T:
 * ~7x less than the upper bound axvs_axial_layer_workspace_bytes returns).  want_attn_maps: h_attn / w_attn will be non-NULL;
 * sine_pos: the call is axvs_axial_layer_fwd_sine3d.  Depends on axvs_set_option state of the calling thread. */
size_t axvs_axial_layer_workspace_bytes_ex(int B, int T, int H, int W, int C, int heads, int d_ffn, int want_attn_maps,
                                           int sine_pos);
size_t axvs_axial_layer_sine3d_workspace_bytes(int B, int T, int H, int W, int C, int heads, int d_ffn);
int axvs_axial_layer_fwd_sine3d(const float* src, const AxvsSinePos3D* pos, float* out, const void* packed, int B, int T, int H,
                                int W, int C, int heads, int d_ffn, int dtype, void* workspace, size_t workspace_bytes,
                                float* h_attn, float* w_attn, void* stream);

/* ---- the same layer on a [B*T, H*W, C] VIEW whose frames are `frame_stride_rows` rows (of C floats) apart -- one level of the pixel
 *      decoder's concatenated [B*T, sum(H_l W_l), C] token buffer (WC/msdeformattn.py:258-264 splits the levels out, runs the
 *      temporal encoder on each and concatenates them again; here the level is read and written where it lies).  `out` may be
 *      `src` (in place).  Generated positions only, no attention maps; fused tier only (axvs_axial_layer_strided_ok). */
int axvs_axial_layer_strided_ok(int C, int heads, int d_ffn);
size_t axvs_axial_layer_workspace_bytes_strided(int B, int T, int H, int W, int C, int heads, int d_ffn, long long frame_stride_rows);
int axvs_axial_layer_fwd_sine3d_strided(const float* src, const AxvsSinePos3D* pos, float* out, const void* packed, int B, int T, int H,
                                        int W, int C, int heads, int d_ffn, int dtype, long long frame_stride_rows, void* workspace,
                                        size_t workspace_bytes, void* stream);

/* ---- the layer's feed-forward tail alone: out = norm2(y + linear2(relu(linear1(y)))), y = norm1(x)
 *      WC/temporal_attention.py:181-185 + :217.  x/out fp32 [M, C]; weights from a packed AxvsAxialLayerParams. */
size_t axvs_ffn_workspace_bytes(long long M, int C, int d_ffn);
int axvs_ffn_fwd(const float* x, float* out, const void* packed_layer, long long M, int C, int heads, int d_ffn,
                 int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* ---- The same feed-forward tail from its own four parameter pairs: mmcv BaseTransformerLayer with operation_order
 *      ('self_attn', 'norm', 'ffn', 'norm') after the attention, as in every layer of Tube-Link's MSDeformAttnPixelDecoder encoder
 *      (TL/mmdet/models/plugins/msdeformattn_pixel_decoder.py:63-88): norms[0] -> ffns[0] (x + fc2(relu(fc1(x))), mmcv FFN with
 *      add_identity) -> norms[1], LayerNorm eps 1e-5.  norm1 / norm2 = norms[0] / norms[1], linear1 / linear2 = ffns[0].layers[0][0] /
 *      ffns[0].layers[1].  x / out fp32 [M, C] (out may be x: x is copied first); C a multiple of 32; workspace axvs_ffn_workspace_bytes(M, C, d_ffn). */
typedef struct AxvsFfnParams {
  const float *norm1_w, *norm1_b;       /* [C] */
  const float *linear1_w, *linear1_b;   /* [F,C], [F] */
  const float *linear2_w, *linear2_b;   /* [C,F], [C] */
  const float *norm2_w, *norm2_b;       /* [C] */
} AxvsFfnParams;
size_t axvs_ffn_packed_bytes(int C, int d_ffn);
int axvs_ffn_pack(const AxvsFfnParams* p, void* packed, int C, int d_ffn, int dtype, void* stream);
int axvs_ffn_packed_fwd(const float* x, float* out, const void* packed_ffn, long long M, int C, int d_ffn, int dtype, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- FPN tail of Tube-Link's MSDeformAttnPixelDecoder for one level the encoder does not see (TL:311-325, stride 4 in every
 *      shipped config), lateral_convs[i] / output_convs[i] ConvModules with GroupNorm and no conv bias (use_bias = norm_cfg is None, TL:136):
 *        m = GN(conv1x1(x)) + F.interpolate(up, size = (H, W), mode = 'bilinear', align_corners = False)      TL:313-318
 *        c = ReLU(GN(conv3x3(m, padding = 1)))                                                                  TL:319
 *        mask_feature = conv1x1(c) + bias  (the mask_feature Conv2d, TL:324; only for the last level)
 *      x: backbone map, NCHW fp32 [N, Cin, H, W].  up: the next-coarser level's output as fp32 token rows, row (n, y*Wu + x) at
 *      up + n*up_batch_stride + (y*Wu + x)*up_ld (a level slice of the encoder's [N, S, C] buffer, read where it lies; any size ratio).
 *      y (NULL: not written): ReLU(GN(conv3x3(m))) as fp32 token rows [N, H*W, C].  mask_feature (NULL: not computed): NCHW fp32
 *      [N, Cm, H, W].  m is stored once as f16 channels-last rows (the 3x3 conv's operand type); the 3x3 conv is an implicit GEMM on
 *      16x16x32 f16 (bf16) MFMAs with fp32 accumulation, writes fp32 rows and per-tile partial sums; the GroupNorm statistics are reduced in
 *      a fixed order (bit-identical run to run); the mask_feature GEMM normalises c in its operand loader.
 *      Bounds: H, W, Hu, Wu >= 1; Cin, C multiples of 32 (C <= 4096); Cm a multiple of 32 (0: the pack holds no mask_feature weights);
 *      groups divides C; N <= 65535; N*H*W < 2^31 / 64 (the 32-bit row indices of the GEMMs); up_ld / up_batch_stride multiples of 4, up 16-byte aligned.  Otherwise AXVS_ERR_ARG. */
typedef struct AxvsFpnLevelParams {
  const float* lateral_w;                        /* lateral_convs[i].conv.weight [C, Cin, 1, 1] */
  const float *lateral_gn_w, *lateral_gn_b;      /* lateral_convs[i].gn [C] */
  const float* output_w;                         /* output_convs[i].conv.weight [C, C, 3, 3] */
  const float *output_gn_w, *output_gn_b;        /* output_convs[i].gn [C] */
  const float *mask_w, *mask_b;                  /* mask_feature [Cm, C, 1, 1], [Cm]; may be NULL when Cm = 0 */
} AxvsFpnLevelParams;
size_t axvs_fpn_level_packed_bytes(int Cin, int C, int Cm);
int axvs_fpn_level_pack(const AxvsFpnLevelParams* p, void* packed, int Cin, int C, int Cm, int dtype, void* stream);
size_t axvs_fpn_level_workspace_bytes(int N, int H, int W, int Cin, int C, int groups);
int axvs_fpn_level_fwd(const float* x, const float* up, long long up_batch_stride, long long up_ld, int Hu, int Wu, float* y,
                       float* mask_feature, const void* packed, int N, int H, int W, int Cin, int C, int Cm, int groups, float eps, int dtype,
                       void* workspace, size_t workspace_bytes, void* stream);

/* =====================================================================================================
 * Cross-clip tracking module (CC/maxtron_cross_clip_tracking_module.py), d_model = 256, 8 heads, norm_fn = 'ln'.
 * ===================================================================================================== */
typedef struct AxvsBN { const float *w, *b, *mean, *var; } AxvsBN;   /* eval-mode (Sync)BatchNorm, eps = 1e-3 */

/* one iteration of the layer loop, CC/...:286-297 */
typedef struct AxvsCCLayerParams {
  AxvsTrajParams attn;                    /* TrajectoryAttention (:78-130); qkv passed as three row slices      */
  const float *norm_w, *norm_b;           /* TrajectoryAttentionLayer.norm, LayerNorm eps 1e-5 (:140,:156-161)  */
  const float *aspp_w[3], *aspp_b[3];     /* ASPP._aspp_conv{0,1,2}: Conv1d(256,256,3) weights [256,256,3]      */
  const float *aspp_proj_w;               /* ASPP._proj_conv_bn_act.conv: [256,768,1], no bias                  */
  const float *aspp_norm_w, *aspp_norm_b; /* ... .norm: channels-first LayerNorm eps 1e-6                       */
  const float *conv_norm_w, *conv_norm_b; /* conv_norms[i]: LayerNorm eps 1e-5 (:263,:293-295)                  */
} AxvsCCLayerParams;

size_t axvs_cc_layer_packed_bytes(void);
int axvs_cc_layer_pack(const AxvsCCLayerParams* p, void* packed, int dtype, void* stream);
size_t axvs_cc_layer_workspace_bytes(int B, int Q, int Tc);
/* clip_query / out: fp32 [B, Q, Tc, 256] (out may not alias clip_query); rates: the three atrous rates */
int axvs_cc_layer_fwd(const float* clip_query, float* out, const void* packed, int B, int Q, int Tc, const int* rates,
                      int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* embedding projections + MaXTronCCPredictor (eval branch), CC/...:45-75, :266-270, :300-309 */
typedef struct AxvsCCHeadParams {
  const float* class_proj_w; AxvsBN class_proj_bn;   /* _class_embedding_projection: conv [256,256,1] + BN + GELU */
  const float* mask_proj_w;  AxvsBN mask_proj_bn;    /* _mask_embedding_projection                                */
  const float* mask_head_w;  AxvsBN mask_head_bn;    /* _predictor._transformer_mask_head: conv [128,256,1] + BN  */
  const float *class_head_w, *class_head_b;          /* _predictor._transformer_class_head: [K1,256,1], [K1]      */
  const float *act_head_w, *act_head_b;              /* _predictor._transformer_class_activation_head: [1,256,1]  */
  AxvsBN pixel_bn;                                   /* _predictor._pixel_space_mask_batch_norm (1 channel)       */
} AxvsCCHeadParams;

size_t axvs_cc_heads_packed_bytes(int K1);
int axvs_cc_heads_pack(const AxvsCCHeadParams* p, void* packed, int K1, int dtype, void* stream);
size_t axvs_cc_heads_workspace_bytes(int B, int Q, int Tc);
/* clip_query fp32 [B,Q,Tc,256]; panoptic_features fp32 [B,128,Tc*V,H,W];
 * pred_logits fp32 [1,Q,K1] (softmax pooling runs over all B*Tc entries, like the reference's dim-0 softmax);
 * pred_masks fp32 [B,Q,Tc*V,H,W] (any V*H*W: rows of pixels may start at any 4-byte boundary). */
int axvs_cc_heads_fwd(const float* clip_query, const float* panoptic_features, float* pred_logits, float* pred_masks,
                      const void* packed, int B, int Q, int Tc, int V, int H, int W, int K1, int dtype, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- Tube-Link flavour of the cross-clip heads.  The cross-clip layers themselves are axvs_cc_layer_*:
 *      TL/models/video/tube_link_vis/mask2former_video_cc_head.py:927-946 is the same computation as CC/...:286-297.
 *      Replaces forward_head_clips (:761-781) + pred_class (:783-797) for ONE decoder layer's output. */
typedef struct AxvsTLHeadParams {
  const float *post_norm_w, *post_norm_b;               /* transformer_decoder.post_norm: LayerNorm(256), eps 1e-5 (:767) */
  const float *activation_proj_w, *activation_proj_b;   /* Linear(256,1) (:394, :791)                                      */
  const float *cls_embed_w, *cls_embed_b;               /* Linear(256,K1) (:365, :796)                                     */
  const float* mask_embed_w[3];                         /* Linear(256,256), Linear(256,256), Linear(256,Cm) (:368-371)     */
  const float* mask_embed_b[3];
} AxvsTLHeadParams;

size_t axvs_tl_heads_packed_bytes(int K1, int Cm);
int axvs_tl_heads_pack(const AxvsTLHeadParams* p, void* packed, int K1, int Cm, int dtype, void* stream);
size_t axvs_tl_heads_workspace_bytes(int B, int Q, int Tc, int Cm);
/* clip_query fp32 [B,Q,Tc,256] (a cross-clip layer's output, axvs_cc_layer_fwd layout); mask_feature fp32 [B,Tc*fpc,Cm,h,w];
 * cls_logits fp32 [B,Q,K1]; mask_logits fp32 [B,Tc*fpc,Q,h,w].  Cm in {128,256}; any h*w. */
int axvs_tl_heads_fwd(const float* clip_query, const float* mask_feature, float* cls_logits, float* mask_logits,
                      const void* packed, int B, int Q, int Tc, int frames_per_clip, int h, int w, int K1, int Cm, int dtype,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- The whole layer loop of the cross-clip modules in one call: CrossClipTrackingModule.forward's loop
 *      (CC/maxtron_cross_clip_tracking_module.py:283-318) and Tube-Link's (TLCC:925-950 + forward_head_clips :761-781 + pred_class
 *      :783-797).  packed_layers: HOST array of num_layers device pointers (axvs_cc_layer_pack); packed_heads: axvs_cc_heads_pack /
 *      axvs_tl_heads_pack.  Outputs for EVERY layer (the reference collects them for aux_outputs): pred_logits fp32
 *      [num_layers][1 | B][Q][K1], pred_masks fp32 [num_layers][...one layer's mask tensor...]; last_query fp32 [B,Q,Tc,256].
 *      The layer chain runs first; the predictor heads share their weights across layers, so the class logits and mask kernels
 *      of all layers are one launch per GEMM and the mask einsum reads the pixel features once for all layers.  */
size_t axvs_cc_module_workspace_bytes(int B, int Q, int Tc, int num_layers);
int axvs_cc_module_fwd(const float* clip_query, const float* panoptic_features, float* pred_logits, float* pred_masks,
                       float* last_query, const void* const* packed_layers, const void* packed_heads, int num_layers, int B,
                       int Q, int Tc, int V, int H, int W, int K1, const int* rates, int dtype, void* workspace,
                       size_t workspace_bytes, void* stream);
size_t axvs_tl_cc_module_workspace_bytes(int B, int Q, int Tc, int Cm, int num_layers);
int axvs_tl_cc_module_fwd(const float* clip_query, const float* mask_feature, float* cls_logits, float* mask_logits,
                          float* last_query, const void* const* packed_layers, const void* packed_heads, int num_layers, int B,
                          int Q, int Tc, int frames_per_clip, int h, int w, int K1, int Cm, const int* rates, int dtype,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- Multi-scale deformable attention forward.
 *      OPS = MaXTron_Video-kMaX/maxtron_deeplab/modeling/within_clip_tracking_module/ops
 *      axvs_msda_fwd  replaces MSDeformAttn.forward (OPS/modules/ms_deform_attn.py:81-125): value_proj (+ padding mask),
 *      sampling_offsets, attention_weights + softmax, sampling locations, the gather, output_proj.
 *      axvs_msda_core_fwd replaces the native op ms_deform_attn_forward (OPS/src/ms_deform_attn.h:24-47,
 *      OPS/src/cuda/ms_deform_attn_cuda.cu:21-86) with its fp32 tensors as they are; level_start_index follows from
 *      spatial_shapes and im2col_step has no meaning here. */
typedef struct AxvsMsdaParams {        /* fp32 device pointers, nn.Linear layout [out,in] (OPS/modules/ms_deform_attn.py:59-62) */
  const float *value_proj_w, *value_proj_b;                 /* [C,C], [C]                  */
  const float *sampling_offsets_w, *sampling_offsets_b;     /* [heads*L*P*2, C], [..]      */
  const float *attention_weights_w, *attention_weights_b;   /* [heads*L*P, C], [..]        */
  const float *output_proj_w, *output_proj_b;               /* [C,C], [C]                  */
} AxvsMsdaParams;

size_t axvs_msda_packed_bytes(int C, int heads, int L, int P);
int axvs_msda_pack(const AxvsMsdaParams* p, void* packed, int C, int heads, int L, int P, int dtype, void* stream);
size_t axvs_msda_workspace_bytes(int N, int Lq, int S, int C, int heads, int L, int P);
/* query fp32 [N,Lq,C]; reference_points fp32 [N,Lq,L,ref_dim], ref_dim 2 or 4; input_flatten fp32 [N,S,C];
 * padding_mask: NULL or bytes [N,S], non-zero = padding (value rows zeroed); spatial_shapes: HOST ints [L][2] = (H_l, W_l),
 * sum H_l*W_l == S; out fp32 [N,Lq,C]. */
int axvs_msda_fwd(const float* query, const float* reference_points, int ref_dim, const float* input_flatten,
                  const unsigned char* padding_mask, const int* spatial_shapes, float* out, const void* packed, int N, int Lq,
                  int S, int C, int heads, int L, int P, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* The module in two halves, for the Tube-Link plugin MultiScaleDeformableAxialTrajectoryAttention.forward
 * (TL/mmdet/models/plugins/msdeformattn_pixel_decoder.py:566-638), which runs its temporal encoder on the sampled rows of the
 * coarsest levels BEFORE output_proj (:613-633):
 *   axvs_msda_sample_fwd       :594-611  value_proj(value) (+ key_padding_mask), sampling_offsets / attention_weights of
 *                                        (query + query_pos), softmax, bilinear gather -> sampled fp32 [N,Lq,C]
 *   axvs_msda_output_proj_fwd  :633-638  out = output_proj(x) + identity (identity may be NULL); head_dim 32 only.
 * query_pos: NULL or fp32 [N,Lq,C].  Workspace: axvs_msda_workspace_bytes. */
int axvs_msda_sample_fwd(const float* query, const float* query_pos, const float* reference_points, int ref_dim,
                         const float* value, const unsigned char* padding_mask, const int* spatial_shapes, float* sampled,
                         const void* packed, int N, int Lq, int S, int C, int heads, int L, int P, int dtype, void* workspace,
                         size_t workspace_bytes, void* stream);
int axvs_msda_output_proj_fwd(const float* x, const float* identity, float* out, const void* packed, long long rows, int C,
                              int heads, int L, int P, int dtype, void* stream);
/* MSDeformAttnTransformerEncoderLayer.forward (WC/msdeformattn.py:177-216), eval:
 *   x = norm1(src + MSDeformAttn(src + pos, reference_points, src, ...));  out = norm2(x + linear2(relu(linear1(x)))) */
typedef struct AxvsMsdaLayerParams {
  AxvsMsdaParams self_attn;
  const float *norm1_w, *norm1_b, *linear1_w, *linear1_b, *linear2_w, *linear2_b, *norm2_w, *norm2_b;
} AxvsMsdaLayerParams;
size_t axvs_msda_layer_packed_bytes(int C, int heads, int L, int P, int d_ffn);
int axvs_msda_layer_pack(const AxvsMsdaLayerParams* p, void* packed, int C, int heads, int L, int P, int d_ffn, int dtype,
                         void* stream);
size_t axvs_msda_layer_workspace_bytes(int N, int S, int C, int heads, int L, int P, int d_ffn);
/* src / out fp32 [N,S,C] (out must not alias src); pos fp32 [N,S,C] or NULL; reference_points fp32 [N,S,L,ref_dim] */
int axvs_msda_layer_fwd(const float* src, const float* pos, const float* reference_points, int ref_dim,
                        const unsigned char* padding_mask, const int* spatial_shapes, float* out, const void* packed, int N,
                        int S, int C, int heads, int L, int P, int d_ffn, int dtype, void* workspace, size_t workspace_bytes,
                        void* stream);
/* value fp32 [N,S,M,D]; sampling_loc fp32 [N,Lq,M,L,P,2]; attn_weight fp32 [N,Lq,M,L,P]; out fp32 [N,Lq,M*D] */
int axvs_msda_core_fwd(const float* value, const int* spatial_shapes, const float* sampling_loc, const float* attn_weight,
                       float* out, int N, int S, int M, int D, int Lq, int L, int P, void* stream);
/* backward of the native op: replaces ms_deform_attn_backward (OPS/src/ms_deform_attn.h:49-67, OPS/src/cuda/ms_deform_attn_cuda.cu:
 * 89-157, the ms_deformable_col2im kernels of OPS/src/cuda/ms_deform_im2col_cuda.cuh).  grad_output fp32 [N,Lq,M*D] ->
 * grad_value fp32 [N,S,M,D] (zeroed here, accumulated with atomic adds like the reference: the summation order is not fixed),
 * grad_sampling_loc fp32 [N,Lq,M,L,P,2], grad_attn_weight fp32 [N,Lq,M,L,P] (written; for D not a power of two <= 64 accumulated). */
int axvs_msda_core_bwd(const float* value, const int* spatial_shapes, const float* sampling_loc, const float* attn_weight,
                       const float* grad_output, float* grad_value, float* grad_sampling_loc, float* grad_attn_weight, int N, int S, int M,
                       int D, int Lq, int L, int P, void* stream);

/* ---- Training tier of MSDeformAttnTransformerEncoderLayer: WC/msdeformattn.py:177-216 in train() mode under autograd --
 *      value_proj(src) with the rows of padded keys zeroed, one GEMM for sampling_offsets | attention_weights on src + pos, the
 *      softmax over each (query, head)'s L*P logits and the sampling locations (OPS/modules/ms_deform_attn.py:98-117, both
 *      reference-point forms), the fp32 core op above (forward and backward), output_proj, dropout1 + residual, norm1, FFN, norm2.
 *      fp32 activations, split-precision GEMMs and the counter-based dropout of the trajectory layers' tier (see above).
 *      Dropout sites (element index = the element's offset in the reference's tensor at that site):
 *        7  dropout1 (p_attn_drop), the attention output [N, S, C]        (:210)
 *        8  dropout2 (p_dropout), the FFN hidden [N, S, d_ffn]            (:202)
 *        9  dropout3 (p_dropout), the FFN output [N, S, C]                (:204)
 *      Bounds (the size functions return 0 and axvs_last_error() names the bound): head_dim in {8,16,32,64}, n_levels <= 8,
 *      n_levels * n_points <= 32, n_heads * n_levels * n_points a multiple of 8, d_ffn a multiple of 8, N*S < 2^31.
 *      reference_points are constants: they get no gradient. */
typedef struct AxvsMsdaGrads {        /* same field order as AxvsMsdaParams */
  float *value_proj_w, *value_proj_b, *sampling_offsets_w, *sampling_offsets_b, *attention_weights_w, *attention_weights_b,
      *output_proj_w, *output_proj_b;
} AxvsMsdaGrads;
typedef struct AxvsMsdaLayerGrads {   /* same field order as AxvsMsdaLayerParams; every buffer is WRITTEN (not accumulated) */
  AxvsMsdaGrads self_attn;
  float *norm1_w, *norm1_b, *linear1_w, *linear1_b, *linear2_w, *linear2_b, *norm2_w, *norm2_b;
} AxvsMsdaLayerGrads;
size_t axvs_msda_layer_train_saved_bytes(int N, int S, int C, int heads, int L, int P, int d_ffn);
size_t axvs_msda_layer_train_scratch_bytes(int N, int S, int C, int heads, int L, int P, int d_ffn, int backward);
/* src fp32 [N,S,C]; pos fp32 [N,S,C] or NULL; reference_points fp32 [N,S,L,ref_dim], ref_dim 2 or 4; padding_mask NULL or bytes
 * [N,S] (non-zero = padding); spatial_shapes HOST ints [L][2] = (H_l, W_l), sum H_l*W_l == S; out fp32 [N,S,C]. */
int axvs_msda_layer_train_fwd(const float* src, const float* pos, const float* reference_points, int ref_dim, const unsigned char* padding_mask,
                              const int* spatial_shapes, float* out, const AxvsMsdaLayerParams* params, int N, int S, int C, int heads, int L, int P,
                              int d_ffn, float p_dropout, float p_attn_drop, unsigned seed, void* saved, size_t saved_bytes, void* scratch,
                              size_t scratch_bytes, void* stream);
/* d_out: gradient of `out`.  Writes d_src, d_pos (NULL: not wanted; needs pos) and every buffer of `grads`.  recompute != 0: `saved`
 * is rebuilt from (src, pos, params, seed) first. */
int axvs_msda_layer_train_bwd(const float* d_out, const float* src, const float* pos, const float* reference_points, int ref_dim,
                              const unsigned char* padding_mask, const int* spatial_shapes, const AxvsMsdaLayerParams* params,
                              const AxvsMsdaLayerGrads* grads, float* d_src, float* d_pos, int N, int S, int C, int heads, int L, int P, int d_ffn,
                              float p_dropout, float p_attn_drop, unsigned seed, int recompute, void* saved, size_t saved_bytes, void* scratch,
                              size_t scratch_bytes, void* stream);

/* ---- Pixel-decoder glue: nn.Sequential(Conv2d(k=1), GroupNorm) between backbone NCHW maps and token rows
 *      (WC/msdeformattn.py:349-375 input_proj / output_proj; used at :412 and :434), PositionEmbeddingSine
 *      (WC/pos_embeddings.py:12-53) in token form. */
typedef struct AxvsConvGnParams {
  const float *conv_w, *conv_b;   /* Conv2d weight [Cout,Cin,1,1], bias [Cout] */
  const float *gn_w, *gn_b;       /* GroupNorm affine [Cout]                    */
} AxvsConvGnParams;
size_t axvs_conv1x1_gn_packed_bytes(int Cin, int Cout);
int axvs_conv1x1_gn_pack(const AxvsConvGnParams* p, void* packed, int Cin, int Cout, int dtype, void* stream);
size_t axvs_conv1x1_gn_workspace_bytes(int N, int HW, int Cout, int groups);
/* layouts: 0 = NCHW fp32 [N,C,H*W] (contiguous; strides ignored), 1 = token rows: row (n,p) at base + n*batch_stride + p*ld
 * (elements), so a level slice of a concatenated [N,S,C] buffer can be read / written in place. */
int axvs_conv1x1_gn_fwd(const float* x, int in_layout, long long in_batch_stride, long long in_ld, float* out, int out_layout,
                        long long out_batch_stride, long long out_ld, const void* packed, int N, int HW, int Cin, int Cout,
                        int groups, float eps, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* The same projection in train() mode under autograd (round 6): forward on the raw fp32 parameters (three-piece bf16 GEMM: fp32 accuracy; GroupNorm statistics
 * in fp32, fixed summation order) and backward (d_gamma, d_beta, d_W, d_b, d_x).  `saved` travels from the forward to the backward call (conv output, statistics,
 * the input as token rows when it was not); `scratch` is free between calls.  Layouts / strides as above; Cin, Cout multiples of 8.
 * An input gradient is produced in NCHW or contiguous token rows (d_x may be NULL). */
typedef struct AxvsConvGnGrads { float *conv_w, *conv_b, *gn_w, *gn_b; } AxvsConvGnGrads;   /* field order of AxvsConvGnParams */
size_t axvs_conv1x1_gn_train_saved_bytes(int N, int HW, int Cin, int Cout, int groups, int in_layout, long long in_batch_stride, long long in_ld);
size_t axvs_conv1x1_gn_train_scratch_bytes(int N, int HW, int Cin, int Cout, int groups, int backward);
int axvs_conv1x1_gn_train_fwd(const float* x, int in_layout, long long in_batch_stride, long long in_ld, float* out, int out_layout,
                              long long out_batch_stride, long long out_ld, const AxvsConvGnParams* p, int N, int HW, int Cin, int Cout, int groups,
                              float eps, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream);
int axvs_conv1x1_gn_train_bwd(const float* d_out, int out_layout, long long out_batch_stride, long long out_ld, const float* x, int in_layout,
                              long long in_batch_stride, long long in_ld, const AxvsConvGnParams* p, const AxvsConvGnGrads* grads, float* d_x, int N, int HW,
                              int Cin, int Cout, int groups, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream);
/* x[i] += v[i % C] in place (level_embed_3d on a channels-last position embedding, WC/msdeformattn.py:117-118) */
int axvs_add_channel_vector(float* x, const float* v, size_t n, int C, void* stream);
/* pos[n][row0 + y*W + x][c] (+ add[c] if add != NULL) inside a fp32 [N][S][C] buffer */
int axvs_pos2d(float* pos, const float* add, int N, int H, int W, int C, long long S, long long row0, float temperature,
               int normalize, float scale, void* stream);

/* ---- Clip-to-clip query alignment, maxtron_cc_model.py:360-369 `match_from_embds` without the host round trip.
 *      axvs_linear_sum_assignment: `batch` square problems, cost fp32 [batch][n][n] -> col4row int64 [batch][n] (the column
 *      assigned to every row) = scipy.optimize.linear_sum_assignment(cost)[1]; n <= 512.
 *      axvs_match_embds: tgt/cur fp32 [Q,C] -> indices int64 [Q] such that cur[indices] aligns with tgt
 *      (cost = 1 - cosine similarity, rows = target queries). */
int axvs_linear_sum_assignment(const float* cost, long long* col4row, int batch, int n, void* stream);
size_t axvs_match_embds_workspace_bytes(int Q, int C);
int axvs_match_embds(const float* tgt_embds, const float* cur_embds, long long* indices, int Q, int C, void* workspace,
                     size_t workspace_bytes, void* stream);
/* The per-video clip loop of maxtron_cc_model.py:280-301 for a batch of videos in three launches:
 *   prev = e[v,0];  for i in 1..Tc-1:  idx = match_from_embds(prev, e[v,i]);  prev = e[v,i][idx];  indices[v,i-1,:] = idx
 * mask_embeddings fp32 [V,Tc,Q,C]; indices int64 [V,Tc-1,Q] (the permutation that aligns clip i to the aligned clip i-1). */
size_t axvs_match_clips_workspace_bytes(int V, int Tc, int Q, int C);
int axvs_match_clips(const float* mask_embeddings, long long* indices, int V, int Tc, int Q, int C, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---- Prediction-to-ground-truth matching (VideoHungarianMatcher, maxtron_deeplab/modeling/matcher.py:48-124) on the device.
 *      axvs_linear_sum_assignment_rect: `batch` problems of nr rows; problem z is cost + z*nr*ld (fp32, row stride ld >= nc_max) and has
 *      nc_per_problem[z] columns (a HOST array; NULL: nc_max for all).  (rows_out, cols_out) int64 [batch][min(nr, nc_max)] =
 *      scipy.optimize.linear_sum_assignment(cost_z): min(nr, nc_z) pairs sorted by row, the unused tail -1.  nr in 1..512, nc in 0..512
 *      (nc_max == 0: nothing is written); otherwise AXVS_ERR_ARG.  Costs must be finite (SciPy raises on NaN / -inf; the kernel
 *      does not look).
 *      axvs_video_matcher: all (layer, video) problems of a training step in one call, no host synchronisation.
 *        pred_masks / pred_logits  HOST arrays of L device pointers: layer l's masks [B][Q][P] (mask_dtype AXVS_F16 / AXVS_BF16 / AXVS_F32,
 *                                  P = T*H*W) and logits fp32 [B][Q][K1] (K1 = K + 1: the void class last)
 *        targets, labels           the videos' ground truth concatenated along M: masks [sum M_b][P] (target_dtype AXVS_U8 for bool / uint8,
 *                                  or AXVS_F32) and int64 labels [sum M_b] (a label outside 0..K-1 is clamped; the reference raises)
 *        m_per_video               HOST array of B object counts (0 allowed), M_max their maximum
 *        sims                      fp32 [3][L*B][Q][M_max]: mask similarity, class similarity, cost = -mask_sim * class_sim (columns >= M_b zero)
 *        rows_out, cols_out        int64 [L*B][min(Q, M_max)], problem (l, b) at l*B + b: min(Q, M_b) pairs, the tail -1
 *        matched_dice, matched_cls fp32 [L*B][min(Q, M_max)]: mask / class similarity at the matched pairs (tail 0)
 *      L <= 16, B <= 64, Q and M_max <= 512 with ceil32(Q) + ceil32(M_max) <= 576, otherwise AXVS_ERR_ARG.  pred_masks is read ONCE
 *      while ceil(Q/32) * ceil(M_max/32) <= 16 (the 32 x 32 output blocks one workgroup accumulates: Q = 128 with M <= 128, Q = 256
 *      with M <= 64); beyond that the blocks are split into chunks of 16 over the grid and every chunk reads the logits and
 *      redoes the softmax of its pixels (2 chunks: two passes). */
int axvs_linear_sum_assignment_rect(const float* cost, long long ld, int nr, int nc_max, const int* nc_per_problem, long long* rows_out,
                                    long long* cols_out, int batch, void* stream);
size_t axvs_video_matcher_workspace_bytes(int L, int B, int Q, int M_max, long long P);
int axvs_video_matcher(const void* const* pred_masks, int mask_dtype, const float* const* pred_logits, const void* targets, int target_dtype,
                       const long long* labels, const int* m_per_video, int L, int B, int Q, int K1, long long P, int M_max, int masking_void_pixel,
                       float* sims, long long* rows_out, long long* cols_out, float* matched_dice, float* matched_cls, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- The set criterion's `labels` and `masks` losses and their gradients (MaXTronCCSetCriterion / MaXTronWCSetCriterion,
 *      maxtron_deeplab/modeling/cc_criterion.py:144-200, :237-266, :338-412) on top of axvs_video_matcher's device indices: all
 *      (layer, video) problems of a step per call, no host synchronisation, no atomics (results are run-to-run identical), and no
 *      [B][N][P] temporary besides the gradient itself.  Layer 0 is the final prediction, layer 1 + i is aux_outputs[i].
 *        pred_masks / pred_logits  HOST arrays of L device pointers: fp32 [B][N][P] and fp32 [B][N][K1], as axvs_video_matcher takes them
 *        targets, labels, m_per_video   as axvs_video_matcher takes them (target_dtype AXVS_U8 or AXVS_F32; a label outside 0..K-1 is clamped)
 *        rows, cols, matched_dice, matched_cls   axvs_video_matcher's outputs, [LM*B][kmax] with LM = 1 when share_final_matching
 *                                  (one matching serves every layer, and the void IoU of an unmatched query is taken on layer 0's
 *                                  masks), else LM = L (matching l*B + b serves layer l); kmax = 0: no object in any video
 *        losses                    fp32 [L][3]: loss_ce, loss_mask, loss_dice of every layer
 *        saved                     axvs_set_criterion_saved_bytes(L, B, N) bytes the forward writes and the backward reads: O(L*B*N)
 *        grad_losses               DEVICE fp32 [L][3]: the upstream gradients of `losses`
 *        d_pred_masks / d_pred_logits   HOST arrays of L device pointers shaped like the inputs; a NULL entry skips that gradient
 *      workspace_bytes travels as long long.  L <= 16, B <= 64, N <= 512, M_b <= 512, any P <= 2^40; otherwise AXVS_ERR_ARG (the size
 *      functions return 0 and axvs_last_error() names the bound).  pred_masks is read once by the forward and once by the backward
 *      while N <= 128; beyond that a pixel tile is read three times per pass, the second and third time from L2. */
size_t axvs_set_criterion_saved_bytes(int L, int B, int N);
size_t axvs_set_criterion_workspace_bytes(int L, int B, int N, int K1, long long P);
int axvs_set_criterion_fwd(const float* const* pred_masks, const float* const* pred_logits, const void* targets, int target_dtype,
                           const long long* labels, const int* m_per_video, const long long* rows, const long long* cols,
                           const float* matched_dice, const float* matched_cls, int kmax, int L, int B, int N, int K1, long long P,
                           int masking_void_pixel, int share_final_matching, float* losses, void* saved, void* workspace,
                           long long workspace_bytes, void* stream);
int axvs_set_criterion_bwd(const float* grad_losses, const float* const* pred_masks, const float* const* pred_logits, const void* targets,
                           int target_dtype, const int* m_per_video, int L, int B, int N, int K1, long long P, int masking_void_pixel,
                           int share_final_matching, const void* saved, float* const* d_pred_masks, float* const* d_pred_logits, void* stream);

/* ---- Tube-Link's point-sampled training loss (Mask2FormerVideoCCHeadTube.loss / loss_single / _get_target_single,
 *      models/video/tube_link_vis/mask2former_video_cc_head.py:519-694, with mmdet's ClassificationCost / CrossEntropyLossCost / DiceCost,
 *      MaskHungarianAssigner, get_uncertain_point_coords_with_randomness, CrossEntropyLoss and the naive DiceLoss): matching cost at
 *      num_points shared points, the device assignment, the k most uncertain of S candidate points per matched pair, the three losses
 *      and their gradients for all (layer, video) problems of a step.  Forward: 5 launches (one more per 256 problems beyond the first
 *      256), backward: 3; one stream, no host synchronisation, no copy to the host, no floating-point atomics (two runs give the same
 *      bits).  The random coordinates are INPUTS, so every shape is known on the host before anything runs.
 *        cls_scores / mask_preds   HOST arrays of L device pointers: fp32 [B][Q][K1] and fp32 [B][T][Q][h][w] (16-byte aligned).  The "long
 *                                  image" of a query has T*h rows: row r is line r % h of frame r / h, and a sample near a frame boundary
 *                                  blends the two frames, as the reference's flatten(1, 2) does
 *        targets, labels           uint8 / fp32 [sum M_b][T][Hg][Wg] and int64 [sum M_b], concatenated over the videos (a label outside
 *                                  0..K-1 is clamped); m_per_video: HOST int [B]
 *        class_weight              fp32 [K1];  num_total_masks: DEVICE fp32 scalar, max(reduce_mean(G), 1) in the reference
 *        match_coords              fp32 [L][B][num_points][2], cand_coords [L][G][S][2], rand_coords [L][G][num_points - k][2] in [0, 1):
 *                                  (x along w, y along the T*h rows); G = sum_b min(Q, M_b); pair g of a layer is the g-th matched
 *                                  query in (video, query) order
 *        losses                    fp32 [L][3]: loss_cls, loss_mask, loss_dice of every layer, times their loss weights
 *        rows, cols                int64 [L*B][min(Q, M_max)] in the layout of axvs_linear_sum_assignment_rect
 *        cost                      NULL, or fp32 [L*B][Q][M_max]: the matching cost
 *        sel_idx                   NULL, or int32 [L][G][k]: the kept candidates of every pair, in increasing order.  The k candidates with
 *                                  the smallest |logit| are kept; among EQUAL |logit| the lower index (the reference's topk leaves ties open)
 *        saved                     axvs_tl_loss_saved_bytes bytes the forward writes and the backward reads: O(L * G * num_points)
 *        grad_losses               DEVICE fp32 [L][3];  d_cls_scores / d_mask_preds: HOST arrays of L device pointers shaped like the inputs,
 *                                  a NULL entry skips that gradient.  Unmatched queries get exactly zero
 *      L <= 16, B <= 64, Q <= 512, M_b <= 512, num_points <= 16384, S <= 65536, k <= min(num_points, S), T*h <= 8192; otherwise AXVS_ERR_ARG
 *      (the size functions return 0 and axvs_last_error() names the bound). */
typedef struct AxvsTLLossCfg {
  int L, B, Q, K1, T, h, w, Hg, Wg;
  int num_points, num_cand, num_kept;      /* P, S = int(P * oversample_ratio), k = int(importance_sample_ratio * P) */
  int target_dtype;                        /* AXVS_U8 or AXVS_F32 */
  float cost_cls, cost_mask, cost_dice;    /* weights of the three matching costs (2, 5, 5) */
  float loss_cls, loss_mask, loss_dice;    /* weights of the three losses (2, 5, 5) */
  float dice_eps;                          /* eps of DiceCost and DiceLoss (1) */
} AxvsTLLossCfg;
size_t axvs_tl_loss_saved_bytes(const AxvsTLLossCfg* cfg, const int* m_per_video);
size_t axvs_tl_loss_workspace_bytes(const AxvsTLLossCfg* cfg, const int* m_per_video);
int axvs_tl_loss_fwd(const AxvsTLLossCfg* cfg, const float* const* cls_scores, const float* const* mask_preds, const void* targets,
                     const long long* labels, const int* m_per_video, const float* class_weight, const float* match_coords,
                     const float* cand_coords, const float* rand_coords, const float* num_total_masks, float* losses, long long* rows,
                     long long* cols, float* cost, int* sel_idx, void* saved, void* workspace, long long workspace_bytes, void* stream);
int axvs_tl_loss_bwd(const AxvsTLLossCfg* cfg, const float* grad_losses, const float* const* cls_scores, const float* const* mask_preds,
                     const void* targets, const int* m_per_video, const float* class_weight, const float* num_total_masks, const void* saved,
                     float* const* d_cls_scores, float* const* d_mask_preds, void* stream);

/* ---- The sampled pixel losses of the within-clip criterion (wc_criterion.py:62-142, :271-305, :341-415): Gumbel top-k sampling of
 *      k out of P = T*H*W pixels, `loss_pixel_insdis` of every layer, `loss_aux_semantic`, and their gradients.  One stream, no host
 *      synchronisation, no K x K tensor, no floating-point atomics (two runs give the same bits).  The uniform noise is an INPUT.
 *      With t the matched targets of a matching and video: area[i] = sum_p t[i,p], pix_area[p] = sum_i t[i,p] area[i], void[p] =
 *      sum_i t[i,p] < 1, key[p] = log(reciprocal(max(pix_area, 1)) * P) * temperature + void * -99999 + -log(-log u[p]), each fp32
 *      operation rounded once in this order.  The samples of a row are its k largest keys (equal keys: the lower pixel first), stored
 *      in increasing pixel order.
 *        targets, m_per_video, cols, kmax   as axvs_set_criterion_fwd takes them: cols int64 [LM*B][kmax] is the matcher's; LM matchings
 *        noise                     HOST array of R device pointers: fp32 [B][P] in [0, 1) per noise row
 *        row_matching / row_temperature / row_k   HOST [R]: the matching a row samples from, its temperature, its k (0: nothing selected)
 *        area, keys                device buffers the call fills: fp32 [LM*B][kmax] (NULL when kmax = 0) and fp32 [R][B][P] (the keys)
 *        idx                       int32 [R][B][kstride]: entries 0 .. k_r - 1 of a row are written
 *      axvs_pixel_insdis_*: per layer l and video b with F = pixel_feature[l][b][:, idx] and G = the matched targets at idx (matching 0
 *      when share_final_matching, else matching l), S = F^T F / 0.3 on the f32-input MFMA, g = G^T G, c_j = sum_k g[k,j],
 *      loss_j = (logsumexp_k S[k,j] c_j - sum_k g[k,j] S[k,j]) / max(c_j, 1); losses[l] = mean_b sum_j loss_j / max(#{loss_j != 0}, 1).
 *        pixel_feature / d_pixel_feature   HOST arrays of L device pointers, fp32 [B][C][P]; d_pixel_feature[l] must be ZERO-FILLED by
 *                                  the caller (only the sampled pixels are written), a NULL entry skips that layer
 *        idx                       int32 [L][B][kstride], distinct pixels per row (what axvs_pixel_sample wrote)
 *        saved                     axvs_pixel_insdis_saved_bytes: O(L*B*k); grad_losses: DEVICE fp32 [L]
 *      axvs_pixel_semantic_*: cross-entropy of pred fp32 [B][Cs][P] against sem int64 [B][P] at idx int32 [B][kstride]; a class of -1,
 *      num_classes or outside 0 .. Cs-1 is ignored; the same nonzero-count mean.  d_pred must be zero-filled by the caller.
 *      L <= 16, B <= 64, N <= 512, M_b <= 512, C a multiple of 4 up to 256, Cs <= 256, k <= min(8192, P), P <= 2^20, R <= 17; otherwise
 *      AXVS_ERR_ARG with the offending value named.  workspace_bytes travels as long long. */
int axvs_pixel_sample(const void* targets, int target_dtype, const int* m_per_video, const long long* cols, int kmax, int LM, int B, int N,
                      long long P, const float* const* noise, const int* row_matching, const float* row_temperature, const int* row_k, int R,
                      float* area, float* keys, int* idx, int kstride, void* stream);
size_t axvs_pixel_insdis_saved_bytes(int L, int B, int k);
size_t axvs_pixel_insdis_workspace_bytes(int L, int B, int C, int kmax, int k);
int axvs_pixel_insdis_fwd(const float* const* pixel_feature, const void* targets, int target_dtype, const int* m_per_video, const long long* cols,
                          int kmax, int share_final_matching, int L, int B, int N, int C, long long P, const int* idx, int k, int kstride,
                          float* losses, void* saved, void* workspace, long long workspace_bytes, void* stream);
int axvs_pixel_insdis_bwd(const float* grad_losses, const float* const* pixel_feature, const void* targets, int target_dtype,
                          const int* m_per_video, const long long* cols, int kmax, int share_final_matching, int L, int B, int N, int C,
                          long long P, const int* idx, int k, int kstride, const void* saved, float* const* d_pixel_feature, void* workspace,
                          long long workspace_bytes, void* stream);
size_t axvs_pixel_semantic_saved_bytes(int B, int k);
int axvs_pixel_semantic_fwd(const float* pred, const long long* sem, const int* idx, int k, int kstride, int B, int Cs, long long P,
                            int num_classes, float* loss, void* saved, void* stream);
int axvs_pixel_semantic_bwd(const float* grad_loss, const float* pred, const long long* sem, const int* idx, int k, int kstride, int B, int Cs,
                            long long P, int num_classes, const void* saved, float* d_pred, void* stream);

/* ---- Video panoptic post-processing (maxtron_cc_model.py:442-571, maxtron_wc_model.py:440-551: `video_seg_post_processing` +
 *      `panoptic_mask_inference`) on the device, in three launches and without the [N,T,H,W] tensor: per output pixel the bilinearly
 *      resized logits of the N slots (one stage + crop, or two stages with the crop between them; torch's align_corners True / False
 *      index arithmetic), their softmax and the slots above pixel_confidence_threshold; then, in one workgroup, the class softmax, the
 *      reorder (descending; EQUAL reorder scores go to the lower slot index, where the reference's argsort leaves ties open) and the
 *      reference's sequential merge; then the relabelled map.  Areas are exact integers (the reference's fp32 sums are inexact above
 *      2^24 pixels per slot) and the score sums are exact fixed-point integers: results are bit-equal from run to run.
 *        mask_cls     fp32 [N][K1] (K1 = K + 1: the void class last)
 *        mask_pred    [N][T][h][w], mask_dtype AXVS_F16 / AXVS_BF16 / AXVS_F32 (arithmetic in fp32)
 *        is_thing, cat_id   DEVICE int32 [K]: per contiguous class id whether it is a thing, and its category id
 *                     (sorted(thing_ids + stuff_ids)[label] in the reference)
 *        out_map      int32 [T][H][W]: cat_id * label_divisor + ii for things (ii: acceptance order per category), cat_id for stuff, -1 unassigned
 *        slot_ints    int32 [axvs_video_panoptic_table_ints(N)] = 4 + 7 N: {accepted things, segments, contested pixels, 0}, then per slot
 *                     final id (-1: not painted), merge rank, class label, area; then the accepted things in acceptance order: slot, category id, ii
 *                     (tail -1)
 *        slot_floats  fp32 [3][N]: class score, mean mask score over the area, reorder score
 *      cfg: the stage-1 resize goes to image_h x image_w; with two_stage the crop [:crop_h, :crop_w] of it is resized to H x W, otherwise
 *      the map is its crop [:H, :W].  N <= 512, any K >= 1, T*H*W < 2^31, pixel_confidence_threshold in (0.25, 1) (at most three slots
 *      pass per pixel); otherwise AXVS_ERR_ARG.  Arguments are checked before anything is launched; workspace_bytes travels as long long. */
typedef struct AxvsPanopticCfg {
  int N, K1, T, h, w;
  int image_h, image_w;
  int two_stage, crop_h, crop_w;
  int H, W;
  int align_corners, label_divisor;
  double pixel_confidence_threshold, overlap_threshold, class_threshold_thing, class_threshold_stuff;
  double reorder_class_weight, reorder_mask_weight;
} AxvsPanopticCfg;
size_t axvs_video_panoptic_workspace_bytes(const AxvsPanopticCfg* cfg);
size_t axvs_video_panoptic_table_ints(int N);
int axvs_video_panoptic_fwd(const AxvsPanopticCfg* cfg, const float* mask_cls, const void* mask_pred, int mask_dtype, const int* is_thing,
                            const int* cat_id, int* out_map, int* slot_ints, float* slot_floats, void* workspace, long long workspace_bytes,
                            void* stream);

/* ---- Video instance post-processing for Tube-Link VIS (mask2former_video_cc_head.py:1026-1034: the whole-video resize to
 *      batch_input_shape; maskformer_fusion_head.py:405-462: `instance_postprocess` per frame with its second resize to ori_shape;
 *      mask/utils.py:68-89: `mask2bbox`; mask2former_vis_video.py:184-193: the per-frame top 30) on the device, in four kernels and one memset and
 *      without a resized [T,Q,H,W] tensor.  Both resizes are bilinear with align_corners=False.
 *        mask_cls     fp32 [Q][K1] (K1 = C + 1: the void class last)
 *        mask_pred    [T][Q][h][w], mask_dtype AXVS_F16 / AXVS_BF16 / AXVS_F32 (arithmetic in fp32); frames num_frames..T-1 are not read
 *        out_masks    mask_bits 0: uint8 [num_frames][k_out][H][W]; mask_bits 1: 64-bit words [num_frames][k_out][H][ceil(W/64)], bit i of
 *                     word j = pixel 64 j + i of the row, the bits past W zero.  Rows past a frame's count are empty masks.
 *        table_ints   int32, in this order: {candidates kept, queries referenced}; candidate query [k_cand], candidate label [k_cand]
 *                     (tail -1); area [num_frames][k_cand] (tail -1); count [num_frames]; then per frame the selected rows, tail -1:
 *                     track id [num_frames][k_out] (1 + candidate position), label [.][k_out], query [.][k_out]
 *        table_floats fp32, in this order: candidate class score [k_cand]; mask score [num_frames][k_cand]; detection score [.][k_cand];
 *                     candidate box [.][k_cand][4]; selected box [num_frames][k_out][4]; selected score [num_frames][k_out] (tails -1)
 *      Candidates: the k_cand largest softmax scores over Q x C in DESCENDING order, equal scores to the lower flat index (the
 *      reference's topk(sorted=False) leaves the order open), then those with label < num_things, order kept.  Per frame and candidate:
 *      binary = resized logit > 0, area (exact integer), mask score = sum(sigmoid * binary) / (area + 1e-6) from an exact fixed-point
 *      sum (bit-equal from run to run), detection score = class score * mask score, box = {xmin, ymin, xmax + 1, ymax + 1} or zeros.
 *      Selection: the k_out largest detection scores, equal scores to the lower candidate position.
 *      Q <= 512, Q*C <= 2^17, 1 <= k_out <= k_cand <= min(Q*C, 256), 1 <= num_frames <= T, img_shape (crop) inside batch input (image),
 *      H*W < 2^31; otherwise AXVS_ERR_ARG.  Arguments are checked before anything is launched; workspace_bytes travels as long long. */
typedef struct AxvsVisCfg {
  int Q, K1, T, num_frames, h, w;
  int image_h, image_w;      /* batch_input_shape */
  int crop_h, crop_w;        /* img_shape */
  int H, W;                  /* ori_shape */
  int num_things, k_cand, k_out, mask_bits;
} AxvsVisCfg;
size_t axvs_video_instance_workspace_bytes(const AxvsVisCfg* cfg);
int axvs_video_instance_fwd(const AxvsVisCfg* cfg, const float* mask_cls, const void* mask_pred, int mask_dtype, void* out_masks,
                            int* table_ints, float* table_floats, void* workspace, long long workspace_bytes, void* stream);

/* ---- PositionEmbeddingSine3D.forward(x, mask=None) in channels-last form
 *      WC/pos_embeddings.py:86-130: pos fp32 [B,T,H,W,C], C = 2*num_pos_feats. */
int axvs_pos3d(float* pos, int B, int T, int H, int W, int C, float temperature, int normalize, float scale,
               void* stream);

/* The same with a padding mask (WC/pos_embeddings.py:96-106: coordinates = not_mask.cumsum along t / h / w, normalised by the
 * count over the whole axis).  mask: uint8 [B,T,H,W], non-zero = padded position. */
int axvs_pos3d_masked(float* pos, const unsigned char* mask, int B, int T, int H, int W, int C, float temperature, int normalize,
                      float scale, void* stream);

/* ---- out[i] = a[i] + gamma[i % C] * b[i]   (Tube-Link residual, TL/...pixel_decoder.py:625-627) */
int axvs_scaled_residual(const float* a, const float* b, const float* gamma, float* out, size_t n, int C,
                         void* stream);

/* =====================================================================================================
 * Training tier of the layer: forward that keeps its activations + backward.
 * Semantics: TemporalAxialTrajectoryAttentionLayer.forward in train() mode, WC/temporal_attention.py:187-220 under autograd:
 * dropout(p_dropout) on the spatial attention maps (:32, :55 -- the layer passes `dropout` as the attention's attn_drop, :164-165),
 * dropout1(p_attn_drop) on both pass outputs (:166, :204, :213), dropout2 / dropout3(p_dropout) in the FFN (:172-174, :182-183).
 * fp32 activations in natural [B,T,H,W,C] order; the Linear layers run on split-precision bf16 MFMA GEMMs (axvs_train_gemm.h,
 * no vendor BLAS); head_dim in {8,16,32,64}; T <= 16.
 * Dropout masks are a pure function of (seed, site, element offset in the reference's tensor at that site):
 *   h = seed ^ (site * 0x9E3779B9);  h = fmix32(h ^ lo32(idx));  h = fmix32(h ^ hi32(idx));  keep iff (h >> 8) >= floor(p * 2^24)
 *   (fmix32 = MurmurHash3's finaliser); sites: 1 height attention map [(B W) heads, T H, T, H], 2 height pass output [(B W), T H, C],
 *   3 width attention map [(B H) heads, T W, T, W], 4 width pass output [(B H), T W, C], 5 FFN hidden [M, F], 6 FFN output [M, C].
 * so backward (and a recomputed forward, and a CPU oracle) regenerate them: nothing but `seed` is kept.
 * ===================================================================================================== */
typedef struct AxvsTrajGrads {
  float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b, *proj_q_w, *proj_q_b, *proj_kv_w, *proj_kv_b, *proj_w, *proj_b;
} AxvsTrajGrads;
typedef struct AxvsAxialLayerGrads {   /* same field order as AxvsAxialLayerParams; every buffer is WRITTEN (not accumulated) */
  AxvsTrajGrads height_attn, width_attn;
  float *norm1_w, *norm1_b, *linear1_w, *linear1_b, *linear2_w, *linear2_b, *norm2_w, *norm2_b;
} AxvsAxialLayerGrads;
/* `saved`: the activations backward needs (kept between the two calls, or rebuilt by backward when recompute != 0: then any
 * buffer of that size will do); `scratch`: temporaries of one call (backward != 0: size for axvs_axial_layer_train_bwd). */
size_t axvs_axial_layer_train_saved_bytes(int B, int T, int H, int W, int C, int heads, int d_ffn);
size_t axvs_axial_layer_train_scratch_bytes(int B, int T, int H, int W, int C, int heads, int d_ffn, int backward);
/* src fp32 [(B T),(H W),C]; pos fp32 [B,T,H,W,C]; out like src.  params: the fp32 nn.Parameter storages themselves. */
int axvs_axial_layer_train_fwd(const float* src, const float* pos, float* out, const AxvsAxialLayerParams* params, int B, int T, int H,
                               int W, int C, int heads, int d_ffn, float p_dropout, float p_attn_drop, unsigned seed, void* saved,
                               size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream);
/* d_out: gradient of `out`.  Writes d_src, d_pos (NULL: not wanted) and every buffer of `grads`.  recompute != 0: `saved` is
 * rebuilt from (src, pos, params, seed) first -- the forward pass then only has to keep its inputs. */
int axvs_axial_layer_train_bwd(const float* d_out, const float* src, const float* pos, const AxvsAxialLayerParams* params,
                               const AxvsAxialLayerGrads* grads, float* d_src, float* d_pos, int B, int T, int H, int W, int C, int heads,
                               int d_ffn, float p_dropout, float p_attn_drop, unsigned seed, int recompute, void* saved, size_t saved_bytes,
                               void* scratch, size_t scratch_bytes, void* stream);

/* ---- the same tier for TemporalTrajectoryAttentionLayer (the full T*H*W layer, temporal_attn_type = "trajectory"):
 *      WC/temporal_attention.py:103-155 in train() mode under autograd -- ONE TrajectoryAttention over all T*HW tokens of a clip
 *      (q = k = src + pos, v = src, frames of HW keys), residual, norm1, FFN, norm2.  Arguments as for the axial layer with HW in
 *      place of H, W.  Dropout sites (element index = the element's offset in the reference's tensor at that site):
 *        1  the attention map [(B heads), T HW, T, HW]    (`dropout`, the attention's attn_drop: :109, :55)
 *        2  the attention output [B, T HW, C]              (dropout1 = `attn_drop`: :110, :145)
 *        5  the FFN hidden [M, F], 6  the FFN output [M, C] (dropout2 / dropout3 = `dropout`: :124-128)
 *      The attention map's indices pass 2^31 at [1,4,256,64,64]: they are formed in 64 bits.  head_dim 32 takes frames of any
 *      length (keys chunked through LDS, online softmax); head_dim 8 / 16 / 64 hold a frame in LDS: HW <= 2560 / 1280 / 320
 *      (the size functions return 0, axvs_last_error() names the bound).  T <= 16, B*T*HW*T < 2^31. */
typedef struct AxvsTrajLayerGrads {   /* same field order as AxvsTrajLayerParams; every buffer is WRITTEN (not accumulated) */
  AxvsTrajGrads temporal_attn;
  float *norm1_w, *norm1_b, *linear1_w, *linear1_b, *linear2_w, *linear2_b, *norm2_w, *norm2_b;
} AxvsTrajLayerGrads;
size_t axvs_traj_layer_train_saved_bytes(int B, int T, int HW, int C, int heads, int d_ffn);
size_t axvs_traj_layer_train_scratch_bytes(int B, int T, int HW, int C, int heads, int d_ffn, int backward);
/* src fp32 [(B T), HW, C]; pos fp32 [B,T,H,W,C] (= [B, T HW, C]); out like src */
int axvs_traj_layer_train_fwd(const float* src, const float* pos, float* out, const AxvsTrajLayerParams* params, int B, int T, int HW, int C,
                              int heads, int d_ffn, float p_dropout, float p_attn_drop, unsigned seed, void* saved, size_t saved_bytes,
                              void* scratch, size_t scratch_bytes, void* stream);
int axvs_traj_layer_train_bwd(const float* d_out, const float* src, const float* pos, const AxvsTrajLayerParams* params,
                              const AxvsTrajLayerGrads* grads, float* d_src, float* d_pos, int B, int T, int HW, int C, int heads, int d_ffn,
                              float p_dropout, float p_attn_drop, unsigned seed, int recompute, void* saved, size_t saved_bytes, void* scratch,
                              size_t scratch_bytes, void* stream);

/* =====================================================================================================
 * Training tier of the cross-clip tracking module: CrossClipTrackingModule.forward in train() mode,
 * CC/maxtron_cross_clip_tracking_module.py:275-322 under autograd -- the module the reference trains on its own with the
 * segmenter frozen (maxtron_cc_model.py:104-108).  Per layer: TrajectoryAttentionLayer (:133-173; attention-map dropout
 * p_attn_drop, site 10 + 2 l, index as in the layer above), ASPP (:176-201; _proj_drop p_aspp_drop, site 11 + 2 l, element
 * index of the reference's [(B Q), 256, Tc] tensor) + residual + LayerNorm (:293-295); then for EVERY layer the embedding
 * projections and the predictor's training branch (:300-309, :45-57) with (Sync)BatchNorm on BATCH statistics (eps 1e-3).
 * Sizes: C = 256, 8 heads, mask channels 128, norm_fn 'ln', kernel sizes 3; Q % 8 == 0, Tc <= 16, any V*H*W (the shipped
 * training setting: 12 clips of 2 frames, 193 x 337 pixel features).
 *
 * SyncBatchNorm: `allreduce` (NULL in a single process) is called with a device buffer of partial sums (and the row count)
 * that it must SUM over the ranks in place, ordered on `stream` -- three times per forward and three times per backward call.
 * The parameter gradients written are this rank's own share (like nn.SyncBatchNorm under DDP: ranks are averaged afterwards).
 * bn_stats (forward, out): [class_proj [nl][2][256] | mask_proj [nl][2][256] | mask_head [nl][2][128] | pixel [nl][2]] = the batch
 * mean and UNBIASED variance of each layer's call, for the caller's running-statistics update (momentum 0.01, in layer order).
 * The running means are only read (as the shift of the variance sums); gradients are WRITTEN, not accumulated; no gradient is
 * produced for panoptic_features (the frozen segmenter's output).
 * ===================================================================================================== */
typedef struct AxvsCCLayerGrads {     /* field order of AxvsCCLayerParams */
  AxvsTrajGrads attn;
  float *norm_w, *norm_b;
  float *aspp_w[3], *aspp_b[3];
  float *aspp_proj_w;
  float *aspp_norm_w, *aspp_norm_b;
  float *conv_norm_w, *conv_norm_b;
} AxvsCCLayerGrads;
typedef struct AxvsBNGrads { float *w, *b; } AxvsBNGrads;
typedef struct AxvsCCHeadGrads {      /* field order of AxvsCCHeadParams */
  float* class_proj_w; AxvsBNGrads class_proj_bn;
  float* mask_proj_w;  AxvsBNGrads mask_proj_bn;
  float* mask_head_w;  AxvsBNGrads mask_head_bn;
  float *class_head_w, *class_head_b;
  float *act_head_w, *act_head_b;
  AxvsBNGrads pixel_bn;
} AxvsCCHeadGrads;
typedef int (*axvs_allreduce_fn)(void* user, float* device_buf, size_t n, void* stream);   /* 0 = success */
typedef struct AxvsCCTrainCfg {
  int B, Q, Tc, V, H, W, K1, num_layers;
  int rates[3];
  float p_attn_drop, p_aspp_drop;
  unsigned seed;
  axvs_allreduce_fn allreduce;
  void* allreduce_user;
  int chain_only;            /* != 0: buffers and checks for axvs_cc_layers_train_* only (any Q; V, H, W, K1 ignored) */
} AxvsCCTrainCfg;
size_t axvs_cc_module_train_saved_bytes(const AxvsCCTrainCfg* cfg);
size_t axvs_cc_module_train_scratch_bytes(const AxvsCCTrainCfg* cfg, int backward);
size_t axvs_cc_module_train_bn_stats_floats(const AxvsCCTrainCfg* cfg);
/* clip_query fp32 [B,Q,Tc,256]; panoptic_features fp32 [B,128,Tc*V,H,W]; pred_logits fp32 [nl,1,Q,K1]; pred_masks fp32
 * [nl,B,Q,Tc*V,H,W]; layers: array of num_layers parameter sets (the fp32 nn.Parameter storages themselves; AxvsBN.mean / .var =
 * the running buffers). */
int axvs_cc_module_train_fwd(const float* clip_query, const float* panoptic_features, float* pred_logits, float* pred_masks, float* bn_stats,
                             const AxvsCCLayerParams* layers, const AxvsCCHeadParams* heads, const AxvsCCTrainCfg* cfg, void* saved,
                             size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream);
/* d_logits / d_masks: gradients of pred_logits / pred_masks (all layers: the auxiliary outputs are part of the loss, CC:311-318).
 * `saved` as the forward call left it.  Writes d_clip_query [B,Q,Tc,256] and every buffer of layer_grads[0..nl) / head_grads. */
int axvs_cc_module_train_bwd(const float* d_logits, const float* d_masks, const float* clip_query, const float* panoptic_features,
                             const AxvsCCLayerParams* layers, const AxvsCCHeadParams* heads, const AxvsCCLayerGrads* layer_grads,
                             const AxvsCCHeadGrads* head_grads, float* d_clip_query, const AxvsCCTrainCfg* cfg, void* saved, size_t saved_bytes,
                             void* scratch, size_t scratch_bytes, void* stream);

/* The layer chain alone (TrajectoryAttentionLayer + ASPP + norms of every layer, no prediction heads): Tube-Link's
 * Mask2FormerVideoCCHeadTube trains its own heads around the same layers (TL/models/video/tube_link_vis/mask2former_video_cc_head.py:
 * 925-947).  cfg: B, Q, Tc, num_layers, rates, dropouts, seed, chain_only = 1 (no all-reduce: the chain has no BatchNorm); buffers
 * sized by axvs_cc_module_train_saved_bytes / _scratch_bytes of that cfg.  out_queries / d_queries: fp32 [nl,B,Q,Tc,256] -- the clip
 * queries after every layer / the gradient that reaches each of them from outside the chain. */
int axvs_cc_layers_train_fwd(const float* clip_query, float* out_queries, const AxvsCCLayerParams* layers, const AxvsCCTrainCfg* cfg, void* saved,
                             size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream);
int axvs_cc_layers_train_bwd(const float* d_queries, const float* clip_query, const AxvsCCLayerParams* layers, const AxvsCCLayerGrads* layer_grads,
                             float* d_clip_query, const AxvsCCTrainCfg* cfg, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes,
                             void* stream);

/* Training tier of the Tube-Link cross-clip head's prediction heads (TLCC:761-797 under autograd) for ALL layers at once:
 * post_norm LayerNorm (eps 1e-5), class pooling (activation_proj, softmax over the Tc clips of each (layer, b, q), weighted sum),
 * cls_embed (no void bias), the three-Linear mask_embed MLP and the per-clip 'bqc,btchw->btqhw' einsum.  The parameters are shared
 * by the layers (AxvsTLHeadParams, the fp32 nn.Parameter storages).  Split-precision GEMMs as in the chain (16-bit products under
 * option train_amp); no atomics: a step is bit-reproducible.
 * Bounds (the size functions return 0 and axvs_last_error() names the bound): C = 256 (the queries), Cm in {128, 256}, Q a multiple
 * of 4, Tc <= 16, num_layers <= 16, h*w <= 2^26 (any h, w: rows of pixels need no alignment), num_layers*B*Q*Tc*256 < 2^31; any B,
 * frames_per_clip, K1.  Buffers: `saved` (forward -> backward) and `scratch` sized by the functions below; the backward scratch
 * holds num_layers shares of one frame's mask-feature gradient (num_layers*Cm*h*w floats) when num_layers > 1. */
typedef struct AxvsTLHeadGrads {      /* field order of AxvsTLHeadParams; every buffer is WRITTEN (not accumulated) */
  float *post_norm_w, *post_norm_b;
  float *activation_proj_w, *activation_proj_b;
  float *cls_embed_w, *cls_embed_b;
  float* mask_embed_w[3];
  float* mask_embed_b[3];
} AxvsTLHeadGrads;
typedef struct AxvsTLHeadTrainCfg {
  int B, Q, Tc, frames_per_clip, h, w, K1, Cm, num_layers;
} AxvsTLHeadTrainCfg;
size_t axvs_tl_heads_train_saved_bytes(const AxvsTLHeadTrainCfg* cfg);
size_t axvs_tl_heads_train_scratch_bytes(const AxvsTLHeadTrainCfg* cfg, int backward);
/* queries fp32 [nl,B,Q,Tc,256] (what axvs_cc_layers_train_fwd writes); mask_feature fp32 [B,Tc*fpc,Cm,h,w];
 * cls_logits fp32 [nl,B,Q,K1]; mask_logits fp32 [nl,B,Tc*fpc,Q,h,w]. */
int axvs_tl_heads_train_fwd(const float* queries, const float* mask_feature, float* cls_logits, float* mask_logits, const AxvsTLHeadParams* params,
                            const AxvsTLHeadTrainCfg* cfg, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream);
/* d_cls / d_masks: gradients of cls_logits / mask_logits; `saved` as the forward left it (the mask logits are not read).  Writes
 * d_queries [nl,B,Q,Tc,256] (the d_queries of axvs_cc_layers_train_bwd), every buffer of `grads`, and d_mask_feature
 * [B,Tc*fpc,Cm,h,w] when it is not NULL. */
int axvs_tl_heads_train_bwd(const float* d_cls, const float* d_masks, const float* queries, const float* mask_feature, const AxvsTLHeadParams* params,
                            const AxvsTLHeadGrads* grads, float* d_queries, float* d_mask_feature, const AxvsTLHeadTrainCfg* cfg, void* saved,
                            size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* ---- Tube-Link's per-clip masked-attention query decoder (Mask2FormerVideoCCHeadTube.forward: the nine DetrTransformerDecoderLayers
 * with forward_head_video in front of each; frozen and in eval() in training and inference alike, so forward only) --------------------
 * All tensors fp32.  N (video, clip) pairs are independent and may be stacked.  Every contraction is fp32-accurate: the Linear layers on
 * the three-piece split-precision GEMM, the mask logits and the attention on f32-input MFMAs.  Equal inputs give equal bits.
 * Bounds (AXVS_ERR_ARG outside them): C 256, 8 heads, FFN 2048, 3 levels, 1..16 layers, Q <= 256, T <= 16, T*lh*lw < 2^24 per level,
 * h*w < 2^24, N <= 4095.  Layer i attends to level i % 3.
 * Parameters: a layer's tensors under the reference's names -- attentions.0 = cross-attention (in_proj [3C,C] / [3C], out_proj),
 * norms.0, attentions.1 = self-attention, norms.1, ffns.0.layers.0.0 [F,C], ffns.0.layers.1 [C,F], norms.2. */
typedef struct AxvsM2fLayerParams {
  const float *cross_in_w, *cross_in_b, *cross_out_w, *cross_out_b, *norm0_w, *norm0_b;
  const float *self_in_w, *self_in_b, *self_out_w, *self_out_b, *norm1_w, *norm1_b;
  const float *ffn1_w, *ffn1_b, *ffn2_w, *ffn2_b, *norm2_w, *norm2_b;
} AxvsM2fLayerParams;
/* query_embed / query_feat [Q,C]; level_embed [3,C]; mask_embed: three Linear layers [C,C]; cls_embed [K1,C] */
typedef struct AxvsM2fHeadParams {
  const float *post_norm_w, *post_norm_b, *query_embed, *query_feat, *level_embed;
  const float* mask_embed_w[3];
  const float* mask_embed_b[3];
  const float *cls_embed_w, *cls_embed_b;
} AxvsM2fHeadParams;
/* mask features [N,T,C,h,w]; level l memory [N,T,C,lh[l],lw[l]] (low to high resolution); K1 = classes + 1;
 * pos_*: SinePositionalEncoding3D(num_feats = C/2) -- temperature, normalize, scale */
typedef struct AxvsM2fCfg {
  int N, Q, T, C, heads, ffn, num_layers, num_levels, K1, h, w;
  int lh[3], lw[3];
  int return_predictions, pos_normalize;
  float pos_temperature, pos_scale;
} AxvsM2fCfg;
size_t axvs_m2f_decoder_packed_bytes(const AxvsM2fCfg* cfg);      /* depends on Q, K1, num_layers only; 0: cfg refused (axvs_last_error) */
/* layers: num_layers structs.  Copies on `stream`; the parameter tensors must stay alive until they have run. */
int axvs_m2f_decoder_pack(const AxvsM2fLayerParams* layers, const AxvsM2fHeadParams* head, const AxvsM2fCfg* cfg, void* packed, void* stream);
size_t axvs_m2f_decoder_workspace_bytes(const AxvsM2fCfg* cfg);
/* memories: host array of the three levels' device pointers.  query_out [N,Q,C]: the queries after the last layer.  With
 * cfg->return_predictions: cls_pred [N,Q,K1] and mask_pred [N,T,Q,h,w] of the last layer (the one full-resolution mask einsum); else both
 * may be NULL.  debug_bits / debug_flags (both or neither): every layer's attention mask as the layer consumed it, layer after layer --
 * bits uint32 [N,Q,ceil(S_i/32)] (bit k & 31 of word k / 32 set = key k masked, S_i = T*lh*lw of level i % 3, bits past S_i zero) and
 * flags int32 [N,Q] per layer (0 = every key masked: the query attends to all keys). */
int axvs_m2f_decoder_fwd(const AxvsM2fCfg* cfg, const void* packed, const float* mask_features, const float* const* memories, float* query_out,
                         float* cls_pred, float* mask_pred, unsigned* debug_bits, int* debug_flags, void* workspace, long long workspace_bytes,
                         void* stream);
/* Stage entries.  One mask head: x [N,Q,C] (queries before post_norm) -> bits [N,Q,ceil(S/32)], flags [N,Q] at `level`. */
size_t axvs_m2f_attn_mask_workspace_bytes(const AxvsM2fCfg* cfg, int level);
int axvs_m2f_attn_mask_fwd(const AxvsM2fCfg* cfg, const void* packed, const float* x, const float* mask_features, int level, unsigned* bits, int* flags,
                           void* workspace, long long workspace_bytes, void* stream);
/* One layer given its attention mask: x [N,Q,C], memory of level layer % 3 -> out [N,Q,C] (may be x). */
size_t axvs_m2f_layer_workspace_bytes(const AxvsM2fCfg* cfg, int layer);
int axvs_m2f_layer_fwd(const AxvsM2fCfg* cfg, const void* packed, int layer, const float* x, const float* memory, const unsigned* bits,
                       const int* flags, float* out, void* workspace, long long workspace_bytes, void* stream);

/* ---- Video-kMaX's k-means query decoder (MaXTronTransformerDecoder in eval mode: kMaXTransformerLayers over three feature levels and the
 * final kMaXPredictor) ---------------------------------------------------------------------------------------------------------------
 * All tensors fp32; forward only.  B clips of T frames: features [(B T), C_l, h_l, w_l] and panoptic features [(B T), 256, H, W] are viewed
 * as the stacked maps b c (t h) w, as the reference views them (the predictor's depthwise 5 x 5 crosses frame boundaries).  Queries
 * travel as rows [B, L, 256].  The [B, L, T*h*w] mask logits of a layer never exist: a pixel's cluster is the argmax of a z + b over
 * the clusters, equal maxima to the lower index.  Equal inputs give equal bits, and a clip's bits do not depend on the clips beside it.
 * Bounds (AXVS_ERR_ARG outside them): 1 <= L <= 256, K1 <= 256, in_channels multiples of 16 up to 2048, pan_channels 256, T <= 16,
 * 1..16 layers over levels 0..2, heads 8, base_filters 128, T*h*w < 2^24 per map, h <= 16383, B <= 4095.
 * Parameters arrive FOLDED (every BatchNorm as an affine map on its running statistics, eps 1e-3, folded in float64 by the caller into
 * the convolution in front of it) and in the layouts the kernels read:
 *   dw_w [25][256] (tap-major), ph1 [256][256], ph2 [128][256] + [128], mh [128][256] + [128], cls [K1][256] + [K1] (bias towards void
 *   included), mask_ab [4] = (a, b, 0, 0) of the one-channel mask BatchNorm;
 *   pix1 [256][C_l], q1 [256][256]; kv_w [256][260]: the value projection under both BatchNorms that follow it, column 256 = its bias
 *   under the same (multiplied by the cluster's pixel count), 257..259 zero; kv_b [256]: the constant term; k3 [256][256];
 *   qkv [512][256] (q 128, k 128, v 256 rows); sim_ab [16] = a[8], b[8] per head; rv_ab [512] = a[256], b[256]; a3 [256][256];
 *   f1 [2048][256], f2 [256][2048]; centers [L][256]; cep / mep [256][256]. */
typedef struct AxvsKmaxPredictorParams {
  const float *dw_w, *dw_b, *ph1_w, *ph1_b, *ph2_w, *ph2_b, *mh_w, *mh_b, *cls_w, *cls_b, *mask_ab;
} AxvsKmaxPredictorParams;
typedef struct AxvsKmaxLayerParams {
  const float *pix1_w, *pix1_b, *q1_w, *q1_b;
  AxvsKmaxPredictorParams pred;
  const float *kv_w, *kv_b, *k3_w, *k3_b, *qkv_w, *qkv_b, *sim_ab, *rv_ab, *a3_w, *a3_b, *f1_w, *f1_b, *f2_w, *f2_b;
} AxvsKmaxLayerParams;
typedef struct AxvsKmaxHeadParams {
  const float *centers, *cep_w, *cep_b, *mep_w, *mep_b;
  AxvsKmaxPredictorParams pred;
} AxvsKmaxHeadParams;
/* layer i reads level layer_level[i]; level l: in_channels[l] x h[l] x w[l]; panoptic features pan_channels x H x W; K1 = classes + 1;
 * want_masks / want_pixel_feature: which of the two full-resolution outputs the final predictor writes */
typedef struct AxvsKmaxCfg {
  int B, T, L, K1, num_layers;
  int layer_level[16];
  int in_channels[3], h[3], w[3];
  int pan_channels, H, W;
  int heads, base_filters;
  int want_masks, want_pixel_feature;
} AxvsKmaxCfg;
size_t axvs_kmax_decoder_packed_bytes(const AxvsKmaxCfg* cfg);      /* depends on L, K1, the layers' levels and in_channels; 0: cfg refused */
/* layers: num_layers structs.  Copies on `stream`; the parameter tensors must stay alive until they have run. */
int axvs_kmax_decoder_pack(const AxvsKmaxLayerParams* layers, const AxvsKmaxHeadParams* head, const AxvsKmaxCfg* cfg, void* packed, void* stream);
size_t axvs_kmax_decoder_workspace_bytes(const AxvsKmaxCfg* cfg);
/* features: host array of the three levels' device pointers (a level no layer reads may be NULL).  pred_logits [B,L,K1], pred_masks
 * [B,L,T,H,W] (want_masks), pred_mask_embeddings [B,L,128], pixel_feature [B,128,T,H,W] (want_pixel_feature), cluster_centers [B,L,256].
 * debug_idx (nullable): every layer's index map as the layer consumed it, int32 [B, T*h*w] of the layer's level, layer after layer. */
int axvs_kmax_decoder_fwd(const AxvsKmaxCfg* cfg, const void* packed, const float* const* features, const float* panoptic, float* pred_logits,
                          float* pred_masks, float* pred_mask_embeddings, float* pixel_feature, float* cluster_centers, int* debug_idx, void* workspace,
                          long long workspace_bytes, void* stream);
/* Stage entries (update_stage 0: axvs_kmax_assign_fwd, 1: axvs_kmax_layer_fwd).  query [B,L,256]; feature: the layer's level. */
size_t axvs_kmax_stage_workspace_bytes(const AxvsKmaxCfg* cfg, int layer, int update_stage);
/* the assignment of one layer: idx int32 [B, T*h*w], class_logits [B,L,K1] (the layer's own class head, bias towards void included) */
int axvs_kmax_assign_fwd(const AxvsKmaxCfg* cfg, const void* packed, int layer, const float* query, const float* feature, int* idx, float* class_logits,
                         void* workspace, long long workspace_bytes, void* stream);
/* the same layer given its index map (an index outside 0..L-1 joins no cluster) -> out [B,L,256], the new query feature */
int axvs_kmax_layer_fwd(const AxvsKmaxCfg* cfg, const void* packed, int layer, const float* query, const float* feature, const int* idx, float* out,
                        void* workspace, long long workspace_bytes, void* stream);

/* ---- Video-kMaX's pixel decoder (kMaXPixelDecoder in eval mode: four stages of SingleBlocks from stride 32 down to stride 4, a
 * ResizedFuse in front of stages 1..3) ------------------------------------------------------------------------------------------------
 * All tensors fp32; forward only.  N frames, each on its own: features[i] [N, in_channels[i], h[i], w[i]], stage 0 the coarsest.
 * Stage i: blocks[i] SingleBlocks of base filter base[i], axial[i] != 0: axial-attention blocks (1x1 -> height-axis and width-axis
 * attention with relative positions, 8 heads, key depth base/8, value depth 2*base/8 -> 1x1), else bottleneck blocks (1x1 -> 3x3 ->
 * 1x1); a stage's output has 4 * base[i] channels.  Equal inputs give equal bits, and a frame's bits do not depend on the frames beside it.
 * Bounds (AXVS_ERR_ARG outside them): heads 8; 1..16 blocks per stage; axial base filter 512, 256 or 128 and axis lengths h, w <= 128
 * (<= 80 at base filter 512: what the attention kernel's LDS holds), N * max(h, w) <= 65535; bottleneck base filter a multiple of 32
 * up to 256; in_channels multiples of 16 up to 2048; N*h*w < 2^24 per stage, N <= 4096.
 * Parameters arrive FOLDED (every BatchNorm as an affine map on its running statistics, eps 1e-3, folded in float64 by the caller into
 * the convolution in front of it) and in the layouts the kernels read.  A block: sc [4b][cin] + [4b] (only when cin != 4b, else NULL),
 * c1 [mid][cin] + [mid] (mid = 2b axial, b bottleneck), c2 [9][b][b] tap-major + [b] (bottleneck only), c3 [4b][mid] + [4b]; an axis
 * (axial only): qkv [4b][2b] + [4b] (q b, k b, v 2b rows, heads outermost), eq / ek [509][b/8], ev [509][2b/8] (row r + 254 for the
 * offset r = m - l), sim_a [24] the gains of the similarity BatchNorm (channel part*8 + head; its offsets cancel in the softmax),
 * out_ab [3][2b]: the gains of the retrieved content and of the retrieved positions, then the sum of the two offsets.
 * A fuse (in front of stage i): ln [in_channels[i]] x 2 the LayerNorm (eps 1e-6) of the high-resolution input, low [b][4 b_prev] + [b]
 * (only when 4 b_prev != b), high [b][in_channels[i]] + [b] (only when in_channels[i] != b). */
typedef struct AxvsKpixAxisParams {
  const float *qkv_w, *qkv_b, *eq, *ek, *ev, *sim_a, *out_ab;
} AxvsKpixAxisParams;
typedef struct AxvsKpixBlockParams {
  const float *sc_w, *sc_b, *c1_w, *c1_b, *c2_w, *c2_b;
  AxvsKpixAxisParams height, width;
  const float *c3_w, *c3_b;
} AxvsKpixBlockParams;
typedef struct AxvsKpixFuseParams {
  const float *ln_w, *ln_b, *low_w, *low_b, *high_w, *high_b;
} AxvsKpixFuseParams;
typedef struct AxvsKpixCfg {
  int N;
  int in_channels[4], h[4], w[4];
  int base[4], blocks[4], axial[4];
  int heads;
} AxvsKpixCfg;
size_t axvs_kmax_pix_packed_bytes(const AxvsKpixCfg* cfg);      /* depends on the channels, blocks and stage types only; 0: cfg refused */
/* blocks: sum(cfg->blocks) structs, stage after stage; fuses: three; ln0: the LayerNorm of features[0].  Copies on `stream`; the
 * parameter tensors must stay alive until they have run. */
int axvs_kmax_pix_pack(const AxvsKpixBlockParams* blocks, const AxvsKpixFuseParams* fuses, const float* ln0_w, const float* ln0_b, const AxvsKpixCfg* cfg,
                       void* packed, void* stream);
size_t axvs_kmax_pix_workspace_bytes(const AxvsKpixCfg* cfg);   /* enough for the decoder and for every stage entry below */
/* features, outputs: host arrays of four device pointers; outputs[i] [N, 4 base[i], h[i], w[i]]: the raw (pre-gelu) output of stage i */
int axvs_kmax_pix_decoder_fwd(const AxvsKpixCfg* cfg, const void* packed, const float* const* features, float* const* outputs, void* workspace,
                              long long workspace_bytes, void* stream);
/* Stage entries.  block_index counts the blocks of all stages; the block's stage gives h, w and the base filter b.
 * One axis pass (axis 0: the columns of a frame, 1: its rows) on qkv rows [N, h, w, 4b] (after the qkv BatchNorm) -> out [N, h, w, 2b]. */
int axvs_kmax_pix_axial_attn_fwd(const AxvsKpixCfg* cfg, const void* packed, int block_index, int axis, const float* qkv, float* out, void* stream);
/* one SingleBlock: x [N, cin, h, w] -> out [N, 4b, h, w] */
int axvs_kmax_pix_block_fwd(const AxvsKpixCfg* cfg, const void* packed, int block_index, const float* x, float* out, void* workspace,
                            long long workspace_bytes, void* stream);
/* one ResizedFuse (fuse_index 0..2, in front of stage fuse_index + 1), the LayerNorm of its high-resolution input included:
 * low [N, 4 b_prev, h_prev, w_prev], high = features[fuse_index + 1] -> out [N, b, h, w] */
int axvs_kmax_pix_fuse_fwd(const AxvsKpixCfg* cfg, const void* packed, int fuse_index, const float* low, const float* high, float* out, void* workspace,
                           long long workspace_bytes, void* stream);

/* ---- ConvNeXt / ConvNeXtV2 backbone (eval forward; csrc/axvs_convnext.hip) ---------------------------------------------------------------
 * All tensors fp32; forward only.  N frames, each on its own.  image [N, 3, H, W] -> stem / stage maps of dims[i] channels, h[0] =
 * floor((H + 3) / 4), w[0] likewise, h[i] = floor((h[i-1] + 1) / 2): the reference's zero padding in front of each patchify convolution.
 * Stage i: depths[i] blocks (depthwise 7 x 7 -> LayerNorm -> Linear 4x + gelu -> [v2: GRN] -> Linear + residual).  Activations are rows
 * [N][h][w][C] (channels-last) between the entries; only axvs_cnx_fwd writes NCHW.  Equal inputs give equal bits, and a frame's bits do
 * not depend on the frames beside it.
 * Bounds (AXVS_ERR_ARG outside them): dims multiples of 16 in 16..2048; 1..64 blocks per stage; N in 1..4096; h, w in 1..16383 and
 * N*h*w < 2^24 per stage.  axvs_cnx_fwd also wants h / w to be the sizes H / W give; the step entries read h[stage], w[stage] alone.
 * Parameters arrive FOLDED by the caller (float64) and in the layouts the kernels read.  Stem (downs[0]): w [dims[0]][48] (the
 * convolution weight's own (c, ky, kx) order), b, and ln: the LayerNorm BEHIND it.  downs[i], i = 1..3: ln [dims[i-1]] x 2 the LayerNorm in
 * FRONT, w [dims[i]][4 dims[i-1]] in patch order (ky, kx, c), b.  A block: dw_w [49][C] (tap ky*7 + kx, channel fastest), dw_b, ln x 2,
 * w1 [4C][C], b1, w2 [C][4C], b2 -- v1: gamma folded into w2 and b2; v2: b2 = W2 beta + b2 and grn_gamma [4C] (NULL for v1). */
typedef struct AxvsCnxDownParams {
  const float *ln_w, *ln_b, *w, *b;
} AxvsCnxDownParams;
typedef struct AxvsCnxBlockParams {
  const float *dw_w, *dw_b, *ln_w, *ln_b, *w1, *b1, *w2, *b2, *grn_gamma;
} AxvsCnxBlockParams;
typedef struct AxvsCnxCfg {
  int N, H, W;
  int dims[4], depths[4], h[4], w[4];
  int v2;
} AxvsCnxCfg;
size_t axvs_cnx_packed_bytes(const AxvsCnxCfg* cfg);      /* depends on dims, depths and v2 only; 0: cfg refused */
/* downs: four structs (the stem first); blocks: sum(cfg->depths), stage after stage.  Copies on `stream`; the parameter tensors must stay
 * alive until they have run. */
int axvs_cnx_pack(const AxvsCnxDownParams* downs, const AxvsCnxBlockParams* blocks, const AxvsCnxCfg* cfg, void* packed, void* stream);
size_t axvs_cnx_workspace_bytes(const AxvsCnxCfg* cfg);   /* enough for the network and for every step entry below */
/* outputs: a host array of five device pointers -- stem, res2 .. res5 as [N, dims, h, w]; NULL: that map is not written */
int axvs_cnx_fwd(const AxvsCnxCfg* cfg, const void* packed, const float* image, float* const* outputs, void* workspace, long long workspace_bytes,
                 void* stream);
/* Step entries, rows in and out.  image [N, 3, H, W] -> out [N, h[0], w[0], dims[0]] (patches, convolution, LayerNorm) */
int axvs_cnx_stem_fwd(const AxvsCnxCfg* cfg, const void* packed, const float* image, float* out, void* workspace, long long workspace_bytes, void* stream);
/* downsample layer `index` (1..3): x [N, h[index-1], w[index-1], dims[index-1]] -> out [N, h[index], w[index], dims[index]] */
int axvs_cnx_down_fwd(const AxvsCnxCfg* cfg, const void* packed, int index, const float* x, float* out, void* workspace, long long workspace_bytes,
                      void* stream);
/* block_index counts the blocks of all stages; the block's stage gives h, w and C.  Depthwise 7 x 7 + LayerNorm: x [N, h, w, C] -> out alike */
int axvs_cnx_dwln_fwd(const AxvsCnxCfg* cfg, const void* packed, int block_index, const float* x, float* out, void* stream);
/* one whole block: x [N, h, w, C] -> out alike (out != x) */
int axvs_cnx_block_fwd(const AxvsCnxCfg* cfg, const void* packed, int block_index, const float* x, float* out, void* workspace, long long workspace_bytes,
                       void* stream);

/* ---- ResNet bottleneck backbone (eval forward; csrc/axvs_resnet.hip) ------------------------------------------------------------------------
 * All tensors fp32; forward only.  N frames, each on its own.  image [N, 3, H, W] -> the stem (7x7 / stride 2 / padding 3 convolution,
 * BatchNorm, ReLU, 3x3 / stride 2 / padding 1 max pool: stem_channels at ceil(ceil(H / 2) / 2)) -> four stages of bottleneck blocks (1x1
 * -> 3x3 -> 1x1, each with its BatchNorm, ReLU behind the first two and behind the sum with the shortcut).  Stage i: blocks[i] blocks of
 * bottleneck width width[i] and out_channels[i] outputs; its first block has stride[i] (in the 1x1 with stride_in_1x1, else in the 3x3)
 * and a projection shortcut where its input channels differ from out_channels[i]; every 3x3 of the stage has dilation[i] = its padding.
 * h[i] x w[i] is the map stage i READS; it leaves ceil(h[i] / stride[i]) x ceil(w[i] / stride[i]).  Activations are rows [N][h][w][C]
 * (channels-last) between the entries; only axvs_rn_fwd writes NCHW.  Equal inputs give equal bits, and a frame's bits do not depend on
 * the frames beside it.
 * Bounds (AXVS_ERR_ARG outside them): in_channels 3; stem_channels a multiple of 16 in 16..128; 1..64 blocks per stage; width a multiple
 * of 32 in 32..512; out_channels multiples of 16 in 16..2048; stride and dilation 1 or 2, stride 2 only where the channels change and not together with dilation 2; N in
 * 1..4096; h, w in 1..16383 and N*h*w < 2^24 per stage.  axvs_rn_fwd also wants h / w to be the sizes H / W give; the step entries read
 * h[stage], w[stage] alone (and axvs_rn_stem_fwd H, W, h[0], w[0]).
 * Parameters arrive with every BatchNorm FOLDED by the caller (float64): w = conv weight * bn_w / sqrt(running_var + eps) per output channel,
 * b = bn_b - running_mean * that scale.  Stem: w [147][stem_channels] ((colour, ky, kx) major, output channel fastest), b.  A block: w1
 * [width][in], w2 [width][9][width] (output channel, tap ky*3 + kx, input channel), w3 [out][width], ws [out][in] the projection (NULL
 * with bs where the block has none), each with its b.  The workspace size goes LAST in these entries. */
typedef struct AxvsRnStemParams {
  const float *w, *b;
} AxvsRnStemParams;
typedef struct AxvsRnBlockParams {
  const float *w1, *b1, *w2, *b2, *w3, *b3, *ws, *bs;
} AxvsRnBlockParams;
typedef struct AxvsRnCfg {
  int N, H, W;
  int in_channels, stem_channels;
  int width[4], out_channels[4], blocks[4], stride[4], dilation[4], h[4], w[4];
  int stride_in_1x1;
} AxvsRnCfg;
size_t axvs_rn_packed_bytes(const AxvsRnCfg* cfg);      /* depends on the channels, blocks and strides only; 0: cfg refused */
/* blocks: sum(cfg->blocks) structs, stage after stage.  Copies and splits on `stream`; the parameter tensors must stay alive until they
 * have run. */
int axvs_rn_pack(const AxvsRnStemParams* stem, const AxvsRnBlockParams* blocks, const AxvsRnCfg* cfg, void* packed, void* stream);
size_t axvs_rn_workspace_bytes(const AxvsRnCfg* cfg);   /* enough for the network and for every step entry below */
/* outputs: a host array of five device pointers -- stem, res2 .. res5 as [N, C, h, w]; NULL: that map is not written */
int axvs_rn_fwd(const AxvsRnCfg* cfg, const void* packed, const float* image, float* const* outputs, void* stream, void* workspace,
                long long workspace_bytes);
/* Step entries, rows in and out.  image [N, 3, H, W] -> out [N, h[0], w[0], stem_channels] */
int axvs_rn_stem_fwd(const AxvsRnCfg* cfg, const void* packed, const float* image, float* out, void* stream);
/* block_index counts the blocks of all stages.  The block's 3x3 convolution + BatchNorm + ReLU on conv1's map: x [N, hm, wm, width] ->
 * out [N, ceil(hm / s), ceil(wm / s), width], s the stride the block puts into its 3x3 (out != x) */
int axvs_rn_conv3_fwd(const AxvsRnCfg* cfg, const void* packed, int block_index, const float* x, float* out, void* stream);
/* one whole block: x [N, hin, win, in] -> out [N, ho, wo, out_channels] (out != x); a stage's first block reads h[stage] x w[stage], the
 * others the map the stage leaves */
int axvs_rn_block_fwd(const AxvsRnCfg* cfg, const void* packed, int block_index, const float* x, float* out, void* stream, void* workspace,
                      long long workspace_bytes);

/* ---- test hooks, not part of the drop-in surface ----------------------------------------------------------------------------------
 * One call of the training tier's split-precision GEMM dispatch (tr_gemm_nt_kernel / tr_gemm_tn_kernel behind the host code every
 * training entry point above uses), with every operand, stride and epilogue field explicit: what tests/test_hip_train_gemm.py holds
 * against float64.  The call goes through the same host functions as the training tiers, so the choice of kernel instantiation is part
 * of what it exercises; option "train_amp" applies as it does there (under it `exact` is ignored).
 *   op AXVS_TEST_GEMM_NT         c[M,N] (row stride ldc; with ksteps > 0 the zsplits split-K partials [z][M][ldc]) = epilogue(A B^T), A = a[M,K] (lda, +a2,
 *                                or with aff the per-row-group affine form of a and a2, aff_rows rows per group), B = b[N,K] (ldb); rows at al_a / al_b floats
 *      AXVS_TEST_GEMM_FWD        the same on contiguous rows (strides, alignments, aff and split-K ignored)
 *      AXVS_TEST_GEMM_WGRAD      c[N,K] = mul a[M,N]^T b[M,K] (row strides lda / ldb, 0: N / K) and, when db != NULL, db[N] = mul (column sums of a):
 *                                the 64-way row-split partials and their deterministic reduction
 *      AXVS_TEST_GEMM_DGRAD      c[M,K] = beta c + mul a[M,N] b[N,K] + res + res2 (a's row stride lda, 0: N): transpose, then the nt form
 *      AXVS_TEST_GEMM_TN_DIRECT  c[N,K] (row stride ldc) = a[M,N]^T b[M,K] (lda, ldb), M <= 2^31 - 1 rows in one split; rows of b / c at al_b / al_c floats;
 *                                stat_part != NULL: the tile statistics (stat_* as GemmLd, axvs_gemm_nt.h); grp_rows > 0: output row n at
 *                                c + (n / grp_rows) grp_ld + (n % grp_rows) ldc
 *   Epilogue of NT / FWD: (acc + bias) * mul, ReLU, dropout of element row * N + col (drop_thr = floor(p 2^24), drop_scale = 1 / (1 - p); 0: none),
 *   + beta c, + res, + res2 (both [M][ldc]); out16 != NULL: one f16 (kind16 1) / bf16 (2) value per element in the blocked layout [ceil(N/32)][M][32]
 *   instead, rows with zero_rows[row] != 0 written as zeros.  relu = 2: exact GELU in the ReLU's place, relu = 3: exact GELU after the sums (out =
 *   gelu(... + res + res2)) -- the ACT instantiation the query decoders' Linear layers run: three pieces (`exact`, no train_amp), 16-byte rows, K % 4 == 0,
 *   no a2, fp32 rows out; anything else is refused.
 *   variant (out): the instantiation launched last, 0x100 | NS | GEN << 2 | ADD << 3 | F16 << 4 | AFF << 5 | ACT << 6 | SUM << 7 for
 *   tr_gemm_nt_kernel<NS, GEN, ADD, F16, AFF, ACT, SUM> (SUM: the step sums three pieces take where an accumulator contracts over more than 64
 *   k-steps, K > 2048 unsplit; every caller in the library launches these same instantiations: axvs_gemm_nt.hip holds them all),
 *   0x200 | GEN | AMP << 1 | STATS << 3 | GRP << 4 for tr_gemm_tn_kernel<GEN, AMP, STATS, GRP>; 0 when nothing was launched.
 *   scratch: axvs_test_train_gemm_scratch_bytes(t) bytes (0 for NT, FWD and TN_DIRECT).  Refusals before any device work return AXVS_ERR_ARG. */
#define AXVS_TEST_GEMM_NT 0
#define AXVS_TEST_GEMM_FWD 1
#define AXVS_TEST_GEMM_WGRAD 2
#define AXVS_TEST_GEMM_DGRAD 3
#define AXVS_TEST_GEMM_TN_DIRECT 4
typedef struct AxvsTestGemm {
  int op;
  const float* a;
  const float* b;
  float* c;
  long long M;
  int N, K;
  long long lda, ldb, ldc;
  int al_a, al_b, al_c;
  const float* a2;
  const float* aff;
  int aff_rows;
  int ksteps, zsplits;
  const float* bias;
  float mul;
  int relu;
  unsigned drop_seed, drop_site, drop_thr;
  float drop_scale;
  float beta;
  const float* res;
  const float* res2;
  unsigned short* out16;
  int kind16;
  const unsigned char* zero_rows;
  float* db;
  int exact;
  float* stat_part;
  const float* stat_shift;
  int stat_nblk, stat_blk0, stat_rows;
  int grp_rows;
  long long grp_ld;
  int variant;
} AxvsTestGemm;
size_t axvs_test_train_gemm_scratch_bytes(const AxvsTestGemm* t);
int axvs_test_train_gemm(AxvsTestGemm* t, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AXVS_H */
