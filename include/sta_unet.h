/*
 * sta_unet.h — C-ABI of the HBM-bound glue kernels around the cross-attention path (same library,
 * same conventions as sta_xattn.h: raw device pointers, caller-owned buffers, stream-ordered, 0 / STA_E_*).
 *
 * These replace eager-PyTorch sequences in the CALLERS of the hot path (SURVEY.md §8 rows a3/a4/a6:
 * BasicTransformerBlock._forward, SpatialTransformer.forward, ResBlock._forward), each of which is a chain of
 * one-pass-per-op elementwise / normalisation kernels over [2I, C, H, W] or [2I, N, C] activations:
 * pure HBM traffic. One pass per chain instead of one per op. Inference (no autograd) only — the Python
 * wrappers fall back to the eager ops whenever gradients are being recorded.
 *
 * dtype: STA_BF16 / STA_F16 for activations and affine parameters; statistics and arithmetic in fp32.
 */
#ifndef STA_UNET_H
#define STA_UNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * y = act( GroupNorm_G( x + add[b, c] ) * gamma[c] + beta[c] ),  act = SiLU if silu != 0 else identity.
 *   x, y  [B][C][HW] (NCHW, contiguous), HW % 8 == 0, C % G == 0;  add [B][C] fp32 or NULL;  gamma, beta [C].
 * Replaces (reference openaimodel.py ResBlock._forward, util.py GroupNorm32, attention.py:335-337):
 *   `h + emb_out[..., None, None]` (with the producing conv's bias folded into `add`)  ->  GroupNorm32  ->  SiLU.
 * One workgroup per (b, group) slab; slabs up to 64 Ki elements are held in registers between the statistics
 * and the normalisation (one HBM read, exact two-pass variance), larger ones are read twice.
 */
int sta_groupnorm_silu(const void* x, const float* add, const void* gamma, const void* beta, void* y,
                       int B, int C, int HW, int G, float eps, int silu, int dtype, void* stream);

/*
 * y[r][j] = x[r][j] * gelu(x[r][D + j])  (exact erf GELU), x [R][2D], y [R][D], D % 8 == 0.
 * Replaces GEGLU.forward after the projection (attention.py:43-45): chunk + gelu + mul = 3 passes -> 1.
 */
int sta_geglu(const void* x, void* y, long R, int D, int dtype, void* stream);

/*
 * s = x + f + bias (row-broadcast, bias may be NULL; f may be NULL: s = x);  y = LayerNorm(s) * gamma + beta.
 *   x, f, s, y [R][C], C % 8 == 0, C <= 2048. s may be NULL (not stored) or alias x.
 * Replaces `x = attn(norm(x)) + x` followed by the next `norm(x)` of BasicTransformerBlock._forward
 * (attention.py:274-299): residual add and LayerNorm in one pass. One wave per row.
 */
int sta_add_layernorm(const void* x, const void* f, const void* bias, const void* gamma, const void* beta,
                      void* s, void* y, long R, int C, float eps, int dtype, void* stream);

/*
 * sta_add_layernorm with y in QUERY-FRAGMENT order, the private layout between norm2 and the projection-fused
 * cross-attention (attention.py:279-281 -> :178): rows are taken in groups of 16 consecutive rows; group P, fragment
 * s (C/32 per group, 1 KiB each) holds at byte offset (P * C/32 + s) * 1024 + (16 g + c) * 16 the 8 values
 * y[16 P + c][32 s + 8 g .. + 7] — one fragment is one MFMA B operand of sta_xattn_fwd_proj_qfrag (lane = 16 g + c),
 * fetched by one fully coalesced 1-KiB load. Same bytes in total as row-major. s (if not NULL) stays row-major.
 * R % 16 == 0, C % 32 == 0, C <= 1024 (two chunks per lane above 512). Values are bit-identical to sta_add_layernorm's.
 */
int sta_add_layernorm_qfrag(const void* x, const void* f, const void* bias, const void* gamma, const void* beta,
                            void* s, void* y, long R, int C, float eps, int dtype, void* stream);

/*
 * The first half of the block's feed-forward in one pass (csrc/sta_ffgemm.hip):
 *     h = (y W_v^T + b_v) * gelu(y W_g^T + b_g)      GEGLU.forward (attention.py:42-45), exact-erf GELU as sta_geglu
 * y = norm3(x) read in QUERY-FRAGMENT order (sta_add_layernorm_qfrag / sta_to_out_ln_ofrag with y_qfrag), proj.weight
 * [2 * inner][C] re-laid out once per model by sta_ff_geglu_pack_w (sta_ff_geglu_packed_w_bytes bytes; 0 = unsupported:
 * C = 320, inner = 1280 only) and streamed through LDS; the [R][2 * inner] projection never exists in HBM (row-major: a library
 * GEMM that writes it + sta_geglu that reads it back).
 *   bias: [2 * inner] dtype (value half, then gate half) or NULL;  h: [R][inner] dtype, row-major (h_frag = 0) or in the
 *   fragment order of sta_ff_out_res_hfrag (h_frag = 1);  R % 16 == 0
 */
size_t sta_ff_geglu_packed_w_bytes(int C, int inner);
int sta_ff_geglu_pack_w(const void* w, void* packed, int C, int inner, int dtype, void* stream);
int sta_ff_geglu_qfrag(const void* y_qfrag, const void* packed_w, const void* bias, void* h, long R, int C, int inner,
                       int h_frag, int dtype, void* stream);
/*
 * ... and the second half with the block's last residual (attention.py:66-69 and the `+ x` of :299):
 *     out = x + h W2^T + b2
 * h read in FRAGMENT order (sta_ff_geglu_qfrag with h_frag = 1: per 16-row group inner/32 fragments of 1 KiB, lane 16 g + c =
 * row c, channels 32 s + 8 g .. + 7 — one contiguous KiB per store of the first kernel, one coalesced load of this one);
 * net[2].weight [C][inner] re-laid out once by sta_ff_out_pack_w (sta_ff_out_packed_w_bytes bytes; C = 320, inner = 1280 only).
 * Row-major this is a library GEMM + a separate residual add; here h crosses HBM once in each direction as whole KiB.
 *   bias: [C] or NULL;  x, out: [R][C] dtype row-major;  R % 16 == 0
 */
size_t sta_ff_out_packed_w_bytes(int C, int inner);
int sta_ff_out_pack_w(const void* w, void* packed, int C, int inner, int dtype, void* stream);
int sta_ff_out_res_hfrag(const void* h_frag, const void* packed_w, const void* bias, const void* x, void* out, long R, int C,
                         int inner, int dtype, void* stream);

/*
 * The first half of the feed-forward at SD-v1 level 1 in one pass (csrc/sta_ffgemm.hip, the same kernel template): sta_ff_geglu_qfrag's computation,
 * operand orders, GELU and single rounding at C = 640, inner = 2560 (sta_ff_geglu_c640_packed_w_bytes: 0 for any other shape;
 * the packed image differs from sta_ff_geglu_pack_w's: a sub-chunk holds one half of the reduction dimension). h leaves row-major.
 *   bias: [2 * inner] dtype or NULL;  h: [R][inner] dtype;  R % 16 == 0, R * inner * 2 bytes < 4 GiB
 *   max_workgroups: 0 = one persistent workgroup per CU; n > 0 caps the grid (tests: several 256-row passes per workgroup)
 */
size_t sta_ff_geglu_c640_packed_w_bytes(int C, int inner);
int sta_ff_geglu_c640_pack_w(const void* w, void* packed, int C, int inner, int dtype, void* stream);
int sta_ff_geglu_c640_qfrag(const void* y_qfrag, const void* packed_w, const void* bias, void* h, long R, int C, int inner,
                            int max_workgroups, int dtype, void* stream);

/*
 * The front end of the block's self-attention in one pass (csrc/sta_lnqkv.hip):
 *     s = x + bias;  y = LayerNorm(s) * gamma + beta;  q|k = y [Wq'; Wk]^T;  V^T = Wv y^T
 * instead of sta_add_layernorm + two library GEMMs that read y back: y never exists in HBM. bias (may be NULL) and s (may be
 * NULL) as in sta_add_layernorm (s is stored in the activation type and normalised as stored); y is bit-identical to
 * sta_add_layernorm's and is written row-major to y_dbg if that is not NULL (tests; NULL in the product).
 *   wqk: [2C][C], rows 0 .. C-1 = Wq already multiplied by softmax scale * log2 e, rows C .. = Wk;  wv: [C][C];  no biases.
 *   Re-laid out once per model by sta_ln_qkv_pack_w (sta_ln_qkv_packed_w_bytes bytes; 0 = unsupported: C = 320 only).
 *   qk: [R][2C] row-major (columns 0 .. C-1 = q, C .. 2C-1 = k);  vt: [C][R], vt[c][r] = (y Wv^T)[r][c] — the layouts
 *   sta_selfattn_fwd* reads (vt_row_stride = R, vt_batch_stride = N).  R % 16 == 0, R * 2C * 2 bytes < 4 GiB, fp32 accumulation.
 */
size_t sta_ln_qkv_packed_w_bytes(int C);
int sta_ln_qkv_pack_w(const void* wqk, const void* wv, void* packed, int C, int dtype, void* stream);
int sta_ln_qkv(const void* x, const void* bias, const void* gamma, const void* beta, const void* packed_w, void* s, void* y_dbg,
               void* qk, void* vt, long R, int C, float eps, int dtype, void* stream);

/*
 * The 3x3, stride-1, padding-1 convolutions of the UNet trunk on NHWC activations as an implicit GEMM on the MFMAs
 * (ResBlock in_layers / out_layers, openaimodel.py:163-275; Upsample.conv :107-120; csrc/sta_conv.hip):
 *     out = conv(x) + bias + res            (`skip_connection(x) + out_layers(h)` of ResBlock._forward in the epilogue)
 *   x: [B][H >> up2][W >> up2][Cin] dtype;  out: [B][H][W][Cout] dtype;  zeros: >= 2 * Cin bytes of zeros (the padding halo);
 *   bias: [Cout] dtype or NULL;  res: [B][H][W][Cout] dtype or NULL (may not alias out);
 *   stats: NULL, or [B + 1][sta_conv3x3_stats_slots(H, W)][Cout][2] fp32: every wave stores the partial sum and sum of squares of the values it
 *   writes, per output channel (plain stores, fixed slots; the spare image absorbs a half-empty tile); sta_stats_finalize folds them into
 *   [B][Cout][2] — the statistics of the GroupNorm that consumes `out` (sta_groupnorm_silu_nhwc_cstats), whose own statistics pass drops;
 *   packed_w: the weight re-laid out once per model by sta_conv3x3_pack_w (element (o, i, ky, kx) of the source at
 *   o*so + i*si + ky*sy + kx*sx, strides in elements: any memory format of a [Cout][Cin][3][3] tensor);
 *   up2 = 1: the input is the nearest-neighbour 2x upsampling of x (Upsample.forward), read through (y >> 1, x >> 1) — the
 *   upsampled tensor never exists.
 * sta_conv3x3_nhwc_supported: W % 32 == 0 and H % 8 == 0, or W == 16 and H % 16 == 0, or H == W == 8; Cin % 64 == 0; Cout % 160 == 0 or
 * Cout % 128 == 0 (a workgroup owns 160 or 128 output channels);
 * out below 4 GiB. Everything else stays with the library convolution.
 */
int sta_conv3x3_nhwc_supported(int B, int H, int W, int Cin, int Cout);
int sta_conv3x3_stats_slots(int H, int W);
int sta_stats_finalize(const float* partial, float* stats, int B, int slots, int C, void* stream);
size_t sta_conv3x3_packed_w_bytes(int Cin, int Cout);
int sta_conv3x3_pack_w(const void* w, long so, long si, long sy, long sx, void* packed, int Cin, int Cout, int dtype, void* stream);
int sta_conv3x3_nhwc(const void* x, const void* packed_w, const void* zeros, const void* bias, const void* res, void* out, float* stats, int B,
                     int H, int W, int Cin, int Cout, int up2, int dtype, void* stream);

/*
 * The up2 = 1 convolution above as four 2x2 sub-pixel convolutions of the half-resolution tensor, one per output phase (a, b) =
 * (row parity, column parity) — 16 instead of 36 multiply-adds per input pixel, channel and output channel:
 *     out[b][2y + a][2x + b'][o] = bias[o] + res + sum_{u, v in {0,1}, i} W'_ab'[o][i][u][v] * x[b][y + u + a - 1][x + v + b' - 1][i]
 *     W'_ab'[u][v] = sum_{ky in R_a(u)} sum_{kx in R_b'(v)} w[ky][kx],   R_0 = ({0}, {1, 2}),  R_1 = ({0, 1}, {2})
 * (zero outside x; identical to the 3x3 convolution of the upsampled tensor in exact arithmetic). sta_conv3x3_up2_pack_w forms W' in
 * fp32, ky-major and kx-minor, rounds ONCE to dtype and writes 1-KiB A-operand fragments [phase 2a + b'][part][kc][u][v][tile t]: lane
 * (g, c) of a fragment holds W'[16 nt part + 16 t + c][32 kc + 8 g .. + 7][u][v] (nt = 10 or 8 row tiles per part, as for
 * sta_conv3x3_pack_w). The result differs from sta_conv3x3_nhwc(up2 = 1) by that one rounding of every summed weight.
 *   H, W: the OUTPUT size (x is [B][H / 2][W / 2][Cin]); all other arguments as for sta_conv3x3_nhwc;
 *   stats: NULL, or [B + 1][sta_conv3x3_up2_stats_slots(H, W)][Cout][2] (four times the slots of the H / 2 x W / 2 geometry: one per phase).
 * sta_conv3x3_up2_nhwc_supported: H, W even and the H / 2 x W / 2 input one of sta_conv3x3_nhwc's geometries (W / 2 % 32 == 0 and
 * H / 2 % 8 == 0, or W / 2 == 16 and H / 2 % 16 == 0, or 8 x 8); Cin % 64 == 0; Cout % 160 == 0 or Cout % 128 == 0; out below 4 GiB.
 * Everything else stays with sta_conv3x3_nhwc(up2 = 1).
 */
int sta_conv3x3_up2_nhwc_supported(int B, int H, int W, int Cin, int Cout);
int sta_conv3x3_up2_stats_slots(int H, int W);
size_t sta_conv3x3_up2_packed_w_bytes(int Cin, int Cout);
int sta_conv3x3_up2_pack_w(const void* w, long so, long si, long sy, long sx, void* packed, int Cin, int Cout, int dtype, void* stream);
int sta_conv3x3_up2_nhwc(const void* x, const void* packed_w, const void* zeros, const void* bias, const void* res, void* out, float* stats, int B,
                         int H, int W, int Cin, int Cout, int dtype, void* stream);

/*
 * The Linear layers / 1x1 convolutions of the transformer blocks and ResBlock skips as one row GEMM (csrc/sta_gemm.hip; reference
 * CrossAttention.to_q / to_k / to_v / to_out attention.py:158-215, FeedForward :48-69, SpatialTransformer.proj_in / proj_out :322-333,
 * ResBlock.skip_connection openaimodel.py:196-206):
 *     out[r][n] = sum_k x[r][k] w[n][k] + bias[n] + res[r][n]
 *   x: [R][K] dtype (tokens of a [B, N, C] tensor or NHWC pixels);  out, res: [R][N] dtype (res may be NULL, may not alias out);
 *   bias: [N] dtype or NULL;  zeros: >= 2 * K bytes of zeros;  packed_w: sta_linear_rows_pack_w of the weight (element (n, k) at
 *   n*sn + k*sk, strides in elements), once per model.
 * Supported: K % 64 == 0; N % 160 == 0 or N % 128 == 0; out below 4 GiB. Outside autograd only.
 */
int sta_linear_rows_supported(long R, int K, int N);
size_t sta_linear_rows_packed_w_bytes(int K, int N);
int sta_linear_rows_pack_w(const void* w, long sn, long sk, void* packed, int K, int N, int dtype, void* stream);
int sta_linear_rows(const void* x, const void* packed_w, const void* zeros, const void* bias, const void* res, void* out, long R, int K,
                    int N, int dtype, void* stream);
/* ... storing per-(image, slot) partial sums / sums of squares of the stored values to stats [R / rows_per_image + 1][rows_per_image / 64][N][2]
 * fp32 as sta_conv3x3_nhwc does (fold with sta_stats_finalize): rows_per_image % 256 == 0 (every 256-row tile inside one image) */
int sta_linear_rows_stats(const void* x, const void* packed_w, const void* zeros, const void* bias, const void* res, void* out, float* stats,
                          long rows_per_image, long R, int K, int N, int dtype, void* stream);
/* ... with x the column concatenation [xa | xb] of two row tensors ([R][Ka] and [R][K - Ka], Ka % 64 == 0) read in place — the 1x1
 * skip convolution over `torch.cat([h, skip], dim=1)` of the UNet's output blocks (openaimodel.py:740) without the concatenated tensor */
int sta_linear_rows_cat(const void* xa, const void* xb, int Ka, const void* packed_w, const void* zeros, const void* bias, const void* res,
                        void* out, long R, int K, int N, int dtype, void* stream);

/*
 * y = a + b + bias[c]  over NCHW tensors [B][C][HW] (HW % 8 == 0); b and/or bias may be NULL.
 * Replaces a convolution's separate bias pass plus the residual add that follows it
 * (`skip_connection(x) + out_layers(h)`, openaimodel.py ResBlock._forward; `proj_out(x) + x_in`, attention.py:346).
 */
int sta_add_bias_nchw(const void* a, const void* b, const void* bias, void* y, int B, int C, int HW,
                      int dtype, void* stream);

/*
 * NHWC ("channels_last") variants: x, y [B][HW][C]. GroupNorm needs a caller-owned workspace of
 * sta_groupnorm_nhwc_workspace_bytes(B, HW, G) bytes (per-chunk partial moments; written then read inside the
 * call, no initialisation needed). Limits: C % 8 == 0, C / G >= 8 or == 4 (an 8-channel column spans at most two groups), C <= 4096, G <= 64.
 * MIOpen's bf16 convolutions are NHWC kernels; keeping the UNet trunk in NHWC removes the two layout transposes
 * MIOpen wraps around every NCHW convolution and makes 'b c h w -> b (h w) c' (attention.py:338) a view.
 */
size_t sta_groupnorm_nhwc_workspace_bytes(int B, int HW, int G);
int sta_groupnorm_silu_nhwc(const void* x, const float* add, const void* gamma, const void* beta, void* y,
                            void* workspace, int B, int C, int HW, int G, float eps, int silu, int dtype, void* stream);
/* ... of the channel concatenation [xa | xb] (Ca and C - Ca channels, Ca % 8 == 0) read in place: y is the normalised concatenated
 * tensor [B][HW][C]; `torch.cat([h, skip], dim=1)` in front of an output block's first GroupNorm never exists */
int sta_groupnorm_silu_nhwc_cat(const void* xa, const void* xb, int Ca, const float* add, const void* gamma, const void* beta, void* y,
                                void* workspace, int B, int C, int HW, int G, float eps, int silu, int dtype, void* stream);
/* ... with the statistics ALREADY accumulated per channel by the producing kernel (stats_a [B][Ca][2], stats_b [B][C - Ca][2] or NULL
 * with xb; fp32 sum and sum of squares over the HW pixels): one pass instead of two. xb = NULL, Ca = C: a single input tensor. */
int sta_groupnorm_silu_nhwc_cstats(const void* xa, const void* xb, int Ca, const float* stats_a, const float* stats_b, const float* add,
                                   const void* gamma, const void* beta, void* y, int B, int C, int HW, int G, float eps, int silu, int dtype,
                                   void* stream);

/* y = a + b + bias (row-broadcast) over [rows][C] tensors (NHWC activations / token tensors); b, bias may be NULL. */
int sta_add_bias_rows(const void* a, const void* b, const void* bias, void* y, long rows, int C, int dtype, void* stream);

/*
 * Row-wise dynamic quantisation to OCP fp8 (e4m3fn) for the fp8-weight GEMMs of BASELINE configs[4]:
 *   scale[r] = max_c |x[r, c]| / 448 (1 if the row is all zero);  xq[r, c] = e4m3( x[r, c] / scale[r] )
 *   x [rows][C] dtype, xq [rows][C] bytes, scale [rows] fp32;  C % 8 == 0, C <= 5120.
 * Stands in front of the nn.Linear layers of the transformer blocks (reference attention.py:50,69,164-171) when their
 * weights are stored as e4m3 with one fp32 scale per output channel: the GEMM is then hipBLASLt's row-scaled e4m3 GEMM (a
 * library call; non-block-scaled fp8 runs at the 16-bit MFMA rate on gfx950, so this is a weight-memory option, not a
 * rate option: DESIGN.md section 5) and the two scale vectors are applied to its fp32 accumulators.
 */
int sta_quant_rows_fp8(const void* x, void* xq, float* scale, long rows, int C, int dtype, void* stream);

/*
 * MXFP8 (OCP MX v1.0: e4m3fn elements, one e8m0 scale byte per 32 consecutive K elements) for the transformer-block Linears on
 * gfx950's block-scaled MFMA (v_mfma_scale_f32_32x32x64_f8f6f4: twice the 16-bit rate). csrc/sta_mxfp8.hip.
 *
 * sta_mx8_quant_rows: x [rows][K] dtype -> xq [rows][K] e4m3fn bytes, xs [rows][K/32] e8m0 bytes (both plain row-major); K % 32 == 0,
 *   x and xq 16-byte aligned. Per 32-block: X = 2^clamp(floor(log2 amax) - 8, -127, 127), xq = e4m3fn(x / X) rounded to nearest even
 *   and saturated to +-448, xs = log2 X + 127. An all-zero block: codes 0, scale byte 127 (X = 1).
 * sta_mx8_gemm: out[m][n] = sum_k P[m][k] 2^(ps[m][k/32] - 127) * Q[n][k] 2^(qs[n][k/32] - 127), fp32 accumulation.
 *   P [M][K], Q [N][K] e4m3fn (16-byte aligned), ps [M][K/32], qs [N][K/32] e8m0; K % 32 == 0 (K % 64 == 32 runs a zero half-step).
 *   flags 0: out [M][ldo] dtype, out[m][n] = acc * col_scale[n] + bias[n] (col_scale fp32 [N], bias dtype [N]; either may be NULL).
 *   flags STA_MX8_GEGLU: Q holds the GEGLU projection packed in groups of 64 rows (32 value rows h .. h+31, then the gate rows
 *     H + h .. H + h + 31; H = N / 2, N % 64 == 0) and bias [N] packed the same way; out [M][ldo] dtype with
 *     out[m][h] = value * gelu_erf(gate) (reference attention.py:47-49), ldo % 4 == 0.
 *   flags STA_MX8_GEGLU | STA_MX8_MX_OUT: the same result as MXFP8 — out [M][H] e4m3fn bytes, out_scale [M][H/32] e8m0 (ldo == H),
 *     quantised from the 16-bit-rounded GEGLU values by the sta_mx8_quant_rows rule (same scales; codes bit-identical in bf16).
 */
enum { STA_MX8_GEGLU = 1, STA_MX8_MX_OUT = 2 };
int sta_mx8_quant_rows(const void* x, void* xq, void* xs, long rows, int K, int dtype, void* stream);
int sta_mx8_gemm(const void* p, const void* ps, const void* q, const void* qs, void* out, void* out_scale, const void* bias,
                 const float* col_scale, long M, int N, int K, long ldo, int flags, int dtype, void* stream);

/*
 * Input gradients of the glue kernels, for the tracked (weight-optimisation) epochs (plms.py:220-277): the blend weights
 * are the only leaf and every model parameter is frozen, so each op needs d(input) only. csrc/sta_unet_bwd.hip.
 *
 * sta_groupnorm_silu_nhwc_bwd: dx of y = act(GroupNorm_G(x + add) * gamma + beta) on NHWC activations. fwd_workspace is the
 *   workspace the FORWARD call filled for the same x (its per-chunk moments; mean / rstd are rebuilt from it), bwd_workspace
 *   another sta_groupnorm_nhwc_workspace_bytes(B, HW, G) bytes. Same limits as the forward. (add gets no gradient: the
 *   timestep embedding does not depend on the blend weights.)
 * sta_geglu_bwd: dx [R][2D] of y = x[:, :D] * gelu(x[:, D:]) given dy [R][D].
 * sta_layernorm_bwd: ds = dLayerNorm(s)^T dy + dres for y = LayerNorm(s) * gamma + beta; s, dy, dres (may be NULL: the
 *   gradient reaching s through the residual connection), ds [R][C]; C % 8 == 0, C <= 2048.
 */
int sta_groupnorm_silu_nhwc_bwd(const void* x, const float* add, const void* gamma, const void* beta, const void* dy, void* dx,
                                const void* fwd_workspace, void* bwd_workspace, int B, int C, int HW, int G, float eps, int silu,
                                int dtype, void* stream);
/*
 * The VAE encoder's Downsample (reference model.py:60-79: F.pad(x, (0, 1, 0, 1)) then a 3x3 convolution with stride 2) on NHWC
 * activations, without the padded tensor (csrc/sta_encode.hip):
 *     out[b][y][x][o] = bias[o] + sum_{ky, kx, i} w[o][i][ky][kx] * x[b][2y + ky][2x + kx][i]      (x = 0 at row >= H or col >= W)
 *   x: [B][H][W][Cin] dtype (H, W: the INPUT size);  out: [B][H / 2][W / 2][Cout] dtype;  zeros: >= 2 * Cin bytes of zeros;
 *   bias: [Cout] dtype or NULL;  packed_w: sta_conv3x3_pack_w's image of the [Cout][Cin][3][3] weight (its 128-channel parts);
 *   stats: NULL, or [B + 1][sta_conv3x3_s2_stats_slots(H, W)][Cout][2] fp32 partial sums / sums of squares of the stored values, folded by
 *   sta_stats_finalize into the statistics of the GroupNorm that consumes `out` (the next ResnetBlock's norm1), as for sta_conv3x3_nhwc.
 * sta_conv3x3_s2_nhwc_supported: H % 16 == 0, W % 32 == 0 (8 x 16 output tiles); Cin == Cout (Downsample), a multiple of 128 and not of
 * 160; x below 4 GiB. The SD-v1 encoder's three Downsample shapes at 512^2 and 768^2 are inside (each measured faster than F.pad + the
 * library convolution). Everything else stays with F.pad + the library convolution.
 */
int sta_conv3x3_s2_nhwc_supported(int B, int H, int W, int Cin, int Cout);
int sta_conv3x3_s2_stats_slots(int H, int W);
int sta_conv3x3_s2_nhwc(const void* x, const void* packed_w, const void* zeros, const void* bias, void* out, float* stats, int B, int H, int W,
                        int Cin, int Cout, int dtype, void* stream);

/*
 * From the encoder's conv_out result to the first UNet call's input of img2img, per latent pixel, in fp32 (csrc/sta_encode.hip):
 *     moments    = quant_w h + quant_b                               quant_conv, 8x8 1x1 (reference autoencoder.py:324-328)
 *     mean       = moments[0:4],  logvar = clamp(moments[4:8], -30, 20)
 *     z0         = scale_factor (mean + exp(logvar / 2) n_post)       DiagonalGaussianDistribution.sample + get_first_stage_encoding
 *     x          = sqrt_a z0 + sqrt_1ma n_enc                         DDIMSampler.stochastic_encode
 *   h: [B][hw][8] dtype (NHWC, 16-byte aligned);  quant_w [8][8], quant_b [8] fp32;  n_post, n_enc, x, z0: [B][4][hw] fp32 (z0 may be NULL);
 *   xin: NULL, or [2B][4][hw] dtype = (x, x) per image, the first UNet call's CFG input pair (bitwise the 16-bit rounding of x).
 */
int sta_vae_encode_step(const void* h, const float* quant_w, const float* quant_b, const float* n_post, const float* n_enc, float* x, float* z0,
                        void* xin, long B, long hw, float scale_factor, float sqrt_a, float sqrt_1ma, int dtype, void* stream);

int sta_geglu_bwd(const void* x, const void* dy, void* dx, long R, int D, int dtype, void* stream);
int sta_layernorm_bwd(const void* s, const void* gamma, const void* dy, const void* dres, void* ds, long R, int C, float eps,
                      int dtype, void* stream);

/*
 * One step of the DPM-Solver++(2M) / DDIM samplers after a CFG UNet call, in one pass (csrc/sta_sampler.hip):
 *     e      = eps[2i] + scale (eps[2i+1] - eps[2i])         guided noise (dpm_solver.py:345-346, ddim.py:176-177)
 *     m      = (x - sigma_t e) / alpha_t                      data prediction at the call's time (dpm_solver.py:393, ddim.py:190)
 *     x_next = c_x x + c_m m + c_p m_prev + c_e e + c_n noise
 * DPM-Solver++ multistep, order 2 (dpm_solver.py:755-790, predict_x0, solver_type "dpm_solver"):
 *     c_x = sigma_next / sigma_t, c_m = -alpha_next (e^-h - 1)(1 + 1/(2 r0)), c_p = alpha_next (e^-h - 1)/(2 r0), c_e = c_n = 0;
 *     first-order steps (dpm_solver.py:525-530) have c_p = 0.
 * DDIM (ddim.py:180-205): c_m = sqrt(a_prev), c_e = sqrt(1 - a_prev - sigma^2), c_n = sigma, c_x = c_p = 0.
 *   eps: [2b][n] dtype, uncond / cond rows adjacent per image;  x, m_prev, noise, x_next, m: [b][n] fp32 (m_prev / noise may be NULL
 *   when their coefficient is 0);  xin: NULL, or [2b][n] dtype = (x_next, x_next) per image, the next UNet call's input.
 *   n % 8 == 0; every pointer 16-byte aligned; outputs may not alias inputs.
 * sta_sampler_step_bwd: the step is linear in (eps, x, m_prev). Given g_xn = dL/dx_next and g_m = dL/dm (NULL = 0), writes
 *   g_x = dL/dx [b][n] fp32, g_eps = dL/deps [2b][n] dtype, g_mprev = dL/dm_prev [b][n] fp32 (NULL = not written). No noise gradient.
 */
int sta_sampler_step(const void* eps, const float* x, const float* m_prev, const float* noise, float* x_next, float* m, void* xin,
                     long b, long n, float scale, float sigma_t, float alpha_t, float c_x, float c_m, float c_p, float c_e, float c_n,
                     int dtype, void* stream);
int sta_sampler_step_bwd(const float* g_xn, const float* g_m, float* g_x, void* g_eps, float* g_mprev, long b, long n, float scale,
                         float sigma_t, float alpha_t, float c_x, float c_m, float c_p, float c_e, int dtype, void* stream);

/*
 * Layout-guided inpainting (csrc/sta_inpaint.hip). Before UNet call i at integer timestep t_i the kept region is re-noised
 * (reference ddim.py:144-147, plms.py:232-235):
 *     x <- keep (q_a x0 + q_b n_i) + (1 - keep) x,   q_a = sqrt(acp[t_i]), q_b = sqrt(1 - acp[t_i]) (float32 roots, host)
 *   keep: [b][hw] fp32 in [0, 1], 1 = keep the original, broadcast over the n / hw channels;  x0, qnoise: [b][n] fp32, constants.
 * sta_sampler_step_masked: everything sta_sampler_step does for call i, then the blend OF CALL i + 1 (q_a, q_b of t_{i+1}, qnoise =
 *   n_{i+1}) on x_next: writes the blended x_next, the unchanged m and xin = the 16-bit pair of the blended state. Where keep == 0 the
 *   result is bit-equal to sta_sampler_step's. The last call of a trajectory takes sta_sampler_step (no blend after the last step).
 * sta_sampler_step_masked_bwd: sta_sampler_step_bwd with g_xn (the gradient of the blended state) multiplied by (1 - keep).
 * sta_latent_blend: the blend alone (first call): x, x0, keep, noise -> x_out [b][n] fp32 and xin (NULL = not written). No backward:
 *   the start latent is a constant.
 * sta_image_composite: out = keep_px orig + (1 - keep_px) clamp((dec + 1) / 2, 0, 1) over [b][3][hw]; dec, out: dtype; orig [b][3][hw],
 *   keep_px [b][hw]: fp32; fp32 arithmetic, rounded to dtype once.
 * sta_image_composite_bwd: g_dec = 0.5 (1 - keep_px) g where -1 <= dec <= 1 (inclusive, as torch.clamp's gradient), else 0; g, g_dec: dtype.
 * Rules (STA_E_ARG with text, nothing launched): hw % 8 == 0 and n % hw == 0 (a lane's 8 elements then never straddle a channel: its mask
 * values are 32 contiguous bytes at (8 col) % hw); every pointer 16-byte aligned; x0, keep, qnoise / noise non-NULL; alpha_t != 0.
 */
int sta_sampler_step_masked(const void* eps, const float* x, const float* m_prev, const float* noise, const float* x0, const float* keep,
                            const float* qnoise, float* x_next, float* m, void* xin, long b, long n, long hw, float scale, float sigma_t,
                            float alpha_t, float c_x, float c_m, float c_p, float c_e, float c_n, float q_a, float q_b, int dtype,
                            void* stream);
int sta_sampler_step_masked_bwd(const float* g_xn, const float* g_m, const float* keep, float* g_x, void* g_eps, float* g_mprev, long b,
                                long n, long hw, float scale, float sigma_t, float alpha_t, float c_x, float c_m, float c_p, float c_e,
                                int dtype, void* stream);
int sta_latent_blend(const float* x, const float* x0, const float* keep, const float* noise, float* x_out, void* xin, long b, long n, long hw,
                     float q_a, float q_b, int dtype, void* stream);
int sta_image_composite(const void* dec, const float* orig, const float* keep_px, void* out, long b, long hw, int dtype, void* stream);
int sta_image_composite_bwd(const void* g, const void* dec, const float* keep_px, void* g_dec, long b, long hw, int dtype, void* stream);

/*
 * Attention-guided sampling (csrc/sta_guide.hip): the latent steps down the gradient of the attention-layout energy before a UNet call.
 * The UNet's input is the 16-bit CFG pair (rows 2i, 2i + 1 = the same latent), so autograd hands the gradient back as a pair as well.
 *   g: [2b][n] dtype, the gradient w.r.t. the input pair;  x, x_out: [b][n] fp32;  keep: [b][hw] fp32 or NULL (inpainting: the kept region
 *   is not guided; NULL = factor 1), broadcast over the n / hw channels;  step: [b] fp32;  xin: [2b][n] dtype or NULL;  stats: [b] fp32 or NULL.
 * Per image i, fp32 arithmetic:
 *     d_j   = (g[2i][j] + g[2i+1][j]) (1 - keep[i][j mod hw])
 *     rms_i = sqrt(sum_j d_j^2 / n)
 *     s_i   = normalize ? step[i] / rms_i : step[i] inv_scale            (inv_scale undoes the loss scale of a 16-bit backward)
 *     x_out = x - s_i d  if rms_i is finite and > 0, else x_out = x bit for bit (the image is skipped: a zero or non-finite gradient)
 *     xin   = (x_out, x_out) rounded once to dtype, rows 2i and 2i + 1;  stats[i] = rms_i (non-finite or 0 marks a skipped image)
 * One launch, no atomics: every workgroup of an image reduces the whole image's gradient in the same fixed order, so the result is
 * bit-reproducible from launch to launch and an image's outputs depend on that image's inputs alone.
 * Rules (STA_E_ARG with text, nothing launched): g, x, step, x_out non-NULL; n % 8 == 0, hw % 8 == 0, n % hw == 0 (also with keep == NULL);
 * g, x, keep, x_out, xin 16-byte aligned (step, stats: 4-byte); no output may overlap an input or another output.
 */
int sta_latent_guide(const void* g, const float* x, const float* keep, const float* step, float* x_out, void* xin, float* stats, long b, long n,
                     long hw, int normalize, float inv_scale, int dtype, void* stream);

/*
 * Wide canvases sampled as overlapping square windows, the MultiDiffusion way (csrc/sta_window.hip). The canvas latent is [P][C][Hc][Wc];
 * every UNet call sees T = ny nx square windows of side s of each canvas as T images of one CFG batch. Window w = j nx + i has its corner
 * at (oy[j], ox[i]); the UNet batch is canvas-major, then window, then (uncond, cond): row 2 (p T + w) + r.
 *   ny, nx, oy, ox, s: the grid; oy / ox are HOST arrays of ny / nx offsets (copied into the kernel arguments: no device-side table).
 * Rules (STA_E_ARG with text, nothing launched): non-NULL 16-byte aligned tensors, non-NULL oy / ox; s, Hc, Wc and every offset multiples
 * of 8 (a lane's 8 elements never straddle a window edge), 8 <= s <= Hc, Wc; 1 .. STA_MAX_WINDOW_OFFSETS offsets per axis, the first 0,
 * ascending, consecutive ones at most s apart and the last window ending at the canvas edge (no gap); dtype STA_BF16 / STA_F16.
 * Every canvas element is owned by one lane that visits its covering windows in ascending w: no atomics, no LDS, bit-reproducible.
 *
 * sta_window_split: src [P rows][C][Hc][Wc] -> xin [2 P T][C][s][s] dtype. rows = 1: canvas states, written to both rows of every window's
 *   pair; rows = 2: an input pair tensor, row r to row r. src_dtype: STA_SRC_F32 (rounded to nearest even once) or dtype itself (copied).
 * sta_window_fuse: eps [2 P T][C][s][s] dtype -> out [2 P][C][Hc][Wc] dtype: per element the covering windows' values summed in fp32 in
 *   ascending w, starting from the first one's value, divided by their count (IEEE fp32 division), rounded to nearest even once.
 * sta_sampler_step_windows: sta_sampler_step on the two overlap means of eps (fp32, NOT rounded to dtype), the same expressions in the
 *   same order; x, m_prev, noise, x_next, m: [P][C][Hc][Wc] fp32 (m_prev / noise may be NULL); xin: NULL, or [2 P T][C][s][s] dtype =
 *   the rounded x_next in both rows of every covering window, the next UNet call's input. With T = 1 bit-equal to sta_sampler_step.
 *
 * Inpainting and outpainting on a canvas: the blend of sta_sampler_step_masked / sta_latent_blend (one device definition, csrc/
 * sta_blend_dev.h) with canvas-shaped constants: x0, qnoise / noise [P][C][Hc][Wc] fp32, keep [P][Hc][Wc] fp32 in [0, 1] (1 = keep the
 * original), broadcast over the channels. All three are required (STA_E_ARG when NULL) and 16-byte aligned like every other tensor.
 * sta_sampler_step_windows_masked: sta_sampler_step_windows for call i, then the blend OF CALL i + 1 (q_a, q_b, qnoise of that call) on
 *   x_next: x_next = keep (q_a x0 + q_b qnoise) + (1 - keep) t, and where keep == 0 the unblended t bit for bit (= sta_sampler_step_windows).
 *   m is the unblended data prediction. xin: NULL, or the rounded BLENDED x_next in both rows of every covering window. With T = 1
 *   bit-equal to sta_sampler_step_masked. The last call of a trajectory takes sta_sampler_step_windows (no blend after the last step).
 * sta_window_blend: the blend of the first call, x_out = keep (q_a x0 + q_b noise) + (1 - keep) x on [P][C][Hc][Wc] fp32, and xin (NULL =
 *   not written) = the windows of the rounded result: sta_latent_blend and sta_window_split (rows = 1) in one launch.
 *
 * Wrap-around canvases (360 degree panoramas: x closes on itself; tileable images: both axes): every entry point of this section takes
 * `int wrap` directly after s. wrap: bit 0 = the x axis (columns, length Wc) is cyclic, bit 1 = the y axis (rows, length Hc); wrap = 0 is
 * the clamped grid above. On a cyclic axis of length L the window at offset o covers the canvas positions (o + d) mod L, d = 0 .. s - 1: a
 * window may run over the seam, and the first and the last column share windows. The visiting order (ascending w), the sum from the first
 * covering window's value and the division by the count are unchanged.
 * Rules of a cyclic axis (STA_E_ARG with text, nothing launched; a non-cyclic axis keeps the rules above): wrap in 0 .. 3; 1 ..
 * STA_MAX_WINDOW_OFFSETS offsets, the first 0, ascending multiples of 8, every offset < L (o + s <= L is NOT required), consecutive ones at
 * most s apart, and the ring closes without a gap: L - o[n - 1] <= s; s <= L (a window covers an element at most once).
 *
 * img2img on a canvas: sta_vae_encode_step_windows goes from the encoder's conv_out result on the WHOLE canvas to the canvas state and the
 * first UNet call's window inputs in one launch: per latent pixel exactly sta_vae_encode_step's arithmetic (one device definition, csrc/
 * sta_encode_dev.h: quant_conv, logvar clamped to [-30, 20], z0 = scale_factor (mean + exp(logvar / 2) n_post), x = sqrt_a z0 + sqrt_1ma
 * n_enc), then sta_window_split (rows = 1, STA_SRC_F32) of x. Bit-equal to those two launches one after the other.
 *   h: [P][Hc][Wc][8] dtype (NHWC, 16-byte aligned);  quant_w [8][8], quant_b [8] fp32;  n_post, n_enc, x, z0: [P][4][Hc][Wc] fp32 (z0 may be
 *   NULL);  xin: NULL, or [2 P T][4][s][s] dtype = the rounded x in both rows of every covering window's pair, in sta_window_split's order.
 * Rules (STA_E_ARG with text, nothing launched): the grid rules above (C = 4); every tensor but z0 / xin non-NULL; h, n_post, n_enc, x, z0,
 * xin 16-byte aligned; wrap in 0 .. 3; dtype STA_BF16 / STA_F16.
 *
 * Attention guidance on a canvas: sta_latent_guide_windows is sta_latent_guide carried to a canvas, one launch from the gradient w.r.t. the
 * WINDOW input pairs to the updated canvas state and the next call's window inputs. The windows are sta_window_split (rows = 1) of the canvas
 * state, so the gradient w.r.t. the state is the split's adjoint: a SUM over the covering windows and both pair rows (not the overlap mean).
 *   g: [2 P T][C][s][s] dtype;  x, x_out: [P][C][Hc][Wc] fp32;  keep: [P][Hc][Wc] fp32 or NULL (the kept region is not guided), broadcast over
 *   the channels;  step, count: [P] fp32;  xin: NULL, or [2 P T][C][s][s] dtype;  stats: [P] fp32 or NULL.
 * Per canvas p, fp32 arithmetic:
 *     d[c][y][x] = (sum over the windows w covering (y, x), ascending w, of (g[2 (p T + w)] + g[2 (p T + w) + 1])[c][dy][dx]) (1 - keep[p][y][x])
 *                  (each window's g_u + g_c is formed first; the sum starts from the first covering window's value)
 *     rms_p = sqrt(sum d^2 / count[p])       count[p]: the number of canvas elements (channels included) that can receive gradient, the
 *                                            host's; C Hc Wc on a canvas whose windows all contribute; 0 leaves the canvas untouched
 *     s_p   = normalize ? step[p] / rms_p : step[p] inv_scale
 *     x_out = x - s_p d  if rms_p is finite and > 0, else x_out = x bit for bit;  stats[p] = rms_p
 *     xin   = sta_window_split (rows = 1) of x_out: the rounded vector in both rows of every covering window's pair
 * Every workgroup of a canvas reduces the whole canvas's sum of squares in the same fixed order (no atomics, no hand-off): bit-reproducible,
 * a canvas's outputs depend on that canvas's inputs alone. With T = 1 bit-equal to sta_latent_guide (b = P, n = C s s, hw = s s).
 * Rules (STA_E_ARG with text, nothing launched): the grid rules above; g, x, step, count, x_out non-NULL; g, x, keep, x_out, xin 16-byte
 * aligned (step, count, stats: 4-byte); no output may overlap an input or another output; wrap in 0 .. 3; dtype STA_BF16 / STA_F16.
 *
 * The hi-res fix on a canvas: sta_latent_upscale_step_windows goes from a smaller latent (the x0 of a finished trajectory, a square image or
 * a canvas) to the upscaled canvas state, noised to the decode's start, and the first UNet call's window inputs in one launch.
 *   z: [P][C][h][w] fp32;  noise, x, z_up: [P][C][Hc][Wc] fp32 (z_up may be NULL);  xin: NULL, or [2 P T][C][s][s] dtype = the rounded x in
 *   both rows of every covering window's pair, in sta_window_split's order.
 * Per canvas element and axis (output length L_out, source length L_in), fp32, every operation rounded on its own (no contraction):
 *     scale = (float)L_in / (float)L_out;  src = (d + 0.5f) * scale - 0.5f
 *     clamped axis: src = max(src, 0), i0 = floor(src), i1 = min(i0 + 1, L_in - 1)
 *     wrapped axis (a set bit of wrap): no clamp, i0 = floor(src), both taps modulo L_in (the source is itself closed on that axis)
 *     l1 = src - i0, l0 = 1 - l1
 *     z_up = l0y (l0x z00 + l1x z01) + l1y (l0x z10 + l1x z11)
 *     x    = sqrt_a z_up + sqrt_1ma noise      (the noising of sta_vae_encode_step: one device definition, csrc/sta_encode_dev.h)
 * which is torch.nn.functional.interpolate(mode="bilinear", align_corners=False) on the clamped axes. No LDS, no atomics, one writer per
 * element.
 * Rules (STA_E_ARG with text, nothing launched): z, noise, x non-NULL; the grid rules above; h, w positive multiples of 8; Hc >= h and
 * Wc >= w (upscale only); z, noise, x, z_up, xin 16-byte aligned; wrap in 0 .. 3; dtype STA_BF16 / STA_F16.
 */
#define STA_MAX_WINDOW_OFFSETS 16
#define STA_SRC_F32 2
int sta_window_split(const void* src, void* xin, long P, int rows, int C, int Hc, int Wc, int ny, int nx, const int* oy, const int* ox, int s,
                     int wrap, int src_dtype, int dtype, void* stream);
int sta_window_fuse(const void* eps, void* out, long P, int C, int Hc, int Wc, int ny, int nx, const int* oy, const int* ox, int s, int wrap,
                    int dtype, void* stream);
int sta_sampler_step_windows(const void* eps, const float* x, const float* m_prev, const float* noise, float* x_next, float* m, void* xin, long P,
                             int C, int Hc, int Wc, int ny, int nx, const int* oy, const int* ox, int s, int wrap, float scale, float sigma_t,
                             float alpha_t, float c_x, float c_m, float c_p, float c_e, float c_n, int dtype, void* stream);
int sta_sampler_step_windows_masked(const void* eps, const float* x, const float* m_prev, const float* noise, const float* x0,
                                    const float* keep, const float* qnoise, float* x_next, float* m, void* xin, long P, int C, int Hc, int Wc,
                                    int ny, int nx, const int* oy, const int* ox, int s, int wrap, float scale, float sigma_t, float alpha_t,
                                    float c_x, float c_m, float c_p, float c_e, float c_n, float q_a, float q_b, int dtype, void* stream);
int sta_window_blend(const float* x, const float* x0, const float* keep, const float* noise, float* x_out, void* xin, long P, int C, int Hc,
                     int Wc, int ny, int nx, const int* oy, const int* ox, int s, int wrap, float q_a, float q_b, int dtype, void* stream);
int sta_vae_encode_step_windows(const void* h, const float* quant_w, const float* quant_b, const float* n_post, const float* n_enc, float* x,
                                float* z0, void* xin, long P, int Hc, int Wc, int ny, int nx, const int* oy, const int* ox, int s, int wrap,
                                float scale_factor, float sqrt_a, float sqrt_1ma, int dtype, void* stream);
int sta_latent_guide_windows(const void* g, const float* x, const float* keep, const float* step, const float* count, float* x_out, void* xin,
                             float* stats, long P, int C, int Hc, int Wc, int ny, int nx, const int* oy, const int* ox, int s, int wrap,
                             int normalize, float inv_scale, int dtype, void* stream);
int sta_latent_upscale_step_windows(const float* z, const float* noise, float* x, float* z_up, void* xin, long P, int C, int h, int w, int Hc,
                                    int Wc, int ny, int nx, const int* oy, const int* ox, int s, int wrap, float sqrt_a, float sqrt_1ma, int dtype,
                                    void* stream);

/*
 * The image front end of the CLIP fidelity loss (csrc/sta_clip.hip): the 224^2 views CLIP ViT-B/32 is fed, written directly as the rows
 * of its patch-embedding GEMM, and the gradient of the image from the gradient of those rows.
 *   img:   [B][3][H][W] fp32 in [0, 1] (the clamped decoder output);
 *   boxes: [n_views][5] int32 (image, y1, y2, x1, x2) in DEVICE memory, boxes_host the same table in HOST memory (the rules below are
 *          checked on it before the launch; the kernels read the device copy and clamp what they read into the image);
 *   out:   [n_views][49][3072] dtype, 16-byte aligned: row = patch (py, px) of the 7 x 7 grid, column = (c, dy, dx), the column order of
 *          visual.conv1.weight.view(width, 3072). View pixel (c, Y, X) is row (Y / 32) 7 + X / 32, column c 1024 + (Y % 32) 32 + X % 32.
 * A view whose box is the whole image is the GLOBAL view, AvgPool2d(p)(Upsample(scale_factor=7, nearest)(x)) with p = 7 H / 224 (16 at
 * 512^2, the reference's constant, plms.py:36-44): integer overlap weights over p^2, fp32. Any other box is a CROP view:
 * F.interpolate(x[:, y1:y2, x1:x2], (224, 224), mode="bilinear", align_corners=False), source index clamped inside the box. The result is
 * rounded to dtype once.
 * sta_clip_views_bwd: dout [n_views][49][3072] dtype -> dimg [B][3][H][W] fp32, every element written (no memset, no atomics: a gather,
 * bitwise reproducible). boxes must be grouped by image, in image order.
 * Rules (STA_E_UNSUP / STA_E_ARG with text): H == W, H % 32 == 0, 256 <= H <= 1024 (below 224 the pool window is narrower than an upsampled
 * pixel and a source pixel would feed more than 2 x 2 global outputs); every box inside the image and at least 2 x 2; n_views 49 3072 < 2^31.
 */
int sta_clip_views(const float* img, const int* boxes, const int* boxes_host, void* out, int B, int H, int W, int n_views, int out_dtype,
                   void* stream);
int sta_clip_views_bwd(const void* dout, const int* boxes, const int* boxes_host, float* dimg, int B, int H, int W, int n_views, int dtype,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
