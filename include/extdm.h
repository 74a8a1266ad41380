/* ExtDM sampling path — C ABI of libextdm_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary under the package's Python mirror of the reference API.
 * Plain pointers and sizes only; every tensor is fp32, contiguous NCDHW
 * (`b c t h w`) and caller-owned; device pointers live on the handle's device.
 * Every function returns 0 on success or a negative status; the message is in
 * extdm_last_error() (thread-local), which the Python layer raises as
 * RuntimeError. A handle is not thread-safe; different handles may run
 * concurrently (one per device / process).
 *
 * Reference interfaces replaced (file:line in the reference tree):
 *   extdm_create / extdm_load_weight / extdm_finalize
 *       Unet3D.__init__ + load_state_dict          DenoiseNet_..._u12.py:864-1003,
 *                                                   _ada.py:865-1018, _ada_u22.py:1009-1170,
 *                                                   _wo_ref_adaptor_cross_multi.py:755-904
 *       GaussianDiffusion.__init__ buffers          Diffusion.py:52-122
 *       Generator.__init__ (decoder half)           LFAE/generator.py:26-62
 *   extdm_unet_forward   Unet3D.forward / forward_with_cond_scale(cond_scale=1)
 *                                                   u12:1005-1086, ada:1020-1089,
 *                                                   ada_u22:1172-1306 (path=0), wo_ref:906-967
 *   extdm_sample         GaussianDiffusion.p_sample_loop / ddim_sample
 *                                                   Diffusion.py:180-189, 209-258
 *   extdm_sampler_step   one p_sample / DDIM update given eps
 *                                                   Diffusion.py:145-177, 231-255
 *   extdm_sampler_step_t the same update with a per-sample t (p_sample with a mixed t)
 *   extdm_sampler_step_hist  one DPM-Solver++(2M) update given eps (no reference counterpart)
 *   extdm_q_sample       GaussianDiffusion.q_sample                 Diffusion.py:276-284
 *   extdm_x0_loss        p_losses after the denoiser (loss, thresholded x0)
 *                                                   Diffusion.py:294-319
 *   extdm_p_losses       GaussianDiffusion.p_losses / forward       Diffusion.py:286-327
 *   extdm_abs_diff_sum   nn.L1Loss()(pred_frames, fake_out_vid) (rec_loss, rec_warp_loss)
 *                                                   VideoFlowDiffusion_multi_w_ref.py:212-213
 *   extdm_decode         Generator.forward_with_flow   LFAE/generator.py:152-206
 *   extdm_region_params  RegionPredictor.forward       LFAE/region_predictor.py:62-150
 *   extdm_bg_params      BGMotionPredictor.forward     LFAE/bg_motion_predictor.py:47-64
 *   extdm_flow_predict   PixelwiseFlowPredictor.forward LFAE/pixelwise_flow_predictor.py:106-153
 *   extdm_bottleneck     Generator.forward_bottle      LFAE/generator.py:95-102
 *   extdm_frame_metrics  img_psnr / calculate_ssim_function per frame (the per-frame
 *                        loops of calculate_psnr2 / calculate_ssim2, valid.py:226-233)
 *                                                   metrics/calculate_psnr.py:6-15,
 *                                                   metrics/calculate_ssim.py:6-41
 *   extdm_fvd_create / _load_weight / _finalize
 *                        InceptionI3d.__init__ + load_state_dict      metrics/pytorch_i3d.py:172-303
 *   extdm_fvd_features   InceptionI3d.forward / extract_features      metrics/pytorch_i3d.py:305-322
 *   extdm_fvd_endpoint   the same forward cut after a VALID_ENDPOINTS name (parity hook)
 *   extdm_fvd_preprocess trans + preprocess_single   metrics/calculate_fvd.py:6-14, fvd.py:161-187
 *
 * Limits: a denoiser sees tc + tp model frames (WO_REF: tc - 1 + tp); the temporal attention
 * holds one pixel's frames in at most 64 token slots, so extdm_finalize refuses more than 64
 * model frames ("temporal attention over more than 64 frames"). Up to 32 frames run the
 * 8 / 16 / 32-slot kernels, 33..64 frames (e.g. KTH 10 -> 40) the 64-slot ones.
 */
#ifndef EXTDM_H
#define EXTDM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ExtdmHandle ExtdmHandle;

/* Unet3D denoiser variants, one per reference module:
 *   U12      DenoiseNet_STWAtt_w_w_ref_adaptor_cross_multi_traj_u12.py (== _u22.py): BAIR
 *   ADA      ..._traj_ada.py: KTH (window 4x4x4, dim_head 16, cond_adaptor + cond_temporal_attn)
 *   ADA_U22  ..._traj_ada_u22.py: Cityscapes / UCF (b1,b2,STW,STW,adaptor,temporal per level)
 *   WO_REF   DenoiseNet_STWAtt_w_wo_ref_adaptor_cross_multi.py: SMMNIST (tc-1 cond frames,
 *            cond_fea at latent resolution, fea: [B,fea_ch,tc-1+tp,L,L]) */
enum { EXTDM_ARCH_U12 = 0, EXTDM_ARCH_ADA = 1, EXTDM_ARCH_ADA_U22 = 2, EXTDM_ARCH_WO_REF = 3 };
/* DPMPP: DPM-Solver++(2M), the data-prediction second-order multistep solver of Lu et al. 2022.
 * Not part of the reference; deterministic (no noise term). */
enum { EXTDM_SAMPLER_DDPM = 0, EXTDM_SAMPLER_DDIM = 1, EXTDM_SAMPLER_DPMPP = 2 };
/* Arithmetic of the direct convolutions (every tensor stays fp32):
 *   FP32   v_mfma_f32_32x32x2_f32 (exact fp32 products and sums)
 *   F16X3  fp32 operands split as hi + lo fp16 pairs, three fp16 MFMAs per product
 *          (lo*hi + hi*lo + hi*hi) into fp32 accumulators: fp32-level error, 5.3x
 *          the fp32 MFMA rate. Needs |activation| < 65504 at conv inputs; a value
 *          outside raises the range flag (extdm_range_flag; extdm_sample fails).
 *   BF16_ATTN  F16X3 convolutions; the attention QK^T / PV contractions of the STW
 *          window and temporal layers on bf16 MFMA (v_mfma_f32_32x32x16_bf16, fp32
 *          accumulate; q, k, probabilities and v rounded to bf16), the configuration
 *          BASELINE names for UCF-101 256. Not fp32-faithful: tests/test_gpu_bf16_attn.py
 *          states its tolerance against the fp32 reference.
 *   F16_CONV   F16X3 with ONE fp16 MFMA per product (hi(a) * hi(b), fp32 accumulate) in the
 *          convolutions of the denoiser forward (extdm_unet_forward, the forward inside
 *          extdm_sample and extdm_p_losses): both conv operands rounded to fp16. Attention,
 *          norms and the sampler as in F16X3; every other entry point of the handle (the LFAE
 *          encoder calls, extdm_decode, extdm_attn_layer) runs F16X3 bit for bit. The range
 *          flag works as in F16X3. Not fp32-faithful: tests/test_gpu_f16_modes.py.
 *   F16    F16_CONV plus the attention routing of BF16_ATTN: the fast inference mode. */
enum { EXTDM_PRECISION_FP32 = 0, EXTDM_PRECISION_F16X3 = 1, EXTDM_PRECISION_BF16_ATTN = 2,
       EXTDM_PRECISION_F16_CONV = 3, EXTDM_PRECISION_F16 = 4 };

typedef struct ExtdmConfig {
  int arch;            /* EXTDM_ARCH_* */
  int dim;             /* Unet base width (64) */
  int channels;        /* init_conv input channels (256 + 256) */
  int dim_mults[4];
  int n_levels;        /* entries used in dim_mults */
  int window[3];       /* (2, 4, 4) */
  int heads;           /* attn_heads (8) */
  int dim_head;        /* attn_dim_head (32) */
  int tc, tp;          /* cond / pred frames; tc + tp (WO_REF: tc - 1 + tp) <= 64 */
  int latent;          /* flow-latent H = W (32) */
  int fea_size;        /* cond_fea H = W (16) */
  int fea_ch;          /* cond_fea channels (256) */
  int timesteps;       /* diffusion T (1000) */
  int max_batch;       /* workspace is sized for this batch (clips) */
  int device;          /* HIP device ordinal */
  /* LFAE Generator decoder (flow_params.generator_params); image = frame size */
  int image, num_channels, gen_block_expansion, gen_max_features, gen_num_down_blocks, gen_num_bottleneck_blocks;
  int precision;       /* EXTDM_PRECISION_* */
} ExtdmConfig;

int extdm_create(const ExtdmConfig* cfg, ExtdmHandle** out);
void extdm_destroy(ExtdmHandle* h);
const char* extdm_last_error(void);

/* Copy one named tensor (reference state_dict key: Unet keys without the
 * `denoise_fn.` prefix, GaussianDiffusion buffers by their own names, decoder
 * keys with a `generator.` prefix). dtype: 0 = float32, 1 = int64. Host memory. */
int extdm_load_weight(ExtdmHandle* h, const char* name, const void* host_ptr, int dtype, const int64_t* shape,
                      int ndim);
/* Pack weights into the GEMM layouts, build t-only tables (time-MLP, FiLM,
 * rotary, relative-position biases) and the workspace. */
int extdm_finalize(ExtdmHandle* h);
int64_t extdm_workspace_bytes(const ExtdmHandle* h);

/* eps = Unet3D(x, t, cond_frames, cond_fea). x, out: [B,3,tp,L,L]; t: int64 [B];
 * cond: [B,3,tc,L,L]; fea: [B,fea_ch,T,fs,fs] with T = tc+tp (tc-1+tp for WO_REF).
 * All device pointers. */
int extdm_unet_forward(ExtdmHandle* h, int B, const float* x, const int64_t* t, const float* cond,
                       const float* fea, float* out, void* stream);

/* Whole reverse loop. times[k] is the model timestep of step k and
 * times_next[k] the DDIM target (ignored for DDPM). x_T (device, may be NULL:
 * Philox stream), noise (device [S][B][n] or NULL: Philox stream), out (device
 * [B,3,tp,L,L]) receives x_0. use_graph != 0 replays one captured step.
 * EXTDM_SAMPLER_DPMPP: times must be strictly decreasing; step k goes from times[k] to
 * times[k + 1] and the last step to the clean sample. eta and times_next are ignored and a
 * non-NULL noise is an error. The handle's first such call allocates a [max_batch][n] fp32
 * history buffer (the previous step's thresholded x0), cleared at the start of every call. */
int extdm_sample(ExtdmHandle* h, int B, int sampler, int S, const int* times, const int* times_next, float eta,
                 const float* x_cond, const float* cond_fea, const float* x_T, const float* noise, uint64_t seed,
                 int sample_base, int round, float* out, int use_graph, void* stream);

/* Record the dynamic-threshold value s = max(1, quantile(|x0|, 0.9)) of every step and sample
 * of later extdm_sample calls into buf[k * B + b] (device fp32, cap floats >= S x B; NULL
 * stops recording). Verification hook for the captured-graph sampler (the threshold inside
 * p_mean_variance, Diffusion.py:150-163); the step itself is unchanged. */
int extdm_record_thresholds(ExtdmHandle* h, float* buf, int64_t cap);

/* One sampler update in place on x given eps (the step-k coefficients). DDPM and DDIM only:
 * EXTDM_SAMPLER_DPMPP is an error here and in extdm_sampler_step_t (extdm_sampler_step_hist). */
int extdm_sampler_step(ExtdmHandle* h, int B, int sampler, int t, int t_next, float eta, float* x, const float* eps,
                       const float* noise, float* thresh_out, void* stream);

/* One DPM-Solver++(2M) update in place on x given eps, from t towards t_next with t_prev the
 * step before (t_prev > t > t_next). x0 = the thresholded sqrt_recip[t] x - sqrt_recipm1[t] eps
 * as in every other sampler; with alpha = sqrt(alphas_cumprod), sigma = sqrt(1 - alphas_cumprod),
 * lambda = log(alpha / sigma), h = lambda(t_next) - lambda(t), r = (lambda(t) - lambda(t_prev)) / h
 * and a = alpha(t_next) (1 - exp(-h)), computed in fp64 and rounded once to fp32:
 *   x = ((sigma(t_next) / sigma(t)) x + a (1 + 1 / (2 r)) x0) + (-a / (2 r)) x0_prev
 * in fp32 in that order (three products, no contraction), then x0_prev = x0. t_prev < 0: the
 * first-order start (x0 weight a, history weight 0); t_next < 0: the final step, x = x0.
 * x0_prev: device [B][n], read and written. x and x0_prev must hold finite values even where
 * their weight is 0 (first and final step): 0 times a non-finite value is NaN.
 * thresh_out: [B] or NULL. The step extdm_sample replays for EXTDM_SAMPLER_DPMPP. */
int extdm_sampler_step_hist(ExtdmHandle* h, int B, int t_prev, int t, int t_next, float* x, const float* eps,
                            float* x0_prev, float* thresh_out, void* stream);

/* ---- Teacher-forced evaluation step (Diffusion.py:276-327), inference only --------------
 * Every t (and t_next) is a device int64 [B] vector as in extdm_unet_forward, each in
 * [0, timesteps); the calls read it back to build the per-sample coefficient table on the host
 * in fp32 with the reference's expressions (they synchronise `stream`). A sample's results never
 * depend on the batch it sits in or on the other samples' t. */

/* One sampler update in place on x given eps, sample b at its own t[b] (DDIM: towards
 * t_next[b]; DDPM ignores t_next, which may be NULL). noise: [B][n] (or NULL when no sample
 * uses noise), thresh_out: [B] or NULL. Sample b's result equals extdm_sampler_step at t[b]
 * bit for bit. */
int extdm_sampler_step_t(ExtdmHandle* h, int B, int sampler, const int64_t* t, const int64_t* t_next, float eta,
                         float* x, const float* eps, const float* noise, float* thresh_out, void* stream);

/* x_t[b] = sqrt_alphas_cumprod[t_b] x0[b] + sqrt_one_minus_alphas_cumprod[t_b] noise[b] in fp32
 * in that order. noise NULL: the sampler's Philox stream keyed by (seed, sample_base + b, round)
 * under a stream id no x_T or step uses; the drawn noise goes to noise_out when non-NULL. */
int extdm_q_sample(ExtdmHandle* h, int B, const int64_t* t, const float* x0, const float* noise, uint64_t seed,
                   int sample_base, int round, float* noise_out, float* x_t, void* stream);

/* The part of p_losses after the denoiser: pred_x0 = x0_hat = sqrt_recip[t] x_t - sqrt_recipm1[t] eps,
 * with clip_denoised != 0 clamped to +-s and divided by s = max(1, quantile(|x0_hat|, 0.9)) (exact
 * order statistics; s to thresh_out[B] when non-NULL), else raw. loss_sum[b] (device double [B]) =
 * sum |noise - eps| (L1) or sum (10 noise - 10 eps)^2 (L2) over sample b: fp32 terms added in
 * fp64 in a fixed order. The reference's mean loss is sum_b loss_sum[b] / (B n). */
enum { EXTDM_LOSS_L1 = 0, EXTDM_LOSS_L2 = 1 };
int extdm_x0_loss(ExtdmHandle* h, int B, const int64_t* t, const float* x_t, const float* eps, const float* noise,
                  int loss_type, int clip_denoised, float* pred_x0, double* loss_sum, float* thresh_out,
                  void* stream);

/* q_sample, the denoiser forward and x0_loss chained on the handle's workspace. x_cond: [B,3,tc,L,L],
 * x_start / pred_x0: [B,3,tp,L,L], cond_fea as in extdm_unet_forward, noise as in extdm_q_sample.
 * Fails like extdm_sample when the F16X3 range flag is raised by the forward. */
int extdm_p_losses(ExtdmHandle* h, int B, const int64_t* t, const float* x_cond, const float* x_start,
                   const float* cond_fea, const float* noise, uint64_t seed, int sample_base, int round, int loss_type,
                   int clip_denoised, float* pred_x0, double* loss_sum, void* stream);

/* sums[b] = sum_i |a[b][i] - b[b][i]|, i < n, in fp64 in a fixed order (the numerator of the
 * reference wrappers' rec_loss / rec_warp_loss, nn.L1Loss). a, b: contiguous device fp32 [B][n];
 * sums: device double [B]; work: device scratch of B x extdm_abs_diff_chunks(n) doubles. Not tied
 * to a handle. */
int extdm_abs_diff_chunks(int n);
int extdm_abs_diff_sum(const float* a, const float* b, int B, int n, double* sums, double* work, void* stream);

/* Measurement hook for bench.py: time `iters` launches of one hot-path conv
 * exactly as the forward issues it, on random operands, with HIP events on the
 * handle's stream; returns the average ms per launch and the algorithmic FLOPs
 * per launch. layer 0 = init_conv (1,7,7) channels->dim (two sources); 1, 2, 3 =
 * ResnetBlock (1,3,3) convs at levels 0, 1, 2 (downs.{0,1,2}.0.block2) from an fp32
 * input; 4 = the level-0 up ResnetBlock's 1x1 res_conv (ups.3.0.res_conv); 5 = the
 * level-0 block2 conv from block1's pre-split operand, as the F16X3 forward issues it. */
int extdm_bench_layer(ExtdmHandle* h, int B, int layer, int iters, float* ms_out, double* flops_out);
/* (6 / 7: the level-0 STW / init_temporal attention layer — one fused launch, or on the unfused
 * core route the attention core alone; 14 / 15: that STW layer's qkv / proj 1x1 conv alone and
 * 16 / 17: the temporal layer's qkv / to_out, on the core route only; 8-13: see runtime.cpp.)
 * The kernel template the last extdm_bench_layer call of `layer` launched for the attention
 * layers (e.g. "stw64_x3_kernel<64, 16, 8, false>"), written to buf (cap bytes, NUL-terminated;
 * empty when not recorded). bench.py prices a layer by that kernel's arithmetic. */
int extdm_bench_layer_kernel(ExtdmHandle* h, int layer, char* buf, int cap);

/* The F16X3 activation-range flag: nonzero if an operand split since the last reset
 * had |v| >= 65504 (results computed meanwhile are not fp32-accurate): bit 0 = a conv /
 * GEMM / cross-attention input, bit 1 = a fused-attention operand; 0 if not, <0 on
 * error; reset != 0 clears it. Synchronises `stream`. */
int extdm_range_flag(ExtdmHandle* h, int reset, void* stream);

/* One attention layer as the forward issues it (parity tests): prefix names a
 * Residual(PreNorm(STWAttentionLayer)) (e.g. "downs.0.1", shifted per the layer's
 * position, u12:961-963) or a temporal Residual(PreNorm(AttentionLayer)) (e.g.
 * "init_temporal_attn", u12:915). x, out: [B,C,T,H,W] device tensors. */
int extdm_attn_layer(ExtdmHandle* h, const char* prefix, int B, int C, int T, int H, int W, int shifted,
                     const float* x, float* out, void* stream);

/* LFAE decoder (Generator.forward_with_flow) for B clips x T frames.
 * ref: [B,C,S,S] source image; flow: [B,2,T,fh,fw] (x, y grid); occ: [B,1,T,fh,fw]
 * occlusion in [0,1] or NULL (reference quirk: without occlusion the prediction
 * equals the warped source); pred: [B,C,T,S,S]; warped: [B,C,T,S,S] or NULL
 * ('deformed'). Needs the decoder weights (keys 'generator.*') unless occ is NULL. */
int extdm_decode(ExtdmHandle* h, int B, int C, int T, int S, int fh, int fw, const float* ref, const float* flow,
                 const float* occ, float* pred, float* warped, void* stream);

/* ---- LFAE encoder ------------------------------------------
 * flow_params.model_params of the config/DM YAML files. Set before extdm_finalize on a
 * handle that holds 'region_predictor.*', 'bg_predictor.*' and/or 'generator.*'
 * (incl. 'generator.pixelwise_flow_predictor.*') weights. Images are [N][C][S][S]
 * fp32 device tensors, S = image; N <= max_batch. */
typedef struct ExtdmLfaeConfig {
  int num_regions, num_channels, image, revert_axis_swap;
  float rp_temperature, rp_scale_factor;
  int rp_pad, rp_num_blocks, rp_pca_based;
  int bg_type; /* 0 zero, 1 shift, 2 affine, 3 perspective */
  int bg_num_blocks;
  float pf_scale_factor, pf_region_var;
  int pf_num_blocks, pf_use_covar_heatmap, pf_use_deformed_source;
} ExtdmLfaeConfig;
int extdm_set_lfae(ExtdmHandle* h, const ExtdmLfaeConfig* c);

/* RegionPredictor.forward, PCA-based (LFAE/region_predictor.py:62-150):
 * shift [N][R][2], covar [N][R][2][2], affine [N][R][2][2] = U sqrt(S) with
 * torch.svd's (LAPACK sgesdd) sign convention; u [N][R][2][2], sv [N][R][2] (sqrt of
 * the singular values, the diagonal of 'd') and heatmap [N][R][h][w] optional (NULL).
 * extdm_region_hw gives the heatmap side h = w. */
int extdm_region_params(ExtdmHandle* h, int N, const float* img, float* shift, float* covar, float* affine,
                        float* u, float* sv, float* heatmap, void* stream);
int extdm_region_hw(const ExtdmHandle* h);

/* BGMotionPredictor.forward (LFAE/bg_motion_predictor.py:47-64): out [N][3][3]. */
int extdm_bg_params(ExtdmHandle* h, int N, const float* src, const float* drv, float* out, void* stream);

/* PixelwiseFlowPredictor.forward (LFAE/pixelwise_flow_predictor.py:106-153) for
 * source images src and the region params above (+ bg [N][3][3] or NULL):
 * flow [N][2][h][w] (x, y; the reference's optical_flow permuted), occ [N][1][h][w]
 * or NULL (needs the occlusion head). h = w = extdm_flow_hw(). */
int extdm_flow_predict(ExtdmHandle* h, int N, const float* src, const float* drv_shift, const float* drv_covar,
                       const float* drv_affine, const float* src_shift, const float* src_covar,
                       const float* src_affine, const float* bg, float* flow, float* occ, void* stream);
int extdm_flow_hw(const ExtdmHandle* h);

/* Generator.forward_bottle / compute_fea (LFAE/generator.py:95-102, 202-206):
 * out [N][C_bottleneck][S / 2^d][S / 2^d]. */
int extdm_bottleneck(ExtdmHandle* h, int N, const float* img, float* out, void* stream);

/* Per-frame PSNR and SSIM of two frame sets a, b (device fp32, [N][T][C][H][W] through
 * element strides sN, sT, sC; planes contiguous H*W) into device doubles psnr[N*T],
 * ssim[N*T], in fp64 like the reference's numpy evaluation. C must be 1 or 3 and
 * H, W > 10 (the 11x11 window's valid region). `work` is device scratch of
 * extdm_frame_metrics_workspace() bytes. Not tied to a handle. */
size_t extdm_frame_metrics_workspace(int N, int T, int C, int H, int W);
int extdm_frame_metrics(const float* a, const float* b, int N, int T, int C, int H, int W, long sN, long sT, long sC,
                        double* psnr, double* ssim, void* work, void* stream);

/* Bilinear resize (align_corners=False, F.interpolate(mode='bilinear')) of frames into a
 * contiguous dst [B][C][T][OH][OW]: frame t < t_split from a at frame t, frame t >= t_split from
 * b at frame t - t_split (element strides per batch / channel / frame; planes contiguous H*W;
 * a frame stride of 0 repeats one frame). Replaces the multi1248 wrapper's per-frame
 * interpolate of the cond features (multi1248.py:240-245). Not tied to a handle. */
int extdm_bilinear_frames(float* dst, int B, int C, int T, int OH, int OW, const float* a, long a_sb, long a_sc,
                          long a_st, const float* b, long b_sb, long b_sc, long b_st, int t_split, int H, int W,
                          void* stream);

/* ---- FVD features: InceptionI3d (metrics/pytorch_i3d.py:135-322) on a handle of its own ----
 * The network shares nothing with an ExtdmHandle. Weights go in under the reference's state_dict
 * keys (the public i3d_pretrained_400.pt layout: `Conv3d_1a_7x7.conv3d.weight`,
 * `Mixed_3b.b1b.bn.running_var`, `logits.conv3d.bias`, ...; `num_batches_tracked` entries are
 * accepted and ignored). extdm_fvd_finalize packs them for the f16x3 3-D convolution, folds every
 * BatchNorm3d (eval, eps 1e-5) into a per-channel scale / shift and plans the workspace at
 * max_batch x max_frames x 224 x 224; a missing key is an error naming the key. */
typedef struct ExtdmFvdHandle ExtdmFvdHandle;
int extdm_fvd_create(int num_classes, int in_channels, int max_batch, int max_frames, int device,
                     ExtdmFvdHandle** out);
void extdm_fvd_destroy(ExtdmFvdHandle* h);
int extdm_fvd_load_weight(ExtdmFvdHandle* h, const char* name, const void* host_ptr, int dtype,
                          const int64_t* shape, int ndim);
/* The arithmetic of the handle's 3-D convolutions, between create and finalize (afterwards an
 * error): EXTDM_PRECISION_F16X3 (the default) or EXTDM_PRECISION_FP32, the exact-fp32 kernels on
 * v_mfma_f32_32x32x2_f32. finalize packs the chosen route's weights only. An FP32 handle never
 * narrows an operand: its range flag stays 0 and extdm_fvd_features never raises the fp16 range
 * error. EXTDM_PRECISION_BF16_ATTN, _F16_CONV and _F16 are errors (denoiser modes). */
int extdm_fvd_set_precision(ExtdmFvdHandle* h, int mode);
int extdm_fvd_finalize(ExtdmFvdHandle* h);

/* trans + preprocess_single (calculate_fvd.py:6-14, fvd.py:161-187) in one launch: in
 * [B][T][C][H][W] in [0, 1] through element strides (planes contiguous H*W), C = 1 replicated to
 * 3; temporal crop to sequence_length frames (0: none); bilinear resize (align_corners=False) of
 * the shorter side to `resolution`, the longer to ceil(side * resolution / shorter); centre crop;
 * (v - 0.5) * 2 -> out [B][3][T'][resolution][resolution]. Not tied to a handle. */
int extdm_fvd_preprocess(const float* in, int B, int T, int C, int H, int W, long sb, long st, long sc,
                         int sequence_length, int resolution, float* out, void* stream);

/* InceptionI3d.forward / extract_features on x [N][in_channels][T][224][224]: logits_out
 * [N][num_classes] (pre-softmax, the mean over the time slots) and / or pooled_out
 * [N][1024][T'' - 1] (the AvgPool3d([2, 7, 7]) output), either may be NULL. T >= 9 (the
 * reference's avg-pool raises below that) and N <= max_batch, T <= max_frames. A video's outputs
 * do not depend on the batch it sits in. Fails if an f16x3 convolution input reached
 * |v| >= 65504 (the sticky range flag, reset at entry). Synchronises the stream. */
int extdm_fvd_features(ExtdmFvdHandle* h, int N, int T, const float* x, float* logits_out, float* pooled_out,
                       void* stream);

/* The parity hook: the network from x [N][in_channels][T][H][W] (any size the workspace holds) up
 * to and including endpoint_name, one of VALID_ENDPOINTS `Conv3d_1a_7x7` ... `Mixed_5c`
 * (pytorch_i3d.py:151-167), into out [N][C'][T'][H'][W']; extdm_fvd_endpoint_shape writes
 * dims = {C', T', H', W'}. */
int extdm_fvd_endpoint(ExtdmFvdHandle* h, int N, int T, int H, int W, const float* x, const char* endpoint_name,
                       float* out, void* stream);
int extdm_fvd_endpoint_shape(const ExtdmFvdHandle* h, int T, int H, int W, const char* endpoint_name, int* dims);

/* MaxPool3dSamePadding.forward (pytorch_i3d.py:15-34) of a contiguous x [B][C][T][H][W] into a
 * contiguous out [B][C][ceil(T/st)][ceil(H/sh)][ceil(W/sw)]: the 'same' rule's zero padding, then
 * the max, so a padded 0 beats negative values. Windows [1,3,3], [3,3,3] and [2,2,2] (the
 * network's), any stride. Not tied to a handle. */
int extdm_fvd_maxpool(const float* x, int B, int C, int T, int H, int W, int kt, int kh, int kw, int st, int sh,
                      int sw, float* out, void* stream);

/* The host pad arithmetic of the launches above: the 'same' rule of Unit3D / MaxPool3dSamePadding
 * (pytorch_i3d.py:9-13, 71-95) for one dimension. Returns the output extent ceil(size / stride)
 * and writes the front and back zero pads (-1: bad argument). No device needed. */
int extdm_fvd_same_pad(int size, int kernel, int stride, int* front, int* back);

/* 1 if a convolution input of this handle reached |v| >= 65504 since the last reset. */
int extdm_fvd_range_flag(ExtdmFvdHandle* h, int reset, void* stream);

/* ---- LPIPS: lpips.LPIPS(net='alex', version='0.1') on a handle of its own ----
 * The metric of metrics/calculate_lpips.py:12. The `lpips` package is not part of the reference, so
 * the network is restated from the published package: ScalingLayer.forward, the five ReLU taps of
 * pretrained_networks.alexnet.forward, normalize_tensor, NetLinLayer, upsample / spatial_average and
 * the sum of LPIPS.forward. Weights go in under the package's state_dict keys: `scaling_layer.shift`
 * / `.scale` [1][3][1][1], `net.slice1.0`, `net.slice2.3`, `net.slice3.6`, `net.slice4.8`,
 * `net.slice5.10` with `.weight` / `.bias`, and `linK.model.1.weight` [1][C_K][1][1], K = 0 .. 4;
 * `lins.K.model.1.weight` is accepted as an alias of `linK...` and must equal it if both are given.
 * extdm_lpips_finalize packs the convs for the f16x3 2-D convolution and allocates the workspace for
 * max_pairs pairs of max_h x max_w images; a missing key is an error naming the key. The fp32
 * tiles of the exact-fp32 route are packed and uploaded by the handle's first call with
 * EXTDM_LPIPS_FP32 (about 10 MB); a handle that never sees the flag allocates nothing for it. */
typedef struct ExtdmLpipsHandle ExtdmLpipsHandle;
int extdm_lpips_create(int max_pairs, int max_h, int max_w, int device, ExtdmLpipsHandle** out);
void extdm_lpips_destroy(ExtdmLpipsHandle* h);
int extdm_lpips_load_weight(ExtdmLpipsHandle* h, const char* name, const void* host_ptr, int dtype,
                            const int64_t* shape, int ndim);
int extdm_lpips_finalize(ExtdmLpipsHandle* h);

/* flags of extdm_lpips_distance / extdm_lpips_features */
#define EXTDM_LPIPS_NORMALIZE 1  /* LPIPS.forward(normalize=True): x * 2 - 1 first */
#define EXTDM_LPIPS_TRANS 2      /* trans (calculate_lpips.py:15-23): x * 2 - 1 first */
#define EXTDM_LPIPS_PLAIN_MEAN 4 /* mean_out as LPIPS(spatial=False): spatial_average of each lin map */
/* The five convolutions of this call in exact fp32 on v_mfma_f32_32x32x2_f32 instead of f16x3: no
 * fp16 range limit, so the range flag is neither raised nor consulted and stays 0. The pools, the
 * distance head, the mean and the map are the same launches on both routes. */
#define EXTDM_LPIPS_FP32 8

/* LPIPS.forward(in0, in1) for N pairs in one batch (replaces the one-pair-per-forward loops of
 * calculate_lpips.py:40-60, 83-93, 102-112, 122-132): in0, in1 [N][C][H][W] through the element
 * strides sn / sc (planes contiguous H*W), C = 1 replicated to 3 (trans, calculate_lpips.py:17-18).
 * mean_out [N]: the mean of the spatial map (calculate_lpips.py:59 `.mean()`), computed from the
 * small lin maps as sum_ij wy[i] wx[j] m[i][j] (extdm_lpips_mean_weights) in fp64; with
 * EXTDM_LPIPS_PLAIN_MEAN the spatial=False value instead. map_out [N][H][W]: the spatial=True map
 * (bilinear upsample, align_corners=False, of the five lin maps, summed). Either may be NULL. Errors
 * on H or W < 31 (the second MaxPool2d(3, 2) has no output), N > max_pairs, H > max_h or W > max_w.
 * A pair's values do not depend on the batch it sits in, on either route. Without
 * EXTDM_LPIPS_FP32 the call fails if an f16x3 convolution input reached |v| >= 65504 (the sticky
 * range flag, reset at entry). Synchronises the stream. */
int extdm_lpips_distance(ExtdmLpipsHandle* h, int N, int C, int H, int W, const float* in0, long sn0, long sc0,
                         const float* in1, long sn1, long sc1, int flags, float* mean_out, float* map_out,
                         void* stream);

/* The parity hook: tap 0 .. 4 = relu1 .. relu5 of pretrained_networks.alexnet.forward for one image
 * set x [N][C][H][W] (N <= 2 max_pairs), post-ReLU and un-normalised, into out [N][C'][h][w], on
 * the f16x3 route or, with EXTDM_LPIPS_FP32, the exact-fp32 one;
 * extdm_lpips_feature_shape writes dims = {C', h, w} (no device needed; 0 extents where the input
 * is too small). */
int extdm_lpips_features(ExtdmLpipsHandle* h, int N, int C, int H, int W, const float* x, long sn, long sc, int flags,
                         int tap, float* out, void* stream);
int extdm_lpips_feature_shape(int H, int W, int tap, int* dims);

/* nn.MaxPool2d(kernel_size=3, stride=2) (torchvision alexnet features 2 and 5) of a contiguous x
 * [B][C][H][W] into out [B][C][(H-3)/2+1][(W-3)/2+1]. Not tied to a handle. */
int extdm_lpips_maxpool(const float* x, int B, int C, int H, int W, float* out, void* stream);

/* The separable weights of the mean of an upsampled map (lpips.upsample + calculate_lpips.py:59):
 * w[i], i < in, the column means of the 1-D bilinear (align_corners=False) interpolation matrix
 * from `in` to `out` samples, in fp64; they sum to 1. A host function, no device. -1: bad argument. */
int extdm_lpips_mean_weights(int in, int out, double* w);

/* 1 if an f16x3 convolution input of this handle reached |v| >= 65504 since the last reset (calls
 * with EXTDM_LPIPS_FP32 leave it 0). */
int extdm_lpips_range_flag(ExtdmLpipsHandle* h, int reset, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* EXTDM_H */
