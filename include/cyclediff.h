/* libcyclediff — C ABI of the MI355X-native CycleDiffusion engine.
 *
 * The reference (ChenWu98/cycle-diffusion) is pure Python/PyTorch and has no FFI; this header is
 * the seam a maintainer binds (ctypes) underneath the reference's plugin API:
 *   model/gan_wrapper/stable_diffusion_stochastic_text_wrapper.py:102-253  (SDStochasticTextWrapper)
 *   model/gan_wrapper/latentdiff_stochastic_text_wrapper.py               (LatentDiffStochasticTextWrapper)
 *   model/gan_wrapper/ddpm_ddim_wrapper.py:317-542                         (DDPMDDIMWrapper)
 * Each entry point names the reference function it replaces.
 *
 * Conventions: every pointer is a DEVICE pointer unless its name ends in _host; tensors at the
 * boundary are fp32, NCHW, contiguous (the reference's layout); all calls are asynchronous on the
 * engine's HIP stream; return value 0 = ok, non-zero = error with text in cd_last_error();
 * no exception crosses the ABI; one handle per rank / stream. A handle is not thread safe (one host
 * thread at a time), but DIFFERENT handles are independent - own stream, workspace, split-K scratch -
 * and may be driven concurrently from different host threads on the same GPU (several batches in
 * flight; tests/test_gpu_concurrency.py). The caller owns every buffer it passes, the engine owns
 * weights and workspace.
 */
#ifndef CYCLEDIFF_H
#define CYCLEDIFF_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cd_engine* cd_handle;

enum { CD_NET_UNET_OPENAI = 1, CD_NET_UNET_HO = 2, CD_NET_VAE_KL = 3, CD_NET_CLIP_TEXT = 4, CD_NET_BERT_XTR = 5,
       CD_NET_OCLIP_TEXT = 6, CD_NET_OCLIP_VISION = 7, CD_NET_INCEPTION_FID = 8, CD_NET_LPIPS = 9 };
enum { CD_SCHED_DDIM = 0, CD_SCHED_DDPM = 1 };
enum { CD_PREC_16 = 0, CD_PREC_F32 = 1, CD_PREC_F32X3 = 2 };
/* what a keep-mask holds its region to: q_sample(x0, t) freshly noised per step (the reference, ddim.py:427-430), or the
 * DPM-Encoder's own x_t of the level (coupled loop only) */
enum { CD_MASK_QSAMPLE = 0, CD_MASK_ENCODER = 1 };

/* Architecture descriptor (the hyper-parameters of the reference's YAML / dict configs):
 *   UNET_OPENAI : ldm/modules/diffusionmodules/openaimodel.py:413-470 (SD v1, LDM text2img) and
 *                 model/lib/ddpm_ddim/models/improved_ddpm/unet.py:401-470 (i_DDPM AFHQ)
 *   UNET_HO     : model/lib/ddpm_ddim/models/ddpm/diffusion.py:192-290
 *   VAE_KL      : ldm/models/autoencoder.py:285-333 + diffusionmodules/model.py:368-568; with n_embed > 0 the VQ-f4
 *                 first stage (VQModelInterface) of the unconditional LDMs
 *   CLIP_TEXT   : the HF `CLIPTextModel` behind FrozenCLIPEmbedder (ldm/modules/encoders/modules.py:136-161);
 *                 descriptor fields reused: model_channels = width (768), num_res_blocks = layers (12),
 *                 num_heads (12), context_dim = MLP width (3072), in_channels = vocabulary (49408),
 *                 image_size = positions (77); weights keyed by `text_model.*` (HF state_dict names)
 *   BERT_XTR    : BERTEmbedder.transformer, the x-transformers TransformerWrapper(Encoder(dim 1280, depth 32)) of
 *                 LDM text2img (model/lib/latentdiff/ldm/modules/encoders/modules.py:75-98); same fields plus
 *                 num_head_channels = dim_head (64; heads 8 -> inner 512); weights keyed by `token_emb`,
 *                 `pos_emb.emb`, `attn_layers.layers.*`, `norm`
 *   OCLIP_TEXT / OCLIP_VISION : the text and image towers of OpenAI CLIP (ViT-B/32 in the reference:
 *                 model/energy/clean_clip.py:10 `clip.load("ViT-B/32")`), weights keyed by the openai/CLIP package's
 *                 state_dict names; out_channels = embedding width (512); VISION: image_size = input resolution
 *                 (224), z_channels = patch size (32), in_channels = 3
 *   INCEPTION_FID : the Inception-v3 of the FID / KID metrics (torchvision Inception3 with the FIDInceptionA / C / E_1 / E_2
 *                 blocks of pytorch-fid and clean-fid) up to its 2048-d pool3 features; image_size = 299, precision =
 *                 CD_PREC_16 (the only one implemented), no other field is read. Weights keyed by that network's
 *                 state_dict names, `X.conv.weight`, `X.bn.weight`, `X.bn.bias`, `X.bn.running_mean`, `X.bn.running_var`
 *                 for every BasicConv2d X (`Conv2d_1a_3x3`, `Mixed_5b.branch1x1`, ...); BatchNorm (eps 1e-3) is folded
 *                 into the packed weights inside the engine before the next forward
 *   LPIPS       : the perceptual distance LPIPS v0.1 on the torchvision AlexNet or VGG16 `features` stack; descriptor field
 *                 reused: num_res_blocks = number of convs, which selects the backbone (5 = AlexNet, 13 = VGG16); precision =
 *                 CD_PREC_16 (the only one implemented); no image_size (any H x W from 31 / 16 up), no other field is read.
 *                 Weights keyed `features.N.weight`, `features.N.bias` (N = the torchvision `features` index of the conv) and
 *                 `lin{l}.weight` [1, C_l, 1, 1] for the five taps l */
typedef struct cd_net_desc {
  int kind;
  int image_size;          /* spatial size of the network input (latent 64, pixel 256, ...)      */
  int in_channels, out_channels;
  int model_channels;      /* `model_channels` / `ch`                                            */
  int num_res_blocks;
  int n_mult;  int channel_mult[8];
  int n_attn;  int attn[8];/* OPENAI: downsample rates with attention; HO/VAE: resolutions       */
  int num_heads;           /* -1 when num_head_channels is used                                   */
  int num_head_channels;   /* -1 when num_heads is used                                           */
  int use_spatial_transformer, context_dim, transformer_depth;
  int use_scale_shift_norm, resblock_updown, conv_resample;
  /* VAE */
  int z_channels, embed_dim, double_z;
  /* Storage / arithmetic of the network: CD_PREC_16 = 16-bit activations and weights, fp32 accumulate (default);
   * CD_PREC_F32 = fp32 activations, weights and matrix instructions - what the reference itself computes in
   * (`use_fp16=False`, improved_ddpm/script_util.py:15; `precision = "full"`,
   * stable_diffusion_stochastic_text_wrapper.py:117). U-Nets only: the pixel-space DDPMs of ddpm_ddim_wrapper.py, whose
   * 'ddim' chain needs eps_hat at fp32 resolution, and - round 4 - the text-conditioned SD / LDM U-Nets
   * (SpatialTransformer blocks with fp32 LayerNorm, fp32 flash attention and exact-erf GEGLU, csrc/st_f32.hip), for which
   * it restores the encode -> decode cycle the 16-bit engine only closes to 2e-2;
   * CD_PREC_F32X3 = the fp32 network with its GroupNorm- / LayerNorm-fed convolutions and projections evaluated as
   * three-term split-fp16 products on the 16-bit matrix cores (x = hi + lo, w = wh + wl; hi.wh + lo.wh + hi.wl, fp32
   * accumulate: 2^-22 per product instead of 2^-24; everything else as CD_PREC_F32). fp16 build of the library only. */
  int precision;
  /* VAE_KL only: > 0 selects the VQ first stage of the unconditional LDMs (VQModelInterface,
   * model/lib/latentdiff/ldm/models/autoencoder.py:264-282, `n_embed` codebook rows of width embed_dim): double_z = 0,
   * encode = encoder + quant_conv (no sampling), decode = nearest-codebook quantisation + post_quant_conv + decoder */
  int n_embed;
  int reserved[6];
} cd_net_desc;

/* Per-step scheduler coefficients, evaluated by the host in fp32 in the reference's operation
 * order (ddim.py:570-579 / ddpm_ddim_wrapper.py:291-302); see csrc/kernels.h StepCoef. */
typedef struct cd_step_coef {
  float sa, s1a, sap, dirc, sigma, r, t_mask;
  int32_t t;
} cd_step_coef;

const char* cd_last_error(void);
int cd_version(void);
/* 16-bit storage format of activations / packed weights inside the engine: 1 = IEEE fp16, 0 = bfloat16 */
int cd_act_format(void);

/* engine lifetime; `hip_stream` is a hipStream_t (0 = default stream) */
int cd_engine_create(void* hip_stream, size_t workspace_bytes, cd_handle* out);
int cd_engine_destroy(cd_handle h);
int cd_engine_workspace_high_water(cd_handle h, size_t* bytes);
/* wait for everything queued on the engine's stream, SLEEPING (blocking-sync event) instead of spinning: what a rank
 * calls where the reference's Trainer would call torch.cuda.synchronize() (trainer/trainer.py:1055-1062 times
 * evaluate() around it). The sampler entry points also pace themselves: the host never runs more than two sampler
 * steps ahead of the GPU (CYCLEDIFF_HOST_PACING=0 turns that off). */
int cd_engine_synchronize(cd_handle h);
/* per-launch timing of the implicit-GEMM kernel family with HIP events on the engine's stream
 * (bench.py roofline leg): enable, run, then collect launches / summed ms / summed 2*M*N*K flops */
int cd_prof_enable(cd_handle h, int on);
int cd_prof_collect(cd_handle h, int* launches, double* total_ms, double* total_flops);

/* networks: build from a descriptor, then load weights by the reference's state_dict names
 * (replaces load_model_from_config, model/lib/stable_diffusion/txt2img.py:25-42, and
 *  generator.load_state_dict, ddpm_ddim_wrapper.py:378-379) */
int cd_net_create(cd_handle h, const cd_net_desc* desc, int* net_id);
int cd_net_param_count(cd_handle h, int net, int* n);
int cd_net_param_info(cd_handle h, int net, int index, char* name, int name_cap, int* ndim, int64_t shape[4]);
int cd_net_load_param(cd_handle h, int net, const char* name, const float* data_host, int ndim,
                      const int64_t* shape);
int cd_net_missing_params(cd_handle h, int net, int* n_missing, char* first_name, int name_cap);

/* eps_hat = UNet(x, t, context)  — LatentDiffusion.apply_model -> DiffusionWrapper.forward ->
 * UNetModel.forward (ddpm.py:882-983,1392-1394; openaimodel.py:710-742) and DDPM.forward
 * (ddpm/diffusion.py:292-337). x [B,C,H,W]; t [B] float timesteps; ctx [B,L,Dc] or NULL;
 * eps_out [B,Cout,H,W]. */
int cd_unet_forward(cd_handle h, int net, const float* x, const float* t, const float* ctx, int B,
                    int ctx_len, float* eps_out);

/* c = FrozenCLIPEmbedder(text): last_hidden_state of the CLIP text transformer for already tokenised text
 * (modules.py:148-158: tokenizer(..., max_length=77, padding="max_length") then transformer(input_ids)).
 * tokens [B,L] int32 (device), out [B,L,width] fp32 - the `ctx` tensors of the sampler entry points.
 * For a BERT_XTR net: BERTEmbedder.forward (tokens -> transformer(tokens, return_embeddings=True)). */
int cd_text_encode(cd_handle h, int net, const int32_t* tokens, int B, int L, float* out);

/* DirectionalCLIP's feature extractors (model/energy/clean_clip.py:24-31): model.encode_text(tokens) and
 * model.encode_image(preprocessed) of OpenAI CLIP, un-normalised. tokens [B,L] int32; img [B,3,R,R] fp32 already
 * resized / centre-cropped / mean-std normalised; out [B,embed] fp32. */
/* Inception-v3 features for FID / KID (clean-fid's `build_feature_extractor` network; evaluation/translate_to_dog.py
 * computes the metrics on them). img [B,3,299,299] fp32, already resized and normalised ((x - 128) / 128 on the 0..255
 * scale). stop_block = -1: out = pool3 [B,2048]. stop_block = k >= 0: out = the output of entry k of the block list as
 * fp32 NCHW [B,C,H,W]: 0 Conv2d_1a_3x3 (32x149x149), 1 Conv2d_2a_3x3 (32x147x147), 2 Conv2d_2b_3x3 (64x147x147),
 * 3 max-pool (64x73x73), 4 Conv2d_3b_1x1 (80x73x73), 5 Conv2d_4a_3x3 (192x71x71), 6 max-pool (192x35x35), 7-9 Mixed_5b/5c/5d
 * (256/288/288x35x35), 10 Mixed_6a (768x17x17), 11-14 Mixed_6b..6e (768x17x17), 15 Mixed_7a (1280x8x8), 16-17 Mixed_7b/7c
 * (2048x8x8). */
int cd_inception_features(cd_handle h, int net, const float* img, int B, int stop_block, float* out);
/* LPIPS v0.1 (the `lpips` package's `LPIPS(net=...)(x0, x1)`, spatial=False): img0, img1 [B,3,H,W] fp32 in [-1,1] -> out [B];
 * per_layer (or NULL) [B,5] = the five tap terms whose sum (in tap order) is out. Both images run as one batch of 2 B.
 * Refused before any launch: B < 1, H or W below 31 (alex) / 16 (vgg) - a tap would be empty. */
int cd_lpips(cd_handle h, int net, const float* img0, const float* img1, int B, int H, int W, float* per_layer, float* out);
/* the un-normalised ReLU output of tap 0..4 of the backbone (scaling layer included) as fp32 NCHW [B,C_tap,H_tap,W_tap] */
int cd_lpips_tap(cd_handle h, int net, const float* img, int B, int H, int W, int tap, float* out);
int cd_clip_text_features(cd_handle h, int net, const int32_t* tokens, int B, int L, float* out);
int cd_clip_image_features(cd_handle h, int net, const float* img, int B, float* out);

/* z0 = scale * posterior(E(img)).sample() (or .mode() when sample==0) — encode_first_stage +
 * get_first_stage_encoding (ddpm.py:817-854, 536-543); img [B,3,R,R] in [-1,1]; noise [B,zc,R/8,R/8]
 * or NULL (then Philox(seed)); z0 [B,zc,R/8,R/8]. */
int cd_vae_encode(cd_handle h, int net, const float* img, const float* noise, uint64_t seed, int B, int R,
                  int sample, float scale, float* z0);
/* img = D(z0/scale)*out_mul + out_add — decode_first_stage (ddpm.py:698-755); the wrapper's
 * post_process (x+1)/2 (sd_wrapper:135-137) is out_mul=0.5, out_add=0.5. */
int cd_vae_decode(cd_handle h, int net, const float* z0, int B, int hlat, float scale, float out_mul,
                  float out_add, float* img);
/* The same two on a rectangle (the first stage is fully convolutional; its one attention block runs over the h*w tokens it is
 * given): img [B,3,H,W], H and W multiples of the first-stage factor f (refused otherwise), z0 / noise [B,zc,H/f,W/f]; decode:
 * z0 [B,zc,hl,wl] -> img [B,3,hl*f,wl*f]. The square entry points are these with H = W = R, bit for bit. */
int cd_vae_encode_hw(cd_handle h, int net, const float* img, const float* noise, uint64_t seed, int B, int H, int W,
                     int sample, float scale, float* z0);
int cd_vae_decode_hw(cd_handle h, int net, const float* z0, int B, int hl, int wl, float scale, float out_mul,
                     float out_add, float* img);

/* DPM-Encoder: DDIMSampler.ddpm_ddim_encoding / _ddpm_ddim_encoding (ddim.py:230-286, 450-501)
 * and DDPMDDIMWrapper.encode's loop (ddpm_ddim_wrapper.py:483-520).
 *   x0 [B,C,H,W]; ctx_c / ctx_uc [B,L,Dc] or NULL (pixel DDPMs); guidance g as in ddim.py:550-559;
 *   coef_host: K+1 rows — row K initialises x_T (sa, s1a), rows K-1..0 are the loop steps;
 *   noise [K,B,C,H,W] (slot 0 = x_T draw, slots 1..K-1 = per-step draws in loop order) or NULL;
 *   z_out [B,K+1,C,H,W] = stack([x_T, eps_{K-1}, ..., eps_0], dim=1) (sd_wrapper:203).
 *   last_uses_x0: 1 = latent sampler (index 0 returns x0, no draw, ddim.py:583-584);
 *                 0 = pixel wrapper (K-1 ordinary steps; z has K entries).
 *   A white-box prefix shorter than the chain (`white_box_steps` of the text wrappers, ddim.py:486: the loop breaks after
 *   n < K steps) is the same call on the n + 1 table rows [K-n .. K-1, K] with last_uses_x0 = 0 and n + 1 noise slots - every
 *   row carries its own timestep; K = 0 draws x_T only (white_box_steps = -1). */
int cd_dpm_encode(cd_handle h, int net, int sched_kind, const float* x0, const float* ctx_c,
                  const float* ctx_uc, int ctx_len, float guidance, int B, int K,
                  const cd_step_coef* coef_host, const float* noise, uint64_t seed,
                  int last_uses_x0, float* z_out);

/* Decode with injected eps: DDIMSampler.sample_with_eps / ddim_sampling_with_eps /
 * p_sample_ddim_with_eps (ddim.py:170-228, 395-448, 603-646) and DDPMDDIMWrapper.generate
 * (ddpm_ddim_wrapper.py:392-455).
 *   z [B,T,C,H,W] with z[:,0] = x_T and z[:,1+i] the eps of loop step i; steps i >= n_eps draw fresh
 *   noise (`noise_tail` [K-n_eps,B,C,H,W] or Philox). coef_host: K rows in loop order index K-1..0
 *   stored at row index = k. x_out [B,C,H,W]. */
int cd_ddim_decode(cd_handle h, int net, int sched_kind, const float* z, int z_slots, int n_eps,
                   const float* ctx_c, const float* ctx_uc, int ctx_len, float guidance, int B, int K,
                   const cd_step_coef* coef_host, const float* noise_tail, uint64_t seed, float* x_out);

/* The same with one classifier-free-guidance scale PER SAMPLE (`guidance_per_sample`: device pointer, B floats, each
 * neither 0 nor 1): the ensemble loop of the text wrappers decodes every z at each of
 * `decoder_unconditional_guidance_scales` (stable_diffusion_stochastic_text_wrapper.py:155-166) - members that differ
 * only in that scale run as one batch. Per-sample arithmetic is that of cd_ddim_decode with the sample's scale. */
int cd_ddim_decode_v(cd_handle h, int net, int sched_kind, const float* z, int z_slots, int n_eps,
                     const float* ctx_c, const float* ctx_uc, int ctx_len, const float* guidance_per_sample, int B,
                     int K, const cd_step_coef* coef_host, const float* noise_tail, uint64_t seed, float* x_out);

/* Deterministic DDIM inversion, the encoder of the DDIB baseline: DiffusionCLIP's denoising_step(..., eta=0,
 * sampling_type='ddim') walked towards noise, t_next > t (model/lib/ddpm_ddim/utils/diffusion_utils.py:114-121).
 *   x0 [B,C,H,W]; ctx_* / guidance as cd_dpm_encode's (classifier-free guidance doubles the rows, ddim.py:550-559);
 *   coef_host: K rows in LOOP order, row j = step j: t = timestep of the input's level, sa / r = sqrt(a_in) /
 *   sqrt(1 - a_in), sap / dirc = sqrt(a_out) / sqrt(1 - a_out), sigma = 0 (required);
 *   step j: x0_hat = (x - r*e)/sa, x <- sap*x0_hat + dirc*e (one forward per step);
 *   x_out [B,C,H,W] = the last x; traj_out [K,B,C,H,W] (x after every step) or NULL. sched_kind must be CD_SCHED_DDIM. */
int cd_ddim_invert(cd_handle h, int net, int sched_kind, const float* x0, const float* ctx_c, const float* ctx_uc,
                   int ctx_len, float guidance, int B, int K, const cd_step_coef* coef_host, float* x_out,
                   float* traj_out);

/* Region-keeping decode: DDIMSampler.sample_with_eps(..., mask=, x0=) (ddim.py:170-228; the branch at :427-430). Ahead of the
 * forward of EVERY step, the first included, the running latent is replaced by
 *     x <- src_k * m + (1 - m) * x          (fp32, in that operation order; m = 1 keeps the source, m is broadcast over C)
 * and the blended x is what the network, x0_hat and the step formula see; nothing is blended after the last step.
 *   Everything up to `seed` as cd_ddim_decode; guidance_per_sample non-NULL selects cd_ddim_decode_v's per-sample scales
 *   (`guidance` is then ignored). mask [B_mask,1,H,W] in [0,1], x0 [B_mask,C,H,W], B a multiple of B_mask: sample b uses row
 *   b % B_mask (ensemble members folded into the batch share their sample's mask). mask_source must be CD_MASK_QSAMPLE here:
 *   src_k = qa[k]*x0 + qb[k]*n_k (LatentDiffusion.q_sample, ddpm.py:271-274) with qsample_coef_host = K rows of (qa, qb) =
 *   float32(sqrt(alphas_cumprod))[tau[k]], float32(sqrt(1 - alphas_cumprod))[tau[k]] stored at row index = k (the fp64 square
 *   roots of ddpm.py:141-142, NOT the sa / s1a of the DDIM table) and n_k = mask_noise[K-1-k] of mask_noise [K,B,C,H,W] (slot i
 *   = the draw of loop iteration i, the reference's randn_like(x_start)), or Philox(mask_seed) when mask_noise is NULL.
 * Refused (error text, nothing launched): sched_kind != CD_SCHED_DDIM and the pixel networks (the reference has no mask hook on
 * DDPMDDIMWrapper), B % B_mask != 0, CD_MASK_ENCODER (the encoder's trajectory does not exist in a separate decode). */
int cd_ddim_decode_masked(cd_handle h, int net, int sched_kind, const float* z, int z_slots, int n_eps, const float* ctx_c,
                          const float* ctx_uc, int ctx_len, float guidance, const float* guidance_per_sample, int B, int K,
                          const cd_step_coef* coef_host, const float* noise_tail, uint64_t seed, const float* mask,
                          const float* x0, int B_mask, int mask_source, const float* qsample_coef_host,
                          const float* mask_noise, uint64_t mask_seed, float* x_out);

/* ---- the coupled translate loop: cd_cycle_translate(h, &args), its options as structs of their own (NULL = off) ---------- */

/* The keep-mask on the decoder rows of cd_cycle_translate: the fields as the mask arguments of cd_ddim_decode_masked with the
 * decoder's batch n_dec*B in the place of B (noise [K,n_dec*B,C,H,W]; decoder row r uses mask row r % B_mask, B a multiple of
 * B_mask), x0 [B_mask,C,H,W] the x0 of the blend.
 *   source = CD_MASK_QSAMPLE: per-sample arithmetic of cd_dpm_encode followed by cd_ddim_decode_masked, bit for bit.
 *   source = CD_MASK_ENCODER: src_k = the encoder's x_t at level k of encoder sample r % B, bit for bit (x_T for the first
 *   forward); no noise is drawn; qsample_coef_host and noise must be NULL, x0 is not read.
 * A struct whose `mask` is NULL is refused; no keep-mask is cd_translate_args.mask = NULL. */
typedef struct cd_keep_mask {
  const float* mask;               /* [B_mask,1,H,W] in [0,1]; 1 keeps the source */
  const float* x0;                 /* [B_mask,C,H,W] */
  int B_mask;
  int source;                      /* CD_MASK_QSAMPLE / CD_MASK_ENCODER */
  const float* qsample_coef_host;  /* K rows of (qa, qb), row index = k */
  const float* noise;              /* [K,n_dec*B,C,H,W] or NULL -> Philox(seed) */
  uint64_t seed;
} cd_keep_mask;

/* Cross-attention control (prompt-to-prompt on the coupled loop; the paper's "CycleDiffusion + CAC") on the first n_ctrl
 * iterations (iteration 0 = the noisiest step), with or without a keep-mask. In every text
 * cross-attention of those iterations, head h of decoder CONDITIONAL row r (sample b = r % B) computes
 *     P = w * (alpha * (P_src . M) + (1 - alpha) * P_own),   O = P . V_own        (rows of P are not renormalised)
 * where P_own is the row's own softmax(Q K^T * scale) and P_src that of the encoder's conditional row of sample b in the SAME
 * forward against the source context; the products with alpha [L] and w [L] run over the key axis. mapper [B_ctrl,L,L],
 * alpha / weight [B_ctrl,L] are fp32 device tensors, B a multiple of B_ctrl: sample b uses entry b % B_ctrl (members of a
 * folded ensemble share their sample's control). Encoder rows, unconditional rows and iterations >= n_ctrl run exactly the
 * kernels of the call without control: z_out is bit-identical to the uncontrolled call's, and n_ctrl = 0 is that call.
 * Refused (error text, nothing launched): coefficient tables whose rows k < K disagree on the timestep (checked for every
 * n_ctrl), and for n_ctrl != 0: n_ctrl outside [0, K], sched_kind != CD_SCHED_DDIM, networks without a text context, networks
 * of precision CD_PREC_F32 / CD_PREC_F32X3, ctx_len > 96, B % B_ctrl != 0, a pass without conditional rows (guidance 0). */
typedef struct cd_attn_ctrl {
  const float* mapper;  /* [B_ctrl,L,L] */
  const float* alpha;   /* [B_ctrl,L] */
  const float* weight;  /* [B_ctrl,L] */
  int B_ctrl;
  int n_ctrl;
} cd_attn_ctrl;

/* Prompt-to-prompt's LocalBlend (Hertz et al. 2022; no counterpart in the reference tree,
 * DESIGN.md 18): the target is edited only where the word maps of this very sampling run - source branch and target branch
 * together - look at the chosen words; elsewhere the decoder's latent is held to the DPM-Encoder's own x_t of every level.
 * With or without cross-attention control; it excludes a keep-mask and semantic guidance. sel_src /
 * sel_tgt [B_sel,L] fp32 device weights over the key positions of the source / target prompt, B a multiple of B_sel.
 * With Bd = n_dec*B, k = K-1-i, h the latent side and f = h / side, iteration i does:
 *   1. The one forward over [enc rows | dec rows] of cd_cycle_translate. In every text cross-attention (attn2) of a
 *      transformer block whose token grid side equals `side`, for the encoder's CONDITIONAL rows (sample b, selector
 *      sel_src[b % B_sel]) and the decoder's CONDITIONAL rows (the last Bd rows; row r, selector sel_tgt[(r % B) % B_sel]):
 *          m[r, q] = (1/H) * sum_hd sum_j sel[j] * P_hd[q, j]   (hd ascending),   P = softmax(Q_own K_own^T * scale)
 *      (cd_word_maps' quantity with N = 1) - the row's OWN attention also in an iteration under control.
 *   2. acc[row] [side,side] fp32, zero before iteration 0, gains the layers one by one in the forward's order: one running
 *      sum over the iterations in loop order.
 *   3. The encoder's step kernel, unchanged: z_out is bit-identical to cd_cycle_translate's.
 *   4. If i >= n_start, the mask: for decoder row r, b = r % B, and each A of acc_src[b], acc_tgt[r]:
 *          p = max of A over |dy|, |dx| <= pool/2 inside the image;  mx = max p over the image;
 *          e_A = (mx > 0) && (p / mx > thr)                          (fp32 division)
 *      keep = 1 - (e_src | e_tgt), exact 0 / 1, each cell replicated f x f onto [Bd,1,h,w]; 1 = keep the source.
 *   5. The decode step of row k (cd_ddim_decode's arithmetic) and, if i >= n_start, the blend
 *          x <- src * keep + (1 - keep) * x       (fp32, in cd_ddim_decode_masked's operation order)
 *      with src = the encoder's x of the level just arrived at (after step 3), of encoder row r % B. Unlike the keep-mask
 *      entry points the blend also follows the LAST step (under last_uses_x0 the kept cells of x_out are x0 bit for bit), and
 *      nothing is blended ahead of the first forward. Iterations i < n_start run exactly the launches of the call without
 *      the blend.
 * acc_out [(B + Bd),side,side] or NULL: the final sums, source rows first. keep_out [Bd,1,h,w] or NULL: the mask of the last
 * iteration, all ones if n_start == K. thr < 0 edits everywhere a map is above 0, thr >= 1 edits nowhere.
 * Refused (error text, nothing launched), for every n_ctrl: tables whose rows k < K disagree on the timestep, sched_kind !=
 * CD_SCHED_DDIM, networks without a text context, precision CD_PREC_F32 / CD_PREC_F32X3, ctx_len > 96, a pass without
 * conditional rows (guidance 0); B % B_sel != 0; side > 64, h % side != 0, a side that matches no block; pool even or outside
 * [1, 7]; n_start outside [0, K]; thr not finite; a keep-mask or concepts in the same call; and what cd_attn_ctrl refuses of
 * the control for n_ctrl != 0. */
typedef struct cd_local_blend {
  const float* sel_src;  /* [B_sel,L] */
  const float* sel_tgt;  /* [B_sel,L] */
  int B_sel;
  int side;
  int pool;
  float thr;
  int n_start;
  float* acc_out;        /* [B+n_dec*B,side,side] or NULL */
  float* keep_out;       /* [n_dec*B,1,h,w] or NULL */
} cd_local_blend;

/* One edit concept of semantic guidance. Its quantile threshold q in [0, 1] over the N = C*H*W values of a latent arrives as
 * the rank and the weight of the two order statistics it lies between, computed by the caller in float64:
 * lo = floor(q*(N-1)), frac = (float)(q*(N-1) - lo); the kernels see no float64 and no q. */
typedef struct cd_sega_concept {
  float scale;   /* s_e, signed: negative steers away from the concept */
  float weight;  /* w_e of the sum over concepts */
  int32_t lo;    /* in [0, N-1] */
  float frac;    /* in [0, 1) */
  int32_t warm;  /* the concept is active on iterations warm <= i < cool (iteration 0 = the noisiest step) */
  int32_t cool;
} cd_sega_concept;

/* Semantic guidance (SEGA; Brack et al., NeurIPS 2023; no counterpart in the
 * reference tree): E edit concepts, each a text context with its own signed scale, threshold, weight and window
 * of iterations, steer the decoder rows beside the one target prompt. With or without a keep-mask and cross-attention
 * control. edit_ctx [E*Bd,L,Dc] fp32 device, concept-major (row e*Bd + r is
 * concept e for decoder row r, Bd = n_dec*B), concepts_host [E] and the momentum's scale s_m and decay beta.
 * The forward of every iteration runs over the batch rows
 *     [ enc (uncond | cond) | dec uncond Bd | dec concept 0 Bd | ... | dec concept E-1 Bd | dec cond Bd ]
 * every concept row on the decoder row's latent. With u, c, p_e the network's outputs of decoder row r's unconditional,
 * conditional and concept-e rows, g_r the row's guidance scale and N = C*H*W, iteration i computes per element j, in fp32
 * in this operation order without contraction:
 *     base   = u + g_r * (c - u)
 *     d_e    = (p_e - u) * s_e ,  a_e = |d_e|                       for the concepts with warm_e <= i < cool_e
 *     tau_e  = A[lo_e] + (A[hi_e] - A[lo_e]) * frac_e               A = the N values a_e[r, .] ascending, hi = min(lo+1, N-1)
 *     m_e    = (a_e >= tau_e) ? d_e : 0
 *     gamma  = ((0 + w_0*m_0) + w_1*m_1) + ...                      active concepts only, ascending e
 *     gamma' = gamma + s_m * nu[r, j]
 *     nu[r,j] <- beta * nu[r,j] + (1 - beta) * gamma'               nu = 0 before iteration 0; updated in every iteration
 *     eps    = base + gamma'
 * and the decode step of row k = K-1-i (cd_ddim_decode's arithmetic, the keep-mask blend included) consumes eps in the place
 * of the classifier-free-guidance combine. tau is torch.quantile(|d|.flatten(1), q, dim = 1) to rounding; q = 0 keeps
 * every element, q = 1 only the maximum. The order statistics are exact (radix selection on the bit patterns); a NaN sorts
 * above +inf. An inactive concept contributes nothing: the momentum is built from applied guidance only. The encoder's rows,
 * the unconditional and conditional rows and z_out are those of the call without concepts, bit for bit; nothing is kept
 * between calls.
 * tau_out [K,Bd,E] fp32, kept_out [K,Bd,E] int32 (#{a_e >= tau_e}), both by iteration and 0 where the concept is inactive;
 * mask_out [Bd,E,C,H,W] fp32 of 0 / 1: the kept elements of the last iteration in which any concept was active, 0 for a
 * concept inactive in it. Each may be NULL.
 * Refused (error text, nothing launched): E outside [1, 8]; sched_kind != CD_SCHED_DDIM; a network without a text context;
 * precision CD_PREC_F32 / CD_PREC_F32X3; a decoder pass without both its unconditional and its conditional rows
 * (dec_guidance 0 or 1, a missing context); lo outside [0, N-1]; frac outside [0, 1); warm / cool outside
 * 0 <= warm <= cool <= K; a non-finite scale, weight, momentum_scale or momentum_beta; momentum_beta outside [0, 1]; tables
 * whose rows k < K disagree on the timestep; and what cd_keep_mask / cd_attn_ctrl refuse of a mask or a control. The
 * local blend (cd_local_blend) is not built together with concepts. */
typedef struct cd_sega {
  const float* edit_ctx;                 /* [E*n_dec*B,L,Dc], concept-major */
  const cd_sega_concept* concepts_host;  /* [E] */
  int E;
  float momentum_scale;
  float momentum_beta;
  float* tau_out;                        /* [K,n_dec*B,E] or NULL */
  int32_t* kept_out;                     /* [K,n_dec*B,E] or NULL */
  float* mask_out;                       /* [n_dec*B,E,C,H,W] or NULL */
} cd_sega;

/* The coupled source -> target loop in ONE call: what Model.forward composes from the wrapper's encode() and forward()
 * (model/text_unsupervised_translation.py:24-40: z = gan_wrapper.encode(image, encode_text); img = gan_wrapper(z, ...)) when
 * both run on the same network over the whole chain (white_box_steps = custom_steps + 1): the DPM-Encoder step and the decode
 * step of index k evaluate the network at the same timestep, and the decode step needs eps_k only after its forward, so each
 * of the K iterations runs ONE forward over [encoder rows | decoder rows], then the encoder's step kernel (ddim.py:582-601,
 * 545-580) and the decoder's (ddim.py:603-646), which reads the eps the encoder just wrote.
 *   x0 [B,C,H,W]; enc_ctx_* [B,L,Dc] and enc_guidance as cd_dpm_encode's; the decoder runs n_dec decodes per encoder sample
 *   (the wrapper's decoder_unconditional_guidance_scales of one kind, sd_wrapper:155-166): dec_ctx_* [n_dec*B,L,Dc], decoder
 *   row j*B + b decodes the z of encoder sample b; dec_guidance (scalar) or dec_guidance_per_sample (device, n_dec*B floats,
 *   each neither 0 nor 1) as cd_ddim_decode / cd_ddim_decode_v; coef_enc_host K+1 rows, coef_dec_host K rows (the same rows
 *   0..K-1); noise [K,B,C,H,W] or NULL and last_uses_x0 as cd_dpm_encode's.
 *   z_out [B,K+1,C,H,W] (what encode() returns), x_out [n_dec*B,C,H,W] (what the decode returns).
 * The caller sets `size` to sizeof(cd_translate_args): a call built against another layout of the struct is refused before
 * anything is read from it. mask / ctrl / blend / sega: NULL = the feature is off; each struct says what it adds and what is
 * refused with it. The structs are read during the call only.
 *
 * Fused windows (MultiDiffusion, Bar-Tal et al. 2023; no counterpart in the reference tree): images larger than
 * the network. n_win > 0 puts the running latents on a canvas of canvas_h x canvas_w latent cells (each >= S = image_size)
 * covered by n_win S x S windows, win_host [n_win, 2] int32 HOST pairs (y, x) of their top-left cells. x0, noise, z_out and
 * x_out then have canvas_h x canvas_w in the place of H x W, and so have the element indices of the counter-based generator.
 * Each iteration crops every window of the encoder's and of the decoder's latent into network rows (window-major inside each
 * [uncond | cond] part, the contexts repeated per window), runs the ONE forward over n_win x the rows of the call without
 * windows, and defines the noise prediction of a canvas cell, per part, as
 *     acc = e_{w_first};  acc = acc + e_w  (the other windows that cover the cell, ascending w);  eps = acc / (float)count
 * in fp32 without contraction; the guidance combine and the step arithmetic are those of the call without windows, on the
 * canvas. Encoder and decoder share the fused prediction, so z_out and the decode are the unchanged arithmetic on a bigger
 * tensor and the cycle of the same prompt at guidance 1 still closes. One window (0, 0) on an S x S canvas is the call without
 * windows, bit for bit. n_win = 0 is off: canvas_h, canvas_w must be 0 and win_host NULL.
 * Refused (error text, nothing launched): n_win outside [0, 64]; a canvas smaller than S; a window outside the canvas; two
 * equal windows; a canvas cell that no window covers; precision CD_PREC_F32 / CD_PREC_F32X3; a keep-mask, control, blend or
 * concepts in the same call - windows are not built together with mask / ctrl / blend / sega yet. */
typedef struct cd_translate_args {
  uint32_t size;
  int net;
  int sched_kind;
  const float* x0;
  const float* enc_ctx_c;
  const float* enc_ctx_uc;
  float enc_guidance;
  const float* dec_ctx_c;
  const float* dec_ctx_uc;
  float dec_guidance;
  const float* dec_guidance_per_sample;
  int ctx_len;
  int B;
  int n_dec;
  int K;
  const cd_step_coef* coef_enc_host;
  const cd_step_coef* coef_dec_host;
  const float* noise;
  uint64_t seed;
  int last_uses_x0;
  float* z_out;
  float* x_out;
  const cd_keep_mask* mask;
  const cd_attn_ctrl* ctrl;
  const cd_local_blend* blend;
  const cd_sega* sega;
  int canvas_h;
  int canvas_w;
  int n_win;
  const int32_t* win_host;
} cd_translate_args;

int cd_cycle_translate(cd_handle h, const cd_translate_args* a);

/* ILVR (Choi et al., ICCV 2021: Iterative Latent Variable Refinement), the reference-image-conditioned sampler of the
 * paper's unpaired table; no counterpart in the reference tree. cd_ddim_decode's loop on an unconditional
 * pixel DDPM, with the running image pulled to the low-pass band of a reference image after the step of every row k > range_t:
 *     x' = the decode step of row k (sched_kind, bit for bit cd_ddim_decode's)
 *     y' = qa_k * ref + qb_k * n_k,  x = x' + phi_N(y' - x'),  phi_N(X) = U D X D^T U^T per channel image,
 * D the antialiased cubic down-by-down_n [R / down_n, R] and U the cubic up-by-down_n (cycle-diffusion_amd/utils/lowpass.py;
 * fp32, taps ascending, rows then columns). Row 0 is never conditioned; range_t >= K - 1 conditions nothing and is
 * cd_ddim_decode bit for bit.
 *   Arguments up to `seed` as cd_ddim_decode's, without contexts and guidance. ref [B_ref,C,R,R] in [-1, 1], B a multiple of
 *   B_ref: sample b uses row b % B_ref. qsample_coef_host: K rows of (qa, qb) = (sqrt(abar), sqrt(1 - abar)) of the level the
 *   step of row k ARRIVES at, row index = k (PixelSchedule.coef_ilvr). n_k = ref_noise[K-1-k] of ref_noise [K,B,C,R,R] (slot i =
 *   the draw of loop iteration i) or Philox(ref_seed) when ref_noise is NULL.
 * Refused (error text, nothing launched): networks with a text context, down_n < 1, R % down_n != 0, R / down_n < 4,
 * range_t < 0, B % B_ref != 0, qsample_coef_host == NULL, R > 1024. down_n = 1 is the identity filter: x = x' + (y' - x'). */
int cd_ilvr_decode(cd_handle h, int net, int sched_kind, const float* z, int z_slots, int n_eps, int B, int K,
                   const cd_step_coef* coef_host, const float* noise_tail, uint64_t seed, const float* ref, int B_ref,
                   int down_n, int range_t, const float* qsample_coef_host, const float* ref_noise, uint64_t ref_seed,
                   float* x_out);

/* Keep-mask estimation from the two prompts (DiffEdit, Couairon et al. 2022, step 1; no counterpart in the reference tree,
 * DESIGN.md 16): where do the noise predictions under the source and under the target context disagree on the noised source?
 *     x_i = qa*x0 + qb*n_i (fp32, in that order), i < n_draws; one forward over rows [src (i, b) | tgt (i, b)] at timestep t
 *     (cd_unet_forward's call on those rows; the second half of its input is the copy of the first);
 *     map[b, p]  = (sum_i sum_c |e_tgt[i,b,c,p] - e_src[i,b,c,p]|) / float(n_draws * C)   (i ascending, c ascending inside)
 *     mean[b]    = (sum_p map[b, p]) / HW per image (fixed order, independent of B);  cl = ratio * mean[b]
 *     v = min(map, cl) / cl (0 where cl == 0);  edit = v > thr;  edit' = max of edit over |dy|, |dx| <= dilate inside the image
 *     keep_out [B,1,H,W] = 1 - edit' (exact 0 / 1; 1 = keep the source, the orientation of `mask` everywhere);
 *     map_out [B,1,H,W] or NULL.
 *   x0 [B,C,H,W]; ctx_src / ctx_tgt [B,L,Dc]; (t, qa, qb): the level - qa / qb as a row of cd_ddim_decode_masked's q-sample
 *   table, t its timestep; noise [n_draws,B,C,H,W] or NULL -> Philox(seed), stream 0x6000 + i, element = the flat index in
 *   [B,C,H,W]. max_rows: the most rows a forward may have; max(1, max_rows / (2B)) draws run per forward, and the result does not
 *   depend on that cut, bit for bit. Classifier-free guidance needs no rows here: eps_g(tgt) - eps_g(src) = g (e_c(tgt) -
 *   e_c(src)) for one x_t, and the division by the image's own mean cancels g. Any precision of the network.
 * Refused (error text, nothing launched): networks without a text context (the pixel DDPMs), n_draws outside [1, 4095],
 * ratio <= 0, thr outside [0, 1), dilate outside [0, 8], max_rows < 2B. */
int cd_automask(cd_handle h, int net, const float* x0, const float* ctx_src, const float* ctx_tgt, int ctx_len, int B,
                int n_draws, int t, float qa, float qb, const float* noise, uint64_t seed, int max_rows, float ratio, float thr,
                int dilate, float* map_out, float* keep_out);

/* Per-word cross-attention heat maps (DAAM, Tang et al. 2022; the maps prompt-to-prompt's local blend thresholds; no counterpart
 * in the reference tree): how much softmax mass do the text cross-attentions put on chosen words, per pixel?
 *     x_i = qa*x0 + qb*n_i (fp32, in that order), i < n_draws; rows [draw i, sample b] through ONE conditional forward per
 *     chunk at timestep t - no unconditional rows. In every transformer block whose token grid side s has
 *     min_side <= s <= max_side (0, 0: every block), for the block's text cross-attention (attn2), row r, query q:
 *         P = softmax(Q K^T * scale) over the L keys
 *         m_layer[r, n, q] = (1/H) * sum_hd sum_j sel[b % B_sel, n, j] * P_hd[q, j]                (hd ascending)
 *     maps_out[b, n, y, x] = (1 / (n_draws * n_layers)) * sum_i sum_layer m_layer[i*B + b, n, (y / f)*s + (x / f)],  f = h / s
 *     (nearest replication onto the latent grid; fp32 throughout; per draw the layers are added in the forward's order, then the
 *     draws in ascending order). n_layers_out (or NULL): the number of blocks included.
 *   x0 [B,C,h,w]; ctx [B,L,Dc]; sel [B_sel,N,L] fp32 weights over the key positions, N words, sample b uses entry b % B_sel;
 *   (t, qa, qb): the level, as cd_automask takes it; noise [n_draws,B,C,h,w] or NULL -> Philox(seed), stream 0x8000 + i, element
 *   = the flat index in [B,C,h,w] (the band at 0x7000 holds the VAE posterior's 0x7a65). max_rows: the most rows a forward may
 *   have; max(1, max_rows / B) draws run per forward, and the result does not depend on that cut, bit for bit. The collection
 *   changes no bit of the network's own output, and a forward without it runs the launches it always ran.
 * Refused (error text, nothing launched): networks without a text context, fp32 / fp32x3 precision, ctx_len > 96, N outside
 * [1, 8], n_draws outside [1, 4095], B % B_sel != 0, max_rows < B, min_side > max_side, a side window that matches no block. */
int cd_word_maps(cd_handle h, int net, const float* x0, const float* ctx, int ctx_len, int B, const float* sel, int B_sel,
                 int N, int n_draws, int t, float qa, float qb, const float* noise, uint64_t seed, int max_rows,
                 int min_side, int max_side, float* maps_out /* [B,N,h,w] */, int* n_layers_out);

/* Stochastic refinement (ddpm_ddim_wrapper.py:431-453): x_t = sa*x + s1a*n (row R of coef_host),
 * then R random-noise steps rows R-1..0. noise [R+1,B,C,H,W] or NULL. In/out x [B,C,H,W]. */
int cd_pix_refine(cd_handle h, int net, int sched_kind, float* x, int B, int R,
                  const cd_step_coef* coef_host, const float* noise, uint64_t seed);

/* ---- single-kernel entry points (parity tests call the HIP kernels through these) ----------- */
int cd_op_pack_conv_weight(cd_handle h, const float* w_host, int N, int Cin, int KH, int KW, int geglu,
                           void** packed_dev, int* Npad, int* Cpad);
int cd_op_free(cd_handle h, void* dev);
/* x: fp32 NCHW [B,C0(,+C1),H,W] (x1 optional second source); y: fp32 NCHW [B,N,Ho,Wo] */
int cd_op_conv2d(cd_handle h, const float* x0, int C0, const float* x1, int C1, int B, int H, int W,
                 const void* packed_w, int N, int KH, int KW, int stride, int pad, int asym_pad, int up,
                 const float* bias, const float* rowvec, const float* resid, int act, int tile, float* y);
/* the same convolution with the engine's 16-bit output (the product path's format; y still arrives as fp32 NCHW) and,
 * if `stats` is given, the fused GroupNorm statistics of the output: fp32 [B*Ho*Wo / 32][2][N] = per-channel sum |
 * sum of squares over each block of 32 rows. tile = 30 selects the streaming K = 320 linear kernel (lin_stream.hip);
 * act | 0x400 additionally LayerNorm-s the input rows inside that kernel (statistics only, eps 1e-5; >= 65536 rows). */
int cd_op_conv2d_16(cd_handle h, const float* x0, int C0, const float* x1, int C1, int B, int H, int W,
                    const void* packed_w, int N, int KH, int KW, int stride, int pad, int asym_pad, int up,
                    const float* bias, const float* rowvec, const float* resid, int act, int tile, float* y,
                    float* stats);
/* what the calling thread's most recent implicit-GEMM launch (any convolution / linear layer, the two entry points above
 * included) ran after every fallback of the launcher: tile_id = the tile configuration whose instantiation was launched (a
 * configuration without a 32-deep instantiation of its own reports the one it borrows; 30 = the streaming linear kernel),
 * bk = K-step depth (32 or 64), splitk = effective split-K factor (1 = none), chm = 1 if the channel-major K order was taken,
 * tile_group = group size of the tile walk (0 = row-major). Read-only; any pointer may be NULL. */
int cd_op_last_gemm_config(cd_handle h, int* tile_id, int* bk, int* splitk, int* chm, int* tile_group);
/* the reorder pass behind a phase-form x2 convolution on its own (16-bit values): x fp32 [B, 4, C, H, W], the second index
 * the output parity 2 a + b -> y fp32 NCHW [B, C, 2 H, 2 W] with y[.., 2 i + a, 2 j + b] = x[.., 2 a + b, .., i, j]; C % 8 == 0.
 * cd_op_conv2d_16 with up = 1 takes the phase form (and this pass) for 3 x 3 weights without a residual on images of a
 * multiple of 256 pixels, unless the environment says CYCLEDIFF_UP_PHASE=0 at the time of the call. */
int cd_op_up_phase_reorder(cd_handle h, const float* x, int B, int C, int H, int W, float* y);
int cd_op_groupnorm(cd_handle h, const float* x, int B, int C, int H, int W, int G, float eps,
                    const float* gamma, const float* beta, const float* film, int silu, float* y);
/* GroupNorm(32) the way the networks call it. x0 fp32 NCHW [B,C0,H,W] and, if x1 is given, x1 [B,C1,H,W]: the channel
 * concat [x0 | x1] is normalised. Each source is stored NHWC with row stride C + pad; the pad columns hold NaN. film: fp32
 * [B][film_ld] rows of scale(C) | shift(C), film_ld = 0: one row shared by the batch. stats0 / stats1 (either may be NULL):
 * the block statistics a producing convolution's epilogue writes, fp32 [B*H*W / 32][2][C0] and [..][2][C1] (see
 * cd_op_conv2d_16); they are used only where the networks would use them (both sources carry them, pad = 0, H*W % 32 == 0),
 * otherwise the tensor is read. precision: 0 = the 16-bit path (y fp32 NCHW [B,C0+C1,H,W]), 1 = the fp32 path (the same),
 * 2 = its split mode: y receives the raw fp16 pairs [B*H*W][hi(C) | lo(C)], value = (hi + lo) / 16, and the call fails
 * with the range-guard error when an output left the representable range (|y| >= 4094). */
int cd_op_groupnorm_ex(cd_handle h, const float* x0, int C0, int pad0, const float* x1, int C1, int pad1, int B, int H,
                       int W, float eps, const float* gamma, const float* beta, const float* film, int film_ld, int silu,
                       const float* stats0, const float* stats1, int precision, void* y);
/* ---- single-kernel entry points of the fp32 execution path (CD_PREC_F32 = precision 1, CD_PREC_F32X3 = precision 2) ----
 * The engine's building blocks as the networks call them. Activations are stored with row stride C + pad (pad % 4 == 0 where a
 * kernel reads vectors); the pad columns hold NaN. Precision 2 results that are split activations arrive as the raw fp16 pairs
 * [rows][hi(C) | lo(C)], value = (hi + lo) / 16; every call synchronises and fails with the range-guard error ("fp16 range") when
 * a scaled value left the fp16 range. */
/* weights for cd_op_conv2d_prec: fp32 rows and (fp16 build) their three-term split [wh | wh | wl]; |w| >= 255 raises here */
int cd_op_pack_conv_weight_prec(cd_handle h, const float* w_host, int N, int Cin, int KH, int KW, int geglu,
                                void** packed_dev);
/* precision 1: conv_fwd -> k_conv_f32 (the channel concat [x0 | x1] inside the kernel). precision 2: the input in split form
 * (one source, via_split_rows = 0: straight from NCHW as the U-Net input is uploaded; otherwise split_rows_f32_fwd(x0, x1) on the
 * padded fp32 rows) -> the three-term GEMM with its fp32 residual and, if `stats` is given, the GroupNorm block statistics
 * of the output (fp32 [B*Ho*Wo / 32][2][N]; an error where the convolution writes none). rowvec: fp32 [B][N], or one [N] row
 * with rowvec_shared; resid: fp32 NCHW [B,N,Ho,Wo], stored with row stride N + resid_pad (any resid_pad >= 0); raw_geglu:
 * weights packed with geglu = 1 leave their [32 value | 32 gate] column blocks as they are; y = fp32 NCHW [B,N,Ho,Wo]. */
int cd_op_conv2d_prec(cd_handle h, const float* x0, int C0, int pad0, const float* x1, int C1, int pad1, int B, int H, int W,
                      const void* packed_w, int N, int KH, int KW, int stride, int pad, int asym_pad, int up,
                      const float* bias, const float* rowvec, int rowvec_shared, const float* resid, int resid_pad, int act,
                      int raw_geglu, int tile, int precision, int via_split_rows, float alpha, float* y, float* stats);
/* q [B,Tq,H*D], k, v [B,Tk,H*D] fp32 -> o [B,Tq,H*D]. mode 0 = attention_f32_fwd on a fused q | k tensor (row stride
 * 2 H D + padq; flash for D <= 160, else one wave per query), 1 = the wave-per-query kernel forced, both with Tq = Tk and an
 * optional output bias [H*D]; 2 = attention_flash_f32_fwd with separate q / k / v row strides H D + pad, Tq != Tk, q_log2
 * (q already carries scale * log2 e) and, at precision 2, the split output. */
int cd_op_attention_prec(cd_handle h, const float* q, const float* k, const float* v, int B, int H, int Tq, int Tk, int D,
                         int padq, int padk, int padv, float scale, int q_log2, const float* obias, int mode, int precision,
                         void* o);
/* row-wise pieces on fp32 rows x0 [rows][C0] (stride C0 + pad0): op 0 = layernorm_fwd (eps 1e-5), 1 = geglu_f32_fwd
 * (C0 = 2 Nout in the packed [32 value | 32 gate] order -> [rows][Nout]), 2 = split_rows_f32_fwd(x0, x1) (precision 2 only) */
int cd_op_rows_prec(cd_handle h, int op, const float* x0, int64_t rows, int C0, int pad0, const float* x1, int C1, int pad1,
                    const float* gamma, const float* beta, int precision, void* y);
/* x fp32 NCHW [B,C,H,W]: op 0 = avgpool2_fwd (precision 1 -> y fp32 NCHW [B,C,H/2,W/2]; precision 2: split input and
 * output, y = the raw pairs [B*H/2*W/2][2C]), op 1 = upsample2_fwd (precision 1, y fp32 NCHW [B,C,2H,2W]) */
int cd_op_resample_prec(cd_handle h, int op, const float* x, int B, int C, int H, int W, int precision, void* y);
int cd_op_layernorm(cd_handle h, const float* x, int rows, int C, const float* gamma, const float* beta,
                    float eps, float* y);
/* the entry of a 320-channel SpatialTransformer block with 40-wide heads on the 16-bit path, as the U-Net runs it:
 * x fp32 NCHW [B,320,H,W] -> h = proj_in(GroupNorm32(x)) (h_out, NCHW [B,320,H,W]), [q | k] = [to_q | to_k](LayerNorm(h))
 * (qk_out, NCHW [B,640,H,W]) and V^T = to_v(LayerNorm(h))^T per image (vt_out, [B][320][round_up(H*W, 64)]). w_in, w_qk
 * ([to_q rows; to_k rows], 640 x 320) and w_v are handles of cd_op_pack_conv_weight; every other pointer is fp32 device
 * memory (b_in, v_bias may be NULL). stages: bit 0 = one q | k | v launch of the streaming kernel with a V^T exit, bit 1 =
 * LayerNorm folded into it (needs bit 0), bit 2 = the GroupNorm apply inside proj_in's launch; -1 = what CYCLEDIFF_ST_ENTRY
 * says (default 7). Shapes the fused launches do not take (H*W % 256 != 0, fewer rows than the streaming kernel's
 * threshold of 32 768; bit 1 also where CYCLEDIFF_LN_FOLD / CYCLEDIFF_LN_FOLD_MIN_ROWS keep the other LayerNorm folds off)
 * run the separate launches whatever `stages` says; *stages_run (may be NULL) receives the bits whose launches ran.
 * v_bias needs bit 0 in effect. The two derived 960 x 320 weights are allocated once per (engine, w_qk, w_v) and live, like
 * every op weight, until the engine is destroyed; each call refills them. */
int cd_op_st_entry(cd_handle h, const float* x, int B, int H, int W, const float* gn_gamma, const float* gn_beta,
                   float gn_eps, const void* w_in, const float* b_in, const float* ln_gamma, const float* ln_beta,
                   const void* w_qk, const void* w_v, const float* v_bias, int stages, float* h_out, float* qk_out,
                   float* vt_out, int* stages_run);
/* q [B,Tq,H*D], k,v [B,Tk,H*D] fp32 -> o [B,Tq,H*D]; use_transpose_kernel: 0 = V consumed token-major (the U-Net
   path: fused q|k|v projection, LDS transpose reads), 1 = V pre-transposed to [B,H,D,Tk_pad] first */
int cd_op_attention(cd_handle h, const float* q, const float* k, const float* v, int B, int H, int Tq,
                    int Tk, int D, float scale, int use_transpose_kernel, float* o);
/* one launch of the controlled cross-attention (k_cross_attention_ctrl) on caller tensors, fp32 device: q_own [B,Tq,H*D],
   q_src [B_src,Tq,H*D], k_own [B,L_buf,H*D], k_src [B_src,L_buf,H*D] (rows L..L_buf-1 of each sample are never used),
   v_own [B,L,H*D], mapper [B_ctrl,L,L], alpha / weight [B_ctrl,L] -> o [B,Tq,H*D]; row b uses source b % B_src and control
   b % B_ctrl. L <= 96, D in {32, 40, 64, 80, 160}. */
int cd_op_cross_attention_ctrl(cd_handle h, const float* q_own, const float* q_src, const float* k_own, const float* k_src,
                               const float* v_own, const float* mapper, const float* alpha, const float* weight, int B,
                               int B_src, int B_ctrl, int H, int Tq, int L, int L_buf, int D, float scale, float* o);
/* cd_op_cross_attention_ctrl with q_log2 (both q tensors already carry scale * log2 e; scale is then ignored) and an output
   row stride of H*D + opad (opad % 4 == 0): o [B*Tq][H*D + opad] comes back pad columns included - the 16-bit output buffer
   starts as NaN, so a column the kernel did not write reads NaN. */
int cd_op_cross_attention_ctrl_ex(cd_handle h, const float* q_own, const float* q_src, const float* k_own, const float* k_src,
                                  const float* v_own, const float* mapper, const float* alpha, const float* weight, int B,
                                  int B_src, int B_ctrl, int H, int Tq, int L, int L_buf, int D, float scale, int q_log2,
                                  int opad, float* o);
/* one launch of the per-word map kernel (k_cross_attention_maps) on caller tensors, fp32 device: q [B,Tq,H*D], k [B,L_buf,H*D]
   (rows L..L_buf-1 of each sample are never used), sel [B_sel,N,L] -> maps [B,N,Tq] = (1/H) sum_hd sum_j sel[b % B_sel,n,j]
   P_hd[q,j]. q_log2: q already carries scale * log2 e (scale is then ignored). L <= 96, N <= 8, D in {32, 40, 64, 80, 160}. */
int cd_op_cross_attention_maps(cd_handle h, const float* q, const float* k, const float* sel, int B, int B_sel, int H,
                               int Tq, int L, int L_buf, int D, int N, float scale, int q_log2, float* maps /* [B,N,Tq] */);
/* launch_attention in the operand forms the networks use. q [B,Tq,H*D], k, v [B,Tk,H*D] fp32 as cd_op_attention takes them,
 * staged as 16-bit tensors by `layout`: 0 = three tensors, each padded: row strides H*D + pad (q), H*D + 2 pad (k),
 * H*D + 3 pad (v), so that no two are equal; 1 = q | k as column blocks of one
 * tensor of row stride 2 H*D + pad (k = q + H*D; Tq = Tk), v apart with stride H*D + pad; 2 = q | k | v in one tensor of row
 * stride 3 H*D + pad (Tq = Tk, token-major V only). pad % 8 == 0. v_transposed: V^T [B][H][D + d_extra][round_up(Tk, 64) +
 * 64 t_extra] made by the transpose kernel (its padding: zeros), else V token-major where it was staged. q_log2: q already
 * carries scale * log2 e (scale is then ignored); obias: fp32 [H*D] or NULL; causal: key j visible to query i iff j <= i.
 * o: fp32 [B*Tq][H*D + opad] (opad % 4 == 0), pad columns included. Every staged 16-bit buffer, the output included, starts
 * as 0xFF bytes (NaN in fp16 and bf16) and has one more 64-row block of them behind its last row. */
int cd_op_attention_ex(cd_handle h, const float* q, const float* k, const float* v, int B, int H, int Tq, int Tk, int D,
                       int layout, int pad, int v_transposed, int d_extra, int t_extra, float scale, int q_log2,
                       const float* obias, int causal, int opad, float* o);
/* y = phi_N(x) on caller tensors, fp32 NCHW [B,C,R,R], through the two kernels of cd_ilvr_decode (x' = 0, qa = 1, qb = 0);
 * refused as cd_ilvr_decode refuses its geometry. */
int cd_op_lowpass(cd_handle h, const float* x, int B, int C, int R, int down_n, float* y);
int cd_op_softmax_rows(cd_handle h, const float* s, int64_t rows, int cols, float* p);
int cd_op_timestep_embedding(cd_handle h, const float* t, int B, int dim, int mode, float* out);
/* one scheduler step on explicit tensors (bit-exact checks): mode 0 init_xt, 1 encode, 2 decode */
int cd_op_sched_step(cd_handle h, int mode, int sched_kind, const cd_step_coef* coef_host, const float* x0,
                     float* xt, const float* eps_hat, int cfg, float guidance, const float* noise,
                     const float* eps_in, int is_last, int B, int C, int HW, float* z_slot);
/* n raw draws of the counter-based Gaussian generator every sampler falls back to when its noise pointer is NULL
 * (Philox4x32-10 + Box-Muller, csrc/gauss.h): out[i] = the draw of element first + i of (seed, stream), fp32 device, i < n.
 * The stream of every loop is tabulated in DESIGN.md section 3; a loop that draws refuses more than 4095 steps, the width
 * of its band. `first` reaches the element indices around 2^32 and 2^33 with a handful of elements. */
int cd_op_gauss(cd_handle h, uint64_t seed, uint32_t stream, int64_t first, int64_t n, float* out);
/* the reduction of cd_automask (the same kernels) on caller-built predictions: eps_src / eps_tgt fp32 device [n,B,C,H,W] ->
 * map_out [B,1,H,W] (or NULL), mean_out [B] (or NULL), keep_out [B,1,H,W]; refused as cd_automask refuses n, ratio, thr, dilate */
int cd_op_automask_reduce(cd_handle h, const float* eps_src, const float* eps_tgt, int n, int B, int C, int H, int W,
                          float ratio, float thr, int dilate, float* map_out, float* mean_out, float* keep_out);
/* one launch of the local blend's (cd_local_blend) mask kernel (k_local_blend_mask, step 4 of its definition) on caller-built sums:
 * acc_src [B,side,side], acc_tgt [Bd,side,side] fp32 device, Bd a multiple of B -> keep_out [Bd,1,side*f,side*f] of 0 / 1.
 * Refused: side outside [1, 64], f < 1, pool even or outside [1, 7], Bd % B != 0. */
int cd_op_local_blend_mask(cd_handle h, const float* acc_src, const float* acc_tgt, int B, int Bd, int side, int f, int pool,
                           float thr, float* keep_out);
/* the two kernels of the fused windows (cd_translate_args.n_win) on caller tensors. win_host [n_win,2] int32 HOST pairs (y, x),
 * checked as cd_cycle_translate checks them. gather: x [Bp,C,Hc,Wc] fp32 -> y_out [(1+dup)*n_win*Bp, S*S, cpad], the 16-bit
 * rows of the network input widened to fp32: row d*n_win*Bp + w*Bp + b is x[b, :, y_w:y_w+S, x_w:x_w+S] rounded to the format
 * of cd_act_format(), channels C..cpad-1 zero; dup 0 or 1, cpad a multiple of 8. fuse: e [parts*n_win*Bp, S*S, ld] fp32 (row
 * d*n_win*Bp + w*Bp + b, the first C of ld channels) -> out [parts*Bp,C,Hc,Wc]: per cell acc = e_{w_first}, acc = acc + e_w over
 * the covering windows in ascending w, out = acc / (float)count. */
int cd_op_window_gather(cd_handle h, const float* x, const int32_t* win_host, int n_win, int Bp, int C, int Hc, int Wc, int S,
                        int cpad, int dup, float* y_out);
int cd_op_window_fuse(cd_handle h, const float* e, const int32_t* win_host, int n_win, int Bp, int C, int Hc, int Wc, int S,
                      int ld, int parts, float* out);
/* the masked step kernels on explicit tensors (bit-exact checks). mode 0: x <- blend(x) (the blend ahead of the first forward);
 * mode 2: the CD_SCHED_DDIM decode step of cd_op_sched_step followed, when blend != 0, by the blend. src [B_mask,C,HW] is x0
 * (CD_MASK_QSAMPLE: src_k = qa*x0 + qb*mask_noise, mask_noise [B,C,HW] required) or the source latent itself (CD_MASK_ENCODER);
 * xin16_out (or NULL): the next forward's 16-bit NHWC input [B (2B with cfg_dup), HW, C] in the format of cd_act_format(). */
int cd_op_sched_step_masked(cd_handle h, int mode, const cd_step_coef* coef_host, float* x, const float* eps_hat, int cfg,
                            float guidance, const float* eps_in, const float* mask, const float* src, int B_mask,
                            int mask_source, float qa, float qb, const float* mask_noise, int blend, int B, int C, int HW,
                            void* xin16_out, int cfg_dup);
/* one iteration of semantic guidance (cd_sega) - its two launches, k_sega_threshold and k_sega_combine - on caller
 * tensors (bit-exact checks). eps_all [(2+E)*Bd,C,HW] fp32 device NCHW in batch-row order uncond | concept 0 .. E-1 | cond; the
 * op stages it to the form the network writes, fp32 NHWC with row stride ld >= C, and the kernels read that. guidance, or
 * guidance_per_sample [Bd] (device) when not NULL; concepts_host [E]; iteration: the i that warm / cool are held against;
 * nu [Bd,C,HW] in / out. Outputs: eps_out [Bd,C,HW]; tau_out [Bd,E], kept_out [Bd,E] (0 for an inactive concept); mask_out
 * [Bd,E,C,HW] or NULL. Refused as cd_sega refuses the concept rows and the momentum, and ld < C. */
int cd_op_sega_guidance(cd_handle h, const float* eps_all, int Bd, int C, int HW, int E, int ld, float guidance,
                        const float* guidance_per_sample, const cd_sega_concept* concepts_host, int iteration,
                        float momentum_scale, float momentum_beta, float* nu, float* eps_out, float* tau_out,
                        int32_t* kept_out, float* mask_out);
/* ---- bare single-kernel entry points of the small HBM-bound kernels (csrc/elementwise.hip), test-only ----
 * Every pointer is device memory that the caller laid out itself; a 16-bit tensor is the storage words of cd_act_format().
 * Each call checks its arguments, makes exactly one launch and synchronises: no staging kernel of the engine's sits between
 * the caller's bytes and the kernel, or between the kernel and the bytes read back. */
/* to_nchw = 0: x fp32 NCHW [B,C,HW] -> y 16-bit [B*HW][ld] (ld = Cpad >= C, columns C.. zero), y = x * scale + shift; dup:
 * the same rows again behind the first B*HW*ld words. to_nchw = 1: x [B*HW][ld] 16-bit (src_f32 = 0) or fp32 (src_f32 = 1)
 * -> y fp32 NCHW [B,C,HW] = x * scale + shift */
int cd_op_layout(cd_handle h, int to_nchw, const void* x, void* y, int B, int C, int HW, int ld, int src_f32, float scale,
                 float shift, int dup);
/* op 0: 2 x 2 average pool [B,H,W,C] -> [B,H/2,W/2,C]; op 1: nearest x2 upsample -> [B,2H,2W,C]; 16-bit NHWC, C % 8 == 0 */
int cd_op_resample16(cd_handle h, int op, const void* x, void* y, int B, int H, int W, int C);
/* rows x cols 16-bit words from row stride lds to row stride ldd (cols, lds, ldd multiples of 8) */
int cd_op_copy_rows16(cd_handle h, const void* src, int lds, void* dst, int ldd, int64_t rows, int cols);
/* y[b][n] = act_out(sum_k act_in(x[b][k]) W[n][k] + bias[n]), fp32, act = SiLU where the flag is set; bias may be NULL */
int cd_op_vec_linear(cd_handle h, const float* x, int ldx, const float* W, const float* bias, float* y, int ldy, int B, int K,
                     int N, int silu_in, int silu_out);
/* op 0: out[b][l] = tok[clamp(ids[b][l], 0, vocab - 1)] + pos[l] (tok [vocab][D], pos [L][D] fp32, out 16-bit [B][L][D]);
 * op 1: out [B][L + 1][D] = [tok (the class row [D]) ; x16 (patches, 16-bit [B][L][D])] + pos [L + 1][D];
 * op 2: out [B][D] = x16[b][first argmax_l ids[b][l]] (x16 16-bit [B][L][D]). D % 8 == 0 for op 0 and 1. */
int cd_op_tokens(cd_handle h, int op, const int* ids, const void* x16, const float* tok, const float* pos, void* out, int B,
                 int L, int D, int vocab);
/* mom fp32 [B*HW][ld] = mean(zc) | logvar(zc) | ...; z fp32 NCHW [B,zc,HW] = scale * (mean + exp(0.5 clamp(logvar, -30, 20))
 * * noise) or scale * mean with use_mean; noise fp32 [B,zc,HW], NULL = the generator's draws for `seed` */
int cd_op_posterior_sample(cd_handle h, const float* mom, int ld, const float* noise, uint64_t seed, float* z, int B, int zc,
                           int HW, float scale, int use_mean);
/* z fp32 NCHW [B,zc,HW], codebook fp32 [n_embed][zc] -> out16 [B*HW][Cpad]: the nearest code (first minimum) of z * in_mul in
 * columns < zc, zero words behind; zc <= 8 and a codebook of at most 150 KB */
int cd_op_vq_quantize(cd_handle h, const float* z, float in_mul, const float* codebook, int n_embed, int zc, int B, int HW,
                      void* out16, int Cpad);
/* the implicit-GEMM kernel as a batched plain GEMM on the caller's device bytes (one launch, no staging):
 * out[z][m][n] = act(alpha * sum_k a[z][m][k] w[z][n][k] + bias[n]) + resid[z][m][n], z < nbatch. a 16-bit [M][lda] at
 * a + z * a_bs, w 16-bit [N][ldw] at w + z * w_bs (element strides; 0 = shared), K % 32 == 0; out 16-bit or fp32 (out_f32)
 * [M][out_ld] at out + z * o_bs; resid 16-bit [M][resid_ld] at resid + z * o_bs, or NULL; stats fp32 [nbatch][ceil(M/32)][2][N]
 * (sums and sums of squares of the final values over 32-row blocks) or NULL; bias fp32 [N] or NULL; act as cd_op_conv2d;
 * tile = id | split << 8 | bk32 << 16, 0 = the launcher's choice (read back with cd_op_last_gemm_config) */
int cd_op_gemm_batched(cd_handle h, const void* a, int lda, int64_t a_bs, const void* w, int ldw, int64_t w_bs, int M, int N,
                       int K, int nbatch, float alpha, const float* bias, const void* resid, int resid_ld, float* stats, int act,
                       int tile, void* out, int out_ld, int64_t o_bs, int out_f32);
/* the single-head AttnBlock (Ho-DDPM U-Net, first stages) between its q | k projection and proj_out, on the caller's device
 * bytes: qk 16-bit [B*T][ldqk] = q (C) | k (C), n 16-bit [B*T][ldn] the normalised rows, packed_v the [C][C] value weight from
 * cd_op_pack_conv_weight, v_bias fp32 [C] -> o 16-bit [B*T][ldo] = softmax(C^-1/2 q k^T) (Wv n) + v_bias; vt_out (or NULL)
 * 16-bit [B][C][round_up(T, 64)] = V^T, zero behind column T; *branch = 0: the flash kernel (C <= 160), 1: scores materialised
 * per image (T % 32 == 0) */
int cd_op_attn_block_core(cd_handle h, const void* qk, int ldqk, const void* n, int ldn, const void* packed_v,
                          const float* v_bias, int B, int T, int C, void* o, int ldo, void* vt_out, int* branch);
/* ---- the kernels and launch forms of the FID Inception-v3 (csrc/inception.hip), one at a time, test-only ----
 * Every 16-bit buffer a kernel reads past or writes into starts as 0xFF bytes (NaN in fp16 and bf16) and has one more 64-row
 * block of them behind its last row. */
/* the 3 x 3 pool (max != 0: maximum, else the mean over the in-image taps) as the network launches it: x fp32 NCHW [B,C,H,W],
 * stored NHWC with row stride C + in_pad (pad columns NaN); the output rows [B*Ho*Wo] (Ho = (H + 2 pad - 3) / stride + 1) go
 * to columns [out_off, out_off + C) of a buffer of row stride out_ld. y: the whole buffer, guard rows included, as fp32
 * [B*Ho*Wo + 64][out_ld]. Refused: C % 8, in_pad % 8, out_off % 8, out_ld % 8, out_off + C > out_ld. */
int cd_op_pool3x3(cd_handle h, const float* x, int B, int C, int H, int W, int in_pad, int max, int stride, int pad,
                  int out_off, int out_ld, float* y);
/* the global average pool behind Mixed_7c: x fp32 NCHW [B,C,HW], stored with row stride C + in_pad (pad columns NaN) -> y fp32
 * [B][C]. Refused: C % 8, in_pad % 8. */
int cd_op_global_avg(cd_handle h, const float* x, int B, int HW, int C, int in_pad, float* y);
/* one BasicConv2d (conv without bias, BatchNorm eps 1e-3, ReLU) as the network runs it: the raw fp32 weight w [N][Cin][KH][KW]
 * and the BatchNorm vectors [N] (all fp32 device) are folded by the network's own fold kernel into a packed weight allocated as
 * the network allocates it; x fp32 NCHW [B,Cin,H,W] is stored NHWC with row stride in_ld (>= Cpad = round_up(Cin, 32); channels
 * [Cin, Cpad) zero, [Cpad, in_ld) NaN); the implicit GEMM, filled in by the network's own function with N rounded up to 32, writes
 * columns [out_off, out_off + round_up(N, 32)) of a buffer of row stride out_ld. tile as cd_op_gemm_batched (read back with
 * cd_op_last_gemm_config). y: the whole output buffer, guard rows included, fp32 [B*Ho*Wo + 64][out_ld]; w_packed (or NULL): the
 * packed 16-bit weights as fp32 [round_up(N, 128)][KH][KW][Cpad]; bias_out (or NULL): fp32 [round_up(N, 128)].
 * Refused: in_ld % 8, in_ld < Cpad, out_off % 8, out_ld % 8, out_off + round_up(N, 32) > out_ld. */
int cd_op_basic_conv(cd_handle h, const float* x, int B, int Cin, int H, int W, int in_ld, const float* w, const float* gamma,
                     const float* beta, const float* mean, const float* var, int N, int KH, int KW, int stride, int pad_t,
                     int pad_l, int out_off, int out_ld, int tile, float* y, float* w_packed, float* bias_out);
/* ---- the kernels of LPIPS (csrc/lpips.hip), one at a time, test-only; NaN / 0xFF guards as above ----
 * one tap's distance: f0, f1 fp32 [B][HW][C] (pixel rows), stored 16-bit with row stride C + in_pad (pad columns NaN, a 64-row
 * block of 0xFF behind the last row), w fp32 [C] -> out [B] = mean over pixels of sum_c w_c (f0_c / (|f0| + 1e-10) - f1_c /
 * (|f1| + 1e-10))^2. Refused: C % 8, C > 512, (C + in_pad) % 8. */
int cd_op_lpips_layer(cd_handle h, const float* f0, const float* f1, const float* w, int B, int HW, int C, int in_pad,
                      float* out);
/* the 2 x 2 stride-2 max pool of VGG16 (floor of odd sizes), operands and result laid out as cd_op_pool3x3's: y = the whole
 * buffer fp32 [B*(H/2)*(W/2) + 64][out_ld]. Refused: C % 8, in_pad % 8, out_off % 8, out_ld % 8, out_off + C > out_ld, H or W < 2. */
int cd_op_pool2x2(cd_handle h, const float* x, int B, int C, int H, int W, int in_pad, int out_off, int out_ld, float* y);
/* micro-benchmark of one conv / GEMM shape on synthetic data (scripts/bench_gemm.py): average ms per launch.
 * act: low byte = activation; | 0x100 = in-place residual update of the output; | 0x200 = fused GroupNorm statistics */
int cd_op_bench_conv(cd_handle h, int B, int H, int W, int C0, int C1, int N, int k, int stride, int up,
                     int act, int tile, int iters, float* ms_out);
/* what the matrix cores of this device sustain on 16-bit operands under its power cap: a bare MFMA loop on every CU for
 * about target_ms (no reference counterpart: measurement support for bench.py's roofline object) */
int cd_op_bench_mfma_sustained(cd_handle h, int target_ms, float* tflops_out, float* ghz_out);
/* raw MFMA / LDS layout probe used by tests/test_gpu_ops.py */
int cd_op_probe(cd_handle h, int which, const void* in, void* out, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CYCLEDIFF_H */
