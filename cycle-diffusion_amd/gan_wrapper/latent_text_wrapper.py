"""Text-conditioned latent wrappers on the HIP engine: drop-ins for
  SDStochasticTextWrapper          model/gan_wrapper/stable_diffusion_stochastic_text_wrapper.py:102-253
  LatentDiffStochasticTextWrapper  model/gan_wrapper/latentdiff_stochastic_text_wrapper.py
Same constructor kwargs (the [gan] section of config/experiments/*.cfg), same
encode(image, encode_text) -> z_ensemble and forward(z_ensemble, original_img, encode_text,
decode_text) -> img contracts, same ensemble ordering (trial -> encoder scale -> skip_steps, then
decoder scales) and z layout torch.stack(z_list, dim=1).view(bsz, -1).

Conditioning enters through `cond_stage` (a callable list[str] -> [B, 77, context_dim]). With a real checkpoint
the text encoder stored in it is used, as in the reference: CLIP ViT-L/14 text (SD) or the BERT-tokenizer
x-transformer (LDM), both on the engine (text_encoders.py), and a missing tokenizer vocabulary is an error.
`[gan] text_encoder = clip | bert` forces one. Only in synthetic-weight runs (CYCLEDIFF_SYNTHETIC_WEIGHTS=1, no
checkpoint) a deterministic stand-in embedding is used, and SAYS SO in its name. `[gan] ranker = directional_clip`
is the reference's DirectionalCLIP on the engine (ranker.py); its ViT-B/32 weights come from `ranker_path` /
CYCLEDIFF_CLIP_RANKER (the `clip.load("ViT-B/32")` state_dict saved with torch.save).

Ensemble members that share (guidance scale, skip) differ only in their noise: they are folded into the batch
dimension of ONE engine call - same draws, same member order, larger GEMMs.
"""
import hashlib
import os

import numpy as np

import torch

from .. import _ffi, attn_control, schedule
from .. import semantic_guidance as sgm
from .. import auto_mask as am
from .. import windows as wnd
from ..engine import kl_f8_vae_desc, ldm_text_unet_desc, sd_v1_unet_desc
from ..runtime import get_engine, load_or_init_weights, read_checkpoint, synthetic_allowed


class StandInTextEmbedder:
    """Deterministic N(0,1) embedding per string — NOT a text encoder; keeps tensor shapes and the
    call pattern of get_learned_conditioning (ddpm.py:545-556) when no CLIP/BERT weights exist."""

    def __init__(self, context_dim, length=77):
        self.context_dim, self.length = context_dim, length

    def __call__(self, texts):
        out = []
        for t in texts:
            seed = int.from_bytes(hashlib.sha256(t.encode("utf-8")).digest()[:8], "little") % (2 ** 63)
            g = torch.Generator().manual_seed(seed)
            out.append(torch.randn(self.length, self.context_dim, generator=g))
        return torch.stack(out, 0)


class LatentMask:
    """A keep-mask that is latent already, [B, 1, h, w] in [0, 1]: `mask=LatentMask(m)` passes it to forward() / translate()
    without the block mean a pixel-space mask goes through."""

    def __init__(self, m):
        self.m = torch.as_tensor(m)


AUTO_MASK = object()  # in the place of a mask inside the wrappers: estimate it from the two prompts (`[gan] auto_mask`)

TEXT_PRECISIONS = {"fp16": _ffi.CD_PREC_16, "16": _ffi.CD_PREC_16, "fp32": _ffi.CD_PREC_F32, "fp32x3": _ffi.CD_PREC_F32X3}


class _LatentStochasticTextWrapper(torch.nn.Module):
    # subclass constants
    UNET_DESC = None
    RESOLUTION = None
    SAMPLE_POSTERIOR = True
    LINEAR_START, LINEAR_END = 0.00085, 0.0120
    SCALE_FACTOR = 0.18215
    VAE_DESC = staticmethod(kl_f8_vae_desc)
    MAX_FOLD = 32  # samples per engine call when ensemble members are folded into the batch
    # first-stage calls are cut at this many pixels (32 images of 512 x 512): the KL-f8 decoder's 512 x 512 x 128-channel
    # level is 64 MiB per image and tensor in 16 bits (256 MiB in fp32), several of them live at once - a look-ahead fold of
    # 64 images through ONE decode would need ~25 GB of workspace for 1.5 % of the path's FLOPs
    VAE_MAX_PIXELS = 32 * 512 * 512
    COUPLE_MAX_TOKENS = 96 * 64 * 64  # rows x latent tokens of one coupled forward (translate())

    def __init__(self, source_model_type, custom_steps, eta, white_box_steps, skip_steps,
                 encoder_unconditional_guidance_scales=None, decoder_unconditional_guidance_scales=None,
                 n_trials=None, cond_stage=None, ranker=None, device=None, text_encoder=None,
                 noise_on_cpu=False, fold_ensemble=True, ranker_path=None, precision="fp16", couple=True,
                 mask_source="q_sample", cac_steps=0.0, cac_mode="refine", auto_mask=None, auto_mask_draws=10,
                 auto_mask_strength=0.5, auto_mask_ratio=3.0, auto_mask_threshold=0.5, auto_mask_dilate=0, auto_mask_seed=0,
                 local_blend=None, local_blend_threshold=0.3, local_blend_pool=3, local_blend_side=0, local_blend_start=0.2,
                 edit_concepts="", edit_momentum_scale=0.3, edit_momentum_beta=0.6, window_stride=0):
        super().__init__()
        # `[gan] window_stride` (latent cells; 0 = off, the default): fused windows (MultiDiffusion) - translate()
        # takes images larger than the network, [B, 3, H, W] with H and W multiples of the first-stage factor and a latent of
        # at least image_size x image_size; the coupled loop runs the network on the windows window_grid() lays over the latent
        self.window_stride = int(window_stride)
        if self.window_stride < 0:
            raise ValueError("window_stride must be a number of latent cells (0: off), got %r" % (window_stride,))
        if self.window_stride and str(precision) in ("fp32", "fp32x3"):
            raise ValueError("window_stride needs the 16-bit precision: the fused windows are not built for the fp32 / fp32x3 "
                             "networks")
        # `[gan] edit_concepts = "+glasses:5:0.9; -smile"` (default: none): semantic guidance on the coupled loop -
        # each item `[+|-]text[:scale[:threshold]]` is an edit concept that steers every sample of a translate() call towards
        # (+) or away from (-) its text beside the target prompt; `edit_momentum_scale` / `edit_momentum_beta`: the momentum
        self.edit_concepts = sgm.parse_concepts(edit_concepts)
        self.edit_momentum_scale, self.edit_momentum_beta = float(edit_momentum_scale), float(edit_momentum_beta)
        if self.edit_concepts:
            sgm.check_concepts(self.edit_concepts, self.edit_momentum_scale, self.edit_momentum_beta)
            if str(precision) in ("fp32", "fp32x3"):
                raise ValueError("edit_concepts needs the 16-bit precision: semantic guidance is not built for the fp32 / fp32x3 "
                                 "networks")
        self.last_edit_masks, self.last_edit_taus = None, None
        # `[gan] local_blend = words` (default none): prompt-to-prompt's local blend on the coupled loop - the
        # decoder's latent is held to the encoder's outside the region the word maps of the edited words mark, the mask rebuilt
        # after every step from iteration int(local_blend_start * K) on. `local_blend_side`: the token grid whose blocks are
        # collected (0: image_size / 4), `local_blend_pool` / `local_blend_threshold`: the LocalBlend rule
        self.local_blend = "none" if local_blend is None else str(local_blend)
        if self.local_blend not in attn_control.LOCAL_BLEND_MODES:
            raise ValueError("local_blend must be one of %s" % (attn_control.LOCAL_BLEND_MODES,))
        self.local_blend_threshold, self.local_blend_pool = float(local_blend_threshold), int(local_blend_pool)
        self.local_blend_side, self.local_blend_start = int(local_blend_side), float(local_blend_start)
        if not np.isfinite(self.local_blend_threshold):
            raise ValueError("local_blend_threshold must be finite, got %r" % (local_blend_threshold,))
        if self.local_blend_pool % 2 != 1 or not 1 <= self.local_blend_pool <= 7:
            raise ValueError("local_blend_pool must be an odd number in [1, 7], got %r" % (local_blend_pool,))
        if self.local_blend_side < 0:
            raise ValueError("local_blend_side must be a token grid side (0: image_size / 4), got %r" % (local_blend_side,))
        attn_control.local_blend_start(self.local_blend_start, 1)
        if self.local_blend != "none" and str(precision) in ("fp32", "fp32x3"):
            raise ValueError("local_blend needs the 16-bit precision: the word maps are not built for the fp32 / fp32x3 "
                             "networks' transformer blocks")
        self.last_local_blend_mask, self.last_local_blend_masks = None, None
        # `[gan] auto_mask = diffedit` (default none): translate() / forward() without a `mask=` estimate the keep-mask from the
        # two prompts (the keys: auto_mask.py) and take the masked path with it; an explicit `mask=` wins
        self.auto_mask_opts = am.AutoMaskOptions(auto_mask, auto_mask_draws, auto_mask_strength, auto_mask_ratio,
                                                 auto_mask_threshold, auto_mask_dilate, auto_mask_seed)
        self.last_auto_mask = self.last_auto_map = None
        # `[gan] cac_steps` (0 = off, the default): cross-attention control (prompt-to-prompt on the coupled loop)
        # on the first int(cac_steps * K) of the K decode steps a member runs; `cac_mode = refine | replace`: how the target
        # prompt's tokens are matched to the source's (attn_control.build_control)
        self.cac_steps = float(cac_steps)
        if not 0.0 <= self.cac_steps <= 1.0:
            raise ValueError("cac_steps must lie in [0, 1] (the controlled fraction of the decode steps), got %r" % (cac_steps,))
        if str(cac_mode) not in attn_control.MODES:
            raise ValueError("cac_mode must be one of %s" % (attn_control.MODES,))
        self.cac_mode = str(cac_mode)
        # `[gan] mask_source`: what a keep-mask (forward / translate `mask=`) holds its region to - 'q_sample': a freshly noised
        # copy of the source latent per step, the reference's sample_with_eps(mask=, x0=) (ddim.py:427-430); 'encoder': the
        # DPM-Encoder's own x_t of every level (coupled loop only, no extra noise)
        if str(mask_source) not in _ffi.MASK_SOURCES:
            raise ValueError("mask_source must be one of %s" % sorted(_ffi.MASK_SOURCES))
        self.mask_source = str(mask_source)
        # `[gan] precision`: arithmetic of the U-Net AND (round 5) of the first stage - the reference's `precision = "full"` covers
        # both (sd_wrapper:117, autoencoder.py:324-333); the text towers stay 16-bit (their output is the conditioning, rounded
        # once). 'fp16' (default):
        # 16-bit storage, the benchmarked engine (55 dB against the reference on C2, 99-step self-cycle 2e-2 rms); 'fp32': the
        # reference's own arithmetic (`precision = "full"`, stable_diffusion_stochastic_text_wrapper.py:117) - fp32 storage,
        # fp32 matrix instructions, fp32 flash attention; 'fp32x3': the same network with every GroupNorm- / LayerNorm-fed
        # convolution and projection as three-term split-fp16 products (include/cyclediff.h CD_PREC_F32X3)
        if str(precision) not in TEXT_PRECISIONS:
            raise ValueError("precision must be one of %s" % sorted(TEXT_PRECISIONS))
        self.precision = str(precision)
        if self.precision == "fp32x3" and _ffi.load_library().cd_act_format() != 1:
            raise ValueError("precision='fp32x3' needs the fp16 build of the library (this is the bf16 build): use 'fp32'")
        self.encoder_unconditional_guidance_scales = encoder_unconditional_guidance_scales
        self.decoder_unconditional_guidance_scales = decoder_unconditional_guidance_scales
        self.n_trials = n_trials
        self.eta, self.custom_steps = eta, custom_steps
        self.white_box_steps, self.skip_steps = white_box_steps, skip_steps
        self.resolution = self.RESOLUTION
        # parity runs draw every noise tensor on the CPU in the reference's order; throughput
        # runs draw on the device
        self.noise_on_cpu, self.fold_ensemble = bool(noise_on_cpu), bool(fold_ensemble)
        # `[gan] couple = False`: translate() runs encode() then forward() as two loops (the reference's own order of work).
        # The coupled loop is taken while its forward - [encoder rows | decoder rows] x latent tokens - stays below
        # COUPLE_MAX_TOKENS: measured on MI355X (profiles/r6_coupled_loop_ab.json) it is +28 % at a batch of 4 (12 rows of
        # 64 x 64 tokens per forward instead of 4, then 8), +7 % on config 3 (192 rows of 32 x 32) and -1.4 % at 64 images of
        # 512 x 512 (192 rows of 64 x 64: a 503 MB activation per 320-channel tensor no longer stays in the 256 MB Infinity
        # Cache between producer and consumer, where the two loops run 64 and 128 rows)
        self.couple = bool(couple) and os.environ.get("CYCLEDIFF_COUPLE", "1") != "0"
        self.couple_max_tokens = int(os.environ.get("CYCLEDIFF_COUPLE_MAX_TOKENS", self.COUPLE_MAX_TOKENS))
        self.last_translate_coupled = None
        self.noise_source = None
        self.engine = get_engine(device)
        udesc = self.UNET_DESC()
        udesc.precision = TEXT_PRECISIONS[self.precision]
        self.channels, self.image_size = udesc.in_channels, udesc.image_size
        self.unet = self.engine.create_net(udesc)
        vdesc = self.VAE_DESC()
        vdesc.precision = TEXT_PRECISIONS[self.precision]
        self.vae = self.engine.create_net(vdesc)
        self.vae_factor = 2 ** (vdesc.n_mult - 1)
        ckpt = self.checkpoint_path(source_model_type)
        ckpt_sd = read_checkpoint(ckpt)
        self.weights_origin = load_or_init_weights(self.engine, ckpt, {
            self.unet: "model.diffusion_model.", self.vae: "first_stage_model."}, state_dict=ckpt_sd)
        if cond_stage is None and text_encoder is None and ckpt_sd is not None:
            # a real checkpoint carries its text encoder (cond_stage_model.*): use it, as the reference does
            text_encoder = "clip" if udesc.context_dim == 768 else "bert"
        strict_tok = ckpt_sd is not None or not synthetic_allowed()
        if cond_stage is None and text_encoder == "clip":
            # `[gan] text_encoder = clip`: FrozenCLIPEmbedder on the engine (768-wide contexts: the SD U-Net)
            from .text_encoders import FrozenCLIPEmbedderHIP
            assert udesc.context_dim == 768, "the CLIP ViT-L/14 text encoder conditions the SD-v1 U-Net"
            cond_stage = FrozenCLIPEmbedderHIP(self.engine, state_dict=ckpt_sd,  # cond_stage_model.transformer.*
                                               require_vocab=strict_tok)
        elif cond_stage is None and text_encoder == "bert":
            # `[gan] text_encoder = bert`: BERTEmbedder of LDM text2img-large (1280-wide contexts)
            from .text_encoders import BERTEmbedderHIP
            assert udesc.context_dim == 1280, "the BERT / x-transformer encoder conditions the LDM text2img U-Net"
            cond_stage = BERTEmbedderHIP(self.engine, state_dict=ckpt_sd, require_vocab=strict_tok)
        if cond_stage is None:
            if not synthetic_allowed():
                raise RuntimeError("no text encoder: pass cond_stage / text_encoder, or load a checkpoint that has one")
            cond_stage = StandInTextEmbedder(udesc.context_dim)
        self.cond_stage = cond_stage
        n_candidates = self._ensemble_size()
        if ranker is None and n_candidates > 1:
            # the reference builds its DirectionalCLIP unconditionally (sd_wrapper:140) and uses it when there is more
            # than one candidate (:213-235): an ensemble config needs no extra key here either
            ranker = "directional_clip"
        if ranker == "directional_clip":  # `[gan] ranker = directional_clip`: the reference's DirectionalCLIP on the engine
            from .ranker import DirectionalCLIPHIP
            rpath = ranker_path or os.environ.get("CYCLEDIFF_CLIP_RANKER")
            rsd = None
            if rpath:
                rsd = torch.load(rpath, map_location="cpu")
                rsd = rsd.get("state_dict", rsd) if isinstance(rsd, dict) else rsd.state_dict()
            elif not synthetic_allowed():
                raise FileNotFoundError("ranker = directional_clip needs the CLIP ViT-B/32 state_dict: set `ranker_path` "
                                        "or CYCLEDIFF_CLIP_RANKER (or CYCLEDIFF_SYNTHETIC_WEIGHTS=1 for random towers)")
            ranker = DirectionalCLIPHIP(self.engine, state_dict=rsd, require_vocab=rsd is not None)
        self.ranker = ranker
        self.alphas_cumprod = schedule.latent_alphas_cumprod(1000, self.LINEAR_START, self.LINEAR_END)
        # `next(self.parameters()).device` must work (sd_wrapper:251-253) and DDP must be able to wrap us
        self._anchor = torch.nn.Parameter(torch.zeros(1, device=self.engine.device), requires_grad=True)

    # ---- conditioning (sd_wrapper:28-36)
    def get_condition(self, text, bs):
        assert isinstance(text, list) and isinstance(text[0], str)
        uc = self.cond_stage(bs * [""]).to(self.device, torch.float32)
        c = self.cond_stage(text).to(self.device, torch.float32)
        return c, uc

    def _schedule(self):
        return schedule.DDIMSchedule(self.alphas_cumprod, self.custom_steps, self.eta)

    def _vae_batch(self, pixels=None):
        """images per first-stage call (fp32 / split-mode activations are twice the bytes of the 16-bit ones); `pixels`: of
        one image, when it is not the wrapper's square resolution"""
        px = self.VAE_MAX_PIXELS if getattr(self, "precision", "fp16") == "fp16" else self.VAE_MAX_PIXELS // 2
        res = getattr(self, "resolution", None) or self.RESOLUTION or 512
        return max(1, px // (pixels or res * res))

    def _randn(self, shape, cpu=None):
        """One noise draw. `noise_source` (a callable shape -> CPU tensor; parity tests) replaces the generator: it lets
        a test hand every sample of a batch its own stream, e.g. the stream a fixture was made with."""
        if self.noise_source is not None:
            return self.noise_source(tuple(shape)).to(self.device, torch.float32)
        if self.noise_on_cpu if cpu is None else cpu:
            return torch.randn(shape).to(self.device)
        return torch.randn(shape, device=self.device)

    @staticmethod
    def _chunks(idx, per_call):
        """split a group into the fewest engine calls of at most `per_call` members, as evenly as possible (75 members
        at 32 per call -> 25 + 25 + 25 rather than 32 + 32 + 11: no small tail call, one batch shape per group)"""
        n_calls = -(-len(idx) // per_call)
        size = -(-len(idx) // n_calls)
        return [idx[i:i + size] for i in range(0, len(idx), size)]

    def _groups(self, keys):
        """indices of ensemble members grouped by key, in first-appearance order; singletons when folding is off"""
        if not self.fold_ensemble:
            return [[i] for i in range(len(keys))]
        order, groups = [], {}
        for i, k in enumerate(keys):
            if k not in groups:
                groups[k] = []
                order.append(k)
            groups[k].append(i)
        return [groups[k] for k in order]

    def _ensemble_size(self):
        """candidates per sample: trial x encoder scale x skip x decoder scale (sd_wrapper:155-166, 186-204)"""
        return (self.n_trials or 1) * len(self.skip_steps or [0]) * len(self.encoder_unconditional_guidance_scales or [1]) * \
            len(self.decoder_unconditional_guidance_scales or [1])

    # ---- encode (sd_wrapper:169-206)
    def _first_stage(self, image):
        """z0 = scale * E(2 * image - 1), the posterior sampled (its noise drawn first, on the CPU) or its mean"""
        image = (image - 0.5) * 2.0
        if not getattr(self, "window_stride", 0):
            assert image.shape[2] == image.shape[3] == self.resolution
        image = image.to(self.device, torch.float32)
        bsz = image.shape[0]
        noise = None
        if self.SAMPLE_POSTERIOR:
            # DiagonalGaussianDistribution.sample draws on the CPU and moves (distributions.py:36)
            h, w = image.shape[2] // self.vae_factor, image.shape[3] // self.vae_factor
            noise = self._randn((bsz, self.channels, h, w), cpu=True)
        per = self._vae_batch(image.shape[2] * image.shape[3])
        x0 = torch.cat([self.engine.vae_encode(self.vae, image[i:i + per], noise=None if noise is None else noise[i:i + per],
                                               sample=self.SAMPLE_POSTERIOR, scale=self.SCALE_FACTOR)
                        for i in range(0, bsz, per)], 0)
        return x0

    def _encode_front(self, image, encode_text):
        """first stage, conditioning and the members' noise in the reference's draw order -> (x0, c, uc, members)"""
        x0 = self._first_stage(image)
        bsz = x0.shape[0]
        sch = self._schedule()
        assert self.eta > 0
        c, uc = self.get_condition(encode_text, bsz)
        # members in the reference's order: trial -> encoder scale -> skip; noise drawn member by member in the
        # draw order of _ddpm_ddim_encoding: randn_like(x0) then K-1 x randn(shape) (ddim.py:479,599)
        members = []
        for _trial in range(self.n_trials):
            for enc_scale in self.encoder_unconditional_guidance_scales:
                for skip in self.skip_steps:
                    K = len(sch) - skip
                    # the DPM-Encoder loop breaks after white_box_steps - skip - 1 steps (ddim.py:486): the reference's
                    # configs set white_box_steps = custom_steps (the whole chain, n_loop = K); a shorter prefix leaves the
                    # rest of the decode to fresh noise (`eps=None`, ddim.py:437), -1 keeps x_T only
                    n_loop = self._white_box_loop(K, skip)
                    n_draw = K if n_loop == K else n_loop + 1  # x_T + one per executed step; index 0 draws nothing
                    if self.noise_on_cpu or self.noise_source is not None:
                        nz = torch.stack([self._randn(tuple(x0.shape)) for _ in range(n_draw)], 0)
                    else:
                        nz = self._randn((n_draw,) + tuple(x0.shape))
                    members.append((float(enc_scale), int(skip), nz))
        return x0, c, uc, members

    def encode(self, image, encode_text):
        if getattr(self, "window_stride", 0):
            raise ValueError("window_stride needs translate(): the fused windows run on the coupled loop, which encode() + "
                             "forward() do not take; use translate(image, encode_text, decode_text)")
        x0, c, uc, members = self._encode_front(image, encode_text)
        return self._encode_members(x0, c, uc, members)

    def _encode_members(self, x0, c, uc, members):
        bsz, sch = x0.shape[0], self._schedule()
        z_ensemble = [None] * len(members)
        per_call = max(1, self.MAX_FOLD // bsz)
        for grp in self._groups([(m[0], m[1]) for m in members]):
            enc_scale, skip = members[grp[0]][0], members[grp[0]][1]
            for idx in self._chunks(grp, per_call):
                n = len(idx)
                coef, K = sch.coef_encode(skip), len(sch) - skip
                n_loop = self._white_box_loop(K, skip)
                if n_loop < K:  # the first n_loop steps of the chain: table rows K-n_loop .. K-1 + the x_T row
                    coef = np.concatenate([coef[K - n_loop:K], coef[K:K + 1]])
                z = self.engine.dpm_encode(self.unet, _ffi.CD_SCHED_DDIM, x0.repeat(n, 1, 1, 1), coef,
                                           ctx_c=c.repeat(n, 1, 1), ctx_uc=uc.repeat(n, 1, 1), guidance=enc_scale,
                                           noise=torch.cat([members[i][2] for i in idx], dim=1), last_uses_x0=n_loop == K)
                for j, i in enumerate(idx):
                    z_ensemble[i] = z[j * bsz:(j + 1) * bsz].reshape(bsz, -1)
        return z_ensemble

    def _white_box_loop(self, K, skip):
        """DPM-Encoder steps that run for a chain of K steps (ddim.py:486 `if i < white_box_steps - skip_steps - 1`)."""
        if self.white_box_steps == -1:
            return 0
        return max(0, min(K, self.white_box_steps - skip - 1))

    # ---- generate (sd_wrapper:142-167)
    # ---- keep-mask (sample_with_eps(mask=, x0=), ddim.py:427-430)
    def _latent_mask(self, mask, bsz):
        """pixel-space [B, 1, R, R] in [0, 1] (1 = keep the source) -> latent [B, 1, R/f, R/f]: the f x f block mean, f the
        first stage's down-sampling factor; not thresholded - the blend is linear in m, a feathered mask stays feathered.
        A LatentMask is latent already and passes as it is."""
        if isinstance(mask, LatentMask):
            if tuple(mask.m.shape) != (bsz, 1, self.image_size, self.image_size):
                raise ValueError("latent mask must be [%d, 1, %d, %d], got %s" % (bsz, self.image_size, self.image_size,
                                                                                  tuple(mask.m.shape)))
            return mask.m.to(self.device, torch.float32).contiguous()
        mask = torch.as_tensor(mask).to(self.device, torch.float32)
        if mask.dim() != 4 or tuple(mask.shape) != (bsz, 1, self.resolution, self.resolution):
            raise ValueError("mask must be [%d, 1, %d, %d], got %s" % (bsz, self.resolution, self.resolution, tuple(mask.shape)))
        if bool((mask < 0).any()) or bool((mask > 1).any()):
            raise ValueError("mask values must lie in [0, 1] (1 = keep the source)")
        return torch.nn.functional.avg_pool2d(mask, self.vae_factor).contiguous()

    # ---- keep-mask estimated from the two prompts
    def _auto_mask_on(self):
        o = getattr(self, "auto_mask_opts", None)
        return o is not None and o.on

    def auto_mask_level(self):
        """(t, qa, qb) of the estimate's level: row k = am.level_index(strength, S) of this wrapper's own schedule"""
        sch = self._schedule()
        k = am.level_index(self.auto_mask_opts.strength, len(sch))
        qa, qb = sch.coef_qsample(0)[k]
        return int(sch.coef_decode(0)["t"][k]), float(qa), float(qb)

    def auto_mask(self, x0, encode_text, decode_text):
        """keep [B, 1, h, w] (exact 0 / 1, 1 = keep the source) and map [B, 1, h, w] of the latent x0 [B, C, h, w] under the
        two prompts, by the `auto_mask_*` keys whatever `auto_mask` itself says. The draws come from the counter-based
        generator (auto_mask_seed), never from torch's: nothing else draws differently for it."""
        bsz = x0.shape[0]
        c_src, _ = self.get_condition(encode_text, bsz)
        c_tgt, _ = self.get_condition(decode_text, bsz)
        return self._auto_mask_ctx(x0, c_src, c_tgt)

    def _auto_mask_ctx(self, x0, c_src, c_tgt):
        o = self.auto_mask_opts
        t, qa, qb = self.auto_mask_level()
        # rows of one forward as the other calls bound them: MAX_FOLD samples of a guided call, COUPLE_MAX_TOKENS tokens
        max_rows = max(2, min(2 * self.MAX_FOLD, self.couple_max_tokens // self.image_size ** 2))
        per = max(1, max_rows // 2)  # samples per call (a sample's draw index is its place in its call)
        keeps, maps = [], []
        for i in range(0, x0.shape[0], per):
            k, m = self.engine.automask(self.unet, x0[i:i + per].contiguous(), c_src[i:i + per].contiguous(),
                                        c_tgt[i:i + per].contiguous(), t, qa, qb, n_draws=o.draws, seed=o.seed,
                                        max_rows=max_rows, ratio=o.ratio, thr=o.threshold, dilate=o.dilate)
            keeps.append(k)
            maps.append(m)
        self.last_auto_mask, self.last_auto_map = torch.cat(keeps, 0), torch.cat(maps, 0)
        return self.last_auto_mask, self.last_auto_map

    # ---- per-word cross-attention heat maps
    def word_maps(self, x0, text, words=None, other_text=None, strength=0.5, draws=4, seed=0, sides=None):
        """maps [B, N, h, w] of the latent x0 [B, C, h, w] under the prompts `text`: the softmax mass the text cross-attentions
        put on chosen words, averaged over heads, transformer blocks and `draws` noised copies of x0 at the level
        auto_mask.level_index(strength, S) of this wrapper's own schedule. `words`: N strings, each tokenised by the text
        encoder's tokenizer and marked wherever it occurs in a sample's prompt; or `other_text`: the one map (N = 1) of the
        tokens `text` introduces against `other_text` (attn_control.edited_selector). sides = (min, max) keeps the blocks
        whose token grid side lies in that window (None: all). The draws come from the counter-based generator (seed)."""
        if (words is None) == (other_text is None):
            raise ValueError("word_maps takes either words= or other_text=")
        bsz = x0.shape[0]
        c, _ = self.get_condition(text, bsz)
        ids, eos = self._control_ids(text)
        if other_text is not None:
            oids, _ = self._control_ids(other_text)
            sel = [attn_control.edited_selector(oids[b], ids[b], eos) for b in range(bsz)]
        else:
            wids, _ = self._control_ids(list(words))
            toks = [list(r[1:attn_control.prompt_length(r, eos)]) for r in wids]
            sel = [attn_control.word_selector(ids[b], toks, eos) for b in range(bsz)]
        sel = torch.from_numpy(np.stack(sel, 0)).to(self.device)
        sch = self._schedule()
        k = am.level_index(strength, len(sch))
        qa, qb = sch.coef_qsample(0)[k]
        t = int(sch.coef_decode(0)["t"][k])
        # rows of one forward as the other calls bound them: MAX_FOLD samples, COUPLE_MAX_TOKENS tokens
        max_rows = max(1, min(self.MAX_FOLD, self.couple_max_tokens // self.image_size ** 2))
        x0 = x0.to(self.device, torch.float32)
        out = []
        for i in range(0, bsz, max_rows):  # a sample's draw index is its place in its call
            m, _ = self.engine.word_maps(self.unet, x0[i:i + max_rows].contiguous(), c[i:i + max_rows].contiguous(),
                                         sel[i:i + max_rows].contiguous(), t, float(qa), float(qb), n_draws=int(draws),
                                         seed=int(seed), max_rows=max_rows, sides=sides or (0, 0))
            out.append(m)
        return torch.cat(out, 0)

    def _mask_draws(self, K, bsz, n_eps=None):
        """the K q_sample draws of ONE sample_with_eps(mask=) call in its own order (randn_like(x0) at the top of every step,
        ddim.py:429), and - interleaved as the reference draws them - the fresh noise of the steps past the white-box prefix
        (ddim.py:437 `eps=None`) -> (mask_noise [K, bsz, C, h, w], tail or None)"""
        shape = (bsz, self.channels, self.image_size, self.image_size)
        n_eps = K if n_eps is None else n_eps
        if not (self.noise_on_cpu or self.noise_source is not None):
            return self._randn((K,) + shape), (self._randn((K - n_eps,) + shape) if K > n_eps else None)
        mn, tail = [], []
        for i in range(K):
            mn.append(self._randn(shape))
            if i >= n_eps:
                tail.append(self._randn(shape))
        return torch.stack(mn, 0), (torch.stack(tail, 0) if tail else None)

    def generate(self, z_ensemble, decode_text, latents=None, mask=None, x0=None, mask_noise=None):
        """`latents` (translate()): {output slot: latent [bsz, C, h, w]} of candidates the coupled loop already decoded.
        `mask` (LATENT mask [bsz, 1, h, w]) with `x0` [bsz, C, h, w]: the "q_sample" keep-mask decode; every candidate draws
        its own K noise tensors in the order the reference's loop would call sample_with_eps (z member -> decoder scale);
        `mask_noise`: {output slot: [K, bsz, C, h, w]} of draws translate() already made in that order."""
        sch = self._schedule()
        n_dec = len(self.decoder_unconditional_guidance_scales)
        bsz = z_ensemble[0].shape[0]
        c, uc = self.get_condition(decode_text, bsz)
        latents = dict(latents or {})
        jobs = []  # (output slot, skip, decoder scale, z) in the reference's order: z member -> decoder scale
        for i, z in enumerate(z_ensemble):
            skip = self.skip_steps[i % len(self.skip_steps)]
            slots = self.white_box_steps - skip if self.white_box_steps != -1 else 1  # sd_wrapper:149-152
            zz = z.view(bsz, slots, self.channels, self.image_size, self.image_size)
            # decode steps beyond the white-box prefix draw fresh noise (ddim.py:437 `eps=None`): one tensor per step and
            # candidate, drawn here in candidate order so that folding candidates into one call changes nothing
            n_tail = (len(sch) - skip) - (slots - 1)
            for j, dec_scale in enumerate(self.decoder_unconditional_guidance_scales):
                tail = None
                if mask is not None:
                    slot = i * n_dec + j
                    if mask_noise is not None and slot in mask_noise:
                        mn = mask_noise[slot]
                    elif slot in latents:
                        mn = None
                    else:
                        mn, tail = self._mask_draws(len(sch) - skip, bsz, n_eps=slots - 1)
                    jobs.append((slot, int(skip), float(dec_scale), zz, tail, mn))
                    continue
                if n_tail > 0:
                    shape = (bsz, self.channels, self.image_size, self.image_size)
                    if self.noise_on_cpu or self.noise_source is not None:
                        tail = torch.stack([self._randn(shape) for _ in range(n_tail)], 0)
                    else:
                        tail = self._randn((n_tail,) + shape)
                jobs.append((i * n_dec + j, int(skip), float(dec_scale), zz, tail))
        n_jobs = len(jobs)
        per_call = max(1, self.MAX_FOLD // bsz)
        todo = [jb for jb in jobs if jb[0] not in latents]

        # jobs that share the skip and the batch structure fold into one engine call; inside a classifier-free-guidance
        # group every sample carries its own scale (cd_ddim_decode_v), so the 5 guided scales of the reference's config
        # fill the calls instead of running 15 members at a time
        for grp in self._groups([(jb[1], self._kind(jb[2]), jb[2] if self._kind(jb[2]) != "cfg" else None) for jb in todo]):
            skip = todo[grp[0]][1]
            for idx in self._chunks(grp, per_call):
                n = len(idx)
                scales = [todo[i][2] for i in idx]
                if self._kind(scales[0]) == "cfg" and len(set(scales)) > 1:
                    guidance = torch.tensor([sc for sc in scales for _ in range(bsz)], dtype=torch.float32)
                else:
                    guidance = scales[0]
                if mask is not None:
                    x = self.engine.ddim_decode_masked(
                        self.unet, _ffi.CD_SCHED_DDIM, torch.cat([todo[i][3] for i in idx], dim=0).contiguous(),
                        sch.coef_decode(skip), mask, x0, sch.coef_qsample(skip),
                        mask_noise=torch.cat([todo[i][5] for i in idx], dim=1).contiguous(), ctx_c=c.repeat(n, 1, 1),
                        ctx_uc=uc.repeat(n, 1, 1), guidance=guidance,
                        noise_tail=None if todo[idx[0]][4] is None else torch.cat([todo[i][4] for i in idx], dim=1).contiguous())
                    for j, i in enumerate(idx):
                        latents[todo[i][0]] = x[j * bsz:(j + 1) * bsz]
                    continue
                x = self.engine.ddim_decode(self.unet, _ffi.CD_SCHED_DDIM,
                                            torch.cat([todo[i][3] for i in idx], dim=0).contiguous(),
                                            sch.coef_decode(skip), ctx_c=c.repeat(n, 1, 1), ctx_uc=uc.repeat(n, 1, 1),
                                            guidance=guidance,
                                            noise_tail=None if todo[idx[0]][4] is None else
                                            torch.cat([todo[i][4] for i in idx], dim=1).contiguous())
                for j, i in enumerate(idx):
                    latents[todo[i][0]] = x[j * bsz:(j + 1) * bsz]
        # decode_first_stage, then post_process (x+1)/2 fused into the final layout kernel; candidates in output order, in calls
        # of at most _vae_batch() images
        per = self._vae_batch()
        self.last_latents = [latents[k] for k in range(n_jobs)]  # the candidates' latents ahead of the first stage
        lat = torch.cat(self.last_latents, 0)
        img = torch.cat([self.engine.vae_decode(self.vae, lat[i:i + per].contiguous(), scale=self.SCALE_FACTOR,
                                                out_mul=0.5, out_add=0.5) for i in range(0, lat.shape[0], per)], 0)
        return [img[k * bsz:(k + 1) * bsz] for k in range(n_jobs)]

    @staticmethod
    def _kind(scale):  # which network batch a scale needs (ddim.py:550-559)
        return "cond" if scale == 1.0 else ("uncond" if scale == 0.0 else "cfg")

    # ---- encode + generate as ONE coupled loop (north_star; include/cyclediff.h cd_cycle_translate)
    def translate(self, image, encode_text, decode_text, mask=None, attn_ctrl=None, local_blend=None, edit_concepts=None):
        """What Model.forward composes (model/text_unsupervised_translation.py:24-40): `self(encode(image, encode_text), image,
        encode_text, decode_text)`, with the DPM-Encoder and the decode of every ensemble member running as one loop - step k of
        both evaluates the same U-Net at the same timestep, and the decode step needs eps_k only after its forward, so each
        step is ONE forward over [encoder rows | decoder rows] (C2: 12 rows per step for a batch of 4 instead of 4, then 8).
        Same draws in the same order, same member order, same per-sample arithmetic as the two calls. Chains that leave part
        of the decode to fresh noise (white_box_steps shorter than the chain) take the two calls, and so does a forward of
        more than COUPLE_MAX_TOKENS.
        `mask` (pixel-space [B, 1, R, R] in [0, 1], 1 = keep the source; or a LatentMask): the region-keeping edit - ahead of
        every forward the decoder's latent becomes src_k * m + (1 - m) * x, m the block mean of `mask` (ddim.py:427-430). x0 of
        the blend is the first-stage encoding encode() works on (the sampled z0 for the SD family). mask_source 'q_sample':
        src_k = q_sample(x0, tau[k]) with K fresh draws per candidate, made after the encoder's in the reference's order (every
        member encoded, then member -> decoder scale) - coupled or as two calls, by the same rule as without a mask.
        'encoder': src_k = the DPM-Encoder's own x_t of level k, which exists in the coupled loop only: ALWAYS the coupled loop
        - past COUPLE_MAX_TOKENS it runs in chunks of samples. The decoded image is NOT pasted over in pixel space: the kept
        region goes through the first stage like the rest. Without a mask every call below is the unmasked path's.
        `attn_ctrl` (a prebuilt (M, alpha, w) of attn_control.build_control) or `[gan] cac_steps > 0`: cross-attention control -
        in the first n_ctrl = int(cac_steps * K) iterations of a member's K-step loop the decoder's conditional rows take the
        source prompt's attention maps on the source image - recomputed from the encoder's rows of the same forward - for the
        tokens both prompts share (`attn_ctrl` replaces the built (M, alpha, w)). The source rows only exist in the coupled
        loop, so this ALWAYS runs coupled too, in chunks of samples past COUPLE_MAX_TOKENS. Composes with a keep-mask of either
        source; draw order and member order do not change. With cac_steps = 0 and no attn_ctrl nothing below changes.
        `[gan] auto_mask = diffedit` without a `mask`: the keep-mask is estimated from the two prompts on the x0 the masked
        path works on (auto_mask()) and that path runs with it; with auto_mask = none nothing below changes.
        `[gan] local_blend = words` or `local_blend` = (src_words, tgt_words), two lists of strings: prompt-to-prompt's local
        blend. The word maps of the source and of the target rows of this very run are summed over blocks and
        steps, and from iteration int(local_blend_start * K) of a member's K-step loop on every decode step is followed by x <-
        x_enc * keep + (1 - keep) * x, keep rebuilt from the sums each time. Without words the selectors mark the tokens the
        prompts do not share (attn_control.local_blend_selectors); identical prompts mark none and keep everything. ALWAYS
        the coupled loop, in chunks of samples past COUPLE_MAX_TOKENS; composes with cac_steps / attn_ctrl, not with a
        keep-mask. last_local_blend_masks: the final masks [B, 1, h, w] per candidate, last_local_blend_mask the first one's.
        With local_blend off nothing below changes.
        `[gan] edit_concepts` or `edit_concepts` = a list of semantic_guidance.EditConcept (which overrides the config; an empty
        list switches it off): semantic guidance. Every concept's context - from get_condition, like the
        prompts' - rides as one more decoder row per candidate in the forward of every step, and the decode step consumes
        eps = e_u + g (e_c - e_u) + the thresholded, weighted sum of the concept directions + momentum. The list applies to
        every sample of the call. ALWAYS the coupled loop, in chunks of samples past COUPLE_MAX_TOKENS (the concept rows are
        counted); composes with a keep-mask and with cac_steps / attn_ctrl, not with local_blend. last_edit_masks: per
        candidate the kept elements [B, E, C, h, w] of the last iteration with an active concept, last_edit_taus the
        thresholds [K, B, E]. Without concepts nothing below changes.
        `[gan] window_stride > 0`: fused windows - `image` is [B, 3, H, W], any H and W that are multiples of
        the first-stage factor with a latent of at least image_size x image_size; see _translate_windows. With window_stride =
        0 nothing below changes."""
        if getattr(self, "window_stride", 0):
            return self._translate_windows(image, encode_text, decode_text, mask, attn_ctrl, local_blend, edit_concepts)
        concepts = list(edit_concepts) if edit_concepts is not None else list(getattr(self, "edit_concepts", None) or [])
        sega = len(concepts) > 0
        blend = local_blend is not None or getattr(self, "local_blend", "none") != "none"
        if sega:
            s_m, beta = getattr(self, "edit_momentum_scale", 0.3), getattr(self, "edit_momentum_beta", 0.6)
            sgm.check_concepts(concepts, s_m, beta)
            if blend:
                raise ValueError("edit_concepts and local_blend are not built together: switch one of them off")
            if self.precision in ("fp32", "fp32x3"):
                raise ValueError("edit_concepts needs the 16-bit precision: semantic guidance is not built for the fp32 / fp32x3 "
                                 "networks")
        if blend and (mask is not None or self._auto_mask_on()):
            raise ValueError("local_blend builds its own keep-mask after every step: it takes no mask= and no auto_mask")
        if blend and self.precision in ("fp32", "fp32x3"):
            raise ValueError("local_blend needs the 16-bit precision: the word maps are not built for the fp32 / fp32x3 "
                             "networks' transformer blocks")
        if mask is None and self._auto_mask_on():
            mask = AUTO_MASK  # estimated below, once x0 exists
        sch = self._schedule()
        bsz = image.shape[0]
        whole = all(self._white_box_loop(len(sch) - sk, sk) == len(sch) - sk for sk in self.skip_steps)
        dec_scales = [float(sc) for sc in self.decoder_unconditional_guidance_scales]
        n_dec = len(dec_scales)
        kinds = [self._kind(sc) for sc in dec_scales]
        main = "cfg" if "cfg" in kinds else kinds[0]  # the decoder scales that ride with the encoder (the others decode from z)
        ride = [j for j in range(n_dec) if kinds[j] == main and (main == "cfg" or dec_scales[j] == dec_scales[kinds.index(main)])]
        enc_kinds = [self._kind(float(sc)) for sc in self.encoder_unconditional_guidance_scales]
        rows1 = (2 if "cfg" in enc_kinds else 1) + len(ride) * (2 if main == "cfg" else 1)  # rows of one sample of one member
        if sega:
            rows1 += len(ride) * len(concepts)  # one more decoder row per concept and candidate
        tokens = self.image_size ** 2
        fits = bsz * rows1 * tokens <= self.couple_max_tokens
        ctrl = attn_ctrl is not None or self.cac_steps > 0
        if ctrl and not whole:
            raise ValueError("cross-attention control needs the DPM-Encoder over the whole chain (white_box_steps = custom_steps "
                             "+ 1): the steps past a shorter prefix have no source rows")
        if ctrl and (len(ride) != n_dec or main == "uncond" or "uncond" in enc_kinds):
            raise ValueError("cross-attention control: every decoder scale must ride in the coupled loop (all guided, or one "
                             "unguided scale) and no scale may be 0 - the control acts on conditional rows")
        if sega and not whole:
            raise ValueError("edit_concepts needs the DPM-Encoder over the whole chain (white_box_steps = custom_steps + 1): "
                             "the guidance lives in the coupled loop")
        if sega and (len(ride) != n_dec or main != "cfg"):
            raise ValueError("edit_concepts: every decoder scale must ride in the coupled loop and be guided (neither 0 nor "
                             "1) - a concept's direction is taken against the unconditional row")
        if blend and not whole:
            raise ValueError("local_blend needs the DPM-Encoder over the whole chain (white_box_steps = custom_steps + 1): the "
                             "steps past a shorter prefix have no source rows")
        if blend and (len(ride) != n_dec or main == "uncond" or "uncond" in enc_kinds):
            raise ValueError("local_blend: every decoder scale must ride in the coupled loop (all guided, or one unguided "
                             "scale) and no scale may be 0 - the maps are those of conditional rows")
        m = None if mask is None or mask is AUTO_MASK else self._latent_mask(mask, bsz)
        encoder = mask is not None and self.mask_source == "encoder"
        if encoder and not whole:
            raise ValueError("mask_source = 'encoder' needs the DPM-Encoder over the whole chain (white_box_steps = "
                             "custom_steps + 1): a shorter prefix has no encoder trajectory for the remaining steps")
        if encoder and len(ride) != n_dec:
            raise ValueError("mask_source = 'encoder': every decoder scale must ride in the coupled loop (all guided, or "
                             "one unguided scale) - a candidate decoded from z afterwards has no encoder trajectory")
        coupled = ctrl or encoder or blend or sega or bool(self.couple and whole and fits)
        self.last_translate_coupled = coupled
        sels, keep_parts = None, {}
        if blend:
            src_ids, eos = self._control_ids(encode_text)
            tgt_ids, _ = self._control_ids(decode_text)
            words = None
            if local_blend is not None:
                words = []
                for ws in local_blend:
                    wids = self._control_ids(list(ws))[0] if len(ws) else []
                    words.append([list(r[1:attn_control.prompt_length(r, eos)]) for r in wids])
            pairs = [attn_control.local_blend_selectors(src_ids[b], tgt_ids[b], eos, words) for b in range(bsz)]
            sels = [torch.from_numpy(np.stack([p[i] for p in pairs], 0)).to(self.device) for i in (0, 1)]
            side = self.local_blend_side or self.image_size // 4
        ctl = None
        if ctrl:
            if attn_ctrl is None:
                src_ids, eos = self._control_ids(encode_text)
                tgt_ids, _ = self._control_ids(decode_text)
                attn_ctrl = attn_control.build_control(src_ids, tgt_ids, self.cac_mode, eos_id=eos)
            ctl = [torch.as_tensor(t, dtype=torch.float32).to(self.device) for t in attn_ctrl]
            if ctl[0].shape[0] != bsz:
                raise ValueError("attn_ctrl must carry one control per sample (%d), got %d" % (bsz, ctl[0].shape[0]))
        x0, c_src, uc, members = self._encode_front(image, encode_text)
        c_tgt = self.get_condition(decode_text, bsz)[0] if coupled or mask is AUTO_MASK else None
        if mask is AUTO_MASK:
            m = self._auto_mask_ctx(x0, c_src, c_tgt)[0]
        masked = {} if m is None else dict(mask=m, x0=x0)  # generate()'s share of the keep-mask
        c_edit, emask_parts, tau_parts = None, {}, {}
        if sega:
            c_edit = [self.get_condition([str(cc.text)] * bsz, bsz)[0] for cc in concepts]
        if not coupled:  # what encode() + forward() do
            z_ensemble = self._encode_members(x0, c_src, uc, members)
            return self._select(self.generate(z_ensemble, decode_text, **masked), image, encode_text, decode_text)
        mask_noise = {}
        if m is not None and not encoder:  # the reference's order: every member encoded, then member -> decoder scale, K draws
            for i, mem in enumerate(members):
                for j in range(n_dec):
                    mask_noise[i * n_dec + j] = self._mask_draws(len(sch) - mem[1], bsz)[0]
        bc = bsz if fits else max(1, self.couple_max_tokens // (rows1 * tokens))  # samples per coupled call
        per_call = max(1, min(self.MAX_FOLD // (bc * (1 + len(ride))), self.couple_max_tokens // (bc * rows1 * tokens)))
        z_parts, lat_parts = [[] for _ in members], {}
        for s0 in range(0, bsz, bc):
            sl = slice(s0, min(bsz, s0 + bc))
            nb = sl.stop - sl.start
            for grp in self._groups([(mm[0], mm[1]) for mm in members]):
                enc_scale, skip = members[grp[0]][0], members[grp[0]][1]
                for idx in self._chunks(grp, per_call):
                    n, nr = len(idx), len(ride)
                    if main == "cfg" and len({dec_scales[j] for j in ride}) > 1:
                        guidance = torch.tensor([dec_scales[j] for j in ride for _ in range(n * nb)], dtype=torch.float32)
                    else:
                        guidance = dec_scales[ride[0]]
                    args = (self.unet, _ffi.CD_SCHED_DDIM, x0[sl].repeat(n, 1, 1, 1), sch.coef_encode(skip), sch.coef_decode(skip))
                    kw = dict(enc_ctx_c=c_src[sl].repeat(n, 1, 1), enc_ctx_uc=uc[sl].repeat(n, 1, 1), enc_guidance=enc_scale,
                              dec_ctx_c=c_tgt[sl].repeat(n * nr, 1, 1), dec_ctx_uc=uc[sl].repeat(n * nr, 1, 1),
                              dec_guidance=guidance, n_dec=nr, last_uses_x0=True,
                              noise=torch.cat([members[i][2][:, sl] for i in idx], dim=1).contiguous())
                    if m is not None:
                        kw["mask_source"] = self.mask_source
                        if not encoder:  # decoder row (jr * n + mi) * nb + b
                            kw.update(mask_x0=x0[sl].contiguous(), qcoef=sch.coef_qsample(skip), mask_noise=torch.cat(
                                [mask_noise[i * n_dec + j][:, sl] for j in ride for i in idx], dim=1).contiguous())
                    if sega:
                        K = len(sch) - skip
                        if m is not None:
                            kw["mask"] = m[sl].contiguous()
                        z, x, taus, _kept, emask = self.engine.cycle_translate_sega(
                            *args, torch.cat([ce[sl].repeat(n * nr, 1, 1) for ce in c_edit], 0).contiguous(),
                            sgm.concept_table(concepts, K, int(np.prod(x0.shape[1:]))), s_m, beta,
                            ctrl=None if ctl is None else (ctl[0][sl].contiguous(), ctl[1][sl].contiguous(),
                                                           ctl[2][sl].contiguous(), int(self.cac_steps * K)), **kw)
                        for mi, i in enumerate(idx):
                            for jr, j in enumerate(ride):
                                rows = slice((jr * n + mi) * nb, (jr * n + mi + 1) * nb)
                                emask_parts.setdefault(i * n_dec + j, []).append(emask[rows])
                                tau_parts.setdefault(i * n_dec + j, []).append(taus[:, rows])
                    elif sels is not None:
                        K = len(sch) - skip
                        z, x, _acc, keep = self.engine.cycle_translate_blend(
                            *args, sels[0][sl].contiguous(), sels[1][sl].contiguous(), side, pool=self.local_blend_pool,
                            thr=self.local_blend_threshold, n_start=attn_control.local_blend_start(self.local_blend_start, K),
                            ctrl=None if ctl is None else (ctl[0][sl].contiguous(), ctl[1][sl].contiguous(),
                                                           ctl[2][sl].contiguous(), int(self.cac_steps * K)), **kw)
                        for mi, i in enumerate(idx):
                            for jr, j in enumerate(ride):
                                keep_parts.setdefault(i * n_dec + j, []).append(keep[(jr * n + mi) * nb:(jr * n + mi + 1) * nb])
                    elif ctl is not None:
                        if m is not None:
                            kw["mask"] = m[sl].contiguous()
                        z, x = self.engine.cycle_translate_ctrl(
                            *args, mapper=ctl[0][sl].contiguous(), alpha=ctl[1][sl].contiguous(), weight=ctl[2][sl].contiguous(),
                            n_ctrl=int(self.cac_steps * (len(sch) - skip)), **kw)
                    elif m is not None:
                        z, x = self.engine.cycle_translate_masked(*args, m[sl].contiguous(), **kw)
                    else:
                        z, x = self.engine.cycle_translate(*args, **kw)
                    for mi, i in enumerate(idx):
                        z_parts[i].append(z[mi * nb:(mi + 1) * nb].reshape(nb, -1))
                        for jr, j in enumerate(ride):
                            lat_parts.setdefault(i * n_dec + j, []).append(x[(jr * n + mi) * nb:(jr * n + mi + 1) * nb])
        z_ensemble = [p[0] if len(p) == 1 else torch.cat(p, 0) for p in z_parts]  # one part: the whole batch fitted
        latents = {k: v[0] if len(v) == 1 else torch.cat(v, 0) for k, v in lat_parts.items()}
        if sega:
            self.last_edit_masks = [torch.cat(emask_parts[k], 0) for k in sorted(emask_parts)]
            self.last_edit_taus = [torch.cat(tau_parts[k], 1) for k in sorted(tau_parts)]
        if sels is not None:
            self.last_local_blend_masks = [torch.cat(keep_parts[k], 0) for k in sorted(keep_parts)]
            self.last_local_blend_mask = self.last_local_blend_masks[0]
        img_ensemble = self.generate(z_ensemble, decode_text, latents=latents, mask_noise=mask_noise, **masked)
        return self._select(img_ensemble, image, encode_text, decode_text)

    def _translate_windows(self, image, encode_text, decode_text, mask=None, attn_ctrl=None, local_blend=None,
                           edit_concepts=None):
        """translate() with `[gan] window_stride > 0`: the latent of a [B, 3, H, W] image is a canvas [H / f, W / f] on which
        the noise prediction of a cell is the average over the image_size x image_size windows that cover it
        (windows.window_grid, cd_translate_args.n_win). Same draws in the same order as translate() on the canvas's shape,
        same member order. ALWAYS the coupled loop, in chunks of samples so that rows x windows x tokens stays within
        COUPLE_MAX_TOKENS; the whole chain and every decoder scale riding in the loop are required. The keep-mask, cross-
        attention control, the local blend and semantic guidance are not built together with windows yet."""
        given = [n for n, on in (("mask=", mask is not None), ("auto_mask", self._auto_mask_on()),
                                 ("attn_ctrl=", attn_ctrl is not None), ("cac_steps", self.cac_steps > 0),
                                 ("local_blend", local_blend is not None or getattr(self, "local_blend", "none") != "none"),
                                 ("edit_concepts", bool(edit_concepts) or (edit_concepts is None and
                                                                           bool(getattr(self, "edit_concepts", None))))) if on]
        if given:
            raise ValueError("window_stride is not built together with %s yet: switch the windows or %s off"
                             % (", ".join(given), "it" if len(given) == 1 else "them"))
        f, S = self.vae_factor, self.image_size
        if image.dim() != 4 or image.shape[2] % f or image.shape[3] % f or image.shape[2] // f < S or image.shape[3] // f < S:
            raise ValueError("window_stride: the image must be [B, 3, H, W] with H and W multiples of %d and at least %d, got %s"
                             % (f, f * S, tuple(image.shape)))
        Hc, Wc = image.shape[2] // f, image.shape[3] // f
        win = wnd.window_grid(Hc, Wc, S, self.window_stride)
        sch = self._schedule()
        bsz, n_win = image.shape[0], len(win)
        if not all(self._white_box_loop(len(sch) - sk, sk) == len(sch) - sk for sk in self.skip_steps):
            raise ValueError("window_stride needs the DPM-Encoder over the whole chain (white_box_steps = custom_steps + 1): the "
                             "fused windows live in the coupled loop")
        dec_scales = [float(sc) for sc in self.decoder_unconditional_guidance_scales]
        n_dec = len(dec_scales)
        kinds = [self._kind(sc) for sc in dec_scales]
        main = "cfg" if "cfg" in kinds else kinds[0]
        if any(k != main for k in kinds) or (main != "cfg" and len(set(dec_scales)) > 1):
            raise ValueError("window_stride: every decoder scale must ride in the coupled loop (all guided, or one unguided "
                             "scale) - a candidate decoded from z afterwards would run the network without windows")
        enc_kinds = [self._kind(float(sc)) for sc in self.encoder_unconditional_guidance_scales]
        rows1 = ((2 if "cfg" in enc_kinds else 1) + n_dec * (2 if main == "cfg" else 1)) * n_win  # network rows of one sample
        tokens = S * S
        self.last_translate_coupled = True
        x0, c_src, uc, members = self._encode_front(image, encode_text)
        c_tgt = self.get_condition(decode_text, bsz)[0]
        bc = max(1, min(bsz, self.couple_max_tokens // (rows1 * tokens)))  # samples per coupled call
        per_call = max(1, min(self.MAX_FOLD // (bc * (1 + n_dec)), self.couple_max_tokens // (bc * rows1 * tokens)))
        z_parts, lat_parts = [[] for _ in members], {}
        for s0 in range(0, bsz, bc):
            sl = slice(s0, min(bsz, s0 + bc))
            nb = sl.stop - sl.start
            for grp in self._groups([(mm[0], mm[1]) for mm in members]):
                enc_scale, skip = members[grp[0]][0], members[grp[0]][1]
                for idx in self._chunks(grp, per_call):
                    n = len(idx)
                    if main == "cfg" and len(set(dec_scales)) > 1:
                        guidance = torch.tensor([sc for sc in dec_scales for _ in range(n * nb)], dtype=torch.float32)
                    else:
                        guidance = dec_scales[0]
                    z, x = self.engine.cycle_translate(
                        self.unet, _ffi.CD_SCHED_DDIM, x0[sl].repeat(n, 1, 1, 1), sch.coef_encode(skip), sch.coef_decode(skip),
                        enc_ctx_c=c_src[sl].repeat(n, 1, 1), enc_ctx_uc=uc[sl].repeat(n, 1, 1), enc_guidance=enc_scale,
                        dec_ctx_c=c_tgt[sl].repeat(n * n_dec, 1, 1), dec_ctx_uc=uc[sl].repeat(n * n_dec, 1, 1),
                        dec_guidance=guidance, n_dec=n_dec, last_uses_x0=True,
                        noise=torch.cat([members[i][2][:, sl] for i in idx], dim=1).contiguous(), windows=win)
                    for mi, i in enumerate(idx):
                        z_parts[i].append(z[mi * nb:(mi + 1) * nb].reshape(nb, -1))
                        for j in range(n_dec):
                            lat_parts.setdefault(i * n_dec + j, []).append(x[(j * n + mi) * nb:(j * n + mi + 1) * nb])
        self.last_z_ensemble = [p[0] if len(p) == 1 else torch.cat(p, 0) for p in z_parts]
        self.last_latents = [lat_parts[k][0] if len(lat_parts[k]) == 1 else torch.cat(lat_parts[k], 0)
                             for k in range(len(members) * n_dec)]
        lat = torch.cat(self.last_latents, 0)
        per = self._vae_batch(image.shape[2] * image.shape[3])
        img = torch.cat([self.engine.vae_decode(self.vae, lat[i:i + per].contiguous(), scale=self.SCALE_FACTOR,
                                                out_mul=0.5, out_add=0.5) for i in range(0, lat.shape[0], per)], 0)
        return self._select([img[k * bsz:(k + 1) * bsz] for k in range(len(self.last_latents))], image, encode_text, decode_text)

    def _control_ids(self, texts):
        """token ids [B, L] of the prompts and the id that ends a prompt, from the text encoder's own tokenizer; a conditioning
        stage without one (a callable embedder) falls back to the whitespace hash tokenizer, padded to the context length"""
        from .text_encoders import EOS, BertHashTokenizer, BertWordPieceTokenizer, HashTokenizer
        tok = getattr(self.cond_stage, "tokenizer", None)
        if tok is None:
            tok = HashTokenizer(getattr(self.cond_stage, "length", 77))
        eos = BertHashTokenizer.SEP if isinstance(tok, (BertHashTokenizer, BertWordPieceTokenizer)) else EOS
        return np.asarray(tok(list(texts))), eos

    def forward(self, z_ensemble, original_img, encode_text, decode_text, mask=None):
        """`mask` (pixel-space [B, 1, R, R] in [0, 1], 1 = keep the source): the reference's sample_with_eps(mask=, x0=) decode.
        The blend's x0 is `original_img` re-encoded here with the posterior MEAN - no noise is drawn for it, whatever the
        family's encode() samples. Only mask_source 'q_sample' exists on this two-call path: the encoder's trajectory is gone
        once encode() has returned. The decoded image is not pasted over in pixel space: the kept region goes through the
        first stage like the rest."""
        if getattr(self, "window_stride", 0):
            raise ValueError("window_stride needs translate(): the fused windows run on the coupled loop, which encode() + "
                             "forward() do not take; use translate(image, encode_text, decode_text)")
        if getattr(self, "cac_steps", 0.0) > 0:
            raise ValueError("cac_steps > 0 needs translate(): in encode() + forward() the source rows whose attention maps the "
                             "control injects no longer exist; use translate(image, encode_text, decode_text)")
        if getattr(self, "edit_concepts", None):
            raise ValueError("edit_concepts needs translate(): in encode() + forward() the coupled loop in which the concept "
                             "rows ride no longer exists; use translate(image, encode_text, decode_text)")
        if getattr(self, "local_blend", "none") != "none":
            raise ValueError("local_blend needs translate(): in encode() + forward() the source rows whose word maps and whose "
                             "latents the blend uses no longer exist; use translate(image, encode_text, decode_text)")
        if mask is None and self._auto_mask_on():
            mask = AUTO_MASK  # estimated below on the re-encoded x0
        if mask is None:
            return self._select(self.generate(z_ensemble, decode_text), original_img, encode_text, decode_text)
        if self.mask_source == "encoder":
            raise ValueError("mask_source = 'encoder' needs translate(): in encode() + forward() the encoder's trajectory no "
                             "longer exists; use translate(image, encode_text, decode_text, mask=) or mask_source = q_sample")
        bsz = z_ensemble[0].shape[0]
        m = None if mask is AUTO_MASK else self._latent_mask(mask, bsz)
        img = ((original_img - 0.5) * 2.0).to(self.device, torch.float32)
        per = self._vae_batch()
        x0 = torch.cat([self.engine.vae_encode(self.vae, img[i:i + per], sample=False, scale=self.SCALE_FACTOR)
                        for i in range(0, bsz, per)], 0)
        if m is None:
            m = self.auto_mask(x0, encode_text, decode_text)[0]
        return self._select(self.generate(z_ensemble, decode_text, mask=m, x0=x0), original_img, encode_text, decode_text)

    def _select(self, img_ensemble, original_img, encode_text, decode_text):
        """the candidate the reference returns (sd_wrapper:213-249): the only one, or per sample the directional-CLIP argmax"""
        assert len(img_ensemble) == self._ensemble_size()
        if len(img_ensemble) == 1:
            return img_ensemble[0]
        if self.ranker is None:
            raise NotImplementedError(
                "ensemble of %d candidates needs a DirectionalCLIP ranker (model/energy/clean_clip.py) — out of "
                "scope for the hot path; pass ranker=callable(img, original_img, encode_text, decode_text)"
                % len(img_ensemble))
        def score(img):  # DirectionalCLIP returns (clip_score, dclip_score) and the reference ranks by the latter
            r = self.ranker(img, original_img, encode_text, decode_text)
            return r[1] if isinstance(r, (tuple, list)) else r
        if self.fold_ensemble:
            # the reference scores candidate by candidate (sd_wrapper:216-227); candidates are independent samples of the
            # ranker's batch, so they are scored MAX_FOLD images at a time (same per-sample scores, 1/32 of the calls)
            bsz, per_call = original_img.shape[0], max(1, self.MAX_FOLD // original_img.shape[0])
            parts = []
            for j0 in range(0, len(img_ensemble), per_call):
                chunk = img_ensemble[j0:j0 + per_call]
                n = len(chunk)
                if hasattr(self.ranker, "score_folded"):  # the built-in ranker encodes texts and source images once
                    sc = self.ranker.score_folded(torch.cat(chunk, dim=0), original_img, encode_text, decode_text, n)
                else:
                    sc = self.ranker(torch.cat(chunk, dim=0), original_img.repeat(n, 1, 1, 1), list(encode_text) * n,
                                     list(decode_text) * n)
                sc = sc[1] if isinstance(sc, (tuple, list)) else sc
                parts.append(sc.view(n, bsz).t())
            scores = torch.cat(parts, dim=1)
        else:
            scores = torch.stack([score(img) for img in img_ensemble], dim=1)
        best = torch.argmax(scores, dim=1)  # per-sample argmax over the ensemble (sd_wrapper:228-235)
        return torch.stack([img_ensemble[best[b].item()][b] for b in range(scores.shape[0])], dim=0)

    @property
    def device(self):
        return next(self.parameters()).device


class SDStochasticTextWrapper(_LatentStochasticTextWrapper):
    """gan_type = SDStochasticText (v1-inference.yaml; 512 px; posterior SAMPLED, ddpm.py:538)."""
    UNET_DESC = staticmethod(sd_v1_unet_desc)
    RESOLUTION = 512
    SAMPLE_POSTERIOR = True

    @staticmethod
    def checkpoint_path(source_model_type):  # sd_wrapper:24
        return os.path.join("ckpts", "stable_diffusion", source_model_type)


class LatentDiffStochasticTextWrapper(_LatentStochasticTextWrapper):
    """gan_type = LatentDiffStochasticText (txt2img-1p4B-eval.yaml; 256 px; posterior MEAN,
    model/lib/latentdiff/ldm/models/diffusion/ddpm.py:535-538; linear schedule 0.00085..0.012)."""
    UNET_DESC = staticmethod(ldm_text_unet_desc)
    RESOLUTION = 256
    SAMPLE_POSTERIOR = False

    @staticmethod
    def checkpoint_path(source_model_type):  # latentdiff_stochastic_text_wrapper.py:20-23
        if source_model_type != "text2img-large":
            raise ValueError(source_model_type)
        return os.path.join("ckpts", "ldm_models", source_model_type, "model.ckpt")
