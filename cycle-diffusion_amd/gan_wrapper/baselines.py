"""The baselines the paper compares CycleDiffusion with (README "CycleDiffusion (ours) vs DDIB vs SDEdit"; the unpaired
Cat -> Dog / Wild -> Dog tables, which also list ILVR), as gan_types beside the wrappers they mirror - same text encoders,
first stage, ranker, precision and noise hooks:

  DDIB   deterministic DDIM inversion under the source (model / text), then a deterministic DDIM decode under the target.
         Inversion: include/cyclediff.h cd_ddim_invert on DDIMSchedule.coef_invert / PixelSchedule.coef_invert rows
         (DiffusionCLIP's denoising_step(eta=0, 'ddim') walked with t_next > t, diffusion_utils.py:114-121); decode:
         cd_ddim_decode(_v) on eta = 0 rows (DDIMSampler.decode on a ddim_eta = 0 schedule, ddim.py:663-681).
  SDEdit q-sample the source to an intermediate level, then run the target's ordinary stochastic decode from there:
         stochastic_encode + decode (ddim.py:648-681) for the latent models, sample_xt + generate()'s chain for the pixel
         DDPMs (ddpm_ddim_wrapper.py:310-314, 392-430). The q-sample is cd_dpm_encode with K = 0, the decode is the
         existing decode-with-eps path (cd_ddim_decode(_v) with the per-step noise injected as eps).
  ILVR   (pixel DDPMs only) the target's ordinary stochastic chain from pure noise; after every step above `ilvr_range_t` the
         running image takes the low-pass band of the freshly noised source image, x <- x' + phi_N(y' - x') (Choi et al.,
         ICCV 2021, Algorithm 1; cd_ilvr_decode). No source model is evaluated.

None of these classes has a translate(): Model.forward runs encode() then forward(), as the reference composes them.
"""
import torch

from .. import _ffi, attn_control, auto_mask, schedule, semantic_guidance, windows
from .ddpm_ddim_wrapper import DDPMDDIMWrapper
from .latent_text_wrapper import LatentDiffStochasticTextWrapper, SDStochasticTextWrapper


def _reject(method, **keys):
    """[gan] keys that mean nothing for a method are an error, not silently dropped"""
    given = sorted(k for k, v in keys.items() if v is not None)
    if given:
        raise ValueError("%s does not use %s: remove %s from the [gan] section" % (method, ", ".join(given),
                                                                                  "it" if len(given) == 1 else "them"))


class _NoCoupledLoop:
    @property
    def translate(self):  # the coupled loop is CycleDiffusion's: hasattr(wrapper, "translate") is False here
        raise AttributeError("translate")


class _LatentBaseline(_NoCoupledLoop):
    """Shared decode of the latent baselines: jobs (output slot, decode rows, n_eps, decoder scale, z [B, T, C, h, w]) that
    share their rows and batch structure fold into one cd_ddim_decode(_v) call, as the CycleDiffusion wrapper folds its
    ensemble; then the first stage and the post-process (x + 1) / 2."""

    @property
    def word_maps(self):  # the per-word attention maps belong to the CycleDiffusion text wrappers, like translate
        raise AttributeError("word_maps")

    def forward(self, z_ensemble, original_img, encode_text, decode_text, mask=None):
        if mask is not None:
            raise ValueError("%s takes no keep-mask: the region-keeping decode is CycleDiffusion's (SDStochasticText / "
                             "LatentDiffStochasticText)" % type(self).__name__)
        return super().forward(z_ensemble, original_img, encode_text, decode_text)

    def _decode_jobs(self, jobs, decode_text, bsz):
        c, uc = self.get_condition(decode_text, bsz)
        latents = {}
        per_call = max(1, self.MAX_FOLD // bsz)
        keys = [(jb[1].tobytes(), jb[2], self._kind(jb[3]), jb[3] if self._kind(jb[3]) != "cfg" else None) for jb in jobs]
        for grp in self._groups(keys):
            rows, n_eps = jobs[grp[0]][1], jobs[grp[0]][2]
            for idx in self._chunks(grp, per_call):
                n = len(idx)
                scales = [jobs[i][3] for i in idx]
                if self._kind(scales[0]) == "cfg" and len(set(scales)) > 1:
                    guidance = torch.tensor([sc for sc in scales for _ in range(bsz)], dtype=torch.float32)
                else:
                    guidance = scales[0]
                x = self.engine.ddim_decode(self.unet, _ffi.CD_SCHED_DDIM, torch.cat([jobs[i][4] for i in idx], 0).contiguous(),
                                            rows, n_eps=n_eps, ctx_c=c.repeat(n, 1, 1), ctx_uc=uc.repeat(n, 1, 1),
                                            guidance=guidance)
                for j, i in enumerate(idx):
                    latents[jobs[i][0]] = x[j * bsz:(j + 1) * bsz]
        self.last_latents = [latents[k] for k in range(len(jobs))]
        per = self._vae_batch()
        lat = torch.cat(self.last_latents, 0)
        img = torch.cat([self.engine.vae_decode(self.vae, lat[i:i + per].contiguous(), scale=self.SCALE_FACTOR,
                                                out_mul=0.5, out_add=0.5) for i in range(0, lat.shape[0], per)], 0)
        return [img[k * bsz:(k + 1) * bsz] for k in range(len(jobs))]


class _LatentDDIBText(_LatentBaseline):
    """DDIB on a text-conditioned latent model. Ensemble: encoder scale -> skip (one trial: the method is deterministic), then
    decoder scales; encode() returns one x_T [B, C*h*w] per (encoder scale, skip)."""

    def __init__(self, source_model_type, custom_steps, skip_steps=(0,), eta=None, n_trials=1, white_box_steps=None, **kw):
        if eta not in (None, 0, 0.0):
            raise ValueError("DDIB is deterministic: eta must be 0 or absent, got %r" % (eta,))
        if (n_trials or 1) != 1:
            raise ValueError("DDIB is deterministic: n_trials must be 1, got %r" % (n_trials,))
        # the inversion is the whole chain (skip_steps shortens it); cross-attention control needs the coupled loop's source rows
        _reject("DDIB", white_box_steps=white_box_steps, cac_steps=kw.pop("cac_steps", None), cac_mode=kw.pop("cac_mode", None))
        auto_mask.refuse(kw, "DDIB")
        attn_control.refuse_local_blend(kw, "DDIB")
        semantic_guidance.refuse(kw, "DDIB")
        windows.refuse(kw, "DDIB")
        kw.setdefault("encoder_unconditional_guidance_scales", [1.0])
        kw.setdefault("decoder_unconditional_guidance_scales", [1.0])
        super().__init__(source_model_type, custom_steps, 0.0, -1, list(skip_steps), n_trials=1, couple=False, **kw)
        for skip in self.skip_steps:
            assert 0 <= skip < custom_steps, skip

    def _schedule(self):  # ddim_eta = 0: sigma = 0 rows for the decode; a / a_prev do not depend on eta
        return schedule.DDIMSchedule(self.alphas_cumprod, self.custom_steps, 0.0)

    def encode(self, image, encode_text):
        x0 = self._first_stage(image)
        bsz, sch = x0.shape[0], self._schedule()
        c, uc = self.get_condition(encode_text, bsz)
        z_ensemble = []
        for enc_scale in self.encoder_unconditional_guidance_scales:
            for skip in self.skip_steps:
                xT = self.engine.ddim_invert(self.unet, x0, sch.coef_invert(skip), ctx_c=c, ctx_uc=uc,
                                             guidance=float(enc_scale))
                z_ensemble.append(xT.reshape(bsz, -1))
        return z_ensemble

    def generate(self, z_ensemble, decode_text):
        sch = self._schedule()
        bsz = z_ensemble[0].shape[0]
        jobs = []
        for i, z in enumerate(z_ensemble):
            skip = int(self.skip_steps[i % len(self.skip_steps)])
            zz = z.view(bsz, 1, self.channels, self.image_size, self.image_size)
            for dec_scale in self.decoder_unconditional_guidance_scales:
                jobs.append((len(jobs), sch.coef_decode(skip), 0, float(dec_scale), zz))
        return self._decode_jobs(jobs, decode_text, bsz)


class _LatentSDEditText(_LatentBaseline):
    """SDEdit on a text-conditioned latent model. `sdedit_strengths` (list): strength s starts the target's decode at
    t_enc = int(s * custom_steps), 1 <= t_enc <= custom_steps - 1. Ensemble: trial -> strength, then decoder scales; encode()
    returns [z_t, n_1 .. n_t_enc] as [B, (t_enc + 1)*C*h*w] per (trial, strength)."""

    def __init__(self, source_model_type, custom_steps, eta, sdedit_strengths, n_trials=1, skip_steps=None,
                 white_box_steps=None, encoder_unconditional_guidance_scales=None, **kw):
        self.sdedit_strengths = [float(s) for s in sdedit_strengths]
        self.t_encs = [int(s * custom_steps) for s in self.sdedit_strengths]
        for s, t in zip(self.sdedit_strengths, self.t_encs):
            if not 1 <= t <= custom_steps - 1:
                raise ValueError("sdedit strength %r gives t_enc = %d outside [1, %d]" % (s, t, custom_steps - 1))
        # no DPM-Encoder and no inversion: the strength alone sets where the decode starts
        _reject("SDEdit", skip_steps=skip_steps, white_box_steps=white_box_steps,
                encoder_unconditional_guidance_scales=encoder_unconditional_guidance_scales,
                cac_steps=kw.pop("cac_steps", None), cac_mode=kw.pop("cac_mode", None))
        auto_mask.refuse(kw, "SDEdit")
        attn_control.refuse_local_blend(kw, "SDEdit")
        semantic_guidance.refuse(kw, "SDEdit")
        windows.refuse(kw, "SDEdit")
        kw.setdefault("decoder_unconditional_guidance_scales", [1.0])
        super().__init__(source_model_type, custom_steps, eta, -1, [0], encoder_unconditional_guidance_scales=[1.0],
                         n_trials=n_trials or 1, couple=False, **kw)

    def _ensemble_size(self):
        return (self.n_trials or 1) * len(self.sdedit_strengths) * len(self.decoder_unconditional_guidance_scales or [1])

    def encode(self, image, encode_text):
        x0 = self._first_stage(image)
        bsz, sch = x0.shape[0], self._schedule()
        c, _uc = self.get_condition(encode_text, bsz)
        z_ensemble = []
        for _trial in range(self.n_trials):
            for t_enc in self.t_encs:
                # draw order of stochastic_encode (randn_like(x0), ddim.py:659) then decode's noise_like per step (:537)
                if self.noise_on_cpu or self.noise_source is not None:
                    nz = torch.stack([self._randn(tuple(x0.shape)) for _ in range(t_enc + 1)], 0)
                else:
                    nz = self._randn((t_enc + 1,) + tuple(x0.shape))
                start, _rows = sch.coef_sdedit(t_enc)
                # the q-sample is cd_dpm_encode with K = 0 (no forward; the context only satisfies the network's contract)
                zt = self.engine.dpm_encode(self.unet, _ffi.CD_SCHED_DDIM, x0, start, ctx_c=c, noise=nz[:1],
                                            last_uses_x0=False)
                z = torch.cat([zt, nz[1:].transpose(0, 1)], 1)
                z_ensemble.append(z.reshape(bsz, -1))
        return z_ensemble

    def generate(self, z_ensemble, decode_text):
        sch = self._schedule()
        bsz = z_ensemble[0].shape[0]
        jobs = []
        for i, z in enumerate(z_ensemble):
            t_enc = self.t_encs[i % len(self.t_encs)]
            # decode(z_t, t_start=t_enc): the noise of level t_enc meets decode indices t_enc-1 .. 0 - a deliberate copy of
            # the reference's img2img pairing (ddim.py:648-681, stable_diffusion/scripts/img2img.py), not an off-by-one here
            _start, rows = sch.coef_sdedit(t_enc)
            zz = z.view(bsz, t_enc + 1, self.channels, self.image_size, self.image_size)
            for dec_scale in self.decoder_unconditional_guidance_scales:
                jobs.append((len(jobs), rows, t_enc, float(dec_scale), zz))
        return self._decode_jobs(jobs, decode_text, bsz)


class SDDDIBTextWrapper(_LatentDDIBText, SDStochasticTextWrapper):
    """gan_type = SDDDIBText"""


class LatentDiffDDIBTextWrapper(_LatentDDIBText, LatentDiffStochasticTextWrapper):
    """gan_type = LatentDiffDDIBText"""


class SDSDEditTextWrapper(_LatentSDEditText, SDStochasticTextWrapper):
    """gan_type = SDSDEditText"""


class LatentDiffSDEditTextWrapper(_LatentSDEditText, LatentDiffStochasticTextWrapper):
    """gan_type = LatentDiffSDEditText"""


# ------------------------------------------------------------------------------------ pixel DDPMs (two models)
class DDPMDDIBWrapper(_NoCoupledLoop, DDPMDDIMWrapper):
    """gan_type = DDPM_DDIB. Source side: encode(image) = DiffusionCLIP's inversion loop over generate()'s seq_inv (t = seq[k-1]
    -> t_next = seq[k], k = 1 .. es_steps-1, eta = 0) -> x_T [B, C*R*R]. Target side: forward(z) = the eta = 0 decode over the
    reversed pairs (the last step to t_next = -1), then the wrapper's refinement and post-process."""

    def __init__(self, source_model_type, custom_steps, es_steps, sample_type="ddim", eta=None, **kw):
        super().__init__(source_model_type, sample_type, custom_steps, es_steps, eta=0.0 if eta is None else eta, **kw)
        self.latent_dim = self.resolution ** 2 * self.channels

    @staticmethod
    def _check_eta(sample_type, eta):  # in place of the stochastic chain's eta > 0: the tables are built with eta = 0
        if sample_type != "ddim" or eta != 0:
            raise ValueError("DDIB runs the deterministic 'ddim' chain: sample_type = ddim and eta 0 or absent, got %r / %r"
                             % (sample_type, eta))

    def encode(self, image, class_label=None):
        x0 = ((image - 0.5) * 2.0).to(self.device, torch.float32)
        assert x0.shape[2] == x0.shape[3] == self.resolution
        xT = self.engine.ddim_invert(self.net, x0, self.sched.coef_invert())
        self._range_guard()
        return xT.reshape(x0.shape[0], -1)

    def generate(self, z, class_label):
        bsz = z.shape[0]
        zz = z.view(bsz, 1, self.channels, self.resolution, self.resolution).contiguous()
        x = self.engine.ddim_decode(self.net, _ffi.CD_SCHED_DDIM, zz, self.sched.coef_decode_eta0(), n_eps=0)
        x = self._refine(x)
        self._range_guard()
        return x


class DDPMSDEditWrapper(_NoCoupledLoop, DDPMDDIMWrapper):
    """gan_type = DDPM_SDEdit, key `sdedit_strengths` (a list of ONE value here - two pixel models have no ranker - shared by
    both sides). Source side: encode(image) =
    sample_xt(x0, t=seq[i_s]) with i_s = int(strength * (es_steps - 1)) - no network. Target side: forward(z) = generate()'s
    chain from index i_s down with fresh noise per step (the configured sample_type / eta), then refinement and post-process."""

    def __init__(self, source_model_type, sample_type, custom_steps, es_steps, sdedit_strengths, **kw):
        if len(sdedit_strengths) != 1:
            raise ValueError("DDPM_SDEdit takes one strength (no ranker across two pixel models), got %r" % (sdedit_strengths,))
        super().__init__(source_model_type, sample_type, custom_steps, es_steps, **kw)
        self.sdedit_strength = float(sdedit_strengths[0])
        self.i_s = self.sched.coef_sdedit(self.sdedit_strength)[0]
        self.latent_dim = self.resolution ** 2 * self.channels

    def encode(self, image, class_label=None):
        x0 = ((image - 0.5) * 2.0).to(self.device, torch.float32)
        assert x0.shape[2] == x0.shape[3] == self.resolution
        _i_s, start, _rows = self.sched.coef_sdedit(self.sdedit_strength)
        nz = self._randn(1, tuple(x0.shape))  # sample_xt's randn_like
        z = self.engine.dpm_encode(self.net, self.sched.kind, x0, start, noise=nz, last_uses_x0=False)
        return z.reshape(x0.shape[0], -1)

    def generate(self, z, class_label):
        bsz = z.shape[0]
        i_s, _start, rows = self.sched.coef_sdedit(self.sdedit_strength)
        zz = z.view(bsz, 1, self.channels, self.resolution, self.resolution).contiguous()
        nz = self._randn(i_s + 1, tuple(zz[:, 0].shape))  # one randn_like per denoising_step
        x = self.engine.ddim_decode(self.net, self.sched.kind, zz, rows, n_eps=0, noise_tail=nz)
        x = self._refine(x)
        self._range_guard()
        return x


class DDPMILVRWrapper(_NoCoupledLoop, DDPMDDIMWrapper):
    """gan_type = DDPM_ILVR, keys `ilvr_down_n` (N of the low-pass filter phi_N; divides the resolution, R / N >= 4) and
    `ilvr_range_t` (default 0: the steps of decode rows k > ilvr_range_t are conditioned, so only the last one is free).
    Source side: encode(image) = the image itself in [-1, 1] as [B, C*R*R] - no network. Target side: forward(z) = generate()'s
    chain from x_T ~ N(0, I) with fresh noise per step (the configured sample_type / eta) and the conditioning after each step,
    then refinement and post-process."""

    def __init__(self, source_model_type, sample_type, custom_steps, es_steps, ilvr_down_n, ilvr_range_t=0,
                 sdedit_strengths=None, skip_steps=None, white_box_steps=None, **kw):
        from ..utils import lowpass
        from .ddpm_ddim_wrapper import MODEL_TYPES, _desc
        _reject("ILVR", sdedit_strengths=sdedit_strengths, skip_steps=skip_steps, white_box_steps=white_box_steps)
        auto_mask.refuse(kw, "ILVR")
        attn_control.refuse_local_blend(kw, "ILVR")
        semantic_guidance.refuse(kw, "ILVR")
        windows.refuse(kw, "ILVR")
        for name, v, lo in (("ilvr_down_n", ilvr_down_n, 1), ("ilvr_range_t", ilvr_range_t, 0)):
            if isinstance(v, bool) or not isinstance(v, int) or v < lo:
                raise ValueError("%s must be an integer >= %d, got %r" % (name, lo, v))
        if source_model_type not in MODEL_TYPES:
            raise NotImplementedError(source_model_type)
        net_desc = kw.get("net_desc")
        res = (net_desc if net_desc is not None else _desc(MODEL_TYPES[source_model_type][0])).image_size
        lowpass.check_geometry(res, ilvr_down_n)  # before the engine and the weights exist
        super().__init__(source_model_type, sample_type, custom_steps, es_steps, **kw)
        self.ilvr_down_n, self.ilvr_range_t = ilvr_down_n, ilvr_range_t
        self.latent_dim = self.resolution ** 2 * self.channels

    def encode(self, image, class_label=None):
        assert image.shape[2] == image.shape[3] == self.resolution
        return ((image - 0.5) * 2.0).to(self.device, torch.float32).reshape(image.shape[0], -1)

    def generate(self, z, class_label):
        bsz, K = z.shape[0], self.es_steps
        y = z.view(bsz, self.channels, self.resolution, self.resolution).contiguous()
        xT = self._randn(1, tuple(y.shape))
        # per step: denoising_step's randn_like, then the draw that noises the reference (Algorithm 1's order)
        nz = self._randn(2 * K, tuple(y.shape))
        x = self.engine.ilvr_decode(self.net, self.sched.kind, xT.transpose(0, 1).contiguous(), self.sched.coef_decode(), y,
                                    self.ilvr_down_n, self.sched.coef_ilvr(), range_t=self.ilvr_range_t, n_eps=0,
                                    noise_tail=nz[0::2].contiguous(), ref_noise=nz[1::2].contiguous())
        x = self._refine(x)
        self._range_guard()
        return x


GAN_TYPES = {"SDDDIBText": SDDDIBTextWrapper, "LatentDiffDDIBText": LatentDiffDDIBTextWrapper,
             "SDSDEditText": SDSDEditTextWrapper, "LatentDiffSDEditText": LatentDiffSDEditTextWrapper,
             "DDPM_DDIB": DDPMDDIBWrapper, "DDPM_SDEdit": DDPMSDEditWrapper}
# the samplers that take the source IMAGE rather than a latent of a source model; get_gan_wrapper looks here after GAN_TYPES
SAMPLER_TYPES = {"DDPM_ILVR": DDPMILVRWrapper}
