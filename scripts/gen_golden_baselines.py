"""Generate tests/golden/baselines_*.npz: the DDIB and SDEdit baselines (gan_wrapper/baselines.py) run through the
REFERENCE's own functions on the small networks of the other fixtures, CPU fp32.

  latent SDEdit  DDIMSampler.stochastic_encode + DDIMSampler.decode (ddim.py:648-681), p_sample_ddim inside
  latent DDIB    DDIMSampler.decode on a ddim_eta = 0 schedule; the inversion has no reference function: it is the
                 restatement in tests/_baselines_ref.py on the reference sampler's own tables, checked step by step
                 against denoising_step on the SD betas by tests/test_baselines_host.py
  pixel DDIB     denoising_step(eta=0, 'ddim') up generate()'s seq_inv, then down its reversed pairs
  pixel SDEdit   sample_xt + denoising_step (ddpm_ddim_wrapper.py:310-314; diffusion_utils.py:23-136)

Run where the reference tree is mounted:   python scripts/gen_golden_baselines.py
Each file holds tensors, the (name, shape) lists of the weights and the seeds only; inputs and weights are rebuilt from
those (oracle.nets.synth_state_dict, torch.Generator seeds). TEST INFRASTRUCTURE ONLY.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import gen_golden as gg, ref_import  # noqa: E402
import _baselines_ref as br  # noqa: E402

# The synthetic networks get a down-scaled output layer (`out_scale`, tests/_baselines_ref.synth_weights): unscaled, DDIM
# inversion of a random network diverges and the DDIB round trip reconstructs nothing. With these settings the reference's own
# round trip closes to 1.2 % (latent, sampled posterior; 6.7 % on the smaller posterior mean) and 2 % (pixel) of max|x0|.
# the latent setting: tiny SD U-Net + tiny KL VAE (64 px -> 16 x 16 latents), 50 DDIM steps
LAT = dict(S=50, eta=0.1, enc_scale=1.0, dec_scale=3.0, strength=0.5, B=2, unet_seed=121, vae_seed=122, image_seed=123,
           ctx_seeds=[124, 125, 126], noise_seed=127, out_prefix="out.2.", out_scale=0.01)
# the pixel setting: two toy Ho-DDPMs (32 px), 40-step schedule, the first 20 (es_steps, as C5's 850 of 1000), 'ddim' eta 0.1
# for SDEdit
PIX = dict(custom_steps=40, es_steps=20, eta=0.1, strength=0.5, src_seed=106, tgt_seed=108, image_seed=131, noise_seed=132,
           out_prefix="conv_out.", out_scale=0.1)


def load_scaled(module, seed, p):
    ns = gg.named_shapes(module)
    module.load_state_dict(br.synth_weights(ns, seed, p["out_prefix"], p["out_scale"]))
    module.eval()
    return ns


class RefTables:
    """the reference DDIMSampler's tables in the attribute names of the restatement"""

    def __init__(self, sampler):
        self.timesteps = np.asarray(sampler.ddim_timesteps)
        self.a = sampler.ddim_alphas.numpy()
        self.a_prev = np.asarray(sampler.ddim_alphas_prev)
        self.sigma = np.asarray(sampler.ddim_sigmas, dtype=np.float64)
        self.r = np.asarray(sampler.ddim_sqrt_one_minus_alphas)

    def __len__(self):
        return len(self.timesteps)


def latent_contexts(seeds, B):
    """(c_src, c_tgt, uc) [B, 77, 64]: per-sample source / target rows, one shared unconditional row"""
    c_src, c_tgt = gg.rnd((B, 77, 64), seeds[0]), gg.rnd((B, 77, 64), seeds[1])
    uc = gg.rnd((1, 77, 64), seeds[2]).expand(B, 77, 64).contiguous()
    return c_src, c_tgt, uc


def gen_latent():
    from ldm.modules.distributions.distributions import DiagonalGaussianDistribution
    Sampler = ref_import.ddim_sampler_cls()
    p = LAT
    S, B = p["S"], p["B"]
    u = gg.build_ref_sd_unet()
    uns = load_scaled(u, p["unet_seed"], p)
    vae = gg.RefVAE()
    vns, _ = gg.load_synth(vae, p["vae_seed"])
    shim = ref_import.LatentShim(u)
    c_src, c_tgt, uc = latent_contexts(p["ctx_seeds"], B)
    image = torch.rand((B, 3, 64, 64), generator=torch.Generator().manual_seed(p["image_seed"]))
    unet = lambda x, t, c: u(x, t, context=c)
    out = {}
    with torch.no_grad(), ref_import.quiet():
        mom = vae.moments((image - 0.5) * 2.0)
        for mode in ("sd", "ldm"):  # first stage: posterior sample (SD) / mean (LDM)
            torch.manual_seed(p["noise_seed"])
            post = DiagonalGaussianDistribution(mom)
            z0 = (post.sample() if mode == "sd" else post.mode()) * 0.18215
            # SDEdit: the draws continue from the posterior's: randn_like(z0), then one noise_like per decode step (ddim.py:537)
            t_enc = int(p["strength"] * S)
            smp = Sampler(shim)
            smp.make_schedule(S, ddim_eta=p["eta"], verbose=False)
            noise = torch.randn_like(z0)
            zt = smp.stochastic_encode(z0, torch.full((B,), t_enc, dtype=torch.long), noise=noise)
            x_sde = smp.decode(zt, c_tgt, t_enc, unconditional_guidance_scale=p["dec_scale"], unconditional_conditioning=uc)
            # DDIB: inversion on the eta = 0 sampler's tables (source text, encoder scale), decode under the target
            smp0 = Sampler(shim)
            smp0.make_schedule(S, ddim_eta=0.0, verbose=False)
            tab = RefTables(smp0)
            xT, traj = br.latent_ddib_invert(br.cfg_eps(unet, c_src, uc, p["enc_scale"]), z0, tab)
            x_ddib = smp0.decode(xT, c_tgt, S, unconditional_guidance_scale=p["dec_scale"], unconditional_conditioning=uc)
            # the round trip: the same text and scale 1 both ways
            x_rt = smp0.decode(xT, c_src, S, unconditional_guidance_scale=1.0, unconditional_conditioning=uc) \
                if p["enc_scale"] == 1.0 else None
            img = lambda x: (vae.decode(x / 0.18215) + 1.0) / 2.0
            out.update({mode + "_z0": z0, mode + "_ddib_xT": xT, mode + "_ddib_x": x_ddib, mode + "_ddib_img": img(x_ddib),
                        mode + "_sdedit_zt": zt, mode + "_sdedit_x": x_sde, mode + "_sdedit_img": img(x_sde),
                        mode + "_rt_err_max": (x_rt - z0).abs().max(), mode + "_rt_err_rms": (x_rt - z0).pow(2).mean().sqrt()})
            if mode == "sd":
                out["sd_ddib_traj"] = torch.stack(traj, 0)
                # the reference sampler's tables, to which the host schedule rows are pinned
                out.update(ref_t=tab.timesteps, ref_a=tab.a, ref_a_prev=tab.a_prev.astype(np.float32),
                           ref_sigma_eta=np.asarray(smp.ddim_sigmas, dtype=np.float32))
    gg.save("baselines_latent", unet_names=json.dumps(uns), vae_names=json.dumps(vns), params=json.dumps(LAT), **out)


def pixel_seq(custom_steps, es_steps, t_0=999):
    """generate()'s seq_inv / seq_inv_next (ddpm_ddim_wrapper.py:392-399)"""
    if (t_0 + 1) % custom_steps == 0:
        seq = range(0, t_0 + 1, (t_0 + 1) // custom_steps)
    else:
        seq = np.linspace(0, 1, custom_steps) * t_0
    seq = [int(s) for s in list(seq)][:es_steps]
    return seq, ([-1] + list(seq[:-1]))[:es_steps]


def gen_pixel():
    import model.gan_wrapper.ddpm_ddim_wrapper as W
    p = PIX
    src, tgt = gg.build_ref_ho(), gg.build_ref_ho()
    sns = load_scaled(src, p["src_seed"], p)
    tns = load_scaled(tgt, p["tgt_seed"], p)
    w = gg.build_ref_pixel_wrapper(tgt, custom_steps=p["custom_steps"], es_steps=p["es_steps"], eta=p["eta"])
    seq, seq_next = pixel_seq(p["custom_steps"], p["es_steps"])
    img = torch.rand((1, 3, 32, 32), generator=torch.Generator().manual_seed(p["image_seed"]))
    x0 = (img - 0.5) * 2.0
    kw = dict(logvars=w.logvar, b=w.betas, learn_sigma=False)
    T = lambda v: torch.ones(1) * v
    with torch.no_grad(), ref_import.quiet():
        x = x0
        for k in range(1, len(seq)):  # DiffusionCLIP's inversion (t = seq[k-1] -> t_next = seq[k])
            x = W.denoising_step(x, t=T(seq[k - 1]), t_next=T(seq[k]), models=src, sampling_type="ddim", eta=0.0, **kw)
        xT = x
        for i, j in zip(reversed(seq), reversed(seq_next)):
            x = W.denoising_step(x, t=T(i), t_next=T(j), models=tgt, sampling_type="ddim", eta=0.0, **kw)
        x_ddib = x
        x = xT  # the DDIB round trip on the source model
        for i, j in zip(reversed(seq), reversed(seq_next)):
            x = W.denoising_step(x, t=T(i), t_next=T(j), models=src, sampling_type="ddim", eta=0.0, **kw)
        rt = x
        i_s = int(p["strength"] * (p["es_steps"] - 1))
        torch.manual_seed(p["noise_seed"])
        xt = W.sample_xt(x0=x0, t=T(seq[i_s]), b=w.betas)
        x = xt
        for i, j in zip(reversed(seq[:i_s + 1]), reversed(seq_next[:i_s + 1])):
            x = W.denoising_step(x, t=T(i), t_next=T(j), models=tgt, sampling_type="ddim", eta=p["eta"], **kw)
        x_sde = x
    gg.save("baselines_pixel", src_names=json.dumps(sns), tgt_names=json.dumps(tns), params=json.dumps(PIX),
            ddib_xT=xT, ddib_x=x_ddib, ddib_img=(x_ddib + 1.0) / 2.0, sdedit_xt=xt, sdedit_x=x_sde,
            sdedit_img=(x_sde + 1.0) / 2.0, seq=np.asarray(seq),
            rt_err_max=(rt - x0).abs().max(), rt_err_rms=(rt - x0).pow(2).mean().sqrt(), i_s=i_s)


if __name__ == "__main__":
    with ref_import.session():
        gen_latent()
        gen_pixel()
