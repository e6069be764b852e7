"""Generate tests/golden/masked_latent.npz: the region-keeping decode run through the REFERENCE's own functions on the small
networks of tests/golden/baselines_latent.npz (tiny SD-shaped U-Net with the scaled output layer + tiny KL VAE, 64 px -> 16 x 16
latents, S = 50, eta 0.1, encoder scale 1, decoder scale 3, B = 2), CPU fp32:

  DDIMSampler.ddpm_ddim_encoding on the first-stage encoding encode() uses (SD: the sampled posterior, LDM: its mean), then
  DDIMSampler.sample_with_eps(mask=, x0=) with x0 = the scaled posterior MEAN (what forward(mask=) re-encodes) - ddim.py:427-430

oracle.ref_import's LatentShim gets a q_sample here: LatentDiffusion's own method where ddpm.py imports under the stubs, else
the two-line formula of ddpm.py:271-274; either way over buffers built as ddpm.py:141-142 (tests/_masked_ref.py checks that
formula against register_schedule's expressions). Masks: sample 0 a hard rectangle, sample 1 a feathered ramp, both at pixel
resolution; the latent mask is their 4 x 4 block mean (the tiny VAE's factor).

Run where the reference tree is mounted:   python scripts/gen_golden_masked.py
The file holds tensors, the (name, shape) lists of the weights and the seeds only. TEST INFRASTRUCTURE ONLY.
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from oracle import gen_golden as gg, ref_import  # noqa: E402
import _masked_ref as mr  # noqa: E402
import gen_golden_baselines as gb  # noqa: E402

P = dict(gb.LAT, mask_noise_seed=128)


def give_q_sample(shim):
    """-> which q_sample the shim got: 'reference' (LatentDiffusion.q_sample itself) or 'formula'"""
    ac = shim.alphas_cumprod  # fp32 buffer; the square roots come from the fp64 cumprod (ddpm.py:141-142)
    from ldm.modules.diffusionmodules.util import make_beta_schedule
    betas = make_beta_schedule("linear", shim.num_timesteps, linear_start=0.00085, linear_end=0.0120)
    ac64 = np.cumprod(1. - betas, axis=0)
    assert np.array_equal(ac64.astype(np.float32), ac.numpy())
    shim.sqrt_alphas_cumprod = torch.tensor(np.sqrt(ac64), dtype=torch.float32)
    shim.sqrt_one_minus_alphas_cumprod = torch.tensor(np.sqrt(1. - ac64), dtype=torch.float32)
    try:
        with ref_import.quiet():
            from ldm.models.diffusion.ddpm import DDPM
        shim.q_sample = types.MethodType(DDPM.q_sample, shim)
        return "reference"
    except Exception as e:  # noqa: BLE001
        print("ddpm.py does not import under the stubs (%s: %s): q_sample is the two-line formula" % (type(e).__name__, e))
        shim.q_sample = lambda x_start, t, noise=None: mr.q_sample(
            x_start, t, torch.randn_like(x_start) if noise is None else noise,
            (shim.sqrt_alphas_cumprod, shim.sqrt_one_minus_alphas_cumprod))
        return "formula"


def gen():
    from ldm.modules.distributions.distributions import DiagonalGaussianDistribution
    Sampler = ref_import.ddim_sampler_cls()
    p = P
    S, B = p["S"], p["B"]
    u = gg.build_ref_sd_unet()
    uns = gb.load_scaled(u, p["unet_seed"], p)
    vae = gg.RefVAE()
    vns, _ = gg.load_synth(vae, p["vae_seed"])
    shim = ref_import.LatentShim(u)
    kind = give_q_sample(shim)
    c_src, c_tgt, uc = gb.latent_contexts(p["ctx_seeds"], B)
    image = torch.rand((B, 3, 64, 64), generator=torch.Generator().manual_seed(p["image_seed"]))
    mask_px = mr.fixture_masks(B, 64)
    mask_lat = mr.block_mean(mask_px, 4)
    assert 0 < mask_px[1].min() and mask_px[1].max() < 1
    out = {}
    with torch.no_grad(), ref_import.quiet():
        mom = vae.moments((image - 0.5) * 2.0)
        for mode in ("sd", "ldm"):
            torch.manual_seed(p["noise_seed"])
            post = DiagonalGaussianDistribution(mom)
            z0 = (post.sample() if mode == "sd" else post.mode()) * 0.18215
            z0_mean = post.mode() * 0.18215
            z_list = Sampler(shim).ddpm_ddim_encoding(S, batch_size=B, shape=(4, 16, 16), conditioning=c_src, eta=p["eta"],
                                                      white_box_steps=S + 1, skip_steps=0, verbose=False, x0=z0,
                                                      unconditional_guidance_scale=p["enc_scale"],
                                                      unconditional_conditioning=uc)
            z = torch.stack(z_list, dim=1)
            torch.manual_seed(p["mask_noise_seed"])  # q_sample: randn_like(x0) at the top of every step, K draws in loop order
            x, _ = Sampler(shim).sample_with_eps(S, z[:, 1:], conditioning=c_tgt, batch_size=B, shape=(4, 16, 16), eta=p["eta"],
                                                 verbose=False, x_T=z[:, 0], skip_steps=0,
                                                 unconditional_guidance_scale=p["dec_scale"], unconditional_conditioning=uc,
                                                 mask=mask_lat, x0=z0_mean)
            x_plain, _ = Sampler(shim).sample_with_eps(S, z[:, 1:], conditioning=c_tgt, batch_size=B, shape=(4, 16, 16),
                                                       eta=p["eta"], verbose=False, x_T=z[:, 0], skip_steps=0,
                                                       unconditional_guidance_scale=p["dec_scale"],
                                                       unconditional_conditioning=uc)
            out.update({mode + "_z0": z0, mode + "_z0_mean": z0_mean, mode + "_z_sub": z[:, [0, 1, 25, 50]],
                        mode + "_x": x,
                        mode + "_img": (vae.decode(x / 0.18215) + 1.0) / 2.0,
                        mode + "_mask_effect": (x - x_plain).abs().max()})
            if mode == "sd":
                out["sd_eps"] = z  # the whole z of one family: the host replay of tests/test_masked_host.py decodes it
        smp = Sampler(shim)
        smp.make_schedule(S, ddim_eta=p["eta"], verbose=False)
        ts = np.asarray(smp.ddim_timesteps)
        qcoef = np.stack([shim.sqrt_alphas_cumprod.numpy()[ts], shim.sqrt_one_minus_alphas_cumprod.numpy()[ts]], 1)
    gg.save("masked_latent", unet_names=json.dumps(uns), vae_names=json.dumps(vns), params=json.dumps(dict(P, q_sample=kind)),
            mask_pixel=mask_px, mask_latent=mask_lat, qcoef=qcoef, timesteps=ts, **out)


if __name__ == "__main__":
    with ref_import.session():
        gen()
