"""CPU torch restatement of the region-keeping decode, DDIMSampler.ddim_sampling_with_eps(mask=, x0=) (ddim.py:395-448; the
branch at :427-430), in the reference's fp32 operation order, on any eps_hat callable - and the pieces the masked tests share.
Every scalar enters as a [B, 1, 1, 1] fp32 tensor, as in the reference. Tables come from the host schedule
(cycle_diffusion_amd/schedule.py, pinned against the reference by tests/test_schedule.py and tests/test_masked_host.py).

  blend          img = img_orig * mask + (1. - mask) * img                                   (ddim.py:430)
  q_sample       extract(sqrt_alphas_cumprod, t) * x_start + extract(sqrt_one_minus_alphas_cumprod, t) * noise
                 (ddpm.py:271-274) over the buffers of register_schedule (ddpm.py:141-142)
  step           p_sample_ddim_with_eps (ddim.py:603-646), as tests/_baselines_ref.latent_decode writes it
"""
import json
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLD, "masked_latent.npz")


def load_fixture():
    return np.load(FIXTURE, allow_pickle=False)


def params(fx):
    return json.loads(str(fx["params"]))


def _full(v, B):
    return torch.full((B, 1, 1, 1), float(v), dtype=torch.float32)


def qsample_buffers(timesteps=1000, linear_start=0.00085, linear_end=0.0120):
    """register_schedule's expressions for the two q-sample buffers (ddpm.py:117-142, 'linear' betas of util.py:21-37):
    to_torch(np.sqrt(alphas_cumprod)), to_torch(np.sqrt(1. - alphas_cumprod)) with to_torch = float32"""
    betas = (torch.linspace(linear_start ** 0.5, linear_end ** 0.5, timesteps, dtype=torch.float64) ** 2).numpy()
    alphas_cumprod = np.cumprod(1. - betas, axis=0)
    return (torch.tensor(np.sqrt(alphas_cumprod), dtype=torch.float32),
            torch.tensor(np.sqrt(1. - alphas_cumprod), dtype=torch.float32))


def q_sample(x_start, t, noise, buffers=None):
    """the two-line formula of ddpm.py:271-274; t [B] long"""
    sa, s1a = buffers or qsample_buffers()
    ex = lambda a: a.gather(-1, t).reshape(t.shape[0], 1, 1, 1)
    return ex(sa) * x_start + ex(s1a) * noise


def blend(src, mask, x):
    return src * mask + (1. - mask) * x


def decode_step(x, e, row, eps):
    """one p_sample_ddim_with_eps on a host table row (sa, s1a, sap, dirc, sigma, r, ...): the arithmetic of the engine's
    decode kernel, already held bit-exact against the reference's expressions by tests/test_gpu_ops.py"""
    B = x.shape[0]
    pred_x0 = (x - _full(row["r"], B) * e) / _full(row["sa"], B)
    return _full(row["sap"], B) * pred_x0 + _full(row["dirc"], B) * e + _full(row["sigma"], B) * eps


def masked_decode(eps_fn, z, coef, qcoef, mask, x0, mask_noise):
    """sample_with_eps(mask=, x0=) over the K rows of `coef` (DDIMSchedule.coef_decode) and `qcoef` (coef_qsample):
    z [B, K+1, C, h, w], eps_fn(x, t) -> guided eps_hat, mask [B, 1, h, w], mask_noise [K, B, C, h, w] in loop order"""
    B, K = z.shape[0], len(coef)
    x = z[:, 0]
    for i in range(K):
        k = K - 1 - i
        src = _full(qcoef[k, 0], B) * x0 + _full(qcoef[k, 1], B) * mask_noise[i]
        x = blend(src, mask, x)
        x = decode_step(x, eps_fn(x, int(coef["t"][k])), coef[k], z[:, 1 + i])
    return x


def encoder_trajectory(x0, coef_enc, noise):
    """the DPM-Encoder's x_t of every level, which does not depend on the network (sample_xt_next, ddim.py:582-601; x_T at
    :477-479): -> list indexed by level k = K-1 .. 0 as {k: x_t}. coef_enc K+1 rows, noise [K, B, C, h, w]."""
    B, K = x0.shape[0], len(coef_enc) - 1
    r = coef_enc[K]
    x = _full(r["sa"], B) * x0 + _full(r["s1a"], B) * noise[0]
    traj = {K - 1: x}
    for i in range(K - 1):
        k = K - 1 - i
        r = coef_enc[k]
        et = (x - _full(r["sa"], B) * x0) / _full(r["s1a"], B)
        x = _full(r["sap"], B) * x0 + _full(r["dirc"], B) * et + _full(r["sigma"], B) * noise[1 + i]
        traj[k - 1] = x
    return traj


def fixture_masks(B=2, R=64):
    """the fixture's pixel masks: sample 0 a hard rectangle, sample 1 a feathered ramp strictly inside (0, 1)"""
    m = torch.zeros(B, 1, R, R)
    m[0, 0, R // 4:3 * R // 4, R // 8:R // 2] = 1.0
    ramp = torch.linspace(0.05, 0.95, R)
    m[1, 0] = ramp[None, :].expand(R, R)
    return m


def block_mean(mask, f):
    return torch.nn.functional.avg_pool2d(mask, f)
