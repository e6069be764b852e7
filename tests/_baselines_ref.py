"""CPU torch restatement of the four baseline loops (gan_wrapper/baselines.py), in the reference's fp32 operation order, on
any eps_hat callable. The tables come from the host schedules (cycle_diffusion_amd/schedule.py, pinned against the reference
by tests/test_schedule.py); every scalar enters as a [B, 1, 1, 1] fp32 tensor, as in the reference.

  latent DDIB    inversion: x0_hat = (x - sqrt(1-a_prev[j]) e)/sqrt(a_prev[j]); x <- sqrt(a[j]) x0_hat + sqrt(1-a[j]) e, e at the
                 input level's timestep (0, then tau[j-1]); decode: DDIMSampler.decode on an eta = 0 schedule
  latent SDEdit  stochastic_encode(z0, t_enc) then DDIMSampler.decode(t_start=t_enc) (ddim.py:648-681, 503-543)
  pixel DDIB     DiffusionCLIP's denoising_step(eta=0, 'ddim') up seq, then down the reversed pairs (diffusion_utils.py:23-136)
  pixel SDEdit   sample_xt(x0, seq[i_s]) then generate()'s chain from index i_s (ddpm_ddim_wrapper.py:310-314, 392-430)
"""
import numpy as np
import torch

from oracle import nets


def synth_weights(named_shapes, seed, out_prefix, out_scale):
    """oracle.nets.synth_state_dict with the tensors of the network's output layer (`out_prefix`) scaled by `out_scale`.
    The baseline fixtures need it: with the unscaled synthetic output layer, eps_hat of the random network changes so fast
    with t that DDIM inversion diverges (the reference's own round trip misses z0 by 12x its size), and a round-trip or
    16-bit check on it measures nothing. Scaled, the reference's round trip closes to a few % of |z0|."""
    sd = nets.synth_state_dict(named_shapes, seed)
    for k in sd:
        if k.startswith(out_prefix):
            sd[k] = sd[k] * out_scale
    return sd


def _full(v, B):
    return torch.full((B, 1, 1, 1), float(v), dtype=torch.float32)


def cfg_eps(unet, c, uc, g):
    """ddim.py:550-559: scale 1 -> conditional only, 0 -> unconditional only, else uncond + g * (cond - uncond)"""
    def f(x, t):
        tt = torch.full((x.shape[0],), int(t), dtype=torch.long)
        if uc is None or g == 1.0:
            return unet(x, tt, c)
        if g == 0.0:
            return unet(x, tt, uc)
        e_u, e_c = unet(torch.cat([x] * 2), torch.cat([tt] * 2), torch.cat([uc, c])).chunk(2)
        return e_u + g * (e_c - e_u)
    return f


# ---------------------------------------------------------------------------------------------------- latent
def latent_ddib_invert(eps, z0, sch, skip=0):
    """-> (x_T, [x_1 .. x_K]) over the K - skip steps of DDIMSchedule `sch`"""
    B = z0.shape[0]
    x, traj = z0, []
    for j in range(len(sch) - skip):
        t = 0 if j == 0 else int(sch.timesteps[j - 1])
        a_in, a_out = _full(sch.a_prev[j], B), _full(sch.a[j], B)
        e = eps(x, t)
        x0_hat = (x - (1. - a_in).sqrt() * e) / a_in.sqrt()
        x = a_out.sqrt() * x0_hat + (1. - a_out).sqrt() * e
        traj.append(x)
    return x, traj


def latent_decode(eps, x, sch, t_start, noises=None):
    """DDIMSampler.decode: indices t_start-1 .. 0 with p_sample_ddim (ddim.py:503-543); noises[i] is step i's noise_like
    draw (None: sigma must be 0 and no draw is needed)"""
    B = x.shape[0]
    for i in range(t_start):
        index = t_start - 1 - i
        e = eps(x, int(sch.timesteps[index]))
        a_t, a_prev = _full(sch.a[index], B), _full(sch.a_prev[index], B)
        sigma_t, sq1m = _full(sch.sigma[index], B), _full(sch.r[index], B)
        pred_x0 = (x - sq1m * e) / a_t.sqrt()
        dir_xt = (1. - a_prev - sigma_t ** 2).sqrt() * e
        n = torch.zeros_like(x) if noises is None else noises[i]
        x = a_prev.sqrt() * pred_x0 + dir_xt + sigma_t * n * 1.
    return x


def latent_sdedit_start(z0, sch, t_enc, noise):
    """stochastic_encode(z0, t_enc, noise) (ddim.py:648-661)"""
    B = z0.shape[0]
    return _full(np.sqrt(sch.a[t_enc]), B) * z0 + _full(sch.r[t_enc], B) * noise


# ---------------------------------------------------------------------------------------------------- pixel
def _acp(b):
    return (1.0 - b).cumprod(dim=0)


def _ddim_step(eps, x, t, t_next, b, eta=0.0, noise=None):
    """denoising_step(..., sampling_type='ddim') on a plain eps callable (diffusion_utils.py:23-136)"""
    B = x.shape[0]
    e = eps(x, t)
    at = _full(_acp(b)[t], B)
    at_next = torch.ones_like(at) if t_next == -1 else _full(_acp(b)[t_next], B)
    x0_t = (x - e * (1 - at).sqrt()) / at.sqrt()
    if eta == 0:
        return at_next.sqrt() * x0_t + (1 - at_next).sqrt() * e
    c1 = eta * ((1 - at / at_next) * (1 - at_next) / (1 - at)).sqrt()
    c2 = ((1 - at_next) - c1 ** 2).sqrt()
    return at_next.sqrt() * x0_t + c2 * e + c1 * noise


def _ddpm_step(eps, x, t, b, logvar, noise):
    """denoising_step(..., sampling_type='ddpm')"""
    B = x.shape[0]
    e = eps(x, t)
    bt, at = _full(b[t], B), _full(_acp(b)[t], B)
    weight = bt / torch.sqrt(1 - at)
    mean = 1 / torch.sqrt(1.0 - bt) * (x - weight * e)
    mask = 1 - float(t == 0)
    return mean + mask * torch.exp(0.5 * _full(logvar[t], B)) * noise


def pixel_ddib(eps_src, eps_tgt, x0, sched):
    """-> (x_T, x): inversion over (seq[k-1] -> seq[k]), then the eta = 0 decode over the reversed pairs"""
    b = torch.from_numpy(sched.b)
    x = x0
    for k in range(1, len(sched.seq)):
        x = _ddim_step(eps_src, x, sched.seq[k - 1], sched.seq[k], b)
    xT = x
    for i, j in zip(reversed(sched.seq), reversed(sched.seq_next)):
        x = _ddim_step(eps_tgt, x, i, j, b)
    return xT, x


def pixel_sdedit(eps_tgt, x0, sched, i_s, noise0, noises):
    """-> (x_t, x): sample_xt at seq[i_s], then the chain from index i_s with one fresh draw per step"""
    b = torch.from_numpy(sched.b)
    B = x0.shape[0]
    at = _full(_acp(b)[sched.seq[i_s]], B)
    x = at.sqrt() * x0 + (1 - at).sqrt() * noise0
    xt = x
    pairs = list(zip(reversed(sched.seq[:i_s + 1]), reversed(sched.seq_next[:i_s + 1])))
    for n, (i, j) in zip(noises, pairs):
        if sched.sample_type == "ddim":
            x = _ddim_step(eps_tgt, x, i, j, b, sched.eta, n)
        else:
            x = _ddpm_step(eps_tgt, x, i, b, sched.logvar, n)
    return xt, x
