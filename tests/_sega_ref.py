"""Torch restatement of semantic guidance (include/cyclediff.h cd_sega / cd_op_sega_guidance).
  guidance_step          one iteration's guidance on explicit tensors, in the operation order of the header, in the dtype of
                         its inputs (fp32: the bit-exact reference of cd_op_sega_guidance); order statistics from torch.sort
  coupled_translate_sega _attn_control_ref.coupled_translate extended by the concept rows, the guidance and the momentum
  E2E / e2e_*            the inputs the GPU end-to-end tests and the CPU discrimination tests share
"""
import contextlib

import torch
import torch.nn.functional as F

import _attn_control_ref as acr
import golden_util as gu
from cycle_diffusion_amd import semantic_guidance as sgm
from oracle import nets, samplers


def guidance_step(u, c, p, concepts, i, nu, g, s_m, beta):
    """u, c [Bd, ...], p [E, Bd, ...] network outputs; concepts: rows with fields scale, weight, lo, frac, warm, cool; g a
    scalar or [Bd]; nu [Bd, ...]. Returns (eps, nu_new, tau [Bd, E], kept [Bd, E] int32, mask [Bd, E, ...], ties [Bd, E] bool:
    the sorted |d| of that row holds equal neighbours). Inactive concepts: tau = kept = mask = 0."""
    dt = u.dtype
    f = lambda v: torch.as_tensor(float(v), dtype=dt)
    Bd, E = u.shape[0], len(concepts)
    N = u[0].numel()
    col = (Bd,) + (1,) * (u.dim() - 1)
    gs = torch.as_tensor(g, dtype=dt).reshape(col) if torch.is_tensor(g) or isinstance(g, (list, tuple)) else f(g)
    base = u + gs * (c - u)
    gamma = torch.zeros_like(u)
    tau = torch.zeros(Bd, E, dtype=dt)
    kept = torch.zeros(Bd, E, dtype=torch.int32)
    ties = torch.zeros(Bd, E, dtype=torch.bool)
    mask = torch.zeros((Bd, E) + tuple(u.shape[1:]), dtype=dt)
    for e, cp in enumerate(concepts):
        if not int(cp["warm"]) <= i < int(cp["cool"]):
            continue
        d = (p[e] - u) * f(cp["scale"])
        a = d.abs()
        A = torch.sort(a.flatten(1), dim=1).values
        lo = int(cp["lo"])
        hi = min(lo + 1, N - 1)
        t = A[:, lo] + (A[:, hi] - A[:, lo]) * f(cp["frac"])
        keep = a >= t.reshape(col)
        m = torch.where(keep, d, torch.zeros_like(d))
        gamma = gamma + f(cp["weight"]) * m
        tau[:, e] = t
        kept[:, e] = keep.flatten(1).sum(1).to(torch.int32)
        ties[:, e] = (A[:, 1:] == A[:, :-1]).any(1)
        mask[:, e] = keep.to(dt)
    gp = gamma + f(s_m) * nu
    nu_new = f(beta) * nu + (f(1.0) - f(beta)) * gp
    return base + gp, nu_new, tau, kept, mask, ties


@contextlib.contextmanager
def _network_in(dtype):
    """oracle.nets pins two places to fp32 whatever the weights are - the timestep embedding and the input of GroupNorm. Inside
    the context both follow `dtype` (replaced from the test side, as _attn_control_ref.controlled_mha replaces the attention),
    so that the network runs in float64 when its weights and inputs are float64; in fp32 nothing is replaced."""
    if dtype == torch.float32:
        yield
        return
    emb, gn = nets.timestep_embedding_cos_sin, nets._gn
    nets.timestep_embedding_cos_sin = lambda t, dim: emb(t, dim).to(dtype)
    nets._gn = lambda sd, p, x, eps: F.group_norm(x.to(dtype), 32, sd[p + ".weight"], sd[p + ".bias"], eps)
    try:
        yield
    finally:
        nets.timestep_embedding_cos_sin, nets._gn = emb, gn


def kept_rule(N, lo, frac):
    """#{a >= tau} on distinct values"""
    return N - lo if frac == 0 else N - min(lo + 1, N - 1)


def coupled_translate_sega(sd, cfg, x0, c_src, c_tgt, uc, dec_g, S, skip, eta, noises, edit_ctx=None, concepts=(), s_m=0.0,
                           beta=0.0, perturb=None):
    """acr.coupled_translate without a control, with E = len(concepts) concept rows per decoder row in the one forward of a
    step - batch rows [encoder cond | decoder uncond | concept 0 | ... | concept E-1 | decoder cond], edit_ctx [E * B, L, Dc]
    concept-major - and guidance_step between the forward and the decode step. No concepts: acr.coupled_translate line for line.
    perturb = (std_rel, generator): every forward's output gains Gaussian noise of standard deviation std_rel * its maximum.
    Returns (z list, x, info) with info = dict(tau [K, B, E], kept [K, B, E], ties [K, B, E], mask [B, E, C, H, W] of the last
    iteration with an active concept)."""
    _full = samplers._full
    ts, a, a_prev, sig, r = samplers.ddim_tables(samplers.sd_alphas_cumprod(), S, eta)
    K = len(ts) - skip
    B, E = x0.shape[0], len(concepts)
    ctx = torch.cat([c_src, uc] + ([edit_ctx] if E else []) + [c_tgt], 0)
    at = a[K - 1]
    xe = at.sqrt() * x0 + (1 - at).sqrt() * noises[0]
    xd = xe
    z = [xe]
    it = 1
    nu = torch.zeros_like(x0)
    info = dict(tau=torch.zeros(K, B, E, dtype=x0.dtype), kept=torch.zeros(K, B, E, dtype=torch.int32),
                ties=torch.zeros(K, B, E, dtype=torch.bool), mask=torch.zeros((B, E) + tuple(x0.shape[1:]), dtype=x0.dtype))
    for i in range(K):
        k = K - i - 1
        t = torch.full(((3 + E) * B,), int(ts[k]), dtype=torch.long)
        a_t, a_p, s_t, r_t = _full(B, a[k]), _full(B, a_prev[k]), _full(B, sig[k]), _full(B, r[k])
        if k == 0:
            x_next = x0
        else:
            e_post = (xe - a_t.sqrt() * x0) / (1 - a_t).sqrt()
            x_next = a_p.sqrt() * x0 + (1. - a_p - s_t ** 2).sqrt() * e_post + s_t * noises[it]
            it += 1
        with torch.no_grad(), _network_in(x0.dtype):
            e = nets.openai_unet(sd, cfg, torch.cat([xe] + [xd] * (2 + E), 0), t, ctx)
        if perturb is not None:
            e = e + torch.randn(e.shape, generator=perturb[1], dtype=e.dtype) * (perturb[0] * e.abs().max())
        e_enc, e_u, e_c = e[:B], e[B:2 * B], e[(2 + E) * B:]
        pred_x0 = (xe - r_t * e_enc) / a_t.sqrt()
        eps = (x_next - a_p.sqrt() * pred_x0 - (1. - a_p - s_t ** 2).sqrt() * e_enc) / s_t / 1.0
        z.append(eps)
        if E:
            p = e[2 * B:(2 + E) * B].reshape((E, B) + tuple(x0.shape[1:]))
            ed, nu, info["tau"][i], info["kept"][i], m, info["ties"][i] = guidance_step(e_u, e_c, p, concepts, i, nu, dec_g, s_m,
                                                                                       beta)
            if any(int(cp["warm"]) <= i < int(cp["cool"]) for cp in concepts):
                info["mask"] = m
        else:
            ed = e_u + dec_g * (e_c - e_u)
        pred_d = (xd - r_t * ed) / a_t.sqrt()
        xd = a_p.sqrt() * pred_d + (1. - a_p - s_t ** 2).sqrt() * ed + s_t * eps * 1.0
        xe = x_next
    return z, xd, info


# ---------------------------------------------------------------------------------------------------------- shared inputs
# acr.e2e_inputs() (tiny SD network, latent_cycle_tiny weights, latent 4 x 16 x 16 so N = 1024, B = 2, K = 20) with concept
# contexts drawn as N(0, 4^2), the scale e2e_inputs gives the prompts' contexts. Rows: (scale, weight, q, warm, cool).
E2E = dict(acr.E2E, s_m=0.3, beta=0.6, ctx_seed=100, N=1024, K=20)
SETS = {
    "q0": [(5.0, 1.0, 0.0, 2, 20)],
    "thr": [(5.0, 1.0, 0.9, 2, 20)],
    "two": [(5.0, 1.0, 0.9, 2, 20), (-4.0, 1.0, 0.8, 4, 16)],
}
# What the GPU end-to-end tests of the thresholded sets hold the engine to (tests/test_sega_host.py re-measures what they come
# from and asserts that they are no looser than that allows): the threshold is discontinuous - a cell that crosses it moves eps
# there by about tau - so a thresholded run is held to a PSNR floor and a cap on differing cells of the final mask, not to
# the maximum error. Perturbing every forward of the restatement by the engine's own end-to-end error on this network (5e-4
# of the maximum) gives 45.6 - 48.3 dB and at most 14 of 2048 differing cells (0.7 %) over three draws.
E2E_THR_DB = 42.0      # at least 3 dB below the worst of those, never below the 40 dB of the other end-to-end tests
E2E_MASK_DIFF = 0.02   # share of the final mask's cells; at least twice the worst of those, 2 % at most


def e2e_table(name):
    return sgm.table_rows(SETS[name], E2E["K"], E2E["N"])


def e2e_edit_ctx(name, B=2, n_dec=1):
    """[E * n_dec * B, 77, 64] concept-major: concept e's context is one draw per sample, shared by the ensemble members"""
    return torch.cat([gu.rnd((B, 77, 64), E2E["ctx_seed"] + e, E2E["ctx_scale"]).repeat(n_dec, 1, 1)
                      for e in range(len(SETS[name]))], 0)


def e2e_run(sd, x0, c, uc, c2, noise, name=None, dtype=None, s_m=None, perturb=None):
    """the restatement on the shared inputs; name = None: no concepts"""
    e = E2E
    cast = (lambda t: t.to(dtype)) if dtype is not None else (lambda t: t)
    if dtype is not None:
        sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    kw = {}
    if name is not None:
        kw = dict(edit_ctx=cast(e2e_edit_ctx(name)), concepts=e2e_table(name), s_m=e["s_m"] if s_m is None else s_m,
                  beta=e["beta"])
    return coupled_translate_sega(sd, gu.TINY_SD_CFG, cast(x0), cast(c), cast(c2), cast(uc), e["dec_g"], e["S"], e["skip"],
                                  e["eta"], [cast(n) for n in noise], perturb=perturb, **kw)
