"""Torch restatement of the cross-attention control (include/cyclediff.h cd_attn_ctrl), in its
literal form: P = w * (alpha * (P_src . M) + (1 - alpha) * P_own), O = P . V_own - NOT the engine's V_a / V_b form, so the
linear rewrite is under test too. Three layers:
  ctrl_attention_ref   one controlled cross-attention on explicit tensors (float64)
  controlled_mha       context manager: oracle.nets._mha replaced (from the test side) by a version that applies the control to
                       the text cross-attention calls of the stacked batch [encoder rows | decoder uncond | decoder cond]
  coupled_translate    the coupled DPM-Encoder / decode loop in oracle.samplers' arithmetic with n_ctrl gating
"""
import contextlib

import torch

from oracle import nets, samplers


def ctrl_attention_ref(q_own, q_src, k_own, k_src, v_own, M, alpha, w, H, scale):
    """q_own [B, Tq, C], q_src [B_src, Tq, C], k_own [B, L, C], k_src [B_src, L, C], v_own [B, L, C], M [B_ctrl, L, L],
    alpha / w [B_ctrl, L] -> [B, Tq, C] in float64; row b uses source b % B_src and control b % B_ctrl."""
    B, Tq, C = q_own.shape
    L, D = k_own.shape[1], C // H
    Bs, Bc = q_src.shape[0], M.shape[0]
    hs = lambda t: t.double().reshape(t.shape[0], t.shape[1], H, D).transpose(1, 2)
    src = torch.arange(B) % Bs
    ctl = torch.arange(B) % Bc
    p_own = torch.softmax(hs(q_own) @ hs(k_own).transpose(-1, -2) * scale, dim=-1)               # [B, H, Tq, L]
    p_src = torch.softmax(hs(q_src)[src] @ hs(k_src)[src].transpose(-1, -2) * scale, dim=-1)
    a = alpha.double()[ctl][:, None, None, :]
    ww = w.double()[ctl][:, None, None, :]
    p = ww * (a * (p_src @ M.double()[ctl][:, None]) + (1 - a) * p_own)
    return (p @ hs(v_own)).transpose(1, 2).reshape(B, Tq, C)


def random_control(g, Bc, L, fractional=False):
    """a permutation-with-holes mapper (every target column takes at most one source row, about a quarter take none), alpha in
    {0, 1} (or fractional), w in [0.5, 2]"""
    M = torch.zeros(Bc, L, L)
    alpha = torch.zeros(Bc, L)
    for b in range(Bc):
        perm = torch.randperm(L, generator=g)
        hole = torch.rand(L, generator=g) < 0.25
        for j in range(L):
            if not hole[j]:
                M[b, perm[j], j] = 1.0
                alpha[b, j] = 1.0
    if fractional:
        alpha = alpha * torch.rand(Bc, L, generator=g)
    w = 0.5 + 1.5 * torch.rand(Bc, L, generator=g)
    return M, alpha, w


# --------------------------------------------------------------------------------------------------------------- network
@contextlib.contextmanager
def controlled_mha(ctrl):
    """ctrl: None (the oracle's own attention) or dict(row0, rows, src_b0, B_src, M, alpha, w, L): inside the context every
    nets._mha call whose keys are the L context tokens and whose batch reaches row0 + rows - the text cross-attention of the
    stacked batch - takes the controlled probabilities for rows [row0, row0 + rows)."""
    if ctrl is None:
        yield
        return
    orig = nets._mha

    def mha(q, k, v, heads):
        B, Tq, C = q.shape
        if k.shape[1] != ctrl["L"] or k.shape[0] != ctrl["row0"] + ctrl["rows"] or Tq == k.shape[1]:
            return orig(q, k, v, heads)
        out = orig(q, k, v, heads).clone()  # every uncontrolled row: the oracle's own arithmetic
        D = C // heads
        hs = lambda t: t.reshape(t.shape[0], t.shape[1], heads, D).transpose(1, 2)
        r = torch.arange(ctrl["rows"])
        own = ctrl["row0"] + r
        src = ctrl["src_b0"] + r % ctrl["B_src"]
        ctl = (r % ctrl["B_src"]) % ctrl["M"].shape[0]
        p_own = torch.softmax(hs(q[own]) @ hs(k[own]).transpose(-1, -2) * D ** -0.5, dim=-1)  # [rows, H, Tq, L]
        p_src = torch.softmax(hs(q[src]) @ hs(k[src]).transpose(-1, -2) * D ** -0.5, dim=-1)
        a = ctrl["alpha"].to(q.dtype)[ctl][:, None, None, :]
        ww = ctrl["w"].to(q.dtype)[ctl][:, None, None, :]
        p = ww * (a * (p_src @ ctrl["M"].to(q.dtype)[ctl][:, None]) + (1 - a) * p_own)
        out[own] = (p @ hs(v[own])).transpose(1, 2).reshape(ctrl["rows"], Tq, C)
        return out

    nets._mha = mha
    try:
        yield
    finally:
        nets._mha = orig


def coupled_translate(sd, cfg, x0, c_src, c_tgt, uc, dec_g, S, skip, eta, noises, ctrl=None, n_ctrl=0):
    """The coupled loop of cd_cycle_translate (cd_attn_ctrl) on the oracle network, encoder guidance 1 and a guided decoder: one
    forward per step over [encoder cond | decoder uncond | decoder cond], then the DPM-Encoder step and the decode step on the
    eps it just recorded - the arithmetic of oracle.samplers.latent_encode / latent_decode, line for line. noises: the list
    latent_encode takes. ctrl = (M, alpha, w), applied on iterations i < n_ctrl. Returns (z list, x)."""
    _full = samplers._full
    ts, a, a_prev, sig, r = samplers.ddim_tables(samplers.sd_alphas_cumprod(), S, eta)
    K = len(ts) - skip
    B, L = x0.shape[0], c_src.shape[1]
    ctx = torch.cat([c_src, uc, c_tgt], 0)
    desc = None
    if ctrl is not None:
        desc = dict(row0=2 * B, rows=B, src_b0=0, B_src=B, M=ctrl[0], alpha=ctrl[1], w=ctrl[2], L=L)
    at = a[K - 1]
    xe = at.sqrt() * x0 + (1 - at).sqrt() * noises[0]
    xd = xe
    z = [xe]
    it = 1
    for i in range(K):
        k = K - i - 1
        t = torch.full((3 * B,), int(ts[k]), dtype=torch.long)
        a_t, a_p, s_t, r_t = _full(B, a[k]), _full(B, a_prev[k]), _full(B, sig[k]), _full(B, r[k])
        if k == 0:
            x_next = x0
        else:
            e_post = (xe - a_t.sqrt() * x0) / (1 - a_t).sqrt()
            x_next = a_p.sqrt() * x0 + (1. - a_p - s_t ** 2).sqrt() * e_post + s_t * noises[it]
            it += 1
        with torch.no_grad(), controlled_mha(desc if i < n_ctrl else None):
            e = nets.openai_unet(sd, cfg, torch.cat([xe, xd, xd], 0), t, ctx)
        e_enc, e_u, e_c = e[:B], e[B:2 * B], e[2 * B:]
        pred_x0 = (xe - r_t * e_enc) / a_t.sqrt()
        eps = (x_next - a_p.sqrt() * pred_x0 - (1. - a_p - s_t ** 2).sqrt() * e_enc) / s_t / 1.0
        z.append(eps)
        ed = e_u + dec_g * (e_c - e_u)
        pred_d = (xd - r_t * ed) / a_t.sqrt()
        xd = a_p.sqrt() * pred_d + (1. - a_p - s_t ** 2).sqrt() * ed + s_t * eps * 1.0
        xe = x_next
    return z, xd


# the inputs the GPU end-to-end test and the CPU discrimination test share (tiny SD network, latent_cycle_tiny weights)
E2E = dict(S=50, skip=30, eta=0.1, dec_g=3.0, n_ctrl=8, noise_seed=77, ctx_scale=4.0)


def e2e_inputs():
    """(x0, c_src, uc, c_tgt): golden_util.latent_cycle_inputs with both prompts' contexts scaled by E2E["ctx_scale"]. At unit
    scale the synthetic network's cross-attention scores are far below 1, every softmax is nearly uniform, P_src and P_own are
    the same flat map and a control has nothing to move (controlled and uncontrolled restatement 1.0e-2 of the maximum apart).
    A context of standard deviation 4 gives the peaked, prompt-dependent maps a trained text encoder's outputs give; the two
    runs are then 1.8e-1 apart (tests/test_attn_control_host.py asserts at least 8e-2). The unconditional context is left."""
    import golden_util as gu
    x0, c, uc, c2 = gu.latent_cycle_inputs()
    return x0, c * E2E["ctx_scale"], uc, c2 * E2E["ctx_scale"]


def e2e_control(L=77, Bc=2):
    """a refine-style control: identity mapper over the whole context with two holes (positions that keep their own map)"""
    M = torch.eye(L).repeat(Bc, 1, 1)
    alpha = torch.ones(Bc, L)
    for b, holes in enumerate(((2, 5), (3, 4))[:Bc]):
        for j in holes:
            M[b, j, j] = 0.0
            alpha[b, j] = 0.0
    return M, alpha, torch.ones(Bc, L)
