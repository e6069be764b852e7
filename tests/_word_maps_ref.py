"""Torch restatement of the per-word cross-attention maps (include/cyclediff.h cd_word_maps / cd_op_cross_attention_maps,
DESIGN.md 17). Three layers:
  maps_ref64       one launch of the map kernel on explicit tensors, in float64
  collecting_mha   context manager: oracle.nets._mha replaced (from the test side) by a version that also records, for every
                   text cross-attention call in the side window, the head-mean softmax mass on the selector's key positions
  word_maps_ref    the whole call on the oracle network: noising, one conditional forward per draw, the layer / draw mean and
                   the nearest replication onto the latent grid
"""
import contextlib
import math

import torch

from oracle import nets

STREAM0 = 0x8000  # draw i of cd_word_maps is Philox stream STREAM0 + i (the band at 0x7000 holds the VAE posterior's 0x7a65)
TINY_SIDES = {16: 3, 8: 4}  # text cross-attention blocks of the tiny SD network by token grid side, from its description:
#   channel_mult (1, 2), one ResBlock per level, attention at both levels -> 16 x 16: one input block and two output blocks;
#   8 x 8: one input block, the middle block and two output blocks


def maps_ref64(q, k, sel, H, scale, log2=False):
    """q [B, Tq, C], k [B, L, C], sel [B_sel, N, L] -> [B, N, Tq] float64: (1/H) sum_hd sum_j sel[b % B_sel, n, j] P_hd[q, j].
    log2: q already carries scale * log2(e), the softmax is taken in base 2."""
    B, Tq, C = q.shape
    D = C // H
    hs = lambda t: t.double().reshape(t.shape[0], t.shape[1], H, D).transpose(1, 2)
    s = hs(q) @ hs(k).transpose(-1, -2) * (math.log(2.0) if log2 else scale)
    p = torch.softmax(s, dim=-1)                                   # [B, H, Tq, L]
    w = sel.double()[torch.arange(B) % sel.shape[0]]               # [B, N, L]
    return torch.einsum("bhqj,bnj->bnq", p, w) / H


@contextlib.contextmanager
def collecting_mha(sel, B, L, sides, out):
    """inside the context every nets._mha call whose keys are the L context tokens (and whose queries are not) appends
    m_layer [rows, N, Tq] (float64) to `out` when its token grid side lies in sides = (min, max) ((0, 0): every call); the
    attention output is the oracle's own. Row r uses selector entry (r % B) % B_sel."""
    orig = nets._mha

    def mha(q, k, v, heads):
        rows, Tq, _ = q.shape
        side = int(round(math.sqrt(Tq)))
        if k.shape[1] == L and Tq != L and (tuple(sides) == (0, 0) or sides[0] <= side <= sides[1]):
            w = sel[(torch.arange(rows) % B) % sel.shape[0]]
            out.append(maps_ref64(q, k, w, heads, (q.shape[2] // heads) ** -0.5))
        return orig(q, k, v, heads)

    nets._mha = mha
    try:
        yield
    finally:
        nets._mha = orig


def word_maps_ref(sd, cfg, x0, ctx, sel, t, qa, qb, noise, sides=(0, 0)):
    """(maps [B, N, h, w] float64, n_layers) of cd_word_maps on the oracle network (fp32 forward, float64 maps)"""
    B, _, h, w = x0.shape
    n = noise.shape[0]
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    x = (f32(qa) * x0)[None] + f32(qb) * noise  # [n, B, C, h, w]: qa*x0, qb*n_i, then the add
    layers = []
    with torch.no_grad(), collecting_mha(sel, B, ctx.shape[1], sides, layers):
        nets.openai_unet(sd, cfg, x.reshape(n * B, *x0.shape[1:]), torch.full((n * B,), int(t), dtype=torch.long),
                         ctx.repeat(n, 1, 1))
    total = torch.zeros(B, sel.shape[1], h, w, dtype=torch.float64)
    for m in layers:
        s = int(round(math.sqrt(m.shape[2])))
        up = m.reshape(n, B, -1, s, s).repeat_interleave(h // s, 3).repeat_interleave(w // s, 4)
        total += up.sum(0)
    return total / (n * len(layers)), len(layers)


# the inputs the GPU end-to-end test and the CPU discrimination test share (tiny SD network, latent_cycle_tiny weights)
E2E = dict(S=12, strength=0.5, eta=0.1, n_draws=2, noise_seed=31, ctx_scale=4.0, keys=(3, 11))


def e2e_inputs():
    """(x0, ctx, noise [n_draws, B, C, h, w], (t, qa, qb)): the latent and the first prompt's context of
    _attn_control_ref.e2e_inputs() - contexts at standard deviation 4, where the synthetic network's softmaxes are peaked and
    depend on the key (at unit scale every map is the constant |sel| / L and any kernel passes) - rescaled to
    E2E["ctx_scale"] should that differ, and the level a 12-step schedule picks at strength 0.5."""
    import _attn_control_ref as acr
    from cycle_diffusion_amd import auto_mask, schedule
    x0, c, _uc, _c2 = acr.e2e_inputs()
    c = c * (E2E["ctx_scale"] / acr.E2E["ctx_scale"])
    noise = torch.randn((E2E["n_draws"],) + tuple(x0.shape), generator=torch.Generator().manual_seed(E2E["noise_seed"]))
    sch = schedule.DDIMSchedule(schedule.latent_alphas_cumprod(), E2E["S"], E2E["eta"])
    k = auto_mask.level_index(E2E["strength"], len(sch))
    qa, qb = (float(v) for v in sch.coef_qsample(0)[k])
    return x0, c, noise, (int(sch.coef_decode(0)["t"][k]), qa, qb)


def one_key(j, L=77):
    """selector [1, 1, L] of the single key position j"""
    s = torch.zeros(1, 1, L)
    s[0, 0, j] = 1.0
    return s
