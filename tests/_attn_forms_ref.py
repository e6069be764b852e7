"""The attention kernels in the operand forms the networks launch: case table, seeded inputs and the float64 reference for
tests/test_attn_forms_host.py (CPU) and tests/test_gpu_attention_forms.py (GPU, through cd_op_attention_ex /
cd_op_cross_attention_ctrl_ex).

  CASES        one row per launch form (the call sites are named beside each family below); the smallest shapes that still
               reach the kernel instance, the ragged tiles and the workgroup counts of the form
  build        seeded operands of a case, rounded to the activation format, the prescaled q' where the form carries q in log2
               units, and the float64 reference of the features the case switches on
  ref64        softmax(scale q k^T [+ causal mask]) v [+ obias] in float64; q_log2: softmax(ln 2 . q' k^T) on the prescaled q'
  prescale_q   q' = round16(fp32(q) * fp32(scale * log2 e)): the product the kernels form on a q that is NOT in log2 units
               (csrc/attn.hip: `f[e] *= qsc` ahead of pack8), rounded to nearest even as pack8 rounds - so a launch with
               q_log2 = 1 on q' holds the very Q fragments a launch with q_log2 = 0 on q computes

Bounds (the GPU test): those of tests/test_gpu_ops.py::test_attention - rel_to_max < 4e-3 f, mean_rel < 1.5e-3 f, f = 1 for
fp16 storage and 8 for bf16 - measured on these kernels with this input distribution (unit normal q, k, v). No form below adds
a rounding: q_log2 removes the rounding of q * scale (the reference starts from the same q'), obias is an fp32 add ahead of
the single output rounding and drawn at 0.05 so the output scale stays where it was; the comparison is made on got - obias
against ref - obias, where a bias taken from another channel or head is an error of full size.
"""
import functools
import math

import numpy as np
import torch

LOG2E_F32 = np.float32(1.44269504088896340736)  # the literal of csrc/attn.hip
LN2 = math.log(2.0)
REL, MEAN = 4e-3, 1.5e-3  # x f (1 fp16, 8 bf16): tests/test_gpu_ops.py::test_attention
OBIAS_STD = 0.05


def _case(name, D, H, B, Tq, Tk=None, layout=0, pad=0, vt=False, d_extra=0, t_extra=0, opad=0, q_log2=False, obias=False,
          causal=False, nan2=False, fallback=False):
    return dict(name=name, D=D, H=H, B=B, Tq=Tq, Tk=Tq if Tk is None else Tk, layout=layout, pad=pad, vt=vt, d_extra=d_extra,
                t_extra=t_extra, opad=opad, q_log2=q_log2, obias=obias, causal=causal, nan2=nan2, fallback=fallback)


# layout 0: q, k, v apart with row strides C + pad, C + 2 pad, C + 3 pad (no two equal: a stride taken from the wrong operand
# shows); 1: q | k in one tensor (row stride 2C + pad), v apart (C + pad); 2: q | k | v in one tensor (3C + pad).
# vt: V^T [B][H][D + d_extra][round_up(Tk, 64) + 64 t_extra] from the transpose kernel. nan2: K and V of the second batch element
# are NaN (they follow element 0's rows in memory) and element 0 alone is compared. opad: extra output columns, which must
# come back as the NaN they were filled with (set here and there: the output stride is its own parameter in every kernel).
CASES = [
    # SD / LDM self-attention, d = 80 / 160 (unet_openai.hip st_core16 on s.qkv1): one [B*T][3C] tensor, V token-major, q_log2
    _case("sd_qkv_d80/pad0", 80, 2, 2, 256, layout=2, q_log2=True),
    _case("sd_qkv_d80/pad8", 80, 2, 2, 256, layout=2, pad=8, opad=8, q_log2=True),
    _case("sd_qkv_d160", 160, 2, 1, 64, layout=2, q_log2=True),
    # ... d = 40: q | k in [B*T][2C], V^T with the entry's Tpad, q_log2; T >= 1024 runs k_attention_d40<8>
    _case("sd_qk_vt_d40", 40, 2, 2, 256, layout=1, pad=8, vt=True, t_extra=1, q_log2=True),
    _case("sd_qk_vt_d40_long", 40, 2, 2, 1024, layout=1, vt=True, q_log2=True),
    _case("sd_qk_vt_d40_long_ragged", 40, 2, 2, 1100, layout=1, pad=8, vt=True, d_extra=8, opad=8, q_log2=True, nan2=True),
    # ... an output stride that is no multiple of 8 fails k_attention_d40's 16-byte gate: k_attention<48, 64, 40, 2, false, 32, 8>
    _case("d40_long_ldo4_fallback", 40, 2, 1, 1024, layout=1, vt=True, opad=4, fallback=True),
    # cross-attention: 77 context keys, token-major V, q_log2
    _case("cross_d40", 40, 2, 2, 256, 77, layout=0, pad=8, opad=8, q_log2=True, nan2=True),
    _case("cross_d160", 160, 2, 2, 64, 77, layout=0, pad=8, q_log2=True, nan2=True),
    # improved-DDPM AttentionBlock (d = 64) and the Ho / VAE AttnBlock (one head): q | k in [B*T][2C], V^T, obias, plain scale
    _case("ab_d64_obias/t256", 64, 2, 2, 256, layout=1, vt=True, obias=True),
    _case("ab_d64_obias/t100", 64, 2, 2, 100, layout=1, pad=8, vt=True, opad=8, obias=True),
    _case("vae_1head_d128_obias", 128, 1, 1, 64, layout=1, pad=8, vt=True, obias=True),
    # CLIP / BERT text towers and ViT (clip_text.hip): q | k in [B*L][2 inner], V^T, obias, causal for the CLIP text tower;
    # L = 77 puts a ragged 64-key tile and the causal mask together
    _case("clip_causal/l20", 64, 2, 2, 20, layout=1, vt=True, obias=True, causal=True),
    _case("clip_causal/l64", 64, 2, 2, 64, layout=1, pad=8, vt=True, obias=True, causal=True),
    _case("clip_causal/l65", 64, 2, 2, 65, layout=1, vt=True, obias=True, causal=True),
    _case("clip_causal/l77", 64, 2, 2, 77, layout=1, vt=True, opad=8, obias=True, causal=True, nan2=True),
    _case("clip_causal/l130", 64, 2, 2, 130, layout=1, pad=8, vt=True, opad=8, obias=True, causal=True),
]
BY_NAME = {c["name"]: c for c in CASES}
CAUSAL_J0 = (33, 64, 65)  # first replaced key of the causality test: inside a 32-key group, at a tile edge, one past it


def scale_of(c):
    return c["D"] ** -0.5


def prescale_q(q, scale, r16):
    """q' = round16(fp32(q) * fp32(fp32(scale) * fp32(log2 e)))"""
    qsc = np.float32(scale) * LOG2E_F32
    assert qsc.dtype == np.float32
    return r16(q.float() * torch.tensor(float(qsc), dtype=torch.float32))


def ref64(q, k, v, H, scale=None, q_log2=False, causal=False, obias=None):
    """q [B, Tq, C], k / v [B, Tk, C] -> [B, Tq, C] float64. q_log2: q is the prescaled q' and the logits are ln 2 . q' k^T"""
    B, Tq, C = q.shape
    Tk, D = k.shape[1], C // H
    hs = lambda t: t.double().reshape(t.shape[0], t.shape[1], H, D).transpose(1, 2)
    s = hs(q) @ hs(k).transpose(-1, -2) * (LN2 if q_log2 else scale)
    if causal:
        assert Tq == Tk
        i = torch.arange(Tq)
        s = s.masked_fill(i[None, :] > i[:, None], float("-inf"))
    o = (torch.softmax(s, dim=-1) @ hs(v)).transpose(1, 2).reshape(B, Tq, C)
    return o + obias.double() if obias is not None else o


def _seed(name):
    return 1000 + [c["name"] for c in CASES].index(name)


def build(name, r16, fmt):
    """operands of case `name` (fmt: "fp16" | "bf16", the cache key of the rounding r16): q, k, v rounded to the format,
    qp = the prescaled q' (q_log2 cases), obias, and ref = float64 with the case's features on - of batch element 0 alone when
    the second element's K / V are NaN. Nothing of it is ever written to: tests that change operands clone them."""
    return _build(name, fmt, r16)


@functools.lru_cache(maxsize=None)
def _build(name, fmt, r16):
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(_seed(name))
    C = c["H"] * c["D"]
    q = r16(torch.randn(c["B"], c["Tq"], C, generator=g))
    k = r16(torch.randn(c["B"], c["Tk"], C, generator=g))
    v = r16(torch.randn(c["B"], c["Tk"], C, generator=g))
    obias = OBIAS_STD * torch.randn(C, generator=g) if c["obias"] else None
    if c["nan2"]:
        k[1] = float("nan")
        v[1] = float("nan")
    nb = 1 if c["nan2"] else c["B"]  # batch elements that are compared
    scale = scale_of(c)
    qp = prescale_q(q, scale, r16) if c["q_log2"] else None
    ref = ref64((qp if c["q_log2"] else q)[:nb], k[:nb], v[:nb], c["H"], scale, q_log2=c["q_log2"], causal=c["causal"],
                obias=obias)
    return dict(case=c, q=q, k=k, v=v, qp=qp, obias=obias, scale=scale, nb=nb, ref=ref)
