"""CPU: the float64 reference of tests/test_gpu_attention_forms.py (tests/_attn_forms_ref.py) is the attention torch computes,
with and without the causal mask and the output bias, and its q_log2 form - softmax(ln 2 . q' k^T) on the prescaled q' - is the
plain-scale attention up to the one rounding of q'."""
import pytest
import torch
import torch.nn.functional as F

import _attn_forms_ref as R
import _ops
from cycle_diffusion_amd import _ffi


def _fmt():
    fp16 = _ffi.load_library().cd_act_format() == 1
    return "fp16" if fp16 else "bf16", 2.0 ** -11 if fp16 else 2.0 ** -8  # half a unit in the last place


def _sdpa(q, k, v, H, scale, causal):
    B, Tq, C = q.shape
    hs = lambda t: t.double().reshape(t.shape[0], t.shape[1], H, C // H).transpose(1, 2)
    return F.scaled_dot_product_attention(hs(q), hs(k), hs(v), is_causal=causal, scale=scale).transpose(1, 2).reshape(B, Tq, C)


# (B, H, D, Tq, Tk, causal): the causal form is self-attention
_SDPA_SHAPES = [(2, 2, 64, 77, 77, False), (2, 2, 64, 77, 77, True), (1, 3, 40, 130, 130, False), (1, 3, 40, 130, 130, True),
                (2, 1, 128, 20, 20, True), (1, 2, 80, 64, 77, False)]


@pytest.mark.parametrize("shape", _SDPA_SHAPES, ids=lambda s: "b%d_h%d_d%d_tq%d_tk%d_causal%d" % s)
def test_reference_matches_torch_sdpa(shape):
    B, H, D, Tq, Tk, causal = shape
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(B, T, H * D, generator=g).double() for T in (Tq, Tk, Tk))
    obias = R.OBIAS_STD * torch.randn(H * D, generator=g)
    want = _sdpa(q, k, v, H, D ** -0.5, causal)
    assert (R.ref64(q, k, v, H, D ** -0.5, causal=causal) - want).abs().max() < 1e-12
    assert (R.ref64(q, k, v, H, D ** -0.5, causal=causal, obias=obias) - (want + obias.double())).abs().max() < 1e-12


def test_causal_reference_ignores_later_keys():
    g = torch.Generator().manual_seed(6)
    q, k, v = (torch.randn(1, 77, 128, generator=g) for _ in range(3))
    a = R.ref64(q, k, v, 2, 0.125, causal=True)
    k2, v2 = k.clone(), v.clone()
    k2[:, 33:] *= 4.0
    v2[:, 33:] = 4.0 * torch.randn(1, 44, 128, generator=g)
    b = R.ref64(q, k2, v2, 2, 0.125, causal=True)
    assert torch.equal(a[:, :33], b[:, :33]) and (a[:, 33:] != b[:, 33:]).any(-1).all()
    assert (a[:, 0] - v[:, 0].double()).abs().max() < 1e-15  # the first row sees its own key alone


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES if c["q_log2"]])
def test_prescaled_reference_is_the_plain_one_up_to_the_rounding_of_q(name):
    """q' = round16(q * scale * log2 e) is representable, at most half a unit in the last place (+ the fp32 product's 2^-24)
    from the exact product, and ln 2 . q' k^T moves a logit by at most u scale |q_i| |k_j| (Cauchy-Schwarz on the relative
    errors): the softmax row then moves by at most twice that in the 1-norm, the output by that times max |v|."""
    fmt, u = _fmt()
    d = R.build(name, _ops.bf16_round, fmt)
    c, nb = d["case"], d["nb"]
    q, qp, k, v = d["q"][:nb], d["qp"][:nb], d["k"][:nb], d["v"][:nb]
    assert torch.equal(qp, _ops.bf16_round(qp))
    exact = q.double() * d["scale"] * 1.44269504088896340736
    tiny = 2.0 ** -24 if fmt == "fp16" else 0.0  # fp16 subnormals: absolute spacing 2^-24
    assert ((qp.double() - exact).abs() <= (u + 2.0 ** -23) * exact.abs() + tiny).all()
    plain = R.ref64(q, k, v, c["H"], d["scale"])
    assert (plain - _sdpa(q, k, v, c["H"], d["scale"], False)).abs().max() < 1e-12
    hs = lambda t: t.double().reshape(t.shape[0], t.shape[1], c["H"], c["D"]).transpose(1, 2)
    ds = (u + 2.0 ** -22) * d["scale"] * hs(q).norm(dim=-1).max() * hs(k).norm(dim=-1).max() + tiny * hs(k).abs().sum(-1).max()
    bound = 2.0 * ds * v.abs().max()
    err = (d["ref"] - plain).abs().max()
    print(name, "prescaled - plain: %.3e (bound %.3e)" % (err.item(), bound.item()))
    assert 0 < err <= bound


def test_case_table_covers_every_form():
    """the table the GPU test walks: every layout, both V forms, every feature, and the sizes where the kernels change path"""
    cs = R.CASES
    assert {c["layout"] for c in cs} == {0, 1, 2}
    assert {c["vt"] for c in cs} == {False, True}
    assert any(c["D"] == 40 and c["vt"] and c["Tq"] >= 1024 and not c["fallback"] for c in cs)       # k_attention_d40
    assert any(c["fallback"] and c["opad"] % 8 == 4 and c["Tq"] >= 1024 for c in cs)                  # its 8-wave fallback
    assert any(c["causal"] and c["Tk"] % 64 and c["Tk"] > 64 for c in cs)                             # mask + ragged tile
    assert all(c["pad"] % 8 == 0 and c["opad"] % 4 == 0 for c in cs)
    assert all(c["layout"] == 0 or c["Tq"] == c["Tk"] for c in cs)
    assert all(j < 77 for j in R.CAUSAL_J0)
    assert len({c["name"] for c in cs}) == len(cs)
