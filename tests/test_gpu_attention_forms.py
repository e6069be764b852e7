"""k_attention, k_attention_d40 and k_cross_attention_ctrl (csrc/attn.hip) in the operand forms the networks launch, through
cd_op_attention_ex / cd_op_cross_attention_ctrl_ex: q | k (| v) as column blocks of one padded tensor, V^T with spare rows
and key tiles, q in log2 units, the output bias, the causal mask, a padded output. cd_op_attention launches none of these
(dense operands, q_log2 = 0, no bias, no mask), so an index that is only right where every stride equals C passes its tests.

Cases, inputs and the float64 reference: tests/_attn_forms_ref.py (checked on the host by tests/test_attn_forms_host.py).
  1. the strided / fused / padded launch equals cd_op_attention on the same values bit for bit
  2. every case with its features on, against float64 at test_attention's bounds; every figure goes to the report
  3. q_log2 = 1 on the prescaled q' equals q_log2 = 0 on q bit for bit
  4. the pad columns of the output come back as the NaN they were filled with (asserted on every call here)
  5. the causal mask is exact: keys >= j0 do not move a bit of rows < j0
  6. the control kernel with q_log2 = 1 and a padded output, against the float64 restatement of tests/_attn_control_ref.py

Kernel instance per case (launch_attention's dispatch, defaults of the CD_ATTN_* switches), `tok` = VTOK, `vt` = V^T:
  sd_qkv_d80            k_attention<80, 96, 80, 2, tok, 32>       sd_qkv_d160          k_attention<160, 160, 0, 1, tok, 64>
  sd_qk_vt_d40          k_attention<48, 64, 40, 2, vt, 32>        sd_qk_vt_d40_long(_ragged)  k_attention_d40<8>
  d40_long_ldo4_fallback  k_attention<48, 64, 40, 2, vt, 32, 8>   cross_d40 / cross_d160  <48, 64, 40, 2, tok, 32> / <160, 160, 0, 1, tok, 64>
  ab_d64_obias, clip_causal  k_attention<64, 64, 0, 2, vt, 64>    vae_1head_d128_obias  k_attention<128, 128, 0, 1, vt, 64>
  ctrl_q_log2           k_cross_attention_ctrl<48, 64>, <160, 160>, <80, 96>
"""
import pytest
import torch

import _attn_control_ref as acr
import _attn_forms_ref as R
import _ops
from _ops import bf16_round as r16
from cycle_diffusion_amd import _ffi
from test_gpu_attn_control import CTRL_CASES, _operands as ctrl_operands, ctrl_attention

pytestmark = pytest.mark.gpu

FP16 = _ffi.load_library().cd_act_format() == 1
FMT = "fp16" if FP16 else "bf16"
F8 = 1.0 if FP16 else 8.0
NAMES = [c["name"] for c in R.CASES]


def _form(c):
    return dict(layout=c["layout"], pad=c["pad"], v_transposed=c["vt"], d_extra=c["d_extra"], t_extra=c["t_extra"],
                opad=c["opad"])


def _result(out, C, nb, what):
    """[B, Tq, C + opad] -> the result columns of the compared batch elements. Every pad column holds the NaN the output buffer
    was filled with, every result column of a compared element is finite."""
    assert torch.isnan(out[..., C:]).all(), (what, "pad columns of the output were written")
    res = out[:nb, :, :C]
    assert torch.isfinite(res).all(), (what, "non-finite result")
    return res


_GOT = {}  # case name -> the features-on result (computed once, shared by tests 2 and 3)


def _features_on(engine, name):
    if name not in _GOT:
        d = R.build(name, r16, FMT)
        c = d["case"]
        out = _ops.attention_ex(engine, d["qp"] if c["q_log2"] else d["q"], d["k"], d["v"], c["H"], d["scale"],
                                q_log2=c["q_log2"], obias=d["obias"], causal=c["causal"], **_form(c))
        _GOT[name] = _result(out, c["H"] * c["D"], d["nb"], name)
    return _GOT[name]


# ------------------------------------------------------------------------------------------------ 1. layout changes nothing
@pytest.mark.parametrize("name", [c["name"] for c in R.CASES if not c["fallback"]])
def test_layout_changes_nothing(engine, name):
    """q_log2, obias and causal off: the same values at other addresses are the same launch of the same kernel instance as
    cd_op_attention's (same v_transposed), so every bit agrees. (The fallback case is left out: there the output stride
    selects another kernel than the dense call runs.)"""
    d = R.build(name, r16, FMT)
    c = d["case"]
    want = _ops.attention(engine, d["q"], d["k"], d["v"], c["H"], d["scale"], v_transposed=c["vt"])[:d["nb"]]
    got = _result(_ops.attention_ex(engine, d["q"], d["k"], d["v"], c["H"], d["scale"], **_form(c)), c["H"] * c["D"], d["nb"], name)
    assert torch.isfinite(want).all()
    assert torch.equal(got, want), (name, (got - want).abs().max().item(), int((got != want).sum()))


# ------------------------------------------------------------------------------------------------ 2. against float64
@pytest.mark.parametrize("name", NAMES)
def test_forms_vs_float64(engine, report, name):
    d = R.build(name, r16, FMT)
    got, ref = _features_on(engine, name).double(), d["ref"]
    if d["obias"] is not None:  # the bias out of both sides: a bias from the wrong channel / head is then an error of its full size
        got, ref = got - d["obias"].double(), ref - d["obias"].double()
    st = _ops.err_stats(got, ref)
    report.add("attention_forms/" + name, **st)
    print("attention_forms/%s %s" % (name, st))
    assert st["rel_to_max"] < R.REL * F8 and st["mean_rel"] < R.MEAN * F8, (name, st)


# ------------------------------------------------------------------------------------------------ 3. q_log2 adds nothing
@pytest.mark.parametrize("name", [c["name"] for c in R.CASES if c["q_log2"]])
def test_q_log2_adds_nothing(engine, name):
    """q' = round16(q * scale * log2 e) on the host is the fragment the kernel forms from q when q_log2 = 0 (fp32 product,
    round to nearest even): both launches then run the same arithmetic on the same bits"""
    d = R.build(name, r16, FMT)
    c = d["case"]
    plain = _result(_ops.attention_ex(engine, d["q"], d["k"], d["v"], c["H"], d["scale"], q_log2=False, **_form(c)),
                    c["H"] * c["D"], d["nb"], name)
    got = _features_on(engine, name)
    assert torch.equal(got, plain), (name, (got - plain).abs().max().item(), int((got != plain).sum()))


# ------------------------------------------------------------------------------------------------ 5. causality
def _ulp(x):
    """spacing of the storage format at |x| (normal range; fp16 subnormals: 2^-24)"""
    _, e = torch.frexp(x.abs().double())
    u = torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - (11 if FP16 else 8))
    return u.clamp_min(2.0 ** -24) if FP16 else u


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES if c["causal"]])
def test_causal_mask_is_exact(engine, name):
    """Keys >= j0 replaced by finite values four times larger: rows < j0 keep every bit (a masked score is -inf ahead of the
    maximum, and a row whose maximum did not grow is rescaled by exactly 1), rows >= j0 all change. Row 0 sees key 0 alone:
    p = 1, l = 1, so it is round16(v[0] + obias), to one unit in the last place."""
    d = R.build(name, r16, FMT)
    c, nb = d["case"], d["nb"]
    C, L = c["H"] * c["D"], c["Tq"]
    base = _features_on(engine, name)
    row0 = r16(d["v"][:nb, 0] + d["obias"])
    assert ((base[:, 0].double() - row0.double()).abs() <= _ulp(row0)).all(), (name, (base[:, 0] - row0).abs().max().item())
    g = torch.Generator().manual_seed(99)
    for j0 in [j for j in R.CAUSAL_J0 if j < L]:
        k2, v2 = d["k"].clone(), d["v"].clone()
        k2[:nb, j0:] = r16(4.0 * torch.randn(nb, L - j0, C, generator=g))
        v2[:nb, j0:] = r16(4.0 * torch.randn(nb, L - j0, C, generator=g))
        out = _ops.attention_ex(engine, d["q"], k2, v2, c["H"], d["scale"], obias=d["obias"], causal=True, **_form(c))
        got = _result(out, C, nb, (name, j0))
        assert torch.equal(got[:, :j0], base[:, :j0]), (name, j0, int((got[:, :j0] != base[:, :j0]).any(-1).sum()))
        assert (got[:, j0:] != base[:, j0:]).any(-1).all(), (name, j0)


# ------------------------------------------------------------------------------------------------ 6. the control kernel
@pytest.mark.parametrize("case", CTRL_CASES[:3], ids=["b%d_s%d_h%d_t%d_l%d_d%d" % c for c in CTRL_CASES[:3]])
def test_ctrl_q_log2(engine, report, case):
    """k_cross_attention_ctrl as the coupled loop launches it - both q tensors in log2 units, the output rows inside a wider
    tensor - against the float64 restatement on the prescaled q' (logits ln 2 . q' k^T), at test_ctrl_attention_vs_float64's
    bounds; bit for bit against q_log2 = 0 on q, and the dense, unpadded form against cd_op_cross_attention_ctrl."""
    B, Bs, H, Tq, L, D = case
    t, g = ctrl_operands(case)
    M, alpha, w = acr.random_control(g, Bs, L, fractional=True)
    scale, C, opad = D ** -0.5, H * D, 8
    tp = dict(t, q_own=R.prescale_q(t["q_own"], scale, r16), q_src=R.prescale_q(t["q_src"], scale, r16))
    run = lambda tt, **kw: _ops.cross_attention_ctrl_ex(engine, tt["q_own"], tt["q_src"], tt["k_own"], tt["k_src"], tt["v_own"],
                                                        M, alpha, w, H, scale, **kw)
    name = "ctrl_q_log2/" + "x".join(map(str, case))
    got = _result(run(tp, q_log2=True, opad=opad), C, B, name)
    ref = acr.ctrl_attention_ref(M=M, alpha=alpha, w=w, H=H, scale=R.LN2, **tp)
    st = _ops.err_stats(got.double(), ref)
    report.add("attention_forms/" + name, **st)
    print("attention_forms/%s %s" % (name, st))
    assert st["rel_to_max"] < R.REL * F8 and st["mean_rel"] < R.MEAN * F8, (name, st)
    plain = _result(run(t, q_log2=False, opad=opad), C, B, name)
    assert torch.equal(got, plain), (name, (got - plain).abs().max().item())
    dense = ctrl_attention(engine, t["q_own"], t["q_src"], t["k_own"], t["k_src"], t["v_own"], M, alpha, w, H, scale)
    assert torch.equal(plain, dense), (name, (plain - dense).abs().max().item())
