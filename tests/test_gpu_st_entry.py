"""GPU: the entry of the 64 x 64 SpatialTransformer blocks (d_head = 40) - GroupNorm -> proj_in -> LayerNorm1 -> to_q | to_k ->
V^T - through cd_op_st_entry, with the three stages of DESIGN.md section 8 switched one by one:

  A (bit 0)  one q | k | v launch of the streaming kernel whose last 320 columns leave as V^T: the same bits as the q | k
             launch (the streaming kernel, tile 30, and a k_conv_gemm tile) and the V^T GEMM on the same operands
  B (bit 1)  LayerNorm1 inside that launch, gain and bias in its weights: one more rounding of the weights, so its bound is
             not a fixed number - the unfused path (k_layernorm + stage A) is measured against the same float64 result and
             the fused path may show up to twice its max-abs and RMS error (the margin of the phase-form weights, section 3)
  C (bit 2)  GroupNorm's multiply-add applied in proj_in's registers: the same bits as k_gn_apply followed by proj_in

K = 320 throughout. Inputs are seeded, rounded to 16 bits, with a per-pixel offset so that row means are not zero.

Measured on an MI355X, fp16 storage (max-abs / RMS error against float64, unfused -> fused; profiles/r8_st_entry_accuracy.json):
    stage B  b17_64x64  q | k  2.802e-03 / 2.259e-04 -> 2.976e-03 / 2.700e-04   (x 1.06 / 1.20)
                        V^T    2.608e-03 / 3.144e-04 -> 3.084e-03 / 3.753e-04   (x 1.18 / 1.19)
    all      b17_64x64  q | k  2.895e-03 / 3.066e-04 -> 3.133e-03 / 3.405e-04   (x 1.08 / 1.11)
                        V^T    2.988e-03 / 4.247e-04 -> 3.116e-03 / 4.716e-04   (x 1.04 / 1.11)
"""
import ctypes as C
import math
import zlib

import pytest
import torch

import _ops
from _ops import bf16_round as r16
from cycle_diffusion_amd._ffi import check, ptr

pytestmark = pytest.mark.gpu

K = 320
# name, B, H, W, fused launches expected
CASES = [
    ("b8_64x64", 8, 64, 64, True),     # 32 768 rows: the row threshold, 128 strips
    ("b17_64x64", 17, 64, 64, True),   # 272 strips: some workgroups take a second strip, an image boundary inside their sequence
    ("b16_32x64", 16, 32, 64, True),   # 8 strips per image: the image index of the coefficients and of V^T
    ("b21_40x40", 21, 40, 40, False),  # H W % 256 != 0: the gate refuses, the parent's launches run
]
FUSED = [c[0] for c in CASES if c[4]]


@pytest.fixture(scope="module")
def cases(engine):
    """name -> operands, float64 references and every stage combination's outputs: computed once per case, shared, not
    modified, and released (several GB of device memory) when the module's tests are done"""
    cache = {}
    yield lambda name: _case(engine, name, cache)
    cache.clear()
    torch.cuda.empty_cache()


def _entry(engine, c, stages, vbias=None):
    B, H, W = c["B"], c["H"], c["W"]
    T = H * W
    Tpad = (T + 63) // 64 * 64
    h = torch.empty((B, K, H, W), device="cuda", dtype=torch.float32)
    qk = torch.empty((B, 2 * K, H, W), device="cuda", dtype=torch.float32)
    vt = torch.empty((B, K, Tpad), device="cuda", dtype=torch.float32)
    ran = C.c_int(-1)
    check(engine.lib.cd_op_st_entry(engine.h, ptr(c["x"]), B, H, W, ptr(c["gn_g"]), ptr(c["gn_b"]), C.c_float(1e-6),
                                    c["h_in"], ptr(c["b_in"]), ptr(c["ln_g"]), ptr(c["ln_b"]), c["h_qk"], c["h_v"],
                                    ptr(vbias), stages, ptr(h), ptr(qk), ptr(vt), C.byref(ran)))
    torch.cuda.synchronize()
    return dict(h=h, qk=qk, vt=vt[:, :, :T], ran=ran.value)


def _rows(t):  # NCHW -> [B * H * W][C]
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _ln64(rows, g, b):
    r = rows.double()
    mu = r.mean(1, keepdim=True)
    var = r.var(1, unbiased=False, keepdim=True)
    return (r - mu) / torch.sqrt(var + 1e-5) * g.double() + b.double()


def _qkv64(n1, c, B, T, vbias=None):
    """float64 q | k rows [B T][640] and V^T [B][320][T] of normalised rows"""
    qk = n1 @ c["w_qk"].double().cuda().t()
    v = n1 @ c["w_v"].double().cuda().t()
    if vbias is not None:
        v = v + vbias.double()
    return qk, v.reshape(B, T, K).transpose(1, 2)


def _case(engine, name, cache):
    if name in cache:
        return cache[name]
    _, B, H, W, fused = next(c for c in CASES if c[0] == name)
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % (2 ** 31))
    x = r16(torch.randn(B, K, H, W, generator=g) * 1.7 + 0.3 * torch.randn(B, 1, H, W, generator=g))
    qscale = 1.44269504088896340736 / math.sqrt(40.0)
    w_in = r16(torch.randn(K, K, generator=g) / math.sqrt(K))
    w_qk = r16(torch.cat([torch.randn(K, K, generator=g) * qscale, torch.randn(K, K, generator=g)]) / math.sqrt(K))
    w_v = r16(torch.randn(K, K, generator=g) / math.sqrt(K))
    c = dict(B=B, H=H, W=W, x=x.cuda(), w_in=w_in, w_qk=w_qk, w_v=w_v,
             b_in=(torch.randn(K, generator=g) * 0.5).cuda(),
             gn_g=(1.0 + 0.2 * torch.randn(K, generator=g)).cuda(), gn_b=(0.2 * torch.randn(K, generator=g)).cuda(),
             ln_g=(1.0 + 0.2 * torch.randn(K, generator=g)).cuda(), ln_b=(0.3 * torch.randn(K, generator=g)).cuda(),
             vbias=(torch.randn(K, generator=g) * 0.5).cuda())
    c["h_in"], _ = _ops.pack_conv(engine, w_in)
    c["h_qk"], _ = _ops.pack_conv(engine, w_qk)
    c["h_v"], _ = _ops.pack_conv(engine, w_v)
    c["out"] = {s: _entry(engine, c, s) for s in (0, 1, 3, 4, 7)}
    if fused:
        c["out_vbias"] = _entry(engine, c, 1, vbias=c["vbias"])
        T = H * W
        # stage B's reference starts from the 16-bit h every path shares; the whole segment's from x
        h16 = _rows(c["out"][0]["h"])
        c["ref_b"] = _qkv64(_ln64(h16, c["ln_g"], c["ln_b"]), c, B, T)
        # stage A's operand: k_layernorm's 16-bit output of those rows, and float64 values of the V^T it must produce with a bias
        n1 = torch.empty((B * T, K), device="cuda", dtype=torch.float32)
        check(engine.lib.cd_op_layernorm(engine.h, ptr(h16.contiguous()), B * T, K, ptr(c["ln_g"]), ptr(c["ln_b"]),
                                         C.c_float(1e-5), ptr(n1)))
        torch.cuda.synchronize()
        c["n1"] = n1
        c["ref_a_vbias"] = _qkv64(n1.double(), c, B, T, c["vbias"])[1]
        gn = torch.nn.functional.group_norm(c["x"].double(), 32, c["gn_g"].double(), c["gn_b"].double(), 1e-6)
        h64 = _rows(gn) @ w_in.double().cuda().t() + c["b_in"].double()
        c["ref_all"] = _qkv64(_ln64(h64, c["ln_g"], c["ln_b"]), c, B, T)
    cache[name] = c
    return c


def _errs(got, ref):
    d = got.double() - ref
    return d.abs().max().item(), d.pow(2).mean().sqrt().item()


def _conv16(engine, x, handle, N, tile):
    """cd_op_conv2d_16 on device tensors: a 1 x 1 layer without bias on an explicit tile"""
    B, Cin, H, W = x.shape
    y = torch.empty((B, N, H, W), device="cuda", dtype=torch.float32)
    check(engine.lib.cd_op_conv2d_16(engine.h, ptr(x), Cin, None, 0, B, H, W, handle, N, 1, 1, 1, 0, 0, 0, None, None, None,
                                     0, tile, ptr(y), None))
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("name,fused", [(c[0], c[4]) for c in CASES])
def test_gate_follows_the_image_size(engine, cases, name, fused):
    """40 x 40 images are no multiple of 256 tokens: the parent's launches run whatever the switch says, so every output agrees
    with the all-off run bit for bit"""
    c = cases(name)
    for s in (1, 3, 4, 7):
        assert c["out"][s]["ran"] == (s if fused else 0), (name, s, c["out"][s]["ran"])
    if not fused:
        for s in (1, 3, 4, 7):
            for k in ("h", "qk", "vt"):
                assert torch.equal(c["out"][s][k], c["out"][0][k]), (name, s, k)


@pytest.mark.parametrize("name", FUSED)
def test_stage_a_same_bits_as_qk_launch_and_vt_gemm(engine, cases, name):
    c = cases(name)
    off, on = c["out"][0], c["out"][1]
    assert torch.isfinite(on["qk"]).all() and torch.isfinite(on["vt"]).all()
    assert torch.equal(on["h"], off["h"])
    assert torch.equal(on["qk"], off["qk"])  # the launch the U-Net ran before
    assert torch.equal(on["vt"], off["vt"])  # vt_gemm on the same operands
    # the q | k launch on the streaming kernel (tile 30) and on a k_conv_gemm tile, from the same normalised rows
    B, H, W = c["B"], c["H"], c["W"]
    n1 = c["n1"].reshape(B, H, W, K).permute(0, 3, 1, 2).contiguous()
    for tile in (30, 2):
        assert torch.equal(on["qk"], _conv16(engine, n1, c["h_qk"], 2 * K, tile)), (name, tile)


@pytest.mark.parametrize("name", FUSED)
def test_stage_a_value_bias_against_float64(engine, cases, report, name):
    """to_v has no bias in the reference, but the V^T exit adds one per channel (stage B's W beta): with a non-zero bias the
    result is one rounding of the float64 value of the same 16-bit operands (k_layernorm's output, the stored weights), plus
    the error of an fp32 sum of 320 products of magnitude <= 4, which is far below that rounding."""
    c = cases(name)
    got, ref = c["out_vbias"]["vt"], c["ref_a_vbias"]
    assert torch.equal(c["out_vbias"]["qk"], c["out"][1]["qk"])
    fp16 = engine.lib.cd_act_format() == 1
    ulp = 2.0 ** -11 if fp16 else 2.0 ** -8  # half a unit in the last place, relative
    d = (got.double() - ref).abs()
    bound = ulp * ref.abs().clamp_min(2.0 ** -14) * 1.02 + 320 * 2.0 ** -24 * 4.0
    report.add("st_entry/vbias_" + name, max_abs=d.max().item())
    assert (d <= bound).all(), (name, d.max().item())
    assert (got - c["out"][1]["vt"]).abs().max().item() > 0.1  # the bias is really there


@pytest.mark.parametrize("name", FUSED)
def test_stage_c_same_bits_as_gn_apply_and_proj_in(engine, cases, name):
    c = cases(name)
    assert torch.isfinite(c["out"][4]["h"]).all()
    for k in ("h", "qk", "vt"):
        assert torch.equal(c["out"][4][k], c["out"][0][k]), (name, k)


def _twice_rule(report, tag, name, unfused, fused, ref):
    figs = {}
    for k, r in (("qk", ref[0]), ("vt", ref[1])):
        u = fused[k] if k == "vt" else _rows(fused[k])
        b = unfused[k] if k == "vt" else _rows(unfused[k])
        b_max, b_rms = _errs(b, r)
        f_max, f_rms = _errs(u, r)
        print("st_entry/%s/%s/%s unfused max_abs %.6e rms %.6e | fused max_abs %.6e rms %.6e" % (tag, name, k, b_max, b_rms, f_max, f_rms))
        figs[k] = (b_max, b_rms, f_max, f_rms)
        report.add("st_entry/%s/%s/%s" % (tag, name, k), unfused_max_abs=b_max, unfused_rms=b_rms, fused_max_abs=f_max, fused_rms=f_rms)
    for k, (b_max, b_rms, f_max, f_rms) in figs.items():
        assert b_max > 0 and b_rms > 0
        assert f_max <= 2.0 * b_max, (tag, name, k, f_max, b_max)
        assert f_rms <= 2.0 * b_rms, (tag, name, k, f_rms, b_rms)


@pytest.mark.parametrize("name", FUSED)
def test_stage_b_error_within_twice_the_unfused_path(engine, cases, report, name):
    c = cases(name)
    assert torch.isfinite(c["out"][3]["qk"]).all() and torch.isfinite(c["out"][3]["vt"]).all()
    assert torch.equal(c["out"][3]["h"], c["out"][1]["h"])
    assert not torch.equal(c["out"][3]["qk"], c["out"][1]["qk"])  # folded weights: some output rounds the other way
    _twice_rule(report, "stage_b", name, c["out"][1], c["out"][3], c["ref_b"])


@pytest.mark.parametrize("name", FUSED)
def test_whole_entry_error_within_twice_the_separate_launches(engine, cases, report, name):
    c = cases(name)
    assert torch.equal(c["out"][7]["h"], c["out"][0]["h"])
    assert torch.equal(c["out"][7]["qk"], c["out"][3]["qk"]) and torch.equal(c["out"][7]["vt"], c["out"][3]["vt"])
    _twice_rule(report, "all", name, c["out"][0], c["out"][7], c["ref_all"])
