"""CPU: the float64 references of tests/_inception_ops_ref.py against torch in float64 (F.avg_pool2d with
count_include_pad=False, F.max_pool2d, F.conv2d with tuple padding, an eval-mode nn.BatchNorm2d(eps=1e-3) behind the conv), and
the bounds of tests/test_gpu_inception_ops.py against fp32 restatements of the kernels' arithmetic: every restatement must sit
inside its bound on the inputs the GPU test uses, and every wrong variant (divisor 9, eps 1e-5) must fall outside."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _inception_ops_ref as ir

FMTS = ("fp16", "bf16")


def test_one_rounding_from_float64():
    g = torch.Generator().manual_seed(0)
    v = torch.cat([torch.randn(20000, generator=g, dtype=torch.float64) * 3, torch.randn(2000, generator=g, dtype=torch.float64) * 1e-5])
    assert torch.equal(ir.round16_f64(v, "fp16"), torch.from_numpy(v.numpy().astype(np.float16).astype(np.float64)))
    # a value a hair above a tie: by way of fp32 it would land on the tie and round down to even
    tie = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -40, 1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)
    assert ir.round16_f64(tie[:1], "fp16").item() == 1.0 + 2.0 ** -10
    assert ir.round16_f64(tie[1:], "bf16").item() == 1.0 + 2.0 ** -7
    b = ir.round16_f64(v, "bf16")
    assert torch.equal(b, b.float().to(torch.bfloat16).double())  # representable
    assert ((b - v).abs() <= 0.5 * ir.step16(v, "bf16")).all()


@pytest.mark.parametrize("c", ir.POOL_CASES, ids=[c["name"] for c in ir.POOL_CASES])
@pytest.mark.parametrize("fmt", FMTS)
def test_pool_references_and_bounds(c, fmt):
    worst = 0.0
    for C, _, _, kind in ir.pool_variants(c)[::4]:  # in_pad and the output slice do not enter the values
        x = ir.pool_input(c, C, kind, fmt)
        if kind == "relu":
            assert 0.3 < (x == 0).double().mean() < 0.7
        Ho, Wo = ir.pool_out_hw(c["H"], c["W"], c["stride"], c["pad"])
        if c["max"]:
            ref = ir.max_pool_ref(x, c["stride"], c["pad"])
            assert ref.shape == (c["B"], C, Ho, Wo)
            assert torch.equal(ref, F.max_pool2d(x, 3, c["stride"], c["pad"]))
            continue
        ref, mean, _, n = ir.avg_pool_ref(x, c["stride"], c["pad"], fmt)
        assert ref.shape == (c["B"], C, Ho, Wo)
        want = F.avg_pool2d(x, 3, c["stride"], c["pad"], count_include_pad=False)
        assert (mean - want).abs().max() <= 1e-15 * max(1.0, float(want.abs().max()))
        assert set(n.unique().tolist()) <= {4.0, 6.0, 9.0}
        if (c["H"], c["W"]) == (3, 3):
            assert (n < 9).sum() == 8  # every output pixel but the centre lacks taps
        else:
            assert (n == 9).any() and (n == 6).any() and (n == 4).any()
        # the kernel's arithmetic in fp32 stays inside both conditions ...
        v = ir.avg_verify(ir.avg_pool_emulate(x, c["stride"], c["pad"], fmt), x, c["stride"], c["pad"], fmt)
        assert v["ratio"] <= 1.0 and v["equal"] >= 0.95, v
        worst = max(worst, 1.0 - v["equal"])
        # ... a kernel that divides by 9 everywhere does not, and the divisor-9 reference rejects the right kernel
        bad = ir.avg_verify(ir.avg_pool_emulate(x, c["stride"], c["pad"], fmt, divisor9=True), x, c["stride"], c["pad"], fmt)
        assert bad["ratio"] > 1.0 and bad["border_fail"] >= 0.5, bad
        mut = ir.avg_verify(ir.avg_pool_emulate(x, c["stride"], c["pad"], fmt), x, c["stride"], c["pad"], fmt, divisor9=True)
        assert mut["ratio"] > 1.0 and mut["border_fail"] >= 0.5, mut
    print("%s %s: largest share of restated outputs off the correctly rounded value %.4f" % (c["name"], fmt, worst))


@pytest.mark.parametrize("c", ir.GAVG_CASES, ids=[c["name"] for c in ir.GAVG_CASES])
@pytest.mark.parametrize("fmt", FMTS)
def test_global_average_bound(c, fmt):
    x = ir.gavg_input(c, fmt)
    assert ir.gavg_verify(x.mean(2), x) == 0.0
    r = ir.gavg_verify(ir.gavg_emulate(x), x)
    assert r <= 1.0, r
    assert ir.gavg_verify(x.sum(2) / (x.shape[2] + 1), x) > 1.0  # a wrong divisor falls outside


@pytest.mark.parametrize("c", ir.CONV_CASES, ids=[c["name"] for c in ir.CONV_CASES])
def test_conv_reference_against_torch(c):
    o = ir.conv_operands(c, "fp16")
    d = {k: v.double() for k, v in o.items()}
    want = F.conv2d(d["x"], d["w"], None, c["stride"], c["pad"])
    got = ir.conv2d_f64(o["x"], o["w"], c["stride"], c["pad"])
    assert got.shape == want.shape == (c["B"], c["N"]) + ir.conv_out_hw(c)
    assert (got - want).abs().max() <= 1e-13 * float(want.abs().max())
    # conv -> BatchNorm2d(eps = 1e-3, eval) -> ReLU as torch modules: the unfolded reference, and the float64 fold
    bn = nn.BatchNorm2d(c["N"], eps=1e-3).double().eval()
    with torch.no_grad():
        bn.weight.copy_(d["gamma"]); bn.bias.copy_(d["beta"]); bn.running_mean.copy_(d["mean"]); bn.running_var.copy_(d["var"])
        ref = F.relu(bn(want))
    unf = ir.bn_conv_ref(o, c["stride"], c["pad"])
    scale = float(ref.abs().max())
    assert (unf - ref).abs().max() <= 1e-12 * scale
    wf, bf, _ = ir.fold_ref(o)
    folded = (ir.conv2d_f64(o["x"], wf, c["stride"], c["pad"]) + bf[None, :, None, None]).clamp_min(0.0)
    assert (folded - ref).abs().max() <= 1e-12 * scale
    clipped = (ref == 0).double().mean().item()
    if c["balanced"]:
        assert 0.3 < clipped < 0.7, clipped
    assert float(o["var"].min()) <= 1e-5 and float(o["gamma"].min()) < 0 < float(o["gamma"].max())


@pytest.mark.parametrize("c", ir.CONV_CASES, ids=[c["name"] for c in ir.CONV_CASES])
@pytest.mark.parametrize("fmt", FMTS)
def test_fold_bounds(c, fmt):
    o = ir.conv_operands(c, fmt)
    N, Cin, KH, KW = c["N"], c["Cin"], c["KH"], c["KW"]
    Cpad, Npad = -(-Cin // 32) * 32, -(-N // 128) * 128
    w, b = ir.fold_emulate(o, fmt)
    wp, bo = torch.zeros(Npad, KH, KW, Cpad), torch.zeros(Npad)
    wp[:N, :, :, :Cin] = w.permute(0, 2, 3, 1).float()
    bo[:N] = b.float()
    v = ir.fold_verify(c, o, wp, bo, fmt)
    assert v["w_ratio"] <= 1.0 and v["b_ratio"] <= 1.0 and v["nonzero"] == 0, v
    bad = ir.fold_verify(c, o, wp, bo, fmt, eps=1e-5)  # the wrong eps in the reference rejects the right fold
    assert bad["w_ratio"] > 1.0 and bad["b_ratio"] > 1.0, bad
    w5, b5 = ir.fold_emulate(o, fmt, eps=1e-5)         # ... and the right reference a fold with the wrong eps
    wp[:N, :, :, :Cin] = w5.permute(0, 2, 3, 1).float()
    bo[:N] = b5.float()
    bad = ir.fold_verify(c, o, wp, bo, fmt)
    assert bad["w_ratio"] > 1.0 and bad["b_ratio"] > 1.0, bad
    wp[N - 1, 0, 0, Cpad - 1] = 1.0 if Cpad > Cin else 0.0
    if Npad > N:
        bo[N] = 1.0
    assert ir.fold_verify(c, o, wp, bo, fmt)["nonzero"] == (Cpad > Cin) + (Npad > N)


def test_case_tables_cover_the_forms_of_the_network():
    cs = ir.CONV_CASES
    assert {(c["KH"], c["KW"], c["pad"]) for c in cs} >= {(1, 7, (0, 3)), (7, 1, (3, 0)), (1, 3, (0, 1)), (3, 1, (1, 0)),
                                                          (5, 5, (2, 2)), (3, 3, (0, 0)), (1, 1, (0, 0))}
    assert {(c["off"], c["ld"], c["N"]) for c in cs} >= {(0, 32, 32), (64, 288, 32), (224, 256, 32), (1856, 2048, 192)}
    assert {c["B"] for c in cs} == {1, 2, 3}
    M = [c["B"] * ir.conv_out_hw(c)[0] * ir.conv_out_hw(c)[1] for c in cs]
    assert sum(m % 32 != 0 for m in M) >= len(cs) - 4
    assert sum(c["balanced"] for c in cs) * 2 >= len(cs) - 1
    assert {80, 48} <= {c["N"] for c in cs} and any(c["Cin"] == 3 for c in cs) and any(c["in_ld"] > -(-c["Cin"] // 32) * 32 for c in cs)
    assert all(n in ir.CONV and ir.CONV[n]["KH"] * ir.CONV[n]["KW"] > 1 for n in ir.CONV_CHM)
    assert all(max(c["H"], c["W"]) <= 17 for c in cs + ir.POOL_CASES)
