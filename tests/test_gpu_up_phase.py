"""GPU: the nearest-x2 3 x 3 convolutions in their phase form (four 2 x 2 convs on the stored grid) through
the op entry point of the 16-bit path, cd_op_conv2d_16 with up = 1, against a float64 evaluation of the definition:
nearest-neighbour upsample, then the 3 x 3 conv with the unsummed weights as stored in 16 bits.

The phase path rounds every summed weight once more, so its bound is not a fixed number: the x2-gather path
(CYCLEDIFF_UP_PHASE=0, read per call) is measured on the same inputs against the same float64 result, and the phase path may
show up to twice its max-abs and RMS error - one more rounding of the same size per term can at most double the worst case.

Measured on an MI355X (max-abs / RMS error against float64, gather path -> phase path; profiles/r7_up_phase_accuracy.json):
    fp16 storage  b3_16x16_64_64   1.874e-03 / 2.291e-04 -> 2.235e-03 / 3.065e-04   (x 1.19 / 1.34)
                  b2_32x32_64_128  1.947e-03 / 2.326e-04 -> 2.426e-03 / 3.090e-04   (x 1.25 / 1.33)
    bf16 storage  b3_16x16_64_64   1.546e-02 / 1.834e-03 -> 1.723e-02 / 2.446e-03   (x 1.11 / 1.33)
                  b2_32x32_64_128  1.559e-02 / 1.861e-03 -> 1.956e-02 / 2.479e-03   (x 1.25 / 1.33)
"""
import math
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

import _ops
from _ops import bf16_round as r16

pytestmark = pytest.mark.gpu

# name, B, C, H, W, N, phase form expected
CASES = [
    ("b3_16x16_64_64", 3, 64, 16, 16, 64, True),     # one 256-row tile per phase and image; 12 row tiles: an uneven XCD walk
    ("b2_32x32_64_128", 2, 64, 32, 32, 128, True),   # several tiles per phase, N != C
    ("b1_8x8_64_64", 1, 64, 8, 8, 64, False),        # 64 stored pixels: below the 256-pixel condition, the gather path
]
_CACHE = {}


def _switch(on):
    os.environ["CYCLEDIFF_UP_PHASE"] = "1" if on else "0"


def _case(engine, name):
    """operands, float64 reference and both paths' results of a case: computed once, shared, not modified"""
    if name in _CACHE:
        return _CACHE[name]
    _, B, C, H, W, N, _ = next(c for c in CASES if c[0] == name)
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % (2 ** 31))
    x = r16(torch.randn(B, C, H, W, generator=g))
    w = r16(torch.randn(N, C, 3, 3, generator=g) / math.sqrt(C * 9))
    bias = torch.randn(N, generator=g) * 0.5
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), w.double(), bias.double(), padding=1)
    prev = os.environ.get("CYCLEDIFF_UP_PHASE")
    try:
        _switch(False)
        gather = _ops.conv2d16(engine, x, w, pad=1, bias=bias, up=True, want_stats=True)
        _switch(True)
        phase = _ops.conv2d16(engine, x, w, pad=1, bias=bias, up=True, want_stats=True)
    finally:
        if prev is None:
            os.environ.pop("CYCLEDIFF_UP_PHASE", None)
        else:
            os.environ["CYCLEDIFF_UP_PHASE"] = prev
    _CACHE[name] = dict(x=x, w=w, bias=bias, ref=ref, gather=gather, phase=phase)
    return _CACHE[name]


def _errs(got, ref):
    d = got.double() - ref
    return d.abs().max().item(), d.pow(2).mean().sqrt().item()


def _block_stats(rows):
    blk = rows.reshape(-1, 32, rows.shape[-1])
    return torch.stack([blk.sum(1), (blk * blk).sum(1)], 1)


def _image_order_rows(ref):
    return ref.permute(0, 2, 3, 1).reshape(-1, ref.shape[1])


def _phase_order_rows(ref):
    B, N, H2, W2 = ref.shape
    r = ref.reshape(B, N, H2 // 2, 2, W2 // 2, 2)            # b, n, y, a, x, b'
    return r.permute(0, 3, 5, 2, 4, 1).reshape(-1, N)        # (b, a, b', y, x) rows


@pytest.mark.parametrize("name", [c[0] for c in CASES if c[6]])
def test_phase_conv_error_within_twice_the_gather_path(engine, report, name):
    c = _case(engine, name)
    g_max, g_rms = _errs(c["gather"][0], c["ref"])
    p_max, p_rms = _errs(c["phase"][0], c["ref"])
    print("up_phase/%s gather max_abs %.6e rms %.6e | phase max_abs %.6e rms %.6e" % (name, g_max, g_rms, p_max, p_rms))
    report.add("up_phase/" + name, gather_max_abs=g_max, gather_rms=g_rms, phase_max_abs=p_max, phase_rms=p_rms)
    assert torch.isfinite(c["phase"][0]).all()
    assert g_max > 0 and g_rms > 0
    assert p_max <= 2.0 * g_max, (name, p_max, g_max)
    assert p_rms <= 2.0 * g_rms, (name, p_rms, g_rms)


@pytest.mark.parametrize("name,phase", [(c[0], c[6]) for c in CASES])
def test_dispatch_follows_the_image_size_and_the_switch(engine, name, phase):
    """The statistics blocks tell the paths apart: 32-row sums in (image, phase, y, x) row order on the phase path, in image
    order on the gather path. 8 x 8 must take the gather path whatever the switch says - and then both runs agree bit for bit."""
    c = _case(engine, name)
    want_img = _block_stats(_image_order_rows(c["ref"]))
    want_ph = _block_stats(_phase_order_rows(c["ref"]))
    scale = want_img.abs().max().item()
    assert (want_img - want_ph).abs().max().item() / scale > 0.05  # the two orders are told apart by far more than the tolerance

    def rel(st, want):
        return (st.double() - want).abs().max().item() / scale

    assert rel(c["gather"][1], want_img) < 2e-3
    if phase:
        assert rel(c["phase"][1], want_ph) < 2e-3 and rel(c["phase"][1], want_img) > 0.05
        assert not torch.equal(c["phase"][0], c["gather"][0])  # summed weights: some output rounds the other way
    else:
        assert rel(c["phase"][1], want_img) < 2e-3
        assert torch.equal(c["phase"][0], c["gather"][0]) and torch.equal(c["phase"][1], c["gather"][1])


@pytest.mark.parametrize("name", [c[0] for c in CASES if c[6]])
def test_groupnorm_mean_rstd_from_the_emitted_statistics(engine, report, name):
    """per image and group (32 groups): mean and 1 / sqrt(var + eps) from the sums the epilogue wrote, as k_gn_fold forms them,
    against float64 on the reference output; the tolerance of the fused statistics in test_gpu_ops.py (2e-3 of the largest)"""
    c = _case(engine, name)
    ref, st = c["ref"], c["phase"][1].double()
    B, N = ref.shape[:2]
    G, rows = 32, ref.shape[2] * ref.shape[3]
    cpg = N // G
    per_img = st.reshape(B, rows // 32, 2, N).sum(1)                 # all of an image's blocks
    s = per_img[:, 0].reshape(B, G, cpg).sum(2) / (rows * cpg)
    q = per_img[:, 1].reshape(B, G, cpg).sum(2) / (rows * cpg)
    mean, rstd = s, 1.0 / torch.sqrt(q - s * s + 1e-5)
    r = ref.reshape(B, G, cpg * rows)
    want_mean = r.mean(2)
    want_rstd = 1.0 / torch.sqrt(r.var(2, unbiased=False) + 1e-5)
    e_mean = (mean - want_mean).abs().max().item() / want_mean.abs().max().item()
    e_rstd = (rstd - want_rstd).abs().max().item() / want_rstd.abs().max().item()
    report.add("up_phase_gn/" + name, mean_rel=e_mean, rstd_rel=e_rstd)
    assert e_mean < 2e-3 and e_rstd < 2e-3, (name, e_mean, e_rstd)


@pytest.mark.parametrize("name", [c[0] for c in CASES if c[6]])
def test_reorder_pass_is_bit_exact(engine, name):
    """[b][2a+b'][y][x][C] -> [b][2y+a][2x+b'][C] on 16-bit values, against a pixel-shuffle style index map"""
    _, B, C, H, W, N, _ = next(c for c in CASES if c[0] == name)
    g = torch.Generator().manual_seed(17)
    x = r16(torch.randn(B, 4, N, H, W, generator=g))
    y = torch.empty((B, N, 2 * H, 2 * W), device="cuda", dtype=torch.float32)
    xs = _ops.dev(x)
    _ops.check(engine.lib.cd_op_up_phase_reorder(engine.h, _ops.ptr(xs), B, N, H, W, _ops.ptr(y)))
    torch.cuda.synchronize()
    want = x.reshape(B, 2, 2, N, H, W).permute(0, 3, 4, 1, 5, 2).reshape(B, N, 2 * H, 2 * W)
    assert torch.equal(y.cpu(), want)
