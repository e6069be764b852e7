"""CPU: the phase form of a nearest-x2 3 x 3 convolution (csrc/conv_gemm.hip k_up_phase_weights and the
`up_phase` row decode of k_conv_gemm) restated in torch and held against the definition in float64.

    out[2y+a, 2x+b] = sum_{dy,dx in {0,1}} W_ab[dy][dx] . x[y + dy + a - 1, x + dx + b - 1]
    a = 0: rows {w0, w1 + w2}    a = 1: rows {w0 + w1, w2}    (columns alike with b)

A tap that falls into the zero padding of the upsampled grid falls outside the stored grid too, so the form is exact at
the borders. This pins the tap sums and the padding before any kernel runs."""
import torch
import torch.nn.functional as F


def phase_weights(w):
    """[N, C, 3, 3] -> [4, N, C, 2, 2], phase = 2 a + b: the sums k_up_phase_weights forms"""
    rows = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}  # parity -> filter taps behind stored-grid tap 0 / 1
    out = torch.zeros((4,) + tuple(w.shape[:2]) + (2, 2), dtype=w.dtype)
    for a in (0, 1):
        for b in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    for r in rows[a][dy]:
                        for s in rows[b][dx]:
                            out[2 * a + b, :, :, dy, dx] += w[:, :, r, s]
    return out


def phase_conv(x, w, bias=None):
    """the four 2 x 2 convs on the stored grid, first tap at (y + a - 1, x + b - 1), interleaved into the x2 image"""
    B, C, H, W = x.shape
    wp = phase_weights(w)
    y = torch.zeros((B, w.shape[0], 2 * H, 2 * W), dtype=x.dtype)
    for a in (0, 1):
        for b in (0, 1):
            xp = F.pad(x, (1 - b, b, 1 - a, a))  # (left, right, top, bottom): rows y + a - 1 .. y + a
            y[:, :, a::2, b::2] = F.conv2d(xp, wp[2 * a + b], bias)
    return y


def test_phase_form_equals_upsample_then_conv_in_float64():
    g = torch.Generator().manual_seed(5)
    for B, C, N, H, W in ((2, 3, 5, 4, 4), (1, 2, 2, 1, 1), (1, 4, 3, 2, 5)):
        x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
        w = torch.randn(N, C, 3, 3, generator=g, dtype=torch.float64)
        bias = torch.randn(N, generator=g, dtype=torch.float64)
        ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, bias, padding=1)
        got = phase_conv(x, w, bias)
        assert got.shape == ref.shape
        assert (got - ref).abs().max().item() < 1e-12, (B, C, N, H, W)


def test_phase_form_border_taps_see_the_padding():
    """an all-ones image and filter: the output counts the taps inside the upsampled grid - 4 at the corners, 6 on the
    edges, 9 inside - in both forms"""
    x = torch.ones(1, 1, 4, 4, dtype=torch.float64)
    w = torch.ones(1, 1, 3, 3, dtype=torch.float64)
    got = phase_conv(x, w)
    assert got[0, 0, 0, 0] == 4 and got[0, 0, 7, 7] == 4 and got[0, 0, 0, 3] == 6 and got[0, 0, 4, 7] == 6
    assert (got[0, 0, 1:7, 1:7] == 9).all()
    assert torch.equal(got, F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1))
