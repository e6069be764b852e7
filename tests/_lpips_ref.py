"""Torch restatement of LPIPS v0.1 (the `lpips` package, neither it nor torchvision is installed): scaling layer, the
AlexNet / VGG16 `features` stacks in literal order (scale, zero-padded conv, ReLU, pool), unit-normalisation over channels
with eps 1e-10 added to the norm, 1 x 1 `lin` weights, spatial mean, sum over the five taps. Runs in the dtype of its inputs
(the tests call it in float64, test 9 in float32 on the GPU). State_dicts use the engine's naming (`features.N.*`,
`lin{l}.weight`)."""
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)

# (features index, kernel, stride, pad, pool ahead of it (0 / 2 / 3), tap or -1)
ALEX = ((0, 11, 4, 2, 0, 0), (3, 5, 1, 2, 3, 1), (6, 3, 1, 1, 3, 2), (8, 3, 1, 1, 0, 3), (10, 3, 1, 1, 0, 4))
_VGG_TAPS = {2: 0, 7: 1, 14: 2, 21: 3, 28: 4}
VGG = tuple((i, 3, 1, 1, 2 if i in (5, 10, 17, 24) else 0, _VGG_TAPS.get(i, -1))
            for i in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28))
LAYERS = {"alex": ALEX, "vgg": VGG}


def scaling(x):
    shift = torch.tensor(SHIFT, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    return (x - shift) / scale


def taps(sd, net, x, fold_scaling=False, round_fn=None):
    """the five un-normalised ReLU outputs for x [B, 3, H, W] in [-1, 1]. fold_scaling: the scaling layer folded into the
    first conv's weights and bias (w / scale, b - sum w shift / scale) - equal inside the image, WRONG on the border, where
    the reference pads the scaled image with zeros; only the host check uses it. round_fn: applied to the scaled input and to
    every stored activation (a model of 16-bit storage)."""
    rf = round_fn or (lambda t: t)
    cast = lambda t: t.to(dtype=x.dtype, device=x.device)
    out = []
    h = x if fold_scaling else rf(scaling(x))
    for n, (idx, k, stride, pad, pool, tap) in enumerate(LAYERS[net]):
        if pool == 3:
            h = F.max_pool2d(h, 3, 2)
        elif pool == 2:
            h = F.max_pool2d(h, 2, 2)
        w, b = cast(sd["features.%d.weight" % idx]), cast(sd["features.%d.bias" % idx])
        if n == 0 and fold_scaling:
            shift = torch.tensor(SHIFT, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
            scale = torch.tensor(SCALE, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
            b = b - (w * shift / scale).sum(dim=(1, 2, 3))
            w = w / scale
        h = rf(F.relu(F.conv2d(h, w, b, stride=stride, padding=pad)))
        if tap >= 0:
            out.append(h)
    return out


def layer_distance(f0, f1, w):
    """one tap: f0, f1 [B, C, ...] (any trailing pixel dims), w [C] -> [B], the two-step form"""
    B, C = f0.shape[:2]
    a, b = f0.reshape(B, C, -1), f1.reshape(B, C, -1)
    n0 = a / (a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    n1 = b / (b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return ((n0 - n1).pow(2) * w.to(a.dtype).to(a.device).view(1, C, 1)).sum(1).mean(1)


def layer_distance_one_pass(f0, f1, w):
    """the expanded form sum w a^2 / |a|^2 + sum w b^2 / |b|^2 - 2 sum w a b / (|a| |b|): cancels when the maps are close"""
    B, C = f0.shape[:2]
    a, b = f0.reshape(B, C, -1), f1.reshape(B, C, -1)
    wv = w.to(a.dtype).to(a.device).view(1, C, 1)
    na = a.pow(2).sum(1).sqrt() + 1e-10
    nb = b.pow(2).sum(1).sqrt() + 1e-10
    t = (wv * a * a).sum(1) / (na * na) + (wv * b * b).sum(1) / (nb * nb) - 2 * (wv * a * b).sum(1) / (na * nb)
    return t.mean(1)


def lpips(sd, net, x0, x1, per_layer=False, return_taps=False, fold_scaling=False, round_fn=None):
    t0 = taps(sd, net, x0, fold_scaling, round_fn)
    t1 = taps(sd, net, x1, fold_scaling, round_fn)
    d = torch.stack([layer_distance(a, b, sd["lin%d.weight" % l].reshape(-1)) for l, (a, b) in enumerate(zip(t0, t1))], 1)
    total = d[:, 0]
    for l in range(1, 5):
        total = total + d[:, l]
    res = (total, d) if per_layer else total
    return (res, t0, t1) if return_taps else res


def round16(x, fp16):
    """round to the engine's 16-bit storage format and back (fp16 saturates at 65504)"""
    if fp16:
        return x.clamp(-65504.0, 65504.0).to(torch.float16).to(x.dtype)
    return x.to(torch.bfloat16).to(x.dtype)


def lowpass(n, seed, H, W, base=12, gain=1.0, offset=0.0):
    """seeded low-pass noise in (-1, 1), as tests/test_gpu_inception_fid.py's _lowpass makes it: base x base Gaussian noise,
    bicubic to H x W, tanh-squashed"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, base, base, generator=g)
    x = F.interpolate(x, size=(H, W), mode="bicubic", align_corners=False)
    return torch.tanh(gain * x + offset).contiguous()


def border_ring(t):
    """the outermost ring of [B, C, H, W] as [B, C, ring pixels]"""
    return torch.cat([t[:, :, 0, :], t[:, :, -1, :], t[:, :, 1:-1, 0], t[:, :, 1:-1, -1]], dim=2)


def full_package_sd(net, sd):
    """the engine-named synthetic weights re-keyed as a full lpips.LPIPS(net=...) state_dict"""
    out = {"scaling_layer.shift": torch.tensor(SHIFT).view(1, 3, 1, 1),
           "scaling_layer.scale": torch.tensor(SCALE).view(1, 3, 1, 1)}
    slice_of = {}
    k = 1
    for idx, _k, _s, _p, _pool, tap in LAYERS[net]:
        slice_of[idx] = k
        if tap >= 0:
            k += 1
    for name, v in sd.items():
        if name.startswith("features."):
            _, idx, kind = name.split(".")
            out["net.slice%d.%s.%s" % (slice_of[int(idx)], idx, kind)] = v
        else:
            l = name[3]
            out["lin%s.model.1.weight" % l] = v
            out["lins.%s.model.1.weight" % l] = v
    return out


def near_identical_maps(fp16, C=64, HW=1920, seed=5):
    """tap-0-like maps 1e-3 apart, both exactly representable in the storage format: [1, HW, C] float64 each, and w [C]"""
    g = torch.Generator().manual_seed(seed)
    f0 = round16(torch.relu(torch.randn(1, HW, C, generator=g, dtype=torch.float64) + 0.5), fp16)
    f1 = round16(f0 * (1 + 1e-3 * torch.randn(1, HW, C, generator=g, dtype=torch.float64)), fp16)
    w = (2.0 / C) * torch.rand(C, generator=g, dtype=torch.float64).float().double()
    return f0, f1, w
