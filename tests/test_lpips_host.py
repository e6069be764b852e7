"""CPU: the host side of LPIPS (engine.py's checkpoint mapping and synthetic weights, utils/lpips.py's loader) and the
float64 restatement tests/_lpips_ref.py itself - including the two checks that make the GPU tests discriminate: folding the
scaling layer into the first conv is visibly wrong on the border, and the one-pass expansion of the distance cancels in fp32."""
import pytest
import torch

import _lpips_ref as lr

from cycle_diffusion_amd import engine as E

BF16_TOL = 6e-2  # tests/test_gpu_inception_fid.py _tol() of the bf16 build, the looser of the two


@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_both_checkpoint_layouts_map_to_the_engine_naming(net):
    sd = E.lpips_synthetic_state_dict(net, 1)
    full = lr.full_package_sd(net, sd)
    assert any(k.startswith("lins.") for k in full) and "scaling_layer.shift" in full
    got = E.lpips_engine_state_dict(full)
    assert set(got) == set(sd) and all(got[k] is sd[k] for k in sd)
    # a torchvision backbone state_dict plus the package's linear file
    two = {k: v for k, v in sd.items() if k.startswith("features.")}
    two["classifier.1.weight"], two["classifier.1.bias"] = torch.zeros(8, 8), torch.zeros(8)
    two.update({"lin%d.model.1.weight" % l: sd["lin%d.weight" % l] for l in range(5)})
    got = E.lpips_engine_state_dict(two)
    assert set(got) == set(sd) and all(got[k] is sd[k] for k in sd)
    # other scaling constants than the ones the engine applies are refused
    bad = dict(full)
    bad["scaling_layer.shift"] = torch.zeros(1, 3, 1, 1)
    with pytest.raises(AssertionError):
        E.lpips_engine_state_dict(bad)


def test_synthetic_state_dict_shapes():
    want = {"alex": ([(64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3)],
                     [64, 192, 384, 256, 256]),
            "vgg": ([(64, 3, 3, 3), (64, 64, 3, 3), (128, 64, 3, 3), (128, 128, 3, 3), (256, 128, 3, 3), (256, 256, 3, 3),
                     (256, 256, 3, 3), (512, 256, 3, 3)] + [(512, 512, 3, 3)] * 5, [64, 128, 256, 512, 512])}
    for net, (convs, taps) in want.items():
        sd = E.lpips_synthetic_state_dict(net, 0)
        layers = E.lpips_layers(net)
        assert [tuple(sd["features.%d.weight" % l[0]].shape) for l in layers] == convs
        assert [tuple(sd["features.%d.bias" % l[0]].shape) for l in layers] == [(c[0],) for c in convs]
        assert [tuple(sd["lin%d.weight" % l].shape) for l in range(5)] == [(1, c, 1, 1) for c in taps]
        assert len(sd) == 2 * len(convs) + 5
        for l, c in enumerate(taps):
            w = sd["lin%d.weight" % l]
            assert float(w.min()) >= 0.0 and 0.5 / c < float(w.mean()) < 2.0 / c
        assert [s[0] for s in E.lpips_tap_shapes(net, 64, 64)] == taps
    assert E.lpips_tap_shapes("alex", 31, 31)[-1] == (256, 1, 1) and E.lpips_tap_shapes("alex", 30, 30)[-1][1] < 1
    assert E.lpips_tap_shapes("vgg", 16, 16)[-1] == (512, 1, 1) and E.lpips_tap_shapes("vgg", 15, 15)[-1][1] < 1
    assert E.lpips_desc("alex").num_res_blocks == 5 and E.lpips_desc("vgg").num_res_blocks == 13
    with pytest.raises(ValueError):
        E.lpips_desc("squeeze")


def test_pair_footprint_counts_the_stages():
    # vgg at 32 x 32, per image in elements: input 32*32*32; stage 0 holds pool0 (64*16*16) + two 64*32*32 maps at its peak
    per_image = 32 * 32 * 32 + 64 * 16 * 16 + 2 * 64 * 32 * 32
    assert E.lpips_pair_bytes("vgg", 32, 32) == 2 * 2 * per_image
    assert E.lpips_pair_bytes("vgg", 512, 512) > E.lpips_pair_bytes("alex", 512, 512)


def test_loader_without_weights_says_what_to_pass(monkeypatch):
    from cycle_diffusion_amd.utils import lpips
    monkeypatch.delenv("CYCLEDIFF_LPIPS_WEIGHTS", raising=False)
    monkeypatch.setenv("CYCLEDIFF_SYNTHETIC_WEIGHTS", "0")
    with pytest.raises(FileNotFoundError, match="CYCLEDIFF_LPIPS_WEIGHTS"):
        lpips.load_lpips(None, "alex")


@pytest.mark.parametrize("net,H,W", [("alex", 67, 75), ("vgg", 40, 48)])
def test_restatement_zero_symmetric_non_negative(net, H, W):
    sd = {k: v.double() for k, v in E.lpips_synthetic_state_dict(net, 2).items()}
    x0 = lr.lowpass(2, 0, H, W).double()
    x1 = (x0 + 0.3 * lr.lowpass(2, 1, H, W).double()).clamp(-1, 1)
    with torch.no_grad():
        same = lr.lpips(sd, net, x0, x0)
        (d01, l01), t0, _ = lr.lpips(sd, net, x0, x1, per_layer=True, return_taps=True)
        d10 = lr.lpips(sd, net, x1, x0)
    assert torch.equal(same, torch.zeros(2, dtype=torch.float64))
    assert torch.equal(d01, d10)
    assert bool((l01 >= 0).all()) and bool((d01 > 0).all())
    assert [tuple(t.shape[1:]) for t in t0] == E.lpips_tap_shapes(net, H, W)


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_folded_scaling_is_wrong_on_the_border():
    """the low-contrast input of the GPU border test: a kernel that folds the scaling layer into conv 0 is off by far more than
    the 16-bit tolerance on the outermost ring of tap 0, so that test tells the two apart"""
    sd = {k: v.double() for k, v in E.lpips_synthetic_state_dict("vgg", 2).items()}
    x = 0.05 * lr.lowpass(3, 0, 40, 48).double()
    with torch.no_grad():
        ref = lr.taps(sd, "vgg", x)[0]
        fold = lr.taps(sd, "vgg", x, fold_scaling=True)[0]
        bf = lr.taps(sd, "vgg", x, round_fn=lambda t: lr.round16(t, False))[0]
    inner = _rel(fold[:, :, 2:-2, 2:-2], ref[:, :, 2:-2, 2:-2])
    ring = _rel(lr.border_ring(fold), lr.border_ring(ref))
    ring_bf16 = _rel(lr.border_ring(bf), lr.border_ring(ref))
    print("folded scaling layer: inner %.2e, border ring %.3f; bf16 storage on the ring %.2e" % (inner, ring, ring_bf16))
    assert inner < 1e-12
    assert ring >= 5 * BF16_TOL
    assert ring_bf16 < BF16_TOL


@pytest.mark.parametrize("fp16", [True, False], ids=["fp16", "bf16"])
def test_one_pass_form_cancels_in_float32(fp16):
    f0, f1, w = lr.near_identical_maps(fp16)
    a, b = f0.permute(0, 2, 1), f1.permute(0, 2, 1)
    ref = lr.layer_distance(a, b, w)
    two = lr.layer_distance(a.float(), b.float(), w.float()).double()
    one = lr.layer_distance_one_pass(a.float(), b.float(), w.float()).double()
    e2, e1 = float(((two - ref) / ref).abs().max()), float(((one - ref) / ref).abs().max())
    print("near-identical maps (%s): d = %.3e, float32 two-step off by %.1e, one-pass off by %.1e"
          % ("fp16" if fp16 else "bf16", float(ref), e2, e1))
    assert e2 < 1e-5
    assert e1 > 1e-4
