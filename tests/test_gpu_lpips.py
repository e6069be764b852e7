"""GPU: LPIPS on the engine (csrc/lpips.hip: cd_lpips, cd_lpips_tap, cd_op_lpips_layer, cd_op_pool2x2) against the float64
restatement tests/_lpips_ref.py on seeded synthetic weights, then main.py's --lpips. Figures go to the parity report under
lpips/.

The distance kernel's operands are staged the way the network stores them (row stride C + in_pad, NaN pad columns, a block of
0xFF guard rows behind the last row), so a read outside the operand shows as a NaN result.

Measured on MI355X (fp16 build / bf16 build; the table is in DESIGN.md section 19):
  k_lpips_layer vs float64   worst of the 72 cases 1.9e-7 / 1.4e-7 relative (bounds 1.7e-6 .. 3.4e-6); maps 1e-3 apart 2.0e-8 / 8.8e-7
  taps, relative L2          vgg 4.3e-4 .. 9.3e-4 / 3.6e-3 .. 7.1e-3, alex 3.6e-4 .. 6.1e-4 / 2.9e-3 .. 4.8e-3 (bounds 1e-2 / 6e-2)
  border ring at 0.05        vgg 4.2e-4 / 3.5e-3, alex 3.5e-4 / 2.7e-3
  cd_lpips                   total 8.9e-5 / 8.4e-4 (vgg), 4.6e-5 / 4.2e-4 (alex); worst layer 1.0e-3 / 1.4e-2 (bounds 1e-2 / 5e-2);
                             5 pairs at once, 2 + 3 and singles: the same bits
"""
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cycle_diffusion_amd as cda
from cycle_diffusion_amd import _ffi
from cycle_diffusion_amd._ffi import check, ptr
from cycle_diffusion_amd.engine import lpips_tap_shapes
from cycle_diffusion_amd.utils import lpips as ulpips

import _lpips_ref as lr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD_ROWS = 64
SIZES = {"vgg": (40, 48), "alex": (67, 75)}
SEED = 3


def _fp16():
    return _ffi.load_library().cd_act_format() == 1


def _fmt():
    return "fp16" if _fp16() else "bf16"


def _tol():  # relative L2 of a feature map: tests/test_gpu_inception_fid.py _tol()
    return 1e-2 if _fp16() else 6e-2


def _dtol():  # relative error of a distance: the FID test's bound
    return 1e-2 if _fp16() else 5e-2


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module")
def nets():
    e = cda.Engine("cuda:0")
    out = {}
    for name in ("alex", "vgg"):
        sd = cda.lpips_synthetic_state_dict(name, SEED)
        net = e.create_net(cda.lpips_desc(name))
        e.load_lpips_state_dict(net, sd)
        out[name] = (net, sd, {k: v.double() for k, v in sd.items()})
    yield e, out
    e.close()


_REFS = {}


def _images(name, amp=1.0):
    H, W = SIZES[name]
    return amp * lr.lowpass(3, 0, H, W)


def _ref_taps(name, sd64, amp=1.0):
    """float64 taps of the three test images, computed once per (backbone, amplitude)"""
    key = (name, amp)
    if key not in _REFS:
        with torch.no_grad():
            _REFS[key] = lr.taps(sd64, name, _images(name, amp).double())
    return _REFS[key]


# ------------------------------------------------------------------------------------------------ 1. declaration, refusals
@pytest.mark.parametrize("name", ["alex", "vgg"])
def test_params_match_the_state_dict_and_refusals(nets, name):
    e, out = nets
    net, sd, _ = out[name]
    params = e.net_params(net)
    assert dict(params) == {k: tuple(v.shape) for k, v in sd.items()}
    assert len(params) == len(sd) == (15 if name == "alex" else 31)
    assert e.missing(net)[0] == 0
    e.load_lpips_state_dict(net, lr.full_package_sd(name, sd))  # a full package checkpoint: lins.*, scaling_layer.* skipped
    assert e.missing(net)[0] == 0
    d = cda.lpips_desc(name)
    d.precision = _ffi.CD_PREC_F32
    with pytest.raises(_ffi.EngineError, match="CD_PREC_16"):
        e.create_net(d)
    small = 30 if name == "alex" else 15
    x = torch.zeros(1, 3, small, 64, device="cuda")
    with pytest.raises(_ffi.EngineError, match="minimum size is %d" % (small + 1)):
        e.lpips(net, x, x)
    with pytest.raises(_ffi.EngineError, match="minimum size is %d" % (small + 1)):
        e.lpips_tap(net, x.transpose(2, 3).contiguous(), 0)
    ok = torch.zeros(1, 3, small + 1, small + 1, device="cuda")
    assert e.lpips_tap(net, ok, 4).shape[2:] == (1, 1)
    assert float(e.lpips(net, ok, ok)) == 0.0
    with pytest.raises(_ffi.EngineError, match="at least one image"):
        check(e.lib.cd_lpips(e.h, net, ptr(ok), ptr(ok), 0, small + 1, small + 1, None, ptr(torch.zeros(1, device="cuda"))))


# ------------------------------------------------------------------------------------------------ the distance kernel alone
def op_layer(e, f0, f1, w, in_pad=0):
    """cd_op_lpips_layer: f0, f1 [B, HW, C], w [C] -> [B] on the host"""
    B, HW, C = f0.shape
    a, b, wv = (t.to("cuda", torch.float32).contiguous() for t in (f0, f1, w))
    out = torch.full((B,), float("nan"), device="cuda", dtype=torch.float32)
    check(e.lib.cd_op_lpips_layer(e.h, ptr(a), ptr(b), ptr(wv), B, HW, C, in_pad, ptr(out)))
    torch.cuda.synchronize()
    return out.cpu()


def _maps(B, HW, C, seed):
    """two independent ReLU-like maps, already rounded to the storage format, and non-negative weights of mean 1 / C"""
    g = torch.Generator().manual_seed(seed)
    f0 = lr.round16(torch.relu(torch.randn(B, HW, C, generator=g, dtype=torch.float64) + 0.5), _fp16())
    f1 = lr.round16(torch.relu(torch.randn(B, HW, C, generator=g, dtype=torch.float64) + 0.5), _fp16())
    w = ((2.0 / C) * torch.rand(C, generator=g)).double()
    return f0, f1, w


def _ref64(f0, f1, w):
    return lr.layer_distance(f0.permute(0, 2, 1), f1.permute(0, 2, 1), w)


@pytest.mark.parametrize("C", [64, 128, 192, 256, 384, 512])
def test_layer_kernel_against_float64(nets, report, C):
    """2. Bound: 20 x the error the restatement shows when evaluated in float32 on the CPU on the same inputs, never looser than
    1e-4 relative. The float32 error is taken as the largest over this width's cases (HW x B x in_pad): a single float32 value
    can land far closer to the float64 one than half an ulp by chance, which no float32 result can be held to."""
    e, _ = nets
    cases, e32 = [], 0.0
    for HW in (1, 35, 3969):
        for B in (1, 3):
            f0, f1, w = _maps(B, HW, C, 1000 * C + 10 * HW + B)
            ref = _ref64(f0, f1, w)
            d32 = _ref64(f0.float(), f1.float(), w.float()).double()
            e32 = max(e32, float(((d32 - ref) / ref).abs().max()))
            cases.append((HW, B, f0, f1, w, ref))
    bound = min(20.0 * e32, 1e-4)
    worst, failures = 0.0, []
    for HW, B, f0, f1, w, ref in cases:
        for in_pad in (0, 8):
            got = op_layer(e, f0, f1, w, in_pad).double()
            err = float(((got - ref) / ref).abs().max()) if bool(torch.isfinite(got).all()) else float("inf")
            print("lpips_layer C %d HW %d B %d in_pad %d: rel err %.2e (bound %.2e)" % (C, HW, B, in_pad, err, bound))
            worst = max(worst, err)
            if not err <= bound:
                failures.append((HW, B, in_pad, err))
    report.add("lpips/layer/c%d" % C, fmt=_fmt(), max_rel=worst, float32_restatement_rel=e32, bound=bound)
    assert not failures, (bound, failures)


def test_layer_kernel_refusals(nets):
    e, _ = nets
    for C, in_pad in ((60, 0), (520, 0), (64, 4)):
        f = torch.ones(1, 2, C)
        with pytest.raises(_ffi.EngineError):
            op_layer(e, f, f, torch.ones(C), in_pad)


def test_layer_kernel_properties(nets, report):
    """3. identity, symmetry, scale invariance, all-zero pixels, batch independence"""
    e, _ = nets
    f0, f1, w = _maps(3, 35, 192, 7)
    assert torch.equal(op_layer(e, f0, f0, w, 8), torch.zeros(3))
    ab, ba = op_layer(e, f0, f1, w), op_layer(e, f1, f0, w)
    assert float(((ab - ba).abs() / ab).max()) <= 1e-6
    twice = op_layer(e, f0, 2 * f0, w)  # 2 * f0 is exact in fp16 and bf16
    assert bool(torch.isfinite(twice).all()) and float(twice.max()) < 1e-6 * float(w.sum())
    # pixels that are all-zero in f0, in f1, in both
    z0, z1 = f0.clone(), f1.clone()
    z0[:, 3] = 0
    z1[:, 5] = 0
    z0[:, 9] = 0
    z1[:, 9] = 0
    z0[0], z1[1] = 0, 0  # and whole images
    got, ref = op_layer(e, z0, z1, w, 8).double(), _ref64(z0, z1, w)
    assert bool(torch.isfinite(got).all())
    err = float(((got - ref) / ref).abs().max())
    report.add("lpips/layer/zero_pixels", fmt=_fmt(), max_rel=err)
    assert err <= 1e-5, err  # a float32 two-step evaluation is at 1e-6 (tests/test_lpips_host.py)
    # a B = 3 call equals three B = 1 calls bit for bit, at one and at many workgroups per image
    for HW, C in ((35, 192), (3969, 64)):
        g0, g1, gw = _maps(3, HW, C, 11)
        whole = op_layer(e, g0, g1, gw)
        ones = torch.cat([op_layer(e, g0[i:i + 1], g1[i:i + 1], gw) for i in range(3)])
        assert torch.equal(whole, ones), (HW, C, whole, ones)


def test_layer_kernel_near_identical_maps(nets, report):
    """4. the cancellation guard: maps 1e-3 apart. A one-pass expansion is off by 5e-4 and more already in float32 on the host
    (tests/test_lpips_host.py); the two-step form stays at 1e-6."""
    e, _ = nets
    f0, f1, w = lr.near_identical_maps(_fp16())
    ref = _ref64(f0, f1, w)
    got = op_layer(e, f0, f1, w).double()
    err = float(((got - ref) / ref).abs().max())
    print("lpips_layer near-identical maps: d %.3e, rel err %.2e" % (float(ref), err))
    report.add("lpips/layer/near_identical", fmt=_fmt(), d=float(ref), rel=err)
    assert err <= 1e-4, err


# ------------------------------------------------------------------------------------------------ 5. the 2 x 2 pool
@pytest.mark.parametrize("H,W", [(7, 5), (12, 9)])
def test_pool2x2(nets, H, W):
    e, _ = nets
    B, C, off, ld, in_pad = 2, 64, 32, 128, 8
    g = torch.Generator().manual_seed(H)
    x = lr.round16(torch.randn(B, C, H, W, generator=g), _fp16())
    Ho, Wo = H // 2, W // 2
    y = torch.zeros((B * Ho * Wo + GUARD_ROWS, ld), device="cuda", dtype=torch.float32)
    xs = x.cuda().contiguous()
    check(e.lib.cd_op_pool2x2(e.h, ptr(xs), B, C, H, W, in_pad, off, ld, ptr(y)))
    torch.cuda.synchronize()
    y = y.cpu()
    rows = B * Ho * Wo
    inside = y[:rows, off:off + C]
    outside = y.clone()
    outside[:rows, off:off + C] = float("nan")
    assert bool(torch.isnan(outside).all()), "a store outside the slice"
    got = inside.reshape(B, Ho, Wo, C).permute(0, 3, 1, 2)
    assert torch.equal(got, F.max_pool2d(x, 2, 2))
    for kw in (dict(in_pad=4), dict(off=4), dict(ld=88 + 4), dict(off=96)):
        a = dict(in_pad=in_pad, off=off, ld=ld)
        a.update(kw)
        assert e.lib.cd_op_pool2x2(e.h, ptr(xs), B, C, H, W, a["in_pad"], a["off"], a["ld"], ptr(y.cuda())) != 0


# ------------------------------------------------------------------------------------------------ 6 / 7. the backbones
@pytest.mark.parametrize("name", ["vgg", "alex"])
def test_tap_parity(nets, report, name):
    e, out = nets
    net, _, sd64 = out[name]
    x = _images(name)
    ref = _ref_taps(name, sd64)
    errs = []
    for t in range(5):
        y = e.lpips_tap(net, x.cuda(), t).cpu()
        assert y.shape == ref[t].shape == (3,) + lpips_tap_shapes(name, *SIZES[name])[t]
        assert float(ref[t].abs().mean()) > 1e-2, (t, float(ref[t].abs().mean()))
        errs.append(_rel(y, ref[t]))
    print("lpips %s taps (relative L2, %s): %s" % (name, _fmt(), ", ".join("%.2e" % v for v in errs)))
    report.add("lpips/taps/" + name, fmt=_fmt(), **{"tap%d" % t: v for t, v in enumerate(errs)})
    assert all(np.isfinite(v) and v <= _tol() for v in errs), errs


@pytest.mark.parametrize("name", ["vgg", "alex"])
def test_border_ring_of_tap0_at_low_contrast(nets, report, name):
    """7. at amplitude 0.05 the scaling layer's shift dominates the input: a scaling layer folded into the first conv is off by
    0.4 on this ring (tests/test_lpips_host.py)"""
    e, out = nets
    net, _, sd64 = out[name]
    ref = _ref_taps(name, sd64, amp=0.05)[0]
    y = e.lpips_tap(net, _images(name, 0.05).cuda(), 0).cpu()
    err = _rel(lr.border_ring(y), lr.border_ring(ref))
    print("lpips %s tap 0 border ring at amplitude 0.05: %.2e" % (name, err))
    report.add("lpips/border/" + name, fmt=_fmt(), rel_l2=err)
    assert err <= _tol(), err


# ------------------------------------------------------------------------------------------------ 8. the distance
@pytest.mark.parametrize("name", ["vgg", "alex"])
def test_distance_against_float64(nets, report, name):
    e, out = nets
    net, _, sd64 = out[name]
    H, W = SIZES[name]
    x0 = lr.lowpass(5, 0, H, W)  # the first three are the tap tests' images
    x1 = (x0 + 0.3 * lr.lowpass(5, 1, H, W)).clamp(-1, 1)
    with torch.no_grad():
        ref, ref_l = lr.lpips(sd64, name, x0[:3].double(), x1[:3].double(), per_layer=True)
    a, b = x0.cuda(), x1.cuda()
    got, got_l = e.lpips(net, a[:3], b[:3], per_layer=True)
    got, got_l = got.double().cpu(), got_l.double().cpu()
    e_tot = float(((got - ref) / ref).abs().max())
    e_lay = [float(((got_l[:, l] - ref_l[:, l]) / ref_l[:, l]).abs().max()) for l in range(5)]
    print("lpips %s (%s): d %s, total rel %.2e, per layer %s" % (name, _fmt(), ["%.4f" % v for v in ref], e_tot,
                                                                 ", ".join("%.2e" % v for v in e_lay)))
    report.add("lpips/distance/" + name, fmt=_fmt(), total_rel=e_tot, **{"layer%d_rel" % l: v for l, v in enumerate(e_lay)})
    assert bool((ref > 0).all())
    assert e_tot <= _dtol() and all(v <= _dtol() for v in e_lay), (e_tot, e_lay)
    tap_sum = got_l[:, 0].float()
    for l in range(1, 5):
        tap_sum = tap_sum + got_l[:, l].float()
    assert torch.equal(tap_sum.double(), got)  # the total is the five terms added in tap order
    assert torch.equal(e.lpips(net, a, a).cpu(), torch.zeros(5))
    # 5 pairs in one call against 2 + 3 and against singles
    full = e.lpips(net, a, b).double().cpu()
    split = torch.cat([e.lpips(net, a[:2], b[:2]), e.lpips(net, a[2:], b[2:])]).double().cpu()
    singles = torch.cat([e.lpips(net, a[i:i + 1], b[i:i + 1]) for i in range(5)]).double().cpu()
    d1, d2 = float(((split - full) / full).abs().max()), float(((singles - full) / full).abs().max())
    print("lpips %s batch splits: 2 + 3 vs 5 %.2e, singles vs 5 %.2e" % (name, d1, d2))
    assert d1 <= _dtol() and d2 <= _dtol(), (d1, d2)


# ------------------------------------------------------------------------------------------------ 9. full-size pairs
@pytest.mark.parametrize("name,R", [("vgg", 512), ("alex", 256)])
def test_full_size_pair_against_float32_torch(nets, report, name, R):
    """the large-M tiles and the channel-major K order of the implicit GEMM run here; reference: the restatement in float32 torch
    on the GPU"""
    e, out = nets
    net, sd, _ = out[name]
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    x0 = lr.lowpass(1, 4, R, R, base=32).cuda()
    x1 = (x0 + 0.3 * lr.lowpass(1, 5, R, R, base=32).cuda()).clamp(-1, 1)
    sd_gpu = {k: v.cuda() for k, v in sd.items()}
    with torch.no_grad():
        ref, ref_l = lr.lpips(sd_gpu, name, x0, x1, per_layer=True)
    got, got_l = e.lpips(net, x0, x1, per_layer=True)
    e_tot = float(((got.double() - ref.double()) / ref.double()).abs().max())
    e_lay = [float(((got_l[:, l].double() - ref_l[:, l].double()) / ref_l[:, l].double()).abs().max()) for l in range(5)]
    print("lpips %s at %d x %d (%s): d %.4f, total rel %.2e, per layer %s" % (name, R, R, _fmt(), float(ref), e_tot,
                                                                             ", ".join("%.2e" % v for v in e_lay)))
    report.add("lpips/full_size/%s_%d" % (name, R), fmt=_fmt(), total_rel=e_tot, **{"layer%d_rel" % l: v for l, v in enumerate(e_lay)})
    assert e_tot <= _dtol() and all(v <= _dtol() for v in e_lay), (e_tot, e_lay)


# ------------------------------------------------------------------------------------------------ 10. the driver
def _run_main(args):
    sys.path.insert(0, ROOT)
    import main as driver
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert driver.main(args) == 0


def _png(path):
    from PIL import Image
    return torch.from_numpy(np.array(Image.open(path).convert("RGB"))).permute(2, 0, 1).float().div(255.0)[None]


def test_main_lpips_on_the_c1_config(tmp_path, monkeypatch):
    from PIL import Image
    from cycle_diffusion_amd.data.triplets import TripletDataset
    from cycle_diffusion_amd.runtime import get_engine
    monkeypatch.delenv("CYCLEDIFF_LPIPS_WEIGHTS", raising=False)
    monkeypatch.setenv("CYCLEDIFF_SYNTHETIC_WEIGHTS", "1")
    rng = np.random.RandomState(0)
    meta = []
    for i in range(3):
        Image.fromarray(rng.randint(0, 255, (40, 32, 3), dtype=np.uint8)).save(tmp_path / ("im%d.png" % i))
        meta.append({"img_path": "im%d.png" % i})
    (tmp_path / "data.json").write_text(json.dumps(meta))
    base = ["--cfg", "experiments/toy_ddpm_c1.cfg", "--data", str(tmp_path / "data.json"), "--per_device_eval_batch_size", "2"]
    _run_main(base + ["--output_dir", str(tmp_path / "plain")])
    _run_main(base + ["--output_dir", str(tmp_path / "lp"), "--lpips", "alex", "--synthetic-weights"])
    plain = json.loads((tmp_path / "plain" / "metrics.json").read_text())
    res = json.loads((tmp_path / "lp" / "metrics.json").read_text())
    assert set(plain) == {"summary", "weights_origin", "samples"}
    assert set(plain["summary"]) == {"psnr", "ssim", "l2"}
    assert set(plain["samples"][0]) == {"sample_id", "psnr", "ssim", "l2"}
    assert set(res) == set(plain) | {"lpips_eval"}
    assert set(res["summary"]) == set(plain["summary"]) | {"lpips"}
    assert all(set(r) == set(plain["samples"][0]) | {"lpips"} for r in res["samples"])
    assert res["lpips_eval"] == {"net": "alex", "weights_origin": "synthetic(seed=%d)" % ulpips.SYNTHETIC_SEED, "n": 3}
    vals = [r["lpips"] for r in res["samples"]]
    assert abs(res["summary"]["lpips"] - sum(vals) / 3) <= 1e-12
    # the same numbers from utils/lpips.py applied to the written PNG and the source image at the wrapper's resolution
    e = get_engine(torch.device("cuda", 0))
    net, _ = ulpips.load_lpips(e, "alex")
    ds = TripletDataset(str(tmp_path / "data.json"), 32, 0, None)
    for i, v in enumerate(vals):
        want = float(ulpips.distance(e, net, _png(tmp_path / "lp" / ("%06d.png" % i)), ds[i]["original_image"][None])[0])
        print("main.py --lpips alex sample %d: %.6f (direct %.6f)" % (i, v, want))
        assert np.isfinite(v) and v > 0 and abs(v - want) <= 1e-6 * max(1.0, abs(want)), (i, v, want)


def test_main_lpips_keep_on_a_masked_text_run(tmp_path, monkeypatch):
    from PIL import Image
    monkeypatch.delenv("CYCLEDIFF_LPIPS_WEIGHTS", raising=False)
    monkeypatch.delenv("CYCLEDIFF_CLIP_RANKER", raising=False)
    monkeypatch.setenv("CYCLEDIFF_SYNTHETIC_WEIGHTS", "1")
    rng = np.random.RandomState(7)
    Image.fromarray(rng.randint(0, 255, (64, 64, 3), dtype=np.uint8)).resize((512, 512), Image.BICUBIC).save(tmp_path / "im.png")
    m = np.zeros((512, 512), dtype=np.uint8)
    m[128:384, 64:256] = 255
    Image.fromarray(m).save(tmp_path / "mask.png")
    (tmp_path / "data.json").write_text(json.dumps([{"img_path": "im.png", "encode_text": "a cat", "decode_text": "a dog",
                                                     "mask_path": "mask.png"}]))
    # the masked text run of tests/test_gpu_masked.py on a tenth of its steps: the metric does not care how good the edit is
    cfg = open(os.path.join(ROOT, "config", "experiments", "bench_sd_c2.cfg")).read()
    assert "custom_steps = 99" in cfg and "white_box_steps = 100" in cfg
    (tmp_path / "short.cfg").write_text(cfg.replace("custom_steps = 99", "custom_steps = 9")
                                        .replace("white_box_steps = 100", "white_box_steps = 10"))
    _run_main(["--cfg", str(tmp_path / "short.cfg"), "--data", str(tmp_path / "data.json"), "--output_dir", str(tmp_path / "out"),
               "--per_device_eval_batch_size", "1", "--synthetic-weights", "--lpips", "alex"])
    res = json.loads((tmp_path / "out" / "metrics.json").read_text())
    (a,) = res["samples"]
    assert np.isfinite(a["lpips"]) and a["lpips"] > 0 and np.isfinite(a["lpips_keep"])
    assert res["summary"]["lpips_keep"] == a["lpips_keep"] and res["summary"]["lpips"] == a["lpips"]
    assert res["lpips_eval"]["n"] == 1
    # this project's definition: both PNG-quantised images times the keep-mask in [-1, 1] space
    from cycle_diffusion_amd.runtime import get_engine
    e = get_engine(torch.device("cuda", 0))
    net, _ = ulpips.load_lpips(e, "alex")
    keep = torch.from_numpy(m).float().div(255.0)[None, None]
    out_img, src = _png(tmp_path / "out" / "000000.png"), _png(tmp_path / "im.png")
    want = float(ulpips.distance_keep(e, net, out_img, src, keep)[0])
    print("main.py lpips %.6f lpips_keep %.6f (direct %.6f)" % (a["lpips"], a["lpips_keep"], want))
    assert abs(a["lpips_keep"] - want) <= 1e-6 * max(1.0, abs(want))
