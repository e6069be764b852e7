"""GPU: the FID Inception-v3 on the engine (csrc/inception.hip, cd_inception_features) against the torch restatement of the
same network (tests/_inception_ref.py) on seeded synthetic weights - block by block, across batch splits, and through the
FID / KID arithmetic of utils/fid.py; then main.py's --fid_ref_dir and --text_metrics on small runs."""
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
from cycle_diffusion_amd.engine import INCEPTION_BLOCKS
from cycle_diffusion_amd.utils import fid

import _ops
from _inception_ref import inception_fid_forward

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fp16():
    return _ffi.load_library().cd_act_format() == 1


def _tol():  # relative L2 error of pool3 (and of every block on the way)
    return 1e-2 if _fp16() else 6e-2


def _lowpass(n, seed, res=299, base=24, offset=0.0, gain=1.0):
    """seeded low-pass noise in the normalised input range: base x base Gaussian noise, bicubic to res, tanh-squashed"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, base, base, generator=g)
    x = F.interpolate(x, size=(res, res), mode="bicubic", align_corners=False)
    return torch.tanh(gain * x + offset).contiguous()


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module")
def eng():
    e = cda.Engine("cuda:0")
    sd = cda.inception_synthetic_state_dict(3)
    net = e.create_net(cda.inception_fid_desc())
    e.load_inception_state_dict(net, sd)
    yield e, net, sd
    e.close()


def test_param_names_and_shapes_match_the_state_dict(eng):
    e, net, sd = eng
    params = e.net_params(net)
    assert dict(params) == {k: tuple(v.shape) for k, v in sd.items()}
    assert len(params) == len(sd) == 94 * 5
    assert e.missing(net)[0] == 0
    # a checkpoint's extra tensors are skipped by the loader
    extra = dict(sd)
    extra["fc.weight"], extra["fc.bias"] = torch.zeros(1008, 2048), torch.zeros(1008)
    extra["Conv2d_1a_3x3.bn.num_batches_tracked"] = torch.tensor(0)
    e.load_inception_state_dict(net, extra)


def test_other_precisions_are_refused(eng):
    e, _, _ = eng
    d = cda.inception_fid_desc()
    d.precision = _ffi.CD_PREC_F32
    with pytest.raises(_ffi.EngineError, match="CD_PREC_16"):
        e.create_net(d)


def test_block_by_block_parity(eng):
    e, net, sd = eng
    x = _lowpass(3, 0)
    with torch.no_grad():
        ref_pool3, ref_outs = inception_fid_forward(sd, x, return_all=True)
    errs = []
    for k, name in enumerate(INCEPTION_BLOCKS):
        y = e.inception_features(net, x.cuda(), stop_block=k).cpu()
        assert y.shape == ref_outs[k].shape, (name, y.shape, ref_outs[k].shape)
        errs.append((name, _rel(y, ref_outs[k])))
    p3 = e.inception_features(net, x.cuda()).cpu()
    errs.append(("pool3", _rel(p3, ref_pool3)))
    print("inception block parity (relative L2, %s): %s" % ("fp16" if _fp16() else "bf16",
                                                             ", ".join("%s %.2e" % t for t in errs)))
    assert all(np.isfinite(v) for _, v in errs)
    assert float(ref_pool3.abs().mean()) > 1e-2  # the synthetic weights keep the activations at scale
    bad = [(n, v) for n, v in errs if v > _tol()]
    assert not bad, bad


# The smallest batch at which all four 3 x 3 stem convs take the channel-major K order (conv_gemm.hip takes_channel_major: at
# least 64 x 64 stored pixels and 32 MiB of activation): Conv2d_1a (299 x 299 x 32 channels) from 6 images, Conv2d_2a / 2b
# (149 / 147 squared x 32) from 24 / 25, Conv2d_4a (73 x 73 x 96) from 33 - at 32 images its activation is 31.2 MiB.
# utils/fid.py feeds 64 images at a time.
STEM_CHM_BATCH = 33
STEM_3X3_BLOCKS = (0, 1, 2, 5)  # Conv2d_1a, 2a, 2b, 4a in the block list


def test_stem_convs_at_the_production_k_order(eng, report):
    """The block-by-block test runs 3 images, which is tap-major everywhere. Here every 3 x 3 stem conv runs channel-major
    (asserted through the launcher's read-back) and is held to test_channel_major_order's rule against the same images fed one
    at a time (tap-major, asserted): max|err| against the float64 restatement at most 2 x the tap-major run's + one fp32 ulp
    of max|ref|."""
    e, net, sd = eng
    n = STEM_CHM_BATCH
    x = _lowpass(n, 3).cuda()
    sd64 = {k: v.double().cuda() for k, v in sd.items()}
    failures = []
    for k in STEM_3X3_BLOCKS:
        with torch.no_grad():
            ref = inception_fid_forward(sd64, x.double(), stop_block=k)
        big = e.inception_features(net, x, stop_block=k)
        torch.cuda.synchronize()
        rb = _ops.last_gemm_config(e)
        assert rb["chm"] == 1, (INCEPTION_BLOCKS[k], rb)
        assert big.shape == ref.shape
        err_big = float((big.double() - ref).abs().max())
        err_one = 0.0
        for i in range(n):
            one = e.inception_features(net, x[i:i + 1], stop_block=k)
            torch.cuda.synchronize()
            rb1 = _ops.last_gemm_config(e)
            assert rb1["chm"] == 0, (INCEPTION_BLOCKS[k], i, rb1)
            err_one = max(err_one, float((one.double() - ref[i:i + 1]).abs().max()))
        ref_max = float(ref.abs().max())
        ulp = float(np.spacing(np.float32(ref_max)))
        ratio = err_big / max(err_one, 1e-30)
        print("inception stem %s at %d images: channel-major (tile %d) max_abs %.3e, one image at a time (tap-major) %.3e, "
              "ratio %.3f, max|ref| %.3f" % (INCEPTION_BLOCKS[k], n, rb["tile"], err_big, err_one, ratio, ref_max))
        report.add("inception_stem_chm/" + INCEPTION_BLOCKS[k], batch=n, tile_ran=rb["tile"], bk=rb["bk"], max_abs=err_big,
                   max_abs_tap_major=err_one, ratio=ratio, rel_l2=_rel(big, ref))
        if not (np.isfinite(err_big) and err_big <= 2.0 * err_one + ulp):
            failures.append((INCEPTION_BLOCKS[k], err_big, err_one))
        if not _rel(big, ref) <= _tol():
            failures.append((INCEPTION_BLOCKS[k], "relative L2", _rel(big, ref)))
    assert not failures, failures


def test_batch_splits_agree(eng):
    e, net, _ = eng
    x = _lowpass(48, 1).cuda()
    full = e.inception_features(net, x).cpu()
    split = torch.cat([e.inception_features(net, x[:17]), e.inception_features(net, x[17:])]).cpu()
    singles = torch.cat([e.inception_features(net, x[i:i + 1]) for i in (0, 23, 47)]).cpu()
    per = lambda a, b: max(_rel(a[i], b[i]) for i in range(a.shape[0]))
    e1, e2 = per(split, full), per(singles, full[[0, 23, 47]])
    print("inception batch splits: 17 + 31 vs 48 %.2e, single images vs 48 %.2e" % (e1, e2))
    assert e1 <= _tol() and e2 <= _tol(), (e1, e2)


def test_fid_kid_engine_vs_restatement(eng):
    e, net, sd = eng
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    sets = [_lowpass(256, 10, gain=1.0), _lowpass(256, 11, base=12, offset=0.3, gain=1.5)]
    sd_gpu = {k: v.cuda() for k, v in sd.items()}
    fe, fr = [], []
    for s in sets:
        fe.append(torch.cat([e.inception_features(net, s[i:i + 64].cuda()) for i in range(0, 256, 64)]).double().cpu().numpy())
        with torch.no_grad():
            fr.append(torch.cat([inception_fid_forward(sd_gpu, s[i:i + 32].cuda()) for i in range(0, 256, 32)])
                      .double().cpu().numpy())
    re_, rr = fid.fid_kid(fe[0], fe[1], seed=0), fid.fid_kid(fr[0], fr[1], seed=0)
    dfid = abs(re_["fid"] - rr["fid"]) / abs(rr["fid"])
    dkid = abs(re_["kid"] - rr["kid"]) / abs(rr["kid"])
    print("FID engine %.6g restatement %.6g (rel %.2e); KID engine %.6g restatement %.6g (rel %.2e); sqrtm imag %.1e"
          % (re_["fid"], rr["fid"], dfid, re_["kid"], rr["kid"], dkid, re_["fid_sqrtm_imag"]))
    assert np.isfinite(re_["fid"]) and rr["kid"] > 0
    tol = 1e-2 if _fp16() else 5e-2
    assert dfid <= tol and dkid <= tol, (dfid, dkid)


def _run_main(args):
    sys.path.insert(0, ROOT)
    import main as driver
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert driver.main(args) == 0


def test_main_fid_flags_on_the_c1_config(tmp_path, monkeypatch):
    from PIL import Image
    from cycle_diffusion_amd.runtime import get_engine
    monkeypatch.delenv("CYCLEDIFF_FID_INCEPTION", raising=False)
    monkeypatch.setenv("CYCLEDIFF_SYNTHETIC_WEIGHTS", "1")
    rng = np.random.RandomState(0)
    meta = []
    for i in range(5):
        Image.fromarray(rng.randint(0, 255, (40, 32, 3), dtype=np.uint8)).save(tmp_path / ("im%d.png" % i))
        meta.append({"img_path": "im%d.png" % i})
    (tmp_path / "data.json").write_text(json.dumps(meta))
    ref = tmp_path / "ref" / "sub"
    ref.mkdir(parents=True)
    for i in range(4):
        Image.fromarray(rng.randint(0, 255, (64, 64, 3), dtype=np.uint8)).save(ref / ("r%d.png" % i))
    base = ["--cfg", "experiments/toy_ddpm_c1.cfg", "--data", str(tmp_path / "data.json"), "--per_device_eval_batch_size", "2"]
    _run_main(base + ["--output_dir", str(tmp_path / "plain")])
    _run_main(base + ["--output_dir", str(tmp_path / "fid"), "--fid_ref_dir", str(tmp_path / "ref"),
                      "--fid_ref_stats", str(tmp_path / "ref.npz"), "--synthetic-weights"])
    plain = json.loads((tmp_path / "plain" / "metrics.json").read_text())
    res = json.loads((tmp_path / "fid" / "metrics.json").read_text())
    assert set(plain) == {"summary", "weights_origin", "samples"}
    assert set(plain["summary"]) == {"psnr", "ssim", "l2"}
    assert set(plain["samples"][0]) == {"sample_id", "psnr", "ssim", "l2"}
    assert set(res["samples"][0]) == set(plain["samples"][0])
    s = res["summary"]
    assert np.isfinite(s["fid"]) and np.isfinite(s["kid"]) and np.isfinite(s["fid_sqrtm_imag"])
    assert res["fid_eval"]["n_gen"] == 5 and res["fid_eval"]["n_ref"] == 4
    assert res["fid_eval"]["weights_origin"].startswith("synthetic")
    # the same numbers from utils/fid.py applied to engine features of the PNGs main.py wrote (in main.py's batches of 2)
    e = get_engine(torch.device("cuda", 0))
    net, _ = fid.load_inception(e)
    gen = [np.asarray(Image.open(tmp_path / "fid" / ("%06d.png" % i)).convert("RGB")) for i in range(5)]
    want = fid.fid_kid(fid.features_u8(e, net, gen, batch=2), fid.features_u8(e, net, fid.load_reference_images(
        str(tmp_path / "ref"), 32)))
    print("main.py C1: fid %.6g kid %.6g (direct: %.6g %.6g)" % (s["fid"], s["kid"], want["fid"], want["kid"]))
    assert abs(s["fid"] - want["fid"]) <= 1e-6 * max(1.0, abs(want["fid"]))
    assert abs(s["kid"] - want["kid"]) <= 1e-6 * max(1.0, abs(want["kid"]))
    assert np.load(tmp_path / "ref.npz")["features"].shape == (4, 2048)


def test_text_scores_match_the_ranker():
    from cycle_diffusion_amd.gan_wrapper.ranker import DirectionalCLIPHIP
    from cycle_diffusion_amd.runtime import get_engine
    from cycle_diffusion_amd.utils import text_metrics
    e = get_engine(torch.device("cuda", 0))
    ranker = DirectionalCLIPHIP(e, state_dict=None, seed=5)
    g = torch.Generator().manual_seed(2)
    img = (torch.rand(3, 3, 64, 64, generator=g) * 1.4 - 0.2).cuda()  # outside [0, 1]: the scores see it unclamped
    orig = torch.rand(3, 3, 64, 64, generator=g).cuda()
    enc, dec = ["a cat", "a dog", "a house"], ["a lion", "a wolf", "a castle"]
    clip, dclip = text_metrics.text_scores(ranker, img, orig, enc, dec)
    c2, d2 = ranker(img, orig, enc, dec)
    assert clip == [float(v) for v in c2.cpu()] and dclip == [float(v) for v in d2.cpu()]
    c3, _ = ranker(img.clamp(0, 1), orig, enc, dec)
    assert clip != [float(v) for v in c3.cpu()]


def test_main_text_metrics_on_a_short_text_run(tmp_path, monkeypatch):
    from PIL import Image
    monkeypatch.setenv("CYCLEDIFF_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.delenv("CYCLEDIFF_CLIP_RANKER", raising=False)
    rng = np.random.RandomState(4)
    meta = []
    for i in range(3):
        Image.fromarray(rng.randint(0, 255, (64, 64, 3), dtype=np.uint8)).resize((512, 512), Image.BICUBIC).save(
            tmp_path / ("im%d.png" % i))
        meta.append({"img_path": "im%d.png" % i, "encode_text": "source %d" % i, "decode_text": "target %d" % i})
    (tmp_path / "data.json").write_text(json.dumps(meta))
    _run_main(["--cfg", "experiments/bench_sd_c2.cfg", "--data", str(tmp_path / "data.json"), "--output_dir",
               str(tmp_path / "out"), "--per_device_eval_batch_size", "1", "--range", "0", "1", "--text_metrics",
               "--synthetic-weights"])
    res = json.loads((tmp_path / "out" / "metrics.json").read_text())
    assert len(res["samples"]) == 1
    r = res["samples"][0]
    assert np.isfinite(r["clip"]) and np.isfinite(r["d-clip"])
    assert res["summary"]["clip"] == r["clip"] and res["summary"]["d-clip"] == r["d-clip"]
    print("main.py --text_metrics: clip %.4f d-clip %.4f" % (r["clip"], r["d-clip"]))
