"""The DDIB / SDEdit baselines (gan_wrapper/baselines.py) on the engine, through their public wrappers, against the reference
fixtures of scripts/gen_golden_baselines.py (tests/golden/baselines_*.npz): the latent family on the small SD-shaped U-Net +
KL VAE in 16 bits and in fp32, the pixel family on two toy Ho-DDPMs in fp32. Also: cd_ddim_invert's trajectory, the DDIB
round trip, SDEdit's decode being cd_ddim_decode itself, and main.py on each new config."""
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

import _baselines_ref as br
import golden_util as gu
from cycle_diffusion_amd import _ffi, schedule
from cycle_diffusion_amd.gan_wrapper import baselines
from oracle import nets
from test_gpu_models import tiny_sd_desc, tiny_vae_desc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = 1.0 if _ffi.load_library().cd_act_format() == 1 else 8.0
# bounds of the existing tests of the same networks: images 40 dB (tests/test_gpu_wrappers.py); latents 2e-3 relative in fp32,
# in 16 bits the tiny SD U-Net's own forward bound, 8e-3 (tests/test_gpu_models.py)
LAT_REL = {"fp16": 8e-3 * FMT, "fp32": 2e-3}
PSNR_FLOOR = {"fp16": 40.0 if FMT == 1.0 else 25.0, "fp32": 40.0}
SRC, TGT = ["a photo of a cat", "a red car"], ["a photo of a dog", "a blue car"]


def _tiny(cls):
    class Tiny(cls):
        UNET_DESC = staticmethod(tiny_sd_desc)
        VAE_DESC = staticmethod(tiny_vae_desc)
        RESOLUTION = 64  # tiny VAE: factor 4 -> latent 16

        @staticmethod
        def checkpoint_path(source_model_type):
            return None
    return Tiny


class TableEmbedder:
    """the fixture's contexts by text: per-sample source / target rows, one unconditional row for ''"""

    def __init__(self, p):
        B, s = p["B"], p["ctx_seeds"]
        c_src, c_tgt = gu.rnd((B, 77, 64), s[0]), gu.rnd((B, 77, 64), s[1])
        self.table = {"": gu.rnd((1, 77, 64), s[2])[0]}
        for i in range(B):
            self.table[SRC[i]], self.table[TGT[i]] = c_src[i], c_tgt[i]

    def __call__(self, texts):
        return torch.stack([self.table[t] for t in texts], 0)


def _latent(cls, prec, monkeypatch, **kw):
    monkeypatch.setenv("CYCLEDIFF_SYNTHETIC_WEIGHTS", "1")
    fx = gu.load("baselines_latent")
    p = json.loads(str(fx["params"]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w = _tiny(cls)(source_model_type="none", custom_steps=p["S"], cond_stage=TableEmbedder(p), noise_on_cpu=True,
                       precision=prec, **kw)
    usd = br.synth_weights(json.loads(str(fx["unet_names"])), p["unet_seed"], p["out_prefix"], p["out_scale"])
    vsd = nets.synth_state_dict(json.loads(str(fx["vae_names"])), p["vae_seed"])
    assert w.engine.load_state_dict(w.unet, usd)[0] == 0 and w.engine.load_state_dict(w.vae, vsd)[0] == 0
    image = torch.rand((p["B"], 3, 64, 64), generator=torch.Generator().manual_seed(p["image_seed"])).cuda()
    return w, fx, p, image


def _rel(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return ((a - b).norm() / b.norm()).item()


FAMILIES = [("sd", baselines.SDDDIBTextWrapper, baselines.SDSDEditTextWrapper),
            ("ldm", baselines.LatentDiffDDIBTextWrapper, baselines.LatentDiffSDEditTextWrapper)]


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("fam", FAMILIES, ids=["sd", "ldm"])
def test_latent_ddib_vs_reference_fixture(monkeypatch, report, fam, prec):
    mode, ddib, _sde = fam
    w, fx, p, image = _latent(ddib, prec, monkeypatch, encoder_unconditional_guidance_scales=[1.0],
                              decoder_unconditional_guidance_scales=[3.0], skip_steps=[0])
    assert p["enc_scale"] == 1.0 and p["dec_scale"] == 3.0
    torch.manual_seed(p["noise_seed"])
    with torch.no_grad():
        z = w.encode(image, SRC)
        img = w(z, image, SRC, TGT)
    assert len(z) == 1 and z[0].shape == (2, 4 * 16 * 16)
    rz = _rel(z[0].view(2, 4, 16, 16), fx[mode + "_ddib_xT"])
    rx = _rel(w.last_latents[0], fx[mode + "_ddib_x"])
    ps = gu.psnr(img, torch.as_tensor(fx[mode + "_ddib_img"]))
    report.add("baselines/ddib_%s_%s" % (mode, prec), xT_rel=rz, x_rel=rx, psnr_db=ps)
    assert rz < LAT_REL[prec] and rx < LAT_REL[prec] and ps > PSNR_FLOOR[prec], (rz, rx, ps)


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("fam", FAMILIES, ids=["sd", "ldm"])
def test_latent_sdedit_vs_reference_fixture(monkeypatch, report, fam, prec):
    mode, _ddib, sde = fam
    w, fx, p, image = _latent(sde, prec, monkeypatch, eta=0.1, sdedit_strengths=[0.5],
                              decoder_unconditional_guidance_scales=[3.0])
    assert p["eta"] == 0.1 and p["strength"] == 0.5
    t_enc = int(0.5 * p["S"])
    torch.manual_seed(p["noise_seed"])
    with torch.no_grad():
        z = w.encode(image, SRC)
        img = w(z, image, SRC, TGT)
    assert len(z) == 1 and z[0].shape == (2, (t_enc + 1) * 4 * 16 * 16)
    zz = z[0].view(2, t_enc + 1, 4, 16, 16)
    rz = _rel(zz[:, 0], fx[mode + "_sdedit_zt"])
    rx = _rel(w.last_latents[0], fx[mode + "_sdedit_x"])
    ps = gu.psnr(img, torch.as_tensor(fx[mode + "_sdedit_img"]))
    report.add("baselines/sdedit_%s_%s" % (mode, prec), zt_rel=rz, x_rel=rx, psnr_db=ps)
    assert rz < LAT_REL[prec] and rx < LAT_REL[prec] and ps > PSNR_FLOOR[prec], (rz, rx, ps)
    # the noise slots are the reference's draws in its order: the posterior's (SD), randn_like(z0), then one per decode step
    torch.manual_seed(p["noise_seed"])
    if mode == "sd":
        torch.randn(2, 4, 16, 16)
    torch.randn(2, 4, 16, 16)
    want = torch.stack([torch.randn(2, 4, 16, 16) for _ in range(t_enc)], 1)
    assert torch.equal(zz[:, 1:].cpu(), want)


def test_sdedit_decode_is_cd_ddim_decode_bit_for_bit(monkeypatch):
    w, fx, p, image = _latent(baselines.SDSDEditTextWrapper, "fp16", monkeypatch, eta=0.1, sdedit_strengths=[0.5],
                              decoder_unconditional_guidance_scales=[3.0])
    t_enc = int(0.5 * p["S"])
    torch.manual_seed(p["noise_seed"])
    with torch.no_grad():
        z = w.encode(image, SRC)
        w(z, image, SRC, TGT)
        c, uc = w.get_condition(TGT, 2)
        _start, rows = schedule.DDIMSchedule(w.alphas_cumprod, p["S"], 0.1).coef_sdedit(t_enc)
        x = w.engine.ddim_decode(w.unet, _ffi.CD_SCHED_DDIM, z[0].view(2, t_enc + 1, 4, 16, 16).contiguous(), rows,
                                 n_eps=t_enc, ctx_c=c, ctx_uc=uc, guidance=3.0)
    w.engine.synchronize()
    assert torch.equal(x, w.last_latents[0])


@pytest.mark.parametrize("prec", ["fp32"])
def test_ddim_invert_trajectory_and_round_trip(monkeypatch, report, prec):
    """cd_ddim_invert step by step against the fixture's inversion trajectory, and the DDIB round trip (same text, scale 1
    both ways) reconstructing z0 within 2x of the reference's own CPU round-trip error"""
    w, fx, p, image = _latent(baselines.SDDDIBTextWrapper, prec, monkeypatch, encoder_unconditional_guidance_scales=[1.0],
                              decoder_unconditional_guidance_scales=[1.0], skip_steps=[0])
    z0_ref = torch.as_tensor(fx["sd_z0"]).cuda()
    c, uc = w.get_condition(SRC, 2)
    sch = schedule.DDIMSchedule(w.alphas_cumprod, p["S"], 0.0)
    with torch.no_grad():
        xT, traj = w.engine.ddim_invert(w.unet, z0_ref, sch.coef_invert(0), ctx_c=c, ctx_uc=uc, guidance=1.0, trajectory=True)
    steps = [_rel(traj[j], fx["sd_ddib_traj"][j]) for j in range(p["S"])]
    assert torch.equal(traj[-1], xT)
    assert max(steps) < LAT_REL[prec], steps
    torch.manual_seed(p["noise_seed"])
    with torch.no_grad():
        z0 = w._first_stage(image)
        torch.manual_seed(p["noise_seed"])  # the same posterior draw as z0's
        z = w.encode(image, SRC)
        w.generate(z, SRC)
    err = (w.last_latents[0] - z0).abs().max().item()
    ref_err = float(fx["sd_rt_err_max"])
    # the setting is well conditioned: the reference's own round trip closes to a small fraction of |z0|
    assert ref_err < 0.1 * float(np.abs(fx["sd_z0"]).max()), ref_err
    # and the bound separates: the same x_T decoded under the target text (CFG 3, the fixture's translation) misses z0 by more
    w.decoder_unconditional_guidance_scales = [3.0]
    with torch.no_grad():
        w.generate(z, TGT)
    err_tgt = (w.last_latents[0] - z0).abs().max().item()
    report.add("baselines/ddib_round_trip_%s" % prec, engine_err=err, reference_err=ref_err, target_text_err=err_tgt,
               worst_step_rel=max(steps))
    assert err <= 2.0 * ref_err < err_tgt, (err, ref_err, err_tgt)
    # rows with sigma != 0 are refused
    bad = sch.coef_invert(0)
    bad["sigma"][3] = 0.1
    with pytest.raises(RuntimeError, match="sigma"):
        w.engine.ddim_invert(w.unet, z0_ref, bad, ctx_c=c)


def _pixel(cls, monkeypatch, **kw):
    monkeypatch.setenv("CYCLEDIFF_SYNTHETIC_WEIGHTS", "1")
    fx = gu.load("baselines_pixel")
    p = json.loads(str(fx["params"]))
    out = []
    for side in ("src", "tgt"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            w = cls(source_model_type="toy32", custom_steps=p["custom_steps"], es_steps=p["es_steps"], noise_on_cpu=True,
                    **kw)
        sd = br.synth_weights(json.loads(str(fx[side + "_names"])), p[side + "_seed"], p["out_prefix"], p["out_scale"])
        assert w.engine.load_state_dict(w.net, sd)[0] == 0
        out.append(w)
    img = torch.rand((1, 3, 32, 32), generator=torch.Generator().manual_seed(p["image_seed"])).cuda()
    return out[0], out[1], fx, p, img


def _max_rel(a, b):
    """max |a - b| / max |b|, the metric of the existing fp32 pixel-chain tests (tests/test_gpu_f32_path.py)"""
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


def test_pixel_ddib_vs_reference_fixture(monkeypatch, report):
    src, tgt, fx, p, img = _pixel(baselines.DDPMDDIBWrapper, monkeypatch, sample_type="ddim")
    assert src.precision == "fp32"
    with torch.no_grad():
        z = src.encode(img)
        x = tgt.generate(z, None)  # unclamped, before the post-process
        out = tgt(z)
        rt = src.generate(z, None)
    rz = _max_rel(z.view(1, 3, 32, 32), fx["ddib_xT"])
    rx = _max_rel(x, fx["ddib_x"])
    ps = gu.psnr(out, torch.as_tensor(fx["ddib_img"]))
    x0 = img * 2 - 1
    rt_err, ref_rt = (rt - x0).abs().max().item(), float(fx["rt_err_max"])
    tgt_err = (x - x0).abs().max().item()
    report.add("baselines/ddib_pixel_fp32", xT_max_rel=rz, x_max_rel=rx, psnr_db=ps, round_trip_err=rt_err, reference_rt=ref_rt,
               target_model_err=tgt_err)
    assert z.shape == (1, 3 * 32 * 32) and rz < 1e-3 and rx < 1e-3 and ps >= 40.0, (rz, rx, ps)
    # a well-conditioned round trip (the reference's closes to a few % of |x0| <= 1), and a bound that the target model misses
    assert ref_rt < 0.1 and rt_err <= 2.0 * ref_rt < tgt_err, (rt_err, ref_rt, tgt_err)


def test_pixel_sdedit_vs_reference_fixture(monkeypatch, report):
    src, tgt, fx, p, img = _pixel(baselines.DDPMSDEditWrapper, monkeypatch, sample_type="ddim", eta=0.1,
                                  sdedit_strengths=[0.5])
    assert p["eta"] == 0.1 and src.i_s == int(fx["i_s"])
    torch.manual_seed(p["noise_seed"])
    with torch.no_grad():
        z = src.encode(img)
        x = tgt.generate(z, None)  # unclamped, before the post-process
    rz = _max_rel(z.view(1, 3, 32, 32), fx["sdedit_xt"])
    rx = _max_rel(x, fx["sdedit_x"])
    ps = gu.psnr((x + 1.0) / 2.0, torch.as_tensor(fx["sdedit_img"]))
    report.add("baselines/sdedit_pixel_fp32", xt_max_rel=rz, x_max_rel=rx, psnr_db=ps)
    assert rz < 1e-6 and rx < 1e-3 and ps >= 40.0, (rz, rx, ps)


CFGS = ["bench_sd_c2_ddib", "bench_sd_c2_sdedit", "bench_ldm_c3_ddib", "bench_ldm_c3_sdedit", "bench_afhq_c5_ddib",
        "bench_afhq_c5_sdedit"]


@pytest.mark.parametrize("cfg", CFGS)
def test_main_runs_each_baseline_config(tmp_path, monkeypatch, cfg):
    from PIL import Image
    monkeypatch.setenv("CYCLEDIFF_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.delenv("CYCLEDIFF_CLIP_RANKER", raising=False)
    res = 512 if "sd_c2" in cfg else 256
    rng = np.random.RandomState(7)
    Image.fromarray(rng.randint(0, 255, (64, 64, 3), dtype=np.uint8)).resize((res, res), Image.BICUBIC).save(tmp_path / "im.png")
    row = {"img_path": "im.png"} if "afhq" in cfg else {"img_path": "im.png", "encode_text": "a cat", "decode_text": "a dog"}
    (tmp_path / "data.json").write_text(json.dumps([row]))
    sys.path.insert(0, ROOT)
    import main as driver
    out = tmp_path / "out"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert driver.main(["--cfg", "experiments/%s.cfg" % cfg, "--data", str(tmp_path / "data.json"), "--output_dir",
                            str(out), "--per_device_eval_batch_size", "1", "--synthetic-weights"]) == 0
    m = json.loads((out / "metrics.json").read_text())
    assert len(m["samples"]) == 1 and np.isfinite(m["summary"]["psnr"])
    assert (out / "000000.png").exists()
