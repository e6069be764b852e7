"""CPU: the DDIB / SDEdit baselines (gan_wrapper/baselines.py) on the host side - their schedule rows, the torch restatement of
the four loops (tests/_baselines_ref.py) against the committed reference fixtures (scripts/gen_golden_baselines.py), the live
reference where it is mounted, the configs and the factory."""
import inspect
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

import _baselines_ref as br
import golden_util as gu
from cycle_diffusion_amd import schedule
from oracle import nets, ref_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["SDDDIBText", "SDSDEditText", "LatentDiffDDIBText", "LatentDiffSDEditText", "DDPM_DDIB", "DDPM_SDEdit"]


def _latent_setting():
    fx = gu.load("baselines_latent")
    p = json.loads(str(fx["params"]))
    usd = br.synth_weights(json.loads(str(fx["unet_names"])), p["unet_seed"], p["out_prefix"], p["out_scale"])
    unet = lambda x, t, c: nets.openai_unet(usd, gu.TINY_SD_CFG, x, t, c)
    B, s = p["B"], p["ctx_seeds"]
    c_src, c_tgt = gu.rnd((B, 77, 64), s[0]), gu.rnd((B, 77, 64), s[1])
    uc = gu.rnd((1, 77, 64), s[2]).expand(B, 77, 64).contiguous()
    return fx, p, unet, c_src, c_tgt, uc


def _rel(a, b):
    a, b = torch.as_tensor(a).float(), torch.as_tensor(b).float()
    return ((a - b).norm() / b.norm()).item()


def test_latent_rows():
    """coef_invert: row j = level a_prev[j] -> a[j] at the input level's timestep, sigma 0; coef_sdedit: the q-sample row of
    level t_enc and the decode rows t_enc-1 .. 0; the eta = 0 decode table has sigma 0 and sqrt(1 - a_prev) directions"""
    S = 20
    sch = schedule.DDIMSchedule(schedule.latent_alphas_cumprod(), S, 0.0)
    inv = sch.coef_invert(0)
    assert len(inv) == S and len(sch.coef_invert(5)) == S - 5
    assert list(inv["t"]) == [0] + [int(t) for t in sch.timesteps[:-1]]
    assert (inv["sigma"] == 0).all() and (inv["t_mask"] == 1).all()
    np.testing.assert_array_equal(inv["sa"], np.sqrt(sch.a_prev))
    np.testing.assert_array_equal(inv["r"], np.sqrt(np.float32(1) - sch.a_prev))
    np.testing.assert_array_equal(inv["sap"], np.sqrt(sch.a))
    np.testing.assert_array_equal(inv["dirc"], np.sqrt(np.float32(1) - sch.a))
    # chained levels: the output level of step j is the input level of step j + 1
    np.testing.assert_array_equal(inv["sap"][:-1], inv["sa"][1:])
    dec = sch.coef_decode(0)
    assert (dec["sigma"] == 0).all()
    np.testing.assert_array_equal(dec["dirc"], np.sqrt(np.float32(1) - sch.a_prev))
    sch1 = schedule.DDIMSchedule(schedule.latent_alphas_cumprod(), S, 0.1)
    start, rows = sch1.coef_sdedit(10)
    assert len(start) == 1 and start["sa"][0] == np.sqrt(sch1.a[10]) and start["s1a"][0] == sch1.r[10]
    np.testing.assert_array_equal(rows, sch1.coef_decode(0)[:10])
    for bad in (0, S):
        with pytest.raises(AssertionError):
            sch1.coef_sdedit(bad)
    # against the reference sampler's own tables stored in the fixture (make_schedule with ddim_eta 0 and 0.1)
    fx = gu.load("baselines_latent")
    S = json.loads(str(fx["params"]))["S"]
    sch0 = schedule.DDIMSchedule(schedule.latent_alphas_cumprod(), S, 0.0)
    inv, dec0 = sch0.coef_invert(0), sch0.coef_decode(0)
    ref_a, ref_ap = fx["ref_a"], fx["ref_a_prev"]
    assert list(inv["t"]) == [0] + [int(t) for t in fx["ref_t"][:-1]] and list(dec0["t"]) == [int(t) for t in fx["ref_t"]]
    np.testing.assert_array_equal(inv["sa"], np.sqrt(ref_ap))
    np.testing.assert_array_equal(inv["sap"], np.sqrt(ref_a))
    np.testing.assert_array_equal(inv["dirc"], np.sqrt(np.float32(1) - ref_a))
    np.testing.assert_array_equal(dec0["sap"], np.sqrt(ref_ap))
    sch1 = schedule.DDIMSchedule(schedule.latent_alphas_cumprod(), S, 0.1)
    np.testing.assert_array_equal(sch1.sigma, fx["ref_sigma_eta"])
    start, rows = sch1.coef_sdedit(S // 2)
    assert start["sa"][0] == np.sqrt(ref_a[S // 2])
    # the existing tables are what they were
    np.testing.assert_array_equal(sch1.coef_decode(3), schedule.DDIMSchedule(schedule.latent_alphas_cumprod(), S, 0.1).coef_decode(3))


def test_pixel_rows():
    sch = schedule.PixelSchedule(40, 40, sample_type="ddim", eta=0.0)
    inv = sch.coef_invert()
    assert len(inv) == 39 and list(inv["t"]) == sch.seq[:-1]
    assert (inv["sigma"] == 0).all() and np.isfinite(inv.view(np.float32).reshape(39, 8)[:, :7]).all()
    np.testing.assert_array_equal(inv["sap"], np.sqrt(sch.acp[sch.seq[1:]]))
    dec = sch.coef_decode_eta0()
    assert len(dec) == 40 and dec["sap"][0] == 1.0 and dec["dirc"][0] == 0.0 and (dec["sigma"] == 0).all()
    s1 = schedule.PixelSchedule(40, 40, sample_type="ddim", eta=0.1)
    i_s, start, rows = s1.coef_sdedit(0.5)
    assert i_s == 19 and start["sa"][0] == np.sqrt(s1.acp[s1.seq[19]])
    np.testing.assert_array_equal(rows, s1.coef_decode()[:20])
    fx = gu.load("baselines_pixel")
    p = json.loads(str(fx["params"]))
    sp = schedule.PixelSchedule(p["custom_steps"], p["es_steps"], sample_type="ddim", eta=0.0)
    assert sp.seq == [int(t) for t in fx["seq"]]  # generate()'s seq_inv, as the fixture's reference loops walked it
    assert list(sp.coef_invert()["t"]) == sp.seq[:-1] and sp.coef_sdedit(p["strength"])[0] == int(fx["i_s"])


def test_latent_restatement_reproduces_the_fixture():
    fx, p, unet, c_src, c_tgt, uc = _latent_setting()
    S = p["S"]
    with torch.no_grad():
        for mode in ("sd", "ldm"):
            z0 = torch.as_tensor(fx[mode + "_z0"])
            sch0 = schedule.DDIMSchedule(schedule.latent_alphas_cumprod(), S, 0.0)
            xT, traj = br.latent_ddib_invert(br.cfg_eps(unet, c_src, uc, p["enc_scale"]), z0, sch0)
            assert _rel(xT, fx[mode + "_ddib_xT"]) < 1e-5
            if mode == "sd":
                assert max(_rel(a, b) for a, b in zip(traj, fx["sd_ddib_traj"])) < 1e-5
            x = br.latent_decode(br.cfg_eps(unet, c_tgt, uc, p["dec_scale"]), torch.as_tensor(fx[mode + "_ddib_xT"]), sch0, S)
            assert _rel(x, fx[mode + "_ddib_x"]) < 1e-5
            # SDEdit: the draws continue after the posterior's (SD) from the fixture's seed
            sch = schedule.DDIMSchedule(schedule.latent_alphas_cumprod(), S, p["eta"])
            t_enc = int(p["strength"] * S)
            torch.manual_seed(p["noise_seed"])
            if mode == "sd":
                torch.randn(z0.shape)
            n0 = torch.randn(z0.shape)
            noises = [torch.randn(z0.shape) for _ in range(t_enc)]
            zt = br.latent_sdedit_start(z0, sch, t_enc, n0)
            assert _rel(zt, fx[mode + "_sdedit_zt"]) < 1e-6
            x = br.latent_decode(br.cfg_eps(unet, c_tgt, uc, p["dec_scale"]), zt, sch, t_enc, noises)
            assert _rel(x, fx[mode + "_sdedit_x"]) < 1e-5
        assert float(fx["sd_rt_err_max"]) > 0  # the fixture's round-trip yardstick exists


def test_pixel_restatement_reproduces_the_fixture():
    fx = gu.load("baselines_pixel")
    p = json.loads(str(fx["params"]))
    src_sd = br.synth_weights(json.loads(str(fx["src_names"])), p["src_seed"], p["out_prefix"], p["out_scale"])
    tgt_sd = br.synth_weights(json.loads(str(fx["tgt_names"])), p["tgt_seed"], p["out_prefix"], p["out_scale"])
    f = lambda sd: (lambda x, t: nets.ho_unet(sd, gu.TOY_HO_CFG, x, torch.full((x.shape[0],), int(t), dtype=torch.long)))
    img = torch.rand((1, 3, 32, 32), generator=torch.Generator().manual_seed(p["image_seed"]))
    x0 = (img - 0.5) * 2.0
    with torch.no_grad():
        sch0 = schedule.PixelSchedule(p["custom_steps"], p["es_steps"], sample_type="ddim", eta=0.0)
        xT, x = br.pixel_ddib(f(src_sd), f(tgt_sd), x0, sch0)
        assert _rel(xT, fx["ddib_xT"]) < 1e-5 and _rel(x, fx["ddib_x"]) < 1e-5
        sch = schedule.PixelSchedule(p["custom_steps"], p["es_steps"], sample_type="ddim", eta=p["eta"])
        i_s = int(fx["i_s"])
        torch.manual_seed(p["noise_seed"])
        n0 = torch.randn(x0.shape)
        noises = [torch.randn(x0.shape) for _ in range(i_s + 1)]
        xt, x = br.pixel_sdedit(f(tgt_sd), x0, sch, i_s, n0, noises)
        assert _rel(xt, fx["sdedit_xt"]) < 1e-6 and _rel(x, fx["sdedit_x"]) < 1e-5


@pytest.mark.skipif(not ref_import.available(), reason="reference tree not mounted")
def test_restatement_against_the_live_reference():
    """step by step: the latent inversion step against denoising_step(eta=0, 'ddim') on the SD betas (its alpha-bar is a fp32
    cumprod, the sampler's a fp64 one: agreement to fp32 resolution), the restated decode against DDIMSampler.decode, the
    pixel steps against denoising_step itself"""
    try:
        _live_checks()
    finally:
        # WORKAROUND for oracle/ref_import.teardown() (oracle/ stays as it is): teardown drops the reference's modules by file,
        # but namespace packages without a file (e.g. `model.lib.ddpm_ddim`) survive it, and a stale one breaks the next test
        # module's imports from the reference tree (KeyError: 'model.lib')
        for name in list(sys.modules):
            m = sys.modules.get(name)
            if m is None or getattr(m, "__file__", None) is not None or not hasattr(m, "__path__"):
                continue
            try:
                stale = any(str(q).startswith(ref_import.REF) for q in list(m.__path__))
            except KeyError:  # a namespace path whose parent package is already gone
                stale = True
            if stale:
                del sys.modules[name]


def _live_checks():
    fx, p, unet, c_src, c_tgt, uc = _latent_setting()
    S = p["S"]
    with ref_import.session(), torch.no_grad(), ref_import.quiet():
        from model.lib.ddpm_ddim.utils.diffusion_utils import denoising_step
        from ldm.modules.diffusionmodules.util import make_beta_schedule
        betas = torch.from_numpy(make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.0120)).float()
        sch0 = schedule.DDIMSchedule(schedule.latent_alphas_cumprod(), S, 0.0)
        eps = br.cfg_eps(unet, c_src, uc, p["enc_scale"])
        z0 = torch.as_tensor(fx["sd_z0"])
        _xT, traj = br.latent_ddib_invert(eps, z0, sch0)
        x = z0
        for j in range(S):
            t = 0 if j == 0 else int(sch0.timesteps[j - 1])
            model = lambda xx, tt: eps(xx, int(tt[0]))
            y = denoising_step(x, torch.full((2,), float(t)), torch.full((2,), float(sch0.timesteps[j])), models=model,
                               logvars=np.zeros(1000), b=betas, sampling_type="ddim", eta=0.0)
            assert _rel(traj[j], y) < 1e-5, j
            x = traj[j]
        # the restated decode against DDIMSampler.decode (eta 0.1, CFG 3)
        Sampler = ref_import.ddim_sampler_cls()
        smp = Sampler(types.SimpleNamespace(**vars(ref_import.LatentShim(None))))
        smp.model.apply_model = lambda xx, tt, cc: unet(xx, tt, cc)
        smp.make_schedule(S, ddim_eta=0.1, verbose=False)
        sch = schedule.DDIMSchedule(schedule.latent_alphas_cumprod(), S, 0.1)
        zt = torch.as_tensor(fx["sd_sdedit_zt"])
        torch.manual_seed(5)
        want = smp.decode(zt, c_tgt, 7, unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
        torch.manual_seed(5)
        noises = [torch.randn(zt.shape) for _ in range(7)]
        got = br.latent_decode(br.cfg_eps(unet, c_tgt, uc, 3.0), zt, sch, 7, noises)
        assert torch.equal(got, want) or _rel(got, want) < 1e-6
        # pixel: one inversion step and one eta 0.1 step against denoising_step
        pf = gu.load("baselines_pixel")
        pp = json.loads(str(pf["params"]))
        sd = br.synth_weights(json.loads(str(pf["src_names"])), pp["src_seed"], pp["out_prefix"], pp["out_scale"])
        f = lambda xx, tt: nets.ho_unet(sd, gu.TOY_HO_CFG, xx, torch.full((xx.shape[0],), int(tt), dtype=torch.long))
        fm = lambda xx, tt: f(xx, int(tt[0]))
        ps = schedule.PixelSchedule(40, 40, sample_type="ddim", eta=0.1)
        b = torch.from_numpy(ps.b)
        xp = gu.rnd((1, 3, 32, 32), 3)
        y = denoising_step(xp, torch.ones(1) * 100, torch.ones(1) * 125, models=fm, logvars=ps.logvar.astype(np.float64),
                           b=b, sampling_type="ddim", eta=0.0)
        assert torch.equal(br._ddim_step(f, xp, 100, 125, b), y)
        n = gu.rnd((1, 3, 32, 32), 4)
        torch.manual_seed(6)
        y = denoising_step(xp, torch.ones(1) * 125, torch.ones(1) * 100, models=fm, logvars=ps.logvar.astype(np.float64),
                           b=b, sampling_type="ddim", eta=0.1)
        torch.manual_seed(6)
        n = torch.randn(xp.shape)
        assert _rel(br._ddim_step(f, xp, 125, 100, b, 0.1, n), y) < 1e-6


def test_factory_knows_the_six_baselines(monkeypatch):
    from cycle_diffusion_amd.gan_wrapper import baselines, get_gan_wrapper as g
    assert sorted(baselines.GAN_TYPES) == sorted(NAMES)
    classes = set(baselines.GAN_TYPES.values())
    for name in NAMES:
        seen = {}
        monkeypatch.setitem(baselines.GAN_TYPES, name, lambda **kw: seen.update(kw) or "made")
        pairs = [("gan_type", name), ("custom_steps", 9), ("source_model_type", "a"), ("target_model_type", "b")]

        class Args(types.SimpleNamespace):
            def __iter__(self):
                return iter(pairs)
        assert g.get_gan_wrapper(Args(gan_type=name), target=True) == "made"
        assert seen == {"custom_steps": 9, "source_model_type": "b"}
    with pytest.raises(ValueError):
        g.get_gan_wrapper(Args(gan_type="NoSuchBaseline"))
    # no coupled loop: Model.forward takes encode() + forward()
    for cls in classes:
        assert isinstance(inspect.getattr_static(cls, "translate"), property)
        assert not hasattr(object.__new__(cls), "translate")


def test_keys_without_meaning_are_refused():
    from cycle_diffusion_amd.gan_wrapper import baselines
    baselines._reject("SDEdit", skip_steps=None, white_box_steps=None)
    with pytest.raises(ValueError, match="skip_steps, white_box_steps"):
        baselines._reject("SDEdit", skip_steps=[0], white_box_steps=100, encoder_unconditional_guidance_scales=None)
    baselines.DDPMDDIBWrapper._check_eta("ddim", 0.0)
    for st, eta in (("ddim", 0.1), ("ddpm", 0.0), ("ddpm", None)):
        with pytest.raises(ValueError):
            baselines.DDPMDDIBWrapper._check_eta(st, eta)


def test_configs_parse():
    from cycle_diffusion_amd.utils.config_utils import get_config
    for base in ("bench_sd_c2", "bench_ldm_c3", "bench_afhq_c5"):
        for m, gt in (("ddib", ("SDDDIBText", "LatentDiffDDIBText", "DDPM_DDIB")),
                      ("sdedit", ("SDSDEditText", "LatentDiffSDEditText", "DDPM_SDEdit"))):
            path = os.path.join(ROOT, "config", "experiments", "%s_%s.cfg" % (base, m))
            assert os.path.exists(path), path
            args = get_config(path)
            assert args.gan.gan_type in gt
            keys = dict(list(args.gan))
            if m == "sdedit":
                assert isinstance(keys["sdedit_strengths"], list)
            elif base != "bench_afhq_c5":  # the pixel wrappers default to fp32 already
                assert keys["precision"] == "fp32"
