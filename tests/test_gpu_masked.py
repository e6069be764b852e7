"""The region-keeping decode (include/cyclediff.h cd_ddim_decode_masked / cd_keep_mask / cd_op_sched_step_masked;
wrapper forward(mask=) / translate(mask=)): DDIMSampler.sample_with_eps(mask=, x0=) (ddim.py:427-430) on the engine, and the
"encoder" mode of the coupled loop. Bit-exact wherever two paths do the same fp32 arithmetic; the reference fixture
(tests/golden/masked_latent.npz, scripts/gen_golden_masked.py) within the bounds tests/test_gpu_baselines.py holds the SDEdit
decode of the same networks to."""
import ctypes as C
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

import _masked_ref as mr
import golden_util as gu
from cycle_diffusion_amd import _ffi, schedule
from cycle_diffusion_amd._ffi import check, ptr
from test_gpu_models import _load, tiny_sd_desc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = 1.0 if _ffi.load_library().cd_act_format() == 1 else 8.0
DDIM = _ffi.CD_SCHED_DDIM
H16 = torch.float16 if FMT == 1.0 else torch.bfloat16


def _masks(B=2, h=16):
    """latent masks: sample 0 a hard rectangle, sample 1 soft values strictly inside (0, 1)"""
    m = torch.zeros(B, 1, h, h)
    m[0, 0, 4:12, 2:9] = 1.0
    m[1:] = torch.rand((B - 1, 1, h, h), generator=torch.Generator().manual_seed(3)) * 0.9 + 0.05
    return m


def _setup(engine, S=12, skip=0, prec=None):
    fx = gu.load("latent_cycle_tiny")
    d = tiny_sd_desc()
    if prec is not None:
        d.precision = prec
    net, _sd = _load(engine, d, fx)
    x0, c, uc, c2 = (t.cuda() for t in gu.latent_cycle_inputs())
    K = S - skip
    sch = schedule.DDIMSchedule(schedule.latent_alphas_cumprod(), S, 0.1)
    noise = torch.stack(gu.latent_noise(77, x0.shape, K), 0).cuda()
    return net, x0, c, uc, c2, sch, K, noise


def _mask_noise(seed, K, B):
    torch.manual_seed(seed)
    return torch.stack([torch.randn(B, 4, 16, 16) for _ in range(K)], 0).cuda()


# ------------------------------------------------------------------------------------------------ 1. step kernel
def _step_masked(engine, mode, row, x, eh, cfg, g, eps, mask, src, source, qa, qb, nz, blend, cfg_dup):
    B, Cc, H, W = x.shape
    coef = _ffi.coef_array([row])
    xd = x.cuda().contiguous()
    dev = lambda t: None if t is None else t.cuda().contiguous()
    ehd, epd, md, sd, nd = dev(eh), dev(eps), dev(mask), dev(src), dev(nz)
    xin = torch.zeros(((2 if cfg_dup else 1) * B, H * W, Cc), device="cuda", dtype=torch.int16)
    check(engine.lib.cd_op_sched_step_masked(engine.h, mode, C.c_void_p(coef.ctypes.data), ptr(xd), ptr(ehd), int(cfg),
                                             C.c_float(g), ptr(epd), ptr(md), ptr(sd), mask.shape[0], source, C.c_float(qa),
                                             C.c_float(qb), ptr(nd), int(blend), B, Cc, H * W, ptr(xin), int(cfg_dup)))
    torch.cuda.synchronize()
    return xd.cpu(), xin.cpu()


@pytest.mark.parametrize("cfg", [False, True], ids=["nocfg", "cfg"])
@pytest.mark.parametrize("source", ["q_sample", "encoder"])
def test_masked_step_kernel_bit_exact(engine, cfg, source):
    """k_decode_step_ddim<true> / k_mask_blend_init against the torch fp32 restatement of the blended step: hard and soft mask
    rows, x and the 16-bit NHWC input of the next forward (with its classifier-free-guidance duplicate)"""
    from test_gpu_ops import _coef
    g = torch.Generator().manual_seed(41)
    B, Cc, H, W = 2, 4, 16, 16
    x0, xt, e_u, e_c, nz, eps = [torch.randn(B, Cc, H, W, generator=g) for _ in range(6)]
    mask = _masks(B, H)
    a_t, a_prev, sig = 0.4321, 0.4876, 0.0123
    row = _coef(a_t, a_prev, sig)
    rowd = _ffi.coef_array([row])[0]
    qa, qb = float(np.float32(0.69831)), float(np.float32(0.71579))
    gs = 3.0
    e_t = e_u + gs * (e_c - e_u) if cfg else e_c
    eh = torch.cat([e_u, e_c], 0) if cfg else e_c
    src_id = _ffi.MASK_SOURCES[source]
    src = mr._full(qa, B) * x0 + mr._full(qb, B) * nz if source == "q_sample" else x0
    mnz = nz if source == "q_sample" else None

    def nhwc16(v):
        t = v.permute(0, 2, 3, 1).reshape(B, H * W, Cc).contiguous().to(H16).view(torch.int16)
        return torch.cat([t, t], 0) if cfg else t

    x_prev = mr.decode_step(xt, e_t, rowd, eps)
    want = mr.blend(src, mask, x_prev)
    got, xin = _step_masked(engine, 2, row, xt, eh, cfg, gs, eps, mask, x0, src_id, qa, qb, mnz, 1, cfg)
    assert torch.equal(got, want), (got - want).abs().max().item()
    assert torch.equal(xin, nhwc16(want))
    # the last step: nothing is blended after it
    got, xin = _step_masked(engine, 2, row, xt, eh, cfg, gs, eps, mask, x0, src_id, qa, qb, mnz, 0, cfg)
    assert torch.equal(got, x_prev) and torch.equal(xin, nhwc16(x_prev))
    # the blend ahead of the first forward
    want0 = mr.blend(src, mask, xt)
    got, xin = _step_masked(engine, 0, row, xt, None, False, 1.0, None, mask, x0, src_id, qa, qb, mnz, 1, cfg)
    assert torch.equal(got, want0) and torch.equal(xin, nhwc16(want0))
    # and the blend really moved the kept region
    assert (want - x_prev).abs().max() > 0.1


# ------------------------------------------------------------------------------------------------ 2. no-op identities
@pytest.mark.parametrize("prec", [None, _ffi.CD_PREC_F32], ids=["16bit", "fp32"])
def test_zero_mask_is_the_unmasked_path_bit_for_bit(engine, prec):
    net, x0, c, uc, c2, sch, K, noise = _setup(engine, prec=prec)
    B = x0.shape[0]
    m0 = torch.zeros(B, 1, 16, 16).cuda()
    ce, cd, q = sch.coef_encode(0), sch.coef_decode(0), sch.coef_qsample(0)
    z = engine.dpm_encode(net, DDIM, x0, ce, ctx_c=c, ctx_uc=uc, guidance=1.0, noise=noise)
    mn = _mask_noise(5, K, B)
    for guidance in (3.0, [1.5, 4.0]):
        x_ref = engine.ddim_decode(net, DDIM, z, cd, ctx_c=c2, ctx_uc=uc, guidance=guidance)
        x = engine.ddim_decode_masked(net, DDIM, z, cd, m0, x0, q, mask_noise=mn, ctx_c=c2, ctx_uc=uc, guidance=guidance)
        engine.synchronize()
        assert torch.equal(x, x_ref), (x - x_ref).abs().max().item()
    zc, xc = engine.cycle_translate(net, DDIM, x0, ce, cd, enc_ctx_c=c, enc_ctx_uc=uc, dec_ctx_c=c2, dec_ctx_uc=uc,
                                    dec_guidance=3.0, noise=noise)
    for source in ("q_sample", "encoder"):
        kw = dict(mask_x0=x0, qcoef=q, mask_noise=mn) if source == "q_sample" else {}
        zm, xm = engine.cycle_translate_masked(net, DDIM, x0, ce, cd, m0, mask_source=source, enc_ctx_c=c, enc_ctx_uc=uc,
                                               dec_ctx_c=c2, dec_ctx_uc=uc, dec_guidance=3.0, noise=noise, **kw)
        engine.synchronize()
        assert torch.equal(zm, zc) and torch.equal(xm, xc), (source, (xm - xc).abs().max().item())


# ------------------------------------------------------------------------------------------------ 3. full keep
def test_full_keep_is_one_step_from_the_last_q_sample(engine):
    """m = 1: ahead of the last forward x is q_sample(x0, tau[0]) on the last draw, whatever came before"""
    net, x0, c, uc, c2, sch, K, noise = _setup(engine)
    B = x0.shape[0]
    cd, q = sch.coef_decode(0), sch.coef_qsample(0)
    z = engine.dpm_encode(net, DDIM, x0, sch.coef_encode(0), ctx_c=c, ctx_uc=uc, guidance=1.0, noise=noise)
    mn = _mask_noise(6, K, B)
    x = engine.ddim_decode_masked(net, DDIM, z, cd, torch.ones(B, 1, 16, 16).cuda(), x0, q, mask_noise=mn, ctx_c=c2,
                                  ctx_uc=uc, guidance=3.0)
    src0 = (mr._full(q[0, 0], B) * x0.cpu() + mr._full(q[0, 1], B) * mn[K - 1].cpu()).cuda()
    z1 = torch.stack([src0, z[:, K]], 1).contiguous()
    x_ref = engine.ddim_decode(net, DDIM, z1, cd[:1].copy(), ctx_c=c2, ctx_uc=uc, guidance=3.0)
    engine.synchronize()
    assert torch.equal(x, x_ref), (x - x_ref).abs().max().item()


# ------------------------------------------------------------------------------------------------ 5. coupled = two calls
@pytest.mark.parametrize("case", ["cfg3", "two_scales", "cond_only", "skip4_cfg3", "fp32_cfg3"])
def test_masked_coupled_loop_equals_the_two_calls_bit_for_bit(engine, case):
    prec = _ffi.CD_PREC_F32 if case.startswith("fp32") else None
    skip = 4 if case.startswith("skip4") else 0
    net, x0, c, uc, c2, sch, K, noise = _setup(engine, S=16, skip=skip, prec=prec)
    B = x0.shape[0]
    n_dec, dec_g = 1, 3.0
    if case == "two_scales":
        n_dec, dec_g = 2, [1.5] * B + [4.0] * B
    elif case == "cond_only":
        dec_g = 1.0
    mask = _masks(B).cuda()
    ce, cd, q = sch.coef_encode(skip), sch.coef_decode(skip), sch.coef_qsample(skip)
    mn = _mask_noise(7, K, n_dec * B)
    c_tgt, ucd = c2.repeat(n_dec, 1, 1), uc.repeat(n_dec, 1, 1)
    z_ref = engine.dpm_encode(net, DDIM, x0, ce, ctx_c=c, ctx_uc=uc, guidance=1.0, noise=noise)
    x_ref = engine.ddim_decode_masked(net, DDIM, z_ref.repeat(n_dec, 1, 1, 1, 1), cd, mask, x0, q, mask_noise=mn, ctx_c=c_tgt,
                                      ctx_uc=ucd, guidance=dec_g)  # the mask is shared through b % B
    z, x = engine.cycle_translate_masked(net, DDIM, x0, ce, cd, mask, mask_x0=x0, qcoef=q, mask_noise=mn, enc_ctx_c=c,
                                         enc_ctx_uc=uc, dec_ctx_c=c_tgt, dec_ctx_uc=ucd, dec_guidance=dec_g, n_dec=n_dec,
                                         noise=noise)
    engine.synchronize()
    assert torch.isfinite(x).all()
    assert torch.equal(z, z_ref) and torch.equal(x, x_ref), (x - x_ref).abs().max().item()
    x_plain = engine.ddim_decode(net, DDIM, z_ref.repeat(n_dec, 1, 1, 1, 1), cd, ctx_c=c_tgt, ctx_uc=ucd, guidance=dec_g)
    assert (x - x_plain).abs().max() > 1e-3  # the mask does something


# ------------------------------------------------------------------------------------------------ 6. encoder mode
def test_encoder_mode_full_keep_follows_the_encoder_trajectory(engine):
    """m = 1, "encoder": the decoder's input of every level is the encoder's x_t, which needs no network to recompute
    (ddim.py:582-601) - so the output is one unmasked decode step from the recomputed level-0 x_t under the target context"""
    net, x0, c, uc, c2, sch, K, noise = _setup(engine)
    B = x0.shape[0]
    ce, cd = sch.coef_encode(0), sch.coef_decode(0)
    z, x = engine.cycle_translate_masked(net, DDIM, x0, ce, cd, torch.ones(B, 1, 16, 16).cuda(), mask_source="encoder",
                                         enc_ctx_c=c, enc_ctx_uc=uc, dec_ctx_c=c2, dec_ctx_uc=uc, dec_guidance=3.0, noise=noise)
    traj = mr.encoder_trajectory(x0.cpu(), ce, noise.cpu())
    assert torch.equal(z[:, 0].cpu(), traj[K - 1])
    z1 = torch.stack([traj[0].cuda(), z[:, K]], 1).contiguous()
    x_ref = engine.ddim_decode(net, DDIM, z1, cd[:1].copy(), ctx_c=c2, ctx_uc=uc, guidance=3.0)
    engine.synchronize()
    assert torch.equal(x, x_ref), (x - x_ref).abs().max().item()


def test_encoder_mode_same_text_stays_on_the_cycle(engine, report):
    """hard rectangle, encode text == decode text at scale 1: the decoder retraces the encoder's trajectory up to round-off,
    so keeping a region ON that trajectory changes nothing beyond the bound tests/test_gpu_models.py::test_latent_cycle_tiny
    holds the unmasked same-text cycle to (8e-3 max-abs, x the format factor)"""
    net, x0, c, uc, c2, sch, K, noise = _setup(engine, S=99)
    B = x0.shape[0]
    mask = torch.zeros(B, 1, 16, 16)
    mask[:, 0, 4:12, 2:9] = 1.0
    ce, cd = sch.coef_encode(0), sch.coef_decode(0)
    kw = dict(enc_ctx_c=c, enc_ctx_uc=uc, dec_ctx_c=c, dec_ctx_uc=uc, dec_guidance=1.0, noise=noise)
    _z0, x_plain = engine.cycle_translate(net, DDIM, x0, ce, cd, **kw)
    _z1, x = engine.cycle_translate_masked(net, DDIM, x0, ce, cd, mask.cuda(), mask_source="encoder", **kw)
    engine.synchronize()
    err = (x - x_plain).abs().max().item()
    report.add("masked/encoder_same_text_vs_unmasked_cycle", maxabs=err, cycle=(x_plain - x0).abs().max().item())
    assert err < 8e-3 * FMT, err


def test_encoder_mode_is_refused_on_the_two_call_path(engine):
    net, x0, c, uc, c2, sch, K, noise = _setup(engine, S=4)
    z = engine.dpm_encode(net, DDIM, x0, sch.coef_encode(0), ctx_c=c, ctx_uc=uc, guidance=1.0, noise=noise)
    with pytest.raises(ValueError, match="coupled loop"):
        engine.ddim_decode_masked(net, DDIM, z, sch.coef_decode(0), torch.ones(2, 1, 16, 16).cuda(), x0, None,
                                  mask_source="encoder")
    w, _emb, _u, _v = _tiny_wrapper(mask_source="encoder", n_trials=1, skip_steps=[0])
    image = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        zz = w.encode(image, ["a", "b"])
        with pytest.raises(ValueError, match="translate"):
            w(zz, image, ["a", "b"], ["c", "d"], mask=torch.ones(2, 1, 64, 64))
        assert torch.isfinite(w(zz, image, ["a", "b"], ["c", "d"])).all()


# ------------------------------------------------------------------------------------------------ 7. ensemble order
def _tiny_wrapper(**kw):
    from test_gpu_wrappers import _make
    return _make(True, **kw)


@pytest.mark.parametrize("path", ["forward", "translate"])
def test_folded_masked_ensemble_reproduces_each_member_alone(path):
    """2 skips x 2 decoder scales with a mask, folded into the batch, against every member run alone on the draws it would
    make alone: the reference's generate() calls sample_with_eps member by member (sd_wrapper:142-167), K draws each"""
    src, tgt = ["a photo", "a cat"], ["a drawing", "a dog"]
    image = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(5)).cuda()
    mask = mr.fixture_masks(2, 64)
    common = dict(n_trials=1, precision="fp32", ranker=lambda img, orig, s, t: img.flatten(1).mean(1))
    w, _emb, _u, _v = _tiny_wrapper(skip_steps=[0, 4], decoder_unconditional_guidance_scales=[2.0, 3.0], **common)
    K = {0: len(w._schedule()), 4: len(w._schedule()) - 4}
    shape = (2, 4, 16, 16)
    with torch.no_grad():
        torch.manual_seed(11)
        if path == "forward":
            w(w.encode(image, src), image, src, tgt, mask=mask)
        else:
            w.translate(image, src, tgt, mask=mask)
            assert w.last_translate_coupled
        folded = [t.clone() for t in w.last_latents]
        # the draws in the reference's order: posterior, member noises (skip 0, skip 4), then per candidate K mask draws
        torch.manual_seed(11)
        post = torch.randn(shape)
        enc = {sk: torch.stack([torch.randn(shape) for _ in range(K[sk])], 0) for sk in (0, 4)}
        mdraw = {(sk, sc): torch.stack([torch.randn(shape) for _ in range(K[sk])], 0) for sk in (0, 4) for sc in (2.0, 3.0)}
        slot = 0
        for sk in (0, 4):
            for sc in (2.0, 3.0):
                w1, _e, _u1, _v1 = _tiny_wrapper(skip_steps=[sk], decoder_unconditional_guidance_scales=[sc], **common)
                feed = [post] + list(enc[sk]) + list(mdraw[(sk, sc)])
                w1.noise_source = lambda shp, feed=feed: feed.pop(0).reshape(shp)
                if path == "forward":
                    w1(w1.encode(image, src), image, src, tgt, mask=mask)
                else:
                    w1.translate(image, src, tgt, mask=mask)
                assert not feed
                assert torch.equal(w1.last_latents[0], folded[slot]), (sk, sc, (w1.last_latents[0] - folded[slot]).abs().max().item())
                slot += 1


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_masked_entry_points_refuse_what_they_cannot_do(engine):
    import cycle_diffusion_amd as cda
    net, x0, c, uc, c2, sch, K, noise = _setup(engine, S=4)
    B = x0.shape[0]
    ce, cd, q = sch.coef_encode(0), sch.coef_decode(0), sch.coef_qsample(0)
    z = engine.dpm_encode(net, DDIM, x0, ce, ctx_c=c, ctx_uc=uc, guidance=1.0, noise=noise)
    mask = _masks(B).cuda()
    mn = _mask_noise(8, K, B)
    lib, h = engine.lib, engine.h
    x = torch.empty_like(x0)
    zo = torch.empty_like(z)
    qp = C.c_void_p(q.ctypes.data)

    def decode(kind, net_id, zz, b_mask, source=_ffi.CD_MASK_QSAMPLE):
        return lib.cd_ddim_decode_masked(h, net_id, kind, ptr(zz), zz.shape[1], zz.shape[1] - 1, ptr(c2), ptr(uc), 77,
                                         C.c_float(3.0), None, B, K, C.c_void_p(cd.ctypes.data), None, C.c_uint64(0), ptr(mask),
                                         ptr(x0), b_mask, source, qp, ptr(mn), C.c_uint64(0), ptr(x))

    def coupled(source, qtab, nzp):
        keep = _ffi.KeepMask(mask=ptr(mask), x0=ptr(x0), B_mask=B, source=source, qsample_coef_host=qtab, noise=nzp, seed=0)
        a = _ffi.TranslateArgs(
            size=C.sizeof(_ffi.TranslateArgs), net=net, sched_kind=DDIM, x0=ptr(x0), enc_ctx_c=ptr(c), enc_ctx_uc=ptr(uc),
            enc_guidance=1.0, dec_ctx_c=ptr(c2), dec_ctx_uc=ptr(uc), dec_guidance=3.0, ctx_len=77, B=B, n_dec=1, K=K,
            coef_enc_host=ce.ctypes.data, coef_dec_host=cd.ctypes.data, noise=ptr(noise), seed=0, last_uses_x0=1, z_out=ptr(zo),
            x_out=ptr(x), mask=C.pointer(keep))
        return lib.cd_cycle_translate(h, C.byref(a))

    err = lambda: lib.cd_last_error().decode()
    assert decode(_ffi.CD_SCHED_DDPM, net, z, B) != 0 and "CD_SCHED_DDIM" in err()
    ho = engine.create_net(cda.ho_ddpm_desc(32, 32, (1, 2, 2), 1, (16,)))  # a pixel network
    assert decode(DDIM, ho, z, B) != 0 and "pixel" in err()
    mask3 = torch.cat([mask, mask[:1]], 0).contiguous()
    assert decode(DDIM, net, z, 3) != 0 and "mask shape mismatch" in err()
    with pytest.raises(ValueError, match="mask must be"):
        engine.ddim_decode_masked(net, DDIM, z, cd, mask3, x0, q, mask_noise=mn, ctx_c=c2, ctx_uc=uc, guidance=3.0)
    with pytest.raises(ValueError, match="mask must be"):
        engine.ddim_decode_masked(net, DDIM, z, cd, mask[:, :, :8].contiguous(), x0, q, ctx_c=c2, ctx_uc=uc, guidance=3.0)
    assert decode(DDIM, net, z, B, _ffi.CD_MASK_ENCODER) != 0 and "coupled loop" in err()
    assert coupled(_ffi.CD_MASK_ENCODER, qp, None) != 0 and "NULL" in err()
    assert coupled(_ffi.CD_MASK_ENCODER, None, ptr(mn)) != 0 and "NULL" in err()
    assert coupled(_ffi.CD_MASK_QSAMPLE, None, ptr(mn)) != 0 and "q-sample" in err()
    # the engine is usable after the refusals
    x_ok = engine.ddim_decode(net, DDIM, z, cd, ctx_c=c2, ctx_uc=uc, guidance=3.0)
    assert coupled(_ffi.CD_MASK_ENCODER, None, None) == 0 and decode(DDIM, net, z, B) == 0
    engine.synchronize()
    assert torch.isfinite(x_ok).all() and torch.isfinite(x).all()
    # the wrappers without a mask hook reject one by name
    from cycle_diffusion_amd.gan_wrapper import baselines
    from cycle_diffusion_amd.gan_wrapper.ddpm_ddim_wrapper import DDPMDDIMWrapper
    with pytest.raises(ValueError, match="keep-mask"):
        DDPMDDIMWrapper.forward(object.__new__(DDPMDDIMWrapper), None, mask=mask)
    with pytest.raises(ValueError, match="keep-mask"):
        baselines._LatentBaseline.forward(object.__new__(baselines.SDSDEditTextWrapper), None, None, None, None, mask=mask)


# ------------------------------------------------------------------------------------------------ 4. reference fixture
@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("mode", ["sd", "ldm"])
def test_wrapper_forward_with_mask_vs_reference_fixture(monkeypatch, report, mode, prec):
    """encode() + forward(mask=) in "q_sample" mode against the reference's own ddpm_ddim_encoding + sample_with_eps(mask=,
    x0=) (tests/golden/masked_latent.npz), held to the bounds of the SDEdit decode on these networks
    (tests/test_gpu_baselines.py LAT_REL / PSNR_FLOOR: same nets, same chain length, same kind of path)."""
    from test_gpu_baselines import LAT_REL, PSNR_FLOOR, SRC, TGT, TableEmbedder, _rel, _tiny
    import _baselines_ref as br
    from cycle_diffusion_amd.gan_wrapper import latent_text_wrapper as ltw
    from oracle import nets
    monkeypatch.setenv("CYCLEDIFF_SYNTHETIC_WEIGHTS", "1")
    fx = mr.load_fixture()
    p = mr.params(fx)
    cls = ltw.SDStochasticTextWrapper if mode == "sd" else ltw.LatentDiffStochasticTextWrapper
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w = _tiny(cls)(source_model_type="none", custom_steps=p["S"], eta=p["eta"], white_box_steps=p["S"] + 1, skip_steps=[0],
                       encoder_unconditional_guidance_scales=[p["enc_scale"]],
                       decoder_unconditional_guidance_scales=[p["dec_scale"]], n_trials=1, cond_stage=TableEmbedder(p),
                       noise_on_cpu=True, precision=prec)
    usd = br.synth_weights(json.loads(str(fx["unet_names"])), p["unet_seed"], p["out_prefix"], p["out_scale"])
    vsd = nets.synth_state_dict(json.loads(str(fx["vae_names"])), p["vae_seed"])
    assert w.engine.load_state_dict(w.unet, usd)[0] == 0 and w.engine.load_state_dict(w.vae, vsd)[0] == 0
    image = torch.rand((p["B"], 3, 64, 64), generator=torch.Generator().manual_seed(p["image_seed"])).cuda()
    mask = torch.as_tensor(fx["mask_pixel"])
    torch.manual_seed(p["noise_seed"])
    with torch.no_grad():
        z = w.encode(image, SRC)
        torch.manual_seed(p["mask_noise_seed"])  # K draws of randn(B, 4, 16, 16) in loop order
        img = w(z, image, SRC, TGT, mask=mask)
    K = p["S"]
    rz = _rel(z[0].view(2, K + 1, 4, 16, 16)[:, 0], fx[mode + "_z_sub"][:, 0])
    rx = _rel(w.last_latents[0], fx[mode + "_x"])
    ps = gu.psnr(img, torch.as_tensor(fx[mode + "_img"]))
    report.add("masked/forward_%s_%s" % (mode, prec), xT_rel=rz, x_rel=rx, psnr_db=ps)
    print("masked/forward_%s_%s xT_rel=%.3e x_rel=%.3e psnr=%.2f" % (mode, prec, rz, rx, ps))
    assert rz < LAT_REL[prec] and rx < LAT_REL[prec] and ps > PSNR_FLOOR[prec], (rz, rx, ps)


# ------------------------------------------------------------------------------------------------ 9. inner seam
def test_sampler_written_against_latent_diffusion_runs_the_masked_decode(engine, report):
    """sample_with_eps(mask=, x0=) over LatentDiffusionHIP (its q_sample and buffers) against cd_ddim_decode_masked on the same
    draws, within the bound tests/test_gpu_compat.py holds the unmasked pair to (5e-3 x format factor, relative max):
    the reference's unmodified sampler where the staged reference exists, else the restatement of tests/_masked_ref.py"""
    from cycle_diffusion_amd.compat import LatentDiffusionHIP
    from oracle import ref_import
    S, skip = 99, 91
    net, x0, c, uc, c2, sch, K, noise = _setup(engine, S=S, skip=skip)
    B = x0.shape[0]
    model = LatentDiffusionHIP(engine, net)
    sa, s1a = mr.qsample_buffers()
    assert torch.equal(model.sqrt_alphas_cumprod.cpu(), sa) and torch.equal(model.sqrt_one_minus_alphas_cumprod.cpu(), s1a)
    mask = _masks(B).cuda()
    cd, q = sch.coef_decode(skip), sch.coef_qsample(skip)
    z = engine.dpm_encode(net, DDIM, x0, sch.coef_encode(skip), ctx_c=c, ctx_uc=uc, guidance=1.0, noise=noise)
    torch.cuda.manual_seed(99)
    mn = torch.stack([torch.randn(tuple(x0.shape), device="cuda") for _ in range(K)], 0)
    x = engine.ddim_decode_masked(net, DDIM, z, cd, mask, x0, q, mask_noise=mn, ctx_c=c2, ctx_uc=uc, guidance=3.0)
    t0 = torch.full((B,), int(cd["t"][K - 1]), dtype=torch.long, device="cuda")
    want = mr._full(q[K - 1, 0], B).cuda() * x0 + mr._full(q[K - 1, 1], B).cuda() * mn[0]
    assert torch.equal(model.q_sample(x0, t0, noise=mn[0]), want)
    if ref_import.available():
        with ref_import.session():
            from ldm.models.diffusion.ddim import DDIMSampler  # the reference's class, as it is
            torch.cuda.manual_seed(99)  # q_sample draws randn_like(x0) at the top of every step
            with ref_import.quiet(), torch.no_grad():
                x_ref, _ = DDIMSampler(model).sample_with_eps(S, z[:, 1:], conditioning=c2, batch_size=B, shape=(4, 16, 16),
                                                              eta=0.1, verbose=False, x_T=z[:, 0], skip_steps=skip,
                                                              unconditional_guidance_scale=3.0, unconditional_conditioning=uc,
                                                              mask=mask, x0=x0)
    else:
        def eps_fn(xx, t):
            tt = torch.full((2 * B,), t, dtype=torch.long, device="cuda")
            e_u, e_c = model.apply_model(torch.cat([xx.cuda()] * 2), tt, torch.cat([uc, c2])).cpu().chunk(2)
            return e_u + 3.0 * (e_c - e_u)
        with torch.no_grad():
            x_ref = mr.masked_decode(eps_fn, z.cpu(), cd, q, mask.cpu(), x0.cpu(), mn.cpu()).cuda()
    engine.synchronize()
    rel = ((x - x_ref).abs().max() / x_ref.abs().max()).item()
    report.add("masked/sampler_over_hip_unet", latent_rel=rel, reference_sampler=bool(ref_import.available()))
    assert rel < 5e-3 * FMT, rel


# ------------------------------------------------------------------------------------------------ 10. driver
def test_main_writes_keep_and_edit_psnr_for_masked_samples_only(tmp_path, monkeypatch):
    from PIL import Image
    monkeypatch.setenv("CYCLEDIFF_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.delenv("CYCLEDIFF_CLIP_RANKER", raising=False)
    rng = np.random.RandomState(7)
    Image.fromarray(rng.randint(0, 255, (64, 64, 3), dtype=np.uint8)).resize((512, 512), Image.BICUBIC).save(tmp_path / "im.png")
    m = np.zeros((512, 512), dtype=np.uint8)
    m[128:384, 64:256] = 255
    Image.fromarray(m).save(tmp_path / "mask.png")
    row = {"img_path": "im.png", "encode_text": "a cat", "decode_text": "a dog"}
    sys.path.insert(0, ROOT)
    import main as driver

    def run(rows, name):
        (tmp_path / (name + ".json")).write_text(json.dumps(rows))
        out = tmp_path / name
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert driver.main(["--cfg", "experiments/bench_sd_c2.cfg", "--data", str(tmp_path / (name + ".json")),
                                "--output_dir", str(out), "--per_device_eval_batch_size", "2", "--synthetic-weights"]) == 0
        return json.loads((out / "metrics.json").read_text())

    masked = run([dict(row, mask_path="mask.png"), row], "masked")
    plain = run([row, row], "plain")
    a, b = masked["samples"]
    assert np.isfinite(a["psnr_keep"]) and np.isfinite(a["psnr_edit"])
    assert "psnr_keep" not in b and "psnr_edit" not in b
    assert set(masked["summary"]) == set(plain["summary"]) | {"psnr_keep", "psnr_edit"}
    assert set(a) - {"psnr_keep", "psnr_edit"} == set(b) == set(plain["samples"][0])
    assert masked["summary"]["psnr_keep"] == a["psnr_keep"]
