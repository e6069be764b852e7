"""Fused windows on the coupled translate loop (include/cyclediff.h cd_translate_args.n_win, cd_op_window_gather /
cd_op_window_fuse, cd_vae_encode_hw / cd_vae_decode_hw; csrc/windows.hip).

  1. the two kernels against torch, bit for bit, on the three canvases of tests/_windows_ref.py
  2. one window on a 16 x 16 canvas is the call without windows, bit for bit
  3. the windowed loop end to end against the torch restatement, and the cycle of one prompt at guidance 1
  4. refusals, each with its own text, the outputs untouched
  5. the rectangular first stage
  6. the wrapper switch `window_stride`
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _attn_control_ref as acr
import _ops
import _windows_ref as wr
import golden_util as gu
from _ops import bf16_round as r16
from cycle_diffusion_amd import _ffi, schedule, windows
from cycle_diffusion_amd._ffi import check, ptr
from oracle import nets
from test_gpu_models import NET_MEAN, NET_REL, _load, tiny_sd_desc, tiny_vae_desc

pytestmark = pytest.mark.gpu

FMT = 1.0 if _ffi.load_library().cd_act_format() == 1 else 8.0
DDIM = _ffi.CD_SCHED_DDIM
S = wr.S
CANVAS_IDS = ["%dx%d_s%d" % c for c in wr.CANVASES]


# ------------------------------------------------------------------------------------------------ 1. the kernels
def op_gather(eng, x, win, cpad, dup):
    Bp, Cc, Hc, Wc = x.shape
    win = np.ascontiguousarray(win, dtype=np.int32)
    y = torch.empty((1 + dup) * len(win) * Bp, S * S, cpad, device="cuda")
    check(eng.lib.cd_op_window_gather(eng.h, ptr(_ops.dev(x)), C.c_void_p(win.ctypes.data), len(win), Bp, Cc, Hc, Wc, S, cpad,
                                      dup, ptr(y)))
    return y.cpu()


def op_fuse(eng, e, win, Bp, Cc, Hc, Wc, parts):
    win = np.ascontiguousarray(win, dtype=np.int32)
    out = torch.empty(parts * Bp, Cc, Hc, Wc, device="cuda")
    check(eng.lib.cd_op_window_fuse(eng.h, ptr(_ops.dev(e)), C.c_void_p(win.ctypes.data), len(win), Bp, Cc, Hc, Wc, S, e.shape[-1],
                                    parts, ptr(out)))
    return out.cpu()


@pytest.mark.parametrize("dup", [0, 1])
@pytest.mark.parametrize("canvas", wr.CANVASES, ids=CANVAS_IDS)
def test_window_gather_is_the_rounded_crop(engine, canvas, dup):
    Hc, Wc, stride = canvas
    win = windows.window_grid(Hc, Wc, S, stride)
    x = gu.rnd((3, 4, Hc, Wc), 21)
    got = op_gather(engine, x, win, 32, dup)
    assert torch.equal(got, wr.gather_ref(x, win, S, 32, dup, r16))
    # a channel count that fills more than one 16-byte item and is no multiple of 8
    x = gu.rnd((1, 11, Hc, Wc), 22)
    assert torch.equal(op_gather(engine, x, win, 32, dup), wr.gather_ref(x, win, S, 32, dup, r16))


@pytest.mark.parametrize("parts,ld,Cc", [(1, 4, 4), (2, 4, 4), (2, 6, 4), (1, 4, 3)], ids=["p1", "p2", "p2_ld6", "c3"])
@pytest.mark.parametrize("canvas", wr.CANVASES, ids=CANVAS_IDS)
def test_window_fuse_is_the_fp32_restatement(engine, canvas, parts, ld, Cc):
    """(C, ld) = (4, 4) takes the one-pixel-per-lane form, the others the generic one"""
    Hc, Wc, stride = canvas
    win = windows.window_grid(Hc, Wc, S, stride)
    Bp = 3
    e = gu.rnd((parts * len(win) * Bp, S * S, ld), 23)
    e[0, 0, 0] = -0.0  # canvas cell (0, 0) has one covering window: its value comes back bit for bit
    got = op_fuse(engine, e, win, Bp, Cc, Hc, Wc, parts)
    ref = wr.fuse_ref(e, win, Bp, Cc, Hc, Wc, S, parts)
    assert torch.equal(got, ref), (got - ref).abs().max().item()
    assert torch.signbit(got[0, 0, 0, 0])


# ------------------------------------------------------------------------------------------------ 2. / 3. the loop
def _setup(engine, Hc, Wc):
    fx = gu.load("latent_cycle_tiny")
    net, sd = _load(engine, tiny_sd_desc(), fx)
    x0, c, uc, c2 = wr.canvas_inputs(Hc, Wc)
    e = acr.E2E
    sch = schedule.DDIMSchedule(schedule.latent_alphas_cumprod(), e["S"], e["eta"])
    return net, x0, c, uc, c2, sch, e["skip"], wr.canvas_noise(Hc, Wc)


def _kw(c, uc, c2, noise, n_dec=1, dec_g=acr.E2E["dec_g"]):
    return dict(enc_ctx_c=c.cuda(), enc_ctx_uc=uc.cuda(), enc_guidance=1.0, dec_ctx_c=c2.repeat(n_dec, 1, 1).cuda(),
                dec_ctx_uc=uc.repeat(n_dec, 1, 1).cuda(), dec_guidance=dec_g, n_dec=n_dec, noise=torch.stack(noise, 0).cuda())


@pytest.mark.parametrize("n_dec", [1, 2])
def test_one_window_is_the_call_without_windows_bit_for_bit(engine, n_dec):
    net, x0, c, uc, c2, sch, skip, noise = _setup(engine, 16, 16)
    ce, cd = sch.coef_encode(skip), sch.coef_decode(skip)
    g = acr.E2E["dec_g"] if n_dec == 1 else [1.5] * 2 + [4.0] * 2
    kw = _kw(c, uc, c2, noise, n_dec, g)
    z0, x0_ = engine.cycle_translate(net, DDIM, x0.cuda(), ce, cd, **kw)
    z1, x1 = engine.cycle_translate(net, DDIM, x0.cuda(), ce, cd, windows=[[0, 0]], **kw)
    engine.synchronize()
    assert torch.isfinite(x1).all()
    assert torch.equal(z0, z1) and torch.equal(x0_, x1), ((z0 - z1).abs().max().item(), (x0_ - x1).abs().max().item())


@pytest.mark.parametrize("canvas", wr.CANVASES, ids=CANVAS_IDS)
def test_windowed_loop_vs_restatement(engine, report, canvas):
    """The bound tests/test_gpu_attn_control.py holds its uncontrolled end-to-end run to on this network and chain: 8e-3 x
    format factor of the maximum, 40 dB (bf16 build: 25 dB); the averaging amplifies no rounding. A fuse that took the first
    covering window would be 1.2e-1 .. 2.0e-1 away (tests/test_windows_host.py)."""
    Hc, Wc, stride = canvas
    net, x0, c, uc, c2, sch, skip, noise = _setup(engine, Hc, Wc)
    win = windows.window_grid(Hc, Wc, S, stride)
    z, x = engine.cycle_translate(net, DDIM, x0.cuda(), sch.coef_encode(skip), sch.coef_decode(skip), windows=win,
                                  **_kw(c, uc, c2, noise))
    engine.synchronize()
    assert z.shape == (2, len(noise) + 1, 4, Hc, Wc) and x.shape == (2, 4, Hc, Wc)
    zr, xr = wr.restatement(*canvas)
    floor = 40.0 if FMT == 1.0 else 25.0
    assert torch.equal(z[:, 0].cpu(), zr[:, 0])  # x_T: scheduler arithmetic on the canvas, no network
    for name, got, ref in (("z", z.cpu(), zr), ("x", x.cpu(), xr)):
        d = got - ref
        rel = (d.abs().max() / ref.abs().max()).item()
        db = (20.0 * torch.log10(ref.abs().max() / d.pow(2).mean().sqrt())).item()
        report.add("windows/e2e_%s_%dx%d_s%d" % ((name,) + canvas), rel_to_max=rel, psnr_db=db)
        print("windows/e2e_%s %s rel_to_max=%.3e psnr=%.2f dB" % (name, canvas, rel, db))
        assert torch.isfinite(got).all() and rel < 8e-3 * FMT and db > floor, (name, canvas, rel, db)


def test_the_cycle_closes_on_a_canvas(engine, report):
    """the same prompt both ways at guidance 1: encoder and decoder read the same fused prediction, so the decode retraces the
    encoder - the `cyc` bound of tests/test_gpu_models.py::test_latent_cycle_tiny"""
    Hc, Wc, stride = 24, 24, 8
    net, x0, c, uc, _c2, sch, skip, noise = _setup(engine, Hc, Wc)
    _z, x = engine.cycle_translate(net, DDIM, x0.cuda(), sch.coef_encode(skip), sch.coef_decode(skip),
                                   windows=windows.window_grid(Hc, Wc, S, stride), **_kw(c, uc, c, noise, dec_g=1.0))
    cyc = (x.cpu() - x0).abs().max().item()
    report.add("windows/cycle_maxabs_24x24_s8", err=cyc)
    print("windows/cycle_maxabs %.3e" % cyc)
    assert cyc < 8e-3 * FMT, cyc


# ------------------------------------------------------------------------------------------------ 4. refusals
def _raw_args(net, x0, ctx, ce, cd, z, x, Hc, Wc, win):
    """a cd_translate_args of an unguided call on caller-owned outputs; returns (args, what must outlive the call)"""
    a = _ffi.TranslateArgs(size=C.sizeof(_ffi.TranslateArgs))
    a.net, a.sched_kind, a.x0, a.ctx_len, a.B, a.n_dec, a.K = net, DDIM, ptr(x0), ctx.shape[1], x0.shape[0], 1, len(cd)
    a.enc_ctx_c, a.enc_guidance, a.dec_ctx_c, a.dec_guidance = ptr(ctx), 1.0, ptr(ctx), 1.0
    a.coef_enc_host, a.coef_dec_host, a.seed, a.last_uses_x0 = ce.ctypes.data, cd.ctypes.data, 3, 1
    a.z_out, a.x_out = ptr(z), ptr(x)
    w = None if win is None else np.ascontiguousarray(win, dtype=np.int32).reshape(-1, 2)
    a.canvas_h, a.canvas_w = Hc, Wc
    if w is not None:
        a.n_win, a.win_host = len(w), w.ctypes.data
    return a, w


def test_windows_refuse_what_they_cannot_do(engine):
    fx = gu.load("latent_cycle_tiny")
    net, _sd = _load(engine, tiny_sd_desc(), fx)
    d32 = tiny_sd_desc()
    d32.precision = _ffi.CD_PREC_F32
    net32, _ = _load(engine, d32, fx)
    Hc, Wc = 16, 24
    x0, c, _uc, _c2 = wr.canvas_inputs(Hc, Wc)
    x0, ctx = x0.cuda(), c.cuda()
    sch = schedule.DDIMSchedule(schedule.latent_alphas_cumprod(), 4, 0.1)
    ce, cd = np.ascontiguousarray(sch.coef_encode(0)), np.ascontiguousarray(sch.coef_decode(0))
    z = torch.full((2, len(cd) + 1, 4, Hc, Wc), 7.0, device="cuda")
    x = torch.full((2, 4, Hc, Wc), 7.0, device="cuda")
    good = [[0, 0], [0, 8]]
    zero = dict(mask=_ffi.KeepMask(), ctrl=_ffi.AttnCtrl(), blend=_ffi.LocalBlend(), sega=_ffi.Sega())

    def refused(text, win=good, canvas=(Hc, Wc), n_win=None, net_=net, opt=None):
        a, keep = _raw_args(net_, x0, ctx, ce, cd, z, x, canvas[0], canvas[1], win)
        if n_win is not None:
            a.n_win = n_win
        if opt is not None:
            setattr(a, opt, C.pointer(zero[opt]))
        rc = engine.lib.cd_cycle_translate(engine.h, C.byref(a))
        msg = engine.lib.cd_last_error().decode()
        engine.synchronize()
        assert rc != 0 and text in msg, (text, rc, msg)
        assert bool((z == 7.0).all()) and bool((x == 7.0).all()), text  # nothing was launched
        return msg

    msgs = [refused("n_win = 65 outside", n_win=65), refused("n_win = -1 outside", n_win=-1),
            refused("is smaller than the network", win=[[0, 0]], canvas=(8, 24)),
            refused("lies outside the", win=[[0, 0], [0, 9]]), refused("lies outside the", win=[[0, 0], [1, 8]]),
            refused("are equal", win=[[0, 0], [0, 8], [0, 0]]),
            refused("no window covers canvas cell (0, 20)", win=[[0, 0], [0, 4]]),
            refused("CD_PREC_F32", net_=net32),
            refused("n_win = 0 (off) takes", win=None)]
    msgs += [refused("not built together", opt=o) for o in ("mask", "ctrl", "blend", "sega")]
    assert len(set(msgs[:9])) == 9  # each refusal its own text
    a, keep = _raw_args(net, x0, ctx, ce, cd, z, x, Hc, Wc, good)  # the engine is usable after the refusals
    check(engine.lib.cd_cycle_translate(engine.h, C.byref(a)))
    engine.synchronize()
    assert torch.isfinite(x).all() and not bool((x == 7.0).any())


# ------------------------------------------------------------------------------------------------ 5. first stage
def test_rectangular_first_stage_vs_oracle(engine, report):
    fx = gu.load("vae_tiny")
    net, sd = _load(engine, tiny_vae_desc(), fx)
    img = torch.rand((2, 3, 64, 96), generator=torch.Generator().manual_seed(4)) * 2 - 1
    with torch.no_grad():
        mom = nets.vae_encode_moments(sd, gu.TINY_VAE_CFG, img)
    z = engine.vae_encode(net, img.cuda(), sample=False, scale=1.0)
    assert z.shape == (2, 4, 16, 24)
    for name, got, ref in (("mean", z, mom[:, :4]),):
        st = _ops.err_stats(got, ref)
        report.add("windows/vae_64x96_" + name, **st)
        print("windows/vae_64x96_%s %s" % (name, st))
        assert st["finite"] and st["rel_to_max"] < NET_REL and st["mean_rel"] < NET_MEAN, (name, st)
    zz = gu.rnd((2, 4, 16, 24), 5, 0.5)
    with torch.no_grad():
        ref = nets.vae_decode(sd, gu.TINY_VAE_CFG, zz)
    dec = engine.vae_decode(net, zz.cuda(), scale=1.0)
    assert dec.shape == (2, 3, 64, 96)
    st = _ops.err_stats(dec, ref)
    report.add("windows/vae_64x96_decode", **st)
    print("windows/vae_64x96_decode %s" % (st,))
    assert st["finite"] and st["rel_to_max"] < NET_REL and st["mean_rel"] < NET_MEAN, st
    # the other orientation runs too
    assert torch.isfinite(engine.vae_encode(net, img.transpose(2, 3).contiguous().cuda(), sample=False)).all()


def test_square_calls_through_the_hw_entry_points_keep_their_bits(engine):
    fx = gu.load("vae_tiny")
    net, _sd = _load(engine, tiny_vae_desc(), fx)
    img = (torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(4)) * 2 - 1).cuda()
    nz = gu.rnd((2, 4, 16, 16), 77).cuda()
    z_sq = engine.vae_encode(net, img, noise=nz, sample=True, scale=0.18215)
    z_hw = torch.empty_like(z_sq)
    check(engine.lib.cd_vae_encode_hw(engine.h, net, ptr(img), ptr(nz), C.c_uint64(0), 2, 64, 64, 1, C.c_float(0.18215), ptr(z_hw)))
    zz = gu.rnd((2, 4, 16, 16), 5, 0.5).cuda()
    d_sq = engine.vae_decode(net, zz, scale=0.18215, out_mul=0.5, out_add=0.5)
    d_hw = torch.empty_like(d_sq)
    check(engine.lib.cd_vae_decode_hw(engine.h, net, ptr(zz), 2, 16, 16, C.c_float(0.18215), C.c_float(0.5), C.c_float(0.5),
                                      ptr(d_hw)))
    engine.synchronize()
    assert torch.equal(z_sq, z_hw) and torch.equal(d_sq, d_hw)
    with pytest.raises(RuntimeError, match="no multiple of the factor"):
        engine.vae_encode(net, torch.zeros(1, 3, 64, 66).cuda())


# ------------------------------------------------------------------------------------------------ 6. wrapper
def _tiny_wrapper(cls=None, **kw):
    from test_gpu_wrappers import _make
    return _make(True, cls=cls, **kw)


def test_wrapper_window_switch(report):
    """the SD-family text wrapper at the size the wrapper tests use (tests/test_gpu_wrappers.py): tiny VAE, factor 4, a 64 x 96
    image is a 16 x 24 latent, two windows at stride 8"""
    from test_gpu_wrappers import TinyLdmTextWrapper
    common = dict(n_trials=1, skip_steps=[4])
    image = torch.rand((2, 3, 64, 96), generator=torch.Generator().manual_seed(5)).cuda()
    src, tgt = ["a photo of a cat", "a red car"], ["a photo of a small dog", "a blue car"]
    w0, _e, _u, _v = _tiny_wrapper(decoder_unconditional_guidance_scales=[3.0], **common)
    with torch.no_grad(), pytest.raises(AssertionError):
        w0.translate(image, src, tgt)  # window_stride = 0: today's assertion
    w1, _e, _u, _v = _tiny_wrapper(decoder_unconditional_guidance_scales=[3.0], window_stride=8, **common)
    calls = []
    real = w1.engine.cycle_translate
    w1.engine.cycle_translate = lambda *a, **k: (calls.append(np.asarray(k["windows"]).tolist()), real(*a, **k))[1]
    try:
        torch.manual_seed(9)
        with torch.no_grad():
            img = w1.translate(image, src, tgt)
    finally:
        w1.engine.cycle_translate = real
    assert calls == [[[0, 0], [0, 8]]] and w1.last_translate_coupled
    assert img.shape == (2, 3, 64, 96) and torch.isfinite(img).all()
    assert w1.last_latents[0].shape == (2, 4, 16, 24)
    # a budget of one sample's rows (3 x 2 windows) per call: two calls of one sample each, the same draws - the latents agree
    # within the end-to-end bound (another batch may take other GEMM tiles, so not bit for bit)
    lat = w1.last_latents[0].clone()
    w1.couple_max_tokens = 3 * 2 * S * S
    sizes = []
    w1.engine.cycle_translate = lambda *a, **k: (sizes.append(a[2].shape[0]), real(*a, **k))[1]
    try:
        torch.manual_seed(9)
        with torch.no_grad():
            w1.translate(image, src, tgt)
    finally:
        w1.engine.cycle_translate = real
    rel = ((w1.last_latents[0] - lat).abs().max() / lat.abs().max()).item()
    print("windows/wrapper_chunked rel_to_max=%.3e" % rel)
    assert sizes == [1, 1] and rel < 8e-3 * FMT, (sizes, rel)
    # same text both ways at scales 1 on the posterior-mean twin: the latent comes back to the first-stage encoding, whose
    # decode is the first-stage round trip - the bound tests/test_gpu_attn_control.py holds its same-text case to
    w2, _e, _u, _v = _tiny_wrapper(cls=TinyLdmTextWrapper, decoder_unconditional_guidance_scales=[1.0], window_stride=8, **common)
    torch.manual_seed(9)
    with torch.no_grad():
        img_c = w2.translate(image, src, src)
        x0 = w2.engine.vae_encode(w2.vae, (image - 0.5) * 2.0, sample=False, scale=w2.SCALE_FACTOR)
        trip = w2.engine.vae_decode(w2.vae, x0, scale=w2.SCALE_FACTOR, out_mul=0.5, out_add=0.5)
    err = (w2.last_latents[0] - x0).abs().max().item()
    report.add("windows/wrapper_same_text", latent_maxabs=err, image_maxabs=(img_c - trip).abs().max().item())
    print("windows/wrapper_same_text latent maxabs=%.3e image maxabs=%.3e" % (err, (img_c - trip).abs().max().item()))
    assert torch.isfinite(img_c).all() and err < 8e-3 * FMT, err


def test_wrappers_refuse_windows_where_they_cannot_exist():
    w, _emb, _u, _v = _tiny_wrapper(n_trials=1, skip_steps=[0], decoder_unconditional_guidance_scales=[3.0], window_stride=8)
    image = torch.rand((2, 3, 64, 96), generator=torch.Generator().manual_seed(5)).cuda()
    src, tgt = ["a cat", "a car"], ["a dog", "a bus"]
    with torch.no_grad():
        with pytest.raises(ValueError, match="translate"):
            w.encode(image, src)
        with pytest.raises(ValueError, match="translate"):
            w([torch.zeros(2, 8).cuda()], image, src, tgt)
        with pytest.raises(ValueError, match="mask="):
            w.translate(image, src, tgt, mask=torch.ones(2, 1, 64, 96).cuda())
        with pytest.raises(ValueError, match="attn_ctrl="):
            w.translate(image, src, tgt, attn_ctrl=acr.e2e_control())
        with pytest.raises(ValueError, match="local_blend"):
            w.translate(image, src, tgt, local_blend=(["cat"], ["dog"]))
        from cycle_diffusion_amd import semantic_guidance as sgm
        with pytest.raises(ValueError, match="edit_concepts"):
            w.translate(image, src, tgt, edit_concepts=sgm.parse_concepts("+glasses:5:0.9"))
        with pytest.raises(ValueError, match="multiples of 4 and at least 64"):
            w.translate(image[:, :, :, :62], src, tgt)
        with pytest.raises(ValueError, match="multiples of 4 and at least 64"):
            w.translate(image[:, :, :48], src, tgt)
    from cycle_diffusion_amd.gan_wrapper import baselines
    with pytest.raises(ValueError, match="window_stride"):
        baselines.SDDDIBTextWrapper(source_model_type="none", custom_steps=4, window_stride=8)
    with pytest.raises(ValueError, match="window_stride"):
        _tiny_wrapper(window_stride=8, precision="fp32")
