"""Cross-attention control on the coupled translate loop (include/cyclediff.h cd_attn_ctrl /
cd_op_cross_attention_ctrl; csrc/attn.hip k_cross_attention_ctrl).

  1. the kernel against float64 torch on 16-bit-rounded inputs, at the bound of tests/test_gpu_ops.py::test_attention
  2. what must stay bit-identical: n_ctrl = 0, the encoder's z under control, folded ensemble members, the CFG shared prefix
  3. the controlled loop end to end against the torch restatement (tests/_attn_control_ref.py: the literal P_src . M form)
  4. refusals, each with its message
  5. the wrapper switch `cac_steps`
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _attn_control_ref as acr
import _ops
import golden_util as gu
from _ops import bf16_round as r16
from cycle_diffusion_amd import _ffi, attn_control, schedule
from cycle_diffusion_amd._ffi import check, ptr
from test_gpu_models import _load, tiny_sd_desc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FMT = 1.0 if _ffi.load_library().cd_act_format() == 1 else 8.0
DDIM = _ffi.CD_SCHED_DDIM
REL, MEAN = 4e-3 * FMT, 1.5e-3 * FMT  # tests/test_gpu_ops.py::test_attention


# ------------------------------------------------------------------------------------------------ 1. the kernel
def ctrl_attention(eng, q_own, q_src, k_own, k_src, v_own, M, alpha, w, H, scale, L=None):
    """cd_op_cross_attention_ctrl on torch tensors; L < k.shape[1]: the caller's key buffers carry rows the op must not use"""
    B, Tq, Cc = q_own.shape
    L_buf = k_own.shape[1]
    L = L_buf if L is None else L
    t = [_ops.dev(x) for x in (q_own, q_src, k_own, k_src, v_own, M, alpha, w)]
    o = torch.empty(B, Tq, Cc, device="cuda")
    check(eng.lib.cd_op_cross_attention_ctrl(eng.h, *[ptr(x) for x in t], B, q_src.shape[0], M.shape[0], H, Tq, L, L_buf,
                                             Cc // H, C.c_float(scale), ptr(o)))
    torch.cuda.synchronize()
    return o.cpu()


def _check(report, name, got, ref):
    st = _ops.err_stats(got, ref.float())
    report.add("attn_control/" + name, **st)
    print("attn_control/%s %s" % (name, st))
    assert st["finite"], name
    assert st["rel_to_max"] < REL and st["mean_rel"] < MEAN, (name, st)


# (B_dec, B_src, H, Tq, L, D): the modulo source index; a strip shorter than the tile; a ragged last strip; the tiny network's
# two head dims; a short context
CTRL_CASES = [(2, 1, 8, 256, 77, 40), (1, 1, 8, 64, 77, 160), (1, 1, 8, 320, 77, 80), (2, 2, 2, 64, 77, 32),
              (1, 1, 2, 256, 77, 64), (1, 1, 1, 64, 33, 40)]


def _operands(case, seed=41):
    B, Bs, H, Tq, L, D = case
    g = torch.Generator().manual_seed(seed)
    Cc = H * D
    rnd = lambda *s: r16(torch.randn(*s, generator=g))
    return dict(q_own=rnd(B, Tq, Cc), q_src=rnd(Bs, Tq, Cc), k_own=rnd(B, L, Cc), k_src=rnd(Bs, L, Cc), v_own=rnd(B, L, Cc)), g


@pytest.mark.parametrize("frac", [False, True], ids=["alpha01", "alpha_fractional"])
@pytest.mark.parametrize("case", CTRL_CASES, ids=["b%d_s%d_h%d_t%d_l%d_d%d" % c for c in CTRL_CASES])
def test_ctrl_attention_vs_float64(engine, report, case, frac):
    B, Bs, H, Tq, L, D = case
    t, g = _operands(case)
    M, alpha, w = acr.random_control(g, Bs, L, fractional=frac)
    ref = acr.ctrl_attention_ref(M=M, alpha=alpha, w=w, H=H, scale=D ** -0.5, **t)
    got = ctrl_attention(engine, t["q_own"], t["q_src"], t["k_own"], t["k_src"], t["v_own"], M, alpha, w, H, D ** -0.5)
    _check(report, "op/%s/%s" % ("x".join(map(str, case)), "frac" if frac else "01"), got, ref)


@pytest.mark.parametrize("case", CTRL_CASES, ids=["b%d_s%d_h%d_t%d_l%d_d%d" % c for c in CTRL_CASES])
def test_ctrl_attention_limits(engine, report, case):
    """alpha = 0, w = 1: plain attention on the row's own Q / K. alpha = 1, M = I: attention(Q_src, K_src, V_own). V = 1: every
    output is sum_j P_j (w and the missing renormalisation)."""
    B, Bs, H, Tq, L, D = case
    t, g = _operands(case, seed=43)
    scale = D ** -0.5
    name = "x".join(map(str, case))
    hs = lambda x: x.double().view(x.shape[0], x.shape[1], H, D).transpose(1, 2)
    src = torch.arange(B) % Bs
    run = lambda M, a, w, **kw: ctrl_attention(engine, kw.get("q_own", t["q_own"]), t["q_src"], t["k_own"], t["k_src"],
                                               kw.get("v_own", t["v_own"]), M, a, w, H, scale)
    eye, one, zero = torch.eye(L).repeat(Bs, 1, 1), torch.ones(Bs, L), torch.zeros(Bs, L)
    p_own = torch.softmax(hs(t["q_own"]) @ hs(t["k_own"]).transpose(-1, -2) * scale, -1)
    p_src = torch.softmax(hs(t["q_src"])[src] @ hs(t["k_src"])[src].transpose(-1, -2) * scale, -1)
    back = lambda o: o.transpose(1, 2).reshape(B, Tq, H * D)
    _check(report, "own/" + name, run(eye, zero, one), back(p_own @ hs(t["v_own"])))
    _check(report, "src/" + name, run(eye, one, one), back(p_src @ hs(t["v_own"])))
    M, alpha, w = acr.random_control(g, Bs, L, fractional=True)
    ctl = torch.arange(B) % Bs
    a, ww = alpha.double()[ctl][:, None, None], w.double()[ctl][:, None, None]
    p = ww * (a * (p_src @ M.double()[ctl][:, None]) + (1 - a) * p_own)
    ones = torch.ones_like(t["v_own"])
    _check(report, "rowsum/" + name, run(M, alpha, w, v_own=ones), back(p.sum(-1, keepdim=True).expand(-1, -1, -1, D)))


def test_ctrl_attention_spike_and_garbage_keys(engine, report):
    """one source score and one own score 30 above the rest (the maximum is subtracted: finite, in bound), and rows L .. 95 of
    the caller's key buffers filled with large values: they must not change a bit of the result"""
    case = (2, 1, 8, 256, 77, 40)
    B, Bs, H, Tq, L, D = case
    t, g = _operands(case, seed=47)
    scale = D ** -0.5
    for name, qrow, krow in (("q_own", 5, 70), ("q_src", 37, 3)):
        kname = "k_own" if name == "q_own" else "k_src"
        for h in range(H):
            d = t[name][0, qrow, h * D:(h + 1) * D]
            t[kname][0, krow, h * D:(h + 1) * D] = d / d.norm() ** 2 * 30.0 / scale
    t = {k: r16(v) for k, v in t.items()}
    M, alpha, w = acr.random_control(g, Bs, L, fractional=True)
    ref = acr.ctrl_attention_ref(M=M, alpha=alpha, w=w, H=H, scale=scale, **t)
    got = ctrl_attention(engine, t["q_own"], t["q_src"], t["k_own"], t["k_src"], t["v_own"], M, alpha, w, H, scale)
    _check(report, "spike", got, ref)
    pad = lambda k: torch.cat([k, torch.full((k.shape[0], 96 - L, k.shape[2]), 3.0e4)], 1)
    got2 = ctrl_attention(engine, t["q_own"], t["q_src"], pad(t["k_own"]), pad(t["k_src"]), t["v_own"], M, alpha, w, H, scale, L=L)
    assert torch.equal(got, got2), (got - got2).abs().max().item()


# ------------------------------------------------------------------------------------------------ 2. bit-exact
def _setup(engine, S=acr.E2E["S"], skip=acr.E2E["skip"], inputs=gu.latent_cycle_inputs):
    fx = gu.load("latent_cycle_tiny")
    net, sd = _load(engine, tiny_sd_desc(), fx)
    x0, c, uc, c2 = inputs()
    K = S - skip
    noise = gu.latent_noise(acr.E2E["noise_seed"], x0.shape, K)
    sch = schedule.DDIMSchedule(schedule.latent_alphas_cumprod(), S, acr.E2E["eta"])
    return net, sd, x0, c, uc, c2, sch, skip, K, noise


def _kw(c, uc, c2, noise, n_dec=1, dec_g=3.0):
    return dict(enc_ctx_c=c.cuda(), enc_ctx_uc=uc.cuda(), enc_guidance=1.0, dec_ctx_c=c2.repeat(n_dec, 1, 1).cuda(),
                dec_ctx_uc=uc.repeat(n_dec, 1, 1).cuda(), dec_guidance=dec_g, n_dec=n_dec, noise=torch.stack(noise, 0).cuda())


def test_n_ctrl_zero_is_the_uncontrolled_call_bit_for_bit(engine):
    net, _sd, x0, c, uc, c2, sch, skip, K, noise = _setup(engine)
    ce, cd = sch.coef_encode(skip), sch.coef_decode(skip)
    ctl = acr.e2e_control()
    kw = _kw(c, uc, c2, noise)
    z0, x0_ = engine.cycle_translate(net, DDIM, x0.cuda(), ce, cd, **kw)
    z1, x1 = engine.cycle_translate_ctrl(net, DDIM, x0.cuda(), ce, cd, *ctl, 0, **kw)
    engine.synchronize()
    assert torch.equal(z0, z1) and torch.equal(x0_, x1)
    mask = torch.zeros(2, 1, 16, 16)
    mask[:, 0, 4:12, 2:9] = 1.0
    z2, x2 = engine.cycle_translate_masked(net, DDIM, x0.cuda(), ce, cd, mask.cuda(), mask_source="encoder", **kw)
    z3, x3 = engine.cycle_translate_ctrl(net, DDIM, x0.cuda(), ce, cd, *ctl, 0, mask=mask.cuda(), mask_source="encoder", **kw)
    engine.synchronize()
    assert torch.equal(z2, z3) and torch.equal(x2, x3)
    assert not torch.equal(x2, x0_)


def test_control_never_reaches_the_encoder_rows(engine):
    net, _sd, x0, c, uc, c2, sch, skip, K, noise = _setup(engine)
    ce, cd = sch.coef_encode(skip), sch.coef_decode(skip)
    kw = _kw(c, uc, c2, noise)
    z0, xu = engine.cycle_translate(net, DDIM, x0.cuda(), ce, cd, **kw)
    z1, xc = engine.cycle_translate_ctrl(net, DDIM, x0.cuda(), ce, cd, *acr.e2e_control(), acr.E2E["n_ctrl"], **kw)
    engine.synchronize()
    assert torch.equal(z0, z1), (z0 - z1).abs().max().item()
    assert torch.isfinite(xc).all() and (xc - xu).abs().max().item() > 1e-3


def test_folded_ensemble_equals_each_member_alone(engine):
    """n_dec = 2 with two guidance scales (the case of tests/test_gpu_coupled.py): both members share their sample's control"""
    net, _sd, x0, c, uc, c2, sch, skip, K, noise = _setup(engine)
    ce, cd = sch.coef_encode(skip), sch.coef_decode(skip)
    B, ctl, n = x0.shape[0], acr.e2e_control(), acr.E2E["n_ctrl"]
    z, x = engine.cycle_translate_ctrl(net, DDIM, x0.cuda(), ce, cd, *ctl, n, **_kw(c, uc, c2, noise, 2, [1.5] * B + [4.0] * B))
    for j, g in enumerate((1.5, 4.0)):
        zj, xj = engine.cycle_translate_ctrl(net, DDIM, x0.cuda(), ce, cd, *ctl, n, **_kw(c, uc, c2, noise, 1, g))
        engine.synchronize()
        assert torch.equal(z, zj) and torch.equal(x[j * B:(j + 1) * B], xj), (g, (x[j * B:(j + 1) * B] - xj).abs().max().item())
    assert (x[:B] - x[B:]).abs().max() > 1e-3


def test_cfg_shared_prefix_on_and_off_give_the_same_bits(engine, tmp_path):
    """CYCLEDIFF_CFG_SHARE is read once per process: the off run is a child process (tests/_attn_control_child.py)"""
    net, _sd, x0, c, uc, c2, sch, skip, K, noise = _setup(engine)
    z, x = engine.cycle_translate_ctrl(net, DDIM, x0.cuda(), sch.coef_encode(skip), sch.coef_decode(skip), *acr.e2e_control(),
                                       acr.E2E["n_ctrl"], **_kw(c, uc, c2, noise))
    engine.synchronize()
    out = str(tmp_path / "share_off.npz")
    env = dict(os.environ, CYCLEDIFF_CFG_SHARE="0")
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(HERE), HERE] + [p for p in [env.get("PYTHONPATH")] if p])
    r = subprocess.run([sys.executable, os.path.join(HERE, "_attn_control_child.py"), out], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    off = np.load(out)
    assert np.array_equal(off["z"], z.cpu().numpy()) and np.array_equal(off["x"], x.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 3. end to end
def test_controlled_loop_vs_restatement(engine, report):
    """Bounds of the 16-bit decode in tests/test_gpu_baselines.py / test_gpu_masked.py: 8e-3 x format factor relative to the
    maximum, 40 dB (bf16 build: 25 dB, as there). The uncontrolled run of the same inputs is recorded next to it. The inputs
    are acr.e2e_inputs(): contexts strong enough that the control moves the restatement by 20 x this bound
    (tests/test_attn_control_host.py::test_the_end_to_end_control_is_no_no_op), so a no-op cannot pass."""
    net, sd, x0, c, uc, c2, sch, skip, K, noise = _setup(engine, inputs=acr.e2e_inputs)
    ce, cd = sch.coef_encode(skip), sch.coef_decode(skip)
    ctl, n, e = acr.e2e_control(), acr.E2E["n_ctrl"], acr.E2E
    kw = _kw(c, uc, c2, noise, dec_g=e["dec_g"])
    _z, xu = engine.cycle_translate(net, DDIM, x0.cuda(), ce, cd, **kw)
    _z, xc = engine.cycle_translate_ctrl(net, DDIM, x0.cuda(), ce, cd, *ctl, n, **kw)
    engine.synchronize()
    floor = 40.0 if FMT == 1.0 else 25.0
    for name, got, ctrl, nn in (("uncontrolled", xu, None, 0), ("controlled", xc, ctl, n)):
        _zr, ref = acr.coupled_translate(sd, gu.TINY_SD_CFG, x0, c, c2, uc, e["dec_g"], e["S"], skip, e["eta"], noise, ctrl, nn)
        d = got.cpu() - ref
        rel = (d.abs().max() / ref.abs().max()).item()
        db = (20.0 * torch.log10(ref.abs().max() / d.pow(2).mean().sqrt())).item()
        report.add("attn_control/e2e_" + name, rel_to_max=rel, psnr_db=db)
        print("attn_control/e2e_%s rel_to_max=%.3e psnr=%.2f dB" % (name, rel, db))
        assert rel < 8e-3 * FMT and db > floor, (name, rel, db)


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_ctrl_entry_point_refuses_what_it_cannot_do(engine):
    net, _sd, x0, c, uc, c2, sch, skip, K, noise = _setup(engine, S=4, skip=0)
    ce, cd = sch.coef_encode(0), sch.coef_decode(0)
    ctl = acr.e2e_control()
    kw = _kw(c, uc, c2, noise)
    run = lambda net_, kind, ce_, cd_, ctl_, n: engine.cycle_translate_ctrl(net_, kind, x0.cuda(), ce_, cd_, *ctl_, n, **kw)
    d = tiny_sd_desc()
    d.precision = _ffi.CD_PREC_F32
    net32, _ = _load(engine, d, gu.load("latent_cycle_tiny"))
    with pytest.raises(RuntimeError, match="fp32"):
        run(net32, DDIM, ce, cd, ctl, 2)
    with pytest.raises(RuntimeError, match="CD_SCHED_DDIM"):
        run(net, _ffi.CD_SCHED_DDPM, ce, cd, ctl, 2)
    with pytest.raises(RuntimeError, match="control shape mismatch"):
        run(net, DDIM, ce, cd, tuple(torch.cat([t, t[:1]], 0) for t in ctl), 2)  # 3 control rows, batch of 2
    with pytest.raises(RuntimeError, match="n_ctrl"):
        run(net, DDIM, ce, cd, ctl, K + 1)
    cd_bad = cd.copy()
    cd_bad["t"][1] += 1
    with pytest.raises(RuntimeError, match="disagree"):
        run(net, DDIM, ce, cd_bad, ctl, 2)
    with pytest.raises(RuntimeError, match="disagree"):
        run(net, DDIM, ce, cd_bad, ctl, 0)
    z, x = run(net, DDIM, ce, cd, ctl, 2)  # the engine is usable after the refusals
    engine.synchronize()
    assert torch.isfinite(x).all()


def _tiny_wrapper(**kw):
    from test_gpu_wrappers import _make
    return _make(True, **kw)


def test_wrappers_refuse_control_where_it_cannot_exist():
    w, _emb, _u, _v = _tiny_wrapper(n_trials=1, skip_steps=[0], decoder_unconditional_guidance_scales=[3.0], cac_steps=0.4)
    image = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        with pytest.raises(ValueError, match="translate"):
            w(w.encode(image, ["a cat", "a car"]), image, ["a cat", "a car"], ["a dog", "a bus"])
    from cycle_diffusion_amd.gan_wrapper import baselines
    with pytest.raises(ValueError, match="cac_steps"):
        baselines.SDDDIBTextWrapper(source_model_type="none", custom_steps=4, cac_steps=0.4)


# ------------------------------------------------------------------------------------------------ 5. wrapper
def test_wrapper_cac_switch():
    """the SD-family text wrapper at the size the wrapper tests use (tests/test_gpu_wrappers.py TinyTextWrapper)"""
    common = dict(n_trials=1, skip_steps=[4])
    image = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(5)).cuda()
    src, tgt = ["a photo of a cat", "a red car"], ["a photo of a small dog", "a blue car"]

    def run(w, s, t):
        torch.manual_seed(9)
        with torch.no_grad():
            img = w.translate(image, s, t)
        return img, w.last_latents[0].clone()

    w0, _e, _u, _v = _tiny_wrapper(decoder_unconditional_guidance_scales=[3.0], **common)
    w1, _e, _u, _v = _tiny_wrapper(decoder_unconditional_guidance_scales=[3.0], cac_steps=0.0, **common)
    w2, _e, _u, _v = _tiny_wrapper(decoder_unconditional_guidance_scales=[3.0], cac_steps=0.4, cac_mode="refine", **common)
    a, _ = run(w0, src, tgt)
    b, _ = run(w1, src, tgt)
    assert torch.equal(a, b)
    calls = []
    real = w2.engine.cycle_translate_ctrl
    w2.engine.cycle_translate_ctrl = lambda *aa, **k: (calls.append(k["n_ctrl"]), real(*aa, **k))[1]
    try:
        cimg, _ = run(w2, src, tgt)
    finally:
        w2.engine.cycle_translate_ctrl = real
    assert calls == [int(0.4 * (len(w2._schedule()) - 4))] and w2.last_translate_coupled
    assert torch.isfinite(cimg).all() and not torch.equal(cimg, a)
    # identical prompts at scale 1: the decoder retraces the encoder, P_src ~ P_own, and the control changes nothing beyond the
    # bound tests/test_gpu_masked.py holds "same text both ways" to
    w3, _e, _u, _v = _tiny_wrapper(decoder_unconditional_guidance_scales=[1.0], **common)
    w4, _e, _u, _v = _tiny_wrapper(decoder_unconditional_guidance_scales=[1.0], cac_steps=0.4, **common)
    _, lat_plain = run(w3, src, src)
    img_c, lat_c = run(w4, src, src)
    err = (lat_c - lat_plain).abs().max().item()
    print("attn_control/wrapper_same_text maxabs=%.3e" % err)
    assert torch.isfinite(img_c).all() and err < 8e-3 * FMT, err
