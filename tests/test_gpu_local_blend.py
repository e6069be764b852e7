"""Prompt-to-prompt's local blend on the coupled translate loop (include/cyclediff.h cd_local_blend /
cd_op_local_blend_mask; csrc/automask.hip k_local_blend_mask).

  1. the mask kernel against the torch rule (attn_control.blend_mask on either map, then the union): exact equality
  2. what must stay bit-identical: n_start = K, thr = -1, thr = 1, samples and folded members alone, both batch layouts, the
     CFG shared prefix, keep_out against the mask kernel on acc_out, the same call twice, the forward and cd_word_maps around it
  3. the sums and the blended loop against the torch restatement (tests/_local_blend_ref.py)
  4. refusals, each with its message
  5. the wrapper switch `local_blend`
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _attn_control_ref as acr
import _local_blend_ref as lbr
import golden_util as gu
from cycle_diffusion_amd import _ffi, schedule
from cycle_diffusion_amd._ffi import ptr
from test_gpu_models import _load, tiny_sd_desc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FMT = 1.0 if _ffi.load_library().cd_act_format() == 1 else 8.0
DDIM = _ffi.CD_SCHED_DDIM
E = lbr.E2E


# ------------------------------------------------------------------------------------------------ 1. the mask kernel
@pytest.mark.parametrize("case", lbr.MASK_CASES, ids=["b%d_bd%d_s%d_f%d_p%d" % c for c in lbr.MASK_CASES])
def test_mask_kernel_equals_the_torch_rule(engine, case):
    B, Bd, side, f, pool = case
    src, tgt = lbr.mask_operands(case)
    got = engine.local_blend_mask(src.cuda(), tgt.cuda(), f=f, pool=pool, thr=lbr.MASK_THR).cpu()
    want = lbr.mask_ref(src, tgt, f, pool, lbr.MASK_THR)
    assert tuple(got.shape) == (Bd, 1, side * f, side * f)
    assert 0 < float(want.mean()) < 1 and torch.equal(got, want), (got != want).sum().item()


@pytest.mark.parametrize("name", lbr.MASK_SPECIALS)
def test_mask_kernel_edge_cases(engine, name):
    src, tgt, f, pool, thr = lbr.mask_special(name)
    got = engine.local_blend_mask(src.cuda(), tgt.cuda(), f=f, pool=pool, thr=thr).cpu()
    want = lbr.mask_ref(src, tgt, f, pool, thr)
    assert torch.equal(got, want), (name, (got != want).sum().item())
    edited = (1.0 - got)[0, 0]
    if name == "all_zero":
        assert float(edited.sum()) == 0
    elif name == "corner":  # the 2 x 2 cells the 3 x 3 pool reaches inside the image, each replicated 2 x 2
        assert float(edited.sum()) == 16 and float(edited[:4, 12:].sum()) == 16
    elif name in ("only_src_edits", "only_tgt_edits"):
        assert float(edited.sum()) == 9 and float(edited[2:5, 3:6].sum()) == 9
    else:
        assert float(edited.sum()) == 4 * 18


# ------------------------------------------------------------------------------------------------ 2. bit-exact
@pytest.fixture(scope="module")
def tiny(engine):
    net, sd = _load(engine, tiny_sd_desc(), gu.load("latent_cycle_tiny"))
    x0, c, uc, c2 = acr.e2e_inputs()
    K = E["S"] - E["skip"]
    noise = gu.latent_noise(E["noise_seed"], x0.shape, K)
    sch = schedule.DDIMSchedule(schedule.latent_alphas_cumprod(), E["S"], E["eta"])
    return dict(net=net, sd=sd, x0=x0, c=c, uc=uc, c2=c2, K=K, noise=noise, ce=sch.coef_encode(E["skip"]),
                cd=sch.coef_decode(E["skip"]), sel_s=lbr.key_selector(E["keys_src"]), sel_t=lbr.key_selector(E["keys_tgt"]))


def _kw(t, n_dec=1, dec_g=E["dec_g"], enc_g=1.0, rows=slice(None)):
    B = t["x0"][rows].shape[0]
    nz = torch.stack(t["noise"], 0)[:, rows].contiguous()
    return dict(enc_ctx_c=t["c"][rows].cuda(), enc_ctx_uc=t["uc"][rows].cuda(), enc_guidance=enc_g,
                dec_ctx_c=t["c2"][rows].repeat(n_dec, 1, 1).cuda(), dec_ctx_uc=t["uc"][rows].repeat(n_dec, 1, 1).cuda(),
                dec_guidance=dec_g, n_dec=n_dec, noise=nz.cuda()), B


def _blend(engine, t, side=E["side"], pool=E["pool"], thr=E["thr"], n_start=E["n_start"], ctrl=None, rows=slice(None), **kwa):
    kw, _B = _kw(t, rows=rows, **kwa)
    out = engine.cycle_translate_blend(t["net"], DDIM, t["x0"][rows].cuda(), t["ce"], t["cd"], t["sel_s"], t["sel_t"], side,
                                       pool=pool, thr=thr, n_start=n_start, ctrl=ctrl, **kw)
    engine.synchronize()
    return out


def _plain(engine, t, ctrl=None, rows=slice(None), **kwa):
    kw, _B = _kw(t, rows=rows, **kwa)
    if ctrl is None:
        out = engine.cycle_translate(t["net"], DDIM, t["x0"][rows].cuda(), t["ce"], t["cd"], **kw)
    else:
        out = engine.cycle_translate_ctrl(t["net"], DDIM, t["x0"][rows].cuda(), t["ce"], t["cd"], *ctrl, **kw)
    engine.synchronize()
    return out


# encoder guidance 1: rows [enc cond | dec uncond | dec cond], the decoder's cond half repeats its uncond half (dup_tail);
# encoder guidance 2: rows [enc uncond | enc cond | dec uncond | dec cond], no repeated tail, the source rows start at B
LAYOUTS = pytest.mark.parametrize("enc_g", [1.0, 2.0], ids=["dup_tail", "enc_cfg"])


@LAYOUTS
def test_n_start_K_is_the_unblended_call_bit_for_bit(engine, tiny, enc_g):
    z0, x0_ = _plain(engine, tiny, enc_g=enc_g)
    z1, x1, acc, keep = _blend(engine, tiny, n_start=tiny["K"], enc_g=enc_g)
    assert torch.equal(z0, z1) and torch.equal(x0_, x1)
    assert bool((keep == 1).all()) and float(acc.min()) > 0 and torch.isfinite(acc).all()


@LAYOUTS
def test_threshold_below_zero_edits_everywhere(engine, tiny, enc_g):
    z0, x0_ = _plain(engine, tiny, enc_g=enc_g)
    z1, x1, _acc, keep = _blend(engine, tiny, thr=-1.0, n_start=0, enc_g=enc_g)
    assert bool((keep == 0).all()) and torch.equal(z0, z1) and torch.equal(x0_, x1)
    ctl = acr.e2e_control() + (3,)
    z2, x2 = _plain(engine, tiny, ctrl=ctl, enc_g=enc_g)
    z3, x3, _acc, keep = _blend(engine, tiny, thr=-1.0, n_start=0, ctrl=ctl, enc_g=enc_g)
    assert bool((keep == 0).all()) and torch.equal(z2, z3) and torch.equal(x2, x3) and not torch.equal(x2, x0_)


@LAYOUTS
def test_threshold_one_keeps_the_source_bit_for_bit(engine, tiny, enc_g):
    z0, _x = _plain(engine, tiny, enc_g=enc_g)
    z1, x1, _acc, keep = _blend(engine, tiny, thr=1.0, n_start=0, n_dec=2, dec_g=[1.5] * 2 + [4.0] * 2, enc_g=enc_g)
    assert bool((keep == 1).all()) and torch.equal(z0, z1)
    assert torch.equal(x1, tiny["x0"].repeat(2, 1, 1, 1).cuda())


def test_each_sample_equals_the_sample_alone(engine, tiny):
    z, x, acc, keep = _blend(engine, tiny)
    B = tiny["x0"].shape[0]
    assert 0 < float(keep.mean()) < 1
    for b in range(B):
        zb, xb, accb, keepb = _blend(engine, tiny, rows=slice(b, b + 1))
        assert torch.equal(z[b:b + 1], zb) and torch.equal(x[b:b + 1], xb) and torch.equal(keep[b:b + 1], keepb)
        assert torch.equal(acc[[b, B + b]], accb)


def test_folded_ensemble_equals_each_member_alone(engine, tiny):
    B = tiny["x0"].shape[0]
    z, x, acc, keep = _blend(engine, tiny, n_dec=2, dec_g=[1.5] * B + [4.0] * B)
    for j, g in enumerate((1.5, 4.0)):
        zj, xj, accj, keepj = _blend(engine, tiny, dec_g=g)
        rows = slice(j * B, (j + 1) * B)
        assert torch.equal(z, zj) and torch.equal(x[rows], xj) and torch.equal(keep[rows], keepj)
        assert torch.equal(acc[:B], accj[:B]) and torch.equal(acc[B + j * B:B + (j + 1) * B], accj[B:])
    assert (x[:B] - x[B:]).abs().max() > 1e-3


@LAYOUTS
def test_keep_out_is_the_mask_kernel_on_acc_out_and_runs_repeat(engine, tiny, enc_g):
    z, x, acc, keep = _blend(engine, tiny, enc_g=enc_g)
    B = tiny["x0"].shape[0]
    again = engine.local_blend_mask(acc[:B], acc[B:], f=16 // E["side"], pool=E["pool"], thr=E["thr"])
    assert torch.equal(keep, again) and 0 < float(keep.mean()) < 1
    z2, x2, acc2, keep2 = _blend(engine, tiny, enc_g=enc_g)
    assert torch.equal(z, z2) and torch.equal(x, x2) and torch.equal(acc, acc2) and torch.equal(keep, keep2)
    _z, xu = _plain(engine, tiny, enc_g=enc_g)
    assert not torch.equal(x, xu)


def test_cfg_shared_prefix_on_and_off_give_the_same_bits(engine, tiny, tmp_path):
    """CYCLEDIFF_CFG_SHARE is read once per process: the off run is a child process (tests/_local_blend_child.py)"""
    z, x, acc, keep = _blend(engine, tiny, ctrl=acr.e2e_control() + (3,))
    out = str(tmp_path / "share_off.npz")
    env = dict(os.environ, CYCLEDIFF_CFG_SHARE="0")
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(HERE), HERE] + [p for p in [env.get("PYTHONPATH")] if p])
    r = subprocess.run([sys.executable, os.path.join(HERE, "_local_blend_child.py"), out], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    off = np.load(out)
    for name, got in (("z", z), ("x", x), ("acc", acc), ("keep", keep)):
        assert np.array_equal(off[name], got.cpu().numpy()), name


def test_the_blend_leaves_the_forward_and_the_word_maps_alone(engine, tiny):
    t = tiny
    x, tv = t["x0"].cuda(), torch.full((2,), 400.0).cuda()
    sel = torch.stack([t["sel_s"], t["sel_t"]], 1).cuda()  # [1, 2, L]
    before = engine.unet_forward(t["net"], x, tv, t["c"].cuda())
    m_before, n = engine.word_maps(t["net"], x, t["c"].cuda(), sel, 400, 0.8, 0.6, n_draws=1, seed=3)
    _blend(engine, t)
    after = engine.unet_forward(t["net"], x, tv, t["c"].cuda())
    m_after, n2 = engine.word_maps(t["net"], x, t["c"].cuda(), sel, 400, 0.8, 0.6, n_draws=1, seed=3)
    engine.synchronize()
    assert torch.isfinite(before).all() and torch.equal(before, after) and n == n2 and torch.equal(m_before, m_after)


# ------------------------------------------------------------------------------------------------ 3. the restatement
@pytest.mark.parametrize("side", [16, 8])
def test_sums_vs_restatement(engine, report, tiny, side):
    """acc_out with n_start = K (no mask ever built: the trajectory is the unblended one) against the float64 sums of the
    oracle network, at DESIGN.md 17's bound: 8e-3 x the format factor, relative to the maximum."""
    t = tiny
    _z, _x, acc, _keep = _blend(engine, t, side=side, n_start=t["K"])
    ref = lbr.coupled_translate_blend(t["sd"], gu.TINY_SD_CFG, t["x0"], t["c"], t["c2"], t["uc"], E["dec_g"], E["S"], E["skip"],
                                      E["eta"], t["noise"], t["sel_s"], t["sel_t"], side, E["pool"], E["thr"], t["K"])["acc"]
    rel = ((acc.cpu().double() - ref).abs().max() / ref.abs().max()).item()
    report.add("local_blend/acc_%d" % side, rel_to_max=rel)
    print("local_blend/acc_%d rel_to_max=%.3e" % (side, rel))
    assert rel < lbr.ACC_REL * FMT, rel


def test_blended_loop_vs_restatement(engine, report, tiny):
    """x_out of the flip-free fixture (tests/test_local_blend_host.py asserts its margin and that the blend moves the result by
    10 x this bound) at DESIGN.md 14's bounds: 8e-3 x the format factor relative to the maximum, 40 dB (bf16 build: 25 dB)."""
    t = tiny
    _z, x, acc, keep = _blend(engine, t)
    ref = lbr.coupled_translate_blend(t["sd"], gu.TINY_SD_CFG, t["x0"], t["c"], t["c2"], t["uc"], E["dec_g"], E["S"], E["skip"],
                                      E["eta"], t["noise"], t["sel_s"], t["sel_t"], E["side"], E["pool"], E["thr"], E["n_start"])
    d = x.cpu() - ref["x"]
    rel = (d.abs().max() / ref["x"].abs().max()).item()
    db = (20.0 * torch.log10(ref["x"].abs().max() / d.pow(2).mean().sqrt())).item()
    acc_rel = ((acc.cpu().double() - ref["acc"]).abs().max() / ref["acc"].abs().max()).item()
    flips = int((keep.cpu() != ref["keep"]).sum())
    report.add("local_blend/e2e", rel_to_max=rel, psnr_db=db, acc_rel_to_max=acc_rel, mask_flips=flips)
    print("local_blend/e2e rel_to_max=%.3e psnr=%.2f dB acc=%.3e flips=%d" % (rel, db, acc_rel, flips))
    assert flips == 0
    assert rel < lbr.E2E_REL * FMT and db > (lbr.E2E_DB if FMT == 1.0 else 25.0), (rel, db)


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_blend_entry_point_refuses_what_it_cannot_do(engine, tiny):
    t = tiny
    K, B = t["K"], 2
    lib, h = engine.lib, engine.h
    x0, c, uc, c2 = (v.cuda() for v in (t["x0"], t["c"], t["uc"], t["c2"]))
    nz = torch.stack(t["noise"], 0).cuda()
    sel = torch.cat([t["sel_s"], t["sel_t"], t["sel_s"]], 0).cuda()  # three entries for the B_sel case
    z = torch.full((B, K + 1, 4, 16, 16), -7.0).cuda()
    x = torch.full((B, 4, 16, 16), -7.0).cuda()
    ce, cd = np.ascontiguousarray(t["ce"]), np.ascontiguousarray(t["cd"])

    def entry(net=t["net"], kind=DDIM, ctx=c, enc_g=1.0, dec_g=3.0, cd_=cd, B_sel=1, side=8, pool=3, thr=0.3, n_start=0):
        has = ctx is not None
        blend = _ffi.LocalBlend(sel_src=ptr(sel), sel_tgt=ptr(sel), B_sel=B_sel, side=side, pool=pool, thr=thr, n_start=n_start)
        a = _ffi.TranslateArgs(
            size=C.sizeof(_ffi.TranslateArgs), net=net, sched_kind=kind, x0=ptr(x0), enc_ctx_c=ptr(ctx) if has else None,
            enc_ctx_uc=ptr(uc) if has else None, enc_guidance=enc_g, dec_ctx_c=ptr(c2 if ctx is c else ctx) if has else None,
            dec_ctx_uc=ptr(uc) if has else None, dec_guidance=dec_g, ctx_len=ctx.shape[1] if has else 0, B=B, n_dec=1, K=K,
            coef_enc_host=ce.ctypes.data, coef_dec_host=cd_.ctypes.data, noise=ptr(nz), seed=0, last_uses_x0=1, z_out=ptr(z),
            x_out=ptr(x), blend=C.pointer(blend))
        return lib.cd_cycle_translate(h, C.byref(a))

    err = lambda: lib.cd_last_error().decode()
    d = tiny_sd_desc()
    d.precision = _ffi.CD_PREC_F32
    cd_bad = cd.copy()
    cd_bad["t"][1] += 1
    cases = [
        (dict(net=engine.create_net(d)), "fp32"),
        (dict(kind=_ffi.CD_SCHED_DDPM), "CD_SCHED_DDIM"),
        (dict(ctx=None), "text context"),
        (dict(ctx=torch.zeros(B, 97, 64).cuda()), "context length 97"),
        (dict(dec_g=0.0), "conditional rows"),
        (dict(enc_g=0.0), "conditional rows"),
        (dict(cd_=cd_bad), "disagree"),
        (dict(B_sel=3), "selector entries"),
        (dict(side=4), "no transformer block"),
        (dict(side=5), "does not divide"),
        (dict(side=128), "side = 128"),
        (dict(pool=2), "pool = 2"),
        (dict(pool=9), "pool = 9"),
        (dict(pool=0), "pool = 0"),
        (dict(n_start=-1), "n_start"),
        (dict(n_start=K + 1), "n_start"),
        (dict(thr=float("nan")), "not finite"),
        (dict(thr=float("inf")), "not finite"),
    ]
    for kw, word in cases:
        assert entry(**kw) != 0 and word in err(), (kw, err())
    torch.cuda.synchronize()
    assert bool((x == -7.0).all()) and bool((z == -7.0).all())  # nothing ran
    assert entry() == 0  # the engine is usable after the refusals
    engine.synchronize()
    assert torch.isfinite(x).all()
    with pytest.raises(ValueError, match="no mask"):
        engine._cycle_translate(t["net"], DDIM, x0, t["ce"], t["cd"], c, uc, 1.0, c2, uc, 3.0, 1, nz, 0, True,
                                mask=torch.ones(2, 1, 16, 16).cuda(), mask_source="encoder",
                                blend=(t["sel_s"], t["sel_t"], 8, 3, 0.3, 0))


# ------------------------------------------------------------------------------------------------ 5. wrapper
def _tiny_wrapper(**kw):
    from test_gpu_wrappers import _make
    return _make(True, **kw)[0]


SRC, TGT = ["a photo of a cat", "a red car"], ["a photo of a dog", "a blue car"]


def test_wrapper_same_text_returns_the_first_stage_round_trip():
    w = _tiny_wrapper(n_trials=1, skip_steps=[4], decoder_unconditional_guidance_scales=[3.0], local_blend="words",
                      local_blend_side=8)
    image = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        torch.manual_seed(9)
        x0 = w._first_stage(image)  # the first draw of translate(): the posterior's noise
        torch.manual_seed(9)
        img = w.translate(image, SRC, SRC)
        want = w.engine.vae_decode(w.vae, x0.contiguous(), scale=w.SCALE_FACTOR, out_mul=0.5, out_add=0.5)
    assert w.last_translate_coupled and bool((w.last_local_blend_mask == 1).all())
    assert torch.equal(w.last_latents[0], x0) and torch.equal(img, want)


def test_wrapper_local_blend_switch_and_its_mask():
    from cycle_diffusion_amd import attn_control
    common = dict(n_trials=1, skip_steps=[4], decoder_unconditional_guidance_scales=[3.0])
    w0, w1 = _tiny_wrapper(**common), _tiny_wrapper(local_blend="words", local_blend_threshold=0.8, local_blend_side=8, **common)
    image = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(5)).cuda()
    calls = []
    real = w1.engine.cycle_translate_blend

    def spy(*a, **k):
        out = real(*a, **k)
        calls.append((a, k, out))
        return out

    w1.engine.cycle_translate_blend = spy
    try:
        with torch.no_grad():
            torch.manual_seed(9)
            plain = w0.translate(image, SRC, TGT)
            torch.manual_seed(9)
            img = w1.translate(image, SRC, TGT)
    finally:
        w1.engine.cycle_translate_blend = real
    K = len(w1._schedule()) - 4
    (a, k, out), = calls
    assert a[7] == 8
    assert k["n_start"] == int(0.2 * K) and k["pool"] == 3 and k["thr"] == 0.8 and k["ctrl"] is None
    src_ids, eos = w1._control_ids(SRC)
    tgt_ids, _ = w1._control_ids(TGT)
    for b in range(2):
        ss, st = attn_control.local_blend_selectors(src_ids[b], tgt_ids[b], eos)
        assert np.array_equal(a[5][b].cpu().numpy(), ss) and np.array_equal(a[6][b].cpu().numpy(), st)
    keep = w1.last_local_blend_mask
    h = w1.image_size
    assert tuple(keep.shape) == (2, 1, h, h) and bool(((keep == 0) | (keep == 1)).all()) and torch.equal(keep, out[3])
    assert torch.isfinite(img).all() and not torch.equal(img, plain)
    # words by hand: the same call when they are the words the prompts do not share
    with torch.no_grad():
        torch.manual_seed(9)
        img_w = w1.translate(image, SRC[:1] * 2, TGT[:1] * 2, local_blend=(["cat"], ["dog"]))
        torch.manual_seed(9)
        img_d = w1.translate(image, SRC[:1] * 2, TGT[:1] * 2)
    assert torch.equal(img_w, img_d)


def test_wrappers_refuse_the_blend_where_it_cannot_exist():
    w = _tiny_wrapper(n_trials=1, skip_steps=[0], decoder_unconditional_guidance_scales=[3.0], local_blend="words",
                      local_blend_side=8)
    image = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        with pytest.raises(ValueError, match="translate"):
            w(w.encode(image, SRC), image, SRC, TGT)
        with pytest.raises(ValueError, match="no mask="):
            w.translate(image, SRC, TGT, mask=torch.ones(2, 1, 64, 64))
