"""ILVR on the engine (cd_ilvr_decode / cd_op_lowpass, csrc/ilvr.hip): the low-pass filter against float64
within its derived bound, one conditioned step on explicit tensors, the 50-step chains against a torch restatement driven by
the engine's own forward, the bit-for-bit identities, the refusals, and the driver on the toy config. The reference tree has
no ILVR: every yardstick here is tests/_ilvr_ref.py."""
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

import _baselines_ref as br
import _ilvr_ref as ir
import golden_util as gu
from cycle_diffusion_amd import _ffi, engine as cde, schedule
from test_gpu_baselines import _max_rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, C = 32, 3
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def toy(engine):
    """the toy Ho-DDPM in fp32 with the baselines fixture's tamed output layer (tests/_baselines_ref.py synth_weights)"""
    fx = gu.load("baselines_pixel")
    p = json.loads(str(fx["params"]))
    net = engine.create_net(cde.ho_ddpm_desc(32, 32, (1, 2, 2), 1, (16,), precision=_ffi.CD_PREC_F32))
    sd = br.synth_weights(json.loads(str(fx["tgt_names"])), p["tgt_seed"], p["out_prefix"], p["out_scale"])
    assert engine.load_state_dict(net, sd)[0] == 0
    return net


def _rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _image(B, seed):
    """smooth-ish reference images in [-1, 1]"""
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand((B, C, 4, 4), generator=g) * 2 - 1
    y = torch.nn.functional.interpolate(lo, size=(R, R), mode="bilinear", align_corners=False)
    return (0.8 * y + 0.2 * (torch.rand((B, C, R, R), generator=g) * 2 - 1)).cuda().contiguous()


def _eps(engine, net):
    return lambda x, t: engine.unet_forward(net, x.contiguous(), torch.full((x.shape[0],), float(t), device=x.device))


# ------------------------------------------------------------------------------------------------ 1. phi_N against float64
@pytest.mark.parametrize("B,Cc,Rr,N", ir.OP_CASES)
def test_lowpass_op_within_the_derived_bound(engine, report, B, Cc, Rr, N):
    x = ir.op_input(B, Cc, Rr)
    got = engine.op_lowpass(torch.from_numpy(x).cuda(), N).cpu().numpy().astype(np.float64)
    ref, bound = ir.phi64(x, Rr, N), ir.phi_bound(x, Rr, N)
    ratio = float((np.abs(got - ref) / bound).max())
    emu = float(np.abs(got - ir.emulate32(x, Rr, N)).max())
    const = np.full((1, Cc, Rr, Rr), 3.0, dtype=np.float32)
    cu = float(ir.ulps(engine.op_lowpass(torch.from_numpy(const).cuda(), N).cpu().numpy(), const).max())
    print("lowpass R=%d N=%d: max err / bound %.3g, max err %.3g, max bound %.3g, |got - emulation| %.3g, constant %.2f ulp"
          % (Rr, N, ratio, np.abs(got - ref).max(), bound.max(), emu, cu))
    report.add("ilvr/lowpass_R%d_N%d" % (Rr, N), err_over_bound=ratio, max_err=float(np.abs(got - ref).max()),
               max_bound=float(bound.max()), vs_emulation=emu, constant_ulp=cu)
    assert ratio <= 1.0, ratio
    assert cu <= 4.0, cu
    if N == 1:
        assert np.array_equal(got.astype(np.float32), x)


# ------------------------------------------------------------------------------------------------ 2. one conditioned step
def _noop_row0(coef):
    """row 0 made the identity step: x0_hat = (x - 0 e) / 1, x <- 1 x0_hat + 0 e + 0"""
    coef = coef.copy()
    coef[0] = (1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, int(coef["t"][0]))
    return coef


def test_one_conditioned_step_on_explicit_tensors(engine, toy, report):
    """K = 2, range_t = 0, row 0 the identity step: the output is x after row 1. The same call with range_t = 1 gives x', the
    decode step's own output, bit for bit; y' and y' - x' are fp32 elementwise operations torch repeats exactly. What is left
    is phi_N's rounding and the rounding of the final add: |x - (x' + phi(d))| <= bound(d) (1 + 2^-24) + 2^-24 |x' + phi(d)|."""
    B, N = 2, 4
    sch = schedule.PixelSchedule(50, 50, sample_type="ddim", eta=0.1)
    coef = _noop_row0(sch.coef_decode()[[0, 30]])
    q = np.ascontiguousarray(sch.coef_ilvr()[[0, 30]])
    z, y = _rnd((B, 1, C, R, R), 1), _image(B, 2)
    nt, rn = _rnd((2, B, C, R, R), 3), _rnd((2, B, C, R, R), 4)
    kw = dict(noise_tail=nt, ref_noise=rn)
    xp = engine.ilvr_decode(toy, _ffi.CD_SCHED_DDIM, z, coef, y, N, q, range_t=1, **kw)
    x = engine.ilvr_decode(toy, _ffi.CD_SCHED_DDIM, z, coef, y, N, q, range_t=0, **kw)
    plain = engine.ddim_decode(toy, _ffi.CD_SCHED_DDIM, z, coef, n_eps=0, noise_tail=nt)
    engine.synchronize()
    assert torch.equal(xp, plain)
    _want, d = ir.condition(xp, y, q[1, 0], q[1, 1], rn[0], R, N)
    dn = d.cpu().numpy()
    ref = xp.cpu().numpy().astype(np.float64) + ir.phi64(dn, R, N)
    bound = ir.phi_bound(dn, R, N) * (1 + U24) + U24 * np.abs(ref)
    err = np.abs(x.cpu().numpy().astype(np.float64) - ref)
    ratio = float((err / bound).max())
    moved = (x - xp).abs().max().item()
    print("one step: max err / bound %.3g, max err %.3g, the step moved x by %.3g" % (ratio, err.max(), moved))
    report.add("ilvr/one_step", err_over_bound=ratio, max_err=float(err.max()), moved=moved)
    assert ratio <= 1.0 and moved > 0.1, (ratio, moved)


# ------------------------------------------------------------------------------------------------ 3. the chains
@pytest.mark.parametrize("st,eta", [("ddim", 0.1), ("ddpm", None)])
def test_chain_against_the_torch_restatement(engine, toy, report, st, eta):
    B, K, N, rt = 2, 50, 4, 5
    sch = schedule.PixelSchedule(K, K, sample_type=st, eta=eta)
    coef, q = sch.coef_decode(), sch.coef_ilvr()
    z, y = _rnd((B, 1, C, R, R), 11), _image(B, 12)
    nt, rn = _rnd((K, B, C, R, R), 13), _rnd((K, B, C, R, R), 14)
    x = engine.ilvr_decode(toy, sch.kind, z, coef, y, N, q, range_t=rt, noise_tail=nt, ref_noise=rn)
    with torch.no_grad():
        want = ir.ilvr_chain(_eps(engine, toy), sch.kind, z[:, 0], coef, q, y, nt, rn, N, rt)
    rel = _max_rel(x, want)
    print("chain %s: max rel %.3g" % (st, rel))
    report.add("ilvr/chain_%s" % st, max_rel=rel)
    assert torch.isfinite(x).all() and rel < 1e-3, rel


# ------------------------------------------------------------------------------------------------ 4. identities
def test_identities_bit_for_bit(engine, toy):
    K, N = 6, 4
    sch = schedule.PixelSchedule(50, K, sample_type="ddim", eta=0.1)
    coef, q = sch.coef_decode(), sch.coef_ilvr()
    z, y = _rnd((3, 1, C, R, R), 21), _image(3, 22)
    nt, rn = _rnd((K, 3, C, R, R), 23), _rnd((K, 3, C, R, R), 24)
    dec = lambda zz, yy, n1, n2, **kw: engine.ilvr_decode(toy, sch.kind, zz.contiguous(), coef, yy.contiguous(), N, q,
                                                          noise_tail=None if n1 is None else n1.contiguous(),
                                                          ref_noise=None if n2 is None else n2.contiguous(), **kw)
    # range_t = K - 1 conditions nothing: cd_ddim_decode itself
    for rt in (K - 1, K + 3):
        assert torch.equal(dec(z, y, nt, rn, range_t=rt), engine.ddim_decode(toy, sch.kind, z, coef, n_eps=0, noise_tail=nt))
    # a sample's result does not depend on its batch
    x3 = dec(z, y, nt, rn, range_t=1)
    x1 = dec(z[1:2], y[1:2], nt[:, 1:2], rn[:, 1:2], range_t=1)
    assert torch.equal(x3[1:2], x1) and not torch.equal(x3[0:1], x1)
    # one reference shared by two samples is that reference repeated
    a = dec(z[:2], y[:1], nt[:, :2], rn[:, :2], range_t=1)
    b = dec(z[:2], y[:1].repeat(2, 1, 1, 1), nt[:, :2], rn[:, :2], range_t=1)
    assert torch.equal(a, b)
    # the Philox path: one seed, one result; another seed, another
    p1 = dec(z, y, nt, None, range_t=1, ref_seed=7)
    p2 = dec(z, y, nt, None, range_t=1, ref_seed=7)
    p3 = dec(z, y, nt, None, range_t=1, ref_seed=8)
    assert torch.equal(p1, p2) and not torch.equal(p1, p3) and torch.isfinite(p1).all()
    # the 16-bit network takes its next input from the conditioning kernel: the same call twice, and not the unconditioned one
    net16 = engine.create_net(cde.ho_ddpm_desc(32, 32, (1, 2, 2), 1, (16,)))
    engine.random_init(net16, seed=3)
    h1 = engine.ilvr_decode(net16, sch.kind, z, coef, y, N, q, range_t=1, noise_tail=nt, ref_noise=rn)
    h0 = engine.ilvr_decode(net16, sch.kind, z, coef, y, N, q, range_t=K, noise_tail=nt, ref_noise=rn)
    assert torch.equal(h0, engine.ddim_decode(net16, sch.kind, z, coef, n_eps=0, noise_tail=nt))
    assert torch.isfinite(h1).all() and not torch.equal(h1, h0)


# ------------------------------------------------------------------------------------------------ 5. it conditions
def test_conditioning_pulls_the_low_band_to_the_reference(engine, toy, report):
    """N = 4, range_t = 0: the low band of the result lies at least 5 x closer to the reference's than the unconditioned
    decode of the same x_T. The torch restatement alone gives the ratio printed (seed 31: recorded in DESIGN.md 15)."""
    B, K, N = 2, 50, 4
    sch = schedule.PixelSchedule(K, K, sample_type="ddim", eta=0.1)
    coef, q = sch.coef_decode(), sch.coef_ilvr()
    z, y = _rnd((B, 1, C, R, R), 31), _image(B, 32)
    nt, rn = _rnd((K, B, C, R, R), 33), _rnd((K, B, C, R, R), 34)
    with torch.no_grad():
        w_c = ir.ilvr_chain(_eps(engine, toy), sch.kind, z[:, 0], coef, q, y, nt, rn, N, 0)
        w_u = ir.ilvr_chain(_eps(engine, toy), sch.kind, z[:, 0], coef, q, y, nt, rn, N, K)
    ratio_ref = ir.down_norm(w_u - y, R, N) / ir.down_norm(w_c - y, R, N)
    x_c = engine.ilvr_decode(toy, sch.kind, z, coef, y, N, q, range_t=0, noise_tail=nt, ref_noise=rn)
    x_u = engine.ddim_decode(toy, sch.kind, z, coef, n_eps=0, noise_tail=nt)
    ratio = ir.down_norm(x_u - y, R, N) / ir.down_norm(x_c - y, R, N)
    print("conditioning: restatement ratio %.3g, engine ratio %.3g" % (ratio_ref, ratio))
    report.add("ilvr/conditioning", restatement_ratio=ratio_ref, engine_ratio=ratio)
    assert ratio_ref >= 10.0, ratio_ref  # the restatement passes with margin
    assert ratio >= 5.0, ratio


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_engine_usable(engine, toy):
    from test_gpu_models import tiny_sd_desc
    K = 3
    sch = schedule.PixelSchedule(50, K, sample_type="ddim", eta=0.1)
    coef, q = sch.coef_decode(), sch.coef_ilvr()
    z, y = _rnd((2, 1, C, R, R), 41), _image(2, 42)
    good = dict(net=toy, kind=sch.kind, z=z, coef=coef, ref=y, down_n=4, qcoef=q, range_t=0)
    for change, text in ((dict(down_n=3), "divide"), (dict(down_n=16), "fewer than 4"), (dict(down_n=0), "down_n"),
                         (dict(down_n=-2), "down_n"), (dict(range_t=-1), "range_t"),
                         (dict(z=_rnd((3, 1, C, R, R), 43)), "reference")):
        with pytest.raises(_ffi.EngineError, match=text):
            engine.ilvr_decode(**{**good, **change})
    # a NULL table, below the binding (which insists on a [K, 2] array)
    import ctypes as Cc
    x = torch.empty_like(y)
    rc = engine.lib.cd_ilvr_decode(engine.h, toy, sch.kind, _ffi.ptr(z), 1, 0, 2, K, Cc.c_void_p(coef.ctypes.data), None,
                                   Cc.c_uint64(0), _ffi.ptr(y), 2, 4, 0, None, None, Cc.c_uint64(0), _ffi.ptr(x))
    assert rc != 0 and b"q-sample" in engine.lib.cd_last_error()
    # a network with a text context
    txt = engine.create_net(tiny_sd_desc())
    zt, yt = _rnd((1, 1, 4, 16, 16), 44), _rnd((1, 4, 16, 16), 45)
    with pytest.raises(_ffi.EngineError, match="text context"):
        engine.ilvr_decode(txt, sch.kind, zt, coef, yt, 4, q)
    with pytest.raises(_ffi.EngineError, match="divide"):
        engine.op_lowpass(y, 5)
    assert torch.isfinite(engine.ilvr_decode(**good)).all()


# ------------------------------------------------------------------------------------------------ 7. driver
def test_main_runs_the_toy_ilvr_config(tmp_path, monkeypatch):
    from PIL import Image
    monkeypatch.setenv("CYCLEDIFF_SYNTHETIC_WEIGHTS", "1")
    rng = np.random.RandomState(7)
    Image.fromarray(rng.randint(0, 255, (8, 8, 3), dtype=np.uint8)).resize((32, 32), Image.BICUBIC).save(tmp_path / "im.png")
    (tmp_path / "data.json").write_text(json.dumps([{"img_path": "im.png"}]))
    sys.path.insert(0, ROOT)
    import main as driver
    out = tmp_path / "out"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert driver.main(["--cfg", "experiments/toy_ddpm_c1_ilvr.cfg", "--data", str(tmp_path / "data.json"), "--output_dir",
                            str(out), "--per_device_eval_batch_size", "1", "--synthetic-weights"]) == 0
    m = json.loads((out / "metrics.json").read_text())
    assert len(m["samples"]) == 1 and np.isfinite(m["summary"]["psnr"])
    assert (out / "000000.png").exists()


def test_factory_builds_the_afhq_config(monkeypatch):
    from cycle_diffusion_amd.gan_wrapper import baselines
    from cycle_diffusion_amd.gan_wrapper.get_gan_wrapper import get_gan_wrapper
    from cycle_diffusion_amd.utils.config_utils import get_config
    monkeypatch.setenv("CYCLEDIFF_SYNTHETIC_WEIGHTS", "1")
    args = get_config(os.path.join(ROOT, "config", "experiments", "bench_afhq_c5_ilvr.cfg"))
    gan = dict(list(args.gan))
    gan["source_model_path"] = gan["target_model_path"] = None  # no checkpoints in this tree: seeded synthetic weights

    class Args:
        gan_type = "DDPM_ILVR"

        def __iter__(self):
            return iter(gan.items())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w = get_gan_wrapper(Args(), target=True)
    assert isinstance(w, baselines.DDPMILVRWrapper) and (w.ilvr_down_n, w.ilvr_range_t, w.resolution) == (32, 20, 256)
    assert w.es_steps == 850 and len(w.sched.coef_ilvr()) == 850 and not hasattr(w, "translate")
