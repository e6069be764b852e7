"""The counter-based Gaussian generator (csrc/gauss.h, Philox4x32-10 + Box-Muller) and every noise = NULL path that draws from
it. cd_op_gauss (Engine.gauss) lays the raw draws bare:

  * against the float64 restatement of tests/_philox_ref.py: the rounds, the key schedule, the counter layout up to 64-bit
    element indices, the 24-bit uniforms and the Box-Muller pairing - any structural error moves a draw by order 1, the fast
    intrinsics (__logf, __sinf, __cosf) by TOL at most;
  * range, moments, correlations and the Kolmogorov-Smirnov distance of what the kernel produced, on the host test's bounds;
  * every consumer bit for bit: a noise = NULL call equals the same call on tensors filled by Engine.gauss with the stream
    tests/_philox_ref.py STREAMS states for that draw - the element index each kernel feeds to draw() and the stream each loop
    iteration uses;
  * a loop that would leave its 4096-stream band is refused."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import _ops
import _philox_ref as pr
import golden_util as gu
from cycle_diffusion_amd import _ffi, engine as cde, schedule
from cycle_diffusion_amd._ffi import ptr

pytestmark = pytest.mark.gpu

DDIM, DDPM = _ffi.CD_SCHED_DDIM, _ffi.CD_SCHED_DDPM

# max |device draw - float64 Box-Muller of the same uniforms| measured on MI355X over every case of
# test_draws_against_the_restatement (3 x 2^22 draws and the edge cases); the bound is 4 x that, for inputs other than the ones
# measured, and may not exceed 1e-3 (a structural error is of order 1)
MEASURED_MAX_DEV = 1.9416e-6  # seed 7, stream 0x1001; the other cases 0.6e-6 .. 1.9e-6
TOL = 4.0 * MEASURED_MAX_DEV
assert TOL <= 1e-3

BIG_SEED = 0x9E3779B97F4A7C15
# (seed, stream, first, n): the three statistics sequences (2^22 elements: above the 2048 x 256 threads a launch is capped at,
# so the grid-stride loop wraps); a seed with a non-zero high word; the last stream; an odd first element (the pair of the first
# draw starts one element earlier); n no multiple of the 256-thread block, one block and a ragged second one
DRAW_CASES = [(s, st, 0, pr.STAT_N) for s, st in pr.STAT_CASES] + [
    (BIG_SEED, 0x1000, 0, 70001),
    (7, 0xFFFFFFFF, 0, 4099),
    (7, 0x2001, 12345, 4099),
    (BIG_SEED, 0x4000, 7, 315),
]


def _dev(engine, seed, stream, first, n):
    got = engine.gauss(seed, stream, n, first=first).cpu().numpy()
    ref = pr.normals_range(seed, stream, first, n)
    return got, float(np.abs(got.astype(np.float64) - ref).max())


# ------------------------------------------------------------------------------------------------ 1. the generator
@pytest.mark.parametrize("seed,stream,first,n", DRAW_CASES,
                         ids=["s7_0x1000", "s7_0x1001", "s8_0x1000", "seed_high_word", "last_stream", "odd_first", "ragged"])
def test_draws_against_the_restatement(engine, report, seed, stream, first, n):
    got, dev = _dev(engine, seed, stream, first, n)
    print("gauss seed=%#x stream=%#x first=%d n=%d: max |device - float64| = %.4e" % (seed, stream, first, n, dev))
    report.add("philox/draws_%x_%x_%d_%d" % (seed, stream, first, n), max_abs_dev=dev)
    assert got.dtype == np.float32 and got.shape == (n,) and np.isfinite(got).all()
    assert dev <= TOL, dev


@pytest.mark.parametrize("first", [(1 << 32) - 4, (1 << 33) - 4, (1 << 34) + 1], ids=["2^32-4", "2^33-4", "2^34+1"])
def test_draws_at_64_bit_element_indices(engine, first):
    """16 elements across the wrap of counter word 0 (element 2^33) and into word 1; 2^32 is where a 32-bit index would wrap"""
    got, dev = _dev(engine, BIG_SEED, 0x5003, first, 16)
    print("gauss first=%d: max |device - float64| = %.4e" % (first, dev))
    assert dev <= TOL, dev
    # the case can tell: with the index cut to 32 or to 33 bits the restatement itself gives other numbers
    idx = np.arange(first, first + 16, dtype=np.uint64)
    ref = pr.normals_range(BIG_SEED, 0x5003, first, 16)
    for bits in (32, 33):
        if first + 15 >= 1 << bits:
            assert np.abs(ref - pr.normals(BIG_SEED, 0x5003, idx % np.uint64(1 << bits))).max() > 0.1, bits


def test_range_of_2_to_the_24_draws(engine, report):
    """every draw is finite and |z| <= sqrt(50 ln 2) = 5.887 (u1 >= 2^-25) + TOL, over 2^24 draws - 2^23 counters, so the
    extreme 24-bit uniforms (u1 = 1.0, radius 0; u1 = 2^-25, the largest radius) are likely to occur"""
    chunk, worst = 1 << 22, 0.0
    for j in range(4):
        z = engine.gauss(7, 0x1000, chunk, first=j * chunk)
        assert bool(torch.isfinite(z).all())
        worst = max(worst, float(z.abs().max()))
    print("max |z| over 2^24 draws: %.6f (bound %.6f)" % (worst, pr.MAX_ABS))
    report.add("philox/range", max_abs=worst, bound=pr.MAX_ABS)
    assert worst <= pr.MAX_ABS + TOL, worst
    assert worst > 4.5  # P(max of 2^24 normals < 4.5) = exp(-2^24 * 6.8e-6) ~ 1e-50: the tail is there


def test_statistics_of_the_device_draws(engine, report):
    """the host test's moment, correlation and KS checks on what the kernel produced, on the same bounds"""
    seqs = [engine.gauss(s, st, pr.STAT_N).cpu().numpy().astype(np.float64) for s, st in pr.STAT_CASES]
    stats, ks = pr.statistics(*seqs)
    dev = pr.check_statistics(stats, ks, "device")
    report.add("philox/statistics", worst_sigmas=float(max(abs(d) for d in dev.values())), ks_sqrt_n=float(max(ks.values())))


# ------------------------------------------------------------------------------------------------ 2. the step kernels
def _g(engine, seed, loop, it, shape):
    return engine.gauss(seed, pr.STREAMS(loop, it), int(np.prod(shape))).view(*shape)


@pytest.mark.parametrize("shape", [(3, 3, 5, 7), (2, 4, 256, 260)], ids=["odd_315", "grid_stride_wrap"])
def test_step_kernels_draw_element_i_of_stream_0(engine, shape):
    """cd_op_sched_step with noise = NULL (seed 0, stream 0) against the same launch on gauss(0, 0, n): k_init_xt,
    k_encode_step_ddim / _ddpm, and the decode steps without an injected eps (sigma != 0). An odd shape, and one whose element
    count exceeds the launch's thread cap."""
    from test_gpu_ops import _coef
    g = torch.Generator().manual_seed(53)
    x0, xt, e = [torch.randn(*shape, generator=g) for _ in range(3)]
    nz = engine.gauss(0, 0, x0.numel()).view(*shape).cpu()
    assert nz.abs().max() > 2.0
    ddim_row = _coef(0.4321, 0.4876, 0.0123)
    sch = schedule.PixelSchedule(20, 20, sample_type="ddpm", eta=None)
    enc_row, dec_row = tuple(sch.coef_encode()[9]), tuple(sch.coef_decode()[10])
    calls = [("init", dict(mode=0, kind=DDIM, coef_row=ddim_row, x0=x0)),
             ("encode_ddim", dict(mode=1, kind=DDIM, coef_row=ddim_row, x0=x0, xt=xt, eps_hat=e)),
             ("encode_ddpm", dict(mode=1, kind=DDPM, coef_row=enc_row, x0=x0, xt=xt, eps_hat=e)),
             ("decode_ddim", dict(mode=2, kind=DDIM, coef_row=ddim_row, xt=xt, eps_hat=e)),
             ("decode_ddpm", dict(mode=2, kind=DDPM, coef_row=dec_row, xt=xt, eps_hat=e))]
    for name, kw in calls:
        x_none, z_none = _ops.sched_step(engine, noise=None, **kw)
        x_expl, z_expl = _ops.sched_step(engine, noise=nz, **kw)
        x_zero, _ = _ops.sched_step(engine, noise=torch.zeros(*shape), **kw)
        assert torch.isfinite(x_none).all(), name
        assert torch.equal(x_none, x_expl) and torch.equal(z_none, z_expl), (name, (x_none - x_expl).abs().max().item())
        assert (x_none - x_zero).abs().max() > 1e-3, name  # the draw is really in the result


# ------------------------------------------------------------------------------------------------ 3. the pixel loops
@pytest.fixture(scope="module")
def toy(engine):
    """the toy Ho-DDPM in fp32 with the baselines fixture's tamed output layer, as tests/test_gpu_ilvr.py builds it"""
    import _baselines_ref as br
    fx = gu.load("baselines_pixel")
    p = json.loads(str(fx["params"]))
    net = engine.create_net(cde.ho_ddpm_desc(32, 32, (1, 2, 2), 1, (16,), precision=_ffi.CD_PREC_F32))
    sd = br.synth_weights(json.loads(str(fx["tgt_names"])), p["tgt_seed"], p["out_prefix"], p["out_scale"])
    assert engine.load_state_dict(net, sd)[0] == 0
    return net


PIX = (3, 3, 32, 32)  # an odd batch of the toy network's images


def _rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).cuda()


@pytest.mark.parametrize("st,eta", [("ddim", 0.1), ("ddpm", None)])
def test_dpm_encode_and_decode_tail_draw_their_streams(engine, toy, st, eta):
    """K = 3 encoder steps: z[:, 0] is stream 0 and slot 1 + i stream 1 + i; the 4-step decode with n_eps = 1 draws its three
    tail steps from 0x1000 + i with the LOOP's iteration i (1, 2, 3), not the index into the tail (0, 1, 2)"""
    seed, K = 0x1234567890, 3
    sch = schedule.PixelSchedule(50, K + 1, sample_type=st, eta=eta)
    ce, cd = sch.coef_encode(), sch.coef_decode()
    assert len(ce) == K + 1 and len(cd) == K + 1
    x0 = _rnd(PIX, 61).clamp(-1, 1)
    z = engine.dpm_encode(toy, sch.kind, x0, ce, noise=None, seed=seed, last_uses_x0=False)
    nz = torch.stack([_g(engine, seed, "encode_init", 0, PIX)] + [_g(engine, seed, "encode", i, PIX) for i in range(K)], 0)
    z_expl = engine.dpm_encode(toy, sch.kind, x0, ce, noise=nz, last_uses_x0=False)
    engine.synchronize()
    assert torch.isfinite(z).all()
    for slot in range(K + 1):
        assert torch.equal(z[:, slot], z_expl[:, slot]), (slot, (z[:, slot] - z_expl[:, slot]).abs().max().item())
    assert not torch.equal(z, engine.dpm_encode(toy, sch.kind, x0, ce, noise=None, seed=seed + 1, last_uses_x0=False))
    # the decode's tail
    n_eps = 1
    x = engine.ddim_decode(toy, sch.kind, z, cd, n_eps=n_eps, noise_tail=None, seed=seed)
    tail = torch.stack([_g(engine, seed, "decode", i, PIX) for i in range(n_eps, len(cd))], 0)
    x_expl = engine.ddim_decode(toy, sch.kind, z, cd, n_eps=n_eps, noise_tail=tail)
    wrong = torch.stack([_g(engine, seed, "decode", i - n_eps, PIX) for i in range(n_eps, len(cd))], 0)
    x_wrong = engine.ddim_decode(toy, sch.kind, z, cd, n_eps=n_eps, noise_tail=wrong)
    engine.synchronize()
    assert torch.isfinite(x).all()
    assert torch.equal(x, x_expl), (x - x_expl).abs().max().item()
    assert not torch.equal(x, x_wrong)


def test_pix_refine_draws_0x2000_then_0x2001_plus_i(engine, toy):
    seed, R = 99, 3
    sch = schedule.PixelSchedule(50, 50, sample_type="ddim", eta=0.1, refine_steps=R)
    coef = sch.coef_refine()
    assert len(coef) == R + 1
    x0 = _rnd(PIX, 62).clamp(-1, 1)
    x = engine.pix_refine(toy, sch.kind, x0, coef, noise=None, seed=seed)
    nz = torch.stack([_g(engine, seed, "refine_init", 0, PIX)] + [_g(engine, seed, "refine", i, PIX) for i in range(R)], 0)
    x_expl = engine.pix_refine(toy, sch.kind, x0, coef, noise=nz)
    engine.synchronize()
    assert torch.isfinite(x).all() and (x - x0).abs().max() > 1e-2
    assert torch.equal(x, x_expl), (x - x_expl).abs().max().item()


@pytest.mark.parametrize("path", ["vec4", "scalar"])
def test_ilvr_reference_draws_0x5000_plus_i(engine, toy, path):
    """ref_noise = NULL against ref_noise from 0x5000 + i, through form_d4 (16-byte path: R % 4 == 0 and aligned tensors) and
    through the scalar form_d. Every Ho-DDPM's resolution is a multiple of 8 (its mid attention takes token counts that are
    multiples of 32), so the scalar path is reached the way cd_ilvr_decode itself reaches it: a reference image that is not
    16-byte aligned."""
    seed, ref_seed, K, N = 5, 0xABCDEF0123, 3, 4
    sch = schedule.PixelSchedule(50, K, sample_type="ddim", eta=0.1)
    coef, q = sch.coef_decode(), sch.coef_ilvr()
    assert (q[1:, 1] != 0).all()  # the conditioned rows do draw
    z = _rnd((PIX[0], 1) + PIX[1:], 63)
    y = _rnd(PIX, 64).clamp(-1, 1)
    if path == "scalar":
        flat = torch.zeros(y.numel() + 1, device="cuda")
        flat[1:] = y.flatten()
        y = flat[1:].view(*PIX)
        assert y.data_ptr() % 16 == 4 and y.is_contiguous()
    else:
        assert y.data_ptr() % 16 == 0
    nt = _rnd((K,) + PIX, 65)
    x = engine.ilvr_decode(toy, sch.kind, z, coef, y, N, q, range_t=0, noise_tail=nt, ref_noise=None, ref_seed=ref_seed)
    rn = torch.stack([_g(engine, ref_seed, "ilvr", i, PIX) for i in range(K)], 0)
    x_expl = engine.ilvr_decode(toy, sch.kind, z, coef, y, N, q, range_t=0, noise_tail=nt, ref_noise=rn)
    x_off = engine.ilvr_decode(toy, sch.kind, z, coef, y, N, q, range_t=0, noise_tail=nt, ref_noise=rn.roll(1, dims=-1))
    # both generators at once: the step's own draws come from 0x1000 + i of `seed`
    x_both = engine.ilvr_decode(toy, sch.kind, z, coef, y, N, q, range_t=0, n_eps=0, noise_tail=None, seed=seed, ref_noise=None,
                                ref_seed=ref_seed)
    nt2 = torch.stack([_g(engine, seed, "decode", i, PIX) for i in range(K)], 0)
    x_both_expl = engine.ilvr_decode(toy, sch.kind, z, coef, y, N, q, range_t=0, noise_tail=nt2, ref_noise=rn)
    engine.synchronize()
    assert torch.isfinite(x).all()
    assert torch.equal(x, x_expl), (x - x_expl).abs().max().item()
    assert not torch.equal(x, x_off)
    assert torch.equal(x_both, x_both_expl), (x_both - x_both_expl).abs().max().item()


# ------------------------------------------------------------------------------------------------ 4. the latent loops
def test_coupled_loop_with_one_seed_equals_the_two_calls(engine):
    """cycle_translate(noise = NULL, seed) against dpm_encode and ddim_decode with the same seed, and against the coupled loop
    on the explicit encoder draws"""
    from test_gpu_masked import _setup
    net, x0, c, uc, c2, sch, K, _noise = _setup(engine, S=4)
    seed = 77
    ce, cd = sch.coef_encode(0), sch.coef_decode(0)
    kw = dict(enc_ctx_c=c, enc_ctx_uc=uc, dec_ctx_c=c2, dec_ctx_uc=uc, dec_guidance=3.0)
    z, x = engine.cycle_translate(net, DDIM, x0, ce, cd, noise=None, seed=seed, last_uses_x0=False, **kw)
    z_ref = engine.dpm_encode(net, DDIM, x0, ce, ctx_c=c, ctx_uc=uc, guidance=1.0, noise=None, seed=seed, last_uses_x0=False)
    x_ref = engine.ddim_decode(net, DDIM, z_ref, cd, ctx_c=c2, ctx_uc=uc, guidance=3.0, seed=seed)
    shape = tuple(x0.shape)
    nz = torch.stack([_g(engine, seed, "encode_init", 0, shape)] + [_g(engine, seed, "encode", i, shape) for i in range(K)], 0)
    z_expl, x_expl = engine.cycle_translate(net, DDIM, x0, ce, cd, noise=nz, last_uses_x0=False, **kw)
    engine.synchronize()
    assert torch.isfinite(x).all()
    assert torch.equal(z, z_ref) and torch.equal(x, x_ref), (x - x_ref).abs().max().item()
    assert torch.equal(z, z_expl) and torch.equal(x, x_expl), (z - z_expl).abs().max().item()


@pytest.mark.parametrize("rep", [1, 2], ids=["B_mask=B", "B_mask<B"])
def test_masked_decode_draws_0x4000_plus_slot(engine, rep):
    """q_sample mode with mask_noise = NULL against mask_noise from 0x4000 + slot (slot 0: the blend ahead of the first
    forward). With B_mask < B the draw takes the full-batch element index while mask and x0 take row b % B_mask."""
    from test_gpu_masked import _masks, _setup
    net, x0, c, uc, c2, sch, K, noise = _setup(engine, S=4)
    mask_seed = 0x600DF00D5
    Bm = x0.shape[0]
    B = rep * Bm
    cd, q = sch.coef_decode(0), sch.coef_qsample(0)
    z = engine.dpm_encode(net, DDIM, x0, sch.coef_encode(0), ctx_c=c, ctx_uc=uc, guidance=1.0, noise=noise)
    z = z.repeat(rep, 1, 1, 1, 1).contiguous()
    ct, ucd = c2.repeat(rep, 1, 1), uc.repeat(rep, 1, 1)
    mask = _masks(Bm).cuda()
    kw = dict(ctx_c=ct, ctx_uc=ucd, guidance=3.0)
    x = engine.ddim_decode_masked(net, DDIM, z, cd, mask, x0, q, mask_noise=None, mask_seed=mask_seed, **kw)
    shape = (B,) + tuple(x0.shape[1:])
    mn = torch.stack([_g(engine, mask_seed, "mask", slot, shape) for slot in range(K)], 0)
    x_expl = engine.ddim_decode_masked(net, DDIM, z, cd, mask, x0, q, mask_noise=mn, **kw)
    engine.synchronize()
    assert torch.isfinite(x).all()
    assert torch.equal(x, x_expl), (x - x_expl).abs().max().item()
    if rep == 2:  # the two copies of a sample took different draws
        assert (x[:Bm] - x[Bm:]).abs().max() > 1e-3


def test_vae_posterior_draws_0x7a65(engine):
    """vae_encode(noise = NULL, seed) against noise = gauss(seed, 0x7a65): k_posterior_sample's flat index, and the only check
    that the generator's copy in csrc/elementwise.hip agrees with csrc/gauss.h"""
    from test_gpu_models import _load, tiny_vae_desc
    net, _sd = _load(engine, tiny_vae_desc(), gu.load("vae_tiny"))
    seed = 0xFEDCBA9876
    img = (torch.rand((3, 3, 64, 64), generator=torch.Generator().manual_seed(4)) * 2 - 1).cuda()
    z = engine.vae_encode(net, img, noise=None, seed=seed, sample=True)
    nz = _g(engine, seed, "vae", 0, tuple(z.shape))
    z_expl = engine.vae_encode(net, img, noise=nz, sample=True)
    z_mean = engine.vae_encode(net, img, sample=False)
    engine.synchronize()
    assert torch.isfinite(z).all() and (z - z_mean).abs().max() > 1e-4
    assert torch.equal(z, z_expl), (z - z_expl).abs().max().item()


# ------------------------------------------------------------------------------------------------ 5. the band's end
def test_a_loop_that_leaves_its_stream_band_is_refused(engine, toy):
    """4096 steps with noise = NULL would draw step 4095 from the next loop's first stream: refused ahead of any launch, with
    the limit in the message. The same call with a noise tensor passes that check - and is stopped here by a later refusal
    (a context the toy network cannot take, range_t < 0, a keep-mask on a pixel network, an unknown network), never run."""
    K = pr.MAX_STEPS + 1
    lib, h = engine.lib, engine.h
    coef = np.zeros(K + 1, dtype=_ffi.STEP_COEF_DTYPE)
    cp = C.c_void_p(coef.ctypes.data)
    qtab = np.zeros((K, 2), dtype=np.float32)
    qp = C.c_void_p(qtab.ctypes.data)
    B = 1
    buf = torch.zeros(4 * 3 * 32 * 32, device="cuda")  # stands for every tensor: no call below reaches a launch
    p = ptr(buf)
    err = lambda: lib.cd_last_error().decode()
    f1, u0 = C.c_float(1.0), C.c_uint64(0)

    def refused_for_the_band(rc, what):
        msg = err()
        assert rc != 0 and "stream band" in msg and str(pr.MAX_STEPS) in msg and what in msg, msg

    def past_the_band(rc, text):
        msg = err()
        assert rc != 0 and "stream band" not in msg and text in msg, msg

    # cd_dpm_encode
    enc = lambda nz, ctx: lib.cd_dpm_encode(h, toy, DDIM, p, ctx, None, 1, f1, B, K, cp, nz, u0, 0, p)
    refused_for_the_band(enc(None, None), "noise")
    past_the_band(enc(p, p), "cross-attention")
    # cd_ddim_decode
    dec = lambda nz, ctx: lib.cd_ddim_decode(h, toy, DDIM, p, 1, 0, ctx, None, 1, f1, B, K, cp, nz, u0, p)
    refused_for_the_band(dec(None, None), "noise_tail")
    past_the_band(dec(p, p), "cross-attention")
    # cd_ddim_decode_masked, q_sample mode: the step noise and the mask noise each
    mdec = lambda nz, mnz: lib.cd_ddim_decode_masked(h, toy, DDIM, p, 1, 0, None, None, 0, f1, None, B, K, cp, nz, u0, p, p, 1,
                                                     _ffi.CD_MASK_QSAMPLE, qp, mnz, u0, p)
    refused_for_the_band(mdec(None, p), "noise_tail")
    refused_for_the_band(mdec(p, None), "mask_noise")
    past_the_band(mdec(p, p), "pixel")
    # cd_cycle_translate
    cyc = lambda nz, ctx: lib.cd_cycle_translate(h, C.byref(_ffi.TranslateArgs(
        size=C.sizeof(_ffi.TranslateArgs), net=toy, sched_kind=DDIM, x0=p, enc_ctx_c=ctx, enc_guidance=1.0, dec_guidance=1.0,
        ctx_len=1, B=B, n_dec=1, K=K, coef_enc_host=cp, coef_dec_host=cp, noise=nz, seed=0, last_uses_x0=0, z_out=p, x_out=p)))
    refused_for_the_band(cyc(None, None), "noise")
    past_the_band(cyc(p, p), "contexts for both passes")
    # cd_pix_refine: nothing later refuses a call on the toy network, so the pair runs on a network that does not exist
    ref = lambda net, nz: lib.cd_pix_refine(h, net, DDIM, p, B, K, cp, nz, u0)
    refused_for_the_band(ref(toy, None), "noise")
    refused_for_the_band(ref(-1, None), "noise")
    past_the_band(ref(-1, p), "bad net id")
    # cd_ilvr_decode: the step noise and the reference noise each
    ilvr = lambda nz, rnz, rt: lib.cd_ilvr_decode(h, toy, DDIM, p, 1, 0, B, K, cp, nz, u0, p, 1, 4, rt, qp, rnz, u0, p)
    refused_for_the_band(ilvr(None, p, 0), "noise_tail")
    refused_for_the_band(ilvr(p, None, 0), "ref_noise")
    past_the_band(ilvr(p, p, -1), "range_t")
    # 4095 steps are inside the band: the check lets the NULL call through to the later refusal
    assert lib.cd_ilvr_decode(h, toy, DDIM, p, 1, 0, B, K - 1, cp, None, u0, p, 1, 4, -1, qp, None, u0, p) != 0
    assert "range_t" in err()
    # the engine is usable after the refusals
    assert torch.isfinite(engine.gauss(1, 2, 8)).all()
