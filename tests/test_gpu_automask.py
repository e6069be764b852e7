"""The keep-mask estimate on the engine (include/cyclediff.h cd_automask / cd_op_automask_reduce, csrc/automask.hip; wrapper
`[gan] auto_mask = diffedit`): the reduction against the float64 definition within the derived bounds of
tests/_automask_ref.py, and bit for bit wherever two paths do the same fp32 arithmetic - chunked forwards, the composition
from cd_unet_forward, the generator's draws, and the wrapper's auto-masked call against the explicit-mask call."""
import ctypes as C

import pytest
import torch

import _automask_ref as ar
import golden_util as gu
from cycle_diffusion_amd import _ffi, auto_mask, schedule
from cycle_diffusion_amd._ffi import ptr
from test_gpu_models import _load, tiny_sd_desc

pytestmark = pytest.mark.gpu

FP16_BUILD = _ffi.load_library().cd_act_format() == 1
PRECS = [None, _ffi.CD_PREC_F32] + ([_ffi.CD_PREC_F32X3] if FP16_BUILD else [])
PREC_IDS = ["16bit", "fp32"] + (["fp32x3"] if FP16_BUILD else [])


def _setup(engine, prec=None):
    """the tiny SD network of tests/test_gpu_masked.py, its inputs (B = 2, C = 4, 16 x 16), and the level the wrapper would
    pick on a 12-step schedule at strength 0.5"""
    fx = gu.load("latent_cycle_tiny")
    d = tiny_sd_desc()
    if prec is not None:
        d.precision = prec
    net, _sd = _load(engine, d, fx)
    x0, c, _uc, c2 = (t.cuda() for t in gu.latent_cycle_inputs())
    sch = schedule.DDIMSchedule(schedule.latent_alphas_cumprod(), 12, 0.1)
    k = auto_mask.level_index(0.5, len(sch))
    qa, qb = (float(v) for v in sch.coef_qsample(0)[k])
    return net, x0, c, c2, int(sch.coef_decode(0)["t"][k]), qa, qb


def _noise(n, shape, seed=21):
    return torch.randn((n,) + tuple(shape), generator=torch.Generator().manual_seed(seed)).cuda()


# ------------------------------------------------------------------------------------------------ 1. the reduction
_CASES = {}


def _case(shape):
    """inputs of a shape, made once: the second sample's predictions are equal (its mean is 0)"""
    if shape not in _CASES:
        _CASES[shape] = ar.make_case(5, *shape, equal_sample=1 if shape[1] > 1 else None)
    return _CASES[shape]


@pytest.mark.parametrize("thr", [0.0, 0.5])
@pytest.mark.parametrize("d", [0, 1, 3])
@pytest.mark.parametrize("shape", ar.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reduce_against_float64(engine, shape, d, thr):
    n, B, Cc, H, W = shape
    es, et = _case(shape)
    ref = ar.reference64(es, et, 3.0, thr, d)
    keep, mp, mean = engine.op_automask_reduce(torch.from_numpy(es).cuda(), torch.from_numpy(et).cuda(), 3.0, thr, d)
    assert keep.shape == mp.shape == (B, 1, H, W)
    ar.compare(mp.cpu().numpy(), mean.cpu().numpy(), keep.cpu().numpy(), ref, n, Cc, thr, d,
               label="automask/reduce %s d=%d thr=%g" % (shape, d, thr))
    if B > 1:
        assert float(mean[1]) == 0.0 and bool((mp[1] == 0).all()) and bool((keep[1] == 1).all())


def test_reduce_without_vector_loads(engine):
    """HW = 35 is no multiple of 4: the accumulate kernel's scalar path (the case table's shapes all take 16-byte loads), with
    tiles of the finish kernel that hang over the image on both sides"""
    shape, d, thr = (2, 2, 3, 5, 7), 2, 0.5
    es, et = ar.make_case(6, *shape)
    keep, mp, mean = engine.op_automask_reduce(torch.from_numpy(es).cuda(), torch.from_numpy(et).cuda(), 3.0, thr, d)
    ar.compare(mp.cpu().numpy(), mean.cpu().numpy(), keep.cpu().numpy(), ar.reference64(es, et, 3.0, thr, d), 2, 3, thr, d,
               label="automask/reduce scalar %s" % (shape,))


def test_reduce_sample_alone_equals_the_sample_in_its_batch(engine):
    shape = (2, 3, 3, 8, 24)
    es, et = (torch.from_numpy(a).cuda() for a in _case(shape))
    keep, mp, mean = engine.op_automask_reduce(es, et, 3.0, 0.5, 1)
    for b in range(shape[1]):
        k1, m1, mean1 = engine.op_automask_reduce(es[:, b:b + 1].contiguous(), et[:, b:b + 1].contiguous(), 3.0, 0.5, 1)
        assert torch.equal(k1[0], keep[b]) and torch.equal(m1[0], mp[b]) and torch.equal(mean1[0], mean[b]), b


# ------------------------------------------------------------------------------------------------ 2. chunking
def test_chunked_forwards_give_the_same_bits(engine):
    net, x0, c, c2, t, qa, qb = _setup(engine)
    B = x0.shape[0]
    got = [engine.automask(net, x0, c, c2, t, qa, qb, n_draws=3, seed=7, max_rows=rows, dilate=1)
           for rows in (2 * B, 4 * B, 6 * B)]
    engine.synchronize()
    assert float(got[0][1].max()) > 0
    for keep, mp in got[1:]:
        print("automask/chunking map max abs diff %.3e" % (mp - got[0][1]).abs().max().item())
        assert torch.equal(mp, got[0][1]) and torch.equal(keep, got[0][0])


# ------------------------------------------------------------------------------------------------ 3. composition
@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
def test_entry_is_qsample_forward_and_reduction(engine, prec):
    net, x0, c, c2, t, qa, qb = _setup(engine, prec)
    n, B = 3, x0.shape[0]
    noise = _noise(n, x0.shape)
    keep, mp = engine.automask(net, x0, c, c2, t, qa, qb, n_draws=n, noise=noise, max_rows=2 * n * B, dilate=1)
    f = lambda v: torch.tensor(v, dtype=torch.float32, device="cuda")
    x = (f(qa) * x0)[None] + f(qb) * noise  # [n, B, C, H, W]: qa*x0, qb*n_i, then the add
    rows = x.reshape(n * B, *x0.shape[1:])
    eps = engine.unet_forward(net, torch.cat([rows, rows]).contiguous(), torch.full((2 * n * B,), float(t)).cuda(),
                              torch.cat([c.repeat(n, 1, 1), c2.repeat(n, 1, 1)]).contiguous())
    es, et = (e.reshape(n, B, *x0.shape[1:]).contiguous() for e in eps.chunk(2))
    keep2, mp2, _mean = engine.op_automask_reduce(es, et, 3.0, 0.5, 1)
    engine.synchronize()
    print("automask/composition map max abs diff %.3e" % (mp - mp2).abs().max().item())
    assert float(mp2.max()) > 0 and torch.equal(mp, mp2) and torch.equal(keep, keep2)


# ------------------------------------------------------------------------------------------------ 4. noise source
def test_generator_draws_are_the_streams_of_the_band(engine):
    net, x0, c, c2, t, qa, qb = _setup(engine)
    n, per = 3, x0.numel()
    noise = torch.stack([engine.gauss(11, ar.STREAM0 + i, per) for i in range(n)]).reshape((n,) + tuple(x0.shape))
    keep_n, mp_n = engine.automask(net, x0, c, c2, t, qa, qb, n_draws=n, noise=noise)
    keep_s, mp_s = engine.automask(net, x0, c, c2, t, qa, qb, n_draws=n, seed=11)
    _k, mp_o = engine.automask(net, x0, c, c2, t, qa, qb, n_draws=n, seed=12)
    engine.synchronize()
    assert torch.equal(mp_n, mp_s) and torch.equal(keep_n, keep_s)
    assert not torch.equal(mp_o, mp_s)


# ------------------------------------------------------------------------------------------------ 5. prompts
def test_the_map_comes_from_the_prompts(engine):
    net, x0, c, c2, t, qa, qb = _setup(engine)
    keep, mp = engine.automask(net, x0, c, c, t, qa, qb, n_draws=2, seed=3, thr=0.0, dilate=2)
    engine.synchronize()
    assert bool((mp == 0).all()) and bool((keep == 1).all())
    c3 = torch.randn(c.shape, generator=torch.Generator().manual_seed(9)).cuda()
    _k2, mp2 = engine.automask(net, x0, c, c2, t, qa, qb, n_draws=2, seed=3)
    _k3, mp3 = engine.automask(net, x0, c, c3, t, qa, qb, n_draws=2, seed=3)
    engine.synchronize()
    assert float(mp2.max()) > 0 and float(mp3.max()) > 0 and not torch.equal(mp2, mp3)


# ------------------------------------------------------------------------------------------------ 6. wrapper
SRC, TGT = ["a photo of a cat", "a red car"], ["a photo of a dog", "a blue car"]


def _pair(**kw):
    """a wrapper with the key and its twin without, on the same weights and embeddings"""
    from test_gpu_wrappers import FixedEmbedder, _make
    emb = FixedEmbedder()
    common = dict(n_trials=1, skip_steps=[0], decoder_unconditional_guidance_scales=[3.0], cond_stage=emb)
    common.update(kw)
    auto = _make(True, auto_mask="diffedit", auto_mask_draws=3, auto_mask_threshold=0.6, auto_mask_dilate=1,
                 auto_mask_seed=5, **common)[0]
    return auto, _make(True, **common)[0]


def _image():
    return torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(5)).cuda()


def _pixel_mask(w):
    m = w.last_auto_mask
    assert tuple(m.shape) == (2, 1, 16, 16) and bool(((m == 0) | (m == 1)).all())
    assert tuple(w.last_auto_map.shape) == (2, 1, 16, 16) and float(w.last_auto_map.max()) > 0
    print("automask/wrapper edit fraction %s" % (1 - m.mean((1, 2, 3))).tolist())
    assert 0 < float(m.mean()) < 1  # neither everything nor nothing: the two calls below differ from the unmasked one
    return m.repeat_interleave(w.vae_factor, 2).repeat_interleave(w.vae_factor, 3)


@pytest.mark.parametrize("kw", [dict(mask_source="q_sample"), dict(mask_source="encoder"), dict(mask_source="q_sample", cac_steps=0.4)],
                         ids=["q_sample", "encoder", "q_sample_cac"])
def test_auto_masked_translate_is_the_explicit_mask_call(kw):
    auto, plain = _pair(**kw)
    image = _image()
    with torch.no_grad():
        torch.manual_seed(11)
        got = auto.translate(image, SRC, TGT)
        assert auto.last_translate_coupled
        M = _pixel_mask(auto)
        torch.manual_seed(11)
        want = plain.translate(image, SRC, TGT, mask=M)
        torch.manual_seed(11)
        unmasked = plain.translate(image, SRC, TGT)
    assert torch.equal(got, want), (got - want).abs().max().item()
    assert not torch.equal(got, unmasked)
    assert plain.last_auto_mask is None


def test_auto_masked_forward_is_the_explicit_mask_call():
    auto, plain = _pair()
    image = _image()
    with torch.no_grad():
        torch.manual_seed(12)
        got = auto(auto.encode(image, SRC), image, SRC, TGT)
        M = _pixel_mask(auto)
        torch.manual_seed(12)
        want = plain(plain.encode(image, SRC), image, SRC, TGT, mask=M)
    assert torch.equal(got, want), (got - want).abs().max().item()


def test_an_explicit_mask_overrides_the_key():
    from cycle_diffusion_amd.gan_wrapper.latent_text_wrapper import LatentMask
    auto, plain = _pair()
    image = _image()
    M = torch.zeros(2, 1, 64, 64)
    M[:, :, 8:40, 16:56] = 1.0
    with torch.no_grad():
        torch.manual_seed(13)
        got = auto.translate(image, SRC, TGT, mask=M)
        assert auto.last_auto_mask is None  # nothing was estimated
        torch.manual_seed(13)
        want = plain.translate(image, SRC, TGT, mask=M)
        torch.manual_seed(13)
        latent = plain.translate(image, SRC, TGT, mask=LatentMask(torch.nn.functional.avg_pool2d(M, 4)))
    assert torch.equal(got, want) and torch.equal(latent, want)
    # auto_mask() itself answers whatever the key says
    keep, mp = plain.auto_mask(torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(1)).cuda(), SRC, TGT)
    assert tuple(keep.shape) == tuple(mp.shape) == (2, 1, 16, 16)


# ------------------------------------------------------------------------------------------------ driver
def test_main_writes_the_auto_mask_metrics_and_masks(tmp_path, monkeypatch):
    import json
    import os
    import sys
    import warnings
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.setenv("CYCLEDIFF_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.delenv("CYCLEDIFF_CLIP_RANKER", raising=False)
    import numpy as np
    rng = np.random.RandomState(7)
    Image.fromarray(rng.randint(0, 255, (64, 64, 3), dtype=np.uint8)).resize((512, 512), Image.BICUBIC).save(tmp_path / "im.png")
    row = {"img_path": "im.png", "encode_text": "a cat", "decode_text": "a dog"}
    (tmp_path / "data.json").write_text(json.dumps([row, row]))
    base = open(os.path.join(root, "config", "experiments", "bench_sd_c2.cfg")).read()
    base = base.replace("custom_steps = 99", "custom_steps = 4").replace("white_box_steps = 100", "white_box_steps = 5")
    (tmp_path / "on.cfg").write_text(base + "\nauto_mask = diffedit\nauto_mask_draws = 2\nmask_source = encoder\n")
    sys.path.insert(0, root)
    import main as driver
    out = tmp_path / "on"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert driver.main(["--cfg", str(tmp_path / "on.cfg"), "--data", str(tmp_path / "data.json"), "--output_dir", str(out),
                            "--per_device_eval_batch_size", "2", "--synthetic-weights", "--save_masks"]) == 0
    on = json.loads((out / "metrics.json").read_text())
    # what a run without the key writes (tests/test_gpu_masked.py holds the driver to it), and the three new entries
    plain, new = {"psnr", "ssim", "l2"}, {"psnr_keep", "psnr_edit", "edit_fraction"}
    assert plain | {"edit_fraction"} <= set(on["summary"]) <= plain | new
    for r in on["samples"]:
        assert {"sample_id", "encode_text", "decode_text", "edit_fraction"} | plain <= set(r) <= \
            {"sample_id", "encode_text", "decode_text"} | plain | new
        m = np.asarray(Image.open(out / ("%06d_mask.png" % r["sample_id"])))
        assert m.shape == (512, 512) and set(np.unique(m)) <= {0, 255}
        assert abs(float((m == 0).mean()) - r["edit_fraction"]) < 1e-6
        for k, some in (("psnr_keep", r["edit_fraction"] < 1.0), ("psnr_edit", r["edit_fraction"] > 0.0)):
            assert (k in r) == some and (not some or np.isfinite(r[k]))
    assert on["summary"]["edit_fraction"] == sum(r["edit_fraction"] for r in on["samples"]) / len(on["samples"])


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_name_the_parameter_and_launch_nothing(engine):
    import cycle_diffusion_amd as cda
    net, x0, c, c2, t, qa, qb = _setup(engine)
    B = x0.shape[0]
    lib, h = engine.lib, engine.h
    keep = torch.full((B, 1, 16, 16), -7.0).cuda()
    es = torch.zeros(2, B, 4, 16, 16).cuda()

    def entry(net_id=net, n=2, ratio=3.0, thr=0.5, dilate=0, max_rows=4 * B):
        return lib.cd_automask(h, net_id, ptr(x0), ptr(c), ptr(c2), c.shape[1], B, n, t, C.c_float(qa), C.c_float(qb), None,
                               C.c_uint64(0), max_rows, C.c_float(ratio), C.c_float(thr), dilate, None, ptr(keep))

    def reduce_(n=2, ratio=3.0, thr=0.5, dilate=0):
        return lib.cd_op_automask_reduce(h, ptr(es), ptr(es), n, B, 4, 16, 16, C.c_float(ratio), C.c_float(thr), dilate, None,
                                         None, ptr(keep))

    err = lambda: lib.cd_last_error().decode()
    ho = engine.create_net(cda.ho_ddpm_desc(32, 32, (1, 2, 2), 1, (16,)))  # a pixel network
    assert entry(net_id=ho) != 0 and "text context" in err()
    for call in (entry, reduce_):
        for kw, word in ((dict(n=0), "n_draws"), (dict(n=4096), "n_draws"), (dict(ratio=0.0), "ratio"),
                         (dict(ratio=-1.0), "ratio"), (dict(thr=1.0), "thr"), (dict(thr=-0.1), "thr"),
                         (dict(dilate=9), "dilate"), (dict(dilate=-1), "dilate")):
            assert call(**kw) != 0 and word in err(), (call.__name__, kw, err())
    assert entry(max_rows=2 * B - 1) != 0 and "max_rows" in err()
    torch.cuda.synchronize()
    assert bool((keep == -7.0).all())  # nothing ran
    # the engine is usable after the refusals
    assert entry() == 0 and reduce_() == 0
    engine.synchronize()
    assert bool(((keep == 0) | (keep == 1)).all())
    # the wrappers without a keep-mask refuse the key by name, before they touch the engine
    from cycle_diffusion_amd.gan_wrapper import baselines
    from cycle_diffusion_amd.gan_wrapper.ddpm_ddim_wrapper import DDPMDDIMWrapper
    with pytest.raises(ValueError, match="auto_mask"):
        baselines.SDSDEditTextWrapper("none", 12, 0.1, [0.5], auto_mask="diffedit")
    with pytest.raises(ValueError, match="auto_mask"):
        baselines.LatentDiffDDIBTextWrapper("none", 12, auto_mask="diffedit")
    with pytest.raises(ValueError, match="auto_mask"):
        DDPMDDIMWrapper("none", "ddim", 10, 10, auto_mask="diffedit")
