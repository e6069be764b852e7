"""Per-word cross-attention heat maps (include/cyclediff.h cd_word_maps / cd_op_cross_attention_maps; csrc/attn.hip
k_cross_attention_maps, csrc/automask.hip k_word_map_accumulate / k_word_map_fold).

  1. the kernel against float64 torch on 16-bit-rounded q / k, at the bound of tests/test_gpu_ops.py::test_attention
  2. identities of the kernel: bit for bit where no summation order differs, else at the bound of 1
  3. cd_word_maps on the tiny SD network: what must be bit-identical, what the forward must not notice, the layer counts
  4. end to end against the oracle restatement (tests/_word_maps_ref.py), at the tiny SD forward's bound
  5. refusals, each with its message
  6. the wrapper's word_maps() and the composition with blend_mask() and translate(mask=)
  7. main.py --word_maps
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _ops
import _word_maps_ref as wr
import golden_util as gu
from _ops import bf16_round as r16
from cycle_diffusion_amd import _ffi, attn_control
from cycle_diffusion_amd._ffi import ptr
from test_gpu_models import NET_REL, _load, tiny_sd_desc

pytestmark = pytest.mark.gpu

FMT = 1.0 if _ffi.load_library().cd_act_format() == 1 else 8.0
REL, MEAN = 4e-3 * FMT, 1.5e-3 * FMT  # tests/test_gpu_ops.py::test_attention
LOG2E = 1.44269504088896340736


def _check(report, name, got, ref, rel=REL, mean=MEAN):
    st = _ops.err_stats(got, ref.float())
    report.add("word_maps/" + name, **st)
    print("word_maps/%s %s" % (name, st))
    assert st["finite"], name
    assert st["rel_to_max"] < rel and (mean is None or st["mean_rel"] < mean), (name, st)


# ------------------------------------------------------------------------------------------------ 1. the kernel
# (B, B_sel, H, Tq, L, D, N): the modulo selector index; a strip shorter than the tile and the widest head; a ragged last strip
# and the most words; the tiny network's head dims at 16 x 16 and at 8 x 8; a short context
CASES = [(2, 1, 8, 256, 77, 40, 3), (1, 1, 8, 64, 77, 160, 1), (1, 1, 8, 320, 77, 80, 8), (2, 2, 2, 256, 77, 32, 2),
         (1, 1, 2, 64, 77, 64, 2), (1, 1, 1, 64, 33, 40, 1)]
CASE_IDS = ["b%d_s%d_h%d_t%d_l%d_d%d_n%d" % c for c in CASES]


def _operands(case, seed=53):
    B, Bs, H, Tq, L, D, N = case
    g = torch.Generator().manual_seed(seed)
    q, k = (r16(torch.randn(B, T, H * D, generator=g)) for T in (Tq, L))
    sel = torch.rand(Bs, N, L, generator=g) * (torch.rand(Bs, N, L, generator=g) < 0.3)  # fp32 weights, most of them 0
    return q, k, sel


def _run(engine, q, k, sel, H, **kw):
    m = engine.cross_attention_maps(_ops.dev(q), _ops.dev(k), _ops.dev(sel), H, **kw)
    torch.cuda.synchronize()
    return m.cpu()


@pytest.mark.parametrize("q_log2", [0, 1], ids=["scale", "q_log2"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_maps_kernel_vs_float64(engine, report, case, q_log2):
    B, Bs, H, Tq, L, D, N = case
    q, k, sel = _operands(case)
    scale = D ** -0.5
    if q_log2:
        q = r16(q * (scale * LOG2E))  # the form the networks' to_q emits; the reference takes the softmax in base 2 on it
    ref = wr.maps_ref64(q, k, sel, H, scale, log2=bool(q_log2))
    got = _run(engine, q, k, sel, H, scale=scale, q_log2=bool(q_log2))
    assert tuple(got.shape) == (B, N, Tq)
    _check(report, "op/%s/%s" % ("x".join(map(str, case)), "log2" if q_log2 else "scale"), got, ref)


# ------------------------------------------------------------------------------------------------ 2. identities
def test_every_key_selected_gives_one(engine, report):
    """sel = 1 on every key: the head mean of the row sums of P, 1 within the bound (the probabilities are not renormalised)"""
    case = (2, 1, 8, 320, 77, 40, 1)
    q, k, _ = _operands(case, seed=59)
    got = _run(engine, q, k, torch.ones(1, 1, 77), 8)
    _check(report, "ones", got, torch.ones_like(got))


def test_swapped_selector_rows_swap_the_outputs_bit_for_bit(engine):
    case = (2, 1, 8, 320, 77, 40, 2)
    q, k, _ = _operands(case, seed=61)
    sel = torch.zeros(1, 2, 77)
    sel[0, 0, 5], sel[0, 1, 40] = 1.0, 1.0
    a, b = _run(engine, q, k, sel, 8), _run(engine, q, k, sel.flip(1), 8)
    assert float(a.max()) > 0 and not torch.equal(a[:, 0], a[:, 1])
    assert torch.equal(a[:, 0], b[:, 1]) and torch.equal(a[:, 1], b[:, 0])


def test_spike_garbage_keys_and_repeatability(engine, report):
    """one score 30 above the rest (the maximum is subtracted: finite, in bound); rows L .. 95 of the caller's key buffer filled
    with large values change no bit; the same launch twice gives the same bits"""
    case = (2, 1, 8, 256, 77, 40, 3)
    B, Bs, H, Tq, L, D, N = case
    q, k, sel = _operands(case, seed=67)
    scale = D ** -0.5
    for h in range(H):
        d = q[0, 5, h * D:(h + 1) * D]
        k[0, 70, h * D:(h + 1) * D] = d / d.norm() ** 2 * 30.0 / scale
    k = r16(k)
    sel[0, 0, 70] = 1.0
    got = _run(engine, q, k, sel, H)
    _check(report, "spike", got, wr.maps_ref64(q, k, sel, H, scale))
    assert abs(float(got[0, 0, 5]) - 1.0) < REL  # nearly all of that query's mass
    pad = torch.cat([k, torch.full((B, 96 - L, H * D), 3.0e4)], 1)
    assert torch.equal(got, _run(engine, q, pad, sel, H, L=L))
    assert torch.equal(got, _run(engine, q, k, sel, H))


# ------------------------------------------------------------------------------------------------ 3. cd_word_maps
@pytest.fixture(scope="module")
def tiny(engine):
    """the tiny SD network on the shared end-to-end inputs, and the oracle's maps on them (made once, left unchanged)"""
    fx = gu.load("latent_cycle_tiny")
    net, sd = _load(engine, tiny_sd_desc(), fx)
    x0, c, noise, (t, qa, qb) = wr.e2e_inputs()
    sel = torch.cat([wr.one_key(j) for j in wr.E2E["keys"]], 1)  # [1, 2, L]
    ref = {sides: wr.word_maps_ref(sd, gu.TINY_SD_CFG, x0, c, sel, t, qa, qb, noise, sides) for sides in ((0, 0), (16, 16))}
    return dict(net=net, x0=x0.cuda(), c=c.cuda(), noise=noise.cuda(), sel=sel.cuda(), level=(t, qa, qb), ref=ref)


def test_samples_of_a_batch_equal_the_samples_alone(engine, tiny):
    t = tiny
    sel = torch.cat([t["sel"], t["sel"].flip(1)], 0)  # B_sel = 2: a selector per sample
    both, n = engine.word_maps(t["net"], t["x0"], t["c"], sel, *t["level"], n_draws=2, noise=t["noise"])
    assert n == sum(wr.TINY_SIDES.values()) and tuple(both.shape) == (2, 2, 16, 16) and float(both.min()) > 0
    for b in range(2):
        one, _ = engine.word_maps(t["net"], t["x0"][b:b + 1], t["c"][b:b + 1], sel[b:b + 1], *t["level"], n_draws=2,
                                  noise=t["noise"][:, b:b + 1].contiguous())
        assert torch.equal(one[0], both[b]), (b, (one[0] - both[b]).abs().max().item())
    # one selector entry for both samples: sample b uses entry b % B_sel
    shared, _ = engine.word_maps(t["net"], t["x0"], t["c"], t["sel"], *t["level"], n_draws=2, noise=t["noise"])
    assert torch.equal(shared[0], both[0]) and torch.equal(shared[1], both[1].flip(0))


def test_chunked_forwards_and_repeated_calls_give_the_same_bits(engine, tiny):
    t = tiny
    B = t["x0"].shape[0]
    got = [engine.word_maps(t["net"], t["x0"], t["c"], t["sel"], *t["level"], n_draws=3, seed=7, max_rows=rows)[0]
           for rows in (3 * B, B, 2 * B, 3 * B)]  # all draws in one forward; one per forward; two and one; the first again
    engine.synchronize()
    for m in got[1:]:
        assert torch.equal(m, got[0]), (m - got[0]).abs().max().item()


def test_generator_draws_are_the_streams_of_the_band(engine, tiny):
    import _philox_ref as pr
    t = tiny
    n, per = 3, t["x0"].numel()
    draws = [engine.gauss(11, wr.STREAM0 + i, per) for i in range(n)]
    # ... which are the reference generator's streams STREAM0 + i, element = the flat index in [B, C, h, w]
    for i in (0, n - 1):
        want = torch.from_numpy(pr.normals_range(11, wr.STREAM0 + i, 0, per).copy()).float()
        assert (draws[i].cpu() - want).abs().max() <= 1e-3
    noise = torch.stack(draws).reshape((n,) + tuple(t["x0"].shape))
    m_n, _ = engine.word_maps(t["net"], t["x0"], t["c"], t["sel"], *t["level"], n_draws=n, noise=noise)
    m_s, _ = engine.word_maps(t["net"], t["x0"], t["c"], t["sel"], *t["level"], n_draws=n, seed=11)
    m_o, _ = engine.word_maps(t["net"], t["x0"], t["c"], t["sel"], *t["level"], n_draws=n, seed=12)
    engine.synchronize()
    assert torch.equal(m_n, m_s) and not torch.equal(m_o, m_s)


def test_the_collection_leaves_the_forward_alone(engine, tiny):
    t = tiny
    tl, qa, qb = t["level"]
    f = lambda v: torch.tensor(v, dtype=torch.float32, device="cuda")
    rows = ((f(qa) * t["x0"])[None] + f(qb) * t["noise"]).reshape(-1, *t["x0"].shape[1:]).contiguous()
    tv, cx = torch.full((rows.shape[0],), float(tl)).cuda(), t["c"].repeat(2, 1, 1).contiguous()
    before = engine.unet_forward(t["net"], rows, tv, cx)
    engine.word_maps(t["net"], t["x0"], t["c"], t["sel"], *t["level"], n_draws=2, noise=t["noise"])
    after = engine.unet_forward(t["net"], rows, tv, cx)
    engine.synchronize()
    assert torch.isfinite(before).all() and torch.equal(before, after)


def test_side_windows_count_the_blocks_of_the_description(engine, tiny):
    t = tiny
    run = lambda sides: engine.word_maps(t["net"], t["x0"], t["c"], t["sel"], *t["level"], n_draws=1, seed=3, sides=sides)
    (m_all, n_all), (m16, n16), (m8, n8) = run((0, 0)), run((16, 16)), run((8, 8))
    assert (n_all, n16, n8) == (wr.TINY_SIDES[16] + wr.TINY_SIDES[8], wr.TINY_SIDES[16], wr.TINY_SIDES[8])
    assert run((8, 16))[1] == n_all and run((1, 8))[1] == n8
    # an 8 x 8 map is constant on 2 x 2 blocks of the latent; the mean over all layers is the weighted mean of the two windows
    assert torch.equal(m8, m8.reshape(2, 2, 8, 2, 8, 2)[:, :, :, :1, :, :1].expand(-1, -1, -1, 2, -1, 2).reshape(2, 2, 16, 16))
    assert not torch.equal(m16, m8)
    assert torch.allclose(m_all, (n16 * m16 + n8 * m8) / n_all, rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------------------------------------ 4. end to end
@pytest.mark.parametrize("sides", [(0, 0), (16, 16)], ids=["all", "16x16"])
def test_word_maps_vs_oracle(engine, report, tiny, sides):
    """the relative-to-maximum bound tests/test_gpu_models.py holds the tiny SD forward to in 16 bits (8e-3 x FMT); the two
    reference maps are 7.6e-1 / 8.6e-1 of the maximum apart (tests/test_word_maps_host.py).
    Measured on MI355X, fp16 build: all layers 8.4e-4, the 16 x 16 window 6.7e-4 of the maximum."""
    t = tiny
    ref, n_ref = t["ref"][sides]
    got, n = engine.word_maps(t["net"], t["x0"], t["c"], t["sel"], *t["level"], n_draws=wr.E2E["n_draws"], noise=t["noise"],
                              sides=sides)
    assert n == n_ref
    _check(report, "e2e/%dx%d" % sides, got, ref, rel=NET_REL, mean=None)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_name_the_parameter_and_launch_nothing(engine, tiny):
    import cycle_diffusion_amd as cda
    t = tiny
    tl, qa, qb = t["level"]
    x0, c, sel = t["x0"], t["c"], t["sel"]
    B = x0.shape[0]
    lib, h = engine.lib, engine.h
    out = torch.full((B, 2, 16, 16), -7.0).cuda()
    nl = C.c_int(-1)

    def entry(net_id=t["net"], ctx=c, N=2, B_sel=1, n=2, max_rows=2 * B, sides=(0, 0)):
        return lib.cd_word_maps(h, net_id, ptr(x0), ptr(ctx), ctx.shape[1], B, ptr(sel), B_sel, N, n, tl, C.c_float(qa),
                                C.c_float(qb), None, C.c_uint64(0), max_rows, sides[0], sides[1], ptr(out), C.byref(nl))

    err = lambda: lib.cd_last_error().decode()
    ho = engine.create_net(cda.ho_ddpm_desc(32, 32, (1, 2, 2), 1, (16,)))  # a pixel network
    assert entry(net_id=ho) != 0 and "text context" in err()
    d = tiny_sd_desc()
    d.precision = _ffi.CD_PREC_F32
    assert entry(net_id=engine.create_net(d)) != 0 and "fp32" in err()
    assert entry(ctx=torch.zeros(B, 97, 64).cuda()) != 0 and "context length 97" in err()
    for kw, word in ((dict(N=0), "N = 0"), (dict(N=9), "N = 9"), (dict(n=0), "n_draws"), (dict(n=4096), "n_draws"),
                     (dict(B_sel=3), "selector entries"), (dict(max_rows=B - 1), "max_rows"), (dict(sides=(16, 8)), "min_side"),
                     (dict(sides=(9, 15)), "no transformer block"), (dict(sides=(32, 64)), "no transformer block")):
        assert entry(**kw) != 0 and word in err(), (kw, err())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and nl.value == -1  # nothing ran
    assert entry() == 0  # the engine is usable after the refusals
    engine.synchronize()
    assert nl.value == 7 and float(out.min()) > 0


# ------------------------------------------------------------------------------------------------ 6. wrapper
SRC, TGT = ["a photo of a cat", "a red car"], ["a photo of a dog", "a blue car"]


def test_wrapper_word_maps_and_the_blend_composition():
    from cycle_diffusion_amd import auto_mask
    from test_gpu_wrappers import _make
    w = _make(True, n_trials=1, skip_steps=[0], decoder_unconditional_guidance_scales=[3.0])[0]
    x0 = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(1)).cuda()
    # the whitespace hash tokenizer: TGT[0] = start a photo of a dog end, TGT[1] = start a blue car end
    src_ids, eos = w._control_ids(SRC)
    tgt_ids, _ = w._control_ids(TGT)
    sch = w._schedule()
    k = auto_mask.level_index(0.5, len(sch))
    qa, qb = (float(v) for v in sch.coef_qsample(0)[k])
    level = (int(sch.coef_decode(0)["t"][k]), qa, qb)
    c, _ = w.get_condition(TGT, 2)
    with torch.no_grad():
        got = w.word_maps(x0, TGT, words=["a"], draws=2, seed=5)
        got1 = w.word_maps(x0[1:], TGT[1:], words=["a", "car"], draws=2, seed=5)
        edited = w.word_maps(x0, TGT, other_text=SRC, draws=2, seed=5)
    with pytest.raises(ValueError, match="does not occur"):
        w.word_maps(x0, TGT, words=["car"])  # the first prompt has no car
    with pytest.raises(ValueError, match="either"):
        w.word_maps(x0, TGT)
    # words=: the engine call with the selectors built by hand
    hand = torch.zeros(2, 1, 77)
    hand[0, 0, 1], hand[0, 0, 4], hand[1, 0, 1] = 1.0, 1.0, 1.0
    want, _ = w.engine.word_maps(w.unet, x0, c, hand.cuda(), *level, n_draws=2, seed=5)
    assert tuple(got.shape) == (2, 1, 16, 16) and torch.equal(got, want)
    hand1 = torch.zeros(1, 2, 77)
    hand1[0, 0, 1], hand1[0, 1, 3] = 1.0, 1.0
    want1, _ = w.engine.word_maps(w.unet, x0[1:], c[1:].contiguous(), hand1.cuda(), *level, n_draws=2, seed=5)
    assert tuple(got1.shape) == (1, 2, 16, 16) and torch.equal(got1, want1)
    # other_text=: edited_selector's row (dog at position 5 of the first prompt, blue at position 2 of the second)
    esel = torch.from_numpy(np.stack([attn_control.edited_selector(src_ids[b], tgt_ids[b], eos) for b in range(2)]))
    assert esel[0, 0].nonzero().flatten().tolist() == [5] and esel[1, 0].nonzero().flatten().tolist() == [2]
    want_e, _ = w.engine.word_maps(w.unet, x0, c, esel.cuda(), *level, n_draws=2, seed=5)
    assert tuple(edited.shape) == (2, 1, 16, 16) and torch.equal(edited, want_e)
    for m, marked in ((got[0], 2), (got[1], 1), (got1, 1), (edited, 1)):  # at most the number of marked tokens
        assert torch.isfinite(m).all() and float(m.min()) >= 0 and float(m.max()) <= marked
    # blend_mask of it goes where translate(mask=) takes a mask; the same call with the mask built independently
    f = w.vae_factor
    keep = attn_control.blend_mask(edited, threshold=0.9, pool=3, factor=f)
    e = edited.cpu().numpy()
    lit = np.ones((2, 1, 16 * f, 16 * f), dtype=np.float32)
    for b in range(2):
        d = np.array([[e[b, 0, max(0, y - 1):y + 2, max(0, x - 1):x + 2].max() for x in range(16)] for y in range(16)])
        lit[b, 0] = np.kron(1.0 - (d / d.max() > 0.9), np.ones((f, f)))
    assert 0 < float(keep.mean()) < 1 and np.array_equal(keep.cpu().numpy(), lit)
    image = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        torch.manual_seed(11)
        a = w.translate(image, SRC, TGT, mask=keep)
        torch.manual_seed(11)
        b = w.translate(image, SRC, TGT, mask=torch.from_numpy(lit))
    assert torch.isfinite(a).all() and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 7. driver
def test_main_writes_the_word_maps(tmp_path, monkeypatch):
    import json
    import os
    import sys
    import warnings
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.setenv("CYCLEDIFF_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.delenv("CYCLEDIFF_CLIP_RANKER", raising=False)
    rng = np.random.RandomState(7)
    Image.fromarray(rng.randint(0, 255, (64, 64, 3), dtype=np.uint8)).resize((512, 512), Image.BICUBIC).save(tmp_path / "im.png")
    row = {"img_path": "im.png", "encode_text": "a cat", "decode_text": "a dog"}
    (tmp_path / "data.json").write_text(json.dumps([row, row]))
    base = open(os.path.join(root, "config", "experiments", "bench_sd_c2.cfg")).read()
    base = base.replace("custom_steps = 99", "custom_steps = 4").replace("white_box_steps = 100", "white_box_steps = 5")
    (tmp_path / "c.cfg").write_text(base)
    sys.path.insert(0, root)
    import main as driver

    def run(name, *flags):
        out = tmp_path / name
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert driver.main(["--cfg", str(tmp_path / "c.cfg"), "--data", str(tmp_path / "data.json"), "--output_dir", str(out),
                                "--per_device_eval_batch_size", "2", "--synthetic-weights"] + list(flags)) == 0
        return out, json.loads((out / "metrics.json").read_text())

    on_dir, on = run("on", "--word_maps")
    off_dir, off = run("off")
    assert set(on["summary"]) == set(off["summary"]) and set(on) == set(off)
    assert [set(r) for r in on["samples"]] == [set(r) for r in off["samples"]]
    assert not (off_dir / "word_maps").exists()
    assert sorted(p.name for p in (on_dir / "word_maps").iterdir()) == ["%06d.png" % r["sample_id"] for r in on["samples"]]
    for r in on["samples"]:
        m = np.asarray(Image.open(on_dir / "word_maps" / ("%06d.png" % r["sample_id"])))
        assert m.shape == (512, 512) and m.dtype == np.uint8 and m.max() == 255
        assert np.array_equal(m, np.kron(m[::8, ::8], np.ones((8, 8), dtype=np.uint8)))  # nearest x 8 of the 64 x 64 latent
