"""Host side of the local blend (no GPU): the selectors, the keys and their refusals, translate()'s call on a
recording stand-in engine, and the fixtures the GPU tests compare with - that the mask kernel's operands stay clear of the
threshold, that the restatement is the unblended loop when the blend is off, and that the end-to-end fixture is flip-free, moves
the result far beyond the GPU test's bound and keeps as well as edits."""
import numpy as np
import pytest
import torch

import _attn_control_ref as acr
import _local_blend_ref as lbr
import _translate_calls as tc
import golden_util as gu
from cycle_diffusion_amd import attn_control
from cycle_diffusion_amd.gan_wrapper import baselines
from cycle_diffusion_amd.gan_wrapper.latent_text_wrapper import _LatentStochasticTextWrapper

BOS, EOS, L = 49406, 49407, 12


def ids(*toks):
    out = np.full((L,), EOS, dtype=np.int64)
    out[:len(toks) + 2] = [BOS] + list(toks) + [EOS]
    return out


# ------------------------------------------------------------------------------------------------ selectors, n_start
def test_selectors_of_a_swap_an_insertion_and_identical_prompts():
    ss, st = attn_control.local_blend_selectors(ids(5, 6, 7), ids(5, 9, 7), EOS)
    assert ss.dtype == st.dtype == np.float32 and ss.shape == st.shape == (L,)
    assert ss.nonzero()[0].tolist() == [2] and st.nonzero()[0].tolist() == [2]  # the swapped word, on either side
    ss, st = attn_control.local_blend_selectors(ids(5, 6, 7), ids(5, 9, 6, 7), EOS)
    assert not ss.any() and st.nonzero()[0].tolist() == [2]  # an insertion leaves the source without a word of its own
    ss, st = attn_control.local_blend_selectors(ids(5, 9, 6, 7), ids(5, 6, 7), EOS)
    assert ss.nonzero()[0].tolist() == [2] and not st.any()  # ... and a removal the target
    ss, st = attn_control.local_blend_selectors(ids(5, 6, 7), ids(5, 6, 7), EOS)
    assert not ss.any() and not st.any()  # identical prompts: zero selectors, and a zero map keeps everything
    z = torch.zeros(1, 8, 8)
    assert bool((lbr.mask_ref(z, z, 2, 3, 0.3) == 1).all())
    # words by hand: every occurrence, several tokens per word, an empty side
    ss, st = attn_control.local_blend_selectors(ids(5, 6, 7, 6), ids(5, 9, 8, 7), EOS, words=([[6]], [[9, 8], [7]]))
    assert ss.nonzero()[0].tolist() == [2, 4] and st.nonzero()[0].tolist() == [2, 3, 4]
    ss, st = attn_control.local_blend_selectors(ids(5, 6), ids(5, 9), EOS, words=([], [[9]]))
    assert not ss.any() and st.nonzero()[0].tolist() == [2]
    with pytest.raises(ValueError, match="does not occur"):
        attn_control.local_blend_selectors(ids(5, 6), ids(5, 9), EOS, words=([[9]], [[9]]))
    with pytest.raises(ValueError, match="one id row"):
        attn_control.local_blend_selectors(ids(5, 6)[None], ids(5, 9)[None], EOS)


@pytest.mark.parametrize("frac, K, want", [(0.2, 99, 19), (0.2, 95, 19), (0.2, 20, 4), (0.0, 8, 0), (1.0, 8, 8), (0.5, 7, 3),
                                           (0.2, 4, 0)])
def test_n_start_per_member(frac, K, want):
    assert attn_control.local_blend_start(frac, K) == want


def test_n_start_refuses_a_fraction_outside_the_unit_interval():
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="local_blend_start"):
            attn_control.local_blend_start(bad, 10)


# ------------------------------------------------------------------------------------------------ keys and refusals
def _init(**kw):
    """the wrapper's __init__ up to the point where it would create the engine: the keys are checked ahead of it"""
    args = dict(source_model_type="none", custom_steps=4, eta=0.1, white_box_steps=5, skip_steps=[0], device="no-such-device")
    args.update(kw)
    return _LatentStochasticTextWrapper(**args)


@pytest.mark.parametrize("kw, word", [
    (dict(local_blend="pixels"), "local_blend must be one of"),
    (dict(local_blend="words", local_blend_pool=4), "local_blend_pool"),
    (dict(local_blend="words", local_blend_pool=9), "local_blend_pool"),
    (dict(local_blend="words", local_blend_side=-1), "local_blend_side"),
    (dict(local_blend="words", local_blend_start=1.2), "local_blend_start"),
    (dict(local_blend="words", local_blend_threshold=float("nan")), "local_blend_threshold"),
    (dict(local_blend="words", precision="fp32"), "16-bit precision"),
    (dict(local_blend="words", precision="fp32x3"), "16-bit precision"),
])
def test_keys_are_refused_by_name_before_the_engine_exists(kw, word):
    with pytest.raises(ValueError, match=word):
        _init(**kw)


def test_other_wrappers_refuse_the_keys():
    with pytest.raises(ValueError, match="DDIB does not use local_blend"):
        baselines.SDDDIBTextWrapper(source_model_type="none", custom_steps=4, local_blend="words")
    with pytest.raises(ValueError, match="SDEdit does not use local_blend, local_blend_pool"):
        baselines.SDSDEditTextWrapper(source_model_type="none", custom_steps=4, eta=0.1, sdedit_strengths=[0.5], local_blend="words",
                                      local_blend_pool=3)
    from cycle_diffusion_amd.gan_wrapper.ddpm_ddim_wrapper import DDPMDDIMWrapper
    with pytest.raises(ValueError, match="does not use local_blend"):
        DDPMDDIMWrapper("none", "ddim", 4, 4, local_blend="words")
    kw = dict(local_blend="none")  # `none` is no request: the keys are dropped
    attn_control.refuse_local_blend(kw, "X")
    assert kw == {}


class _Engine(tc.StandInEngine):
    def cycle_translate_blend(self, *a, **kw):
        z, x = self._coupled("cycle_translate_blend", a, kw)
        nd = kw.get("n_dec", 1)
        B = a[2].shape[0]
        keep = ((torch.arange(nd * B * tc.LAT * tc.LAT) + len(self.calls)) % 2).float().reshape(nd * B, 1, tc.LAT, tc.LAT)
        return z, x, torch.zeros((1 + nd) * B, a[7], a[7]), keep


def _wrapper(dec=(3.0,), enc=(1.0,), **attrs):
    blend = dict(local_blend="words", local_blend_threshold=0.3, local_blend_pool=3, local_blend_side=0, local_blend_start=0.2)
    blend.update(attrs)
    w = tc.make_wrapper(list(dec), list(enc), **blend)
    w.engine = _Engine()
    return w


SRC, TGT = ["a cat", "a red car", "x"], ["a dog", "a blue car", "x"]


def _image():
    return tc.ramp((tc.BSZ, 3, tc.RES, tc.RES), 5) + 0.5


def test_translate_calls_the_blend_entry_with_the_keys_and_the_selectors():
    w = _wrapper()
    w.translate(_image(), SRC, TGT)
    calls = [c for c in w.engine.calls if c[0] == "cycle_translate_blend"]
    assert w.last_translate_coupled is True and len(calls) >= 1
    assert not [c for c in w.engine.calls if c[0] in ("cycle_translate", "cycle_translate_masked", "cycle_translate_ctrl")]
    for name, args, kw in calls:
        kw = dict(kw)
        assert args[7] == tc.LAT // 4  # local_blend_side = 0: image_size / 4
        assert kw["pool"] == 3 and kw["thr"] == 0.3 and kw["ctrl"] is None
    assert len(w.last_local_blend_masks) == w._ensemble_size()
    assert tuple(w.last_local_blend_mask.shape) == (tc.BSZ, 1, tc.LAT, tc.LAT)


def test_n_start_follows_each_member_s_chain(monkeypatch):
    w = _wrapper(local_blend_start=0.5)
    seen = []
    real = w.engine.cycle_translate_blend
    w.engine.cycle_translate_blend = lambda *a, **k: (seen.append((len(a[4]), k["n_start"])), real(*a, **k))[1]
    w.translate(_image(), SRC, TGT)
    assert seen and {K for K, _ in seen} == {tc.STEPS - sk for sk in w.skip_steps}  # members of both chain lengths ran
    assert all(n == int(0.5 * K) for K, n in seen)


def test_translate_composes_with_the_control_and_chunks_past_the_token_limit():
    w = _wrapper(cac_steps=0.5)
    seen = []
    real = w.engine.cycle_translate_blend
    w.engine.cycle_translate_blend = lambda *a, **k: (seen.append((a[2].shape[0], len(a[4]), k["ctrl"])), real(*a, **k))[1]
    w.couple_max_tokens = 3 * tc.LAT * tc.LAT  # one sample of one member per call
    w.translate(_image(), SRC, TGT)
    assert w.last_translate_coupled is True and len(seen) == tc.BSZ * w._ensemble_size()
    for rows, K, ctrl in seen:
        assert rows == 1 and ctrl is not None and ctrl[3] == int(0.5 * K) and tuple(ctrl[0].shape) == (1, tc.CTX_LEN, tc.CTX_LEN)
    assert tuple(w.last_local_blend_mask.shape) == (tc.BSZ, 1, tc.LAT, tc.LAT)


def test_translate_refuses_what_the_blend_cannot_compose_with():
    w = _wrapper()
    with pytest.raises(ValueError, match="no mask= and no auto_mask"):
        w.translate(_image(), SRC, TGT, mask=tc.pixel_mask())
    w = _wrapper()
    w.auto_mask_opts = type(w.auto_mask_opts)("diffedit", 10, 0.5, 3.0, 0.5, 0, 0)
    with pytest.raises(ValueError, match="no mask= and no auto_mask"):
        w.translate(_image(), SRC, TGT)
    w = _wrapper(precision="fp32")
    with pytest.raises(ValueError, match="16-bit precision"):
        w.translate(_image(), SRC, TGT)
    w = _wrapper(white_box_steps=3)
    with pytest.raises(ValueError, match="local_blend needs the DPM-Encoder over the whole chain"):
        w.translate(_image(), SRC, TGT)
    w = _wrapper(dec=(3.0, 1.0))
    with pytest.raises(ValueError, match="local_blend: every decoder scale must ride"):
        w.translate(_image(), SRC, TGT)
    w = _wrapper()
    with pytest.raises(ValueError, match="local_blend needs translate"):
        w.forward([torch.zeros(tc.BSZ, 4)], _image(), SRC, TGT)
    # switched off, a per-call request still works and the attribute-less wrapper of the pinned records is untouched
    w = _wrapper(local_blend="none")
    w.translate(_image(), SRC, TGT)
    assert not [c for c in w.engine.calls if c[0] == "cycle_translate_blend"] and getattr(w, "last_local_blend_mask", None) is None
    w.translate(_image(), ["x y"] * tc.BSZ, ["x z"] * tc.BSZ, local_blend=(["x"], ["z"]))
    assert [c for c in w.engine.calls if c[0] == "cycle_translate_blend"]


# ------------------------------------------------------------------------------------------------ the GPU tests' fixtures
@pytest.mark.parametrize("case", lbr.MASK_CASES, ids=["b%d_bd%d_s%d_f%d_p%d" % c for c in lbr.MASK_CASES])
def test_mask_operands_stay_clear_of_the_threshold(case):
    """the fp32 quotient of the kernel and torch's are both correctly rounded, and were they not, 1e-5 is 80 ulp of 1"""
    _B, _Bd, _s, _f, pool = case
    for t in lbr.mask_operands(case):
        assert t.dtype == torch.float32 and float(t.min()) >= 0
        assert float((lbr.ratios(t, pool) - lbr.MASK_THR).abs().min()) > lbr.MASK_GAP
        assert float((lbr.ratios(t.double(), pool) - lbr.MASK_THR).abs().min()) > lbr.MASK_GAP


@pytest.mark.parametrize("name", lbr.MASK_SPECIALS)
def test_mask_edge_cases_stay_clear_of_the_threshold(name):
    src, tgt, f, pool, thr = lbr.mask_special(name)
    for t in (src, tgt):
        assert float((lbr.ratios(t, pool) - thr).abs().min()) > lbr.MASK_GAP
    keep = lbr.mask_ref(src, tgt, f, pool, thr)
    assert tuple(keep.shape) == (1, 1, 8 * f, 8 * f) and bool(((keep == 0) | (keep == 1)).all())


@pytest.fixture(scope="module")
def e2e():
    e = lbr.E2E
    sd = gu.weights(gu.load("latent_cycle_tiny"))
    x0, c, uc, c2 = acr.e2e_inputs()
    K = e["S"] - e["skip"]
    noise = gu.latent_noise(e["noise_seed"], x0.shape, K)
    run = lambda n_start: lbr.coupled_translate_blend(
        sd, gu.TINY_SD_CFG, x0, c, c2, uc, e["dec_g"], e["S"], e["skip"], e["eta"], noise, lbr.key_selector(e["keys_src"]),
        lbr.key_selector(e["keys_tgt"]), e["side"], e["pool"], e["thr"], n_start)
    plain = acr.coupled_translate(sd, gu.TINY_SD_CFG, x0, c, c2, uc, e["dec_g"], e["S"], e["skip"], e["eta"], noise)
    return dict(K=K, on=run(e["n_start"]), off=run(K), plain=plain)


def test_the_restatement_with_the_blend_off_is_the_unblended_loop(e2e):
    z, x = e2e["plain"]
    assert torch.equal(e2e["off"]["x"], x) and all(torch.equal(a, b) for a, b in zip(e2e["off"]["z"], z))
    assert e2e["off"]["margin"] == float("inf") and bool((e2e["off"]["keep"] == 1).all())


def test_the_end_to_end_fixture_is_flip_free(e2e):
    """no p / mx of any cell, map and step within 10 x the bound the GPU test holds acc_out to (relative to the maximum, as
    p / mx is): an error of the engine's sums within that bound cannot move a cell across the threshold"""
    assert 0 < lbr.E2E["n_start"] < e2e["K"]
    print("local_blend/e2e margin %.4f" % e2e["on"]["margin"])
    assert e2e["on"]["margin"] >= lbr.E2E_MARGIN, e2e["on"]["margin"]


def test_the_end_to_end_blend_is_no_no_op(e2e):
    _z, xu = e2e["plain"]
    apart = ((e2e["on"]["x"] - xu).abs().max() / xu.abs().max()).item()
    print("local_blend/e2e blended vs unblended %.3e of the maximum" % apart)
    assert apart >= 10 * lbr.E2E_REL, apart
    keep = e2e["on"]["keep"]
    assert all(0 < float(keep[b].mean()) < 1 for b in range(keep.shape[0]))  # kept and edited cells in every sample
    assert all(torch.equal(a, b) for a, b in zip(e2e["on"]["z"], e2e["plain"][0]))  # the encoder never sees the blend
