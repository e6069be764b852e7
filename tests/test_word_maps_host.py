"""Host side of the per-word cross-attention maps (cycle-diffusion_amd/attn_control.py word_selector / edited_selector /
blend_mask, tests/_word_maps_ref.py): the selectors on hand-written id arrays, the LocalBlend rule against a
literal restatement, the C ABI declarations, and that the reference maps the GPU end-to-end test compares against depend on
the chosen key and on the pixel far beyond that test's bound (a kernel that returned |sel| / L could not pass it)."""
import os
import re

import numpy as np
import pytest
import torch

import _word_maps_ref as wr
import golden_util as gu
from cycle_diffusion_amd import _ffi
from cycle_diffusion_amd.attn_control import blend_mask, edited_selector, word_selector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOS, EOS, L = 49406, 49407, 12


def ids(*toks):
    out = np.full((L,), EOS, dtype=np.int64)
    out[:len(toks) + 2] = [BOS] + list(toks) + [EOS]
    return out


def marked(row):
    return [int(j) for j in np.nonzero(row)[0]]


# ------------------------------------------------------------------------------------------------ word_selector
def test_word_selector_single_multi_and_repeated_words():
    p = ids(5, 6, 7, 6, 7, 8)
    sel = word_selector(p, [[5], [6, 7], [8]], EOS)
    assert sel.dtype == np.float32 and sel.shape == (3, L) and set(np.unique(sel)) <= {0.0, 1.0}
    assert marked(sel[0]) == [1]             # a single-token word
    assert marked(sel[1]) == [2, 3, 4, 5]    # a two-token word occurring twice
    assert marked(sel[2]) == [6]
    assert marked(word_selector(p, [[7, 6]], EOS)[0]) == [3, 4]  # the sequence, not the set
    assert marked(word_selector(ids(9, 9, 9), [[9]], EOS)[0]) == [1, 2, 3]


def test_word_selector_marks_nothing_from_the_end_token_on():
    p = ids(5, 6)
    for w in ([EOS], [6, EOS], [BOS]):  # the end token, a sequence running into it, the start token
        with pytest.raises(ValueError, match="does not occur"):
            word_selector(p, [w], EOS)
    sel = word_selector(p, [[5], [6]], EOS)
    assert not sel[:, 3:].any() and not sel[:, 0].any()
    # another end-token id (the BERT tokenizers' [SEP] = 102 with [PAD] = 0 behind it)
    p2 = np.array([101, 5, 0, 102, 0, 0])
    assert marked(word_selector(p2, [[0]], eos_id=102)[0]) == [2]


def test_word_selector_refusals():
    p = ids(5, 6, 7)
    with pytest.raises(ValueError, match=r"word 1 .*\[9\].* does not occur"):
        word_selector(p, [[5], [9]], EOS)
    with pytest.raises(ValueError, match="1 to 8 words, got 9"):
        word_selector(p, [[5]] * 9, EOS)
    with pytest.raises(ValueError, match="1 to 8 words, got 0"):
        word_selector(p, [], EOS)
    assert word_selector(p, [[5]] * 8, EOS).shape == (8, L)


# ------------------------------------------------------------------------------------------------ edited_selector
def test_edited_selector_on_the_refine_and_replace_pairs():
    # the prompt pairs of tests/test_attn_control_host.py: one substituted token, one inserted word, one removed word
    sel = edited_selector(ids(5, 6, 7), ids(5, 9, 7), EOS)
    assert sel.dtype == np.float32 and sel.shape == (1, L) and marked(sel[0]) == [2]
    assert marked(edited_selector(ids(5, 6, 7), ids(5, 9, 6, 7), EOS)[0]) == [2]
    assert marked(edited_selector(ids(500, 600, 700), ids(500, 900, 600, 900), EOS)[0]) == [2, 4]
    with pytest.raises(ValueError, match="introduces no token"):
        edited_selector(ids(5, 9, 6, 7), ids(5, 6, 7), EOS)  # a removed word introduces nothing
    with pytest.raises(ValueError, match="introduces no token"):
        edited_selector(ids(5, 6, 7), ids(5, 6, 7), EOS)
    with pytest.raises(ValueError, match="one id row"):
        edited_selector(ids(5)[None], ids(6)[None], EOS)


# ------------------------------------------------------------------------------------------------ blend_mask
def _blend_literal(maps, threshold, pool):
    B, N, h, w = maps.shape
    keep = np.ones((B, 1, h, w), dtype=np.float32)
    r = pool // 2
    for b in range(B):
        s = maps[b].sum(0)
        d = np.zeros_like(s)
        for y in range(h):
            for x in range(w):
                d[y, x] = s[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1].max()
        if d.max() > 0:
            keep[b, 0] = 1.0 - (d / d.max() > threshold)
    return keep


@pytest.mark.parametrize("pool", [1, 3, 5])
def test_blend_mask_is_the_local_blend_rule(pool):
    maps = np.zeros((3, 2, 8, 8), dtype=np.float32)
    maps[0, 0, 4, 3] = 4.0                      # a single hot pixel
    maps[1, 0, 0, 0], maps[1, 1, 0, 0] = 1.0, 2.0  # a corner, summed over the words; and a weaker pixel below the threshold
    maps[1, 1, 6, 6] = 0.5
    # image 2 is all zero
    got = blend_mask(torch.from_numpy(maps), threshold=0.3, pool=pool)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 1, 8, 8)
    assert np.array_equal(got.numpy(), _blend_literal(maps, 0.3, pool))
    r = pool // 2
    edit = 1.0 - got[0, 0].numpy()
    assert edit.sum() == pool * pool and edit[4 - r:4 + r + 1, 3 - r:3 + r + 1].all()  # the hot pixel dilates to pool x pool
    assert bool((got[2] == 1).all())                                                    # an all-zero image keeps everything
    assert got[1, 0, 6, 6] == 1 and got[1, 0, 0, 0] == 0                                # 0.5 / 3 < 0.3


def test_blend_mask_factor_gives_the_latent_mask_back_under_the_block_mean():
    g = torch.Generator().manual_seed(3)
    maps = torch.randint(0, 5, (2, 3, 8, 8), generator=g).float() * (torch.rand(2, 3, 8, 8, generator=g) < 0.1)
    lat = blend_mask(maps, 0.3, 3)
    pix = blend_mask(maps, 0.3, 3, factor=4)
    assert tuple(pix.shape) == (2, 1, 32, 32) and 0 < float(lat.mean()) < 1
    assert torch.equal(torch.nn.functional.avg_pool2d(pix, 4), lat)
    with pytest.raises(ValueError, match="pool"):
        blend_mask(maps, pool=2)
    with pytest.raises(ValueError, match=r"\[B, N, h, w\]"):
        blend_mask(maps[0])


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_and_ffi_declare_the_new_entry_points():
    txt = open(os.path.join(ROOT, "include", "cyclediff.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _ffi.load_library()
    for s in ("cd_word_maps", "cd_op_cross_attention_maps"):
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert s in _ffi.SIGNATURES and hasattr(lib, s), s
        n_args = len(re.search(r"\b%s\s*\((.*?)\)" % s, txt, flags=re.S).group(1).split(","))
        assert n_args == len(_ffi.SIGNATURES[s]), (s, n_args)
    assert len(_ffi.SIGNATURES["cd_word_maps"]) == 20 and len(_ffi.SIGNATURES["cd_op_cross_attention_maps"]) == 15


def test_the_draws_have_a_stream_band_of_their_own():
    """n_draws goes up to 4095: streams STREAM0 .. STREAM0 + 4094 may meet no other loop's, the keep-mask estimate's band and
    the VAE posterior's 0x7a65 (which sits inside the band at 0x7000) included"""
    import _automask_ref as ar
    import _philox_ref as pr
    mine = set(range(wr.STREAM0, wr.STREAM0 + pr.MAX_STEPS))
    assert wr.STREAM0 % pr.BAND == 0
    for loop in pr._LOOPS:
        assert not mine & pr.band_streams(loop, pr.MAX_STEPS), loop
    assert not mine & set(range(ar.STREAM0, ar.STREAM0 + pr.MAX_STEPS))


def test_only_the_cycle_diffusion_text_wrappers_have_word_maps():
    """instances made without __init__, as tests/_translate_calls.py makes them: no engine is touched"""
    from cycle_diffusion_amd.gan_wrapper import baselines
    from cycle_diffusion_amd.gan_wrapper.ddpm_ddim_wrapper import DDPMDDIMWrapper
    from cycle_diffusion_amd.gan_wrapper.latent_text_wrapper import LatentDiffStochasticTextWrapper, SDStochasticTextWrapper
    for cls in (SDStochasticTextWrapper, LatentDiffStochasticTextWrapper):
        assert callable(getattr(cls.__new__(cls), "word_maps"))
    for cls in (baselines.SDSDEditTextWrapper, baselines.LatentDiffSDEditTextWrapper, baselines.SDDDIBTextWrapper,
                baselines.LatentDiffDDIBTextWrapper, baselines.DDPMDDIBWrapper, baselines.DDPMSDEditWrapper,
                baselines.DDPMILVRWrapper, DDPMDDIMWrapper):
        assert not hasattr(cls.__new__(cls), "word_maps"), cls


# ------------------------------------------------------------------------------------------------ discrimination
def test_reference_maps_depend_on_the_key_and_on_the_pixel():
    """The GPU end-to-end test holds the engine to 8e-3 (fp16 build) of the maximum against word_maps_ref: two one-key maps
    must be at least ten times that apart (8e-2 of the maximum), and each map's spatial standard deviation must be at least
    8e-2 of its own maximum. Measured on wr.e2e_inputs() (contexts at standard deviation 4), keys 3 and 11: all layers 7.6e-1
    apart, std / max 1.2e-1 .. 1.6e-1; the 16 x 16 window 8.6e-1 apart, std / max 9.9e-2 .. 1.7e-1. At unit scale the
    softmaxes are flat and every map is the constant 1 / L."""
    fx = gu.load("latent_cycle_tiny")
    sd = gu.weights(fx)
    x0, c, noise, (t, qa, qb) = wr.e2e_inputs()
    floor = 10 * 8e-3
    for sides, n_want in (((0, 0), 7), ((16, 16), 3)):
        (a, n_layers), (b, _) = [wr.word_maps_ref(sd, gu.TINY_SD_CFG, x0, c, wr.one_key(j), t, qa, qb, noise, sides)
                                 for j in wr.E2E["keys"]]
        assert n_layers == n_want and tuple(a.shape) == (2, 1, 16, 16)
        apart = ((a - b).abs().max() / max(a.max(), b.max())).item()
        spread = [(m.std(dim=(2, 3)) / m.amax(dim=(2, 3))).min().item() for m in (a, b)]
        print("word_maps/discrimination sides %s: apart %.3e of the maximum, std / max %s" % (sides, apart, spread))
        assert apart >= floor and min(spread) >= floor, (sides, apart, spread)
        assert bool((a >= 0).all()) and float(a.max()) <= 1.0
