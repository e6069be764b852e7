"""CPU: the keep-mask estimate's definition (tests/_automask_ref.py) checks itself - the fp32 emulation in the kernels' order
meets the derived bounds against float64, the comparison notices three known ways of getting it wrong, chunked accumulation is
the unchunked one - and the `[gan] auto_mask*` keys parse, refuse what is out of range and pick the stated level."""
import os

import numpy as np
import pytest

import _automask_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = range(20)


@pytest.mark.parametrize("shape", ar.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_emulation_meets_the_derived_bounds(shape):
    n, B, C, H, W = shape
    worst = 0.0
    for seed in SEEDS:
        es, et = ar.make_case(seed, *shape, equal_sample=1 if B > 1 and seed % 2 else None)
        for d in (0, 1, 3):
            for thr in (0.0, 0.5):
                ref = ar.reference64(es, et, 3.0, thr, d)
                em = ar.emulate32(es, et, 3.0, thr, d)
                worst = max(worst, ar.compare(em["map"], em["mean"], em["keep"], ref, n, C, thr, d)["map_rel"])
    assert worst <= 2.3e-7  # far inside (n C + 2) u: the bound is not what makes the comparison pass


def test_case_inputs_keep_clear_of_the_threshold():
    """what the case table was chosen for, at ratio 3 and thr 0.5: no pixel within 1e-4 of the threshold (the band of the
    largest case is 6e-5 wide), an edit share of 12 - 19 %"""
    for shape in ar.SHAPES:
        for seed in SEEDS:
            ref = ar.reference64(*ar.make_case(seed, *shape), 3.0, 0.5, 0)
            assert np.abs(ref["v"] - 0.5).min() > 1e-4, (shape, seed)
            assert 0.12 <= ref["edit"].mean() <= 0.19, (shape, seed, ref["edit"].mean())
            assert not ar.excluded(ref, shape[0], shape[2], 0.5, 3).any()


def _caught(mutant, es, et, thr, d):
    n, _B, C = es.shape[:3]
    ref = ar.reference64(es, et, 3.0, thr, d)
    good = ar.emulate32(es, et, 3.0, thr, d)
    ar.compare(good["map"], good["mean"], good["keep"], ref, n, C, thr, d)
    bad = ar.emulate32(es, et, 3.0, thr, d, mutant=mutant)
    with pytest.raises(AssertionError):
        ar.compare(bad["map"], bad["mean"], bad["keep"], ref, n, C, thr, d)


def test_whole_batch_mean_is_caught():
    _caught("batch_mean", *ar.make_case(0, 3, 2, 4, 16, 16), 0.5, 0)


def test_greater_or_equal_is_caught_on_a_tie():
    """a pixel whose two predictions are equal has v == 0 exactly, on both sides: at thr = 0 it is a tie, and not in the band"""
    es, et = ar.make_case(1, 3, 2, 4, 16, 16)
    et[:, 0, :, 2, 3] = es[:, 0, :, 2, 3]
    ref = ar.reference64(es, et, 3.0, 0.0, 0)
    assert ref["v"][0, 2, 3] == 0.0 and ref["keep"][0, 2, 3] == 1.0
    _caught("ge", es, et, 0.0, 0)


@pytest.mark.parametrize("d", [1, 3])
def test_short_dilation_window_is_caught(d):
    _caught("short_window", *ar.make_case(2, 3, 2, 4, 16, 16), 0.5, d)


def test_chunked_accumulation_is_the_unchunked_one_bit_for_bit():
    es, et = ar.make_case(3, 10, 2, 4, 32, 32)
    whole = ar.emulate32(es, et, 3.0, 0.5, 1)
    for chunks in ([1] * 10, [2] * 5, [3, 3, 3, 1], [4, 4, 2]):
        part = ar.emulate32(es, et, 3.0, 0.5, 1, chunks=chunks)
        for k in ("map", "mean", "keep"):
            assert np.array_equal(part[k], whole[k]), (chunks, k)


def test_identical_predictions_keep_everything():
    es, _ = ar.make_case(4, 3, 2, 4, 16, 16)
    for thr in (0.0, 0.5):
        for d in (0, 3):
            for r in (ar.reference64(es, es, 3.0, thr, d), ar.emulate32(es, es, 3.0, thr, d)):
                assert (r["map"] == 0).all() and (r["mean"] == 0).all() and (r["keep"] == 1).all()


# ------------------------------------------------------------------------------------------------ the [gan] keys
def test_gan_keys_parse_from_a_config(tmp_path):
    from cycle_diffusion_amd import auto_mask
    from cycle_diffusion_amd.utils.config_utils import get_config
    args = get_config("experiments/bench_sd_c2_diffedit.cfg", config_root=os.path.join(ROOT, "config"))
    kw = dict(iter(args.gan))
    assert kw["auto_mask"] == "diffedit" and kw["mask_source"] == "encoder"
    o = auto_mask.AutoMaskOptions(**auto_mask.pop_keys(kw))
    assert o.on and (o.draws, o.strength, o.ratio, o.threshold, o.dilate, o.seed) == (10, 0.5, 3.0, 0.5, 0, 0)
    assert not any(k.startswith("auto_mask") for k in kw)
    (tmp_path / "c.cfg").write_text("[gan]\nauto_mask = none\nauto_mask_draws = 4\nauto_mask_strength = 0.25\n"
                                    "auto_mask_ratio = 2\nauto_mask_threshold = 0.4\nauto_mask_dilate = 2\nauto_mask_seed = 9\n")
    o = auto_mask.AutoMaskOptions(**auto_mask.pop_keys(dict(iter(get_config("c.cfg", config_root=str(tmp_path)).gan))))
    assert not o.on and (o.draws, o.strength, o.ratio, o.threshold, o.dilate, o.seed) == (4, 0.25, 2.0, 0.4, 2, 9)
    assert not auto_mask.AutoMaskOptions().on and auto_mask.STREAM0 == ar.STREAM0
    # the plain configuration carries none of the keys
    assert not auto_mask.pop_keys(dict(iter(get_config("experiments/bench_sd_c2.cfg", config_root=os.path.join(ROOT, "config")).gan)))


@pytest.mark.parametrize("key,value", [("auto_mask", "grabcut"), ("auto_mask_draws", 0), ("auto_mask_draws", 4096),
                                       ("auto_mask_draws", 2.5), ("auto_mask_strength", 0.0), ("auto_mask_strength", 1.5),
                                       ("auto_mask_ratio", 0.0), ("auto_mask_ratio", -1.0), ("auto_mask_threshold", 1.0),
                                       ("auto_mask_threshold", -0.1), ("auto_mask_dilate", 9), ("auto_mask_dilate", -1),
                                       ("auto_mask_seed", -1)])
def test_out_of_range_values_raise_by_name(key, value):
    from cycle_diffusion_amd import auto_mask
    with pytest.raises(ValueError, match=key):
        auto_mask.AutoMaskOptions(**{key: value})


def test_level_index():
    from cycle_diffusion_amd import auto_mask
    for S, want in ((99, {0.01: 0, 0.5: 48, 1.0: 98}), (12, {0.01: 0, 0.5: 5, 1.0: 11})):
        for strength, k in want.items():
            assert auto_mask.level_index(strength, S) == k == max(0, min(S - 1, int(strength * S) - 1))


def test_wrappers_without_a_keep_mask_refuse_the_key_by_name():
    from cycle_diffusion_amd import auto_mask
    from cycle_diffusion_amd.gan_wrapper import baselines
    from cycle_diffusion_amd.gan_wrapper.ddpm_ddim_wrapper import DDPMDDIMWrapper
    from cycle_diffusion_amd.gan_wrapper.latent_wrapper import LatentDiffStochasticWrapper
    with pytest.raises(ValueError, match="auto_mask"):
        baselines.SDDDIBTextWrapper("none", 12, auto_mask="diffedit")
    with pytest.raises(ValueError, match="auto_mask_draws"):
        baselines.SDSDEditTextWrapper("none", 12, 0.1, [0.5], auto_mask_draws=4)
    with pytest.raises(ValueError, match="auto_mask"):
        DDPMDDIMWrapper("none", "ddim", 10, 10, auto_mask="diffedit")
    with pytest.raises(ValueError, match="auto_mask"):
        baselines.DDPMILVRWrapper("none", "ddim", 10, 10, 4, auto_mask="diffedit")
    with pytest.raises(ValueError, match="auto_mask"):
        LatentDiffStochasticWrapper("none", 10, 0.1, 10, auto_mask="diffedit")
    kw = {"auto_mask": "none", "auto_mask_seed": None, "eta": 0.1}
    auto_mask.refuse(kw, "x")  # off is not a refusal, and the keys are gone either way
    assert kw == {"eta": 0.1}
