"""Host side of the cross-attention control (cycle-diffusion_amd/attn_control.py, tests/_attn_control_ref.py): the mapper
builder on hand-written id arrays, the C ABI declarations, and the torch restatement the GPU tests compare against - that it
is the oracle's loop when the control is off, and that the control the GPU end-to-end test uses moves the result far beyond
that test's bound (a no-op implementation cannot pass it)."""
import os
import re

import numpy as np
import pytest
import torch

import _attn_control_ref as acr
import golden_util as gu
from cycle_diffusion_amd import _ffi
from cycle_diffusion_amd.attn_control import align, build_control
from oracle import nets, samplers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOS, EOS, L = 49406, 49407, 12


def ids(*rows):
    out = np.full((len(rows), L), EOS, dtype=np.int64)
    for b, r in enumerate(rows):
        out[b, :len(r) + 2] = [BOS] + list(r) + [EOS]
    return out


def pairs(M):
    return sorted((int(i), int(j)) for i, j in zip(*np.nonzero(M)))


# ------------------------------------------------------------------------------------------------ build_control
@pytest.mark.parametrize("mode", ["refine", "replace"])
def test_identical_prompts_give_the_identity(mode):
    a = ids([5, 6, 7], [8, 9])
    M, alpha, w = build_control(a, a, mode)
    assert M.dtype == alpha.dtype == w.dtype == np.float32 and M.shape == (2, L, L) and alpha.shape == w.shape == (2, L)
    assert np.array_equal(M, np.broadcast_to(np.eye(L, dtype=np.float32), (2, L, L)))
    assert np.array_equal(alpha, np.ones((2, L))) and np.array_equal(w, np.ones((2, L)))


def test_one_substituted_token():
    src, tgt = ids([5, 6, 7]), ids([5, 9, 7])
    M, alpha, _ = build_control(src, tgt, "refine")
    assert alpha[0, 2] == 0 and not M[0, :, 2].any()  # the substituted token keeps its own attention
    assert alpha[0].sum() == L - 1 and pairs(M[0]) == [(j, j) for j in range(L) if j != 2]
    M, alpha, _ = build_control(src, tgt, "replace")
    assert alpha[0, 2] == 1 and np.array_equal(M[0], np.eye(L))  # ... or takes the map of the token it replaces


def test_one_inserted_word_shifts_the_later_tokens():
    src, tgt = ids([5, 6, 7]), ids([5, 9, 6, 7])
    M, alpha, _ = build_control(src, tgt, "refine")
    assert list(alpha[0, :6]) == [1, 1, 0, 1, 1, 1]
    assert pairs(M[0])[:5] == [(0, 0), (1, 1), (2, 3), (3, 4), (4, 5)]  # 6 -> 6, 7 -> 7, end token -> end token
    assert align([5, 6, 7], [5, 9, 6, 7]) == [0, -1, 1, 2]
    # a removed word: the later tokens shift the other way, nothing is left without a map
    M, alpha, _ = build_control(tgt, src, "refine")
    assert alpha[0].sum() == L and pairs(M[0])[:5] == [(0, 0), (1, 1), (3, 2), (4, 3), (5, 4)]


def test_replace_refuses_prompts_of_unequal_length():
    with pytest.raises(ValueError, match="same number of tokens"):
        build_control(ids([5, 6, 7]), ids([5, 9, 6, 7]), "replace")
    with pytest.raises(ValueError, match="mode"):
        build_control(ids([5]), ids([5]), "blend")
    with pytest.raises(ValueError, match=r"\[B, L\]"):
        build_control(ids([5]), ids([5], [6]), "refine")


def test_padding_maps_in_order_and_is_clipped():
    src, tgt = ids([5, 6, 7, 8, 9]), ids([5])  # source end token at 6, target end token at 2
    M, alpha, _ = build_control(src, tgt, "refine")
    want = [(0, 0), (1, 1)] + [(min(6 + k, L - 1), 2 + k) for k in range(L - 2)]
    assert pairs(M[0]) == sorted(want) and alpha[0].sum() == L
    assert M[0, L - 1, 2 + (L - 1 - 6):].all()  # the clipped tail all reads the last source position
    # another end-token id (the BERT tokenizers' [SEP] = 102 with [PAD] = 0 behind it)
    s2 = np.array([[101, 5, 6, 102, 0, 0]])
    t2 = np.array([[101, 5, 102, 0, 0, 0]])
    M2, a2, _ = build_control(s2, t2, "refine", eos_id=102)
    assert pairs(M2[0]) == [(0, 0), (1, 1), (3, 2), (4, 3), (5, 4), (5, 5)] and a2[0].sum() == 6


def test_reweight_by_position_and_by_token_id():
    src, tgt = ids([500, 600, 700]), ids([500, 900, 600, 900])
    _, _, w = build_control(src, tgt, "refine", reweight={900: 2.0, 1: 0.5})
    want = np.ones(L, dtype=np.float32)
    want[[2, 4]] = 2.0
    want[1] = 0.5
    assert np.array_equal(w[0], want)


def test_header_and_ffi_declare_the_new_entry_points():
    txt = open(os.path.join(ROOT, "include", "cyclediff.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _ffi.load_library()
    for s in ("cd_op_cross_attention_ctrl",):
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert s in _ffi.SIGNATURES and hasattr(lib, s), s
        n_args = len(re.search(r"\b%s\s*\((.*?)\)" % s, txt, flags=re.S).group(1).split(","))
        assert n_args == len(_ffi.SIGNATURES[s]), (s, n_args)
    # the control of the coupled loop is an option struct of cd_cycle_translate: in the header and in _ffi with equal fields
    # (tests/test_abi.py holds their types and offsets to the header's), beside the keep-mask's and not in its place
    body = re.search(r"typedef\s+struct\s+cd_attn_ctrl\s*\{(.*?)\}\s*cd_attn_ctrl\s*;", txt, flags=re.S).group(1)
    names = [re.search(r"(\w+)$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert names == [f for f, _ in _ffi.AttnCtrl._fields_] == ["mapper", "alpha", "weight", "B_ctrl", "n_ctrl"]
    fields = dict(_ffi.TranslateArgs._fields_)
    assert fields["ctrl"]._type_ is _ffi.AttnCtrl and fields["mask"]._type_ is _ffi.KeepMask
    assert re.search(r"const\s+cd_attn_ctrl\s*\*\s*ctrl\s*;", txt) and re.search(r"const\s+cd_keep_mask\s*\*\s*mask\s*;", txt)


def test_example_config_carries_the_switch():
    from cycle_diffusion_amd.utils.config_utils import get_config
    gan = dict(iter(get_config("experiments/bench_sd_c2_cac.cfg", config_root=os.path.join(ROOT, "config")).gan))
    base = dict(iter(get_config("experiments/bench_sd_c2.cfg", config_root=os.path.join(ROOT, "config")).gan))
    assert gan.pop("cac_steps") == 0.4 and gan.pop("cac_mode") == "refine" and gan == base


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.fixture(scope="module")
def tiny():
    fx = gu.load("latent_cycle_tiny")
    sd = gu.weights(fx)
    x0, c, uc, c2 = acr.e2e_inputs()
    e = acr.E2E
    noise = gu.latent_noise(e["noise_seed"], x0.shape, e["S"] - e["skip"])
    run = lambda ctrl, n: acr.coupled_translate(sd, gu.TINY_SD_CFG, x0, c, c2, uc, e["dec_g"], e["S"], e["skip"], e["eta"], noise,
                                                ctrl, n)
    z, x = run(None, 0)  # computed once, shared, left unchanged
    return dict(sd=sd, x0=x0, c=c, uc=uc, c2=c2, noise=noise, run=run, z=z, x=x)


def test_restatement_without_control_is_the_oracle_loop(tiny):
    e = acr.E2E
    unet = lambda x, t, cc: nets.openai_unet(tiny["sd"], gu.TINY_SD_CFG, x, t, cc)
    with torch.no_grad():
        z = samplers.latent_encode(samplers.cfg_model(unet, tiny["c"], tiny["uc"], 1.0), tiny["x0"], e["S"], e["eta"],
                                   tiny["noise"], skip_steps=e["skip"])
        x = samplers.latent_decode(samplers.cfg_model(unet, tiny["c2"], tiny["uc"], e["dec_g"]), z[0], torch.stack(z[1:], 1),
                                   e["S"], e["eta"], skip_steps=e["skip"])
    # one stacked forward against the oracle's separate ones: the same per-sample arithmetic (a host GEMM may block a batch of
    # 6 differently from 2 and 4, so the comparison is to fp32 rounding over the 20 steps, not to the bit)
    assert torch.allclose(torch.stack(tiny["z"], 1), torch.stack(z, 1), rtol=1e-4, atol=1e-4)
    assert torch.allclose(tiny["x"], x, rtol=1e-4, atol=1e-4)
    # n_ctrl = 0 with a control given: exactly the uncontrolled loop
    z0, x0_ = tiny["run"](acr.e2e_control(), 0)
    assert torch.equal(x0_, tiny["x"]) and all(torch.equal(a, b) for a, b in zip(z0, tiny["z"]))


def test_restatement_alpha_zero_is_the_uncontrolled_loop_to_rounding(tiny):
    Lc = tiny["c"].shape[1]
    ctl = (torch.eye(Lc).repeat(2, 1, 1), torch.zeros(2, Lc), torch.ones(2, Lc))
    z, x = tiny["run"](ctl, acr.E2E["n_ctrl"])
    assert all(torch.equal(a, b) for a, b in zip(z, tiny["z"]))  # the encoder rows are the oracle's own arithmetic
    assert torch.allclose(x, tiny["x"], rtol=1e-4, atol=1e-4)


def test_the_end_to_end_control_is_no_no_op(tiny):
    """The GPU end-to-end test holds the engine to 8e-3 (fp16 build) of the maximum against this restatement: the controlled
    and the uncontrolled restatement must be at least ten times that apart (8e-2), and the encoder's z must not move at all.
    Measured on acr.e2e_inputs() at n_ctrl = 8: 1.8e-1 (noise seed 3: 1.7e-1); on unit-scale contexts it is 1.0e-2, which is
    why the end-to-end inputs scale them (see e2e_inputs)."""
    z, x = tiny["run"](acr.e2e_control(), acr.E2E["n_ctrl"])
    assert all(torch.equal(a, b) for a, b in zip(z, tiny["z"]))
    rel = ((x - tiny["x"]).abs().max() / tiny["x"].abs().max()).item()
    print("controlled vs uncontrolled restatement: %.3e of the maximum" % rel)
    assert torch.isfinite(x).all() and rel >= 10 * 8e-3, rel
