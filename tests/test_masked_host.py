"""CPU: the host side of the region-keeping decode - the q-sample coefficient rows, the block-mean latent mask, the triplet
reader's `mask_path`, the new C-ABI symbols, and the restatement of tests/_masked_ref.py replaying the reference fixture
(tests/golden/masked_latent.npz, scripts/gen_golden_masked.py) on the oracle's small U-Net."""
import json
import os
import re

import numpy as np
import torch

import _baselines_ref as br
import _masked_ref as mr
import golden_util as gu
from cycle_diffusion_amd import _ffi, schedule
from oracle import nets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["cd_ddim_decode_masked", "cd_op_sched_step_masked"]


def _sched(p):
    return schedule.DDIMSchedule(schedule.latent_alphas_cumprod(), p["S"], p["eta"])


def test_coef_qsample_equals_the_reference_rows_bit_for_bit():
    fx = mr.load_fixture()
    p = mr.params(fx)
    sch = _sched(p)
    assert np.array_equal(sch.timesteps, fx["timesteps"])
    for skip in (0, 7):
        q = sch.coef_qsample(skip)
        assert q.dtype == np.float32 and q.shape == (p["S"] - skip, 2)
        assert np.array_equal(q.view(np.uint32), fx["qcoef"][:p["S"] - skip].view(np.uint32))
    # the rows are the q-sample buffers of register_schedule, not the DDIM table's fp32 square roots
    sa, s1a = mr.qsample_buffers()
    ts = torch.as_tensor(fx["timesteps"])
    assert np.array_equal(fx["qcoef"][:, 0], sa[ts].numpy()) and np.array_equal(fx["qcoef"][:, 1], s1a[ts].numpy())
    dec = sch.coef_decode(0)
    assert np.allclose(dec["sa"], fx["qcoef"][:, 0], rtol=3e-7, atol=0) and np.allclose(dec["s1a"], fx["qcoef"][:, 1], rtol=3e-6, atol=0)
    assert not np.array_equal(dec["s1a"], fx["qcoef"][:, 1])  # and they do differ in the last bits on this schedule


def test_q_sample_formula_is_register_schedules():
    """the two-line formula the fixture generator hands the shim, against ddpm.py:271-274 written out on the buffers"""
    sa, s1a = mr.qsample_buffers()
    x, n = gu.rnd((2, 4, 16, 16), 1), gu.rnd((2, 4, 16, 16), 2)
    t = torch.tensor([21, 981])
    want = sa[t].view(2, 1, 1, 1) * x + s1a[t].view(2, 1, 1, 1) * n
    assert torch.equal(mr.q_sample(x, t, n), want)


def test_block_mean_latent_mask_equals_the_fixtures():
    fx = mr.load_fixture()
    px = torch.as_tensor(fx["mask_pixel"])
    assert torch.equal(px, mr.fixture_masks(2, 64))
    assert set(np.unique(fx["mask_pixel"][0])) == {0.0, 1.0} and 0 < fx["mask_pixel"][1].min() and fx["mask_pixel"][1].max() < 1
    from cycle_diffusion_amd.gan_wrapper.latent_text_wrapper import _LatentStochasticTextWrapper as W
    w = object.__new__(W)  # _latent_mask reads three attributes only
    torch.nn.Module.__init__(w)
    w._anchor = torch.nn.Parameter(torch.zeros(1))
    w.resolution, w.vae_factor = 64, 4
    lat = w._latent_mask(px, 2)
    assert lat.shape == (2, 1, 16, 16) and torch.equal(lat, torch.as_tensor(fx["mask_latent"]))
    assert 0 < lat[0].min() + 1 and ((lat[0] > 0) & (lat[0] < 1)).sum() == 0  # the rectangle sits on the 4-px grid
    for bad in (px[:, :, :32], px * 2.0, px[:1]):
        try:
            w._latent_mask(bad, 2)
        except ValueError:
            continue
        raise AssertionError("accepted a bad mask")


def test_triplets_read_an_optional_mask(tmp_path):
    from PIL import Image
    from cycle_diffusion_amd.data.triplets import TripletDataset, collate
    rng = np.random.RandomState(3)
    Image.fromarray(rng.randint(0, 255, (40, 48, 3), dtype=np.uint8)).save(tmp_path / "a.png")
    m = np.zeros((40, 48), dtype=np.uint8)
    m[:, 24:] = 255
    Image.fromarray(m).save(tmp_path / "m.png")
    rows = [{"img_path": "a.png", "encode_text": "a", "decode_text": "b", "mask_path": "m.png"},
            {"img_path": "a.png", "encode_text": "c", "decode_text": "d"}]
    (tmp_path / "d.json").write_text(json.dumps(rows))
    ds = TripletDataset(str(tmp_path / "d.json"), 32)
    both = collate([ds[0], ds[1]])
    assert both["mask"].shape == (2, 1, 32, 32) and both["has_mask"] == [True, False]
    assert float(both["mask"].min()) >= 0 and float(both["mask"].max()) == 1.0
    assert torch.equal(both["mask"][1], torch.zeros(1, 32, 32))
    # the same centre crop as the image: 40 x 40 around the centre, so the white half starts at the middle column
    assert torch.equal(both["mask"][0, 0, :, :12], torch.zeros(32, 12)) and torch.equal(both["mask"][0, 0, :, 20:], torch.ones(32, 12))
    none = collate([ds[1]])
    assert "mask" not in none and "has_mask" not in none
    assert sorted(none) == ["decode_text", "encode_text", "original_image", "sample_id"]


def test_new_symbols_in_header_ffi_and_library():
    txt = open(os.path.join(ROOT, "include", "cyclediff.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _ffi.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert s in _ffi.SIGNATURES and hasattr(lib, s), s
        n_args = len(re.search(r"\b%s\s*\((.*?)\)" % s, txt, flags=re.S).group(1).split(","))
        assert n_args == len(_ffi.SIGNATURES[s]), (s, n_args)
    # the coupled loop takes its keep-mask as an option struct of cd_cycle_translate: in the header and in _ffi with equal
    # fields (tests/test_abi.py holds their types and offsets to the header's)
    body = re.search(r"typedef\s+struct\s+cd_keep_mask\s*\{(.*?)\}\s*cd_keep_mask\s*;", txt, flags=re.S).group(1)
    names = [re.search(r"(\w+)$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert names == [f for f, _ in _ffi.KeepMask._fields_]
    assert names == ["mask", "x0", "B_mask", "source", "qsample_coef_host", "noise", "seed"]
    assert dict(_ffi.TranslateArgs._fields_)["mask"]._type_ is _ffi.KeepMask
    assert _ffi.MASK_SOURCES == {"q_sample": 0, "encoder": 1}
    assert "CD_MASK_QSAMPLE = 0" in txt and "CD_MASK_ENCODER = 1" in txt


def test_restatement_replays_the_reference_masked_decode():
    """tests/_masked_ref.masked_decode on the oracle's small U-Net against the reference's sample_with_eps(mask=, x0=), within
    the bound tests/test_oracle_golden.py holds the oracle's latent decode under CFG 3 to (atol 5e-3, rtol 1e-3)"""
    fx = mr.load_fixture()
    p = mr.params(fx)
    sd = br.synth_weights(json.loads(str(fx["unet_names"])), p["unet_seed"], p["out_prefix"], p["out_scale"])
    unet = lambda x, t, cc: nets.openai_unet(sd, gu.TINY_SD_CFG, x, t, cc)
    B, s = p["B"], p["ctx_seeds"]
    c_tgt, uc = gu.rnd((B, 77, 64), s[1]), gu.rnd((1, 77, 64), s[2]).expand(B, 77, 64).contiguous()
    sch = _sched(p)
    torch.manual_seed(p["mask_noise_seed"])
    mn = torch.stack([torch.randn(B, 4, 16, 16) for _ in range(p["S"])], 0)
    with torch.no_grad():
        x = mr.masked_decode(br.cfg_eps(unet, c_tgt, uc, p["dec_scale"]), torch.as_tensor(fx["sd_eps"]), sch.coef_decode(0),
                             sch.coef_qsample(0), torch.as_tensor(fx["mask_latent"]), torch.as_tensor(fx["sd_z0_mean"]), mn)
    ref = torch.as_tensor(fx["sd_x"])
    err = (x - ref).abs().max().item()
    assert torch.allclose(x, ref, atol=5e-3, rtol=1e-3), err
    assert float(fx["sd_mask_effect"]) > 50 * 5e-3  # the mask moves the latent far beyond that bound
