"""CPU: the oracle restatement against the reference modules on seeds and inputs that differ from the other fixtures - the
fixtures pin the oracle everywhere, this reaches oracle branches no other fixture reaches (per-sample timesteps, batch > 1
VAE, a second draw of weights). The reference's outputs come from tests/golden/reference_second_draw.npz (oracle/gen_golden.py
--only records); where the reference tree is mounted with every module they need, from the live modules as well, and the
committed fixtures are re-run through it to catch one that has gone stale against the reference."""
import json

import pytest
import torch

import golden_util as gu
from oracle import gen_golden as gg
from oracle import nets, ref_import


def _close(a, b, atol=3e-5):
    b = torch.as_tensor(b)
    err = (a - b).abs().max().item()
    assert err < atol * max(1.0, b.abs().max().item()), err


def _oracle_outputs(fx):
    sd = lambda k: nets.synth_state_dict(json.loads(str(fx[k + "_names"])), int(fx[k + "_wseed"]))
    x, t, ctx = gu.rnd((3, 4, 16, 16), 31), torch.tensor([1, 501, 981]), gu.rnd((3, 77, 64), 32)
    yield "sd_y", nets.openai_unet(sd("sd"), gu.TINY_SD_CFG, x, t, ctx)
    x, t = gu.rnd((2, 3, 32, 32), 33), torch.tensor([999.0, 0.0])
    yield "iddpm_y", nets.openai_unet(sd("iddpm"), gu.TINY_IDDPM_CFG, x, t)
    img = torch.rand((3, 3, 64, 64), generator=torch.Generator().manual_seed(34)) * 2 - 1
    yield "vae_moments", nets.vae_encode_moments(sd("vae"), gu.TINY_VAE_CFG, img)
    yield "vae_decoded", nets.vae_decode(sd("vae"), gu.TINY_VAE_CFG, gu.rnd((3, 4, 16, 16), 35, 0.7))
    x, t = gu.rnd((2, 3, 32, 32), 36), torch.tensor([10.0, 870.0])
    yield "ho_y", nets.ho_unet(sd("ho"), gu.TOY_HO_CFG, x, t)
    x, t = gu.rnd((2, 3, 16, 16), 37), torch.tensor([3, 777])
    yield "ldm_uncond_y", nets.openai_unet(sd("ldm_uncond"), gu.TINY_LDM_UNCOND_CFG, x, t)


def test_networks_match_live_reference_modules():
    fx = gu.load("reference_second_draw")
    live = None
    if gg.reference_has(gg.SECOND_DRAW_FILES):
        with ref_import.session():
            live = gg.second_draw()
        assert all(live[k] == fx[k] for k in fx.files if k.endswith("_names"))  # the same weight tensors
    with torch.no_grad():
        for key, y in _oracle_outputs(fx):
            _close(y, fx[key])
            if live is not None:
                _close(y, live[key])


@pytest.mark.skipif(not ref_import.available(), reason="reference tree not mounted")
def test_committed_fixtures_still_match_the_reference():
    """re-run one network fixture and the schedule through the live reference: bit-for-bit what is committed"""
    import numpy as np
    fx = gu.load("unet_tiny_sd")
    with torch.no_grad():
        u = gg.build_ref_sd_unet()
        u.load_state_dict(nets.synth_state_dict(json.loads(str(fx["names"])), int(fx["wseed"])))
        u.eval()
        x, t, ctx = gu.tiny_sd_inputs()
        assert np.array_equal(u(x, t, context=ctx).numpy(), fx["y"])
