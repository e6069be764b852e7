"""Recorder behind tests/test_translate_calls_host.py: drives _LatentStochasticTextWrapper.translate() on a stand-in engine
and writes down, per configuration, every engine call it makes - method, argument names, shapes and a digest of every tensor
and table - the order of the noise draws, the result and `last_translate_coupled`. It touches the wrapper through translate()
and public attributes only, so the fixture (tests/golden/translate_calls.json) pins translate()'s host code whatever its
inner structure: `python tests/_translate_calls.py --write` regenerates it.

Nothing here draws from a torch generator and every value is the exact result of one IEEE operation on integers, so the
digests depend on neither torch's RNG nor the order of a reduction."""
import hashlib
import itertools
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cycle_diffusion_amd import auto_mask as am, schedule  # noqa: E402
from cycle_diffusion_amd.gan_wrapper.latent_text_wrapper import LatentMask, _LatentStochasticTextWrapper  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "translate_calls.json")
BSZ, CH, LAT, RES, FACTOR, STEPS, CTX_LEN, CTX_DIM = 3, 4, 2, 4, 2, 6, 8, 4
COUPLED = ("cycle_translate", "cycle_translate_masked", "cycle_translate_ctrl")


def ramp(shape, n, mod=257):
    """element i of the n-th tensor: ((i + 31 n) mod 257) / 257 - 0.5"""
    numel = int(np.prod(shape))
    return (((torch.arange(numel) + 31 * n) % mod).float() / mod - 0.5).reshape(shape)


def digest(v):
    """JSON-able record of one argument: tensors and numpy tables as (shape, sha1 of the float32 / raw bytes)"""
    if isinstance(v, torch.Tensor):
        return ["tensor", list(v.shape), hashlib.sha1(v.detach().cpu().float().contiguous().numpy().tobytes()).hexdigest()]
    if isinstance(v, np.ndarray):
        return ["table", list(v.shape), hashlib.sha1(np.ascontiguousarray(v).tobytes()).hexdigest()]
    if isinstance(v, (list, tuple)):
        return [digest(t) for t in v]
    if isinstance(v, (np.integer, np.floating)):
        return v.item()
    assert v is None or isinstance(v, (bool, int, float, str)), type(v)
    return v


class StandInEngine:
    """records (method, positional args, sorted kwargs); answers with a tensor of the right shape made from the call's index"""

    def __init__(self):
        self.calls = []

    def _rec(self, name, args, kw):
        self.calls.append([name, [digest(a) for a in args], [[k, digest(kw[k])] for k in sorted(kw)]])
        return len(self.calls)

    def vae_encode(self, *a, **kw):
        n = self._rec("vae_encode", a, kw)
        return ramp((a[1].shape[0], CH, a[1].shape[2] // FACTOR, a[1].shape[3] // FACTOR), 1000 + n)

    def vae_decode(self, *a, **kw):
        n = self._rec("vae_decode", a, kw)
        return ramp((a[1].shape[0], 3, a[1].shape[2] * FACTOR, a[1].shape[3] * FACTOR), 2000 + n) + 0.5

    def dpm_encode(self, *a, **kw):
        n = self._rec("dpm_encode", a, kw)
        return ramp((a[2].shape[0], len(a[3])) + tuple(a[2].shape[1:]), 3000 + n)

    def ddim_decode(self, *a, **kw):
        n = self._rec("ddim_decode", a, kw)
        return ramp((a[2].shape[0],) + tuple(a[2].shape[2:]), 4000 + n)

    def ddim_decode_masked(self, *a, **kw):
        n = self._rec("ddim_decode_masked", a, kw)
        return ramp((a[2].shape[0],) + tuple(a[2].shape[2:]), 5000 + n)

    def _coupled(self, name, a, kw):
        n = self._rec(name, a, kw)
        x0, n_dec = a[2], kw.get("n_dec", 1)
        return (ramp((x0.shape[0], len(a[3])) + tuple(x0.shape[1:]), 6000 + n),
                ramp((n_dec * x0.shape[0],) + tuple(x0.shape[1:]), 7000 + n))

    def cycle_translate(self, *a, **kw):
        return self._coupled("cycle_translate", a, kw)

    def cycle_translate_masked(self, *a, **kw):
        return self._coupled("cycle_translate_masked", a, kw)

    def cycle_translate_ctrl(self, *a, **kw):
        return self._coupled("cycle_translate_ctrl", a, kw)

    def automask(self, *a, **kw):
        n = self._rec("automask", a, kw)
        shape = (a[1].shape[0], 1) + tuple(a[1].shape[2:])
        return ((torch.arange(int(np.prod(shape))) + n) % 3 == 0).float().reshape(shape), ramp(shape, 8000 + n) + 0.5


class CondStage:
    """a pure function of the text: element i of a prompt's embedding is byte i of its sha256 chain, over 256"""
    length = CTX_LEN

    def __call__(self, texts):
        out = []
        for t in texts:
            raw, h = b"", t.encode("utf-8")
            while len(raw) < CTX_LEN * CTX_DIM:
                h = hashlib.sha256(h).digest()
                raw += h
            out.append(torch.tensor(list(raw[:CTX_LEN * CTX_DIM]), dtype=torch.float32).reshape(CTX_LEN, CTX_DIM) / 256)
        return torch.stack(out, 0)


def ranker(img, original_img, encode_text, decode_text):
    """a pure function of every image on its own, in integers: the argmax over candidates does not depend on a summation order"""
    return ((img.flatten(1) * 257).round().long() * torch.arange(1, img[0].numel() + 1)).sum(1).remainder(10007).float()


def make_wrapper(dec_scales, enc_scales, auto=None, **attrs):
    w = object.__new__(_LatentStochasticTextWrapper)
    torch.nn.Module.__init__(w)
    w.custom_steps, w.eta, w.channels, w.image_size, w.resolution, w.vae_factor = STEPS, 0.1, CH, LAT, RES, FACTOR
    w.n_trials, w.skip_steps, w.white_box_steps = 2, [0, 2], STEPS + 1
    w.encoder_unconditional_guidance_scales, w.decoder_unconditional_guidance_scales = enc_scales, dec_scales
    w.precision, w.noise_on_cpu, w.fold_ensemble = "fp16", False, True
    w.couple, w.couple_max_tokens, w.last_translate_coupled = True, w.COUPLE_MAX_TOKENS, "untouched"
    w.mask_source, w.cac_steps, w.cac_mode = "q_sample", 0.0, "refine"
    w.auto_mask_opts = am.AutoMaskOptions(auto, 10, 0.5, 3.0, 0.5, 0, 0)
    w.last_auto_mask = w.last_auto_map = None
    w.alphas_cumprod = schedule.latent_alphas_cumprod(1000, 0.00085, 0.0120)
    w.cond_stage, w.ranker, w.unet, w.vae = CondStage(), ranker, "unet", "vae"
    w._anchor = torch.nn.Parameter(torch.zeros(1))
    w.engine = StandInEngine()
    draws = []

    def noise_source(shape):
        draws.append(list(shape))
        return ramp(shape, len(draws))

    w.noise_source, w.draws = noise_source, draws
    for k, v in attrs.items():
        setattr(w, k, v)
    return w


def pixel_mask():
    """[B, 1, R, R] in quarters: the block mean of the first stage is exact"""
    return ((torch.arange(BSZ * RES * RES) * 3) % 5).float().reshape(BSZ, 1, RES, RES) / 4


def control(bsz=BSZ):
    return (ramp((bsz, CTX_LEN, CTX_LEN), 9001) + 0.5, ramp((bsz, CTX_LEN), 9002) + 0.5, ramp((bsz, CTX_LEN), 9003) + 1.5)


MODES = {  # name -> (wrapper attributes, auto_mask, with a mask)
    "plain": ({}, None, False),
    "mask": ({}, None, True),
    "mask_enc": ({"mask_source": "encoder"}, None, True),
    "ctrl": ({"cac_steps": 0.4}, None, False),
    "ctrl_mask": ({"cac_steps": 0.4}, None, True),
    "ctrl_mask_enc": ({"cac_steps": 0.4, "mask_source": "encoder"}, None, True),
    "auto": ({}, "diffedit", False),
}
CAPS = {"none": {}, "tokens40": {"couple_max_tokens": 40}, "fold6": {"MAX_FOLD": 6}, "wb5": {"white_box_steps": 5},
        "nocouple": {"couple": False}}
DEC_SCALES = {"d1": [1.0], "d23": [2.0, 3.0], "d12": [1.0, 2.0]}
ENC_SCALES = {"e1": [1.0], "e2": [2.0]}


def cases():
    """name -> (make_wrapper arguments, translate() keyword arguments as a thunk)"""
    out = {}
    for (dn, d), (en, e), (mn, (attrs, auto, masked)), (cn, cap) in itertools.product(
            DEC_SCALES.items(), ENC_SCALES.items(), MODES.items(), CAPS.items()):
        out["%s-%s-%s-%s" % (dn, en, mn, cn)] = (dict(dec_scales=d, enc_scales=e, auto=auto, **attrs, **cap),
                                                 (lambda masked=masked: {"mask": pixel_mask()} if masked else {}))
    guided, t40 = dict(dec_scales=[2.0, 3.0], enc_scales=[2.0]), {"couple_max_tokens": 40}
    latent = lambda: LatentMask(((torch.arange(BSZ * LAT * LAT) * 3) % 5).float().reshape(BSZ, 1, LAT, LAT) / 4)  # noqa: E731
    extra = {
        "x-attn_ctrl": (guided, lambda: {"attn_ctrl": control()}),
        "x-attn_ctrl-tokens40": (dict(guided, **t40), lambda: {"attn_ctrl": control()}),
        "x-attn_ctrl-mask-fold6": (dict(guided, MAX_FOLD=6), lambda: {"attn_ctrl": control(), "mask": pixel_mask()}),
        "x-attn_ctrl-auto": (dict(guided, auto="diffedit"), lambda: {"attn_ctrl": control()}),
        "x-attn_ctrl-wrong_batch": (guided, lambda: {"attn_ctrl": control(BSZ - 1)}),
        "x-latent_mask": (guided, lambda: {"mask": latent()}),
        "x-latent_mask-tokens40": (dict(guided, **t40), lambda: {"mask": latent()}),
        "x-latent_mask-enc-ctrl": (dict(guided, mask_source="encoder", cac_steps=0.4), lambda: {"mask": latent()}),
        "x-latent_mask-wrong_shape": (guided, lambda: {"mask": LatentMask(torch.zeros(BSZ, 1, RES, RES))}),
        "x-mask-wrong_shape": (guided, lambda: {"mask": torch.zeros(BSZ, 1, LAT, LAT)}),
        "x-mask-out_of_range": (guided, lambda: {"mask": pixel_mask() * 2}),
        "x-mask-out_of_range-ctrl": (dict(guided, cac_steps=0.4), lambda: {"mask": pixel_mask() - 0.5}),
        "x-mask-out_of_range-enc-wb5": (dict(guided, mask_source="encoder", white_box_steps=5),
                                        lambda: {"mask": pixel_mask() * 2}),
        "x-mask-out_of_range-ctrl-wb5": (dict(guided, cac_steps=0.4, white_box_steps=5), lambda: {"mask": pixel_mask() * 2}),
        "x-ctrl-dec0": (dict(dec_scales=[0.0], enc_scales=[1.0], cac_steps=0.4), lambda: {}),
        "x-ctrl-enc0": (dict(dec_scales=[2.0], enc_scales=[0.0], cac_steps=0.4), lambda: {}),
        "x-ctrl-replace": (dict(guided, cac_steps=1.0, cac_mode="replace"), lambda: {}),
        "x-dec0-dec0": (dict(dec_scales=[0.0, 0.0], enc_scales=[1.0]), lambda: {}),
        "x-d1235-fold6": (dict(dec_scales=[1.0, 2.0, 3.0, 5.0], enc_scales=[1.0, 2.0], MAX_FOLD=6), lambda: {}),
    }
    for mn, (attrs, auto, masked) in MODES.items():
        for cn in ("none", "tokens40"):
            extra["x-unfolded-%s-%s" % (mn, cn)] = (dict(guided, auto=auto, fold_ensemble=False, **attrs, **CAPS[cn]),
                                                    (lambda masked=masked: {"mask": pixel_mask()} if masked else {}))
    assert not set(extra) & set(out)
    out.update(extra)
    return out


def run_case(args, kwargs):
    """-> (summary for the fixture, full records)"""
    w = make_wrapper(**args)
    image = ramp((BSZ, 3, RES, RES), 0) + 0.5
    try:
        result = digest(w.translate(image, ["a photo of a cat", "a dog", "a red car"], ["a photo of a dog", "a cat", "a blue car"],
                                    **kwargs()))
    except Exception as e:  # the test holds the set of texts against the preconditions' own
        result = "%s: %s" % (type(e).__name__, e)
    full = {"result": result, "coupled": w.last_translate_coupled, "draws": w.draws, "calls": w.engine.calls}
    sha = hashlib.sha1(json.dumps(full, sort_keys=True).encode("utf-8")).hexdigest()
    return {"result": result, "coupled": w.last_translate_coupled, "methods": [c[0] for c in w.engine.calls], "sha1": sha}, full


def record():
    return {name: run_case(*c)[0] for name, c in cases().items()}


if __name__ == "__main__":
    rec = record()
    if "--write" in sys.argv:
        with open(FIXTURE, "w") as f:
            f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(rec[k], sort_keys=True)) for k in rec) + "\n}\n")
    done = [k for k in rec if isinstance(rec[k]["result"], list)]
    print("%d cases, %d complete, %d raise" % (len(rec), len(done), len(rec) - len(done)))
    for t in sorted({rec[k]["result"] for k in rec if k not in done}):
        print("  ", t[:150])
