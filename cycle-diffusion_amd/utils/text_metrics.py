"""CLIP and directional CLIP of the reference's text evaluator (evaluation/translate_text.py:65-77): DirectionalCLIP
(model/energy/clean_clip.py) on the UNCLAMPED output against the original image with the batch's texts; the clamp to
[0, 1] comes only afterwards, for PSNR / SSIM. Both CLIP towers run on the engine (gan_wrapper/ranker.py)."""
import os

import torch


def make_ranker(engine, path=None):
    """DirectionalCLIPHIP with the ViT-B/32 state_dict from `path` / CYCLEDIFF_CLIP_RANKER, else seeded synthetic towers
    when CYCLEDIFF_SYNTHETIC_WEIGHTS=1 (the ranker's own rule, latent_text_wrapper.py)"""
    from ..gan_wrapper.ranker import DirectionalCLIPHIP
    from ..runtime import synthetic_allowed
    path = path or os.environ.get("CYCLEDIFF_CLIP_RANKER")
    sd = None
    if path:
        sd = torch.load(path, map_location="cpu")
        sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd.state_dict()
    elif not synthetic_allowed():
        raise FileNotFoundError("text metrics need the CLIP ViT-B/32 state_dict: set CYCLEDIFF_CLIP_RANKER (or "
                                "CYCLEDIFF_SYNTHETIC_WEIGHTS=1 for random towers)")
    return DirectionalCLIPHIP(engine, state_dict=sd, require_vocab=sd is not None)


def text_scores(ranker, img, original, encode_text, decode_text):
    """per-sample (clip, d-clip) lists of float: img / original [B, 3, H, W] as the model returned them (not clamped)"""
    clip, dclip = ranker(img, original, list(encode_text), list(decode_text))
    return [float(v) for v in clip.float().cpu()], [float(v) for v in dclip.float().cpu()]
