"""FID and KID of the reference's unpaired evaluator (evaluation/translate_to_dog.py:81-88: clean-fid's `compute_fid` /
`compute_kid`, "clean" mode) with the Inception-v3 on the engine (csrc/inception.hip, cd_inception_features).

Host side, fp64 numpy / scipy, following clean-fid's formulas:
  * clean_resize: each channel of a uint8 HWC image as a PIL float ("F") image, bicubic to 299 x 299, clipped to [0, 255];
  * features: images -> (x - INCEPTION_SHIFT) / INCEPTION_SCALE -> pool3 [N, 2048] on the engine;
  * frechet_distance: |mu1 - mu2|^2 + tr(s1) + tr(s2) - 2 tr(sqrtm(s1 s2)) (retried with 1e-6 I added to both covariances
    when the square root is not finite);
  * kernel_distance: the unbiased MMD^2 of the polynomial kernel (x.y / d + 1)^3 averaged over random subsets - drawn from
    a SEEDED RandomState here (clean-fid draws from numpy's global generator).
Numerical parity with clean-fid itself needs its real Inception weights, which are not in this tree.
"""
import os

import numpy as np
import torch
from PIL import Image

# clean-fid's feature wrapper feeds the TF-ported Inception (x - 128) / 128 of the 0..255 resized image
INCEPTION_SHIFT = 128.0
INCEPTION_SCALE = 128.0
INCEPTION_RES = 299
SYNTHETIC_SEED = 11


def clean_resize(img_u8, size=INCEPTION_RES):
    """uint8 [H, W, 3] -> float32 [3, size, size] in [0, 255]: clean-fid's PIL bicubic resize, one float channel at a time."""
    img_u8 = np.asarray(img_u8)
    assert img_u8.ndim == 3 and img_u8.shape[2] == 3, img_u8.shape
    out = np.empty((3, size, size), dtype=np.float32)
    for c in range(3):
        ch = Image.fromarray(img_u8[:, :, c].astype(np.float32))  # a 2-D float32 array is a mode "F" image
        assert ch.mode == "F"
        out[c] = np.asarray(ch.resize((size, size), resample=Image.BICUBIC)).clip(0, 255)
    return out


def quantise(images):
    """[N, 3, H, W] tensor in [0, 1] -> uint8 [N, H, W, 3], rounded as the PNGs main.py writes ((x * 255 + 0.5) -> uint8)."""
    x = images.detach().float().clamp(0, 1).cpu().permute(0, 2, 3, 1).numpy()
    return (x * 255 + 0.5).astype(np.uint8)


def load_inception(engine, path=None):
    """Create the FID Inception-v3 on `engine` and load its weights: `path` / CYCLEDIFF_FID_INCEPTION (a pytorch-fid or
    clean-fid state_dict), else the seeded synthetic weights when CYCLEDIFF_SYNTHETIC_WEIGHTS=1. Returns
    (net, weights_origin)."""
    from ..engine import inception_fid_desc, inception_synthetic_state_dict
    from ..runtime import synthetic_allowed
    path = path or os.environ.get("CYCLEDIFF_FID_INCEPTION")
    if path:
        sd = torch.load(path, map_location="cpu")
        sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd.state_dict()
        origin = "checkpoint:%s" % os.path.basename(path)
    elif synthetic_allowed():
        sd = inception_synthetic_state_dict(SYNTHETIC_SEED)
        origin = "synthetic(seed=%d)" % SYNTHETIC_SEED
    else:
        raise FileNotFoundError("FID / KID need the Inception-v3 state_dict (pytorch-fid pt_inception-2015-12-05-*.pth): pass "
                                "--fid_inception PATH or set CYCLEDIFF_FID_INCEPTION (or CYCLEDIFF_SYNTHETIC_WEIGHTS=1 for "
                                "seeded synthetic weights)")
    net = engine.create_net(inception_fid_desc())
    engine.load_inception_state_dict(net, sd)
    return net, origin


def features_u8(engine, net, images_u8, batch=64):
    """uint8 [N, H, W, 3] (a sequence of HWC arrays) -> pool3 features float64 [N, 2048]"""
    feats = []
    for i in range(0, len(images_u8), batch):
        x = np.stack([clean_resize(im) for im in images_u8[i:i + batch]])
        x = torch.from_numpy((x - INCEPTION_SHIFT) / INCEPTION_SCALE).to(engine.device)
        feats.append(engine.inception_features(net, x).double().cpu().numpy())
    return np.concatenate(feats, 0) if feats else np.zeros((0, 2048))


def features(engine, net, images, batch=64):
    """[N, 3, H, W] tensor in [0, 1] -> pool3 features float64 [N, 2048] of the PNG-quantised images"""
    return features_u8(engine, net, quantise(images), batch)


def statistics(feats):
    feats = np.asarray(feats, dtype=np.float64)
    return feats.mean(0), np.cov(feats, rowvar=False)


def frechet_distance(mu1, s1, mu2, s2, eps=1e-6):
    """(FID, largest |imaginary part| of sqrtm(s1 s2) dropped). All fp64."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, np.float64)), np.atleast_1d(np.asarray(mu2, np.float64))
    s1, s2 = np.atleast_2d(np.asarray(s1, np.float64)), np.atleast_2d(np.asarray(s2, np.float64))
    diff = mu1 - mu2
    covmean = linalg.sqrtm(s1.dot(s2))
    if not np.isfinite(covmean).all():
        off = np.eye(s1.shape[0]) * eps
        covmean = linalg.sqrtm((s1 + off).dot(s2 + off))
    imag = float(np.abs(covmean.imag).max()) if np.iscomplexobj(covmean) else 0.0
    covmean = covmean.real
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2.0 * np.trace(covmean)), imag


def kernel_distance(f1, f2, num_subsets=100, max_subset_size=1000, seed=0):
    """KID: unbiased MMD^2 of k(x, y) = (x.y / d + 1)^3 over `num_subsets` random subsets of m = min(N1, N2, max) rows"""
    f1, f2 = np.asarray(f1, np.float64), np.asarray(f2, np.float64)
    rng = np.random.RandomState(seed)
    d = f1.shape[1]
    m = min(f1.shape[0], f2.shape[0], max_subset_size)
    t = 0.0
    for _ in range(num_subsets):
        x = f2[rng.choice(f2.shape[0], m, replace=False)]
        y = f1[rng.choice(f1.shape[0], m, replace=False)]
        a = (x @ x.T / d + 1) ** 3 + (y @ y.T / d + 1) ** 3
        b = (x @ y.T / d + 1) ** 3
        t += (a.sum() - np.diag(a).sum()) / (m - 1) - b.sum() * 2 / m
    return float(t / num_subsets / m)


def fid_kid(gen_feats, ref_feats, seed=0):
    """{fid, kid, fid_sqrtm_imag, n_gen, n_ref} of two feature sets"""
    mu1, s1 = statistics(gen_feats)
    mu2, s2 = statistics(ref_feats)
    fid, imag = frechet_distance(mu1, s1, mu2, s2)
    kid = kernel_distance(gen_feats, ref_feats, seed=seed)
    return {"fid": fid, "kid": kid, "fid_sqrtm_imag": imag, "n_gen": int(len(gen_feats)), "n_ref": int(len(ref_feats))}


def list_images(root):
    """png / jpg files under `root`, recursively, sorted"""
    out = []
    for d, _, files in os.walk(root):
        out += [os.path.join(d, f) for f in files if f.lower().endswith((".png", ".jpg", ".jpeg"))]
    return sorted(out)


def load_reference_images(root, resolution):
    """the target-domain test set as uint8 HWC arrays, resized with PIL bilinear to `resolution` where the size differs
    (translate_to_dog.py:20-21, 51-56: 512 -> 256)"""
    ims = []
    for p in list_images(root):
        im = Image.open(p).convert("RGB")
        if im.size != (resolution, resolution):
            im = im.resize((resolution, resolution), resample=Image.BILINEAR)
        ims.append(np.asarray(im, dtype=np.uint8))
    return ims
