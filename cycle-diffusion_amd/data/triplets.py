"""(image, source text, target text) triplets for evaluation - the reference's DevDataset
(preprocess/translate_text512.py:41-83 over data/translate-text.json: a list of {"img_path", "encode_text",
"decode_text"}): CenterCropLongEdge -> Resize(resolution) -> ToTensor, one item per JSON entry in [start, end).
Unpaired (image-only) entries simply omit the two texts. An entry may carry a "mask_path": a grey image, white = keep the
source there (the wrappers' `mask=`), cropped and resized like the image."""
import json
import os

import numpy as np
import torch
from PIL import Image


def center_crop_long_edge(img):
    """utils/transform_utils.py CenterCropLongEdge: square crop of the short-edge size around the centre"""
    w, h = img.size
    s = min(w, h)
    left, top = int(round((w - s) / 2.0)), int(round((h - s) / 2.0))
    return img.crop((left, top, left + s, top + s))


def center_crop_aspect(img, H, W):
    """the largest centred rectangle of aspect H : W (integer arithmetic; a square H = W is center_crop_long_edge's crop)"""
    w, h = img.size
    if w * H >= h * W:  # too wide: keep the height
        cw, ch = max(1, (h * W) // H), h
    else:
        cw, ch = w, max(1, (w * H) // W)
    left, top = int(round((w - cw) / 2.0)), int(round((h - ch) / 2.0))
    return img.crop((left, top, left + cw, top + ch))


def _crop_resize(img, resolution):
    """resolution: an int (the reference's square: CenterCropLongEdge, Resize) or (H, W) (the largest centred rectangle of
    that aspect, then the same bilinear resize)"""
    if isinstance(resolution, (tuple, list)):
        H, W = int(resolution[0]), int(resolution[1])
        img = center_crop_aspect(img, H, W)
    else:
        H = W = int(resolution)
        img = center_crop_long_edge(img)
    if img.size != (W, H):
        img = img.resize((W, H), Image.BILINEAR)  # transforms.Resize default for PIL images
    return img


def load_image(path, resolution):
    """-> [3, R, R] for an int resolution, [3, H, W] for (H, W)"""
    img = _crop_resize(Image.open(path).convert("RGB"), resolution)  # utils/file_utils.pil_loader
    return torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0).permute(2, 0, 1).contiguous()  # ToTensor


def load_mask(path, resolution):
    """grey keep-mask -> [1, R, R] (or [1, H, W]) in [0, 1] (white = keep): the image's centre crop and bilinear resize"""
    img = _crop_resize(Image.open(path).convert("L"), resolution)
    return torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0)[None].contiguous()


class TripletDataset(torch.utils.data.Dataset):
    def __init__(self, json_path, resolution, start=0, end=None, root=None):
        with open(json_path) as fh:
            raw = json.load(fh)
        self.items = list(enumerate(raw))[start:end]
        self.resolution = resolution
        self.root = root if root is not None else os.path.dirname(os.path.abspath(json_path))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, index):
        idx, meta = self.items[index]
        path = meta["img_path"]
        if not os.path.isabs(path):
            path = os.path.join(self.root, path)
        item = {"sample_id": torch.tensor(idx, dtype=torch.long), "original_image": load_image(path, self.resolution)}
        for k in ("encode_text", "decode_text"):
            if k in meta:
                item[k] = meta[k]
        if "mask_path" in meta:
            mpath = meta["mask_path"]
            if not os.path.isabs(mpath):
                mpath = os.path.join(self.root, mpath)
            item["mask"] = load_mask(mpath, self.resolution)
        return item


def collate(items):
    out = {"sample_id": torch.stack([it["sample_id"] for it in items]),
           "original_image": torch.stack([it["original_image"] for it in items])}
    for k in ("encode_text", "decode_text"):
        if k in items[0]:
            out[k] = [it[k] for it in items]
    if any("mask" in it for it in items):  # a batch without any mask carries no `mask` key at all
        zero = torch.zeros((1,) + tuple(items[0]["original_image"].shape[1:]))
        out["mask"] = torch.stack([it.get("mask", zero) for it in items])
        out["has_mask"] = ["mask" in it for it in items]  # host-side bookkeeping: never handed to the model
    return out
