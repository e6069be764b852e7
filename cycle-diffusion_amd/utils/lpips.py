"""LPIPS v0.1 (Zhang et al. 2018, the `lpips` package's `LPIPS(net="alex" | "vgg")`) of image pairs on the engine
(csrc/lpips.hip, cd_lpips): how much of the source image an edit kept, as the editing papers report it.

  * weights: one full `lpips.LPIPS(net=...)` state_dict, or `backbone.pth,linear.pth` (a torchvision AlexNet / VGG16
    state_dict and the package's `weights/v0.1/{alex,vgg}.pth`), from `path` or CYCLEDIFF_LPIPS_WEIGHTS;
  * distance: both sides are PNG-quantised first, so the number is the one anyone gets from the written files.
Numerical parity with the `lpips` package itself needs its real weights, which are not in this tree.
"""
import os

import torch

from . import fid

SYNTHETIC_SEED = 13


def _read(path):
    sd = torch.load(path, map_location="cpu")
    if not isinstance(sd, dict):
        sd = sd.state_dict()
    return sd.get("state_dict", sd)


def load_lpips(engine, net="alex", path=None):
    """Create the LPIPS network `net` on `engine` and load its weights: `path` / CYCLEDIFF_LPIPS_WEIGHTS (one full state_dict,
    or `backbone.pth,linear.pth`), else the seeded synthetic weights when CYCLEDIFF_SYNTHETIC_WEIGHTS=1. Returns
    (net, weights_origin)."""
    from ..engine import lpips_desc, lpips_synthetic_state_dict
    from ..runtime import synthetic_allowed
    path = path or os.environ.get("CYCLEDIFF_LPIPS_WEIGHTS")
    if path:
        sd = {}
        for p in path.split(","):
            sd.update(_read(p.strip()))
        origin = "checkpoint:%s" % ",".join(os.path.basename(p.strip()) for p in path.split(","))
    elif synthetic_allowed():
        sd = lpips_synthetic_state_dict(net, SYNTHETIC_SEED)
        origin = "synthetic(seed=%d)" % SYNTHETIC_SEED
    else:
        raise FileNotFoundError("LPIPS needs its weights (a full lpips.LPIPS(net='%s') state_dict, or a torchvision backbone "
                                "state_dict and the package's linear file as backbone.pth,linear.pth): pass --lpips_weights "
                                "PATH[,PATH] or set CYCLEDIFF_LPIPS_WEIGHTS (or CYCLEDIFF_SYNTHETIC_WEIGHTS=1 for seeded "
                                "synthetic weights)" % net)
    nid = engine.create_net(lpips_desc(net))
    engine.load_lpips_state_dict(nid, sd)
    return nid, origin


def pairs_per_call(engine, net, H, W, batch):
    """How many pairs one cd_lpips call may take: `batch`, cut so that the arena's high-water (engine.lpips_pair_bytes per
    pair) stays inside half of the engine's workspace."""
    from ..engine import lpips_pair_bytes
    per = lpips_pair_bytes(engine._lpips_name(net), H, W)
    return int(max(1, min(batch, (engine.workspace_bytes // 2) // per)))


def to_signed(images):
    """[N, 3, H, W] in [0, 1] -> PNG-quantised ((x * 255 + 0.5) -> uint8, as main.py writes) -> fp32 in [-1, 1]"""
    u8 = torch.from_numpy(fid.quantise(images)).permute(0, 3, 1, 2)
    return u8.float() / 255.0 * 2.0 - 1.0


def distance_signed(engine, net, a, b, batch=16):
    """LPIPS of [N, 3, H, W] fp32 tensors already in [-1, 1], chunked: float64 numpy [N]"""
    assert a.shape == b.shape and a.dim() == 4, (a.shape, b.shape)
    n = pairs_per_call(engine, net, a.shape[2], a.shape[3], batch)
    out = []
    for i in range(0, a.shape[0], n):
        out.append(engine.lpips(net, a[i:i + n].to(engine.device, torch.float32).contiguous(),
                                b[i:i + n].to(engine.device, torch.float32).contiguous()).double().cpu())
    return torch.cat(out).numpy() if out else torch.zeros(0, dtype=torch.float64).numpy()


def distance(engine, net, a, b, batch=16):
    """LPIPS of the PNG-quantised pairs: a, b [N, 3, H, W] tensors in [0, 1] -> float64 numpy [N]"""
    return distance_signed(engine, net, to_signed(a), to_signed(b), batch)


def distance_keep(engine, net, a, b, keep, batch=16):
    """This project's masked variant: both PNG-quantised images are multiplied by the keep-mask ([N, 1, H, W], 1 = kept) in
    [-1, 1] space, so the edit region is the same mid-grey in both and only the kept region can differ."""
    m = (keep.detach().float().cpu() >= 0.5).float()
    return distance_signed(engine, net, to_signed(a) * m, to_signed(b) * m, batch)
