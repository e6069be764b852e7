"""What the local blend costs: translate() at batch 4 on the C2 shapes (config/experiments/bench_sd_c2_cac.cfg,
99 steps, synthetic weights) with `local_blend = words` (config/experiments/bench_sd_c2_localblend.cfg) against `none`. One
process, interleaved, median of 3 after a warm-up (the protocol of DESIGN.md 13). Per step the blend adds the map kernel and
the accumulate launch on two row ranges in each of the five 16 x 16 text cross-attentions, and one mask launch.

  CYCLEDIFF_SYNTHETIC_WEIGHTS=1 python scripts/local_blend_cost.py out.json
"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out_path, batch=4, reps=3):
    import cycle_diffusion_amd  # noqa: F401
    from cycle_diffusion_amd.gan_wrapper.get_gan_wrapper import get_gan_wrapper
    from cycle_diffusion_amd.utils.config_utils import get_config
    cfgs = {"none": "experiments/bench_sd_c2_cac.cfg", "words": "experiments/bench_sd_c2_localblend.cfg"}
    ws = {k: get_gan_wrapper(get_config(v, config_root=os.path.join(ROOT, "config")).gan) for k, v in cfgs.items()}
    image = torch.rand((batch, 3, ws["none"].resolution, ws["none"].resolution), generator=torch.Generator().manual_seed(0)).cuda()
    src, tgt = ["a photo of a cat on a sofa"] * batch, ["a photo of a dog on a sofa"] * batch

    def timed(w):
        torch.manual_seed(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            w.translate(image, src, tgt)
        w.engine.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for w in ws.values():
        timed(w)
    times = {k: [] for k in ws}
    for _ in range(reps):
        for k, w in ws.items():
            times[k].append(timed(w))
    med = {k: statistics.median(v) for k, v in times.items()}
    keep = ws["words"].last_local_blend_mask
    res = {"configs": cfgs, "batch": batch, "steps": ws["none"].custom_steps, "side": ws["words"].image_size // 4,
           "translate_s": times, "median_s": med, "difference_s": med["words"] - med["none"],
           "difference_percent": 100.0 * (med["words"] - med["none"]) / med["none"],
           "edit_fraction_synthetic_weights": float(1.0 - keep.mean())}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1])
