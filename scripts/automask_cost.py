"""What `[gan] auto_mask = diffedit` costs: translate() at batch 4 on the C2 shapes (config/experiments/bench_sd_c2_diffedit.cfg,
99 steps, synthetic weights), the key on against the explicit-mask call with the mask it estimated - the same masked path, so
the difference is the estimate alone. One process, interleaved, median of 3 after a warm-up (the protocol of DESIGN.md 13).

  CYCLEDIFF_SYNTHETIC_WEIGHTS=1 python scripts/automask_cost.py out.json
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
    args = get_config("experiments/bench_sd_c2_diffedit.cfg", config_root=os.path.join(ROOT, "config"))
    w = get_gan_wrapper(args.gan)
    image = torch.rand((batch, 3, w.resolution, w.resolution), generator=torch.Generator().manual_seed(0)).cuda()
    src, tgt = ["a photo of a cat"] * batch, ["a photo of a dog"] * batch

    def timed(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            w.translate(image, src, tgt, **kw)
        w.engine.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    timed()  # warm-up of both calls; the explicit mask is the estimated one
    f = w.vae_factor
    mask = w.last_auto_mask.repeat_interleave(f, 2).repeat_interleave(f, 3)
    timed(mask=mask)
    auto, explicit = [], []
    for _ in range(reps):
        auto.append(timed())
        explicit.append(timed(mask=mask))
    ma, me = statistics.median(auto), statistics.median(explicit)
    o = w.auto_mask_opts
    res = {"config": "bench_sd_c2_diffedit.cfg", "batch": batch, "steps": w.custom_steps, "auto_mask_draws": o.draws,
           "mask_source": w.mask_source, "edit_fraction": float(1 - w.last_auto_mask.mean()),
           "auto_mask_s": auto, "explicit_mask_s": explicit, "median_auto_mask_s": ma, "median_explicit_mask_s": me,
           "estimate_s": ma - me, "overhead_percent": 100.0 * (ma - me) / me,
           "forward_rows": {"estimate": 2 * o.draws * batch, "translate": w.custom_steps * 3 * batch}}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1])
