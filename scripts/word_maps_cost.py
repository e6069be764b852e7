"""What the per-word attention maps cost: one cd_word_maps call on the C2 shapes (config/experiments/
bench_sd_c2.cfg, synthetic weights) at batch 4 and 4 draws - one forward of 16 rows with the map kernel beside all 16 text
cross-attentions - against four plain cd_unet_forward calls of 4 of those rows each. One process, interleaved, median of 3 after
a warm-up (the protocol of DESIGN.md 13).

  CYCLEDIFF_SYNTHETIC_WEIGHTS=1 python scripts/word_maps_cost.py out.json
"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out_path, batch=4, draws=4, reps=3):
    import cycle_diffusion_amd  # noqa: F401
    from cycle_diffusion_amd import auto_mask
    from cycle_diffusion_amd.gan_wrapper.get_gan_wrapper import get_gan_wrapper
    from cycle_diffusion_amd.utils.config_utils import get_config
    args = get_config("experiments/bench_sd_c2.cfg", config_root=os.path.join(ROOT, "config"))
    w = get_gan_wrapper(args.gan)
    eng = w.engine
    g = torch.Generator().manual_seed(0)
    x0 = torch.randn((batch, w.channels, w.image_size, w.image_size), generator=g).cuda()
    noise = torch.randn((draws,) + tuple(x0.shape), generator=g).cuda()
    c, _ = w.get_condition(["a photo of a dog"] * batch, batch)
    sel = torch.zeros(1, 1, c.shape[1]).cuda()
    sel[0, 0, 5] = 1.0
    sch = w._schedule()
    k = auto_mask.level_index(0.5, len(sch))
    qa, qb = (float(v) for v in sch.coef_qsample(0)[k])
    t = int(sch.coef_decode(0)["t"][k])
    rows = (qa * x0[None] + qb * noise).contiguous()  # [draws, batch, C, h, w]
    tv = torch.full((batch,), float(t)).cuda()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            fn()
        eng.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    n_layers = []
    maps = lambda: n_layers.append(eng.word_maps(w.unet, x0, c, sel, t, qa, qb, n_draws=draws, noise=noise)[1])
    plain = lambda: [eng.unet_forward(w.unet, rows[i], tv, c) for i in range(draws)]
    timed(maps)
    timed(plain)
    tm, tp = [], []
    for _ in range(reps):
        tm.append(timed(maps))
        tp.append(timed(plain))
    mm, mp = statistics.median(tm), statistics.median(tp)
    res = {"config": "bench_sd_c2.cfg", "batch": batch, "draws": draws, "words": 1, "n_layers": n_layers[0],
           "word_maps_s": tm, "plain_forwards_s": tp, "median_word_maps_s": mm, "median_plain_forwards_s": mp,
           "difference_s": mm - mp, "difference_percent": 100.0 * (mm - mp) / mp,
           "forward_rows": {"word_maps": [draws * batch], "plain": [batch] * draws}}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1])
