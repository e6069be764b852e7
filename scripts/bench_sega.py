"""What semantic guidance costs: translate() at batch 4 on the C2 shapes (config/experiments/bench_sd_c2.cfg, 99
steps, synthetic weights) with E = 0 / 1 / 2 edit concepts (the two of config/experiments/bench_sd_c2_sega.cfg). One process,
one wrapper, interleaved, median of 3 after a warm-up (the protocol of DESIGN.md 13). Per concept a step gains one decoder row
per sample in its forward, and with any concept the two launches of csrc/sega.hip and the loss of the shared
classifier-free-guidance prefix. Every translate() call runs under its own time limit: a call that exceeds it ends the process
with exit status 124 and a JSON line that says which one.

  CYCLEDIFF_SYNTHETIC_WEIGHTS=1 python scripts/bench_sega.py out.json
"""
import json
import os
import statistics
import sys
import threading
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALL_LIMIT_S = 120.0


def _limited(what, fn, limit=CALL_LIMIT_S):
    def expired():
        print(json.dumps({"error": "time limit", "call": what, "limit_s": limit}), flush=True)
        os._exit(124)
    t = threading.Timer(limit, expired)
    t.daemon = True
    t.start()
    try:
        return fn()
    finally:
        t.cancel()


def main(out_path, batch=4, reps=3):
    import cycle_diffusion_amd  # noqa: F401
    from cycle_diffusion_amd.gan_wrapper.get_gan_wrapper import get_gan_wrapper
    from cycle_diffusion_amd.semantic_guidance import parse_concepts
    from cycle_diffusion_amd.utils.config_utils import get_config
    root = os.path.join(ROOT, "config")
    w = get_gan_wrapper(get_config("experiments/bench_sd_c2.cfg", config_root=root).gan)
    two = parse_concepts(dict(iter(get_config("experiments/bench_sd_c2_sega.cfg", config_root=root).gan))["edit_concepts"])
    sets = {"E0": [], "E1": two[:1], "E2": two}
    image = torch.rand((batch, 3, w.resolution, w.resolution), generator=torch.Generator().manual_seed(0)).cuda()
    src, tgt = ["a photo of a man"] * batch, ["a photo of an old man"] * batch

    def timed(name):
        def call():
            torch.manual_seed(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                w.translate(image, src, tgt, edit_concepts=sets[name])
            w.engine.synchronize()
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        return _limited("translate %s" % name, call)

    for name in sets:
        timed(name)
    times = {k: [] for k in sets}
    for _ in range(reps):
        for name in sets:
            times[name].append(timed(name))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"config": "experiments/bench_sd_c2.cfg", "concepts": "experiments/bench_sd_c2_sega.cfg", "batch": batch,
           "steps": w.custom_steps, "rows_per_forward": {k: batch * (3 + len(v)) for k, v in sets.items()},
           "translate_s": times, "median_s": med,
           "ratio_to_E0": {k: med[k] / med["E0"] for k in sets},
           "growth_per_concept": {"E1": med["E1"] / med["E0"] - 1.0, "E2": (med["E2"] / med["E0"] - 1.0) / 2.0},
           "edited_share_synthetic_weights": float(w.last_edit_masks[0].mean())}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1])
