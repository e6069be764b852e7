"""Throughput of LPIPS on the engine (cd_lpips, csrc/lpips.hip) on seeded synthetic weights; prints ONE JSON line.

  python scripts/bench_lpips.py [--sizes 256 512] [--pairs 16] [--iters 10] [--window_ms 300] [--repeats 3]

Per backbone (alex, vgg) and image size: the first call (which includes the autotuner's first look at the backbone's GEMM
shapes) is timed on its own; then, after warm-up, windows of at least `iters` calls and `window_ms` of device time are timed
with device events: pairs/s from the median of `repeats` windows, with their range. `lpips_layer_share` is the share of a call
that the five k_lpips_layer launches (and their finishing steps) take, from a second timing of the same 2 B images through the
backbone alone (cd_lpips_tap, tap 4): (t_lpips - t_backbone) / t_lpips. For the kernel split itself run it under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_lpips.py` in a run of its own.
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_calls(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def timed(fn, iters, window_ms, repeats):
    """ms per call: median and range of `repeats` windows of at least `iters` calls and about window_ms of device time"""
    n = max(iters, int(window_ms / max(time_calls(fn, iters), 1e-3)) + 1)
    ms = sorted(time_calls(fn, n) for _ in range(repeats))
    return ms[len(ms) // 2], ms[0], ms[-1], n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--pairs", type=int, default=16, help="pairs per call")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window_ms", type=float, default=300.0, help="least device time of a timed window")
    ap.add_argument("--repeats", type=int, default=3, help="timed windows per figure (median and range are printed)")
    a = ap.parse_args()
    import cycle_diffusion_amd as cda
    from cycle_diffusion_amd.engine import lpips_pair_bytes
    eng = cda.Engine("cuda:0")
    out = {"workload": "lpips", "pairs_per_call": a.pairs, "act_format": "fp16" if eng.lib.cd_act_format() == 1 else "bf16"}
    g = torch.Generator().manual_seed(0)
    for name in ("alex", "vgg"):
        net = eng.create_net(cda.lpips_desc(name))
        eng.load_lpips_state_dict(net, cda.lpips_synthetic_state_dict(name, 0))
        out[name] = {}
        for R in a.sizes:
            x0 = torch.tanh(F.interpolate(torch.randn(a.pairs, 3, 24, 24, generator=g), size=(R, R), mode="bicubic")).cuda()
            x1 = (x0 + 0.3 * torch.tanh(F.interpolate(torch.randn(a.pairs, 3, 24, 24, generator=g), size=(R, R),
                                                      mode="bicubic")).cuda()).clamp(-1, 1)
            both = torch.cat([x0, x1]).contiguous()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.lpips(net, x0, x1)
            torch.cuda.synchronize()
            first_s = time.perf_counter() - t0
            for _ in range(a.warmup):
                eng.lpips(net, x0, x1)
                eng.lpips_tap(net, both, 4)
            ms, lo, hi, n = timed(lambda: eng.lpips(net, x0, x1), a.iters, a.window_ms, a.repeats)
            ms_net, _, _, _ = timed(lambda: eng.lpips_tap(net, both, 4), a.iters, a.window_ms, a.repeats)
            out[name][str(R)] = {"ms": ms, "ms_min": lo, "ms_max": hi, "calls_per_window": n, "pairs_per_s": a.pairs / ms * 1e3,
                                 "backbone_ms": ms_net, "lpips_layer_share": max(0.0, (ms - ms_net) / ms),
                                 "first_call_s": first_s, "arena_mb_per_pair": lpips_pair_bytes(name, R, R) / 2 ** 20}
    out["device"] = torch.cuda.get_device_name(0)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
