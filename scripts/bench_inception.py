"""Throughput of the FID Inception-v3 on the engine (cd_inception_features, csrc/inception.hip) on seeded synthetic weights;
prints ONE JSON line.

  python scripts/bench_inception.py [--batches 64 256] [--iters 10] [--no-torch]

Per batch size: the first call (which includes the autotuner's first look at the network's ~90 GEMM shapes at that batch
size) is timed on its own, then `iters` calls after warm-up with device events: images/s and algorithmic TFLOP/s (2 * M * N *
K of every convolution, FLOPs from the layer table below; the pools are not counted). The comparison is the same network as
a torch restatement (BatchNorm folded into the conv weights and bias, as on the engine) in fp16, channels_last, on the same
GPU - MIOpen / hipBLASLt convolutions. For the kernel split run it under `rocprofv3 --kernel-trace --stats -- python
scripts/bench_inception.py --no-torch --batches 256` in a run of its own.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def conv_flops_per_image():
    """2 * Hout * Wout * Cout * Cin * KH * KW summed over the 94 convolutions (stride / padding from the layer table)"""
    from cycle_diffusion_amd.engine import inception_fid_units
    # output spatial size of every unit: stem by name, blocks by their resolution (stride-2 units reduce to the next one)
    stem = {"Conv2d_1a_3x3": 149, "Conv2d_2a_3x3": 147, "Conv2d_2b_3x3": 147, "Conv2d_3b_1x1": 73, "Conv2d_4a_3x3": 71}
    s2 = {"Mixed_6a.branch3x3": 17, "Mixed_6a.branch3x3dbl_3": 17, "Mixed_7a.branch3x3_2": 8, "Mixed_7a.branch7x7x3_4": 8}
    res = {"Mixed_5": 35, "Mixed_6": 17, "Mixed_7a": 17, "Mixed_7b": 8, "Mixed_7c": 8}
    total = 0
    for name, cin, cout, (kh, kw) in inception_fid_units():
        if name in stem:
            hw = stem[name]
        elif name in s2:
            hw = s2[name]
        else:
            hw = next(v for k, v in res.items() if name.startswith(k))
        total += 2 * hw * hw * cout * cin * kh * kw
    return total


def time_calls(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    import cycle_diffusion_amd as cda
    flops = conv_flops_per_image()
    eng = cda.Engine("cuda:0")
    sd = cda.inception_synthetic_state_dict(0)
    net = eng.create_net(cda.inception_fid_desc())
    eng.load_inception_state_dict(net, sd)
    out = {"workload": "inception_fid_features", "conv_gflop_per_image": flops / 1e9,
           "act_format": "fp16" if eng.lib.cd_act_format() == 1 else "bf16", "engine": {}}
    g = torch.Generator().manual_seed(0)
    for B in a.batches:
        x = torch.tanh(F.interpolate(torch.randn(B, 3, 24, 24, generator=g), size=(299, 299), mode="bicubic")).cuda()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.inception_features(net, x)
        torch.cuda.synchronize()
        first_s = time.perf_counter() - t0
        for _ in range(a.warmup):
            eng.inception_features(net, x)
        ms = time_calls(lambda: eng.inception_features(net, x), a.iters)
        out["engine"][str(B)] = {"ms": ms, "images_per_s": B / ms * 1e3, "tflops": flops * B / ms / 1e9,
                                 "first_call_s": first_s}
    if not a.no_torch:
        import _inception_ref as ref

        def folded_conv(P, name, x, stride=1, padding=0):
            return F.relu(F.conv2d(x, P.get(name + ".conv.weight"), P.get(name + ".conv.bias"), stride=stride,
                                   padding=padding))
        ref._conv = folded_conv
        fsd = {}
        for name, *_ in cda.engine.inception_fid_units():
            sc = sd[name + ".bn.weight"] / torch.sqrt(sd[name + ".bn.running_var"] + 1e-3)
            fsd[name + ".conv.weight"] = (sd[name + ".conv.weight"] * sc.view(-1, 1, 1, 1)).half().cuda() \
                .to(memory_format=torch.channels_last)
            fsd[name + ".conv.bias"] = (sd[name + ".bn.bias"] - sd[name + ".bn.running_mean"] * sc).half().cuda()
        torch.backends.cudnn.benchmark = True
        out["torch_fp16_channels_last"] = {"label": "comparison: torch restatement, BN folded, fp16 channels_last"}
        for B in a.batches:
            x = torch.tanh(F.interpolate(torch.randn(B, 3, 24, 24, generator=g), size=(299, 299), mode="bicubic"))
            x = x.half().cuda().to(memory_format=torch.channels_last)
            with torch.no_grad():
                for _ in range(a.warmup):
                    ref.inception_fid_forward(fsd, x)
                ms = time_calls(lambda: ref.inception_fid_forward(fsd, x), a.iters)
            out["torch_fp16_channels_last"][str(B)] = {"ms": ms, "images_per_s": B / ms * 1e3,
                                                       "tflops": flops * B / ms / 1e9}
    out["device"] = torch.cuda.get_device_name(0)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
