"""B = 16, 256 x 256, N = 32 on the AFHQ i-DDPM (fp32): 4 decode rows, 3 of them conditioned, explicit noise tensors"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import cycle_diffusion_amd as cda
from cycle_diffusion_amd import _ffi, schedule
eng = cda.Engine("cuda:0")
net = eng.create_net(cda.afhq_iddpm_desc(256, precision=_ffi.CD_PREC_F32))
eng.random_init(net, seed=1)
B, K = 16, 4
sch = schedule.PixelSchedule(1000, K, sample_type="ddim", eta=0.1)
g = torch.Generator().manual_seed(0)
z = torch.randn((B, 1, 3, 256, 256), generator=g).cuda()
y = (torch.rand((B, 3, 256, 256), generator=g) * 2 - 1).cuda()
nt = torch.randn((K, B, 3, 256, 256), generator=g).cuda()
rn = torch.randn((K, B, 3, 256, 256), generator=g).cuda()
for _ in range(2):
    x = eng.ilvr_decode(net, sch.kind, z, sch.coef_decode(), y, 32, sch.coef_ilvr(), range_t=0, noise_tail=nt, ref_noise=rn)
eng.synchronize()
print("finite", bool(torch.isfinite(x).all()))
t = torch.full((B,), 500.0).cuda()
ms = []
for _ in range(4):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); eng.unet_forward(net, z[:, 0].contiguous(), t); b.record(); torch.cuda.synchronize()
    ms.append(a.elapsed_time(b))
print("forward B=16 fp32 ms (events, 4 runs):", ["%.1f" % m for m in ms])
eng.close()
