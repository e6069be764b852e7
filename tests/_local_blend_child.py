"""Child process of tests/test_gpu_local_blend.py (not collected): the U-Net reads CYCLEDIFF_CFG_SHARE once per process, so the
blended loop without the shared classifier-free-guidance prefix needs a process of its own.

    python _local_blend_child.py OUT.npz

runs the parent's call (the fixture of tests/_local_blend_ref.py under three controlled iterations) on the same inputs and
writes z, x, acc and keep. It checks nothing: the parent does."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import _attn_control_ref as acr  # noqa: E402
import _local_blend_ref as lbr  # noqa: E402
import golden_util as gu  # noqa: E402
from cycle_diffusion_amd import _ffi, schedule  # noqa: E402


def main(out_path):
    import cycle_diffusion_amd as cda
    from test_gpu_models import _load, tiny_sd_desc
    eng = cda.Engine("cuda:0")
    e = lbr.E2E
    net, _sd = _load(eng, tiny_sd_desc(), gu.load("latent_cycle_tiny"))
    x0, c, uc, c2 = acr.e2e_inputs()
    K = e["S"] - e["skip"]
    noise = torch.stack(gu.latent_noise(e["noise_seed"], x0.shape, K), 0)
    sch = schedule.DDIMSchedule(schedule.latent_alphas_cumprod(), e["S"], e["eta"])
    z, x, acc, keep = eng.cycle_translate_blend(
        net, _ffi.CD_SCHED_DDIM, x0.cuda(), sch.coef_encode(e["skip"]), sch.coef_decode(e["skip"]), lbr.key_selector(e["keys_src"]),
        lbr.key_selector(e["keys_tgt"]), e["side"], pool=e["pool"], thr=e["thr"], n_start=e["n_start"],
        ctrl=acr.e2e_control() + (3,), enc_ctx_c=c.cuda(), enc_ctx_uc=uc.cuda(), enc_guidance=1.0, dec_ctx_c=c2.cuda(),
        dec_ctx_uc=uc.cuda(), dec_guidance=e["dec_g"], noise=noise.cuda())
    eng.synchronize()
    np.savez(out_path, z=z.cpu().numpy(), x=x.cpu().numpy(), acc=acc.cpu().numpy(), keep=keep.cpu().numpy())
    eng.close()


if __name__ == "__main__":
    main(sys.argv[1])
