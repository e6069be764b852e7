"""References for the single-kernel tests of the fp32 execution path: tests/test_f32_path_host.py (CPU) and
tests/test_gpu_f32_ops.py (GPU, through cd_op_conv2d_prec / cd_op_attention_prec / cd_op_rows_prec / cd_op_resample_prec).

For every kernel family, in plain torch on the host:
  * a float64 reference on the fp32 operands;
  * an fp32 emulation of the kernel's documented arithmetic - for the GEMM-like kernels (k_conv_f32, the three-term split GEMM,
    the attention kernels) with the accumulation in the kernel's order: k ascending, sequential, one fused multiply-add per
    term (a float64 product-and-sum rounded to fp32). torch.matmul / F.conv2d in fp32 sum in blocks and are 3-5 x closer to
    float64 than a sequential chain of the same length, so they would set a bound that a correct kernel misses;
  * the tolerance, per element |got - ref64| <= tol:
      fp32 kernels     max(F32_FACTOR x max|emulation - ref64|, 2^-22 max|ref64|)                            (tol_f32)
      split conv       F32_FACTOR x max|emulation - ref64| + 2^-21 |alpha| (|x| conv |w|)                    (conv_tol)
      split outputs    + 2^-21 |ref64| for the fp16 pair of an output written in split form
      split_rows, avgpool2_split   2^-21 |ref| + 2^-28       (pair_tol: two 11-bit halves, absolute floor below 2^-6)
      avgpool2_f32     2 ulp of the float64 result on POSITIVE operands: three fp32 additions of same-sign terms err by at most
                       1.5 ulp of the sum, and the sum / 4 is exact. (With mixed signs the partial sums can exceed the result
                       and no ulp bound of the result holds for a correct kernel, so the pool cases use |x| + 0.1.)
      upsample2_f32    bit-exact
  * operands where a wrong index moves the result by O(1): every image, channel and filter tap has its own offset and scale, the
    weights are not symmetric across taps, q / k / v differ per head; the entry points put NaN into every padding column;
  * mutants - subtly wrong kernels evaluated on the host - that the host test shows to be >= 5 tolerances away.

F32_FACTOR = 4 is the project's fp32 convention (tests/_groupnorm_ref.py tol32). Over the order-faithful emulation it covers what
nobody has measured: how v_mfma_f32_32x32x2_f32 rounds inside its two-term step, and expf / exp2f / erff against torch's.
Observed on MI355X (largest err / tol per family over the rows f32op/... of the parity report; no family needed more than 4):
  k_conv_f32 0.25 | split conv 0.19, its statistics 0.06, forced tiles 0.05, conv -> GroupNorm fold 0.19
  k_flash_f32 0.32 (split output 0.26) | k_attention_f32 0.24 | k_layernorm_f32 0.25 (split 0.24) | k_geglu_f32 0.18 (split 0.13)
  raw-GEGLU conv -> GEGLU 0.25 (split 0.07) | k_split_rows_f32 0.45 | k_avgpool2_f32 0.75 (of 2 ulp) | k_upsample2_f32 exact
"""
import functools
import math

import torch
import torch.nn.functional as F

from _groupnorm_ref import _seed, make_x

F32_FACTOR = 4.0
ACT_SCALE, WGT_SCALE = 16.0, 256.0  # csrc/kernels.h kX3ActScale, kX3WgtScale
LOG2E = 1.44269504088896340736


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def fma32(a, b, c):
    """fp32(a * b + c) with one rounding: the product of two fp32 values is exact in float64"""
    return (a.double() * b.double() + c.double()).float()


def tol_f32(ref, emu_err, split=False):
    """emu_err: max|fp32 evaluation - ref| on the same operands"""
    t = torch.full_like(ref, max(F32_FACTOR * emu_err, 2.0 ** -22 * ref.abs().max().item()))
    return t + 2.0 ** -21 * ref.abs() if split else t


def pair_tol(ref):
    return 2.0 ** -21 * ref.abs() + 2.0 ** -28


def ulp32(ref):
    """spacing of fp32 at |ref| (float64 tensor, ref != 0)"""
    return 2.0 ** (torch.floor(torch.log2(ref.abs())) - 23)


def split_pair(x, scale):
    """the kernels' split_f16: hi = fp16(scale x), lo = fp16(scale x - hi) (exact difference) -> float64 hi, lo (scaled)"""
    v = (x.float() * scale).clamp(-65504.0, 65504.0)
    hi = v.to(torch.float16).float()
    lo = (v - hi).to(torch.float16).float()
    return hi.double(), lo.double()


def decode(x, scale=ACT_SCALE):
    hi, lo = split_pair(x, scale)
    return (hi + lo) / scale


# ==================================================================================================== convolution
def _cc(name, B, C0, H, W, N, k, **kw):
    d = dict(name=name, B=B, C0=C0, C1=0, H=H, W=W, N=N, k=k, stride=1, pad=k // 2, asym=False, up=False, pad0=0, pad1=0,
             bias=False, rowvec=None, act=0, resid=None, alpha=1.0, prec=(1,), via_split_rows=False, stats=False, geglu=False,
             x_range=None, w_range=None)
    d.update(kw)
    return d


_EPI = dict(bias=True, rowvec="img", resid=4, alpha=0.7)
_GEOM = [("s2p1", dict(stride=2)), ("s2asym", dict(stride=2, asym=True)), ("up", dict(up=True)), ("cin3", dict(C0=3))]

CONV_CASES = [
    # ---- k_conv_f32 <64,64>: M = 105 and 64, N below / above one 32-column MFMA block and one 64-column tile, nk = 2 and 54
    _cc("m105_n3_1x1_k32", 3, 32, 5, 7, 3, 1),
    _cc("m105_n6_3x3_k864", 3, 96, 5, 7, 6, 3, **_EPI),
    _cc("m105_n70_3x3_k864", 3, 96, 5, 7, 70, 3, act=1, **_EPI),
    _cc("m64_n64_1x1_k32", 1, 32, 8, 8, 64, 1),
    _cc("m64_n70_3x3", 1, 32, 8, 8, 70, 3, bias=True),
    # ---- <128,64>: ceil(8281 / 128) * ceil(200 / 64) = 260 tiles, M % 128 = 89, N % 64 = 8
    _cc("big_m8281_n200_3x3", 1, 32, 91, 91, 200, 3, bias=True, rowvec="shared"),
    # ---- the tile switch: 2 x 4096 rows, N = 256 -> 256 big tiles -> <128,64>; one image alone: 128 -> <64,64>
    _cc("tile_switch_64x64_n256", 2, 32, 64, 64, 256, 1, bias=True),
    # ---- concat 32 + 64 with different padded strides
    _cc("concat32+64_pads", 3, 32, 5, 7, 70, 3, C1=64, pad0=4, pad1=8, prec=(1, 2), **_EPI),
    # ---- the epilogue pieces alone
    _cc("epi_bias", 3, 32, 5, 7, 70, 3, bias=True),
    _cc("epi_rowvec_img", 3, 32, 5, 7, 70, 3, rowvec="img", prec=(1, 2)),
    _cc("epi_rowvec_shared", 3, 32, 5, 7, 70, 3, rowvec="shared", prec=(1, 2)),
    _cc("epi_silu", 3, 32, 5, 7, 70, 3, act=1),
    _cc("epi_gelu", 3, 32, 5, 7, 70, 3, act=2),
    _cc("epi_resid_pad3", 3, 32, 5, 7, 70, 3, resid=3, prec=(1, 2)),
    _cc("epi_alpha", 3, 32, 5, 7, 70, 3, alpha=-1.3, prec=(1, 2)),
]
# ---- geometry: stride 2 pad 1, stride 2 asymmetric, folded x2 upsample at 5 x 6, Cin = 3 padded to 32 - both precisions, 3x3 and 1x1
for _k in (3, 1):
    for _n, _kw in _GEOM:
        _d = dict(C0=32, bias=True, prec=(1, 2), pad=1 if _k == 3 else 0)
        _d.update(_kw)
        _C0 = _d.pop("C0")
        CONV_CASES.append(_cc("geom_%s_%dx%d" % (_n, _k, _k), 2, _C0, 5 if _n == "up" else 6, 6 if _n == "up" else 8, 70, _k, **_d))
CONV_CASES += [
    # ---- split GEMM: nvalid < 8 (N = 3, 6, 70), element-wise stores (N % 4 != 0), element-wise residual (stride 73, and 97 with nvalid = 8)
    _cc("split_n3", 3, 32, 5, 7, 3, 3, prec=(2,), **_EPI),
    _cc("split_n6_resid_pad1", 3, 32, 5, 7, 6, 1, prec=(2,), bias=True, resid=1),
    _cc("split_n70_resid_pad3", 3, 64, 5, 7, 70, 3, prec=(2,), bias=True, rowvec="img", resid=3),
    _cc("split_n96_resid_pad1", 3, 32, 5, 7, 96, 3, prec=(2,), bias=True, resid=1, alpha=0.7),
    _cc("split_n96_k2880", 2, 320, 4, 4, 96, 3, prec=(2,), bias=True),
    # ---- statistics of an fp32 output: Hout * Wout % 32 == 0 (and none at 5 x 7: test_split_conv_no_statistics)
    _cc("split_stats_n96", 2, 32, 8, 8, 96, 3, prec=(2,), stats=True, bias=True, resid=0),
    _cc("split_stats_n70_resid", 2, 32, 8, 8, 70, 3, prec=(2,), stats=True, resid=3, rowvec="img"),
    _cc("split_stats_1x1", 2, 64, 8, 4, 96, 1, prec=(2,), stats=True),
    # ---- forced tile configurations (test_split_conv_tile_configurations)
    _cc("split_tiles_c64_n96", 2, 64, 8, 8, 96, 3, prec=(2,), stats=True, bias=True, resid=0),
    # ---- two sources through split_rows, one source through split_rows
    _cc("split_rows_32+64", 2, 32, 8, 8, 70, 3, C1=64, pad0=8, pad1=4, prec=(2,), via_split_rows=True, bias=True),
    _cc("split_rows_one", 2, 32, 5, 7, 70, 1, pad0=4, prec=(2,), via_split_rows=True),
    # ---- the documented ranges: activations 2^-10 .. 2^10, weights 2^-12 .. 2^6
    _cc("split_ranges", 2, 32, 5, 7, 70, 3, prec=(2,), x_range=(-10, 10), w_range=(-12, 6)),
]
CONV_BY_NAME = {c["name"]: c for c in CONV_CASES}
assert len(CONV_BY_NAME) == len(CONV_CASES)
# forced configurations of the split GEMM, from the shipped tile table (tests/_gemm_sweep.py table_triples): (tile, bk32, split)
SPLIT_TILE_CONFIGS = [(18, 0, 1), (8, 0, 3)]  # a 16-wave tile (256x128 w4x4), a split-K entry (64x64, 3 ranges)


def _log_uniform(gen, shape, lo, hi):
    """random signs, magnitudes 2^lo .. 2^hi log-uniformly, the two ends present"""
    e = lo + (hi - lo) * torch.rand(shape, generator=gen)
    v = torch.pow(2.0, e) * (torch.randint(0, 2, shape, generator=gen) * 2.0 - 1.0)
    flat = v.reshape(-1)
    flat[0], flat[1] = 2.0 ** lo, -(2.0 ** hi)
    return v.float()


def make_w(gen, N, Cin, k):
    """every filter tap its own scale and offset (not symmetric across taps), every output channel its own scale"""
    K = Cin * k * k
    t = torch.arange(k * k, dtype=torch.float32).reshape(1, 1, k, k)
    scale = 0.6 + 0.15 * t
    off = 0.25 * (1.0 + t) * (1.0 - 2.0 * (t % 2)) / K
    rows = (0.7 + 0.6 * torch.rand(N, generator=gen))[:, None, None, None]
    return (rows * (scale * torch.randn(N, Cin, k, k, generator=gen) / math.sqrt(K) + off)).float()


def conv_out_hw(c):
    Hin, Win = (2 * c["H"], 2 * c["W"]) if c["up"] else (c["H"], c["W"])
    k, s = c["k"], c["stride"]
    if c["asym"]:
        return (Hin + 1 - k) // s + 1, (Win + 1 - k) // s + 1
    return (Hin + 2 * c["pad"] - k) // s + 1, (Win + 2 * c["pad"] - k) // s + 1


def im2col(x, c):
    """[B, C, H, W] -> [M, k*k, C] in the kernels' K order (tap-major, channels of the concat inside a tap), same dtype"""
    if c["up"]:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    k = c["k"]
    if c["asym"]:
        x = F.pad(x, (0, 1, 0, 1))
        cols = F.unfold(x, k, stride=c["stride"])
    else:
        cols = F.unfold(x, k, padding=c["pad"], stride=c["stride"])
    B, Cc = x.shape[:2]
    return cols.reshape(B, Cc, k * k, -1).permute(0, 3, 2, 1).reshape(-1, k * k, Cc)


def _act64(v, act):
    if act == 1:
        return v * torch.sigmoid(v)
    if act == 2:
        return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    return v


def conv_epilogue(acc, o, dtype, rowvec_shift=0):
    """act(alpha acc + bias + rowvec) + resid in `dtype`, in the kernels' order; acc [M, N] -> [B, N, Ho, Wo]"""
    c = o["case"]
    B, N = c["B"], c["N"]
    Ho, Wo = conv_out_hw(c)
    v = acc.to(dtype) * torch.tensor(c["alpha"], dtype=torch.float32).to(dtype)
    if o["bias"] is not None:
        v = v + o["bias"].to(dtype)[None]
    if o["rowvec"] is not None:
        rv = o["rowvec"].to(dtype)
        if rv.dim() == 2:
            rv = rv.roll(rowvec_shift, 0).repeat_interleave(Ho * Wo, 0)
        v = v + rv
    if dtype == torch.float64:
        v = _act64(v, c["act"])
    elif c["act"] == 1:
        v = v / (1.0 + torch.exp(-v))
    elif c["act"] == 2:
        v = F.gelu(v)
    v = v.reshape(B, Ho, Wo, N).permute(0, 3, 1, 2)
    if o["resid"] is not None:
        v = v + o["resid"].to(dtype)
    return v.contiguous()


def seq_gemm32(A, Wt):
    """[M, K] x [N, K] -> [M, N], k ascending, sequential, one fp32 fused multiply-add per term"""
    acc = torch.zeros(A.shape[0], Wt.shape[0], dtype=torch.float32)
    A, Wt = A.double(), Wt.double()
    for kk in range(A.shape[1]):
        acc = (A[:, kk, None] * Wt[None, :, kk] + acc.double()).float()
    return acc


def split_terms(A, Wm, drop_hi_wl=False, lo_from_rounded=False):
    """operands of the three-term GEMM in its K order: per tap [hi | lo | hi] x [wh | wh | wl]; A [M, T, C], Wm [N, T, C]"""
    hi, lo = split_pair(A, ACT_SCALE)
    if lo_from_rounded:  # mutant: lo = fp16(fp16(16 x) - hi) = 0
        lo = torch.zeros_like(lo)
    wh, wl = split_pair(Wm, WGT_SCALE)
    if drop_hi_wl:
        wl = torch.zeros_like(wl)
    a3 = torch.cat([hi, lo, hi], 2).reshape(A.shape[0], -1)
    w3 = torch.cat([wh, wh, wl], 2).reshape(Wm.shape[0], -1)
    return a3, w3


@functools.lru_cache(maxsize=None)
def conv_operands(name):
    c = CONV_BY_NAME[name]
    gen = torch.Generator().manual_seed(_seed("f32op/conv/" + name))
    B, C0, C1, H, W, N, k = (c[x] for x in ("B", "C0", "C1", "H", "W", "N", "k"))
    Ho, Wo = conv_out_hw(c)
    if c["x_range"]:
        x = _log_uniform(gen, (B, C0 + C1, H, W), *c["x_range"])
    else:
        x = make_x(gen, B, C0 + C1, H, W).float()
    w = _log_uniform(gen, (N, C0 + C1, k, k), *c["w_range"]) if c["w_range"] else make_w(gen, N, C0 + C1, k)
    o = dict(case=c, x=x, x0=x[:, :C0].contiguous(), x1=x[:, C0:].contiguous() if C1 else None, w=w)
    o["bias"] = (0.5 * torch.randn(N, generator=gen)).float() if c["bias"] else None
    o["rowvec"] = None
    if c["rowvec"] == "img":  # every image its own row, far apart
        o["rowvec"] = (torch.randn(B, N, generator=gen) + 2.0 * torch.arange(B)[:, None]).float()
    elif c["rowvec"] == "shared":
        o["rowvec"] = torch.randn(N, generator=gen).float()
    o["resid"] = make_x(gen, B, N, Ho, Wo).float() if c["resid"] is not None else None
    return o


@functools.lru_cache(maxsize=None)
def conv_build(name):
    """operands + float64 reference, the fp32 / split emulations' errors and the tolerances of the case's precisions"""
    o = dict(conv_operands(name))
    c = o["case"]
    A = im2col(o["x"].double(), c)                                     # [M, T, C]
    Wm = o["w"].double().permute(0, 2, 3, 1).reshape(c["N"], c["k"] ** 2, -1)  # [N, T, C]
    Af, Wf = A.reshape(A.shape[0], -1), Wm.reshape(c["N"], -1)
    o["A"], o["Wm"] = A, Wm
    o["ref"] = conv_epilogue(Af @ Wf.T, o, torch.float64)
    o["absconv"] = (abs(c["alpha"]) * (Af.abs() @ Wf.abs().T)).reshape(c["B"], *conv_out_hw(c), c["N"]).permute(0, 3, 1, 2)
    o["tol"], o["emu"] = {}, {}
    if 1 in c["prec"]:
        emu = conv_epilogue(seq_gemm32(Af, Wf), o, torch.float32)
        o["emu"][1] = emu
        o["tol"][1] = tol_f32(o["ref"], (emu.double() - o["ref"]).abs().max().item())
    if 2 in c["prec"]:
        o["emu"][2] = emu = conv_emulate_split(o)
        o["tol"][2] = conv_tol_split(o, emu)
    return o


def conv_emulate_split(o, **mut):
    a3, w3 = split_terms(o["A"], o["Wm"], **mut)
    acc = seq_gemm32(a3, w3)
    oo = dict(o)
    oo["case"] = dict(o["case"], alpha=f32(o["case"]["alpha"] * f32(1.0 / (ACT_SCALE * WGT_SCALE))))
    return conv_epilogue(acc, oo, torch.float32)


def conv_tol_split(o, emu):
    return F32_FACTOR * (emu.double() - o["ref"]).abs().max().item() + 2.0 ** -21 * o["absconv"]


def conv_call_args(o, precision):
    """keyword arguments of _ops.conv2d_prec for a built case"""
    c = o["case"]
    return dict(precision=precision, x1=o["x1"], pad0=c["pad0"] if (precision == 1 or c["via_split_rows"] or o["x1"] is not None) else 0,
                pad1=c["pad1"], stride=c["stride"], pad=c["pad"], asym=c["asym"], up=c["up"], bias=o["bias"], rowvec=o["rowvec"],
                resid=o["resid"], resid_pad=c["resid"] or 0, act=c["act"], alpha=c["alpha"], geglu=c["geglu"],
                via_split_rows=c["via_split_rows"] and precision == 2, want_stats=c["stats"] and precision == 2)


# mutants of the convolution: each returns a float64 [B, N, Ho, Wo] of a subtly wrong kernel on the case's operands
def conv_mutant_tap_shift(o):
    """filter tap 0 reads the pixel of tap 1"""
    A = o["A"].clone()
    A[:, 0] = o["A"][:, 1]
    return conv_epilogue(A.reshape(A.shape[0], -1) @ o["Wm"].reshape(o["case"]["N"], -1).T, o, torch.float64)


def conv_mutant_seam(o):
    """the concat seam one 16-channel K step late: channels C0 .. C0 + 15 come from the wrong place (here: the next 16 of x1)"""
    C0 = o["case"]["C0"]
    A = o["A"].clone()
    A[:, :, C0:C0 + 16] = o["A"][:, :, C0 + 16:C0 + 32]
    return conv_epilogue(A.reshape(A.shape[0], -1) @ o["Wm"].reshape(o["case"]["N"], -1).T, o, torch.float64)


def conv_mutant_rowvec(o):
    """the row vector of the neighbouring image"""
    Af, Wf = o["A"].reshape(o["A"].shape[0], -1), o["Wm"].reshape(o["case"]["N"], -1)
    return conv_epilogue(Af @ Wf.T, o, torch.float64, rowvec_shift=1)


# ==================================================================================================== attention
def _ac(name, mode, H, D, Tq, Tk, **kw):
    d = dict(name=name, mode=mode, B=2, H=H, D=D, Tq=Tq, Tk=Tk, padq=0, padk=0, padv=0, q_log2=False, obias=False, spike=None,
             prec=(1,))
    d.update(kw)
    return d


ATTN_CASES = [
    # ---- flash (mode 2): every DB 1..5 in both output forms, three widths that are no multiple of 32, Tq / Tk ragged
    _ac("flash_d8_tq1_tk1", 2, 3, 8, 1, 1, prec=(1, 2)),
    _ac("flash_d8_tq33_tk5", 2, 1, 8, 33, 5, prec=(1, 2), padq=4, padk=8, padv=12),
    _ac("flash_d32_tq129_tk31", 2, 3, 32, 129, 31, prec=(1, 2), q_log2=True),
    _ac("flash_d40_tq200_tk77", 2, 3, 40, 200, 77, prec=(1, 2), padq=8, padk=4, padv=4, q_log2=True),
    _ac("flash_d64_tq33_tk33", 2, 1, 64, 33, 33, prec=(1, 2)),
    _ac("flash_d80_tq129_tk77", 2, 3, 80, 129, 77, prec=(1, 2), padk=4),
    _ac("flash_d128_tq1_tk33", 2, 1, 128, 1, 33, prec=(1, 2), q_log2=True),
    _ac("flash_d160_tq200_tk5", 2, 3, 160, 200, 5, prec=(1, 2), padq=4),
    _ac("flash_d160_tq33_tk31", 2, 1, 160, 33, 31, prec=(1, 2)),
    _ac("flash_d64_tk3_half1_empty", 2, 3, 64, 33, 3),
    # ---- the maximum arrives in the last key tile, after the first tiles were accumulated; one score of about +60 / -60
    _ac("flash_spike_last_tile", 2, 3, 40, 129, 77, spike=(70, 60.0), prec=(1, 2)),
    _ac("flash_spike_last_tile_log2", 2, 1, 64, 33, 77, spike=(76, 60.0), q_log2=True),
    _ac("flash_spike_minus60", 2, 3, 32, 33, 33, spike=(32, -60.0)),
    # ---- mode 0: the networks' entry (fused q | k), with the value bias; D = 64, T = 256 as the improved-DDPM blocks
    _ac("fwd_d64_t256_obias", 0, 2, 64, 256, 256, obias=True, padq=4, padv=4),
    _ac("fwd_d160_t100", 0, 1, 160, 100, 100, obias=True),
    _ac("fwd_d164_t100", 0, 1, 164, 100, 100, obias=True),
    # ---- mode 1: one wave per query
    _ac("wave_d68_t64", 1, 2, 68, 64, 64, obias=True, padq=4, padv=8),
    _ac("wave_d68_t100", 1, 1, 68, 100, 100),
    _ac("wave_d512_t256", 1, 1, 512, 256, 256, obias=True),
    _ac("wave_d512_t100", 1, 2, 512, 100, 100, padq=8),
    _ac("wave_d160_t100", 1, 1, 160, 100, 100, obias=True),
    _ac("wave_d164_t100", 1, 1, 164, 100, 100, obias=True),
]
ATTN_BY_NAME = {c["name"]: c for c in ATTN_CASES}
assert len(ATTN_BY_NAME) == len(ATTN_CASES)


def _heads(t, H):
    B, T, C = t.shape
    return t.reshape(B, T, H, C // H).permute(0, 2, 1, 3)  # [B, H, T, D]


def attn_ref64(q, k, v, H, scale, q_log2=False, obias=None, drop_last_key=False, extra_zero_key=False):
    q, k, v = _heads(q.double(), H), _heads(k.double(), H), _heads(v.double(), H)
    if drop_last_key:      # mutant: the last key of the ragged tile excluded
        k, v = k[:, :, :-1], v[:, :, :-1]
    if extra_zero_key:     # mutant: the first padding key (a zero row of K and V) included
        k, v = F.pad(k, (0, 0, 0, 1)), F.pad(v, (0, 0, 0, 1))
    s = q @ k.transpose(2, 3)
    p = torch.softmax(s * math.log(2.0) if q_log2 else s * scale, -1)
    o = (p @ v).permute(0, 2, 1, 3).reshape(q.shape[0], q.shape[2], -1)
    return o + obias.double() if obias is not None else o


def _scores32(q, k):
    """fp32 q . k, d ascending, sequential fused multiply-adds: [B, H, Tq, Tk]"""
    s = torch.zeros(q.shape[0], q.shape[1], q.shape[2], k.shape[2], dtype=torch.float32)
    for d in range(q.shape[3]):
        s = fma32(q[..., :, None, d], k[..., None, :, d], s)
    return s


def attn_emulate_flash(q, k, v, H, scale, q_log2=False, obias=None):
    """k_flash_f32: q times qmul, scores, exp2 softmax over 32-key blocks with the running maximum, then P V; all fp32"""
    q, k, v = _heads(q.float(), H), _heads(k.float(), H), _heads(v.float(), H)
    if not q_log2:
        q = q * torch.tensor(scale * LOG2E, dtype=torch.float32)
    s = _scores32(q, k)
    B, _, Tq, Tk = s.shape
    m = torch.full((B, H, Tq), -math.inf)
    l = torch.zeros(B, H, Tq)
    o = torch.zeros(B, H, Tq, v.shape[3])
    for k0 in range(0, Tk, 32):
        sb = s[..., k0:k0 + 32]
        mn = torch.maximum(m, sb.max(-1).values)
        alpha = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - mn))
        p = torch.exp2(sb - mn[..., None])
        ps = torch.zeros_like(l)
        for j in range(p.shape[-1]):
            ps = ps + p[..., j]
        l = l * alpha + ps
        m = mn
        o = o * alpha[..., None]
        for j in range(p.shape[-1]):
            o = fma32(p[..., j, None], v[:, :, k0 + j, None, :], o)
    o = o * (1.0 / l)[..., None]
    o = o.permute(0, 2, 1, 3).reshape(B, Tq, -1)
    return o + obias.float() if obias is not None else o


def attn_emulate_wave(q, k, v, H, scale, obias=None):
    """k_attention_f32: scores times scale, exp(s - max), the weighted sum over the keys in order, times 1 / den, + bias"""
    q, k, v = _heads(q.float(), H), _heads(k.float(), H), _heads(v.float(), H)
    s = _scores32(q, k) * torch.tensor(scale, dtype=torch.float32)
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    den = e.sum(-1)
    o = torch.zeros(*s.shape[:3], v.shape[3])
    for j in range(s.shape[3]):
        o = fma32(e[..., j, None], v[:, :, j, None, :], o)
    o = (o * (1.0 / den)[..., None]).permute(0, 2, 1, 3).reshape(q.shape[0], q.shape[2], -1)
    return o + obias.float() if obias is not None else o


def attn_kernel(c):
    """which kernel a case reaches: "flash" or "wave" (attention_f32_fwd: flash for D <= 160)"""
    return "flash" if c["mode"] == 2 or (c["mode"] == 0 and c["D"] <= 160) else "wave"


@functools.lru_cache(maxsize=None)
def attn_build(name):
    c = ATTN_BY_NAME[name]
    gen = torch.Generator().manual_seed(_seed("f32op/attn/" + name))
    B, H, D, Tq, Tk = (c[x] for x in ("B", "H", "D", "Tq", "Tk"))
    hs = (1.0 + 0.5 * torch.arange(H, dtype=torch.float32)).repeat_interleave(D)  # every head its own scale and offset
    ho = (0.3 * (torch.arange(H, dtype=torch.float32) - 1.0)).repeat_interleave(D)
    img = torch.tensor([1.0, 1.4])[:B, None, None]
    q = (img * hs * torch.randn(B, Tq, H * D, generator=gen) + ho).float()
    k = (hs.flip(0) * torch.randn(B, Tk, H * D, generator=gen) - ho).float()
    v = (img * (hs * torch.randn(B, Tk, H * D, generator=gen) + 2.0 * ho + 0.5)).float()
    scale = 1.0 / math.sqrt(D)
    if c["spike"]:  # one key along a direction every query carries: its score is about `target` in log2 units for every query
        j, target = c["spike"]
        u = torch.zeros(H * D)
        u[::D] = 1.0                               # first dimension of every head
        q[:, :, ::D] = 3.0
        k[:, :, ::D] = 0.0
        k[:, j] = k[:, j] + u * (target / (3.0 * scale * LOG2E))
    if c["q_log2"]:  # q arrives in log2 units (the scale folded into the to_q weights): one fp32 rounding, part of the operand
        q = (q * f32(scale * LOG2E)).float()
    obias = (0.5 * torch.randn(H * D, generator=gen) + 1.0).float() if c["obias"] else None
    o = dict(case=c, q=q, k=k, v=v, scale=scale, obias=obias)
    o["ref"] = attn_ref64(q, k, v, H, scale, c["q_log2"], obias)
    if attn_kernel(c) == "flash":
        o["emu"] = attn_emulate_flash(q, k, v, H, scale, c["q_log2"], obias)
    else:
        o["emu"] = attn_emulate_wave(q, k, v, H, scale, obias)
    err = (o["emu"].double() - o["ref"]).abs().max().item()
    o["tol"] = {p: tol_f32(o["ref"], err, split=p == 2) for p in c["prec"]}
    return o


def attn_call_args(o, precision):
    c = o["case"]
    return dict(heads=c["H"], scale=o["scale"], mode=c["mode"], precision=precision, padq=c["padq"], padk=c["padk"], padv=c["padv"],
                q_log2=c["q_log2"], obias=o["obias"])


# ==================================================================================================== rows
def _rc(name, op, rows, C, **kw):
    d = dict(name=name, op=op, rows=rows, C=C, C1=0, pad0=0, pad1=0, large_mean=False, prec=(1, 2))
    d.update(kw)
    return d


ROWS_CASES = [_rc("layernorm_c%d_r%d" % (C, r), "layernorm", r, C, pad0=p)
              for C, r, p in ((4, 1, 0), (4, 301, 4), (64, 5, 0), (260, 301, 12), (320, 5, 4), (1280, 1, 0), (1280, 301, 0),
                              (2048, 5, 8))]
ROWS_CASES += [
    _rc("layernorm_large_mean", "layernorm", 5, 320, large_mean=True, pad0=4),
    _rc("geglu_n32_r5", "geglu", 5, 64), _rc("geglu_n96_r301", "geglu", 301, 192), _rc("geglu_n1280_r5", "geglu", 5, 2560),
    _rc("split_rows_c64", "split_rows", 301, 64, prec=(2,)),
    _rc("split_rows_c36_pad", "split_rows", 5, 36, pad0=4, prec=(2,)),
    _rc("split_rows_c32+64_pads", "split_rows", 301, 32, C1=64, pad0=4, pad1=8, prec=(2,)),
    _rc("split_rows_c4+4", "split_rows", 5, 4, C1=4, pad1=4, prec=(2,)),
    _rc("split_rows_ranges", "split_rows", 5, 64, prec=(2,)),
]
ROWS_BY_NAME = {c["name"]: c for c in ROWS_CASES}
assert len(ROWS_BY_NAME) == len(ROWS_CASES)
LN_LARGE_MEAN = (100.0, 0.1)  # offset, spread


def geglu_ref(h, dtype, swap_block=None):
    """h [rows][2 Nout] in the packed order (blocks of 64 = [32 value | 32 gate]) -> value * gelu(gate), exact erf"""
    hb = h.to(dtype).reshape(h.shape[0], -1, 2, 32)
    val, gate = hb[:, :, 0], hb[:, :, 1]
    if swap_block is not None:  # mutant: the halves of one 64-column block swapped
        val, gate = val.clone(), gate.clone()
        val[:, swap_block], gate[:, swap_block] = hb[:, swap_block, 1], hb[:, swap_block, 0]
    g = 0.5 * gate * (1.0 + torch.erf(gate / math.sqrt(2.0))) if dtype == torch.float64 else F.gelu(gate)
    return (val * g).reshape(h.shape[0], -1)


def layernorm_uncentred32(x, gamma, beta, eps=1e-5):
    """mutant: var = E[x^2] - mean^2 in fp32"""
    x = x.float()
    mean = x.mean(1, keepdim=True)
    var = (x * x).mean(1, keepdim=True) - mean * mean
    return (x - mean) / torch.sqrt(var.clamp(min=0) + eps) * gamma.float() + beta.float()


@functools.lru_cache(maxsize=None)
def rows_build(name):
    c = ROWS_BY_NAME[name]
    gen = torch.Generator().manual_seed(_seed("f32op/rows/" + name))
    rows, C, C1 = c["rows"], c["C"], c["C1"]
    rs = (1.0 + 0.1 * (torch.arange(rows) % 7))[:, None]   # every row its own scale and offset, every column its own offset
    ro = (0.3 * ((torch.arange(rows) % 5) - 2.0))[:, None]
    x = (rs * torch.randn(rows, C + C1, generator=gen) + ro + 0.5 * torch.randn(C + C1, generator=gen)).float()
    if c["large_mean"]:
        x = (LN_LARGE_MEAN[0] + LN_LARGE_MEAN[1] * x).float()
    if name == "split_rows_ranges":
        x = _log_uniform(gen, (rows, C), -10, 10)
    o = dict(case=c, x=x, x0=x[:, :C].contiguous(), x1=x[:, C:].contiguous() if C1 else None, gamma=None, beta=None)
    if c["op"] == "layernorm":
        o["gamma"] = (1.0 + 0.2 * torch.randn(C, generator=gen)).float()
        o["beta"] = (0.2 * torch.randn(C, generator=gen)).float()
        o["ref"] = F.layer_norm(x.double(), (C,), o["gamma"].double(), o["beta"].double(), 1e-5)
        o["emu"] = F.layer_norm(x, (C,), o["gamma"], o["beta"], 1e-5)
    elif c["op"] == "geglu":
        o["ref"], o["emu"] = geglu_ref(x, torch.float64), geglu_ref(x, torch.float32)
    else:
        o["ref"], o["emu"] = x.double(), decode(x)
    if c["op"] == "split_rows":
        o["tol"] = {2: pair_tol(o["ref"])}
    else:
        err = (o["emu"].double() - o["ref"]).abs().max().item()
        o["tol"] = {p: tol_f32(o["ref"], err, split=p == 2) for p in c["prec"]}
    return o


def rows_call_args(o, precision):
    c = o["case"]
    return dict(precision=precision, x1=o["x1"], pad0=c["pad0"], pad1=c["pad1"], gamma=o["gamma"], beta=o["beta"])


# ---- the composition raw-GEGLU projection -> GEGLU: x W^T -> chunk -> a * gelu(g) in float64
@functools.lru_cache(maxsize=None)
def geglu_chain_build():
    gen = torch.Generator().manual_seed(_seed("f32op/geglu_chain"))
    rows, Cin, Nout = 37, 64, 96
    x = (torch.randn(rows, Cin, generator=gen) + 0.3 * torch.randn(Cin, generator=gen)).float()
    w = (torch.randn(2 * Nout, Cin, generator=gen) / math.sqrt(Cin)).float()
    bias = (0.3 * torch.randn(2 * Nout, generator=gen)).float()
    h = x.double() @ w.double().T + bias.double()
    a, g = h.chunk(2, 1)
    ref = a * (0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0))))
    hs = seq_gemm32(x, w) + bias
    a32, g32 = hs.chunk(2, 1)
    emu = a32 * F.gelu(g32)
    return dict(x=x, w=w, bias=bias, ref=ref, emu=emu, Nout=Nout)


# ==================================================================================================== resample
RESAMPLE_CASES = [dict(name="b2_c4_6x10", B=2, C=4, H=6, W=10), dict(name="b2_c96_6x10", B=2, C=96, H=6, W=10)]
# more than 4096 x 256 output vectors of 4 channels: the grid-stride loops wrap
RESAMPLE_WRAP = {"avgpool": dict(name="wrap_c260_256x256", B=1, C=260, H=256, W=256),
                 "upsample": dict(name="wrap_c260_64x64", B=1, C=260, H=64, W=64)}


@functools.lru_cache(maxsize=None)
def resample_x(name):
    c = next(r for r in RESAMPLE_CASES + list(RESAMPLE_WRAP.values()) if r["name"] == name)
    gen = torch.Generator().manual_seed(_seed("f32op/resample/" + name))
    return (make_x(gen, c["B"], c["C"], c["H"], c["W"]).abs() + 0.1).float()  # positive: see the module docstring


def avgpool_ref64(x):
    return F.avg_pool2d(x.double(), 2)


# ==================================================================================================== table
if __name__ == "__main__":  # emulation error / tolerance per case
    for c in CONV_CASES:
        o = conv_build(c["name"])
        for p in c["prec"]:
            e = (o["emu"][p].double() - o["ref"]).abs()
            print("conv/%s p%d  emu %.2e of max|ref| %.2f, emu / tol %.3f" %
                  (c["name"], p, (e.max() / o["ref"].abs().max()).item(), o["ref"].abs().max().item(), (e / o["tol"][p]).max().item()))
    for c in ATTN_CASES:
        o = attn_build(c["name"])
        e = (o["emu"].double() - o["ref"]).abs()
        print("attn/%s  emu %.2e of max|ref|, emu / tol %.3f" % (c["name"], (e.max() / o["ref"].abs().max()).item(),
                                                                 (e / o["tol"][1]).max().item()))
