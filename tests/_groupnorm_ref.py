"""GroupNorm(32) references for tests/test_groupnorm_host.py (CPU) and tests/test_gpu_groupnorm.py (GPU).

Three pieces, all plain torch on the host:
  * ref64            float64 GroupNorm of one tensor or a channel concat, + FiLM (a row per image or one shared row), + SiLU;
                     optionally with the statistics of ANOTHER tensor (what the fold kernels compute when they are handed
                     that tensor's block sums)
  * block_stats      the [B*HW/32][2][C] per-32-row-block channel sums (ConvGemmParams::stats layout) of any tensor, float64
  * emulate16        the 16-bit path's arithmetic in fp32: one-pass sums in the kernels' order (k_gn_fold: strided items + a
                     256-wide tree; k_gn_stats / k_gn_coef: rows `rif` apart, slabs in order), var = q/n - mean^2, one
                     multiply-add coefficient pair per (image, channel), x/(1+exp(-x)). Not rounded to the storage format.
  * emulate32        the fp32 path: float64 statistics, fp32 coefficient pair and apply
and the case tables both test modules walk, so the host test covers exactly the inputs the GPU test uses.
"""
import functools
import math
import zlib

import torch
import torch.nn.functional as F

G = 32

# ------------------------------------------------------------------------------------------------------------ tolerance
# 16-bit path, per element: |got - ref| <= u |ref| + s max|ref|
#   u = one unit in the last place of the storage format (2^-10 fp16, 2^-7 bf16): the single rounding of the output
#   s = GN16_S covers the fp32 one-pass statistics and the fast sigmoid. It is twice the largest max|emulate16 - ref64| /
#       max|ref64| over every case below (tests/test_groupnorm_host.py asserts the emulation within half the tolerance).
# Per-family maxima of the emulation (python tests/_groupnorm_ref.py prints the table):
#                 fold      proof     fallback  tensor    large_mean  producer
#   fp16 inputs   2.57e-07  1.22e-07  4.17e-07  4.77e-07  1.10e-05    3.38e-05
#   bf16 inputs   2.66e-07  1.60e-07  5.64e-07  3.67e-07  7.29e-06    2.49e-04
# The producer cases set it (largest: the plain 3x3 conv, N = 96): a conv epilogue sums its outputs BEFORE their
# 16-bit rounding, so its statistics are those of a tensor one rounding away from the stored one - a difference that scales
# with the storage format's step, hence one constant per format.
GN16_S = {True: 6.8e-5, False: 5.0e-4}  # fp16 storage, bf16 storage


def unit16(fp16):
    return 2.0 ** -10 if fp16 else 2.0 ** -7


def tol16(ref, fp16):
    return unit16(fp16) * ref.abs() + GN16_S[bool(fp16)] * ref.abs().max()


# fp32 paths: 4 x the error of torch's own fp32 group_norm (+ FiLM, SiLU in fp32) on the same input, floor 2^-22 max|ref|;
# the split output adds 2^-21 |ref| for the hi/lo fp16 pair
def tol32(ref, torch_err, split):
    """torch_err: max|torch fp32 - float64| on the same input"""
    b = max(4.0 * torch_err, 2.0 ** -22 * ref.abs().max().item())
    t = torch.full_like(ref, b)
    return t + 2.0 ** -21 * ref.abs() if split else t


# ------------------------------------------------------------------------------------------------------------ references
def _film_rows(film, B, C):
    """film [B, 2C] or a shared [2C] row -> scale, shift as [B or 1, C, 1, 1]"""
    f = film.reshape(-1, 2 * C)
    return f[:, :C, None, None], f[:, C:, None, None]


def ref64(x, gamma, beta, eps, film=None, silu=False, stats_of=None):
    x = x.double()
    s = x if stats_of is None else stats_of.double()
    B, C = x.shape[:2]
    sg = s.reshape(B, G, -1)
    mean, var = sg.mean(2, keepdim=True), sg.var(2, unbiased=False, keepdim=True)
    y = ((x.reshape(B, G, -1) - mean) / torch.sqrt(var + eps)).reshape(x.shape)
    y = y * gamma.double()[None, :, None, None] + beta.double()[None, :, None, None]
    if film is not None:
        sc, sh = _film_rows(film.double(), B, C)
        y = y * (1 + sc) + sh
    return y * torch.sigmoid(y) if silu else y


def torch32(x, gamma, beta, eps, film=None, silu=False):
    y = F.group_norm(x.float(), G, gamma.float(), beta.float(), eps)
    if film is not None:
        sc, sh = _film_rows(film.float(), x.shape[0], x.shape[1])
        y = y * (1 + sc) + sh
    return F.silu(y) if silu else y


def block_stats(x):
    """float64 [B*HW/32][2][C]: per-channel sum | sum of squares over each block of 32 NHWC rows"""
    B, C, H, W = x.shape
    assert (H * W) % 32 == 0
    rows = x.double().permute(0, 2, 3, 1).reshape(-1, 32, C)
    return torch.stack([rows.sum(1), (rows * rows).sum(1)], 1)


# ------------------------------------------------------------------------------------------------------------ emulation
def _fold_sums32(st0, st1, B, HW):
    """k_gn_fold: thread t adds items t, t + 256, ... (item = row block * cpg + channel in group), then a 256-wide tree"""
    s = st0 if st1 is None else torch.cat([st0, st1], 2)
    s = s.float()
    C, nb = s.shape[2], HW // 32
    cpg = C // G
    v = s.reshape(B, nb, 2, G, cpg).permute(0, 3, 2, 1, 4).reshape(B, G, 2, nb * cpg)
    k = -(-v.shape[3] // 256)
    v = F.pad(v, (0, k * 256 - v.shape[3])).reshape(B, G, 2, k, 256)
    acc = torch.zeros(B, G, 2, 256)
    for j in range(k):
        acc = acc + v[:, :, :, j]
    o = 128
    while o:
        acc = torch.cat([acc[..., :o] + acc[..., o:2 * o], acc[..., o:]], -1)
        o //= 2
    return acc[..., 0]  # [B, G, 2]


def _tensor_sums32(x):
    """k_gn_stats + k_gn_coef: per slab, rows `rif` apart per thread; a group's thread folds (r, c) in order; slabs in order"""
    B, C, H, W = x.shape
    HW, cpg, nvec = H * W, C // G, C // 8
    rif = 256 // nvec if nvec <= 256 else 1
    S = max(1, min(64, HW // 64))
    rps = -(-HW // S)
    rows = x.float().permute(0, 2, 3, 1).reshape(B, HW, C)
    tot = torch.zeros(B, G, 2)
    for s in range(S):
        slab = rows[:, s * rps:min(HW, (s + 1) * rps)]
        ga, gq = torch.zeros(B, G), torch.zeros(B, G)
        part = []
        for r0 in range(rif):
            a, q = torch.zeros(B, C), torch.zeros(B, C)
            for i in range(r0, slab.shape[1], rif):
                a = a + slab[:, i]
                q = q + slab[:, i] * slab[:, i]
            part.append((a.reshape(B, G, cpg), q.reshape(B, G, cpg)))
        for a, q in part:
            for c in range(cpg):
                ga = ga + a[:, :, c]
                gq = gq + q[:, :, c]
        tot = tot + torch.stack([ga, gq], 2)
    return tot


def _coef_apply32(x, mean, rstd, gamma, beta, film, silu):
    """gn_write_coef + k_gn_apply in fp32: y = x*al + be; mean, rstd [B, G] fp32"""
    B, C = x.shape[:2]
    cpg = C // G
    mean = mean.float().repeat_interleave(cpg, 1)
    a = rstd.float().repeat_interleave(cpg, 1) * gamma.float()[None]
    bb = beta.float()[None] - mean * a
    if film is not None:
        f = film.float().reshape(-1, 2 * C)
        sc = 1.0 + f[:, :C]
        a = a * sc
        bb = bb * sc + f[:, C:]
    y = x.float() * a[:, :, None, None] + bb[:, :, None, None]
    return y / (1.0 + torch.exp(-y)) if silu else y


def emulate16(x, gamma, beta, eps, film=None, silu=False, st0=None, st1=None):
    """x: the (concatenated) 16-bit-representable input; st0 / st1: block statistics -> the fold path, else the tensor path"""
    B, C, H, W = x.shape
    sums = _fold_sums32(st0, st1, B, H * W) if st0 is not None else _tensor_sums32(x)
    n = torch.tensor(float((C // G) * H * W), dtype=torch.float32)
    mean = sums[..., 0] / n
    var = torch.clamp(sums[..., 1] / n - mean * mean, min=0.0)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    return _coef_apply32(x, mean, rstd, gamma, beta, film, silu)


def emulate32(x, gamma, beta, eps, film=None, silu=False, st0=None, st1=None):
    """fp32 path: float64 statistics (of the tensor, or folded from fp32 block statistics), fp32 coefficients and apply"""
    B, C, H, W = x.shape
    n = (C // G) * H * W
    if st0 is not None:
        s = (st0 if st1 is None else torch.cat([st0, st1], 2)).float().double()
        s = s.reshape(B, (H * W) // 32, 2, G, C // G).sum((1, 4))  # [B, 2, G]
        a, q = s[:, 0], s[:, 1]
    else:
        xg = x.float().double().reshape(B, G, -1)
        a, q = xg.sum(2), (xg * xg).sum(2)
    mean = a / n
    var = torch.clamp(q / n - mean * mean, min=0.0)
    rstd = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
    return _coef_apply32(x, mean, rstd, gamma, beta, film, silu)


# ------------------------------------------------------------------------------------------------------------ inputs
def _seed(name):
    return zlib.crc32(name.encode()) % (2 ** 31)


IMG_OFF = (0.6, -1.2, 1.8, -0.3)
IMG_SCALE = (1.0, 1.5, 2.0, 0.7)
IMG_OFF_OTHER = (-0.9, 1.5, -0.3, 0.8)
IMG_SCALE_OTHER = (2.0, 2.5, 3.0, 1.4)  # wider than IMG_SCALE: the outputs of the proof cases stay below their own GroupNorm's


def make_x(gen, B, C, H, W, off=IMG_OFF, scale=IMG_SCALE):
    """every image its own offset and scale, every channel its own offset: a wrong image, channel or slot moves the result by O(1)"""
    o = torch.tensor(off[:B])[:, None, None, None]
    s = torch.tensor(scale[:B])[:, None, None, None]
    ch = 0.8 * torch.randn(C, generator=gen)[None, :, None, None]
    return o + ch + s * torch.randn(B, C, H, W, generator=gen)


def make_x_large_mean(gen, B, C, H, W, offset):
    """per-group offset `offset`, spread 0.5 (x 1.0, 1.2 per image): mean^2 / var = 4 offset^2 (144 at offset 6)"""
    s = torch.tensor([0.5 * (1.0 + 0.2 * b) for b in range(B)])[:, None, None, None]
    o = torch.tensor([0.05 * b for b in range(B)])[:, None, None, None]
    ch = 0.05 * torch.randn(C, generator=gen)[None, :, None, None]
    return offset + o + ch + s * torch.randn(B, C, H, W, generator=gen)


LARGE_MEAN_OFFSET = 6.0


def _c(name, B, C0, C1, H, W, **kw):
    d = dict(name=name, B=B, C0=C0, C1=C1, H=H, W=W, silu=False, film=None, pad0=0, pad1=0, stats=None, eps=1e-5,
             large_mean=False)
    d.update(kw)
    return d


# stats: "own" = block statistics of the input itself (fold path), "other" = of a different tensor (proof the fold ran),
#        "nan" = all-NaN arrays that must not be read (fallbacks), "nan0" = NaN stats0 and no stats1, None = no statistics
# film:  None | "2C" | "2C+64" | "shared"
_FOLD_SHAPES = [("c96", 3, 96, 0, 8, 8), ("c64+32", 3, 64, 32, 8, 8), ("c32", 2, 32, 0, 8, 8),
                ("c1280+640", 2, 1280, 640, 8, 8), ("c1280+1280", 1, 1280, 1280, 8, 8), ("c128_32x32", 2, 128, 0, 32, 32),
                ("c320_64x32", 1, 320, 0, 64, 32)]

CASES16 = []
for _n, _B, _C0, _C1, _H, _W in _FOLD_SHAPES:
    for _silu in (False, True):
        CASES16.append(_c("fold/%s%s" % (_n, "_silu" if _silu else ""), _B, _C0, _C1, _H, _W, silu=_silu, stats="own",
                          eps=1e-6 if _n == "c32" else 1e-5))
for _n, _C0, _C1 in (("c96", 96, 0), ("c64+32", 64, 32)):
    for _f, _silu in (("2C", True), ("2C+64", False), ("shared", True)):
        CASES16.append(_c("fold/%s_film_%s" % (_n, _f), 3, _C0, _C1, 8, 8, silu=_silu, film=_f, stats="own"))
CASES16 += [
    _c("proof/c96", 3, 96, 0, 8, 8, stats="other"),
    _c("proof/c64+32", 3, 64, 32, 8, 8, stats="other", silu=True),
    _c("fallback/hw36", 3, 96, 0, 6, 6, stats="nan"),
    _c("fallback/hw36_concat", 3, 64, 32, 6, 6, stats="nan", silu=True),
    _c("fallback/pad0", 3, 96, 0, 8, 8, stats="nan", pad0=8),
    _c("fallback/stats1_null", 3, 64, 32, 8, 8, stats="nan0"),
    _c("tensor/c64+32", 3, 64, 32, 8, 8),
    _c("tensor/c64+32_film_shared_silu", 3, 64, 32, 8, 8, film="shared", silu=True),
    _c("tensor/c64+32_film_2C+64", 3, 64, 32, 8, 8, film="2C+64"),
    _c("tensor/c1280+640", 2, 1280, 640, 8, 8, silu=True),
    _c("tensor/c1280+1280", 1, 1280, 1280, 8, 8),
    _c("tensor/c64+32_pads", 3, 64, 32, 8, 8, pad0=8, pad1=16, silu=True),
    _c("tensor/c1280+1280_hw36", 1, 1280, 1280, 6, 6, silu=True),
    _c("tensor/c64+32_hw100", 2, 64, 32, 10, 10),
    _c("large_mean/fold", 2, 128, 0, 32, 32, stats="own", large_mean=True),
    _c("large_mean/tensor", 2, 128, 0, 32, 32, large_mean=True, silu=True),
]

# the fp32 path (precision 1) and its split mode (precision 2) run every one of these
CASES32 = [
    _c("f32/c96", 2, 96, 0, 8, 8),
    _c("f32/c64+32_film_silu", 2, 64, 32, 8, 8, film="2C", silu=True),
    _c("f32/c64+32_film_shared", 2, 64, 32, 8, 8, film="shared"),
    _c("f32/c64+32_pads", 2, 64, 32, 8, 8, pad0=4, pad1=8, silu=True),
    _c("f32/c768+512_wide", 1, 768, 512, 8, 8, silu=True),
    _c("f32/c96_hw36", 2, 96, 0, 6, 6, stats="nan"),
    _c("f32/fold_c96", 2, 96, 0, 8, 8, stats="own", silu=True),
    _c("f32/fold_c64+32_film", 2, 64, 32, 8, 8, stats="own", film="2C+64"),
    _c("f32/fold_c768+512", 1, 768, 512, 8, 8, stats="own"),
    _c("f32/proof_c96", 2, 96, 0, 8, 8, stats="other"),
    _c("f32/proof_c64+32", 2, 64, 32, 8, 8, stats="other", silu=True),
]


def _identity(t):
    return t


@functools.lru_cache(maxsize=None)
def _build(name, table, rnd_key):
    case = next(c for c in (CASES16 if table == 16 else CASES32) if c["name"] == name)
    rnd = _ROUNDERS[rnd_key]
    B, C0, C1, H, W = (case[k] for k in ("B", "C0", "C1", "H", "W"))
    C = C0 + C1
    gen = torch.Generator().manual_seed(_seed(name))
    if case["large_mean"]:
        x = rnd(make_x_large_mean(gen, B, C, H, W, LARGE_MEAN_OFFSET))
    else:
        x = rnd(make_x(gen, B, C, H, W))
    gamma = 1.0 + 0.2 * torch.randn(C, generator=gen)
    beta = 0.2 * torch.randn(C, generator=gen)
    film = None
    if case["film"] == "shared":
        film = 0.3 * torch.randn(2 * C, generator=gen)
    elif case["film"]:
        film = 0.3 * torch.randn(B, 2 * C, generator=gen)
    d = dict(case=case, x=x, x0=x[:, :C0].contiguous(), x1=x[:, C0:].contiguous() if C1 else None, gamma=gamma, beta=beta,
             film=film, film_ld=2 * C + 64 if case["film"] == "2C+64" else None, st0=None, st1=None, other=None)
    src = None
    if case["stats"] == "own":
        src = x
    elif case["stats"] == "other":
        src = d["other"] = rnd(make_x(gen, B, C, H, W, IMG_OFF_OTHER, IMG_SCALE_OTHER))
    if src is not None:
        st = block_stats(src).float()
        d["st0"], d["st1"] = st[:, :, :C0].contiguous(), st[:, :, C0:].contiguous() if C1 else None
    elif case["stats"] in ("nan", "nan0"):
        nb = -(-B * H * W // 32)
        d["st0"] = torch.full((nb, 2, C0), float("nan"))
        d["st1"] = torch.full((nb, 2, C1), float("nan")) if C1 and case["stats"] == "nan" else None
    kw = dict(film=film, silu=case["silu"])
    d["ref"] = ref64(x, gamma, beta, case["eps"], stats_of=d["other"], **kw)
    d["ref_own"] = ref64(x, gamma, beta, case["eps"], **kw) if d["other"] is not None else d["ref"]
    folds = src is not None
    emu = emulate16 if table == 16 else emulate32
    d["emu"] = emu(x, gamma, beta, case["eps"], st0=d["st0"] if folds else None, st1=d["st1"] if folds else None, **kw)
    if table == 32:  # the bound comes from torch's fp32 group_norm of the same input (own statistics, also for the proof cases)
        d["torch_err"] = (torch32(x, gamma, beta, case["eps"], **kw).double() - d["ref_own"]).abs().max().item()
    return d


_ROUNDERS = {"none": _identity}


def build16(name, rnd, fmt):
    """operands, float64 reference and fp32 emulation of a CASES16 entry, computed once per storage format (`rnd` rounds to it)"""
    _ROUNDERS[fmt] = rnd
    return _build(name, 16, fmt)


def build32(name):
    return _build(name, 32, "none")


def call_args(d):
    """keyword arguments of _ops.groupnorm_ex for a built case (without precision)"""
    c = d["case"]
    return dict(x1=d["x1"], pad0=c["pad0"], pad1=c["pad1"], silu=c["silu"], film=d["film"], film_shared=c["film"] == "shared",
                film_ld=d["film_ld"], stats0=d["st0"], stats1=d["st1"])


# ------------------------------------------------------------------------------------------------------------ conv producers
# composition with the real producers (cd_op_conv2d_16 with statistics -> cd_op_groupnorm_ex): name, B, Cin, H, W, N, up, tile
CONV_PRODUCERS = [("conv3x3", 2, 64, 16, 16, 96, False, 0), ("conv3x3_split3", 2, 64, 16, 16, 96, False, 20 | (3 << 8)),
                  ("conv3x3_up", 2, 64, 16, 16, 64, True, 0), ("concat_a64", 2, 64, 16, 16, 64, False, 0),
                  ("concat_b32", 2, 64, 16, 16, 32, False, 0)]


@functools.lru_cache(maxsize=None)
def conv_operands(name, fmt):
    _, B, Cin, H, W, N, up, tile = next(p for p in CONV_PRODUCERS if p[0] == name)
    rnd = _ROUNDERS[fmt]
    gen = torch.Generator().manual_seed(_seed("producer/" + name))
    x = rnd(make_x(gen, B, Cin, H, W))
    w = rnd(torch.randn(N, Cin, 3, 3, generator=gen) / math.sqrt(Cin * 9))
    bias = 0.5 * torch.randn(N, generator=gen)
    gamma = 1.0 + 0.2 * torch.randn(N, generator=gen)
    beta = 0.2 * torch.randn(N, generator=gen)
    xin = F.interpolate(x.double(), scale_factor=2, mode="nearest") if up else x.double()
    y64 = F.conv2d(xin, w.double(), bias.double(), padding=1)
    return dict(x=x, w=w, bias=bias, gamma=gamma, beta=beta, up=up, tile=tile, y64=y64)


def conv_operands_for(name, rnd, fmt):
    _ROUNDERS[fmt] = rnd
    return conv_operands(name, fmt)


PRODUCER_CHAINS = [("conv3x3",), ("conv3x3_split3",), ("conv3x3_up",), ("concat_a64", "concat_b32")]


def producer_host(names, rnd, fmt):
    """host model of conv(s) -> GroupNorm + SiLU (eps 1e-5): the float64 conv results rounded to the storage format, block
    statistics of the UNROUNDED results (what the epilogue sums) -> (float64 GroupNorm of the stored tensor, emulation)"""
    ops = [conv_operands_for(n, rnd, fmt) for n in names]
    y16 = torch.cat([rnd(o["y64"].float()) for o in ops], 1)
    sts = [block_stats(o["y64"]).float() for o in ops]
    gamma, beta = torch.cat([o["gamma"] for o in ops]), torch.cat([o["beta"] for o in ops])
    ref = ref64(y16, gamma, beta, 1e-5, silu=True)
    emu = emulate16(y16, gamma, beta, 1e-5, silu=True, st0=sts[0], st1=sts[1] if len(sts) > 1 else None)
    return ref, emu


# ------------------------------------------------------------------------------------------------------------ table
def needed_s(rnd, fmt):
    """per-case max|emulate16 - ref64| / max|ref64|: what GN16_S is derived from"""
    out = {}
    for c in CASES16:
        d = build16(c["name"], rnd, fmt)
        out[c["name"]] = ((d["emu"].double() - d["ref"]).abs().max() / d["ref"].abs().max()).item()
    for names in PRODUCER_CHAINS:
        ref, emu = producer_host(names, rnd, fmt)
        out["producer/" + "+".join(names)] = ((emu.double() - ref).abs().max() / ref.abs().max()).item()
    return out


if __name__ == "__main__":
    for fmt, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        r = needed_s(lambda t, dt=dt: t.to(dt).to(torch.float32), fmt)
        fam = {}
        for k, v in r.items():
            fam[k.split("/")[0]] = max(fam.get(k.split("/")[0], 0.0), v)
        print(fmt, {k: "%.2e" % v for k, v in fam.items()}, "max %.3e (%s)" % (max(r.values()), max(r, key=r.get)))
