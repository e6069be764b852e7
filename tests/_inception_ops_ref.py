"""Case tables and float64 references for the kernels and launch forms of the FID Inception-v3 (csrc/inception.hip) one at a
time: tests/test_inception_ops_host.py (CPU: the references against torch in float64, the bounds against fp32 restatements of
the kernels' arithmetic) and tests/test_gpu_inception_ops.py (GPU, through cd_op_pool3x3 / cd_op_global_avg /
cd_op_basic_conv). Not collected. Nothing here is taken from the kernels: the references are sums over explicitly shifted views.

  k_pool3x3<MAX>   bit for bit the maximum of the in-image taps of the 16-bit input
  k_pool3x3<AVG>   ref = float64 mean over the in-image taps (count_include_pad = False), rounded once to the storage format;
                   |got - ref| <= 1 ulp16(ref) + 9 x 2^-24 max|taps| (the fp32 sum of at most 9 terms, the fp32 reciprocal, one
                   rounding) and at least 95 % of a case's elements equal ref. The same reference with the divisor fixed at 9
                   must fail on the border pixels (avg_verify(..., divisor9=True)).
  k_global_avg     |got - float64 mean| <= HW x 2^-24 mean|x| per channel: HW - 1 fp32 additions, each within 2^-24 of the
                   running sum of magnitudes, and the product with the fp32 reciprocal
  k_fold_bn        packed weight within 1 ulp16 of round16(w gamma / sqrt(var + 1e-3)) computed in float64; bias within
                   2^-21 (|beta| + |mean sc|) (fp32: the sum, the square root and the quotient in sc, the product, the
                   difference - 4.5 x 2^-24 at most); channels [Cin, Cpad), rows and bias entries [N, Npad) exactly zero. With
                   eps = 1e-5 in the reference the check must fail (var reaches down to 1e-5).
  BasicConv2d      float64 conv2d of the 16-bit input with the DOWNLOADED packed weights and bias, ReLU; the operator's bounds
                   (_gemm_sweep.within_bounds); columns [N, round_up(N, 32)) exactly zero; everything outside the slice NaN.
"""
import zlib

import numpy as np
import torch

import _gemm_sweep as gs
from _glue_ref import lib_fmt, round16, step16  # noqa: F401  (lib_fmt: re-exported for the GPU test)

BN_EPS = 1e-3
GUARD_ROWS = 64  # tests/_ops.py: NaN rows behind every output buffer


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) % (2 ** 31))


def r16(v, fmt):
    """fp32 -> the storage format and back (float64)"""
    return round16(v, fmt).double()


def round16_f64(v, fmt):
    """float64 -> the nearest value of the storage format (ties to even), in ONE rounding (a conversion by way of fp32 rounds
    twice). v / step is exact (step is a power of two) and rint rounds halves to even; values in range only."""
    v = v.double()
    st = step16(v, fmt)
    return torch.from_numpy(np.rint((v / st).numpy())) * st


# ================================================================================================ 3 x 3 pools
def pool_out_hw(H, W, stride, pad):
    return (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1


def pool_taps(x, stride, pad):
    """x float64 [B, C, H, W] -> (taps [9, B, C, Ho, Wo] with NaN where the tap lies outside the image, inside [9, Ho, Wo])"""
    B, C, H, W = x.shape
    Ho, Wo = pool_out_hw(H, W, stride, pad)
    xp = torch.full((B, C, H + 2 * pad + 2, W + 2 * pad + 2), float("nan"), dtype=torch.float64)  # + 2: slices never run out
    xp[:, :, pad:pad + H, pad:pad + W] = x
    taps = torch.stack([xp[:, :, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride]
                        for r in range(3) for s in range(3)])
    return taps, ~torch.isnan(taps[:, 0, 0])


def max_pool_ref(x, stride, pad):
    taps, _ = pool_taps(x.double(), stride, pad)
    return torch.where(torch.isnan(taps), torch.full_like(taps, float("-inf")), taps).max(0).values


def avg_pool_ref(x, stride, pad, fmt, divisor9=False):
    """(ref rounded once to the storage format, the unrounded float64 mean, max|taps| per element, taps-in-image count [Ho, Wo])"""
    taps, inside = pool_taps(x.double(), stride, pad)
    t0 = torch.nan_to_num(taps, nan=0.0)
    n = inside.sum(0).double()
    mean = t0.sum(0) / (9.0 if divisor9 else n)
    return round16_f64(mean, fmt), mean, t0.abs().max(0).values, n


def avg_pool_emulate(x, stride, pad, fmt, divisor9=False):
    """the kernel's arithmetic restated in fp32: taps added in (r, s) order, times the fp32 reciprocal of the count, one rounding"""
    taps, inside = pool_taps(x.double(), stride, pad)
    acc = torch.zeros(taps.shape[1:], dtype=torch.float32)
    for t in range(9):
        acc = torch.where(inside[t], acc + torch.nan_to_num(taps[t], nan=0.0).float(), acc)  # fp32 + fp32, rounded to fp32
    n = inside.sum(0).float()
    inv = torch.ones((), dtype=torch.float32) / (torch.full_like(n, 9.0) if divisor9 else n)
    return r16(acc * inv, fmt)


def avg_verify(got, x, stride, pad, fmt, divisor9=False):
    """got float64 [B, C, Ho, Wo] against the reference -> dict(ratio = worst |got - ref| / bound, equal = share of elements that
    are the correctly rounded value, border_fail = share of the border elements with a non-zero reference that miss the bound)"""
    ref, _, tmax, n = avg_pool_ref(x, stride, pad, fmt, divisor9)
    bound = step16(ref, fmt) + 9.0 * 2.0 ** -24 * tmax
    err = (got.double() - ref).abs()
    err = torch.where(torch.isfinite(got.double()), err, torch.full_like(err, float("inf")))
    ratio = err / bound
    border = (n < 9)[None, None].expand_as(ref) & (ref != 0)
    return dict(ratio=ratio.max().item(), equal=(got.double() == ref).double().mean().item(),
                border_fail=(ratio[border] > 1).double().mean().item() if border.any() else 0.0)


def _pool(kind, H, W):
    mx, stride, pad = {"avg_s1p1": (False, 1, 1), "max_s1p1": (True, 1, 1), "max_s2p0": (True, 2, 0)}[kind]
    return dict(name="%s_%dx%d" % (kind, H, W), max=mx, stride=stride, pad=pad, H=H, W=W, B=2)


# every (stride, pad) the network uses; 7 x 9 and 8 x 8: corners, edges and interior differ; 5 x 5 at stride 2: a 2 x 2 output;
# 3 x 3 at pad 1: every output pixel but the centre lacks taps
POOL_CASES = [_pool(k, 7, 9) for k in ("avg_s1p1", "max_s1p1", "max_s2p0")] + \
             [_pool(k, 8, 8) for k in ("avg_s1p1", "max_s1p1", "max_s2p0")] + \
             [_pool("max_s2p0", 5, 5), _pool("avg_s1p1", 3, 3), _pool("max_s1p1", 3, 3)]
POOL_CHANNELS = (8, 40)
POOL_IN_PADS = (0, 24)
POOL_INPUTS = ("signed", "relu")


def pool_slices(C):
    """(out_off, out_ld): dense, and a slice of a 256-wide concat row - at column 224 (8 channels: 24 NaN columns stay to its
    right), or, for the 40 channels that do not fit there, the last 40 columns (a spill lands in the next row's column 0)"""
    return ((0, C), (224, 256) if 224 + C <= 256 else (256 - C, 256))


def pool_variants(c):
    """every (C, in_pad, (out_off, out_ld), input kind) of a pool case"""
    return [(C, ip, sl, kind) for C in POOL_CHANNELS for ip in POOL_IN_PADS for sl in pool_slices(C) for kind in POOL_INPUTS]


def pool_input(c, C, kind, fmt):
    """signed: N(0, 1.5^2); relu: max(N(0, 1), 0) - half of it exact zeros, as behind a ReLU. 16-bit values, float64."""
    g = _gen("pool %s %d %s" % (c["name"], C, kind))
    x = torch.randn(c["B"], C, c["H"], c["W"], generator=g)
    return r16(x * 1.5 if kind == "signed" else x.clamp_min(0.0), fmt)


def slice_report(buf, rows, off, width):
    """buf [rows + GUARD_ROWS, ld] as an entry point returns it -> (the slice [rows, width], number of non-NaN elements outside
    it - other columns, guard rows -, number of NaN elements inside it)"""
    assert buf.shape[0] == rows + GUARD_ROWS
    inside = torch.zeros(buf.shape, dtype=torch.bool)
    inside[:rows, off:off + width] = True
    return buf[:rows, off:off + width], int((~torch.isnan(buf[~inside])).sum()), int(torch.isnan(buf[inside]).sum())


def rows_to_nchw(rows, B, Ho, Wo):
    return rows.reshape(B, Ho, Wo, -1).permute(0, 3, 1, 2).contiguous()


# ================================================================================================ global average pool
GAVG_CASES = [dict(name="hw%d_c%d_pad%d" % (HW, C, ip), B=3, HW=HW, C=C, in_pad=ip)
              for HW in (64, 49) for C in (2048, 40) for ip in (0, 8)]


def gavg_input(c, fmt):
    g = _gen("gavg " + c["name"])
    x = torch.randn(c["B"], c["C"], c["HW"], generator=g)
    x[:, ::2] = x[:, ::2].clamp_min(0.0)  # even channels as behind a ReLU, odd channels signed (the sum cancels)
    return r16(x, fmt)


def gavg_emulate(x):
    acc = torch.zeros(x.shape[:2], dtype=torch.float32)
    for q in range(x.shape[2]):
        acc = acc + x[:, :, q].float()
    return (acc * (torch.ones((), dtype=torch.float32) / torch.tensor(float(x.shape[2]), dtype=torch.float32))).double()


def gavg_verify(got, x):
    """-> worst |got - mean| / (HW 2^-24 mean|x|) over the channels"""
    HW = x.shape[2]
    tol = HW * 2.0 ** -24 * x.abs().mean(2)
    err = (got.double() - x.mean(2)).abs()
    err = torch.where(torch.isfinite(got.double()), err, torch.full_like(err, float("inf")))
    return (err / tol.clamp_min(1e-300)).max().item()


# ================================================================================================ BasicConv2d forms
def _conv(name, B, Cin, H, W, N, KH, KW, stride=1, pad=(0, 0), in_ld=None, slc=None, balanced=True):
    Cpad, Nrun = -(-Cin // 32) * 32, -(-N // 32) * 32
    off, ld = slc if slc else (0, Nrun)
    return dict(name=name, B=B, Cin=Cin, H=H, W=W, N=N, KH=KH, KW=KW, stride=stride, pad=pad, in_ld=in_ld or Cpad, off=off,
                ld=ld, balanced=balanced)


# M = B Ho Wo is no multiple of 32 unless noted; B = 1 and B = 3 both occur. `balanced` cases (every other one) have signed
# inputs and centred BatchNorm shifts: about half of the outputs are clipped by the ReLU; the others follow a ReLU themselves.
CONV_CASES = [
    _conv("1x7_c128", 3, 128, 9, 11, 128, 1, 7, pad=(0, 3)),                                 # M 297
    _conv("1x7_c160", 1, 160, 9, 11, 160, 1, 7, pad=(0, 3), balanced=False),                 # M 99
    _conv("7x1_c128", 1, 128, 9, 11, 128, 7, 1, pad=(3, 0)),
    _conv("7x1_c160_last_slice", 3, 160, 9, 11, 192, 7, 1, pad=(3, 0), slc=(1856, 2048), balanced=False),
    _conv("1x3_c384", 3, 384, 8, 8, 384, 1, 3, pad=(0, 1)),                                  # M 192
    _conv("3x1_c384", 1, 384, 8, 8, 384, 3, 1, pad=(1, 0), balanced=False),                  # M 64
    _conv("5x5_c48", 2, 48, 7, 9, 64, 5, 5, pad=(2, 2)),                                     # Cpad 64; M 126
    _conv("3x3_valid_s1", 3, 32, 9, 11, 32, 3, 3, balanced=False),                           # 7 x 9: M 189
    _conv("3x3_valid_s2_17", 1, 96, 17, 17, 96, 3, 3, stride=2),                             # 17 -> 8: M 64
    _conv("3x3_valid_s2_11x9", 3, 64, 11, 9, 64, 3, 3, stride=2, balanced=False),            # 5 x 4: M 60
    _conv("stem_c3_s2", 3, 3, 15, 15, 32, 3, 3, stride=2),                                   # 3 -> 32 channels, 7 x 7: M 147
    _conv("1x1_c80_ld96", 1, 80, 7, 9, 192, 1, 1, in_ld=96, balanced=False),                 # M 63
    _conv("1x1_n80", 3, 64, 7, 9, 80, 1, 1),                                                 # columns 80 .. 95 zero
    _conv("1x1_n48", 1, 192, 7, 9, 48, 1, 1, balanced=False),                                # columns 48 .. 63 zero
    _conv("3x3_n32_dense", 3, 64, 7, 9, 32, 3, 3, pad=(1, 1), slc=(0, 32)),
    _conv("3x3_n32_at64_of288", 1, 64, 7, 9, 32, 3, 3, pad=(1, 1), slc=(64, 288), balanced=False),
    _conv("1x1_n32_at224_of256", 3, 192, 7, 9, 32, 1, 1, slc=(224, 256)),
    _conv("1x1_n192_last_slice", 1, 768, 7, 9, 192, 1, 1, slc=(1856, 2048), balanced=False),
    _conv("1x3_nan_pad", 1, 96, 8, 8, 64, 1, 3, pad=(0, 1), in_ld=128),                      # channels 96 .. 127 of the input NaN
]
CONV = {c["name"]: c for c in CONV_CASES}
assert len(CONV) == len(CONV_CASES)
# the forms that meet the channel-major K order (child process, CYCLEDIFF_KORDER=2): the valid 3 x 3 at stride 1 and 2 on odd
# sizes, the 3 -> 32 channel stem conv, 1 x 7 and 7 x 1
CONV_CHM = ["3x3_valid_s1", "3x3_valid_s2_17", "3x3_valid_s2_11x9", "stem_c3_s2", "1x7_c128", "1x7_c160", "7x1_c128",
            "7x1_c160_last_slice"]
CONV_TILES = (0, 3)  # 0: the launcher's choice (read back and reported), 3: the anchor tile of the GEMM sweep


def conv_out_hw(c):
    return ((c["H"] + 2 * c["pad"][0] - c["KH"]) // c["stride"] + 1, (c["W"] + 2 * c["pad"][1] - c["KW"]) // c["stride"] + 1)


def conv_operands(c, fmt):
    """x (16-bit values), the raw fp32 weight and the BatchNorm vectors: gamma of both signs, a quarter of var in [1e-5, 2e-3]
    (the eps = 1e-3 term decides the scale there)"""
    g = _gen("conv " + c["name"])
    B, Cin, H, W, N, KH, KW = (c[k] for k in ("B", "Cin", "H", "W", "N", "KH", "KW"))
    x = torch.randn(B, Cin, H, W, generator=g)
    x = x if c["balanced"] else x.clamp_min(0.0)
    w = torch.randn(N, Cin, KH, KW, generator=g) / (Cin * KH * KW) ** 0.5
    sign = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
    gamma = sign * (0.5 + torch.rand(N, generator=g))
    var = 0.5 + 1.5 * torch.rand(N, generator=g)
    small = torch.arange(N) % 4 == 1
    var[small] = 10.0 ** (-5.0 + 2.3 * torch.rand(int(small.sum()), generator=g))
    var[1 % N] = 1e-5
    mean = 0.3 * torch.randn(N, generator=g)
    beta = 0.3 * torch.randn(N, generator=g) + (0.0 if c["balanced"] else 0.5)
    return dict(x=r16(x, fmt).float(), w=w, gamma=gamma, beta=beta, mean=mean, var=var)


def fold_ref(o, eps=BN_EPS):
    """float64: (w gamma / sqrt(var + eps) [N, Cin, KH, KW], beta - mean sc [N], |beta| + |mean sc|)"""
    d = {k: v.double() for k, v in o.items()}
    sc = d["gamma"] / torch.sqrt(d["var"] + eps)
    return d["w"] * sc[:, None, None, None], d["beta"] - d["mean"] * sc, d["beta"].abs() + (d["mean"] * sc).abs()


def fold_emulate(o, fmt, eps=BN_EPS):
    """k_fold_bn restated in fp32 -> (weights [N, Cin, KH, KW] as 16-bit values, bias), float64"""
    sc = o["gamma"].float() / torch.sqrt(o["var"].float() + torch.tensor(eps, dtype=torch.float32))
    return r16(o["w"].float() * sc[:, None, None, None], fmt), (o["beta"].float() - o["mean"].float() * sc).double()


def fold_verify(c, o, wp, bo, fmt, eps=BN_EPS):
    """wp [Npad, KH, KW, Cpad], bo [Npad] as downloaded -> dict(w_ratio = worst |w - round16(fold)| / ulp16, b_ratio = worst
    |bias - fold| / (2^-21 (|beta| + |mean sc|)), nonzero = number of padding words that are not exactly zero)"""
    N, Cin = c["N"], c["Cin"]
    wf, bf, bmag = fold_ref(o, eps)
    wref = round16_f64(wf, fmt)
    got = wp[:N, :, :, :Cin].permute(0, 3, 1, 2).double()
    w_ratio = ((got - wref).abs() / step16(wref, fmt)).max().item()
    b_ratio = ((bo[:N].double() - bf).abs() / (2.0 ** -21 * bmag)).max().item()
    finite = bool(torch.isfinite(wp).all() and torch.isfinite(bo).all())
    nonzero = int((wp[:N, :, :, Cin:] != 0).sum() + (wp[N:] != 0).sum() + (bo[N:] != 0).sum())
    return dict(w_ratio=w_ratio if finite else float("inf"), b_ratio=b_ratio if finite else float("inf"), nonzero=nonzero)


def conv2d_f64(x, w, stride, pad):
    """float64 cross-correlation as a sum over explicitly shifted views: x [B, Cin, H, W], w [N, Cin, KH, KW], pad = (top, left),
    the same on the opposite sides"""
    x, w = x.double(), w.double()
    B, Cin, H, W = x.shape
    N, _, KH, KW = w.shape
    Ho, Wo = (H + 2 * pad[0] - KH) // stride + 1, (W + 2 * pad[1] - KW) // stride + 1
    xp = torch.zeros(B, Cin, H + 2 * pad[0], W + 2 * pad[1], dtype=torch.float64)
    xp[:, :, pad[0]:pad[0] + H, pad[1]:pad[1] + W] = x
    y = torch.zeros(B, N, Ho, Wo, dtype=torch.float64)
    for r in range(KH):
        for s in range(KW):
            v = xp[:, :, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride]
            y += torch.einsum("bchw,nc->bnhw", v, w[:, :, r, s])
    return y


def conv_ref(c, o, wp, bo):
    """the reference of a case from the DOWNLOADED packed weights wp [Npad, KH, KW, Cpad] and bias bo [Npad]: (ReLU output
    [B, Nrun, Ho, Wo] over all round_up(N, 32) columns the GEMM writes, share of the first N columns the ReLU clips)"""
    Nrun = -(-c["N"] // 32) * 32
    w = wp[:Nrun, :, :, :c["Cin"]].permute(0, 3, 1, 2)
    pre = conv2d_f64(o["x"], w, c["stride"], c["pad"]) + bo[:Nrun].double()[None, :, None, None]
    return pre.clamp_min(0.0), (pre[:, :c["N"]] <= 0).double().mean().item()


def bn_conv_ref(o, stride, pad, eps=BN_EPS):
    """conv -> BatchNorm (running statistics) -> ReLU in float64 without the fold (the host test holds it against torch modules)"""
    d = {k: v.double() for k, v in o.items()}
    y = conv2d_f64(d["x"], d["w"], stride, pad)
    v = lambda t: t[None, :, None, None]
    return ((y - v(d["mean"])) / torch.sqrt(v(d["var"]) + eps) * v(d["gamma"]) + v(d["beta"])).clamp_min(0.0)


def check_basic_conv(c, o, buf, wp, bo, fmt):
    """one run of cd_op_basic_conv against the references -> (failures, figures)"""
    failures = []
    N, Nrun = c["N"], -(-c["N"] // 32) * 32
    Ho, Wo = conv_out_hw(c)
    M = c["B"] * Ho * Wo
    # the fold, through the weights and the bias the launch read
    f = fold_verify(c, o, wp, bo, fmt)
    if not (f["w_ratio"] <= 1.0 and f["b_ratio"] <= 1.0):
        failures.append(("fold", f))
    if f["nonzero"]:
        failures.append(("padding channels / rows / bias entries that are not zero", f["nonzero"]))
    f5 = fold_verify(c, o, wp, bo, fmt, eps=1e-5)
    if not (f5["w_ratio"] > 1.0 and f5["b_ratio"] > 1.0):
        failures.append(("the eps = 1e-5 reference was not rejected", f5))
    # the launch
    rows, outside, nan_inside = slice_report(buf.double(), M, c["off"], Nrun)
    if outside or nan_inside:
        failures.append(("written outside the slice: %d, NaN inside: %d" % (outside, nan_inside),))
        return failures, dict(fold_w=f["w_ratio"], fold_b=f["b_ratio"])
    ref, clipped = conv_ref(c, o, wp, bo)
    got = rows_to_nchw(rows, c["B"], Ho, Wo)
    if c["balanced"] and not 0.3 < clipped < 0.7:  # the clip is exercised on both sides
        failures.append(("share of outputs the ReLU clips", clipped))
    if Nrun > N and not bool((got[:, N:] == 0).all()):
        failures.append(("padding columns [N, round_up(N, 32)) are not exact zeros",))
    es = gs.err_stats(got, ref)
    if not gs.within_bounds(es):
        failures.append(("float64 bounds", es))
    return failures, dict(rel_to_max=es["rel_to_max"], mean_rel=es["mean_rel"], max_abs=es["max_abs"], fold_w=f["w_ratio"],
                          fold_b=f["b_ratio"], clipped=clipped)
