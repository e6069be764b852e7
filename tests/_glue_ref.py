"""References for the single-kernel tests of the small HBM-bound kernels of csrc/elementwise.hip: tests/test_glue_host.py (CPU)
and tests/test_gpu_glue.py (GPU, through the bare entry points cd_op_layout / cd_op_resample16 / cd_op_copy_rows16 /
cd_op_vec_linear / cd_op_tokens / cd_op_posterior_sample / cd_op_vq_quantize: the caller's device bytes in, one launch, the
kernel's bytes out - no staging kernel on either side).

For every kernel, in plain torch on the host:
  * the operands exactly as the device sees them (16-bit tensors are int16 storage words; every padding column of a strided
    operand holds NaN, every output buffer starts as a sentinel and has a guard of sentinel words behind it);
  * `*_emulate`: the kernel's arithmetic in fp32, through the kernel's own flat-index decode - and, with `mutant=...`, a subtly
    wrong kernel;
  * `*_verify(o, got)` -> dict(ratio, mismatch): ratio = worst |got - float64 reference| / tolerance over the toleranced words,
    mismatch = number of words that fail an exact check. The GPU test asks ratio <= 1 and mismatch == 0, the host test asks
    ratio <= 0.5 of every emulation and ratio >= 5 or mismatch > 0 of every mutant.

Exact checks (words compared): k_upsample2, k_copy_strided_bf16 (destination columns >= cols keep the sentinel), k_gather_eot,
k_nhwc_to_nchw from 16 bits with scale 1 / shift 0 (widening is exact), k_nchw_to_nhwc with scale 1 / shift 0 (the saturating
round-to-nearest-even, round16), k_embed_tokens and k_vit_tokens (one IEEE fp32 addition and one conversion leave no freedom),
every zero-filled padding channel, every dup copy, every guard.

Tolerances against float64, step16(v) = the storage format's step at |v| with its subnormal floor:
  k_avgpool2          1 step16(max(|got|, |ref|)) + 3 x 2^-24 mean|x| over the four taps
  layout, to 16 bits  1 step16 + 2^-23 (|x scale| + |shift|)
  layout, to fp32     2^-23 (|v scale| + |shift|)        (the compiler may or may not contract the multiply-add)
  k_vec_linear        (ceil(K / 64) + 16) x 2^-24 x (sum_k |act(x_k) w_k| + |bias|), x 1.1 with silu_out: the terms a lane adds,
                      six shuffle additions, the bias, SiLU's expf (|SiLU'| <= 1.1)
  k_posterior_sample  8 x 2^-24 |scale| (|mean| + |sd noise|)
  k_vq_quantize       the argmin of (z^2 + e^2) - 2 z.e in fp32 against float64 squared distances. A vector is decidable when the
                      float64 gap between its two nearest (distinct) codes exceeds 2 (2 zc + 4) 2^-24 (|z| + max|e|)^2: there the
                      code must be the float64 one; elsewhere the chosen code's float64 distance must lie within that bound of the
                      minimum. At most 1 % of a case's vectors may be undecidable (VQ_CAP; asserted on the host per case). Given
                      the code, channels < zc are the 16-bit rounding of fp32 z + (e - z): bit for bit with in_mul = 1, within one
                      step16 otherwise (the z in_mul product may be contracted); channels zc .. Cpad - 1 are the zero word.
                      Identical codebook rows cannot be told apart in the output and count as one code (the lowest index). Exact
                      fp32 ties that can be seen: z = 0 against a codebook of mirrored rows +e / -e, where e^2 and z.e = +-0 have
                      the same bits for both - the first of the pair must come out (case "ties").

Worst err / tol measured on MI355X (fp16 build; rows glue/... of the parity report):
  kernel                               cases   worst err / tol
  k_nchw_to_nhwc, scale 1 shift 0        5     exact (0 mismatching words), +-70000 -> +-65504
  k_nchw_to_nhwc, 1/0.18215 and 0.25     2     0.496  (the 16-bit rounding itself is 0.5 step16 of the 1 allowed)
  k_nhwc_to_nchw, scale 1 shift 0        4     exact
  k_nhwc_to_nchw, 0.5 and 0.5            2     0.486  (fp32 rows; 0.000 from 16-bit rows, where the sum is exact)
  k_avgpool2                             6     0.500  (one 16-bit rounding; the fp32 sum adds < 0.001)
  k_upsample2, k_copy_strided_bf16       5     exact
  k_vec_linear                           9     0.065  (K = 32; 0.017 on the scalar path at K = 322, <= 0.01 at K >= 1024)
  k_embed_tokens, k_vit_tokens, k_gather_eot  5   exact
  k_posterior_sample                     6     0.321
  k_vq_quantize                         10     0 wrong codes, 0 mismatching words (0.46 % undecidable at 8192 x 3)
"""
import functools
import math

import torch

FMTS = ("fp16", "bf16")
NAN16 = -1        # 0xFFFF: NaN in fp16 and in bf16
SENT16 = 0x5A5A   # what every 16-bit output buffer starts as
SENT32 = 12345.0  # ... and every fp32 one
GUARD = 64        # sentinel words behind every output
VQ_CAP = 0.01


def lib_fmt():
    from cycle_diffusion_amd import _ffi
    return "fp16" if _ffi.load_library().cd_act_format() == 1 else "bf16"


def _dt(fmt):
    return torch.float16 if fmt == "fp16" else torch.bfloat16


def round16(v, fmt):
    """fp32 -> the storage format: round-to-nearest-even; the fp16 build saturates at +-65504 (csrc/common.h f2bf)"""
    v = v.float()
    if fmt == "fp16":
        v = v.clamp(-65504.0, 65504.0)
    return v.to(_dt(fmt))


def to16(v, fmt):
    return round16(v, fmt).view(torch.int16)


def from16(w, fmt):
    return w.view(_dt(fmt)).float()


def step16(v, fmt):
    v = v.double().abs()
    emin, mant = (-14, 10) if fmt == "fp16" else (-126, 7)
    e = (torch.frexp(v)[1] - 1).double()
    e = torch.where(v == 0, torch.full_like(e, emin), e).clamp_min(emin)
    return torch.pow(2.0, e - mant)


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _gen(name):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31))


def _names(cases):
    d = {c["name"]: c for c in cases}
    assert len(d) == len(cases)
    return d


def _result(ratio=0.0, mismatch=0, **kw):
    return dict(ratio=float(ratio), mismatch=int(mismatch), **kw)


def _ratio(got, ref, tol):
    """worst |got - ref| / tol; a non-finite word counts as infinitely far"""
    r = (got.double() - ref).abs() / tol
    r = torch.where(torch.isfinite(got.double()), r, torch.full_like(r, float("inf")))
    return r.max().item() if r.numel() else 0.0


def silu32(x):
    return x / (1.0 + torch.exp(-x))  # csrc/common.h silu_acc, in the dtype of x


# ================================================================================== k_nchw_to_nhwc (fp32 NCHW -> 16-bit rows)
def _n2h(name, B, C, Cpad, HW, dup=0, scale=1.0, shift=0.0, sat=False):
    return dict(name=name, B=B, C=C, Cpad=Cpad, HW=HW, dup=dup, scale=scale, shift=shift, sat=sat)


_AFF = dict(scale=1.0 / 0.18215, shift=0.25)
N2H_CASES = [
    _n2h("c3_pad32_hw35", 2, 3, 32, 35),
    _n2h("c3_pad32_hw35_dup", 2, 3, 32, 35, dup=1),
    _n2h("c3_pad32_hw35_affine", 2, 3, 32, 35, **_AFF),
    _n2h("c3_pad32_hw35_dup_affine", 2, 3, 32, 35, dup=1, **_AFF),
    _n2h("rows_b77_c8", 77, 8, 8, 1),                 # the rows form of capi.hip: HW = 1, no padding
    _n2h("saturate_70000", 2, 3, 32, 35, sat=True),   # fp16 build: +-70000 -> +-65504
    _n2h("wrap_hw16640", 2, 4, 32, 128 * 130),        # 1 064 960 words > 4096 x 256 threads: the grid-stride loop wraps
]
N2H = _names(N2H_CASES)


@functools.lru_cache(maxsize=None)
def n2h_build(name):
    c = N2H[name]
    g = _gen("n2h" + name)
    x = torch.randn(c["B"], c["C"], c["HW"], generator=g) * (1.0 + torch.arange(c["C"]).float())[None, :, None]
    if c["sat"]:
        x.view(-1)[:6] = torch.tensor([70000.0, -70000.0, 65519.0, -65519.0, 65520.0, 65504.0])
    return dict(case=c, x=x.contiguous())


def n2h_emulate(o, fmt, fused=False, mutant=None):
    """-> int16 [(1 + dup) B HW Cpad + GUARD], through the kernel's flat-index decode"""
    c = o["case"]
    B, C, Cpad, HW = c["B"], c["C"], c["Cpad"], c["HW"]
    n = B * HW * Cpad
    i = torch.arange(n)
    ch = i % Cpad
    bp = i // Cpad
    b, pix = bp // HW, bp % HW
    xf = o["x"].reshape(-1)
    src = (b * (Cpad if mutant == "cpad_for_c" else C) + ch) * HW + pix
    xv = xf[src % xf.numel()]  # (a mutant's reads past the tensor are folded back into it)
    s, t = torch.tensor(c["scale"], dtype=torch.float32), torch.tensor(c["shift"], dtype=torch.float32)
    v = (xv.double() * s.double() + t.double()).float() if fused else xv * s + t
    w = to16(torch.where(ch < C, v, torch.zeros_like(v)), fmt)
    out = torch.full(((1 + c["dup"]) * n + GUARD,), SENT16, dtype=torch.int16)
    if mutant == "pad_not_zeroed":
        out[:n][ch < C] = w[ch < C]
    else:
        out[:n] = w
    if c["dup"]:
        off = B * HW * C if mutant == "dup_offset" else n
        out[off:off + n] = w
    return out


def n2h_verify(o, got, fmt):
    c = o["case"]
    B, C, Cpad, HW = c["B"], c["C"], c["Cpad"], c["HW"]
    n = B * HW * Cpad
    first = got[:n].view(B, HW, Cpad)
    mism = (first[..., C:] != 0).sum().item() + (got[(1 + c["dup"]) * n:] != SENT16).sum().item()
    if c["dup"]:
        mism += (got[n:2 * n] != got[:n]).sum().item()
    xr = o["x"].permute(0, 2, 1)  # [B, HW, C]
    if c["scale"] == 1.0 and c["shift"] == 0.0:
        return _result(0.0, mism + (first[..., :C] != to16(xr, fmt)).sum().item())
    s, t = f32(c["scale"]), f32(c["shift"])
    ref = xr.double() * s + t
    g = from16(first[..., :C].contiguous(), fmt)
    tol = step16(torch.maximum(g.double().abs(), ref.abs()), fmt) + 2.0 ** -23 * ((xr.double() * s).abs() + abs(t))
    return _result(_ratio(g, ref, tol), mism)


# ================================================================================== k_nhwc_to_nchw (rows -> fp32 NCHW)
def _h2n(name, B, C, ld, HW, src_f32=0, scale=1.0, shift=0.0):
    return dict(name=name, B=B, C=C, ld=ld, HW=HW, src_f32=src_f32, scale=scale, shift=shift)


H2N_CASES = [
    _h2n("h16_c80_ld96", 2, 80, 96, 35),
    _h2n("f32_c5_ld8", 2, 5, 8, 35, src_f32=1),
    _h2n("h16_c80_ld96_affine", 2, 80, 96, 35, scale=0.5, shift=0.5),
    _h2n("f32_c5_ld8_affine", 2, 5, 8, 35, src_f32=1, scale=0.5, shift=0.5),
    _h2n("h16_hw1_b77", 77, 8, 8, 1),
    _h2n("wrap_hw262656", 1, 4, 8, 512 * 513),  # 1 050 624 elements > 4096 x 256 threads
]
H2N = _names(H2N_CASES)


@functools.lru_cache(maxsize=None)
def h2n_build(name, fmt):
    """x: the source rows as stored, [B HW][ld] int16 words (or fp32), NaN in the columns >= C"""
    c = H2N[name]
    g = _gen("h2n" + name)
    v = torch.randn(c["B"] * c["HW"], c["C"], generator=g) * (1.0 + torch.arange(c["C"]).float())[None, :]
    if c["src_f32"]:
        x = torch.full((c["B"] * c["HW"], c["ld"]), float("nan"))
        x[:, :c["C"]] = v
    else:
        x = torch.full((c["B"] * c["HW"], c["ld"]), NAN16, dtype=torch.int16)
        x[:, :c["C"]] = to16(v, fmt)
        v = from16(x[:, :c["C"]].contiguous(), fmt)
    return dict(case=c, x=x.contiguous(), v=v)  # v: the fp32 values of the valid columns


def h2n_emulate(o, fmt, fused=False, mutant=None):
    c = o["case"]
    B, C, HW, ld = c["B"], c["C"], c["HW"], c["ld"]
    n = B * C * HW
    i = torch.arange(n)
    pix, bc = i % HW, i // HW
    Cd = ld if mutant == "ld_for_c" else C
    ch, b = bc % Cd, bc // Cd
    xf = (o["x"] if c["src_f32"] else from16(o["x"], fmt)).reshape(-1)
    v = xf[(((b * HW + pix) * ld) + ch) % xf.numel()]
    s, t = torch.tensor(c["scale"], dtype=torch.float32), torch.tensor(c["shift"], dtype=torch.float32)
    y = (v.double() * s.double() + t.double()).float() if fused else v * s + t
    return torch.cat([y, torch.full((GUARD,), SENT32)])


def h2n_verify(o, got, fmt):
    c = o["case"]
    B, C, HW = c["B"], c["C"], c["HW"]
    n = B * C * HW
    mism = (got[n:] != SENT32).sum().item()
    v = o["v"].view(B, HW, C).permute(0, 2, 1).contiguous()  # [B, C, HW]
    g = got[:n].view(B, C, HW)
    if c["scale"] == 1.0 and c["shift"] == 0.0:
        return _result(0.0, mism + (g.view(torch.int32) != v.view(torch.int32)).sum().item())
    s, t = f32(c["scale"]), f32(c["shift"])
    ref = v.double() * s + t
    tol = 2.0 ** -23 * ((v.double() * s).abs() + abs(t))
    return _result(_ratio(g, ref, tol), mism)


# ================================================================================== k_avgpool2 / k_upsample2 (16-bit NHWC)
def _rs(name, op, B, H, W, C, scale=1.0):
    return dict(name=name, op=op, B=B, H=H, W=W, C=C, scale=scale)


RESAMPLE_CASES = [
    _rs("pool_b2_6x10_c40", "avgpool", 2, 6, 10, 40),
    _rs("pool_b2_7x5_c40", "avgpool", 2, 7, 5, 40),              # odd H and W: the last row and column are ignored
    _rs("pool_b2_6x10_c40_3e-5", "avgpool", 2, 6, 10, 40, 3e-5),  # fp16: subnormal inputs and results
    _rs("pool_b2_7x5_c40_3e-5", "avgpool", 2, 7, 5, 40, 3e-5),
    _rs("pool_b2_6x10_c40_200", "avgpool", 2, 6, 10, 40, 200.0),
    _rs("pool_wrap_258x258_c512", "avgpool", 1, 258, 258, 512),   # 1 065 024 vectors > 4096 x 256 threads
    _rs("up_b2_3x5_c40", "upsample", 2, 3, 5, 40),
    _rs("up_wrap_65x65_c512", "upsample", 1, 65, 65, 512),        # 1 081 600 vectors
]
RESAMPLE = _names(RESAMPLE_CASES)


def resample_out_hw(c):
    return (c["H"] // 2, c["W"] // 2) if c["op"] == "avgpool" else (2 * c["H"], 2 * c["W"])


@functools.lru_cache(maxsize=4)
def resample_build(name, fmt):
    c = RESAMPLE[name]
    g = _gen("rs" + name)
    x = to16(torch.randn(c["B"], c["H"], c["W"], c["C"], generator=g) * c["scale"], fmt)
    return dict(case=c, x=x)


def _resample_index(c, mutant):
    """the kernels' decode of the flat vector index -> (source word index of tap (0, 0) [n, 8], destination word index [n, 8])"""
    B, H, W, C = c["B"], c["H"], c["W"], c["C"]
    Ho, Wo = resample_out_hw(c)
    nvec = C // 8
    i = torch.arange(B * Ho * Wo * nvec)
    v, t = i % nvec, i // nvec
    Wd = W if mutant == "w_for_wo" else Wo
    ox, t = t % Wd, t // Wd
    oy, b = t % Ho, t // Ho
    e = torch.arange(8)[None, :]
    dst = ((((b * Ho + oy) * Wo + ox) * C + v * 8)[:, None] + e) % (B * Ho * Wo * C)
    if c["op"] == "avgpool":
        src = ((b * H + oy * 2) * W + ox * 2) * C + v * 8
    else:
        src = ((b * H + oy // 2) * W + ox // 2) * C + v * 8
    return src[:, None] + e, dst


def resample_emulate(o, fmt, mutant=None):
    c = o["case"]
    Ho, Wo = resample_out_hw(c)
    src, dst = _resample_index(c, mutant)
    xw = o["x"].reshape(-1)
    N = xw.numel()
    out = torch.full((c["B"] * Ho * Wo * c["C"] + GUARD,), SENT16, dtype=torch.int16)
    if c["op"] == "upsample":
        out[dst.reshape(-1)] = xw[src.reshape(-1) % N]
        return out
    xf = from16(xw, fmt)
    a = torch.zeros(src.shape, dtype=torch.float32)
    for dy in range(2):
        for dx in range(2):
            if mutant == "3_of_4_taps" and dy == 1 and dx == 1:
                continue
            a = a + xf[(src + (dy * c["W"] + dx) * c["C"]).reshape(-1) % N].view(src.shape)
    out[dst.reshape(-1)] = to16(a * 0.25, fmt).reshape(-1)
    return out


def avgpool_ref64(xf):
    """[B, H, W, C] float64 -> (mean, mean of |x|) over the 2 x 2 windows that fit; the last odd row / column is ignored"""
    H2, W2 = xf.shape[1] // 2 * 2, xf.shape[2] // 2 * 2
    taps = [xf[:, dy:H2:2, dx:W2:2] for dy in range(2) for dx in range(2)]
    return sum(taps) / 4.0, sum(t.abs() for t in taps) / 4.0


def upsample_ref(x):
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


def resample_verify(o, got, fmt):
    c = o["case"]
    Ho, Wo = resample_out_hw(c)
    n = c["B"] * Ho * Wo * c["C"]
    mism = (got[n:] != SENT16).sum().item()
    g = got[:n].view(c["B"], Ho, Wo, c["C"])
    if c["op"] == "upsample":
        return _result(0.0, mism + (g != upsample_ref(o["x"])).sum().item())
    ref, mabs = avgpool_ref64(from16(o["x"], fmt).double())
    gf = from16(g, fmt)
    tol = step16(torch.maximum(gf.double().abs(), ref.abs()), fmt) + 3.0 * 2.0 ** -24 * mabs
    return _result(_ratio(gf, ref, tol), mism)


# ================================================================================== k_copy_strided_bf16
COPY_CASES = [
    dict(name="r77_c40_lds48_ldd64", rows=77, cols=40, lds=48, ldd=64, tail=0),
    dict(name="dup_rows_n21_tail7_c40", rows=21, cols=40, lds=40, ldd=40, tail=7),  # unet_openai.hip dup_rows: two launches
    dict(name="wrap_r16400_c512", rows=16400, cols=512, lds=512, ldd=512, tail=0),  # 1 049 600 vectors
]
COPY = _names(COPY_CASES)


@functools.lru_cache(maxsize=None)
def copy_build(name):
    c = COPY[name]
    g = _gen("cp" + name)
    src = torch.full((c["rows"], c["lds"]), NAN16, dtype=torch.int16)
    src[:, :c["cols"]] = torch.randint(-32768, 32768, (c["rows"], c["cols"]), generator=g).to(torch.int16)  # any 16 bits
    return dict(case=c, src=src.contiguous())


def copy_launches(c):
    """(first source row, first destination row, rows) of every launch"""
    out = [(0, 0, c["rows"])]
    if c["tail"]:
        out.append((c["rows"] - c["tail"], c["rows"], c["tail"]))
    return out


def copy_emulate(o, mutant=None):
    c = o["case"]
    nvec = c["cols"] // 8
    dst = torch.full(((c["rows"] + c["tail"]) * c["ldd"] + GUARD,), SENT16, dtype=torch.int16)
    sw = o["src"].reshape(-1)
    for r0, d0, rows in copy_launches(c):
        i = torch.arange(rows * nvec)
        r, v = i // nvec, i % nvec
        if mutant == "ldd_for_lds":
            s = (r0 + r) * c["ldd"] + v * 8
        else:
            s = (r0 + r) * c["lds"] + v * 8
        if mutant == "tail_from_row0" and r0:
            s = r * c["lds"] + v * 8
        e = torch.arange(8)[None, :]
        dst[(((d0 + r) * c["ldd"] + v * 8)[:, None] + e).reshape(-1)] = sw[(s[:, None] + e).reshape(-1) % sw.numel()]
    return dst


def copy_verify(o, got):
    c = o["case"]
    want = torch.full((c["rows"] + c["tail"], c["ldd"]), SENT16, dtype=torch.int16)
    want[:c["rows"], :c["cols"]] = o["src"][:, :c["cols"]]
    if c["tail"]:
        want[c["rows"]:, :c["cols"]] = o["src"][c["rows"] - c["tail"]:, :c["cols"]]
    want = torch.cat([want.reshape(-1), torch.full((GUARD,), SENT16, dtype=torch.int16)])
    return _result(0.0, (got != want).sum().item())


# ================================================================================== k_vec_linear
def _vl(name, B, K, N, silu_in, silu_out, ldx=None, ldy=None, bias=True):
    return dict(name=name, B=B, K=K, N=N, silu_in=silu_in, silu_out=silu_out, ldx=ldx or K, ldy=ldy or N, bias=bias)


VEC_CASES = [
    _vl("b3_k4_n5", 3, 4, 5, 0, 0),                            # one vector; B N = 15 is no multiple of the 4 waves of a block
    _vl("b2_k32_n128_silu_out", 2, 32, 128, 0, 1, ldy=132),    # the tiny networks' form
    _vl("b2_k1024_n9_silu_both", 2, 1024, 9, 1, 1, ldx=1028),  # all four segments, exactly one trip
    _vl("b2_k1028_n6", 2, 1028, 6, 0, 0),                      # second trip, one lane
    _vl("b3_k1280_n37_silu_in", 3, 1280, 37, 1, 0, ldy=40),    # second trip, segment 0 only: the SD width
    _vl("b2_k37_n6_silu_in", 2, 37, 6, 1, 0, ldx=41),          # scalar path (K % 4 != 0)
    _vl("b1_k322_n3", 1, 322, 3, 0, 0),                        # scalar path, six trips
    _vl("b2_k36_n7_ldx38", 2, 36, 7, 0, 0, ldx=38, ldy=9),     # K % 4 == 0, scalar because of ldx
    _vl("b2_k64_n5_nobias_silu_in", 2, 64, 5, 1, 0, bias=False),
]
VEC = _names(VEC_CASES)


@functools.lru_cache(maxsize=None)
def vec_build(name):
    c = VEC[name]
    g = _gen("vl" + name)
    x = torch.full((c["B"], c["ldx"]), float("nan"))
    x[:, :c["K"]] = torch.randn(c["B"], c["K"], generator=g) * 1.5 + 0.3
    W = torch.randn(c["N"], c["K"], generator=g) / math.sqrt(c["K"]) + 0.5 / c["K"]
    bias = (torch.randn(c["N"], generator=g) * 0.5 + 1.0) if c["bias"] else None
    return dict(case=c, x=x.contiguous(), W=W.contiguous(), bias=bias)


def _k_mask(c, mutant):
    """which k the (mutated) kernel adds"""
    K = c["K"]
    keep = torch.ones(K, dtype=torch.bool)
    if (K % 4 == 0) and (c["ldx"] % 4 == 0):
        v = torch.arange(K) // 4
        if mutant == "no_segment_3":
            keep = (v % 256) // 64 != 3
        if mutant == "no_second_trip":
            keep = v < 256
    return keep


def vec_ref64(o, mutant=None):
    """-> (y [B, N], sum_k |act(x_k) w_k| + |bias|) in float64"""
    c = o["case"]
    si, so = c["silu_in"], c["silu_out"]
    if mutant == "silu_wrong_side":
        si, so = so, si
    x = o["x"][:, :c["K"]].double()
    a = x * torch.sigmoid(x) if si else x
    a = a * _k_mask(c, mutant).double()[None, :]
    W = o["W"].double()
    y = a @ W.T
    mag = a.abs() @ W.abs().T
    if o["bias"] is not None and mutant != "no_bias":
        y = y + o["bias"].double()[None, :]
        mag = mag + o["bias"].double().abs()[None, :]
    return (y * torch.sigmoid(y) if so else y), mag


def vec_emulate(o):
    """fp32 in the kernel's order: per lane its vectors / elements ascending (four segment sums on the vector path), the
    segment sums pairwise, the butterfly over 64 lanes, bias, SiLU. -> [B, ldy] with the sentinel in the columns >= N"""
    c = o["case"]
    B, K, N = c["B"], c["K"], c["N"]
    x = o["x"][:, :K]
    a = silu32(x) if c["silu_in"] else x
    p = a[:, None, :] * o["W"][None, :, :]  # [B, N, K] fp32 products
    if (K % 4 == 0) and (c["ldx"] % 4 == 0):
        nv = K // 4
        nvp = (nv + 255) // 256 * 256
        q = torch.zeros(B, N, nvp, 4)
        q[:, :, :nv] = p.view(B, N, nv, 4)
        d = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]          # one vector's dot product, left to right
        d = d.view(B, N, nvp // 256, 4, 64)                            # [trip][segment u][lane]
        a4 = torch.zeros(B, N, 4, 64)
        for trip in range(nvp // 256):
            a4 = a4 + d[:, :, trip]
        acc = (a4[:, :, 0] + a4[:, :, 1]) + (a4[:, :, 2] + a4[:, :, 3])
    else:
        Kp = (K + 63) // 64 * 64
        q = torch.zeros(B, N, Kp)
        q[:, :, :K] = p
        q = q.view(B, N, Kp // 64, 64)
        acc = torch.zeros(B, N, 64)
        for trip in range(Kp // 64):
            acc = acc + q[:, :, trip]
    lane = torch.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, lane ^ s]
    v = acc[:, :, 0]
    if o["bias"] is not None:
        v = v + o["bias"][None, :]
    if c["silu_out"]:
        v = silu32(v)
    y = torch.full((B, c["ldy"]), SENT32)
    y[:, :N] = v
    return y


def vec_tol(o):
    c = o["case"]
    _, mag = vec_ref64(o)
    return (math.ceil(c["K"] / 64) + 16) * 2.0 ** -24 * mag * (1.1 if c["silu_out"] else 1.0)


def vec_verify(o, got):
    """got [B, ldy] (float32 or float64)"""
    c = o["case"]
    ref, _ = vec_ref64(o)
    mism = (got[:, c["N"]:] != SENT32).sum().item()
    return _result(_ratio(got[:, :c["N"]], ref, vec_tol(o)), mism)


# ================================================================================== k_embed_tokens / k_vit_tokens / k_gather_eot
TOKEN_CASES = [
    dict(name="embed_b2_l77_d24_v50", op="embed", B=2, L=77, D=24, vocab=50),
    dict(name="embed_wrap_b110_l77_d1024", op="embed", B=110, L=77, D=1024, vocab=50),  # 1 084 160 vectors
    dict(name="vit_b2_t49_d24", op="vit", B=2, L=49, D=24, vocab=0),
    dict(name="eot_b3_l77_d40", op="eot", B=3, L=77, D=40, vocab=0),
    dict(name="eot_b3_l77_d1280", op="eot", B=3, L=77, D=1280, vocab=0),               # above the block's 256 threads
]
TOKENS = _names(TOKEN_CASES)


@functools.lru_cache(maxsize=4)
def tokens_build(name, fmt):
    c = TOKENS[name]
    g = _gen("tk" + name)
    B, L, D = c["B"], c["L"], c["D"]
    o = dict(case=c)
    if c["op"] == "embed":
        ids = torch.randint(0, c["vocab"], (B, L), generator=g, dtype=torch.int32)
        ids[0, 3], ids[0, 4], ids[-1, 5], ids[-1, L - 1] = -1, c["vocab"], c["vocab"] + 5, c["vocab"] - 1
        o.update(ids=ids, tok=torch.randn(c["vocab"], D, generator=g), pos=torch.randn(L, D, generator=g) * 0.3)
    elif c["op"] == "vit":
        o.update(x16=to16(torch.randn(B, L, D, generator=g), fmt), tok=torch.randn(D, generator=g),
                 pos=torch.randn(L + 1, D, generator=g) * 0.3)
    else:
        ids = torch.randint(1, 1000, (B, L), generator=g, dtype=torch.int32)
        ids[0, 0] = 49407                      # the maximum at position 0 ...
        ids[1, L - 1] = 49407                  # ... at L - 1 ...
        ids[2, 10] = ids[2, 50] = 49407        # ... and tied: the first wins
        o.update(ids=ids, x16=torch.randint(-32768, 32768, (B, L, D), generator=g).to(torch.int16))
    return o


def tokens_out_words(c):
    return c["B"] * {"embed": c["L"], "vit": c["L"] + 1, "eot": 1}[c["op"]] * c["D"]


def tokens_emulate(o, fmt, mutant=None):
    c = o["case"]
    B, L, D = c["B"], c["L"], c["D"]
    if c["op"] == "embed":
        ids = o["ids"].long()
        ids = ids.clamp(0, c["vocab"] - 1)
        l = torch.arange(L)[None, :].expand(B, L)
        if mutant == "pos_by_bl":  # pos[b L + l]: rows past the table are read as its last row
            l = (torch.arange(B)[:, None] * L + l).clamp_max(L - 1)
        w = to16(o["tok"][ids] + o["pos"][l], fmt)
    elif c["op"] == "vit":
        rows = torch.cat([o["tok"][None, None, :].expand(B, 1, D), from16(o["x16"], fmt)], 1)
        t = torch.arange(L + 1)
        if mutant == "pos_by_bl":
            w = to16(rows + o["pos"][(torch.arange(B)[:, None] * (L + 1) + t[None, :]).clamp_max(L)], fmt)
        else:
            w = to16(rows + o["pos"][None], fmt)
    else:
        ids = o["ids"]
        if mutant == "last_maximum":
            best = L - 1 - ids.flip(1).argmax(1)
        else:
            best = ids.argmax(1)
        w = o["x16"][torch.arange(B), best]
    return torch.cat([w.reshape(-1), torch.full((GUARD,), SENT16, dtype=torch.int16)])


def tokens_verify(o, got, fmt):
    """exact; the expected words are written here a second time, not through the emulation's index arithmetic"""
    c = o["case"]
    B, L, D = c["B"], c["L"], c["D"]
    if c["op"] == "embed":
        want = torch.empty(B, L, D, dtype=torch.int16)
        for b in range(B):
            rows = o["tok"][o["ids"][b].long().clamp(0, c["vocab"] - 1)]
            want[b] = to16(rows + o["pos"], fmt)  # one IEEE fp32 addition, one conversion
    elif c["op"] == "vit":
        want = torch.empty(B, L + 1, D, dtype=torch.int16)
        want[:, 0] = to16(o["tok"] + o["pos"][0], fmt)
        want[:, 1:] = to16(from16(o["x16"], fmt) + o["pos"][1:][None], fmt)
    else:
        want = torch.empty(B, D, dtype=torch.int16)
        for b in range(B):
            row = o["ids"][b].tolist()
            want[b] = o["x16"][b, row.index(max(row))]
    want = torch.cat([want.reshape(-1), torch.full((GUARD,), SENT16, dtype=torch.int16)])
    return _result(0.0, (got != want).sum().item())


# ================================================================================== k_posterior_sample
def _ps(name, B, zc, HW, ld, use_mean=0):
    return dict(name=name, B=B, zc=zc, HW=HW, ld=ld, use_mean=use_mean, scale=0.18215)


POST_CASES = [
    _ps("zc3_ld6", 2, 3, 35, 6), _ps("zc3_ld10", 2, 3, 35, 10), _ps("zc4_ld8", 2, 4, 35, 8), _ps("zc4_ld12", 2, 4, 35, 12),
    _ps("zc4_ld12_use_mean", 2, 4, 35, 12, use_mean=1),  # the log-variance half is NaN and noise NULL: nothing of either is read
    _ps("wrap_zc4_hw262656", 1, 4, 512 * 513, 8),        # 1 050 624 elements
]
POST = _names(POST_CASES)


@functools.lru_cache(maxsize=None)
def post_build(name):
    c = POST[name]
    g = _gen("ps" + name)
    B, zc, HW = c["B"], c["zc"], c["HW"]
    mom = torch.full((B * HW, c["ld"]), float("nan"))
    mom[:, :zc] = torch.randn(B * HW, zc, generator=g) * 3.0
    if not c["use_mean"]:
        lv = torch.rand(B * HW, zc, generator=g) * 70.0 - 40.0  # [-40, 30]: both clamps bind
        lv.view(-1)[:4] = torch.tensor([-40.0, 30.0, -30.0, 20.0])
        mom[:, zc:2 * zc] = lv
    noise = None if c["use_mean"] else torch.randn(B, zc, HW, generator=g)
    return dict(case=c, mom=mom.contiguous(), noise=noise)


def post_eval(o, dtype, mutant=None):
    """-> (z [B, zc, HW], |mean| + |sd noise|) in `dtype`, in the kernel's order of operations"""
    c = o["case"]
    B, zc, HW = c["B"], c["zc"], c["HW"]
    m = o["mom"].view(B, HW, c["ld"]).permute(0, 2, 1).to(dtype)  # [B, ld, HW]
    mean = m[:, :zc]
    s = torch.tensor(c["scale"], dtype=torch.float32).to(dtype)
    if c["use_mean"]:
        return s * mean, mean.abs()
    lv = m[:, zc:2 * zc]
    if mutant != "no_clamp":
        lv = lv.clamp(-30.0, 20.0)
    sd = torch.exp(lv) if mutant == "exp_lv" else torch.exp(0.5 * lv)
    t = sd * o["noise"].to(dtype)
    return s * (mean + t), mean.abs() + t.abs()


def post_verify(o, got):
    c = o["case"]
    n = c["B"] * c["zc"] * c["HW"]
    ref, mag = post_eval(o, torch.float64)
    tol = 8.0 * 2.0 ** -24 * abs(f32(c["scale"])) * mag
    return _result(_ratio(got[:n].view(ref.shape), ref, tol), (got[n:] != SENT32).sum().item())


# ================================================================================== k_vq_quantize
def _vq(name, n_embed, zc, B, HW, in_mul=1.0, ties=False):
    return dict(name=name, n_embed=n_embed, zc=zc, B=B, HW=HW, in_mul=in_mul, ties=ties, Cpad=32)


_IM = 1.0 / 0.18215
VQ_CASES = [
    _vq("e256_zc3", 256, 3, 2, 35), _vq("e256_zc3_in_mul", 256, 3, 2, 35, _IM),
    _vq("e8192_zc3_96KB", 8192, 3, 1, 4096),  # the VQ-f4 codebook: 96 KB of dynamic LDS
    _vq("e8192_zc3_96KB_in_mul", 8192, 3, 1, 4096, _IM),
    _vq("e37_zc1", 37, 1, 2, 35), _vq("e37_zc1_in_mul", 37, 1, 2, 35, _IM),
    _vq("e1000_zc8", 1000, 8, 1, 300), _vq("e1000_zc8_in_mul", 1000, 8, 1, 300, _IM),
    _vq("ties", 40, 3, 2, 35, ties=True),
    _vq("wrap_e64_zc3_hw66000", 64, 3, 2, 66000),  # 132 000 vectors > 512 x 256 threads
]
VQ = _names(VQ_CASES)
N_TIED = 6  # the first pixels of image 0 of the "ties" case are z = 0


def _vq_chunks(n, n_embed):
    step = max(1, (1 << 23) // n_embed)  # at most 8M float64 distances at a time
    return [(a, min(n, a + step)) for a in range(0, n, step)]


@functools.lru_cache(maxsize=4)
def vq_build(name):
    c = VQ[name]
    g = _gen("vq" + name)
    B, zc, HW, ne = c["B"], c["zc"], c["HW"], c["n_embed"]
    in_mul = torch.tensor(c["in_mul"], dtype=torch.float32)
    if c["ties"]:  # rows k, k + 10, k + 20, k + 30 = +e, -e, +e, -e: duplicates, and mirrored pairs that tie exactly at z = 0
        base = torch.randn(ne // 4, zc, generator=g)
        cb = torch.cat([base, -base, base, -base])
    else:
        cb = torch.randn(ne, zc, generator=g)
    z = torch.randn(B, zc, HW, generator=g) / in_mul
    if c["ties"]:
        z[0, :, :N_TIED] = 0.0
    zv = (z * in_mul).permute(0, 2, 1).reshape(B * HW, zc).contiguous()  # fp32(z in_mul): what the kernel quantises
    # identical rows count as one code, named by its lowest index
    uniq, inv = torch.unique(cb, dim=0, return_inverse=True)
    first = torch.full((uniq.shape[0],), ne, dtype=torch.long).scatter_reduce(0, inv, torch.arange(ne), "amin")
    n = B * HW
    idx = torch.empty(n, dtype=torch.long)
    d1, d2 = torch.empty(n, dtype=torch.float64), torch.empty(n, dtype=torch.float64)
    u64 = uniq.double()
    for a, b in _vq_chunks(n, uniq.shape[0]):
        d = ((zv[a:b].double()[:, None, :] - u64[None]) ** 2).sum(-1)
        if uniq.shape[0] > 1:
            two, where = torch.topk(d, 2, dim=1, largest=False)
            d1[a:b], d2[a:b], idx[a:b] = two[:, 0], two[:, 1], first[where[:, 0]]
        else:
            d1[a:b], d2[a:b], idx[a:b] = d[:, 0], float("inf"), first[0]
    emax = cb.double().norm(dim=1).max()
    bound = 2.0 * (2 * zc + 4) * 2.0 ** -24 * (zv.double().norm(dim=1) + emax) ** 2
    must = torch.zeros(n, dtype=torch.bool)
    if c["ties"]:  # z = 0: the smallest row of `base` and its mirror tie bit for bit; the first (+e, the lower index) wins
        must[:N_TIED] = True
        idx[:N_TIED] = base.double().norm(dim=1).argmin()
        assert (zv[:N_TIED] == 0).all()
    undecidable = ((d2 - d1) <= bound) & ~must
    return dict(case=c, z=z.contiguous(), cb=cb.contiguous(), zv=zv, idx=idx, bound=bound, undecidable=undecidable, must=must)


def vq_words(o, idx, fmt):
    """the kernel's output row for code idx: fp32 z + (e - z), rounded to 16 bits, zeros behind -> (words, the fp32 values)"""
    zv = o["zv"]
    v = zv + (o["cb"][idx] - zv)
    return to16(v, fmt), v


def vq_emulate(o, fmt, mutant=None):
    c = o["case"]
    zv, cb = o["zv"], o["cb"]
    n, ne = zv.shape[0], c["n_embed"]
    z2 = torch.zeros(n)
    e2 = torch.zeros(ne)
    for ch in range(c["zc"]):
        z2 = z2 + zv[:, ch] * zv[:, ch]
        e2 = e2 + cb[:, ch] * cb[:, ch]
    idx = torch.empty(n, dtype=torch.long)
    for a, b in _vq_chunks(n, 2 * ne):
        dot = torch.zeros(b - a, ne)
        for ch in range(c["zc"]):
            dot = dot + zv[a:b, ch, None] * cb[None, :, ch]
        d = (z2[a:b, None] + (0.0 if mutant == "no_e2" else e2[None, :])) - 2.0 * dot
        idx[a:b] = (ne - 1 - d.flip(1).argmin(1)) if mutant == "last_minimum" else d.argmin(1)
    out = torch.zeros(n, c["Cpad"], dtype=torch.int16)
    out[:, :c["zc"]] = vq_words(o, idx, fmt)[0]
    return torch.cat([out.reshape(-1), torch.full((GUARD,), SENT16, dtype=torch.int16)])


def _vq_row_ok(o, got_rows, idx, fmt):
    """[n] bool: the rows are what the kernel writes for codes idx"""
    c = o["case"]
    w, v = vq_words(o, idx, fmt)
    if c["in_mul"] == 1.0:
        return (got_rows == w).all(1)
    g = from16(got_rows.contiguous(), fmt)
    tol = step16(torch.maximum(g.double().abs(), v.double().abs()), fmt)
    return (((g.double() - v.double()).abs() <= tol) & torch.isfinite(g)).all(1)


def vq_verify(o, got, fmt):
    c = o["case"]
    n, zc = o["zv"].shape[0], c["zc"]
    rows = got[:n * c["Cpad"]].view(n, c["Cpad"])
    mism = (rows[:, zc:] != 0).sum().item() + (got[n * c["Cpad"]:] != SENT16).sum().item()
    ok = _vq_row_ok(o, rows[:, :zc], o["idx"], fmt)
    und = o["undecidable"]
    wrong = (~ok & ~und).sum().item()
    # undecidable vectors that did not take the float64 code: any code within the bound of the minimum will do
    cb64 = o["cb"].double()
    for v in torch.nonzero(~ok & und).reshape(-1).tolist():
        d = ((o["zv"][v].double()[None, :] - cb64) ** 2).sum(-1)
        cand = torch.nonzero(d <= d.min() + o["bound"][v]).reshape(-1)
        zrow = o["zv"][v][None, :].expand(cand.shape[0], zc)
        sub = dict(case=c, zv=zrow, cb=o["cb"])
        if not _vq_row_ok(sub, rows[v, :zc][None, :].expand(cand.shape[0], zc), cand, fmt).any():
            wrong += 1
    return _result(0.0, mism + wrong, wrong_codes=wrong, undecidable=und.float().mean().item())
