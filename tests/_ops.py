"""Thin helpers that call the single-kernel C-ABI entry points (cd_op_*) with torch tensors."""
import ctypes as C

import numpy as np
import torch

from cycle_diffusion_amd import _ffi
from cycle_diffusion_amd._ffi import check, ptr


def bf16_round(t):
    """Round an fp32 tensor to the engine's 16-bit storage format (fp16 by default, cd_act_format())."""
    dt = torch.float16 if _ffi.load_library().cd_act_format() == 1 else torch.bfloat16
    return t.to(dt).to(torch.float32)


def dev(t):
    return t.detach().to(torch.float32).contiguous().cuda()


def err_stats(got, ref):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    d = (got - ref).abs()
    scale = ref.abs().max().item() + 1e-12
    return dict(max_abs=d.max().item(), rel_to_max=d.max().item() / scale,
                mean_rel=d.mean().item() / (ref.abs().mean().item() + 1e-12),
                finite=bool(torch.isfinite(got).all().item()))


def pack_conv(eng, w, geglu=False):
    w = w.detach().float().cpu().contiguous()
    if w.dim() == 2:
        w = w[:, :, None, None].contiguous()
    N, Cin, KH, KW = w.shape
    out = C.c_void_p()
    npad, cpad = C.c_int(), C.c_int()
    check(eng.lib.cd_op_pack_conv_weight(eng.h, C.c_void_p(w.data_ptr()), N, Cin, KH, KW, int(geglu),
                                         C.byref(out), C.byref(npad), C.byref(cpad)))
    return out, (N, Cin, KH, KW)


def geglu_pack_vec(v):
    """bias in the packed row order used for GEGLU weights: blocks of 64 = [32 value | 32 gate]."""
    n = v.shape[0]
    half = n // 2
    out = torch.empty_like(v)
    for j in range(n):
        blk, within = divmod(j, 64)
        src = blk * 32 + within if within < 32 else half + blk * 32 + (within - 32)
        out[j] = v[src]
    return out


def conv2d(eng, x0, w, x1=None, stride=1, pad=1, asym=False, up=False, bias=None, rowvec=None, resid=None,
           act=0, tile=0, geglu=False):
    handle, (N, Cin, KH, KW) = pack_conv(eng, w, geglu)
    B, C0, H, W = x0.shape
    C1 = x1.shape[1] if x1 is not None else 0
    Hin, Win = (2 * H, 2 * W) if up else (H, W)
    if asym:
        Ho, Wo = (Hin + 1 - KH) // stride + 1, (Win + 1 - KW) // stride + 1
    else:
        Ho, Wo = (Hin + 2 * pad - KH) // stride + 1, (Win + 2 * pad - KW) // stride + 1
    Nout = N // 2 if geglu else N
    y = torch.empty((B, Nout, Ho, Wo), device="cuda", dtype=torch.float32)
    b = None
    if bias is not None:
        b = dev(geglu_pack_vec(bias) if geglu else bias)
    xs0, xs1 = dev(x0), dev(x1) if x1 is not None else None
    rv, rs = dev(rowvec) if rowvec is not None else None, dev(resid) if resid is not None else None
    check(eng.lib.cd_op_conv2d(eng.h, ptr(xs0), C0, ptr(xs1), C1, B, H, W, handle, N, KH, KW, stride, pad,
                               int(asym), int(up), ptr(b), ptr(rv), ptr(rs), act, tile, ptr(y)))
    torch.cuda.synchronize()
    return y.cpu()


def conv2d16(eng, x0, w, stride=1, pad=1, bias=None, resid=None, act=0, tile=0, geglu=False, want_stats=False, rowvec=None,
             x1=None, asym=False, up=False):
    """cd_op_conv2d_16: the convolution with the engine's 16-bit output (+ the fused GroupNorm statistics)"""
    handle, (N, Cin, KH, KW) = pack_conv(eng, w, geglu)
    B, C0, H, W = x0.shape
    C1 = x1.shape[1] if x1 is not None else 0
    Hin, Win = (2 * H, 2 * W) if up else (H, W)
    if asym:
        Ho, Wo = (Hin + 1 - KH) // stride + 1, (Win + 1 - KW) // stride + 1
    else:
        Ho, Wo = (Hin + 2 * pad - KH) // stride + 1, (Win + 2 * pad - KW) // stride + 1
    Nout = N // 2 if geglu else N
    y = torch.empty((B, Nout, Ho, Wo), device="cuda", dtype=torch.float32)
    st = torch.zeros((B * Ho * Wo // 32, 2, Nout), device="cuda", dtype=torch.float32) if want_stats else None
    b = None
    if bias is not None:
        b = dev(geglu_pack_vec(bias) if geglu else bias)
    xs0, xs1 = dev(x0), dev(x1) if x1 is not None else None
    rs = dev(resid) if resid is not None else None
    rv = dev(rowvec) if rowvec is not None else None
    check(eng.lib.cd_op_conv2d_16(eng.h, ptr(xs0), C0, ptr(xs1), C1, B, H, W, handle, N, KH, KW, stride, pad, int(asym),
                                  int(up), ptr(b), ptr(rv), ptr(rs), act, tile, ptr(y), ptr(st)))
    torch.cuda.synchronize()
    return (y.cpu(), st.cpu()) if want_stats else y.cpu()


def last_gemm_config(eng):
    """cd_op_last_gemm_config: what this thread's most recent implicit-GEMM launch ran, after the launcher's fallbacks"""
    v = [C.c_int() for _ in range(5)]
    check(eng.lib.cd_op_last_gemm_config(eng.h, *[C.byref(x) for x in v]))
    return dict(zip(("tile", "bk", "split", "chm", "tile_group"), (x.value for x in v)))


def run_conv_case(eng, c, o, tile):
    """One case of the configuration sweep (tests/_gemm_sweep.py: case dict `c`, operands `o`) on `tile` (id | split << 8 |
    bk32 << 16): (y, statistics or None, read-back of what ran)."""
    kw = dict(x1=o["x1"], stride=c["stride"], pad=c["pad"], asym=c["asym"], up=c["up"], bias=o["bias"], rowvec=o["rowvec"],
              resid=o["resid"], act=c["act"], tile=tile, geglu=c["geglu"])
    st = None
    if c["out16"]:
        y = conv2d16(eng, o["x0"], o["w"], want_stats=c["stats"], **kw)
        if c["stats"]:
            y, st = y
    else:
        y = conv2d(eng, o["x0"], o["w"], **kw)
    return y, st, last_gemm_config(eng)


def groupnorm(eng, x, gamma, beta, eps, silu=False, film=None):
    B, Cc, H, W = x.shape
    y = torch.empty_like(x, device="cuda")
    xs, g, b = dev(x), dev(gamma), dev(beta)
    f = dev(film) if film is not None else None
    check(eng.lib.cd_op_groupnorm(eng.h, ptr(xs), B, Cc, H, W, 32, C.c_float(eps), ptr(g), ptr(b), ptr(f),
                                  int(silu), ptr(y)))
    torch.cuda.synchronize()
    return y.cpu()


X3_ACT_SCALE = 16.0  # csrc/kernels.h kX3ActScale


def groupnorm_ex(eng, x0, gamma, beta, eps, x1=None, pad0=0, pad1=0, silu=False, film=None, film_shared=False,
                 film_ld=None, stats0=None, stats1=None, precision=0):
    """cd_op_groupnorm_ex: groupnorm_fwd as the networks call it. film [B, 2C] (or [2C] with film_shared: film_ld = 0);
    film_ld > 2C pads every FiLM row with NaN. precision 2 decodes the fp16 pairs of the split output."""
    B, C0, H, W = x0.shape
    C1 = x1.shape[1] if x1 is not None else 0
    Cc = C0 + C1
    f, ld = None, 0
    if film is not None:
        if film_shared:
            assert film.shape == (2 * Cc,)
            f = dev(film)
        else:
            ld = film_ld or 2 * Cc
            rows = torch.full((B, ld), float("nan"))
            rows[:, :2 * Cc] = film
            f = dev(rows)
    xs0, xs1 = dev(x0), dev(x1) if x1 is not None else None
    g, b = dev(gamma), dev(beta)

    def guarded(st):  # one more block of NaN behind the statistics: an index past the end stays in the tensor and shows
        if st is None:
            return None
        return dev(torch.cat([st.float(), torch.full((1,) + tuple(st.shape[1:]), float("nan"))], 0))

    s0, s1 = guarded(stats0), guarded(stats1)
    if precision == 2:
        y = torch.empty((B * H * W, 2 * Cc), device="cuda", dtype=torch.float16)
    else:
        y = torch.empty((B, Cc, H, W), device="cuda", dtype=torch.float32)
    check(eng.lib.cd_op_groupnorm_ex(eng.h, ptr(xs0), C0, pad0, ptr(xs1), C1, pad1, B, H, W, C.c_float(eps), ptr(g), ptr(b),
                                     ptr(f), ld, int(silu), ptr(s0), ptr(s1), precision, ptr(y)))
    torch.cuda.synchronize()
    if precision == 2:  # (hi + lo) / kX3ActScale: exact in float64
        y = y.cpu().double()
        y = (y[:, :Cc] + y[:, Cc:]) / X3_ACT_SCALE
        return y.reshape(B, H, W, Cc).permute(0, 3, 1, 2).contiguous()
    return y.cpu()


# ---------------------------------------------------------------------------------------------- fp32 path (precision 1 / 2)
def decode_pairs(y, Cc):
    """raw fp16 pairs [rows][hi(C) | lo(C)] -> float64 [rows][C] = (hi + lo) / kX3ActScale (exact)"""
    y = y.cpu().double()
    return (y[:, :Cc] + y[:, Cc:]) / X3_ACT_SCALE


def pack_conv_prec(eng, w, geglu=False):
    """cd_op_pack_conv_weight_prec: fp32 rows + their three-term fp16 split; raises the range error for |w| >= 255"""
    w = w.detach().float().cpu().contiguous()
    if w.dim() == 2:
        w = w[:, :, None, None].contiguous()
    N, Cin, KH, KW = w.shape
    out = C.c_void_p()
    check(eng.lib.cd_op_pack_conv_weight_prec(eng.h, C.c_void_p(w.data_ptr()), N, Cin, KH, KW, int(geglu), C.byref(out)))
    return out, (N, Cin, KH, KW)


def conv_out_hw(H, W, k, stride, pad, asym, up):
    Hin, Win = (2 * H, 2 * W) if up else (H, W)
    if asym:
        return (Hin + 1 - k) // stride + 1, (Win + 1 - k) // stride + 1
    return (Hin + 2 * pad - k) // stride + 1, (Win + 2 * pad - k) // stride + 1


def conv2d_prec(eng, x0, w, precision, x1=None, pad0=0, pad1=0, stride=1, pad=1, asym=False, up=False, bias=None, rowvec=None,
                resid=None, resid_pad=0, act=0, alpha=1.0, tile=0, geglu=False, via_split_rows=False, want_stats=False):
    """cd_op_conv2d_prec: conv_fwd on the fp32 path (precision 1: k_conv_f32; 2: the three-term split GEMM). rowvec [B, N] or
    a shared [N] row; geglu: weights packed with geglu = 1, columns returned raw in the packed order. -> y or (y, stats)"""
    handle, (N, Cin, KH, KW) = pack_conv_prec(eng, w, geglu)
    B, C0, H, W = x0.shape
    C1 = x1.shape[1] if x1 is not None else 0
    Ho, Wo = conv_out_hw(H, W, KH, stride, pad, asym, up)
    y = torch.empty((B, N, Ho, Wo), device="cuda", dtype=torch.float32)
    st = torch.zeros((B * Ho * Wo // 32, 2, N), device="cuda", dtype=torch.float32) if want_stats else None
    b = None
    if bias is not None:
        b = dev(geglu_pack_vec(bias) if geglu else bias)
    xs0, xs1 = dev(x0), dev(x1) if x1 is not None else None
    rv, rs = dev(rowvec) if rowvec is not None else None, dev(resid) if resid is not None else None
    shared = rowvec is not None and rowvec.dim() == 1
    check(eng.lib.cd_op_conv2d_prec(eng.h, ptr(xs0), C0, pad0, ptr(xs1), C1, pad1, B, H, W, handle, N, KH, KW, stride, pad,
                                    int(asym), int(up), ptr(b), ptr(rv), int(shared), ptr(rs), resid_pad, act, int(geglu), tile,
                                    precision, int(via_split_rows), C.c_float(alpha), ptr(y), ptr(st)))
    torch.cuda.synchronize()
    return (y.cpu(), st.cpu()) if want_stats else y.cpu()


def attention_prec(eng, q, k, v, heads, scale, mode, precision=1, padq=0, padk=0, padv=0, q_log2=False, obias=None):
    """cd_op_attention_prec: q [B, Tq, H D], k / v [B, Tk, H D] -> [B, Tq, H D] (float64 of the decoded pairs at precision 2)"""
    B, Tq, Cc = q.shape
    Tk = k.shape[1]
    o = torch.empty((B * Tq, 2 * Cc), device="cuda", dtype=torch.float16) if precision == 2 else \
        torch.empty((B * Tq, Cc), device="cuda", dtype=torch.float32)
    qs, ks, vs = dev(q), dev(k), dev(v)
    ob = dev(obias) if obias is not None else None
    check(eng.lib.cd_op_attention_prec(eng.h, ptr(qs), ptr(ks), ptr(vs), B, heads, Tq, Tk, Cc // heads, padq, padk, padv,
                                       C.c_float(scale), int(q_log2), ptr(ob), mode, precision, ptr(o)))
    torch.cuda.synchronize()
    o = decode_pairs(o, Cc) if precision == 2 else o.cpu()
    return o.reshape(B, Tq, Cc)


def rows_prec(eng, op, x0, precision, x1=None, pad0=0, pad1=0, gamma=None, beta=None):
    """cd_op_rows_prec: op "layernorm" | "geglu" | "split_rows" on fp32 rows [rows, C]"""
    code = {"layernorm": 0, "geglu": 1, "split_rows": 2}[op]
    rows, C0 = x0.shape
    C1 = x1.shape[1] if x1 is not None else 0
    Cout = C0 // 2 if code == 1 else C0 + C1
    y = torch.empty((rows, 2 * Cout), device="cuda", dtype=torch.float16) if precision == 2 else \
        torch.empty((rows, Cout), device="cuda", dtype=torch.float32)
    xs0, xs1 = dev(x0), dev(x1) if x1 is not None else None
    g, b = dev(gamma) if gamma is not None else None, dev(beta) if beta is not None else None
    check(eng.lib.cd_op_rows_prec(eng.h, code, ptr(xs0), rows, C0, pad0, ptr(xs1), C1, pad1, ptr(g), ptr(b), precision, ptr(y)))
    torch.cuda.synchronize()
    return decode_pairs(y, Cout) if precision == 2 else y.cpu()


def resample_prec(eng, op, x, precision):
    """cd_op_resample_prec: op "avgpool" (precision 1, or 2 = split in and out, decoded) | "upsample" (precision 1); NCHW"""
    B, Cc, H, W = x.shape
    Ho, Wo = (H // 2, W // 2) if op == "avgpool" else (2 * H, 2 * W)
    y = torch.empty((B * Ho * Wo, 2 * Cc), device="cuda", dtype=torch.float16) if precision == 2 else \
        torch.empty((B, Cc, Ho, Wo), device="cuda", dtype=torch.float32)
    xs = dev(x)
    check(eng.lib.cd_op_resample_prec(eng.h, 0 if op == "avgpool" else 1, ptr(xs), B, Cc, H, W, precision, ptr(y)))
    torch.cuda.synchronize()
    if precision == 2:
        return decode_pairs(y, Cc).reshape(B, Ho, Wo, Cc).permute(0, 3, 1, 2).contiguous()
    return y.cpu()


def layernorm(eng, x, gamma, beta, eps=1e-5):
    rows, Cc = x.shape
    y = torch.empty_like(x, device="cuda")
    xs, g, b = dev(x), dev(gamma), dev(beta)
    check(eng.lib.cd_op_layernorm(eng.h, ptr(xs), rows, Cc, ptr(g), ptr(b), C.c_float(eps), ptr(y)))
    torch.cuda.synchronize()
    return y.cpu()


def attention(eng, q, k, v, heads, scale, v_transposed=False):
    B, Tq, Cc = q.shape
    Tk = k.shape[1]
    o = torch.empty_like(q, device="cuda")
    qs, ks, vs = dev(q), dev(k), dev(v)
    check(eng.lib.cd_op_attention(eng.h, ptr(qs), ptr(ks), ptr(vs), B, heads, Tq, Tk, Cc // heads,
                                  C.c_float(scale), 1 if v_transposed else 0, ptr(o)))
    torch.cuda.synchronize()
    return o.cpu()


def attention_ex(eng, q, k, v, heads, scale, layout=0, pad=0, v_transposed=False, d_extra=0, t_extra=0, q_log2=False,
                 obias=None, causal=False, opad=0):
    """cd_op_attention_ex: launch_attention on strided / fused operands. -> [B, Tq, H D + opad], pad columns included"""
    B, Tq, Cc = q.shape
    Tk = k.shape[1]
    o = torch.zeros((B, Tq, Cc + opad), device="cuda", dtype=torch.float32)
    qs, ks, vs = dev(q), dev(k), dev(v)
    ob = dev(obias) if obias is not None else None
    check(eng.lib.cd_op_attention_ex(eng.h, ptr(qs), ptr(ks), ptr(vs), B, heads, Tq, Tk, Cc // heads, layout, pad,
                                     int(v_transposed), d_extra, t_extra, C.c_float(scale), int(q_log2), ptr(ob), int(causal),
                                     opad, ptr(o)))
    torch.cuda.synchronize()
    return o.cpu()


def cross_attention_ctrl_ex(eng, q_own, q_src, k_own, k_src, v_own, M, alpha, w, heads, scale, q_log2=False, opad=0):
    """cd_op_cross_attention_ctrl_ex -> [B, Tq, H D + opad], pad columns included"""
    B, Tq, Cc = q_own.shape
    L = k_own.shape[1]
    t = [dev(x) for x in (q_own, q_src, k_own, k_src, v_own, M, alpha, w)]
    o = torch.zeros((B, Tq, Cc + opad), device="cuda", dtype=torch.float32)
    check(eng.lib.cd_op_cross_attention_ctrl_ex(eng.h, *[ptr(x) for x in t], B, q_src.shape[0], M.shape[0], heads, Tq, L, L,
                                                Cc // heads, C.c_float(scale), int(q_log2), opad, ptr(o)))
    torch.cuda.synchronize()
    return o.cpu()


def softmax_rows(eng, s):
    rows, cols = s.shape
    p = torch.empty_like(s, device="cuda")
    ss = dev(s)
    check(eng.lib.cd_op_softmax_rows(eng.h, ptr(ss), rows, cols, ptr(p)))
    torch.cuda.synchronize()
    return p.cpu()


def timestep_embedding(eng, t, dim, mode):
    B = t.shape[0]
    out = torch.empty((B, dim), device="cuda", dtype=torch.float32)
    ts = dev(t)
    check(eng.lib.cd_op_timestep_embedding(eng.h, ptr(ts), B, dim, mode, ptr(out)))
    torch.cuda.synchronize()
    return out.cpu()


def sched_step(eng, mode, kind, coef_row, x0=None, xt=None, eps_hat=None, cfg=False, g=1.0, noise=None,
               eps_in=None, is_last=False):
    coef = _ffi.coef_array([coef_row])
    ref = xt if xt is not None else x0
    B, Cc, H, W = ref.shape
    xt_d = dev(xt) if xt is not None else torch.empty((B, Cc, H, W), device="cuda")
    z = torch.zeros((B, Cc, H, W), device="cuda")
    x0_d = dev(x0) if x0 is not None else None
    eh = dev(eps_hat) if eps_hat is not None else None
    nz = dev(noise) if noise is not None else None
    ei = dev(eps_in) if eps_in is not None else None
    check(eng.lib.cd_op_sched_step(eng.h, mode, kind, C.c_void_p(coef.ctypes.data), ptr(x0_d), ptr(xt_d), ptr(eh),
                                   int(cfg), C.c_float(g), ptr(nz), ptr(ei), int(is_last), B, Cc, H * W, ptr(z)))
    torch.cuda.synchronize()
    return xt_d.cpu(), z.cpu()


def probe(eng, which, nfloats):
    out = torch.zeros(nfloats, device="cuda", dtype=torch.float32)
    check(eng.lib.cd_op_probe(eng.h, which, None, ptr(out), nfloats * 4))
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ------------------------------------------------------------------------------ bare entry points of csrc/elementwise.hip
# The caller's bytes in, one launch, the kernel's bytes out (tests/_glue_ref.py: operands, sentinels, guards). 16-bit tensors
# are torch.int16 storage words; nothing here converts, pads or transposes on the device.
def _up(t):
    return None if t is None else t.contiguous().cuda()


def _out16(words, guard, sent):
    return torch.full((words + guard,), sent, dtype=torch.int16, device="cuda")


def _out32(n, guard, sent):
    return torch.full((n + guard,), sent, dtype=torch.float32, device="cuda")


def _finish(eng, rc, y, refusal):
    """the output buffer; with refusal = True the call must have been refused: (its error text, the buffer as it left it)"""
    if not refusal:
        check(rc)
        return y.cpu()
    assert rc != 0, "the call was not refused"
    msg = eng.lib.cd_last_error().decode("utf-8", "replace")
    torch.cuda.synchronize()
    return msg, y.cpu()


def glue_nchw_to_nhwc(eng, x, Cpad, scale, shift, dup, guard, sent):
    """k_nchw_to_nhwc: x fp32 [B, C, HW] -> int16 [(1 + dup) B HW Cpad + guard]"""
    B, Cc, HW = x.shape
    xs, y = _up(x), _out16((1 + dup) * B * HW * Cpad, guard, sent)
    check(eng.lib.cd_op_layout(eng.h, 0, ptr(xs), ptr(y), B, Cc, HW, Cpad, 1, C.c_float(scale), C.c_float(shift), dup))
    return y.cpu()


def glue_nhwc_to_nchw(eng, x, B, Cc, HW, scale, shift, guard, sent):
    """k_nhwc_to_nchw: x [B HW][ld] int16 words or fp32 -> fp32 [B C HW + guard]"""
    xs, y = _up(x), _out32(B * Cc * HW, guard, sent)
    check(eng.lib.cd_op_layout(eng.h, 1, ptr(xs), ptr(y), B, Cc, HW, x.shape[1], int(x.dtype == torch.float32),
                               C.c_float(scale), C.c_float(shift), 0))
    return y.cpu()


def glue_resample16(eng, op, x, guard, sent, refusal=False):
    """k_avgpool2 / k_upsample2: x int16 [B, H, W, C] -> int16 [B Ho Wo C + guard]"""
    B, H, W, Cc = x.shape
    Ho, Wo = (H // 2, W // 2) if op == "avgpool" else (2 * H, 2 * W)
    xs, y = _up(x), _out16(B * Ho * Wo * Cc, guard, sent)
    rc = eng.lib.cd_op_resample16(eng.h, 0 if op == "avgpool" else 1, ptr(xs), ptr(y), B, H, W, Cc)
    return _finish(eng, rc, y, refusal)


def glue_copy_rows16(eng, src, ldd, cols, launches, total_rows, guard, sent, refusal=False):
    """k_copy_strided_bf16: src int16 [rows][lds]; launches = (first source row, first destination row, rows) each"""
    lds = src.shape[1]
    xs, y = _up(src), _out16(total_rows * ldd, guard, sent)
    rc = 0
    for r0, d0, rows in launches:
        rc = rc or eng.lib.cd_op_copy_rows16(eng.h, ptr(xs[r0:]), lds, ptr(y[d0 * ldd:]), ldd, rows, cols)
    return _finish(eng, rc, y, refusal)


def glue_vec_linear(eng, x, W, bias, K, ldy, silu_in, silu_out, sent):
    """k_vec_linear: x fp32 [B][ldx], W [N][K] -> fp32 [B][ldy], the columns >= N as they were"""
    B, N = x.shape[0], W.shape[0]
    xs, ws, bs = _up(x), _up(W), _up(bias)
    y = torch.full((B, ldy), sent, dtype=torch.float32, device="cuda")
    check(eng.lib.cd_op_vec_linear(eng.h, ptr(xs), x.shape[1], ptr(ws), ptr(bs), ptr(y), ldy, B, K, N, int(silu_in),
                                   int(silu_out)))
    return y.cpu()


def glue_tokens(eng, op, B, L, D, vocab, out_words, guard, sent, ids=None, x16=None, tok=None, pos=None):
    """k_embed_tokens / k_vit_tokens / k_gather_eot -> int16 [out_words + guard]"""
    t = [_up(v) for v in (ids, x16, tok, pos)]
    y = _out16(out_words, guard, sent)
    check(eng.lib.cd_op_tokens(eng.h, {"embed": 0, "vit": 1, "eot": 2}[op], ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), ptr(y),
                               B, L, D, vocab))
    return y.cpu()


def glue_posterior_sample(eng, mom, noise, B, zc, HW, scale, use_mean, guard, sent, seed=0):
    """k_posterior_sample: mom fp32 [B HW][ld] -> fp32 [B zc HW + guard]"""
    ms, ns, z = _up(mom), _up(noise), _out32(B * zc * HW, guard, sent)
    check(eng.lib.cd_op_posterior_sample(eng.h, ptr(ms), mom.shape[1], ptr(ns), seed, ptr(z), B, zc, HW, C.c_float(scale),
                                         int(use_mean)))
    return z.cpu()


def glue_vq_quantize(eng, z, in_mul, codebook, B, HW, Cpad, guard, sent, refusal=False):
    """k_vq_quantize: z fp32 [B, zc, HW], codebook [n_embed][zc] -> int16 [B HW Cpad + guard]"""
    zs, cs, y = _up(z), _up(codebook), _out16(B * HW * Cpad, guard, sent)
    rc = eng.lib.cd_op_vq_quantize(eng.h, ptr(zs), C.c_float(in_mul), ptr(cs), codebook.shape[0], codebook.shape[1], B, HW, ptr(y),
                                   Cpad)
    return _finish(eng, rc, y, refusal)


# ------------------------------------------------------------------------------ the batched GEMM forms and the AttnBlock core
# tests/_gemm_batched_ref.py: operands as int16 storage words, sentinels and guards; nothing is staged on the device.
def _at(t, elems):
    """device pointer `elems` elements into tensor t"""
    return None if t is None else C.c_void_p(t.data_ptr() + elems * t.element_size())


def gemm_batched(eng, o, tile, singles=False, guard=0, sent16=0, sent32=0.0):
    """cd_op_gemm_batched on the operands of _gemm_batched_ref.gemm_build: one launch with nbatch = nb, or (singles) nb launches
    with nbatch = 1 and every pointer advanced by its batch stride, into the same buffers. -> (out, statistics or None, the
    read-back of every launch), the buffers with their guards"""
    c = o["case"]
    M, N, K, nb, out_ld = c["M"], c["N"], c["K"], c["nb"], c["out_ld"]
    o_bs, nblk = M * out_ld, M // 32
    A = _up(o["A"])
    W = A if o["W"] is None else _up(o["W"])
    bias, resid = _up(o["bias"]), _up(o["resid"])
    out = _out32(nb * o_bs, guard, sent32) if c["out_f32"] else _out16(nb * o_bs, guard, sent16)
    st = _out32(nb * nblk * 2 * N, guard, sent32) if c["stats"] else None
    rbs = []
    for z, n in ([(z, 1) for z in range(nb)] if singles else [(0, nb)]):
        check(eng.lib.cd_op_gemm_batched(
            eng.h, _at(A, o["a_off"] + z * c["a_bs"]), c["lda"], c["a_bs"], _at(W, o["w_off"] + z * c["w_bs"]), c["ldw"], c["w_bs"],
            M, N, K, n, C.c_float(c["alpha"]), ptr(bias), _at(resid, z * o_bs), N if resid is not None else 0,
            _at(st, z * nblk * 2 * N), 0, tile, _at(out, z * o_bs), out_ld, o_bs, c["out_f32"]))
        rbs.append(last_gemm_config(eng))
    return out.cpu(), (st.cpu() if st is not None else None), rbs


def gemm_raw(eng, a, lda, a_bs, w, ldw, w_bs, M, N, K, nb, alpha, bias, out, out_ld, out_f32, tile=0):
    """cd_op_gemm_batched on device pointers (ctypes) / tensors the caller laid out; out [nb][M][out_ld] on the device"""
    as_ptr = lambda t: t if isinstance(t, C.c_void_p) else ptr(t)
    check(eng.lib.cd_op_gemm_batched(eng.h, as_ptr(a), lda, a_bs, as_ptr(w), ldw, w_bs, M, N, K, nb, C.c_float(alpha), ptr(bias),
                                     None, 0, None, 0, tile, ptr(out), out_ld, M * out_ld, out_f32))


def attn_block_core(eng, o, guard, sent16, want_vt=True, refusal=False):
    """cd_op_attn_block_core on the operands of _gemm_batched_ref.core_build -> (o words, V^T words or None, branch); with
    refusal = True: (the error text, o words)"""
    c = o["case"]
    B, T, Cc = c["B"], c["T"], c["C"]
    handle, _ = pack_conv(eng, o["wv"])
    qk, n, vb = _up(o["qk"]), _up(o["n"]), _up(o["vbias"])
    out = _out16(B * T * c["ldo"], guard, sent16)
    vt = _out16(B * Cc * c["Tpad"], guard, sent16) if want_vt else None
    branch = C.c_int(-1)
    rc = eng.lib.cd_op_attn_block_core(eng.h, ptr(qk), c["ldqk"], ptr(n), c["ldn"], handle, ptr(vb), B, T, Cc, ptr(out), c["ldo"],
                                       ptr(vt), C.byref(branch))
    if refusal:
        return _finish(eng, rc, out, True)
    check(rc)
    return out.cpu(), (vt.cpu() if vt is not None else None), branch.value


def softmax_rows_dev(eng, s_dev):
    """cd_op_softmax_rows on a device tensor fp32 [rows, cols] -> fp32 on the device (16-bit values, widened)"""
    rows, cols = s_dev.shape
    p = torch.empty_like(s_dev)
    check(eng.lib.cd_op_softmax_rows(eng.h, ptr(s_dev), rows, cols, ptr(p)))
    return p


# ------------------------------------------------------------------------------ the FID Inception-v3's kernels and launch forms
# tests/_inception_ops_ref.py. Every output comes back whole: [rows + GUARD_ROWS, out_ld] with NaN wherever nothing was written.
GUARD_ROWS = 64


def pool3x3(eng, x, max_pool, stride, pad, in_pad=0, out_off=0, out_ld=None):
    """cd_op_pool3x3: x [B, C, H, W] -> the whole output buffer [B Ho Wo + 64, out_ld] (NaN outside the slice)"""
    B, Cc, H, W = x.shape
    out_ld = Cc if out_ld is None else out_ld
    Ho, Wo = (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1
    y = torch.zeros((B * Ho * Wo + GUARD_ROWS, out_ld), device="cuda", dtype=torch.float32)
    xs = dev(x)
    check(eng.lib.cd_op_pool3x3(eng.h, ptr(xs), B, Cc, H, W, in_pad, int(max_pool), stride, pad, out_off, out_ld, ptr(y)))
    torch.cuda.synchronize()
    return y.cpu()


def global_avg(eng, x, in_pad=0):
    """cd_op_global_avg: x [B, C, HW] -> fp32 [B, C]"""
    B, Cc, HW = x.shape
    y = torch.full((B, Cc), float("nan"), device="cuda", dtype=torch.float32)
    xs = dev(x)
    check(eng.lib.cd_op_global_avg(eng.h, ptr(xs), B, HW, Cc, in_pad, ptr(y)))
    torch.cuda.synchronize()
    return y.cpu()


def basic_conv(eng, x, w, gamma, beta, mean, var, stride=1, pad=(0, 0), in_ld=None, out_off=0, out_ld=None, tile=0):
    """cd_op_basic_conv: x [B, Cin, H, W], raw weight w [N, Cin, KH, KW] and the BatchNorm vectors [N] -> (the whole output buffer
    [B Ho Wo + 64, out_ld], the packed weights [Npad, KH, KW, Cpad], the bias [Npad], the read-back of what ran)"""
    B, Cin, H, W = x.shape
    N, _, KH, KW = w.shape
    Cpad, Npad, Nrun = -(-Cin // 32) * 32, -(-N // 128) * 128, -(-N // 32) * 32
    in_ld = Cpad if in_ld is None else in_ld
    out_ld = Nrun if out_ld is None else out_ld
    Ho, Wo = (H + 2 * pad[0] - KH) // stride + 1, (W + 2 * pad[1] - KW) // stride + 1
    y = torch.zeros((B * Ho * Wo + GUARD_ROWS, out_ld), device="cuda", dtype=torch.float32)
    wp = torch.full((Npad, KH, KW, Cpad), float("nan"), device="cuda", dtype=torch.float32)
    bo = torch.full((Npad,), float("nan"), device="cuda", dtype=torch.float32)
    t = [dev(v) for v in (x, w, gamma, beta, mean, var)]
    check(eng.lib.cd_op_basic_conv(eng.h, ptr(t[0]), B, Cin, H, W, in_ld, ptr(t[1]), ptr(t[2]), ptr(t[3]), ptr(t[4]), ptr(t[5]),
                                   N, KH, KW, stride, pad[0], pad[1], out_off, out_ld, tile, ptr(y), ptr(wp), ptr(bo)))
    torch.cuda.synchronize()
    return y.cpu(), wp.cpu(), bo.cpu(), last_gemm_config(eng)
