"""The implicit-GEMM kernel (csrc/conv_gemm.hip k_conv_gemm) as the batched plain GEMM the attention call sites launch, the
AttnBlock core (csrc/engine.hip at_core, one head) and k_softmax_rows: case tables, seeded operands, float64 references, fp32
emulations and their mutants for tests/test_gemm_batched_host.py (CPU) and tests/test_gpu_gemm_batched.py (GPU, through
cd_op_gemm_batched / cd_op_attn_block_core: the caller's device bytes in, the kernel's bytes out).

kernel form (call sites)                                   cases
V^T[z] = Wv X[z]^T   vt_gemm_fwd (engine.hip; at_core,     vt/c320_t77 (generic 16-bit epilogue, N & 7 != 0, clamped B rows),
                     clip_text.hip, st_entry_qkv):         vt/c192_t96_ld200 (fast epilogue, ldw != K, NaN padding),
                     a_bs = 0, wgt = tokens, out_ld > N    vt/c512_t256 (BM = 256 tiles)
S[z] = alpha Q K^T   at_core, C > 160: both operands in    s/c192_t96 (ragged M and N, ld = 2C + 8), s/c224_t64 (K % 64 = 32),
                     one [B T][ld] tensor, fp32 output     s/c512_t256; x/split2 (16-bit output, zb-indexed split-K workspace)
O[z] = P V + vbias   at_core, C > 160: K = T, ldw = Tpad   o/t96_c192 (ldw != Ktot, NaN in the V^T padding, ldo = C + 8),
                                                           o/t256_c512; x/resid_stats (residual and statistics per batch)
at_core              engine.hip (attn_block_fwd)           core/flash_c128_t100, core/wide_c192_t96, core/wide_c192_t64,
                                                           core/wide_c320_t160, core/wide_c512_t256; refusal T = 100, C = 192
k_softmax_rows       norm.hip                              sm/r5_c96, sm/r3_c64, sm/r2_c4096, sm/spike_r4_c300, sm/const_r2_c96

Every batch element has operands of its own (a batch stride taken from the wrong operand is an error of full size), every
padding column of a strided 16-bit input holds NaN, the shared V weight has nbatch - 1 blocks of NaN behind it (a_bs != 0
reads them), every output buffer starts as R.SENT16 / R.SENT32 and carries R.GUARD sentinel words behind its end.

  gemm_build / core_build / sm_build   operands as the device sees them (int16 storage words) and their fp32 values
  gemm_ref64 / core_ref64 / sm_ref64   float64 on the rounded operands, the epilogue applied in float64
  gemm_emulate / core_emulate / sm_emulate
                                       the kernels' roundings on the host: fp32 accumulation of the 16-bit operands, alpha in
                                       fp32, P rounded to 16 bits, one output rounding - and, with mutant = ..., a subtly wrong
                                       kernel through the same flat-index arithmetic
  gemm_verify / core_verify / sm_verify
                                       dict(rel_to_max, mean_rel, err_over_tol, mismatch, ...): err_over_tol = the worst of
                                       rel_to_max and mean_rel (and the statistics' error) over its bound, infinite for a
                                       non-finite word; mismatch = sentinel, guard and must-be-zero words that are not intact

Bounds. GEMM forms: _gemm_sweep.REL_TOL / MEAN_TOL / STATS_TOL (5e-3, 2e-3, 2e-3). AttnBlock core: _attn_forms_ref.REL / MEAN
x f, f = 1 for fp16 storage and 8 for bf16, on o - vbias; its V^T: the GEMM bounds. Softmax rows: 1e-2 / 5e-3
(test_gpu_ops.py::test_softmax_rows).
"""
import functools
import math

import torch

import _attn_forms_ref as AF
import _gemm_sweep as gs
import _glue_ref as R

FMTS = R.FMTS
SM_REL, SM_MEAN = 1e-2, 5e-3
BRANCH_FLASH, BRANCH_WIDE = 0, 1


def fmt_factor(fmt):
    return 1.0 if fmt == "fp16" else 8.0


def _names(cases):
    d = {c["name"]: c for c in cases}
    assert len(d) == len(cases)
    return d


def _nan_rows(vals, ld, fmt):
    """[rows, C] fp32 -> int16 [rows, ld], NaN words in the columns >= C"""
    rows, C = vals.shape
    x = torch.full((rows, ld), R.NAN16, dtype=torch.int16)
    x[:, :C] = R.to16(vals, fmt)
    return x


# ================================================================================================== GEMM forms
def _vt(name, C, K, T, Tpad, nb, ldx=None):
    return dict(name=name, form="vt", M=C, N=T, K=K, nb=nb, lda=K, a_bs=0, ldw=ldx or K, w_bs=T * (ldx or K), out_ld=Tpad,
                out_f32=0, alpha=1.0, bias=False, resid=False, stats=False, tiles=None)


def _s(name, K, T, nb, ld=None, out_f32=1, tiles=None):
    ld = ld or 2 * K
    return dict(name=name, form="s", M=T, N=T, K=K, nb=nb, lda=ld, a_bs=T * ld, ldw=ld, w_bs=T * ld, out_ld=T, out_f32=out_f32,
                alpha=K ** -0.5, bias=False, resid=False, stats=False, tiles=tiles)


def _o(name, T, C, nb, Tpad=None, ldo=None, resid=False, stats=False):
    Tpad = Tpad or T
    return dict(name=name, form="o", M=T, N=C, K=T, nb=nb, lda=T, a_bs=T * T, ldw=Tpad, w_bs=C * Tpad, out_ld=ldo or C,
                out_f32=0, alpha=1.0, bias=True, resid=resid, stats=stats, tiles=None)


GEMM_CASES = [
    _vt("vt/c320_t77", 320, 320, 77, 128, 3),
    _vt("vt/c192_t96_ld200", 192, 192, 96, 128, 2, ldx=200),
    _vt("vt/c512_t256", 512, 512, 256, 256, 2),
    _s("s/c192_t96", 192, 96, 3, ld=2 * 192 + 8),
    _s("s/c224_t64", 224, 64, 2),
    _s("s/c512_t256", 512, 256, 2),
    _o("o/t96_c192", 96, 192, 3, Tpad=128, ldo=192 + 8),
    _o("o/t256_c512", 256, 512, 2),
    _s("x/split2", 512, 64, 3, out_f32=0, tiles=[3 | (2 << 8)]),
    _o("x/resid_stats", 64, 128, 2, resid=True, stats=True),
]
GEMM = _names(GEMM_CASES)


def gemm_tiles(c):
    """the `tile` arguments a case is launched with: 0 = the launcher's choice, then explicit ids"""
    if c["tiles"]:
        return list(c["tiles"])
    return [0, 3, 2, 1, 24] + ([5, 22] if c["M"] >= 256 else [])


def expected_launch(c, tile):
    """read-back (tile id, bk, split) an explicit `tile` argument must give (none of the ids used here has a BK = 32 alias)"""
    tid, split, bk32 = tile & 0xff, (tile >> 8) & 0xff, (tile >> 16) & 1
    assert tid and tid not in gs.bk32_alias()
    bk = 32 if (c["K"] % 64 or bk32 or tid in gs.always_bk32()) else 64
    return tid, bk, max(split, 1)


def anchor_tile(c, bk, split):
    """tile 3 at depth bk and the same split: the family's bit-identity anchor"""
    return gs.ANCHOR_TILE | ((split if split > 1 else 0) << 8) | ((1 << 16) if (bk == 32 and c["K"] % 64 == 0) else 0)


@functools.lru_cache(maxsize=None)
def gemm_build(name, fmt):
    """A / W: the int16 buffers the launch reads (the S form has one, W = A + K words); a_off / w_off: element offsets of the
    operands in them; Af [nb or 1, M, K], Wf [nb, N, K]: the fp32 values of the rounded operands; bias fp32 [N]; resid int16
    [nb, M, out_ld] (its batch stride is the output's)"""
    c = GEMM[name]
    g = R._gen("gb" + name)
    M, N, K, nb = c["M"], c["N"], c["K"], c["nb"]
    o = dict(case=c, a_off=0, w_off=0, bias=None, resid=None)
    if c["form"] == "vt":
        wv = torch.randn(M, K, generator=g) / math.sqrt(K)
        x = torch.randn(nb * N, K, generator=g) * (1.0 + 0.25 * torch.arange(nb).repeat_interleave(N).float())[:, None]
        A = torch.full((nb, M, K), R.NAN16, dtype=torch.int16)  # blocks 1 .. nb - 1: what a_bs != 0 would read
        A[0] = R.to16(wv, fmt)
        W = _nan_rows(x, c["ldw"], fmt)
        o.update(A=A.reshape(-1), W=W.reshape(-1), Af=R.from16(A[:1], fmt),
                 Wf=R.from16(W[:, :K].contiguous(), fmt).view(nb, N, K))
    elif c["form"] == "s":
        qk = torch.randn(nb * M, 2 * K, generator=g)
        qk = qk * (1.0 + 0.25 * torch.arange(nb).repeat_interleave(M).float())[:, None]
        buf = _nan_rows(qk, c["lda"], fmt)
        v = R.from16(buf[:, :2 * K].contiguous(), fmt).view(nb, M, 2 * K)
        o.update(A=buf.reshape(-1), W=None, w_off=K, Af=v[..., :K].contiguous(), Wf=v[..., K:].contiguous())
    else:
        p = torch.softmax(2.0 * torch.randn(nb, M, K, generator=g), -1)
        vt = torch.randn(nb * N, K, generator=g) * (1.0 + 0.25 * torch.arange(nb).repeat_interleave(N).float())[:, None]
        A = R.to16(p, fmt)
        W = _nan_rows(vt, c["ldw"], fmt)
        o.update(A=A.reshape(-1), W=W.reshape(-1), Af=R.from16(A, fmt), Wf=R.from16(W[:, :K].contiguous(), fmt).view(nb, N, K))
    if c["bias"]:
        o["bias"] = torch.randn(N, generator=g) * 0.5
    if c["resid"]:
        assert c["out_ld"] == N
        o["resid"] = R.to16(torch.randn(nb, M, N, generator=g), fmt)
    return o


def _stats64(y):
    """[nb, M, N] float64 -> [nb, M / 32, 2, N]: sums and sums of squares over 32-row blocks"""
    nb, M, N = y.shape
    blk = y.reshape(nb, M // 32, 32, N)
    return torch.stack([blk.sum(2), (blk * blk).sum(2)], 2)


def gemm_ref64(o, fmt):
    """-> (y [nb, M, N], statistics or None) in float64"""
    c = o["case"]
    y = torch.tensor(c["alpha"], dtype=torch.float32).double() * (o["Af"].double() @ o["Wf"].double().transpose(1, 2))
    if o["bias"] is not None:
        y = y + o["bias"].double()[None, None, :]
    if o["resid"] is not None:
        y = y + R.from16(o["resid"], fmt).double()
    return y, (_stats64(y) if c["stats"] else None)


def out_words(c):
    return c["nb"] * c["M"] * c["out_ld"]


def stats_words(c):
    return c["nb"] * (c["M"] // 32) * 2 * c["N"]


def gemm_emulate(o, fmt, mutant=None):
    """The launch on the host, through the kernel's address arithmetic on the flat buffers (reads past a buffer are folded back
    into it). -> (out [out_words + GUARD] int16 or fp32, statistics [stats_words + GUARD] or None)"""
    c = o["case"]
    M, N, K, nb, lda, ldw, out_ld = (c[k] for k in ("M", "N", "K", "nb", "lda", "ldw", "out_ld"))
    a_bs, w_bs, o_bs = c["a_bs"], c["w_bs"], M * out_ld
    Aw = o["A"]
    Ww = o["A"] if o["W"] is None else o["W"]
    if mutant == "w_bs_for_a_bs":
        a_bs = w_bs
    if mutant == "vt_a_bs":
        a_bs = M * lda
    if mutant == "ktot_for_ldw":
        ldw = K
    Ku = K // 64 * 64 if mutant == "k_trunc64" else K
    alpha = torch.tensor(c["alpha"], dtype=torch.float32)
    if mutant == "alpha_dropped":
        alpha = torch.tensor(1.0)
    if mutant == "alpha_twice":
        alpha = alpha * alpha
    Af, Wf = R.from16(Aw, fmt), R.from16(Ww, fmt)
    m, n, k = torch.arange(M)[:, None], torch.arange(N)[:, None], torch.arange(Ku)[None, :]
    out = torch.full((out_words(c) + R.GUARD,), R.SENT32 if c["out_f32"] else R.SENT16,
                     dtype=torch.float32 if c["out_f32"] else torch.int16)
    st = torch.full((stats_words(c) + R.GUARD,), R.SENT32) if c["stats"] else None
    nblk = M // 32
    for z in range(nb):
        a = Af[(o["a_off"] + z * a_bs + m * lda + k) % Af.numel()]
        w = Wf[(o["w_off"] + z * w_bs + n * ldw + k) % Wf.numel()]
        v = (a @ w.T) * alpha  # fp32 accumulation, alpha in fp32
        if o["bias"] is not None:
            v = v + (o["bias"][torch.arange(M) % N][:, None] if mutant == "bias_by_row" else o["bias"][None, :])
        if o["resid"] is not None:
            v = v + R.from16(o["resid"][0 if mutant == "resid_no_zb" else z], fmt)
        rows = out[z * o_bs:(z + 1) * o_bs].view(M, out_ld)
        rows[:, :N] = v if c["out_f32"] else R.to16(v, fmt)
        if mutant == "pad_written" and out_ld > N:
            rows[:, N:] = 0
        if st is not None:
            zs = 0 if mutant == "stats_no_zb" else z
            st[zs * nblk * 2 * N:(zs + 1) * nblk * 2 * N] = _stats64(v[None].double())[0].float().reshape(-1)
    return out, st


def _err_over(es, rel, mean):
    if not es["finite"]:
        return float("inf")
    return max(es["rel_to_max"] / rel, es["mean_rel"] / mean)


def gemm_verify(o, out, st, fmt):
    """out / st: the flat buffers as they came back, guards included"""
    c = o["case"]
    M, N, nb, out_ld = c["M"], c["N"], c["nb"], c["out_ld"]
    sent = R.SENT32 if c["out_f32"] else R.SENT16
    rows = out[:out_words(c)].view(nb, M, out_ld)
    mism = (rows[..., N:] != sent).sum().item() + (out[out_words(c):] != sent).sum().item()
    got = rows[..., :N].contiguous()
    got = got if c["out_f32"] else R.from16(got, fmt)
    ref, ref_st = gemm_ref64(o, fmt)
    es = gs.err_stats(got, ref)
    r = dict(rel_to_max=es["rel_to_max"], mean_rel=es["mean_rel"], finite=es["finite"],
             err_over_tol=_err_over(es, gs.REL_TOL, gs.MEAN_TOL))
    if c["stats"]:
        mism += (st[stats_words(c):] != R.SENT32).sum().item()
        s = st[:stats_words(c)].view(ref_st.shape).double()
        serr = ((s - ref_st).abs().max() / ref_st.abs().max()).item() if bool(torch.isfinite(s).all()) else float("inf")
        r["stats_rel"] = serr
        r["err_over_tol"] = max(r["err_over_tol"], serr / gs.STATS_TOL)
    r["mismatch"] = int(mism)
    return r


def single_rounding_floor(o, fmt):
    """mean_rel / rel_to_max of the float64 reference rounded ONCE to the storage format: what no 16-bit output can beat"""
    ref, _ = gemm_ref64(o, fmt)
    return gs.err_stats(R.round16(ref.float(), fmt).float(), ref)


# ================================================================================================== AttnBlock core
def _core(name, B, C, T, branch, ldqk=None, ldo=None):
    return dict(name=name, B=B, C=C, T=T, Tpad=(T + 63) // 64 * 64, branch=branch, ldqk=ldqk or 2 * C, ldn=C, ldo=ldo or C)


CORE_CASES = [
    _core("core/flash_c128_t100", 2, 128, 100, BRANCH_FLASH, ldqk=2 * 128 + 8, ldo=128 + 8),
    _core("core/wide_c192_t96", 2, 192, 96, BRANCH_WIDE, ldqk=2 * 192 + 8, ldo=192 + 8),
    _core("core/wide_c192_t64", 2, 192, 64, BRANCH_WIDE),
    _core("core/wide_c320_t160", 2, 320, 160, BRANCH_WIDE),
    _core("core/wide_c512_t256", 1, 512, 256, BRANCH_WIDE),
]
CORE = _names(CORE_CASES)
CORE_REFUSED = _core("core/refused_c192_t100", 2, 192, 100, BRANCH_WIDE)


def _core_operands(c, fmt):
    g = R._gen("core" + c["name"])
    B, C, T = c["B"], c["C"], c["T"]
    scale_b = (1.0 + 0.25 * torch.arange(B).repeat_interleave(T).float())[:, None]
    qk = _nan_rows(torch.randn(B * T, 2 * C, generator=g), c["ldqk"], fmt)
    n = _nan_rows(torch.randn(B * T, C, generator=g) * scale_b, c["ldn"], fmt)
    wv = R.round16(torch.randn(C, C, generator=g) / math.sqrt(C), fmt).float()
    vbias = AF.OBIAS_STD * torch.randn(C, generator=g)
    qkf = R.from16(qk[:, :2 * C].contiguous(), fmt).view(B, T, 2 * C)
    return dict(case=c, qk=qk, n=n, wv=wv, vbias=vbias, q=qkf[..., :C].contiguous(), k=qkf[..., C:].contiguous(),
                nf=R.from16(n[:, :C].contiguous(), fmt).view(B, T, C))


@functools.lru_cache(maxsize=None)
def core_build(name, fmt):
    return _core_operands(CORE_REFUSED if name == CORE_REFUSED["name"] else CORE[name], fmt)


def core_ref64(o):
    """-> (softmax(C^-1/2 q k^T) v [B, T, C] WITHOUT the bias, v [B, T, C]), v in float64 from n and Wv"""
    c = o["case"]
    v = o["nf"].double() @ o["wv"].double().T
    s = (o["q"].double() @ o["k"].double().transpose(1, 2)) * (c["C"] ** -0.5)
    return torch.softmax(s, -1) @ v, v


def core_emulate(o, fmt, mutant=None):
    """-> (o words [B T ldo + GUARD], V^T words [B C Tpad + GUARD])"""
    c = o["case"]
    B, C, T, Tpad, ldo = c["B"], c["C"], c["T"], c["Tpad"], c["ldo"]
    v = R.round16(o["nf"] @ o["wv"].T, fmt)  # the V^T GEMM: fp32 sums, one rounding
    vt = torch.zeros(B, C, Tpad, dtype=torch.int16)
    vt[:, :, :T] = v.view(torch.int16).transpose(1, 2)
    alpha = torch.tensor(1.0 / math.sqrt(C), dtype=torch.float32)
    if mutant == "alpha_dropped":
        alpha = torch.tensor(1.0)
    if mutant == "alpha_twice":
        alpha = alpha * alpha
    s = (o["q"] @ o["k"].transpose(1, 2)) * alpha
    p = R.round16(sm_emulate_rows(s.reshape(B * T, T)), fmt).float().view(B, T, T)
    vf = v.float()
    if mutant == "v_batch0":
        vf = vf[:1].expand(B, T, C)
    out = torch.full((B * T * ldo + R.GUARD,), R.SENT16, dtype=torch.int16)
    out[:B * T * ldo].view(B * T, ldo)[:, :C] = R.to16((p @ vf).reshape(B * T, C) + o["vbias"][None, :], fmt)
    return out, torch.cat([vt.reshape(-1), torch.full((R.GUARD,), R.SENT16, dtype=torch.int16)])


def core_verify(o, out, vt, fmt):
    """out / vt as they came back (vt may be None) -> (result for o, result for V^T or None)"""
    c = o["case"]
    B, C, T, Tpad, ldo = c["B"], c["C"], c["T"], c["Tpad"], c["ldo"]
    f = fmt_factor(fmt)
    ref, v64 = core_ref64(o)
    rows = out[:B * T * ldo].view(B * T, ldo)
    mism = (rows[:, C:] != R.SENT16).sum().item() + (out[B * T * ldo:] != R.SENT16).sum().item()
    got = R.from16(rows[:, :C].contiguous(), fmt).double() - o["vbias"].double()[None, :]
    es = gs.err_stats(got.view(B, T, C), ref)
    ro = dict(rel_to_max=es["rel_to_max"], mean_rel=es["mean_rel"], finite=es["finite"], mismatch=int(mism),
              err_over_tol=_err_over(es, AF.REL * f, AF.MEAN * f))
    if vt is None:
        return ro, None
    w = vt[:B * C * Tpad].view(B, C, Tpad)
    mv = (w[:, :, T:] != 0).sum().item() + (vt[B * C * Tpad:] != R.SENT16).sum().item()
    ev = gs.err_stats(R.from16(w[:, :, :T].contiguous(), fmt), v64.transpose(1, 2))
    rv = dict(rel_to_max=ev["rel_to_max"], mean_rel=ev["mean_rel"], finite=ev["finite"], mismatch=int(mv),
              err_over_tol=_err_over(ev, gs.REL_TOL, gs.MEAN_TOL))
    return ro, rv


# ================================================================================================== softmax rows
SM_CASES = [
    dict(name="sm/r5_c96", rows=5, cols=96, kind="randn"),
    dict(name="sm/r3_c64", rows=3, cols=64, kind="randn"),
    dict(name="sm/r2_c4096", rows=2, cols=4096, kind="randn"),
    dict(name="sm/spike_r4_c300", rows=4, cols=300, kind="spike"),  # the maximum in the last column, the rest 80 below
    dict(name="sm/const_r2_c96", rows=2, cols=96, kind="const"),    # -> 1 / cols
]
SM = _names(SM_CASES)


@functools.lru_cache(maxsize=None)
def sm_build(name):
    c = SM[name]
    g = R._gen("sm" + name)
    if c["kind"] == "randn":
        s = torch.randn(c["rows"], c["cols"], generator=g) * 4
    elif c["kind"] == "spike":
        s = 20.0 + 0.5 * torch.randn(c["rows"], c["cols"], generator=g)
        s[:, -1] = 100.0 + torch.arange(c["rows"]).float()
    else:
        s = torch.tensor([3.5, -7.0])[:c["rows"], None].expand(c["rows"], c["cols"]).contiguous()
    return dict(case=c, s=s)


def sm_ref64(s):
    return torch.softmax(s.double(), -1)


def sm_emulate_rows(s, mutant=None):
    """k_softmax_rows in fp32: exp(s - max), their sum, the products with 1 / sum (not yet rounded to 16 bits)"""
    mx = torch.zeros(s.shape[0], 1) if mutant == "no_max" else s.max(-1, keepdim=True).values
    e = torch.exp(s - mx)
    return e * (1.0 / e.sum(-1, keepdim=True))


def sm_verify(o, got, fmt):
    """got fp32 [rows, cols]: the 16-bit result widened. Where float64 gives a word of the format exactly after one rounding
    and the kernel has no freedom (the spike rows: 1 in the last column, 0 where exp(-80) underflows the format), the word
    must be that one"""
    c = o["case"]
    ref = sm_ref64(o["s"])
    es = gs.err_stats(got, ref)
    mism = 0
    if c["kind"] == "spike":
        mism += (got[:, -1] != 1.0).sum().item()
        tiny = ref < 0.25 * R.step16(torch.zeros(()), fmt)  # under half the smallest subnormal, with room
        mism += (got[tiny] != 0).sum().item()
    return dict(rel_to_max=es["rel_to_max"], mean_rel=es["mean_rel"], finite=es["finite"], mismatch=int(mism),
                err_over_tol=_err_over(es, SM_REL, SM_MEAN))
