"""The small HBM-bound kernels of csrc/elementwise.hip, one by one, through the bare entry points (cd_op_layout, cd_op_resample16,
cd_op_copy_rows16, cd_op_vec_linear, cd_op_tokens, cd_op_posterior_sample, cd_op_vq_quantize): the test's own device bytes in,
one launch, the kernel's bytes out. No staging kernel of the engine's sits on either side - k_nchw_to_nhwc and k_nhwc_to_nchw,
which stage every other op test, are themselves under test here.

Operands, float64 references, tolerances and exact checks come from tests/_glue_ref.py; tests/test_glue_host.py shows on the
CPU that an fp32 emulation of every case stays within half its tolerance and that every mutant (W decoded for Wo, Cpad for C,
padding not zeroed, a dup copy at the wrong offset, a pool of three taps, pos[b L + l], the last maximum, vec_linear without
segment 3 / its second trip / its bias / with SiLU on the wrong side, a posterior without clamp or with exp(lv), VQ with <= or
without e^2) fails. Padding columns of strided operands hold NaN, output buffers start as a sentinel and carry a guard of
sentinel words. Every case writes err_over_tol and its mismatching words to the parity report (glue/...).

kernel                  cases
k_nchw_to_nhwc          test_nchw_to_nhwc: C = 3 -> Cpad = 32 with dup 0 / 1 and scale, shift = 1, 0 (exact) / 1/0.18215, 0.25; the
                        rows form (HW = 1, B = 77); +-70000 saturating in the fp16 build; the grid-stride wrap
k_nhwc_to_nchw          test_nhwc_to_nchw: 16-bit rows C = 80 of 96 (exact), fp32 rows 5 of 8, both with 0.5, 0.5; HW = 1; the wrap
k_avgpool2              test_resample[pool_*]: B = 2, 6 x 10 and the odd 7 x 5, 5 vectors per pixel, scales 1 / 3e-5 / 200; the wrap
k_upsample2             test_resample[up_*] (exact)
k_copy_strided_bf16     test_copy_rows: 77 x 40 from stride 48 to 64, the dup_rows pattern in two launches, the wrap (all exact)
launch_* refusals       test_vector_launchers_refuse_c12 (pool, upsample, copy: C = 12), test_vq_refusals (zc = 9, > 150 KB)
k_vec_linear            test_vec_linear: one vector; the tiny networks' K = 32; four segments in one trip; the second trip with one
                        lane and at the SD width 1280; the scalar path by K % 4 and by ldx % 4; no bias; ldy > N
k_embed_tokens          test_tokens[embed_*]: ids -1, vocab, vocab + 5 clamped; the wrap (exact)
k_vit_tokens            test_tokens[vit_*] (exact)
k_gather_eot            test_tokens[eot_*]: the maximum first, last and tied; D = 40 and 1280 (exact)
k_posterior_sample      test_posterior_sample: zc 3 / 4, ld = 2 zc and 2 zc + 4, log-variances over [-40, 30], use_mean with a NaN
                        log-variance half and no noise; the wrap. (noise = NULL with use_mean = 0: tests/test_gpu_philox.py)
k_vq_quantize           test_vq_quantize: 256 x 3, the 96 KB codebook 8192 x 3, 37 x 1, 1000 x 8, in_mul 1 and 1/0.18215, exact
                        ties, the wrap above 512 x 256 threads
"""
import pytest
import torch

import _glue_ref as R
import _ops

pytestmark = pytest.mark.gpu

FMT = R.lib_fmt()
G = dict(guard=R.GUARD)


def _check(report, name, r):
    report.add("glue/" + name, err_over_tol=r["ratio"], mismatch=r["mismatch"],
               **{k: v for k, v in r.items() if k not in ("ratio", "mismatch")})
    print("glue/%s err / tol %.3f, %d mismatching words %s" % (name, r["ratio"], r["mismatch"],
                                                              {k: v for k, v in r.items() if k not in ("ratio", "mismatch")}))
    assert r["mismatch"] == 0, (name, r)
    assert r["ratio"] <= 1.0, (name, r)


@pytest.mark.parametrize("name", list(R.N2H))
def test_nchw_to_nhwc(engine, report, name):
    o = R.n2h_build(name)
    c = o["case"]
    got = _ops.glue_nchw_to_nhwc(engine, o["x"], c["Cpad"], c["scale"], c["shift"], c["dup"], sent=R.SENT16, **G)
    if c["sat"] and FMT == "fp16":  # x[0, 0, 0] = 70000, x[0, 0, 1] = -70000: column 0 of rows 0 and 1
        assert R.from16(got[:2 * c["Cpad"]:c["Cpad"]].contiguous(), FMT).tolist() == [65504.0, -65504.0]
    _check(report, "nchw_to_nhwc/" + name, R.n2h_verify(o, got, FMT))


@pytest.mark.parametrize("name", list(R.H2N))
def test_nhwc_to_nchw(engine, report, name):
    o = R.h2n_build(name, FMT)
    c = o["case"]
    got = _ops.glue_nhwc_to_nchw(engine, o["x"], c["B"], c["C"], c["HW"], c["scale"], c["shift"], sent=R.SENT32, **G)
    _check(report, "nhwc_to_nchw/" + name, R.h2n_verify(o, got, FMT))


@pytest.mark.parametrize("name", list(R.RESAMPLE))
def test_resample(engine, report, name):
    o = R.resample_build(name, FMT)
    got = _ops.glue_resample16(engine, o["case"]["op"], o["x"], sent=R.SENT16, **G)
    _check(report, "resample16/" + name, R.resample_verify(o, got, FMT))


@pytest.mark.parametrize("name", list(R.COPY))
def test_copy_rows(engine, report, name):
    o = R.copy_build(name)
    c = o["case"]
    got = _ops.glue_copy_rows16(engine, o["src"], c["ldd"], c["cols"], R.copy_launches(c), c["rows"] + c["tail"], sent=R.SENT16, **G)
    _check(report, "copy_rows16/" + name, R.copy_verify(o, got))


def test_vector_launchers_refuse_c12(engine):
    """a channel / column count that is no multiple of 8 would lose its tail: the launchers refuse it and launch nothing"""
    x = torch.zeros((1, 2, 2, 12), dtype=torch.int16)
    for op in ("avgpool", "upsample"):
        msg, y = _ops.glue_resample16(engine, op, x, sent=R.SENT16, refusal=True, **G)
        assert "16-byte vectors" in msg, msg
        assert (y == R.SENT16).all()
    src = torch.zeros((4, 16), dtype=torch.int16)
    msg, y = _ops.glue_copy_rows16(engine, src, 16, 12, [(0, 0, 4)], 4, sent=R.SENT16, refusal=True, **G)
    assert "16-byte vectors" in msg and (y == R.SENT16).all(), msg
    # strides that are no multiple of 8: refused as well
    msg, y = _ops.glue_copy_rows16(engine, torch.zeros((4, 12), dtype=torch.int16), 16, 8, [(0, 0, 4)], 4, sent=R.SENT16,
                                   refusal=True, **G)
    assert "16-byte vectors" in msg and (y == R.SENT16).all(), msg


@pytest.mark.parametrize("name", list(R.VEC))
def test_vec_linear(engine, report, name):
    o = R.vec_build(name)
    c = o["case"]
    got = _ops.glue_vec_linear(engine, o["x"], o["W"], o["bias"], c["K"], c["ldy"], c["silu_in"], c["silu_out"], sent=R.SENT32)
    _check(report, "vec_linear/" + name, R.vec_verify(o, got))


@pytest.mark.parametrize("name", list(R.TOKENS))
def test_tokens(engine, report, name):
    o = R.tokens_build(name, FMT)
    c = o["case"]
    got = _ops.glue_tokens(engine, c["op"], c["B"], c["L"], c["D"], c["vocab"], R.tokens_out_words(c), sent=R.SENT16,
                           ids=o.get("ids"), x16=o.get("x16"), tok=o.get("tok"), pos=o.get("pos"), **G)
    _check(report, "tokens/" + name, R.tokens_verify(o, got, FMT))


@pytest.mark.parametrize("name", list(R.POST))
def test_posterior_sample(engine, report, name):
    o = R.post_build(name)
    c = o["case"]
    got = _ops.glue_posterior_sample(engine, o["mom"], o["noise"], c["B"], c["zc"], c["HW"], c["scale"], c["use_mean"],
                                     sent=R.SENT32, **G)
    assert torch.isfinite(got).all()  # use_mean: the NaN log-variances and the absent noise were not read
    _check(report, "posterior_sample/" + name, R.post_verify(o, got))


@pytest.mark.parametrize("name", list(R.VQ))
def test_vq_quantize(engine, report, name):
    o = R.vq_build(name)
    c = o["case"]
    got = _ops.glue_vq_quantize(engine, o["z"], c["in_mul"], o["cb"], c["B"], c["HW"], c["Cpad"], sent=R.SENT16, **G)
    _check(report, "vq_quantize/" + name, R.vq_verify(o, got, FMT))


def test_vq_refusals(engine):
    z9, cb9 = torch.zeros(1, 9, 4), torch.zeros(16, 9)
    msg, y = _ops.glue_vq_quantize(engine, z9, 1.0, cb9, 1, 4, 32, sent=R.SENT16, refusal=True, **G)
    assert "embed_dim 9" in msg and (y == R.SENT16).all(), msg
    n = 150 * 1024 // 4 + 1  # one code more than 150 KB of fp32
    msg, y = _ops.glue_vq_quantize(engine, torch.zeros(1, 1, 4), 1.0, torch.zeros(n, 1), 1, 4, 32, sent=R.SENT16, refusal=True, **G)
    assert "does not fit LDS" in msg and (y == R.SENT16).all(), msg
