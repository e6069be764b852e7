"""k_conv_gemm as the batched plain GEMM of the attention call sites, and the AttnBlock core built on it, against float64 -
through cd_op_gemm_batched / cd_op_attn_block_core: the test's own device bytes in, the kernels' bytes out.

Case tables, operands, references, bounds: tests/_gemm_batched_ref.py (its docstring maps kernel form -> cases).
tests/test_gemm_batched_host.py shows on the CPU that an emulation of the kernels' roundings stays within half of every bound
and that every mutant (a batch stride from the other operand, a_bs != 0 on the shared V weight, Ktot for ldw, alpha dropped or
doubled, bias by row, residual / statistics without zb, padding written, K cut to 64s) fails.

test_gemm_form, for every tile of the case (0 = the launcher's choice, 3, 2, 1, 24, and 5, 22 where M >= 256):
  (a) what ran: an explicit tile is the tile that ran, 32 deep where K % 64 != 0
  (b) float64 bounds (5e-3 / 2e-3, statistics 2e-3), output finite
  (c) bit-identical to nbatch launches with nbatch = 1 and the pointers advanced by the strides, same tile / depth / split
  (d) bit-identical to tile 3 at the same depth and split
  (e) every sentinel (padding columns) and guard word untouched
test_attn_block_core: o - vbias against float64 softmax(C^-1/2 q k^T) v, v in float64 from n and Wv, at the attention bounds
  (4e-3 f / 1.5e-3 f, f = 1 fp16, 8 bf16); V^T at the GEMM bounds with zero padding columns; the branch flag; and for the wide
  cases o bit for bit equal to cd_op_gemm_batched (S form) -> cd_op_softmax_rows -> cd_op_gemm_batched (O form) on the
  returned V^T - which ties at_core's parameters to the forms verified above.
test_attn_block_core_refuses_ragged_tokens: T = 100 at C = 192 is a CD_CHECK, the output stays the sentinel.

Measured on MI355X, the materialised chain (wide cases, o - vbias against float64; rows attn_block/... of the parity report) -
the host emulation of tests/test_gemm_batched_host.py gives the same figures to three digits:
  fp16  rel_to_max 4.0-5.0e-4, mean_rel 3.4-3.7e-4   (bounds 4e-3 / 1.5e-3)
  bf16  rel_to_max 3.5-5.4e-3, mean_rel 2.8-3.0e-3   (bounds 3.2e-2 / 1.2e-2)
the flash case: fp16 5.7e-4 / 3.9e-4, bf16 6.6e-3 / 3.1e-3. GEMM forms, err / bound: 16-bit output 0.088 (fp16), 0.70-0.71 (bf16:
one rounding to 8 significant bits is 0.70 of 5e-3 / 2e-3 by itself); fp32 output 4-7e-5; statistics 1.6e-7 of 2e-3. All
outputs bit-identical across batch forms and tiles; the launcher's own choice (tile 0) was tile 3 or 8.
"""
import numpy as np
import pytest
import torch

import _gemm_batched_ref as G
import _glue_ref as R
import _ops

pytestmark = pytest.mark.gpu

FMT = R.lib_fmt()
SENT = dict(guard=R.GUARD, sent16=R.SENT16, sent32=R.SENT32)


def _same(a, b):
    """bit for bit (fp32 buffers compared as words: the sentinel and NaN-free values alike)"""
    if a is None and b is None:
        return True
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def _add(report, name, r, **kw):
    report.add(name, **{k: v for k, v in r.items()}, **kw)
    print("%-44s %s %s" % (name, {k: ("%.3e" % v if isinstance(v, float) else v) for k, v in r.items()}, kw))


@pytest.mark.parametrize("name", list(G.GEMM))
def test_gemm_form(engine, report, name):
    o = G.gemm_build(name, FMT)
    c = o["case"]
    anchors = {}

    def anchor(bk, split):
        if (bk, split) not in anchors:
            out, st, rb = _ops.gemm_batched(engine, o, G.anchor_tile(c, bk, split), **SENT)
            assert (rb[0]["tile"], rb[0]["bk"], rb[0]["split"]) == (3, bk, split), rb
            anchors[(bk, split)] = (out, st)
        return anchors[(bk, split)]

    failures = []
    for tile in G.gemm_tiles(c):
        out, st, rb = _ops.gemm_batched(engine, o, tile, **SENT)
        ran = (rb[0]["tile"], rb[0]["bk"], rb[0]["split"])
        key = "gemm_batched/%s/t%d" % (name, tile)
        if tile:  # (a)
            if ran != G.expected_launch(c, tile):
                failures.append((key, "ran", ran, G.expected_launch(c, tile)))
        elif c["K"] % 64 and ran[1] != 32:
            failures.append((key, "depth", ran))
        r = G.gemm_verify(o, out, st, FMT)  # (b), (e)
        # (c) the same tile, depth and split, one batch element per launch
        explicit = ran[0] | ((ran[2] if ran[2] > 1 else 0) << 8) | ((1 << 16) if (ran[1] == 32 and c["K"] % 64 == 0) else 0)
        out1, st1, rb1 = _ops.gemm_batched(engine, o, explicit, singles=True, **SENT)
        batch_same = _same(out, out1) and _same(st, st1) and all((x["tile"], x["bk"], x["split"]) == ran for x in rb1)
        # (d) tile 3 at that depth and split: the output (the statistics' 32-row sums are added in an order that follows the
        # tile's chunk width: held to STATS_TOL above, and bit for bit to the single launches of the same tile)
        out3, _ = anchor(ran[1], ran[2])
        tile_same = _same(out, out3)
        _add(report, key, r, bit_identical=bool(batch_same and tile_same), ran="t%d bk%d s%d" % ran)
        if not (r["finite"] and r["err_over_tol"] <= 1.0):
            failures.append((key, "float64 bounds", r))
        if r["mismatch"]:
            failures.append((key, "sentinel / guard words", r["mismatch"]))
        if not batch_same:
            failures.append((key, "differs from nbatch single launches", rb1))
        if not tile_same:
            failures.append((key, "differs from tile 3", ran))
    assert not failures, failures


@pytest.mark.parametrize("name", list(G.CORE))
def test_attn_block_core(engine, report, name):
    o = G.core_build(name, FMT)
    c = o["case"]
    B, T, Cc, Tpad, ldo = c["B"], c["T"], c["C"], c["Tpad"], c["ldo"]
    out, vt, branch = _ops.attn_block_core(engine, o, R.GUARD, R.SENT16)
    ro, rv = G.core_verify(o, out, vt, FMT)
    same = None
    if c["branch"] == G.BRANCH_WIDE:
        # the chain on the same operands: S = alpha q k^T (fp32) -> softmax rows -> P (16 bits, exact) -> P V^T^T + vbias
        qk = o["qk"].cuda()
        S = torch.empty((B, T, T), device="cuda", dtype=torch.float32)
        alpha = float(np.float32(1.0) / np.sqrt(np.float32(Cc)))  # at_core's 1.0f / sqrtf((float)D), D = C with one head
        _ops.gemm_raw(engine, qk, c["ldqk"], T * c["ldqk"], _ops._at(qk, Cc), c["ldqk"], T * c["ldqk"], T, T, Cc, B, alpha,
                      None, S, T, 1)
        Pf = _ops.softmax_rows_dev(engine, S.view(B * T, T))
        P16 = Pf.to(torch.float16 if FMT == "fp16" else torch.bfloat16)
        assert torch.equal(P16.float(), Pf)  # the widened 16-bit values: rounding back is exact
        vt_dev = vt[:B * Cc * Tpad].cuda()
        chain = _ops._out16(B * T * ldo, R.GUARD, R.SENT16)
        vb = o["vbias"].cuda()
        _ops.gemm_raw(engine, P16.view(torch.int16), T, T * T, vt_dev, Tpad, Cc * Tpad, T, Cc, T, B, 1.0, vb, chain, ldo, 0)
        same = bool(torch.equal(chain.cpu(), out))
    _add(report, "attn_block/" + name, ro, bit_identical=same, branch=branch)
    _add(report, "attn_block/" + name + "/vt", rv)
    assert branch == c["branch"], branch
    assert ro["finite"] and ro["mismatch"] == 0 and ro["err_over_tol"] <= 1.0, ro
    assert rv["finite"] and rv["mismatch"] == 0 and rv["err_over_tol"] <= 1.0, rv
    assert same is not False, "o differs from cd_op_gemm_batched -> cd_op_softmax_rows -> cd_op_gemm_batched"


def test_attn_block_core_refuses_ragged_tokens(engine):
    """the materialised branch needs T % 32 == 0: a host-side CD_CHECK ahead of its launches, the output untouched"""
    o = G.core_build(G.CORE_REFUSED["name"], FMT)
    msg, out = _ops.attn_block_core(engine, o, R.GUARD, R.SENT16, want_vt=False, refusal=True)
    assert "must be a multiple of 32" in msg, msg
    assert (out == R.SENT16).all()
