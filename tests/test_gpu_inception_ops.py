"""GPU: the three hand-written kernels of the FID Inception-v3 (k_pool3x3<MAX>, k_global_avg, k_fold_bn) and the forms in which
its BasicConv2d units launch the implicit GEMM (csrc/inception.hip), one at a time against float64, through the launchers the
network itself calls (cd_op_pool3x3, cd_op_global_avg, cd_op_basic_conv). Case tables, references and the reasoning behind every
bound: tests/_inception_ops_ref.py; tests/test_inception_ops_host.py holds the same bounds against fp32 restatements on the host.

Every operand is stored the way the network stores it - a row stride wider than the channel count, NaN in the pad columns - and
every output lands at a column offset of a NaN-prefilled buffer with 64 NaN rows behind it: a read past the operand or a store
outside the slice shows.

Measured on MI355X, fp16 build (rows inception_ops/... of the parity report):
  max pools      bit-exact in all 6 cases x 16 variants
  average pools  every output of all 3 cases x 16 variants equals the correctly rounded value (largest share that differs: 0;
                 err / bound 0): a sum of 16-bit values divided by 4, 6 or 9 lies at least 1/18 of its quantum from a rounding
                 tie, far more than the fp32 arithmetic moves it. The divisor-9 reference fails on every border element.
  global average worst err / bound 0.035 (hw49_c2048_pad8): the bound is a worst case, the error of 49 additions is not
  BN fold        weights 0 or exactly 1 ulp16 from the float64 fold rounded once (tight), bias worst 0.31 of its bound
  conv forms     worst rel_to_max 4.0e-4, mean_rel 1.8e-4 (the 16-bit rounding of the output); tile 0 ran tiles 3 and 8
"""
import pytest
import torch

import _inception_ops_ref as ir
import _ops

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 3 x 3 pools
@pytest.mark.parametrize("c", ir.POOL_CASES, ids=[c["name"] for c in ir.POOL_CASES])
def test_pool3x3(engine, report, c):
    fmt = ir.lib_fmt()
    B, stride, pad = c["B"], c["stride"], c["pad"]
    Ho, Wo = ir.pool_out_hw(c["H"], c["W"], stride, pad)
    failures, worst, off_rounded, worst_fail9 = [], 0.0, 0.0, 1.0
    for C, in_pad, (off, ld), kind in ir.pool_variants(c):
        tag = "%s/c%d_pad%d_at%d_of%d_%s" % (c["name"], C, in_pad, off, ld, kind)
        x = ir.pool_input(c, C, kind, fmt)
        buf = _ops.pool3x3(engine, x.float(), c["max"], stride, pad, in_pad=in_pad, out_off=off, out_ld=ld).double()
        rows, outside, nan_inside = ir.slice_report(buf, B * Ho * Wo, off, C)
        if outside or nan_inside:  # a store outside the slice / a NaN read from the pad columns or left unwritten
            failures.append((tag, "written outside the slice: %d, NaN inside: %d" % (outside, nan_inside)))
            continue
        got = ir.rows_to_nchw(rows, B, Ho, Wo)
        if c["max"]:
            same = torch.equal(got, ir.max_pool_ref(x, stride, pad))
            print("%-48s bit-exact %s" % (tag, same))
            if not same:
                failures.append((tag, "not the maximum of the in-image taps"))
            continue
        v = ir.avg_verify(got, x, stride, pad, fmt)
        v9 = ir.avg_verify(got, x, stride, pad, fmt, divisor9=True)
        print("%-48s err/bound %.3f correctly rounded %.4f | divisor 9: err/bound %.1f, border elements failing %.2f"
              % (tag, v["ratio"], v["equal"], v9["ratio"], v9["border_fail"]))
        worst, off_rounded = max(worst, v["ratio"]), max(off_rounded, 1.0 - v["equal"])
        worst_fail9 = min(worst_fail9, v9["border_fail"])
        if not (v["ratio"] <= 1.0 and v["equal"] >= 0.95):
            failures.append((tag, "average pool", v))
        if not (v9["ratio"] > 1.0 and v9["border_fail"] >= 0.5):  # the test must tell count_include_pad = True apart
            failures.append((tag, "the divisor-9 reference was not rejected on the border", v9))
    if c["max"]:
        report.add("inception_ops/pool/" + c["name"], variants=len(ir.pool_variants(c)), bit_exact=not failures)
    else:
        report.add("inception_ops/pool/" + c["name"], variants=len(ir.pool_variants(c)), err_over_bound=worst,
                   share_not_correctly_rounded=off_rounded, divisor9_border_fail_min=worst_fail9)
    assert not failures, failures


def test_pool3x3_refusals(engine):
    x = torch.zeros(1, 8, 5, 5)
    for kw in (dict(in_pad=4), dict(out_off=4, out_ld=16), dict(out_off=8, out_ld=8), dict(out_ld=12)):
        with pytest.raises(_ops._ffi.EngineError):
            _ops.pool3x3(engine, x, True, 1, 1, **kw)
    with pytest.raises(_ops._ffi.EngineError):
        _ops.pool3x3(engine, torch.zeros(1, 12, 5, 5), True, 1, 1)  # C % 8


# ------------------------------------------------------------------------------------------------ global average pool
@pytest.mark.parametrize("c", ir.GAVG_CASES, ids=[c["name"] for c in ir.GAVG_CASES])
def test_global_avg(engine, report, c):
    x = ir.gavg_input(c, ir.lib_fmt())
    got = _ops.global_avg(engine, x.float(), in_pad=c["in_pad"])
    assert got.shape == (c["B"], c["C"]) and bool(torch.isfinite(got).all())
    r = ir.gavg_verify(got, x)
    print("global_avg %-20s err/bound %.3f" % (c["name"], r))
    report.add("inception_ops/global_avg/" + c["name"], err_over_bound=r)
    assert r <= 1.0, r


# ------------------------------------------------------------------------------------------------ BN fold and conv forms
@pytest.mark.parametrize("c", ir.CONV_CASES, ids=[c["name"] for c in ir.CONV_CASES])
def test_basic_conv_forms(engine, report, c):
    fmt = ir.lib_fmt()
    o = ir.conv_operands(c, fmt)
    failures = []
    for tile in ir.CONV_TILES:
        buf, wp, bo, rb = _ops.basic_conv(engine, o["x"], o["w"], o["gamma"], o["beta"], o["mean"], o["var"], stride=c["stride"],
                                          pad=c["pad"], in_ld=c["in_ld"], out_off=c["off"], out_ld=c["ld"], tile=tile)
        assert rb["chm"] == 0 and (tile == 0 or (rb["tile"], rb["split"]) == (tile, 1)), rb  # tap-major at these sizes
        fails, fig = ir.check_basic_conv(c, o, buf, wp, bo, fmt)
        print("%-28s tile %d -> %2d bk %d  %s" % (c["name"], tile, rb["tile"], rb["bk"],
                                                 " ".join("%s %.3e" % kv for kv in sorted(fig.items()))))
        report.add("inception_ops/conv/%s/tile%d" % (c["name"], tile), tile_ran=rb["tile"], bk=rb["bk"], **fig)
        failures += [(c["name"], "tile %d" % tile) + f for f in fails]
    assert not failures, failures


def test_basic_conv_refusals(engine):
    c = ir.CONV["3x3_n32_dense"]
    o = ir.conv_operands(c, ir.lib_fmt())
    run = lambda **kw: _ops.basic_conv(engine, o["x"], o["w"], o["gamma"], o["beta"], o["mean"], o["var"], pad=c["pad"], **kw)
    for kw in (dict(out_off=4, out_ld=64), dict(out_off=8, out_ld=32), dict(out_off=32, out_ld=56), dict(in_ld=32), dict(in_ld=68)):
        with pytest.raises(_ops._ffi.EngineError):
            run(**kw)
    with pytest.raises(_ops._ffi.EngineError):  # N = 80 runs 96 columns: a row of 88 does not hold them
        c80, o80 = ir.CONV["1x1_n80"], ir.conv_operands(ir.CONV["1x1_n80"], ir.lib_fmt())
        _ops.basic_conv(engine, o80["x"], o80["w"], o80["gamma"], o80["beta"], o80["mean"], o80["var"], out_ld=88)
