"""GroupNorm(32) as the networks run it (cd_op_groupnorm_ex -> groupnorm_fwd) against float64: the fold of the producing
convs' block statistics (k_gn_fold, k_gn_fold_f32), two concatenated sources with their own row strides on every path, the
fallbacks to the tensor's own statistics, FiLM rows per image / padded / shared, the fp32 path and its split output with
the range guard, batch invariance bit for bit, and the composition conv epilogue -> fold.

Inputs (tests/_groupnorm_ref.py): every image has its own offset and scale and every channel its own offset, so a wrong image,
channel, C0/C1 slot or sum / sum-of-squares slot moves the result by O(1); pad columns, unused statistics and FiLM padding
hold NaN. Tolerances are derived there and verified on the host by tests/test_groupnorm_host.py:
  16-bit  |got - ref| <= u |ref| + s max|ref|, u = one ulp of the storage format, s = twice what an fp32 emulation needs
  fp32    4 x the error of torch's own fp32 group_norm on the same input (floor 2^-22 max|ref|), + 2^-21 |ref| for the split pair
"""
import pytest
import torch

import _groupnorm_ref as R
import _ops
from _ops import bf16_round as r16
from cycle_diffusion_amd import _ffi

pytestmark = pytest.mark.gpu


def _fmt():
    fp16 = _ffi.load_library().cd_act_format() == 1
    return fp16, "fp16" if fp16 else "bf16"


def _check(report, name, got, ref, tol):
    got = got.double()
    err = (got - ref).abs()
    ratio = (err / tol).max().item()
    report.add("groupnorm_ex/" + name, max_abs=err.max().item(), rel_to_max=(err.max() / ref.abs().max()).item(),
               err_over_tol=ratio, finite=bool(torch.isfinite(got).all().item()))
    print("groupnorm_ex/%s max|err| %.3e (%.3e of max|ref|), err / tol %.3f" %
          (name, err.max().item(), (err.max() / ref.abs().max()).item(), ratio))
    assert torch.isfinite(got).all(), name
    assert (err <= tol).all(), (name, ratio)
    return err


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES16])
def test_groupnorm_16bit(engine, report, name):
    """fold/      caller-built block statistics of the input (k_gn_fold): 1, 3, 60 and 80 channels per group, a group across the
                  concat seam, fewer and more items than threads, FiLM at film_ld 2C, 2C + 64 and 0
    proof/        statistics of a DIFFERENT tensor: the result follows them (the fold ran), > 10 tolerances from the input's own
    fallback/     NaN statistics that must not be read: HW % 32 != 0, a padded row stride, a second source without statistics
    tensor/       k_gn_stats / k_gn_coef / k_gn_apply on two sources: padded strides, two vectors per thread across C0, ragged slabs
    large_mean/   per-group offset 6, spread 0.5 (mean^2 / var ~ 140) through the one-pass E[x^2] - mean^2, both paths: the fp32
                  emulation is 1.1e-5 of max|ref| off float64 here (fp16 inputs), inside half the tolerance at offset 6"""
    fp16, fmt = _fmt()
    d = R.build16(name, r16, fmt)
    got = _ops.groupnorm_ex(engine, d["x0"], d["gamma"], d["beta"], d["case"]["eps"], **R.call_args(d))
    tol = R.tol16(d["ref"], fp16)
    _check(report, name, got, d["ref"], tol)
    if d["case"]["stats"] == "other":
        assert ((got.double() - d["ref_own"]).abs().max() > 10 * tol.max()).item(), name


@pytest.mark.parametrize("names", R.PRODUCER_CHAINS, ids=["+".join(n) for n in R.PRODUCER_CHAINS])
def test_groupnorm_after_conv_epilogue(engine, report, names):
    """conv (16-bit output + epilogue statistics) -> GroupNorm + SiLU through the fold: a plain 3x3 conv, a split-K tile, the
    x2-upsample conv (blocks in phase order), and a concat of two different convs. Reference: float64 GroupNorm of the
    returned tensor (the epilogue sums before the 16-bit rounding; the host test shows that inside the slack)."""
    fp16, fmt = _fmt()
    ys, sts, gammas, betas = [], [], [], []
    for n in names:
        o = R.conv_operands_for(n, r16, fmt)
        y, st = _ops.conv2d16(engine, o["x"], o["w"], pad=1, bias=o["bias"], up=o["up"], tile=o["tile"], want_stats=True)
        assert (y.double() - o["y64"]).abs().max() < 5e-3 * o["y64"].abs().max()  # the producer itself (test_conv2d_16bit_epilogue)
        if n == "conv3x3_split3":
            assert _ops.last_gemm_config(engine)["split"] == 3
        ys.append(y), sts.append(st), gammas.append(o["gamma"]), betas.append(o["beta"])
    gamma, beta = torch.cat(gammas), torch.cat(betas)
    ref = R.ref64(torch.cat(ys, 1), gamma, beta, 1e-5, silu=True)
    got = _ops.groupnorm_ex(engine, ys[0], gamma, beta, 1e-5, x1=ys[1] if len(ys) > 1 else None, silu=True, stats0=sts[0],
                            stats1=sts[1] if len(sts) > 1 else None)
    _check(report, "producer/" + "+".join(names), got, ref, R.tol16(ref, fp16))
    # and the fold really consumed them: the tensor path on the same tensor is a different (if close) computation
    own = _ops.groupnorm_ex(engine, ys[0], gamma, beta, 1e-5, x1=ys[1] if len(ys) > 1 else None, silu=True)
    _check(report, "producer_tensor_path/" + "+".join(names), own, ref, R.tol16(ref, fp16))


def _run16(engine, d, sl, with_stats, rep=1):
    """the case's images `sl` (repeated `rep` times along the batch), statistics cut to the same images"""
    c = d["case"]
    nb = c["H"] * c["W"] // 32
    cut = lambda t: t[sl].repeat(rep, *([1] * (t.dim() - 1))).contiguous() if t is not None else None
    cut_st = lambda t: cut(t.reshape(c["B"], nb, 2, -1)).reshape(-1, 2, t.shape[2]) if t is not None and with_stats else None
    film = d["film"]
    return cut(d["x0"]), dict(x1=cut(d["x1"]), silu=c["silu"], film=cut(film) if film is not None else None,
                              stats0=cut_st(d["st0"]), stats1=cut_st(d["st1"]))


@pytest.mark.parametrize("name", ["fold/c64+32_film_2C", "fold/c320_64x32_silu", "fold/c1280+640"])
@pytest.mark.parametrize("path", ["fold", "tensor"])
@pytest.mark.parametrize("precision", [0, 1, 2])
def test_groupnorm_batch_invariance(engine, name, path, precision):
    """An image's result does not depend on the batch it travels in, bit for bit (groupnorm_slabs): image 1
    of a batch of 3 (2 where the case has 2) against the same image alone, and image 0 of a batch against that batch
    duplicated, which is how the CFG decode pass presents it. Fold and tensor statistics; 16-bit, fp32 and split."""
    fp16, fmt = _fmt()
    d = R.build16(name, r16, fmt)
    B = d["case"]["B"]
    run = lambda sl, rep=1: (lambda x0, kw: _ops.groupnorm_ex(engine, x0, d["gamma"], d["beta"], 1e-5, precision=precision,
                                                              **kw))(*_run16(engine, d, sl, path == "fold", rep))
    full = run(slice(0, B))
    i = B - 1 if B < 3 else 1
    assert torch.equal(run(slice(i, i + 1))[0], full[i])
    dup = run(slice(0, B), rep=2)
    assert torch.equal(dup[:B], full) and torch.equal(dup[B:], full)


@pytest.mark.parametrize("precision", [1, 2], ids=["f32", "split"])
@pytest.mark.parametrize("name", [c["name"] for c in R.CASES32])
def test_groupnorm_f32(engine, report, name, precision):
    """The fp32 path (k_gn_partial_f32 both branches, k_gn_coef_f32, k_gn_fold_f32, k_gn_apply_f32) and its split-fp16
    output, on fp32 inputs: single source, concat, padded strides, C4 > 256, no fold at HW = 36, caller-built statistics and
    the different-tensor proof, FiLM and SiLU."""
    d = R.build32(name)
    got = _ops.groupnorm_ex(engine, d["x0"], d["gamma"], d["beta"], d["case"]["eps"], precision=precision, **R.call_args(d))
    tol = R.tol32(d["ref"], d["torch_err"], split=precision == 2)
    _check(report, "%s_p%d" % (name, precision), got, d["ref"], tol)
    if d["case"]["stats"] == "other":
        assert ((got.double() - d["ref_own"]).abs().max() > 10 * tol.max()).item(), name


def test_groupnorm_split_range_guard(engine):
    """The split representation holds |y| < 4094: a gain that pushes outputs past it makes the call fail with the range
    error; the next call on the same engine is unaffected."""
    d = R.build32("f32/c96")
    with pytest.raises(_ffi.EngineError, match="fp16 range"):
        _ops.groupnorm_ex(engine, d["x0"], d["gamma"] * 5000.0, d["beta"], 1e-5, precision=2)
    got = _ops.groupnorm_ex(engine, d["x0"], d["gamma"], d["beta"], 1e-5, precision=2)
    tol = R.tol32(d["ref"], d["torch_err"], split=True)
    assert ((got - d["ref"]).abs() <= tol).all()
    # the fp32 output has no such limit
    big = _ops.groupnorm_ex(engine, d["x0"], d["gamma"] * 5000.0, d["beta"], 1e-5, precision=1)
    assert torch.isfinite(big).all() and big.abs().max() > 4094
