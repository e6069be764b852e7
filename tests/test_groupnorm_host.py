"""CPU: the tolerances of tests/test_gpu_groupnorm.py are honest. For every input the GPU tests use, an fp32 emulation of
the kernels' arithmetic in plain torch (tests/_groupnorm_ref.py) stays within HALF of the tolerance the GPU test applies
against the float64 reference - so a correct kernel has a factor two of room, and a case whose input makes fp32 itself
miss the bound is found here, not on the GPU. The references are checked against torch on the way."""
import pytest
import torch
import torch.nn.functional as F

import _groupnorm_ref as R
import _ops
from cycle_diffusion_amd import _ffi


def _fmt():
    fp16 = _ffi.load_library().cd_act_format() == 1
    return fp16, "fp16" if fp16 else "bf16"


def test_reference_matches_torch():
    g = torch.Generator().manual_seed(3)
    x = R.make_x(g, 3, 96, 8, 8).double()
    gamma, beta = torch.randn(96, generator=g).double(), torch.randn(96, generator=g).double()
    film = torch.randn(3, 192, generator=g).double()
    ref = F.group_norm(x, 32, gamma, beta, 1e-5)
    assert (R.ref64(x, gamma, beta, 1e-5) - ref).abs().max() < 1e-12
    ref = F.silu(ref * (1 + film[:, :96, None, None]) + film[:, 96:, None, None])
    assert (R.ref64(x, gamma, beta, 1e-5, film=film, silu=True) - ref).abs().max() < 1e-12
    shared = R.ref64(x, gamma, beta, 1e-5, film=film[1])
    assert (shared - R.ref64(x, gamma, beta, 1e-5, film=film[1][None].expand(3, -1))).abs().max() == 0
    # block statistics: summed over an image's blocks they are the image's channel sums
    st = R.block_stats(x).reshape(3, 2, 2, 96).sum(1)
    assert (st[:, 0] - x.sum((2, 3))).abs().max() < 1e-10 and (st[:, 1] - (x * x).sum((2, 3))).abs().max() < 1e-9
    # statistics of another tensor: the same as normalising with that tensor's mean and variance
    other = R.make_x(g, 3, 96, 8, 8, R.IMG_OFF_OTHER, R.IMG_SCALE_OTHER).double()
    og = other.reshape(3, 32, -1)
    want = ((x.reshape(3, 32, -1) - og.mean(2, keepdim=True)) / torch.sqrt(og.var(2, unbiased=False, keepdim=True) + 1e-5))
    got = R.ref64(x, torch.ones(96), torch.zeros(96), 1e-5, stats_of=other)
    assert (got - want.reshape(x.shape)).abs().max() < 1e-12


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES16])
def test_fp32_emulation_within_half_the_16bit_tolerance(name):
    fp16, fmt = _fmt()
    d = R.build16(name, _ops.bf16_round, fmt)
    assert torch.equal(d["x"], _ops.bf16_round(d["x"]))  # the input is representable in the storage format
    err = (d["emu"].double() - d["ref"]).abs()
    tol = R.tol16(d["ref"], fp16)
    print(name, "emulation max err / max|ref| %.3e" % (err.max() / d["ref"].abs().max()).item())
    assert torch.isfinite(d["emu"]).all()
    assert (err <= 0.5 * tol).all(), (name, (err / tol).max().item())
    if d["case"]["stats"] == "other":  # the proof cases: a result within tolerance is > 10 tolerances from the input's own GroupNorm
        assert (d["ref"] - d["ref_own"]).abs().max() > 11 * tol.max()


@pytest.mark.parametrize("names", R.PRODUCER_CHAINS, ids=["+".join(n) for n in R.PRODUCER_CHAINS])
def test_epilogue_statistics_before_rounding_fit_the_slack(names):
    """A conv epilogue sums its outputs before their 16-bit rounding; the GroupNorm reference of the composition tests is
    that of the stored (rounded) tensor. On the float64 conv results of the same operands the difference, with the fp32
    arithmetic on top, is within half the tolerance."""
    fp16, fmt = _fmt()
    ref, emu = R.producer_host(names, _ops.bf16_round, fmt)
    err = (emu.double() - ref).abs()
    print(names, "emulation max err / max|ref| %.3e" % (err.max() / ref.abs().max()).item())
    assert (err <= 0.5 * R.tol16(ref, fp16)).all(), (err / R.tol16(ref, fp16)).max().item()


def test_s_is_twice_what_the_emulation_needs():
    """GN16_S is derived, not chosen: at most twice the emulation's largest error (and not below it)."""
    fp16, fmt = _fmt()
    need = max(R.needed_s(_ops.bf16_round, fmt).values())
    assert 2.0 * need <= R.GN16_S[fp16] <= 2.1 * need, (need, R.GN16_S[fp16])


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES32])
def test_fp32_path_emulation_within_half_the_bound(name):
    """fp32 path: float64 statistics (folded from fp32 block sums where the case hands them in), fp32 coefficients and
    apply, against the bound derived from torch's own fp32 group_norm"""
    d = R.build32(name)
    err = (d["emu"].double() - d["ref"]).abs()
    tol = R.tol32(d["ref"], d["torch_err"], split=False)
    print(name, "emulation max err %.3e, bound %.3e" % (err.max().item(), tol.max().item()))
    assert (err <= 0.5 * tol).all(), (name, (err / tol).max().item())
    if d["case"]["stats"] == "other":
        assert (d["ref"] - d["ref_own"]).abs().max() > 11 * (tol + 2.0 ** -21 * d["ref"].abs()).max()
