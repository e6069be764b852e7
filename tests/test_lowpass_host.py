"""CPU: ILVR's low-pass filter on the host (cycle-diffusion_amd/utils/lowpass.py), the schedule rows of the conditioning, the
fp32 emulation of the kernels against the bound the GPU test asserts, and the wrapper's constructor checks."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _ilvr_ref as ir
from cycle_diffusion_amd import schedule
from cycle_diffusion_amd.utils import lowpass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(32, 4), (32, 8), (64, 16), (256, 32)]


def _direct(n_in, n_out):
    """resize_matrix written output by output, tap by tap, without the module"""
    s = n_out / n_in
    w = 4.0 / s if s < 1 else 4.0
    taps = math.ceil(w) + 2

    def h(x):
        x = abs(x)
        if x <= 1:
            return 1.5 * x ** 3 - 2.5 * x ** 2 + 1.0
        if x < 2:
            return -0.5 * x ** 3 + 2.5 * x ** 2 - 4.0 * x + 2.0
        return 0.0

    M = np.zeros((n_out, n_in))
    for i in range(n_out):
        u = (i + 0.5) / s - 0.5
        j0 = math.floor(u - w / 2) + 1
        ws = [s * h(s * (u - j)) if s < 1 else h(u - j) for j in range(j0, j0 + taps)]
        tot = sum(ws)
        for j, v in zip(range(j0, j0 + taps), ws):
            if j < 0:
                j = -j - 1
            elif j >= n_in:
                j = 2 * n_in - 1 - j
            M[i, j] += v / tot
    return M


@pytest.mark.parametrize("R,N", SIZES + [(32, 1), (15, 3)])
def test_resize_matrix_against_a_direct_loop(R, N):
    # two float64 evaluations of the cubic (Horner there, powers here; terms up to 8 before they cancel) and of the
    # normalising sum differ by a few units of 2^-53 * 8: 1e-13 is two orders above that and twelve below a wrong tap
    D, U = lowpass.lowpass_matrices(R, N)
    np.testing.assert_allclose(D, _direct(R, R // N), rtol=0, atol=1e-13)
    np.testing.assert_allclose(U, _direct(R // N, R), rtol=0, atol=1e-13)


@pytest.mark.parametrize("R,N", SIZES)
def test_the_four_properties(R, N):
    D, U = lowpass.lowpass_matrices(R, N)
    r = R // N
    assert np.abs(D.sum(1) - 1).max() < 1e-15 and np.abs(U.sum(1) - 1).max() < 1e-15
    assert np.linalg.matrix_rank(U @ D) == r
    assert np.abs(U @ D).sum(1).max() <= 1.25
    # interior rows of D are torch's antialiased bicubic: column j of D is the response to an impulse at j
    eye = torch.eye(R, dtype=torch.float64)[:, None, None, :]  # R images of 1 x R
    resp = F.interpolate(eye, size=(1, r), mode="bicubic", antialias=True, align_corners=False)[:, 0, 0, :].numpy().T  # [r, R]
    s, w = r / R, 4.0 * N
    inside = [i for i in range(r)
              if math.floor((i + 0.5) / s - 0.5 - w / 2) + 1 >= 0 and math.floor((i + 0.5) / s - 0.5 - w / 2) + 1 + 4 * N + 2 <= R]
    if inside:
        assert np.abs(D[inside] - resp[inside]).max() <= 1e-15
    # only the border rows differ: torch clips the window and renormalises, this filter mirrors. The figure is a property of
    # the two conventions, 0.08 to its one stated digit (0.0822 at (32, 4), where a row has the most weight per tap)
    border = [i for i in range(r) if i not in inside]
    diff = np.abs(D[border] - resp[border]).max()
    assert border and 0 < diff < 0.085, diff


def test_identity_and_refusals():
    for n in (4, 7, 32):
        assert np.array_equal(lowpass.resize_matrix(n, n), np.eye(n))
    for R, N in ((32, 0), (32, 3), (32, 16), (12, 4)):
        with pytest.raises(ValueError):
            lowpass.lowpass_matrices(R, N)


@pytest.mark.parametrize("R,N", SIZES + [(32, 1), (15, 3)])
def test_tap_packing_round_trips(R, N):
    for M, n_in, n_out in zip(lowpass.lowpass_matrices(R, N), (R, R // N), (R // N, R)):
        first, taps = lowpass.pack_taps(M)
        P = lowpass.tap_count(n_in, n_out)
        assert taps.shape == (n_out, P) and P == min(n_in, (4 * N + 2) if n_out < n_in else 6)
        assert first.min() >= 0 and (first + P).max() <= n_in
        assert np.array_equal(lowpass.unpack_taps(first, taps, n_in), M)


def test_coef_ilvr_rows():
    for st, eta in (("ddim", 0.1), ("ddpm", None)):
        sch = schedule.PixelSchedule(50, 40, sample_type=st, eta=eta)
        q = sch.coef_ilvr()
        assert q.dtype == np.float32 and q.shape == (40, 2) and len(sch.coef_decode()) == 40
        assert sch.seq_next[0] == -1 and tuple(q[0]) == (1.0, 0.0)
        nxt = np.asarray(sch.seq_next[1:])
        np.testing.assert_array_equal(q[1:, 0], np.sqrt(sch.acp[nxt]))
        np.testing.assert_array_equal(q[1:, 1], np.sqrt(np.float32(1) - sch.acp[nxt]))
        # the level a row arrives at is the level the next lower row starts from
        if st == "ddim":
            np.testing.assert_array_equal(q[1:, 0], sch.coef_decode()["sa"][:-1])


@pytest.mark.parametrize("B,C,R,N", ir.OP_CASES)
def test_fp32_emulation_stays_inside_the_bound(B, C, R, N):
    x = ir.op_input(B, C, R)
    ref, bound = ir.phi64(x, R, N), ir.phi_bound(x, R, N)
    err = np.abs(ir.emulate32(x, R, N).astype(np.float64) - ref)
    assert (err <= bound).all(), (err / bound).max()
    # and the bound is not loose beyond use: it stays below 2e-4 of the image's scale at the largest chain (272 taps)
    assert bound.max() <= 2e-4 * np.abs(x).max()
    const = np.full((1, 1, R, R), 3.0, dtype=np.float32)
    assert ir.ulps(ir.emulate32(const, R, N), const).max() <= 4
    if N == 1:
        assert np.array_equal(ir.emulate32(x, R, N), x)


def test_wrapper_refuses_bad_keys_before_any_engine(monkeypatch):
    from cycle_diffusion_amd.gan_wrapper import baselines, ddpm_ddim_wrapper

    def no_engine(*a, **k):
        raise AssertionError("the engine was created before the keys were checked")
    monkeypatch.setattr(ddpm_ddim_wrapper, "get_engine", no_engine)
    ok = dict(source_model_type="toy32", sample_type="ddim", custom_steps=50, es_steps=50, eta=0.1)
    for bad in (dict(ilvr_down_n=3), dict(ilvr_down_n=16), dict(ilvr_down_n=0), dict(ilvr_down_n=4.0),
                dict(ilvr_down_n=4, ilvr_range_t=-1), dict(ilvr_down_n=4, sdedit_strengths=[0.5]),
                dict(ilvr_down_n=4, skip_steps=[0])):
        with pytest.raises(ValueError):
            baselines.DDPMILVRWrapper(**ok, **bad)
    with pytest.raises(AssertionError, match="engine was created"):  # good keys get as far as the engine
        baselines.DDPMILVRWrapper(**ok, ilvr_down_n=4, ilvr_range_t=5)
    assert baselines.SAMPLER_TYPES["DDPM_ILVR"] is baselines.DDPMILVRWrapper
    assert not hasattr(object.__new__(baselines.DDPMILVRWrapper), "translate")


def test_configs_parse():
    from cycle_diffusion_amd.utils.config_utils import get_config
    for name, n, rt in (("bench_afhq_c5_ilvr", 32, 20), ("toy_ddpm_c1_ilvr", 4, None)):
        keys = dict(list(get_config(os.path.join(ROOT, "config", "experiments", name + ".cfg")).gan))
        assert keys["gan_type"] == "DDPM_ILVR" and keys["ilvr_down_n"] == n and keys.get("ilvr_range_t") == rt
    twin = dict(list(get_config(os.path.join(ROOT, "config", "experiments", "bench_afhq_c5_sdedit.cfg")).gan))
    keys = dict(list(get_config(os.path.join(ROOT, "config", "experiments", "bench_afhq_c5_ilvr.cfg")).gan))
    for k in ("sample_type", "eta", "custom_steps", "es_steps", "refine_steps", "target_model_type", "target_model_path"):
        assert keys[k] == twin[k], k
