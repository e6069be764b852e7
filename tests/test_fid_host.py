"""CPU: the host half of the FID / KID evaluation (cycle_diffusion_amd/utils/fid.py) against closed forms and independent
restatements, and the synthetic Inception-v3 state_dict against the layer table (stated here on its own) through the torch
restatement of the network (tests/_inception_ref.py)."""
import numpy as np
import pytest
import torch
from PIL import Image

from cycle_diffusion_amd.utils import fid


def test_frechet_distance_identical_statistics_is_zero():
    rng = np.random.RandomState(0)
    f = rng.standard_normal((400, 32))
    mu, s = fid.statistics(f)
    d, imag = fid.frechet_distance(mu, s, mu, s)
    assert abs(d) < 1e-8 and imag < 1e-6


def test_frechet_distance_diagonal_closed_form():
    rng = np.random.RandomState(1)
    d = 64
    mu1, mu2 = rng.standard_normal(d), rng.standard_normal(d)
    v1, v2 = rng.uniform(0.1, 3.0, d), rng.uniform(0.1, 3.0, d)
    got, imag = fid.frechet_distance(mu1, np.diag(v1), mu2, np.diag(v2))
    want = ((mu1 - mu2) ** 2).sum() + (v1 + v2 - 2 * np.sqrt(v1 * v2)).sum()
    assert abs(got - want) <= 1e-9 * abs(want), (got, want)
    assert imag == 0.0 or imag < 1e-9


def test_frechet_distance_is_symmetric():
    rng = np.random.RandomState(2)
    f1, f2 = rng.standard_normal((300, 24)), rng.standard_normal((300, 24)) * 1.3 + 0.2
    a, _ = fid.frechet_distance(*fid.statistics(f1), *fid.statistics(f2))
    b, _ = fid.frechet_distance(*fid.statistics(f2), *fid.statistics(f1))
    assert abs(a - b) <= 1e-7 * abs(a), (a, b)


def test_frechet_distance_finite_on_rank_deficient_covariance():
    rng = np.random.RandomState(3)
    f1, f2 = rng.standard_normal((50, 2048)), rng.standard_normal((60, 2048)) + 0.1  # N < d: singular covariances
    d, imag = fid.frechet_distance(*fid.statistics(f1), *fid.statistics(f2))
    assert np.isfinite(d) and np.isfinite(imag)


def _kid_loop(f1, f2, num_subsets, max_subset_size, seed):
    """independent O(m^2) statement of the unbiased polynomial-kernel MMD^2 over the same seeded subsets"""
    rng = np.random.RandomState(seed)
    d = f1.shape[1]
    m = min(len(f1), len(f2), max_subset_size)
    k = lambda a, b: (float(np.dot(a, b)) / d + 1.0) ** 3
    tot = 0.0
    for _ in range(num_subsets):
        x = f2[rng.choice(len(f2), m, replace=False)]
        y = f1[rng.choice(len(f1), m, replace=False)]
        kxx = sum(k(x[i], x[j]) for i in range(m) for j in range(m) if i != j) / (m * (m - 1))
        kyy = sum(k(y[i], y[j]) for i in range(m) for j in range(m) if i != j) / (m * (m - 1))
        kxy = sum(k(x[i], y[j]) for i in range(m) for j in range(m)) / (m * m)
        tot += kxx + kyy - 2 * kxy
    return tot / num_subsets


def test_kernel_distance_matches_loop_and_is_seeded():
    rng = np.random.RandomState(4)
    f1, f2 = rng.standard_normal((30, 16)), rng.standard_normal((25, 16)) + 0.3
    got = fid.kernel_distance(f1, f2, num_subsets=5, max_subset_size=20, seed=7)
    want = _kid_loop(f1, f2, 5, 20, 7)
    assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (got, want)
    assert fid.kernel_distance(f1, f2, num_subsets=5, max_subset_size=20, seed=7) == got
    assert fid.kernel_distance(f1, f2, num_subsets=5, max_subset_size=20, seed=8) != got


def test_clean_resize_equals_per_channel_pil():
    rng = np.random.RandomState(5)
    img = rng.randint(0, 256, (64, 48, 3), dtype=np.uint8)
    got = fid.clean_resize(img)
    assert got.shape == (3, 299, 299) and got.dtype == np.float32
    assert got.min() >= 0 and got.max() <= 255
    for c in range(3):
        ch = Image.fromarray(img[:, :, c].astype(np.float32), mode="F").resize((299, 299), resample=Image.BICUBIC)
        np.testing.assert_array_equal(got[c], np.asarray(ch).clip(0, 255))


def test_quantise_matches_png_rounding():
    x = torch.tensor([0.0, 0.4999 / 255, 0.5 / 255, 0.5, 1.0, 1.2, -0.1]).view(1, 1, 7, 1).repeat(1, 3, 1, 1)
    q = fid.quantise(x)
    assert q.dtype == np.uint8 and q.shape == (1, 7, 1, 3)
    assert q[0, :, 0, 0].tolist() == [0, 0, 1, 128, 255, 255, 0]


def test_missing_weights_raise(monkeypatch):
    monkeypatch.delenv("CYCLEDIFF_FID_INCEPTION", raising=False)
    monkeypatch.setenv("CYCLEDIFF_SYNTHETIC_WEIGHTS", "0")
    with pytest.raises(FileNotFoundError):
        fid.load_inception(engine=None)


# the layer table of the FID Inception-v3 (torchvision Inception3 names): unit -> (in, out, kh, kw)
def _table():
    t = {"Conv2d_1a_3x3": (3, 32, 3, 3), "Conv2d_2a_3x3": (32, 32, 3, 3), "Conv2d_2b_3x3": (32, 64, 3, 3),
         "Conv2d_3b_1x1": (64, 80, 1, 1), "Conv2d_4a_3x3": (80, 192, 3, 3)}
    for n, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        t.update({n + ".branch1x1": (cin, 64, 1, 1), n + ".branch5x5_1": (cin, 48, 1, 1), n + ".branch5x5_2": (48, 64, 5, 5),
                  n + ".branch3x3dbl_1": (cin, 64, 1, 1), n + ".branch3x3dbl_2": (64, 96, 3, 3),
                  n + ".branch3x3dbl_3": (96, 96, 3, 3), n + ".branch_pool": (cin, pf, 1, 1)})
    t.update({"Mixed_6a.branch3x3": (288, 384, 3, 3), "Mixed_6a.branch3x3dbl_1": (288, 64, 1, 1),
              "Mixed_6a.branch3x3dbl_2": (64, 96, 3, 3), "Mixed_6a.branch3x3dbl_3": (96, 96, 3, 3)})
    for n, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        t.update({n + ".branch1x1": (768, 192, 1, 1), n + ".branch7x7_1": (768, c7, 1, 1), n + ".branch7x7_2": (c7, c7, 1, 7),
                  n + ".branch7x7_3": (c7, 192, 7, 1), n + ".branch7x7dbl_1": (768, c7, 1, 1),
                  n + ".branch7x7dbl_2": (c7, c7, 7, 1), n + ".branch7x7dbl_3": (c7, c7, 1, 7),
                  n + ".branch7x7dbl_4": (c7, c7, 7, 1), n + ".branch7x7dbl_5": (c7, 192, 1, 7),
                  n + ".branch_pool": (768, 192, 1, 1)})
    t.update({"Mixed_7a.branch3x3_1": (768, 192, 1, 1), "Mixed_7a.branch3x3_2": (192, 320, 3, 3),
              "Mixed_7a.branch7x7x3_1": (768, 192, 1, 1), "Mixed_7a.branch7x7x3_2": (192, 192, 1, 7),
              "Mixed_7a.branch7x7x3_3": (192, 192, 7, 1), "Mixed_7a.branch7x7x3_4": (192, 192, 3, 3)})
    for n, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        t.update({n + ".branch1x1": (cin, 320, 1, 1), n + ".branch3x3_1": (cin, 384, 1, 1),
                  n + ".branch3x3_2a": (384, 384, 1, 3), n + ".branch3x3_2b": (384, 384, 3, 1),
                  n + ".branch3x3dbl_1": (cin, 448, 1, 1), n + ".branch3x3dbl_2": (448, 384, 3, 3),
                  n + ".branch3x3dbl_3a": (384, 384, 1, 3), n + ".branch3x3dbl_3b": (384, 384, 3, 1),
                  n + ".branch_pool": (cin, 192, 1, 1)})
    return t


def test_synthetic_state_dict_matches_layer_table():
    from cycle_diffusion_amd import inception_synthetic_state_dict
    sd = inception_synthetic_state_dict(0)
    want = {}
    for unit, (cin, cout, kh, kw) in _table().items():
        want[unit + ".conv.weight"] = (cout, cin, kh, kw)
        for k in ("weight", "bias", "running_mean", "running_var"):
            want[unit + ".bn." + k] = (cout,)
    assert len(_table()) == 94
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert all(bool((sd[k] > 0).all()) for k in sd if k.endswith("running_var"))
    sd2 = inception_synthetic_state_dict(0)
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)


def test_restatement_consumes_synthetic_state_dict():
    from cycle_diffusion_amd import inception_synthetic_state_dict
    from _inception_ref import inception_fid_forward
    sd = inception_synthetic_state_dict(1)
    x = torch.randn(2, 3, 299, 299, generator=torch.Generator().manual_seed(0)) * 0.5
    with torch.no_grad():
        pool3, outs = inception_fid_forward(sd, x, return_all=True)
    assert pool3.shape == (2, 2048) and torch.isfinite(pool3).all()
    from cycle_diffusion_amd.engine import INCEPTION_BLOCK_SHAPES
    assert [tuple(o.shape[1:]) for o in outs] == list(INCEPTION_BLOCK_SHAPES)
    # He-normal weights keep the activations at scale through the 94 ReLU layers (no 16-bit underflow)
    assert 1e-2 < float(pool3.abs().mean()) < 1e2
    with pytest.raises(KeyError):  # strict names
        inception_fid_forward({k: v for k, v in sd.items() if k != "Mixed_6c.branch7x7_2.bn.bias"}, x[:1])
