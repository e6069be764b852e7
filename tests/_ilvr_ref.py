"""ILVR references for tests/test_lowpass_host.py (CPU) and tests/test_gpu_ilvr.py (GPU).

  * phi64        phi_N(X) = U D X D^T U^T in float64 from cycle-diffusion_amd/utils/lowpass.py's dense matrices
  * phi_bound    the per-output error bound of an fp32 evaluation of phi_N, derived below
  * emulate32    phi_N in numpy fp32 in the kernels' order (csrc/ilvr.hip): fp32-rounded taps, products rounded, compensated
                 sums over the taps ascending; the image's row index first, then the column index, for D and then for U
  * ilvr_chain   the sampler restated in torch fp32 around any eps function, with phi_N applied in float64
  * the op cases both test modules walk

The bound. Every output is a four-fold sum  sum U[X,a] D[a,j] X[j,x] D[b,x] U[Y,b]. An fp32 evaluation in four passes rounds,
along the path of one term, each weight once (4), each product once (4) and adds P - 1 times per pass: at most
2 P_D + 2 P_U + 4 roundings, P_D / P_U the taps of a row of D / U. To first order (n u << 1) the error of an output is at most
    gamma * (|U| |D| |X| |D|^T |U|^T),   gamma = (chain + 4) * 2^-24,   chain = 2 P_D + 2 P_U,
whatever the order of the sums; the kernels' compensated sums stay far inside it (the host test measures how far)."""
import functools

import numpy as np
import torch

from cycle_diffusion_amd.utils import lowpass

U24 = 2.0 ** -24

# (B, C, R, N): several blocks and channels; R / N = 4 where every window mirrors; the real size; the identity
OP_CASES = [(3, 3, 32, 4), (1, 3, 32, 8), (2, 3, 64, 16), (2, 3, 256, 32), (1, 1, 32, 1)]


@functools.lru_cache(maxsize=None)
def matrices(R, N):
    return lowpass.lowpass_matrices(R, N)


def gamma(R, N):
    r = R // N
    return (2 * lowpass.tap_count(R, r) + 2 * lowpass.tap_count(r, R) + 4) * U24


def phi64(x, R, N):
    D, U = matrices(R, N)
    A = U @ D
    return A @ np.asarray(x, dtype=np.float64) @ A.T


def phi_bound(x, R, N):
    D, U = matrices(R, N)
    A = np.abs(U) @ np.abs(D)
    return gamma(R, N) * (A @ np.abs(np.asarray(x, dtype=np.float64)) @ A.T)


def _kahan_rows(w, first, src):
    """out[..., i, :] = sum_t w[i, t] * src[..., first[i] + t, :] in fp32, taps ascending, compensated"""
    n_out, P = w.shape
    acc = np.zeros(src.shape[:-2] + (n_out, src.shape[-1]), dtype=np.float32)
    cmp = np.zeros_like(acc)
    rows = np.asarray(first, dtype=np.int64)
    for t in range(P):
        v = w[:, t][:, None] * src[..., rows + t, :]
        yk = v - cmp
        s = acc + yk
        cmp = (s - acc) - yk
        acc = s
    return acc


def emulate32(x, R, N):
    r = R // N
    D, U = matrices(R, N)
    fd, td = lowpass.pack_taps(D)
    fu, tu = lowpass.pack_taps(U)
    td, tu = td.astype(np.float32), tu.astype(np.float32)
    d = np.asarray(x, dtype=np.float32)
    V = _kahan_rows(td, fd, d)                                      # [.., r, R]   rows of the image
    T = np.swapaxes(_kahan_rows(td, fd, np.swapaxes(V, -1, -2)), -1, -2)   # [.., r, r]   then its columns
    W = _kahan_rows(tu, fu, T)                                      # [.., R, r]
    out = np.swapaxes(_kahan_rows(tu, fu, np.swapaxes(W, -1, -2)), -1, -2)
    assert T.shape[-2:] == (r, r) and out.shape[-2:] == (R, R)
    return out


@functools.lru_cache(maxsize=None)
def op_input(B, C, R, seed=0):
    """offset 3, unit spread, an impulse of 40 in every corner of every image"""
    g = torch.Generator().manual_seed(1000 * R + 10 * B + C + seed)
    x = 3.0 + torch.randn(B, C, R, R, generator=g)
    for i in (0, R - 1):
        for j in (0, R - 1):
            x[:, :, i, j] = 40.0
    return x.numpy()


def ulps(got, want):
    """distance in units in the last place of fp32 at `want`"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ the sampler
def decode_step(kind, co, x, e, nz):
    """one decode step in the kernels' fp32 operation order (csrc/sched.hip k_decode_step_ddim<false> / k_decode_step_ddpm);
    co: a row of PixelSchedule.coef_decode(); kind 0 = 'ddim', 1 = 'ddpm'"""
    f = lambda k: torch.tensor(float(co[k]), dtype=torch.float32, device=x.device)
    if kind == 0:
        px0 = (x - f("r") * e) / f("sa")
        nn = f("sigma") * nz if float(co["sigma"]) != 0.0 else torch.zeros_like(x)
        return f("sap") * px0 + f("dirc") * e + nn
    mean = f("r") * (x - f("dirc") * e)
    return mean + f("t_mask") * f("sigma") * nz


def condition(xp, y, qa, qb, n, R, N):
    """x = x' + phi_N((qa*y + qb*n) - x'): y' and the difference in fp32 in the kernel's order, phi_N in float64, one rounding
    of phi_N, then the add in fp32. Returns (x, d) with d the fp32 difference phi_N was applied to."""
    dev = xp.device
    q = lambda v: torch.tensor(float(v), dtype=torch.float32, device=dev)
    d = (q(qa) * y + q(qb) * n) - xp
    D, U = matrices(R, N)
    A = torch.as_tensor(U @ D, dtype=torch.float64, device=dev)
    phi = A @ d.double() @ A.T
    return xp + phi.float(), d


def ilvr_chain(eps_fn, kind, xT, coef, qcoef, y, step_noise, ref_noise, N, range_t):
    """eps_fn(x, t) -> eps_hat [B, C, R, R]; step_noise / ref_noise [K, B, C, R, R], slot i = loop iteration i"""
    K, R = len(coef), xT.shape[-1]
    x = xT
    for i in range(K):
        k = K - 1 - i
        e = eps_fn(x, int(coef["t"][k]))[:, :x.shape[1]]
        x = decode_step(kind, coef[k], x, e, step_noise[i])
        if k > range_t:
            yy = y if y.shape[0] == x.shape[0] else y.repeat(x.shape[0] // y.shape[0], 1, 1, 1)
            x, _ = condition(x, yy, qcoef[k, 0], qcoef[k, 1], ref_noise[i], R, N)
    return x


def down_norm(v, R, N):
    """|| D v D^T || over a batch of images, float64"""
    D, _ = matrices(R, N)
    Dt = torch.as_tensor(D, dtype=torch.float64, device=v.device)
    return (Dt @ v.double() @ Dt.T).norm().item()
