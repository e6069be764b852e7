"""ILVR's low-pass filter phi_N on the host, float64: phi_N(X) = U D X D^T U^T per channel image with
D = resize_matrix(R, R / N) and U = resize_matrix(R / N, R), the published antialiased cubic resize (Keys kernel, a = -0.5;
away from the border the weights of F.interpolate(mode="bicubic", antialias=True, align_corners=False)). At the border an
index outside the image is mirrored with the edge repeated (-1 -> 0, -2 -> 1, n -> n - 1) and its weight added to the
mirrored index. The engine builds the same taps itself (csrc/ilvr.hip build_lowpass_taps); this module is what the
tests and any host-side use compare against."""
import math

import numpy as np


def keys(x, a=-0.5):
    """the cubic convolution kernel h(x)"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    far = ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a
    return np.where(x <= 1.0, near, np.where(x < 2.0, far, 0.0))


def _geometry(n_in, n_out):
    s = n_out / n_in
    w = 4.0 / s if s < 1.0 else 4.0
    return s, w, int(math.ceil(w)) + 2


def tap_count(n_in, n_out):
    """taps stored per row: the window of the resize, or the whole input where the input is shorter than the window"""
    return min(_geometry(n_in, n_out)[2], n_in)


def resize_matrix(n_in, n_out):
    """[n_out, n_in] float64"""
    s, w, P = _geometry(n_in, n_out)
    M = np.zeros((n_out, n_in), dtype=np.float64)
    for i in range(n_out):
        u = (i + 0.5) / s - 0.5
        j = int(math.floor(u - w / 2.0)) + 1 + np.arange(P)
        wt = s * keys(s * (u - j)) if s < 1.0 else keys(u - j)
        wt = wt / wt.sum()
        jm = np.where(j < 0, -j - 1, np.where(j >= n_in, 2 * n_in - 1 - j, j))
        assert jm.min() >= 0 and jm.max() < n_in, "one reflection does not suffice: (%d, %d)" % (n_in, n_out)
        np.add.at(M[i], jm, wt)
    return M


def check_geometry(R, N):
    if N < 1 or R % N != 0 or R // N < 4:
        raise ValueError("ILVR's down_N must be >= 1, divide the resolution and leave at least 4 pixels: R = %d, N = %d" % (R, N))


def lowpass_matrices(R, N):
    """(D [R / N, R], U [R, R / N])"""
    check_geometry(R, N)
    return resize_matrix(R, R // N), resize_matrix(R // N, R)


def first_tap(n_in, n_out):
    """first stored column of every row: the window's first index, clamped so that the P stored taps lie inside the input"""
    s, w, _ = _geometry(n_in, n_out)
    P = tap_count(n_in, n_out)
    f = [int(math.floor((i + 0.5) / s - 0.5 - w / 2.0)) + 1 for i in range(n_out)]
    return np.clip(np.asarray(f, dtype=np.int64), 0, n_in - P).astype(np.int32)


def pack_taps(M):
    """dense [n_out, n_in] of resize_matrix -> (first int32 [n_out], taps float64 [n_out, P]); raises if a nonzero is left out"""
    n_out, n_in = M.shape
    first, P = first_tap(n_in, n_out), tap_count(n_in, n_out)
    taps = np.stack([M[i, first[i]:first[i] + P] for i in range(n_out)], 0)
    if not np.array_equal(unpack_taps(first, taps, n_in), M):
        raise ValueError("a nonzero of the matrix lies outside its row's tap window")
    return first, taps


def unpack_taps(first, taps, n_in):
    M = np.zeros((taps.shape[0], n_in), dtype=np.float64)
    for i in range(taps.shape[0]):
        M[i, first[i]:first[i] + taps.shape[1]] = taps[i]
    return M


def lowpass(x, R, N):
    """phi_N of [..., R, R] in float64"""
    D, U = lowpass_matrices(R, N)
    A = U @ D
    return A @ np.asarray(x, dtype=np.float64) @ A.T
