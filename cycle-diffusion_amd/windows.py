"""Fused windows (MultiDiffusion, Bar-Tal et al. 2023): the window grid of a latent canvas larger than the
network's S x S input. Host side only: the grid is a small int32 table that cd_cycle_translate takes as `win_host`."""
import numpy as np

MAX_WINDOWS = 64  # kMaxWindows of csrc/kernels.h


def window_offsets(L, S, stride):
    """top-left offsets of the windows of size S along an extent of L cells: every `stride` cells, and a last window clamped to
    the end - (16, 16, 8) -> [0], (24, 16, 8) -> [0, 8], (28, 16, 5) -> [0, 5, 10, 12]"""
    L, S, stride = int(L), int(S), int(stride)
    if S <= 0 or stride <= 0:
        raise ValueError("window size and stride must be positive, got S = %d, stride = %d" % (S, stride))
    if L < S:
        raise ValueError("an extent of %d cells is smaller than the %d-cell window" % (L, S))
    return list(range(0, L - S, stride)) + [L - S]


def window_grid(Hc, Wc, S, stride):
    """int32 [n, 2] of (y, x) pairs, row-major with y outer: the windows of a Hc x Wc canvas. A stride above S would leave
    cells uncovered and is refused, and so are more than MAX_WINDOWS windows."""
    if int(stride) > int(S):
        raise ValueError("a window stride of %d cells leaves gaps between windows of %d cells" % (stride, S))
    ys, xs = window_offsets(Hc, S, stride), window_offsets(Wc, S, stride)
    if len(ys) * len(xs) > MAX_WINDOWS:
        raise ValueError("a %d x %d canvas at stride %d takes %d windows, more than the %d one call runs"
                         % (Hc, Wc, stride, len(ys) * len(xs), MAX_WINDOWS))
    return np.asarray([(y, x) for y in ys for x in xs], dtype=np.int32).reshape(-1, 2)


def check_grid(win, Hc, Wc, S):
    """what cd_cycle_translate refuses of a window table, as a ValueError ahead of the call; returns the table as contiguous
    int32 [n, 2]"""
    win = np.ascontiguousarray(win, dtype=np.int32)
    if win.ndim != 2 or win.shape[1] != 2 or not 1 <= win.shape[0] <= MAX_WINDOWS:
        raise ValueError("windows must be [n, 2] (y, x) pairs with 1 <= n <= %d, got shape %s" % (MAX_WINDOWS, win.shape))
    if Hc < S or Wc < S:
        raise ValueError("a canvas of %d x %d is smaller than the network's %d x %d input" % (Hc, Wc, S, S))
    if (win < 0).any() or (win[:, 0] > Hc - S).any() or (win[:, 1] > Wc - S).any():
        raise ValueError("a window lies outside the %d x %d canvas" % (Hc, Wc))
    if len({(int(y), int(x)) for y, x in win}) != win.shape[0]:
        raise ValueError("two windows are equal")
    if (coverage(win, Hc, Wc, S) == 0).any():
        raise ValueError("a canvas cell is covered by no window")
    return win


def refuse(kw, who):
    """wrappers without the coupled text loop refuse the [gan] key of the fused windows by name (removed from `kw` either way)"""
    v = kw.pop("window_stride", None)
    if v is not None and int(v) != 0:
        raise ValueError("%s does not use window_stride: the fused windows run on the coupled translate loop of the latent "
                         "text wrappers (SDStochasticText / LatentDiffStochasticText); remove it from the [gan] section" % who)


def coverage(win, Hc, Wc, S):
    """int32 [Hc, Wc]: how many windows cover each cell"""
    n = np.zeros((Hc, Wc), dtype=np.int32)
    for y, x in np.asarray(win).reshape(-1, 2):
        n[y:y + S, x:x + S] += 1
    return n
