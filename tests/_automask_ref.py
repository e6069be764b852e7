"""Reference for the keep-mask estimate (cd_automask / cd_op_automask_reduce, csrc/automask.hip):

  * STREAM0       the Philox stream of the estimate's draw 0 (draw i is STREAM0 + i; element = the flat index in [B, C, H, W])
  * reference64   the definition in float64
  * emulate32     the same loops in numpy float32, in the kernels' order (draws ascending, channels ascending inside a draw,
                  the per-image sum as 1024-pixel blocks of four strided pixels per lane and a halving tree); `mutant` breaks it
                  in one of three known ways, so that the comparison can be shown to notice
  * compare       what the tests hold a result to, with the bounds below
  * make_case     the inputs of the case table

Bounds, u = 2^-24 (fp32 unit roundoff), first order in u. Every term |e_tgt - e_src| carries the one rounding of its
difference (relative u). A pixel's n C terms meet in n C - 1 additions that round (C - 1 inside a draw, n - 1 across draws and
the n that add a draw's sum, less the additions to an exact 0), each at most u relative to a partial sum of non-negative
terms, which never exceeds the total; the division by n C rounds once: |map32 - map64| <= (n C + 1) u map64, held here to
(n C + 2) u. The mean adds HW such maps (any order: at most HW - 1 additions of non-negative partial sums) and divides once:
(n C + HW + 2) u relative. v = min(map, cl) / cl with cl = ratio * mean takes the map's and the mean's relative errors, the
rounding of ratio, one product and one division; v is at most 1, so the relative (n C + HW + 8) u bounds it absolutely.
A pixel whose v lies that close to the threshold may fall on either side; it and, under dilation, every pixel whose window
holds it are left out of the 0 / 1 comparison. A pixel whose float64 map is exactly 0 is not: all its differences are 0, which
fp32 computes exactly, so v is exactly 0 on both sides whatever the mean."""
import numpy as np

STREAM0 = 0x6000
U = 2.0 ** -24
MAX_EXCLUDED = 0.01  # share of an image's pixels the band may leave out
SUM_BLOCK, SUM_LANES = 1024, 256

# (n, B, C, H, W): one image; the tiny network's shape; more than one block of the sum; odd C, HW no multiple of the block, H != W
SHAPES = ((1, 1, 4, 16, 16), (3, 2, 4, 16, 16), (10, 2, 4, 32, 32), (2, 3, 3, 8, 24))


def tol_map(n, C):
    return (n * C + 2) * U


def tol_mean(n, C, HW):
    return (n * C + HW + 2) * U


def tol_v(n, C, HW):
    return (n * C + HW + 8) * U


def make_case(seed, n, B, C, H, W, equal_sample=None):
    """e_src ~ N(0, 1); e_tgt = 0.9 e_src + 0.1 N(0, 1) + 0.5 bump N(0, 1), bump a rectangle per sample (rows H/4 .. H/4 + H/3
    + b, columns W/5 .. W/5 + W/2); `equal_sample`: that sample's two predictions are equal (its map and mean are 0)"""
    rng = np.random.default_rng(seed)
    e_src = rng.standard_normal((n, B, C, H, W))
    bump = np.zeros((1, B, 1, H, W))
    for b in range(B):
        bump[0, b, 0, H // 4:H // 4 + H // 3 + b, W // 5:W // 5 + W // 2] = 1.0
    e_tgt = 0.9 * e_src + 0.1 * rng.standard_normal(e_src.shape) + 0.5 * bump * rng.standard_normal(e_src.shape)
    e_src, e_tgt = e_src.astype(np.float32), e_tgt.astype(np.float32)
    if equal_sample is not None:
        e_tgt[:, equal_sample] = e_src[:, equal_sample]
    return e_src, e_tgt


def dilate(edit, d, short=False):
    """max of edit [B, H, W] over |dy|, |dx| <= d inside the image; short: the window misses its last column and row"""
    B, H, W = edit.shape
    out = np.zeros_like(edit)
    hi = d - 1 if short else d
    for dy in range(-d, hi + 1):
        for dx in range(-d, hi + 1):
            ys, yd = slice(max(0, dy), H + min(0, dy)), slice(max(0, -dy), H + min(0, -dy))
            xs, xd = slice(max(0, dx), W + min(0, dx)), slice(max(0, -dx), W + min(0, -dx))
            out[:, yd, xd] |= edit[:, ys, xs]
    return out


def reference64(e_src, e_tgt, ratio, thr, d):
    es, et = np.asarray(e_src, np.float64), np.asarray(e_tgt, np.float64)
    n, B, C, H, W = es.shape
    mp = np.abs(et - es).sum(axis=(0, 2)) / (n * C)  # [B, H, W]
    mean = mp.reshape(B, -1).sum(1) / (H * W)
    cl = ratio * mean
    safe = np.where(cl == 0, 1.0, cl)[:, None, None]
    v = np.where(cl[:, None, None] == 0, 0.0, np.minimum(mp, cl[:, None, None]) / safe)
    edit = v > thr
    return {"map": mp, "mean": mean, "v": v, "edit": edit, "keep": 1.0 - dilate(edit, d).astype(np.float64)}


def _sum32(x):
    """one image's pixels [HW] fp32 in the order of k_automask_sum / k_automask_finish"""
    f = np.float32
    nblk = -(-x.size // SUM_BLOCK)
    pad = np.zeros(nblk * SUM_BLOCK, f)
    pad[:x.size] = x
    total = f(0)
    for blk in pad.reshape(nblk, SUM_BLOCK // SUM_LANES, SUM_LANES):
        lane = np.zeros(SUM_LANES, f)
        for j in range(blk.shape[0]):
            lane = (lane + blk[j]).astype(f)
        w = SUM_LANES // 2
        while w > 0:
            lane[:w] = (lane[:w] + lane[w:2 * w]).astype(f)
            w //= 2
        total = f(total + lane[0])
    return total


def emulate32(e_src, e_tgt, ratio, thr, d, chunks=None, mutant=None):
    """mutant: None | "batch_mean" | "ge" | "short_window"; chunks: draws per accumulate launch (default: all at once)"""
    f = np.float32
    es, et = np.asarray(e_src, f), np.asarray(e_tgt, f)
    n, B, C, H, W = es.shape
    acc = np.zeros((B, H, W), f)
    chunks = [n] if chunks is None else list(chunks)
    assert sum(chunks) == n
    i0 = 0
    for nc in chunks:
        a = acc.copy()  # what lies in memory between two launches
        for i in range(i0, i0 + nc):
            s = np.zeros((B, H, W), f)
            for c in range(C):
                s = (s + np.abs((et[i, :, c] - es[i, :, c]).astype(f))).astype(f)
            a = (a + s).astype(f)
        acc = a
        i0 += nc
    mp = (acc / f(n * C)).astype(f)
    mean = np.array([f(_sum32(mp[b].reshape(-1)) / f(H * W)) for b in range(B)], f)
    if mutant == "batch_mean":
        mean = np.full(B, f(mean.astype(np.float64).mean()), f)
    cl = (f(ratio) * mean).astype(f)
    v = np.zeros((B, H, W), f)
    for b in range(B):
        if cl[b] != 0:
            v[b] = (np.minimum(mp[b], cl[b]) / cl[b]).astype(f)
    edit = v >= f(thr) if mutant == "ge" else v > f(thr)
    keep = (1 - dilate(edit, d, short=mutant == "short_window")).astype(f)
    return {"map": mp, "mean": mean, "keep": keep}


def excluded(ref, n, C, thr, d):
    """pixels left out of the 0 / 1 comparison [B, H, W]; asserts on the float64 reference that they are few"""
    B, H, W = ref["v"].shape
    band = (np.abs(ref["v"] - thr) <= tol_v(n, C, H * W)) & (ref["map"] > 0)
    out = dilate(band, d)
    share = out.reshape(B, -1).mean(1)
    assert (share <= MAX_EXCLUDED).all(), "the band around the threshold leaves out %s of the images' pixels" % (share,)
    return out


def compare(got_map, got_mean, got_keep, ref, n, C, thr, d, label=None):
    """holds a result (arrays [B, H, W], [B], [B, H, W]) to the float64 reference; returns the figures it checked (and
    prints them under `label` before it asserts)"""
    B, H, W = ref["v"].shape
    out = excluded(ref, n, C, thr, d)  # first: a reference that excludes too much checks nothing
    gm, gk = np.asarray(got_map, np.float64).reshape(B, H, W), np.asarray(got_keep, np.float64).reshape(B, H, W)
    gmean = np.asarray(got_mean, np.float64).reshape(B)
    assert np.isin(gk, (0.0, 1.0)).all(), "keep holds something other than 0.0 and 1.0"
    err_map = float((np.abs(gm - ref["map"]) / np.where(ref["map"] == 0, 1.0, ref["map"])).max())
    err_mean = float((np.abs(gmean - ref["mean"]) / np.where(ref["mean"] == 0, 1.0, ref["mean"])).max())
    figures = {"map_rel": err_map, "mean_rel": err_mean, "excluded": int(out.sum()),
               "keep_mismatch": int(((gk != ref["keep"]) & ~out).sum())}
    if label:
        print("%s %s bounds map %.3e mean %.3e" % (label, figures, tol_map(n, C), tol_mean(n, C, H * W)))
    assert err_map <= tol_map(n, C), figures
    assert err_mean <= tol_mean(n, C, H * W), figures
    assert figures["keep_mismatch"] == 0, figures
    return figures
