"""The counter-based Gaussian generator of csrc/gauss.h restated in NumPy, for tests/test_philox_host.py (CPU) and
tests/test_gpu_philox.py (GPU). Nothing here runs on a GPU or reads anything but its arguments.

  * philox4x32_10   Philox4x32-10 (Salmon et al., SC'11) on uint64 arrays holding 32-bit words
  * uniforms        the two fp32 uniforms of an element, bit for bit what the kernel forms
  * normals         Box-Muller in float64 on those uniforms: what the kernel's fast intrinsics approximate
  * STREAMS         which Philox stream every draw of every sampler loop uses - the one written statement of the layout
                    (csrc/capi.hip sets the values; DESIGN.md section 3 mirrors this table)
  * statistics      moments, correlations and the Kolmogorov-Smirnov distance of three sequences, with their bounds

Element `idx` of (seed, stream) is one normal: the counter is (idx >> 1, idx >> 33, stream, 0x9E3779B9), the key the two
halves of the seed, and idx & 1 selects the cosine or the sine member of the counter's Box-Muller pair."""
import functools

import numpy as np

_U = np.uint64
_MASK = _U(0xFFFFFFFF)
_M0, _M1 = _U(0xD2511F53), _U(0xCD9E8D57)
_W0, _W1 = _U(0x9E3779B9), _U(0xBB67AE85)
_S32 = _U(32)
COUNTER_WORD3 = 0x9E3779B9


def _words(v):
    a = np.atleast_1d(np.asarray(v, dtype=np.uint64))
    assert (a <= _MASK).all()
    return a


def philox4x32_10(counter, key):
    """counter: four arrays of 32-bit words, key: two; returns the four output words (uint64 arrays, values < 2^32)"""
    c0, c1, c2, c3 = (_words(c) for c in counter)
    k0, k1 = (_words(k) for k in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2  # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def _raw(seed, stream, idx):
    idx = np.atleast_1d(np.asarray(idx, dtype=np.uint64))
    seed = int(seed)
    assert 0 <= seed < 1 << 64 and 0 <= int(stream) < 1 << 32
    one = np.ones_like(idx)
    ctr = ((idx >> _U(1)) & _MASK, (idx >> _U(33)) & _MASK, one * _U(int(stream)), one * _U(COUNTER_WORD3))
    return philox4x32_10(ctr, (_U(seed & 0xFFFFFFFF), _U(seed >> 32)))


def _u24(word):
    """((float)(c >> 8) + 0.5f) * 2^-24 in fp32. c >> 8 < 2^24 converts exactly; the sum is exact below 2^23 and rounds to
    even from there (numpy's fp32 add is IEEE round-to-nearest-even), so the top value 2^24 - 1 gives exactly 1.0."""
    x = (word >> _U(8)).astype(np.float32)
    return (x + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def uniforms(seed, stream, idx):
    """(u1, u2) fp32 of every element of idx; both members of a Box-Muller pair (idx, idx ^ 1) share them"""
    c0, c1, _c2, _c3 = _raw(seed, stream, idx)
    return _u24(c0), _u24(c1)


def normals(seed, stream, idx):
    """float64 Box-Muller of the fp32 uniforms; the angle is the fp32 product 6.2831855f * u2 widened"""
    idx = np.atleast_1d(np.asarray(idx, dtype=np.uint64))
    u1, u2 = uniforms(seed, stream, idx)
    rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    ang = (np.float32(6.28318530717958647692) * u2).astype(np.float64)
    return np.where((idx & _U(1)) == _U(1), rad * np.sin(ang), rad * np.cos(ang))


@functools.lru_cache(maxsize=8)
def normals_range(seed, stream, first, n):
    """normals() of the elements first .. first + n - 1, computed once per test session; the array is read-only"""
    out = np.empty(n, dtype=np.float64)
    step = 1 << 20
    for a in range(0, n, step):
        b = min(n, a + step)
        out[a:b] = normals(seed, stream, np.arange(first + a, first + b, dtype=np.uint64))
    out.setflags(write=False)
    return out


# the largest |z|: the smallest u1 is (0 + 0.5) * 2^-24 = 2^-25, so |z| <= sqrt(-2 ln 2^-25) = sqrt(50 ln 2)
MAX_ABS = float(np.sqrt(50.0 * np.log(2.0)))

# ------------------------------------------------------------------------------------------------------------ the streams
BAND = 0x1000       # streams to a band
MAX_STEPS = 0xFFF   # a loop that draws from the generator is refused beyond this many steps (csrc/capi.hip)
_LOOPS = {
    # loop: (stream of iteration 0, what the iteration number is)
    "encode_init": (0x0000, None),   # x_T of cd_dpm_encode / cd_cycle_translate
    "encode": (0x0001, "i"),         # DPM-Encoder step i (loop order): x_{t-1} ~ q(. | x_t, x_0)
    "decode": (0x1000, "i"),         # decode step i of the loop, whether or not earlier steps took an injected eps
    "refine_init": (0x2000, None),   # the re-noising ahead of cd_pix_refine's loop
    "refine": (0x2001, "i"),         # refinement step i
    "invert": (0x3000, "j"),         # cd_ddim_invert step j (eta = 0 rows: reserved, nothing is drawn)
    "mask": (0x4000, "slot"),        # keep-mask q-sample: slot 0 ahead of the first forward, slot i + 1 after decode step i
    "ilvr": (0x5000, "i"),           # ILVR's q-sample of the reference after decode step i
    "vae": (0x7a65, None),           # the VAE posterior sample (cd_vae_encode)
}


def STREAMS(loop, it=0):
    """the Philox stream of iteration `it` of `loop` (see _LOOPS); loops without an iteration take it = 0"""
    base, counted = _LOOPS[loop]
    it = int(it)
    if counted is None:
        assert it == 0, (loop, it)
        return base
    assert 0 <= it, (loop, it)
    return base + it


def band_streams(loop, steps):
    """every stream a `steps`-step run of `loop` can use"""
    _base, counted = _LOOPS[loop]
    if counted is None:
        return {STREAMS(loop)}
    n = steps + 1 if counted == "slot" else steps  # slots 0 .. steps
    return {STREAMS(loop, i) for i in range(n)}


# ------------------------------------------------------------------------------------------------------------ statistics
STAT_CASES = ((7, 0x1000), (7, 0x1001), (8, 0x1000))  # a sequence, its neighbour stream, its neighbour seed
STAT_N = 1 << 22
SIGMAS = 5.0
KS_BOUND = 2.0


def _ks(z):
    """sup |F_n - Phi| of a sample against N(0, 1)"""
    import torch
    s = torch.from_numpy(np.sort(z))
    cdf = (0.5 * (1.0 + torch.erf(s / np.sqrt(2.0)))).numpy()
    n = len(z)
    i = np.arange(1, n + 1, dtype=np.float64)
    return float(max((i / n - cdf).max(), (cdf - (i - 1) / n).max()))


def statistics(a, b, c):
    """a, b, c: the three sequences of STAT_CASES, float64. Returns {name: (value, null value, standard error)} of the moment
    and correlation statistics - raw moments and raw mean products, whose variances under N(0, 1) are 1, 2, 15, 96 and 1 -
    and {name: KS * sqrt(N)}."""
    out, ks = {}, {}
    for tag, z in (("a", a), ("b", b), ("c", c)):
        z = np.asarray(z, dtype=np.float64)
        n = len(z)
        z2 = z * z
        out["mean/" + tag] = (z.mean(), 0.0, np.sqrt(1.0 / n))
        out["variance/" + tag] = (z2.mean(), 1.0, np.sqrt(2.0 / n))
        out["third/" + tag] = ((z2 * z).mean(), 0.0, np.sqrt(15.0 / n))
        out["fourth_minus_3/" + tag] = ((z2 * z2).mean() - 3.0, 0.0, np.sqrt(96.0 / n))
        out["lag1/" + tag] = ((z[:-1] * z[1:]).mean(), 0.0, np.sqrt(1.0 / n))
        out["box_muller_pair/" + tag] = ((z[0::2] * z[1::2]).mean(), 0.0, np.sqrt(1.0 / (n / 2)))
        ks[tag] = _ks(z) * np.sqrt(n)
    n = len(a)
    out["cross_stream"] = ((np.asarray(a, np.float64) * b).mean(), 0.0, np.sqrt(1.0 / n))
    out["cross_seed"] = ((np.asarray(a, np.float64) * c).mean(), 0.0, np.sqrt(1.0 / n))
    return out, ks


def check_statistics(stats, ks, label):
    """print every figure, then hold each to SIGMAS standard errors of its null value and KS * sqrt(N) to KS_BOUND"""
    dev = {k: (v - null) / se for k, (v, null, se) in stats.items()}
    for k in sorted(dev):
        print("%s %-22s %+.4e  (%+.2f standard errors)" % (label, k, stats[k][0], dev[k]))
    for k in sorted(ks):
        print("%s KS*sqrt(N)/%s %.3f" % (label, k, ks[k]))
    bad = {k: round(d, 2) for k, d in dev.items() if not abs(d) <= SIGMAS}
    assert not bad, bad
    assert all(v <= KS_BOUND for v in ks.values()), ks
    return dev
