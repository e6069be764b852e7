"""CPU: the NumPy restatement of the counter-based Gaussian generator (tests/_philox_ref.py) is a real Philox4x32-10 with a
sound Box-Muller on top, and the stream layout it states keeps every loop's draws apart. tests/test_gpu_philox.py then holds
the device code of csrc/gauss.h to this restatement."""
import numpy as np
import pytest

import _philox_ref as pr

# Random123's kat_vectors for philox4x32 with 10 rounds: counter, key, output
KNOWN_ANSWERS = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KNOWN_ANSWERS, ids=["zeros", "ones", "pi"])
def test_known_answers(ctr, key, want):
    got = pr.philox4x32_10(ctr, key)
    assert tuple(int(w[0]) for w in got) == want, [hex(int(w[0])) for w in got]


def test_known_answers_vectorised():
    """the three at once: the rounds act on arrays element by element"""
    ctr = [np.array([k[0][j] for k in KNOWN_ANSWERS], dtype=np.uint64) for j in range(4)]
    key = [np.array([k[1][j] for k in KNOWN_ANSWERS], dtype=np.uint64) for j in range(2)]
    got = pr.philox4x32_10(ctr, key)
    for j in range(4):
        assert [int(v) for v in got[j]] == [k[2][j] for k in KNOWN_ANSWERS]


def test_counter_layout_and_uniform_conversion():
    """element idx uses counter (idx >> 1, idx >> 33, stream, 0x9E3779B9) and key (seed low, seed high); the fp32 uniform is
    ((c >> 8) + 0.5) * 2^-24 with the add rounded to even from 2^23"""
    seed, stream = 0x9E3779B97F4A7C15, 0xFFFFFFFF
    for idx in (0, 1, 2, 3, (1 << 33) - 2, (1 << 33) + 5, (1 << 34) + 1):
        c = pr.philox4x32_10((idx >> 1 & 0xFFFFFFFF, idx >> 33, stream, pr.COUNTER_WORD3), (seed & 0xFFFFFFFF, seed >> 32))
        u1, u2 = pr.uniforms(seed, stream, [idx])
        for u, w in ((u1, c[0]), (u2, c[1])):
            x = int(w[0]) >> 8
            exact = (x + 0.5) / 2.0 ** 24
            assert u.dtype == np.float32
            if x < 1 << 23:
                assert float(u[0]) == exact
            else:  # x + 0.5 is a tie between x and x + 1: the even one
                assert float(u[0]) * 2.0 ** 24 == (x if x % 2 == 0 else x + 1)
    # the pair shares its uniforms, the members are the cosine and the sine of one angle
    z = pr.normals(seed, stream, np.array([10, 11], dtype=np.uint64))
    u1, u2 = pr.uniforms(seed, stream, [10])
    rad2 = -2.0 * np.log(float(u1[0]))
    assert abs(z[0] ** 2 + z[1] ** 2 - rad2) < 1e-12 * max(1.0, rad2)
    ang = float(np.float32(6.28318530717958647692) * u2[0])
    assert abs(z[0] - np.sqrt(rad2) * np.cos(ang)) < 1e-15 and abs(z[1] - np.sqrt(rad2) * np.sin(ang)) < 1e-15
    # the extreme words: u = 1.0 exactly (radius 0) and u = 2^-25 (the largest radius, MAX_ABS)
    top, bottom = pr._u24(np.array([0xFFFFFFFF, 0], dtype=np.uint64))
    assert float(top) == 1.0 and float(bottom) == 2.0 ** -25
    assert abs(np.sqrt(-2.0 * np.log(float(bottom))) - pr.MAX_ABS) < 1e-12 and abs(pr.MAX_ABS - 5.887) < 1e-3


def test_statistics_of_the_restatement():
    """N = 2^22 of (seed 7, stream 0x1000), its neighbour stream and its neighbour seed: the first four moments, the lag-1 and
    Box-Muller-pair correlations of each, the cross-stream and cross-seed correlations within 5 standard errors of their
    null values, KS * sqrt(N) <= 2.0 (the 0.1 % point of the Kolmogorov distribution is 1.95)."""
    seqs = [pr.normals_range(s, st, 0, pr.STAT_N) for s, st in pr.STAT_CASES]
    stats, ks = pr.statistics(*seqs)
    pr.check_statistics(stats, ks, "restatement")
    assert max(np.abs(z).max() for z in seqs) <= pr.MAX_ABS


def test_stream_bands_do_not_overlap():
    """no two loops of up to MAX_STEPS iterations share a stream, and one more step would: the limit the engine enforces
    (csrc/capi.hip check_stream_band) is the layout's own"""
    loops = sorted(pr._LOOPS)
    sets = {l: pr.band_streams(l, pr.MAX_STEPS) for l in loops}
    for i, a in enumerate(loops):
        assert all(0 <= s <= 0xFFFFFFFF for s in sets[a])
        for b in loops[i + 1:]:
            assert not (sets[a] & sets[b]), (a, b, sorted(sets[a] & sets[b])[:4])
    for steps in (1, 3, 50, 1000, pr.MAX_STEPS):  # shorter loops use subsets
        for l in loops:
            assert pr.band_streams(l, steps) <= sets[l]
    assert pr.band_streams("encode", pr.MAX_STEPS + 1) & sets["decode"] == {0x1000}
    assert pr.band_streams("refine", pr.MAX_STEPS + 1) & sets["invert"] == {0x3000}
    # the values csrc/capi.hip sets
    assert [pr.STREAMS("encode_init"), pr.STREAMS("encode", 0), pr.STREAMS("decode", 2), pr.STREAMS("refine_init"),
            pr.STREAMS("refine", 0), pr.STREAMS("invert", 1), pr.STREAMS("mask", 0), pr.STREAMS("ilvr", 3),
            pr.STREAMS("vae")] == [0, 1, 0x1002, 0x2000, 0x2001, 0x3001, 0x4000, 0x5003, 0x7a65]
