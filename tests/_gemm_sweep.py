"""Shared by the tile-table tests, the GEMM configuration sweep (test_gpu_gemm_configs.py) and its child process
(_gemm_env_child.py); not collected. Three parts, none of which touches the GPU:

* parsers of csrc/conv_gemm.hip (kCfgs, cfg_needs_bk64, bk32_alias, cfg_always_bk32, the launch_cfg<...> instantiations of
  dispatch<BK>) and of the shipped tile table;
* the list of configurations under test and the shape battery of each, derived from the tile's BM / BN / BK / ring depth;
* operands (seeded by the case name) and the float64 reference of a case.
"""
import math
import os
import re
import zlib

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "cycle-diffusion_amd", "tune_gfx950.txt")
SRC = os.path.join(ROOT, "cycle-diffusion_amd", "csrc", "conv_gemm.hip")
LIN_STREAM_TILE = 30
ANCHOR_TILE = 3  # pinned against torch by test_gpu_ops.py on its own

# the operator's bounds (test_conv2d, test_conv2d_16bit_epilogue)
REL_TOL, MEAN_TOL, STATS_TOL = 5e-3, 2e-3, 2e-3


# ---------------------------------------------------------------------------------------------- parsers
def _src():
    return open(SRC).read()


def cfg_table():
    """id -> dict(BM, BN, TN, WM, WN, stages, name) from kCfgs (the name carries the wave grid and the ring depth)"""
    src = _src()
    body = src[src.index("const CfgInfo kCfgs[] = {"):src.index("constexpr int kNumCfgs")]
    out = {}
    for m in re.finditer(r"\{(\d+), (\d+), (\d+), (\d+), \"([^\"]*)\"\}", body):
        cid, BM, BN, TN = (int(m.group(i)) for i in range(1, 5))
        n = re.match(r"(\d+)x(\d+) w(\d+)x(\d+) s(\d+)", m.group(5))
        assert n and int(n.group(1)) == BM and int(n.group(2)) == BN, m.group(0)
        out[cid] = dict(BM=BM, BN=BN, TN=TN, WM=int(n.group(3)), WN=int(n.group(4)), stages=int(n.group(5)), name=m.group(5))
    return out


def cfg_ids():
    """(id -> BN, ids that exist with 64-deep K steps only)"""
    return {k: v["BN"] for k, v in cfg_table().items()}, bk64_only()


def _ids_in(func):
    src = _src()
    return src[src.index(func):].split("\n", 1)[0]


def bk64_only():
    return {int(x) for x in re.findall(r"id == (\d+)", _ids_in("inline bool cfg_needs_bk64"))}


def always_bk32():
    return {int(x) for x in re.findall(r"id == (\d+)", _ids_in("inline bool cfg_always_bk32"))}


def bk32_alias():
    """ids whose BK = 32 request launches another id's instantiation: {id: id launched}"""
    return {int(a): int(b) for a, b in re.findall(r"id == (\d+) \? (\d+)", _ids_in("inline int bk32_alias"))}


def dispatch_instantiations():
    """{(id, bk): (BM, BN, BK, WM, WN, stages)} as written in dispatch<BK>"""
    src = _src()
    body = src[src.index("int dispatch(hipStream_t st"):src.index("thread_local const char* g_last_cfg")]
    out = {}
    inst = r"launch_cfg<(\d+), (\d+), (BK|\d+), (\d+), (\d+), (\d+)>"
    for m in re.finditer(r"case (\d+): return " + inst, body):  # one line, both depths (or one literal depth)
        cid, v = int(m.group(1)), m.groups()[1:]
        for bk in ((32, 64) if v[2] == "BK" else (int(v[2]),)):
            out[(cid, bk)] = (int(v[0]), int(v[1]), bk, int(v[3]), int(v[4]), int(v[5]))
    for m in re.finditer(r"case (\d+):\n\s*if constexpr \(BK == 64\) return " + inst + r"[^\n]*\n\s*else return " + inst, body):
        g = m.groups()
        cid = int(g[0])
        out[(cid, 64)] = (int(g[1]), int(g[2]), 64, int(g[4]), int(g[5]), int(g[6]))
        out[(cid, 32)] = (int(g[7]), int(g[8]), 32, int(g[10]), int(g[11]), int(g[12]))
    for m in re.finditer(r"if \(id == (\d+)\) return " + inst, body):  # the 320- / 256-wide family
        g = m.groups()
        out[(int(g[0]), int(g[3]))] = (int(g[1]), int(g[2]), int(g[3]), int(g[4]), int(g[5]), int(g[6]))
    m = re.search(r"else return " + inst + r"\(st, p\);\n\s*\} else \{", body)  # its last 64-deep member has no `if`
    last = [c for c in bk64_only() | {22} if (c, 64) not in out]
    assert m and len(last) == 1, last
    g = m.groups()
    out[(last[0], 64)] = (int(g[0]), int(g[1]), 64, int(g[3]), int(g[4]), int(g[5]))
    return out


def table_rows():
    rows = []
    for ln in open(TABLE):
        v = ln.split()
        assert len(v) == 15, ln
        rows.append([int(x) for x in v])
    return rows


def table_triples():
    """distinct (tile, bk32 flag, split) of the shipped table; split 0 and 1 both mean none; the streaming kernel aside"""
    out = set()
    for r in table_rows():
        val = r[14]
        tile, split, bk32 = val & 0xff, (val >> 8) & 0xff, (val >> 16) & 1
        if tile != LIN_STREAM_TILE:
            out.add((tile, bk32, max(split, 1)))
    return out


# ---------------------------------------------------------------------------------------------- configurations
def configs_under_test():
    """(tile, bk32 flag, split): every kCfgs id at its own depth, every id the launcher accepts with the BK = 32 flag, every
    triple of the shipped table"""
    ids = cfg_table()
    cfgs = {(t, 0, 1) for t in ids}
    cfgs |= {(t, 1, 1) for t in ids if t not in bk64_only() and t not in always_bk32()}
    cfgs |= table_triples()
    return sorted(cfgs)


def config_id(cfg):
    return "t%d_bk%s_s%d" % (cfg[0], "32" if cfg[1] else "own", cfg[2])


def tile_arg(cfg):
    tile, bk32, split = cfg
    return tile | ((split if split > 1 else 0) << 8) | (bk32 << 16)


def effective_bk(tile, bk32):
    return 32 if (bk32 or tile in always_bk32()) else 64


def launched(cfg, geglu=False):
    """what the launcher's read-back must report for this request: (tile id, bk, split)"""
    tile, bk32, split = cfg
    if geglu and cfg_table()[tile]["TN"] % 64:  # value and gate halves meet in one 64-column chunk of a wave tile
        tile = 2
    bk = effective_bk(tile, bk32)
    return (bk32_alias().get(tile, tile) if bk == 32 else tile, bk, split)


def geometry(cfg):
    """(BM, BN, BK, stages) of the instantiation this request launches"""
    tile, bk, _ = launched(cfg)
    BM, BN, BK, _, _, stages = dispatch_instantiations()[(tile, bk)]
    assert BK == bk
    return BM, BN, BK, stages


# ---------------------------------------------------------------------------------------------- the battery
def _case(name, B, C0, H, W, N, k, C1=0, stride=1, pad=None, asym=False, up=False, bias=True, rowvec=False, resid=False,
          act=0, geglu=False, out16=False, stats=False):
    return dict(name=name, B=B, C0=C0, C1=C1, H=H, W=W, N=N, k=k, stride=stride, pad=k // 2 if pad is None else pad,
                asym=asym, up=up, bias=bias, rowvec=rowvec, resid=resid, act=act, geglu=geglu, out16=out16, stats=stats)


def ragged_n(BN):
    return {320: 200, 256: 192}.get(BN, BN + 24)


def battery(cfg):
    """The shapes one configuration is run on. Images are 8 x 12 / 5 x 7 / 9 x 11 / 6 x 10 (never powers of two: the epilogue's
    row tables index by division); 8 x 12 = 96 rows per image, so B = 3 or 7 images give M = 2 BM + 32 odd."""
    BM, BN, BK, stages = geometry(cfg)
    split = cfg[2]
    tag = config_id(cfg)
    nr, nf = ragged_n(BN), BN
    b2 = 7 if BM == 256 else 3
    assert (96 * b2 - 2 * BM) % 64 == 32 and 35 < BM
    c = []
    # rows: fewer than one tile / two tiles and an odd number of 32-row blocks; columns: masked / exactly one tile
    c.append(_case("m_small_3x3", 1, 2 * BK, 5, 7, nr, 3))
    c.append(_case("m_2bm_odd_3x3", b2, 2 * BK, 8, 12, nf, 3, rowvec=True, resid=True))
    # K steps against the ring depth (prologue / drain): 1 x 1, C = nk * BK
    for nk in sorted({1, stages - 1, stages, stages + 1}):
        c.append(_case("nk%d_1x1" % nk, 2, nk * BK, 8, 12, nr, 1))
    c.append(_case("s2_pad1", 2, BK, 9, 11, nf, 3, stride=2))
    c.append(_case("s2_asym", 2, BK, 9, 11, nf, 3, stride=2, pad=0, asym=True))
    c.append(_case("up_3x3", 2, BK, 5, 6, nr, 3, up=True))
    c.append(_case("5x5_pad2", 2, BK, 6, 10, nf, 5))
    c.append(_case("concat_3x3", 1, 3 * BK, 8, 12, nr, 3, C1=BK))  # boundary inside the K range (BK = 32: not 64-aligned)
    c.append(_case("silu_1x1", 2, 2 * BK, 8, 12, nr, 1, act=1))
    c.append(_case("gelu_1x1", 2, 2 * BK, 5, 7, nf, 1, act=2))
    c.append(_case("geglu_1x1", 2, 2 * BK, 8, 12, 2 * BN + 64, 1, geglu=True))
    # the 16-bit epilogue: bias + time-embedding row + residual + GroupNorm statistics
    c.append(_case("e16_all_3x3", b2, 2 * BK, 8, 12, nr, 3, rowvec=True, resid=True, out16=True, stats=True))
    c.append(_case("e16_all_1x1", 1, 2 * BK, 8, 12, nf, 1, rowvec=True, resid=True, out16=True, stats=True))
    c.append(_case("e16_m_small", 1, BK, 5, 7, nr, 3, resid=True, out16=True))
    if split > 1:
        # deep K (9 * 4 = 36 steps, ranges that start mid-tap); more splits than K steps (empty ranges)
        c.append(_case("split_deep_3x3", b2, 4 * BK, 8, 12, nr, 3, rowvec=True, resid=True))
        c.append(_case("split_empty_1x1", 2, max(1, split // 2) * BK, 8, 12, nf, 1, resid=True))
        c.append(_case("split_e16_3x3", 1, 4 * BK, 8, 12, nf, 3, rowvec=True, resid=True, out16=True, stats=True))
    for x in c:
        x["name"] = "%s/%s" % (tag, x["name"])
    return c


# channel-major K order (child process with CYCLEDIFF_KORDER=2): one shape set for every tile, so the outputs are comparable
# across tiles; every channel count a multiple of 64 (tile 20), the BK = 32 variant has its own concat case
CHM_TILES = [(3, 0), (3, 1), (14, 0), (15, 0), (18, 0), (20, 0), (22, 0), (24, 0), (25, 0), (14, 1)]


def chm_battery():
    """(case, split, chm expected). The K order falls back to tap-major for more than 8 x 8 taps and for the folded upsample."""
    c = [
        (_case("chm/3x3_s1_10x10", 2, 128, 10, 10, 200, 3, rowvec=True, resid=True), 1, 1),
        (_case("chm/3x3_s1_5x7", 3, 64, 5, 7, 200, 3), 1, 1),
        (_case("chm/3x3_s2_pad1", 2, 128, 9, 11, 200, 3, stride=2), 1, 1),
        (_case("chm/3x3_s2_asym", 2, 128, 9, 11, 200, 3, stride=2, pad=0, asym=True), 1, 1),
        (_case("chm/3x3_valid_s1_9x11", 2, 64, 9, 11, 200, 3, pad=0), 1, 1),   # the Inception stem's forms: no padding at all,
        (_case("chm/3x3_valid_s2_11x9", 3, 64, 11, 9, 200, 3, stride=2, pad=0), 1, 1),  # odd sizes at stride 2 (last tap row in-image)
        (_case("chm/5x5_pad2_5x7", 2, 64, 5, 7, 200, 5), 1, 1),
        (_case("chm/5x5_pad2_10x10", 1, 64, 10, 10, 200, 5), 1, 1),
        (_case("chm/8x8_s8", 2, 64, 24, 16, 200, 8, stride=8, pad=0), 1, 1),
        (_case("chm/16x16_s16_tapmajor", 2, 64, 32, 48, 200, 16, stride=16, pad=0), 1, 0),
        (_case("chm/3x3_up_tapmajor", 2, 64, 5, 6, 200, 3, up=True), 1, 0),
        (_case("chm/concat_3x3", 1, 192, 10, 10, 200, 3, C1=64), 1, 1),
        (_case("chm/e16_3x3", 3, 128, 8, 12, 200, 3, rowvec=True, resid=True, out16=True, stats=True), 1, 1),
        (_case("chm/split2_3x3", 2, 128, 10, 10, 200, 3, resid=True), 2, 1),
        (_case("chm/split3_3x3", 2, 128, 10, 10, 200, 3, resid=True), 3, 1),
        (_case("chm/split3_concat_s2", 2, 192, 9, 11, 200, 3, C1=64, stride=2), 3, 1),
    ]
    return c


CHM_BK32_ONLY = (_case("chm/concat_3x3_c96_32", 1, 96, 10, 10, 200, 3, C1=32), 1, 1)  # boundary not 64-aligned

# the grouped tile walk (child process with CYCLEDIFF_TILE_GROUP=3 CYCLEDIFF_TILE_GROUP_MIN_N=64)
GROUP_TILES = [3, 14, 22]
GROUP_SIZE = 3


def group_battery(tile):
    """tiles_m in {1, 3, 4, 7} (fewer row tiles than a group, one full group, a group + a ragged last group twice over) x
    1, 2, 5 column tiles; rows and columns ragged against the tile"""
    t = cfg_table()[tile]
    out = []
    for tm in (1, 3, 4, 7):
        for tn in (1, 2, 5):
            M, N = tm * t["BM"] - 24, max(64, tn * t["BN"] - 8)  # (the child's threshold for the grouped walk is N >= 64)
            assert M % 4 == 0 and -(-M // t["BM"]) == tm and -(-N // t["BN"]) == tn
            out.append(_case("group/t%d_m%d_n%d" % (tile, tm, tn), 1, 64, M // 4, 4, N, 1, resid=True))
    return out


# ---------------------------------------------------------------------------------------------- operands and reference
def out_hw(c):
    Hin, Win = (2 * c["H"], 2 * c["W"]) if c["up"] else (c["H"], c["W"])
    k, s = c["k"], c["stride"]
    if c["asym"]:
        return (Hin + 1 - k) // s + 1, (Win + 1 - k) // s + 1
    return (Hin + 2 * c["pad"] - k) // s + 1, (Win + 2 * c["pad"] - k) // s + 1


def operands(c, r16):
    """Seeded by the case's name without its configuration prefix: the configurations that share a shape share operands."""
    g = torch.Generator().manual_seed(zlib.crc32(("%s %s" % (c["name"].split("/", 1)[1], sorted(
        (k, v) for k, v in c.items() if k != "name"))).encode()) % (2 ** 31))
    B, C0, C1, H, W, N, k = (c[x] for x in ("B", "C0", "C1", "H", "W", "N", "k"))
    Cin = C0 + C1
    o = dict(x0=r16(torch.randn(B, C0, H, W, generator=g)))
    o["x1"] = r16(torch.randn(B, C1, H, W, generator=g)) if C1 else None
    o["w"] = r16(torch.randn(N, Cin, k, k, generator=g) / math.sqrt(Cin * k * k))
    o["bias"] = torch.randn(N, generator=g) * 0.5 if c["bias"] else None
    Nout = N // 2 if c["geglu"] else N
    Ho, Wo = out_hw(c)
    o["rowvec"] = torch.randn(B, N, generator=g) if c["rowvec"] else None
    o["resid"] = r16(torch.randn(B, Nout, Ho, Wo, generator=g)) if c["resid"] else None
    return o


def reference(c, o, zero_tap=None, shift_x1=0):
    """float64 convolution of the (already 16-bit-rounded) operands + the epilogue in float64; returns (y, stats or None).
    zero_tap=(r, s) / shift_x1=n build the WRONG answers of a dropped filter tap / a second concat source read n columns
    off - what the bounds must reject (test_tune_table.py)."""
    d = lambda t: None if t is None else t.double()
    x0, x1, w = d(o["x0"]), d(o["x1"]), d(o["w"])
    if zero_tap is not None:
        w = w.clone()
        w[:, :, zero_tap[0], zero_tap[1]] = 0
    if x1 is not None and shift_x1:
        x1 = torch.roll(x1, shift_x1, dims=3)
    x = torch.cat([x0, x1], 1) if x1 is not None else x0
    if c["up"]:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    if c["asym"]:
        x = F.pad(x, (0, 1, 0, 1))
    y = F.conv2d(x, w, d(o["bias"]), stride=c["stride"], padding=0 if c["asym"] else c["pad"])
    if o["rowvec"] is not None:
        y = y + d(o["rowvec"])[:, :, None, None]
    if c["geglu"]:
        val, gate = y.chunk(2, dim=1)
        y = val * F.gelu(gate)
    elif c["act"] == 1:
        y = F.silu(y)
    elif c["act"] == 2:
        y = F.gelu(y)
    if o["resid"] is not None:
        y = y + d(o["resid"])
    st = None
    if c["stats"]:  # sums over 32-row blocks of the NHWC row order, of the values before their 16-bit rounding
        rows = y.permute(0, 2, 3, 1).reshape(-1, 32, y.shape[1])
        st = torch.stack([rows.sum(1), (rows * rows).sum(1)], 1)
    return y, st


def err_stats(got, ref):
    """as _ops.err_stats, against a float64 reference"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    d = (got - ref).abs()
    scale = ref.abs().max().item() + 1e-12
    return dict(max_abs=d.max().item(), rel_to_max=d.max().item() / scale,
                mean_rel=d.mean().item() / (ref.abs().mean().item() + 1e-12), finite=bool(torch.isfinite(got).all().item()),
                ref_max=scale)


def within_bounds(st):
    return st["finite"] and st["rel_to_max"] < REL_TOL and st["mean_rel"] < MEAN_TOL
