"""The kernels of the fp32 execution path and of its split-fp16 mode, one by one, against float64 (cd_op_conv2d_prec,
cd_op_attention_prec, cd_op_rows_prec, cd_op_resample_prec: the engine's building blocks under a Ctx with f32 / x3 set).

Operands, references, emulations and tolerances come from tests/_f32_path_ref.py; tests/test_f32_path_host.py shows on the CPU
that every emulation is within half of its tolerance and every mutant (a tap shifted, the concat seam off by a K step, a ragged
key in or out, the row vector of the wrong image, hi.wl dropped, lo from the rounded value, GEGLU halves swapped, an
uncentred LayerNorm variance) at least 5 tolerances away. Every case writes err_over_tol to the parity report (f32op/...).

kernel                         cases
k_conv_f32<64,64>              test_conv[*-p1] but the two below; image 0 alone of test_conv_tile_switch
k_conv_f32<128,64>             test_conv[big_m8281_n200_3x3-p1, tile_switch_64x64_n256-p1]; the batch of test_conv_tile_switch
three-term split GEMM          test_conv[*-p2] (conv_split_fwd -> launch_conv_gemm with out_f32, resid_f32, stats), nvalid < 8 at
                               N = 3 / 6 / 70, element-wise residual at strides 73 / 97 / 7, test_split_conv_statistics,
                               test_split_conv_tile_configurations, test_split_conv_then_groupnorm_fold
k_pack_w3                      every p2 convolution; test_split_range_guard (|w| = 300)
k_nchw_to_nhwc_split           the one-source p2 convolutions (Cin = 3 -> 32 in geom_cin3_*), test_resample avgpool p2
k_split_rows_f32               test_rows[split_rows_*]; test_conv[concat32+64_pads-p2, split_rows_*-p2]
k_flash_f32<DB, split>         test_attention: DB 1 = d8 / d32, 2 = d40 / d64, 3 = d80, 4 = d128, 5 = d160, each at p1 and p2;
                               mode 0 (fwd_*) with the value bias
k_attention_f32                test_attention[wave_*, fwd_d164_t100]; test_attention_dispatch
k_layernorm_f32<split>         test_rows[layernorm_*-p1 / -p2]
k_geglu_f32<split>             test_rows[geglu_*-p1 / -p2]; test_raw_geglu_conv_then_geglu
k_avgpool2_f32 / _split, k_upsample2_f32   test_resample, test_resample_grid_stride_wrap

The activations of the conv epilogue (SiLU, GELU) are tested at precision 1 only: no network of the split mode uses them (its
SiLU lives in GroupNorm), and the general epilogue of conv_gemm.hip evaluates them in the 16-bit path's fast forms.
"""
import pytest
import torch

import _f32_path_ref as R
import _gemm_sweep as S
import _groupnorm_ref as GN
import _ops
from cycle_diffusion_amd import _ffi

pytestmark = pytest.mark.gpu

FMT = 1.0 if _ffi.load_library().cd_act_format() == 1 else 8.0


def _need_fp16(precision):
    if precision == 2 and FMT != 1.0:
        pytest.skip("the split mode needs the fp16 build")


def _check(report, name, got, ref, tol):
    got = got.double()
    err = (got - ref).abs()
    ratio = (err / tol).max().item()
    scale = ref.abs().max().item() + 1e-300
    report.add("f32op/" + name, max_abs=err.max().item(), rel_to_max=err.max().item() / scale, err_over_tol=ratio,
               finite=bool(torch.isfinite(got).all().item()))
    print("f32op/%s max|err| %.3e (%.3e of max|ref|), err / tol %.3f" % (name, err.max().item(), err.max().item() / scale, ratio))
    assert torch.isfinite(got).all(), name
    assert (err <= tol).all(), (name, ratio)


def _pairs(cases):
    return [(c["name"], p) for c in cases for p in c["prec"]]


def _ids(pairs):
    return ["%s-p%d" % np for np in pairs]


# ==================================================================================================== convolution
_CONV = _pairs(R.CONV_CASES)


def _run_conv(engine, o, p, **over):
    kw = R.conv_call_args(o, p)
    kw.update(over)
    x0 = kw.pop("x0", o["x0"])
    return _ops.conv2d_prec(engine, x0, o["w"], **kw)


@pytest.mark.parametrize("name,p", _CONV, ids=_ids(_CONV))
def test_conv(engine, report, name, p):
    """precision 1: conv_fwd -> k_conv_f32, both tiles, ragged M and N, nk = 2 .. 54, stride / asymmetric padding / folded
    upsample / padded Cin, the concat inside the kernel with padded strides, every epilogue piece alone and together.
    precision 2: the three-term split GEMM on the same geometry, N = 3 / 6 / 70 / 96, fp32 residual with strides that are no
    multiple of 4, the two-source form through split_rows, activations 2^-10 .. 2^10 against weights 2^-12 .. 2^6."""
    _need_fp16(p)
    o = R.conv_build(name)
    got = _run_conv(engine, o, p)
    if o["case"]["stats"] and p == 2:
        got = got[0]
    _check(report, "conv/%s_p%d" % (name, p), got, o["ref"], o["tol"][p])


def test_conv_tile_switch(engine):
    """The accumulation order of k_conv_f32 does not depend on M - at the one place where M changes the kernel: a 64 x 64 image
    with N = 256 alone is 128 big tiles (<64,64>), first in a batch of two it is 256 (<128,64>). Same bits."""
    o = R.conv_build("tile_switch_64x64_n256")
    both = _run_conv(engine, o, 1)
    alone = _run_conv(engine, o, 1, x0=o["x0"][:1].contiguous())
    assert torch.equal(alone[0], both[0])
    assert not torch.equal(both[0], both[1])


_STATS = [c["name"] for c in R.CONV_CASES if c["stats"]]


@pytest.mark.parametrize("name", _STATS)
def test_split_conv_statistics(engine, report, name):
    """The GroupNorm block statistics of an fp32 output (general epilogue, p.stats with p.out_f32) against float64 block sums of
    the returned tensor. Bound: an fp32 sum of 32 terms in any order is within 32 x 2^-24 of sum|v|; the squares add a rounding."""
    _need_fp16(2)
    o = R.conv_build(name)
    y, st = _run_conv(engine, o, 2)
    want = GN.block_stats(y)
    absum = GN.block_stats(y.abs())
    tol = torch.stack([2.0 ** -19 * absum[:, 0], 2.0 ** -18 * absum[:, 1]], 1) + 1e-30
    _check(report, "conv_stats/" + name, st, want, tol)


def test_split_conv_no_statistics(engine):
    """Hout * Wout % 32 != 0: the convolution writes no statistics (and the entry point says so); fp32 without the split mode: never"""
    _need_fp16(2)
    o = R.conv_build("split_n96_resid_pad1")
    with pytest.raises(_ffi.EngineError, match="no GroupNorm statistics"):
        _run_conv(engine, o, 2, want_stats=True)
    o = R.conv_build("split_stats_n96")
    with pytest.raises(_ffi.EngineError, match="no GroupNorm statistics"):
        _run_conv(engine, o, 1, want_stats=True)


@pytest.mark.parametrize("name", ["split_stats_n96", "split_stats_1x1"])
def test_split_conv_then_groupnorm_fold(engine, report, name):
    """conv (split mode, fp32 output + epilogue statistics) -> GroupNorm + SiLU through k_gn_fold_f32, as
    test_groupnorm_after_conv_epilogue does for 16 bits. Reference: float64 GroupNorm of the returned tensor."""
    _need_fp16(2)
    o = R.conv_build(name)
    y, st = _run_conv(engine, o, 2)
    gen = torch.Generator().manual_seed(7)
    N = o["case"]["N"]
    gamma, beta = 1.0 + 0.2 * torch.randn(N, generator=gen), 0.2 * torch.randn(N, generator=gen)
    ref = GN.ref64(y, gamma, beta, 1e-5, silu=True)
    terr = (GN.torch32(y, gamma, beta, 1e-5, silu=True).double() - ref).abs().max().item()
    got = _ops.groupnorm_ex(engine, y, gamma, beta, 1e-5, silu=True, stats0=st, precision=2)
    _check(report, "conv_then_groupnorm/" + name, got, ref, GN.tol32(ref, terr, split=True))
    # the fold consumed them: with the sums of squares of a tensor twice as wide the result moves by O(1)
    wide = st.clone()
    wide[:, 1] *= 4.0
    other = _ops.groupnorm_ex(engine, y, gamma, beta, 1e-5, silu=True, stats0=wide, precision=2)
    assert (other - got).abs().max() > 0.1


def test_split_conv_tile_configurations(engine, report):
    """tile = 0 and two forced configurations of the shipped table - a 16-wave tile and a split-K entry - read back with
    last_gemm_config. The 16-bit GEMMs accumulate k-ascending in every TILE configuration: the 16-wave tile gives the bits of
    tile 0, statistics included. A split factor is not a tile configuration: it sums its K ranges in range order (conv_gemm.hip
    header; measured here: y and statistics differ from tile 0 in the last bits), so its bits are those of the same split on any
    other tile, and it meets the same tolerance against float64. Split factors come only from the shipped table, per shape, so
    the split mode stays bit-reproducible (tests/test_gpu_f32_path.py)."""
    _need_fp16(2)
    o = R.conv_build("split_tiles_c64_n96")
    y0, st0 = _run_conv(engine, o, 2, tile=0)
    auto = _ops.last_gemm_config(engine)
    assert auto["split"] == 1, auto  # no table row for this shape: the tuner picks tiles only
    results = {}
    for cfg in R.SPLIT_TILE_CONFIGS:
        y, st = _run_conv(engine, o, 2, tile=S.tile_arg(cfg))
        ran = _ops.last_gemm_config(engine)
        assert (ran["tile"], ran["bk"], ran["split"]) == S.launched(cfg), (cfg, ran)
        _check(report, "conv_tiles/%s" % S.config_id(cfg), y, o["ref"], o["tol"][2])
        results[cfg] = (y, st)
        print(S.config_id(cfg), "equal to tile 0: y", torch.equal(y, y0), "statistics", torch.equal(st, st0))
    wave16, splitk = R.SPLIT_TILE_CONFIGS
    assert torch.equal(results[wave16][0], y0) and torch.equal(results[wave16][1], st0)
    y3, st3 = _run_conv(engine, o, 2, tile=S.tile_arg((S.ANCHOR_TILE, 0, splitk[2])))
    assert _ops.last_gemm_config(engine)["split"] == splitk[2]
    assert torch.equal(results[splitk][0], y3) and torch.equal(results[splitk][1], st3)


def test_split_range_guard(engine):
    """|x| = 5000 and |w| = 300 leave the fp16 range of the scaled pairs: the call (the pack) raises instead of saturating, through
    both uploads of the input; the next call on the engine is clean."""
    _need_fp16(2)
    o = R.conv_build("split_rows_one")
    x = o["x0"].clone()
    x[1, 7, 2, 3] = 5000.0
    for via in (False, True):
        with pytest.raises(_ffi.EngineError, match="fp16 range"):
            _run_conv(engine, o, 2, x0=x, via_split_rows=via, pad0=4 if via else 0)
        got = _run_conv(engine, o, 2)
        assert ((got.double() - o["ref"]).abs() <= o["tol"][2]).all()
    w = o["w"].clone()
    w[3, 5, 0, 0] = -300.0
    with pytest.raises(_ffi.EngineError, match="fp16 range"):
        _ops.pack_conv_prec(engine, w)
    got = _run_conv(engine, o, 2)
    assert ((got.double() - o["ref"]).abs() <= o["tol"][2]).all()
    # fp32 has no such limit
    big = _ops.conv2d_prec(engine, x, o["w"], 1, pad=0)
    assert torch.isfinite(big).all() and big.abs().max() > 100


# ==================================================================================================== attention
_ATTN = _pairs(R.ATTN_CASES)


@pytest.mark.parametrize("name,p", _ATTN, ids=_ids(_ATTN))
def test_attention(engine, report, name, p):
    """flash (mode 2): every DB in both output forms, D = 8 / 40 / 80 (no multiple of 32), Tq = 1 / 33 / 129 / 200, Tk = 1 / 3 /
    5 / 31 / 33 / 77, padded strides, q in log2 units, the maximum arriving in the last key tile, a score of +-60.
    mode 0: the networks' fused q | k entry with the value bias (flash at D <= 160, else one wave per query).
    mode 1: k_attention_f32 at D = 68 / 512, T = 64 / 100 / 256."""
    _need_fp16(p)
    o = R.attn_build(name)
    got = _ops.attention_prec(engine, o["q"], o["k"], o["v"], **R.attn_call_args(o, p))
    _check(report, "attn/%s_p%d" % (name, p), got, o["ref"], o["tol"][p])


def test_attention_dispatch(engine):
    """attention_f32_fwd takes the flash kernel at D = 160 and one wave per query at D = 164: equality with the forced modes"""
    o = R.attn_build("fwd_d160_t100")
    kw = R.attn_call_args(o, 1)
    kw["obias"] = None
    run = lambda mode, oo: _ops.attention_prec(engine, oo["q"], oo["k"], oo["v"], **dict(kw, mode=mode))
    fwd, wave, flash = run(0, o), run(1, o), run(2, o)
    assert torch.equal(fwd, flash) and not torch.equal(fwd, wave)
    o = R.attn_build("fwd_d164_t100")
    assert torch.equal(run(0, o), run(1, o))
    with pytest.raises(_ffi.EngineError, match="flash_f32"):
        run(2, o)


# ==================================================================================================== rows
_ROWS = _pairs(R.ROWS_CASES)


@pytest.mark.parametrize("name,p", _ROWS, ids=_ids(_ROWS))
def test_rows(engine, report, name, p):
    """k_layernorm_f32 (C = 4 .. 2048: one to eight vectors per lane, a ragged last one; 1, 5, 301 rows; padded ldx; offset 100 with
    spread 0.1), k_geglu_f32 (Nout = 32 / 96 / 1280, odd row counts), k_split_rows_f32 (one and two sources, padded strides,
    2^-10 .. 2^10), each in fp32 and split output"""
    _need_fp16(p)
    o = R.rows_build(name)
    got = _ops.rows_prec(engine, o["case"]["op"], o["x0"], **R.rows_call_args(o, p))
    _check(report, "rows/%s_p%d" % (name, p), got, o["ref"], o["tol"][p])


def test_rows_range_guard(engine):
    _need_fp16(2)
    o = R.rows_build("layernorm_c320_r5")
    kw = R.rows_call_args(o, 2)
    with pytest.raises(_ffi.EngineError, match="fp16 range"):
        _ops.rows_prec(engine, "layernorm", o["x0"], **dict(kw, gamma=o["gamma"] * 5000.0))
    got = _ops.rows_prec(engine, "layernorm", o["x0"], **kw)
    assert ((got - o["ref"]).abs() <= o["tol"][2]).all()
    big = _ops.rows_prec(engine, "layernorm", o["x0"], **dict(R.rows_call_args(o, 1), gamma=o["gamma"] * 5000.0))
    assert torch.isfinite(big).all() and big.abs().max() > 4094
    o = R.rows_build("split_rows_c32+64_pads")
    x1 = o["x1"].clone()
    x1[300, 63] = -5000.0
    with pytest.raises(_ffi.EngineError, match="fp16 range"):
        _ops.rows_prec(engine, "split_rows", o["x0"], **dict(R.rows_call_args(o, 2), x1=x1))
    got = _ops.rows_prec(engine, "split_rows", o["x0"], **R.rows_call_args(o, 2))
    assert ((got - o["ref"]).abs() <= o["tol"][2]).all()


@pytest.mark.parametrize("p", [1, 2])
def test_raw_geglu_conv_then_geglu(engine, report, p):
    """the feed-forward of the fp32 transformer blocks: a projection with weights packed geglu = 1 leaves its [32 value | 32 gate]
    column blocks raw, k_geglu_f32 follows - against x W^T -> chunk -> a * gelu(g) in float64"""
    _need_fp16(p)
    ch = R.geglu_chain_build()
    rows, Cin = ch["x"].shape
    x = ch["x"].reshape(rows, Cin, 1, 1)
    h = _ops.conv2d_prec(engine, x, ch["w"], p, pad=0, bias=ch["bias"], geglu=True)  # [rows, 2 Nout, 1, 1], packed order
    got = _ops.rows_prec(engine, "geglu", h.reshape(rows, -1), p)
    err = (ch["emu"].double() - ch["ref"]).abs().max().item()
    tol = R.tol_f32(ch["ref"], err, split=p == 2)
    if p == 2:  # the projection is a three-term product: its representational term, through |a| |gelu'| <= 1.13 |a| + |gelu(g)|
        absconv = ch["x"].double().abs() @ ch["w"].double().abs().T
        a, g = (ch["x"].double() @ ch["w"].double().T + ch["bias"].double()).chunk(2, 1)
        aa, ag = absconv.chunk(2, 1)
        gel = 0.5 * g * (1.0 + torch.erf(g / 2.0 ** 0.5))
        tol = tol + 2.0 ** -21 * (aa * gel.abs() + 1.13 * a.abs() * ag)
    _check(report, "geglu_chain_p%d" % p, got, ch["ref"], tol)


# ==================================================================================================== resample
@pytest.mark.parametrize("name", [c["name"] for c in R.RESAMPLE_CASES])
def test_resample(engine, report, name):
    """k_avgpool2_f32 within 2 ulp of float64, k_avgpool2_split within the pair bound of the float64 pool of its decoded input,
    k_upsample2_f32 bit-exact; C = 4 and 96 at 6 x 10"""
    x = R.resample_x(name)
    ref = R.avgpool_ref64(x)
    _check(report, "avgpool/%s_p1" % name, _ops.resample_prec(engine, "avgpool", x, 1), ref, 2.0 * R.ulp32(ref))
    up = _ops.resample_prec(engine, "upsample", x, 1)
    assert torch.equal(up, torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest"))
    report.add("f32op/upsample/%s" % name, max_abs=0.0, rel_to_max=0.0, err_over_tol=0.0, finite=True)
    if FMT == 1.0:
        ref = R.avgpool_ref64(R.decode(x))
        _check(report, "avgpool/%s_p2" % name, _ops.resample_prec(engine, "avgpool", x, 2), ref, R.pair_tol(ref))


@pytest.mark.parametrize("op,p", [("avgpool", 1), ("avgpool", 2), ("upsample", 1)])
def test_resample_grid_stride_wrap(engine, report, op, p):
    """more than 4096 x 256 vectors: the grid-stride loops take a second trip; the wrapped elements are held to the same bound"""
    _need_fp16(p)
    c = R.RESAMPLE_WRAP[op]
    x = R.resample_x(c["name"])
    nvec = c["B"] * (c["C"] // 4) * (c["H"] * c["W"] // 4 if op == "avgpool" else c["H"] * c["W"] * 4)
    assert nvec > 4096 * 256
    got = _ops.resample_prec(engine, op, x, p)
    if op == "upsample":
        assert torch.equal(got, torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest"))
        report.add("f32op/upsample/%s" % c["name"], max_abs=0.0, rel_to_max=0.0, err_over_tol=0.0, finite=True)
    elif p == 1:
        ref = R.avgpool_ref64(x)
        _check(report, "avgpool/%s_p1" % c["name"], got, ref, 2.0 * R.ulp32(ref))
    else:
        ref = R.avgpool_ref64(R.decode(x))
        _check(report, "avgpool/%s_p2" % c["name"], got, ref, R.pair_tol(ref))
