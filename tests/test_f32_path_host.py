"""CPU: the references and tolerances of tests/test_gpu_f32_ops.py are honest (tests/_f32_path_ref.py).

  * the float64 references agree with torch's own operators;
  * for every case the GPU tests run, the fp32 emulation of the kernel's arithmetic lies within HALF of the tolerance the GPU test
    applies against float64 - a case whose operands make fp32 itself miss the bound is found here, not on the GPU;
  * every mutant - a subtly wrong kernel evaluated on the host - is at least 5 tolerances away at its worst element: the GPU
    tests would fail on it;
  * the documented ranges of the split representation hold (kX3ActScale 16, kX3WgtScale 256).
"""
import math

import pytest
import torch
import torch.nn.functional as F

import _f32_path_ref as R
import _gemm_sweep as S


def _ratio(got, ref, tol):
    return ((got.double() - ref).abs() / tol).max().item()


# ------------------------------------------------------------------------------------------------------- references
def test_conv_reference_matches_torch():
    for name in ("m105_n70_3x3_k864", "concat32+64_pads", "geom_s2p1_3x3", "geom_s2asym_3x3", "geom_up_3x3", "geom_cin3_1x1",
                 "geom_s2asym_1x1"):
        o = R.conv_build(name)
        c = o["case"]
        x = o["x"].double()
        if c["up"]:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        if c["asym"]:
            y = F.conv2d(F.pad(x, (0, 1, 0, 1)), o["w"].double(), stride=c["stride"])
        else:
            y = F.conv2d(x, o["w"].double(), stride=c["stride"], padding=c["pad"])
        y = y * R.f32(c["alpha"])  # the kernel takes alpha as fp32
        if o["bias"] is not None:
            y = y + o["bias"].double()[None, :, None, None]
        if o["rowvec"] is not None:
            y = y + o["rowvec"].double()[:, :, None, None]
        if c["act"] == 1:
            y = F.silu(y)
        if o["resid"] is not None:
            y = y + o["resid"].double()
        assert (y - o["ref"]).abs().max() < 1e-11 * max(1.0, y.abs().max().item()), name


def test_attention_and_rows_references_match_torch():
    o = R.attn_build("flash_d40_tq200_tk77")
    c = o["case"]
    q, k, v = (R._heads(t.double(), c["H"]) for t in (o["q"], o["k"], o["v"]))
    want = F.scaled_dot_product_attention(q, k, v, scale=math.log(2.0)).permute(0, 2, 1, 3).reshape(o["ref"].shape)
    assert (want - o["ref"]).abs().max() < 1e-12
    o = R.rows_build("geglu_n96_r301")
    a, g = o["x"].double().reshape(301, -1, 2, 32).unbind(2)
    assert (a.reshape(301, -1) * F.gelu(g.reshape(301, -1)) - o["ref"]).abs().max() < 1e-13
    ch = R.geglu_chain_build()
    assert (F.gelu(ch["emu"].double()) - F.gelu(ch["ref"])).abs().max() < 1e-4  # same thing, fp32 against float64


def test_sequential_sum_is_what_sets_the_gemm_bound():
    """an fp32 F.conv2d sums in blocks and is closer to float64 than the kernel's documented sequential order: 4 x torch
    would fail a correct kernel, 4 x the order-faithful emulation does not depend on torch's blocking"""
    o = R.conv_build("split_n96_k2880")
    Af, Wf = o["A"].reshape(o["A"].shape[0], -1), o["Wm"].reshape(96, -1)
    ref = Af @ Wf.T
    seq = (R.seq_gemm32(Af, Wf).double() - ref).abs().max().item()
    blocked = ((Af.float() @ Wf.float().T).double() - ref).abs().max().item()
    print("K = 2880: sequential %.3e, torch blocked %.3e, ratio %.2f" % (seq, blocked, seq / blocked))
    assert seq > 1.5 * blocked


# ------------------------------------------------------------------------------------------------------- emulations
@pytest.mark.parametrize("name", [c["name"] for c in R.CONV_CASES])
def test_conv_emulation_within_half_the_tolerance(name):
    o = R.conv_build(name)
    for p in o["case"]["prec"]:
        r = _ratio(o["emu"][p], o["ref"], o["tol"][p])
        print("conv/%s p%d emulation / tol %.3f" % (name, p, r))
        assert torch.isfinite(o["emu"][p]).all() and r <= 0.5, (name, p, r)
    if 2 in o["case"]["prec"]:  # the pairs alone (exact arithmetic on the decoded operands) sit inside the representational term
        c = o["case"]
        a = R.decode(o["A"]).reshape(o["A"].shape[0], -1)
        w = R.decode(o["Wm"], R.WGT_SCALE).reshape(c["N"], -1)
        pairs = R.conv_epilogue(a @ w.T, o, torch.float64)
        assert ((pairs - o["ref"]).abs() <= 2.0 ** -21 * o["absconv"] + 1e-300).all(), name


@pytest.mark.parametrize("name", [c["name"] for c in R.ATTN_CASES])
def test_attention_emulation_within_half_the_tolerance(name):
    o = R.attn_build(name)
    for p in o["case"]["prec"]:
        r = _ratio(o["emu"], o["ref"], o["tol"][p])
        print("attn/%s p%d emulation / tol %.3f" % (name, p, r))
        assert torch.isfinite(o["emu"]).all() and r <= 0.5, (name, p, r)


@pytest.mark.parametrize("name", [c["name"] for c in R.ROWS_CASES])
def test_rows_emulation_within_half_the_tolerance(name):
    o = R.rows_build(name)
    for p in o["case"]["prec"]:
        r = _ratio(o["emu"], o["ref"], o["tol"][p])
        print("rows/%s p%d emulation / tol %.3f" % (name, p, r))
        assert r <= 0.5, (name, p, r)


def test_geglu_chain_and_pool_bounds():
    ch = R.geglu_chain_build()
    err = (ch["emu"].double() - ch["ref"]).abs().max().item()
    assert _ratio(ch["emu"], ch["ref"], R.tol_f32(ch["ref"], err)) <= 0.5
    # the average pool: fp32 in the kernel's order on positive operands is within 1.5 ulp of float64, inside the bound of 2
    x = R.resample_x("b2_c96_6x10")
    assert (x > 0).all()
    p32 = ((x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2] + x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2]) * 0.25)
    ref = R.avgpool_ref64(x)
    assert ((p32.double() - ref).abs() <= 1.5 * R.ulp32(ref)).all()
    # ... and the split pool: the decoded pairs of the fp32 sum of the decoded inputs
    d = R.decode(x)
    ref = R.avgpool_ref64(d)
    s32 = ((d[:, :, 0::2, 0::2].float() + d[:, :, 0::2, 1::2].float() + d[:, :, 1::2, 0::2].float() + d[:, :, 1::2, 1::2].float())
           * 0.25)
    assert ((R.decode(s32) - ref).abs() <= 0.5 * R.pair_tol(ref)).all()


# ------------------------------------------------------------------------------------------------------- mutants
def _mutant_ratio(mut, o, p):
    r = _ratio(mut, o["ref"], o["tol"][p])
    assert r >= 5.0, r
    return r


def test_conv_mutants_exceed_the_tolerance():
    o = R.conv_build("m105_n70_3x3_k864")
    print("tap shifted, fp32: %.1f tolerances" % _mutant_ratio(R.conv_mutant_tap_shift(o), o, 1))
    o = R.conv_build("concat32+64_pads")
    for p in (1, 2):
        print("tap shifted p%d: %.1f" % (p, _mutant_ratio(R.conv_mutant_tap_shift(o), o, p)))
        print("seam off by 16 channels p%d: %.1f" % (p, _mutant_ratio(R.conv_mutant_seam(o), o, p)))
        print("rowvec of the wrong image p%d: %.1f" % (p, _mutant_ratio(R.conv_mutant_rowvec(o), o, p)))
    o = R.conv_build("epi_rowvec_img")
    print("rowvec of the wrong image alone: %.1f" % _mutant_ratio(R.conv_mutant_rowvec(o), o, 2))


@pytest.mark.parametrize("name", ["split_n96_k2880", "split_n70_resid_pad3", "split_n3", "geom_up_3x3", "split_ranges"])
def test_split_mutants_exceed_the_tolerance(name):
    """hi . wl dropped; lo taken as fp16(16 x) - hi (= 0): both lose the low halves, 2^-11 relative per term"""
    o = R.conv_build(name)
    print(name, "hi.wl dropped: %.1f tolerances" % _mutant_ratio(R.conv_emulate_split(o, drop_hi_wl=True), o, 2))
    print(name, "lo from the rounded value: %.1f tolerances" % _mutant_ratio(R.conv_emulate_split(o, lo_from_rounded=True), o, 2))


@pytest.mark.parametrize("name", ["flash_d8_tq33_tk5", "flash_d40_tq200_tk77", "flash_d160_tq33_tk31", "flash_d64_tq33_tk33",
                                  "wave_d68_t100"])
def test_attention_mutants_exceed_the_tolerance(name):
    o = R.attn_build(name)
    c = o["case"]
    for kw in (dict(drop_last_key=True), dict(extra_zero_key=True)):
        mut = R.attn_ref64(o["q"], o["k"], o["v"], c["H"], o["scale"], c["q_log2"], o["obias"], **kw)
        for p in c["prec"]:
            print(name, kw, "p%d: %.1f tolerances" % (p, _mutant_ratio(mut, o, p)))


def test_rows_mutants_exceed_the_tolerance():
    o = R.rows_build("geglu_n96_r301")
    for blk in (0, 2):
        for p in (1, 2):
            print("GEGLU halves of block %d swapped p%d: %.1f" % (blk, p, _mutant_ratio(R.geglu_ref(o["x"], torch.float64, blk), o, p)))
    o = R.rows_build("layernorm_large_mean")
    mut = R.layernorm_uncentred32(o["x"], o["gamma"], o["beta"])
    for p in (1, 2):
        print("LayerNorm variance not centred p%d: %.1f" % (p, _mutant_ratio(mut, o, p)))


# ------------------------------------------------------------------------------------------------------- split ranges
def test_split_representation_ranges():
    g = torch.Generator().manual_seed(5)
    x = R._log_uniform(g, (200000,), -6, math.log2(4094.0))
    x = x[x.abs() < 4094.0]
    assert ((R.decode(x) - x.double()).abs() <= 2.0 ** -22 * x.abs().double()).all()
    assert torch.isfinite(R.decode(torch.tensor([4093.9, -4093.9]))).all()
    small = R._log_uniform(g, (200000,), -20, -6)
    assert ((R.decode(small) - small.double()).abs() <= 2.0 ** -28).all()
    w = R._log_uniform(g, (200000,), -10, math.log2(255.0))
    w = w[w.abs() < 255.0]
    assert ((R.decode(w, R.WGT_SCALE) - w.double()).abs() <= 2.0 ** -22 * w.abs().double()).all()
    # beyond the range the scaled value leaves fp16: the kernels raise instead of saturating
    assert 4096.0 * R.ACT_SCALE > 65504.0 and 256.0 * R.WGT_SCALE > 65504.0


def test_forced_tile_configurations_are_in_the_shipped_table():
    triples = S.table_triples()
    for cfg in R.SPLIT_TILE_CONFIGS:
        assert cfg in triples, cfg
    t = S.cfg_table()
    assert t[R.SPLIT_TILE_CONFIGS[0][0]]["WM"] * t[R.SPLIT_TILE_CONFIGS[0][0]]["WN"] == 16 and R.SPLIT_TILE_CONFIGS[1][2] > 1
