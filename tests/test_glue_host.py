"""CPU: the references and tolerances of tests/test_gpu_glue.py are honest (tests/_glue_ref.py).

  * the float64 references agree with torch's own operators (F.avg_pool2d, F.interpolate nearest, F.embedding, the first-index
    rule of argmax / argmin, F.linear, F.silu) and round16 with tests/_ops.py bf16_round;
  * for every case the GPU test runs, the fp32 emulation of the kernel's arithmetic lies within HALF of the tolerance the GPU
    test applies against float64 (and passes every exact check), in both storage formats;
  * every mutant - a subtly wrong kernel evaluated on the host - fails its case: at least 5 tolerances away at its worst
    element, or at least one mismatching word where the check is exact;
  * at most 1 % of the vectors of every VQ case are undecidable, by the reference alone.
"""
import pytest
import torch
import torch.nn.functional as F

import _glue_ref as R

FMTS = R.FMTS


def _passes(r, name):
    print("%s: emulation / tol %.3f, %d mismatching words" % (name, r["ratio"], r["mismatch"]))
    assert r["ratio"] <= 0.5 and r["mismatch"] == 0, (name, r)


def _fails(r, name):
    print("%s: %.1f tolerances, %d mismatching words" % (name, r["ratio"], r["mismatch"]))
    assert r["ratio"] >= 5.0 or r["mismatch"] > 0, (name, r)


# ------------------------------------------------------------------------------------------------------- references
def test_round16_and_step16():
    import _ops
    fmt = R.lib_fmt()
    x = torch.randn(4000, generator=R._gen("r16")) * torch.pow(2.0, torch.randint(-20, 15, (4000,), generator=R._gen("r16e")).float())
    assert torch.equal(R.round16(x, fmt).float(), _ops.bf16_round(x))  # in range: the suite's rounding
    big = torch.tensor([70000.0, -70000.0, 65519.9, 65520.0, 1e30, -1e30])
    assert R.round16(big, "fp16").float().tolist() == [65504.0, -65504.0, 65504.0, 65504.0, 65504.0, -65504.0]
    assert R.round16(big[:2], "bf16").float().tolist() == [70144.0, -70144.0]
    for fmt, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        v = torch.tensor([1.0, 1.5, 2.0, 0.75, 1000.0, 0.0, 1e-7, 3e-5, 6.2e-5])
        one = torch.tensor(1, dtype=torch.int16)
        w = R.to16(v, fmt)
        up = (R.from16(w + one, fmt).double() - R.from16(w, fmt).double())  # the next word up: the step at |v|
        assert torch.equal(R.step16(R.from16(w, fmt), fmt), up), fmt


def test_pool_and_upsample_references_match_torch():
    for name in ("pool_b2_6x10_c40", "pool_b2_7x5_c40"):
        x = R.from16(R.resample_build(name, "fp16")["x"], "fp16").double()
        ref, mabs = R.avgpool_ref64(x)
        want = F.avg_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        assert ref.shape == want.shape and (ref - want).abs().max() < 1e-15
        assert (mabs - F.avg_pool2d(x.abs().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)).abs().max() < 1e-15
    x = R.resample_build("up_b2_3x5_c40", "fp16")["x"]
    want = F.interpolate(R.from16(x, "fp16").permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(R.from16(R.upsample_ref(x), "fp16"), want)


def test_vec_linear_reference_matches_torch():
    for name in ("b2_k1024_n9_silu_both", "b3_k1280_n37_silu_in", "b2_k64_n5_nobias_silu_in", "b2_k36_n7_ldx38"):
        o = R.vec_build(name)
        c = o["case"]
        x = o["x"][:, :c["K"]].double()
        y = F.linear(F.silu(x) if c["silu_in"] else x, o["W"].double(), o["bias"].double() if o["bias"] is not None else None)
        y = F.silu(y) if c["silu_out"] else y
        assert (y - R.vec_ref64(o)[0]).abs().max() < 1e-13, name
        # torch's own fp32 linear is inside the bound too (blocked sums: closer than the kernel's order)
        y32 = F.linear(F.silu(x.float()) if c["silu_in"] else x.float(), o["W"], o["bias"])
        y32 = F.silu(y32) if c["silu_out"] else y32
        assert R._ratio(y32, R.vec_ref64(o)[0], R.vec_tol(o)) <= 0.5, name
    x = torch.linspace(-20, 20, 401)
    assert (R.silu32(x.double()) - F.silu(x.double())).abs().max() < 1e-15


def test_token_references_match_torch():
    o = R.tokens_build("embed_b2_l77_d24_v50", "fp16")
    c = o["case"]
    ids = o["ids"].long()
    assert ids.min() < 0 and ids.max() > c["vocab"]  # the documented clamp to [0, vocab) is exercised
    want = R.to16(F.embedding(ids.clamp(0, c["vocab"] - 1), o["tok"]) + o["pos"][None], "fp16")
    assert torch.equal(R.tokens_emulate(o, "fp16")[:-R.GUARD].view(want.shape), want)
    # the first-index rule of argmax / argmin, as the kernels document it
    o = R.tokens_build("eot_b3_l77_d40", "fp16")
    assert o["ids"].argmax(1).tolist() == [0, 76, 10] and (o["ids"][2] == o["ids"][2].max()).sum() == 2
    assert torch.tensor([[3.0, 1.0, 1.0, 3.0]]).argmin(1).item() == 1 and torch.tensor([[3, 1, 1, 3]]).argmax(1).item() == 0
    assert torch.topk(torch.tensor([[3.0, 1.0, 1.0, 3.0]]).double(), 2, largest=False)[0].tolist() == [[1.0, 1.0]]


def test_posterior_reference_matches_the_formula():
    o = R.post_build("zc4_ld12")
    c = o["case"]
    m = o["mom"].double().view(c["B"], c["HW"], c["ld"]).permute(0, 2, 1)
    lv = m[:, 4:8].clamp(-30.0, 20.0)
    assert (m[:, 4:8] < -30).any() and (m[:, 4:8] > 20).any()
    want = R.f32(c["scale"]) * (m[:, :4] + torch.exp(lv).sqrt() * o["noise"].double())
    ref = R.post_eval(o, torch.float64)[0]
    assert ((ref - want).abs() <= 1e-14 * want.abs() + 1e-300).all()


# ------------------------------------------------------------------------------------------------------- emulations
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(R.N2H))
def test_nchw_to_nhwc_emulation(name, fmt):
    o = R.n2h_build(name)
    for fused in (False, True):
        _passes(R.n2h_verify(o, R.n2h_emulate(o, fmt, fused=fused), fmt), "n2h/%s fused=%d" % (name, fused))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(R.H2N))
def test_nhwc_to_nchw_emulation(name, fmt):
    o = R.h2n_build(name, fmt)
    for fused in (False, True):
        _passes(R.h2n_verify(o, R.h2n_emulate(o, fmt, fused=fused), fmt), "h2n/%s fused=%d" % (name, fused))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(R.RESAMPLE))
def test_resample_emulation(name, fmt):
    o = R.resample_build(name, fmt)
    _passes(R.resample_verify(o, R.resample_emulate(o, fmt), fmt), "resample/" + name)


@pytest.mark.parametrize("name", list(R.COPY))
def test_copy_emulation(name):
    o = R.copy_build(name)
    _passes(R.copy_verify(o, R.copy_emulate(o)), "copy/" + name)


@pytest.mark.parametrize("name", list(R.VEC))
def test_vec_linear_emulation(name):
    o = R.vec_build(name)
    _passes(R.vec_verify(o, R.vec_emulate(o)), "vec_linear/" + name)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(R.TOKENS))
def test_tokens_emulation(name, fmt):
    o = R.tokens_build(name, fmt)
    _passes(R.tokens_verify(o, R.tokens_emulate(o, fmt), fmt), "tokens/" + name)


@pytest.mark.parametrize("name", list(R.POST))
def test_posterior_emulation(name):
    o = R.post_build(name)
    z = torch.cat([R.post_eval(o, torch.float32)[0].reshape(-1), torch.full((R.GUARD,), R.SENT32)])
    assert torch.isfinite(z).all()
    _passes(R.post_verify(o, z), "posterior/" + name)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(R.VQ))
def test_vq_emulation_and_cap(name, fmt):
    o = R.vq_build(name)
    und = o["undecidable"].float().mean().item()
    print("vq/%s: %.3f %% of %d vectors undecidable" % (name, 100 * und, o["zv"].shape[0]))
    assert und <= R.VQ_CAP, (name, und)
    assert o["must"].sum().item() == (R.N_TIED if o["case"]["ties"] else 0)
    _passes(R.vq_verify(o, R.vq_emulate(o, fmt), fmt), "vq/" + name)


# ------------------------------------------------------------------------------------------------------- mutants
@pytest.mark.parametrize("fmt", FMTS)
def test_layout_mutants_fail(fmt):
    for name in ("c3_pad32_hw35", "c3_pad32_hw35_affine"):
        o = R.n2h_build(name)
        _fails(R.n2h_verify(o, R.n2h_emulate(o, fmt, mutant="cpad_for_c"), fmt), "n2h/%s Cpad for C" % name)
        _fails(R.n2h_verify(o, R.n2h_emulate(o, fmt, mutant="pad_not_zeroed"), fmt), "n2h/%s padding not zeroed" % name)
    o = R.n2h_build("c3_pad32_hw35_dup")
    _fails(R.n2h_verify(o, R.n2h_emulate(o, fmt, mutant="dup_offset"), fmt), "n2h dup copy at B HW C")
    for name in ("h16_c80_ld96", "f32_c5_ld8_affine"):
        o = R.h2n_build(name, fmt)
        _fails(R.h2n_verify(o, R.h2n_emulate(o, fmt, mutant="ld_for_c"), fmt), "h2n/%s ld for C" % name)


@pytest.mark.parametrize("fmt", FMTS)
def test_resample_and_copy_mutants_fail(fmt):
    for name in ("pool_b2_6x10_c40", "pool_b2_7x5_c40", "pool_b2_6x10_c40_3e-5"):
        o = R.resample_build(name, fmt)
        for m in ("w_for_wo", "3_of_4_taps"):
            r = R.resample_verify(o, R.resample_emulate(o, fmt, mutant=m), fmt)
            _fails(r, "resample/%s %s" % (name, m))
            assert r["ratio"] >= 5.0  # by the tolerance, not by the guard
    o = R.resample_build("up_b2_3x5_c40", fmt)
    _fails(R.resample_verify(o, R.resample_emulate(o, fmt, mutant="w_for_wo"), fmt), "upsample W for Wo")
    o = R.copy_build("r77_c40_lds48_ldd64")
    _fails(R.copy_verify(o, R.copy_emulate(o, mutant="ldd_for_lds")), "copy ldd for lds")
    o = R.copy_build("dup_rows_n21_tail7_c40")
    _fails(R.copy_verify(o, R.copy_emulate(o, mutant="tail_from_row0")), "dup_rows tail from row 0")


def test_vec_linear_mutants_fail():
    def mutant(name, m):
        o = R.vec_build(name)
        y = torch.full((o["case"]["B"], o["case"]["ldy"]), R.SENT32, dtype=torch.float64)
        y[:, :o["case"]["N"]] = R.vec_ref64(o, mutant=m)[0]
        r = R.vec_verify(o, y)
        _fails(r, "vec_linear/%s %s" % (name, m))
        assert r["ratio"] >= 5.0

    mutant("b2_k1024_n9_silu_both", "no_segment_3")
    for name in ("b2_k1028_n6", "b3_k1280_n37_silu_in"):
        mutant(name, "no_second_trip")
    for name in ("b3_k4_n5", "b2_k32_n128_silu_out", "b3_k1280_n37_silu_in"):
        mutant(name, "no_bias")
    for name in ("b2_k32_n128_silu_out", "b3_k1280_n37_silu_in", "b2_k37_n6_silu_in"):
        mutant(name, "silu_wrong_side")


@pytest.mark.parametrize("fmt", FMTS)
def test_token_mutants_fail(fmt):
    for name in ("embed_b2_l77_d24_v50", "vit_b2_t49_d24"):
        o = R.tokens_build(name, fmt)
        _fails(R.tokens_verify(o, R.tokens_emulate(o, fmt, mutant="pos_by_bl"), fmt), "%s pos[b L + l]" % name)
    for name in ("eot_b3_l77_d40", "eot_b3_l77_d1280"):
        o = R.tokens_build(name, fmt)
        _fails(R.tokens_verify(o, R.tokens_emulate(o, fmt, mutant="last_maximum"), fmt), "%s last maximum" % name)


def test_posterior_mutants_fail():
    for name in ("zc3_ld6", "zc4_ld12"):
        o = R.post_build(name)
        for m in ("no_clamp", "exp_lv"):
            z = torch.cat([R.post_eval(o, torch.float64, mutant=m)[0].reshape(-1), torch.full((R.GUARD,), R.SENT32).double()])
            r = R.post_verify(o, z)
            _fails(r, "posterior/%s %s" % (name, m))
            assert r["ratio"] >= 5.0


@pytest.mark.parametrize("fmt", FMTS)
def test_vq_mutants_fail(fmt):
    o = R.vq_build("ties")
    _fails(R.vq_verify(o, R.vq_emulate(o, fmt, mutant="last_minimum"), fmt), "vq/ties last minimum (<=)")
    for name in ("e256_zc3", "e37_zc1_in_mul", "e1000_zc8", "ties"):
        o = R.vq_build(name)
        _fails(R.vq_verify(o, R.vq_emulate(o, fmt, mutant="no_e2"), fmt), "vq/%s without e^2" % name)
