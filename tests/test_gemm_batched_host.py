"""CPU: the references and bounds of tests/test_gpu_gemm_batched.py and of the new test_softmax_rows cases are honest
(tests/_gemm_batched_ref.py).

  * for every case the GPU tests run, the host emulation of the kernel's roundings (fp32 accumulation of the 16-bit operands,
    alpha in fp32, P rounded to 16 bits, one output rounding) lies within HALF of the bound the GPU test applies against
    float64, in both storage formats, and leaves every sentinel, guard and must-be-zero word intact;
  * every mutant - a subtly wrong kernel evaluated through the same flat-index arithmetic - fails its case: a batch stride taken
    from the other operand, a batch stride on the shared V weight, Ktot for ldw, alpha dropped or applied twice, the bias indexed
    by row, the residual or the statistics without their batch offset, padding columns written, K cut to a multiple of 64, a
    softmax without its maximum;
  * the float64 references agree with torch's own operators.

One exception to "half", by arithmetic and not by choice of inputs: a bf16 word keeps 8 significant bits, so ONE rounding of the
exact result already costs mean_rel = 2^-9 / 1.5 = 1.4e-3 and rel_to_max up to 2^-8 = 3.9e-3 - 0.70 of the GEMM bounds (5e-3 /
2e-3), whatever the operands are. For the GEMM forms with 16-bit output in bf16 the emulation is therefore held to the full
bound AND to 1.05 x the error of the float64 result rounded once: it may add nothing of its own. Measured (err / bound):
fp16 0.088 (16-bit output), 1e-4 (fp32 output); bf16 0.70-0.71 = the single rounding, 5e-5 (fp32 output).

The materialised chain of the AttnBlock core, measured here (emulation against float64, o - vbias):
  fp16  rel_to_max 4.0-5.2e-4, mean_rel 3.4-3.7e-4   (bounds 4e-3 / 1.5e-3)
  bf16  rel_to_max 3.5-5.4e-3, mean_rel 2.8-3.0e-3   (bounds 3.2e-2 / 1.2e-2)
(v is rounded to 16 bits on its way through V^T and compared with the float64 v: a little above a chain fed a rounded v)
"""
import pytest
import torch
import torch.nn.functional as F

import _attn_forms_ref as AF
import _gemm_batched_ref as G
import _gemm_sweep as gs
import _glue_ref as R


def _show(name, r):
    print("%s: %s" % (name, {k: ("%.3e" % v if isinstance(v, float) else v) for k, v in r.items()}))


def _passes(name, r, limit=0.5):
    _show(name, r)
    assert r["finite"] and r["mismatch"] == 0 and r["err_over_tol"] <= limit, (name, r)


def _fails(name, r):
    _show(name, r)
    assert r["err_over_tol"] >= 2.0 or r["mismatch"] > 0, (name, r)


# ------------------------------------------------------------------------------------------------------- references
def test_gemm_reference_matches_torch():
    for name in ("vt/c192_t96_ld200", "s/c192_t96", "x/resid_stats"):
        o = G.gemm_build(name, "fp16")
        c = o["case"]
        y, st = G.gemm_ref64(o, "fp16")
        for z in range(c["nb"]):
            a = o["Af"][0 if c["form"] == "vt" else z].double()
            want = F.linear(a, o["Wf"][z].double()) * float(torch.tensor(c["alpha"], dtype=torch.float32))
            if o["bias"] is not None:
                want = want + o["bias"].double()
            if o["resid"] is not None:
                want = want + R.from16(o["resid"][z], "fp16").double()
            assert (y[z] - want).abs().max() < 1e-12, name
        if st is not None:
            rows = y.reshape(-1, 32, c["N"])
            assert torch.equal(st.reshape(-1, 2, c["N"]), torch.stack([rows.sum(1), (rows * rows).sum(1)], 1))
    o = G.core_build("core/wide_c192_t64", "fp16")
    ref, v = G.core_ref64(o)
    want = F.scaled_dot_product_attention(o["q"].double(), o["k"].double(), v)  # scale = C^-1/2
    assert (ref - want).abs().max() < 1e-12
    assert torch.equal(G.sm_ref64(G.sm_build("sm/r5_c96")["s"]), torch.softmax(G.sm_build("sm/r5_c96")["s"].double(), -1))


def test_case_tables_say_what_they_reach():
    c = G.GEMM
    assert c["vt/c320_t77"]["N"] % 8 and c["vt/c320_t77"]["out_ld"] > c["vt/c320_t77"]["N"]        # generic epilogue, padding
    assert c["vt/c192_t96_ld200"]["N"] % 8 == 0 and c["vt/c192_t96_ld200"]["ldw"] != c["vt/c192_t96_ld200"]["K"]
    assert c["s/c224_t64"]["K"] % 64 == 32 and c["o/t96_c192"]["K"] % 64 == 32
    assert c["o/t96_c192"]["ldw"] == 128 and c["o/t96_c192"]["out_ld"] == 200
    assert all(x["a_bs"] == 0 for x in G.GEMM_CASES if x["form"] == "vt")
    assert G.gemm_tiles(c["x/split2"]) == [3 | (2 << 8)] and G.gemm_tiles(c["vt/c512_t256"]) == [0, 3, 2, 1, 24, 5, 22]
    assert G.gemm_tiles(c["s/c192_t96"]) == [0, 3, 2, 1, 24]
    assert G.expected_launch(c["s/c224_t64"], 1) == (1, 32, 1) and G.expected_launch(c["s/c512_t256"], 24) == (24, 32, 1)
    assert G.expected_launch(c["x/split2"], 3 | (2 << 8)) == (3, 64, 2) and G.expected_launch(c["vt/c512_t256"], 22) == (22, 64, 1)
    assert G.anchor_tile(c["s/c512_t256"], 32, 1) == 3 | (1 << 16) and G.anchor_tile(c["x/split2"], 64, 2) == 3 | (2 << 8)
    for x in G.CORE_CASES:
        assert (x["branch"] == G.BRANCH_FLASH) == (x["C"] <= 160) and (x["branch"] == G.BRANCH_FLASH or x["T"] % 32 == 0)
    assert G.CORE_REFUSED["T"] % 32 and G.CORE_REFUSED["C"] > 160


# ------------------------------------------------------------------------------------------------------- emulations
@pytest.mark.parametrize("fmt", G.FMTS)
@pytest.mark.parametrize("name", list(G.GEMM))
def test_gemm_emulation_within_half_the_bound(name, fmt):
    o = G.gemm_build(name, fmt)
    out, st = G.gemm_emulate(o, fmt)
    r = G.gemm_verify(o, out, st, fmt)
    if fmt == "bf16" and not o["case"]["out_f32"]:  # the single rounding alone is 0.70 of the bound (module docstring)
        fl = G.single_rounding_floor(o, fmt)
        _passes(name + "/" + fmt, r, limit=1.0)
        assert r["mean_rel"] <= 1.05 * fl["mean_rel"] and r["rel_to_max"] <= 1.05 * fl["rel_to_max"], (r, fl)
        assert r.get("stats_rel", 0.0) <= 0.5 * gs.STATS_TOL
    else:
        _passes(name + "/" + fmt, r)


@pytest.mark.parametrize("fmt", G.FMTS)
@pytest.mark.parametrize("name", list(G.CORE))
def test_core_emulation_within_half_the_bound(name, fmt):
    o = G.core_build(name, fmt)
    out, vt = G.core_emulate(o, fmt)
    ro, rv = G.core_verify(o, out, vt, fmt)
    _passes(name + "/o/" + fmt, ro)
    _passes(name + "/vt/" + fmt, rv, limit=1.0 if fmt == "bf16" else 0.5)  # V^T: a 16-bit GEMM output, as above


@pytest.mark.parametrize("fmt", G.FMTS)
@pytest.mark.parametrize("name", list(G.SM))
def test_softmax_emulation_within_half_the_bound(name, fmt):
    o = G.sm_build(name)
    got = R.round16(G.sm_emulate_rows(o["s"]), fmt).float()
    _passes(name + "/" + fmt, G.sm_verify(o, got, fmt))
    if o["case"]["kind"] == "const":
        assert torch.equal(got, R.round16(torch.full_like(got, 1.0 / o["case"]["cols"]), fmt).float())


# ------------------------------------------------------------------------------------------------------- mutants
GEMM_MUTANTS = [
    ("o/t96_c192", "w_bs_for_a_bs"), ("x/resid_stats", "w_bs_for_a_bs"),
    ("vt/c320_t77", "vt_a_bs"), ("vt/c192_t96_ld200", "vt_a_bs"), ("vt/c512_t256", "vt_a_bs"),
    ("vt/c192_t96_ld200", "ktot_for_ldw"), ("o/t96_c192", "ktot_for_ldw"), ("s/c192_t96", "ktot_for_ldw"),
    ("s/c192_t96", "alpha_dropped"), ("s/c192_t96", "alpha_twice"), ("s/c512_t256", "alpha_twice"), ("x/split2", "alpha_dropped"),
    ("o/t96_c192", "bias_by_row"), ("o/t256_c512", "bias_by_row"),
    ("x/resid_stats", "resid_no_zb"), ("x/resid_stats", "stats_no_zb"),
    ("vt/c320_t77", "pad_written"), ("o/t96_c192", "pad_written"),
    ("s/c224_t64", "k_trunc64"), ("o/t96_c192", "k_trunc64"),
]


@pytest.mark.parametrize("fmt", G.FMTS)
@pytest.mark.parametrize("name,mutant", GEMM_MUTANTS)
def test_gemm_mutants_fail(name, mutant, fmt):
    o = G.gemm_build(name, fmt)
    out, st = G.gemm_emulate(o, fmt, mutant=mutant)
    _fails("%s/%s/%s" % (name, mutant, fmt), G.gemm_verify(o, out, st, fmt))


@pytest.mark.parametrize("fmt", G.FMTS)
@pytest.mark.parametrize("mutant", ["alpha_dropped", "alpha_twice", "v_batch0"])
def test_core_mutants_fail(mutant, fmt):
    for name in ("core/wide_c192_t96", "core/wide_c512_t256", "core/flash_c128_t100"):
        if mutant == "v_batch0" and G.CORE[name]["B"] == 1:
            continue
        o = G.core_build(name, fmt)
        out, vt = G.core_emulate(o, fmt, mutant=mutant)
        _fails("%s/%s/%s" % (name, mutant, fmt), G.core_verify(o, out, vt, fmt)[0])


@pytest.mark.parametrize("fmt", G.FMTS)
def test_softmax_without_max_fails_on_the_spike_rows(fmt):
    o = G.sm_build("sm/spike_r4_c300")
    got = R.round16(G.sm_emulate_rows(o["s"], mutant="no_max"), fmt).float()
    r = G.sm_verify(o, got, fmt)
    _show("sm/spike/no_max/" + fmt, r)
    assert not r["finite"] and r["err_over_tol"] == float("inf")
    # ... and the bounded-score cases would not have noticed
    o2 = G.sm_build("sm/r5_c96")
    assert G.sm_verify(o2, R.round16(G.sm_emulate_rows(o2["s"], mutant="no_max"), fmt).float(), fmt)["err_over_tol"] <= 0.5


def test_chain_figures_are_the_documented_ones():
    """the materialised chain's emulation error, printed beside its bounds (module docstring; the GPU test's docstring)"""
    for fmt in G.FMTS:
        f = G.fmt_factor(fmt)
        for name in G.CORE:
            o = G.core_build(name, fmt)
            ro, _ = G.core_verify(o, *G.core_emulate(o, fmt), fmt)
            print("%s %s rel_to_max %.2e (bound %.1e) mean_rel %.2e (bound %.1e)" % (fmt, name, ro["rel_to_max"], AF.REL * f,
                                                                                    ro["mean_rel"], AF.MEAN * f))
            assert ro["rel_to_max"] <= 0.5 * AF.REL * f and ro["mean_rel"] <= 0.5 * AF.MEAN * f
