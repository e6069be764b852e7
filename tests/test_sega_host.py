"""Host side of semantic guidance (cycle-diffusion_amd/semantic_guidance.py, tests/_sega_ref.py): the concept
table and its threshold against torch.quantile, the grammar and its refusals, and the torch restatement the GPU tests compare
against - that it is the plain coupled loop without concepts, that every concept set of the end-to-end tests moves the result
far beyond their bound, and how sensitive the thresholded sets are to the engine's own forward error, which is where the GPU
bounds of those sets come from."""
import math

import numpy as np
import pytest
import torch

import _attn_control_ref as acr
import _sega_ref as sr
import golden_util as gu
from cycle_diffusion_amd import semantic_guidance as sgm
from cycle_diffusion_amd.semantic_guidance import EditConcept, concept_table, parse_concepts

NS = [2, 3, 256, 300, 1024, 16384, 36864]
QS = [0.0, 0.5, 0.9, 0.95, 0.999, 1.0]


# ------------------------------------------------------------------------------------------------ 1. table and threshold
@pytest.mark.parametrize("N", NS)
def test_table_rank_and_threshold_against_torch_quantile(N):
    g = torch.Generator().manual_seed(N)
    u, c = torch.randn(2, N, generator=g), torch.randn(2, N, generator=g)
    p = torch.randn(1, 2, N, generator=g)
    for q in QS:
        tab = concept_table([EditConcept("x", scale=3.0, threshold=q, warmup=0.0)], K=10, N=N)
        lo, frac = int(tab["lo"][0]), float(tab["frac"][0])
        pos = q * (N - 1)
        assert lo == min(int(math.floor(pos)), N - 1) and 0.0 <= frac < 1.0
        assert frac == float(np.float32(pos - lo)), (N, q, lo, frac)
        assert (int(tab["warm"][0]), int(tab["cool"][0])) == (0, 10) and float(tab["scale"][0]) == 3.0
        _eps, _nu, tau, kept, mask, ties = sr.guidance_step(u, c, p, tab, 0, torch.zeros(2, N), 3.0, 0.3, 0.6)
        a = ((p[0] - u) * 3.0).abs()
        t32 = torch.quantile(a, q, dim=1)
        t64 = torch.quantile(a.double(), q, dim=1)
        r32 = ((tau[:, 0] - t32).abs() / t32.abs().clamp_min(1e-30)).max().item()
        r64 = ((tau[:, 0].double() - t64).abs() / t64.abs().clamp_min(1e-30)).max().item()
        print("N=%d q=%g rel to fp32 quantile %.2e, to float64 %.2e" % (N, q, r32, r64))
        assert r32 <= 1e-5 and r64 <= 1e-6, (N, q, r32, r64)
        assert torch.equal(mask.flatten(1).sum(1).to(torch.int32), kept.flatten())
        # the count rule, on distinct values (N random fp32 draws are not distinct at the larger N): a shuffled ramp
        ramp = ((torch.randperm(N, generator=g).float() + 1.0) * torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0))[None]
        _e, _n, _t, kept, _m, ties = sr.guidance_step(torch.zeros(1, N), torch.zeros(1, N), ramp[None], tab, 0,
                                                      torch.zeros(1, N), 3.0, 0.3, 0.6)
        assert not ties.any() and (kept == sr.kept_rule(N, lo, frac)).all(), (N, q, kept, lo, frac)
    # q = 0 keeps everything, q = 1 only the maximum
    assert sr.kept_rule(N, *sgm.quantile_rank(0.0, N)) == N and sr.kept_rule(N, *sgm.quantile_rank(1.0, N)) == 1


def test_threshold_with_ties():
    """values quantised to multiples of 1/8: runs of equal values straddle the threshold; tau is still the quantile and the
    kept count is what >= gives"""
    g = torch.Generator().manual_seed(5)
    for N in (256, 300, 1024):
        u = torch.zeros(1, N)
        p = (torch.randn(1, 1, N, generator=g) * 8).round() / 8
        for q in QS:
            tab = sgm.table_rows([(1.0, 1.0, q, 0, 1)], 1, N)
            _e, _n, tau, kept, _m, ties = sr.guidance_step(u, u, p, tab, 0, torch.zeros(1, N), 1.0, 0.0, 0.0)
            t64 = torch.quantile(p[0].abs().double(), q, dim=1)
            assert ties.all() and abs(tau.item() - t64.item()) <= 1e-6 * max(abs(t64.item()), 1e-30)
            assert kept.item() == int((p[0].abs() >= tau).sum())


# ------------------------------------------------------------------------------------------------ 2. grammar
def test_parse_concepts():
    assert parse_concepts("") == [] and parse_concepts(None) == [] and parse_concepts("   ") == []
    cs = parse_concepts("+glasses:5:0.9; -smile")
    assert cs == [EditConcept("glasses", 5.0, 0.9, False), EditConcept("smile", 5.0, 0.9, True)]
    cs = parse_concepts("a red hat:7.5 ;-  beard : 2 : 0.5")
    assert [(c.text, c.scale, c.threshold, c.reverse) for c in cs] == [("a red hat", 7.5, 0.9, False), ("beard", 2.0, 0.5, True)]
    tab = concept_table(cs, K=20, N=1024)
    assert list(tab["scale"]) == [7.5, -2.0] and list(tab["warm"]) == [2, 2] and list(tab["cool"]) == [20, 20]
    assert tab.dtype.itemsize == 24


@pytest.mark.parametrize("spec, match", [
    ("+a;;-b", "empty item"), ("+:5", "no text"), ("a:1:2:3", "more than"), ("a:x", "not a number"), ("a:5:1.5", "threshold"),
    ("a:-3", "negative"), ("a:inf", "finite"), (";".join("c%d" % i for i in range(9)), "1 to 8"),
])
def test_parse_refusals(spec, match):
    with pytest.raises(ValueError, match=match):
        parse_concepts(spec)


def test_table_refusals():
    ok = EditConcept("x")
    with pytest.raises(ValueError, match="1 to 8"):
        concept_table([], 10, 100)
    with pytest.raises(ValueError, match="1 to 8"):
        concept_table([ok] * 9, 10, 100)
    for kw, match in ((dict(threshold=-0.1), "threshold"), (dict(threshold=float("nan")), "finite"),
                      (dict(scale=float("inf")), "finite"), (dict(weight=float("nan")), "finite"),
                      (dict(warmup=0.5, cooldown=0.4), "warmup"), (dict(cooldown=1.5), "cooldown"), (dict(warmup=-0.1), "warmup"),
                      (dict(text=" "), "text")):
        with pytest.raises(ValueError, match=match):
            concept_table([EditConcept(**dict(dict(text="x"), **kw))], 10, 100)
    # the rows the engine would refuse: lo / frac come out in range by construction, warm / cool and the numbers are checked
    for row, match in (((1.0, 1.0, 0.5, 3, 2), "warm"), ((1.0, 1.0, 0.5, 0, 11), "warm"), ((1.0, 1.0, 0.5, -1, 2), "warm"),
                       ((float("nan"), 1.0, 0.5, 0, 2), "finite"), ((1.0, float("inf"), 0.5, 0, 2), "finite"),
                       ((1.0, 1.0, 1.01, 0, 2), "threshold")):
        with pytest.raises(ValueError, match=match):
            sgm.table_rows([row], 10, 100)
    for s_m, beta, match in ((float("nan"), 0.5, "edit_momentum_scale"), (0.3, float("inf"), "edit_momentum_beta"),
                             (0.3, 1.5, "edit_momentum_beta"), (0.3, -0.1, "edit_momentum_beta")):
        with pytest.raises(ValueError, match=match):
            sgm.check_concepts([ok], s_m, beta)
    tab = sgm.table_rows([(1.0, 1.0, 0.999, 0, 10)], 10, 36864)
    assert 0 <= tab["lo"][0] <= 36863 and 0.0 <= tab["frac"][0] < 1.0


def test_example_config_carries_the_keys():
    import os
    from cycle_diffusion_amd.utils.config_utils import get_config
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config")
    gan = dict(iter(get_config("experiments/bench_sd_c2_sega.cfg", config_root=root).gan))
    base = dict(iter(get_config("experiments/bench_sd_c2.cfg", config_root=root).gan))
    cs = parse_concepts(gan.pop("edit_concepts"))
    assert [(c.text, c.scale, c.threshold, c.reverse) for c in cs] == [("glasses", 5.0, 0.9, False), ("smile", 4.0, 0.8, True)]
    assert gan.pop("edit_momentum_scale") == 0.3 and gan.pop("edit_momentum_beta") == 0.6 and gan == base


def test_wrappers_without_the_coupled_loop_refuse_the_keys():
    kw = dict(edit_concepts="+glasses", other=1)
    with pytest.raises(ValueError, match="SDEdit does not use edit_concepts"):
        sgm.refuse(kw, "SDEdit")
    assert kw == dict(other=1)
    kw = dict(edit_concepts="", edit_momentum_beta=None)
    sgm.refuse(kw, "DDIB")  # the defaults of a config that leaves the feature off
    assert kw == {}


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.fixture(scope="module")
def tiny():
    fx = gu.load("latent_cycle_tiny")
    sd = gu.weights(fx)
    x0, c, uc, c2 = acr.e2e_inputs()
    e = sr.E2E
    noise = gu.latent_noise(e["noise_seed"], x0.shape, e["S"] - e["skip"])
    run = lambda name, **kw: sr.e2e_run(sd, x0, c, uc, c2, noise, name, **kw)
    base = run(None)
    sets = {name: run(name) for name in sr.SETS}  # computed once, shared, left unchanged
    return dict(sd=sd, x0=x0, c=c, uc=uc, c2=c2, noise=noise, run=run, base=base, sets=sets)


def test_restatement_without_concepts_is_the_coupled_loop(tiny):
    e = sr.E2E
    z, x = acr.coupled_translate(tiny["sd"], gu.TINY_SD_CFG, tiny["x0"], tiny["c"], tiny["c2"], tiny["uc"], e["dec_g"], e["S"],
                                 e["skip"], e["eta"], tiny["noise"])
    zs, xs, _info = tiny["base"]
    assert torch.equal(x, xs) and len(z) == len(zs) and all(torch.equal(a, b) for a, b in zip(z, zs))


def _rel(x, ref):
    return ((x - ref).abs().max() / ref.abs().max()).item()


def _psnr(x, ref):
    return (20.0 * torch.log10(ref.abs().max() / (x - ref).pow(2).mean().sqrt())).item()


def test_every_concept_set_is_no_no_op(tiny):
    """the GPU end-to-end test holds x to 8e-3 of the maximum (q0) or to the PSNR floor: each set must move x by ten times
    8e-3 at least, and the momentum alone must move it too. The encoder's z never moves."""
    zb, xb, _ = tiny["base"]
    for name in sr.SETS:
        z, x, info = tiny["sets"][name]
        rel = _rel(x, xb)
        print("sega/%s against no concepts: %.3e of the maximum" % (name, rel))
        assert torch.isfinite(x).all() and rel >= 10 * 8e-3, (name, rel)
        assert all(torch.allclose(a, b, rtol=1e-4, atol=1e-4) for a, b in zip(z, zb))
        assert set(info["mask"].unique().tolist()) <= {0.0, 1.0}
    _z, x_nomom, _ = tiny["run"]("thr", s_m=0.0)
    rel = _rel(x_nomom, tiny["sets"]["thr"][1])
    print("sega/thr momentum 0.3 against 0: %.3e of the maximum" % rel)
    assert rel >= 8e-3, rel
    # q0 keeps every element on every active iteration; the thresholded sets keep what the count rule says
    assert (tiny["sets"]["q0"][2]["kept"][2:] == sr.E2E["N"]).all() and (tiny["sets"]["q0"][2]["kept"][:2] == 0).all()


def test_sensitivity_of_the_thresholded_sets_bounds_the_gpu_test(tiny):
    """thr and two again with every forward's output perturbed by Gaussian noise of 5e-4 of its maximum - the end-to-end error
    DESIGN.md 14 records for this network on the engine - for three seeds. E2E_THR_DB may lie at most as low as 40 dB and must
    lie at least 3 dB below the worst PSNR measured here; E2E_MASK_DIFF may be 2 % at most and must be at least twice the worst
    share of differing final-mask cells. The margins cover the draw of the perturbation, not more."""
    worst_db, worst_share = 1e9, 0.0
    for name in ("thr", "two"):
        _z, x, info = tiny["sets"][name]
        for seed in (1, 2, 3):
            _zp, xp, ip = tiny["run"](name, perturb=(5e-4, torch.Generator().manual_seed(seed)))
            db, rel = _psnr(xp, x), _rel(xp, x)
            share = (ip["mask"] != info["mask"]).float().mean().item()
            print("sega/%s perturbed seed %d: %.2f dB, %.3e of the maximum, %d of %d mask cells differ"
                  % (name, seed, db, rel, int(round(share * info["mask"].numel())), info["mask"].numel()))
            worst_db, worst_share = min(worst_db, db), max(worst_share, share)
    _z, xq, _ = tiny["run"]("q0", perturb=(5e-4, torch.Generator().manual_seed(1)))
    _z, xn, _ = tiny["run"](None, perturb=(5e-4, torch.Generator().manual_seed(1)))
    print("sega/q0 perturbed: %.3e of the maximum, %.2f dB; no concepts: %.3e, %.2f dB"
          % (_rel(xq, tiny["sets"]["q0"][1]), _psnr(xq, tiny["sets"]["q0"][1]), _rel(xn, tiny["base"][1]),
             _psnr(xn, tiny["base"][1])))
    assert 40.0 <= sr.E2E_THR_DB <= worst_db - 3.0, (sr.E2E_THR_DB, worst_db)
    assert 2.0 * worst_share <= sr.E2E_MASK_DIFF <= 0.02, (sr.E2E_MASK_DIFF, worst_share)
