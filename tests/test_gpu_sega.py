"""Semantic guidance on the coupled translate loop (include/cyclediff.h cd_sega / cd_op_sega_guidance;
csrc/sega.hip k_sega_threshold, k_sega_combine).

  1. the two kernels against the fp32 torch restatement (tests/_sega_ref.py guidance_step), bit for bit
  2. the loop end to end without a threshold (q = 0) against the float64 restatement, at the bounds of the other end-to-end tests
  3. the thresholded sets at the PSNR floor and the mask cap tests/test_sega_host.py derives
  4. what must stay bit-identical
  5. refusals, each with its message and nothing written
  6. the wrapper
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _attn_control_ref as acr
import _sega_ref as sr
import golden_util as gu
from cycle_diffusion_amd import _ffi, schedule
from cycle_diffusion_amd import semantic_guidance as sgm
from cycle_diffusion_amd._ffi import ptr
from test_gpu_models import _load, tiny_iddpm_desc, tiny_sd_desc

pytestmark = pytest.mark.gpu

FMT = 1.0 if _ffi.load_library().cd_act_format() == 1 else 8.0
DDIM = _ffi.CD_SCHED_DDIM
QS = [0.0, 0.5, 0.9, 0.999, 1.0]


# ------------------------------------------------------------------------------------------------ 1. the kernels
def _op(engine, eps_all, tab, i, nu, g, s_m, beta, ld=None):
    """cd_op_sega_guidance and guidance_step on the same tensors -> (got, ref), each (eps, nu, tau, kept, mask)"""
    E = len(tab)
    Bd = eps_all.shape[0] // (2 + E)
    nu_d = nu.clone().cuda()
    gd = torch.as_tensor(g, dtype=torch.float32).cuda() if not isinstance(g, float) else g
    eps, tau, kept, mask = engine.op_sega_guidance(eps_all.cuda(), tab, i, nu_d, guidance=gd, momentum_scale=s_m,
                                                   momentum_beta=beta, ld=ld)
    torch.cuda.synchronize()
    u, c = eps_all[:Bd], eps_all[(1 + E) * Bd:]
    p = eps_all[Bd:(1 + E) * Bd].reshape((E, Bd) + tuple(eps_all.shape[1:]))
    r_eps, r_nu, r_tau, r_kept, r_mask, _ties = sr.guidance_step(u, c, p, tab, i, nu, g, s_m, beta)
    return (eps.cpu(), nu_d.cpu(), tau.cpu(), kept.cpu(), mask.cpu()), (r_eps, r_nu, r_tau, r_kept, r_mask)


def _same(got, ref, what):
    for name, a, b in zip(("eps", "nu", "tau", "kept", "mask"), got, ref):
        assert torch.equal(a, b), (what, name, (a.double() - b.double()).abs().max().item())


def _table(rows, N, K=8):
    return sgm.table_rows(rows, K, N)


# (Bd, C, HW, E): two values; odd sizes below one pass of the workgroup; several rows and concepts; the eight-concept limit
# at N = 16384; the 96 x 96 latent's N = 36864
OP_CASES = [(1, 1, 2, 1), (3, 3, 100, 1), (2, 4, 256, 3), (1, 4, 4096, 8), (1, 4, 9216, 2)]


@pytest.mark.parametrize("pad", [0, 4], ids=["ld_c", "ld_c4"])
@pytest.mark.parametrize("case", OP_CASES, ids=["b%d_c%d_hw%d_e%d" % c for c in OP_CASES])
def test_op_vs_restatement_bit_for_bit(engine, case, pad):
    """every q of QS on every concept slot (concept e of call n takes QS[(n + e) % 5]), odd concepts reversed, weights that
    differ; scalar guidance on the dense layout and per-sample guidance on the padded one; nu carried from call to call"""
    Bd, Cc, HW, E = case
    g = torch.Generator().manual_seed(Bd * 1000 + HW + E)
    eps_all = torch.randn((2 + E) * Bd, Cc, HW, generator=g)
    nu = torch.randn(Bd, Cc, HW, generator=g) * 0.1
    guid = 3.0 if pad == 0 else [1.5 + 0.5 * r for r in range(Bd)]
    for n in range(len(QS)):
        rows = [((-1.0) ** e * (2.0 + e), 1.0 + 0.25 * e, QS[(n + e) % len(QS)], 0, 8) for e in range(E)]
        got, ref = _op(engine, eps_all, _table(rows, Cc * HW), 3, nu, guid, 0.3, 0.6, ld=Cc + pad)
        _same(got, ref, (case, pad, n))
        assert set(got[4].unique().tolist()) <= {0.0, 1.0}
        nu = ref[1]


def test_op_inactive_concepts(engine):
    """one inactive concept among active ones contributes nothing and reports tau = kept = mask = 0; with none active eps is
    base + s_m * nu and nu decays"""
    g = torch.Generator().manual_seed(3)
    Bd, Cc, HW, E = 2, 4, 256, 3
    eps_all = torch.randn((2 + E) * Bd, Cc, HW, generator=g)
    nu = torch.randn(Bd, Cc, HW, generator=g)
    rows = [(3.0, 1.0, 0.9, 0, 8), (5.0, 1.0, 0.5, 4, 8), (-2.0, 0.5, 0.8, 2, 3)]
    tab = _table(rows, Cc * HW)
    got, ref = _op(engine, eps_all, tab, 2, nu, 3.0, 0.3, 0.6)  # concept 1 not yet active
    _same(got, ref, "one inactive")
    assert not got[2][:, 1].any() and not got[3][:, 1].any() and not got[4][:, 1].any() and got[3][:, 0].all()
    got, ref = _op(engine, eps_all, _table([(3.0, 1.0, 0.9, 5, 8)] * 3, Cc * HW), 2, nu, 3.0, 0.3, 0.6)
    _same(got, ref, "all inactive")
    u, c = eps_all[:Bd], eps_all[4 * Bd:]
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    assert torch.equal(got[0], (u + f(3.0) * (c - u)) + (torch.zeros_like(u) + f(0.3) * nu))
    got0, _ = _op(engine, torch.cat([eps_all[:2 * Bd], c], 0), _table([(3.0, 1.0, 0.9, 5, 8)], Cc * HW), 2, nu, 3.0, 0.0, 0.6)
    assert torch.equal(got0[0], u + f(3.0) * (c - u)) and torch.equal(got0[1], f(0.6) * nu + (f(1.0) - f(0.6)) * torch.zeros_like(nu))


def test_op_ties_zeros_and_equal_rows(engine):
    g = torch.Generator().manual_seed(4)
    Bd, Cc, HW, E = 2, 4, 300, 2
    N = Cc * HW
    # inputs quantised to multiples of 1/8: runs of equal |d| straddle every threshold
    eps_all = (torch.randn((2 + E) * Bd, Cc, HW, generator=g) * 4).round() / 8
    nu = torch.zeros(Bd, Cc, HW)
    for q in QS:
        got, ref = _op(engine, eps_all, _table([(1.0, 1.0, q, 0, 8), (-0.5, 2.0, q, 0, 8)], N), 0, nu, 3.0, 0.3, 0.6, ld=Cc + 4)
        _same(got, ref, ("ties", q))
    # p_e == u everywhere: tau = 0, everything kept, gamma = 0
    same = eps_all.clone()
    same[Bd:3 * Bd] = same[:Bd].repeat(2, 1, 1)
    got, ref = _op(engine, same, _table([(5.0, 1.0, 0.9, 0, 8), (-5.0, 1.0, 0.5, 0, 8)], N), 0, nu, 3.0, 0.3, 0.6)
    _same(got, ref, "p == u")
    assert not got[2].any() and (got[3] == N).all() and got[4].all()
    u, c = same[:Bd], same[3 * Bd:]
    assert torch.equal(got[0], u + torch.tensor(3.0) * (c - u))
    # values with +0 and -0, half of |d| exactly zero
    z = torch.randn((2 + E) * Bd, Cc, HW, generator=g)
    z[:, :, ::2] = 0.0
    z[1::2, :, ::4] = -0.0
    for q in (0.25, 0.5, 0.75):
        got, ref = _op(engine, z, _table([(2.0, 1.0, q, 0, 8), (-2.0, 1.0, q, 0, 8)], N), 0, nu, [2.0, 4.0], 0.3, 0.6)
        _same(got, ref, ("zeros", q))


def test_op_three_chained_iterations_carry_nu(engine):
    g = torch.Generator().manual_seed(6)
    Bd, Cc, HW, E = 2, 4, 256, 2
    tab = _table([(5.0, 1.0, 0.9, 1, 8), (-4.0, 1.0, 0.8, 0, 2)], Cc * HW)
    nu_g = nu_r = torch.zeros(Bd, Cc, HW)
    for i in range(3):
        eps_all = torch.randn((2 + E) * Bd, Cc, HW, generator=g)
        got, _ = _op(engine, eps_all, tab, i, nu_g, 3.0, 0.3, 0.6)
        _, ref = _op(engine, eps_all, tab, i, nu_r, 3.0, 0.3, 0.6)
        _same(got, ref, ("chain", i))
        nu_g, nu_r = got[1], ref[1]
    assert nu_g.abs().max() > 0


# ------------------------------------------------------------------------------------------------ shared end-to-end runs
class _Setup:
    def __init__(self, engine):
        fx = gu.load("latent_cycle_tiny")
        self.net, self.sd = _load(engine, tiny_sd_desc(), fx)
        self.x0, self.c, self.uc, self.c2 = acr.e2e_inputs()
        e = sr.E2E
        self.K = e["S"] - e["skip"]
        self.noise = gu.latent_noise(e["noise_seed"], self.x0.shape, self.K)
        sch = schedule.DDIMSchedule(schedule.latent_alphas_cumprod(), e["S"], e["eta"])
        self.ce, self.cd = sch.coef_encode(e["skip"]), sch.coef_decode(e["skip"])
        self.engine = engine

    def kw(self, n_dec=1, dec_g=None, rows=slice(None)):
        g = sr.E2E["dec_g"] if dec_g is None else dec_g
        return dict(enc_ctx_c=self.c[rows].cuda(), enc_ctx_uc=self.uc[rows].cuda(), enc_guidance=1.0,
                    dec_ctx_c=self.c2[rows].repeat(n_dec, 1, 1).cuda(), dec_ctx_uc=self.uc[rows].repeat(n_dec, 1, 1).cuda(),
                    dec_guidance=g, n_dec=n_dec, noise=torch.stack(self.noise, 0)[:, rows].contiguous().cuda())

    def sega(self, name, tab=None, s_m=None, n_dec=1, ectx=None, **kw):
        e = sr.E2E
        ectx = sr.e2e_edit_ctx(name, n_dec=n_dec) if ectx is None else ectx
        out = self.engine.cycle_translate_sega(self.net, DDIM, kw.pop("x0", self.x0).cuda(), self.ce, self.cd, ectx.cuda(),
                                               sr.e2e_table(name) if tab is None else tab, e["s_m"] if s_m is None else s_m,
                                               e["beta"], **dict(self.kw(n_dec=n_dec), **kw))
        self.engine.synchronize()
        return out


@pytest.fixture(scope="module")
def su(engine):
    return _Setup(engine)


@pytest.fixture(scope="module")
def runs(su):
    """the engine's and the float64 restatement's run of every concept set, computed once and left unchanged"""
    out = {}
    for name in sr.SETS:
        ref = sr.e2e_run(su.sd, su.x0, su.c, su.uc, su.c2, su.noise, name, dtype=torch.float64)
        out[name] = (tuple(t.cpu() for t in su.sega(name)), ref)
    return out


def _rel_db(got, ref):
    d = got.double() - ref
    return (d.abs().max() / ref.abs().max()).item(), (20.0 * torch.log10(ref.abs().max() / d.pow(2).mean().sqrt())).item()


# ------------------------------------------------------------------------------------------------ 2. end to end, q = 0
def test_loop_without_threshold_vs_float64_restatement(su, runs, report):
    """bounds of tests/test_gpu_attn_control.py::test_controlled_loop_vs_restatement: 8e-3 x format factor of the maximum and
    40 dB (bf16 build: 25 dB); every active iteration keeps all N elements"""
    (z, x, tau, kept, mask), (zr, xr, info) = runs["q0"]
    rel, db = _rel_db(x, xr)
    zrel, _ = _rel_db(z, torch.stack(zr, 1))
    report.add("sega/e2e_q0", rel_to_max=rel, psnr_db=db, z_rel_to_max=zrel)
    print("sega/e2e_q0 rel_to_max=%.3e psnr=%.2f dB z rel=%.3e" % (rel, db, zrel))
    assert torch.isfinite(x).all() and rel < 8e-3 * FMT and db > (40.0 if FMT == 1.0 else 25.0), (rel, db)
    assert zrel < 8e-3 * FMT, zrel
    assert (kept[2:] == sr.E2E["N"]).all() and not kept[:2].any() and not tau[:2].any()
    assert mask.all()


# ------------------------------------------------------------------------------------------------ 3. thresholded sets
@pytest.mark.parametrize("name", ["thr", "two"])
def test_thresholded_loop_vs_float64_restatement(su, runs, report, name):
    """The threshold is discontinuous, so these sets are held to the PSNR floor and the mask cap that
    tests/test_sega_host.py::test_sensitivity_of_the_thresholded_sets_bounds_the_gpu_test derives from the engine's own
    forward error (sr.E2E_THR_DB, sr.E2E_MASK_DIFF), tau to 5 % on the iterations before the first one whose kept count
    disagrees, and the kept count to the count rule wherever the restatement has no ties."""
    (z, x, tau, kept, mask), (zr, xr, info) = runs[name]
    tab = sr.e2e_table(name)
    K, N = su.K, sr.E2E["N"]
    rel, db = _rel_db(x, xr)
    share = (mask.double() != info["mask"]).double().mean().item()
    bad = [i for i in range(K) if not torch.equal(kept[i], info["kept"][i])]
    first_bad = bad[0] if bad else (K - 1 if share > 0 else K)
    active = torch.tensor([[int(cp["warm"]) <= i < int(cp["cool"]) for cp in tab] for i in range(K)])[:, None, :].expand(K, 2, -1)
    dev = ((tau.double() - info["tau"]).abs() / info["tau"].abs().clamp_min(1e-30))
    tdev = dev[:first_bad][active[:first_bad]].max().item() if first_bad else 0.0
    report.add("sega/e2e_" + name, rel_to_max=rel, psnr_db=db, mask_cells_differ=int(round(share * mask.numel())),
               mask_cells=mask.numel(), tau_rel=tdev, first_iteration_kept_differs=first_bad)
    print("sega/e2e_%s rel_to_max=%.3e psnr=%.2f dB, %d of %d mask cells differ, tau rel %.3e before iteration %d"
          % (name, rel, db, int(round(share * mask.numel())), mask.numel(), tdev, first_bad))
    assert torch.isfinite(x).all() and db >= sr.E2E_THR_DB, db
    assert share <= sr.E2E_MASK_DIFF, share
    assert tdev <= 0.05, tdev
    assert not tau[~active].any() and not kept[~active].any()
    for e, cp in enumerate(tab):
        rule = sr.kept_rule(N, int(cp["lo"]), float(cp["frac"]))
        ok = active[:, :, e] & ~info["ties"][:, :, e]
        assert (kept[:, :, e][ok] == rule).all(), (name, e, rule, kept[:, :, e])
    assert set(mask.unique().tolist()) <= {0.0, 1.0}


# ------------------------------------------------------------------------------------------------ 4. bit-exact
def _never(name):
    tab = sr.e2e_table(name).copy()
    tab["cool"] = tab["warm"]
    return tab


def test_z_is_the_plain_calls(su, runs):
    z0, _x0 = su.engine.cycle_translate(su.net, DDIM, su.x0.cuda(), su.ce, su.cd, **su.kw())
    su.engine.synchronize()
    for name in sr.SETS:
        assert torch.equal(runs[name][0][0], z0.cpu()), name


def test_never_active_concepts_without_momentum_are_the_plain_calls(su):
    eng, x0 = su.engine, su.x0.cuda()
    ctl = acr.e2e_control()
    mask = torch.zeros(2, 1, 16, 16)
    mask[:, 0, 4:12, 2:9] = 1.0
    z0, xp = eng.cycle_translate(su.net, DDIM, x0, su.ce, su.cd, **su.kw())
    _z, xm = eng.cycle_translate_masked(su.net, DDIM, x0, su.ce, su.cd, mask.cuda(), mask_source="encoder", **su.kw())
    _z, xc = eng.cycle_translate_ctrl(su.net, DDIM, x0, su.ce, su.cd, *ctl, acr.E2E["n_ctrl"], **su.kw())
    eng.synchronize()
    for what, ref, kw in (("plain", xp, {}), ("masked", xm, dict(mask=mask.cuda(), mask_source="encoder")),
                          ("ctrl", xc, dict(ctrl=ctl + (acr.E2E["n_ctrl"],)))):
        z, x, tau, kept, m = su.sega("two", tab=_never("two"), s_m=0.0, **kw)
        assert torch.equal(z, z0) and torch.equal(x, ref), (what, (x - ref).abs().max().item())
        assert not tau.any() and not kept.any() and not m.any()
    assert not torch.equal(xm, xp) and not torch.equal(xc, xp)
    # ... and an active set composes with both: finite, and not the result without them
    z, x, _t, _k, _m = su.sega("two", mask=mask.cuda(), mask_source="encoder", ctrl=ctl + (acr.E2E["n_ctrl"],))
    assert torch.isfinite(x).all() and torch.equal(z, z0) and not torch.equal(x, xm)


def test_folded_ensemble_equals_each_member_alone(su):
    B = 2
    z, x, tau, kept, m = su.sega("two", n_dec=2, dec_guidance=[1.5] * B + [4.0] * B)
    for j, g in enumerate((1.5, 4.0)):
        zj, xj, tj, kj, mj = su.sega("two", dec_guidance=g)
        rows = slice(j * B, (j + 1) * B)
        assert torch.equal(z, zj) and torch.equal(x[rows], xj), (g, (x[rows] - xj).abs().max().item())
        assert torch.equal(tau[:, rows], tj) and torch.equal(kept[:, rows], kj) and torch.equal(m[rows], mj)
    assert (x[:B] - x[B:]).abs().max() > 1e-3


def test_one_sample_alone_is_its_row_of_the_batch_and_calls_repeat(su, runs):
    z, x, tau, kept, m = runs["two"][0]
    E = len(sr.SETS["two"])
    ectx = sr.e2e_edit_ctx("two").reshape(E, 2, 77, 64)[:, :1].reshape(E, 77, 64)
    z1, x1, t1, k1, m1 = su.sega("two", ectx=ectx, x0=su.x0[:1], **su.kw(rows=slice(0, 1)))
    assert torch.equal(z1.cpu(), z[:1]) and torch.equal(x1.cpu(), x[:1])
    assert torch.equal(t1.cpu(), tau[:, :1]) and torch.equal(k1.cpu(), kept[:, :1]) and torch.equal(m1.cpu(), m[:1])
    again = su.sega("two")  # the engine holds no momentum between calls
    for a, b in zip(again, runs["two"][0]):
        assert torch.equal(a.cpu(), b)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_entry_point_refuses_what_it_cannot_do(su):
    eng, K, B = su.engine, su.K, 2
    lib = eng.lib
    kw = su.kw()
    x0 = su.x0.cuda()
    ectx = sr.e2e_edit_ctx("two").cuda()
    z = torch.full((B, K + 1, 4, 16, 16), -7.0, device="cuda")
    x = torch.full((B, 4, 16, 16), -7.0, device="cuda")
    d32 = tiny_sd_desc()
    d32.precision = _ffi.CD_PREC_F32
    net32, _ = _load(eng, d32, gu.load("latent_cycle_tiny"))
    net_pix, _ = _load(eng, tiny_iddpm_desc(), gu.load("unet_tiny_iddpm"))

    def call(tab=None, E=None, net=su.net, kind=DDIM, dec_g=3.0, s_m=0.3, beta=0.6, cd=su.cd, **row):
        tab = sr.e2e_table("two").copy() if tab is None else tab
        for k, v in row.items():
            tab[k][1] = v
        sega = _ffi.Sega(edit_ctx=ptr(ectx), concepts_host=tab.ctypes.data, E=len(tab) if E is None else E, momentum_scale=s_m,
                         momentum_beta=beta)
        a = _ffi.TranslateArgs(
            size=C.sizeof(_ffi.TranslateArgs), net=net, sched_kind=kind, x0=ptr(x0), enc_ctx_c=ptr(kw["enc_ctx_c"]),
            enc_ctx_uc=ptr(kw["enc_ctx_uc"]), enc_guidance=1.0, dec_ctx_c=ptr(kw["dec_ctx_c"]), dec_ctx_uc=ptr(kw["dec_ctx_uc"]),
            dec_guidance=dec_g, ctx_len=77, B=B, n_dec=1, K=K, coef_enc_host=su.ce.ctypes.data, coef_dec_host=cd.ctypes.data,
            noise=ptr(kw["noise"]), seed=0, last_uses_x0=1, z_out=ptr(z), x_out=ptr(x), sega=C.pointer(sega))
        return lib.cd_cycle_translate(eng.h, C.byref(a))

    cd_bad = su.cd.copy()
    cd_bad["t"][1] += 1
    nan, inf = float("nan"), float("inf")
    refused = [
        (dict(E=0), "E = 0"), (dict(E=9), "E = 9"), (dict(kind=_ffi.CD_SCHED_DDPM), "CD_SCHED_DDIM"),
        (dict(net=net_pix), "text context"), (dict(net=net32), "CD_PREC_F32"), (dict(dec_g=1.0), "dec_guidance"),
        (dict(dec_g=0.0), "dec_guidance"), (dict(lo=-1), "lo = -1"), (dict(lo=1024), "lo = 1024"), (dict(frac=1.0), "frac"),
        (dict(frac=-0.25), "frac"), (dict(frac=nan), "frac"), (dict(warm=5, cool=4), "warm = 5"), (dict(cool=K + 1), "cool = 21"),
        (dict(warm=-1), "warm = -1"), (dict(scale=nan), "scale"), (dict(scale=inf), "scale"), (dict(weight=-inf), "weight"),
        (dict(s_m=nan), "momentum_scale"), (dict(beta=nan), "momentum_beta"), (dict(beta=1.5), "momentum_beta"),
        (dict(beta=-0.1), "momentum_beta"), (dict(cd=cd_bad), "disagree"),
    ]
    for args, text in refused:
        assert call(**args) != 0, args
        err = lib.cd_last_error().decode()
        assert text in err, (args, err)
        eng.synchronize()
        assert bool((x == -7.0).all()) and bool((z == -7.0).all()), args
    assert call() == 0, lib.cd_last_error().decode()
    eng.synchronize()
    assert torch.isfinite(x).all() and torch.isfinite(z).all() and not bool((x == -7.0).any())
    # the Python binding refuses the local blend beside concepts before the engine is called
    with pytest.raises(ValueError, match="local blend"):
        eng._cycle_translate(su.net, DDIM, x0, su.ce, su.cd, kw["enc_ctx_c"], kw["enc_ctx_uc"], 1.0, kw["dec_ctx_c"], kw["dec_ctx_uc"],
                             3.0, 1, kw["noise"], 0, True, blend=(None, None, 8, 3, 0.3, 0),
                             sega=(ectx, sr.e2e_table("two"), 0.3, 0.6))


# ------------------------------------------------------------------------------------------------ 6. wrapper
def _tiny_wrapper(**kw):
    from test_gpu_wrappers import _make
    return _make(True, **kw)


def test_wrapper_edit_concepts():
    """the SD-family text wrapper at the size the wrapper tests use (tests/test_gpu_wrappers.py TinyTextWrapper)"""
    from cycle_diffusion_amd.semantic_guidance import EditConcept, concept_table
    common = dict(n_trials=1, skip_steps=[4], decoder_unconditional_guidance_scales=[3.0])
    image = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(5)).cuda()
    src, tgt = ["a photo of a cat", "a red car"], ["a photo of a small dog", "a blue car"]
    concepts = [EditConcept("glasses", 5.0, 0.9), EditConcept("smile", 4.0, 0.8, reverse=True, warmup=0.2, cooldown=0.8)]

    def run(w, **kw):
        torch.manual_seed(9)
        with torch.no_grad():
            img = w.translate(image, src, tgt, **kw)
        return img, w.last_latents[0].clone()

    def recorded(w, name):
        calls = []
        real = getattr(w.engine, name)
        setattr(w.engine, name, lambda *a, **k: (calls.append((a, k, real(*a, **k))), calls[-1][2])[1])
        return calls, lambda: setattr(w.engine, name, real)

    w0, emb, _u, _v = _tiny_wrapper(**common)
    w1, _e, _u, _v = _tiny_wrapper(edit_concepts="", **common)
    w2, _e, _u, _v = _tiny_wrapper(edit_concepts="+glasses:5:0.9", **common)
    plain, plain_lat = run(w0)
    # an empty string: the calls of today - the plain coupled entry point, never the new one
    calls, undo = recorded(w1, "cycle_translate_sega")
    plain_calls, undo2 = recorded(w1, "cycle_translate")
    try:
        same, _ = run(w1)
    finally:
        undo(), undo2()
    assert torch.equal(same, plain) and not calls and len(plain_calls) == 1 and w1.last_edit_masks is None
    # the keyword: one engine call on the inputs the wrapper builds from its own get_condition and concept_table
    calls, undo = recorded(w0, "cycle_translate_sega")
    try:
        img_kw, lat_kw = run(w0, edit_concepts=concepts)
    finally:
        undo()
    assert len(calls) == 1 and w0.last_translate_coupled
    args, kw, (z, x, tau, kept, mask) = calls[0]
    K, N = len(w0._schedule()) - 4, 4 * 16 * 16
    assert np.array_equal(args[6], concept_table(concepts, K, N)) and (args[7], args[8]) == (0.3, 0.6)
    want_ctx = torch.cat([emb([c.text] * 2) for c in concepts], 0).to(args[5].device, torch.float32)
    assert torch.equal(args[5], want_ctx)
    z2, x2, tau2, kept2, mask2 = w0.engine.cycle_translate_sega(*args, **kw)
    w0.engine.synchronize()
    assert torch.equal(x2, lat_kw) and torch.equal(x, lat_kw) and torch.equal(mask2, mask)
    assert torch.isfinite(img_kw).all() and not torch.equal(img_kw, plain)
    assert len(w0.last_edit_masks) == 1 and tuple(w0.last_edit_masks[0].shape) == (2, 2, 4, 16, 16)
    assert set(w0.last_edit_masks[0].unique().tolist()) <= {0.0, 1.0} and 0 < w0.last_edit_masks[0].mean() < 1
    assert tuple(w0.last_edit_taus[0].shape) == (K, 2, 2) and torch.equal(w0.last_edit_taus[0], tau)
    # the config string gives what the keyword gives, and an empty list switches the config off
    img_cfg, lat_cfg = run(w2)
    img_one, lat_one = run(w0, edit_concepts=[EditConcept("glasses", 5.0, 0.9)])
    assert torch.equal(lat_cfg, lat_one) and torch.equal(img_cfg, img_one)
    off, _ = run(w2, edit_concepts=[])
    assert torch.equal(off, plain)
    # encode() + forward() has no coupled loop
    with torch.no_grad(), pytest.raises(ValueError, match="translate"):
        w2(w2.encode(image, src), image, src, tgt)
    from cycle_diffusion_amd.gan_wrapper import baselines
    with pytest.raises(ValueError, match="edit_concepts"):
        baselines.SDDDIBTextWrapper(source_model_type="none", custom_steps=4, edit_concepts="+glasses")
    w3, _e, _u, _v = _tiny_wrapper(n_trials=1, skip_steps=[4], decoder_unconditional_guidance_scales=[1.0])
    with torch.no_grad(), pytest.raises(ValueError, match="guided"):
        w3.translate(image, src, tgt, edit_concepts=concepts)
