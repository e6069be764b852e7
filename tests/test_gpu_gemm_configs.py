"""Every tile configuration, K-step depth, split and K order the implicit-GEMM launcher can pick (csrc/conv_gemm.hip), each on
a shape battery derived from its own BM / BN / BK / ring depth (tests/_gemm_sweep.py).

The configuration list is parsed, not written down: every kCfgs id at its own depth, every id the launcher accepts with the
BK = 32 flag, every (tile, bk32, split) triple of the shipped tile table (tests/test_tune_table.py checks on the host that
nothing is missing). Every case

  0. asserts through cd_op_last_gemm_config that the tile, K-step depth and split it asked for are what ran (the GEGLU
     fallback of the tiles whose wave tile is not a multiple of 64 columns is asserted as such);
  1. is held to the operator's bounds against torch.nn.functional.conv2d in float64 on the 16-bit-rounded operands, the
     epilogue applied in float64: rel_to_max < 5e-3, mean_rel < 2e-3, GroupNorm block sums < 2e-3 of their maximum, finite;
  2. must equal, bit for bit, tile 3 at the same K-step depth, split and K order (the reduction is k-ascending with the same
     epilogue arithmetic on every tile), and - without split-K - the other K-step depth as well.

Channel-major K order and the grouped tile walk are process-wide settings (read once): they run in child processes
(tests/_gemm_env_child.py), one at a time; nothing more is started on the GPU after a child that failed. A third child runs
the launch forms of the FID Inception-v3's BasicConv2d units that meet the channel-major order at its production batch (valid
3 x 3 at stride 1 and 2 on odd sizes, 3 channels padded to 32, 1 x 7 and 7 x 1) through cd_op_basic_conv, under the same rule.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _gemm_sweep as gs
import _inception_ops_ref as ir
import _ops
from _ops import bf16_round as r16

pytestmark = pytest.mark.gpu

CONFIGS = gs.configs_under_test()
HERE = os.path.dirname(os.path.abspath(__file__))

# Pairs that are NOT bit-identical by construction are listed here with the reason, and held to the float64 bounds only.
# (config id, case name without the configuration prefix) -> reason.
_T9 = ("256x64 w8x1 s4 at BK = 64 fills the LDS with its ring and has no bias / time-embedding tables (TileCfg::HAS_TAB), so its "
       "16-bit output takes the generic epilogue, which adds (acc + bias) + row vector; every other tile takes the table "
       "epilogue, which adds acc + (bias + row vector): one fp32 rounding apart, visible as one 16-bit ulp in a few outputs. "
       "Only with bias AND row vector AND 16-bit output without activation; the shipped table never picks this tile.")
NOT_BIT_IDENTICAL = {("t9_bkown_s1", "e16_all_3x3"): _T9, ("t9_bkown_s1", "e16_all_1x1"): _T9}

_anchor_cache = {}


def _anchor(engine, c, o, bk32, split):
    """tile 3 on the same operands at the given depth and split; cached per shape (many configurations share shapes)"""
    key = (c["name"].split("/", 1)[1], tuple(sorted((k, v) for k, v in c.items() if k != "name")), bk32, split)
    if key not in _anchor_cache:
        cfg = (gs.ANCHOR_TILE, bk32, split)
        y, st, rb = _ops.run_conv_case(engine, c, o, gs.tile_arg(cfg))
        want = gs.launched(cfg, c["geglu"])
        assert (rb["tile"], rb["bk"], rb["split"]) == want and rb["chm"] == 0, (c["name"], rb, want)
        _anchor_cache[key] = y
    return _anchor_cache[key]


def _check_stats(c, st, ref_st):
    err = (st.double() - ref_st).abs().max().item() / max(ref_st.abs().max().item(), 1e-6)
    return err


@pytest.mark.parametrize("cfg", CONFIGS, ids=[gs.config_id(c) for c in CONFIGS])
def test_gemm_configuration(engine, report, cfg):
    tile, bk32, split = cfg
    bk = gs.effective_bk(tile, bk32)
    worst = dict(rel_to_max=0.0, mean_rel=0.0, stats_rel=0.0)
    bit_identical, failures, ncases = True, [], 0
    for c in gs.battery(cfg):
        ncases += 1
        short = c["name"].split("/", 1)[1]
        o = gs.operands(c, r16)
        ref, ref_st = gs.reference(c, o)
        got, st, rb = _ops.run_conv_case(engine, c, o, gs.tile_arg(cfg))
        # 0. the requested configuration ran (tap-major, row-major walk: these shapes are far below the launcher's thresholds)
        want = gs.launched(cfg, c["geglu"])
        assert (rb["tile"], rb["bk"], rb["split"]) == want, (c["name"], rb, want)
        assert rb["chm"] == 0 and rb["tile_group"] == 0, (c["name"], rb)
        # 1. float64
        es = gs.err_stats(got, ref)
        print("%-40s rel_to_max %.3e mean_rel %.3e" % (c["name"], es["rel_to_max"], es["mean_rel"]))
        worst["rel_to_max"] = max(worst["rel_to_max"], es["rel_to_max"])
        worst["mean_rel"] = max(worst["mean_rel"], es["mean_rel"])
        if not gs.within_bounds(es):
            failures.append((c["name"], "float64 bounds", es))
        if c["stats"]:
            serr = _check_stats(c, st, ref_st)
            worst["stats_rel"] = max(worst["stats_rel"], serr)
            if not (serr < gs.STATS_TOL and bool(torch.isfinite(st).all())):
                failures.append((c["name"], "statistics", serr))
        # 2. tile 3, same depth / split / K order; without split-K the other depth too (split ranges are cut in K steps of
        # the launched depth, so with split-K the two depths sum different partial ranges)
        others = [("tile 3", bk == 32, split)]
        if split == 1 and (c["C0"] % 64 == 0 and c["C1"] % 64 == 0):
            others.append(("tile 3 at the other depth", bk != 32, 1))
        for what, a_bk32, a_split in others:
            same = torch.equal(got, _anchor(engine, c, o, int(a_bk32), a_split))
            if not same and (gs.config_id(cfg), short) not in NOT_BIT_IDENTICAL:
                bit_identical = False
                failures.append((c["name"], "not bit-identical to " + what,
                                 (got - _anchor(engine, c, o, int(a_bk32), a_split)).abs().max().item()))
    report.add("gemm_config/" + gs.config_id(cfg), cases=ncases, bit_identical=bit_identical, **worst)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ child processes
_child_failed = []  # the first child that failed, died on a signal or timed out: nothing else is started on the GPU after it


def _run_child(battery, env_extra, tmp, timeout):
    if _child_failed:
        pytest.fail("not started: an earlier child process failed (%s)" % (_child_failed[0],))
    out = os.path.join(str(tmp), battery + ".npz")
    env = dict(os.environ, **env_extra)
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(HERE), HERE] + [p for p in [env.get("PYTHONPATH")] if p])
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "_gemm_env_child.py"), battery, out], env=env,
                           capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        _child_failed.append("%s: timed out after %d s; stderr tail: %s" % (battery, timeout, str(e.stderr or "")[-1500:]))
        pytest.fail(_child_failed[0])
    if r.returncode != 0:
        _child_failed.append("%s: exit status %d; stderr tail: %s" % (battery, r.returncode, r.stderr[-1500:]))
        pytest.fail(_child_failed[0])
    return np.load(out)


@pytest.fixture(scope="module")
def chm_child(tmp_path_factory, engine):
    return _run_child("chm", {"CYCLEDIFF_KORDER": "2"}, tmp_path_factory.mktemp("gemm_chm"), 600)


@pytest.fixture(scope="module")
def group_child(tmp_path_factory, engine, chm_child):  # after the channel-major child: one child at a time, none after a failure
    return _run_child("group", {"CYCLEDIFF_TILE_GROUP": str(gs.GROUP_SIZE), "CYCLEDIFF_TILE_GROUP_MIN_N": "64"},
                      tmp_path_factory.mktemp("gemm_group"), 600)


def _chm_cases(tile, bk32):
    cases = gs.chm_battery()
    if bk32:  # its own concat case (boundary not 64-aligned); channel counts that are multiples of 32 only fit this variant
        cases = cases + [gs.CHM_BK32_ONLY]
    return cases


# (b) of the channel-major acceptance: max|err| vs float64 at most CHM_ERR_FACTOR x the tap-major run's + one fp32 ulp of max|ref|
CHM_ERR_FACTOR = 2.0


@pytest.mark.parametrize("tb", gs.CHM_TILES, ids=["t%d_bk%s" % (t, "32" if b else "own") for t, b in gs.CHM_TILES])
def test_channel_major_order(engine, report, chm_child, tb):
    tile, bk32 = tb
    bk = gs.effective_bk(tile, bk32)
    failures = []
    for c, split, chm_want in _chm_cases(tile, bk32):
        cfg = (tile, bk32, split)
        key = "%s|%s" % (c["name"], gs.config_id(cfg))
        got = torch.from_numpy(child_arr(chm_child, key + "|y"))
        rb = child_arr(chm_child, key + "|rb").tolist()  # tile, bk, split, chm, tile_group
        want = gs.launched(cfg)
        assert tuple(rb[:3]) == want and rb[3] == chm_want and rb[4] == 0, (key, rb, want, chm_want)
        o = gs.operands(c, r16)
        ref, ref_st = gs.reference(c, o)
        es = gs.err_stats(got, ref)
        # the parent process runs tap-major (default K order: channel-major only from 64 x 64 images and 32 MiB up)
        tap, _, rb_tap = _ops.run_conv_case(engine, c, o, gs.tile_arg((gs.ANCHOR_TILE, int(bk == 32), split)))
        assert rb_tap["chm"] == 0 and rb_tap["tile"] == gs.ANCHOR_TILE and rb_tap["split"] == split, rb_tap
        es_tap = gs.err_stats(tap, ref)
        ulp = float(np.spacing(np.float32(es["ref_max"])))
        ratio = es["max_abs"] / max(es_tap["max_abs"], 1e-30)
        report.add("gemm_chm/" + key, rel_to_max=es["rel_to_max"], mean_rel=es["mean_rel"], max_abs=es["max_abs"],
                   max_abs_tap_major=es_tap["max_abs"], ratio=ratio, chm=rb[3])
        print("%-60s chm %d max_abs %.3e tap-major %.3e ratio %.3f" % (key, rb[3], es["max_abs"], es_tap["max_abs"], ratio))
        if not gs.within_bounds(es):  # (a)
            failures.append((key, "float64 bounds", es))
        if not es["max_abs"] <= CHM_ERR_FACTOR * es_tap["max_abs"] + ulp:  # (b)
            failures.append((key, "error vs tap-major", es["max_abs"], es_tap["max_abs"]))
        if c["stats"]:
            serr = _check_stats(c, torch.from_numpy(child_arr(chm_child, key + "|st")), ref_st)
            if not serr < gs.STATS_TOL:
                failures.append((key, "statistics", serr))
        if not chm_want and not torch.equal(got, tap):  # the fallback IS the tap-major kernel
            failures.append((key, "tap-major fallback differs from the parent's tap-major run"))
        # (c) across tiles at equal split and depth: the first tile of the list with this depth is the anchor
        a_tile = next(t for t, b in gs.CHM_TILES if gs.effective_bk(t, b) == bk)
        a_bk32 = next(b for t, b in gs.CHM_TILES if gs.effective_bk(t, b) == bk)
        akey = "%s|%s|y" % (c["name"], gs.config_id((a_tile, a_bk32, split)))
        if akey in chm_child.files and not torch.equal(got, torch.from_numpy(chm_child[akey])):
            failures.append((key, "not bit-identical to tile %d" % a_tile))
    assert not failures, failures


def child_arr(npz, key):
    assert key in npz.files, "the child process did not write %s" % key
    return npz[key]


@pytest.mark.parametrize("tile", gs.GROUP_TILES, ids=["t%d" % t for t in gs.GROUP_TILES])
def test_grouped_tile_walk(engine, report, group_child, tile):
    """The walk only permutes which workgroup computes which tile: bit-identical to this process's row-major run."""
    failures = []
    for c in gs.group_battery(tile):
        rb = child_arr(group_child, c["name"] + "|rb").tolist()
        assert tuple(rb[:3]) == (tile, 64, 1) and rb[4] == gs.GROUP_SIZE, (c["name"], rb)
        o = gs.operands(c, r16)
        here, _, rb_here = _ops.run_conv_case(engine, c, o, tile)
        assert rb_here["tile"] == tile and rb_here["tile_group"] == 0, rb_here
        es = gs.err_stats(here, gs.reference(c, o)[0])
        if not gs.within_bounds(es):
            failures.append((c["name"], "float64 bounds", es))
        same = torch.equal(torch.from_numpy(child_arr(group_child, c["name"] + "|y")), here)
        report.add("gemm_group/" + c["name"], bit_identical=same, rel_to_max=es["rel_to_max"], mean_rel=es["mean_rel"])
        if not same:
            failures.append((c["name"], "grouped walk differs from the row-major walk"))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ Inception forms, channel-major
@pytest.fixture(scope="module")
def inception_chm_child(tmp_path_factory, engine, chm_child, group_child):  # after the two others, one child at a time
    return _run_child("inception_chm", {"CYCLEDIFF_KORDER": "2"}, tmp_path_factory.mktemp("gemm_inception_chm"), 600)


@pytest.mark.parametrize("name", ir.CONV_CHM)
def test_inception_forms_channel_major(engine, report, inception_chm_child, name):
    """test_channel_major_order's acceptance on the BasicConv2d forms (tests/_inception_ops_ref.py): chm == 1 in the read-back,
    the float64 bounds, max|err| at most CHM_ERR_FACTOR x the tap-major run's + one fp32 ulp of max|ref|; and nothing written
    outside the slice."""
    fmt = ir.lib_fmt()
    c = ir.CONV[name]
    o = ir.conv_operands(c, fmt)
    run = _ops.basic_conv(engine, o["x"], o["w"], o["gamma"], o["beta"], o["mean"], o["var"], stride=c["stride"], pad=c["pad"],
                          in_ld=c["in_ld"], out_off=c["off"], out_ld=c["ld"], tile=gs.ANCHOR_TILE)
    assert run[3]["chm"] == 0 and run[3]["tile"] == gs.ANCHOR_TILE, run[3]
    fails_tap, fig_tap = ir.check_basic_conv(c, o, run[0], run[1], run[2], fmt)
    assert not fails_tap, fails_tap
    failures = []
    for tile in ir.CONV_TILES:
        key = "%s|tile%d" % (name, tile)
        buf, wp, bo = (torch.from_numpy(child_arr(inception_chm_child, key + s)) for s in ("|y", "|w", "|b"))
        rb = child_arr(inception_chm_child, key + "|rb").tolist()  # tile, bk, split, chm, tile_group
        assert rb[3] == 1 and rb[4] == 0 and (tile == 0 or rb[0] == tile), (key, rb)
        assert torch.equal(wp, run[1]) and torch.equal(bo, run[2]), key  # the same fold in both processes
        fails, fig = ir.check_basic_conv(c, o, buf, wp, bo, fmt)
        failures += [(key,) + f for f in fails]
        if "max_abs" not in fig:
            continue
        ref_max = float(ir.conv_ref(c, o, wp, bo)[0].abs().max())
        ulp = float(np.spacing(np.float32(ref_max)))
        ratio = fig["max_abs"] / max(fig_tap["max_abs"], 1e-30)
        report.add("inception_ops/chm/" + key, tile_ran=rb[0], bk=rb[1], rel_to_max=fig["rel_to_max"], mean_rel=fig["mean_rel"],
                   max_abs=fig["max_abs"], max_abs_tap_major=fig_tap["max_abs"], ratio=ratio, chm=rb[3])
        print("%-40s chm %d tile %2d max_abs %.3e tap-major %.3e ratio %.3f" % (key, rb[3], rb[0], fig["max_abs"],
                                                                                fig_tap["max_abs"], ratio))
        if not fig["max_abs"] <= CHM_ERR_FACTOR * fig_tap["max_abs"] + ulp:
            failures.append((key, "error vs tap-major", fig["max_abs"], fig_tap["max_abs"]))
    assert not failures, failures
