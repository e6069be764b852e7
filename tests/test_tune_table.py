"""The shipped tile table (cycle-diffusion_amd/tune_gfx950.txt) and the tool that maintains it.

Every line is a 14-integer GEMM shape key + the chosen configuration: tile id in the low byte, split-K factor in
bits 8-15, bit 16 = the 32-deep K-step variant. The ids must exist in csrc/conv_gemm.hip's kCfgs, keys must be unique
(the engine's std::map would silently keep one), and split factors / BK = 32 flags must be ones the launcher accepts -
a bad entry only shows up on the GPU as a CD_CHECK failure in the middle of a sampler call."""
import os
import subprocess
import sys

import _gemm_sweep as gs
from _gemm_sweep import ROOT, cfg_ids as _cfg_ids, table_rows as _rows


def test_table_entries_are_valid_configurations():
    ids, bk64_only = _cfg_ids()
    assert len(ids) >= 23 and 20 in ids and ids[20] == 320
    rows = _rows()
    assert len(rows) > 600
    keys = set()
    for r in rows:
        key, val = tuple(r[:14]), r[14]
        assert key not in keys, "duplicate shape key %s" % (key,)
        keys.add(key)
        tile, split, bk32 = val & 0xff, (val >> 8) & 0xff, (val >> 16) & 1
        M, N, K, KH, C0, C1 = key[:6]
        if tile == 30:  # the streaming K = 320 linear kernel (csrc/lin_stream.hip): only where it is defined
            assert val == 30 and K == 320 and KH == 1 and C0 == 320 and C1 == 0, (key, val)
            assert key[6] == 1 and key[7] == 0 and key[9] == 1 and key[10] == 0, (key, val)  # stride, up, nbatch, f32
            assert N % 64 == 0 and 320 <= N <= 2560 and M % 32 == 0 and key[8] in (0, 3) and not key[13] & 2, (key, val)
            continue
        assert tile in ids, (key, val)
        assert val >> 17 == 0 and 0 <= split <= 16, (key, val)
        assert K == KH * KH * (C0 + C1) or KH == 1, key
        assert C0 % 32 == 0 and C1 % 32 == 0, key
        if tile in bk64_only:  # 320-wide tiles: 64-deep K steps only, channel counts multiples of 64
            assert not bk32 and C0 % 64 == 0 and C1 % 64 == 0, (key, val)
        if bk32:
            assert split <= 1, (key, val)  # the tuner never combines the BK = 32 variants with split-K
        if key[8] == 3:  # GEGLU epilogue: value and gate halves meet in one 64-column chunk
            assert N % 64 == 0, key


def test_merge_tune_overrides_and_keeps_order(tmp_path):
    a, b, out = tmp_path / "a.txt", tmp_path / "b.txt", tmp_path / "o.txt"
    k1 = "1 2 3 1 32 0 1 0 0 1 0 8 8 0"
    k2 = "4 5 6 1 64 0 1 0 0 1 0 8 8 1"
    k3 = "7 8 9 3 64 0 1 0 0 1 0 8 8 0"
    a.write_text("%s 2\n%s 20\n" % (k1, k2))
    b.write_text("%s 276\nnot a table line\n%s 5\n" % (k2, k3))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "merge_tune.py"), str(a), str(b), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_text().splitlines() == [k1 + " 2", k2 + " 276", k3 + " 5"]


# ---- the GPU configuration sweep (tests/test_gpu_gemm_configs.py) covers what the kernel and the table can select
def _sweep_params():
    """the configurations test_gemm_configuration is parametrised over, read from its parametrize mark (importing the GPU
    module needs no GPU)"""
    import test_gpu_gemm_configs as m
    marks = [k for k in m.test_gemm_configuration.pytestmark if k.name == "parametrize"]
    assert len(marks) == 1 and marks[0].args[0] == "cfg"
    return list(marks[0].args[1])


def test_gpu_sweep_covers_every_tile_and_table_triple():
    cfgs = set(_sweep_params())
    ids, bk64_only = _cfg_ids()
    for t in ids:
        assert (t, 0, 1) in cfgs, "tile %d has no case in the GPU sweep" % t
        if t not in bk64_only and t not in gs.always_bk32():
            assert (t, 1, 1) in cfgs, "tile %d | 1 << 16 has no case in the GPU sweep" % t
    for r in _rows():
        val = r[14]
        tile, split, bk32 = val & 0xff, (val >> 8) & 0xff, (val >> 16) & 1
        if tile != gs.LIN_STREAM_TILE:
            assert (tile, bk32, max(split, 1)) in cfgs, "table row %s has no case in the GPU sweep" % (r,)
    # every configuration's battery can be built and asks for something the launcher accepts
    for cfg in cfgs:
        BM, BN, BK, stages = gs.geometry(cfg)
        names = [c["name"] for c in gs.battery(cfg)]
        assert len(set(names)) == len(names)
        for c in gs.battery(cfg):
            assert c["C0"] % BK == 0 and c["C1"] % BK == 0, c
            assert not c["stats"] or (gs.out_hw(c)[0] * gs.out_hw(c)[1]) % 32 == 0, c
        nks = {c["C0"] // BK for c in gs.battery(cfg) if "/nk" in c["name"]}
        assert {1, stages - 1, stages, stages + 1} <= nks, (cfg, nks)
        if cfg[2] > 1:
            assert any("split_empty" in c["name"] and c["C0"] // BK < cfg[2] for c in gs.battery(cfg))
    # the batteries of the two child processes can be built; their families exist
    for t in gs.GROUP_TILES:
        assert len(gs.group_battery(t)) == 12
    for c, split, chm in gs.chm_battery() + [gs.CHM_BK32_ONLY]:
        assert (chm == 1) == (1 < c["k"] <= 8 and not c["up"]), c
        assert not c["stats"] or (gs.out_hw(c)[0] * gs.out_hw(c)[1]) % 32 == 0, c
    assert {t for t, _ in gs.CHM_TILES} <= set(ids) and set(gs.GROUP_TILES) <= set(ids)


def test_launched_instantiations_match_dispatch():
    """The sweep sizes its shapes from the instantiation a request launches: the parsed kCfgs names, the BK = 32 aliases and
    the one-depth ids must agree with the launch_cfg<...> lines of dispatch<BK>."""
    tab, inst, alias = gs.cfg_table(), gs.dispatch_instantiations(), gs.bk32_alias()
    assert gs.always_bk32() == {24, 25} and set(alias) == {9, 13, 18, 19}
    for t, c in tab.items():
        own = 32 if t in gs.always_bk32() else 64
        assert inst[(t, own)] == (c["BM"], c["BN"], own, c["WM"], c["WN"], c["stages"]), (t, inst[(t, own)], c)
        assert c["TN"] == c["BN"] // c["WN"], (t, c)
        if t in gs.bk64_only() or t in gs.always_bk32():
            continue
        if t in alias:  # the 32-deep branch of this id is literally the alias target's instantiation
            assert inst[(t, 32)] == inst[(alias[t], 32)], (t, alias[t])
            a = tab[alias[t]]
            assert inst[(t, 32)][:2] + inst[(t, 32)][3:] == (a["BM"], a["BN"], a["WM"], a["WN"], a["stages"])
        elif t == 22:  # 256 x 256 with 32-deep steps has a 4-deep ring of its own
            assert inst[(22, 32)] == (256, 256, 32, 4, 2, 4)
        else:
            assert inst[(t, 32)] == (c["BM"], c["BN"], 32, c["WM"], c["WN"], c["stages"]), t


def test_reference_rejects_a_dropped_tap_and_a_shifted_concat_source():
    """The float64 reference helper with one filter tap zeroed, or with the second concat source read one column off, must
    violate the sweep's bounds (5e-3 / 2e-3) on the battery's shapes: the bounds have teeth for the bugs the sweep is for.
    Hardest case: 5 x 5 (one of 25 taps), 192 = 128 + 64 channels, 10 x 10."""
    import torch
    r16 = lambda t: t.to(torch.float16).float()
    hard = gs._case("x/5x5_concat", 1, 128, 10, 10, 64, 5, C1=64)
    cases = [hard] + [c for c in gs.battery((14, 0, 1)) + gs.battery((15, 1, 1)) + [x[0] for x in gs.chm_battery()]
                      if c["k"] > 1 or c["C1"]]
    assert len(cases) > 20
    for c in cases:
        o = gs.operands(c, r16)
        ref, _ = gs.reference(c, o)
        assert gs.within_bounds(gs.err_stats(ref, ref))
        if c["k"] > 1:
            for tap in ((0, 0), (c["k"] // 2, c["k"] // 2), (c["k"] - 1, c["k"] - 1)):
                es = gs.err_stats(gs.reference(c, o, zero_tap=tap)[0], ref)
                assert es["rel_to_max"] > 4 * gs.REL_TOL and es["mean_rel"] > 4 * gs.MEAN_TOL, (c["name"], tap, es)
        if c["C1"]:
            es = gs.err_stats(gs.reference(c, o, shift_x1=1)[0], ref)
            assert es["rel_to_max"] > 4 * gs.REL_TOL and es["mean_rel"] > 4 * gs.MEAN_TOL, (c["name"], es)
    es = gs.err_stats(gs.reference(hard, gs.operands(hard, r16), zero_tap=(2, 2))[0], gs.reference(hard, gs.operands(hard, r16))[0])
    assert es["rel_to_max"] > 0.1 and es["mean_rel"] > 0.1, es
