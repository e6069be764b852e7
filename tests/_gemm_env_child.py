"""Child process of tests/test_gpu_gemm_configs.py (not collected): the launcher reads CYCLEDIFF_KORDER, CYCLEDIFF_TILE_GROUP and
CYCLEDIFF_TILE_GROUP_MIN_N once per process, so the channel-major K order and the grouped tile walk need a process of their own.

    python _gemm_env_child.py chm|group|inception_chm OUT.npz

runs the named battery of tests/_gemm_sweep.py through tests/_ops.py and writes every output ("<key>|y"), its GroupNorm
statistics ("<key>|st") and the launcher's read-back ("<key>|rb" = tile, bk, split, chm, tile_group) to OUT.npz. It checks
nothing: the parent does, against float64 and against its own runs of the same cases. The inception_chm battery runs the
BasicConv2d forms of tests/_inception_ops_ref.py (CONV_CHM) through cd_op_basic_conv and writes the whole output buffer
("<key>|y"), the packed weights and bias the launch read ("<key>|w", "<key>|b") and the read-back."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import _gemm_sweep as gs  # noqa: E402
import _ops  # noqa: E402


def main(battery, out_path):
    import cycle_diffusion_amd as cda
    eng = cda.Engine("cuda:0")
    out = {}

    def run(key, c, tile):
        o = gs.operands(c, _ops.bf16_round)
        y, st, rb = _ops.run_conv_case(eng, c, o, tile)
        out[key + "|y"] = y.numpy()
        if st is not None:
            out[key + "|st"] = st.numpy()
        out[key + "|rb"] = np.array([rb[k] for k in ("tile", "bk", "split", "chm", "tile_group")], dtype=np.int32)

    if battery == "chm":
        assert os.environ.get("CYCLEDIFF_KORDER") == "2"
        for tile, bk32 in gs.CHM_TILES:
            for c, split, _ in gs.chm_battery() + ([gs.CHM_BK32_ONLY] if bk32 else []):
                cfg = (tile, bk32, split)
                run("%s|%s" % (c["name"], gs.config_id(cfg)), c, gs.tile_arg(cfg))
    elif battery == "group":
        assert os.environ.get("CYCLEDIFF_TILE_GROUP") == str(gs.GROUP_SIZE)
        for tile in gs.GROUP_TILES:
            for c in gs.group_battery(tile):
                run(c["name"], c, tile)
    elif battery == "inception_chm":
        import _inception_ops_ref as ir
        assert os.environ.get("CYCLEDIFF_KORDER") == "2"
        fmt = ir.lib_fmt()
        for name in ir.CONV_CHM:
            c = ir.CONV[name]
            o = ir.conv_operands(c, fmt)
            for tile in ir.CONV_TILES:
                buf, wp, bo, rb = _ops.basic_conv(eng, o["x"], o["w"], o["gamma"], o["beta"], o["mean"], o["var"],
                                                  stride=c["stride"], pad=c["pad"], in_ld=c["in_ld"], out_off=c["off"],
                                                  out_ld=c["ld"], tile=tile)
                key = "%s|tile%d" % (name, tile)
                out[key + "|y"], out[key + "|w"], out[key + "|b"] = buf.numpy(), wp.numpy(), bo.numpy()
                out[key + "|rb"] = np.array([rb[k] for k in ("tile", "bk", "split", "chm", "tile_group")], dtype=np.int32)
    else:
        raise SystemExit("unknown battery %r" % battery)
    eng.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
