"""Recorder behind tests/test_engine_translate_args_host.py: calls Engine.cycle_translate / cycle_translate_masked /
cycle_translate_ctrl / ddim_decode_masked on a stand-in library and writes down which C symbol each reaches and with which
argument list. Integers, c_float and c_uint64 are recorded by value; a pointer as None, as the name of the input tensor it
points at, as "out:<i>" for the i-th returned tensor, or - a host table - as the sha1 of the table's bytes.
The fixture dates from the time when the coupled loop had one entry point per feature, each with a positional list. The one
cd_cycle_translate(h, &args) of today is recorded in that form: the stand-in names the form from the option pointers that are
set (FORMS) and flattens the struct back to that form's positional list through its field-order table.
`python tests/_engine_translate_args.py --write` regenerates tests/golden/engine_translate_args.json."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cycle_diffusion_amd import _ffi, schedule  # noqa: E402
from cycle_diffusion_amd.engine import Engine  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_translate_args.json")
SYMBOLS = ("cd_cycle_translate", "cd_cycle_translate_masked", "cd_cycle_translate_ctrl", "cd_ddim_decode_masked")
# the positional lists of the former entry points as (struct, field) rows; "z_out", "x_out" close each of them
_BASE = [("", f) for f in ("net sched_kind x0 enc_ctx_c enc_ctx_uc enc_guidance dec_ctx_c dec_ctx_uc dec_guidance "
                           "dec_guidance_per_sample ctx_len B n_dec K coef_enc_host coef_dec_host noise seed "
                           "last_uses_x0").split()]
_MASK = [("mask", f) for f in "mask x0 B_mask source qsample_coef_host noise seed".split()]
_CTRL = [("ctrl", f) for f in "mapper alpha weight B_ctrl n_ctrl".split()]
_OUT = [("", "z_out"), ("", "x_out")]
FORMS = {"cd_cycle_translate": _BASE + _OUT, "cd_cycle_translate_masked": _BASE + _MASK + _OUT,
         "cd_cycle_translate_ctrl": _BASE + _MASK + _CTRL + _OUT}


def flatten(h, args):
    """(former symbol, its positional arguments) of one cd_cycle_translate(h, byref(args)) call; an absent option struct
    flattens to the zeros / NULLs the positional form passed in its place"""
    a = args._obj
    assert isinstance(a, _ffi.TranslateArgs) and a.size == C.sizeof(_ffi.TranslateArgs)
    assert not a.blend and not a.sega, "the fixture has no such form"
    sym = "cd_cycle_translate_ctrl" if a.ctrl else "cd_cycle_translate_masked" if a.mask else "cd_cycle_translate"
    out = [h]
    for opt, field in FORMS[sym]:
        p = getattr(a, opt) if opt else None
        st = a if not opt else p.contents if p else type(p)._type_()
        v, ctype = getattr(st, field), dict(type(st)._fields_)[field]
        out.append(v if ctype is C.c_int else None if ctype is C.c_void_p and v is None else ctype(v))
    return sym, tuple(out)


B, CH, HW, L, DC, K = 2, 4, 2, 3, 5, 3


class RecordingLib:
    def __init__(self):
        self.calls = []
        self.cd_ddim_decode_masked = lambda *a: self.calls.append(("cd_ddim_decode_masked", a)) or 0
        self.cd_cycle_translate = lambda h, args: self.calls.append(flatten(h, args)) or 0


class HostEngine(Engine):
    def _f32(self, t):  # the engine's own, without the is_cuda assertion
        assert t.dtype == torch.float32
        return t.contiguous()


def make_engine():
    eng = object.__new__(HostEngine)
    eng.lib, eng.h, eng._keep = RecordingLib(), 0, None
    return eng


def t(*shape, base=0):
    n = int(np.prod(shape))
    return ((torch.arange(n) * 7 + base) % 64).float().reshape(shape) / 64


def flat_tensors(v):
    if isinstance(v, torch.Tensor):
        return [v]
    if isinstance(v, (list, tuple)):
        return sum((flat_tensors(u) for u in v), [])
    return []


def operands(n_dec=1):
    """every tensor and table a call may take, by argument name"""
    sch = schedule.DDIMSchedule(schedule.latent_alphas_cumprod(1000, 0.00085, 0.0120), 6, 0.1)
    skip = len(sch) - K
    return dict(
        x0=t(B, CH, HW, HW), z=t(n_dec * B, K + 1, CH, HW, HW, base=1), coef_enc=sch.coef_encode(skip),
        coef_dec=sch.coef_decode(skip), qcoef=sch.coef_qsample(skip), enc_ctx_c=t(B, L, DC, base=2), enc_ctx_uc=t(B, L, DC, base=3),
        dec_ctx_c=t(n_dec * B, L, DC, base=4), dec_ctx_uc=t(n_dec * B, L, DC, base=5), noise=t(K, B, CH, HW, HW, base=6),
        mask=t(1, 1, HW, HW, base=7), mask_x0=t(1, CH, HW, HW, base=8), mask_noise=t(K, n_dec * B, CH, HW, HW, base=9),
        mapper=t(1, L, L, base=10), alpha=t(1, L, base=11), weight=t(1, L, base=12), noise_tail=t(1, n_dec * B, CH, HW, HW, base=13),
        gvec=torch.tensor([1.5 + i for i in range(n_dec * B)]))


def _coupled(method, n_dec, guidance, masked=None, ctrl=False, drop=(), **over):
    """a thunk (engine, operands) -> result of one coupled call in the positional form the tests and the wrapper use"""
    def call(eng, op):
        op = dict(op, **over)
        pos = [3, _ffi.CD_SCHED_DDIM, op["x0"], op["coef_enc"], op["coef_dec"]]
        kw = dict(enc_ctx_c=op["enc_ctx_c"], enc_ctx_uc=op["enc_ctx_uc"], enc_guidance=2.0, dec_ctx_c=op["dec_ctx_c"],
                  dec_ctx_uc=op["dec_ctx_uc"], dec_guidance=op["gvec"] if guidance == "vector" else guidance, n_dec=n_dec,
                  noise=op["noise"], seed=11, last_uses_x0=True)
        if masked:
            mk = dict(mask_source=masked, mask_seed=5)
            if masked == "q_sample":
                mk.update(mask_x0=op["mask_x0"], qcoef=op["qcoef"], mask_noise=op["mask_noise"])
            if ctrl:
                kw.update(mask=op["mask"], **mk)
            else:
                pos.append(op["mask"])
                kw.update(mk)
        if ctrl:
            pos[5:5] = [op["mapper"], op["alpha"], op["weight"], 2]
        for k in drop:
            kw[k] = None
        return getattr(eng, method)(*pos, **kw)
    return n_dec, call


def _decode(guidance, drop=(), **over):
    def call(eng, op):
        op = dict(op, **over)
        kw = dict(mask_noise=op["mask_noise"], mask_seed=5, ctx_c=op["dec_ctx_c"], ctx_uc=op["dec_ctx_uc"],
                  guidance=op["gvec"] if guidance == "vector" else guidance, noise_tail=op["noise_tail"], seed=11)
        kw.update({k: over[k] for k in ("mask_source", "n_eps") if k in over})
        for k in drop:
            kw[k] = None
        return eng.ddim_decode_masked(3, _ffi.CD_SCHED_DDIM, op["z"], op["coef_dec"], op["mask"], op["mask_x0"], op["qcoef"], **kw)
    return 1, call


def _encoder_with_qcoef(eng, op):
    return eng.cycle_translate_masked(3, _ffi.CD_SCHED_DDIM, op["x0"], op["coef_enc"], op["coef_dec"], op["mask"], qcoef=op["qcoef"],
                                      mask_source="encoder", dec_ctx_c=op["dec_ctx_c"], dec_guidance=1.0)


CASES = {
    "plain-scalar": _coupled("cycle_translate", 1, 3.0),
    "plain-unguided-no_uc-no_noise": _coupled("cycle_translate", 1, 1.0, drop=("enc_ctx_uc", "dec_ctx_uc", "noise")),
    "plain-vector-n_dec2": _coupled("cycle_translate", 2, "vector"),
    "masked-q_sample-scalar": _coupled("cycle_translate_masked", 1, 3.0, masked="q_sample"),
    "masked-q_sample-vector-n_dec2-seeded": _coupled("cycle_translate_masked", 2, "vector", masked="q_sample", drop=("mask_noise",)),
    "masked-encoder-n_dec2": _coupled("cycle_translate_masked", 2, 3.0, masked="encoder"),
    "ctrl-scalar": _coupled("cycle_translate_ctrl", 1, 3.0, ctrl=True),
    "ctrl-q_sample-vector-n_dec2": _coupled("cycle_translate_ctrl", 2, "vector", masked="q_sample", ctrl=True),
    "ctrl-encoder": _coupled("cycle_translate_ctrl", 1, 3.0, masked="encoder", ctrl=True),
    "decode-scalar": _decode(3.0),
    "decode-vector-seeded-n_eps": _decode("vector", drop=("mask_noise", "noise_tail"), n_eps=K),
    # the ValueErrors
    "plain-vector-holds-1": _coupled("cycle_translate", 1, "vector", gvec=torch.tensor([2.0, 1.0])),
    "plain-vector-short": _coupled("cycle_translate", 2, "vector", gvec=torch.tensor([2.0, 3.0])),
    "masked-vector-holds-1": _coupled("cycle_translate_masked", 1, "vector", masked="q_sample", gvec=torch.tensor([2.0, 1.0])),
    "ctrl-vector-holds-0": _coupled("cycle_translate_ctrl", 1, "vector", ctrl=True, gvec=torch.tensor([0.0, 2.0])),
    "decode-vector-holds-1": _decode("vector", gvec=torch.tensor([2.0, 1.0])),
    "decode-vector-long": _decode("vector", gvec=torch.tensor([2.0, 3.0, 4.0])),
    "masked-mask-shape": _coupled("cycle_translate_masked", 1, 3.0, masked="q_sample", mask=t(1, 1, HW, HW + 1)),
    "ctrl-mask-shape": _coupled("cycle_translate_ctrl", 1, 3.0, masked="q_sample", ctrl=True, mask=t(B + 1, 1, HW, HW)),
    "masked-mask_noise-shape": _coupled("cycle_translate_masked", 2, 3.0, masked="q_sample", mask_noise=t(K, B, CH, HW, HW)),
    "masked-mask_source-unknown": _coupled("cycle_translate_masked", 1, 3.0, masked="pixels"),
    "ctrl-control-shape": _coupled("cycle_translate_ctrl", 1, 3.0, ctrl=True, alpha=t(1, L + 1)),
    "masked-encoder-qcoef": (1, _encoder_with_qcoef),
    "decode-encoder": _decode(3.0, mask_source="encoder"),
    # a mask check comes ahead of the guidance check, the control check between them
    "masked-mask-shape-and-vector-holds-1": _coupled("cycle_translate_masked", 1, "vector", masked="q_sample",
                                                     mask=t(1, 1, HW + 1, HW), gvec=torch.tensor([2.0, 1.0])),
    "ctrl-control-shape-and-vector-holds-1": _coupled("cycle_translate_ctrl", 1, "vector", ctrl=True, weight=t(1, L + 1),
                                                      gvec=torch.tensor([2.0, 1.0])),
}


def run_case(n_dec, call):
    """-> (record for the fixture, tensors whose pointer went to the library and that the method must keep alive)"""
    eng, op = make_engine(), operands(n_dec)
    try:
        out = call(eng, op)
    except ValueError as e:
        assert not eng.lib.calls
        return {"error": "ValueError: %s" % e}, None
    (sym, args), = eng.lib.calls
    out = list(out) if isinstance(out, tuple) else [out]
    names = {v.data_ptr(): k for k, v in op.items() if isinstance(v, torch.Tensor)}
    names.update({v.data_ptr(): "out:%d" % i for i, v in enumerate(out)})
    tables = {v.ctypes.data: hashlib.sha1(v.tobytes()).hexdigest() for v in op.values() if isinstance(v, np.ndarray)}
    rec, passed = [], []
    for a in args:
        if isinstance(a, C.c_void_p):
            assert a.value is None or a.value in names or a.value in tables, "a pointer to nothing the caller handed over"
            rec.append(None if a.value is None else names.get(a.value) or "table:" + tables[a.value])
            if a.value in names and not names[a.value].startswith("out:"):
                passed.append(names[a.value])
        elif isinstance(a, (C.c_float, C.c_uint64)):
            rec.append([type(a).__name__, a.value])
        else:
            assert a is None or isinstance(a, int), type(a)
            rec.append(a)
    kept = {v.data_ptr() for v in flat_tensors(eng._keep)}
    held = [k for k in passed if op[k].data_ptr() in kept]
    return {"symbol": sym, "args": rec, "out": [list(v.shape) for v in out]}, (passed, held)


def record():
    return {name: run_case(*c)[0] for name, c in CASES.items()}


if __name__ == "__main__":
    rec = record()
    if "--write" in sys.argv:
        with open(FIXTURE, "w") as f:
            f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(rec[k], sort_keys=True)) for k in rec) + "\n}\n")
    for k, v in rec.items():
        print(k, v.get("error") or v["symbol"])
