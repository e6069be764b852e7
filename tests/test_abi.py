"""CPU: the C-ABI shared library builds, loads, and exports every symbol include/cyclediff.h declares
(no compute calls without a GPU); the product refuses to run without a HIP device."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    txt = open(os.path.join(ROOT, "include", "cyclediff.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cd_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    from cycle_diffusion_amd import _ffi
    lib = _ffi.load_library()
    syms = _header_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(lib, s), s
    # the ctypes signature table covers exactly the header
    assert sorted(_ffi.SIGNATURES.keys()) == syms
    assert lib.cd_version() >= 100


def _translate_structs():
    """C struct name -> ctypes class, for cd_translate_args and its option structs"""
    from cycle_diffusion_amd import _ffi
    return {"cd_keep_mask": _ffi.KeepMask, "cd_attn_ctrl": _ffi.AttnCtrl, "cd_local_blend": _ffi.LocalBlend,
            "cd_sega": _ffi.Sega, "cd_translate_args": _ffi.TranslateArgs}


def _header_fields(struct):
    """[(field name, ctypes type)] of `typedef struct <struct> { ... }` as the header declares it"""
    import ctypes as C
    txt = open(os.path.join(ROOT, "include", "cyclediff.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (struct, struct), txt, flags=re.S).group(1)
    scalars = {"int": C.c_int, "float": C.c_float, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, star, name = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)", decl).groups()
        if not star:
            fields.append((name, scalars[ctype]))
        elif ctype in _translate_structs():  # an option struct
            fields.append((name, C.POINTER(_translate_structs()[ctype])))
        else:  # device tensors and host tables cross as untyped addresses
            assert ctype in ("float", "int32_t", "cd_step_coef", "cd_sega_concept"), decl
            fields.append((name, C.c_void_p))
    return fields


def test_struct_layouts_match_the_header(tmp_path):
    import ctypes as C
    import subprocess
    from cycle_diffusion_amd import _ffi
    assert C.sizeof(_ffi.StepCoef) == 32 and _ffi.STEP_COEF_DTYPE.itemsize == 32
    assert C.sizeof(_ffi.NetDesc) == 4 * (6 + 1 + 8 + 1 + 8 + 2 + 3 + 3 + 3 + 8)
    # the argument structs of cd_cycle_translate: first, the ctypes fields are the header's in name, order and type
    structs = _translate_structs()
    for cname, cls in structs.items():
        assert list(cls._fields_) == _header_fields(cname), cname
    # second, the host compiler lays them out as ctypes does: sizeof and every offsetof, printed by a C program
    lines = ['#include <stdio.h>', '#include "cyclediff.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f) for f, _ in cls._fields_]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    cc = os.environ.get("CC") or "cc"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    want = {}
    for cname, cls in structs.items():
        want[cname] = str(C.sizeof(cls))
        want.update({"%s.%s" % (cname, f): str(getattr(cls, f).offset) for f, _ in cls._fields_})
    assert got == want


def test_no_cpu_fallback():
    import torch
    import cycle_diffusion_amd as cda
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(Exception) as e:
        cda.Engine("cuda:0")
    assert "no CPU fallback" in str(e.value)
    # and the C entry point itself fails loudly
    import ctypes as C
    from cycle_diffusion_amd import _ffi
    lib = _ffi.load_library()
    h = C.c_void_p()
    assert lib.cd_engine_create(None, C.c_size_t(1 << 28), C.byref(h)) != 0
    assert b"no CPU fallback" in lib.cd_last_error()
