"""CPU: the fused windows without a GPU - the window grid, its refusals, the restatement of the two kernels and
of the windowed coupled loop (tests/_windows_ref.py), the marshalling of the new cd_translate_args fields, the (H, W) loader."""
import ctypes as C

import numpy as np
import pytest
import torch

import _attn_control_ref as acr
import _engine_translate_args as ea
import _windows_ref as wr
import golden_util as gu
from cycle_diffusion_amd import _ffi, windows
from cycle_diffusion_amd.data import triplets

S = wr.S


@pytest.mark.parametrize("L,size,stride,want", [(16, 16, 8, [0]), (24, 16, 8, [0, 8]), (28, 16, 5, [0, 5, 10, 12]),
                                                 (96, 64, 32, [0, 32]), (128, 64, 32, [0, 32, 64])])
def test_window_offsets(L, size, stride, want):
    assert windows.window_offsets(L, size, stride) == want


def test_window_grid_is_row_major_and_covers_every_cell():
    g = windows.window_grid(24, 28, 16, 8)
    assert g.dtype == np.int32 and g.shape == (6, 2)
    assert g.tolist() == [[0, 0], [0, 8], [0, 12], [8, 0], [8, 8], [8, 12]]
    for Hc, Wc, stride in wr.CANVASES + [(16, 16, 8), (64, 96, 32), (64, 128, 32), (80, 100, 32)]:
        win = windows.window_grid(Hc, Wc, 16 if Hc < 64 else 64, stride)
        size = 16 if Hc < 64 else 64
        cov = windows.coverage(win, Hc, Wc, size)
        assert cov.min() >= 1, (Hc, Wc, stride)
        assert (win[:, 0] + size <= Hc).all() and (win[:, 1] + size <= Wc).all() and (win >= 0).all()
        assert windows.check_grid(win, Hc, Wc, size) is not None
    assert [len(windows.window_grid(*c[:2], S, c[2])) for c in wr.CANVASES] == [wr.N_WINDOWS[c] for c in wr.CANVASES]
    assert windows.coverage(windows.window_grid(24, 24, S, 8), 24, 24, S).max() == 4
    assert windows.coverage(windows.window_grid(24, 24, S, 8), 24, 24, S)[0, 0] == 1
    assert windows.coverage(windows.window_grid(16, 28, S, 5), 16, 28, S).max() == 4
    assert 3 in windows.coverage(windows.window_grid(16, 28, S, 5), 16, 28, S)


def test_the_host_refusals_fire():
    with pytest.raises(ValueError, match="smaller"):
        windows.window_offsets(12, 16, 8)
    with pytest.raises(ValueError, match="positive"):
        windows.window_offsets(24, 16, 0)
    with pytest.raises(ValueError, match="gaps"):
        windows.window_grid(64, 64, 16, 24)
    with pytest.raises(ValueError, match="more than"):
        windows.window_grid(16, 16 + 65, 16, 1)
    ok = [[0, 0], [0, 8]]
    assert windows.check_grid(ok, 16, 24, 16).tolist() == ok
    with pytest.raises(ValueError, match="smaller"):
        windows.check_grid([[0, 0]], 8, 24, 16)
    with pytest.raises(ValueError, match="outside"):
        windows.check_grid([[0, 0], [0, 9]], 16, 24, 16)
    with pytest.raises(ValueError, match="outside"):
        windows.check_grid([[-1, 0], [0, 8]], 16, 24, 16)
    with pytest.raises(ValueError, match="equal"):
        windows.check_grid([[0, 0], [0, 8], [0, 0]], 16, 24, 16)
    with pytest.raises(ValueError, match="no window"):
        windows.check_grid([[0, 0], [0, 16]], 16, 33, 16)
    with pytest.raises(ValueError, match=r"\[n, 2\]"):
        windows.check_grid(np.zeros((65, 2)), 16, 24, 16)
    with pytest.raises(ValueError, match="window_stride"):
        windows.refuse(dict(window_stride=8), "DDIB")
    kw = dict(window_stride=0, other=1)
    windows.refuse(kw, "DDIB")
    assert kw == dict(other=1)


@pytest.mark.parametrize("canvas", wr.CANVASES, ids=lambda c: "%dx%d_s%d" % c)
@pytest.mark.parametrize("parts,ld", [(1, 4), (2, 4), (2, 6)])
def test_fuse_restatement_is_the_float64_mean(canvas, parts, ld):
    Hc, Wc, stride = canvas
    win = windows.window_grid(Hc, Wc, S, stride)
    Bp, Cc = 3, 4
    e = gu.rnd((parts * len(win) * Bp, S * S, ld), 91)
    got = wr.fuse_ref(e, win, Bp, Cc, Hc, Wc, S, parts)
    ref = wr.fuse_f64(e, win, Bp, Cc, Hc, Wc, S, parts)
    assert got.dtype == torch.float32 and got.shape == (parts * Bp, Cc, Hc, Wc)
    # at most 3 fp32 adds and one division, each half an ulp of a partial sum of at most 4 max|e|: 4 * 2^-24 * 4 max|e|
    assert (got.double() - ref).abs().max().item() <= 4 * 2.0 ** -24 * 4 * e.abs().max().item()
    # a cell with one covering window is that window's value, bit for bit, -0 included
    e[0, 0, 0] = -0.0
    one = wr.fuse_ref(e, win, Bp, Cc, Hc, Wc, S, parts)
    assert torch.equal(one[0, :, 0, 0], e[0, 0, :Cc]) and torch.signbit(one[0, 0, 0, 0])


def test_gather_restatement_layout():
    win = windows.window_grid(16, 28, S, 5)
    x = gu.rnd((2, 4, 16, 28), 5)
    y = wr.gather_ref(x, win, S, 32, 1, lambda t: t.half().float())
    assert y.shape == (2 * 4 * 2, S * S, 32)
    assert torch.equal(y[:8], y[8:]) and not y[:, :, 4:].any()
    w, b, py, px = 3, 1, 7, 11  # row w * Bp + b, pixel (py, px): x[b, :, y_w + py, x_w + px]
    assert torch.equal(y[w * 2 + b, py * S + px, :4], x[b, :, py, 12 + px].half().float())


def test_one_window_is_the_unwindowed_restatement():
    e = acr.E2E
    sd = gu.weights(gu.load("latent_cycle_tiny"))
    x0, c, uc, c2 = wr.canvas_inputs(16, 16)
    assert torch.equal(x0, acr.e2e_inputs()[0])
    noise = wr.canvas_noise(16, 16)
    z0, xd0 = acr.coupled_translate(sd, gu.TINY_SD_CFG, x0, c, c2, uc, e["dec_g"], e["S"], e["skip"], e["eta"], noise, None)
    z1, xd1 = wr.restatement(16, 16, 8)
    assert windows.window_grid(16, 16, S, 8).tolist() == [[0, 0]]
    assert torch.equal(torch.stack(z0, 1), z1) and torch.equal(xd0, xd1)


@pytest.mark.parametrize("canvas", wr.CANVASES, ids=lambda c: "%dx%d_s%d" % c)
def test_averaging_is_told_apart_from_first_window_wins(canvas):
    """what the GPU end-to-end bound (8e-3 of the maximum) must be able to see: a fuse that kept the first covering window
    instead of averaging moves x by at least 8e-2 of its maximum (measured 1.2e-1, 1.65e-1, 2.0e-1)"""
    _z, x_mean = wr.restatement(*canvas)
    _z, x_first = wr.restatement(*canvas, rule="first")
    rel = ((x_mean - x_first).abs().max() / x_mean.abs().max()).item()
    print("windows/first_vs_mean %s rel_to_max=%.3e" % (canvas, rel))
    assert torch.isfinite(x_mean).all() and rel >= 8e-2, rel


class _Lib:
    def __init__(self):
        self.seen = []

    def cd_cycle_translate(self, h, args):
        a = args._obj
        win = None
        if a.win_host:
            win = np.ctypeslib.as_array(C.cast(a.win_host, C.POINTER(C.c_int32)), shape=(a.n_win, 2)).copy()
        self.seen.append((a.size, a.canvas_h, a.canvas_w, a.n_win, a.win_host, win))
        return 0


def test_the_window_fields_are_marshalled():
    eng = ea.make_engine()
    eng.lib = _Lib()
    op = ea.operands(1)
    kw = dict(enc_ctx_c=op["enc_ctx_c"], dec_ctx_c=op["dec_ctx_c"], dec_guidance=1.0, noise=op["noise"])
    eng.cycle_translate(3, _ffi.CD_SCHED_DDIM, op["x0"], op["coef_enc"], op["coef_dec"], **kw)
    size, ch, cw, n, p, win = eng.lib.seen[-1]
    assert size == C.sizeof(_ffi.TranslateArgs) and (ch, cw, n, p, win) == (0, 0, 0, None, None)
    x0 = ea.t(ea.B, ea.CH, 3, 5)
    z, x = eng.cycle_translate(3, _ffi.CD_SCHED_DDIM, x0, op["coef_enc"], op["coef_dec"], windows=[[0, 0], [1, 3], [0, 2]],
                               enc_ctx_c=op["enc_ctx_c"], dec_ctx_c=op["dec_ctx_c"], dec_guidance=1.0)
    size, ch, cw, n, p, win = eng.lib.seen[-1]
    assert (ch, cw, n) == (3, 5, 3) and win.tolist() == [[0, 0], [1, 3], [0, 2]]
    assert z.shape == (ea.B, ea.K + 1, ea.CH, 3, 5) and x.shape == (ea.B, ea.CH, 3, 5)
    assert any(isinstance(k, np.ndarray) and k.ctypes.data == p for k in eng._keep)  # the table outlives the call
    with pytest.raises(ValueError, match=r"\[n, 2\]"):
        eng.cycle_translate(3, _ffi.CD_SCHED_DDIM, x0, op["coef_enc"], op["coef_dec"], windows=[0, 0, 1, 3])
    # the struct ends with the four flat fields, in the header's order
    assert [f for f, _ in _ffi.TranslateArgs._fields_][-4:] == ["canvas_h", "canvas_w", "n_win", "win_host"]


def _synthetic(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 5) % 256, (yy * 7) % 256, (xx + 3 * yy) % 256], -1).astype(np.uint8)


@pytest.mark.parametrize("size,hw,box", [((41, 30), (20, 10), (13, 0, 28, 30)),   # too wide: the height stays, 15 columns
                                         ((30, 44), (10, 30), (0, 17, 30, 27)),   # too tall: the width stays, 10 rows
                                         ((36, 24), (16, 24), (0, 0, 36, 24))])   # the aspect already: a resize only
def test_the_rectangular_loader_crops_then_resizes(tmp_path, size, hw, box):
    from PIL import Image
    arr = _synthetic(*size)
    path = str(tmp_path / "img.png")
    Image.fromarray(arr).save(path)
    Image.fromarray(arr[:, :, 0]).save(str(tmp_path / "mask.png"))
    got = triplets.load_image(path, hw)
    assert got.shape == (3,) + hw and got.dtype == torch.float32
    want = Image.fromarray(arr).crop(box).resize((hw[1], hw[0]), Image.BILINEAR)
    assert torch.equal(got, torch.from_numpy(np.asarray(want, dtype=np.float32) / 255.0).permute(2, 0, 1))
    m = triplets.load_mask(str(tmp_path / "mask.png"), hw)
    assert m.shape == (1,) + hw and torch.equal(m[0], got[0])
    # the int form is the reference's square crop, and (R, R) is the same picture
    assert torch.equal(triplets.load_image(path, 12), triplets.load_image(path, (12, 12)))
    ds_item = triplets.TripletDataset.__new__(triplets.TripletDataset)
    ds_item.items, ds_item.resolution, ds_item.root = [(0, {"img_path": path})], hw, str(tmp_path)
    assert ds_item[0]["original_image"].shape == (3,) + hw
