"""Torch restatement of the fused windows on the coupled loop (include/cyclediff.h cd_translate_args.n_win):
  gather_ref / fuse_ref / fuse_f64   the two kernels on explicit tensors, and the fuse's float64 definition
  windowed_translate                 tests/_attn_control_ref.coupled_translate on a canvas: per step the windows of the
                                     encoder's and of the decoder's latent through the oracle network as more batch rows, the
                                     predictions fused per cell, then the unchanged step arithmetic on the canvas
The shapes every test shares: the tiny SD network (S = 16), B = 2, the E2E chain of _attn_control_ref (K = 20)."""
import functools

import numpy as np
import torch

import _attn_control_ref as acr
import golden_util as gu
from oracle import nets, samplers

S = 16
# (Hc, Wc, stride): the smallest overlap; a centre covered 4 times and corners once; a clamped last window and a count of 3
CANVASES = [(16, 24, 8), (24, 24, 8), (16, 28, 5)]
N_WINDOWS = {(16, 24, 8): 2, (24, 24, 8): 4, (16, 28, 5): 4}


def crop(x, win, S=S):
    """x [Bp, C, Hc, Wc] -> [n_win * Bp, C, S, S], window-major"""
    return torch.cat([x[:, :, y:y + S, xx:xx + S] for y, xx in np.asarray(win).tolist()], 0)


def gather_ref(x, win, S, cpad, dup, to16):
    """k_window_gather: [(1 + dup) * n_win * Bp, S * S, cpad] fp32 holding the 16-bit values; to16: the build's rounding"""
    rows = crop(x, win, S)                                    # [n_win * Bp, C, S, S]
    nhwc = rows.permute(0, 2, 3, 1).reshape(rows.shape[0], S * S, rows.shape[1])
    out = torch.zeros(rows.shape[0], S * S, cpad)
    out[:, :, :rows.shape[1]] = to16(nhwc)
    return out.repeat(1 + dup, 1, 1)


def _canvas_planes(e, win, Bp, C, S, parts):
    """e [parts * n_win * Bp, S * S, ld] -> per window [parts * Bp, C, S, S] (the first C channels), rows d * Bp + b"""
    n_win = len(win)
    e = e.reshape(parts, n_win, Bp, S, S, e.shape[-1])[..., :C]
    return [e[:, w].reshape(parts * Bp, S, S, C).permute(0, 3, 1, 2) for w in range(n_win)]


def fuse_ref(e, win, Bp, C, Hc, Wc, S=S, parts=1, rule="mean"):
    """k_window_fuse in fp32: acc = e_{w_first}, acc = acc + e_w over the covering windows in ascending w, out = acc /
    float32(count). acc is never zero-initialised: one covering window returns its value bit for bit. rule = "first": the
    first covering window wins (what the averaging is told apart from)."""
    planes = _canvas_planes(e.float(), win, Bp, C, S, parts)
    acc = torch.zeros(parts * Bp, C, Hc, Wc)
    cnt = torch.zeros(Hc, Wc, dtype=torch.int32)
    for (y, x), p in zip(np.asarray(win).tolist(), planes):
        first = (cnt[y:y + S, x:x + S] == 0)[None, None]
        reg = acc[:, :, y:y + S, x:x + S]
        acc[:, :, y:y + S, x:x + S] = torch.where(first, p, reg if rule == "first" else reg + p)
        cnt[y:y + S, x:x + S] += 1
    assert int(cnt.min()) >= 1
    return acc if rule == "first" else acc / cnt.float()[None, None]


def fuse_f64(e, win, Bp, C, Hc, Wc, S=S, parts=1):
    """the definition: the mean over the covering windows, in float64"""
    planes = _canvas_planes(e.double(), win, Bp, C, S, parts)
    acc = torch.zeros(parts * Bp, C, Hc, Wc, dtype=torch.float64)
    cnt = torch.zeros(Hc, Wc, dtype=torch.float64)
    for (y, x), p in zip(np.asarray(win).tolist(), planes):
        acc[:, :, y:y + S, x:x + S] += p
        cnt[y:y + S, x:x + S] += 1
    return acc / cnt[None, None]


def windowed_translate(sd, cfg, x0, c_src, c_tgt, uc, dec_g, steps, skip, eta, noises, win, rule="mean", c_enc_uc=None):
    """acr.coupled_translate (ctrl = None) on a canvas: x0 / noises [B, C, Hc, Wc]; the forward of every step runs over
    [encoder cond | decoder uncond | decoder cond], each part window-major (row w * B + b), contexts repeated per window;
    the fused prediction of every part is what the step arithmetic - acr.coupled_translate's, line for line - reads.
    dec_g = 1 runs [encoder cond | decoder cond] (no unconditional rows, as the engine at guidance 1)."""
    _full = samplers._full
    ts, a, a_prev, sig, r = samplers.ddim_tables(samplers.sd_alphas_cumprod(), steps, eta)
    K = len(ts) - skip
    B, C, Hc, Wc = x0.shape
    n_win = len(win)
    rep = lambda c: c.repeat(n_win, 1, 1)
    guided = dec_g != 1.0
    ctx = torch.cat([rep(c_src), rep(uc), rep(c_tgt)] if guided else [rep(c_src), rep(c_tgt)], 0)
    fuse = lambda e: fuse_ref(e.permute(0, 2, 3, 1).reshape(e.shape[0], S * S, C), win, B, C, Hc, Wc, S, 1, rule)
    at = a[K - 1]
    xe = at.sqrt() * x0 + (1 - at).sqrt() * noises[0]
    xd = xe
    z = [xe]
    it = 1
    nb = n_win * B
    for i in range(K):
        k = K - i - 1
        a_t, a_p, s_t, r_t = _full(B, a[k]), _full(B, a_prev[k]), _full(B, sig[k]), _full(B, r[k])
        if k == 0:
            x_next = x0
        else:
            e_post = (xe - a_t.sqrt() * x0) / (1 - a_t).sqrt()
            x_next = a_p.sqrt() * x0 + (1. - a_p - s_t ** 2).sqrt() * e_post + s_t * noises[it]
            it += 1
        rows = [crop(xe, win), crop(xd, win), crop(xd, win)] if guided else [crop(xe, win), crop(xd, win)]
        t = torch.full((len(rows) * nb,), int(ts[k]), dtype=torch.long)
        with torch.no_grad():
            e = nets.openai_unet(sd, cfg, torch.cat(rows, 0), t, ctx)
        e_enc = fuse(e[:nb])
        if guided:
            e_u, e_c = fuse(e[nb:2 * nb]), fuse(e[2 * nb:])
            ed = e_u + dec_g * (e_c - e_u)
        else:
            ed = fuse(e[nb:])
        pred_x0 = (xe - r_t * e_enc) / a_t.sqrt()
        eps = (x_next - a_p.sqrt() * pred_x0 - (1. - a_p - s_t ** 2).sqrt() * e_enc) / s_t / 1.0
        z.append(eps)
        pred_d = (xd - r_t * ed) / a_t.sqrt()
        xd = a_p.sqrt() * pred_d + (1. - a_p - s_t ** 2).sqrt() * ed + s_t * eps * 1.0
        xe = x_next
    return z, xd


def canvas_inputs(Hc, Wc):
    """(x0 [2, 4, Hc, Wc], c_src, uc, c_tgt): acr.e2e_inputs' contexts; the latent drawn as golden_util.latent_cycle_inputs
    draws its own, so that the 16 x 16 canvas IS that input"""
    _x0, c, uc, c2 = acr.e2e_inputs()
    return gu.rnd((2, 4, Hc, Wc), 7, 0.8), c, uc, c2


def canvas_noise(Hc, Wc):
    e = acr.E2E
    return gu.latent_noise(e["noise_seed"], (2, 4, Hc, Wc), e["S"] - e["skip"])


@functools.lru_cache(maxsize=None)
def restatement(Hc, Wc, stride, rule="mean"):
    """(z [B, K + 1, C, Hc, Wc], x) of the E2E chain on one canvas - computed once, shared by the tests of a session"""
    from cycle_diffusion_amd import windows
    e = acr.E2E
    sd = gu.weights(gu.load("latent_cycle_tiny"))
    x0, c, uc, c2 = canvas_inputs(Hc, Wc)
    win = windows.window_grid(Hc, Wc, S, stride)
    z, x = windowed_translate(sd, gu.TINY_SD_CFG, x0, c, c2, uc, e["dec_g"], e["S"], e["skip"], e["eta"], canvas_noise(Hc, Wc),
                              win, rule)
    return torch.stack(z, 1), x
