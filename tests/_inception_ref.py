"""Torch restatement of the FID Inception-v3 (torchvision Inception3 with pytorch-fid's FIDInceptionA / C / E_1 / E_2 blocks)
up to pool3, written from the layer table in DESIGN.md section 11: a functional forward over a state_dict keyed by the
checkpoint's names, with STRICT name matching (every tensor used once, none left over). The test oracle of
tests/test_gpu_inception_fid.py; fp32 (or whatever dtype the state_dict and input carry)."""
import torch
import torch.nn.functional as F

BLOCKS = ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3", "maxpool1", "Conv2d_3b_1x1", "Conv2d_4a_3x3", "maxpool2",
          "Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a",
          "Mixed_7b", "Mixed_7c")


class _Params:
    def __init__(self, sd):
        self.sd = {k: v for k, v in sd.items() if not k.startswith("fc.") and not k.endswith("num_batches_tracked")}
        self.used = set()

    def get(self, k):
        self.used.add(k)
        return self.sd[k]  # KeyError on a missing name

    def check_all_used(self):
        left = sorted(set(self.sd) - self.used)
        assert not left, "unused tensors: %s" % left[:5]


def _conv(P, name, x, stride=1, padding=0):
    """BasicConv2d: conv (no bias) + BatchNorm(eps 1e-3, inference) + ReLU"""
    w = P.get(name + ".conv.weight")
    y = F.conv2d(x, w, stride=stride, padding=padding)
    y = F.batch_norm(y, P.get(name + ".bn.running_mean"), P.get(name + ".bn.running_var"), P.get(name + ".bn.weight"),
                     P.get(name + ".bn.bias"), training=False, eps=1e-3)
    return F.relu(y)


def _avg(x):
    return F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False)


def _block_a(P, n, x):
    b1 = _conv(P, n + ".branch1x1", x)
    b5 = _conv(P, n + ".branch5x5_2", _conv(P, n + ".branch5x5_1", x), padding=2)
    d = _conv(P, n + ".branch3x3dbl_1", x)
    d = _conv(P, n + ".branch3x3dbl_2", d, padding=1)
    d = _conv(P, n + ".branch3x3dbl_3", d, padding=1)
    bp = _conv(P, n + ".branch_pool", _avg(x))
    return torch.cat([b1, b5, d, bp], 1)


def _block_b(P, n, x):
    b3 = _conv(P, n + ".branch3x3", x, stride=2)
    d = _conv(P, n + ".branch3x3dbl_1", x)
    d = _conv(P, n + ".branch3x3dbl_2", d, padding=1)
    d = _conv(P, n + ".branch3x3dbl_3", d, stride=2)
    return torch.cat([b3, d, F.max_pool2d(x, 3, stride=2)], 1)


def _block_c(P, n, x):
    b1 = _conv(P, n + ".branch1x1", x)
    s = _conv(P, n + ".branch7x7_1", x)
    s = _conv(P, n + ".branch7x7_2", s, padding=(0, 3))
    s = _conv(P, n + ".branch7x7_3", s, padding=(3, 0))
    d = _conv(P, n + ".branch7x7dbl_1", x)
    d = _conv(P, n + ".branch7x7dbl_2", d, padding=(3, 0))
    d = _conv(P, n + ".branch7x7dbl_3", d, padding=(0, 3))
    d = _conv(P, n + ".branch7x7dbl_4", d, padding=(3, 0))
    d = _conv(P, n + ".branch7x7dbl_5", d, padding=(0, 3))
    bp = _conv(P, n + ".branch_pool", _avg(x))
    return torch.cat([b1, s, d, bp], 1)


def _block_d(P, n, x):
    t = _conv(P, n + ".branch3x3_2", _conv(P, n + ".branch3x3_1", x), stride=2)
    s = _conv(P, n + ".branch7x7x3_1", x)
    s = _conv(P, n + ".branch7x7x3_2", s, padding=(0, 3))
    s = _conv(P, n + ".branch7x7x3_3", s, padding=(3, 0))
    s = _conv(P, n + ".branch7x7x3_4", s, stride=2)
    return torch.cat([t, s, F.max_pool2d(x, 3, stride=2)], 1)


def _block_e(P, n, x, max_pool):
    b1 = _conv(P, n + ".branch1x1", x)
    t = _conv(P, n + ".branch3x3_1", x)
    t = torch.cat([_conv(P, n + ".branch3x3_2a", t, padding=(0, 1)), _conv(P, n + ".branch3x3_2b", t, padding=(1, 0))], 1)
    d = _conv(P, n + ".branch3x3dbl_1", x)
    d = _conv(P, n + ".branch3x3dbl_2", d, padding=1)
    d = torch.cat([_conv(P, n + ".branch3x3dbl_3a", d, padding=(0, 1)),
                   _conv(P, n + ".branch3x3dbl_3b", d, padding=(1, 0))], 1)
    p = F.max_pool2d(x, 3, stride=1, padding=1) if max_pool else _avg(x)
    bp = _conv(P, n + ".branch_pool", p)
    return torch.cat([b1, t, d, bp], 1)


def inception_fid_forward(sd, x, stop_block=-1, return_all=False):
    """x: normalised [B, 3, 299, 299]. stop_block -1: pool3 [B, 2048]; k >= 0: the output of BLOCKS[k].
    return_all: (pool3, [output of every block]) - one pass for block-by-block comparisons."""
    P = _Params(sd)
    outs = []

    def keep(h):
        outs.append(h)
        return len(outs) - 1 == stop_block and not return_all

    h = _conv(P, "Conv2d_1a_3x3", x, stride=2)
    if keep(h):
        return h
    h = _conv(P, "Conv2d_2a_3x3", h)
    if keep(h):
        return h
    h = _conv(P, "Conv2d_2b_3x3", h, padding=1)
    if keep(h):
        return h
    h = F.max_pool2d(h, 3, stride=2)
    if keep(h):
        return h
    h = _conv(P, "Conv2d_3b_1x1", h)
    if keep(h):
        return h
    h = _conv(P, "Conv2d_4a_3x3", h)
    if keep(h):
        return h
    h = F.max_pool2d(h, 3, stride=2)
    if keep(h):
        return h
    for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        h = _block_a(P, n, h)
        if keep(h):
            return h
    h = _block_b(P, "Mixed_6a", h)
    if keep(h):
        return h
    for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        h = _block_c(P, n, h)
        if keep(h):
            return h
    h = _block_d(P, "Mixed_7a", h)
    if keep(h):
        return h
    h = _block_e(P, "Mixed_7b", h, max_pool=False)
    if keep(h):
        return h
    h = _block_e(P, "Mixed_7c", h, max_pool=True)
    if keep(h):
        return h
    P.check_all_used()
    pool3 = F.adaptive_avg_pool2d(h, 1).flatten(1)
    return (pool3, outs) if return_all else pool3
