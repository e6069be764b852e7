"""Host-side handle on the HIP engine: device memory and stream come from PyTorch-ROCm, every
computation goes through the C ABI (include/cyclediff.h)."""
import ctypes as C

import numpy as np
import torch

from . import _ffi
from ._ffi import NetDesc, check, ptr


def make_desc(kind, *, image_size, in_channels, out_channels, model_channels, num_res_blocks, channel_mult,
              attn=(), num_heads=-1, num_head_channels=-1, use_spatial_transformer=False, context_dim=0,
              transformer_depth=1, use_scale_shift_norm=False, resblock_updown=False, conv_resample=True,
              z_channels=0, embed_dim=0, double_z=False, precision=_ffi.CD_PREC_16, n_embed=0):
    d = NetDesc()
    d.precision = int(precision)
    d.n_embed = int(n_embed)
    d.kind = kind
    d.image_size = image_size
    d.in_channels, d.out_channels = in_channels, out_channels
    d.model_channels, d.num_res_blocks = model_channels, num_res_blocks
    d.n_mult = len(channel_mult)
    for i, m in enumerate(channel_mult):
        d.channel_mult[i] = int(m)
    d.n_attn = len(attn)
    for i, a in enumerate(attn):
        d.attn[i] = int(a)
    d.num_heads, d.num_head_channels = num_heads, num_head_channels
    d.use_spatial_transformer = int(use_spatial_transformer)
    d.context_dim = int(context_dim or 0)
    d.transformer_depth = transformer_depth
    d.use_scale_shift_norm = int(use_scale_shift_norm)
    d.resblock_updown = int(resblock_updown)
    d.conv_resample = int(conv_resample)
    d.z_channels, d.embed_dim, d.double_z = z_channels, embed_dim, int(double_z)
    return d


# ---- the architectures the reference ships configs for ------------------------------------------
def sd_v1_unet_desc(image_size=64):
    """model/lib/stable_diffusion/configs/stable-diffusion/v1-inference.yaml:29-44"""
    return make_desc(_ffi.CD_NET_UNET_OPENAI, image_size=image_size, in_channels=4, out_channels=4,
                     model_channels=320, num_res_blocks=2, channel_mult=(1, 2, 4, 4), attn=(4, 2, 1),
                     num_heads=8, use_spatial_transformer=True, context_dim=768)


def ldm_text_unet_desc(image_size=32):
    """model/lib/latentdiff/configs/latent-diffusion/txt2img-1p4B-eval.yaml (context 1280)"""
    return make_desc(_ffi.CD_NET_UNET_OPENAI, image_size=image_size, in_channels=4, out_channels=4,
                     model_channels=320, num_res_blocks=2, channel_mult=(1, 2, 4, 4), attn=(4, 2, 1),
                     num_heads=8, use_spatial_transformer=True, context_dim=1280)


def kl_f8_vae_desc():
    """v1-inference.yaml:46-65 (first_stage_config ddconfig)"""
    return make_desc(_ffi.CD_NET_VAE_KL, image_size=0, in_channels=3, out_channels=3, model_channels=128,
                     num_res_blocks=2, channel_mult=(1, 2, 4, 4), z_channels=4, embed_dim=4, double_z=True)


def vq_f4_vae_desc():
    """first_stage_config of the unconditional LDMs (model/lib/latentdiff/models/ldm/{celeba256,ffhq256}/config.yaml):
    VQModelInterface, embed_dim 3, n_embed 8192, ch 128, ch_mult (1, 2, 4), 2 res blocks, double_z False"""
    return make_desc(_ffi.CD_NET_VAE_KL, image_size=0, in_channels=3, out_channels=3, model_channels=128,
                     num_res_blocks=2, channel_mult=(1, 2, 4), z_channels=3, embed_dim=3, double_z=False, n_embed=8192)


def ldm_uncond_unet_desc(image_size=64):
    """unet_config of celeba256 / ffhq256 (same files): UNetModel with AttentionBlocks (legacy QKV order), 224
    channels, mult (1, 2, 3, 4), attention at downsample rates 2 / 4 / 8, 32-channel heads, no conditioning"""
    return make_desc(_ffi.CD_NET_UNET_OPENAI, image_size=image_size, in_channels=3, out_channels=3,
                     model_channels=224, num_res_blocks=2, channel_mult=(1, 2, 3, 4), attn=(8, 4, 2),
                     num_head_channels=32)


def clip_text_desc(width=768, layers=12, heads=12, mlp=3072, vocab=49408, positions=77):
    """HF CLIPTextConfig of "openai/clip-vit-large-patch14" (ldm/modules/encoders/modules.py:138-141)"""
    return make_desc(_ffi.CD_NET_CLIP_TEXT, image_size=positions, in_channels=vocab, out_channels=width,
                     model_channels=width, num_res_blocks=layers, channel_mult=(1,), num_heads=heads,
                     context_dim=mlp)


def oclip_text_desc(width=512, layers=12, heads=8, vocab=49408, positions=77, embed=512):
    """text tower of OpenAI CLIP ViT-B/32 (clip/model.py CLIP.__init__: transformer_width 512, heads 8, layers 12)"""
    return make_desc(_ffi.CD_NET_OCLIP_TEXT, image_size=positions, in_channels=vocab, out_channels=embed,
                     model_channels=width, num_res_blocks=layers, channel_mult=(1,), num_heads=heads,
                     context_dim=4 * width)


def oclip_vision_desc(width=768, layers=12, heads=12, resolution=224, patch=32, embed=512):
    """image tower of OpenAI CLIP ViT-B/32 (clip/model.py VisionTransformer: width 768, patch 32, 12 layers)"""
    return make_desc(_ffi.CD_NET_OCLIP_VISION, image_size=resolution, in_channels=3, out_channels=embed,
                     model_channels=width, num_res_blocks=layers, channel_mult=(1,), num_heads=heads,
                     context_dim=4 * width, z_channels=patch)


def bert_xtransformer_desc(width=1280, layers=32, vocab=30522, positions=77, heads=8, dim_head=64):
    """BERTEmbedder(n_embed=1280, n_layer=32) of txt2img-1p4B-eval.yaml: x-transformers Encoder (8 heads x 64, FF x4)"""
    return make_desc(_ffi.CD_NET_BERT_XTR, image_size=positions, in_channels=vocab, out_channels=width,
                     model_channels=width, num_res_blocks=layers, channel_mult=(1,), num_heads=heads,
                     num_head_channels=dim_head, context_dim=4 * width)


def afhq_iddpm_desc(image_size=256, precision=_ffi.CD_PREC_16):
    """improved_ddpm/script_util.py:5-22,45-104 (AFHQ_DICT; learn_sigma -> 6 output channels)"""
    return make_desc(_ffi.CD_NET_UNET_OPENAI, image_size=image_size, in_channels=3, out_channels=6,
                     model_channels=128, num_res_blocks=1, channel_mult=(1, 1, 2, 2, 4, 4),
                     attn=(image_size // 16,), num_heads=4, num_head_channels=64,
                     use_scale_shift_norm=True, resblock_updown=True, precision=precision)


def ho_ddpm_desc(image_size, ch, ch_mult, num_res_blocks, attn_resolutions, in_channels=3, out_ch=3,
                 precision=_ffi.CD_PREC_16):
    """ddpm/diffusion.py:192-205 (config.model.*)"""
    return make_desc(_ffi.CD_NET_UNET_HO, image_size=image_size, in_channels=in_channels, out_channels=out_ch,
                     model_channels=ch, num_res_blocks=num_res_blocks, channel_mult=tuple(ch_mult),
                     attn=tuple(attn_resolutions), precision=precision)


def inception_fid_desc():
    """The FID Inception-v3 (csrc/inception.hip): 299 x 299 input, 16-bit storage; no other descriptor field is read."""
    return make_desc(_ffi.CD_NET_INCEPTION_FID, image_size=299, in_channels=3, out_channels=2048, model_channels=0,
                     num_res_blocks=0, channel_mult=(), precision=_ffi.CD_PREC_16)


def inception_fid_units():
    """[(name, in_channels, out_channels, (kh, kw))] of every BasicConv2d of the FID Inception-v3 (torchvision Inception3
    naming), in the engine's declaration order."""
    u = [("Conv2d_1a_3x3", 3, 32, (3, 3)), ("Conv2d_2a_3x3", 32, 32, (3, 3)), ("Conv2d_2b_3x3", 32, 64, (3, 3)),
         ("Conv2d_3b_1x1", 64, 80, (1, 1)), ("Conv2d_4a_3x3", 80, 192, (3, 3))]
    for name, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        u += [(name + ".branch1x1", cin, 64, (1, 1)), (name + ".branch5x5_1", cin, 48, (1, 1)),
              (name + ".branch5x5_2", 48, 64, (5, 5)), (name + ".branch3x3dbl_1", cin, 64, (1, 1)),
              (name + ".branch3x3dbl_2", 64, 96, (3, 3)), (name + ".branch3x3dbl_3", 96, 96, (3, 3)),
              (name + ".branch_pool", cin, pf, (1, 1))]
    u += [("Mixed_6a.branch3x3", 288, 384, (3, 3)), ("Mixed_6a.branch3x3dbl_1", 288, 64, (1, 1)),
          ("Mixed_6a.branch3x3dbl_2", 64, 96, (3, 3)), ("Mixed_6a.branch3x3dbl_3", 96, 96, (3, 3))]
    for name, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        u += [(name + ".branch1x1", 768, 192, (1, 1)), (name + ".branch7x7_1", 768, c7, (1, 1)),
              (name + ".branch7x7_2", c7, c7, (1, 7)), (name + ".branch7x7_3", c7, 192, (7, 1)),
              (name + ".branch7x7dbl_1", 768, c7, (1, 1)), (name + ".branch7x7dbl_2", c7, c7, (7, 1)),
              (name + ".branch7x7dbl_3", c7, c7, (1, 7)), (name + ".branch7x7dbl_4", c7, c7, (7, 1)),
              (name + ".branch7x7dbl_5", c7, 192, (1, 7)), (name + ".branch_pool", 768, 192, (1, 1))]
    u += [("Mixed_7a.branch3x3_1", 768, 192, (1, 1)), ("Mixed_7a.branch3x3_2", 192, 320, (3, 3)),
          ("Mixed_7a.branch7x7x3_1", 768, 192, (1, 1)), ("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7)),
          ("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1)), ("Mixed_7a.branch7x7x3_4", 192, 192, (3, 3))]
    for name, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        u += [(name + ".branch1x1", cin, 320, (1, 1)), (name + ".branch3x3_1", cin, 384, (1, 1)),
              (name + ".branch3x3_2a", 384, 384, (1, 3)), (name + ".branch3x3_2b", 384, 384, (3, 1)),
              (name + ".branch3x3dbl_1", cin, 448, (1, 1)), (name + ".branch3x3dbl_2", 448, 384, (3, 3)),
              (name + ".branch3x3dbl_3a", 384, 384, (1, 3)), (name + ".branch3x3dbl_3b", 384, 384, (3, 1)),
              (name + ".branch_pool", cin, 192, (1, 1))]
    return u


# output shapes (C, H, W) of cd_inception_features' block list: the stem convs and pools one by one, then each Mixed block
INCEPTION_BLOCKS = ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3", "maxpool1", "Conv2d_3b_1x1", "Conv2d_4a_3x3",
                    "maxpool2", "Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d",
                    "Mixed_6e", "Mixed_7a", "Mixed_7b", "Mixed_7c")
INCEPTION_BLOCK_SHAPES = ((32, 149, 149), (32, 147, 147), (64, 147, 147), (64, 73, 73), (80, 73, 73), (192, 71, 71),
                          (192, 35, 35), (256, 35, 35), (288, 35, 35), (288, 35, 35), (768, 17, 17), (768, 17, 17),
                          (768, 17, 17), (768, 17, 17), (768, 17, 17), (1280, 8, 8), (2048, 8, 8), (2048, 8, 8))


def inception_synthetic_state_dict(seed=0):
    """Seeded synthetic weights for the FID Inception-v3, keyed as its checkpoint (`X.conv.weight`, `X.bn.*`): He-normal
    convs (std sqrt(2 / fan_in), so that activations keep their scale through 94 ReLU layers), BN weight ~ 1, small bias and
    mean, running_var = 1 + a small positive term (Engine.random_init would draw negative variances)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, cin, cout, (kh, kw) in inception_fid_units():
        fan_in = cin * kh * kw
        sd[name + ".conv.weight"] = torch.randn((cout, cin, kh, kw), generator=g) * float(np.sqrt(2.0 / fan_in))
        sd[name + ".bn.weight"] = 1.0 + 0.05 * torch.randn(cout, generator=g)
        sd[name + ".bn.bias"] = 0.05 * torch.randn(cout, generator=g)
        sd[name + ".bn.running_mean"] = 0.05 * torch.randn(cout, generator=g)
        sd[name + ".bn.running_var"] = 1.0 + 0.1 * torch.rand(cout, generator=g)
    return sd


# ---- LPIPS (csrc/lpips.hip): the torchvision `features` stacks the `lpips` package taps
LPIPS_SHIFT = (-.030, -.088, -.188)
LPIPS_SCALE = (.458, .448, .450)
LPIPS_MIN_SIZE = {"alex": 31, "vgg": 16}


def lpips_desc(net="alex"):
    """LPIPS v0.1 on the AlexNet ("alex") or VGG16 ("vgg") backbone: num_res_blocks carries the number of convs (5 / 13),
    which selects the backbone; 16-bit storage, any input size from LPIPS_MIN_SIZE up; no other descriptor field is read."""
    if net not in ("alex", "vgg"):
        raise ValueError("LPIPS backbone %r: 'alex' or 'vgg'" % (net,))
    return make_desc(_ffi.CD_NET_LPIPS, image_size=0, in_channels=3, out_channels=1, model_channels=0,
                     num_res_blocks=5 if net == "alex" else 13, channel_mult=(), precision=_ffi.CD_PREC_16)


def lpips_layers(net="alex"):
    """[(features index, in_channels, out_channels, kernel, stride, pad, pool ahead of it (0 / 2 / 3), tap or -1)] of every
    conv of the backbone, in the engine's declaration order. Pools are stride 2: 3 x 3 (alex) or 2 x 2 (vgg), floor mode."""
    if net == "alex":
        return [(0, 3, 64, 11, 4, 2, 0, 0), (3, 64, 192, 5, 1, 2, 3, 1), (6, 192, 384, 3, 1, 1, 3, 2),
                (8, 384, 256, 3, 1, 1, 0, 3), (10, 256, 256, 3, 1, 1, 0, 4)]
    if net != "vgg":
        raise ValueError("LPIPS backbone %r: 'alex' or 'vgg'" % (net,))
    out, cin, tap = [], 3, 0
    for idx, width in zip((0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28),
                          (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)):
        is_tap = idx in (2, 7, 14, 21, 28)
        out.append((idx, cin, width, 3, 1, 1, 2 if idx in (5, 10, 17, 24) else 0, tap if is_tap else -1))
        tap += int(is_tap)
        cin = width
    return out


def lpips_tap_shapes(net, H, W):
    """[(C, h, w)] of the five taps for an H x W input"""
    shapes, h, w = [], H, W
    for _, _, cout, k, stride, pad, pool, tap in lpips_layers(net):
        if pool == 2:
            h, w = h // 2, w // 2
        elif pool == 3:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        h, w = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        if tap >= 0:
            shapes.append((cout, h, w))
    return shapes


def lpips_pair_bytes(net, H, W):
    """Arena high-water of cd_lpips per PAIR of H x W images (16-bit activations; lpips.hip's allocation order: the input
    rows, then per stage the next stage's pooled input ahead of the stage's own conv outputs, which are released behind the
    pool). The per-image partial sums of k_lpips_layer (a few KB) are not counted."""
    layers = lpips_layers(net)
    held = H * W * 32  # elements per image that stay allocated
    peak, h, w, i = held, H, W, 0
    while i < len(layers):
        e = i
        while layers[e][7] < 0:
            e += 1
        sizes, hh, ww = [], h, w
        for _, _, cout, k, stride, pad, _, _ in layers[i:e + 1]:
            hh, ww = (hh + 2 * pad - k) // stride + 1, (ww + 2 * pad - k) // stride + 1
            sizes.append(cout * hh * ww)
        pool = layers[e + 1][6] if e + 1 < len(layers) else 0
        if pool:
            h, w = (hh // 2, ww // 2) if pool == 2 else ((hh - 3) // 2 + 1, (ww - 3) // 2 + 1)
            held += layers[e][2] * h * w
            peak = max(peak, held + sum(sizes))
        else:
            h, w = hh, ww
            held += sum(sizes)
            peak = max(peak, held)
        i = e + 1
    return 2 * 2 * peak  # two images, two bytes per element


def lpips_synthetic_state_dict(net="alex", seed=0):
    """Seeded synthetic LPIPS weights in the engine's naming (`features.N.weight|bias`, `lin{l}.weight`): He-normal convs
    (std sqrt(2 / fan_in)), small biases, and NON-NEGATIVE `lin` weights of mean about 1 / C (as the trained ones are
    non-negative), so that activations and the five terms stay at scale through all 13 layers."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for idx, cin, cout, k, _, _, _, tap in lpips_layers(net):
        sd["features.%d.weight" % idx] = torch.randn((cout, cin, k, k), generator=g) * float(np.sqrt(2.0 / (cin * k * k)))
        sd["features.%d.bias" % idx] = 0.05 * torch.randn(cout, generator=g)
        if tap >= 0:
            sd["lin%d.weight" % tap] = (2.0 / cout) * torch.rand((1, cout, 1, 1), generator=g)
    return sd


def lpips_engine_state_dict(sd):
    """Either checkpoint layout -> the engine's naming. A full `lpips.LPIPS(net=...)` state_dict has
    `net.slice{k}.{N}.weight|bias` (N = the torchvision `features` index), `lin{l}.model.1.weight`, the same again under
    `lins.{l}.*`, and `scaling_layer.shift|scale`; the alternative is a torchvision backbone state_dict (`features.N.*`,
    `classifier.*`) merged with the package's linear file (`lin{l}.model.1.weight`). `lins.*`, `classifier.*` and
    `scaling_layer.*` are skipped; the scaling constants, when present, must be the ones the engine applies."""
    out = {}
    for k, v in sd.items():
        if k.startswith(("lins.", "classifier.")) or k.endswith(".num_batches_tracked"):
            continue
        if k.startswith("scaling_layer."):
            want = LPIPS_SHIFT if k.endswith("shift") else LPIPS_SCALE
            got = [float(t) for t in torch.as_tensor(v).flatten()]
            assert len(got) == 3 and all(abs(a - b) < 1e-6 for a, b in zip(got, want)), (k, got)
            continue
        parts = k.split(".")
        if parts[0] == "net" and parts[1].startswith("slice"):
            k = "features." + ".".join(parts[2:])
        elif parts[0].startswith("lin") and parts[1:] == ["model", "1", "weight"]:
            k = parts[0] + ".weight"
        out[k] = v
    return out


class Engine:
    """One engine per rank / stream (cd_engine_create)."""

    def __init__(self, device="cuda:0", workspace_bytes=None):
        self.lib = _ffi.load_library()
        if not torch.cuda.is_available():
            raise _ffi.EngineError("no HIP device visible to PyTorch: the CycleDiffusion engine has no CPU fallback")
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        if workspace_bytes is None:
            free, _total = torch.cuda.mem_get_info(self.device)
            # the bump arena is reserved up front: 32 GB covers the largest folded-ensemble VAE decode (32 images
            # at 512x512) many times over and leaves room for several engines per GPU (bench.py replicas)
            workspace_bytes = int(min(32 << 30, free * 0.45))
        self.workspace_bytes = int(workspace_bytes)
        self.stream = torch.cuda.current_stream(self.device)
        h = C.c_void_p()
        check(self.lib.cd_engine_create(C.c_void_p(self.stream.cuda_stream), C.c_size_t(workspace_bytes), C.byref(h)))
        self.h = h
        self._descs = {}

    def synchronize(self):
        """Wait for the engine's stream without spinning (cd_engine_synchronize)."""
        check(self.lib.cd_engine_synchronize(self.h))

    def close(self):
        if getattr(self, "h", None):
            torch.cuda.synchronize(self.device)
            self.lib.cd_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- networks
    def create_net(self, desc):
        nid = C.c_int(-1)
        check(self.lib.cd_net_create(self.h, C.byref(desc), C.byref(nid)))
        self._descs[nid.value] = desc
        return nid.value

    def net_params(self, net):
        n = C.c_int()
        check(self.lib.cd_net_param_count(self.h, net, C.byref(n)))
        out = []
        buf = C.create_string_buffer(512)
        nd = C.c_int()
        shp = (C.c_int64 * 4)()
        for i in range(n.value):
            check(self.lib.cd_net_param_info(self.h, net, i, buf, 512, C.byref(nd), shp))
            out.append((buf.value.decode(), tuple(int(shp[j]) for j in range(nd.value))))
        return out

    def load_param(self, net, name, tensor):
        t = tensor.detach().to(torch.float32).cpu().contiguous()
        shp = (C.c_int64 * max(1, t.dim()))(*t.shape)
        check(self.lib.cd_net_load_param(self.h, net, name.encode(), C.c_void_p(t.data_ptr()), t.dim(), shp))

    def load_state_dict(self, net, sd, prefix="", strict=True):
        """Load weights keyed by the reference's state_dict names (txt2img.py:25-42)."""
        names = [n for n, _ in self.net_params(net)]
        for n in names:
            key = prefix + n
            if key in sd:
                self.load_param(net, n, sd[key])
            elif strict:
                raise KeyError("missing parameter %s" % key)
        return self.missing(net)

    def missing(self, net):
        n = C.c_int()
        buf = C.create_string_buffer(512)
        check(self.lib.cd_net_missing_params(self.h, net, C.byref(n), buf, 512))
        return n.value, buf.value.decode()

    _SYNTH_CACHE = {}  # (seed, names+shapes) -> tensors; lets several engines of one process share the host work

    def random_init(self, net, seed=0, std=0.02, cache=False):
        """Synthetic weights for benchmarks: N(0, fan-in scaled) matrices, unit norms.
        (There are no checkpoints in the tree)"""
        params = self.net_params(net)
        key = (seed, tuple((n, tuple(s)) for n, s in params))
        if cache and key in Engine._SYNTH_CACHE:
            for (name, _), t in zip(params, Engine._SYNTH_CACHE[key]):
                self.load_param(net, name, t)
            n, first = self.missing(net)
            assert n == 0, first
            return
        made = []
        g = torch.Generator().manual_seed(seed)
        for name, shape in params:
            if len(shape) == 1:
                base = name.rsplit(".", 1)[0]
                is_norm = name.endswith("weight") and (".norm" in name or "in_layers.0" in name or "out_layers.0" in name
                                                       or name.startswith("out.0") or "norm_out" in name
                                                       or "layer_norm" in name or ".ln_" in name
                                                       or name.startswith("ln_"))
                if is_norm:
                    t = 1.0 + 0.05 * torch.randn(shape, generator=g)
                else:
                    t = 0.02 * torch.randn(shape, generator=g)
                del base
            else:
                fan_in = int(np.prod(shape[1:]))
                t = torch.randn(shape, generator=g) * (1.0 / np.sqrt(fan_in))
            self.load_param(net, name, t)
            if cache:
                made.append(t)
        if cache:
            Engine._SYNTH_CACHE[key] = made
        n, first = self.missing(net)
        assert n == 0, first

    # ---- forward passes
    def _f32(self, t):
        assert t.is_cuda and t.dtype == torch.float32
        return t.contiguous()

    def unet_forward(self, net, x, t, ctx=None):
        x, t = self._f32(x), self._f32(t.float())
        ctx = self._f32(ctx) if ctx is not None else None
        out_ch = self._out_channels(net)
        y = torch.empty((x.shape[0], out_ch, x.shape[2], x.shape[3]), device=x.device, dtype=torch.float32)
        check(self.lib.cd_unet_forward(self.h, net, ptr(x), ptr(t), ptr(ctx), x.shape[0],
                                       ctx.shape[1] if ctx is not None else 0, ptr(y)))
        return y

    def _out_channels(self, net):
        return self._descs[net].out_channels

    def text_encode(self, net, tokens):
        """tokens [B, L] integer ids -> last_hidden_state [B, L, width] fp32 (FrozenCLIPEmbedder.forward)."""
        ids = tokens.to(device=self.device, dtype=torch.int32).contiguous()
        B, L = ids.shape
        out = torch.empty((B, L, self._descs[net].model_channels), device=self.device, dtype=torch.float32)
        check(self.lib.cd_text_encode(self.h, net, ptr(ids), B, L, ptr(out)))
        return out

    def clip_text_features(self, net, tokens):
        """model.encode_text(tokens) of OpenAI CLIP: [B, L] ids -> [B, embed] fp32 (un-normalised)."""
        ids = tokens.to(device=self.device, dtype=torch.int32).contiguous()
        B, L = ids.shape
        out = torch.empty((B, self._descs[net].out_channels), device=self.device, dtype=torch.float32)
        check(self.lib.cd_clip_text_features(self.h, net, ptr(ids), B, L, ptr(out)))
        return out

    def clip_image_features(self, net, img):
        """model.encode_image(img) of OpenAI CLIP: preprocessed [B, 3, R, R] fp32 -> [B, embed] fp32."""
        img = self._f32(img)
        d = self._descs[net]
        assert img.shape[1:] == (3, d.image_size, d.image_size), img.shape
        out = torch.empty((img.shape[0], d.out_channels), device=self.device, dtype=torch.float32)
        check(self.lib.cd_clip_image_features(self.h, net, ptr(img), img.shape[0], ptr(out)))
        return out

    def load_inception_state_dict(self, net, sd):
        """A pytorch-fid / clean-fid Inception state_dict: every tensor the network declares, `fc.*` and
        `*.num_batches_tracked` skipped. Raises KeyError on a missing tensor."""
        sd = {k: v for k, v in sd.items() if not k.startswith("fc.") and not k.endswith(".num_batches_tracked")}
        n, first = self.load_state_dict(net, sd, strict=True)
        if n:
            raise KeyError("Inception state_dict lacks %d tensors, first: %s" % (n, first))

    def inception_features(self, net, img, stop_block=-1):
        """cd_inception_features: normalised [B, 3, 299, 299] fp32 -> pool3 [B, 2048] fp32 (stop_block -1), or the fp32 NCHW
        output of block list entry `stop_block` (include/cyclediff.h)."""
        img = self._f32(img)
        assert img.shape[1:] == (3, 299, 299), img.shape
        B = img.shape[0]
        if stop_block < 0:
            shape = (B, 2048)
        else:
            shape = (B,) + INCEPTION_BLOCK_SHAPES[stop_block]
        out = torch.empty(shape, device=img.device, dtype=torch.float32)
        check(self.lib.cd_inception_features(self.h, net, ptr(img), B, int(stop_block), ptr(out)))
        return out

    def load_lpips_state_dict(self, net, sd):
        """LPIPS weights in either checkpoint layout or the engine's own naming (lpips_engine_state_dict). Raises KeyError
        on a missing tensor."""
        n, first = self.load_state_dict(net, lpips_engine_state_dict(sd), strict=True)
        if n:
            raise KeyError("LPIPS state_dict lacks %d tensors, first: %s" % (n, first))

    def _lpips_name(self, net):
        return "alex" if self._descs[net].num_res_blocks == 5 else "vgg"

    def lpips(self, net, img0, img1, per_layer=False):
        """cd_lpips: [B, 3, H, W] fp32 in [-1, 1], twice -> the LPIPS distance [B] (and the five tap terms [B, 5])."""
        img0, img1 = self._f32(img0), self._f32(img1)
        assert img0.dim() == 4 and img0.shape[1] == 3 and img0.shape == img1.shape, (img0.shape, img1.shape)
        B, _, H, W = img0.shape
        out = torch.empty((B,), device=img0.device, dtype=torch.float32)
        layers = torch.empty((B, 5), device=img0.device, dtype=torch.float32) if per_layer else None
        check(self.lib.cd_lpips(self.h, net, ptr(img0), ptr(img1), B, H, W, ptr(layers), ptr(out)))
        return (out, layers) if per_layer else out

    def lpips_tap(self, net, img, tap):
        """cd_lpips_tap: the un-normalised ReLU output of tap 0..4 as fp32 NCHW."""
        img = self._f32(img)
        assert img.dim() == 4 and img.shape[1] == 3, img.shape
        B, _, H, W = img.shape
        if not 0 <= int(tap) < 5:
            raise ValueError("LPIPS tap %r outside 0..4" % (tap,))
        shapes = lpips_tap_shapes(self._lpips_name(net), H, W)
        shape = shapes[int(tap)] if min(shapes[-1]) > 0 else (1, 1, 1)  # too small: the engine refuses and names the minimum
        out = torch.empty((B,) + tuple(shape), device=img.device, dtype=torch.float32)
        check(self.lib.cd_lpips_tap(self.h, net, ptr(img), B, H, W, int(tap), ptr(out)))
        return out

    def vae_encode(self, net, img, noise=None, seed=0, sample=True, scale=0.18215):
        """img [B, 3, H, W], H and W multiples of the first-stage factor f -> z [B, zc, H / f, W / f]; a square image takes
        cd_vae_encode, a rectangle cd_vae_encode_hw"""
        img = self._f32(img)
        d = self._descs[net]
        B, _, H, W = img.shape
        f = 2 ** (d.n_mult - 1)
        z = torch.empty((B, d.embed_dim, H // f, W // f), device=img.device, dtype=torch.float32)
        if noise is not None:
            noise = self._f32(noise)
        if H == W:
            check(self.lib.cd_vae_encode(self.h, net, ptr(img), ptr(noise), C.c_uint64(seed), B, H, int(sample),
                                         C.c_float(scale), ptr(z)))
        else:
            check(self.lib.cd_vae_encode_hw(self.h, net, ptr(img), ptr(noise), C.c_uint64(seed), B, H, W, int(sample),
                                            C.c_float(scale), ptr(z)))
        return z

    def vae_decode(self, net, z, scale=0.18215, out_mul=1.0, out_add=0.0):
        """z [B, zc, h, w] -> img [B, 3, h * f, w * f]; a square latent takes cd_vae_decode, a rectangle cd_vae_decode_hw"""
        z = self._f32(z)
        d = self._descs[net]
        B, _, hl, wl = z.shape
        f = 2 ** (d.n_mult - 1)
        img = torch.empty((B, d.out_channels, hl * f, wl * f), device=z.device, dtype=torch.float32)
        if hl == wl:
            check(self.lib.cd_vae_decode(self.h, net, ptr(z), B, hl, C.c_float(scale), C.c_float(out_mul),
                                         C.c_float(out_add), ptr(img)))
        else:
            check(self.lib.cd_vae_decode_hw(self.h, net, ptr(z), B, hl, wl, C.c_float(scale), C.c_float(out_mul),
                                            C.c_float(out_add), ptr(img)))
        return img

    def dpm_encode(self, net, kind, x0, coef, ctx_c=None, ctx_uc=None, guidance=1.0, noise=None, seed=0,
                   last_uses_x0=True):
        """coef: numpy struct array (STEP_COEF_DTYPE) with K+1 rows; returns z [B, K+1, C, H, W]."""
        x0 = self._f32(x0)
        K = len(coef) - 1
        B, Cc, H, W = x0.shape
        z = torch.empty((B, K + 1, Cc, H, W), device=x0.device, dtype=torch.float32)
        coef = np.ascontiguousarray(coef)
        L = ctx_c.shape[1] if ctx_c is not None else (ctx_uc.shape[1] if ctx_uc is not None else 0)
        check(self.lib.cd_dpm_encode(self.h, net, kind, ptr(x0),
                                     ptr(self._f32(ctx_c)) if ctx_c is not None else None,
                                     ptr(self._f32(ctx_uc)) if ctx_uc is not None else None,
                                     L, C.c_float(guidance), B, K, C.c_void_p(coef.ctypes.data),
                                     ptr(self._f32(noise)) if noise is not None else None,
                                     C.c_uint64(seed), int(last_uses_x0), ptr(z)))
        return z

    def ddim_decode(self, net, kind, z, coef, n_eps=None, ctx_c=None, ctx_uc=None, guidance=1.0, noise_tail=None,
                    seed=0):
        """z [B, T, C, H, W]; coef K rows; returns x [B, C, H, W]. `guidance`: one scale, or a sequence / tensor of B
        scales (each neither 0 nor 1: cd_ddim_decode_v) when the samples of the batch differ in it."""
        z = self._f32(z)
        B, T, Cc, H, W = z.shape
        K = len(coef)
        if n_eps is None:
            n_eps = T - 1
        x = torch.empty((B, Cc, H, W), device=z.device, dtype=torch.float32)
        coef = np.ascontiguousarray(coef)
        L = ctx_c.shape[1] if ctx_c is not None else (ctx_uc.shape[1] if ctx_uc is not None else 0)
        cc = ptr(self._f32(ctx_c)) if ctx_c is not None else None
        cu = ptr(self._f32(ctx_uc)) if ctx_uc is not None else None
        nt = ptr(self._f32(noise_tail)) if noise_tail is not None else None
        if isinstance(guidance, (int, float)):
            check(self.lib.cd_ddim_decode(self.h, net, kind, ptr(z), T, n_eps, cc, cu, L, C.c_float(guidance), B, K,
                                          C.c_void_p(coef.ctypes.data), nt, C.c_uint64(seed), ptr(x)))
        else:
            g = torch.as_tensor(guidance, dtype=torch.float32).to(z.device).contiguous()
            if g.numel() != B or bool(((g == 0) | (g == 1)).any()):
                raise ValueError("per-sample guidance: B scales, none of them 0 or 1")
            check(self.lib.cd_ddim_decode_v(self.h, net, kind, ptr(z), T, n_eps, cc, cu, L, ptr(g), B, K,
                                            C.c_void_p(coef.ctypes.data), nt, C.c_uint64(seed), ptr(x)))
            self._keep = g  # the launches read it asynchronously
        return x

    def ddim_invert(self, net, x0, coef, ctx_c=None, ctx_uc=None, guidance=1.0, trajectory=False):
        """cd_ddim_invert: deterministic DDIM inversion (DDIB's encoder) over the K rows of `coef` (loop order, sigma 0:
        DDIMSchedule.coef_invert / PixelSchedule.coef_invert). Returns x_K [B, C, H, W], or (x_K, [K, B, C, H, W] of every
        step's x) with trajectory=True."""
        x0 = self._f32(x0)
        K = len(coef)
        coef = np.ascontiguousarray(coef)
        x = torch.empty_like(x0)
        traj = torch.empty((K,) + tuple(x0.shape), device=x0.device, dtype=torch.float32) if trajectory else None
        L = ctx_c.shape[1] if ctx_c is not None else (ctx_uc.shape[1] if ctx_uc is not None else 0)
        check(self.lib.cd_ddim_invert(self.h, net, _ffi.CD_SCHED_DDIM, ptr(x0),
                                      ptr(self._f32(ctx_c)) if ctx_c is not None else None,
                                      ptr(self._f32(ctx_uc)) if ctx_uc is not None else None,
                                      L, C.c_float(guidance), x0.shape[0], K, C.c_void_p(coef.ctypes.data), ptr(x),
                                      ptr(traj)))
        return (x, traj) if trajectory else x

    def cycle_translate(self, net, kind, x0, coef_enc, coef_dec, enc_ctx_c=None, enc_ctx_uc=None, enc_guidance=1.0,
                        dec_ctx_c=None, dec_ctx_uc=None, dec_guidance=1.0, n_dec=1, noise=None, seed=0, last_uses_x0=True,
                        windows=None):
        """The coupled loop (cd_cycle_translate): dpm_encode and ddim_decode of the same network over the whole chain with ONE
        forward per step over [encoder rows | decoder rows]. x0 [B, C, H, W]; dec_ctx_* [n_dec * B, L, Dc] (decoder row
        j * B + b decodes encoder sample b); dec_guidance one scale or n_dec * B of them (none 0 or 1).
        `windows` (int32 [n, 2] of (y, x), windows.window_grid): fused windows - x0 / noise are then a canvas [.., Hc, Wc] at
        least as large as the network's S x S, covered by the n windows; the forward runs n x the rows.
        Returns (z [B, K+1, C, H, W], x [n_dec * B, C, H, W])."""
        return self._cycle_translate(net, kind, x0, coef_enc, coef_dec, enc_ctx_c, enc_ctx_uc, enc_guidance, dec_ctx_c, dec_ctx_uc,
                                     dec_guidance, n_dec, noise, seed, last_uses_x0, windows=windows)

    def _cycle_translate(self, net, kind, x0, coef_enc, coef_dec, enc_ctx_c, enc_ctx_uc, enc_guidance, dec_ctx_c, dec_ctx_uc,
                         dec_guidance, n_dec, noise, seed, last_uses_x0, mask=None, mask_x0=None, qcoef=None, mask_noise=None,
                         mask_seed=0, mask_source="q_sample", ctrl=None, blend=None, sega=None, windows=None):
        """The marshalling of cd_cycle_translate: one cd_translate_args, and an option struct for each of the keep-mask, `ctrl` =
        (mapper, alpha, weight, n_ctrl), `blend` = (sel_src, sel_tgt, side, pool, thr, n_start) - it returns (z, x, acc, keep) -
        and `sega` = (edit_ctx, concepts, momentum_scale, momentum_beta) - it returns (z, x, tau, kept, mask). An option that is
        None stays a NULL pointer; which options go together is cycle_translate_impl's decision, repeated here only where a
        ValueError can say it earlier."""
        x0 = self._f32(x0)
        K = len(coef_dec)
        assert len(coef_enc) == K + 1
        B, Cc, H, W = x0.shape
        if mask is not None:
            mask, mask_x0, Bm, src, qcoef, mask_noise = self._mask_args(mask, mask_x0, B, qcoef, mask_noise, mask_source, H, W,
                                                                        Cc, K, b_noise=n_dec * B)
        else:
            mask_x0 = qcoef = mask_noise = None
        z = torch.empty((B, K + 1, Cc, H, W), device=x0.device, dtype=torch.float32)
        x = torch.empty((n_dec * B, Cc, H, W), device=x0.device, dtype=torch.float32)
        coef_enc, coef_dec = np.ascontiguousarray(coef_enc), np.ascontiguousarray(coef_dec)
        ctxs = [self._f32(t) if t is not None else None for t in (enc_ctx_c, enc_ctx_uc, dec_ctx_c, dec_ctx_uc)]
        L = next((t.shape[1] for t in ctxs if t is not None), 0)
        for t, rows in zip(ctxs, (B, B, n_dec * B, n_dec * B)):
            assert t is None or t.shape[0] == rows, (t.shape, rows)
        a = _ffi.TranslateArgs(size=C.sizeof(_ffi.TranslateArgs))
        ctl, sels, outs = None, None, ()
        if blend is not None and mask is not None:
            raise ValueError("the local blend rewrites the keep-mask after every step: it takes no mask of the caller's")
        if blend is not None and sega is not None:
            raise ValueError("semantic guidance and the local blend are not built together")
        if mask is not None:
            a.mask = C.pointer(_ffi.KeepMask(
                mask=ptr(mask), x0=ptr(mask_x0), B_mask=Bm, source=src,
                qsample_coef_host=qcoef.ctypes.data if qcoef is not None else None, noise=ptr(mask_noise), seed=mask_seed))
        if ctrl is not None:
            ctl = [torch.as_tensor(t, dtype=torch.float32).to(x0.device).contiguous() for t in ctrl[:3]]
            Bc = ctl[0].shape[0]
            if tuple(ctl[0].shape) != (Bc, L, L) or tuple(ctl[1].shape) != (Bc, L) or tuple(ctl[2].shape) != (Bc, L):
                raise ValueError("control tensors must be mapper [B_ctrl, %d, %d], alpha / weight [B_ctrl, %d], got %s"
                                 % (L, L, L, [tuple(t.shape) for t in ctl]))
            a.ctrl = C.pointer(_ffi.AttnCtrl(mapper=ptr(ctl[0]), alpha=ptr(ctl[1]), weight=ptr(ctl[2]), B_ctrl=Bc,
                                             n_ctrl=int(ctrl[3])))
        if sega is not None:
            ectx = self._f32(sega[0])
            table = np.ascontiguousarray(sega[1], dtype=_ffi.SEGA_CONCEPT_DTYPE)
            E, Bd = len(table), n_dec * B
            if ectx.dim() != 3 or ectx.shape[0] != E * Bd or (L and ectx.shape[1] != L):
                raise ValueError("edit_ctx must be [E * n_dec * B = %d, %d, Dc] (concept-major), got %s"
                                 % (E * Bd, L, tuple(ectx.shape)))
            tau = torch.empty((K, Bd, E), device=x0.device, dtype=torch.float32)
            kept = torch.empty((K, Bd, E), device=x0.device, dtype=torch.int32)
            emask = torch.empty((Bd, E, Cc, H, W), device=x0.device, dtype=torch.float32)
            a.sega = C.pointer(_ffi.Sega(edit_ctx=ptr(ectx), concepts_host=table.ctypes.data, E=E, momentum_scale=sega[2],
                                         momentum_beta=sega[3], tau_out=ptr(tau), kept_out=ptr(kept), mask_out=ptr(emask)))
            sels = (ectx, table)
            outs = (tau, kept, emask)
        if blend is not None:
            sels = [torch.as_tensor(t, dtype=torch.float32).to(x0.device).contiguous() for t in blend[:2]]
            Bs = sels[0].shape[0]
            if sels[0].dim() != 2 or tuple(sels[0].shape) != (Bs, L) or tuple(sels[1].shape) != (Bs, L):
                raise ValueError("the local blend's selectors must both be [B_sel, %d], got %s"
                                 % (L, [tuple(t.shape) for t in sels]))
            side, pool, thr, n_start = int(blend[2]), int(blend[3]), float(blend[4]), int(blend[5])
            if side <= 0:
                raise ValueError("the local blend: side = %d is not a token grid side" % side)
            acc = torch.empty(((1 + n_dec) * B, side, side), device=x0.device, dtype=torch.float32)
            keep = torch.empty((n_dec * B, 1, H, W), device=x0.device, dtype=torch.float32)
            a.blend = C.pointer(_ffi.LocalBlend(sel_src=ptr(sels[0]), sel_tgt=ptr(sels[1]), B_sel=Bs, side=side, pool=pool,
                                                thr=thr, n_start=n_start, acc_out=ptr(acc), keep_out=ptr(keep)))
            outs = (acc, keep)
        gvec, gscalar = self._guidance(dec_guidance, n_dec * B, "n_dec * B", x0.device)
        nz = self._f32(noise) if noise is not None else None
        win = None
        if windows is not None:  # the canvas is x0's own extent; what the table may hold is cd_cycle_translate's to refuse
            win = np.ascontiguousarray(windows, dtype=np.int32)
            if win.ndim != 2 or win.shape[1] != 2:
                raise ValueError("windows must be [n, 2] (y, x) pairs, got shape %s" % (win.shape,))
            a.canvas_h, a.canvas_w, a.n_win, a.win_host = H, W, win.shape[0], win.ctypes.data
        a.net, a.sched_kind, a.x0, a.ctx_len, a.B, a.n_dec, a.K = net, kind, ptr(x0), L, B, n_dec, K
        a.enc_ctx_c, a.enc_ctx_uc, a.enc_guidance = ptr(ctxs[0]), ptr(ctxs[1]), enc_guidance
        a.dec_ctx_c, a.dec_ctx_uc, a.dec_guidance, a.dec_guidance_per_sample = ptr(ctxs[2]), ptr(ctxs[3]), gscalar, ptr(gvec)
        a.coef_enc_host, a.coef_dec_host = coef_enc.ctypes.data, coef_dec.ctypes.data
        a.noise, a.seed, a.last_uses_x0, a.z_out, a.x_out = ptr(nz), seed, int(last_uses_x0), ptr(z), ptr(x)
        check(self.lib.cd_cycle_translate(self.h, C.byref(a)))
        self._keep = (gvec, ctxs, nz, mask, mask_x0, mask_noise, ctl, sels, win)  # the launches read them asynchronously
        return (z, x) + outs

    @staticmethod
    def _guidance(guidance, rows, what, device):
        """(gvec, gscalar) of a decoder guidance: one scale, or `rows` of them on the device when the samples differ in it"""
        if isinstance(guidance, (int, float)):
            return None, float(guidance)
        gvec = torch.as_tensor(guidance, dtype=torch.float32).to(device).contiguous()
        if gvec.numel() != rows or bool(((gvec == 0) | (gvec == 1)).any()):
            raise ValueError("per-sample guidance: %s scales, none of them 0 or 1" % what)
        return gvec, 1.0

    def _mask_args(self, mask, x0, B, qcoef, mask_noise, mask_source, H, W, Cc, K, b_noise=None):
        """checked (mask, x0, B_mask, source id, qcoef, noise) of the masked entry points; `b_noise`: the decoder's batch"""
        b_noise = B if b_noise is None else b_noise
        if mask_source not in _ffi.MASK_SOURCES:
            raise ValueError("mask_source must be one of %s" % sorted(_ffi.MASK_SOURCES))
        mask = self._f32(mask)
        if mask.dim() != 4 or mask.shape[1:] != (1, H, W) or B % mask.shape[0] != 0:
            raise ValueError("mask must be [B_mask, 1, %d, %d] with B_mask dividing %d, got %s" % (H, W, B, tuple(mask.shape)))
        Bm = mask.shape[0]
        if mask_source == "encoder":
            if qcoef is not None or mask_noise is not None:
                raise ValueError("mask_source = 'encoder' takes no q-sample table and no mask noise")
            return mask, None, Bm, _ffi.CD_MASK_ENCODER, None, None
        x0 = self._f32(x0)
        if tuple(x0.shape) != (Bm, Cc, H, W):
            raise ValueError("the blend's x0 must be %s, got %s" % ((Bm, Cc, H, W), tuple(x0.shape)))
        qcoef = np.ascontiguousarray(qcoef, dtype=np.float32)
        if qcoef.shape != (K, 2):
            raise ValueError("q-sample table must be [%d, 2] (DDIMSchedule.coef_qsample), got %s" % (K, qcoef.shape))
        if mask_noise is not None:
            mask_noise = self._f32(mask_noise)
            if tuple(mask_noise.shape) != (K, b_noise, Cc, H, W):
                raise ValueError("mask_noise must be %s, got %s" % ((K, b_noise, Cc, H, W), tuple(mask_noise.shape)))
        return mask, x0, Bm, _ffi.CD_MASK_QSAMPLE, qcoef, mask_noise

    def ddim_decode_masked(self, net, kind, z, coef, mask, x0, qcoef, mask_noise=None, mask_seed=0, n_eps=None, ctx_c=None,
                           ctx_uc=None, guidance=1.0, noise_tail=None, seed=0, mask_source="q_sample"):
        """cd_ddim_decode_masked: ddim_decode with the keep-mask blend x <- src_k*m + (1-m)*x ahead of every forward
        (sample_with_eps(mask=, x0=), ddim.py:427-430). mask [B_mask, 1, H, W] (1 = keep), x0 [B_mask, C, H, W], B_mask
        dividing B; qcoef = DDIMSchedule.coef_qsample(skip); mask_noise [K, B, C, H, W] (slot i = the draw of loop iteration
        i) or None (Philox(mask_seed)). mask_source = "encoder" is refused here: it exists on the coupled loop only."""
        if mask_source == "encoder":
            raise ValueError("mask_source = 'encoder' needs the coupled loop (cycle_translate_masked / translate()): the "
                             "encoder's trajectory no longer exists in a separate decode")
        z = self._f32(z)
        B, T, Cc, H, W = z.shape
        K = len(coef)
        if n_eps is None:
            n_eps = T - 1
        mask, x0, Bm, src, qcoef, mask_noise = self._mask_args(mask, x0, B, qcoef, mask_noise, mask_source, H, W, Cc, K)
        x = torch.empty((B, Cc, H, W), device=z.device, dtype=torch.float32)
        coef = np.ascontiguousarray(coef)
        L = ctx_c.shape[1] if ctx_c is not None else (ctx_uc.shape[1] if ctx_uc is not None else 0)
        cc = self._f32(ctx_c) if ctx_c is not None else None
        cu = self._f32(ctx_uc) if ctx_uc is not None else None
        nt = self._f32(noise_tail) if noise_tail is not None else None
        gvec, gscalar = self._guidance(guidance, B, "B", z.device)
        check(self.lib.cd_ddim_decode_masked(self.h, net, kind, ptr(z), T, n_eps, ptr(cc), ptr(cu), L, C.c_float(gscalar),
                                             ptr(gvec), B, K, C.c_void_p(coef.ctypes.data), ptr(nt), C.c_uint64(seed),
                                             ptr(mask), ptr(x0), Bm, src, C.c_void_p(qcoef.ctypes.data), ptr(mask_noise),
                                             C.c_uint64(mask_seed), ptr(x)))
        self._keep = (gvec, cc, cu, nt, mask, x0, mask_noise)  # the launches read them asynchronously
        return x

    def cycle_translate_masked(self, net, kind, x0, coef_enc, coef_dec, mask, mask_x0=None, qcoef=None, mask_noise=None,
                               mask_seed=0, mask_source="q_sample", enc_ctx_c=None, enc_ctx_uc=None, enc_guidance=1.0,
                               dec_ctx_c=None, dec_ctx_uc=None, dec_guidance=1.0, n_dec=1, noise=None, seed=0,
                               last_uses_x0=True):
        """cd_keep_mask: cycle_translate with the keep-mask on the decoder rows. mask [B_mask, 1, H, W], B_mask
        dividing B. "q_sample": mask_x0 [B_mask, C, H, W], qcoef = coef_qsample(skip), mask_noise [K, n_dec * B, C, H, W] or
        None; "encoder": the kept region follows the encoder's own x_t of every level, nothing else is passed or drawn."""
        # _f32(mask): the mask is not optional here - None is an error, never the unmasked loop
        return self._cycle_translate(net, kind, x0, coef_enc, coef_dec, enc_ctx_c, enc_ctx_uc, enc_guidance, dec_ctx_c, dec_ctx_uc,
                                     dec_guidance, n_dec, noise, seed, last_uses_x0, self._f32(mask), mask_x0, qcoef, mask_noise,
                                     mask_seed, mask_source)

    def cycle_translate_ctrl(self, net, kind, x0, coef_enc, coef_dec, mapper, alpha, weight, n_ctrl, mask=None, mask_x0=None,
                             qcoef=None, mask_noise=None, mask_seed=0, mask_source="q_sample", enc_ctx_c=None, enc_ctx_uc=None,
                             enc_guidance=1.0, dec_ctx_c=None, dec_ctx_uc=None, dec_guidance=1.0, n_dec=1, noise=None, seed=0,
                             last_uses_x0=True):
        """cd_attn_ctrl: cycle_translate (mask=None) or cycle_translate_masked with cross-attention control on the
        first n_ctrl iterations. mapper [B_ctrl, L, L], alpha / weight [B_ctrl, L] (attn_control.build_control), B_ctrl
        dividing B; the decoder's conditional rows take P = w * (alpha * (P_src . M) + (1 - alpha) * P_own) in every text
        cross-attention, P_src from the encoder's conditional row of the same sample in the same forward."""
        return self._cycle_translate(net, kind, x0, coef_enc, coef_dec, enc_ctx_c, enc_ctx_uc, enc_guidance, dec_ctx_c, dec_ctx_uc,
                                     dec_guidance, n_dec, noise, seed, last_uses_x0, mask, mask_x0, qcoef, mask_noise, mask_seed,
                                     mask_source, ctrl=(mapper, alpha, weight, n_ctrl))

    def cycle_translate_blend(self, net, kind, x0, coef_enc, coef_dec, sel_src, sel_tgt, side, pool=3, thr=0.3, n_start=0,
                              ctrl=None, enc_ctx_c=None, enc_ctx_uc=None, enc_guidance=1.0, dec_ctx_c=None, dec_ctx_uc=None,
                              dec_guidance=1.0, n_dec=1, noise=None, seed=0, last_uses_x0=True):
        """cd_local_blend: cycle_translate (or, with ctrl = (mapper, alpha, weight, n_ctrl), cycle_translate_ctrl)
        with prompt-to-prompt's local blend. sel_src / sel_tgt [B_sel, L] weigh the key positions of the source / target
        prompt, B_sel dividing B; the maps of the text cross-attentions of token grid `side` on them are summed over layers and
        steps, and from iteration n_start on every step is followed by x <- x_enc * keep + (1 - keep) * x with keep rebuilt from
        the sums (pool, threshold on the map's own maximum, union of source and target).
        Returns (z, x, acc [(1 + n_dec) * B, side, side], keep [n_dec * B, 1, H, W])."""
        return self._cycle_translate(net, kind, x0, coef_enc, coef_dec, enc_ctx_c, enc_ctx_uc, enc_guidance, dec_ctx_c, dec_ctx_uc,
                                     dec_guidance, n_dec, noise, seed, last_uses_x0, ctrl=ctrl,
                                     blend=(sel_src, sel_tgt, side, pool, thr, n_start))

    def cycle_translate_sega(self, net, kind, x0, coef_enc, coef_dec, edit_ctx, concepts, momentum_scale=0.3, momentum_beta=0.6,
                             ctrl=None, mask=None, mask_x0=None, qcoef=None, mask_noise=None, mask_seed=0,
                             mask_source="q_sample", enc_ctx_c=None, enc_ctx_uc=None, enc_guidance=1.0, dec_ctx_c=None,
                             dec_ctx_uc=None, dec_guidance=1.0, n_dec=1, noise=None, seed=0, last_uses_x0=True):
        """cd_sega: cycle_translate (or, with mask / ctrl = (mapper, alpha, weight, n_ctrl), its masked /
        controlled form) with semantic guidance. edit_ctx [E * n_dec * B, L, Dc] concept-major; concepts: E rows of
        (scale, weight, lo, frac, warm, cool) (semantic_guidance.concept_table). Returns (z, x, tau [K, n_dec * B, E],
        kept [K, n_dec * B, E] int32, mask [n_dec * B, E, C, H, W] of 0 / 1 from the last iteration with an active concept)."""
        return self._cycle_translate(net, kind, x0, coef_enc, coef_dec, enc_ctx_c, enc_ctx_uc, enc_guidance, dec_ctx_c, dec_ctx_uc,
                                     dec_guidance, n_dec, noise, seed, last_uses_x0, mask, mask_x0, qcoef, mask_noise, mask_seed,
                                     mask_source, ctrl=ctrl, sega=(edit_ctx, concepts, momentum_scale, momentum_beta))

    def op_sega_guidance(self, eps_all, concepts, iteration, nu, guidance=1.0, momentum_scale=0.3, momentum_beta=0.6, ld=None,
                         want_mask=True):
        """cd_op_sega_guidance: one iteration's two launches. eps_all [(2 + E) * Bd, C, HW] in batch-row order uncond |
        concepts | cond, nu [Bd, C, HW] (updated in place) -> (eps [Bd, C, HW], tau [Bd, E], kept [Bd, E] int32, mask
        [Bd, E, C, HW] or None)."""
        eps_all, nu = self._f32(eps_all), self._f32(nu)
        table = np.ascontiguousarray(concepts, dtype=_ffi.SEGA_CONCEPT_DTYPE)
        E = len(table)
        rows, Cc, HW = eps_all.shape
        Bd = rows // (2 + E)
        if Bd * (2 + E) != rows or tuple(nu.shape) != (Bd, Cc, HW):
            raise ValueError("eps_all %s / nu %s do not fit E = %d" % (tuple(eps_all.shape), tuple(nu.shape), E))
        gvec, gscalar = (None, float(guidance)) if isinstance(guidance, (int, float)) else \
            (torch.as_tensor(guidance, dtype=torch.float32).to(eps_all.device).contiguous(), 1.0)
        eps = torch.empty((Bd, Cc, HW), device=eps_all.device, dtype=torch.float32)
        tau = torch.empty((Bd, E), device=eps_all.device, dtype=torch.float32)
        kept = torch.empty((Bd, E), device=eps_all.device, dtype=torch.int32)
        mask = torch.empty((Bd, E, Cc, HW), device=eps_all.device, dtype=torch.float32) if want_mask else None
        check(self.lib.cd_op_sega_guidance(self.h, ptr(eps_all), Bd, Cc, HW, E, Cc if ld is None else int(ld), C.c_float(gscalar),
                                           ptr(gvec), C.c_void_p(table.ctypes.data), int(iteration), C.c_float(momentum_scale),
                                           C.c_float(momentum_beta), ptr(nu), ptr(eps), ptr(tau), ptr(kept), ptr(mask)))
        return eps, tau, kept, mask

    def local_blend_mask(self, acc_src, acc_tgt, f=1, pool=3, thr=0.3):
        """cd_op_local_blend_mask: one launch of the blend's mask kernel. acc_src [B, side, side], acc_tgt [Bd, side, side]
        (decoder row r belongs to source row r % B) -> keep [Bd, 1, side * f, side * f] of 0 / 1, 1 = keep the source."""
        a, t = self._f32(acc_src), self._f32(acc_tgt)
        if a.dim() != 3 or t.dim() != 3 or a.shape[1] != a.shape[2] or tuple(t.shape[1:]) != tuple(a.shape[1:]):
            raise ValueError("the sums must be [B, side, side] and [Bd, side, side], got %s and %s"
                             % (tuple(a.shape), tuple(t.shape)))
        side = a.shape[1]
        keep = torch.empty((t.shape[0], 1, side * int(f), side * int(f)), device=a.device, dtype=torch.float32)
        check(self.lib.cd_op_local_blend_mask(self.h, ptr(a), ptr(t), a.shape[0], t.shape[0], side, int(f), int(pool),
                                              C.c_float(thr), ptr(keep)))
        return keep

    def ilvr_decode(self, net, kind, z, coef, ref, down_n, qcoef, range_t=0, n_eps=0, noise_tail=None, seed=0, ref_noise=None,
                    ref_seed=0):
        """cd_ilvr_decode: ddim_decode on an unconditional pixel DDPM with ILVR's low-pass conditioning on the reference image
        `ref` [B_ref, C, R, R] (B_ref dividing B) after the step of every row k > range_t. qcoef = PixelSchedule.coef_ilvr()
        [K, 2]; ref_noise [K, B, C, R, R] (slot i = the draw of loop iteration i) or None (Philox(ref_seed))."""
        z = self._f32(z)
        B, T, Cc, H, W = z.shape
        K = len(coef)
        ref = self._f32(ref)
        if ref.dim() != 4 or tuple(ref.shape[1:]) != (Cc, H, W):
            raise ValueError("the reference image must be [B_ref, %d, %d, %d], got %s" % (Cc, H, W, tuple(ref.shape)))
        qcoef = np.ascontiguousarray(qcoef, dtype=np.float32)
        if qcoef.shape != (K, 2):
            raise ValueError("q-sample table must be [%d, 2] (PixelSchedule.coef_ilvr), got %s" % (K, qcoef.shape))
        nt = self._f32(noise_tail) if noise_tail is not None else None
        if ref_noise is not None:
            ref_noise = self._f32(ref_noise)
            if tuple(ref_noise.shape) != (K, B, Cc, H, W):
                raise ValueError("ref_noise must be %s, got %s" % ((K, B, Cc, H, W), tuple(ref_noise.shape)))
        x = torch.empty((B, Cc, H, W), device=z.device, dtype=torch.float32)
        coef = np.ascontiguousarray(coef)
        check(self.lib.cd_ilvr_decode(self.h, net, kind, ptr(z), T, n_eps, B, K, C.c_void_p(coef.ctypes.data), ptr(nt),
                                      C.c_uint64(seed), ptr(ref), ref.shape[0], int(down_n), int(range_t),
                                      C.c_void_p(qcoef.ctypes.data), ptr(ref_noise), C.c_uint64(ref_seed), ptr(x)))
        self._keep = (z, nt, ref, ref_noise)  # the launches read them asynchronously
        return x

    def op_lowpass(self, x, down_n):
        """cd_op_lowpass: phi_N of fp32 [B, C, R, R] through the two ILVR kernels"""
        x = self._f32(x)
        B, Cc, R, W = x.shape
        assert R == W, x.shape
        y = torch.empty_like(x)
        check(self.lib.cd_op_lowpass(self.h, ptr(x), B, Cc, R, int(down_n), ptr(y)))
        return y

    def gauss(self, seed, stream, n, first=0):
        """cd_op_gauss: the n draws first .. first + n - 1 of Philox(seed, stream), as every noise=None path takes them"""
        out = torch.empty((int(n),), device=self.device, dtype=torch.float32)
        check(self.lib.cd_op_gauss(self.h, C.c_uint64(seed), C.c_uint32(stream), int(first), int(n), ptr(out)))
        return out

    def automask(self, net, x0, ctx_src, ctx_tgt, t, qa, qb, n_draws=10, noise=None, seed=0, max_rows=None, ratio=3.0,
                 thr=0.5, dilate=0, want_map=True):
        """cd_automask: the keep-mask of DiffEdit's first step. x0 [B, C, H, W] noised n_draws times to the level (t, qa, qb),
        the network under ctx_src and under ctx_tgt [B, L, Dc] on each, map = mean |e_tgt - e_src| over draws and channels,
        clipped at ratio x the image's own mean, thresholded and dilated -> (keep [B, 1, H, W] of 0 / 1 with 1 = keep the
        source, map [B, 1, H, W] or None). noise [n_draws, B, C, H, W] or None (Philox(seed), stream 0x6000 + i); max_rows:
        rows of one forward (default: all 2 * n_draws * B)."""
        x0 = self._f32(x0)
        B, Cc, H, W = x0.shape
        cs, ct = self._f32(ctx_src), self._f32(ctx_tgt)
        if cs.dim() != 3 or cs.shape[0] != B or tuple(ct.shape) != tuple(cs.shape):
            raise ValueError("contexts must both be [%d, L, Dc], got %s and %s" % (B, tuple(cs.shape), tuple(ct.shape)))
        if noise is not None:
            noise = self._f32(noise)
            if tuple(noise.shape) != (int(n_draws), B, Cc, H, W):
                raise ValueError("noise must be %s, got %s" % ((int(n_draws), B, Cc, H, W), tuple(noise.shape)))
        keep = torch.empty((B, 1, H, W), device=x0.device, dtype=torch.float32)
        mp = torch.empty_like(keep) if want_map else None
        max_rows = 2 * int(n_draws) * B if max_rows is None else int(max_rows)
        check(self.lib.cd_automask(self.h, net, ptr(x0), ptr(cs), ptr(ct), cs.shape[1], B, int(n_draws), int(t), C.c_float(qa),
                                   C.c_float(qb), ptr(noise), C.c_uint64(seed), max_rows, C.c_float(ratio), C.c_float(thr),
                                   int(dilate), ptr(mp), ptr(keep)))
        self._keep = (x0, cs, ct, noise)  # the launches read them asynchronously
        return keep, mp

    def word_maps(self, net, x0, ctx, sel, t, qa, qb, n_draws=4, noise=None, seed=0, max_rows=None, sides=(0, 0)):
        """cd_word_maps: per-word heat maps of the text cross-attention. x0 [B, C, h, w] noised n_draws times to the level
        (t, qa, qb), one conditional forward under ctx [B, L, Dc]; in every transformer block whose token grid side lies in
        sides = (min, max) ((0, 0): all) the softmax mass on the key positions sel [B_sel, N, L] marks, averaged over heads,
        blocks and draws -> (maps [B, N, h, w], number of blocks included). noise [n_draws, B, C, h, w] or None (Philox(seed),
        stream 0x8000 + i); max_rows: rows of one forward (default: all n_draws * B)."""
        x0 = self._f32(x0)
        B, Cc, H, W = x0.shape
        cx, sel = self._f32(ctx), self._f32(sel)
        if cx.dim() != 3 or cx.shape[0] != B:
            raise ValueError("the context must be [%d, L, Dc], got %s" % (B, tuple(cx.shape)))
        if sel.dim() != 3 or sel.shape[2] != cx.shape[1]:
            raise ValueError("the selector must be [B_sel, N, %d], got %s" % (cx.shape[1], tuple(sel.shape)))
        if noise is not None:
            noise = self._f32(noise)
            if tuple(noise.shape) != (int(n_draws), B, Cc, H, W):
                raise ValueError("noise must be %s, got %s" % ((int(n_draws), B, Cc, H, W), tuple(noise.shape)))
        N = sel.shape[1]
        maps = torch.empty((B, N, H, W), device=x0.device, dtype=torch.float32)
        max_rows = int(n_draws) * B if max_rows is None else int(max_rows)
        n_layers = C.c_int(0)
        check(self.lib.cd_word_maps(self.h, net, ptr(x0), ptr(cx), cx.shape[1], B, ptr(sel), sel.shape[0], N, int(n_draws),
                                    int(t), C.c_float(qa), C.c_float(qb), ptr(noise), C.c_uint64(seed), max_rows,
                                    int(sides[0]), int(sides[1]), ptr(maps), C.byref(n_layers)))
        self._keep = (x0, cx, sel, noise)  # the launches read them asynchronously
        return maps, n_layers.value

    def cross_attention_maps(self, q, k, sel, H, L=None, scale=None, q_log2=False):
        """cd_op_cross_attention_maps: one launch of the map kernel. q [B, Tq, H*D], k [B, L_buf, H*D] (the first L rows are the
        keys), sel [B_sel, N, L] -> maps [B, N, Tq] = head mean of sum_j sel[b % B_sel, n, j] softmax(q k^T scale)[q, j]."""
        q, k, sel = self._f32(q), self._f32(k), self._f32(sel)
        B, Tq, Cq = q.shape
        D = Cq // H
        L = k.shape[1] if L is None else int(L)
        if sel.dim() != 3 or sel.shape[2] != L or k.shape[0] != B or k.shape[2] != Cq:
            raise ValueError("q %s, k %s, sel %s with L = %d" % (tuple(q.shape), tuple(k.shape), tuple(sel.shape), L))
        scale = D ** -0.5 if scale is None else float(scale)
        maps = torch.empty((B, sel.shape[1], Tq), device=q.device, dtype=torch.float32)
        check(self.lib.cd_op_cross_attention_maps(self.h, ptr(q), ptr(k), ptr(sel), B, sel.shape[0], H, Tq, L, k.shape[1], D,
                                                  sel.shape[1], C.c_float(scale), int(bool(q_log2)), ptr(maps)))
        return maps

    def op_automask_reduce(self, eps_src, eps_tgt, ratio=3.0, thr=0.5, dilate=0):
        """cd_op_automask_reduce: the reduction of automask() on fp32 [n, B, C, H, W] predictions -> (keep, map [B, 1, H, W],
        mean [B])"""
        es, et = self._f32(eps_src), self._f32(eps_tgt)
        if es.dim() != 5 or tuple(es.shape) != tuple(et.shape):
            raise ValueError("predictions must both be [n, B, C, H, W], got %s and %s" % (tuple(es.shape), tuple(et.shape)))
        n, B, Cc, H, W = es.shape
        keep = torch.empty((B, 1, H, W), device=es.device, dtype=torch.float32)
        mp, mean = torch.empty_like(keep), torch.empty((B,), device=es.device, dtype=torch.float32)
        check(self.lib.cd_op_automask_reduce(self.h, ptr(es), ptr(et), n, B, Cc, H, W, C.c_float(ratio), C.c_float(thr),
                                             int(dilate), ptr(mp), ptr(mean), ptr(keep)))
        return keep, mp, mean

    def pix_refine(self, net, kind, x, coef, noise=None, seed=0):
        x = self._f32(x).clone()
        R = len(coef) - 1
        coef = np.ascontiguousarray(coef)
        check(self.lib.cd_pix_refine(self.h, net, kind, ptr(x), x.shape[0], R, C.c_void_p(coef.ctypes.data),
                                     ptr(self._f32(noise)) if noise is not None else None, C.c_uint64(seed)))
        return x

    def prof_enable(self, on=True):
        check(self.lib.cd_prof_enable(self.h, int(on)))

    def prof_collect(self):
        """(launches, total_ms, total_flops) of the implicit-GEMM kernel since prof_enable."""
        n, ms, fl = C.c_int(), C.c_double(), C.c_double()
        check(self.lib.cd_prof_collect(self.h, C.byref(n), C.byref(ms), C.byref(fl)))
        return n.value, ms.value, fl.value

    def mfma_sustained(self, target_ms=300):
        """(TFLOP/s, GHz) of a bare 16-bit MFMA loop on every CU for ~target_ms: what this device's matrix cores sustain
        under its power cap (csrc/diag.hip). Measurement support for bench.py, not part of the path."""
        tf, ghz = C.c_float(), C.c_float()
        check(self.lib.cd_op_bench_mfma_sustained(self.h, int(target_ms), C.byref(tf), C.byref(ghz)))
        return tf.value, ghz.value

    def workspace_high_water(self):
        v = C.c_size_t()
        check(self.lib.cd_engine_workspace_high_water(self.h, C.byref(v)))
        return v.value
