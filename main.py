"""Evaluation driver: config + triplet JSON -> translated images + metrics, on the HIP engine.

A compact stand-in for the reference's `main.py --do_eval` (HF Trainer harness, main.py:57-160,
trainer/trainer.py:793-900): same experiment configs (`--cfg experiments/*.cfg`), same model API, same per-rank
sharding (HF ShardSampler: global batches of B * world split contiguously, last one padded by wrap-around) and the same per-image metrics (evaluation/translate_text.py: PSNR, SSIM,
L2 against the input; CLIP / directional CLIP when the config selects `ranker = directional_clip`).

  python main.py --cfg experiments/toy_ddpm_c1.cfg --data triplets.json --output_dir out [--per_device_eval_batch_size 4]
  python -m torch.distributed.run --nproc-per-node 8 main.py ...        # one process per GPU

`--fold N` is the engine's look-ahead: N consecutive dataloader batches of this rank run as ONE model() call (the operating
point bench.py's headline is measured at: 16 batches of 4 = 64 images through the DPM-Encoder, 128 rows through the guided
decode), and the outputs are split back per sample. The reference's driver issues one batch per call
(trainer/trainer.py:788-833 with --per_device_eval_batch_size 4, README.md:153); the samples of a batch are independent, so
folding changes no result beyond kernel summation order. To make that checkable, every SAMPLE owns its noise stream (a
device generator seeded by --seed and the sample id): a run's images do not depend on --fold, on the batch size, on the
number of ranks, or on which rank / batch / slot a sample lands in - including the duplicates the sampler's wrap-around
padding creates (they reproduce the original's image and are not written a second time).
"""
import argparse
import json
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


class SampleStreams:
    """noise_source of the wrappers: one generator per SAMPLE of a (folded) call, seeded by (--seed, sample id); a draw of
    shape [n samples, ...] is the concatenation of each sample's own [1, ...] draw - what that sample draws in any other
    call, batch, slot or rank (round-5 advisor: per-batch streams keyed by the batch's first id made a wrap-around duplicate
    that lands in another batch position draw other noise than its original, and then overwrite it)"""

    def __init__(self, seed, sample_ids, device):
        self.device = device
        self.gens = [torch.Generator(device=device).manual_seed((seed * 1000003 + 7919 * int(i)) % (2 ** 63))
                     for i in sample_ids]

    def __call__(self, shape):
        assert shape[0] == len(self.gens), (shape, len(self.gens))
        return torch.cat([torch.randn((1,) + tuple(shape[1:]), generator=g, device=self.device) for g in self.gens], 0)


def folded_calls(model, batches, fold, seed, device):
    """The look-ahead loop: `batches` (an iterable of collated dataloader batches of this rank, in order; pulled `fold` at a
    time, so a generator keeps host memory at one folded call) run `fold` at a time as ONE model() call; yields (batch dict of
    the folded call, original images, translated images). Every wrapper of the model that has a `noise_source` hook draws
    from the per-sample streams above."""
    import itertools
    wrappers = [w for w in (getattr(model, "gan_wrapper", None), getattr(model, "source_gan_wrapper", None),
                            getattr(model, "target_gan_wrapper", None)) if w is not None]
    fold = max(1, int(fold))
    it = iter(batches)
    while True:
        parts = list(itertools.islice(it, fold))
        if not parts:
            break
        batch = {"sample_id": torch.cat([p["sample_id"] for p in parts]),
                 "original_image": torch.cat([p["original_image"] for p in parts])}
        for k in ("encode_text", "decode_text"):
            if k in parts[0]:
                batch[k] = [t for p in parts for t in p[k]]
        for k in ("is_padding",):  # host-side bookkeeping of the driver: passed through, never handed to the model
            if k in parts[0]:
                batch[k] = [t for p in parts for t in p[k]]
        if any("mask" in p for p in parts):  # keep-masks (data/triplets.py): all-zero for the batches that have none
            batch["mask"] = torch.cat([p["mask"] if "mask" in p else torch.zeros_like(p["original_image"][:, :1]) for p in parts])
            batch["has_mask"] = [t for p in parts for t in p.get("has_mask", [False] * p["sample_id"].shape[0])]
        streams = SampleStreams(seed, batch["sample_id"].tolist(), device)
        for w in wrappers:
            if hasattr(w, "noise_source"):
                w.noise_source = streams
        kw = {"sample_id": batch["sample_id"].to(device), "original_image": batch["original_image"].to(device)}
        if "encode_text" in batch:
            kw.update(encode_text=batch["encode_text"], decode_text=batch["decode_text"])
        if "mask" in batch:
            kw.update(mask=batch["mask"].to(device))
        with torch.no_grad():
            (orig, img), _loss, _ = model(**kw)
        if "mask" not in batch:  # `[gan] auto_mask`: the keep-mask the wrapper estimated for this call, as pixels
            for w in wrappers:
                if getattr(getattr(w, "auto_mask_opts", None), "on", False) and w.last_auto_mask is not None:
                    f = w.vae_factor  # nearest x f: every latent pixel becomes its f x f block
                    batch["auto_keep"] = w.last_auto_mask.repeat_interleave(f, 2).repeat_interleave(f, 3).cpu()
                # `[gan] local_blend = words`: the final mask of the blend takes the same path (first candidate's)
                if getattr(w, "local_blend", "none") != "none" and getattr(w, "last_local_blend_mask", None) is not None:
                    f = w.vae_factor
                    batch["auto_keep"] = w.last_local_blend_mask.repeat_interleave(f, 2).repeat_interleave(f, 3).cpu()
        # `[gan] edit_concepts`: per concept the channel-max of the first candidate's final edit mask, as pixels
        for w in wrappers:
            if getattr(w, "edit_concepts", None) and getattr(w, "last_edit_masks", None):
                f = w.vae_factor
                batch["edit_masks"] = w.last_edit_masks[0].amax(2).repeat_interleave(f, 2).repeat_interleave(f, 3).cpu()
        yield batch, orig, img


def word_map_images(wrapper, orig, text, other_text, seed):
    """--word_maps: uint8 [B, R, R] heat maps of the words `text` introduces against `other_text`, taken on the source images
    `orig` (in [0, 1]) encoded with the posterior mean, as forward(mask=) encodes them; every image divided by its own
    maximum and nearest-upsampled to the image size"""
    img = ((orig - 0.5) * 2.0).to(wrapper.device, torch.float32)
    per = wrapper._vae_batch()
    with torch.no_grad():
        x0 = torch.cat([wrapper.engine.vae_encode(wrapper.vae, img[i:i + per], sample=False, scale=wrapper.SCALE_FACTOR)
                        for i in range(0, img.shape[0], per)], 0)
        m = wrapper.word_maps(x0, list(text), other_text=list(other_text), seed=seed)[:, 0]
    m = m / m.amax(dim=(1, 2), keepdim=True).clamp_min(torch.finfo(torch.float32).tiny)
    f = wrapper.vae_factor
    m = m.repeat_interleave(f, 1).repeat_interleave(f, 2)
    return (m * 255 + 0.5).clamp(0, 255).to(torch.uint8).cpu()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", required=True)
    ap.add_argument("--data", required=True, help="JSON list of {img_path[, encode_text, decode_text]}")
    ap.add_argument("--output_dir", default="output")
    ap.add_argument("--per_device_eval_batch_size", type=int, default=4)
    ap.add_argument("--range", type=int, nargs=2, default=None, metavar=("START", "END"))
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--fold", type=int, default=1,
                    help="look-ahead: run N consecutive batches of this rank as one model() call (larger GEMMs; bench.py's "
                         "headline operating point is --per_device_eval_batch_size 4 --fold 16; under the reference's own Trainer "
                         "the same launch sets are reached with --per_device_eval_batch_size 64); results per image are those of "
                         "--fold 1 up to kernel summation order")
    ap.add_argument("--grid", action="store_true",
                    help="also write the reference's multi_image pair grids (original | translated, 8 per row)")
    ap.add_argument("--synthetic-weights", action="store_true",
                    help="run on seeded synthetic weights when a checkpoint file is missing (default: error, as the "
                         "reference's torch.load); recorded as weights_origin in metrics.json")
    ap.add_argument("--fid_ref_dir", default=None,
                    help="target-domain images (png / jpg, searched recursively): adds FID / KID of the written outputs "
                         "against them to metrics.json (evaluation/translate_to_dog.py); Inception-v3 on the engine")
    ap.add_argument("--fid_ref_stats", default=None,
                    help="npz cache of the reference images' Inception features (read if present, else written)")
    ap.add_argument("--fid_inception", default=None,
                    help="Inception-v3 state_dict for FID / KID (pytorch-fid pt_inception-2015-12-05-*.pth; default "
                         "CYCLEDIFF_FID_INCEPTION, or seeded synthetic weights with --synthetic-weights)")
    ap.add_argument("--lpips", default=None, choices=("alex", "vgg"),
                    help="adds per-sample LPIPS v0.1 of the written output against the source image (at the wrapper's "
                         "resolution) to metrics.json, and `lpips_keep` for samples with a keep-mask; backbone on the engine")
    ap.add_argument("--lpips_weights", default=None, metavar="PATH[,PATH]",
                    help="LPIPS weights: one full lpips.LPIPS state_dict, or backbone.pth,linear.pth (default "
                         "CYCLEDIFF_LPIPS_WEIGHTS, or seeded synthetic weights with --synthetic-weights)")
    ap.add_argument("--save_masks", action="store_true",
                    help="`[gan] auto_mask = diffedit`: also write every sample's estimated keep-mask, upsampled to the image "
                         "(white = kept), as <id>_mask.png beside its image; `[gan] edit_concepts`: every concept's final edit "
                         "mask (channel maximum, white = edited) as edit_masks/<id>_<e>.png")
    ap.add_argument("--text_metrics", action="store_true",
                    help="text tasks: per-sample CLIP and directional CLIP (evaluation/translate_text.py) on the unclamped "
                         "outputs; ViT-B/32 weights from CYCLEDIFF_CLIP_RANKER")
    ap.add_argument("--word_maps", action="store_true",
                    help="text tasks: also write every sample's cross-attention heat map of the words its target prompt "
                         "introduces (against the source prompt), on the source image, as word_maps/<id>.png")
    ap.add_argument("--canvas", default=None, metavar="HxW",
                    help="`[gan] window_stride > 0` (fused windows): load every image as H x W pixels - the largest centred "
                         "rectangle of that aspect, resized - instead of the wrapper's square resolution, e.g. 512x768")
    a = ap.parse_args(argv)
    canvas = None
    if a.canvas is not None:
        try:
            canvas = tuple(int(v) for v in a.canvas.lower().split("x"))
        except ValueError:
            canvas = ()
        if len(canvas) != 2 or min(canvas) <= 0:
            ap.error("--canvas takes HxW in pixels, e.g. 512x768, got %r" % (a.canvas,))
    if a.synthetic_weights:
        os.environ["CYCLEDIFF_SYNTHETIC_WEIGHTS"] = "1"

    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world)

    import cycle_diffusion_amd  # noqa: F401
    from cycle_diffusion_amd.data.triplets import TripletDataset, collate
    from cycle_diffusion_amd.parallel import shard_indices, shard_padding
    from cycle_diffusion_amd.utils import metrics
    from cycle_diffusion_amd.utils.config_utils import get_config
    from cycle_diffusion_amd.utils.program_utils import get_model

    args = get_config(a.cfg, config_root=os.path.join(ROOT, "config"))
    torch.manual_seed(a.seed)  # same weights / streams on every rank (main.py:66 set_seed)
    model = get_model(args.model.name)(args).eval()
    wrapper = getattr(model, "gan_wrapper", None) or model.source_gan_wrapper
    start, end = a.range if a.range else (0, None)
    if canvas is not None and not getattr(wrapper, "window_stride", 0):
        raise SystemExit("--canvas needs a [gan] window_stride > 0 (fused windows): without it the wrapper takes its square "
                         "resolution only")
    ds = TripletDataset(a.data, canvas or wrapper.resolution, start, end)
    os.makedirs(a.output_dir, exist_ok=True)
    dev = torch.device("cuda", local)
    rows, grid_pairs = [], []
    import time
    t_start, n_done = time.perf_counter(), 0
    steps = shard_indices(len(ds), a.per_device_eval_batch_size, world, rank)
    pads = shard_padding(len(ds), a.per_device_eval_batch_size, world, rank)

    def batches():  # decoded and collated as the loop pulls them: host memory holds one folded call, not the shard
        for step_idx, pad in zip(steps, pads):
            b = collate([ds[i] for i in step_idx])
            b["is_padding"] = list(pad)
            yield b

    fid_net = fid_origin = ranker = None
    engine = getattr(wrapper, "engine", None)
    lpips_net = lpips_origin = None
    if a.fid_ref_dir or a.text_metrics or a.lpips:
        from cycle_diffusion_amd.runtime import get_engine
        engine = engine or get_engine(dev)
    if a.fid_ref_dir:
        from cycle_diffusion_amd.utils import fid
        fid_net, fid_origin = fid.load_inception(engine, a.fid_inception)
    if a.lpips:
        from cycle_diffusion_amd.utils import lpips
        lpips_net, lpips_origin = lpips.load_lpips(engine, a.lpips, a.lpips_weights)
    if a.text_metrics:
        from cycle_diffusion_amd.utils import text_metrics
        ranker = getattr(wrapper, "ranker", None)
        if not hasattr(ranker, "features"):
            ranker = text_metrics.make_ranker(engine)

    grid_cap = 100 * a.per_device_eval_batch_size  # the reference keeps 100 dataloader batches for its grids
    for batch, orig, img in folded_calls(model, batches(), a.fold, a.seed, dev):
        n_done += img.shape[0]
        if a.grid and rank == 0 and sum(p[0].shape[0] for p in grid_pairs) < grid_cap:
            grid_pairs.append((orig.detach().clamp(0, 1).cpu(), img.detach().clamp(0, 1).cpu()))
        keep = [j for j in range(img.shape[0]) if not batch["is_padding"][j]]
        feats = fid.features(engine, fid_net, img[keep]) if fid_net is not None and keep else None
        lp = lp_keep = None
        if lpips_net is not None and keep:
            lp = lpips.distance(engine, lpips_net, img[keep], orig[keep])
            # this project's definition: both images times the keep-mask in [-1, 1] space (the edit region mid-grey in both)
            km = [batch["mask"][j] if "mask" in batch and batch["has_mask"][j] else
                  batch["auto_keep"][j] if "auto_keep" in batch else None for j in keep]
            sel = [i for i, m in enumerate(km) if m is not None]
            if sel:
                idx = [keep[i] for i in sel]
                d = lpips.distance_keep(engine, lpips_net, img[idx], orig[idx], torch.stack([km[i] for i in sel]))
                lp_keep = {keep[i]: float(v) for i, v in zip(sel, d)}
        heat = None
        if a.word_maps and "encode_text" in batch and hasattr(wrapper, "word_maps"):
            heat = word_map_images(wrapper, orig, batch["decode_text"], batch["encode_text"], a.seed)
            os.makedirs(os.path.join(a.output_dir, "word_maps"), exist_ok=True)
        scores = None
        if ranker is not None and "encode_text" in batch:
            scores = text_metrics.text_scores(ranker, img, orig, batch["encode_text"], batch["decode_text"])
        for j in range(img.shape[0]):
            if batch["is_padding"][j]:  # wrap-around padding of the last global batch: its original is written elsewhere
                continue
            o, g = orig[j].clamp(0, 1).cpu(), img[j].clamp(0, 1).cpu()
            sid = int(batch["sample_id"][j])
            row = {"sample_id": sid, "psnr": float(metrics.calculate_psnr(g, o)),
                   "ssim": float(metrics.calculate_ssim(g.permute(1, 2, 0) * 255, o.permute(1, 2, 0) * 255)),
                   "l2": float(metrics.calculate_l2(g, o))}
            for k in ("encode_text", "decode_text"):
                if k in batch:
                    row[k] = batch[k][j]
            if "mask" in batch and batch["has_mask"][j]:  # PSNR against the input inside / outside the kept region
                keep_px = (batch["mask"][j] >= 0.5).expand_as(o)
                for k, sel in (("psnr_keep", keep_px), ("psnr_edit", ~keep_px)):
                    if bool(sel.any()):
                        row[k] = float(metrics.calculate_psnr(g[sel], o[sel]))
            if "auto_keep" in batch:  # the same against the estimated keep-mask, and the share of the image it edits
                keep_px = (batch["auto_keep"][j] >= 0.5).expand_as(o)
                for k, sel in (("psnr_keep", keep_px), ("psnr_edit", ~keep_px)):
                    if bool(sel.any()):
                        row[k] = float(metrics.calculate_psnr(g[sel], o[sel]))
                row["edit_fraction"] = float(1.0 - batch["auto_keep"][j].mean())
                if a.save_masks:
                    from PIL import Image
                    Image.fromarray((batch["auto_keep"][j, 0].numpy() * 255).astype("uint8")).save(
                        os.path.join(a.output_dir, "%06d_mask.png" % sid))
            if a.save_masks and "edit_masks" in batch:  # white = the elements concept e edited in its last active iteration
                from PIL import Image
                os.makedirs(os.path.join(a.output_dir, "edit_masks"), exist_ok=True)
                for e in range(batch["edit_masks"].shape[1]):
                    Image.fromarray((batch["edit_masks"][j, e].numpy() * 255).astype("uint8")).save(
                        os.path.join(a.output_dir, "edit_masks", "%06d_%d.png" % (sid, e)))
            if lp is not None:
                row["lpips"] = float(lp[keep.index(j)])
                if lp_keep is not None and j in lp_keep:
                    row["lpips_keep"] = lp_keep[j]
            if scores is not None:
                row["clip"], row["d-clip"] = scores[0][j], scores[1][j]
            if feats is not None:
                row["_inception"] = feats[keep.index(j)]  # travels with the row to rank 0, dropped before writing
            rows.append(row)
            from PIL import Image
            if heat is not None:
                Image.fromarray(heat[j].numpy()).save(os.path.join(a.output_dir, "word_maps", "%06d.png" % sid))
            Image.fromarray((g.permute(1, 2, 0).numpy() * 255 + 0.5).astype("uint8")).save(
                os.path.join(a.output_dir, "%06d.png" % sid))
    torch.cuda.synchronize(dev)
    wall = time.perf_counter() - t_start  # translation + per-image metrics + PNG writes of this rank
    if world > 1:
        gathered = [None] * world
        dist.all_gather_object(gathered, rows)
        rows = [r for part in gathered for r in part]
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0 and grid_pairs:
        from cycle_diffusion_amd.utils.visualize import visualize
        visualize((torch.cat([p[0] for p in grid_pairs]), torch.cat([p[1] for p in grid_pairs])), "eval", a.output_dir, 0)
    if rank == 0:
        assert len({r["sample_id"] for r in rows}) == len(rows)  # padding rows were skipped where they were produced
        rows.sort(key=lambda r: r["sample_id"])
        summary = {k: sum(r[k] for r in rows) / max(1, len(rows)) for k in ("psnr", "ssim", "l2")}
        for k in ("psnr_keep", "psnr_edit", "edit_fraction", "lpips_keep"):  # only when masked / auto-masked samples exist
            masked = [r[k] for r in rows if k in r]
            if masked:
                summary[k] = sum(masked) / len(masked)
        extra = {}
        if a.text_metrics:
            scored = [r for r in rows if "clip" in r]
            if scored:
                for k in ("clip", "d-clip"):
                    summary[k] = sum(r[k] for r in scored) / len(scored)
            extra["text_metrics"] = {"n": len(scored), "weights_origin": getattr(ranker, "weights_origin", None)}
        if a.lpips:
            scored = [r["lpips"] for r in rows if "lpips" in r]
            if scored:
                summary["lpips"] = sum(scored) / len(scored)
            extra["lpips_eval"] = {"net": a.lpips, "weights_origin": lpips_origin, "n": len(scored)}
        if fid_net is not None:
            import numpy as np
            gen = np.stack([r.pop("_inception") for r in rows])
            ref = None
            if a.fid_ref_stats and os.path.exists(a.fid_ref_stats):
                ref = np.load(a.fid_ref_stats)["features"]
            if ref is None:
                ref = fid.features_u8(engine, fid_net, fid.load_reference_images(a.fid_ref_dir, wrapper.resolution))
                if a.fid_ref_stats:
                    np.savez(a.fid_ref_stats, features=ref)
            r = fid.fid_kid(gen, ref)
            summary.update(fid=r["fid"], kid=r["kid"], fid_sqrtm_imag=r["fid_sqrtm_imag"])
            extra["fid_eval"] = {"n_gen": r["n_gen"], "n_ref": r["n_ref"], "weights_origin": fid_origin}
        with open(os.path.join(a.output_dir, "metrics.json"), "w") as fh:
            json.dump({"summary": summary, "weights_origin": getattr(wrapper, "weights_origin", None), **extra,
                       "samples": rows}, fh, indent=1)
        print(json.dumps({"n": len(rows), **summary, "seconds": wall, "images_per_s_this_rank": n_done / wall}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
