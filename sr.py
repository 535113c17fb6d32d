#!/usr/bin/env python
"""``sr.py -p val -c config/sid.yaml --checkpoint <prefix>`` — validation entry point.

Counterpart of the reference's ``sr.py`` val branch (sr.py:320-400, 505-586): same flags, same YAML
schema, same per-image outputs ``{results}/{fname}_{name}_{sr,hr,lr,inf}.jpg`` and the
``# Validation # PSNR/SSIM`` log lines; ``--niqe`` adds the no-reference score of the reference's ``eval1.py``, ``--lpips`` its LPIPS.  One process per GPU; with N ranks
(``python -m torch.distributed.run --nproc-per-node N sr.py ...``):
  * images small enough for one denoiser call are strided over ranks like the reference's EnlargedSampler
    (data/data_sampler.py:44-45), no data-path collective;
  * images that take the inter-step patch split (padded area > 1024^2, model/ucdir.py:298) are restored by ALL ranks
    together: the windows of every step are sharded over the ranks with one RCCL all-gather per step
    (ucdir_amd/patch.py), every rank draws the same noise; rank 0 writes the outputs.
Training (``-p train``) is out of scope for this build.

Without a checkpoint (none ships with the reference) ``--synthetic-weights`` fills the network with
the deterministic generator used by the tests, so the plumbing can be exercised end to end.
"""
import argparse
import logging
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from ucdir_amd import config as Config  # noqa: E402
from ucdir_amd import metrics as Metrics  # noqa: E402
from ucdir_amd import model as Model  # noqa: E402
from ucdir_amd.data import ImagenetJPGDataset, ImagenetSRDataset, PairDataset, RealESRGANDataset  # noqa: E402

VAL_DATASETS = {"PairDataset": PairDataset, "ImagenetJPGDataset": ImagenetJPGDataset, "ImagenetSRDataset": ImagenetSRDataset,
                "RealESRGANDataset": RealESRGANDataset}


def item_hw(item):
    """(H, W) of the image a val item is restored at: its SR, or the gt of a gt / lq item (DDPM_realsr scales lq up to it)."""
    return tuple((item["SR"] if "SR" in item else item["gt"]).shape[-2:])


def make_val_dataset(val_opt, decode_device="cpu"):
    """The val loader named by ``datasets.val.datasetname`` (reference data/__init__.py:59-61; absent: PairDataset).
    ``decode_device``: where the ImageNet loaders decode their JPEG files; PairDataset ignores it."""
    name = val_opt.get("datasetname") or "PairDataset"
    if name not in VAL_DATASETS:
        raise ValueError("datasets.val.datasetname %r is not supported by -p val (known: %s)" % (name, ", ".join(VAL_DATASETS)))
    if VAL_DATASETS[name] is PairDataset:
        return PairDataset(val_opt["data_args"], phase="val")
    return VAL_DATASETS[name](val_opt["data_args"], phase="val", decode_device=decode_device)


def apply_sampler_flags(opt, args):
    """--sampler / --sampler-steps / --sampler-order / --ddim-eta override the keys of model.sampler (DDPM.__init__ reads it);
    --sampler-threshold / --sampler-threshold-max / --sampler-threshold-ratio those of its ``thresholding`` mapping."""
    over = {"name": args.sampler, "steps": args.sampler_steps, "order": args.sampler_order, "eta": args.ddim_eta}
    over = {k: v for k, v in over.items() if v is not None}
    thr = {"kind": args.sampler_threshold, "max_val": args.sampler_threshold_max, "ratio": args.sampler_threshold_ratio}
    thr = {k: v for k, v in thr.items() if v is not None}
    if over or thr:
        spec = dict(opt["model"].get("sampler") or {})
        spec.update(over)
        if thr:
            was = spec.get("thresholding")
            spec["thresholding"] = dict({"kind": was} if isinstance(was, str) else (was or {}), **thr)
        opt["model"]["sampler"] = spec
    return opt


def image_seed_base(seed):
    """Base of the per-image noise seeds: ``seed`` when given, else a draw from torch's CPU generator.  With an initialised process
    group of more than one rank the draw is rank 0's, broadcast to all: every rank must derive the same streams (a sharded image's
    x_T and step noise), and a rank whose CPU generator was consumed earlier would otherwise draw another base."""
    if seed is not None:
        return seed
    base = int(torch.randint(0, 2 ** 31, (1,)).item())
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
        t = torch.tensor([base], dtype=torch.int64, device=dev)
        dist.broadcast(t, src=0)
        base = int(t.item())
    return base


def parse_val_loss_steps(text, T):
    """``--val-loss-t 1,50,...`` -> the list of steps, each in [1, T]; None when the flag is absent."""
    if text is None:
        return None
    try:
        ts = [int(v) for v in text.split(",") if v.strip()]
    except ValueError:
        raise SystemExit("--val-loss-t wants comma-separated integers, got %r" % text)
    if not ts or any(not 1 <= t <= T for t in ts):
        raise SystemExit("--val-loss-t: every step must lie in [1, %d], got %r" % (T, text))
    return ts


def val_loss_table(opt, which):
    """The noise levels the loss is evaluated on (``--val-loss-schedule``): sqrt of the cumulative alpha product of
    ``model.beta_schedule[which]`` with a leading 1 - the trainer's ``sqrt_alphas_cumprod_prev`` for ``train`` - built here, so the
    sampler's buffers (set for the val schedule) are not touched."""
    from ucdir_amd.diffusion import make_beta_schedule
    so = opt["model"]["beta_schedule"][which]
    betas = make_beta_schedule(schedule=so["schedule"], n_timestep=so["n_timestep"], linear_start=so["linear_start"], linear_end=so["linear_end"])
    return np.sqrt(np.append(1.0, np.cumprod(1.0 - betas, axis=0)))


def val_index_line(i, l_pix=None):
    """The per-image val log line; ``l_pix`` is appended only under ``--val-loss``."""
    return "val index %d" % i if l_pix is None else "val index %d l_pix: %.4e" % (i, l_pix)


def make_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("-c", "--config", type=str, default="config/sid.yaml")
    parser.add_argument("-p", "--phase", type=str, choices=["train", "val"], default="val")
    parser.add_argument("-gpu", "--gpu_ids", type=str, default=None)
    parser.add_argument("-debug", "-d", action="store_true")
    parser.add_argument("-enable_wandb", action="store_true")
    parser.add_argument("-log_wandb_ckpt", action="store_true")
    parser.add_argument("-log_eval", action="store_true")
    parser.add_argument("--local_rank", type=int, default=0)
    parser.add_argument("-launcher", default="pytorch")
    parser.add_argument("--checkpoint", type=str, default=None)
    parser.add_argument("--synthetic-weights", action="store_true",
                        help="fill netG with the deterministic test weights (no checkpoint ships with the reference)")
    parser.add_argument("--max-images", type=int, default=-1)
    parser.add_argument("--batch", type=int, default=16,
                        help="restore up to this many same-sized val images per DDPM.test call (1: the reference's one-by-one loop)")
    parser.add_argument("--seed", type=int, default=None, help="base of the per-image noise seeds (default: drawn from torch's CPU generator on rank 0)")
    parser.add_argument("--sampler", choices=["ddpm", "ddim", "dpm_solver++"], default=None,
                        help="restore with this sampler (overrides model.sampler of the YAML; ddpm: the T-step ancestral sampler)")
    parser.add_argument("--sampler-steps", type=int, default=None, help="network calls of a ddim / dpm_solver++ restoration")
    parser.add_argument("--sampler-order", type=int, choices=[1, 2], default=None, help="dpm_solver++ multistep order")
    parser.add_argument("--ddim-eta", type=float, default=None, help="ddim noise scale (0: deterministic, 1: the reference's setting)")
    parser.add_argument("--sampler-threshold", choices=["none", "static", "dynamic"], default=None,
                        help="dpm_solver++ x0 correction: clamp to +-max (static) or Imagen's dynamic thresholding (per-image quantile)")
    parser.add_argument("--sampler-threshold-max", type=float, default=None, help="max value of the x0 correction (default 1)")
    parser.add_argument("--sampler-threshold-ratio", type=float, default=None, help="quantile of dynamic thresholding (default 0.995)")
    parser.add_argument("--metrics-device", choices=["cpu", "gpu"], default="cpu",
                        help="score PSNR / SSIM on the host (numpy / scipy) or on the GPU (HIP kernel, the same uint8 images)")
    parser.add_argument("--jpeg-device", choices=["cpu", "gpu"], default="cpu",
                        help="write the sr / hr / lr / inf JPEGs with Pillow on the host or encode them on the GPU (HIP baseline encoder, "
                             "the same bytes)")
    parser.add_argument("--decode-device", choices=["cpu", "gpu"], default="cpu",
                        help="decode the input JPEGs of the ImageNet val loaders with Pillow on the host or on the GPU (HIP baseline "
                             "decoder, the same pixels; files it does not take fall back to Pillow one by one)")
    parser.add_argument("--decode-batch", type=int, default=1,
                        help="with --decode-device gpu: decode the input JPEGs of this many val images ahead in one batch call "
                             "(1: file by file); the files, logs and scores are the same")
    parser.add_argument("--niqe", action="store_true",
                        help="also score the restored images with NIQE, the no-reference score of the reference's eval1.py")
    parser.add_argument("--niqe-params", type=str, default="./metric/niqe_pris_params.npz",
                        help="pristine-model statistics of NIQE (the reference's metric/niqe_pris_params.npz)")
    parser.add_argument("--lpips", action="store_true",
                        help="also score the restored images against HR with LPIPS (AlexNet variant), the perceptual score of the "
                             "reference's eval1.py")
    parser.add_argument("--lpips-weights", type=str, nargs="+", default=[], metavar="FILE",
                        help="LPIPS weights: torchvision's AlexNet state dict and the lpips package's alex.pth (.pth or .npz), merged")
    parser.add_argument("--val-loss", type=int, default=0, metavar="K",
                        help="also evaluate the denoising loss l_pix of every val image: K random (step, level) draws per image, seeded "
                             "per image index (0: off)")
    parser.add_argument("--val-loss-t", type=str, default=None, metavar="T1,T2,...",
                        help="with --val-loss: evaluate at these steps (K level draws each) instead of random ones, and print a per-step table")
    parser.add_argument("--val-loss-schedule", choices=["train", "val"], default="train",
                        help="beta schedule whose noise levels --val-loss draws from (default: train, the one the loss is defined on)")
    return parser


def main(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    if args.val_loss_t is not None and args.val_loss <= 0:
        parser.error("--val-loss-t needs --val-loss K (K >= 1 level draws per step)")
    if args.phase != "val":
        raise SystemExit("only -p val is implemented (sampling path); training is out of scope of this build")
    # a missing LPIPS weight file or tensor stops the run here, before a device is touched or the model is built
    lpips_weights = Metrics.load_lpips_weights(args.lpips_weights) if args.lpips else None

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", str(args.local_rank)))
    torch.cuda.set_device(local)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world)

    opt = Config.parse(args, world_size=world)
    opt["rank"], opt["world_size"] = rank, world
    apply_sampler_flags(opt, args)
    logging.basicConfig(level=logging.INFO if rank == 0 else logging.ERROR, format="%(asctime)s %(message)s")
    logger = logging.getLogger("base")
    fh = logging.FileHandler(os.path.join(opt["path"]["log"], "val.log"))
    logging.getLogger("val").addHandler(fh)

    niqe_params = Metrics.load_niqe_params(args.niqe_params) if args.niqe else None      # a missing file stops the run here
    val_set = make_val_dataset(opt["datasets"]["val"], args.decode_device)
    if args.synthetic_weights:
        opt["path"]["resume_state"] = None
    diffusion = Model.create_model(opt)
    diffusion.niqe_params = niqe_params
    diffusion.lpips_weights = lpips_weights
    if args.synthetic_weights:
        from ucdir_amd.weights import synth_state_dict
        sd = synth_state_dict(diffusion.netG.denoise_fn.cfg, 0)
        Model.load_checkpoint_state(diffusion.netG, {k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    diffusion.set_new_noise_schedule(opt["model"]["beta_schedule"]["val"], schedule_phase="val")

    logger.info("Begin Model Evaluation. len %d" % len(val_set))
    result_path = opt["path"]["results"]
    os.makedirs(result_path, exist_ok=True)
    tot_psnr = tot_ssim = tot_niqe = tot_lpips = tot_lpix = 0.0
    n = 0
    loss_table = loss_ts = None
    loss_steps = {}                                               # step -> [sum of l_pix, images] under --val-loss-t
    if args.val_loss > 0:
        loss_table = val_loss_table(opt, args.val_loss_schedule)
        loss_ts = parse_val_loss_steps(args.val_loss_t, len(loss_table) - 1)
    idxs = list(range(len(val_set)))
    if args.max_images > 0:
        idxs = idxs[:args.max_images * world]
    dn = diffusion.netG.denoise_fn
    thr = dn.patch_threshold
    # Per-image noise streams: image i draws Philox(seed_base + 1000003 i) with counters local to the image, whatever batch or rank it is
    # restored in.  --seed fixes the base; without it rank 0 draws it from torch's CPU generator and broadcasts it (the generator's
    # default seed is fixed, so runs get the same base unless torch.manual_seed or an earlier draw moves it).
    diffusion.image_seed_base = image_seed_base(args.seed)
    t_restore, n_restored = 0.0, 0
    group_times = []                                              # (images, seconds) of every DDPM.test call (the first one packs the weights)

    def restore(group):
        """One DDPM.test call for a group of images of identical (H, W): a batch is B independent restorations (model/diffusion.py:185-211
        is written for a batch; the reference's val loader feeds it batch_size 1, data/__init__.py:47)."""
        nonlocal tot_psnr, tot_ssim, tot_niqe, tot_lpips, tot_lpix, n, t_restore, n_restored
        items = [g[1] for g in group]
        data = {k: torch.stack([it[k] for it in items]) for k in ("HR", "SR", "LR", "gt", "lq") if k in items[0]}
        data["Index"] = [g[0] for g in group]                    # DDPM.test derives every image's noise stream from its index
        h, w = item_hw(items[0])
        small = (h + 128) * (w + 128) <= thr
        dn.set_graph(len(group) == 1 and small)                  # batch-1 remainders: HIP-graph replay of the forward (latency path)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            diffusion.feed_data(data)
            diffusion.test(continous=True)
        torch.cuda.synchronize()
        t_restore += time.perf_counter() - t0
        n_restored += len(group)
        group_times.append((len(group), time.perf_counter() - t0))
        l_pix = None
        if loss_table is not None:                                # outside the timed restoration; every rank of a sharded image takes part
            # the loss's forwards run on fresh tensors: without replay they leave no graphs behind.  Switching replay off drops the
            # restoration's graph, so under --val-loss a batch-1 restoration captures its forward again for every image.
            replay = dn.use_graph
            dn.set_graph(False)
            l_pix, per_step = diffusion.val_loss(args.val_loss, loss_ts, loss_table, seed=args.seed or 0)
            dn.set_graph(replay)
        if group[0][2] and rank != 0:
            return                                                # sharded image: every rank holds the same result; rank 0 reports it
        if l_pix is not None:                                     # counted once: by rank 0 for a sharded image, by its rank otherwise
            for t, vals in per_step.items():
                acc_t = loss_steps.setdefault(t, [0.0, 0])
                acc_t[0] += sum(vals)
                acc_t[1] += len(vals)
        name = opt["name"]
        dev_scores = diffusion.current_metrics() if args.metrics_device == "gpu" else None
        dev_niqe = diffusion.current_niqe() if args.niqe and args.metrics_device == "gpu" else None
        jpgs = diffusion.visuals_jpeg() if args.jpeg_device == "gpu" else None      # the four files of every image, as bytes
        dev_lpips = diffusion.current_lpips() if args.lpips and args.metrics_device == "gpu" else None
        need_u8 = jpgs is None or dev_scores is None or (args.niqe and dev_niqe is None) or (args.lpips and dev_lpips is None)
        for j, (i, _, _) in enumerate(group):
            fname = os.path.splitext(os.path.basename(val_set.sr_path[i]))[0]
            if need_u8:                                           # the uint8 images cross PCIe for Pillow or for host scoring only
                vis = diffusion.visuals_u8(j)
                hr_img, lr_img, fake_img, sr_img = vis["HR"], vis["LR"], vis["INF"], vis["SR"]
            if jpgs is not None:
                for key, tag in (("SR", "sr"), ("HR", "hr"), ("LR", "lr"), ("INF", "inf")):
                    with open("{}/{}_{}_{}.jpg".format(result_path, fname, name, tag), "wb") as f:
                        f.write(jpgs[j][key])
            else:
                Metrics.save_jpg(sr_img, "{}/{}_{}_sr.png".format(result_path, fname, name))
                Metrics.save_jpg(hr_img, "{}/{}_{}_hr.png".format(result_path, fname, name))
                Metrics.save_jpg(lr_img, "{}/{}_{}_lr.png".format(result_path, fname, name))
                Metrics.save_jpg(fake_img, "{}/{}_{}_inf.png".format(result_path, fname, name))
            if dev_scores is not None:
                tot_psnr += dev_scores[0][j]
                tot_ssim += dev_scores[1][j]
            else:
                tot_psnr += Metrics.calculate_psnr(sr_img, hr_img)
                tot_ssim += Metrics.calculate_ssim(sr_img, hr_img)
            if args.niqe:                                         # the uint8 SR image itself, not the JPEG read back
                tot_niqe += dev_niqe[j] if dev_niqe is not None else Metrics.calculate_niqe(sr_img, niqe_params)
            if args.lpips:
                tot_lpips += dev_lpips[j] if dev_lpips is not None else Metrics.calculate_lpips(sr_img, hr_img, lpips_weights)
            n += 1
            if l_pix is not None:
                tot_lpix += l_pix[j]
            logger.info(val_index_line(i, None if l_pix is None else l_pix[j]))

    pending = {}                                                  # (H, W) -> images of this rank waiting for a full batch (first-seen order)
    nsmall = 0
    ahead = args.decode_batch if args.decode_device == "gpu" and hasattr(val_set, "prefetch") else 1
    in_flight = ()                                                # the indices the last prefetch decoded
    for pos, i in enumerate(idxs):
        if ahead > 1 and i not in in_flight:
            in_flight = idxs[pos:pos + ahead]
            val_set.prefetch(in_flight)
        item = val_set[i]
        h, w = item_hw(item)
        shared = world > 1 and (h + 128) * (w + 128) > thr        # DDPM.test pads 64 per side: this image is patch-split
        if not shared:
            mine = (nsmall % world) == rank
            nsmall += 1
            if not mine:
                continue
        if shared or args.batch <= 1 or (h + 128) * (w + 128) > thr:
            restore([(i, item, shared)])                          # patch-split images (1024^2 windows as engine batches) go one at a time
            continue
        grp = pending.setdefault((h, w), [])
        grp.append((i, item, False))
        if len(grp) >= args.batch:
            restore(pending.pop((h, w)))
    for key in list(pending):
        restore(pending.pop(key))
    dn.set_graph(False)
    if n_restored:
        logger.info("restored %d images in %.2f s on this rank (%.2f img/s, batches of up to %d)" % (n_restored, t_restore, n_restored / t_restore, args.batch))
    main.last_throughput = (n_restored, t_restore)
    main.last_decode_fallbacks = list(getattr(val_set, "decode_fallbacks", []))
    if args.decode_device == "gpu":
        logger.info("decoded on the GPU; %d images fell back to Pillow%s" % (
            len(main.last_decode_fallbacks), "".join(" [%d: %s]" % f for f in main.last_decode_fallbacks[:8])))
    main.last_groups = group_times
    acc = torch.tensor([tot_psnr, tot_ssim, float(n), tot_niqe, tot_lpips, tot_lpix], dtype=torch.float64, device="cuda")
    if world > 1:
        dist.all_reduce(acc)
    avg_psnr, avg_ssim = (acc[0] / acc[2]).item(), (acc[1] / acc[2]).item()
    logger.info("# Validation # PSNR: {:.4e}".format(avg_psnr))
    logger.info("# Validation # SSIM: {:.4e}".format(avg_ssim))
    main.last_niqe = (acc[3] / acc[2]).item() if args.niqe else None
    main.last_lpips = (acc[4] / acc[2]).item() if args.lpips else None
    line = "psnr: {:.4e}, ssim: {:.4e}".format(avg_psnr, avg_ssim)
    if args.niqe:
        logger.info("# Validation # NIQE: {:.4e}".format(main.last_niqe))
        line += ", niqe: {:.4e}".format(main.last_niqe)
    if args.lpips:
        logger.info("# Validation # LPIPS: {:.4e}".format(main.last_lpips))
        line += ", lpips: {:.4e}".format(main.last_lpips)
    main.last_l_pix = (acc[5] / acc[2]).item() if loss_table is not None else None
    if loss_table is not None:
        logger.info("# Validation # l_pix: {:.4e}".format(main.last_l_pix))
        line += ", l_pix: {:.4e}".format(main.last_l_pix)
        steps = torch.tensor([loss_steps.get(t, [0.0, 0]) for t in (loss_ts or [])], dtype=torch.float64, device="cuda").reshape(-1, 2)
        if world > 1 and steps.numel():
            dist.all_reduce(steps)                                # every rank holds the same --val-loss-t: one row per step
        for t, (tot, cnt) in zip(loss_ts or [], steps.tolist()):
            if cnt:
                logger.info("# Validation # l_pix at step %d: %.4e (%d images)" % (t, tot / cnt, int(cnt)))
    logging.getLogger("val").info(line)
    if world > 1:
        dist.destroy_process_group()
    return avg_psnr, avg_ssim


if __name__ == "__main__":
    main()
