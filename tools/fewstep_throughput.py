"""Throughput of the few-step samplers against the 50-step ancestral sampler, on the flagship configuration of bench.py (full SID
UNet, synthetic weights, T = 50, linear_end 0.4):

    python tools/fewstep_throughput.py [--steps K] [--warmup W] [--configs ddim-5,dpm_solver++-20] [--no-patch] [--thresholding]

prints ONE JSON line: restored images/s at B = 16, 256^2 (the UNet computes at 288^2) for ddpm-50 (cross-check against bench.py),
ddim-5/10/25 and dpm_solver++-10/20, and seconds per image for the full-resolution 1424 x 2128 image through the inter-step patch
split (DDPM.test's reflect pad 64, one GPU) at ddpm-50 and dpm_solver++-20.  Times are wall-clock around whole restorations
(predictor + sampler) after a synchronize; each restoration draws its noise in-kernel.  With synthetic weights the restored images
mean nothing: this measures cost, not quality ("finite_fraction": the random network is no noise predictor, and DPM-Solver++'s
unclipped x0 = (x - sigma eps) / alpha can run away to inf on it - the work per call is the same).

``--thresholding`` adds, in the same run, dpm_solver++-20 with static and with dynamic x0 thresholding (tags
``dpm_solver++-20:static`` / ``:dynamic``) and a ``ms_per_call`` entry (restoration time / network calls) for them and the
unthresholded dpm_solver++-20 row they are read against."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ("ddpm-50", "ddim-5", "ddim-10", "ddim-25", "dpm_solver++-10", "dpm_solver++-20")
PATCH_CONFIGS = ("ddpm-50", "dpm_solver++-20")
THRESHOLD_BASE = "dpm_solver++-20"


def sampler_of(tag):
    tag, _, kind = tag.partition(":")
    name, steps = tag.rsplit("-", 1)
    if name == "ddpm":
        return None
    out = {"sampler": name, "steps": int(steps), "order": 2, "eta": 1.0, "time_input": "level"}
    if kind:
        out["thresholding"] = {"kind": kind, "max_val": 1.0, "ratio": 0.995}
    return out


def timed(net, x, tag, steps, warmup):
    net.sampler = sampler_of(tag)
    with torch.no_grad():
        for i in range(warmup + steps):
            if i == warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            torch.manual_seed(1 + i)
            out = net.super_resolution(x, False)
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    net.sampler = None
    return dt / steps, float(torch.isfinite(out).float().mean().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--no-patch", action="store_true", help="skip the full-resolution patch-split leg")
    ap.add_argument("--thresholding", action="store_true", help="add dpm_solver++-20 with static and dynamic x0 thresholding")
    args = ap.parse_args()
    import torch.nn.functional as F
    from bench import sid_opt
    from ucdir_amd import model as umodel
    from ucdir_amd import networks
    from ucdir_amd.weights import synth_inputs, synth_state_dict
    dev = torch.device("cuda", 0)
    net = networks.define_G(sid_opt())
    sd = synth_state_dict(net.denoise_fn.cfg, 0)
    umodel.load_checkpoint_state(net, {k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    net = net.to(dev).eval()
    net.set_new_noise_schedule(dict(schedule="linear", n_timestep=50, linear_start=1e-6, linear_end=0.4), dev)
    B, S = args.batch, args.size
    cond = torch.from_numpy(synth_inputs(B, S, S, seed=0)[0]).to(dev)
    rec = {"metric": "few-step samplers: restored images/s at B=%d, %dx%d SID; s/image full-resolution patch split" % (B, S, S),
           "batch": B, "size": S, "steps": args.steps, "warmup": args.warmup, "data": "synthetic weights (cost only, not quality)",
           "img_per_s": {}, "patch_s_per_image": {}, "finite_fraction": {}}
    tags = args.configs.split(",")
    if args.thresholding:
        tags = [t for t in tags if t != THRESHOLD_BASE] + [THRESHOLD_BASE, THRESHOLD_BASE + ":static", THRESHOLD_BASE + ":dynamic"]
        rec["ms_per_call"] = {}
    for tag in tags:
        dt, rec["finite_fraction"][tag] = timed(net, cond, tag, args.steps, args.warmup)
        rec["img_per_s"][tag] = B / dt
        if args.thresholding and tag.startswith(THRESHOLD_BASE):
            rec["ms_per_call"][tag] = 1e3 * dt / sampler_of(tag)["steps"]
    if not args.no_patch:
        H, W = 1424, 2128
        img = torch.from_numpy(synth_inputs(1, H, W, seed=0)[0]).to(dev)
        sr = F.pad(img, (64, 64, 64, 64), mode="reflect")
        rec["patch_size"] = [H, W]
        for tag in PATCH_CONFIGS:
            rec["patch_s_per_image"][tag] = timed(net, sr, tag, 1, 1)[0]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
