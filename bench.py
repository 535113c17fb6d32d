#!/usr/bin/env python
"""Headline benchmark: restored 256x256 SID images/s at the 50-step ancestral sampler.

One "step" = one pass of the hot path over one batch: ``super_resolution`` of B=16 synthetic
256x256 crops = predictor + 50 x (DY3h forward on the HIP engine + fused sampler update), i.e.
BASELINE.json configs[1].  Inputs are resident in HBM before the timed region starts.

  python bench.py --gpus 1 --steps 3 --warmup 1
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W

N > 1: independent replicas (each rank restores its own batch; no data-path collective), weak
scaling; time = max over ranks between two barriers.  Rank 0 prints ONE JSON line.

``--mode patch`` times BASELINE.json configs[2] instead: one 1424x2128 image through ``DDPM.test`` (reflect-pad 64) ->
inter-step patch split, six 1024^2 windows per step sharded over the N ranks with one RCCL all-gather per step
(strong scaling: the image is fixed, N grows).  ``--latency`` adds B = 1 numbers (HIP-graph replay) at 256^2 and at the
``DDPM.test`` size (384^2 padded input, UNet at 416^2) to the JSON line under "latency".

``--dump-outputs DIR`` writes what the last timed step returned (the restored batch, or the restored padded image in patch
mode) as ``DIR/restored.npy`` in float32 after the timed region.  Every step restores the same inputs with the same noise, so
two builds run with the same arguments can be compared output for output, whatever --steps and --warmup are.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

MFMA_BF16_PEAK_TFLOPS = 2500.0   # dense bf16, /opt/skills/guides/MI355X_MICROARCH.md
KEY_NAMES = {0: "cgemm<64,std,s1>", 1: "cgemm<64,std,down>", 2: "cgemm<64,std,up>", 3: "cgemm<64,std,plain>",
             4: "cgemm<64,std,s1c>", 10: "cgemm<64,akgm>", 11: "akgm64_halo", 20: "conv3x3_halo<64>", 22: "conv3x3_halo<64>+res", 120: "conv3x3_halo<128>", 21: "upconv_halo<64>", 121: "upconv_halo<128>", 100: "cgemm<128,std,s1>", 101: "cgemm<128,std,down>",
             102: "cgemm<128,std,up>", 103: "cgemm<128,std,plain>", 104: "cgemm<128,std,s1c>", 110: "cgemm<128,akgm>", 111: "akgm_halo", 112: "akgm_pre",
             105: "qkv_ws", 113: "akgm_ws<8>", 114: "akgm_ws<16>", 115: "akgm_ws32", 116: "akgm_ws64", 23: "conv_ws<64>", 24: "conv_ws<128->64>+res",
             125: "conv_sk<8 waves>", 126: "upconv_sk<8 waves>", 127: "conv_sk<4 waves>+res", 128: "upconv_sk<4 waves>", 
             130: "flash_attn<bf16>", 131: "flash_attn<fp16>"}


def sid_opt():
    return {"model": {"which_model_G": "ucdir", "unet_name": "DY3h", "diffusion_name": "ResiGaussianGuideDY",
                      "unet": dict(in_channel=6, out_channel=3, inner_channel=64, channel_mults=[1, 2, 4, 8, 8],
                                   attn_res=[16], res_blocks=2, dropout=0.1, norm_groups=1),
                      "diffusion": dict(image_size=128, channels=3, conditional=True)}}


def host_cpu_info():
    """CPU model and core counts of the box the baseline ran on (`lscpu`): `cores` in the record is the thread
    count the oracle was given, these say what the host has."""
    info = {"cpu_model": None, "physical_cores": None, "logical_cpus": os.cpu_count(), "sockets": None}
    try:
        import subprocess
        txt = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        kv = {}
        for line in txt.splitlines():
            if ":" in line:
                k, v = line.split(":", 1)
                kv[k.strip()] = v.strip()
        info["cpu_model"] = kv.get("Model name")
        sockets = int(kv.get("Socket(s)", "0") or 0)
        cps = int(kv.get("Core(s) per socket", "0") or 0)
        info["sockets"] = sockets or None
        info["physical_cores"] = sockets * cps if sockets and cps else None
    except Exception:
        pass
    return info


def cpu_baseline(T, size):
    """CPU restatement (the oracle) on the host cores: bounded sample = predictor + 3 of the T forwards (min), B=1."""
    from oracle import ucdir_oracle as O
    from ucdir_amd.spec import UNetConfig
    from ucdir_amd.weights import synth_inputs, synth_state_dict
    # torch/oneDNN on this model stops scaling (and collapses when oversubscribed) well below the
    # host's 256 hardware threads; 32 threads is the fastest setting measured on the GPU box
    cores = min(os.cpu_count() or 1, int(os.environ.get("UCDIR_CPU_THREADS", "32")))
    torch.set_num_threads(cores)
    cfg = UNetConfig(inner_channel=64, channel_mults=(1, 2, 4, 8, 8), res_blocks=2, attn_res=(16,), image_size=128)
    sd = O.to_torch_sd(synth_state_dict(cfg, 0))
    cond, guide, x_t = map(torch.from_numpy, synth_inputs(1, size, size, seed=0))
    with torch.no_grad():
        t0 = time.time(); g = O.predictor_forward(sd, cond); tp = time.time() - t0
        x6 = torch.cat([cond, x_t], 1)
        lvl = torch.tensor([[0.5]])
        O.dy3h_forward(sd, x6, lvl, g)                 # warm-up (thread pools, mkldnn primitives)
        n, times = 3, []
        for _ in range(n):
            t0 = time.time()
            O.dy3h_forward(sd, x6, lvl, g)
            times.append(time.time() - t0)
        tf = min(times)
    return {"value": 1.0 / (T * tf + tp), "unit": "images/s", "cores": cores, "kind": "port", **host_cpu_info(),
            "sample": f"B=1 {size}x{size}: predictor + {n} of {T} UNet forwards timed, fastest {tf:.3f} s/forward "
                      f"(all: {', '.join('%.3f' % t for t in times)}), extrapolated to {T} steps; fp32 torch CPU "
                      f"restatement (oracle/)"}


class LaunchProfile:
    """HIP-event brackets around the GEMM-core launches of selected forwards (library hooks ucdir_profile_*), read back as
    per-kernel-instantiation totals: the roofline leg, measured inside the timed region."""
    CAP = 32

    def __init__(self, L, ulib):
        self.L, self.ulib = L, ulib
        c = self.CAP
        self.keys = (ctypes.c_int32 * c)(); self.ln = (ctypes.c_int32 * c)(); self.ms = (ctypes.c_double * c)()
        self.fl = (ctypes.c_double * c)(); self.by = (ctypes.c_double * c)(); self.nr = ctypes.c_int32(0)

    def read(self):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.ulib.check(self.L.ucdir_profile_read(self.CAP, self.keys, self.ln, self.ms, self.fl, self.by,
                                                  ctypes.byref(self.nr), st))
        rows = [dict(key=int(self.keys[i]), kernel=KEY_NAMES.get(int(self.keys[i]), str(self.keys[i])),
                     launches=int(self.ln[i]), ms=float(self.ms[i]), flops=float(self.fl[i]), bytes=float(self.by[i]))
                for i in range(self.nr.value)]
        # key 129 = launches of conv_sk_kernel<1, 4, 9> that carry wide + short units (the 36^2 level): the same kernel symbol as key 127 (the
        # library keeps the key apart so that tests can assert the mixed schedule engaged) - one row, as in rocprofv3's statistics
        mixed = [r for r in rows if r["key"] == 129]
        base = [r for r in rows if r["key"] == 127]
        if mixed and base:
            for f in ("launches", "ms", "flops", "bytes"):
                base[0][f] += mixed[0][f]
            rows = [r for r in rows if r["key"] != 129]
        elif mixed:
            mixed[0]["key"], mixed[0]["kernel"] = 127, KEY_NAMES[127]
        rows.sort(key=lambda r: -r["ms"])
        return rows


def sustained_matrix_rate(L, ulib):
    """Matrix-core rate this box sustains on operands like the conv kernels' (ucdir_matrix_rate: MFMAs only, ~4 ms bursts, after the
    timed region): the clock the chip holds under matrix load depends on the operand bits, so the practical roof sits below `peak`."""
    import ctypes
    import torch
    out = {}
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, rnd in (("random_operands", 1), ("small_integer_operands", 0)):
        v = ctypes.c_double(0.0)
        ulib.check(L.ucdir_matrix_rate(15000, rnd, ctypes.byref(v), st))
        out[name] = v.value
    return out


def roofline_record(rows, whole_tflops=None, sustained=None):
    """`roofline` object of the JSON line for the instantiation with the largest total time."""
    if not rows:
        return None
    d = rows[0]
    ach = d["flops"] / (d["ms"] * 1e-3) / 1e12
    traffic = None
    tf = os.path.join(ROOT, "profiles", "traffic.json")   # PMC-derived HBM bytes / launch
    if os.path.exists(tf):
        try:
            traffic = json.load(open(tf)).get(d["kernel"])
        except Exception:
            traffic = None
    roof = {"bound": "mfma", "kernel": d["kernel"], "achieved": ach, "peak": MFMA_BF16_PEAK_TFLOPS,
            "unit": "TFLOP/s", "frac": ach / MFMA_BF16_PEAK_TFLOPS, "traffic": traffic,
            "traffic_source": "stored: PMC FETCH_SIZE / WRITE_SIZE per launch of the profiled build (profiles/traffic.json), not measured in this run",
            "launches": d["launches"], "avg_launch_us": d["ms"] * 1e3 / d["launches"],
            "flops_per_launch": d["flops"] / d["launches"], "bytes_per_launch": d["bytes"] / d["launches"],
            "all_kernels": [{"kernel": r["kernel"], "launches": r["launches"], "ms": round(r["ms"], 3),
                             "tflops": round(r["flops"] / (r["ms"] * 1e-3) / 1e12, 1)} for r in rows]}
    if whole_tflops is not None:
        roof["forward_tflops_whole"] = whole_tflops
        roof["forward_frac_whole"] = whole_tflops / MFMA_BF16_PEAK_TFLOPS      # all launches of a forward against the dense bf16 peak
    if sustained:
        # measured in this run, NOT the `peak` that `frac` is priced against: what v_mfma_f32_32x32x16_bf16 alone reaches on this box
        roof["sustained_peak"] = {"unit": "TFLOP/s", **{k: round(v, 1) for k, v in sustained.items()},
                                  "frac_of_random_operand_rate": ach / sustained["random_operands"],
                                  "source": "ucdir_matrix_rate (MFMA-only kernel, two waves per SIMD, no memory traffic), after the timed region"}
    return roof


DUMP_BYTES = 60 << 20          # with the .npy header still under 64 MB (10^6 or 2^20 bytes)


def dump_output(out_dir, name, t):
    """``out_dir/<name>.npy`` in float32; above DUMP_BYTES a fixed seeded sample of the flattened elements (sorted indices),
    the same for every run of the same shape."""
    a = t.detach().float().cpu().numpy()
    if a.nbytes > DUMP_BYTES:
        a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, DUMP_BYTES // 4, replace=False))]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, name + ".npy"), a)


def latency_leg(net, dev, T):
    """B = 1 restorations with the forward replayed from a HIP graph: 256^2 (UNet at 288^2) and the DDPM.test size
    (256^2 crop reflect-padded by 64 -> 384^2 input, UNet at 416^2; the reference's val loader is batch_size = 1)."""
    import torch.nn.functional as F
    from ucdir_amd.weights import synth_inputs
    out = {}
    net.denoise_fn.set_graph(True)
    try:
        for tag, pad in (("256", 0), ("ddpm_test_384", 64)):
            cond = torch.from_numpy(synth_inputs(1, 256, 256, seed=7)[0]).to(dev)
            if pad:
                cond = F.pad(cond, (pad, pad, pad, pad), mode="reflect")
            with torch.no_grad():
                net.super_resolution(cond, False)                     # plan + capture
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = 3
                for _ in range(n):
                    net.super_resolution(cond, False)
                torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / n
            out[tag] = {"images_per_s": 1.0 / dt, "ms_per_image": dt * 1e3, "ms_per_step": dt * 1e3 / T}
    finally:
        net.denoise_fn.set_graph(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--timesteps", type=int, default=50)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--mode", choices=["replicas", "patch"], default="replicas")
    ap.add_argument("--latency", action="store_true", help="add B = 1 HIP-graph latency numbers to the JSON line")
    ap.add_argument("--patch-batch", type=int, default=0, help="patch mode: windows per engine call (0 = the module's default)")
    ap.add_argument("--height", type=int, default=1424)
    ap.add_argument("--width", type=int, default=2128)
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's output to DIR/restored.npy (float32)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the denoiser has no CPU path")
    torch.cuda.set_device(local)
    dist = None
    # under a torch.distributed launcher (the driver's `python -m torch.distributed.run ... bench.py`) RCCL is initialised even for one
    # rank: the launch line of a scaling run is then exercised end to end on a one-GPU box (barriers, the max over ranks, and in
    # patch mode the per-step all-gather branch)
    launched = "RANK" in os.environ and "MASTER_PORT" in os.environ
    if world > 1 or launched:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world)
    dev = torch.device("cuda", local)

    from ucdir_amd import lib as ulib
    from ucdir_amd import networks
    from ucdir_amd.spec import UNetConfig
    from ucdir_amd.weights import synth_inputs, synth_state_dict

    from ucdir_amd import model as umodel
    net = networks.define_G(sid_opt())
    sd = synth_state_dict(net.denoise_fn.cfg, 0)
    umodel.load_checkpoint_state(net, {k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    net = net.to(dev).eval()
    T = args.timesteps
    net.set_new_noise_schedule(dict(schedule="linear", n_timestep=T, linear_start=1e-6, linear_end=0.4), dev)
    if args.mode == "patch":
        return patch_mode(args, net, dev, dist, rank, world, T)
    B, S = args.batch, args.size
    cond = torch.from_numpy(synth_inputs(B, S, S, seed=rank)[0]).to(dev)

    def restore():
        # each restoration takes its noise seed from torch's CPU generator: reseeded, every step draws the same noise
        torch.manual_seed(1 + rank)
        return net.super_resolution(cond, False)

    # bracket the GEMM-core launches of ONE forward per restoration with HIP events (roofline leg)
    L = ulib.load()
    calls = {"n": 0}
    inner = net.denoise_fn.forward_split

    def wrapped(*a, **k):
        prof = (calls["n"] % T) == T // 2
        calls["n"] += 1
        if prof:
            L.ucdir_profile_enable(1)
        try:
            return inner(*a, **k)
        finally:
            if prof:
                L.ucdir_profile_enable(0)
    net.denoise_fn.forward_split = wrapped

    def sync():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    with torch.no_grad():
        for _ in range(args.warmup):
            restore()
        prof = LaunchProfile(L, ulib)
        prof.read()                                            # drop warm-up profile rows
        sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = restore()
        sync()
        t1 = time.perf_counter()
    elapsed = torch.tensor([t1 - t0], dtype=torch.float64, device=dev)
    if dist is not None:
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    elapsed = float(elapsed.item())
    assert torch.isfinite(out).all()
    if args.dump_outputs and rank == 0:
        dump_output(args.dump_outputs, "restored", out)

    rows = prof.read()

    if rank == 0:
        fwd_flops = net.denoise_fn.forward_flops()          # algorithmic FLOPs of one B-sample forward
        value = world * B * args.steps / elapsed
        roof = roofline_record(rows, fwd_flops * T * args.steps / elapsed / 1e12, sustained_matrix_rate(L, ulib))
        rec = {"metric": "restored images/sec at 50-step p_sample_loop, 256x256 SID", "value": value,
               "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
               "config": {"workload": f"SID denoising {S}x{S} batch={B}, {T}-step sampler (BASELINE.json configs[1]); "
                                      f"UNet computes at {(S // 32 + 1) * 32}^2; random-init DY3h 97.35M + predictor",
                          "global_batch": world * B, "timesteps": T, "parallelism": f"replicas x{world}",
                          "gflop_per_forward_per_image": fwd_flops / B / 1e9},
               "roofline": roof}
        if args.latency:
            net.denoise_fn.forward_split = inner
            rec["latency"] = latency_leg(net, dev, T)
        if world == 1 and not args.no_cpu_baseline:
            rec["cpu_baseline"] = cpu_baseline(T, S)
        print(json.dumps(rec))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def patch_mode(args, net, dev, dist, rank, world, T):
    """BASELINE configs[2]: one full-resolution image, windows of every step sharded over the ranks (utils/util.py:108-146)."""
    import torch.nn.functional as F
    from ucdir_amd import patch
    from ucdir_amd.weights import synth_inputs
    H, W = args.height, args.width
    if dist is not None:
        net.denoise_fn.patch_group = dist.group.WORLD
        net.denoise_fn.patch_force_gather = True              # (a one-rank group under the launcher still runs the collective)
    net.noise_seed = 1234                                     # every rank applies the identical sampler update
    net.denoise_fn.patch_timers = [] if dist is not None else None    # (start, end) events of every all-gather
    if args.patch_batch:
        net.denoise_fn.patch_max_batch = args.patch_batch
    cond = torch.from_numpy(synth_inputs(1, H, W, seed=0)[0]).to(dev)
    sr = F.pad(cond, (64, 64, 64, 64), mode="reflect")         # DDPM.test (model/model.py:127-128)
    pd = patch.patch_pad(sr.shape[-2], sr.shape[-1], net.denoise_fn.patch_skip, net.denoise_fn.patch_padding)
    nwin = len(patch.patch_windows(sr.shape[-2] + 2 * pd, sr.shape[-1] + 2 * pd, net.denoise_fn.patch_skip,
                                   net.denoise_fn.patch_padding))

    from ucdir_amd import lib as ulib
    L = ulib.load()
    calls = {"n": 0}
    inner = net.denoise_fn.forward                             # one call per sampler step: all of this rank's windows

    def wrapped(*a, **k):                                      # HIP-event brackets around the launches of ONE step per image
        on = (calls["n"] % T) == T // 2
        calls["n"] += 1
        if on:
            L.ucdir_profile_enable(1)
        try:
            return inner(*a, **k)
        finally:
            if on:
                L.ucdir_profile_enable(0)
    net.denoise_fn.forward = wrapped

    def sync():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
    with torch.no_grad():
        for _ in range(args.warmup):
            net.super_resolution(sr, False)
        prof = LaunchProfile(L, ulib)
        prof.read()
        sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = net.super_resolution(sr, False)
        sync()
        t1 = time.perf_counter()
    rows = prof.read()
    elapsed = torch.tensor([t1 - t0], dtype=torch.float64, device=dev)
    if dist is not None:
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    elapsed = float(elapsed.item())
    assert torch.isfinite(out).all()
    if args.dump_outputs and rank == 0:
        dump_output(args.dump_outputs, "restored", out)
    # self-explaining scaling line: windows this rank evaluates per step and what the collective costs per step
    per = (nwin + world - 1) // world
    mine = max(0, min(per, nwin - rank * per))
    tm = net.denoise_fn.patch_timers or []
    gather_ms = (sum(a.elapsed_time(b) for a, b in tm[-T * args.steps:]) / max(1, min(len(tm), T * args.steps))) if tm else 0.0
    info = torch.tensor([float(mine), gather_ms], dtype=torch.float64, device=dev)
    infos = [info.clone() for _ in range(world)]
    if dist is not None:
        dist.all_gather(infos, info)
    if rank == 0:
        ws = L.ucdir_workspace_bytes(net.denoise_fn._handle())
        rec = {"metric": f"restored full-resolution images/sec at {T}-step p_sample_loop, inter-step patch split",
               "value": args.steps / elapsed, "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
               "dtype": "bf16", "data": "synthetic",
               "config": {"workload": f"SID full-res {H}x{W} (BASELINE.json configs[2]): DDPM.test pad 64 -> {nwin} windows of "
                                      f"1024^2 per step (skip 1024, padding 64), {T}-step sampler; windows sharded over "
                                      f"{world} rank(s), one all-gather per step",
                          "global_batch": 1, "timesteps": T, "parallelism": f"patch-shard x{world}",
                          "windows_per_step": nwin, "windows_per_engine_batch": int(net.denoise_fn.patch_max_batch),
                          "windows_per_rank": [int(v[0].item()) for v in infos],
                          "all_gather_ms_per_step_per_rank": [round(float(v[1].item()), 4) for v in infos],
                          "workspace_bytes_rank0": int(ws)},
               "roofline": roofline_record(rows, sustained=sustained_matrix_rate(L, ulib))}
        print(json.dumps(rec))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
