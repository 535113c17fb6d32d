"""Time of LPIPS (AlexNet variant) at the two val shapes, three ways in one process, alternating: the HIP path (csrc/lpips.hip.h,
the bare ucdir_lpips_forward on a preallocated workspace), the same network composed from torch ops on the device (fp32 conv2d /
max_pool2d on whatever library torch dispatches to), and the host path (metrics.calculate_lpips, float32): B = 16 pairs at 256^2
(the patch-val batch) and one 1424 x 2128 pair (the full-size val set).  Synthetic weights (weights.synth_lpips_weights).

    python tools/lpips_time.py [--out profiles/lpips_time.json]

The achieved fraction is the conv FLOPs of the 2B images (2 * MAC of the un-padded problem) over the median time of the whole
forward, against the nominal 157 TFLOP/s of the f32-input MFMA."""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ucdir_amd import lib, metrics as M  # noqa: E402
from ucdir_amd.ucdir import _ptr, _stream_ptr  # noqa: E402
from ucdir_amd.weights import synth_lpips_weights  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_TFLOPS = 157.0


def conv_flops(H, W):
    """2 * MAC of the five convs for ONE image."""
    total, h, w = 0, H, W
    for _, cin, cout, k, stride, pad, pool in M.LPIPS_LAYERS:
        if pool:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        h, w = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        total += 2 * h * w * cout * cin * k * k
    return total


def hip_call(a, b, weights):
    L = lib.load()
    obj = M.lpips_handle(weights, a.device)
    B, H, W, _ = a.shape
    ws = torch.empty(L.ucdir_lpips_workspace_bytes(B, H, W), dtype=torch.uint8, device=a.device)
    out = torch.empty(6 * B, dtype=torch.float64, device=a.device)

    def call():
        lib.check(L.ucdir_lpips_forward(obj._h, _ptr(a), _ptr(b), B, H, W, _ptr(out), _ptr(out[B:]), _ptr(ws), _stream_ptr(a.device)))
    return call, out


def torch_call(a, b, weights):
    dev = a.device
    w = {k: torch.from_numpy(v).to(dev) for k, v in weights.items()}
    shift = torch.tensor(M.LPIPS_SHIFT, device=dev).view(1, 3, 1, 1)
    scale = torch.tensor(M.LPIPS_SCALE, device=dev).view(1, 3, 1, 1)
    B = a.shape[0]
    res = {}

    def call():
        x = torch.cat([a, b]).permute(0, 3, 1, 2).float() / 127.5 - 1
        x = (x - shift) / scale
        total = 0
        for l, (key, _, _, _, stride, pad, pool) in enumerate(M.LPIPS_LAYERS):
            if pool:
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, w[key + ".weight"], w[key + ".bias"], stride=stride, padding=pad))
            n = x / (torch.sqrt(torch.sum(x * x, dim=1, keepdim=True)) + 1e-10)
            d = (n[:B] - n[B:]) ** 2 * w[f"lin{l}.model.1.weight"].view(1, -1, 1, 1)
            total = total + d.sum(dim=1).mean(dim=(1, 2))
        res["scores"] = total
    return call, res


def timed_alternating(fns, iters=20, warm=3):
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))
    return [(float(np.median(t)), float(np.min(t))) for t in ts]


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "lpips_time.json")
    weights = synth_lpips_weights(0)
    res = {"device": torch.cuda.get_device_name(0), "weights": "synth_lpips_weights(0)", "peak_tflops_nominal_f32_mfma": PEAK_TFLOPS,
           "cases": []}
    for B, H, W in ((16, 256, 256), (1, 1424, 2128)):
        g = torch.Generator(device="cuda").manual_seed(1)
        a = torch.randint(0, 256, (B, H, W, 3), device="cuda", generator=g, dtype=torch.uint8)
        b = (a.int() + torch.randint(-20, 21, a.shape, device="cuda", generator=g)).clamp(0, 255).to(torch.uint8)
        hip, hip_out = hip_call(a, b, weights)
        tch, tch_out = torch_call(a, b, weights)
        (hip_ms, hip_min), (tch_ms, tch_min) = timed_alternating([hip, tch])
        an, bn = a.cpu().numpy(), b.cpu().numpy()
        t0 = time.perf_counter()
        host = [M.calculate_lpips(an[j], bn[j], weights) for j in range(B)]
        host_ms = (time.perf_counter() - t0) * 1e3
        flops = 2 * B * conv_flops(H, W)
        dev = hip_out[:B].cpu().tolist()
        row = {"B": B, "H": H, "W": W, "conv_gflop_per_image": conv_flops(H, W) / 1e9, "conv_gflop_total": flops / 1e9,
               "hip_forward_ms_median": hip_ms, "hip_forward_ms_min": hip_min,
               "torch_ops_on_device_ms_median": tch_ms, "torch_ops_on_device_ms_min": tch_min,
               "host_calculate_lpips_float32_ms": host_ms,
               "hip_tflops_at_median": flops / hip_ms / 1e9, "hip_fraction_of_157_tflops": flops / hip_ms / 1e9 / PEAK_TFLOPS,
               "torch_ops_tflops_at_median": flops / tch_ms / 1e9,
               "max_rel_diff_hip_vs_host_float32": float(max(abs(x - y) / abs(y) for x, y in zip(dev, host))),
               "max_rel_diff_torch_ops_vs_host_float32": float(max(abs(x - y) / abs(y) for x, y in zip(tch_out["scores"].cpu().tolist(), host)))}
        print(json.dumps(row))
        res["cases"].append(row)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
