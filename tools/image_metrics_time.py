"""Kernel-time driver of the device-side val scores (csrc/image_metrics.hip.h): B = 16 at 256^2 and one 1424 x 2128 image,
`iters` calls each after a warm-up (`python tools/image_metrics_time.py [iters] [small|full|both]`).  Run it under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/image_metrics_time.py 20 small` (and `full`) for the kernel times; it prints the work each call implies (bytes read, fp64 operations) and an event-timed mean per call."""
import json
import sys
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ucdir_amd.ucdir import image_metrics_  # noqa: E402


def work(B, C, H, W):
    """Bytes the kernels must read and the fp64 operations of the separable filter + SSIM formula (2 per multiply-add)."""
    ho, wo = max(H - 10, 0), max(W - 10, 0)
    h_pass = 5 * 11 * 2 * H * wo + 3 * 11 * H * wo     # 5 planes x 11 taps (FMA), + the 3 products a^2, b^2, ab per tap
    v_pass = 5 * 11 * 2 * ho * wo + 20 * ho * wo        # 5 planes x 11 taps, + the SSIM formula
    return {"bytes_read": 2 * 4 * B * C * H * W, "fp64_ops": B * C * (h_pass + v_pass)}


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    which = sys.argv[2] if len(sys.argv) > 2 else "both"          # small | full | both: one shape per profiler run
    shapes = {"small": [(16, 256, 256)], "full": [(1, 1424, 2128)]}.get(which, [(16, 256, 256), (1, 1424, 2128)])
    res = {}
    for B, H, W in shapes:
        g = torch.Generator(device="cuda").manual_seed(0)
        a = torch.rand(B, 3, H, W, device="cuda", generator=g) * 2 - 1
        b = torch.rand(B, 3, H, W, device="cuda", generator=g) * 2 - 1
        for _ in range(3):
            image_metrics_(a, b)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            image_metrics_(a, b)
        e1.record()
        torch.cuda.synchronize()
        res[f"B{B}_{H}x{W}"] = dict(work(B, 3, H, W), call_ms_event_mean=e0.elapsed_time(e1) / iters, iters=iters)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
