"""Kernel time of the device-side NIQE features (csrc/niqe.hip.h) at the two val shapes, and the host path on the same box:
B = 16 at 256^2 (the patch-val batch) and one 1424 x 2128 image (the full-size val set).

    python tools/niqe_time.py [--out profiles/niqe_time.json]

For per-kernel times run it under ``rocprofv3 --kernel-trace --stats -- python tools/niqe_time.py``."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ucdir_amd import lib, metrics as M  # noqa: E402
from ucdir_amd.ucdir import _ptr, _stream_ptr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def features_call(x, params):
    """The bare ucdir_niqe_features call on preallocated buffers (what the events time)."""
    L = lib.load()
    B, C, H, W = x.shape
    nblk = (H // 96) * (W // 96)
    ws = torch.empty(L.ucdir_niqe_workspace_bytes(B, C, H, W) // 8, dtype=torch.int64, device=x.device)
    feats = torch.empty((B, nblk, 36), dtype=torch.float64, device=x.device)
    tables = torch.from_numpy(M.niqe_tables()).to(x.device)
    window = np.ascontiguousarray(params["window"])

    def call():
        lib.check(L.ucdir_niqe_features(_ptr(x), x.stride(0), x.stride(1), x.stride(2), B, C, H, W, window.ctypes.data, _ptr(tables),
                                        _ptr(feats), None, _ptr(ws), _stream_ptr(x.device)))
    return call


def timed(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "niqe_time.json")
    params = M.load_niqe_params(os.path.join(ROOT, "tests", "golden", "niqe_pris_params.npz"))
    res = {"device": torch.cuda.get_device_name(0), "cases": []}
    for B, H, W in ((16, 256, 256), (1, 1424, 2128)):
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.rand(B, 3, H, W, device="cuda", generator=g) * 2 - 1
        dev_ms, dev_min = timed(features_call(x, params))
        t0 = time.perf_counter()
        scores = M.niqe_device(x, params)
        torch.cuda.synchronize()
        e2e_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        host = [M.calculate_niqe(M.tensor2img_u8_device(x[j]), params) for j in range(B)]
        host_ms = (time.perf_counter() - t0) * 1e3
        read = B * 3 * (H // 96 * 96) * (W // 96 * 96) * 4
        row = {"B": B, "H": H, "W": W, "features_kernels_ms_median": dev_ms, "features_kernels_ms_min": dev_min,
               "niqe_device_end_to_end_ms": e2e_ms, "host_calculate_niqe_ms": host_ms, "input_bytes_read": read,
               "input_read_GBps_at_median": read / dev_ms / 1e6,
               "max_rel_diff_device_vs_host": float(max(abs(a - b) / abs(b) for a, b in zip(scores, host)))}
        print(json.dumps(row))
        res["cases"].append(row)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
