"""Time of the Pillow-exact resampling of the 4x super-resolution val task (csrc/resample.hip.h): the loader's three-call chain
(crop -> 256^2 -> 64^2 -> 256^2, bicubic) for one 375^2 crop, and a batch of 16 at 256^2 -> 64^2 -> 256^2; `iters` chains each
after a warm-up, timed with events, the whole measurement run twice; next to Pillow's single-thread host chain on the same
images, and the bytes the kernels move against the HBM rate.  Checks the bytes against Pillow too.

    python tools/resample_time.py [iters] [out.json]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ucdir_amd.metrics import resample_device  # noqa: E402

HBM_BYTES_PER_S = 6.3e12                 # achievable HBM3E streaming rate of an MI355X (8.0e12 peak): a floor for the moved bytes


def images(B, H, W):
    """Tiles of the stored real image (tests/golden/sid_real_image.npz), shifted per image."""
    real = np.load(os.path.join(ROOT, "tests", "golden", "sid_real_image.npz"))["cond_u8"]
    big = np.tile(real, (-(-(H + 7 * B) // real.shape[0]) + 1, -(-(W + 11 * B) // real.shape[1]) + 1, 1))
    return np.ascontiguousarray(np.stack([big[7 * b:7 * b + H, 11 * b:11 * b + W] for b in range(B)]))


def chain_sizes(H):
    """(Hin, Hout) of each call of the chain from a square crop of side H; a 256^2 crop starts with Pillow's copy."""
    return ((H, 256), (256, 64), (64, 256))


def device_chain(x):
    hr = resample_device(x, (256, 256), "bicubic")
    lr = resample_device(hr, (64, 64), "bicubic")
    return hr, lr, resample_device(lr, (256, 256), "bicubic")


def pillow_chain(img):
    from PIL import Image
    hr = Image.fromarray(img).resize((256, 256), Image.BICUBIC)
    lr = hr.resize((64, 64), Image.BICUBIC)
    return np.asarray(hr), np.asarray(lr), np.asarray(lr.resize((256, 256), Image.BICUBIC))


def moved_bytes(B, H):
    """Image bytes the two passes of every call read and write once (tables left out): in + 2 x intermediate + out."""
    n = 0
    for a, b in chain_sizes(H):
        n += B * 3 * (2 * a * a if a == b else a * a + 2 * a * b + b * b)
    return n


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    res = {"iters": iters, "filter": "bicubic", "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S, "runs": []}
    for run in range(2):
        entry = {}
        for B, H in ((1, 375), (16, 256)):
            host = images(B, H, H)
            x = torch.from_numpy(host).cuda()
            for _ in range(10):
                got = device_chain(x)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                got = device_chain(x)
            e1.record()
            torch.cuda.synchronize()
            dev_ms = e0.elapsed_time(e1) / iters
            got = [g.cpu().numpy() for g in got]
            pillow_chain(host[0])
            t0 = time.perf_counter()
            ref = [pillow_chain(host[b]) for b in range(B)]
            host_ms = 1e3 * (time.perf_counter() - t0)
            exact = all(np.array_equal(got[k][b], ref[b][k]) for b in range(B) for k in range(3))
            nbytes = moved_bytes(B, H)
            entry[f"B{B}_{H}x{H}"] = {"device_ms_per_chain": dev_ms, "pillow_ms_single_thread": host_ms, "bytes_equal_to_pillow": exact,
                                      "moved_bytes": nbytes, "hbm_floor_us": 1e6 * nbytes / HBM_BYTES_PER_S,
                                      "device_not_slower_than_pillow": dev_ms <= host_ms}
        res["runs"].append(entry)
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
