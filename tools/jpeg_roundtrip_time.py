"""Kernel time of the JPEG round trip of the JPEG-restoration val task (csrc/jpeg_roundtrip.hip.h): B = 16 at 512^2 and one
500 x 375-class image cropped to 496 x 368, `iters` calls each after a warm-up, timed with events; next to Pillow's
single-thread host round trip (libjpeg-turbo encode at the same quality + decode) of the same images.  Checks the bytes too.

    python tools/jpeg_roundtrip_time.py [iters] [quality]
"""
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ucdir_amd.metrics import jpeg_roundtrip_device  # noqa: E402


def images(B, H, W):
    """Tiles of the stored real image (tests/golden/sid_real_image.npz), shifted per image."""
    real = np.load(os.path.join(ROOT, "tests", "golden", "sid_real_image.npz"))["cond_u8"]
    big = np.tile(real, (-(-H // real.shape[0]) + 1, -(-W // real.shape[1]) + 1, 1))
    return np.stack([big[7 * b:7 * b + H, 11 * b:11 * b + W] for b in range(B)])


def pillow(img, q):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(buf, "JPEG", quality=q)
    buf.seek(0)
    return np.asarray(Image.open(buf).convert("RGB"))[..., ::-1]


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    q = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    res = {"quality": q, "iters": iters}
    for B, H, W in ((16, 512, 512), (1, 368, 496)):
        host = images(B, H, W)
        x = torch.from_numpy(host).cuda()
        for _ in range(5):
            y = jpeg_roundtrip_device(x, q)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            y = jpeg_roundtrip_device(x, q)
        e1.record()
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        t0 = time.perf_counter()
        ref = [pillow(host[b], q) for b in range(B)]
        t_host = time.perf_counter() - t0
        exact = all(np.array_equal(got[b], ref[b]) for b in range(B))
        res[f"B{B}_{H}x{W}"] = {"device_ms_per_call": e0.elapsed_time(e1) / iters, "pillow_ms_single_thread": 1e3 * t_host,
                                "bytes_equal_to_pillow": exact}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
