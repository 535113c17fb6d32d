"""Time of the HIP baseline JPEG encoder of the val loop's files (csrc/jpeg_encode.hip.h) at quality 100, 4:4:4: B = 16 at 256^2 and
one 1424 x 2128 image, each with restored-image-like content (a smooth image plus small noise) and with uniform noise.  Per case,
each the mean over `iters` passes after a warm-up: the event-timed device work of one ucdir_jpeg_encode call (seven kernel
launches and one memset; buffers allocated once), the wall time of metrics.jpeg_encode_device (allocation, the wait for the
lengths, the packed copy of the used bytes), Pillow on one host thread on the same images (imported and run once before the
clock starts), and the bytes each way moves over PCIe.  Checks the bytes too.

    python tools/jpeg_encode_time.py [iters] > profiles/jpeg_encode_time.json
"""
import io
import json
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ucdir_amd import lib  # noqa: E402
from ucdir_amd.metrics import jpeg_encode_device  # noqa: E402
from ucdir_amd.ucdir import _ptr, _stream_ptr  # noqa: E402

QUALITY, SUBSAMPLING = 100, 0


def images(kind, B, H, W):
    rs = np.random.RandomState(B * 1000 + H)
    if kind == "noise":
        return rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for b in range(B):
        base = 128 + 90 * np.sin((x + 13 * b) / 37.0)[..., None] * np.cos((y + 7 * b) / 29.0)[..., None] * np.array([1.0, 0.8, 0.6])
        out.append(np.clip(base + rs.normal(0, 3, (H, W, 3)), 0, 255).astype(np.uint8))
    return np.stack(out)


def pillow(img):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=QUALITY, subsampling=SUBSAMPLING)
    return buf.getvalue()


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    L = lib.load()
    res = {"quality": QUALITY, "subsampling": "4:4:4", "iters": iters, "cases": {}}
    for B, H, W in ((16, 256, 256), (1, 1424, 2128)):
        for kind in ("smooth", "noise"):
            host = images(kind, B, H, W)
            x = torch.from_numpy(host).cuda()
            bound = L.ucdir_jpeg_encode_bound(H, W, SUBSAMPLING)
            ws = torch.empty(L.ucdir_jpeg_encode_workspace_bytes(B, H, W, SUBSAMPLING), dtype=torch.uint8, device="cuda")
            out = torch.empty((B, bound), dtype=torch.uint8, device="cuda")
            lengths = torch.empty(B, dtype=torch.int32, device="cuda")

            def call():
                lib.check(L.ucdir_jpeg_encode(_ptr(x), _ptr(out), _ptr(lengths), B, H, W, QUALITY, SUBSAMPLING, 0, _ptr(ws),
                                              _stream_ptr(x.device)))
            for _ in range(10):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                call()
            e1.record()
            torch.cuda.synchronize()
            for _ in range(5):
                files = jpeg_encode_device(x, QUALITY, SUBSAMPLING)
            t0 = time.perf_counter()
            for _ in range(iters):
                files = jpeg_encode_device(x, QUALITY, SUBSAMPLING)
            t_py = (time.perf_counter() - t0) / iters
            for _ in range(2):
                ref = [pillow(host[b]) for b in range(B)]
            t0 = time.perf_counter()
            for _ in range(iters):
                ref = [pillow(host[b]) for b in range(B)]
            t_host = (time.perf_counter() - t0) / iters
            for _ in range(5):
                x.cpu()
            t0 = time.perf_counter()
            for _ in range(iters):
                x.cpu()
            t_copy = (time.perf_counter() - t0) / iters
            res["cases"][f"B{B}_{H}x{W}_{kind}"] = {
                "device_ms_per_call": e0.elapsed_time(e1) / iters,
                "jpeg_encode_device_wall_ms_per_call": 1e3 * t_py,
                "pillow_ms_per_batch_single_thread": 1e3 * t_host,
                "uint8_fetch_ms_per_call": 1e3 * t_copy,
                "file_bytes_device_to_host": sum(len(f) for f in files),
                "uint8_bytes_device_to_host_for_pillow": int(host.nbytes),
                "workspace_bytes": int(ws.numel()), "output_slot_bytes": int(bound),
                "bytes_equal_to_pillow": files == ref}
            del ws, out
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
