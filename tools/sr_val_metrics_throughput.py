"""`sr.py -p val` loop throughput with the val scores on the host and on the GPU (--metrics-device cpu | gpu), in one call:
    python tools/sr_val_metrics_throughput.py [n_images] [size] > profiles/sr_val_gpu_metrics.json
Two workloads through the full SID configuration (config/sid.yaml, synthetic weights, --seed 1), each run with both metric devices:
  * n same-sized pairs of size^2 (default 48 of 256^2) at --batch 16;
  * one 1424 x 2128 pair (the SID full size), restored on the inter-step patch path.
Per run: loop_wall_s (the whole sr.main call: restoration, JPEG writes, scores), loop_images_per_s, restore_s (DDPM.test calls only),
and the returned averages (PSNR equal and SSIM within 1e-9 between the two devices, tests/test_image_metrics_gpu.py)."""
import importlib.util
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_pairs(tmp, n, h, w):
    from PIL import Image
    rs = np.random.RandomState(0)
    for d in ("lq", "gt"):
        os.makedirs(os.path.join(tmp, d))
    for i in range(n):
        gt = (rs.rand(h // 8, w // 8, 3) * 255).astype(np.uint8).repeat(8, 0).repeat(8, 1)
        Image.fromarray(gt).save(os.path.join(tmp, "gt", f"{i:03d}.png"))
        Image.fromarray((gt * 0.25).astype(np.uint8)).save(os.path.join(tmp, "lq", f"{i:03d}.png"))


def run_workload(sr, tag, n, h, w, batch):
    import yaml
    res = {"images": n, "height": h, "width": w, "batch": batch, "runs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        write_pairs(tmp, n, h, w)
        cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "sid.yaml")))
        cfg["datasets"]["val"]["data_args"]["dataroot"] = {"lq": os.path.join(tmp, "lq"), "gt": os.path.join(tmp, "gt")}
        yaml.safe_dump(cfg, open(os.path.join(tmp, "sid.yaml"), "w"))
        for dev in ("cpu", "gpu"):
            wd = os.path.join(tmp, f"{tag}_{dev}")
            os.makedirs(wd)
            os.chdir(wd)
            t0 = time.perf_counter()
            psnr, ssim = sr.main(["-p", "val", "-c", os.path.join(tmp, "sid.yaml"), "--synthetic-weights", "--batch", str(batch),
                                  "--seed", "1", "--metrics-device", dev])
            wall = time.perf_counter() - t0
            nr, tr = sr.main.last_throughput
            res["runs"][dev] = {"metrics_device": dev, "loop_wall_s": wall, "loop_images_per_s": n / wall, "restore_s": tr,
                                "restore_images_per_s": nr / tr, "calls": len(sr.main.last_groups), "psnr": psnr, "ssim": ssim}
            print(tag, dev, json.dumps(res["runs"][dev]), file=sys.stderr, flush=True)
        os.chdir(ROOT)
    return res


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 48
    size = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    spec = importlib.util.spec_from_file_location("sr_entry_mtp", os.path.join(ROOT, "sr.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    out = {"config": "config/sid.yaml (full SID UNet, T = 50), synthetic weights, --seed 1",
           "note": "each workload runs cpu first, then gpu, in one process: the first sr.main call also packs the weights",
           "workloads": {f"{n}x{size}sq_batch16": run_workload(sr, "small", n, size, size, 16),
                         "1x1424x2128_patch": run_workload(sr, "full", 1, 1424, 2128, 1)}}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
