"""`sr.py -p val` loop throughput with the four JPEGs of every image written by Pillow on the host and by the HIP encoder
(--jpeg-device cpu | gpu), both with --metrics-device gpu, in one call:
    python tools/sr_val_jpeg_device_throughput.py [n_images] [size] > profiles/sr_val_jpeg_device.json
The two workloads of tools/sr_val_metrics_throughput.py through the full SID configuration (config/sid.yaml, synthetic weights,
--seed 1).  Each workload runs once unrecorded first (that sr.main call packs the weights and warms the allocator), then cpu,
then gpu.  Per run: loop_wall_s (the whole sr.main call: dataset loading, model set-up, restoration, scores, JPEG files),
loop_images_per_s, restore_s (DDPM.test calls only), after_restore_s (their difference) and whether the files of the two runs are
byte-identical."""
import importlib.util
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sr_val_metrics_throughput import write_pairs  # noqa: E402


def read_jpgs(wd):
    return {f: open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(os.path.join(wd, "experiments")) for f in fs
            if f.endswith(".jpg")}


def run_workload(sr, tag, n, h, w, batch):
    import yaml
    res = {"images": n, "height": h, "width": w, "batch": batch, "runs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        write_pairs(tmp, n, h, w)
        cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "sid.yaml")))
        cfg["datasets"]["val"]["data_args"]["dataroot"] = {"lq": os.path.join(tmp, "lq"), "gt": os.path.join(tmp, "gt")}
        yaml.safe_dump(cfg, open(os.path.join(tmp, "sid.yaml"), "w"))
        files = {}
        for run, dev in (("warmup", "cpu"), ("cpu", "cpu"), ("gpu", "gpu")):
            wd = os.path.join(tmp, f"{tag}_{run}")
            os.makedirs(wd)
            os.chdir(wd)
            t0 = time.perf_counter()
            psnr, ssim = sr.main(["-p", "val", "-c", os.path.join(tmp, "sid.yaml"), "--synthetic-weights", "--batch", str(batch),
                                  "--seed", "1", "--metrics-device", "gpu", "--jpeg-device", dev])
            wall = time.perf_counter() - t0
            if run == "warmup":
                continue
            nr, tr = sr.main.last_throughput
            files[run] = read_jpgs(wd)
            res["runs"][run] = {"jpeg_device": dev, "metrics_device": "gpu", "loop_wall_s": wall, "loop_images_per_s": n / wall,
                                "restore_s": tr, "restore_images_per_s": nr / tr, "after_restore_s": wall - tr,
                                "calls": len(sr.main.last_groups), "jpeg_files": len(files[run]),
                                "jpeg_bytes": sum(len(v) for v in files[run].values()), "psnr": psnr, "ssim": ssim}
            print(tag, run, json.dumps(res["runs"][run]), file=sys.stderr, flush=True)
        res["files_byte_identical"] = files["cpu"] == files["gpu"] and len(files["cpu"]) == 4 * n
        os.chdir(ROOT)
    return res


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 48
    size = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    spec = importlib.util.spec_from_file_location("sr_entry_jtp", os.path.join(ROOT, "sr.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    out = {"config": "config/sid.yaml (full SID UNet, T = 50), synthetic weights, --seed 1, --metrics-device gpu",
           "note": "each workload: one unrecorded run, then --jpeg-device cpu, then gpu, in one process",
           "workloads": {f"{n}x{size}sq_batch16": run_workload(sr, "small", n, size, size, 16),
                         "1x1424x2128_patch": run_workload(sr, "full", 1, 1424, 2128, 1)}}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
