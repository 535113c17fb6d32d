#!/usr/bin/env python
"""LPIPS (AlexNet variant) of a directory of restored images: the LPIPS column of the reference's eval1.py (eval1.py:194-196 sorts the
files whose name contains "hr" and the files whose name contains "sr" and pairs them in that order).

    python tools/eval_lpips.py -s experiments/<run>/results --weights alexnet.pth alex.pth [--device cpu|gpu] [--decode-device cpu|gpu]

The files are decoded with PIL, or with --decode-device gpu by the HIP baseline decoder (the same pixels; a file it does not take
falls back to PIL).  --device gpu scores same-sized pairs in batches with the HIP kernels (metrics.lpips_u8_device);
--device cpu uses metrics.calculate_lpips.  Prints one line per pair and the mean.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ucdir_amd import metrics as M  # noqa: E402

EXTS = (".png", ".jpg", ".jpeg", ".bmp")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-s", "--source", required=True, help="directory with the *hr* and *sr* images")
    ap.add_argument("--weights", nargs="+", required=True, metavar="FILE",
                    help="torchvision's AlexNet state dict and the lpips package's alex.pth (.pth or .npz)")
    ap.add_argument("--device", choices=["cpu", "gpu"], default="cpu")
    ap.add_argument("--decode-device", choices=["cpu", "gpu"], default="cpu", help="where the files are decoded")
    ap.add_argument("--batch", type=int, default=16, help="pairs per device call (--device gpu)")
    args = ap.parse_args(argv)
    weights = M.load_lpips_weights(args.weights)
    names = [f for f in os.listdir(args.source) if f.lower().endswith(EXTS)]
    hr, sr = sorted(f for f in names if "hr" in f), sorted(f for f in names if "sr" in f)
    if not sr or len(hr) != len(sr):
        raise SystemExit("need as many files with 'hr' as with 'sr' in their name under %s, got %d and %d" % (args.source, len(hr), len(sr)))
    fallbacks = []
    on_gpu = args.decode_device == "gpu"                  # then the images are CUDA tensors
    load = lambda f: M.load_rgb_u8(os.path.join(args.source, f), args.decode_device, fallbacks)
    pairs = [(s, load(s), load(h)) for h, s in zip(hr, sr)]
    scores = {}
    if args.device == "cpu":
        for s, a, b in pairs:
            scores[s] = M.calculate_lpips(a.cpu().numpy(), b.cpu().numpy(), weights) if on_gpu else M.calculate_lpips(a, b, weights)
    else:
        import torch
        groups = {}
        for p in pairs:
            groups.setdefault((tuple(p[1].shape), tuple(p[2].shape)), []).append(p)
        for grp in groups.values():
            for i in range(0, len(grp), args.batch):
                part = grp[i:i + args.batch]
                stack = lambda k: torch.stack([p[k] for p in part]) if on_gpu else torch.from_numpy(np.stack([p[k] for p in part])).cuda()
                a, b = stack(1), stack(2)
                for p, q in zip(part, M.lpips_u8_device(a, b, weights)):
                    scores[p[0]] = q
    for s in sr:
        print("%s LPIPS %.12g" % (s, scores[s]))
    if on_gpu:
        print("decoded on the GPU; %d files fell back to PIL" % len(fallbacks))
    print("mean LPIPS over %d pairs: %.12g" % (len(sr), float(np.mean([scores[s] for s in sr]))))
    return scores


if __name__ == "__main__":
    main()
