#!/usr/bin/env python
"""NIQE of a directory of restored images: the NIQE part of the reference's eval1.py (eval1.py:209 scores every file whose name
contains "sr" with calculate_niqe(img, 0, 'HWC', 'y')).

    python tools/eval_niqe.py -s experiments/<run>/results [--device cpu|gpu] [--niqe-params metric/niqe_pris_params.npz]

The files are decoded with PIL.  --device gpu scores same-sized images in batches with the HIP kernels (metrics.niqe_device);
--device cpu uses metrics.calculate_niqe.  Prints one line per file and the mean.
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
    ap.add_argument("-s", "--source", required=True, help="directory with the restored images (files whose name contains 'sr')")
    ap.add_argument("--device", choices=["cpu", "gpu"], default="cpu")
    ap.add_argument("--niqe-params", default="./metric/niqe_pris_params.npz")
    ap.add_argument("--batch", type=int, default=16, help="images per device call (--device gpu)")
    args = ap.parse_args(argv)
    from PIL import Image
    params = M.load_niqe_params(args.niqe_params)
    files = sorted(f for f in os.listdir(args.source) if "sr" in f and f.lower().endswith(EXTS))
    if not files:
        raise SystemExit("no file with 'sr' in its name under %s" % args.source)
    imgs = {f: np.asarray(Image.open(os.path.join(args.source, f)).convert("RGB")) for f in files}
    scores = {}
    if args.device == "cpu":
        for f in files:
            scores[f] = M.calculate_niqe(imgs[f], params)
    else:
        import torch
        groups = {}
        for f in files:
            groups.setdefault(imgs[f].shape, []).append(f)
        for names in groups.values():
            for i in range(0, len(names), args.batch):
                part = names[i:i + args.batch]
                x = torch.from_numpy(np.stack([imgs[f] for f in part])).cuda().permute(0, 3, 1, 2).float() / 127.5 - 1
                for f, q in zip(part, M.niqe_device(x, params)):
                    scores[f] = q
    for f in files:
        print("%s NIQE %.12g" % (f, scores[f]))
    print("mean NIQE over %d images: %.12g" % (len(files), float(np.mean([scores[f] for f in files]))))
    return scores


if __name__ == "__main__":
    main()
