#!/usr/bin/env python
"""NIQE of a directory of restored images: the NIQE part of the reference's eval1.py (eval1.py:209 scores every file whose name
contains "sr" with calculate_niqe(img, 0, 'HWC', 'y')).

    python tools/eval_niqe.py -s experiments/<run>/results [--device cpu|gpu] [--decode-device cpu|gpu]
                               [--niqe-params metric/niqe_pris_params.npz]

The files are decoded with PIL, or with --decode-device gpu by the HIP baseline decoder (the same pixels; a file it does not take
falls back to PIL).  --device gpu scores same-sized images in batches with the HIP kernels (metrics.niqe_device);
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
    ap.add_argument("--decode-device", choices=["cpu", "gpu"], default="cpu", help="where the files are decoded")
    ap.add_argument("--niqe-params", default="./metric/niqe_pris_params.npz")
    ap.add_argument("--batch", type=int, default=16, help="images per device call (--device gpu)")
    args = ap.parse_args(argv)
    params = M.load_niqe_params(args.niqe_params)
    files = sorted(f for f in os.listdir(args.source) if "sr" in f and f.lower().endswith(EXTS))
    if not files:
        raise SystemExit("no file with 'sr' in its name under %s" % args.source)
    fallbacks = []
    imgs = {f: M.load_rgb_u8(os.path.join(args.source, f), args.decode_device, fallbacks) for f in files}
    on_gpu = args.decode_device == "gpu"                  # then the images are CUDA tensors
    scores = {}
    if args.device == "cpu":
        for f in files:
            scores[f] = M.calculate_niqe(imgs[f].cpu().numpy() if on_gpu else imgs[f], params)
    else:
        import torch
        groups = {}
        for f in files:
            groups.setdefault(tuple(imgs[f].shape), []).append(f)
        for names in groups.values():
            for i in range(0, len(names), args.batch):
                part = names[i:i + args.batch]
                x = torch.stack([imgs[f] for f in part]) if on_gpu else torch.from_numpy(np.stack([imgs[f] for f in part])).cuda()
                x = x.permute(0, 3, 1, 2).contiguous().float() / 127.5 - 1
                for f, q in zip(part, M.niqe_device(x, params)):
                    scores[f] = q
    for f in files:
        print("%s NIQE %.12g" % (f, scores[f]))
    if on_gpu:
        print("decoded on the GPU; %d files fell back to PIL" % len(fallbacks))
    print("mean NIQE over %d images: %.12g" % (len(files), float(np.mean([scores[f] for f in files]))))
    return scores


if __name__ == "__main__":
    main()
