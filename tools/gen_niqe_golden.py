#!/usr/bin/env python
"""Write the NIQE fixtures of tests/golden/ from the reference's own metric/niqe.py (run where a checkout of the reference is at hand;
no test imports this file).

    python tools/gen_niqe_golden.py --reference /path/to/reference

cv2 is not needed: the one call the reference makes, cv2.resize(img, (w // 2, h // 2), INTER_LINEAR) at an exact factor of 2, is
stood in for by the 2x2 mean (a + b + c + d) * 0.25f that OpenCV computes at that factor.  The feature matrix is recorded by wrapping
the module's compute_feature (the reference loops over scale 1's blocks, then scale 2's).

Outputs:
  tests/golden/niqe_pris_params.npz   the reference's pristine-model data file, copied byte for byte
  tests/golden/niqe_reference.npz     names, and per image: img_<name> uint8 RGB, niqe_<name>, feats_<name> (nblk, 36)
"""
import argparse
import importlib
import os
import shutil
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def cv2_stand_in():
    m = types.ModuleType("cv2")
    m.INTER_LINEAR = 1

    def resize(img, dsize, interpolation=None):
        w, h = dsize
        assert img.dtype == np.float32 and img.shape == (2 * h, 2 * w) and interpolation == m.INTER_LINEAR
        return (((img[0::2, 0::2] + img[0::2, 1::2]) + img[1::2, 0::2]) + img[1::2, 1::2]) * np.float32(0.25)
    m.resize = resize
    return m


def smooth_plus_noise(rs, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 90 * np.sin(xx / (9.0 + 4 * c) + c) * np.cos(yy / (13.0 - 3 * c)) for c in range(3)], -1)
    return np.clip(base + rs.normal(0, 12, (h, w, 3)), 0, 255).round().astype(np.uint8)


def make_images(reference):
    from PIL import Image
    rs = np.random.RandomState(20240)
    imgs = {"smooth192": smooth_plus_noise(rs, 192, 192), "smooth200x300": smooth_plus_noise(rs, 200, 300)}
    noise = rs.randint(0, 256, (192, 288, 3)).astype(np.uint8)
    imgs["noise"] = noise
    black, grey = noise.copy(), noise.copy()
    black[:, :104] = 0
    grey[:, :104] = 77
    imgs["black_cols"], imgs["grey_cols"] = black, grey
    face = np.asarray(Image.open(os.path.join(reference, "dataset", "celebahq_16_128", "hr_128", "00031.png")).convert("RGB"))
    imgs["natural"] = np.ascontiguousarray(np.tile(face, (2, 2, 1))[:200, :250])
    return imgs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    args = ap.parse_args()
    ref = os.path.abspath(args.reference)
    sys.modules["cv2"] = cv2_stand_in()
    sys.path.insert(0, ref)
    os.chdir(ref)                                       # calculate_niqe opens ./metric/niqe_pris_params.npz
    warnings.simplefilter("ignore")
    rn = importlib.import_module("metric.niqe")
    rows = []
    real = rn.compute_feature

    def recording(block):
        f = real(block)
        rows.append(f)
        return f
    rn.compute_feature = recording

    out = {}
    imgs = make_images(ref)
    for name, img in imgs.items():
        rows.clear()
        score = rn.calculate_niqe(img[..., ::-1], 0, "HWC", "y")        # the reference takes BGR
        nblk = len(rows) // 2
        feats = np.concatenate([np.array(rows[:nblk], np.float64), np.array(rows[nblk:], np.float64)], axis=1)
        assert feats.shape == ((img.shape[0] // 96) * (img.shape[1] // 96), 36)
        out["img_" + name], out["niqe_" + name], out["feats_" + name] = img, np.float64(np.asarray(score).reshape(())), feats
        print("%-14s %s  NIQE %.9g  NaN rows %d of %d" % (name, img.shape, out["niqe_" + name], np.isnan(feats).any(1).sum(), nblk))
    out["names"] = np.array(list(imgs))
    os.makedirs(GOLDEN, exist_ok=True)
    np.savez_compressed(os.path.join(GOLDEN, "niqe_reference.npz"), **out)
    shutil.copyfile(os.path.join(ref, "metric", "niqe_pris_params.npz"), os.path.join(GOLDEN, "niqe_pris_params.npz"))
    print("niqe_reference.npz: %d bytes" % os.path.getsize(os.path.join(GOLDEN, "niqe_reference.npz")))


if __name__ == "__main__":
    main()
