"""Record tests/golden/realsr_reference.npz from a checkout of the reference (CPU only):

    python tools/gen_realsr_golden.py --reference /path/to/reference

It loads the reference's data/degradations.py and data/diffjpeg.py by file and records
  * blur kernels from direct calls with explicit arguments to bivariate_Gaussian (isotropic and anisotropic),
    bivariate_generalized_Gaussian, bivariate_plateau and circular_lowpass_kernel at sizes 7, 13 and 21 (float64);
  * DiffJPEG(differentiable=False) outputs on CPU float32 at qualities 30, 50 and 95 for a 48 x 64 crop of the real photograph of
    tests/golden/sid_real_image.npz and for its 17 x 33 and 5 x 7 corners (the zero padding), with the inputs.
degradations.py imports cv2 and torchvision, which the functions recorded here never touch: when they are not installed, empty
stand-in modules take their names for the import only.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "realsr_reference.npz")

KERNEL_SIZES = (7, 13, 21)
# (sig_x, sig_y, theta, beta) of the recorded kernels, one set per size
KERNEL_ARGS = {7: (0.9, 1.7, 0.6, 0.8), 13: (2.1, 1.2, -1.1, 1.6), 21: (2.9, 0.7, 2.4, 3.1)}
SINC_CUTOFF = {7: 2.2, 13: 1.1, 21: 2.9}
JPEG_SIZES = ((48, 64), (17, 33), (5, 7))
JPEG_QUALITIES = (30.0, 50.0, 95.0)


def load_by_file(name, path, stand_ins=()):
    added = []
    for mod in stand_ins:
        try:
            importlib.import_module(mod)
        except ImportError:
            sys.modules[mod] = types.ModuleType(mod)
            added.append(mod)
    if "torchvision.transforms.functional_tensor" in added:
        sys.modules["torchvision.transforms.functional_tensor"].rgb_to_grayscale = None
    try:
        spec = importlib.util.spec_from_file_location(name, path)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        for mod in added:
            del sys.modules[mod]
    return m


def jpeg_inputs():
    """(3, 3, H, W) float32 inputs per size: the photograph's crop three times (one per quality), values u8 / 255."""
    real = np.load(os.path.join(ROOT, "tests", "golden", "sid_real_image.npz"))["cond_u8"]
    out = {}
    for H, W in JPEG_SIZES:
        img = (real[:H, :W].astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)
        out[(H, W)] = np.ascontiguousarray(np.stack([img] * len(JPEG_QUALITIES)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a checkout of the reference")
    args = ap.parse_args()
    deg = load_by_file("ref_degradations", os.path.join(args.reference, "data", "degradations.py"),
                       ("cv2", "torchvision", "torchvision.transforms", "torchvision.transforms.functional_tensor"))
    dj = load_by_file("ref_diffjpeg", os.path.join(args.reference, "data", "diffjpeg.py"))
    rec = {"kernel_sizes": np.array(KERNEL_SIZES), "jpeg_qualities": np.array(JPEG_QUALITIES, dtype=np.float32)}
    for k in KERNEL_SIZES:
        sx, sy, th, beta = KERNEL_ARGS[k]
        rec[f"args_{k}"] = np.array([sx, sy, th, beta, SINC_CUTOFF[k]])
        rec[f"iso_{k}"] = deg.bivariate_Gaussian(k, sx, sy, th, isotropic=True)
        rec[f"aniso_{k}"] = deg.bivariate_Gaussian(k, sx, sy, th, isotropic=False)
        rec[f"generalized_iso_{k}"] = deg.bivariate_generalized_Gaussian(k, sx, sy, th, beta, isotropic=True)
        rec[f"generalized_aniso_{k}"] = deg.bivariate_generalized_Gaussian(k, sx, sy, th, beta, isotropic=False)
        rec[f"plateau_iso_{k}"] = deg.bivariate_plateau(k, sx, sy, th, beta, isotropic=True)
        rec[f"plateau_aniso_{k}"] = deg.bivariate_plateau(k, sx, sy, th, beta, isotropic=False)
        rec[f"sinc_{k}"] = deg.circular_lowpass_kernel(SINC_CUTOFF[k], k, pad_to=0)
    rec["sinc_7_pad21"] = deg.circular_lowpass_kernel(SINC_CUTOFF[7], 7, pad_to=21)
    jpeger = dj.DiffJPEG(differentiable=False)
    with torch.no_grad():
        for (H, W), x in jpeg_inputs().items():
            q = torch.tensor(JPEG_QUALITIES, dtype=torch.float32)
            rec[f"jpeg_in_{H}x{W}"] = x
            rec[f"jpeg_out_{H}x{W}"] = jpeger(torch.from_numpy(x.copy()), quality=q).numpy().astype(np.float32)
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
