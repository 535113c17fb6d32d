"""Degradations of the real-world ("blind") super-resolution val task.

Device operators on the HIP kernels of csrc/realsr.hip.h (reference data/degradations.py:13-89, data/diffjpeg.py):
``filter2d_device``, ``usm_sharp_device``, ``diffjpeg_device``; the host makers of the blur kernels (reference
data/degradations.py:98-556) in numpy float64; ``draw_realsr_params``, every random decision of one image from
``np.random.RandomState(index)``; and ``realsr_degrade_device``, the second-order degradation chain of reference
model/model.py:459-546 on one image.  Resizes (F.interpolate) and the noise draws (torch.Generator) are PyTorch plumbing.
"""
import math
import os

import numpy as np

KERNEL_RANGE = tuple(2 * v + 1 for v in range(3, 11))          # blur kernel sizes 7, 9, ..., 21
KERNEL_PAD = 21
RESIZE_MODES = ("area", "bilinear", "bicubic")
KERNEL_TYPES = ("iso", "aniso", "generalized_iso", "generalized_aniso", "plateau_iso", "plateau_aniso")
SETTINGS_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", "realsr_degradations.yaml")


def load_settings(spec):
    """Degradation (``dopt``, ``dopt1``) or kernel (``param``, ``param1``) settings: a dict is returned as it is, a name is looked up
    in config/realsr_degradations.yaml (the reference evaluates such names as Python; here they are data)."""
    if isinstance(spec, dict):
        return spec
    import yaml
    with open(SETTINGS_FILE) as f:
        known = yaml.safe_load(f)
    if spec not in known:
        raise ValueError("unknown degradation settings %r (known: %s)" % (spec, ", ".join(known)))
    return known[spec]


# ---- device operators ------------------------------------------------------------------------------------------------------------
def _check_image(fn, x, channels=None):
    import torch
    if not torch.is_tensor(x) or not x.is_cuda:
        raise ValueError(f"{fn} takes a float32 tensor on the GPU")
    if x.dtype != torch.float32:
        raise ValueError(f"{fn} takes float32 images, got {x.dtype}")
    if x.dim() != 4 or x.numel() == 0 or (channels is not None and x.shape[1] != channels):
        raise ValueError(f"{fn} takes (B, {channels or 'C'}, H, W) images, got {tuple(x.shape)}")
    if not x.is_contiguous():
        raise ValueError(f"{fn} takes a contiguous tensor")


def filter2d_device(x, kernel):
    """``filter2D`` of the reference on the GPU: reflect-pad (B, C, H, W) by k // 2 and correlate (no flip) with ``kernel``,
    (B, k, k) - one per sample - or (1, k, k) / (k, k) - shared.  k odd, at most 21, and k // 2 below H and W."""
    import torch
    from . import lib
    from .ucdir import _ptr, _stream_ptr
    _check_image("filter2d_device", x)
    if not torch.is_tensor(kernel) or kernel.dim() not in (2, 3) or kernel.shape[-1] != kernel.shape[-2]:
        raise ValueError("filter2d_device: the kernel must be a (k, k), (1, k, k) or (B, k, k) tensor")
    kernel = kernel.to(device=x.device, dtype=torch.float32).reshape(-1, kernel.shape[-1], kernel.shape[-1]).contiguous()
    B, C, H, W = x.shape
    k = kernel.shape[-1]
    if kernel.shape[0] not in (1, B):
        raise ValueError(f"filter2d_device: {kernel.shape[0]} kernels for a batch of {B} (one, or one per sample)")
    if k % 2 == 0:
        raise ValueError(f"filter2d_device: the kernel size must be odd, got {k}")
    if k > 21:
        raise ValueError(f"filter2d_device: the kernel size must be at most 21, got {k}")
    if H <= k // 2 or W <= k // 2:
        raise ValueError(f"filter2d_device: the reflect pad {k // 2} must be smaller than the {H} x {W} plane")
    if B * C > 65535:
        raise ValueError("filter2d_device: more than 65535 planes (B * C)")
    y = torch.empty_like(x)
    lib.check(lib.load().ucdir_filter2d(_ptr(x), _ptr(kernel), _ptr(y), B, C, H, W, k, 1 if kernel.shape[0] > 1 else 0,
                                       _stream_ptr(x.device)))
    return y


def usm_sharp_device(x, radius=15, weight=0.5, threshold=10):
    """``USMSharp(radius).forward(x, weight, threshold)`` of the reference on the GPU, (B, C, H, W) in [0, 1]."""
    import torch
    from . import lib
    from .ucdir import _ptr, _stream_ptr
    _check_image("usm_sharp_device", x)
    if isinstance(radius, bool) or int(radius) != radius or radius < 1:
        raise ValueError(f"usm_sharp_device: radius must be a positive integer, got {radius!r}")
    k = int(radius) | 1
    B, C, H, W = x.shape
    if k > 21:
        raise ValueError(f"usm_sharp_device: the kernel size must be at most 21, got radius {radius}")
    if H <= k // 2 or W <= k // 2:
        raise ValueError(f"usm_sharp_device: the reflect pad {k // 2} must be smaller than the {H} x {W} plane")
    if B * C > 65535:
        raise ValueError("usm_sharp_device: more than 65535 planes (B * C)")
    L = lib.load()
    ws = torch.empty(L.ucdir_usm_sharp_workspace_bytes(B, C, H, W), dtype=torch.uint8, device=x.device)
    y = torch.empty_like(x)
    lib.check(L.ucdir_usm_sharp(_ptr(x), _ptr(y), B, C, H, W, int(radius), float(weight), float(threshold), _ptr(ws),
                                _stream_ptr(x.device)))
    return y


def quality_to_factor(quality):
    """The reference's ``quality_to_factor`` in float32, elementwise: 5000 / q / 100 below 50, else (200 - 2 q) / 100."""
    q = np.asarray(quality, dtype=np.float32)
    with np.errstate(divide="ignore"):
        low = np.float32(5000.0) / q
    high = np.float32(200.0) - q * np.float32(2.0)
    return (np.where(q < 50, low, high) / np.float32(100.0)).astype(np.float32)


def diffjpeg_device(x, quality):
    """``DiffJPEG(differentiable=False)(x, quality)`` of the reference on the GPU: (B, 3, H, W) RGB in [0, 1]; ``quality`` a number
    or a (B,) tensor, 1 <= quality < 100 (at 100 the reference divides by a zero table)."""
    import torch
    from . import lib
    from .ucdir import _ptr, _stream_ptr
    _check_image("diffjpeg_device", x, channels=3)
    B, _, H, W = x.shape
    if torch.is_tensor(quality):
        q = quality.detach().to("cpu", torch.float32).reshape(-1).numpy()
    elif isinstance(quality, bool):
        raise ValueError("diffjpeg_device: quality must be a number or a (B,) tensor")
    else:
        q = np.full(B, quality, dtype=np.float32)
    if q.shape != (B,):
        raise ValueError(f"diffjpeg_device: {q.size} qualities for a batch of {B}")
    if not np.all((q >= 1) & (q < 100)):
        raise ValueError(f"diffjpeg_device: quality must satisfy 1 <= quality < 100, got {q.tolist()}")
    if B > 65535:
        raise ValueError("diffjpeg_device: more than 65535 images")
    factors = torch.from_numpy(quality_to_factor(q)).to(x.device)
    y = torch.empty_like(x)
    lib.check(lib.load().ucdir_diffjpeg(_ptr(x), _ptr(y), _ptr(factors), B, H, W, _stream_ptr(x.device)))
    return y


# ---- host kernel makers (numpy float64) ------------------------------------------------------------------------------------------
def _quadratic_form(size, sig_x, sig_y, theta, isotropic):
    """(size, size) array of p^T Sigma^-1 p over the pixel grid centred on zero, p = (column offset, row offset)."""
    ax = np.arange(-size // 2 + 1.0, size // 2 + 1.0)
    xx, yy = np.meshgrid(ax, ax)
    if isotropic:
        sigma = np.array([[sig_x ** 2, 0.0], [0.0, sig_x ** 2]])
    else:
        rot = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
        sigma = np.dot(rot, np.dot(np.array([[sig_x ** 2, 0.0], [0.0, sig_y ** 2]]), rot.T))
    grid = np.stack([xx, yy], axis=2)
    return np.sum(np.dot(grid, np.linalg.inv(sigma)) * grid, 2)


def gaussian_kernel(size, sig_x, sig_y=None, theta=0.0, isotropic=True):
    """Bivariate Gaussian, normalised to sum 1; the isotropic form uses ``sig_x`` alone."""
    k = np.exp(-0.5 * _quadratic_form(size, sig_x, sig_y, theta, isotropic))
    return k / np.sum(k)


def generalized_gaussian_kernel(size, sig_x, sig_y, theta, beta, isotropic=True):
    """exp(-0.5 (p^T Sigma^-1 p)^beta), normalised; beta = 1 is the Gaussian."""
    k = np.exp(-0.5 * np.power(_quadratic_form(size, sig_x, sig_y, theta, isotropic), beta))
    return k / np.sum(k)


def plateau_kernel(size, sig_x, sig_y, theta, beta, isotropic=True):
    """1 / ((p^T Sigma^-1 p)^beta + 1), normalised."""
    k = np.reciprocal(np.power(_quadratic_form(size, sig_x, sig_y, theta, isotropic), beta) + 1)
    return k / np.sum(k)


def circular_lowpass_kernel(cutoff, size, pad_to=0):
    """2-D circularly symmetric sinc (ideal low-pass) filter of cutoff ``cutoff`` radians: cutoff J1(cutoff r) / (2 pi r), the
    centre tap cutoff^2 / (4 pi), normalised; zero-padded to ``pad_to`` when that is larger."""
    from scipy import special
    if size % 2 != 1:
        raise ValueError("circular_lowpass_kernel: the size must be odd")
    c = (size - 1) / 2
    i, j = np.meshgrid(np.arange(size, dtype=np.float64), np.arange(size, dtype=np.float64), indexing="ij")
    r = np.sqrt((i - c) ** 2 + (j - c) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = cutoff * special.j1(cutoff * r) / (2 * np.pi * r)
    k[(size - 1) // 2, (size - 1) // 2] = cutoff ** 2 / (4 * np.pi)
    k = k / np.sum(k)
    return pad_kernel(k, pad_to) if pad_to > size else k


def pad_kernel(k, to=KERNEL_PAD):
    """Zero-pad an odd kernel symmetrically to ``to`` x ``to``."""
    p = (to - k.shape[0]) // 2
    return np.pad(k, ((p, p), (p, p)))


def make_kernel(spec):
    """The unpadded float64 kernel a ``draw_realsr_params`` kernel spec describes."""
    kind, size = spec["type"], spec["size"]
    if kind == "pulse":
        return np.ones((1, 1))
    if kind == "sinc":
        return circular_lowpass_kernel(spec["omega"], size)
    iso = kind.endswith("iso") and not kind.endswith("aniso")
    args = (size, spec["sigma_x"], spec["sigma_y"], spec["rotation"])
    if kind.startswith("generalized"):
        return generalized_gaussian_kernel(*args, spec["beta"], isotropic=iso)
    if kind.startswith("plateau"):
        return plateau_kernel(*args, spec["beta"], isotropic=iso)
    return gaussian_kernel(*args, isotropic=iso)


# ---- the random decisions of one image -------------------------------------------------------------------------------------------
def _draw_blur(rs, kopt, suffix):
    """One blur kernel of the dataset (reference data/LRHR_dataset.py:760-790).  Draws, in order: size; sinc or not; then omega, or
    type, sigma_x, [sigma_y, rotation], [beta side, beta]."""
    size = KERNEL_RANGE[rs.randint(len(KERNEL_RANGE))]
    if rs.uniform() < kopt["sinc_prob" + suffix]:
        return {"type": "sinc", "size": size, "omega": rs.uniform(np.pi / 3 if size < 13 else np.pi / 5, np.pi)}
    names = kopt["kernel_list" + suffix]
    kind = names[rs.choice(len(names), p=np.asarray(kopt["kernel_prob" + suffix], dtype=np.float64))]
    if kind not in KERNEL_TYPES:
        raise ValueError(f"unknown blur kernel type {kind!r} (known: {', '.join(KERNEL_TYPES)})")
    lo, hi = kopt["blur_sigma" + suffix]
    spec = {"type": kind, "size": size, "sigma_x": rs.uniform(lo, hi)}
    if kind.endswith("aniso"):
        spec["sigma_y"] = rs.uniform(lo, hi)
        spec["rotation"] = rs.uniform(-math.pi, math.pi)
    else:
        spec["sigma_y"], spec["rotation"] = spec["sigma_x"], 0.0
    if kind in ("iso", "aniso"):
        return spec
    blo, bhi = kopt[("betag_range" if kind.startswith("generalized") else "betap_range") + suffix]
    spec["beta"] = rs.uniform(blo, 1) if rs.uniform() < 0.5 else rs.uniform(1, bhi)
    return spec


def _draw_resize(rs, prob, rng):
    kind = ("up", "down", "keep")[rs.choice(3, p=np.asarray(prob, dtype=np.float64))]
    scale = rs.uniform(1, rng[1]) if kind == "up" else rs.uniform(rng[0], 1) if kind == "down" else 1.0
    return {"direction": kind, "scale": float(scale), "mode": RESIZE_MODES[rs.randint(3)]}


def _draw_noise(rs, dopt, suffix):
    gaussian = bool(rs.uniform() < dopt["gaussian_noise_prob" + suffix])
    lo, hi = dopt["noise_range" + suffix] if gaussian else dopt["poisson_scale_range" + suffix]
    return {"kind": "gaussian" if gaussian else "poisson", "level": float(rs.uniform(lo, hi)),
            "gray": bool(rs.uniform() < dopt["gray_noise_prob" + suffix])}


def _draw_quality(rs, rng):
    """A JPEG quality as the float32 the reference draws, kept below 100 (diffjpeg_device refuses 100)."""
    q = np.float32(rs.uniform(rng[0], rng[1]))
    return float(min(q, np.nextafter(np.float32(100), np.float32(0))))


def draw_realsr_params(index, dopt, kopt):
    """Every random decision of image ``index`` -> dict.  All draws come from ``np.random.RandomState(index)`` in this fixed order:
    kernel1, kernel2 (``_draw_blur``); final sinc (yes/no, then size and omega); stage-1 resize (direction, scale, mode); stage-1
    noise (Gaussian or Poisson, level, grey); jpeg1; second blur yes/no; stage-2 resize; stage-2 noise; final order (sinc first or
    JPEG first); final resize mode; jpeg2; the 63-bit seed of the tensor noise.  ``dopt``: the degradation settings (reference
    model/model.py:339-386), ``kopt``: the kernel settings (reference data/LRHR_dataset.py:638-665)."""
    rs = np.random.RandomState(int(index))
    p = {"index": int(index)}
    spec1, spec2 = _draw_blur(rs, kopt, ""), _draw_blur(rs, kopt, "2")
    if rs.uniform() < kopt["final_sinc_prob"]:
        size = KERNEL_RANGE[rs.randint(len(KERNEL_RANGE))]
        spec3 = {"type": "sinc", "size": size, "omega": rs.uniform(np.pi / 3, np.pi)}
    else:
        spec3 = {"type": "pulse", "size": 1}
    p["kernel_specs"] = (spec1, spec2, spec3)
    p["kernel1"], p["kernel2"], p["sinc_kernel"] = (pad_kernel(make_kernel(s)).astype(np.float32) for s in p["kernel_specs"])
    p["resize1"] = _draw_resize(rs, dopt["resize_prob"], dopt["resize_range"])
    p["noise1"] = _draw_noise(rs, dopt, "")
    p["jpeg1"] = _draw_quality(rs, dopt["jpeg_range"])
    p["second_blur"] = bool(rs.uniform() < dopt["second_blur_prob"])
    p["resize2"] = _draw_resize(rs, dopt["resize_prob2"], dopt["resize_range2"])
    p["noise2"] = _draw_noise(rs, dopt, "2")
    p["sinc_first"] = bool(rs.uniform() < 0.5)
    p["final_mode"] = RESIZE_MODES[rs.randint(3)]
    p["jpeg2"] = _draw_quality(rs, dopt["jpeg_range2"])
    p["noise_seed"] = (int(rs.randint(0, 2 ** 31)) << 32) | int(rs.randint(0, 2 ** 32, dtype=np.uint64))
    return p


# ---- the chain -------------------------------------------------------------------------------------------------------------------
def trim_kernel(k):
    """The centred sub-kernel that holds every non-zero tap of a zero-padded kernel.  The zero border adds nothing to a sum, so the
    filter's result is the same bits, and the smaller reflect pad fits planes the padded kernel's would not."""
    k = np.asarray(k)
    c = k.shape[-1] // 2
    nz = np.argwhere(k != 0)
    r = int(np.abs(nz - c).max()) if nz.size else 0
    return k[c - r:c + r + 1, c - r:c + r + 1]


def blur_stage(x, kernel):
    import torch
    return filter2d_device(x, torch.from_numpy(np.ascontiguousarray(trim_kernel(kernel), dtype=np.float32)))


def resize_stage(x, mode, scale_factor=None, size=None):
    """``F.interpolate`` with the reference's arguments (align_corners at its default)."""
    import torch.nn.functional as F
    return F.interpolate(x, scale_factor=scale_factor, size=size, mode=mode)


def _unique_levels(img):
    import torch
    return float(2 ** np.ceil(np.log2(len(torch.unique(img)))))


def noise_stage(x, noise, gen):
    """``random_add_gaussian_noise_pt`` / ``random_add_poisson_noise_pt`` (clip=True, rounds=False) of the reference with the level
    and grey flag of ``noise`` and every tensor draw from the device generator ``gen``.  Gaussian: the grey plane is drawn first,
    then the colour noise (always).  Poisson: likewise, each on the image rounded to the u8 grid and scaled by the power of two
    at or above its count of unique values."""
    import torch
    _, _, h, w = x.shape
    level, gray = noise["level"], noise["gray"]
    if noise["kind"] == "gaussian":
        ng = torch.randn(h, w, dtype=x.dtype, device=x.device, generator=gen) * level / 255.0 if gray else None
        n = torch.randn(x.shape, dtype=x.dtype, device=x.device, generator=gen) * level / 255.0
        if gray:                                        # the colour draw above still advances the generator
            n = ng.view(1, 1, h, w).expand_as(x)
    else:
        if gray:
            g = (0.2989 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.114 * x[:, 2:3])
            g = torch.clamp((g * 255.0).round(), 0, 255) / 255.0
            vals = _unique_levels(g)
            ng = (torch.poisson(g * vals, generator=gen) / vals - g).expand(-1, 3, -1, -1)
        q = torch.clamp((x * 255.0).round(), 0, 255) / 255.0
        vals = _unique_levels(q)
        n = torch.poisson(q * vals, generator=gen) / vals - q
        if gray:
            n = ng
        n = n * level
    return torch.clamp(x + n, 0, 1)


def jpeg_stage(x, quality):
    import torch
    return diffjpeg_device(torch.clamp(x, 0, 1).contiguous(), quality)


def final_stage(x):
    import torch
    return torch.clamp((x * 255.0).round(), 0, 255) / 255.0


def realsr_degrade_device(gt, params, dopt):
    """The reference's second-order degradation (model/model.py:459-546) of one (1, 3, H, W) image in [0, 1] on the GPU with the
    decisions of ``params`` (draw_realsr_params) -> (1, 3, H // scale, W // scale) on the u8 grid.  As there, the chain starts
    from the USM-sharpened image."""
    import torch
    _check_image("realsr_degrade_device", gt, channels=3)
    if gt.shape[0] != 1:
        raise ValueError("realsr_degrade_device takes one image, (1, 3, H, W)")
    s = int(dopt["scale"])
    h, w = gt.shape[-2:]
    gen = torch.Generator(device=gt.device)
    gen.manual_seed(params["noise_seed"])
    out = blur_stage(usm_sharp_device(gt), params["kernel1"])
    out = resize_stage(out, params["resize1"]["mode"], scale_factor=params["resize1"]["scale"])
    out = noise_stage(out, params["noise1"], gen)
    out = jpeg_stage(out, params["jpeg1"])
    if params["second_blur"]:
        out = blur_stage(out.contiguous(), params["kernel2"])
    sc = params["resize2"]["scale"]
    out = resize_stage(out, params["resize2"]["mode"], size=(int(h / s * sc), int(w / s * sc)))
    out = noise_stage(out, params["noise2"], gen)
    if params["sinc_first"]:
        out = resize_stage(out, params["final_mode"], size=(h // s, w // s))
        out = blur_stage(out.contiguous(), params["sinc_kernel"])
        out = jpeg_stage(out, params["jpeg2"])
    else:
        out = jpeg_stage(out, params["jpeg2"])
        out = resize_stage(out, params["final_mode"], size=(h // s, w // s))
        out = blur_stage(out.contiguous(), params["sinc_kernel"])
    return final_stage(out)
