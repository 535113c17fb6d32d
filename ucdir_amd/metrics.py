"""Image conversion and full-reference metrics of the val loop (reference: core/metrics.py).

cv2 / torchvision are not available here: JPEG writing uses PIL (quality 100 like
core/metrics.py:42-45), SSIM uses scipy's correlate with the same 11x11 sigma-1.5 Gaussian window
and valid-region crop as core/metrics.py:58-99.
"""
import math

import numpy as np


def tensor2img_u8_device(tensor, min_max=(-1, 1)):
    """tensor2img for ONE image that lives on the GPU: clamp / rescale / round / HWC on the device, then a uint8 copy
    (4x fewer bytes over PCIe than the reference's fp32 ``.cpu()``; same arithmetic, same rounding: torch.round and
    numpy.round are both round-half-to-even)."""
    t = tensor.detach().squeeze().float().clamp(*min_max)
    t = (t - min_max[0]) / (min_max[1] - min_max[0])
    if t.dim() != 3:
        raise ValueError("tensor2img_u8_device takes one (3,H,W) image")
    return (t * 255.0).round().to(__import__("torch").uint8).permute(1, 2, 0).contiguous().cpu().numpy()


def tensor2img(tensor, out_type=np.uint8, min_max=(-1, 1)):
    """core/metrics.py:8-34 for 3-D / single-image 4-D tensors: clamp, rescale to [0,1], HWC, round to uint8."""
    t = tensor.squeeze().float().cpu().clamp(*min_max)
    t = (t - min_max[0]) / (min_max[1] - min_max[0])
    if t.dim() == 4:          # a stack of images: tile them in a row (make_grid is unavailable)
        t = torch_hcat(t)
    img = t.numpy()
    if img.ndim == 3:
        img = np.transpose(img, (1, 2, 0))
    if out_type == np.uint8:
        img = (img * 255.0).round()
    return img.astype(out_type)


def torch_hcat(t):
    import torch
    return torch.cat(list(t), dim=-1)


def save_jpg(img, img_path, mode="RGB"):
    from PIL import Image
    Image.fromarray(img).save(img_path.replace(".png", ".jpg"), quality=100, subsampling=0)


def save_img(img, img_path, mode="RGB"):
    from PIL import Image
    Image.fromarray(img).save(img_path)


def calculate_psnr(img1, img2):
    mse = np.mean((img1.astype(np.float64) - img2.astype(np.float64)) ** 2)
    if mse == 0:
        return float("inf")
    return 20 * math.log10(255.0 / math.sqrt(mse))


def _ssim(img1, img2):
    from scipy.ndimage import correlate
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    img1, img2 = img1.astype(np.float64), img2.astype(np.float64)
    ax = np.arange(11) - 5
    k = np.exp(-(ax ** 2) / (2 * 1.5 ** 2))
    k /= k.sum()
    window = np.outer(k, k)
    f = lambda a: correlate(a, window, mode="reflect")[5:-5, 5:-5]
    mu1, mu2 = f(img1), f(img2)
    s1 = f(img1 ** 2) - mu1 ** 2
    s2 = f(img2 ** 2) - mu2 ** 2
    s12 = f(img1 * img2) - mu1 * mu2
    return (((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s1 + s2 + C2))).mean()


def calculate_ssim(img1, img2):
    if img1.ndim == 2:
        return _ssim(img1, img2)
    return float(np.mean([_ssim(img1[..., c], img2[..., c]) for c in range(img1.shape[2])]))


def psnr_ssim_device(sr, hr):
    """calculate_psnr / calculate_ssim of the uint8 images tensor2img_u8_device makes of ``sr`` and ``hr``, scored on the GPU
    (csrc/image_metrics.hip.h) without moving the images: (B, C, H, W) or (C, H, W) CUDA tensors in [-1, 1] -> (psnr list, ssim
    list), one value per image.  One device-to-host copy of the (image, channel) sums.  PSNR is bit-equal to the host formula (the
    numpy sum of integer-valued float64 is exact, and so is the kernel's integer SSE); SSIM is the same fp64 map summed in another
    order, and NaN when H or W is below 11 like numpy's mean of an empty map."""
    import torch
    from .ucdir import image_metrics_
    if sr.dim() == 3:
        sr, hr = sr.unsqueeze(0), hr.unsqueeze(0)
    if sr.dim() != 4:
        raise ValueError("psnr_ssim_device takes (B, C, H, W) or (C, H, W) tensors")
    B, C, H, W = sr.shape
    out = torch.empty(2 * B * C, dtype=torch.int64, device=sr.device if sr.is_cuda else "cpu")
    image_metrics_(sr, hr, out=out)
    host = out.cpu()                                # the only synchronisation: sse and ssim_sum share this buffer
    sse_h = host[:B * C].tolist()
    ssim_h = host[B * C:].view(torch.float64).tolist()
    psnr, ssim = [], []
    for n in range(B):
        mse = sum(sse_h[n * C:(n + 1) * C]) / (C * H * W)
        psnr.append(float("inf") if mse == 0 else 20 * math.log10(255.0 / math.sqrt(mse)))
        if H < 11 or W < 11:
            ssim.append(float("nan"))
        else:
            ssim.append(float(np.mean([ssim_h[n * C + c] / ((H - 10) * (W - 10)) for c in range(C)])))
    return psnr, ssim



def jpeg_roundtrip_device(x_u8, quality, bgr=True):
    """JPEG encode at ``quality`` + decode of uint8 images on the GPU (csrc/jpeg_roundtrip.hip.h): byte for byte what libjpeg-turbo's
    defaults (4:2:0, ISLOW DCT; Pillow's Image.save(JPEG, quality) + convert("RGB")) make of them.  ``x_u8``: (B, H, W, 3) or
    (H, W, 3) contiguous uint8 CUDA tensor, H and W at least 16 -> a new tensor of the same shape on the same device, computed on
    the current stream.  bgr=True (the default) reproduces the reference's cv2.imencode / cv2.imdecode of an RGB array, which
    libjpeg reads as BGR (data/LRHR_dataset.py:505-506); bgr=False is the plain RGB round trip."""
    import torch
    from . import lib
    from .ucdir import _ptr, _stream_ptr
    if not torch.is_tensor(x_u8) or not x_u8.is_cuda:
        raise ValueError("jpeg_roundtrip_device takes a uint8 tensor on the GPU")
    if x_u8.dtype != torch.uint8:
        raise ValueError(f"jpeg_roundtrip_device takes uint8 images, got {x_u8.dtype}")
    if x_u8.dim() not in (3, 4) or x_u8.shape[-1] != 3:
        raise ValueError(f"jpeg_roundtrip_device takes (B, H, W, 3) or (H, W, 3) images, got {tuple(x_u8.shape)}")
    if not x_u8.is_contiguous():
        raise ValueError("jpeg_roundtrip_device takes a contiguous tensor")
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= quality <= 100:
        raise ValueError(f"jpeg_roundtrip_device: quality must be an integer in 1..100, got {quality!r}")
    x = x_u8 if x_u8.dim() == 4 else x_u8.unsqueeze(0)
    B, H, W, _ = x.shape
    if H < 16 or W < 16:
        raise ValueError(f"jpeg_roundtrip_device: H and W must be at least 16, got {H} x {W}")
    L = lib.load()
    ws = torch.empty(L.ucdir_jpeg_roundtrip_workspace_bytes(B, H, W), dtype=torch.uint8, device=x.device)
    out = torch.empty_like(x_u8)
    lib.check(L.ucdir_jpeg_roundtrip(_ptr(x), _ptr(out), B, H, W, int(quality), 1 if bgr else 0, _ptr(ws), _stream_ptr(x.device)))
    return out


RESAMPLE_FILTERS = {"box": 0, "bilinear": 1, "bicubic": 2, "lanczos": 3}


def resample_device(x_u8, size, filter="bicubic"):
    """PIL.Image.resize of uint8 RGB images on the GPU (csrc/resample.hip.h): byte for byte what Pillow's 8-bit resampling makes of
    them.  ``x_u8``: (B, H, W, 3) or (H, W, 3) contiguous uint8 CUDA tensor; ``size``: (Hout, Wout); ``filter``: one of
    RESAMPLE_FILTERS -> a new tensor of the same rank on the same device, computed on the current stream.  Equal sizes copy, as
    Pillow does."""
    import torch
    from . import lib
    from .ucdir import _ptr, _stream_ptr
    if not torch.is_tensor(x_u8) or not x_u8.is_cuda:
        raise ValueError("resample_device takes a uint8 tensor on the GPU")
    if x_u8.dtype != torch.uint8:
        raise ValueError(f"resample_device takes uint8 images, got {x_u8.dtype}")
    if x_u8.dim() not in (3, 4) or x_u8.shape[-1] != 3 or x_u8.numel() == 0:
        raise ValueError(f"resample_device takes (B, H, W, 3) or (H, W, 3) images, got {tuple(x_u8.shape)}")
    if not x_u8.is_contiguous():
        raise ValueError("resample_device takes a contiguous tensor")
    try:
        Hout, Wout = size
        ok = all(not isinstance(v, bool) and int(v) == v and v >= 1 for v in (Hout, Wout))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"resample_device: size must be (Hout, Wout) with positive integers, got {size!r}")
    if filter not in RESAMPLE_FILTERS:
        raise ValueError(f"resample_device: filter must be one of {', '.join(RESAMPLE_FILTERS)}, got {filter!r}")
    Hout, Wout = int(Hout), int(Wout)
    x = x_u8 if x_u8.dim() == 4 else x_u8.unsqueeze(0)
    B, H, W, _ = x.shape
    L = lib.load()
    nbytes = L.ucdir_resample_workspace_bytes(B, H, W, Hout, Wout)
    if nbytes < 0:
        raise ValueError(f"resample_device: {H} x {W} -> {Hout} x {Wout} is outside what ucdir_resample supports (include/ucdir_hip.h)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    out = torch.empty((B, Hout, Wout, 3), dtype=torch.uint8, device=x.device)
    lib.check(L.ucdir_resample(_ptr(x), _ptr(out), B, H, W, Hout, Wout, RESAMPLE_FILTERS[filter], _ptr(ws), _stream_ptr(x.device)))
    return out if x_u8.dim() == 4 else out[0]
