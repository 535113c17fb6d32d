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


def tensor2img_u8_batch_device(tensor, min_max=(-1, 1)):
    """tensor2img_u8_device for a whole (B, 3, H, W) batch, left ON the device: the same clamp / rescale / round -> a contiguous
    (B, H, W, 3) uint8 tensor, bit-equal per image to the per-image function (the operations are elementwise)."""
    if tensor.dim() != 4 or tensor.shape[1] != 3:
        raise ValueError(f"tensor2img_u8_batch_device takes a 4-D (B, 3, H, W) batch, got {tuple(tensor.shape)}")
    t = tensor.detach().float().clamp(*min_max)
    t = (t - min_max[0]) / (min_max[1] - min_max[0])
    return (t * 255.0).round().to(__import__("torch").uint8).permute(0, 2, 3, 1).contiguous()


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


def jpeg_encode_device(x_u8, quality=100, subsampling=0, bgr=False):
    """Baseline JPEG files of uint8 images, encoded on the GPU (csrc/jpeg_encode.hip.h): byte for byte what Pillow's
    Image.save(JPEG, quality=quality, subsampling=subsampling) writes.  ``x_u8``: (B, H, W, 3) or (H, W, 3) contiguous uint8 CUDA
    tensor, H and W from 1 -> a list of ``bytes``, one complete file per image, encoded on the current stream.  subsampling 0 is
    4:4:4 (what save_jpg writes), 2 is 4:2:0 (libjpeg's default); bgr=True reads channel 0 as B and channel 2 as R.  The call waits
    once, for the B file lengths; then only the used bytes of every slot cross PCIe, packed into one copy."""
    import torch
    from . import lib
    from .ucdir import _ptr, _stream_ptr
    if not torch.is_tensor(x_u8) or not x_u8.is_cuda:
        raise ValueError("jpeg_encode_device takes a uint8 tensor on the GPU")
    if x_u8.dtype != torch.uint8:
        raise ValueError(f"jpeg_encode_device takes uint8 images, got {x_u8.dtype}")
    if x_u8.dim() not in (3, 4) or x_u8.shape[-1] != 3 or x_u8.numel() == 0:
        raise ValueError(f"jpeg_encode_device takes (B, H, W, 3) or (H, W, 3) images, got {tuple(x_u8.shape)}")
    if not x_u8.is_contiguous():
        raise ValueError("jpeg_encode_device takes a contiguous tensor")
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= quality <= 100:
        raise ValueError(f"jpeg_encode_device: quality must be an integer in 1..100, got {quality!r}")
    if isinstance(subsampling, bool) or subsampling not in (0, 2):
        raise ValueError(f"jpeg_encode_device: subsampling must be 0 (4:4:4) or 2 (4:2:0), got {subsampling!r}")
    x = x_u8 if x_u8.dim() == 4 else x_u8.unsqueeze(0)
    B, H, W, _ = x.shape
    L = lib.load()
    nbytes, bound = L.ucdir_jpeg_encode_workspace_bytes(B, H, W, subsampling), L.ucdir_jpeg_encode_bound(H, W, subsampling)
    if nbytes < 0 or bound < 0:
        raise ValueError(f"jpeg_encode_device: {B} x {H} x {W} is outside what ucdir_jpeg_encode supports (include/ucdir_hip.h)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    out = torch.empty((B, bound), dtype=torch.uint8, device=x.device)
    lengths = torch.empty(B, dtype=torch.int32, device=x.device)
    lib.check(L.ucdir_jpeg_encode(_ptr(x), _ptr(out), _ptr(lengths), B, H, W, int(quality), int(subsampling), 1 if bgr else 0, _ptr(ws),
                                  _stream_ptr(x.device)))
    n = lengths.cpu().tolist()                      # the synchronisation
    if min(n) < 0:
        raise lib.UcdirError("ucdir_jpeg_encode: a file would pass ucdir_jpeg_encode_bound; nothing was written for it")
    packed = torch.cat([out[i, :n[i]] for i in range(B)]).cpu().numpy().tobytes()
    ends = np.cumsum(n).tolist()
    return [packed[e - k:e] for e, k in zip(ends, n)]


class JpegUnsupported(ValueError):
    """A file jpeg_decode_device does not decode: ``code`` is what ucdir_jpeg_decode_info answered (positive: valid but not built,
    negative: damaged) or, with ``device_status`` set, the damage bits the kernels found in the entropy data; ``reason`` says it
    in words."""

    def __init__(self, code, reason, device_status=False):
        super().__init__(f"jpeg_decode_device: {reason} (code {code})")
        self.code, self.reason, self.device_status = code, reason, device_status


JPEG_INFO_FIELDS = ("width", "height", "components", "h_samp", "v_samp", "restart_interval", "blocks_per_mcu", "blocks", "segments",
                    "packed_bytes", "entropy_bytes", "mcus_x", "mcus_y", "subsequences", "subsequence_bits", "reserved")
JPEG_INFO_REASONS = {
    1: "progressive or another SOF than baseline", 2: "arithmetic coding", 3: "12-bit samples",
    4: "four components or an RGB / YCCK coded file", 5: "a sampling other than 4:4:4, 4:2:2 or 4:2:0", 6: "more than one scan",
    7: "16-bit quantisation tables", 8: "entropy data above 2^28 bytes",
    -1: "no SOI: not a JPEG file", -2: "a truncated segment or a bad length", -3: "a table the scan needs is missing",
    -4: "no SOS", -5: "no EOI", -6: "bad header values", -7: "restart markers that do not fit the restart interval"}
JPEG_STATUS_BITS = {1: "a category out of range", 2: "a code outside its Huffman table", 4: "a coefficient outside its block or segment",
                    8: "a wrong block total", 16: "no fixed point", 32: "a bad segment table"}


def _jpeg_info_words(data):
    """(code, the 16 info words as a numpy int32 array)"""
    from . import lib
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise ValueError(f"a JPEG file is given as bytes, got {type(data).__name__}")
    buf = np.frombuffer(data, dtype=np.uint8)
    info = np.zeros(16, dtype=np.int32)
    src = np.ascontiguousarray(buf) if len(buf) else np.zeros(1, np.uint8)
    return lib.load().ucdir_jpeg_decode_info(src.ctypes.data, len(buf), info.ctypes.data), info, src


def jpeg_info(data):
    """What ucdir_jpeg_decode_info says about the bytes of a JPEG file: a dict of JPEG_INFO_FIELDS.  Host only.  Raises
    JpegUnsupported for every file jpeg_decode_device would not take."""
    code, info, _ = _jpeg_info_words(data)
    if code != 0:
        raise JpegUnsupported(code, JPEG_INFO_REASONS.get(code, "unknown"))
    return dict(zip(JPEG_INFO_FIELDS, info.tolist()))


def _jpeg_crop(crop, info, who):
    """``crop`` (None: the whole image) as four ints inside the image of ``info``, or a ValueError in ``who``'s name."""
    W, H = int(info[0]), int(info[1])
    if crop is None:
        return 0, 0, W, H
    try:
        x0, y0, w, h = crop
        ok = all(not isinstance(v, bool) and int(v) == v for v in crop)
    except (TypeError, ValueError):
        ok = False
    if not ok or w < 1 or h < 1 or x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
        raise ValueError(f"{who}: crop (left, top, width, height) = {crop!r} does not lie inside the {W} x {H} image")
    return int(x0), int(y0), int(w), int(h)


def jpeg_decode_device(data, crop=None, bgr=False, device=None):
    """Decode the bytes of a baseline JPEG file on the GPU (csrc/jpeg_decode.hip.h): byte for byte what Pillow's
    Image.open(...).convert("RGB") gives.  ``data``: bytes; ``crop``: None or (left, top, width, height) inside the image;
    bgr=True swaps channels 0 and 2; ``device``: a CUDA device (default: the current one) -> an (h, w, 3) uint8 tensor there, decoded
    on the current stream.  The host frames the file (markers, tables, byte unstuffing) and uploads it in one copy; the call waits
    once, for the status word.  Raises JpegUnsupported for every file outside what include/ucdir_hip.h lists and for damaged
    entropy data."""
    import torch
    from . import lib
    from .ucdir import _ptr, _stream_ptr
    code, info, src = _jpeg_info_words(data)
    if code != 0:
        raise JpegUnsupported(code, JPEG_INFO_REASONS.get(code, "unknown"))
    L = lib.load()
    x0, y0, w, h = _jpeg_crop(crop, info, "jpeg_decode_device")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"jpeg_decode_device decodes on a GPU, got device {dev}")
    packed = torch.empty(int(info[9]), dtype=torch.uint8)
    n = L.ucdir_jpeg_decode_pack(src.ctypes.data, len(data), packed.data_ptr(), packed.numel())
    nbytes = L.ucdir_jpeg_decode_workspace_bytes(info.ctypes.data)
    if n != packed.numel() or nbytes < 0:
        raise lib.UcdirError("ucdir_jpeg_decode_pack / ucdir_jpeg_decode_workspace_bytes disagree with ucdir_jpeg_decode_info")
    with torch.cuda.device(dev):
        packed_dev = packed.to(dev)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty((int(h), int(w), 3), dtype=torch.uint8, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        lib.check(L.ucdir_jpeg_decode(_ptr(packed_dev), packed.numel(), info.ctypes.data, _ptr(out), int(x0), int(y0), int(w), int(h),
                                      1 if bgr else 0, _ptr(ws), _ptr(status), _stream_ptr(dev)))
        st = int(status.item())                        # the synchronisation
    if st != 0:
        raise JpegUnsupported(st, _damage_reason(st), device_status=True)
    return out


def _damage_reason(st):
    return "damaged entropy data: " + ", ".join(v for k, v in JPEG_STATUS_BITS.items() if st & k)


def jpeg_decode_batch_device(datas, crops=None, bgr=False, device=None):
    """Decode the bytes of several baseline JPEG files on the GPU in one call (csrc/jpeg_decode.hip.h, "several files per call").
    ``datas``: a sequence of bytes; ``crops``: None, or per file None or (left, top, width, height); ``bgr`` and ``device`` as
    jpeg_decode_device takes them -> a list: entry k is the (h, w, 3) uint8 tensor jpeg_decode_device(datas[k], crops[k]) returns,
    or, for a file that decoder does not take, the JpegUnsupported it would raise, as an instance in the list (a refusal by the
    host framing: the info code; damage the kernels found: that file's status bits, device_status=True); the other files are not
    affected.  One parse and pack per file on the host, one upload, one batch call, and one wait for all status words.  The
    tensors are views into ONE allocation that lives as long as any of them: clone what is to outlive the rest cheaply.
    Raises ValueError, naming the file's position, for an entry that is not bytes or a crop outside its image."""
    import torch
    from . import lib
    from .ucdir import _ptr, _stream_ptr
    datas = list(datas)
    crops = [None] * len(datas) if crops is None else list(crops)
    if len(crops) != len(datas):
        raise ValueError(f"jpeg_decode_batch_device: {len(crops)} crops for {len(datas)} files")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"jpeg_decode_batch_device decodes on a GPU, got device {dev}")
    res, take = [None] * len(datas), []                   # take: (position, info words, file bytes as an array, crop)
    for k, (data, crop) in enumerate(zip(datas, crops)):
        try:
            code, info, src = _jpeg_info_words(data)
        except ValueError as e:
            raise ValueError(f"jpeg_decode_batch_device: file {k}: {e}") from None
        if code != 0:
            res[k] = JpegUnsupported(code, JPEG_INFO_REASONS.get(code, "unknown"))
            continue
        take.append((k, info, src, _jpeg_crop(crop, info, f"jpeg_decode_batch_device: file {k}")))
    if not take:
        return res
    L = lib.load()
    n = len(take)
    infos = np.ascontiguousarray(np.stack([t[1] for t in take]))
    crop_arr = np.array([t[3] for t in take], np.int32)
    ws_bytes = np.zeros(1, np.int64)
    table = L.ucdir_jpeg_decode_batch_plan(n, infos.ctypes.data, None, None, None, None, 0, ws_bytes.ctypes.data)
    if table < 0:
        lib.check(1)
    packed_off = table + np.concatenate([[0], np.cumsum((infos[:, 9].astype(np.int64) + 15) // 16 * 16)])
    npix = crop_arr[:, 2].astype(np.int64) * crop_arr[:, 3]
    out_off = np.concatenate([[0], np.cumsum(3 * npix)]).astype(np.int64)
    packed_off = packed_off.astype(np.int64)
    buf = torch.zeros(int(packed_off[-1]), dtype=torch.uint8)
    for j, (_, info, src, _) in enumerate(take):
        if L.ucdir_jpeg_decode_pack(src.ctypes.data, len(src), buf.data_ptr() + int(packed_off[j]), int(info[9])) != int(info[9]):
            raise lib.UcdirError("ucdir_jpeg_decode_pack disagrees with ucdir_jpeg_decode_info")
    if L.ucdir_jpeg_decode_batch_plan(n, infos.ctypes.data, crop_arr.ctypes.data, packed_off.ctypes.data, out_off.ctypes.data,
                                      buf.data_ptr(), buf.numel(), None) != table:
        lib.check(1)
    with torch.cuda.device(dev):
        buf_dev = buf.to(dev)                             # the one upload
        ws = torch.empty(int(ws_bytes[0]), dtype=torch.uint8, device=dev)
        out = torch.empty(int(out_off[-1]), dtype=torch.uint8, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        lib.check(L.ucdir_jpeg_decode_batch(_ptr(buf_dev), buf.data_ptr(), buf.numel(), _ptr(out), out.numel(), 1 if bgr else 0, _ptr(ws),
                                            ws.numel(), _ptr(status), _stream_ptr(dev)))
        st = status.cpu().tolist()                        # the one synchronisation
    for j, (k, _, _, (_, _, w, h)) in enumerate(take):
        if st[j] != 0:
            res[k] = JpegUnsupported(st[j], _damage_reason(st[j]), device_status=True)
        else:
            res[k] = out[int(out_off[j]):int(out_off[j + 1])].view(h, w, 3)
    return res


def load_rgb_u8(path, decode_device="cpu", fallbacks=None):
    """An image file as (H, W, 3) uint8 RGB.  "cpu": Image.open(path).convert("RGB") as a numpy array.  "gpu": the file's bytes
    decoded by jpeg_decode_device, a tensor on the current GPU with the same pixels; a file that decoder does not take (not a JPEG,
    progressive, ...) is decoded with Pillow and uploaded, and ``fallbacks`` (a list) gains (path, reason)."""
    from PIL import Image
    if decode_device not in ("cpu", "gpu"):
        raise ValueError(f"decode_device must be 'cpu' or 'gpu', got {decode_device!r}")
    if decode_device == "gpu":
        import torch
        with open(path, "rb") as f:
            data = f.read()
        try:
            return jpeg_decode_device(data)
        except JpegUnsupported as e:
            if fallbacks is not None:
                fallbacks.append((path, e.reason))
            return torch.from_numpy(np.array(Image.open(path).convert("RGB"), dtype=np.uint8)).cuda()
    return np.asarray(Image.open(path).convert("RGB"))


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


# ---- NIQE, the no-reference score of the val loop (reference metric/niqe.py calculate_niqe(img, 0, 'HWC', 'y')) ------------------
# The recipe: the image-sized part runs in the reference's float32 steps (scipy's filter returns the input's
# dtype), everything per block and after it in float64.  niqe_features_host / calculate_niqe are the project's CPU oracle of
# csrc/niqe.hip.h; niqe_device is the same arithmetic on the GPU up to the summation order of the block moments.
NIQE_BLOCK = 96
NIQE_NGRID = 9801
NIQE_ALPHA_COLS = (0, 2, 6, 10, 14, 18, 20, 24, 28, 32)
_NIQE_SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
_niqe_tables_cache = {}


def load_niqe_params(path):
    """The pristine-image model of NIQE (the reference's metric/niqe_pris_params.npz): ``mu`` (36,), ``cov`` (36, 36) and the 7x7
    Gaussian ``window``, all float64."""
    import os
    if not os.path.isfile(path):
        raise FileNotFoundError(f"NIQE pristine-model file {path!r} is missing (the reference ships it as metric/niqe_pris_params.npz; "
                                "pass its location with --niqe-params)")
    with np.load(path) as z:
        return {"mu": np.asarray(z["mu_pris_param"], np.float64).reshape(-1),
                "cov": np.asarray(z["cov_pris_param"], np.float64),
                "window": np.ascontiguousarray(z["gaussian_window"], np.float64)}


def niqe_tables():
    """(4, 9801) float64: gamma(1/a), gamma(2/a), gamma(3/a) and r_gam = g2^2 / (g1 g3) on a = arange(0.2, 10.001, 0.001).  Made once;
    the kernel evaluates no gamma function."""
    if "t" not in _niqe_tables_cache:
        from scipy.special import gamma
        a = np.arange(0.2, 10.001, 0.001)
        g1, g2, g3 = gamma(1 / a), gamma(2 / a), gamma(3 / a)
        _niqe_tables_cache["t"] = np.ascontiguousarray(np.stack([g1, g2, g3, g2 * g2 / (g1 * g3)]))
        _niqe_tables_cache["a"] = a
        assert a.size == NIQE_NGRID
    return _niqe_tables_cache["t"]


def _niqe_check_shape(C, H, W):
    if C not in (1, 3):
        raise ValueError(f"NIQE takes images of 1 or 3 channels, got {C}")
    if H < NIQE_BLOCK or W < NIQE_BLOCK:
        raise ValueError(f"NIQE needs at least {NIQE_BLOCK} pixels on each side, got {H} x {W}")
    if (H // NIQE_BLOCK) * (W // NIQE_BLOCK) < 2:
        raise ValueError(f"NIQE needs at least 2 blocks of {NIQE_BLOCK} x {NIQE_BLOCK} (a covariance over blocks), got {H} x {W}")


def niqe_y(img):
    """Step 1: the float32 Y plane in [0, 255] of a uint8 RGB (H, W, 3) or grey (H, W) / (H, W, 1) image."""
    img = np.asarray(img)
    if img.dtype != np.uint8:
        raise ValueError(f"NIQE takes uint8 images, got {img.dtype}")
    if img.ndim == 3 and img.shape[2] not in (1, 3):
        raise ValueError(f"NIQE takes images of 1 or 3 channels, got {img.shape[2]}")
    if img.ndim == 3 and img.shape[2] == 1:
        img = img[..., 0]
    if img.ndim == 2:
        return img.astype(np.float32)
    if img.ndim != 3:
        raise ValueError(f"NIQE takes (H, W, 3) or (H, W) images, got shape {img.shape}")
    x = img.astype(np.float32) / np.float32(255)
    r, g, b = (x[..., c].astype(np.float64) for c in range(3))
    y64 = b * 24.966 + g * 128.553 + r * 65.481 + 16.0
    return (y64 / 255.0).astype(np.float32) * np.float32(255)


def niqe_mscn_host(Y, window):
    """Step 3: (Y - mu) / (sigma + 1), float32, 7x7 window with replicated borders."""
    from scipy.ndimage import correlate
    Y = np.ascontiguousarray(Y, np.float32)
    mu = correlate(Y, window, mode="nearest")
    e2 = correlate(Y * Y, window, mode="nearest")
    sigma = np.sqrt(np.abs(e2 - mu * mu))
    return (Y - mu) / (sigma + np.float32(1))


def _niqe_aggd(m, tables):
    """estimate_aggd_param of one float32 map, in float64: (grid index, alpha, beta_l, beta_r)."""
    v = m.astype(np.float64).ravel()
    neg, pos = v[v < 0], v[v > 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        left = np.sqrt(np.float64(np.sum(neg * neg)) / np.float64(neg.size))
        right = np.sqrt(np.float64(np.sum(pos * pos)) / np.float64(pos.size))
        g = left / right
        rhat = (np.sum(np.abs(v)) / v.size) ** 2 / (np.sum(v * v) / v.size + 1e-10)
        rhatnorm = (rhat * (g * g * g + 1) * (g + 1)) / ((g * g + 1) * (g * g + 1))
        i = 0 if np.isnan(rhatnorm) else int(np.argmin((tables[3] - rhatnorm) ** 2))
        s = np.sqrt(tables[0][i] / tables[2][i])
        return i, _niqe_tables_cache["a"][i], left * s, right * s


def _niqe_block_features(block, tables):
    i, alpha, bl, br = _niqe_aggd(block, tables)
    feat = [alpha, (bl + br) / 2]
    for sh in _NIQE_SHIFTS:
        i, alpha, bl, br = _niqe_aggd(block * np.roll(block, sh, axis=(0, 1)), tables)
        feat += [alpha, (br - bl) * (tables[1][i] / tables[0][i]), bl, br]
    return feat


def niqe_features_host(img, params, return_mscn=False):
    """Steps 1-5 on the host: the (nblk, 36) float64 feature matrix of a uint8 RGB / grey image (NaN where a block is flat);
    with ``return_mscn`` also the two float32 MSCN planes."""
    Y = niqe_y(img)
    _niqe_check_shape(1 if np.asarray(img).ndim == 2 else np.asarray(img).shape[2], *Y.shape)
    tables = niqe_tables()
    nh, nw = Y.shape[0] // NIQE_BLOCK, Y.shape[1] // NIQE_BLOCK
    Y = np.ascontiguousarray(Y[:nh * NIQE_BLOCK, :nw * NIQE_BLOCK])
    feats, planes = [], []
    for scale in (1, 2):
        n = niqe_mscn_host(Y, params["window"])
        planes.append(n)
        bs = NIQE_BLOCK // scale
        feats.append(np.array([_niqe_block_features(n[ih * bs:(ih + 1) * bs, iw * bs:(iw + 1) * bs], tables)
                               for iw in range(nw) for ih in range(nh)], np.float64))
        if scale == 1:
            t = Y / np.float32(255)
            Y = (((t[0::2, 0::2] + t[0::2, 1::2]) + t[1::2, 0::2]) + t[1::2, 1::2]) * np.float32(0.25) * np.float32(255)
    feats = np.concatenate(feats, axis=1)
    return (feats, planes) if return_mscn else feats


def niqe_from_features(feats, params):
    """Step 6: fit a Gaussian to the feature rows and return its distance to the pristine model; NaN when fewer than 2 rows are
    NaN-free (no covariance)."""
    feats = np.asarray(feats, np.float64)
    good = feats[~np.isnan(feats).any(axis=1)]
    if good.shape[0] < 2:
        return float("nan")
    mu = np.nanmean(feats, axis=0)
    cov = np.cov(good, rowvar=False)
    d = params["mu"] - mu
    return float(np.sqrt(d @ np.linalg.pinv((params["cov"] + cov) / 2) @ d))


def calculate_niqe(img, params):
    """NIQE of a uint8 RGB (H, W, 3) or grey (H, W) image on the host."""
    return niqe_from_features(niqe_features_host(img, params), params)


def niqe_features_device(x, params, return_mscn=False):
    """Steps 1-5 on the GPU (csrc/niqe.hip.h) for fp32 (B, C, H, W) CUDA images in [-1, 1], read in place (unit column stride):
    a (B, nblk, 36) float64 CPU tensor, one device-to-host copy; with ``return_mscn`` also the (B, 5/4 Hc Wc) float32 MSCN planes
    (scale 1 then scale 2 per image) as a CUDA tensor."""
    import torch
    from . import lib
    from .ucdir import _ptr, _stream_ptr
    if not torch.is_tensor(x) or not x.is_cuda:
        raise ValueError("niqe_device takes a tensor on the GPU")
    if x.dtype != torch.float32:
        raise ValueError(f"niqe_device takes fp32 images, got {x.dtype}")
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if x.dim() != 4 or x.shape[0] < 1:
        raise ValueError(f"niqe_device takes (B, C, H, W) or (C, H, W) images, got {tuple(x.shape)}")
    B, C, H, W = x.shape
    _niqe_check_shape(C, H, W)
    if x.stride(3) != 1:
        raise ValueError("niqe_device: the column stride of x must be 1")
    L = lib.load()
    key = ("dev", x.device)
    if key not in _niqe_tables_cache:
        _niqe_tables_cache[key] = torch.from_numpy(niqe_tables()).to(x.device)
    tables = _niqe_tables_cache[key]
    nbytes = L.ucdir_niqe_workspace_bytes(B, C, H, W)
    if nbytes < 0:
        raise ValueError(f"niqe_device: {C} x {H} x {W} is outside what ucdir_niqe_features supports (include/ucdir_hip.h)")
    nblk = (H // NIQE_BLOCK) * (W // NIQE_BLOCK)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=x.device)
    feats = torch.empty((B, nblk, 36), dtype=torch.float64, device=x.device)
    mscn = torch.empty((B, nblk * NIQE_BLOCK * NIQE_BLOCK * 5 // 4), dtype=torch.float32, device=x.device) if return_mscn else None
    window = np.ascontiguousarray(params["window"], np.float64)
    if window.shape != (7, 7):
        raise ValueError("niqe_device: the Gaussian window must be 7 x 7")
    lib.check(L.ucdir_niqe_features(_ptr(x), x.stride(0), x.stride(1), x.stride(2), B, C, H, W, window.ctypes.data, _ptr(tables),
                                    _ptr(feats), _ptr(mscn) if return_mscn else None, _ptr(ws), _stream_ptr(x.device)))
    host = feats.cpu()
    return (host, mscn) if return_mscn else host


def niqe_device(x, params):
    """NIQE of the uint8 images tensor2img_u8_device makes of ``x``, (B, C, H, W) or (C, H, W) fp32 CUDA tensors in [-1, 1], with the
    image-sized work on the GPU: a list of floats, one per image.  The 36 x 36 algebra of step 6 stays on the host."""
    return [niqe_from_features(f, params) for f in niqe_features_device(x, params).numpy()]


# ---- LPIPS (AlexNet variant), the full-reference perceptual score of the reference's eval1.py ------------------------------------
# The definition: x = q / 127.5 - 1, (x - shift) / scale, the five ReLU taps of torchvision's AlexNet
# ``features``, unit-normalised over channels, squared difference weighted by the 1x1 ``lin`` layers, spatial mean, summed over the
# taps.  No weights ship: load_lpips_weights reads the user's files.  calculate_lpips is the host path in torch CPU ops (float64:
# the tests' oracle of csrc/lpips.hip.h), lpips_device the same arithmetic on the GPU.
LPIPS_SHIFT = (-0.030, -0.088, -0.188)
LPIPS_SCALE = (0.458, 0.448, 0.450)
# (state-dict prefix, Cin, Cout, kernel, stride, pad, 3/2 max pool in front)
LPIPS_LAYERS = (("features.0", 3, 64, 11, 4, 2, False), ("features.3", 64, 192, 5, 1, 2, True), ("features.6", 192, 384, 3, 1, 1, True),
                ("features.8", 384, 256, 3, 1, 1, False), ("features.10", 256, 256, 3, 1, 1, False))
LPIPS_MIN_SIDE = 31
_lpips_handles = {}


def lpips_weight_shapes():
    """Name -> shape of the 15 tensors LPIPS-alex needs (the ``lin`` weights may also come as (1, C, 1, 1))."""
    out = {}
    for l, (key, cin, cout, k, _, _, _) in enumerate(LPIPS_LAYERS):
        out[key + ".weight"] = (cout, cin, k, k)
        out[key + ".bias"] = (cout,)
        out[f"lin{l}.model.1.weight"] = (cout,)
    return out


def load_lpips_weights(paths):
    """The LPIPS-alex tensors from one or more ``.npz`` / ``.pth`` files, merged (later files win): torchvision's AlexNet state dict
    (``features.N.weight`` / ``.bias``) and the lpips package's ``alex.pth`` (``linL.model.1.weight``) are the two files in the wild.
    Keys it does not need are ignored; a missing file or tensor stops with a message that names it.  Returns name -> float32 array."""
    import os
    if isinstance(paths, (str, bytes, os.PathLike)):
        paths = [paths]
    paths = [os.fspath(p) for p in paths]
    if not paths:
        raise ValueError("load_lpips_weights needs at least one file (--lpips-weights)")
    need = lpips_weight_shapes()
    found = {}
    for path in paths:
        if not os.path.isfile(path):
            raise FileNotFoundError(f"LPIPS weight file {path!r} is missing (pass torchvision's AlexNet state dict and the lpips package's "
                                    "alex.pth, as .pth or .npz, with --lpips-weights)")
        if path.endswith(".npz"):
            with np.load(path) as z:
                sd = {k: z[k] for k in z.files if k in need}
        else:
            import torch
            sd = torch.load(path, map_location="cpu", weights_only=True)
            sd = {k: v.detach().cpu().numpy() for k, v in sd.items() if k in need}
        found.update(sd)
    out = {}
    for name, shape in need.items():
        if name not in found:
            raise KeyError(f"LPIPS tensor {name!r} is in none of {paths}")
        a = np.asarray(found[name], np.float32)
        if name.startswith("lin") and a.shape == (1, shape[0], 1, 1):
            a = a.reshape(shape)
        if a.shape != shape:
            raise ValueError(f"LPIPS tensor {name!r} has shape {a.shape}, expected {shape}")
        out[name] = np.ascontiguousarray(a)
    return out


def _lpips_check_images(img1, img2):
    a, b = np.asarray(img1), np.asarray(img2)
    if a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError(f"LPIPS takes uint8 images, got {a.dtype} and {b.dtype}")
    if a.ndim != 3 or a.shape[2] != 3 or a.shape != b.shape:
        raise ValueError(f"LPIPS takes two (H, W, 3) images of equal size, got {a.shape} and {b.shape}")
    if a.shape[0] < LPIPS_MIN_SIDE or a.shape[1] < LPIPS_MIN_SIDE:
        raise ValueError(f"LPIPS needs at least {LPIPS_MIN_SIDE} pixels on each side, got {a.shape[0]} x {a.shape[1]}")
    return a, b


def lpips_features_host(img_u8, weights, dtype=None):
    """The five ReLU feature maps, each (C_l, H_l, W_l), of one uint8 RGB (H, W, 3) image, in torch CPU ops of ``dtype`` (default
    float32)."""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float32
    img, _ = _lpips_check_images(img_u8, img_u8)
    x = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).to(dtype) / 127.5 - 1
    x = (x - torch.tensor(LPIPS_SHIFT, dtype=dtype).view(3, 1, 1)) / torch.tensor(LPIPS_SCALE, dtype=dtype).view(3, 1, 1)
    x = x.unsqueeze(0)
    feats = []
    for key, _, _, _, stride, pad, pool in LPIPS_LAYERS:
        if pool:
            x = F.max_pool2d(x, 3, 2)
        w = torch.from_numpy(weights[key + ".weight"]).to(dtype)
        b = torch.from_numpy(weights[key + ".bias"]).to(dtype)
        x = F.relu(F.conv2d(x, w, b, stride=stride, padding=pad))
        feats.append(x[0])
    return feats


def lpips_from_features(f0, f1, weights):
    """The five per-layer distances of two feature lists, as a tensor of the features' dtype."""
    import torch
    out = []
    for l, (a, b) in enumerate(zip(f0, f1)):
        lin = torch.from_numpy(weights[f"lin{l}.model.1.weight"]).to(a.dtype).view(-1, 1, 1)
        na = a / (torch.sqrt(torch.sum(a * a, dim=0, keepdim=True)) + 1e-10)
        nb = b / (torch.sqrt(torch.sum(b * b, dim=0, keepdim=True)) + 1e-10)
        out.append(torch.sum(lin * (na - nb) ** 2, dim=0).mean())
    return torch.stack(out)


def calculate_lpips(img1_u8, img2_u8, weights, dtype=None, return_layers=False):
    """LPIPS-alex of two uint8 RGB (H, W, 3) images on the host; ``dtype=torch.float64`` is the tests' oracle.  With
    ``return_layers`` also the five per-layer distances."""
    a, b = _lpips_check_images(img1_u8, img2_u8)
    d = lpips_from_features(lpips_features_host(a, weights, dtype), lpips_features_host(b, weights, dtype), weights).double()
    score = float(d.sum())
    return (score, d.numpy()) if return_layers else score


class LpipsDevice:
    """The device object of csrc/lpips.hip.h: packed weights on one GPU.  ``forward`` scores (B, H, W, 3) uint8 CUDA batches."""

    def __init__(self, weights, device):
        import ctypes
        from . import lib
        self._lib = L = lib.load()
        self.device = device
        h = ctypes.c_void_p()
        lib.check(L.ucdir_lpips_create(device.index if device.index is not None else 0, ctypes.byref(h)))
        self._h = h
        for name, shape in lpips_weight_shapes().items():
            if name not in weights:
                raise KeyError(f"LPIPS tensor {name!r} is missing from the weights")
            a = np.ascontiguousarray(weights[name], np.float32)
            sh = (ctypes.c_int64 * a.ndim)(*a.shape)
            lib.check(L.ucdir_lpips_load_weight(h, name.encode(), a.ctypes.data, sh, a.ndim))
        lib.check(L.ucdir_lpips_finalize(h))
        self._ws = None

    def forward(self, a_u8, b_u8):
        """(scores (B), per_layer (B, 5)) float64 CUDA tensors; asynchronous on the current stream."""
        import torch
        from . import lib
        from .ucdir import _ptr, _stream_ptr
        for t in (a_u8, b_u8):
            if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.uint8:
                raise ValueError("LPIPS on the device takes uint8 tensors on the GPU")
            if t.dim() != 4 or t.shape[-1] != 3 or not t.is_contiguous():
                raise ValueError(f"LPIPS on the device takes contiguous (B, H, W, 3) images, got {tuple(t.shape)}")
        if a_u8.shape != b_u8.shape or a_u8.device != b_u8.device or a_u8.device != self.device:
            raise ValueError("LPIPS on the device takes two batches of equal shape on the object's device")
        B, H, W, _ = a_u8.shape
        nbytes = self._lib.ucdir_lpips_workspace_bytes(B, H, W)
        if nbytes < 0:
            raise ValueError(f"LPIPS needs at least {LPIPS_MIN_SIDE} pixels on each side, got {H} x {W} (batch {B})")
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)       # kept: debug_read reads the features out of it
        out = torch.empty(B * 6, dtype=torch.float64, device=self.device)
        lib.check(self._lib.ucdir_lpips_forward(self._h, _ptr(a_u8), _ptr(b_u8), B, H, W, _ptr(out), _ptr(out[B:]), _ptr(self._ws),
                                                _stream_ptr(self.device)))
        self._shape = (B, H, W)
        return out[:B], out[B:].view(B, 5)

    def debug_read(self, layer, which):
        """ReLU features of tap ``layer`` of the last forward's first (0) / second (1) input: (B, C, H_l, W_l) fp32 CUDA tensor."""
        import torch
        from . import lib
        from .ucdir import _ptr, _stream_ptr
        if self._ws is None:
            raise RuntimeError("LpipsDevice.debug_read: no forward has run")
        if layer not in range(5) or which not in (0, 1):
            raise ValueError(f"LpipsDevice.debug_read: layer must lie in 0..4 and which be 0 or 1, got {layer!r}, {which!r}")
        B, h, w = self._shape
        for _, _, _, k, stride, pad, pool in LPIPS_LAYERS[:layer + 1]:
            if pool:
                h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
            h, w = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        dst = torch.empty((B, LPIPS_LAYERS[layer][2], h, w), dtype=torch.float32, device=self.device)
        lib.check(self._lib.ucdir_lpips_debug_read(self._h, layer, which, _ptr(dst), dst.numel(), _stream_ptr(self.device)))
        return dst

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.ucdir_lpips_destroy(h)


def lpips_handle(weights, device):
    """The LpipsDevice of (this weights dict, this device), made on first use: packing and upload happen once per run."""
    key = (id(weights), device.index)
    hit = _lpips_handles.get(key)
    if hit is None or hit[0] is not weights:
        hit = (weights, LpipsDevice(weights, device))
        _lpips_handles[key] = hit
    return hit[1]


def lpips_u8_device(a_u8, b_u8, weights, return_layers=False):
    """LPIPS-alex of (B, H, W, 3) uint8 CUDA batches on the GPU: a list of floats, one per pair; one device-to-host copy."""
    scores, layers = lpips_handle(weights, a_u8.device).forward(a_u8, b_u8)
    host = scores.cpu().tolist()
    return (host, layers.cpu().numpy()) if return_layers else host


def lpips_device(x, y, weights, return_layers=False):
    """LPIPS-alex of the uint8 images tensor2img_u8_device makes of ``x`` and ``y``, fp32 (B, 3, H, W) or (3, H, W) CUDA tensors in
    [-1, 1], scored on the GPU (csrc/lpips.hip.h): the same uint8 images the JPEGs are written from.  A list of floats."""
    import torch
    for t in (x, y):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError("lpips_device takes tensors on the GPU")
        if t.dtype != torch.float32:
            raise ValueError(f"lpips_device takes fp32 images, got {t.dtype}")
    if x.dim() == 3:
        x, y = x.unsqueeze(0), y.unsqueeze(0)
    if x.dim() != 4 or x.shape[1] != 3 or x.shape != y.shape:
        raise ValueError(f"lpips_device takes two (B, 3, H, W) or (3, H, W) batches of equal shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.shape[2] < LPIPS_MIN_SIDE or x.shape[3] < LPIPS_MIN_SIDE:
        raise ValueError(f"LPIPS needs at least {LPIPS_MIN_SIDE} pixels on each side, got {x.shape[2]} x {x.shape[3]}")
    return lpips_u8_device(tensor2img_u8_batch_device(x), tensor2img_u8_batch_device(y), weights, return_layers)
