"""Paired-image loader for ``-p val`` (reference: data/LRHR_dataset.py:230-297 PairDataset, val split, datatype img):
sorted file lists of dataroot.lq / dataroot.gt, RGB, scaled to [-1, 1] (data/util.py:76-83), dict with 'HR', 'SR', 'LR',
'Index'; the JPEG-restoration loader ImagenetJPGDataset (reference: data/LRHR_dataset.py:446-516); and the 4x super-resolution
loader ImagenetSRDataset (reference: data/LRHR_dataset.py:385-443); and the real-world SR loader RealESRGANDataset (reference:
data/LRHR_dataset.py:668-807).  The three ImageNet loaders take ``decode_device``: "cpu" (the default) decodes the file with
Pillow on the host and uploads the pixels; "gpu" uploads the file's bytes and decodes them with csrc/jpeg_decode.hip.h, the same
pixels, falling back to Pillow per image for what that decoder does not take (``decode_fallbacks``); ``prefetch(indices)`` then
decodes a set of files through one batch call ahead of the items that use them."""
import os

import numpy as np
import torch

IMG_EXT = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")


def _listdir(d):
    return sorted(os.path.join(d, f) for f in os.listdir(d) if f.lower().endswith(IMG_EXT))


def _load(path):
    from PIL import Image
    a = np.asarray(Image.open(path).convert("RGB"), dtype=np.float32) / 255.0
    return torch.from_numpy(a.transpose(2, 0, 1)) * 2.0 - 1.0


class PairDataset:
    def __init__(self, data_args, phase="val"):
        root = data_args["dataroot"]
        self.sr_path = _listdir(root["lq"])
        self.hr_path = _listdir(root["gt"])
        if len(self.sr_path) != len(self.hr_path):
            raise ValueError("lq / gt directories hold a different number of images")
        n = data_args.get("data_len", -1) if hasattr(data_args, "get") else -1
        if n and n > 0:
            self.sr_path, self.hr_path = self.sr_path[:n], self.hr_path[:n]
        self.crop = data_args.get("crop_size", None) if phase == "val_crop" else None

    def __len__(self):
        return len(self.sr_path)

    def __getitem__(self, i):
        sr, hr = _load(self.sr_path[i]), _load(self.hr_path[i])
        return {"HR": hr, "SR": sr, "LR": sr, "Index": i}


# u8 -> [-1, 1] exactly as _load forms it (numpy fp32 u8 / 255, then * 2 - 1 in torch fp32), as a 256-entry table: a division by a
# scalar on the GPU multiplies by the reciprocal and can land one ulp away
_U8_TO_UNIT = torch.from_numpy(np.arange(256, dtype=np.float32) / 255.0) * 2.0 - 1.0
_unit_tables = {}


def _check_decode_device(v):
    if v not in ("cpu", "gpu"):
        raise ValueError("decode_device must be 'cpu' or 'gpu', got %r" % (v,))
    return v


def _region_of(data, region):
    """The (left, top, width, height) crop ``region`` takes of the JPEG file ``data``, or None for the whole image.  Raises
    JpegUnsupported for a file the decoder does not take and for an empty crop."""
    from .metrics import JpegUnsupported, jpeg_info
    info = jpeg_info(data)
    crop = region(info["width"], info["height"])
    if crop is not None and (crop[2] < 1 or crop[3] < 1):
        raise JpegUnsupported(0, "the loader's crop of this image is empty")
    return crop


def decode_u8_device(ds, i, region, dev):
    """The ``decode_device = "gpu"`` half of the ImageNet loaders: read the bytes of image ``i`` of loader ``ds`` and decode them on
    ``dev`` (csrc/jpeg_decode.hip.h, byte for byte Pillow's convert("RGB")).  ``region(w, h)`` -> None for the whole image or the
    (left, top, width, height) crop the loader takes of a w x h image.  Returns (uint8 CUDA tensor, whether it is already cropped),
    or None for a file the decoder does not take (not a JPEG, progressive, CMYK, damaged, ...): the loader then decodes that image
    with Pillow, and ``ds.decode_fallbacks`` gains (index, reason).  An image that ``prefetch`` decoded is taken from there, once."""
    from .metrics import JpegUnsupported, jpeg_decode_device
    try:
        got = ds.prefetched.pop(i, None)                 # what prefetch left: (tensor, cropped) or the decoder's refusal
        if isinstance(got, JpegUnsupported):
            raise got
        if got is not None and got[0].device == dev:
            return got
        with open(ds.hr_path[i], "rb") as f:
            data = f.read()
        crop = _region_of(data, region)
        return jpeg_decode_device(data, crop=crop, device=dev), crop is not None
    except JpegUnsupported as e:
        ds.decode_fallbacks.append((i, e.reason))
        return None


def prefetch_u8_device(ds, indices, region, dev=None):
    """The ``prefetch`` of the ImageNet loaders: with ``decode_device = "gpu"``, read the files of ``indices``, take each one's
    ``region`` crop from its info and decode the whole set through ONE metrics.jpeg_decode_batch_device call on ``dev`` (default:
    the current GPU).  The results wait in ``ds.prefetched`` until decode_u8_device asks for that index, which hands each out
    once; a file the decoder refused waits there as its JpegUnsupported and takes the Pillow fallback then, so that
    ``decode_fallbacks`` fills as it does without prefetch.  With "cpu" nothing happens."""
    from .metrics import JpegUnsupported, jpeg_decode_batch_device
    if ds.decode_device != "gpu":
        return
    dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)
    idx, datas, crops = [], [], []
    for i in dict.fromkeys(int(i) for i in indices):
        with open(ds.hr_path[i], "rb") as f:
            data = f.read()
        try:
            crop = _region_of(data, region)
        except JpegUnsupported as e:
            ds.prefetched[i] = e
            continue
        idx.append(i)
        datas.append(data)
        crops.append(crop)
    for i, crop, got in zip(idx, crops, jpeg_decode_batch_device(datas, crops, device=dev)):
        ds.prefetched[i] = got if isinstance(got, JpegUnsupported) else (got, crop is not None)


def _u8_to_unit(x):
    """(H, W, 3) uint8 on a device -> (3, H, W) fp32 in [-1, 1] on that device."""
    lut = _unit_tables.get(x.device)
    if lut is None:
        lut = _unit_tables[x.device] = _U8_TO_UNIT.to(x.device)
    return lut[x.long()].permute(2, 0, 1).contiguous()


_U8_TO_01 = torch.from_numpy(np.arange(256, dtype=np.float32) / 255.0)
_01_tables = {}


def _u8_to_01(x):
    """(H, W, 3) uint8 on a device -> (3, H, W) fp32 in [0, 1] there, u8 / 255 as numpy float32 forms it on the host (a table, for the
    reason _U8_TO_UNIT is one)."""
    lut = _01_tables.get(x.device)
    if lut is None:
        lut = _01_tables[x.device] = _U8_TO_01.to(x.device)
    return lut[x.long()].permute(2, 0, 1).contiguous()


class ImagenetJPGDataset:
    """JPEG-restoration val loader (reference: data/LRHR_dataset.py:446-516, ImagenetJPGDataset): file names from the first field
    of each line of dataroot.txt under dataroot.root; HR = a centered crop of the RGB image; SR = HR after a JPEG round trip at
    quality factor ``factor``, computed on the current GPU (csrc/jpeg_roundtrip.hip.h) with the reference's cv2 channel order.

    The quality factor is ``factor[0]`` when both ends agree (the ``jpg-`` val setting, [10, 10]); otherwise it is drawn from a
    generator seeded by the image index, not from numpy's global RNG as the reference does, so an image's degradation does not
    depend on rank, batch or order."""

    def __init__(self, data_args, phase="val", decode_device="cpu"):
        root = data_args["dataroot"]
        self.root = root["root"]
        with open(root["txt"]) as f:
            names = [ln.split()[0] for ln in f if ln.strip()]
        n = data_args.get("data_len", -1)
        if n and n > 0:
            names = names[:n]
        self.hr_path = [os.path.join(self.root, s) for s in names]
        self.sr_path = self.hr_path                  # sr.py names its outputs after sr_path
        self.crop_size = data_args.get("crop_size") or 0
        self.factor = list(data_args.get("factor") or [5, 5])
        self.decode_device = _check_decode_device(decode_device)
        self.decode_fallbacks = []                   # (index, reason) of every image "gpu" had to leave to Pillow
        self.prefetched = {}                         # index -> what prefetch decoded and no item has asked for yet

    def __len__(self):
        return len(self.hr_path)

    def load_u8(self, i):
        """Host half: decode to RGB and crop -> (H, W, 3) uint8, contiguous.  The reference names PIL's (width, height) h, w; the
        crop below is the one it takes."""
        from PIL import Image
        img = Image.open(self.hr_path[i]).convert("RGB")
        cs = self.crop_size
        if min(img.size) < cs:
            img = img.resize((cs, cs))
        w, h = img.size
        cw, ch = (cs, cs) if cs > 0 else (w // 16 * 16, h // 16 * 16)
        left, top = (w - cw) // 2, (h - ch) // 2
        img = img.crop((left, top, left + cw, top + ch))
        return np.array(img, dtype=np.uint8)             # a writable copy (torch.from_numpy of PIL's read-only view warns)

    def region(self, w, h):
        """The crop the decoder takes of a w x h image: load_u8's centred crop, or None (the whole image) below crop_size."""
        cs = self.crop_size
        if min(w, h) < cs:
            return None
        cw, ch = (cs, cs) if cs > 0 else (w // 16 * 16, h // 16 * 16)
        return (w - cw) // 2, (h - ch) // 2, cw, ch

    def prefetch(self, indices, dev=None):
        """Decode the files of ``indices`` in one batch call ahead of their items (prefetch_u8_device)."""
        prefetch_u8_device(self, indices, self.region, dev)

    def load_u8_device(self, i, dev):
        """load_u8 with the decode on the GPU -> the same (H, W, 3) uint8 image as a tensor on ``dev``.  The centred crop is taken
        inside the decoder; an image below crop_size is decoded whole and resized there first (Pillow's resize default, bicubic)."""
        from .metrics import resample_device
        cs = self.crop_size
        got = decode_u8_device(self, i, self.region, dev)
        if got is None:
            return torch.from_numpy(self.load_u8(i)).to(dev)
        img, cropped = got
        return img if cropped else resample_device(img, (cs, cs), "bicubic")       # the crop of a cs x cs image is all of it

    def quality(self, i):
        lo, hi = int(self.factor[0]), int(self.factor[1])
        if lo == hi:
            return lo
        return int(np.random.RandomState(i).randint(lo, hi + 1))

    def __getitem__(self, i):
        from .metrics import jpeg_roundtrip_device
        dev = torch.device("cuda", torch.cuda.current_device())
        hr_u8 = self.load_u8_device(i, dev) if self.decode_device == "gpu" else torch.from_numpy(self.load_u8(i)).to(dev)
        sr_u8 = jpeg_roundtrip_device(hr_u8, self.quality(i), bgr=True)
        sr = _u8_to_unit(sr_u8)
        return {"HR": _u8_to_unit(hr_u8), "SR": sr, "LR": sr, "Index": i}


def sr_geometry(w, h, size=256):
    """Host-only geometry of the SR loader for a (w, h) image -> (pre, (left, top, s)).  ``pre`` is None or the (w, h) the image is
    resized to first: when its shorter side is below ``size`` that side becomes ``size`` and the longer int(size * long / short)
    (torchvision's resize to an int).  Then the centered square crop of side s = min(w, h), placed with Python's round as
    torchvision's center_crop places it (a .5 goes to the even neighbour)."""
    pre = None
    if min(w, h) < size:
        pre = (size, int(size * h / w)) if w <= h else (int(size * w / h), size)
        w, h = pre
    s = min(w, h)
    return pre, (int(round((w - s) / 2.0)), int(round((h - s) / 2.0)), s)


class ImagenetSRDataset:
    """4x super-resolution val loader (reference: data/LRHR_dataset.py:385-443, ImagenetSRDataset): file names from the first field
    of each line of dataroot.txt under dataroot.root.  The image is decoded on the host and uploaded once; HR = the centered square
    crop resized to 256^2, LR64 = HR resized to 64^2, SR = LR64 resized back to 256^2, all bicubic and all computed on the current
    GPU with Pillow's arithmetic (csrc/resample.hip.h), so HR and SR equal the reference's PIL images byte for byte.  The 64^2
    image of the last item stays reachable as ``last_lr64``."""
    sizes = (64, 256)

    def __init__(self, data_args, phase="val", decode_device="cpu"):
        root = data_args["dataroot"]
        self.root = root["root"]
        with open(root["txt"]) as f:
            names = [ln.split()[0] for ln in f if ln.strip()]
        n = data_args.get("data_len", -1)
        if n and n > 0:
            names = names[:n]
        self.hr_path = [os.path.join(self.root, s) for s in names]
        self.sr_path = self.hr_path                  # sr.py names its outputs after sr_path
        self.last_lr64 = None
        self.decode_device = _check_decode_device(decode_device)
        self.decode_fallbacks = []                   # (index, reason) of every image "gpu" had to leave to Pillow
        self.prefetched = {}                         # index -> what prefetch decoded and no item has asked for yet

    def __len__(self):
        return len(self.hr_path)

    def load_u8(self, i):
        """Host half: decode to RGB -> (H, W, 3) uint8, contiguous; every resize and the crop happen on the device."""
        from PIL import Image
        return np.array(Image.open(self.hr_path[i]).convert("RGB"), dtype=np.uint8)

    def degrade_u8(self, img_u8):
        """Device half on an uploaded (H, W, 3) uint8 image -> (HR 256^2, LR 64^2, SR 256^2), uint8."""
        from .metrics import resample_device
        lo, hi = self.sizes
        pre, (left, top, s) = sr_geometry(img_u8.shape[1], img_u8.shape[0], hi)
        if pre is not None:
            img_u8 = resample_device(img_u8, (pre[1], pre[0]), "bicubic")
        crop = img_u8[top:top + s, left:left + s].contiguous()
        hr = resample_device(crop, (hi, hi), "bicubic")
        lr64 = resample_device(hr, (lo, lo), "bicubic")
        return hr, lr64, resample_device(lr64, (hi, hi), "bicubic")

    def load_u8_device(self, i, dev):
        """load_u8 with the decode on the GPU: the whole image, as degrade_u8 takes it."""
        got = decode_u8_device(self, i, self.region, dev)
        return torch.from_numpy(self.load_u8(i)).to(dev) if got is None else got[0]

    def region(self, w, h):
        """The decoder takes the whole image."""
        return None

    def prefetch(self, indices, dev=None):
        """Decode the files of ``indices`` in one batch call ahead of their items (prefetch_u8_device)."""
        prefetch_u8_device(self, indices, self.region, dev)

    def __getitem__(self, i):
        dev = torch.device("cuda", torch.cuda.current_device())
        img = self.load_u8_device(i, dev) if self.decode_device == "gpu" else torch.from_numpy(self.load_u8(i)).to(dev)
        hr_u8, self.last_lr64, sr_u8 = self.degrade_u8(img)
        sr = _u8_to_unit(sr_u8)
        return {"HR": _u8_to_unit(hr_u8), "SR": sr, "LR": sr, "Index": i}


def reflect101_pad(img, size):
    """Pad an (H, W, 3) array bottom and right up to ``size`` like cv2.copyMakeBorder(..., BORDER_REFLECT_101): the mirror does not
    repeat the edge and starts over when the image is shorter than the pad."""
    return img[reflect101_index(img.shape[0], size)][:, reflect101_index(img.shape[1], size)]


def reflect101_index(n, size):
    """Source index of every row (column) of an axis of n samples padded at its end up to ``size`` by reflect101_pad's rule."""
    if n >= size:
        return np.arange(n)
    if n == 1:
        return np.zeros(size, dtype=np.int64)
    i = np.arange(size) % (2 * n - 2)
    return np.where(i < n, i, 2 * n - 2 - i)


class RealESRGANDataset:
    """Real-world SR val loader (reference: data/LRHR_dataset.py:668-807, RealESRGANDataset): file names from the first field of each
    line of dataroot.txt under dataroot.root.  ``gt`` = the centred ``crop_size`` crop of the RGB image in [0, 1] (smaller images
    are padded bottom and right first), decoded on the host and uploaded once; ``lq`` = gt after the second-order degradation
    (degradations.realsr_degrade_device) at crop_size / scale, computed on the current GPU.

    The reference's val split returns no ``lq`` and draws from global generators; here every random decision of image ``i`` comes
    from a stream seeded by ``i`` (degradations.draw_realsr_params), so an image's input does not depend on rank, batch or
    order.  ``data_args.dopt`` / ``data_args.param``: the degradation and kernel settings, a name from
    config/realsr_degradations.yaml or a dict."""

    def __init__(self, data_args, phase="val", decode_device="cpu"):
        from .degradations import load_settings
        root = data_args["dataroot"]
        if "root" not in root or "txt" not in root:
            raise ValueError("RealESRGANDataset reads dataroot.root and dataroot.txt (an image directory and a list of names), got "
                             "dataroot keys %s" % sorted(root))
        self.root = root["root"]
        with open(root["txt"]) as f:
            names = [ln.split()[0] for ln in f if ln.strip()]
        n = data_args.get("data_len", -1)
        if n and n > 0:
            names = names[:n]
        self.hr_path = [os.path.join(self.root, s) for s in names]
        self.sr_path = self.hr_path                  # sr.py names its outputs after sr_path
        self.crop_size = int(data_args.get("crop_size") or 256)
        if self.crop_size < 32 or self.crop_size % 4:
            raise ValueError("RealESRGANDataset: crop_size must be a multiple of 4 and at least 32, got %d" % self.crop_size)
        self.dopt = load_settings(data_args.get("dopt") or "dopt")
        self.kopt = load_settings(data_args.get("param") or "param")
        self.decode_device = _check_decode_device(decode_device)
        self.decode_fallbacks = []                   # (index, reason) of every image "gpu" had to leave to Pillow
        self.prefetched = {}                         # index -> what prefetch decoded and no item has asked for yet

    def __len__(self):
        return len(self.hr_path)

    def load_u8(self, i):
        """Host half: decode to RGB, pad to crop_size, centred crop -> (crop_size, crop_size, 3) uint8, contiguous."""
        from PIL import Image
        img = reflect101_pad(np.asarray(Image.open(self.hr_path[i]).convert("RGB"), dtype=np.uint8), self.crop_size)
        cs = self.crop_size
        top, left = (img.shape[0] - cs) // 2, (img.shape[1] - cs) // 2
        return np.ascontiguousarray(img[top:top + cs, left:left + cs])

    def region(self, w, h):
        """The crop the decoder takes of a w x h image: the centred one where the image covers it, else None (the whole image)."""
        cs = self.crop_size
        return ((w - cs) // 2, (h - cs) // 2, cs, cs) if w >= cs and h >= cs else None

    def prefetch(self, indices, dev=None):
        """Decode the files of ``indices`` in one batch call ahead of their items (prefetch_u8_device)."""
        prefetch_u8_device(self, indices, self.region, dev)

    def load_u8_device(self, i, dev):
        """load_u8 with the decode on the GPU -> the same (crop_size, crop_size, 3) uint8 image as a tensor on ``dev``.  An image
        that covers the crop is cropped inside the decoder; a smaller one is decoded whole, then padded and cropped there by
        gathering the rows and columns reflect101_index names."""
        cs = self.crop_size
        got = decode_u8_device(self, i, self.region, dev)
        if got is None:
            return torch.from_numpy(self.load_u8(i)).to(dev)
        img, cropped = got
        if cropped:
            return img
        rows, cols = reflect101_index(img.shape[0], cs), reflect101_index(img.shape[1], cs)
        top, left = (len(rows) - cs) // 2, (len(cols) - cs) // 2
        rows, cols = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (rows[top:top + cs], cols[left:left + cs]))
        return img.index_select(0, rows).index_select(1, cols).contiguous()

    def __getitem__(self, i):
        from .degradations import draw_realsr_params, realsr_degrade_device
        dev = torch.device("cuda", torch.cuda.current_device())
        if self.decode_device == "gpu":
            gt = _u8_to_01(self.load_u8_device(i, dev))
            lq = realsr_degrade_device(gt.unsqueeze(0), draw_realsr_params(i, self.dopt, self.kopt), self.dopt)[0]
            return {"gt": gt, "lq": lq, "Index": i}
        # u8 / 255 in numpy float32 on the host, as the reference forms it (a division by a scalar on the GPU can land one ulp away)
        gt = torch.from_numpy(np.ascontiguousarray((self.load_u8(i).astype(np.float32) / 255.0).transpose(2, 0, 1))).to(dev)
        lq = realsr_degrade_device(gt.unsqueeze(0), draw_realsr_params(i, self.dopt, self.kopt), self.dopt)[0]
        return {"gt": gt, "lq": lq, "Index": i}
