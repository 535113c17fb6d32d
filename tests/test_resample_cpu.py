"""Pillow-exact 8-bit resampling of the 4x super-resolution val task, host side (csrc/resample.hip.h): a numpy
model of Pillow's Resample.c (fixed-point coefficient tables, horizontal pass into a uint8 intermediate, vertical pass) equals
PIL.Image.resize byte for byte over four filters, nine geometries and three kinds of content, and over the loader's whole crop ->
256 -> 64 -> 256 chain; the library's host-only coefficient function returns the model's tables; the C ABI surface and its argument
checks; the ImagenetSRDataset listing and geometry; the dataset selection of sr.py and config/sr.yaml.  No GPU needed."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from ucdir_amd import lib
from ucdir_amd.data import ImagenetSRDataset, PairDataset, sr_geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = ("box", "bilinear", "bicubic", "lanczos")
FILTER_ID = {"box": 0, "bilinear": 1, "bicubic": 2, "lanczos": 3}
SUPPORT = {"box": 0.5, "bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}
# (W, H) -> (W', H')
GEOMETRIES = (((256, 256), (64, 64)), ((64, 64), (256, 256)), ((375, 375), (256, 256)), ((500, 375), (341, 256)),
              ((333, 500), (256, 384)), ((100, 80), (320, 256)), ((17, 33), (256, 256)), ((256, 256), (256, 64)),
              ((1000, 1000), (256, 256)))
CONTENTS = ("noise", "bw", "gradient")
PRECISION_BITS = 22


def pil_filter(name):
    from PIL import Image
    return {"box": Image.BOX, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[name]


def pil_resize(img, size_hw, filt):
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((size_hw[1], size_hw[0]), pil_filter(filt)))


def make_content(kind, H, W, seed=0):
    rng = np.random.RandomState(1000 * seed + H * 7 + W)
    if kind == "noise":
        return rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    if kind == "bw":                                   # saturated blocks and single pixels: the overshoot of the negative lobes clips
        img = (rng.randint(0, 2, (-(-H // 3), -(-W // 5), 3)) * 255).astype(np.uint8)
        img = np.repeat(np.repeat(img, 3, 0), 5, 1)[:H, :W].copy()
        img[::7, ::11] = 255 - img[::7, ::11]
        return img
    if kind == "gradient":
        y, x = np.mgrid[0:H, 0:W]
        return np.stack([(x * 255 // max(W - 1, 1)), (y * 255 // max(H - 1, 1)), ((x + y + seed) % 256)], -1).astype(np.uint8)
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------------------------
# the numpy model of Pillow's Resample.c, 8 bits per channel
# ---------------------------------------------------------------------------------------------------------------------
def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def filter_value(filt, x):
    if filt == "box":
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if filt == "lanczos":
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    x = abs(x)
    if filt == "bilinear":
        return 1.0 - x if x < 1.0 else 0.0
    a = -0.5
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def model_coeffs(n_in, n_out, filt):
    """-> kk (n_out, ksize) int32, bounds (n_out, 2) int32 as (xmin, xmax), ksize."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[filt] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((n_out, ksize), np.int32)
    bounds = np.zeros((n_out, 2), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [filter_value(filt, (x + xmin - center + 0.5) / fs) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return kk, bounds, ksize


def _one_pass(img, n_out, filt, axis):
    kk, bounds, _ = model_coeffs(img.shape[axis], n_out, filt)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.int64)
    for xx in range(n_out):
        x0, n = bounds[xx]
        acc = np.tensordot(kk[xx, :n].astype(np.int64), src[x0:x0 + n], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max() < 2 ** 31          # the int32 sum of the kernel does not wrap
        out[xx] = acc >> PRECISION_BITS
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


def resample_model(img, size_hw, filt):
    H, W = size_hw
    if W != img.shape[1]:
        img = _one_pass(img, W, filt, 1)
    if H != img.shape[0]:
        img = _one_pass(img, H, filt, 0)
    return img.copy()


def pil_sr_chain(img):
    """The reference loader's PIL chain on an RGB array -> (HR 256^2, LR 64^2, SR 256^2), with torchvision's resize-to-int and
    center_crop rules restated on PIL alone."""
    from PIL import Image
    im = Image.fromarray(img)
    w, h = im.size
    if min(w, h) < 256:
        im = im.resize((256, int(256 * h / w)) if w <= h else (int(256 * w / h), 256), Image.BICUBIC)
    w, h = im.size
    s = min(w, h)
    top, left = int(round((h - s) / 2.0)), int(round((w - s) / 2.0))
    im = im.crop((left, top, left + s, top + s))
    hr = im.resize((256, 256), Image.BICUBIC)
    lr = hr.resize((64, 64), Image.BICUBIC)
    sr = lr.resize((256, 256), Image.BICUBIC)
    return np.asarray(hr), np.asarray(lr), np.asarray(sr)


@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: "%dx%d-%dx%d" % (g[0] + g[1]))
@pytest.mark.parametrize("filt", FILTERS)
def test_model_equals_pillow(filt, geom):
    (W, H), (Wo, Ho) = geom
    for kind in CONTENTS:
        img = make_content(kind, H, W)
        got, ref = resample_model(img, (Ho, Wo), filt), pil_resize(img, (Ho, Wo), filt)
        bad = np.argwhere(got != ref)
        assert got.shape == ref.shape and bad.size == 0, (kind, len(bad), bad[:3].tolist())


def test_model_chain_equals_pillow():
    for kind in CONTENTS:
        img = make_content(kind, 375, 500)
        hr, lr, sr = pil_sr_chain(img)
        crop = img[:, 62:437]                       # (500 - 375) / 2 = 62.5 -> 62
        m_hr = resample_model(crop, (256, 256), "bicubic")
        m_lr = resample_model(m_hr, (64, 64), "bicubic")
        m_sr = resample_model(m_lr, (256, 256), "bicubic")
        assert np.array_equal(m_hr, hr) and np.array_equal(m_lr, lr) and np.array_equal(m_sr, sr), kind


def test_identity_resize_copies():
    img = make_content("noise", 20, 30)
    assert np.array_equal(resample_model(img, (20, 30), "bicubic"), img)
    assert np.array_equal(pil_resize(img, (20, 30), "bicubic"), img)


# ---------------------------------------------------------------------------------------------------------------------
# the library's coefficient tables (host only)
# ---------------------------------------------------------------------------------------------------------------------
def lib_coeffs(n_in, n_out, filt):
    L = lib.load()
    ks = ctypes.c_int32(0)
    assert L.ucdir_resample_coeffs(n_in, n_out, FILTER_ID[filt], None, None, ctypes.byref(ks)) == 0, L.ucdir_last_error()
    kk = np.full((n_out, ks.value), -7, np.int32)
    bounds = np.full((n_out, 2), -7, np.int32)
    ks2 = ctypes.c_int32(0)
    assert L.ucdir_resample_coeffs(n_in, n_out, FILTER_ID[filt], kk.ctypes.data, bounds.ctypes.data, ctypes.byref(ks2)) == 0
    assert ks2.value == ks.value
    return kk, bounds, ks.value


def axis_pairs():
    pairs = {(1, 7), (7, 1), (4096, 256)}
    for (W, H), (Wo, Ho) in GEOMETRIES:
        pairs.add((W, Wo))
        pairs.add((H, Ho))
    return sorted(pairs)


@pytest.mark.parametrize("filt", FILTERS)
def test_library_tables_equal_the_model(filt):
    for n_in, n_out in axis_pairs():
        kk, bounds, ks = lib_coeffs(n_in, n_out, filt)
        m_kk, m_bounds, m_ks = model_coeffs(n_in, n_out, filt)
        assert ks == m_ks, (n_in, n_out)
        assert np.array_equal(bounds, m_bounds), (n_in, n_out)
        bad = np.argwhere(kk != m_kk)
        assert bad.size == 0, (n_in, n_out, len(bad), bad[:3].tolist())


def test_coeff_rows_sum_to_one():
    """Every row of a table sums to 2^22 within the rounding of its taps, so a constant image stays constant."""
    for filt in FILTERS:
        kk, bounds, ks = lib_coeffs(375, 256, filt)
        assert np.abs(kk.sum(1) - (1 << PRECISION_BITS)).max() <= ks
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= 375).all() and (bounds[:, 1] <= ks).all()


# ---------------------------------------------------------------------------------------------------------------------
# C ABI surface (no device needed: the argument checks come first)
# ---------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_checks_arguments():
    L = lib.load()
    assert lib.ABI_VERSION == L.ucdir_abi_version() == 5
    sigs = {"ucdir_resample_coeffs": 6, "ucdir_resample_workspace_bytes": 5, "ucdir_resample": 10}
    for name, nargs in sigs.items():
        assert name in lib.EXPORTED and len(lib._SIGS[name][1]) == nargs
    assert lib._SIGS["ucdir_resample_workspace_bytes"][0] is ctypes.c_int64
    header = open(os.path.join(ROOT, "include", "ucdir_hip.h")).read()
    assert all(name + "(" in header for name in sigs) and "#define UCDIR_ABI_VERSION 5" in header
    # tables sized for Lanczos (support 3): out * (ksize + 2) int32 per changing axis, rounded up to 16 bytes, then the
    # (B, Hin, Wout, 3) intermediate when both axes change
    # 256^2 -> 64^2: ksize = ceil(3 * 4) * 2 + 1 = 25 on both axes -> 2 * 64 * 27 ints; intermediate 16 * 256 * 64 * 3
    assert L.ucdir_resample_workspace_bytes(16, 256, 256, 64, 64) == 2 * 64 * 27 * 4 + 16 * 256 * 64 * 3
    # 375 x 500 (H x W) -> 375 x 341: only the horizontal axis, ksize = ceil(3 * 500 / 341) * 2 + 1 = 11 -> 341 * 13 ints = 17732
    # bytes -> 17744 after rounding; no intermediate
    assert L.ucdir_resample_workspace_bytes(1, 375, 500, 375, 341) == 17744
    assert L.ucdir_resample_workspace_bytes(2, 64, 64, 64, 64) == 16           # a copy needs no workspace; never empty
    for bad in ((0, 64, 64, 32, 32), (1, 0, 64, 32, 32), (1, 64, 64, 32, 0), (1, 64, -3, 32, 32), (1, 70000, 64, 64, 64)):
        assert L.ucdir_resample_workspace_bytes(*bad) == -1, bad
    a, b, c = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(16384)          # never dereferenced
    for args in ((None, b, c), (a, None, c), (a, b, None)):
        rc = L.ucdir_resample(args[0], args[1], 1, 64, 64, 32, 32, 2, args[2], None)
        assert rc != 0 and b"null argument" in L.ucdir_last_error()
    for shape in ((0, 64, 64, 32, 32), (1, 64, 0, 32, 32), (1, 64, 64, 0, 32)):
        rc = L.ucdir_resample(a, b, *shape, 2, c, None)
        assert rc != 0 and b"at least 1" in L.ucdir_last_error()
    rc = L.ucdir_resample(a, b, 1, 64, 64, 32, 32, 9, c, None)
    assert rc != 0 and b"unknown filter" in L.ucdir_last_error()
    rc = L.ucdir_resample(a, b, 1, 64, 64, 32, 32, -1, c, None)
    assert rc != 0 and b"unknown filter" in L.ucdir_last_error()
    # bicubic at 64:1 spans ceil(2 * 64) * 2 + 1 = 257 taps, above the cap of 129
    rc = L.ucdir_resample(a, b, 1, 64, 4096, 64, 64, 2, c, None)
    assert rc != 0 and b"ksize cap" in L.ucdir_last_error()
    ks = ctypes.c_int32(0)
    assert L.ucdir_resample_coeffs(0, 4, 2, None, None, ctypes.byref(ks)) != 0 and b"at least 1" in L.ucdir_last_error()
    assert L.ucdir_resample_coeffs(4, 4, 7, None, None, ctypes.byref(ks)) != 0 and b"unknown filter" in L.ucdir_last_error()
    assert L.ucdir_resample_coeffs(4, 4, 2, None, None, None) != 0 and b"null argument" in L.ucdir_last_error()


def test_the_cap_admits_sixteen_to_one():
    L = lib.load()
    for filt in FILTERS:
        ks = ctypes.c_int32(0)
        assert L.ucdir_resample_coeffs(4096, 256, FILTER_ID[filt], None, None, ctypes.byref(ks)) == 0
        assert ks.value == int(math.ceil(SUPPORT[filt] * 16)) * 2 + 1 <= 129
    assert L.ucdir_resample_workspace_bytes(1, 4096, 4096, 256, 256) > 0


def test_resample_device_refuses_host_tensors():
    from ucdir_amd.metrics import resample_device
    with pytest.raises(ValueError, match="GPU"):
        resample_device(torch.zeros(32, 32, 3, dtype=torch.uint8), (16, 16))


# ---------------------------------------------------------------------------------------------------------------------
# loader, host half
# ---------------------------------------------------------------------------------------------------------------------
def write_tree(tmp_path, sizes, fmt="PNG"):
    """ImageNet-style tree: images of the given (H, W) under images/val, a list file with a label field."""
    from PIL import Image
    d = tmp_path / "images" / "val"
    os.makedirs(d)
    lines = []
    for k, (h, w) in enumerate(sizes):
        name = f"ILSVRC2012_val_{k:08d}.JPEG"
        Image.fromarray(make_content("gradient" if k % 2 else "noise", h, w, seed=k)).save(d / name, fmt)
        lines.append(f"{name} {k}\n" if k % 2 == 0 else f"{name}\t{k}\n")
    txt = tmp_path / "list.txt"
    txt.write_text("".join(lines) + "\n")
    return {"root": str(d), "txt": str(txt)}


def test_loader_lists_files_and_honours_data_len(tmp_path):
    from PIL import Image
    root = write_tree(tmp_path, [(40, 50), (37, 70), (64, 64)])
    ds = ImagenetSRDataset({"dataroot": root, "data_len": -1})
    assert len(ds) == 3 and ds.sr_path == ds.hr_path and tuple(ds.sizes) == (64, 256)
    assert [os.path.basename(p) for p in ds.hr_path] == [f"ILSVRC2012_val_{k:08d}.JPEG" for k in range(3)]
    assert all(os.path.isfile(p) for p in ds.hr_path)
    assert len(ImagenetSRDataset({"dataroot": root, "data_len": 2})) == 2
    assert len(ImagenetSRDataset({"dataroot": root, "data_len": 9})) == 3
    assert len(ImagenetSRDataset({"dataroot": root})) == 3
    u8 = ds.load_u8(1)                                  # the host half decodes and does nothing else
    assert u8.dtype == np.uint8 and u8.flags.c_contiguous and u8.flags.writeable
    assert np.array_equal(u8, np.asarray(Image.open(ds.hr_path[1]).convert("RGB")))


def _pil_geometry(w, h):
    """torchvision's resize-to-int and center_crop rules on a blank PIL image -> (pre-resize target or None, crop box)."""
    pre = None
    if min(w, h) < 256:
        pre = (256, int(256 * h / w)) if w <= h else (int(256 * w / h), 256)
        w, h = pre
    s = min(w, h)
    return pre, (int(round((w - s) / 2.0)), int(round((h - s) / 2.0)), s)


@pytest.mark.parametrize("w,h", [(500, 375), (375, 500), (256, 256), (180, 200), (200, 90), (257, 256), (301, 256), (256, 301)])
def test_geometry_helper(w, h):
    pre, (left, top, s) = sr_geometry(w, h)
    assert (pre, (left, top, s)) == _pil_geometry(w, h)
    pw, ph = pre or (w, h)
    assert s == min(pw, ph) >= 256 and 0 <= left <= pw - s and 0 <= top <= ph - s
    assert (pre is None) == (min(w, h) >= 256)


def test_geometry_helper_hand_cases():
    assert sr_geometry(500, 375) == (None, (62, 0, 375))            # 62.5 rounds to even
    assert sr_geometry(375, 500) == (None, (0, 62, 375))
    assert sr_geometry(301, 256) == (None, (22, 0, 256))            # (301 - 256) / 2 = 22.5 -> 22
    assert sr_geometry(303, 256) == (None, (24, 0, 256))            # 23.5 -> 24
    assert sr_geometry(256, 256) == (None, (0, 0, 256))
    assert sr_geometry(180, 200) == ((256, 284), (0, 14, 256))      # int(256 * 200 / 180) = 284
    assert sr_geometry(200, 90) == ((568, 256), (156, 0, 256))      # int(256 * 200 / 90) = 568


# ---------------------------------------------------------------------------------------------------------------------
# sr.py: dataset selection and config/sr.yaml
# ---------------------------------------------------------------------------------------------------------------------
def _sr_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sr_entry_resample", os.path.join(ROOT, "sr.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_sr_selects_the_sr_dataset_class(tmp_path):
    sr = _sr_module()
    root = write_tree(tmp_path, [(32, 48)])
    ds = sr.make_val_dataset({"datasetname": "ImagenetSRDataset", "data_args": {"dataroot": root, "data_len": 5000}})
    assert type(ds) is ImagenetSRDataset and len(ds) == 1
    for d in ("lq", "gt"):
        os.makedirs(tmp_path / d)
    pair_args = {"dataroot": {"lq": str(tmp_path / "lq"), "gt": str(tmp_path / "gt")}}
    assert type(sr.make_val_dataset({"data_args": pair_args})) is PairDataset
    with pytest.raises(ValueError, match="RealESRGANDataset"):
        sr.make_val_dataset({"datasetname": "RealESRGANDataset", "data_args": pair_args})


def test_sr_config_parses_to_the_sr_loader(tmp_path, monkeypatch):
    import argparse

    import yaml
    from ucdir_amd import config as Config
    path = os.path.join(ROOT, "config", "sr.yaml")
    cfg = yaml.safe_load(open(path))
    assert "sr-" in cfg["name"] and cfg["datasets"]["val"]["datasetname"] == "ImagenetSRDataset"
    assert set(cfg["datasets"]["val"]["data_args"]["dataroot"]) == {"root", "txt"}
    assert cfg["model"]["unet"] == yaml.safe_load(open(os.path.join(ROOT, "config", "jpg.yaml")))["model"]["unet"]
    monkeypatch.chdir(tmp_path)
    opt = Config.parse(argparse.Namespace(config=path, phase="val", checkpoint=None), make_dirs=False)
    assert opt["datasets"]["val"]["datasetname"] == "ImagenetSRDataset"
    da = opt["datasets"]["val"]["data_args"]
    assert da["data_len"] == 5000 and da["split"] == "val"
    assert da["dataroot"] == cfg["datasets"]["val"]["data_args"]["dataroot"]
    sched = opt["model"]["beta_schedule"]["val"]
    assert sched == cfg["model"]["beta_schedule"]["val"]           # no override for `sr-` names: the written schedule holds
    assert sched["n_timestep"] == 50 and sched["linear_end"] == 0.4 and sched["schedule"] == "linear"
    assert "_s50" in opt["path"]["experiments_root"]
