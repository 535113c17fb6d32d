"""Pillow-exact resampling of the 4x super-resolution val task on the GPU (csrc/resample.hip.h, metrics.resample_device): byte for
byte PIL.Image.resize and the numpy model of test_resample_cpu.py over the same filter x geometry x content matrix, batched and one
by one; single-axis and identity cases; the current stream; argument checks; bit-reproducibility; the ImagenetSRDataset loader on
the device; and `sr.py -p val` end to end on an `sr-` config."""
import os
import sys

import numpy as np
import pytest
import torch

from ucdir_amd import metrics as M
from ucdir_amd.data import ImagenetSRDataset, _u8_to_unit

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_resample_cpu import (CONTENTS, FILTERS, GEOMETRIES, make_content, pil_resize, pil_sr_chain, resample_model,  # noqa: E402
                               write_tree)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 16


def _batch(H, W, n=BATCH):
    """The three contents of the CPU matrix first, then further seeds of them."""
    return np.stack([make_content(CONTENTS[j % len(CONTENTS)], H, W, seed=j // len(CONTENTS)) for j in range(n)])


@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: "%dx%d-%dx%d" % (g[0] + g[1]))
@pytest.mark.parametrize("filt", FILTERS)
def test_kernel_equals_pillow_and_model(filt, geom):
    (W, H), (Wo, Ho) = geom
    host = _batch(H, W)
    x = torch.from_numpy(host).cuda()
    got = M.resample_device(x, (Ho, Wo), filt)
    assert got.shape == (BATCH, Ho, Wo, 3) and got.dtype == torch.uint8 and got.device == x.device
    got = got.cpu().numpy()
    for j in range(BATCH):
        ref = pil_resize(host[j], (Ho, Wo), filt)
        bad = np.argwhere(got[j] != ref)
        assert bad.size == 0, (j, len(bad), bad[:3].tolist())
        if j < len(CONTENTS):
            assert np.array_equal(ref, resample_model(host[j], (Ho, Wo), filt)), j
    for j in range(BATCH):                          # one by one, (H, W, 3): batching changes no byte
        one = M.resample_device(x[j], (Ho, Wo), filt)
        assert one.shape == (Ho, Wo, 3) and one.device == x.device
        assert np.array_equal(one.cpu().numpy(), got[j]), j
    assert np.array_equal(x.cpu().numpy(), host)    # the input is left alone


@pytest.mark.parametrize("size", [(50, 40), (50, 97), (23, 40), (131, 40), (3, 2), (3, 40), (50, 2), (50, 3), (200, 200)])
@pytest.mark.parametrize("filt", FILTERS)
def test_single_axis_identity_and_odd_sizes(filt, size):
    """From 50 x 40 (H x W): the same size (a copy), one axis alone in both directions, the smallest outputs the tap cap admits for
    Lanczos (50 -> 3 spans 101 taps, 40 -> 2 spans 121), three output columns, and both axes at once."""
    host = _batch(50, 40, 5)
    x = torch.from_numpy(host).cuda()
    got = M.resample_device(x, size, filt)
    assert got.data_ptr() != x.data_ptr()
    got = got.cpu().numpy()
    for j in range(5):
        assert np.array_equal(got[j], pil_resize(host[j], size, filt)), j
    assert np.array_equal(x.cpu().numpy(), host)


def test_one_pixel_and_one_row_inputs():
    for H, W in ((1, 1), (1, 9), (9, 1)):
        host = _batch(H, W, 3)
        x = torch.from_numpy(host).cuda()
        for filt in FILTERS:
            got = M.resample_device(x, (12, 7), filt).cpu().numpy()
            for j in range(3):
                assert np.array_equal(got[j], pil_resize(host[j], (12, 7), filt)), (H, W, filt, j)


def test_one_pixel_and_one_row_outputs():
    host = _batch(9, 12, 3)
    x = torch.from_numpy(host).cuda()
    for size in ((1, 1), (1, 12), (9, 1), (1, 30), (30, 1)):
        for filt in FILTERS:
            got = M.resample_device(x, size, filt).cpu().numpy()
            for j in range(3):
                assert np.array_equal(got[j], pil_resize(host[j], size, filt)), (size, filt, j)


def test_sr_chain_equals_pillow():
    """Crop 375^2 of a 500 x 375 image -> 256^2 -> 64^2 -> 256^2, every stage."""
    for kind in CONTENTS:
        img = make_content(kind, 375, 500)
        hr, lr, sr = pil_sr_chain(img)
        x = torch.from_numpy(img).cuda()[:, 62:437].contiguous()
        d_hr = M.resample_device(x, (256, 256))                 # bicubic is the default
        d_lr = M.resample_device(d_hr, (64, 64))
        d_sr = M.resample_device(d_lr, (256, 256))
        for got, ref in ((d_hr, hr), (d_lr, lr), (d_sr, sr)):
            assert np.array_equal(got.cpu().numpy(), ref), kind


def test_runs_on_the_current_stream():
    host = _batch(64, 48)
    x = torch.from_numpy(host).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y = M.resample_device(x, (150, 100))
    s.synchronize()
    assert np.array_equal(y.cpu().numpy()[3], pil_resize(host[3], (150, 100), "bicubic"))


def test_bit_reproducible():
    x = torch.from_numpy(_batch(375, 500, 4)).cuda()
    for filt in FILTERS:
        a = M.resample_device(x, (256, 341), filt)
        b = M.resample_device(x, (256, 341), filt)
        assert torch.equal(a, b), filt


def test_bad_arguments_are_refused():
    x = torch.zeros(2, 32, 32, 3, dtype=torch.uint8, device="cuda")
    for bad, match in ((x.cpu(), "GPU"), (x.float(), "uint8"), (x.transpose(1, 2), "contiguous"),
                       (x[:, :, :, :2].contiguous(), r"\(B, H, W, 3\)"), (x[0, 0], r"\(B, H, W, 3\)"),
                       (x[:0], r"\(B, H, W, 3\)")):
        with pytest.raises(ValueError, match=match):
            M.resample_device(bad, (16, 16))
    for size in ((0, 16), (16, -1), (16.5, 16), (16,), 16, (16, 16, 3), (True, 16), None):
        with pytest.raises(ValueError, match="size"):
            M.resample_device(x, size)
    for filt in ("nearest", "BICUBIC", 2, None):
        with pytest.raises(ValueError, match="filter"):
            M.resample_device(x, (16, 16), filt)
    with pytest.raises(Exception, match="ksize cap"):           # 32 -> 1 with Lanczos spans 193 taps
        M.resample_device(x, (1, 16), "lanczos")


# ---------------------------------------------------------------------------------------------------------------------
# the loader on the device
# ---------------------------------------------------------------------------------------------------------------------
def test_loader_equals_the_pil_chain(tmp_path):
    from PIL import Image
    sizes = [(300, 400), (256, 256), (200, 180)]     # (H, W); the last has its shorter side below 256: the pre-resize path
    root = write_tree(tmp_path, sizes)
    ds = ImagenetSRDataset({"dataroot": root, "data_len": -1})
    for i in range(len(sizes)):
        full = np.asarray(Image.open(ds.hr_path[i]).convert("RGB"))
        assert full.shape[:2] == sizes[i]
        hr, lr, sr = pil_sr_chain(full)
        item = ds[i]
        assert np.array_equal(ds.last_lr64.cpu().numpy(), lr), i
        d_hr, d_lr, d_sr = ds.degrade_u8(torch.from_numpy(full.copy()).cuda())
        for got, ref in ((d_hr, hr), (d_lr, lr), (d_sr, sr)):
            assert got.is_cuda and np.array_equal(got.cpu().numpy(), ref), i
        assert item["Index"] == i and item["HR"].is_cuda and item["HR"].shape == (3, 256, 256)
        assert torch.equal(item["HR"], _u8_to_unit(torch.from_numpy(hr.copy()).cuda()))
        assert torch.equal(item["SR"], _u8_to_unit(torch.from_numpy(sr.copy()).cuda()))
        assert torch.equal(item["LR"], item["SR"])


# ---------------------------------------------------------------------------------------------------------------------
# end to end through sr.py
# ---------------------------------------------------------------------------------------------------------------------
def _decode(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def test_sr_val_entry_point_sr(tmp_path, monkeypatch):
    """`sr.py -p val` on an `sr-` config: an ImageNet-style tree, HR / LR / SR formed on the GPU, the three 256^2 images restored as
    one batch by a small UNet with synthetic weights."""
    import importlib.util

    import yaml
    from PIL import Image
    run = tmp_path / "run"
    os.makedirs(run)
    sizes = [(300, 400), (256, 256), (200, 180)]
    root = write_tree(tmp_path, sizes)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "sr.yaml")))
    cfg["model"]["unet"].update(channel_mults=[1, 2, 4], res_blocks=1, attn_res=[32])
    cfg["datasets"]["val"]["data_args"]["dataroot"] = root
    yaml.safe_dump(cfg, open(tmp_path / "sr_small.yaml", "w"))
    monkeypatch.chdir(run)
    spec = importlib.util.spec_from_file_location("sr_entry_sr_gpu", os.path.join(ROOT, "sr.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    psnr, ssim = sr.main(["-p", "val", "-c", str(tmp_path / "sr_small.yaml"), "--synthetic-weights", "--seed", "1"])
    assert np.isfinite(psnr) and -1.0 <= ssim <= 1.0
    assert [g[0] for g in sr.main.last_groups] == [3]               # every image is 256^2: one DDPM.test call
    outs = {f: os.path.join(d, f) for d, _, fs in os.walk(run / "experiments") for f in fs if f.endswith(".jpg")}
    for k in range(len(sizes)):
        stem = f"ILSVRC2012_val_{k:08d}"
        for kind in ("sr", "hr", "lr", "inf"):
            assert [f for f in outs if f.startswith(stem + "_") and f.endswith(f"_{kind}.jpg")], (stem, kind, sorted(outs))
        hr, _, lr = pil_sr_chain(np.asarray(Image.open(os.path.join(root["root"], stem + ".JPEG")).convert("RGB")))
        for kind, ref in (("hr", hr), ("lr", lr)):
            M.save_jpg(ref, str(tmp_path / f"{stem}_{kind}_ref.png"))
            got = [p for f, p in outs.items() if f.startswith(stem + "_") and f.endswith(f"_{kind}.jpg")][0]
            assert np.array_equal(_decode(got), _decode(tmp_path / f"{stem}_{kind}_ref.jpg")), (stem, kind)
