"""JPEG degradation of the ImageNet val task on the GPU (csrc/jpeg_roundtrip.hip.h, metrics.jpeg_roundtrip_device): byte for byte
Pillow's libjpeg-turbo round trip and the numpy model of test_jpeg_roundtrip_cpu.py, batched and one by one; argument checks; and
`sr.py -p val` end to end on a `jpg-` config with the ImagenetJPGDataset loader."""
import os
import sys

import numpy as np
import pytest
import torch

from ucdir_amd import metrics as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_jpeg_roundtrip_cpu import CONTENTS, QUALITIES, SIZES, jpeg_model, make_content, pillow_roundtrip  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 16


def _batch(H, W):
    """The five contents of the CPU matrix, then more noise / real / black-and-white images up to 16."""
    imgs = [make_content(k, H, W) for k in CONTENTS]
    extra = ("noise", "real", "bw", "edges")
    imgs += [make_content(extra[j % len(extra)], H, W, seed=j + 1) for j in range(BATCH - len(imgs))]
    return np.stack(imgs)


@pytest.mark.parametrize("H,W", SIZES + ((375, 500),))
@pytest.mark.parametrize("bgr", [False, True])
def test_kernel_equals_pillow_and_model(H, W, bgr):
    host = _batch(H, W)
    x = torch.from_numpy(host).cuda()
    for q in QUALITIES:
        got = M.jpeg_roundtrip_device(x, q, bgr=bgr).cpu().numpy()
        for j in range(BATCH):
            ref = pillow_roundtrip(host[j], q, bgr)
            bad = np.argwhere(got[j] != ref)
            assert bad.size == 0, (q, j, len(bad), bad[:3].tolist())
            if j < len(CONTENTS):
                assert np.array_equal(ref, jpeg_model(host[j], q, bgr)), (q, j)
        for j in range(BATCH):                      # one by one, (H, W, 3): batching changes no byte
            one = M.jpeg_roundtrip_device(x[j], q, bgr=bgr)
            assert one.shape == (H, W, 3) and one.device == x.device
            assert np.array_equal(one.cpu().numpy(), got[j]), (q, j)
    assert np.array_equal(x.cpu().numpy(), host)   # the input is left alone


def test_runs_on_the_current_stream():
    host = _batch(64, 48)
    x = torch.from_numpy(host).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y = M.jpeg_roundtrip_device(x, 10)
    s.synchronize()
    assert np.array_equal(y.cpu().numpy()[3], pillow_roundtrip(host[3], 10, True))


def test_bad_arguments_are_refused():
    x = torch.zeros(2, 32, 32, 3, dtype=torch.uint8, device="cuda")
    for bad, match in ((x.cpu(), "GPU"), (x.float(), "uint8"), (x.transpose(1, 2), "contiguous"),
                       (x[:, :, :, :2].contiguous(), r"\(B, H, W, 3\)"), (x[:, :15].contiguous(), "at least 16"),
                       (x[:, :, :8].contiguous(), "at least 16"), (x[0, 0], r"\(B, H, W, 3\)")):
        with pytest.raises(ValueError, match=match):
            M.jpeg_roundtrip_device(bad, 10)
    for q in (0, 101, 10.5, -3, True):
        with pytest.raises(ValueError, match="quality"):
            M.jpeg_roundtrip_device(x, q)


def _decode(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def test_sr_val_entry_point_jpg(tmp_path, monkeypatch):
    """`sr.py -p val` on a `jpg-` config: ImageNet-style JPEGs under ../data/images/val, list ./imagenet_val_1k.txt, degraded on the
    GPU at quality 10 with the reference's channel order, restored by a small UNet with synthetic weights."""
    import importlib.util

    import yaml
    from PIL import Image
    val = tmp_path / "data" / "images" / "val"
    run = tmp_path / "run"
    os.makedirs(val)
    os.makedirs(run)
    # DDPM.test reflect-pads 64 per side, so every crop is above 64: two crop to 96 x 112, one to 80 x 128
    sizes = {"ILSVRC2012_val_00000001.JPEG": (100, 120), "ILSVRC2012_val_00000002.JPEG": (98, 125),
             "ILSVRC2012_val_00000003.JPEG": (83, 141)}
    for k, (name, (h, w)) in enumerate(sizes.items()):
        Image.fromarray(make_content("real", h, w, seed=k)).save(val / name, "JPEG", quality=90)
    (run / "imagenet_val_1k.txt").write_text("".join(f"{n} {k}\n" for k, n in enumerate(sizes)))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "jpg.yaml")))
    cfg["model"]["unet"].update(channel_mults=[1, 2, 4], res_blocks=1, attn_res=[32])
    yaml.safe_dump(cfg, open(tmp_path / "jpg_small.yaml", "w"))
    monkeypatch.chdir(run)
    spec = importlib.util.spec_from_file_location("sr_entry_jpg_gpu", os.path.join(ROOT, "sr.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    psnr, ssim = sr.main(["-p", "val", "-c", str(tmp_path / "jpg_small.yaml"), "--synthetic-weights", "--seed", "1"])
    assert np.isfinite(psnr) and -1.0 <= ssim <= 1.0
    outs = {f: os.path.join(d, f) for d, _, fs in os.walk(run / "experiments") for f in fs if f.endswith(".jpg")}
    for name, (h, w) in sizes.items():
        stem = os.path.splitext(name)[0]
        for kind in ("sr", "hr", "lr", "inf"):
            assert [f for f in outs if f.startswith(stem + "_") and f.endswith(f"_{kind}.jpg")], (name, kind, sorted(outs))
        full = _decode(val / name)
        h16, w16 = h // 16 * 16, w // 16 * 16
        top, left = (h - h16) // 2, (w - w16) // 2
        crop = np.ascontiguousarray(full[top:top + h16, left:left + w16])
        M.save_jpg(pillow_roundtrip(crop, 10, bgr=True), str(tmp_path / f"{stem}_ref.png"))
        lr = [p for f, p in outs.items() if f.startswith(stem + "_") and f.endswith("_lr.jpg")][0]
        assert np.array_equal(_decode(lr), _decode(tmp_path / f"{stem}_ref.jpg")), name
        hr = [p for f, p in outs.items() if f.startswith(stem + "_") and f.endswith("_hr.jpg")][0]
        ref_hr = tmp_path / f"{stem}_hr_ref.png"
        M.save_jpg(crop, str(ref_hr))
        assert np.array_equal(_decode(hr), _decode(str(ref_hr).replace(".png", ".jpg"))), name
