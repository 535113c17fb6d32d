"""The HIP baseline JPEG encoder (csrc/jpeg_encode.hip.h) on the GPU: its files equal Pillow's and the numpy model's
(tests/jpeg_encode_model.py) byte for byte - one image at a time over the matrix of tests/test_jpeg_encode_cpu.py, in a batch of
mixed content, at shapes past one workgroup's scan and past one round of the second-level scan - twice the same, and
``sr.py --jpeg-device gpu`` writes the files ``--jpeg-device cpu`` writes."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import jpeg_encode_model as M
from test_jpeg_encode_cpu import QUALITIES, SIZES, first_diff
from ucdir_amd import metrics as Metrics

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(img):
    return torch.from_numpy(np.ascontiguousarray(img)).cuda()


@functools.lru_cache(maxsize=None)
def references(kind, H, W, seed, q, sub, bgr):
    """(image, Pillow's file, the model's file); bgr: both of the channel-reversed array, which is what the flag means."""
    img = M.make_content(kind, H, W, seed)
    seen = np.ascontiguousarray(img[..., ::-1]) if bgr else img
    return img, M.pillow(seen, q, sub), M.encode(seen, q, sub)


def check_one(kind, H, W, seed, q, sub, bgr):
    img, ref, model = references(kind, H, W, seed, q, sub, bgr)
    got, = Metrics.jpeg_encode_device(dev(img), quality=q, subsampling=sub, bgr=bool(bgr))
    assert got == ref, (kind, H, W, q, sub, bgr, first_diff(got, ref))
    assert got == model


@pytest.mark.parametrize("bgr", [0, 1])
@pytest.mark.parametrize("sub", [0, 2])
def test_kernel_equals_pillow_and_model(sub, bgr):
    for H, W in SIZES:
        for kind in ("noise", "real", "gradient"):
            for q in QUALITIES:
                check_one(kind, H, W, 0, q, sub, bgr)
    check_one("noise", 256, 256, 0, 100, sub, bgr)


@pytest.mark.parametrize("sub", [0, 2])
def test_kernel_on_the_contents_that_reach_each_arm(sub):
    for kind, q, H, W, seed in (("flat", 100, 16, 16, 0), ("flat", 100, 8, 8, 0), ("noise", 100, 64, 64, 0), ("checker", 100, 16, 16, 0),
                                ("bwblocks", 100, 16, 16, 0), ("coef63", 75, 16, 16, 0), ("run15", 75, 16, 16, 0),
                                ("run16", 75, 16, 16, 0), ("gradient", 75, 40, 56, 0), ("real", 100, 48, 64, 0),
                                ("noise", 100, 8, 8, 18)):
        check_one(kind, H, W, seed, q, sub, 0)


def mixed_batch():
    # seeds picked so that the 16 files differ in length at both settings test_batch_of_mixed_content uses, bgr or not
    kinds = [("real", 0), ("gradient", 0), ("flat", 0), ("checker", 0), ("bwblocks", 0), ("coef63", 0), ("run15", 0), ("run16", 0),
             ("noise", 0), ("noise", 1), ("noise", 3), ("noise", 4), ("smooth", 0), ("smooth", 1), ("smooth", 2), ("smooth", 5)]
    return np.stack([M.make_content(k, 64, 64, s) for k, s in kinds])


@pytest.mark.parametrize("bgr", [0, 1])
@pytest.mark.parametrize("sub,q", [(0, 100), (2, 75)])
def test_batch_of_mixed_content(sub, q, bgr):
    """16 images of 64 x 64 whose files all differ in length: every image's offsets and length are its own."""
    imgs = mixed_batch()
    files = Metrics.jpeg_encode_device(dev(imgs), quality=q, subsampling=sub, bgr=bool(bgr))
    refs = [M.pillow(np.ascontiguousarray(a[..., ::-1]) if bgr else a, q, sub) for a in imgs]
    assert len(set(len(r) for r in refs)) == 16
    for n, (f, r) in enumerate(zip(files, refs)):
        assert f == r, (n, first_diff(f, r))
    # one image on its own gives the file it gives in the batch
    assert Metrics.jpeg_encode_device(dev(imgs[5]), quality=q, subsampling=sub, bgr=bool(bgr)) == [files[5]]


@pytest.mark.parametrize("kind,H,W,q,sub", [
    ("noise", 1001, 1503, 100, 0),       # 71064 blocks: 556 groups of 128, three rounds of the 256-wide group scan; ~1200 chunks of stuffing
    ("noise", 1001, 1503, 100, 2),       # 35532 blocks: 278 groups, two rounds; dummy luma blocks on the right and bottom edges
    ("smooth", 1424, 2128, 100, 0),      # the patch-split val image
])
def test_larger_shapes(kind, H, W, q, sub):
    img = M.make_content(kind, H, W)
    got, = Metrics.jpeg_encode_device(dev(img), quality=q, subsampling=sub)
    ref = M.pillow(img, q, sub)
    assert got == ref, first_diff(got, ref)


def test_same_bytes_twice():
    imgs = dev(mixed_batch())
    a = Metrics.jpeg_encode_device(imgs, quality=100, subsampling=0)
    b = Metrics.jpeg_encode_device(imgs, quality=100, subsampling=0)
    assert a == b
    big = dev(M.make_content("noise", 250, 333))
    assert Metrics.jpeg_encode_device(big, 100, 0) == Metrics.jpeg_encode_device(big, 100, 0)


def test_python_layer_validates():
    x = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device="cuda")
    for kw, pat in ((dict(quality=0), "quality"), (dict(quality=101), "quality"), (dict(quality=7.5), "quality"),
                    (dict(subsampling=1), "subsampling")):
        with pytest.raises(ValueError, match=pat):
            Metrics.jpeg_encode_device(x, **kw)
    with pytest.raises(ValueError, match="uint8"):
        Metrics.jpeg_encode_device(x.float())
    with pytest.raises(ValueError, match="contiguous"):
        Metrics.jpeg_encode_device(x.permute(0, 2, 1, 3))
    with pytest.raises(ValueError, match="images"):
        Metrics.jpeg_encode_device(x[..., :2].contiguous())
    assert len(Metrics.jpeg_encode_device(x)) == 2 and len(Metrics.jpeg_encode_device(x[0])) == 1


def test_batch_conversion_equals_per_image():
    """Values outside [-1, 1] and exact .5 ties ((k + 0.5) / 255 * 2 - 1 sits on a rounding tie wherever it is exact in fp32)."""
    g = torch.Generator().manual_seed(3)
    t = torch.randn(5, 3, 9, 13, generator=g) * 0.8
    ties = (torch.arange(0, 255, dtype=torch.float32) + 0.5) / 255.0 * 2 - 1
    t.view(-1)[:255] = ties
    t[1, 0, 0, :4] = torch.tensor([-7.0, 7.0, -1.0, 1.0])
    t = t.cuda()
    got = Metrics.tensor2img_u8_batch_device(t)
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (5, 9, 13, 3) and got.is_contiguous()
    for j in range(5):
        assert np.array_equal(got[j].cpu().numpy(), Metrics.tensor2img_u8_device(t[j]))
    assert int(got.min()) == 0 and int(got.max()) == 255


@pytest.mark.parametrize("metrics_device", ["cpu", "gpu"])
def test_sr_py_jpeg_device_parity(tmp_path, monkeypatch, metrics_device):
    """Three 72 x 88 images with --batch 2: one batched group and one batch-1 remainder.  Same file names, same bytes, same scores."""
    import yaml
    from PIL import Image
    rs = np.random.RandomState(0)
    for d in ("lq", "gt"):
        os.makedirs(tmp_path / d)
    for i in range(3):
        gt = rs.randint(0, 255, (72, 88, 3)).astype(np.uint8)
        Image.fromarray(gt).save(tmp_path / "gt" / f"{i:03d}.png")
        Image.fromarray((gt * 0.2).astype(np.uint8)).save(tmp_path / "lq" / f"{i:03d}.png")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "sid.yaml")))
    cfg["datasets"]["val"]["data_args"]["dataroot"] = {"lq": str(tmp_path / "lq"), "gt": str(tmp_path / "gt")}
    cfg["model"]["unet"].update(channel_mults=[1, 2, 4], res_blocks=1, attn_res=[32])
    yaml.safe_dump(cfg, open(tmp_path / "sid_small.yaml", "w"))
    spec = importlib.util.spec_from_file_location("sr_entry_jpeg_device", os.path.join(ROOT, "sr.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    res, jpgs = {}, {}
    for jd in ("cpu", "gpu"):
        wd = tmp_path / jd
        os.makedirs(wd)
        monkeypatch.chdir(wd)
        res[jd] = sr.main(["-p", "val", "-c", str(tmp_path / "sid_small.yaml"), "--synthetic-weights", "--seed", "7", "--batch", "2",
                           "--metrics-device", metrics_device, "--jpeg-device", jd])
        assert sorted(g[0] for g in sr.main.last_groups) == [1, 2]
        jpgs[jd] = {f: open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(wd / "experiments") for f in fs if f.endswith(".jpg")}
    assert res["cpu"] == res["gpu"]
    assert len(jpgs["cpu"]) == 12 and sorted(jpgs["cpu"]) == sorted(jpgs["gpu"])
    for f in jpgs["cpu"]:
        assert jpgs["cpu"][f] == jpgs["gpu"][f], (f, first_diff(jpgs["gpu"][f], jpgs["cpu"][f]))
