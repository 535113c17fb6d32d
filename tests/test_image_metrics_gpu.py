"""Device-side val scores (csrc/image_metrics.hip.h, metrics.psnr_ssim_device) against the host path of the val loop:
metrics.calculate_psnr / calculate_ssim applied to the uint8 images of tensor2img_u8_device."""
import importlib.util
import math
import os
import warnings

import numpy as np
import pytest
import torch

from ucdir_amd import metrics as M
from ucdir_amd.ucdir import image_metrics_

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def u8(t):
    """tensor2img_u8_device, also for one-channel images (HW uint8)."""
    if t.shape[0] == 3:
        return M.tensor2img_u8_device(t)
    return (((t[0].float().clamp(-1, 1) + 1) / 2) * 255.0).round().to(torch.uint8).cpu().numpy()


def host_scores(sr, hr):
    ps, ss = [], []
    for j in range(sr.shape[0]):
        a, b = u8(sr[j]), u8(hr[j])
        ps.append(M.calculate_psnr(a, b))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)     # numpy's mean of an empty map (H or W below 11)
            ss.append(float(M.calculate_ssim(a, b)))
    return ps, ss


def pair(B, C, H, W, seed, noise=0.3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    hr = torch.rand(B, C, H, W, device="cuda", generator=g) * 2.2 - 1.1             # a little beyond [-1, 1]: the clamp is exercised
    sr = hr + noise * torch.randn(B, C, H, W, device="cuda", generator=g)
    return sr, hr


def check(sr, hr, ssim_tol=1e-9):
    ps, ss = M.psnr_ssim_device(sr, hr)
    rp, rs = host_scores(sr, hr)
    assert ps == rp, (ps, rp)
    for a, b in zip(ss, rs):
        if math.isnan(b):
            assert math.isnan(a)
        else:
            assert abs(a - b) <= ssim_tol, (a, b)
    return ps, ss


def test_batch16_256():
    check(*pair(16, 3, 256, 256, 1))


def test_full_size_image():
    sr, hr = pair(1, 3, 1424, 2128, 2)
    check(sr, hr)


@pytest.mark.parametrize("hw", [(11, 11), (12, 37), (72, 88)])
def test_odd_sizes(hw):
    check(*pair(3, 3, hw[0], hw[1], 3))


def test_one_channel():
    check(*pair(4, 1, 72, 88, 4))


def test_cropped_strided_view_of_a_padded_stack():
    """DDPM.SR: the last block of an (11 B, 3, H + 128, W + 128) stack, cropped by 64 per side, read in place."""
    B, H, W = 2, 72, 88
    g = torch.Generator(device="cuda").manual_seed(5)
    out = torch.rand(11 * B, 3, H + 128, W + 128, device="cuda", generator=g) * 2 - 1
    sr = out[..., 64:-64, 64:-64][-B:]
    hr = torch.rand(B, 3, H, W, device="cuda", generator=g) * 2 - 1
    assert not sr.is_contiguous() and sr.stride(3) == 1
    ps, ss = check(sr, hr)
    assert (ps, ss) == M.psnr_ssim_device(sr.contiguous(), hr)


def test_rounding_half_steps():
    """x = (2k + 1) / 255 - 1 lands on q = k + 0.5 before rounding (in fp32 up to its rounding): pins round half to even."""
    k = torch.arange(0, 255, device="cuda", dtype=torch.float32)
    x = (2 * k + 1) / 255 - 1
    row = x.repeat(64)[: 64 * 48].view(48, 64)
    hr = torch.stack([row, row.flip(0), row.flip(1)])[None].repeat(2, 1, 1, 1)
    sr = hr.roll(1, dims=3).clone()
    sr[1] = hr[1]
    sr[1, 0, 0, 0] = 1.0
    check(sr, hr)
    # the uint8 values themselves: the PSNR of x against its own torch rounding is inf only if every pixel agrees
    ref = ((((hr.clamp(-1, 1) + 1) / 2) * 255.0).round() / 255.0) * 2 - 1
    ps, _ = M.psnr_ssim_device(hr, ref)
    assert ps == [float("inf")] * 2


def test_edge_values():
    sr, _ = pair(2, 3, 40, 50, 6)
    ps, ss = M.psnr_ssim_device(sr, sr.clone())
    assert ps == [float("inf")] * 2 and all(abs(s - 1.0) <= 1e-12 for s in ss)
    const_a = torch.full((2, 3, 40, 50), 0.25, device="cuda")
    const_b = torch.full((2, 3, 40, 50), -0.5, device="cuda")
    check(const_a, const_b)          # zero variance: SSIM = (2 mu_a mu_b + C1) / (mu_a^2 + mu_b^2 + C1)
    check(const_a, sr)
    ps, ss = check(*pair(2, 3, 10, 40, 7))
    assert all(math.isnan(s) for s in ss) and all(math.isfinite(p) for p in ps)


def test_bit_reproducible():
    for B, H, W in ((16, 256, 256), (1, 1424, 2128)):
        sr, hr = pair(B, 3, H, W, 8)
        s1, m1 = (t.clone() for t in image_metrics_(sr, hr))
        s2, m2 = image_metrics_(sr, hr)
        assert torch.equal(s1, s2)
        assert torch.equal(m1.view(torch.int64), m2.view(torch.int64))


@pytest.mark.parametrize("batch", [1, 2])
def test_sr_py_metrics_device_parity(tmp_path, monkeypatch, batch):
    import yaml
    from PIL import Image
    rs = np.random.RandomState(0)
    for d in ("lq", "gt"):
        os.makedirs(tmp_path / d)
    for i in range(2):
        gt = rs.randint(0, 255, (72, 88, 3)).astype(np.uint8)
        Image.fromarray(gt).save(tmp_path / "gt" / f"{i:03d}.png")
        Image.fromarray((gt * 0.2).astype(np.uint8)).save(tmp_path / "lq" / f"{i:03d}.png")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "sid.yaml")))
    cfg["datasets"]["val"]["data_args"]["dataroot"] = {"lq": str(tmp_path / "lq"), "gt": str(tmp_path / "gt")}
    cfg["model"]["unet"].update(channel_mults=[1, 2, 4], res_blocks=1, attn_res=[32])
    yaml.safe_dump(cfg, open(tmp_path / "sid_small.yaml", "w"))
    spec = importlib.util.spec_from_file_location("sr_entry_metrics", os.path.join(ROOT, "sr.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    res, jpgs = {}, {}
    for dev in ("cpu", "gpu"):
        wd = tmp_path / dev
        os.makedirs(wd)
        monkeypatch.chdir(wd)
        res[dev] = sr.main(["-p", "val", "-c", str(tmp_path / "sid_small.yaml"), "--synthetic-weights", "--seed", "7",
                            "--batch", str(batch), "--metrics-device", dev])
        jpgs[dev] = {f: open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(wd / "experiments") for f in fs
                     if f.endswith("_sr.jpg")}
    assert res["cpu"][0] == res["gpu"][0]
    assert abs(res["cpu"][1] - res["gpu"][1]) <= 1e-9
    assert len(jpgs["cpu"]) == 2 and jpgs["cpu"] == jpgs["gpu"]
