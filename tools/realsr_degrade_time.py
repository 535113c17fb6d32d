"""Time of the real-world SR degradation on the GPU: the three HIP operators of csrc/realsr.hip.h and the whole per-image chain
(degradations.realsr_degrade_device at 256^2 -> 64^2), each next to the same work composed from torch ops on the same GPU
(F.pad + F.conv2d for the blurs; the 4-D tensordots of a DiffJPEG written the way the reference writes it).  Per case the mean
over `iters` calls after a warm-up, event-timed on the device; the chain as wall time per image around a synchronise, over the
first `images` indices (their draws differ, so do their sizes).  Checks that both ways agree.  There is no pass mark.

    python tools/realsr_degrade_time.py [iters] [images] > profiles/realsr_degrade_time.json
"""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ucdir_amd import degradations as D  # noqa: E402
import realsr_model as RM  # noqa: E402


def torch_filter2d(x, kernel):
    k = kernel.shape[-1]
    b, c, h, w = x.shape
    xp = F.pad(x, (k // 2,) * 4, mode="reflect")
    if kernel.shape[0] == 1:
        return F.conv2d(xp.view(b * c, 1, *xp.shape[-2:]), kernel.view(1, 1, k, k)).view(b, c, h, w)
    wgt = kernel.view(b, 1, k, k).repeat(1, c, 1, 1).view(b * c, 1, k, k)
    return F.conv2d(xp.view(1, b * c, *xp.shape[-2:]), wgt, groups=b * c).view(b, c, h, w)


def torch_usm(x, K, weight=0.5, threshold=10):
    res = x - torch_filter2d(x, K)
    soft = torch_filter2d((res.abs() * 255 > threshold).float(), K)
    return soft * torch.clip(x + weight * res, 0, 1) + (1 - soft) * x


class TorchDiffJPEG:
    """DiffJPEG(differentiable=False) from torch ops in float32: 4-D cosine tensors contracted with tensordot, as the reference."""

    def __init__(self, dev):
        c = RM.COS
        self.fwd_t = torch.tensor(np.einsum("xu,yv->xyuv", c, c), dtype=torch.float32, device=dev)
        self.inv_t = torch.tensor(np.einsum("xu,yv->uvxy", c, c), dtype=torch.float32, device=dev)
        self.scale = torch.tensor(RM.SCALE, dtype=torch.float32, device=dev)
        self.alpha = torch.tensor(RM.ALPHA2, dtype=torch.float32, device=dev)
        self.tables = [torch.tensor(t, device=dev) for t in (RM.LUMA, RM.CHROMA, RM.CHROMA)]
        self.fwd_m, self.inv_m = torch.tensor(RM.FWD.T.copy(), device=dev), torch.tensor(RM.INV.T.copy(), device=dev)
        self.shift = torch.tensor([0.0, 128.0, 128.0], device=dev)

    @staticmethod
    def split(p):
        b, h, w = p.shape
        return p.view(b, h // 8, 8, w // 8, 8).permute(0, 1, 3, 2, 4).contiguous().view(b, -1, 8, 8)

    @staticmethod
    def merge(p, h, w):
        return p.view(p.shape[0], h // 8, w // 8, 8, 8).permute(0, 1, 3, 2, 4).contiguous().view(p.shape[0], h, w)

    def __call__(self, x, factors):
        b, _, h, w = x.shape
        x = F.pad(x, (0, -w % 16, 0, -h % 16))
        H, W = x.shape[-2:]
        ycc = torch.tensordot(x.permute(0, 2, 3, 1) * 255, self.fwd_m, dims=1) + self.shift
        planes = [ycc[..., 0], F.avg_pool2d(ycc[..., 1].unsqueeze(1), 2).squeeze(1), F.avg_pool2d(ycc[..., 2].unsqueeze(1), 2).squeeze(1)]
        rec = []
        for p, t in zip(planes, self.tables):
            tab = t.expand(b, 1, 8, 8) * factors.view(b, 1, 1, 1)
            coef = self.scale * torch.tensordot(self.split(p) - 128, self.fwd_t, dims=2)
            deq = torch.round(coef / tab) * tab
            pix = 0.25 * torch.tensordot(deq * self.alpha, self.inv_t, dims=2) + 128
            rec.append(self.merge(pix, *p.shape[-2:]))
        up = lambda c: c.repeat_interleave(2, 1).repeat_interleave(2, 2)  # noqa: E731
        img = torch.stack([rec[0], up(rec[1]), up(rec[2])], dim=3) - self.shift
        rgb = torch.tensordot(img, self.inv_m, dims=1).permute(0, 3, 1, 2)
        return (torch.clamp(rgb, 0, 255) / 255)[:, :, :h, :w].contiguous()


def event_ms(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def torch_chain(gt, p, dopt, K, jpeg):
    """realsr_degrade_device with the three operators replaced by the torch compositions above (same draws, same plumbing)."""
    dev = gt.device
    blur = lambda t, k: torch_filter2d(t, torch.from_numpy(np.ascontiguousarray(D.trim_kernel(k), dtype=np.float32)).to(dev)[None])  # noqa: E731
    jp = lambda t, q: jpeg(torch.clamp(t, 0, 1), torch.from_numpy(D.quality_to_factor(np.float32([q]))).to(dev))  # noqa: E731
    s, (h, w) = dopt["scale"], gt.shape[-2:]
    gen = torch.Generator(device=dev)
    gen.manual_seed(p["noise_seed"])
    out = blur(torch_usm(gt, K), p["kernel1"])
    out = D.resize_stage(out, p["resize1"]["mode"], scale_factor=p["resize1"]["scale"])
    out = jp(D.noise_stage(out, p["noise1"], gen), p["jpeg1"])
    if p["second_blur"]:
        out = blur(out, p["kernel2"])
    out = D.resize_stage(out, p["resize2"]["mode"], size=(int(h / s * p["resize2"]["scale"]), int(w / s * p["resize2"]["scale"])))
    out = D.noise_stage(out, p["noise2"], gen)
    back = lambda t: blur(D.resize_stage(t, p["final_mode"], size=(h // s, w // s)), p["sinc_kernel"])  # noqa: E731
    out = jp(back(out), p["jpeg2"]) if p["sinc_first"] else back(jp(out, p["jpeg2"]))
    return D.final_stage(out)


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    nimg = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    dev = torch.device("cuda")
    res = {"iters": iters, "operators": {}, "chain": {}}
    real = np.load(os.path.join(ROOT, "tests", "golden", "sid_real_image.npz"))["cond_u8"]
    img = torch.from_numpy((real.astype(np.float32) / 255.0).transpose(2, 0, 1).copy()).to(dev)
    K = torch.from_numpy(RM.usm_kernel(15)).to(dev)[None]
    jpeg = TorchDiffJPEG(dev)
    for B in (1, 16):
        x = img[None].repeat(B, 1, 1, 1).contiguous()
        ks = torch.stack([torch.from_numpy(D.pad_kernel(D.gaussian_kernel(21, 1.0 + 0.1 * b, 2.0, 0.3 * b, isotropic=False))
                                           .astype(np.float32)) for b in range(B)]).to(dev)
        q = torch.linspace(30, 95, B)
        f = torch.from_numpy(D.quality_to_factor(q.numpy())).to(dev)
        a, b_ = D.filter2d_device(x, ks), torch_filter2d(x, ks)
        u, v = D.usm_sharp_device(x), torch_usm(x, K)
        j, k_ = D.diffjpeg_device(x, q), jpeg(x, f)
        res["operators"][f"B{B}_3x256x256"] = {
            "filter2d_k21_hip_ms": event_ms(lambda: D.filter2d_device(x, ks), iters),
            "filter2d_k21_torch_ms": event_ms(lambda: torch_filter2d(x, ks), iters),
            "filter2d_max_abs_diff": float((a - b_).abs().max()),
            "usm_sharp_hip_ms": event_ms(lambda: D.usm_sharp_device(x), iters),
            "usm_sharp_torch_ms": event_ms(lambda: torch_usm(x, K), iters),
            "usm_share_of_pixels_differing_above_1e-4": float(((u - v).abs() > 1e-4).float().mean()),
            "diffjpeg_hip_ms": event_ms(lambda: D.diffjpeg_device(x, q), iters),
            "diffjpeg_torch_ms": event_ms(lambda: jpeg(x, f), iters),
            "diffjpeg_share_of_pixels_differing_above_1e-4": float(((j - k_).abs() > 1e-4).float().mean())}
    dopt, kopt = D.load_settings("dopt"), D.load_settings("param")
    gt = img[None].contiguous()
    params = [D.draw_realsr_params(i, dopt, kopt) for i in range(nimg)]
    runs = {"hip": lambda p: D.realsr_degrade_device(gt, p, dopt), "torch": lambda p: torch_chain(gt, p, dopt, K, jpeg)}
    for name, fn in runs.items():
        for p in params:                                          # warm every shape the timed pass uses
            fn(p)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for p in params:
            fn(p)
        torch.cuda.synchronize()
        res["chain"][f"{name}_wall_ms_per_image"] = 1e3 * (time.perf_counter() - t0) / nimg
    diff = [float((runs["hip"](p) - runs["torch"](p)).abs().mean()) * 255 for p in params]
    res["chain"].update(images=nimg, size="256x256 -> 64x64",
                        mean_abs_diff_u8_levels_hip_vs_torch={"mean": float(np.mean(diff)), "max": float(np.max(diff))})
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
