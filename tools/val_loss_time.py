"""Event-timed cost of the denoising loss's two kernels (csrc/loss.hip.h) on one MI355X:

    python tools/val_loss_time.py [reps] [out.json]          # default 20 and profiles/val_loss_time.json

At B = 16, 256^2 and at one 1424 x 2128 image, `reps` alternating repetitions, medians; a repetition is LAUNCHES calls back to back
between two events, divided by LAUNCHES, so that the window is milliseconds of device work and not one launch's overhead:
  * fused:    qsample_ (regenerating nothing: it draws z) and noise_loss_ (regenerating z), no noise tensor in memory;
  * composed: the same arithmetic from torch ops on the same device - HR - x_init, fill_normal_ into a noise tensor (torch.randn is
              another generator; the stream is kept so that both sides draw the same z), the three scalings, abs / square and the
              fp32 sums - the yardstick;
  * share:    both kernels in one p_losses call of the full SID configuration with synthetic weights (predictor and denoiser
              forward included).
Bytes each kernel must move (reads + writes, fp32) are computed from the shapes and set against the 6.3 TB/s a float4 copy reaches on
this chip (8.0 TB/s is the HBM3E specification)."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ucdir_amd.ucdir import fill_normal_, noise_loss_, noise_loss_workspace_bytes, qsample_  # noqa: E402

HBM_MEASURED = 6.3e12        # bytes / s, float4 copy
SHAPES = ((16, 256, 256), (1, 1424, 2128))
LAUNCHES = 100               # calls per timed window


def timed(fn, launches=LAUNCHES):
    """Milliseconds per call: `launches` calls back to back between two events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def kernels_case(B, H, W, reps):
    shape = (B, 3, H, W)
    n, per = B * 3 * H * W, 3 * H * W
    g = torch.Generator(device="cuda").manual_seed(0)
    hr, xi, eps = (torch.rand(shape, device="cuda", generator=g) * 2 - 1 for _ in range(3))
    lv = torch.rand(B, device="cuda", generator=g)
    out, both = torch.empty_like(hr), torch.empty(2 * B, dtype=torch.float64, device="cuda")
    ws = torch.empty(noise_loss_workspace_bytes(B, per), dtype=torch.uint8, device="cuda")

    def fused_q():
        qsample_(hr, xi, lv, out=out, seed=7)

    def fused_l():
        noise_loss_(eps, seed=7, out=both, workspace=ws)

    def torch_q():
        z = fill_normal_(torch.empty_like(hr), 7)
        c = lv.view(B, 1, 1, 1)
        return c * (hr - xi) + torch.sqrt(1.0 - c * c) * z, z

    zt = fill_normal_(torch.empty_like(hr), 7)

    def torch_l():
        d = zt - eps
        return d.abs().sum(), (d * d).sum()

    fns = {"qsample": fused_q, "noise_loss": fused_l, "torch_qsample": torch_q, "torch_loss": torch_l}
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):                                     # alternating
        for k, f in fns.items():
            ms[k].append(timed(f))
    med = {k: statistics.median(v) for k, v in ms.items()}
    bytes_q, bytes_l = 3 * 4 * n + 4 * B, 4 * n + ws.numel() * 2 + 16 * B      # hr, x_init, x_noisy | eps, partials written and read
    return {
        "fused_ms": {"qsample": med["qsample"], "noise_loss": med["noise_loss"], "both": med["qsample"] + med["noise_loss"]},
        "torch_ms": {"qsample": med["torch_qsample"], "loss": med["torch_loss"], "both": med["torch_qsample"] + med["torch_loss"]},
        "spread_ms": {k: [min(v), max(v)] for k, v in ms.items()},
        "bytes": {"qsample": bytes_q, "noise_loss": bytes_l},
        "share_of_hbm_copy_rate": {"qsample": bytes_q / (med["qsample"] * 1e-3) / HBM_MEASURED,
                                   "noise_loss": bytes_l / (med["noise_loss"] * 1e-3) / HBM_MEASURED},
        "reps": reps, "launches_per_window": LAUNCHES,
    }


def sid_net():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hip_checks as C
    from ucdir_amd.spec import UNetConfig
    net, _ = C.build_net(UNetConfig(inner_channel=64, channel_mults=(1, 2, 4, 8, 8), res_blocks=2, attn_res=(16,), image_size=128))
    net.set_new_noise_schedule(dict(schedule="linear", n_timestep=50, linear_start=1e-6, linear_end=0.4), torch.device("cuda"))
    return net


def share_case(net, B, H, W, reps, kernels):
    """One whole p_losses call (predictor, noising, denoiser, reduction) of the SID configuration with synthetic weights."""
    g = torch.Generator(device="cuda").manual_seed(1)
    x = {k: torch.rand((B, 3, H, W), device="cuda", generator=g) * 2 - 1 for k in ("HR", "SR")}
    net.noise_seed = 3
    lv = np.linspace(0.1, 0.9, B).astype(np.float32)
    for _ in range(2):
        net.p_losses(x, levels=lv)
    torch.cuda.synchronize()
    ms = [timed(lambda: net.p_losses(x, levels=lv), 1) for _ in range(max(reps // 4, 3))]
    call = statistics.median(ms)
    return {"p_losses_ms": call, "kernels_share": kernels / call}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "val_loss_time.json")
    assert torch.cuda.is_available(), "val_loss_time.py measures on an MI355X; there is nothing to fall back to"
    res = {"device": torch.cuda.get_device_name(0), "hbm_copy_rate_bytes_per_s": HBM_MEASURED}
    net = sid_net()
    for B, H, W in SHAPES:
        r = kernels_case(B, H, W, reps)
        r.update(share_case(net, B, H, W, reps, r["fused_ms"]["both"]))
        res["B%d_%dx%d" % (B, H, W)] = r
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
