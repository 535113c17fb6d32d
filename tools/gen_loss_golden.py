"""Record tests/golden/p_losses_reference.npz by running the reference's ResiGaussianGuideDY.p_losses (CPU only, eval mode):

    python tools/gen_loss_golden.py

The reference is imported through oracle.gen_golden.import_reference() and never copied: only data is written.  The tiny
configuration of oracle/gen_golden.py (weights from ucdir_amd.weights.synth_state_dict, seed 0), the 50-step schedule, B = 2 at
64 x 64.  Recorded:
  * the seeds of the inputs (SR = cond, HR = guide of synth_inputs) and of the injected noise (torch.randn on a CPU generator);
  * the t and the fp32 levels numpy drew after np.random.seed(NP_SEED);
  * x_init (the reference predictor's output), x_noisy (what q_sample returned), eps (the denoiser's output);
  * the reference's l1 and l2 losses (nn.L1Loss / nn.MSELoss, reduction='sum', fp32).
Dropout is off (eval mode): the engine has none, so this is the loss the product evaluates.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "p_losses_reference.npz")
NP_SEED, NOISE_SEED, INPUT_SEED, B, H, W = 1234, 77, 41, 2, 64, 64


def main():
    from oracle import gen_golden as G
    from ucdir_amd.weights import synth_inputs
    networks = G.import_reference()
    net, cfg, _ = G.ref_model(networks, G.TINY, seed=0)
    net.set_new_noise_schedule(dict(G.SCHED50), torch.device("cpu"))
    net.eval()
    cond, guide, _ = synth_inputs(B, H, W, seed=INPUT_SEED)
    x_in = {"SR": torch.from_numpy(cond), "HR": torch.from_numpy(guide)}
    noise = torch.randn((B, 3, H, W), generator=torch.Generator().manual_seed(NOISE_SEED))
    rec = {"np_seed": NP_SEED, "noise_seed": NOISE_SEED, "input_seed": INPUT_SEED, "shape": np.array([B, 3, H, W]),
           "n_timestep": G.SCHED50["n_timestep"]}
    seen = {}
    q_sample, denoise = net.q_sample, net.denoise_fn.forward

    def q_spy(*a, **k):
        seen["x_noisy"] = q_sample(*a, **k)
        seen["levels"] = k["continuous_sqrt_alpha_cumprod"].reshape(-1).clone()
        return seen["x_noisy"]

    def d_spy(x, level, **k):
        seen["x_init"] = k["guide"]
        seen["eps"] = denoise(x, level, **k)
        return seen["eps"]
    net.q_sample, net.denoise_fn.forward = q_spy, d_spy
    with torch.no_grad():
        for kind in ("l1", "l2"):
            net.loss_type = kind
            net.set_loss(torch.device("cpu"))
            np.random.seed(NP_SEED)
            rec[kind] = np.float32(net.p_losses(x_in, noise=noise).item())
    # the draws written out, as a cross-check of what the spy saw
    np.random.seed(NP_SEED)
    t = np.random.randint(1, net.num_timesteps + 1)
    lv = torch.FloatTensor(np.random.uniform(net.sqrt_alphas_cumprod_prev[t - 1], net.sqrt_alphas_cumprod_prev[t], size=B))
    assert torch.equal(lv, seen["levels"])
    rec.update(t=t, levels=lv.numpy(), x_init=seen["x_init"].numpy(), x_noisy=seen["x_noisy"].numpy(), eps=seen["eps"].numpy())
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; t", t, "levels", lv.tolist(), "l1", rec["l1"], "l2", rec["l2"])


if __name__ == "__main__":
    main()
