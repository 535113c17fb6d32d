"""A restatement of the denoising loss's forward half (model/diffusion.py:306-343) in numpy, shared by tests/test_loss_cpu.py and
tests/test_loss_gpu.py.  It needs no device to import and calls nothing of the product."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "p_losses_reference.npz")
BLOCK = 4096            # elements of a sample per stage-one partial (csrc/loss.hip.h LOSS_BLOCK)
U64 = 2.0 ** -53        # unit roundoff of float64
U32 = 2.0 ** -24        # ... of fp32


def level_table(sched):
    """sqrt_alphas_cumprod_prev of a linear schedule: sqrt of the cumulative alpha product with a leading 1 (float64)."""
    assert sched["schedule"] == "linear"
    betas = np.linspace(sched["linear_start"], sched["linear_end"], sched["n_timestep"], dtype=np.float64)
    return np.sqrt(np.append(1.0, np.cumprod(1.0 - betas)))


def two_numpy_calls(prev, B, seed):
    """The reference's draws, written out: randint then uniform on numpy's global generator, rounded to fp32."""
    np.random.seed(seed)
    t = np.random.randint(1, len(prev))
    return t, np.random.uniform(prev[t - 1], prev[t], size=B).astype(np.float32)


def loss_sums(z, eps):
    """Per sample: the float64 sums of the fp32 terms |z - eps| and fl32((z - eps)^2)."""
    d = np.asarray(z, np.float32) - np.asarray(eps, np.float32)
    B = d.shape[0]
    return (np.abs(d).astype(np.float64).reshape(B, -1).sum(1), (d * d).astype(np.float64).reshape(B, -1).sum(1))


def workspace_bytes(B, per):
    return max(16, B * ((per - 1) // BLOCK + 1) * 16)


def profile_steps(ts, B, draws=1):
    """Sample b of call k takes step ts[(k B + b) % len(ts)]; len(ts) * draws evaluations, B to a call."""
    calls = -(-len(ts) * draws // B)
    return [[ts[(k * B + b) % len(ts)] for b in range(B)] for k in range(calls)]
