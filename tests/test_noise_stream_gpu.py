"""GPU tests of the sampler's in-kernel noise against its float64 host reference (oracle.philox_normal, the stream include/ucdir_hip.h
states): fill_normal_, sampler_step_rng_ and fewstep_update_ with one stream or per-sample streams, the step numbering of every
sampling loop, and the per-sample keys of GaussianDiffusion.  Bounds: hip_checks.NOISE_Z_TOL / NOISE_LOOP_TOL / NOISE_LOOP_RMS_TOL.

Not reached here: the counter's high word (group >= 2^32 needs a buffer above 2^34 elements); tests/test_noise_stream_cpu.py checks the
reference there."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_checks as C  # noqa: E402
from oracle import ucdir_oracle as O  # noqa: E402
from ucdir_amd.spec import UNetConfig  # noqa: E402
from ucdir_amd.ucdir import FEWSTEP_CLIP, FEWSTEP_FACTORED, fewstep_update_, fill_normal_, sampler_step_rng_  # noqa: E402
from ucdir_amd.weights import synth_inputs  # noqa: E402

DEV = torch.device("cuda")
M64 = 2 ** 64 - 1
SEEDS = [0, 1234, 2 ** 32 + 7, 2 ** 63 + 5, M64]
STEPS = [0, 1, 49, 2 ** 31 + 3, 2 ** 32 - 1]
SIZES = [1, 3, 5, 1027, 2 ** 20 + 2]
GRID_PASSES = 4 * 4096 * 256 + 6      # the launch caps at 4096 blocks of 256 threads, four elements each: two grid-stride passes and a tail
HIGH_SEEDS = [2 ** 32 + 7, 2 ** 63 + 5, M64, 0x9E3779B97F4A7C15, 2 ** 40 + 1234]


def _dz(got, ref):
    return float(np.abs(got.detach().cpu().double().numpy().reshape(-1) - ref.reshape(-1)).max())


def _keys(seeds):
    """Per-sample seeds as the int64 CUDA tensor of their uint64 bit patterns."""
    return torch.from_numpy(np.array([int(s) & M64 for s in seeds], dtype=np.uint64).view(np.int64)).to(DEV)


def _guarded(n, fill=float("nan")):
    """An n-element view at the start of a buffer with 8 guard elements after it: a write past element n - 1 shows."""
    buf = torch.full((n + 8,), fill, device=DEV)
    return buf, buf[:n]


# ---- fill_normal_ -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_fill_normal_is_the_reference_stream(seed):
    worst = 0.0
    for step in STEPS:
        for n in SIZES:
            buf, x = _guarded(n)
            fill_normal_(x, seed, step)
            torch.cuda.synchronize()
            assert bool(torch.isnan(buf[n:]).all()), (seed, step, n)        # nothing written past the tail
            d = _dz(x, O.philox_normal(n, seed, step))
            worst = max(worst, d)
            assert d <= C.NOISE_Z_TOL, (seed, step, n, d)
    if seed == 2 ** 63 + 5:
        buf, x = _guarded(GRID_PASSES)
        fill_normal_(x, seed, 49)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[GRID_PASSES:]).all())
        d = _dz(x, O.philox_normal(GRID_PASSES, seed, 49))
        worst = max(worst, d)
        assert d <= C.NOISE_Z_TOL, d
    print("fill_normal_ seed %d: worst |dz| %.3e" % (seed, worst))


@pytest.mark.parametrize("per", [12, 3 * 40 * 56])
def test_fill_normal_per_sample_streams_are_the_reference_streams(per):
    """B = 5 samples, each seed with its high word set: sample b is the stream of seeds[b] counted from its own first element."""
    worst = 0.0
    for step in (0, 49, 2 ** 32 - 1):
        x = torch.full((5, per), float("nan"), device=DEV)
        fill_normal_(x, 0, step, seeds=_keys(HIGH_SEEDS))
        ref = O.philox_normal(5 * per, 0, step, per=per, seeds=HIGH_SEEDS).reshape(5, per)
        for b, s in enumerate(HIGH_SEEDS):
            d = _dz(x[b], ref[b])
            worst = max(worst, d)
            assert d <= C.NOISE_Z_TOL, (per, step, b, d)
            assert np.array_equal(ref[b], O.philox_normal(per, s, step))
    print("fill_normal_ per-sample per=%d: worst |dz| %.3e" % (per, worst))


# ---- the update kernels with their own noise ---------------------------------------------------------------------------------------
def _inputs(shape, seed):
    g = C.rng(seed)
    return torch.randn(shape, generator=g), torch.randn(shape, generator=g)


def _bound(ref, sigma):
    """fp32 evaluation of the update (as in test_update_kernel_matches_float64_formula) plus sigma times the noise bound."""
    return 1e-6 * max(float(ref.abs().max()), 1.0) + abs(float(np.float32(sigma))) * C.NOISE_Z_TOL


@pytest.mark.parametrize("batched", [False, True])
def test_sampler_step_rng_is_the_formula_on_reference_noise(batched):
    """x0 = clamp(c_recip x - c_recipm1 eps), x <- coef1 x0 + coef2 x + sigma z with z = philox_normal in float64; sigma = 0 (the last
    step) adds nothing.  One stream on a tail size, or five per-sample streams."""
    shape, seeds = ((5, 3, 40, 56), HIGH_SEEDS) if batched else ((4001,), None)
    x, eps = _inputs(shape, 3 + batched)
    n = x.numel()
    worst = 0.0
    for seed, step, sigma in ((2 ** 63 + 5, 5, 0.25), (M64, 2 ** 32 - 1, 1.3), (1234, 7, 0.0)):
        c_recip, c_recipm1, coef1, coef2 = 1.7, 1.3, 0.4, 0.6
        xd = x.to(DEV)
        sampler_step_rng_(xd, eps.to(DEV), seed, step, c_recip, c_recipm1, coef1, coef2, sigma,
                          seeds=_keys(seeds) if batched else None)
        z = O.philox_normal(n, seed, step, per=n // 5 if batched else None, seeds=seeds).reshape(shape)
        f32 = lambda v: float(np.float32(v))
        x64, e64 = x.double(), eps.double()
        x0 = (f32(c_recip) * x64 - f32(c_recipm1) * e64).clamp(-1.0, 1.0)
        ref = f32(coef1) * x0 + f32(coef2) * x64 + f32(sigma) * torch.from_numpy(z)
        d = (xd.cpu().double() - ref).abs().max().item()
        worst = max(worst, d)
        assert d <= _bound(ref, sigma), (seed, step, sigma, d)
    print("sampler_step_rng_ batched=%s: worst |dx| %.3e" % (batched, worst))


FEW_CASES = {                           # the cases of test_update_kernel_matches_float64_formula that draw noise
    "ddim": (3.1, 2.9, FEWSTEP_CLIP, 0.83, 0.0, 0.41, 0.0, 0, 0.37),
    "ddim_noclip": (3.1, 2.9, 0, 0.83, 0.0, 0.41, 0.0, 0, 0.37),
    "clip_factored_noise": (1.9, 0.7, FEWSTEP_CLIP | FEWSTEP_FACTORED, 0.6, 0.1, 0.2, 0.0, 1, 0.5),
}


@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("case", sorted(FEW_CASES))
def test_fewstep_update_is_the_formula_on_reference_noise(case, batched):
    coef = FEW_CASES[case]
    c_recip, c_recipm1, flags, p, q, r, b1, store_m, sigma = coef
    shape, seeds = ((5, 3, 40, 56), HIGH_SEEDS) if batched else ((4001,), None)
    x, eps = _inputs(shape, 7 + batched)
    n = x.numel()
    worst = 0.0
    for seed, step in ((2 ** 63 + 5, 3), (M64, 2 ** 31 + 3)):
        xd, md = x.to(DEV), torch.zeros(shape, device=DEV)
        fewstep_update_(xd, eps.to(DEV), md if store_m else None, c_recip, c_recipm1, flags, p, q, r, b1, store_m, sigma,
                        seed=seed, step=step, seeds=_keys(seeds) if batched else None)
        z = torch.from_numpy(O.philox_normal(n, seed, step, per=n // 5 if batched else None, seeds=seeds).reshape(shape))
        ref, x0 = C.fewstep_formula(coef, x.double(), eps.double(), torch.zeros(shape, dtype=torch.float64), z)
        d = (xd.cpu().double() - ref).abs().max().item()
        worst = max(worst, d)
        assert d <= _bound(ref, sigma), (case, seed, step, d)
        if store_m:
            assert (md.cpu().double() - x0).abs().max().item() <= 1e-6 * max(x0.abs().max().item(), 1.0)
    print("fewstep_update_ %s batched=%s: worst |dx| %.3e" % (case, batched, worst))


# ---- the sampling loops ----------------------------------------------------------------------------------------------------------------
SMALL = UNetConfig(inner_channel=64, channel_mults=(1, 2, 4), res_blocks=1, attn_res=(32,), image_size=128)
SCHED8 = dict(schedule="linear", n_timestep=8, linear_start=1e-6, linear_end=0.4)


@pytest.fixture(scope="module")
def small_net():
    net, _ = C.build_net(SMALL)
    net.set_new_noise_schedule(SCHED8, DEV)
    return net


def _reset(net):
    net.noise_source, net.sample_seeds, net.noise_seed, net.noise_index, net.sampler = None, None, None, 0, None
    net.denoise_fn.set_graph(False)


def _reference_source(seeds, shift=0):
    """noise_source drawing philox_normal for loop counter k (+ ``shift``: a loop whose step numbering is off by ``shift``)."""
    def source(shape, device, k):
        n = int(np.prod(shape))
        z = O.philox_normal(n, 0, k + shift, per=n // len(seeds), seeds=seeds)
        return torch.from_numpy(z.reshape(shape)).float().to(device)
    return source


LOOPS = {   # name: (sampler, B, graph replay, per-sample streams of `seeds` (else one stream: noise_seed = seeds[0]), seeds)
    "p_sample_loop_noise_seed": ("ddpm", 1, False, False, [2 ** 32 + 7]),
    "p_sample_loop_sample_seeds": ("ddpm", 2, False, True, [2 ** 63 + 5, 2 ** 40 + 3]),
    "p_sample_loop_graph": ("ddpm", 1, True, True, [M64]),
    "ddim_eta1": ("ddim", 2, False, True, [0x9E3779B97F4A7C15, 77]),
    "ddim_eta1_graph": ("ddim", 1, True, False, [2 ** 63 + 5]),
    "dpm_solver++": ("dpm_solver++", 1, False, False, [2 ** 32 + 7]),
}


def _restore(net, sampler, cond, guide):
    with torch.no_grad():
        if sampler == "ddpm":
            return net.p_sample_loop(cond, False, kwargs={"guide": guide}).clone()
        steps = 5 if sampler == "ddim" else 6
        return net.fewstep_sample(cond, sampler, steps, eta=1.0, kwargs={"guide": guide}).clone()


@pytest.mark.parametrize("name", sorted(LOOPS))
def test_loop_draws_x_T_at_step_0_and_update_k_at_step_k(small_net, name):
    """A restoration on kernel noise equals the same restoration fed philox_normal(seed, k) for the loop's noise counter k (x_T: k = 0)
    within NOISE_LOOP_TOL / NOISE_LOOP_RMS_TOL; the same reference with k off by one lies far outside both."""
    net = small_net
    sampler, B, graph, per_sample, seeds = LOOPS[name]
    cond, guide, _ = (t.to(DEV) for t in map(torch.from_numpy, synth_inputs(B, 64, 64, seed=41)))
    try:
        net.denoise_fn.set_graph(graph)
        if per_sample:
            net.sample_seeds = seeds
        else:
            net.noise_seed = seeds[0]
        kern = _restore(net, sampler, cond, guide)
        if graph:
            assert torch.equal(_restore(net, sampler, cond, guide), kern)            # capture, then replay
        net.noise_source = _reference_source(seeds)
        ref = _restore(net, sampler, cond, guide)
        net.noise_source = _reference_source(seeds, shift=1)
        off = _restore(net, sampler, cond, guide)
    finally:
        _reset(net)
    m, mf = C.metrics(kern, ref), C.metrics(off, ref)
    print("%s: kernel vs reference noise max |dx| %.3e rel-rms %.3e; step off by one: max |dx| %.3e rel-rms %.3e"
          % (name, m["max_abs"], m["rel_rms"], mf["max_abs"], mf["rel_rms"]))
    assert not m["nan"] and m["max_abs"] <= C.NOISE_LOOP_TOL and m["rel_rms"] <= C.NOISE_LOOP_RMS_TOL, m
    assert mf["max_abs"] > 25 * C.NOISE_LOOP_TOL and mf["rel_rms"] > 50 * C.NOISE_LOOP_RMS_TOL, mf


@pytest.mark.parametrize("seed", [2 ** 63 + 5, -3])
def test_sample_seeds_key_equals_noise_seed_key(small_net, seed):
    """sample_seeds = [s] (per-sample key tensor, batched kernels) and noise_seed = s (the single-stream wrappers) are one stream:
    the restorations agree bit for bit, for seeds whose uint64 bit pattern has the top bit set."""
    net = small_net
    cond, guide, _ = (t.to(DEV) for t in map(torch.from_numpy, synth_inputs(1, 64, 64, seed=43)))
    try:
        for sampler in ("ddpm", "ddim"):
            net.sample_seeds = [seed]
            a = _restore(net, sampler, cond, guide)
            net.sample_seeds, net.noise_seed = None, seed
            b = _restore(net, sampler, cond, guide)
            net.noise_seed = None
            assert torch.equal(a, b), (sampler, seed)
    finally:
        _reset(net)
