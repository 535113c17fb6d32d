"""CPU evidence behind tests/test_uneven_batches_gpu.py: what the uneven batch (hip_checks.UNEVEN_LADDER), the small-scale
samples and the peaked softmax see that identically distributed unit-scale inputs do not.

A model of the conv kernels' algebra - bf16 operands, fp32 accumulation, ``rstd * acc - mean * rstd * Tg + Tb + bias``, swish,
bf16 store - is compared with the float64 reference of hip_checks.conv_case(uneven=True), per sample.  Without a fault it
meets the operator bounds on the uneven batch (the bounds are reachable from the numerics plan alone); with a neighbouring
sample's statistics, a wrong or missing epsilon, sample 0's statistics for everyone, a statistic that misses a tile or two
swapped statistics rows it exceeds them by two orders of magnitude - while the neighbour and epsilon faults pass every bound
on today's inputs.  The attention emulation's two summation orders agree within the ATT_EMU bounds on logits of up to 286,
the denoiser's emulation agrees with itself on the four value regimes of hip_checks.regime_inputs, and the time embedding's
sensitivity to one ulp of the level (the bound of the GPU test at levels above 1) is the one recorded in hip_checks.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import hip_checks as C
from oracle import ucdir_oracle as O
from ucdir_amd.spec import UNetConfig, unet_layers
from ucdir_amd.weights import synth_state_dict

OP_TOL = 4e-3          # single operator, bf16-representable inputs (tests/test_hip_gpu.py)
SID = UNetConfig(inner_channel=64, channel_mults=(1, 2, 4, 8, 8), res_blocks=2, attn_res=(16,), image_size=128)
SHAPES = {"64ch_64x80": (6, 64, 64, 64, 80), "128ch_20x24": (6, 128, 256, 20, 24)}
_cache = {}


def _stats(x, eps=1e-5, miss_tile=False):
    """Per-sample (mean, rstd) of x (B, C, H, W) from float64 sums, as the kernels form them from the accumulated (S, Q);
    ``miss_tile``: S lacks the contribution of the first 16 x 16 tile (all channels)."""
    n = x[0].numel()
    S, Q = x.double().sum(dim=(1, 2, 3)), x.double().pow(2).sum(dim=(1, 2, 3))
    if miss_tile:
        S = S - x[:, :, :16, :16].double().sum(dim=(1, 2, 3))
    mean = S / n
    var = (Q / n - mean * mean).clamp(min=0)
    return mean.float().view(-1, 1, 1, 1), (1.0 / torch.sqrt(var + eps)).float().view(-1, 1, 1, 1)


def _setup(name, uneven):
    """(x, parts of the kernel algebra, float64 reference) of one shape, computed once."""
    if (name, uneven) not in _cache:
        B, cin, cout, H, W = SHAPES[name]
        g = C.rng(11)
        z = torch.randn(B, cin, H, W, generator=g)
        x = C.uneven_batch(z, 0) if uneven else C.bfr(z * 1.3 + 0.6)
        w = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(1.5 / (cin * 9))
        b = torch.randn(cout, generator=g) * 0.1
        gamma, beta = 1 + 0.25 * torch.randn(cin, generator=g), 0.2 * torch.randn(cin, generator=g)
        wq = C.bfr(w * gamma.view(1, -1, 1, 1))
        acc = F.conv2d(x, wq, padding=1)
        tg = F.conv2d(torch.ones(1, cin, H, W), wq, padding=1)
        tb = F.conv2d(beta.view(1, cin, 1, 1).expand(1, cin, H, W).contiguous(), w, padding=1) + b.view(1, -1, 1, 1)
        ref = O.swish(F.conv2d(F.group_norm(x.double(), 1, gamma.double(), beta.double(), eps=1e-5), w.double(), b.double(), padding=1))
        _cache[name, uneven] = (x, acc, tg, tb, ref)
    return _cache[name, uneven]


def _model(parts, mean, rstd):
    """The stored output for per-sample (or per-sample-and-row) mean / rstd."""
    _, acc, tg, tb, _ = parts
    return C.bfr(O.swish(rstd * acc - mean * rstd * tg + tb))


def _faulty(parts, fault):
    x = parts[0]
    B, _, H, _ = x.shape
    mean, rstd = _stats(x)
    if fault == "neighbour_rows":          # the last two rows of every sample take the next sample's (mean, rstd)
        mean, rstd = mean.expand(B, 1, H, 1).clone(), rstd.expand(B, 1, H, 1).clone()
        mean[:, :, H - 2:], rstd[:, :, H - 2:] = mean.roll(-1, 0)[:, :, H - 2:].clone(), rstd.roll(-1, 0)[:, :, H - 2:].clone()
    elif fault == "no_eps":
        mean, rstd = _stats(x, eps=0.0)
    elif fault == "eps_1e-6":
        mean, rstd = _stats(x, eps=1e-6)
    elif fault == "sample0_stats":
        mean, rstd = mean[:1].expand(B, 1, 1, 1), rstd[:1].expand(B, 1, 1, 1)
    elif fault == "sum_misses_tile":
        mean, rstd = _stats(x, miss_tile=True)
    elif fault == "rows_swapped":          # statistics rows (0, 1), (2, 3), (4, 5) exchanged
        perm = [1, 0, 3, 2, 5, 4]
        mean, rstd = mean[perm], rstd[perm]
    else:
        raise ValueError(fault)
    return _model(parts, mean, rstd)


FAULTS = ["neighbour_rows", "no_eps", "eps_1e-6", "sample0_stats", "sum_misses_tile", "rows_swapped"]


@pytest.mark.parametrize("name", list(SHAPES))
def test_fault_free_model_meets_the_operator_bounds_on_the_uneven_batch(name):
    parts = _setup(name, True)
    x = parts[0]
    assert bool(torch.isfinite(x).all()) and float(x.abs().max()) < 64 and all(float(x[b].std()) > 0 for b in range(6))
    m = C.per_sample_metrics(_model(parts, *_stats(x)), parts[4])
    print(name, "fault-free, per sample:", m["per_sample"])
    assert C.op_ok(m, OP_TOL), m


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_modelled_faults_exceed_the_bound_on_the_uneven_batch(name, fault):
    parts = _setup(name, True)
    m = C.per_sample_metrics(_faulty(parts, fault), parts[4])
    print(name, fault, [round(p["rel_rms"], 4) for p in m["per_sample"]])
    assert m["rel_rms"] > 100 * OP_TOL, m


@pytest.mark.parametrize("fault", ["neighbour_rows", "no_eps", "eps_1e-6"])
def test_neighbour_and_epsilon_faults_pass_every_bound_on_todays_inputs(fault):
    """The gap: on identically distributed unit-scale samples (conv_case's default draw) at 6 x 64 x 64 x 80 a neighbour's
    statistics on two rows, a missing epsilon and epsilon 1e-6 stay under the global, the tile-local and the element bound.
    If the default inputs change so that this fails, the gap is closed there: update this assertion, do not drop it."""
    parts = _setup("64ch_64x80", False)
    good = C.metrics(_model(parts, *_stats(parts[0])), parts[4])
    m = C.metrics(_faulty(parts, fault), parts[4])
    print(fault, "on today's inputs:", {k: m[k] for k in ("rel_rms", "tile_max", "elem_max")}, " fault-free:", good["rel_rms"])
    assert C.op_ok(good, OP_TOL) and C.op_ok(m, OP_TOL), (good, m)


# ---- attention: the peaked softmax ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["flash_bf16", "flash_fp16", "scores"])
@pytest.mark.parametrize("factor", [2, 4])
@pytest.mark.parametrize("shape", [(2, 128, 8, 8), (1, 256, 36, 36)], ids=["C128_N64", "C256_N1296"])
def test_attention_emulation_agrees_with_itself_on_peaked_softmax(shape, factor, path):
    """q and k rows of the qkv weight times 2 | 4 (logits times 4 | 16), attention_emu_case's random inputs without a further
    offset: the reference's largest |logit| is >= 60 | 250 and the mean largest probability >= 0.8, and the emulation's two
    summation orders (torch fp32, float64 sums) stay within the ATT_EMU bounds - the regime says something about a kernel.
    Worst over these cases: rel-RMS 2.8e-4, tile 1.0e-3, element 2.9e-2."""
    x, sd = C.attention_inputs(*shape, seed=0, logit_scale=float(factor))
    st = C.attention_logit_stats(x, sd)
    m = C.attention_emu_self(x, sd, fp16=path == "flash_fp16", scores=path == "scores")
    print(shape, factor, path, st, {k: m[k] for k in ("rel_rms", "tile_max", "elem_max")})
    assert st["max_logit"] >= (60 if factor == 2 else 250) and st["mean_pmax"] >= 0.8, st
    assert not m["nan"] and m["rel_rms"] < C.ATT_EMU_TOL and m["tile_max"] < C.ATT_EMU_TILE_TOL and m["elem_max"] < C.ATT_EMU_ELEM_TOL, m


GPU_ATT_SHAPES = [(3, 512, 4, 4), (3, 512, 7, 9), (3, 512, 8, 8), (3, 512, 5, 13), (3, 512, 8, 16), (3, 256, 36, 36)]


@pytest.mark.parametrize("factor", [2, 4])
@pytest.mark.parametrize("shape", GPU_ATT_SHAPES, ids=lambda s: f"c{s[1]}_n{s[2] * s[3]}")
def test_attention_emulation_agrees_with_itself_on_the_gpu_cases(shape, factor):
    """The cases of test_uneven_batches_gpu.py::test_attention_peaked_softmax_on_an_uneven_batch (B = 3, x on the ladder's
    entries 5, 0, 1: hip_checks.ATT_LADDER_PHASE): the emulation's two summation orders meet the ATT_EMU bounds on every sample,
    every type and both paths."""
    x, sd = C.attention_inputs(*shape, seed=40, uneven=True, logit_scale=float(factor))
    for path in ("flash_bf16", "flash_fp16", "scores"):
        m = C.attention_emu_self(x, sd, fp16=path == "flash_fp16", scores=path == "scores")
        print(shape, factor, path, [(f"{p['rel_rms']:.2e}", f"{p['tile_max']:.2e}", f"{p['elem_max']:.2e}") for p in m["per_sample"]])
        assert not m["nan"] and m["rel_rms"] < C.ATT_EMU_TOL and m["tile_max"] < C.ATT_EMU_TILE_TOL and m["elem_max"] < C.ATT_EMU_ELEM_TOL, m


def test_attention_branch_metric_says_nothing_on_the_large_residual_samples():
    """Why the attention batch leaves out the ladder's entries 2 and 4: with x = 8 z - 12 (third sample at phase 0) the stored
    sum x + branch reaches 45 and one bf16 step of it is 0.25, 0.12 of the branch's RMS - the emulation's own two summation orders
    then differ by 3.8e-3 in a tile and 0.122 in an element (C = 256, N = 1296, fp16, factor 2), beyond ATT_EMU_TILE_TOL and
    ATT_EMU_ELEM_TOL, while the same case on the entries 5, 0, 1 is within them (the test above)."""
    x, sd = C.attention_inputs(3, 256, 36, 36, seed=40, uneven=True, logit_scale=2.0, phase=0)
    m = C.attention_emu_self(x, sd, fp16=True)
    print(m["per_sample"])
    assert float(x[2].abs().max()) > 32
    s8 = m["per_sample"][2]
    assert s8["tile_max"] > C.ATT_EMU_TILE_TOL and s8["elem_max"] > C.ATT_EMU_ELEM_TOL, s8
    assert all(p["tile_max"] < C.ATT_EMU_TILE_TOL and p["elem_max"] < C.ATT_EMU_ELEM_TOL for p in m["per_sample"][:2]), m["per_sample"]


# ---- the whole denoiser on four value regimes -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sid_sd():
    return O.to_torch_sd(synth_state_dict(SID, 0))


def test_emulation_agrees_with_itself_on_the_value_regimes(sid_sd):
    """hip_checks.regime_inputs (dark, synthetic, saturated, flat) at 64 x 96, padded as forward_split pads them: the
    emulation's two summation orders meet the EMU bounds on every layer, so the GPU test may hold the HIP path to them.
    Worst: rel-RMS 1.4e-4, tile 2.9e-4, element 2.5e-2."""
    cond, guide, x_t = C.regime_inputs(64, 96, seed=7)
    assert float(cond[0].max()) < -0.7 and set(cond[2].unique().tolist()) == {-1.0, 1.0} and float(cond[3].std()) == 0.0
    inp = C.pad_to_compute(cond, guide, x_t)
    out = C.emu_self_comparison(sid_sd, SID, 4, 96, 128, list(C.REGIME_LEVELS), 0, inputs=inp)
    assert len(out) == 36 + 27 + 1, len(out)
    for f in ("rel_rms", "tile_max", "elem_max"):
        k = max(out, key=lambda k: out[k][f])
        print(f"worst {f}: {out[k][f]:.3e} ({k})")
    for k, m in out.items():
        assert C.emu_layer_ok(m), (k, m)


def test_time_embedding_sensitivity_is_the_recorded_one(sid_sd):
    """hip_checks.TIME_ULP_CHANGE: what one ulp of the level moves the block weights by, in the float64 oracle, at the levels of
    the GPU test; and the fp32 oracle itself stays within the GPU test's bound at every level.  A CPU model
    of time_mlp_kernel's own fp32 algebra and summation order meets 4x the one-ulp change at 49, 250.3 and 999 but not at 3.7, where
    that is 4.3e-7, under the noise of the fp32 sums at any level: there the bound is 1.5x the model's value (hip_checks.time_bound)."""
    blocks = [Ld.name for Ld in unet_layers(SID) if Ld.kind == "block"]
    lv = list(C.TIME_LEVELS)
    ch = C.time_ulp_change(sid_sd, lv, blocks)
    temb = O.noise_embedding(sid_sd, torch.tensor(lv).view(-1, 1), "denoise_fn.")
    f32 = torch.stack([O.time_weights(sid_sd, "denoise_fn." + n + ".res_block.", temb) for n in blocks])
    err = C.time_rel_err(f32, C.time_weights_f64(sid_sd, lv, blocks))
    print("one-ulp change per level:", ch.tolist(), " fp32 oracle vs float64:", err.tolist())
    assert len(blocks) == 27
    ref = C.time_weights_f64(sid_sd, lv, blocks)
    model = C.time_rel_err(torch.stack([C.time_mlp_fp32_model(sid_sd, l, blocks) for l in lv], 1), ref)
    print("the kernel's fp32 algebra and order on the CPU vs float64:", model.tolist())
    for i, l in enumerate(lv):
        if l > 1:
            assert abs(float(ch[i]) / C.TIME_ULP_CHANGE[l] - 1) < 0.02, (l, float(ch[i]))
        assert float(err[i]) < C.time_bound(l), (l, float(err[i]))
        if l in C.TIME_FP32_MODEL_ERR:         # the plan itself misses 4x the one-ulp change here, and only here
            assert 4 * C.TIME_ULP_CHANGE[l] < float(model[i]) and abs(float(model[i]) / C.TIME_FP32_MODEL_ERR[l] - 1) < 0.02, (l, float(model[i]))
        else:
            assert float(model[i]) < (2e-5 if l <= 1 else 4 * C.TIME_ULP_CHANGE[l]), (l, float(model[i]))
