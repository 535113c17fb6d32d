"""Parity checks of the HIP path against the CPU oracle (shared by pytest -m gpu and tools/gpu_check.py).

Every function returns a dict of error metrics; thresholds live in the tests.
Tolerances (stated once): the HIP path computes convolutions / attention with bf16 operands and
fp32 accumulation and stores activations in bf16, so vs the fp32 oracle we expect
  * single operator on bf16-representable inputs : rel-RMS <~ 3e-3 (weight + output rounding), bound OP_TOL = 4e-3
  * full 61-GroupNorm-deep forward               : rel-RMS 1.2e-2 (small configuration) / 1.43-1.51e-2 (full SID) measured; the oracle's
    bf16-emulation mode (oracle.dy3h_naive_forward_emu: rounding where the kernels round) sits at 1.47-1.50e-2 from the fp32 oracle on the
    same inputs, i.e. the whole difference IS the numerics plan; bound FWD_TOL = 1.7e-2 (tests/test_hip_gpu.py)
  * one layer against the emulation on the HIP path's own input activations (layerwise_emu_case): <= 6.7e-4 measured, bound 2e-3
Every metric above is a global rel-RMS, which dilutes an error confined to one tile, strip column or sample-boundary row of
a large layer.  metrics() therefore also reports, for 4-D tensors, ``tile_max`` (the worst RMS error of one block of
1 sample x 64 channels x 32 x 32 positions, relative to the GLOBAL reference RMS) and ``elem_max`` (the worst single element,
same scale); tests/test_tile_metric_cpu.py shows which modelled faults each bound catches.
"""
import ctypes
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ucdir_oracle as O
from ucdir_amd import lib as ulib
from ucdir_amd.spec import UNetConfig
from ucdir_amd.weights import synth_inputs, synth_state_dict

DEV = "cuda"

EMU_LAYER_TOL = 2e-3   # one layer of the HIP path against the oracle's bf16-emulation mode ON THE SAME INPUTS (teacher forcing): what is left is
                       # fp32 summation order and single bf16 rounding flips.  Measured (tools/_emu_probe.py): worst layer 6.7e-4 (full SID, B = 1),
                       # 4.4e-4 (B = 4), 8.9e-4 (small configuration) - the attention blocks of the 18^2 / 36^2 levels; everything else <= 4e-4.
                       # The val shapes (tests/test_val_shapes_gpu.py: 416^2, non-square, akgm_ws64's limits, 416 x 1664): worst 5.90e-4
                       # (mid.0, B = 1 at 416^2).  The smallest shapes (tests/test_small_denoiser_gpu.py: 32^2 ... 64 x 32, 33^2 ... 63 x 40,
                       # B = 64 at 33^2; a GroupNorm over 2k - 8k values): worst 1.38e-3 (mid.0, naiveforward 3 x 32 x 64).  The four value
                       # regimes (tests/test_uneven_batches_gpu.py: dark, synthetic, saturated, flat; B = 4 at 64 x 96): worst 1.03e-3 (mid.0)
TILE = (64, 32, 32)    # (channels, rows, columns) of one tile_max block; one sample per block
# tile-local bounds (metrics() keys tile_max / elem_max) and the attention-vs-emulation bounds: each about 1.5x the worst value
# measured on the MI355X over every case that asserts it; tests/test_tile_metric_cpu.py shows the modelled faults exceed them
OP_TILE_TOL = 4e-3     # single operator vs torch: worst 2.61e-3 (test_conv_stream_k_with_res_conv[level4_ksplit], the res_conv output); planes
                       # below one tile (tests/test_small_planes_gpu.py): 3.43e-3 (conv_sk 4-wave kind, B = 64 on 2 x 2, a 256-element block;
                       # rel-RMS <= 2.47e-3), AKGM 2.77e-3; the tile cover (tests/test_tile_cover_gpu.py): conv 2.78e-3, AKGM 2.55e-3; the
                       # uneven batches (tests/test_uneven_batches_gpu.py, every figure PER SAMPLE, relative to that sample's own RMS): conv
                       # with fold rel-RMS 2.41e-3, tile 2.51e-3; conv1 of the fused res_conv launches 3.17e-3, 3.20e-3 (tap10_192; others
                       # <= 2.5e-3), their res_conv 2.47e-3, 2.49e-3; Downsample / Upsample 2.41e-3, 2.46e-3; AKGM 2.30e-3, 2.47e-3
OP_ELEM_TOL = 5.5e-2   # ... worst 3.65e-2 (test_akgm_block_kernel_at_narrow_groups[cg8_th8]): one bf16 step of a large output; planes below one
                       # tile 3.18e-2, the tile cover 3.18e-2; the uneven batches, per sample: conv 2.95e-2, res_conv 1.83e-2, resamplers
                       # 1.67e-2, AKGM 3.18e-2.  Their statistics per sample and column (stats_per_sample, bound 1e-3): sums <= 2.3e-5 of
                       # n rms_b, sums of squares <= 1.44e-4 (conv_sk kind 1, 5 x 12 x 18: 55 k elements per sample)
EMU_TILE_TOL = 1.3e-3  # one layer vs the emulation: worst 8.84e-4 (full SID B = 1, an attention block at 36^2); B = 32: 6.3e-4,
                       # 1024^2 windows: 4.3e-4, fp16 attention windows: 4.2e-4 (tests/test_layerwise_gpu.py); the val shapes: 6.34e-4
                       # (ups.5, B = 4 at 288 x 800); the smallest shapes, blocks of >= EMU_TILE_MIN_BLOCK elements: 1.26e-3 (downs.11, a 4096-element
                       # block of forward_split 2 x 63 x 40; smaller blocks: EMU_TILE_MIN_BLOCK), while a layer with its last 32 columns one row down (shift_last_strip) gives >= 1.41;
                       # the four value regimes: 1.15e-3 (mid.0, the flat sample)
EMU_ELEM_TOL = 6.5e-2  # ... one element (asserted by tests/test_predictor_gpu.py): worst 4.19e-2 (conv8_2, B = 16 at 384^2); the denoiser's smallest
                       # shapes: 5.54e-2 (mid.0:h1, naiveforward 3 x 32 x 64: one bf16 step of an output of ~10 RMS); the predictor's
                       # layers against its emulation: rel-RMS <= 1.04e-4, tile_max <= 3.46e-4 (all shapes; no GroupNorm to amplify rounding).
                       # The four value regimes: denoiser 4.09e-2 (downs.7:h1, the dark sample); predictor rel-RMS <= 1.31e-4, tile_max
                       # <= 3.64e-4, element <= 2.02e-2 (the dark image; the flat one 2.6e-5, 6.7e-5, 1.2e-2)
PRED_TILE_TOL = 1e-2   # the whole predictor vs the fp32 oracle (test_predictor, 3 channels x 32 x 32 blocks): worst 6.79e-3 (B = 2, 64 x 96)
PRED_ELEM_TOL = 6e-2   # ... worst 3.93e-2 (1 x 256^2)
ATT_EMU_TOL = 2.5e-3   # attention vs self_attention_emu, rel-RMS of the branch: worst 1.62e-3 (C = 384, N = 4096, flash); N = 16 ... 64
                       # (tests/test_small_planes_gpu.py): 8.34e-4 (C = 512, N = 63, materialised, masking inputs); logits of up to 322 on an
                       # uneven batch (tests/test_uneven_batches_gpu.py, per sample): 1.30e-3 (C = 512, N = 16, materialised, factor 4)
ATT_EMU_TILE_TOL = 3e-3  # ... worst 1.98e-3 (C = 512, N = 1296, B = 2, flash); N = 16 ... 64: 1.38e-3 (C = 512, N = 32, B = 3, materialised);
                         # peaked softmax, uneven batch: 1.48e-3 (C = 512, N = 16, materialised, factor 4)
ATT_EMU_ELEM_TOL = 6e-2  # ... worst 3.90e-2 (C = 512, N = 16384, flash); N = 16 ... 64: 2.32e-2 (C = 512, N = 63, flash, masking inputs);
                         # peaked softmax, uneven batch: 3.05e-2 (C = 256, N = 1296, flash, factor 2); the rescale case (95 % of the mass on
                         # the last key, jump of the running maximum 124): rel-RMS <= 3.8e-5, element <= 7.0e-3 on all three paths
# the in-kernel Philox noise against oracle.philox_normal in float64 (tests/test_noise_stream_gpu.py); the kernel's __logf, v_sin_f32 and
# v_cos_f32 are approximations, so z agrees to a few fp32 ulps of |z| <= 5.77.  tests/test_noise_stream_cpu.py shows every modelled
# fault of the stream's statement exceeds NOISE_Z_TOL by orders of magnitude
NOISE_Z_TOL = 1.2e-6   # max |dz| over every element drawn: worst 7.91e-7 (fill_normal_, seed 1234; at |z| ~ 4.4); per-sample streams
                       # 4.57e-7; the elements with |z| < 1 are within 7.7e-7 relative
NOISE_LOOP_TOL = 4e-2  # a T = 8 / DDIM / DPM-Solver++ restoration (small configuration) on kernel noise against the same restoration fed
                       # philox_normal: max |dx| of the result, worst 2.67e-2 (p_sample_loop, one stream).  The bf16 forward turns the
                       # ulp-level difference in x_t into another realisation of its rounding noise; the graph-replayed DDIM run stays at 8.9e-7
NOISE_LOOP_RMS_TOL = 8e-3  # ... rel-RMS, worst 5.20e-3 (DDIM eta = 1, B = 2).  Noise counters off by one step: max |dx| >= 2.0, rel-RMS >= 0.76


def bfr(t):
    return t.to(torch.bfloat16).float()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else ctypes.c_void_p(0)


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def tile_metrics(d, rms):
    """Tile-local view of the difference ``d`` (B, C, H, W) against a reference of global RMS ``rms``: ``tile_max`` = max over
    blocks of one sample x TILE of sqrt(mean(d^2 over the block)) / rms (ragged edge blocks divide by their true element
    count), ``tile_at`` = (sample, channel, row, column) of that block's first element, ``elem_max`` = max |d| / rms,
    ``block`` = the elements of the tensor's largest block, min(C, 64) x min(H, 32) x min(W, 32)."""
    B, Cc, H, W = d.shape
    tc, th, tw = TILE
    nc, nh, nw = -(-Cc // tc), -(-H // th), -(-W // tw)
    sums = torch.zeros(B, nc, nh, nw, dtype=torch.float64)
    for b in range(B):                       # one sample at a time: a 1024^2 layer is 270 MB per sample
        for ci in range(nc):
            blk = d[b, ci * tc:(ci + 1) * tc].pow(2)
            if nh * th != H or nw * tw != W:
                blk = F.pad(blk, (0, nw * tw - W, 0, nh * th - H))
            sums[b, ci] = blk.reshape(blk.shape[0], nh, th, nw, tw).sum(dim=(0, 2, 4)).double()
    cnt = lambda n, t, k: torch.tensor([min(t, n - i * t) for i in range(k)], dtype=torch.float64)
    count = cnt(Cc, tc, nc).view(nc, 1, 1) * cnt(H, th, nh).view(1, nh, 1) * cnt(W, tw, nw).view(1, 1, nw)
    tile = (sums / count).sqrt() / max(rms, 1e-12)
    i = int(tile.flatten().argmax())
    b, r = divmod(i, nc * nh * nw)
    ci, r = divmod(r, nh * nw)
    hi, wi = divmod(r, nw)
    return {"tile_max": float(tile.flatten()[i]), "tile_at": (b, ci * tc, hi * th, wi * tw),
            "elem_max": float(d.abs().max()) / max(rms, 1e-12), "block": min(Cc, tc) * min(H, th) * min(W, tw)}


def metrics(got, ref):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    d = got - ref
    rms = ref.pow(2).mean().sqrt().item()
    m = {"rel_rms": (d.pow(2).mean().sqrt().item() / max(rms, 1e-12)), "max_abs": d.abs().max().item(),
         "ref_rms": rms, "nan": bool(torch.isnan(got).any())}
    if d.dim() == 4:
        m.update(tile_metrics(d, rms))
    return m


def profile_keys(L, fn):
    """Run fn() with the library's per-launch event profiler on and return {key: launches} of the kernels it dispatched."""
    ulib.check(L.ucdir_profile_enable(1))
    try:
        r = fn()
    finally:
        ulib.check(L.ucdir_profile_enable(0))
    cap = 64
    keys, ln = (ctypes.c_int32 * cap)(), (ctypes.c_int32 * cap)()
    ms, fl, by = (ctypes.c_double * cap)(), (ctypes.c_double * cap)(), (ctypes.c_double * cap)()
    nr = ctypes.c_int32(0)
    ulib.check(L.ucdir_profile_read(cap, keys, ln, ms, fl, by, ctypes.byref(nr), _st()))
    return r, {int(keys[i]): int(ln[i]) for i in range(nr.value)}


class debug_flags:
    """Context: ucdir_debug_flag settings for the launches inside it (convsk, skmix, persist_grid, splitk, flash), put back to
    the engine's own choice (persist_grid: 0, the others: -1) on the way out."""

    def __init__(self, **flags):
        self.flags = flags

    def __enter__(self):
        from ucdir_amd.ucdir import debug_flag       # (a DY3h that holds a plan prepares and plans again under the flags)
        for k, v in self.flags.items():
            debug_flag(k, v)

    def __exit__(self, *exc):
        from ucdir_amd.ucdir import debug_flag
        for k in self.flags:
            debug_flag(k, 0 if k == "persist_grid" else -1)


def rng(seed):
    return torch.Generator().manual_seed(seed)


# The uneven batch (tests/test_uneven_batches_*.py): sample b of an activation that feeds a GroupNorm is z * s + o with (s, o) =
# UNEVEN_LADDER[(b + phase) % 6] - unit scale, 2^-8 and 2^-11 (where GroupNorm's epsilon 1e-5 is 0.7 and 42 times the
# variance), scale 8 with a mean of -12, means of 8 and -1.5 standard deviations.  Two neighbouring samples differ in mean or rstd
# by orders of magnitude, so a tile, range or list entry that takes the neighbour's statistics is off by more than the output
# itself.  Largest magnitude ~45; sums of squares <= 208 per element, 1e9 for the largest tensor the tests run, against the
# +-8.8e12 range of the fixed-point accumulators (csrc/common.h).
UNEVEN_LADDER = ((1.0, 0.6), (2.0 ** -8, 0.6 * 2.0 ** -8), (8.0, -12.0), (2.0 ** -11, 0.0), (1.0, 8.0), (0.25, -1.5))
UNEVEN_ATT_SCALE = (0.25, 4.0, 1.0, 2.0, 0.5)     # akgm_case(uneven=True): sample b's ``att`` is scaled by entry b % 5


def uneven_batch(z, phase=0):
    """z (B, ...) ~ N(0, 1) -> bf16-representable z * s_b + o_b along UNEVEN_LADDER, starting at ``phase``."""
    B = z.shape[0]
    so = torch.tensor([UNEVEN_LADDER[(b + phase) % len(UNEVEN_LADDER)] for b in range(B)], dtype=torch.float32)
    shape = (B,) + (1,) * (z.dim() - 1)
    return bfr(z * so[:, 0].view(shape) + so[:, 1].view(shape))


def per_sample_metrics(got, ref):
    """metrics() of every sample against ITS OWN reference (the error relative to that sample's reference RMS, so that a sample
    at scale 2^-11 of an operator without GroupNorm does not vanish under one at scale 8): the worst rel_rms, tile_max,
    elem_max and max_abs over the batch under the usual keys, ``ref_rms`` = the smallest, ``per_sample`` = the list."""
    ms = [metrics(got[b:b + 1], ref[b:b + 1]) for b in range(got.shape[0])]
    m = {k: max(x[k] for x in ms) for k in ("rel_rms", "max_abs", "tile_max", "elem_max") if k in ms[0]}
    m["nan"] = any(x["nan"] for x in ms) or not bool(torch.isfinite(got).all())
    m["ref_rms"] = min(x["ref_rms"] for x in ms)
    m["per_sample"] = [{k: x[k] for k in ("rel_rms", "tile_max", "elem_max", "ref_rms") if k in x} for x in ms]
    return m


def stats_per_sample(stats, out):
    """The (B, 2) table of (sum S, sum of squares Q) a launch accumulated for its output against float64 sums of the output
    it stored, per sample and per column: ``stats_s`` = worst |S - S_ref| / (n rms_b) (n elements per sample, rms_b the RMS of
    that sample's stored output: a sum is compared with the scale of what it sums, not with Q), ``stats_q`` = worst
    |Q - Q_ref| / Q_ref.  Bound 1e-3 each (the bound of stats_rel).  The accumulators resolve 2^-20 per atomic add, i.e. a
    launch of k adds is off by at most k x 2^-21.  No output of the uneven-batch tests is small enough for that to matter: every
    operator adds a bias of RMS 0.1 or a residual, so even the 2^-11 sample of a resampler has an output RMS >= 0.09 (measured
    0.0917), and with n >= 25,600 elements per sample Q_ref >= 215 and n rms_b >= 2,300; k = 10^4 adds (more than any of these
    launches has workgroups) would move Q by 5e-3 absolute = 2.2e-5 of the smallest Q_ref, S by 2e-6 of the smallest n rms_b.
    So no case needs a bound derived from the resolution, and none has one."""
    o = out.detach().double().cpu()
    n = o[0].numel()
    S, Q = o.sum(dim=(1, 2, 3)).numpy(), o.pow(2).sum(dim=(1, 2, 3)).numpy()
    es = np.abs(stats[:, 0] - S) / (n * np.sqrt(Q / n))
    eq = np.abs(stats[:, 1] - Q) / Q
    return {"stats_s": float(es.max()), "stats_q": float(eq.max()), "stats_s_all": es.tolist(), "stats_q_all": eq.tolist()}


def uneven_ok(m, stats=True):
    """The bounds of an uneven-batch operator case: op_ok per sample (m from per_sample_metrics) and the per-column statistics."""
    return op_ok(m) and (not stats or (m["stats_s"] < 1e-3 and m["stats_q"] < 1e-3))


def conv_case(B, H, W, c0, c1, cout, ksize, mode, gn, act, residual, seed=0, uneven=False):
    """ucdir_op_conv vs torch on bf16-representable inputs.  ``act``: 0 none, 1 swish, 2 LeakyReLU(0.2) (the predictor's
    epilogue); True / False mean 1 / 0.  ``neg_frac``: the share of negative pre-activations in the reference.
    ``uneven``: x0 and x1 along UNEVEN_LADDER (x1 three entries on), a float64 reference, metrics per sample
    (per_sample_metrics) and the statistics per sample and column against the stored output (stats_per_sample)."""
    act = int(act)
    assert act in (0, 1, 2), act
    L = ulib.load()
    g = rng(seed)
    cin = c0 + c1
    z0 = torch.randn(B, c0, H, W, generator=g)
    x0 = uneven_batch(z0, 0) if uneven else bfr(z0 * 1.3 + 0.6)
    z1 = torch.randn(B, c1, H, W, generator=g) if c1 else None
    x1 = (uneven_batch(z1, 3) if uneven else bfr(z1 * 0.7 - 0.4)) if c1 else None
    w = torch.randn(cout, cin, ksize, ksize, generator=g) * math.sqrt(1.5 / (cin * ksize * ksize))
    b = torch.randn(cout, generator=g) * 0.1
    gamma = (1 + 0.25 * torch.randn(cin, generator=g)) if gn else None
    beta = (0.2 * torch.randn(cin, generator=g)) if gn else None
    Ho, Wo = (H // 2, W // 2) if mode == 1 else ((2 * H, 2 * W) if mode == 2 else (H, W))
    res = bfr(torch.randn(B, cout, Ho, Wo, generator=g)) if residual else None
    # reference (uneven: in float64)
    r_ = (lambda t: t.double()) if uneven else (lambda t: t)
    x = r_(torch.cat([x0, x1], 1) if c1 else x0)
    h = F.group_norm(x, 1, r_(gamma), r_(beta), eps=1e-5) if gn else x
    if mode == 1:
        y = F.conv2d(h, r_(w), r_(b), stride=2, padding=1)
    elif mode == 2:
        y = F.conv2d(F.interpolate(h, scale_factor=2, mode="nearest"), r_(w), r_(b), padding=1)
    else:
        y = F.conv2d(h, r_(w), r_(b), padding=ksize // 2)
    neg_frac = float((y < 0).float().mean())
    if act == 1:
        y = O.swish(y)
    elif act == 2:
        y = torch.max(0.2 * y, y)
    if residual:
        y = y + r_(res)
    # device
    dx0, dx1 = x0.to(DEV), (x1.to(DEV) if c1 else None)
    dres = res.to(DEV) if residual else None
    dy = torch.empty(B, cout, Ho, Wo, device=DEV)
    stats = np.zeros((B, 2), dtype=np.float64)
    wn, bn = w.numpy().copy(), b.numpy().copy()
    gn_, bt_ = (gamma.numpy().copy(), beta.numpy().copy()) if gn else (None, None)
    ulib.check(L.ucdir_op_conv(_p(dx0), c0, _p(dx1), c1, B, H, W, _hp(wn), _hp(bn), _hp(gn_), _hp(bt_), cout, ksize,
                               mode, act, _p(dres), _p(dy), _hp(stats), _st()))
    torch.cuda.synchronize()
    m = per_sample_metrics(dy, y) if uneven else metrics(dy, y)
    m["neg_frac"] = neg_frac
    ref_stats = np.stack([y.double().sum(dim=(1, 2, 3)).numpy(), y.double().pow(2).sum(dim=(1, 2, 3)).numpy()], 1)
    m["stats_rel"] = float(np.abs(stats - ref_stats).max() / np.abs(ref_stats).max())
    if uneven:
        m.update(stats_per_sample(stats, dy))
    # border vs interior error (a wrong GroupNorm border class shows up here)
    d = (dy.cpu() - y).abs()
    m["max_abs_border"] = float(torch.cat([d[..., 0, :].flatten(), d[..., -1, :].flatten(), d[..., :, 0].flatten(),
                                           d[..., :, -1].flatten()]).max())
    return m


def conv_res_case(B, H, W, c0, c1, cout, seed=0, uneven=False):
    """ucdir_op_conv_res (conv1 with GroupNorm fold + swish, and the block's 1x1 res_conv, one launch) vs torch.
    ``uneven``: as conv_case; the res_conv output (no GroupNorm) too is measured per sample."""
    L = ulib.load()
    g = rng(seed)
    cin = c0 + c1
    z0 = torch.randn(B, c0, H, W, generator=g)
    x0 = uneven_batch(z0, 0) if uneven else bfr(z0 * 1.3 + 0.6)
    z1 = torch.randn(B, c1, H, W, generator=g) if c1 else None
    x1 = (uneven_batch(z1, 3) if uneven else bfr(z1 * 0.7 - 0.4)) if c1 else None
    w = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(1.5 / (cin * 9))
    b = torch.randn(cout, generator=g) * 0.1
    wr = torch.randn(cout, cin, 1, 1, generator=g) * math.sqrt(1.5 / cin)
    br = torch.randn(cout, generator=g) * 0.1
    gamma = 1 + 0.25 * torch.randn(cin, generator=g)
    beta = 0.2 * torch.randn(cin, generator=g)
    r_ = (lambda t: t.double()) if uneven else (lambda t: t)
    x = r_(torch.cat([x0, x1], 1) if c1 else x0)
    y = O.swish(F.conv2d(F.group_norm(x, 1, r_(gamma), r_(beta), eps=1e-5), r_(w), r_(b), padding=1))
    yr = F.conv2d(x, r_(wr), r_(br))
    dx0, dx1 = x0.to(DEV), (x1.to(DEV) if c1 else None)
    dy = torch.empty(B, cout, H, W, device=DEV); dyr = torch.empty(B, cout, H, W, device=DEV)
    stats = np.zeros((B, 2), dtype=np.float64)
    ulib.check(L.ucdir_op_conv_res(_p(dx0), c0, _p(dx1), c1, B, H, W, _hp(w.numpy().copy()), _hp(b.numpy().copy()),
                                   _hp(gamma.numpy().copy()), _hp(beta.numpy().copy()), _hp(wr.numpy().copy()), _hp(br.numpy().copy()),
                                   cout, 1, _p(dy), _p(dyr), _hp(stats), _st()))
    torch.cuda.synchronize()
    m = per_sample_metrics(dy, y) if uneven else metrics(dy, y)
    mr = per_sample_metrics(dyr, yr) if uneven else metrics(dyr, yr)
    m["res_rel_rms"], m["res_nan"] = mr["rel_rms"], mr["nan"]
    m["res_tile_max"], m["res_elem_max"] = mr["tile_max"], mr["elem_max"]
    got = dy.double().cpu()
    st_ref = np.stack([got.sum(dim=(1, 2, 3)).numpy(), got.pow(2).sum(dim=(1, 2, 3)).numpy()], 1)
    m["stats_rel"] = float(np.abs(stats - st_ref).max() / np.abs(st_ref).max())
    if uneven:
        m.update(stats_per_sample(stats, dy))
    d = (dy.cpu() - y).abs()
    m["max_abs_border"] = float(torch.cat([d[..., 0, :].flatten(), d[..., -1, :].flatten(), d[..., :, 0].flatten(),
                                           d[..., :, -1].flatten()]).max())
    return m


def akgm_case(B, C, H, W, seed=0, uneven=False):
    """ucdir_op_akgm vs torch.  ``uneven``: ``h`` along UNEVEN_LADDER and sample b's ``att`` scaled by UNEVEN_ATT_SCALE[b % 5]
    (a neighbour's att or fold table shows), a float64 reference, metrics and statistics per sample."""
    L = ulib.load()
    g = rng(seed)
    zh = torch.randn(B, C, H, W, generator=g)
    h = uneven_batch(zh, 0) if uneven else bfr(zh.abs() * 0.8 - 0.2)
    att = torch.randn(B, 8, H, W, generator=g) * 0.5
    if uneven:
        att = att * torch.tensor([UNEVEN_ATT_SCALE[b % len(UNEVEN_ATT_SCALE)] for b in range(B)]).view(B, 1, 1, 1)
    res = bfr(torch.randn(B, C, H, W, generator=g))
    wsp = torch.randn(8 * C, C // 8, 3, 3, generator=g) * math.sqrt(1.5 / (9 * C // 8))
    bsp = torch.randn(8 * C, generator=g) * 0.1
    gamma = 1 + 0.25 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    r_ = (lambda t: t.double()) if uneven else (lambda t: t)
    hn = F.group_norm(r_(h), 1, r_(gamma), r_(beta), eps=1e-5)
    hset = F.conv2d(hn, r_(wsp), r_(bsp), padding=1, groups=8).view(B, C, 8, H, W)
    y = O.swish((hset * r_(att).unsqueeze(1)).sum(2)) + r_(res)
    dy = torch.empty(B, C, H, W, device=DEV)
    dh, datt, dres = h.to(DEV), att.to(DEV), res.to(DEV)      # keep alive: raw pointers cross the ABI
    stats = np.zeros((B, 2), dtype=np.float64)
    ulib.check(L.ucdir_op_akgm(_p(dh), _p(datt), _p(dres), B, C, H, W, _hp(wsp.numpy().copy()),
                               _hp(bsp.numpy().copy()), _hp(gamma.numpy().copy()), _hp(beta.numpy().copy()), _p(dy), _hp(stats), _st()))
    torch.cuda.synchronize()
    m = per_sample_metrics(dy, y) if uneven else metrics(dy, y)
    # (sum, sum of squares) the launch accumulated for its output vs float64 sums of the output it stored (bf16-rounded after
    # the statistics were taken: the rounding noise averages out)
    got = dy.double().cpu()
    st_ref = np.stack([got.sum(dim=(1, 2, 3)).numpy(), got.pow(2).sum(dim=(1, 2, 3)).numpy()], 1)
    m["stats_rel"] = float(np.abs(stats - st_ref).max() / np.abs(st_ref).max())
    m["stats"] = stats.tolist()
    if uneven:
        m.update(stats_per_sample(stats, dy))
    d = (dy.cpu() - y).abs()
    m["max_abs_border"] = float(torch.cat([d[..., 0, :].flatten(), d[..., -1, :].flatten(), d[..., :, 0].flatten(),
                                           d[..., :, -1].flatten()]).max())
    return m


def attention_case(B, C, H, W, seed=0, fp16=False, flash=1):
    """flash: 1 forces the flash kernel (the engine's own choice sends grids of < 32 query blocks through the three-launch
    materialised path), 0 forces the materialised path, -1 leaves the choice to the engine."""
    L = ulib.load()
    g = rng(seed)
    x = bfr(torch.randn(B, C, H, W, generator=g) * 1.2 + 0.3)
    sd = attention_weights(C, g)
    y = O.self_attention(sd, "a.", x)
    dy = torch.empty(B, C, H, W, device=DEV)
    n = lambda k: sd[k].numpy().copy()
    dx = x.to(DEV)
    # (straight at the library: the ucdir_op_* entry point reads the flag when it runs and no DY3h is involved; a DY3h that holds a plan needs ucdir_amd.ucdir.debug_flag, as hip_checks.debug_flags does)
    ulib.check(L.ucdir_debug_flag(b"flash", flash))
    try:
        ulib.check(L.ucdir_op_attention(_p(dx), B, C, H, W, _hp(n("a.norm.weight")), _hp(n("a.norm.bias")),
                                        _hp(n("a.qkv.weight")), _hp(n("a.out.weight")), _hp(n("a.out.bias")), int(fp16),
                                        _p(dy), _st()))
        torch.cuda.synchronize()
    finally:
        ulib.check(L.ucdir_debug_flag(b"flash", -1))
    # the residual dominates y; report the error relative to the attention branch alone
    m = metrics(dy, y)
    branch = y - x
    m["rel_rms_branch"] = float(((dy.cpu() - y).pow(2).mean().sqrt() / branch.pow(2).mean().sqrt()).item())
    return m


def attention_weights(C, g):
    return {"a.norm.weight": 1 + 0.25 * torch.randn(C, generator=g), "a.norm.bias": 0.2 * torch.randn(C, generator=g),
            "a.qkv.weight": torch.randn(3 * C, C, 1, 1, generator=g) * math.sqrt(3.0 / C),
            "a.out.weight": torch.randn(C, C, 1, 1, generator=g) * math.sqrt(1.5 / C),
            "a.out.bias": torch.randn(C, generator=g) * 0.1}


def last_token_share(x, sd):
    """Mean over the query rows of the softmax weight the LAST key gets (fp32 oracle algebra, model/ucdir.py:165-182)."""
    B, C, H, W = x.shape
    h = F.group_norm(x, 1, sd["a.norm.weight"], sd["a.norm.bias"], eps=1e-5).reshape(B, C, H * W)
    w = sd["a.qkv.weight"].reshape(3 * C, C)
    q, k = w[:C] @ h, w[C:2 * C] @ h
    return float(torch.softmax(torch.bmm(q.transpose(1, 2), k) / math.sqrt(C), dim=-1)[..., -1].mean())


def masking_attention_inputs(B, C, H, W, seed=0, share=0.4):
    """Attention inputs on which a masking error of the LAST key or query moves the output by far more than 1 / N: every
    token carries a common channel direction e, the last token in addition a large distinct direction f (its value row and
    its residual differ from every other token's), and rank-1 terms in the q / k weights (q_i ~ u for every token, k ~ u for
    the last token only) give the last key about ``share`` of every row's softmax mass, whatever N.  A clamped duplicate of
    key N - 1 counted once more then moves every row's branch by p (1 - p) / (1 + p) |v'(N - 1) - v'(rest)| (p = share; 0.17
    at p = 0.4, the maximum) instead of the ~1 / N a random input gives (tests/test_tile_metric_cpu.py)."""
    g = rng(seed)
    N = H * W
    e = torch.randn(C, generator=g); e -= e.mean(); e /= e.norm()
    f = torch.randn(C, generator=g); f -= f.mean(); f -= (f @ e) * e; f /= f.norm()
    u = torch.randn(C, generator=g); u /= u.norm()
    x = 0.5 * torch.randn(B, C, N, generator=g) + 2.0 * math.sqrt(C) * e.view(1, C, 1)
    x[:, :, N - 1] += 4.0 * math.sqrt(C) * f
    x = bfr(x.view(B, C, H, W))
    sd = attention_weights(C, g)
    sd["a.norm.bias"].zero_()
    sd["a.norm.weight"].fill_(1.0)
    w = sd["a.qkv.weight"].view(3 * C, C)
    w[:C] += 2.0 * torch.outer(u, e)                               # q_i ~ 2 u for every token
    base = w[C:2 * C].clone()
    lo, hi = -64.0, 64.0                                           # k(N - 1) ~ a u: bisect a for the wanted share
    for _ in range(40):
        a = 0.5 * (lo + hi)
        w[C:2 * C] = base + a * torch.outer(u, f)
        lo, hi = (a, hi) if last_token_share(x, sd) < share else (lo, a)
    w[C:2 * C] = base + 0.5 * (lo + hi) * torch.outer(u, f)
    return x, sd


def scale_qk(sd, f):
    """A copy of the attention weights with the q and the k rows of a.qkv.weight scaled by ``f``: every logit times f^2."""
    sd = {k: v.clone() for k, v in sd.items()}
    Cc = sd["a.qkv.weight"].shape[1]
    sd["a.qkv.weight"][:2 * Cc] *= f
    return sd


def attention_logit_stats(x, sd, tile=64):
    """The logits of the attention in float64 (fp32 oracle algebra): ``max_logit`` = the largest |logit|, ``mean_pmax`` = the
    mean over the query rows of the largest probability, ``last_tile_jump`` = the median over the rows of (largest logit among
    the keys of the LAST ``tile``-key tile) - (largest logit among the keys before it): what a running maximum moves by at the
    final tile (negative where the maximum sits earlier; nan if there is one tile only), ``jump_rows`` = the share of the rows
    where it exceeds 88 (exp(-88) is the smallest normal fp32: the rescale factor of everything accumulated before underflows)."""
    B, Cc, H, W = x.shape
    N = H * W
    h = F.group_norm(x.double(), 1, sd["a.norm.weight"].double(), sd["a.norm.bias"].double(), eps=1e-5).reshape(B, Cc, N)
    w = sd["a.qkv.weight"].reshape(3 * Cc, Cc).double()
    s = torch.bmm((w[:Cc] @ h).transpose(1, 2), w[Cc:2 * Cc] @ h) / math.sqrt(Cc)
    first = (N - 1) // tile * tile
    j = (s[..., first:].max(-1).values - s[..., :first].max(-1).values) if first else torch.full((1,), float("nan"), dtype=s.dtype)
    return {"max_logit": float(s.abs().max()), "mean_pmax": float(torch.softmax(s, -1).max(-1).values.mean()),
            "last_tile_jump": float(j.median()), "jump_rows": float((j > 88).double().mean())}


def attention_emu_self(x, sd, fp16=False, scores=False):
    """oracle.self_attention_emu with torch's fp32 sums against the same with float64 sums (emu_float64_sums): what two correct
    implementations of the numerics plan differ by on these inputs.  Metrics on the branch, per sample, as
    attention_emu_case(uneven=True) reports them."""
    dt = "fp16" if fp16 else "bf16"
    a = bfr(O.self_attention_emu(sd, "a.", x, True, dt, scores=scores))
    with emu_float64_sums():
        b = bfr(O.self_attention_emu(sd, "a.", x, True, dt, scores=scores))
    return per_sample_metrics(a - x, b - x)


ATT_LADDER_PHASE = 5    # attention_inputs(uneven=True): a batch of 3 takes the ladder's entries 5, 0, 1 (0.25 z - 1.5, z + 0.6, 2^-8 (z + 0.6)).
                        # The attention metrics are taken on the BRANCH, stored output minus residual input.  On the entries 2 and 4 the
                        # stored sum x + branch reaches 45 | 11, where one bf16 step is 0.25 | 0.0625 against a branch of RMS ~2: a single
                        # rounding flip of the stored sum is 0.12 | 0.03 of it, and the emulation's own two summation orders miss the tile and
                        # element bounds there (3.8e-3, 0.122: tests/test_uneven_batches_cpu.py) - such a sample says nothing about a kernel


def attention_inputs(B, C, H, W, seed=0, masking=False, uneven=False, logit_scale=1.0, share=0.4, phase=ATT_LADDER_PHASE):
    """(x, weights) of attention_emu_case: random or masking_attention_inputs; ``uneven``: x along UNEVEN_LADDER (GroupNorm
    normalises it, the residual differs per sample); ``logit_scale``: scale_qk; ``share``: of masking_attention_inputs."""
    if masking:
        x, sd = masking_attention_inputs(B, C, H, W, seed, share)
    else:
        g = rng(seed)
        z = torch.randn(B, C, H, W, generator=g)
        x = uneven_batch(z, phase) if uneven else bfr(z * 1.2 + 0.3)
        sd = attention_weights(C, g)
    return x, (scale_qk(sd, logit_scale) if logit_scale != 1.0 else sd)


def attention_emu_case(B, C, H, W, seed=0, fp16=False, flash=1, masking=False, uneven=False, logit_scale=1.0, share=0.4):
    """ucdir_op_attention against oracle.self_attention_emu on the same bf16 input (rounding where the kernels round, fp32
    accumulation; fp16: the attn_fp16 rounding points).  The emulation follows the path the engine took (profiler key 130 / 131
    = the flash kernel, otherwise the materialised-score path, which rounds the NORMALISED probabilities: scores=True).
    Metrics on the attention branch (output minus the residual input, both sides), the emulation rounded to bf16 like the
    stored output.  ``masking``: masking_attention_inputs instead of random ones.  ``logit_scale`` f: the q and k rows of the
    qkv weight times f (logits times f^2: the peaked softmax whose exp overflows without the running maximum); with it or with
    ``uneven`` (attention_inputs) the metrics are per sample and ``finite`` says whether every stored value is finite."""
    L = ulib.load()
    x, sd = attention_inputs(B, C, H, W, seed, masking, uneven, logit_scale, share)
    dy = torch.empty(B, C, H, W, device=DEV)
    n = lambda k: sd[k].numpy().copy()
    dx = x.to(DEV)
    hp = [n(k) for k in ("a.norm.weight", "a.norm.bias", "a.qkv.weight", "a.out.weight", "a.out.bias")]

    def run():
        ulib.check(L.ucdir_op_attention(_p(dx), B, C, H, W, *[_hp(a) for a in hp], int(fp16), _p(dy), _st()))
        torch.cuda.synchronize()
    # (straight at the library: the ucdir_op_* entry point reads the flag when it runs and no DY3h is involved; a DY3h that holds a plan needs ucdir_amd.ucdir.debug_flag, as hip_checks.debug_flags does)
    ulib.check(L.ucdir_debug_flag(b"flash", flash))
    try:
        _, keys = profile_keys(L, run)
    finally:
        ulib.check(L.ucdir_debug_flag(b"flash", -1))
    is_flash = (131 if fp16 else 130) in keys
    e = bfr(O.self_attention_emu(sd, "a.", x, True, "fp16" if fp16 else "bf16", scores=not is_flash))
    if uneven or logit_scale != 1.0:
        m = per_sample_metrics(dy.cpu() - x, e - x)
        m["finite"] = bool(torch.isfinite(dy).all())
        m.update(attention_logit_stats(x, sd))
    else:
        m = metrics(dy.cpu() - x, e - x)
    m["flash"] = is_flash
    m["keys"] = sorted(keys)
    if masking:
        m["last_share"] = last_token_share(x, sd)
    return m


class HipLayers:
    """One sample of the last HIP forward, layer by layer, for oracle.dy3h_naive_forward_emu without holding the network on the
    host: as ``force`` it reads a stored activation (debug_read, sliced to the sample on the device) when the emulation asks
    for it; as ``taps`` it compares the emulated layer output (bf16-rounded, like the stored one) with it and keeps only the
    metrics (``self.out``).  No other forward may run on the network while it is in use: debug_read reads the last one.
    ``controls``: {layer or layer:h1: fn}; the emulated output of each such layer is also compared with fn(stored activation),
    a deliberately wrong host-side copy (``self.controls_out``), while the emulation still continues from the stored one."""

    def __init__(self, dn, b, prefix="denoise_fn.", controls=None):
        from ucdir_amd.spec import unet_layers
        self.dn, self.b, self.out, self._last = dn, b, {}, (None, None)
        self.controls, self.controls_out = dict(controls or {}), {}
        self.names = {}
        for Ld in unet_layers(dn.cfg):
            self.names[prefix + Ld.name] = (Ld.name, Ld.name, "out")
            if Ld.kind == "block":
                self.names[prefix + Ld.name + ".res_block.h1"] = (Ld.name + ":h1", Ld.name, "h1")

    def __contains__(self, key):
        return key in self.names

    def __getitem__(self, key):
        if self._last[0] != key:
            _, layer, what = self.names[key]
            t = self.dn.debug_read(layer, what)[self.b:self.b + 1].float().cpu()
            torch.cuda.synchronize()
            self._last = (key, t)
        return self._last[1]

    def __setitem__(self, key, y):
        if key in self.names:
            name = self.names[key][0]
            self.out[name] = metrics(self[key], bfr(y))
            if name in self.controls:
                self.controls_out[name] = metrics(self.controls[name](self[key]), bfr(y))


def layerwise_emu_sample(dn, sd, x6, lvl, guide, b, pad, attn_dtype="bf16", controls=None, eps=None, attn_scores=False):
    """Layer-wise metrics of sample ``b`` of the LAST forward of ``dn`` (x6, lvl, guide: that forward's host inputs; ``pad``:
    the forward reflect-padded them by pad32 like forward_split, else they are already multiples of 32) against the emulation
    fed with the HIP path's own activations.  Returns {layer or layer:h1: metrics}; with ``controls`` (HipLayers) the pair
    ({layer: metrics}, {controlled layer: metrics of the wrong copy}).  ``eps``: that forward's output (B, 3, H, W); adds
    "eps" = the final conv on the HIP path's last activation (cropped like the forward's) against it.  ``attn_scores``: the
    forward took the materialised-score attention path (oracle.dy3h_naive_forward_emu)."""
    xs, gs = x6[b:b + 1], guide[b:b + 1]
    if pad:
        ph, pw = O.pad32(x6.shape[-2]), O.pad32(x6.shape[-1])
        xs, gs = F.pad(xs, (0, pw, 0, ph), mode="reflect"), F.pad(gs, (0, pw, 0, ph), mode="reflect")
    hl = HipLayers(dn, b, controls=controls)
    e = O.dy3h_naive_forward_emu(sd, xs, lvl[b:b + 1], gs, taps=hl, force=hl, attn_dtype=attn_dtype, attn_scores=attn_scores)
    if eps is not None:
        hl.out["eps"] = metrics(eps[b:b + 1], e[..., :x6.shape[-2], :x6.shape[-1]])
    return (hl.out, hl.controls_out) if controls is not None else hl.out


def shift_last_strip(t, cols=TILE[2]):
    """Negative control: a copy of activation ``t`` (..., H, W) whose last ``cols`` columns are shifted down by one row (row r
    holds row r - 1; row 0 is kept), as a kernel that mixed up a strip's row offset would store it.  Host-side only."""
    y = t.clone()
    c = min(cols, t.shape[-1])
    y[..., 1:, -c:] = t[..., :-1, -c:]
    return y


AKGM_KEYS = (110, 111, 112, 113, 114, 115, 116)   # profiler keys of the AKGM launch of a residual block (one per block and forward)


def ws64_tile(B, H, W, ncu):
    """Python copy of the engine's akgm_ws64 dispatch rule (engine.hip, run_akgm_halo) for a C = 512 AKGM plane of H x W at
    batch B on a device of ``ncu`` compute units: the tile size the persistent kernel takes (128 | 64 positions; key 116), or
    0 for the one-shot akgm_halo_stage_kernel (key 111).  A tile's halo, 32 npt + 2 (W + 2) + 2 positions, must fit the 272
    of AkWs64::HPOS; 128-position tiles engage from four per tile range, 64-position ones when a range holds 1.5 halos."""
    if H < 2 or (H + 2) * (W + 2) >= 32768:
        return 0
    nrole = 16                                   # 128 / AkWs64::NW
    nslots = max(ncu // nrole * nrole, nrole) // nrole
    span = (H - 1) * (W + 2) + W
    for npt in (4, 2):
        hpos = 32 * npt + 2 * (W + 2) + 2
        if hpos > 272:
            continue
        tps = -(-span // (32 * npt))
        enough = B * tps >= 4 * nslots if npt == 4 else 2 * B * span >= 3 * nslots * hpos
        if enough:
            return 32 * npt
    return 0


def ws64_prediction(cfg, B, Hc, Wc, ncu):
    """{level: (H, W, tile, blocks)} for every level whose residual blocks run AKGM at C = 512 (ws64_tile's choice), on a
    forward of compute size Hc x Wc."""
    from ucdir_amd.spec import unet_layers
    out = {}
    for Ld in unet_layers(cfg):
        if Ld.kind == "block" and Ld.cout == 512:
            h, w = Hc >> Ld.level, Wc >> Ld.level
            _, _, t, n = out.get(Ld.level, (h, w, ws64_tile(B, h, w, ncu), 0))
            out[Ld.level] = (h, w, t, n + 1)
    return out


def conv_sk_layout(MW, NW):
    """Python copy of CvSk<MW, NW> (conv_sk.hip.h): positions per unit, the fixed number of halo pieces, the LDS offset of the
    halo buffers and the workgroup's LDS limit."""
    stage, rows, lds_tab = 8192 * MW, 128 * MW, NW == 8
    off_ms = 4 * stage + (2 * 9 * rows * 4 if lds_tab else 0)
    nhw = 6 if NW == 4 else (4 if MW == 2 else 7)
    return {"NPX": 64 * (NW // MW), "NHP_MAX": NW * nhw, "OFF_H": off_ms + 64 * 8, "LDS_MAX": (160 if NW == 8 else 80) * 1024}


def conv_sk_strips(MW, NW, W):
    """Python copy of the engine's conv_sk_strips<MW, NW> (engine.hip, try_conv_sk_mw): (vertical strips, halo pieces per
    chunk) of a plane of W columns - the fewest strips whose halo fits the LDS and the fixed piece count - or None."""
    L = conv_sk_layout(MW, NW)
    ns = 1
    while True:
        Ws = -(-W // ns)
        Wpe = Ws + 1 if ns == 1 else Ws + 2
        nhp = (L["NPX"] + 2 * Wpe + 2 + 15) // 16
        if nhp <= L["NHP_MAX"] and L["OFF_H"] + 2 * nhp * 1024 <= L["LDS_MAX"]:
            return ns, nhp
        if Ws <= 8:
            return None
        ns += 1


def conv_sk_strip_switches(MW, NW, max_strips=3, wmax=1024):
    """The widths on both sides of every change of conv_sk_strips' strip count up to ``max_strips`` strips: [(W - 1, W), ...]
    with strips(W - 1) != strips(W) and both <= max_strips."""
    out = []
    for W in range(9, wmax):
        a, b = conv_sk_strips(MW, NW, W - 1), conv_sk_strips(MW, NW, W)
        if a and b and a[0] != b[0] and max(a[0], b[0]) <= max_strips:
            out.append((W - 1, W))
    return out


HALO_PX = 324          # conv_halo.hip.h, HC_HALO_PX: positions of a pixel tile's halo
_TILE_CAND = []


def choose_tile(H, W):
    """Python copy of the engine's choose_tile (engine.hip): the th x tw pixel tile of conv3x3_halo, its Upsample parity
    launches and the one-shot AKGM kernels on an H x W plane - th 1..64, tw 4..256, th tw <= 256, halo (th + 2)(tw + 2) <= 324,
    the first candidate (th ascending, then tw) of the best slot utilisation, the same double arithmetic in the same order."""
    if not _TILE_CAND:
        a, b = np.repeat(np.arange(1, 65), 253), np.tile(np.arange(4, 257), 64)
        ok = (a * b <= 256) & ((a + 2) * (b + 2) <= HALO_PX)
        _TILE_CAND.extend([a[ok], b[ok], 1e-4 * (a[ok] + 2) * (b[ok] + 2) / 324.0])
    a, b, pen = _TILE_CAND
    tiles = ((H + a - 1) // a).astype(np.float64) * ((W + b - 1) // b)
    util = float(H * W) / (tiles * 256.0) - pen
    i = int(np.argmax(util))
    return int(a[i]), int(b[i])


_TILE_MAPS = {}


def tile_map(lo=2, hi=112):
    """{(H, W): choose_tile(H, W)} for H, W in lo..hi (memoised)."""
    if (lo, hi) not in _TILE_MAPS:
        _TILE_MAPS[lo, hi] = {(H, W): choose_tile(H, W) for H in range(lo, hi + 1) for W in range(lo, hi + 1)}
    return _TILE_MAPS[lo, hi]


def tile_plane(tile, lo=2, hi=112, admit=None):
    """The smallest plane (H W, then H) with H, W in lo..hi on which choose_tile gives ``tile``, among those with the most axes
    (2, 1, 0) that hold at least two tiles; ``admit``: a predicate on (H, W) the plane must meet.  None if there is none."""
    th, tw = tile
    n = lambda hw: (-(-hw[0] // th) >= 2) + (-(-hw[1] // tw) >= 2)
    planes = [hw for hw, t in tile_map(lo, hi).items() if t == tile and (admit is None or admit(hw))]
    if not planes:
        return None
    best = max(n(hw) for hw in planes)
    return min((hw for hw in planes if n(hw) == best), key=lambda hw: (hw[0] * hw[1], hw))


def tile_cover(lo=2, hi=112):
    """A cover of the distinct pixel tiles of the planes with H, W in lo..hi: for every th that occurs the tiles with its
    smallest and largest tw, for every tw those with its smallest and largest th, every tile whose halo has >= 300 positions
    and every tile of exactly 256 positions.  Returns [((th, tw), (H, W))] sorted by tile; (H, W) is the smallest plane of the
    range that yields the tile with at least two tiles along both axes, else with two along one axis, else any (tile_plane)."""
    tm = tile_map(lo, hi)
    tiles = sorted(set(tm.values()))
    cover = set()
    for th in {t[0] for t in tiles}:
        tws = [t[1] for t in tiles if t[0] == th]
        cover |= {(th, min(tws)), (th, max(tws))}
    for tw in {t[1] for t in tiles}:
        ths = [t[0] for t in tiles if t[1] == tw]
        cover |= {(min(ths), tw), (max(ths), tw)}
    cover |= {t for t in tiles if (t[0] + 2) * (t[1] + 2) >= 300 or t[0] * t[1] == 256}
    return [(t, tile_plane(t, lo, hi)) for t in sorted(cover)]


EMU_TILE_MIN_BLOCK = 4096   # EMU_TILE_TOL applies to activations whose tile_max block (metrics()["block"]) holds at least this many elements.
                            # A block of n elements that holds the activation's largest bf16 flip has tile_max >= elem_max / sqrt(n): the flips of
                            # the emulation against itself (2.2e-2, tests/test_small_shapes_cpu.py) are 1.4e-3 on the 256 elements of a 2 x 2 plane
                            # and 3.5e-4 on 4096.  MI355X, the smallest shapes, blocks below 4096: worst tile_max 2.45e-3 (naiveforward
                            # 3 x 32 x 64, a 512-element block: the flip of 5.54e-2 alone, 5.54e-2 / sqrt(512)), others 0.89 - 1.93e-3


def emu_small_ok(m):
    """emu_layer_ok with the block-size condition of the smallest planes: the tile-local bound only where a block holds at least
    EMU_TILE_MIN_BLOCK elements (on a smaller plane one wrong position already moves rel_rms by orders of magnitude)."""
    return ((not m["nan"]) and m["rel_rms"] < EMU_LAYER_TOL and m["elem_max"] < EMU_ELEM_TOL
            and (m["block"] < EMU_TILE_MIN_BLOCK or m["tile_max"] < EMU_TILE_TOL))


def op_ok(m, tol=4e-3):
    """The bounds of a single-operator case (tol = OP_TOL of tests/test_hip_gpu.py): global, tile-local and element."""
    return (not m["nan"]) and m["rel_rms"] < tol and m["tile_max"] < OP_TILE_TOL and m["elem_max"] < OP_ELEM_TOL


class _Float64Sums:
    """Stand-in for a module (torch / torch.nn.functional) inside the oracle whose conv2d / bmm accumulate in float64 and round
    the result to fp32 once; everything else is the module's own."""

    def __init__(self, mod):
        self._mod = mod

    def __getattr__(self, name):
        return getattr(self._mod, name)

    def conv2d(self, x, w, bias=None, *a, **k):
        return self._mod.conv2d(x.double(), w.double(), None if bias is None else bias.double(), *a, **k).float()

    def bmm(self, a, b):
        return self._mod.bmm(a.double(), b.double()).float()


class emu_float64_sums:
    """Context: the oracle's emulation modes with a second summation order - every conv and batched matrix product summed in
    float64 and rounded to fp32 once (the exactly-rounded sum) instead of torch's fp32 accumulation.  The rounding points of the
    numerics plan stay where they are."""

    def __enter__(self):
        self._saved = (O.F, O.torch)
        O.F, O.torch = _Float64Sums(F), _Float64Sums(torch)

    def __exit__(self, *exc):
        O.F, O.torch = self._saved


def emu_self_comparison(sd, cfg, B, H, W, levels, seed, inputs=None, attn_scores=False):
    """Two summation orders of the emulation on the same inputs, layer by layer as layerwise_emu_case compares the HIP path with
    it: one forward stores its activations as bf16; then every layer is evaluated on those stored activations (teacher forcing)
    once with torch's fp32 sums - the role of the HIP path - and once with float64 sums.  {activation | "eps": metrics}.
    ``inputs``: (cond, guide, x_t) tensors of (B, 3, H, W) instead of synth_inputs(B, H, W, seed)."""
    cond, guide, x_t = inputs if inputs is not None else map(torch.from_numpy, synth_inputs(B, H, W, seed=seed))
    lvl = torch.tensor(levels, dtype=torch.float32).view(B, 1)
    x6 = torch.cat([cond, x_t], 1)
    first = {}
    O.dy3h_naive_forward_emu(sd, x6, lvl, guide, taps=first, attn_scores=attn_scores)
    force = {k: bfr(v) for k, v in first.items()}
    t32, t64 = {}, {}
    e32 = O.dy3h_naive_forward_emu(sd, x6, lvl, guide, taps=t32, force=force, attn_scores=attn_scores)
    with emu_float64_sums():
        e64 = O.dy3h_naive_forward_emu(sd, x6, lvl, guide, taps=t64, force=force, attn_scores=attn_scores)
    out = {"eps": metrics(e32, e64)}
    for k in force:
        out[k[len("denoise_fn."):]] = metrics(bfr(t32[k]), bfr(t64[k]))
    return out


def build_net(cfg: UNetConfig, seed=0):
    """Product netG (DY3h on the HIP engine) + oracle state dict with identical synthetic weights."""
    from ucdir_amd import networks
    opt = {"model": {"which_model_G": "ucdir", "unet_name": "DY3h", "diffusion_name": "ResiGaussianGuideDY",
                     "unet": dict(in_channel=cfg.in_channel, out_channel=cfg.out_channel,
                                  inner_channel=cfg.inner_channel, channel_mults=list(cfg.channel_mults),
                                  attn_res=list(cfg.attn_res), res_blocks=cfg.res_blocks, dropout=cfg.dropout,
                                  norm_groups=1, image_size=cfg.image_size),
                     "diffusion": dict(image_size=128, channels=3, conditional=True)}}
    net = networks.define_G(opt)
    np_sd = synth_state_dict(cfg, seed)
    missing, unexpected = net.load_state_dict({k: torch.from_numpy(v) for k, v in np_sd.items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    net = net.to(DEV).eval()
    return net, O.to_torch_sd(np_sd)


def forward_case(cfg: UNetConfig, B, H, W, levels, seed=11, taps=False, net_sd=None, emu=False):
    """HIP forward vs the fp32 oracle (``eps``, and per layer with ``taps``).  ``emu``: also against the oracle's bf16-emulation
    mode (oracle.dy3h_naive_forward_emu: rounding where the kernels round), final output ``eps_emu`` and per layer ``<name>@emu``:
    what is left between HIP and the emulation is summation order, not the rounding plan, so that bound is several times tighter."""
    net, sd = net_sd if net_sd is not None else build_net(cfg)
    cond, guide, x_t = synth_inputs(B, H, W, seed=seed)
    cond, guide, x_t = map(torch.from_numpy, (cond, guide, x_t))
    lvl = torch.tensor(levels, dtype=torch.float32).view(B, 1)
    x6 = torch.cat([cond, x_t], 1)
    otaps = {} if taps else None
    etaps = {} if (taps and emu) else None
    ph, pw = O.pad32(H), O.pad32(W)
    if taps:
        ref_full = O.dy3h_naive_forward(sd, F.pad(x6, (0, pw, 0, ph), mode="reflect"), lvl,
                                        F.pad(guide, (0, pw, 0, ph), mode="reflect"), taps=otaps)
        ref = ref_full[..., :-ph, :-pw]
    else:
        ref = O.dy3h_forward(sd, x6, lvl, guide)
    ref_emu = O.dy3h_forward(sd, x6, lvl, guide, emulate_bf16=True, taps=etaps) if emu else None
    with torch.no_grad():
        eps = net.denoise_fn(x6.to(DEV), lvl.to(DEV), guide.to(DEV))
    torch.cuda.synchronize()
    out = {"eps": metrics(eps, ref)}
    if emu:
        out["eps_emu"] = metrics(eps, ref_emu)
        out["emu_vs_oracle"] = metrics(ref_emu, ref)
    if taps:
        from ucdir_amd.spec import unet_layers
        for Ld in unet_layers(cfg):
            key = "denoise_fn." + Ld.name
            got = net.denoise_fn.debug_read(Ld.name, "out")
            torch.cuda.synchronize()
            out[Ld.name] = metrics(got, otaps[key])
            if emu:
                out[Ld.name + "@emu"] = metrics(got, etaps[key])
            if Ld.kind == "block":
                got = net.denoise_fn.debug_read(Ld.name, "h1")
                torch.cuda.synchronize()
                out[Ld.name + ":h1"] = metrics(got, otaps[key + ".res_block.h1"])
                if emu:
                    out[Ld.name + ":h1@emu"] = metrics(got, etaps[key + ".res_block.h1"])
    return out, eps.cpu(), ref


def layerwise_emu_case(cfg: UNetConfig, B, H, W, levels, seed=11, net_sd=None):
    """Every layer of a HIP forward against the oracle's bf16-emulation mode evaluated ON THE HIP PATH'S OWN INPUTS (teacher
    forcing: oracle.dy3h_naive_forward_emu(force=...)): per layer {name: metrics(HIP stored activation, bf16(emulated layer
    output))}, plus 'eps' = the final conv on the HIP path's last activation.  Two realisations of the rounding noise decorrelate
    over the depth of the network (HIP vs emulation end to end: 1.2e-2, like HIP vs the fp32 oracle); layer by layer on identical
    inputs they differ by summation order only, so a systematic error of a few 1e-3 in ANY single layer shows."""
    net, sd = net_sd if net_sd is not None else build_net(cfg)
    cond, guide, x_t = map(torch.from_numpy, synth_inputs(B, H, W, seed=seed))
    lvl = torch.tensor(levels, dtype=torch.float32).view(B, 1)
    x6 = torch.cat([cond, x_t], 1)
    with torch.no_grad():
        eps = net.denoise_fn(x6.to(DEV), lvl.to(DEV), guide.to(DEV))
    torch.cuda.synchronize()
    from ucdir_amd.spec import unet_layers
    force = {}
    for Ld in unet_layers(cfg):
        key = "denoise_fn." + Ld.name
        force[key] = net.denoise_fn.debug_read(Ld.name, "out").float().cpu()
        if Ld.kind == "block":
            force[key + ".res_block.h1"] = net.denoise_fn.debug_read(Ld.name, "h1").float().cpu()
    torch.cuda.synchronize()
    ph, pw = O.pad32(H), O.pad32(W)
    etaps = {}
    e = O.dy3h_naive_forward_emu(sd, F.pad(x6, (0, pw, 0, ph), mode="reflect"), lvl, F.pad(guide, (0, pw, 0, ph), mode="reflect"),
                                 taps=etaps, force=force)[..., :-ph, :-pw]
    out = {"eps": metrics(eps, e)}
    for k, v in force.items():
        out[k[len("denoise_fn."):]] = metrics(v, etaps[k].to(torch.bfloat16).float())
    return out


def conv_stats_case(B, H, W, cin, cout, ksize, mode, gn, runs=3, seed=0, uneven=False):
    """GroupNorm statistics a conv launch accumulates for its OUTPUT (fixed-point atomics) against float64 sums of the
    output it stored, and their run-to-run reproducibility.  A size-independent property: usable at bench size."""
    L = ulib.load()
    g = rng(seed)
    z = torch.randn(B, cin, H, W, generator=g)
    x = (uneven_batch(z, 0) if uneven else bfr(z * 1.3 + 0.6)).to(DEV)
    w = (torch.randn(cout, cin, ksize, ksize, generator=g) * math.sqrt(1.5 / (cin * ksize * ksize))).numpy().copy()
    b = (torch.randn(cout, generator=g) * 0.1).numpy().copy()
    gm = (1 + 0.25 * torch.randn(cin, generator=g)).numpy().copy() if gn else None
    bt = (0.2 * torch.randn(cin, generator=g)).numpy().copy() if gn else None
    Ho, Wo = (H // 2, W // 2) if mode == 1 else ((2 * H, 2 * W) if mode == 2 else (H, W))
    outs, sts = [], []
    for _ in range(runs):
        y = torch.empty(B, cout, Ho, Wo, device=DEV)
        st = np.zeros((B, 2), dtype=np.float64)
        ulib.check(L.ucdir_op_conv(_p(x), cin, _p(None), 0, B, H, W, _hp(w), _hp(b), _hp(gm), _hp(bt), cout, ksize, mode, 1,
                                   _p(None), _p(y), _hp(st), _st()))
        torch.cuda.synchronize()
        outs.append(y); sts.append(st.copy())
    ref = np.stack([outs[0].double().sum(dim=(1, 2, 3)).cpu().numpy(), outs[0].double().pow(2).sum(dim=(1, 2, 3)).cpu().numpy()], 1)
    m = {"stats_rel": float(np.abs((sts[0] - ref) / ref).max()),
         "outputs_reproducible": all(torch.equal(outs[0], o) for o in outs[1:]),
         "stats_reproducible": all(np.array_equal(sts[0], s_) for s_ in sts[1:])}
    if uneven:
        m.update(stats_per_sample(sts[0], outs[0]))
        m["finite"] = bool(torch.isfinite(outs[0]).all())
    return m


def predictor_case(B, H, W, seed=3, net_sd=None):
    """UNetSeeInDark on the HIP engine vs the oracle (model/ucdir.py:352-403)."""
    net, sd = net_sd if net_sd is not None else build_net(UNetConfig(inner_channel=64, channel_mults=(1, 2), res_blocks=1,
                                                                    attn_res=(64,), image_size=128))
    x = torch.from_numpy(synth_inputs(B, H, W, seed=seed)[0])
    ref = O.predictor_forward(sd, x)
    with torch.no_grad():
        got = net.predictor(x.to(DEV))
    torch.cuda.synchronize()
    return metrics(got, ref)


# the predictor's activations in forward order, by the reference's module names (UNetSeeInDark.debug_read)
PREDICTOR_LAYERS = (["conv1_1", "conv1_2", "pool1"] + [n for l in range(2, 5) for n in (f"conv{l}_1", f"conv{l}_2", f"pool{l}")]
                    + ["conv5_1", "conv5_2"] + [n for l in range(6, 10) for n in (f"upv{l}", f"conv{l}_1", f"conv{l}_2")])


def assert_layers_ok(outs, keys, what):
    """Print and assert the per-layer bounds of a whole-network layer-wise check.  outs: {sample: {activation: metrics}} as
    layerwise_emu_sample returns them for the full SID configuration; keys: the forward's profiler keys."""
    for b, out in outs.items():
        worst = max(out, key=lambda k: out[k]["rel_rms"])
        worst_t = max(out, key=lambda k: out[k]["tile_max"])
        print(f"{what}, sample {b}: {len(out)} activations, worst {worst}: {out[worst]['rel_rms']:.3e}, "
              f"worst tile {worst_t}: {out[worst_t]['tile_max']:.3e} at {out[worst_t]['tile_at']}")
    print(f"{what}: profiler keys {sorted(keys)}")
    for b, out in outs.items():
        assert len(out) == 36 + 27, len(out)    # 36 layer outputs (stem, 27 blocks, 4 + 4 resamplers) + 27 h1 tensors
        for k, m in out.items():
            assert not m["nan"] and m["rel_rms"] < EMU_LAYER_TOL, (b, k, m)
            assert m["tile_max"] < EMU_TILE_TOL, (b, k, m)


def emu_layer_ok(m):
    """The bounds one teacher-forced layer of the HIP path must meet against the emulation (global, tile-local, element)."""
    return (not m["nan"]) and m["rel_rms"] < EMU_LAYER_TOL and m["tile_max"] < EMU_TILE_TOL and m["elem_max"] < EMU_ELEM_TOL


def predictor_real_channels(name):
    """Real channel count of a predictor activation (the engine carries the 32-channel ones as 64)."""
    l = int(name[-1]) if name.startswith(("pool", "upv")) else int(name[4])
    lvl = l - 1 if name.startswith("pool") else (9 - l if name.startswith("upv") or l > 5 else l - 1)
    return 32 << lvl


class PredictorLayers:
    """One sample of the last HIP predictor forward, layer by layer, for oracle.predictor_forward_emu (the HipLayers protocol):
    as ``force`` it reads the stored activation (UNetSeeInDark.debug_read, sliced to the sample and to the real channels); as
    ``taps`` it keeps only the metrics of the emulated layer (bf16-rounded, like the stored one) against it.  Every read also
    checks that the stored values are finite and that the upper half of a 32-channel layer carried as 64 is exactly zero
    (``self.upper``: {layer: max |upper half|}, ``self.finite``: {layer: bool})."""

    def __init__(self, pred, b):
        self.pred, self.b, self.out, self.upper, self.finite, self._last = pred, b, {}, {}, {}, (None, None)

    def __contains__(self, key):
        return key in PREDICTOR_LAYERS

    def __getitem__(self, key):
        if self._last[0] != key:
            full = self.pred.debug_read(key)[self.b:self.b + 1]
            real = predictor_real_channels(key)
            self.finite[key] = bool(torch.isfinite(full).all())
            if full.shape[1] > real:
                self.upper[key] = float(full[:, real:].abs().max())
            t = full[:, :real].float().cpu()
            del full
            torch.cuda.synchronize()
            self._last = (key, t)
        return self._last[1]

    def __setitem__(self, key, y):
        if key in PREDICTOR_LAYERS:
            self.out[key] = metrics(self[key], bfr(y))


def predictor_emu_case(net, sd, B, H, W, seed=3, samples=None, x=None):
    """UNetSeeInDark on the HIP engine, layer by layer, against oracle.predictor_forward_emu fed with the HIP path's own
    activations (teacher forcing), per sample in ``samples`` (default: all): {sample: {layer | "out": metrics}}, plus the upper
    halves / finiteness PredictorLayers checked.  "out" = conv10_1 (fp32 output, cropped) on the HIP path's conv9_2.
    ``x``: the (B, 3, H, W) input instead of synth_inputs(B, H, W, seed)[0]."""
    if x is None:
        x = torch.from_numpy(synth_inputs(B, H, W, seed=seed)[0])
    with torch.no_grad():
        got = net.predictor(x.to(DEV)).cpu()
    torch.cuda.synchronize()
    res = {"samples": {}, "upper": {}, "finite": {}, "out_finite": bool(torch.isfinite(got).all())}
    for b in (range(B) if samples is None else samples):
        hl = PredictorLayers(net.predictor, b)
        e = O.predictor_forward_emu(sd, x[b:b + 1], taps=hl, force=hl)
        hl.out["out"] = metrics(got[b:b + 1], e)
        res["samples"][b] = hl.out
        res["upper"].update({k: max(v, res["upper"].get(k, 0.0)) for k, v in hl.upper.items()})
        res["finite"].update({k: v and res["finite"].get(k, True) for k, v in hl.finite.items()})
    return res, got, x


def fewstep_formula(coef, x, eps, m, z):
    """ucdir_fewstep_update in float64 on float64 tensors: (x <- ..., m_prev <- x0) for coef = (c_recip, c_recipm1, flags, p, q, r,
    b1, store_m, sigma), each coefficient rounded to the fp32 the kernel takes."""
    from ucdir_amd.ucdir import FEWSTEP_CLIP, FEWSTEP_FACTORED
    c_recip, c_recipm1, flags, p, q, r, b1, store_m, sigma = coef
    f32 = lambda v: float(np.float32(v))
    if flags & FEWSTEP_FACTORED:
        x0 = f32(c_recip) * (x - f32(c_recipm1) * eps)
    else:
        x0 = f32(c_recip) * x - f32(c_recipm1) * eps
    if flags & FEWSTEP_CLIP:
        x0 = x0.clamp(-1.0, 1.0)
    return f32(p) * x0 + f32(q) * x + f32(r) * eps + f32(b1) * m + f32(sigma) * z, x0


def sampler_step_case(seed=0):
    from ucdir_amd.ucdir import sampler_step_
    g = rng(seed)
    tab = O.schedule_tables(dict(schedule="linear", n_timestep=50, linear_start=1e-6, linear_end=0.4))
    out = {}
    for t in (49, 25, 1, 0):
        x = torch.randn(2, 3, 40, 56, generator=g)
        eps = torch.randn(2, 3, 40, 56, generator=g)
        nz = torch.randn(2, 3, 40, 56, generator=g)
        ref = O.p_sample_step(tab, x, eps, t, nz)
        sig = float(np.exp(np.float32(0.5) * tab["posterior_log_variance_clipped"][t])) if t > 0 else 0.0
        dx = x.to(DEV).clone()
        sampler_step_(dx, eps.to(DEV), nz.to(DEV) if t > 0 else None, tab["sqrt_recip_alphas_cumprod"][t],
                      tab["sqrt_recipm1_alphas_cumprod"][t], tab["posterior_mean_coef1"][t],
                      tab["posterior_mean_coef2"][t], sig)
        torch.cuda.synchronize()
        out[f"t{t}"] = metrics(dx, ref)
    return out


def sampler_case(cfg: UNetConfig, H, W, T, seed=5, net_sd=None):
    """T-step restoration with injected noise: HIP path vs oracle; returns PSNR on uint8 images."""
    net, sd = net_sd if net_sd is not None else build_net(cfg)
    sched = dict(schedule="linear", n_timestep=T, linear_start=1e-6, linear_end=0.4)
    tab = O.schedule_tables(sched)
    net.set_new_noise_schedule(sched, torch.device(DEV))
    cond = torch.from_numpy(synth_inputs(1, H, W, seed=seed)[0])
    g = rng(seed + 100)
    noises = [torch.randn(1, 3, H, W, generator=g) for _ in range(T)]
    ref = O.super_resolution(sd, tab, cond, noises, continous=False)
    net.noise_source = lambda shape, device, k: noises[k].to(device)
    with torch.no_grad():
        got = net.super_resolution(cond.to(DEV), False)
    net.noise_source = None
    torch.cuda.synchronize()
    m = metrics(got, ref.view_as(got.cpu()))
    m["psnr_u8"] = O.psnr(O.tensor2img(got.cpu()), O.tensor2img(ref))
    return m


# ---- value regimes of the whole denoiser / predictor (tests/test_uneven_batches_*.py) ------------------------------------------
REGIME_LEVELS = (0.9999, 0.5, 0.03, 1e-4)


def regime_inputs(H, W, seed=0):
    """Four samples of H x W that differ in kind, as (cond, guide, x_t) tensors of (4, 3, H, W): 0 dark like the SID workload
    (cond = guide = clip(-0.92 + 0.03 z), x_t ~ N(0, 1)), 1 synth_inputs, 2 saturated (random 8 x 8 blocks of -1 and +1,
    x_t = 0.05 z + cond), 3 flat (cond = guide = 0.25 everywhere, x_t ~ N(0, 1))."""
    g = rng(seed)
    cond, guide, x_t = (torch.from_numpy(a).repeat(4, 1, 1, 1) for a in synth_inputs(1, H, W, seed=seed))
    cond[0] = guide[0] = (-0.92 + 0.03 * torch.randn(3, H, W, generator=g)).clamp(-1, 1)
    x_t[0] = torch.randn(3, H, W, generator=g)
    blocks = (torch.rand(3, -(-H // 8), -(-W // 8), generator=g) < 0.5).float() * 2 - 1
    cond[2] = guide[2] = blocks.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W]
    x_t[2] = 0.05 * torch.randn(3, H, W, generator=g) + cond[2]
    cond[3] = guide[3] = 0.25
    x_t[3] = torch.randn(3, H, W, generator=g)
    return cond.contiguous(), guide.contiguous(), x_t.contiguous()


def pad_to_compute(*ts):
    """forward_split's reflect pad (pad32) of (B, C, H, W) tensors: the compute-size inputs of the emulation."""
    ph, pw = O.pad32(ts[0].shape[-2]), O.pad32(ts[0].shape[-1])
    return tuple(F.pad(t, (0, pw, 0, ph), mode="reflect") for t in ts)


# ---- time embedding at the levels DPM-Solver++ feeds (0 ... 999) ---------------------------------------------------------------
TIME_LEVELS = (0.0, 3.7, 49.0, 250.3, 999.0)


def time_weights_f64(sd, levels, blocks, prefix="denoise_fn."):
    """The oracle's PositionalEncoding + noise_level_mlp + every block's noise_func in float64 at fp32 ``levels`` (a list):
    (len(blocks), B, 8)."""
    sd64 = {k: v.double() for k, v in sd.items() if "noise_" in k}
    lvl = torch.tensor(levels, dtype=torch.float32).double().view(-1, 1)
    temb = O.noise_embedding(sd64, lvl, prefix)
    return torch.stack([O.time_weights(sd64, prefix + n + ".res_block.", temb) for n in blocks])


def time_rel_err(got, ref):
    """(B,) per level: the worst over the blocks of max |got - ref| over the level's 8 weights, relative to the largest |ref| of
    the block's whole (B, 8) table - the measure of test_time_embedding_direct, resolved by level; got, ref (blocks, B, 8)."""
    return ((got.double() - ref).abs().amax(-1) / ref.abs().amax((-1, -2)).unsqueeze(-1)).amax(0)


def time_ulp_change(sd, levels, blocks):
    """time_rel_err between the float64 oracle at each fp32 level and at the next fp32 number above it: what one ulp of the
    level alone moves the block weights by."""
    up = np.nextafter(np.asarray(levels, dtype=np.float32), np.float32(np.inf)).tolist()
    return time_rel_err(time_weights_f64(sd, up, blocks), time_weights_f64(sd, levels, blocks))


# time_ulp_change on the synthetic SID weights at TIME_LEVELS, in the float64 oracle (tests/test_uneven_batches_cpu.py asserts them).
# Above level 1 the fp32 algebra itself is sensitive: the encoder's argument level * exp(-ln(1e4) k / half) reaches the level itself,
# and sin / cos of an argument of 999 carry its ulp (6.1e-5) whole.  The fp32 oracle against the float64 one: 3.6e-7, 6.8e-7,
# 4.8e-6, 1.8e-5 at these levels
TIME_ULP_CHANGE = {3.7: 1.075e-7, 49.0: 2.161e-6, 250.3: 8.783e-6, 999.0: 2.197e-5}


def time_mlp_fp32_model(sd, level, blocks, prefix="denoise_fn."):
    """time_mlp_kernel's algebra on the CPU in its own precision and order: fp32 throughout, every sum accumulated serially from
    the bias on with one rounding per term (a fused multiply-add, as the kernel compiles).  (len(blocks), 8) for one level."""
    f = np.float32
    n = lambda k: sd[prefix + k].numpy().astype(f)

    def serial(Wm, b, x):
        a = b.copy()
        for k in range(Wm.shape[1]):
            a = (a.astype(np.float64) + Wm[:, k].astype(np.float64) * np.float64(x[k])).astype(f)
        return a
    sw = lambda a: (a / (f(1) + np.exp(-a).astype(f))).astype(f)
    w1 = n("noise_level_mlp.1.weight")
    half = w1.shape[1] // 2
    step = (np.arange(half, dtype=f) / f(half)).astype(f)
    e = (f(level) * np.exp((f(-9.210340371976184) * step).astype(f)).astype(f)).astype(f)
    enc = np.concatenate([np.sin(e).astype(f), np.cos(e).astype(f)])
    temb = serial(n("noise_level_mlp.3.weight"), n("noise_level_mlp.3.bias"), sw(serial(w1, n("noise_level_mlp.1.bias"), enc)))
    out = []
    for name in blocks:
        q = name + ".res_block.noise_func."
        out.append(serial(n(q + "2.weight"), n(q + "2.bias"), sw(serial(n(q + "0.weight"), n(q + "0.bias"), temb))))
    return torch.from_numpy(np.stack(out))


# Level 3.7 is the one regime where that bound lies under the fp32 algebra's own noise: one ulp of 3.7 moves the weights by 1.08e-7,
# while the fp32 sums of the two MLPs alone leave 5 - 8e-7 at EVERY level (level 0, where the argument is exact: fp32 oracle 4.9e-7,
# the kernel 6.7e-7).  time_mlp_fp32_model, the kernel's own precision and summation order on the CPU, sits at 6.77e-7 from the
# float64 oracle at 3.7 (5.16e-7 with separately rounded products): the numerics plan misses 4 x 1.08e-7, so the bound there is 1.5x
# the model's value (tests/test_uneven_batches_cpu.py asserts both).  MI355X: 6.67e-7, 8.91e-7, 5.66e-7, 4.67e-6, 1.66e-5 at
# levels 0, 3.7, 49, 250.3, 999
TIME_FP32_MODEL_ERR = {3.7: 6.77e-7}


def time_bound(level):
    """The bound of time_rel_err at ``level``: 2e-5 (test_time_embedding_direct's) up to level 1; above, 4x what one ulp of the
    level moves the weights by - the encoder's argument is the product of two rounded fp32 factors, on each side - or, where
    the fp32 model of the kernel itself misses that (TIME_FP32_MODEL_ERR), 1.5x the model's distance."""
    if level <= 1:
        return 2e-5
    return max(4 * TIME_ULP_CHANGE[level], 1.5 * TIME_FP32_MODEL_ERR.get(level, 0.0))
