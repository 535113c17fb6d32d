"""GPU tests of the full SID denoiser at the smallest shapes the engine accepts (``pytest -m gpu``): forward_split
(reflect pad to the next multiple of 32) from 33 x 33 - compute 64 x 64, level-4 planes of 4 x 4, attention on 64 tokens - and
naiveforward (no pad) from 32 x 32 - level-4 planes of 2 x 2, attention on 16 tokens.  Every stored activation (36 layer
outputs + 27 h1 tensors) and eps of every sample against the oracle's bf16 emulation on the HIP path's own activations
(hip_checks.layerwise_emu_sample), with EMU_LAYER_TOL and EMU_ELEM_TOL for every activation and EMU_TILE_TOL for those whose
tile_max block holds at least EMU_TILE_MIN_BLOCK elements (tests/test_small_shapes_cpu.py measures why); eps end to end
against the fp32 oracle with CROP_TOL, the bound for an estimate from a few thousand values.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_checks as C  # noqa: E402
from oracle import ucdir_oracle as O  # noqa: E402
from ucdir_amd.spec import UNetConfig, unet_layers  # noqa: E402
from ucdir_amd.weights import synth_inputs  # noqa: E402

SID = UNetConfig(inner_channel=64, channel_mults=(1, 2, 4, 8, 8), res_blocks=2, attn_res=(16,), image_size=128)
CROP_TOL = 2.0e-2     # eps against the fp32 oracle on 3k - 18k values (tests/test_hip_gpu.py: the bound of a 3 x 32 x 32 crop; the
                      # emulation itself sits 1.48 - 1.57e-2 from the oracle at these shapes)


@pytest.fixture(scope="module")
def sid_net():
    return C.build_net(SID)


def _levels(B):
    return torch.linspace(0.02, 0.97, B).reshape(B, 1) if B > 1 else torch.full((1, 1), 0.41)


def _forward(net, B, H, W, seed, pad):
    """One forward of B inputs of H x W under the profiler: forward_split (pad) or naiveforward.  (host inputs, eps, keys)."""
    cond, guide, x_t = map(torch.from_numpy, synth_inputs(B, H, W, seed=seed))
    lvl = _levels(B)
    x6 = torch.cat([cond, x_t], 1)
    dn = net.denoise_fn

    def fwd():
        with torch.no_grad():
            e = (dn.forward_split(cond.cuda(), x_t.cuda(), lvl.cuda(), guide.cuda()) if pad
                 else dn.naiveforward(x6.cuda(), lvl.cuda(), guide.cuda()))
        torch.cuda.synchronize()
        return e.cpu()
    eps, keys = C.profile_keys(C.ulib.load(), fwd)
    return (x6, lvl, guide), eps, keys


def _layers_ok(net, sd, inputs, eps, keys, samples, pad, what):
    x6, lvl, guide = inputs
    assert bool(torch.isfinite(eps).all()) and eps.shape == (x6.shape[0], 3) + tuple(x6.shape[-2:]), eps.shape
    print(f"{what}: profiler keys {sorted(keys)}")
    for b in samples:
        out = C.layerwise_emu_sample(net.denoise_fn, sd, x6, lvl, guide, b, pad=pad, eps=eps)
        big = {k: m for k, m in out.items() if m["block"] >= C.EMU_TILE_MIN_BLOCK}
        wr, we, wt = (max(d, key=lambda k: d[k][f]) for d, f in ((out, "rel_rms"), (out, "elem_max"), (big, "tile_max")))
        ws = max(m["tile_max"] for m in out.values() if m["block"] < C.EMU_TILE_MIN_BLOCK)
        print(f"{what}, sample {b}: {len(out)} activations, worst {wr}: {out[wr]['rel_rms']:.3e}, worst element {we}: "
              f"{out[we]['elem_max']:.3e}, worst tile (blocks >= {C.EMU_TILE_MIN_BLOCK}) {wt}: {big[wt]['tile_max']:.3e} at "
              f"{big[wt]['tile_at']}; on smaller blocks {ws:.3e}")
        assert len(out) == 36 + 27 + 1, len(out)            # 36 layer outputs (stem, 27 blocks, 4 + 4 resamplers) + 27 h1 tensors + eps
        for k, m in out.items():
            assert C.emu_small_ok(m), (b, k, m)
        ref = O.dy3h_forward(sd, x6[b:b + 1], lvl[b:b + 1], guide[b:b + 1]) if pad else O.dy3h_naive_forward(sd, x6[b:b + 1], lvl[b:b + 1], guide[b:b + 1])
        m = C.metrics(eps[b:b + 1], ref)
        print(f"{what}, sample {b}: eps vs the fp32 oracle {m['rel_rms']:.3e} ({ref.numel()} values)")
        assert not m["nan"] and m["rel_rms"] < CROP_TOL, (b, m)


@pytest.mark.parametrize("shape", [(1, 33, 33), (3, 33, 95), (2, 63, 40)], ids=["1x33x33", "3x33x95", "2x63x40"])
def test_forward_split_at_the_smallest_shapes(sid_net, shape):
    """forward_split (pad_mode 1): 33 x 33 is the smallest input the reflect pad admits (31 rows and columns of pad, compute
    64 x 64); 33 x 95 pads one column (64 x 96), 63 x 40 one row and 24 columns (64 x 64).  Level-4 planes 4 x 4 and 4 x 6."""
    net, sd = sid_net
    B, H, W = shape
    inputs, eps, keys = _forward(net, B, H, W, seed=131 + W, pad=True)
    _layers_ok(net, sd, inputs, eps, keys, range(B), True, f"forward_split B = {B}, {H} x {W}")


@pytest.mark.parametrize("shape", [(1, 32, 32), (3, 32, 64), (2, 64, 32)], ids=["1x32x32", "3x32x64", "2x64x32"])
def test_naiveforward_at_the_smallest_shapes(sid_net, shape):
    """naiveforward (pad_mode 0) from 32 x 32: level-4 planes of 2 x 2, 2 x 4 and 4 x 2 (every position a corner or an edge),
    Downsample to 2 x 2, Upsample from it, attention on 16 and 32 tokens (less than one key tile)."""
    net, sd = sid_net
    B, H, W = shape
    inputs, eps, keys = _forward(net, B, H, W, seed=141 + W, pad=False)
    _layers_ok(net, sd, inputs, eps, keys, range(B), False, f"naiveforward B = {B}, {H} x {W}")


def test_forward_split_b64_on_the_smallest_planes(sid_net):
    """B = 64 at 33 x 33 (compute 64 x 64): level-4 planes of 4 x 4 with 64 samples in flight - conv_sk units that hold ten
    samples, per-sample lists filled to their last entry.  Samples 0 and 63 against the emulation.  Level 0 has 16 tiles of
    16 x 16 per sample: by the engine's 4-tiles-per-CU rule the persistent conv_ws (key 23) and akgm_ws (113) engage exactly when
    1024 >= 4 x CUs (they do on the 256 CUs of an MI355X)."""
    net, sd = sid_net
    B = 64
    inputs, eps, keys = _forward(net, B, 33, 33, seed=151, pad=True)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    rule = B * (64 // 16) * (64 // 16) >= 4 * ncu
    print(f"B = 64, 33 x 33 on {ncu} CUs: 4-tiles-per-CU rule {rule}")
    _layers_ok(net, sd, inputs, eps, keys, (0, B - 1), True, "forward_split B = 64, 33 x 33")
    assert (23 in keys) == rule and (113 in keys) == rule, (sorted(keys), ncu)
    assert sum(keys.get(k, 0) for k in C.AKGM_KEYS) == sum(1 for Ld in unet_layers(SID) if Ld.kind == "block"), keys


def test_smallest_graph_replay_is_bit_identical(sid_net):
    """HIP-graph replay at the smallest shape (B = 1, 33 x 33): two replays equal the eager forward bit for bit, in eps and in
    every stored activation; a replay on other contents of the same buffers in between changes all of them."""
    net, _ = sid_net
    dn = net.denoise_fn
    cond, guide, x_t = (torch.from_numpy(a).cuda() for a in synth_inputs(1, 33, 33, seed=161))
    lvl = torch.full((1, 1), 0.23, device="cuda")
    eps = torch.empty_like(x_t)
    names = [(Ld.name, w) for Ld in unet_layers(SID) for w in (("out", "h1") if Ld.kind == "block" else ("out",))]

    def acts():
        a = {k: dn.debug_read(*k).clone() for k in names}
        torch.cuda.synchronize()
        return a
    with torch.no_grad():
        e0 = dn.forward_split(cond, x_t, lvl, guide).clone()
        a0 = acts()
        x0 = x_t.clone()
        dn.set_graph(True)
        try:
            g1 = dn.forward_split(cond, x_t, lvl, guide, out=eps).clone()          # captured + launched
            x_t.mul_(0.5); lvl.fill_(0.71)
            gb = dn.forward_split(cond, x_t, lvl, guide, out=eps).clone()          # replayed on other contents
            ab = acts()
            x_t.copy_(x0); lvl.fill_(0.23)
            g2 = dn.forward_split(cond, x_t, lvl, guide, out=eps).clone()          # replayed on the first contents
            a2 = acts()
        finally:
            dn.set_graph(False)
    diff = [k for k in names if not torch.equal(a0[k], a2[k])]
    same = [k for k in names if torch.equal(a0[k], ab[k])]
    print(f"33 x 33 graph replay: eps equal {torch.equal(e0, g1) and torch.equal(e0, g2)}, {len(names) - len(diff)} of "
          f"{len(names)} activations equal; the replay on other contents changed {len(names) - len(same)} of them")
    assert bool(torch.isfinite(e0).all())
    assert torch.equal(e0, g1) and torch.equal(e0, g2) and not torch.equal(e0, gb)
    assert not same, same
    assert not diff, diff


def test_shapes_below_the_smallest_are_refused(sid_net):
    """forward_split needs 33 rows and columns for its reflect pad; naiveforward needs multiples of 16 (four Downsamples) of at
    least 32, so that the level-4 planes keep 2 x 2 positions (no kernel was written for a plane with a side of 1).  Anything
    else is refused when the forward is planned, before any launch, with a message."""
    net, _ = sid_net
    dn = net.denoise_fn
    for (H, W), pad, msg in (((32, 40), True, "must be >= 33"), ((40, 32), True, "must be >= 33"), ((24, 32), False, "divisible"),
                             ((16, 32), False, "at least 2\\^levels"), ((32, 16), False, "at least 2\\^levels")):
        cond, guide, x_t = (torch.from_numpy(a).cuda() for a in synth_inputs(1, H, W, seed=171))
        lvl = torch.full((1, 1), 0.3, device="cuda")
        for _ in range(2):       # the second call too: a refused shape must not be remembered as the planned one
            with pytest.raises(C.ulib.UcdirError, match=msg):
                if pad:
                    dn.forward_split(cond, x_t, lvl, guide)
                else:
                    dn.naiveforward(torch.cat([cond, x_t], 1), lvl, guide)
    cond, guide, x_t = (torch.from_numpy(a).cuda() for a in synth_inputs(1, 33, 33, seed=172))
    with torch.no_grad():
        e = dn.forward_split(cond, x_t, torch.full((1, 1), 0.3, device="cuda"), guide)
    assert bool(torch.isfinite(e).all())
